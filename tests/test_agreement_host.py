"""Host side of the chain agreement: the header declares
gs_occupancy_agreement, gs_motif_run_batch_agreement (gs_motif_run_batch_summary's parameters
with the six outputs appended) and gs_agreement_last_ms, _native binds them with the declared
argument counts, ChainStats.agreement() equals a literal triple loop over hand-made bins,
rhat() equals the Gelman-Rubin formula, and MotifSampler.runSweepsBatchedAgreement makes one
Context.motif_run_batch_agreement call that asks for no bins.  The context is a stand-in: no
device is touched."""
import math
import re

import numpy as np
import pytest

from gibbssampling_amd import (ChainAgreement, ChainStats, ChainSummary, ListChainStats,
                               MotifSampler, _native, sampler)
from gibbssampling_amd.sampler import createMotifIndex

SOURCES = [b"ACGTACGTACGTACGT"] * 3
W = 5
OFF = np.array([0, 13, 26, 39], np.int64)  # 1 + (16 - 5 + 1) bins a sequence
CELLS = 4 * W + 4
NAMES = ("gs_occupancy_agreement", "gs_motif_run_batch_agreement", "gs_agreement_last_ms")
GROUP = ["int32_t *agree_out", "int64_t *spread_out", "int32_t *spread_chain_out",
         "int32_t *chain_agree_out", "int64_t *chain_dist_out"]


def declaration(name):
    """The parameter list of `name` in include/gibbs_hip.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_the_header_declares_the_entry_points():
    assert set(NAMES) <= set(_native.header_symbols())
    ret, params = declaration("gs_motif_run_batch_agreement")
    # (the summary's own n_pooled_out is already in the list: the agreement's has its name)
    assert ret == "int" and params == (declaration("gs_motif_run_batch_summary")[1] + GROUP +
                                       ["int32_t *agree_n_pooled_out"])
    ret, params = declaration("gs_occupancy_agreement")
    assert ret == "int"
    assert params == ["gs_ctx *ctx", "int32_t W", "const int32_t *occ", "int32_t n_chains",
                      "int64_t n_counted", "const int32_t *pooled"] + GROUP + ["int32_t *n_pooled_out"]
    assert declaration("gs_agreement_last_ms") == ("int", ["const gs_ctx *ctx", "double out[1]"])
    text = re.sub(r" \* ", " ", " ".join(_native.HEADER_PATH.read_text().split()))
    for phrase in ("total variation distance", "the lowest r that has it", "the row is (0, 0, -1)",
                   "a chain that is not pooled gets (-1, -1)", "below 2^62",
                   "nothing is indexed by a bin's value",
                   "no agreement variant of the single-chain or of the list run calls"):
        assert phrase in text, phrase


def test_native_binds_them_with_their_argument_counts():
    class Lib:
        """Records what _declare sets on each entry point."""
        def __getattr__(self, name):
            f = type("F", (), {})()
            object.__setattr__(self, name, f)
            return f

    lib = Lib()
    _native._declare(lib, strict=True)
    for name in NAMES:
        assert len(getattr(lib, name).argtypes) == len(declaration(name)[1]), name
    assert lib.gs_occupancy_agreement.argtypes[4] is _native.C.c_int64          # n_counted
    assert lib.gs_motif_run_batch_agreement.argtypes[7] is _native.C.c_int64    # first_sweep
    for m in ("occupancy_agreement", "motif_run_batch_agreement", "agreement_last_ms"):
        assert callable(getattr(_native.Context, m))


# ---- ChainStats.agreement() against a literal triple loop ----

def triple_loop(occ, off, flags):
    """The issue's quantities, Python ints, no vectorisation."""
    R, N = len(occ), len(off) - 1
    pooled = [r for r in range(R) if flags[r]]
    P = len(pooled)
    agree, spread, spread_chain = [0] * N, [0] * N, [-1] * N
    chain_agree = [0 if flags[r] else -1 for r in range(R)]
    chain_dist = [0 if flags[r] else -1 for r in range(R)]
    for n in range(N):
        bins = range(int(off[n]), int(off[n + 1]))
        pool = {b: 0 for b in bins}
        for r in pooled:
            for b in bins:
                pool[b] += int(occ[r][b])
        mstar, top = None, None
        for b in bins:
            if top is None or pool[b] > top:
                mstar, top = b, pool[b]
        largest = None
        for r in pooled:
            m, top, d = None, None, 0
            for b in bins:
                x = int(occ[r][b])
                if top is None or x > top:
                    m, top = b, x
                d += abs(P * x - pool[b])
            if m == mstar:
                agree[n] += 1
                chain_agree[r] += 1
            chain_dist[r] += d
            if largest is None or d > largest:
                largest, spread_chain[n] = d, r
        spread[n] = 0 if largest is None else largest
    return agree, spread, spread_chain, chain_agree, chain_dist, P


def stats_of(occ, nc):
    occ = np.asarray(occ, np.int32)
    R = len(occ)
    return ChainStats(occ, OFF, np.zeros((R, nc)), np.full(R, -1, np.int64), [[]] * R)


def check(occ, nc, mask=None):
    st = stats_of(occ, nc)
    got = st.agreement(mask)
    flags = st.finished() if mask is None else [m != 0 for m in mask]
    want = triple_loop(np.asarray(occ), OFF, flags)
    assert isinstance(got, ChainAgreement)
    assert (got.agree.tolist(), got.spread.tolist(), got.spread_chain.tolist(),
            got.chain_agree.tolist(), got.chain_dist.tolist(), got.n_pooled) == want
    assert got.agree.dtype == np.int32 and got.spread.dtype == np.int64
    assert got.spread_chain.dtype == np.int32 and got.chain_agree.dtype == np.int32
    assert got.chain_dist.dtype == np.int64 and got.n_counted == nc
    return got


def finished_bins(R, nc, seed):
    """R chains whose every row sums to nc, the counts spread over a few bins."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((R, OFF[-1]), np.int32)
    for r in range(R):
        for n in range(3):
            for b in rng.integers(OFF[n], OFF[n + 1], nc):
                occ[r, b] += 1
    return occ


def test_identical_chains():
    occ = np.repeat(finished_bins(1, 9, 1), 4, axis=0)
    a = check(occ, 9)
    assert a.n_pooled == 4 and a.agree.tolist() == [4] * 3 and a.spread.tolist() == [0] * 3
    assert a.spread_chain.tolist() == [0] * 3  # the lowest chain among equals
    assert a.chain_dist.tolist() == [0] * 4 and a.chain_agree.tolist() == [3] * 4
    assert a.distance().tolist() == [0.0] * 3 and len(a.outliers(0.0)) == 0


def test_one_outlier_chain():
    nc = 8
    occ = np.zeros((4, OFF[-1]), np.int32)
    occ[:, OFF[:-1] + 1 + 3] = nc        # everybody at start 3 ...
    occ[2] = 0
    occ[2, OFF[:-1] + 1 + 9] = nc        # ... but chain 2 at start 9
    a = check(occ, nc)
    assert a.n_pooled == 4 and a.agree.tolist() == [3] * 3
    assert a.spread_chain.tolist() == [2] * 3
    # chain 2: |4 * 8 - 8| at its bin and |0 - 24| at the others' = 48; the others 8 + 8
    assert a.spread.tolist() == [48] * 3 and a.chain_dist.tolist() == [48, 48, 144, 48]
    assert a.chain_agree.tolist() == [3, 3, 0, 3]
    assert a.distance().tolist() == [48 / (2 * 4 * nc)] * 3       # = 0.75
    assert a.outliers(0.5).tolist() == [2] and a.outliers(0.2).tolist() == [0, 1, 2, 3]


def test_an_unfinished_chain_in_the_middle():
    occ = finished_bins(3, 7, 2)
    b = OFF[0] + int(np.argmax(occ[1, OFF[0]:OFF[1]]))
    occ[1, b] -= 1                       # sequence 0 of chain 1 sums to 6
    a = check(occ, 7)
    assert a.n_pooled == 2 and a.chain_dist[1] == -1 and a.chain_agree[1] == -1
    assert 1 not in a.spread_chain.tolist()
    assert (a.chain_dist[[0, 2]] >= 0).all()
    # two chains: each is as far from the pool as the other, the lower one is reported
    assert a.spread_chain.tolist() == [0] * 3 and a.chain_dist[0] == a.chain_dist[2]


def test_an_explicit_mask():
    occ = finished_bins(4, 5, 3)
    occ[3, OFF[0]] += 1                  # not finished by the rule, pooled by the mask
    a = check(occ, 5, mask=[1, 0, 0, 7])
    assert a.n_pooled == 2 and a.chain_dist[[1, 2]].tolist() == [-1, -1]
    b = check(occ, 5)
    assert b.n_pooled == 3 and b.chain_dist[3] == -1
    # list chains: finished() is their own, and it is the default mask
    sites = np.full((4, 3, 3), 0, np.int32)
    sites[:, :, 1] = 5
    sites[2, 1, 1] = 4
    lst = ListChainStats(occ, OFF, np.zeros((4, 5)), np.full(4, -1, np.int64), [[]] * 4, sites, W)
    c = lst.agreement()
    assert c.n_pooled == 3 and c.chain_dist[2] == -1
    want = triple_loop(occ, OFF, [True, True, False, True])
    assert (c.agree.tolist(), c.spread.tolist(), c.spread_chain.tolist(), c.chain_agree.tolist(),
            c.chain_dist.tolist(), c.n_pooled) == want


def test_no_pooled_chain_and_a_single_one():
    occ = finished_bins(3, 6, 4)
    a = check(occ, 7)                    # rows sum to 6: nobody pooled
    assert a.n_pooled == 0
    assert (a.agree.tolist(), a.spread.tolist(), a.spread_chain.tolist()) == ([0] * 3, [0] * 3,
                                                                              [-1] * 3)
    assert a.chain_dist.tolist() == [-1] * 3 and a.chain_agree.tolist() == [-1] * 3
    assert a.distance().tolist() == [0.0] * 3 and len(a.outliers(0.0)) == 0
    one = check(occ, 6, mask=[0, 1, 0])  # P = 1: the chain is its own pool
    assert one.n_pooled == 1 and one.agree.tolist() == [1] * 3 and one.spread.tolist() == [0] * 3
    assert one.spread_chain.tolist() == [1] * 3 and one.chain_dist.tolist() == [-1, 0, -1]
    assert one.chain_agree.tolist() == [-1, 3, -1]
    # first-maximum ties: a chain tied at two bins agrees only where the pool's first one is
    tie = np.zeros((2, OFF[-1]), np.int32)
    tie[0, [OFF[0] + 2, OFF[0] + 5]] = 3
    tie[1, [OFF[0] + 5, OFF[0] + 7]] = 3
    tie[:, OFF[1:-1]] = 6
    t = check(tie, 6)
    assert t.agree[0] == 1               # the pool's maximum is bin 5, the chains' 2 and 5 ...
    tie[0, OFF[0] + 2], tie[0, OFF[0] + 6] = 0, 3
    assert check(tie, 6).agree[0] == 2   # ... and now everybody's first maximum is bin 5


# ---- rhat ----

def test_rhat_is_the_formula():
    rng = np.random.default_rng(5)
    ic = rng.normal(size=(4, 11)) + np.arange(4)[:, None]
    occ = np.zeros((4, OFF[-1]), np.int32)
    occ[:, OFF[0] + 1] = 11
    occ[2, OFF[0] + 1] = 10              # chain 2 did not finish: left out
    st = ChainStats(occ, OFF, ic, np.full(4, -1, np.int64), [[]] * 4)
    rows = [[float(x) for x in ic[r]] for r in (0, 1, 3)]
    m, n = 3, 11
    means = [math.fsum(r) / n for r in rows]
    grand = math.fsum(means) / m
    b_over_n = math.fsum((x - grand) ** 2 for x in means) / (m - 1)
    wv = math.fsum(math.fsum((x - mu) ** 2 for x in r) / (n - 1) for r, mu in zip(rows, means)) / m
    want = math.sqrt(((n - 1) / n * wv + b_over_n) / wv)
    assert st.rhat() == pytest.approx(want, rel=1e-12)
    assert st.rhat() > 1.0
    # the summary carries the trace: over every chain without an agreement, over the pooled
    # ones with it
    args = (np.zeros((4, 3), np.int32), np.zeros((4, 3), np.int32), np.zeros((4, CELLS), np.int64),
            np.zeros(3, np.int32), np.zeros(3, np.int64), np.zeros(CELLS, np.int64), 3, 11, ic,
            np.full(4, -1, np.int64), [[]] * 4, W, 4)
    s = ChainSummary(*args)
    assert s.agreement is None
    assert s.rhat() == pytest.approx(ChainStats(np.zeros((4, 0), np.int32), np.zeros(1, np.int64),
                                                ic, None, None).rhat(), rel=1e-12)
    s = ChainSummary(*args, agreement=st.agreement())
    assert s.rhat() == pytest.approx(want, rel=1e-12)


def test_rhat_nan_cases():
    occ = np.zeros((3, OFF[-1]), np.int32)
    occ[:, OFF[0] + 1] = 4

    def rhat(ic, o=occ):
        ic = np.asarray(ic, np.float64)
        return ChainStats(o[:len(ic)], OFF, ic, None, None).rhat()

    good = [[1.0, 2.0, 4.0, 3.0], [2.0, 2.5, 1.0, 0.0], [0.0, 1.0, 5.0, 2.0]]
    assert math.isfinite(rhat(good))
    assert math.isnan(rhat(good[:1]))                                   # m < 2
    short = occ.copy()
    short[1:, OFF[0] + 1] = 3
    assert math.isnan(rhat(good, short))                                # one finished chain
    one = np.zeros((3, OFF[-1]), np.int32)
    one[:, OFF[0] + 1] = 1
    assert math.isnan(rhat([[1.0], [2.0], [3.0]], one))                 # n < 2
    assert math.isnan(rhat([[1.0] * 4, [2.0] * 4, [3.0] * 4]))          # Wv == 0
    bad = [row[:] for row in good]
    bad[1][2] = float("nan")
    assert math.isnan(rhat(bad))                                        # a NaN in a trace
    # ... but not in the trace of a chain that did not finish
    short = occ.copy()
    short[1, OFF[0] + 1] = 2
    assert math.isfinite(rhat(bad, short))


# ---- runSweepsBatchedAgreement ----

class FakeCtx:
    """motif_run_batch_agreement over a table."""

    def __init__(self):
        self.calls = []

    def motif_run_batch_agreement(self, W, pc, cutoff, n_sweeps, seeds, pos=None, init_mode=0,
                                  first_sweep=0, u=None, burn_in=0, thin=1, occupancy=False,
                                  **kw):
        self.calls.append((W, pc, cutoff, n_sweeps, list(seeds), pos, init_mode, first_sweep, u,
                           burn_in, thin, occupancy, kw))
        n, R = len(SOURCES), len(seeds)
        nc = len(range(burn_in, n_sweeps, thin))
        stats = {"ic": np.arange(R * nc, dtype=np.float64).reshape(R, nc),
                 "best_sweep": np.full(R, first_sweep + burn_in, np.int64),
                 "best_pos": np.full((R, n), -1, np.int32), "best_pwms": np.full((R, n), 2.5),
                 "mode_pos": np.tile(np.arange(n, dtype=np.int32), (R, 1)),
                 "mode_count": np.full((R, n), nc, np.int32),
                 "counts": np.full((R, CELLS), nc, np.int64),
                 "pooled_pos": np.arange(n, dtype=np.int32),
                 "pooled_count": np.full(n, R * nc, np.int64),
                 "pooled_counts": np.full(CELLS, R * nc, np.int64),
                 "n_pooled": np.array([R], np.int32),
                 "agree": np.full(n, R, np.int32), "spread": np.arange(n, dtype=np.int64),
                 "spread_chain": np.zeros(n, np.int32), "chain_agree": np.full(R, n, np.int32),
                 "chain_dist": np.arange(R, dtype=np.int64) * 4 * R * nc * n,
                 "agree_n_pooled": np.array([R], np.int32), "n_counted": nc}
        return (np.tile(np.arange(n, dtype=np.int32), (R, 1)), np.tile(np.arange(n) / 4.0, (R, 1)),
                np.zeros(R, np.int32), stats)


def test_one_call_and_no_bins(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    chains, s = MotifSampler.runSweepsBatchedAgreement(W, 1e-4, 1.0, "ACGT", SOURCES, 20,
                                                       [2**64 + 11, 12], burn_in=5, thin=3,
                                                       first_sweep=40)
    assert len(ctx.calls) == 1
    call = ctx.calls[0]
    assert call[:5] == (W, 1e-4, 1.0, 20, [11, 12]) and call[6:11] == (0, 40, None, 5, 3)
    assert call[11] is False and not call[12].get("occupancy", False)   # no bins asked for
    assert chains == [[createMotifIndex(n / 4.0, [n]) for n in range(3)]] * 2
    assert isinstance(s, ChainSummary) and s.occupancy is None and s.offsets is None
    a = s.agreement
    assert isinstance(a, ChainAgreement) and a.n_pooled == 2 and a.n_counted == 5
    assert a.agree.tolist() == [2] * 3 and a.spread.tolist() == [0, 1, 2]
    assert a.distance().tolist() == [0.0, 1 / 20, 2 / 20]
    # mean distances 0 and 4 R nc N / (2 R nc N) = 2
    assert a.outliers(1.0).tolist() == [1]
    assert s.n_pooled == 2 and s.mode() == [createMotifIndex(1.0, [n]) for n in range(3)]
    assert math.isfinite(s.rhat())


def test_the_existing_methods_leave_the_field_unset(monkeypatch):
    class Ctx(FakeCtx):
        def motif_run_batch_summary(self, *a, **k):
            out = self.motif_run_batch_agreement(*a, **k)
            for key in ("agree", "spread", "spread_chain", "chain_agree", "chain_dist",
                        "agree_n_pooled"):
                del out[3][key]
            return out

    ctx = Ctx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    _, s = MotifSampler.runSweepsBatchedSummary(W, 1e-4, 1.0, "ACGT", SOURCES, 6, [1, 2])
    assert s.agreement is None

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    with pytest.raises(_native.ArgumentError):
        MotifSampler.runSweepsBatchedAgreement(W, 1e-4, 1.0, "ACGT", SOURCES, 6, [1, 2],
                                               motifAmount=2)
