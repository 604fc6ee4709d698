"""GPU parity of the chain agreement: gs_occupancy_agreement on hand-made bins
against ChainStats.agreement() (the numpy restatement, itself checked against a literal triple
loop in test_agreement_host.py), the planted edges by name, and gs_motif_run_batch_agreement
against gs_motif_run_batch_summary (bit for bit) and against the agreement of the bins that
gs_motif_run_batch_stats returns.  Everything is integers or bits: every comparison is exact."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset
from gibbssampling_amd import ChainStats, Context, MotifSampler, _native
from test_gpu_run_stats import CASES, CUTOFF, PC, T, bits, counted_sweeps, dataset
from test_gpu_summary import random_bins

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# bins a row: the lane (64), chunk (256) and stage (512) boundaries; two bins is L = W; 513 and
# 600 are summed again a chunk instead of staged
BINS = (2, 3, 63, 64, 65, 128, 129, 200, 256, 257, 512, 513, 600)
BIG = 2**31 - 1
KEYS = ("agree", "spread", "spread_chain", "chain_agree", "chain_dist", "n_pooled")
RUN_KEYS = ("agree", "spread", "spread_chain", "chain_agree", "chain_dist", "agree_n_pooled")


def ragged(N, W, alpha, seed, bins=BINS):
    """N sequences whose rows have `bins` bins in turn."""
    rng = np.random.default_rng(seed)
    lens = np.array([bins[n % len(bins)] + W - 2 for n in range(N)], np.int64)
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    a = np.frombuffer(alpha, np.uint8)
    return a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8), offsets


def restate(occ, off, n_counted, mask=None):
    """ChainStats.agreement() of the bins -> the dict of Context.occupancy_agreement.  The
    pool is finished()'s unless a mask is given (or n_counted is too large for a trace)."""
    occ = np.asarray(occ, np.int32)
    R = len(occ)
    small = n_counted < 10_000
    if mask is None and not small:
        mask = occ[:, off[0]:off[1]].astype(np.int64).sum(axis=1) == n_counted
    st = ChainStats(occ, off, np.zeros((R, n_counted if small else 0)), np.full(R, -1, np.int64),
                    [[]] * R)
    a = st.agreement(mask)
    return {"agree": a.agree, "spread": a.spread, "spread_chain": a.spread_chain,
            "chain_agree": a.chain_agree, "chain_dist": a.chain_dist,
            "n_pooled": np.array([a.n_pooled], np.int32)}


def same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def agreement_twice(ctx, W, occ, n_counted, pooled=None):
    """Every call twice: integer adds, so the outputs are bit-equal."""
    a = ctx.occupancy_agreement(W, occ, n_counted, pooled)
    b = ctx.occupancy_agreement(W, occ, n_counted, pooled)
    assert set(a) == set(b) == set(KEYS)
    same(a, b)
    return a


# ---- hand-made bins ----

N_RAGGED, W_DNA, NC = 2 * len(BINS) + 1, 12, 37


@pytest.fixture(scope="module")
def dna_rows():
    codes, offsets = ragged(N_RAGGED, W_DNA, DNA, seed=3)
    codes.setflags(write=False)
    offsets.setflags(write=False)
    return codes, offsets


@pytest.mark.parametrize("R", [1, 2, 3, 5, 64])
def test_hand_made_bins(gpu_ctx, dna_rows, R):
    codes, offsets = dna_rows
    gpu_ctx.set_sequences(codes, offsets, DNA)
    off = gpu_ctx.occupancy_offsets(W_DNA)
    assert sorted(set(np.diff(off).tolist())) == sorted(BINS)
    occ = random_bins(off, R, NC, seed=100 + R)
    got = agreement_twice(gpu_ctx, W_DNA, occ, NC)
    same(got, restate(occ, off, NC))
    assert got["n_pooled"][0] == R and gpu_ctx.agreement_last_ms() > 0.0
    assert (got["agree"] >= (1 if R == 1 else 0)).all() and (got["chain_dist"] >= 0).all()
    if R == 1:  # the chain is its own pool
        assert not got["spread"].any() and got["chain_agree"][0] == N_RAGGED
    else:
        assert got["spread"].any() and (got["agree"] < R).any()
    # one chain left out by the rule, in the middle; and put back by the mask
    if R >= 3:
        short = occ.copy()
        short[R // 2, off[0] + int(np.argmax(short[R // 2, off[0]:off[1]]))] -= 1
        got = agreement_twice(gpu_ctx, W_DNA, short, NC)
        same(got, restate(short, off, NC))
        assert got["n_pooled"][0] == R - 1 and got["chain_dist"][R // 2] == -1
        got = agreement_twice(gpu_ctx, W_DNA, short, NC, np.ones(R, np.int32))
        same(got, restate(short, off, NC, np.ones(R, bool)))
        assert got["n_pooled"][0] == R and got["chain_dist"][R // 2] >= 0


def rows_with(off, nb):
    """The sequences (never sequence 0) whose rows have nb bins."""
    return [n for n in np.nonzero(np.diff(off) == nb)[0].tolist() if n > 0]


def test_planted_edges(gpu_ctx, dna_rows):
    codes, offsets = dna_rows
    ctx = gpu_ctx
    ctx.set_sequences(codes, offsets, DNA)
    off = ctx.occupancy_offsets(W_DNA)
    nc, R = 10, 3
    base = random_bins(off, R, nc, seed=7)

    def put(occ, n, rows):
        """Row n of chain r becomes rows[r]: {bin: count}."""
        for r, row in enumerate(rows):
            occ[r, off[n]:off[n + 1]] = 0
            for b, c in row.items():
                occ[r, off[n] + b] = c

    occ = base.copy()
    # two chains with the same largest D: chain 0 sits half on each of their bins, so
    # D = (0, 30, 30) and the lower of the two is reported; once in a staged row and once in
    # a row that is summed again (600 bins, the bins in different chunks)
    tied = {}
    for nb, (b1, b2) in ((129, (5, 128)), (600, (70, 599))):
        n = rows_with(off, nb)[0]
        put(occ, n, [{b1: 5, b2: 5}, {b1: nc}, {b2: nc}])
        tied[n] = (b1, b2)
    # a chain tied at two bins on its mode count, the pool as well: the first maximum.  Chains
    # 0 and 1: 5 at bins 64 and 200; chain 2: 5 at bins 3 and 200, so the pool has 15 at bin
    # 200 and everybody's mode is ... bin 64, 64, 3, pool 200: nobody agrees; then the
    # mirrored row, where the pool ties at bins 3 and 200 and its first maximum is bin 3
    n_tie = rows_with(off, 257)[0]
    put(occ, n_tie, [{64: 5, 200: 5}, {64: 5, 200: 5}, {3: 5, 200: 5}])
    n_tie2 = rows_with(off, 256)[0]
    put(occ, n_tie2, [{3: 5, 200: 5}, {3: 5, 200: 5}, {3: 5, 200: 5}])
    # an all-zero row (never sequence 0: the rule reads it)
    n_zero = rows_with(off, 65)[0]
    put(occ, n_zero, [{}, {}, {}])
    got = agreement_twice(ctx, W_DNA, occ, nc)
    same(got, restate(occ, off, nc))
    assert got["n_pooled"][0] == 3
    for n in tied:  # (the pool ties on the two bins: its first maximum is chains 0 and 1's)
        assert got["spread"][n] == 30 and got["spread_chain"][n] == 1 and got["agree"][n] == 2
    assert got["agree"][n_tie] == 0
    assert got["agree"][n_tie2] == 3 and got["spread"][n_tie2] == 0
    assert got["agree"][n_zero] == 3 and got["spread"][n_zero] == 0
    assert got["spread_chain"][n_zero] == 0 and got["spread_chain"][n_tie2] == 0

    # a chain whose sequence-0 row sums to n_counted - 1: not pooled, (-1, -1), absent from
    # the pool: the others read as if it were not there
    short = occ.copy()
    short[1, off[0] + int(np.argmax(short[1, off[0]:off[1]]))] -= 1
    got = agreement_twice(ctx, W_DNA, short, nc)
    same(got, restate(short, off, nc))
    assert got["n_pooled"][0] == 2
    assert got["chain_dist"][1] == -1 and got["chain_agree"][1] == -1
    assert 1 not in got["spread_chain"].tolist()
    without = agreement_twice(ctx, W_DNA, short[[0, 2]], nc)
    same(got, without, ("agree", "spread"))
    assert np.array_equal(got["chain_dist"][[0, 2]], without["chain_dist"])
    assert np.array_equal(got["chain_agree"][[0, 2]], without["chain_agree"])
    # ... and pooled through an explicit mask
    got = agreement_twice(ctx, W_DNA, short, nc, np.array([1, 5, -1], np.int32))
    same(got, restate(short, off, nc, np.ones(3, bool)))
    assert got["n_pooled"][0] == 3 and got["chain_dist"][1] >= 0
    for n in tied:
        assert got["spread"][n] == 30 and got["spread_chain"][n] == 1
    got = agreement_twice(ctx, W_DNA, short, nc, np.array([0, 1, 0], np.int32))
    same(got, restate(short, off, nc, np.array([False, True, False])))
    assert got["n_pooled"][0] == 1 and not got["spread"].any() and (got["agree"] == 1).all()
    assert (got["spread_chain"] == 1).all() and got["chain_dist"].tolist() == [-1, 0, -1]

    # no pooled chain: (0, 0, -1) rows, (-1, -1) chains, n_pooled 0
    for mask in (None, np.zeros(3, np.int32)):
        got = agreement_twice(ctx, W_DNA, occ, nc + 1 if mask is None else nc, mask)
        assert got["n_pooled"][0] == 0
        assert not got["agree"].any() and not got["spread"].any()
        assert (got["spread_chain"] == -1).all()
        assert (got["chain_dist"] == -1).all() and (got["chain_agree"] == -1).all()
    same(got, restate(occ, off, nc, np.zeros(3, bool)))

    # bins of 2^31 - 1 with three chains: the products and sums are int64
    big = np.zeros((3, int(off[-1])), np.int32)
    wide = np.nonzero(np.diff(off) >= 3)[0]   # (sequence 0 has two bins)
    for r in range(3):
        big[r, off[:-1]] = BIG                # sequence 0 sums to BIG: the rule pools it
        big[r, off[wide] + 1 + (r % 2)] = BIG  # chains 0 and 2 against chain 1
    got = agreement_twice(ctx, W_DNA, big, BIG)
    same(got, restate(big, off, BIG))
    assert got["n_pooled"][0] == 3
    # chain 1: |3 BIG - BIG| at its bin and |0 - 2 BIG| at the others'
    assert (got["spread"][wide] == 4 * BIG).all() and (got["spread_chain"][wide] == 1).all()
    assert got["chain_dist"].tolist() == [2 * BIG * len(wide), 4 * BIG * len(wide),
                                          2 * BIG * len(wide)]
    assert got["chain_dist"][1] > 2**33 and (got["agree"] == 3).all()

    # no chains: nothing to do
    got = ctx.occupancy_agreement(W_DNA, np.zeros((0, int(off[-1])), np.int32), 3)
    assert got["chain_dist"].shape == (0,) and got["n_pooled"][0] == 0
    assert not got["agree"].any() and (got["spread_chain"] == -1).all()


def test_protein_alphabet_changes_only_the_offsets(gpu_ctx):
    W = 20
    codes, offsets = ragged(9, W, PROTEIN, seed=11, bins=(2, 65, 257, 513, 64))
    gpu_ctx.set_sequences(codes, offsets, PROTEIN)
    off = gpu_ctx.occupancy_offsets(W)
    assert np.array_equal(np.diff(off), np.diff(offsets) - W + 2)
    occ = random_bins(off, 5, NC, seed=12)
    same(agreement_twice(gpu_ctx, W, occ, NC), restate(occ, off, NC))


# ---- the run call ----

B_SEEDS = [1001, 77, 5_000_000_007, 77, 12]  # rows 1 and 3: the same seed


@pytest.mark.parametrize("name", ["dna", "protein"])
def test_run_batch_agreement(gpu_ctx, name):
    spec = CASES[name]
    W, alpha, (burn_in, thin) = spec["W"], spec["alpha"], spec["count"]
    codes, offsets, _ = dataset(spec["N"], *spec["L"], W, alpha, seed=17)
    ctx = gpu_ctx
    ctx.set_sequences(codes, offsets, alpha)
    kw = dict(init_mode=1, burn_in=burn_in, thin=thin)
    nc = len(counted_sweeps(T, burn_in, thin))
    R = len(B_SEEDS)
    pos, pw, status, st = ctx.motif_run_batch_stats(W, PC, CUTOFF, T, B_SEEDS, **kw)
    spos, spw, sstatus, s = ctx.motif_run_batch_summary(W, PC, CUTOFF, T, B_SEEDS, occupancy=True,
                                                        **kw)
    apos, apw, astatus, a = ctx.motif_run_batch_agreement(W, PC, CUTOFF, T, B_SEEDS,
                                                          occupancy=True, **kw)
    assert ctx.agreement_last_ms() > 0.0 and ctx.summary_last_ms() > 0.0
    assert not status.any() and not sstatus.any() and not astatus.any()
    # every output of the summary call, bit for bit
    assert np.array_equal(apos, spos) and np.array_equal(bits(apw), bits(spw))
    assert np.array_equal(apos, pos) and np.array_equal(bits(apw), bits(pw))
    assert set(a) == set(s) | set(RUN_KEYS)
    for k in s:
        if k == "n_counted":
            assert a[k] == s[k] == nc
        elif s[k].dtype == np.float64:
            assert np.array_equal(bits(a[k]), bits(s[k])), k
        else:
            assert a[k].dtype == s[k].dtype and np.array_equal(a[k], s[k]), k
    # the agreement of the bins the stats call returns
    want = restate(st["occupancy"], st["offsets"], nc)
    got = dict(a, n_pooled=a["agree_n_pooled"])
    same(got, want)
    assert a["agree_n_pooled"][0] == a["n_pooled"][0] == R
    # the same seed, the same chain
    assert a["chain_dist"][1] == a["chain_dist"][3] and a["chain_agree"][1] == a["chain_agree"][3]
    # from the summary's own arrays
    assert np.array_equal(a["agree"], (a["mode_pos"] == a["pooled_pos"][None, :]).sum(axis=0))
    assert np.array_equal(a["chain_agree"], (a["mode_pos"] == a["pooled_pos"][None, :]).sum(axis=1))
    # without the bins, and without the summary's pooled outputs (the pool is then the
    # agreement's own decision)
    for extra in ({}, {"pool": False}, {"modes": False, "counts": False, "pool": False,
                                        "ic": False, "best": False}):
        _, _, _, lean = ctx.motif_run_batch_agreement(W, PC, CUTOFF, T, B_SEEDS, **kw, **extra)
        assert "occupancy" not in lean
        same(dict(lean, n_pooled=lean["agree_n_pooled"]), want)
    # the six outputs null: the summary call
    npos, npw, nstatus, none = ctx.motif_run_batch_agreement(W, PC, CUTOFF, T, B_SEEDS,
                                                             occupancy=True, agreement=False, **kw)
    assert set(none) == set(s) and not nstatus.any()
    assert np.array_equal(npos, spos) and np.array_equal(bits(npw), bits(spw))
    for k in s:
        if k != "n_counted":
            assert np.array_equal(none[k].view(np.uint8), s[k].view(np.uint8)), k
    # the sampler's entry point
    if name == "dna":
        sources = [codes[offsets[n]:offsets[n + 1]].tobytes() for n in range(spec["N"])]
        chains, summary = MotifSampler.runSweepsBatchedAgreement(W, PC, CUTOFF, alpha, sources, T,
                                                                 B_SEEDS, init_mode=1,
                                                                 burn_in=burn_in, thin=thin)
        ag = summary.agreement
        assert summary.occupancy is None and ag.n_pooled == R and ag.n_counted == nc
        for k in KEYS[:5]:
            assert np.array_equal(getattr(ag, k), want[k]), k
        assert np.array_equal(ag.distance(), want["spread"] / (2.0 * R * nc))
        assert (ag.distance() <= 1.0).all()


def test_a_raising_chain_is_left_out(gpu_ctx):
    """The recipe of test_gpu_summary.py: chain 1 raises in sweep 1."""
    R, n, N, W = 3, 4, 30, 6
    codes, offsets = make_dataset(N, 40, W, seed=51)
    p0 = init_positions(offsets, W, 52)
    u = np.random.default_rng(53).random((R, n, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    starts = np.tile(p0, (R, 1))
    _, _, status, a = gpu_ctx.motif_run_batch_agreement(W, PC, CUTOFF, n, [1, 2, 3], pos=starts,
                                                        u=u, occupancy=True)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    assert a["agree_n_pooled"][0] == a["n_pooled"][0] == 2
    assert a["chain_dist"][1] == -1 and a["chain_agree"][1] == -1
    assert 1 not in a["spread_chain"].tolist()
    same(dict(a, n_pooled=a["agree_n_pooled"]), restate(a["occupancy"], a["offsets"], n))
    # the others are as without it
    _, _, sto, b = gpu_ctx.motif_run_batch_agreement(W, PC, CUTOFF, n, [1, 3], pos=starts[[0, 2]],
                                                     u=u[[0, 2]])
    assert not sto.any() and b["agree_n_pooled"][0] == 2
    same(a, b, ("agree", "spread"))
    assert np.array_equal(a["chain_dist"][[0, 2]], b["chain_dist"])
    assert np.array_equal(a["spread_chain"], np.array([0, 2], np.int32)[b["spread_chain"]])


# ---- refusals ----

def test_refusals(gpu_ctx):
    N, L, W, R = 12, 30, 8, 2
    codes, offsets = make_dataset(N, L, W, seed=5)
    ctx = gpu_ctx
    ctx.set_sequences(codes, offsets, DNA)
    off = ctx.occupancy_offsets(W)
    occ = random_bins(off, R, 10, seed=4)
    P = _native._ptr
    lib = ctx.lib
    out = {"ag": np.full(N, 7, np.int32), "sp": np.full(N, 7, np.int64),
           "sc": np.full(N, 7, np.int32), "ca": np.full(R, 7, np.int32),
           "cd": np.full(R, 7, np.int64), "np_": np.full(1, 7, np.int32)}

    def call(W_=W, occ_=occ, R_=R, nc=10, c=ctx, **over):
        o = dict(out, **over)
        return lib.gs_occupancy_agreement(c.h, W_, P(occ_), R_, nc, None, P(o["ag"]), P(o["sp"]),
                                          P(o["sc"]), P(o["ca"]), P(o["cd"]), P(o["np_"]))

    p0 = init_positions(offsets, W, 9, 0.2)
    ctx.set_positions(W, p0)
    ctx.synchronize()
    before, state = ctx.stats(), ctx.get_state()
    assert call(R_=0) == _native.GS_OK and call(R_=0, occ_=None) == _native.GS_OK
    # GS_E_ARG: a bad W, no bins, negative counts, half of the group
    for kw in ({"W_": 0}, {"W_": 65}, {"W_": L + 1}, {"occ_": None}, {"R_": -1}, {"nc": -1},
               *({k: None} for k in out), {"ag": None, "sp": None, "sc": None}):
        assert call(**kw) == _native.GS_E_ARG, kw
    for a in out.values():
        assert (a == 7).all()
    # half of the group on the run call
    seeds = np.array([1, 2], np.uint64)
    rows_i, rows_d, stw = np.tile(p0, (R, 1)), np.zeros((R, N)), np.zeros(R, np.int32)
    for k in out:
        o = dict(out, **{k: None})
        rc = lib.gs_motif_run_batch_agreement(
            ctx.h, W, PC, CUTOFF, 3, P(seeds), R, 0, -1, None, 0, 1, P(rows_i), P(rows_d), P(stw),
            None, None, None, None, None, None, None, None, None, None, None, None,
            P(o["ag"]), P(o["sp"]), P(o["sc"]), P(o["ca"]), P(o["cd"]), P(o["np_"]))
        assert rc == _native.GS_E_ARG, k
    # nothing ran, and gs_occupancy_agreement leaves the snapshot alone
    assert ctx.stats() == before
    assert call() == _native.GS_OK
    assert ctx.stats() == before
    got = ctx.get_state()
    assert np.array_equal(got[0], state[0]) and np.array_equal(bits(got[1]), bits(state[1]))
    want = restate(occ, off, 10)
    for k, key in zip(out, KEYS):
        assert np.array_equal(out[k], want[key]), key
    fresh = Context(0)
    try:
        assert call(c=fresh) == _native.GS_E_STATE  # no sequences
        fresh.set_sequences(codes, offsets, DNA)
        assert call(c=fresh) == _native.GS_OK       # ... but no snapshot is needed
        fresh.set_sequences(codes, offsets, DNA, n_global=N + 5)
        assert call(c=fresh) == _native.GS_E_UNSUPPORTED  # sharded sequences
    finally:
        fresh.close()
