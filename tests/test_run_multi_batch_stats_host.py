"""Host side of the list chains' statistics: the header declares
gs_motif_run_multi_batch_stats with the plain call's leading parameters and _native binds it;
MotifSampler.runSweepsBatchedListStats makes one Context.motif_run_multi_batch_stats call and
wraps what comes back in a ListChainStats, whose finished / marginals / siteCounts / mode pool
the finished chains and take first maxima.  The context is a stand-in: no device is touched."""
import re
from pathlib import Path

import numpy as np
import pytest

from gibbssampling_amd import ArgumentError, ListChainStats, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex

ROOT = Path(__file__).resolve().parent.parent
SOURCES = [b"ACGTACGTACGTACGT"] * 3
W = 5
OFF = np.array([0, 13, 26, 39], np.int64)  # 1 + (16 - 5 + 1) bins a sequence


def declaration(name):
    """The parameter list of `int name(...)` in the public header, comments removed."""
    text = re.sub(r"/\*.*?\*/", " ", (ROOT / "include" / "gibbs_hip.h").read_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_header_declares_the_plain_calls_leading_parameters():
    plain = declaration("gs_motif_run_multi_batch")
    stats = declaration("gs_motif_run_multi_batch_stats")
    lead = plain[:plain.index("const double *u") + 1]
    assert len(lead) == 12 and stats[:12] == lead
    assert stats[12:14] == ["int32_t burn_in", "int32_t thin"]
    assert stats[14:18] == plain[12:]
    assert stats[18:] == ["int32_t *occ_out", "int32_t *sites_out", "double *ic_out",
                          "int64_t *best_sweep_out", "int32_t *best_cnt_out",
                          "int32_t *best_pos_out", "double *best_pwms_out"]
    header = (ROOT / "include" / "gibbs_hip.h").read_text()
    assert "s[0] == occ[off[n]]" in header  # the identities of sites_out are stated


def test_native_binds_the_declared_argument_count():
    class Fn:
        restype = argtypes = None

    class Lib:
        def __getattr__(self, name):
            fn = Fn()
            setattr(self, name, fn)
            return fn

    lib = Lib()
    _native._declare(lib)
    fn = lib.__dict__["gs_motif_run_multi_batch_stats"]
    assert len(fn.argtypes) == len(declaration("gs_motif_run_multi_batch_stats")) == 25
    plain = lib.__dict__["gs_motif_run_multi_batch"].argtypes
    assert list(fn.argtypes[:12]) == list(plain[:12])
    assert list(fn.argtypes[14:18]) == list(plain[12:])


class FakeCtx:
    """motif_run_multi_batch_stats over a table: chain r ends with sequence n holding the
    list [n, n + 7] (r even) or [] (r odd), PWMS (r + n) / 4; its best state is all-[] with
    PWMS r."""

    def __init__(self, status=None):
        self.status = status
        self.calls = []

    def motif_run_multi_batch_stats(self, motif_amount, W, pc, cutoff, n_sweeps, seeds, cnt=None,
                                    pos=None, init_mode=0, first_sweep=0, cap=None, u=None,
                                    burn_in=0, thin=1):
        self.calls.append((motif_amount, W, pc, cutoff, n_sweeps, list(seeds),
                           None if cnt is None else np.array(cnt).tolist(),
                           None if pos is None else np.array(pos).tolist(), init_mode,
                           first_sweep, cap, u, burn_in, thin))
        R, n, M = len(seeds), len(SOURCES), motif_amount
        cnt_out = np.where(np.arange(R)[:, None] % 2 == 0, 2, 0) * np.ones((R, n), np.int32)
        pos_out = np.full((R, n, cap), -1, np.int32)
        for r in range(0, R, 2):
            for i in range(n):
                pos_out[r, i, :2] = [i, i + 7]
        pwms = (np.arange(R)[:, None] + np.arange(n)[None, :]) / 4.0
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        nc = len(range(burn_in, n_sweeps, thin))
        occ = np.zeros((R, OFF[-1]), np.int32)
        occ[:, OFF[:-1]] = nc
        sites = np.zeros((R, n, M + 1), np.int32)
        sites[:, :, 0] = nc
        stats = {"occupancy": occ, "offsets": OFF.copy(), "sites": sites,
                 "ic": np.arange(R * nc, dtype=np.float64).reshape(R, nc),
                 "best_sweep": np.array([first_sweep + burn_in if nc else -1] * R, np.int64),
                 "best_cnt": np.zeros((R, n), np.int32),
                 "best_pos": np.full((R, n, cap), -1, np.int32),
                 "best_pwms": np.tile(np.arange(R, dtype=np.float64)[:, None], (1, n))}
        return cnt_out.astype(np.int32), pos_out, pwms, status, stats


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


def test_one_call_with_the_seeds_masked_to_64_bits(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    mems = [[createMotifIndex(0.5, [3, 11]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])],
            [createMotifIndex(0.0, []), createMotifIndex(2.0, [1]), createMotifIndex(0.0, [])]]
    chains, st = MotifSampler.runSweepsBatchedListStats(W, 1e-4, 1.0, "ACGT", SOURCES, 20,
                                                        [10, 2**64 + 11], mems, first_sweep=40,
                                                        burn_in=5, thin=3, motifAmount=2)
    assert ctx.calls == [(2, W, 1e-4, 1.0, 20, [10, 11], [[2, 0, 1], [0, 1, 0]],
                          [[[3, 11], [-1, -1], [7, -1]], [[-1, -1], [1, -1], [-1, -1]]], 0, 40, 2,
                          None, 5, 3)]
    assert chains == [[createMotifIndex(0.0, [0, 7]), createMotifIndex(0.25, [1, 8]),
                       createMotifIndex(0.5, [2, 9])],
                      [createMotifIndex(0.25, []), createMotifIndex(0.5, []),
                       createMotifIndex(0.75, [])]]
    assert isinstance(st, ListChainStats) and st.motifLength == W
    assert st.occupancy.shape == (2, 39) and np.array_equal(st.offsets, OFF)
    assert st.sites.shape == (2, 3, 3) and st.ic.shape == (2, 5)
    assert st.best_sweep.tolist() == [45, 45]
    assert st.best == [[createMotifIndex(0.0, [])] * 3, [createMotifIndex(1.0, [])] * 3]
    assert st.finished().tolist() == [True, True]
    assert st.mode() == [createMotifIndex(1.0, [])] * 3


def test_without_starts_the_init_mode_goes_through(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    chains, st = MotifSampler.runSweepsBatchedListStats(W, 1e-4, 1.0, "ACGT", SOURCES, 7,
                                                        [1, 2, 3], init_mode=1, burn_in=7,
                                                        motifAmount=3)
    assert ctx.calls == [(3, W, 1e-4, 1.0, 7, [1, 2, 3], None, None, 1, 0, 3, None, 7, 1)]
    assert len(chains) == 3 and st.ic.shape == (3, 0)
    assert st.best == [[], [], []] and st.best_sweep.tolist() == [-1, -1, -1]


def test_bad_chains_touch_no_device_and_the_old_method_keeps_refusing(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    full = [createMotifIndex(0.0, [1])] * len(SOURCES)
    with pytest.raises(ArgumentError):  # one chain's motifMem shorter than the sources
        MotifSampler.runSweepsBatchedListStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2],
                                               [full, full[:2]], motifAmount=2)
    with pytest.raises(ArgumentError):  # fewer motifMems than seeds
        MotifSampler.runSweepsBatchedListStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [full],
                                               motifAmount=2)
    with pytest.raises(ArgumentError):
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], motifAmount=2)


def test_a_set_status_raises_the_mapped_exception(monkeypatch):
    bind(monkeypatch, FakeCtx([0, _native.GS_E_ROULETTE_OVERRUN, 0]))
    with pytest.raises(_native.GibbsError) as e:
        MotifSampler.runSweepsBatchedListStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3],
                                               motifAmount=2)
    assert e.value.status == _native.GS_E_ROULETTE_OVERRUN


def hand_made():
    """Motif length 1, motifAmount 2, two sequences of 7 bins (starts 0 .. 5), three chains of
    4 counted sweeps; chain 2 raised after one of them and is left out of the pool.

    Sequence 0, pooled over chains 0 and 1: site counts [2, 3, 3] for 0 / 1 / 2 sites, a tie
    of one and two sites that the first maximum (one site) wins; starts 1 and 4 tie at 3, the
    first wins.  Sequence 1: site counts [0, 1, 7], two sites; its starts by frequency are 2
    (7), 3 (5), 0 (3): start 3 is no more than W from start 2 and is skipped, start 0 is the second."""
    off = np.array([0, 7, 14], np.int64)
    #               [] 0  1  2  3  4  5 | [] 0  1  2  3  4  5
    occ = np.array([[1, 0, 2, 0, 0, 1, 1, 0, 1, 0, 4, 3, 0, 0],
                    [1, 0, 1, 1, 0, 2, 1, 0, 2, 0, 3, 2, 0, 0],
                    [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0]], np.int32)
    sites = np.array([[[1, 2, 1], [0, 0, 4]],
                      [[1, 1, 2], [0, 1, 3]],
                      [[0, 1, 0], [0, 1, 0]]], np.int32)
    ic = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0], [1.0, np.nan, np.nan, np.nan]])
    return ListChainStats(occ, off, ic, np.array([3, 3, 0]), [[], [], []], sites, 1)


def test_finished_marginals_and_site_counts_pool_the_finished_chains():
    st = hand_made()
    # the identities of a finished chain hold in the table
    for r in (0, 1):
        for n in (0, 1):
            row = st.occupancy[r, st.offsets[n]:st.offsets[n + 1]]
            assert st.sites[r, n].sum() == 4 and st.sites[r, n, 0] == row[0]
            assert st.sites[r, n] @ np.arange(3) == row[1:].sum()
    assert st.finished().tolist() == [True, True, False]
    m = st.marginals()
    assert m[0].tolist() == [2 / 8, 0.0, 3 / 8, 1 / 8, 0.0, 3 / 8, 2 / 8]
    assert m[1].tolist() == [0.0, 3 / 8, 0.0, 7 / 8, 5 / 8, 0.0, 0.0]
    # bins 1.. sum to the mean number of sites
    assert m[0][1:].sum() == 9 / 8 and m[1][1:].sum() == 15 / 8
    s = st.siteCounts()
    assert [a.tolist() for a in s] == [[2 / 8, 3 / 8, 3 / 8], [0.0, 1 / 8, 7 / 8]]
    per = st.marginals(pool=False)
    assert per[0][0].tolist() == [0.25, 0.0, 0.5, 0.0, 0.0, 0.25, 0.25]
    assert per[0][2].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # over its one counted sweep
    assert per[1][1].tolist() == [0.0, 0.5, 0.0, 0.75, 0.5, 0.0, 0.0]
    per_s = st.siteCounts(pool=False)
    assert per_s[0].tolist() == [[0.25, 0.5, 0.25], [0.25, 0.25, 0.5], [0.0, 1.0, 0.0]]
    assert per_s[1].tolist() == [[0.0, 0.0, 1.0], [0.0, 0.25, 0.75], [0.0, 1.0, 0.0]]


def test_mode_takes_first_maxima_and_skips_a_start_too_close():
    assert hand_made().mode() == [createMotifIndex(3 / 8, [1]), createMotifIndex(7 / 8, [0, 2])]
    none = ListChainStats(np.zeros((1, 14), np.int32), np.array([0, 7, 14]), np.zeros((1, 0)),
                          np.array([-1]), [[]], np.zeros((1, 2, 3), np.int32), 2)
    assert [a.tolist() for a in none.marginals()] == [[0.0] * 7] * 2
    assert [a.tolist() for a in none.siteCounts()] == [[0.0] * 3] * 2
    assert none.mode() == [createMotifIndex(0.0, [])] * 2
