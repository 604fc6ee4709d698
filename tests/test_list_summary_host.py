"""Host side of the list chain summaries: the header declares gs_list_occupancy_summary and
gs_motif_run_multi_batch_summary (the run call: its stats sibling's parameters with the
summary's appended), _native binds them with the declared argument counts, ListChainSummary
reads hand-made arrays as ListChainStats reads the same chains' bins and site counts, and
MotifSampler.runSweepsBatchedListSummary makes one Context.motif_run_multi_batch_summary call
that asks for no bins.  The context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import ListChainStats, ListChainSummary, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex
from test_summary_host import declaration

SOURCES = [b"ACGTACGTACGTACGTACGT"] * 3
W, M = 3, 2
OFF = np.array([0, 19, 38, 57], np.int64)  # 1 + (20 - 3 + 1) bins a sequence
CELLS = 4 * W + 4

MODES = ["int32_t *mode_sites_out", "int32_t *mode_sites_count_out", "int32_t *mode_cnt_out",
         "int32_t *mode_pos_out", "int32_t *mode_count_out", "int64_t *counts_out"]
POOLED = ["int32_t *pool_mode_sites_out", "int64_t *pool_mode_sites_count_out",
          "int32_t *pool_mode_cnt_out", "int32_t *pool_mode_pos_out",
          "int64_t *pool_mode_count_out", "int64_t *pool_counts_out", "int32_t *n_pooled_out"]
NAMES = ("gs_list_occupancy_summary", "gs_motif_run_multi_batch_summary")


def test_the_header_declares_the_entry_points():
    assert set(NAMES) <= set(_native.header_symbols())
    ret, params = declaration("gs_motif_run_multi_batch_summary")
    assert ret == "int"
    assert params == declaration("gs_motif_run_multi_batch_stats")[1] + MODES + POOLED
    ret, params = declaration("gs_list_occupancy_summary")
    assert ret == "int"
    assert params == ["gs_ctx *ctx", "int32_t W", "int32_t motif_amount", "const int32_t *occ",
                      "const int32_t *sites", "int32_t n_chains", "int64_t n_counted"] + \
        MODES + POOLED
    text = " ".join(_native.HEADER_PATH.read_text().replace(" * ", " ").split())
    for phrase in ("the smallest c in 0 .. M whose site count is the row's largest",
                   "excluded when |k - q| <= W", "a zero bin is a candidate like any other",
                   "every sequence's site counts sum to n_counted",
                   "downloaded only when occ_out / sites_out are non-null",
                   "Negative bins or site counts are the caller's error"):
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
    assert lib.gs_list_occupancy_summary.argtypes[6] is _native.C.c_int64         # n_counted
    assert lib.gs_motif_run_multi_batch_summary.argtypes[8] is _native.C.c_int64  # first_sweep
    assert len(_native.Context._LIST_SUMMARY_KEYS) == len(MODES + POOLED)
    for m in ("list_occupancy_summary", "motif_run_multi_batch_summary"):
        assert callable(getattr(_native.Context, m))


def reduce_lists(occ, sites, off, n_counted, width):
    """The pooled arrays of hand-made bins and site counts, by numpy (the per-chain ones and
    the cells left empty)."""
    occ, sites = np.asarray(occ, np.int64), np.asarray(sites, np.int64)
    N, amount = len(off) - 1, sites.shape[2] - 1
    keep = (sites.sum(axis=2) == n_counted).all(axis=1)
    bins, cnts = occ[keep].sum(axis=0), sites[keep].sum(axis=0)
    ps, pc = np.zeros(N, np.int32), np.zeros(N, np.int32)
    psc = np.zeros(N, np.int64)
    pp, pk = np.full((N, amount), -1, np.int32), np.zeros((N, amount), np.int64)
    for n in range(N):
        row = bins[off[n] + 1:off[n + 1]]
        ps[n] = int(np.argmax(cnts[n]))
        psc[n] = cnts[n, ps[n]]
        taken = []
        for _ in range(ps[n]):
            free = [k for k in range(len(row)) if all(abs(k - q) > width for q in taken)]
            if not free:
                break
            taken.append(max(free, key=lambda k: (row[k], -k)))
        pc[n] = len(taken)
        pp[n, :pc[n]] = sorted(taken)
        pk[n, :pc[n]] = row[sorted(taken)]
    return ps, psc, pc, pp, pk, int(keep.sum())


def summary_of(occ, sites, n_counted, cells=None, pooled_cells=None):
    R, N = len(occ), len(OFF) - 1
    ps, psc, pc, pp, pk, n_pooled = reduce_lists(occ, sites, OFF, n_counted, W)
    zeros = np.zeros((R, N), np.int32)
    return ListChainSummary(zeros, zeros, zeros, np.full((R, N, M), -1, np.int32),
                            np.zeros((R, N, M), np.int32),
                            np.zeros((R, CELLS), np.int64) if cells is None else cells,
                            ps, psc, pc, pp, pk,
                            np.zeros(CELLS, np.int64) if pooled_cells is None else pooled_cells,
                            n_pooled, n_counted, np.zeros((R, n_counted)),
                            np.full(R, -1, np.int64), [[]] * R, W, 4)


def stats_of(occ, sites, n_counted):
    R = len(occ)
    return ListChainStats(occ, OFF, np.zeros((R, n_counted)), np.full(R, -1, np.int64), [[]] * R,
                          sites, W)


def test_mode_is_list_chain_stats_mode_of_the_same_slabs():
    nc = 6
    occ = np.zeros((3, 57), np.int32)
    sites = np.zeros((3, 3, M + 1), np.int32)
    for r in range(3):
        sites[r, 0] = (0, 0, nc)                         # sequence 0: two sites ...
        occ[r, OFF[0] + 1 + 2] = nc                      # ... start 2 always,
        occ[r, OFF[0] + 1 + 2 + W] = nc - 1              # the runner-up exactly W away: excluded,
        occ[r, OFF[0] + 1 + 10], occ[r, OFF[0] + 1 + 14] = 2, 2  # a tie: the first wins
        sites[r, 1] = (0, 3, 3)                          # sequence 1: one and two sites tie
        occ[r, OFF[1] + 1 + 7] = 5
        sites[r, 2] = (1, 1, 4)                          # sequence 2: two sites, two starts that fit
        occ[r, OFF[2] + 1 + 0], occ[r, OFF[2] + 1 + 1] = 4, 3
    sites[1, 2] = (1, 1, 3)                              # chain 1 did not finish its last sequence
    s, st = summary_of(occ, sites, nc), stats_of(occ, sites, nc)
    assert s.n_pooled == 2 and st.finished().tolist() == [True, False, True]
    assert s.mode() == st.mode()
    assert s.mode() == [createMotifIndex(1.0, [2, 10]), createMotifIndex(0.5, [7]),
                        createMotifIndex(8 / 12, [0, 4])]
    assert s.pooled_count[2].tolist() == [8, 0]          # a zero-count pick


def test_a_short_list_no_pooled_chain_and_no_counted_state():
    nc = 5
    occ = np.zeros((2, 57), np.int32)
    sites = np.zeros((2, 3, M + 1), np.int32)
    sites[:, :, 2] = nc
    occ[:, OFF[:-1] + 1 + 9] = nc
    s, st = summary_of(occ, sites, nc), stats_of(occ, sites, nc)
    assert s.mode() == st.mode() and s.n_pooled == 2
    # the starts 0 .. 17 are 18: with W = 3 two fit around start 9; with 16 only one does
    assert [m.Positions for m in s.mode()] == [(0, 9)] * 3
    wide = ListChainSummary(**{**s.__dict__, "motifLength": 16})
    short = reduce_lists(occ, sites, OFF, nc, 16)
    assert short[2].tolist() == [1, 1, 1] and short[3][:, 1].tolist() == [-1] * 3
    wide.pooled_cnt, wide.pooled_pos, wide.pooled_count = short[2], short[3], short[4]
    theirs = ListChainStats(occ, OFF, np.zeros((2, nc)), np.full(2, -1, np.int64), [[]] * 2,
                            sites, 16)
    assert wide.mode() == theirs.mode() == [createMotifIndex(1.0, [9])] * 3
    none = summary_of(occ, sites, nc + 2)  # every site row sums to 5: nobody pooled
    assert none.n_pooled == 0 and none.mode() == [createMotifIndex(0.0, [])] * 3
    assert none.mode() == stats_of(occ, sites, nc + 2).mode()
    zero = np.zeros_like(occ), np.zeros_like(sites)
    empty = summary_of(*zero, 0)  # nothing counted: everybody pooled
    assert empty.n_pooled == 2 and empty.mode() == [createMotifIndex(0.0, [])] * 3
    assert empty.mode() == stats_of(*zero, 0).mode()


def test_count_matrix_shapes():
    cells = np.arange(2 * CELLS, dtype=np.int64).reshape(2, CELLS)
    pooled = np.arange(CELLS, dtype=np.int64) * 3
    s = summary_of(np.zeros((2, 57), np.int32), np.zeros((2, 3, M + 1), np.int32), 0, cells,
                   pooled)
    C, T = s.countMatrix()
    assert C.shape == (4, W) and T.shape == (4,)
    assert C[2, 1] == 3 * (2 * W + 1) and T.tolist() == [36, 39, 42, 45]
    C, T = s.countMatrix(pool=False)
    assert C.shape == (2, 4, W) and T.shape == (2, 4)
    assert C[1, 2, 1] == CELLS + 2 * W + 1 and T[1].tolist() == [28, 29, 30, 31]


class FakeCtx:
    """motif_run_multi_batch_summary over a table: every chain ends with the list [n] in
    sequence n, PWMS n / 4, and was there in every counted sweep."""

    def __init__(self):
        self.calls = []

    def motif_run_multi_batch_summary(self, motif_amount, W, pc, cutoff, n_sweeps, seeds, cnt, pos,
                                      init_mode, first_sweep, cap, burn_in=0, thin=1,
                                      occupancy=False, sites=False):
        self.calls.append((motif_amount, W, pc, cutoff, n_sweeps, list(seeds),
                           None if cnt is None else np.array(cnt).tolist(), init_mode,
                           first_sweep, cap, burn_in, thin, occupancy, sites))
        R, n, nc = len(seeds), len(SOURCES), len(range(burn_in, n_sweeps, thin))
        lists = np.full((R, n, cap), -1, np.int32)
        lists[:, :, 0] = np.arange(n)
        stats = {"ic": np.tile(np.arange(nc, dtype=np.float64), (R, 1)),
                 "best_sweep": np.full(R, first_sweep + burn_in if nc else -1, np.int64),
                 "best_cnt": np.ones((R, n), np.int32), "best_pos": lists,
                 "best_pwms": np.full((R, n), 2.5),
                 "mode_sites": np.ones((R, n), np.int32),
                 "mode_sites_count": np.full((R, n), nc, np.int32),
                 "mode_cnt": np.ones((R, n), np.int32), "mode_pos": lists,
                 "mode_count": np.full((R, n, cap), nc, np.int32),
                 "counts": np.full((R, CELLS), nc, np.int64),
                 "pooled_sites": np.full(n, 1 if nc else 0, np.int32),
                 "pooled_sites_count": np.full(n, R * nc, np.int64),
                 "pooled_cnt": np.full(n, 1 if nc else 0, np.int32), "pooled_pos": lists[0],
                 "pooled_count": np.full((n, cap), R * nc, np.int64),
                 "pooled_counts": np.full(CELLS, R * nc, np.int64),
                 "n_pooled": np.array([R], np.int32), "n_counted": nc}
        if occupancy:
            stats["occupancy"] = np.zeros((R, OFF[-1]), np.int32)
            stats["offsets"] = OFF.copy()
        if sites:
            stats["sites"] = np.zeros((R, n, motif_amount + 1), np.int32)
        return (np.ones((R, n), np.int32), lists, np.tile(np.arange(n) / 4.0, (R, 1)),
                np.zeros(R, np.int32), stats)


def test_one_call_and_no_bins_by_default(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    chains, s = MotifSampler.runSweepsBatchedListSummary(
        W, 1e-4, 1.0, "ACGT", SOURCES, 20, [2**64 + 11, 12], first_sweep=40, burn_in=5, thin=3,
        motifAmount=M)
    assert ctx.calls == [(M, W, 1e-4, 1.0, 20, [11, 12], None, 0, 40, M, 5, 3, False, False)]
    assert chains == [[createMotifIndex(n / 4.0, [n]) for n in range(3)]] * 2
    assert isinstance(s, ListChainSummary)
    assert s.occupancy is None and s.offsets is None and s.sites is None
    assert s.mode_pos.shape == (2, 3, M) and s.counts.shape == (2, CELLS)
    assert s.n_pooled == 2 and s.n_counted == 5 and s.pooled_sites_count.dtype == np.int64
    assert s.motifLength == W and s.alphabetSize == 4
    assert s.best_sweep.tolist() == [45, 45] and s.best == [[createMotifIndex(2.5, [n])
                                                             for n in range(3)]] * 2
    assert s.mode() == [createMotifIndex(1.0, [n]) for n in range(3)]
    C, T = s.countMatrix()
    assert C.shape == (4, W) and (C == 10).all() and T.tolist() == [10] * 4
    # the bins and the site counts on request, starts as lists
    mems = [[createMotifIndex(0.0, [1, 9]), createMotifIndex(0.0, []), createMotifIndex(0.0, [4])]]
    _, s = MotifSampler.runSweepsBatchedListSummary(W, 1e-4, 1.0, "ACGT", SOURCES, 4, [3], mems,
                                                    motifAmount=M, occupancy=True)
    assert len(ctx.calls) == 2 and ctx.calls[-1][-2:] == (True, True)
    assert ctx.calls[-1][6] == [[2, 0, 1]]
    assert s.occupancy.shape == (1, 57) and np.array_equal(s.offsets, OFF)
    assert s.sites.shape == (1, 3, M + 1)
    # nothing counted
    _, s = MotifSampler.runSweepsBatchedListSummary(W, 1e-4, 1.0, "ACGT", SOURCES, 7, [3],
                                                    burn_in=7, motifAmount=M)
    assert s.n_counted == 0 and s.mode() == [createMotifIndex(0.0, [])] * 3 and s.best == [[]]

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    with pytest.raises(_native.ArgumentError):  # one motifMem for two seeds
        MotifSampler.runSweepsBatchedListSummary(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], mems,
                                                 motifAmount=M)
    with pytest.raises(_native.ArgumentError):  # a motifMem shorter than the sources
        MotifSampler.runSweepsBatchedListSummary(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1],
                                                 [mems[0][:2]], motifAmount=M)
