"""Host side of the chain summaries: the header declares gs_occupancy_summary,
gs_run_sweeps_summary, gs_motif_run_summary, gs_motif_run_batch_summary and gs_summary_last_ms
(the run calls: their stats siblings' parameters with the summary's appended), _native binds
them with the declared argument counts, ChainSummary reads hand-made arrays as ChainStats reads
the same chains' bins, and MotifSampler.runSweepsSummary makes one Context.motif_run_summary
call that asks for no bins.  The context is a stand-in: no device is touched."""
import re

import numpy as np
import pytest

from gibbssampling_amd import ChainStats, ChainSummary, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex

SOURCES = [b"ACGTACGTACGTACGT"] * 3
W = 5
OFF = np.array([0, 13, 26, 39], np.int64)  # 1 + (16 - 5 + 1) bins a sequence
CELLS = 4 * W + 4

MODES = ["int32_t *mode_pos_out", "int32_t *mode_count_out", "int64_t *counts_out"]
POOLED = ["int32_t *pool_mode_pos_out", "int64_t *pool_mode_count_out",
          "int64_t *pool_counts_out", "int32_t *n_pooled_out"]
NAMES = ("gs_occupancy_summary", "gs_run_sweeps_summary", "gs_motif_run_summary",
         "gs_motif_run_batch_summary", "gs_summary_last_ms")


def declaration(name):
    """The parameter list of `name` in include/gibbs_hip.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_the_header_declares_the_entry_points():
    assert set(NAMES) <= set(_native.header_symbols())
    # the run calls: the stats siblings' parameters, the new ones at the end
    for name, sibling, extra in (("gs_run_sweeps_summary", "gs_run_sweeps_stats", MODES),
                                 ("gs_motif_run_summary", "gs_motif_run_stats", MODES),
                                 ("gs_motif_run_batch_summary", "gs_motif_run_batch_stats",
                                  MODES + POOLED)):
        ret, params = declaration(name)
        assert ret == "int" and params == declaration(sibling)[1] + extra, name
    ret, params = declaration("gs_occupancy_summary")
    assert ret == "int"
    assert params == ["gs_ctx *ctx", "int32_t W", "const int32_t *occ", "int32_t n_chains",
                      "int64_t n_counted"] + MODES + POOLED
    assert declaration("gs_summary_last_ms") == ("int", ["const gs_ctx *ctx", "double out[1]"])
    text = re.sub(r" \* ", " ", " ".join(_native.HEADER_PATH.read_text().split()))
    for phrase in ("the first maximum", "a row of zeros gives (-1, 0)",
                   "exactly the sum of gs_counts over the counted states",
                   "downloaded only when occ_out is non-null",
                   "Negative bins are the caller's error"):
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
    assert lib.gs_occupancy_summary.argtypes[4] is _native.C.c_int64      # n_counted
    assert lib.gs_run_sweeps_summary.argtypes[4] is _native.C.c_uint64    # the seed
    assert lib.gs_motif_run_summary.argtypes[5] is _native.C.c_uint64
    for m in ("occupancy_summary", "run_sweeps_summary", "motif_run_summary",
              "motif_run_batch_summary", "summary_last_ms"):
        assert callable(getattr(_native.Context, m))


def reduce_bins(occ, off, n_counted):
    """The summary's arrays of hand-made bins, by numpy (cells left zero)."""
    occ = np.asarray(occ, np.int32)
    R, N = len(occ), len(off) - 1
    keep = occ[:, off[0]:off[1]].sum(axis=1) == n_counted
    total = occ[keep].astype(np.int64).sum(axis=0)
    mp, mc = np.zeros((R, N), np.int32), np.zeros((R, N), np.int32)
    pp, pc = np.zeros(N, np.int32), np.zeros(N, np.int64)
    for n in range(N):
        for r in range(R):
            row = occ[r, off[n]:off[n + 1]]
            mp[r, n], mc[r, n] = np.argmax(row) - 1, row.max()
        row = total[off[n]:off[n + 1]]
        pp[n], pc[n] = np.argmax(row) - 1, row.max()
    return mp, mc, pp, pc, int(keep.sum())


def summary_of(occ, n_counted, cells=None, pooled_cells=None):
    mp, mc, pp, pc, n_pooled = reduce_bins(occ, OFF, n_counted)
    R = len(occ)
    return ChainSummary(mp, mc, np.zeros((R, CELLS), np.int64) if cells is None else cells, pp, pc,
                        np.zeros(CELLS, np.int64) if pooled_cells is None else pooled_cells,
                        n_pooled, n_counted, np.zeros((R, n_counted)), np.full(R, -1, np.int64),
                        [[]] * R, W, 4)


def test_mode_is_chain_stats_mode_of_the_same_bins():
    nc = 6
    occ = np.zeros((3, 39), np.int32)
    for r in range(3):
        occ[r, OFF[0] + 1 + 2] = nc                      # sequence 0: always start 2
        occ[r, OFF[1]], occ[r, OFF[1] + 4] = 3, 3        # sequence 1: [] and start 3 tie
        occ[r, OFF[2] + 1 + r] = 2                       # sequence 2: pooled tie of 0, 1, 2 ...
        occ[r, OFF[2] + 12] = nc - 2                     # ... below start 11
    occ[1, OFF[0] + 3] -= 1                              # chain 1 did not finish
    s = summary_of(occ, nc)
    st = ChainStats(occ, OFF, np.zeros((3, nc)), np.full(3, -1, np.int64), [[]] * 3)
    assert s.n_pooled == 2 and st.finished().tolist() == [True, False, True]
    assert s.mode() == st.mode()
    assert s.mode() == [createMotifIndex(1.0, [2]), createMotifIndex(0.5, []),
                        createMotifIndex(4 / 6, [11])]
    # a first-maximum tie inside one chain, and chain 1's own row still there
    assert s.mode_pos[:, 1].tolist() == [-1, -1, -1] and s.mode_count[1, 0] == nc - 1


def test_no_pooled_chain_and_no_counted_state():
    occ = np.zeros((2, 39), np.int32)
    occ[:, OFF[:-1] + 4] = 5
    none = summary_of(occ, 7)  # sequence 0 sums to 5: nobody pooled
    assert none.n_pooled == 0
    assert none.mode() == [createMotifIndex(0.0, [])] * 3
    st = ChainStats(occ, OFF, np.zeros((2, 7)), np.full(2, -1, np.int64), [[]] * 2)
    assert none.mode() == st.mode()
    empty = summary_of(np.zeros((2, 39), np.int32), 0)  # nothing counted: everybody pooled
    assert empty.n_pooled == 2 and empty.mode() == [createMotifIndex(0.0, [])] * 3
    st = ChainStats(np.zeros((2, 39), np.int32), OFF, np.zeros((2, 0)), np.full(2, -1, np.int64),
                    [[]] * 2)
    assert empty.mode() == st.mode()


def test_count_matrix_shapes():
    cells = np.arange(2 * CELLS, dtype=np.int64).reshape(2, CELLS)
    pooled = np.arange(CELLS, dtype=np.int64) * 3
    s = summary_of(np.zeros((2, 39), np.int32), 0, cells, pooled)
    C, T = s.countMatrix()
    assert C.shape == (4, W) and T.shape == (4,)
    assert C[2, 3] == 3 * (2 * W + 3) and T.tolist() == [60, 63, 66, 69]
    C, T = s.countMatrix(pool=False)
    assert C.shape == (2, 4, W) and T.shape == (2, 4)
    assert C[1, 2, 3] == CELLS + 2 * W + 3 and T[1].tolist() == [44, 45, 46, 47]


class FakeCtx:
    """motif_run_summary over a table: sequence n ends at start n with PWMS n / 4, and was
    there in every counted sweep."""

    def __init__(self):
        self.calls = []

    def motif_run_summary(self, W, pc, cutoff, n_sweeps, seed, pos, first_sweep=0, u=None,
                          burn_in=0, thin=1, occupancy=False):
        self.calls.append((W, pc, cutoff, n_sweeps, seed, np.array(pos).tolist(), first_sweep, u,
                           burn_in, thin, occupancy))
        n = len(SOURCES)
        nc = len(range(burn_in, n_sweeps, thin))
        stats = {"ic": np.arange(nc, dtype=np.float64),
                 "best_sweep": np.array([first_sweep + burn_in if nc else -1], np.int64),
                 "best_pos": np.full(n, -1, np.int32), "best_pwms": np.full(n, 2.5),
                 "mode_pos": np.arange(n, dtype=np.int32) if nc else np.full(n, -1, np.int32),
                 "mode_count": np.full(n, nc, np.int32),
                 "counts": np.full(CELLS, nc, np.int64), "status": 0}
        if occupancy:
            stats["occupancy"] = np.zeros(OFF[-1], np.int32)
            stats["offsets"] = OFF.copy()
        return np.arange(n, dtype=np.int32), np.arange(n) / 4.0, stats


def test_one_call_and_no_bins_by_default(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    mem = [createMotifIndex(0.5, [3]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])]
    chain, s = MotifSampler.runSweepsSummary(W, 1e-4, 1.0, "ACGT", SOURCES, mem, 20, 5, 3,
                                             seed=2**64 + 11, first_sweep=40)
    assert ctx.calls == [(W, 1e-4, 1.0, 20, 11, [3, -1, 7], 40, None, 5, 3, False)]
    assert chain == [createMotifIndex(n / 4.0, [n]) for n in range(3)]
    assert isinstance(s, ChainSummary) and s.occupancy is None and s.offsets is None
    assert s.mode_pos.shape == (1, 3) and s.counts.shape == (1, CELLS)
    assert s.n_pooled == 1 and s.n_counted == 5 and s.pooled_count.dtype == np.int64
    assert s.motifLength == W and s.alphabetSize == 4
    assert s.best_sweep.tolist() == [45] and s.best == [[createMotifIndex(2.5, [])] * 3]
    assert s.mode() == [createMotifIndex(1.0, [n]) for n in range(3)]
    C, T = s.countMatrix()
    assert C.shape == (4, W) and (C == 5).all() and T.tolist() == [5] * 4
    # the bins on request
    _, s = MotifSampler.runSweepsSummary(W, 1e-4, 1.0, "ACGT", SOURCES, mem, 4, occupancy=True)
    assert ctx.calls[-1][-1] is True and len(ctx.calls) == 2
    assert s.occupancy.shape == (1, 39) and np.array_equal(s.offsets, OFF)
    # nothing counted
    _, s = MotifSampler.runSweepsSummary(W, 1e-4, 1.0, "ACGT", SOURCES, mem, 7, 7)
    assert s.n_counted == 0 and s.mode() == [createMotifIndex(0.0, [])] * 3 and s.best == [[]]

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    with pytest.raises(_native.ArgumentError):  # a list of two positions
        MotifSampler.runSweepsSummary(W, 1e-4, 1.0, "ACGT", SOURCES,
                                      [createMotifIndex(0.0, [1, 9])] + mem[1:], 3)
    with pytest.raises(_native.ArgumentError):  # motifMem shorter than the sources
        MotifSampler.runSweepsSummary(W, 1e-4, 1.0, "ACGT", SOURCES, mem[:2], 3)
