"""Host side of the single chain's statistics: the header declares gs_run_sweeps_stats,
gs_motif_run_stats and gs_run_stats_last_ms and _native binds them with their argument
counts; MotifSampler.runSweepsStats makes one Context.motif_run_stats call with the arguments
passed through and wraps what comes back in a ChainStats of one chain.  The context is a
stand-in: no device is touched."""
import re

import numpy as np
import pytest

from gibbssampling_amd import ArgumentError, ChainStats, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex

SOURCES = [b"ACGTACGTACGTACGT"] * 3
W = 5
OFF = np.array([0, 13, 26, 39], np.int64)  # 1 + (16 - 5 + 1) bins a sequence


def declaration(name):
    """The parameter list of `name` in include/gibbs_hip.h, comments removed."""
    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_the_header_declares_the_entry_points():
    assert {"gs_run_sweeps_stats", "gs_motif_run_stats", "gs_run_stats_last_ms",
            "gs_state_motif_length"} <= set(_native.header_symbols())
    ret, params = declaration("gs_run_sweeps_stats")
    assert ret == "int"
    assert params == ["gs_ctx *ctx", "double pseudo_count", "double cut_off", "int32_t n_sweeps",
                      "uint64_t seed", "int64_t first_sweep", "const double *u", "int32_t burn_in",
                      "int32_t thin", "int32_t *occ_out", "double *ic_out",
                      "int64_t *best_sweep_out", "int32_t *best_pos_out", "double *best_pwms_out"]
    ret, params = declaration("gs_motif_run_stats")
    assert ret == "int" and len(params) == 17
    assert params[:2] == ["gs_ctx *ctx", "int32_t W"] and params[10:12] == ["int32_t *pos_inout",
                                                                           "double *pwms_out"]
    assert declaration("gs_run_stats_last_ms") == ("int", ["const gs_ctx *ctx", "double out[2]"])
    # the semantics are stated where the caller reads them
    text = " ".join(_native.HEADER_PATH.read_text().split())
    for phrase in ("t >= burn_in and (t - burn_in) % thin == 0", "written, not accumulated",
                   "a NaN never replaces", "quiet NaN", "A fixed PCV is allowed"):
        assert phrase in re.sub(r" \* ", " ", text), phrase


def test_native_binds_them_with_their_argument_counts():
    class Lib:
        """Records what _declare sets on each entry point."""
        def __getattr__(self, name):
            f = type("F", (), {})()
            object.__setattr__(self, name, f)
            return f

    lib = Lib()
    _native._declare(lib, strict=True)
    for name in ("gs_run_sweeps_stats", "gs_motif_run_stats", "gs_run_stats_last_ms"):
        assert len(getattr(lib, name).argtypes) == len(declaration(name)[1]), name
    assert lib.gs_run_sweeps_stats.argtypes[4] is _native.C.c_uint64   # the seed
    assert lib.gs_run_sweeps_stats.argtypes[5] is _native.C.c_int64    # first_sweep
    assert lib.gs_motif_run_stats.argtypes[5] is _native.C.c_uint64
    for m in ("run_sweeps_stats", "motif_run_stats", "run_stats_last_ms"):
        assert callable(getattr(_native.Context, m))


class FakeCtx:
    """motif_run_stats over a table: the chain ends with sequence n at n (at [] where n is
    odd), PWMS n / 4; its histogram puts every counted sweep of sequence n at start n, but
    sequence 1 at [] for all but one of them."""

    def __init__(self):
        self.calls = []

    def motif_run_stats(self, W, pc, cutoff, n_sweeps, seed, pos, first_sweep=0, u=None,
                        burn_in=0, thin=1):
        self.calls.append((W, pc, cutoff, n_sweeps, seed, np.array(pos).tolist(), first_sweep, u,
                           burn_in, thin))
        n = len(SOURCES)
        out = np.arange(n, dtype=np.int32)
        pwms = out / 4.0
        out[out % 2 == 1] = -1
        nc = len(range(burn_in, n_sweeps, thin))
        occ = np.zeros(OFF[-1], np.int32)
        for i in range(n):
            occ[OFF[i] + 1 + i] = nc
        if nc:
            occ[OFF[1] + 2] = 1
            occ[OFF[1]] = nc - 1
        stats = {"occupancy": occ, "offsets": OFF.copy(), "ic": np.arange(nc, dtype=np.float64),
                 "best_sweep": np.array([first_sweep + burn_in if nc else -1], np.int64),
                 "best_pos": np.full(n, -1, np.int32), "best_pwms": np.full(n, 2.5), "status": 0}
        return out, pwms, stats


def test_one_call_with_the_arguments_passed_through(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    mem = [createMotifIndex(0.5, [3]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])]
    chain, st = MotifSampler.runSweepsStats(W, 1e-4, 1.0, "ACGT", SOURCES, mem, 20, 5, 3,
                                            seed=2**64 + 11, first_sweep=40)
    assert ctx.calls == [(W, 1e-4, 1.0, 20, 11, [3, -1, 7], 40, None, 5, 3)]
    assert chain == [createMotifIndex(0.0, [0]), createMotifIndex(0.25, []),
                     createMotifIndex(0.5, [2])]
    assert isinstance(st, ChainStats)
    assert st.occupancy.shape == (1, 39) and np.array_equal(st.offsets, OFF)
    assert st.ic.shape == (1, 5) and st.best_sweep.tolist() == [45]
    assert st.best == [[createMotifIndex(2.5, [])] * 3]
    assert st.finished().tolist() == [True]
    # the hand-made histogram: sequence 0 always at start 0, sequence 1 at [] four times of
    # five, sequence 2 always at start 2
    assert st.mode() == [createMotifIndex(1.0, [0]), createMotifIndex(0.8, []),
                         createMotifIndex(1.0, [2])]
    assert [m.sum() for m in st.marginals()] == [1.0, 1.0, 1.0]


def test_no_counted_sweep_and_bad_arguments(monkeypatch):
    ctx = FakeCtx()
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    mem = [createMotifIndex(0.0, [1])] * 3
    chain, st = MotifSampler.runSweepsStats(W, 1e-4, 1.0, "ACGT", SOURCES, mem, 7, 7, 1, seed=9)
    assert ctx.calls == [(W, 1e-4, 1.0, 7, 9, [1, 1, 1], 0, None, 7, 1)]
    assert st.ic.shape == (1, 0) and st.best == [[]] and st.best_sweep.tolist() == [-1]

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    with pytest.raises(ArgumentError):  # a list of two positions
        MotifSampler.runSweepsStats(W, 1e-4, 1.0, "ACGT", SOURCES,
                                    [createMotifIndex(0.0, [1, 9])] + mem[1:], 3, 0, 1)
    with pytest.raises(ArgumentError):  # motifMem shorter than the sources
        MotifSampler.runSweepsStats(W, 1e-4, 1.0, "ACGT", SOURCES, mem[:2], 3, 0, 1)
