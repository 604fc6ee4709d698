"""Host side of the chain statistics: MotifSampler.runSweepsBatchedStats makes one
Context.motif_run_batch_stats call with the arguments passed through and wraps what comes
back in a ChainStats; ChainStats.marginals / mode pool the finished chains and take the
first maximum; sampler.informationContent restates the device's summation order.  The
context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import (ArgumentError, ChainStats, ChecksumOverflowError, MotifSampler,
                               _native, sampler)
from gibbssampling_amd.sampler import createMotifIndex, informationContent

SOURCES = [b"ACGTACGTACGTACGT"] * 3
W = 5
OFF = np.array([0, 13, 26, 39], np.int64)  # 1 + (16 - 5 + 1) bins a sequence


class FakeCtx:
    """motif_run_batch_stats over a table: chain r ends with sequence n at r + n (at []
    where r + n is odd), PWMS (r + n) / 4; its best state is all-[] with PWMS r."""

    def __init__(self, status=None):
        self.status = status
        self.calls = []

    def motif_run_batch_stats(self, W, pc, cutoff, n_sweeps, seeds, pos=None, init_mode=0,
                              first_sweep=0, u=None, burn_in=0, thin=1):
        self.calls.append((W, pc, cutoff, n_sweeps, list(seeds),
                           None if pos is None else np.array(pos).tolist(), init_mode,
                           first_sweep, u, burn_in, thin))
        R, n = len(seeds), len(SOURCES)
        out = (np.arange(R)[:, None] + np.arange(n)[None, :]).astype(np.int32)
        pwms = out / 4.0
        out[out % 2 == 1] = -1
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        nc = len(range(burn_in, n_sweeps, thin))
        occ = np.zeros((R, OFF[-1]), np.int32)
        occ[:, OFF[:-1]] = nc
        stats = {"occupancy": occ, "offsets": OFF.copy(),
                 "ic": np.arange(R * nc, dtype=np.float64).reshape(R, nc),
                 "best_sweep": np.array([first_sweep + burn_in if nc else -1] * R, np.int64),
                 "best_pos": np.full((R, n), -1, np.int32),
                 "best_pwms": np.tile(np.arange(R, dtype=np.float64)[:, None], (1, n))}
        return out, pwms, status, stats


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


def test_one_call_with_the_arguments_passed_through(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    mems = [[createMotifIndex(0.5, [3]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])],
            [createMotifIndex(0.0, []), createMotifIndex(2.0, [1]), createMotifIndex(0.0, [])]]
    chains, st = MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 20,
                                                    [10, 2**64 + 11], mems, first_sweep=40,
                                                    burn_in=5, thin=3)
    assert ctx.calls == [(W, 1e-4, 1.0, 20, [10, 11], [[3, -1, 7], [-1, 1, -1]], 0, 40, None, 5, 3)]
    assert chains == [[createMotifIndex(0.0, [0]), createMotifIndex(0.25, []),
                       createMotifIndex(0.5, [2])],
                      [createMotifIndex(0.25, []), createMotifIndex(0.5, [2]),
                       createMotifIndex(0.75, [])]]
    assert isinstance(st, ChainStats)
    assert st.occupancy.shape == (2, 39) and np.array_equal(st.offsets, OFF)
    assert st.ic.shape == (2, 5) and st.best_sweep.tolist() == [45, 45]
    assert st.best == [[createMotifIndex(0.0, [])] * 3, [createMotifIndex(1.0, [])] * 3]
    assert st.finished().tolist() == [True, True]
    assert st.mode() == [createMotifIndex(1.0, [])] * 3


def test_without_starts_the_init_mode_goes_through(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    chains, st = MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 7, [1, 2, 3],
                                                    init_mode=1, burn_in=7)
    assert ctx.calls == [(W, 1e-4, 1.0, 7, [1, 2, 3], None, 1, 0, None, 7, 1)]
    assert len(chains) == 3 and st.ic.shape == (3, 0)
    assert st.best == [[], [], []] and st.best_sweep.tolist() == [-1, -1, -1]


def test_only_single_positions_of_motif_amount_one(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    full = [createMotifIndex(0.0, [1])] * len(SOURCES)
    with pytest.raises(ArgumentError):
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], motifAmount=2)
    with pytest.raises(ArgumentError):  # a list of two positions
        two = [createMotifIndex(0.0, [1, 9])] + full[1:]
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [full, two])
    with pytest.raises(ArgumentError):  # one chain's motifMem shorter than the sources
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2],
                                           [full, full[:2]])
    with pytest.raises(ArgumentError):  # fewer motifMems than seeds
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [full])


def test_a_set_status_raises_the_mapped_exception(monkeypatch):
    bind(monkeypatch, FakeCtx([0, _native.GS_E_OVERFLOW, 0]))
    with pytest.raises(ChecksumOverflowError) as e:
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3])
    assert e.value.status == _native.GS_E_OVERFLOW
    bind(monkeypatch, FakeCtx([_native.GS_E_ROULETTE_OVERRUN, 0, 0]))
    with pytest.raises(_native.GibbsError) as e:
        MotifSampler.runSweepsBatchedStats(W, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3])
    assert e.value.status == _native.GS_E_ROULETTE_OVERRUN


def hand_made():
    """Two sequences of 3 and 2 bins, three chains of 4 counted sweeps; chain 2 raised
    after one of them and is left out of the pool."""
    off = np.array([0, 3, 5], np.int64)
    occ = np.array([[1, 3, 0, 2, 2],
                    [3, 1, 0, 1, 3],
                    [0, 0, 1, 1, 0]], np.int32)
    ic = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0],
                   [1.0, np.nan, np.nan, np.nan]])
    return ChainStats(occ, off, ic, np.array([3, 3, 0]), [[], [], []])


def test_marginals_pool_the_finished_chains():
    st = hand_made()
    assert st.finished().tolist() == [True, True, False]
    m = st.marginals()
    assert [a.tolist() for a in m] == [[4 / 8, 4 / 8, 0.0], [3 / 8, 5 / 8]]
    per = st.marginals(pool=False)
    assert per[0].tolist() == [[0.25, 0.75, 0.0], [0.75, 0.25, 0.0], [0.0, 0.0, 1.0]]
    assert per[1].tolist() == [[0.5, 0.5], [0.25, 0.75], [1.0, 0.0]]


def test_mode_takes_the_first_maximum():
    # sequence 0 ties between [] and start 0: the first bin, Positions []
    assert hand_made().mode() == [createMotifIndex(0.5, []), createMotifIndex(5 / 8, [0])]
    none = ChainStats(np.zeros((1, 5), np.int32), np.array([0, 3, 5]), np.zeros((1, 0)),
                      np.array([-1]), [[]])
    assert [a.tolist() for a in none.marginals()] == [[0.0] * 3, [0.0] * 2]


def test_information_content_restates_the_summation_order():
    # 130 entries: lane 0 adds x[0], x[64], x[128]; lane 1 x[1], x[65], x[129]
    x = np.zeros(130)
    x[0], x[64], x[128] = 1e300, -1e300, 3.0     # lane 0: (1e300 - 1e300) + 3 = 3
    x[1], x[65], x[129] = 1.0, 1e300, -1e300     # lane 1: (1 + 1e300) - 1e300 = 0
    x[33] = 0.5                                   # joins lane 1 at s = 32, lane 0 at s = 1
    # the tree: v[1] = 0 + 0.5; v[0] = 3 + 0.5
    assert informationContent(x) == 3.5
    # any other order gives another value: left to right the 3.0 is absorbed, not the 1.0
    assert float(np.add.reduce(x[[0, 64, 128, 1, 65, 129, 33]])) != 3.5
    left = 0.0
    for v in x:
        left += v
    assert left != 3.5
    # terms 1 apart sit in different lanes and meet only in the tree
    y = np.zeros(64)
    y[0], y[1], y[2] = 1e300, -1e300, 1.0
    # s = 1 is the last step: v[0] = 1e300 + 1 (from lane 2 at s = 2) = 1e300, then - 1e300
    assert informationContent(y) == 0.0
    z = np.zeros(64)
    z[0], z[1], z[3] = 1e300, -1e300, 1.0
    # lane 3 joins lane 1 at s = 2: v[1] = -1e300 + 1 = -1e300; v[0] = 1e300 - 1e300
    assert informationContent(z) == 0.0
    w = np.zeros(128)
    w[0], w[64], w[1] = 1e300, -1e300, 1.0      # 64 apart: cancelled inside lane 0 first
    assert informationContent(w) == 1.0
    assert informationContent([]) == 0.0 and informationContent([2.5]) == 2.5
    assert np.isnan(informationContent([1.0, np.nan]))
