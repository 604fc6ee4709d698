"""Host side of MotifSampler.runSweepsBatched: one Context.motif_run_batch call over the
seeds, the chains' starts as rows of single positions (-1 = Positions []), one
list[MotifIndex] per seed back; a chain whose status is set raises the mapped exception.
The context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import ArgumentError, MotifSampler, ChecksumOverflowError, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex

SOURCES = [b"ACGTACGTACGTACGT"] * 3


class FakeCtx:
    """motif_run_batch over a table: chain r moves sequence n to r + n (to [] where
    r + n is odd) with PWMS r + n / 4."""

    def __init__(self, status=None):
        self.status = status
        self.calls = []

    def motif_run_batch(self, W, pc, cutoff, n_sweeps, seeds, pos=None, init_mode=0,
                        first_sweep=0, u=None):
        self.calls.append((W, pc, cutoff, n_sweeps, list(seeds),
                           None if pos is None else np.array(pos).tolist(), init_mode,
                           first_sweep, u))
        R, n = len(seeds), len(SOURCES)
        out = (np.arange(R)[:, None] + np.arange(n)[None, :]).astype(np.int32)
        pwms = out / 4.0
        out[out % 2 == 1] = -1
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        return out, pwms, status


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


def test_one_call_over_all_seeds_with_the_starts_as_rows(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    mems = [[createMotifIndex(0.5, [3]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])],
            [createMotifIndex(0.0, []), createMotifIndex(2.0, [1]), createMotifIndex(0.0, [])]]
    out = MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 20, [10, 2**64 + 11], mems,
                                        first_sweep=40)
    # (the mirror passes no init_mode of its own meaning: the given rows imply -1 below it)
    assert ctx.calls == [(5, 1e-4, 1.0, 20, [10, 11], [[3, -1, 7], [-1, 1, -1]], 0, 40, None)]
    assert out == [[createMotifIndex(0.0, [0]), createMotifIndex(0.25, []),
                    createMotifIndex(0.5, [2])],
                   [createMotifIndex(0.25, []), createMotifIndex(0.5, [2]),
                    createMotifIndex(0.75, [])]]


def test_without_starts_the_init_mode_goes_through(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    out = MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 7, [1, 2, 3], init_mode=1)
    assert ctx.calls == [(5, 1e-4, 1.0, 7, [1, 2, 3], None, 1, 0, None)]
    assert len(out) == 3 and all(len(chain) == len(SOURCES) for chain in out)
    assert MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 7, []) == []


def test_motif_mems_of_differing_length_are_rejected(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    full = [createMotifIndex(0.0, [1])] * len(SOURCES)
    with pytest.raises(ArgumentError):  # one chain's motifMem shorter than the sources
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [full, full[:2]])
    with pytest.raises(ArgumentError):  # fewer motifMems than seeds
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [full])


def test_a_set_status_raises_the_mapped_exception(monkeypatch):
    bind(monkeypatch, FakeCtx([0, _native.GS_E_OVERFLOW, 0]))
    with pytest.raises(ChecksumOverflowError) as e:
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3])
    assert e.value.status == _native.GS_E_OVERFLOW
    bind(monkeypatch, FakeCtx([_native.GS_E_ROULETTE_OVERRUN, 0, 0]))
    with pytest.raises(_native.GibbsError) as e:
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3])
    assert e.value.status == _native.GS_E_ROULETTE_OVERRUN
