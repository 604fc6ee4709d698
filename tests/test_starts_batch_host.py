"""Host side of SiteSampler.getPWMOfRandomStartsBatched: one Context.random_starts_batch call
over the seeds, one [(score, start)] list per seed back; a chain whose status is set raises
the mapped exception naming the chain.  The context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import ChecksumOverflowError, SiteSampler, _native, sampler

SOURCES = [b"ACGTACGTACGTACGT"] * 3


class FakeCtx:
    """random_starts_batch over a table: chain r puts sequence n at r + n with score
    -(r + n) / 4."""

    def __init__(self, status=None):
        self.status = status
        self.calls = []

    def random_starts_batch(self, W, pc, seeds, mode=0):
        self.calls.append((W, pc, list(seeds), mode))
        R, n = len(seeds), len(SOURCES)
        pos = (np.arange(R)[:, None] + np.arange(n)[None, :]).astype(np.int32)
        score = -pos / 4.0
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        return score, pos, status


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


def test_one_call_over_all_seeds_with_one_list_per_seed(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    out = SiteSampler.getPWMOfRandomStartsBatched(5, 1e-4, "ACGT", SOURCES, [10, 2**64 + 11, -1],
                                                  init_mode=1)
    # the seeds are masked to 64 bits before they reach the context
    assert ctx.calls == [(5, 1e-4, [10, 11, 2**64 - 1], 1)]
    assert out == [[(0.0, 0), (-0.25, 1), (-0.5, 2)],
                   [(-0.25, 1), (-0.5, 2), (-0.75, 3)],
                   [(-0.5, 2), (-0.75, 3), (-1.0, 4)]]
    assert all(isinstance(s, float) and isinstance(p, int) for row in out for s, p in row)


def test_the_defaults_and_no_seed(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    out = SiteSampler.getPWMOfRandomStartsBatched(5, 1e-4, "ACGT", SOURCES, [1, 2])
    assert ctx.calls == [(5, 1e-4, [1, 2], 0)]
    assert len(out) == 2 and all(len(chain) == len(SOURCES) for chain in out)
    assert SiteSampler.getPWMOfRandomStartsBatched(5, 1e-4, "ACGT", SOURCES, []) == []


def test_a_set_status_raises_the_mapped_exception_naming_the_chain(monkeypatch):
    bind(monkeypatch, FakeCtx([0, _native.GS_E_OVERFLOW, 0]))
    with pytest.raises(ChecksumOverflowError) as e:
        SiteSampler.getPWMOfRandomStartsBatched(5, 1e-4, "ACGT", SOURCES, [1, 2, 3])
    assert e.value.status == _native.GS_E_OVERFLOW and "chain 1" in str(e.value)
    bind(monkeypatch, FakeCtx([0, 0, _native.GS_E_HIP]))
    with pytest.raises(_native.DeviceError) as e:
        SiteSampler.getPWMOfRandomStartsBatched(5, 1e-4, "ACGT", SOURCES, [1, 2, 3])
    assert e.value.status == _native.GS_E_HIP and "chain 2" in str(e.value)
