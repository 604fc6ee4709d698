"""Host side of SiteSampler.getMotifsWithBestInformationContent(batch=True): one
Context.site_sampling_batch call over the seeds base … base + numberOfRepetitions, replayed
by the loop of .fs:615-640; a run whose status is set raises when the loop asks for it.
The context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import SiteSampler, _native, sampler


class FakeCtx:
    """site_sampling_batch over a table of runs (score rows), positions = the row index."""

    def __init__(self, scores, status=None):
        self.scores = np.asarray(scores, np.float64)
        self.status = status
        self.calls = []

    def site_sampling_batch(self, W, pc, seeds, init_mode=0, max_passes=1000):
        self.calls.append((W, pc, list(seeds), init_mode))
        R, n = len(seeds), self.scores.shape[1]
        pos = np.repeat(np.arange(R, dtype=np.int32)[:, None], n, axis=1)
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        return pos, self.scores[:R].copy(), np.ones((R, 3), np.int32), status


def run_batch(monkeypatch, ctx, reps, seed=10, init_mode=1):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return SiteSampler.getMotifsWithBestInformationContent(reps, 5, 1e-4, "ACGT", [b"ACGTACGT"] * 2,
                                                          seed=seed, init_mode=init_mode,
                                                          batch=True)


def test_one_batch_call_over_all_seeds_then_the_replay(monkeypatch):
    # run 0 is adopted, run 1 loses, run 2 beats it, run 3 loses
    ctx = FakeCtx([[1.0, 1.0], [0.5, 0.5], [3.0, 3.0], [2.0, 2.0]])
    best = run_batch(monkeypatch, ctx, 3)
    assert ctx.calls == [(5, 1e-4, [10, 11, 12, 13], 1)]
    assert best == [(3.0, 2), (3.0, 2)]
    table = [[(float(s), r) for s in row] for r, row in enumerate(ctx.scores)]
    want = sampler._replay_repetitions(3, table.__getitem__, lambda xs: sum(s for s, _ in xs),
                                       [(0.0, 0)])
    assert best == want


def test_a_failed_run_raises_when_the_loop_asks_for_it(monkeypatch):
    scores = [[1.0, 1.0], [2.0, 2.0], [1.0, 1.0]]
    # the loop asks for run 0, adopts it one step later (no run asked there), then asks
    # for run 2: that one failed
    with pytest.raises(_native.GibbsError) as e:
        run_batch(monkeypatch, FakeCtx(scores, [0, 0, _native.GS_E_OVERFLOW]), 2)
    assert e.value.status == _native.GS_E_OVERFLOW
    # run 1 is computed but never asked for: its status does not surface
    ctx = FakeCtx(scores, [0, _native.GS_E_OVERFLOW, 0])
    assert run_batch(monkeypatch, ctx, 2) == [(1.0, 0), (1.0, 0)]
    assert ctx.calls[0][2] == [10, 11, 12]
