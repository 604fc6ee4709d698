"""Host side of MotifSampler.getMotifsWithBestInformationContentsBatched: with motifAmount >=
2 one Context.motif_sampling_multi_batch call over the seeds base … base +
numberOfRepetitions, replayed by the loop of .fs:973-998 with the list form of MotifIndex; a
run whose status is set raises when the loop asks for it.  motifAmount = 1 keeps
Context.motif_sampling_batch, there and in getMotifsWithBestInformationContents(batch=True).
The context is a stand-in: no device is touched."""
import numpy as np
import pytest

from gibbssampling_amd import ArgumentError, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex


class FakeCtx:
    """Both batch calls over a table of runs (PWMS rows); run r's lists are [r + n, n]
    for sequence n (single positions: r + n)."""

    def __init__(self, pwms, status=None):
        self.pwms = np.asarray(pwms, np.float64)
        self.status = status
        self.calls = []

    def _status(self, R):
        return np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)

    def motif_sampling_multi_batch(self, motif_amount, W, pc, cutoff, seeds, init_mode=0,
                                   max_passes=1000, cap=None):
        self.calls.append(("multi", motif_amount, W, pc, cutoff, list(seeds), init_mode))
        R, n = len(seeds), self.pwms.shape[1]
        cap = cap or motif_amount
        cnt = np.full((R, n), 2, np.int32)
        pos = np.full((R, n, cap), -1, np.int32)
        pos[:, :, 0] = np.arange(R)[:, None] + np.arange(n)[None, :]
        pos[:, :, 1] = np.arange(n)[None, :]
        return cnt, pos, self.pwms[:R].copy(), np.ones(R, np.int32), self._status(R)

    def motif_sampling_batch(self, W, pc, cutoff, seeds, init_mode=0, max_passes=1000):
        self.calls.append(("single", W, pc, cutoff, list(seeds), init_mode))
        R, n = len(seeds), self.pwms.shape[1]
        pos = (np.arange(R)[:, None] + np.arange(n)[None, :]).astype(np.int32)
        return pos, self.pwms[:R].copy(), np.ones(R, np.int32), self._status(R)


def run_batch(monkeypatch, ctx, reps, motif_amount=2, seed=10, init_mode=1):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return MotifSampler.getMotifsWithBestInformationContentsBatched(
        reps, motif_amount, 5, 1e-4, 1.0, "ACGT", [b"ACGTACGTACGTACGT"] * 2, seed=seed,
        init_mode=init_mode)


def table_of(ctx):
    return [[createMotifIndex(w, [r + n, n]) for n, w in enumerate(row)]
            for r, row in enumerate(ctx.pwms)]


def test_one_list_batch_call_over_all_seeds_then_the_replay(monkeypatch):
    # run 0 is adopted, run 1 loses, run 2 beats it, run 3 loses
    ctx = FakeCtx([[1.0, 1.0], [0.5, 0.5], [3.0, 3.0], [2.0, 2.0]])
    best = run_batch(monkeypatch, ctx, 3)
    assert ctx.calls == [("multi", 2, 5, 1e-4, 1.0, [10, 11, 12, 13], 1)]
    assert best == [createMotifIndex(3.0, [2, 0]), createMotifIndex(3.0, [3, 1])]
    want = sampler._replay_repetitions(3, table_of(ctx).__getitem__,
                                       lambda xs: sum(x.PWMS for x in xs),
                                       [createMotifIndex(0.0, [])])
    assert best == want


def test_a_failed_run_raises_when_the_loop_asks_for_it(monkeypatch):
    pwms = [[1.0, 1.0], [2.0, 2.0], [1.0, 1.0]]
    # the loop asks for run 0, adopts it one step later (no run asked there), then asks
    # for run 2: that one failed
    with pytest.raises(_native.GibbsError) as e:
        run_batch(monkeypatch, FakeCtx(pwms, [0, 0, _native.GS_E_OVERFLOW]), 2)
    assert e.value.status == _native.GS_E_OVERFLOW
    # run 1 is computed but never asked for: its status does not surface
    ctx = FakeCtx(pwms, [0, _native.GS_E_UNSUPPORTED, 0])
    assert run_batch(monkeypatch, ctx, 2) == table_of(ctx)[0]
    assert ctx.calls[0][5] == [10, 11, 12]


def test_motif_amount_one_keeps_the_single_position_batch(monkeypatch):
    ctx = FakeCtx([[1.0, 1.0], [0.5, 0.5]])
    best = run_batch(monkeypatch, ctx, 1, motif_amount=1)
    assert ctx.calls == [("single", 5, 1e-4, 1.0, [10, 11], 1)]
    assert best == [createMotifIndex(1.0, [0]), createMotifIndex(1.0, [1])]
    # ... and so does the batch keyword of the loop's own entry point
    again = MotifSampler.getMotifsWithBestInformationContents(
        1, 1, 5, 1e-4, 1.0, "ACGT", [b"ACGTACGTACGTACGT"] * 2, seed=10, init_mode=1, batch=True)
    assert ctx.calls[1] == ctx.calls[0] and again == best


def test_motif_amount_out_of_range_raises_before_a_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    for amount in (0, 17):
        with pytest.raises(ArgumentError):
            MotifSampler.getMotifsWithBestInformationContentsBatched(
                3, amount, 5, 1e-4, 1.0, "ACGT", [b"ACGTACGT"] * 4, seed=1)
