"""Host side of the batched repetition driver: the replay helper that the on-demand loop
and getMotifsWithBestInformationContents(batch=True) share, over synthetic run tables."""
import numpy as np
import pytest

from gibbssampling_amd import ArgumentError, MotifSampler
from gibbssampling_amd.sampler import _best_of_repetitions, _replay_repetitions


def loop_of_the_reference(numberOfRepetitions, run, ic, initial_best):
    """.fs:973-998 transcribed on its own: `loop n acc bestMotifs`."""
    def loop(n, acc, best):
        if n > numberOfRepetitions:
            return best
        if acc == best:
            return best
        if ic(acc) > ic(best):
            return loop(n + 1, [], best if not acc else acc)
        return loop(n + 1, run(n), best)
    return loop(0, [], initial_best)


def ic(xs):
    return sum(s for s, _ in xs)


def tables(seed):
    """Run tables of 7 runs x 3 entries: scores from a small set so that equal runs
    (the loop's early stop), runs beating the best and runs losing to it all occur."""
    rng = np.random.default_rng(seed)
    pool = [[(float(rng.integers(-2, 4)), int(rng.integers(0, 3))) for _ in range(3)]
            for _ in range(3)]
    return [list(pool[int(rng.integers(0, len(pool)))]) for _ in range(7)]


@pytest.mark.parametrize("reps", range(7))
def test_replay_over_a_table_is_the_on_demand_loop(reps):
    early = beaten = 0
    for seed in range(60):
        table = tables(seed)
        asked = []

        def run(r):
            asked.append(r)
            return table[r]
        want = loop_of_the_reference(reps, lambda r: table[r], ic, [(0.0, 0)])
        assert _replay_repetitions(reps, table.__getitem__, ic, [(0.0, 0)]) == want
        assert _best_of_repetitions(reps, run, ic, [(0.0, 0)]) == want
        # the batch computes runs 0 ... reps: the loop never asks for another
        assert all(0 <= r <= reps for r in asked)
        early += len(asked) < reps + 1
        beaten += want != [(0.0, 0)]
    if reps >= 3:
        assert early > 0 and beaten > 0  # the tables reach both branches


def test_replay_keeps_the_first_of_equal_runs_and_a_later_better_one():
    a, b = [(1.0, 5)], [(3.0, 2)]
    # run 0 is adopted at n = 1 (no run asked there), run 2 equals it: stop
    assert _replay_repetitions(6, [a, b, a, b, b, b, b].__getitem__, ic, [(0.0, 0)]) == a
    # b beats a and is adopted one step later
    assert _replay_repetitions(6, [a, a, b, a, a, a, a].__getitem__, ic, [(0.0, 0)]) == \
        loop_of_the_reference(6, [a, a, b, a, a, a, a].__getitem__, ic, [(0.0, 0)])


def test_batch_needs_motif_amount_one(monkeypatch):
    from gibbssampling_amd import sampler

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(sampler, "_bind", no_device)
    with pytest.raises(ArgumentError):
        MotifSampler.getMotifsWithBestInformationContents(3, 2, 5, 1e-4, 1.0, "ACGT",
                                                         [b"ACGTACGT"] * 4, seed=1, batch=True)
