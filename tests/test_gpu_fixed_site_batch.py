"""GPU parity of gs_site_sampling_batch_fixed (Context.site_sampling_batch(pcv=, ppm=)):
R repetitions of doSiteSamplingWithBPV (getMotifsWithBestInformationContentWithBPV,
.fs:434-459) or of doSiteSamplingWithPPM (getBestInformationContentOfPPM, .fs:664-689) in
one call.  Every row against the oracle's composition random_starts (…WithBPV / …OfPPM) ->
site_refine 0 / -1 / +1 for its seed, the three pass counts included, and against the
sequential entry point gs_site_sampling on a second context that has the values set on it.

Bar: positions and pass counts exact, scores within 1e-12 relative; against the
site_switch = 0 single chain (the star engine on both sides, the shifted scan the same
device function on the same integer aggregates) bit-identical scores."""
import numpy as np
import pytest

from conftest import make_dataset
from fixed_batch_cases import (PC, SEEDS, SHAPES, bits, close, dataset, pcv49, ppm49, set_fixed,
                               sources_of, values)
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

MODES = (0, 1)
KINDS = ("pcv", "ppm")


def oracle_site_sampling(S, W, seed, mode, pcv, ppm):
    """-> (pos, score, the three pass counts, starts moved by each stage)."""
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=mode, pcv49=pcv, ppm49=ppm)
    passes, moved = [], []
    for shift in (0, -1, 1):
        p2, sc, np_ = ol.site_refine(S, W, PC, shift, p, sc, pcv49=pcv)
        passes.append(np_)
        moved.append(int((p2 != p).sum()))
        p = p2
    return p, sc, tuple(passes), tuple(moved)


def fresh(tuning=None):
    from gibbssampling_amd import Context
    return Context(0, tuning=tuning)


@pytest.fixture(scope="module")
def other_ctx():
    ctx = fresh()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def star_ctx():
    """Sequential runs with every Gauss–Seidel pass on the star engine, as the batch's."""
    ctx = fresh({"site_switch": 0})
    yield ctx
    ctx.close()


_cases = {}
_oracle = {}


def case(name, mode, kind, batch_starts=0):
    key = (name, mode, kind, batch_starts)
    if key not in _cases:
        alpha, _, N, L, W, _, _ = SHAPES[name]
        codes, offsets = dataset(name)
        pcv, ppm = values(name, kind)
        ctx = fresh({"batch_starts": batch_starts})
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.site_sampling_batch(W, PC, SEEDS, mode, pcv=pcv, ppm=ppm)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


def oracle_case(name, mode, kind, seed):
    key = (name, mode, kind, seed)
    if key not in _oracle:
        alpha, _, N, L, W, _, _ = SHAPES[name]
        codes, offsets = dataset(name)
        pcv, ppm = values(name, kind)
        _oracle[key] = oracle_site_sampling(ol.Seqs(codes, offsets, alpha), W, seed, mode, pcv, ppm)
    return _oracle[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name, mode, kind):
    alpha, _, N, L, W, _, _ = SHAPES[name]
    pos, score, passes, status = case(name, mode, kind)
    assert pos.shape == (len(SEEDS), N) and score.shape == (len(SEEDS), N)
    assert passes.shape == (len(SEEDS), 3)
    assert not status.any()
    for r, seed in enumerate(SEEDS):
        op, osc, opass, _ = oracle_case(name, mode, kind, seed)
        assert np.array_equal(pos[r], op), (seed, r)
        assert tuple(passes[r]) == opass, (seed, r)
        assert close(score[r], osc), (seed, r)
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3]) and np.array_equal(passes[1], passes[3])
    assert np.array_equal(bits(score[1]), bits(score[3]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_shifted_passes_move_starts_under_a_pcv(name, mode):
    """The batched scan's branch for the caller's PCV is exercised: on the oracle's side
    chains move starts in the left-shifted and in the right-shifted stage, take more than
    one pass there, and do not stop together."""
    runs = [oracle_case(name, mode, "pcv", seed) for seed in SEEDS]
    for stage in (1, 2):
        assert any(r[3][stage] > 0 for r in runs), (stage, [r[3] for r in runs])
        assert any(r[2][stage] > 1 for r in runs), (stage, [r[2] for r in runs])
    assert len({r[2] for r in runs}) > 1
    _, _, passes, _ = case(name, mode, "pcv")
    assert [tuple(p) for p in passes] == [r[2] for r in runs]


@pytest.mark.parametrize("kind", KINDS + ("both",))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_both_ways_of_making_the_starts_honour_the_values(name, mode, kind):
    a, b = case(name, mode, kind, 0), case(name, mode, kind, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert not a[3].any() and not b[3].any()


@pytest.mark.parametrize("kind", KINDS + ("both",))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, mode, kind, other_ctx, star_ctx):
    alpha, _, N, L, W, _, _ = SHAPES[name]
    codes, offsets = dataset(name)
    pcv, ppm = values(name, kind)
    pos, score, passes, status = case(name, mode, kind)
    for ctx in (other_ctx, star_ctx):
        ctx.set_sequences(codes, offsets, alpha)
        set_fixed(ctx, pcv, ppm, W)
    try:
        for r, seed in enumerate(SEEDS):
            sp, ssc, spass = other_ctx.site_sampling(W, PC, seed, mode)
            assert np.array_equal(pos[r], sp) and np.array_equal(passes[r], spass), (seed, r)
            assert close(score[r], ssc), (seed, r)
            tp, tsc, tpass = star_ctx.site_sampling(W, PC, seed, mode)
            assert np.array_equal(pos[r], tp) and np.array_equal(passes[r], tpass), (seed, r)
            assert np.array_equal(bits(score[r]), bits(tsc)), (seed, r)
    finally:
        for ctx in (other_ctx, star_ctx):
            set_fixed(ctx, None, None, W)


@pytest.mark.parametrize("N", [5, 12])
def test_more_chains_than_cus_fewer_targets_than_wavefronts(N, gpu_ctx, other_ctx):
    L, W, R = 30, 5, 300
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=90 + N, mut=0.1)
    pcv = pcv49(b"ACGT", N)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    seeds = [7000 + 3 * r for r in range(R)]
    pos, score, passes, status = gpu_ctx.site_sampling_batch(W, PC, seeds, pcv=pcv)
    assert not status.any()
    other_ctx.set_fixed_pcv(pcv)
    try:
        for r, seed in enumerate(seeds):
            sp, ssc, spass = other_ctx.site_sampling(W, PC, seed)
            assert np.array_equal(pos[r], sp) and np.array_equal(passes[r], spass), (seed, r)
            assert close(score[r], ssc), (seed, r)
    finally:
        other_ctx.set_fixed_pcv(None)
    assert len({p.tobytes() for p in pos}) > 1  # the seeds reach the chains


def test_last_ms_reports_the_fixed_call(gpu_ctx):
    alpha, _, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = dataset("protein")
    pcv, _ = values("protein", "pcv")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    gpu_ctx.site_sampling_batch(W, PC, SEEDS, pcv=pcv)
    ms = gpu_ctx.site_batch_last_ms()
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)


@pytest.mark.parametrize("reps", [3, 0])
def test_mirrors_batch_keyword(reps):
    from gibbssampling_amd import SiteSampler
    N, L, W, seed = 40, 60, 7, 99
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = sources_of(codes, offsets)
    pcv, ppm = pcv49(b"ACGT", 5), ppm49(W, 6)
    for mode in MODES:
        loop = SiteSampler.getMotifsWithBestInformationContentWithBPV(
            reps, W, PC, "ACGT", sources, pcv, seed=seed, init_mode=mode)
        batch = SiteSampler.getMotifsWithBestInformationContentWithBPV(
            reps, W, PC, "ACGT", sources, pcv, seed=seed, init_mode=mode, batch=True)
        assert [p for _, p in batch] == [p for _, p in loop]
        assert close([s for s, _ in batch], [s for s, _ in loop])
        assert len(batch) == (N if reps else 1)
    loop = SiteSampler.getBestInformationContentOfPPM(reps, W, PC, "ACGT", sources, ppm, seed=seed)
    batch = SiteSampler.getBestInformationContentOfPPM(reps, W, PC, "ACGT", sources, ppm,
                                                       seed=seed, batch=True)
    assert [p for _, p in batch] == [p for _, p in loop]
    assert close([s for s, _ in batch], [s for s, _ in loop])
    assert len(batch) == (N if reps else 1)
