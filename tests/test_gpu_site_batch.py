"""GPU parity of gs_site_sampling_batch: R independent doSiteSampling chains
(.fs:697-701) whose Gauss–Seidel passes run as R concurrent workgroups and whose shifted
passes run side by side, one synchronisation per pass for all chains.  Every row against
the oracle's composition random_starts -> site_refine 0 / -1 / +1 for its seed, and
against the sequential entry point gs_site_sampling on a second context."""
import numpy as np
import pytest

from conftest import make_dataset
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC = 1e-4
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]

# name: (alphabet, N, L, W, ragged, init_mode, dataset seed)
SHAPES = {
    "dna-mode0": (b"ACGT", 150, 90, 9, True, 0, 77),
    "dna-mode1": (b"ACGT", 150, 90, 9, True, 1, 78),
    "gap-symbol": (b"ATGC-", 150, 90, 9, True, 0, 79),
    "protein": (PROTEIN, 40, 60, 8, False, 0, 80),
}


def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    same = g == o
    rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(same | (rel <= RTOL)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def oracle_site_sampling(S, W, seed, init_mode, max_passes=1000):
    """oracle_site_sampling of test_gpu_drivers.py, keeping the three pass counts."""
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=init_mode)
    passes = []
    for shift in (0, -1, 1):
        p, sc, np_ = ol.site_refine(S, W, PC, shift, p, sc, max_passes=max_passes)
        passes.append(np_)
    return p, sc, tuple(passes)


@pytest.fixture(scope="module")
def other_ctx():
    """The sequential side: a second context with the shipped defaults."""
    from gibbssampling_amd import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def star_ctx():
    """Sequential runs with every Gauss–Seidel pass on the star engine, as the batch's."""
    from gibbssampling_amd import Context
    ctx = Context(0, tuning={"site_switch": 0})
    yield ctx
    ctx.close()


_cases = {}
_oracle = {}


def case(name):
    """Dataset and one batch result per shape, computed once and left unchanged."""
    if name not in _cases:
        from gibbssampling_amd import Context
        alpha, N, L, W, ragged, mode, dseed = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
        ctx = Context(0)
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.site_sampling_batch(W, PC, SEEDS, mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[name] = (codes, offsets, out)
    return _cases[name]


def oracle_case(name, seed):
    """The oracle's run of one seed of a shape, computed once."""
    if (name, seed) not in _oracle:
        alpha, N, L, W, ragged, mode, _ = SHAPES[name]
        codes, offsets, _ = case(name)
        _oracle[name, seed] = oracle_site_sampling(ol.Seqs(codes, offsets, alpha), W, seed, mode)
    return _oracle[name, seed]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name):
    alpha, N, L, W, ragged, mode, _ = SHAPES[name]
    codes, offsets, (pos, score, passes, status) = case(name)
    assert pos.shape == (len(SEEDS), N) and score.shape == (len(SEEDS), N)
    assert passes.shape == (len(SEEDS), 3)
    assert not status.any()
    if ragged:  # sequences of one window: both shifts clamp
        assert (np.diff(offsets) == W).any()
    for r, seed in enumerate(SEEDS):
        op, osc, opass = oracle_case(name, seed)
        assert np.array_equal(pos[r], op), (seed, r)
        assert tuple(passes[r]) == opass, (seed, r)
        assert close(score[r], osc), (seed, r)
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3]) and np.array_equal(passes[1], passes[3])
    assert np.array_equal(bits(score[1]), bits(score[3]))


@pytest.mark.parametrize("name", ["dna-mode1", "protein"])
def test_the_chains_do_not_stop_together(name):
    """The per-chain finish flag is exercised: in each of the three stages the oracle's
    pass counts differ across the seeds, and the batch reproduces them."""
    _, _, (pos, score, passes, status) = case(name)
    triples = [oracle_case(name, seed)[2] for seed in SEEDS]
    for stage in range(3):
        assert len({t[stage] for t in triples}) > 1, (stage, triples)
    assert [tuple(p) for p in passes] == triples


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, other_ctx, star_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES[name]
    codes, offsets, (pos, score, passes, status) = case(name)
    other_ctx.set_sequences(codes, offsets, alpha)
    star_ctx.set_sequences(codes, offsets, alpha)
    for r, seed in enumerate(SEEDS):
        sp, ssc, spass = other_ctx.site_sampling(W, PC, seed, mode)
        assert np.array_equal(pos[r], sp) and np.array_equal(passes[r], spass), (seed, r)
        assert close(score[r], ssc), (seed, r)
        # site_switch = 0: the star engine on both sides for the Gauss–Seidel passes, and
        # the batch's shifted scan is gs_starts_kernel's mode-2 body on the same integer
        # aggregates (ppm = (count + pc) / den, best_pwms_scan, log(best) / ln 2): the same
        # binary64 operations in the same order, so the scores are bit-identical
        tp, tsc, tpass = star_ctx.site_sampling(W, PC, seed, mode)
        assert np.array_equal(pos[r], tp) and np.array_equal(passes[r], tpass), (seed, r)
        assert np.array_equal(bits(score[r]), bits(tsc)), (seed, r)


@pytest.mark.parametrize("N", [5, 12])
def test_more_chains_than_cus_fewer_targets_than_wavefronts(N, gpu_ctx, other_ctx):
    L, W, R = 30, 5, 300
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=90 + N, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    seeds = [7000 + 3 * r for r in range(R)]
    pos, score, passes, status = gpu_ctx.site_sampling_batch(W, PC, seeds)
    assert not status.any()
    for r, seed in enumerate(seeds):
        sp, ssc, spass = other_ctx.site_sampling(W, PC, seed)
        assert np.array_equal(pos[r], sp) and np.array_equal(passes[r], spass), (seed, r)
        assert close(score[r], ssc), (seed, r)
    assert len({p.tobytes() for p in pos}) > 1  # the seeds reach the chains


def test_one_pass_only(gpu_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES["dna-mode0"]
    codes, offsets, _ = case("dna-mode0")
    S = ol.Seqs(codes, offsets, alpha)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    pos, score, passes, status = gpu_ctx.site_sampling_batch(W, PC, SEEDS, mode, max_passes=1)
    assert not status.any()
    assert (passes == 1).all()
    for r, seed in enumerate(SEEDS):
        op, osc, opass = oracle_site_sampling(S, W, seed, mode, max_passes=1)
        assert opass == (1, 1, 1)
        assert np.array_equal(pos[r], op) and close(score[r], osc), (seed, r)


def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES["protein"]
    codes, offsets, _ = case("protein")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    want = other_ctx.site_sampling(W, PC, 31)

    # one chain is gs_site_sampling
    pos, score, passes, status = gpu_ctx.site_sampling_batch(W, PC, [31])
    assert pos.shape == (1, N) and passes.shape == (1, 3) and status[0] == 0
    assert np.array_equal(pos[0], want[0]) and np.array_equal(passes[0], want[2])
    assert close(score[0], want[1])
    ms = gpu_ctx.site_batch_last_ms()
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0.0 for m in ms)
    # no snapshot is left behind
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    # ... and the next single run behaves as on a fresh context
    again = gpu_ctx.site_sampling(W, PC, 31)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[2], want[2])
    assert np.array_equal(bits(again[1]), bits(want[1]))
    assert isinstance(gpu_ctx.stats(), dict)  # the counters go on

    # no chains: nothing to do
    pos, score, passes, status = gpu_ctx.site_sampling_batch(W, PC, [])
    assert pos.shape == (0, N) and score.shape == (0, N)
    assert passes.shape == (0, 3) and status.shape == (0,)

    # argument errors before any launch
    before = gpu_ctx.stats()
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.site_sampling_batch(L + 1, PC, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.site_sampling_batch(W, PC, [1, 2], init_mode=2)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.site_sampling_batch(W, PC, [1, 2], max_passes=0)
    assert gpu_ctx.stats() == before

    # the WithBPV twin is not batched
    gpu_ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            gpu_ctx.site_sampling_batch(W, PC, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        gpu_ctx.set_fixed_pcv(None)


def test_mirror_batch_keyword():
    from gibbssampling_amd import SiteSampler
    N, L, W, seed = 40, 60, 7, 99
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    loop = SiteSampler.getMotifsWithBestInformationContent(3, W, PC, "ACGT", sources, seed=seed)
    batch = SiteSampler.getMotifsWithBestInformationContent(3, W, PC, "ACGT", sources, seed=seed,
                                                            batch=True)
    assert [p for _, p in batch] == [p for _, p in loop]
    assert close([s for s, _ in batch], [s for s, _ in loop])
    assert len(batch) == N
