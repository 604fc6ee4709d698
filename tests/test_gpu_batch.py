"""GPU parity of gs_motif_sampling_batch: R independent doMotifSampling chains
(.fs:1034-1038) whose greedy passes run as R concurrent workgroups.  Every row against
the oracle's composition random_starts -> sweep(u of sweep 0) -> greedy for its seed,
and against the sequential entry point gs_motif_sampling on a second context."""
import numpy as np
import pytest

from conftest import make_dataset
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC, CUTOFF = 1e-4, 1.0
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


def oracle_motif_sampling(S, N, W, seed, init_mode, max_passes=1000):
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=init_mode)
    u = np.array([ol.uniform(seed, ol.stream_sweep(0), n) for n in range(N)])
    p1, w1, _ = ol.sweep(S, W, PC, CUTOFF, p, u)
    return ol.greedy(S, W, PC, CUTOFF, p1, w1, max_passes=max_passes)


@pytest.fixture(scope="module")
def other_ctx():
    """The sequential side: a second context with the shipped defaults."""
    from gibbssampling_amd import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def star_ctx():
    """Sequential runs with every pass on the star engine, as the batch's chains."""
    from gibbssampling_amd import Context
    ctx = Context(0, tuning={"greedy_switch": 0})
    yield ctx
    ctx.close()


_cases = {}


def case(name):
    """Dataset and one batch result per shape, computed once and left unchanged."""
    if name not in _cases:
        from gibbssampling_amd import Context
        alpha, N, L, W, ragged, mode, dseed = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
        ctx = Context(0)
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[name] = (codes, offsets, out)
    return _cases[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name):
    alpha, N, L, W, ragged, mode, _ = SHAPES[name]
    codes, offsets, (pos, pwms, passes, status) = case(name)
    assert pos.shape == (len(SEEDS), N) and pwms.shape == (len(SEEDS), N)
    assert not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    for seed in sorted(set(SEEDS)):
        op, ow, opass = oracle_motif_sampling(S, N, W, seed, mode)
        for r in [i for i, s in enumerate(SEEDS) if s == seed]:
            assert np.array_equal(pos[r], op), (seed, r)
            assert passes[r] == opass, (seed, r)
            assert close(pwms[r], ow), (seed, r)
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3]) and passes[1] == passes[3]
    assert np.array_equal(pwms[1].view(np.uint64), pwms[3].view(np.uint64))


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, other_ctx, star_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES[name]
    codes, offsets, (pos, pwms, passes, status) = case(name)
    other_ctx.set_sequences(codes, offsets, alpha)
    star_ctx.set_sequences(codes, offsets, alpha)
    for r, seed in enumerate(SEEDS):
        sp, sw, spass = other_ctx.motif_sampling(W, PC, CUTOFF, seed, mode)
        assert np.array_equal(pos[r], sp) and passes[r] == spass, (seed, r)
        assert close(pwms[r], sw), (seed, r)
        # the star engine on both sides: the same binary64 operations in the same order
        tp, tw, tpass = star_ctx.motif_sampling(W, PC, CUTOFF, seed, mode)
        assert np.array_equal(pos[r], tp) and passes[r] == tpass, (seed, r)
        assert np.array_equal(pwms[r].view(np.uint64), tw.view(np.uint64)), (seed, r)


@pytest.mark.parametrize("N", [5, 12])
def test_more_chains_than_cus_fewer_targets_than_wavefronts(N, gpu_ctx, other_ctx):
    L, W, R = 30, 5, 300
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=90 + N, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    seeds = [7000 + 3 * r for r in range(R)]
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, seeds)
    assert not status.any()
    for r, seed in enumerate(seeds):
        sp, sw, spass = other_ctx.motif_sampling(W, PC, CUTOFF, seed)
        assert np.array_equal(pos[r], sp) and passes[r] == spass, (seed, r)
        assert close(pwms[r], sw), (seed, r)
    assert len({p.tobytes() for p in pos}) > 1  # the seeds reach the chains


def test_one_pass_only(gpu_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES["dna-mode0"]
    codes, offsets, _ = case("dna-mode0")
    S = ol.Seqs(codes, offsets, alpha)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, mode,
                                                             max_passes=1)
    assert not status.any()
    assert (passes == 1).all()
    for r, seed in enumerate(SEEDS):
        op, ow, opass = oracle_motif_sampling(S, N, W, seed, mode, max_passes=1)
        assert opass == 1
        assert np.array_equal(pos[r], op) and close(pwms[r], ow), (seed, r)


def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, ragged, mode, _ = SHAPES["protein"]
    codes, offsets, _ = case("protein")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    want = other_ctx.motif_sampling(W, PC, CUTOFF, 31)

    # one chain is gs_motif_sampling
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [31])
    assert pos.shape == (1, N) and status[0] == 0
    assert np.array_equal(pos[0], want[0]) and passes[0] == want[2] and close(pwms[0], want[1])
    # no snapshot is left behind
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    # ... and the next single run behaves as on a fresh context
    again = gpu_ctx.motif_sampling(W, PC, CUTOFF, 31)
    assert np.array_equal(again[0], want[0]) and again[2] == want[2]
    assert np.array_equal(again[1].view(np.uint64), want[1].view(np.uint64))
    assert gpu_ctx.get_state()[0].shape == (N,)
    assert isinstance(gpu_ctx.stats(), dict)  # the counters go on

    # no chains: nothing to do
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [])
    assert pos.shape == (0, N) and passes.shape == (0,) and status.shape == (0,)

    # argument errors before any launch
    before = gpu_ctx.stats()
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_batch(L + 1, PC, CUTOFF, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [1, 2], init_mode=2)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [1, 2], max_passes=0)
    assert gpu_ctx.stats() == before

    # the ByPCV twin is not batched
    gpu_ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        gpu_ctx.set_fixed_pcv(None)


def test_mirror_batch_keyword():
    from gibbssampling_amd import MotifSampler
    N, L, W, seed = 40, 60, 7, 99
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    loop = MotifSampler.getMotifsWithBestInformationContents(3, 1, W, PC, CUTOFF, "ACGT",
                                                             sources, seed=seed)
    batch = MotifSampler.getMotifsWithBestInformationContents(3, 1, W, PC, CUTOFF, "ACGT",
                                                              sources, seed=seed, batch=True)
    assert [m.Positions for m in batch] == [m.Positions for m in loop]
    assert close([m.PWMS for m in batch], [m.PWMS for m in loop])
    assert len(batch) == N
