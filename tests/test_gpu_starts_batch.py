"""GPU parity of gs_random_starts_batch: R independent getPWMOfRandomStarts runs
(.fs:589-611) in a constant number of launches over the (chain, target) pairs.  Every row
against the oracle's random_starts for its seed (positions equal, scores within 1e-12
relative) and against the single-chain entry point gs_random_starts on a second context
(positions and score bits equal: the scan is the same device function).  The tuning field
batch_starts, which routes the four batched drivers' starts through the same launches, must
not change a bit of what they return."""
import numpy as np
import pytest

from conftest import make_dataset
from gibbssampling_amd import ArgumentError, GibbsError, _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC, CUTOFF = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]

# name: (alphabet, N, L, W, ragged, dataset seed, extra, extra_rate)
SHAPES = {
    "dna": (b"ACGT", 150, 90, 9, True, 77, b"", 0.0),
    "gap-symbol": (b"ATGC-", 150, 90, 9, True, 79, b"*", 0.005),
    "protein": (PROTEIN, 40, 60, 8, False, 80, b"", 0.0),
}
LONG_W = 12


def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    same = g == o  # also equal infinities (log2 of a zero best score)
    with np.errstate(invalid="ignore"):
        rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(same | (rel <= RTOL)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def new_ctx(tuning=None):
    from gibbssampling_amd import Context
    return Context(0, tuning=tuning)


@pytest.fixture(scope="module")
def other_ctx():
    """The single-chain side: a second context with the shipped defaults."""
    ctx = new_ctx()
    yield ctx
    ctx.close()


_data, _cases = {}, {}


def long_dataset():
    """Four DNA sequences, the first of 12 000 bp: its D table (4 x 12 001 x 4 B = 192 KB)
    does not fit the 160 KB of LDS and goes to HBM."""
    parts = [make_dataset(1, L, LONG_W, b"ACGT", seed=300 + i, mut=0.1)[0]
             for i, L in enumerate((12_000, 50, 137, 200))]
    offsets = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.concatenate(parts), offsets


def data(name):
    if name not in _data:
        if name == "long":
            _data[name] = long_dataset()
        else:
            alpha, N, L, W, ragged, dseed, extra, rate = SHAPES[name]
            _data[name] = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1,
                                       extra=extra, extra_rate=rate)
    return _data[name]


def shape(name):
    if name == "long":
        return b"ACGT", 4, LONG_W, SEEDS[:3]
    alpha, N, _, W = SHAPES[name][:4]
    return alpha, N, W, SEEDS


def case(name, mode):
    """One batch result per (shape, mode), computed once and left unchanged."""
    if (name, mode) not in _cases:
        alpha, N, W, seeds = shape(name)
        codes, offsets = data(name)
        ctx = new_ctx()
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.random_starts_batch(W, PC, seeds, mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[(name, mode)] = out
    return _cases[(name, mode)]


def assert_rows_equal_the_oracle(name, mode, **twin):
    alpha, N, W, seeds = shape(name)
    codes, offsets = data(name)
    score, pos, status = twin.pop("result", None) or case(name, mode)
    assert score.shape == (len(seeds), N) and pos.shape == (len(seeds), N)
    assert not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    for seed in sorted(set(seeds)):
        os_, op = ol.random_starts(S, W, PC, seed=seed, mode=mode, **twin)
        for r in [i for i, s in enumerate(seeds) if s == seed]:
            assert np.array_equal(pos[r], op), (seed, r)
            assert close(score[r], os_), (seed, r)


def assert_rows_equal_the_loop(ctx, W, seeds, mode, score, pos):
    for r, seed in enumerate(seeds):
        ss, sp = ctx.random_starts(W, PC, seed, mode)
        assert np.array_equal(pos[r], sp), (seed, r)
        assert np.array_equal(bits(score[r]), bits(ss)), (seed, r)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_row_equals_the_oracle(name, mode):
    if name == "dna":  # one window only and more windows than a wavefront both occur
        K = np.diff(data(name)[1]) - SHAPES[name][3] + 1
        assert K.min() == 1 and (K > 64).sum() >= 10
    assert_rows_equal_the_oracle(name, mode)
    score, pos, _ = case(name, mode)
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3])
    assert np.array_equal(bits(score[1]), bits(score[3]))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_row_equals_the_single_chain_call(name, mode, other_ctx):
    alpha, N, W, seeds = shape(name)
    other_ctx.set_sequences(*data(name), alpha)
    score, pos, status = case(name, mode)
    assert not status.any()
    assert_rows_equal_the_loop(other_ctx, W, seeds, mode, score, pos)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("N", [5, 12])
def test_more_chains_than_cus_fewer_targets_than_a_wavefront(N, mode, gpu_ctx, other_ctx):
    L, W, R = 30, 5, 300
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=40 + N, mut=0.1)
    seeds = [1000 + 7 * i for i in range(R)]
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    score, pos, status = gpu_ctx.random_starts_batch(W, PC, seeds, mode)
    assert score.shape == (R, N) and not status.any()
    assert_rows_equal_the_loop(other_ctx, W, seeds, mode, score, pos)
    # the seeds reach the chains
    assert len({tuple(row) for row in pos}) > 1


def test_chains_whose_targets_fill_a_launch(gpu_ctx, other_ctx):
    """From 8 targets per CU (2 048 on 256 CUs) mode 0 counts chain after chain with the
    single-chain kernel, each chain into its slab; the scans stay one launch."""
    N, L, W = 2100, 24, 6
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=61, ragged=True, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    seeds = SEEDS[1:4]
    for mode in (0, 1):
        score, pos, status = gpu_ctx.random_starts_batch(W, PC, seeds, mode)
        assert not status.any()
        assert_rows_equal_the_loop(other_ctx, W, seeds, mode, score, pos)
        assert not np.array_equal(pos[0], pos[1])


@pytest.mark.parametrize("mode", [0, 1])
def test_the_d_table_in_hbm(mode, other_ctx):
    alpha, N, W, seeds = shape("long")
    other_ctx.set_sequences(*data("long"), alpha)
    score, pos, status = case("long", mode)
    assert not status.any()
    assert_rows_equal_the_loop(other_ctx, W, seeds, mode, score, pos)
    assert_rows_equal_the_oracle("long", mode)


def pcv49(alpha, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.6, 49)
    v[[c - 42 for c in alpha]] = rng.dirichlet(np.ones(len(alpha)))
    return v


@pytest.mark.parametrize("mode", [0, 1])
def test_the_twins(mode):
    alpha, N, W, seeds = shape("dna")
    ctx = new_ctx()
    ctx.set_sequences(*data("dna"), alpha)
    pcv = pcv49(alpha, 12)
    ctx.set_fixed_pcv(pcv)
    out = ctx.random_starts_batch(W, PC, seeds, mode)
    assert_rows_equal_the_oracle("dna", mode, result=out, pcv49=pcv)
    ctx.set_fixed_pcv(None)
    ppm = np.random.default_rng(13).uniform(0.01, 1.0, (49, W))
    ctx.set_fixed_ppm(ppm, W)
    out = ctx.random_starts_batch(W, PC, seeds, mode)
    assert_rows_equal_the_oracle("dna", mode, result=out, ppm49=ppm)
    # the fixed PPM of another motifLength: refused as by gs_random_starts
    with pytest.raises(ArgumentError):
        ctx.random_starts_batch(W - 1, PC, seeds, mode)
    ctx.close()


def test_edges(other_ctx):
    alpha, N, W, seeds = shape("dna")
    codes, offsets = data("dna")
    ctx = new_ctx()
    ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    # one chain
    for mode in (0, 1):
        score, pos, status = ctx.random_starts_batch(W, PC, [seeds[2]], mode)
        assert score.shape == (1, N) and not status.any()
        assert_rows_equal_the_loop(other_ctx, W, [seeds[2]], mode, score, pos)
    # no chain
    score, pos, status = ctx.random_starts_batch(W, PC, [], 0)
    assert score.shape == (0, N) and pos.shape == (0, N) and status.shape == (0,)
    # no snapshot is left, and the next call runs as on a fresh context
    ctx.random_starts_batch(W, PC, seeds, 1)
    with pytest.raises(GibbsError) as e:
        ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    after = ctx.motif_sampling(W, PC, CUTOFF, 5)
    fresh = other_ctx.motif_sampling(W, PC, CUTOFF, 5)
    assert np.array_equal(after[0], fresh[0]) and after[2] == fresh[2]
    assert np.array_equal(bits(after[1]), bits(fresh[1]))
    ctx.close()


def test_bad_arguments_launch_nothing():
    L, W = 30, 5
    codes, offsets = make_dataset(12, L, W, b"ACGT", seed=52, mut=0.1)
    ctx = new_ctx()
    ctx.set_sequences(codes, offsets, b"ACGT")
    before = ctx.stats()
    with pytest.raises(ArgumentError):
        ctx.random_starts_batch(L + 1, PC, SEEDS, 0)
    with pytest.raises(ArgumentError):
        ctx.random_starts_batch(W, PC, SEEDS, 2)
    assert ctx.stats() == before
    # a shard of the sequences: the chains' counts would need the other ranks
    ctx.set_sequences(codes, offsets, b"ACGT", n_global=20, global_offset=0)
    with pytest.raises(GibbsError) as e:
        ctx.random_starts_batch(W, PC, SEEDS, 0)
    assert e.value.status == _native.GS_E_UNSUPPORTED
    ctx.close()


def same(a, b):
    """Two results of one batched call, bit for bit."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


def same_lists(a, b):
    """(cnt, pos[R, N, cap], pwms, passes, status): list entries only up to cnt."""
    same((a[0], a[2], a[3], a[4]), (b[0], b[2], b[3], b[4]))
    live = np.arange(a[1].shape[2])[None, None, :] < a[0][:, :, None]
    assert np.array_equal(a[1][live], b[1][live])


def test_batch_starts_does_not_change_the_rows():
    alpha, N, W, seeds = shape("dna")
    codes, offsets = data("dna")
    ctxs = [new_ctx({"batch_starts": v}) for v in (0, 1)]
    assert [c.get_tuning("batch_starts") for c in ctxs] == [0.0, 1.0]
    for c in ctxs:
        c.set_sequences(codes, offsets, alpha)
    for mode in (0, 1):
        same(*[c.motif_sampling_batch(W, PC, CUTOFF, seeds, mode) for c in ctxs])
        same(*[c.site_sampling_batch(W, PC, seeds, mode) for c in ctxs])
        same(*[c.motif_run_batch(W, PC, CUTOFF, 4, seeds, init_mode=mode) for c in ctxs])
    # motifAmount 2 on the first 40 sequences
    for c in ctxs:
        c.set_sequences(codes[:offsets[40]], offsets[:41], alpha)
    for mode in (0, 1):
        same_lists(*[c.motif_sampling_multi_batch(2, 6, PC, CUTOFF, seeds, mode) for c in ctxs])
    # the D table in HBM
    alpha, N, W, seeds = shape("long")
    for c in ctxs:
        c.set_sequences(*data("long"), alpha)
    same(*[c.motif_run_batch(W, PC, CUTOFF, 4, seeds, init_mode=0) for c in ctxs])
    for c in ctxs:
        c.close()
