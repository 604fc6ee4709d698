"""GPU parity of gs_motif_run_batch: R independent chains of T synchronous sweeps
(.fs:935-970, motifAmount = 1), one launch a sweep over all (chain, target) pairs.  Every
row against the oracle's composition random_starts -> T x sweep(u of sweep t) for its seed,
and against the sequential entry point gs_motif_run on a second context.  Positions and
statuses are compared exactly, PWMS within 1e-12 relative."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset, uniforms
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC, CUTOFF = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]
T_ORACLE, T_SEQ = 4, 25

# name: (alphabet, N, L, W, ragged, dataset seed)
SHAPES = {
    "dna": (b"ACGT", 150, 90, 9, True, 77),
    "gap-symbol": (b"ATGC-", 150, 90, 9, True, 79),
    "protein": (PROTEIN, 40, 60, 8, False, 80),
}


def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    same = g == o
    rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(same | (rel <= RTOL)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def oracle_chain(S, N, W, seed, pos, T, first=0, u=None):
    """T oracle sweeps from `pos`; the counter RNG's uniforms, or the rows of u."""
    pw = None
    for t in range(T):
        ut = uniforms(seed, ol.stream_sweep(first + t), N) if u is None else u[t]
        pos, pw, _ = ol.sweep(S, W, PC, CUTOFF, pos, ut)
    return pos, pw


@pytest.fixture(scope="module")
def other_ctx():
    """The sequential side: a second context with the shipped defaults."""
    from gibbssampling_amd import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


_data, _cases = {}, {}


def data(name):
    if name not in _data:
        alpha, N, L, W, ragged, dseed = SHAPES[name]
        _data[name] = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
    return _data[name]


def case(name, mode, T):
    """One batch result per (shape, init_mode, sweeps), computed once and left unchanged."""
    if (name, mode, T) not in _cases:
        from gibbssampling_amd import Context
        alpha, N, L, W, _, _ = SHAPES[name]
        codes, offsets = data(name)
        ctx = Context(0)
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_run_batch(W, PC, CUTOFF, T, SEEDS, init_mode=mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[(name, mode, T)] = out
    return _cases[(name, mode, T)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name, mode):
    alpha, N, L, W, _, _ = SHAPES[name]
    codes, offsets = data(name)
    pos, pwms, status = case(name, mode, T_ORACLE)
    assert pos.shape == (len(SEEDS), N) and pwms.shape == (len(SEEDS), N)
    assert not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    kinds = set()
    for seed in sorted(set(SEEDS)):
        _, p0 = ol.random_starts(S, W, PC, seed=seed, mode=mode)
        op, ow = oracle_chain(S, N, W, seed, p0, T_ORACLE)
        kinds |= {bool(x) for x in op >= 0}
        for r in [i for i, s in enumerate(SEEDS) if s == seed]:
            assert np.array_equal(pos[r], op), (seed, r)
            assert close(pwms[r], ow), (seed, r)
    if mode == 1:  # from shared draws: kept motifs and [] entries both occur
        assert kinds == {True, False}
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3])
    assert np.array_equal(bits(pwms[1]), bits(pwms[3]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, gpu_ctx, other_ctx):
    alpha, N, L, W, _, _ = SHAPES[name]
    codes, offsets = data(name)
    pos, pwms, status = case(name, 1, T_SEQ)
    assert not status.any()
    other_ctx.set_sequences(codes, offsets, alpha)
    starts = []
    for r, seed in enumerate(SEEDS):
        _, p0 = other_ctx.random_starts(W, PC, seed, 1)
        starts.append(p0)
        sp, sw = other_ctx.motif_run(W, PC, CUTOFF, T_SEQ, seed, p0)
        assert np.array_equal(pos[r], sp), (seed, r)
        assert close(pwms[r], sw), (seed, r)
    # 10 sweeps, then 15 more from their positions: the same chains, the same PWMS bits
    gpu_ctx.set_sequences(codes, offsets, alpha)
    p10, _, st = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 10, SEEDS, init_mode=1)
    assert not st.any()
    p25, w25, st = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 15, SEEDS, pos=p10, first_sweep=10)
    assert not st.any()
    assert np.array_equal(p25, pos)
    assert np.array_equal(bits(w25), bits(pwms))
    # ... and so do uploaded starts
    pu, wu, st = gpu_ctx.motif_run_batch(W, PC, CUTOFF, T_SEQ, SEEDS, pos=np.array(starts))
    assert not st.any()
    assert np.array_equal(pu, pos) and np.array_equal(bits(wu), bits(pwms))


@pytest.mark.parametrize("clear,blocks", [(0, 1), (0, 32), (1, 1), (1, 8)])
def test_launch_choices_do_not_change_the_rows(clear, blocks):
    """The next aggregate rows zeroed by a memset or in-kernel, few or many workgroups
    a CU: the same chains, bit for bit (11 sweeps: every rotation of the three rows)."""
    from gibbssampling_amd import Context
    alpha, N, L, W, _, _ = SHAPES["gap-symbol"]
    codes, offsets = data("gap-symbol")
    pos, pwms, status = case("gap-symbol", 1, 11)
    ctx = Context(0, tuning={"run_batch_clear": clear, "run_batch_blocks": blocks})
    ctx.set_sequences(codes, offsets, alpha)
    p, w, st = ctx.motif_run_batch(W, PC, CUTOFF, 11, SEEDS, init_mode=1)
    ctx.close()
    assert not st.any() and not status.any()
    assert np.array_equal(p, pos) and np.array_equal(bits(w), bits(pwms))


def test_all_background_chains(gpu_ctx, other_ctx):
    alpha, N, L, W, _, _ = SHAPES["dna"]
    codes, offsets = data("dna")
    S = ol.Seqs(codes, offsets, alpha)
    p0 = init_positions(offsets, 9, 3, 0.1)
    starts = np.tile(p0, (len(SEEDS), 1))
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 4, SEEDS, pos=starts)
    assert not status.any()
    for r, seed in enumerate(SEEDS):
        op = p0
        kept = []
        for t in range(4):
            op, ow, _ = ol.sweep(S, W, PC, CUTOFF, op, uniforms(seed, ol.stream_sweep(t), N))
            kept.append(int((op >= 0).sum()))
        assert kept[1:] == [0, 0, 0], (seed, kept)  # sweeps 2 onward see every list empty
        assert np.array_equal(pos[r], op), (seed, r)
        assert close(pwms[r], ow), (seed, r)
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 12, SEEDS, pos=starts)
    assert not status.any()
    for r, seed in enumerate(SEEDS):
        sp, sw = other_ctx.motif_run(W, PC, CUTOFF, 12, seed, p0)
        assert np.array_equal(pos[r], sp), (seed, r)
        assert close(pwms[r], sw), (seed, r)


@pytest.mark.parametrize("N", [5, 12])
def test_more_pairs_than_the_grid_fewer_targets_than_a_wavefront(N, gpu_ctx, other_ctx):
    L, W, R, T = 30, 5, 300, 8
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=90 + N, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    seeds = [7000 + 3 * r for r in range(R)]
    p0 = init_positions(offsets, W, 5)
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, T, seeds, pos=np.tile(p0, (R, 1)))
    assert not status.any()
    for r, seed in enumerate(seeds):
        sp, sw = other_ctx.motif_run(W, PC, CUTOFF, T, seed, p0)
        assert np.array_equal(pos[r], sp), (seed, r)
        assert close(pwms[r], sw), (seed, r)
    assert len({p.tobytes() for p in pos}) > 1  # the seeds reach the chains


def test_explicit_uniforms_and_error_isolation(gpu_ctx):
    from gibbssampling_amd import RouletteOverrunError
    R, T, N, W = 3, 3, 30, 6
    codes, offsets = make_dataset(N, 40, W, seed=51)
    p0 = init_positions(offsets, W, 52)
    u = np.random.default_rng(53).random((R, T, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    starts = np.tile(p0, (R, 1))
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, T, [1, 2, 3], pos=starts, u=u)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    with pytest.raises(RouletteOverrunError) as ei:
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, T, [1, 2, 3], pos=starts, u=u, strict=True)
    assert ei.value.index == 7
    S = ol.Seqs(codes, offsets, b"ACGT")
    for r in (0, 2):
        op, ow = oracle_chain(S, N, W, 0, p0, T, u=u[r])
        assert np.array_equal(pos[r], op) and close(pwms[r], ow), r
    p1, _ = oracle_chain(S, N, W, 0, p0, 1, u=u[1])
    with pytest.raises(ol.OracleError):
        ol.sweep(S, W, PC, CUTOFF, p1, u[1, 1])


def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = data("protein")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    p0 = init_positions(offsets, W, 9, 0.2)
    want = other_ctx.motif_run(W, PC, CUTOFF, 6, 31, p0)
    fresh = other_ctx.motif_sampling(W, PC, CUTOFF, 31)

    # one chain is gs_motif_run
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 6, [31], pos=p0[None, :])
    assert pos.shape == (1, N) and status[0] == 0
    assert np.array_equal(pos[0], want[0]) and close(pwms[0], want[1])
    # no snapshot is left behind
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    # ... and the next single run behaves as on a fresh context
    again = gpu_ctx.motif_sampling(W, PC, CUTOFF, 31)
    assert np.array_equal(again[0], fresh[0]) and again[2] == fresh[2]
    assert np.array_equal(bits(again[1]), bits(fresh[1]))
    # the same after a call that ran the starts on the context's own state
    gpu_ctx.motif_run_batch(W, PC, CUTOFF, 2, [5, 6], init_mode=1)
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    again = gpu_ctx.motif_sampling(W, PC, CUTOFF, 31)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(bits(again[1]), bits(fresh[1]))

    # no sweeps: the positions stay as given; the starts come back for init_mode 0 / 1
    pos, _, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 0, [31, 32], pos=np.tile(p0, (2, 1)))
    assert np.array_equal(pos, np.tile(p0, (2, 1))) and not status.any()
    pos, _, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 0, [31], init_mode=1)
    assert np.array_equal(pos[0], other_ctx.random_starts(W, PC, 31, 1)[1])

    # no chains: nothing to do
    pos, pwms, status = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [])
    assert pos.shape == (0, N) and pwms.shape == (0, N) and status.shape == (0,)

    # argument errors before any launch
    before = gpu_ctx.stats()
    two = np.tile(p0, (2, 1))
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_run_batch(L + 1, PC, CUTOFF, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [1, 2], init_mode=2)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, -1, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [1, 2], pos=two, first_sweep=-1)
    bad = two.copy()
    bad[1, 4] = L - W + 1
    with pytest.raises(_native.ArgumentError) as e:
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [1, 2], pos=bad)
    assert e.value.index == 4
    bad[1, 4] = -2
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [1, 2], pos=bad)
    assert gpu_ctx.stats() == before

    # the ByPCV twin is not batched
    gpu_ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            gpu_ctx.motif_run_batch(W, PC, CUTOFF, 3, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        gpu_ctx.set_fixed_pcv(None)


def test_mirror_runs_the_chains_of_runSweeps():
    from gibbssampling_amd import MotifSampler
    from gibbssampling_amd.sampler import createMotifIndex
    N, L, W, T = 40, 60, 7, 6
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    seeds = [99, 100, 2**40 + 1]
    mems = [[createMotifIndex(0.0, [] if p < 0 else [p])
             for p in init_positions(offsets, W, 20 + r, 0.1)] for r in range(len(seeds))]
    batch = MotifSampler.runSweepsBatched(W, PC, CUTOFF, "ACGT", sources, T, seeds, mems,
                                          first_sweep=3)
    assert len(batch) == len(seeds)
    for r, seed in enumerate(seeds):
        loop = MotifSampler.runSweeps(W, PC, CUTOFF, "ACGT", sources, mems[r], T, seed,
                                      first_sweep=3)
        assert [m.Positions for m in batch[r]] == [m.Positions for m in loop]
        assert close([m.PWMS for m in batch[r]], [m.PWMS for m in loop])
