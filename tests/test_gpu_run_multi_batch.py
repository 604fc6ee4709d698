"""GPU parity of gs_motif_run_multi_batch: R independent chains of T synchronous sweeps
(.fs:935-970) with Positions lists (any motifAmount), one launch a sweep over all (chain,
target) pairs and, from motifAmount 3 on, a second small one for the pairs whose combinations
overflowed the first arena.  Every row against the oracle's composition random_starts ->
one-position lists -> T x sweep_lists(u of sweep t) for its seed, and against a loop of the
sequential entry point gs_motif_sweep_multi on a second context.

Bar against the oracle: list lengths and positions in cons order identical, PWMS within
1e-12 relative (log() may differ in the last ulp between the device library and glibc).
Against gs_motif_sweep_multi: lists identical, PWMS bit-identical (the same device functions
in the same operation order; the aggregates are integers)."""
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import init_positions, make_dataset, uniforms
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC = 1e-4
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
GOLDEN = Path(__file__).resolve().parent / "golden"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]
T_ORACLE = 4

# name: (alphabet, N, L, W, ragged, M, cut-off, init_mode, dataset seed): the shapes of
# test_gpu_multi_batch.py
SHAPES = {
    "dna-m2": (b"ACGT", 60, 60, 6, True, 2, 1.0, 0, 77),
    "dna-m3-shared": (b"ACGT", 60, 60, 6, True, 3, 1.0, 1, 78),
    "gap-m2": (b"ATGC-", 50, 70, 5, True, 2, 0.5, 0, 79),
    "protein-m2": (PROTEIN, 30, 60, 8, False, 2, 1.0, 0, 80),
    "m4": (b"ATGC-", 30, 60, 4, False, 4, 2.0, 0, 81),
    "neg-cutoff": (b"ACGT", 25, 40, 6, True, 2, -3.0, 0, 6),
}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def one_lists(p, cap):
    """Start positions as one-position lists."""
    lst = np.full((len(p), cap), -1, np.int32)
    lst[:, 0] = p
    return np.ones(len(p), np.int32), lst


def oracle_chain(S, M, W, cutoff, seed, cnt, pos, T, first=0, u=None, cap=None):
    """T oracle sweeps from the lists; the counter RNG's uniforms, or the rows of u."""
    pw = None
    for t in range(T):
        ut = uniforms(seed, ol.stream_sweep(first + t), S.n) if u is None else u[t]
        cnt, pos, pw = ol.sweep_lists(S, M, W, PC, cutoff, cnt, pos, cap or M, ut)
    return cnt, pos, pw


def check_oracle(g, o, what):
    """(cnt, pos, pwms) of one chain against the oracle's: no target left out."""
    gc, gp, gw = g
    oc, op, ow = o
    assert np.array_equal(gc, oc), what
    for n in range(len(gc)):
        assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), (what, n)
    rel = np.abs(gw - ow) / np.maximum(np.abs(ow), 1e-300)
    assert np.all((gw == ow) | (rel <= RTOL)), (what, float(np.nanmax(rel)))


def check_sequential(g, s, what):
    """(cnt, pos, pwms) of one chain against the loop of gs_motif_sweep_multi's."""
    gc, gp, gw = g
    sc, sp, sw = s
    assert np.array_equal(gc, sc), what
    assert np.array_equal(gp, sp), what  # entries past cnt are -1 on both sides
    assert np.array_equal(bits(gw), bits(sw)), what


def sequential_chain(ctx, M, W, cutoff, seed, cnt, pos, T, first=0, cap=None):
    pw = None
    for t in range(T):
        u = uniforms(seed, ol.stream_sweep(first + t), len(cnt))
        cnt, pos, pw = ctx.motif_sweep_multi(M, W, PC, cutoff, cnt, pos, u, cap)
    return cnt, pos, pw


def row(out, r):
    return out[0][r], out[1][r], out[2][r]


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
        alpha, N, L, W, ragged, _, _, _, dseed = SHAPES[name]
        _data[name] = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
    return _data[name]


def case(name, T):
    """One batch result per (shape, sweeps), computed once and left unchanged."""
    if (name, T) not in _cases:
        from gibbssampling_amd import Context
        alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
        codes, offsets = data(name)
        ctx = Context(0)
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_run_multi_batch(M, W, PC, cutoff, T, SEEDS, init_mode=mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[(name, T)] = out
    return _cases[(name, T)]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    cnt, pos, pwms, status = out = case(name, T_ORACLE)
    R = len(SEEDS)
    assert cnt.shape == (R, N) and pos.shape == (R, N, M) and pwms.shape == (R, N)
    assert status.shape == (R,) and not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    for seed in sorted(set(SEEDS)):
        _, p0 = ol.random_starts(S, W, PC, seed=seed, mode=mode)
        o = oracle_chain(S, M, W, cutoff, seed, *one_lists(p0, M), T_ORACLE)
        for r in [i for i, s in enumerate(SEEDS) if s == seed]:
            check_oracle(row(out, r), o, (name, seed, r))
    # entries past cnt are -1
    assert np.all(np.where(np.arange(M)[None, None, :] >= cnt[:, :, None], pos, -1) == -1)
    # the duplicate seed: identical rows
    assert np.array_equal(cnt[1], cnt[3]) and np.array_equal(pos[1], pos[3])
    assert np.array_equal(bits(pwms[1]), bits(pwms[3]))
    if name == "m4":  # seed 12: every list empty from sweep 0 on, the absorbing state
        assert not cnt[SEEDS.index(12)].any()
        assert all(cnt[r].any() for r, s in enumerate(SEEDS) if s != 12)


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, other_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    out = case(name, T_ORACLE)
    other_ctx.set_sequences(codes, offsets, alpha)
    for r, seed in enumerate(SEEDS):
        _, p0 = other_ctx.random_starts(W, PC, seed, mode)
        s = sequential_chain(other_ctx, M, W, cutoff, seed, *one_lists(p0, M), T_ORACLE)
        check_sequential(row(out, r), s, (name, seed, r))


@pytest.mark.parametrize("name", ["dna-m2", "dna-m3-shared"])
def test_the_starts_chain_after_chain_give_the_same_rows(name):
    """batch_starts 0 (what the drivers do from 2 048 sequences on): the starts of init_mode 0
    / 1 on the context's single-chain state, the same chains bit for bit."""
    from gibbssampling_amd import Context
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    cnt, pos, pwms, status = case(name, T_ORACLE)
    ctx = Context(0, tuning={"batch_starts": 0})
    ctx.set_sequences(codes, offsets, alpha)
    c, p, w, st = ctx.motif_run_multi_batch(M, W, PC, cutoff, T_ORACLE, SEEDS, init_mode=mode)
    ctx.close()
    assert not st.any() and not status.any()
    assert np.array_equal(c, cnt) and np.array_equal(p, pos)
    assert np.array_equal(bits(w), bits(pwms))


@pytest.mark.parametrize("name", ["dna-m2", "dna-m3-shared"])
def test_continuation(name, gpu_ctx):
    """10 sweeps, then 15 more from their lists: the chains of 25 sweeps, the same PWMS bits;
    and so do uploaded starts."""
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    cnt, pos, pwms, status = case(name, 25)
    assert not status.any()
    gpu_ctx.set_sequences(codes, offsets, alpha)
    c10, p10, _, st = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 10, SEEDS, init_mode=mode)
    assert not st.any()
    c25, p25, w25, st = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 15, SEEDS, c10, p10,
                                                      first_sweep=10)
    assert not st.any()
    assert np.array_equal(c25, cnt) and np.array_equal(p25, pos)
    assert np.array_equal(bits(w25), bits(pwms))
    c0, p0, _, st = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 0, SEEDS, init_mode=mode)
    cu, pu, wu, st = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 25, SEEDS, c0, p0)
    assert not st.any()
    assert np.array_equal(cu, cnt) and np.array_equal(pu, pos)
    assert np.array_equal(bits(wu), bits(pwms))


def test_overflow_on_the_device(gpu_ctx):
    """Every window and every pair passes (cut-off -1000): each target needs 119 + 116 * 117
    / 2 = 6 905 arena entries, above the first arena (2 048) and below the overflow launch's
    (32 768): every pair is rescored on the device, no chain parks."""
    N, L, W, M, cutoff, T = 12, 120, 2, 3, -1000.0, 3
    seeds = [7, 8, 9, 10]
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    S = ol.Seqs(codes, offsets, b"ACGT")
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, T, seeds)
    assert not out[3].any()
    info = gpu_ctx.run_multi_batch_last_info()
    assert info["rescored"] > 0 and info["parked"] == 0 and info["resume_rounds"] == 0
    assert info["arena"] == 2048
    for r, seed in enumerate(seeds):
        _, p0 = ol.random_starts(S, W, PC, seed=seed, mode=0)
        o = oracle_chain(S, M, W, cutoff, seed, *one_lists(p0, M), T)
        check_oracle(row(out, r), o, (seed, r))


def test_parking_and_resuming(gpu_ctx):
    """Each target needs 263 + 260 * 261 / 2 = 34 193 arena entries, above the overflow
    launch's 32 768: both chains park in sweep 0 and are run again with larger arenas."""
    N, L, W, M, cutoff, T = 4, 264, 2, 3, -1000.0, 2
    seeds = [7, 8]
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    S = ol.Seqs(codes, offsets, b"ACGT")
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, T, seeds)
    assert not out[3].any()
    info = gpu_ctx.run_multi_batch_last_info()
    assert info["parked"] == 2 and info["resume_rounds"] >= 1
    for r, seed in enumerate(seeds):
        _, p0 = ol.random_starts(S, W, PC, seed=seed, mode=0)
        o = oracle_chain(S, M, W, cutoff, seed, *one_lists(p0, M), T)
        check_oracle(row(out, r), o, (seed, r))


def test_amount_one_through_the_list_chains(gpu_ctx):
    """motifAmount = 1: the list chains' rows are motif_run_batch's (the `dna` shape of
    test_gpu_run_batch.py)."""
    N, L, W, T = 150, 90, 9, 4
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=77, ragged=True, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    for mode in (0, 1):
        cnt, pos, pwms, status = gpu_ctx.motif_run_multi_batch(1, W, PC, 1.0, T, SEEDS,
                                                               init_mode=mode)
        spos, spwms, sstatus = gpu_ctx.motif_run_batch(W, PC, 1.0, T, SEEDS, init_mode=mode)
        assert not status.any() and not sstatus.any()
        assert pos.shape == (len(SEEDS), N, 1)
        assert np.array_equal(cnt, (spos >= 0).astype(np.int32))
        assert np.array_equal(pos[:, :, 0], spos)
        # the same device functions on the same integer aggregates: the same bits
        assert np.array_equal(bits(pwms), bits(spwms))


def test_explicit_uniforms_and_error_isolation(gpu_ctx):
    from gibbssampling_amd import RouletteOverrunError
    R, T, N, W, M = 3, 3, 30, 6, 2
    codes, offsets = make_dataset(N, 40, W, seed=51)
    cnt0, pos0 = one_lists(init_positions(offsets, W, 52), M)
    u = np.random.default_rng(53).random((R, T, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    cnts, poss = np.tile(cnt0, (R, 1)), np.tile(pos0, (R, 1, 1))
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, 1.0, T, [1, 2, 3], cnts, poss, u=u)
    assert out[3].tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    with pytest.raises(RouletteOverrunError) as ei:
        gpu_ctx.motif_run_multi_batch(M, W, PC, 1.0, T, [1, 2, 3], cnts, poss, u=u, strict=True)
    assert ei.value.index == 7
    S = ol.Seqs(codes, offsets, b"ACGT")
    for r in (0, 2):
        check_oracle(row(out, r), oracle_chain(S, M, W, 1.0, 0, cnt0, pos0, T, u=u[r]), r)
    c1, p1, _ = oracle_chain(S, M, W, 1.0, 0, cnt0, pos0, 1, u=u[1])
    with pytest.raises(ol.OracleError):
        ol.sweep_lists(S, M, W, PC, 1.0, c1, p1, M, u[1, 1])


def fsx_set():
    seqs = json.loads((GOLDEN / "fsx_sets.json").read_text())["bioTestsWithMultipleSamples"]["seqs"]
    codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
    offsets = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return seqs, codes, offsets


def test_more_chains_than_cus_fewer_targets_than_a_wavefront(gpu_ctx, other_ctx):
    """The .fsx:407 data set (N = 5, L = 27, W = 6, motifAmount 2), 300 chains of 5 sweeps."""
    seqs, codes, offsets = fsx_set()
    alpha, W, M, R, T = b"ATGC-", 6, 2, 300, 5
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    seeds = [7000 + 3 * r for r in range(R)]
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, 1.0, T, seeds)
    assert not out[3].any()
    for r in range(0, R, 23):
        _, p0 = other_ctx.random_starts(W, PC, seeds[r], 0)
        s = sequential_chain(other_ctx, M, W, 1.0, seeds[r], *one_lists(p0, M), T)
        check_sequential(row(out, r), s, (seeds[r], r))
    assert len({(c.tobytes(), p.tobytes()) for c, p in zip(out[0], out[1])}) > 1


def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES["protein-m2"]
    codes, offsets = data("protein-m2")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    fresh = other_ctx.motif_sampling_multi(M, W, PC, cutoff, 31)
    cnt0, pos0 = one_lists(init_positions(offsets, W, 9), M)
    pos0[3, 1], cnt0[3] = 0 if pos0[3, 0] > W else L - W, 2  # one two-position list
    cnt0[5] = 0  # and one Positions []

    # one chain is gs_motif_run_multi, and a loop of gs_motif_sweep_multi
    want = sequential_chain(other_ctx, M, W, cutoff, 31, cnt0, pos0, 6)
    got = gpu_ctx.motif_run_multi(M, W, PC, cutoff, 6, 31, cnt0, pos0)
    check_sequential(got, want, "one chain")
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 6, [31], cnt0[None], pos0[None])
    assert out[0].shape == (1, N) and out[1].shape == (1, N, M) and out[3][0] == 0
    check_sequential(row(out, 0), want, "a batch of one")
    ms = gpu_ctx.run_multi_batch_last_ms()
    assert len(ms) == 2 and all(np.isfinite(m) and m >= 0.0 for m in ms)
    # no snapshot is left behind
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    # ... and the next single run behaves as on a fresh context
    again = gpu_ctx.motif_sampling_multi(M, W, PC, cutoff, 31)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(bits(again[2]), bits(fresh[2]))
    # the same after a call that ran the starts on the context's own state
    gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 2, [5, 6], init_mode=1)
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    again = gpu_ctx.motif_sampling_multi(M, W, PC, cutoff, 31)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(bits(again[2]), bits(fresh[2]))

    # lists longer than motifAmount, up to the capacity
    c3, p3 = one_lists(init_positions(offsets, W, 9), 3)
    p3[2], c3[2] = [L - W, (L - W) // 2, 0], 3
    want3 = sequential_chain(other_ctx, M, W, cutoff, 31, c3, p3, 3, cap=3)
    out = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 3, [31, 32], np.tile(c3, (2, 1)),
                                        np.tile(p3, (2, 1, 1)), cap=3)
    assert out[1].shape == (2, N, 3) and not out[3].any()
    check_sequential(row(out, 0), want3, "cap 3")

    # no sweeps: the lists stay as given; the starts come back for init_mode 0 / 1
    two_c, two_p = np.tile(cnt0, (2, 1)), np.tile(pos0, (2, 1, 1))
    c, p, _, status = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 0, [31, 32], two_c, two_p)
    assert np.array_equal(c, two_c) and np.array_equal(p, two_p) and not status.any()
    for m in (0, 1):
        c, p, _, status = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 0, [31], init_mode=m)
        assert (c == 1).all() and (p[0, :, 1:] == -1).all() and not status.any()
        assert np.array_equal(p[0, :, 0], other_ctx.random_starts(W, PC, 31, m)[1])

    # no chains: nothing to do
    for kw in ({}, {"init_mode": 1}):
        c, p, w, status = gpu_ctx.motif_run_multi_batch(M, W, PC, cutoff, 3, [], **kw)
        assert c.shape == (0, N) and p.shape == (0, N, M) and w.shape == (0, N)
        assert status.shape == (0,)

    # argument errors before any launch
    before = gpu_ctx.stats()
    run = gpu_ctx.motif_run_multi_batch
    with pytest.raises(_native.ArgumentError):
        run(M, L + 1, PC, cutoff, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], init_mode=2)
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, -1, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], two_c, two_p, first_sweep=-1)
    with pytest.raises(_native.ArgumentError):
        run(17, W, PC, cutoff, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(0, W, PC, cutoff, 3, [1, 2], cap=1)
    with pytest.raises(_native.ArgumentError):
        run(3, W, PC, cutoff, 3, [1, 2], cap=2)
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], cap=17)
    bad = two_p.copy()
    bad[1, 4, 0] = L - W + 1
    with pytest.raises(_native.ArgumentError) as e:
        run(M, W, PC, cutoff, 3, [1, 2], two_c, bad)
    assert e.value.index == 4
    bad[1, 4, 0] = -1
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], two_c, bad)
    badc = two_c.copy()
    badc[0, 2] = M + 1
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], badc, two_p)
    badc[0, 2] = -1
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, 3, [1, 2], badc, two_p)

    # the ByPCV twin is not batched
    gpu_ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            run(M, W, PC, cutoff, 3, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        gpu_ctx.set_fixed_pcv(None)
    assert gpu_ctx.stats() == before
    # the context is usable afterwards
    check_sequential(gpu_ctx.motif_run_multi(M, W, PC, cutoff, 6, 31, cnt0, pos0), want, "after")


def test_null_pointers_are_argument_errors(gpu_ctx):
    """A null seeds or a null output: GS_E_ARG before any launch (the wrapper always passes
    them, so the library is called directly)."""
    alpha, N, L, W, _, M, cutoff, _, _ = SHAPES["protein-m2"]
    codes, offsets = data("protein-m2")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    lib, h, ptr = gpu_ctx.lib, gpu_ctx.h, _native._ptr
    seeds = np.array([1, 2], np.uint64)
    cnt, pos = np.zeros((2, N), np.int32), np.full((2, N, M), -1, np.int32)
    pwms, status = np.zeros((2, N)), np.zeros(2, np.int32)

    def batch(s, c, p, w):
        return lib.gs_motif_run_multi_batch(h, M, W, PC, cutoff, 3, ptr(s), 2, 0, 0, M, None,
                                            ptr(c), ptr(p), ptr(w), ptr(status))

    def one(c, p, w):
        return lib.gs_motif_run_multi(h, M, W, PC, cutoff, 3, 1, 0, M, ptr(c), ptr(p), ptr(w))

    before = gpu_ctx.stats()
    assert batch(None, cnt, pos, pwms) == _native.GS_E_ARG
    assert batch(seeds, None, pos, pwms) == _native.GS_E_ARG
    assert batch(seeds, cnt, None, pwms) == _native.GS_E_ARG
    assert batch(seeds, cnt, pos, None) == _native.GS_E_ARG
    assert one(None, pos[0], pwms[0]) == _native.GS_E_ARG
    assert one(cnt[0], None, pwms[0]) == _native.GS_E_ARG
    assert one(cnt[0], pos[0], None) == _native.GS_E_ARG
    assert lib.gs_motif_run_multi_batch(None, M, W, PC, cutoff, 3, ptr(seeds), 2, 0, 0, M, None,
                                        ptr(cnt), ptr(pos), ptr(pwms), None) == _native.GS_E_ARG
    assert gpu_ctx.stats() == before
    # the same call with every pointer, and a null status_out, runs
    assert batch(seeds, cnt, pos, pwms) == _native.GS_OK and not status.any()
    assert lib.gs_motif_run_multi_batch(h, M, W, PC, cutoff, 3, ptr(seeds), 2, 0, 0, M, None,
                                        ptr(cnt), ptr(pos), ptr(pwms), None) == _native.GS_OK


def test_unsupported_calls_launch_nothing():
    """Sharded sequences, slabs beyond 4 GiB and sequences too long for the list path's LDS
    carve: GS_E_UNSUPPORTED, nothing launched, the context usable afterwards."""
    from gibbssampling_amd import Context
    alpha, N, L, W, _, M, cutoff, _, _ = SHAPES["dna-m3-shared"]
    codes, offsets = data("dna-m3-shared")
    ctx = Context(0)
    ctx.set_sequences(codes, offsets, alpha)
    want = ctx.motif_run_multi_batch(M, W, PC, cutoff, 2, [1, 2], init_mode=1)

    def refused(*args, **kw):
        before = ctx.stats()
        with pytest.raises(_native.GibbsError) as e:
            ctx.motif_run_multi_batch(*args, **kw)
        assert e.value.status == _native.GS_E_UNSUPPORTED
        assert ctx.stats() == before

    # the per-sweep overflow counts of 2^30 sweeps alone pass the 4 GiB a batch may hold
    refused(M, W, PC, cutoff, 2**30, [1, 2], init_mode=1)
    # a shard of the sequences: a chain's aggregates would need the other ranks
    ctx.set_sequences(codes, offsets, alpha, n_global=N + 8, global_offset=0)
    refused(M, W, PC, cutoff, 2, [1, 2], init_mode=1)
    cnt0, pos0 = one_lists(np.zeros(N, np.int32), M)
    refused(M, W, PC, cutoff, 2, [1, 2], np.tile(cnt0, (2, 1)), np.tile(pos0, (2, 1, 1)))
    # one sequence of 200 000 symbols: its staging alone passes the LDS of a workgroup
    rng = np.random.default_rng(3)
    long_codes = np.frombuffer(alpha, np.uint8)[rng.integers(0, 4, 200_000 + 2 * 50)]
    ctx.set_sequences(long_codes, np.array([0, 200_000, 200_050, 200_100], np.int64), alpha)
    refused(M, W, PC, cutoff, 2, [1, 2], init_mode=1)
    refused(2, W, PC, cutoff, 2, [1, 2], np.ones((2, 3), np.int32), np.zeros((2, 3, 2), np.int32))
    # the context goes on
    ctx.set_sequences(codes, offsets, alpha)
    again = ctx.motif_run_multi_batch(M, W, PC, cutoff, 2, [1, 2], init_mode=1)
    ctx.close()
    assert all(np.array_equal(a, b) for a, b in zip(again[:2], want[:2]))
    assert np.array_equal(bits(again[2]), bits(want[2])) and not again[3].any()


def test_a_chain_beyond_the_last_arena_is_given_up_alone():
    """The tuning field run_multi_arena_max (default 2^28 categories) lowered to the overflow
    launch's 32 768, so that the branch is reached with small arenas.  Chain 1's lists hold,
    in every sequence, each symbol at both motif columns: with any three of them as the
    others every cell of the profile is counted, so with pc 1e-4 every window has S >= (1 /
    3.0004)^2 and every pair of windows a product >= 0.0123, log2 >= -6.4: at cut-off -10 all
    pass, 263 + 260 * 261 / 2 = 34 193 arena entries a target.  The chain parks in sweep 0,
    the next arena size would pass the limit, and it gets GS_E_UNSUPPORTED in its own status
    entry.  Chain 0 starts from empty lists: every cell is pc / 3.0004, S about 1.8e-8, log2
    about -26 < -10, no window passes, its targets need no arena entry and it finishes."""
    from gibbssampling_amd import Context
    N, L, W, M, cap, cutoff, T = 4, 264, 2, 3, 8, -10.0, 2
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    cnt = np.zeros((2, N), np.int32)
    pos = np.full((2, N, cap), -1, np.int32)
    for n in range(N):
        s = codes[offsets[n]:offsets[n + 1]]
        first = [int(np.nonzero(s[:L - 1] == a)[0][0]) for a in b"ACGT"]       # a at column 0
        second = [int(np.nonzero(s[1:] == a)[0][0]) for a in b"ACGT"]          # a at column 1
        pos[1, n], cnt[1, n] = first + second, cap
    ctx = Context(0, tuning={"run_multi_arena_max": 32768})
    assert ctx.get_tuning("run_multi_arena_max") == 32768.0
    ctx.set_sequences(codes, offsets, b"ACGT")
    c, p, w, status = ctx.motif_run_multi_batch(M, W, PC, cutoff, T, [7, 8], cnt, pos, cap=cap)
    info = ctx.run_multi_batch_last_info()
    assert status.tolist() == [0, _native.GS_E_UNSUPPORTED]
    assert info["parked"] == 1 and info["resume_rounds"] == 0 and info["rescored"] == N
    assert not c[0].any() and (p[0] == -1).all() and np.all(np.isfinite(w[0]) & (w[0] > 0))
    with pytest.raises(_native.GibbsError) as e:
        ctx.motif_run_multi_batch(M, W, PC, cutoff, T, [7, 8], cnt, pos, cap=cap, strict=True)
    assert e.value.status == _native.GS_E_UNSUPPORTED
    # with the default limit the same call resumes the chain and finishes it
    ctx.close()
    ctx = Context(0)
    assert ctx.get_tuning("run_multi_arena_max") == 2.0**28
    ctx.set_sequences(codes, offsets, b"ACGT")
    c2, p2, w2, status = ctx.motif_run_multi_batch(M, W, PC, cutoff, T, [7, 8], cnt, pos, cap=cap)
    info = ctx.run_multi_batch_last_info()
    ctx.close()
    assert not status.any() and info["parked"] == 1 and info["resume_rounds"] == 1
    assert np.array_equal(c2[0], c[0]) and np.array_equal(bits(w2[0]), bits(w[0]))


def test_mirror_runs_the_chains_of_runSweeps():
    from gibbssampling_amd import MotifSampler
    from gibbssampling_amd.sampler import createMotifIndex
    N, L, W, T = 40, 60, 7, 6
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    seeds = [99, 100, 2**40 + 1]
    mems = [[createMotifIndex(0.0, [] if p < 0 else [p])
             for p in init_positions(offsets, W, 20 + r, 0.1)] for r in range(len(seeds))]
    mems[1][0] = createMotifIndex(0.0, [L - W, 0])
    batch = MotifSampler.runSweepsBatched(W, PC, 1.0, "ACGT", sources, T, seeds, mems,
                                          first_sweep=3, motifAmount=2)
    assert len(batch) == len(seeds)
    for r, seed in enumerate(seeds):
        loop = MotifSampler.runSweeps(W, PC, 1.0, "ACGT", sources, mems[r], T, seed,
                                      first_sweep=3, motifAmount=2)
        assert [m.Positions for m in batch[r]] == [m.Positions for m in loop]
        assert [m.PWMS for m in batch[r]] == [m.PWMS for m in loop]
    assert any(len(m.Positions) == 2 for chain in batch for m in chain)
