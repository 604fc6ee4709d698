"""GPU parity of gs_motif_sampling_multi_batch: R independent doMotifSampling chains
(.fs:1034-1038) with Positions lists (any motifAmount), sweep 0 over all (chain, target)
pairs at once and the greedy passes as speculative steps for all chains.  Every row against
the oracle's composition random_starts -> lists -> sweep_lists (uniforms of sweep 0) ->
greedy_lists for its seed, and against the sequential entry point gs_motif_sampling_multi on
a second context.

Bar against the oracle: list lengths, positions in cons order and pass counts identical,
PWMS within 1e-12 relative (log() may differ in the last ulp between the device library and
glibc).  Against gs_motif_sampling_multi: lengths, positions[:cnt] and passes equal and the
PWMS bit-identical: the same device functions in the same operation order with the same
multi_greedy_threads."""
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import make_dataset
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC = 1e-4
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
GOLDEN = Path(__file__).resolve().parent / "golden"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]

# name: (alphabet, N, L, W, ragged, M, cut-off, init_mode, dataset seed,
#        oracle passes of seeds 12, 77, 1001, 5e9+7)
SHAPES = {
    "dna-m2": (b"ACGT", 60, 60, 6, True, 2, 1.0, 0, 77, (4, 4, 4, 4)),
    "dna-m3-shared": (b"ACGT", 60, 60, 6, True, 3, 1.0, 1, 78, (6, 4, 5, 5)),
    "gap-m2": (b"ATGC-", 50, 70, 5, True, 2, 0.5, 0, 79, (3, 3, 3, 3)),
    "protein-m2": (PROTEIN, 30, 60, 8, False, 2, 1.0, 0, 80, (4, 2, 3, 4)),
    "m4": (b"ATGC-", 30, 60, 4, False, 4, 2.0, 0, 81, (1, 4, 4, 5)),
    "neg-cutoff": (b"ACGT", 25, 40, 6, True, 2, -3.0, 0, 6, (4, 5, 5, 3)),
}
PASS_SEEDS = (12, 77, 1001, 5_000_000_007)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_oracle(g, o, what):
    """(cnt, pos, pwms, passes) of one chain against the oracle's."""
    gc, gp, gw, gpass = g
    oc, op, ow, opass = o
    assert np.array_equal(gc, oc), what
    for n in range(len(gc)):
        assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), (what, n)
    rel = np.abs(gw - ow) / np.maximum(np.abs(ow), 1e-300)
    assert np.all((gw == ow) | (rel <= RTOL)), (what, float(np.nanmax(rel)))
    assert gpass == opass, what


def check_sequential(g, s, what):
    """(cnt, pos, pwms, passes) of one chain against gs_motif_sampling_multi's."""
    gc, gp, gw, gpass = g
    sc, sp, sw, spass = s
    assert np.array_equal(gc, sc) and gpass == spass, what
    for n in range(len(gc)):
        assert np.array_equal(gp[n, :gc[n]], sp[n, :sc[n]]), (what, n)
    assert np.array_equal(bits(gw), bits(sw)), what


def oracle_sampling(S, N, M, W, cutoff, seed, init_mode, max_passes=1000):
    """The composition of test_gpu_multi.py::test_motif_sampling_multi."""
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=init_mode)
    u = np.array([ol.uniform(seed, ol.stream_sweep(0), n) for n in range(N)])
    lst = np.full((N, M), -1, np.int32)
    lst[:, 0] = p
    c1, p1, w1 = ol.sweep_lists(S, M, W, PC, cutoff, np.ones(N, np.int32), lst, M, u)
    return ol.greedy_lists(S, M, W, PC, cutoff, c1, p1, M, w1, max_passes=max_passes)


def row(out, r):
    cnt, pos, pwms, passes, status = out
    return cnt[r], pos[r], pwms[r], int(passes[r])


@pytest.fixture(scope="module")
def other_ctx():
    """The sequential side: a second context with the shipped defaults."""
    from gibbssampling_amd import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


_cases = {}
_oracle = {}


def case(name):
    """Dataset and one batch result per shape, computed once and left unchanged."""
    if name not in _cases:
        from gibbssampling_amd import Context
        alpha, N, L, W, ragged, M, cutoff, mode, dseed, _ = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
        ctx = Context(0)
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_sampling_multi_batch(M, W, PC, cutoff, SEEDS, mode)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[name] = (codes, offsets, out)
    return _cases[name]


def oracle_case(name, seed):
    """The oracle's run of one seed of a shape, computed once."""
    if (name, seed) not in _oracle:
        alpha, N, L, W, ragged, M, cutoff, mode, _, _ = SHAPES[name]
        codes, offsets, _ = case(name)
        _oracle[name, seed] = oracle_sampling(ol.Seqs(codes, offsets, alpha), N, M, W, cutoff,
                                              seed, mode)
    return _oracle[name, seed]


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name):
    alpha, N, L, W, ragged, M, cutoff, mode, _, want_passes = SHAPES[name]
    codes, offsets, out = case(name)
    cnt, pos, pwms, passes, status = out
    R = len(SEEDS)
    assert cnt.shape == (R, N) and pos.shape == (R, N, M) and pwms.shape == (R, N)
    assert passes.shape == (R,) and status.shape == (R,)
    assert not status.any()
    for r, seed in enumerate(SEEDS):
        check_oracle(row(out, r), oracle_case(name, seed), (name, seed, r))
    assert tuple(oracle_case(name, s)[3] for s in PASS_SEEDS) == want_passes
    # the duplicate seed: identical rows
    assert np.array_equal(cnt[1], cnt[3]) and passes[1] == passes[3]
    assert np.array_equal(np.where(np.arange(M)[None, :] < cnt[1][:, None], pos[1], -1),
                          np.where(np.arange(M)[None, :] < cnt[3][:, None], pos[3], -1))
    assert np.array_equal(bits(pwms[1]), bits(pwms[3]))


def test_the_chains_do_not_stop_together():
    """m4: seed 12's sweep empties every list and its chain ends after one pass with all
    lists empty, while the other chains fill every list to four."""
    _, _, (cnt, pos, pwms, passes, status) = case("m4")
    r12 = SEEDS.index(12)
    assert passes[r12] == 1 and not cnt[r12].any()
    for r, seed in enumerate(SEEDS):
        if seed != 12:
            assert passes[r] > 1 and (cnt[r] == 4).all(), (seed, r)


@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, other_ctx):
    alpha, N, L, W, ragged, M, cutoff, mode, _, _ = SHAPES[name]
    codes, offsets, out = case(name)
    other_ctx.set_sequences(codes, offsets, alpha)
    for r, seed in enumerate(SEEDS):
        s = other_ctx.motif_sampling_multi(M, W, PC, cutoff, seed, init_mode=mode)
        check_sequential(row(out, r), s, (name, seed, r))


def test_arena_growth_in_the_sweep_and_the_greedy(gpu_ctx):
    """Every window and every pair passes (cut-off -1000): each target needs 119 + 116 * 117
    / 2 = 6 905 arena entries, above the sweep's first arena (2 048) and the greedy's
    (4 096): the sweep rescores in a further round, every chain's greedy is restarted."""
    N, L, W, M, cutoff = 12, 120, 2, 3, -1000.0
    seeds = [7, 8, 9, 10]
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    S = ol.Seqs(codes, offsets, b"ACGT")
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, seeds)
    assert not out[4].any()
    info = gpu_ctx.multi_batch_last_info()
    assert info["sweep_rounds"] >= 1 and info["chains_restarted"] == 4
    assert info["restart_rounds"] >= 1
    want_passes = (2, 2, 2, 3)
    for r, seed in enumerate(seeds):
        o = oracle_sampling(S, N, M, W, cutoff, seed, 0)
        assert o[3] == want_passes[r]
        check_oracle(row(out, r), o, (seed, r))


def fsx_set():
    seqs = json.loads((GOLDEN / "fsx_sets.json").read_text())["bioTestsWithMultipleSamples"]["seqs"]
    codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
    offsets = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return seqs, codes, offsets


def test_more_chains_than_cus_fewer_targets_than_slots(gpu_ctx, other_ctx):
    """The .fsx:407 data set (N = 5, L = 27, W = 6, motifAmount 2), 300 chains."""
    seqs, codes, offsets = fsx_set()
    alpha, W, M, R = b"ATGC-", 6, 2, 300
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    seeds = [7000 + 3 * r for r in range(R)]
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, 1.0, seeds)
    assert not out[4].any()
    assert 1 <= gpu_ctx.multi_batch_last_info()["slots"] <= len(seqs)
    rows = set()
    for r, seed in enumerate(seeds):
        s = other_ctx.motif_sampling_multi(M, W, PC, 1.0, seed)
        check_sequential(row(out, r), s, (seed, r))
        rows.add((s[0].tobytes(), bits(s[2]).tobytes()))
    assert len(rows) > 1  # the seeds reach the chains


def test_one_pass_only(gpu_ctx):
    alpha, N, L, W, ragged, M, cutoff, mode, _, _ = SHAPES["dna-m2"]
    codes, offsets, _ = case("dna-m2")
    S = ol.Seqs(codes, offsets, alpha)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, SEEDS, mode, max_passes=1)
    assert not out[4].any()
    assert (out[3] == 1).all()
    for r, seed in enumerate(SEEDS):
        o = oracle_sampling(S, N, M, W, cutoff, seed, mode, max_passes=1)
        assert o[3] == 1
        check_oracle(row(out, r), o, (seed, r))


def test_amount_one_through_the_list_batch(gpu_ctx):
    """motifAmount = 1: the list batch's rows are motif_sampling_batch's."""
    N, L, W = 150, 90, 9
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=77, ragged=True, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    cnt, pos, pwms, passes, status = gpu_ctx.motif_sampling_multi_batch(1, W, PC, 1.0, SEEDS)
    spos, spwms, spasses, sstatus = gpu_ctx.motif_sampling_batch(W, PC, 1.0, SEEDS)
    assert not status.any() and not sstatus.any()
    assert pos.shape == (len(SEEDS), N, 1)
    assert np.array_equal(cnt, (spos >= 0).astype(np.int32))
    assert np.array_equal(np.where(cnt > 0, pos[:, :, 0], -1), spos)
    assert np.array_equal(passes, spasses)
    rel = np.abs(pwms - spwms) / np.maximum(np.abs(spwms), 1e-300)
    assert np.all((pwms == spwms) | (rel <= RTOL))


def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, ragged, M, cutoff, mode, _, _ = SHAPES["protein-m2"]
    codes, offsets, _ = case("protein-m2")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    want = other_ctx.motif_sampling_multi(M, W, PC, cutoff, 31)

    # one chain is gs_motif_sampling_multi
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [31])
    assert out[0].shape == (1, N) and out[1].shape == (1, N, M) and out[4][0] == 0
    check_sequential(row(out, 0), want, "one chain")
    ms = gpu_ctx.multi_batch_last_ms()
    assert len(ms) == 3 and all(np.isfinite(m) and m >= 0.0 for m in ms)
    # no snapshot is left behind
    with pytest.raises(_native.GibbsError) as e:
        gpu_ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    # ... and the next single run behaves as on a fresh context
    check_sequential(gpu_ctx.motif_sampling_multi(M, W, PC, cutoff, 31), want, "after the batch")
    assert isinstance(gpu_ctx.stats(), dict)  # the counters go on

    # a list capacity above motifAmount
    want3 = other_ctx.motif_sampling_multi(M, W, PC, cutoff, 31, cap=3)
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [31, 32], cap=3)
    assert out[1].shape == (2, N, 3) and not out[4].any()
    check_sequential(row(out, 0), want3, "cap 3")

    # no chains: nothing to do
    cnt, pos, pwms, passes, status = gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [])
    assert cnt.shape == (0, N) and pos.shape == (0, N, M) and pwms.shape == (0, N)
    assert passes.shape == (0,) and status.shape == (0,)

    # argument errors before any launch
    before = gpu_ctx.stats()
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(M, L + 1, PC, cutoff, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [1, 2], init_mode=2)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [1, 2], max_passes=0)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(17, W, PC, cutoff, [1, 2])
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(3, W, PC, cutoff, [1, 2], cap=2)
    assert gpu_ctx.stats() == before

    # the ByPCV twin is not batched
    gpu_ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            gpu_ctx.motif_sampling_multi_batch(M, W, PC, cutoff, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        gpu_ctx.set_fixed_pcv(None)


@pytest.mark.parametrize("reps", [3, 0])
def test_mirror_batched_repetitions(reps):
    """.fsx:407's call through getMotifsWithBestInformationContentsBatched equals the loop.  Per the CPU oracle the runs of seeds
    5 … 8 have Σ PWMS 16.07, 10.18, 9.49 and 59.63: the loop adopts run 0 one step later (run
    1 is computed by the batch and never asked for), then asks for runs 2 and 3 and returns
    run 0, so the replay over a finished table is on the tested path.  numberOfRepetitions =
    0 asks for run 0 alone and returns the initial best."""
    from gibbssampling_amd import MotifSampler
    seqs, _, _ = fsx_set()
    loop = MotifSampler.getMotifsWithBestInformationContents(reps, 2, 6, 1e-4, 1.0, "ATGC-", seqs,
                                                             seed=5)
    batch = MotifSampler.getMotifsWithBestInformationContentsBatched(reps, 2, 6, 1e-4, 1.0,
                                                                     "ATGC-", seqs, seed=5)
    assert [m.Positions for m in batch] == [m.Positions for m in loop]
    assert all(a.PWMS == b.PWMS or abs(a.PWMS - b.PWMS) <= RTOL * abs(b.PWMS)
               for a, b in zip(batch, loop))
    assert len(batch) == (len(seqs) if reps else 1)
