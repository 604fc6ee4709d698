"""GPU parity of gs_motif_sampling_batch_fixed (Context.motif_sampling_batch(pcv=, ppm=)):
R repetitions of the ByPCV pipeline (findBestInormationContentContainingMotifsWithPCV,
.fs:856-881) or of doMotifSamplingWithPPM (getBestPWMSsOfPPM, .fs:1001-1026) in one call.
Every row against the oracle's composition for its seed and against the sequential entry
point gs_motif_sampling on a second context that has the values set on it; then the
contract of the three *_batch_fixed entry points.

Bar: positions and pass counts exact, PWMS within 1e-12 relative of the oracle.  Under a
PCV the single chain stays on the star engine, as the batch's chains: bit-identical PWMS.
Under a PPM alone the default single chain hands over to speculative passes (within 1e-12)
and the greedy_switch = 0 one is bit-identical."""
import numpy as np
import pytest

from conftest import make_dataset
from fixed_batch_cases import (CUTOFF, PC, SEEDS, SHAPES, bits, close, dataset, pcv49, ppm49,
                               set_fixed, sources_of, values)
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

MODES = (0, 1)
KINDS = ("pcv", "ppm")


def oracle_motif_sampling(S, N, W, seed, mode, pcv, ppm):
    """random_starts (…WithBPV / …OfPPM) -> sweep 0 of the seed -> greedy, ByPCV under a PCV."""
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=mode, pcv49=pcv, ppm49=ppm)
    u = np.array([ol.uniform(seed, ol.stream_sweep(0), n) for n in range(N)])
    if pcv is not None:
        p1, w1, _ = ol.sweep_pcv(S, W, PC, CUTOFF, pcv, p, u)
        return ol.greedy_pcv(S, W, PC, CUTOFF, pcv, p1, w1)
    p1, w1, _ = ol.sweep(S, W, PC, CUTOFF, p, u)
    return ol.greedy(S, W, PC, CUTOFF, p1, w1)


def fresh(tuning=None):
    from gibbssampling_amd import Context
    return Context(0, tuning=tuning)


@pytest.fixture(scope="module")
def other_ctx():
    """The sequential side: a second context, the values set on it by the test."""
    ctx = fresh()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def star_ctx():
    """Sequential runs with every pass on the star engine, as the batch's chains."""
    ctx = fresh({"greedy_switch": 0})
    yield ctx
    ctx.close()


_cases = {}
_plain = {}


def case(name, mode, kind, batch_starts=0):
    """One batch result per (shape, init mode, values, way of making the starts), computed
    once and left unchanged."""
    key = (name, mode, kind, batch_starts)
    if key not in _cases:
        alpha, _, N, L, W, _, _ = SHAPES[name]
        codes, offsets = dataset(name)
        pcv, ppm = values(name, kind)
        ctx = fresh({"batch_starts": batch_starts})
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, mode, pcv=pcv, ppm=ppm)
        ctx.close()
        for a in out:
            a.setflags(write=False)
        _cases[key] = out
    return _cases[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_chain_equals_the_oracle(name, mode, kind):
    alpha, extra, N, L, W, _, _ = SHAPES[name]
    codes, offsets = dataset(name)
    if extra:  # the symbol outside the alphabet is in the data
        assert np.isin(codes, np.frombuffer(extra, np.uint8)).any()
    pcv, ppm = values(name, kind)
    pos, pwms, passes, status = case(name, mode, kind)
    assert pos.shape == (len(SEEDS), N) and pwms.shape == (len(SEEDS), N)
    assert not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    for seed in sorted(set(SEEDS)):
        op, ow, opass = oracle_motif_sampling(S, N, W, seed, mode, pcv, ppm)
        for r in [i for i, s in enumerate(SEEDS) if s == seed]:
            assert np.array_equal(pos[r], op), (seed, r)
            assert passes[r] == opass, (seed, r)
            assert close(pwms[r], ow), (seed, r)
    # the duplicate seed: identical rows
    assert np.array_equal(pos[1], pos[3]) and passes[1] == passes[3]
    assert np.array_equal(bits(pwms[1]), bits(pwms[3]))
    if kind == "pcv":  # the seeds reach the chains (a random PPM alone decides every start)
        assert len({p.tobytes() for p in pos}) > 1


@pytest.mark.parametrize("kind", KINDS + ("both",))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_both_ways_of_making_the_starts_honour_the_values(name, mode, kind):
    a, b = case(name, mode, kind, 0), case(name, mode, kind, 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert not a[3].any() and not b[3].any()
    # ... and they change the result: not the plain batch's
    if (name, mode) not in _plain:
        alpha, _, N, L, W, _, _ = SHAPES[name]
        codes, offsets = dataset(name)
        ctx = fresh()
        ctx.set_sequences(codes, offsets, alpha)
        _plain[name, mode] = ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, mode)
        ctx.close()
    assert not np.array_equal(_plain[name, mode][0], a[0])


@pytest.mark.parametrize("kind", KINDS + ("both",))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, mode, kind, other_ctx, star_ctx):
    alpha, _, N, L, W, _, _ = SHAPES[name]
    codes, offsets = dataset(name)
    pcv, ppm = values(name, kind)
    pos, pwms, passes, status = case(name, mode, kind)
    for ctx in (other_ctx, star_ctx):
        ctx.set_sequences(codes, offsets, alpha)
        set_fixed(ctx, pcv, ppm, W)
    try:
        for r, seed in enumerate(SEEDS):
            sp, sw, spass = other_ctx.motif_sampling(W, PC, CUTOFF, seed, mode)
            assert np.array_equal(pos[r], sp) and passes[r] == spass, (seed, r)
            if pcv is not None:  # the single chain stays on the star engine
                assert np.array_equal(bits(pwms[r]), bits(sw)), (seed, r)
            else:
                assert close(pwms[r], sw), (seed, r)
            tp, tw, tpass = star_ctx.motif_sampling(W, PC, CUTOFF, seed, mode)
            assert np.array_equal(pos[r], tp) and passes[r] == tpass, (seed, r)
            assert np.array_equal(bits(pwms[r]), bits(tw)), (seed, r)
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
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, seeds, pcv=pcv)
    assert not status.any()
    other_ctx.set_fixed_pcv(pcv)
    try:
        for r, seed in enumerate(seeds):
            sp, sw, spass = other_ctx.motif_sampling(W, PC, CUTOFF, seed)
            assert np.array_equal(pos[r], sp) and passes[r] == spass, (seed, r)
            assert np.array_equal(bits(pwms[r]), bits(sw)), (seed, r)
    finally:
        other_ctx.set_fixed_pcv(None)
    assert len({p.tobytes() for p in pos}) > 1  # the seeds reach the chains


# ---- the contract of the three entry points ------------------------------------------------

def calls(ctx, W, M=2):
    """The three batched drivers of a context as (name, call(**values))."""
    return [
        ("motif", lambda **kw: ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, **kw)),
        ("site", lambda **kw: ctx.site_sampling_batch(W, PC, SEEDS, **kw)),
        ("multi", lambda **kw: ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, SEEDS, **kw)),
    ]


def same_outputs(a, b):
    return all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                              y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def test_both_null_is_the_plain_batch(gpu_ctx):
    """The *_fixed symbols with null pcv49 and ppm49 against the plain symbols, bit for bit
    (the keywords' None goes to the plain symbols, so the symbols are called directly)."""
    alpha, _, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = dataset("protein")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    lib, h, R, M = gpu_ctx.lib, gpu_ctx.h, len(SEEDS), 2
    seeds = np.array(SEEDS, np.uint64)
    p = _native._ptr

    def outs(*extra):
        return (np.zeros((R, N) + extra, np.int32), np.zeros((R, N), np.float64),
                np.zeros(R, np.int32), np.zeros(R, np.int32))

    plain = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS)
    pos, pw, pas, st = outs()
    assert lib.gs_motif_sampling_batch_fixed(h, W, PC, CUTOFF, None, None, p(seeds), R, 0, 1000,
                                             p(pos), p(pw), p(pas), p(st)) == 0
    assert same_outputs(plain, (pos, pw, pas, st))

    plain = gpu_ctx.site_sampling_batch(W, PC, SEEDS)
    pos, sc, _, st = outs()
    pas = np.zeros((R, 3), np.int32)
    assert lib.gs_site_sampling_batch_fixed(h, W, PC, None, None, p(seeds), R, 0, 1000, p(pos),
                                            p(sc), p(pas), p(st)) == 0
    assert same_outputs(plain, (pos, sc, pas, st))

    plain = gpu_ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, SEEDS)
    pos, pw, pas, st = outs(M)
    cnt = np.zeros((R, N), np.int32)
    assert lib.gs_motif_sampling_multi_batch_fixed(h, M, W, PC, CUTOFF, None, None, p(seeds), R, 0,
                                                   1000, M, p(cnt), p(pos), p(pw), p(pas),
                                                   p(st)) == 0
    live = np.arange(M)[None, None, :] < cnt[:, :, None]
    assert np.array_equal(plain[0], cnt) and np.array_equal(plain[3], pas)
    assert np.array_equal(np.where(live, plain[1], -1), np.where(live, pos, -1))
    assert np.array_equal(bits(plain[2]), bits(pw)) and not st.any()


def test_one_source_of_the_values_per_call(gpu_ctx):
    """While the context holds a fixed PCV or PPM the *_fixed entry points refuse, with a
    message saying to pass the values as arguments, and launch nothing."""
    alpha, _, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = dataset("protein")
    pcv, ppm = values("protein", "both")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    for own in ("pcv", "ppm"):
        set_fixed(gpu_ctx, pcv if own == "pcv" else None, ppm if own == "ppm" else None, W)
        try:
            before = gpu_ctx.stats()
            for name, call in calls(gpu_ctx, W):
                for kw in (dict(pcv=pcv), dict(ppm=ppm), dict(pcv=pcv, ppm=ppm)):
                    with pytest.raises(_native.GibbsError) as e:
                        call(**kw)
                    assert e.value.status == _native.GS_E_UNSUPPORTED, (own, name)
                    assert "as arguments" in str(e.value), (own, name)
            assert gpu_ctx.stats() == before
        finally:
            set_fixed(gpu_ctx, None, None, W)


def test_argument_errors_before_any_launch(gpu_ctx):
    alpha, _, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = dataset("protein")
    pcv, ppm = values("protein", "both")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    before = gpu_ctx.stats()
    for name, call in calls(gpu_ctx, W):
        with pytest.raises(_native.ArgumentError) as e:  # a PPM of another motifLength
            call(ppm=ppm49(W + 1, 3))
        assert e.value.status == _native.GS_E_ARG, name
        with pytest.raises(_native.ArgumentError):
            call(pcv=pcv[:48])
        with pytest.raises(_native.ArgumentError):  # what the sibling refuses
            call(pcv=pcv, init_mode=2)
        with pytest.raises(_native.ArgumentError):
            call(pcv=pcv, max_passes=0)
    for name, call in calls(gpu_ctx, L + 1):
        with pytest.raises(_native.ArgumentError):
            call(pcv=pcv)
    with pytest.raises(_native.ArgumentError):
        gpu_ctx.motif_sampling_multi_batch(17, W, PC, CUTOFF, SEEDS, pcv=pcv)
    assert gpu_ctx.stats() == before
    # no chains: nothing to do
    pos, pwms, passes, status = gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, [], pcv=pcv, ppm=ppm)
    assert pos.shape == (0, N) and passes.shape == (0,) and status.shape == (0,)


@pytest.mark.parametrize("driver", ["motif", "site", "multi"])
def test_the_context_is_as_before_after_a_fixed_call(driver):
    """After a *_fixed call a plain motif_sampling, a plain motif_sampling_batch and
    sweep_kernel_name() equal a fresh context's, no snapshot is left, the context's own
    fixed state is untouched and set_fixed_pcv still makes the old entry point refuse.
    dna_mode 1: the plain single chain sweeps with a packed DNA kernel, which excludes a
    fixed PCV, so a value left behind would show in the kernel choice."""
    alpha, _, N, L, W, _, _ = SHAPES["dna"]
    codes, offsets = dataset("dna")
    pcv, ppm = values("dna", "both")
    used, new = fresh({"dna_mode": 1}), fresh({"dna_mode": 1})
    try:
        for ctx in (used, new):
            ctx.set_sequences(codes, offsets, alpha)
        assert new.sweep_kernel_name() != "gs_sweep_kernel"
        out = dict(calls(used, W))[driver](pcv=pcv, ppm=ppm)
        assert not out[-1].any()
        with pytest.raises(_native.GibbsError) as e:
            used.get_state()
        assert e.value.status == _native.GS_E_STATE
        assert used.sweep_kernel_name() == new.sweep_kernel_name()
        a, b = used.motif_sampling(W, PC, CUTOFF, 31), new.motif_sampling(W, PC, CUTOFF, 31)
        assert np.array_equal(a[0], b[0]) and a[2] == b[2]
        assert np.array_equal(bits(a[1]), bits(b[1]))
        assert used.sweep_kernel_name() == new.sweep_kernel_name()
        assert used.last_sweep_launch() == new.last_sweep_launch()
        assert same_outputs(used.motif_sampling_batch(W, PC, CUTOFF, SEEDS),
                            new.motif_sampling_batch(W, PC, CUTOFF, SEEDS))
        assert same_outputs(used.site_sampling_batch(W, PC, SEEDS),
                            new.site_sampling_batch(W, PC, SEEDS))
        # the values went with the call: the single chain is the plain one again (above),
        # and the context's own PCV still makes the old batch entry points refuse
        used.set_fixed_pcv(pcv)
        with pytest.raises(_native.GibbsError) as e:
            used.motif_sampling_batch(W, PC, CUTOFF, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
        # ... and is what the single chain then uses
        new.set_fixed_pcv(pcv)
        a, b = used.motif_sampling(W, PC, CUTOFF, 31), new.motif_sampling(W, PC, CUTOFF, 31)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    finally:
        used.close()
        new.close()


def test_last_ms_reports_the_fixed_call(gpu_ctx):
    alpha, _, N, L, W, _, _ = SHAPES["protein"]
    codes, offsets = dataset("protein")
    pcv, _ = values("protein", "pcv")
    gpu_ctx.set_sequences(codes, offsets, alpha)
    gpu_ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS, pcv=pcv)
    ms = gpu_ctx.batch_last_ms()
    assert len(ms) == 2 and all(np.isfinite(m) and m > 0.0 for m in ms)


# ---- the mirrors ---------------------------------------------------------------------------

def same_motifs(batch, loop):
    assert [list(m.Positions) for m in batch] == [list(m.Positions) for m in loop]
    assert close([m.PWMS for m in batch], [m.PWMS for m in loop])


@pytest.mark.parametrize("reps", [3, 0])
def test_mirrors_batch_keyword(reps):
    from gibbssampling_amd import MotifSampler
    N, L, W, seed = 40, 60, 7, 99
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = sources_of(codes, offsets)
    pcv, ppm = pcv49(b"ACGT", 5), ppm49(W, 6)
    for M in (1, 2):
        loop = MotifSampler.findBestInormationContentContainingMotifsWithPCV(
            reps, M, W, PC, CUTOFF, "ACGT", sources, pcv, seed=seed)
        batch = MotifSampler.findBestInormationContentContainingMotifsWithPCV(
            reps, M, W, PC, CUTOFF, "ACGT", sources, pcv, seed=seed, batch=True)
        same_motifs(batch, loop)
        assert len(batch) == (N if reps else 1)
    loop = MotifSampler.getBestPWMSsOfPPM(reps, 1, W, PC, CUTOFF, "ACGT", sources, ppm, seed=seed)
    batch = MotifSampler.getBestPWMSsOfPPM(reps, 1, W, PC, CUTOFF, "ACGT", sources, ppm,
                                           seed=seed, batch=True)
    same_motifs(batch, loop)
    assert len(batch) == (N if reps else 1)
