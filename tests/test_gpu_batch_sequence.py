"""What a batch call leaves behind on a context that goes on being used: the four batched
entry points, a rejected call and two single-chain calls, one after the other on one
context.  Every result must equal, bit for bit, the same call made first on a fresh
context; the rejected call raises GS_E_UNSUPPORTED and changes nothing that follows."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset
from gibbssampling_amd import _native

pytestmark = pytest.mark.gpu

PC, CUTOFF = 1e-4, 1.0
N, L, W = 12, 40, 6
SEEDS = [11, 5_000_000_011, 12]
# four symbols: the packed-layout sweeps are the chains' scratch; five: the general sweep
ALPHABETS = {"dna": b"ACGT", "gap-symbol": b"ATGC-"}


def words(a):
    """An array's bits: equal arrays of doubles are equal words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def lists_only(out):
    """A list batch's result with the entries past cnt (unspecified) masked."""
    cnt, pos, pwms, passes, status = out
    pos = np.where(np.arange(pos.shape[2])[None, None, :] < cnt[:, :, None], pos, -1)
    return cnt, pos, pwms, passes, status


def steps(offsets):
    """(name, call on a context) in the order of the sequence."""
    rows = np.stack([init_positions(offsets, W, 30 + r, 0.1) for r in range(len(SEEDS))])
    p0 = init_positions(offsets, W, 40, 0.1)

    def rejected(ctx):
        ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
        try:
            with pytest.raises(_native.GibbsError) as e:
                ctx.site_sampling_batch(W, PC, SEEDS)
            return (np.array([e.value.status]),)
        finally:
            ctx.set_fixed_pcv(None)

    def sweeps_from_positions(ctx):
        ctx.set_positions(W, p0)
        ctx.run_sweeps(PC, CUTOFF, 3, SEEDS[1])
        return ctx.get_state()

    return [
        ("motif_sampling_batch", lambda ctx: ctx.motif_sampling_batch(W, PC, CUTOFF, SEEDS)),
        ("site_sampling_batch", lambda ctx: ctx.site_sampling_batch(W, PC, SEEDS)),
        ("motif_sampling_multi_batch",
         lambda ctx: lists_only(ctx.motif_sampling_multi_batch(2, W, PC, CUTOFF, SEEDS))),
        ("motif_run_batch, drawn starts",
         lambda ctx: ctx.motif_run_batch(W, PC, CUTOFF, 3, SEEDS, init_mode=0)),
        ("motif_run_batch, uploaded rows",
         lambda ctx: ctx.motif_run_batch(W, PC, CUTOFF, 3, SEEDS, pos=rows)),
        ("rejected site_sampling_batch", rejected),
        ("motif_sampling", lambda ctx: ctx.motif_sampling(W, PC, CUTOFF, SEEDS[0])[:3]),
        ("run_sweeps after set_positions", sweeps_from_positions),
    ]


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_each_call_in_sequence_equals_the_call_on_a_fresh_context(name):
    from gibbssampling_amd import Context
    alpha = ALPHABETS[name]
    codes, offsets = make_dataset(N, L, W, alpha, seed=3)
    used = Context(0)
    used.set_sequences(codes, offsets, alpha)
    try:
        for what, call in steps(offsets):
            fresh = Context(0)
            fresh.set_sequences(codes, offsets, alpha)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            got = call(used)
            assert len(got) == len(want), what
            for k, (g, w) in enumerate(zip(got, want)):
                g, w = np.asarray(g), np.asarray(w)
                assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
                assert np.array_equal(words(g), words(w)), (what, k)
            if what.startswith("rejected"):
                assert got[0][0] == _native.GS_E_UNSUPPORTED
            elif "batch" in what:
                assert not got[-1].any(), what  # every chain's status
    finally:
        used.close()
