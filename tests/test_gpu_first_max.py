"""GPU parity of every argmax on exact ties: the first maximum wins.

The fixtures of tests/first_max.py are repeat sequences (a short unit tiled along each
sequence, a few point mutations) whose maximum is attained by several windows: in
different lanes (k mod 64), 64-window chunks and 512-thread blocks.  A reduction that
lets the lowest lane, the last chunk or the lowest wavefront win instead of the lowest
window passes every i.i.d. parity test and fails here.  tests/test_first_max_host.py
asserts on the CPU that the oracle's pick is the truth at every visit (no near-tie of
distinct motif products, no fresh-against-stored comparison that a last-place
difference of the logs could flip), so this module needs no tolerance on positions.

Bar: positions and pass counts identical to the oracle; scores within 1e-12 relative,
infinities and NaN equal; a background pick's PWMS (a raw binary64 product, no log)
bit for bit; gs_counts of the refined positions equal to the oracle's.  The batched
drivers are compared row by row with the single-chain calls, bit for bit.
"""
import numpy as np
import pytest

import first_max as fm
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC = fm.PC
STAR = ["dna", "atgc", "protein", "wide"]


def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    same = (g == o) | (np.isnan(g) & np.isnan(o))  # equal infinities and NaN included
    with np.errstate(invalid="ignore"):
        rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(same | (rel <= RTOL)))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def check_greedy(ctx, f, g, o, what):
    gpos, gpw, gpass = g
    opos, opw, opass = o
    bad = np.nonzero(gpos != opos)[0]
    assert bad.size == 0, f"{what}: positions differ at {bad[:10]}: {gpos[bad[:5]]} vs {opos[bad[:5]]}"
    assert gpass == opass, f"{what}: {gpass} passes, the oracle {opass}"
    assert close(gpw, opw), f"{what}: PWMS differ"
    none = opos < 0  # [] is a background pick (or the untouched memory): a product, no log
    assert np.array_equal(bits(gpw[none]), bits(opw[none])), f"{what}: background PWMS not bit-equal"
    Cg, Tg = ctx.counts(f.W, gpos, len(f.alpha))
    Co, To = ol.counts(f.seqs, f.W, gpos)
    assert np.array_equal(Cg, Co) and np.array_equal(Tg, To), f"{what}: aggregates differ"


def check_site(g, o, what):
    gp, gs, gpass = g
    op, os_, opass = o
    bad = np.nonzero(gp != op)[0]
    assert bad.size == 0, f"{what}: positions differ at {bad[:10]}: {gp[bad[:5]]} vs {op[bad[:5]]}"
    assert gpass == opass, f"{what}: {gpass} passes, the oracle {opass}"
    assert close(gs, os_), f"{what}: scores differ"


def load(ctx, f):
    ctx.set_sequences(f.codes, f.offsets, f.alpha)


@pytest.fixture
def fixed(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_fixed_pcv(None)
    gpu_ctx.set_fixed_ppm(None)


def tuned(tuning):
    from gibbssampling_amd import Context
    return Context(0, tuning=tuning)


# ---- the star greedy ------------------------------------------------------------------
def star_greedy(ctx, f, tag):
    for cutoff in fm.CUTOFFS:
        for mp in (1, 1000):
            g = ctx.motif_greedy(f.W, PC, cutoff, f.pos0, f.pw0, max_passes=mp)
            check_greedy(ctx, f, g, f.greedy(cutoff, mp), f"{f.name} {tag} cut-off {cutoff:g} max_passes {mp}")


@pytest.mark.parametrize("name", STAR + ["zero"])
def test_star_greedy(gpu_ctx, name):
    f = fm.fixture(name)
    load(gpu_ctx, f)
    star_greedy(gpu_ctx, f, "default")


GREEDY_TUNINGS = {
    "waves1": {"greedy_waves": 1}, "waves3": {"greedy_waves": 3}, "waves8": {"greedy_waves": 8},
    "lone": {"motif_coop": 1, "greedy_switch": 0},   # every wavefront on one visit
    "handover": {"greedy_switch": 1},                # to the speculative list path
    "midpass": {"greedy_exit_chunk": 16, "greedy_exit_ratio": 4},  # ... inside the first pass
}


@pytest.mark.parametrize("tuning", list(GREEDY_TUNINGS))
@pytest.mark.parametrize("name", STAR)
def test_star_greedy_engines(name, tuning):
    f = fm.fixture(name)
    c = tuned(GREEDY_TUNINGS[tuning])
    try:
        load(c, f)
        star_greedy(c, f, tuning)
    finally:
        c.close()


@pytest.mark.parametrize("name", STAR)
def test_greedy_by_pcv(fixed, name):
    f = fm.fixture(name)
    load(fixed, f)
    fixed.set_fixed_pcv(f.pcv)
    for mp in (1, 1000):
        g = fixed.motif_greedy(f.W, PC, 1.0, f.pos0, f.pw0, max_passes=mp)
        check_greedy(fixed, f, g, f.greedy(1.0, mp, pcv=True), f"{name} ByPCV max_passes {mp}")


# ---- the site sampler -----------------------------------------------------------------
def site_all(ctx, f, tag):
    """The scans and the three refinements, with the fixed PCV (the tie cases) and with
    the drifting background (plain parity on the same data)."""
    for pcv in (True, False):
        ctx.set_fixed_pcv(f.pcv if pcv else None)
        what = f"{f.name} {tag} {'fixed PCV' if pcv else 'drifting'}"
        gs, gp = ctx.site_scan(f.W, PC, f.r0)
        os_, op = f.site_scan(pcv)
        assert np.array_equal(gp, op), f"{what}: scan differs at {np.nonzero(gp != op)[0][:10]}"
        assert close(gs, os_), f"{what}: scan scores differ"
        for shift in (0, -1, 1):
            g = ctx.site_refine(f.W, PC, shift, f.r0, f.sc0)
            check_site(g, f.site_refine(shift, pcv), f"{what} shift {shift}")


@pytest.mark.parametrize("name", STAR + ["zero"])
def test_site_scans_and_refinements(fixed, name):
    f = fm.fixture(name)
    load(fixed, f)
    site_all(fixed, f, "default")


SITE_TUNINGS = {
    "switch0": {"site_switch": 0}, "switch1": {"site_switch": 1},
    "coop0": {"site_coop": 0, "site_switch": 0}, "coop1": {"site_coop": 1, "site_switch": 0},
    "waves1": {"greedy_waves": 1}, "waves8": {"greedy_waves": 8},
    "midpass": {"site_exit_chunk": 16, "site_exit_ratio": 4, "site_switch": 4},
}


@pytest.mark.parametrize("tuning", list(SITE_TUNINGS))
@pytest.mark.parametrize("name", STAR)
def test_site_engines(name, tuning):
    f = fm.fixture(name)
    c = tuned(SITE_TUNINGS[tuning])
    try:
        load(c, f)
        site_all(c, f, tuning)
    finally:
        c.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", STAR + ["zero"])
def test_random_starts_fixed_pcv_and_ppm(fixed, name, mode):
    f = fm.fixture(name)
    load(fixed, f)
    fixed.set_fixed_pcv(f.pcv)
    gs, gp = fixed.random_starts(f.W, PC, 77, mode)
    os_, op = ol.random_starts(f.seqs, f.W, PC, seed=77, mode=mode, pcv49=f.pcv)
    assert np.array_equal(gp, op) and close(gs, os_), f"{name}: WithBPV starts"
    fixed.set_fixed_pcv(None)
    ppm = np.random.default_rng(13).uniform(0.01, 1.0, (49, f.W))
    fixed.set_fixed_ppm(ppm, f.W)
    gs, gp = fixed.random_starts(f.W, PC, 78, mode)
    os_, op = ol.random_starts(f.seqs, f.W, PC, seed=78, mode=mode, ppm49=ppm)
    assert np.array_equal(gp, op) and close(gs, os_), f"{name}: OfPPM starts"


def test_best_pwms_zero_case(gpu_ctx):
    """getBestPWMSs where no window beats the 0.0 it starts from: (log2 0., 0); where
    only windows k >= 64 do; and on a homopolymer."""
    f = fm.fixture("zero")
    load(gpu_ctx, f)
    rng = np.random.default_rng(5)
    fcv = np.zeros(49, np.int64)
    ppm = np.zeros((49, f.W))
    for a in f.alpha:
        fcv[a - 42] = rng.integers(200, 400)
        ppm[a - 42] = rng.random(f.W) + 1e-3
    ppm /= ppm.sum(0, keepdims=True)
    for n in range(4):
        want = ol.best_pwms(f.seqs, f.W, PC, n, fcv, ppm[[a - 42 for a in f.alpha]])
        got = gpu_ctx.best_pwms(f.W, PC, n, fcv, ppm)
        assert got[1] == want[1] and close([got[0]], [want[0]]), f"target {n}: {got} vs {want}"
        if n == 0:
            assert got == (-np.inf, 0)
        if n == 1:
            assert got[1] >= 64


# ---- the Positions lists --------------------------------------------------------------
def check_lists(g, o, what):
    gc, gp, gw, gpass = g
    oc, op, ow, opass = o
    assert np.array_equal(gc, oc), f"{what}: list lengths differ at {np.nonzero(gc != oc)[0][:10]}"
    for n in range(len(gc)):
        assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), f"{what}: positions differ at {n}"
    assert gpass == opass, f"{what}: {gpass} passes, the oracle {opass}"
    assert close(gw, ow), f"{what}: PWMS differ"


def list_greedy(ctx, f, tag):
    for mp in (1, 1000):
        g = ctx.motif_greedy_multi(f.M, f.W, PC, 1.0, f.cnt0, f.pos0, f.pw0, max_passes=mp)
        check_lists(g, f.greedy(1.0, mp), f"{f.name} {tag} max_passes {mp}")


@pytest.mark.parametrize("name", ["lists2", "lists3"])
def test_list_greedy(gpu_ctx, name):
    f = fm.fixture(name)
    load(gpu_ctx, f)
    list_greedy(gpu_ctx, f, "default")


@pytest.mark.parametrize("tuning", [{"multi_greedy_threads": 64}, {"multi_greedy_threads": 1024},
                                    {"multi_spec_slots": 1}, {"multi_spec_slots": 64}],
                         ids=["threads64", "threads1024", "slots1", "slots64"])
@pytest.mark.parametrize("name", ["lists2", "lists3"])
def test_list_greedy_engines(name, tuning):
    f = fm.fixture(name)
    c = tuned(tuning)
    try:
        load(c, f)
        list_greedy(c, f, str(tuning))
    finally:
        c.close()


@pytest.mark.parametrize("name", ["dna", "wide"])
def test_list_greedy_amount_one_equals_star(gpu_ctx, name):
    f = fm.fixture(name)
    load(gpu_ctx, f)
    cnt = (f.pos0 >= 0).astype(np.int32)
    lst = f.pos0.reshape(-1, 1)
    for cutoff in fm.CUTOFFS:
        lc, lp, lw, lpass = gpu_ctx.motif_greedy_multi(1, f.W, PC, cutoff, cnt, lst, f.pw0)
        o = f.greedy(cutoff)
        assert np.array_equal(np.where(lc > 0, lp[:, 0], -1), o[0]) and lpass == o[2]
        assert close(lw, o[1])
        star = gpu_ctx.motif_greedy(f.W, PC, cutoff, f.pos0, f.pw0)
        assert np.array_equal(bits(lw), bits(star[1]))


# ---- the batched drivers, GPU against GPU ----------------------------------------------
SEEDS = [11, 12, 13, 14]


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("batch_starts", [0, 1])
def test_batched_rows_equal_single_chains(batch_starts):
    """Row r of every batched driver equals the single-chain call with seeds[r], bit for
    bit (both sides use the device log: no libm question)."""
    f = fm.fixture("dna")
    W = f.W
    c = tuned({"batch_starts": batch_starts})
    try:
        load(c, f)
        for mode in (0, 1):
            bp, bw, bpass, st = c.motif_sampling_batch(W, PC, 1.0, SEEDS, init_mode=mode)
            assert not st.any()
            for r, s in enumerate(SEEDS):
                p, w, k = c.motif_sampling(W, PC, 1.0, s, init_mode=mode)
                assert np.array_equal(bp[r], p) and same_bits(bw[r], w) and bpass[r] == k, \
                    f"motif_sampling_batch mode {mode} row {r}"
            bp, bs, bpass, st = c.site_sampling_batch(W, PC, SEEDS, init_mode=mode)
            assert not st.any()
            for r, s in enumerate(SEEDS):
                p, sc, k = c.site_sampling(W, PC, s, init_mode=mode)
                assert np.array_equal(bp[r], p) and same_bits(bs[r], sc) and list(bpass[r]) == list(k), \
                    f"site_sampling_batch mode {mode} row {r}"
            for pcv in (None, f.pcv):
                c.set_fixed_pcv(pcv)
                bs, bp, st = c.random_starts_batch(W, PC, SEEDS, mode)
                assert not st.any()
                for r, s in enumerate(SEEDS):
                    sc, p = c.random_starts(W, PC, s, mode)
                    assert np.array_equal(bp[r], p) and same_bits(bs[r], sc), \
                        f"random_starts_batch mode {mode} pcv {pcv is not None} row {r}"
                    if pcv is not None:  # the tie case: also against the oracle itself
                        osc, op = ol.random_starts(f.seqs, W, PC, seed=s, mode=mode, pcv49=pcv)
                        assert np.array_equal(bp[r], op) and close(bs[r], osc)
            c.set_fixed_pcv(None)
        bc, bp, bw, bpass, st = c.motif_sampling_multi_batch(2, W, PC, 1.0, SEEDS)
        assert not st.any()
        for r, s in enumerate(SEEDS):
            cn, p, w, k = c.motif_sampling_multi(2, W, PC, 1.0, s)
            assert np.array_equal(bc[r], cn) and same_bits(bw[r], w) and bpass[r] == k, \
                f"motif_sampling_multi_batch row {r}"
            for n in range(f.N):
                assert list(bp[r, n, :cn[n]]) == list(p[n, :cn[n]]), f"multi_batch row {r} target {n}"
    finally:
        c.close()
