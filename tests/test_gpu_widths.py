"""GPU parity at every motif width class, W up to the documented maximum of 64.

gs_sweep_kernel<WM, H, GL, EK, ONE> and gs_greedy_kernel<SITE, WM, DT, BATCH> are compiled
once per width class WM = gs_sweep_wm(W): 4, 8, .., 32, 40, 48, 56, 64.  This module runs
every W of 1..64 through the general sweep for DNA (the four-symbol kernel where W is a
multiple of 4 up to 32), ATGC- and protein, the wide classes at 16, 32 and 64 lanes a
sequence, both paths of the four-symbol kernel on its unsplit side (W = 20, 24, 28), the
workgroup shapes the LDS carve falls back to (4, 2, 1 wavefronts for the pair tables, 12,
6, 3 for H = 1), the shape the carve refuses, the greedy and site passes, and at W = 64
and one padded width the initialiser, best_pwms, the ByPCV twins, the drivers, the batched
drivers and the list path.  tests/widths.py builds the snapshots and restates the launch
arithmetic; tests/test_widths_host.py checks on the CPU what they promise.

Bar: positions, counts and pass counts identical to the oracle's, no tolerance and no
target left out; PWMS and scores within 1e-12 relative, infinities equal; rescan_recheck
and desc_oob stay 0.  Every sweep case asserts the kernel and the launch that ran.
"""
import re

import numpy as np
import pytest

import widths as wd
from conftest import make_dataset, uniforms
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

PC, CUT, RTOL = wd.PC, wd.CUT, 1e-12
MARGIN = 1e-9  # a condition on the inputs (the oracle's own margin), never on the GPU's picks

# ---- the W lists (tests/test_widths_host.py checks the classes they reach) ------------
LANES_ATGC5 = (21, 24, 28, 32, 41, 48, 57, 64)
LANES_EK4 = (20, 24, 28)
LANES_PROTEIN = (41, 64)
LANES_LMAX = {16: 200, 32: 400, 64: 700}
EK4_PATHS_W = (8, 20, 24, 28)
GREEDY_W = {"dna": (21, 26, 28, 30, 32, 33, 40, 48, 50, 56, 57, 64), "atgc5": (24, 41, 64), "protein": (21, 41, 64)}
GREEDY_EXTRA = {"dna": b"", "atgc5": b"*", "protein": b""}
GREEDY_TUNINGS = {"default": {}, "waves1": {"greedy_waves": 1.0}, "waves2": {"greedy_waves": 2.0},
                  "waves8": {"greedy_waves": 8.0}}
COOP = (("dna", 21), ("dna", 28), ("dna", 30), ("dna", 33), ("atgc5", 41), ("dna", 50), ("protein", 64))
COOP_W = tuple(W for _, W in COOP)
TOP_W = (64, 57)
FOREIGN11 = b"BDEFHIJKLMN"
LADDER_N = 64 * 4 + 5


def ladder_shapes(limit):
    """(H, wavefronts, alphabet, foreign symbols, W) of the first candidate whose automatic
    launch takes each wavefront count under `limit` bytes of LDS (Lmax <= W + 70: 16 lanes
    a sequence for the pair tables, 32 for H = 1), the widest first.  At 163840 B: H = 2
    takes 4 at ATGC- W = 48, 2 at ATGC- W = 64 and 1 at ATGC- with three foreign
    symbols, W = 64; H = 1 takes 12 at protein W = 21, 6 at W = 41 and 3 at W = 64."""
    out, seen = [], set()
    for alpha, extra in ((b"ATGC-", b""), (b"ATGC-", b"BDE"), (wd.PROTEIN, b"")):
        A, E = len(alpha), len(alpha) + len(extra)
        for W in (64, 57, 48, 41, 32, 21, 8):
            waves = wd.auto_waves(A, E, W, W + 70, limit)
            key = (wd.scan_group(E), waves)
            if waves is not None and key not in seen:
                seen.add(key)
                out.append((key[0], waves, alpha, extra, W))
    return out


# ---- contexts -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctxs():
    """One Context per tuning, created on first use; the counters are checked as it closes."""
    from gibbssampling_amd import Context
    made = {}

    def get(**tuning):
        key = tuple(sorted(tuning.items()))
        if key not in made:
            made[key] = Context(0, tuning={k: float(v) for k, v in tuning.items()})
        return made[key]

    yield get
    for key, c in made.items():
        st = c.stats()
        c.close()
        assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, (key, st)


@pytest.fixture(scope="module")
def lds_limit(ctxs):
    """The device's LDS bytes per workgroup as the library sees them: launch_sweep names
    them when it refuses a shape (ATGC- with eleven foreign symbols, W = 64, fits at no
    wavefront count under any limit up to 160 KiB)."""
    from gibbssampling_amd._native import GS_E_UNSUPPORTED, GibbsError
    c = ctxs(dna_mode=0)
    codes, offsets, _ = wd.lanes_dataset(4, 134, 64, b"ATGC-", 77, extra=FOREIGN11, extra_rate=0.05)
    c.set_sequences(codes, offsets, b"ATGC-")
    with pytest.raises(GibbsError) as e:
        c.motif_sweep(64, PC, CUT, np.full(4, -1, np.int32), np.full(4, 0.5))
    assert e.value.status == GS_E_UNSUPPORTED
    m = re.search(r"up to (\d+)", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


# ---- comparisons ----------------------------------------------------------------------
def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    eq = g == o  # also equal infinities
    with np.errstate(invalid="ignore"):
        rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(eq | (rel <= RTOL)))


def same(g, o, what):
    (gpos, gpw), (opos, opw) = g, o[:2]
    bad = np.nonzero(gpos != opos)[0]
    assert bad.size == 0, f"{what}: {bad.size} positions differ, first {bad[:8]}: gpu {gpos[bad[:8]]} oracle {opos[bad[:8]]}"
    assert close(gpw, opw), f"{what}: PWMS differ"


def ran(c, what, **want):
    """gs_sweep_kernel ran with this launch (ek, gl, waves, one)."""
    assert c.sweep_kernel_name() == "gs_sweep_kernel", what
    launch = c.last_sweep_launch()
    for k, v in want.items():
        assert launch[k] == v, (what, k, v, launch)


def want_waves(alpha, codes, W, Lmax, limit):
    """The wavefronts a workgroup of the general layout's automatic launch under `limit`."""
    E = len(np.unique(np.concatenate([codes, np.frombuffer(bytes(alpha), np.uint8)])))
    w = wd.auto_waves(len(alpha), E, W, Lmax, limit)
    assert w is not None, (alpha, W, Lmax, limit)
    return w


def sweep_both_scans(c, alpha, codes, offsets, W, pos, u, o, limit, what, gl=None):
    """One synchronous sweep with the certified scan and one with the exact scan."""
    assert np.min(o[2]) >= MARGIN, (what, float(np.min(o[2])))
    Lmax = int(np.diff(offsets).max())
    E = len(np.unique(np.concatenate([codes, np.frombuffer(bytes(alpha), np.uint8)])))
    gl = gl or wd.group_lanes(E, Lmax)
    assert gl == wd.group_lanes(E, Lmax), what
    for exact in (False, True):
        c.set_scan_mode(exact=exact)
        try:
            g = c.motif_sweep(W, PC, CUT, pos, u)
        finally:
            c.set_scan_mode(exact=False)
        ek = wd.expect_ek(alpha, W, exact)
        waves = 4 if ek == 4 else want_waves(alpha, codes, W, Lmax, limit)
        ran(c, what, ek=ek, gl=gl, waves=waves)
        same(g, o, f"{what}, {'exact' if exact else 'certified'} scan")


# ---- all widths, the general sweep ------------------------------------------------------
@pytest.mark.parametrize("W", wd.ALL_W)
@pytest.mark.parametrize("name", ["dna", "atgc5", "protein"])
def test_all_widths(ctxs, lds_limit, name, W):
    """W = 1..64, N = 24, L <= W + 70: from the initialiser's positions (motif picks) and
    from uniform positions with a third of them -1 (mostly background picks), the
    certified and the exact scan."""
    s = wd.snap(name, W)
    c = ctxs(dna_mode=0)
    c.set_sequences(s.codes, s.offsets, s.alpha)
    for kind, pos, o in s.starts():
        sweep_both_scans(c, s.alpha, s.codes, s.offsets, W, pos, s.u, o, lds_limit,
                         f"{name} W = {W}, {kind} starts")


def test_subnormal_window_scores(ctxs, lds_limit):
    """ATGC-, N = 32, W = 64, every position -1: the window scores are binary64
    subnormals and the background products below the binary32 range."""
    codes, offsets, seqs, pos, u = wd.all_none()
    c = ctxs(dna_mode=0, bg_mode=0)
    c.set_sequences(codes, offsets, b"ATGC-")
    o = ol.sweep(seqs, 64, PC, CUT, pos, u)
    sweep_both_scans(c, b"ATGC-", codes, offsets, 64, pos, u, o, lds_limit, "all -1, W = 64")
    assert (o[0] == -1).all()


# ---- lanes per sequence ---------------------------------------------------------------
LANES_CASES = ([("atgc5", W, gl) for W in LANES_ATGC5 for gl in (16, 32, 64)] +
               [("dna", W, gl) for W in LANES_EK4 for gl in (16, 32, 64)] +
               [("protein", W, gl) for W in LANES_PROTEIN for gl in (32, 64)])


@pytest.mark.parametrize("name,W,gl", LANES_CASES)
def test_lanes_per_sequence(ctxs, lds_limit, name, W, gl):
    """GL = 16, 32, 64 through Lmax (200, 400, 700); N = 11, the last sequence the longest."""
    alpha = wd.ALPHAS[name]
    codes, offsets, planted = wd.lanes_dataset(11, LANES_LMAX[gl], W, alpha, 500 + W + gl)
    assert int(np.argmax(np.diff(offsets))) == 10
    seqs = ol.Seqs(codes, offsets, alpha)
    pos = wd.mixed_starts(planted, 501 + W)
    u = np.random.default_rng(502 + W + gl).random(11)
    o = ol.sweep(seqs, W, PC, CUT, pos, u)
    assert (o[0] >= 0).sum() >= 4 and (pos < 0).sum() >= 1
    c = ctxs(dna_mode=0)
    c.set_sequences(codes, offsets, alpha)
    sweep_both_scans(c, alpha, codes, offsets, W, pos, u, o, lds_limit, f"{name} W = {W}, {gl} lanes", gl=gl)


# ---- the four-symbol kernel, both paths -------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("gl", [16, 32, 64])
@pytest.mark.parametrize("W", EK4_PATHS_W)
def test_four_symbol_kernel_both_paths(ctxs, W, gl):
    """sweep_one 0 and 1 (the loop and the one-iteration path): one sweep bit-identical and
    the oracle's, and a 3-sweep motif_run equal to three oracle sweeps.  W = 20, 24, 28
    are the widths whose table build does not split the motif cells (4 WM > 64)."""
    alpha, N = b"ACGT", 11
    codes, offsets, planted = wd.lanes_dataset(N, LANES_LMAX[gl], W, alpha, 600 + W + gl)
    seqs = ol.Seqs(codes, offsets, alpha)
    pos = wd.mixed_starts(planted, 601 + W)
    u = np.random.default_rng(602 + W + gl).random(N)
    o = ol.sweep(seqs, W, PC, CUT, pos, u)
    assert np.min(o[2]) >= MARGIN and (o[0] >= 0).sum() >= 4
    oc, ow = pos, None
    for t in range(3):
        oc, ow, mg = ol.sweep(seqs, W, PC, CUT, oc, uniforms(96, ol.stream_sweep(t), N))
        assert np.min(mg) >= MARGIN
    out = []
    for one in (0, 1):
        c = ctxs(dna_mode=0, sweep_one=one, bg_mode=0)
        c.set_sequences(codes, offsets, alpha)
        g = c.motif_sweep(W, PC, CUT, pos, u)
        ran(c, f"W = {W}, one = {one}", ek=4, gl=gl, waves=4, one=one)
        same(g, o, f"four symbols W = {W}, {gl} lanes, one = {one}")
        r = c.motif_run(W, PC, CUT, 3, 96, pos)
        ran(c, f"W = {W}, one = {one}, chain", ek=4, gl=gl, waves=4, one=one)
        same(r, (oc, ow), f"four symbols W = {W}, {gl} lanes, one = {one}, 3 sweeps")
        out.append((g, r))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (W, gl)


# ---- the wavefront ladder -----------------------------------------------------------------
def ladder_data(alpha, extra, W, seed):
    """LADDER_N = 261 ragged sequences: every wavefront of a workgroup has work and the
    last workgroup is partly empty."""
    codes, offsets, planted = wd.lanes_dataset(LADDER_N, W + 70, W, alpha, seed, extra=extra,
                                               extra_rate=0.03 if extra else 0.0)
    seqs = ol.Seqs(codes, offsets, alpha)
    pos = wd.mixed_starts(planted, seed + 1)
    u = np.random.default_rng(seed + 2).random(LADDER_N)
    return codes, offsets, pos, u, ol.sweep(seqs, W, PC, CUT, pos, u, threads=8)


@pytest.mark.parametrize("H,waves", [(2, 4), (2, 2), (2, 1), (1, 12), (1, 6), (1, 3)])
def test_wavefront_ladder(ctxs, lds_limit, H, waves):
    """The automatic launch at 4, 2, 1 wavefronts a workgroup (pair tables) and 12, 6, 3
    (H = 1): launch_sweep halves them until the carve fits the device's LDS.  On an
    MI355X (163840 B a workgroup): ladder_shapes' docstring names each shape."""
    shape = [s for s in ladder_shapes(lds_limit) if s[:2] == (H, waves)]
    assert shape, f"no candidate shape launches {waves} wavefronts (H = {H}) under {lds_limit} B"
    _, _, alpha, extra, W = shape[0]
    codes, offsets, pos, u, o = ladder_data(alpha, extra, W, 700 + 10 * H + waves)
    assert np.min(o[2]) >= MARGIN
    c = ctxs(dna_mode=0)
    c.set_sequences(codes, offsets, alpha)
    g = c.motif_sweep(W, PC, CUT, pos, u)
    ran(c, f"ladder H = {H}", ek=0, gl=16 if H == 2 else 32, waves=waves)
    assert c.last_sweep_launch()["grid"] > 1
    same(g, o, f"{alpha.decode()} + {extra.decode()!r} W = {W}: {waves} wavefronts")


@pytest.mark.parametrize("W", [8, 40])
@pytest.mark.parametrize("waves", [1, 2])
def test_pair_table_kernel_with_fewer_wavefronts(ctxs, waves, W):
    """The sweep_waves tuning at 1 and 2 for the pair tables' kernel (H = 2)."""
    codes, offsets, pos, u, o = ladder_data(b"ATGC-", b"", W, 750 + W)
    assert np.min(o[2]) >= MARGIN
    c = ctxs(dna_mode=0, sweep_waves=waves)
    c.set_sequences(codes, offsets, b"ATGC-")
    g = c.motif_sweep(W, PC, CUT, pos, u)
    ran(c, f"sweep_waves {waves}", ek=0, gl=16, waves=waves)
    same(g, o, f"ATGC- W = {W}, sweep_waves {waves}")


# ---- refusal --------------------------------------------------------------------------
def test_refused_shape_then_a_supported_one(ctxs, lds_limit):
    """ATGC- with eleven foreign symbols (E = 16: the pair tables at their largest), W = 64,
    Lmax = 300: the carve fits at no wavefront count, launch_sweep returns
    GS_E_UNSUPPORTED before any launch, and the context's next sweep is the oracle's."""
    from gibbssampling_amd._native import GS_E_UNSUPPORTED, GibbsError
    assert wd.auto_waves(5, 16, 64, 300, lds_limit) is None, lds_limit
    codes, offsets, planted = wd.lanes_dataset(6, 300, 64, b"ATGC-", 800, extra=FOREIGN11, extra_rate=0.05)
    assert len(np.unique(codes)) == 16
    c = ctxs(dna_mode=0)
    c.set_sequences(codes, offsets, b"ATGC-")
    pos = wd.mixed_starts(planted, 801)
    s0 = c.stats()
    with pytest.raises(GibbsError) as e:
        c.motif_sweep(64, PC, CUT, pos, np.random.default_rng(802).random(6))
    assert e.value.status == GS_E_UNSUPPORTED
    assert c.stats() == s0
    # the same data at a width the carve admits, then another alphabet
    for alpha, extra, W in ((b"ATGC-", FOREIGN11, 21), (b"ATGC-", b"", 64)):
        if extra == b"":
            codes, offsets, planted = wd.lanes_dataset(6, 300, W, alpha, 803)
            c.set_sequences(codes, offsets, alpha)
        seqs = ol.Seqs(codes, offsets, alpha)
        pos = np.where(planted + W <= np.diff(offsets), wd.mixed_starts(planted, 804), -1).astype(np.int32)
        u = np.random.default_rng(805).random(6)
        o = ol.sweep(seqs, W, PC, CUT, pos, u)
        assert np.min(o[2]) >= MARGIN
        g = c.motif_sweep(W, PC, CUT, pos, u)
        ran(c, "after the refusal", ek=0, gl=32, waves=want_waves(alpha, codes, W, 300, lds_limit))
        same(g, o, f"after the refusal, W = {W}")


# ---- greedy and site passes -----------------------------------------------------------------
_greedy = {}


def greedy_case(name, W, N=24, L=None):
    """Sequences, the oracle's sweep from the initialiser's positions (the motif memory,
    two targets without a motif) and the initialiser's (score, position) for the site
    passes, with the oracle's results of both: computed once."""
    key = (name, W, N, L)
    if key not in _greedy:
        alpha, extra = wd.ALPHAS[name], GREEDY_EXTRA[name]
        codes, offsets = make_dataset(N, L or W + 70, W, alpha, seed=900 + W, ragged=L is None, mut=0.15,
                                      extra=extra, extra_rate=0.04 if extra else 0.0)
        seqs = ol.Seqs(codes, offsets, alpha)
        sc0, p0 = ol.random_starts(seqs, W, PC, seed=9, mode=1)
        start = p0.astype(np.int32).copy()
        start[[1, N - 2]] = -1
        mp, mw, _ = ol.sweep(seqs, W, PC, CUT, start, np.random.default_rng(901 + W).random(N))
        _greedy[key] = dict(codes=codes, offsets=offsets, alpha=alpha, seqs=seqs, mem=(mp, mw),
                            greedy=ol.greedy(seqs, W, PC, CUT, mp, mw), start=(p0.astype(np.int32), sc0),
                            site={sh: ol.site_refine(seqs, W, PC, sh, p0, sc0) for sh in (0, -1, 1)})
    return _greedy[key]


def check_greedy(g, o, what):
    assert np.array_equal(g[0], o[0]), f"{what}: positions differ at {np.nonzero(g[0] != o[0])[0][:8]}"
    assert g[2] == o[2], f"{what}: passes {g[2]} vs {o[2]}"
    assert close(g[1], o[1]), f"{what}: scores differ"


@pytest.mark.parametrize("tuning", list(GREEDY_TUNINGS))
@pytest.mark.parametrize("name,W", [(n, W) for n, ws in GREEDY_W.items() for W in ws])
def test_greedy_and_site_passes(ctxs, name, W, tuning):
    """motif_greedy from the oracle's sweep output and the three site refinements from the
    initialiser's, at the default tuning and at 1, 2 and 8 wavefronts (protein at W = 64
    cannot hold eight wavefronts' tables: greedy_carve gives it 4)."""
    k = greedy_case(name, W)
    c = ctxs(**GREEDY_TUNINGS[tuning])
    c.set_sequences(k["codes"], k["offsets"], k["alpha"])
    what = f"{name} W = {W}, {tuning}"
    check_greedy(c.motif_greedy(W, PC, CUT, *k["mem"]), k["greedy"], what + ", motif greedy")
    Cg, Tg = c.counts(W, k["greedy"][0], len(k["alpha"]))
    Co, To = ol.counts(k["seqs"], W, k["greedy"][0])
    assert np.array_equal(Cg, Co) and np.array_equal(Tg, To), what
    for sh in (0, -1, 1):
        check_greedy(c.site_refine(W, PC, sh, *k["start"]), k["site"][sh], what + f", site shift {sh}")


@pytest.mark.parametrize("name,W", COOP)
def test_greedy_whole_workgroup_visits(ctxs, name, W):
    """kMotifCoop (WM >= 16): every visit scored by the whole workgroup (motif_coop 1), the
    star engine for every pass (greedy_switch 0)."""
    k = greedy_case(name, W)
    c = ctxs(motif_coop=1, greedy_switch=0)
    c.set_sequences(k["codes"], k["offsets"], k["alpha"])
    check_greedy(c.motif_greedy(W, PC, CUT, *k["mem"]), k["greedy"], f"{name} W = {W}, motif_coop 1")


@pytest.mark.parametrize("L,dt16", [(1100, 1), (134, 0)])
def test_site_passes_with_the_int32_table(ctxs, L, dt16):
    """Lmax W >= 65536 at W = 64 (N = 6, L = 1100): the site passes' D table holds int32
    entries; and the same layout through site_dt16 0 at a small L."""
    W = 64
    assert (L * W >= 65536) == bool(dt16)
    k = greedy_case("dna", W, N=6, L=L)
    c = ctxs(site_dt16=dt16)
    c.set_sequences(k["codes"], k["offsets"], k["alpha"])
    for sh in (0, -1, 1):
        check_greedy(c.site_refine(W, PC, sh, *k["start"]), k["site"][sh], f"L = {L}, site shift {sh}")


# ---- everything else once at the top --------------------------------------------------------
TOP = [(n, W) for n in ("dna", "protein") for W in TOP_W]
SEEDS = (11, 12, 13)


def load_top(ctxs, name, W, **tuning):
    s = wd.snap(name, W)
    c = ctxs(**tuning)
    c.set_sequences(s.codes, s.offsets, s.alpha)
    c.set_fixed_pcv(None)
    c.set_fixed_ppm(None)
    return s, c


def pcv49(alpha, seed):
    """tests/test_gpu_variants.py's ProbabilityCompositeVector."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.6, 49)
    v[[a - 42 for a in alpha]] = rng.dirichlet(np.ones(len(alpha)))
    return v


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name,W", TOP)
def test_initialiser(ctxs, name, W, mode):
    s, c = load_top(ctxs, name, W)
    gs, gp = c.random_starts(W, PC, 77, mode)
    os_, op = ol.random_starts(s.seqs, W, PC, seed=77, mode=mode)
    assert np.array_equal(gp, op) and close(gs, os_), f"{name} W = {W} mode {mode}"
    bs, bp, st = c.random_starts_batch(W, PC, SEEDS, mode)
    assert not st.any()
    for r, seed in enumerate(SEEDS):
        ss, sp = c.random_starts(W, PC, seed, mode)
        assert np.array_equal(bp[r], sp) and close(bs[r], ss), (name, W, mode, seed)
        os_, op = ol.random_starts(s.seqs, W, PC, seed=seed, mode=mode)
        assert np.array_equal(bp[r], op) and close(bs[r], os_), (name, W, mode, seed)


@pytest.mark.parametrize("name,W", TOP)
def test_best_pwms(ctxs, name, W):
    s, c = load_top(ctxs, name, W)
    rng = np.random.default_rng(40 + W)
    fcv = np.zeros(49, np.int64)
    ppm = np.zeros((49, W))
    for a in s.alpha:
        fcv[a - 42] = rng.integers(200, 400)
        ppm[a - 42] = rng.random(W) + 1e-3
    ppm /= ppm.sum(0, keepdims=True)
    for n in range(s.N):
        want = ol.best_pwms(s.seqs, W, PC, n, fcv, ppm[[a - 42 for a in s.alpha]])
        got = c.best_pwms(W, PC, n, fcv, ppm)
        assert got[1] == want[1] and close([got[0]], [want[0]]), f"{name} W = {W} target {n}: {got} vs {want}"


@pytest.mark.parametrize("name,W", TOP)
def test_by_pcv_sweep_and_greedy(ctxs, lds_limit, name, W):
    s, c = load_top(ctxs, name, W, dna_mode=0)
    pcv = pcv49(s.alpha, W)
    c.set_fixed_pcv(pcv)
    try:
        pos = ol.random_starts(s.seqs, W, PC, seed=5, mode=1, pcv49=pcv)[1].astype(np.int32)
        pos[[2, s.N - 3]] = -1
        op, ow, mg = ol.sweep_pcv(s.seqs, W, PC, CUT, pcv, pos, s.u)
        assert np.min(mg) >= MARGIN
        g = c.motif_sweep(W, PC, CUT, pos, s.u)
        ran(c, "ByPCV", ek=0, gl=wd.group_lanes(len(s.alpha), s.Lmax),
            waves=want_waves(s.alpha, s.codes, W, s.Lmax, lds_limit))
        same(g, (op, ow), f"{name} W = {W} ByPCV sweep")
        check_greedy(c.motif_greedy(W, PC, CUT, op, ow), ol.greedy_pcv(s.seqs, W, PC, CUT, pcv, op, ow),
                     f"{name} W = {W} ByPCV greedy")
    finally:
        c.set_fixed_pcv(None)


def oracle_motif_sampling(S, W, seed, mode):
    p = ol.random_starts(S, W, PC, seed=seed, mode=mode)[1]
    p1, w1, mg = ol.sweep(S, W, PC, CUT, p, uniforms(seed, ol.stream_sweep(0), S.n))
    assert np.min(mg) >= MARGIN, (seed, float(np.min(mg)))
    return ol.greedy(S, W, PC, CUT, p1, w1)


def oracle_site_sampling(S, W, seed, mode):
    sc, p = ol.random_starts(S, W, PC, seed=seed, mode=mode)
    passes = []
    for shift in (0, -1, 1):
        p, sc, n = ol.site_refine(S, W, PC, shift, p, sc)
        passes.append(n)
    return p, sc, passes


@pytest.mark.parametrize("name,W", TOP)
def test_drivers_and_their_batches(ctxs, lds_limit, name, W):
    """motif_sampling and site_sampling against the oracle's composition of the stages, and
    the batched drivers with three seeds against their single-chain calls."""
    s, c = load_top(ctxs, name, W)
    waves = want_waves(s.alpha, s.codes, W, s.Lmax, lds_limit)
    gl = wd.group_lanes(len(s.alpha), s.Lmax)
    single = {}
    for seed in SEEDS:
        gp, gw, gpass = c.motif_sampling(W, PC, CUT, seed, 1)
        ran(c, "motif_sampling", ek=0, gl=gl, waves=waves)
        check_greedy((gp, gw, gpass), oracle_motif_sampling(s.seqs, W, seed, 1), f"{name} W = {W} motif_sampling {seed}")
        sp, ssc, spass = c.site_sampling(W, PC, seed, 1)
        op, osc, opass = oracle_site_sampling(s.seqs, W, seed, 1)
        assert np.array_equal(sp, op) and list(spass) == opass and close(ssc, osc), (name, W, seed)
        single[seed] = (gp, gw, gpass, sp, ssc, spass)
    bp, bw, bpass, st = c.motif_sampling_batch(W, PC, CUT, SEEDS, 1)
    assert not st.any()
    qp, qsc, qpass, st = c.site_sampling_batch(W, PC, SEEDS, 1)
    assert not st.any()
    for r, seed in enumerate(SEEDS):
        gp, gw, gpass, sp, ssc, spass = single[seed]
        assert np.array_equal(bp[r], gp) and bpass[r] == gpass and close(bw[r], gw), (name, W, seed)
        assert np.array_equal(qp[r], sp) and np.array_equal(qpass[r], spass) and close(qsc[r], ssc), (name, W, seed)


@pytest.mark.parametrize("name,W", TOP)
def test_run_batch(ctxs, lds_limit, name, W):
    """motif_run_batch with three seeds: each row its motif_run from that seed's starts, and
    three oracle sweeps."""
    s, c = load_top(ctxs, name, W, dna_mode=0)
    T = 3
    bp, bw, st = c.motif_run_batch(W, PC, CUT, T, SEEDS, init_mode=1)
    assert not st.any()
    for r, seed in enumerate(SEEDS):
        start = c.random_starts(W, PC, seed, 1)[1]
        gp, gw = c.motif_run(W, PC, CUT, T, seed, start)
        ran(c, "motif_run", ek=0, gl=wd.group_lanes(len(s.alpha), s.Lmax),
            waves=want_waves(s.alpha, s.codes, W, s.Lmax, lds_limit))
        assert np.array_equal(bp[r], gp) and close(bw[r], gw), (name, W, seed)
        op, ow = ol.random_starts(s.seqs, W, PC, seed=seed, mode=1)[1], None
        for t in range(T):
            op, ow, mg = ol.sweep(s.seqs, W, PC, CUT, op, uniforms(seed, ol.stream_sweep(t), s.N))
            assert np.min(mg) >= MARGIN
        same((bp[r], bw[r]), (op, ow), f"{name} W = {W} run_batch seed {seed}")


def check_lists(g, o, what):
    gc, gp, gw = g[:3]
    oc, op, ow = o[:3]
    assert np.array_equal(gc, oc), f"{what}: list lengths differ at {np.nonzero(gc != oc)[0][:8]}"
    for n in range(len(gc)):
        assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), (what, n)
    assert close(gw, ow), what
    if len(g) > 3:
        assert g[3] == o[3], (what, g[3], o[3])


@pytest.mark.parametrize("name,W", TOP)
def test_list_path_with_pairs(ctxs, name, W):
    """motifAmount 2 on sequences that hold two occurrences each: the list sweep, the list
    greedy and a 3-sweep motif_run_multi; pairs are picked (asserted)."""
    codes, offsets, seqs, cnt, pos, u = wd.list_fixture(name, W)
    c = ctxs()
    c.set_sequences(codes, offsets, wd.ALPHAS[name])
    c.set_fixed_pcv(None)
    c.set_fixed_ppm(None)
    oc, op, ow = ol.sweep_lists(seqs, 2, W, PC, CUT, cnt, pos, 2, u)
    assert int((oc == 2).sum()) >= 4
    check_lists(c.motif_sweep_multi(2, W, PC, CUT, cnt, pos, u), (oc, op, ow), f"{name} W = {W} list sweep")
    o = ol.greedy_lists(seqs, 2, W, PC, CUT, oc, op, 2, ow)
    assert int((o[0] == 2).sum()) >= 4
    check_lists(c.motif_greedy_multi(2, W, PC, CUT, oc, op, ow), o, f"{name} W = {W} list greedy")
    rc, rp, rw = cnt, pos, None
    for t in range(3):
        rc, rp, rw = ol.sweep_lists(seqs, 2, W, PC, CUT, rc, rp, 2, uniforms(97, ol.stream_sweep(t), seqs.n))
    check_lists(c.motif_run_multi(2, W, PC, CUT, 3, 97, cnt, pos), (rc, rp, rw), f"{name} W = {W} motif_run_multi")
