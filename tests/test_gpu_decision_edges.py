"""Decision-boundary parity of every sweep kernel's certified pick.

Every sweep kernel decides most targets from an approximate scan (fixed-point or
binary32 window scores, DPP prefix sums, a Newton-refined reciprocal) and accepts a
decision only when an error bound certifies it: the cut-off band cutOff +- epsS and the
roulette band delta = delta_round + delta_approx around every CDF edge.  Uniform u never
comes near an edge, so these tests put u there: on the reference's own acc_c and one ulp
either side of it where no log enters the weights (log-free snapshots), at d = 1e-11 ..
1e-3 from it where motif categories do -- from just beyond what a 1e-12 relative log
error can move an edge to beyond the widest band -- and the cut-off at d = 1e-9 .. 1e-3
from a window's log2 score.  tests/decision_edges.py builds the probes from the oracle
and states which are legitimate; tests/test_decision_edges_host.py checks that
construction on the CPU.  One sweep probes one edge per target, the kinds rotating over
n mod 6 (phase edge, lane-block join, chunk join, random, first / last, motif edge).

Bar: positions identical to the oracle's, no tolerance and no target left out; PWMS
within 1e-12 relative, infinities equal; on an edge the fallbacks must have run;
rescan_recheck and desc_oob stay 0.
"""
import numpy as np
import pytest

import decision_edges as de
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12

# name: tuning, what to do to the context after set_sequences, the kernel that must
# run (gs_sweep_kernel rows: the launch's ek / gl / one as well), the lane-block
# geometry of its scan, and the shapes (decision_edges.SHAPES; the first one also takes
# the cut-off probes)
ROWS = {
    "general": dict(tuning={"dna_mode": 0}, kernel="gs_sweep_kernel", launch={"ek": 0, "gl": 16},
                    geo=de.geometry_groups(16, quad=True), shapes=["atgc5", "atgc5_w64", "dna_w61", "pcv_w40"]),
    "ek4_loop": dict(tuning={"dna_mode": 0, "sweep_one": 0, "bg_mode": 0}, kernel="gs_sweep_kernel",
                     launch={"ek": 4, "gl": 16, "one": 0}, geo=de.geometry_groups(16, quad=True),
                     shapes=["dna12", "dna_w28", "dna_w20"]),
    "ek4_one": dict(tuning={"dna_mode": 0, "sweep_one": 1, "bg_mode": 0}, kernel="gs_sweep_kernel",
                    launch={"ek": 4, "gl": 16, "one": 1}, geo=de.geometry_groups(16, quad=True),
                    shapes=["dna12", "dna_w28", "dna_w20"]),
    "ek4_gl32": dict(tuning={"dna_mode": 0, "sweep_one": 0}, kernel="gs_sweep_kernel",
                     launch={"ek": 4, "gl": 32, "one": 0}, geo=de.geometry_groups(32),
                     shapes=["dna8_300", "dna_w24_300"]),
    "protein": dict(tuning={}, kernel="gs_sweep_kernel", launch={"ek": 0, "gl": 32},
                    geo=de.geometry_groups(32), shapes=["protein", "protein_w64", "protein_w41"]),
    # the binary64-for-every-window scan: one 64-lane group a target, the band is rounding only
    "general_exact": dict(tuning={"dna_mode": 0}, exact=True, kernel="gs_sweep_kernel", launch={"ek": 0},
                          geo=de.geometry_groups(64), shapes=["atgc5", "atgc5_w64"]),
    "protein_exact": dict(tuning={}, exact=True, kernel="gs_sweep_kernel", launch={"ek": 0},
                          geo=de.geometry_groups(64), shapes=["protein", "protein_w64"]),
    "long": dict(tuning={"dna_mode": 1, "long_mode": 1}, kernel="gs_sweep_long_kernel",
                 geo=de.geometry_long(), shapes=["dna15_526", "dna12_300"]),
    "live1": dict(tuning={"live_mode": 1, "live_G": 1}, kernel="gs_sweep_live_kernel",
                  geo=de.geometry_packed(1), shapes=["dna12"]),
    "live4": dict(tuning={"live_mode": 1, "live_G": 4}, kernel="gs_sweep_live_kernel",
                  geo=de.geometry_packed(4), shapes=["dna12", "dna13_300"]),
    "dna1": dict(tuning={"dna_mode": 1, "live_mode": 0, "dna_G": 1}, kernel="gs_sweep_dna_kernel",
                 geo=de.geometry_packed(1), shapes=["dna12"]),
    "dna4": dict(tuning={"dna_mode": 1, "live_mode": 0, "dna_G": 4}, kernel="gs_sweep_dna_kernel",
                 geo=de.geometry_packed(4), shapes=["dna12", "dna13_300"]),
    "pcv": dict(tuning={}, kernel="gs_sweep_kernel", geo=de.geometry_groups(16, quad=True),
                shapes=["pcv10"]),
}
# the all-background kernel: log-free snapshots only (every position -1)
BG_ROWS = {f"bg{g}": dict(tuning={"bg_mode": 1, "bg_G": g}, geo=de.geometry_packed(g), shapes=["dna12"])
           for g in (1, 8, 64)}
# the kernels whose serial replay follows their binary64 rescan: both counters rise
RESCAN_FIRST = {"gs_sweep_kernel", "gs_sweep_long_kernel", "gs_sweep_live_kernel", "gs_sweep_dna_kernel"}

CASES = [(r, s) for r, row in ROWS.items() for s in row["shapes"]]
# the wide shapes (W = 20 .. 64) take the cut-off probes in every row they are in
WIDE = ("atgc5_w64", "dna_w61", "dna_w28", "dna_w20", "dna_w24_300", "protein_w64", "protein_w41", "pcv_w40")
CUT_CASES = [(r, s) for r, row in ROWS.items() for i, s in enumerate(row["shapes"]) if i == 0 or s in WIDE]
# the alphabet's wavefronts a workgroup (gs_common.h sweep_waves) where the LDS carve cannot
# hold them: these shapes launch fewer (launch_sweep halves them until the workgroup fits)
FEWER_WAVES = {"atgc5_w64": 4, "protein_w64": 12}


@pytest.fixture(scope="module")
def ctxs():
    """One Context per row, created on first use."""
    from gibbssampling_amd import Context
    made = {}

    def get(row):
        if row not in made:
            made[row] = Context(0, tuning={**ROWS, **BG_ROWS}[row]["tuning"])
        return made[row]

    yield get
    for name, c in made.items():
        st = c.stats()
        c.close()
        assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, (name, st)


def load(ctxs, row, snap, bg_off=False):
    """The row's context holding the snapshot's sequences (bg_off: the all-background
    takeover off, so that the row's own kernel walks a log-free snapshot)."""
    spec = {**ROWS, **BG_ROWS}[row]
    c = ctxs(row)
    c.set_tuning("bg_mode", 0 if bg_off else spec["tuning"].get("bg_mode", -1))
    c.set_sequences(snap.codes, snap.offsets, snap.alpha)
    c.set_fixed_pcv(snap.pcv)  # (None clears the one a row's earlier shape set)
    c.set_scan_mode(exact=bool(spec.get("exact")))
    return c, spec


def ran(c, spec, row, shape=None):
    """The intended kernel and path ran."""
    if "kernel" not in spec:
        return
    assert c.sweep_kernel_name() == spec["kernel"], row
    if spec["kernel"] == "gs_sweep_kernel":
        launch = c.last_sweep_launch()
        for k, v in spec.get("launch", {}).items():
            assert launch[k] == v, (row, launch)
        if shape in FEWER_WAVES:
            assert 1 <= launch["waves"] < FEWER_WAVES[shape], (row, shape, launch)


def same(g, o, what):
    (gpos, gpw), (opos, opw) = g, o[:2]
    bad = np.nonzero(gpos != opos)[0]
    assert bad.size == 0, f"{what}: {bad.size} positions differ, first {bad[:8]}: gpu {gpos[bad[:8]]} oracle {opos[bad[:8]]}"
    eq = gpw == opw  # also equal infinities
    with np.errstate(invalid="ignore"):
        rel = np.abs(gpw - opw) / np.maximum(np.abs(opw), 1e-300)
    assert np.all(eq | (rel <= RTOL)), f"{what}: PWMS rel diff {np.nanmax(rel[~eq]):.3e}"


def delta(c, s0):
    s1 = c.stats()
    return {k: s1[k] - s0[k] for k in s1}


@pytest.mark.parametrize("row,shape", CASES)
def test_roulette_edges_at_distance(ctxs, row, shape):
    """u = acc_c +- d on a snapshot with motif categories: every probe is one the
    reference decides whatever the last place of a log (asserted), the restatement and
    the oracle agree on it, and the kernel picks the same."""
    snap = de.snapshot(shape)
    c, spec = load(ctxs, row, snap)
    cs, kind = de.choose_edges(snap.ts, spec["geo"], seed=5)
    edges = de.edge_values(snap.ts, cs)
    for d in de.D_ROULETTE:
        for sign, u in zip("+-", de.probes_at_distance(snap.ts, cs, d)):
            assert de.ambiguous(snap.ts, u) == [], (shape, d)
            o = snap.oracle(u)
            rpos, rmg = de.restated(snap.ts, u)
            assert np.array_equal(rpos, o[0]) and np.array_equal(rmg, np.asarray(o[2]))
            assert (rmg <= np.abs(u - edges)).all()
            g = c.motif_sweep(snap.W, de.PC, snap.cutoff, snap.pos, u)
            ran(c, spec, row, shape)
            same(g, o, f"{row} {shape} u = acc_c {sign} {d:g} (kinds {kind[:6]}...)")
    st = c.stats()
    assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st


@pytest.mark.parametrize("row,shape", CASES + [(r, "dna12") for r in BG_ROWS])
def test_log_free_edges(ctxs, row, shape):
    """Every position -1: the weights are products, bit-identical on host and device, so
    u sits on the reference's own acc_c, on the doubles next to it, at 0.0 and on the
    final acc of a target whose wheel ends below 1 - 2^-53.  On an edge no prefix-sum
    order can certify the pick: the serial replay must have taken every target (and the
    binary64 rescan before it in the kernels that have one); one ulp past the final acc
    the wheel runs off its end in the reference and in the library."""
    from gibbssampling_amd import RouletteOverrunError
    snap = de.snapshot(shape, logfree=True)
    bg = row in BG_ROWS
    c, spec = load(ctxs, row, snap, bg_off=not bg)
    cs, _ = de.choose_edges(snap.ts, spec["geo"], seed=6)
    probes, short = de.logfree_probes(snap, cs)
    assert len(short) == 2
    for key, u in probes.items():
        o = snap.oracle(u)
        rpos, rmg = de.restated(snap.ts, u)
        assert np.array_equal(rpos, o[0]) and np.array_equal(rmg, np.asarray(o[2]))
        assert (o[0] == -1).all()
        s0 = c.stats()
        g = c.motif_sweep(snap.W, de.PC, snap.cutoff, snap.pos, u)
        dl = delta(c, s0)
        ran(c, spec, row, shape)
        same(g, o, f"{row} {shape} log-free, u {key} the edge")
        if bg:
            assert dl["bg_path"] == snap.N, dl
        if key == "on":
            assert (rmg == 0.0).all()
            assert dl["serial_picks"] >= snap.N, (row, dl)
            if spec.get("kernel") in RESCAN_FIRST:
                assert dl["exact_rescans"] >= snap.N, (row, dl)
    # the wheel runs off its end one ulp past the final acc: an error return with the
    # target's index, and the next snapshot sweeps clean
    n = short[0]
    bad = snap.random_u(1)
    bad[n] = np.nextafter(snap.ts[n].acc_last, 1.0)
    with pytest.raises(ol.OracleError) as eo:
        snap.oracle(bad)
    assert eo.value.code == ol.GO_E_ROULETTE_OVERRUN and eo.value.index == n
    with pytest.raises(RouletteOverrunError) as eg:
        c.motif_sweep(snap.W, de.PC, snap.cutoff, snap.pos, bad)
    assert eg.value.index == n
    u = snap.random_u(2)
    same(c.motif_sweep(snap.W, de.PC, snap.cutoff, snap.pos, u), snap.oracle(u), f"{row} after the overrun")
    st = c.stats()
    assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st


@pytest.mark.parametrize("row,shape", CUT_CASES)
def test_cutoff_edges(ctxs, row, shape):
    """The cut-off d above and below a window's log2 score (never on it: the device's
    log may differ in the last place), nothing else nearer than d / 2 (asserted): the
    target's best window, its weakest passing and strongest failing one at cut-off 1 (where
    the shape has one: decision_edges.CUTOFF_KEYS), a window of a target without a motif, and
    the snapshot's maximum -- just above it no
    target has a motif category, just below one target has one."""
    snap = de.snapshot(shape)
    c, spec = load(ctxs, row, snap)
    wins = de.cutoff_windows(snap.ts, snap.pos)
    assert set(wins) == de.CUTOFF_KEYS[shape]
    u = snap.random_u(3)
    for key, (n, k, l2) in wins.items():
        for d in de.D_CUTOFF:
            for cut in (l2 + d, l2 - d):
                assert de.cutoff_clearance(snap.ts, cut) >= d / 2, (key, d)
                o = snap.oracle(u, cutoff=cut)
                g = c.motif_sweep(snap.W, de.PC, cut, snap.pos, u)
                ran(c, spec, row, shape)
                same(g, o, f"{row} {shape} cut-off = l2[{n}][{k}] {cut - l2:+.1e} ({key})")
                if key == "global_max" and cut > l2:
                    assert (g[0] == -1).all()
        # the nearest pair once more with the probed target's u in the middle of the
        # probed window's own category: the reference picks that window just below its
        # score, and cannot just above
        d = de.D_CUTOFF[0]
        t = de.at_cutoff(snap.ts, l2 - d)[n]
        i = t.K + int(np.nonzero(t.win == k)[0][0])
        aimed = u.copy()
        aimed[n] = 0.5 * (t.acc[i] + t.acc[i + 1])
        for cut in (l2 + d, l2 - d):
            assert de.at_cutoff(snap.ts, cut)[n].unambiguous(float(aimed[n]))
            o = snap.oracle(aimed, cutoff=cut)
            assert (o[0][n] == k) == (cut < l2)
            g = c.motif_sweep(snap.W, de.PC, cut, snap.pos, aimed)
            same(g, o, f"{row} {shape} cut-off = l2[{n}][{k}] {cut - l2:+.1e} ({key}), u aimed at the window")
    st = c.stats()
    assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st


def test_list_path_edges(ctxs):
    """motifAmount = 2 (gs_multi_sweep_kernel's roulette): the edges by bisection on the
    oracle's own sweep -- two adjacent doubles with different picks -- and u at d beyond
    them (the pairs' weights hold logs: no probe on an edge)."""
    from gibbssampling_amd import Context
    N, L, W, M = 24, 60, 6, 2
    codes, offsets = de.dataset(N, L, W, b"ACGT", seed=21)
    S = ol.Seqs(codes, offsets, b"ACGT")
    cnt, pos = de.list_snapshot(S, W, M, seed=22)
    lo, hi = de.bisect_list_edges(S, M, W, de.PC, de.CUT, cnt, pos, M, seed=23)
    assert ((hi > lo) & (hi - lo <= 2.0 ** -53)).all()
    c = Context(0)
    try:
        c.set_sequences(codes, offsets, b"ACGT")
        for d in de.D_ROULETTE:
            for u in de.list_probes(lo, hi, d):
                (oc, op), opw, mg, _ = de.list_picks(S, M, W, de.PC, de.CUT, cnt, pos, M, u)
                assert (mg <= d + 2.0 ** -52).all()
                gc, gp, gpw = c.motif_sweep_multi(M, W, de.PC, de.CUT, cnt, pos, u)
                assert np.array_equal(gc, oc), (d, np.nonzero(gc != oc)[0][:8])
                for n in range(N):
                    assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), (d, n)
                eq = gpw == opw
                rel = np.abs(gpw - opw) / np.maximum(np.abs(opw), 1e-300)
                assert np.all(eq | (rel <= RTOL)), (d, np.nanmax(rel))
        st = c.stats()
        assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st
    finally:
        c.close()
