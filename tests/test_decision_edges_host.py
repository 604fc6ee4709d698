"""The decision-boundary probes' construction against the oracle, on the CPU
(tests/decision_edges.py, the helper of tests/test_gpu_decision_edges.py).

For every snapshot the GPU module probes: the helper's restatement of the category list
and the CDF edges picks what ol.sweep / ol.sweep_pcv pick at every probe, its margin is
the oracle's margin bit for bit (and never more than the probe's distance from its edge,
which it equals whenever no other walked edge lies nearer), and every probe of a
snapshot with motif categories keeps its pick when the motif weights move by 1e-12
relative -- the bound the device's log is held to.
"""
import numpy as np
import pytest

import decision_edges as de
from oracle import oracle_lib as ol

GEO = {
    "atgc5": de.geometry_groups(16, quad=True),
    "dna12": de.geometry_groups(16, quad=True),
    "dna8_300": de.geometry_groups(32),
    "dna13_300": de.geometry_packed(4),
    "dna12_300": de.geometry_long(),
    "dna15_526": de.geometry_long(),
    "protein": de.geometry_groups(16),
    "pcv10": de.geometry_groups(16, quad=True),
    "atgc5_w64": de.geometry_groups(16, quad=True),
    "dna_w61": de.geometry_groups(16, quad=True),
    "dna_w28": de.geometry_groups(16, quad=True),
    "dna_w20": de.geometry_groups(16, quad=True),
    "dna_w24_300": de.geometry_groups(32),
    "protein_w64": de.geometry_groups(32),
    "protein_w41": de.geometry_groups(32),
    "pcv_w40": de.geometry_groups(16, quad=True),
}


def check_probe(snap, u, dist=None):
    rpos, rmg = de.restated(snap.ts, u)
    opos, _, omg = snap.oracle(u)
    assert np.array_equal(rpos, opos), np.nonzero(rpos != opos)[0][:8]
    assert np.array_equal(rmg, np.asarray(omg)), np.nonzero(rmg != omg)[0][:8]
    if dist is not None:
        assert (rmg <= dist).all()
    return rmg


@pytest.mark.parametrize("name", sorted(de.SHAPES))
def test_restatement_at_distance_probes(name):
    snap = de.snapshot(name)
    c, kind = de.choose_edges(snap.ts, GEO[name], seed=5)
    assert ((c >= 1) & (c < [t.ncat for t in snap.ts])).all()
    assert set(kind) >= {3, 4}
    for d in de.D_ROULETTE:
        for u in de.probes_at_distance(snap.ts, c, d):
            assert de.ambiguous(snap.ts, u) == [], (name, d)
            dist = np.abs(u - de.edge_values(snap.ts, c))
            mg = check_probe(snap, u, dist)
            # the margin is the probe's distance wherever its own edge is the nearest of
            # all (a larger d reaches past background categories narrower than d)
            nearest = np.array([np.min(np.abs(x - t.acc)) for t, x in zip(snap.ts, u)])
            own = dist == nearest
            assert (mg[own] == dist[own]).all()
            assert own.any()


@pytest.mark.parametrize("name", sorted(de.SHAPES))
def test_restatement_on_edges_of_log_free_snapshots(name):
    snap = de.snapshot(name, logfree=True)
    c, _ = de.choose_edges(snap.ts, GEO[name], seed=6)
    probes, short = de.logfree_probes(snap, c)
    assert len(short) == 2, "no target whose final acc is below 1 - 2^-53: choose another seed"
    for key, u in probes.items():
        mg = check_probe(snap, u)
        if key == "on":
            assert (mg == 0.0).all()
    # on an edge the reference picks the category that ends there; at u = 0 the first,
    # at u = acc_last the last
    on = probes["on"]
    for n, t in enumerate(snap.ts):
        want = 0 if n == 0 else t.ncat - 1 if n in short else int(c[n]) - 1
        assert t.pick(float(on[n])) == want
    # one ulp past the last edge the wheel runs off its end
    n = short[0]
    bad = snap.random_u(1)
    bad[n] = np.nextafter(snap.ts[n].acc_last, 1.0)
    assert snap.ts[n].pick(float(bad[n])) == -1
    with pytest.raises(ol.OracleError) as ei:
        snap.oracle(bad)
    assert ei.value.code == ol.GO_E_ROULETTE_OVERRUN and ei.value.index == n


@pytest.mark.parametrize("name", sorted(de.SHAPES))
def test_cutoff_probe_windows(name):
    """Every cut-off probe clears every other window of every target by d / 2 at least,
    and the restatement at that cut-off picks what the oracle picks.  Each shape yields
    exactly the windows decision_edges.CUTOFF_KEYS names for it."""
    snap = de.snapshot(name)
    wins = de.cutoff_windows(snap.ts, snap.pos)
    assert set(wins) == de.CUTOFF_KEYS[name]
    if "strongest_failing" not in wins:  # no failing window scores above 0
        for t in snap.ts:
            f = t.l2[t.l2 <= de.CUT]
            assert f.size == 0 or f.max() <= 0.0
    u = snap.random_u(2)
    for key, (n, k, l2) in wins.items():
        for d in de.D_CUTOFF:
            for cut in (l2 + d, l2 - d):
                assert cut > 0.0
                assert de.cutoff_clearance(snap.ts, cut) >= d / 2, (key, d)
                ts = de.at_cutoff(snap.ts, cut)
                opos, _, omg = snap.oracle(u, cutoff=cut)
                rpos, rmg = de.restated(ts, u)
                assert np.array_equal(rpos, opos) and np.array_equal(rmg, np.asarray(omg))
                assert (k in ts[n].win) == (cut < l2)
                if key == "global_max":
                    # just above: no motif category anywhere; just below: one target has one
                    assert sum(t.npass for t in ts) == (1 if cut < l2 else 0)


def test_list_path_bisection():
    N, L, W, M = 24, 60, 6, 2
    codes, offsets = de.dataset(N, L, W, b"ACGT", seed=21)
    S = ol.Seqs(codes, offsets, b"ACGT")
    cnt, pos = de.list_snapshot(S, W, M, seed=22)
    lo, hi = de.bisect_list_edges(S, M, W, de.PC, de.CUT, cnt, pos, M, seed=23)
    assert np.isfinite(lo).all()
    assert ((hi > lo) & (hi - lo <= 2.0 ** -53)).all()
    k_lo = de.list_picks(S, M, W, de.PC, de.CUT, cnt, pos, M, lo)[3]
    k_hi = de.list_picks(S, M, W, de.PC, de.CUT, cnt, pos, M, hi)[3]
    assert (k_lo != k_hi).all()
    for d in de.D_ROULETTE:
        for u in de.list_probes(lo, hi, d):
            mg = de.list_picks(S, M, W, de.PC, de.CUT, cnt, pos, M, u)[2]
            # the edge lies in (lo, hi]: the oracle's margin is the probe's distance from
            # it, or less where another edge it walked lies nearer
            dist = np.minimum(np.abs(u - lo), np.abs(u - hi))
            assert (mg <= dist + 2.0 ** -52).all()
            assert (np.abs(mg - dist) <= 2.0 ** -52).mean() >= 0.5
