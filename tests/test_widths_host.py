"""What the wide-motif fixtures promise, on the CPU (tests/widths.py, the helper of
tests/test_gpu_widths.py): the W lists reach every width class of the kernels at W = WM
and below it, the snapshots hold both kinds of pick with margins far from any CDF edge,
the W = 64 fixtures leave the binary32 and the normal binary64 range, and the list
fixture yields pairs -- so that a GPU pass cannot be an empty one.
"""
import numpy as np
import pytest

import test_gpu_widths as gw
import widths as wd
from oracle import oracle_lib as ol


def classes_of(ws):
    full = {wd.sweep_wm(W) for W in ws if wd.sweep_wm(W) == W}
    padded = {wd.sweep_wm(W) for W in ws if wd.sweep_wm(W) != W}
    return full, padded


def test_width_class_restated():
    assert sorted({wd.sweep_wm(W) for W in wd.ALL_W}) == list(wd.CLASSES)
    for W in wd.ALL_W:
        WM = wd.sweep_wm(W)
        assert WM >= W and WM - W < (4 if WM <= 32 else 8) and WM % (4 if WM <= 32 else 8) == 0
    full, padded = classes_of(wd.ALL_W)
    assert full == padded == set(wd.CLASSES)
    # greedy_carve's ring slot, align16(Lmax) + align16(WM) + 32 bytes: W in WM's place gives
    # the same bytes at every width (no test can tell the two apart)
    assert all(wd._a16(W) == wd._a16(wd.sweep_wm(W)) for W in wd.ALL_W)


def test_w_lists_cover_the_classes():
    # the lanes cases (general layout): every class from 24 up, full and padded
    full, padded = classes_of(gw.LANES_ATGC5)
    assert full >= {24, 28, 32, 48, 64} and padded >= {24, 48, 64}
    # the four-symbol kernel's widths on the unsplit side (4 WM > 64) below 32
    assert set(gw.LANES_EK4) == {20, 24, 28}
    assert all(wd.expect_ek(b"ACGT", W) == 4 and 4 * W > 64 for W in gw.LANES_EK4)
    # greedy and site: every class from 24 up, at W = WM and at a W < WM
    ws = [W for v in gw.GREEDY_W.values() for W in v]
    full, padded = classes_of(ws)
    wide = {c for c in wd.CLASSES if c >= 24}
    assert full >= wide and padded >= wide
    assert all(64 in v for v in gw.GREEDY_W.values())
    assert {wd.sweep_wm(W) for W in gw.COOP_W} == {wd.sweep_wm(W) for W in ws}
    assert all(wd.sweep_wm(W) >= 16 for W in gw.COOP_W)
    assert gw.TOP_W[0] == wd.W_MAX and wd.sweep_wm(gw.TOP_W[1]) != gw.TOP_W[1]


@pytest.mark.parametrize("name", sorted(wd.ALPHAS))
def test_both_kinds_of_pick(name):
    """Summed over W = 1..64 and both starts: (motif, background) picks from the
    initialiser's positions DNA (1413, 123), ATGC- (1410, 126), protein (1464, 72)."""
    motif = bg = 0
    for W in wd.ALL_W:
        s = wd.snap(name, W)
        assert s.Lmax <= W + 70 and int(np.diff(s.offsets).min()) >= W
        for kind, pos, (opos, opw, omg) in s.starts():
            assert np.min(omg) >= 1e-9, (name, W, kind, float(np.min(omg)))
        motif += int((s.o_init[0] >= 0).sum())
        bg += int((s.o_init[0] < 0).sum())
        assert (s.unif < 0).sum() >= 1 and (s.unif >= 0).sum() >= 1
    assert motif >= 1000 and bg >= 50, (motif, bg)
    assert motif + bg == 24 * len(wd.ALL_W)
    # the uniform starts give mostly background picks
    ub = sum(int((wd.snap(name, W).o_unif[0] < 0).sum()) for W in wd.ALL_W)
    assert ub >= 24 * len(wd.ALL_W) // 2, ub


@pytest.mark.parametrize("name", ["dna", "protein"])
def test_background_products_leave_binary32(name):
    s = wd.snap(name, 64)
    g, _ = wd.detail_ranges(s.seqs, 64, s.init)
    assert 0.0 < g < 2.0 ** -126, g


def test_window_scores_become_subnormal():
    codes, offsets, seqs, pos, u = wd.all_none()
    _, smin = wd.detail_ranges(seqs, 64, pos)
    assert 0.0 < smin < 2.0 ** -1022, smin
    opos, opw, omg = ol.sweep(seqs, 64, wd.PC, wd.CUT, pos, u)
    assert (opos == -1).all() and np.min(omg) >= 1e-9


@pytest.mark.parametrize("name,W", [(n, W) for n in ("dna", "protein") for W in (64, 57)])
def test_list_fixture_has_pairs(name, W):
    codes, offsets, seqs, cnt, pos, u = wd.list_fixture(name, W)
    oc, op, ow = ol.sweep_lists(seqs, 2, W, wd.PC, wd.CUT, cnt, pos, 2, u)
    assert int((oc == 2).sum()) >= 4, oc
    gc, gp, gpw, _ = ol.greedy_lists(seqs, 2, W, wd.PC, wd.CUT, oc, op, 2, ow)
    assert int((gc == 2).sum()) >= 4, gc


def test_carve_restated():
    """The restated carve at the 160 KiB of an MI355X workgroup: the ladder shapes of the GPU
    module take the wavefront counts they are there for (the GPU test asserts what the
    device launched), and the refusal shape fits at no count, there or at 64 KiB."""
    got = {(h, w): (alpha, extra, W) for h, w, alpha, extra, W in gw.ladder_shapes(163840)}
    assert got == {(2, 4): (b"ATGC-", b"", 48), (2, 2): (b"ATGC-", b"", 64), (2, 1): (b"ATGC-", b"BDE", 64),
                   (1, 12): (wd.PROTEIN, b"", 21), (1, 6): (wd.PROTEIN, b"", 41), (1, 3): (wd.PROTEIN, b"", 64)}
    for limit in (163840, 65536):
        assert wd.auto_waves(5, 16, 64, 300, limit) is None
        assert wd.auto_waves(5, 16, 64, 134, limit) is None
    # launch_sweep's tuning: from 2 or 1 wavefronts the carve fits at W = 8 and W = 40
    for W in (8, 40):
        assert [wd.auto_waves(5, 5, W, W + 70, 163840, start=s) for s in (1, 2)] == [1, 2]
    assert wd.greedy_waves(20, 20, 64, 134, 163840) == 4
    assert wd.greedy_waves(20, 20, 41, 111, 163840) == 8
