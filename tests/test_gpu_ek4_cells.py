"""The four-symbol kernel's table build and quad scan through the outputs (gs_sweep.hip,
DESIGN.md §9.20: the workgroup's sum of T kept beside the totals, the quad scan's
one-compare window mask): chains against the oracle and the loop path against the
one-iteration path bit for bit, at every motif width class (W = 4, 12, 16: one column a
lane of a 16-lane group, W = 32: two), at 32 and 64 lanes a sequence, on the
no-window-can-pass branch (all cells 0), through the exact rescan (a zero PCV) and for
targets without a motif, with PWMS on the last sweep only, and on the decision edges of
tests/decision_edges.py.  The all-background takeover is off (bg_mode 0).
"""
import numpy as np
import pytest

import decision_edges as de
from conftest import uniforms
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

ALPHA = b"ACGT"
PC, CUT = 1e-4, 1.0
RTOL = 1e-12
STATS = ("exact_rescans", "serial_picks", "rescan_flagged", "desc_oob")


@pytest.fixture(scope="module")
def ctx_pair():
    """(loop path, one-iteration path) of gs_sweep_kernel's four-symbol instantiation."""
    from gibbssampling_amd import Context
    c0 = Context(0, tuning={"dna_mode": 0.0, "sweep_one": 0.0, "bg_mode": 0.0})
    c1 = Context(0, tuning={"dna_mode": 0.0, "sweep_one": 1.0, "bg_mode": 0.0})
    yield c0, c1
    for c in (c0, c1):
        st = c.stats()
        c.close()
        assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st


def same_as_oracle(gp, gw, op, ow, what):
    assert np.array_equal(gp, op), f"{what}: positions differ at {np.nonzero(gp != op)[0][:8]}"
    eq = gw == ow
    with np.errstate(invalid="ignore"):
        rel = np.abs(gw - ow) / np.maximum(np.abs(ow), 1e-300)
    assert np.all(eq | (rel <= RTOL)), f"{what}: PWMS rel diff {np.nanmax(rel[~eq]):.3e}"


def launch_is(c, one, gl):
    launch = c.last_sweep_launch()
    assert launch["ek"] == 4 and launch["gl"] == gl and launch["one"] == one, launch


def starts(lens, W, kind, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    if kind == "none":
        pos[:] = -1
    elif kind == "mixed":
        pos[rng.random(len(lens)) < 0.4] = -1
        pos[0] = -1
        if len(pos) > 1:
            pos[1] = max(pos[1], 0)
    return pos


def chain(c, codes, offsets, W, pos, seed, cut=CUT, sweeps=3):
    c.set_sequences(codes, offsets, ALPHA)
    s0 = c.stats()
    c.set_positions(W, pos)
    c.run_sweeps(PC, cut, sweeps, seed)
    p, w = c.get_state()
    s1 = c.stats()
    return p, w, c.agg_download(), {k: s1[k] - s0[k] for k in STATS}


def oracle_chain(codes, offsets, W, pos, seed, cut=CUT, sweeps=3):
    S = ol.Seqs(codes, offsets, ALPHA)
    p, w = pos, None
    for t in range(sweeps):
        p, w, _ = ol.sweep(S, W, PC, cut, p, uniforms(seed, ol.stream_sweep(t), len(pos)), threads=8)
    return p, w


def both_paths(ctx_pair, codes, offsets, W, pos, seed, gl, what, cut=CUT):
    """The chain through sweep_one 0 and 1: equal bit for bit, and the oracle's."""
    out = []
    for c, one in zip(ctx_pair, (0, 1)):
        out.append(chain(c, codes, offsets, W, pos, seed, cut))
        launch_is(c, one, gl)
    (p0, w0, a0, s0), (p1, w1, a1, s1) = out
    assert np.array_equal(p0, p1), (what, np.nonzero(p0 != p1)[0][:8])
    assert w0.tobytes() == w1.tobytes(), what
    assert a0.tobytes() == a1.tobytes(), what
    assert s0 == s1, (what, s0, s1)
    op, ow = oracle_chain(codes, offsets, W, pos, seed, cut)
    same_as_oracle(p1, w1, op, ow, what)
    return p1, w1, s1


# W, Lmax, lanes a sequence: the 16-lane group's one and two columns a lane, and W = 12 at
# 32 and 64 lanes
SHAPES = [(4, 70, 16), (12, 90, 16), (16, 90, 16), (32, 120, 16), (12, 300, 32), (12, 600, 64)]


@pytest.mark.parametrize("N", [1, 5, 17])
@pytest.mark.parametrize("kind", ["none", "placed", "mixed"])
@pytest.mark.parametrize("W,L,gl", SHAPES)
def test_chains(ctx_pair, W, L, gl, kind, N):
    codes, offsets = de.dataset(N, L, W, ALPHA, 400 + W + N, lmin=W)
    pos = starts(np.diff(offsets), W, kind, 401 + W + N)
    both_paths(ctx_pair, codes, offsets, W, pos, 402 + W, gl, f"W = {W}, L = {L}, N = {N}, starts {kind}")


@pytest.mark.parametrize("W,L,gl", [(12, 90, 16), (32, 120, 16), (12, 300, 32)])
def test_no_window_can_pass(ctx_pair, W, L, gl):
    """A cut-off of 500 is above the sum of the column maxima of any snapshot here (a
    term is at most log2(1 / PCV) < 30): every cell is 0, every pick a background one."""
    N = 17
    codes, offsets = de.dataset(N, L, W, ALPHA, 410 + W, lmin=W)
    pos = starts(np.diff(offsets), W, "mixed", 411 + W)
    p, _, _ = both_paths(ctx_pair, codes, offsets, W, pos, 412 + W, gl, f"cut-off 500, W = {W}", cut=500.0)
    assert (p == -1).all()


@pytest.mark.parametrize("W,gl,L", [(12, 16, 90), (32, 16, 120), (12, 32, 300)])
def test_zero_pcv_goes_to_the_rescan(ctx_pair, W, gl, L):
    """Pseudo-count 0 and no T anywhere but in one sequence's motif segment: that
    sequence's hold-one-out background counts no T (PCV 0: the exact rescan), and two
    targets have no motif.  One sweep, both paths, against the oracle."""
    N = 9
    rng = np.random.default_rng(420 + W)
    a = np.frombuffer(ALPHA, np.uint8)
    lens = np.full(N, L)
    offsets = np.arange(0, N * L + 1, L, dtype=np.int64)
    codes = a[rng.integers(0, 3, N * L)].astype(np.uint8)
    pos = (rng.random(N) * (lens - W + 1)).astype(np.int32)
    pos[[2, 7]] = -1
    codes[4 * L + pos[4]: 4 * L + pos[4] + W] = a[3]  # every T of the data is in this segment
    S = ol.Seqs(codes, offsets, ALPHA)
    u = rng.random(N)
    out = []
    for c, one in zip(ctx_pair, (0, 1)):
        c.set_sequences(codes, offsets, ALPHA)
        s0 = c.stats()
        out.append(c.motif_sweep(W, 0.0, CUT, pos, u))
        s1 = c.stats()
        launch_is(c, one, gl)
        assert s1["exact_rescans"] - s0["exact_rescans"] >= 1, (s0, s1)
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    op, ow, _ = ol.sweep(S, W, 0.0, CUT, pos, u)
    same_as_oracle(out[1][0], out[1][1], op, ow, f"zero PCV, W = {W}")


def test_pwms_of_the_last_sweep_only(ctx_pair):
    """A 3-sweep chain (PWMS on its last sweep only) against three 1-sweep calls (PWMS on
    each): bit for bit, and the oracle's."""
    c = ctx_pair[1]
    N, L, W = 17, 120, 12
    codes, offsets = de.dataset(N, L, W, ALPHA, 431)
    pos = starts(np.diff(offsets), W, "mixed", 432)
    p3, w3, a3, _ = chain(c, codes, offsets, W, pos, 433)
    c.set_positions(W, pos)
    for t in range(3):
        c.run_sweeps(PC, CUT, 1, 433, first_sweep=t)
        p1, w1 = c.get_state()
    assert np.array_equal(p3, p1) and w3.tobytes() == w1.tobytes()
    assert a3.tobytes() == c.agg_download().tobytes()
    op, ow = oracle_chain(codes, offsets, W, pos, 433)
    same_as_oracle(p3, w3, op, ow, "chain with PWMS on its last sweep")


_snap = []


def edge_snap():
    """18 ragged sequences (K = 3 .. 109: short and empty last lane blocks), W = 12,
    doMotifSampling's starts, two targets without a motif."""
    if not _snap:
        N, L, W = 18, 120, 12
        codes, offsets = de.dataset(N, L, W, ALPHA, 441, lmin=14)
        seqs = ol.Seqs(codes, offsets, ALPHA)
        pos = ol.random_starts(seqs, W, PC, seed=441, mode=1)[1].astype(np.int32)
        pos[[3, N - 2]] = -1
        _snap.append((codes, offsets, seqs, pos, de.targets(seqs, W, PC, CUT, pos)))
    return _snap[0]


@pytest.mark.parametrize("one", [0, 1])
def test_roulette_edges(ctx_pair, one):
    """u = acc_c +- d, d = 1e-11 .. 1e-3 (tests/decision_edges.py): a probe the reference
    itself decides by the last place of a log keeps a random u, at most a quarter may."""
    c = ctx_pair[one]
    W = 12
    codes, offsets, seqs, pos, ts = edge_snap()
    geo = de.geometry_groups(16, quad=True)
    has = [n for n, t in enumerate(ts) if t.ncat >= 2]
    assert len(has) >= len(ts) // 2
    sub = [ts[n] for n in has]
    cs, _ = de.choose_edges(sub, geo, seed=5)
    c.set_sequences(codes, offsets, ALPHA)
    probed = 0
    for d in de.D_ROULETTE:
        for sign, us in zip("+-", de.probes_at_distance(sub, cs, d)):
            u = np.random.default_rng(7).random(len(ts))
            amb = set(de.ambiguous(sub, us))
            for i, n in enumerate(has):
                if i not in amb:
                    u[n] = us[i]
                    probed += 1
            o = ol.sweep(seqs, W, PC, CUT, pos, u)
            g = c.motif_sweep(W, PC, CUT, pos, u)
            launch_is(c, one, 16)
            same_as_oracle(g[0], g[1], o[0], o[1], f"one={one} u = acc_c {sign} {d:g}")
    assert 4 * probed >= 3 * len(has) * 2 * len(de.D_ROULETTE), probed
