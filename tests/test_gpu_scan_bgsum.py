"""The pair-table scan's binary32 background sums and the four-symbol kernel's pair table
built from its 4 W cells (gs_sweep.hip kQuad / ek4_layout g_cell).

The quad scan sums a sequence's background weights as v_exp_f32(lg - r) in binary32,
relative to the sequence's integer reference r = rint(W max_e log2 PCV[e]), and scales
the lane sums back by 2^r.  What can go wrong, and what looks for it here:

- a window whose lg - r leaves (-96, 96) must send its sequence to the exact rescan,
  never be flushed (test_range_flag: a composition so skewed that windows of the rare
  symbol cross the limit in some targets, asserted from the oracle's PCV on the CPU);
- the error term of the binary32 accumulation and of lg - r must cover what they are
  derived for: the decision-edge probes of tests/decision_edges.py at the largest lane
  block the 16-lane groups take (R = 16), at ragged lengths and at L = W;
- the loop path's copy of the changed scan and table build: sweep_one 0 against 1, bit
  for bit;
- the pair table (bit-identical entries: the same integers, the same binary32 pair sum)
  and the readers of the hold-one-out's PCV, through the outputs: chains at W = 4, 12, 32
  from every kind of start against the oracle, the PWMS factors (a one-sweep call; a
  chain's last sweep), the exact rescan of targets with a motif (every target of
  test_every_target_rescanned) and of targets without one.
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
RANGE = 96.0  # gs_common.h kBg32Range (tests/test_scan_bgsum_host.py reads it from the library)
STATS = ("exact_rescans", "serial_picks", "rescan_flagged", "desc_oob")


@pytest.fixture(scope="module")
def ctx_pair():
    """(loop path, one-iteration path) of the four-symbol kernel, the all-background
    takeover off: every sweep is gs_sweep_kernel's."""
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


def delta(c, s0):
    s1 = c.stats()
    return {k: s1[k] - s0[k] for k in STATS}


def ek4(c, one):
    launch = c.last_sweep_launch()
    assert launch["ek"] == 4 and launch["gl"] == 16 and launch["one"] == one, launch


def oracle_chain(S, W, pos, seed, sweeps=3):
    p, w = pos, None
    for t in range(sweeps):
        p, w, _ = ol.sweep(S, W, PC, CUT, p, uniforms(seed, ol.stream_sweep(t), len(pos)), threads=8)
    return p, w


def chain(c, codes, offsets, W, pos, seed, sweeps=3):
    c.set_sequences(codes, offsets, ALPHA)
    s0 = c.stats()
    c.set_positions(W, pos)
    c.run_sweeps(PC, CUT, sweeps, seed)
    p, w = c.get_state()
    return p, w, c.agg_download(), delta(c, s0)


# ---- range flag -----------------------------------------------------------------------
def skewed(N, L, W, probs, runs, seed):
    """N sequences of L symbols drawn with `probs` over ACGT; the sequences in `runs` hold
    one run of W 'T' (windows made of the rarest symbol)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(ALPHA, np.uint8)
    codes = a[rng.choice(4, N * L, p=probs)].astype(np.uint8)
    for n in runs:
        s = n * L + int(rng.integers(0, L - W + 1))
        codes[s:s + W] = a[3]
    return codes, np.arange(0, N * L + 1, L, dtype=np.int64)


def window_offsets(S, W, pos):
    """Per target: min and max over its windows of lg - r, from the oracle's PCV and
    background products: r = rint(W max_e log2 PCV[e]) as the kernel takes it (binary32)."""
    lo, hi = [], []
    for n in range(S.n):
        d = ol.target_detail(S, W, PC, pos, n)
        lq = np.log2(d["pcv"][[b - 42 for b in ALPHA]]).astype(np.float32)
        r = float(np.rint(np.float32(W) * lq.max()))
        off = np.log2(d["G"]) - r
        lo.append(off.min())
        hi.append(off.max())
    return np.array(lo), np.array(hi)


@pytest.mark.parametrize("one", [0, 1])
def test_range_flag(ctx_pair, one):
    """N = 17, L = 256, W = 16, almost all A, T only in two runs of W: a window of T
    lies more than 96 below the reference in the two sequences that hold a run and in
    no other.  The crossing targets are rescanned; the chain is the oracle's."""
    c = ctx_pair[one]
    N, L, W = 17, 256, 16
    runs = [2, 11]
    codes, offsets = skewed(N, L, W, [0.985, 0.0075, 0.0075, 0.0], runs, 41)
    S = ol.Seqs(codes, offsets, ALPHA)
    pos = ol.random_starts(S, W, PC, seed=42, mode=1)[1].astype(np.int32)
    lo, hi = window_offsets(S, W, pos)
    cross = lo < -(RANGE + 1.0)
    inside = (lo > -(RANGE - 1.0)) & (hi < 2.0)
    assert np.array_equal(np.nonzero(cross)[0], runs), (lo, hi)
    assert inside.sum() == N - len(runs), (lo, hi)
    c.set_sequences(codes, offsets, ALPHA)
    u = np.random.default_rng(43).random(N)
    s0 = c.stats()
    gp, gw = c.motif_sweep(W, PC, CUT, pos, u)
    dl = delta(c, s0)
    ek4(c, one)
    op, ow, _ = ol.sweep(S, W, PC, CUT, pos, u)
    same_as_oracle(gp, gw, op, ow, "one sweep over the range limit")
    assert dl["exact_rescans"] >= len(runs) and dl["rescan_flagged"] >= len(runs), dl
    p, w, _, dl = chain(c, codes, offsets, W, pos, 44)
    op, ow = oracle_chain(S, W, pos, 44)
    same_as_oracle(p, w, op, ow, "3-sweep chain over the range limit")
    assert dl["exact_rescans"] > 0, dl


@pytest.mark.parametrize("one", [0, 1])
def test_mild_skew_flags_nothing(ctx_pair, one):
    """W = 12, A 70 % and 10 % each of the others: every window of every target within
    the range (asserted), no sequence flagged, the chain is the oracle's."""
    c = ctx_pair[one]
    N, L, W = 17, 256, 12
    codes, offsets = skewed(N, L, W, [0.7, 0.1, 0.1, 0.1], [2, 11], 51)
    S = ol.Seqs(codes, offsets, ALPHA)
    pos = ol.random_starts(S, W, PC, seed=52, mode=1)[1].astype(np.int32)
    lo, hi = window_offsets(S, W, pos)
    assert (lo > -(RANGE - 1.0)).all() and (hi < 2.0).all() and lo.min() < -20.0, (lo, hi)
    p, w, _, dl = chain(c, codes, offsets, W, pos, 54)
    ek4(c, one)
    op, ow = oracle_chain(S, W, pos, 54)
    same_as_oracle(p, w, op, ow, "3-sweep chain, mild skew")
    assert dl["rescan_flagged"] == 0, dl


# ---- accumulation bound: the decision-edge probes at the scan's extreme shapes -----------
class Snap:
    """decision_edges.Snapshot for lengths of this file's choosing."""

    def __init__(self, N, L, W, lmin, seed):
        self.N, self.W = N, W
        self.codes, self.offsets = de.dataset(N, L, W, ALPHA, seed, lmin=lmin)
        self.seqs = ol.Seqs(self.codes, self.offsets, ALPHA)
        self.pos = ol.random_starts(self.seqs, W, PC, seed=seed, mode=1)[1].astype(np.int32)
        self.pos[[3, N - 2]] = -1  # two targets without a motif of their own
        self.ts = de.targets(self.seqs, W, PC, CUT, self.pos)


EDGE_SHAPES = {
    "R16": (12, 256, 12, 250, 61),    # K = 239 .. 245: blocks of 16 windows, the largest
    "ragged": (18, 256, 12, 14, 62),  # K = 3 .. 245: short and empty last blocks
    "LeqW": (12, 12, 12, 12, 63),     # one window a target
}
_snaps = {}


def edge_snap(name):
    if name not in _snaps:
        _snaps[name] = Snap(*EDGE_SHAPES[name])
    return _snaps[name]


@pytest.mark.parametrize("one", [0, 1])
@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_roulette_edges_at_the_scan_extremes(ctx_pair, shape, one):
    """u = acc_c +- d, d = 1e-11 .. 1e-3, on the four-symbol rows of
    tests/test_gpu_decision_edges.py at R = 16, at ragged lengths and at L = W.  Targets
    with a single category (L = W, the window failing) have no edge and keep a random u;
    a probe the reference itself decides by the last place of a log (decision_edges
    `unambiguous`) is replaced by a random u, and at most a quarter of them may be."""
    c = ctx_pair[one]
    snap = edge_snap(shape)
    geo = de.geometry_groups(16, quad=True)
    has = [n for n, t in enumerate(snap.ts) if t.ncat >= 2]
    assert len(has) >= snap.N // 2, shape
    sub = [snap.ts[n] for n in has]
    cs, _ = de.choose_edges(sub, geo, seed=5)
    if shape == "R16":
        assert {geo.block(t.K) for t in snap.ts} == {16}
    c.set_sequences(snap.codes, snap.offsets, ALPHA)
    probed = 0
    for d in de.D_ROULETTE:
        for sign, us in zip("+-", de.probes_at_distance(sub, cs, d)):
            u = np.random.default_rng(7).random(snap.N)
            amb = set(de.ambiguous(sub, us))
            for i, n in enumerate(has):
                if i not in amb:
                    u[n] = us[i]
                    probed += 1
            o = ol.sweep(snap.seqs, snap.W, PC, CUT, snap.pos, u)
            g = c.motif_sweep(snap.W, PC, CUT, snap.pos, u)
            ek4(c, one)
            same_as_oracle(g[0], g[1], o[0], o[1], f"{shape} one={one} u = acc_c {sign} {d:g}")
    assert 4 * probed >= 3 * len(has) * 2 * len(de.D_ROULETTE), (shape, probed)


# ---- the loop path's copy of the scan --------------------------------------------------
@pytest.mark.parametrize("N,ragged", [(1, False), (1, True), (5, False), (5, True), (17, False), (17, True)])
def test_paths_agree(ctx_pair, N, ragged):
    """A 3-sweep chain through sweep_one 0 and 1 on a skewed composition (so that the
    reference r is far from the windows' logs): positions, PWMS bits, aggregates and
    fallback counts equal."""
    L, W = 200, 12
    rng = np.random.default_rng(70 + N + ragged)
    a = np.frombuffer(ALPHA, np.uint8)
    lens = rng.integers(W, L + 1, N) if ragged else np.full(N, L)
    lens[0] = L
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = a[rng.choice(4, int(offsets[-1]), p=[0.55, 0.25, 0.15, 0.05])].astype(np.uint8)
    pos = (rng.random(N) * (lens - W + 1)).astype(np.int32)
    if N > 1:
        pos[1] = -1
    out = [chain(c, codes, offsets, W, pos, 75) for c in ctx_pair]
    for c, one in zip(ctx_pair, (0, 1)):
        ek4(c, one)
    (p0, w0, a0, s0), (p1, w1, a1, s1) = out
    assert np.array_equal(p0, p1), np.nonzero(p0 != p1)[0][:8]
    assert w0.tobytes() == w1.tobytes()
    assert a0.tobytes() == a1.tobytes()
    assert s0 == s1 and s1["desc_oob"] == 0, (s0, s1)


# ---- the pair table and the PCV's division, through the outputs -------------------------
def starts(lens, W, kind, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    if kind == "none":
        pos[:] = -1
    elif kind == "mixed":
        pos[rng.random(len(lens)) < 0.4] = -1
        pos[0] = -1
        pos[1] = max(pos[1], 0)
    return pos


@pytest.mark.parametrize("W", [4, 12, 32])
@pytest.mark.parametrize("kind", ["none", "placed", "mixed"])
def test_chains_against_the_oracle(ctx_pair, W, kind):
    c = ctx_pair[1]
    N, L = 17, 90
    codes, offsets = de.dataset(N, L, W, ALPHA, 80 + W, lmin=W)
    pos = starts(np.diff(offsets), W, kind, 81 + W)
    p, w, _, dl = chain(c, codes, offsets, W, pos, 82 + W)
    ek4(c, 1)
    op, ow = oracle_chain(ol.Seqs(codes, offsets, ALPHA), W, pos, 82 + W)
    same_as_oracle(p, w, op, ow, f"W = {W}, starts {kind}")
    assert dl["desc_oob"] == 0


@pytest.mark.parametrize("one", [0, 1])
def test_every_target_rescanned(ctx_pair, one):
    """Every sequence is A but for one run of W = 32 symbols cycling C, G, T (each about
    4 % of the data, and only in the runs), so a window of the run lies more than 200
    below the reference in every target (asserted): each takes the exact rescan, whose
    table divides by the hold-one-out's PCV -- targets with a motif and, two of them,
    without."""
    c = ctx_pair[one]
    N, L, W = 9, 256, 32
    a = np.frombuffer(ALPHA, np.uint8)
    codes = np.full(N * L, a[0], np.uint8)
    offsets = np.arange(0, N * L + 1, L, dtype=np.int64)
    for n in range(N):
        codes[n * L + 11 * n: n * L + 11 * n + W] = a[1 + (np.arange(W) + n) % 3]
    S = ol.Seqs(codes, offsets, ALPHA)
    pos = ol.random_starts(S, W, PC, seed=92, mode=1)[1].astype(np.int32)
    pos[[1, 6]] = -1
    lo, _ = window_offsets(S, W, pos)
    if not (lo < -(RANGE + 1.0)).all():
        pytest.fail(f"construction does not cross the limit everywhere: {lo}")
    c.set_sequences(codes, offsets, ALPHA)
    u = np.random.default_rng(93).random(N)
    s0 = c.stats()
    gp, gw = c.motif_sweep(W, PC, CUT, pos, u)
    dl = delta(c, s0)
    ek4(c, one)
    op, ow, _ = ol.sweep(S, W, PC, CUT, pos, u)
    same_as_oracle(gp, gw, op, ow, "every target through the exact rescan")
    assert dl["exact_rescans"] == N, dl


def test_pwms_of_the_last_sweep_only(ctx_pair):
    """A 3-sweep chain (PWMS on its last sweep only) against three 1-sweep calls (PWMS,
    and so the picked window's factors PPM' / PCV, on each): bit for bit, and the oracle's."""
    c = ctx_pair[1]
    N, L, W = 17, 120, 12
    codes, offsets = de.dataset(N, L, W, ALPHA, 95)
    pos = starts(np.diff(offsets), W, "mixed", 96)
    p3, w3, a3, _ = chain(c, codes, offsets, W, pos, 97)
    c.set_positions(W, pos)
    for t in range(3):
        c.run_sweeps(PC, CUT, 1, 97, first_sweep=t)
        p1, w1 = c.get_state()
    assert np.array_equal(p3, p1) and w3.tobytes() == w1.tobytes()
    assert a3.tobytes() == c.agg_download().tobytes()
    op, ow = oracle_chain(ol.Seqs(codes, offsets, ALPHA), W, pos, 97)
    same_as_oracle(p3, w3, op, ow, "chain with PWMS on its last sweep")
