"""Wide-motif fixtures: every width class of gs_sweep_kernel and gs_greedy_kernel, W up to
the documented maximum of 64 (CPU only).

Not a conftest and not collected: the helper of tests/test_gpu_widths.py and
tests/test_widths_host.py.  It restates the library's width class (gs_sweep_wm), its
lanes per sequence (gs_sweep_group_lanes) and the general sweep's LDS carve
(gs_engine.cpp sweep_carve, launch_sweep's halving of the wavefronts) so that a test can
say which kernel instantiation and which workgroup shape a case must run, and builds the
snapshots from conftest.make_dataset and the oracle.  Everything the GPU tests rely on
(both kinds of pick present, margins, the ranges the wide fixtures reach, pairs in the
list fixture) is asserted on the CPU by tests/test_widths_host.py.
"""
from __future__ import annotations

import numpy as np

from conftest import make_dataset
from oracle import oracle_lib as ol

PC, CUT = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
ALPHAS = {"dna": b"ACGT", "atgc5": b"ATGC-", "protein": PROTEIN}
W_MAX = 64
CLASSES = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64)
ALL_W = tuple(range(1, W_MAX + 1))


# ---- the library's launch arithmetic, restated ---------------------------------------
def sweep_wm(W):
    """gs_sweep_wm: W rounded up to 4 up to 32, to 8 above."""
    r = (W + 3) // 4 * 4
    return r if r <= 32 else (W + 7) // 8 * 8


def scan_group(E):
    """H of gs_sweep_kernel: 2 (pair tables) up to 16 encoded symbols, else 1."""
    return 2 if E <= 16 else 1


def group_lanes(E, Lmax):
    """gs_sweep_group_lanes."""
    gl = 16
    while gl < 64 and (E + 1 > gl or Lmax > 16 * gl):
        gl *= 2
    return max(gl, 32) if scan_group(E) == 1 else gl


def expect_ek(alpha, W, exact=False, pcv=False):
    """launch_sweep's choice of the four-symbol kernel (dna_mode 0, four symbols and no
    other in the data, the default 4 wavefronts)."""
    return 4 if (bytes(alpha) == b"ACGT" and not exact and not pcv and W % 4 == 0 and W <= 32) else 0


def _a16(x):
    return (x + 15) & ~15


def sweep_lds(A, E, W, Lmax, gl, waves):
    """Bytes of dynamic LDS of the general layout (sweep_carve with ek4 = false)."""
    WM, H, ng = sweep_wm(W), scan_group(E), 64 // gl
    o = 0

    def take(b):
        nonlocal o
        o = _a16(o + b)

    take(4 * A * W)
    take(8 * (A + 1))
    take(8 * A * W)
    take(8 * A * W)
    take((16 if H == 2 else 8) * A * W)
    take(4 * 16)
    take(8 * (4 * (W + 1) + 1))
    base, o = o, 0
    take(4 * A * W)
    take(8 * A)
    take(32)
    tab = 16 * (WM + 1) * E
    if H == 2:
        take(16 * 64)
        lt = _a16(8 * (WM + 1) * E)
        take(ng * lt)
        if ng * lt < tab:
            take(tab)
    else:
        gs = _a16(4 * (WM + 1) * E) + _a16(4 * (Lmax + 1))
        if ng > 1:
            gs = (gs + 127) // 256 * 256 + 128
        take(max(ng * gs, tab))
    wave_fixed, o = o, 0
    if H == 2:
        take(8 * (WM // 2 + 1) * E * E)
    take(Lmax + WM + 96)
    take(8 * gl)
    take(8 * gl)
    take(16 * WM)
    return base + waves * (wave_fixed + ng * o)


def auto_waves(A, E, W, Lmax, limit, start=None):
    """The wavefronts a workgroup launch_sweep settles on under `limit` bytes of LDS (from
    `start`, the sweep_waves tuning, or the alphabet's 4 / 12), None when it refuses."""
    gl = group_lanes(E, Lmax)
    waves = start or (4 if scan_group(E) == 2 else 12)
    while waves > 1 and sweep_lds(A, E, W, Lmax, gl, waves) > limit:
        waves //= 2
    return waves if sweep_lds(A, E, W, Lmax, gl, waves) <= limit else None


def greedy_waves(A, E, W, Lmax, limit, want=8, n=1 << 30):
    """greedy_carve's wavefronts for the motif passes (site = 0): decremented until the
    workgroup fits, at most n, then truncated to a power of two."""
    WM = sweep_wm(W)
    fixed = _a16(4 * A * W) + _a16(8 * A) + 2 * _a16(8 * A * W) + 256
    ring = _a16(Lmax) + _a16(WM) + 32
    wb = _a16(16 * E * (WM + 1)) + 8 * 64
    per = wb + 2 * (ring + 12 + 8 + 256) + 64 + 32
    waves = want
    while waves > 1 and fixed + per * waves > limit:
        waves -= 1
    waves = max(1, min(waves, n))
    while waves & (waves - 1):
        waves &= waves - 1
    return waves


# ---- part 1: one snapshot per alphabet and width -------------------------------------
_cache = {}


class Snap:
    """N = 24 ragged sequences, L <= W + 70, with the initialiser's positions, uniform
    positions (a third of them -1) and the oracle's sweep of both."""

    def __init__(self, name, W):
        self.name, self.W, self.alpha = name, W, ALPHAS[name]
        self.N = 24
        self.codes, self.offsets = make_dataset(self.N, W + 70, W, self.alpha, seed=1000 + W,
                                                ragged=True, mut=0.1)
        self.seqs = ol.Seqs(self.codes, self.offsets, self.alpha)
        self.Lmax = int(np.diff(self.offsets).max())
        self.u = np.random.default_rng(W).random(self.N)
        self.init = ol.random_starts(self.seqs, W, PC, seed=5, mode=1)[1].astype(np.int32)
        rng = np.random.default_rng(3000 + W)
        lens = np.diff(self.offsets)
        self.unif = (rng.random(self.N) * (lens - W + 1)).astype(np.int32)
        self.unif[rng.random(self.N) < 1.0 / 3.0] = -1
        self.unif[0] = -1
        self.o_init = ol.sweep(self.seqs, W, PC, CUT, self.init, self.u)
        self.o_unif = ol.sweep(self.seqs, W, PC, CUT, self.unif, self.u)

    def starts(self):
        return (("init", self.init, self.o_init), ("uniform", self.unif, self.o_unif))


def snap(name, W) -> Snap:
    if (name, W) not in _cache:
        _cache[name, W] = Snap(name, W)
    return _cache[name, W]


def all_none(name="atgc5", N=32, W=64):
    """Every position -1: the PWM holds pseudo-counts only, and at W = 64 the window scores
    are binary64 subnormals.  (codes, offsets, seqs, pos, u)."""
    key = ("none", name, N, W)
    if key not in _cache:
        codes, offsets = make_dataset(N, W + 70, W, ALPHAS[name], seed=1100 + W, ragged=True, mut=0.1)
        _cache[key] = (codes, offsets, ol.Seqs(codes, offsets, ALPHAS[name]),
                       np.full(N, -1, np.int32), np.random.default_rng(1100 + W).random(N))
    return _cache[key]


def detail_ranges(seqs, W, pos):
    """(smallest positive background product, smallest positive window score) over every
    target of the snapshot (go_target_detail)."""
    g, s = np.inf, np.inf
    for n in range(seqs.n):
        d = ol.target_detail(seqs, W, PC, pos, n)
        g = min(g, float(d["G"][d["G"] > 0].min(initial=np.inf)))
        s = min(s, float(d["S"][d["S"] > 0].min(initial=np.inf)))
    return g, s


# ---- shapes whose longest sequence is the last ---------------------------------------
def lanes_dataset(N, Lmax, W, alpha, seed, extra=b"", extra_rate=0.0):
    """N ragged sequences (lengths in [W + 1, 2 Lmax / 3]) and a last one of length Lmax (the
    lanes per sequence follow the longest, wherever it is), a mutated copy of one consensus
    planted in each; every symbol of `extra` (foreign to the alphabet) occurs, sprinkled at
    extra_rate outside the planted copies.  Returns (codes, offsets, planted starts)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alpha), np.uint8)
    lens = rng.integers(W + 1, max(W + 2, Lmax * 2 // 3 + 1), N)
    lens[-1] = Lmax
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8)
    if extra:
        e = np.frombuffer(extra, np.uint8)
        hit = rng.random(codes.size) < extra_rate
        codes[hit] = e[rng.integers(0, len(e), int(hit.sum()))]
        codes[offsets[-1] - len(e):] = e  # (the last sequence's tail: every one occurs)
    cons = a[rng.integers(0, len(a), W)]
    planted = np.zeros(N, np.int32)
    for n in range(N):
        m = cons.copy()
        flip = rng.random(W) < 0.1
        m[flip] = a[rng.integers(0, len(a), int(flip.sum()))]
        room = lens[n] - W + 1 - (len(extra) if n == N - 1 else 0)
        planted[n] = int(rng.random() * room)
        s = int(offsets[n]) + planted[n]
        codes[s:s + W] = m
    return codes, offsets, planted


def mixed_starts(planted, seed):
    """The planted positions with a quarter of them -1 (the first one among them)."""
    pos = np.array(planted, np.int32, copy=True)
    pos[np.random.default_rng(seed).random(len(pos)) < 0.25] = -1
    pos[0] = -1
    return pos


# ---- the list fixture: two occurrences a sequence ------------------------------------
def list_fixture(name, W, N=16):
    """Equal lengths L = 3 W + 20; a copy of each sequence's initialiser segment planted
    W + 5 after it (before it where that does not fit).  Returns (codes, offsets, seqs,
    cnt, pos[N, 2], u) with the initialiser's one-position lists."""
    key = ("list", name, W, N)
    if key not in _cache:
        alpha, L = ALPHAS[name], 3 * W + 20
        codes, offsets = make_dataset(N, L, W, alpha, seed=1200 + W, mut=0.1)
        codes = codes.copy()
        p0 = ol.random_starts(ol.Seqs(codes, offsets, alpha), W, PC, seed=5, mode=1)[1]
        for n in range(N):
            s = int(offsets[n])
            q = p0[n] + W + 5 if p0[n] + 2 * W + 5 <= L else p0[n] - W - 5
            assert 0 <= q <= L - W
            codes[s + q:s + q + W] = codes[s + p0[n]:s + p0[n] + W]
        seqs = ol.Seqs(codes, offsets, alpha)
        init = ol.random_starts(seqs, W, PC, seed=5, mode=1)[1].astype(np.int32)
        pos = np.full((N, 2), -1, np.int32)
        pos[:, 0] = init
        _cache[key] = (codes, offsets, seqs, np.ones(N, np.int32), pos,
                       np.random.default_rng(1200 + W).random(N))
    return _cache[key]
