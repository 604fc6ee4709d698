"""Decision-boundary probes for the sweep's roulette pick and cut-off (CPU only).

Not a conftest and not collected: the helper of tests/test_gpu_decision_edges.py and
tests/test_decision_edges_host.py.

For a snapshot (S, W, pc, cutoff, pos) and a target n this restates what the oracle's
score_target / roulette() do after go_target_detail (oracle/gibbs_oracle.c): the
category list is the K background products G[k] followed by log(S[k]) / ln2 of every
window with log2 S > cutoff, in window order; `sum` the left-to-right sum of the
weights; `acc` the running left-to-right sum of w / sum; the pick the first i with
acc_i <= u <= acc_i + w_i / sum.  Every quantity is the oracle's own binary64 value
(np.cumsum adds sequentially; math.log is the C library's log, as in go_log2), so a u
placed on, next to or at a distance d from acc_c probes the reference's edge itself.

A sweep is synchronous -- a target's pick depends on the input snapshot and its own
u[n] only -- so one sweep probes one edge per target.

Which probes are legitimate.  The device's log may differ from the C library's in the
last place (the project holds it to 1e-12 relative), and every edge depends on `sum`,
which holds the motif categories' logs.  So u sits exactly on an edge (or one ulp from
it) only in log-free snapshots, where no window of any target passes the cut-off and
every weight is a product; with motif categories u = acc_c +- d, d >= 1e-11, and
`unambiguous` requires the pick to stay when every motif weight moves by 1e-12
relative (all up, all down, alternating both ways): a condition on the inputs, asserted
for every probe by the tests, never a tolerance on the GPU's positions.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle_lib as ol

LN2 = float.fromhex("0x1.62e42fefa39efp-1")  # go_log2's divisor
TOP = 1.0 - 2.0 ** -53                       # the largest u a [0, 1) generator gives
D_ROULETTE = (1e-11, 1e-9, 1e-7, 1e-5, 1e-3)
D_CUTOFF = (1e-9, 1e-7, 1e-5, 1e-3)
LOG_REL = 1e-12                              # the device log's bound (relative)
N_KINDS = 6


def dataset(N, L, W, alpha=b"ACGT", seed=0, mut=0.1, lmin=None):
    """N sequences over `alpha` with a mutated consensus W-mer planted in each; ragged
    lengths in [lmin, L] (default max(W + 1, L // 3): at least two windows, and long
    enough that every symbol occurs), the first one L (so Lmax = L decides the lane
    groups)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alpha), np.uint8)
    lo = max(W + 1, L // 3) if lmin is None else lmin
    lens = rng.integers(lo, L + 1, N)
    lens[0] = L
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8)
    cons = a[rng.integers(0, len(a), W)]
    for n in range(N):
        m = cons.copy()
        flip = rng.random(W) < mut
        m[flip] = a[rng.integers(0, len(a), int(flip.sum()))]
        s = int(offsets[n]) + int(rng.random() * (lens[n] - W + 1))
        codes[s:s + W] = m
    return codes, offsets


def log2_scores(S):
    """go_log2 of every window score: log(S) / ln2 with the C library's log."""
    return np.array([math.log(float(s)) / LN2 if s > 0.0 else -math.inf for s in S], np.float64)


def detail_pcv(seqs: ol.Seqs, W, pc, pos, n, pcv49, counts):
    """(S, G) of target n as score_target computes them with a caller's
    ProbabilityCompositeVector (go_sweep_pcv): the PWM divides by pcv49 and the
    background products multiply it; `counts` is ol.counts(seqs, W, pos)[0]."""
    A = seqs.A
    src = seqs.codes[seqs.off[n]:seqs.off[n + 1]].astype(np.int64) - 42
    Cn = np.array(counts, np.int64).reshape(A, W).copy()
    aidx = {int(b) - 42: a for a, b in enumerate(seqs.alpha)}
    if pos[n] >= 0:
        for j in range(W):
            a = aidx.get(int(src[pos[n] + j]), -1)
            if a >= 0:
                Cn[a, j] -= 1
    pcv = np.asarray(pcv49, np.float64)
    den = float(seqs.n - 1) + float(A) * pc
    pwm = np.zeros((49, W), np.float64)
    for a in range(A):
        b = int(seqs.alpha[a]) - 42
        pwm[b] = ((Cn[a].astype(np.float64) + pc) / den) / pcv[b]
    K = len(src) - W + 1
    sv, gv = np.ones(K), np.ones(K)
    for j in range(W):  # the reference's left folds, every window at once
        sv = sv * pwm[src[j:j + K], j]
        gv = gv * pcv[src[j:j + K]]
    return sv, gv


class Target:
    """One target's categories and CDF edges, as the reference computes them."""

    def __init__(self, S, G, cutoff):
        self.K = len(G)
        self.G = np.asarray(G, np.float64)
        self.l2 = log2_scores(S)
        self.recut(cutoff)

    def recut(self, cutoff):
        """The categories at another cut-off (same snapshot)."""
        self.win = np.nonzero(self.l2 > cutoff)[0].astype(np.int32)  # the motif categories' windows
        self._set(np.concatenate([self.G, self.l2[self.win]]))
        return self

    def _set(self, w):
        self.w = w
        self.ncat = len(w)
        self.sum = float(np.cumsum(w)[-1])                 # List.sum: left to right from 0
        self.acc = np.concatenate([[0.0], np.cumsum(w / self.sum)])  # acc[i]: category i's left edge

    @property
    def npass(self):
        return self.ncat - self.K

    @property
    def acc_last(self):
        return float(self.acc[-1])

    def pick(self, u):
        """The first category i with acc_i <= u <= acc_i + w_i / sum; -1: the wheel runs
        off its end (the reference's list index throws)."""
        hit = np.nonzero((self.acc[:-1] <= u) & (u <= self.acc[1:]))[0]
        return int(hit[0]) if hit.size else -1

    def position(self, cat):
        """The sweep's output position of category `cat`: -1 for a background."""
        return -1 if cat < self.K else int(self.win[cat - self.K])

    def margin(self, u):
        """roulette()'s margin: the least |u - edge| over the edges it walked."""
        i = self.pick(u)
        last = self.ncat if i < 0 else i + 1
        return float(np.min(np.abs(u - self.acc[:last + 1])))

    def scaled(self, factors):
        """The same target with every motif weight times its factor."""
        t = object.__new__(Target)
        t.K, t.G, t.l2, t.win = self.K, self.G, self.l2, self.win
        w = self.w.copy()
        w[self.K:] = w[self.K:] * factors
        t._set(w)
        return t

    def unambiguous(self, u):
        """Does the pick stay when every motif weight moves by LOG_REL (all up, all
        down, alternating both ways)?  Log-free targets are always unambiguous."""
        if self.npass == 0:
            return True
        want = self.pick(u)
        alt = np.where(np.arange(self.npass) % 2 == 0, 1.0 + LOG_REL, 1.0 - LOG_REL)
        for f in (np.full(self.npass, 1.0 + LOG_REL), np.full(self.npass, 1.0 - LOG_REL), alt, 2.0 - alt):
            if self.scaled(f).pick(u) != want:
                return False
        return True


def targets(seqs: ol.Seqs, W, pc, cutoff, pos, pcv49=None):
    """Target(n) for every n of the snapshot."""
    out = []
    counts = ol.counts(seqs, W, pos)[0] if pcv49 is not None else None
    for n in range(seqs.n):
        if pcv49 is None:
            d = ol.target_detail(seqs, W, pc, pos, n)
            S, G = d["S"], d["G"]
        else:
            S, G = detail_pcv(seqs, W, pc, pos, n, pcv49, counts)
        out.append(Target(S, G, cutoff))
    return out


# ---- lane-block geometry of the kernels (where their prefix sums join) -----------
class Geometry:
    """joins(K): the category indices where two lanes' blocks of K windows meet;
    chunk: the windows a lane's block is walked at a time (0: it is walked whole)."""

    def __init__(self, joins, chunk, block):
        self.joins, self.chunk, self.block = joins, chunk, block


def _multiples(R, K):
    return np.arange(R, K, R, dtype=np.int64) if R > 0 else np.zeros(0, np.int64)


def geometry_groups(GL, quad=False):
    """gs_sweep_kernel: group lane l owns windows [l R, l R + R), R = ceil(K / GL)
    (rounded up to 4 for the pair tables' 16-lane groups); the pick walks the chosen
    lane's block GL windows at a time.  GL = 64 with R = ceil(K / 64) is also the
    binary64 rescan's and the exact scan's layout."""
    def block(K):
        R = (K + GL - 1) // GL
        return (R + 3) & ~3 if quad else R
    return Geometry(lambda K: _multiples(block(K), K), GL, block)


def geometry_packed(G):
    """The packed kernels (gs_sweep_dna / live / bg): lane `part` of G owns Rn windows,
    Rn = K (G = 1) or ceil(K / G) rounded up to 16, in blocks of 16 windows."""
    def block(K):
        return K if G == 1 else (((K + G - 1) // G) + 15) & ~15
    def joins(K):
        j = _multiples(block(K), K)
        return j if j.size else _multiples(16, K)
    return Geometry(joins, 16, block)


def geometry_long(lanes=16, bw=8):
    """gs_sweep_long_kernel: lane q of 16 owns K / 16 windows and one more in the first
    K % 16 lanes, in blocks of 8 windows."""
    def joins(K):
        q = np.arange(1, lanes, dtype=np.int64)
        x0 = q * (K // lanes) + np.minimum(q, K % lanes)
        return np.unique(x0[(x0 > 0) & (x0 < K)])
    return Geometry(joins, bw, lambda K: (K + lanes - 1) // lanes)


def choose_edges(ts, geo: Geometry, seed):
    """One edge c (1 <= c <= ncat - 1) per target, the kinds rotating over n mod 6:
    0 the phase edge c = K (the last background and the first motif category), 1 a
    background edge at a lane-block join, 2 the background edge c = chunk inside the first
    lane's block (when the block is longer), 3 a random interior edge, 4 the first /
    last interior edge alternating, 5 a random edge between two motif categories.  A
    kind the target does not have falls to 3.  Returns (c[n], kind[n])."""
    rng = np.random.default_rng(seed)
    c = np.zeros(len(ts), np.int64)
    kind = np.zeros(len(ts), np.int64)
    for n, t in enumerate(ts):
        assert t.ncat >= 2, f"target {n} has a single category"
        k, e = n % N_KINDS, -1
        if k == 0 and t.npass > 0:
            e = t.K
        elif k == 1:
            j = geo.joins(t.K)
            e = int(j[rng.integers(0, len(j))]) if len(j) else -1
        elif k == 2 and geo.chunk and geo.block(t.K) > geo.chunk and geo.chunk < t.K:
            e = geo.chunk
        elif k == 4:
            e = 1 if (n // N_KINDS) % 2 == 0 else t.ncat - 1
        elif k == 5 and t.npass >= 2:
            e = int(rng.integers(t.K + 1, t.ncat))
        if e < 0:
            k, e = 3, int(rng.integers(1, t.ncat))
        c[n], kind[n] = e, k
    return c, kind


def edge_values(ts, c):
    return np.array([t.acc[int(ci)] for t, ci in zip(ts, c)], np.float64)


def probes_at_distance(ts, c, d):
    """u = acc_c + d and acc_c - d for every target, clipped to [0, TOP]."""
    e = edge_values(ts, c)
    return np.clip(e + d, 0.0, TOP), np.clip(e - d, 0.0, TOP)


def restated(ts, u):
    """(positions, margins) of the restatement for one u per target; position -2 where
    the wheel overruns."""
    pos = np.empty(len(ts), np.int32)
    mg = np.empty(len(ts), np.float64)
    for n, t in enumerate(ts):
        i = t.pick(float(u[n]))
        pos[n] = -2 if i < 0 else t.position(i)
        mg[n] = t.margin(float(u[n]))
    return pos, mg


def ambiguous(ts, u):
    """The targets whose probe violates the LOG_REL precondition."""
    return [n for n, t in enumerate(ts) if not t.unambiguous(float(u[n]))]


# ---- cut-off probes -----------------------------------------------------------------
def cutoff_windows(ts, pos, base_cutoff=1.0):
    """The (n*, k*) whose score the cut-off probes sit next to: a target's best window,
    its weakest passing window at `base_cutoff`, its strongest failing one (scores above
    0: a cut-off below 0 admits negative weights), a window of a target whose position
    is -1 (if any), and the snapshot's global maximum.  {name: (n, k, l2)}."""
    every = np.sort(np.concatenate([t.l2[np.isfinite(t.l2)] for t in ts]))

    def clear(x):  # the probes' precondition: nothing else within d / 2 of x +- d
        for d in D_CUTOFF:
            for cut in (x + d, x - d):
                i = np.searchsorted(every, cut)
                near = every[max(i - 1, 0):i + 1]
                if cut <= 0.0 or np.min(np.abs(near - cut)) < d / 2:
                    return False
        return True

    def pick(select):
        """The first target's window that `select` names and whose probes are clear."""
        for n, t in enumerate(ts):
            k = select(n, t)
            if k is not None and clear(float(t.l2[k])):
                return n, int(k)
        return None

    def weakest(n, t):
        p = np.nonzero(t.l2 > base_cutoff)[0]
        return p[np.argmin(t.l2[p])] if p.size else None

    def strongest_failing(n, t):
        f = np.nonzero(t.l2 <= base_cutoff)[0]
        return f[np.argmax(t.l2[f])] if f.size else None

    out = {
        "best": pick(lambda n, t: np.argmax(t.l2)),
        "weakest_passing": pick(weakest),
        "strongest_failing": pick(strongest_failing),
        "no_motif_target": pick(lambda n, t: np.argmax(t.l2) if pos[n] < 0 else None),
    }
    ng = int(np.argmax([t.l2.max() for t in ts]))
    out["global_max"] = (ng, int(np.argmax(ts[ng].l2)))
    return {k: (v[0], v[1], float(ts[v[0]].l2[v[1]])) for k, v in out.items() if v is not None}


def cutoff_clearance(ts, cutoff):
    """min |l2 - cutoff| over every window of every target."""
    return min(float(np.min(np.abs(t.l2[np.isfinite(t.l2)] - cutoff))) for t in ts)


def at_cutoff(ts, cutoff):
    """Copies of the targets with their categories at another cut-off."""
    out = []
    for t in ts:
        c = object.__new__(Target)
        c.K, c.G, c.l2 = t.K, t.G, t.l2
        out.append(c.recut(cutoff))
    return out


# ---- edges of the list path, from the oracle itself ---------------------------------
def list_snapshot(seqs, W, cap, seed):
    """A Positions-list snapshot: 0..cap in-bounds starts per sequence, the first one
    the initialiser's (so that windows and pairs pass the cut-off)."""
    rng = np.random.default_rng(seed)
    lens = seqs.lengths
    init = ol.random_starts(seqs, W, PC, seed=seed, mode=1)[1]
    cnt = rng.integers(0, cap + 1, len(lens)).astype(np.int32)
    pos = np.full((len(lens), cap), -1, np.int32)
    for n in range(len(lens)):
        pos[n, :cnt[n]] = rng.integers(0, lens[n] - W + 1, cnt[n])
        if cnt[n]:
            pos[n, 0] = init[n]
    return cnt, pos



def list_picks(seqs, M, W, pc, cutoff, cnt, pos, cap, u):
    """ol.sweep(..., motif_amount=M): ((cnt, pos), pwms, margin) and one int64 key per
    target that identifies its picked list."""
    (oc, op), pw, mg = ol.sweep(seqs, W, pc, cutoff, None, u, motif_amount=M, in_cnt=cnt,
                                in_pos=pos, in_cap=cap)
    # (the weight tells the background categories apart: they all pick [])
    key = np.ascontiguousarray(pw).view(np.int64) ^ (oc.astype(np.int64) << 56)
    for m in range(op.shape[1]):
        key = key * 100003 + np.where(m < oc, op[:, m], -1).astype(np.int64) + 1
    return (oc, op), pw, mg, key


def list_probes(lo, hi, d):
    """u = hi + d and lo - d, clipped to [0, TOP]."""
    return np.clip(hi + d, 0.0, TOP), np.clip(lo - d, 0.0, TOP)


def bisect_list_edges(seqs, M, W, pc, cutoff, cnt, pos, cap, seed, halvings=60):
    """Vectorised bisection on the oracle's sweep: per target two doubles lo < hi, at
    most 2^-53 apart, with different picks (an edge of the reference lies in (lo, hi]).
    Targets with a single category keep lo = hi = nan."""
    rng = np.random.default_rng(seed)
    N = seqs.n
    pick = lambda u: list_picks(seqs, M, W, pc, cutoff, cnt, pos, cap, u)[3]
    lo = rng.random(N) * 0.5
    hi = np.full(N, 0.999)  # (below every final acc: no overrun)
    klo, khi = pick(lo), pick(hi)
    for _ in range(8):  # a start whose pick differs from the top's
        same = klo == khi
        if not same.any():
            break
        lo = np.where(same, lo * 0.5, lo)
        klo = pick(lo)
    live = klo != khi
    for _ in range(halvings):
        mid = lo + (hi - lo) * 0.5
        km = pick(mid)
        left = km == klo
        lo = np.where(left, mid, lo)
        hi = np.where(left, hi, mid)
    lo[~live] = np.nan
    hi[~live] = np.nan
    return lo, hi


# ---- the snapshots the probes are built on ------------------------------------------
PC, CUT = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# name: (N, L, W, alphabet, start, cutoff, seed).  The smallest shapes that still reach
# the structure named: start "init" is getPWMOfRandomStarts' output (every target keeps
# a motif), "uniform" random positions (with cut-off 0 a median of ~20 windows pass)
SHAPES = {
    "atgc5": (64, 120, 6, b"ATGC-", "uniform", 0.0, 11),    # the general kernel's pair tables
    "dna12": (64, 120, 12, b"ACGT", "init", CUT, 12),       # 16-lane groups, one lane a target
    "dna8_300": (32, 300, 8, b"ACGT", "init", CUT, 13),     # 32-lane groups, R > 1
    "dna13_300": (32, 300, 13, b"ACGT", "init", CUT, 14),   # several 16-window blocks a lane
    "dna12_300": (32, 300, 12, b"ACGT", "init", CUT, 15),
    # 512 windows, the most gs_sweep_long_kernel takes (gs_long_fits): 32-window lane ranges
    "dna15_526": (32, 526, 15, b"ACGT", "init", CUT, 16),
    "protein": (32, 160, 20, PROTEIN, "init", CUT, 17),     # H = 1: binary32 scores
    "pcv10": (64, 120, 10, b"ACGT", "init", CUT, 18),       # the fixed-PCV twin
    # the wide width classes (WM = 64, 28, 20, 24, 48, 40; W = 61 and 41 with padding columns):
    # the bands' W terms at their largest, background products below the binary32 range
    "atgc5_w64": (32, 160, 64, b"ATGC-", "init", CUT, 31),  # the pair tables with fewer than 4 wavefronts
    "dna_w61": (32, 160, 61, b"ACGT", "init", CUT, 32),
    "dna_w28": (32, 120, 28, b"ACGT", "init", CUT, 33),     # the four-symbol kernel's unsplit table build
    "dna_w20": (32, 120, 20, b"ACGT", "init", CUT, 36),
    "dna_w24_300": (32, 300, 24, b"ACGT", "init", CUT, 37),
    "protein_w64": (32, 200, 64, PROTEIN, "init", CUT, 34),
    "protein_w41": (32, 200, 41, PROTEIN, "init", CUT, 35),
    "pcv_w40": (32, 160, 40, b"ACGT", "init", CUT, 38),
}
# the cut-off probe windows each shape yields (cutoff_windows): at W = 61 and 64 the window
# scores run from about -500 to +110 and no failing window scores above 0, so there is no
# strongest failing one to put a positive cut-off next to
CUTOFF_ALL = frozenset({"best", "weakest_passing", "strongest_failing", "no_motif_target", "global_max"})
CUTOFF_KEYS = {name: CUTOFF_ALL for name in SHAPES}
for _name in ("atgc5_w64", "dna_w61", "protein_w64"):
    CUTOFF_KEYS[_name] = CUTOFF_ALL - {"strongest_failing"}
_cache = {}


def fixed_pcv(alpha, seed):
    """A caller's ProbabilityCompositeVector: a probability vector over the alphabet,
    arbitrary values in the other slots."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.6, 49)
    v[[c - 42 for c in alpha]] = rng.dirichlet(np.ones(len(alpha)))
    return v


class Snapshot:
    """A shape's sequences with one input snapshot and its targets' edges.  logfree:
    every position -1 (no window of any target then passes the cut-off: asserted)."""

    def __init__(self, name, logfree=False):
        N, L, W, alpha, start, cutoff, seed = SHAPES[name]
        self.name, self.N, self.L, self.W, self.alpha, self.cutoff = name, N, L, W, alpha, cutoff
        self.logfree = logfree
        self.codes, self.offsets = dataset(N, L, W, alpha, seed)
        self.seqs = ol.Seqs(self.codes, self.offsets, alpha)
        self.pcv = fixed_pcv(alpha, seed) if name.startswith("pcv") else None
        if logfree:
            self.pos = np.full(N, -1, np.int32)
            self.cutoff = CUT
        elif start == "init":
            self.pos = ol.random_starts(self.seqs, W, PC, seed=seed, mode=1, pcv49=self.pcv)[1].astype(np.int32)
        else:
            lens = np.diff(self.offsets)
            self.pos = (np.random.default_rng(seed + 1).random(N) * (lens - W + 1)).astype(np.int32)
        if not logfree:
            self.pos[[3, N - 2]] = -1  # two targets without a motif of their own
        self.ts = targets(self.seqs, W, PC, self.cutoff, self.pos, self.pcv)
        if logfree:
            assert all(t.npass == 0 for t in self.ts), f"{name}: a window passes without any motif"

    def oracle(self, u, cutoff=None):
        """(positions, pwms, margins) of the oracle's sweep of this snapshot."""
        cutoff = self.cutoff if cutoff is None else cutoff
        if self.pcv is not None:
            return ol.sweep_pcv(self.seqs, self.W, PC, cutoff, self.pcv, self.pos, u)
        return ol.sweep(self.seqs, self.W, PC, cutoff, self.pos, u)

    def random_u(self, seed=0):
        return np.random.default_rng(1000 + seed).random(self.N)


def snapshot(name, logfree=False) -> Snapshot:
    key = (name, logfree)
    if key not in _cache:
        _cache[key] = Snapshot(name, logfree)
    return _cache[key]


def logfree_probes(snap: Snapshot, c):
    """The log-free snapshot's u vectors: exactly on acc_c and on the doubles next to it;
    target 0 takes u = 0.0 (category 0: acc <= pick holds at acc = 0) and the first two
    targets whose final acc is below TOP take u = acc_last (the last category) in the
    on-edge vector.  Returns ({name: u}, the targets with u = acc_last)."""
    e = edge_values(snap.ts, c)
    short = [n for n, t in enumerate(snap.ts) if n > 0 and t.acc_last < TOP][:2]
    on = e.copy()
    on[0] = 0.0
    for n in short:
        on[n] = snap.ts[n].acc_last
    return {"on": on, "below": np.nextafter(e, 0.0), "above": np.nextafter(e, 1.0)}, short
