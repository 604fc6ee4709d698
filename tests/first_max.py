"""First-maximum fixtures: repeat sequences whose argmax is an exact tie (CPU only).

Not a conftest and not collected: the helper of tests/test_first_max_host.py and
tests/test_gpu_first_max.py.

Every argmax of the reference is a first maximum: the strict `>` from (0.0, 0) of
getBestPWMSs / getBestPWMSsWithBPV (.fs:477, .fs:312) and the stable
List.sortByDescending |> List.head of the greedy passes (.fs:917-920, NaN lowest).
I.i.d. sequences with one planted motif almost never hold the same W-mer twice, so
they never ask which of two equal windows wins.  `repeats` tiles a short unit along
every sequence (microsatellites, poly-A tracts): the maximum is then attained by
several windows, often in different lanes, 64-window chunks and 512-thread blocks.

The replays walk the reference's passes visit by visit (ol.target_detail /
ol.counts for the star greedy, numpy left folds for the site scans, oracle/gibbs_ref.py
for the Positions lists) and must equal the oracle's own drivers exactly.  Per visit
they return the tied set at the maximum, the level of the pick, and the two
conditions under which the oracle's pick is the truth for a device whose log may
differ from the C library's in the last place (decision_edges.LOG_REL):

trap 1  every passing motif category whose product is at least P* (1 - 2^-40) (the
        kernels' own band) has a product bit-identical to P*, the pick's:
        no two distinct products whose logs might or might not compare equal.
        Background categories are compared as products and are exempt; the site
        scans compare products too.
trap 2  the fresh top value and the stored one (`pick.pwms > pwms[n]`, .fs:923;
        `sc > score[n]`, .fs:579) differ by more than 1e-9 relative (1000 x LOG_REL),
        or the stored value was written by an earlier visit of the same run from a
        bit-identical product (both sides then see exact equality), or one of them is
        not finite.  Start memories therefore hold 0.0, -inf, +1e9 and NaN, never an
        oracle sweep's logs.

Both are conditions on the inputs, asserted on the CPU; never a tolerance on the GPU's
positions.
"""
from __future__ import annotations

import math

import numpy as np

import decision_edges as de
from oracle import gibbs_ref as gr
from oracle import oracle_lib as ol

PC = 1e-4
BAND = 1.0 - 2.0 ** -40      # the kernels' near-maximum band
STORED_REL = 1e-9            # trap 2: 1000 x decision_edges.LOG_REL
PROTEIN = de.PROTEIN


# ---- the generator ------------------------------------------------------------------
def repeats(N, L, W, alpha=b"ACGT", seed=0, pmin=3, pmax=40, n_mut=2, prefix_rate=0.5,
            prefix_max=100, shared=0.6, lmin=None, extra=b"", n_extra=0):
    """N ragged sequences (lengths in [lmin, L], the first one L), each a unit of period
    pmin..pmax tiled from a random phase; a sequence takes its unit from a small shared
    pool with probability `shared` (so the count matrix is peaked), about `prefix_rate`
    of them carry a random non-periodic prefix of 0..prefix_max symbols, and each gets
    exactly `n_mut` point mutations in its periodic part (a count, not a rate: a rate
    leaves a long sequence without ties) and `n_extra` symbols of `extra` (non-alphabet
    codes).  Returns (codes, offsets)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(bytes(alpha), np.uint8)
    lo = max(2 * W, L // 3) if lmin is None else lmin
    lens = rng.integers(lo, L + 1, N)
    lens[0] = L
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    pool = [a[rng.integers(0, len(a), int(rng.integers(pmin, pmax + 1)))]
            for _ in range(max(1, N // 4))]
    codes = np.empty(int(offsets[-1]), np.uint8)
    for n in range(N):
        Ln = int(lens[n])
        if rng.random() < shared:
            unit = pool[int(rng.integers(0, len(pool)))]
        else:
            unit = a[rng.integers(0, len(a), int(rng.integers(pmin, pmax + 1)))]
        pre = 0
        if rng.random() < prefix_rate:
            pre = int(rng.integers(0, min(prefix_max, Ln - 2 * W) + 1))
        phase = int(rng.integers(0, len(unit)))
        body = np.tile(unit, (Ln - pre + phase) // len(unit) + 2)[phase:phase + Ln - pre]
        s = np.concatenate([a[rng.integers(0, len(a), pre)], body]).astype(np.uint8)
        for i in rng.choice(np.arange(pre, Ln), size=min(n_mut, Ln - pre), replace=False):
            s[i] = a[(int(np.nonzero(a == s[i])[0][0]) + 1 + int(rng.integers(0, len(a) - 1))) % len(a)]
        if extra and n_extra:
            e = np.frombuffer(bytes(extra), np.uint8)
            s[rng.choice(Ln, size=min(n_extra, Ln), replace=False)] = e[rng.integers(0, len(e), min(n_extra, Ln))]
        codes[offsets[n]:offsets[n + 1]] = s
    return codes, offsets


def start_memory(seqs: ol.Seqs, W, seed, none_rate=0.1):
    """A start snapshot for the greedy passes: the initialiser's positions (a peaked
    count matrix, so that windows pass the cut-off; a few [] = -1) and stored PWMS of
    0.0, with -inf, +1e9 (never accepts) and NaN (never accepts) on a few targets:
    never an oracle sweep's logs (trap 2)."""
    rng = np.random.default_rng(seed)
    N = seqs.n
    pos = ol.random_starts(seqs, W, PC, seed=seed, mode=1)[1].astype(np.int32)
    pos[rng.random(N) < none_rate] = -1
    pw = np.zeros(N)
    if N >= 8:
        pick = rng.choice(N, size=4, replace=False)
        pw[pick[0]] = -np.inf
        pw[pick[1]] = 1e9
        pw[pick[2]] = np.nan
        pw[pick[3]] = -np.inf
    return pos, pw


def start_scores(N, seed):
    """Stored scores for the site refinements: -inf (every target takes its first scan),
    0.0, and +1e9 / NaN on a few targets."""
    rng = np.random.default_rng(seed)
    sc = np.where(rng.random(N) < 0.5, -np.inf, 0.0)
    if N >= 8:
        pick = rng.choice(N, size=2, replace=False)
        sc[pick[0]] = 1e9
        sc[pick[1]] = np.nan
    return sc


# ---- per-visit records --------------------------------------------------------------
class Visit:
    """One visit of a pass: target n, the windows (or categories, for lists) tied at the
    maximum in category order, the pick's level (0 background, m = a list of m
    positions; site scans: 1), and the two trap conditions."""
    __slots__ = ("n", "npass", "tied", "level", "trap1", "trap2")

    def __init__(self, n, npass, tied, level, trap1, trap2):
        self.n, self.npass, self.tied, self.level = n, npass, tied, level
        self.trap1, self.trap2 = trap1, trap2


def _stored_ok(top, top_prod, stored, stored_prod):
    """Trap 2 for one visit."""
    if not (math.isfinite(top) and math.isfinite(stored)):
        return True  # infinities and NaN compare alike under any log
    if stored_prod is not None and top_prod == stored_prod:
        return True  # written by this run from a bit-identical product
    return abs(top - stored) > STORED_REL * max(abs(top), abs(stored))


def _band_ok(prods, P):
    """Trap 1: every product in [P BAND, inf) is bit-identical to P."""
    prods = np.asarray(prods, np.float64)
    return bool(np.all(prods[prods >= P * BAND] == P))


# ---- the star greedy (motifAmount 1), plain and ByPCV --------------------------------
def replay_greedy(seqs: ol.Seqs, W, pc, cutoff, pos, pwms, max_passes=1000, pcv49=None):
    """findBestMotifIndicesWithStartPositions (.fs:885-929) with motifAmount 1, or its
    ByPCV twin (.fs:788-823): (pos, pwms, passes, visits)."""
    N = seqs.n
    pos = np.array(pos, np.int32, copy=True)
    pw = np.array(pwms, np.float64, copy=True)
    src = [None] * N
    visits, passes = [], 0
    while True:
        best = pos.copy()
        passes += 1
        for n in range(N):
            if pcv49 is None:
                d = ol.target_detail(seqs, W, pc, pos, n)
                S, G = d["S"], d["G"]
            else:
                S, G = de.detail_pcv(seqs, W, pc, pos, n, pcv49, ol.counts(seqs, W, pos)[0])
            K = len(G)
            l2 = de.log2_scores(S)
            win = np.nonzero(l2 > cutoff)[0]
            w = np.concatenate([G, l2[win]])
            prod = np.concatenate([G, S[win]])
            kk = np.concatenate([np.arange(K), win])
            assert not np.isnan(w).any()
            i = int(np.argmax(w))  # the first maximum
            level = 0 if i < K else 1
            same = np.nonzero(w == w[i])[0]
            same = same[(same < K) == (i < K)]
            t1 = True
            if level:
                t1 = _band_ok(prod[K:], prod[i])
            other = w[K:] if level == 0 else w[:K]  # a log against a product
            if other.size:
                t1 = t1 and abs(w[i] - other.max()) > STORED_REL * abs(w[i])
            t2 = _stored_ok(float(w[i]), float(prod[i]), float(pw[n]), src[n])
            visits.append(Visit(n, passes, kk[same].astype(np.int64), level, t1, t2))
            if w[i] > pw[n]:
                pw[n], src[n] = w[i], float(prod[i])
                pos[n] = -1 if i < K else int(kk[i])
        if np.array_equal(best, pos) or passes >= max_passes:
            break
    return pos, pw, passes, visits


# ---- the site sampler's scans -------------------------------------------------------
class SiteData:
    """Per-sequence slot codes and compositions, computed once."""

    def __init__(self, seqs: ol.Seqs):
        self.seqs = seqs
        self.src = [seqs.codes[seqs.off[n]:seqs.off[n + 1]].astype(np.int64) - 42
                    for n in range(seqs.n)]
        self.comp = np.array([np.bincount(s, minlength=49) for s in self.src], np.int64)
        self.slots = seqs.alpha.astype(np.int64) - 42
        self.aidx = np.full(49, -1, np.int64)
        self.aidx[self.slots] = np.arange(seqs.A)


def site_inputs(sd: SiteData, W, pc, n, r):
    """(bg[49], ppm[A, W]) of target n with every other sequence m at r[m] (.fs:565-577)."""
    N, A = sd.seqs.n, sd.seqs.A
    bg = np.zeros(49, np.int64)
    pfm = np.zeros((A, W), np.int64)
    for m in range(N):
        if m == n:
            continue
        seg = sd.src[m][r[m]:r[m] + W]
        c = sd.comp[m] - np.bincount(seg, minlength=49)
        bg[sd.slots] += c[sd.slots]
        a = sd.aidx[seg]
        ok = a >= 0
        np.add.at(pfm, (a[ok], np.nonzero(ok)[0]), 1)
    den = float(N - 1) + float(A) * pc
    return bg, (pfm.astype(np.float64) + pc) / den


def scan_products(sd: SiteData, W, pc, n, bg, ppm, pcv49=None):
    """The K window scores of getBestPWMSsWithBPV (pcv49 given, .fs:301-313) or
    getBestPWMSs (.fs:462-479, the composite vector drifting window by window): the
    reference's left folds, every window at once."""
    src = sd.src[n]
    A = sd.seqs.A
    K = len(src) - W + 1
    sv = np.ones(K)
    a_of = sd.aidx[src]
    if pcv49 is not None:
        pcv = np.asarray(pcv49, np.float64)
        for j in range(W):
            b, a = src[j:j + K], a_of[j:j + K]
            sv = sv * np.where(a >= 0, ppm[np.maximum(a, 0), j] / pcv[b], 0.0)
        return sv
    # fcv after window k: bg + (k + 1) comp(source) - the segments' counts so far (the
    # clamp at 0 of substractSegmentCountsFrom never binds: a segment is part of the
    # source that was just added)
    onehot = np.zeros((len(src), 49), np.int64)
    onehot[np.arange(len(src)), src] = 1
    pre = np.concatenate([np.zeros((1, 49), np.int64), np.cumsum(onehot, axis=0)])
    segc = pre[W:W + K] - pre[:K]
    fcv = bg[None, :] + np.arange(1, K + 1)[:, None] * sd.comp[n][None, :] - np.cumsum(segc, axis=0)
    assert (fcv >= 0).all()
    tot = fcv.sum(axis=1).astype(np.float64) + float(A) * pc
    rows = np.arange(K)
    for j in range(W):
        b, a = src[j:j + K], a_of[j:j + K]
        p = (fcv[rows, b].astype(np.float64) + pc) / tot
        sv = sv * np.where(a >= 0, ppm[np.maximum(a, 0), j] / p, 0.0)
    return sv


def first_max_scan(sv):
    """`if tmp > high` from (0.0, 0): (log2 score, position, product, tied windows)."""
    m = float(sv.max())
    if not m > 0.0:
        return -math.inf, 0, 0.0, np.arange(len(sv), dtype=np.int64)
    k = int(np.argmax(sv))
    return math.log(m) / de.LN2, k, m, np.nonzero(sv == m)[0].astype(np.int64)


def replay_site_scan(seqs: ol.Seqs, W, pc, r, pcv49=None):
    """ol.site_scan: (score, pos, visits)."""
    sd = SiteData(seqs)
    N = seqs.n
    score, pos, visits = np.zeros(N), np.zeros(N, np.int32), []
    for n in range(N):
        bg, ppm = site_inputs(sd, W, pc, n, r)
        score[n], pos[n], _, tied = first_max_scan(scan_products(sd, W, pc, n, bg, ppm, pcv49))
        visits.append(Visit(n, 1, tied, 1, True, True))
    return score, pos, visits


def replay_site_refine(seqs: ol.Seqs, W, pc, shift, pos, score, max_passes=1000, pcv49=None):
    """ol.site_refine: (pos, score, passes, visits)."""
    sd = SiteData(seqs)
    N = seqs.n
    lens = seqs.lengths
    pos = np.array(pos, np.int32, copy=True)
    score = np.array(score, np.float64, copy=True)
    src = [None] * N
    visits, passes = [], 0
    while True:
        best = pos.copy()
        passes += 1
        if shift > 0:
            r = np.where(best <= lens - W - 1, best + 1, best)
        elif shift < 0:
            r = np.where(best > 0, best - 1, best)
        for n in range(N):
            bg, ppm = site_inputs(sd, W, pc, n, pos if shift == 0 else r)
            sc, p, prod, tied = first_max_scan(scan_products(sd, W, pc, n, bg, ppm, pcv49))
            visits.append(Visit(n, passes, tied, 1, True,
                                _stored_ok(sc, prod, float(score[n]), src[n])))
            if sc > score[n]:
                score[n], pos[n], src[n] = sc, p, prod
        if np.array_equal(best, pos) or passes >= max_passes:
            break
    return pos, score, passes, visits


# ---- the list greedy (motifAmount >= 2), after oracle/gibbs_ref.py --------------------
def _list_cats(cutoff, M, W, source, pcv, pwm):
    """calculateNormalizedSegmentScores (.fs:759-784) with every category's product kept:
    [(weight, positions, product)], backgrounds first, then the levels 1..M."""
    K = len(source) - W + 1
    segs = [list(source[k:k + W]) for k in range(K)]
    items = [(gr.pwm_segment_score(pwm, s), k) for k, s in enumerate(segs)]
    cats = []
    for s in segs:
        g = gr.bg_segment_score(pcv, s)
        cats.append((g, [], g))

    def loop(prob, positions, size, i):  # calculatePWMsForSegmentCombinations (.fs:727-742)
        if i < len(items):
            x = items[i]
            if size > 0 and gr.ceckForDistance(W, [x[1]] + positions) \
                    and gr.log2(x[0] * prob) > cutoff:
                loop(x[0] * prob, [x[1]] + positions, size - 1, i + 1)
            if size >= 0:
                loop(prob, positions, size, i + 1)
        elif size == 0:
            cats.append((gr.log2(prob), positions, prob))

    for m in range(1, M + 1):
        loop(1.0, [], m, 0)
    return cats, K


def replay_greedy_lists(seqs: ol.Seqs, M, W, pc, cutoff, cnt, pos, pwms, max_passes=1000):
    """ol.greedy_lists (cap = M): (cnt, pos, pwms, passes, visits)."""
    N = seqs.n
    alphabet = [int(c) for c in seqs.alpha]
    sources = [[int(c) for c in seqs.codes[seqs.off[n]:seqs.off[n + 1]]] for n in range(N)]
    pos = np.asarray(pos, np.int32).reshape(N, M)
    acc = [(float(pwms[n]), [int(p) for p in pos[n, :cnt[n]]]) for n in range(N)]
    src = [None] * N
    visits, passes = [], 0
    while True:
        best = [list(ps) for _, ps in acc]
        passes += 1
        for n in range(N):
            pcv, pwm = gr._target_pwm(W, pc, alphabet, sources, acc, n)
            cats, K = _list_cats(cutoff, M, W, sources[n], pcv, pwm)
            w = np.array([c[0] for c in cats])
            prod = np.array([c[2] for c in cats])
            assert not np.isnan(w).any()
            i = int(np.argmax(w))
            level = len(cats[i][1])
            same = np.nonzero(w == w[i])[0]
            same = same[(same < K) == (i < K)]
            t1 = True
            if level:
                t1 = _band_ok(prod[K:], prod[i])
            other = w[K:] if level == 0 else w[:K]
            if other.size:
                t1 = t1 and abs(w[i] - other.max()) > STORED_REL * abs(w[i])
            t2 = _stored_ok(float(w[i]), float(prod[i]), acc[n][0], src[n])
            visits.append(Visit(n, passes, same.astype(np.int64), level, t1, t2))
            if w[i] > acc[n][0]:
                acc[n], src[n] = (float(w[i]), list(cats[i][1])), float(prod[i])
        if [ps for _, ps in acc] == best or passes >= max_passes:
            break
    oc = np.array([len(ps) for _, ps in acc], np.int32)
    op = np.full((N, M), -1, np.int32)
    for n, (_, ps) in enumerate(acc):
        op[n, :len(ps)] = ps
    return oc, op, np.array([p for p, _ in acc]), passes, visits


# ---- geometry of the tied sets ------------------------------------------------------
def geometry(visits, levels=None):
    """The counts the host test asserts, over the targets with at least one visit that
    ties at the maximum: `tie` such targets; `lane` those where a later tied window has
    a lower k mod 64 than the first; `late` those whose first tied window has k >= 64;
    `block` those with tied windows in different 512-blocks, a later one at a lower
    k mod 512; `bg` / `motif` the tying targets by the pick's level."""
    sets = {"tie": set(), "lane": set(), "late": set(), "block": set(), "bg": set(),
            "motif": set()}
    for v in visits:
        if len(v.tied) < 2 or (levels is not None and v.level not in levels):
            continue
        k0, rest = int(v.tied[0]), v.tied[1:]
        sets["tie"].add(v.n)
        sets["bg" if v.level == 0 else "motif"].add(v.n)
        if (rest % 64 < k0 % 64).any():
            sets["lane"].add(v.n)
        if k0 >= 64:
            sets["late"].add(v.n)
        if ((rest // 512 != k0 // 512) & (rest % 512 < k0 % 512)).any():
            sets["block"].add(v.n)
    return {k: len(s) for k, s in sets.items()}


def traps(visits):
    """The visits that violate trap 1 / trap 2."""
    return ([(v.npass, v.n) for v in visits if not v.trap1],
            [(v.npass, v.n) for v in visits if not v.trap2])


# ---- the fixture table ---------------------------------------------------------------
# name: the generator's arguments; seeds tuned on the CPU until test_first_max_host.py's
# conditions hold (the thresholds are the issue's, never tuned).  The smallest shapes
# that still exercise the geometry: K > 64 (lanes and 64-window chunks), and for `wide`
# K > 1024 (512-thread blocks, L > 1024 staging).
FIXTURES = {
    "dna": dict(N=40, L=300, W=8, alpha=b"ACGT", seed=1),
    "atgc": dict(N=40, L=300, W=12, alpha=b"ATGC-", seed=21, pmax=20, extra=b"*", n_extra=1),
    "protein": dict(N=30, L=300, W=10, alpha=PROTEIN, seed=1, lmin=150),
    "wide": dict(N=16, L=1500, W=9, alpha=b"ACGT", seed=2, lmin=1100, n_mut=1, prefix_max=120, shared=0.8),
}
LIST_FIXTURES = {
    "lists2": dict(N=12, L=60, W=6, M=2, alpha=b"ACGT", seed=1, pmin=3, pmax=40, n_mut=1,
                   prefix_max=10),
    "lists3": dict(N=10, L=48, W=5, M=3, alpha=b"ACGT", seed=1, pmin=2, pmax=9, n_mut=1,
                   prefix_max=8),
}
CUTOFFS = (1.0, 1e9)  # 1e9: no window passes, the background categories alone
_cache = {}


class Fixture:
    """A named case: sequences, a start snapshot, a fixed PCV, and (lazily, once) the
    oracle's results and the replays' visits."""

    def __init__(self, name):
        kw = dict(FIXTURES[name])
        self.name = name
        self.N, self.L, self.W, self.alpha = kw.pop("N"), kw.pop("L"), kw.pop("W"), kw.pop("alpha")
        self.seed = kw.pop("seed")
        self.codes, self.offsets = repeats(self.N, self.L, self.W, self.alpha, self.seed, **kw)
        self._finish()

    def _finish(self):
        self.seqs = ol.Seqs(self.codes, self.offsets, self.alpha)
        self.pos0, self.pw0 = start_memory(self.seqs, self.W, self.seed + 100)
        self.pcv = de.fixed_pcv(self.alpha, self.seed + 200)
        # the scans' start positions: the initialiser's (a peaked matrix: the best window
        # is then one of the repeat's, not a unique one of a prefix)
        self.r0 = ol.random_starts(self.seqs, self.W, PC, seed=self.seed + 300, mode=1)[1].astype(np.int32)
        self.sc0 = start_scores(self.N, self.seed + 400)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    # the oracle's drivers (computed once, shared, never changed)
    def greedy(self, cutoff, max_passes=1000, pcv=False):
        p = self.pcv if pcv else None
        if pcv:
            f = lambda: ol.greedy_pcv(self.seqs, self.W, PC, cutoff, p, self.pos0, self.pw0, max_passes)
        else:
            f = lambda: ol.greedy(self.seqs, self.W, PC, cutoff, self.pos0, self.pw0,
                                  max_passes=max_passes)
        return self.memo(("greedy", cutoff, max_passes, pcv), f)

    def site_scan(self, pcv=True):
        p = self.pcv if pcv else None
        return self.memo(("scan", pcv), lambda: ol.site_scan(self.seqs, self.W, PC, self.r0, pcv49=p))

    def site_refine(self, shift, pcv=True, max_passes=1000):
        p = self.pcv if pcv else None
        return self.memo(("refine", shift, pcv, max_passes),
                         lambda: ol.site_refine(self.seqs, self.W, PC, shift, self.r0, self.sc0,
                                                max_passes, pcv49=p))

    # the replays
    def replay_greedy(self, cutoff, pcv=False):
        p = self.pcv if pcv else None
        return self.memo(("rgreedy", cutoff, pcv),
                         lambda: replay_greedy(self.seqs, self.W, PC, cutoff, self.pos0, self.pw0,
                                               pcv49=p))

    def replay_site_scan(self, pcv=True):
        p = self.pcv if pcv else None
        return self.memo(("rscan", pcv),
                         lambda: replay_site_scan(self.seqs, self.W, PC, self.r0, pcv49=p))

    def replay_site_refine(self, shift, pcv=True):
        p = self.pcv if pcv else None
        return self.memo(("rrefine", shift, pcv),
                         lambda: replay_site_refine(self.seqs, self.W, PC, shift, self.r0,
                                                    self.sc0, pcv49=p))


class ZeroFixture(Fixture):
    """The `dna` shape with three sequences replaced: 0 holds a non-alphabet symbol in
    every window (the scan's pick is (log2 0., 0)), 1 only scores above zero in windows
    k >= 64, 2 is a homopolymer (all K windows tie)."""

    def __init__(self):
        self.name = "zero"
        self.N, self.L, self.W, self.alpha, self.seed = 12, 200, 8, b"ACGT", 7
        self.codes, self.offsets = repeats(self.N, self.L, self.W, self.alpha, self.seed, lmin=150)
        W, star = self.W, ord("*")
        s0 = self.codes[self.offsets[0]:self.offsets[1]]
        s0[W - 1::W] = star
        s1 = self.codes[self.offsets[1]:self.offsets[2]]
        s1[W - 1:64:W] = star
        s1[63] = star
        self.codes[self.offsets[2]:self.offsets[3]] = ord("A")
        self._finish()
        self.sc0[:3] = -np.inf
        self.pw0[:3] = 0.0


class ListFixture:
    """A Positions-list case: sequences, start lists (0..M starts each) and stored PWMS."""

    def __init__(self, name):
        kw = dict(LIST_FIXTURES[name])
        self.name = name
        self.N, self.L, self.W, self.M = kw.pop("N"), kw.pop("L"), kw.pop("W"), kw.pop("M")
        self.alpha, self.seed = kw.pop("alpha"), kw.pop("seed")
        self.codes, self.offsets = repeats(self.N, self.L, self.W, self.alpha, self.seed,
                                           lmin=self.L * 2 // 3, **kw)
        self.seqs = ol.Seqs(self.codes, self.offsets, self.alpha)
        rng = np.random.default_rng(self.seed + 100)
        lens = np.diff(self.offsets)
        self.cnt0 = rng.integers(0, self.M + 1, self.N).astype(np.int32)
        self.pos0 = np.full((self.N, self.M), -1, np.int32)
        for n in range(self.N):
            self.pos0[n, :self.cnt0[n]] = rng.integers(0, lens[n] - self.W + 1, self.cnt0[n])
        self.pw0 = np.zeros(self.N)
        self.pw0[[1, self.N - 2]] = -np.inf, np.nan
        self.pw0[self.N // 2] = 1e9
        self._memo = {}

    memo = Fixture.memo

    def greedy(self, cutoff=1.0, max_passes=1000):
        return self.memo(("greedy", cutoff, max_passes),
                         lambda: ol.greedy_lists(self.seqs, self.M, self.W, PC, cutoff, self.cnt0,
                                                 self.pos0, self.M, self.pw0, max_passes))

    def replay(self, cutoff=1.0):
        return self.memo(("replay", cutoff),
                         lambda: replay_greedy_lists(self.seqs, self.M, self.W, PC, cutoff,
                                                     self.cnt0, self.pos0, self.pw0))


def fixture(name):
    if name not in _cache:
        _cache[name] = (ZeroFixture() if name == "zero" else
                        ListFixture(name) if name in LIST_FIXTURES else Fixture(name))
    return _cache[name]


# ---- what the host test asserts, fixture by fixture ---------------------------------
NEED = {"tie": 8, "lane": 5, "late": 2}  # the thresholds (never tuned; the seeds are)
NEED_BLOCK = 2                           # for `wide`
NEED_LAST_LEVEL = 3                      # for lists: visits tying at level motifAmount


def same(a, b):
    """Exact equality of result tuples (NaN equal to NaN)."""
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def runs(f: Fixture):
    """Every replay of a star / site fixture against the oracle's driver:
    [(label, replay equals oracle, visits, is a tie case)].  The tie cases carry the
    geometry thresholds; the others (ByPCV greedy, refinements, the drifting
    background) only the equality and the trap conditions."""
    out = []
    for cut in CUTOFFS:
        r = f.replay_greedy(cut)
        out.append((f"greedy cut-off {cut:g}", same(r[:3], f.greedy(cut)), r[3], True))
    r = f.replay_greedy(1.0, pcv=True)
    out.append(("greedy ByPCV", same(r[:3], f.greedy(1.0, pcv=True)), r[3], False))
    r = f.replay_site_scan()
    out.append(("site scan fixed PCV", same(r[:2], f.site_scan()), r[2], True))
    r = f.replay_site_scan(False)
    out.append(("site scan drifting", same(r[:2], f.site_scan(False)), r[2], False))
    for shift in (0, -1, 1):
        for pcv in (True, False):
            r = f.replay_site_refine(shift, pcv)
            out.append((f"site refine shift {shift} {'fixed PCV' if pcv else 'drifting'}",
                        same(r[:3], f.site_refine(shift, pcv)), r[3], False))
    return out


def list_run(f: ListFixture):
    """(replay equals oracle, visits, visits that tie at the last level)."""
    r, o = f.replay(), f.greedy()
    used = np.arange(f.M)[None, :] < o[0][:, None]
    eq = same(r[:4], (o[0], np.where(used, o[1], -1), o[2], o[3]))
    last = sum(1 for v in r[4] if v.level == f.M and len(v.tied) >= 2)
    return eq, r[4], last
