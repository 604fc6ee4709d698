"""Host-side mirror of the reference's F# entry points for the hot path.

Same names, argument order and meaning as GibbsSampling.fs; the work runs in
libgibbs_hip.so on the GPU.  Error behaviour follows the .NET exceptions the
reference raises (see _native.py for the mapping).
"""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import Callable, Sequence

import numpy as np

from . import _native
from .bioarray import alphabet_codes, pack


@dataclass(frozen=True)
class MotifIndex:
    """MotifSampler.MotifIndex (.fs:712-716)."""
    PWMS: float
    Positions: tuple


def createMotifIndex(pwms: float, pos) -> MotifIndex:       # .fs:719-723
    return MotifIndex(float(pwms), tuple(int(p) for p in pos))


#: the reference loops until a pass moves nothing (.fs:886-888, .fs:556-559); the
#: mirror's default pass cap is effectively unbounded, and a run that reaches an
#: explicit cap warns instead of passing for converged
UNBOUNDED = 2**31 - 1


def _passes(passes: int, max_passes: int) -> None:
    if max_passes < UNBOUNDED and passes >= max_passes:
        import warnings
        warnings.warn(f"refinement stopped at max_passes={max_passes}; the last pass may "
                      "still have moved positions (the reference loops until none moves)",
                      RuntimeWarning, stacklevel=3)


_contexts: dict[int, _native.Context] = {}


def context(device: int = 0) -> _native.Context:
    if device not in _contexts:
        _contexts[device] = _native.Context(device)
    return _contexts[device]


class _Bound:
    """Keeps the (sources, alphabet) last handed to a context to avoid re-uploads."""

    def __init__(self, ctx: _native.Context):
        self.ctx = ctx
        self.key = None

    def bind(self, alphabet, sources) -> None:
        codes, offsets = pack(sources)
        alpha = alphabet_codes(alphabet)
        key = (alpha, offsets.tobytes(), hash(codes.tobytes()))
        if key != self.key:
            self.ctx.set_sequences(codes, offsets, alpha)
            self.key = key


_bound: dict[int, _Bound] = {}


def _bind(alphabet, sources, device: int) -> _native.Context:
    if device not in _bound:
        _bound[device] = _Bound(context(device))
    _bound[device].bind(alphabet, sources)
    return _bound[device].ctx


def _uniforms(rnd, n: int) -> np.ndarray:
    """The n NextDouble() draws of `let rnd = new System.Random()` (.fs:936)."""
    if rnd is None:
        return np.random.default_rng().random(n)
    if isinstance(rnd, np.random.Generator):
        return rnd.random(n)
    if callable(rnd):
        return np.array([float(rnd()) for _ in range(n)], np.float64)
    if hasattr(rnd, "NextDouble"):
        return np.array([float(rnd.NextDouble()) for _ in range(n)], np.float64)
    u = np.asarray(rnd, np.float64)
    if u.shape != (n,):
        raise _native.ArgumentError(_native.GS_E_ARG, "need one uniform per sequence")
    return u


def _single_positions(motifMem: Sequence[MotifIndex]) -> np.ndarray:
    pos = np.empty(len(motifMem), np.int32)
    for i, m in enumerate(motifMem):
        pos[i] = m.Positions[0] if m.Positions else -1
    return pos


def informationContent(pwms) -> float:
    """The sum of a state's PWMS (the reference's quality of a run, .fs:981-989) in the
    fixed binary64 order of the device's trace (gs_motif_run_batch_stats): 64 partial sums
    v[l] from +0.0, v[l] adding the entries n = l, l + 64, ... in increasing n; then for
    s = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + s] for l < s; the result is v[0]."""
    x = np.ascontiguousarray(pwms, np.float64).ravel()
    # (padded with +0.0: a partial sum that started from +0.0 is never -0.0, so adding
    # +0.0 changes no bit)
    pad = np.zeros((-len(x)) % 64, np.float64)
    v = np.zeros(64, np.float64)
    for row in np.concatenate([x, pad]).reshape(-1, 64):
        v = v + row
    s = 32
    while s >= 1:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return float(v[0])


@dataclass
class ChainAgreement:
    """Whether pooling R chains was justified: the chains against the pool of
    the n_pooled chains that finished.  With pool the sum of the pooled chains' bins, D(r, n)
    is the sum over sequence n's bins of |n_pooled occupancy[r] - pool|, an integer; D / (2
    n_pooled n_counted) is the total variation distance between chain r's marginal of the
    sequence and the pooled marginal.  agree[N]: the pooled chains whose most frequent bin of
    the sequence (the first among equals) is the pool's.  spread[N] (int64) / spread_chain[N]:
    the largest D(r, n) over the pooled chains and the lowest chain that has it; (0, 0, -1)
    without a pooled chain.  chain_dist[R] (int64): the sum of D(r, n) over the sequences;
    chain_agree[R]: the sequences whose chain mode is the pool's; (-1, -1) for a chain that is
    not pooled.  n_counted: the counted sweeps of a chain."""
    agree: np.ndarray
    spread: np.ndarray
    spread_chain: np.ndarray
    chain_agree: np.ndarray
    chain_dist: np.ndarray
    n_pooled: int
    n_counted: int

    def distance(self) -> np.ndarray:
        """[N] float64: per sequence the largest total variation distance between a pooled
        chain's marginal and the pooled one, spread / (2 n_pooled n_counted); 0 without a
        pooled counted state."""
        den = 2.0 * float(int(self.n_pooled) * int(self.n_counted))
        x = np.asarray(self.spread, np.float64)
        return x / den if den > 0 else np.zeros_like(x)

    def outliers(self, threshold: float) -> np.ndarray:
        """The pooled chains whose total variation distance to the pool, averaged over the
        sequences, chain_dist / (2 n_pooled n_counted N), exceeds threshold."""
        den = 2.0 * float(int(self.n_pooled) * int(self.n_counted) * len(self.agree))
        d = np.asarray(self.chain_dist)
        if den <= 0:
            return np.zeros(0, np.int64)
        return np.nonzero((d >= 0) & (d.astype(np.float64) / den > threshold))[0]


def _rhat(ic, keep) -> float:
    """The Gelman-Rubin potential scale reduction of the traces ic[keep] (m chains of n
    entries), in binary64: B / n the variance of the chain means, Wv the mean of the chains'
    variances (both ddof 1); sqrt(((n - 1) / n Wv + B / n) / Wv).  NaN with fewer than two
    chains or entries, Wv == 0, or a NaN in a trace."""
    x = np.asarray(ic, np.float64)[np.asarray(keep, bool)]
    m, n = x.shape if x.ndim == 2 else (0, 0)
    if m < 2 or n < 2 or np.isnan(x).any():
        return float("nan")
    b_over_n = float(np.var(x.mean(axis=1), ddof=1))
    wv = float(np.mean(np.var(x, axis=1, ddof=1)))
    if wv == 0:
        return float("nan")
    return float(np.sqrt(((n - 1) / n * wv + b_over_n) / wv))


@dataclass
class ChainStats:
    """What MotifSampler.runSweepsBatchedStats gathered over the counted sweeps of R chains
    (MotifSampler.runSweepsStats: of the single chain, R = 1).
    occupancy[R, H]: the counted sweeps whose state has its sequence at that bin; sequence n
    owns the bins offsets[n] .. offsets[n + 1] - 1, the first one counting Positions [], bin
    offsets[n] + 1 + k start k.  ic[R, n_counted]: informationContent of every counted
    sweep (NaN from the sweep in which a chain raised).  best_sweep[R] and best[R]: the
    sweep of each chain's first largest ic (-1: none) and its state."""
    occupancy: np.ndarray
    offsets: np.ndarray
    ic: np.ndarray
    best_sweep: np.ndarray
    best: list

    def finished(self) -> np.ndarray:
        """[R] bool: the chains every counted sweep of which was counted (a chain that
        raised stops counting in that sweep)."""
        off = self.offsets
        if len(off) < 2:
            return np.ones(len(self.occupancy), bool)
        return self.occupancy[:, off[0]:off[1]].sum(axis=1) == self.ic.shape[1]

    def marginals(self, pool: bool = True) -> list:
        """Per sequence the occupancy of its bins divided by the counted sweeps: pooled
        over the finished chains (one array of 1 + L_n - W + 1 frequencies a sequence), or
        with pool=False chain by chain ([R, bins] a sequence, each chain over its own
        counted sweeps).  Without any counted state the frequencies are 0."""
        occ = np.asarray(self.occupancy, np.float64)
        off = self.offsets
        if pool:
            keep = self.finished()
            total = occ[keep].sum(axis=0)
            den = float(keep.sum() * self.ic.shape[1])
            total = total / den if den > 0 else np.zeros_like(total)
            return [total[off[n]:off[n + 1]] for n in range(len(off) - 1)]
        out = []
        for n in range(len(off) - 1):
            part = occ[:, off[n]:off[n + 1]]
            den = part.sum(axis=1, keepdims=True)
            out.append(np.divide(part, den, out=np.zeros_like(part), where=den > 0))
        return out

    def mode(self) -> list[MotifIndex]:
        """Each sequence's most frequent pooled bin, the first one among equals (the
        .fsx's countBy |> sortByDescending |> head, per site), as a MotifIndex whose PWMS
        field carries that bin's pooled frequency."""
        out = []
        for m in self.marginals(pool=True):
            k = int(np.argmax(m))  # the first maximum
            out.append(createMotifIndex(m[k], [] if k == 0 else [k - 1]))
        return out

    def agreement(self, pooled=None) -> ChainAgreement:
        """The chains against their pool, from the bins, in integers: what
        Context.occupancy_agreement and MotifSampler.runSweepsBatchedAgreement compute on the
        device without the bins coming down.  pooled[R] (non-zero = pooled) replaces
        finished() as the choice of the pool."""
        occ = np.asarray(self.occupancy, np.int64)
        off = np.asarray(self.offsets, np.int64)
        R, N = len(occ), max(len(off) - 1, 0)
        keep = self.finished() if pooled is None else np.asarray(pooled) != 0
        idx = np.nonzero(keep)[0]
        P = len(idx)
        agree = np.zeros(N, np.int32)
        spread = np.zeros(N, np.int64)
        spread_chain = np.full(N, -1, np.int32)
        chain_agree = np.where(keep, 0, -1).astype(np.int32)
        chain_dist = np.where(keep, 0, -1).astype(np.int64)
        if P > 0 and N > 0:
            start, lens = off[:-1], np.diff(off)
            rows = occ[idx]                               # [P, H]
            pool = rows.sum(axis=0)
            d = np.add.reduceat(np.abs(P * rows - pool), start, axis=1)  # D[P, N]
            where = np.arange(off[-1], dtype=np.int64)

            def first_max(x):  # the first-maximum bin of every row of x[..., H], per sequence
                top = np.repeat(np.maximum.reduceat(x, start, axis=-1), lens, axis=-1)
                return np.minimum.reduceat(np.where(x == top, where, off[-1]), start, axis=-1)

            same = first_max(rows) == first_max(pool)     # [P, N]
            agree[:] = same.sum(axis=0)
            spread[:] = d.max(axis=0)
            spread_chain[:] = idx[d.argmax(axis=0)]       # the first maximum: the lowest chain
            chain_dist[idx] = d.sum(axis=1)
            chain_agree[idx] = same.sum(axis=1)
        return ChainAgreement(agree, spread, spread_chain, chain_agree, chain_dist, P,
                              int(self.ic.shape[1]))

    def rhat(self) -> float:
        """The Gelman-Rubin potential scale reduction of the ic trace over the finished
        chains, in binary64 on the host: m chains of n entries, B / n the variance of the chain
        means and Wv the mean of the chains' variances (ddof 1), sqrt(((n - 1) / n Wv + B / n)
        / Wv).  NaN when m < 2, n < 2, Wv == 0 or a finished chain's trace holds a NaN."""
        return _rhat(self.ic, self.finished())


@dataclass
class ChainSummary:
    """What MotifSampler.runSweepsSummary / runSweepsBatchedSummary reduced on the device from
    the occupancy of R chains (the single chain: R = 1), without the bins coming down.
    mode_pos[R, N] / mode_count[R, N]: each chain's most frequent bin of every sequence minus
    one (-1 = Positions []), the first among equals, and its count.  counts[R, A W + A]: each
    chain's count matrix summed over its counted states (C[a W + j], then T[a], as
    Context.counts).  pooled_pos[N], pooled_count[N], pooled_counts[A W + A]: the same over
    the sum of the n_pooled finished chains' bins.  n_counted: the counted sweeps of a chain.
    ic, best_sweep, best: as ChainStats.  occupancy / offsets: the bins, only when asked
    for."""
    mode_pos: np.ndarray
    mode_count: np.ndarray
    counts: np.ndarray
    pooled_pos: np.ndarray
    pooled_count: np.ndarray
    pooled_counts: np.ndarray
    n_pooled: int
    n_counted: int
    ic: np.ndarray
    best_sweep: np.ndarray
    best: list
    motifLength: int
    alphabetSize: int
    occupancy: np.ndarray | None = None
    offsets: np.ndarray | None = None
    #: the chains against their pool, only from MotifSampler.runSweepsBatchedAgreement
    agreement: ChainAgreement | None = None

    def rhat(self) -> float:
        """ChainStats.rhat() of the ic trace: over the chains the agreement pooled, or, without
        an agreement, over every chain (a chain that raised leaves NaN in its trace, and the
        result is then NaN)."""
        keep = (np.asarray(self.agreement.chain_dist) >= 0 if self.agreement is not None
                else np.ones(len(self.ic), bool))
        return _rhat(self.ic, keep)

    def mode(self) -> list[MotifIndex]:
        """ChainStats.mode() of the same chains: each sequence's most frequent pooled bin, the
        first among equals, its PWMS field the pooled frequency pooled_count / (n_pooled
        n_counted), or 0 without a pooled counted state."""
        den = float(int(self.n_pooled) * int(self.n_counted))
        out = []
        for p, k in zip(np.asarray(self.pooled_pos), np.asarray(self.pooled_count)):
            f = float(np.float64(k) / den) if den > 0 else 0.0
            out.append(createMotifIndex(f, [] if p < 0 else [int(p)]))
        return out

    def countMatrix(self, pool: bool = True):
        """(C[A, W], T[A]) summed over the counted states of the pooled chains, or with
        pool=False chain by chain: (C[R, A, W], T[R, A])."""
        A, W = int(self.alphabetSize), int(self.motifLength)
        if pool:
            x = np.asarray(self.pooled_counts)
            return x[:A * W].reshape(A, W), x[A * W:A * W + A]
        x = np.asarray(self.counts)
        return x[:, :A * W].reshape(-1, A, W), x[:, A * W:A * W + A]


@dataclass
class ListChainStats(ChainStats):
    """What MotifSampler.runSweepsBatchedListStats gathered over the counted sweeps of R
    chains of Positions lists: ChainStats, where bin offsets[n] counts the counted sweeps
    whose list of sequence n is empty and bin offsets[n] + 1 + k those whose list contains
    start k, and best[r] holds lists; sites[R, N, M + 1]: the counted sweeps whose list of
    sequence n has 0 .. M positions.  motifLength is the W the chains ran with."""
    sites: np.ndarray
    motifLength: int

    def finished(self) -> np.ndarray:
        """[R] bool: the chains every counted sweep of which was counted: every sequence's
        site counts sum to the number of counted sweeps (a chain that raised stops counting
        in that sweep)."""
        return (self.sites.sum(axis=2) == self.ic.shape[1]).all(axis=1)

    def marginals(self, pool: bool = True) -> list:
        """Per sequence its bins divided by the counted sweeps: pooled over the finished
        chains (one array of 1 + L_n - W + 1 frequencies a sequence), or with pool=False
        chain by chain ([R, bins] a sequence, each chain over the sweeps it counted).  A list
        holds up to M starts, so bins 1.. sum to the mean number of sites of the sequence,
        not to 1 minus the empty share.  Without any counted state the frequencies are 0."""
        occ = np.asarray(self.occupancy, np.float64)
        off = self.offsets
        if pool:
            return ChainStats.marginals(self, pool=True)
        den = self.sites.sum(axis=2).astype(np.float64)  # [R, N]: the sweeps a chain counted
        out = []
        for n in range(len(off) - 1):
            part, d = occ[:, off[n]:off[n + 1]], den[:, n:n + 1]
            out.append(np.divide(part, d, out=np.zeros_like(part), where=d > 0))
        return out

    def siteCounts(self, pool: bool = True) -> list:
        """Per sequence the frequencies of 0 .. M sites over the counted sweeps: pooled over
        the finished chains (one array of M + 1 a sequence), or with pool=False chain by
        chain ([R, M + 1] a sequence, each chain over the sweeps it counted)."""
        sites = np.asarray(self.sites, np.float64)
        if pool:
            keep = self.finished()
            total = sites[keep].sum(axis=0)
            den = float(keep.sum() * self.ic.shape[1])
            total = total / den if den > 0 else np.zeros_like(total)
            return [total[n] for n in range(sites.shape[1])]
        den = sites.sum(axis=2, keepdims=True)
        freq = np.divide(sites, den, out=np.zeros_like(sites), where=den > 0)
        return [freq[:, n] for n in range(sites.shape[1])]

    def mode(self) -> list[MotifIndex]:
        """Per sequence a MotifIndex list: the most frequent pooled site count c (the first
        maximum), then the c most occupied pooled starts that are pairwise more than
        motifLength apart (.fs:129-140), chosen greedily by descending frequency, the first
        among equals; fewer when no further start is far enough from those taken.  Positions
        are in ascending order; the PWMS field carries the pooled frequency of c sites."""
        out = []
        for m, s in zip(self.marginals(pool=True), self.siteCounts(pool=True)):
            c = int(np.argmax(s))  # the first maximum
            taken: list[int] = []
            for k in np.argsort(-m[1:], kind="stable"):
                if len(taken) == c:
                    break
                if all(abs(int(k) - q) > self.motifLength for q in taken):
                    taken.append(int(k))
            out.append(createMotifIndex(s[c], sorted(taken)))
        return out


@dataclass
class ListChainSummary:
    """What MotifSampler.runSweepsBatchedListSummary reduced on the device from the bins and site
    counts of R chains of Positions lists, without either coming down.
    mode_sites[R, N] / mode_sites_count[R, N]: each chain's most frequent number of sites of
    every sequence, the first among equals, and how often.  mode_cnt[R, N], mode_pos[R, N, M],
    mode_count[R, N, M]: that many most occupied starts pairwise more than motifLength apart,
    taken greedily (the first among equals), in ascending order, with their bins; -1 / 0 past
    mode_cnt.  counts[R, A W + A]: each chain's count matrix summed over its counted states
    (C[a W + j], then T[a], as Context.counts).  pooled_*: the same over the sums of the
    n_pooled finished chains' bins and site counts.  n_counted: the counted sweeps of a chain.
    ic, best_sweep, best: as ListChainStats.  occupancy / offsets / sites: the bins and site
    counts, only when asked for."""
    mode_sites: np.ndarray
    mode_sites_count: np.ndarray
    mode_cnt: np.ndarray
    mode_pos: np.ndarray
    mode_count: np.ndarray
    counts: np.ndarray
    pooled_sites: np.ndarray
    pooled_sites_count: np.ndarray
    pooled_cnt: np.ndarray
    pooled_pos: np.ndarray
    pooled_count: np.ndarray
    pooled_counts: np.ndarray
    n_pooled: int
    n_counted: int
    ic: np.ndarray
    best_sweep: np.ndarray
    best: list
    motifLength: int
    alphabetSize: int
    occupancy: np.ndarray | None = None
    offsets: np.ndarray | None = None
    sites: np.ndarray | None = None

    def mode(self) -> list[MotifIndex]:
        """ListChainStats.mode() of the same chains: per sequence the pooled list, its PWMS
        field the pooled frequency of its number of sites, pooled_sites_count / (n_pooled
        n_counted), or 0 without a pooled counted state."""
        den = float(int(self.n_pooled) * int(self.n_counted))
        out = []
        for k, c, p in zip(np.asarray(self.pooled_sites_count), np.asarray(self.pooled_cnt),
                           np.asarray(self.pooled_pos)):
            f = float(np.float64(k) / den) if den > 0 else 0.0
            out.append(createMotifIndex(f, [int(q) for q in p[:int(c)]]))
        return out

    def countMatrix(self, pool: bool = True):
        """(C[A, W], T[A]) summed over the counted states of the pooled chains, or with
        pool=False chain by chain: (C[R, A, W], T[R, A])."""
        A, W = int(self.alphabetSize), int(self.motifLength)
        if pool:
            x = np.asarray(self.pooled_counts)
            return x[:A * W].reshape(A, W), x[A * W:A * W + A]
        x = np.asarray(self.counts)
        return x[:, :A * W].reshape(-1, A, W), x[:, A * W:A * W + A]


class MotifSampler:
    """MotifSampler module (.fs:709-1038): the hot-path entry points."""

    @staticmethod
    def findBestMotifIndicesByWithStartPositions(motifAmount: int, motifLength: int,
                                                 pseudoCount: float, cutOff: float, alphabet,
                                                 sources, motifMem: Sequence[MotifIndex],
                                                 rnd=None, device: int = 0) -> list[MotifIndex]:
        """One synchronous stochastic sweep (.fs:935-970).  motifAmount = 1 with single
        positions runs the ★ sweep kernel; otherwise the Positions-list path."""
        if len(motifMem) != len(sources):
            raise _native.ArgumentError(_native.GS_E_ARG, "motifMem and sources differ in length")
        ctx = _bind(alphabet, sources, device)
        u = _uniforms(rnd, len(sources))
        if _is_single(motifAmount, motifMem):
            pos_out, pwms = ctx.motif_sweep(motifLength, pseudoCount, cutOff,
                                            _single_positions(motifMem), u)
            return _motif_indices(pos_out, pwms)
        cap, cnt, pos = _lists(motifAmount, motifMem)
        co, po, pw = ctx.motif_sweep_multi(motifAmount, motifLength, pseudoCount, cutOff, cnt,
                                           pos, u, cap)
        return _motif_lists(co, po, pw)

    @staticmethod
    def runSweeps(motifLength: int, pseudoCount: float, cutOff: float, alphabet, sources,
                  motifMem: Sequence[MotifIndex], sweeps: int, seed: int, first_sweep: int = 0,
                  device: int = 0, motifAmount: int = 1) -> list[MotifIndex]:
        """`sweeps` chained sweeps on the device (uniforms from the counter RNG).  With
        motifAmount >= 2, or a MotifIndex of more than one position, the chain runs on the
        Positions-list path (Context.motif_run_multi)."""
        ctx = _bind(alphabet, sources, device)
        if _is_single(motifAmount, motifMem):
            pos, pwms = ctx.motif_run(motifLength, pseudoCount, cutOff, sweeps, seed,
                                      _single_positions(motifMem), first_sweep)
            return _motif_indices(pos, pwms)
        cap, cnt, pos = _lists(motifAmount, motifMem)
        co, po, pw = ctx.motif_run_multi(motifAmount, motifLength, pseudoCount, cutOff, sweeps,
                                         seed, cnt, pos, first_sweep, cap)
        return _motif_lists(co, po, pw)

    @staticmethod
    def runSweepsStats(motifLength: int, pseudoCount: float, cutOff: float, alphabet, sources,
                       motifMem: Sequence[MotifIndex], sweeps: int, burn_in: int = 0,
                       thin: int = 1, seed: int = 0, first_sweep: int = 0, device: int = 0):
        """runSweeps (motifAmount 1, single positions) with the statistics a chain is run
        for, gathered on the device behind its sweeps in the same single call
        (Context.motif_run_stats) -> (chain, ChainStats with R = 1): the occupancy of every
        motif start over the counted sweeps (t >= burn_in, every thin-th), the trace of
        informationContent, and the best state visited.  The single chain runs on the fast
        sweep kernels: the way to a posterior from about 2 000 sequences on, where the chain
        batch (runSweepsBatchedStats) no longer pays.  A chain that raises
        raises here."""
        start = _single_start(motifMem, sources)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, st = ctx.motif_run_stats(motifLength, pseudoCount, cutOff, sweeps,
                                            int(seed) & (2**64 - 1), start, first_sweep,
                                            burn_in=burn_in, thin=thin)
        best = _best_states(st, single_chain=True)
        stats = ChainStats(st["occupancy"][None, :], st.get("offsets", np.zeros(1, np.int64)),
                           st["ic"][None, :], st["best_sweep"], best)
        return _motif_indices(pos, pwms), stats

    @staticmethod
    def runSweepsSummary(motifLength: int, pseudoCount: float, cutOff: float, alphabet, sources,
                         motifMem: Sequence[MotifIndex], sweeps: int, burn_in: int = 0,
                         thin: int = 1, seed: int = 0, first_sweep: int = 0, device: int = 0,
                         occupancy: bool = False):
        """runSweepsStats with the bins reduced on the device (Context.motif_run_summary) ->
        (chain, ChainSummary with R = 1): where the motif is in each sequence and how often,
        and the count matrix over the counted states, without the histogram coming down
        (DESIGN.md §9.28).  occupancy=True also returns the bins.  A chain that raises raises
        here."""
        start = _single_start(motifMem, sources)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, st = ctx.motif_run_summary(motifLength, pseudoCount, cutOff, sweeps,
                                              int(seed) & (2**64 - 1), start, first_sweep,
                                              burn_in=burn_in, thin=thin, occupancy=occupancy)
        best = _best_states(st, single_chain=True)
        n_counted = st["ic"].shape[0]
        # the single chain finished (a raise raised above): it is the pool
        summary = ChainSummary(st["mode_pos"][None, :], st["mode_count"][None, :],
                               st["counts"][None, :], st["mode_pos"],
                               st["mode_count"].astype(np.int64), st["counts"], 1, n_counted,
                               st["ic"][None, :], st["best_sweep"], best, int(motifLength),
                               len(alphabet_codes(alphabet)),
                               st["occupancy"][None, :] if occupancy else None,
                               st.get("offsets") if occupancy else None)
        return _motif_indices(pos, pwms), summary

    @staticmethod
    def runSweepsBatchedSummary(motifLength: int, pseudoCount: float, cutOff: float, alphabet,
                                sources, sweeps: int, seeds, motifMems=None, init_mode: int = 0,
                                first_sweep: int = 0, burn_in: int = 0, thin: int = 1,
                                device: int = 0, motifAmount: int = 1, occupancy: bool = False):
        """runSweepsBatchedStats with the bins reduced on the device
        (Context.motif_run_batch_summary) -> (chains, ChainSummary): every chain's modes and
        count matrix and those pooled over the finished chains.  occupancy=True also returns
        the bins.  motifAmount 1 with single positions only."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        if motifAmount != 1:
            raise _native.ArgumentError(_native.GS_E_ARG,
                                        "the chain statistics need motifAmount = 1")
        pos = _chain_starts(motifMems, seeds, sources, single=True)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, status, st = ctx.motif_run_batch_summary(
            motifLength, pseudoCount, cutOff, sweeps, seeds, pos, init_mode, first_sweep,
            burn_in=burn_in, thin=thin, occupancy=occupancy)
        _raise_failed_chain(status)
        R = len(seeds)
        best = _best_states(st)
        summary = ChainSummary(st["mode_pos"], st["mode_count"], st["counts"], st["pooled_pos"],
                               st["pooled_count"], st["pooled_counts"], int(st["n_pooled"][0]),
                               st["ic"].shape[1], st["ic"], st["best_sweep"], best,
                               int(motifLength), len(alphabet_codes(alphabet)),
                               st["occupancy"] if occupancy else None,
                               st.get("offsets") if occupancy else None)
        return [_motif_indices(pos[r], pwms[r]) for r in range(R)], summary

    @staticmethod
    def runSweepsBatchedAgreement(motifLength: int, pseudoCount: float, cutOff: float, alphabet,
                                  sources, sweeps: int, seeds, motifMems=None,
                                  init_mode: int = 0, first_sweep: int = 0, burn_in: int = 0,
                                  thin: int = 1, device: int = 0, motifAmount: int = 1):
        """runSweepsBatchedSummary with the chains' agreement with their pool reduced on the
        device in the same single call (Context.motif_run_batch_agreement, which is asked for
        no bins) -> (chains, ChainSummary with its agreement field set): how many chains share
        the pooled mode of each sequence, how far the farthest chain's marginal is from the
        pooled one, and every chain's distance summed over the sequences.
        motifAmount 1 with single positions only."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        if motifAmount != 1:
            raise _native.ArgumentError(_native.GS_E_ARG,
                                        "the chain statistics need motifAmount = 1")
        pos = _chain_starts(motifMems, seeds, sources, single=True)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, status, st = ctx.motif_run_batch_agreement(
            motifLength, pseudoCount, cutOff, sweeps, seeds, pos, init_mode, first_sweep,
            burn_in=burn_in, thin=thin, occupancy=False)
        _raise_failed_chain(status)
        R = len(seeds)
        n_counted = st["ic"].shape[1]
        agreement = ChainAgreement(st["agree"], st["spread"], st["spread_chain"],
                                   st["chain_agree"], st["chain_dist"],
                                   int(st["agree_n_pooled"][0]), n_counted)
        summary = ChainSummary(st["mode_pos"], st["mode_count"], st["counts"], st["pooled_pos"],
                               st["pooled_count"], st["pooled_counts"], int(st["n_pooled"][0]),
                               n_counted, st["ic"], st["best_sweep"], _best_states(st),
                               int(motifLength), len(alphabet_codes(alphabet)),
                               agreement=agreement)
        return [_motif_indices(pos[r], pwms[r]) for r in range(R)], summary

    @staticmethod
    def runSweepsBatched(motifLength: int, pseudoCount: float, cutOff: float, alphabet, sources,
                         sweeps: int, seeds, motifMems=None, init_mode: int = 0,
                         first_sweep: int = 0, device: int = 0,
                         motifAmount: int = 1) -> list[list[MotifIndex]]:
        """One independent chain of `sweeps` chained sweeps per seed, all in one
        Context.motif_run_batch call: entry r is runSweeps(..., motifMems[r], sweeps,
        seeds[r], first_sweep).  Without motifMems chain r starts from getPWMOfRandomStarts
        of seeds[r] (init_mode as in doMotifSampling).  A chain that raised raises here.
        Faster than the loop up to about 2 000 sequences a chain, slower beyond
        (DESIGN.md §9.13).  With motifAmount >= 2, or a MotifIndex of more than one
        position, the chains run on the Positions-list path in one
        Context.motif_run_multi_batch call: faster than the loop at every shape measured,
        5 to 2 000 sequences a chain; not measured beyond."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        _chain_starts(motifMems, seeds, sources)
        if not all(_is_single(motifAmount, m) for m in motifMems or [[]]):
            return _run_lists_batched(motifAmount, motifLength, pseudoCount, cutOff, alphabet,
                                      sources, sweeps, seeds, motifMems, init_mode, first_sweep,
                                      device)
        pos = _chain_starts(motifMems, seeds, sources, single=True)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, status = ctx.motif_run_batch(motifLength, pseudoCount, cutOff, sweeps, seeds,
                                                pos, init_mode, first_sweep)
        _raise_failed_chain(status)
        return [_motif_indices(pos[r], pwms[r]) for r in range(len(seeds))]

    @staticmethod
    def runSweepsBatchedStats(motifLength: int, pseudoCount: float, cutOff: float, alphabet,
                              sources, sweeps: int, seeds, motifMems=None, init_mode: int = 0,
                              first_sweep: int = 0, burn_in: int = 0, thin: int = 1,
                              device: int = 0, motifAmount: int = 1):
        """runSweepsBatched with the statistics a chain is run for, gathered on the device
        in the same single call (Context.motif_run_batch_stats) -> (chains, ChainStats):
        the occupancy of every motif start over the counted sweeps (t >= burn_in, every
        thin-th), the trace of informationContent, and the best state each chain visited.
        motifAmount 1 with single positions only."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        if motifAmount != 1:
            raise _native.ArgumentError(_native.GS_E_ARG,
                                        "the chain statistics need motifAmount = 1")
        pos = _chain_starts(motifMems, seeds, sources, single=True)
        ctx = _bind(alphabet, sources, device)
        pos, pwms, status, st = ctx.motif_run_batch_stats(
            motifLength, pseudoCount, cutOff, sweeps, seeds, pos, init_mode, first_sweep,
            burn_in=burn_in, thin=thin)
        _raise_failed_chain(status)
        R = len(seeds)
        best = _best_states(st)
        stats = ChainStats(st["occupancy"], st.get("offsets", np.zeros(1, np.int64)), st["ic"],
                           st["best_sweep"], best)
        return [_motif_indices(pos[r], pwms[r]) for r in range(R)], stats

    @staticmethod
    def runSweepsBatchedListStats(motifLength: int, pseudoCount: float, cutOff: float, alphabet,
                                  sources, sweeps: int, seeds, motifMems=None, init_mode: int = 0,
                                  first_sweep: int = 0, burn_in: int = 0, thin: int = 1,
                                  device: int = 0, motifAmount: int = 1):
        """runSweepsBatchedStats for chains of Positions lists (any motifAmount), in one
        Context.motif_run_multi_batch_stats call -> (chains, ListChainStats): the occupancy
        of every motif start and the number of sites of every sequence over the counted
        sweeps (t >= burn_in, every thin-th), the trace of informationContent, and the best
        state each chain visited."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        _chain_starts(motifMems, seeds, sources)
        cap, cnt, pos = _chain_lists(motifAmount, motifMems, len(sources))
        ctx = _bind(alphabet, sources, device)
        cnt, pos, pwms, status, st = ctx.motif_run_multi_batch_stats(
            motifAmount, motifLength, pseudoCount, cutOff, sweeps, seeds, cnt, pos, init_mode,
            first_sweep, cap, burn_in=burn_in, thin=thin)
        _raise_failed_chain(status)
        R = len(seeds)
        best = _best_states(st)
        stats = ListChainStats(st["occupancy"], st.get("offsets", np.zeros(1, np.int64)),
                               st["ic"], st["best_sweep"], best, st["sites"], int(motifLength))
        return [_motif_lists(cnt[r], pos[r], pwms[r]) for r in range(R)], stats

    @staticmethod
    def runSweepsBatchedListSummary(motifLength: int, pseudoCount: float, cutOff: float, alphabet,
                                    sources, sweeps: int, seeds, motifMems=None,
                                    init_mode: int = 0, first_sweep: int = 0, burn_in: int = 0,
                                    thin: int = 1, device: int = 0, motifAmount: int = 1,
                                    occupancy: bool = False):
        """runSweepsBatchedListStats with the bins and site counts reduced on the device
        (Context.motif_run_multi_batch_summary) -> (chains, ListChainSummary): every chain's
        modal lists and count matrix and those pooled over the finished chains, what
        ListChainStats.mode() and a count matrix over the counted states give, without the
        slabs coming down.  occupancy=True also returns the bins and the
        site counts."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        _chain_starts(motifMems, seeds, sources)
        cap, cnt, pos = _chain_lists(motifAmount, motifMems, len(sources))
        ctx = _bind(alphabet, sources, device)
        cnt, pos, pwms, status, st = ctx.motif_run_multi_batch_summary(
            motifAmount, motifLength, pseudoCount, cutOff, sweeps, seeds, cnt, pos, init_mode,
            first_sweep, cap, burn_in=burn_in, thin=thin, occupancy=occupancy, sites=occupancy)
        _raise_failed_chain(status)
        R = len(seeds)
        best = _best_states(st)
        summary = ListChainSummary(
            st["mode_sites"], st["mode_sites_count"], st["mode_cnt"], st["mode_pos"],
            st["mode_count"], st["counts"], st["pooled_sites"], st["pooled_sites_count"],
            st["pooled_cnt"], st["pooled_pos"], st["pooled_count"], st["pooled_counts"],
            int(st["n_pooled"][0]), st["ic"].shape[1], st["ic"], st["best_sweep"], best,
            int(motifLength), len(alphabet_codes(alphabet)),
            st["occupancy"] if occupancy else None, st.get("offsets") if occupancy else None,
            st["sites"] if occupancy else None)
        return [_motif_lists(cnt[r], pos[r], pwms[r]) for r in range(R)], summary

    @staticmethod
    def findBestMotifIndicesWithStartPositions(motifAmount: int, motifLength: int,
                                               pseudoCount: float, cutOff: float, alphabet,
                                               sources, motifMem: Sequence[MotifIndex],
                                               max_passes: int = UNBOUNDED,
                                               device: int = 0) -> list[MotifIndex]:
        """Greedy passes until no position moves (.fs:885-929)."""
        if len(motifMem) != len(sources):
            raise _native.ArgumentError(_native.GS_E_ARG, "motifMem and sources differ in length")
        ctx = _bind(alphabet, sources, device)
        pwms = np.array([m.PWMS for m in motifMem], np.float64)
        if _is_single(motifAmount, motifMem):
            pos, pwms, np_ = ctx.motif_greedy(motifLength, pseudoCount, cutOff,
                                              _single_positions(motifMem), pwms, max_passes)
            _passes(np_, max_passes)
            return _motif_indices(pos, pwms)
        cap, cnt, pos = _lists(motifAmount, motifMem)
        co, po, pw, np_ = ctx.motif_greedy_multi(motifAmount, motifLength, pseudoCount, cutOff,
                                                 cnt, pos, pwms, max_passes, cap)
        _passes(np_, max_passes)
        return _motif_lists(co, po, pw)

    @staticmethod
    def doMotifSampling(motifAmount: int, motifLength: int, pseudoCount: float, cutOff: float,
                        alphabet, sources, seed: int | None = None, init_mode: int = 0,
                        device: int = 0) -> list[MotifIndex]:
        """getPWMOfRandomStarts |> one sweep |> greedy passes (.fs:1034-1038), on the
        device.  seed None draws a fresh one (the reference's time-seeded Randoms)."""
        ctx = _bind(alphabet, sources, device)
        return _sampling(ctx, motifAmount, motifLength, pseudoCount, cutOff, _seed(seed),
                         init_mode)

    @staticmethod
    def getMotifsWithBestInformationContents(numberOfRepetitions: int, motifAmount: int,
                                             motifLength: int, pseudoCount: float,
                                             cutOff: float, alphabet, sources,
                                             seed: int | None = None, init_mode: int = 0,
                                             device: int = 0,
                                             batch: bool = False) -> list[MotifIndex]:
        """Repeated doMotifSampling keeping the run of largest Σ PWMS (.fs:973-998);
        run r uses seed + r.  batch=True (motifAmount = 1) computes every run
        r = 0 … numberOfRepetitions in one Context.motif_sampling_batch call, the runs'
        greedy passes side by side on the GPU, and replays the same loop over them:
        the same result, all runs paid for even when the loop stops early.  With Positions
        lists (motifAmount >= 2) that is getMotifsWithBestInformationContentsBatched."""
        base = _seed(seed)
        if batch:
            if motifAmount != 1:
                raise _native.ArgumentError(
                    _native.GS_E_ARG, "batch=True runs the single-position chains only "
                    "(motifAmount = 1)")
            ctx = _bind(alphabet, sources, device)
            return _replay_repetitions(
                numberOfRepetitions,
                _batched_runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength,
                              pseudoCount, cutOff, base, init_mode),
                lambda xs: sum(x.PWMS for x in xs), [createMotifIndex(0.0, [])])
        return _best_of_repetitions(
            numberOfRepetitions,
            lambda r: MotifSampler.doMotifSampling(motifAmount, motifLength, pseudoCount,
                                                   cutOff, alphabet, sources, base + r,
                                                   init_mode, device),
            lambda xs: sum(x.PWMS for x in xs), [createMotifIndex(0.0, [])])

    @staticmethod
    def getMotifsWithBestInformationContentsBatched(numberOfRepetitions: int, motifAmount: int,
                                                    motifLength: int, pseudoCount: float,
                                                    cutOff: float, alphabet, sources,
                                                    seed: int | None = None, init_mode: int = 0,
                                                    device: int = 0) -> list[MotifIndex]:
        """getMotifsWithBestInformationContents with every run r = 0 … numberOfRepetitions
        computed by one call, for any motifAmount: Context.motif_sampling_batch for
        motifAmount = 1, Context.motif_sampling_multi_batch (Positions lists) above, then
        the loop of .fs:973-998 replayed over the runs: the result of the loop, all runs
        paid for even when it stops early."""
        if not 1 <= motifAmount <= 16:
            raise _native.ArgumentError(_native.GS_E_ARG, "motifAmount must be in [1, 16]")
        ctx = _bind(alphabet, sources, device)
        runs = _batched_runs if motifAmount == 1 else \
            functools.partial(_batched_list_runs, motifAmount=motifAmount)
        return _replay_repetitions(
            numberOfRepetitions,
            runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength, pseudoCount, cutOff,
                 _seed(seed), init_mode),
            lambda xs: sum(x.PWMS for x in xs), [createMotifIndex(0.0, [])])

    # ---- the caller's background (…ByPCV, .fs:788-881) and profile (…OfPPM) twins
    @staticmethod
    def findBestMotifPositionsWithStartPositionsByPCV(motifAmount: int, motifLength: int,
                                                      pseudoCount: float, cutOff: float,
                                                      alphabet, sources, pcv,
                                                      motifMem: Sequence[MotifIndex], rnd=None,
                                                      device: int = 0) -> list[MotifIndex]:
        """One stochastic sweep with the caller's pcv (.fs:828-853)."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, pcv=pcv):
            return MotifSampler.findBestMotifIndicesByWithStartPositions(
                motifAmount, motifLength, pseudoCount, cutOff, alphabet, sources, motifMem, rnd,
                device)

    @staticmethod
    def findBestMotifPositionsWithStartPositionByPCV(motifAmount: int, motifLength: int,
                                                     pseudoCount: float, cutOff: float,
                                                     alphabet, sources, pcv,
                                                     motifMem: Sequence[MotifIndex],
                                                     max_passes: int = UNBOUNDED,
                                                     device: int = 0) -> list[MotifIndex]:
        """The greedy passes with the caller's pcv (.fs:788-823)."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, pcv=pcv):
            return MotifSampler.findBestMotifIndicesWithStartPositions(
                motifAmount, motifLength, pseudoCount, cutOff, alphabet, sources, motifMem,
                max_passes, device)

    @staticmethod
    def findBestInormationContentContainingMotifsWithPCV(numberOfRepetitions: int,
                                                          motifAmount: int, motifLength: int,
                                                          pseudoCount: float, cutOff: float,
                                                          alphabet, sources, pcv,
                                                          seed: int | None = None,
                                                          device: int = 0,
                                                          batch: bool = False) -> list[MotifIndex]:
        """Repetitions of getPWMOfRandomStartsWithBPV |> ByPCV sweep |> ByPCV greedy
        (.fs:856-881); run r uses seed + r.  batch=True computes every run
        r = 0 … numberOfRepetitions in one Context.motif_sampling_batch(pcv=) call
        (motif_sampling_multi_batch for motifAmount >= 2) and replays the same loop over
        them: the same result, all runs paid for even when the loop stops early."""
        base = _seed(seed)
        if batch:
            return _batched_motif_twin(numberOfRepetitions, motifAmount, motifLength, pseudoCount,
                                       cutOff, alphabet, sources, base, device, pcv=pcv)
        ctx = _bind(alphabet, sources, device)

        def run(r):
            with _fixed(ctx, pcv=pcv):
                return _sampling(ctx, motifAmount, motifLength, pseudoCount, cutOff, base + r, 0)
        return _best_of_repetitions(numberOfRepetitions, run, lambda xs: sum(x.PWMS for x in xs),
                                    [createMotifIndex(0.0, [])])

    @staticmethod
    def doMotifSamplingWithPPM(motifAmount: int, motifLength: int, pseudoCount: float,
                               cutOff: float, alphabet, sources, positionProbabilityMatrix,
                               seed: int | None = None, device: int = 0) -> list[MotifIndex]:
        """getMotifsWithBestPWMSOfPPM |> sweep |> greedy passes (.fs:1028-1032)."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, ppm=positionProbabilityMatrix, W=motifLength):
            return _sampling(ctx, motifAmount, motifLength, pseudoCount, cutOff, _seed(seed), 0)

    @staticmethod
    def getBestPWMSsOfPPM(numberOfRepetitions: int, motifAmount: int, motifLength: int,
                          pseudoCount: float, cutOff: float, alphabet, sources,
                          positionProbabilityMatrix, seed: int | None = None,
                          device: int = 0, batch: bool = False) -> list[MotifIndex]:
        """Repetitions of doMotifSamplingWithPPM (.fs:1001-1026); run r uses seed + r.
        batch=True computes every run r = 0 … numberOfRepetitions in one
        Context.motif_sampling_batch(ppm=) call (motif_sampling_multi_batch for
        motifAmount >= 2) and replays the same loop over them: the same result, all runs
        paid for even when the loop stops early."""
        base = _seed(seed)
        if batch:
            return _batched_motif_twin(numberOfRepetitions, motifAmount, motifLength, pseudoCount,
                                       cutOff, alphabet, sources, base, device,
                                       ppm=positionProbabilityMatrix)
        return _best_of_repetitions(
            numberOfRepetitions,
            lambda r: MotifSampler.doMotifSamplingWithPPM(
                motifAmount, motifLength, pseudoCount, cutOff, alphabet, sources,
                positionProbabilityMatrix, base + r, device),
            lambda xs: sum(x.PWMS for x in xs), [createMotifIndex(0.0, [])])


def _batched_motif_twin(numberOfRepetitions, motifAmount, motifLength, pseudoCount, cutOff,
                        alphabet, sources, base, device, pcv=None, ppm=None):
    """The repetition loop of a ByPCV / OfPPM driver over runs 0 … numberOfRepetitions
    computed by one batch call: Context.motif_sampling_batch for motifAmount = 1,
    Context.motif_sampling_multi_batch (Positions lists) above."""
    if not 1 <= motifAmount <= 16:
        raise _native.ArgumentError(_native.GS_E_ARG, "motifAmount must be in [1, 16]")
    ctx = _bind(alphabet, sources, device)
    runs = _batched_runs if motifAmount == 1 else \
        functools.partial(_batched_list_runs, motifAmount=motifAmount)
    return _replay_repetitions(
        numberOfRepetitions,
        runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength, pseudoCount, cutOff, base, 0,
             pcv=pcv, ppm=ppm),
        lambda xs: sum(x.PWMS for x in xs), [createMotifIndex(0.0, [])])


class _fixed:
    """Sets the caller's pcv / ppm on a context for the duration of one call."""

    def __init__(self, ctx, pcv=None, ppm=None, W=None):
        self.ctx, self.pcv, self.ppm, self.W = ctx, pcv, ppm, W

    def __enter__(self):
        if self.pcv is not None:
            self.ctx.set_fixed_pcv(np.asarray(self.pcv, np.float64))
        if self.ppm is not None:
            self.ctx.set_fixed_ppm(np.asarray(self.ppm, np.float64), self.W)
        return self.ctx

    def __exit__(self, *exc):
        if self.pcv is not None:
            self.ctx.set_fixed_pcv(None)
        if self.ppm is not None:
            self.ctx.set_fixed_ppm(None)
        return False


def _is_single(motifAmount: int, motifMem: Sequence[MotifIndex]) -> bool:
    """motifAmount = 1 and no list longer than one: the ★ kernels' snapshot form."""
    return motifAmount == 1 and all(len(m.Positions) <= 1 for m in motifMem)


def _lists(motifAmount: int, motifMem: Sequence[MotifIndex]):
    """MotifIndex[] -> (cap, cnt[N], pos[N, cap]) in F# list order."""
    if not 1 <= motifAmount <= 16:
        raise _native.ArgumentError(_native.GS_E_ARG, "motifAmount must be in [1, 16]")
    cap = max([motifAmount] + [len(m.Positions) for m in motifMem])
    cnt = np.array([len(m.Positions) for m in motifMem], np.int32)
    pos = np.full((len(motifMem), cap), -1, np.int32)
    for i, m in enumerate(motifMem):
        pos[i, :len(m.Positions)] = m.Positions
    return cap, cnt, pos


def _sampling(ctx, motifAmount, motifLength, pseudoCount, cutOff, seed, init_mode):
    """doMotifSampling on the device: the ★ kernels for motifAmount = 1, else the
    Positions-list path."""
    if motifAmount == 1:
        pos, pwms, _ = ctx.motif_sampling(motifLength, pseudoCount, cutOff, seed, init_mode,
                                          UNBOUNDED)
        return _motif_indices(pos, pwms)
    co, po, pw, _ = ctx.motif_sampling_multi(motifAmount, motifLength, pseudoCount, cutOff, seed,
                                             init_mode, UNBOUNDED)
    return _motif_lists(co, po, pw)


def _raise_failed_chain(status) -> None:
    for r, st in enumerate(status):
        if st != _native.GS_OK:
            raise _native._ERRORS.get(int(st), _native.DeviceError)(
                int(st), f"chain {r} of the batch failed")


def _single_start(motifMem, sources) -> np.ndarray:
    """The single chain statistics' start: one single position a sequence -> pos[N]."""
    if len(motifMem) != len(sources):
        raise _native.ArgumentError(_native.GS_E_ARG, "motifMem and sources differ in length")
    if not _is_single(1, motifMem):
        raise _native.ArgumentError(_native.GS_E_ARG, "the chain statistics need single positions")
    return _single_positions(motifMem)


def _chain_starts(motifMems, seeds, sources, single: bool = False):
    """What every batched chain driver checks of the starts it is given: one motifMem a seed,
    one entry a sequence.  With `single` they are single positions too -> pos[R, N] (None
    without motifMems, or without `single`)."""
    if motifMems is None:
        return None
    if len(motifMems) != len(seeds):
        raise _native.ArgumentError(_native.GS_E_ARG, "motifMems and seeds differ in length")
    if any(len(m) != len(sources) for m in motifMems):
        raise _native.ArgumentError(_native.GS_E_ARG, "a motifMem and sources differ in length")
    if not single:
        return None
    if not all(_is_single(1, m) for m in motifMems):
        raise _native.ArgumentError(_native.GS_E_ARG, "the chain statistics need single positions")
    return np.array([_single_positions(m) for m in motifMems],
                    np.int32).reshape(len(seeds), len(sources))


def _best_states(st, single_chain: bool = False) -> list:
    """The best state every chain visited, from a statistics dict: MotifIndex lists by
    _motif_lists where the chains have Positions lists ("best_cnt"), else by _motif_indices;
    [] for a chain that completed no counted sweep."""
    cnt, pos, pwms = st.get("best_cnt"), st["best_pos"], st["best_pwms"]
    if single_chain:
        pos, pwms = pos[None], pwms[None]
    return [[] if sweep < 0 else
            _motif_indices(pos[r], pwms[r]) if cnt is None else
            _motif_lists(cnt[r], pos[r], pwms[r]) for r, sweep in enumerate(st["best_sweep"])]


def _chain_lists(motifAmount, motifMems, n_sources):
    """The chains' lists at one capacity (the longest list's, at least motifAmount) ->
    (cap, cnt[R, N], pos[R, N, cap]); without motifMems (cap, None, None)."""
    if motifMems is None:
        return motifAmount, None, None
    cap = max([motifAmount] + [_lists(motifAmount, m)[0] for m in motifMems])
    cnt = np.zeros((len(motifMems), n_sources), np.int32)
    pos = np.full((len(motifMems), n_sources, cap), -1, np.int32)
    for r, mem in enumerate(motifMems):
        c1, cnt[r], p1 = _lists(motifAmount, mem)
        pos[r, :, :c1] = p1
    return cap, cnt, pos


def _run_lists_batched(motifAmount, motifLength, pseudoCount, cutOff, alphabet, sources, sweeps,
                       seeds, motifMems, init_mode, first_sweep, device):
    """runSweepsBatched on the Positions-list path: one Context.motif_run_multi_batch call,
    the chains' lists at one capacity (the longest list's, at least motifAmount)."""
    cap, cnt, pos = _chain_lists(motifAmount, motifMems, len(sources))
    ctx = _bind(alphabet, sources, device)
    cnt, pos, pwms, status = ctx.motif_run_multi_batch(motifAmount, motifLength, pseudoCount,
                                                       cutOff, sweeps, seeds, cnt, pos, init_mode,
                                                       first_sweep, cap)
    _raise_failed_chain(status)
    return [_motif_lists(cnt[r], pos[r], pwms[r]) for r in range(len(seeds))]


def _motif_indices(pos, pwms) -> list[MotifIndex]:
    return [createMotifIndex(w, [] if p < 0 else [p]) for p, w in zip(pos, pwms)]


def _motif_lists(cnt, pos, pwms) -> list[MotifIndex]:
    return [createMotifIndex(w, pos[n, :cnt[n]]) for n, w in enumerate(pwms)]


def _seed(seed: int | None) -> int:
    if seed is None:
        return int.from_bytes(os.urandom(8), "little")
    return int(seed) & (2**64 - 1)


def _fixed_kw(pcv, ppm) -> dict:
    """The pcv= / ppm= keywords of a batch call of the twins (none for the plain drivers)."""
    kw = {}
    if pcv is not None:
        kw["pcv"] = np.asarray(pcv, np.float64)
    if ppm is not None:
        kw["ppm"] = np.asarray(ppm, np.float64)
    return kw


def _batched_runs(ctx, count: int, motifLength, pseudoCount, cutOff, base: int,
                  init_mode: int, pcv=None, ppm=None) -> Callable[[int], list]:
    """Runs r = 0 … count - 1 of doMotifSampling (seed base + r) by one batch call,
    as a run(r) lookup for _replay_repetitions.  A run that raised raises when the
    loop asks for it, as the sequential loop would.  pcv / ppm: the ByPCV / WithPPM twin."""
    pos, pwms, _, status = ctx.motif_sampling_batch(
        motifLength, pseudoCount, cutOff, [base + r for r in range(count)], init_mode, UNBOUNDED,
        **_fixed_kw(pcv, ppm))

    def run(r: int) -> list:
        if status[r] != _native.GS_OK:
            raise _native._ERRORS.get(int(status[r]), _native.DeviceError)(
                int(status[r]), f"run {r} of the batch failed")
        return _motif_indices(pos[r], pwms[r])
    return run


def _batched_list_runs(ctx, count: int, motifLength, pseudoCount, cutOff, base: int,
                       init_mode: int, motifAmount: int, pcv=None,
                       ppm=None) -> Callable[[int], list]:
    """_batched_runs with Positions lists (motifAmount >= 2): one
    Context.motif_sampling_multi_batch call."""
    cnt, pos, pwms, _, status = ctx.motif_sampling_multi_batch(
        motifAmount, motifLength, pseudoCount, cutOff, [base + r for r in range(count)],
        init_mode, UNBOUNDED, **_fixed_kw(pcv, ppm))

    def run(r: int) -> list:
        if status[r] != _native.GS_OK:
            raise _native._ERRORS.get(int(status[r]), _native.DeviceError)(
                int(status[r]), f"run {r} of the batch failed")
        return _motif_lists(cnt[r], pos[r], pwms[r])
    return run


def _batched_site_runs(ctx, count: int, motifLength, pseudoCount, base: int,
                       init_mode: int, pcv=None, ppm=None) -> Callable[[int], list]:
    """Runs r = 0 … count - 1 of doSiteSampling (seed base + r) by one batch call, as a
    run(r) lookup for _replay_repetitions.  A run that raised raises when the loop asks
    for it, as the sequential loop would.  pcv / ppm: the WithBPV / WithPPM twin."""
    pos, score, _, status = ctx.site_sampling_batch(
        motifLength, pseudoCount, [base + r for r in range(count)], init_mode, UNBOUNDED,
        **_fixed_kw(pcv, ppm))

    def run(r: int) -> list:
        if status[r] != _native.GS_OK:
            raise _native._ERRORS.get(int(status[r]), _native.DeviceError)(
                int(status[r]), f"run {r} of the batch failed")
        return _pairs(score[r], pos[r])
    return run


def _best_of_repetitions(numberOfRepetitions: int, run: Callable[[int], list], ic: Callable,
                         initial_best: list) -> list:
    """The repetition loop shared by getMotifsWithBestInformationContent(s)
    (.fs:615-640, .fs:973-998), each run computed when the loop reaches it."""
    return _replay_repetitions(numberOfRepetitions, run, ic, initial_best)


def _replay_repetitions(numberOfRepetitions: int, run: Callable[[int], list], ic: Callable,
                        initial_best: list) -> list:
    """The loop of .fs:615-640 / .fs:973-998 over a run(r) lookup (computed on demand, or
    a finished table of runs 0 … numberOfRepetitions): stop after numberOfRepetitions or
    when a run equals the best; a run whose Σ score beats the best replaces it (one
    step later)."""
    n, acc, best = 0, [], initial_best
    while True:
        if n > numberOfRepetitions or acc == best:
            return best
        if ic(acc) > ic(best):
            n, acc, best = n + 1, [], (best if not acc else acc)
        else:
            n, acc = n + 1, run(n)


class SiteSampler:
    """SiteSampler module (.fs:298-707): the initialiser used by every driver."""

    @staticmethod
    def getPWMOfRandomStarts(motifLength: int, pseudoCount: float, alphabet, sources,
                             seed: int = 0, mode: int = 0, device: int = 0):
        """.fs:589-611 -> [(log2 best score, start)].  mode 0: every target draws its own
        starts for all others (the reference's O(N^2) structure); mode 1: one shared vector."""
        ctx = _bind(alphabet, sources, device)
        score, pos = ctx.random_starts(motifLength, pseudoCount, seed, mode)
        return _pairs(score, pos)

    @staticmethod
    def getPWMOfRandomStartsBatched(motifLength: int, pseudoCount: float, alphabet, sources,
                                    seeds, init_mode: int = 0, device: int = 0):
        """One getPWMOfRandomStarts per seed, all in one Context.random_starts_batch call:
        entry r is getPWMOfRandomStarts(..., seeds[r], init_mode).  A chain that raised
        raises here.  Faster than the loop at every measured size."""
        seeds = [int(s) & (2**64 - 1) for s in seeds]
        ctx = _bind(alphabet, sources, device)
        score, pos, status = ctx.random_starts_batch(motifLength, pseudoCount, seeds, init_mode)
        for r, st in enumerate(status):
            if st != _native.GS_OK:
                raise _native._ERRORS.get(int(st), _native.DeviceError)(
                    int(st), f"chain {r} of the batch failed")
        return [_pairs(score[r], pos[r]) for r in range(len(seeds))]

    @staticmethod
    def _refine(shift: int, motifLength: int, pseudoCount: float, alphabet, sources,
                startPositions, max_passes: int, device: int):
        if len(startPositions) != len(sources):
            raise _native.ArgumentError(_native.GS_E_ARG,
                                        "startPositions and sources differ in length")
        ctx = _bind(alphabet, sources, device)
        score = np.array([s for s, _ in startPositions], np.float64)
        pos = np.array([p for _, p in startPositions], np.int32)
        pos, score, np_ = ctx.site_refine(motifLength, pseudoCount, shift, pos, score, max_passes)
        _passes(np_, max_passes)
        return _pairs(score, pos)

    @staticmethod
    def getBestPWMSsWithStartPositions(motifLength: int, pseudoCount: float, alphabet, sources,
                                       startPositions, max_passes: int = UNBOUNDED, device: int = 0):
        """Gauss–Seidel passes over the live positions (.fs:554-585)."""
        return SiteSampler._refine(0, motifLength, pseudoCount, alphabet, sources,
                                   startPositions, max_passes, device)

    @staticmethod
    def getLeftShiftedBestPWMSs(motifLength: int, pseudoCount: float, alphabet, sources,
                                startPositions, max_passes: int = UNBOUNDED, device: int = 0):
        """Passes with the others one position upstream (.fs:519-550)."""
        return SiteSampler._refine(-1, motifLength, pseudoCount, alphabet, sources,
                                   startPositions, max_passes, device)

    @staticmethod
    def getRightShiftedBestPWMSs(motifLength: int, pseudoCount: float, alphabet, sources,
                                 startPositions, max_passes: int = UNBOUNDED, device: int = 0):
        """Passes with the others one position downstream (.fs:483-517)."""
        return SiteSampler._refine(1, motifLength, pseudoCount, alphabet, sources,
                                   startPositions, max_passes, device)

    @staticmethod
    def doSiteSampling(motifLength: int, pseudoCount: float, alphabet, sources,
                       seed: int | None = None, init_mode: int = 0, device: int = 0):
        """getPWMOfRandomStarts |> getBestPWMSsWithStartPositions |> left |> right
        shifted passes (.fs:697-701), on the device."""
        ctx = _bind(alphabet, sources, device)
        pos, score, _ = ctx.site_sampling(motifLength, pseudoCount, _seed(seed), init_mode,
                                          UNBOUNDED)
        return _pairs(score, pos)

    @staticmethod
    def getMotifsWithBestInformationContent(numberOfRepetitions: int, motifLength: int,
                                            pseudoCount: float, alphabet, sources,
                                            seed: int | None = None, init_mode: int = 0,
                                            device: int = 0, batch: bool = False):
        """Repeated doSiteSampling keeping the run of largest Σ score (.fs:615-640);
        run r uses seed + r.  batch=True computes every run r = 0 … numberOfRepetitions
        in one Context.site_sampling_batch call and replays the same loop over them: the
        same result, all runs paid for even when the loop stops early."""
        base = _seed(seed)
        if batch:
            ctx = _bind(alphabet, sources, device)
            return _replay_repetitions(
                numberOfRepetitions,
                _batched_site_runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength,
                                   pseudoCount, base, init_mode),
                lambda xs: sum(s for s, _ in xs), [(0.0, 0)])
        return _best_of_repetitions(
            numberOfRepetitions,
            lambda r: SiteSampler.doSiteSampling(motifLength, pseudoCount, alphabet, sources,
                                                 base + r, init_mode, device),
            lambda xs: sum(s for s, _ in xs), [(0.0, 0)])

    # ---- the caller's background (…WithBPV, .fs:301-459, .fs:691-695) and profile
    # (…OfPPM, .fs:644-689, .fs:703-707) twins
    @staticmethod
    def getPWMOfRandomStartsWithBPV(motifLength: int, pseudoCount: float, alphabet, sources,
                                    pcv, seed: int = 0, mode: int = 0, device: int = 0):
        """.fs:412-431: random starts, the others' PPM, getBestPWMSsWithBPV."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, pcv=pcv):
            score, pos = ctx.random_starts(motifLength, pseudoCount, seed, mode)
        return _pairs(score, pos)

    @staticmethod
    def _refine_bpv(shift, motifLength, pseudoCount, alphabet, sources, pcv, startPositions,
                    max_passes, device):
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, pcv=pcv):
            return SiteSampler._refine(shift, motifLength, pseudoCount, alphabet, sources,
                                       startPositions, max_passes, device)

    @staticmethod
    def findBestMotifWithStartPosition(motifLength: int, pseudoCount: float, alphabet, sources,
                                       pcv, startPositions, max_passes: int = UNBOUNDED,
                                       device: int = 0):
        """Gauss–Seidel passes with the caller's pcv (.fs:381-409)."""
        return SiteSampler._refine_bpv(0, motifLength, pseudoCount, alphabet, sources, pcv,
                                       startPositions, max_passes, device)

    @staticmethod
    def getLeftShiftedBestPWMSsWithBPV(motifLength: int, pseudoCount: float, alphabet, sources,
                                       pcv, startPositions, max_passes: int = UNBOUNDED,
                                       device: int = 0):
        """.fs:350-378."""
        return SiteSampler._refine_bpv(-1, motifLength, pseudoCount, alphabet, sources, pcv,
                                       startPositions, max_passes, device)

    @staticmethod
    def getRightShiftedBestPWMSsWithBPV(motifLength: int, pseudoCount: float, alphabet, sources,
                                        pcv, startPositions, max_passes: int = UNBOUNDED,
                                        device: int = 0):
        """.fs:318-347."""
        return SiteSampler._refine_bpv(1, motifLength, pseudoCount, alphabet, sources, pcv,
                                       startPositions, max_passes, device)

    @staticmethod
    def doSiteSamplingWithBPV(motifLength: int, pseudoCount: float, alphabet, sources, pcv,
                              seed: int | None = None, init_mode: int = 0, device: int = 0):
        """.fs:691-695: every stage with the caller's pcv."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, pcv=pcv):
            pos, score, _ = ctx.site_sampling(motifLength, pseudoCount, _seed(seed), init_mode,
                                          UNBOUNDED)
        return _pairs(score, pos)

    @staticmethod
    def getMotifsWithBestInformationContentWithBPV(numberOfRepetitions: int, motifLength: int,
                                                   pseudoCount: float, alphabet, sources, pcv,
                                                   seed: int | None = None, init_mode: int = 0,
                                                   device: int = 0, batch: bool = False):
        """.fs:434-459; run r uses seed + r.  batch=True computes every run
        r = 0 … numberOfRepetitions in one Context.site_sampling_batch(pcv=) call and
        replays the same loop over them: the same result, all runs paid for even when the
        loop stops early."""
        base = _seed(seed)
        if batch:
            ctx = _bind(alphabet, sources, device)
            return _replay_repetitions(
                numberOfRepetitions,
                _batched_site_runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength,
                                   pseudoCount, base, init_mode, pcv=pcv),
                lambda xs: sum(s for s, _ in xs), [(0.0, 0)])
        return _best_of_repetitions(
            numberOfRepetitions,
            lambda r: SiteSampler.doSiteSamplingWithBPV(motifLength, pseudoCount, alphabet,
                                                        sources, pcv, base + r, init_mode, device),
            lambda xs: sum(s for s, _ in xs), [(0.0, 0)])

    @staticmethod
    def getMotifsWithBestPWMSOfPPM(motifLength: int, pseudoCount: float, alphabet, sources,
                                   positionProbabilityMatrix, seed: int = 0, mode: int = 0,
                                   device: int = 0):
        """.fs:644-662: the random starts give the background, the caller's PPM scores."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, ppm=positionProbabilityMatrix, W=motifLength):
            score, pos = ctx.random_starts(motifLength, pseudoCount, seed, mode)
        return _pairs(score, pos)

    @staticmethod
    def doSiteSamplingWithPPM(motifLength: int, pseudoCount: float, alphabet, sources,
                              positionProbabilityMatrix, seed: int | None = None,
                              init_mode: int = 0, device: int = 0):
        """.fs:703-707: getMotifsWithBestPWMSOfPPM |> the three refinements."""
        ctx = _bind(alphabet, sources, device)
        with _fixed(ctx, ppm=positionProbabilityMatrix, W=motifLength):
            pos, score, _ = ctx.site_sampling(motifLength, pseudoCount, _seed(seed), init_mode,
                                          UNBOUNDED)
        return _pairs(score, pos)

    @staticmethod
    def getBestInformationContentOfPPM(numberOfRepetitions: int, motifLength: int,
                                       pseudoCount: float, alphabet, sources,
                                       positionProbabilityMatrix, seed: int | None = None,
                                       init_mode: int = 0, device: int = 0, batch: bool = False):
        """.fs:664-689; run r uses seed + r.  batch=True computes every run
        r = 0 … numberOfRepetitions in one Context.site_sampling_batch(ppm=) call and
        replays the same loop over them: the same result, all runs paid for even when the
        loop stops early."""
        base = _seed(seed)
        if batch:
            ctx = _bind(alphabet, sources, device)
            return _replay_repetitions(
                numberOfRepetitions,
                _batched_site_runs(ctx, max(0, int(numberOfRepetitions)) + 1, motifLength,
                                   pseudoCount, base, init_mode, ppm=positionProbabilityMatrix),
                lambda xs: sum(s for s, _ in xs), [(0.0, 0)])
        return _best_of_repetitions(
            numberOfRepetitions,
            lambda r: SiteSampler.doSiteSamplingWithPPM(motifLength, pseudoCount, alphabet,
                                                        sources, positionProbabilityMatrix,
                                                        base + r, init_mode, device),
            lambda xs: sum(s for s, _ in xs), [(0.0, 0)])


def _pairs(score, pos) -> list[tuple[float, int]]:
    return [(float(s), int(p)) for s, p in zip(score, pos)]
