"""GPU parity of the chain statistics kernels (gs_chainstats.hip) at the sizes their own loops
and capacity switches turn on: a second trip of every chunked loop and the far side of every
switch.  The shapes are the smallest that cross them:

  * the single chain's register-batched ordered sum (1 536 entries a batch, two batches drained
    in turn, the tail loaded first and added last): 0 to 4 whole batches, tails of 0, 1, 63 and
    1 535 entries;
  * the chain batch's and the list chains' ordered sum through LDS (2 048 entries a chunk) and
    the batch's bins split over several workgroups a chain (256 targets a tile);
  * modes of rows longer than one trip of 256 bins, per chain and pooled;
  * the pool decisions (256 threads a chain) past the first 256 bins and sequences;
  * the agreement beyond the 512 chains whose sums a workgroup collects in LDS.

The references are those of the files the helpers come from: the stepwise loop on a second
context with informationContent, np.argmax by restate, ChainStats.agreement().  Everything is
integers or bits: every comparison is exact."""
import numpy as np
import pytest

from conftest import make_dataset
from gibbssampling_amd import Context
from gibbssampling_amd.sampler import informationContent
from test_gpu_agreement import KEYS as AGR_KEYS
from test_gpu_agreement import agreement_twice, ragged
from test_gpu_agreement import restate as agreement_restate
from test_gpu_agreement import same as same_agreement
from test_gpu_list_summary import POOL as LIST_POOL
from test_gpu_list_summary import count_cells, random_slabs, sequences
from test_gpu_list_summary import restate as list_restate
from test_gpu_list_summary import same as same_list
from test_gpu_list_summary import summary_twice as list_summary_twice
from test_gpu_run_batch_stats import first_best, tally
from test_gpu_run_multi_batch_stats import check_chain
from test_gpu_run_multi_batch_stats import stepwise as list_stepwise
from test_gpu_run_stats import (CUTOFF, PC, SEED, Pair, bits, check_exact, counted_sweeps,
                                dataset, stepwise)
from test_gpu_summary import GROUPS, random_bins, reduce_rows, restate, same, summary_twice

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
BATCH = 1536  # 64 * kStatsDepth: entries a register batch of gs_run_stats_kernel
CHUNK = 2048  # kSumChunk: entries of a PWMS row a workgroup stages through LDS at a time
TRIP = 256    # 64 * kSumDepth: bins of a row a wavefront reads a trip


def plain_sum(row):
    """The row added up from the left, in index order."""
    acc = 0.0
    for x in np.asarray(row, np.float64).tolist():
        acc = acc + x
    return acc


def order_matters(rows):
    """Whether the plain left-to-right sum of some row differs in bits from the trace's fixed
    order: a kernel that added the entries in another order would then be seen."""
    return any(bits([plain_sum(q)])[0] != bits([informationContent(q)])[0] for q in rows)


# ---- a. the single chain's ordered sum (gs_run_stats_kernel) ----

# N: the data set's seed.  Chosen so that the targets at the seams hold a motif in every
# counted sweep (a Positions [] target's PWMS entry is 0.0, and a dropped zero changes no sum).
SINGLE = {1535: 1535, 1536: 1536, 1537: 1537, 3072: 3072, 3073: 3073, 4608: 4608, 6207: 6207}


def single_seams(N):
    """The last entry of every whole batch, the first after it, and the row's last."""
    whole = N // BATCH
    at = {N - 1}
    for k in range(1, whole + 1):
        at |= {k * BATCH - 1, k * BATCH}
    return sorted(i for i in at if i < N)


@pytest.mark.parametrize("N", list(SINGLE))
def test_single_chain_sum_across_register_batches(N):
    W, T = 12, 3
    burn_in, thin = 0, 1
    codes, offsets, _ = dataset(N, 24, 40, W, DNA, seed=SINGLE[N])
    pair = Pair({"bg_mode": 0}, DNA, codes, offsets)
    try:
        p0 = pair.step.random_starts(W, PC, SEED, 1)[1]  # starts that hold a motif
        P, Q = stepwise(pair.step, W, p0, T)
        off = pair.step.occupancy_offsets(W)
        pos, pw, s = pair.stat.motif_run_stats(W, PC, CUTOFF, T, SEED, p0, burn_in=burn_in,
                                               thin=thin)
    finally:
        pair.close()
    assert np.array_equal(pos, P[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
    check_exact(s, P, Q, off, burn_in, thin)
    ts = counted_sweeps(T, burn_in, thin)
    seams = single_seams(N)
    assert (Q[ts][:, seams] != 0.0).all(), (seams, Q[ts][:, seams])
    assert order_matters(Q[ts])


# ---- b. the chain batch: the sum through LDS chunks, the bins over several workgroups ----

B_SEEDS = [77, 5_000_000_007, 77]  # rows 0 and 2: the same seed
B_W, B_T, B_BURN = 8, 4, 1
# N: the data set's seed, chosen as SINGLE's
BATCHES = {257: 257, 2048: 2048, 2049: 2049, 4100: 4100}
_batch = {}


def batch_reference(gpu_ctx, N):
    """One size, computed once and left unchanged: the data, the stepwise states (B_T one-sweep
    calls from the starts of mode 1) and the bins' offsets."""
    if N not in _batch:
        codes, offsets = make_dataset(N, 40, B_W, DNA, seed=BATCHES[N], ragged=True, mut=0.1)
        gpu_ctx.set_sequences(codes, offsets, DNA)
        pos, _, st = gpu_ctx.motif_run_batch(B_W, PC, CUTOFF, 0, B_SEEDS, init_mode=1)
        assert not st.any()
        P, Q = [], []
        for t in range(B_T):
            pos, pw, st = gpu_ctx.motif_run_batch(B_W, PC, CUTOFF, 1, B_SEEDS, pos=pos,
                                                  first_sweep=t)
            assert not st.any()
            P.append(pos)
            Q.append(pw)
        out = (codes, offsets, np.array(P), np.array(Q), gpu_ctx.occupancy_offsets(B_W))
        for a in out:
            a.setflags(write=False)
        _batch[N] = out
    return _batch[N]


def batch_call(ctx, codes, offsets):
    ctx.set_sequences(codes, offsets, DNA)
    pos, pw, status, s = ctx.motif_run_batch_stats(B_W, PC, CUTOFF, B_T, B_SEEDS, init_mode=1,
                                                   burn_in=B_BURN)
    assert not status.any()
    return pos, pw, s


def same_batch(got, want):
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(bits(a) if a.dtype == np.float64 else a,
                              bits(b) if b.dtype == np.float64 else b)
    assert set(got[2]) == set(want[2])
    for k, v in want[2].items():
        assert got[2][k].shape == v.shape, k
        assert np.array_equal(bits(got[2][k]) if v.dtype == np.float64 else got[2][k],
                              bits(v) if v.dtype == np.float64 else v), k


@pytest.mark.parametrize("N", list(BATCHES))
def test_batch_sum_across_chunks_and_bins_across_workgroups(gpu_ctx, N):
    codes, offsets, P, Q, off = batch_reference(gpu_ctx, N)
    auto = batch_call(gpu_ctx, codes, offsets)
    pos, pw, s = auto
    ts = counted_sweeps(B_T, B_BURN, 1)
    R = len(B_SEEDS)
    assert np.array_equal(s["offsets"], off)
    assert s["occupancy"].shape == (R, off[-1]) and s["ic"].shape == (R, len(ts))
    assert np.array_equal(pos, P[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
    for r in range(R):
        assert np.array_equal(s["occupancy"][r], tally(off, [P[t][r] for t in ts])), r
        per_seq = np.add.reduceat(s["occupancy"][r], off[:-1])
        assert np.array_equal(per_seq, np.full(N, len(ts))), r
        ics = [informationContent(Q[t][r]) for t in ts]
        assert np.array_equal(bits(s["ic"][r]), bits(ics)), r
        b = first_best(ics)
        assert s["best_sweep"][r] == ts[b], r
        assert np.array_equal(s["best_pos"][r], P[ts[b]][r]), r
        assert np.array_equal(bits(s["best_pwms"][r]), bits(Q[ts[b]][r])), r
    # the duplicate seed: identical rows
    for k in ("occupancy", "ic", "best_sweep", "best_pos"):
        assert np.array_equal(s[k][0], s[k][2]), k
    assert np.array_equal(bits(s["best_pwms"][0]), bits(s["best_pwms"][2]))
    # the entries either side of the chunk's end and the row's last are there to be dropped
    seams = sorted({i for i in (CHUNK - 1, CHUNK, N - 1) if i < N})
    assert (Q[ts][:, :, seams] != 0.0).all(), (seams, Q[ts][:, :, seams])
    assert order_matters(Q[t][r] for t in ts for r in range(R))
    # workgroups past a chain's first have motifs to count
    assert (P[ts][:, :, TRIP:] >= 0).any()
    if N < CHUNK + 1:
        return
    # three workgroups a chain do not divide the 256-target tiles evenly
    for tuning in ({"run_stats_blocks": 3}, {"run_stats_blocks": 3, "run_stats_atomic": 0}):
        ctx = Context(0, tuning=tuning)
        try:
            other = batch_call(ctx, codes, offsets)
        finally:
            ctx.close()
        same_batch(other, auto)


# ---- c. a list chain's ordered sum (gs_run_multi_batch_stats_kernel) ----

C_DATA_SEED = 2049


def test_list_chain_sum_across_chunks():
    N, M, cap, W, T, seeds = CHUNK + 1, 2, 2, 6, 3, [3, 4, 5]
    codes, offsets = make_dataset(N, 40, W, DNA, seed=C_DATA_SEED, ragged=True, mut=0.1)
    step, stat = Context(0), Context(0)
    try:
        for ctx in (step, stat):
            ctx.set_sequences(codes, offsets, DNA)
        c0, p0, _, st = step.motif_run_multi_batch(M, W, PC, 1.0, 0, seeds, cap=cap)
        assert not st.any()
        C, P, Q, st = list_stepwise(step, M, W, 1.0, T, seeds, c0, p0, cap=cap)
        assert not st.any()
        cnt, pos, pw, status, s = stat.motif_run_multi_batch_stats(M, W, PC, 1.0, T, seeds, cap=cap)
    finally:
        step.close()
        stat.close()
    assert not status.any() and s["best_pos"].shape == (3, N, cap)
    assert np.array_equal(cnt, C[-1]) and np.array_equal(pos, P[-1])
    assert np.array_equal(bits(pw), bits(Q[-1]))
    for r in range(len(seeds)):
        check_chain(s, r, s["offsets"], M, C, P, Q, list(range(T)))
    seams = [CHUNK - 1, CHUNK, N - 1]
    assert (Q[:, :, seams] != 0.0).all(), Q[:, :, seams]
    assert order_matters(Q[t][r] for t in range(T) for r in range(len(seeds)))
    assert C.max() >= 2  # lists of more than one position occur


# ---- d. modes of rows longer than one trip (gs_summary_kernel, summary_pooled_rows) ----

ROW_BINS = (2, 255, 256, 257, 300, 512, 513, 1100)
# name: (bins of the row, {bin: count} in every chain, or one dict a chain)
PLANTED = {
    # the same lane and register slot, one trip apart: the first wins
    "same_slot": (600, {5: 9, 5 + TRIP: 9, 7: 8}),
    # ... and in the third and fifth trip
    "same_slot_later": (1100, {2 * TRIP + 44: 9, 4 * TRIP + 44: 9, 3: 8}),
    # lane 63 of one trip and lane 0 of the next
    "trip_neighbours": (300, {TRIP - 1: 9, TRIP: 9, 100: 8}),
    # the only maximum at the row's last bin, in a partial last trip
    "last_of_257": (257, {256: 9, 10: 3}),
    "last_of_1100": (1100, {1099: 9, 10: 3, 1000: 8}),
    # a maximum in the second trip larger than the first trip's
    "second_trip": (513, {7: 5, 300: 9, 20: 4}),
    # a tie that only the pool has: the chains' modes differ
    "pooled_tie": (600, [{17: 9}, {17 + TRIP: 9}, {17: 4, 17 + TRIP: 4}]),
}
# name: (mode bin of every chain or one a chain, its count likewise, pooled bin, pooled count)
EXPECT = {
    "same_slot": (5, 9, 5, 27),
    "same_slot_later": (2 * TRIP + 44, 9, 2 * TRIP + 44, 27),
    "trip_neighbours": (TRIP - 1, 9, TRIP - 1, 27),
    "last_of_257": (256, 9, 256, 27),
    "last_of_1100": (1099, 9, 1099, 27),
    "second_trip": (300, 9, 300, 27),
    "pooled_tie": ([17, 17 + TRIP, 17], [9, 9, 4], 17, 13),
}


@pytest.mark.parametrize("alpha,W", [(DNA, 12), (PROTEIN, 4)])
def test_modes_of_long_rows(gpu_ctx, alpha, W):
    R, nc = 3, 40
    names = list(PLANTED)
    codes, offsets = sequences(ROW_BINS + tuple(PLANTED[k][0] for k in names), W, alpha,
                               seed=W + len(alpha))
    gpu_ctx.set_sequences(codes, offsets, alpha)
    off = gpu_ctx.occupancy_offsets(W)
    assert np.diff(off).tolist()[:len(ROW_BINS)] == list(ROW_BINS)
    occ = random_bins(off, R, nc, seed=W)
    where = {}
    for i, k in enumerate(names):
        n = where[k] = len(ROW_BINS) + i  # never sequence 0: the pool's rule reads it
        rows = PLANTED[k][1]
        occ[:, off[n]:off[n + 1]] = 0
        for r in range(R):
            for b, c in (rows[r] if isinstance(rows, list) else rows).items():
                occ[r, off[n] + b] = c
    want = restate(occ, off, nc, codes, offsets, alpha, W)
    got = summary_twice(gpu_ctx, W, occ, nc)
    same(got, want)
    assert got["n_pooled"][0] == R
    for k, (mode, count, pmode, pcount) in EXPECT.items():
        n = where[k]
        assert (got["mode_pos"][:, n] == np.array(mode) - 1).all(), k
        assert (got["mode_count"][:, n] == np.array(count)).all(), k
        assert got["pooled_pos"][n] == pmode - 1 and got["pooled_count"][n] == pcount, k
    # the random rows' modes lie past the first trip as well
    mp, _ = reduce_rows(occ, off)
    assert (mp[:, :len(ROW_BINS)] >= TRIP).any()
    # each output group alone equals the same group of the full call
    for g, keys in GROUPS.items():
        part = summary_twice(gpu_ctx, W, occ, nc, **{k: k == g for k in GROUPS})
        assert set(part) == set(keys)
        same(part, got, keys)


# ---- e. the pool decisions past the first 256 bins and sequences ----

def test_pool_rule_reads_all_of_a_long_first_row(gpu_ctx):
    """gs_summary_pool_kernel: sequence 0 has 600 bins and every count of it lies in bins from
    256 on, one of them from 512 on."""
    W, R, nc = 12, 3, 40
    codes, offsets = sequences((600, 65, 257), W, DNA, seed=5)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    off = gpu_ctx.occupancy_offsets(W)
    assert off[1] - off[0] == 600
    occ = random_bins(off, R, nc, seed=6)
    occ[:, off[0]:off[1]] = 0
    for r in range(R):
        for b, c in {TRIP + r: 10, 300: 7, 2 * TRIP - 1: 3, 2 * TRIP: 12, 599: 8}.items():
            occ[r, off[0] + b] = c
    assert not occ[:, off[0]:off[0] + TRIP].any()
    assert (occ[:, off[0]:off[1]].sum(axis=1) == nc).all()
    got = summary_twice(gpu_ctx, W, occ, nc)
    same(got, restate(occ, off, nc, codes, offsets, DNA, W))
    assert got["n_pooled"][0] == 3
    agr = agreement_twice(gpu_ctx, W, occ, nc)
    same_agreement(agr, agreement_restate(occ, off, nc))
    assert agr["n_pooled"][0] == 3 and (agr["chain_dist"] >= 0).all()
    # one count less in a bin of the third trip: exactly that chain drops out
    short = occ.copy()
    short[1, off[0] + 599] -= 1
    got = summary_twice(gpu_ctx, W, short, nc)
    same(got, restate(short, off, nc, codes, offsets, DNA, W))
    assert got["n_pooled"][0] == 2
    assert np.array_equal(got["pooled_counts"], got["counts"][[0, 2]].sum(axis=0))
    agr = agreement_twice(gpu_ctx, W, short, nc)
    same_agreement(agr, agreement_restate(short, off, nc))
    assert agr["n_pooled"][0] == 2
    assert agr["chain_dist"][1] == -1 and agr["chain_agree"][1] == -1
    assert (agr["chain_dist"][[0, 2]] >= 0).all() and 1 not in agr["spread_chain"].tolist()


def test_list_pool_rule_reads_the_sequences_past_256(gpu_ctx):
    """gs_list_summary_pool_kernel: only sequence 256, a second trip of the chain's 256 threads,
    is one site count short."""
    N, W, M, R, nc = 257, 4, 2, 3, 40
    codes, offsets = sequences([(2, 3, 40, 65)[n % 4] for n in range(N)], W, DNA, seed=9)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    off = gpu_ctx.occupancy_offsets(W)
    occ, sites = random_slabs(off, R, M, nc, seed=10)
    cells = count_cells(occ, off, codes, offsets, DNA, W)
    short = sites.copy()
    short[1, N - 1, int(np.argmax(short[1, N - 1]))] -= 1
    assert (short[:, :N - 1].sum(axis=2) == nc).all() and short[1, N - 1].sum() == nc - 1
    want, _, _ = list_restate(occ, short, off, nc, W, cells)
    got = list_summary_twice(gpu_ctx, W, M, occ, short, nc)
    same_list(got, want)
    assert want["n_pooled"][0] == 2 and got["n_pooled"][0] == 2
    same_list(got, want, LIST_POOL)
    assert np.array_equal(got["pooled_counts"], got["counts"][[0, 2]].sum(axis=0))
    # the row repaired: everybody is pooled
    want, _, _ = list_restate(occ, sites, off, nc, W, cells)
    got = list_summary_twice(gpu_ctx, W, M, occ, sites, nc)
    same_list(got, want)
    assert got["n_pooled"][0] == 3


# ---- f. the agreement beyond the LDS accumulators (gs_agreement_kernel) ----

F_BINS = (2, 65, 257, 512, 513, 64)  # one row longer than the 512 staged bins
F_W, F_NC = 12, 37


def distance(occ, pooled, r):
    """Chain r's D summed over the sequences, from the definition."""
    rows = np.asarray(occ, np.int64)
    idx = np.nonzero(pooled)[0]
    pool = rows[idx].sum(axis=0)
    return int(np.abs(len(idx) * rows[r] - pool).sum())


def check_left_out(got, out, R):
    """The chains `out` got (-1, -1) and no sequence names one of them; the others did not."""
    keep = np.setdiff1d(np.arange(R), out)
    assert (got["chain_dist"][out] == -1).all() and (got["chain_agree"][out] == -1).all()
    assert (got["chain_dist"][keep] >= 0).all() and (got["chain_agree"][keep] >= 0).all()
    assert not np.isin(got["spread_chain"], out).any()
    assert got["n_pooled"][0] == len(keep)


@pytest.mark.parametrize("R", [257, 512, 513])
def test_agreement_of_more_chains_than_the_accumulators(gpu_ctx, R):
    codes, offsets = ragged(len(F_BINS), F_W, DNA, seed=21, bins=F_BINS)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    off = gpu_ctx.occupancy_offsets(F_W)
    assert np.diff(off).tolist() == list(F_BINS)
    occ = random_bins(off, R, F_NC, seed=300 + R)
    got = agreement_twice(gpu_ctx, F_W, occ, F_NC)
    same_agreement(got, agreement_restate(occ, off, F_NC))
    check_left_out(got, np.array([], np.int64), R)
    assert got["spread"].any() and (got["agree"] < R).any() and got["chain_agree"].any()
    everyone = np.ones(R, bool)
    for r in (0, R - 1):
        assert got["chain_dist"][r] == distance(occ, everyone, r), r
    if R <= 512:
        return
    # one chain left out by the rule, first and last
    for r in (0, R - 1):
        short = occ.copy()
        short[r, off[0] + int(np.argmax(short[r, off[0]:off[1]]))] -= 1
        got = agreement_twice(gpu_ctx, F_W, short, F_NC)
        same_agreement(got, agreement_restate(short, off, F_NC))
        check_left_out(got, np.array([r]), R)
        pooled = everyone.copy()
        pooled[r] = False
        other = R - 1 - r
        assert got["chain_dist"][other] == distance(short, pooled, other)
    # an explicit mask: three chains pooled, either side of the accumulators' end
    mask = np.zeros(R, np.int32)
    mask[[0, 511, 512]] = 1
    got = agreement_twice(gpu_ctx, F_W, occ, F_NC, mask)
    same_agreement(got, agreement_restate(occ, off, F_NC, mask != 0))
    check_left_out(got, np.nonzero(mask == 0)[0], R)
    for r in (0, 512):
        assert got["chain_dist"][r] == distance(occ, mask != 0, r), r
    assert set(got) == set(AGR_KEYS)
