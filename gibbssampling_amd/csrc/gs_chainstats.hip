// gs_chainstats.hip — the device-side consumers of a chain batch's sweeps
// (gs_motif_run_batch_stats, DESIGN.md §9.25, and gs_motif_run_multi_batch_stats, §9.26): per
// counted sweep one launch, stream-ordered right after that sweep's launches, which left the
// chains' positions (or Positions lists) and PWMS rows and their skip words.  And the
// consumer of the single chain's sweeps (gs_run_sweeps_stats, §9.27): one launch after a
// counted sweep of any of the sweep kernels, which left d_pos, d_pwms and the error word.
// And the reduction of the bins those launches filled to what a caller keeps of them (the
// ..._summary calls and gs_occupancy_summary, §9.28): each sequence's first-maximum bin and the
// count matrix over the counted states.  And the chains' agreement with their pool
// (gs_occupancy_agreement, gs_motif_run_batch_agreement, §9.31).
#include "gs_ctx.h"
#include "gs_wave.h"

namespace {

constexpr int kSumChunk = 2048;  // doubles of LDS a workgroup stages a PWMS row through

// Workgroup 0 of a running chain, all 256 threads: the ordered sum of the chain's PWMS row
// (the contract of both entry points' traces: 64 lane-strided serial sums from +0.0, lane l
// adding n = l, l + 64, .. in increasing n, then the halving tree v[l] += v[l + s],
// s = 32 .. 1), its trace entry, and the decision against the running best (the first counted
// sweep is taken; later ones only when strictly larger, .fs:989; a NaN never wins).  Whether
// this sweep became the chain's best, workgroup-uniform.
__device__ __forceinline__ bool chain_sum_best(const double *pwms_row, int n_local, double *ic_entry,
                                               int64_t *best_sweep, double *best_ic, int64_t sweep,
                                               double *buf, int *win) {
    const int tid = threadIdx.x;
    if (tid == 0) *win = 0;
    // the row through LDS, kSumChunk entries at a time (a multiple of 64: lane l keeps
    // n = l mod 64): the whole workgroup's loads are in flight at once, and the
    // serial adds of wavefront 0 wait on LDS only (10 000 targets: a launch measured
    // 15 us against 40 with wavefront 0 reading global memory)
    double v = 0.0;
    for (int base = 0; base < n_local; base += kSumChunk) {
        const int m = min(kSumChunk, n_local - base);
        __syncthreads();
        for (int i = tid; i < m; i += 256) buf[i] = pwms_row[base + i];
        __syncthreads();
        if (tid < 64)
            for (int i = tid; i < m; i += 64) v = v + buf[i];
    }
    if (tid < 64) {
        for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
        if (tid == 0) {
            if (ic_entry) *ic_entry = v;
            if (best_sweep && (*best_sweep < 0 || v > *best_ic)) {
                *best_sweep = sweep;
                *best_ic = v;
                *win = 1;
            }
        }
    }
    __syncthreads();
    return *win != 0;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// One to a bin that no other thread of the launch touches.
__device__ __forceinline__ void bump(int32_t *bin, int atomic) {
    if (atomic)
        atomicAdd(bin, 1);
    else
        *bin += 1;
}

}  // namespace

// gridDim.x / n_chains workgroups a chain.  A chain whose skip word is set contributes
// nothing (its trace entry is a quiet NaN).  Workgroup 0 of a chain: wavefront 0 forms the
// ordered sum of the PWMS row, which the workgroup stages through LDS, writes the trace entry
// and decides against the running best (chain_sum_best); on a win the whole workgroup copies
// the two rows into the best slabs.
// All workgroups: one to bin off[n] + 1 + pos[n] of the chain's histogram for their share
// of the targets.  A chain's bins of one sweep are distinct and launches are stream-ordered,
// so the plain read-modify-write (a.atomic == 0) and the non-returning atomic add race with
// nothing; a position outside [-1, L - W] is not counted.
extern "C" __global__ void __launch_bounds__(256)
gs_run_batch_stats_kernel(RunStatsArgs a) {
    __shared__ double buf[kSumChunk];
    __shared__ int win;
    const int tid = threadIdx.x;
    const int bpc = gridDim.x / a.n_chains;
    const int r = blockIdx.x / bpc, blk = blockIdx.x - r * bpc;
    const bool skipped = a.skip[r] != 0;  // workgroup-uniform
    const int64_t row = (int64_t)r * a.n_local;
    const bool sums = a.ic || a.best_sweep;
    if (blk == 0 && sums && skipped && tid == 0 && a.ic)
        a.ic[(int64_t)r * a.ic_stride] = quiet_nan();
    if (skipped) return;
    if (blk == 0 && sums &&
        chain_sum_best(a.pwms + row, a.n_local, a.ic ? a.ic + (int64_t)r * a.ic_stride : nullptr,
                       a.best_sweep ? a.best_sweep + r : nullptr, a.best_ic + r, a.sweep, buf, &win))
        for (int n = tid; n < a.n_local; n += 256) {
            a.best_pos[row + n] = a.pos[row + n];
            a.best_pwms[row + n] = a.pwms[row + n];
        }
    if (!a.occ) return;
    int32_t *occ = a.occ + (int64_t)r * a.H;
    for (int n = blk * 256 + tid; n < a.n_local; n += bpc * 256) {
        const int64_t o = a.off[n];
        const int64_t k = (int64_t)a.pos[row + n] + 1;
        if (k < 0 || k >= a.off[n + 1] - o) continue;
        bump(&occ[o + k], a.atomic);
    }
}

hipError_t gs_run_batch_stats_launch(const RunStatsArgs &a, int blocks_per_chain, hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_run_batch_stats_kernel, dim3(a.n_chains * blocks_per_chain), dim3(256), 0,
                       s, a);
    return hipGetLastError();
}

// The same over Positions lists (gs_motif_run_multi_batch_stats), for the
// chains of one round: gridDim.x / n_chains workgroups a launch index c, chain r = chains[c].
// A chain whose skip word is set (it raised, or was parked, in this sweep or before)
// contributes nothing; its trace entry is a quiet NaN, which the round that resumes a parked
// chain overwrites.  Workgroup 0 of a chain: chain_sum_best, and on a win the cnt row, the
// pos rows (flat over n_local * cap) and the PWMS row into the best slabs.  All workgroups,
// one thread a (target, slot) pair of the flat list slab, so that a wavefront's reads of pos
// are one coalesced load deep: slot 0 adds one to sites[n][cnt] and, for an empty list, to
// bin off[n]; slot i < cnt one to bin off[n] + 1 + pos[i].  A sweep's list holds pairwise
// distinct starts (.fs:727-742), so the bins one launch touches in one chain are distinct
// and launches are stream-ordered: both kinds of add race with nothing.  A length outside
// [0, M] and a start outside [0, L - W] are not counted: no store leaves the chain's slab.
extern "C" __global__ void __launch_bounds__(256)
gs_run_multi_batch_stats_kernel(RunMultiStatsArgs a) {
    __shared__ double buf[kSumChunk];
    __shared__ int win;
    const int tid = threadIdx.x;
    const int bpc = gridDim.x / a.n_chains;
    const int c = blockIdx.x / bpc, blk = blockIdx.x - c * bpc;
    const int r = a.chains ? a.chains[c] : c;
    const int64_t row = (int64_t)r * a.n_local;
    const int cap = a.cap, flat = a.n_local * cap;  // (the slabs' 4 GiB bound: < 2^30)
    if (a.skip[r] != 0) {  // workgroup-uniform
        if (blk == 0 && tid == 0 && a.ic) a.ic[(int64_t)r * a.ic_stride] = quiet_nan();
        return;
    }
    if (blk == 0 && (a.ic || a.best_sweep) &&
        chain_sum_best(a.pwms + row, a.n_local, a.ic ? a.ic + (int64_t)r * a.ic_stride : nullptr,
                       a.best_sweep ? a.best_sweep + r : nullptr, a.best_ic + r, a.sweep, buf,
                       &win)) {
        for (int n = tid; n < a.n_local; n += 256) {
            a.best_cnt[row + n] = a.cnt[row + n];
            a.best_pwms[row + n] = a.pwms[row + n];
        }
        for (int x = tid; x < flat; x += 256) a.best_pos[row * cap + x] = a.pos[row * cap + x];
    }
    if (!a.occ && !a.sites) return;
    int32_t *occ = a.occ ? a.occ + (int64_t)r * a.H : nullptr;
    for (int x = blk * 256 + tid; x < flat; x += bpc * 256) {
        const int n = x / cap, i = x - n * cap;
        const int cnt = a.cnt[row + n];
        if (cnt < 0 || cnt > a.M) continue;
        if (i == 0 && a.sites) bump(&a.sites[(row + n) * (a.M + 1) + cnt], a.atomic);
        if (!occ || (i > 0 && i >= cnt)) continue;
        const int64_t o = a.off[n];
        const int64_t k = cnt == 0 ? 0 : (int64_t)a.pos[row * cap + x] + 1;
        if (k < (cnt == 0 ? 0 : 1) || k >= a.off[n + 1] - o) continue;
        bump(&occ[o + k], a.atomic);
    }
}

hipError_t gs_run_multi_batch_stats_launch(const RunMultiStatsArgs &a, int blocks_per_chain,
                                           hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_run_multi_batch_stats_kernel, dim3(a.n_chains * blocks_per_chain),
                       dim3(256), 0, s, a);
    return hipGetLastError();
}

// The consumer of one counted sweep of the single chain (gs_run_sweeps_stats, DESIGN.md
// §9.27): one long row instead of 64 short ones.  Workgroup 0, when the trace or the best
// state is asked for: wavefront 0 forms the ordered sum of the contract (64 lane-strided
// serial sums from +0.0, lane l adding n = l, l + 64, .. in increasing n, then the halving
// tree) with its entries loaded straight into registers, kStatsDepth coalesced 512-byte
// wavefront loads a batch and the next batch in flight under the adds of this one; there is
// no barrier a chunk and no LDS staging.  An entry past the row's end is +0.0: a partial
// sum that started from +0.0 is never -0.0, so the add changes no bit.  Lane 0 writes the
// trace entry and decides against the running best (chain_sum_best's rule: the first
// counted sweep is taken, a later one only when strictly larger, a NaN never); on a win the
// whole workgroup copies the two rows, behind the one barrier that hands the decision
// over, or, for a long row (copy_inline == 0), the workgroups of gs_run_stats_best_kernel
// do, launched behind this kernel.  Every other workgroup (all of them without sums): one to bin off[n] + 1 + pos[n]
// for its share of the targets, a position outside [-1, L - W] not counted.  The bins one
// launch touches are distinct and launches are stream-ordered: both kinds of add race with
// nothing.  No workgroup waits on another.  A set error word (the chain raised in this
// sweep or before): the trace entry is a quiet NaN and nothing else is written.
constexpr int kStatsDepth = 24;  // wavefront loads a batch: so many in flight ahead of the adds

extern "C" __global__ void __launch_bounds__(256)
gs_run_stats_kernel(ChainStatsArgs a) {
    __shared__ int win;
    const int tid = threadIdx.x;
    const bool sums = a.ic || a.best_sweep;
    if (*a.err != 0) {  // grid-uniform
        if (blockIdx.x == 0 && tid == 0 && a.ic) *a.ic = quiet_nan();
        return;
    }
    int blk = blockIdx.x, nblk = gridDim.x;
    if (sums) {
        if (blk == 0) {
            if (tid == 0) win = 0;
            if (tid < 64) {
                // Two register batches, A and B, filled and drained in turn: the loads of one
                // are in flight under the adds of the other.  Every load is issued, at an
                // index clamped into the row, and an entry past the end is replaced where it
                // is added: a branch around a load, or a copy of a batch, would make the adds
                // wait for each load in turn.
                const unsigned n = (unsigned)a.n_local, lane = (unsigned)tid;
                constexpr unsigned kBatch = 64 * kStatsDepth;
                const unsigned whole = n / kBatch;  // batches with every entry in the row
                // batch b of the row; past the last whole one that one again (never added)
                const auto fill = [&](double (&r)[kStatsDepth], unsigned b) {
                    const double *p = a.pwms + (size_t)min(b, whole - 1) * kBatch + lane;
#pragma unroll
                    for (int k = 0; k < kStatsDepth; ++k) r[k] = p[64 * k];
                };
                double v = 0.0;
                const auto drain = [&](const double (&r)[kStatsDepth]) {
#pragma unroll
                    for (int k = 0; k < kStatsDepth; ++k) v = v + r[k];
                };
                // the row's tail, short of a batch: loaded first, added last
                double T[kStatsDepth], A[kStatsDepth], B[kStatsDepth];
#pragma unroll
                for (int k = 0; k < kStatsDepth; ++k) {
                    const unsigned i = whole * kBatch + lane + 64 * k;
                    const double x = a.pwms[min(i, n - 1)];
                    T[k] = i < n ? x : 0.0;
                }
                if (whole > 0) {  // wavefront-uniform, like every branch below
                    fill(A, 0);
                    for (unsigned b = 0; b < whole; b += 2) {
                        // (the scheduler is held to this order: it would otherwise sink a
                        // batch's loads below the other's adds, and the two would take turns)
                        fill(B, b + 1);
                        __builtin_amdgcn_sched_barrier(0);
                        drain(A);
                        __builtin_amdgcn_sched_barrier(0);
                        fill(A, b + 2);
                        __builtin_amdgcn_sched_barrier(0);
                        if (b + 1 < whole) drain(B);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                drain(T);
                for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
                if (tid == 0) {
                    if (a.ic) *a.ic = v;
                    if (a.best_sweep && (*a.best_sweep < 0 || v > *a.best_ic)) {
                        *a.best_sweep = a.sweep;
                        *a.best_ic = v;
                        win = 1;
                    }
                }
            }
            __syncthreads();
            if (win && a.copy_inline)
                for (int n = tid; n < a.n_local; n += 256) {
                    a.best_pos[n] = a.pos[n];
                    a.best_pwms[n] = a.pwms[n];
                }
            return;
        }
        --blk;
        --nblk;
    }
    if (!a.occ) return;
    for (int n = blk * 256 + tid; n < a.n_local; n += nblk * 256) {
        const int64_t o = a.off[n];
        const int64_t k = (int64_t)a.pos[n] + 1;
        if (k < 0 || k >= a.off[n + 1] - o) continue;
        bump(&a.occ[o + k], a.atomic);
    }
}

// The best rows of a long chain, behind gs_run_stats_kernel on the stream: the running
// best's sweep number is this sweep's exactly when this sweep won (the numbers of one call
// are distinct), else every workgroup returns at once.  1 024 targets a workgroup.
extern "C" __global__ void __launch_bounds__(256)
gs_run_stats_best_kernel(ChainStatsArgs a) {
    if (*a.err != 0 || *a.best_sweep != a.sweep) return;  // grid-uniform
    for (int n = blockIdx.x * 256 + threadIdx.x; n < a.n_local; n += gridDim.x * 256) {
        a.best_pos[n] = a.pos[n];
        a.best_pwms[n] = a.pwms[n];
    }
}

// bin_blocks workgroups over the targets' bins (none without occ), and one more in front
// for the sum when the trace or the best state is asked for; then, with copy_inline == 0,
// the launch that copies the best rows.
hipError_t gs_run_stats_launch(const ChainStatsArgs &a, int bin_blocks, hipStream_t s) {
    if (a.n_local <= 0) return hipSuccess;
    const int grid = (a.ic || a.best_sweep ? 1 : 0) + (a.occ ? bin_blocks : 0);
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_run_stats_kernel, dim3(grid), dim3(256), 0, s, a);
    if (a.best_sweep && !a.copy_inline)
        hipLaunchKernelGGL(gs_run_stats_best_kernel, dim3(std::min(1024, (a.n_local + 1023) / 1024)),
                           dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- Chain summaries (gs_occupancy_summary and the ..._summary run calls) ----
// The reduction of the bins a chain's statistics launches filled (or a caller uploaded) to
// what a caller keeps: each sequence's first-maximum bin with its count, and the count matrix
// summed over the counted states.  Two launches at most: gs_summary_pool_kernel decides which
// chains are pooled (only with the pooled outputs), gs_summary_kernel reads every row once.
namespace {

constexpr int kSumDepth = 4;  // wavefront loads of a row in flight ahead of the compares

// Whether (c2, i2) comes before (c1, i1): count descending, bin index ascending.
template <class T>
__device__ __forceinline__ bool mode_before(T c2, int i2, T c1, int i1) {
    return c2 > c1 || (c2 == c1 && i2 < i1);
}

// The first maximum over the 64 lanes' (count, smallest index with it), in every lane.
template <class T>
__device__ __forceinline__ void wave_first_max(T &cnt, int &idx) {
    for (int o = 32; o >= 1; o >>= 1) {
        const T c2 = __shfl_xor(cnt, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (mode_before(c2, i2, cnt, idx)) {
            cnt = c2;
            idx = i2;
        }
    }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The count matrix of a workgroup's rows (gs_summary_kernel and gs_list_summary_kernel): an LDS
// copy of 64-bit cells, [A * W] C then [A] T, zeroed by cells_clear, filled a bin at a time by
// cells_bin and a row at a time by cells_row, and added to the chain's and the pooled cells
// by cells_flush.  A cell holds at most the sum of a workgroup's bins, each below 2^31, far
// below 2^63.
__device__ __forceinline__ void cells_clear(unsigned long long *cell, int cells) {
    for (int i = threadIdx.x; i < cells; i += 256) cell[i] = 0;
    __syncthreads();
}

// Bin b >= 1 (start b - 1 <= L - W: the window stays inside the sequence) with count x: x to
// the W cells [s[b - 1 + j]][j], symbols outside the alphabet skipped as the sweeps' fold skips
// them, and to the row's sum S.  A zero bin and bin 0 add nothing.
__device__ __forceinline__ void cells_bin(unsigned long long *cell, const uint8_t *s, int b,
                                          int32_t x, int A, int W, long long &S) {
    if (x == 0 || b == 0) return;
    const unsigned long long c = (unsigned long long)(long long)x;
    S += x;
    // (the window's symbols eight loads at a time, so that the adds wait for a round trip a
    // chunk and not one a symbol; j < W keeps every load inside it)
    for (int j0 = 0; j0 < W; j0 += 8) {
        int sy[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) sy[i] = j0 + i < W ? s[b - 1 + j0 + i] : A;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (sy[i] < A) atomicAdd(&cell[sy[i] * W + j0 + i], c);
    }
}

// The row's share of T, by its wavefront: S comp[a] over the lanes' sums S of bins 1.. .
__device__ __forceinline__ void cells_row(unsigned long long *cell, const int32_t *comp,
                                          long long S, int lane, int A, int AW) {
    S = wave_sum_i64(S);
    if (S != 0 && lane < A)
        atomicAdd(&cell[AW + lane], (unsigned long long)(S * (long long)comp[lane]));
}

// The workgroup's cells, T[a] less the sum of its row of C (T_n[a] = S_n comp_n[a] -
// sum_j C_n[a][j]), every non-zero one by one 64-bit atomic add to the chain's cells (counts,
// nullable) and to the pooled ones (pool_counts, nullable).
__device__ __forceinline__ void cells_flush(const unsigned long long *cell, int A, int W,
                                            int64_t *counts, int64_t *pool_counts) {
    const int AW = A * W;
    __syncthreads();
    for (int i = threadIdx.x; i < AW + A; i += 256) {
        unsigned long long val = cell[i];
        if (i >= AW)
            for (int j = 0; j < W; ++j) val -= cell[(i - AW) * W + j];
        if (val == 0) continue;
        if (counts) atomicAdd((unsigned long long *)&counts[i], val);
        if (pool_counts) atomicAdd((unsigned long long *)&pool_counts[i], val);
    }
}

// The pooled view, one wavefront a sequence: the first maximum of the pooled chains' bins
// summed in int64.  Lane l takes the bins l, l + 64, .. of the row in increasing order, so a
// strict comparison keeps its first; no pooled chain leaves every sum 0, i.e. (-1, 0).
__device__ __forceinline__ void summary_pooled_rows(const SummaryArgs &a, int blk, int nblk) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int n = blk * 4 + w; n < a.n_local; n += nblk * 4) {
        const int64_t o = a.off[n];
        const int len = (int)(a.off[n + 1] - o);
        long long best = LLONG_MIN;
        int bidx = INT_MAX;
        for (int base = 0; base < len; base += 64 * kSumDepth) {
            long long x[kSumDepth];
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) x[k] = 0;
            for (int r = 0; r < a.n_chains; ++r) {
                if (!a.flags[r]) continue;  // wavefront-uniform
                const int32_t *row = a.occ + (int64_t)r * a.H + o;
#pragma unroll
                for (int k = 0; k < kSumDepth; ++k) {
                    const int b = base + lane + 64 * k;
                    x[k] += b < len ? row[b] : 0;
                }
            }
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) {
                const int b = base + lane + 64 * k;
                if (b < len && x[k] > best) {
                    best = x[k];
                    bidx = b;
                }
            }
        }
        wave_first_max(best, bidx);
        if (lane == 0) {
            a.pool_pos[n] = bidx - 1;
            a.pool_count[n] = best;
        }
    }
}

}  // namespace

// One workgroup a chain: whether the bins of local sequence 0 sum to n_counted
// (ChainStats.finished), and the number of such chains.
extern "C" __global__ void __launch_bounds__(256)
gs_summary_pool_kernel(SummaryArgs a) {
    __shared__ long long part[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t o = a.off[0];
    const int len = (int)(a.off[1] - o);
    const int32_t *row = a.occ + (int64_t)r * a.H + o;
    long long s = 0;
    for (int b = tid; b < len; b += 256) s += row[b];
    s = wave_sum_i64(s);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        const int f = part[0] + part[1] + part[2] + part[3] == a.n_counted ? 1 : 0;
        a.flags[r] = f;
        if (f) atomicAdd(a.n_pooled, 1);
    }
}

// gridDim.x / views workgroups a view: view v < n_chains is chain v, view n_chains (only with
// the pooled outputs) the pooled modes.  A chain's view, one wavefront a
// (chain, sequence) row, every row read once in coalesced wavefront loads, kSumDepth of them
// issued ahead of the compares; a bin index is checked against the row's length before its
// load.  Mode: lane l keeps (maximum, first index) over the bins l, l + 64, ..; the cross-lane
// step orders by (count descending, index ascending).  Counts (asked for, or the chain is
// pooled): a non-zero bin 1 + k with count c adds c to the W cells [s[k + j]][j] of the
// workgroup's LDS copy (64-bit cells: a cell holds at most the sum of a workgroup's bins, each
// below 2^31, far below 2^63), symbols outside the alphabet skipped as the sweeps' fold skips
// them; per row S = the sum of its bins 1.., and S comp[n][a] goes to the copy's T cell a.
// At the end T[a] loses the sum of its row of C (T_n[a] = S_n comp_n[a] - sum_j C_n[a][j]) and
// every non-zero cell goes to the chain's cells, and for a pooled chain to the pooled ones, by
// one 64-bit atomic add each.  Integer adds: the result does not depend on their order.  No
// workgroup waits on another.  Negative bins are the caller's error: nothing is indexed by a
// bin's value, so no access depends on them.
extern "C" __global__ void __launch_bounds__(256)
gs_summary_kernel(SummaryArgs a) {
    extern __shared__ unsigned long long cell[];  // [A * W] C, then [A] T
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nblk = gridDim.x / (a.n_chains + (a.flags ? 1 : 0));
    const int v = blockIdx.x / nblk, blk = blockIdx.x - v * nblk;
    if (v == a.n_chains) {  // workgroup-uniform
        summary_pooled_rows(a, blk, nblk);
        return;
    }
    const int A = a.A, W = a.W, AW = A * W, cells = AW + A;
    const bool pooled = a.flags && a.flags[v] != 0;
    const bool want_cells = a.counts || pooled, want_mode = a.mode_pos != nullptr;
    if (!want_cells && !want_mode) return;
    if (want_cells) cells_clear(cell, cells);
    const int32_t *occ = a.occ + (int64_t)v * a.H;
    for (int n = blk * 4 + w; n < a.n_local; n += nblk * 4) {
        const int64_t o = a.off[n];
        const int len = (int)(a.off[n + 1] - o);  // 1 + (L - W + 1) bins
        const int32_t *row = occ + o;
        const uint8_t *s = a.seq + a.doff[n];
        int best = INT_MIN, bidx = INT_MAX;
        long long S = 0;
        for (int base = 0; base < len; base += 64 * kSumDepth) {
            int32_t x[kSumDepth];
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) {
                const int b = base + lane + 64 * k;
                x[k] = b < len ? row[b] : 0;
            }
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) {
                const int b = base + lane + 64 * k;
                if (b >= len) continue;
                if (x[k] > best) {
                    best = x[k];
                    bidx = b;
                }
                if (want_cells) cells_bin(cell, s, b, x[k], A, W, S);
            }
        }
        if (want_mode) {
            wave_first_max(best, bidx);
            if (lane == 0) {
                a.mode_pos[(int64_t)v * a.n_local + n] = bidx - 1;
                a.mode_count[(int64_t)v * a.n_local + n] = best;
            }
        }
        if (want_cells) cells_row(cell, a.comp + (int64_t)n * a.CS, S, lane, A, AW);
    }
    if (!want_cells) return;
    cells_flush(cell, A, W, a.counts ? a.counts + (int64_t)v * cells : nullptr,
                pooled ? a.pool_counts : nullptr);
}

// The pooled outputs go together (flags, n_pooled, pool_*): first the launch that decides the
// pool, then blocks workgroups a view over the chains' views and the pooled one.  The cells
// (counts, pool_counts) and n_pooled are zero at launch.
hipError_t gs_summary_launch(const SummaryArgs &a, int blocks, hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    if (a.flags)
        hipLaunchKernelGGL(gs_summary_pool_kernel, dim3(a.n_chains), dim3(256), 0, s, a);
    const size_t lds = (size_t)(a.A * a.W + a.A) * 8;
    hipLaunchKernelGGL(gs_summary_kernel, dim3(blocks * (a.n_chains + (a.flags ? 1 : 0))),
                       dim3(256), lds, s, a);
    return hipGetLastError();
}

// ---- List summaries (gs_list_occupancy_summary and gs_motif_run_multi_batch_summary, DESIGN.md
// §9.29) ----
// The reduction of the bins and site counts of Positions-list chains (the statistics launches
// of §9.26 filled them, or a caller uploaded them) to what ListChainStats.mode() and a count
// matrix keep: per sequence the modal site count c*, then c* rounds that each take the most
// occupied start (the first among equals) not within W of a start already taken
// (ceckForDistance, .fs:129-140), in ascending order; and the cells of §9.28, which are the
// list aggregates' sum.  Two launches at most: gs_list_summary_pool_kernel decides which chains
// are pooled (only with the pooled outputs), gs_list_summary_kernel reduces every row.
namespace {

// Bins of a row a wavefront keeps in LDS for its rounds (a longer row is read again a round)
constexpr int kListStageBins = 512;

template <class T>
__device__ __forceinline__ constexpr T list_lowest() {
    return sizeof(T) == 4 ? (T)INT_MIN : (T)LLONG_MIN;
}

// kSumDepth wavefront loads of a view's row from bin `base` on, all issued ahead of their use:
// chain v's bins (T = int32_t), or for the pooled view (T = int64_t) the pooled chains' bins
// summed in int64.  A bin index is checked against the row's length before its load.
template <class T>
__device__ __forceinline__ void list_load(const ListSummaryArgs &a, int v, int64_t o, int len,
                                          int base, int lane, T (&x)[kSumDepth]) {
    if constexpr (sizeof(T) == 4) {
        const int32_t *row = a.occ + (int64_t)v * a.H + o;
#pragma unroll
        for (int k = 0; k < kSumDepth; ++k) {
            const int b = base + lane + 64 * k;
            x[k] = b < len ? row[b] : 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kSumDepth; ++k) x[k] = 0;
        for (int r = 0; r < a.n_chains; ++r) {
            if (!a.flags[r]) continue;  // wavefront-uniform
            const int32_t *row = a.occ + (int64_t)r * a.H + o;
            // (every load issued, at an index clamped into the row, and the value past the end
            // dropped where it is added: a branch around a load makes the widening of its
            // value, and so the wait, part of the branch, one round trip a load)
            int32_t y[kSumDepth];
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) y[k] = row[min(base + lane + 64 * k, len - 1)];
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) x[k] += base + lane + 64 * k < len ? y[k] : 0;
        }
    }
}

// visit(b, x) for every bin b of the row with its count x: lane l sees the bins l, l + 64, ..
// in increasing order.
template <class T, class F>
__device__ __forceinline__ void list_scan(const ListSummaryArgs &a, int v, int64_t o, int len,
                                          int lane, F visit) {
    for (int base = 0; base < len; base += 64 * kSumDepth) {
        T x[kSumDepth];
        list_load(a, v, o, len, base, lane, x);
#pragma unroll
        for (int k = 0; k < kSumDepth; ++k) {
            const int b = base + lane + 64 * k;
            if (b < len) visit(b, x[k]);
        }
    }
}

// One (view, sequence) row by one wavefront.  The row is read once: every bin goes to the
// workgroup's cells (cell non-null: a chain's view that wants them) and, when the row fits,
// into the wavefront's LDS stage, bin b by the lane b mod 64 that reads it again in the
// rounds, so that no lane reads what another wrote.  The site counts: lane l <= M holds
// count l, the first maximum across the wavefront is c*.  A round: every lane keeps the
// first maximum over its free starts, the wavefront takes the first maximum of those; lane i
// keeps the i-th start taken and its count, and a start is free when it is more than W from
// every one of them, read by a uniform-index lane read.  The rounds end when no lane has a
// free start.  At the end lane i ranks its start among those taken and writes it there.
// Nothing is indexed by a bin's or a site count's value.
template <class T>
__device__ __forceinline__ void list_row(const ListSummaryArgs &a, int v, int n, int lane,
                                         T *stage, unsigned long long *cell, int32_t *o_sites,
                                         T *o_sites_count, int32_t *o_cnt, int32_t *o_pos,
                                         T *o_count) {
    const int64_t o = a.off[n];
    const int len = (int)(a.off[n + 1] - o);  // 1 + (L - W + 1) bins
    const int M = a.M, W = a.W;
    const bool fits = len <= kListStageBins, want_mode = o_sites != nullptr;
    if (cell || (fits && want_mode)) {
        const uint8_t *s = a.seq + a.doff[n];
        long long S = 0;
        list_scan<T>(a, v, o, len, lane, [&](int b, T x) {
            if (fits) stage[b] = x;
            if constexpr (sizeof(T) == 4)
                if (cell) cells_bin(cell, s, b, x, a.A, W, S);
        });
        if constexpr (sizeof(T) == 4)
            if (cell) cells_row(cell, a.comp + (int64_t)n * a.CS, S, lane, a.A, a.A * W);
    }
    if (!want_mode) return;
    // the modal site count
    T sc = list_lowest<T>();
    int si = INT_MAX;
    if (lane <= M) {
        si = lane;
        if constexpr (sizeof(T) == 4) {
            sc = a.sites[((int64_t)v * a.n_local + n) * (M + 1) + lane];
        } else {
            sc = 0;
            for (int r = 0; r < a.n_chains; ++r)
                if (a.flags[r]) sc += a.sites[((int64_t)r * a.n_local + n) * (M + 1) + lane];
        }
    }
    wave_first_max(sc, si);
    const int cstar = __builtin_amdgcn_readfirstlane(si);
    // the rounds
    int taken = 0, ntaken = 0;  // lane i < ntaken: the i-th start taken, and its count
    T tcount = 0;
    for (int round = 0; round < cstar; ++round) {
        T best = list_lowest<T>();
        int bidx = INT_MAX;
        const auto cand = [&](int b, T x) {
            if (b == 0) return;
            const int k = b - 1;
            bool is_free = true;
            for (int q = 0; q < ntaken; ++q) {
                const int d = k - __builtin_amdgcn_readlane(taken, q);
                is_free = is_free && (d > W || d < -W);
            }
            if (is_free && (bidx == INT_MAX || x > best)) {
                best = x;
                bidx = k;
            }
        };
        if (fits) {
            for (int b = lane; b < len; b += 64) cand(b, stage[b]);
        } else {
            list_scan<T>(a, v, o, len, lane, cand);
        }
        wave_first_max(best, bidx);
        if (__builtin_amdgcn_readfirstlane(bidx) == INT_MAX) break;  // every start excluded
        if (lane == ntaken) {
            taken = bidx;
            tcount = best;
        }
        ++ntaken;
    }
    // ascending starts: the rank of a lane's start among the (distinct) starts taken
    int rank = 0;
    for (int q = 0; q < ntaken; ++q) rank += __builtin_amdgcn_readlane(taken, q) < taken ? 1 : 0;
    if (lane == 0) {
        o_sites[n] = cstar;
        o_sites_count[n] = sc;
        o_cnt[n] = ntaken;
    }
    if (lane < M) {
        const bool t = lane < ntaken;
        const int64_t slot = (int64_t)n * M + (t ? rank : lane);
        o_pos[slot] = t ? taken : -1;
        o_count[slot] = t ? tcount : (T)0;
    }
}

}  // namespace

// One workgroup a chain: whether every sequence's site counts sum to n_counted
// (ListChainStats.finished), and the number of such chains.
extern "C" __global__ void __launch_bounds__(256)
gs_list_summary_pool_kernel(ListSummaryArgs a) {
    __shared__ int short_rows;
    const int r = blockIdx.x, tid = threadIdx.x, m1 = a.M + 1;
    if (tid == 0) short_rows = 0;
    __syncthreads();
    const int32_t *sites = a.sites + (int64_t)r * a.n_local * m1;
    bool bad = false;
    for (int n = tid; n < a.n_local; n += 256) {
        long long s = 0;
        for (int i = 0; i < m1; ++i) s += sites[(int64_t)n * m1 + i];
        bad = bad || s != a.n_counted;
    }
    if (bad) atomicOr(&short_rows, 1);
    __syncthreads();
    if (tid == 0) {
        const int f = short_rows ? 0 : 1;
        a.flags[r] = f;
        if (f) atomicAdd(a.n_pooled, 1);
    }
}

// gridDim.x / views workgroups a view, as gs_summary_kernel: view v < n_chains is chain v, view
// n_chains (only with the pooled outputs) the pooled one, whose bins and site counts are the
// pooled chains' summed in int64 (once, into the stage, when the row fits).  One wavefront a
// (view, sequence) row (list_row).  A chain's view also fills the workgroup's cells
// (cells_bin / cells_row / cells_flush: gs_summary_kernel's arithmetic) when its counts are
// asked for or the chain is pooled.  Dynamic LDS: the cells, then kListStageBins 64-bit
// entries a wavefront.  Integer sums only; no workgroup waits on another.
extern "C" __global__ void __launch_bounds__(256)
gs_list_summary_kernel(ListSummaryArgs a) {
    extern __shared__ unsigned long long cell[];  // [A * W] C, [A] T, then the four stages
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nblk = gridDim.x / (a.n_chains + (a.flags ? 1 : 0));
    const int v = blockIdx.x / nblk, blk = blockIdx.x - v * nblk;
    const int cells = a.A * a.W + a.A;
    int64_t *stage = (int64_t *)(cell + cells) + w * kListStageBins;
    if (v == a.n_chains) {  // workgroup-uniform
        for (int n = blk * 4 + w; n < a.n_local; n += nblk * 4)
            list_row<int64_t>(a, v, n, lane, stage, nullptr, a.pool_sites, a.pool_sites_count,
                              a.pool_cnt, a.pool_pos, a.pool_count);
        return;
    }
    const bool pooled = a.flags && a.flags[v] != 0;
    const bool want_cells = a.counts || pooled, want_mode = a.mode_sites != nullptr;
    if (!want_cells && !want_mode) return;
    if (want_cells) cells_clear(cell, cells);
    const int64_t vrow = (int64_t)v * a.n_local;
    for (int n = blk * 4 + w; n < a.n_local; n += nblk * 4)
        list_row<int32_t>(a, v, n, lane, (int32_t *)stage, want_cells ? cell : nullptr,
                          want_mode ? a.mode_sites + vrow : nullptr, a.mode_sites_count + vrow,
                          a.mode_cnt + vrow, a.mode_pos + vrow * a.M, a.mode_count + vrow * a.M);
    if (want_cells)
        cells_flush(cell, a.A, a.W, a.counts ? a.counts + (int64_t)v * cells : nullptr,
                    pooled ? a.pool_counts : nullptr);
}

// As gs_summary_launch: the pooled outputs go together, the cells and n_pooled are zero at
// launch.
hipError_t gs_list_summary_launch(const ListSummaryArgs &a, int blocks, hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    if (a.flags)
        hipLaunchKernelGGL(gs_list_summary_pool_kernel, dim3(a.n_chains), dim3(256), 0, s, a);
    const size_t lds = (size_t)(a.A * a.W + a.A) * 8 + (size_t)4 * kListStageBins * 8;
    hipLaunchKernelGGL(gs_list_summary_kernel, dim3(blocks * (a.n_chains + (a.flags ? 1 : 0))),
                       dim3(256), lds, s, a);
    return hipGetLastError();
}

// ---- Chain agreement (gs_occupancy_agreement and gs_motif_run_batch_agreement, DESIGN.md
// §9.31) ----
// Whether pooling the chains was justified: with P pooled chains and pool[b] the sum of their
// bins in int64, D(r, n) = the sum over the bins b of sequence n's row of |P occ[r][b] -
// pool[b]| (for chains that finished, 2 P n_counted times the total variation distance between
// chain r's marginal of the sequence and the pooled one); m(r, n) and m*(n) are the first
// maxima of the chain's and of the pooled row, as gs_summary_kernel takes them.  One launch
// behind the launch that decides the pool, unless the flags are already there (a summary's of
// the same call, or the caller's mask).
namespace {

constexpr int kAgrStageBins = kListStageBins;  // bins of a pooled row a wavefront keeps in LDS
constexpr int kAgrLdsChains = 512;             // chains whose sums a workgroup collects in LDS

// kSumDepth wavefront loads of the pooled row from bin `base` on: the pooled chains' bins
// summed in int64.  Every load is issued, at an index clamped into the row, and the value past
// the end dropped where it is added (list_load's reason).
__device__ __forceinline__ void agr_pool_load(const AgreementArgs &a, int64_t o, int len, int base,
                                              int lane, long long (&x)[kSumDepth]) {
#pragma unroll
    for (int k = 0; k < kSumDepth; ++k) x[k] = 0;
    for (int r = 0; r < a.n_chains; ++r) {
        if (!a.flags[r]) continue;  // wavefront-uniform
        const int32_t *row = a.occ + (int64_t)r * a.H + o;
        int32_t y[kSumDepth];
#pragma unroll
        for (int k = 0; k < kSumDepth; ++k) y[k] = row[min(base + lane + 64 * k, len - 1)];
#pragma unroll
        for (int k = 0; k < kSumDepth; ++k) x[k] += base + lane + 64 * k < len ? y[k] : 0;
    }
}

}  // namespace

// One wavefront a sequence row, four a workgroup; lane l owns the bins l, l + 64, .. in
// increasing order, kSumDepth coalesced wavefront loads issued ahead of their use, every bin
// index clamped into the row before its load.  Phase A: the pooled row, its first maximum m*,
// and, when the row has at most kAgrStageBins bins, the row into the wavefront's LDS stage, bin
// b by the lane b mod 64 that reads it again, so that no lane reads what another wrote (a
// longer row is summed again a chunk in phase B).  Phase B, per pooled chain in increasing r:
// the chain's first maximum and D; the running largest D by a strict comparison, so the lowest
// r keeps it.  A chain's D and agreement go to the workgroup's LDS accumulators, and every
// non-zero one to the chain's sums by one atomic add at the workgroup's end (more than
// kAgrLdsChains chains: straight to global memory).  Integer adds: the result does not depend
// on their order.  A chain that is not pooled gets (-1, -1) from workgroup 0; nothing is added
// to it.  No workgroup waits on another.  Negative bins are the caller's error: nothing is
// indexed by a bin's value, so no access depends on them.
extern "C" __global__ void __launch_bounds__(256)
gs_agreement_kernel(AgreementArgs a) {
    extern __shared__ unsigned long long agr_lds[];  // four stages, the chains' D, their agreement
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int R = a.n_chains;
    long long *stage = (long long *)agr_lds + w * kAgrStageBins;
    unsigned long long *acc_d = agr_lds + 4 * kAgrStageBins;
    unsigned int *acc_a = (unsigned int *)(acc_d + kAgrLdsChains);
    const bool in_lds = R <= kAgrLdsChains;  // grid-uniform
    if (in_lds) {
        for (int r = tid; r < R; r += 256) {
            acc_d[r] = 0;
            acc_a[r] = 0;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0)
        for (int r = tid; r < R; r += 256)
            if (!a.flags[r]) {
                a.chain_dist[r] = -1;
                a.chain_agree[r] = -1;
            }
    int P = 0;
    for (int r = lane; r < R; r += 64) P += a.flags[r] != 0 ? 1 : 0;
    P = (int)wave_sum_i64(P);
    for (int n = blockIdx.x * 4 + w; n < a.n_local; n += gridDim.x * 4) {
        const int64_t o = a.off[n];
        const int len = (int)(a.off[n + 1] - o);  // 1 + (L - W + 1) bins
        if (len <= 0) continue;
        const bool fits = len <= kAgrStageBins;
        // ---- phase A: the pooled row and its first maximum ----
        long long best = LLONG_MIN;
        int bidx = INT_MAX;
        for (int base = 0; base < len; base += 64 * kSumDepth) {
            long long x[kSumDepth];
            agr_pool_load(a, o, len, base, lane, x);
#pragma unroll
            for (int k = 0; k < kSumDepth; ++k) {
                const int b = base + lane + 64 * k;
                if (b >= len) continue;
                if (fits) stage[b] = x[k];
                if (x[k] > best) {
                    best = x[k];
                    bidx = b;
                }
            }
        }
        wave_first_max(best, bidx);  // m* = bidx, in every lane
        // ---- phase B: every pooled chain against the pool ----
        long long maxd = -1;
        int argr = -1, agree = 0;
        for (int r = 0; r < R; ++r) {
            if (!a.flags[r]) continue;  // wavefront-uniform
            const int32_t *row = a.occ + (int64_t)r * a.H + o;
            int cbest = INT_MIN, cidx = INT_MAX;
            long long d = 0;
            for (int base = 0; base < len; base += 64 * kSumDepth) {
                int32_t y[kSumDepth];
                long long pv[kSumDepth];
#pragma unroll
                for (int k = 0; k < kSumDepth; ++k) y[k] = row[min(base + lane + 64 * k, len - 1)];
                if (fits) {
#pragma unroll
                    for (int k = 0; k < kSumDepth; ++k) {
                        const int b = base + lane + 64 * k;
                        pv[k] = b < len ? stage[b] : 0;
                    }
                } else {
                    agr_pool_load(a, o, len, base, lane, pv);
                }
#pragma unroll
                for (int k = 0; k < kSumDepth; ++k) {
                    const int b = base + lane + 64 * k;
                    if (b >= len) continue;
                    if (y[k] > cbest) {
                        cbest = y[k];
                        cidx = b;
                    }
                    const long long t = (long long)P * y[k] - pv[k];
                    d += t < 0 ? -t : t;
                }
            }
            wave_first_max(cbest, cidx);
            d = wave_sum_i64(d);
            const bool same = cidx == bidx;
            agree += same ? 1 : 0;
            if (d > maxd) {
                maxd = d;
                argr = r;
            }
            if (lane == 0) {
                if (in_lds) {
                    if (d != 0) atomicAdd(&acc_d[r], (unsigned long long)d);
                    if (same) atomicAdd(&acc_a[r], 1u);
                } else {
                    if (d != 0)
                        atomicAdd((unsigned long long *)&a.chain_dist[r], (unsigned long long)d);
                    if (same) atomicAdd(&a.chain_agree[r], 1);
                }
            }
        }
        if (lane == 0) {
            a.agree[n] = agree;
            a.spread[n] = argr >= 0 ? maxd : 0;
            a.spread_chain[n] = argr;
        }
    }
    if (!in_lds) return;
    __syncthreads();
    for (int r = tid; r < R; r += 256) {
        if (acc_d[r] != 0) atomicAdd((unsigned long long *)&a.chain_dist[r], acc_d[r]);
        if (acc_a[r] != 0) atomicAdd(&a.chain_agree[r], (int)acc_a[r]);
    }
}

// With a.decide first the launch that decides the pool by the summaries' rule
// (gs_summary_pool_kernel: flags and n_pooled, which is zero at launch); then `blocks`
// workgroups over the sequence rows.  chain_agree and chain_dist are zero at launch.
hipError_t gs_agreement_launch(const AgreementArgs &a, int blocks, hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    if (a.decide) {
        SummaryArgs p{};
        p.n_chains = a.n_chains;
        p.n_local = a.n_local;
        p.H = a.H;
        p.n_counted = a.n_counted;
        p.occ = a.occ;
        p.off = a.off;
        p.flags = a.flags;
        p.n_pooled = a.n_pooled;
        hipLaunchKernelGGL(gs_summary_pool_kernel, dim3(a.n_chains), dim3(256), 0, s, p);
    }
    const size_t lds = (size_t)4 * kAgrStageBins * 8 + (size_t)kAgrLdsChains * 12;
    hipLaunchKernelGGL(gs_agreement_kernel, dim3(blocks), dim3(256), lds, s, a);
    return hipGetLastError();
}
