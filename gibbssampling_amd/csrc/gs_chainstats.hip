// gs_chainstats.hip — the device-side consumer of a chain batch's sweeps
// (gs_motif_run_batch_stats): per counted sweep one launch, stream-ordered
// right after that sweep's gs_run_batch_sweep_kernel, which left the chains' positions and
// PWMS rows and their skip words.
#include "gs_ctx.h"
#include "gs_wave.h"

// gridDim.x / n_chains workgroups a chain.  A chain whose skip word is set contributes
// nothing (its trace entry is a quiet NaN).  Workgroup 0 of a chain: wavefront 0 forms the
// ordered sum of the PWMS row, which the workgroup stages through LDS (64 lane-strided serial
// sums from +0.0, then the halving tree
// v[l] += v[l + s], s = 32 .. 1), writes the trace entry and decides against the running
// best (the first counted sweep is taken; later ones only when strictly larger, .fs:989; a
// NaN never wins); on a win the whole workgroup copies the two rows into the best slabs.
// All workgroups: one to bin off[n] + 1 + pos[n] of the chain's histogram for their share
// of the targets.  A chain's bins of one sweep are distinct and launches are stream-ordered,
// so the plain read-modify-write (a.atomic == 0) and the non-returning atomic add race with
// nothing; a position outside [-1, L - W] is not counted.
extern "C" __global__ void __launch_bounds__(256)
gs_run_batch_stats_kernel(RunStatsArgs a) {
    constexpr int kChunk = 2048;
    __shared__ double buf[kChunk];
    __shared__ int win;
    const int tid = threadIdx.x;
    const int bpc = gridDim.x / a.n_chains;
    const int r = blockIdx.x / bpc, blk = blockIdx.x - r * bpc;
    const bool skipped = a.skip[r] != 0;  // workgroup-uniform
    const int64_t row = (int64_t)r * a.n_local;
    const bool sums = a.ic || a.best_sweep;
    if (blk == 0 && sums && skipped && tid == 0 && a.ic)
        a.ic[(int64_t)r * a.ic_stride] = __longlong_as_double(0x7ff8000000000000ll);
    if (skipped) return;
    if (blk == 0 && sums) {
        if (tid == 0) win = 0;
        // the row through LDS, kChunk entries at a time (a multiple of 64: lane l keeps
        // n = l mod 64): the whole workgroup's loads are in flight at once, and the
        // serial adds of wavefront 0 wait on LDS only (10 000 targets: a launch measured
        // 15 us against 40 with wavefront 0 reading global memory)
        double v = 0.0;
        for (int base = 0; base < a.n_local; base += kChunk) {
            const int m = min(kChunk, a.n_local - base);
            __syncthreads();
            for (int i = tid; i < m; i += 256) buf[i] = a.pwms[row + base + i];
            __syncthreads();
            if (tid < 64)
                for (int i = tid; i < m; i += 64) v = v + buf[i];
        }
        if (tid < 64) {
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
            if (tid == 0) {
                if (a.ic) a.ic[(int64_t)r * a.ic_stride] = v;
                if (a.best_sweep && (a.best_sweep[r] < 0 || v > a.best_ic[r])) {
                    a.best_sweep[r] = a.sweep;
                    a.best_ic[r] = v;
                    win = 1;
                }
            }
        }
        __syncthreads();
        if (win)
            for (int n = tid; n < a.n_local; n += 256) {
                a.best_pos[row + n] = a.pos[row + n];
                a.best_pwms[row + n] = a.pwms[row + n];
            }
    }
    if (!a.occ) return;
    int32_t *occ = a.occ + (int64_t)r * a.H;
    for (int n = blk * 256 + tid; n < a.n_local; n += bpc * 256) {
        const int64_t o = a.off[n];
        const int64_t k = (int64_t)a.pos[row + n] + 1;
        if (k < 0 || k >= a.off[n + 1] - o) continue;
        if (a.atomic)
            atomicAdd(&occ[o + k], 1);
        else
            occ[o + k] += 1;
    }
}

hipError_t gs_run_batch_stats_launch(const RunStatsArgs &a, int blocks_per_chain, hipStream_t s) {
    if (a.n_local <= 0 || a.n_chains <= 0) return hipSuccess;
    hipLaunchKernelGGL(gs_run_batch_stats_kernel, dim3(a.n_chains * blocks_per_chain), dim3(256), 0,
                       s, a);
    return hipGetLastError();
}
