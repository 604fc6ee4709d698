// gs_bgwalk.h — the ratio-table walk over a packed target's background categories,
// shared by gs_sweep_bg.hip (every target) and gs_sweep_dna.hip (a wavefront whose
// lanes all skipped the motif scan): G_k = prod_j PCV[s_{k+j}] (.fs:123-124,
// .fs:759-784) by incremental binary64 products, g_k = g_{k-1} R[s_{k-1+W}][s_{k-1}]
// from a per-lane ratio table R[i][o] = PCV[i] (1 / PCV[o]) in LDS ([16 rows][64
// lanes], a lane's row r at rt[64 r]: the 64 lanes of a read hit 64 distinct banks),
// the lane's first window pcv[0]^W times its rows (s_j, 0).  Each g_k is within
// bg_walk_rel_err(W, K) (gs_common.h) of the reference's fold.  Here: the table
// build, the 16-window block, the first pass's visitor and the choice of the second
// pass's start among the first's 8 chunk sums.  The loops over a target's words
// (their sources differ: global memory, staged LDS words) and the certification
// margins (they differ by caller) stay with the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "gs_common.h"

namespace gs {

// row i + 4 o = pcv[i] (1 / pcv[o])
__device__ __forceinline__ void bg_ratio_table(double *rt, const double (&pcv)[4]) {
    double inv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) inv[e] = 1.0 / pcv[e];
#pragma unroll
    for (int c = 0; c < 16; ++c) rt[c * 64] = pcv[c & 3] * inv[c >> 2];
}

// Walk visitors (state by value: lambdas capturing locals by reference left them in
// scratch): blk(t) at the start of each 16-window block (t relative to the walk's
// first window), blkw(w1, w2) with the block's words where the walk has them, win(k,
// g) for every window in order; a lane leaves once win returns true.
// Pass 1: the lane's sum and its value at the starts of 8 chunks of Cz windows
// (whole 16-window blocks).
struct BgSum {
    double B, pre[8];
    int ci, nck, Cz;
    __device__ __forceinline__ void blk(int t) {
        if (t == nck) {
#pragma unroll
            for (int i = 0; i < 8; ++i) pre[i] = i == ci ? B : pre[i];
            ++ci;
            nck += Cz;
        }
    }
    static constexpr bool kStops = false;  // never ends a walk early
    __device__ __forceinline__ void blkw(uint32_t, uint32_t) {}
    __device__ __forceinline__ bool win(int, double g) {
        B = B + g;
        return false;
    }
};
// (Pass 2's visitors stay with the kernels: gs_sweep_bg.hip's keeps the block's words
// and the found window's symbols, gs_sweep_dna.hip's does not.  One struct for both
// with the words grew every dna kernel by 457 instructions; the words in a struct
// derived from a shared one moved gs_sweep_bg_kernel<8> and <16> from 32 and 34
// spilled SGPRs to 39 and 41.)

// One 16-window block: nw / ow the symbols entering / leaving its windows.  The 16
// table reads are issued before the first product (a product a window waited for its
// read otherwise); FULL: every window of the block is in the lane's range.
template <bool FULL, class V>
__device__ __forceinline__ void bg_walk_block(double &g, bool &done, uint32_t nw, uint32_t ow, int b,
                                              int nwin, int x0, const double *rt, V &v) {
    double r[16];
#pragma unroll
    for (int R = 0; R < 16; ++R) {
        const uint32_t ci = __builtin_amdgcn_ubfe(nw, 2 * R, 2), co = __builtin_amdgcn_ubfe(ow, 2 * R, 2);
        r[R] = rt[(ci | (co << 2)) * 64];
    }
#pragma unroll
    for (int R = 0; R < 16; ++R) {
        if (R > 0 || b > 0) g = g * r[R];
        if constexpr (V::kStops) {
            if (!done && (FULL || b + R < nwin)) done = v.win(x0 + b + R, g);
        } else {
            if (FULL || b + R < nwin) v.win(x0 + b + R, g);
        }
    }
}

// The second pass starts at the last of pass 1's 8 chunk starts (chunks of Cz windows,
// nb in the lane's range) whose running sum, with the lane's prefix Bpre, lies below
// Tb: returns the chunk, P its running sum.
__device__ __forceinline__ int bg_chunk_start(const double (&pre)[8], int Cz, int nb, double Bpre, double Tb,
                                              double &P) {
    int cst = 0;
    P = Bpre;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const bool in = i * Cz < nb && Bpre + pre[i] < Tb;
        cst = in ? i : cst;
        P = in ? Bpre + pre[i] : P;
    }
    return cst;
}

}  // namespace gs
