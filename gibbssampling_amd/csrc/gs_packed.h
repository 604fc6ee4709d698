// gs_packed.h — device helpers of the 2-bit packed sequence layout (16 symbols a
// word, alphabets of at most 4 symbols), shared by the kernels that sweep it
// (gs_sweep_dna.hip, gs_sweep_live.hip and through it gs_sweep_long.hip,
// gs_sweep_bg.hip): the packed int16 ring arithmetic, symbol counts and funnel shifts
// of packed words, the reference's PCV fold of a packed window, and rescan_packed, the
// exact binary64 rescan of one packed target by a whole wavefront (its pick is
// gs_pick.h exact_pick).
#pragma once
#include <hip/hip_runtime.h>

#include "gs_common.h"
#include "gs_fold.h"
#include "gs_pick.h"
#include "gs_wave.h"

namespace gs {

typedef short s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_add(uint32_t x, uint32_t y) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(s2, x) + __builtin_bit_cast(s2, y));
}

// The window completed by a ring step: low int16 of the register it was born in
// plus the high int16 of the register born 8 positions later, as a sign-extended
// int32 (one SDWA add: the sum of two entries of at most 4 x 4095 never wraps).
__device__ __forceinline__ int half_sum(uint32_t lo_reg, uint32_t hi_reg) {
    int r;
    asm("v_add_u16_sdwa %0, %1, %2 dst_sel:WORD_0 dst_unused:UNUSED_SEXT src0_sel:WORD_0 "
        "src1_sel:WORD_1"
        : "=v"(r)
        : "v"(lo_reg), "v"(hi_reg));
    return r;
}

// count of symbol e among the first W symbols of a packed word (wmask: 2W bits)
__device__ __forceinline__ int sym_count(uint32_t x, int e, uint32_t wmask) {
    const uint32_t y = ~(x ^ (0x55555555u * (uint32_t)e));
    return __popc(y & (y >> 1) & 0x55555555u & wmask);
}

__device__ __forceinline__ uint32_t funnel(uint32_t hi, uint32_t lo, int sh) {
    return __builtin_amdgcn_alignbit(hi, lo, (uint32_t)sh);
}

// The sweep's first error wins the code, the least global index the index (the
// pointers as the caller reads its kernel arguments).
__device__ __forceinline__ void raise_error(int32_t *err_code, unsigned long long *err_index, int code,
                                            int64_t gidx) {
    atomicCAS(err_code, 0, code);
    atomicMin(err_index, (unsigned long long)gidx);
}

__device__ __forceinline__ uint4 load_words(const uint32_t *p) {
    uint4 v;
    __builtin_memcpy(&v, p, 16);  // 4-byte aligned 16-byte load
    return v;
}

// Pair code * 16 of position P of a chunk whose words are ww[1..4], ww[0] the word
// before and ww[5] the first word of the next chunk (P < 64 + 14: ww[6] only
// feeds bits that are masked off).
template <int P>
__device__ __forceinline__ uint32_t pair16(const uint32_t (&ww)[7]) {
    constexpr int rr = P & 15, wi = (P >> 4) + 1;
    uint32_t v;
    if constexpr (rr >= 2)
        v = funnel(ww[wi + 1], ww[wi], 2 * rr - 4);
    else
        v = funnel(ww[wi], ww[wi - 1], 28 + 2 * rr);
    return v & 0xF0u;
}

// The reference's binary64 fold of a window's PCV factors (.fs:123-124), its W
// symbols at the low bits of wv.
__device__ __forceinline__ double fold_bits(uint32_t wv, int W, const double (&pcv)[4]) {
    double g = 1.0;
    for (int j = 0; j < W; ++j) {
        const uint32_t e = (wv >> (2 * j)) & 3u;
        g = g * (e == 0 ? pcv[0] : e == 1 ? pcv[1] : e == 2 ? pcv[2] : pcv[3]);
    }
    return g;
}

// The same for window k of the sequence at seqw.
__device__ __forceinline__ double fold_window(const uint32_t *seqw, int k, int W, const double (&pcv)[4]) {
    const uint32_t *q = seqw + (k >> 4);
    return fold_bits(funnel(q[1], q[0], 2 * (k & 15)), W, pcv);
}

// The 16 symbols of a packed word, one byte each.
__device__ __forceinline__ uint4 unpack_word(uint32_t v) {
    uint32_t d[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) x |= ((v >> (2 * (4 * t + b))) & 3u) << (8 * b);
        d[t] = x;
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// Exact binary64 rescan of target sq (wave-uniform) by the whole wavefront: the
// reference's folds for every window (.fs:759-777), the pick certified against
// rounding alone, else one lane replays the reference's sequential sums
// (.fs:747-754): exact_pick.  Writes pos_out / pwms_out (or raises the overrun error)
// and adds the new segment to the wavefront's aggregates.  Staging in the wavefront's
// slice: the unpacked sequence at seq_off, the (PWM, PCV) table at tab_off, 40 bytes of
// scratch (pcv[4], the pick's two ints) at misc_off.  The kernel arguments through
// `a`: the kernel's own by-value struct where the rescan is inlined into the kernel
// (ArgT = DnaArgs), the kernarg segment where it is called out of line (a function
// called out of line has no kernarg segment pointer of its own: the caller passes the
// segment, ArgT a constant-address-space DnaArgs, its fields scalar loads where used).
// mark(11..14): the phase ends of a caller that stamps them (gs_sweep_dna.hip).
template <int WM, class ArgT, class Marks = NoMarks>
__device__ __forceinline__ void rescan_packed(const ArgT &a, int sq, uint64_t rng_stream,
                                              unsigned char *wslice, int seq_off, int tab_off,
                                              int misc_off, const double2 *sPPM, const int64_t *sT,
                                              int64_t sumT, int lane, int32_t *waggC, int64_t *waggT,
                                              const Marks &mark = Marks()) {
    const int A = a.A, W = a.W;
    const uint32_t wmask = W >= 16 ? 0xffffffffu : ((1u << (2 * W)) - 1u);
    const int Lx = a.len[sq], px = a.pos_in[sq];
    const int64_t wox = a.pkoff[sq];
    const int64_t gx = a.global_offset + sq;
    const double ux = a.u_in ? a.u_in[sq] : uniform(a.seed, rng_stream, (uint64_t)gx);
    uint32_t gwx = 0;
    if (px >= 0) {
        const uint32_t *q = a.pk + wox + (px >> 4);
        gwx = funnel(q[1], q[0], 2 * (px & 15)) & wmask;
    }
    uint8_t *sx = wslice + seq_off;
    unsigned char *tab = wslice + tab_off;
    double *mpcv = (double *)(wslice + misc_off);
    int32_t *mres = (int32_t *)(wslice + misc_off + 32);
    // hold-one-out PCV (.fs:945-954), as in the scan
    if (lane < A) {
        const int64_t tot = sumT + (px >= 0 ? W : Lx);
        const int64_t bgc =
            sT[lane] + (px >= 0 ? sym_count(gwx, lane, wmask) : a.comp[(int64_t)sq * (A + 1) + lane]);
        mpcv[lane] = ((double)bgc + a.pc) / ((double)tot + a.apc);
    }
    // unpack the sequence: one word (16 symbols) per lane step
    const int nwx = (Lx + 15) >> 4;
    for (int i = lane; i < nwx; i += 64)
        *(uint4 *)(sx + 16 * i) = keep_bytes(unpack_word(a.pk[wox + i]), Lx - 16 * i);
    for (int i = 16 * nwx + 16 * lane; i < Lx + WM + 96; i += 16 * 64)
        *(uint4 *)(sx + i) = make_uint4(0, 0, 0, 0);
    wave_sync();
    mark(11);
    // (PWM, PCV) [e][tab_stride(WM)], columns past W (1, 1)
    constexpr int WS = tab_stride(WM);
    for (int c = lane; c < A * WS; c += 64) {
        const int e = c / WS, j = c - e * WS;
        double2 v = make_double2(1.0, 1.0);
        if (j < W) {
            const bool own = px >= 0 && (int)((gwx >> (2 * j)) & 3u) == e;
            const double2 pp = sPPM[j * 4 + e];
            const double pe = mpcv[e];
            v = make_double2((own ? pp.y : pp.x) / pe, pe);
        }
        *(double2 *)(tab + (e * WS + j) * 16) = v;
    }
    wave_sync();
    mark(12);
    const double thr_lo = a.thr_lo;
    auto evx = [&](int k, double &gg, double &mm) {
        exact_eval<WM>(sx, tab, thr_lo, a.cutoff, k, gg, mm);
    };
    const ExactPick r = exact_pick(
        evx, Lx - W + 1, lane, ux, [&] { return &GS_STAT(a)[1]; }, mres, mark);
    if (r.kind < 0) {
        if (lane == 0) {
            raise_error(a.err_code, a.err_index, 2, gx);  // every category missed (.fs:752)
            a.pos_out[sq] = -1;
        }
    } else {
        const int newp = r.kind == 0 ? -1 : r.win;
        if (lane == 0) {
            a.pos_out[sq] = newp;
            a.pwms_out[sq] = r.w;
        }
        if (newp >= 0) {
            // the new segment into the wavefront's aggregates
            const int e = lane < W ? sx[newp + lane] : 0;
            if (lane < W) atomicAdd(&waggC[e * W + lane], 1);
            if (lane < A) {
                int sc = 0;
                for (int j = 0; j < W; ++j) sc += sx[newp + j] == lane ? 1 : 0;
                waggT[lane] += (int64_t)(a.comp[(int64_t)sq * (A + 1) + lane] - sc);
            }
        }
    }
    wave_sync();  // the staging area is rewritten for the next target
}

}  // namespace gs
