// The host-side plan of the chain statistics (gibbssampling_amd/csrc/gs_statplan.h) checked by a
// plain host program, built under AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_stats_plan_host.py: the counted-sweep rule against a brute-force loop, the two slab
// layouts' alignment / disjointness / zero prefix, and the byte estimates against the
// expressions the entry points used before the plan existed, written out literally.
#include <cstdio>

#include "gs_statplan.h"

using namespace gs_plan;

static long failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #x); \
        }                                                               \
    } while (0)

static void count_plan() {
    for (int32_t T = 0; T <= 12; ++T)
        for (int32_t burn_in = 0; burn_in <= T; ++burn_in)
            for (int32_t thin = 1; thin <= 5; ++thin) {
                const CountPlan p{burn_in, thin, T};
                int64_t n = 0;
                for (int32_t t = 0; t < T; ++t) {
                    bool hit = false;  // t is burn_in plus a multiple of thin
                    for (int32_t s = burn_in; s <= t; s += thin) hit = hit || s == t;
                    CHECK(p.counted(t) == hit);
                    if (hit) CHECK(p.slot(t) == n);  // 0, 1, ... in order
                    n += hit;
                }
                CHECK(p.n_counted() == n);
            }
}

// What every slab has to satisfy: wanted parts aligned to their element, pairwise disjoint and
// inside the total; the zero-at-launch parts exactly tile [0, zeroed); unwanted parts take
// nothing.
template <int N>
static void check_slab(const Slab<N> &s) {
    int64_t zero_bytes = 0, bytes = 0;
    for (int i = 0; i < N; ++i) {
        const Part &p = s.part[i];
        if (!p.wanted) {
            CHECK(p.bytes() == 0);
            continue;
        }
        bytes += p.bytes();
        CHECK(p.elem == 4 || p.elem == 8);
        CHECK(p.off % p.elem == 0);
        CHECK(p.off >= 0 && p.off + p.bytes() <= s.total);
        if (p.zero) {
            zero_bytes += p.bytes();
            CHECK(p.off + p.bytes() <= s.zeroed);
        } else {
            CHECK(p.off >= s.zeroed);
        }
        for (int j = 0; j < i; ++j) {
            const Part &q = s.part[j];
            if (q.wanted && p.bytes() > 0 && q.bytes() > 0)
                CHECK(p.off + p.bytes() <= q.off || q.off + q.bytes() <= p.off);
        }
    }
    // disjoint parts inside [0, zeroed) that sum to it leave no gap
    CHECK(zero_bytes == s.zeroed);
    CHECK(s.zeroed <= s.total);
    // padding only: less than one element before each part
    CHECK(s.total - bytes < 8 * N);
}

static void summary_table() {
    for (int mask = 0; mask < 8; ++mask)
        for (const bool list : {false, true})
            for (const int64_t R : {1, 3})
                for (const int64_t n : {1, 5})
                    for (const int64_t M : {1, 3})
                        for (const int64_t cells : {4 * 3 + 4, 20 * 5 + 20}) {
                            const bool m = mask & 1, k = mask & 2, p = mask & 4;
                            const bool want[kSummaryGroups] = {m, k, p};
                            const Slab<kSummaryParts> s = summary_slab(R, n, cells, M, list, want);
                            check_slab(s);
                            for (int i = 0; i < kSummaryParts; ++i)
                                CHECK(s.part[i].wanted ==
                                      (want[kSummaryPartOf[i].group] &&
                                       (list || !kSummaryPartOf[i].list_only)));
                            // the kernels' shapes
                            CHECK(s.part[kCounts].bytes() == (k ? R * cells * 8 : 0));
                            CHECK(s.part[kModePos].bytes() == (m ? R * n * M * 4 : 0));
                            CHECK(s.part[kModeSites].bytes() == (m && list ? R * n * 4 : 0));
                            CHECK(s.part[kPoolCount].bytes() == (p ? n * M * 8 : 0));
                            CHECK(s.part[kPoolFlags].bytes() == (p ? R * 4 : 0));
                            CHECK(s.part[kCounts].zero && s.part[kPoolCounts].zero &&
                                  s.part[kNPooled].zero);
                            // today's estimates, literally
                            const int64_t single = (m ? R * n * 8 : 0) + (k ? R * cells * 8 : 0) +
                                                   (p ? n * 12 + cells * 8 + R * 4 + 8 : 0);
                            const int64_t lists = (m ? R * n * (12 + 8 * M) : 0) +
                                                  (k ? R * cells * 8 : 0) +
                                                  (p ? n * (16 + 12 * M) + cells * 8 + R * 4 + 8 : 0);
                            CHECK(summary_bytes(R, n, cells, M, list, want) == (list ? lists : single));
                        }
}

static void stats_slab_table() {
    const int64_t n = 5, H = 51, n_counted = 3, M = 3;  // H odd
    for (int mask = 0; mask < 16; ++mask)
        for (const bool list : {false, true})
            for (const int64_t R : {1, 3})
                for (const int64_t cap : {1, 5}) {
                    const StatsWant w{(mask & 1) != 0, (mask & 2) != 0, (mask & 4) != 0,
                                      (mask & 8) != 0};
                    const Slab<kStatsParts> s = stats_slab(R, n, H, n_counted, cap, M, list, w);
                    check_slab(s);
                    CHECK(s.part[kStatOcc].bytes() == (w.occ ? R * H * 4 : 0));
                    CHECK(s.part[kStatOff].bytes() == (w.occ ? (n + 1) * 8 : 0));
                    CHECK(s.part[kStatSites].bytes() == (w.sites && list ? R * n * (M + 1) * 4 : 0));
                    CHECK(s.part[kStatIc].bytes() == (w.ic ? R * n_counted * 8 : 0));
                    CHECK(s.part[kStatBestSweep].bytes() == (w.best ? R * 8 : 0));
                    CHECK(s.part[kStatBestIc].bytes() == (w.best ? R * 8 : 0));
                    CHECK(s.part[kStatBestCnt].bytes() == (w.best && list ? R * n * 4 : 0));
                    CHECK(s.part[kStatBestPos].bytes() == (w.best ? R * n * cap * 4 : 0));
                    CHECK(s.part[kStatBestPwms].bytes() == (w.best ? R * n * 8 : 0));
                    // the initial values: zero, but best_sweep (-1) and a list's best_pos (-1),
                    // which the slab's holder fills; the trace and offsets are written in full
                    CHECK(s.part[kStatOcc].zero && s.part[kStatSites].zero &&
                          s.part[kStatBestIc].zero && s.part[kStatBestCnt].zero &&
                          s.part[kStatBestPwms].zero);
                    CHECK(!s.part[kStatBestSweep].zero && s.part[kStatBestPos].zero == !list);
                    // today's estimates, literally: run_batch / run_sweeps (R = 1), run_multi_batch
                    const int64_t rows = R * n;
                    const int64_t single = (w.occ ? R * H * 4 + (n + 1) * 8 : 0) +
                                           (w.ic ? R * n_counted * 8 : 0) +
                                           (w.best ? R * (16 + n * 12) : 0);
                    const int64_t lists = (w.occ ? R * H * 4 + (n + 1) * 8 : 0) +
                                          (w.sites ? rows * (M + 1) * 4 : 0) +
                                          (w.ic ? R * n_counted * 8 : 0) +
                                          (w.best ? R * 16 + rows * (4 + 4 * cap + 8) : 0);
                    CHECK(stats_bytes(R, n, H, n_counted, list ? cap : 1, M, list, w) ==
                          (list ? lists : single));
                }
}

int main() {
    count_plan();
    summary_table();
    stats_slab_table();
    if (failures) {
        std::printf("%ld checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
