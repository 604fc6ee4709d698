// gs_statplan.h — the host-side decisions of the chain statistics, summaries and agreement
// (DESIGN.md §9.30, §9.31), free of HIP so that a plain host compiler builds and tests them
// (tests/host/stats_plan_main.cpp, agreement_plan_main.cpp): which sweeps count, where the
// parts of a call's device slab lie, and how many bytes a call is charged before it is refused.
#pragma once
#include <cstdint>
#include <initializer_list>

namespace gs_plan {

// Which of a chain's T sweeps count: every thin-th from burn_in on.  The only place the rule
// is written.
struct CountPlan {
    int32_t burn_in, thin, T;
    bool counted(int32_t t) const { return t >= burn_in && (t - burn_in) % thin == 0; }
    int64_t n_counted() const { return burn_in < T ? ((int64_t)T - burn_in + thin - 1) / thin : 0; }
    // the trace entry of a counted sweep
    int64_t slot(int32_t t) const { return (t - burn_in) / thin; }
};

// One part of a slab: `count` elements of `elem` bytes (4 or 8), present when wanted, zero at
// launch or not.  The carve fills `off`.
struct Part {
    int64_t elem, count;
    bool wanted, zero;
    int64_t off;
    int64_t bytes() const { return wanted ? elem * count : 0; }
};

// Hands out offsets, each aligned to its part's element; an unwanted part takes no bytes.
struct Carve {
    int64_t total = 0;
    int64_t take(const Part &p) {
        if (!p.wanted) return total;
        const int64_t o = (total + p.elem - 1) / p.elem * p.elem;
        total = o + p.elem * p.count;
        return o;
    }
};

// A slab of N parts: the zero-at-launch parts first, 8-byte elements before 4-byte ones, so
// that they tile [0, zeroed) with no gap (one memset); then the others.
template <int N>
struct Slab {
    Part part[N];
    int64_t zeroed = 0, total = 0;
    void carve() {
        Carve c;
        for (const bool zero : {true, false}) {
            for (const int64_t elem : {8, 4})
                for (Part &p : part)
                    if (p.zero == zero && p.elem == elem) p.off = c.take(p);
            if (zero) zeroed = c.total;
        }
        total = c.total;
    }
};

// ---- the chain summary's result slab (gs_summary_kernel / gs_list_summary_kernel) ----
// The outputs in the order of the C entry points' arguments, then the pooled flags, which
// stay on the device.  The single-position form has no kModeSites .. kModeCnt and no
// kPoolSites .. kPoolCnt, and M = 1.
enum SummaryPart {
    kModeSites, kModeSitesCount, kModeCnt, kModePos, kModeCount,
    kCounts,
    kPoolSites, kPoolSitesCount, kPoolCnt, kPoolPos, kPoolCount, kPoolCounts, kNPooled,
    kSummaryOutputs,
    kPoolFlags = kSummaryOutputs,
    kSummaryParts
};
enum SummaryGroup { kGroupModes, kGroupCells, kGroupPool, kSummaryGroups };
// (the group of every part; whether only the list form has it)
constexpr struct { SummaryGroup group; bool list_only; } kSummaryPartOf[kSummaryParts] = {
    {kGroupModes, true}, {kGroupModes, true},  {kGroupModes, true}, {kGroupModes, false},
    {kGroupModes, false}, {kGroupCells, false}, {kGroupPool, true},  {kGroupPool, true},
    {kGroupPool, true},  {kGroupPool, false},  {kGroupPool, false}, {kGroupPool, false},
    {kGroupPool, false}, {kGroupPool, false}};

inline Slab<kSummaryParts> summary_slab(int64_t R, int64_t n, int64_t cells, int64_t M, bool list,
                                        const bool want[kSummaryGroups]) {
    // element size, element count, zero at launch
    const struct { int64_t elem, count; bool zero; } row[kSummaryParts] = {
        {4, R * n, false},     // mode_sites
        {4, R * n, false},     // mode_sites_count
        {4, R * n, false},     // mode_cnt
        {4, R * n * M, false}, // mode_pos
        {4, R * n * M, false}, // mode_count
        {8, R * cells, true},  // counts
        {4, n, false},         // pool_sites
        {8, n, false},         // pool_sites_count
        {4, n, false},         // pool_cnt
        {4, n * M, false},     // pool_pos
        {8, n * M, false},     // pool_count
        {8, cells, true},      // pool_counts
        {4, 1, true},          // n_pooled
        {4, R, false}};        // the chains' pooled flags
    Slab<kSummaryParts> s;
    for (int i = 0; i < kSummaryParts; ++i)
        s.part[i] = Part{row[i].elem, row[i].count,
                         want[kSummaryPartOf[i].group] && (list || !kSummaryPartOf[i].list_only),
                         row[i].zero, 0};
    s.carve();
    return s;
}

// ---- the chain agreement's result slab (gs_agreement_kernel) ----
// The outputs in the order of the C entry points' arguments, then the pooled flags, which stay
// on the device.  The per-chain parts collect atomic adds and are zero at launch, and so is the
// pool's count where this slab decides the pool by the rule; the per-sequence parts are written
// in full.  own_flags: the flags are this slab's (the rule, or the caller's mask), not a
// summary's of the same call; own_count: the rule decides them here, and counts them.
enum AgreementPart {
    kAgrAgree, kAgrSpread, kAgrSpreadChain, kAgrChainAgree, kAgrChainDist, kAgrNPooled,
    kAgreementOutputs,
    kAgrFlags = kAgreementOutputs,
    kAgreementParts
};

inline Slab<kAgreementParts> agreement_slab(int64_t R, int64_t n, bool own_flags, bool own_count) {
    Slab<kAgreementParts> s;
    s.part[kAgrAgree] = Part{4, n, true, false, 0};
    s.part[kAgrSpread] = Part{8, n, true, false, 0};
    s.part[kAgrSpreadChain] = Part{4, n, true, false, 0};
    s.part[kAgrChainAgree] = Part{4, R, true, true, 0};
    s.part[kAgrChainDist] = Part{8, R, true, true, 0};
    s.part[kAgrNPooled] = Part{4, 1, own_flags && own_count, true, 0};
    s.part[kAgrFlags] = Part{4, R, own_flags, false, 0};
    s.carve();
    return s;
}

// ---- the statistics' slab of the three chain drivers ----
// (run_sweeps: R = 1; the single-position drivers: cap = 1, no kStatSites, no kStatBestCnt)
enum StatsPart {
    kStatOcc, kStatSites, kStatIc, kStatBestSweep, kStatBestIc, kStatBestCnt, kStatBestPos,
    kStatBestPwms, kStatOff,
    kStatsParts
};
struct StatsWant {
    bool occ, sites, ic, best;
};

// Zero at launch: the bins, the site counts, best_ic, best_cnt, best_pwms, and the
// single-position drivers' best_pos.  The holder of the slab (StatsSlab) sets best_sweep and
// the list driver's best_pos to all-ones; the trace and the offsets are written in full.
inline Slab<kStatsParts> stats_slab(int64_t R, int64_t n, int64_t H, int64_t n_counted, int64_t cap,
                                    int64_t M, bool list, const StatsWant &w) {
    Slab<kStatsParts> s;
    s.part[kStatOcc] = Part{4, R * H, w.occ, true, 0};
    s.part[kStatSites] = Part{4, R * n * (M + 1), w.sites && list, true, 0};
    s.part[kStatIc] = Part{8, R * n_counted, w.ic, false, 0};
    s.part[kStatBestSweep] = Part{8, R, w.best, false, 0};
    s.part[kStatBestIc] = Part{8, R, w.best, true, 0};
    s.part[kStatBestCnt] = Part{4, R * n, w.best && list, true, 0};
    s.part[kStatBestPos] = Part{4, R * n * cap, w.best, !list, 0};
    s.part[kStatBestPwms] = Part{8, R * n, w.best, true, 0};
    s.part[kStatOff] = Part{8, n + 1, w.occ, false, 0};
    s.carve();
    return s;
}

// ---- what a call is charged against the 4 GiB a call may hold ----
// These sums decide GS_E_UNSUPPORTED and appear in its text: they are not the slabs' sizes
// (no padding, no flags' alignment) and stay as they are.
inline int64_t summary_bytes(int64_t R, int64_t n, int64_t cells, int64_t M, bool list,
                             const bool want[kSummaryGroups]) {
    return (want[kGroupModes] ? (list ? R * n * (12 + 8 * M) : R * n * 8) : 0) +
           (want[kGroupCells] ? R * cells * 8 : 0) +
           (want[kGroupPool] ? (list ? n * (16 + 12 * M) : n * 12) + cells * 8 + R * 4 + 8 : 0);
}
// the agreement's five arrays, the pooled flags and the pool's count
inline int64_t agreement_bytes(int64_t R, int64_t n) { return n * 16 + R * 12 + R * 4 + 8; }
// the bins and their offsets, the site counts, the trace, the running best and its rows
inline int64_t stats_bytes(int64_t R, int64_t n, int64_t H, int64_t n_counted, int64_t cap,
                           int64_t M, bool list, const StatsWant &w) {
    return (w.occ ? R * H * 4 + (n + 1) * 8 : 0) + (w.sites && list ? R * n * (M + 1) * 4 : 0) +
           (w.ic ? R * n_counted * 8 : 0) +
           (w.best ? R * 16 + R * n * ((list ? 4 : 0) + 4 * cap + 8) : 0);
}

}  // namespace gs_plan
