// gs_stats.h — the host side of the chain statistics and summaries,
// for gs_api.cpp, gs_engine.cpp and gs_batch.cpp only: what the caller asked for, the holder of
// the statistics' device slab, the summary run.  The decisions (counted sweeps, slab layouts,
// byte estimates) are gs_statplan.h's; the kernels' argument structs are gs_ctx.h's.
#pragma once
#include "gs_ctx.h"
#include "gs_statplan.h"

namespace gs_host {
using namespace gs_plan;

// Where a chain summary goes: the host arrays by SummaryPart, each
// group (the chains' modes, the chains' cells, the pooled outputs) nullable as a whole.  The
// single-position form leaves the parts only lists have null; shapes are those of M = 1.
struct SummaryOut {
    void *out[kSummaryOutputs];
    bool list;
    static SummaryOut single(int32_t *mode_pos, int32_t *mode_count, int64_t *counts,
                             int32_t *pool_pos, int64_t *pool_count, int64_t *pool_counts,
                             int32_t *n_pooled) {
        return SummaryOut{{nullptr, nullptr, nullptr, mode_pos, mode_count, counts, nullptr, nullptr,
                           nullptr, pool_pos, pool_count, pool_counts, n_pooled},
                          false};
    }
    // how many of a group's pointers this form has, and how many of them are given
    void tally(int group, int &have, int &given) const {
        have = given = 0;
        for (int i = 0; i < kSummaryOutputs; ++i)
            if (kSummaryPartOf[i].group == group && (list || !kSummaryPartOf[i].list_only)) {
                ++have;
                given += out[i] != nullptr;
            }
    }
    bool whole(int group) const {
        int have, given;
        tally(group, have, given);
        return given == have;
    }
    bool modes() const { return whole(kGroupModes); }
    bool counts() const { return whole(kGroupCells); }
    bool pool() const { return whole(kGroupPool); }
    bool any() const { return modes() || counts() || pool(); }
    // half of a group given
    bool ragged() const {
        for (int g = 0; g < kSummaryGroups; ++g) {
            int have, given;
            tally(g, have, given);
            if (given != 0 && given != have) return true;
        }
        return false;
    }
    int64_t bytes(int64_t R, int64_t n, int64_t cells, int64_t M) const {
        const bool want[kSummaryGroups] = {modes(), counts(), pool()};
        return summary_bytes(R, n, cells, M, list, want);
    }
};

// Where a chain agreement goes: the host arrays by AgreementPart, one group,
// nullable as a whole.
struct AgreementOut {
    void *out[kAgreementOutputs];
    int given() const {
        int g = 0;
        for (void *p : out) g += p != nullptr;
        return g;
    }
    bool any() const { return given() == kAgreementOutputs; }
    // half of the group given
    bool ragged() const { return given() != 0 && given() != kAgreementOutputs; }
};

// The caller's side of the ..._stats and ..._summary entries: which sweeps count and where the
// chains' statistics go (each nullable; the best rows go with best_sweep_out).  sites_out and
// best_cnt_out: Positions-list chains only.
struct RunStats {
    int32_t burn_in, thin;
    int32_t *occ_out;
    double *ic_out;
    int64_t *best_sweep_out;
    int32_t *best_pos_out;
    double *best_pwms_out;
    // the reduction of the bins (and site counts), null: none
    const SummaryOut *sum = nullptr;
    int32_t *sites_out = nullptr, *best_cnt_out = nullptr;
    // the chains' agreement with their pool (run_batch only), null: none
    const AgreementOut *agr = nullptr;
    bool summed() const { return sum && sum->any(); }
    bool agreed() const { return agr && agr->any(); }
    bool any() const {
        return occ_out || sites_out || ic_out || best_sweep_out || summed() || agreed();
    }
    // what lives on the device: the bins and site counts for the caller, for the summary or
    // (the bins) for the agreement
    StatsWant want() const {
        return StatsWant{occ_out || summed() || agreed(), sites_out || summed(), ic_out != nullptr,
                         best_sweep_out != nullptr};
    }
    CountPlan plan(int32_t T) const { return CountPlan{burn_in, thin, T}; }
    // what every entry refuses: burn_in / thin out of range, the best rows (with best_cnt_out
    // on lists) not all-or-none with best_sweep_out, half of a summary's output group or of the
    // agreement's
    bool bad(int32_t n_sweeps, bool list) const {
        const bool rows = best_pos_out && best_pwms_out && (!list || best_cnt_out);
        const bool any_row = best_pos_out || best_pwms_out || (list && best_cnt_out);
        return burn_in < 0 || burn_in > n_sweeps || thin < 1 || (best_sweep_out != nullptr) != rows ||
               (!best_sweep_out && any_row) || (sum && sum->ragged()) || (agr && agr->ragged());
    }
};

// The statistics' device memory of one call of run_batch, run_multi_batch or run_sweeps (R =
// 1): one allocation carved by stats_slab, freed once nothing is in flight on it.
struct StatsSlab {
    gs_ctx *c;
    char *mem = nullptr;
    Slab<kStatsParts> lay{};
    std::vector<int64_t> h_off;  // alive until its upload is over
    explicit StatsSlab(gs_ctx *ctx) : c(ctx) {}
    StatsSlab(const StatsSlab &) = delete;
    StatsSlab &operator=(const StatsSlab &) = delete;
    ~StatsSlab();
    // The allocation and, on the stream, the initial values (zero bins and site counts, no
    // best yet: best_sweep -1 over zero rows, a list's best positions -1) and the offsets.
    int init(int32_t W, int64_t R, int64_t H, int64_t n_counted, int64_t cap, int64_t M, bool list,
             const StatsWant &w);
    template <class T>
    T *dev(int part) const {
        return lay.part[part].wanted ? (T *)(mem + lay.part[part].off) : nullptr;
    }
    // a part to the caller's array on the stream (dst null: it stays on the device)
    int download(int part, void *dst) const;
    // every part the caller asked for
    int download(const RunStats &st) const;
};

// The reduction of R histograms resident at d_occ ([R][H], bins of d_off; lists: site counts
// at d_sites, [R][n][M + 1]) behind whatever is on the stream: enqueue() carves and allocates
// the result slab (summary_slab), zeroes its prefix and launches between two events;
// download() enqueues the copies to the caller's arrays; finish(), after the caller's
// synchronisation, reads the device time into the context.  The slab lives until the object
// goes, which the caller lets happen only with nothing in flight.
struct SummaryRun {
    gs_ctx *c;
    char *slab = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    Slab<kSummaryParts> lay{};
    explicit SummaryRun(gs_ctx *ctx) : c(ctx) {}
    SummaryRun(const SummaryRun &) = delete;
    SummaryRun &operator=(const SummaryRun &) = delete;
    ~SummaryRun();
    int enqueue(int32_t W, int32_t M, const int32_t *d_occ, const int32_t *d_sites,
                const int64_t *d_off, int64_t H, int32_t R, int64_t n_counted, const SummaryOut &out);
    int download(const SummaryOut &out);
    void finish();
    template <class T>
    T *dev(int part) const {
        return lay.part[part].wanted ? (T *)(slab + lay.part[part].off) : nullptr;
    }
};
// The agreement of R histograms resident at d_occ with their pool, behind
// whatever is on the stream, as SummaryRun: enqueue() carves and allocates the result slab
// (agreement_slab), zeroes its prefix and launches between two events; download() enqueues the
// copies; finish(), after the caller's synchronisation, reads the device time into the context.
// The pooled flags are, in this order: the summary's of the same call (d_flags with its count
// d_n_pooled: the pool is decided once); the caller's mask (mask, [R], non-zero = pooled); the
// summaries' rule, decided here.
struct AgreementRun {
    gs_ctx *c;
    char *slab = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    Slab<kAgreementParts> lay{};
    std::vector<int32_t> h_flags;        // the mask as flags, alive until its upload is over
    int32_t h_pooled = 0;                // ... and their number
    const int32_t *d_n_pooled = nullptr; // where the pool's count is on the device (no mask)
    explicit AgreementRun(gs_ctx *ctx) : c(ctx) {}
    AgreementRun(const AgreementRun &) = delete;
    AgreementRun &operator=(const AgreementRun &) = delete;
    ~AgreementRun();
    int enqueue(const int32_t *d_occ, const int64_t *d_off, int64_t H, int32_t R, int64_t n_counted,
                int32_t *d_flags, const int32_t *d_n_pooled, const int32_t *mask);
    int download(const AgreementOut &out);
    void finish();
    template <class T>
    T *dev(int part) const {
        return lay.part[part].wanted ? (T *)(slab + lay.part[part].off) : nullptr;
    }
};
// What chains over no sequences leave: no bins, an all-NaN trace, no best, summary_of_nothing.
int stats_of_nothing(const gs_ctx *c, int32_t W, int64_t R, int64_t n_counted, const RunStats &st);
// The summary of chains over no sequences: no modes, zero cells, every chain pooled.
void summary_of_nothing(const gs_ctx *c, int32_t W, int64_t R, const SummaryOut &out);
// gs_occupancy_summary (sites null) and gs_list_occupancy_summary
int occupancy_summary(gs_ctx *c, int32_t W, int32_t M, const int32_t *occ, const int32_t *sites,
                      int32_t R, int64_t n_counted, const SummaryOut &out);
// The agreement of chains over no sequences: every chain pooled (or the mask's), (0, 0) a
// pooled chain.
void agreement_of_nothing(int64_t R, const int32_t *mask, const AgreementOut &out);
// gs_occupancy_agreement
int occupancy_agreement(gs_ctx *c, int32_t W, const int32_t *occ, int32_t R, int64_t n_counted,
                        const int32_t *mask, const AgreementOut &out);
int64_t occupancy_offsets(const gs_ctx *c, int32_t W, int64_t *off);
// gs_batch.cpp: the drivers of the chain batches and of the batched starts (arguments
// validated; stats null, or with no output: the entry without statistics)
int run_batch(gs_ctx *c, int32_t W, double pc, double cutoff, int32_t T, const uint64_t *seeds,
              int32_t R, int64_t first_sweep, int32_t mode, const double *u, int32_t *pos_inout,
              double *pwms_out, int32_t *status_out, const RunStats *stats = nullptr);
int starts_batch(gs_ctx *c, int32_t W, double pc, const uint64_t *seeds, int32_t R, int32_t mode,
                 double *score_out, int32_t *pos_out, int32_t *status_out);
int run_multi_batch(gs_ctx *c, int32_t M, int32_t W, double pc, double cutoff, int32_t T,
                    const uint64_t *seeds, int32_t R, int64_t first_sweep, int32_t mode, int32_t cap,
                    const double *u, int32_t *cnt_inout, int32_t *pos_inout, double *pwms_out,
                    int32_t *status_out, const RunStats *stats = nullptr);

}  // namespace gs_host
