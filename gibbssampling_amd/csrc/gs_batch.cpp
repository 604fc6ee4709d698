// gs_batch.cpp — the host drivers of the batched entry points:
// motif_batch (gs_motif_sampling_batch), site_batch (gs_site_sampling_batch), multi_batch
// (gs_motif_sampling_multi_batch), run_batch (gs_motif_run_batch and, with the chains'
// statistics, gs_motif_run_batch_stats, §9.25), run_multi_batch
// (gs_motif_run_multi_batch and, with statistics, gs_motif_run_multi_batch_stats, §9.26) and
// starts_batch (gs_random_starts_batch), and the host side of the chain statistics and
// summaries (gs_stats.h, §9.30: StatsSlab for the three chain drivers, SummaryRun and
// occupancy_summary for gs_occupancy_summary, gs_list_occupancy_summary and the ..._summary
// calls, §9.28, §9.29), over one copy of the stages they share.  gs_api.cpp validates the arguments; the single-chain pieces they reuse
// (set_snapshot_dev, starts_enqueue, starts_pass, greedy_carve, one_sweep) are in
// gs_engine.cpp.
#include "gs_stats.h"

namespace gs_host {
namespace {

// One device allocation, freed on scope exit.
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { dfree(p); }
    int alloc(gs_ctx *c, int64_t elems) {
        HIP_TRY(c, hipMalloc(&p, (size_t)elems * sizeof(T)));
        return GS_OK;
    }
    operator T *() const { return p; }
};
// (a stage's status, handed on when it is not GS_OK)
#define GS_TRY(x)                      \
    do {                               \
        if (int rc_ = (x)) return rc_; \
    } while (0)

// The boundaries of a call's N - 1 timed stages: pooled events, recorded on the stream in
// order, back in the pool on every path.
template <int N>
struct StageEvents {
    gs_ctx *c;
    hipEvent_t ev[N];
    int next = 0;
    explicit StageEvents(gs_ctx *ctx) : c(ctx) {
        for (hipEvent_t &e : ev) e = get_event(c);
    }
    StageEvents(const StageEvents &) = delete;
    StageEvents &operator=(const StageEvents &) = delete;
    ~StageEvents() {
        for (hipEvent_t e : ev) c->ev_pool.push_back(e);
    }
    hipError_t mark() { return hipEventRecord(ev[next++], c->stream); }
    // After the stages (rc: their outcome, which is returned): a failed call synchronises,
    // so that nothing is in flight on the slabs when they go; a good one (synchronised by
    // its last stage) leaves the intervals in ms[N - 1], 0.0 where one cannot be read.
    int finish(int rc, double *ms) {
        if (rc) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
        for (int i = 0; i + 1 < N; ++i) {
            float t = 0.0f;
            ms[i] = hipEventElapsedTime(&t, ev[i], ev[i + 1]) == hipSuccess ? (double)t : 0.0;
        }
        return GS_OK;
    }
};

// No target: every chain is done after no pass.
int no_targets(int32_t R, int32_t *passes_out, int per_chain, int32_t *status_out) {
    for (int32_t r = 0; r < R; ++r) {
        for (int k = 0; passes_out && k < per_chain; ++k) passes_out[per_chain * r + k] = 0;
        if (status_out) status_out[r] = GS_OK;
    }
    return GS_OK;
}

int batch_bytes_refuse(gs_ctx *c, const char *entry, int64_t bytes) {
    if (bytes <= kBatchBytesMax) return GS_OK;
    return fail(c, GS_E_UNSUPPORTED,
                std::string(entry) + ": the chains' slabs take " + std::to_string(bytes) +
                    " B, more than the " + std::to_string(kBatchBytesMax) +
                    " B a batch may hold: split the seeds over several calls");
}

// Workgroups per chain of the batched aggregate passes: 256 targets each, the GPU four
// deep over all chains.
int agg_blocks(const gs_ctx *c, int64_t n, int32_t R) {
    return (int)std::max<int64_t>(
        1, std::min<int64_t>((n + 255) / 256, std::max<int64_t>(1, (int64_t)c->n_cu * 4 / R)));
}

// Mode 1: every chain's shared draws (row r: seed r), drawn on the host, one upload.  The
// host copy lives as long as the device one (the upload reads pageable memory).
struct SharedStarts {
    DevBuf<int32_t> d;
    std::vector<int32_t> h;
    int draw(gs_ctx *c, int32_t W, const uint64_t *seeds, int32_t R) {
        const int64_t n = c->n_local;
        GS_TRY(d.alloc(c, R * n));
        h.resize((size_t)(R * n));
        for (int32_t r = 0; r < R; ++r)
            for (int64_t i = 0; i < n; ++i)
                h[(size_t)(r * n + i)] =
                    uniform_int(seeds[r], stream_init_shared(), (uint64_t)(c->global_offset + i),
                                c->h_len[i] - W + 1);
        HIP_TRY(c, hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, c->stream));
        return GS_OK;
    }
    const int32_t *row(gs_ctx *c, int32_t r) const { return d ? d + (int64_t)r * c->n_local : nullptr; }
};

// The starts of one chain on the context's single-chain state: the start vector the
// aggregate pass reads (the shared draws d_starts_row, mode 1, or any valid one: mode 0
// takes only the composition totals from it) -> snapshot -> getPWMOfRandomStarts into
// d_pos[1], d_pwms.  The error words are reset first and keep what the chain raises.
int chain_starts(gs_ctx *c, int mode, int32_t W, double pc, uint64_t seed,
                 const int32_t *d_starts_row, int32_t *d_cpart) {
    const size_t n = (size_t)c->n_local;
    if (mode == 0) HIP_TRY(c, hipMemsetAsync(c->d_pos[0], 0, n * 4, c->stream));
    GS_TRY(set_snapshot_dev(c, W, mode == 0 ? c->d_pos[0] : d_starts_row, true));
    // a target that raises (.fs:117) writes no start: every entry stays a valid one
    HIP_TRY(c, hipMemsetAsync(c->d_pos[1], 0, n * 4, c->stream));
    return starts_enqueue(c, mode, W, pc, seed, d_cpart);
}

// tune.batch_starts: whether a driver takes its chains' starts from BatchStarts.  Automatic:
// while a chain has fewer targets than a launch has workgroups (8 a CU); from there on a
// chain's own launches fill the GPU and the batched starts measured no faster (§9.15).
bool batched_starts(const gs_ctx *c) {
    return c->tune.batch_starts == 1 ||
           (c->tune.batch_starts < 0 && c->n_global < (int64_t)c->n_cu * 8);
}

// The starts of all chains in a constant number of launches (the drivers under
// batched_starts, and gs_random_starts_batch): what the loop over
// chain_starts leaves in d_pos[1] / d_pwms and the context's error words, chain after
// chain, as row r of the caller's slabs.  prepare() allocates and uploads before the timed
// stages; enqueue() only enqueues.  Mode 0 runs the chains in groups whose cpart stays under
// kStartsCpartBudget (a chain's own slab may pass it: then one chain a group), and counts
// with the chain-indexed kernel while a chain has fewer targets than the launch has
// workgroups, beyond with the single-chain kernel chain after chain (the chain-indexed one
// measured 17.4 against 12.5 ms at 10k sequences x 8 chains).
struct BatchStarts {
    DevBuf<int64_t> agg;     // mode 1: [R][cells] of the shared draws; mode 0: one row
    DevBuf<int32_t> cpart;   // mode 0: [group][n_global][A * W]
    DevBuf<uint64_t> seeds;  // [R]
    const uint64_t *h_seeds = nullptr;  // the caller's, alive for the call
    StartsArgs sa{};
    PartialArgs pa{};
    int64_t lds = 0, cpart_chain = 0;
    int32_t R = 0, mode = 0, group = 0, cells = 0;
    // the device time of the counts / aggregates and of the scans, when asked for
    std::vector<hipEvent_t> ev;
    gs_ctx *ctx = nullptr;
    BatchStarts() = default;
    BatchStarts(const BatchStarts &) = delete;
    BatchStarts &operator=(const BatchStarts &) = delete;
    ~BatchStarts() {
        if (ctx) release(ctx);
    }

    int prepare(gs_ctx *c, int32_t W, double pc, const uint64_t *seeds_in, int32_t n_chains,
                int32_t init_mode) {
        ctx = c;
        R = n_chains;
        mode = init_mode;
        cells = c->A * W + c->A;
        // (a fixed PCV / PPM applies as in starts_enqueue: the context's own for
        // gs_random_starts_batch, the caller's arguments for the *_batch_fixed drivers)
        GS_TRY(starts_pass(c, mode, W, pc, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                           c->use_ppm ? c->d_ppm_fixed : nullptr, &sa, &lds));
        cpart_chain = mode == 0 ? c->n_global * c->A * W : 0;
        group = mode == 0 ? (int32_t)std::max<int64_t>(
                                1, std::min<int64_t>(R, kStartsCpartBudget / std::max<int64_t>(
                                                            1, cpart_chain * 4)))
                          : R;
        GS_TRY(agg.alloc(c, (int64_t)(mode == 1 ? R : 1) * cells));
        if (mode == 0) GS_TRY(cpart.alloc(c, std::max<int64_t>(1, group * cpart_chain)));
        GS_TRY(seeds.alloc(c, R));
        h_seeds = seeds_in;
        HIP_TRY(c, hipMemcpyAsync(seeds, h_seeds, (size_t)R * 8, hipMemcpyHostToDevice, c->stream));
        pa.seq = c->d_seq;
        pa.doff = c->d_doff;
        pa.len = c->d_len;
        pa.n_local = c->n_local;
        pa.global_offset = c->global_offset;
        pa.n_global = c->n_global;
        pa.A = c->A;
        pa.W = W;
        pa.cpart = cpart;
        sa.agg = agg;
        sa.cpart = cpart;
        return GS_OK;
    }

    // Chain r's scores, starts and (code, index) error words -> row r of the slabs.
    // timed: events around every group's two stages (read by elapsed()).
    int enqueue(gs_ctx *c, double *score, int32_t *pos, int32_t *err_code,
                unsigned long long *err_index, bool timed = false) {
        const int64_t n = c->n_local;
        // a target that raises (.fs:117) writes no start: every entry stays a valid one
        HIP_TRY(c, hipMemsetAsync(pos, 0, (size_t)(R * n) * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(err_code, 0, (size_t)R * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(err_index, 0xff, (size_t)R * 8, c->stream));
        auto mark = [&]() -> hipError_t {
            if (!timed) return hipSuccess;
            ev.push_back(get_event(c));
            return hipEventRecord(ev.back(), c->stream);
        };
        HIP_TRY(c, mark());
        // mode 1: the aggregates of every chain's shared draws; mode 0: the composition
        // totals, the same for every chain, from one row of any valid start vector
        StartsBatchArgs b{};
        b.seeds = seeds;
        b.n_chains = mode == 1 ? R : 1;
        b.blocks = agg_blocks(c, n, b.n_chains);
        b.src = mode;
        b.E = c->E;
        b.comp = c->d_comp;
        b.agg_out = agg;
        b.agg_out_chain = cells;
        HIP_TRY(c, hipMemsetAsync(agg, 0, (size_t)b.n_chains * cells * 8, c->stream));
        HIP_TRY(c, gs_starts_batch_agg_launch(sa, b, c->stream));
        b.agg_chain = mode == 1 ? cells : 0;
        b.cpart_chain = cpart_chain;
        // the scans' workgroups: the D table's slots when it lies in HBM (starts_pass)
        const int64_t wg_max =
            sa.dt_global ? std::max<int>(c->n_cu * 2, c->tune.multi_spec_slots) : (int64_t)c->n_cu * 8;
        for (int32_t g0 = 0; g0 < R; g0 += group) {
            const int32_t ng = std::min(group, R - g0);
            if (g0 > 0) HIP_TRY(c, mark());
            b.seeds = seeds + g0;
            b.n_chains = ng;
            b.n_pairs = (int64_t)ng * n;
            if (mode == 0 && c->n_global < (int64_t)c->n_cu * 8) {
                const int64_t items = (int64_t)ng * c->n_global;
                HIP_TRY(c, gs_starts_batch_partial_launch(
                               pa, b, (int)std::min<int64_t>(items, (int64_t)c->n_cu * 8), c->stream));
            } else if (mode == 0) {
                // a chain's targets fill the launch's workgroups by themselves: the
                // single-chain count kernel, chain after chain, each into its slab
                for (int32_t r = 0; r < ng; ++r) {
                    PartialArgs p1 = pa;
                    p1.seed = h_seeds[g0 + r];
                    p1.cpart = cpart + r * cpart_chain;
                    HIP_TRY(c, gs_starts_partial_launch(p1, c->n_cu * 8, c->stream));
                }
            }
            HIP_TRY(c, mark());
            StartsArgs a = sa;
            a.score_out = score + g0 * n;
            a.pos_out = pos + g0 * n;
            a.err_code = err_code + g0;
            a.err_index = err_index + g0;
            if (mode == 1) a.agg = agg + (int64_t)g0 * cells;
            HIP_TRY(c, gs_starts_batch_launch(a, b, (int)std::min<int64_t>(b.n_pairs, wg_max),
                                              (size_t)lds, c->stream));
            HIP_TRY(c, mark());
        }
        return GS_OK;
    }

    // After the synchronisation: ms[0] the counts / aggregates, ms[1] the scans, summed
    // over the groups; the events go back to the pool.
    void elapsed(gs_ctx *c, double ms[2]) {
        ms[0] = ms[1] = 0.0;
        for (size_t i = 0; i + 2 < ev.size(); i += 3)
            for (int k = 0; k < 2; ++k) {
                float t = 0.0f;
                if (hipEventElapsedTime(&t, ev[i + k], ev[i + k + 1]) == hipSuccess) ms[k] += t;
            }
        release(c);
    }
    void release(gs_ctx *c) {
        for (hipEvent_t e : ev) c->ev_pool.push_back(e);
        ev.clear();
    }
};

// The context's own error words end clear, whatever the last chain's were.
int clear_ctx_error_words(gs_ctx *c) {
    HIP_TRY(c, hipMemsetAsync(c->d_err_code, 0, 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_err_index, 0xff, 8, c->stream));
    return GS_OK;
}

// The context's single-chain buffers were the chains' scratch: no snapshot is left.
void scratch_used(gs_ctx *c) {
    c->have_state = false;
    takeover_reset(c);
    c->ftab_agg = -1;
}

// The chains' status from their (code, index) error words: status_out[r], and the call
// fails with the lowest failing chain's.
int report_chain_errors(gs_ctx *c, const std::vector<int32_t> &code,
                        const std::vector<unsigned long long> &index, int32_t *status_out) {
    int first = -1;
    for (size_t r = 0; r < code.size(); ++r) {
        if (status_out) status_out[r] = code[r];
        if (code[r] != 0 && first < 0) first = (int)r;
    }
    if (first < 0) return GS_OK;
    return fail(c, code[(size_t)first],
                std::string(device_error_message(code[(size_t)first])) + " (chain " +
                    std::to_string(first) + ")",
                (int64_t)index[(size_t)first]);
}

// The same from packed status words.  unsupported (nullable): the text of a chain given
// up with kMultiErrUnsupported.
int report_chain_errors(gs_ctx *c, const std::vector<unsigned long long> &word,
                        int32_t *status_out, const char *unsupported) {
    int first = -1, first_status = GS_OK;
    for (size_t r = 0; r < word.size(); ++r) {
        const bool given_up =
            unsupported && word[r] != ~0ull && (int)(word[r] & 15ull) == kMultiErrUnsupported;
        const int status = given_up ? GS_E_UNSUPPORTED : packed_status(word[r]);
        if (status_out) status_out[r] = status;
        if (status != GS_OK && first < 0) {
            first = (int)r;
            first_status = status;
        }
    }
    if (first < 0) return GS_OK;
    return fail(c, first_status,
                std::string(first_status == GS_E_UNSUPPORTED ? unsupported
                                                             : device_error_message(first_status)) +
                    " (chain " + std::to_string(first) + ")",
                (int64_t)(word[(size_t)first] >> 4));
}

// The slabs of the star greedy batches (row r = chain r) and what both drivers do with
// them: the chain just prepared on the context -> slab r; one launch for all chains.
struct StarSlabs {
    DevBuf<int32_t> pos, passes, err;
    DevBuf<double> pwms;
    DevBuf<int64_t> agg;
    DevBuf<unsigned long long> erri;
    int64_t n = 0, agg_elems = 0;
    int alloc(gs_ctx *c, int32_t R) {
        n = c->n_local;
        agg_elems = (int64_t)kRepl * c->stride;
        GS_TRY(pos.alloc(c, R * n));
        GS_TRY(pwms.alloc(c, R * n));
        GS_TRY(agg.alloc(c, R * agg_elems));
        GS_TRY(passes.alloc(c, R));
        GS_TRY(err.alloc(c, R));
        return erri.alloc(c, R);
    }
    int take_chain(gs_ctx *c, int32_t r) {
        HIP_TRY(c, hipMemcpyAsync(pos + r * n, c->d_pos[c->cur_pos], (size_t)n * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(pwms + r * n, c->d_pwms, (size_t)n * 8, hipMemcpyDeviceToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(agg + r * agg_elems, c->d_agg[c->cur_agg], (size_t)agg_elems * 8,
                                  hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(err + r, c->d_err_code, 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(erri + r, c->d_err_index, 8, hipMemcpyDeviceToDevice, c->stream));
        return GS_OK;
    }
    int launch(gs_ctx *c, GreedyArgs &a, int32_t R, int waves, int64_t lds) {
        a.agg = agg;
        a.pos = pos;
        a.pwms = pwms;
        a.passes_out = passes;
        a.err_code = err;
        a.err_index = erri;
        a.exit_chunk = 0;
        a.exit_out = nullptr;
        // (as greedy_run after the carve: the caller's PCV of the *_batch_fixed entry points)
        a.pcv_fixed = c->use_pcv ? c->d_pcv_fixed : nullptr;
        HIP_TRY(c, gs_greedy_batch_launch(a, R, waves, (size_t)lds, c->stream, nullptr, nullptr));
        return GS_OK;
    }
};

// Speculative slots per chain of the list batch's greedy: the GPU is
// filled by chains first, so the width falls with R from multi_batch_fill (2) scoring
// workgroups per CU in all, about what is resident at once; never more than the single
// chain's width, and the arenas stay under kArenaBudget.
int32_t multi_batch_slots(const gs_ctx *c, int64_t chains, int64_t slot_bytes) {
    int64_t s = std::min<int64_t>(c->n_local, c->tune.multi_spec_slots);
    s = std::min<int64_t>(s, ((int64_t)c->tune.multi_batch_fill * c->n_cu + chains - 1) / chains);
    s = std::min<int64_t>(s, kArenaBudget / (chains * slot_bytes));
    return (int32_t)std::max<int64_t>(1, s);
}

}  // namespace

// R independent doMotifSampling runs (.fs:1034-1038, motifAmount = 1).  Stage 1, chain
// after chain on the context's single-chain state and stream, no host wait in between:
// starts (seed r; under batched_starts all chains' first, into the slabs) -> snapshot of
// them -> sweep 0 of seed r -> device copies of positions, PWMS, replica aggregates and the
// error words into slab r.  Stage 2: one launch of
// gs_greedy_batch_kernel, workgroup r on slab r, every pass in-kernel.  One
// synchronisation, then the slabs come down.  The caller validated the arguments.
int motif_batch(gs_ctx *c, int32_t W, double pc, double cutoff, const uint64_t *seeds, int32_t R,
                int32_t mode, int32_t max_passes, int32_t *pos_out, double *pwms_out,
                int32_t *passes_out, int32_t *status_out) {
    const int64_t n = c->n_local;
    if (n == 0) return no_targets(R, passes_out, 1, status_out);
    GS_TRY(ensure_state(c, W));
    GreedyArgs a{};
    int waves = 0;
    int64_t lds = 0;
    GS_TRY(greedy_carve(c, 0, pc, cutoff, max_passes, a, waves, lds));
    const int64_t agg_elems = (int64_t)kRepl * c->stride;
    const int64_t cpart_bytes = mode == 0 ? c->n_global * c->A * W * 4 : 0;
    GS_TRY(batch_bytes_refuse(
        c, "gs_motif_sampling_batch",
        (int64_t)R * (n * (4 + 8 + (mode == 1 ? 4 : 0)) + agg_elems * 8 + 16) + cpart_bytes));
    StarSlabs b;
    GS_TRY(b.alloc(c, R));
    DevBuf<int32_t> cpart;
    SharedStarts starts;
    BatchStarts bs;
    const bool batched = batched_starts(c);
    if (batched)
        GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
    else if (mode == 0)
        GS_TRY(cpart.alloc(c, std::max<int64_t>(cpart_bytes, 4) / 4));
    else
        GS_TRY(starts.draw(c, W, seeds, R));
    StageEvents<3> ev(c);
    int rc = [&]() -> int {
        HIP_TRY(c, ev.mark());
        // batched: row r of the slabs holds chain r's starts until take_chain replaces it
        if (batched) GS_TRY(bs.enqueue(c, b.pwms, b.pos, b.err, b.erri));
        for (int32_t r = 0; r < R; ++r) {
            if (batched) {
                HIP_TRY(c, hipMemcpyAsync(c->d_err_code, b.err + r, 4, hipMemcpyDeviceToDevice,
                                          c->stream));
                HIP_TRY(c, hipMemcpyAsync(c->d_err_index, b.erri + r, 8, hipMemcpyDeviceToDevice,
                                          c->stream));
            } else {
                GS_TRY(chain_starts(c, mode, W, pc, seeds[r], starts.row(c, r), cpart));
            }
            // its error word stays set: the sweep skips, the chain's slab carries it
            GS_TRY(set_snapshot_dev(c, W, batched ? b.pos + r * n : c->d_pos[1], false));
            if (use_dna(c)) {  // (as gs_run_sweeps: the device sweep counter at sweep 0)
                GS_TRY(need_vec(c));
                HIP_TRY(c, gs_set_counter_launch(c->d_sweep_ctr, 0ull, c->d_done_ctr, c->stream));
            }
            GS_TRY(one_sweep(c, pc, cutoff, nullptr, seeds[r], stream_sweep(0), true));
            GS_TRY(need_rep(c));
            GS_TRY(b.take_chain(c, r));
        }
        HIP_TRY(c, hipMemsetAsync(b.passes, 0, (size_t)R * 4, c->stream));
        HIP_TRY(c, ev.mark());
        GS_TRY(b.launch(c, a, R, waves, lds));
        HIP_TRY(c, ev.mark());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    scratch_used(c);
    GS_TRY(ev.finish(rc, c->batch_ms));
    c->last_greedy_waves = waves;
    std::vector<int32_t> herr((size_t)R), hpass((size_t)R);
    std::vector<unsigned long long> hidx((size_t)R);
    HIP_TRY(c, hipMemcpy(herr.data(), b.err, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hidx.data(), b.erri, (size_t)R * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hpass.data(), b.passes, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pos_out, b.pos, (size_t)(R * n) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pwms_out, b.pwms, (size_t)(R * n) * 8, hipMemcpyDeviceToHost));
    if (passes_out) std::copy(hpass.begin(), hpass.end(), passes_out);
    return report_chain_errors(c, herr, hidx, status_out);
}

// R independent doSiteSampling runs (.fs:697-701), DESIGN.md §9.11.  Stage 1, chain after
// chain on the context's single-chain state and stream, no host wait in between: starts
// (seed r) -> snapshot of them -> device copies of positions, scores, replica aggregates
// and the error words into slab r; under batched_starts the launches of BatchStarts write
// the slabs in place and one more aggregate launch fills the chains' replica 0.  Stage 2: getBestPWMSsWithStartPositions of every
// chain as one launch of the star site engine, workgroup r on slab r, every pass
// in-kernel.  Stage 3: the shifted passes (-1 to completion, then +1), every running
// chain in the same launches, one synchronisation per pass for all chains.  The caller
// validated the arguments.
int site_batch(gs_ctx *c, int32_t W, double pc, const uint64_t *seeds, int32_t R, int32_t mode,
               int32_t max_passes, int32_t *pos_out, double *score_out, int32_t *passes_out,
               int32_t *status_out) {
    const int64_t n = c->n_local;
    if (n == 0) return no_targets(R, passes_out, 3, status_out);
    GS_TRY(ensure_state(c, W));
    GreedyArgs a{};
    int waves = 0;
    int64_t lds = 0;
    GS_TRY(greedy_carve(c, 1, pc, 0.0, max_passes, a, waves, lds));
    const int64_t agg_elems = (int64_t)kRepl * c->stride;
    const int64_t cpart_bytes = mode == 0 ? c->n_global * c->A * W * 4 : 0;
    // per chain: positions, scores, shifted starts (and the shared draws), aggregates,
    // Gauss–Seidel passes, error words, stage passes [3], pass control [3]
    GS_TRY(batch_bytes_refuse(
        c, "gs_site_sampling_batch",
        (int64_t)R * (n * (4 + 8 + 4 + (mode == 1 ? 4 : 0)) + agg_elems * 8 + 4 + 4 + 8 + 12 + 12) +
            cpart_bytes));
    StarSlabs b;
    GS_TRY(b.alloc(c, R));
    // the shifted passes: start vectors, stage pass counts [R][3], pass control [3][R]
    DevBuf<int32_t> shifted, stage_passes, ctl;
    GS_TRY(shifted.alloc(c, R * n));
    GS_TRY(stage_passes.alloc(c, (int64_t)R * 3));
    GS_TRY(ctl.alloc(c, (int64_t)R * 3));
    int32_t *d_run = ctl, *d_moved = ctl + R, *d_left = ctl + 2 * (int64_t)R;
    // the shifted scans' arguments: the chains' slabs, the D table in LDS
    StartsArgs sa{};
    int64_t slds = 0;
    GS_TRY(starts_pass(c, 2, W, pc, 0, shifted, nullptr, b.agg, b.pwms, b.pos, nullptr, &sa, &slds));
    if (sa.dt_global)
        return fail(c, GS_E_UNSUPPORTED,
                    "gs_site_sampling_batch: the scan's D table of the longest sequence does "
                    "not fit in LDS (loop gs_site_sampling)");
    sa.err_code = b.err;
    sa.err_index = b.erri;
    const int scan_blocks =
        (int)std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)c->n_cu * 8 + R - 1) / R));
    const int ablocks = agg_blocks(c, n, R);
    DevBuf<int32_t> cpart;
    SharedStarts starts;
    BatchStarts bs;
    const bool batched = batched_starts(c);
    if (batched)
        GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
    else if (mode == 0)
        GS_TRY(cpart.alloc(c, std::max<int64_t>(cpart_bytes, 4) / 4));
    else
        GS_TRY(starts.draw(c, W, seeds, R));
    StageEvents<4> ev(c);
    std::vector<int32_t> left((size_t)R);
    int rc = [&]() -> int {
        HIP_TRY(c, ev.mark());
        if (batched) {
            // the acc of the refinements in place: the starts and their error words, then
            // the starts' aggregates into replica 0 of every chain's slab
            GS_TRY(bs.enqueue(c, b.pwms, b.pos, b.err, b.erri));
            HIP_TRY(c, hipMemsetAsync(b.agg, 0, (size_t)(R * agg_elems) * 8, c->stream));
            StartsBatchArgs ab{};
            ab.n_chains = R;
            ab.blocks = ablocks;
            ab.src = 2;
            ab.E = c->E;
            ab.comp = c->d_comp;
            ab.pos = b.pos;
            ab.agg_out = b.agg;
            ab.agg_out_chain = agg_elems;
            HIP_TRY(c, gs_starts_batch_agg_launch(bs.sa, ab, c->stream));
        }
        for (int32_t r = 0; !batched && r < R; ++r) {
            GS_TRY(chain_starts(c, mode, W, pc, seeds[r], starts.row(c, r), cpart));
            // the acc of the refinements (site_upload): the starts, their aggregates
            GS_TRY(set_snapshot_dev(c, W, c->d_pos[1], false));
            GS_TRY(b.take_chain(c, r));
        }
        GS_TRY(clear_ctx_error_words(c));
        HIP_TRY(c, hipMemsetAsync(b.passes, 0, (size_t)R * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(stage_passes, 0, (size_t)R * 12, c->stream));
        HIP_TRY(c, ev.mark());
        GS_TRY(b.launch(c, a, R, waves, lds));
        HIP_TRY(c, ev.mark());
        const int32_t dirs[2] = {-1, 1};
        for (int st = 0; st < 2; ++st) {
            HIP_TRY(c, gs_site_batch_ctl_launch(R, 0, 1 + st, max_passes, d_run, d_moved, b.err,
                                                stage_passes, d_left, c->stream));
            for (int32_t pass = 1; pass <= max_passes; ++pass) {
                HIP_TRY(c, hipMemsetAsync(b.agg, 0, (size_t)(R * agg_elems) * 8, c->stream));
                HIP_TRY(c, gs_site_batch_pass_launch(sa, (size_t)slds, R, dirs[st], c->E, c->d_comp,
                                                     d_run, d_moved, shifted, ablocks, scan_blocks,
                                                     c->stream));
                HIP_TRY(c, gs_site_batch_ctl_launch(R, pass, 1 + st, max_passes, d_run, d_moved,
                                                    b.err, stage_passes, d_left, c->stream));
                HIP_TRY(c, hipMemcpyAsync(left.data(), d_left, (size_t)R * 4, hipMemcpyDeviceToHost,
                                          c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                if (std::all_of(left.begin(), left.end(), [](int32_t v) { return v == 0; })) break;
            }
        }
        HIP_TRY(c, ev.mark());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    scratch_used(c);
    GS_TRY(ev.finish(rc, c->site_batch_ms));
    c->last_greedy_waves = waves;
    std::vector<int32_t> herr((size_t)R), hpass((size_t)R), hstage((size_t)R * 3);
    std::vector<unsigned long long> hidx((size_t)R);
    HIP_TRY(c, hipMemcpy(herr.data(), b.err, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hidx.data(), b.erri, (size_t)R * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hpass.data(), b.passes, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hstage.data(), stage_passes, (size_t)R * 12, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pos_out, b.pos, (size_t)(R * n) * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(score_out, b.pwms, (size_t)(R * n) * 8, hipMemcpyDeviceToHost));
    for (int32_t r = 0; passes_out && r < R; ++r) {
        passes_out[3 * r] = hpass[(size_t)r];
        passes_out[3 * r + 1] = hstage[(size_t)r * 3 + 1];
        passes_out[3 * r + 2] = hstage[(size_t)r * 3 + 2];
    }
    return report_chain_errors(c, herr, hidx, status_out);
}

// R independent doMotifSampling runs with Positions lists (.fs:1034-1038, any
// motifAmount), DESIGN.md §9.12.  Stage 1, chain after chain on the context's
// single-chain state and stream, no host wait in between (or, under batched_starts, all
// chains in the launches of BatchStarts and one list conversion): starts (seed r) as the
// lists of slab r.  Stage 2: the aggregates of every chain's starts and sweep 0 over the
// (chain, target) pairs, one host wait per arena round for all chains.  Stage 3: the
// greedy passes, speculative steps of two launches for all chains, one host wait per
// kSpecBatch steps; chains whose arena overflowed start again from the kept sweep output
// with a larger one.  One download.  The caller validated the arguments.
int multi_batch(gs_ctx *c, int32_t M, int32_t W, double pc, double cutoff, const uint64_t *seeds,
                int32_t R, int32_t mode, int32_t max_passes, int32_t cap, int32_t *cnt_out,
                int32_t *pos_out, double *pwms_out, int32_t *passes_out, int32_t *status_out) {
    const int64_t n = c->n_local;
    for (int i = 0; i < 3; ++i) c->multi_batch_ms[i] = 0.0;
    for (int i = 0; i < 4; ++i) c->multi_batch_info[i] = 0;
    if (n == 0) return no_targets(R, passes_out, 1, status_out);
    MultiArgs a{};
    const int64_t lds = multi_args(c, a, M, W, cap, pc, cutoff, true);
    GS_TRY(multi_lds_check(c, lds));
    GS_TRY(ensure_state(c, W));
    const int32_t cells = c->A * W + c->A;
    const int64_t sweep_arena = std::max<int64_t>(2048, 4 * (int64_t)a.kmax);
    const int64_t greedy_arena = std::max<int64_t>(4096, 8 * (int64_t)a.kmax);
    auto slot_bytes = [&](int64_t arena) { return (2 * (int64_t)a.kmax + 3 * arena) * 8; };
    const int64_t sweep_grid0 = std::max<int64_t>(
        1, std::min<int64_t>(std::min<int64_t>((int64_t)R * n, (int64_t)c->n_cu * 8),
                             kArenaBudget / slot_bytes(sweep_arena)));
    if ((int64_t)R * slot_bytes(greedy_arena) > kBatchBytesMax)
        return fail(c, GS_E_UNSUPPORTED,
                    "gs_motif_sampling_multi_batch: one arena per chain takes more than a batch "
                    "may hold: split the seeds over several calls");
    const int32_t slots0 = multi_batch_slots(c, R, slot_bytes(greedy_arena));
    const int64_t cpart_bytes = mode == 0 ? c->n_global * c->A * W * 4 : 0;
    // per chain: three list slabs, two PWMS slabs, two aggregate rows, error word, seed,
    // control block, chain index, speculation results; per pair: overflow and rescoring
    // lists (and the shared draws); the first rounds' arenas
    GS_TRY(batch_bytes_refuse(
        c, "gs_motif_sampling_multi_batch",
        (int64_t)R * (n * (3 * (4 + 4 * (int64_t)cap) + 16 + 8 + (mode == 1 ? 4 : 0)) +
                      (int64_t)cells * 16 + 8 + 8 + (int64_t)sizeof(SpecCtl) + 4 +
                      (int64_t)slots0 * (int64_t)sizeof(SpecRes)) +
            cpart_bytes +
            std::max(sweep_grid0 * slot_bytes(sweep_arena),
                     (int64_t)R * slots0 * slot_bytes(greedy_arena))));
    // the slabs (row r = chain r)
    DevBuf<int32_t> b_cnt[3], b_pos[3];  // starts as lists, sweep output, live
    DevBuf<double> b_pwms[2];            // sweep output, live
    DevBuf<int64_t> b_agg[2];            // of the starts, live
    DevBuf<unsigned long long> b_err;
    DevBuf<uint64_t> b_seeds;
    DevBuf<SpecCtl> b_ctl;
    DevBuf<SpecRes> b_res;
    DevBuf<int32_t> b_ovf, b_pairs, b_chains, cpart;
    SharedStarts starts;
    const int64_t rows = (int64_t)R * n;
    for (auto &q : b_cnt) GS_TRY(q.alloc(c, rows));
    for (auto &q : b_pos) GS_TRY(q.alloc(c, rows * cap));
    for (auto &q : b_pwms) GS_TRY(q.alloc(c, rows));
    for (auto &q : b_agg) GS_TRY(q.alloc(c, (int64_t)R * cells));
    GS_TRY(b_err.alloc(c, R));
    GS_TRY(b_seeds.alloc(c, R));
    GS_TRY(b_ctl.alloc(c, R));
    GS_TRY(b_res.alloc(c, (int64_t)R * slots0));
    GS_TRY(b_ovf.alloc(c, rows + 1));
    GS_TRY(b_pairs.alloc(c, rows));
    GS_TRY(b_chains.alloc(c, R));
    BatchStarts bs;
    DevBuf<int32_t> s_err;             // batched starts: the chains' (code, index) words
    DevBuf<unsigned long long> s_erri;
    const bool batched = batched_starts(c);
    if (batched) {
        GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
        GS_TRY(s_err.alloc(c, R));
        GS_TRY(s_erri.alloc(c, R));
    } else if (mode == 0)
        GS_TRY(cpart.alloc(c, std::max<int64_t>(cpart_bytes, 4) / 4));
    else
        GS_TRY(starts.draw(c, W, seeds, R));
    std::vector<int32_t> live((size_t)R);  // the chains of a greedy round
    for (int32_t r = 0; r < R; ++r) live[(size_t)r] = r;
    HIP_TRY(c, hipMemcpyAsync(b_seeds, seeds, (size_t)R * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b_chains, live.data(), (size_t)R * 4, hipMemcpyHostToDevice,
                              c->stream));
    MultiBatchArgs ba{};
    ba.n_chains = R;
    ba.slots = slots0;
    ba.cells = cells;
    ba.chains = b_chains;
    ba.seeds = b_seeds;
    ba.err = b_err;
    ba.ctl = b_ctl;
    ba.res = b_res;
    ba.ovf_count = b_ovf;
    ba.ovf_list = b_ovf + 1;
    a.u = nullptr;
    a.stream = stream_sweep(0);
    a.max_passes = max_passes;
    a.targets = nullptr;
    a.n_targets = 0;
    const int ablocks = agg_blocks(c, n, R);
    std::vector<SpecCtl> hctl((size_t)R);
    std::vector<unsigned long long> herr((size_t)R);
    int32_t info[4] = {0, 0, 0, slots0};
    // chains whose categories pass kArenaMax: their word takes kMultiErrUnsupported
    auto give_up = [&](const std::vector<int32_t> &chains) -> int {
        for (int32_t r : chains) {
            const unsigned long long w = ((unsigned long long)c->global_offset << 4) |
                                         (unsigned long long)kMultiErrUnsupported;
            HIP_TRY(c, hipMemcpyAsync(b_err + r, &w, 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
        return GS_OK;
    };
    StageEvents<4> ev(c);
    int rc = [&]() -> int {
        // ---- stage 1: every chain's starts, as lists ----
        HIP_TRY(c, ev.mark());
        if (batched) {
            // (the sweep's output slabs are free until stage 2: scores and starts go there)
            GS_TRY(bs.enqueue(c, b_pwms[0], b_cnt[1], s_err, s_erri));
            HIP_TRY(c, gs_starts_batch_lists_launch(b_cnt[1], rows, cap, b_cnt[0], b_pos[0], R, s_err,
                                                    s_erri, b_err, b_ctl, c->stream));
        }
        for (int32_t r = 0; !batched && r < R; ++r) {
            GS_TRY(chain_starts(c, mode, W, pc, seeds[r], starts.row(c, r), cpart));
            HIP_TRY(c, gs_multi_batch_lists_launch(c->d_pos[1], (int32_t)n, cap, b_cnt[0] + r * n,
                                                   b_pos[0] + r * n * cap, c->d_err_code,
                                                   c->d_err_index, b_err + r, b_ctl + r,
                                                   c->stream));
        }
        GS_TRY(clear_ctx_error_words(c));
        HIP_TRY(c, ev.mark());
        // ---- stage 2: aggregates of the starts, sweep 0 of every chain ----
        a.cnt_in = b_cnt[0];
        a.pos_in = b_pos[0];
        a.cnt_out = b_cnt[1];
        a.pos_out = b_pos[1];
        a.pwms_out = b_pwms[0];
        a.agg = b_agg[0];
        a.agg_rw = b_agg[1];
        HIP_TRY(c, hipMemsetAsync(b_agg[0], 0, (size_t)R * cells * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(b_pos[1], 0xff, (size_t)(rows * cap) * 4, c->stream));
        HIP_TRY(c, gs_multi_batch_agg_launch(a, ba, b_agg[0], ablocks, c->stream));
        ba.pairs = nullptr;
        ba.n_pairs = rows;
        for (int64_t arena = sweep_arena;;) {
            int64_t grid = std::min<int64_t>(ba.n_pairs, (int64_t)c->n_cu * 8);
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, kArenaBudget / slot_bytes(arena)));
            GS_TRY(multi_scratch(c, a, grid, arena));
            HIP_TRY(c, hipMemsetAsync(b_ovf, 0, 4, c->stream));
            HIP_TRY(c, gs_multi_batch_sweep_launch(a, ba, (int)grid, (size_t)lds, c->stream));
            int32_t novf = 0;
            HIP_TRY(c, hipMemcpyAsync(&novf, b_ovf, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (novf == 0) break;
            if (arena * 16 > kArenaMax) {
                std::vector<int32_t> pairs((size_t)novf), chains;
                HIP_TRY(c, hipMemcpy(pairs.data(), b_ovf + 1, (size_t)novf * 4,
                                     hipMemcpyDeviceToHost));
                for (int32_t p : pairs) chains.push_back((int32_t)(p / n));
                std::sort(chains.begin(), chains.end());
                chains.erase(std::unique(chains.begin(), chains.end()), chains.end());
                GS_TRY(give_up(chains));
                break;
            }
            arena *= 16;
            ++info[0];
            HIP_TRY(c, hipMemcpyAsync(b_pairs, b_ovf + 1, (size_t)novf * 4, hipMemcpyDeviceToDevice,
                                      c->stream));
            ba.pairs = b_pairs;
            ba.n_pairs = novf;
        }
        HIP_TRY(c, ev.mark());
        // ---- stage 3: greedy passes from the sweep's lists (kept for restarts) ----
        HIP_TRY(c, hipMemcpyAsync(b_cnt[2], b_cnt[1], (size_t)rows * 4, hipMemcpyDeviceToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(b_pos[2], b_pos[1], (size_t)(rows * cap) * 4,
                                  hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(b_pwms[1], b_pwms[0], (size_t)rows * 8, hipMemcpyDeviceToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemsetAsync(b_agg[1], 0, (size_t)R * cells * 8, c->stream));
        HIP_TRY(c, gs_multi_batch_ctl_launch(ba, R, c->stream));
        a.cnt_in = a.cnt_out = b_cnt[2];
        a.pos_in = a.pos_out = b_pos[2];
        a.pwms_out = b_pwms[1];
        a.agg = b_agg[1];
        HIP_TRY(c, gs_multi_batch_agg_launch(a, ba, b_agg[1], ablocks, c->stream));
        const int64_t step_limit = ((int64_t)n + 1) * max_passes + kSpecBatch;
        std::vector<int32_t> next;
        for (int64_t arena = greedy_arena;; arena *= 16) {
            // the chains of this arena size, as many at a time as the arena budget holds
            const int64_t group = std::max<int64_t>(1, kArenaBudget / slot_bytes(arena));
            next.clear();
            for (size_t g0 = 0; g0 < live.size(); g0 += (size_t)group) {
                const int32_t ng = (int32_t)std::min<size_t>((size_t)group, live.size() - g0);
                ba.n_chains = ng;
                ba.slots = std::min(slots0, multi_batch_slots(c, ng, slot_bytes(arena)));
                if (arena != greedy_arena || ng != R) {
                    HIP_TRY(c, hipMemcpyAsync(b_chains, live.data() + g0, (size_t)ng * 4,
                                              hipMemcpyHostToDevice, c->stream));
                    if (arena != greedy_arena) {
                        HIP_TRY(c, gs_multi_batch_restart_launch(ba, (int32_t)n, cap, b_cnt[1],
                                                                 b_pos[1], b_pwms[0], b_cnt[2],
                                                                 b_pos[2], b_pwms[1], b_agg[1],
                                                                 c->stream));
                        HIP_TRY(c, gs_multi_batch_agg_launch(a, ba, b_agg[1], ablocks, c->stream));
                    }
                }
                GS_TRY(multi_scratch(c, a, (int64_t)ng * ba.slots, arena));
                bool running = true;
                for (int64_t steps = 0; running && steps <= step_limit; steps += kSpecBatch) {
                    HIP_TRY(c, gs_multi_batch_spec_launch(a, ba, c->tune.multi_greedy_threads,
                                                          (size_t)lds, kSpecBatch, c->stream));
                    HIP_TRY(c, hipMemcpyAsync(hctl.data(), b_ctl, (size_t)R * sizeof(SpecCtl),
                                              hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                    running = false;
                    for (int32_t i = 0; i < ng; ++i)
                        running |= !hctl[(size_t)live[g0 + (size_t)i]].done;
                }
                if (running) return fail(c, GS_E_HIP, "list-path greedy made no progress");
                HIP_TRY(c, hipMemcpy(herr.data(), b_err, (size_t)R * 8, hipMemcpyDeviceToHost));
                for (int32_t i = 0; i < ng; ++i) {
                    const int32_t r = live[g0 + (size_t)i];
                    if (herr[(size_t)r] != ~0ull && (int)(herr[(size_t)r] & 15ull) == kMultiErrArena)
                        next.push_back(r);
                }
            }
            if (next.empty()) break;
            if (arena * 16 > kArenaMax) {
                GS_TRY(give_up(next));
                break;
            }
            ++info[1];
            info[2] += (int32_t)next.size();
            live = next;
        }
        HIP_TRY(c, ev.mark());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    scratch_used(c);
    GS_TRY(ev.finish(rc, c->multi_batch_ms));
    for (int i = 0; i < 4; ++i) c->multi_batch_info[i] = info[i];
    // ---- stage 4: one download ----
    HIP_TRY(c, hipMemcpyAsync(cnt_out, b_cnt[2], (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(pos_out, b_pos[2], (size_t)(rows * cap) * 4, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(pwms_out, b_pwms[1], (size_t)rows * 8, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(hctl.data(), b_ctl, (size_t)R * sizeof(SpecCtl), hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipMemcpyAsync(herr.data(), b_err, (size_t)R * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int32_t r = 0; passes_out && r < R; ++r) passes_out[r] = hctl[(size_t)r].pass;
    return report_chain_errors(c, herr, status_out,
                               "a sequence has more than 2^28 motif combinations (.fs:727-742)");
}

// R independent chains of T synchronous sweeps (motifAmount = 1), DESIGN.md §9.13.  Stage
// 1: the chains' starts, uploaded rows (mode -1) or, chain after chain on the context's
// single-chain state and stream as in multi_batch (or all at once, batched_starts: the
// starts' position slab is the chains'), those of getPWMOfRandomStarts; then the
// aggregates of every chain's starts.  Stage 2: T launches of gs_run_batch_sweep_kernel
// over the (chain, target) pairs back to back, positions double-buffered, the aggregate
// rows rotating over three buffers (the next one zeroed by a memset before the sweep that
// fills it, or by the sweep before: tune.run_batch_clear).  One synchronisation, one
// download.  The caller validated the arguments.
//
// With statistics (gs_motif_run_batch_stats) every counted sweep writes its
// PWMS as the last one does and is followed on the stream by one launch of
// gs_run_batch_stats_kernel, which reads the rows and skip words that sweep left; the
// chains' histograms, traces and best states come down with the rows.
int run_batch(gs_ctx *c, int32_t W, double pc, double cutoff, int32_t T, const uint64_t *seeds,
              int32_t R, int64_t first_sweep, int32_t mode, const double *u, int32_t *pos_inout,
              double *pwms_out, int32_t *status_out, const RunStats *stats) {
    const int64_t n = c->n_local;
    c->run_batch_ms[0] = c->run_batch_ms[1] = 0.0;
    if (status_out) std::fill(status_out, status_out + R, (int32_t)GS_OK);
    if (stats && !stats->any()) stats = nullptr;
    const CountPlan plan = stats ? stats->plan(T) : CountPlan{T, 1, T};
    const int64_t n_counted = plan.n_counted();
    if (n == 0) return stats ? stats_of_nothing(c, W, R, n_counted, *stats) : GS_OK;
    const int64_t H = stats ? occupancy_offsets(c, W, nullptr) : 0;
    // the bins are kept on the device for the caller or for the summary (§9.28), and come
    // down only for the caller
    const SummaryOut *sum = stats && stats->summed() ? stats->sum : nullptr;
    const AgreementOut *agr = stats && stats->agreed() ? stats->agr : nullptr;
    const StatsWant want = stats ? stats->want() : StatsWant{};
    MultiArgs a{};
    const int64_t lds = multi_args(c, a, 1, W, 1, pc, cutoff, false);
    GS_TRY(multi_lds_check(c, lds));
    const int32_t cells = c->A * W + c->A;
    const int64_t rows = (int64_t)R * n, agg_elems = (int64_t)R * cells + R;
    const int64_t cpart_bytes = mode == 0 ? c->n_global * c->A * W * 4 : 0;
    const int64_t u_elems = u ? rows * T : 0;
    int blocks = 0;
    HIP_TRY(c, gs_run_batch_occupancy(&blocks, (size_t)lds));
    blocks = std::max(1, std::min(blocks, c->tune.run_batch_blocks));
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>(rows, (int64_t)c->n_cu * blocks));
    // per chain: two position rows, a PWMS row, three aggregate rows and skip words, error
    // word, seed, control block (and the shared draws); the explicit uniforms; the window
    // scores of a workgroup when they do not fit in LDS
    GS_TRY(batch_bytes_refuse(
        c, "gs_motif_run_batch",
        (int64_t)R * (n * (8 + 8 + (mode == 1 ? 4 : 0)) + 3 * 8 * ((int64_t)cells + 1) + 8 + 8 +
                      (int64_t)sizeof(SpecCtl)) +
            n * 4 + u_elems * 8 + cpart_bytes + grid * 16 * (int64_t)a.kmax +
            stats_bytes(R, n, H, n_counted, 1, 1, false, want) +
            (sum ? sum->bytes(R, n, cells, 1) : 0) + (agr ? agreement_bytes(R, n) : 0)));
    if (mode >= 0) GS_TRY(ensure_state(c, W));
    GS_TRY(multi_scratch(c, a, grid, 0));
    // the slabs (row r = chain r)
    DevBuf<int32_t> b_pos[2];
    DevBuf<int64_t> b_agg[3];  // rows, then the chains' skip words
    DevBuf<double> b_pwms, b_u;
    DevBuf<unsigned long long> b_err;
    DevBuf<uint64_t> b_seeds;
    DevBuf<SpecCtl> b_ctl;
    DevBuf<int32_t> b_cnt, cpart;
    SharedStarts starts;
    BatchStarts bs;
    DevBuf<int32_t> s_err;  // batched starts: the chains' (code, index) words
    DevBuf<unsigned long long> s_erri;
    for (auto &q : b_pos) GS_TRY(q.alloc(c, rows));
    for (auto &q : b_agg) GS_TRY(q.alloc(c, agg_elems));
    GS_TRY(b_pwms.alloc(c, rows));
    GS_TRY(b_err.alloc(c, R));
    GS_TRY(b_seeds.alloc(c, R));
    if (u_elems > 0) {
        GS_TRY(b_u.alloc(c, u_elems));
        HIP_TRY(c, hipMemcpyAsync(b_u, u, (size_t)u_elems * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(b_seeds, seeds, (size_t)R * 8, hipMemcpyHostToDevice, c->stream));
    for (auto &q : b_agg) HIP_TRY(c, hipMemsetAsync(q, 0, (size_t)agg_elems * 8, c->stream));
    // the statistics' slab; every counted sweep's launch writes its own trace entry of
    // every chain
    StatsSlab st(c);
    SummaryRun srun(c);
    AgreementRun arun(c);
    if (stats) GS_TRY(st.init(W, R, H, n_counted, 1, 1, false, want));
    RunStatsArgs sa{};
    sa.n_chains = R;
    sa.n_local = (int32_t)n;
    sa.atomic = c->tune.run_stats_atomic;
    sa.H = H;
    sa.ic_stride = n_counted;
    sa.off = st.dev<int64_t>(kStatOff);
    sa.occ = st.dev<int32_t>(kStatOcc);
    sa.best_sweep = st.dev<int64_t>(kStatBestSweep);
    sa.best_ic = st.dev<double>(kStatBestIc);
    sa.best_pos = st.dev<int32_t>(kStatBestPos);
    sa.best_pwms = st.dev<double>(kStatBestPwms);
    const int sblocks = c->tune.run_stats_blocks > 0 ? c->tune.run_stats_blocks : agg_blocks(c, n, R);
    RunBatchArgs ba{};
    ba.n_chains = R;
    ba.cells = cells;
    ba.seeds = b_seeds;
    ba.err = b_err;
    ba.n_pairs = rows;
    ba.u_stride = (int64_t)T * n;
    const bool clear_in_kernel = c->tune.run_batch_clear == 1;
    const int ablocks = agg_blocks(c, n, R);
    StageEvents<3> ev(c);
    int rc = [&]() -> int {
        // ---- stage 1: every chain's starts and their aggregates ----
        HIP_TRY(c, ev.mark());
        if (mode < 0) {
            HIP_TRY(c, hipMemcpyAsync(b_pos[0], pos_inout, (size_t)rows * 4, hipMemcpyHostToDevice,
                                      c->stream));
            HIP_TRY(c, hipMemsetAsync(b_err, 0xff, (size_t)R * 8, c->stream));
        } else {
            GS_TRY(b_cnt.alloc(c, n));
            GS_TRY(b_ctl.alloc(c, R));
            const bool batched = batched_starts(c);
            if (batched) {
                // lists of capacity 1: the starts' position slab is the chains' (the PWMS
                // slab, free until the last sweep, takes the scores)
                GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
                GS_TRY(s_err.alloc(c, R));
                GS_TRY(s_erri.alloc(c, R));
                GS_TRY(bs.enqueue(c, b_pwms, b_pos[0], s_err, s_erri));
                HIP_TRY(c, gs_starts_batch_lists_launch(b_pos[0], rows, 1, nullptr, nullptr, R,
                                                        s_err, s_erri, b_err, b_ctl, c->stream));
            } else if (mode == 0)
                GS_TRY(cpart.alloc(c, std::max<int64_t>(cpart_bytes, 4) / 4));
            else
                GS_TRY(starts.draw(c, W, seeds, R));
            for (int32_t r = 0; !batched && r < R; ++r) {
                GS_TRY(chain_starts(c, mode, W, pc, seeds[r], starts.row(c, r), cpart));
                // lists of capacity 1 are the position rows; a chain that raised keeps its word
                HIP_TRY(c, gs_multi_batch_lists_launch(c->d_pos[1], (int32_t)n, 1, b_cnt,
                                                       b_pos[0] + r * n, c->d_err_code,
                                                       c->d_err_index, b_err + r, b_ctl + r,
                                                       c->stream));
            }
            GS_TRY(clear_ctx_error_words(c));
        }
        ba.pos_in = b_pos[0];
        ba.agg_out = b_agg[0];
        HIP_TRY(c, gs_run_batch_agg_launch(a, ba, ablocks, c->stream));
        HIP_TRY(c, ev.mark());
        // ---- stage 2: T sweeps of every chain, no host wait in between ----
        for (int32_t t = 0; t < T; ++t) {
            const int cur = t % 3, nxt = (t + 1) % 3, aft = (t + 2) % 3;
            // buffer nxt is zero from the start (t < 2), from sweep t - 1, or from here
            if (!clear_in_kernel && t >= 2)
                HIP_TRY(c, hipMemsetAsync(b_agg[nxt], 0, (size_t)agg_elems * 8, c->stream));
            ba.pos_in = b_pos[t & 1];
            ba.pos_out = b_pos[(t + 1) & 1];
            const bool count = stats && plan.counted(t);
            ba.pwms_out = t == T - 1 || (count && (want.ic || want.best)) ? b_pwms.p : nullptr;
            ba.agg_in = b_agg[cur];
            ba.agg_out = b_agg[nxt];
            ba.agg_clear = clear_in_kernel && t >= 1 ? b_agg[aft].p : nullptr;
            ba.u = b_u ? b_u + (int64_t)t * n : nullptr;
            a.stream = stream_sweep((uint64_t)(first_sweep + t));
            HIP_TRY(c, gs_run_batch_sweep_launch(a, ba, (int)grid, (size_t)lds, c->stream));
            if (count) {  // the consumer of this sweep's state, before the next sweep's launch
                sa.skip = b_agg[nxt] + (int64_t)R * cells;
                sa.pos = b_pos[(t + 1) & 1];
                sa.pwms = b_pwms;
                sa.ic = want.ic ? st.dev<double>(kStatIc) + plan.slot(t) : nullptr;
                sa.sweep = first_sweep + t;
                HIP_TRY(c, gs_run_batch_stats_launch(sa, sblocks, c->stream));
            }
        }
        HIP_TRY(c, ev.mark());
        // the reduction of the bins as the last statistics launch left them
        if (sum) GS_TRY(srun.enqueue(W, 1, sa.occ, nullptr, sa.off, H, R, n_counted, *sum));
        // the chains against their pool, which the summary decided if it has the pooled outputs
        if (agr)
            GS_TRY(arun.enqueue(sa.occ, sa.off, H, R, n_counted, srun.dev<int32_t>(kPoolFlags),
                                srun.dev<int32_t>(kNPooled), nullptr));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    // uploaded rows never touched the single-chain buffers: only the snapshot goes
    if (mode >= 0)
        scratch_used(c);
    else
        c->have_state = false;
    GS_TRY(ev.finish(rc, c->run_batch_ms));
    // ---- stage 3: one download ----
    std::vector<unsigned long long> herr((size_t)R);
    if (T > 0 || mode >= 0)
        HIP_TRY(c, hipMemcpyAsync(pos_inout, b_pos[T & 1], (size_t)rows * 4, hipMemcpyDeviceToHost,
                                  c->stream));
    if (T > 0)
        HIP_TRY(c, hipMemcpyAsync(pwms_out, b_pwms, (size_t)rows * 8, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipMemcpyAsync(herr.data(), b_err, (size_t)R * 8, hipMemcpyDeviceToHost, c->stream));
    if (stats) GS_TRY(st.download(*stats));
    if (sum) {
        GS_TRY(srun.download(*sum));
        srun.finish();
    }
    if (agr) {
        GS_TRY(arun.download(*agr));
        arun.finish();
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return report_chain_errors(c, herr, status_out, nullptr);
}

// Bins of one chain's occupancy histogram (gs_occupancy_offsets): off[n + 1] = off[n] + 1 +
// (L_n - W + 1), off nullable.  The total H, or -1 for a bad W or no sequences.
int64_t occupancy_offsets(const gs_ctx *c, int32_t W, int64_t *off) {
    if (!c->d_seq || c->n_local <= 0 || W < 1 || W > 64 || c->Lmin < W) return -1;
    int64_t h = 0;
    for (int64_t i = 0; i < c->n_local; ++i) {
        if (off) off[i] = h;
        h += 1 + (c->h_len[(size_t)i] - W + 1);
    }
    if (off) off[c->n_local] = h;
    return h;
}

// The statistics' device side: one slab, the parts that start from zero
// first (one memset), best_sweep and a list's best positions all-ones.
StatsSlab::~StatsSlab() {
    if (mem) (void)hipStreamSynchronize(c->stream);
    dfree(mem);
}

int StatsSlab::init(int32_t W, int64_t R, int64_t H, int64_t n_counted, int64_t cap, int64_t M,
                    bool list, const StatsWant &w) {
    lay = stats_slab(R, c->n_local, H, n_counted, cap, M, list, w);
    HIP_TRY(c, hipMalloc(&mem, (size_t)std::max<int64_t>(lay.total, 8)));
    if (lay.zeroed > 0) HIP_TRY(c, hipMemsetAsync(mem, 0, (size_t)lay.zeroed, c->stream));
    for (const int part : {(int)kStatBestSweep, (int)kStatBestPos}) {
        const Part &p = lay.part[part];
        if (p.bytes() > 0 && !p.zero)
            HIP_TRY(c, hipMemsetAsync(mem + p.off, 0xff, (size_t)p.bytes(), c->stream));
    }
    if (w.occ) {
        h_off.resize((size_t)c->n_local + 1);
        occupancy_offsets(c, W, h_off.data());
        HIP_TRY(c, hipMemcpyAsync(mem + lay.part[kStatOff].off, h_off.data(), h_off.size() * 8,
                                  hipMemcpyHostToDevice, c->stream));
    }
    return GS_OK;
}

int StatsSlab::download(int part, void *dst) const {
    const Part &p = lay.part[part];
    if (dst && p.bytes() > 0)
        HIP_TRY(c, hipMemcpyAsync(dst, mem + p.off, (size_t)p.bytes(), hipMemcpyDeviceToHost,
                                  c->stream));
    return GS_OK;
}

int StatsSlab::download(const RunStats &st) const {
    GS_TRY(download(kStatOcc, st.occ_out));
    GS_TRY(download(kStatSites, st.sites_out));
    GS_TRY(download(kStatIc, st.ic_out));
    GS_TRY(download(kStatBestSweep, st.best_sweep_out));
    GS_TRY(download(kStatBestCnt, st.best_cnt_out));
    GS_TRY(download(kStatBestPos, st.best_pos_out));
    return download(kStatBestPwms, st.best_pwms_out);
}

// No sequences: no bins, no counted sweep completes, and the summary is that of nothing.
int stats_of_nothing(const gs_ctx *c, int32_t W, int64_t R, int64_t n_counted, const RunStats &st) {
    if (st.ic_out) std::fill(st.ic_out, st.ic_out + R * n_counted, std::nan(""));
    if (st.best_sweep_out) std::fill(st.best_sweep_out, st.best_sweep_out + R, (int64_t)-1);
    if (st.sum) summary_of_nothing(c, W, R, *st.sum);
    if (st.agreed()) agreement_of_nothing(R, nullptr, *st.agr);
    return GS_OK;
}

// The chain summary's device side, over the table of its parts
// (summary_slab): one slab, the cells that start from zero first (one memset).
SummaryRun::~SummaryRun() {
    if (slab) (void)hipStreamSynchronize(c->stream);
    dfree(slab);
    for (hipEvent_t e : ev)
        if (e) c->ev_pool.push_back(e);
}

int SummaryRun::enqueue(int32_t W, int32_t M, const int32_t *d_occ, const int32_t *d_sites,
                        const int64_t *d_off, int64_t H, int32_t R, int64_t n_counted,
                        const SummaryOut &out) {
    const int64_t n = c->n_local;
    c->summary_ms = 0.0;
    if (R <= 0 || n <= 0 || !out.any()) return GS_OK;
    const bool want[kSummaryGroups] = {out.modes(), out.counts(), out.pool()};
    lay = summary_slab(R, n, (int64_t)c->A * W + c->A, M, out.list, want);
    HIP_TRY(c, hipMalloc(&slab, (size_t)std::max<int64_t>(lay.total, 8)));
    if (lay.zeroed > 0) HIP_TRY(c, hipMemsetAsync(slab, 0, (size_t)lay.zeroed, c->stream));
    // a wavefront a row, four a workgroup: eight rows a wavefront (a workgroup's cells cost
    // up to A W + A atomic adds at its end) while the GPU is eight deep over all views (what
    // its registers allow: a row is a chain of dependent loads, hidden by other rows only)
    const int64_t views = R + (want[kGroupPool] ? 1 : 0);
    const int blocks = (int)std::max<int64_t>(
        1, std::min<int64_t>((n + 31) / 32, std::max<int64_t>(1, (int64_t)c->n_cu * 8 / views)));
    // what both kernels' arguments share
    const auto fill = [&](auto &a) {
        a.n_chains = R;
        a.n_local = c->n_local;
        a.A = c->A;
        a.W = W;
        a.CS = c->E + 1;
        a.H = H;
        a.n_counted = n_counted;
        a.occ = d_occ;
        a.off = d_off;
        a.seq = c->d_seq;
        a.doff = c->d_doff;
        a.comp = c->d_comp;
        a.mode_pos = dev<int32_t>(kModePos);
        a.mode_count = dev<int32_t>(kModeCount);
        a.counts = dev<int64_t>(kCounts);
        a.flags = dev<int32_t>(kPoolFlags);
        a.n_pooled = dev<int32_t>(kNPooled);
        a.pool_pos = dev<int32_t>(kPoolPos);
        a.pool_count = dev<int64_t>(kPoolCount);
        a.pool_counts = dev<int64_t>(kPoolCounts);
    };
    for (hipEvent_t &e : ev) e = get_event(c);
    HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    if (out.list) {
        ListSummaryArgs a{};
        fill(a);
        a.M = M;
        a.sites = d_sites;
        a.mode_sites = dev<int32_t>(kModeSites);
        a.mode_sites_count = dev<int32_t>(kModeSitesCount);
        a.mode_cnt = dev<int32_t>(kModeCnt);
        a.pool_sites = dev<int32_t>(kPoolSites);
        a.pool_sites_count = dev<int64_t>(kPoolSitesCount);
        a.pool_cnt = dev<int32_t>(kPoolCnt);
        HIP_TRY(c, gs_list_summary_launch(a, blocks, c->stream));
    } else {
        SummaryArgs a{};
        fill(a);
        HIP_TRY(c, gs_summary_launch(a, blocks, c->stream));
    }
    HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    return GS_OK;
}

int SummaryRun::download(const SummaryOut &out) {
    for (int i = 0; slab && i < kSummaryOutputs; ++i)
        if (lay.part[i].bytes() > 0)
            HIP_TRY(c, hipMemcpyAsync(out.out[i], slab + lay.part[i].off, (size_t)lay.part[i].bytes(),
                                      hipMemcpyDeviceToHost, c->stream));
    return GS_OK;
}

void SummaryRun::finish() {
    float ms = 0.0f;
    if (ev[0] && ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->summary_ms = ms;
}

// No sequences: no modes; every chain's (empty) row sums to anything asked.
void summary_of_nothing(const gs_ctx *c, int32_t W, int64_t R, const SummaryOut &out) {
    const int64_t cells = (int64_t)c->A * W + c->A;
    if (R <= 0) return;
    if (out.counts()) std::fill_n((int64_t *)out.out[kCounts], R * cells, (int64_t)0);
    if (out.pool()) {
        std::fill_n((int64_t *)out.out[kPoolCounts], cells, (int64_t)0);
        *(int32_t *)out.out[kNPooled] = (int32_t)R;
    }
}

// gs_occupancy_summary and (sites non-null) gs_list_occupancy_summary: the caller's bins and
// site counts up, the reduction, the result down (arguments validated).  The context's
// snapshot and state are not touched.
int occupancy_summary(gs_ctx *c, int32_t W, int32_t M, const int32_t *occ, const int32_t *sites,
                      int32_t R, int64_t n_counted, const SummaryOut &out) {
    const int64_t n = c->n_local;
    if (n == 0) {
        summary_of_nothing(c, W, R, out);
        return GS_OK;
    }
    const int64_t H = occupancy_offsets(c, W, nullptr), S = (int64_t)R * n * (M + 1);
    std::vector<int64_t> h_off((size_t)n + 1);
    occupancy_offsets(c, W, h_off.data());
    SummaryRun run(c);
    DevBuf<int32_t> d_occ, d_sites;
    DevBuf<int64_t> d_off;
    GS_TRY(d_occ.alloc(c, std::max<int64_t>(1, (int64_t)R * H)));
    if (sites) GS_TRY(d_sites.alloc(c, S));
    GS_TRY(d_off.alloc(c, n + 1));
    int rc = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(d_off, h_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_occ, occ, (size_t)R * H * 4, hipMemcpyHostToDevice, c->stream));
        if (sites)
            HIP_TRY(c, hipMemcpyAsync(d_sites, sites, (size_t)S * 4, hipMemcpyHostToDevice, c->stream));
        GS_TRY(run.enqueue(W, M, d_occ, d_sites, d_off, H, R, n_counted, out));
        GS_TRY(run.download(out));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    if (rc) {  // nothing in flight on the slabs when they go
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    run.finish();
    return GS_OK;
}

// The chain agreement's device side, over the table of its parts
// (agreement_slab): one slab, the chains' sums (and a pool count decided here) first, zero.
AgreementRun::~AgreementRun() {
    if (slab) (void)hipStreamSynchronize(c->stream);
    dfree(slab);
    for (hipEvent_t e : ev)
        if (e) c->ev_pool.push_back(e);
}

int AgreementRun::enqueue(const int32_t *d_occ, const int64_t *d_off, int64_t H, int32_t R,
                          int64_t n_counted, int32_t *d_flags, const int32_t *d_count,
                          const int32_t *mask) {
    const int64_t n = c->n_local;
    c->agreement_ms = 0.0;
    if (R <= 0 || n <= 0) return GS_OK;
    const bool shared = d_flags && d_count && !mask;
    lay = agreement_slab(R, n, !shared, !mask);
    HIP_TRY(c, hipMalloc(&slab, (size_t)std::max<int64_t>(lay.total, 8)));
    if (lay.zeroed > 0) HIP_TRY(c, hipMemsetAsync(slab, 0, (size_t)lay.zeroed, c->stream));
    AgreementArgs a{};
    a.n_chains = R;
    a.n_local = c->n_local;
    a.H = H;
    a.n_counted = n_counted;
    a.occ = d_occ;
    a.off = d_off;
    a.flags = shared ? d_flags : dev<int32_t>(kAgrFlags);
    a.n_pooled = dev<int32_t>(kAgrNPooled);
    a.decide = !shared && !mask;
    a.agree = dev<int32_t>(kAgrAgree);
    a.spread = dev<int64_t>(kAgrSpread);
    a.spread_chain = dev<int32_t>(kAgrSpreadChain);
    a.chain_agree = dev<int32_t>(kAgrChainAgree);
    a.chain_dist = dev<int64_t>(kAgrChainDist);
    d_n_pooled = shared ? d_count : a.n_pooled;
    if (mask) {
        h_flags.resize((size_t)R);
        h_pooled = 0;
        for (int32_t r = 0; r < R; ++r) h_pooled += h_flags[(size_t)r] = mask[r] != 0;
        HIP_TRY(c, hipMemcpyAsync(a.flags, h_flags.data(), (size_t)R * 4, hipMemcpyHostToDevice,
                                  c->stream));
    }
    // a wavefront a row, four a workgroup; a workgroup's chains cost up to 2 R atomic adds at
    // its end, so no more workgroups than keep the GPU eight deep
    const int blocks =
        (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)c->n_cu * 8));
    for (hipEvent_t &e : ev) e = get_event(c);
    HIP_TRY(c, hipEventRecord(ev[0], c->stream));
    HIP_TRY(c, gs_agreement_launch(a, blocks, c->stream));
    HIP_TRY(c, hipEventRecord(ev[1], c->stream));
    return GS_OK;
}

int AgreementRun::download(const AgreementOut &out) {
    for (int i = 0; slab && i < kAgreementOutputs; ++i) {
        if (i == kAgrNPooled) {
            if (!d_n_pooled)
                *(int32_t *)out.out[i] = h_pooled;  // the mask's
            else
                HIP_TRY(c, hipMemcpyAsync(out.out[i], d_n_pooled, 4, hipMemcpyDeviceToHost,
                                          c->stream));
        } else if (lay.part[i].bytes() > 0)
            HIP_TRY(c, hipMemcpyAsync(out.out[i], slab + lay.part[i].off,
                                      (size_t)lay.part[i].bytes(), hipMemcpyDeviceToHost,
                                      c->stream));
    }
    return GS_OK;
}

void AgreementRun::finish() {
    float ms = 0.0f;
    if (ev[0] && ev[1] && hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
        c->agreement_ms = ms;
}

// No sequences: nothing to compare; every chain's (empty) row sums to anything asked, so
// without a mask every chain is pooled (summary_of_nothing), and a pooled chain has no
// distance and no sequence to agree on.
void agreement_of_nothing(int64_t R, const int32_t *mask, const AgreementOut &out) {
    int32_t pooled = 0;
    for (int64_t r = 0; r < R; ++r) {
        const bool f = !mask || mask[r] != 0;
        pooled += f;
        ((int64_t *)out.out[kAgrChainDist])[r] = f ? 0 : -1;
        ((int32_t *)out.out[kAgrChainAgree])[r] = f ? 0 : -1;
    }
    if (R > 0) *(int32_t *)out.out[kAgrNPooled] = pooled;
}

// gs_occupancy_agreement: the caller's bins up, the reduction, the result down (arguments
// validated).  The context's snapshot and state are not touched.
int occupancy_agreement(gs_ctx *c, int32_t W, const int32_t *occ, int32_t R, int64_t n_counted,
                        const int32_t *mask, const AgreementOut &out) {
    const int64_t n = c->n_local;
    if (n == 0) {
        agreement_of_nothing(R, mask, out);
        return GS_OK;
    }
    const int64_t H = occupancy_offsets(c, W, nullptr);
    std::vector<int64_t> h_off((size_t)n + 1);
    occupancy_offsets(c, W, h_off.data());
    AgreementRun run(c);
    DevBuf<int32_t> d_occ;
    DevBuf<int64_t> d_off;
    GS_TRY(d_occ.alloc(c, std::max<int64_t>(1, (int64_t)R * H)));
    GS_TRY(d_off.alloc(c, n + 1));
    int rc = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(d_off, h_off.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_occ, occ, (size_t)R * H * 4, hipMemcpyHostToDevice, c->stream));
        GS_TRY(run.enqueue(d_occ, d_off, H, R, n_counted, nullptr, nullptr, mask));
        GS_TRY(run.download(out));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    if (rc) {  // nothing in flight on the slabs when they go
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    run.finish();
    return GS_OK;
}

// R independent chains of T synchronous sweeps with Positions lists (any motifAmount),
// DESIGN.md §9.19.  Stage 1: the chains' lists, uploaded (mode -1) or their starts as
// one-position lists as in multi_batch; then the aggregates of every chain's lists.  Stage 2:
// per sweep one launch of gs_run_multi_batch_sweep_kernel over the (chain, target) pairs, for
// motifAmount >= 3 followed by a second one with a small grid of 16x arenas that takes the
// overflowed pairs from a device list; lists double-buffered, aggregate rows rotating over
// three buffers (the third cleared in-kernel).  One synchronisation; then, while a pair
// overflowed the larger arena as well and parked its chain at sweep t, a further round runs
// the chains parked at t from their intact snapshot of sweep t with the next arena size up,
// their aggregates rebuilt from the lists.  One download.  The caller validated the arguments.
//
// With statistics (gs_motif_run_multi_batch_stats) every counted sweep's
// launches write their PWMS as the last sweep's do, and one launch of
// gs_run_multi_batch_stats_kernel over the round's chains follows them on the stream; the
// bins, site counts, trace and running best live for the whole call, so a parked chain's
// counted sweeps before t come from the round that parked it and those from t on from the
// round that resumes it.
int run_multi_batch(gs_ctx *c, int32_t M, int32_t W, double pc, double cutoff, int32_t T,
                    const uint64_t *seeds, int32_t R, int64_t first_sweep, int32_t mode, int32_t cap,
                    const double *u, int32_t *cnt_inout, int32_t *pos_inout, double *pwms_out,
                    int32_t *status_out, const RunStats *stats) {
    const int64_t n = c->n_local;
    c->run_multi_batch_ms[0] = c->run_multi_batch_ms[1] = 0.0;
    for (int i = 0; i < 4; ++i) c->run_multi_batch_info[i] = 0;
    if (status_out) std::fill(status_out, status_out + R, (int32_t)GS_OK);
    if (stats && !stats->any()) stats = nullptr;
    const CountPlan plan = stats ? stats->plan(T) : CountPlan{T, 1, T};
    const int64_t n_counted = plan.n_counted();
    if (n == 0) return stats ? stats_of_nothing(c, W, R, n_counted, *stats) : GS_OK;
    // the bins and site counts are kept on the device for the caller or for the summary
    // (§9.29), and come down only for the caller
    const SummaryOut *sum = stats && stats->summed() ? stats->sum : nullptr;
    const StatsWant want = stats ? stats->want() : StatsWant{};
    const int64_t H = want.occ ? occupancy_offsets(c, W, nullptr) : 0;
    MultiArgs a{};
    const int64_t lds = multi_args(c, a, M, W, cap, pc, cutoff, false);
    // (the kernel stages its pick in static LDS beside the carve: both have to fit)
    size_t static_lds = 0;
    HIP_TRY(c, gs_run_multi_batch_static_lds(&static_lds));
    GS_TRY(multi_lds_check(c, lds + (int64_t)static_lds));
    const int32_t cells = c->A * W + c->A;
    const int64_t rows = (int64_t)R * n, agg_elems = (int64_t)R * cells + R;
    const int64_t cpart_bytes = mode == 0 ? c->n_global * c->A * W * 4 : 0;
    const int64_t u_elems = u ? rows * T : 0;
    // the overflow list and its count a sweep: motifAmount >= 3 only
    const int64_t ovf_elems = M >= 3 ? rows : 0, novf_elems = M >= 3 ? T : 0;
    const int64_t arena_max = c->tune.run_multi_arena_max;
    int blocks = 0;
    HIP_TRY(c, gs_run_multi_batch_occupancy(&blocks, (size_t)lds));
    blocks = std::max(1, std::min(blocks, c->tune.run_batch_blocks));
    // motifAmount = 1 builds no level; for 2, level 1 has at most kmax entries: the first
    // arena always holds it.  From 3 on a sweep has its overflow launch, while 16x arenas fit
    // (its grid: a workgroup a CU, as many as 256 MiB of 16x arenas hold)
    const int64_t kOvfGrid = c->n_cu, kOvfBytes = 256ll << 20;
    const int64_t arena0 = M == 1 ? 0 : std::max<int64_t>(2048, 4 * (int64_t)a.kmax);
    auto slot_bytes = [&](int64_t arena) { return (2 * (int64_t)a.kmax + 3 * arena) * 8; };
    auto main_grid = [&](int64_t pairs, int64_t arena) {
        const int64_t g = std::min<int64_t>(pairs, (int64_t)c->n_cu * blocks);
        return std::max<int64_t>(1, std::min<int64_t>(g, kArenaBudget / slot_bytes(arena)));
    };
    auto ovf_arena = [&](int64_t arena) -> int64_t {
        const int64_t big = arena * 16;
        return M >= 3 && big <= arena_max && slot_bytes(big) <= kOvfBytes ? big : 0;
    };
    auto ovf_grid = [&](int64_t big) {
        return std::max<int64_t>(1, std::min<int64_t>(kOvfGrid, kOvfBytes / slot_bytes(big)));
    };
    auto scratch_bytes = [&](int64_t pairs, int64_t arena) {
        const int64_t big = ovf_arena(arena);
        return std::max(main_grid(pairs, arena) * slot_bytes(arena),
                        big ? ovf_grid(big) * slot_bytes(big) : 0);
    };
    // per chain: two list slabs, a PWMS row, three aggregate rows and skip words, error and
    // park words, seed, control block, chain index (and the shared draws); the overflow
    // list and counts; the explicit uniforms; the first round's arenas
    GS_TRY(batch_bytes_refuse(
        c, "gs_motif_run_multi_batch",
        (int64_t)R * (n * (2 * (4 + 4 * (int64_t)cap) + 8 + (mode == 1 ? 4 : 0)) +
                      3 * 8 * ((int64_t)cells + 1) + 8 + 4 + 8 + (int64_t)sizeof(SpecCtl) + 4) +
            (ovf_elems + novf_elems) * 4 + u_elems * 8 + cpart_bytes +
            scratch_bytes(rows, arena0) +
            stats_bytes(R, n, H, n_counted, cap, M, true, want) +
            (sum ? sum->bytes(R, n, cells, M) : 0)));
    if (mode >= 0) GS_TRY(ensure_state(c, W));
    {  // the first round's arenas, so that no sweep waits for an allocation
        MultiArgs sized = a;
        if (const int64_t big = ovf_arena(arena0)) GS_TRY(multi_scratch(c, sized, ovf_grid(big), big));
        GS_TRY(multi_scratch(c, sized, main_grid(rows, arena0), arena0));
    }
    // the slabs (row r = chain r)
    DevBuf<int32_t> b_cnt[2], b_pos[2];
    DevBuf<int64_t> b_agg[3];  // rows, then the chains' skip words
    DevBuf<double> b_pwms, b_u;
    DevBuf<unsigned long long> b_err;
    DevBuf<uint64_t> b_seeds;
    DevBuf<SpecCtl> b_ctl;
    DevBuf<int32_t> b_park, b_chains, b_ovf, b_novf, cpart;
    SharedStarts starts;
    BatchStarts bs;
    DevBuf<int32_t> s_err;  // batched starts: the chains' (code, index) words
    DevBuf<unsigned long long> s_erri;
    for (auto &q : b_cnt) GS_TRY(q.alloc(c, rows));
    for (auto &q : b_pos) GS_TRY(q.alloc(c, rows * cap));
    for (auto &q : b_agg) GS_TRY(q.alloc(c, agg_elems));
    GS_TRY(b_pwms.alloc(c, rows));
    GS_TRY(b_err.alloc(c, R));
    GS_TRY(b_seeds.alloc(c, R));
    GS_TRY(b_park.alloc(c, R));
    GS_TRY(b_chains.alloc(c, R));
    if (ovf_elems > 0) GS_TRY(b_ovf.alloc(c, ovf_elems));
    if (novf_elems > 0) GS_TRY(b_novf.alloc(c, novf_elems));
    if (u_elems > 0) {
        GS_TRY(b_u.alloc(c, u_elems));
        HIP_TRY(c, hipMemcpyAsync(b_u, u, (size_t)u_elems * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipMemcpyAsync(b_seeds, seeds, (size_t)R * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(b_park, 0xff, (size_t)R * 4, c->stream));
    // the statistics' slab, cleared here once for all rounds; the first round's launches
    // write every chain's trace entries
    StatsSlab st(c);
    SummaryRun srun(c);
    if (stats) GS_TRY(st.init(W, R, H, n_counted, cap, M, true, want));
    RunMultiStatsArgs sa{};
    sa.n_local = (int32_t)n;
    sa.cap = cap;
    sa.M = M;
    sa.atomic = c->tune.run_stats_atomic;
    sa.H = H;
    sa.ic_stride = n_counted;
    sa.off = st.dev<int64_t>(kStatOff);
    sa.occ = st.dev<int32_t>(kStatOcc);
    sa.sites = st.dev<int32_t>(kStatSites);
    sa.best_sweep = st.dev<int64_t>(kStatBestSweep);
    sa.best_ic = st.dev<double>(kStatBestIc);
    sa.best_cnt = st.dev<int32_t>(kStatBestCnt);
    sa.best_pos = st.dev<int32_t>(kStatBestPos);
    sa.best_pwms = st.dev<double>(kStatBestPwms);
    RunMultiBatchArgs ba{};
    ba.cells = cells;
    ba.n_all = R;
    ba.seeds = b_seeds;
    ba.err = b_err;
    ba.park = b_park;
    ba.u_stride = (int64_t)T * n;
    a.u = nullptr;
    a.targets = nullptr;
    a.n_targets = 0;
    std::vector<unsigned long long> herr((size_t)R, ~0ull);
    std::vector<int32_t> hpark((size_t)R, -1), hnovf((size_t)novf_elems, 0);
    std::vector<char> given_up((size_t)R, 0);
    int32_t info[4] = {0, 0, 0, (int32_t)arena0};
    // One round: the sweeps t0 .. T - 1 of `chains` (empty: all of them, from the starts)
    // with `arena` as the first arena.
    struct Round {
        std::vector<int32_t> chains;
        int32_t t0;
        int64_t arena;
    };
    StageEvents<3> ev(c);
    auto enqueue_round = [&](const Round &rd, bool first) -> int {
        const int32_t nc = first ? R : (int32_t)rd.chains.size();
        const int64_t pairs = (int64_t)nc * n, big = ovf_arena(rd.arena);
        const int64_t grid = main_grid(pairs, rd.arena), ogrid = big ? ovf_grid(big) : 0;
        // both launches carve the same scratch: the stream runs them one after the other
        MultiArgs am = a, ao = a;
        const bool big_first = big && ogrid * slot_bytes(big) > grid * slot_bytes(rd.arena);
        if (big && big_first) GS_TRY(multi_scratch(c, ao, ogrid, big));
        GS_TRY(multi_scratch(c, am, grid, rd.arena));
        if (big && !big_first) GS_TRY(multi_scratch(c, ao, ogrid, big));
        ba.n_chains = nc;
        ba.chains = first ? nullptr : b_chains.p;
        ba.n_pairs = pairs;
        for (auto &q : b_agg) HIP_TRY(c, hipMemsetAsync(q, 0, (size_t)agg_elems * 8, c->stream));
        if (novf_elems > 0)
            HIP_TRY(c, hipMemsetAsync(b_novf, 0, (size_t)novf_elems * 4, c->stream));
        if (!first) {
            // the parked chains forget their sweep t0, its error word included
            HIP_TRY(c, hipMemcpyAsync(b_chains, rd.chains.data(), (size_t)nc * 4,
                                      hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(b_err, herr.data(), (size_t)R * 8, hipMemcpyHostToDevice,
                                      c->stream));
            HIP_TRY(c, hipMemcpyAsync(b_park, hpark.data(), (size_t)R * 4, hipMemcpyHostToDevice,
                                      c->stream));
        }
        if (T > rd.t0) {
            am.cnt_in = b_cnt[rd.t0 & 1];
            am.pos_in = b_pos[rd.t0 & 1];
            ba.agg_out = b_agg[0];
            HIP_TRY(c, gs_run_multi_batch_agg_launch(am, ba, agg_blocks(c, n, nc), c->stream));
        }
        if (first) HIP_TRY(c, ev.mark());
        for (int32_t t = rd.t0; t < T; ++t) {
            const int k = t - rd.t0, cur = k % 3, nxt = (k + 1) % 3, aft = (k + 2) % 3;
            const bool count = stats && plan.counted(t);
            for (MultiArgs *m : {&am, &ao}) {
                m->cnt_in = b_cnt[t & 1];
                m->pos_in = b_pos[t & 1];
                m->cnt_out = b_cnt[(t + 1) & 1];
                m->pos_out = b_pos[(t + 1) & 1];
                m->pwms_out = t == T - 1 || (count && (want.ic || want.best)) ? b_pwms.p : nullptr;
                m->stream = stream_sweep((uint64_t)(first_sweep + t));
            }
            ba.sweep = t;
            ba.agg_in = b_agg[cur];
            ba.agg_out = b_agg[nxt];
            ba.u = b_u ? b_u + (int64_t)t * n : nullptr;
            // buffer nxt is zero from the round's start (k < 2) or from sweep t - 1
            RunMultiBatchArgs bm = ba;
            bm.agg_clear = k >= 1 ? b_agg[aft].p : nullptr;
            bm.pairs = bm.pairs_count = nullptr;
            bm.ovf_list = big ? b_ovf.p : nullptr;
            bm.ovf_count = big ? b_novf + t : nullptr;
            HIP_TRY(c, gs_run_multi_batch_sweep_launch(am, bm, (int)grid, (size_t)lds, c->stream));
            if (big) {
                // unconditionally: an almost empty launch when the sweep listed no pair
                RunMultiBatchArgs bo = ba;
                bo.agg_clear = nullptr;
                bo.pairs = b_ovf;
                bo.pairs_count = b_novf + t;
                bo.ovf_list = bo.ovf_count = nullptr;
                HIP_TRY(c, gs_run_multi_batch_sweep_launch(ao, bo, (int)ogrid, (size_t)lds,
                                                           c->stream));
            }
            if (count) {  // the consumer of this sweep's state, before the next sweep's launch
                sa.n_chains = nc;
                sa.chains = ba.chains;
                sa.skip = b_agg[nxt] + (int64_t)R * cells;
                sa.cnt = b_cnt[(t + 1) & 1];
                sa.pos = b_pos[(t + 1) & 1];
                sa.pwms = b_pwms;
                sa.ic = want.ic ? st.dev<double>(kStatIc) + plan.slot(t) : nullptr;
                sa.sweep = first_sweep + t;
                const int sblocks = c->tune.run_stats_blocks > 0
                                        ? c->tune.run_stats_blocks
                                        : agg_blocks(c, n * cap, nc);
                HIP_TRY(c, gs_run_multi_batch_stats_launch(sa, sblocks, c->stream));
            }
        }
        return GS_OK;
    };
    int rc = [&]() -> int {
        // ---- stage 1: every chain's lists and their aggregates ----
        HIP_TRY(c, ev.mark());
        if (mode < 0) {
            HIP_TRY(c, hipMemcpyAsync(b_cnt[0], cnt_inout, (size_t)rows * 4, hipMemcpyHostToDevice,
                                      c->stream));
            HIP_TRY(c, hipMemcpyAsync(b_pos[0], pos_inout, (size_t)(rows * cap) * 4,
                                      hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemsetAsync(b_err, 0xff, (size_t)R * 8, c->stream));
        } else {
            const bool batched = batched_starts(c);
            if (batched) {
                // (the next lists' slab and the PWMS slab are free until the sweeps: the
                // starts and their scores go there)
                GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
                GS_TRY(s_err.alloc(c, R));
                GS_TRY(s_erri.alloc(c, R));
                GS_TRY(bs.enqueue(c, b_pwms, b_cnt[1], s_err, s_erri));
                HIP_TRY(c, gs_starts_batch_lists_launch(b_cnt[1], rows, cap, b_cnt[0], b_pos[0], R,
                                                        s_err, s_erri, b_err, nullptr, c->stream));
            } else if (mode == 0)
                GS_TRY(cpart.alloc(c, std::max<int64_t>(cpart_bytes, 4) / 4));
            else
                GS_TRY(starts.draw(c, W, seeds, R));
            if (!batched) GS_TRY(b_ctl.alloc(c, R));
            for (int32_t r = 0; !batched && r < R; ++r) {
                GS_TRY(chain_starts(c, mode, W, pc, seeds[r], starts.row(c, r), cpart));
                HIP_TRY(c, gs_multi_batch_lists_launch(c->d_pos[1], (int32_t)n, cap, b_cnt[0] + r * n,
                                                       b_pos[0] + r * n * cap, c->d_err_code,
                                                       c->d_err_index, b_err + r, b_ctl + r,
                                                       c->stream));
            }
            GS_TRY(clear_ctx_error_words(c));
        }
        // ---- stage 2: the sweeps, then the parked chains again with larger arenas ----
        std::vector<Round> todo;
        todo.push_back(Round{{}, 0, arena0});
        for (bool first = true; !todo.empty(); first = false) {
            const Round rd = std::move(todo.back());
            todo.pop_back();
            GS_TRY(enqueue_round(rd, first));
            if (M < 3 || T == 0) {  // no pair can overflow: nothing to look at
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                break;
            }
            HIP_TRY(c, hipMemcpyAsync(hpark.data(), b_park, (size_t)R * 4, hipMemcpyDeviceToHost,
                                      c->stream));
            HIP_TRY(c, hipMemcpyAsync(herr.data(), b_err, (size_t)R * 8, hipMemcpyDeviceToHost,
                                      c->stream));
            HIP_TRY(c, hipMemcpyAsync(hnovf.data(), b_novf, (size_t)T * 4, hipMemcpyDeviceToHost,
                                      c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (int32_t v : hnovf) info[0] += v;
            // the chains this round parked, by sweep: each group is a round of its own
            const int64_t big = ovf_arena(rd.arena), next = (big ? big : rd.arena) * 16;
            std::vector<std::pair<int32_t, int32_t>> parked;  // (sweep, chain)
            for (int32_t i = 0; i < (first ? R : (int32_t)rd.chains.size()); ++i) {
                const int32_t r = first ? i : rd.chains[(size_t)i];
                if (hpark[(size_t)r] >= 0) parked.emplace_back(hpark[(size_t)r], r);
            }
            std::sort(parked.begin(), parked.end());
            info[1] += (int32_t)parked.size();
            for (const auto &p : parked) {
                hpark[(size_t)p.second] = -1;
                herr[(size_t)p.second] = ~0ull;
                if (next > arena_max) {
                    given_up[(size_t)p.second] = 1;
                    continue;
                }
                if (todo.empty() || todo.back().t0 != p.first || todo.back().arena != next) {
                    todo.push_back(Round{{}, p.first, next});
                    ++info[2];
                }
                todo.back().chains.push_back(p.second);
            }
        }
        HIP_TRY(c, ev.mark());
        // the reduction of the bins and site counts as the last round's last statistics
        // launch left them
        if (sum) GS_TRY(srun.enqueue(W, M, sa.occ, sa.sites, sa.off, H, R, n_counted, *sum));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    // uploaded lists never touched the single-chain buffers: only the snapshot goes
    if (mode >= 0)
        scratch_used(c);
    else
        c->have_state = false;
    GS_TRY(ev.finish(rc, c->run_multi_batch_ms));
    for (int i = 0; i < 4; ++i) c->run_multi_batch_info[i] = info[i];
    // ---- stage 3: one download ----
    if (T > 0 || mode >= 0) {
        HIP_TRY(c, hipMemcpyAsync(cnt_inout, b_cnt[T & 1], (size_t)rows * 4, hipMemcpyDeviceToHost,
                                  c->stream));
        HIP_TRY(c, hipMemcpyAsync(pos_inout, b_pos[T & 1], (size_t)(rows * cap) * 4,
                                  hipMemcpyDeviceToHost, c->stream));
    }
    if (T > 0)
        HIP_TRY(c, hipMemcpyAsync(pwms_out, b_pwms, (size_t)rows * 8, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipMemcpyAsync(herr.data(), b_err, (size_t)R * 8, hipMemcpyDeviceToHost, c->stream));
    if (stats) GS_TRY(st.download(*stats));
    if (sum) {
        GS_TRY(srun.download(*sum));
        srun.finish();
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int32_t r = 0; r < R; ++r)
        if (given_up[(size_t)r])
            herr[(size_t)r] = ((unsigned long long)c->global_offset << 4) |
                              (unsigned long long)kMultiErrUnsupported;
    return report_chain_errors(c, herr, status_out,
                               "a sequence has more than 2^28 motif combinations (.fs:727-742)");
}

// R independent getPWMOfRandomStarts runs (.fs:589-611), DESIGN.md §9.15: the launches of
// BatchStarts on slabs of the call's own, one synchronisation, one download.  The fixed
// PCV / PPM apply as in gs_random_starts.  The caller validated the arguments.
int starts_batch(gs_ctx *c, int32_t W, double pc, const uint64_t *seeds, int32_t R, int32_t mode,
                 double *score_out, int32_t *pos_out, int32_t *status_out) {
    const int64_t n = c->n_local;
    c->starts_batch_ms[0] = c->starts_batch_ms[1] = 0.0;
    if (n == 0) return no_targets(R, nullptr, 0, status_out);
    GS_TRY(ensure_state(c, W));
    const int64_t cells = (int64_t)c->A * W + c->A;
    // per chain: scores, starts, error words, seed (and the aggregate row); one group's cpart
    GS_TRY(batch_bytes_refuse(
        c, "gs_random_starts_batch",
        (int64_t)R * (n * (8 + 4) + 4 + 8 + 8 + (mode == 1 ? cells * 8 : 0)) +
            (mode == 0 ? c->n_global * c->A * W * 4 : 0)));
    DevBuf<double> score;
    DevBuf<int32_t> pos, err;
    DevBuf<unsigned long long> erri;
    BatchStarts bs;
    GS_TRY(score.alloc(c, R * n));
    GS_TRY(pos.alloc(c, R * n));
    GS_TRY(err.alloc(c, R));
    GS_TRY(erri.alloc(c, R));
    GS_TRY(bs.prepare(c, W, pc, seeds, R, mode));
    int rc = [&]() -> int {
        GS_TRY(bs.enqueue(c, score, pos, err, erri, true));
        GS_TRY(clear_ctx_error_words(c));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return GS_OK;
    }();
    scratch_used(c);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    bs.elapsed(c, c->starts_batch_ms);
    std::vector<int32_t> herr((size_t)R);
    std::vector<unsigned long long> hidx((size_t)R);
    HIP_TRY(c, hipMemcpy(herr.data(), err, (size_t)R * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(hidx.data(), erri, (size_t)R * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(score_out, score, (size_t)(R * n) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pos_out, pos, (size_t)(R * n) * 4, hipMemcpyDeviceToHost));
    return report_chain_errors(c, herr, hidx, status_out);
}

}  // namespace gs_host
