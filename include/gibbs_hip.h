/*
 * gibbs_hip.h — C ABI of libgibbs_hip.so, the MI355X-native hot path of the
 * Gibbs motif sampler (drop-in for Etschbeijer/GibbsSampling, GibbsSampling.fs).
 *
 * The reference has no FFI; its "API" is the curried F# module functions.  Each
 * entry point below names the F# function it replaces (".fs" = GibbsSampling/
 * GibbsSampling.fs in the reference).  The P/Invoke shim that binds these from
 * .NET is in INTEGRATION.md.
 *
 * Conventions
 *  - C linkage, no exceptions cross the ABI; every call returns a gs_status.
 *  - Host buffers are caller-owned; device state lives inside the opaque gs_ctx.
 *  - One context drives ONE GPU (one process per GPU).  Several processes form one
 *    sampler through gs_comm_init (RCCL over xGMI); each then holds a contiguous
 *    shard of the sequences and all per-sequence arrays below are shard-local.
 *  - Sequences are ASCII symbol codes (BioItem.symbol, .fs:17) in [42, 90],
 *    already parsed by BioArray.ofNucleotideString / ofAminoAcidSymbolString
 *    (see gibbssampling_amd/bioarray.py for that parsing contract).
 *  - MotifIndex (.fs:712-716) with motifAmount = 1 is passed as
 *    (int32 position, double PWMS); position -1 encodes Positions = [].
 *  - A context is not thread-safe.
 */
#ifndef GIBBS_HIP_H
#define GIBBS_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_ctx gs_ctx;

typedef enum {
    GS_OK = 0,
    GS_E_ARG = 1,              /* .NET ArgumentOutOfRangeException / ArgumentException   */
    GS_E_ROULETTE_OVERRUN = 2, /* list index past the end in rouletteWheelSelection .fs:752 */
    GS_E_OVERFLOW = 3,         /* Checked int32 Array.sum overflow (.fs:117)              */
    GS_E_HIP = 4,              /* HIP runtime failure -> InvalidOperationException        */
    GS_E_RCCL = 5,             /* RCCL failure -> InvalidOperationException               */
    GS_E_STATE = 6,            /* call order violated (no sequences / no snapshot)        */
    GS_E_UNSUPPORTED = 7       /* shape outside what this build handles   */
} gs_status;

#define GS_UNIQUE_ID_BYTES 128

/* --- lifetime ---------------------------------------------------------- */
int gs_create(int32_t device_id, gs_ctx **out);
int gs_destroy(gs_ctx *ctx);
const char *gs_last_error(const gs_ctx *ctx);
/* Global index of the sequence that raised the last per-sequence error (-1 if none). */
int64_t gs_error_index(const gs_ctx *ctx);
const char *gs_version(void);

/* --- data -------------------------------------------------------------- */
/* Replaces the `sources` / `alphabet` arguments shared by every entry point.
 * codes: concatenated ASCII codes of this rank's n_local sequences, offsets[n_local+1].
 * n_global: sequences over all ranks (the N in N-1 of normalizePPM, .fs:964);
 * global_offset: global index of this rank's first sequence.  Single process:
 * n_global = n_local, global_offset = 0. */
int gs_set_sequences(gs_ctx *ctx, const uint8_t *codes, const int64_t *offsets, int32_t n_local,
                     const uint8_t *alphabet, int32_t alphabet_len, int64_t n_global,
                     int64_t global_offset);

/* --- multi-GPU (one process per GPU) ----------------------------------- */
int gs_comm_unique_id(uint8_t out[GS_UNIQUE_ID_BYTES]);
int gs_comm_init(gs_ctx *ctx, const uint8_t id[GS_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank);

/* In-kernel exchange of the per-sweep aggregate vector (round 6; no reference
 * counterpart: it replaces the all-reduce of .fs:940-942's shared snapshot between
 * ranks).  Every rank's context exports an exchange buffer (gs_exchange_handle: a
 * HIP IPC handle, GS_IPC_HANDLE_BYTES), the caller all-gathers the handles over any
 * transport and every rank opens them (gs_exchange_open, then a barrier of the
 * caller's before the next sweep).  From then on the packed-layout sweeps (live and
 * long kernels) end with their last workgroup writing the rank's partial into every
 * rank's buffer and summing every rank's: no all-reduce after the sweep (neither the
 * communicator's nor the caller's host-staged one below).  Positions set from outside
 * still need the caller's (or the communicator's) exchange of their aggregates; other
 * kernels keep theirs.  A peer that does not arrive within 0.5 s fails the sweep with
 * GS_E_RCCL.  gs_exchange_close returns to the all-reduce. */
#define GS_IPC_HANDLE_BYTES 64
int gs_exchange_handle(gs_ctx *ctx, uint8_t out[GS_IPC_HANDLE_BYTES]);
int gs_exchange_open(gs_ctx *ctx, const uint8_t *handles, int32_t nranks, int32_t rank);
int gs_exchange_close(gs_ctx *ctx);

/* Host-staged exchange of the per-sweep aggregates, for callers that combine
 * shards without RCCL (e.g. over their own transport, or several contexts on one
 * device): after gs_state_set_positions / each gs_run_sweeps(.., 1, ..) call,
 * download this rank's partial aggregates, sum them over the shards on the host
 * and upload the sum before the next sweep.  Size in int64 elements. */
int64_t gs_agg_size(const gs_ctx *ctx);
int gs_agg_download(gs_ctx *ctx, int64_t *out);
int gs_agg_upload(gs_ctx *ctx, const int64_t *in);

/* --- ★ the hot path ---------------------------------------------------- */
/* One synchronous sweep == MotifSampler.findBestMotifIndicesByWithStartPositions
 * (.fs:935-970) with motifAmount = 1: for every sequence, hold-one-out count
 * matrix / background rebuild from the snapshot pos_in, PWM, every W-mer window
 * scored, roulette-wheel pick with uniform u[n] (the n-th rnd.NextDouble(), .fs:968).
 * pos_in/u/pos_out/pwms_out are shard-local arrays of n_local entries. */
int gs_motif_sweep(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                   const int32_t *pos_in, const double *u, int32_t *pos_out, double *pwms_out);

/* Device-resident chain of sweeps (the Gibbs iteration).  gs_state_set_positions
 * uploads a snapshot; gs_run_sweeps enqueues n_sweeps sweeps asynchronously, the
 * uniform of sequence n in sweep t being gs_uniform(seed, stream_sweep(t), n);
 * gs_state_get synchronises and downloads the latest snapshot.  PWMS after a chain
 * are those of its last sweep: every sweep overwrites them and nothing can read them
 * in between, so the sweeps of one gs_run_sweeps call before its last compute
 * positions and aggregates only (a call with n_sweeps = 0 leaves the PWMS as they are). */
int gs_state_set_positions(gs_ctx *ctx, int32_t W, const int32_t *pos);
int gs_run_sweeps(gs_ctx *ctx, double pseudo_count, double cut_off, int32_t n_sweeps,
                  uint64_t seed, int64_t first_sweep);
int gs_state_get(gs_ctx *ctx, int32_t *pos_out, double *pwms_out);
/* The motif length of the resident snapshot (what sizes gs_occupancy_size for
 * gs_run_sweeps_stats), 0 when the context holds none. */
int32_t gs_state_motif_length(const gs_ctx *ctx);
/* With a communicator gs_run_sweeps replays chains of 6 sweeps as hipGraphs
 * (captured once per buffer phase and (pseudo_count, cut_off, seed)).  This builds the
 * graph for the current phase ahead of time (no sweep runs); optional. */
int gs_prepare_sweeps(gs_ctx *ctx, double pseudo_count, double cut_off, uint64_t seed);
int gs_synchronize(gs_ctx *ctx);
/* set + run + get in one call. */
int gs_motif_run(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off, int32_t n_sweeps,
                 uint64_t seed, int64_t first_sweep, int32_t *pos_inout, double *pwms_out);

/* --- greedy refinement ------------------------------ */
/* MotifSampler.findBestMotifIndicesWithStartPositions (.fs:885-929), motifAmount
 * = 1: Gauss–Seidel passes over the targets in order, each rebuilt from the live
 * positions, scored like the sweep, the head of the descending category sort kept
 * when its weight beats the target's current one (.fs:923); passes repeat until
 * one moves no position, at most max_passes (>= 1).  Needs every sequence on one
 * device (n_local == n_global), else GS_E_UNSUPPORTED.
 * gs_run_greedy refines the device-resident snapshot in place (after
 * gs_run_sweeps: the doMotifSampling pipeline, .fs:1034-1038) and synchronises;
 * kernel_ms_out (nullable) is the dispatch's own duration.
 * gs_motif_greedy uploads pos/pwms (the motifMem argument), refines, downloads. */
int gs_run_greedy(gs_ctx *ctx, double pseudo_count, double cut_off, int32_t max_passes,
                  int32_t *passes_out, double *kernel_ms_out);
int gs_motif_greedy(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                    int32_t max_passes, int32_t *pos_inout, double *pwms_inout,
                    int32_t *passes_out);
/* doMotifSampling (.fs:1034-1038), motifAmount = 1, device-resident: gs_random_starts
 * (init_mode) -> one sweep (uniforms of sweep 0 of `seed`) -> gs_run_greedy.
 * Single device (the greedy passes). */
int gs_motif_sampling(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                      uint64_t seed, int32_t init_mode, int32_t max_passes, int32_t *pos_out,
                      double *pwms_out, int32_t *passes_out);
/* R independent doMotifSampling runs (.fs:1034-1038, motifAmount = 1): chain r is exactly
 * gs_motif_sampling(ctx, W, pc, cut_off, seeds[r], init_mode, max_passes, ...).
 * pos_out / pwms_out: [n_chains][n_local] row-major; passes_out, status_out: [n_chains]
 * (both nullable).  Returns the status of the lowest-index failing chain (gs_error_index:
 * its sequence), GS_OK if none; the other chains' rows are still valid.
 * The chains' first stages run back to back on the context's stream, their greedy passes
 * as one launch of n_chains workgroups, with one synchronisation in all.  n_chains == 0
 * does nothing.  GS_E_UNSUPPORTED: sharded sequences or a communicator, a fixed PCV or
 * PPM, or chain slabs beyond 4 GiB.  The context holds no snapshot afterwards. */
int gs_motif_sampling_batch(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                            const uint64_t *seeds, int32_t n_chains, int32_t init_mode,
                            int32_t max_passes, int32_t *pos_out, double *pwms_out,
                            int32_t *passes_out, int32_t *status_out);
/* Device times of the last gs_motif_sampling_batch, ms: out[0] the chains' first stages
 * (starts, snapshot, sweep, copies), out[1] the batched greedy launch. */
int gs_batch_last_ms(const gs_ctx *ctx, double out[2]);

/* --- motifAmount >= 1 with Positions lists ---------- */
/* MotifIndex (.fs:712-716) with Positions lists: entry n is (cnt[n], pos[n*cap ..
 * n*cap + cnt[n])) in F# list order (the most recently consed position first, as
 * calculatePWMsForSegmentCombinations builds them, .fs:735) and pwms[n];
 * motif_amount <= cap <= 16.  The categories are those of
 * calculateNormalizedSegmentScores (.fs:759-784): every window's background
 * score, then combos(1) ++ ... ++ combos(motifAmount) (.fs:727-742: windows
 * pairwise more than W apart, every prefix product over the cut-off).
 * gs_motif_sweep_multi: findBestMotifIndicesByWithStartPositions (.fs:935-970),
 *   explicit uniforms; shards over ranks like gs_motif_sweep.
 * gs_motif_greedy_multi: findBestMotifIndicesWithStartPositions (.fs:885-929) in
 *   place (single device).
 * gs_motif_sampling_multi: doMotifSampling (.fs:1034-1038): gs_random_starts
 *   (init_mode) -> one sweep (uniforms of sweep 0 of `seed`) -> greedy passes.
 * Both also follow gs_set_fixed_pcv (the …ByPCV twins, .fs:788-853). */
int gs_motif_sweep_multi(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                         double cut_off, int32_t cap, const int32_t *cnt_in, const int32_t *pos_in,
                         const double *u, int32_t *cnt_out, int32_t *pos_out, double *pwms_out);
int gs_motif_greedy_multi(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                          double cut_off, int32_t max_passes, int32_t cap, int32_t *cnt_inout,
                          int32_t *pos_inout, double *pwms_inout, int32_t *passes_out);
int gs_motif_sampling_multi(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                            double cut_off, uint64_t seed, int32_t init_mode, int32_t max_passes,
                            int32_t cap, int32_t *cnt_out, int32_t *pos_out, double *pwms_out,
                            int32_t *passes_out);
/* R independent doMotifSampling runs (.fs:1034-1038) with Positions lists: chain r is exactly
 * gs_motif_sampling_multi(ctx, motif_amount, W, pc, cut_off, seeds[r], init_mode, max_passes,
 * cap, ...).  Returns the status of the lowest-index failing chain (gs_error_index: its
 * sequence), GS_OK if none; the other chains' rows are still valid, list entries past cnt
 * unspecified.  A chain with more than 2^28 categories gets GS_E_UNSUPPORTED in its own
 * status_out entry and the other chains finish.  The chains' starts run back to back on the
 * context's stream, sweep 0 over all (chain, target) pairs at once, the greedy passes as
 * speculative steps of two launches for all chains; the host waits once per arena round and
 * once per 32 steps.  n_chains == 0 does nothing.  GS_E_ARG before any launch: motif_amount
 * or cap outside 1 .. 16, cap < motif_amount, max_passes < 1, a bad W or init_mode, a null
 * output.  GS_E_UNSUPPORTED: sharded sequences or a communicator, a fixed PCV or PPM, chain
 * slabs (arenas included) beyond 4 GiB, sequences too long for the list path's LDS carve.
 * The context holds no snapshot afterwards and its error words are clear. */
int gs_motif_sampling_multi_batch(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                                  double cut_off, const uint64_t *seeds, int32_t n_chains,
                                  int32_t init_mode, int32_t max_passes, int32_t cap,
                                  int32_t *cnt_out,    /* [n_chains][n_local]      */
                                  int32_t *pos_out,    /* [n_chains][n_local][cap] */
                                  double *pwms_out,    /* [n_chains][n_local]      */
                                  int32_t *passes_out, /* [n_chains], nullable     */
                                  int32_t *status_out  /* [n_chains], nullable     */);
/* Device times of the last gs_motif_sampling_multi_batch, ms: starts, sweep, greedy passes. */
int gs_multi_batch_last_ms(const gs_ctx *ctx, double out[3]);
/* Its rounds: out[0] sweep rounds after the first (arena growth), out[1] greedy restart
 * rounds, out[2] chains restarted in all, out[3] speculative slots per chain of the first
 * greedy round. */
int gs_multi_batch_last_info(const gs_ctx *ctx, int32_t out[4]);

/* R independent chains of n_sweeps synchronous sweeps each (motifAmount = 1) in one call:
 * chain r is exactly gs_motif_run(ctx, W, pc, cut_off, n_sweeps, seeds[r], first_sweep,
 * row r, ...) from its start.  init_mode -1: chain r starts from the caller's row
 * pos_inout[r] (-1 = Positions []); 0 / 1: from the positions of gs_random_starts(ctx, W, pc,
 * seeds[r], init_mode, ...), pos_inout is output only and sweep 0 is the sweep of
 * doMotifSampling.  The uniform of sequence n in sweep t is gs_uniform(seeds[r],
 * gs_stream_sweep(first_sweep + t), global n), or u[r][t][n] with u non-null (as
 * gs_motif_sweep); a second call with init_mode -1 and first_sweep + n_sweeps continues the
 * chains.  One sweep of all chains is one launch over the (chain, target) pairs, the launches
 * back to back with one synchronisation at the end.  PWMS are those of the last sweep;
 * n_sweeps == 0 leaves the positions as they are (init_mode 0 / 1: the starts) and does not
 * write pwms_out; n_chains == 0 does nothing.  Returns the status of the lowest-index failing
 * chain (gs_error_index: its sequence), GS_OK if none: a chain that raises (.fs:752, .fs:117)
 * keeps its status in status_out[r], its later sweeps are skipped and its rows unspecified;
 * the other chains finish.  GS_E_ARG before any launch: a bad W or init_mode, n_sweeps < 0,
 * first_sweep < 0, a null seeds or output, a start outside [-1, L - W] (init_mode -1).
 * GS_E_UNSUPPORTED: sharded sequences or a communicator, a fixed PCV or PPM, chain slabs
 * beyond 4 GiB, sequences too long for the list path's LDS carve.  The context holds no
 * snapshot afterwards and its error words are clear. */
int gs_motif_run_batch(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                       int32_t n_sweeps, const uint64_t *seeds, int32_t n_chains,
                       int64_t first_sweep, int32_t init_mode,
                       const double *u,      /* nullable: [n_chains][n_sweeps][n_local] */
                       int32_t *pos_inout,   /* [n_chains][n_local], -1 = Positions []   */
                       double *pwms_out,     /* [n_chains][n_local]                      */
                       int32_t *status_out   /* [n_chains], nullable                     */);
/* Device times of the last gs_motif_run_batch or gs_motif_run_batch_stats, ms: starts (and
 * first aggregates), sweeps (the statistics launches included). */
int gs_run_batch_last_ms(const gs_ctx *ctx, double out[2]);

/* Bins of one chain's occupancy histogram for motif length W: sequence n owns
 * off[n] .. off[n+1]-1 with off[0] = 0, off[n+1] = off[n] + 1 + (L_n - W + 1);
 * bin off[n] counts Positions [], bin off[n] + 1 + k counts start k. */
int64_t gs_occupancy_size(const gs_ctx *ctx, int32_t W);              /* H, -1 on a bad W / no sequences */
int gs_occupancy_offsets(const gs_ctx *ctx, int32_t W, int64_t *off); /* [n_local + 1] */

/* gs_motif_run_batch with statistics of the chains' sweeps, gathered on the device with no
 * host wait (no reference counterpart; the .fsx tallies whole runs on the host, .fsx:384-388).
 * The chains, pos_inout, pwms_out, status_out, the return value, n_chains == 0, n_sweeps == 0
 * and every refusal are exactly those of gs_motif_run_batch with the same leading arguments;
 * with all three statistics null the call is that call, bit for bit.  Sweep t, 0 <= t <
 * n_sweeps, is counted when t >= burn_in and (t - burn_in) % thin == 0; n_counted is their
 * number; the state of a counted sweep is the snapshot that sweep wrote (the starts are never
 * counted).  occ_out[r][b]: the number of counted sweeps whose state has its sequence at bin b
 * (gs_occupancy_offsets); for a chain that finishes every sequence's bins sum to n_counted.
 * ic_out[r][i]: the sum over the sequences of the PWMS of the i-th counted sweep (the
 * reference's quality of a run, .fs:981-989), in binary64 in one fixed order: 64 partial sums
 * v[l], each from +0.0, v[l] adding the PWMS of n = l, l + 64, ... in increasing n; then for
 * s = 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l + s] for l < s; the result is v[0].  best_*: the
 * counted sweep with the largest ic, a later one replacing it only when strictly larger
 * (.fs:989); the first counted sweep is always taken and a NaN never replaces anything.
 * best_sweep_out[r] is the absolute sweep number first_sweep + t, or -1 when no counted sweep
 * completed (the two rows are then unspecified); the rows are that sweep's positions and PWMS,
 * bit for bit.  A chain that raises in sweep t contributes nothing from sweep t on: its bins
 * hold the counted sweeps before t, its ic entries from t on are quiet NaN, its best is the
 * best before t; the other chains are untouched.  The outputs are written, not accumulated: a
 * continued call (init_mode -1, first_sweep advanced) yields its own counts and the caller
 * adds them.  GS_E_ARG before any launch, besides gs_motif_run_batch's: burn_in outside [0,
 * n_sweeps], thin < 1, best_sweep_out without both best rows or the reverse.  The bins (n_chains
 * x H x 4 bytes), the trace and the best rows count toward the 4 GiB of chain slabs. */
int gs_motif_run_batch_stats(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
        int32_t n_sweeps, const uint64_t *seeds, int32_t n_chains, int64_t first_sweep,
        int32_t init_mode, const double *u,
        int32_t burn_in, int32_t thin,
        int32_t *pos_inout, double *pwms_out, int32_t *status_out,
        int32_t *occ_out,        /* [n_chains][H], nullable            */
        double  *ic_out,         /* [n_chains][n_counted], nullable    */
        int64_t *best_sweep_out, /* [n_chains], nullable               */
        int32_t *best_pos_out,   /* [n_chains][n_local]                */
        double  *best_pwms_out   /* [n_chains][n_local]                */);

/* gs_run_sweeps with the same statistics of the single chain's sweeps, gathered on the device
 * behind each counted sweep of whichever sweep kernel runs it (the general and four-symbol
 * kernels, the DNA, live-chain, long-sequence and all-background ones), with no host wait
 * between sweeps: the way to a posterior at the sizes where the chain batch no longer pays.
 * The chain is exactly the one gs_run_sweeps(ctx, pc, cut_off, n_sweeps, seed, first_sweep)
 * runs from the same snapshot, or, with u non-null, the one whose sweep t uses u[t][n] as
 * gs_motif_sweep would.  The snapshot stays on the context: gs_state_get, a further
 * gs_run_sweeps (first_sweep advanced) and gs_run_greedy work afterwards.  With every
 * statistic null and u null the positions and PWMS left are those of gs_run_sweeps followed
 * by gs_synchronize, bit for bit.  The call synchronises once, at its end; its sweeps are
 * always direct launches (never the captured graphs), an uncounted sweep costs nothing extra.
 * Sweep t, 0 <= t < n_sweeps, is counted when t >= burn_in and (t - burn_in) % thin == 0;
 * n_counted is their number; the state of a counted sweep is the snapshot that sweep wrote
 * (the starts are never counted).  The outputs are written, not accumulated: a continued call
 * yields its own counts and the caller adds them.
 * occ_out[b]: the number of counted sweeps whose state has its sequence at bin b, in the bins
 * of gs_occupancy_offsets (Positions [] goes to bin off[n], start k to bin off[n] + 1 + k); for
 * a chain that finishes every sequence's bins sum to n_counted.
 * ic_out[i]: the sum over the sequences of the PWMS of the i-th counted sweep (.fs:981-989), in
 * binary64 in the fixed order of gs_motif_run_batch_stats: 64 partial sums v[l], each from
 * +0.0, v[l] adding the PWMS of n = l, l + 64, ... in increasing n; then for s = 32, 16, 8, 4,
 * 2, 1: v[l] = v[l] + v[l + s] for l < s; the result is v[0].
 * best_*: the first counted sweep with the largest ic: a later one replaces it only when
 * strictly larger (.fs:989), the first counted sweep is always taken and a NaN never replaces
 * anything.  best_sweep_out[0] is the absolute sweep number first_sweep + t, or -1 when no
 * counted sweep completed (the two rows are then unspecified); the rows are that sweep's
 * positions and PWMS, bit for bit.
 * When the sticky device error is raised in sweep t (.fs:752, .fs:117) nothing is counted from
 * t on: the bins hold the counted sweeps before t, the ic entries from t on are quiet NaN, the
 * best is the best before t; the call returns that status (the statistics are still written)
 * and leaves the context as gs_run_sweeps followed by gs_synchronize leaves it after the same
 * error (no snapshot).
 * Refused before any launch: GS_E_STATE without a snapshot; GS_E_ARG for n_sweeps < 0,
 * first_sweep < 0, burn_in outside [0, n_sweeps], thin < 1, best_sweep_out without both best
 * rows or the reverse; GS_E_UNSUPPORTED for sharded sequences or a communicator (the trace
 * needs every sequence), or when the bins (H x 4 bytes), the trace, the best rows and the
 * explicit uniforms together pass 4 GiB.  A fixed PCV is allowed (gs_set_fixed_pcv: the ByPCV
 * twin): the statistics only read the sweeps' outputs.
 * gs_motif_run_stats: gs_state_set_positions + gs_run_sweeps_stats + gs_state_get in one call
 * (gs_motif_run with the statistics); its refusals come before the snapshot is replaced. */
int gs_run_sweeps_stats(gs_ctx *ctx, double pseudo_count, double cut_off, int32_t n_sweeps,
        uint64_t seed, int64_t first_sweep,
        const double *u,         /* nullable: [n_sweeps][n_local], as gs_motif_sweep's */
        int32_t burn_in, int32_t thin,
        int32_t *occ_out,        /* [H] of gs_occupancy_offsets, nullable              */
        double  *ic_out,         /* [n_counted], nullable                              */
        int64_t *best_sweep_out, /* [1], nullable; goes together with both best rows   */
        int32_t *best_pos_out,   /* [n_local]                                          */
        double  *best_pwms_out   /* [n_local]                                          */);
int gs_motif_run_stats(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
        int32_t n_sweeps, uint64_t seed, int64_t first_sweep, const double *u,
        int32_t burn_in, int32_t thin,
        int32_t *pos_inout,      /* [n_local], -1 = Positions []                       */
        double  *pwms_out,       /* [n_local]                                          */
        int32_t *occ_out, double *ic_out, int64_t *best_sweep_out, int32_t *best_pos_out,
        double *best_pwms_out);
/* Device times of the last gs_run_sweeps_stats, ms: out[0] the chain of launches from the
 * first sweep to the last statistics launch; with the profile on (gs_profile_enable) out[1]
 * is the sum over the statistics launches, each between two events of its own, and out[0] the
 * rest; without it out[1] is 0. */
int gs_run_stats_last_ms(const gs_ctx *ctx, double out[2]);

/* Chain summaries: the reduction of occupancy histograms on the device to what a caller keeps
 * of them (motifAmount 1, the bins of gs_occupancy_offsets(ctx, W, off); A = the alphabet's
 * length).  Per chain r and sequence n the mode: b* is the smallest bin index within the
 * sequence's row whose count is the row's maximum (the first maximum, the .fsx's
 * countBy |> sortByDescending |> head, .fsx:384-388); mode_pos_out[r][n] = b* - 1 (-1 means
 * Positions []), mode_count_out[r][n] that count; a row of zeros gives (-1, 0).  Per chain the
 * mean count matrix times the counted states, counts_out[r][A*W + A] in gs_counts' layout, C
 * then T: C[a*W + j] = sum over n, k of occ[r][off[n]+1+k] where sequence n has alphabet[a] at
 * k + j; T[a] = sum over n, k of occ[r][off[n]+1+k] times the number of alphabet[a] in sequence
 * n outside [k, k+W).  For bins that a chain filled this is exactly the sum of gs_counts over
 * the counted states; a symbol outside the alphabet counts wherever gs_counts counts it, and
 * nowhere else.  Pooled: chain r is pooled when the bins of local sequence 0 sum to n_counted
 * (a chain that raised stopped counting); n_pooled_out[0] is their number,
 * pool_mode_pos_out[n] / pool_mode_count_out[n] the first maximum of the pooled chains' bins
 * summed in int64, pool_counts_out the sum of the pooled chains' cells; with no pooled chain
 * (-1, 0) everywhere and zero cells.  Integer sums only: the results are the same on every run.
 * Each output group is nullable as a whole: the mode pair, the counts, the pooled four.
 * gs_occupancy_summary reduces caller-held bins (sums of several calls, of several processes'
 * chains): it uploads occ, reduces and downloads.  It needs sequences (else GS_E_STATE) but no
 * snapshot, and leaves the context's snapshot untouched.  GS_E_ARG: a bad W, occ null with
 * n_chains > 0, n_chains < 0, n_counted < 0, half of a group given.  n_chains == 0 does
 * nothing.  GS_E_UNSUPPORTED: sharded sequences or a communicator, or bins and results beyond
 * 4 GiB.  Negative bins are the caller's error: the result is unspecified, without a fault. */
int gs_occupancy_summary(gs_ctx *ctx, int32_t W,
        const int32_t *occ,            /* [n_chains][H]                        */
        int32_t n_chains, int64_t n_counted,
        int32_t *mode_pos_out,         /* [n_chains][n_local], nullable        */
        int32_t *mode_count_out,       /* [n_chains][n_local], with the above  */
        int64_t *counts_out,           /* [n_chains][A*W + A], nullable        */
        int32_t *pool_mode_pos_out,    /* [n_local], nullable with the next 3  */
        int64_t *pool_mode_count_out,  /* [n_local]                            */
        int64_t *pool_counts_out,      /* [A*W + A]                            */
        int32_t *n_pooled_out          /* [1]                                  */);
/* gs_run_sweeps_stats / gs_motif_run_stats with the single chain's summary appended
 * (mode_pos_out[n_local], mode_count_out[n_local], counts_out[A*W + A], nullable as above).
 * The bins stay on the device whenever occ_out or a summary output is asked for and are
 * downloaded only when occ_out is non-null; the reduction is one launch behind the last
 * statistics launch, before the call's single synchronisation.  Everything else is the stats
 * call's contract: the chain, the other statistics, the refusals (half of a summary group:
 * GS_E_ARG), the state left on the context, the error rule: after a raise in sweep t the
 * summary is that of the bins as they stand and the status is returned.  With the three
 * summary outputs null the call is the stats call, bit for bit. */
int gs_run_sweeps_summary(gs_ctx *ctx, double pseudo_count, double cut_off, int32_t n_sweeps,
        uint64_t seed, int64_t first_sweep, const double *u, int32_t burn_in, int32_t thin,
        int32_t *occ_out, double *ic_out, int64_t *best_sweep_out, int32_t *best_pos_out,
        double *best_pwms_out,
        int32_t *mode_pos_out, int32_t *mode_count_out, int64_t *counts_out);
int gs_motif_run_summary(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
        int32_t n_sweeps, uint64_t seed, int64_t first_sweep, const double *u,
        int32_t burn_in, int32_t thin, int32_t *pos_inout, double *pwms_out,
        int32_t *occ_out, double *ic_out, int64_t *best_sweep_out, int32_t *best_pos_out,
        double *best_pwms_out,
        int32_t *mode_pos_out, int32_t *mode_count_out, int64_t *counts_out);
/* gs_motif_run_batch_stats with the per-chain and the pooled outputs of gs_occupancy_summary
 * appended; n_counted is the call's own, so a chain that raised is left out of the pool.  The
 * extra slabs count toward the 4 GiB of chain slabs. */
int gs_motif_run_batch_summary(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
        int32_t n_sweeps, const uint64_t *seeds, int32_t n_chains, int64_t first_sweep,
        int32_t init_mode, const double *u, int32_t burn_in, int32_t thin,
        int32_t *pos_inout, double *pwms_out, int32_t *status_out,
        int32_t *occ_out, double *ic_out, int64_t *best_sweep_out, int32_t *best_pos_out,
        double *best_pwms_out,
        int32_t *mode_pos_out, int32_t *mode_count_out, int64_t *counts_out,
        int32_t *pool_mode_pos_out, int64_t *pool_mode_count_out, int64_t *pool_counts_out,
        int32_t *n_pooled_out);
/* Device time of the last summary's reduction (any of the four calls above), ms, between two
 * events around its launches; 0 when nothing was reduced. */
int gs_summary_last_ms(const gs_ctx *ctx, double out[1]);

/* Chain agreement: whether pooling the chains was justified, computed on the device from the
 * same bins (motifAmount 1, occ[n_chains][H] in the bins of gs_occupancy_offsets(ctx, W, off)).
 * With a pooled flag f[r] a chain, P the number of pooled chains and pool[b] the sum of
 * occ[r][b] over the pooled chains in int64, for a pooled chain r and a sequence n:
 * D(r, n) = the sum over the bins b of row n of |P occ[r][b] - pool[b]| in int64; every row of
 * a finished chain sums to n_counted, so D / (2 P n_counted) is the total variation distance
 * between chain r's marginal of sequence n and the pooled marginal.  m(r, n) is the chain's
 * first-maximum bin of row n and m*(n) that of pool, exactly as the summaries take them.
 * Per sequence: agree_out[n] the number of pooled r with m(r, n) == m*(n); spread_out[n] the
 * largest D(r, n) over the pooled r; spread_chain_out[n] the lowest r that has it; with P == 0
 * the row is (0, 0, -1).  Per chain: chain_dist_out[r] the sum over n of D(r, n),
 * chain_agree_out[r] the number of n with m(r, n) == m*(n); a chain that is not pooled gets
 * (-1, -1).  n_pooled_out[0] = P.  The six outputs form one group, nullable as a whole; half
 * of it given is GS_E_ARG.  Integer sums only: the results are the same on every run.
 * Chain r is pooled when the bins of local sequence 0 sum to n_counted (the summaries' rule),
 * or, in gs_occupancy_agreement with pooled non-null, when pooled[r] is non-zero: the mask
 * serves chains of Positions lists, whose rows do not sum to n_counted (pass which chains
 * finished), and a split-half check of one chain (two continued gs_run_sweeps_stats calls
 * uploaded as two chains).
 * Exact while n_chains times the largest bin stays below 2^62, which bins the library wrote
 * always do.  Negative bins are the caller's error: the result is unspecified, without a fault;
 * nothing is indexed by a bin's value.  Without sequences n_pooled = n_chains (or the mask's
 * count) and every pooled chain reads (0, 0).
 * gs_occupancy_agreement reduces caller-held bins: it uploads, reduces and downloads, exactly
 * as gs_occupancy_summary does.  It needs sequences (else GS_E_STATE) but no snapshot, and
 * leaves the snapshot untouched.  GS_E_ARG: a bad W, occ null with n_chains > 0, n_chains < 0,
 * n_counted < 0, half of the group given.  n_chains == 0 does nothing.  GS_E_UNSUPPORTED:
 * sharded sequences or a communicator, or bins and results beyond 4 GiB.
 * There is no agreement variant of the single-chain or of the list run calls: one chain has
 * nothing to compare with, and list chains go through gs_occupancy_agreement with the mask. */
int gs_occupancy_agreement(gs_ctx *ctx, int32_t W,
        const int32_t *occ,            /* [n_chains][H]                        */
        int32_t n_chains, int64_t n_counted,
        const int32_t *pooled,         /* [n_chains], nullable: the rule       */
        int32_t *agree_out,            /* [n_local], nullable with the next 5  */
        int64_t *spread_out,           /* [n_local]                            */
        int32_t *spread_chain_out,     /* [n_local]                            */
        int32_t *chain_agree_out,      /* [n_chains]                           */
        int64_t *chain_dist_out,       /* [n_chains]                           */
        int32_t *n_pooled_out          /* [1]                                  */);
/* gs_motif_run_batch_summary with the agreement group appended (its pool count as
 * agree_n_pooled_out); the reduction is enqueued behind the summary's launches, before the
 * call's single synchronisation, and the bins come down only when occ_out is non-null.
 * n_counted and the pooled rule are the call's own, so a chain that raised is left out and
 * reads (-1, -1); with the summary's pooled outputs asked for the pool is decided once, for
 * both.  With the six agreement outputs null the call is gs_motif_run_batch_summary, bit for
 * bit.  The extra slabs count toward the 4 GiB of chain slabs. */
int gs_motif_run_batch_agreement(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
        int32_t n_sweeps, const uint64_t *seeds, int32_t n_chains, int64_t first_sweep,
        int32_t init_mode, const double *u, int32_t burn_in, int32_t thin,
        int32_t *pos_inout, double *pwms_out, int32_t *status_out,
        int32_t *occ_out, double *ic_out, int64_t *best_sweep_out, int32_t *best_pos_out,
        double *best_pwms_out,
        int32_t *mode_pos_out, int32_t *mode_count_out, int64_t *counts_out,
        int32_t *pool_mode_pos_out, int64_t *pool_mode_count_out, int64_t *pool_counts_out,
        int32_t *n_pooled_out,
        int32_t *agree_out, int64_t *spread_out, int32_t *spread_chain_out,
        int32_t *chain_agree_out, int64_t *chain_dist_out, int32_t *agree_n_pooled_out);
/* Device time of the last agreement's reduction (either call above), ms, between two events
 * around its launches; 0 when nothing was reduced. */
int gs_agreement_last_ms(const gs_ctx *ctx, double out[1]);

/* R independent chains of n_sweeps synchronous sweeps each with Positions lists (any
 * motifAmount) in one call: chain r is exactly n_sweeps calls of gs_motif_sweep_multi(ctx,
 * motif_amount, W, pc, cut_off, cap, ...), each fed the previous output.  init_mode -1:
 * chain r starts from the caller's lists (cnt_inout[r], pos_inout[r]; lists longer than
 * motif_amount are allowed up to cap); 0 / 1: from the positions of gs_random_starts(ctx, W,
 * pc, seeds[r], init_mode, ...) as one-position lists, the lists are output only.  The
 * uniform of sequence n in sweep t is gs_uniform(seeds[r], gs_stream_sweep(first_sweep + t),
 * global n), or u[r][t][n] with u non-null; a second call with init_mode -1 and first_sweep
 * + n_sweeps continues the chains.  One sweep of all chains is one launch over the (chain,
 * target) pairs (motif_amount >= 3: and a second, small one that rescores the pairs whose
 * combinations overflowed the first arena, taken from a device list), the launches back
 * to back with one synchronisation at the end; only a chain with a target beyond the second
 * arena (16 x max(2048, 4 (L - W + 1)) combinations of up to motif_amount - 1 windows) is
 * run again afterwards from the sweep it stopped in, with larger arenas.  PWMS are those of
 * the last sweep, list entries past cnt are -1; n_sweeps == 0 leaves the lists as they are
 * (init_mode 0 / 1: the starts) and does not write pwms_out; n_chains == 0 does nothing.
 * Returns the status of the lowest-index failing chain (gs_error_index: its sequence), GS_OK
 * if none: a chain that raises (.fs:752, .fs:117) keeps its status in status_out[r], its
 * later sweeps are skipped and its rows unspecified; the other chains finish.  A chain with
 * more than 2^28 combinations in a target gets GS_E_UNSUPPORTED in its own status_out entry.
 * GS_E_ARG before any launch: motif_amount or cap outside 1 .. 16, cap < motif_amount, a bad
 * W or init_mode, n_sweeps < 0, first_sweep < 0, a null seeds or output, a cnt outside
 * [0, cap] or a position outside its sequence (init_mode -1).  GS_E_UNSUPPORTED: sharded
 * sequences or a communicator, a fixed PCV or PPM, chain slabs beyond 4 GiB, sequences too
 * long for the list path's LDS carve.  The context holds no snapshot afterwards and its
 * error words are clear. */
int gs_motif_run_multi_batch(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                             double cut_off, int32_t n_sweeps, const uint64_t *seeds,
                             int32_t n_chains, int64_t first_sweep, int32_t init_mode, int32_t cap,
                             const double *u,      /* nullable: [n_chains][n_sweeps][n_local] */
                             int32_t *cnt_inout,   /* [n_chains][n_local]                      */
                             int32_t *pos_inout,   /* [n_chains][n_local][cap], F# list order  */
                             double *pwms_out,     /* [n_chains][n_local]                      */
                             int32_t *status_out   /* [n_chains], nullable                     */);
/* The same for one chain from the caller's lists (init_mode -1). */
int gs_motif_run_multi(gs_ctx *ctx, int32_t motif_amount, int32_t W, double pseudo_count,
                       double cut_off, int32_t n_sweeps, uint64_t seed, int64_t first_sweep,
                       int32_t cap, int32_t *cnt_inout, int32_t *pos_inout, double *pwms_out);
/* gs_motif_run_multi_batch with statistics of the chains' sweeps, gathered on the device with
 * no host wait between sweeps: gs_motif_run_batch_stats for Positions lists.  The chains, the
 * lists, pwms_out, status_out, the return value, n_chains == 0, n_sweeps == 0 and every
 * refusal are exactly those of gs_motif_run_multi_batch with the same leading arguments; with
 * all four statistics null the call is that call, bit for bit.  Counting is
 * gs_motif_run_batch_stats': sweep t counts when t >= burn_in and (t - burn_in) % thin == 0,
 * the state of a counted sweep is the list snapshot that sweep wrote, the starts never count,
 * and the outputs are written, not accumulated.
 * occ_out[r][b], bins of gs_occupancy_offsets: bin off[n] counts the counted sweeps whose list
 * of sequence n is empty, bin off[n] + 1 + k those whose list contains start k (a sweep's list
 * holds pairwise distinct starts, .fs:727-742; a start outside [0, L - W] is not counted).
 * sites_out[r][n][c], 0 <= c <= motif_amount: the counted sweeps whose list of sequence n has
 * length c (a sweep never writes a longer list; a length outside that range is not counted).
 * For a chain that finishes, with occ = occ_out[r] and s = sites_out[r][n]:
 *   (1) s[0] + s[1] + ... + s[motif_amount] == n_counted;
 *   (2) s[0] == occ[off[n]];
 *   (3) 1 s[1] + 2 s[2] + ... + motif_amount s[motif_amount]
 *         == occ[off[n] + 1] + ... + occ[off[n + 1] - 1].
 * ic_out[r][i]: the sum over the sequences of the PWMS of the i-th counted sweep, in the fixed
 * 64-lane order of gs_motif_run_batch_stats (the same contract).  best_*: the first counted
 * sweep with the largest sum (a later one replaces it only when strictly larger, .fs:989; the
 * first counted sweep is always taken; a NaN never wins).  best_sweep_out[r] is the absolute
 * sweep number first_sweep + t, or -1 when no counted sweep completed (the three rows are then
 * unspecified); the rows are that sweep's lists and PWMS, bit for bit.  A chain that raises in
 * sweep t contributes nothing from t on: its bins and site counts hold the counted sweeps
 * before t, its ic entries from t on are quiet NaN, its best is the best before t; the other
 * chains are untouched.  A chain that is run again with larger arenas from the sweep it
 * stopped in contributes every counted sweep exactly once; one given up there
 * (GS_E_UNSUPPORTED in its status) keeps the statistics of the sweeps before that one.
 * GS_E_ARG before any launch, besides gs_motif_run_multi_batch's: burn_in outside [0,
 * n_sweeps], thin < 1, best_sweep_out without all three best rows or the reverse.  The bins,
 * the site counts, the trace and the best rows count toward the 4 GiB of chain slabs. */
int gs_motif_run_multi_batch_stats(gs_ctx *ctx, int32_t motif_amount, int32_t W,
        double pseudo_count, double cut_off, int32_t n_sweeps, const uint64_t *seeds,
        int32_t n_chains, int64_t first_sweep, int32_t init_mode, int32_t cap, const double *u,
        int32_t burn_in, int32_t thin,
        int32_t *cnt_inout, int32_t *pos_inout, double *pwms_out, int32_t *status_out,
        int32_t *occ_out,        /* [n_chains][H], nullable                          */
        int32_t *sites_out,      /* [n_chains][n_local][motif_amount + 1], nullable  */
        double  *ic_out,         /* [n_chains][n_counted], nullable                  */
        int64_t *best_sweep_out, /* [n_chains], nullable                             */
        int32_t *best_cnt_out,   /* [n_chains][n_local]                              */
        int32_t *best_pos_out,   /* [n_chains][n_local][cap], F# list order, -1 past cnt */
        double  *best_pwms_out   /* [n_chains][n_local]                              */);
/* Chain summaries for Positions-list chains: the reduction, on the device, of
 * list bins occ[r] (gs_occupancy_offsets) and site counts sites[r][n][0 .. motif_amount] (as
 * gs_motif_run_multi_batch_stats writes them) to what a caller keeps; M = motif_amount.  For a
 * view (chain r's own bins and site counts, or the pooled ones) and a sequence n:
 *   (1) c* is the smallest c in 0 .. M whose site count is the row's largest:
 *       mode_sites = c*, mode_sites_count that count (an all-zero row: 0, 0);
 *   (2) c* rounds, each taking among the starts k in [0, L_n - W] not yet excluded the one
 *       with the largest bin occ[off[n] + 1 + k], the smallest k among equals; a start is
 *       excluded when |k - q| <= W for a start q already taken (ceckForDistance, .fs:129-140:
 *       the starts kept are pairwise more than W apart); a zero bin is a candidate like any
 *       other; the rounds end early when every start is excluded;
 *   (3) mode_cnt is the number taken, mode_pos[0 .. M) the starts in ascending order (-1 past
 *       mode_cnt) and mode_count[i] the bin of mode_pos[i] (0 past mode_cnt).
 * counts_out[r] and pool_counts_out are gs_occupancy_summary's cells on the same bins: for
 * bins a chain filled, the sum over its counted states of the list aggregates (C over every
 * listed segment, T[a] the sum over list entries of the sequence's alphabet[a] outside that
 * entry's segment).  Pooled: chain r is pooled when every sequence's site counts sum to
 * n_counted; n_pooled_out[0] is their number, the pooled view's bins and site counts are the
 * pooled chains' summed in int64; with no pooled chain every row is (0, 0) with an empty list
 * and the cells are zero.  Integer sums only: the results are the same on every run.  Each
 * output group is nullable as a whole: the five per-chain mode arrays, the counts, the seven
 * pooled outputs.
 * gs_list_occupancy_summary reduces caller-held slabs: it uploads, reduces and downloads.  It
 * needs sequences (else GS_E_STATE) but no snapshot, and leaves the context's snapshot
 * untouched.  GS_E_ARG: a bad W, motif_amount outside 1 .. 16, occ or sites null with
 * n_chains > 0, n_chains < 0, n_counted < 0, half of a group given.  n_chains == 0 does
 * nothing.  GS_E_UNSUPPORTED: sharded sequences or a communicator, or slabs and results
 * beyond 4 GiB.  Negative bins or site counts are the caller's error: the result is
 * unspecified, without a fault. */
int gs_list_occupancy_summary(gs_ctx *ctx, int32_t W, int32_t motif_amount,
        const int32_t *occ,                /* [n_chains][H]                              */
        const int32_t *sites,              /* [n_chains][n_local][motif_amount + 1]      */
        int32_t n_chains, int64_t n_counted,
        int32_t *mode_sites_out,           /* [n_chains][n_local], nullable with the next 4 */
        int32_t *mode_sites_count_out,     /* [n_chains][n_local]                        */
        int32_t *mode_cnt_out,             /* [n_chains][n_local]                        */
        int32_t *mode_pos_out,             /* [n_chains][n_local][motif_amount]          */
        int32_t *mode_count_out,           /* [n_chains][n_local][motif_amount]          */
        int64_t *counts_out,               /* [n_chains][A*W + A], nullable              */
        int32_t *pool_mode_sites_out,      /* [n_local], nullable with the next 6        */
        int64_t *pool_mode_sites_count_out,/* [n_local]                                  */
        int32_t *pool_mode_cnt_out,        /* [n_local]                                  */
        int32_t *pool_mode_pos_out,        /* [n_local][motif_amount]                    */
        int64_t *pool_mode_count_out,      /* [n_local][motif_amount]                    */
        int64_t *pool_counts_out,          /* [A*W + A]                                  */
        int32_t *n_pooled_out              /* [1]                                        */);
/* gs_motif_run_multi_batch_stats with the outputs of gs_list_occupancy_summary appended;
 * n_counted is the call's own.  The bins and site counts are kept on the device whenever the
 * caller asks for them or for any summary output, and are downloaded only when occ_out /
 * sites_out are non-null; the reduction follows the last statistics launch of the last round
 * (the resume rounds of chains run again with larger arenas included), before the final
 * download.  Everything else is the stats call's contract: the chains, the refusals (half of
 * a summary group: GS_E_ARG), the context left without a snapshot, and the rule for a chain
 * that raises: it is summarised from its bins as they stand and left out of the pool, the
 * other chains are untouched.  With every summary output null the call is the stats call, bit
 * for bit.  The extra slabs count toward the 4 GiB of chain slabs.  gs_summary_last_ms reports
 * this reduction's device time too. */
int gs_motif_run_multi_batch_summary(gs_ctx *ctx, int32_t motif_amount, int32_t W,
        double pseudo_count, double cut_off, int32_t n_sweeps, const uint64_t *seeds,
        int32_t n_chains, int64_t first_sweep, int32_t init_mode, int32_t cap, const double *u,
        int32_t burn_in, int32_t thin,
        int32_t *cnt_inout, int32_t *pos_inout, double *pwms_out, int32_t *status_out,
        int32_t *occ_out, int32_t *sites_out, double *ic_out, int64_t *best_sweep_out,
        int32_t *best_cnt_out, int32_t *best_pos_out, double *best_pwms_out,
        int32_t *mode_sites_out, int32_t *mode_sites_count_out, int32_t *mode_cnt_out,
        int32_t *mode_pos_out, int32_t *mode_count_out, int64_t *counts_out,
        int32_t *pool_mode_sites_out, int64_t *pool_mode_sites_count_out,
        int32_t *pool_mode_cnt_out, int32_t *pool_mode_pos_out, int64_t *pool_mode_count_out,
        int64_t *pool_counts_out, int32_t *n_pooled_out);
/* Device times of the last gs_motif_run_multi_batch or gs_motif_run_multi_batch_stats, ms:
 * starts (and first aggregates), sweeps (resumed chains and the statistics launches
 * included). */
int gs_run_multi_batch_last_ms(const gs_ctx *ctx, double out[2]);
/* Its overflow handling: out[0] pairs rescored by overflow launches, out[1] chains parked,
 * out[2] resume rounds, out[3] the first arena's capacity. */
int gs_run_multi_batch_last_info(const gs_ctx *ctx, int32_t out[4]);

/* Global aggregates of a snapshot (parity hook): C[a*W+j] = number of motif
 * segments with alphabet[a] at column j (the PFM of .fs:955-962 over ALL
 * sequences), T[a] = sum over sequences with a motif of the alphabet[a] count
 * outside the segment (createFCVWithout + fuseFrequencyVectors, .fs:945-952). */
int gs_counts(gs_ctx *ctx, int32_t W, const int32_t *pos, int64_t *C_out, int64_t *T_out);

/* --- initialiser ------------------------------------------------------- */
/* SiteSampler.getPWMOfRandomStarts (.fs:589-611): per target, start positions for
 * all other sequences, hold-one-out PWM, getBestPWMSs argmax scan with the
 * reference's in-place background drift (.fs:462-479).
 * mode 0 (exact): every target draws its own N-1 starts,
 *   r_{n,m} = gs_uniform_int(seed, stream_init(n), m, L_m-W+1)   (O(N^2) like .fs);
 * mode 1 (shared): one start vector r_m = gs_uniform_int(seed, stream_init_shared, m, ..).
 * score_out = log2 of the best window score, pos_out = its start (shard-local). */
int gs_random_starts(gs_ctx *ctx, int32_t W, double pseudo_count, uint64_t seed, int32_t mode,
                     double *score_out, int32_t *pos_out);

/* R independent getPWMOfRandomStarts runs (.fs:589-611): chain r is exactly
 * gs_random_starts(ctx, W, pc, seeds[r], mode, row r, row r), every chain in the same
 * launches over the (chain, target) pairs: the counts (mode 0) or the aggregates of the
 * shared draws (mode 1), then the scans; one synchronisation.  It follows gs_set_fixed_pcv /
 * gs_set_fixed_ppm as gs_random_starts does.  n_chains == 0 does nothing.  Returns the status
 * of the lowest-index failing chain (gs_error_index: its sequence), GS_OK if none: a chain
 * that raises (.fs:117) keeps its status in status_out[r] and its rows unspecified (its
 * starts stay valid ones), the other rows are valid.  GS_E_ARG before any launch: a bad W or
 * mode, a null seeds or output, a fixed PPM of another W.  GS_E_UNSUPPORTED: sharded
 * sequences or a communicator, chain slabs beyond 4 GiB.  The context holds no snapshot
 * afterwards and its error words are clear. */
int gs_random_starts_batch(gs_ctx *ctx, int32_t W, double pseudo_count, const uint64_t *seeds,
                           int32_t n_chains, int32_t mode,
                           double *score_out,   /* [n_chains][n_local] */
                           int32_t *pos_out,    /* [n_chains][n_local] */
                           int32_t *status_out  /* [n_chains], nullable */);
/* Device times of the last gs_random_starts_batch, ms: counts / aggregates, scans. */
int gs_starts_batch_last_ms(const gs_ctx *ctx, double out[2]);

/* SiteSampler.getBestPWMSs (.fs:462-479) of local sequence `target` against the
 * caller's background counts fcv49 (FrequencyCompositeVector, 49 slots by
 * code - 42) and position probability matrix ppm49 (49 slot rows x W, row-major),
 * with the reference's in-place background drift (quirk Q1): every window k scores
 * against fcv + (k+1) comp(source) - (the window counts of windows 0..k).
 * score_out = log2 of the first maximal window score (-inf when none is > 0 or
 * L < W), pos_out = its start (0 then).  The reference also leaves fcVector
 * mutated; the library does not write the caller's array (the F# shim in
 * INTEGRATION.md replays that bookkeeping with the reference's own helpers). */
int gs_best_pwms(gs_ctx *ctx, int32_t W, double pseudo_count, int32_t target,
                 const int32_t *fcv49, const double *ppm49, double *score_out, int32_t *pos_out);

/* --- fixed background / fixed profile --------------- */
/* The reference's …ByPCV / …WithBPV twins take the caller's
 * ProbabilityCompositeVector pcv (49 slots, .fs:103-112) instead of the
 * hold-one-out background: PWM = PPM / pcv and background categories Π pcv
 * (.fs:788-853), no background drift in the site scans (getBestPWMSsWithBPV,
 * .fs:301-313), no Checked-sum overflow.  While set (non-null; reset by
 * gs_set_sequences), EVERY entry point computes its twin: gs_motif_sweep /
 * gs_run_sweeps = findBestMotifPositionsWithStartPositionsByPCV, gs_run_greedy =
 * findBestMotifPositionsWithStartPositionByPCV, gs_random_starts =
 * getPWMOfRandomStartsWithBPV, gs_site_refine 0/-1/+1 = findBestMotifWithStartPosition
 * / getLeft / getRightShiftedBestPWMSsWithBPV.
 * gs_set_fixed_ppm: the caller's PositionProbabilityMatrix (49 slot rows x W) for the
 * initialiser only: gs_random_starts = getMotifsWithBestPWMSOfPPM (.fs:644-662), so
 * gs_motif_sampling / gs_site_sampling become doMotifSamplingWithPPM (.fs:1028-1032)
 * / doSiteSamplingWithPPM (.fs:703-707). */
int gs_set_fixed_pcv(gs_ctx *ctx, const double *pcv49);
int gs_set_fixed_ppm(gs_ctx *ctx, const double *ppm49, int32_t W);
/* The batched repetition drivers of the twins (findBestInormationContentContainingMotifsWithPCV
 * .fs:856-881, getBestPWMSsOfPPM .fs:1001-1026, getMotifsWithBestInformationContentWithBPV
 * .fs:434-459, getBestInformationContentOfPPM .fs:664-689): gs_motif_sampling_batch,
 * gs_site_sampling_batch and gs_motif_sampling_multi_batch with the caller's pcv49 (49 slots)
 * and / or ppm49 (49 slot rows x W) as arguments, either nullable.  Chain r is exactly
 * gs_motif_sampling / gs_site_sampling / gs_motif_sampling_multi with seeds[r] on a context
 * where gs_set_fixed_pcv(pcv49) and / or gs_set_fixed_ppm(ppm49, W) are set; both null is
 * exactly the plain batch.  Outputs, per-chain status, return value, n_chains == 0 and the
 * refusals are the sibling's (gs_batch_last_ms / gs_site_batch_last_ms /
 * gs_multi_batch_last_ms / gs_multi_batch_last_info report the last call of either kind).
 * GS_E_UNSUPPORTED also while the context itself holds a fixed PCV or PPM (one source of
 * the values per call: clear it and pass the values as arguments).  The call leaves the
 * context's own fixed state untouched: a later call on it computes what it would on a
 * fresh context. */
int gs_motif_sampling_batch_fixed(gs_ctx *ctx, int32_t W, double pseudo_count, double cut_off,
                                  const double *pcv49, const double *ppm49,
                                  const uint64_t *seeds, int32_t n_chains, int32_t init_mode,
                                  int32_t max_passes, int32_t *pos_out, double *pwms_out,
                                  int32_t *passes_out, int32_t *status_out);
int gs_site_sampling_batch_fixed(gs_ctx *ctx, int32_t W, double pseudo_count,
                                 const double *pcv49, const double *ppm49,
                                 const uint64_t *seeds, int32_t n_chains, int32_t init_mode,
                                 int32_t max_passes, int32_t *pos_out, double *score_out,
                                 int32_t *passes_out /* [n_chains][3], nullable */,
                                 int32_t *status_out /* [n_chains], nullable */);
int gs_motif_sampling_multi_batch_fixed(gs_ctx *ctx, int32_t motif_amount, int32_t W,
                                        double pseudo_count, double cut_off, const double *pcv49,
                                        const double *ppm49, const uint64_t *seeds,
                                        int32_t n_chains, int32_t init_mode, int32_t max_passes,
                                        int32_t cap, int32_t *cnt_out, int32_t *pos_out,
                                        double *pwms_out, int32_t *passes_out,
                                        int32_t *status_out);

/* --- site sampler --------------------------------- */
/* Site-sampler positions are (float*int)[] (.fs:589): a start in [0, L-W] and
 * the log2 score of getBestPWMSs; every array is shard-local.
 * gs_site_scan: getBestPWMSs (.fs:462-479, with the in-place background drift Q1)
 *   of every target with all other sequences at pos (one Jacobi pass; the body
 *   the refinements below share, .fs:489-507 / .fs:525-542 / .fs:560-577). */
int gs_site_scan(gs_ctx *ctx, int32_t W, double pseudo_count, const int32_t *pos,
                 double *score_out, int32_t *pos_out);
/* Refinement passes on (pos, score) = startPositions, in place:
 *   shift  0: getBestPWMSsWithStartPositions (.fs:554-585), Gauss–Seidel over the
 *             live positions (all sequences on one device, else GS_E_UNSUPPORTED);
 *   shift -1: getLeftShiftedBestPWMSs (.fs:519-550), the others at the pass-start
 *             snapshot moved one left (Jacobi: shards over ranks);
 *   shift +1: getRightShiftedBestPWMSs (.fs:483-517), moved one right.
 * A target takes the scan's result when its score is strictly larger; passes
 * repeat until a pass moves no position, at most max_passes (>= 1). */
int gs_site_refine(gs_ctx *ctx, int32_t W, double pseudo_count, int32_t shift,
                   int32_t max_passes, int32_t *pos_inout, double *score_inout,
                   int32_t *passes_out);
/* doSiteSampling (.fs:697-701): gs_random_starts(init_mode) |> refine 0 |> -1 |> +1.
 * passes_out (nullable) receives the three stages' pass counts. */
int gs_site_sampling(gs_ctx *ctx, int32_t W, double pseudo_count, uint64_t seed,
                     int32_t init_mode, int32_t max_passes, int32_t *pos_out,
                     double *score_out, int32_t *passes_out);
/* R independent doSiteSampling runs (.fs:697-701): chain r is exactly
 * gs_site_sampling(ctx, W, pc, seeds[r], init_mode, max_passes, ...).
 * pos_out / score_out: [n_chains][n_local] row-major; passes_out: [n_chains][3],
 * status_out: [n_chains] (both nullable).  Returns the status of the lowest-index failing
 * chain (gs_error_index: its sequence), GS_OK if none; the other chains' rows are still
 * valid.  The chains' starts run back to back on the context's stream, their Gauss–Seidel
 * passes as one launch of n_chains workgroups, their shifted passes together with one
 * synchronisation per pass for all chains.  n_chains == 0 does nothing.
 * GS_E_UNSUPPORTED: sharded sequences or a communicator, a fixed PCV or PPM, chain slabs
 * beyond 4 GiB, or sequences too long for the star site engine's or the scan's LDS carve
 * (loop gs_site_sampling).  The context holds no snapshot afterwards. */
int gs_site_sampling_batch(gs_ctx *ctx, int32_t W, double pseudo_count, const uint64_t *seeds,
                           int32_t n_chains, int32_t init_mode, int32_t max_passes,
                           int32_t *pos_out, double *score_out,
                           int32_t *passes_out /* [n_chains][3], nullable */,
                           int32_t *status_out /* [n_chains], nullable */);
/* Device times of the last gs_site_sampling_batch, ms: out[0] the chains' starts, out[1]
 * the batched Gauss–Seidel launch, out[2] the shifted passes (both directions). */
int gs_site_batch_last_ms(const gs_ctx *ctx, double out[3]);

/* --- counter RNG (identical on host, device and in the oracle) -------- */
double gs_uniform(uint64_t seed, uint64_t stream, uint64_t index);
uint64_t gs_stream_sweep(uint64_t sweep);

/* --- measurement ------------------------------------------------------- */
/* enable = k > 0: every k-th sweep launch (and all-reduce) is timed by hipEvents
 * attached to the dispatch on the library's stream (each timed launch widens the
 * dispatch gap by a few microseconds, so a timed run samples: k = 16 costs ~0.3 us
 * per sweep); enable = 0 switches timing off.  gs_profile_read returns the summed
 * milliseconds and the number of timed launches since the last read. */
int gs_profile_enable(gs_ctx *ctx, int32_t enable);
int gs_profile_read(gs_ctx *ctx, double *sweep_kernel_ms, int64_t *sweep_launches,
                    double *allreduce_ms, int64_t *allreduce_calls);
/* Device time of everything enqueued between the two calls (events on the
 * library's stream; no per-launch events, so no dispatch gap is widened).
 * region_end synchronises; region_stop (optional) records the stop event without
 * waiting, so that a caller's own device synchronisation ends the region and
 * region_end then only reads the time. */
int gs_profile_region_begin(gs_ctx *ctx);
int gs_profile_region_stop(gs_ctx *ctx);
int gs_profile_region_end(gs_ctx *ctx, double *ms);
/* Diagnostics, cumulative per context; fills out[0 .. min(n, GS_N_STATS)-1]:
 *  [0] sequences the certified binary32 scan could not decide (rescanned in binary64),
 *  [1] picks the binary64 scan could not certify either (one lane then redid the
 *      reference's sequential sums, .fs:747-754),
 *  [2..7] reasons for [0]: [2] a score out of range or negative, [3] the exactly
 *      recomputed weight disagreed, [4] total not separated from its error bound,
 *      [5] no candidate lane, [6] u within the bound of a CDF boundary, [7] u
 *      between two lanes' blocks,
 *  [8] sequences whose pick went through a background-weight path (the DNA
 *      sweep's, or the all-background sweep's: no motif category, or u near the
 *      background block), [9] of them, picks certified among the background
 *      categories,
 *  [10..12] the live-chain sweep's reasons for [0] besides [2..6]: [10] a window
 *      within the error bound of the cut-off, [11] more passing windows than a
 *      lane's list holds, [12] no passing window (every pick a background),
 *  [13] descriptor reads at an index outside [0, n_local) (the sweep kernels audit
 *      their descriptor loads; any nonzero value is a defect). */
#define GS_N_STATS 14
int gs_stats(gs_ctx *ctx, int64_t *out, int32_t n);
/* Name of the sweep kernel the next synchronous sweep of the current state runs
 * (for alphabets of <= 4 symbols with no other symbol, W <= 16: "gs_sweep_long_kernel"
 * from 320 windows, "gs_sweep_live_kernel" / "gs_sweep_dna_kernel" at the other sizes
 * where the packed layout is the faster one; else "gs_sweep_kernel"); for
 * measurement records.  A snapshot in the
 * all-background state (no window can pass the cut-off) is swept instead by
 * gs_sweep_bg_kernel, launched ahead of it (gs_stats [8] counts its targets). */
const char *gs_sweep_kernel_name(const gs_ctx *ctx);
/* The last gs_sweep_kernel launch of this context: out[0] its instantiation's EK
 * (4: the four-symbol kernel, 0: the general one), out[1] lanes per sequence, out[2]
 * wavefronts per workgroup, out[3] workgroups; all 0 before the first (diagnostics,
 * for tests that must know which instantiation ran). */
int gs_last_sweep_launch(const gs_ctx *ctx, int32_t *out);
/* 1 when that launch took the four-symbol kernel's one-iteration path (tuning field
 * sweep_one), else 0. */
int gs_last_sweep_one(const gs_ctx *ctx);

/* --- scan mode ---------------------------------------------------------- */
/* GS_SCAN_CERTIFIED (default): windows are scored in the log2 domain in binary32
 * under a rigorous per-sequence error bound; cut-off tests and the roulette pick
 * are decided only when the bound settles them, else in binary64.  Results are
 * identical to GS_SCAN_EXACT, which folds every window in binary64 (.fs:759-777)
 * and exists for diagnostics and parity tests. */
#define GS_SCAN_CERTIFIED 0
#define GS_SCAN_EXACT 1
int gs_set_scan_mode(gs_ctx *ctx, int32_t mode);
/* Engine tuning (no reference counterpart; results never depend on it).  Every
 * field has a fixed default -- the measured choice -- and the library
 * reads no environment variables.  Fields: blocks_per_cu_cap, group_lanes,
 * sweep_waves (1, 2, 3, 4, 6, 8, 12; at most 4 when the data hold <= 16 symbols, the pair
 * tables' kernel, else 12: a larger value fails the sweep with GS_E_ARG), dna_mode (-1 automatic, 0 general sweep kernel, 1 DNA kernel
 * whenever admissible), dna_G, live_mode (-1 automatic: the live-chain packed
 * kernel while one lane holds a sequence's windows, 0 never, 1 always when the
 * packed layout is taken), live_G, live_waves, live_max_win, live_waves_per_simd,
 * live_force (tests: every live-kernel target by the exact rescan), long_mode (-1
 * automatic: the long-sequence kernel from 320 windows, 0 never, 1 whenever it fits:
 * DNA, W <= 16, at most 512 windows), long_waves (2, 4, 8 wavefronts a workgroup), bg_mode (-1
 * automatic, 0 never, 1 whenever
 * admissible: the all-background sweep kernel), bg_G, bg_force_replay (tests:
 * its picks by the exact sequential replay), graph_mode, site_coop, coop_rate, motif_coop,
 * site_dt16, site_exit_chunk, site_exit_ratio, greedy_exit_chunk,
 * greedy_exit_ratio, greedy_waves, multi_greedy_threads, multi_spec_slots, multi_batch_fill,
 * run_batch_clear (gs_motif_run_batch: 0 a memset of the next aggregate rows before each
 * sweep, 1 a third row cleared in-kernel), run_batch_blocks (its workgroups per CU),
 * run_stats_blocks (gs_motif_run_batch_stats: workgroups per chain of a counted sweep's
 * statistics launch, 0 automatic; gs_run_sweeps_stats: the workgroups over the bins), run_stats_atomic
 * (their bins by atomic adds, 1, or plain read-modify-write, 0),
 * run_multi_arena_max (gs_motif_run_multi_batch: the combinations of up to motif_amount - 1
 * windows a target may have before its chain gets GS_E_UNSUPPORTED, 2048 .. 2^28, default
 * 2^28; for tests of that status, and the one field a chain's status depends on),
 * batch_starts (the four batched drivers' starts: 0 chain after chain on the single-chain
 * state, 1 all chains in the launches of gs_random_starts_batch, -1 automatic: 1 while the
 * sequences are fewer than 8 per compute unit, the size range where it measured faster),
 * greedy_switch, site_switch, sweep_one (the four-symbol sweep kernel's one-iteration
 * path, taken when no wavefront of the launch has more sequences than it scores at a
 * time: -1 automatic, 0 never, 1 required -- a sweep where it does not hold then fails
 * with GS_E_ARG and launches nothing).  GS_E_ARG for an unknown name or a value out of
 * range.  Set before gs_set_sequences (launch geometry is fixed there). */
int gs_set_tuning(gs_ctx *ctx, const char *name, double value);
int gs_get_tuning(const gs_ctx *ctx, const char *name, double *value);
/* Measured worst-case errors of the device's binary32 log2 / exp2 (the
 * certified scan's error model budgets 2^-20 for each). */
int gs_fastmath_check(gs_ctx *ctx, double *log2_abs_err, double *exp2_rel_err);

#ifdef __cplusplus
}
#endif
#endif
