/*
 * rsamd.h -- C ABI of the MI355X-native RANSAC-F / PnP hot path and of the bundle adjustment
 * that follows it (rs_bundle_adjust: Tables.BundleAdjustment2 as a Schur-complement
 * Levenberg-Marquardt on the GPU).
 *
 * Drop-in boundary for bioengstrom/tsbb15-3d-reconstruction-project (snapshot v0).  The
 * reference has no FFI: its boundary is the Python module surface.  Each
 * entry point below names the reference function it replaces; the Python shims in
 * tsbb15_amd/ (lab3.py, fun.py, ransac.py, pnp.py, cv.py, tables.py, features.py) bind these
 * through ctypes with the reference's names, argument meaning and ValueError behaviour.
 *
 * Conventions
 *   - every function returns int status: RS_OK (0) or a negative RS_E* code; the message of
 *     the last failure on the calling thread is rs_last_error();
 *   - host pointers are caller-owned; the library never frees or keeps them;
 *   - point sets are row-major (2, n) float64 arrays: row 0 = x (column), row 1 = y (row);
 *   - a context owns one HIP device, one HIP stream and its device buffers; calls on one
 *     context are synchronous (except the *_plan_run launches, which are stream-ordered and
 *     completed by *_plan_result) and must not be issued concurrently from two threads.
 */
#ifndef RSAMD_H
#define RSAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_OK 0
#define RS_EINVAL (-1)   /* shape / argument error  -> ValueError   */
#define RS_EDEVICE (-2)  /* HIP runtime failure     -> RuntimeError */
#define RS_ENODEV (-3)   /* no GPU visible          -> RuntimeError */
#define RS_ECOMM (-4)    /* RCCL failure            -> RuntimeError */
#define RS_ENOMEM (-5)   /* allocation failure      -> MemoryError  */

#define RS_MT_N 624      /* MT19937 state words */

const char *rs_last_error(void);
int rs_version(void);

/* ------------------------------------------------------------------------------------------
 * Host samplers (no device).  Bit-exact replays of the reference's random streams.
 * ---------------------------------------------------------------------------------------- */

/* numpy legacy RandomState: init_genrand(seed) -> key[624], pos = 624 (np.random.seed). */
int rs_np_seed(uint32_t seed, uint32_t *mt_key, int32_t *mt_pos);

/* `count` draws of np.random.choice(np.arange(n), k, replace=False) (fun.py:305-306), i.e.
 * permutation(n)[:k] by Fisher-Yates with masked-rejection random_interval.  Advances the
 * (key, pos) state in place exactly as numpy does.  out: (count, k) int32. */
int rs_np_choice_tuples(uint32_t *mt_key, int32_t *mt_pos, int64_t n, int32_t k, int64_t count,
                        int32_t *out);

/* B independent numpy streams at once on host threads (config C4: one stream per image pair,
 * np.random.seed(1000 + pair), then `count` x choice(n_b, k, replace=False)): mt_keys (B, 624),
 * mt_pos (B) advanced in place (with seeds non-null they are first set to np.random.seed(
 * seeds[b])), out (B, count, k).  Streams with n_b < k are skipped (zero output, state
 * unchanged).  threads <= 0: one per hardware thread, at most 16 (threads > 0: at most 64). */
int rs_np_choice_tuples_multi(int64_t B, const uint32_t *seeds, uint32_t *mt_keys,
                              int32_t *mt_pos, const int64_t *ns, int32_t k, int64_t count,
                              int32_t *out, int32_t threads);

/* CPython random.seed(int) with the int given as 32-bit little-endian words
 * (init_by_array) -> key[624], pos = 624. */
int rs_py_seed(const uint32_t *words, int32_t n_words, uint32_t *mt_key, int32_t *mt_pos);

/* `count` draws of ransac.gen_rnd_indices(n, k) (ransac.py:12-19): random.shuffle(
 * list(range(n)))[:k] with CPython's getrandbits rejection.  out: (count, k) int32. */
int rs_py_shuffle_tuples(uint32_t *mt_key, int32_t *mt_pos, int64_t n, int32_t k, int64_t count,
                         int32_t *out);

/* MT19937 jump-ahead: the (key, pos) state after `steps` more 32-bit outputs, computed as
 * x^J mod phi applied to the state (phi: the generator's characteristic polynomial), without
 * generating the words.  Same representation as np.random.get_state() / random.getstate():
 * key is the raw block holding the next word.  Replaces nothing in the reference; it is the
 * building block for starting many generators along one np.random / random stream. */
int rs_mt_jump(const uint32_t *mt_key, int32_t mt_pos, int64_t steps, uint32_t *key_out,
               int32_t *pos_out);

/* Self-test of the GF(2)[x] product mod phi behind the parity parse's radix-8 jump tree (level
 * polynomials x^(m 8^k J) as products, np_sampler.hip jump_polys_r): 1 iff
 * x^j1 * x^j2 mod phi == x^(j1 + j2) mod phi, 0 if not, RS_EINVAL for a negative exponent.
 * Host only; exported for the CPU test suite. */
int rs_mt_poly_selftest(int64_t j1, int64_t j2);

/* ------------------------------------------------------------------------------------------
 * Context: one per host thread; owns the device buffers, stream and RCCL communicator
 * ---------------------------------------------------------------------------------------- */
typedef struct rs_ctx rs_ctx;

int rs_device_count(int *n);
int rs_ctx_create(int device, rs_ctx **out);
int rs_ctx_destroy(rs_ctx *ctx);
int rs_ctx_synchronize(rs_ctx *ctx);

/* The same stream as rs_np_choice_tuples (k <= 8, n - 1 <= 10240), computed on the GPU of
 * `ctx`: MT19937 jump-ahead windows, the word stream in HBM, a chunked parse from every entry
 * state (hypothesis boundaries), then one lane per hypothesis for its k indices.  Same output
 * and (key, pos) advance, bit for bit; out is host memory (count, k) int32.
 * Replaces the serial host replay behind fun.py:305-306 in parity mode. */
int rs_np_choice_tuples_gpu(rs_ctx *ctx, uint32_t *mt_key, int32_t *mt_pos, int64_t n, int32_t k,
                            int64_t count, int32_t *out);

/* The same stream as rs_py_shuffle_tuples (ransac.gen_rnd_indices, ransac.py:12-19: CPython
 * random.shuffle with getrandbits rejection), k <= 8, n - 1 <= 10240, computed on the GPU by
 * the same pipeline with CPython's draw rule (w >> (32 - bit_length(i + 1)) <= i).  Same
 * output and (key, pos) advance, bit for bit; out is host memory (count, k) int32. */
int rs_py_shuffle_tuples_gpu(rs_ctx *ctx, uint32_t *mt_key, int32_t *mt_pos, int64_t n,
                             int32_t k, int64_t count, int32_t *out);

/* Sharded parity stream ("the host sampler must emit tuples in stream order
 * and hand each GPU its slice; that serial step is the scaling limiter").  The numpy (py = 0)
 * or CPython (py = 1) stream of fun.py:305-306 / ransac.py:12-19 is cut into world x Cr
 * chunks; rank r parses only its own chunks, and the ranks exchange two small records:
 *   rs_np_shard_parse    rank-local: jump to the rank's first word, generate its words, parse
 *                        its chunks from every entry state.  layout[6] = {hypotheses this
 *                        segment covers at most, C, Cr, Wc, draws, map blob bytes};
 *   rs_np_shard_maps     the rank's chunk maps as a blob                -> all-gather;
 *   rs_np_shard_compose  all ranks' blobs (rank order, `stride` bytes apart): the true entry
 *                        state of every chunk, then the rank's hypothesis starts: their number
 *                        and the first (segment draw index)          -> all-gather;
 *   rs_np_shard_tuples   the rank's hypotheses [base, hi) (global indices; base = starts of
 *                        lower ranks) as (hi - base, k) int32 rows, given the next rank's
 *                        first start; final_idx >= 0 on the rank holding start `got`: the
 *                        (key, pos) after the segment's `got` hypotheses (key_out untouched
 *                        when the state stays in the caller's block).
 * tsbb15_amd.parallel.np_sharded_segments runs the exchange; world 1 reproduces
 * rs_np_choice_tuples_gpu bit for bit. */
/* Host milliseconds this process has spent building MT19937 jump polynomials for the GPU parse
 * (once per new generator length; mt_jump.cpp's carry-less products), and the level sets built.
 * No reference counterpart: it accounts for the first-call cost of getFFromLabCode (fun.py:291). */
int rs_np_host_stats(double *jump_ms, int64_t *builds);

/* Step split of the GPU parse of the numpy stream (the sampling of fun.py:305-306): enable = 1
 * records HIP events between the steps of the following world-1 parses on this context (each
 * event is a marker between two kernels: a few microseconds each, so not in timed headline
 * runs).  Returns the last parse call's milliseconds summed over its segments, ms_out[10]:
 * 0 jump (MT windows), 1 first stream pass, 2 entry parse (with its resume launch, which waits
 * for the second pass), 3 tracking, 4 compose, 5 filter / scan / starts, 6 tuples, 7 result
 * copy, 8 the second stream pass (on the second stream, beside the entry parse), 9 the parse
 * from first to last mark; bytes_out[3]: algorithmic HBM bytes -- stream words written, chunk
 * draws read by the parse, hypothesis draws read by the tuple kernel; *segments. */
#define RS_NP_TIMING_SLOTS 10
int rs_np_timing(rs_ctx *ctx, int32_t enable, double *ms_out, double *bytes_out,
                 int64_t *segments);

typedef struct rs_np_shard rs_np_shard;
int rs_np_shard_create(rs_ctx *ctx, int64_t n, int32_t k, int32_t world, int32_t rank, int32_t py,
                       rs_np_shard **out);
int rs_np_shard_destroy(rs_np_shard *shard);
int rs_np_shard_parse(rs_np_shard *shard, const uint32_t *mt_key, int32_t mt_pos, int64_t count,
                      int64_t *layout);
int rs_np_shard_maps(rs_np_shard *shard, uint8_t *out, int64_t cap, int64_t *nbytes);
int rs_np_shard_compose(rs_np_shard *shard, const uint8_t *blobs, int64_t stride, int64_t *nstarts,
                        int64_t *first_start);
int rs_np_shard_tuples(rs_np_shard *shard, int64_t base, int64_t hi, int64_t next_start,
                       int64_t final_idx, int32_t *out, uint32_t *key_out, int32_t *pos_out);

/* ------------------------------------------------------------------------------------------
 * lab3 primitives on the GPU
 * ---------------------------------------------------------------------------------------- */

/* lab3.fmatrix_stls(pl, pr) (lab3.py:269-329): pl, pr (2, n), n >= 8; F_out (3,3) row-major,
 * pl^T F pr = 0.  n == 8 uses the batched minimal kernel, n > 8 the least-squares kernel. */
int rs_fmatrix_stls(rs_ctx *ctx, const double *pl, const double *pr, int64_t n, double *F_out);

/* Batched minimal solves: tuples (count, 8) index (2, n) point sets; F_out (count, 9). */
int rs_fmatrix_stls_batch(rs_ctx *ctx, const double *pl, const double *pr, int64_t n,
                          const int32_t *tuples, int64_t count, double *F_out);

/* lab3.fmatrix_residuals(F, x, y) (lab3.py:188-227): res_out (2, n). */
int rs_fmatrix_residuals(rs_ctx *ctx, const double *F, const double *x, const double *y,
                         int64_t n, double *res_out);

/* ------------------------------------------------------------------------------------------
 * RANSAC-F (fun.getFFromLabCode hypothesis loop, fun.py:298-328)
 * ---------------------------------------------------------------------------------------- */
#define RS_SAMPLER_PHILOX 0   /* throughput mode: counter-based Philox4x32-10 + Floyd   */
#define RS_SAMPLER_TUPLES 1   /* parity mode: host tuples (rs_np_choice_tuples stream)  */

typedef struct rs_f8_result {
  double F[9];            /* F_RANSAC, row-major (fun.py:322)                          */
  int64_t best_index;     /* hypothesis index within the run, -1 if none               */
  int64_t best_count;     /* len(S_RANSAC)                                             */
  double best_std;        /* d_RANSAC = np.std(d) of the winner (fun.py:323)           */
  double best_norm;       /* np.linalg.norm(d) of the winner                           */
  int64_t max_count_fast; /* c* of the counting kernel                                 */
  int64_t n_candidates;   /* hypotheses re-scored in float64 reference order           */
  int64_t guard_mismatch; /* candidates whose re-scored count differs from the fast one */
} rs_f8_result;

typedef struct rs_f8_candidate {
  int64_t index;          /* hypothesis index (run-local + hyp_offset)                 */
  int64_t count;          /* reference-order inlier count                              */
  double std_d;           /* np.std(d)                                                 */
  double norm_d;          /* np.linalg.norm(d)                                         */
  double F[9];
} rs_f8_candidate;

typedef struct rs_f8_plan rs_f8_plan;

/* A plan holds one correspondence set (n points) resident in HBM plus buffers for up to
 * max_hyp hypotheses per run. */
int rs_f8_plan_create(rs_ctx *ctx, int64_t n, int64_t max_hyp, rs_f8_plan **out);
int rs_f8_plan_destroy(rs_f8_plan *plan);
/* H2D upload of p1, p2 (2, n) row-major float64. */
int rs_f8_plan_set_points(rs_f8_plan *plan, const double *p1, const double *p2);
/* Enqueue one RANSAC run of H hypotheses: sample (mode), solve, count, select, re-score,
 * replay the fun.py:320-328 rule, extract inliers.  Philox mode draws hypothesis i from
 * counter (seed, hyp_offset + i); tuple mode reads host_tuples (H, 8) int32.
 * Ordering: runs issued back to back on one plan alternate between two HIP streams (the
 * context's and one owned by the plan; RSAMD_OVERLAP=0: the context's only) and may execute
 * concurrently.  Each run has its own buffer set, Philox counters and result slot, so results
 * are per run and independent of that; rs_f8_plan_result (and the accessors) wait for every run
 * in flight and return the last issued one. */
int rs_f8_plan_run(rs_f8_plan *plan, int64_t H, int32_t mode, uint64_t seed, uint64_t hyp_offset,
                   const int32_t *host_tuples, double thresh);
/* Parity-mode run: the next H tuples of the numpy legacy stream (key, pos) -- the
 * rs_np_choice_tuples stream, fun.py:305-306 -- sampled on the GPU (np_sampler.hip) straight
 * into the run's tuple buffer, then the same pipeline as rs_f8_plan_run.  Advances
 * (key, pos) in place.  Populations beyond the GPU parse (n - 1 > 10240) use the host replay. */
int rs_f8_plan_run_np(rs_f8_plan *plan, int64_t H, uint32_t *mt_key, int32_t *mt_pos,
                      double thresh);
/* Hypotheses [start, start + count) of that H-hypothesis parity run (one rank's shard of the
 * fun.py:303-328 loop): the stream of all H hypotheses is parsed on the GPU,
 * only the slice's tuples are produced and evaluated (candidate indices are local; add start),
 * and (key, pos) advance past all H, exactly as rs_f8_plan_run_np. */
int rs_f8_plan_run_np_slice(rs_f8_plan *plan, int64_t H, int64_t start, int64_t count,
                            uint32_t *mt_key, int32_t *mt_pos, double thresh);
/* Parity mode, sharded: this rank's hypotheses [base, hi) of a sharded parse (rs_np_shard_*
 * after compose) produced straight into the run's tuple buffer, then the same pipeline as
 * rs_f8_plan_run (candidate indices are run-local: add base).  hi == base runs nothing and
 * only reads the final state (final_idx >= 0). */
int rs_f8_plan_run_np_shard(rs_f8_plan *plan, rs_np_shard *shard, int64_t base, int64_t hi,
                            int64_t next_start, int64_t final_idx, uint32_t *key_out,
                            int32_t *pos_out, double thresh);
/* Wait for the last run and copy its result; inliers (S_RANSAC, ascending) up to cap. */
int rs_f8_plan_result(rs_f8_plan *plan, rs_f8_result *out, int64_t *inliers, int64_t cap,
                      int64_t *n_inliers);
/* Candidates (count == max re-scored count) of the last run, ascending index, up to cap. */
int rs_f8_plan_candidates(rs_f8_plan *plan, rs_f8_candidate *out, int64_t cap, int64_t *n_out);
/* Per-hypothesis fast counts / models of the last run (test & diagnostics). */
/* Counting precision of later runs: fp64 != 0 selects the plain float64 counting kernel
 * (reference-order residuals, no fp32 filter); 0 (default) the fp32 kernel with its exact
 * float64 guard band.  Both give bit-identical counts; fp64 is the slower reference form. */
int rs_f8_plan_set_count_precision(rs_f8_plan *plan, int32_t fp64);
int rs_f8_plan_counts(rs_f8_plan *plan, int32_t *counts, int64_t H);
int rs_f8_plan_models(rs_f8_plan *plan, double *F_out, int64_t H);
/* Host waits for one stream lane taken outside rs_f8_plan_result and the other synchronising
 * calls, since the plan was created: the parity entry points (rs_f8_plan_run_np*) wait for
 * lane 1 before their parse, and a run that meets a buffer set still in use on the other lane
 * waits for that lane.  Stays 0 in any sequence of Philox and host-tuple runs. */
int rs_f8_plan_lane_waits(rs_f8_plan *plan, int64_t *waits);
/* The pruned count of the last run (fp32 counting, RSAMD_PRUNE=1): out = {L, K, survivors,
 * npad}.  L is the best full count among the first RSAMD_PRUNE_SAMPLE hypothesis groups, K the
 * number of points every other hypothesis was counted over before the hopeless ones (those that
 * could no longer reach L - 1) were dropped, survivors the hypotheses counted to the end.  A
 * run that was not pruned reports K = npad and no survivors.  Results are those of the
 * unpruned count in every field; rs_f8_plan_counts recounts after a pruned run. */
int rs_f8_plan_prune_stats(rs_f8_plan *plan, int64_t out[4]);
/* The carried bound (fp32 counting, RSAMD_PRUNE=1, RSAMD_CARRY=1): a run on a stream lane whose
 * previous run had the same H and threshold over the same points has no sample; its L (as
 * rs_f8_plan_prune_stats reports it) is that run's best count less a gap (RSAMD_CARRY_GAP).  Such
 * a run is exact when the best full count among its survivors reaches L, which is checked on the
 * device; otherwise the run "fell back": its last kernel selects nothing, and every hypothesis is
 * counted again without pruning when the run is read, inside the first of rs_f8_plan_result and
 * the accessors below called after it.  Only the last run issued can be read; a fallen-back run
 * that is followed by another run, by rs_f8_plan_set_points, rs_f8_plan_set_count_precision or
 * rs_f8_plan_destroy before it is read is never counted again and has no result (the accessors
 * return RS_EINVAL for it until the next run is issued).
 * Results are those of the unpruned count either way.  out = {runs carried since the plan was
 * created, runs among them that fell back, whether the last run was carried, whether it fell
 * back}.  set_points, a retarget, rs_f8_plan_set_count_precision and a run with another H or
 * threshold end the carry: the next run on each lane takes a sample again. */
int rs_f8_plan_carry_stats(rs_f8_plan *plan, int64_t out[4]);
/* out = {fallen-back runs counted again when they were read, since the plan was created; the
 * kernel launches the last run enqueued for its count: 3 with a sample (sample, prefix, rest), 2
 * for a carried run, 1 unpruned, 2 for the float64 kernel and its maximum}.  Host state: no wait. */
int rs_f8_plan_recount_stats(rs_f8_plan *plan, int64_t out[2]);
/* Point order of the pruned count (RSAMD_ORDER=0 turns it off).  A count is a sum over the points
 * and the pruned count's drop rule holds for any fixed order of them, so the counting stages may
 * read the points in an order of the plan's own: the points that a previous run's winner rejected
 * first, where a hypothesis survives the screen only if it finds its inliers among them.  The
 * order is installed once per rs_f8_plan_set_points, inside the first of rs_f8_plan_result and the
 * accessors that completes a run after more than one run has been issued on the resident points
 * (one small upload and one small kernel there; a plan with one run per rs_f8_plan_set_points never
 * installs one); rs_f8_plan_set_points and a new population drop it.  Runs that read the ordered
 * copy screen with the margin max(16, n / 60) unless RSAMD_PRUNE_MARGIN is set.  Results are those of the
 * caller's order, bit for bit; only the stages' own counts of dropped hypotheses
 * (rs_f8_plan_stage_counts) and the survivor count differ.  out = {whether an order is installed,
 * the points placed first, installs since the plan was created}.  Host state: no wait, no install. */
int rs_f8_plan_order_stats(rs_f8_plan *plan, int64_t out[3]);
/* The counting stages' own per-hypothesis counts of the last run, with no recount (test &
 * diagnostics).  After a pruned run: the full count of a sample hypothesis or a survivor, and
 * for a dropped hypothesis K minus its certified outliers among the first K points, an upper
 * bound of its count there (below L - 1 - (n - K)).  Otherwise what rs_f8_plan_counts returns. */
int rs_f8_plan_stage_counts(rs_f8_plan *plan, int32_t *counts, int64_t H);
/* Device time (ms, HIP events on the run's stream lane; a run that records them runs its
 * counting kernel alone, without the other lane's kernels beside it) of the counting kernel,
 * the solve kernel and the whole run: of the last run, or averaged over the last `last_n` runs (<= 64).  Runs
 * may be issued back to back (each owns a result slot in pinned host memory: the header and
 * S_RANSAC, written by the run's last kernel); rs_f8_plan_result waits for the last. */
int rs_f8_plan_kernel_ms(rs_f8_plan *plan, double *score_ms, double *solve_ms, double *total_ms);
/* Timing events recorded by rs_f8_plan_run (each is a marker packet between two kernels,
 * ~3.5 us on MI355X): level 0 none, 1 around the counting kernel (default), 2 also around the
 * solve and the whole run (solve_ms / total_ms are -1 below level 2); `every` = record them on
 * every k-th run only (kernel_avg averages the timed runs among the last `last_n`). */
int rs_f8_plan_set_timing(rs_f8_plan *plan, int32_t level, int32_t every);
int rs_f8_plan_kernel_avg(rs_f8_plan *plan, int64_t last_n, double *score_ms, double *solve_ms,
                          double *total_ms);

/* One call: numpy-exact sampling (advancing mt_key/mt_pos in place) + GPU evaluation. */
int rs_f8_ransac_np(rs_ctx *ctx, const double *p1, const double *p2, int64_t n, int64_t H,
                    uint32_t *mt_key, int32_t *mt_pos, double thresh, rs_f8_result *out,
                    int64_t *inliers, int64_t cap, int64_t *n_inliers);

/* ------------------------------------------------------------------------------------------
 * PnP (pnp.py:132-160 DLT; ransac.py:37-113 consensus semantics)
 * ---------------------------------------------------------------------------------------- */
typedef struct rs_pnp_result {
  double R[9];
  double t[3];
  int64_t best_index;
  int64_t best_count;     /* D_med consensus size (ransac.py:104,108)                  */
} rs_pnp_result;

/* DLT pose from m >= 6 correspondences: X (m,3) world points, y (m,3) C-normalised
 * homogeneous image points (pnp.py:132-160).  R_out (3,3), t_out (3). */
int rs_pnp_dlt(rs_ctx *ctx, const double *X, const double *y, int64_t m, double *R_out,
               double *t_out);

/* RANSAC over minimal samples (ransac.py:37-113).  Tuples (H, k) index the `high` set;
 * consensus e = |pi(y) - pi(R x + t)|^2 <= thresh is counted on the `med` set.  mode as for
 * F; in tuple mode host_tuples come from rs_py_shuffle_tuples.  k in [6, 16]: the DLT
 * (pnp.py:132-160).  k = 3: the reference's p3p branch (ransac.py:81-82, 91-111), Lambda
 * Twist P3P with every pose of a trial scored (best_index is the trial).  The k = 3 winner is
 * chosen in two classes: the first (trial-major, pose-minor) front-facing pose with the largest
 * count, unless the best mirrored-depth pose counts more than twice as many (kMirrorCountWins =
 * 2; then the first such mirrored pose) -- so a mirrored pose with a higher count can lose.
 * Counts are exact in the reference's arithmetic (rs_pnp_count_poses), and the call fails with
 * RS_EDEVICE if the winner's count differs from its D_med consensus size.  Replaces
 * ransac.ransac_robust's loop (ransac.py:72-111). */
/* HIP events around rs_pnp_ransac's solve and count kernels (ransac.py:93-105's work): enable = 1
 * records them in the following calls; returns the last timed call's milliseconds (-1: none). */
int rs_pnp_timing(rs_ctx *ctx, int32_t enable, double *solve_ms, double *count_ms);
int rs_pnp_ransac(rs_ctx *ctx, const double *X_med, const double *y_med, int64_t m_med,
                  const double *X_high, const double *y_high, int64_t m_high, int32_t k,
                  int64_t H, int32_t mode, uint64_t seed, const int32_t *host_tuples,
                  double thresh, rs_pnp_result *out, int64_t *inl_med, int64_t *n_inl_med,
                  int64_t *inl_high, int64_t *n_inl_high);

/* Consensus counts of H given poses (H x 12: R row-major, then t) on m correspondences X (m,3),
 * y (m,3): the scoring of ransac.py:96-105 (`thresh >= dpp_squared(y, R x + t)`) with the same
 * kernel rs_pnp_ransac counts with -- division-free, pairs within a rigorous error band of the
 * threshold re-tested in the reference's arithmetic, so every count equals the reference-order
 * count.  counts_out: H int32. */
int rs_pnp_count_poses(rs_ctx *ctx, const double *X, const double *y, int64_t m,
                       const double *poses, int64_t H, double thresh, int32_t *counts_out);

/* Minimal solvers of the OpenCV drop-ins: RS_PNP_DLT6 the reference's DLT (pnp.py:132-160) on
 * 6-point samples, RS_PNP_EPNP5 EPnP on 5-point samples (OpenCV's solvePnPRansac kernel),
 * RS_PNP_P3P Lambda-Twist P3P on 4-point samples (3 solve, the 4th chooses; OpenCV's kernel
 * for 4 correspondences and for SOLVEPNP_P3P; the reference's unfinished p3p_twist,
 * pnp.py:61-121). */
#define RS_PNP_DLT6 0
#define RS_PNP_EPNP5 1
#define RS_PNP_P3P 2

/* EPnP over all m >= 4 correspondences (method RS_PNP_EPNP5) or P3P over exactly 4
 * (RS_PNP_P3P): X (m,3), y (m,3) C-normalised homogeneous image points; R_out (3,3), t_out
 * (3), err_out = mean reprojection error in normalised units (inf: no pose).  cv.solvePnP
 * with SOLVEPNP_EPNP / SOLVEPNP_P3P (pnp.py:7-10 calls cv.solvePnP). */
int rs_pnp_minimal(rs_ctx *ctx, const double *X, const double *y, int64_t m, int32_t method,
                   double *R_out, double *t_out, double *err_out);

/* Levenberg-Marquardt refinement of a pose (R row-major 3x3, t) on the PIXEL reprojection error
 * |K pi(R x + t) - uv|^2 over m correspondences: the refinement stage of cv.solvePnP with
 * SOLVEPNP_ITERATIVE (pnp.py:7-10) and of cv.solvePnPRansac (tables.py:141-147).  One GPU
 * workgroup; left-multiplied rotation steps, Marquardt damping, only cost-lowering steps taken,
 * at most max_jac Jacobians (OpenCV's CvLevMarq: 20), stop at a relative step below FLT_EPSILON.
 * R_io / t_io are updated in place; cost_out (4 doubles, may be null): initial and final
 * 0.5 |r|^2, Jacobians evaluated, steps taken. */
int rs_pnp_refine_lm(rs_ctx *ctx, const double *X, const double *uv, int64_t m, const double *K,
                     double *R_io, double *t_io, int32_t max_jac, double *cost_out);

/* cv.solvePnPRansac drop-in (tables.py:141-145 call site): world points X (m,3), PIXEL
 * image points uv (m,2), camera matrix K (3,3 row-major, upper triangular), zero distortion.
 * Up to max_iters hypotheses (Philox samples from `seed` of the method's minimal size: EPnP
 * on 5 points as OpenCV's kernel, P3P on 4, or the DLT on 6 with the sample's world points
 * centred and RMS-scaled) are solved and counted on the GPU with OpenCV's pixel test
 * |K pi(R x + t) - uv|^2 <= reproj_err^2; OpenCV's sequential loop (a model wins with
 * goodCount > max(best, model_points - 1), then RANSACUpdateNumIters(confidence, outlier
 * ratio, model_points, niters) shrinks the budget) is replayed over that hypothesis order.
 * guess (R row-major then t, 12 doubles, or null): scored first, as hypothesis 0 (the
 * extrinsic guess of useExtrinsicGuess).  out->best_index = -1 when nothing wins;
 * *iters_used = hypotheses the loop consumed; inliers (<= m) in point order. */
int rs_pnp_ransac_cv(rs_ctx *ctx, const double *X, const double *uv, int64_t m, const double *K,
                     int64_t max_iters, uint64_t seed, double reproj_err, double confidence,
                     int32_t method, const double *guess, rs_pnp_result *out, int64_t *inliers,
                     int64_t *n_inliers, int64_t *iters_used);

/* ------------------------------------------------------------------------------------------
 * Five-point essential matrix (Nister) and E-RANSAC.  No reference counterpart (SURVEY.md 8(a)
 * row a-15, north_star "5-point E"); the reference's convention: y1^T E y2 = 0, E = R^T [t]_x
 * (fun.py:12-21), F = K1^-T E K2^-1 in pixels.
 * ---------------------------------------------------------------------------------------- */
typedef struct rs_e5_result {
  double E[9];            /* winning essential matrix (unit Frobenius norm), row-major      */
  double F[9];            /* its pixel-space F = K1^-T E K2^-1                               */
  int64_t best_sample;    /* minimal sample of the winner, -1 if none                       */
  int64_t best_solution;  /* which of that sample's real solutions (0..9)                   */
  int64_t best_count;     /* consensus size                                                 */
} rs_e5_result;

/* All real solutions of S minimal samples: y1, y2 (5 S, 3) homogeneous C-normalised points,
 * sample s = rows 5s .. 5s+4.  E_out (S, 10, 9): unit-norm solutions, NaN past nsol[s]. */
int rs_e5_solve(rs_ctx *ctx, const double *y1, const double *y2, int64_t S, double *E_out,
                int32_t *nsol);

/* E-RANSAC over S Philox 5-point samples of n pixel correspondences p1, p2 ((2, n) each, the
 * layout of fun.py:298) with cameras K1, K2: every real solution is a hypothesis, scored with
 * the reference's F-RANSAC test (lab3.fmatrix_residuals, max(|r1|, |r2|) < thresh, fun.py:
 * 315-317); among the hypotheses with the largest count the smallest ||d|| (d_i =
 * max(|r1_i|, |r2_i|) over all points, fun.py:317) wins, the first on equal norms. */
int rs_e5_ransac(rs_ctx *ctx, const double *p1, const double *p2, int64_t n, const double *K1,
                 const double *K2, int64_t S, uint64_t seed, double thresh, rs_e5_result *out,
                 int64_t *inliers, int64_t *n_inliers);

/* ------------------------------------------------------------------------------------------
 * Batched RANSAC-F over many image pairs (config C4; fun.py:298-328 per pair)
 * ---------------------------------------------------------------------------------------- */
typedef struct rs_pair_result {
  double F[9];            /* F_RANSAC of the pair (NaN if none)                          */
  int64_t best_index;     /* winning hypothesis, -1 if none (N < 8 or no consensus)      */
  int64_t best_count;     /* len(S_RANSAC)                                               */
  double best_std;        /* d_RANSAC = np.std(d)                                        */
  double best_norm;       /* np.linalg.norm(d) of the winner                             */
  int64_t n_candidates;   /* hypotheses with count == c*                                 */
} rs_pair_result;

/* H hypotheses for each of B pairs in one pass.  p1, p2: (2, total) point sets of all pairs
 * concatenated, pair b = columns off[b] .. off[b+1]-1 (off: B+1 entries, off[0] = 0).
 * Philox mode: pair b draws from seed_base + id_b with counters 0..H-1 (the stream of
 * rs_f8_plan_run(seed = seed_base + id_b)), id_b = seed_ids[b] or b when seed_ids is NULL;
 * tuple mode: host_tuples (B, H, 8) int32.  Pairs with
 * N < 8 are skipped (best_index -1).  Counts use the reference-order float64 distance.
 * out (B); inliers (total) int32: S_RANSAC of pair b at inliers[off[b] .. off[b]+count-1]. */
int rs_pairs_f8_ransac(rs_ctx *ctx, const double *p1, const double *p2, const int64_t *off,
                       int64_t B, int64_t H, int32_t mode, uint64_t seed_base,
                       const int64_t *seed_ids, const int32_t *host_tuples, double thresh,
                       rs_pair_result *out,
                       int32_t *inliers);

/* ------------------------------------------------------------------------------------------
 * Two-view geometry after RANSAC (fun.py:91-102, 209-280, 336-369; lab3.py:331-475)
 * ---------------------------------------------------------------------------------------- */

/* lab3.triangulate_optimal (lab3.py:382-475), batched.  C1, C2: (n_cam, 3, 4) camera pairs;
 * x1, x2: (2, n) point sets (row 0 = x); cam: (n) int32 pair index per point, or NULL for
 * pair 0; X_out: (n, 3). */
int rs_triangulate_optimal(rs_ctx *ctx, const double *C1, const double *C2, int64_t n_cam,
                           const double *x1, const double *x2, const int32_t *cam, int64_t n,
                           double *X_out);

/* fun.camera_resectioning (fun.py:260-280, specRQ 181-188), batched: P (B, 3, 4) ->
 * K (B, 3, 3) upper triangular with K[2,2] = 1, R (B, 3, 3) rotation, t (B, 3). */
int rs_camera_resectioning(rs_ctx *ctx, const double *P, int64_t B, double *K, double *R,
                           double *t);

/* E = K^T F K of fun.getEAndK (fun.py:101), batched: F (B, 3, 3); K (B, 3, 3), or a single
 * (3, 3) K for all when one_k != 0. */
int rs_essential_from_f(rs_ctx *ctx, const double *K, int32_t one_k, const double *F, int64_t B,
                        double *E);

/* fun.relative_camera_pose (fun.py:209-258), batched: E (B, 3, 3); y1, y2 (B, 2) the
 * C-normalised first correspondence (main.py:63).  R (B, 3, 3), t (B, 3); found (B) = 1..4,
 * the candidate taken, or 0 where the reference returns None (R, t NaN). */
int rs_relative_camera_pose(rs_ctx *ctx, const double *E, const double *y1, const double *y2,
                            int64_t B, double *R, double *t, int32_t *found);

/* lab3.fmatrix_cameras (lab3.py:353-380): F (B, 3, 3) -> C1 (B, 3, 4); C2 = [I | 0]. */
int rs_fmatrix_cameras(rs_ctx *ctx, const double *F, int64_t B, double *C1);

/* lab3.fmatrix_from_cameras (lab3.py:331-351): C1, C2 (B, 3, 4) -> F (B, 3, 3). */
int rs_fmatrix_from_cameras(rs_ctx *ctx, const double *C1, const double *C2, int64_t B,
                            double *F);

typedef struct rs_gs_info {
  double cost_init;       /* 0.5 |r|^2 at the start (cameras of F_RANSAC, optimal points)  */
  double cost;            /* 0.5 |r|^2 at the end                                          */
  int32_t iterations;     /* linearisations                                                */
  int32_t accepted;       /* accepted LM steps                                             */
  int32_t status;         /* 0 max_iter, 1 converged (ftol/xtol 1e-15), 2 no further decrease */
  int32_t n;              /* inliers of the pair                                           */
} rs_gs_info;

/* The residual of lab3.fmatrix_residuals_gs (lab3.py:228-266) at the parameter vector x
 * (12 camera entries row-major, then n points xyz; f: 4n, order left x, left y, right x,
 * right y) and, when J is non-null, the forward-difference Jacobian scipy's
 * least_squares(jac='2-point') forms (fun.py:358): the (4n, 12 + 3n) Jacobian stored
 * column-major (J[j * 4n + i] = dF_i / dx_j, scipy's Fortran-ordered J_transposed.T), column
 * j = (f(x with x_j -> xp[j]) - f(x)) / dx[j]; xp and dx are the caller's (scipy's step rule).
 * The projection copies the FMA chain of one OpenBLAS dgemm microkernel (the one
 * OpenBLAS 0.3.29 DYNAMIC_ARCH picks on the build container's SkylakeX cores,
 * tests/golden/gs_trace_blas.json), so f equals the reference's residual bit for bit where
 * numpy runs that kernel; under another BLAS kernel (another CPU type, MKL, a threaded or
 * small-matrix path) the reference's own bits differ and the equality is not guaranteed --
 * the tests then skip the bit-equality assertions.  The host-side TRF iteration of the
 * reference-faithful gold standard calls this. */
int rs_gs_residuals_fd(rs_ctx *ctx, const double *x, const double *xp, const double *dx,
                       const double *pl, const double *pr, int64_t n, double *f, double *J);

/* The gold-standard tail of fun.getFFromLabCode (fun.py:336-369), batched over pairs:
 * F (B, 3, 3) = F_RANSAC per pair; pl, pr (2, total) the inlier points of all pairs
 * concatenated, pair b = columns off[b] .. off[b+1]-1 (off has B+1 entries, off[0] = 0).
 * Minimises lab3.fmatrix_residuals_gs over (C1, X) to convergence (LM, Schur complement).
 * F_gold (B, 3, 3); optional C1_out (B, 3, 4) and X_out (total, 3); info (B). */
int rs_gold_standard(rs_ctx *ctx, const double *F, const double *pl, const double *pr,
                     const int64_t *off, int64_t B, int32_t max_iter, double *F_gold,
                     double *C1_out, double *X_out, rs_gs_info *info);

/* Config C4 end to end (run_pairs with a refiner: fun.py:298-328, 336-369 and main.py:50-63 per
 * pair) in one call: rs_pairs_f8_ransac's stages, then for every pair with a consensus
 * (best_index >= 0 and best_count > 0) rs_gold_standard (max_iter) on its S_RANSAC points,
 * and -- when K (3, 3) is given -- E = K^T F_gold K and rs_relative_camera_pose on y1[b], y2[b]
 * (B, 2), the caller's C-normalised first correspondence of each pair.  Everything between the
 * stages stays on the device (the inlier points are gathered there): one upload, one download.
 * Outputs as the three calls': out (B), inliers (total), F_gold (B, 3, 3), info (B), R (B, 3, 3),
 * t (B, 3), found (B).  Pairs without a consensus: F_gold, R, t NaN, info zero, found 0; K NULL:
 * R, t NaN and found 0 for every pair. */
int rs_pairs_two_view(rs_ctx *ctx, const double *p1, const double *p2, const int64_t *off,
                      int64_t B, int64_t H, int32_t mode, uint64_t seed_base,
                      const int64_t *seed_ids, const int32_t *host_tuples, double thresh,
                      int32_t max_iter, const double *K, const double *y1, const double *y2,
                      rs_pair_result *out, int32_t *inliers, double *F_gold, rs_gs_info *info,
                      double *R, double *t, int32_t *found);

/* ------------------------------------------------------------------------------------------
 * Per-view SfM steps around PnP (tables.py, fun.py:12-21)
 * ---------------------------------------------------------------------------------------- */

/* The 2D<->3D matching loop of Tables.addNewView (tables.py:116-135): for each query (n, 3)
 * (C-normalised homogeneous y1), the point index obs_point[k] of the FIRST observation k of
 * obs (m, 3) -- the last view's observations in observations_index order -- with
 * ||obs_k - query|| < tol, else -1.  out: (n) int64. */
int rs_match_observations(rs_ctx *ctx, const double *obs, const int64_t *obs_point, int64_t m,
                          const double *queries, int64_t n, double tol, int64_t *out);

/* fun.getEFromCameras (fun.py:12-21), batched: C1, C2 (n, 3, 4) = [R | t] -> E (n, 3, 3). */
int rs_e_from_cameras(rs_ctx *ctx, const double *C1, const double *C2, int64_t n, double *E);

/* Tables.addNewPoints (tables.py:161-175) without the table bookkeeping: C1, C2 (3, 4) the two
 * views' [R | t]; y1, y2 (n, 3) C-normalised homogeneous putative correspondences.
 * mask (n) int32 = |y1^T E y2| < gate; X (n, 3) = lab3.triangulate_optimal of the accepted
 * (NaN where rejected). */
int rs_add_new_points(rs_ctx *ctx, const double *C1, const double *C2, const double *y1,
                      const double *y2, int64_t n, double gate, int32_t *mask, double *X);

/* EpsilonBA of Tables.BundleAdjustment2 (tables.py:264-293): cams (nC, 3, 4) as 12 free
 * parameters each, pts (nP, 3), observations (obs_view, obs_point int32, uv (n, 2)).
 * r (2n) = interleaved [u - c1.x / c3.x, v - c2.x / c3.x]. */
int rs_ba_residuals(rs_ctx *ctx, const double *cams, int64_t nC, const double *pts, int64_t nP,
                    const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                    int64_t n, double *r);

/* Jacobian blocks of rs_ba_residuals per observation (the nonzeros of Tables.sparsity_mask,
 * tables.py:339-372): Jc (n, 2, 12) w.r.t. the camera's row-major entries, Jp (n, 2, 3). */
int rs_ba_jacobian(rs_ctx *ctx, const double *cams, int64_t nC, const double *pts, int64_t nP,
                   const int32_t *obs_view, const int32_t *obs_point, int64_t n, double *Jc,
                   double *Jp);

/* Tables.BundleAdjustment2 (tables.py:260-338): the objective of rs_ba_residuals minimised over
 * the cameras (12 free parameters each, camera 0 never touched) and the points by
 * Levenberg-Marquardt, fp64 throughout, the points eliminated by a Schur complement and the
 * reduced camera system solved by Cholesky on the GPU.  cams (nC, 3, 4) and pts (nP, 3) are
 * refined in place.  The rules are those of oracle/tables_ref.bundle_adjust_lm:
 *   - lam = 1e-3, nu = 2 at the start; V* = V + lam diag(V), U* = U + lam diag(U);
 *   - a trial is accepted iff cost_new < cost and the predicted reduction is > 0; then
 *     lam *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; otherwise lam *= nu, nu *= 2;
 *   - a trial with a non-positive Cholesky pivot or a non-finite cost is a rejected trial;
 *   - status 1: an accepted step gained <= ftol * cost; 2: lam > 1e32; 0: max_iter
 *     linearisations done.
 * Cameras and points without an observation come back bit for bit unchanged and stay out of the
 * linear system; nC == 1 refines the points only.  RS_EINVAL: an index out of range, n == 0, a
 * non-finite initial cost, nC > RS_BA_MAX_CAMERAS, n > 2^24, or more than 2^27 pairs of
 * observations that share a point between two free cameras.  The same inputs give bitwise the
 * same outputs (no floating-point atomics; every sum in a fixed order). */
#define RS_BA_MAX_CAMERAS 128   /* reduced system up to 1524 x 1524 */

typedef struct rs_ba_info {
  double cost_init;       /* 0.5 |r|^2 at the start                                        */
  double cost;            /* 0.5 |r|^2 at the end                                          */
  double lambda;          /* the damping after the last trial                              */
  int32_t iterations;     /* linearisations                                                */
  int32_t rejected;       /* rejected trials                                               */
  int32_t status;         /* 0 max_iter, 1 converged (ftol), 2 lam > 1e32                  */
  int32_t reserved;
} rs_ba_info;             /* 40 bytes */

int rs_bundle_adjust(rs_ctx *ctx, double *cams, int64_t nC, double *pts, int64_t nP,
                     const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                     int64_t n, int32_t max_iter, double ftol, rs_ba_info *info);

/* Bundle adjustment over rigid poses: the objective, LM rules, Schur structure, layouts, limits,
 * rs_ba_info and determinism of rs_bundle_adjust, with 6 local coordinates per camera in place
 * of 12 free entries.  Camera k is [R | t]; the update delta = (omega, tau) acts on the left,
 *   R+ = Exp(omega) R,  t+ = Exp(omega) t + tau   (so Xc+ = Exp(omega) Xc + tau),
 * Exp = I + A K + B K^2 with K = [omega]x, A = sin th / th, B = (sin(th/2) / (th/2))^2 / 2
 * (their series below th^2 = 1e-12).  With Xc = (x, y, z), a = x/z, b = y/z, iz = 1/z:
 *   d r / d delta = -[[-ab, 1+a^2, -b, iz, 0, -a iz], [-(1+b^2), ab, a, 0, iz, -b iz]].
 * R is never re-orthonormalised: Exp(omega) R keeps R^T R = I to rounding.  Only the global
 * scale remains as gauge; it is left to the damping.  The free cameras are cameras 1.. with an
 * observation; camera 0, unobserved cameras and unobserved points come back bit for bit and are
 * not looked at.  RS_EINVAL as rs_bundle_adjust, and for a free camera whose R has
 * max |R^T R - I| > 1e-6 or det R <= 0 (the message names the camera).  cams go in and come
 * out as (nC, 3, 4).  rs_ba_timing covers this call with the same 8 slots. */
int rs_bundle_adjust_rigid(rs_ctx *ctx, double *cams, int64_t nC, double *pts, int64_t nP,
                           const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                           int64_t n, int32_t max_iter, double ftol, rs_ba_info *info);

/* Bundle adjustment under a robust loss (scipy.optimize.least_squares' loss= / f_scale=, which
 * the reference's BundleAdjustment2 could pass and the two calls above lack).  rigid == 0: the
 * cameras of rs_bundle_adjust, rigid != 0: those of rs_bundle_adjust_rigid with its rotation
 * check.  Per observation i with the residual (ru, rv) of rs_ba_residuals, s_i = ru^2 + rv^2,
 * z_i = s_i / C^2, C = f_scale:
 *   cost = 0.5 C^2 sum_i rho(z_i),
 *   loss 0 linear   rho = z                                  w = rho' = 1
 *        1 soft_l1  rho = 2 (sqrt(1 + z) - 1)                w = 1 / sqrt(1 + z)
 *        2 huber    rho = z (z <= 1), 2 sqrt(z) - 1 (z > 1)  w = 1 (z <= 1), 1 / sqrt(z)
 *        3 cauchy   rho = log1p(z)                           w = 1 / (1 + z)
 * scipy's names and forms; unlike scipy, rho acts on the squared norm of the observation's
 * residual, not on ru and rv separately.  The iteration is the LM of rs_bundle_adjust, rule for
 * rule, on the re-weighted problem (IRLS; Triggs' first-order form, no rho'' term): at every
 * linearisation w_i is taken from the residuals of the accepted state, r, Jc and Jp of
 * observation i are scaled by sqrt(w_i), and U, V, W, the gradients, the Schur complement, the
 * Cholesky and the predicted reduction are formed from the scaled quantities.  The weights stay
 * fixed over the rejected trials of one linearisation; a trial's cost is the robust cost of the
 * trial state.  info->cost_init and info->cost are robust costs.  weights (n), which may be
 * NULL, gets w_i at the returned state (all 1.0 for loss 0).  loss 0 is rs_bundle_adjust /
 * rs_bundle_adjust_rigid bit for bit, whatever f_scale.  Determinism, limits and the unobserved
 * cameras and points as rs_bundle_adjust.  RS_EINVAL as the two calls above, and for loss
 * outside 0..3 or f_scale not finite or <= 0.  rs_ba_timing covers this call: the weights of
 * the linearisation count in the k_ba_linearize slot, the final weights in the last slot. */
#define RS_BA_LOSS_LINEAR 0
#define RS_BA_LOSS_SOFT_L1 1
#define RS_BA_LOSS_HUBER 2
#define RS_BA_LOSS_CAUCHY 3
int rs_bundle_adjust_robust(rs_ctx *ctx, double *cams, int64_t nC, double *pts, int64_t nP,
                            const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                            int64_t n, int32_t max_iter, double ftol, int32_t rigid, int32_t loss,
                            double f_scale, double *weights, rs_ba_info *info);

/* HIP events between the kernels of the next rs_bundle_adjust / rs_bundle_adjust_rigid /
 * rs_bundle_adjust_robust calls
 * (enable != 0; the rigid call's linearisation counts in the k_ba_linearize slot).  Returns the
 * last timed call's device ms summed per kernel -- k_ba_linearize, k_ba_camera, k_ba_pointsum,
 * k_ba_point, k_ba_schur, k_ba_chol, k_ba_step, k_ba_cost + k_ba_final -- and its trials. */
#define RS_BA_TIMING_SLOTS 8
int rs_ba_timing(rs_ctx *ctx, int32_t enable, double *ms, int64_t *trials);

/* ------------------------------------------------------------------------------------------
 * The wash step (wash.hip): the two steps main.py names and leaves empty.  cams, pts,
 * obs_view, obs_point and uv have the layout of rs_bundle_adjust.  A point's track is its
 * observations in ascending observation index.
 * ------------------------------------------------------------------------------------------ */
#define RS_WASH_MAX_TRACK 128          /* observations of one point; = RS_BA_MAX_CAMERAS */

/* N-view triangulation, the "Re-triangulate" of main.py:101-107 without its robustness (the
 * reference has only the two-view tables.py:161-175): every point from all its observations.
 * The start is the inhomogeneous linear solution of the 2m equations (u c3 - c1).[X;1] = 0,
 * (v c3 - c2).[X;1] = 0 through the 3x3 normal equations and Cholesky; then Levenberg-Marquardt
 * on X in R^3 (Marquardt diagonal damping, lambda0 = 1e-3, Nielsen's update, at most 20
 * linearisations, stop when an accepted step gains <= 1e-15 cost or lambda > 1e32: the scheme
 * of rs_bundle_adjust).  ok[j] = 0 (and pts[j] untouched) for a point with < 2 observations, a
 * singular start or a non-finite result.  RS_EINVAL as rs_wash_points. */
int rs_triangulate_nview(rs_ctx *ctx, const double *cams, int64_t nC, double *pts, int64_t nP,
                         const int32_t *obs_view, const int32_t *obs_point, const double *uv,
                         int64_t n, int32_t *ok);

typedef struct rs_wash_info {
  int64_t hypotheses;        /* valid two-view hypotheses scored */
  int32_t obs_removed, points_removed, points_failed, reserved;
} rs_wash_info;              /* 24 bytes */

/* WASH1 (main.py:101-107, "Remove bad 3D points. Re-triangulate & Remove outliers") and WASH2
 * (main.py:140-168, "remove either 3D points or observation"), per point and with t2 = thresh^2.
 * Observation i is an inlier of X when e_i = |uv_i - proj(cams[view_i], X)|^2 <= t2 (ordered
 * comparison: a NaN is never an inlier) and, if depth_sign != 0, the sign of the depth
 * c3.[X;1] equals depth_sign.
 *   1. every pair a < b of the track in two different views gives a hypothesis: the linear
 *      triangulation of the two observations (above); a non-positive or NaN pivot or a
 *      non-finite X makes it invalid.  Its score is (inliers over the whole track, sum of
 *      their e_i in track order).
 *   2. the winner is the valid hypothesis with >= 2 inliers that is best under the total order
 *      larger count, smaller sum, smaller pair ordinal (a-major, b-minor).  None: the point fails.
 *   3. twice: the Levenberg-Marquardt of rs_triangulate_nview over the current inlier set from
 *      the current X, then every e_i and the inlier set again.  Fewer than 2 inliers before a
 *      refit: the point fails.
 *   4. err2[i] is the final e_i (NaN for every observation of a failed point).  A point is kept
 *      when it did not fail, X is finite and it has >= min_views final inliers: point_keep[j]
 *      = 1, pts[j] = X and obs_keep[i] = 1 exactly for its final inliers.  Every other point
 *      keeps its input bits and all its observations get obs_keep = 0.
 * info: points_failed counts the failures, points_removed every point not kept, obs_removed
 * every obs_keep = 0.  A NaN in uv or in a camera is not an error.  RS_EINVAL: an index out of
 * range, nC < 1, n < 1, n > 2^24, thresh not finite or <= 0, min_views < 2, depth_sign outside
 * {-1, 0, 1}, a track longer than RS_WASH_MAX_TRACK.  The same inputs give bitwise the same
 * outputs (no floating-point atomics; every sum in track order). */
int rs_wash_points(rs_ctx *ctx, const double *cams, int64_t nC, double *pts, int64_t nP,
                   const int32_t *obs_view, const int32_t *obs_point, const double *uv, int64_t n,
                   double thresh, int32_t min_views, int32_t depth_sign,
                   int32_t *obs_keep, int32_t *point_keep, double *err2, rs_wash_info *info);

/* ------------------------------------------------------------------------------------------
 * The image front end (features.hip): the recipe of fun.py:130-151 that turns two images into
 * the (2, N) putative correspondences fun.getFFromLabCode consumes.  Images are row-major
 * (h, w); sides are at most RS_IMAGE_MAX_SIDE.  No floating-point atomics: the same inputs give
 * bitwise the same outputs.
 * ------------------------------------------------------------------------------------------ */
#define RS_IMAGE_MAX_SIDE 32768
#define RS_HARRIS_MAX_BLOCK 31         /* keeps the integer structure tensor below 2^53 */
#define RS_MATCH_MAX_ROI 15
#define RS_MATCH_MAX_N 32768           /* patches per image */
#define RS_MATCH_MAX_PAIRS (1LL << 28) /* n1 * n2 when the matrix is requested (2 GiB) */

/* lab3.harris (lab3.py:131-157) on a uint8 grey image, by the documented cornerHarris: Sobel
 * derivatives of aperture kernel_size (1: [-1 0 1] unsmoothed; 3: [1 2 1] x [-1 0 1]; 5, 7: the
 * binomial extensions), the unnormalised block_size x block_size box sum of Ix^2, IxIy, Iy^2
 * with its anchor at block_size / 2, reflect-101 borders for both steps, scale
 * s = 1 / (2^(kernel_size-1) block_size 255) on both derivatives, response
 * a c - b^2 - k (a + c)^2.  The tensor is summed in integers (exact) and the response is
 * evaluated once in fp64 and rounded to float: the result does not depend on the tiling.
 * raw == 0 sets negatives to zero (lab3.py:156).  RS_EINVAL: kernel_size not in {1, 3, 5, 7}
 * (the text of lab3.py:149), block_size outside 1..RS_HARRIS_MAX_BLOCK, k not finite, a side
 * above RS_IMAGE_MAX_SIDE or not above max(1, kernel_size / 2) + block_size. */
int rs_harris(rs_ctx *ctx, const uint8_t *image, int64_t h, int64_t w, int32_t block_size,
              int32_t kernel_size, double k, int32_t raw, float *out);

/* lab3.non_max_suppression (lab3.py:160-185) on a finite float image: a pixel keeps its value
 * when no pixel of its window_size^2 window is larger and it lies at least (window_size-1)/2
 * from every border; every other pixel becomes 0 * value, as the reference's False * value.
 * Bitwise the reference's result.  RS_EINVAL: an even window_size (the text of lab3.py:175). */
int rs_non_max_suppression(rs_ctx *ctx, const float *image, int64_t h, int64_t w,
                           int32_t window_size, float *out);

/* The corner list of fun.py:135-138: the positions with (double)H > rel * (double)max(H), in
 * row-major scan order (np.nonzero's).  xy has room for (2, cap): x (column) of hit k at xy[k],
 * y (row) at xy[cap + k]; *count is the number of hits.  A device max reduction, then an
 * order-preserving compaction (hits per chunk, scan, write at offset + rank).  H finite.
 * RS_EINVAL: rel not finite, more hits than cap (*count is still set). */
int rs_corners(rs_ctx *ctx, const float *H, int64_t h, int64_t w, double rel, int32_t *xy,
               int64_t cap, int64_t *count);

/* lab3.cut_out_rois (lab3.py:565-602) fused into fun.matchingMatrix (fun.py:113-120) and the
 * two argmins of lab3.joint_min (lab3.py:551-552).  xy1 is (2, n1) int32 -- x row, y row -- of
 * patch centres in img1, xy2 likewise; M[i, j] = |roi1_i - roi2_j|_F over the roi_size^2
 * patches.  row_min[i] = argmin_j M[i, j] with row_val[i] its value, col_min[j] = argmin_i
 * M[i, j]; ties go to the smallest index (np.argmin), whatever the block schedule.  M, (n1, n2)
 * row-major, is written when not null; the argmins never need it in memory.
 * uint8: the squared distance is an exact integer and M its correctly rounded root; wrap != 0
 * takes the differences modulo 256, as the reference's uint8 roi1[i] - roi2[j] does.
 * RS_EINVAL: roi_size even (the text of lab3.py:586) or above RS_MATCH_MAX_ROI, n1 or n2
 * outside 1..RS_MATCH_MAX_N, n1 * n2 > RS_MATCH_MAX_PAIRS with M requested, a centre nearer
 * than roi_size / 2 to a border. */
int rs_match_rois_u8(rs_ctx *ctx, const uint8_t *img1, int64_t h1, int64_t w1,
                     const int32_t *xy1, int64_t n1, const uint8_t *img2, int64_t h2, int64_t w2,
                     const int32_t *xy2, int64_t n2, int32_t roi_size, int32_t wrap,
                     int32_t *row_min, int32_t *col_min, double *row_val, double *M);

/* The same for float64 images: fp64 accumulation over the patch in raster order.  The input
 * must be finite (not checked here). */
int rs_match_rois_f64(rs_ctx *ctx, const double *img1, int64_t h1, int64_t w1,
                      const int32_t *xy1, int64_t n1, const double *img2, int64_t h2, int64_t w2,
                      const int32_t *xy2, int64_t n2, int32_t roi_size, int32_t *row_min,
                      int32_t *col_min, double *row_val, double *M);

/* HIP events before the first and after the last kernel of the next front-end calls (enable
 * != 0).  Returns the last timed call's device ms between its upload and its download, -1 when
 * none (tools/bench_features.py). */
int rs_features_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * The tracking stage (tracking.hip): a pyramidal Lucas-Kanade (KLT) tracker that follows
 * sub-pixel positions from one uint8 grey image into the next, the step that turns images into
 * the track array of imgdata/README images.txt (x1 y1 ... x36 y36 per scene point, -1 where
 * unseen) that correspondences.py serves from.  Every sum over a window is an exact integer, so
 * no result depends on how lanes split the window; every fp64 step below is evaluated in the
 * order written, each operation rounded once (no fused multiply-add).  The same inputs give
 * bitwise the same outputs, and a restatement of this text gives the same bits.
 *
 * Pyramid.  Level 0 is the image.  Level l + 1 has size ((h + 1) / 2, (w + 1) / 2) and at (y, x)
 *   the value (S + 128) >> 8, S the separable [1 4 6 4 1] x [1 4 6 4 1] integer sum of level l
 *   around (2 y, 2 x) over the reflect-101 continuation (gfedcb|abcdefgh|gfedcba).  Both sides
 *   of a level that is reduced must be at least 3.
 * Gradients.  (Gx, Gy) of a level is its aperture-3 integer Sobel pair, [1 2 1] x [-1 0 1] and
 *   its transpose, over the reflect-101 continuation: |G| <= 1020.
 * Sampling.  A position (qx, qy) in fp64 is inside a level of width w and height h for the
 *   half-window r when qx >= r && qx < w - 1 - r && qy >= r && qy < h - 1 - r; NaN and infinity
 *   are outside, and the test is made in fp64 before any conversion to an integer.  With
 *   ix = floor(qx), a = qx - ix, iy = floor(qy), b = qy - iy the weights are
 *     w00 = floor(((1 - a) (1 - b)) 16384 + 0.5),  w01 = floor((a (1 - b)) 16384 + 0.5),
 *     w10 = floor(((1 - a) b) 16384 + 0.5),        w11 = 16384 - w00 - w01 - w10
 *   and the sample of an integer image v at window offset (i, j), -r <= i, j <= r, is
 *     (w00 v[iy+i][ix+j] + w01 v[iy+i][ix+j+1] + w10 v[iy+i+1][ix+j] + w11 v[iy+i+1][ix+j+1]
 *      + 256) >> 9
 *   with an arithmetic shift (floor for negatives): five fractional bits.  A grey sample is at
 *   most 8160, a gradient sample at most 32640 in magnitude, and every window sum below stays
 *   under 2^41 for window <= 31: exact in int64 and exact when converted to fp64.
 * One feature.  Given p (fp64, level 0), a guess g (0 when none), window = 2 r + 1 with
 *   n = window^2 pixels, levels L, max_iter, eps, min_eig, from image A into image B:
 *     tau = (min_eig n) 65536          (65536 = (8 32)^2: the squared gain of a stored gradient
 *                                       sample over a unit grey slope)
 *     for l = L - 1 down to 0:
 *       p_l = p 2^-l
 *       p_l outside level l             ->  l = 0: LOST;  l > 0: g <- 2 g, next level
 *       T, Gx, Gy = samples of A's level l, and of its gradients, at p_l
 *       A = sum Gx Gx, B = sum Gx Gy, C = sum Gy Gy   (integers, then converted to fp64)
 *       det = A C - B B
 *       textured = A + C >= 2 tau  &&  (A - tau) (C - tau) - B B >= 0  &&  det > 0
 *       not textured                    ->  l = 0: FLAT;  l > 0: g <- 2 g, next level
 *       d = g;  at most max_iter times:
 *         q = p_l + d
 *         q outside level l             ->  l = 0: LOST;  l > 0: leave the loop, keeping d
 *         Jv = samples of B's level l at q
 *         bx = sum (T - Jv) Gx,  by = sum (T - Jv) Gy   (integers, then fp64)
 *         dx = (8 (C bx - B by)) / det,  dy = (8 (A by - B bx)) / det
 *         d <- d + (dx, dy);  at l = 0 one more is counted in iters
 *         leave the loop when dx dx + dy dy <= eps eps
 *       g <- 2 d for l > 0, g <- d for l = 0
 *     q = p + g;  q outside level 0     ->  LOST
 *     residual = (sum |T - Jv|) / (32 n), Jv sampled at q from B's level 0;  the result is q, OK
 *   iters is what the forward pass counted, whatever the status.
 * Forward-backward.  With fb_tol >= 0 every feature that reached OK is tracked back from its
 *   result, from image 1 into image 0, with the same parameters and no guess, on the pyramids
 *   already built.  fb is max(|xb - px|, |yb - py|) of the backward result when the backward
 *   pass is OK and -1 otherwise (also where it did not run).  A backward pass that is not OK, or
 *   fb > fb_tol, makes the status FB.
 * A status other than OK gives the position (-1, -1) and the residual -1.
 * ------------------------------------------------------------------------------------------ */
#define RS_KLT_OK 0
#define RS_KLT_LOST 1           /* left the image (or was never inside it) at level 0        */
#define RS_KLT_FLAT 2           /* the level-0 window failed the texture test                */
#define RS_KLT_FB 3             /* failed the forward-backward test                          */
#define RS_KLT_MAX_WINDOW 31    /* at most 16 window pixels per lane                         */
#define RS_KLT_MAX_LEVELS 8
#define RS_KLT_MAX_ITER 1024
#define RS_KLT_MAX_N (1LL << 22) /* features of one call                                     */

/* One pyramid step: out is ((h + 1) / 2, (w + 1) / 2) uint8.  RS_EINVAL: a side below 3 or above
 * RS_IMAGE_MAX_SIDE. */
int rs_pyr_down(rs_ctx *ctx, const uint8_t *image, int64_t h, int64_t w, uint8_t *out);

/* img0 and img1 are (h, w) uint8; pts is (2, n) -- x row, y row; guess is (2, n) or null.
 * Outputs: pos (2, n), status (n) RS_KLT_*, residual (n), iters (n), fb (n).  fb_tol < 0 switches
 * the forward-backward test off.  One launch follows every feature through all its levels.
 * RS_EINVAL before any launch: a null pointer, a side outside 1..RS_IMAGE_MAX_SIDE, window even
 * or outside 3..RS_KLT_MAX_WINDOW, levels outside 1..RS_KLT_MAX_LEVELS, a reduced level with a
 * side below 3, max_iter outside 1..RS_KLT_MAX_ITER, eps NaN or negative, min_eig not finite or
 * negative, fb_tol NaN, n negative or above RS_KLT_MAX_N.  n = 0 returns at once, without a
 * launch.  Points and guesses that are not finite are legal: such a feature is LOST. */
int rs_klt_track(rs_ctx *ctx, const uint8_t *img0, const uint8_t *img1, int64_t h, int64_t w,
                 const double *pts, const double *guess, int64_t n, int32_t window,
                 int32_t levels, int32_t max_iter, double eps, double min_eig, double fb_tol,
                 double *pos, int32_t *status, double *residual, int32_t *iters, double *fb);

/* HIP events between the stages of the next rs_klt_track calls (enable != 0).  Returns the last
 * timed call's device ms: slot 0 both pyramids, 1 the forward launch, 2 the backward launch (-1
 * when fb_tol < 0: there is no such launch); -1 where none (tools/bench_tracking.py). */
#define RS_TRACKING_TIMING_SLOTS 3
int rs_tracking_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * The point-cloud stage (cloud.hip): what main.py does last (main.py:175-176,
 * Tables.get3DPointsColorsAndNormals) and the surface normals 3Dvisualization.py attempts.
 * All fp64, one lane per point, no floating-point atomics: the same inputs give bitwise the
 * same outputs.
 * ------------------------------------------------------------------------------------------ */
#define RS_CLOUD_MAX_POINTS (1LL << 28)
#define RS_CLOUD_MAX_CELLS (1LL << 21) /* cells per axis: 21 bits each in a 63-bit key */

/* The arithmetic of tables.py:189-226.  cams is (nC, 3, 4) [R | t], pts (nP, 3).  The flat list
 * of m entries (entry_point[i], entry_obs[i]) names the observations each point averages over;
 * it is grouped by point with entry_point non-decreasing, and within a point it stands in the
 * order the caller wants summed (an observation may be listed more than once).  obs_view (nObs)
 * is the view of every observation, obs_color (nObs, 3) its colour as doubles.
 *   colors[j]  = (sum of the listed colours / entries of j) / 255
 *   normals[j] = (sum of centre(view) - pts[j]) / entries of j,  centre = -R^T t,
 * not normalised, exactly as the reference.  Both sums run in list order.  A point without an
 * entry gets NaN in both.  RS_EINVAL: an index out of range, entry_point decreasing, nC < 1
 * with m > 0, nP > RS_CLOUD_MAX_POINTS. */
int rs_cloud_attributes(rs_ctx *ctx, const double *cams, int64_t nC, const double *pts,
                        int64_t nP, const int32_t *entry_point, const int32_t *entry_obs,
                        int64_t m, const int32_t *obs_view, const double *obs_color, int64_t nObs,
                        double *colors, double *normals);

typedef struct rs_cloud_info {
  int64_t cells_occupied;    /* grid cells that hold a point                        */
  int64_t largest_cell;      /* points in the fullest cell                          */
  int64_t pairs_tested;      /* distance predicates evaluated                       */
  int64_t neighbours_found;  /* sum of count                                        */
  int64_t rows_not_ok;       /* points with count < 3 (non-finite points included)  */
} rs_cloud_info;             /* 40 bytes */

/* Surface normals from fixed-radius neighbourhoods (the plane fit of 3Dvisualization.py:16-31
 * and :96-113, by its mathematics: the reference's outer product and eigenvector pick are wrong
 * as written).  pts is (n, 3), radius finite and > 0, orient (n, 3) or null.
 *   N(i) = { j : |p_j - p_i|^2 <= radius^2 } evaluated in fp64 (i itself is a member; the last-
 *   bit rounding of the predicate -- FMA contraction -- is not specified), count[i] = |N(i)|.
 *   With d_j = p_j - p_i, s = sum d_j, S = sum d_j d_j^T, k = count[i]:
 *   M = S / k - (s / k)(s / k)^T, both sums over N(i) in ascending j.  That order is the
 *   reproducibility contract.
 *   evals[i] are the eigenvalues of M in ascending order (cyclic Jacobi), normals[i] the unit
 *   eigenvector of the smallest.  A row is ok iff k >= 3; rows that are not ok get NaN normals
 *   and NaN evals, their count is still valid.
 *   Sign: with orient given and orient[i] finite and non-zero, dot(normal, orient[i]) >= 0;
 *   otherwise the component of largest magnitude is positive (the first such on ties).
 *   A non-finite point has count 0, is not ok and is nobody's neighbour.
 * The search is a hash grid: integer cells of side radius (1 + 2^-20) from the minimum corner
 * `lo` of the finite points, 21 bits per axis, an open-addressed table of >= 2n slots, every
 * cell's points sorted by index, and per query a merge of its 27 cells in ascending index.
 * Memory is O(n) whatever the cloud's extent; RS_EINVAL when (p - lo) / radius reaches
 * RS_CLOUD_MAX_CELLS on any axis (the message states the limit), for a radius not finite or
 * <= 0 and for n > RS_CLOUD_MAX_POINTS.  The cost is O(n * 27 * points per cell): a cloud that
 * fits in one cell is O(n^2) by nature, and one lane sorts each cell, so this is not a tool
 * for radii that swallow the cloud.  Every loop is bounded: a hash probe that runs `capacity`
 * steps raises a flag that comes back as RS_EDEVICE.  n = 0 returns at once. */
int rs_cloud_normals(rs_ctx *ctx, const double *pts, int64_t n, double radius,
                     const double *orient, double *normals, int32_t *count, double *evals,
                     rs_cloud_info *info);

/* HIP events between the stages of the next point-cloud calls (enable != 0).  Returns the last
 * timed call's device ms per stage: grid (minimum corner, keys, hash insertion), scan, sort
 * (scatter and per-cell sort), normals (neighbour walk and eigen-solve), attributes
 * (rs_cloud_attributes' kernel); -1 where none (tools/bench_cloud.py). */
#define RS_CLOUD_TIMING_SLOTS 5
int rs_cloud_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* Exact k nearest neighbours on a uniform grid (cloud_knn.hip): what GetKNeighbours of
 * 3Dvisualization.py asks a kd-tree for (tree.query(points[None, j], k)), for every query at
 * once, and two consumers that keep the index lists on the device. */
#define RS_CLOUD_KNN_MAX_K 64
#define RS_CLOUD_KNN_MAX_CELLS (1LL << 24)

typedef struct rs_knn_info {
  int64_t cells;         /* cells of the grid                                   */
  int64_t largest_cell;  /* points in the fullest cell                          */
  int64_t tested;        /* candidates whose d2 was computed                    */
  int64_t found;         /* sum of count                                        */
  int64_t rows_short;    /* queries with count < k                              */
} rs_knn_info;           /* 40 bytes */

/* pts (n, 3); queries (m, 3), or null: the points themselves (then m must equal n).
 *   d2(q, j) = dx*dx + dy*dy + dz*dz with d = q - p_j: the differences first, the sum left to
 *   right, no product fused with a sum -- the bits of the same expression in numpy.
 *   The result of a query is the k smallest elements of { (bits of d2(q, j), j) } in
 *   lexicographic order, j over the finite points with d2(q, j) <= max_dist * max_dist
 *   (max_dist = +inf: all of them), written in that order to idx (m, k) and d2 (m, k).
 *   A point is a candidate for itself like any other.  count[i] is the number of entries found;
 *   the slots past it hold idx = -1 and d2 = +inf.  A non-finite point is nobody's neighbour, a
 *   non-finite query has count 0.
 * A minimum-k set under a total order does not depend on the order in which the candidates are
 * visited, so the result depends neither on the grid, nor on `cell`, nor on the arrival order of
 * an atomic.
 * The search is a dense uniform grid of side `cell` from the minimum corner `lo` of the finite
 * points, floor((hi - lo) / cell) + 1 cells per axis, every point registered in exactly one
 * cell; cell = 0 picks the largest extent / clamp(round(cbrt(number of finite points)), 1, 256)
 * (raised to 2^-24 of the box's largest coordinate magnitude; one cell where the extent is 0).
 * A query walks the Chebyshev rings r = r0, r0 + 1, ... around its own cell
 * floor((q - lo) / cell) (clamped to +-2^29), each clipped to the grid, and stops before ring
 * r >= 1 when its list is full and the k-th d2 <= B^2, B = (r - 1) cell (1 - 2^-20), when
 * B > max_dist, and after the last ring that meets the grid.
 * RS_EINVAL before any launch: k outside 1..RS_CLOUD_KNN_MAX_K, n or m negative or above
 * RS_CLOUD_MAX_POINTS, max_dist NaN or negative, cell negative or not finite, a null pointer
 * where elements are expected.  RS_EINVAL once the box is known (after the box reduction, before
 * any other kernel): a box whose extent hi - lo overflows to infinity on an axis, a grid of more
 * than RS_CLOUD_KNN_MAX_CELLS cells or a cell below 2^-24 of the box's largest coordinate
 * magnitude (the last two say "choose a larger cell").  n = 0 gives count = 0 everywhere; m = 0 returns without a
 * launch. */
int rs_cloud_knn(rs_ctx *ctx, const double *pts, int64_t n, const double *queries, int64_t m,
                 int32_t k, double max_dist, double cell, int32_t *idx, double *d2,
                 int32_t *count, rs_knn_info *info);

/* The plane fit of GetNormalOfPlaneFromPoints(points[NN_index]) (3Dvisualization.py:16-31), by
 * its mathematics, over every point's own k nearest (itself included, max_dist = +inf).  With
 * c = count[i], d_j = p_j - p_i, s = sum d_j, S = sum d_j d_j^T, both in list order:
 * M = S / c - (s / c)(s / c)^T; evals[i] its eigenvalues in ascending order (cyclic Jacobi),
 * normals[i] the unit eigenvector of the smallest, signed as rs_cloud_normals signs it.  A row
 * with c < 3 holds NaN in both.  Two calls give the same bits. */
int rs_cloud_knn_normals(rs_ctx *ctx, const double *pts, int64_t n, int32_t k, double cell,
                         const double *orient, double *normals, double *evals, int32_t *count,
                         rs_knn_info *info);

/* The mean distance to the k nearest other points, 1 <= k <= RS_CLOUD_KNN_MAX_K - 1.  Of the
 * list of the k + 1 nearest of point i the entry with index i is dropped if it is there (it is
 * not when more than k duplicates of p_i have lower indices), otherwise the last entry;
 * mean_dist[i] = (sum of sqrt(d2) over the remaining entries, in list order) / their number,
 * NaN where none remains and for a non-finite point.  count[i] is the length of the list before
 * the drop; info counts rows_short against k + 1. */
int rs_cloud_knn_mean_dist(rs_ctx *ctx, const double *pts, int64_t n, int32_t k, double cell,
                           double *mean_dist, int32_t *count, rs_knn_info *info);

/* HIP events between the stages of the next k-NN calls (enable != 0).  Returns the last timed
 * call's device ms per stage: box (min/max reduction), grid (cell counts), scan, scatter, query,
 * normals, mean_dist; -1 where none (tools/bench_knn.py). */
#define RS_CLOUD_KNN_TIMING_SLOTS 7
int rs_cloud_knn_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * The dense stage (dense.hip): plane-sweep depth maps and their fusion.  The reference project
 * stops at a sparse cloud; nothing here restates code of it.  No atomics, one fixed summation
 * order: the same inputs give bitwise the same outputs.
 * ------------------------------------------------------------------------------------------ */
#define RS_DENSE_MAX_SOURCES 8
#define RS_DENSE_MAX_PATCH 11
#define RS_DENSE_MAX_DEPTHS 4096
#define RS_DENSE_MAX_SIDE 16384
#define RS_DENSE_MAX_PIXELS (1LL << 26)
#define RS_DENSE_MAX_VOLUME (1LL << 28)
#define RS_DENSE_MAX_VIEWS 128

/* Plane sweep of one reference view against S source views.  Images are h x w uint8, row-major;
 * pixel (x, y) is column x, row y, centres at integers.  src holds the S source images one after
 * the other.  With P = K C = [M | m] per view, the caller passes per source s, row-major,
 *   A_s = M_s M_ref^-1 (3 x 3),  b_s = m_s - A_s m_ref (3),
 * and the D plane depths d_k (finite, nonzero, of one sign): plane k is c3_ref . [X; 1] = d_k,
 * fronto-parallel in the reference view.
 *   Warp.  Reference pixel p = (x, y, 1) maps to q = d_k (A_s p) + b_s, the source position is
 *   (x', y') = (q0 / q2, q1 / q2), all fp64.  The sample is valid when q2 d_k > 0,
 *   0 <= x' <= w - 1 and 0 <= y' <= h - 1.
 *   Sample.  x0 = floor(x'), y0 = floor(y'); fx = (float)(x' - x0), fy likewise; the right and
 *   lower neighbours are clamped to the last column and row.  With v = pixel - 128 (exact), in
 *   fp32: top = v00 + fx (v01 - v00), bottom = v10 + fx (v11 - v10),
 *   sample = top + fy (bottom - top).
 *   Score.  r = patch / 2, n = patch^2.  Over the n pixels of the window around (x, y), with
 *   a = reference pixel - 128 and b = the warped sample of that same pixel (each window pixel
 *   goes through the plane's warp itself):
 *     va = n sum a^2 - (sum a)^2   (exact integer),   vb = n sum b^2 - (sum b)^2,
 *     score = (n sum ab - sum a sum b) / sqrt(va vb),
 *   the b-sums in fp32 in raster order.  The sums are accumulated on the values shifted by 128
 *   (one pass, no second centring pass).  The score is valid when the window lies inside the
 *   image, all n samples are valid, va >= min_var n^2 (on the integers) and vb >= min_var n^2.
 *   The second test is made in fp32: vb as the fp32 expression above against
 *   (float)(min_var n^2).  Equality passes both tests.
 *   Cost.  cost(pixel, k) = the sum of the valid sources' scores in source order / their number
 *   nvalid; no valid source: the hypothesis is invalid (NaN in the volume).
 *   Winner.  index = the k of the largest cost, the smallest such k on ties; score its cost,
 *   nvalid its number of sources.  With c-, c0, c+ the costs at index - 1, index, index + 1:
 *   delta = clamp(0.5 (c- - c+) / (c- - 2 c0 + c+), -0.5, 0.5), and 0 when a neighbour is
 *   missing or invalid or the denominator is not negative.  The formula is evaluated in fp32 as
 *   written, (c- - 2 c0) + c+ with a rounding after each step: where c+ == c0 (a repeated depth)
 *   delta is 0.5 or, when c- - 2 c0 rounds, a few floats below it.  A pixel without a valid
 *   hypothesis gets index -1, delta 0, score NaN, nvalid 0.
 * index (h, w) int32, delta and score (h, w) float, nvalid (h, w) uint8; volume (D, h, w) float
 * is written when not null, and the other outputs do not depend on that.
 * RS_EINVAL before any launch: patch even or outside 3..RS_DENSE_MAX_PATCH, S outside
 * 1..RS_DENSE_MAX_SOURCES, D outside 1..RS_DENSE_MAX_DEPTHS, a side not above patch or above
 * RS_DENSE_MAX_SIDE, h w > RS_DENSE_MAX_PIXELS, D h w > RS_DENSE_MAX_VOLUME with a volume,
 * min_var not finite or <= 0, A or b not finite, a depth zero or not finite, depths of mixed
 * sign. */
int rs_dense_plane_sweep(rs_ctx *ctx, const uint8_t *ref, int64_t h, int64_t w,
                         const uint8_t *src, int32_t S, const double *A, const double *b,
                         const double *depths, int64_t D, int32_t patch, double min_var,
                         int32_t *index, float *delta, float *score, uint8_t *nvalid,
                         float *volume);

/* Cross-view agreement of V depth maps, depth (V, h, w) fp64 with NaN for "none".  P is
 * (V, 3, 4) = K C per view, [M | m]; Minv (V, 3, 3) the inverses of the M.  For view i and pixel
 * p = (x, y, 1) with finite depth d: X = Minv_i (d p - m_i).  For every other view j:
 * q = M_j X + m_j, d' = q2, (u, v) = (floor(q0 / q2 + 0.5), floor(q1 / q2 + 0.5)); when
 * 0 <= u <= w - 1 and 0 <= v <= h - 1, view j agrees if d_j = depth[j, v, u] is finite and
 * |d_j - d'| <= rel_tol |d'|.  count[i, y, x] is the number of agreeing views, 0 for a
 * non-finite depth.  All fp64, one lane per (i, pixel).  RS_EINVAL: V outside
 * 1..RS_DENSE_MAX_VIEWS, a side outside 1..RS_DENSE_MAX_SIDE, h w > RS_DENSE_MAX_PIXELS,
 * V h w > RS_DENSE_MAX_VOLUME, rel_tol not finite or negative, a camera not finite. */
int rs_dense_consistency(rs_ctx *ctx, const double *depth, int32_t V, int64_t h, int64_t w,
                         const double *P, const double *Minv, double rel_tol, uint8_t *count);

/* HIP events around the kernel of the next dense calls (enable != 0).  Returns the last timed
 * calls' device ms: slot 0 the plane sweep, slot 1 the consistency count; -1 where none
 * (tools/bench_dense.py). */
#define RS_DENSE_TIMING_SLOTS 2
int rs_dense_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* Semi-global aggregation of the plane-sweep volume (dense_sgm.hip): Hirschmueller's path
 * recursion over the (D, h, w) volume v of rs_dense_plane_sweep, then the winner of the summed
 * cost.  Everything is fp32 and every line below is one rounded operation; there is no
 * multiplication, so nothing can contract, and tests/dense_sgm_ref.py restates it bit for bit.
 *   1. Cost.  c(p, k) = 1.0f - v(p, k) where v is valid, 1.0f where v is NaN: an invalid
 *      hypothesis costs what an uncorrelated one does, and still passes messages.
 *   2. Directions r = (dx, dy), in this order: (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1)
 *      (-1,1).  paths is 4 (the first four) or 8.
 *   3. Path.  For direction r and pixel p with predecessor q = p - r: L_r(p, k) = c(p, k) when q
 *      is outside the image.  Otherwise, with m = min_k L_r(q, k),
 *        t = min(L_r(q, k), m + p2, L_r(q, k-1) + p1, L_r(q, k+1) + p1),
 *      the k-1 and k+1 terms only inside 0..D-1, and L_r(p, k) = (c(p, k) + t) - m.
 *   4. Sum.  S(p, k) = (((L_0 + L_1) + L_2) + ...) in direction order.
 *   5. Winner.  index(p) = the smallest k with minimal S among the valid hypotheses of p (v not
 *      NaN); -1 where p has none, which is the -1 set of rs_dense_plane_sweep.
 *   6. Offset.  With b = S(index - 1), a = S(index + 1), den = (b - 2 S(index)) + a:
 *      delta = clamp((0.5f (b - a)) / den, -0.5, 0.5) when both neighbours exist and are valid
 *      and den > 0, else 0.  The sign convention is that of rs_dense_plane_sweep's delta.
 *   7. Score.  score(p) = v(p, index), the winner's own ZNCC; NaN at index -1.
 * No atomics, one launch per direction in order: the same inputs give bitwise the same outputs.
 *
 * rs_dense_aggregate: volume (D, h, w) float on the host; index (h, w) int32, delta and score
 * (h, w) float; agg (D, h, w) float receives S when not null, and the other outputs do not depend
 * on that.  RS_EINVAL before any launch: a null pointer other than agg, D outside
 * 1..RS_DENSE_SGM_MAX_DEPTHS, a side outside 1..RS_DENSE_MAX_SIDE,
 * D h w > RS_DENSE_SGM_MAX_VOLUME (the volume, c and S live in scratch at once), paths not 4 or 8,
 * p1 or p2 not finite, or not 0 <= p1 <= p2. */
#define RS_DENSE_SGM_MAX_DEPTHS 256
#define RS_DENSE_SGM_MAX_VOLUME (1LL << 27)
int rs_dense_aggregate(rs_ctx *ctx, const float *volume, int64_t D, int64_t h, int64_t w,
                       float p1, float p2, int32_t paths, int32_t *index, float *delta,
                       float *score, float *agg);

/* rs_dense_plane_sweep followed by the aggregation above without a visit to the host: the sweep
 * kernel writes its volume to device scratch, the aggregation and the winner run on it there, and
 * only the four maps come down, plus volume and agg (both (D, h, w) float) when not null.  index,
 * delta and score are those of the aggregation; nvalid is the winner-takes-all winner's number of
 * sources, exactly as rs_dense_plane_sweep gives it (it is not the count of the aggregated
 * winner).  volume is bitwise that of rs_dense_plane_sweep.  RS_EINVAL before any launch: every
 * limit of rs_dense_plane_sweep and of rs_dense_aggregate (D <= RS_DENSE_SGM_MAX_DEPTHS and
 * D h w <= RS_DENSE_SGM_MAX_VOLUME whether or not a volume is asked for). */
int rs_dense_plane_sweep_sgm(rs_ctx *ctx, const uint8_t *ref, int64_t h, int64_t w,
                             const uint8_t *src, int32_t S, const double *A, const double *b,
                             const double *depths, int64_t D, int32_t patch, double min_var,
                             float p1, float p2, int32_t paths, int32_t *index, float *delta,
                             float *score, uint8_t *nvalid, float *volume, float *agg);

/* HIP events between the stages of the next aggregation calls (enable != 0).  Returns the last
 * timed calls' device ms: slot 0 the sweep kernel (rs_dense_plane_sweep_sgm only), slot 1 the
 * aggregation (cost, one launch per direction, S back to the volume's layout), slot 2 the
 * winner; -1 where none (tools/bench_dense_sgm.py).  rs_dense_timing does not see these calls. */
#define RS_DENSE_SGM_TIMING_SLOTS 3
int rs_dense_sgm_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * The surface stage (surface.hip): depth maps fused into a truncated signed distance volume and
 * a welded, consistently oriented triangle mesh extracted from it.  The reference project has no
 * such stage; nothing here restates code of it.  No atomics anywhere: the same inputs give
 * bitwise the same outputs, whatever the launch shape.
 *   Conventions are those of the dense stage: P = K C per view (3, 4) row-major, pixel centres
 * at integers, the depth of X in a view is its third projective coordinate, and depths may be
 * negative.  A volume is indexed [iz, iy, ix], x fastest; node (ix, iy, iz) lies at
 * X = origin + voxel (ix, iy, iz).
 * ------------------------------------------------------------------------------------------ */
#define RS_SURFACE_MAX_SIDE 2048
#define RS_SURFACE_MAX_NODES (1LL << 27)
#define RS_SURFACE_SCAN_CHUNK 2048 /* nodes one workgroup scans (the size boundaries of a test) */

/* TSDF fusion.  depth is (V, h, w) fp64 with NaN for "no depth", weights (V, h, w) float or null
 * (1 everywhere), P (V, 3, 4).  Per node, the views in index order, all fp64:
 *   q = P_v [X; 1], z = q2, u = floor(q0 / q2 + 0.5), v = floor(q1 / q2 + 0.5) (the rounding of
 *   rs_dense_consistency).  View v contributes when 0 <= u <= w - 1 and 0 <= v <= h - 1,
 *   d = depth[v, v, u] is finite, d z > 0, the weight sample wv is finite and > 0, and
 *   s = |d| - |z| >= -trunc.  It then adds wv min(1, s / trunc) to acc and wv to wsum.
 *   With the prior (T0, W0) of the node: W = W0 + wsum, T = (W0 T0 + acc) / W, NaN when W == 0;
 *   T0 is ignored when W0 is not > 0.  Both are stored as float.
 * tsdf and weight are (nz, ny, nx) float.  With has_prior != 0 they are read as the prior and
 * overwritten, so that a later call adds views to a volume that exists; with has_prior == 0 they
 * are only written.  A depth map is indexed only after the bounds test has passed.
 * RS_EINVAL before any launch: a side of the volume outside 1..RS_SURFACE_MAX_SIDE,
 * nx ny nz > RS_SURFACE_MAX_NODES, V outside 1..RS_DENSE_MAX_VIEWS, the image limits of
 * rs_dense_consistency, a camera, origin or voxel not finite, voxel <= 0, trunc not finite
 * or <= 0. */
int rs_surface_integrate(rs_ctx *ctx, const double *depth, const float *weights, int32_t V,
                         int64_t h, int64_t w, const double *P, const double *origin,
                         double voxel, int64_t nz, int64_t ny, int64_t nx, double trunc,
                         int32_t has_prior, float *tsdf, float *weight);

/* Marching tetrahedra on the Kuhn decomposition of every cell.  The 6 x 16 case table follows
 * from a three-line rule (csrc/surface_table.h holds it), and there are no ambiguous cases: the
 * mesh is watertight by construction.  What follows fixes every output bit, the positions
 * included: they are evaluated as written below, no product fused with a sum, which gives the
 * bits of the same expression in numpy.
 *   Negative node.  tsdf < 0; -0.0 and 0.0 are not negative.
 *   Valid cell.  All 8 nodes have weight >= min_weight and a finite tsdf.
 *   Tets.  Tet k (0..5) of a cell is the path 000 -> +e_a -> +e_b -> 111 with (a, b, c) the k-th
 *   permutation of (x, y, z) in lexicographic order; its corners are numbered 0..3 along the path.
 *   Edges.  Every tet edge joins a node o to o + e, e one of (dx, dy, dz) = (1,0,0), (0,1,0),
 *   (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1), its type 0..6 in that order; o owns the edge.
 *   The decomposition is translation-consistent, so neighbouring cells share these edges.
 *   Vertices.  One on an edge iff its two nodes differ in sign and at least one valid cell
 *   contains the edge.  They are numbered by owner in row-major node order, then by edge type.
 *   Position: origin + voxel (o + t e), t = fa / (fa - fb) in fp64 from the float values.  With
 *   fa == 0 the vertex lands on the node; such degenerate triangles are kept, so that the mesh
 *   stays combinatorially closed.
 *   Triangles.  Ordered by valid cell (row-major), then by tet, then by the table's order.  One
 *   corner of the other sign: one triangle on its three edges.  Two against two, n0, n1 the
 *   negative and p0, p1 the positive corners in path order: the quad (n0,p0), (n0,p1), (n1,p1),
 *   (n1,p0), split along (n0,p0)-(n1,p1).
 *   Winding.  The geometric normal points to the positive side.  It comes from the table, never
 *   from computed coordinates: an entry is derived once with every vertex at its edge midpoint
 *   and oriented against the vector from the negative corners' centroid to the positive ones'.
 * vertices is (vcap, 3) fp64 and faces (fcap, 3) int32, provided by the caller (either may be
 * null with capacity 0).  *nv and *nf are always set, to 0 on an argument error and otherwise to
 * the mesh's size.  RS_EINVAL, and no mesh written, when nv > vcap, nf > fcap, or nv or 3 nf
 * exceeds 2^31 - 1: a call with zero capacities learns the sizes, a second one with exact arrays
 * fetches the mesh.  Also RS_EINVAL: the volume limits of rs_surface_integrate, min_weight not
 * finite or <= 0, a negative capacity. */
int rs_surface_extract(rs_ctx *ctx, const float *tsdf, const float *weight, int64_t nz,
                       int64_t ny, int64_t nx, const double *origin, double voxel,
                       double min_weight, double *vertices, int64_t vcap, int32_t *faces,
                       int64_t fcap, int64_t *nv, int64_t *nf);

/* HIP events around the kernels of the next surface calls (enable != 0).  Returns the last timed
 * calls' device ms: slot 0 integrate, 1 classify (cells and nodes), 2 scan (both scans), 3 emit
 * (vertices and faces); -1 where none (tools/bench_surface.py). */
#define RS_SURFACE_TIMING_SLOTS 4
int rs_surface_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Surface from oriented points (cloud_knn.hip): the signed distance volume of a cloud with
 * normals, the step of Hoppe's "surface from unorganised points" that 3Dvisualization.py stops
 * before.  An implicit moving-least-squares field over the k nearest points within a radius; the
 * neighbour lists never leave the chip.  Nothing here restates code of the reference.
 *   Inputs.  pts and normals (n, 3) fp64, a support radius > 0, a neighbour cap k in
 *   1..RS_CLOUD_KNN_MAX_K.  A point is out when any of its six numbers is not finite: it is
 *   nobody's neighbour, as a non-finite point is in rs_cloud_knn.  Normals are used as given,
 *   not normalised.
 *   The list of a position X is the list rs_cloud_knn returns for the query X with
 *   max_dist = radius over the points that are not out: the c <= k smallest pairs (bits of d2, j)
 *   in lexicographic order, d2 = dx dx + dy dy + dz dz with d = X - p_j, the differences first,
 *   the sum left to right, d2 <= radius * radius.
 *   Per slot s of the list, in list order, all fp64, no product fused with a sum, every
 *   operation in exactly this order:
 *     u   = min(sqrt(d2_s) / radius, 1.0)
 *     a   = 1.0 - u;  a2 = a * a
 *     w   = (a2 * a2) * (4.0 * u + 1.0)                   Wendland C2, exactly 0 at the rim
 *     dot = dx * n_j[0] + dy * n_j[1] + dz * n_j[2]
 *     acc += w * dot;  sw += w;  with colours cacc[ch] += w * col_j[ch]
 *   f = acc / sw when sw > 0, otherwise NaN (c == 0, or every neighbour exactly on the rim);
 *   colour[ch] = cacc[ch] / sw under the same condition.  Only + - * /, sqrt and min in a fixed
 *   order: f is bit-equal to a numpy restatement that sums slot by slot (tests/points_ref.py).
 *   Like the lists, f depends neither on the grid nor on `cell`.
 *   Sign.  f > 0 on the side the normals point to, the convention of rs_surface_integrate
 *   (positive in front of the surface): rs_surface_extract's faces then face along the cloud's
 *   normals.
 * The grid is rs_cloud_knn's (the same kernels).  cell = 0 picks radius (1 + 2^-19), the smallest
 * cell for which the bound B > max_dist stops the walk after ring 1 (27 cells; at cell = radius
 * exactly B falls short of it by the factor 1 - 2^-20 and ring 2 is walked as well), raised to
 * 2^-24 of the box's largest coordinate magnitude and then by factors of 9/8 until the grid has at
 * most RS_CLOUD_KNN_MAX_CELLS cells.
 * ------------------------------------------------------------------------------------------ */
typedef struct rs_points_info {
  int64_t cells;         /* cells of the grid                                   */
  int64_t largest_cell;  /* points in the fullest cell                          */
  int64_t tested;        /* candidates whose d2 was computed                    */
  int64_t defined;       /* outputs with a finite value                         */
  int64_t saturated;     /* outputs whose list was full, c == k                 */
} rs_points_info;        /* 40 bytes */

/* The field on the nodes of a volume.  Node (ix, iy, iz) lies at origin + voxel (ix, iy, iz),
 * the expression of rs_surface_integrate with the product rounded before the sum (numpy's bits).
 * tsdf and weight are (nz, ny, nx) float, only written:
 *   tsdf   = (float) max(-1, min(1, f / trunc)), NaN where f is
 *   weight = (float) c, the neighbour count, exact since c <= 64.
 * rs_surface_extract(tsdf, weight, ..., min_weight = m) then reads min_weight as "at least m
 * points within radius of all 8 corners" (Hoppe's density test).
 * RS_EINVAL before any launch: a null pointer, k outside 1..RS_CLOUD_KNN_MAX_K, radius or trunc
 * not finite or <= 0, cell negative or not finite, n negative or above RS_CLOUD_MAX_POINTS, the
 * volume limits of rs_surface_integrate, origin or voxel not finite, voxel <= 0.  Once the box
 * is known: what rs_cloud_knn lists there.  n = 0 or no point that is not out: an all-NaN volume
 * with weight 0 and RS_OK. */
int rs_surface_points_volume(rs_ctx *ctx, const double *pts, const double *normals, int64_t n,
                             int32_t k, double radius, double trunc, double cell,
                             const double *origin, double voxel, int64_t nz, int64_t ny,
                             int64_t nx, float *tsdf, float *weight, rs_points_info *info);

/* The same field at m caller positions queries (m, 3): value[m] fp64 is the unclamped f,
 * count[m] int32 the neighbour count c.  With colors (n, 3) fp64 given, color (m, 3) =
 * cacc / sw, NaN where f is; colors and color are null together.  A non-finite query has count 0
 * and NaN.  RS_EINVAL as above, and for m negative or above RS_CLOUD_MAX_POINTS; m = 0 returns
 * without a launch. */
int rs_surface_points_eval(rs_ctx *ctx, const double *pts, const double *normals,
                           const double *colors, int64_t n, const double *queries, int64_t m,
                           int32_t k, double radius, double cell, double *value, int32_t *count,
                           double *color, rs_points_info *info);

/* HIP events between the stages of the next two calls above (enable != 0).  Returns the last
 * timed call's device ms per stage: box (the mask of the points that are out and the min/max
 * reduction), grid (cell counts), scan, scatter, field; -1 where none (tools/bench_points.py).
 * rs_cloud_knn_timing does not see these calls. */
#define RS_SURFACE_POINTS_TIMING_SLOTS 5
int rs_surface_points_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Colour for the mesh (surface_texture.hip): the mesh rendered into a z-buffer per view, and a
 * colour per vertex from the views that see it.  The reference project has no such code; nothing
 * here restates code of it.  Both entry points are bitwise reproducible from run to run: the only
 * atomics are a minimum, which commutes, and the counter of a list whose order cannot matter.
 *   Conventions are those above: P = K C per view (3, 4) row-major, pixel centres at integers,
 * images uint8, at most RS_DENSE_MAX_VIEWS views and the image limits of rs_dense_consistency.
 * Every camera is turned so that "in front" means a positive third coordinate: with
 * s_v = sign(det(P_v[:, :3])) the rules below read s_v P_v for P.  Negating a camera flips s_v
 * and so changes nothing at all: cameras with negative depths give the positive scene's result
 * bit for bit.
 * ------------------------------------------------------------------------------------------ */
/* A face whose clipped bounding box holds more pixels than this is drawn by a whole wave, lanes
 * across the box, and not by the lane that found it (the size boundaries of a test).  The value
 * is measured: DESIGN.md section 16. */
#ifndef RS_SURFACE_RASTER_SMALL
#define RS_SURFACE_RASTER_SMALL 32
#endif
/* Entries of the list of such faces, (face, view) pairs.  A face that finds the list full is
 * drawn by its own lane after all: slower, the same bits. */
#define RS_SURFACE_TEXTURE_LIST_CAP (1 << 20)

/* The z-buffers of a mesh: depth is (V, h, w) float, NaN where no face covers the pixel.
 * vertices is (nv, 3) fp64, faces (nf, 3) int32, P (V, 3, 4).  All arithmetic is fp64.
 *   Per view and face, with X_i the face's vertices: q_i = P [X_i; 1], z_i = q_i2.  The face is
 *   drawn iff all nine components of q are finite and all three z_i > 0: a face that crosses the
 *   camera plane is skipped, not clipped.  x_i = q_i0 / z_i, y_i = q_i1 / z_i,
 *   A = (x1 - x0)(y2 - y0) - (x2 - x0)(y1 - y0); the face is skipped when A is 0 or not finite.
 *   Both windings are drawn, there is no back-face culling: an open mesh occludes from both sides.
 *   Candidate pixels are the integer (px, py) in [ceil(min x), floor(max x)] x
 *   [ceil(min y), floor(max y)], intersected with the image.  With
 *     b0 = ((x2 - x1)(py - y1) - (y2 - y1)(px - x1)) / A,
 *     b1 = ((x0 - x2)(py - y2) - (y0 - y2)(px - x2)) / A,
 *     b2 = ((x1 - x0)(py - y0) - (y1 - y0)(px - x0)) / A,
 *   each from its own edge function, the pixel is covered iff b0, b1, b2 >= 0.  Its depth is
 *   perspective-correct, zeta = 1 / (b0 / z0 + b1 / z1 + b2 / z2), rounded once to float, and the
 *   pixel keeps the minimum over all the faces that cover it.
 * RS_EINVAL before any launch: nv or 3 nf outside 0..2^31 - 1, a face index outside 0..nv - 1,
 * V outside 1..RS_DENSE_MAX_VIEWS, the image limits of rs_dense_consistency, a camera that is not
 * finite or whose det(P[:, :3]) is zero or not finite. */
int rs_surface_render_depth(rs_ctx *ctx, const double *vertices, int64_t nv,
                            const int32_t *faces, int64_t nf, const double *P, int32_t V,
                            int64_t h, int64_t w, float *depth);

/* A colour per vertex.  The z-buffers are rendered as above and stay in device memory; images is
 * (V, h, w, channels) uint8 with channels 1 or 3, normals (nv, 3) fp64 or null.  Per vertex X,
 * the views in index order, all fp64:
 *   q = P_v [X; 1], z = q2; the view is skipped unless q is finite and z > 0.  u = q0 / z,
 *   v = q1 / z; the vertex is inside iff 0 <= u <= w - 1 and 0 <= v <= h - 1.  x0 = floor(u),
 *   y0 = floor(v), x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1): the footprint of the dense
 *   stage's bilinear rule.  far is the largest finite z-buffer value among the footprint's four
 *   pixels; without one the vertex is not visible, and otherwise it is visible iff
 *   z <= far (1 + rel_tol).  With normals, g = (n . (c_v - X)) / |c_v - X| with the camera centre
 *   c_v = -M_v^-1 p_v, P_v = [M_v | p_v]; the view contributes iff g > min_cos, with weight g.
 *   Without normals the weight g is 1 and min_cos is not read.  Per channel, with fx = u - x0 and
 *   fy = v - y0: top = I[y0, x0] + fx (I[y0, x1] - I[y0, x0]), bot likewise on row y1,
 *   s = top + fy (bot - top); acc += g s, wsum += g, count += 1.
 * colors is (nv, channels) fp64, acc / (255 wsum), and 0 where count, (nv) int32, is 0.  depth is
 * null or (V, h, w) float and then receives the z-buffers of rs_surface_render_depth.
 * RS_EINVAL before any launch: what rs_surface_render_depth lists, channels not 1 or 3, rel_tol
 * not finite or negative, min_cos not finite. */
int rs_surface_colorize(rs_ctx *ctx, const double *vertices, int64_t nv, const int32_t *faces,
                        int64_t nf, const uint8_t *images, int32_t channels, const double *P,
                        int32_t V, int64_t h, int64_t w, const double *normals, double rel_tol,
                        double min_cos, double *colors, int32_t *count, float *depth);

/* HIP events around the kernels of the next two calls above (enable != 0).  Returns the last
 * timed calls' device ms: slot 0 raster_small (the fill and the lane-per-face kernel), 1
 * raster_large (the wave-per-face kernel and +inf to NaN), 2 gather (rs_surface_colorize only);
 * -1 where none (tools/bench_texture.py).  rs_surface_timing does not see these calls. */
#define RS_SURFACE_TEXTURE_TIMING_SLOTS 3
int rs_surface_texture_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * The evaluation stage (eval.hip): the exact distance from many points to a triangle mesh, the
 * operation under the accuracy and completeness measures of tsbb15_amd.evaluation.  The
 * reference's evaluation.py loads the true cameras and stops; nothing here restates code of it.
 * All fp64, one lane per query, integer atomics only.  The result of a query is a minimum over
 * the pair (bits of d2, face index), which no visiting order can change: it depends neither on
 * the grid, nor on `cell`, nor on the arrival order of an atomic, and two calls give the same
 * bits.
 * ------------------------------------------------------------------------------------------ */
#define RS_EVAL_MAX_POINTS (1LL << 28)  /* queries of one call                               */
#define RS_EVAL_MAX_CELLS (1LL << 24)   /* cells of the grid, all three axes multiplied       */
#define RS_EVAL_MAX_ENTRIES (1LL << 27) /* face-cell registrations                            */

typedef struct rs_eval_info {
  int64_t cells[3];       /* grid dimensions along x, y, z                                  */
  int64_t entries;        /* face-cell registrations                                        */
  int64_t largest_cell;   /* registrations in the fullest cell                              */
  int64_t tests;          /* point-triangle tests run                                       */
  int64_t faces_skipped;  /* invalid faces                                                  */
  int64_t beyond;         /* queries answered +inf                                          */
} rs_eval_info;           /* 64 bytes */

/* pts is (n, 3), vertices (nv, 3), faces (nf, 3) int32; max_dist > 0 (+inf allowed), cell > 0
 * and finite.  d2 is (n), face (n) int32, closest (n, 3).
 *   A face (a, b, c) is invalid, skipped and counted in info.faces_skipped, when one of its nine
 *   coordinates is not finite or when, with ab = b - a and ac = c - a, the three components
 *   ab1 ac2 - ab2 ac1, ab2 ac0 - ab0 ac2, ab0 ac1 - ab1 ac0 are all exactly zero (no area; a
 *   repeated index).
 *   The closest point of a valid face to p is Ericson's ClosestPtPointTriangle, by Voronoi region
 *   of the triangle, the vertices first, then the edges, then the interior.  No product is fused
 *   with a sum, every dot product is x x' + y y' + z z' summed left to right, and the first rule
 *   that holds decides:
 *     ab = b - a, ac = c - a, ap = p - a, d1 = ab.ap, d2 = ac.ap
 *     bp = p - b, d3 = ab.bp, d4 = ac.bp;  cp = p - c, d5 = ab.cp, d6 = ac.cp
 *     d1 <= 0 and d2 <= 0                       ->  q = a
 *     d3 >= 0 and d4 <= d3                      ->  q = b
 *     d6 >= 0 and d5 <= d6                      ->  q = c
 *     vc = d1 d4 - d3 d2;  vc <= 0, d1 >= 0, d3 <= 0
 *                                               ->  q = a + (d1 / (d1 - d3)) ab
 *     vb = d5 d2 - d1 d6;  vb <= 0, d2 >= 0, d6 <= 0
 *                                               ->  q = a + (d2 / (d2 - d6)) ac
 *     va = d3 d6 - d5 d4;  va <= 0, d4 - d3 >= 0, d5 - d6 >= 0
 *                                               ->  q = b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) (c - b)
 *     otherwise, s = (va + vb) + vc             ->  q = (a + (vb / s) ab) + (vc / s) ac
 *   q = x + t u stands for x_k + t u_k per coordinate.  The face's squared distance is
 *   e.e with e = p - q.  A face whose squared distance is NaN (possible only where a sliver's
 *   s rounds to zero, or on overflow) never wins.
 *   d2[i] is the minimum over the valid faces, face[i] the lowest index among the faces whose
 *   squared distance is bit-equal to it, closest[i] that face's q.  When no face wins, or when
 *   d2[i] > max_dist max_dist (the fp64 product): d2 = +inf, face = -1, closest = NaN; such
 *   queries are counted in info.beyond.  A query with a coordinate that is not finite gets
 *   d2 = NaN, face = -1, closest = NaN.  nf = 0 or no valid face: every finite query gets +inf.
 * The search is a dense uniform grid of side `cell` from the minimum corner `lo` of the box of
 * the faces with finite coordinates: floor((hi - lo) / cell) + 1 cells per axis.  A valid face
 * is registered in every cell its own box overlaps (count with an integer atomicAdd per cell,
 * exclusive scan, scatter through an integer atomic cursor; the order inside a cell is the
 * arrival order and cannot matter).  A query takes its integer cell coordinate
 * floor((p - lo) / cell), which may lie outside the grid, and walks the Chebyshev rings r = r0,
 * r0 + 1, ... around it, each clipped to the grid, r0 the first that meets the grid.  Before
 * ring r >= 1 it stops when the best squared distance is <= B^2, B = (r - 1) cell (1 - 2^-20),
 * or when B > max_dist: a face not yet seen is registered only in cells of ring >= r, so its box
 * and the face lie at least (r - 1) cell away; the factor covers the rounding of the cell
 * coordinates.  It also stops when the ring has left the grid on every side.  `tests` counts a
 * face once per cell in which a query meets it.
 * RS_EINVAL before any launch: n, nv or nf negative, n > RS_EVAL_MAX_POINTS, nv or 3 nf above
 * 2^31 - 1, a face index outside 0..nv - 1, max_dist not > 0, cell not finite or not > 0, a box
 * whose extent is not finite, cell < 2^-24 of the box's largest coordinate magnitude (the ring
 * bound needs the squared distances accurate to 2^-20), more than RS_EVAL_MAX_CELLS cells or
 * more than RS_EVAL_MAX_ENTRIES registrations (the message names the cap and says "choose a
 * larger cell").  n = 0 returns at once. */
int rs_eval_mesh_distance(rs_ctx *ctx, const double *pts, int64_t n, const double *vertices,
                          int64_t nv, const int32_t *faces, int64_t nf, double max_dist,
                          double cell, double *d2, int32_t *face, double *closest,
                          rs_eval_info *info);

/* HIP events between the stages of the next rs_eval_mesh_distance calls (enable != 0).  Returns
 * the last timed call's device ms: slot 0 bin (validity, triangle packing, count per cell), 1
 * scan, 2 scatter, 3 query; -1 where none (tools/bench_eval.py). */
#define RS_EVAL_TIMING_SLOTS 4
int rs_eval_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Registration (eval.hip): a target mesh and its grid kept on the device (rs_eval_index), queried
 * many times, and one step of trimmed ICP of a source cloud against it, wholly on the device.
 * tsbb15_amd.evaluation.register drives the steps; tests/register_ref.py restates a step in numpy.
 * The index owns its device memory; it uses the stream of the context it was created with and
 * must be destroyed before that context.  One index serves one caller at a time.
 * ------------------------------------------------------------------------------------------ */
typedef struct rs_eval_index rs_eval_index;

/* The grid of rs_eval_mesh_distance for (vertices, faces, cell), built once: the same checks, caps
 * and messages (all but those about the queries), the same bin, scan and scatter kernels, the
 * same cross-check of the host's and the device's entries and skipped faces.  info receives
 * cells, entries, largest_cell and faces_skipped; tests and beyond are 0.  *out is null on an
 * error. */
int rs_eval_index_create(rs_ctx *ctx, const double *vertices, int64_t nv, const int32_t *faces,
                         int64_t nf, double cell, rs_eval_index **out, rs_eval_info *info);
int rs_eval_index_destroy(rs_eval_index *index);   /* null is allowed */

/* rs_eval_mesh_distance's query (the same kernel) against the index: d2, face and closest are
 * bit-equal to that call's on the same mesh, points, max_dist and cell, and so is info.  n = 0
 * returns at once with info as create gave it.  RS_EINVAL: n < 0 or > RS_EVAL_MAX_POINTS,
 * max_dist not > 0, a null pointer. */
int rs_eval_index_query(rs_eval_index *index, const double *pts, int64_t n, double max_dist,
                        double *d2, int32_t *face, double *closest, rs_eval_info *info);

/* The source cloud of the steps that follow, pts (n, 3), uploaded once; 1 <= n <=
 * RS_EVAL_MAX_POINTS.  It replaces an earlier cloud and forgets the last step. */
int rs_eval_index_set_points(rs_eval_index *index, const double *pts, int64_t n);

#define RS_EVAL_REG_POINT 0
#define RS_EVAL_REG_PLANE 1
#define RS_EVAL_REG_SLOTS 40
#define RS_EVAL_REG_BLOCK 2048   /* source indices per block of the moments' sum */

typedef struct rs_eval_step {
  int64_t matched;   /* m: points with face >= 0                                             */
  int64_t kept;      /* points with face >= 0 and d2 <= tau                                  */
  int64_t k;         /* the rank tau was taken at; 0 when m = 0                              */
  int64_t tests;     /* point-triangle tests of this step's query                            */
  double tau;        /* the k-th smallest d2 among the matched; NaN when m = 0               */
  double moments[RS_EVAL_REG_SLOTS];   /* see below; the slots a metric does not use are 0  */
} rs_eval_step;      /* 360 bytes */

/* One step under the similarity T = (s, R row-major, t), 13 doubles, about `origin`.  All fp64,
 * no product fused with a sum, every sum left to right as written.
 *   Transform.  p'_0 = s ((R00 x + R01 y) + R02 z) + t0, rows 1 and 2 likewise.  A point with a
 *     coordinate that is not finite stays not finite.
 *   Query.  rs_eval_mesh_distance's query of p' with max_dist: d2, face, closest.  A point is
 *     matched when face >= 0; m is their number.  A matched d2 is finite and not negative.
 *   Trim.  k = ceil(keep m - 1e-9) (one product, one difference, one ceil), clamped to 1..m.  tau
 *     is the k-th smallest d2 among the matched points, found exactly: a finite double that is not
 *     negative orders as its 64-bit pattern, and eight passes, from the highest byte down, each
 *     count the matched points whose higher bytes equal the prefix found so far in 256 bins of
 *     that byte (one table per workgroup in LDS, merged with integer atomics) and pick the bin
 *     that holds rank k.  A point is kept when it is matched and d2 <= tau: ties at tau are all
 *     kept, kept >= k.  m = 0: kept = k = 0, tau = NaN, every moment 0, RS_OK.
 *   Moments.  x = p' - origin, y = closest - origin, e = p' - closest, per kept point.
 *     RS_EVAL_REG_POINT, 17 slots: 0..2 sum x; 3..5 sum y; 6 + 3 i + j sum y_i x_j; 15 sum
 *     (x0 x0 + x1 x1) + x2 x2; 16 sum d2.
 *     RS_EVAL_REG_PLANE, 37 slots.  (a, b, c) is the matched face, u = b - a, v = c - a,
 *     N = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), l = sqrt((N0 N0 + N1 N1) + N2 N2),
 *     n = N / l per component, r = (n0 e0 + n1 e1) + n2 e2, and the row
 *     J = (x1 n2 - x2 n1, x2 n0 - x0 n2, x0 n1 - x1 n0, n0, n1, n2, (x0 n0 + x1 n1) + x2 n2).
 *     Slots 0..27 sum J_i J_j for i <= j, row after row (00, 01, .., 06, 11, 12, ..); 28..34 sum
 *     J_i r; 35 sum r r; 36 sum d2.  Both signs of n give the same terms.
 *   Order of a sum.  Source index i belongs to block i / RS_EVAL_REG_BLOCK and, inside it, to lane
 *     (i mod RS_EVAL_REG_BLOCK) mod 256.  A lane starts at +0.0 and adds its terms in ascending
 *     index; a point that is not kept, or an index >= n, adds +0.0.  The 256 lane sums fold by
 *     halving: lane l takes l + (l + h) for h = 128, 64, .., 1; lane 0 holds the block's partial.
 *     The total starts at +0.0 and adds the partials in ascending block order.  Nothing in it
 *     depends on the grid, on cell, on an atomic's arrival or on scheduling; there is no
 *     floating-point atomic anywhere.
 * The 16 doubles travel as kernel arguments; the step downloads the record, once, after its one
 * synchronisation.  RS_EINVAL: no source cloud, T or origin not finite, keep outside (0, 1],
 * max_dist not > 0, an unknown metric, a null pointer. */
int rs_eval_index_step(rs_eval_index *index, const double T[13], const double origin[3],
                       double keep, double max_dist, int32_t metric, rs_eval_step *out);

/* The last step's arrays: d2 (n), face (n) int32, closest (n, 3), kept (n) uint8, 1 where kept;
 * a null pointer skips an array.  RS_EINVAL when no step has run since set_points. */
int rs_eval_index_read(rs_eval_index *index, double *d2, int32_t *face, double *closest,
                       uint8_t *kept);

/* HIP events between the stages of the index's next steps (enable != 0).  Returns the last timed
 * step's device ms: slot 0 transform, 1 query, 2 select (16 launches), 3 moments (the blocks'
 * partials and their sum); -1 where none (tools/bench_register.py). */
#define RS_EVAL_REG_TIMING_SLOTS 4
int rs_eval_index_timing(rs_eval_index *index, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Mesh clean-up (mesh.hip): connected components, compaction and Taubin smoothing of the welded
 * index mesh rs_surface_extract returns.  The reference project has no such code; nothing here
 * restates code of it.  vertices is (nv, 3) fp64, faces (nf, 3) int32 with indices in 0..nv - 1.
 * Every result below is unique: integer atomics (a minimum, a sum, a cursor whose order a sort
 * removes) and fp64 sums in a stated order, so two calls give the same bits and
 * tests/mesh_ref.py restates them to the bit.
 *   RS_EINVAL before any launch, for all three calls: nv or nf negative or above the limits, a
 * face index outside 0..nv - 1, a null pointer with a non-zero size.  nv = 0 and nf = 0 are valid.
 * ------------------------------------------------------------------------------------------ */
#define RS_MESH_MAX_VERTICES (1LL << 27)
#define RS_MESH_MAX_FACES (1LL << 27)   /* so that the 6 nf adjacency entries fit an int32 */
#define RS_MESH_MAX_ROUNDS 64           /* hook rounds of rs_mesh_components                */
#define RS_MESH_MAX_ITERATIONS 65536    /* of rs_mesh_smooth                                */
#define RS_MESH_SCAN_CHUNK 2048 /* items one workgroup scans, the chunk of the surface stage's
                                   scans (the size boundaries of a test) */

/* Connected components over shared vertex indices: two vertices are connected when a face names
 * both.  A face may repeat an index.
 *   label (nv) int32: the smallest vertex index of the vertex's component; a vertex in no face
 *   labels itself.  size (nv) int32: the number of faces of the vertex's component, 0 for a
 *   vertex in no face.  *count: the number of components, the vertices in no face included (the
 *   v with label[v] == v).  *rounds: the hook rounds the call ran, the last, which found nothing
 *   to do, included; 0 when nf == 0.
 * Method: union-find.  parent[v] <= v holds at every moment, so a walk to a root strictly
 * decreases and ends.  A round hooks, per face and for two of its edges, the larger of the two
 * ends' roots under the smaller with an atomic minimum, and the next round first shortens every
 * path to its root by pointer jumping.  No kernel waits for another lane or workgroup; the host
 * launches rounds until one hooks nothing.  Every root that has a neighbour of a smaller root is
 * hooked in a round, whatever the diameter: a strip of 100 000 triangles takes 2 rounds numbered
 * along the strip and 11 numbered at random.  RS_EDEVICE, with a message,
 * when RS_MESH_MAX_ROUNDS rounds did not suffice. */
int rs_mesh_components(rs_ctx *ctx, const int32_t *faces, int64_t nf, int64_t nv, int32_t *label,
                       int32_t *size, int64_t *count, int32_t *rounds);

/* Drop vertices and renumber.  keep is (nv) uint8, non-zero: keep.  The kept vertices follow in
 * their original order, their bits copied (they are not examined: a non-finite vertex passes);
 * the faces all three of whose vertices are kept follow in their original order with the new
 * indices; vmap (nv) int32, or null, receives the new index of a vertex or -1.
 *   vertices_out is (vcap, 3) and faces_out (fcap, 3), provided by the caller (either may be null
 * with capacity 0).  *nv_out and *nf_out are always set, to 0 on an argument error and otherwise
 * to the sizes of the result.  RS_EINVAL, and nothing written, vmap included, when a capacity is
 * too small: a call with zero capacities learns the sizes, a second with exact arrays fetches the
 * result (the ABI of rs_surface_extract).  Also RS_EINVAL: a negative capacity.  The offsets are
 * exclusive scans over chunks of RS_MESH_SCAN_CHUNK. */
int rs_mesh_compact(rs_ctx *ctx, const double *vertices, int64_t nv, const int32_t *faces,
                    int64_t nf, const uint8_t *keep, double *vertices_out, int64_t vcap,
                    int32_t *faces_out, int64_t fcap, int32_t *vmap, int64_t *nv_out,
                    int64_t *nf_out);

/* Taubin's lambda|mu smoothing with uniform weights.  out is (nv, 3) fp64.
 *   Row.  The row of v holds, for every face corner that names v, the face's other two indices;
 *   entries equal to v itself (a face that repeats an index) are dropped.  N(v) is the set of the
 *   row's distinct entries: the vertices other than v that share a face with v.
 *   Boundary.  v is a boundary vertex when some u occurs exactly once in its row.  For faces
 *   without repeated indices that is: v shares exactly one face with u, (u, v) is a boundary edge.
 *   Fixed.  v is fixed when fixed (nv, uint8, or null) is non-zero at v, or when pin_boundary != 0
 *   and v is a boundary vertex.
 *   Pass with factor f, all fp64, no product fused with a sum, per coordinate:
 *     s = the sum of x_u over N(v) in ascending order of u, from the first term, left to right;
 *     x'_v = x_v + f (s / |N(v)| - x_v).
 *   A fixed vertex and a vertex with empty N(v) keep their bits.
 *   One iteration is a pass with lambda, then a pass with mu, each reading the positions the
 *   pass before it wrote.  iterations == 0 returns the input bits.
 * The rows are built once per call: count, exclusive scan, scatter through an integer cursor,
 * then each row is sorted and its duplicates removed in place, which removes the cursor's order.
 * Any degree works.  Also RS_EINVAL: a vertex coordinate, lambda or mu not finite, iterations
 * outside 0..RS_MESH_MAX_ITERATIONS. */
int rs_mesh_smooth(rs_ctx *ctx, const double *vertices, int64_t nv, const int32_t *faces,
                   int64_t nf, int32_t iterations, double lambda, double mu, const uint8_t *fixed,
                   int32_t pin_boundary, double *out);

/* HIP events around the kernels of the next three calls above (enable != 0).  Returns the last
 * timed calls' device ms: slot 0 components (all rounds and the sizes), 1 compact (flags, scans
 * and emit), 2 adjacency (rs_mesh_smooth's rows), 3 smooth (its passes); -1 where none
 * (tools/bench_mesh.py). */
#define RS_MESH_TIMING_SLOTS 4
int rs_mesh_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification (simplify.hip): vertex clustering on a uniform grid, the representative of
 * a cell placed by the cell's accumulated error quadric (Lindstrom 2000).  The reference project
 * has no such code; nothing here restates code of it.  The mesh is the index mesh of the calls
 * above, with their limits.  Everything is fp64 in plain IEEE operations, no product fused with
 * a sum, and every sum has a stated order, so two calls give the same bits and
 * tests/simplify_ref.py restates them to the bit; it is also where the order of the operations
 * of step 5 is written out.
 *   1 Cells.  i_a = floor((x_a - origin_a) / cell) per axis a, compared as a double; every i_a
 *     must lie in 0..dims_a - 1.  key = (i_2 dims_1 + i_1) dims_0 + i_0.  A vertex on a cell face
 *     belongs to the upper cell.
 *   2 Clusters.  A cell that holds a vertex, named by a face or not, is a cluster; clusters are
 *     numbered in ascending key order.  vmap[v] is the cluster of v.
 *   3 Mean.  m = the sum of the cluster's vertices in ascending vertex index, from the first
 *     term, left to right, divided by their number.
 *   4 Quadric.  Face f = (a, b, c) has n = (x_b - x_a) x (x_c - x_a), not normalised, and
 *     d = -(n . x_a).  It contributes once to every distinct cluster among its three corners,
 *     whatever becomes of it in step 6.  A cluster's ten numbers, in this order, are
 *     n0 n0, n0 n1, n0 n2, n1 n1, n1 n2, n2 n2 (A), n0 d, n1 d, n2 d (b) and d d, each summed
 *     over its faces in ascending face index from the first term; all 0 without a face.
 *   5 Position.  x = m for placement 0.  For placement 1 A is diagonalised by cyclic Jacobi
 *     (at most 30 sweeps; eigenvalues l_i on the diagonal, eigenvectors v_i in columns 0, 1, 2
 *     as the sweeps leave them), L = max l_i.  Unless L > 0, x = m.  Otherwise
 *     r = (-b) - A m and x = m + sum g_i v_i over the i with l_i > rank_tol L, in the order
 *     i = 0, 1, 2, g_i = (v_i . r) / l_i.  x is accepted when its coordinates are finite and
 *     floor((x_a - origin_a) / cell) is the cell's i_a on every axis; otherwise x = m and the
 *     cluster is a fall-back.
 *   6 Faces.  The corners go through vmap.  A face with two equal clusters is degenerate and
 *     dropped.  Of the remaining faces with the same set of three clusters, in any rotation and
 *     either orientation, the one of lowest index stays.  The survivors keep their order and
 *     their corner order.  fmap[f] is the output index, -1 (degenerate) or -2 (duplicate).
 * Clusters that no surviving face names are kept.
 *   vertices_out is (v_cap, 3) and faces_out (f_cap, 3), the capacity protocol of
 * rs_mesh_compact: *nv_out and *nf_out are always set, to 0 on an argument error; RS_EINVAL and
 * no output byte written (vmap, fmap, quadrics_out and info included) when a capacity is too
 * small.  vmap is (nv) and fmap (nf) int32; quadrics_out (clusters, 10) fp64 within v_cap rows,
 * or null.  nv = 0 and nf = 0 are valid.
 *   RS_EINVAL before any launch, nothing written: what the mesh calls above list, a vertex
 * coordinate or origin not finite, cell not finite or not positive, a dim below 1, more than
 * RS_SIMPLIFY_MAX_CELLS cells, placement outside 0..1, rank_tol outside [0, 1) or NaN, a vertex
 * outside the grid, a negative capacity or a null array of non-zero capacity.
 *   Method: three times "items grouped by bucket, each bucket ascending" -- vertices by cluster,
 * face corners by cluster, faces by their smallest cluster -- each as count, exclusive scan,
 * scatter through an integer cursor and a sort of each row in place by one lane, which removes
 * the cursor's order.  Atomics are integer only; no kernel waits for another lane. */
#define RS_SIMPLIFY_MAX_CELLS (1LL << 27)
#define RS_SIMPLIFY_MEAN 0
#define RS_SIMPLIFY_QUADRIC 1

typedef struct rs_simplify_info {
  int64_t clusters;         /* = *nv_out                                                    */
  int64_t fallbacks;        /* clusters whose quadric position was rejected in step 5       */
  int64_t degenerate_faces; /* fmap == -1                                                   */
  int64_t duplicate_faces;  /* fmap == -2                                                   */
  int64_t longest_row;      /* the most items one lane sorted: vertices of a cluster, face
                               corners of a cluster, or faces that share a smallest cluster */
} rs_simplify_info;

int rs_mesh_simplify(rs_ctx *ctx, const double *vertices, int64_t nv, const int32_t *faces,
                     int64_t nf, const double *origin, double cell, const int64_t *dims,
                     int32_t placement, double rank_tol, double *vertices_out, int64_t v_cap,
                     int32_t *faces_out, int64_t f_cap, int32_t *vmap, int32_t *fmap,
                     double *quadrics_out, int64_t *nv_out, int64_t *nf_out,
                     rs_simplify_info *info);

/* HIP events between the stages of the next rs_mesh_simplify calls (enable != 0).  Returns the
 * last timed call's device ms: slot 0 cluster (keys, occupancy scan, vmap), 1 rows (the vertex
 * and corner rows and the means), 2 quadric (sums and solve), 3 faces (classification, the
 * duplicate rows, scan and emit); -1 where none (tools/bench_simplify.py).  rs_mesh_timing does
 * not see these calls. */
#define RS_SIMPLIFY_TIMING_SLOTS 4
int rs_simplify_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Global registration (global_reg.hip): descriptors, descriptor matching and a RANSAC over
 * three-point similarities, the coarse alignment that lands inside the basin of the trimmed ICP
 * above from any pose.  Every device computation is fp64 without contraction and uses only
 * + - * /, sqrt, floor, min, max and comparisons, with every sum in the order written here, so
 * that every output is a function of the inputs alone; tests/global_ref.py restates it in numpy.
 * Below, dot(a, b) = (a0 b0 + a1 b1) + a2 b2, |a|^2 = dot(a, a) and
 * cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).
 * ---------------------------------------------------------------------------------------- */

/* Fast point feature histograms over k-NN neighbourhoods, 3 x 11 bins, 1 <= k <=
 * RS_CLOUD_KNN_MAX_K - 1.  pts (n, 3), normals (n, 3), used as given (unit length is the caller's
 * business).
 *   Neighbours.  The list of point i is rs_cloud_knn's row of the k + 1 nearest with one entry
 *   dropped by the rule of rs_cloud_knn_mean_dist (the entry that names i, else the last), walked
 *   in list order; d2 is the list's.  The lists stay on the device.
 *   Pairs.  With d = p_j - p_i and c = cross(d, n_i), the pair (i, j) is counted when d2 > 0, the
 *   six numbers of n_i and n_j are finite and |c|^2 > 0.  Then u = n_i, v = c / sqrt(|c|^2),
 *   w = cross(u, v), f1 = dot(v, n_j), f2 = dot(u, d) / sqrt(d2), x = dot(u, n_j),
 *   y = dot(w, n_j).
 *   Pseudo-angle a in [0, 4] of (x, y): den = |x| + |y|; a = 0 unless den > 0; r = y / den;
 *   a = 1 + r where x >= 0, else 3 - r where y >= 0, else (-1 - r) + 4.
 *   Bins.  bin(q) = 0 unless floor(q) >= 0, 10 where floor(q) > 10, else floor(q);
 *   b1 = bin((f1 + 1) 5.5), b2 = bin((f2 + 1) 5.5), b3 = bin(a 2.75).  SPFH_i, 33 int32 counts,
 *   gains one at b1, 11 + b2 and 22 + b3 for every counted pair; c_i is their number.
 *   Histograms.  Over the listed j with d2 > 0 and c_j > 0, in list order from +0.0, with
 *   w_j = 1 / sqrt(d2): A[b] += (w_j SPFH_j[b]) / c_j and W += w_j.  Then
 *   fpfh[i][b] = SPFH_i[b] / c_i + A[b] / W.  A row with c_i = 0 or without such a j is NaN.
 * count[i] = c_i.  info is rs_cloud_knn's for the lists (rows_short against k + 1).  The result
 * does not depend on `cell`.  RS_EINVAL as rs_cloud_knn_mean_dist; n = 0 returns at once. */
#define RS_FPFH_BINS 33
int rs_cloud_fpfh(rs_ctx *ctx, const double *pts, const double *normals, int64_t n, int32_t k,
                  double cell, double *fpfh, int32_t *count, rs_knn_info *info);

/* Nearest descriptor by brute force.  fa (n, D), fb (m, D), 1 <= D <= RS_FEATURE_MATCH_MAX_D.
 *   d2(i, j) = sum over c = 0 .. D - 1, left to right from the first term, of
 *   (fa[i][c] - fb[j][c]) (fa[i][c] - fb[j][c]).
 *   idx[i] is the lowest j among those with the smallest d2(i, j) < +inf, d2[i] that value;
 *   idx[i] = -1 and d2[i] = +inf where there is none: a NaN in row i, in every row of fb, or
 *   m = 0.  A row of fb that holds a NaN is nobody's match.
 * fb goes through LDS in tiles of RS_FEATURE_MATCH_TILE rows; the result does not depend on it.
 * RS_EINVAL: a null pointer where elements are expected, D out of range, n or m negative or
 * above RS_CLOUD_MAX_POINTS.  n = 0 returns at once. */
#define RS_FEATURE_MATCH_MAX_D 64
#define RS_FEATURE_MATCH_TILE 96
int rs_feature_match(rs_ctx *ctx, const double *fa, int64_t n, const double *fb, int64_t m,
                     int32_t D, int32_t *idx, double *d2);

/* RANSAC over the similarities of three correspondences src[i] <-> dst[i], i < M.
 *   Hypothesis h, 0 <= h < H, draws (i0, i1, i2) = floyd_sample<3>(seed, h, M), the sampler of
 *   the F and PnP kernels (tests/philox_ref.py); a_k = src[i_k], b_k = dst[i_k].
 *   Edges (0, 1), (0, 2), (1, 2): la = sqrt(|a_p - a_q|^2), lb = sqrt(|b_p - b_q|^2).
 *   Gates, in this order; a hypothesis leaves at the first it fails, and a comparison with a NaN
 *   fails:
 *   1. no two of b_0, b_1, b_2 are equal in all three coordinates;
 *   2. every la > min_edge;
 *   3. with r = lb / la per edge, max r <= (1 + edge_tol) min r (max and min taken over the
 *      edges in the order above); without with_scale also 1 / (1 + edge_tol) <= r <= 1 + edge_tol
 *      for every edge;
 *   4. scale_lo <= s <= scale_hi;
 *   5. the 13 numbers of the model are finite (a collinear triple is not).
 *   Model.  ca = ((a_0 + a_1) + a_2) / 3, cb likewise.  The frame of a triangle: e1 = a_1 - a_0,
 *   e2 = a_2 - a_0, x = e1 / sqrt(|e1|^2), g = cross(e1, e2), z = g / sqrt(|g|^2),
 *   y = cross(z, x).  R[r][c] = (xb[r] xa[c] + yb[r] ya[c]) + zb[r] za[c].
 *   s = sqrt((|b_0 - cb|^2 + |b_1 - cb|^2) + |b_2 - cb|^2) / sqrt(the same of a), 1 without
 *   with_scale.  t[r] = cb[r] - s ((R[r][0] ca[0] + R[r][1] ca[1]) + R[r][2] ca[2]).
 *   Score.  count = the number of i with |p' - dst[i]|^2 <= inlier_dist inlier_dist, p' the
 *   image of src[i] under rs_eval_index_step's transform expression,
 *   p'[r] = s ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r].
 * out holds the `candidates` best survivors by (count descending, h ascending), found of them
 * (info); the rest of out is zero.  Nothing depends on the launch shape, on the chunks of
 * RS_SIM3_CHUNK hypotheses the call works through or on the order in which survivors are
 * compacted.  RS_EINVAL: a null pointer, M < 3 or above 2^24, H < 1 or above 2^32, candidates
 * outside 1..RS_SIM3_MAX_CANDIDATES, inlier_dist, edge_tol, min_edge negative or not finite,
 * scale_lo or scale_hi NaN or negative. */
#define RS_SIM3_MAX_CANDIDATES 1024
#define RS_SIM3_CHUNK (1 << 20)
typedef struct rs_sim3_candidate {
  int64_t h;        /* the hypothesis                                  */
  int64_t count;    /* its score                                       */
  double model[13]; /* s, R row-major, t                               */
} rs_sim3_candidate; /* 120 bytes */
typedef struct rs_sim3_info {
  int64_t hypotheses; /* H                                             */
  int64_t passed[5];  /* hypotheses that passed gate 1, .., gate 5     */
  int64_t tests;      /* survivors x M                                 */
  int64_t found;      /* entries of out that are filled                */
} rs_sim3_info;       /* 64 bytes */
int rs_sim3_ransac(rs_ctx *ctx, const double *src, const double *dst, int64_t M, int64_t H,
                   double inlier_dist, uint64_t seed, int32_t with_scale, double scale_lo,
                   double scale_hi, double edge_tol, double min_edge, int32_t candidates,
                   rs_sim3_candidate *out, rs_sim3_info *info);

/* HIP events between the kernels of the next global-registration calls (enable != 0).  Returns
 * the last timed call's device ms per stage: spfh, fpfh (rs_cloud_fpfh, after the k-NN stages
 * that rs_cloud_knn_timing reports), match (rs_feature_match), solve, count, gather
 * (rs_sim3_ransac, summed over its chunks); -1 where none (tools/bench_global.py). */
#define RS_GLOBAL_TIMING_SLOTS 6
int rs_global_timing(rs_ctx *ctx, int32_t enable, double *ms);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (RCCL over xGMI).  One process per GPU; the unique id travels out of band.
 * ---------------------------------------------------------------------------------------- */
#define RS_COMM_ID_BYTES 128
int rs_comm_unique_id(uint8_t *id_out);
int rs_comm_init(rs_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t *id);
int rs_comm_destroy(rs_ctx *ctx);
/* All-gather of `bytes` per rank (host buffers; staged through HBM). */
int rs_comm_allgather(rs_ctx *ctx, const void *send, void *recv, int64_t bytes);
/* The RCCL this process runs: version (ncclGetVersion) and the path of the shared object
 * that provides it (up to cap bytes, NUL-terminated). */
int rs_comm_library(int32_t *version, char *path, int64_t cap);
/* Max-all-reduce of one int64 (c* across hypothesis shards). */
int rs_comm_allreduce_max_i64(rs_ctx *ctx, int64_t *value);

#ifdef __cplusplus
}
#endif

#endif /* RSAMD_H */
