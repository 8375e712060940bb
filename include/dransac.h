/*
 * dransac.h -- C ABI of libdransac.so, the MI355X (gfx950) implementation of the
 * differentiable-RANSAC hot path (sampler -> minimal solver -> soft-inlier scoring).
 *
 * The reference (weitong8591/differentiable_ransac) has NO native boundary: its hot path is
 * duck-typed Python objects consumed by RANSAC.__init__ (ransac.py:8-39).  Each entry point
 * below therefore cites the reference *Python* interface it replaces; the Python plugin
 * classes in differentiable_ransac_amd/ bind these symbols through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to a contiguous row-major array, unless marked [host];
 *   - P = image pairs, N = points per pair, B = hypotheses (minimal samples) per pair,
 *     k = sample size, S = model slots per sample, M = models per pair (= B*S);
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *   - return value: DR_OK (0) or a negative DR_E* code; dr_last_error() gives the message of
 *     the last failure on the calling thread.  No entry point throws, aborts or allocates
 *     device memory; scratch space is passed in by the caller where needed;
 *   - *_f32 entry points take float I/O, *_f64 double I/O.  Minimal solvers always compute
 *     in f64 internally (f64 FMA runs at the scalar-f32 rate on CDNA4) so that the f32 entry
 *     points meet the 1e-4 model tolerance that the reference's own f32 path does not.
 *   - numerically failed hypotheses never produce NaN: their slot is eye(3) and valid = 0
 *     (the reference drops them, nister.py:154-157,365-366,400-405).
 */
#ifndef DRANSAC_H_
#define DRANSAC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_OK 0
#define DR_EINVAL (-1)  /* bad argument (null pointer, non-positive size, unsupported k) */
#define DR_ELAUNCH (-2) /* HIP launch / runtime failure */
#define DR_ENOTIMPL (-3)

#define DR_ABI_VERSION 1

int dr_version(void);
const char *dr_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  Gumbel-softmax top-k sampler     GumbelSoftmaxSampler.sample, samplers/gumbel_sampler.py:25-42
 *
 *   g[p,b,n] = (logits[p,n] + gumbel[p,b,n]) / tau ; y = softmax_n(g) ; idx = top-k_n(g).
 *   gumbel == NULL  -> noise generated in-kernel: Philox4x32-7(key = seed, counter = (n/4, b, p, 0)),
 *                      word n%4 of the call = w; u = fl(float(w) * 2^-32 (1-eps-tiny) + tiny) (the u32 -> f32 conversion rounds
 *                      w to 24 significant bits: torch's tiny + rand * (1-eps-tiny) with rand on the 2^-24 grid),
 *                      gumbel = -ln2 * log2(-log2 u) - ln ln 2 = -log(-log u), rounded to an f32 VALUE before it meets the logit;
 *   gumbel != NULL  -> explicit noise [P,B,N] (parity mode: index sets are bit-exact w.r.t. the reference).
 *   Outputs: idx [P,B,k] int32, ASCENDING point index (= the order `points[samples != 0]` yields,
 *   ransac.py:65); y_sel [P,B,k] = y at idx; lse [P,B] = log-sum-exp of g (so y = exp(g - lse));
 *   optional dense outputs (API-faithful mode) y_soft [P,B,N], ret [P,B,N] = y_hard - y + y
 *   (gumbel_sampler.py:38) and gumbel_out [P,B,N] (the noise that was used); NULL to skip.
 *   logits == NULL  -> all-ones logits (gumbel_sampler.py:27-28).
 *   y_sel == NULL and lse == NULL (both, and then no dense outputs) -> index sets only: what test mode consumes
 *   (`points[samples != 0]`, ransac.py:65); the same idx, without the soft-max statistics of the rows.
 * ------------------------------------------------------------------------------------------ */
/* seed_dev (every sampler entry; round 6: ONE entry per sampler, the `_dseed` twins of rounds 2-5 are gone): NULL = the Philox key is `seed`; != NULL = the key is read from DEVICE memory (`*seed_dev`) when the kernel
 * starts and `seed` is ignored -- for steps captured in a HIP graph, where a by-value seed would be frozen at capture time.  Same
 * kernels, same random numbers for equal keys; a device key serves the in-kernel noise of given logits only (no explicit noise,
 * no dense outputs).  dr_seed_next_n advances such a key on the device. */
int dr_gumbel_topk_fwd_f32(const float *logits, const float *gumbel, uint64_t seed, const uint64_t *seed_dev, float tau, int P, int B,
                           int N, int k, int32_t *idx, float *y_sel, float *lse, float *y_soft, float *ret,
                           float *gumbel_out, void *stream);
int dr_gumbel_topk_fwd_f64(const double *logits, const double *gumbel, uint64_t seed, const uint64_t *seed_dev, double tau, int P,
                           int B, int N, int k, int32_t *idx, double *y_sel, double *lse, double *y_soft, double *ret,
                           double *gumbel_out, void *stream);

/* Backward of sampler + gather (K1+K2).  a_sel [P,B,k] = dL/d(straight-through value at idx)
 * (= <grad_sample, matches[idx]> + grad_weight, computed by dr_gather_bwd).  grad_logits [P,N] is
 * OVERWRITTEN with (1/tau) * sum_b y*(a - sum_m y_m a_m).  Needs the forward's noise: pass the same
 * gumbel pointer or the same seed. */
int dr_gumbel_topk_bwd_f32(const float *logits, const float *gumbel, uint64_t seed, const uint64_t *seed_dev, float tau, int P, int B,
                           int N, int k, const int32_t *idx, const float *lse, const float *a_sel, float *grad_logits,
                           void *stream);
/* the same in double: `-pr 2 -tr 1` (model_cl.py:164-169; f64 works end to end upstream) */
int dr_gumbel_topk_bwd_f64(const double *logits, const double *gumbel, uint64_t seed, double tau, int P, int B, int N,
                           int k, const int32_t *idx, const double *lse, const double *a_sel, double *grad_logits,
                           void *stream);

/* K1, inference variant: the index SET of the Gumbel top-k sampler by top-down (Plackett-Luce) sampling -- k sequential
 * draws without replacement from softmax(logits), which is the distribution of the top-k of logits + iid Gumbel noise
 * (any tau > 0).  For callers that only consume `samples != 0` (RANSAC test mode, ransac.py:65); y_sel / lse need the
 * whole noise row and come from dr_gumbel_topk_fwd.  logits [P,N] or NULL (uniform); cdf_ws [P,N] f64 workspace (the
 * per-pair cumulative soft-max weights, overwritten); idx [P,B,k] ascending.
 * Philox4x32-7(key = seed, counter = (draw / 2, b, p, 2)). */
int dr_topdown_sample_f32(const float *logits, uint64_t seed, const uint64_t *seed_dev, int P, int B, int N, int k, double *cdf_ws,
                          int32_t *idx, void *stream);
int dr_topdown_sample_f64(const double *logits, uint64_t seed, int P, int B, int N, int k, double *cdf_ws, int32_t *idx,
                          void *stream);

/* K1u  UniformSampler.batch_generate, samplers/uniform_sampler.py:15-19: idx ~ U{0..N-2}, with replacement.
 * Philox4x32-7(key = seed, counter = (j, b, p, 1)). */
int dr_uniform_sample(uint64_t seed, const uint64_t *seed_dev, int P, int B, int k, int N, int32_t *idx, void *stream);

/* K1p  PROSAC sampler (Chum & Matas, CVPR 2005), index sets only: order [P,N] = the points of every pair from the best-ranked
 * to the worst (NULL = the identity), growth [N-k+1] with growth[i] = T'_{k+i}, the number of draws after which the sampler
 * has moved on from the k+i best-ranked points (strictly increasing, growth[0] = 1; ops.prosac_growth).  Row b of the launch
 * is draw t = t0 + b + 1 of every pair:
 *   t <= T'_N: n = min{ n in [k,N] : T'_n >= t }; the ranks are n-1 and k-1 distinct ranks uniform in [0, n-2]
 *              (draw 1 is the ranks 0..k-1; the paper's listing starts at n = k+1);
 *   t >  T'_N: k distinct ranks uniform in [0, N-1].
 * Distinct ranks by Floyd's algorithm: c out of a pool of s from exactly c words, for i = 0..c-1, j = s-c+i:
 * r = (word_i * (j+1)) >> 32, take j where r is already chosen, else r (bias <= (j+1) / 2^32).  word_i is word i & 3 of
 * Philox4x32-7(key = seed, counter = (i >> 2, b, p, 3)).  idx [P,B,k] = order[p, rank], ascending in the point index.
 * seed_dev != NULL: the key is read from device memory.  Ungated.  DR_EINVAL before any launch for a null idx or growth,
 * k outside [1, 8], N < k, P or B < 1, t0 < 0. */
int dr_prosac_sample(const int32_t *order, const int64_t *growth, uint64_t seed, const uint64_t *seed_dev, int64_t t0, int P,
                     int B, int N, int k, int32_t *idx, void *stream);

/* The per-call key of the batched drivers, advanced on the device (every replay of a captured step then draws fresh hypotheses):
 * state[0] = base, state[1] = number of calls so far -> seeds_out[i] = base * 0x9E3779B97F4A7C15 + calls + i (mod 2^64) for
 * i < n (<= 65 536), calls += n: CONSECUTIVE integers, one per call (ransac.py of this package: `_next_seed`).  n = 1 is the
 * `dr_seed_next` of rounds 2-5. */
int dr_seed_next_n(uint64_t *state, uint64_t *seeds_out, int n, void *stream);

/* K1 in index-only mode + K2 in one call (test mode: `points[samples != 0]`, ransac.py:58-65, with in-kernel noise):
 * idx [P,B,k] ascending and samples [P,B,k,4] = matches[p, idx] (c = 4; buffers not 16-byte aligned: always two launches).  One launch when the
 * register-resident sampler kernel serves the shape (N % 4 == 0, N <= 2048, tau == 1), sampler + gather launches otherwise.
 * Every argument from gate_iters on is optional (NULL / 0): */
/* gate_iters / gate_max_iters (a round > 1 of a multi-round test-mode call): pairs with gate_iters[p] >= gate_max_iters[p] are
 * skipped, their rows keep their contents (see dr_ransac_update and the solver entries below) */
/* sub (round 6, super-rounds): > 0 = the B rows are ceil(B / sub) consecutive SUB-BATCHES of `sub` rows, the batches the loop of
 * ransac.py:55-144 draws one call after the other: row b gets the noise of row b % sub of a call keyed (seed | *seed_dev) + b / sub
 * (the drivers' per-call seeds are consecutive integers), so ONE launch samples what ceil(B / sub) calls of that loop sample and
 * dr_ransac_update(sub_models = sub * S) walks them in order.  0 = one batch. */
/* race_ws (round 6; optional, (N + 32) * P floats, 16-byte aligned): rows of <= 2048 points (N % 4 == 0,
 * tau == 1) then rank key_n = exp(lmax - logit_n) * log2 u_n instead of logit_n - ln(-ln u_n) -- the exponential-race form of the
 * same top-k (gumbel_sampler.py:30-36), ONE logarithm per element; the per-pair weights are written into the workspace by a
 * prologue launch.  Same index sets up to the rounding of near-ties (measured: tests/test_gpu_round6.py); pairs whose logits are
 * not all finite or span more than 80 keep the two-logarithm form.  race_ready != 0: the workspace already holds the weights of
 * these logits (dr_ransac_init wrote them, once for all rounds of the call): no prologue launch.  The workspace holds w [P,N], then
 * a flag word and the key density -1 / (ln 2 sum_n 1 / w_n) per pair: this form selects its k winners on wave compare masks, from
 * a threshold searched on that density (same winners, same order as the candidate list of the other forms). */
int dr_gumbel_topk_gather_f32(const float *logits, const float *matches, uint64_t seed, const uint64_t *seed_dev, float tau,
                              int P, int B, int N, int k, int32_t *idx, float *samples,
                              const int32_t *gate_iters, const double *gate_max_iters, int sub, float *race_ws, int race_ready,
                              void *stream);

/* Train mode (round 5): K1 WITH the soft-max statistics + K2 in one call (GumbelSoftmaxSampler.sample, samplers/gumbel_sampler.py:25-42,
 * followed by `matches * ret` + the mask gather of ransac.py:58-65): idx, y_sel [P,B,k], lse [P,B] as dr_gumbel_topk_fwd_f32 and
 * samples [P,B,k,4] = matches[p, idx] * ((1 - y_sel) + y_sel) as dr_gather_fwd_f32 (c = 4; buffers not 16-byte aligned: always two launches).  One launch
 * when the register-resident kernel serves the shape, sampler + gather launches otherwise.
 * race_ws (round 6; optional, (N + 32) * P floats, 16-byte aligned): the one-logarithm form in train mode -- keys, winners AND the
 * soft-max statistics (y_n = (1 / -key_n) / sum_m (1 / -key_m), lse = lmax + ln sum - ln ln 2) from one logarithm and one reciprocal
 * per element; y_sel / lse agree with the two-logarithm form to rounding, the index sets up to the rounding of near-ties
 * (tests/test_gpu_round6.py).  NULL = the two-logarithm form. */
int dr_gumbel_topk_gather_soft_f32(const float *logits, const float *matches, uint64_t seed, const uint64_t *seed_dev, float tau,
                                   int P, int B, int N, int k, int32_t *idx, float *y_sel, float *lse, float *samples, float *race_ws,
                                   void *stream);
/* ... and the backward of the pair in one launch: grad_logits [P,N] from grad_samples [P,B,k,4] and grad_w [P,B,k]
 * (gradient of the y_sel output; NULL = none) -- dr_gather_bwd_f32's a_sel is formed inside dr_gumbel_topk_bwd_f32's row
 * prologue.  The correspondences receive no gradient from this entry. */
int dr_gumbel_topk_gather_bwd_f32(const float *logits, const float *matches, uint64_t seed, const uint64_t *seed_dev, float tau,
                                  int P, int B, int N, int k, const int32_t *idx, const float *lse, const float *grad_samples,
                                  const float *grad_w, float *grad_logits, void *stream);

/* K1, index sets only, in-kernel noise, with an optional screening workspace (round 4; GumbelSoftmaxSampler.sample,
 * samplers/gumbel_sampler.py:25-42, as test mode consumes it: `points[samples != 0]`, ransac.py:65).
 * screen_ws: (N + 32) * P 32-bit words of device memory, 16-byte aligned, or NULL (then = dr_gumbel_topk_fwd_f32 with
 * y_sel = lse = NULL).  With a workspace, rows longer than the register kernel holds (N > 2048, N % 4 == 0, tau == 1, k <= 5)
 * are SCREENED: one pass over the pair's logits writes, per point, the smallest Philox word that can still lift the point to the
 * score T = logsumexp(logits) - ln(20 + k) (rounded down); a step of a wave (256 points) in which no word reaches its
 * threshold is skipped after Philox + four integer compares -- no Gumbel transform, no logits, no list update.  Steps with a
 * candidate are evaluated in full, so every listed score is exact; a row in which fewer than k evaluated scores reach T
 * (probability < 1e-7) repeats itself unscreened.  The index sets are those of dr_gumbel_topk_fwd_f32 for the same seed, bit
 * for bit (tests/test_gpu_round4.py).  seed_dev != NULL: the Philox key is read from device memory (captured graphs). */
int dr_gumbel_topk_index_f32(const float *logits, uint64_t seed, const uint64_t *seed_dev, float tau, int P, int B, int N, int k,
                             int32_t *idx, uint32_t *screen_ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * K2  straight-through gather          RANSAC.__call__, ransac.py:58-65 (+ :73 weighted)
 *   samples[p,b,j,:] = matches[p, idx[p,b,j], :] * st[p,b,j],  st = (1 - y_sel) + y_sel  (f32 rounding
 *   of y_hard - y_soft + y_soft); y_sel == NULL -> st = 1 (uniform sampler, ransac.py:60).
 *   c = 4 (two-view) or 6 (3-D).
 * ------------------------------------------------------------------------------------------ */
int dr_gather_fwd_f32(const float *matches, const int32_t *idx, const float *y_sel, int P, int N, int B, int k,
                      int c, float *samples, void *stream);
int dr_gather_fwd_f64(const double *matches, const int32_t *idx, const double *y_sel, int P, int N, int B, int k,
                      int c, double *samples, void *stream);
/* a_sel[p,b,j] = <grad_samples[p,b,j,:], matches[p,idx,:]> (+ grad_w[p,b,j] if non-NULL);
 * grad_matches [P,N,c] (may be NULL) += grad_samples * st  (atomic; caller zeroes it). */
int dr_gather_bwd_f32(const float *matches, const int32_t *idx, const float *y_sel, const float *grad_samples,
                      const float *grad_w, int P, int N, int B, int k, int c, float *a_sel, float *grad_matches,
                      void *stream);
int dr_gather_bwd_f64(const double *matches, const int32_t *idx, const double *y_sel, const double *grad_samples,
                      const double *grad_w, int P, int N, int B, int k, int c, double *a_sel, double *grad_matches,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * K3  minimal solvers.  samples [Bt,k,c] (Bt = total hypotheses = P*B, flattened), optional
 *     per-point weights [Bt,k] (NULL = unweighted).  models [Bt,S,9] row-major 3x3 (rigid: [Bt,16]),
 *     valid [Bt,S] uint8.
 *
 *   dr_solve_nister5     EssentialMatrixEstimatorNister.estimate_minimal_model, nister.py:69-408; S = 10;
 *                        n >= 5 points per sample (n > 5 = the non-minimal fallback of nister.py:64-65);
 *                        real roots only, ascending in z; unit Frobenius norm; unused slots = eye(3).
 *   dr_solve_stewenius5  EssentialMatrixEstimator.estimate_minimal_model, stewenius.py:20-80; S = 10;
 *                        unit Frobenius norm (the reference leaves LAPACK's eigenvector scale).
 *   dr_solve_f8          FundamentalMatrixEstimatorNew normalize + estimate_non_minimal_model,
 *                        fundamental_matrix_estimator.py:177-260; S = 1; n >= 8.
 *   dr_solve_f7          7-point with the correct maths (reference degenerate, Q7/Q8); S = 4.
 *   dr_solve_rigid       RigidTransformationSVDBasedSolver.estimate_model, rigid…:11-74; n >= 3, c = 6;
 *                        models [Bt,16] = 4x4, also R [Bt,9], t [Bt,3], scale [Bt] (any may be NULL);
 *                        flag != 0 reproduces the reference default (svd of cov^T cov, R ~ I, Q9).
 * ------------------------------------------------------------------------------------------ */
/* The f32 five-point entries carry every option of the path (round 6: the `_hp`, `_path_`, `_gated_` twins of rounds 3-5 are
 * gone); everything after `valid` is optional (NULL / 0):
 *   models_f64 (Nister, n = 5): train mode -- the models written BOTH as f32 (what the scoring reads) and as f64 polished to the
 *     f64 tolerance (what dr_solve_nister5_bwd_f32 wants), from one launch: the models of dr_solve_nister5_f64 on the widened
 *     samples without the two conversion passes;
 *   path (n = 5): 0 = automatic, 1 = two lanes per sample from the first instruction (the only kernels until round 4), 2 = the
 *     two-phase kernels: ONE lane per sample for the part the two lanes of a sample otherwise compute twice (null space, the ten
 *     constraints, QR, reduced rows, det B(z) of nister.py:117-348 / the action matrix' characteristic polynomial of
 *     stewenius.py:44-74), handed over in registers to the two-lanes-per-sample root search and final stage (nister.py:355-402,
 *     stewenius.py:74-78); automatic = two-phase when the grid is at least two rounds of lane-pair blocks.  Same solutions either
 *     way (Stewenius: bit for bit; Nister: to the rounding of det B(z));
 *   gate_iters / gate_max_iters + per_pair (n = 5; Bt = pairs x per_pair): device-side termination (ransac.py:135-144:
 *     `max_iters = min(max_iterations, adaptive_iteration_number(...))` decides per pair when the loop of ransac.py:55 ends).  The
 *     per-pair counters live on the device (dr_ransac_init / dr_ransac_update: iters [P] int32, max_iters [P] f64); a block all of
 *     whose samples belong to pairs with iters >= max_iters returns at once, its outputs keep their contents, and dr_ransac_update
 *     leaves such a pair's state alone.  The driver can therefore ISSUE every round of a call without reading anything back -- one
 *     HIP graph per call, whatever the data decide. */
int dr_solve_nister5_f32(const float *samples, const float *weights, int Bt, int n, float *models, double *models_f64, uint8_t *valid,
                         int path, int per_pair, const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_solve_nister5_f64(const double *samples, const double *weights, int Bt, int n, double *models,
                         uint8_t *valid, void *stream);
int dr_solve_stewenius5_f32(const float *samples, int Bt, float *models, uint8_t *valid, int path, int per_pair,
                            const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_solve_stewenius5_f64(const double *samples, int Bt, double *models, uint8_t *valid, void *stream);
int dr_solve_f8_f32(const float *samples, const float *weights, int Bt, int n, float *models, uint8_t *valid,
                    void *stream);
int dr_solve_f8_f64(const double *samples, const double *weights, int Bt, int n, double *models, uint8_t *valid,
                    void *stream);
/* Test hook: the real-root search of the five-point kernels (replaces torch.linalg.eigvals of the companion matrix,
 * nister.py:361-370, and eig, stewenius.py:74) on given polynomials.  coef [n,11] ascending; per polynomial two searches,
 * exactly as the solver kernels run them: roots [n,2,10] -- [.,0,.] the roots with |z| <= 1 ascending, [.,1,.] those with
 * |z| > 1 (found as roots w of the reversed polynomial, ascending in w, returned as 1/w) -- and counts [n,2].
 * method 0 = derivative chain (rounds 1-2), 1 = Sturm-sequence isolation (round 3, what the kernels run). */
int dr_debug_real_roots10(const double *coef, int n, int method, double *roots, int32_t *counts, void *stream);
/* K1u + K2 + K3f8 in one launch (round 4; UniformSampler.batch_generate, uniform_sampler.py:15-19 -> `matches[idx]`, ransac.py:60
 * -> FundamentalMatrixEstimatorNew.estimate_model on the minimal sample): matches [P,N,4]; every one of the P x B samples draws
 * its eight indices in [0, N - 2] itself -- the index sets dr_uniform_sample(seed, P, B, 8, N) draws -- and is solved by the
 * 8-point kernel: idx [P,B,8] (may be NULL), models [P*B,9], valid [P*B].  seed_dev != NULL: the key is read from device memory. */
int dr_solve_f8_uniform_f32(const float *matches, uint64_t seed, const uint64_t *seed_dev, int P, int B, int N, int32_t *idx,
                            float *models, uint8_t *valid, void *stream);
int dr_solve_f7_f32(const float *samples, int Bt, float *models, uint8_t *valid, void *stream);
int dr_solve_f7_f64(const double *samples, int Bt, double *models, uint8_t *valid, void *stream);
int dr_solve_rigid_f32(const float *samples, const float *weights, int Bt, int n, int flag, float *models, float *R,
                       float *t, float *scale, uint8_t *valid, void *stream);
int dr_solve_rigid_f64(const double *samples, const double *weights, int Bt, int n, int flag, double *models,
                       double *R, double *t, double *scale, uint8_t *valid, void *stream);

/* Backward of the minimal solvers by implicit differentiation of the defining constraints at the
 * returned model.  grad_models has the forward's model shape; grad_samples [Bt,k,c]
 * is overwritten.  Invalid slots contribute nothing. */
/* models_f64 (optional, preferred): the same models computed by dr_solve_nister5_f64 on the same samples -- with
 * f32-rounded models the epipolar residual (6e-8) is amplified by the conditioning of the tangent-space system. */
int dr_solve_nister5_bwd_f32(const float *samples, const float *models, const double *models_f64,
                             const uint8_t *valid, const float *grad_models, int Bt, float *grad_samples,
                             void *stream);
/* The same with the gradient in the form K5 leaves it (ransac.py:87-96 picks ONE of a sample's ten models): grad_chosen [Bt,9]
 * = gradient of the model in slot which[s] (which [Bt] int32 from dr_select_closest; < 0 = no model picked), all other slots
 * carry none.  Replaces dr_select_closest_bwd + dr_solve_nister5_bwd on the training path (no dense [Bt,10,9] gradient). */
int dr_solve_nister5_bwd_sel_f32(const float *samples, const float *models, const double *models_f64,
                                 const uint8_t *valid, const float *grad_chosen, const int32_t *which, int Bt,
                                 float *grad_samples, void *stream);
/* Round 5: the same backward kernels with f64 samples / models / gradients in memory (`-pr 2 -tr 1`, model_cl.py:164-169, Q17):
 * the arithmetic was f64 already; until round 4 the f64 training path rounded their inputs and outputs to f32. */
int dr_solve_nister5_bwd_f64(const double *samples, const double *models, const uint8_t *valid, const double *grad_models, int Bt,
                             double *grad_samples, void *stream);
int dr_solve_f8_bwd_f64(const double *samples, const double *weights, const double *models, const double *grad_models, int Bt, int n,
                        double *grad_samples, double *grad_weights, void *stream);
/* Non-minimal samples (n > 5 rows per sample, optional row weights: ransac.py:82-83 `num_samples == 8` feeding the five-point
 * estimator, which runs its minimal code on all rows -- nister.py:64-65, weighted rows :88-93).  The returned models lie in the
 * span of the four smallest eigenvectors of sum_r w_r^2 rho_r rho_r^T; the backward differentiates that invariant subspace and
 * the essential-manifold constraints implicitly.  grad_models [Bt,10,9] dense, grad_samples [Bt,n,4] and grad_weights [Bt,n]
 * (optional) are overwritten. */
int dr_solve_nister5_nm_bwd_f32(const float *samples, const float *weights, const float *models, const double *models_f64,
                                const uint8_t *valid, const float *grad_models, int Bt, int n, float *grad_samples,
                                float *grad_weights, void *stream);
/* the same with samples, weights, models and gradients f64 in memory (`-sam 3 -fmat 0 -tr 1 -pr 2`, model_cl.py:164-169; round 6) */
int dr_solve_nister5_nm_bwd_f64(const double *samples, const double *weights, const double *models, const uint8_t *valid,
                                const double *grad_models, int Bt, int n, double *grad_samples, double *grad_weights, void *stream);
int dr_solve_f8_bwd_f32(const float *samples, const float *weights, const float *models, const float *grad_models,
                        int Bt, int n, float *grad_samples, float *grad_weights, void *stream);
int dr_solve_rigid_bwd_f32(const float *samples, const float *models, const float *grad_models, int Bt, int n,
                           int flag, float *grad_samples, void *stream);

/* ------------------------------------------------------------------------------------------
 * K4  MSAC soft-inlier scoring on the Sampson distance      MSACScore.score, scorings/msac_score.py:12-55
 *   matches [P,N,4], models [P,M,9], thr [P] (the `threshold` argument per pair; the kernel applies
 *   the (3/2 thr)^2 of msac_score.py:21).  scores [P,M]; masks [P,M,N] uint8 (torch.bool layout) or NULL.
 *   Models with a non-finite coefficient get score = NaN and an all-false mask (what the reference's
 *   arithmetic yields for them).  valid [P,M] uint8 (optional, NULL = score everything): slots the solver marked
 *   invalid (eye(3) fillers of non-real roots) get score 0 and an all-false mask row without being evaluated.
 * ------------------------------------------------------------------------------------------ */
/*   gate_iters / gate_max_iters (f32; optional, NULL = none; round 6: the `_gated` twin of round 5 folded in): a round > 1 of a
 *   multi-round test-mode call -- the blocks of a pair with gate_iters[p] >= gate_max_iters[p] return at once, its scores / masks
 *   keep their contents (dr_ransac_update ignores such pairs). */
int dr_msac_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr, int P,
                      int M, int N, float *scores, uint8_t *masks, const int32_t *gate_iters, const double *gate_max_iters,
                      void *stream);
int dr_msac_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr, int P,
                      int M, int N, double *scores, uint8_t *masks, void *stream);
/* (The explicit-path entry of rounds 2-5, dr_msac_score_path_f32, is gone: path 0 = path 1 = this kernel family -- every (model,
 * point) through the f32 fma chain on the vector units; rows of <= 256 points: a wave per model with 1 / 2 / 4 points per lane,
 * longer rows: a lane owns 8 / 16 points -- and path 2, the matrix-core candidate filter of round 2, measured slower, left the
 * library in round 4: scratch/k4_filter_kernel.patch.) */
/* dL/dmodels [P,M,9] from dL/dscores [P,M] (flows only through points with d2 < thr2). */
int dr_msac_score_bwd_f32(const float *matches, const float *models, const float *thr, const float *grad_scores,
                          int P, int M, int N, float *grad_models, void *stream);

/* K4r squared residual of rigid models   RigidTransformationSVDBasedSolver.squared_residual, rigid…:76-89
 *   pts [P,N,6] = (p,q); models [P,M,16] (4x4: q_hat = R p + t with the reference's row-vector descriptor
 *   D = model[:3,:]^T, ransac.py:380); res_sum [P,M] = sum_n d2; masks [P,M,N] = d2 < threshold or NULL.
 *   The reference's scalar mean is sum(res_sum)/(M*N), left to the caller. */
/*   accumulate (f32): != 0 = the sums are ADDED to res_sum, which must hold zeros (dr_solve_rigid_gather_f32 with zero_sums =
 *   res_sum, M = B, leaves it so): no memset launch (round 6: the `_acc` twin of round 4 folded in) */
int dr_rigid_residual_f32(const float *pts, const float *models, float threshold, int P, int M, int N,
                          float *res_sum, uint8_t *masks, int accumulate, void *stream);
int dr_rigid_residual_f64(const double *pts, const double *models, double threshold, int P, int M, int N,
                          double *res_sum, uint8_t *masks, void *stream);
/* Round 4, test mode of the 3-D driver (RANSAC3D.__call__, ransac.py:355-367,380): K2 + K3r in one launch and K4r without its
 * memset launch.
 *   dr_solve_rigid_gather_f32: samples are read straight through the index sets -- matches [P,N,6], idx [P,B,k] ->
 *     models [P*B,16], R / t / scale (may be NULL), valid [P*B]; zero_sums [P*B] (may be NULL) is cleared on the way;
 *   dr_rigid_residual_f32(accumulate = 1) then adds the sums to it. */
int dr_solve_rigid_gather_f32(const float *matches, const int32_t *idx, int P, int B, int N, int k, int flag, float *models,
                              float *R, float *t, float *scale, uint8_t *valid, float *zero_sums, void *stream);
int dr_rigid_residual_bwd_f32(const float *pts, const float *models, const float *grad_res, int P, int M, int N,
                              float *grad_models, void *stream);

/* K6 of the 3-D path (RANSAC3D.__call__ test branch, ransac.py:383-406 -- dead code upstream; selection rule =
 * the valid model with the smallest residual sum, as BatchedRANSAC3D documents): per pair the arg-min of res [P,M] over the
 * valid slots (valid [P,M] or NULL; NaN sums never win; ties -> lowest index), compared STRICTLY with best_res_in [P].
 * Where it is better: best_res_out / best_model_out [P,16] take the winner and best_mask [P,N] (or NULL) is rewritten with
 * `d2 < threshold` of the winner; elsewhere the state is copied through and the mask left alone.  The small state is
 * ping-ponged (in != out) because several blocks serve one pair.  best_idx [P] (or NULL): the round's winner, -1 if kept.
 * First round of a call: best_res_in = best_model_in = NULL stands for "no state yet" (residual +inf, model = identity, empty
 * mask -- the mask is then written in full even where no model is selected). */
int dr_ransac3d_update_f32(const float *pts, const float *models, const uint8_t *valid, const float *res, float threshold,
                           int P, int M, int N, const float *best_res_in, const float *best_model_in, float *best_res_out,
                           float *best_model_out, uint8_t *best_mask, int32_t *best_idx, void *stream);
int dr_ransac3d_update_f64(const double *pts, const double *models, const uint8_t *valid, const double *res, double threshold,
                           int P, int M, int N, const double *best_res_in, const double *best_model_in, double *best_res_out,
                           double *best_model_out, uint8_t *best_mask, int32_t *best_idx, void *stream);

/* ------------------------------------------------------------------------------------------
 * Robust 3-D registration (test mode; ransac.BatchedRegistration).  Not a restatement of upstream code: the reference's
 * `valid=True` branch of RANSAC3D raises NameError, and dr_solve_rigid reproduces its estimate_model on purpose (Q9, the row-sum
 * translation of rigid...:66).  matches [P,N,6] = (p, q); models [.,16] = row-major 4x4 [[R, t], [0, 0, 0, 1]]; q_hat = R p + t,
 * d2 = |q - q_hat|^2.  The threshold is a DISTANCE and enters as thr2 [P] = threshold^2: a point is an inlier iff d2 < thr2
 * (dr_rigid_residual compares d2 with its threshold argument itself).  MSAC score = sum_n max(0, 1 - d2_n / thr2).
 *
 *   dr_kabsch_gather        idx [P,B,k] int32, 3 <= k <= 8 -> models [P,B,16], valid [P,B]: the least-squares rigid fit of every
 *     sample, f64 inside: c0, c1 = means, H = sum (p - c0)(q - c1)^T = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t = c1 - R c0.
 *     valid = 0, model = identity: anything non-finite, an index outside [0, N), or the second eigenvalue of H^T H <= 1e-24 x the
 *     first (sigma_2 <= 1e-12 sigma_1: coincident or collinear rows).
 *   dr_rigid_msac_score     models [P,M,16], valid [P,M] or NULL -> scores [P,M], inliers [P,M] int32 (or NULL); invalid slots
 *     score -1 (0 inliers).  No [P,M,N] tensor; every sum is reduced in one fixed order, so a repeated launch gives the same bits.
 *     gate_iters / gate_max_iters (optional): the blocks of pairs with iters >= max_iters return at once.
 *   dr_registration_update  dr_ransac_update's state step: for every pair with iters < max_iters, the first arg-max of scores over
 *     valid, non-NaN models replaces the state if score > best_score or iters == 0 -- best_score, best_model [P,16], best_mask [P,N]
 *     and best_inliers recomputed for the winner, max_iters = min(max_iterations, adaptive_iteration_number(inliers, N, 3)) in f64 --
 *     and iters += B.  No valid model: only iters moves.  Terminated pairs are untouched.  One block per pair writes its state.
 *   dr_refit_rigid          the fit of dr_kabsch_gather over the rows mask [P,N] selects (NULL = all), weights [P,N] (optional)
 *     multiplying a row's term in the means and in H -> model [P,16], valid [P]; valid = 0 below three rows or for a degenerate H.
 *   dr_registration_local_opt  local optimisation of the pair state (BatchedRegistration(lo = 1 | 2)), one launch behind every
 *     dr_registration_update, no read-back.  lo_seen [P,17] is the caller's snapshot (best_score, best_model [16]) of the last visit,
 *     initialised to NaN: a pair whose state still equals it bit for bit returns with nothing written, terminated or not.  Below
 *     three best_inliers only the snapshot is stored.  Otherwise, once (lo = 1) or up to lo_iters times (lo = 2): dr_refit_rigid's
 *     fit over best_mask; its MSAC score and inlier count over all N points (d2 < thr2, strict; one fixed reduction order, no
 *     floating-point atomics); taken only if score > best_score -- strict, as in dr_registration_update -- and then best_score,
 *     best_model, best_mask (the candidate's own row) and best_inliers (that mask's count) are rewritten.  The loop ends on an invalid
 *     or non-finite fit, on a candidate that loses, and on an accepted mask equal to the previous one.  Then max_iters =
 *     min(max_iterations, adaptive_iteration_number(best_inliers, N, 3)) in f64, the snapshot is stored, and lo_refits[p] (NULL = not
 *     counted) grows by the number of fits run.  DR_EINVAL: a null required pointer, P or N < 1, lo not 1 or 2, lo_iters < 1.
 *   dr_rigid_magsac_score   the MAGSAC++ score in dr_rigid_msac_score's place: same arguments, same mapping, same rules (invalid slots
 *     -1 / 0 inliers, gate, fixed reduction order), another per-point term.  The cutoff distance is read as k sigma_max with
 *     k^2 = 11.344866730144373, the 0.99 quantile of chi^2 with 3 degrees of freedom, the noise scale uniform in [0, sigma_max].  With
 *     s = d2 / thr2, u_k = k^2 / 2, c = exp(-u_k):  weight w(s) = (exp(-u_k s) - c) / (1 - c) for s < 1, else 0;  loss
 *     l(s) = (1 - exp(-u_k s) - c u_k s) / (1 - c (1 + u_k)) for s < 1, else 1 (int_0^d x w(x) dx over its value at the cutoff);
 *     scores = sum_n (1 - l(s_n)) in [0, N], inliers = #{d2_n < thr2} as above.  A non-finite d2 contributes nothing.  The
 *     exponential is v_exp_f32 (1 ulp) in f32 and the device library's exp (1 ulp) in f64.
 *   dr_registration_irls    the IRLS polish of the pair state under that loss (BatchedRegistration(scoring = "magsac")), one launch,
 *     no read-back: from (best_model, best_score), up to irls_iters times, the weights w(s_n) under the current model, dr_refit_rigid's
 *     weighted fit over all points, the candidate's MAGSAC++ score over all points; taken only if score > best_score (strict).  The
 *     loop ends before a fit when fewer than three points have d2 < thr2 (a non-zero weight), on an invalid or non-finite fit and on a
 *     candidate that does not win.  best_score and best_model [P,16] are rewritten where a candidate won; irls_fits [P] grows by the
 *     fits run.  The mask, the inlier count, iters and max_iters are not arguments: they stay the RANSAC winner's.  DR_EINVAL: a null
 *     pointer, P or N < 1, irls_iters < 1.
 *   dr_kabsch_gather_checked  dr_kabsch_gather behind a rigidity test of the sample (BatchedRegistration(edge_similarity = ...)): a
 *     rigid motion keeps distances, so a sample of inliers has |p_i - p_j| ~ |q_i - q_j| for every pair of its rows.  For every pair
 *     i < j of a sample's k rows, in f64 from the stored values: a2 = |p_i - p_j|^2, b2 = |q_i - q_j|^2, and with
 *     sigma = edge_similarity^2 the edge passes iff a2 >= sigma b2 && b2 >= sigma a2 (Open3D's
 *     CorrespondenceCheckerBasedOnEdgeLength with similarity_threshold = edge_similarity, on squares); a NaN coordinate fails the edge,
 *     two coincident rows pass it (and the fit then rejects the sample as degenerate).  A sample passes iff all k (k - 1) / 2 edges do,
 *     and then gets exactly dr_kabsch_gather's 16 values and valid byte, bit for bit.  A sample that fails gets the identity and
 *     valid = 0 without a fit and counts once in rejected[pair]; a sample with an index outside [0, N) gets the identity and valid = 0
 *     as in dr_kabsch_gather and is not counted.  rejected [P] int32 (NULL = not counted) is ADDED to -- the caller zeroes it -- with
 *     integer atomics, so a repeated launch gives the same counts.  edge_similarity = 0 passes every sample whose edges are finite:
 *     the outputs of dr_kabsch_gather byte for byte.  DR_EINVAL: as dr_kabsch_gather, and edge_similarity outside [0, 1] (or NaN).
 *
 * Train mode (ops.kabsch, ops.weighted_kabsch, BatchedRegistration(train=True)).  With weights w >= 0 (1 when NULL), W = sum w:
 * c0 = sum w p / W, c1 = sum w q / W, H = sum w (p - c0)(q - c1)^T.  The backward entries recompute this forward in f64 from their
 * inputs (no stored model) and differentiate the optimality condition "R H is symmetric" (no SVD): with G = gR - gt c0^T,
 * A = sym(R H), K = tr(A) I - A, Y = G R^T, a = (Y21 - Y12, Y02 - Y20, Y10 - Y01), z = K^-1 a: gH = -R^T [z]x, g_c0 = -R^T gt,
 * g_c1 = gt, and per row g_p = w gH dq + (w / W) g_c0, g_q = w gH^T dp + (w / W) g_c1, g_w = dp^T gH dq + (dp.g_c0 + dq.g_c1) / W.
 * gR, gt are rows 0..2 of a row-major 4x4 gradient; its last row is not read.  A fit that is not valid, or whose det K or result
 * is not finite, passes exact zeros on.  Every output element is written; no atomics, so a repeated launch gives the same bits.
 *
 *   dr_kabsch               samples [Bt,k,6], 3 <= k <= 8, weights [Bt,k] or NULL -> models [Bt,16], valid [Bt]: the fit of
 *     dr_kabsch_gather on explicit sample tensors; without weights, on samples = matches[idx], its models and valid bit for bit.
 *     valid = 0 also for W <= 0.
 *   dr_kabsch_bwd           grad_models [Bt,16] -> grad_samples [Bt,k,6], grad_weights [Bt,k] (or NULL: not wanted).
 *   dr_refit_rigid_bwd      grad_model [P,16] -> grad_matches [P,N,6] and / or grad_weights [P,N] (NULL: not wanted; at least one);
 *     rows the mask drops get exact zeros, and so does every row of a pair with fewer than three rows or an invalid fit.
 * ------------------------------------------------------------------------------------------ */
int dr_kabsch_gather_f32(const float *matches, const int32_t *idx, int P, int B, int N, int k, float *models, uint8_t *valid,
                         void *stream);
int dr_kabsch_gather_f64(const double *matches, const int32_t *idx, int P, int B, int N, int k, double *models, uint8_t *valid,
                         void *stream);
int dr_rigid_msac_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr2, int P, int M, int N,
                            float *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters,
                            void *stream);
int dr_rigid_msac_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr2, int P, int M,
                            int N, double *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters,
                            void *stream);
int dr_registration_update_f32(const float *matches, const float *models, const uint8_t *valid, const float *scores,
                               const float *thr2, int P, int M, int N, int B, double confidence, double eps, int max_iterations,
                               float *best_score, float *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters,
                               double *max_iters, void *stream);
int dr_registration_update_f64(const double *matches, const double *models, const uint8_t *valid, const double *scores,
                               const double *thr2, int P, int M, int N, int B, double confidence, double eps, int max_iterations,
                               double *best_score, double *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters,
                               double *max_iters, void *stream);
int dr_refit_rigid_f32(const float *matches, const uint8_t *mask, const float *weights, int P, int N, float *model, uint8_t *valid,
                       void *stream);
int dr_refit_rigid_f64(const double *matches, const uint8_t *mask, const double *weights, int P, int N, double *model, uint8_t *valid,
                       void *stream);
int dr_registration_local_opt_f32(const float *matches, const float *thr2, int P, int N, int lo, int lo_iters, double confidence,
                                  double eps, int max_iterations, float *best_score, float *best_model, uint8_t *best_mask,
                                  int32_t *best_inliers, double *max_iters, float *lo_seen, int32_t *lo_refits, void *stream);
int dr_registration_local_opt_f64(const double *matches, const double *thr2, int P, int N, int lo, int lo_iters, double confidence,
                                  double eps, int max_iterations, double *best_score, double *best_model, uint8_t *best_mask,
                                  int32_t *best_inliers, double *max_iters, double *lo_seen, int32_t *lo_refits, void *stream);
int dr_rigid_magsac_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr2, int P, int M, int N,
                              float *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters,
                              void *stream);
int dr_rigid_magsac_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr2, int P, int M,
                              int N, double *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters,
                              void *stream);
int dr_registration_irls_f32(const float *matches, const float *thr2, int P, int N, int irls_iters, float *best_score,
                             float *best_model, int32_t *irls_fits, void *stream);
int dr_registration_irls_f64(const double *matches, const double *thr2, int P, int N, int irls_iters, double *best_score,
                             double *best_model, int32_t *irls_fits, void *stream);
int dr_kabsch_gather_checked_f32(const float *matches, const int32_t *idx, int P, int B, int N, int k, double edge_similarity,
                                 float *models, uint8_t *valid, int32_t *rejected, void *stream);
int dr_kabsch_gather_checked_f64(const double *matches, const int32_t *idx, int P, int B, int N, int k, double edge_similarity,
                                 double *models, uint8_t *valid, int32_t *rejected, void *stream);
int dr_kabsch_f32(const float *samples, const float *weights, int Bt, int k, float *models, uint8_t *valid, void *stream);
int dr_kabsch_f64(const double *samples, const double *weights, int Bt, int k, double *models, uint8_t *valid, void *stream);
int dr_kabsch_bwd_f32(const float *samples, const float *weights, const float *grad_models, int Bt, int k, float *grad_samples,
                      float *grad_weights, void *stream);
int dr_kabsch_bwd_f64(const double *samples, const double *weights, const double *grad_models, int Bt, int k, double *grad_samples,
                      double *grad_weights, void *stream);
int dr_refit_rigid_bwd_f32(const float *matches, const uint8_t *mask, const float *weights, const float *grad_model, int P, int N,
                           float *grad_matches, float *grad_weights, void *stream);
int dr_refit_rigid_bwd_f64(const double *matches, const uint8_t *mask, const double *weights, const double *grad_model, int P, int N,
                           double *grad_matches, double *grad_weights, void *stream);

/* ------------------------------------------------------------------------------------------
 * Plane-induced homographies (ransac.BatchedHomography).  Not a restatement of upstream code.  matches [P,N,4] = (x1, y1, x2, y2) in
 * the caller's coordinates (pixels; there is no K).  A model [.,9] is the row-major 3x3 H with x2 ~ H x1, stored with unit Frobenius
 * norm and det H > 0.  Residual: y = H (x1, 1), z = adj(H) (x2, 1), d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2 (the symmetric
 * transfer error); a point with y_w <= 0 or z_w <= 0 under the det > 0 sign, or with a non-finite d2, is an outlier and contributes
 * nothing.  The threshold is a DISTANCE and enters as thr2 [P] = threshold^2: inlier iff d2 < thr2, MSAC score =
 * sum_n max(0, 1 - d2_n / thr2).
 *
 *   dr_homography4_gather   idx [P,B,4] int32 -> models [P,B,9], valid [P,B]: the closed form, f64 inside, one lane per sample.  Per
 *     image q_i = x_i - centroid, s = sqrt(2) / mean |q_i|, p_i = (s q_i, 1); D_3 = [q0 q1 q2], D_0 = [q3 q1 q2], D_1 = [q0 q3 q2],
 *     D_2 = [q0 q1 q3] (orientation determinants), lambda_i = D_i / D_3, A = [lambda_0 p0 | lambda_1 p1 | lambda_2 p2];
 *     H = T2^-1 A2 adj(A1) T1, then unit norm and det > 0.  valid = 0, model = identity: an index outside [0, N), a D that is zero or
 *     whose sign differs between the images (three collinear points, a sample point sent through infinity), a non-finite or singular H.
 *   dr_homography4          the same on explicit samples [Bt,4,4]; on samples = matches[idx] the same bits.
 *   dr_homography4_bwd      grad_models [Bt,9] -> grad_samples [Bt,4,4]: the reverse pass of the closed form, through the
 *     normalisation and the unit-norm scaling (a multiple of H in grad_models passes nothing on); the forward is recomputed in f64.
 *     A sample without a valid model, or with a non-finite derivative, gets exact zeros.  Every element is written.
 *   dr_homography_score     models [P,M,9], valid [P,M] or NULL -> scores [P,M], inliers [P,M] int32 (or NULL).  A slot with
 *     valid = 0 scores exactly 0 (0 inliers) and is never evaluated; a non-finite model or one with det == 0 scores NaN (0 inliers).
 *     The det > 0 sign is applied here: a model of negative determinant scores like its negation.  f32 computes in f32 (two
 *     v_rcp_f32 per model and point), f64 in f64.  No [P,M,N] tensor, no atomics, one fixed reduction order: a repeated launch gives
 *     the same bits.  P <= 65535.
 *   dr_homography_update    the state step: for every pair with iters < max_iters, the first arg-max of scores over valid, non-NaN
 *     slots replaces the state only if score > best_score (strict) -- best_score, best_model [P,9], best_mask [P,N] and best_inliers
 *     (the mask's count, by dr_homography_score's expression), max_iters = min(max_iterations, adaptive_iteration_number(inliers, N,
 *     4)) in f64 -- and iters += B.  No qualifying slot: only iters moves.  Terminated pairs are untouched.
 *   dr_refit_homography     the normalised DLT over the rows mask [P,N] selects (NULL = all), weights [P,N] (optional) multiplying a
 *     row's terms in the Gram matrix -> model [P,9], valid [P].  Hartley's transforms come from the selected rows, unweighted; the 9x9
 *     Gram matrix of the two DLT rows per point is summed in f64 in one fixed order; its smallest eigenvector (Jacobi) is denormalised,
 *     scaled to unit norm and given det > 0.  valid = 0, model = identity: fewer than four rows, a non-finite or singular result.
 *   dr_refit_homography_bwd grad_model [P,9] = dL/dH of the model dr_refit_homography returns for (matches, mask, weights) ->
 *     grad_matches [P,N,4] and / or grad_weights [P,N] (NULL: not wanted; at least one; grad_weights with weights = NULL is the
 *     derivative at w = 1).  One 256-thread block per pair, f64 inside; nothing is stored by the forward: the same three passes give
 *     the rows, nz_i = (cx_i, cy_i, s_i) and the Gram matrix G bit for bit, the Jacobi all eigenpairs (lambda_i, v_i), h = v_0.  Then
 *       H = sigma H0 / |H0|, H0 = T2^-1 mat(h) T1:  g0 = (sigma / |H0|) (gH - H <H, gH>) (a multiple of H in grad_model passes nothing
 *         on), g_h = T2^-T g0 T1^T, and the direct gradients of (cx, cy, s) of each image;
 *       z = sum_{i != 0} v_i (v_i . g_h) / (lambda_i - lambda_0), gG = -(z h^T + h z^T) / 2 (the sign of h cancels);
 *       per present row, a = (0, -X, v X), b = (X, 0, -u X), X = (x, y, 1):  grad_weights[n] = a^T gG a + b^T gG b =
 *         -[(a . z)(a . h) + (b . z)(b . h)], and w_n times its derivative by (x, y, u, v) is the normalised-coordinate gradient gx_n;
 *       per image g_c = -s sum gx_n + direct, g_s = sum (gx_n . x_n) / s + direct, s = sqrt(2) R / D, D = sum |q_n|:  g_D = -g_s s / D,
 *         g_c -= g_D sum q_n / |q_n|;  grad_matches[n] = s gx_n + g_D q_n / |q_n| + g_c / R (zero subgradient at |q_n| = 0).
 *     Every element of every requested output is written.  Exact zeros: rows the mask drops (never read: a NaN there reaches nothing),
 *     and every row of a pair with fewer than four rows, valid = 0, lambda_i - lambda_0 not positive and finite, or a non-finite
 *     intermediate (one decision per pair).  No atomics, fixed-order sums: a repeated launch gives the same bits.  Weights are
 *     expected >= 0 and not checked.
 *   dr_homography_magsac_score   dr_homography_score's arguments, slot rules and inlier counts with the MAGSAC++ score in the MSAC
 *     score's place: the transfer error is a 4-vector, so thr2 is read as (k sigma_max)^2 with k^2 = chi2.ppf(0.99, 4), and with
 *     s = d2 / thr2 a point with d2 < thr2 adds 1 - l(s), l the two-view loss stated at dr_magsac_score.  Bit-repeatable.
 *   dr_homography_irls      the IRLS polish of the pair state under that loss (BatchedHomography(scoring = "magsac")), one launch, one
 *     block per pair.  Up to irls_iters (>= 1) times from (best_model [P,9], best_score [P]): the rows = the points with d2 < thr2 in
 *     front of both cameras under the current model, each with the weight w(s) stated at dr_magsac_irls (row decision and weight in
 *     f64 for either type); dr_refit_homography's fit over those rows under those weights; the candidate rounded to the type; its
 *     dr_homography_magsac_score score over all points; taken only on a strictly higher score.  Ends before a fit with fewer than four
 *     rows, on an invalid or non-finite candidate, on a candidate that does not win, at the limit.  irls_fits [P] int32 += fits run.
 *     Mask, inlier count, iters and max_iters of the state are neither read nor written.  No atomics: a repeated launch gives the
 *     same bits.
 * ------------------------------------------------------------------------------------------ */
int dr_homography4_gather_f32(const float *matches, const int32_t *idx, int P, int B, int N, float *models, uint8_t *valid,
                              void *stream);
int dr_homography4_gather_f64(const double *matches, const int32_t *idx, int P, int B, int N, double *models, uint8_t *valid,
                              void *stream);
int dr_homography4_f32(const float *samples, int Bt, float *models, uint8_t *valid, void *stream);
int dr_homography4_f64(const double *samples, int Bt, double *models, uint8_t *valid, void *stream);
int dr_homography4_bwd_f32(const float *samples, const float *grad_models, int Bt, float *grad_samples, void *stream);
int dr_homography4_bwd_f64(const double *samples, const double *grad_models, int Bt, double *grad_samples, void *stream);
int dr_homography_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr2, int P, int M, int N,
                            float *scores, int32_t *inliers, void *stream);
int dr_homography_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr2, int P, int M,
                            int N, double *scores, int32_t *inliers, void *stream);
int dr_homography_update_f32(const float *matches, const float *models, const uint8_t *valid, const float *scores,
                             const float *thr2, int P, int M, int N, int B, double confidence, double eps, int max_iterations,
                             float *best_score, float *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters,
                             double *max_iters, void *stream);
int dr_homography_update_f64(const double *matches, const double *models, const uint8_t *valid, const double *scores,
                             const double *thr2, int P, int M, int N, int B, double confidence, double eps, int max_iterations,
                             double *best_score, double *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters,
                             double *max_iters, void *stream);
int dr_refit_homography_f32(const float *matches, const uint8_t *mask, const float *weights, int P, int N, float *model,
                            uint8_t *valid, void *stream);
int dr_refit_homography_f64(const double *matches, const uint8_t *mask, const double *weights, int P, int N, double *model,
                            uint8_t *valid, void *stream);
int dr_refit_homography_bwd_f32(const float *matches, const uint8_t *mask, const float *weights, const float *grad_model, int P, int N,
                                float *grad_matches, float *grad_weights, void *stream);
int dr_refit_homography_bwd_f64(const double *matches, const uint8_t *mask, const double *weights, const double *grad_model, int P,
                                int N, double *grad_matches, double *grad_weights, void *stream);
int dr_homography_magsac_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr2, int P, int M,
                                   int N, float *scores, int32_t *inliers, void *stream);
int dr_homography_magsac_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr2, int P, int M,
                                   int N, double *scores, int32_t *inliers, void *stream);
int dr_homography_irls_f32(const float *matches, const float *thr2, int P, int N, int irls_iters, float *best_score,
                           float *best_model, int32_t *irls_fits, void *stream);
int dr_homography_irls_f64(const double *matches, const double *thr2, int P, int N, int irls_iters, double *best_score,
                           double *best_model, int32_t *irls_fits, void *stream);

/* ------------------------------------------------------------------------------------------
 * Absolute pose from 2D-3D matches (ransac.BatchedPnP).  Not a restatement of upstream code.  matches [P,N,5] = (X, Y, Z, u, v): a
 * world point and its observation in NORMALISED image coordinates (the caller has applied K^-1; there is no K).  A model [.,16] is the
 * row-major 4x4 [[R, t], [0, 0, 0, 1]] with x_c = R X + t, the layout of the registration entries.  Residual:
 * d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2; a point with z_c <= 0 or a non-finite d2 is an outlier and contributes nothing.  The
 * threshold is a DISTANCE in normalised units (pixels / focal length) and enters as thr2 [P] = threshold^2: inlier iff d2 < thr2, MSAC
 * score = sum_n max(0, 1 - d2_n / thr2).
 *
 *   dr_p3p_gather   idx [P,B,3] int32 -> models [P,4B,16], valid [P,4B]: the closed-form P3P of every sample, f64 inside, one lane per
 *     sample.  Bearings f_i = normalize(u_i, v_i, 1); with the depths s_1 = x s_0, s_2 = v s_0 the law of cosines in the three triangles
 *     (camera centre, two points) gives x = p(v) / q(v) and the quartic p^2 - 2 cos(f_0, f_1) p q + q^2 (1 - (c^2 / b^2) g(v)) = 0
 *     (Grunert's P3P in the Fischler-Bolles ratio form; pnp.hip states p, q, g).  Each real root with positive depths, polished by two
 *     Newton steps on the three distance equations, gives one pose through the orthonormal frames of the world and the camera triangle.
 *     Slots 4 b + j of sample b: the valid ones first, in ascending order of v; a valid slot has R orthonormal with det = +1 and the
 *     three sample points at z_c > 0; every other slot is the identity with valid = 0.  All four are invalid for an index outside
 *     [0, N), coincident or collinear world points, coincident bearings, or no surviving root.  No atomics: bit-repeatable.
 *   dr_pnp_score    models [P,M,16], valid [P,M] or NULL -> scores [P,M], inliers [P,M] int32 (or NULL).  A slot with valid = 0
 *     scores exactly 0 (0 inliers) and is never evaluated; a model with a non-finite entry scores NaN (0 inliers).  f32 computes in
 *     f32 (one v_rcp_f32 per model and point), f64 in f64.  gate_iters / gate_max_iters (both or neither): the blocks of pairs with
 *     iters >= max_iters return at once and the pair's outputs keep their contents.  No [P,M,N] tensor, no atomics, one fixed
 *     reduction order: a repeated launch gives the same bits.  P <= 65535.
 *   dr_pnp_update   dr_homography_update's state step with sample size 3 in the adaptive stop and best_model [P,16]: strict
 *     "better?" test in every round, iters += B (B = samples of the round; M = 4 B slots).
 *   dr_refit_pnp    Levenberg-Marquardt on the reprojection error from init_model [P,16] over the rows mask [P,N] selects (NULL = all)
 *     that lie in front of the camera under the current iterate -> model [P,16], valid [P].  `iters` passes at most; a pass solves
 *     (J^T J + lambda diag(J^T J)) step = -J^T r (f64 sums in one fixed order, Cholesky), the step is a left-multiplied rotation vector
 *     and a translation, taken only on a strictly lower cost over the same row set (lambda / 10, else lambda x 10; from 1e-3).
 *     valid = 0, model = identity: a non-finite start or result, fewer than three such rows under the start.  Bit-repeatable.
 *   dr_p3p          dr_p3p_gather on explicit samples [Bt,3,5] -> models [4 Bt,16], valid [4 Bt] (slots 4 b + j, the same rules); on
 *     samples = matches[idx] the same bits: one device function serves both.  What train mode fits.  Bt < 2^29.
 *   dr_p3p_bwd      grad_models [4 Bt,16] -> grad_samples [Bt,3,5]: the reverse pass of the closed form by the implicit function
 *     theorem.  A valid pose is a root of the six reprojection equations of its three rows; with dr_refit_pnp's left-multiplied step
 *     theta = (w, d) and J = d r / d theta (6x6, the two rows per sample row stated there, at x_c = R X_i + t):
 *         g_theta = (sum_j R[:,j] x G_R[:,j] + t x G_t, G_t),   J^T lambda = g_theta,
 *         grad X_i += -(A_i R)^T lambda_i,   grad (u, v)_i += lambda_i,   A_i = (1 / z_c) [[1, 0, -x], [0, 1, -y]]
 *     per valid slot, at the slot's pose after ONE Gauss-Newton step onto the root of those six equations (J delta = -r, the residual
 *     in two-term arithmetic: the theorem holds at the root, and an ill-conditioned sample turns the forward's few ulp of distance
 *     from it into a gradient error hundreds of times as large; the forward's models are not touched), G = the slot's grad_models (rows 0-2; row 3 is ignored; the part of G_R normal to the rotation manifold passes
 *     nothing on).  One lane per sample recomputes the poses with the forward's device function (no model is saved, the slot order is
 *     the forward's) and adds the valid slots' contributions in slot order, f64 inside.  A slot contributes exact zeros when it is
 *     invalid (its grad_models are never read: NaN there reaches nothing), when a pivot of the LU (partial pivoting) is not larger
 *     than 1e-12 x the largest |entry| of J, or when any of its fifteen results is not finite.  Every output element is written.  No
 *     atomics: bit-repeatable.
 *   dr_refit_pnp_weighted   dr_refit_pnp with weights [P,N] (>= 0, not checked; NULL = 1): the same kernel text and Levenberg-Marquardt
 *     loop, a row's weight multiplying its terms in J^T J, J^T r and both costs, so the result minimises sum_i w_i |r_i|^2 over the
 *     row set.  With weights = NULL it launches dr_refit_pnp's instantiation (the same bits); weights of exactly 1 give those bits
 *     too: the weighted sums are written with fma in the shape the unweighted ones compile to.  The MASK is the selection, the
 *     weights are not: a row with w_i = 0 still counts towards the three-row rule (and adds exact zeros to every sum), so a pair
 *     whose positive weights sit on fewer than three rows returns its start with valid = 1, the damped matrix never becoming
 *     positive definite.
 *   dr_refit_pnp_bwd   model [P,16] (what the forward returned), grad_model [P,16] -> grad_matches [P,N,5] and / or grad_weights
 *     [P,N] (either may be NULL, not both): the reverse pass of the weighted fit by the implicit function theorem at the stationary
 *     point g = sum w_i J_i^T r_i = 0, in the chart theta = (w, d) of the left-multiplied step.  With x_c = R X_i + t,
 *     V = [-[x_c]x | I], p = D pi^T r and B = D pi^T D pi + r . D^2 pi (the gradient and Hessian of |r|^2 / 2 in x_c):
 *         H = sum w_i (V^T B V + [[sym(p x_c^T), 0], [0, 0]])    (the full 6x6 Hessian, not J^T J),
 *         g_theta = (sum_j R[:,j] x G_R[:,j] + t x G_t, G_t)     (rows 0-2 of grad_model; row 3 is not read),
 *         H lambda = g_theta by Cholesky,   v = lambda_w x x_c + lambda_d,   phi_i = p . v,
 *         grad w_i = -phi_i,   grad (u, v)_i = w_i D pi v,   grad X_i = -w_i R^T (B v + p x lambda_w).
 *     Before that the pose takes two Newton steps theta = -H^-1 g with this H in f64 (each only if H is positive definite and the
 *     step finite): the forward stops `iters` passes in its type's rounding away from the root the theorem needs.  `model` is not
 *     written.  The row set -- the mask's rows with z_c > 0 and a finite residual under `model` -- is a constant of the derivative.
 *     Exact zeros: rows the mask drops (never read: a NaN there reaches nothing), rows outside the row set, and every row of a pair
 *     with fewer than three rows in the set, a non-finite model, an H that is not positive definite, any non-finite result, or a
 *     row of the set that a Newton step puts behind the camera.
 *     Every output element is written once.  One 256-thread block per pair, four reduction sweeps and one write sweep over its rows;
 *     no atomics: bit-repeatable.
 *   dr_pnp_dlt      the weighted normalised DLT: a pose from six or more rows without a start model.  World points under Hartley's
 *     normalisation (weighted centroid, mean distance sqrt 3), two equations per row, the 12x12 Gram matrix from 40 distinct f64
 *     block sums (four symmetric 4x4 blocks), its smallest eigenvector by cyclic Jacobi in f64, refined by one first-order step with
 *     A^T (A h) summed over the rows (the Gram matrix alone leaves it at the square of the equations' conditioning) -> [M | m]; the sign puts the weighted
 *     majority of the rows in front of the camera, R = the rotation nearest to M, t = m / M's mean singular value.  valid = 0,
 *     model = identity: fewer than six rows under the mask (a row of weight 0 counts), a non-finite sum or result, no positive total
 *     weight, or a smallest eigenvalue that is not simple, lambda_1 - lambda_0 <= 1e-10 lambda_max -- a coplanar world set (its null
 *     space has four dimensions; rounding leaves 1e-16 .. 1e-14 there) and anything flat to 1e-5 of its extent: such a pair needs a
 *     start model from the caller.  Forward only.  Bit-repeatable.
 * ------------------------------------------------------------------------------------------ */
int dr_p3p_gather_f32(const float *matches, const int32_t *idx, int P, int B, int N, float *models, uint8_t *valid, void *stream);
int dr_p3p_gather_f64(const double *matches, const int32_t *idx, int P, int B, int N, double *models, uint8_t *valid, void *stream);
int dr_pnp_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr2, int P, int M, int N,
                     float *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_pnp_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr2, int P, int M, int N,
                     double *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_pnp_update_f32(const float *matches, const float *models, const uint8_t *valid, const float *scores, const float *thr2, int P,
                      int M, int N, int B, double confidence, double eps, int max_iterations, float *best_score, float *best_model,
                      uint8_t *best_mask, int32_t *best_inliers, int32_t *iters, double *max_iters, void *stream);
int dr_pnp_update_f64(const double *matches, const double *models, const uint8_t *valid, const double *scores, const double *thr2,
                      int P, int M, int N, int B, double confidence, double eps, int max_iterations, double *best_score,
                      double *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters, double *max_iters, void *stream);
int dr_refit_pnp_f32(const float *matches, const uint8_t *mask, const float *init_model, int P, int N, int iters, float *model,
                     uint8_t *valid, void *stream);
int dr_refit_pnp_f64(const double *matches, const uint8_t *mask, const double *init_model, int P, int N, int iters, double *model,
                     uint8_t *valid, void *stream);
int dr_p3p_f32(const float *samples, int Bt, float *models, uint8_t *valid, void *stream);
int dr_p3p_f64(const double *samples, int Bt, double *models, uint8_t *valid, void *stream);
int dr_p3p_bwd_f32(const float *samples, const float *grad_models, int Bt, float *grad_samples, void *stream);
int dr_p3p_bwd_f64(const double *samples, const double *grad_models, int Bt, double *grad_samples, void *stream);
int dr_refit_pnp_weighted_f32(const float *matches, const uint8_t *mask, const float *weights, const float *init_model, int P, int N,
                              int iters, float *model, uint8_t *valid, void *stream);
int dr_refit_pnp_weighted_f64(const double *matches, const uint8_t *mask, const double *weights, const double *init_model, int P, int N,
                              int iters, double *model, uint8_t *valid, void *stream);
int dr_refit_pnp_bwd_f32(const float *matches, const uint8_t *mask, const float *weights, const float *model, const float *grad_model,
                         int P, int N, float *grad_matches, float *grad_weights, void *stream);
int dr_refit_pnp_bwd_f64(const double *matches, const uint8_t *mask, const double *weights, const double *model,
                         const double *grad_model, int P, int N, double *grad_matches, double *grad_weights, void *stream);
int dr_pnp_dlt_f32(const float *matches, const uint8_t *mask, const float *weights, int P, int N, float *model, uint8_t *valid,
                   void *stream);
int dr_pnp_dlt_f64(const double *matches, const uint8_t *mask, const double *weights, int P, int N, double *model, uint8_t *valid,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * The training loss of the registration path (loss.RegistrationLoss).  Not a restatement of upstream code: RANSACLayer3D's own loss
 * (model_cl.py:586-589) is the mean squared residual over ALL points, which dr_rigid_residual already reproduces.  matches, models,
 * thr2 as above; mask [P,N] (the ground-truth inliers; NULL = all points), keep [P,M] (NULL = all models).  With r = R p + t - q:
 *     d2[p,m,n]   = |r|^2,   e[p,m,n] = d2 < thr2[p] ? d2 / thr2[p] : 1        (strict <, the inlier test of dr_rigid_msac_score)
 *     sums[p,m]   = sum_{n in mask} e[p,m,n]                                    (#mask_p - sums = the MSAC score on the masked points)
 *     per_pair[p] = sum_{m kept} sums[p,m] / max(#kept_p #mask_p, 1),   coef[p] = 1 / max(#kept_p #mask_p, 1),   mean = sum_p per_pair / P
 *     d sums / d R = (2 / thr2) sum r p^T,   d sums / d t = (2 / thr2) sum r     over the masked points with d2 < thr2
 * The truncated branch and d2 == thr2 pass no gradient; the last row of a 4x4 gradient is written as zeros.  A slot keep drops is
 * skipped (sums 0, gradient 0, its model is not read: it may be NaN); a kept model with a non-finite entry has sums = #mask_p and a
 * zero gradient; a pair with an empty mask or no kept model has per_pair 0 and zero gradients.  Every output element is written; no
 * floating-point atomics and one fixed order for every sum (ascending points per model, lanes then waves in the reduction), so a
 * repeated launch gives the same bits.  Sums are accumulated in the type of the inputs: sums[p,m] is evaluated as
 * (sum of the d2 below thr2) x (1 / thr2) + (number of masked points at or above it), one rounding of the quotient per model and not
 * one per point, and d2 as |q - t - R p|^2 started from q - t, so neither is dr_rigid_msac_score's value to the last bit.  A thr2[p]
 * that is not > 0 (NaN included) leaves no point below it: sums = #mask_p for every kept model of the pair and zero gradients.
 * P <= 65535 and P M < 2^22 (the per-pair / mean reduction is one block).
 *
 *   dr_registration_loss_fused   sums [P,M], grad_unscaled [P,M,16] = d sums[p,m] / d model, per_pair [P], coef [P], mean [1]: value and
 *     gradient from one pass over the (model x point) grid (two launches: the grid, then the per-pair / mean reduction).
 *   dr_registration_loss_scale   grad_models = grad_unscaled x coef[p] x grad_mean[0] / P: the whole backward of the mean.
 *   dr_registration_loss_fwd     the value only (sums, per_pair, coef, mean).
 *   dr_registration_gt_mask      gt_pose [P,16] -> mask [P,N] = (d2 < thr2[p]) under the pair's pose, count [P] int32.
 * ------------------------------------------------------------------------------------------ */
int dr_registration_loss_fused_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                   const float *thr2, int P, int M, int N, float *sums, float *grad_unscaled, float *per_pair,
                                   float *coef, float *mean, void *stream);
int dr_registration_loss_fused_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                   const double *thr2, int P, int M, int N, double *sums, double *grad_unscaled, double *per_pair,
                                   double *coef, double *mean, void *stream);
int dr_registration_loss_scale_f32(const float *grad_unscaled, const float *coef, const float *grad_mean, int P, int M,
                                   float *grad_models, void *stream);
int dr_registration_loss_scale_f64(const double *grad_unscaled, const double *coef, const double *grad_mean, int P, int M,
                                   double *grad_models, void *stream);
int dr_registration_loss_fwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2,
                                 int P, int M, int N, float *sums, float *per_pair, float *coef, float *mean, void *stream);
int dr_registration_loss_fwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                 const double *thr2, int P, int M, int N, double *sums, double *per_pair, double *coef, double *mean,
                                 void *stream);
int dr_registration_gt_mask_f32(const float *matches, const float *gt_pose, const float *thr2, int P, int N, uint8_t *mask,
                                int32_t *count, void *stream);
int dr_registration_gt_mask_f64(const double *matches, const double *gt_pose, const double *thr2, int P, int N, uint8_t *mask,
                                int32_t *count, void *stream);

/* ------------------------------------------------------------------------------------------
 * The training loss of the homography path (loss.HomographyLoss): the registration loss above on the symmetric transfer error.
 * matches [P,N,4], models [P,M,9] (ANY scale and either sign: d2 does not change under a positive scaling of H, and the det > 0
 * sign is applied here), thr2 [P] as for dr_homography_score; mask [P,N] (the ground-truth inliers; NULL = all points), keep [P,M]
 * (NULL = all models).  With h = sign(det H) H, a = adj(H), y = h (x1, 1), z = a (x2, 1), e = x2 - y_xy / y_w, f = x1 - z_xy / z_w:
 *     d2[p,m,n]   = |e|^2 + |f|^2,   live = y_w > 0 and z_w > 0 and d2 < thr2[p]   (strict; false for a NaN),   term = live ? d2 / thr2[p] : 1
 *     sums[p,m]   = sum_{n in mask} term[p,m,n]
 *     per_pair[p] = sum_{m kept} sums[p,m] / max(#kept_p #mask_p, 1),   coef[p] = 1 / max(#kept_p #mask_p, 1),   mean = sum_p per_pair / P
 *     d sums / d h = (2 / thr2) sum (1 / y_w) (-e_0, -e_1, e . y_xy / y_w) (x1, 1)^T,   d sums / d a = the same with f, z, x2, over the live
 *     points;   d sums / d H = sign(det H) (d sums / d h + J^T d sums / d a),  J = d adj(h) / d h (linear in h: applied once per model)
 * so <d sums / d H, H> = 0 up to rounding.  A point behind either camera, at or beyond the threshold or with a NaN distance counts 1
 * and passes no gradient.  A slot keep drops is skipped (sums 0, gradient 0, its model is not read: it may be NaN); a kept model with
 * a non-finite entry, det == 0 or a non-finite determinant (dr_homography_score's NaN-scoring slots) has sums = #mask_p and a zero
 * gradient; a pair with an empty mask or no kept model has per_pair 0 and zero gradients; a thr2[p] that is not > 0 (NaN included)
 * leaves no point below it.  Every output element is written; no floating-point atomics and one fixed order for every sum
 * (ascending points per model, lanes then waves in the reduction), so a repeated launch gives the same bits, and H and -H give the
 * same sums and negated gradients bit for bit.  Sums are accumulated in the type of the inputs, sums[p,m] as (sum of the live d2) x
 * (1 / thr2) + (number of masked points that are not live).  The f32 reciprocals of y_w and z_w are v_rcp_f32 with one Newton step
 * (the gradient is a sum of e / y_w terms), so d2 is dr_homography_score's up to the reciprocal's ulp and `live` is its inlier test
 * wherever the two roundings cannot decide otherwise.  P <= 65535 and P M < 2^22 (the per-pair / mean reduction is one block).
 *
 *   dr_homography_loss_fused   sums [P,M], grad_unscaled [P,M,9] = d sums[p,m] / d H, per_pair [P], coef [P], mean [1]: value and
 *     gradient from one pass over the (model x point) grid (two launches: the grid, then the per-pair / mean reduction).
 *   dr_homography_loss_scale   grad_models = grad_unscaled x coef[p] x grad_mean[0] / P: the whole backward of the mean.
 *   dr_homography_loss_fwd     the value only (sums, per_pair, coef, mean), the same bits as the fused form's.
 *   dr_homography_gt_mask      gt_H [P,9] -> mask [P,N] = dr_homography_score's inlier test under the pair's homography (bit for bit the
 *     mask dr_homography_update writes for that model; all zeros for a NaN-scoring one), count [P] int32.
 * ------------------------------------------------------------------------------------------ */
int dr_homography_loss_fused_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                 const float *thr2, int P, int M, int N, float *sums, float *grad_unscaled, float *per_pair,
                                 float *coef, float *mean, void *stream);
int dr_homography_loss_fused_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                 const double *thr2, int P, int M, int N, double *sums, double *grad_unscaled, double *per_pair,
                                 double *coef, double *mean, void *stream);
int dr_homography_loss_scale_f32(const float *grad_unscaled, const float *coef, const float *grad_mean, int P, int M,
                                 float *grad_models, void *stream);
int dr_homography_loss_scale_f64(const double *grad_unscaled, const double *coef, const double *grad_mean, int P, int M,
                                 double *grad_models, void *stream);
int dr_homography_loss_fwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2,
                               int P, int M, int N, float *sums, float *per_pair, float *coef, float *mean, void *stream);
int dr_homography_loss_fwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                               const double *thr2, int P, int M, int N, double *sums, double *per_pair, double *coef, double *mean,
                               void *stream);
int dr_homography_gt_mask_f32(const float *matches, const float *gt_H, const float *thr2, int P, int N, uint8_t *mask,
                              int32_t *count, void *stream);
int dr_homography_gt_mask_f64(const double *matches, const double *gt_H, const double *thr2, int P, int N, uint8_t *mask,
                              int32_t *count, void *stream);

/* ------------------------------------------------------------------------------------------
 * The training loss of the absolute-pose path (loss.PnPLoss): the registration loss above on the reprojection error.  matches
 * [P,N,5], models [P,M,16], thr2 [P] as for dr_pnp_score; mask [P,N] (the ground-truth inliers; NULL = all points), keep [P,M]
 * (NULL = all models).  With x_c = R X + t, i = 1 / z_c, (x, y) = (x_c, y_c) i, e = (x - u, y - v):
 *     d2[p,m,n]   = |e|^2,   live = z_c > 0 and d2 < thr2[p]   (strict; false for a NaN),   term = live ? d2 / thr2[p] : 1
 *     sums[p,m]   = sum_{n in mask} term[p,m,n]
 *     per_pair[p] = sum_{m kept} sums[p,m] / max(#kept_p #mask_p, 1),   coef[p] = 1 / max(#kept_p #mask_p, 1),   mean = sum_p per_pair / P
 *     h = (2 / thr2) (e_0 i, e_1 i, -(e_0 x + e_1 y) i),   d sums / d t = sum h,   d sums / d R = sum h X^T   over the live points; row 3 = 0
 * A point behind the camera, at or beyond the threshold or with a NaN distance counts 1 and passes no gradient.  A slot keep drops is
 * skipped (sums 0, gradient 0, its model is not read: it may be NaN); a kept model with a non-finite entry among its twelve has
 * sums = #mask_p and a zero gradient; a pair with an empty mask or no kept model has per_pair 0 and zero gradients; a thr2[p] that is
 * not > 0 (NaN included) leaves no point below it.  Every output element is written; no floating-point atomics and one fixed order
 * for every sum, so a repeated launch gives the same bits.  Sums are accumulated in the type of the inputs.  1 / z_c is a division
 * (correctly rounded), not dr_pnp_score's v_rcp_f32: d2 is the score's up to that ulp, and `live` is its inlier test wherever the two
 * roundings cannot decide otherwise.  P <= 65535 and P M < 2^22.  No gradient is computed for the matches.
 *
 *   dr_pnp_loss_fused   sums [P,M], grad_unscaled [P,M,16] = d sums[p,m] / d model, per_pair [P], coef [P], mean [1]: value and
 *     gradient from one pass over the (model x point) grid (two launches: the grid, then the per-pair / mean reduction).
 *   dr_pnp_loss_scale   grad_models = grad_unscaled x coef[p] x grad_mean[0] / P: the whole backward of the mean.
 *   dr_pnp_loss_fwd     the value only (sums, per_pair, coef, mean), the same bits as the fused form's.
 *   dr_pnp_gt_mask      gt_pose [P,16] -> mask [P,N] = dr_pnp_score's inlier test under the pair's pose (bit for bit the mask
 *     dr_pnp_update writes for that model; all zeros for a non-finite one), count [P] int32.
 * ------------------------------------------------------------------------------------------ */
int dr_pnp_loss_fused_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2,
                          int P, int M, int N, float *sums, float *grad_unscaled, float *per_pair, float *coef, float *mean,
                          void *stream);
int dr_pnp_loss_fused_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep, const double *thr2,
                          int P, int M, int N, double *sums, double *grad_unscaled, double *per_pair, double *coef, double *mean,
                          void *stream);
int dr_pnp_loss_scale_f32(const float *grad_unscaled, const float *coef, const float *grad_mean, int P, int M, float *grad_models,
                          void *stream);
int dr_pnp_loss_scale_f64(const double *grad_unscaled, const double *coef, const double *grad_mean, int P, int M, double *grad_models,
                          void *stream);
int dr_pnp_loss_fwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2, int P,
                        int M, int N, float *sums, float *per_pair, float *coef, float *mean, void *stream);
int dr_pnp_loss_fwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep, const double *thr2,
                        int P, int M, int N, double *sums, double *per_pair, double *coef, double *mean, void *stream);
int dr_pnp_gt_mask_f32(const float *matches, const float *gt_pose, const float *thr2, int P, int N, uint8_t *mask, int32_t *count,
                       void *stream);
int dr_pnp_gt_mask_f64(const double *matches, const double *gt_pose, const double *thr2, int P, int N, uint8_t *mask, int32_t *count,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * The differentiable soft-inlier score of the absolute-pose path (ops.pnp_soft_score, loss.PnPExpectedLoss): the DSAC score of every
 * pose on every point, with a reverse pass to the poses and to the points.  matches [P,N,5], models [P,M,16], thr2 [P], mask [P,N]
 * (the points that are scored; NULL = all), keep [P,M] (NULL = all models) as for dr_pnp_loss_*; beta > 0 by value.  With the loss's
 * residual, x_c = R X + t, i = 1 / z_c (a division, correctly rounded), (x, y) = (x_c, y_c) i, e = (x - u, y - v):
 *     d2[p,m,n]  = |e|^2,   a = beta (1 - d2 / thr2[p]),   live = z_c > 0 and d2 finite and a >= -40
 *     w          = live ? 1 / (1 + exp(-a)) : 0,           scores[p,m] = sum_{n in mask} w[p,m,n]
 * (weight 1/2 at the threshold, 1 / (1 + exp(-beta)) at zero residual; the SQUARED error, the package's convention, where DSAC* takes
 * the error itself).  The cutoff a < -40 (w < 4.3e-18) is part of the definition: it makes every w (1 - w) / z_c term of the
 * gradient an exact zero, never 0 x inf.  With g = grad_scores[p,m] (-beta / thr2[p]) w (1 - w) and h = (e_0 i, e_1 i, -(e_0 x + e_1 y) i):
 *     grad_models[p,m]:   d / d t = sum_n 2 g h,   d / d R = sum_n 2 g h X^T   over the masked points, row 3 = 0
 *     grad_matches[p,n]:  d / d X = sum_m R^T (2 g h),   d / d (u, v) = sum_m -2 g e   over the kept models
 * A slot keep drops is never read (score 0, gradient exactly 0, its model and its grad_scores may be NaN); a kept model with a
 * non-finite entry among its twelve scores 0 and passes exact zeros to itself and to the points; a thr2[p] that is not > 0 (NaN
 * included) gives the pair score 0 and zero gradients; a point outside the mask gets exact zeros.  Every output element is written.
 * No floating-point atomics, no workspace, and one order for every sum that depends on (P, M, N) alone: a repeated launch gives the
 * same bits.  e = (x_c - u z_c, y_c - v z_c) / z_c with the numerators formed beyond the type's precision (f32: in f64; f64: a
 * compensated dot product) and rounded once: the cancellation in e costs no digits.  The gradients are accumulated in the type of
 * the inputs, the score with a compensated (TwoSum) sum in it.  P <= 65535 and P M < 2^22.  No gradient for thr2 or beta.
 *
 *   dr_pnp_soft_score       scores [P,M]: one lane per model, the points in ascending order.
 *   dr_pnp_soft_score_bwd   grad_scores [P,M] -> grad_models [P,M,16] (the forward's mapping) and, unless grad_matches is NULL,
 *     grad_matches [P,N,5] by a second launch with the transposed mapping (one lane per point; the models in tiles of 512, every
 *     eighth of a tile summed by its own wave, the eight partial sums added in order).  Both recompute the residuals.
 * ------------------------------------------------------------------------------------------ */
int dr_pnp_soft_score_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2,
                          float beta, int P, int M, int N, float *scores, void *stream);
int dr_pnp_soft_score_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep, const double *thr2,
                          double beta, int P, int M, int N, double *scores, void *stream);
int dr_pnp_soft_score_bwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep, const float *thr2,
                              float beta, const float *grad_scores, int P, int M, int N, float *grad_models, float *grad_matches,
                              void *stream);
int dr_pnp_soft_score_bwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                              const double *thr2, double beta, const double *grad_scores, int P, int M, int N, double *grad_models,
                              double *grad_matches, void *stream);

/* ------------------------------------------------------------------------------------------
 * The differentiable soft-inlier score of the registration path (ops.registration_soft_score, loss.RegistrationExpectedLoss): the
 * DSAC score of every rigid model on every correspondence, with a reverse pass to the models and to the points.  matches [P,N,6] =
 * (p, q), models [P,M,16] = [[R, t], [0,0,0,1]], thr2 [P], mask [P,N] (the points that are scored; NULL = all), keep [P,M] (NULL =
 * all models) as for dr_registration_loss_*; beta > 0 by value.
 *     d = R p + t - q,   d2[p,m,n] = |d|^2,   a = beta (1 - d2 / thr2[p]),   live = d2 finite and a >= -40
 *     w = live ? 1 / (1 + exp(-a)) : 0,       scores[p,m] = sum_{n in mask} w[p,m,n]
 * (weight 1/2 at the threshold, 1 / (1 + exp(-beta)) at zero distance; the SQUARED distance, the package's convention).  The cutoff
 * a < -40 (w < 4.3e-18) is part of the definition, as for dr_pnp_soft_score.  With g = 2 grad_scores[p,m] (-beta / thr2[p]) w (1 - w)
 * per live term:
 *     grad_models[p,m]:   d / d t = sum_n g d,   d / d R = sum_n g d p^T   over the masked points, row 3 = 0
 *     grad_matches[p,n]:  d / d p = sum_m R^T (g d),   d / d q = sum_m -g d   over the kept models
 * A slot keep drops is never read (score 0, gradient exactly 0, its model and its grad_scores may be NaN); a kept model with a
 * non-finite entry among its twelve scores 0 and passes exact zeros to itself and to the points; a thr2[p] that is not > 0 (NaN
 * included) gives the pair score 0 and zero gradients; a point outside the mask gets exact zeros.  Every output element is written.
 * No floating-point atomics, no workspace, and one order for every sum that depends on (P, M, N) alone: a repeated launch gives the
 * same bits.  d is formed beyond the type's precision (f32: in f64; f64: a compensated dot product and TwoSum) and rounded once: its
 * cancellation costs no digits.  The gradients are accumulated in the type of the inputs, the score with a compensated (TwoSum) sum
 * in it.  P <= 65535 and P M < 2^22.  No gradient for thr2 or beta.
 *
 *   dr_registration_soft_score       scores [P,M]: one lane per model, the points in ascending order.
 *   dr_registration_soft_score_bwd   grad_scores [P,M] -> grad_models [P,M,16] (the forward's mapping) and, unless grad_matches is
 *     NULL, grad_matches [P,N,6] by a second launch with the transposed mapping (one lane per point; the models in tiles of 512,
 *     every eighth of a tile summed by its own wave, the eight partial sums added in order).  Both recompute the residuals.
 * ------------------------------------------------------------------------------------------ */
int dr_registration_soft_score_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                   const float *thr2, float beta, int P, int M, int N, float *scores, void *stream);
int dr_registration_soft_score_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                   const double *thr2, double beta, int P, int M, int N, double *scores, void *stream);
int dr_registration_soft_score_bwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                       const float *thr2, float beta, const float *grad_scores, int P, int M, int N,
                                       float *grad_models, float *grad_matches, void *stream);
int dr_registration_soft_score_bwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                       const double *thr2, double beta, const double *grad_scores, int P, int M, int N,
                                       double *grad_models, double *grad_matches, void *stream);

/* ------------------------------------------------------------------------------------------
 * The differentiable soft-inlier score of the homography path (ops.homography_soft_score, loss.HomographyExpectedLoss): the DSAC
 * score of every homography on every match, with a reverse pass to the models and to the matches.  matches [P,N,4] = (x1, y1, x2,
 * y2), models [P,M,9], thr2 [P], mask [P,N] (the points that are scored; NULL = all), keep [P,M] (NULL = all models) as for
 * dr_homography_loss_*; beta > 0 by value.  With the loss's residual,
 *     h = sign(det H) H,  A = adj(H),  y = h (x1, 1),  z = A (x2, 1),  e = x2 - y_xy / y_w,  f = x1 - z_xy / z_w:
 *     d2[p,m,n] = |e|^2 + |f|^2,   a = beta (1 - d2 / thr2[p]),   live = y_w > 0 and z_w > 0 and d2 finite and a >= -40
 *     w = live ? 1 / (1 + exp(-a)) : 0,                            scores[p,m] = sum_{n in mask} w[p,m,n]
 * (weight 1/2 at the threshold, 1 / (1 + exp(-beta)) at zero error; the SQUARED error, the package's convention; the score does not
 * depend on the scale or the sign of a model).  The cutoff a < -40 (w < 4.3e-18) is part of the definition, as for
 * dr_pnp_soft_score.  With g = grad_scores[p,m] (-beta / thr2[p]) w (1 - w) per live term, t = y_xy / y_w,
 * d d2 / d y = (2 / y_w) (-e_0, -e_1, e . t), and the same for z, f and A:
 *     grad_models[p,m]  = sign(det H) sum_n g (d d2 / d y (x1, 1)^T + J_adj(h)^T [d d2 / d z (x2, 1)^T])   over the masked points
 *     grad_matches[p,n] = sum_m g (2 f + h[:, :2]^T d d2 / d y,  2 e + A[:, :2]^T d d2 / d z)               over the kept models
 * A slot keep drops is never read (score 0, gradient exactly 0, its model and its grad_scores may be NaN); a kept model with a
 * non-finite entry, with det == 0 or with a non-finite det scores 0 and passes exact zeros to itself and to the points; a thr2[p]
 * that is not > 0 (NaN included) gives the pair score 0 and zero gradients; a point outside the mask gets exact zeros.  Every output
 * element is written.  No floating-point atomics, no workspace, and one order for every sum that depends on (P, M, N) alone: a
 * repeated launch gives the same bits.  e and f are formed beyond the type's precision and rounded once (f32: adj(H), y, z, the
 * reciprocals and the quotients in f64; f64: every linear form and adjugate entry as a compensated hi + lo, the quotient corrected
 * by its remainder): their cancellation costs no digits.  1 - w is formed as exp(-a) w.  The gradients are accumulated in the type
 * of the inputs, the score with a compensated (TwoSum) sum in it.  P <= 65535 and P M < 2^22.  No gradient for thr2 or beta.
 *
 *   dr_homography_soft_score       scores [P,M]: one lane per model, the points in ascending order.
 *   dr_homography_soft_score_bwd   grad_scores [P,M] -> grad_models [P,M,9] (the forward's mapping; the two outer-product sums apart,
 *     the adjugate's transposed Jacobian applied once per model) and, unless grad_matches is NULL, grad_matches [P,N,4] by a second
 *     launch with the transposed mapping (one lane per point; the models in tiles of 256, every eighth of a tile summed by its own
 *     wave, the eight partial sums added in order).  Both recompute the residuals.
 * ------------------------------------------------------------------------------------------ */
int dr_homography_soft_score_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                 const float *thr2, float beta, int P, int M, int N, float *scores, void *stream);
int dr_homography_soft_score_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                 const double *thr2, double beta, int P, int M, int N, double *scores, void *stream);
int dr_homography_soft_score_bwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *keep,
                                     const float *thr2, float beta, const float *grad_scores, int P, int M, int N,
                                     float *grad_models, float *grad_matches, void *stream);
int dr_homography_soft_score_bwd_f64(const double *matches, const uint8_t *mask, const double *models, const uint8_t *keep,
                                     const double *thr2, double beta, const double *grad_scores, int P, int M, int N,
                                     double *grad_models, double *grad_matches, void *stream);

/* ------------------------------------------------------------------------------------------
 * K5  train-mode best-of-S selection    RANSAC.__call__, ransac.py:87-96
 *   chosen[p,b] = models[p,b,argmin_s ||models[p,b,s] - gt[p]||_F]; invalid slots (valid == 0) are
 *   skipped; which [P*B] int32 (-1 when no slot is valid; chosen = eye(3) then).
 * ------------------------------------------------------------------------------------------ */
/* keep [P*B] uint8 (optional, NULL = not wanted) = (which >= 0): the `nan_filter` of ransac.py:104-106 as a flag the loss consumes
 * (round 6: the `_keep` twin of round 3 folded in). */
int dr_select_closest_f32(const float *models, const uint8_t *valid, const float *gt, int P, int B, int S,
                          float *chosen, int32_t *which, uint8_t *keep, void *stream);
int dr_select_closest_f64(const double *models, const uint8_t *valid, const double *gt, int P, int B, int S,
                          double *chosen, int32_t *which, uint8_t *keep, void *stream);
/* backward: grad_models [P,B,S,9] = grad_chosen [P,B,9] at slot which[p,b], 0 elsewhere (all of it is written). */
int dr_select_closest_bwd_f32(const float *grad_chosen, const int32_t *which, int P, int B, int S, float *grad_models,
                              void *stream);
int dr_select_closest_bwd_f64(const double *grad_chosen, const int32_t *which, int P, int B, int S, double *grad_models,
                              void *stream);

/* ------------------------------------------------------------------------------------------
 * K6  test-mode selection      RANSAC.__call__, ransac.py:111-120
 *   Per pair: best_idx = first arg-max of scores over valid models (NaN scores never win),
 *   best_score, best_mask [P,N] uint8 recomputed for the winning model, inlier count.
 *   valid may be NULL (all valid).
 * ------------------------------------------------------------------------------------------ */
int dr_select_best_f32(const float *matches, const float *models, const uint8_t *valid, const float *scores,
                       const float *thr, int P, int M, int N, int32_t *best_idx, float *best_score,
                       float *best_model, uint8_t *best_mask, int32_t *inliers, void *stream);
int dr_select_best_f64(const double *matches, const double *models, const uint8_t *valid, const double *scores,
                       const double *thr, int P, int M, int N, int32_t *best_idx, double *best_score,
                       double *best_model, uint8_t *best_mask, int32_t *inliers, void *stream);

/* K6 set-up: threshold normalisation of ransac.py:49-53 and the initial per-pair state, one launch.
 *   K1, K2: calibration matrices, [3,3] shared by all pairs (k_stride 0) or [P,3,3] (k_stride 9), or both NULL
 *   (fundamental-matrix mode / threshold already normalised: thr[p] = threshold).  Otherwise
 *   thr[p] = threshold / ((K1[0,0] + K1[1,1] + K1[0,0] + K2[1,1]) / 4)  -- sic, ransac.py:52.
 *   State: best_score = 0, best_model = eye(3), best_mask = 0, best_inliers = 0, iters = 0, max_iters = max_iterations.
 *   seed_state / seeds_out / n_seeds (optional, NULL / 0 = none; round 6): the call's sampler keys from the same launch --
 *   dr_seed_next_n(seed_state, seeds_out, n_seeds), one node fewer in a replayed call.
 *   race_logits [P,N] f32 / race_ws ((N + 32) * P floats; optional, both or neither): the per-pair weights of the one-logarithm
 *   sampler (dr_gumbel_topk_gather_f32's race_ws) from the same launch, once per call: pass the workspace to the sampler with
 *   race_ready = 1. */
int dr_ransac_init_f32(const float *K1, const float *K2, int k_stride, double threshold, int P, int N,
                       int max_iterations, float *thr, float *best_score, float *best_model, uint8_t *best_mask,
                       int32_t *best_inliers, int32_t *iters, double *max_iters, uint64_t *seed_state, uint64_t *seeds_out,
                       int n_seeds, const float *race_logits, float *race_ws, void *stream);
int dr_ransac_init_f64(const double *K1, const double *K2, int k_stride, double threshold, int P, int N,
                       int max_iterations, double *thr, double *best_score, double *best_model, uint8_t *best_mask,
                       int32_t *best_inliers, int32_t *iters, double *max_iters, uint64_t *seed_state, uint64_t *seeds_out,
                       int n_seeds, const float *race_logits, float *race_ws, void *stream);

/* K6 (batched, state on the device)  RANSAC.__call__ ransac.py:109-144 + adaptive_iteration_number :202-215.
 *   For every pair p with iters[p] < max_iters[p] (the others have terminated and are left untouched):
 *     b = first arg-max of scores[p] over valid, non-NaN models;
 *     if scores[p,b] > best_score[p] or iters[p] == 0:  best_score / best_model [P,9] / best_mask [P,N] /
 *         best_inliers <- model b (mask recomputed), max_iters[p] = min(max_iterations,
 *         log10(1-confidence) / log10(1 - (inliers/N)^k + eps))   (computed in f64);
 *     iters[p] += B.
 *   The caller initialises best_score = 0, iters = 0, max_iters = max_iterations (dr_ransac_init does).
 *   k is the exponent of the stop: the estimator's sample_size (ransac.py:204-215; 5 for E, 7 for the F estimator), which
 *   is not the sampler's points per sample (8 for the 8-point F sampler and for `num_samples = 8`).
 *   sub_models (round 6): 0 (or >= M) = the M models are one batch of B hypotheses.  0 < sub_models < M: they are ceil(M / sub_models)
 *   consecutive sub-batches of B hypotheses each (at most 512), and the steps above are applied to one sub-batch after the other, IN
 *   ORDER, stopping as the loop of ransac.py:55 does when iters[p] >= max_iters[p]: the state after the launch is the state that loop
 *   reaches on the same hypotheses batch by batch -- the reference's `-rbs 64` costs the launches of `-rbs 1024`. */
int dr_ransac_update_f32(const float *matches, const float *models, const uint8_t *valid, const float *scores,
                         const float *thr, int P, int M, int N, int B, int k, double confidence, double eps,
                         int max_iterations, float *best_score, float *best_model, uint8_t *best_mask,
                         int32_t *best_inliers, int32_t *iters, double *max_iters, int sub_models, void *stream);
int dr_ransac_update_f64(const double *matches, const double *models, const uint8_t *valid, const double *scores,
                         const double *thr, int P, int M, int N, int B, int k, double confidence, double eps,
                         int max_iterations, double *best_score, double *best_model, uint8_t *best_mask,
                         int32_t *best_inliers, int32_t *iters, double *max_iters, int sub_models, void *stream);

/* ------------------------------------------------------------------------------------------
 * K7  final refit, RANSAC.__call__ ransac.py:148-195, batched over pairs (one cooperative block per pair, the ragged
 *     inlier sets stay on the device).  mask [P,N] uint8 selects the points (NULL = all).
 *   dr_refit_essential    five-point solver on all selected points as ONE sample (nister.py:64-65, the path taken
 *                         when pymagsac is absent; ransac.py:157-165 passes ALL points => mask = NULL), computed in
 *                         f64; models [P,10,9], valid [P,10].
 *   dr_refit_fundamental  Hartley-normalised LSQ 8-point on the selected points (ransac.py:150-155 passes the inliers
 *                         of the best mask); models [P,9], valid [P] (0 when fewer than 8 points are selected).
 *                         weights [P,N] (NULL = unweighted; round 6: the `_w` twin of round 3 folded in): RANSAC.__call__ with
 *                         `weighted=1`, ransac.py:151-153 -- `estimate_model(inlier_points, soft_weights[0, inlier_indices[0]])`,
 *                         the weights multiply the epipolar rows (fundamental_matrix_estimator.py:243-244); the Hartley
 *                         normalisation of the selected points stays unweighted (:177-228).
 *   dr_refit_fundamental_bwd  grad_model [P,9] = dL/dF of the model dr_refit_fundamental returns for (matches, mask, weights) ->
 *     grad_matches [P,N,4] and / or grad_weights [P,N] (NULL: not wanted; at least one; grad_weights with weights = NULL is the
 *     derivative at w = 1).  One 256-thread block per pair, f64 inside; nothing is stored by the forward: the same three passes give
 *     the nsel selected rows' centroids mu, r_i = sqrt(2) nsel / D_i and the Gram matrix G = sum w_n^2 rho_n rho_n^T (the weights
 *     scale the ROWS, so they enter squared) bit for bit, the same Jacobi all eigenpairs (lambda_i, v_i) and fh = v_0 with the
 *     forward's sign.  F = T2^T mat(fh) T1 is differentiated as returned: no rank-2 projection, no unit norm.  Then
 *       g_fh = T2 gF T1^T, and the direct gradients of (mu, r) of each image through T1, T2;
 *       z = sum_{i != 0} v_i (v_i . g_fh) / (lambda_i - lambda_0), gG = -(z fh^T + fh z^T) / 2;
 *       per present row, rho_n unscaled, s_n = -(rho_n . z)(rho_n . fh):  grad_weights[n] = 2 w_n s_n, and w_n^2 times the derivative
 *         of s_n by (x1, y1, x2, y2) is the normalised-coordinate gradient gx_n;
 *       per image g_mu = -r sum gx_n + direct, g_r = sum (gx_n . x_n) / r + direct, D = sum |q_n|:  g_D = -g_r r / D,
 *         g_mu -= g_D sum q_n / |q_n|;  grad_matches[n] = r gx_n + g_D q_n / |q_n| + g_mu / nsel (zero subgradient at |q_n| = 0).
 *     Every element of every requested output is written.  Exact zeros: rows the mask drops (never read: a NaN there reaches nothing),
 *     and every row of a pair with nsel < 8, valid = 0, lambda_i - lambda_0 not positive and finite for some i != 0, or a non-finite
 *     z, direct gradient, g_D or g_mu (one decision per pair).  N may be below 8 (all zeros).  -grad_model negates every output bit
 *     for bit.  No atomics, fixed-order sums: a repeated launch gives the same bytes.  Weights are not checked, as in the forward.
 * ------------------------------------------------------------------------------------------ */
int dr_refit_essential_f32(const float *matches, const uint8_t *mask, int P, int N, float *models, uint8_t *valid,
                           void *stream);
int dr_refit_essential_f64(const double *matches, const uint8_t *mask, int P, int N, double *models, uint8_t *valid,
                           void *stream);
int dr_refit_fundamental_f32(const float *matches, const uint8_t *mask, const float *weights, int P, int N, float *models,
                             uint8_t *valid, void *stream);
int dr_refit_fundamental_f64(const double *matches, const uint8_t *mask, const double *weights, int P, int N, double *models,
                             uint8_t *valid, void *stream);
int dr_refit_fundamental_bwd_f32(const float *matches, const uint8_t *mask, const float *weights, const float *grad_model, int P, int N,
                                 float *grad_matches, float *grad_weights, void *stream);
int dr_refit_fundamental_bwd_f64(const double *matches, const uint8_t *mask, const double *weights, const double *grad_model, int P,
                                 int N, double *grad_matches, double *grad_weights, void *stream);

/* K7 acceptance (ransac.py:173-185): MSAC scores of the S refit candidates of every pair (cand [P,S,9], cand_valid [P,S]
 * or NULL; non-finite and all-zero candidates do not compete, as their NaN score of dr_msac_score would not); where the
 * first best candidate scores strictly higher than best_score[p], best_score[p] and best_model[p] ([P,9]) are replaced in
 * place (the best mask is not touched, as in the reference). */
int dr_refit_accept_f32(const float *matches, const float *cand, const uint8_t *cand_valid, const float *thr, int P, int S,
                        int N, float *best_score, float *best_model, void *stream);
int dr_refit_accept_f64(const double *matches, const double *cand, const uint8_t *cand_valid, const double *thr, int P,
                        int S, int N, double *best_score, double *best_model, void *stream);

/* ------------------------------------------------------------------------------------------
 * K7b local optimisation, RANSAC.localOptimization ransac.py:217-257 with lo = 1 (one LSQ refit on the inliers) or
 *     lo = 2 (up to lo_iters refits), test mode, on the per-pair state of dr_ransac_update, in place.  Meant to be
 *     enqueued right behind every dr_ransac_update (one launch per device round, no host synchronisation: capturable).
 *     One cooperative block per pair:
 *   - lo_seen [P,10] is the caller's snapshot (best_score, best_model) of the last visit, initialised to NaN: a pair whose
 *     best_score / best_model still equal it bit for bit was not replaced since and is left untouched (whether or not
 *     its iteration counter has reached max_iters: LO runs before the loop's stop test, ransac.py:122-144);
 *   - with fewer than 8 (fundamental) / 5 (essential) inliers the pair is left as it is;
 *   - otherwise, up to 1 (lo = 1) or lo_iters (lo = 2) times: the K7 refit on best_mask (fundamental: unweighted
 *     Hartley LSQ 8-point; essential: the five-point solver on the selected rows, f64 inside), the MSAC scores at
 *     1.5 thr of its valid, finite candidates (dr_refit_accept's rule, first arg-max) and, where that score is
 *     >= best_score (a tie is taken, ransac.py:252), the new best_score / best_model and -- with dr_ransac_update's
 *     predicate -- best_mask / best_inliers.  The loop stops when a refit loses or leaves the mask unchanged;
 *   - then max_iters[p] = min(max_iterations, adaptive_iteration_number(best_inliers)) (ransac.py:135-142), the
 *     snapshot is stored, and lo_refits[p] (NULL = not counted) grows by the number of refits run.
 * ------------------------------------------------------------------------------------------ */
int dr_local_opt_f32(const float *matches, const float *thr, int P, int N, int fundamental, int lo, int lo_iters, int k,
                     double confidence, double eps, int max_iterations, float *best_score, float *best_model,
                     uint8_t *best_mask, int32_t *best_inliers, double *max_iters, float *lo_seen, int32_t *lo_refits,
                     void *stream);
int dr_local_opt_f64(const double *matches, const double *thr, int P, int N, int fundamental, int lo, int lo_iters, int k,
                     double confidence, double eps, int max_iterations, double *best_score, double *best_model,
                     uint8_t *best_mask, int32_t *best_inliers, double *max_iters, double *lo_seen, int32_t *lo_refits,
                     void *stream);

/* ------------------------------------------------------------------------------------------
 * K4m / K7m two-view MAGSAC++: the score in dr_msac_score's place and the IRLS polish in the final refit's.
 *     d2 = K4's squared Sampson distance; thr2 = (1.5 thr)^2 with thr the [P] tensor of dr_ransac_init, K4's and K6's own cutoff, read
 *     as (k sigma_max)^2: k^2 = chi2.ppf(0.99, 4) = 13.276704135987622 (the residual has 4 degrees of freedom), the noise scale
 *     uniform in [0, sigma_max].  With s = d2 / thr2, u = u_k s, u_k = k^2 / 2 = 6.638352067993811,
 *     Gamma_k = Gamma(3/2, u_k) = 0.0036112606177586, Gamma_0 = Gamma(3/2) = sqrt(pi) / 2, rho_1 = gamma(5/2, u_k) = 1.3015316073311318:
 *       weight  w(s) = (Gamma(3/2, u) - Gamma_k) / (Gamma_0 - Gamma_k)                 for s < 1, else 0
 *       loss    l(s) = (u Gamma(3/2, u) + gamma(5/2, u) - u Gamma_k) / rho_1           for s < 1, else 1
 *       score        = sum_n (1 - l(s_n)) in [0, N];  inliers = #{s_n < 1};  a non-finite d2 contributes nothing.
 *     Evaluated in closed form, F = Gamma_0 erfc(sqrt u):  Gamma(3/2, u) = F + sqrt(u) exp(-u),
 *     rho(u) = u (F - Gamma_k) - (3/2) Gamma(3/2, u) + 3 sqrt(pi) / 4,  l = rho / rho_1.
 *   dr_magsac_score   dr_msac_score's arguments with the mask pointer replaced by inliers [P,M] int32 (NULL = not counted); both types
 *     take the gate pair.  K4's slot rules, so that dr_ransac_update runs unchanged: an invalid slot gets score exactly 0 and 0
 *     inliers without being evaluated, a non-finite or all-zero model a NaN score (0 inliers), the outputs of a gated pair keep their
 *     contents.  No [P,M,N] tensor, no atomics, fixed reduction order: a repeated launch gives the same bits.
 *   dr_magsac_irls    on the per-pair state of dr_ransac_update, in place, one cooperative block per pair (fundamental != 0: F).  Up to
 *     irls_iters times from (best_model, best_score): w(s_n) under the current model for every point, sqrt(w_n) into the pair's row of
 *     weights_ws [P,N] (workspace); the K7 refit over ALL points with these row weights (F: Hartley LSQ 8-point, normalisation
 *     unweighted; E: the five-point solver on the weighted Gram matrix, f64 inside); the MAGSAC++ score over all points of every valid,
 *     finite candidate, first arg-max; taken only on a STRICTLY higher score.  Ends before a fit when fewer than 8 (F) / 5 (E) points
 *     have s < 1 (so always when N is below that: the state is left as it is), on no valid finite candidate, on a candidate that does not win, at the step limit.  irls_fits[p] grows by the fits
 *     run.  best_mask, best_inliers, iters and max_iters are not touched.  No atomics, no read-back: capturable.
 * ------------------------------------------------------------------------------------------ */
int dr_magsac_score_f32(const float *matches, const float *models, const uint8_t *valid, const float *thr, int P, int M, int N,
                        float *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_magsac_score_f64(const double *matches, const double *models, const uint8_t *valid, const double *thr, int P, int M, int N,
                        double *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream);
int dr_magsac_irls_f32(const float *matches, const float *thr, int P, int N, int fundamental, int irls_iters, float *best_score,
                       float *best_model, float *weights_ws, int32_t *irls_fits, void *stream);
int dr_magsac_irls_f64(const double *matches, const double *thr, int P, int N, int fundamental, int irls_iters, double *best_score,
                       double *best_model, double *weights_ws, int32_t *irls_fits, void *stream);

/* ------------------------------------------------------------------------------------------
 * the training loss right after the path -- MatchLoss (loss.py:107-153) on batch_episym
 * (cv_utils.py:680-695).  sums [P,M] = sum over the points with mask[p,n] != 0 (NULL = all points) of
 * min(ys, 1), ys = (x2^T M x1)^2 (1/((Mx1)_0^2+(Mx1)_1^2+1e-15) + 1/((M^T x2)_0^2+(M^T x2)_1^2+1e-15)).
 * Slots with valid == 0 get 0 (NULL = all valid).  The mean over (models x masked points) and over pairs is the
 * caller's.  Backward: grad_models [P,M,9] from grad_sums [P,M] (the clamp passes no gradient at ys >= 1;
 * invalid slots get 0: every entry of grad_models is written).
 * ------------------------------------------------------------------------------------------ */
int dr_episym_fwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *valid, int P, int M,
                      int N, float *sums, void *stream);
int dr_episym_bwd_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *valid,
                      const float *grad_sums, int P, int M, int N, float *grad_models, void *stream);
/* The rest of MatchLoss.forward (loss.py:146-153: mean over the GT-inlier points, mean over the models, per pair):
 *   per_pair[p] = sum_m sums[p,m] / max(n_in[p] * n_models[p], 1),  coef[p] = 1 / max(n_in[p] * n_models[p], 1)
 * with n_in = number of points with mask != 0 (NULL = N) and n_models = number of slots with keep != 0 (NULL = M); the
 * mean over pairs stays with the caller.  dr_episym_bwd_pair is dr_episym_bwd with ONE gradient per pair
 * (grad_pair[p] = d loss / d sums[p, m] for every m, i.e. upstream gradient x coef[p]). */
int dr_match_loss_pair_f32(const float *sums, const uint8_t *mask, const uint8_t *keep, int P, int M, int N,
                           float *per_pair, float *coef, void *stream);
int dr_episym_bwd_pair_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *valid,
                           const float *grad_pair, int P, int M, int N, float *grad_models, void *stream);
/* MatchLoss down to the scalar (loss.py:146-153 including `.mean()` over the pairs of the batch), one launch:
 *   per_pair / coef as above and mean[0] = sum_p per_pair[p] / P.  dr_episym_bwd_mean is the matching backward:
 *   d loss / d sums[p,m] = grad_mean[0] * coef[p] / P (grad_mean = the upstream gradient of the scalar, one float in device
 *   memory), so no per-pair gradient tensor is formed on the host side. */
/* Round 5: MatchLoss value + gradient in ONE pass over the (model x point) grid (the loss is a scalar mean: its gradient w.r.t. a
 * model is one number per pair times a quantity the forward can write while it holds the residuals in registers).
 * dr_match_loss_fused_f32 = dr_episym_fwd + dr_match_loss_mean + the unscaled gradient grad_unscaled [P,M,9] = d sums[p,m] / d model.
 * dr_match_loss_scale_f32: grad_models = grad_unscaled x coef[p] x grad_mean[0] / P, the whole backward of the loss. */
int dr_match_loss_fused_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *valid, int P, int M, int N,
                            float *sums, float *grad_unscaled, float *per_pair, float *coef, float *mean, void *stream);
int dr_match_loss_scale_f32(const float *grad_unscaled, const float *coef, const float *grad_mean, int P, int M, float *grad_models,
                            void *stream);
int dr_match_loss_mean_f32(const float *sums, const uint8_t *mask, const uint8_t *keep, int P, int M, int N,
                           float *per_pair, float *coef, float *mean, void *stream);
int dr_episym_bwd_mean_f32(const float *matches, const uint8_t *mask, const float *models, const uint8_t *valid,
                           const float *coef, const float *grad_mean, int P, int M, int N, float *grad_models, void *stream);

/* ------------------------------------------------------------------------------------------
 * pose error of essential matrices -- the body of PoseLoss.forward_average (loss.py:11-68) =
 * eval_essential_matrix(svd=False) (cv_utils.py:503-525) for every model of every pair:
 *   Horn decomposition (new_decompose_E, cv_utils.py:118-161) -> candidates (R1,t) (R2,t) (R1,-t) (R2,-t);
 *   votes[c] = number of points triangulated in front of both cameras and closer than distance_threshold
 *   (recoverPose / cheirality_check, cv_utils.py:48-80,177-189; the reference passes 50); which = first arg-max;
 *   err_R, err_t in degrees (evaluate_R_t_tensor, cv_utils.py:361-380).
 *   matches [P,N,4] (normalised coordinates), models [P,M,9], gt_R [P,9], gt_t [P,3];
 *   err_R, err_t [P,M]; which [P,M] int32; votes [P,M,4] int32 or NULL.
 * Backward: grad_models [P,M,9] from grad_err_R, grad_err_t [P,M] at the recorded candidate `which`
 * (the skew matrix of Horn's formula is a constant, as in the reference; non-finite derivatives -> 0).
 * ------------------------------------------------------------------------------------------ */
int dr_pose_error_fwd_f32(const float *matches, const float *models, const float *gt_R, const float *gt_t, int P, int M,
                          int N, double distance_threshold, float *err_R, float *err_t, int32_t *which, int32_t *votes,
                          void *stream);
int dr_pose_error_fwd_f64(const double *matches, const double *models, const double *gt_R, const double *gt_t, int P,
                          int M, int N, double distance_threshold, double *err_R, double *err_t, int32_t *which,
                          int32_t *votes, void *stream);
/* The same with the SVD decomposition of the reference's `svd=True` branch (decompose_E, cv_utils.py:83-116;
 * eval_essential_matrix's default, cv_utils.py:503): R1,2 = U W^(+-T) V^T, t = +-u3.  The four candidate poses are the
 * same set for every SVD sign convention; their order -- `which`, and the winner of an exact tie of votes -- is not.
 * Forward only: the reference's gradient goes through torch.linalg.svd of a matrix with sigma_1 = sigma_2, where it is
 * undefined. */
int dr_pose_error_svd_fwd_f32(const float *matches, const float *models, const float *gt_R, const float *gt_t, int P, int M,
                              int N, double distance_threshold, float *err_R, float *err_t, int32_t *which, int32_t *votes,
                              void *stream);
int dr_pose_error_svd_fwd_f64(const double *matches, const double *models, const double *gt_R, const double *gt_t, int P,
                              int M, int N, double distance_threshold, double *err_R, double *err_t, int32_t *which,
                              int32_t *votes, void *stream);
int dr_pose_error_bwd_f32(const float *models, const float *gt_R, const float *gt_t, const int32_t *which,
                          const float *grad_err_R, const float *grad_err_t, int P, int M, float *grad_models,
                          void *stream);
int dr_pose_error_bwd_f64(const double *models, const double *gt_R, const double *gt_t, const int32_t *which,
                          const double *grad_err_R, const double *grad_err_t, int P, int M, double *grad_models,
                          void *stream);

/* The inlier mask of cv2.recoverPose (loss.py:99,134: the ground-truth inlier mask of ClassificationLoss / MatchLoss):
 * per (pair, model) the points that pass the cheirality test of the winning one of the four candidate poses.
 * models [P,M,9] (normally the ground-truth E, M = 1); which [P,M] int32 or NULL; mask [P,M,N] uint8. */
int dr_recover_pose_mask_f32(const float *matches, const float *models, int P, int M, int N, double distance_threshold,
                             int32_t *which, uint8_t *mask, void *stream);
int dr_recover_pose_mask_f64(const double *matches, const double *models, int P, int M, int N, double distance_threshold,
                             int32_t *which, uint8_t *mask, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DRANSAC_H_ */
