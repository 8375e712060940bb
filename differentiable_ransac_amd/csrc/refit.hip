// K7 -- final refit of the best model (RANSAC.__call__, ransac.py:148-195), batched over pairs with no host round trip:
//   essential:    Nister on ALL N points of the pair as one "sample" (what nister.py:64-65 does when pymagsac is absent,
//                 ransac.py:157-165), in f64;
//   fundamental:  Hartley-normalised LSQ 8-point on the INLIERS of the best mask (ransac.py:150-155,
//                 fundamental_matrix_estimator.py:172-174,177-260).
// One 256-thread block per pair: the four waves accumulate the 9x9 Gram matrix of the (weighted / masked) epipolar rows
// cooperatively (three passes for F: centroid, mean distances, Gram), then wave 0 takes the eigenvectors it needs from a
// wave-cooperative Jacobi eigen-decomposition (F: the smallest one, E: the four smallest) and, for E, runs the five-point pipeline.
// The ragged inlier sets never leave the device.
// Behind it, on the same two fit bodies (refit_fundamental_pair, refit_essential_pair): K7b, the local optimisation, and K7m, the
// MAGSAC++ IRLS polish.  What those two share is PairRefit (LDS layout, candidate arg-max); all four entries launch
// through pair_mode / pair_launch.  The terms, the model classification and the block score pass are ransac_device.hpp's.
#include "fivepoint_device.hpp"
#include "magsac_device.hpp"
#include "ransac_device.hpp"

namespace dr {

constexpr int kRefT = 256;
constexpr int kRefitPairFinishMinPairs = 16;   // launches of fewer pairs keep the light final stage (see refit_essential_kernel)
// dynamic LDS of a refit block: five-point workspace (one slot), gram[81] + red[4] (padded to 96), wave partials [4][45], Jacobi
// V[81] + (C, S)[9]: 4.6 KB -- with a 162-double slot PER LANE (83 KB) a block left room for only two of the four solver blocks a
// CU hosts.  The wave-cooperative final stage overlays the solver's workspace, kNisterPairDoubles.
constexpr int kRefitLdsDoubles = 192 + 96 + 4 * 45 + 81 + 18;   // (the Jacobi's per-index rotation table: C[9], S[9])

__device__ __forceinline__ double block_sum(double v, double *red /* [4] */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// accumulates sum_n w_n * row_n row_n^T (45 unique entries) over this thread's points into gram[81] in LDS
template <bool kFundamental, typename T>
__device__ __forceinline__ void gram_accumulate(const T *__restrict__ mt, const uint8_t *__restrict__ mk,
                                                const T *__restrict__ wt, int N,
                                                const double (&mu)[4], double r1, double r2, double *gram, double *red) {
  double acc[45];
#pragma unroll
  for (int q = 0; q < 45; ++q) acc[q] = 0;
  for (int n = threadIdx.x; n < N; n += kRefT) {
    if (mk && !mk[n]) continue;
    double row[9];
    if (kFundamental)
      epipolar_row_f(((double)mt[4 * n] - mu[0]) * r1, ((double)mt[4 * n + 1] - mu[1]) * r1,
                     ((double)mt[4 * n + 2] - mu[2]) * r2, ((double)mt[4 * n + 3] - mu[3]) * r2,
                     wt ? (double)wt[n] : 1.0, row);   // weights scale the ROWS (fundamental_matrix_estimator.py:243-244)
    else
      epipolar_row_5pt((double)mt[4 * n], (double)mt[4 * n + 1], (double)mt[4 * n + 2], (double)mt[4 * n + 3],
                       wt ? (double)wt[n] : 1.0, row);   // (1.0: the unweighted row, bit for bit)
    int q = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j) acc[q++] += row[i] * row[j];
  }
  // 45 partial sums per thread: reduced inside each wave by DPP (no LDS traffic), one LDS slot per (wave, entry), ONE
  // barrier, then 45 threads add the four wave partials (was: 45 x (wave butterfly over ds_bpermute + two barriers))
  double *part = gram + 96;   // [4][45] behind gram[81] + red[4] (+ padding); kRefitLdsDoubles
#pragma unroll
  for (int q = 0; q < 45; ++q) {
    const double s = wave_sum_lane63(acc[q]);
    if ((threadIdx.x & 63) == 63) part[(threadIdx.x >> 6) * 45 + q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 45) {
    const double s = part[threadIdx.x] + part[45 + threadIdx.x] + part[90 + threadIdx.x] + part[135 + threadIdx.x];
    int i = 0, rem = threadIdx.x;     // entry q of the upper triangle -> (i, j)
    while (rem >= 9 - i) { rem -= 9 - i; ++i; }
    const int j = i + rem;
    gram[i * 9 + j] = s;
    gram[j * 9 + i] = s;
  }
  __syncthreads();
}

// Round 5: the stages after the elimination are the minimal solver's wave-cooperative ones (nister_finish_pair: Sturm isolation,
// refinement and the polish / verification of the candidates dealt out over the wave's lanes) with ONE occupied lane pair -- the
// one-sample form they replace (derivative-chain root search and up to ten polish + verification passes, one after the other,
// every lane redundantly) was 86 of the kernel's 120 us.  The price: the minimal solver's register and LDS footprint (one wave per
// SIMD, 38.9 KB) -- which costs nothing where it matters: a solver wave of the same call takes every register of its SIMD since
// round 3, so a refit wave never shared a SIMD with one; the sampler's and the scoring kernel's light waves still fit beside it.
// kPairFinish is chosen per launch: calls of a few pairs (the drop-in's one pair per call, where the refit hides behind the whole
// chain anyway) keep the light one-sample form -- 256 registers, 4.6 KB of LDS; same-box A/B of the per-pair loop: 0.208-0.211 ms
// per pair with it, 0.214-0.217 with the heavy form -- batched calls take the fast one.
// (register budget of the light form: 256 per lane, waves_per_eu(2, 2), although one wave per pair does the work)
// One pair, the whole block: the 10 candidates of the five-point solver on the rows mt [N,4] selected by mk (NULL = all), row n
// scaled by wt[n] (NULL = unweighted) -> models [10,9], valid [10].  Waves 1-3 return after the Gram matrix, wave 0 solves (a caller that goes on puts a barrier behind).
// lds: the block's dynamic LDS -- [192] five-point workspace, then gram[81] + red[4], wave partials, Jacobi (kRefitLdsDoubles),
// or the solver's whole workspace with kPairFinish (kmax(kRefitLdsDoubles, kNisterPairDoubles)).
template <typename T, bool kPairFinish>
__device__ __forceinline__ void refit_essential_pair(const T *__restrict__ mt, const uint8_t *__restrict__ mk,
                                                     const T *__restrict__ wt, int N, double *lds,
                                                     T *__restrict__ models, uint8_t *__restrict__ valid) {
  double *gram = lds + 192;   // [0,162): the one five-point workspace slot all lanes share (identical values)
  double *red = gram + 81;
  const double mu[4] = {0, 0, 0, 0};
  gram_accumulate<false, T>(mt, mk, wt, N, mu, 1.0, 1.0, gram, red);
  if (threadIdx.x >= 64) return;
  // the rest is one latency-bound wave per pair, usually running next to the scoring kernel of the same call (8 VALU-bound
  // waves per SIMD): raise its issue priority so that it proceeds at its own pace and the scoring waves fill the gaps
  __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x;
  double nb[4][9];
  {
    // 9x9 eigen-decomposition by the whole wave in LDS (was: every lane ran the full cyclic Jacobi redundantly in
    // registers: 324 live doubles, 512 registers + 1.5 KB of scratch per lane and ~120 us of the kernel)
    double *Vl = gram + 96 + 4 * 45, *cs = Vl + 81;
    jacobi_eig9_wave(gram, Vl, cs, lane);
    double ev[4][9];
    smallest_eigvecs9_lds<4>(gram, Vl, ev);
    // nb[3] <-> smallest eigenvalue ... nb[0] <-> fourth smallest (the order of torch.linalg.svd's Vh[-4:])
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 9; ++r) nb[3 - t][r] = ev[t][r];
  }
  double e[3][3][4];
  basis_to_entries(nb, e);
  LaneWs w{lds, 1};   // every lane solves the same system: one shared slot, same-address writes of equal values
  double X[6][10];
  const bool ok = constraints_reduce<NisterOrder, 4>(e, w, 1.0, X);
  if constexpr (kPairFinish) {
    // lane pair 0 holds the sample (lane 0 searches |z| <= 1, lane 1 |z| > 1); the other 31 pairs are empty slots of the wave's
    // task queues, which is where the pair's brackets and candidates are worked on side by side.  The block's LDS is reused whole.
    nister_finish_pair<T>(nb, X, ok, lds, lane, 0, lane < 2, models, valid, nullptr);
  } else {
    // like the minimal solver, two lanes share the sample: even lanes search |z| <= 1 and fill the slots from 0 upwards,
    // odd lanes |z| > 1 from 9 downwards (all 32 lane pairs do the same work; lanes 0 and 1 store)
    nister_finish<T, true>(nb, X, ok, models, valid, lane < 2, lane & 1);
  }
}

template <typename T, bool kPairFinish>
__global__ __launch_bounds__(kRefT) __attribute__((amdgpu_waves_per_eu(kPairFinish ? 1 : 2, kPairFinish ? 1 : 2))) void refit_essential_kernel(const T *__restrict__ matches,
                                                                const uint8_t *__restrict__ mask, int N,
                                                                T *__restrict__ models, uint8_t *__restrict__ valid) {
  extern __shared__ __align__(16) double lds[];
  const int p = blockIdx.x;
  refit_essential_pair<T, kPairFinish>(matches + (size_t)p * N * 4, mask ? mask + (size_t)p * N : nullptr,
                                       static_cast<const T *>(nullptr), N, lds,
                                       models + (size_t)p * 90, valid + (size_t)p * 10);
}

// One pair, the whole block: the (row-weighted when wt != NULL) LSQ 8-point model of the rows mt [N,4] selected by mk (NULL = all)
// -> model [9], valid [1] (0 below 8 rows or when not finite).  Waves 1-3 return after the Gram matrix, wave 0 solves.
template <typename T>
__device__ __forceinline__ void refit_fundamental_pair(const T *__restrict__ mt, const uint8_t *__restrict__ mk,
                                                       const T *__restrict__ wt, int N, double *lds, T *__restrict__ model,
                                                       uint8_t *__restrict__ valid) {
  double *gram = lds + 192;   // [0,162): the one five-point workspace slot all lanes share (identical values)
  double *red = gram + 81;
  // pass 1: centroid of the selected points
  double s[4] = {0, 0, 0, 0}, cnt = 0;
  for (int n = threadIdx.x; n < N; n += kRefT) {
    if (mk && !mk[n]) continue;
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] += (double)mt[4 * n + d];
    cnt += 1.0;
  }
  const double nsel = block_sum(cnt, red);
  double mu[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) mu[d] = block_sum(s[d], red) / nsel;
  // pass 2: mean distances
  double d1 = 0, d2 = 0;
  for (int n = threadIdx.x; n < N; n += kRefT) {
    if (mk && !mk[n]) continue;
    const double a = (double)mt[4 * n] - mu[0], b = (double)mt[4 * n + 1] - mu[1];
    const double c = (double)mt[4 * n + 2] - mu[2], d = (double)mt[4 * n + 3] - mu[3];
    d1 += sqrt(a * a + b * b);
    d2 += sqrt(c * c + d * d);
  }
  const double r1 = M_SQRT2 * nsel / block_sum(d1, red), r2 = M_SQRT2 * nsel / block_sum(d2, red);
  // pass 3: Gram matrix of the normalised rows
  gram_accumulate<true, T>(mt, mk, wt, N, mu, r1, r2, gram, red);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  // The null vector (only the last right singular vector is needed, fundamental_matrix_estimator.py:249-254) is the Gram matrix's
  // smallest eigenvector from the wave-cooperative Jacobi the essential refit runs: exact to rounding for ANY gap between the two
  // smallest eigenvalues.  (Until the refit tests against f64 this was a fixed 24 steps of inverse iteration, whose error is
  // (lambda_9 / lambda_8)^24: fine on clean inliers, ratio < 0.05, and off by 1e-4 ... 1e-1 on a selection that holds outliers,
  // ratio 0.6 ... 0.95 -- the mask local optimisation refits an early best model on.)
  double f[9];
  {
    double *Vl = gram + 96 + 4 * 45, *cs = Vl + 81;
    jacobi_eig9_wave(gram, Vl, cs, lane);
    double ev[1][9];
    smallest_eigvecs9_lds<1>(gram, Vl, ev);
#pragma unroll
    for (int r = 0; r < 9; ++r) f[r] = ev[0][r];
  }
  double G[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[i][0] = f[3 * i] * r1;
    G[i][1] = f[3 * i + 1] * r1;
    G[i][2] = -r1 * (f[3 * i] * mu[0] + f[3 * i + 1] * mu[1]) + f[3 * i + 2];
  }
  double F[9];
  bool ok = nsel >= 8.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = r2 * G[0][j];
    F[3 + j] = r2 * G[1][j];
    F[6 + j] = -r2 * (mu[2] * G[0][j] + mu[3] * G[1][j]) + G[2][j];
  }
#pragma unroll
  for (int q = 0; q < 9; ++q) ok = ok && is_finite(F[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) model[q] = ok ? (T)F[q] : T(q % 4 == 0 ? 1 : 0);
    valid[0] = ok;
  }
}

template <typename T>
__global__ __launch_bounds__(kRefT) __attribute__((amdgpu_waves_per_eu(1, 1))) void refit_fundamental_kernel(const T *__restrict__ matches,
                                                                  const uint8_t *__restrict__ mask,
                                                                  const T *__restrict__ weights, int N,
                                                                  T *__restrict__ models, uint8_t *__restrict__ valid) {
  extern __shared__ __align__(16) double lds[];
  const int p = blockIdx.x;
  // per-point row weights [P,N] (ransac.py:151-153 hands the estimator `soft_weights[0, inlier_indices]`); the Hartley
  // normalisation stays unweighted, as in fundamental_matrix_estimator.py:177-228
  refit_fundamental_pair<T>(matches + (size_t)p * N * 4, mask ? mask + (size_t)p * N : nullptr,
                            weights ? weights + (size_t)p * N : nullptr, N, lds, models + (size_t)p * 9, valid + p);
}

// ---- The pair scaffold: what the per-pair kernels of this file share.  kMode: 0 = F, 1 = E with the light final stage, 2 = E with the
// wave-cooperative one (launches of at least kRefitPairFinishMinPairs pairs: see refit_essential_pair).
// PairMode: the constants and the dynamic LDS of a block, [kWs] refit workspace | candidates [kS][9] (T) | their valid flags (the last
// two for the kernels that fit and score in one launch).
template <int kMode>
struct PairMode {
  static constexpr bool kF = kMode == 0;
  static constexpr int kS = kF ? 1 : 10;                 // candidates per refit
  static constexpr int kMinRows = kF ? 8 : 5;            // rows the LSQ solve needs
  static constexpr int kWs = kMode == 2 ? kmax(kRefitLdsDoubles, kNisterPairDoubles) : kRefitLdsDoubles;
  static constexpr int kCand = (kWs + 3) & ~3;           // (32-byte aligned)
  static constexpr size_t lds_bytes(bool candidates) { return sizeof(double) * (candidates ? kCand + 90 + 2 : kWs); }
};

// PairRefit: the block's candidate slots and the choice among them.  The fit itself (refit_fundamental_pair / refit_essential_pair into
// cand / cvalid, then a barrier) is written out in the two kernels, with their null mask or weight pointer as a typed literal: behind
// a shared fit(mt, mk, wt, N) member the refit bodies compiled differently in EVERY kernel of the file (LOG 21).
template <typename T, int kMode>
struct PairRefit : PairMode<kMode> {
  using PairMode<kMode>::kCand;
  double *lds;
  T *cand;
  uint8_t *cvalid;
  __device__ __forceinline__ explicit PairRefit(double *lds_)
      : lds(lds_), cand(reinterpret_cast<T *>(lds_ + kCand)), cvalid(reinterpret_cast<uint8_t *>(lds_ + kCand + 90)) {}
  // first arg-max (strict: like torch.argmax) of the scores under `term`, over all N points, of the valid candidates that
  // model_kind(..., zero_is_nan) calls scored -> its slot (-1: none) and score cb.  Block-uniform.
  template <typename Term>
  __device__ __forceinline__ int best_candidate(const T *__restrict__ mt, int N, const Term &term, bool zero_is_nan, T *s_part,
                                                T &cb) const {
    cb = -INFINITY;
    int which = -1;
    for (int c = 0; c < PairMode<kMode>::kS; ++c) {
      if (!cvalid[c]) continue;
      T m[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) m[q] = cand[c * 9 + q];
      const int kind = model_kind<T>(m, true, zero_is_nan);
      const T sc = block_score<T, kRefT>(mt, m, N, term, s_part);
      if (kind == kModelScored && sc > cb) { cb = sc; which = c; }
    }
    return which;
  }
};

// The launcher of the per-pair kernels.  pair_mode: the kMode of a launch; pair_launch: Kernel, one block per pair, with kMode's dynamic
// LDS (opted in); pair_family_launch (below the kernels): a kernel family K<T, kMode> at the launch's mode.
inline int pair_mode(bool fundamental, int P) { return fundamental ? 0 : (P >= kRefitPairFinishMinPairs ? 2 : 1); }
template <auto Kernel, int kMode, bool kCandidates, typename... Args>
int pair_launch(const char *name, int P, void *stream, Args... args) {
  constexpr size_t smem = PairMode<kMode>::lds_bytes(kCandidates);
  allow_dynamic_lds<Kernel>(smem);
  return launch_lds(name, Kernel, dim3(P), kRefT, smem, stream, args...);
}

// ---- K7b local optimisation (RANSAC.localOptimization, ransac.py:217-257, lo = 1 / 2), one 256-thread block per pair, once per
// device round right behind dr_ransac_update.  A pair whose (best_score, best_model) still equals its snapshot lo_seen[p] (bit
// for bit: only a replacement by dr_ransac_update changes them, and the snapshot starts as NaN) returns at once.  Otherwise, up
// to `iters` times: the refit of this file on the best mask (F: LSQ 8-point, unweighted; E: the five-point solver on the
// selected rows, f64 inside), the MSAC scores of its valid, finite candidates (first arg-max; an all-zero candidate is not excluded
// here, unlike in refit_accept_kernel), and, if that score is >= the best (ransac.py:252: ties are taken), the new best score / model
// and -- with dr_ransac_update's predicate -- mask and inlier count.  The loop stops early when a refit loses or leaves the mask as it
// was (the next refit would see the same rows: same model, same outcome).  Then max_iters from the new inlier count
// (ransac.py:135-142) and the snapshot.
template <typename T, int kMode>
__global__ __launch_bounds__(kRefT) __attribute__((amdgpu_waves_per_eu(kMode == 1 ? 2 : 1, kMode == 1 ? 2 : 1))) void local_opt_kernel(
    const T *__restrict__ matches, const T *__restrict__ thr, int N, int iters, int k, double confidence, double eps,
    int max_iterations, T *__restrict__ best_score, T *__restrict__ best_model, uint8_t *__restrict__ best_mask,
    int32_t *__restrict__ best_inliers, double *__restrict__ max_iters, T *__restrict__ lo_seen, int32_t *__restrict__ lo_refits) {
  extern __shared__ __align__(16) double lds[];
  const PairRefit<T, kMode> pair(lds);
  constexpr int kMinRows = PairMode<kMode>::kMinRows;
  __shared__ T s_part[kRefT / kWave];
  __shared__ int s_cnt[kRefT / kWave], s_chg[kRefT / kWave];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const T *mt = matches + (size_t)p * N * 4;
  uint8_t *mk = best_mask + (size_t)p * N;
  T *seen = lo_seen + (size_t)p * 10;
  T bs = best_score[p];
  T bm[9];
  bool same = same_bits(bs, seen[0]);
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    bm[q] = best_model[(size_t)p * 9 + q];
    same = same && same_bits(bm[q], seen[1 + q]);
  }
  if (same) return;   // block-uniform: no replacement since the last visit
  const SampsonMsacTerm<T> term(thr[p]);
  // the current inlier count, from the mask itself
  int cnt = 0;
  for (int n = tid; n < N; n += kRefT) cnt += mk[n] != 0;
  cnt = wave_sum(cnt);
  if (lane == 0) s_cnt[wv] = cnt;
  __syncthreads();
  int inl = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  const bool run = inl >= kMinRows;
  int refits = 0;
  for (int it = 0; run && it < iters && inl >= kMinRows; ++it) {
    __syncthreads();   // (the previous pass's s_cnt / s_chg have been read; the refit's LDS is free)
    if constexpr (kMode == 0)
      refit_fundamental_pair<T>(mt, mk, static_cast<const T *>(nullptr), N, lds, pair.cand, pair.cvalid);
    else
      refit_essential_pair<T, kMode == 2>(mt, mk, static_cast<const T *>(nullptr), N, lds, pair.cand, pair.cvalid);
    __syncthreads();
    ++refits;
    T cb;
    const int which = pair.best_candidate(mt, N, term, false, s_part, cb);
    if (which < 0 || !(cb >= bs)) break;                         // ransac.py:252-257
#pragma unroll
    for (int q = 0; q < 9; ++q) bm[q] = pair.cand[which * 9 + q];
    bs = cb;
    int c2 = 0, chg = 0;
    for (int n = tid; n < N; n += kRefT) {
      const T *q = mt + (size_t)n * 4;
      const uint8_t in = term.inlier(term.ratio(sampson_d2<T>(bm, q[0], q[1], q[2], q[3])));
      chg |= in != mk[n];
      mk[n] = in;
      c2 += in;
    }
    c2 = wave_sum(c2);
    chg = wave_sum(chg);
    if (lane == 0) { s_cnt[wv] = c2; s_chg[wv] = chg; }
    __syncthreads();
    inl = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    const bool changed = (s_chg[0] | s_chg[1] | s_chg[2] | s_chg[3]) != 0;
    if (tid == 0) {
      best_score[p] = bs;
      best_inliers[p] = inl;
#pragma unroll
      for (int q = 0; q < 9; ++q) best_model[(size_t)p * 9 + q] = bm[q];
    }
    if (!changed) break;
  }
  if (tid == 0) {
    if (run) max_iters[p] = adaptive_max_iters(inl, N, k, confidence, eps, max_iterations);
    seen[0] = bs;
#pragma unroll
    for (int q = 0; q < 9; ++q) seen[1 + q] = bm[q];
    if (lo_refits) lo_refits[p] += refits;
  }
}

// ---- K7m IRLS polish of the pair state under the two-view MAGSAC++ loss (BatchedRANSAC(scoring = "magsac")), one 256-thread
// block per pair: local_opt_kernel's sibling on the same scaffold.  Up to `iters` times from the pair's (best_model, best_score): the weights
// w(s_n) of magsac_device.hpp under the current model, sqrt(w_n) into the pair's row of weights_ws (the refit bodies scale the ROWS, so
// the Gram matrix is sum_n w_n row_n row_n^T); the refit of this file over ALL points with those weights (F: the Hartley normalisation
// stays unweighted over all points; E: the five-point solver on the weighted Gram matrix); the MAGSAC++ score over all points of every
// valid candidate that is finite and not all zero, first arg-max; taken only on a STRICTLY higher score.  The loop ends before a fit when fewer than 8 (F) /
// 5 (E) points have s < 1 (s and w in f64 for either type), on no such candidate, on a candidate that does not win, and at the step limit.  irls_fits[p] += fits
// run.  best_mask, best_inliers, iters and max_iters are neither read nor written.  Sums go lane, wave butterfly, the four waves in
// order: no atomics, no read-back, a repeated launch gives the same bits.
// (one wave per SIMD in every mode: under local_opt_kernel's two-wave budget the light final stage spills 836 B per lane here)
template <typename T, int kMode>
__global__ __launch_bounds__(kRefT) __attribute__((amdgpu_waves_per_eu(1, 1))) void magsac_irls_kernel(
    const T *__restrict__ matches, const T *__restrict__ thr, int N, int iters, T *__restrict__ best_score, T *__restrict__ best_model,
    T *__restrict__ weights_ws, int32_t *__restrict__ irls_fits) {
  extern __shared__ __align__(16) double lds[];
  const PairRefit<T, kMode> pair(lds);
  __shared__ T s_part[kRefT / kWave];
  __shared__ int s_cnt[kRefT / kWave];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const T *mt = matches + (size_t)p * N * 4;
  T *wt = weights_ws + (size_t)p * N;
  T bs = best_score[p];
  T bm[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) bm[q] = best_model[(size_t)p * 9 + q];
  const Magsac4Term<T> term(thr[p]);
  const Magsac4Term<double> termd((double)thr[p]);
  bool taken = false;
  int fits = 0;
  for (int it = 0; it < iters; ++it) {
    __syncthreads();   // (the state and the previous pass's s_cnt / s_part have been read; the refit's LDS is free)
    int cnt = 0;
    // the weights in f64 whatever T is (the refit is f64 inside): with f32 residuals at a cutoff of 1e-3 the weights are off by
    // ~1e-3 relative and the fitted model by more than its own output rounding
    double bd[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) bd[q] = (double)bm[q];
    for (int n = tid; n < N; n += kRefT) {
      const T *q = mt + (size_t)n * 4;
      const double s = termd.ratio(sampson_d2<double>(bd, (double)q[0], (double)q[1], (double)q[2], (double)q[3]));
      const bool in = termd.inlier(s);
      wt[n] = in ? (T)sqrt(termd.weight(s)) : T(0);
      cnt += in;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();   // (also orders the weights before the refit's reads)
    if (s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3] < PairMode<kMode>::kMinRows) break;   // block-uniform, like every exit below
    if constexpr (kMode == 0)
      refit_fundamental_pair<T>(mt, static_cast<const uint8_t *>(nullptr), wt, N, lds, pair.cand, pair.cvalid);
    else
      refit_essential_pair<T, kMode == 2>(mt, static_cast<const uint8_t *>(nullptr), wt, N, lds, pair.cand, pair.cvalid);
    __syncthreads();
    ++fits;
    T cb;
    const int which = pair.best_candidate(mt, N, term, true, s_part, cb);
    if (which < 0 || !(cb > bs)) break;
#pragma unroll
    for (int q = 0; q < 9; ++q) bm[q] = pair.cand[which * 9 + q];
    bs = cb;
    taken = true;
  }
  if (tid == 0) {
    if (taken) {
      best_score[p] = bs;
#pragma unroll
      for (int q = 0; q < 9; ++q) best_model[(size_t)p * 9 + q] = bm[q];
    }
    irls_fits[p] += fits;
  }
}

template <typename T, int kMode>
struct LocalOpt {
  static constexpr auto kernel = &local_opt_kernel<T, kMode>;
  static constexpr const char *kName = "local_opt_kernel";
};
template <typename T, int kMode>
struct MagsacIrls {
  static constexpr auto kernel = &magsac_irls_kernel<T, kMode>;
  static constexpr const char *kName = "magsac_irls_kernel";
};
// args: the kernel's own argument list
template <template <typename, int> class K, typename T, typename... Args>
int pair_family_launch(bool fundamental, int P, void *stream, Args... args) {
  switch (pair_mode(fundamental, P)) {
    case 0: return pair_launch<K<T, 0>::kernel, 0, true>(K<T, 0>::kName, P, stream, args...);
    case 2: return pair_launch<K<T, 2>::kernel, 2, true>(K<T, 2>::kName, P, stream, args...);
    default: return pair_launch<K<T, 1>::kernel, 1, true>(K<T, 1>::kName, P, stream, args...);
  }
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                              \
  int dr_refit_fundamental_##sfx(const T *matches, const uint8_t *mask, const T *weights, int P, int N, T *models, uint8_t *valid,  \
                                 void *stream) {                                                                                    \
    DR_REQUIRE(matches && models && valid, "null pointer");                                                                         \
    DR_REQUIRE(P > 0 && N >= 8, "bad sizes");                                                                                       \
    return dr::pair_launch<dr::refit_fundamental_kernel<T>, 0, false>("refit_kernel", P, stream, matches, mask, weights, N, models, \
                                                                      valid);                                                       \
  }                                                                                                                                 \
  int dr_refit_essential_##sfx(const T *matches, const uint8_t *mask, int P, int N, T *models, uint8_t *valid, void *stream) {      \
    DR_REQUIRE(matches && models && valid, "null pointer");                                                                         \
    DR_REQUIRE(P > 0 && N >= 5, "bad sizes");                                                                                       \
    if (dr::pair_mode(false, P) == 2)                                                                                               \
      return dr::pair_launch<dr::refit_essential_kernel<T, true>, 2, false>("refit_kernel", P, stream, matches, mask, N, models,    \
                                                                            valid);                                                 \
    return dr::pair_launch<dr::refit_essential_kernel<T, false>, 1, false>("refit_kernel", P, stream, matches, mask, N, models,     \
                                                                           valid);                                                  \
  }                                                                                                                                 \
  int dr_local_opt_##sfx(const T *matches, const T *thr, int P, int N, int fundamental, int lo, int lo_iters, int k,                \
                         double confidence, double eps, int max_iterations, T *best_score, T *best_model, uint8_t *best_mask,       \
                         int32_t *best_inliers, double *max_iters, T *lo_seen, int32_t *lo_refits, void *stream) {                  \
    DR_REQUIRE(matches && thr && best_score && best_model && best_mask && best_inliers && max_iters && lo_seen, "null pointer");    \
    DR_REQUIRE(P > 0 && N >= (fundamental ? 8 : 5) && k > 0, "bad sizes");                                                          \
    DR_REQUIRE(lo == 1 || lo == 2, "lo must be 1 (one refit) or 2 (iterated refits)");                                              \
    DR_REQUIRE(lo == 1 || lo_iters >= 1, "lo_iters must be at least 1");                                                            \
    return dr::pair_family_launch<dr::LocalOpt, T>(fundamental != 0, P, stream, matches, thr, N, lo == 1 ? 1 : lo_iters, k,         \
                                                   confidence, eps, max_iterations, best_score, best_model, best_mask,              \
                                                   best_inliers, max_iters, lo_seen, lo_refits);                                    \
  }                                                                                                                                 \
  int dr_magsac_irls_##sfx(const T *matches, const T *thr, int P, int N, int fundamental, int irls_iters, T *best_score,            \
                           T *best_model, T *weights_ws, int32_t *irls_fits, void *stream) {                                        \
    DR_REQUIRE(matches && thr && best_score && best_model && weights_ws && irls_fits, "null pointer");                              \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");   /* (below 8 / 5 points the kernel ends before its first fit: a no-op polish) */       \
    DR_REQUIRE(irls_iters >= 1, "irls_iters must be at least 1");                                                                   \
    return dr::pair_family_launch<dr::MagsacIrls, T>(fundamental != 0, P, stream, matches, thr, N, irls_iters, best_score,          \
                                                     best_model, weights_ws, irls_fits);                                            \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
