// The differentiable soft-inlier score of the absolute-pose path (ops.pnp_soft_score, loss.PnPExpectedLoss): every pose scored by a
// sigmoid of its squared reprojection error on every point, with a reverse pass to the poses AND to the points -- the (model x point)
// grid with its two reductions.  include/dransac.h states the maths; the residual is pnp_loss.hip's with 1 / z_c a division, its
// numerators formed beyond the type's precision (below: the gradient is a sum of e i terms with the loss's cancellation):
//     x_c = R X + t,  i = 1 / z_c,  (x, y) = (x_c, y_c) i,  e = (x - u, y - v),  d2 = |e|^2,  a = beta (1 - d2 / thr2)
//     live = z_c > 0 and d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0,   score[m] = sum_{n in mask} w[m,n]
// Three launches, no [P,M,N] tensor, no atomics, no workspace:
//   pnp_soft_score_kernel<T, false>   the scores.  pnp_loss_kernel's mapping: one LANE per model, one wave per block, grid
//     (ceil(M / 64), P); the masked points compacted tile by tile into LDS in ascending order, each read as a broadcast; the sum in the
//     order of the points.
//   pnp_soft_score_kernel<T, true>    grad_models: the same mapping and walk with the twelve accumulators of h X^T and h weighted by
//     w (1 - w); the model's factor 2 grad_scores[m] (-beta / thr2) is applied once after the point loop.
//   pnp_soft_score_points_kernel<T>   grad_matches, the TRANSPOSED mapping: a lane owns a point, grid (ceil(N / 64), P).  N / 64 alone
//     gives few waves and M reaches 20 480, so a block is kSSWaves waves that share its 64 points and split the models: the block
//     stages 64 kSSWaves models (with 2 grad_scores (-beta / thr2) and a flag) per tile in LDS, wave k walks models k, k + kSSWaves, ...
//     of the tile reading each as a broadcast (a model that keep drops, a non-finite one, a pair without a threshold: flag off, skipped
//     by a wave-uniform branch, so a NaN there reaches nothing), and at the end the waves' partial sums are added in wave order through
//     LDS.  The order of every sum depends on (M, N) and these constants alone: a repeated launch repeats its bytes.
// Every barrier sits under a block-uniform branch (the tile loops' trip counts depend on M, N alone).
#include "compensated_device.hpp"
#include "pair_loss_device.hpp"
#include "pnp_device.hpp"

namespace dr {

constexpr int kSSTile = 256;                  // points staged per tile of the model-lane kernels: 5 KB of LDS in f32, 10 KB in f64
constexpr int kSSWaves = 8;                   // waves per block of the point-lane kernel
constexpr int kSSModels = 64 * kSSWaves;      // models staged per tile there, one per thread: 26.5 KB of LDS in f32, 53 KB in f64
constexpr float kSSCutoff = -40.0f;           // below it a point has no weight (w < 4.3e-18): w (1 - w) / z_c is an exact zero, not 0 inf

// ---- arithmetic beyond the type's precision, where the type's own does not do ------------------------------------------------------
// e = x_c / z_c - u cancels from |u| ~ 0.3 down to a tenth of the threshold's 0.005 and the weight's argument multiplies what is left by
// beta / thr2 = 2e5: in the type's own arithmetic (pnp_loss.hip's) a weight and every gradient term carry hundreds of eps, as much as
// the rounding of the INPUTS to the type moves them -- and a per-row bound of eight times the latter is then met on most rows only
// (docs/LOG.md, 29: two draws of the same size, the tail of their ratio).  So the numerators n = x_c - u z_c are formed beyond the
// type's precision and rounded once: in f32 through f64 (an f64 fma costs what an unpacked f32 fma does), in f64 through the
// compensated dot product of Ogita, Rump and Oishi (Dot2: TwoProduct by fma, TwoSum) -- e = n / z_c is then good to a few eps of ITSELF.
// The error-free transformations must not be contracted (p = a b; s = c + p is not fma(a, b, c) here): contraction is off inside them.
// two_sum and dot2 stand in compensated_device.hpp, which registration_soft_score.hip shares.

// (a_hi + a_lo) - u (z_hi + z_lo), rounded once
template <typename T>
__device__ __forceinline__ T numerator2(T ahi, T alo, T u, T zhi, T zlo) {
#pragma clang fp contract(off)
  const T q = u * zhi;
  const T eq = fma(u, zhi, -q);
  T d, ed;
  two_sum(ahi, -q, d, ed);
  return d + ((ed + alo) - (eq + u * zlo));
}

// x_c, y_c, z_c rounded to the type and the numerators n0 = x_c - u z_c, n1 = y_c - v z_c
__device__ __forceinline__ void camera_forms(const float (&md)[12], const float (&x)[5], float &xc, float &yc, float &zc, float &n0,
                                             float &n1) {
  const double X = x[0], Y = x[1], Z = x[2];
  const double xd = fma((double)md[0], X, fma((double)md[1], Y, fma((double)md[2], Z, (double)md[3])));
  const double yd = fma((double)md[4], X, fma((double)md[5], Y, fma((double)md[6], Z, (double)md[7])));
  const double zd = fma((double)md[8], X, fma((double)md[9], Y, fma((double)md[10], Z, (double)md[11])));
  xc = (float)xd, yc = (float)yd, zc = (float)zd;
  n0 = (float)fma(-(double)x[3], zd, xd);
  n1 = (float)fma(-(double)x[4], zd, yd);
}
__device__ __forceinline__ void camera_forms(const double (&md)[12], const double (&x)[5], double &xc, double &yc, double &zc,
                                             double &n0, double &n1) {
  double xl, yl, zl;
  dot2(&md[0], x, xc, xl);
  dot2(&md[4], x, yc, yl);
  dot2(&md[8], x, zc, zl);
  n0 = numerator2(xc, xl, x[3], zc, zl);
  n1 = numerator2(yc, yl, x[4], zc, zl);
}

// One (model, point) term.  -> w (0 where the point is not live), `live`, and what the gradients need: e, i, (x, y).  nbt = -beta / thr2.
template <typename T>
__device__ __forceinline__ T soft_weight(const T (&md)[12], const T (&x)[5], T nbt, T beta, bool &live, T &e0, T &e1, T &iz, T &xn,
                                         T &yn) {
  T xc, yc, zc, n0, n1;
  camera_forms(md, x, xc, yc, zc, n0, n1);
  iz = T(1) / zc;                                     // (a division: correctly rounded)
  xn = xc * iz, yn = yc * iz;
  e0 = n0 * iz, e1 = n1 * iz;
  const T d2 = fma(e0, e0, e1 * e1);
  const T a = fma(d2, nbt, beta);                     // beta (1 - d2 / thr2)
  live = zc > T(0) && is_finite(d2) && a >= T(kSSCutoff);      // (false for a NaN anywhere)
  return live ? T(1) / (T(1) + exp(-a)) : T(0);
}

// kGrad = false: out = scores [P,M].  kGrad = true: out = grad_models [P,M,16] for the upstream grad_scores [P,M].
template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void pnp_soft_score_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                            const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                            const T *__restrict__ thr2, T beta, const T *__restrict__ grad_scores,
                                                            int M, int N, T *__restrict__ out) {
  __shared__ T s_pt[kSSTile][5];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const T *pt = matches + (size_t)p * N * 5;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);                      // (false for NaN too: the pair then scores 0 and passes nothing)
  const T nbt = thr_ok ? -beta / t2 : T(0);
  // a slot that keep drops is SKIPPED (its model, possibly NaN, is never read); a kept model with a non-finite entry scores 0
  const bool kept = m < M && (!keep || keep[(size_t)p * M + m] != 0);
  T md[12];
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    md[q] = kept ? models[((size_t)p * M + m) * 16 + q] : T(0);
    finite = finite && is_finite(md[q]);
  }
  if (!finite) {
#pragma unroll
    for (int q = 0; q < 12; ++q) md[q] = T(0);        // z_c = 0: no point is live, nothing non-finite is accumulated
  }

  T acc = T(0), acc_lo = T(0), gR[3][3], gt[3];       // acc + acc_lo: the score, summed with TwoSum (40 weights of ~1 in f32:
                                                      // a plain sum walks off by sqrt(N) eps of the score, above the eps N the tests allow)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gt[i] = T(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) gR[i][j] = T(0);
  }

  for (int n0 = 0; n0 < N; n0 += kSSTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kSSTile / 64; ++j) {
      const int n = n0 + j * 64 + lane;
      const bool on = n < N && (!mk || mk[n] != 0);
      const unsigned long long b = __ballot(on);
      const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (on) {
#pragma unroll
        for (int d = 0; d < 5; ++d) s_pt[pos][d] = pt[(size_t)n * 5 + d];
      }
      count += __popcll(b);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < count; ++i) {
      T x[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) x[d] = s_pt[i][d];
      bool live;
      T e0, e1, iz, xn, yn;
      const T w = soft_weight(md, x, nbt, beta, live, e0, e1, iz, xn, yn);
      if (!kGrad) {
        T err;
        two_sum(acc, w, acc, err);
        acc_lo += err;
      } else {
        const T s = w * (T(1) - w);                   // (0 where the point is not live)
        T h[3];
        h[0] = live ? s * (e0 * iz) : T(0);
        h[1] = live ? s * (e1 * iz) : T(0);
        h[2] = live ? -(s * (fma(e0, xn, e1 * yn) * iz)) : T(0);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          gt[r] += h[r];
#pragma unroll
          for (int c = 0; c < 3; ++c) gR[r][c] = fma(h[r], x[c], gR[r][c]);
        }
      }
    }
    __syncthreads();
  }

  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  const bool good = kept && finite && thr_ok;
  if (!kGrad) {
    out[slot] = good ? acc + acc_lo : T(0);
  } else {
    const T sc = good ? T(2) * nbt * grad_scores[slot] : T(0);      // (a dropped slot's grad_scores, possibly NaN, reaches nothing)
    T *g = out + slot * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[4 * r + c] = good ? sc * gR[r][c] : T(0);
      g[4 * r + 3] = good ? sc * gt[r] : T(0);
    }
    g[12] = g[13] = g[14] = g[15] = T(0);
  }
}

// grad_matches [P,N,5]: d / d X = R^T (2 g h), d / d (u, v) = -2 g e, g = grad_scores[m] (-beta / thr2) w (1 - w), over the kept models
template <typename T>
__global__ __launch_bounds__(kSSModels) void pnp_soft_score_points_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                         const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                                         const T *__restrict__ thr2, T beta,
                                                                         const T *__restrict__ grad_scores, int M, int N,
                                                                         T *__restrict__ grad_matches) {
  __shared__ __attribute__((aligned(16))) T s_md[kSSModels][12];
  __shared__ T s_c[kSSModels];
  __shared__ int s_use[kSSModels];
  static_assert(kSSModels * 12 >= kSSWaves * 5 * 64, "the waves' partial sums reuse the model tile");
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * 64 + lane;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);
  const T nbt = thr_ok ? -beta / t2 : T(0);
  const bool have = n < N;
  const bool on = have && (!mask || mask[(size_t)p * N + n] != 0);
  const bool wave_on = __ballot(on) != 0ull;          // a wave without a masked point only keeps the barriers
  T x[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) x[d] = have ? matches[((size_t)p * N + n) * 5 + d] : T(0);
  T acc[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) acc[d] = T(0);

  for (int m0 = 0; m0 < M; m0 += kSSModels) {
    {
      const int m = m0 + tid;
      const size_t slot = (size_t)p * M + m;
      const bool kept = m < M && (!keep || keep[slot] != 0);
      T md[12];
      bool finite = true;
#pragma unroll
      for (int q = 0; q < 12; ++q) {
        md[q] = kept ? models[slot * 16 + q] : T(0);
        finite = finite && is_finite(md[q]);
      }
      const bool use = kept && finite && thr_ok;
      T c = T(0);
      if (use) c = T(2) * nbt * grad_scores[slot];
#pragma unroll
      for (int q = 0; q < 12; ++q) s_md[tid][q] = use ? md[q] : T(0);
      s_c[tid] = c;
      s_use[tid] = use ? 1 : 0;
    }
    __syncthreads();
    const int count = wave_on ? min(kSSModels, M - m0) : 0;
    for (int i = wv; i < count; i += kSSWaves) {
      if (!s_use[i]) continue;                        // (the same word in every lane: the wave skips the model as one)
      T md[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) md[q] = s_md[i][q];
      bool live;
      T e0, e1, iz, xn, yn;
      const T w = soft_weight(md, x, nbt, beta, live, e0, e1, iz, xn, yn);
      const T s = live ? s_c[i] * (w * (T(1) - w)) : T(0);
      const T h0 = live ? s * (e0 * iz) : T(0);
      const T h1 = live ? s * (e1 * iz) : T(0);
      const T h2 = live ? -(s * (fma(e0, xn, e1 * yn) * iz)) : T(0);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fma(md[c], h0, fma(md[4 + c], h1, fma(md[8 + c], h2, acc[c])));
      acc[3] = live ? fma(-s, e0, acc[3]) : acc[3];
      acc[4] = live ? fma(-s, e1, acc[4]) : acc[4];
    }
    __syncthreads();
  }

  // the waves' partial sums, added in wave order
  T *red = &s_md[0][0];
#pragma unroll
  for (int d = 0; d < 5; ++d) red[(wv * 5 + d) * 64 + lane] = acc[d];
  __syncthreads();
  if (wv == 0 && have) {
#pragma unroll
    for (int d = 0; d < 5; ++d) {
      T t = T(0);
#pragma unroll
      for (int k = 0; k < kSSWaves; ++k) t += red[(k * 5 + d) * 64 + lane];
      grad_matches[((size_t)p * N + n) * 5 + d] = on ? t : T(0);      // an unmasked point: exact zeros
    }
  }
}

}  // namespace dr

extern "C" {

#define DR_SOFT_SCORE_BETA(T) DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite")

#define DR_OP(sfx, T)                                                                                                                \
  int dr_pnp_soft_score_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2, T beta,     \
                              int P, int M, int N, T *scores, void *stream) {                                                        \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                 \
    DR_PAIR_LOSS_SIZES;                                                                                                              \
    DR_SOFT_SCORE_BETA(T);                                                                                                           \
    return dr::launch("pnp_soft_score_kernel", dr::pnp_soft_score_kernel<T, false>, dim3((M + 63) / 64, P), 64, stream, matches,      \
                      mask, models, keep, thr2, beta, (const T *)nullptr, M, N, scores);                                             \
  }                                                                                                                                  \
  int dr_pnp_soft_score_bwd_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2, T beta, \
                                  const T *grad_scores, int P, int M, int N, T *grad_models, T *grad_matches, void *stream) {        \
    DR_REQUIRE(matches && models && thr2 && grad_scores && grad_models, "null pointer");                                             \
    DR_PAIR_LOSS_SIZES;                                                                                                              \
    DR_SOFT_SCORE_BETA(T);                                                                                                           \
    if (int rc = dr::launch("pnp_soft_score_kernel", dr::pnp_soft_score_kernel<T, true>, dim3((M + 63) / 64, P), 64, stream,          \
                            matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_models))                                \
      return rc;                                                                                                                     \
    if (!grad_matches) return DR_OK;                  /* matches that need no gradient: the point pass is not launched */           \
    return dr::launch("pnp_soft_score_points_kernel", dr::pnp_soft_score_points_kernel<T>, dim3((N + 63) / 64, P), dr::kSSModels,     \
                      stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_matches);                             \
  }
DR_F32_F64(DR_OP)
#undef DR_OP
#undef DR_SOFT_SCORE_BETA

}  // extern "C"
