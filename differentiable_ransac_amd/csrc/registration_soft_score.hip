// The differentiable soft-inlier score of the registration path (ops.registration_soft_score, loss.RegistrationExpectedLoss): every
// rigid model scored by a sigmoid of its squared distance on every correspondence, with a reverse pass to the models AND to the
// points -- pnp_soft_score.hip's (model x point) grid with its two reductions, on the registration loss's residual.  include/dransac.h
// states the maths:
//     d = R p + t - q,  d2 = |d|^2,  a = beta (1 - d2 / thr2)
//     live = d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0,   score[m] = sum_{n in mask} w[m,n]
// Three launches, no [P,M,N] tensor, no atomics, no workspace:
//   registration_soft_score_kernel<T, false>   the scores.  registration_loss_kernel's mapping: one LANE per model, one wave per block,
//     grid (ceil(M / 64), P); the masked points compacted tile by tile into LDS in ascending order, each read as a broadcast; the sum
//     in the order of the points.
//   registration_soft_score_kernel<T, true>    grad_models: the same mapping and walk with the twelve accumulators of h p^T and h,
//     h = w (1 - w) d; the model's factor 2 grad_scores[m] (-beta / thr2) is applied once after the point loop.
//   registration_soft_score_points_kernel<T>   grad_matches, the TRANSPOSED mapping: a lane owns a point, grid (ceil(N / 64), P).  A
//     block is kRSWaves waves that share its 64 points and split the models: the block stages 64 kRSWaves models (with
//     2 grad_scores (-beta / thr2) and a flag) per tile in LDS, wave k walks models k, k + kRSWaves, ... of the tile reading each as a
//     broadcast (a model that keep drops, a non-finite one, a pair without a threshold: flag off, skipped by a wave-uniform branch,
//     so a NaN there reaches nothing), and at the end the waves' partial sums are added in wave order through LDS.  The order of every
//     sum depends on (M, N) and these constants alone: a repeated launch repeats its bytes.
// Every barrier sits under a block-uniform branch (the tile loops' trip counts depend on M, N alone).
#include "compensated_device.hpp"
#include "pair_loss_device.hpp"

namespace dr {

constexpr int kRSTile = 256;                  // points staged per tile of the model-lane kernels: 6 KB of LDS in f32, 12 KB in f64
constexpr int kRSWaves = 8;                   // waves per block of the point-lane kernel
constexpr int kRSModels = 64 * kRSWaves;      // models staged per tile there, one per thread: 28 KB of LDS in f32, 54 KB in f64
constexpr float kRSCutoff = -40.0f;           // below it a point has no weight (w < 4.3e-18)

// ---- the residual beyond the type's precision -------------------------------------------------------------------------------------
// d = R p + t - q cancels from |q| ~ 1 down to a fraction of the threshold's 0.05 and the weight's argument multiplies what is left
// by beta / thr2 = 2000: as in pnp_soft_score.hip the cancelling form is computed beyond the type's precision and rounded once, in
// f32 through f64 fma chains, in f64 through Dot2 and a TwoSum of the difference -- d is then good to an eps of ITSELF.
__device__ __forceinline__ float residual_row(const float *m, const float (&x)[6], int r) {
  const double s = fma((double)m[0], (double)x[0], fma((double)m[1], (double)x[1], fma((double)m[2], (double)x[2], (double)m[3])));
  return (float)(s - (double)x[3 + r]);
}
__device__ __forceinline__ double residual_row(const double *m, const double (&x)[6], int r) {
#pragma clang fp contract(off)
  double hi, lo, d, e;
  dot2(m, x, hi, lo);
  two_sum(hi, -x[3 + r], d, e);
  return d + (e + lo);
}

// One (model, point) term.  -> w (0 where the point is not live), `live`, d, and s = w (1 - w) (0 where the point is not live).
// nbt = -beta / thr2.  1 - w is formed as exp(-a) w: no cancellation on the sigmoid's flat top.
template <typename T>
__device__ __forceinline__ T soft_weight(const T (&md)[12], const T (&x)[6], T nbt, T beta, bool &live, T (&d)[3], T &s) {
#pragma unroll
  for (int r = 0; r < 3; ++r) d[r] = residual_row(&md[4 * r], x, r);
  const T d2 = fma(d[0], d[0], fma(d[1], d[1], d[2] * d[2]));
  const T a = fma(d2, nbt, beta);                     // beta (1 - d2 / thr2)
  live = is_finite(d2) && a >= T(kRSCutoff);          // (false for a NaN anywhere)
  const T ex = exp(-a);
  const T w = live ? T(1) / (T(1) + ex) : T(0);
  s = live ? w * (ex * w) : T(0);
  return w;
}

// kGrad = false: out = scores [P,M].  kGrad = true: out = grad_models [P,M,16] for the upstream grad_scores [P,M].
template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void registration_soft_score_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                     const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                                     const T *__restrict__ thr2, T beta,
                                                                     const T *__restrict__ grad_scores, int M, int N,
                                                                     T *__restrict__ out) {
  __shared__ T s_pt[kRSTile][6];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const T *pt = matches + (size_t)p * N * 6;
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
    for (int q = 0; q < 12; ++q) md[q] = T(0);        // nothing non-finite is accumulated; the lane's result is dropped below
  }

  T acc = T(0), acc_lo = T(0), gR[3][3], gt[3];       // acc + acc_lo: the score, summed with TwoSum (a plain f32 sum of N weights of
                                                      // ~1 walks off by sqrt(N) eps of the score, above the eps N the tests allow)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gt[i] = T(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) gR[i][j] = T(0);
  }

  for (int n0 = 0; n0 < N; n0 += kRSTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kRSTile / 64; ++j) {
      const int n = n0 + j * 64 + lane;
      const bool on = n < N && (!mk || mk[n] != 0);
      const unsigned long long b = __ballot(on);
      const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (on) {
#pragma unroll
        for (int d = 0; d < 6; ++d) s_pt[pos][d] = pt[(size_t)n * 6 + d];
      }
      count += __popcll(b);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < count; ++i) {
      T x[6], d[3], s;
#pragma unroll
      for (int c = 0; c < 6; ++c) x[c] = s_pt[i][c];
      bool live;
      const T w = soft_weight(md, x, nbt, beta, live, d, s);
      if (!kGrad) {
        T err;
        two_sum(acc, w, acc, err);
        acc_lo += err;
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const T h = live ? s * d[r] : T(0);
          gt[r] += h;
#pragma unroll
          for (int c = 0; c < 3; ++c) gR[r][c] = fma(h, x[c], gR[r][c]);
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

// grad_matches [P,N,6]: d / d p = R^T (g d), d / d q = -g d, g = 2 grad_scores[m] (-beta / thr2) w (1 - w), over the kept models
template <typename T>
__global__ __launch_bounds__(kRSModels) void registration_soft_score_points_kernel(
    const T *__restrict__ matches, const uint8_t *__restrict__ mask, const T *__restrict__ models, const uint8_t *__restrict__ keep,
    const T *__restrict__ thr2, T beta, const T *__restrict__ grad_scores, int M, int N, T *__restrict__ grad_matches) {
  __shared__ __attribute__((aligned(16))) T s_md[kRSModels][12];
  __shared__ T s_c[kRSModels];
  __shared__ int s_use[kRSModels];
  static_assert(kRSModels * 12 >= kRSWaves * 6 * 64, "the waves' partial sums reuse the model tile");
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * 64 + lane;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);
  const T nbt = thr_ok ? -beta / t2 : T(0);
  const bool have = n < N;
  const bool on = have && (!mask || mask[(size_t)p * N + n] != 0);
  const bool wave_on = __ballot(on) != 0ull;          // a wave without a masked point only keeps the barriers
  T x[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) x[d] = have ? matches[((size_t)p * N + n) * 6 + d] : T(0);
  T acc[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) acc[d] = T(0);

  for (int m0 = 0; m0 < M; m0 += kRSModels) {
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
    const int count = wave_on ? min(kRSModels, M - m0) : 0;
    for (int i = wv; i < count; i += kRSWaves) {
      if (!s_use[i]) continue;                        // (the same word in every lane: the wave skips the model as one)
      T md[12], d[3], s;
#pragma unroll
      for (int q = 0; q < 12; ++q) md[q] = s_md[i][q];
      bool live;
      soft_weight(md, x, nbt, beta, live, d, s);
      const T g = live ? s_c[i] * s : T(0);
      T h[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) h[r] = live ? g * d[r] : T(0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        acc[c] = fma(md[c], h[0], fma(md[4 + c], h[1], fma(md[8 + c], h[2], acc[c])));
        acc[3 + c] -= h[c];
      }
    }
    __syncthreads();
  }

  // the waves' partial sums, added in wave order
  T *red = &s_md[0][0];
#pragma unroll
  for (int d = 0; d < 6; ++d) red[(wv * 6 + d) * 64 + lane] = acc[d];
  __syncthreads();
  if (wv == 0 && have) {
#pragma unroll
    for (int d = 0; d < 6; ++d) {
      T t = T(0);
#pragma unroll
      for (int k = 0; k < kRSWaves; ++k) t += red[(k * 6 + d) * 64 + lane];
      grad_matches[((size_t)p * N + n) * 6 + d] = on ? t : T(0);      // an unmasked point: exact zeros
    }
  }
}

}  // namespace dr

extern "C" {

#define DR_SOFT_SCORE_BETA(T) DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite")

#define DR_OP(sfx, T)                                                                                                               \
  int dr_registration_soft_score_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,   \
                                       T beta, int P, int M, int N, T *scores, void *stream) {                                      \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                \
    DR_PAIR_LOSS_SIZES;                                                                                                             \
    DR_SOFT_SCORE_BETA(T);                                                                                                          \
    return dr::launch("registration_soft_score_kernel", dr::registration_soft_score_kernel<T, false>, dim3((M + 63) / 64, P), 64,    \
                      stream, matches, mask, models, keep, thr2, beta, (const T *)nullptr, M, N, scores);                           \
  }                                                                                                                                 \
  int dr_registration_soft_score_bwd_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep,              \
                                           const T *thr2, T beta, const T *grad_scores, int P, int M, int N, T *grad_models,        \
                                           T *grad_matches, void *stream) {                                                         \
    DR_REQUIRE(matches && models && thr2 && grad_scores && grad_models, "null pointer");                                            \
    DR_PAIR_LOSS_SIZES;                                                                                                             \
    DR_SOFT_SCORE_BETA(T);                                                                                                          \
    if (int rc = dr::launch("registration_soft_score_kernel", dr::registration_soft_score_kernel<T, true>, dim3((M + 63) / 64, P),   \
                            64, stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_models))                   \
      return rc;                                                                                                                    \
    if (!grad_matches) return DR_OK;                  /* matches that need no gradient: the point pass is not launched */          \
    return dr::launch("registration_soft_score_points_kernel", dr::registration_soft_score_points_kernel<T>,                        \
                      dim3((N + 63) / 64, P), dr::kRSModels, stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N,    \
                      grad_matches);                                                                                                \
  }
DR_F32_F64(DR_OP)
#undef DR_OP
#undef DR_SOFT_SCORE_BETA

}  // extern "C"
