// The differentiable soft-inlier score of the pose families (ops.pnp_soft_score, ops.registration_soft_score and the expected pose
// losses on them): every model scored by a sigmoid of its squared residual on every point, with a reverse pass to the models AND to
// the points -- the (model x point) grid with its two reductions.  include/dransac.h states the maths; with the family's squared
// residual d2 and its own further conditions on a point (a Term, below):
//     a = beta (1 - d2 / thr2),   live = d2 finite and a >= -40 [and the family's],   w = live ? 1 / (1 + exp(-a)) : 0,
//     score[m] = sum_{n in mask} w[m,n]
// Three launches, no [P,M,N] tensor, no atomics, no workspace:
//   soft_score_kernel<T, Term, false>   the scores.  The loss kernels' mapping: one LANE per model, one wave per block, grid
//     (ceil(M / 64), P); the masked points compacted tile by tile into LDS in ascending order, each read as a broadcast; the sum in the
//     order of the points.
//   soft_score_kernel<T, Term, true>    grad_models: the same mapping and walk with the twelve accumulators of h x^T and h, h the
//     term's three values weighted by w (1 - w); the model's factor 2 grad_scores[m] (-beta / thr2) is applied once after the
//     point loop.
//   soft_score_points_kernel<T, Term>   grad_matches, the TRANSPOSED mapping: a lane owns a point, grid (ceil(N / 64), P).  N / 64 alone
//     gives few waves and M reaches 20 480, so a block is kSoftWaves waves that share its 64 points and split the models: the block
//     stages 64 kSoftWaves models (with 2 grad_scores (-beta / thr2) and a flag) per tile in LDS, wave k walks models k,
//     k + kSoftWaves, ... of the tile reading each as a broadcast (a model that keep drops, a non-finite one, a pair without a
//     threshold: flag off, skipped by a wave-uniform branch, so a NaN there reaches nothing), and at the end the waves' partial sums
//     are added in wave order through LDS.  The order of every sum depends on (M, N) and these constants alone: a repeated launch
//     repeats its bytes.
// Every barrier sits under a block-uniform branch (the tile loops' trip counts depend on M, N alone).
//
// A family's file keeps its Term: a point is kPoint values of which the first three are the 3-D point the rotation acts on, and
//   Eval<T>                                what one (model, point) pair hands from eval to the hooks, `live` among it
//   T eval(md, x, nbt, beta, Eval<T> &)    -> w; nbt = -beta / thr2.  The residual is formed beyond the type's precision there
//   void model_h(w, ev, h)                 the three h[r] of the model-lane kernel (0 where the point is not live)
//   T point_h(c, w, ev, h)                 the same scaled by the model's *c = 2 grad_scores (-beta / thr2); -> the scale itself.  c
//                                          points into LDS and is read under the term's `live` guard: handed over as a value or a
//                                          reference the read is unconditional, and the point loop loses its branch (docs/LOG.md 32)
//   T tail(ev, s, h, k, a)                 the point-lane accumulator 3 + k (the point's last kPoint - 3 components) after this model
// The accumulators are locals of the kernel bodies and go into no hook by reference: the hooks take and return values.
#pragma once
#include "compensated_device.hpp"
#include "pair_loss_device.hpp"

namespace dr {

constexpr int kSoftTile = 256;                // points staged per tile of the model-lane kernels: 5 | 6 KB of LDS in f32, twice in f64
constexpr int kSoftWaves = 8;                 // waves per block of the point-lane kernel
constexpr int kSoftModels = 64 * kSoftWaves;  // models staged per tile there, one per thread: 28 KB of LDS in f32, 54 KB in f64
constexpr float kSoftCutoff = -40.0f;         // below it a point has no weight (w < 4.3e-18): w (1 - w) times anything is an exact zero

// kGrad = false: out = scores [P,M].  kGrad = true: out = grad_models [P,M,16] for the upstream grad_scores [P,M].
template <typename T, typename Term, bool kGrad>
__global__ __launch_bounds__(64) void soft_score_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                        const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                        const T *__restrict__ thr2, T beta, const T *__restrict__ grad_scores, int M,
                                                        int N, T *__restrict__ out) {
  constexpr int kPoint = Term::kPoint;
  __shared__ T s_pt[kSoftTile][kPoint];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const T *pt = matches + (size_t)p * N * kPoint;
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

  for (int n0 = 0; n0 < N; n0 += kSoftTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kSoftTile / 64; ++j) {
      const int n = n0 + j * 64 + lane;
      const bool on = n < N && (!mk || mk[n] != 0);
      const unsigned long long b = __ballot(on);
      const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (on) {
#pragma unroll
        for (int d = 0; d < kPoint; ++d) s_pt[pos][d] = pt[(size_t)n * kPoint + d];
      }
      count += __popcll(b);
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < count; ++i) {
      T x[kPoint];
#pragma unroll
      for (int d = 0; d < kPoint; ++d) x[d] = s_pt[i][d];
      typename Term::template Eval<T> ev;
      const T w = Term::eval(md, x, nbt, beta, ev);
      if (!kGrad) {
        T err;
        two_sum(acc, w, acc, err);
        acc_lo += err;
      } else {
        T h[3];
        Term::model_h(w, ev, h);
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

// grad_matches [P,N,kPoint]: d / d x[0..2] = R^T h summed over the kept models, the last components by the term's tail
template <typename T, typename Term>
__global__ __launch_bounds__(kSoftModels) void soft_score_points_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                       const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                                       const T *__restrict__ thr2, T beta,
                                                                       const T *__restrict__ grad_scores, int M, int N,
                                                                       T *__restrict__ grad_matches) {
  constexpr int kPoint = Term::kPoint;
  __shared__ __attribute__((aligned(16))) T s_md[kSoftModels][12];
  __shared__ T s_c[kSoftModels];
  __shared__ int s_use[kSoftModels];
  static_assert(kSoftModels * 12 >= kSoftWaves * kPoint * 64, "the waves' partial sums reuse the model tile");
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * 64 + lane;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);
  const T nbt = thr_ok ? -beta / t2 : T(0);
  const bool have = n < N;
  const bool on = have && (!mask || mask[(size_t)p * N + n] != 0);
  const bool wave_on = __ballot(on) != 0ull;          // a wave without a masked point only keeps the barriers
  T x[kPoint];
#pragma unroll
  for (int d = 0; d < kPoint; ++d) x[d] = have ? matches[((size_t)p * N + n) * kPoint + d] : T(0);
  T acc[kPoint];
#pragma unroll
  for (int d = 0; d < kPoint; ++d) acc[d] = T(0);

  for (int m0 = 0; m0 < M; m0 += kSoftModels) {
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
    const int count = wave_on ? min(kSoftModels, M - m0) : 0;
    for (int i = wv; i < count; i += kSoftWaves) {
      if (!s_use[i]) continue;                        // (the same word in every lane: the wave skips the model as one)
      T md[12];
#pragma unroll
      for (int q = 0; q < 12; ++q) md[q] = s_md[i][q];
      typename Term::template Eval<T> ev;
      const T w = Term::eval(md, x, nbt, beta, ev);
      T h[3];
      const T s = Term::point_h(&s_c[i], w, ev, h);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fma(md[c], h[0], fma(md[4 + c], h[1], fma(md[8 + c], h[2], acc[c])));
#pragma unroll
      for (int k = 0; k < kPoint - 3; ++k) acc[3 + k] = Term::tail(ev, s, h, k, acc[3 + k]);
    }
    __syncthreads();
  }

  // the waves' partial sums, added in wave order
  T *red = &s_md[0][0];
#pragma unroll
  for (int d = 0; d < kPoint; ++d) red[(wv * kPoint + d) * 64 + lane] = acc[d];
  __syncthreads();
  if (wv == 0 && have) {
#pragma unroll
    for (int d = 0; d < kPoint; ++d) {
      T t = T(0);
#pragma unroll
      for (int k = 0; k < kSoftWaves; ++k) t += red[(k * kPoint + d) * 64 + lane];
      grad_matches[((size_t)p * N + n) * kPoint + d] = on ? t : T(0);      // an unmasked point: exact zeros
    }
  }
}

}  // namespace dr

// ---- the C entries of one family: dr_<family>_soft_score and dr_<family>_soft_score_bwd ----------------------------------------------
// A family's file stamps them, inside extern "C", with  #define DR_OP(sfx, T) DR_SOFT_SCORE_OP(<family>, dr::<Term>, sfx, T)  under
// DR_F32_F64(DR_OP).
#define DR_SOFT_SCORE_OP(family, Term, sfx, T)                                                                                       \
  int dr_##family##_soft_score_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,      \
                                     T beta, int P, int M, int N, T *scores, void *stream) {                                          \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                  \
    DR_PAIR_LOSS_SIZES;                                                                                                               \
    DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite");                                                \
    return dr::launch(#family "_soft_score_kernel", dr::soft_score_kernel<T, Term, false>, dim3((M + 63) / 64, P), 64, stream,        \
                      matches, mask, models, keep, thr2, beta, (const T *)nullptr, M, N, scores);                                     \
  }                                                                                                                                   \
  int dr_##family##_soft_score_bwd_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,  \
                                         T beta, const T *grad_scores, int P, int M, int N, T *grad_models, T *grad_matches,          \
                                         void *stream) {                                                                              \
    DR_REQUIRE(matches && models && thr2 && grad_scores && grad_models, "null pointer");                                              \
    DR_PAIR_LOSS_SIZES;                                                                                                               \
    DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite");                                                \
    if (int rc = dr::launch(#family "_soft_score_kernel", dr::soft_score_kernel<T, Term, true>, dim3((M + 63) / 64, P), 64, stream,   \
                            matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_models))                                 \
      return rc;                                                                                                                      \
    if (!grad_matches) return DR_OK;                  /* matches that need no gradient: the point pass is not launched */            \
    return dr::launch(#family "_soft_score_points_kernel", dr::soft_score_points_kernel<T, Term>, dim3((N + 63) / 64, P),             \
                      dr::kSoftModels, stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_matches);             \
  }
