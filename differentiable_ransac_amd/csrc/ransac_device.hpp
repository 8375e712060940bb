// Per-point and per-pair pieces of the test-mode loops that several launches share.  Two-view (the v2f / splat typedefs of the packed
// form sit in namespace dr for every file that includes this one):
//   sampson_d2 / sampson_s, sampson_d2_pair   the squared Sampson distance, scalar and two points at a time (v_pk_fma_f32)
//   SampsonMsacTerm                           the MSAC rule on it (scoring, update, refit acceptance, local optimisation); its
//                                             MAGSAC++ sibling Magsac4Term, same interface, is magsac_device.hpp's
//   model_kind                                is a model slot evaluated, skipped, or does it score NaN
//   score_partial / block_score               the score of one model over all points of a pair: a thread's share, the whole block
// Two-view and 3-D:
//   adaptive_max_iters                        the adaptive stop of ransac.py:202-215
//   argmax_merge / block_arg_best             the first arg-best over a pair's scores of the selection and update kernels (2-D and 3-D)
#pragma once
#include "dr_common.hpp"

namespace dr {

// squared Sampson distance: a = M^T x2 ; b = M x1 (first two) ; r = x1 . a       (msac_score.py:33-39)
template <typename T>
__device__ __forceinline__ T sampson_d2(const T m[9], T x1, T y1, T x2, T y2) {
  const T a0 = fma(x2, m[0], fma(y2, m[3], m[6]));
  const T a1 = fma(x2, m[1], fma(y2, m[4], m[7]));
  const T a2 = fma(x2, m[2], fma(y2, m[5], m[8]));
  const T b0 = fma(x1, m[0], fma(y1, m[1], m[2]));
  const T b1 = fma(x1, m[3], fma(y1, m[4], m[5]));
  const T r = fma(x1, a0, fma(y1, a1, a2));
  const T jj = fma(a0, a0, fma(a1, a1, fma(b0, b0, b1 * b1)));
  return (r * r) * fast_rcp(jj);
}

// s = d2/thr2 - 1 ; inlier <=> s < 0 ; soft score = max(-s, 0)
template <typename T>
__device__ __forceinline__ T sampson_s(const T m[9], T x1, T y1, T x2, T y2, T inv_thr2) {
  return fma(sampson_d2<T>(m, x1, y1, x2, y2), inv_thr2, T(-1));
}

// sampson_d2 of a point PAIR, f32: every FMA one v_pk_fma_f32.  ms[q] = the model coefficient q in both halves (an SGPR broadcast
// through op_sel, or a VGPR pair)
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f splat(float a) { return (v2f){a, a}; }
__device__ __forceinline__ v2f sampson_d2_pair(v2f x1, v2f y1, v2f x2, v2f y2, const v2f (&ms)[9]) {
  const v2f a0 = x2 * ms[0] + (y2 * ms[3] + ms[6]);
  const v2f a1 = x2 * ms[1] + (y2 * ms[4] + ms[7]);
  const v2f a2 = x2 * ms[2] + (y2 * ms[5] + ms[8]);
  const v2f b0 = x1 * ms[0] + (y1 * ms[1] + ms[2]);
  const v2f b1 = x1 * ms[3] + (y1 * ms[4] + ms[5]);
  const v2f r = x1 * a0 + (y1 * a1 + a2);
  const v2f jj = a0 * a0 + (a1 * a1 + (b0 * b0 + b1 * b1));
  const v2f rr = r * r;
  v2f rc;
  rc[0] = __builtin_amdgcn_rcpf(jj[0]);
  rc[1] = __builtin_amdgcn_rcpf(jj[1]);
  return rr * rc;
}

// The two-view MSAC term on d2.  Constructed from the pair's threshold: the one place that forms the cutoff (1.5 thr)^2, which
// Magsac4Term reads as its own.  Interface of both terms: ratio(d2) -> s, inlier(s), contrib(d2, live = true).
template <typename T>
struct SampsonMsacTerm {
  T inv;      // 1 / thr2, thr2 = (1.5 thr)^2
  __device__ __forceinline__ explicit SampsonMsacTerm(T thr) {
    const T t = T(1.5) * thr;
    inv = T(1) / (t * t);
  }
  __device__ __forceinline__ T ratio(T d2) const { return fma(d2, inv, T(-1)); }      // s = d2 / thr2 - 1
  __device__ __forceinline__ static bool inlier(T s) { return s < T(0); }             // (false for NaN)
  // max(-s, 0); a 0/0 point (NaN) contributes 0.  `live` (the point exists) is joined to the predicate here, not wrapped round
  // the call: LOG 19
  __device__ __forceinline__ T contrib(T d2, bool live = true) const {
    const T s = ratio(d2);
    return (live && inlier(s)) ? -s : T(0);
  }
};

// One model slot: skipped (the slot is not live: score exactly 0, nothing evaluated), scored, or NaN-scoring (a non-finite model, or
// -- unless zero_is_nan is false -- an all-zero one, the reference's 0/0: it is given a NaN score and never competes)
enum ModelKind : int { kModelSkipped = 0, kModelScored = 1, kModelNan = 2 };
template <typename T>
__device__ __forceinline__ int model_kind(const T *__restrict__ m9, bool live, bool zero_is_nan = true) {
  if (!live) return kModelSkipped;
  bool finite = true, nonzero = !zero_is_nan;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    finite = finite && is_finite(m9[q]);
    nonzero = nonzero || (m9[q] != T(0));
  }
  return (finite && nonzero) ? kModelScored : kModelNan;
}

// this thread's share (points tid, tid + kStride, ...) of the score of model m under `term` over the N points mt [N,4] of one pair
template <typename T, int kStride, typename Term>
__device__ __forceinline__ T score_partial(const T *__restrict__ mt, const T (&m)[9], int N, const Term &term) {
  T acc = T(0);
  for (int n = threadIdx.x; n < N; n += kStride) {
    const T *q = mt + (size_t)n * 4;
    acc += term.contrib(sampson_d2<T>(m, q[0], q[1], q[2], q[3]));
  }
  return acc;
}

// The score by the whole block of kThreads threads; every thread returns it.  Order: a thread's points in order, the wave butterfly,
// the waves in order.  s_part: shared, kThreads / 64 entries, free again on return (two barriers).
template <typename T, int kThreads, typename Term>
__device__ __forceinline__ T block_score(const T *__restrict__ mt, const T (&m)[9], int N, const Term &term, T *s_part) {
  T acc = wave_sum(score_partial<T, kThreads>(mt, m, N, term));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  T sc = s_part[0];
#pragma unroll
  for (int w = 1; w < kThreads / kWave; ++w) sc += s_part[w];
  __syncthreads();
  return sc;
}

// adaptive_iteration_number (ransac.py:202-215) capped at max_iterations (ransac.py:135-142), in f64
__device__ __forceinline__ double adaptive_max_iters(int inliers, int N, int k, double confidence, double eps,
                                                     int max_iterations) {
  const double ratio = (double)inliers / (double)N;
  const double rk = pow(ratio, (double)k);
  const double prob = 1.0 - rk;
  double nmi = (double)max_iterations;
  if (!(prob >= 1.0 - eps)) nmi = fmax(0.0, log10(1.0 - confidence) / log10(1.0 - rk + eps));
  return fmin((double)max_iterations, nmi);
}

// (bv, bi) <- the better of (bv, bi) and (ov, oi): the larger value (kMax = false: the smaller), the lower index on a tie
template <typename T, bool kMax = true>
__device__ __forceinline__ void argmax_merge(T &bv, int &bi, T ov, int oi) {
  if ((kMax ? ov > bv : ov < bv) || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// First arg-best of row[0 .. M) over the entries that are valid (valid == NULL: all of them) and not NaN, by a block of kThreads
// threads: strided scan, wave butterfly, ONE __syncthreads(), then every thread merges the wave results itself, so all threads
// return the same (bv, bi).  bi = 0x7fffffff: no entry qualifies.  s_val, s_idx: shared, kThreads / 64 entries each.
template <typename T, int kThreads, bool kMax>
__device__ __forceinline__ void block_arg_best(const T *__restrict__ row, const uint8_t *__restrict__ valid, int M, T *s_val,
                                               int *s_idx, T &bv, int &bi) {
  bv = kMax ? -INFINITY : INFINITY;
  bi = 0x7fffffff;
  for (int m = threadIdx.x; m < M; m += kThreads) {
    const T v = row[m];
    if ((!valid || valid[m]) && v == v) argmax_merge<T, kMax>(bv, bi, v, m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) argmax_merge<T, kMax>(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
  if ((threadIdx.x & 63) == 0) { s_val[threadIdx.x >> 6] = bv; s_idx[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = s_val[0]; bi = s_idx[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) argmax_merge<T, kMax>(bv, bi, s_val[w], s_idx[w]);
}

}  // namespace dr
