// Per-point and per-pair pieces of the test-mode loop that several launches share: the Sampson / MSAC rule of the scoring,
// update, refit-acceptance and local-optimisation kernels, the adaptive stop of ransac.py:202-215, and the first arg-best over a
// pair's scores of the selection and update kernels (2-D and 3-D).
#pragma once
#include "dr_common.hpp"

namespace dr {

template <typename T>
__device__ __forceinline__ T sampson_s(const T m[9], T x1, T y1, T x2, T y2, T inv_thr2) {
  // a = M^T x2 ; b = M x1 (first two) ; r = x1 . a       (msac_score.py:33-39)
  T a0 = fma(x2, m[0], fma(y2, m[3], m[6]));
  T a1 = fma(x2, m[1], fma(y2, m[4], m[7]));
  T a2 = fma(x2, m[2], fma(y2, m[5], m[8]));
  T b0 = fma(x1, m[0], fma(y1, m[1], m[2]));
  T b1 = fma(x1, m[3], fma(y1, m[4], m[5]));
  T r = fma(x1, a0, fma(y1, a1, a2));
  T jj = fma(a0, a0, fma(a1, a1, fma(b0, b0, b1 * b1)));
  T d2 = (r * r) * fast_rcp(jj);
  return fma(d2, inv_thr2, T(-1));  // s = d2/thr2 - 1 ; inlier <=> s < 0 ; soft score = max(-s, 0)
}

// this thread's share (points tid, tid + kStride, ...) of the MSAC score of model m over the N points of one pair
template <typename T, int kStride>
__device__ __forceinline__ T msac_partial(const T *__restrict__ mp, const T (&m)[9], int N, T inv_thr2) {
  T acc = T(0);
  for (int n = threadIdx.x; n < N; n += kStride) {
    const T *q = mp + (size_t)n * 4;
    const T sv = sampson_s<T>(m, q[0], q[1], q[2], q[3], inv_thr2);
    acc += (sv < T(0)) ? -sv : T(0);      // a 0/0 point (NaN) contributes 0, as in the scoring kernel
  }
  return acc;
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
