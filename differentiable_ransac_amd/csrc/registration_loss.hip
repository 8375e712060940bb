// The training loss of the robust 3-D registration path (loss.RegistrationLoss): the truncated squared distance of EVERY returned
// model on the ground-truth inlier points, value and gradient in one pass over the (model x point) grid -- what dr_match_loss_fused
// is for the two-view path.  Nothing upstream computes this (include/dransac.h states the maths):
//     d2[m,n] = |R_m p_n + t_m - q_n|^2,   e[m,n] = d2 < thr2 ? d2 / thr2 : 1,   sums[m] = sum_{n in mask} e[m,n]
// Mapping: one LANE per model (12 model registers, 1 + 1 + 12 accumulators), one wave per block.  The wave compacts the pair's
// masked points tile by tile into LDS, in ascending order, and every lane walks the tile reading each point as an LDS broadcast: no
// cross-lane reduction, no atomics, and the order of every sum is the order of the points -- a repeated launch repeats bit for bit.
// The grid is arithmetic-bound (~38 vector instructions per model x masked point); a tile's staging is ~1 % of its arithmetic.
#include "pair_loss_device.hpp"
#include "rigid_device.hpp"

namespace dr {

constexpr int kRLTile = 256;      // points staged per tile: 6 KB of LDS in f32, 12 KB in f64

template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void registration_loss_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                               const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                               const T *__restrict__ thr2, int M, int N, T *__restrict__ sums,
                                                               T *__restrict__ grad) {
  __shared__ T s_pt[kRLTile][6];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const T *pt = matches + (size_t)p * N * 6;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);                      // (false for NaN too: every point then takes the truncated branch)
  // a slot that keep drops is SKIPPED (its model, possibly NaN, is never read); a kept model with a non-finite entry is "bad": every
  // masked point counts 1 and nothing flows back
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
    for (int q = 0; q < 12; ++q) md[q] = T(0);
  }

  T acc = T(0), gR[3][3], gt[3];
  int truncated = 0, n_mask = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gt[i] = T(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) gR[i][j] = T(0);
  }

  for (int n0 = 0; n0 < N; n0 += kRLTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kRLTile / 64; ++j) {
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
    n_mask += count;
#pragma unroll 4
    for (int i = 0; i < count; ++i) {
      T x[6], e[3];
#pragma unroll
      for (int d = 0; d < 6; ++d) x[d] = s_pt[i][d];
      // e = q - t - R p, started from q - t so that the partial results shrink towards e: the roundings are of |q - t|, |R_0 p_0 + e|
      // and |e|, not of |t| and |R p + t| as in rigid_d2's q - (R p + t).  The gradient is a sum of e p^T, and for a model with a
      // handful of live points the cancellation in e is its whole error: 3-10 x smaller this way on the test scenes (docs/LOG.md)
      T d2 = T(0);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        e[r] = fma(-md[4 * r], x[0], fma(-md[4 * r + 1], x[1], fma(-md[4 * r + 2], x[2], x[3 + r] - md[4 * r + 3])));
        d2 = fma(e[r], e[r], d2);
      }
      const bool live = d2 < t2;                      // strict; false for a NaN distance
      acc += live ? d2 : T(0);
      truncated += live ? 0 : 1;
      if (kGrad) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const T el = live ? e[r] : T(0);
          gt[r] += el;
#pragma unroll
          for (int c = 0; c < 3; ++c) gR[r][c] = fma(el, x[c], gR[r][c]);
        }
      }
    }
    __syncthreads();
  }

  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  const bool good = kept && finite && thr_ok;
  const T inv = thr_ok ? T(1) / t2 : T(0);
  sums[slot] = !kept ? T(0) : (good ? fma(acc, inv, (T)truncated) : (T)n_mask);
  if (kGrad) {
    // e = q - (R p + t) = -r: d sums / d R = (2 / thr2) sum r p^T, d sums / d t = (2 / thr2) sum r, over the live points
    const T sc = good ? T(-2) * inv : T(0);
    T *g = grad + slot * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[4 * r + c] = good ? sc * gR[r][c] : T(0);
      g[4 * r + 3] = good ? sc * gt[r] : T(0);
    }
    g[12] = g[13] = g[14] = g[15] = T(0);
  }
}

}  // namespace dr

extern "C" {

// (the ground-truth mask is |R p + t - q|^2 < thr2[p]: RigidGeom::inlier = rigid_d2, the score kernels' inlier test)
#define DR_OP(sfx, T) DR_PAIR_LOSS_OP(registration, dr::RigidGeom, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
