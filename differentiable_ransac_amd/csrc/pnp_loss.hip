// The training loss of the absolute-pose path (loss.PnPLoss): the truncated squared reprojection error of EVERY returned pose on the
// ground-truth inlier points, value and gradient in one pass over the (model x point) grid -- what registration_loss.hip is for the
// 3-D path and homography_loss.hip for the homographies.  include/dransac.h states the maths:
//     x_c = R X + t,  i = 1 / z_c,  (x, y) = (x_c, y_c) i,  e = (x - u, y - v),  d2 = |e|^2
//     live = z_c > 0 and d2 < thr2,   term = live ? d2 / thr2 : 1,   sums[m] = sum_{n in mask} term[m,n]
// Mapping (registration_loss_kernel's): one LANE per model (12 model registers, 1 + 1 + 12 accumulators), one wave per block, grid
// (ceil(M / 64), P).  The wave compacts the pair's masked points tile by tile into LDS, in ascending order, and every lane walks the
// tile reading each point as an LDS broadcast: no cross-lane reduction, no atomics, and the order of every sum is the order of the
// points -- a repeated launch repeats bit for bit.
//
// Gradient.  d d2 / d x_c = 2 (e_0 i, e_1 i, -(e_0 x + e_1 y) i) =: 2 h, so per live point d / d t += h and d / d R += h X^T; the
// factor 2 / thr2 is applied once per model after the point loop.  Row 3 of the gradient is zero.
//
// The reciprocal.  reproj_d2 takes v_rcp_f32 as it comes (1 ulp), which is fine for a score.  Here the gradient is a sum of e i terms
// in which e = x_c i - u cancels from |u| ~ 0.1 down to the threshold's 0.005, so an ulp of the reciprocal is tens of ulps of the
// term; the kernel divides (1 / z_c correctly rounded in either type).  d2 is then not reproj_d2's value to the last bit, only to the
// reciprocal's ulp: `live` agrees with PnPGeom::inlier wherever d2 / thr2 is farther from 1 than the rounding of either evaluation
// (the sign of z_c, the same fma chain in both, agrees always).  The ground-truth mask (pair_gt_mask_kernel) IS PnPGeom::inlier: bit
// for bit the mask dr_pnp_update writes for the same model.
#include "pair_loss_device.hpp"
#include "pnp_device.hpp"

namespace dr {

constexpr int kPLTile = 256;      // points staged per tile: 5 KB of LDS in f32, 10 KB in f64

template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void pnp_loss_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                      const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                      const T *__restrict__ thr2, int M, int N, T *__restrict__ sums,
                                                      T *__restrict__ grad) {
  __shared__ T s_pt[kPLTile][5];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const T *pt = matches + (size_t)p * N * 5;
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
    for (int q = 0; q < 12; ++q) md[q] = T(0);        // z_c = 0: no point is live, nothing non-finite is accumulated
  }

  T acc = T(0), gR[3][3], gt[3];
  int truncated = 0, n_mask = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gt[i] = T(0);
#pragma unroll
    for (int j = 0; j < 3; ++j) gR[i][j] = T(0);
  }

  for (int n0 = 0; n0 < N; n0 += kPLTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kPLTile / 64; ++j) {
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
    n_mask += count;
#pragma unroll 4
    for (int i = 0; i < count; ++i) {
      T x[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) x[d] = s_pt[i][d];
      // (reproj_d2's linear forms, the same fma chains: the sign of z_c is the score kernels')
      const T xc = fma(md[0], x[0], fma(md[1], x[1], fma(md[2], x[2], md[3])));
      const T yc = fma(md[4], x[0], fma(md[5], x[1], fma(md[6], x[2], md[7])));
      const T zc = fma(md[8], x[0], fma(md[9], x[1], fma(md[10], x[2], md[11])));
      const T iz = T(1) / zc;
      const T xn = xc * iz, yn = yc * iz;
      const T e0 = xn - x[3], e1 = yn - x[4];
      const T d2 = fma(e0, e0, e1 * e1);
      const bool live = zc > T(0) && d2 < t2;         // strict; false for a NaN distance
      acc += live ? d2 : T(0);
      truncated += live ? 0 : 1;
      if (kGrad) {
        T h[3];
        h[0] = live ? e0 * iz : T(0);
        h[1] = live ? e1 * iz : T(0);
        h[2] = live ? -(fma(e0, xn, e1 * yn) * iz) : T(0);
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
  const T inv = thr_ok ? T(1) / t2 : T(0);
  sums[slot] = !kept ? T(0) : (good ? fma(acc, inv, (T)truncated) : (T)n_mask);
  if (kGrad) {
    const T sc = good ? T(2) * inv : T(0);
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

// (the ground-truth mask is PnPGeom::inlier: reproj_d2 < thr2[p] in front of the camera, the score kernels' inlier test)
#define DR_OP(sfx, T) DR_PAIR_LOSS_OP(pnp, dr::PnPGeom, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
