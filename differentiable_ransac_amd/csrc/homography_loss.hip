// The training loss of the homography path (loss.HomographyLoss): the truncated symmetric transfer error of EVERY returned model on
// the ground-truth inlier points, value and gradient in one pass over the (model x point) grid -- what registration_loss.hip is for
// the 3-D path.  include/dransac.h states the maths:
//     h = sign(det H) H, a = adj(H), y = h (x1, 1), z = a (x2, 1), e = x2 - y_xy / y_w, f = x1 - z_xy / z_w, d2 = |e|^2 + |f|^2
//     live = y_w > 0 and z_w > 0 and d2 < thr2,   term = live ? d2 / thr2 : 1,   sums[m] = sum_{n in mask} term[m,n]
// Mapping (registration_loss_kernel's): one LANE per model (9 + 9 model registers, 1 + 1 + 18 accumulators), one wave per block, grid
// (ceil(M / 64), P).  The wave compacts the pair's masked points tile by tile into LDS, in ascending order, and every lane walks the
// tile reading each point as an LDS broadcast: no cross-lane reduction, no atomics, and the order of every sum is the order of the
// points -- a repeated launch repeats bit for bit.  The grid is arithmetic-bound (~70 vector instructions per model x masked point
// with the gradient); a tile's staging is ~1 % of its arithmetic, so the tile is sized by the LDS it may take, not by the staging.
//
// Gradient.  With t = y_xy / y_w:  d d2 / d y = (2 / y_w) (-e_0, -e_1, e . t), and d d2 / d h = that (x) (x1, 1); the same for z, a and
// x2.  The two outer products are accumulated separately (gh, ga: nine sums each).  adj is quadratic in H, so the transpose of its
// Jacobian is linear in H and is applied ONCE per model after the point loop (adjugate3_vjp); the sign of the determinant and
// 2 / thr2 come last: grad = sign (2 / thr2) (gh + J_adj(h)^T ga).
//
// The reciprocal.  transfer_d2 takes v_rcp_f32 as it comes (1 ulp), which is fine for a score: there the reciprocal's error is one
// more rounding of d2.  Here the gradient is a sum of e / y_w terms in which e = x2 - y_xy / y_w cancels from |x2| ~ 10^2..10^3 pixels
// down to the threshold's few pixels, so an ulp of the reciprocal is ~|x2| / |e| ulps of the term, as much as the three fma of the
// linear form together.  One Newton step r <- r + r (1 - w r) (two fma out of ~70 instructions) brings the f32 reciprocal within
// half an ulp and a bit, and the kernel's error to that of the linear forms alone; f64 divides.  d2 is then not transfer_d2's value
// to the last bit, only to the reciprocal's ulp: `live` agrees with HomographyGeom::inlier wherever d2 / thr2 is farther from 1, and
// y_w, z_w farther from 0, than the rounding of either evaluation, which is the guarantee the two paths can give each other (the
// signs of y_w and z_w, computed by the same fma in the same order, agree always).  The ground-truth mask (pair_gt_mask_kernel)
// IS HomographyGeom::inlier: bit for bit the mask dr_homography_update writes for the same model.
#include "homography_device.hpp"
#include "pair_loss_device.hpp"

namespace dr {

// points staged per tile: 4 KB of LDS in f32, 8 KB in f64.  One wave per block and ~2.5 blocks per SIMD at a train step's shape: the
// LDS of a tile never limits the occupancy (160 KB per CU), and 256 keeps the staging (four loads per lane and tile) at ~1 %
constexpr int kHLTile = 256;

template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void homography_loss_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                             const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                             const T *__restrict__ thr2, int M, int N, T *__restrict__ sums,
                                                             T *__restrict__ grad) {
  __shared__ Match4<T> s_pt[kHLTile];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const Match4<T> *pt = reinterpret_cast<const Match4<T> *>(matches) + (size_t)p * N;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);                      // (false for NaN too: every point then takes the truncated branch)
  // a slot that keep drops is SKIPPED (its model, possibly NaN, is never read); a kept model that prepare_h calls NaN-scoring (a
  // non-finite entry, det == 0, a non-finite det) is "bad": every masked point counts 1 and nothing flows back
  const bool kept = m < M && (!keep || keep[(size_t)p * M + m] != 0);
  T raw[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) raw[q] = kept ? models[((size_t)p * M + m) * 9 + q] : T(0);
  ScoredH<T> s;
  prepare_h(raw, kept, s);
  const bool scored = s.kind == kModelScored;
  // prepare_h has turned h to det > 0; the gradient is turned back at the end (adj(-H) = adj(H): a needs no sign)
  const bool neg = fma(raw[0], s.a[0], fma(raw[1], s.a[3], raw[2] * s.a[6])) < T(0);
  if (!scored) {
#pragma unroll
    for (int q = 0; q < 9; ++q) s.h[q] = s.a[q] = T(0);      // y_w = z_w = 0: no point is live, nothing non-finite is accumulated
  }

  T acc = T(0), gh[9], ga[9];
  int truncated = 0, n_mask = 0;
#pragma unroll
  for (int q = 0; q < 9; ++q) gh[q] = ga[q] = T(0);

  for (int n0 = 0; n0 < N; n0 += kHLTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kHLTile / 64; ++j) {
      const int n = n0 + j * 64 + lane;
      const bool on = n < N && (!mk || mk[n] != 0);
      const unsigned long long b = __ballot(on);
      const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (on) s_pt[pos] = pt[n];
      count += __popcll(b);
    }
    __syncthreads();
    n_mask += count;
#pragma unroll 2
    for (int i = 0; i < count; ++i) {
      const Match4<T> xv = s_pt[i];
      const T(&x)[4] = xv.v;
      const T yx = fma(s.h[0], x[0], fma(s.h[1], x[1], s.h[2]));
      const T yy = fma(s.h[3], x[0], fma(s.h[4], x[1], s.h[5]));
      const T yw = fma(s.h[6], x[0], fma(s.h[7], x[1], s.h[8]));
      const T zx = fma(s.a[0], x[2], fma(s.a[1], x[3], s.a[2]));
      const T zy = fma(s.a[3], x[2], fma(s.a[4], x[3], s.a[5]));
      const T zw = fma(s.a[6], x[2], fma(s.a[7], x[3], s.a[8]));
      const T ry = refined_rcp(yw), rz = refined_rcp(zw);
      const T e0 = fma(-yx, ry, x[2]), e1 = fma(-yy, ry, x[3]);
      const T f0 = fma(-zx, rz, x[0]), f1 = fma(-zy, rz, x[1]);
      const T d2 = fma(e0, e0, fma(e1, e1, fma(f0, f0, f1 * f1)));
      const bool live = yw > T(0) && zw > T(0) && d2 < t2;      // strict; false for a NaN distance
      acc += live ? d2 : T(0);
      truncated += live ? 0 : 1;
      if (kGrad) {
        // (1 / y_w) (-e_0, -e_1, e . t) with t = y_xy / y_w, and the same for z; the 2 is applied with 1 / thr2 at the end
        const T u0 = live ? -(e0 * ry) : T(0), u1 = live ? -(e1 * ry) : T(0);
        const T u2 = live ? fma(e0, yx * ry, e1 * (yy * ry)) * ry : T(0);
        const T v0 = live ? -(f0 * rz) : T(0), v1 = live ? -(f1 * rz) : T(0);
        const T v2 = live ? fma(f0, zx * rz, f1 * (zy * rz)) * rz : T(0);
        gh[0] = fma(u0, x[0], gh[0]), gh[1] = fma(u0, x[1], gh[1]), gh[2] += u0;
        gh[3] = fma(u1, x[0], gh[3]), gh[4] = fma(u1, x[1], gh[4]), gh[5] += u1;
        gh[6] = fma(u2, x[0], gh[6]), gh[7] = fma(u2, x[1], gh[7]), gh[8] += u2;
        ga[0] = fma(v0, x[2], ga[0]), ga[1] = fma(v0, x[3], ga[1]), ga[2] += v0;
        ga[3] = fma(v1, x[2], ga[3]), ga[4] = fma(v1, x[3], ga[4]), ga[5] += v1;
        ga[6] = fma(v2, x[2], ga[6]), ga[7] = fma(v2, x[3], ga[7]), ga[8] += v2;
      }
    }
    __syncthreads();
  }

  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  const bool good = kept && scored && thr_ok;
  const T inv = thr_ok ? T(1) / t2 : T(0);
  sums[slot] = !kept ? T(0) : (good ? fma(acc, inv, (T)truncated) : (T)n_mask);
  if (kGrad) {
    T back[9];
    adjugate3_vjp(s.h, ga, back);
    const T sc = good ? (neg ? T(-2) : T(2)) * inv : T(0);
    T *g = grad + slot * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) g[q] = good ? sc * (gh[q] + back[q]) : T(0);
  }
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T) DR_PAIR_LOSS_OP(homography, dr::HomographyGeom, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
