// What the homography kernels (homography.hip, homography_loss.hip, homography_soft_score.hip) share.
//   refined_rcp             the reciprocal of the two differentiable kernels: v_rcp_f32 and one Newton step in f32, a division in f64
//   adjugate3_vjp           the transpose of adj's Jacobian (linear in H), applied once per model by the two reverse passes
//   ScoredH / prepare_h     a model slot as the score and update kernels evaluate it: the det > 0 sign applied, adj(H), its kind
//   transfer_d2             the symmetric transfer error of one point -- ONE text for the score kernel, the state step's mask and its
//                           count, every product an explicit fma, so that -ffp-contract has nothing to decide and the three round alike
//   TransferMsacTerm        the MSAC term on it
//   TransferMagsacTerm      the MAGSAC++ term on it: the 4-DoF closed forms of magsac_device.hpp behind the MSAC term's cutoff
//   HomographyGeom          the family's policy for pair_state_device.hpp's score kernel and state step
//   canonical_h             unit Frobenius norm, det > 0; false for a non-finite or singular matrix (solver and refit)
//   denormalise_h           T2^-1 M T1 for the two similarity normalisations (solver and refit)
#pragma once
#include "magsac_device.hpp"
#include "ransac_device.hpp"

namespace dr {

// adj(H) = det(H) H^-1, row-major; adj(-H) = adj(H) for a 3x3 matrix, so the sign rule only touches H itself
template <typename T>
__device__ __forceinline__ void adjugate3(const T (&h)[9], T (&a)[9]) {
  a[0] = fma(h[4], h[8], -(h[5] * h[7]));
  a[1] = fma(h[2], h[7], -(h[1] * h[8]));
  a[2] = fma(h[1], h[5], -(h[2] * h[4]));
  a[3] = fma(h[5], h[6], -(h[3] * h[8]));
  a[4] = fma(h[0], h[8], -(h[2] * h[6]));
  a[5] = fma(h[2], h[3], -(h[0] * h[5]));
  a[6] = fma(h[3], h[7], -(h[4] * h[6]));
  a[7] = fma(h[1], h[6], -(h[0] * h[7]));
  a[8] = fma(h[0], h[4], -(h[1] * h[3]));
}

__device__ __forceinline__ float refined_rcp(float w) {
  const float r = __builtin_amdgcn_rcpf(w);
  return fma(r, fma(-w, r, 1.0f), r);      // (w = 0 or inf gives NaN here: the caller's `live` is false for those)
}
__device__ __forceinline__ double refined_rcp(double w) { return 1.0 / w; }

// out = J^T g for a = adj(h): out[q] = sum_k g[k] d a[k] / d h[q], term by term from adjugate3
template <typename T>
__device__ __forceinline__ void adjugate3_vjp(const T (&h)[9], const T (&g)[9], T (&out)[9]) {
  out[0] = fma(g[4], h[8], fma(-g[5], h[5], fma(-g[7], h[7], g[8] * h[4])));
  out[1] = fma(-g[1], h[8], fma(g[2], h[5], fma(g[7], h[6], -(g[8] * h[3]))));
  out[2] = fma(g[1], h[7], fma(-g[2], h[4], fma(-g[4], h[6], g[5] * h[3])));
  out[3] = fma(-g[3], h[8], fma(g[5], h[2], fma(g[6], h[7], -(g[8] * h[1]))));
  out[4] = fma(g[0], h[8], fma(-g[2], h[2], fma(-g[6], h[6], g[8] * h[0])));
  out[5] = fma(-g[0], h[7], fma(g[2], h[1], fma(g[3], h[6], -(g[5] * h[0]))));
  out[6] = fma(g[3], h[5], fma(-g[4], h[2], fma(-g[6], h[4], g[7] * h[1])));
  out[7] = fma(-g[0], h[5], fma(g[1], h[2], fma(g[6], h[3], -(g[7] * h[0]))));
  out[8] = fma(g[0], h[4], fma(-g[1], h[1], fma(-g[3], h[3], g[4] * h[0])));
}

// One model slot, ready to be evaluated: h = H under the det > 0 sign, a = adj(H), kind as model_kind() has it -- skipped (the slot
// is not live: score exactly 0), scored, or NaN-scoring (a non-finite entry, det == 0 or a non-finite det)
template <typename T>
struct ScoredH {
  T h[9], a[9];
  int kind;
};

template <typename T>
__device__ __forceinline__ void prepare_h(const T *__restrict__ m9, bool live, ScoredH<T> &s) {
  bool finite = true;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    s.h[q] = m9[q];
    finite = finite && is_finite(s.h[q]);
  }
  adjugate3(s.h, s.a);
  const T det = fma(s.h[0], s.a[0], fma(s.h[1], s.a[3], s.h[2] * s.a[6]));
  const bool neg = det < T(0);
#pragma unroll
  for (int q = 0; q < 9; ++q) s.h[q] = neg ? -s.h[q] : s.h[q];
  s.kind = !live ? kModelSkipped : ((finite && is_finite(det) && det != T(0)) ? kModelScored : kModelNan);
}

// d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2, y = H (x1, 1), z = adj(H) (x2, 1); -> are both third coordinates positive (a point
// behind a camera is an outlier whatever its d2).  x = (x1, y1, x2, y2).  Two reciprocals (v_rcp_f32 in f32).
template <typename T>
__device__ __forceinline__ bool transfer_d2(const ScoredH<T> &s, const T (&x)[4], T &d2) {
  const T yx = fma(s.h[0], x[0], fma(s.h[1], x[1], s.h[2]));
  const T yy = fma(s.h[3], x[0], fma(s.h[4], x[1], s.h[5]));
  const T yw = fma(s.h[6], x[0], fma(s.h[7], x[1], s.h[8]));
  const T zx = fma(s.a[0], x[2], fma(s.a[1], x[3], s.a[2]));
  const T zy = fma(s.a[3], x[2], fma(s.a[4], x[3], s.a[5]));
  const T zw = fma(s.a[6], x[2], fma(s.a[7], x[3], s.a[8]));
  const T ry = fast_rcp(yw), rz = fast_rcp(zw);
  const T e0 = fma(-yx, ry, x[2]), e1 = fma(-yy, ry, x[3]);
  const T f0 = fma(-zx, rz, x[0]), f1 = fma(-zy, rz, x[1]);
  d2 = fma(e0, e0, fma(e1, e1, fma(f0, f0, f1 * f1)));
  return yw > T(0) && zw > T(0);
}

// MSAC on it: an inlier (d2 < thr2, false for a NaN or infinite d2) adds 1 - d2 / thr2, never below 0 (d2 < thr2 and d2 * inv >= 1
// can meet by one rounding of inv)
template <typename T>
struct TransferMsacTerm {
  T t2, inv;
  __device__ __forceinline__ explicit TransferMsacTerm(T thr2) : t2(thr2), inv(T(1) / thr2) {}
  __device__ __forceinline__ bool inlier(T d2) const { return d2 < t2; }
  __device__ __forceinline__ T contrib(T d2, bool live = true) const {
    const T sv = fma(-d2, inv, T(1));
    return (live && inlier(d2) && sv > T(0)) ? sv : T(0);
  }
};

// MAGSAC++ on it: the symmetric transfer error is a 4-vector residual, so the weight and the loss are magsac_device.hpp's
// 4-degrees-of-freedom closed forms (Magsac4Term::gain, ::weight) as they stand.  thr2 = threshold^2 is read as (k sigma_max)^2,
// k^2 = chi2.ppf(0.99, 4); s = d2 / thr2.  inlier(d2) is the MSAC term's test, so masks, counts and the adaptive stop are the same
// under either score.  contrib = 1 - l(s), never below 0 (l(1) = 1: at the cutoff the closed form ends within its rounding of 0, and
// d2 < thr2 can meet d2 * inv >= 1 by one rounding of inv); weight = w(s) >= 0, 0 outside the cutoff.
template <typename T>
struct TransferMagsacTerm {
  T t2, inv;
  __device__ __forceinline__ explicit TransferMagsacTerm(T thr2) : t2(thr2), inv(T(1) / thr2) {}
  __device__ __forceinline__ bool inlier(T d2) const { return d2 < t2; }
  __device__ __forceinline__ T contrib(T d2, bool live = true) const {
    const T g = Magsac4Term<T>::gain(d2 * inv);
    return (live && inlier(d2) && g > T(0)) ? g : T(0);
  }
  __device__ __forceinline__ T weight(T d2) const { return inlier(d2) ? Magsac4Term<T>::weight(d2 * inv) : T(0); }
};

template <typename T>
struct alignas(4 * sizeof(T)) Match4 {
  T v[4];
};

// The homography family as pair_state_device.hpp's kernels see it.  A lane's chunk is points c0 + 256 j + tid, so one load instruction
// of a wave reads 64 consecutive points; a slot past the end re-reads the last row and is not live.  Per (model, chunk) the sign rule,
// adj(H) and the slot's kind are worked out once; per point: twelve fma, two reciprocals, one compare for the term and the count.
// Slots: valid = 0 scores exactly 0 (0 inliers) and is never evaluated; a non-finite model or det == 0 scores NaN (0 inliers).  The
// state step replaces the state only on a strictly higher score, in the first round too.
struct HomographyGeom {
  static constexpr int kModel = 9, kWidth = 4, kSample = 4;
  static constexpr bool kFirstRoundTakes = false;
  template <typename T>
  using Slot = ScoredH<T>;
  template <typename T>
  struct Point : Match4<T> {
    static __device__ __forceinline__ Point load(const T *matches, size_t row) {
      return Point{reinterpret_cast<const Match4<T> *>(matches)[row]};
    }
  };
  template <typename T>
  struct Chunk {
    Match4<T> x[8];
    int n0, N;
    __device__ __forceinline__ void load(const T *pt, int c0, int tid, int rowN) {
      n0 = c0 + tid;
      N = rowN;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + j * 256;
        x[j] = reinterpret_cast<const Match4<T> *>(pt)[n < N ? n : N - 1];
      }
    }
    __device__ __forceinline__ bool live(int j) const { return n0 + j * 256 < N; }
    __device__ __forceinline__ const T (&point(int j) const)[4] { return x[j].v; }
  };
  template <typename T>
  static __device__ __forceinline__ int prepare(const T *__restrict__ m9, Slot<T> &s) {
    prepare_h(m9, true, s);
    return s.kind;
  }
  template <typename T>
  static __device__ __forceinline__ int kind(const T *__restrict__ m9, bool live) {
    ScoredH<T> s;
    prepare_h(m9, live, s);
    return s.kind;
  }
  template <typename T>
  static __device__ __forceinline__ T dead_score(int kind) { return kind == kModelNan ? T(NAN) : T(0); }
  template <typename T>
  static __device__ __forceinline__ bool d2(const Slot<T> &s, const T (&x)[4], T &out) { return transfer_d2(s, x, out); }
  template <typename T>
  static __device__ __forceinline__ bool inlier(const Slot<T> &s, const T (&x)[4], T thr2) {
    T d2;
    return transfer_d2(s, x, d2) && d2 < thr2;
  }
};

__device__ __forceinline__ double det3(const double (&h)[9]) {
  return h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
}

// h <- sigma h / |h|_F with sigma = sign(det h); -> false (h = identity) unless `usable`, every entry and the determinant are finite
// and det != 0.  nrm, sigma: what the backward needs.
__device__ __forceinline__ bool canonical_h(double (&h)[9], bool usable, double &nrm, double &sigma) {
  double n2 = 0.0;
  bool ok = usable;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    ok = ok && is_finite(h[q]);
    n2 += h[q] * h[q];
  }
  nrm = sqrt(n2);
  const double r = 1.0 / nrm;
#pragma unroll
  for (int q = 0; q < 9; ++q) h[q] *= r;      // (first the norm, then the determinant: no overflow or underflow from the scale)
  const double det = det3(h);
  sigma = det < 0.0 ? -1.0 : 1.0;
  ok = ok && is_finite(det) && det != 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    h[q] *= sigma;
    ok = ok && is_finite(h[q]);
  }
  if (!ok) {
#pragma unroll
    for (int q = 0; q < 9; ++q) h[q] = (q % 4 == 0) ? 1.0 : 0.0;
  }
  return ok;
}

// H = T2^-1 M T1, T_i = [[s_i, 0, -s_i cx_i], [0, s_i, -s_i cy_i], [0, 0, 1]] (nz = (cx, cy, s) of an image)
__device__ __forceinline__ void denormalise_h(const double (&M)[9], const double (&nz1)[3], const double (&nz2)[3], double (&H)[9]) {
  double G[9];      // M T1
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[3 * i] = M[3 * i] * nz1[2];
    G[3 * i + 1] = M[3 * i + 1] * nz1[2];
    G[3 * i + 2] = M[3 * i + 2] - nz1[2] * (M[3 * i] * nz1[0] + M[3 * i + 1] * nz1[1]);
  }
  const double r2 = 1.0 / nz2[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    H[j] = r2 * G[j] + nz2[0] * G[6 + j];
    H[3 + j] = r2 * G[3 + j] + nz2[1] * G[6 + j];
    H[6 + j] = G[6 + j];
  }
}

}  // namespace dr
