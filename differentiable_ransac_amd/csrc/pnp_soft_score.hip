// The soft-inlier score of the absolute-pose path (ops.pnp_soft_score, loss.PnPExpectedLoss): the reprojection term of
// soft_score_device.hpp's kernels, which has the mappings and the launches.  The residual is pnp_loss.hip's with 1 / z_c a division,
// its numerators formed beyond the type's precision (below: the gradient is a sum of e i terms with the loss's cancellation):
//     x_c = R X + t,  i = 1 / z_c,  (x, y) = (x_c, y_c) i,  e = (x - u, y - v),  d2 = |e|^2;  live also needs z_c > 0
// grad_matches [P,N,5]: d / d X = R^T (2 g h), d / d (u, v) = -2 g e, g = grad_scores[m] (-beta / thr2) w (1 - w), over the kept models
#include "pnp_device.hpp"
#include "soft_score_device.hpp"

namespace dr {

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
  live = zc > T(0) && is_finite(d2) && a >= T(kSoftCutoff);      // (false for a NaN anywhere)
  return live ? T(1) / (T(1) + exp(-a)) : T(0);
}

struct PnPSoftTerm {
  static constexpr int kPoint = 5;
  template <typename T>
  struct Eval {
    bool live;
    T e0, e1, iz, xn, yn;
  };
  template <typename T>
  static __device__ __forceinline__ T eval(const T (&md)[12], const T (&x)[5], T nbt, T beta, Eval<T> &ev) {
    return soft_weight(md, x, nbt, beta, ev.live, ev.e0, ev.e1, ev.iz, ev.xn, ev.yn);
  }
  template <typename T>
  static __device__ __forceinline__ void model_h(T w, const Eval<T> &ev, T (&h)[3]) {
    const bool live = ev.live;
    const T e0 = ev.e0, e1 = ev.e1, iz = ev.iz, xn = ev.xn, yn = ev.yn;
    const T s = w * (T(1) - w);                   // (0 where the point is not live)
    h[0] = live ? s * (e0 * iz) : T(0);
    h[1] = live ? s * (e1 * iz) : T(0);
    h[2] = live ? -(s * (fma(e0, xn, e1 * yn) * iz)) : T(0);
  }
  template <typename T>
  static __device__ __forceinline__ T point_h(const T *c, T w, const Eval<T> &ev, T (&h)[3]) {
    const bool live = ev.live;
    const T e0 = ev.e0, e1 = ev.e1, iz = ev.iz, xn = ev.xn, yn = ev.yn;
    const T s = live ? *c * (w * (T(1) - w)) : T(0);
    h[0] = live ? s * (e0 * iz) : T(0);
    h[1] = live ? s * (e1 * iz) : T(0);
    h[2] = live ? -(s * (fma(e0, xn, e1 * yn) * iz)) : T(0);
    return s;
  }
  template <typename T>
  static __device__ __forceinline__ T tail(const Eval<T> &ev, T s, const T (&h)[3], int k, T a) {
    return ev.live ? fma(-s, k == 0 ? ev.e0 : ev.e1, a) : a;      // d / d (u, v)
  }
};

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T) DR_SOFT_SCORE_OP(pnp, dr::PnPSoftTerm, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
