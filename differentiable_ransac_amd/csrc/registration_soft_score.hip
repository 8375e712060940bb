// The soft-inlier score of the registration path (ops.registration_soft_score, loss.RegistrationExpectedLoss): the rigid term of
// soft_score_device.hpp's kernels, which has the mappings and the launches, on the registration loss's residual:
//     d = R p + t - q,  d2 = |d|^2
// grad_matches [P,N,6]: d / d p = R^T (g d), d / d q = -g d, g = 2 grad_scores[m] (-beta / thr2) w (1 - w), over the kept models
#include "soft_score_device.hpp"

namespace dr {

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
  live = is_finite(d2) && a >= T(kSoftCutoff);        // (false for a NaN anywhere)
  const T ex = exp(-a);
  const T w = live ? T(1) / (T(1) + ex) : T(0);
  s = live ? w * (ex * w) : T(0);
  return w;
}

struct RigidSoftTerm {
  static constexpr int kPoint = 6;
  template <typename T>
  struct Eval {
    bool live;
    T d[3], s;
  };
  template <typename T>
  static __device__ __forceinline__ T eval(const T (&md)[12], const T (&x)[6], T nbt, T beta, Eval<T> &ev) {
    return soft_weight(md, x, nbt, beta, ev.live, ev.d, ev.s);
  }
  template <typename T>
  static __device__ __forceinline__ void model_h(T w, const Eval<T> &ev, T (&h)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = ev.live ? ev.s * ev.d[r] : T(0);
  }
  template <typename T>
  static __device__ __forceinline__ T point_h(const T *c, T w, const Eval<T> &ev, T (&h)[3]) {
    const T g = ev.live ? *c * ev.s : T(0);
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = ev.live ? g * ev.d[r] : T(0);
    return g;
  }
  template <typename T>
  static __device__ __forceinline__ T tail(const Eval<T> &ev, T g, const T (&h)[3], int k, T a) {
    return a - h[k];                                  // d / d q
  }
};

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T) DR_SOFT_SCORE_OP(registration, dr::RigidSoftTerm, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
