// The two-view MAGSAC++ term, shared by the scoring kernels (magsac_score.hip) and the IRLS polish (refit.hip): the
// constants, the closed forms and Magsac4Term, which has SampsonMsacTerm's interface (ransac_device.hpp: the distance, the cutoff
// and the block score pass live there).
//
// d2 = the squared Sampson distance of K4 (sampson_d2); thr2 = (1.5 thr)^2, K4's and K6's own cutoff, read as (k sigma_max)^2 with
// k^2 = chi2.ppf(0.99, 4) = 13.276704135987622 (the residual has 4 degrees of freedom), the noise scale uniform in [0, sigma_max].
// With s = d2 / thr2, u = u_k s, u_k = k^2 / 2, Gamma_k = Gamma(3/2, u_k), Gamma_0 = Gamma(3/2) = sqrt(pi) / 2, rho_1 = gamma(5/2, u_k):
//   weight  w(s) = (Gamma(3/2, u) - Gamma_k) / (Gamma_0 - Gamma_k)                       for s < 1, else 0
//   loss    l(s) = (u Gamma(3/2, u) + gamma(5/2, u) - u Gamma_k) / rho_1                 for s < 1, else 1
//   score        = sum_n (1 - l(s_n)),  inliers = #{s_n < 1};  a non-finite d2 contributes nothing.
// Closed forms, F(u) = Gamma_0 erfc(sqrt u), q(u) = sqrt(u) exp(-u):
//   Gamma(3/2, u) = G = F + q
//   rho(u) = u Gamma(3/2, u) + gamma(5/2, u) - u Gamma_k = u (F - Gamma_k) - (3/2) G + 3 sqrt(pi) / 4     (the u^(3/2) e^-u terms cancel)
// so one erfc, one exp and one sqrt serve the weight and the loss.  They are the device library's (OCML) erfc / exp / sqrt of the type;
// tests/magsac_ref.py derives the evaluation error of a term from their ulp bounds.
#pragma once
#include "ransac_device.hpp"

namespace dr {

constexpr double kM4Uk = 6.638352067993811;            // k^2 / 2
constexpr double kM4GammaK = 0.0036112606177586;       // Gamma(3/2, u_k)
constexpr double kM4Gamma0 = 0.88622692545275801365;   // Gamma(3/2) = sqrt(pi) / 2
constexpr double kM4R0 = 1.32934038817913702047;       // 3 sqrt(pi) / 4 = Gamma(5/2)
constexpr double kM4Rho1 = 1.3015316073311318;         // gamma(5/2, u_k)

__device__ __forceinline__ float magsac4_erfc(float x) { return erfcf(x); }
__device__ __forceinline__ double magsac4_erfc(double x) { return erfc(x); }
__device__ __forceinline__ float magsac4_exp(float x) { return expf(x); }
__device__ __forceinline__ double magsac4_exp(double x) { return exp(x); }
__device__ __forceinline__ float magsac4_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double magsac4_sqrt(double x) { return sqrt(x); }

template <typename T>
struct Magsac4Term {
  T inv;      // 1 / thr2, thr2 = (1.5 thr)^2: the MSAC term's cutoff
  __device__ __forceinline__ explicit Magsac4Term(T thr) : inv(SampsonMsacTerm<T>(thr).inv) {}
  __device__ __forceinline__ T ratio(T d2) const { return d2 * inv; }                 // s
  __device__ __forceinline__ static bool inlier(T s) { return s < T(1); }             // (false for NaN): the term's and the count's test
  // Gamma(3/2, u_k s) and F - Gamma_k of the closed form
  __device__ __forceinline__ static void gammas(T s, T &u, T &G, T &Fk) {
    u = s * (T)kM4Uk;
    const T x = magsac4_sqrt(u);
    const T F = (T)kM4Gamma0 * magsac4_erfc(x);
    G = fma(x, magsac4_exp(-u), F);
    Fk = F - (T)kM4GammaK;
  }
  __device__ __forceinline__ static T gain(T s) {                                     // 1 - l(s) where inlier(s)
    T u, G, Fk;
    gammas(s, u, G, Fk);
    const T rho = fma(u, Fk, fma((T)-1.5, G, (T)kM4R0));
    return fma(rho, (T)(-1.0 / kM4Rho1), T(1));
  }
  __device__ __forceinline__ static T weight(T s) {                                   // w(s) where inlier(s); >= 0
    T u, G, Fk;
    gammas(s, u, G, Fk);
    const T w = (G - (T)kM4GammaK) * (T)(1.0 / (kM4Gamma0 - kM4GammaK));
    return w > T(0) ? w : T(0);
  }
  __device__ __forceinline__ T contrib(T d2, bool live = true) const {
    const T s = ratio(d2);
    return (live && inlier(s)) ? gain(s) : T(0);
  }
};

}  // namespace dr
