// Error-free transformations for the kernels that form a cancelling residual beyond the type's precision and round it once
// (pnp_soft_score.hip, registration_soft_score.hip): TwoSum, and the compensated dot product of Ogita, Rump and Oishi (Dot2: TwoProduct
// by fma, TwoSum).  They must not be contracted (p = a b; s = c + p is not fma(a, b, c) here): contraction is off inside them.
#pragma once
#include "dr_common.hpp"

namespace dr {

template <typename T>
__device__ __forceinline__ void two_sum(T a, T b, T &s, T &e) {
#pragma clang fp contract(off)
  s = a + b;
  const T bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// hi + lo = m[0] x[0] + m[1] x[1] + m[2] x[2] + m[3] to about twice the type's precision (x: a point's row, its first three entries)
template <typename T, int K>
__device__ __forceinline__ void dot2(const T *m, const T (&x)[K], T &hi, T &lo) {
#pragma clang fp contract(off)
  static_assert(K >= 3, "a point has three coordinates");
  T s = m[3], c = T(0);
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    const T p = m[k] * x[k];
    const T ep = fma(m[k], x[k], -p);
    T es;
    two_sum(s, p, s, es);
    c += ep + es;
  }
  hi = s, lo = c;
}

}  // namespace dr
