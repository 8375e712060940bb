// What the absolute-pose kernels (pnp.hip) share.
//   matches [P,N,5] = (X, Y, Z, u, v): a world point and its observation in NORMALISED image coordinates (K^-1 applied by the caller).
//   A model is the row-major 4x4 [[R, t], [0, 0, 0, 1]] of the registration family, x_c = R X + t.
//   reproj_d2               d2 = (x_c / z_c - u)^2 + (y_c / z_c - v)^2 of one point -- ONE text for the score kernel, the state step's
//                           mask and its count, every product an explicit fma, so that -ffp-contract has nothing to decide and the
//                           three round alike.  A point with z_c <= 0 does not count at all (HomographyGeom::d2's rule for a point
//                           behind the camera); a non-finite d2 fails every `d2 < thr2` by itself.
//   PnPGeom                 the family's policy for pair_state_device.hpp's score kernel and state step.  The term on d2 is
//                           homography_device.hpp's TransferMsacTerm: MSAC on a squared distance under a cutoff thr2, nothing in it
//                           belongs to the transfer error.
#pragma once
#include "homography_device.hpp"

namespace dr {

template <typename T>
__device__ __forceinline__ bool reproj_d2(const T (&m)[12], const T (&x)[5], T &d2) {
  const T xc = fma(m[0], x[0], fma(m[1], x[1], fma(m[2], x[2], m[3])));
  const T yc = fma(m[4], x[0], fma(m[5], x[1], fma(m[6], x[2], m[7])));
  const T zc = fma(m[8], x[0], fma(m[9], x[1], fma(m[10], x[2], m[11])));
  const T rz = fast_rcp(zc);
  const T e0 = fma(xc, rz, -x[3]), e1 = fma(yc, rz, -x[4]);
  d2 = fma(e0, e0, e1 * e1);
  return zc > T(0);
}

// Slots follow the homography family: valid = 0 scores exactly 0 (0 inliers) and is never evaluated, a model with a non-finite entry
// among its twelve scores NaN (0 inliers); the state step replaces the state only on a strictly higher score, in the first round too.
// A row holds five values, 20 bytes in f32 and 40 in f64: it is not 16-byte aligned, so nothing is loaded as a vector.  Every value
// is one scalar load (global_load_dword / dwordx2) at the row's stride; a lane's chunk is points c0 + 256 j + tid, as in
// HomographyGeom, so the five loads of a wave for one j read the same 64 consecutive rows, 1280 (2560) contiguous bytes, and every
// cache line fetched is used in full across them.  A slot past the end re-reads the last row and is not live.
struct PnPGeom {
  static constexpr int kModel = 16, kWidth = 5, kSample = 3;
  static constexpr bool kFirstRoundTakes = false;
  template <typename T>
  struct Slot {
    T m[12];
  };
  template <typename T>
  struct Point {
    T v[5];
    static __device__ __forceinline__ Point load(const T *matches, size_t row) {
      Point x;
#pragma unroll
      for (int d = 0; d < 5; ++d) x.v[d] = matches[row * 5 + d];
      return x;
    }
  };
  template <typename T>
  struct Chunk {
    T x[8][5];
    int n0, N;
    __device__ __forceinline__ void load(const T *pt, int c0, int tid, int rowN) {
      n0 = c0 + tid;
      N = rowN;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + j * 256;
        const T *r = pt + (size_t)(n < N ? n : N - 1) * 5;
#pragma unroll
        for (int d = 0; d < 5; ++d) x[j][d] = r[d];
      }
    }
    __device__ __forceinline__ bool live(int j) const { return n0 + j * 256 < N; }
    __device__ __forceinline__ const T (&point(int j) const)[5] { return x[j]; }
  };
  template <typename T>
  static __device__ __forceinline__ int prepare(const T *__restrict__ m16, Slot<T> &s) {
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      s.m[q] = m16[q];
      finite = finite && is_finite(s.m[q]);
    }
    return finite ? kModelScored : kModelNan;
  }
  template <typename T>
  static __device__ __forceinline__ int kind(const T *__restrict__ m16, bool live) {
    Slot<T> s;
    return live ? prepare(m16, s) : kModelSkipped;
  }
  template <typename T>
  static __device__ __forceinline__ T dead_score(int kind) { return kind == kModelNan ? T(NAN) : T(0); }
  template <typename T>
  static __device__ __forceinline__ bool d2(const Slot<T> &s, const T (&x)[5], T &out) { return reproj_d2(s.m, x, out); }
  template <typename T>
  static __device__ __forceinline__ bool inlier(const Slot<T> &s, const T (&x)[5], T thr2) {
    T d2;
    return reproj_d2(s.m, x, d2) && d2 < thr2;
  }
};

}  // namespace dr
