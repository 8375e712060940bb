// Device pieces the two 3-D kernel families share (solve_rigid.hip: parity with the reference; registration.hip: robust
// registration): both work on row-major 4x4 models [[R, t], [0, 0, 0, 1]] and 6-column correspondences (p, q).
#pragma once
#include "ransac_device.hpp"

namespace dr {

// d2 = |q - (R p + t)|^2 of one point under one model: the ONE form of every residual, score and best-mask kernel except the packed
// rigid_residual_kernel_f32_pk, so a winner's mask equals its row of the masks and its inlier count bit for bit
template <typename T>
__device__ __forceinline__ T rigid_d2(const T (&m)[12], const T (&x)[6]) {
  T d2 = T(0);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const T pred = fma(m[4 * i], x[0], fma(m[4 * i + 1], x[1], fma(m[4 * i + 2], x[2], m[4 * i + 3])));
    const T e = x[3 + i] - pred;
    d2 = fma(e, e, d2);
  }
  return d2;
}

// points n0 .. n0 + 7 of a row of N (zeros past the end) -> how many of them exist
template <typename T>
__device__ __forceinline__ int load_points8(const T *pt, int n0, int N, T (&x)[8][6]) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int d = 0; d < 6; ++d) x[j][d] = (n0 + j < N) ? pt[(size_t)(n0 + j) * 6 + d] : T(0);
  return min(8, max(0, N - n0));
}

// The rigid family as pair_state_device.hpp's kernels see it.  Residual: d2 = |q - (R p + t)|^2 (rigid_d2); every point may count.
// A lane's chunk is 8 CONSECUTIVE points (load_points8: zeros past the end, live = j < nvalid).  Nothing of a model is classified:
// a slot with valid = 0 scores -1 (0 inliers), every other one is evaluated as it stands, so a NaN model scores 0.  The state step
// takes the first round's best whatever it scores.
struct RigidGeom {
  static constexpr int kModel = 16, kWidth = 6, kSample = 3;
  static constexpr bool kFirstRoundTakes = true;
  template <typename T>
  struct Slot {
    T m[12];
  };
  template <typename T>
  struct Point {
    T v[6];
    static __device__ __forceinline__ Point load(const T *matches, size_t row) {
      Point x;
#pragma unroll
      for (int d = 0; d < 6; ++d) x.v[d] = matches[row * 6 + d];
      return x;
    }
  };
  template <typename T>
  struct Chunk {
    T x[8][6];
    int nvalid;
    __device__ __forceinline__ void load(const T *pt, int c0, int tid, int N) { nvalid = load_points8(pt, c0 + tid * 8, N, x); }
    __device__ __forceinline__ bool live(int j) const { return j < nvalid; }
    __device__ __forceinline__ const T (&point(int j) const)[6] { return x[j]; }
  };
  template <typename T>
  static __device__ __forceinline__ int prepare(const T *__restrict__ m16, Slot<T> &s) {
#pragma unroll
    for (int q = 0; q < 12; ++q) s.m[q] = m16[q];
    return kModelScored;
  }
  template <typename T>
  static __device__ __forceinline__ int kind(const T *, bool live) { return live ? kModelScored : kModelSkipped; }
  template <typename T>
  static __device__ __forceinline__ T dead_score(int) { return T(-1); }
  template <typename T>
  static __device__ __forceinline__ bool d2(const Slot<T> &s, const T (&x)[6], T &out) {
    out = rigid_d2<T>(s.m, x);
    return true;
  }
  template <typename T>
  static __device__ __forceinline__ bool inlier(const Slot<T> &s, const T (&x)[6], T thr2) { return rigid_d2<T>(s.m, x) < thr2; }
};

template <typename T>
__device__ __forceinline__ void store_rigid_model(T *__restrict__ m, const double (&R)[3][3], const double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[4 * i + j] = (T)R[i][j];
    m[4 * i + 3] = (T)t[i];
  }
  m[12] = m[13] = m[14] = T(0);
  m[15] = T(1);
}

// what a sample or selection without a usable model gets (with valid = 0)
__device__ __forceinline__ void set_identity(double (&R)[3][3], double (&t)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = (i == j);
  }
}

__device__ __forceinline__ void gram3(const double (&A)[3][3], double (&ata)[3][3]) {   // A^T A
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) ata[i][j] = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j];
}

__device__ __forceinline__ void swap_if(bool sw, double &a, double &b) {
  const double x = a, y = b;
  a = sw ? y : x;
  b = sw ? x : y;
}
__device__ __forceinline__ void swap_if(bool sw, double (&a)[3], double (&b)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) swap_if(sw, a[i], b[i]);
}

// the three-compare network: key descending, the rows of every companion triple follow their keys
template <typename... V>
__device__ __forceinline__ void sort3_desc(double (&key)[3], V &...rows) {
  auto step = [&](int i, int j) {
    const bool sw = key[i] < key[j];
    swap_if(sw, key[i], key[j]);
    (swap_if(sw, rows[i], rows[j]), ...);
  };
  step(0, 1);
  step(1, 2);
  step(0, 1);
}

// R = [v0 v1 v0xv1][u0 u1 u0xu1]^T of two orthonormal pairs: a proper rotation without a determinant fix -> is every entry finite
__device__ __forceinline__ bool rotation_from_frames(const double (&v0)[3], const double (&v1)[3], const double (&u0)[3],
                                                     const double (&u1)[3], double (&R)[3][3]) {
  const double v2[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
  const double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R[i][j] = v0[i] * u0[j] + v1[i] * u1[j] + v2[i] * u2[j];
      finite = finite && is_finite(R[i][j]);
    }
  return finite;
}

}  // namespace dr
