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
//   jacobi_eig12_wave       the eigen-decomposition of the DLT's 12x12 Gram matrix by one wave, in LDS.
//   nearest_rotation3       M (3x3) -> the rotation nearest to it in the Frobenius norm, and M's mean singular value.
#pragma once
#include "homography_device.hpp"
#include "rigid_device.hpp"
#include "solver_common.hpp"

namespace dr {

// Parallel cyclic Jacobi for ONE symmetric 12x12 matrix held in LDS (A, V: 144 doubles each, row-major), executed by one whole wave:
// jacobi_eig9_wave's two-phase round (solver_common.hpp states it) at the size of the DLT.  It is not that routine with a size
// parameter: the 9x9 one is written around an odd size (nine rounds, the index r rests in round r) and one matrix element per lane,
// and the refits of the benchmark's path run it; here the size is even, so the round-robin has thirteen players of which the last is
// a phantom -- partner i' = (2 r - i) mod 13, an index whose partner is itself or the phantom rests: five or six disjoint rotations
// per round, thirteen rounds per sweep -- and a lane owns two of the 78 upper-triangle elements and three of V's 144.  The rotation,
// the update formulas, the stopping rule (off-diagonal mass at 2e-30 of the diagonal's, or stagnation after four sweeps; 30 sweeps
// at most) and the fences are the 9x9 routine's.  On return the diagonal of A holds the eigenvalues, the columns of V the
// eigenvectors.  `cs` = 24 doubles of LDS scratch.
__device__ __forceinline__ void jacobi_eig12_wave(double *A, double *V, double *cs, int lane) {
  constexpr int n = 12, m = 13, kTri = 78, kAll = 144;
  double *C = cs, *S = cs + n;
  for (int i = lane; i < kAll; i += 64) V[i] = (i % (n + 1) == 0) ? 1.0 : 0.0;
  int ui[2], uj[2];      // this lane's elements lane, lane + 64 of the row-major upper triangle
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    int rem = lane + 64 * e < kTri ? lane + 64 * e : 0, i = 0;
    while (rem >= n - i) { rem -= n - i; ++i; }
    ui[e] = i;
    uj[e] = i + rem;
  }
  // the partner of index i in round r, i itself when it rests
  auto partner = [&](int r, int i) {
    const int ip = (2 * r - i + 2 * m) % m;
    return ip == n ? i : ip;
  };
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  double prev_off = INFINITY;
#pragma unroll 1
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0, dg = 0;
    for (int i = lane; i < kAll; i += 64) {
      const double v = A[i] * A[i];
      if (i % (n + 1) == 0) dg += v; else off += v;
    }
    off = wave_sum(off);
    dg = wave_sum(dg);
    if (!(off > 2e-30 * dg) || (sweep >= 4 && off > 0.25 * prev_off)) break;
    prev_off = off;
#pragma unroll 1
    for (int r = 0; r < m; ++r) {
      if (lane < n) {
        const int i = lane, ip = partner(r, i);
        double c = 1.0, ss = 0.0;
        if (ip != i) {
          const int p = min(i, ip), q = max(i, ip);
          const double apq = A[p * n + q];
          if (fabs(apq) > 1e-300) {
            const double a = A[q * n + q] - A[p * n + p], b2 = 2.0 * apq;
            const double r2 = fma(a, a, b2 * b2);
            const double rr = r2 * rsqrt_nr(r2);
            const double t = (a >= 0 ? b2 : -b2) * rcp_nr(fabs(a) + rr);
            c = rsqrt_nr(fma(t, t, 1.0));
            const double sn = t * c;
            ss = (i < ip) ? -sn : sn;
          }
        }
        C[i] = c;
        S[i] = ss;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
      double na[2] = {0.0, 0.0}, nv[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (lane + 64 * e < kTri) {
          const int i = ui[e], j = uj[e], ip = partner(r, i), jp = partner(r, j);
          const double ci = C[i], si = S[i], cj = C[j], sj = S[j];
          const double rij = fma(si, A[ip * n + j], ci * A[i * n + j]);
          const double rijp = fma(si, A[ip * n + jp], ci * A[i * n + jp]);
          na[e] = fma(sj, rijp, cj * rij);
        }
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int f = lane + 64 * e;
        if (f < kAll) {
          const int k = f / n, j = f % n, jp = partner(r, j);
          nv[e] = fma(S[j], V[k * n + jp], C[j] * V[k * n + j]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (lane + 64 * e < kTri) {
          A[ui[e] * n + uj[e]] = na[e];
          A[uj[e] * n + ui[e]] = na[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (lane + 64 * e < kAll) V[lane + 64 * e] = nv[e];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// The rotation nearest to M in the Frobenius norm, R = U diag(1, 1, det(U V^T)) V^T of M = U S V^T, from rigid_device.hpp's pieces as
// the registration fit builds its own: jacobi_eig3 of M^T M, right vectors by descending eigenvalue, left vectors M v by Gram-Schmidt,
// the third ones by cross products (rotation_from_frames: proper without a determinant fix).  mean_sv = tr(R^T M) / 3, the mean of
// M's singular values with the smallest one signed by det M.  It serves a starting pose: M is a scaled rotation up to the noise, so the
// squared conditioning of M^T M costs nothing here.  false: a non-finite entry, or a second singular value below 1e-12 of the first.
__device__ __forceinline__ bool nearest_rotation3(const double (&M)[3][3], double (&R)[3][3], double &mean_sv) {
  double ata[3][3], V[3][3], ev[3], v[3][3], g[3][3];
  gram3(M, ata);
  jacobi_eig3(ata, V, ev);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[c][k] = V[k][c];
  sort3_desc(ev, v);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) g[c][k] = M[k][0] * v[c][0] + M[k][1] * v[c][1] + M[k][2] * v[c][2];
  const double s1sq = g[0][0] * g[0][0] + g[0][1] * g[0][1] + g[0][2] * g[0][2], r0 = 1.0 / sqrt(s1sq);
  double u0[3], u1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) u0[k] = g[0][k] * r0;
  const double du = u0[0] * g[1][0] + u0[1] * g[1][1] + u0[2] * g[1][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) u1[k] = g[1][k] - du * u0[k];
  const double s2sq = u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2], r1 = 1.0 / sqrt(s2sq);
  bool ok = s2sq > 1e-24 * s1sq;      // (false for NaN and for s1sq = 0)
#pragma unroll
  for (int k = 0; k < 3; ++k) u1[k] *= r1;
  ok = rotation_from_frames(u0, u1, v[0], v[1], R) && ok;
  mean_sv = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) mean_sv += R[i][j] * M[i][j];
  mean_sv *= 1.0 / 3.0;
  return ok && is_finite(mean_sv);
}

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
