// The reverse pass of the weighted eight-point fit (dr_refit_fundamental, refit.hip: refit_fundamental_pair): gF -> the gradient of
// the rows and of their weights (dr_refit_fundamental_bwd; ops.weighted_fundamental).
// The forward, per pair, over the rows the mask selects (nsel of them): mu[4] their centroids, r_i = sqrt(2) nsel / D_i,
// D_i = sum |q_n| of image i, q_n = X_n - mu (Hartley's transforms, UNWEIGHTED); p1 = (x1, y1, 1) = normalised image-1 point, p2 likewise;
// rho_n = vec(p2 p1^T) (epipolar_row_f), G = sum w_n^2 rho_n rho_n^T (the weights scale the ROWS), fh = the eigenvector of G's
// smallest eigenvalue, F = T2^T mat(fh) T1, T_i = [[r, 0, -r mu_x], [0, r, -r mu_y], [0, 0, 1]].  No rank-2 projection, no unit norm.
// Nothing is stored by the forward.  This file restates its three passes (centroids, mean distances, Gram matrix) stage by stage, with
// its expressions and its reduction orders, and runs the same Jacobi (solver_common.hpp) on the result: fh has the forward's bits, and
// with them the forward's SIGN -- gF refers to F as the forward returned it, and every output here is odd in fh.  The stages are a copy
// and not a shared header on purpose: the two-view kernels of refit.hip are pinned byte for byte, and lifting code out of that file has
// changed how its refit bodies compile before (refit.hip, PairRefit).  Backwards:
//   F = T2^T mat(fh) T1         g_fh = T2 gF T1^T;  gT1 = (T2^T mat(fh))^T gF, gT2 = (mat(fh) T1) gF^T give the direct gradients of
//                               (mu_x, mu_y, r) of each image: g_r = gT[0][0] + gT[1][1] - mu_x gT[0][2] - mu_y gT[1][2], g_mu = -r gT[.][2]
//   fh = v_0(G)                 z = sum_{i != 0} v_i (v_i . g_fh) / (lambda_i - lambda_0):  dL = -z^T dG fh,  gG = -(z fh^T + fh z^T) / 2
//   G = sum w^2 rho rho^T       s_n = -(rho_n . z)(rho_n . fh) = -(p2^T Z p1)(p2^T Fh p1):  dL/dw_n = 2 w_n s_n, and w_n^2 ds_n/d(x1, y1, x2, y2)
//                               is the row's normalised-coordinate gradient gx_n
//   x = (X - mu) r              per image: g_mu = -r sum gx (+ direct), g_r = sum (gx . x) / r (+ direct)
//   r = sqrt(2) nsel / D        g_D = -g_r r / D;  the centroid sits inside every |q_n|: g_mu -= g_D sum q_n / |q_n|;  a row gets
//                               r gx_n + g_D q_n / |q_n| + g_mu / nsel  (q_n / |q_n| := 0 for a row at the centroid)
// Mapping: the forward's -- one 256-thread block per pair, f64 inside for either type, thread n owns rows n, n + 256, ....  Wave 0
// hands fh, z and the six direct gradients to the block through LDS; pass A reduces ten sums; pass B writes every row of every requested
// output: exact zeros for rows the mask drops (never loaded) and for every row of a pair with nsel < 8, valid = 0,
// lambda_i - lambda_0 not positive and finite for some i != 0, or a non-finite z, direct gradient, g_D or g_mu -- one block-uniform
// decision.  Every step is linear in gF and rounds symmetrically: -gF negates every output bit for bit.  No atomics, one reduction
// order: a repeated launch gives the same bytes.
#include "homography_device.hpp"
#include "pair_state_device.hpp"
#include "solver_common.hpp"

namespace dr {

constexpr int kF8T = kPairThreads;

struct F8BwdLds {
  double gram[81], red[4], part[4][45], Vl[81], cs[18];   // the forward's: Gram matrix, block_sum's slots, wave partials, Jacobi
  double sums[kF8T / 64][10];                             // pass A
  double fz[18], direct[6];                               // fh, z; the direct gradients of (mu_x, mu_y, r) of the two images
  int ok;
};

// ---- the forward's stages, as refit.hip has them (block_sum, gram_accumulate<true>, the passes of refit_fundamental_pair) --------------
__device__ __forceinline__ double f8_block_sum(double v, double *red /* [4] */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

template <typename T>
__device__ __forceinline__ void f8_gram(const T *__restrict__ mt, const uint8_t *__restrict__ mk, const T *__restrict__ wt, int N,
                                        const double (&mu)[4], double r1, double r2, F8BwdLds &L) {
  double acc[45];
#pragma unroll
  for (int q = 0; q < 45; ++q) acc[q] = 0;
  for (int n = threadIdx.x; n < N; n += kF8T) {
    if (mk && !mk[n]) continue;
    double row[9];
    epipolar_row_f(((double)mt[4 * n] - mu[0]) * r1, ((double)mt[4 * n + 1] - mu[1]) * r1, ((double)mt[4 * n + 2] - mu[2]) * r2,
                   ((double)mt[4 * n + 3] - mu[3]) * r2, wt ? (double)wt[n] : 1.0, row);
    int q = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j) acc[q++] += row[i] * row[j];
  }
#pragma unroll
  for (int q = 0; q < 45; ++q) {
    const double s = wave_sum_lane63(acc[q]);
    if ((threadIdx.x & 63) == 63) L.part[threadIdx.x >> 6][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 45) {
    const int t = threadIdx.x;
    const double s = L.part[0][t] + L.part[1][t] + L.part[2][t] + L.part[3][t];
    int i = 0, rem = t;     // entry q of the upper triangle -> (i, j)
    while (rem >= 9 - i) { rem -= 9 - i; ++i; }
    const int j = i + rem;
    L.gram[i * 9 + j] = s;
    L.gram[j * 9 + i] = s;
  }
  __syncthreads();
}

// -> nsel; mu, r1, r2 and L.gram (behind a barrier).  Every thread of the block calls it and returns the same values.
template <typename T>
__device__ __forceinline__ double f8_system(const T *__restrict__ mt, const uint8_t *__restrict__ mk, const T *__restrict__ wt, int N,
                                            F8BwdLds &L, double (&mu)[4], double &r1, double &r2) {
  double s[4] = {0, 0, 0, 0}, cnt = 0;
  for (int n = threadIdx.x; n < N; n += kF8T) {
    if (mk && !mk[n]) continue;
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] += (double)mt[4 * n + d];
    cnt += 1.0;
  }
  const double nsel = f8_block_sum(cnt, L.red);
#pragma unroll
  for (int d = 0; d < 4; ++d) mu[d] = f8_block_sum(s[d], L.red) / nsel;
  double d1 = 0, d2 = 0;
  for (int n = threadIdx.x; n < N; n += kF8T) {
    if (mk && !mk[n]) continue;
    const double a = (double)mt[4 * n] - mu[0], b = (double)mt[4 * n + 1] - mu[1];
    const double c = (double)mt[4 * n + 2] - mu[2], d = (double)mt[4 * n + 3] - mu[3];
    d1 += sqrt(a * a + b * b);
    d2 += sqrt(c * c + d * d);
  }
  r1 = M_SQRT2 * nsel / f8_block_sum(d1, L.red);
  r2 = M_SQRT2 * nsel / f8_block_sum(d2, L.red);
  f8_gram<T>(mt, mk, wt, N, mu, r1, r2, L);
  return nsel;
}

// ---- the reverse pass ---------------------------------------------------------------------------------------------------------------
// s = -(p2^T Z p1)(p2^T Fh p1) of one row and its derivatives by (x1, y1, x2, y2)
__device__ __forceinline__ void f8_row_bwd(const double (&f)[9], const double (&z)[9], double x1, double y1, double x2, double y2,
                                           double &s, double (&g)[4]) {
  double zp[3], fp[3], zt[2], ft[2];      // Z p1, Fh p1; the first two of Z^T p2, Fh^T p2
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    zp[i] = z[3 * i] * x1 + z[3 * i + 1] * y1 + z[3 * i + 2];
    fp[i] = f[3 * i] * x1 + f[3 * i + 1] * y1 + f[3 * i + 2];
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    zt[j] = z[j] * x2 + z[3 + j] * y2 + z[6 + j];
    ft[j] = f[j] * x2 + f[3 + j] * y2 + f[6 + j];
  }
  const double a = x2 * zp[0] + y2 * zp[1] + zp[2], b = x2 * fp[0] + y2 * fp[1] + fp[2];
  s = -(a * b);
  g[0] = -(zt[0] * b + a * ft[0]);
  g[1] = -(zt[1] * b + a * ft[1]);
  g[2] = -(zp[0] * b + a * fp[0]);
  g[3] = -(zp[1] * b + a * fp[1]);
}

template <typename T>
__global__ __launch_bounds__(kF8T) __attribute__((amdgpu_waves_per_eu(1, 1))) void refit_fundamental_bwd_kernel(
    const T *__restrict__ matches, const uint8_t *__restrict__ mask, const T *__restrict__ weights, const T *__restrict__ grad_model, int N,
    T *__restrict__ grad_matches, T *__restrict__ grad_weights) {
  __shared__ F8BwdLds L;
  const int p = blockIdx.x, tid = threadIdx.x;
  const T *mt = matches + (size_t)p * N * 4;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T *wt = weights ? weights + (size_t)p * N : nullptr;
  double mu[4], r1, r2;
  const double nsel = f8_system<T>(mt, mk, wt, N, L, mu, r1, r2);
  if (tid < 64) {
    jacobi_eig9_wave(L.gram, L.Vl, L.cs, tid);
    double ev[1][9];
    smallest_eigvecs9_lds<1>(L.gram, L.Vl, ev);
    const double(&f)[9] = ev[0];
    int best = 0;      // (the column smallest_eigvecs9_lds took: the first strict minimum)
    double l0 = INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double d = L.gram[i * 10];
      if (d < l0) {
        l0 = d;
        best = i;
      }
    }
    // the forward's F, by its expressions: B = mat(fh) T1, F = T2^T B; valid
    double B[3][3], F[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      B[i][0] = f[3 * i] * r1;
      B[i][1] = f[3 * i + 1] * r1;
      B[i][2] = -r1 * (f[3 * i] * mu[0] + f[3 * i + 1] * mu[1]) + f[3 * i + 2];
    }
    bool ok = nsel >= 8.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      F[j] = r2 * B[0][j];
      F[3 + j] = r2 * B[1][j];
      F[6 + j] = -r2 * (mu[2] * B[0][j] + mu[3] * B[1][j]) + B[2][j];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && is_finite(F[q]);
    double g[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) g[q] = (double)grad_model[(size_t)p * 9 + q];
    // the direct gradients: gT1 = A^T gF with A = T2^T mat(fh), gT2 = B gF^T (columns 0..2 of rows 0, 1 are all that T has)
    double A[3][3], direct[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[0][j] = r2 * f[j];
      A[1][j] = r2 * f[3 + j];
      A[2][j] = -r2 * (mu[2] * f[j] + mu[3] * f[3 + j]) + f[6 + j];
    }
    {
      double t1[2][3], t2[2][3];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          t1[i][j] = A[0][i] * g[j] + A[1][i] * g[3 + j] + A[2][i] * g[6 + j];
          t2[i][j] = B[i][0] * g[3 * j] + B[i][1] * g[3 * j + 1] + B[i][2] * g[3 * j + 2];
        }
      direct[0] = -r1 * t1[0][2];
      direct[1] = -r1 * t1[1][2];
      direct[2] = t1[0][0] + t1[1][1] - mu[0] * t1[0][2] - mu[1] * t1[1][2];
      direct[3] = -r2 * t2[0][2];
      direct[4] = -r2 * t2[1][2];
      direct[5] = t2[0][0] + t2[1][1] - mu[2] * t2[0][2] - mu[3] * t2[1][2];
    }
    // g_fh = T2 gF T1^T
    double gf[9], z[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double U[3];      // row i of T2 gF
      const double m2 = i == 0 ? mu[2] : mu[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) U[j] = i == 2 ? g[6 + j] : r2 * (g[3 * i + j] - m2 * g[6 + j]);
      gf[3 * i] = r1 * (U[0] - mu[0] * U[2]);
      gf[3 * i + 1] = r1 * (U[1] - mu[1] * U[2]);
      gf[3 * i + 2] = U[2];
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) z[q] = 0.0;
#pragma unroll 1
    for (int i = 0; i < 9; ++i) {
      if (i == best) continue;
      const double gap = L.gram[i * 10] - l0;
      ok = ok && gap > 0.0 && is_finite(gap);
      double c = 0.0;
#pragma unroll
      for (int r = 0; r < 9; ++r) c += L.Vl[r * 9 + i] * gf[r];
      c /= gap;
#pragma unroll
      for (int r = 0; r < 9; ++r) z[r] += L.Vl[r * 9 + i] * c;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && is_finite(z[q]);
#pragma unroll
    for (int q = 0; q < 6; ++q) ok = ok && is_finite(direct[q]);
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        L.fz[q] = f[q];
        L.fz[9 + q] = z[q];
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) L.direct[q] = direct[q];
      L.ok = ok;
    }
  }
  __syncthreads();
  bool ok = L.ok != 0;      // (block-uniform, and so is every term added to it below: the totals are the same in every thread)
  double f[9], z[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    f[q] = L.fz[q];
    z[q] = L.fz[9 + q];
  }
  const Match4<T> *pt = reinterpret_cast<const Match4<T> *>(mt);
  // pass A, per image: sum gx, sum (gx . x), sum q / |q| (on the normalised coordinates: the same direction)
  double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int n = tid; ok && n < N; n += kF8T) {
    if (mk && !mk[n]) continue;
    const Match4<T> m = pt[n];
    const double w = wt ? (double)wt[n] : 1.0, w2 = w * w;
    const double x1 = ((double)m.v[0] - mu[0]) * r1, y1 = ((double)m.v[1] - mu[1]) * r1;
    const double x2 = ((double)m.v[2] - mu[2]) * r2, y2 = ((double)m.v[3] - mu[3]) * r2;
    double s, g[4];
    f8_row_bwd(f, z, x1, y1, x2, y2, s, g);
    const double n1 = sqrt(x1 * x1 + y1 * y1), n2 = sqrt(x2 * x2 + y2 * y2);
    const double i1 = n1 > 0.0 ? 1.0 / n1 : 0.0, i2 = n2 > 0.0 ? 1.0 / n2 : 0.0;
    a[0] += w2 * g[0];
    a[1] += w2 * g[1];
    a[2] += w2 * (g[0] * x1 + g[1] * y1);
    a[3] += x1 * i1;
    a[4] += y1 * i1;
    a[5] += w2 * g[2];
    a[6] += w2 * g[3];
    a[7] += w2 * (g[2] * x2 + g[3] * y2);
    a[8] += x2 * i2;
    a[9] += y2 * i2;
  }
  block_sum_f64<10>(a, L.sums);
  // per image: the gradient of D = sum |q_n| (r = sqrt(2) nsel / D) and 1 / nsel of the centroid's
  double gD[2], gc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double r = i ? r2 : r1;
    const double gr = L.direct[3 * i + 2] + a[5 * i + 2] / r;
    gD[i] = -gr * r * r / (M_SQRT2 * nsel);
    gc[i][0] = (L.direct[3 * i] - r * a[5 * i] - gD[i] * a[5 * i + 3]) / nsel;
    gc[i][1] = (L.direct[3 * i + 1] - r * a[5 * i + 1] - gD[i] * a[5 * i + 4]) / nsel;
    ok = ok && is_finite(gD[i]) && is_finite(gc[i][0]) && is_finite(gc[i][1]);
  }
  // pass B: every row of every requested output
  Match4<T> *gm = grad_matches ? reinterpret_cast<Match4<T> *>(grad_matches) + (size_t)p * N : nullptr;
  T *gw = grad_weights ? grad_weights + (size_t)p * N : nullptr;
  for (int n = tid; n < N; n += kF8T) {
    Match4<T> out{{T(0), T(0), T(0), T(0)}};
    T fw = T(0);
    if (ok && !(mk && !mk[n])) {
      const Match4<T> m = pt[n];
      const double w = wt ? (double)wt[n] : 1.0, w2 = w * w;
      const double x1 = ((double)m.v[0] - mu[0]) * r1, y1 = ((double)m.v[1] - mu[1]) * r1;
      const double x2 = ((double)m.v[2] - mu[2]) * r2, y2 = ((double)m.v[3] - mu[3]) * r2;
      double s, g[4];
      f8_row_bwd(f, z, x1, y1, x2, y2, s, g);
      const double n1 = sqrt(x1 * x1 + y1 * y1), n2 = sqrt(x2 * x2 + y2 * y2);
      const double i1 = n1 > 0.0 ? gD[0] / n1 : 0.0, i2 = n2 > 0.0 ? gD[1] / n2 : 0.0;
      out.v[0] = (T)(r1 * w2 * g[0] + i1 * x1 + gc[0][0]);
      out.v[1] = (T)(r1 * w2 * g[1] + i1 * y1 + gc[0][1]);
      out.v[2] = (T)(r2 * w2 * g[2] + i2 * x2 + gc[1][0]);
      out.v[3] = (T)(r2 * w2 * g[3] + i2 * y2 + gc[1][1]);
      fw = (T)(2.0 * w * s);
    }
    if (gm) gm[n] = out;
    if (gw) gw[n] = fw;
  }
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                                \
  int dr_refit_fundamental_bwd_##sfx(const T *matches, const uint8_t *mask, const T *weights, const T *grad_model, int P, int N,      \
                                     T *grad_matches, T *grad_weights, void *stream) {                                                \
    DR_REQUIRE(matches && grad_model, "null pointer");                                                                                \
    DR_REQUIRE(grad_matches || grad_weights, "nothing to write: grad_matches and grad_weights are both null");                        \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");   /* (below 8 rows every requested element is an exact zero) */                           \
    return dr::launch("refit_fundamental_bwd_kernel", dr::refit_fundamental_bwd_kernel<T>, dim3(P), dr::kF8T, stream, matches, mask,  \
                      weights, grad_model, N, grad_matches, grad_weights);                                                            \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
