// Plane-induced homographies (ransac.BatchedHomography): models from minimal samples of four matches by a closed form, its reverse
// pass for train mode, the MSAC score and inlier count of every model against every point under the symmetric transfer error, the
// per-pair state step with the adaptive stop, the normalised DLT refit over the rows a mask selects, and for scoring = "magsac" the
// MAGSAC++ score on the same error and the IRLS polish of the pair state under it.
//   matches [P,N,4] = (x1, y1, x2, y2) in the caller's coordinates (pixels; no K).  A model is the row-major 3x3 H, x2 ~ H x1, stored
//   with unit Frobenius norm and det H > 0 (det(-H) = -det H: the sign is canonical, and under it a point seen in front of both
//   cameras has a positive third coordinate in both directions).
//   Residual: y = H (x1, 1), z = adj(H) (x2, 1), d2 = |x2 - y_xy / y_w|^2 + |x1 - z_xy / z_w|^2; a point with y_w <= 0 or z_w <= 0, or
//   a non-finite d2, is an outlier and contributes nothing.  The threshold is a DISTANCE and enters as thr2 = threshold^2 per pair:
//   inlier <=> d2 < thr2; MSAC score = sum_n max(0, 1 - d2_n / thr2).
#include "homography_device.hpp"
#include "pair_state_device.hpp"
#include "solver_common.hpp"

namespace dr {

// ---- (1) four matches -> H, closed form ------------------------------------------------------------------------------------------
// Per image: c = the centroid of the four points, q_i = x_i - c, s = sqrt(2) / mean |q_i|, p_i = (s q_i, 1).  The four orientation
// determinants D_3 = [q0 q1 q2], D_0 = [q3 q1 q2], D_1 = [q0 q3 q2], D_2 = [q0 q1 q3] ([a b c] = det of the three points with a row
// of ones: twice the signed area) are the cofactors of the 3x3 solve [p0 p1 p2] lambda = p3 -- lambda_i = D_i / D_3, unchanged by
// the similarity (c, s) -- and the sample's validity test: every one non-zero, each with the same sign in both images.  They are taken
// on the centred, unscaled q: for integer coordinates every product and sum is exact, so three collinear points give exactly 0.
// A = [lambda_0 p0 | lambda_1 p1 | lambda_2 p2] maps the projective basis (e0, e1, e2, (1, 1, 1)) to the four points, so
// H = T2^-1 A2 adj(A1) T1 up to scale; then unit norm and det > 0.  All f64, all in registers.
struct H4Image {
  double q[4][2], r[4], nz[3], D[4], lam[3], A[9];      // nz = (cx, cy, s); A row-major
};

__device__ __forceinline__ double tri(const double (&q)[4][2], int i, int j, int k) {
  return q[i][0] * (q[j][1] - q[k][1]) - q[j][0] * (q[i][1] - q[k][1]) + q[k][0] * (q[i][1] - q[j][1]);
}

__device__ __forceinline__ void tri_bwd(const double (&q)[4][2], int i, int j, int k, double g, double (&gq)[4][2]) {
  gq[i][0] += g * (q[j][1] - q[k][1]);
  gq[j][0] -= g * (q[i][1] - q[k][1]);
  gq[k][0] += g * (q[i][1] - q[j][1]);
  gq[i][1] += g * (q[k][0] - q[j][0]);
  gq[j][1] += g * (q[i][0] - q[k][0]);
  gq[k][1] += g * (q[j][0] - q[i][0]);
}

__device__ __forceinline__ void h4_image(const double (&x)[4][2], H4Image &im) {
  im.nz[0] = 0.25 * (x[0][0] + x[1][0] + x[2][0] + x[3][0]);
  im.nz[1] = 0.25 * (x[0][1] + x[1][1] + x[2][1] + x[3][1]);
  double md = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    im.q[i][0] = x[i][0] - im.nz[0];
    im.q[i][1] = x[i][1] - im.nz[1];
    im.r[i] = sqrt(im.q[i][0] * im.q[i][0] + im.q[i][1] * im.q[i][1]);
    md += im.r[i];
  }
  im.nz[2] = M_SQRT2 / (0.25 * md);
  im.D[0] = tri(im.q, 3, 1, 2);
  im.D[1] = tri(im.q, 0, 3, 2);
  im.D[2] = tri(im.q, 0, 1, 3);
  im.D[3] = tri(im.q, 0, 1, 2);
  const double rd = 1.0 / im.D[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    im.lam[c] = im.D[c] * rd;
    im.A[c] = im.lam[c] * (im.nz[2] * im.q[c][0]);
    im.A[3 + c] = im.lam[c] * (im.nz[2] * im.q[c][1]);
    im.A[6 + c] = im.lam[c];
  }
}

// -> valid; H canonical (identity when not valid); M = A2 adj(A1), nrm = |T2^-1 M T1|_F, sigma: kept for the reverse pass
template <typename RowFn>
__device__ __forceinline__ bool homography4_fwd(RowFn row, bool usable, H4Image (&im)[2], double (&M)[9], double (&H)[9], double &nrm,
                                                double &sigma) {
  double x[2][4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto *r = row(i);
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d >> 1][i][d & 1] = (double)r[d];
  }
  h4_image(x[0], im[0]);
  h4_image(x[1], im[1]);
  bool ok = usable;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    ok = ok && ((im[0].D[t] > 0.0 && im[1].D[t] > 0.0) || (im[0].D[t] < 0.0 && im[1].D[t] < 0.0));      // (false for NaN)
  double B[9];
  adjugate3(im[0].A, B);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = im[1].A[3 * i] * B[j] + im[1].A[3 * i + 1] * B[3 + j] + im[1].A[3 * i + 2] * B[6 + j];
  denormalise_h(M, im[0].nz, im[1].nz, H);
  return canonical_h(H, ok, nrm, sigma);
}

template <typename T>
__device__ __forceinline__ void store_h(T *__restrict__ dst, const double (&H)[9]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) dst[q] = (T)H[q];
}

// rows read through the index sets: one lane = one sample (a bad index reads row 0, valid = 0)
template <typename T>
__global__ __launch_bounds__(64) void homography4_gather_kernel(const T *__restrict__ matches, const int32_t *__restrict__ idx, int Bt,
                                                                int B, int N, T *__restrict__ models, uint8_t *__restrict__ valid) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= Bt) return;
  const T *base = matches + (size_t)(s / B) * N * 4;
  const int32_t *gi = idx + (size_t)s * 4;
  bool in_range = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) in_range = in_range && gi[r] >= 0 && gi[r] < N;
  H4Image im[2];
  double M[9], H[9], nrm, sigma;
  valid[s] = homography4_fwd([&](int r) { return base + (size_t)(in_range ? gi[r] : 0) * 4; }, in_range, im, M, H, nrm, sigma);
  store_h(models + (size_t)s * 9, H);
}

// explicit sample tensors [Bt,4,4]: what train mode fits.  On samples = matches[idx] the bits of the gather kernel.
template <typename T>
__global__ __launch_bounds__(64) void homography4_kernel(const T *__restrict__ samples, int Bt, T *__restrict__ models,
                                                         uint8_t *__restrict__ valid) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= Bt) return;
  const T *base = samples + (size_t)s * 16;
  H4Image im[2];
  double M[9], H[9], nrm, sigma;
  valid[s] = homography4_fwd([&](int r) { return base + r * 4; }, true, im, M, H, nrm, sigma);
  store_h(models + (size_t)s * 9, H);
}

// ---- (1c) the reverse pass of (1): gH -> the gradient of the 16 sample values ------------------------------------------------------
// The forward is recomputed in f64 from the sample (no stored model).  Backwards through it:
//   H = sigma H0 / |H0|         g0 = (sigma / |H0|) (gH - H <H, gH>)        (so a multiple of H in gH passes nothing on)
//   H0 = T2^-1 (M T1)           gM, and the direct gradients of (c1, s1) and (c2, s2)
//   M = A2 adj(A1)              gA2 = gM adj(A1)^T;  adj(A)'s rows are a1 x a2, a2 x a0, a0 x a1 of A's columns: cross-product rule
//   a_c = lambda_c (s q_c, 1)   g lambda, gs, gq;  lambda_c = D_c / D_3 -> gD;  D = orientation determinants -> gq
//   s = sqrt(2) / mean |q_i|,  q_i = x_i - c,  c = mean x_i
// one image's part: gA (row-major), the direct gradient gnz of (cx, cy, s) -> gx[4][2]
__device__ __forceinline__ void h4_image_bwd(const H4Image &im, const double (&gA)[9], const double (&gnz)[3], double (&gx)[4][2]) {
  double gq[4][2], gD[4], gs = gnz[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) gq[i][0] = gq[i][1] = 0.0;
  const double s = im.nz[2], rd = 1.0 / im.D[3];
  gD[3] = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double g0 = gA[c], g1 = gA[3 + c], g2 = gA[6 + c];
    const double glam = g0 * (s * im.q[c][0]) + g1 * (s * im.q[c][1]) + g2;
    gs += im.lam[c] * (g0 * im.q[c][0] + g1 * im.q[c][1]);
    gq[c][0] += s * im.lam[c] * g0;
    gq[c][1] += s * im.lam[c] * g1;
    gD[c] = glam * rd;
    gD[3] -= glam * im.lam[c] * rd;
  }
  tri_bwd(im.q, 3, 1, 2, gD[0], gq);
  tri_bwd(im.q, 0, 3, 2, gD[1], gq);
  tri_bwd(im.q, 0, 1, 3, gD[2], gq);
  tri_bwd(im.q, 0, 1, 2, gD[3], gq);
  const double md = 0.25 * (im.r[0] + im.r[1] + im.r[2] + im.r[3]);
  const double gmd = -gs * s / md;
  double sum0 = 0.0, sum1 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double ri = im.r[i] > 0.0 ? 0.25 * gmd / im.r[i] : 0.0;      // (a point on the centroid: |q| is not differentiable, pass 0)
    gq[i][0] += ri * im.q[i][0];
    gq[i][1] += ri * im.q[i][1];
    sum0 += gq[i][0];
    sum1 += gq[i][1];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gx[i][0] = gq[i][0] + 0.25 * (gnz[0] - sum0);
    gx[i][1] = gq[i][1] + 0.25 * (gnz[1] - sum1);
  }
}

__device__ __forceinline__ void cross_acc(const double *a, const double *b, double *out) {      // out += a x b
  out[0] += a[1] * b[2] - a[2] * b[1];
  out[1] += a[2] * b[0] - a[0] * b[2];
  out[2] += a[0] * b[1] - a[1] * b[0];
}

// H0 = T2^-1 (M T1) backwards: g0 = dL/dH0 -> gM and the direct gradients gnz1, gnz2 of (cx, cy, s) of the two images
__device__ __forceinline__ void denormalise_h_bwd(const double (&M)[9], const double (&nz1)[3], const double (&nz2)[3],
                                                  const double (&g0)[9], double (&gM)[9], double (&gnz1)[3], double (&gnz2)[3]) {
  // H0 = T2^-1 G, G = M T1
  const double s1 = nz1[2], cx1 = nz1[0], cy1 = nz1[1];
  const double s2 = nz2[2], cx2 = nz2[0], cy2 = nz2[1], r2 = 1.0 / s2;
  double G[9], gG[9];
  double gr2 = 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) gnz1[q] = gnz2[q] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[3 * i] = M[3 * i] * s1;
    G[3 * i + 1] = M[3 * i + 1] * s1;
    G[3 * i + 2] = M[3 * i + 2] - s1 * (M[3 * i] * cx1 + M[3 * i + 1] * cy1);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    gG[j] = r2 * g0[j];
    gG[3 + j] = r2 * g0[3 + j];
    gG[6 + j] = cx2 * g0[j] + cy2 * g0[3 + j] + g0[6 + j];
    gr2 += g0[j] * G[j] + g0[3 + j] * G[3 + j];
    gnz2[0] += g0[j] * G[6 + j];
    gnz2[1] += g0[3 + j] * G[6 + j];
  }
  gnz2[2] = -gr2 * r2 * r2;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double m0 = M[3 * i], m1 = M[3 * i + 1], g2 = gG[3 * i + 2];
    gM[3 * i] = s1 * (gG[3 * i] - g2 * cx1);
    gM[3 * i + 1] = s1 * (gG[3 * i + 1] - g2 * cy1);
    gM[3 * i + 2] = g2;
    gnz1[2] += gG[3 * i] * m0 + gG[3 * i + 1] * m1 - g2 * (m0 * cx1 + m1 * cy1);
    gnz1[0] -= s1 * g2 * m0;
    gnz1[1] -= s1 * g2 * m1;
  }
}

// every output element is written; exact zeros for a sample without a valid model or with a non-finite derivative
template <typename T>
__global__ __launch_bounds__(64) void homography4_bwd_kernel(const T *__restrict__ samples, const T *__restrict__ grad_models, int Bt,
                                                             T *__restrict__ grad_samples) {
  const int smp = blockIdx.x * 64 + threadIdx.x;
  if (smp >= Bt) return;
  const T *base = samples + (size_t)smp * 16;
  H4Image im[2];
  double M[9], H[9], nrm, sigma;
  bool ok = homography4_fwd([&](int r) { return base + r * 4; }, true, im, M, H, nrm, sigma);
  double g0[9], dot = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    g0[q] = (double)grad_models[(size_t)smp * 9 + q];
    dot += H[q] * g0[q];
  }
  const double sc = sigma / nrm;
#pragma unroll
  for (int q = 0; q < 9; ++q) g0[q] = sc * (g0[q] - H[q] * dot);
  double gnz1[3], gnz2[3], gM[9];
  denormalise_h_bwd(M, im[0].nz, im[1].nz, g0, gM, gnz1, gnz2);
  // M = A2 B, B = adj(A1)
  double Bm[9], gA2[9], gB[9], gA1[9];
  adjugate3(im[0].A, Bm);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gA2[3 * i + k] = gM[3 * i] * Bm[3 * k] + gM[3 * i + 1] * Bm[3 * k + 1] + gM[3 * i + 2] * Bm[3 * k + 2];
      gB[3 * i + k] = im[1].A[i] * gM[k] + im[1].A[3 + i] * gM[3 + k] + im[1].A[6 + i] * gM[6 + k];      // (A2^T gM)[i][k]
    }
  double a[3][3], ga[3][3];      // columns of A1 and their gradients
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a[c][r] = im[0].A[3 * r + c];
      ga[c][r] = 0.0;
    }
  cross_acc(a[2], &gB[0], ga[1]);      // row 0 = a1 x a2
  cross_acc(&gB[0], a[1], ga[2]);
  cross_acc(a[0], &gB[3], ga[2]);      // row 1 = a2 x a0
  cross_acc(&gB[3], a[2], ga[0]);
  cross_acc(a[1], &gB[6], ga[0]);      // row 2 = a0 x a1
  cross_acc(&gB[6], a[0], ga[1]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) gA1[3 * r + c] = ga[c][r];
  double gx1[4][2], gx2[4][2];
  h4_image_bwd(im[0], gA1, gnz1, gx1);
  h4_image_bwd(im[1], gA2, gnz2, gx2);
#pragma unroll
  for (int i = 0; i < 4; ++i) ok = ok && is_finite(gx1[i][0]) && is_finite(gx1[i][1]) && is_finite(gx2[i][0]) && is_finite(gx2[i][1]);
  T *gs = grad_samples + (size_t)smp * 16;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gs[4 * i] = ok ? (T)gx1[i][0] : T(0);
    gs[4 * i + 1] = ok ? (T)gx1[i][1] : T(0);
    gs[4 * i + 2] = ok ? (T)gx2[i][0] : T(0);
    gs[4 * i + 3] = ok ? (T)gx2[i][1] : T(0);
  }
}

// ---- (2), (3) the score of every model against every point and the state step are pair_state_device.hpp's pair_score_kernel and
// pair_update_kernel under HomographyGeom and a term of homography_device.hpp: TransferMsacTerm (dr_homography_score) or
// TransferMagsacTerm (dr_homography_magsac_score: sum_n (1 - l(d2_n / thr2)), the same inlier test and slot rules)

// ---- (4) normalised DLT over the rows a mask selects: one 256-thread block per pair, f64, fixed-order sums -----------------------------
// Three passes of thread n over rows n, n + 256, ...: the count and the coordinate sums (the centroids), the distance sums (the
// scales s_i = sqrt(2) / mean distance: Hartley's transforms of the selected rows, unweighted), the Gram matrix.  With X = (x, y, 1)
// and (u, v) the normalised points, the two DLT rows of a match are a = (0, -X, v X) and b = (X, 0, -u X), so
//   sum w (a a^T + b b^T) = [[S, 0, -Su], [0, S, -Sv], [-Su, -Sv, Sq]],   S = sum w X X^T, Su = sum w u X X^T, Sv = sum w v X X^T,
//   Sq = sum w (u^2 + v^2) X X^T:  24 sums instead of 45.  Sums by block_sum_f64: lane, wave butterfly, the four waves in order.
// Wave 0 then takes the smallest eigenvector with jacobi_eig9_wave, denormalises and canonicalises; valid = 0 (identity) below four
// rows and for a non-finite or singular result.
// The passes are dlt_system, shared with the IRLS polish (5) and open to any kernel that refits over a selection: `sel` answers
// "is row n present, with what weight" -- present(n), row(n), weight(n); the weight is asked for by the third pass only, of present rows.
constexpr int kHRThreads = kPairThreads;

// the LDS of one fit: s_part = [4][K] of the three sums in turn
struct DltLds {
  double s_part[(kHRThreads / 64) * 24], s_tot[24], gram[81], Vl[81], cs[18];
};

// the rows a mask selects (null: all of them), under per-row weights (null: 1)
template <typename T>
struct MaskedRows4 {
  const Match4<T> *pt;
  const uint8_t *mk;
  const T *wt;
  __device__ __forceinline__ bool present(int n) const { return !(mk && !mk[n]); }
  __device__ __forceinline__ Match4<T> row(int n) const { return pt[n]; }
  __device__ __forceinline__ double weight(int n) const { return wt ? (double)wt[n] : 1.0; }
};

// -> the number of rows; nz1, nz2 = (cx, cy, s) of the two images, L.gram = the 9x9 Gram matrix of the normalised system (behind a
// barrier).  Every thread of the block calls it and returns the same values.
template <typename T, typename Rows>
__device__ __forceinline__ double dlt_system(const Rows &sel, int N, DltLds &L, double (&nz1)[3], double (&nz2)[3]) {
  const int tid = threadIdx.x;
  double a[5] = {0, 0, 0, 0, 0};
  for (int n = tid; n < N; n += kHRThreads) {
    if (!sel.present(n)) continue;
    const Match4<T> x = sel.row(n);
#pragma unroll
    for (int d = 0; d < 4; ++d) a[d] += (double)x.v[d];
    a[4] += 1.0;
  }
  block_sum_f64<5>(a, reinterpret_cast<double(*)[5]>(L.s_part));
  const double rows = a[4], rn = 1.0 / rows;
  const double mu[4] = {a[0] * rn, a[1] * rn, a[2] * rn, a[3] * rn};
  double dd[2] = {0, 0};
  for (int n = tid; n < N; n += kHRThreads) {
    if (!sel.present(n)) continue;
    const Match4<T> x = sel.row(n);
    const double q0 = (double)x.v[0] - mu[0], q1 = (double)x.v[1] - mu[1], q2 = (double)x.v[2] - mu[2], q3 = (double)x.v[3] - mu[3];
    dd[0] += sqrt(q0 * q0 + q1 * q1);
    dd[1] += sqrt(q2 * q2 + q3 * q3);
  }
  block_sum_f64<2>(dd, reinterpret_cast<double(*)[2]>(L.s_part));
  nz1[0] = mu[0], nz1[1] = mu[1], nz1[2] = M_SQRT2 * rows / dd[0];
  nz2[0] = mu[2], nz2[1] = mu[3], nz2[2] = M_SQRT2 * rows / dd[1];
  double g[24];
#pragma unroll
  for (int q = 0; q < 24; ++q) g[q] = 0.0;
  for (int n = tid; n < N; n += kHRThreads) {
    if (!sel.present(n)) continue;
    const Match4<T> m = sel.row(n);
    const double w = sel.weight(n);
    const double x = ((double)m.v[0] - nz1[0]) * nz1[2], y = ((double)m.v[1] - nz1[1]) * nz1[2];
    const double u = ((double)m.v[2] - nz2[0]) * nz2[2], v = ((double)m.v[3] - nz2[1]) * nz2[2];
    const double xx[6] = {w * x * x, w * x * y, w * x, w * y * y, w * y, w};
    const double q2 = u * u + v * v;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      g[e] += xx[e];
      g[6 + e] += u * xx[e];
      g[12 + e] += v * xx[e];
      g[18 + e] += q2 * xx[e];
    }
  }
  block_partials_f64<24>(g, reinterpret_cast<double(*)[24]>(L.s_part));
  if (tid < 24) L.s_tot[tid] = block_total_f64<24>(reinterpret_cast<double(*)[24]>(L.s_part), tid);      // (the Gram matrix picks its totals by
  __syncthreads();                                                                                      // a run-time index: they stay in LDS)
  if (tid < 81) {
    const int r = tid / 9, c = tid - 9 * r, br = r / 3, bc = c / 3, i = r - 3 * br, j = c - 3 * bc;
    const int lo = min(i, j), hi = max(i, j), e = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);      // (i, j) -> entry of the symmetric 3x3
    const int bl = min(br, bc), bh = max(br, bc);
    double v = 0.0;
    if (bl == bh) v = bl == 2 ? L.s_tot[18 + e] : L.s_tot[e];
    else if (bh == 2) v = bl == 0 ? -L.s_tot[6 + e] : -L.s_tot[12 + e];
    L.gram[tid] = v;
  }
  __syncthreads();
  return rows;
}

// wave 0 behind dlt_system: the smallest eigenvector, denormalised and canonical -> valid (H = identity when not)
__device__ __forceinline__ bool dlt_solve_wave(DltLds &L, int lane, const double (&nz1)[3], const double (&nz2)[3], double rows,
                                               double (&H)[9]) {
  jacobi_eig9_wave(L.gram, L.Vl, L.cs, lane);
  double ev[1][9];
  smallest_eigvecs9_lds<1>(L.gram, L.Vl, ev);
  double nrm, sigma;
  denormalise_h(ev[0], nz1, nz2, H);
  return canonical_h(H, rows >= 4.0, nrm, sigma);
}

template <typename T>
__global__ __launch_bounds__(kHRThreads) void refit_homography_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                      const T *__restrict__ weights, int N, T *__restrict__ model,
                                                                      uint8_t *__restrict__ valid) {
  __shared__ DltLds L;
  const int p = blockIdx.x, tid = threadIdx.x;
  const MaskedRows4<T> sel{reinterpret_cast<const Match4<T> *>(matches) + (size_t)p * N, mask ? mask + (size_t)p * N : nullptr,
                           weights ? weights + (size_t)p * N : nullptr};
  double nz1[3], nz2[3];
  const double rows = dlt_system<T>(sel, N, L, nz1, nz2);
  if (tid >= 64) return;
  double H[9];
  const bool ok = dlt_solve_wave(L, tid, nz1, nz2, rows, H);
  if (tid == 0) {
    store_h(model + (size_t)p * 9, H);
    valid[p] = ok;
  }
}

// ---- (4b) the reverse pass of (4): gH -> the gradient of the rows and of their weights (dr_refit_homography_bwd) ----------------------
// Nothing is stored by the forward: the same dlt_system call over the same MaskedRows4 gives the rows, the transforms and the Gram
// matrix G bit for bit, wave 0's Jacobi all nine eigenpairs (lambda_i, v_i); h = v_0 is the forward's eigenvector.  Backwards:
//   H = sigma H0 / |H0|         g0 = (sigma / |H0|) (gH - H <H, gH>)       (the rule of (1c): a multiple of H in gH passes nothing on)
//   H0 = T2^-1 (mat(h) T1)      g_h, and the direct gradients of (cx, cy, s) of each image (denormalise_h_bwd)
//   h = v_0(G)                  dh = sum_{i != 0} v_i (v_i^T dG h) / (lambda_0 - lambda_i), so with
//                               z = sum_{i != 0} v_i (v_i . g_h) / (lambda_i - lambda_0):  dL = -z^T dG h,  gG = -(z h^T + h z^T) / 2;
//                               g_h is taken with respect to the vector as returned, so its arbitrary sign cancels in z h^T
//   G = sum w (a a^T + b b^T)   f_n = a^T gG a + b^T gG b = -[(a . z)(a . h) + (b . z)(b . h)] = dL/dw_n (the transforms are unweighted:
//                               the weights enter through G only), and w_n df_n/d(x, y, u, v) is the row's normalised-coordinate gradient
//   x = (X1 - cx1) s1, ...      per image: g_c = -s sum gx (+ direct), g_s = sum (gx . x) / s (+ direct)
//   s = sqrt(2) R / D, D = sum |q_n|, q_n = X_n - c, c = mean X_n:  g_D = -g_s s / D;  the centroid enters the centred coordinates and
//                               D: g_c -= g_D sum q_n / |q_n|;  a row gets  s gx_n + g_D q_n / |q_n| + g_c / R  (q_n / |q_n| := 0 at |q_n| = 0)
// Mapping: (4)'s -- one 256-thread block per pair, f64, thread n owns rows n, n + 256, ....  Wave 0 hands h, z and the six direct
// gradients to the block through LDS; pass A reduces the ten sums above with block_sum_f64; pass B writes every row of every requested
// output: exact zeros for rows the mask drops (never loaded) and for every row of a pair with fewer than four rows, valid = 0,
// lambda_i - lambda_0 not positive and finite for some i != 0, or a non-finite h-path, sum or centroid / scale gradient -- one
// block-uniform decision.  No atomics, one reduction order: a repeated launch gives the same bits.
// f_n and its derivatives for one row; z = the perturbation vector above
__device__ __forceinline__ void dlt_row_bwd(const double (&h)[9], const double (&z)[9], double x, double y, double u, double v,
                                            double &f, double (&g)[4]) {
  const double h2 = h[6] * x + h[7] * y + h[8], z2 = z[6] * x + z[7] * y + z[8];
  const double ah = v * h2 - (h[3] * x + h[4] * y + h[5]), bh = (h[0] * x + h[1] * y + h[2]) - u * h2;
  const double az = v * z2 - (z[3] * x + z[4] * y + z[5]), bz = (z[0] * x + z[1] * y + z[2]) - u * z2;
  f = -(az * ah + bz * bh);
#pragma unroll
  for (int d = 0; d < 2; ++d)      // d/dx, d/dy of a . t = v t2 - t1 and b . t = t0 - u t2
    g[d] = -((v * z[6 + d] - z[3 + d]) * ah + az * (v * h[6 + d] - h[3 + d]) + (z[d] - u * z[6 + d]) * bh + bz * (h[d] - u * h[6 + d]));
  g[2] = z2 * bh + bz * h2;
  g[3] = -(z2 * ah + az * h2);
}

template <typename T>
__global__ __launch_bounds__(kHRThreads) void refit_homography_bwd_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                          const T *__restrict__ weights,
                                                                          const T *__restrict__ grad_model, int N,
                                                                          T *__restrict__ grad_matches, T *__restrict__ grad_weights) {
  __shared__ DltLds L;
  __shared__ double s_hz[18], s_gnz[6];      // h, z; the direct gradients of (cx, cy, s) of the two images
  __shared__ int s_ok;
  const int p = blockIdx.x, tid = threadIdx.x;
  const MaskedRows4<T> sel{reinterpret_cast<const Match4<T> *>(matches) + (size_t)p * N, mask ? mask + (size_t)p * N : nullptr,
                           weights ? weights + (size_t)p * N : nullptr};
  double nz1[3], nz2[3];
  const double rows = dlt_system<T>(sel, N, L, nz1, nz2);
  if (tid < 64) {
    jacobi_eig9_wave(L.gram, L.Vl, L.cs, tid);
    double ev[1][9], H[9], nrm, sigma;
    smallest_eigvecs9_lds<1>(L.gram, L.Vl, ev);
    denormalise_h(ev[0], nz1, nz2, H);
    bool ok = canonical_h(H, rows >= 4.0, nrm, sigma);
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
    double g0[9], dot = 0.0;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      g0[q] = (double)grad_model[(size_t)p * 9 + q];
      dot += H[q] * g0[q];
    }
    const double sc = sigma / nrm;
#pragma unroll
    for (int q = 0; q < 9; ++q) g0[q] = sc * (g0[q] - H[q] * dot);
    double gh[9], gnz1[3], gnz2[3], z[9];
    denormalise_h_bwd(ev[0], nz1, nz2, g0, gh, gnz1, gnz2);
#pragma unroll
    for (int q = 0; q < 9; ++q) z[q] = 0.0;
#pragma unroll 1
    for (int i = 0; i < 9; ++i) {
      if (i == best) continue;
      const double gap = L.gram[i * 10] - l0;
      ok = ok && gap > 0.0 && is_finite(gap);
      double c = 0.0;
#pragma unroll
      for (int r = 0; r < 9; ++r) c += L.Vl[r * 9 + i] * gh[r];
      c /= gap;
#pragma unroll
      for (int r = 0; r < 9; ++r) z[r] += L.Vl[r * 9 + i] * c;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) ok = ok && is_finite(z[q]);
#pragma unroll
    for (int q = 0; q < 3; ++q) ok = ok && is_finite(gnz1[q]) && is_finite(gnz2[q]);
    if (tid == 0) {
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        s_hz[q] = ev[0][q];
        s_hz[9 + q] = z[q];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        s_gnz[q] = gnz1[q];
        s_gnz[3 + q] = gnz2[q];
      }
      s_ok = ok;
    }
  }
  __syncthreads();
  bool ok = s_ok != 0;      // (block-uniform, and so is every term added to it below: the totals are the same in every thread)
  double h[9], z[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    h[q] = s_hz[q];
    z[q] = s_hz[9 + q];
  }
  // pass A, per image: sum w g, sum w (g . x), sum q / |q| (on the normalised coordinates: the same direction)
  double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int n = tid; ok && n < N; n += kHRThreads) {
    if (!sel.present(n)) continue;
    const Match4<T> m = sel.row(n);
    const double w = sel.weight(n);
    const double x = ((double)m.v[0] - nz1[0]) * nz1[2], y = ((double)m.v[1] - nz1[1]) * nz1[2];
    const double u = ((double)m.v[2] - nz2[0]) * nz2[2], v = ((double)m.v[3] - nz2[1]) * nz2[2];
    double f, g[4];
    dlt_row_bwd(h, z, x, y, u, v, f, g);
    const double r1 = sqrt(x * x + y * y), r2 = sqrt(u * u + v * v);
    const double i1 = r1 > 0.0 ? 1.0 / r1 : 0.0, i2 = r2 > 0.0 ? 1.0 / r2 : 0.0;
    a[0] += w * g[0];
    a[1] += w * g[1];
    a[2] += w * (g[0] * x + g[1] * y);
    a[3] += x * i1;
    a[4] += y * i1;
    a[5] += w * g[2];
    a[6] += w * g[3];
    a[7] += w * (g[2] * u + g[3] * v);
    a[8] += u * i2;
    a[9] += v * i2;
  }
  block_sum_f64<10>(a, reinterpret_cast<double(*)[10]>(L.s_part));
  // per image: the gradient of D = sum |q_n| (s = sqrt(2) R / D) and 1 / R of the centroid's
  double gD[2], gc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double s = i ? nz2[2] : nz1[2];
    const double gs = s_gnz[3 * i + 2] + a[5 * i + 2] / s;
    gD[i] = -gs * s * s / (M_SQRT2 * rows);
    gc[i][0] = (s_gnz[3 * i] - s * a[5 * i] - gD[i] * a[5 * i + 3]) / rows;
    gc[i][1] = (s_gnz[3 * i + 1] - s * a[5 * i + 1] - gD[i] * a[5 * i + 4]) / rows;
    ok = ok && is_finite(gD[i]) && is_finite(gc[i][0]) && is_finite(gc[i][1]);
  }
  // pass B: every row of every requested output
  Match4<T> *gm = grad_matches ? reinterpret_cast<Match4<T> *>(grad_matches) + (size_t)p * N : nullptr;
  T *gw = grad_weights ? grad_weights + (size_t)p * N : nullptr;
  for (int n = tid; n < N; n += kHRThreads) {
    Match4<T> out{{T(0), T(0), T(0), T(0)}};
    T fw = T(0);
    if (ok && sel.present(n)) {
      const Match4<T> m = sel.row(n);
      const double w = sel.weight(n);
      const double x = ((double)m.v[0] - nz1[0]) * nz1[2], y = ((double)m.v[1] - nz1[1]) * nz1[2];
      const double u = ((double)m.v[2] - nz2[0]) * nz2[2], v = ((double)m.v[3] - nz2[1]) * nz2[2];
      double f, g[4];
      dlt_row_bwd(h, z, x, y, u, v, f, g);
      const double r1 = sqrt(x * x + y * y), r2 = sqrt(u * u + v * v);
      const double i1 = r1 > 0.0 ? gD[0] / r1 : 0.0, i2 = r2 > 0.0 ? gD[1] / r2 : 0.0;
      out.v[0] = (T)(nz1[2] * w * g[0] + i1 * x + gc[0][0]);
      out.v[1] = (T)(nz1[2] * w * g[1] + i1 * y + gc[0][1]);
      out.v[2] = (T)(nz2[2] * w * g[2] + i2 * u + gc[1][0]);
      out.v[3] = (T)(nz2[2] * w * g[3] + i2 * v + gc[1][1]);
      fw = (T)f;
    }
    if (gm) gm[n] = out;
    if (gw) gw[n] = fw;
  }
}

// ---- (5) IRLS polish of the pair state under the MAGSAC++ loss (BatchedHomography(scoring = "magsac")): pair_polish under this fit ----
//   The rows of a step are the points inside the cutoff and in front of both cameras under the current model, each with
// the weight w(s_n) of TransferMagsacTerm; the fit is the normalised DLT of (4) over those rows (dlt_system: Hartley's transforms
// unweighted over the rows, the weight in the Gram sums) and wave 0's eigenvector, which reaches the block through LDS.  Nothing is
// fitted from a NaN or singular state, which has no rows, or with fewer than four rows (on the count dlt_system returns, so its other
// two passes have run by then, over transforms that are inf / NaN without rows -- nothing of them is used or stored).  The mask stays
// the RANSAC winner's.
// The row decision and the weights are evaluated in f64 for either type (the model and the rows widened, thr2 as stored): the refit's
// sums are f64 already, and f32 weights move a fitted model by more than its output rounding.  They are not stored: the
// three passes evaluate the same expression on the same values.  A step is four block-stride passes over 16 N bytes.
template <typename T>
struct CutoffRows4 {
  const Match4<T> *pt;
  const ScoredH<double> &s;
  const TransferMagsacTerm<double> &term;
  __device__ __forceinline__ bool d2(int n, double &out) const {
    const Match4<T> x = pt[n];
    const double xd[4] = {(double)x.v[0], (double)x.v[1], (double)x.v[2], (double)x.v[3]};
    return transfer_d2<double>(s, xd, out);
  }
  __device__ __forceinline__ bool present(int n) const {
    double v;
    return d2(n, v) && term.inlier(v);
  }
  __device__ __forceinline__ Match4<T> row(int n) const { return pt[n]; }
  __device__ __forceinline__ double weight(int n) const {      // (of a present row: the same expression on the same values)
    double v;
    d2(n, v);
    return term.weight(v);
  }
};

template <typename T>
struct HomographyIrlsFit {
  const Match4<T> *pt;
  int N;
  const TransferMagsacTerm<double> &term;
  DltLds &L;
  T *s_cand;      // shared: the candidate's 9 values and, in s_ok, the fit's validity; both are next written behind dlt_system's
  int *s_ok;      // barriers, after every thread has read them (pair_block_score's two barriers lie in between)
  __device__ __forceinline__ int operator()(const T (&cur)[9], T (&cand)[9]) const {
    double bd[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) bd[q] = (double)cur[q];
    ScoredH<double> s;
    prepare_h(bd, true, s);
    if (s.kind != kModelScored) return kFitStop;
    double nz1[3], nz2[3];
    const double rows = dlt_system<T>(CutoffRows4<T>{pt, s, term}, N, L, nz1, nz2);
    if (!(rows >= 4.0)) return kFitStop;
    if (threadIdx.x < 64) {
      double H[9];
      const bool ok = dlt_solve_wave(L, threadIdx.x, nz1, nz2, rows, H);
      if (threadIdx.x == 0) {
        store_h(s_cand, H);
        *s_ok = ok;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 9; ++q) cand[q] = s_cand[q];
    return *s_ok ? kFitValid : kFitInvalid;
  }
};

template <typename T>
__global__ __launch_bounds__(kHRThreads) void homography_irls_kernel(const T *__restrict__ matches, const T *__restrict__ thr2, int N,
                                                                     int iters, T *__restrict__ best_score, T *__restrict__ best_model,
                                                                     int32_t *__restrict__ irls_fits) {
  __shared__ DltLds L;
  __shared__ T s_part[kHRThreads / 64], s_cand[9];
  __shared__ int s_ok;
  const int p = blockIdx.x;
  const T *pt = matches + (size_t)p * N * 4;
  const TransferMagsacTerm<T> term(thr2[p]);
  const TransferMagsacTerm<double> termd((double)thr2[p]);
  const HomographyIrlsFit<T> fit{reinterpret_cast<const Match4<T> *>(pt), N, termd, L, s_cand, &s_ok};
  pair_polish<T, HomographyGeom>(pt, N, iters, term, fit, s_part, best_score + p, best_model + (size_t)p * 9, irls_fits + p);
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                              \
  int dr_homography4_gather_##sfx(const T *matches, const int32_t *idx, int P, int B, int N, T *models, uint8_t *valid,             \
                                  void *stream) {                                                                                   \
    DR_REQUIRE(matches && idx && models && valid, "null pointer");                                                                  \
    DR_REQUIRE(P > 0 && B > 0 && N > 0 && (long)P * B < (1l << 31), "need P, B, N > 0");                                            \
    return dr::launch("homography4_gather_kernel", dr::homography4_gather_kernel<T>, dim3((P * B + 63) / 64), 64, stream, matches,  \
                      idx, P * B, B, N, models, valid);                                                                             \
  }                                                                                                                                 \
  int dr_homography4_##sfx(const T *samples, int Bt, T *models, uint8_t *valid, void *stream) {                                     \
    DR_REQUIRE(samples && models && valid, "null pointer");                                                                         \
    DR_REQUIRE(Bt > 0, "need Bt > 0");                                                                                              \
    return dr::launch("homography4_kernel", dr::homography4_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples, Bt, models,       \
                      valid);                                                                                                       \
  }                                                                                                                                 \
  int dr_homography4_bwd_##sfx(const T *samples, const T *grad_models, int Bt, T *grad_samples, void *stream) {                     \
    DR_REQUIRE(samples && grad_models && grad_samples, "null pointer");                                                             \
    DR_REQUIRE(Bt > 0, "need Bt > 0");                                                                                              \
    return dr::launch("homography4_bwd_kernel", dr::homography4_bwd_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples,           \
                      grad_models, Bt, grad_samples);                                                                               \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_OP(sfx, T)                                                                                                              \
  int dr_homography_score_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *thr2, int P, int M, int N,        \
                                T *scores, int32_t *inliers, void *stream) {                                                        \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535, "bad sizes");                                                                 \
    return dr::launch_pair_score<T, dr::HomographyGeom, dr::TransferMsacTerm<T>>(matches, models, valid, thr2, P, M, N, scores,     \
                                                                                 inliers, nullptr, nullptr, stream);                \
  }                                                                                                                                 \
  int dr_homography_magsac_score_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *thr2, int P, int M, int N, \
                                       T *scores, int32_t *inliers, void *stream) {                                                 \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535, "bad sizes");                                                                 \
    return dr::launch_pair_score<T, dr::HomographyGeom, dr::TransferMagsacTerm<T>>(matches, models, valid, thr2, P, M, N, scores,   \
                                                                                   inliers, nullptr, nullptr, stream);              \
  }                                                                                                                                 \
  int dr_homography_irls_##sfx(const T *matches, const T *thr2, int P, int N, int irls_iters, T *best_score, T *best_model,         \
                               int32_t *irls_fits, void *stream) {                                                                  \
    DR_REQUIRE(matches && thr2 && best_score && best_model && irls_fits, "null pointer");                                           \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");                                                                                        \
    DR_REQUIRE(irls_iters >= 1, "irls_iters must be at least 1");                                                                   \
    return dr::launch("homography_irls_kernel", dr::homography_irls_kernel<T>, dim3(P), dr::kHRThreads, stream, matches, thr2, N,   \
                      irls_iters, best_score, best_model, irls_fits);                                                               \
  }                                                                                                                                 \
  int dr_homography_update_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *scores, const T *thr2, int P,    \
                                 int M, int N, int B, double confidence, double eps, int max_iterations, T *best_score,             \
                                 T *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters, double *max_iters,       \
                                 void *stream) {                                                                                    \
    DR_REQUIRE(matches && models && scores && thr2 && best_score && best_model && best_mask && best_inliers && iters && max_iters,  \
               "null pointer");                                                                                                     \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && B > 0 && max_iterations > 0, "bad sizes");                                                \
    return dr::launch("pair_update_kernel", dr::pair_update_kernel<T, dr::HomographyGeom>, dim3(P), dr::kPairThreads, stream,       \
                      matches, models, valid, scores, thr2, M, N, B, confidence, eps, max_iterations, best_score, best_model,       \
                      best_mask, best_inliers, iters, max_iters);                                                                   \
  }                                                                                                                                 \
  int dr_refit_homography_##sfx(const T *matches, const uint8_t *mask, const T *weights, int P, int N, T *model, uint8_t *valid,    \
                                void *stream) {                                                                                     \
    DR_REQUIRE(matches && model && valid, "null pointer");                                                                          \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");                                                                                        \
    return dr::launch("refit_homography_kernel", dr::refit_homography_kernel<T>, dim3(P), dr::kHRThreads, stream, matches, mask,    \
                      weights, N, model, valid);                                                                                    \
  }                                                                                                                                 \
  int dr_refit_homography_bwd_##sfx(const T *matches, const uint8_t *mask, const T *weights, const T *grad_model, int P, int N,     \
                                    T *grad_matches, T *grad_weights, void *stream) {                                               \
    DR_REQUIRE(matches && grad_model, "null pointer");                                                                              \
    DR_REQUIRE(grad_matches || grad_weights, "nothing to write: grad_matches and grad_weights are both null");                      \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");                                                                                        \
    return dr::launch("refit_homography_bwd_kernel", dr::refit_homography_bwd_kernel<T>, dim3(P), dr::kHRThreads, stream, matches,  \
                      mask, weights, grad_model, N, grad_matches, grad_weights);                                                    \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
