// Robust 3-D registration (ransac.BatchedRegistration): rigid models from minimal samples by a correct Kabsch fit, MSAC score and
// inlier count of every model against every point, the per-pair state step with the adaptive stop, and the Kabsch refit over the
// rows a mask selects; for train mode the fit of explicit (weighted) samples and the backward of both fits (kabsch3_bwd).
//   matches [P,N,6] = (p, q); a model is the row-major 4x4 [[R, t], [0, 0, 0, 1]]; q_hat = R p + t, d2 = |q - q_hat|^2.
//   The threshold is a DISTANCE and enters as thr2 = threshold^2 per pair: inlier <=> d2 < thr2 (dr_rigid_residual compares d2
//   with its threshold argument itself).  MSAC score = sum_n max(0, 1 - d2_n / thr2).
// Unlike dr_solve_rigid (the reference's estimate_model, kept for parity with its training branch: cov^T cov with flag, the
// row-sum translation of rigid...:66) this is the least-squares rigid fit: R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T,
// t = c1 - R c0.
#include "pair_state_device.hpp"
#include "rigid_device.hpp"
#include "solver_common.hpp"

namespace dr {

// ---- the 3x3 step shared by the minimal solver and the refit -------------------------------------------------------------
// one Hestenes (one-sided Jacobi) rotation: makes columns ga, gb of G = H V orthogonal, V's columns follow
__device__ __forceinline__ void hestenes_rotate(double (&ga)[3], double (&gb)[3], double (&va)[3], double (&vb)[3]) {
  const double a = ga[0] * ga[0] + ga[1] * ga[1] + ga[2] * ga[2];
  const double b = gb[0] * gb[0] + gb[1] * gb[1] + gb[2] * gb[2];
  const double c = ga[0] * gb[0] + ga[1] * gb[1] + ga[2] * gb[2];
  const double h = b - a;
  const double x = h * h + 4.0 * c * c;
  if (!(fabs(c) > 1e-300) || !(x > 1e-280) || !is_finite(x)) return;
  const double t = (h >= 0 ? 2.0 * c : -2.0 * c) / (fabs(h) + sqrt(x));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double g0 = ga[i], g1 = gb[i], v0 = va[i], v1 = vb[i];
    ga[i] = cs * g0 - sn * g1;
    gb[i] = sn * g0 + cs * g1;
    va[i] = cs * v0 - sn * v1;
    vb[i] = sn * v0 + cs * v1;
  }
}

// H = sum w (p - c0)(q - c1)^T, c = (c0, c1) -> R, t; false (R, t = identity) when the caller's sample or selection is not `usable`,
// anything is non-finite or H has fewer than two usable singular directions.  The construction of rigid_kernel (its shared steps
// are rigid_device.hpp's): jacobi_eig3 of H^T H, the two dominant right vectors v0, v1, left vectors by H v, Gram-Schmidt, third
// vectors by cross products -- R = [v0 v1 v0xv1][u0 u1 u0xu1]^T is a proper rotation, equal to V diag(1, 1, det(V U^T)) U^T.
// Two things are added to it here, because this result is compared with an SVD:
//  - H^T H squares the conditioning, and its eigenvectors come out to eps sigma_1^2 / sigma_2^2; two Hestenes sweeps on G = H V
//    (one-sided rotations, which work on H itself) bring them to the eps sigma_1 / sigma_2 of the rotation's own conditioning;
//  - the degeneracy rule "second eigenvalue of H^T H <= 1e-24 x the first" is evaluated on the Rayleigh quotients |H v1|^2 and
//    |H v0|^2 after that: the diagonal the two-sided Jacobi leaves carries eps lambda_1 of rotation residue, which would make an
//    exactly collinear sample look like sigma_2 = 1e-8 sigma_1.
__device__ __forceinline__ bool kabsch3(const double (&H)[3][3], const double (&c)[6], bool usable, double (&R)[3][3],
                                        double (&t)[3]) {
  bool ok = usable;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) ok = ok && is_finite(H[i][j]);
#pragma unroll
  for (int d = 0; d < 6; ++d) ok = ok && is_finite(c[d]);
  double ata[3][3], V[3][3], ev[3];
  gram3(H, ata);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) ata[i][j] = ok ? ata[i][j] : (i == j ? 1.0 : 0.0);
  jacobi_eig3(ata, V, ev);
  double v[3][3];   // v[c] = column c of V, sorted by descending eigenvalue below
#pragma unroll
  for (int cidx = 0; cidx < 3; ++cidx)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[cidx][k] = V[k][cidx];
  sort3_desc(ev, v);
  double g[3][3];   // g[c] = H v[c]
#pragma unroll
  for (int cidx = 0; cidx < 3; ++cidx)
#pragma unroll
    for (int k = 0; k < 3; ++k) g[cidx][k] = H[k][0] * v[cidx][0] + H[k][1] * v[cidx][1] + H[k][2] * v[cidx][2];
#pragma unroll
  for (int sweep = 0; sweep < 2; ++sweep) {
    hestenes_rotate(g[0], g[1], v[0], v[1]);
    hestenes_rotate(g[0], g[2], v[0], v[2]);
    hestenes_rotate(g[1], g[2], v[1], v[2]);
  }
  double n2[3];
#pragma unroll
  for (int cidx = 0; cidx < 3; ++cidx) n2[cidx] = g[cidx][0] * g[cidx][0] + g[cidx][1] * g[cidx][1] + g[cidx][2] * g[cidx][2];
  sort3_desc(n2, v, g);
  double u0[3], u1[3], v0[3], v1[3];
  const double s1sq = n2[0];
  const double r0 = 1.0 / sqrt(s1sq);
#pragma unroll
  for (int k = 0; k < 3; ++k) { u0[k] = g[0][k] * r0; v0[k] = v[0][k]; }
  const double du = u0[0] * g[1][0] + u0[1] * g[1][1] + u0[2] * g[1][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) u1[k] = g[1][k] - du * u0[k];
  const double s2sq = u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2];
  ok = ok && s2sq > 1e-24 * s1sq;      // (false for NaN and for s1sq = 0)
  const double r1 = 1.0 / sqrt(s2sq);
  const double dv = v0[0] * v[1][0] + v0[1] * v[1][1] + v0[2] * v[1][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) { u1[k] *= r1; v1[k] = v[1][k] - dv * v0[k]; }
  const double rv = 1.0 / sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) v1[k] *= rv;
  ok = ok && rotation_from_frames(v0, v1, u0, u1, R);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = c[3 + i] - (R[i][0] * c[0] + R[i][1] * c[1] + R[i][2] * c[2]);
    ok = ok && is_finite(t[i]);
  }
  if (!ok) set_identity(R, t);
  return ok;
}

// ---- the derivative of the fit: (gR, gt) -> (gH, g_c0, g_c1) -----------------------------------------------------------------
// The optimum is characterised by A = R H being symmetric (A = V D S V^T).  A perturbation dH turns R by exp([w]x) with
// K w = -vee(R dH - dH^T R^T), K = tr(A) I - A (symmetric, eigenvalues s1 + s2, s1 + d s3, s2 + d s3), so no SVD is differentiated:
//   G = gR - gt c0^T (t = c1 - R c0), g_c1 = gt, g_c0 = -R^T gt;  Y = G R^T, a = vee(Y - Y^T), z = K^-1 a (adjugate);  gH = -R^T [z]x.
// false (everything zero) when the forward was not `ok`, or det K or any result is not finite: a sample without a usable model, or
// one at the reflection tie / collinear limit where the rotation is not differentiable, passes no gradient on.
__device__ __forceinline__ bool kabsch3_bwd(const double (&H)[3][3], const double (&c)[6], const double (&R)[3][3], bool ok,
                                            const double (&gR)[3][3], const double (&gt)[3], double (&gH)[3][3], double (&gc0)[3],
                                            double (&gc1)[3]) {
  double A[3][3], Y[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[i][j] = R[i][0] * H[0][j] + R[i][1] * H[1][j] + R[i][2] * H[2][j];
      Y[i][j] = (gR[i][0] - gt[i] * c[0]) * R[j][0] + (gR[i][1] - gt[i] * c[1]) * R[j][1] + (gR[i][2] - gt[i] * c[2]) * R[j][2];
    }
  const double tr = A[0][0] + A[1][1] + A[2][2];
  const double k00 = tr - A[0][0], k11 = tr - A[1][1], k22 = tr - A[2][2];
  const double k01 = -0.5 * (A[0][1] + A[1][0]), k02 = -0.5 * (A[0][2] + A[2][0]), k12 = -0.5 * (A[1][2] + A[2][1]);
  const double a[3] = {Y[2][1] - Y[1][2], Y[0][2] - Y[2][0], Y[1][0] - Y[0][1]};
  const double c00 = k11 * k22 - k12 * k12, c01 = k02 * k12 - k01 * k22, c02 = k01 * k12 - k02 * k11;
  const double c11 = k00 * k22 - k02 * k02, c12 = k01 * k02 - k00 * k12, c22 = k00 * k11 - k01 * k01;
  const double det = k00 * c00 + k01 * c01 + k02 * c02;
  const double rd = 1.0 / det;
  const double z[3] = {(c00 * a[0] + c01 * a[1] + c02 * a[2]) * rd, (c01 * a[0] + c11 * a[1] + c12 * a[2]) * rd,
                       (c02 * a[0] + c12 * a[1] + c22 * a[2]) * rd};
  const double Z[3][3] = {{0.0, -z[2], z[1]}, {z[2], 0.0, -z[0]}, {-z[1], z[0], 0.0}};
  ok = ok && is_finite(det);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gc1[i] = gt[i];
    gc0[i] = -(R[0][i] * gt[0] + R[1][i] * gt[1] + R[2][i] * gt[2]);
    ok = ok && is_finite(gc0[i]) && is_finite(gc1[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      gH[i][j] = -(R[0][i] * Z[0][j] + R[1][i] * Z[1][j] + R[2][i] * Z[2][j]);
      ok = ok && is_finite(gH[i][j]);
    }
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      gc0[i] = gc1[i] = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) gH[i][j] = 0.0;
    }
  }
  return ok;
}

// ---- the two accumulations of every fit here, f64: one row x = (p, q) of weight w into the weighted sums a[0..5] and the weight sum,
// and, once the means c = (c0, c1) are known, into H = sum w (p - c0)(q - c1)^T.  The per-lane fit of a sample (1) and the per-block
// fit of a selection (4) share this text, so they round alike; unit weights give the bits of the plain sums (x 1.0 is exact)
template <typename T>
__device__ __forceinline__ void moment_sums(const T *x, double w, double *a, double &W) {
#pragma unroll
  for (int d = 0; d < 6; ++d) a[d] += w * (double)x[d];
  W += w;
}

template <typename T>
__device__ __forceinline__ void moment_outer(const T *x, double w, const double (&c)[6], double (&H)[3][3]) {
  double dp[3], dq[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    dp[d] = w * ((double)x[d] - c[d]);
    dq[d] = (double)x[3 + d] - c[3 + d];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] += dp[i] * dq[j];
}

// ---- (1) minimal samples -> rigid models: one lane = one sample of 3 <= k <= 8 rows -----------------------------------------
// the weighted means c = (c0, c1), H and W = sum w of one sample: rowp(r) -> the six values of row r, wt(r) -> its weight (W = k
// without weights)
template <typename RowFn, typename WFn>
__device__ __forceinline__ double sample_moments(int k, RowFn rowp, WFn wt, double (&c)[6], double (&H)[3][3]) {
  double W = 0.0;
#pragma unroll
  for (int d = 0; d < 6; ++d) c[d] = 0.0;
  for (int r = 0; r < k; ++r) moment_sums(rowp(r), wt(r), c, W);
  const double rn = 1.0 / W;
#pragma unroll
  for (int d = 0; d < 6; ++d) c[d] *= rn;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = 0.0;
  for (int r = 0; r < k; ++r) moment_outer(rowp(r), wt(r), c, H);
  return W;
}

// rows read through the index sets
template <typename T>
__global__ __launch_bounds__(64) void kabsch_gather_kernel(const T *__restrict__ matches, const int32_t *__restrict__ idx, int Bt,
                                                           int B, int N, int k, T *__restrict__ models,
                                                           uint8_t *__restrict__ valid) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= Bt) return;
  const T *base = matches + (size_t)(s / B) * N * 6;
  const int32_t *gi = idx + (size_t)s * k;
  bool in_range = true;
  for (int r = 0; r < k; ++r) in_range = in_range && gi[r] >= 0 && gi[r] < N;
  auto rowp = [&](int r) -> const T * { return base + (size_t)(in_range ? gi[r] : 0) * 6; };   // (a bad index reads row 0, valid = 0)
  double c[6], H[3][3], R[3][3], t[3];
  sample_moments(k, rowp, [](int) { return 1.0; }, c, H);
  valid[s] = kabsch3(H, c, in_range, R, t);
  store_rigid_model(models + (size_t)s * 16, R, t);
}

// ---- (1b) the same behind a rigidity test of the sample (BatchedRegistration(edge_similarity = ...)) ------------------------------
// A rigid motion keeps distances, so a sample of inliers has |p_i - p_j| ~ |q_i - q_j| for every pair of its rows.  With
// sigma = edge_similarity^2 an edge passes iff a2 >= sigma b2 && b2 >= sigma a2, a2 = |p_i - p_j|^2, b2 = |q_i - q_j|^2 in f64 from
// the stored values (Open3D's CorrespondenceCheckerBasedOnEdgeLength on squares; false for a NaN, true for two coincident rows, which
// kabsch3 then rejects); a sample passes iff all k (k - 1) / 2 edges do.  A sample with an index out of range is what (1) makes of it
// (identity, valid = 0) and is not counted; one that fails is the identity with valid = 0 and counts once in rejected[pair] (integer
// atomics: the same total on every launch); one that passes goes through (1)'s sample_moments and kabsch3 on the same rows in the same
// order, so its 16 values and its valid byte are (1)'s bit for bit.
// Mapping: the test is a few loads and compares, the fit some 1800 f64 instructions, and with one lane per sample a wave runs the fit
// as soon as one of its 64 samples survives (at 1 % survivors: 47 % of the waves).  So a block of 256 samples works in two phases:
//  1. every lane tests its own sample; a lane whose sample leaves here stores the identity.  The survivors' numbers are compacted into
//     LDS in ascending order: ballot and prefix count inside the wave, the four wave counts in order across them.
//  2. lane j < survivors fits survivor j and stores it at that sample's own slot: the waves of phase 2 are full but the last, and a
//     block without survivors runs no fit at all.  The output is not compacted, only the work; a fit does not depend on its lane.
constexpr int kCKThreads = 256;

template <typename T>
__global__ __launch_bounds__(kCKThreads) void kabsch_gather_checked_kernel(const T *__restrict__ matches,
                                                                           const int32_t *__restrict__ idx, int Bt, int B, int N, int k,
                                                                           double sigma, T *__restrict__ models,
                                                                           uint8_t *__restrict__ valid, int32_t *__restrict__ rejected) {
  __shared__ int s_wcnt[kCKThreads / 64];
  __shared__ int s_list[kCKThreads];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s0 = blockIdx.x * kCKThreads, s = s0 + tid;
  bool pass = false, dropped = false;   // (both false past the end and for an index out of range)
  if (s < Bt) {
    const T *base = matches + (size_t)(s / B) * N * 6;
    const int32_t *gi = idx + (size_t)s * k;
    bool in_range = true;
    for (int r = 0; r < k; ++r) in_range = in_range && gi[r] >= 0 && gi[r] < N;
    if (in_range) {
      pass = true;
      for (int i = 0; i + 1 < k; ++i) {
        const T *xi = base + (size_t)gi[i] * 6;
        double x[6];
#pragma unroll
        for (int d = 0; d < 6; ++d) x[d] = (double)xi[d];
        for (int j = i + 1; j < k; ++j) {
          const T *xj = base + (size_t)gi[j] * 6;
          double a2 = 0.0, b2 = 0.0;
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const double da = x[d] - (double)xj[d], db = x[3 + d] - (double)xj[3 + d];
            a2 += da * da;
            b2 += db * db;
          }
          pass = pass && a2 >= sigma * b2 && b2 >= sigma * a2;
        }
      }
      dropped = !pass;
    }
    if (!pass) {
      double R[3][3], t[3];
      set_identity(R, t);
      store_rigid_model(models + (size_t)s * 16, R, t);
      valid[s] = 0;
    }
  }
  const int w0 = s0 + wv * 64;          // the wave's first sample; its samples may belong to several pairs
  if (rejected && w0 < Bt) {            // (wave-uniform)
    const int p_last = min(w0 + 63, Bt - 1) / B;
    for (int p = w0 / B; p <= p_last; ++p) {
      const int n = __popcll(__ballot(dropped && s / B == p));
      if (lane == 0 && n) atomicAdd(rejected + p, n);
    }
  }
  const unsigned long long survivors = __ballot(pass);
  if (lane == 0) s_wcnt[wv] = __popcll(survivors);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kCKThreads / 64; ++w) {
    before += w < wv ? s_wcnt[w] : 0;
    total += s_wcnt[w];
  }
  if (pass) s_list[before + __popcll(survivors & ((1ull << lane) - 1ull))] = tid;
  __syncthreads();
  if (tid < total) {                    // phase 2: (1)'s fit of survivor tid, whose indices are in range
    const int f = s0 + s_list[tid];
    const T *base = matches + (size_t)(f / B) * N * 6;
    const int32_t *gi = idx + (size_t)f * k;
    double c[6], H[3][3], R[3][3], t[3];
    sample_moments(k, [&](int r) { return base + (size_t)gi[r] * 6; }, [](int) { return 1.0; }, c, H);
    valid[f] = kabsch3(H, c, true, R, t);
    store_rigid_model(models + (size_t)f * 16, R, t);
  }
}

// explicit sample tensors [Bt,k,6] with optional weights [Bt,k]: what train mode fits (the straight-through samples of SampleGather).
// Without weights, on samples = matches[idx], the models and validity of kabsch_gather_kernel bit for bit.
template <typename T>
__global__ __launch_bounds__(64) void kabsch_kernel(const T *__restrict__ samples, const T *__restrict__ weights, int Bt, int k,
                                                    T *__restrict__ models, uint8_t *__restrict__ valid) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= Bt) return;
  const T *base = samples + (size_t)s * k * 6;
  const T *wb = weights ? weights + (size_t)s * k : nullptr;
  double c[6], H[3][3], R[3][3], t[3];
  const double W = sample_moments(k, [&](int r) { return base + r * 6; }, [&](int r) { return wb ? (double)wb[r] : 1.0; }, c, H);
  valid[s] = kabsch3(H, c, W > 0.0, R, t);
  store_rigid_model(models + (size_t)s * 16, R, t);
}

// its backward: the forward recomputed in f64 from the inputs (no stored model), rows re-read for the third pass; every output element
// is written, exact zeros for a sample without a valid fit or a finite derivative.  Only rows 0..2 of grad_models are read.
template <typename T>
__global__ __launch_bounds__(64) void kabsch_bwd_kernel(const T *__restrict__ samples, const T *__restrict__ weights,
                                                        const T *__restrict__ grad_models, int Bt, int k, T *__restrict__ grad_samples,
                                                        T *__restrict__ grad_weights) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= Bt) return;
  const T *base = samples + (size_t)s * k * 6;
  const T *wb = weights ? weights + (size_t)s * k : nullptr;
  double c[6], H[3][3], R[3][3], t[3];
  const double W = sample_moments(k, [&](int r) { return base + r * 6; }, [&](int r) { return wb ? (double)wb[r] : 1.0; }, c, H);
  const bool fwd = kabsch3(H, c, W > 0.0, R, t);
  const T *gm = grad_models + (size_t)s * 16;
  double gR[3][3], gt[3], gH[3][3], gc0[3], gc1[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) gR[i][j] = (double)gm[4 * i + j];
    gt[i] = (double)gm[4 * i + 3];
  }
  const bool ok = kabsch3_bwd(H, c, R, fwd, gR, gt, gH, gc0, gc1);
  const double rW = 1.0 / W;
  T *gs = grad_samples + (size_t)s * k * 6;
  for (int r = 0; r < k; ++r) {
    const T *x = base + r * 6;
    const double w = wb ? (double)wb[r] : 1.0;
    double dp[3], dq[3], gw = 0.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      dp[d] = (double)x[d] - c[d];
      dq[d] = (double)x[3 + d] - c[3 + d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double hq = gH[d][0] * dq[0] + gH[d][1] * dq[1] + gH[d][2] * dq[2];      // (gH dq)_d
      const double hp = gH[0][d] * dp[0] + gH[1][d] * dp[1] + gH[2][d] * dp[2];      // (gH^T dp)_d
      gs[r * 6 + d] = ok ? (T)(w * (hq + rW * gc0[d])) : T(0);
      gs[r * 6 + 3 + d] = ok ? (T)(w * (hp + rW * gc1[d])) : T(0);
      gw += dp[d] * hq + rW * (dp[d] * gc0[d] + dq[d] * gc1[d]);
    }
    if (grad_weights) grad_weights[(size_t)s * k + r] = ok ? (T)gw : T(0);
  }
}

// ---- (2) score and inlier count of every model against every point: pair_state_device.hpp's pair_score_kernel under RigidGeom and one
// of the two terms below; the polish kernels (5), (6) score their candidates with the same terms through its pair_block_score.
// MSAC: max(0, 1 - d2 / thr2).  The contribution and the count keep their own predicates (sv > 0 and d2 < thr2 can differ by a rounding)
template <typename T>
struct MsacTerm {
  T t2, inv;
  __device__ __forceinline__ explicit MsacTerm(T thr2) : t2(thr2), inv(T(1) / thr2) {}
  __device__ __forceinline__ bool inlier(T d2) const { return d2 < t2; }                  // (false for NaN)
  __device__ __forceinline__ T contrib(T d2, bool live = true) const {
    const T sv = T(1) - d2 * inv;
    return (live && sv > T(0)) ? sv : T(0);
  }
};

// ---- (2b) the MAGSAC++ term --------------------------------------------------------------------------------------------------------
// The cutoff distance is read as k sigma_max, k^2 = the 0.99 quantile of chi^2 with 3 degrees of freedom (the residual is a 3-vector),
// the noise scale uniform in [0, sigma_max].  With s = d2 / thr2, u_k = k^2 / 2, c = exp(-u_k):
//   weight  w(s) = (exp(-u_k s) - c) / (1 - c)                              for s < 1, else 0
//   loss    l(s) = (1 - exp(-u_k s) - c u_k s) / (1 - c (1 + u_k))          for s < 1, else 1     (int_0^d x w(x) dx over its value at the cutoff)
//   score        = sum_n (1 - l(s_n)),  1 - l(s) = A e + B s + C,  e = exp(-u_k s),  A = 1 / D,  B = c u_k / D,  C = -c (1 + u_k) / D,
//                  D = 1 - c (1 + u_k);   inlier <=> d2 < thr2, the test of (2); a NaN distance contributes nothing.
// The constants are f64 literals (u_k = 11.344866730144373 / 2 and what follows from it, rounded once to T); the division by thr2 is
// folded into the factors of d2 once per block.
constexpr double kMagUk = 5.6724333650721865;          // k^2 / 2
constexpr double kMagA = 1.0234888000258247;           // 1 / D
constexpr double kMagB = 0.019968525076541437;         // c u_k / D
constexpr double kMagC0 = -0.02348880002582457;        // -c (1 + u_k) / D
constexpr double kMagW1 = 1.0034513564514345;          // 1 / (1 - c)
constexpr double kMagW0 = -0.0034513564514345773;      // -c / (1 - c)
constexpr double kLog2e = 1.44269504088896340736;

// exp(-u_k s) as f(d2 x): x = -u_k log2(e) / thr2 for f32, -u_k / thr2 for f64.
//  f32: __builtin_amdgcn_exp2f = v_exp_f32, 1 ulp (the V_EXP_F32 entry of the CDNA ISA guide); for an inlier the argument lies in
//       [-8.19, 0], so the result is a normal number and the instruction's flush of denormals plays no part.
//  f64: exp of the device library (OCML), 1 ulp (the double-precision table of the HIP math API reference).
__device__ __forceinline__ float magsac_exp(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ double magsac_exp(double x) { return exp(x); }

template <typename T>
struct MagsacTerm {
  T t2, xs, b;      // thr2, the factor of d2 in the exponential's argument, B / thr2
  __device__ __forceinline__ explicit MagsacTerm(T thr2) : t2(thr2) {
    const T inv = T(1) / thr2;
    xs = (T)(sizeof(T) == 4 ? -kMagUk * kLog2e : -kMagUk) * inv;
    b = (T)kMagB * inv;
  }
  __device__ __forceinline__ bool inlier(T d2) const { return d2 < t2; }                  // (false for NaN)
  __device__ __forceinline__ T gain(T d2) const {                                         // 1 - l(s) where inlier(d2)
    return fma(magsac_exp(d2 * xs), (T)kMagA, fma(d2, b, (T)kMagC0));
  }
  __device__ __forceinline__ T contrib(T d2, bool live = true) const { return (live && inlier(d2)) ? gain(d2) : T(0); }
  __device__ __forceinline__ T weight(T d2) const {                                       // w(s) where inlier(d2); >= 0
    const T w = fma(magsac_exp(d2 * xs), (T)kMagW1, (T)kMagW0);
    return w > T(0) ? w : T(0);
  }
};

// ---- (3) the state step is pair_update_kernel under RigidGeom

// ---- (4) Kabsch refit over the rows a mask selects: one block per pair, f64, two passes, fixed-order reduction ---------------
constexpr int kRFThreads = kPairThreads;

template <typename T>
__device__ __forceinline__ void load_row(const T *pt, int n, T (&x)[6]) {
#pragma unroll
  for (int d = 0; d < 6; ++d) x[d] = pt[(size_t)n * 6 + d];
}

// the two passes of the fit, by the whole block: -> c = (c0, c1), H, rows = the rows that took part, the weight sum (every thread
// holds all of them afterwards).  `row` says which rows take part, in two steps, so that a row is dropped as early as its kind allows:
// row.present(n) before anything of the row is loaded, then row.load(n, x, w), which delivers the six values and the weight and may
// still drop the row.  Both passes ask, so it must answer alike.  Thread n owns rows n, n + 256, ...
template <typename T, typename RowFn>
__device__ __forceinline__ double block_moments(int N, RowFn row, double (*s_red)[9], double (&c)[6], double (&H)[3][3],
                                                double &rows) {
  const int tid = threadIdx.x;
  // pass 1: weighted sums of p and q, the weight sum and the row count (entries 0..5, 6, 7; entry 8 unused)
  double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int n = tid; n < N; n += kRFThreads) {
    if (!row.present(n)) continue;
    T x[6];
    double w;
    if (!row.load(n, x, w)) continue;
    moment_sums(x, w, a, a[6]);
    a[7] += 1.0;
  }
  block_sum_f64<9>(a, s_red);
  rows = a[7];
  const double rw = 1.0 / a[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) c[d] = a[d] * rw;
  // pass 2: H = sum w (p - c0)(q - c1)^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = 0.0;
  for (int n = tid; n < N; n += kRFThreads) {
    if (!row.present(n)) continue;
    T x[6];
    double w;
    if (!row.load(n, x, w)) continue;
    moment_outer(x, w, c, H);
  }
  block_sum_f64<9>(&H[0][0], s_red);
  return a[6];
}

// the rows of (4) and (5): the mask byte first -- a row it drops is not loaded --, then the row, then the optional weight tensor
template <typename T>
struct MaskedRows {
  const T *pt;
  const uint8_t *mk;      // nullptr = every row
  const T *wt;            // nullptr = unit weights
  __device__ __forceinline__ bool present(int n) const { return !mk || mk[n]; }
  __device__ __forceinline__ bool load(int n, T (&x)[6], double &w) const {
    load_row(pt, n, x);
    w = wt ? (double)wt[n] : 1.0;
    return true;
  }
};

template <typename T>
__global__ __launch_bounds__(kRFThreads) void refit_rigid_kernel(const T *__restrict__ pts, const uint8_t *__restrict__ mask,
                                                                 const T *__restrict__ weights, int N, T *__restrict__ model,
                                                                 uint8_t *__restrict__ valid) {
  __shared__ double s_red[kRFThreads / 64][9];
  const int p = blockIdx.x;
  const MaskedRows<T> sel{pts + (size_t)p * N * 6, mask ? mask + (size_t)p * N : nullptr, weights ? weights + (size_t)p * N : nullptr};
  double c[6], H[3][3], rows;
  const double W = block_moments<T>(N, sel, s_red, c, H, rows);
  if (threadIdx.x != 0) return;
  double R[3][3], t[3];
  valid[p] = kabsch3(H, c, rows >= 3.0 && W > 0.0, R, t);
  store_rigid_model(model + (size_t)p * 16, R, t);
}

// its backward: the same two passes (same order, same bits), thread 0 runs the fit and kabsch3_bwd and hands gH, g_c0, g_c1, 1 / W
// to the block through LDS, a third pass writes the gradient of EVERY row -- element by element, so a wave's stores are contiguous --
// with exact zeros for the rows the mask drops and for a pair without a valid fit.  No atomics: a repeated launch gives the same bits.
template <typename T>
__global__ __launch_bounds__(kRFThreads) void refit_rigid_bwd_kernel(const T *__restrict__ pts, const uint8_t *__restrict__ mask,
                                                                     const T *__restrict__ weights, const T *__restrict__ grad_model,
                                                                     int N, T *__restrict__ grad_matches,
                                                                     T *__restrict__ grad_weights) {
  __shared__ double s_red[kRFThreads / 64][9];
  __shared__ double s_g[16];   // gH (9), g_c0 (3), g_c1 (3), 1 / W
  __shared__ int s_ok;
  const int p = blockIdx.x, tid = threadIdx.x;
  const T *pt = pts + (size_t)p * N * 6;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T *wt = weights ? weights + (size_t)p * N : nullptr;
  double c[6], H[3][3], rows;
  const double W = block_moments<T>(N, MaskedRows<T>{pt, mk, wt}, s_red, c, H, rows);
  if (tid == 0) {
    const T *gm = grad_model + (size_t)p * 16;
    double R[3][3], t[3], gR[3][3], gt[3], gH[3][3], gc0[3], gc1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) gR[i][j] = (double)gm[4 * i + j];
      gt[i] = (double)gm[4 * i + 3];
    }
    const bool fwd = kabsch3(H, c, rows >= 3.0 && W > 0.0, R, t);
    s_ok = kabsch3_bwd(H, c, R, fwd, gR, gt, gH, gc0, gc1);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) s_g[3 * i + j] = gH[i][j];
      s_g[9 + i] = gc0[i];
      s_g[12 + i] = gc1[i];
    }
    s_g[15] = 1.0 / W;
  }
  __syncthreads();
  const bool ok = s_ok != 0;
  const double rW = s_g[15];
  if (grad_matches) {
    T *gx = grad_matches + (size_t)p * N * 6;
    for (int e = tid; e < 6 * N; e += kRFThreads) {
      const int n = e / 6, d = e - 6 * n;
      double v = 0.0;
      if (ok && (!mk || mk[n])) {
        const double w = wt ? (double)wt[n] : 1.0;
        if (d < 3) {   // w (gH dq + g_c0 / W)_d
          const double dq[3] = {(double)pt[(size_t)n * 6 + 3] - c[3], (double)pt[(size_t)n * 6 + 4] - c[4],
                                (double)pt[(size_t)n * 6 + 5] - c[5]};
          v = w * (s_g[3 * d] * dq[0] + s_g[3 * d + 1] * dq[1] + s_g[3 * d + 2] * dq[2] + rW * s_g[9 + d]);
        } else {       // w (gH^T dp + g_c1 / W)_j
          const int j = d - 3;
          const double dp[3] = {(double)pt[(size_t)n * 6] - c[0], (double)pt[(size_t)n * 6 + 1] - c[1],
                                (double)pt[(size_t)n * 6 + 2] - c[2]};
          v = w * (s_g[j] * dp[0] + s_g[3 + j] * dp[1] + s_g[6 + j] * dp[2] + rW * s_g[12 + j]);
        }
      }
      gx[e] = (T)v;
    }
  }
  if (grad_weights) {
    T *gw = grad_weights + (size_t)p * N;
    for (int n = tid; n < N; n += kRFThreads) {
      double v = 0.0;
      if (ok && (!mk || mk[n])) {
        double dp[3], dq[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          dp[d] = (double)pt[(size_t)n * 6 + d] - c[d];
          dq[d] = (double)pt[(size_t)n * 6 + 3 + d] - c[3 + d];
        }
#pragma unroll
        for (int d = 0; d < 3; ++d)
          v += dp[d] * (s_g[3 * d] * dq[0] + s_g[3 * d + 1] * dq[1] + s_g[3 * d + 2] * dq[2]) +
               rW * (dp[d] * s_g[9 + d] + dq[d] * s_g[12 + d]);
      }
      gw[n] = (T)v;
    }
  }
}

// ---- (5) local optimisation of the pair state (BatchedRegistration(lo = 1 / 2)): one block per pair, right behind (3) ----------
// A pair whose (best_score, best_model) still equals its snapshot lo_seen[p] bit for bit -- only (3) replaces them, and the snapshot
// starts as NaN -- returns at once, whether or not it has terminated.  Otherwise pair_state_device.hpp's accept loop (pair_polish: the
// mapping and the sum order are stated there) with four things of its own, which is why it is written out here: a fit counts whether
// or not it is valid; the score pass counts the inliers too; an accepted candidate is followed by a pass that rewrites the mask and
// compares it with the old one, and the loop also ends on an accepted mask that equals the previous one (the next fit would see the
// same rows); and the write-back adds the inlier count, max_iters from it, the snapshot, and lo_refits[p] += fits run.  The fit is
// (4)'s over the best mask (block_moments + kabsch3, f64; every thread runs kabsch3 on the block's sums).  Below three inliers only
// the snapshot is stored.
// The candidate's mask is not held anywhere before acceptance: the accepting pass evaluates term.inlier(rigid_d2) again, the same
// expression on the same values as the counting pass, so the count is the written mask's count, for every N.  Thread n owns points
// n, n + 256, ... in every pass, mask bytes included; a pass has 6 ceil(N / 256) independent loads per thread in flight.
template <typename T>
__global__ __launch_bounds__(kRFThreads) void registration_local_opt_kernel(
    const T *__restrict__ pts, const T *__restrict__ thr2, int N, int iters, double confidence, double eps, int max_iterations,
    T *__restrict__ best_score, T *__restrict__ best_model, uint8_t *__restrict__ best_mask, int32_t *__restrict__ best_inliers,
    double *__restrict__ max_iters, T *__restrict__ lo_seen, int32_t *__restrict__ lo_refits) {
  __shared__ double s_red[kRFThreads / 64][9];
  __shared__ T s_part[kRFThreads / 64];
  __shared__ int s_cnt[kRFThreads / 64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const T *pt = pts + (size_t)p * N * 6;
  uint8_t *mk = best_mask + (size_t)p * N;
  T *seen = lo_seen + (size_t)p * 17;
  T bs = best_score[p];
  T bm[16];
  bool same = same_bits(bs, seen[0]);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    bm[q] = best_model[(size_t)p * 16 + q];
    same = same && same_bits(bm[q], seen[1 + q]);
  }
  int inl = best_inliers[p];
  __syncthreads();      // (every thread has read the state and the snapshot: thread 0 writes them below)
  if (same) return;     // block-uniform: no replacement since the last visit
  const MsacTerm<T> term(thr2[p]);
  const MaskedRows<T> sel{pt, mk, nullptr};
  const bool run = inl >= 3;
  bool taken = false;
  int fits = 0;
  for (int it = 0; run && it < iters; ++it) {
    double c[6], H[3][3], rows, R[3][3], t[3];
    const double W = block_moments<T>(N, sel, s_red, c, H, rows);
    bool ok = kabsch3(H, c, rows >= 3.0 && W > 0.0, R, t);
    ++fits;
    T m[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) m[4 * i + j] = (T)R[i][j];
      m[4 * i + 3] = (T)t[i];
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) ok = ok && is_finite(m[q]);
    if (!ok) break;     // (block-uniform, like every exit below: all threads hold the same sums)
    RigidGeom::Slot<T> cs;
    RigidGeom::prepare(m, cs);
    int cnt;
    const T sc = pair_block_score<T, RigidGeom>(pt, N, cs, term, s_part, s_cnt, &cnt);
    if (!(sc > bs)) break;
    int chg = 0;
    for (int n = tid; n < N; n += kRFThreads) {
      T x[6];
      load_row(pt, n, x);
      const uint8_t in = term.inlier(rigid_d2<T>(m, x));
      chg |= in != mk[n];
      mk[n] = in;
    }
    chg = wave_sum(chg);
    if (lane == 0) s_cnt[wv] = chg;
    __syncthreads();
    const bool changed = (s_cnt[0] | s_cnt[1] | s_cnt[2] | s_cnt[3]) != 0;   // (next written behind block_moments' barriers)
    bs = sc;
    inl = cnt;
    taken = true;
#pragma unroll
    for (int q = 0; q < 12; ++q) bm[q] = m[q];
    bm[12] = bm[13] = bm[14] = T(0);
    bm[15] = T(1);
    if (!changed) break;
  }
  if (tid == 0) {
    if (taken) {
      best_score[p] = bs;
      best_inliers[p] = inl;
#pragma unroll
      for (int q = 0; q < 16; ++q) best_model[(size_t)p * 16 + q] = bm[q];
    }
    if (run) max_iters[p] = adaptive_max_iters(inl, N, 3, confidence, eps, max_iterations);
    seen[0] = bs;
#pragma unroll
    for (int q = 0; q < 16; ++q) seen[1 + q] = bm[q];
    if (lo_refits) lo_refits[p] += fits;
  }
}

// ---- (6) IRLS polish of the pair state under the MAGSAC++ loss (BatchedRegistration(scoring = "magsac")): pair_polish under this fit ----
// The sigma-consensus++ step: the weights w(s_n) of (2b) under the current model, the weighted fit over ALL points (block_moments with
// these weights, kabsch3; f64).  Nothing is fitted when fewer than three points have d2 < thr2 (the points with a non-zero weight);
// that exit is taken on the row count block_moments returns, so its second pass has run by then: one more pass over the points, over
// means that are inf / NaN when the weight sum is 0 -- nothing of it is used or stored.  Every thread runs kabsch3 on the block's sums
// (same inputs, same instructions, same bits): no broadcast and no barrier between the fit and the score pass.  The weights are not
// stored: passes 1 and 2 evaluate the same expression on the same values.  The mask stays the RANSAC winner's, as with the single
// final refit of the MSAC path.
// the rows of a step: those inside the cutoff under the current model, with the weight of (2b)
template <typename T>
struct CutoffRows {
  const T *pt;
  const T (&m)[12];
  const MagsacTerm<T> &term;
  __device__ __forceinline__ bool present(int) const { return true; }
  __device__ __forceinline__ bool load(int n, T (&x)[6], double &w) const {
    load_row(pt, n, x);
    const T d2 = rigid_d2<T>(m, x);
    if (!term.inlier(d2)) return false;
    w = (double)term.weight(d2);
    return true;
  }
};

template <typename T>
struct RigidIrlsFit {
  const T *pt;
  int N;
  const MagsacTerm<T> &term;
  double (*s_red)[9];
  __device__ __forceinline__ int operator()(const T (&cur)[16], T (&cand)[16]) const {
    RigidGeom::Slot<T> s;
    RigidGeom::prepare(cur, s);
    double c[6], H[3][3], rows, R[3][3], t[3];
    const double W = block_moments<T>(N, CutoffRows<T>{pt, s.m, term}, s_red, c, H, rows);
    if (!(rows >= 3.0)) return kFitStop;
    const bool ok = kabsch3(H, c, W > 0.0, R, t);
    store_rigid_model(cand, R, t);
    return ok ? kFitValid : kFitInvalid;
  }
};

template <typename T>
__global__ __launch_bounds__(kRFThreads) void registration_irls_kernel(const T *__restrict__ pts, const T *__restrict__ thr2, int N,
                                                                       int iters, T *__restrict__ best_score,
                                                                       T *__restrict__ best_model, int32_t *__restrict__ irls_fits) {
  __shared__ double s_red[kRFThreads / 64][9];
  __shared__ T s_part[kRFThreads / 64];
  const int p = blockIdx.x;
  const T *pt = pts + (size_t)p * N * 6;
  const MagsacTerm<T> term(thr2[p]);
  pair_polish<T, RigidGeom>(pt, N, iters, term, RigidIrlsFit<T>{pt, N, term, s_red}, s_part, best_score + p,
                            best_model + (size_t)p * 16, irls_fits + p);
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                              \
  int dr_kabsch_gather_##sfx(const T *matches, const int32_t *idx, int P, int B, int N, int k, T *models, uint8_t *valid,           \
                             void *stream) {                                                                                        \
    DR_REQUIRE(matches && idx && models && valid, "null pointer");                                                                  \
    DR_REQUIRE(P > 0 && B > 0 && N > 0 && k >= 3 && k <= 8 && (long)P * B < (1l << 31),                                             \
               "need P, B, N > 0 and 3 <= k <= 8 rows per sample");                                                                 \
    return dr::launch("kabsch_gather_kernel", dr::kabsch_gather_kernel<T>, dim3((P * B + 63) / 64), 64, stream, matches, idx, P * B, \
                      B, N, k, models, valid);                                                                                      \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_OP(sfx, T)                                                                                                              \
  int dr_kabsch_gather_checked_##sfx(const T *matches, const int32_t *idx, int P, int B, int N, int k, double edge_similarity,      \
                                     T *models, uint8_t *valid, int32_t *rejected, void *stream) {                                  \
    DR_REQUIRE(matches && idx && models && valid, "null pointer");                                                                  \
    DR_REQUIRE(P > 0 && B > 0 && N > 0 && k >= 3 && k <= 8 && (long)P * B <= (1l << 31) - dr::kCKThreads,                           \
               "need P, B, N > 0 and 3 <= k <= 8 rows per sample");                                                                 \
    DR_REQUIRE(edge_similarity >= 0.0 && edge_similarity <= 1.0, "edge_similarity must lie in [0, 1]");   /* (false for NaN) */     \
    return dr::launch("kabsch_gather_checked_kernel", dr::kabsch_gather_checked_kernel<T>,                                          \
                      dim3((P * B + dr::kCKThreads - 1) / dr::kCKThreads), dr::kCKThreads, stream, matches, idx, P * B, B, N, k,    \
                      edge_similarity * edge_similarity, models, valid, rejected);                                                  \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_KABSCH_CHECKS(out0, out1)                   \
  DR_REQUIRE(samples && out0 && out1, "null pointer"); \
  DR_REQUIRE(Bt > 0 && k >= 3 && k <= 8, "need Bt > 0 and 3 <= k <= 8 rows per sample")

#define DR_OP(sfx, T)                                                                                                              \
  int dr_kabsch_##sfx(const T *samples, const T *weights, int Bt, int k, T *models, uint8_t *valid, void *stream) {                 \
    DR_KABSCH_CHECKS(models, valid);                                                                                                \
    return dr::launch("kabsch_kernel", dr::kabsch_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples, weights, Bt, k, models,     \
                      valid);                                                                                                       \
  }                                                                                                                                 \
  int dr_kabsch_bwd_##sfx(const T *samples, const T *weights, const T *grad_models, int Bt, int k, T *grad_samples,                 \
                          T *grad_weights, void *stream) {                                                                          \
    DR_KABSCH_CHECKS(grad_models, grad_samples);                                                                                    \
    return dr::launch("kabsch_bwd_kernel", dr::kabsch_bwd_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples, weights,            \
                      grad_models, Bt, k, grad_samples, grad_weights);                                                              \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_RIGID_SCORE(term, Term, sfx, T)                                                                                         \
  int dr_rigid_##term##_score_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *thr2, int P, int M, int N,    \
                                    T *scores, int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters,           \
                                    void *stream) {                                                                                 \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535, "bad sizes");                                                                 \
    DR_REQUIRE((gate_iters == nullptr) == (gate_max_iters == nullptr), "gate: both pointers or neither");                           \
    return dr::launch_pair_score<T, dr::RigidGeom, dr::Term<T>>(matches, models, valid, thr2, P, M, N, scores, inliers, gate_iters, \
                                                                gate_max_iters, stream);                                            \
  }
#define DR_OP(sfx, T) DR_RIGID_SCORE(msac, MsacTerm, sfx, T) DR_RIGID_SCORE(magsac, MagsacTerm, sfx, T)
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_OP(sfx, T)                                                                                                              \
  int dr_registration_update_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *scores, const T *thr2, int P,  \
                                   int M, int N, int B, double confidence, double eps, int max_iterations, T *best_score,           \
                                   T *best_model, uint8_t *best_mask, int32_t *best_inliers, int32_t *iters, double *max_iters,     \
                                   void *stream) {                                                                                  \
    DR_REQUIRE(matches && models && scores && thr2 && best_score && best_model && best_mask && best_inliers && iters && max_iters,  \
               "null pointer");                                                                                                     \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && B > 0 && max_iterations > 0, "bad sizes");                                                \
    return dr::launch("pair_update_kernel", dr::pair_update_kernel<T, dr::RigidGeom>, dim3(P), dr::kPairThreads, stream, matches,   \
                      models, valid, scores, thr2, M, N, B, confidence, eps, max_iterations, best_score, best_model, best_mask,     \
                      best_inliers, iters, max_iters);                                                                              \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_OP(sfx, T)                                                                                                              \
  int dr_refit_rigid_##sfx(const T *matches, const uint8_t *mask, const T *weights, int P, int N, T *model, uint8_t *valid,         \
                           void *stream) {                                                                                          \
    DR_REQUIRE(matches && model && valid, "null pointer");                                                                          \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");                                                                                        \
    return dr::launch("refit_rigid_kernel", dr::refit_rigid_kernel<T>, dim3(P), dr::kRFThreads, stream, matches, mask, weights, N,  \
                      model, valid);                                                                                                \
  }                                                                                                                                 \
  int dr_refit_rigid_bwd_##sfx(const T *matches, const uint8_t *mask, const T *weights, const T *grad_model, int P, int N,          \
                               T *grad_matches, T *grad_weights, void *stream) {                                                    \
    DR_REQUIRE(matches && grad_model && (grad_matches || grad_weights), "null pointer");                                            \
    DR_REQUIRE(P > 0 && N > 0 && (long)N * 6 < (1l << 31), "bad sizes");                                                            \
    return dr::launch("refit_rigid_bwd_kernel", dr::refit_rigid_bwd_kernel<T>, dim3(P), dr::kRFThreads, stream, matches, mask,      \
                      weights, grad_model, N, grad_matches, grad_weights);                                                          \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

#define DR_OP(sfx, T)                                                                                                              \
  int dr_registration_local_opt_##sfx(const T *matches, const T *thr2, int P, int N, int lo, int lo_iters, double confidence,       \
                                      double eps, int max_iterations, T *best_score, T *best_model, uint8_t *best_mask,             \
                                      int32_t *best_inliers, double *max_iters, T *lo_seen, int32_t *lo_refits, void *stream) {     \
    DR_REQUIRE(matches && thr2 && best_score && best_model && best_mask && best_inliers && max_iters && lo_seen, "null pointer");   \
    DR_REQUIRE(P > 0 && N > 0 && max_iterations > 0, "bad sizes");                                                                  \
    DR_REQUIRE(lo == 1 || lo == 2, "lo must be 1 (one refit) or 2 (iterated refits)");                                              \
    DR_REQUIRE(lo_iters >= 1, "lo_iters must be at least 1");                                                                       \
    return dr::launch("registration_local_opt_kernel", dr::registration_local_opt_kernel<T>, dim3(P), dr::kRFThreads, stream,       \
                      matches, thr2, N, lo == 1 ? 1 : lo_iters, confidence, eps, max_iterations, best_score, best_model, best_mask, \
                      best_inliers, max_iters, lo_seen, lo_refits);                                                                 \
  }                                                                                                                                 \
  int dr_registration_irls_##sfx(const T *matches, const T *thr2, int P, int N, int irls_iters, T *best_score, T *best_model,       \
                                 int32_t *irls_fits, void *stream) {                                                                \
    DR_REQUIRE(matches && thr2 && best_score && best_model && irls_fits, "null pointer");                                           \
    DR_REQUIRE(P > 0 && N > 0, "bad sizes");                                                                                        \
    DR_REQUIRE(irls_iters >= 1, "irls_iters must be at least 1");                                                                   \
    return dr::launch("registration_irls_kernel", dr::registration_irls_kernel<T>, dim3(P), dr::kRFThreads, stream, matches, thr2,  \
                      N, irls_iters, best_score, best_model, irls_fits);                                                            \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
