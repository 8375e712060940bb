// Absolute pose from 2D-3D matches (ransac.BatchedPnP): up to four poses from every minimal sample of three matches by a closed-form
// P3P, the MSAC score and inlier count of every pose against every point under the reprojection error, the per-pair state step with
// the adaptive stop, and the Levenberg-Marquardt refit over the rows a mask selects.  Conventions, residual and slot rules:
// pnp_device.hpp.  The threshold is a DISTANCE in normalised units and enters as thr2 = threshold^2 per pair: inlier <=> d2 < thr2;
// MSAC score = sum_n max(0, 1 - d2_n / thr2).
#include "pair_state_device.hpp"
#include "pnp_device.hpp"
#include "rigid_device.hpp"
#include "solver_common.hpp"

namespace dr {

// ---- (1) three matches -> up to four poses: Grunert's P3P in the Fischler-Bolles ratio form -----------------------------------------
// Bearings f_i = normalize(u_i, v_i, 1), unknown depths s_i along them (the camera points are Y_i = s_i f_i), world distances
// a = |X_1 - X_2|, b = |X_0 - X_2|, c = |X_0 - X_1| and cosines ca = f_1 . f_2, cb = f_0 . f_2, cg = f_0 . f_1.  The law of cosines in the
// three triangles camera-centre / two points:
//   s_1^2 + s_2^2 - 2 s_1 s_2 ca = a^2      s_0^2 + s_2^2 - 2 s_0 s_2 cb = b^2      s_0^2 + s_1^2 - 2 s_0 s_1 cg = c^2.
// With s_1 = x s_0 and s_2 = v s_0 the middle one gives s_0^2 = b^2 / (1 + v^2 - 2 v cb); dividing the other two by it,
//   x^2 + v^2 - 2 x v ca = (a^2 / b^2) g(v)      1 + x^2 - 2 x cg = (c^2 / b^2) g(v)      g(v) = 1 + v^2 - 2 v cb,
// and their difference is linear in x:  x = p(v) / q(v),  p = (K - 1) v^2 - 2 K cb v + (K + 1),  q = 2 (cg - v ca),  K = (a^2 - c^2) / b^2.
// Put into the second one and multiplied by q^2:  p^2 - 2 cg p q + q^2 (1 - (c^2 / b^2) g(v)) = 0, a quartic in v whose coefficients are
// formed by multiplying the polynomials out.  Its real roots come from solver_common.hpp's real_roots<4>; each one with v > 0 gives
// (s_0, x s_0, v s_0), polished by kP3PNewton Newton steps on the three law-of-cosines equations in (s_0, s_1, s_2) (a fixed number:
// the 64 samples of a wave never wait for one; a step that is not finite is not taken).  A root is kept when the three depths are
// positive and finite.  The pose follows without a decomposition: the orthonormal frames (e_0, e_1, e_0 x e_1) of the world triangle
// and of the camera triangle by Gram-Schmidt on their two edges from point 0, R = sum_k e'_k e_k^T (rotation_from_frames: proper and
// orthonormal by construction, whatever is left of the triangles' incongruence), t = mean Y - R mean X; the slot is valid when every
// entry is finite and R X_i + t has z > 0 for the three points.
// Slots 4 b + j of sample b: the valid ones first, in ascending order of their root v; every other slot is the identity with
// valid = 0.  A sample has four invalid slots when an index is out of range, two world points coincide (a repeated index), the
// world points are collinear or two bearings coincide (sin^2 of the angle below kP3PSin2: 1e-6 rad), or no root survives.
// Mapping: one lane per sample, 64-thread blocks, all f64 in registers for either type, as homography4_gather_kernel.  No atomics, no
// LDS; a repeated launch gives the same bits.
constexpr int kP3PNewton = 2;
constexpr double kP3PSin2 = 1e-12;

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ double cross_norm2(const double (&a)[3], const double (&b)[3]) {
  const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  return c0 * c0 + c1 * c1 + c2 * c2;
}

// e0 = d1 / |d1|, e1 = the part of d2 orthogonal to it, normalised.  The projection is taken out twice: after one pass a thin
// triangle leaves e0 . e1 at eps / sin(angle), after the second it is at eps whatever the angle, so R is orthonormal to rounding.
__device__ __forceinline__ void frame2(const double (&d1)[3], const double (&d2)[3], double (&e0)[3], double (&e1)[3]) {
  const double r1 = 1.0 / sqrt(dot3(d1, d1));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e0[i] = d1[i] * r1;
    e1[i] = d2[i];
  }
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const double h = dot3(e1, e0);
#pragma unroll
    for (int i = 0; i < 3; ++i) e1[i] -= h * e0[i];
  }
  const double r2 = 1.0 / sqrt(dot3(e1, e1));
#pragma unroll
  for (int i = 0; i < 3; ++i) e1[i] *= r2;
}

struct P3PSample {
  double X[3][3], f[3][3];      // world points, unit bearings
  double a2, b2, c2, ca, cb, cg;
  double e0[3], e1[3], xm[3];   // the world triangle's frame and centroid
};

// one root v of the quartic -> the pose (R, t); false: the slot is dropped
__device__ __forceinline__ bool p3p_pose(const P3PSample &S, double v, double (&R)[3][3], double (&t)[3]) {
  const double K = (S.a2 - S.c2) / S.b2;
  const double x = ((K - 1.0) * v * v - 2.0 * K * S.cb * v + (K + 1.0)) / (2.0 * (S.cg - v * S.ca));
  double s[3];
  s[0] = sqrt(S.b2 / (1.0 + v * v - 2.0 * v * S.cb));
  s[1] = x * s[0];
  s[2] = v * s[0];
#pragma unroll
  for (int it = 0; it < kP3PNewton; ++it) {
    const double F0 = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * S.ca - S.a2;
    const double F1 = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * S.cb - S.b2;
    const double F2 = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * S.cg - S.c2;
    // J = [[0, j01, j02], [j10, 0, j12], [j20, j21, 0]]; det J = j01 j12 j20 + j02 j10 j21, the step by Cramer's rule
    const double j01 = 2.0 * (s[1] - s[2] * S.ca), j02 = 2.0 * (s[2] - s[1] * S.ca);
    const double j10 = 2.0 * (s[0] - s[2] * S.cb), j12 = 2.0 * (s[2] - s[0] * S.cb);
    const double j20 = 2.0 * (s[0] - s[1] * S.cg), j21 = 2.0 * (s[1] - s[0] * S.cg);
    const double rd = 1.0 / (j01 * j12 * j20 + j02 * j10 * j21);
    const double d0 = (-j12 * j21 * F0 + j02 * j21 * F1 + j01 * j12 * F2) * rd;
    const double d1 = (j12 * j20 * F0 - j02 * j20 * F1 + j02 * j10 * F2) * rd;
    const double d2 = (j10 * j21 * F0 + j01 * j20 * F1 - j01 * j10 * F2) * rd;
    const bool take = is_finite(d0) && is_finite(d1) && is_finite(d2);
    s[0] = take ? s[0] - d0 : s[0];
    s[1] = take ? s[1] - d1 : s[1];
    s[2] = take ? s[2] - d2 : s[2];
  }
  bool ok = v > 0.0;
  double Y[3][3], ym[3], g1[3], g2[3], c0[3], c1[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ok = ok && s[i] > 0.0 && is_finite(s[i]);
#pragma unroll
    for (int d = 0; d < 3; ++d) Y[i][d] = s[i] * S.f[i][d];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    ym[d] = (Y[0][d] + Y[1][d] + Y[2][d]) * (1.0 / 3.0);
    g1[d] = Y[1][d] - Y[0][d];
    g2[d] = Y[2][d] - Y[0][d];
  }
  frame2(g1, g2, c0, c1);
  ok = rotation_from_frames(c0, c1, S.e0, S.e1, R) && ok;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = ym[i] - (R[i][0] * S.xm[0] + R[i][1] * S.xm[1] + R[i][2] * S.xm[2]);
    ok = ok && is_finite(t[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) ok = ok && (R[2][0] * S.X[i][0] + R[2][1] * S.X[i][1] + R[2][2] * S.X[i][2] + t[2]) > 0.0;
  return ok;
}

__device__ __forceinline__ void sort_step(double &a, double &b) {
  const double lo = fmin(a, b), hi = fmax(a, b);
  a = lo;
  b = hi;
}

// The whole closed form of one sample, shared by the gather kernel, the kernel on explicit samples and the reverse pass: the three rows
// come through row(r) (a pointer to the five values of row r), and slot(j, R, t, S) is called once for every valid pose, in slot
// order j = 0, 1, ... (ascending root).  Returns the number of valid slots.  One text, so the three kernels compute the same poses in
// the same order; the slot loop stays rolled (#pragma unroll 1: four copies of p3p_pose would not fit the register file).
template <typename T, typename RowFn, typename SlotFn>
__device__ __forceinline__ int p3p_fwd(RowFn row, bool usable, SlotFn slot) {
  P3PSample S;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const T *p = row(r);
#pragma unroll
    for (int d = 0; d < 3; ++d) S.X[r][d] = (double)p[d];
    const double u = (double)p[3], w = (double)p[4], rn = 1.0 / sqrt(u * u + w * w + 1.0);
    S.f[r][0] = u * rn;
    S.f[r][1] = w * rn;
    S.f[r][2] = rn;
  }
  double d01[3], d02[3], d12[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    d01[d] = S.X[1][d] - S.X[0][d];
    d02[d] = S.X[2][d] - S.X[0][d];
    d12[d] = S.X[2][d] - S.X[1][d];
    S.xm[d] = (S.X[0][d] + S.X[1][d] + S.X[2][d]) * (1.0 / 3.0);
  }
  S.a2 = dot3(d12, d12);
  S.b2 = dot3(d02, d02);
  S.c2 = dot3(d01, d01);
  S.ca = dot3(S.f[1], S.f[2]);
  S.cb = dot3(S.f[0], S.f[2]);
  S.cg = dot3(S.f[0], S.f[1]);
  // (every test false for NaN)
  usable = usable && S.a2 > 0.0 && S.b2 > 0.0 && S.c2 > 0.0 && cross_norm2(d01, d02) > kP3PSin2 * S.b2 * S.c2;
  usable = usable && cross_norm2(S.f[1], S.f[2]) > kP3PSin2 && cross_norm2(S.f[0], S.f[2]) > kP3PSin2 &&
           cross_norm2(S.f[0], S.f[1]) > kP3PSin2;
  frame2(d01, d02, S.e0, S.e1);
  // the quartic, ascending
  const double K = (S.a2 - S.c2) / S.b2, Cb = S.c2 / S.b2;
  const double p0 = K + 1.0, p1 = -2.0 * K * S.cb, p2 = K - 1.0, q0 = 2.0 * S.cg, q1 = -2.0 * S.ca;
  const double w0 = 1.0 - Cb, w1 = 2.0 * Cb * S.cb, w2 = -Cb;
  const double qq0 = q0 * q0, qq1 = 2.0 * q0 * q1, qq2 = q1 * q1, m2 = -2.0 * S.cg;
  double c[5];
  c[0] = p0 * p0 + m2 * (p0 * q0) + qq0 * w0;
  c[1] = 2.0 * p0 * p1 + m2 * (p0 * q1 + p1 * q0) + qq0 * w1 + qq1 * w0;
  c[2] = 2.0 * p0 * p2 + p1 * p1 + m2 * (p1 * q1 + p2 * q0) + qq0 * w2 + qq1 * w1 + qq2 * w0;
  c[3] = 2.0 * p1 * p2 + m2 * (p2 * q1) + qq1 * w2 + qq2 * w1;
  c[4] = p2 * p2 + qq2 * w2;
  double roots[4];
  int count = 0;
  real_roots<4>(c, roots, count);
  if (!usable) count = 0;
  double r0 = count > 0 ? roots[0] : INFINITY, r1 = count > 1 ? roots[1] : INFINITY, r2 = count > 2 ? roots[2] : INFINITY,
         r3 = count > 3 ? roots[3] : INFINITY;
  sort_step(r0, r1);      // ascending, the unused entries (+inf) last
  sort_step(r2, r3);
  sort_step(r0, r2);
  sort_step(r1, r3);
  sort_step(r1, r2);
  int nv = 0;
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const double v = k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3));
    double R[3][3], t[3];
    if (k < count && p3p_pose(S, v, R, t)) {
      slot(nv, R, t, S);
      ++nv;
    }
  }
  return nv;
}

// the valid poses into slots 0 .. nv - 1 of the sample, the identity with valid = 0 into the rest
template <typename T, typename RowFn>
__device__ __forceinline__ void p3p_store(RowFn row, bool usable, T *__restrict__ out, uint8_t *__restrict__ vout) {
  const int nv = p3p_fwd<T>(row, usable, [&](int j, const double (&R)[3][3], const double (&t)[3], const P3PSample &) {
    store_rigid_model(out + j * 16, R, t);
    vout[j] = 1;
  });
  double R[3][3], t[3];
  set_identity(R, t);
  for (int j = nv; j < 4; ++j) {
    store_rigid_model(out + j * 16, R, t);
    vout[j] = 0;
  }
}

// rows read through the index sets: one lane = one sample (a bad index reads row 0, every slot invalid)
template <typename T>
__global__ __launch_bounds__(64) void p3p_gather_kernel(const T *__restrict__ matches, const int32_t *__restrict__ idx, int Bt, int B,
                                                        int N, T *__restrict__ models, uint8_t *__restrict__ valid) {
  const int smp = blockIdx.x * 64 + threadIdx.x;
  if (smp >= Bt) return;
  const T *base = matches + (size_t)(smp / B) * N * 5;
  const int32_t *gi = idx + (size_t)smp * 3;
  bool usable = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) usable = usable && gi[r] >= 0 && gi[r] < N;
  p3p_store<T>([&](int r) { return base + (size_t)(usable ? gi[r] : 0) * 5; }, usable, models + (size_t)smp * 64,
               valid + (size_t)smp * 4);
}

// explicit sample tensors [Bt,3,5]: what train mode fits.  On samples = matches[idx] the bits of the gather kernel.
template <typename T>
__global__ __launch_bounds__(64) void p3p_kernel(const T *__restrict__ samples, int Bt, T *__restrict__ models,
                                                 uint8_t *__restrict__ valid) {
  const int smp = blockIdx.x * 64 + threadIdx.x;
  if (smp >= Bt) return;
  const T *base = samples + (size_t)smp * 15;
  p3p_store<T>([&](int r) { return base + r * 5; }, true, models + (size_t)smp * 64, valid + (size_t)smp * 4);
}

// ---- (1b) the reverse pass of (1): grad_models [4 Bt,4,4] -> grad_samples [Bt,3,5] ---------------------------------------------------
// A valid pose (R, t) of a sample is a root of the six equations r(theta; sample) = 0, r_i = (x_c / z_c - u_i, y_c / z_c - v_i) at
// x_c = R X_i + t for the three rows: its derivative follows from the implicit function theorem, whatever route the forward took to the
// root (quartic, Newton polish, frames).  theta is dr_refit_pnp's LEFT-multiplied step (w, d): R' = exp([w]x) R, t' = exp([w]x) t + d.
//   1. the incoming G = grad_models of the slot (rows 0-2 read, row 3 ignored) as a tangent gradient:
//        g_theta = (sum_j R[:,j] x G_R[:,j] + t x G_t,  G_t).
//      Only the tangential part of G_R enters: a component normal to the rotation manifold (symmetric G_R R^T) passes nothing on.
//   2. J (6x6) = d r / d theta: per row i the two rows d r_u, d r_v of dr_refit_pnp's header, i.e. A_i [-[x_c]x | I] with
//      A_i = (1 / z_c) [[1, 0, -x], [0, 1, -y]].
//   3. J^T lambda = g_theta by LU with partial pivoting in registers (lu_solve6).
//   4. d r_i / d X_i = A_i R and d r_i / d (u, v)_i = -I, so  grad X_i += -(A_i R)^T lambda_i,  grad (u, v)_i += lambda_i.
// The theorem holds AT the root, and the forward's pose is a few ulp times the sample's conditioning away from it (two Newton steps on
// the depths, then the frames); an ill-conditioned sample turns that distance into a gradient error hundreds of times as large.  So
// before step 1 the slot's pose takes ONE Gauss-Newton step on r = 0 in the same parametrisation, J delta = -r by the same LU,
// (R, t) <- (exp([w]x) R, exp([w]x) t + d) (lm_step): the six equations have six unknowns, the step converges quadratically and one of
// them leaves the pose at the rounding of r, which is evaluated as a two-term sum (dd_row, dd_residual) so that it is the rounding of
// the pose's own entries and not eps times the conditioning.  The step is not taken when a pivot fails the guard below or delta is not finite.  The
// models the forward returned are not touched: the polish moves only the point at which the derivative is evaluated.
// The lane recomputes the sample's poses with p3p_fwd -- the slot order is the forward's by construction, no model is saved -- and adds
// the contributions of the valid slots in slot order.  A slot contributes exact zeros when it is invalid (its gradient is never read:
// NaN there reaches nothing), when a pivot of the elimination is not larger than kP3PPivot times the largest |entry| of J (a pose at
// a double root of the quartic: J is singular there and the derivative does not exist; false for NaN too), or when any of its fifteen
// results is not finite.  Every output element is written; a sample with no contributing slot gets fifteen exact zeros.
// Mapping: the forward's -- one lane per sample, 64-thread blocks, f64 in registers for either type; no atomics, no LDS: a repeated
// launch repeats bit for bit.
constexpr double kP3PPivot = 1e-12;

// A x = b in place (b becomes x) by LU with partial pivoting, fully unrolled: the row exchange is a compare-and-select sweep that
// leaves the column's largest entry in row k, so nothing is indexed at run time and the matrix stays in registers.
// false: a pivot with |pivot| <= tiny (or NaN).
__device__ __forceinline__ bool lu_solve6(double (&A)[6][6], double (&b)[6], double tiny) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const bool sw = fabs(A[r][k]) > fabs(A[k][k]);
#pragma unroll
      for (int c = k; c < 6; ++c) {
        const double hi = A[k][c], lo = A[r][c];
        A[k][c] = sw ? lo : hi;
        A[r][c] = sw ? hi : lo;
      }
      const double hi = b[k], lo = b[r];
      b[k] = sw ? lo : hi;
      b[r] = sw ? hi : lo;
    }
    ok = ok && fabs(A[k][k]) > tiny;
    const double rp = 1.0 / A[k][k];
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
      const double f = A[r][k] * rp;
#pragma unroll
      for (int c = k + 1; c < 6; ++c) A[r][c] -= f * A[k][c];
      b[r] -= f * b[k];
    }
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    double v = b[k];
#pragma unroll
    for (int c = k + 1; c < 6; ++c) v -= A[k][c] * b[c];
    b[k] = v / A[k][k];
  }
  return ok;
}

// the two rows of J = d r / d (w, d) of one sample row at x_c = R X + t (dr_refit_pnp's header), and 1 / z_c, x, y
__device__ __forceinline__ void p3p_jac_rows(const double (&R)[3][3], const double (&t)[3], const double (&X)[3], double (&ju)[6],
                                             double (&jv)[6], double &iz, double &x, double &y) {
  double xc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) xc[r] = R[r][0] * X[0] + R[r][1] * X[1] + R[r][2] * X[2] + t[r];
  iz = 1.0 / xc[2];
  x = xc[0] * iz;
  y = xc[1] * iz;
  ju[0] = -x * y, ju[1] = 1.0 + x * x, ju[2] = -y, ju[3] = iz, ju[4] = 0.0, ju[5] = -x * iz;
  jv[0] = -1.0 - y * y, jv[1] = x * y, jv[2] = x, jv[3] = 0.0, jv[4] = iz, jv[5] = -y * iz;
}

__device__ __forceinline__ void lm_step(const double (&R)[3][3], const double (&t)[3], const double (&s)[6], double (&Rn)[3][3],
                                        double (&tn)[3]);      // (section 4)

// r . X + t as an unevaluated sum hi + lo (exact products by fma, Knuth's two-sum): the residual of the polish cancels from |x_c| to
// 1e-15 and an f64 evaluation would leave the step at eps times the sample's conditioning.  No contraction here: the error terms
// are differences of the very products and sums a contraction would fuse.
__device__ __forceinline__ void dd_row(const double (&r)[3], double t, const double (&X)[3], double &hi, double &lo) {
#pragma clang fp contract(off)
  hi = t;
  lo = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double p = r[j] * X[j], pe = fma(r[j], X[j], -p);
    const double s = hi + p, bb = s - hi;
    lo += ((hi - (s - bb)) + (p - bb)) + pe;
    hi = s;
  }
}

// (x_c - u z_c) / z_c of one coordinate from the two-term forms of x_c and z_c: the subtraction is exact where it cancels
__device__ __forceinline__ double dd_residual(double xh, double xl, double zh, double zl, double u) {
#pragma clang fp contract(off)
  const double q = u * zh, qe = fma(u, zh, -q);
  return ((xh - q) + ((xl - qe) - u * zl)) / zh;
}

template <typename T>
__global__ __launch_bounds__(64) void p3p_bwd_kernel(const T *__restrict__ samples, const T *__restrict__ grad_models, int Bt,
                                                     T *__restrict__ grad_samples) {
  const int smp = blockIdx.x * 64 + threadIdx.x;
  if (smp >= Bt) return;
  const T *base = samples + (size_t)smp * 15;
  double acc[15];
#pragma unroll
  for (int q = 0; q < 15; ++q) acc[q] = 0.0;
  p3p_fwd<T>([&](int r) { return base + r * 5; }, true, [&](int j, const double (&R0)[3][3], const double (&t0)[3], const P3PSample &S) {
    // one Gauss-Newton step onto the root of the sample's six reprojection equations
    double R[3][3], t[3];
    {
      double J[6][6], d[6], big = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double iz, x, y;
        p3p_jac_rows(R0, t0, S.X[i], J[2 * i], J[2 * i + 1], iz, x, y);
        double xh, xl, yh, yl, zh, zl;
        dd_row(R0[0], t0[0], S.X[i], xh, xl);
        dd_row(R0[1], t0[1], S.X[i], yh, yl);
        dd_row(R0[2], t0[2], S.X[i], zh, zl);
        d[2 * i] = -dd_residual(xh, xl, zh, zl, (double)base[5 * i + 3]);
        d[2 * i + 1] = -dd_residual(yh, yl, zh, zl, (double)base[5 * i + 4]);
#pragma unroll
        for (int a = 0; a < 6; ++a) big = fmax(big, fmax(fabs(J[2 * i][a]), fabs(J[2 * i + 1][a])));
      }
      bool step = lu_solve6(J, d, kP3PPivot * big);
#pragma unroll
      for (int a = 0; a < 6; ++a) step = step && is_finite(d[a]);
      if (!step) {
#pragma unroll
        for (int a = 0; a < 6; ++a) d[a] = 0.0;      // (the identity step: the forward's pose)
      }
      lm_step(R0, t0, d, R, t);
    }
    const T *G = grad_models + ((size_t)smp * 4 + j) * 16;
    double gR[3][3], g[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) gR[i][c] = (double)G[4 * i + c];
      g[3 + i] = (double)G[4 * i + 3];
    }
    // sum_j R[:,j] x G_R[:,j] + t x G_t
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int a = (i + 1) % 3, b = (i + 2) % 3;
      double v = t[a] * g[3 + b] - t[b] * g[3 + a];
#pragma unroll
      for (int c = 0; c < 3; ++c) v += R[a][c] * gR[b][c] - R[b][c] * gR[a][c];
      g[i] = v;
    }
    // J^T, column 2 i and 2 i + 1 from row i; the largest |entry|
    double Jt[6][6], iz[3], x[3], y[3], big = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double ju[6], jv[6];
      p3p_jac_rows(R, t, S.X[i], ju, jv, iz[i], x[i], y[i]);
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        Jt[a][2 * i] = ju[a];
        Jt[a][2 * i + 1] = jv[a];
        big = fmax(big, fmax(fabs(ju[a]), fabs(jv[a])));
      }
    }
    bool ok = lu_solve6(Jt, g, kP3PPivot * big);      // g is lambda from here
    double out[15];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int c = 0; c < 3; ++c)      // -(A_i R)^T lambda_i, A_i R = (1 / z_c) (R_0 - x R_2, R_1 - y R_2)
        out[5 * i + c] = -iz[i] * ((R[0][c] - x[i] * R[2][c]) * g[2 * i] + (R[1][c] - y[i] * R[2][c]) * g[2 * i + 1]);
      out[5 * i + 3] = g[2 * i];
      out[5 * i + 4] = g[2 * i + 1];
    }
#pragma unroll
    for (int q = 0; q < 15; ++q) ok = ok && is_finite(out[q]);
#pragma unroll
    for (int q = 0; q < 15; ++q) acc[q] += ok ? out[q] : 0.0;
  });
#pragma unroll
  for (int q = 0; q < 15; ++q) grad_samples[(size_t)smp * 15 + q] = (T)acc[q];
}

// ---- (2), (3) the score of every pose against every point and the state step are pair_state_device.hpp's pair_score_kernel and
// pair_update_kernel under PnPGeom and TransferMsacTerm (dr_pnp_score, dr_pnp_update); M = 4 B slots per round, iters += B

// ---- (4) Levenberg-Marquardt on the reprojection error over the rows a mask selects (dr_refit_pnp) ----------------------------------
// From init_model, `iters` passes at most.  A pass at the iterate (R, t): the row set is the mask's rows with z_c > 0 and a finite
// residual under (R, t); over it the 21 + 6 + 1 sums upper(J^T J), J^T r, cost = sum |r|^2 (only when the iterate has moved since they
// were last taken), with r = (x_c / z_c - u, y_c / z_c - v) and J its derivative with respect to a LEFT-multiplied step
// (w, d): x_c' = exp([w]x) x_c + d, so per row, with i = 1 / z_c, x = x_c i, y = y_c i,
//   d r_u = (-x y, 1 + x^2, -y, i, 0, -x i),   d r_v = (-1 - y^2, x y, x, 0, i, -y i).
// Every thread solves (J^T J + lambda diag(J^T J)) step = -J^T r by Cholesky on the block's sums (they are the same bits in every
// thread: nothing is broadcast), forms the candidate R' = exp([w]x) R, t' = exp([w]x) t + d (Rodrigues; the series below 1e-4 rad),
// and the block sums the candidate's cost over the SAME row set.  The step is taken on a strictly lower cost with every row of the
// set still in front of the camera and finite: lambda /= 10 (not below 1e-12); otherwise, and when the damped matrix is not positive
// definite, lambda *= 10 and the iterate stays.  lambda starts at 1e-3.
// valid = 0 (identity) for a non-finite start, fewer than three rows in front of the camera under the start, or a non-finite result.
// Mapping: a latency kernel like registration_local_opt_kernel -- one 256-thread block per pair, f64, thread n owns rows n, n + 256,
// ...; the passes of a pair are serial, each one two block-stride sweeps over the pair's 5 N values and N mask bytes.  The rows are
// not staged in LDS: a sweep reads each row once, so LDS would only add a copy, and between sweeps the 20 N (40 N) bytes of a pair stay in
// L2 (a few hundred KB at most for the row counts the drivers use); 64 KB of LDS would hold 1600 f64 rows, fewer than a pair may have.
// Sums go lane, wave butterfly, the four waves in order (block_sum_f64); every branch that holds a barrier is block-uniform, no
// atomics: a repeated launch gives the same bits.
constexpr int kPRThreads = kPairThreads;

// x_c = R X + t of a row -> is it in front of the camera with a finite residual; r = the residual
__device__ __forceinline__ bool pnp_row(const double (&R)[3][3], const double (&t)[3], const double (&m)[5], double (&xc)[3],
                                        double (&r)[2]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) xc[i] = R[i][0] * m[0] + R[i][1] * m[1] + R[i][2] * m[2] + t[i];
  const double iz = 1.0 / xc[2];
  r[0] = xc[0] * iz - m[3];
  r[1] = xc[1] * iz - m[4];
  return xc[2] > 0.0 && is_finite(r[0]) && is_finite(r[1]);
}

// (A + lambda diag A) s = -g for the upper triangle a[0..20] (row-major, i <= j) and g = a[21..26] -> is the matrix positive definite
__device__ __forceinline__ bool lm_solve6(const double (&a)[28], double lambda, double (&s)[6]) {
  double L[6][6];
  {
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) L[j][i] = a[q++] * (i == j ? 1.0 + lambda : 1.0);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && d > 0.0 && is_finite(d);
    const double ld = sqrt(d), rl = 1.0 / ld;
    L[j][j] = ld;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v * rl;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = -a[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * s[k];
    s[i] = v / L[i][i];
    ok = ok && is_finite(s[i]);
  }
  return ok;
}

// (R', t') = (exp([w]x) R, exp([w]x) t + d), step = (w, d)
__device__ __forceinline__ void lm_step(const double (&R)[3][3], const double (&t)[3], const double (&s)[6], double (&Rn)[3][3],
                                        double (&tn)[3]) {
  const double th2 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2], th = sqrt(th2);
  const bool small = th < 1e-4;
  const double A = small ? 1.0 - th2 * (1.0 / 6.0) : sin(th) / th;
  const double Bc = small ? 0.5 - th2 * (1.0 / 24.0) : (1.0 - cos(th)) / th2;
  double E[3][3];
  const double w[3] = {s[0], s[1], s[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E[i][j] = Bc * w[i] * w[j] + (i == j ? 1.0 - Bc * th2 : 0.0);      // I + B [w]x^2 = (1 - B th^2) I + B w w^T
  E[0][1] -= A * w[2];
  E[0][2] += A * w[1];
  E[1][0] += A * w[2];
  E[1][2] -= A * w[0];
  E[2][0] -= A * w[1];
  E[2][1] += A * w[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[i][j] = E[i][0] * R[0][j] + E[i][1] * R[1][j] + E[i][2] * R[2][j];
    tn[i] = E[i][0] * t[0] + E[i][1] * t[1] + E[i][2] * t[2] + s[3 + i];
  }
}

// kWeighted (dr_refit_pnp_weighted with a weights pointer): a row's weight w multiplies its terms in J^T J, J^T r and both costs -- the
// minimiser of sum w |r|^2.  The unweighted instantiation's text is the one dr_refit_pnp has always run: nothing of the weight reaches
// it, and -ffp-contract decides how its sums round.  The weighted one must give those bits at w = 1, so it does not leave that to the
// compiler: every sum is written out with fma in the shape the unweighted ones compile to (read from the kernel's assembly and
// pinned by tests/test_gpu_weighted_pnp.py) -- a[q] += fma(one product, the other product rounded), the rounded one being the jv
// product except where ju[2] = -y is a factor (the negation moves the multiplication there); (3,3) and (4,4), whose other product is
// 0 x 0, are one fma into the sum.  This pins the weighted text to what ONE compiler does with the unweighted one: a compiler that
// contracts those sums differently breaks the w = 1 equality without any change here (weights = NULL stays bit-equal: it IS the
// unweighted instantiation), test_weights_of_exactly_one_give_the_bits_of_the_plain_refit is the tripwire, and the repair is to read
// the unweighted kernel's assembly again and restate the shape below.  The weight sits on one factor of each product (w ju, w jv,
// w r).  The row set does not look
// at the weights: a row with w = 0 counts towards the three-row rule and adds exact zeros to every sum (the mask is the selection).
__device__ __forceinline__ double two_products(double ua, double ub, double va, double vb, bool round_u) {
  return round_u ? fma(va, vb, ua * ub) : fma(ua, ub, va * vb);
}

template <typename T, bool kWeighted>
__global__ __launch_bounds__(kPRThreads) void refit_pnp_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                               const T *__restrict__ weights, const T *__restrict__ init_model, int N,
                                                               int iters, T *__restrict__ model, uint8_t *__restrict__ valid) {
  __shared__ double s_red[(kPRThreads / 64) * 28];
  const int p = blockIdx.x, tid = threadIdx.x;
  const T *pt = matches + (size_t)p * N * 5;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T *wt = kWeighted ? weights + (size_t)p * N : nullptr;
  auto scaled = [&](int n, double x) {      // w_n x
    if constexpr (kWeighted) return (double)wt[n] * x;
    else return x;
  };
  double R[3][3], t[3];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R[i][j] = (double)init_model[(size_t)p * 16 + 4 * i + j];
      ok = ok && is_finite(R[i][j]);
    }
    t[i] = (double)init_model[(size_t)p * 16 + 4 * i + 3];
    ok = ok && is_finite(t[i]);
  }
  auto load = [&](int n, double (&m)[5]) {
#pragma unroll
    for (int d = 0; d < 5; ++d) m[d] = (double)pt[(size_t)n * 5 + d];
  };
  double rows[1] = {0.0};
  for (int n = tid; ok && n < N; n += kPRThreads) {
    if (mk && !mk[n]) continue;
    double m[5], xc[3], r[2];
    load(n, m);
    rows[0] += pnp_row(R, t, m, xc, r) ? 1.0 : 0.0;
  }
  block_sum_f64<1>(rows, reinterpret_cast<double(*)[1]>(s_red));
  ok = ok && rows[0] >= 3.0;      // (block-uniform: the start is the same in every thread, the count a block sum)
  double a[28], lambda = 1e-3;
  bool fresh = false;
  for (int it = 0; ok && it < iters; ++it) {
    if (!fresh) {
#pragma unroll
      for (int q = 0; q < 28; ++q) a[q] = 0.0;
      for (int n = tid; n < N; n += kPRThreads) {
        if (mk && !mk[n]) continue;
        double m[5], xc[3], r[2];
        load(n, m);
        if (!pnp_row(R, t, m, xc, r)) continue;
        const double iz = 1.0 / xc[2], x = xc[0] * iz, y = xc[1] * iz;
        const double ju[6] = {-x * y, 1.0 + x * x, -y, iz, 0.0, -x * iz}, jv[6] = {-1.0 - y * y, x * y, x, 0.0, iz, -y * iz};
        const double wr[2] = {scaled(n, r[0]), scaled(n, r[1])};
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          const double wju = scaled(n, ju[i]), wjv = scaled(n, jv[i]);
          if constexpr (kWeighted) {
#pragma unroll
            for (int j = i; j < 6; ++j, ++q) {
              if (i == j && i == 3) a[q] = fma(wju, ju[j], a[q]);
              else if (i == j && i == 4) a[q] = fma(wjv, jv[j], a[q]);
              else a[q] += two_products(wju, ju[j], wjv, jv[j], (i == 2) != (j == 2));
            }
            a[21 + i] += two_products(ju[i], wr[0], jv[i], wr[1], i == 2);
          } else {
#pragma unroll
            for (int j = i; j < 6; ++j) a[q++] += wju * ju[j] + wjv * jv[j];
            a[21 + i] += ju[i] * wr[0] + jv[i] * wr[1];
          }
        }
        if constexpr (kWeighted) a[27] += fma(wr[0], r[0], wr[1] * r[1]);
        else a[27] += wr[0] * r[0] + wr[1] * r[1];
      }
      block_sum_f64<28>(a, reinterpret_cast<double(*)[28]>(s_red));
      fresh = true;
    }
    double step[6], Rc[3][3], tc[3];
    const bool spd = lm_solve6(a, lambda, step);      // (the same in every thread)
    lm_step(R, t, step, Rc, tc);
    double c[2] = {0.0, 0.0};      // the candidate's cost over the iterate's row set; rows it loses
    for (int n = tid; spd && n < N; n += kPRThreads) {
      if (mk && !mk[n]) continue;
      double m[5], xc[3], r[2];
      load(n, m);
      if (!pnp_row(R, t, m, xc, r)) continue;
      if (pnp_row(Rc, tc, m, xc, r)) {
        if constexpr (kWeighted) c[0] += fma(scaled(n, r[0]), r[0], scaled(n, r[1]) * r[1]);
        else c[0] += scaled(n, r[0]) * r[0] + scaled(n, r[1]) * r[1];
      }
      else c[1] += 1.0;
    }
    block_sum_f64<2>(c, reinterpret_cast<double(*)[2]>(s_red));
    if (spd && c[1] == 0.0 && c[0] < a[27]) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = Rc[i][j];
        t[i] = tc[i];
      }
      lambda = fmax(lambda * 0.1, 1e-12);
      fresh = false;
    } else {
      lambda *= 10.0;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) ok = ok && is_finite(R[i][j]);
    ok = ok && is_finite(t[i]);
  }
  if (tid == 0) {
    if (!ok) set_identity(R, t);
    store_rigid_model(model + (size_t)p * 16, R, t);
    valid[p] = ok;
  }
}

// ---- (4b) the reverse pass of the weighted fit (dr_refit_pnp_bwd): grad_model [P,16] -> grad_matches [P,N,5], grad_weights [P,N] -----
// The fit's result is a stationary point of c(theta) = 1/2 sum_i w_i |r_i|^2 over its row set in the chart theta = (w, d) of lm_step:
// g = sum w_i J_i^T r_i = 0, whatever start and damping the forward went through, so its derivative is the implicit function
// theorem's.  Per row at x_c = R X + t, with i = 1 / z_c, (x, y) = (x_c, y_c) i, r = (r_u, r_v), s = r_u x + r_v y:
//   V  = [-[x_c]x | I] (3x6), the derivative of x_c' = exp([w]x) x_c + d at theta = 0;   J = D pi V, D pi = i [[1, 0, -x], [0, 1, -y]];
//   p  = D pi^T r = i (r_u, r_v, -s), the gradient of 1/2 |r|^2 with respect to x_c;
//   B  = D pi^T D pi + r . D^2 pi = i^2 ([[1, 0, -x], [0, 1, -y], [-x, -y, x^2 + y^2]] + [[0, 0, -r_u], [0, 0, -r_v], [-r_u, -r_v, 2 s]]),
//        its Hessian with respect to x_c;
//   H += w (V^T B V + [[sym(p x_c^T), 0], [0, 0]]),   g += w V^T p.
// The last term of H is the second-order part of the chart, p . 1/2 (e_a x (e_b x x_c) + e_b x (e_a x x_c)) = 1/2 (p_a x_b + p_b x_a)
// (p . x_c = 0).  This is the FULL Hessian: with noisy rows the two residual terms are of the size of the gradient they correct.
//   g_theta = (sum_j R[:,j] x G_R[:,j] + t x G_t, G_t) as in dr_p3p_bwd (rows 0-2 of G are read),   H lambda = g_theta by Cholesky,
//   v = lambda_w x x_c + lambda_d,   phi = p . v:   grad w_i = -phi,   grad (u, v)_i = w_i D pi v,
//   grad X_i = -w_i R^T (B v + p x lambda_w)      (the gradient of phi with respect to x_c, r moving with it).
// The forward's model is `iters` passes in the type's rounding away from the root, and the theorem holds AT the root: first
// kBwdNewton Newton steps theta = -H^-1 g with the full H, f64 (each taken only if H is positive definite and the step finite), as
// dr_p3p_bwd polishes its pose.  The model the forward returned is not touched.  The row set is the mask's rows in front of the
// camera with a finite residual under the model the forward returned, and is a constant of the derivative: the polish does not move it.
// Sweeps over the pair's rows: kBwdNewton + 1 reductions of the 21 + 6 sums (plus the row count), one that computes every row's
// gradient to see that all are finite, one that writes each of them once.
// Zeros: a row the mask drops is never read; a row outside the row set; every row of a pair with fewer than three rows in the set, a
// non-finite model, an H that is not positive definite at the polished pose, any non-finite result, or a row of the set that any of
// the polished poses puts behind the camera (or at a non-finite residual): the steps are assumed small, and a pair for which they
// are not has no derivative to give.
// Mapping: refit_pnp_kernel's.  No atomics, fixed summation order: a repeated launch gives the same bits.
constexpr int kBwdNewton = 2;

struct PnPRowTerms {
  double iz, x, y, p[3], B[6];      // B: upper triangle (00, 01, 02, 11, 12, 22)
};

__device__ __forceinline__ void pnp_row_terms(const double (&xc)[3], const double (&r)[2], PnPRowTerms &q) {
  q.iz = 1.0 / xc[2];
  q.x = xc[0] * q.iz;
  q.y = xc[1] * q.iz;
  const double s = r[0] * q.x + r[1] * q.y, i2 = q.iz * q.iz;
  q.p[0] = q.iz * r[0];
  q.p[1] = q.iz * r[1];
  q.p[2] = -q.iz * s;
  q.B[0] = i2;
  q.B[1] = 0.0;
  q.B[2] = -i2 * (q.x + r[0]);
  q.B[3] = i2;
  q.B[4] = -i2 * (q.y + r[1]);
  q.B[5] = i2 * (q.x * q.x + q.y * q.y + 2.0 * s);
}

__device__ __forceinline__ void sym3_mul(const double (&B)[6], const double (&v)[3], double (&o)[3]) {
  o[0] = B[0] * v[0] + B[1] * v[1] + B[2] * v[2];
  o[1] = B[1] * v[0] + B[3] * v[1] + B[4] * v[2];
  o[2] = B[2] * v[0] + B[4] * v[1] + B[5] * v[2];
}

template <typename T>
__global__ __launch_bounds__(kPRThreads) void refit_pnp_bwd_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                   const T *__restrict__ weights, const T *__restrict__ model,
                                                                   const T *__restrict__ grad_model, int N,
                                                                   T *__restrict__ grad_matches, T *__restrict__ grad_weights) {
  __shared__ double s_red[(kPRThreads / 64) * 28];
  const int p = blockIdx.x, tid = threadIdx.x;
  const T *pt = matches + (size_t)p * N * 5;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T *wt = weights ? weights + (size_t)p * N : nullptr;
  double R0[3][3], t0[3], R[3][3], t[3], G[3][4];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R[i][j] = R0[i][j] = (double)model[(size_t)p * 16 + 4 * i + j];
      ok = ok && is_finite(R0[i][j]);
    }
    t[i] = t0[i] = (double)model[(size_t)p * 16 + 4 * i + 3];
    ok = ok && is_finite(t0[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) G[i][j] = (double)grad_model[(size_t)p * 16 + 4 * i + j];
  }
  double lost = 0.0;
  // row n of the set -> m, x_c and r at the current pose (R, t); false: not in the set
  auto row = [&](int n, double (&m)[5], double (&xc)[3], double (&r)[2]) {
    if (mk && !mk[n]) return false;
#pragma unroll
    for (int d = 0; d < 5; ++d) m[d] = (double)pt[(size_t)n * 5 + d];
    if (!pnp_row(R0, t0, m, xc, r)) return false;
    if (!pnp_row(R, t, m, xc, r)) lost += 1.0;      // (the polish took it out of the front: the pair passes nothing on, below)
    return true;
  };
  double a[28], lam[6];
  bool spd = false;
#pragma unroll 1
  for (int pass = 0; pass <= kBwdNewton; ++pass) {
#pragma unroll
    for (int q = 0; q < 28; ++q) a[q] = 0.0;
    for (int n = tid; ok && n < N; n += kPRThreads) {
      double m[5], xc[3], r[2];
      if (!row(n, m, xc, r)) continue;
      const double w = wt ? (double)wt[n] : 1.0;
      PnPRowTerms q;
      pnp_row_terms(xc, r, q);
      const double V[3][6] = {{0.0, xc[2], -xc[1], 1.0, 0.0, 0.0}, {-xc[2], 0.0, xc[0], 0.0, 1.0, 0.0}, {xc[1], -xc[0], 0.0, 0.0, 0.0, 1.0}};
      double BV[3][6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double col[3] = {V[0][c], V[1][c], V[2][c]};
        double o[3];
        sym3_mul(q.B, col, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) BV[k][c] = w * o[k];
      }
      int e = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) {
          double h = V[0][i] * BV[0][j] + V[1][i] * BV[1][j] + V[2][i] * BV[2][j];
          if (j < 3) h += w * 0.5 * (q.p[i] * xc[j] + q.p[j] * xc[i]);
          a[e++] += h;
        }
        a[21 + i] += w * (V[0][i] * q.p[0] + V[1][i] * q.p[1] + V[2][i] * q.p[2]);
      }
      a[27] += 1.0;
    }
    block_sum_f64<28>(a, reinterpret_cast<double(*)[28]>(s_red));
    if (pass < kBwdNewton) {
      double step[6], Rn[3][3], tn[3];
      bool take = lm_solve6(a, 0.0, step);      // step = -H^-1 g
      lm_step(R, t, step, Rn, tn);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) take = take && is_finite(Rn[i][j]);
        take = take && is_finite(tn[i]);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = take ? Rn[i][j] : R[i][j];
        t[i] = take ? tn[i] : t[i];
      }
    } else {
      // -g_theta in g's place: lm_solve6 returns H^-1 g_theta
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int b = (i + 1) % 3, c = (i + 2) % 3;
        double v = t[b] * G[c][3] - t[c] * G[b][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) v += R[b][j] * G[c][j] - R[c][j] * G[b][j];
        a[21 + i] = -v;
        a[24 + i] = -G[i][3];
      }
      spd = lm_solve6(a, 0.0, lam);
    }
  }
  ok = ok && a[27] >= 3.0 && spd;      // (block-uniform: block sums and the model)
  // one row's results: grad X (3), grad (u, v) (2), grad w
  auto grads = [&](int n, double (&o)[6]) {
    double m[5], xc[3], r[2];
#pragma unroll
    for (int d = 0; d < 6; ++d) o[d] = 0.0;
    if (!row(n, m, xc, r)) return;
    const double w = wt ? (double)wt[n] : 1.0;
    PnPRowTerms q;
    pnp_row_terms(xc, r, q);
    const double v[3] = {lam[1] * xc[2] - lam[2] * xc[1] + lam[3], lam[2] * xc[0] - lam[0] * xc[2] + lam[4],
                         lam[0] * xc[1] - lam[1] * xc[0] + lam[5]};
    double gx[3];
    sym3_mul(q.B, v, gx);
    gx[0] += q.p[1] * lam[2] - q.p[2] * lam[1];
    gx[1] += q.p[2] * lam[0] - q.p[0] * lam[2];
    gx[2] += q.p[0] * lam[1] - q.p[1] * lam[0];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = -w * (R[0][c] * gx[0] + R[1][c] * gx[1] + R[2][c] * gx[2]);
    o[3] = w * q.iz * (v[0] - q.x * v[2]);
    o[4] = w * q.iz * (v[1] - q.y * v[2]);
    o[5] = -(q.p[0] * v[0] + q.p[1] * v[1] + q.p[2] * v[2]);
  };
  double bad[1] = {0.0};
  for (int n = tid; ok && n < N; n += kPRThreads) {
    double o[6];
    grads(n, o);
    bool fin = true;
#pragma unroll
    for (int d = 0; d < 6; ++d) fin = fin && is_finite(o[d]);
    bad[0] += fin ? 0.0 : 1.0;
  }
  bad[0] += lost;
  block_sum_f64<1>(bad, reinterpret_cast<double(*)[1]>(s_red));
  ok = ok && bad[0] == 0.0;
  for (int n = tid; n < N; n += kPRThreads) {
    double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) grads(n, o);
    if (grad_matches) {
#pragma unroll
      for (int d = 0; d < 5; ++d) grad_matches[((size_t)p * N + n) * 5 + d] = (T)o[d];
    }
    if (grad_weights) grad_weights[(size_t)p * N + n] = (T)o[5];
  }
}

// ---- (5) the weighted normalised DLT: a pose from six or more rows without a start (dr_pnp_dlt) --------------------------------------
// Hartley normalisation of the WORLD points (the observations are normalised image coordinates already): c = the weighted centroid,
// s = sqrt(3) / the weighted mean distance from it, Xn = (s (X - c), 1).  A row gives the two equations [Xn^T, 0, -u Xn^T] and
// [0, Xn^T, -v Xn^T] on the twelve entries of [M | m] (row-major, x ~ M X + m), and the Gram matrix of all of them under the weights is
//   [[Q1, 0, -Qu], [0, Q1, -Qv], [-Qu, -Qv, Qq]],   Q1 = sum w Xn Xn^T, Qu = sum w u Xn Xn^T, Qv = sum w v Xn Xn^T,
//   Qq = sum w (u^2 + v^2) Xn Xn^T:
// its 78 upper-triangle entries are 40 distinct block sums (four symmetric 4x4), taken through block_sum_f64.  Wave 0 takes all
// eigenpairs with jacobi_eig12_wave; the eigenvector of the smallest eigenvalue, the normalisation undone, is [M | m] up to scale and
// sign.  The sign makes the weighted majority of the rows lie in front of the camera (sum w sign(z) >= 0 of z = the third row on Xn:
// one more block sum), R = the rotation nearest to M (nearest_rotation3) and t = m / M's mean singular value.
// valid = 0 (identity): fewer than six rows under the mask (as in the refit, a row of weight 0 counts: the mask selects), a non-finite
// sum, no positive weight or spread, a non-finite or non-positive scale, a non-finite result, or a smallest eigenvalue that is not
// simple: lambda_1 - lambda_0 <= kDltGap lambda_max.  A coplanar world set has a four-dimensional null space (lambda_0 .. lambda_3 at
// rounding level, 1e-16 lambda_max in f64 sums; world points that f32 rounded off a plane leave 1e-14), a usable set has
// lambda_1 / lambda_max at the square of its relief over its extent.  kDltGap = 1e-10 lies between: it refuses what is flat to 1e-5
// of its extent, where the pose the eigenvector gives is noise anyway, and passes everything a start can be taken from.
// Mapping: refit_pnp_kernel's; 3.8 KB of LDS (the sums' partials, the Gram matrix, its eigenvectors).  No atomics: bit-repeatable.
constexpr double kDltGap = 1e-10;

template <typename T>
__global__ __launch_bounds__(kPRThreads) void pnp_dlt_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                             const T *__restrict__ weights, int N, T *__restrict__ model,
                                                             uint8_t *__restrict__ valid) {
  __shared__ double s_red[(kPRThreads / 64) * 40], s_gram[144], s_vec[144], s_cs[24];
  const int p = blockIdx.x, tid = threadIdx.x;
  const T *pt = matches + (size_t)p * N * 5;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T *wt = weights ? weights + (size_t)p * N : nullptr;
  auto row = [&](int n, double (&m)[5], double &w) {
    if (mk && !mk[n]) return false;
#pragma unroll
    for (int d = 0; d < 5; ++d) m[d] = (double)pt[(size_t)n * 5 + d];
    w = wt ? (double)wt[n] : 1.0;
    return true;
  };
  double a5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // rows, sum w, sum w X
  for (int n = tid; n < N; n += kPRThreads) {
    double m[5], w;
    if (!row(n, m, w)) continue;
    a5[0] += 1.0;
    a5[1] += w;
#pragma unroll
    for (int d = 0; d < 3; ++d) a5[2 + d] += w * m[d];
  }
  block_sum_f64<5>(a5, reinterpret_cast<double(*)[5]>(s_red));
  bool ok = a5[0] >= 6.0 && a5[1] > 0.0;
  const double rw = 1.0 / a5[1], c[3] = {a5[2] * rw, a5[3] * rw, a5[4] * rw};
  double dist[1] = {0.0};
  for (int n = tid; n < N; n += kPRThreads) {
    double m[5], w;
    if (!row(n, m, w)) continue;
    const double dx = m[0] - c[0], dy = m[1] - c[1], dz = m[2] - c[2];
    dist[0] += w * sqrt(dx * dx + dy * dy + dz * dz);
  }
  block_sum_f64<1>(dist, reinterpret_cast<double(*)[1]>(s_red));
  ok = ok && dist[0] > 0.0;
  const double sc = sqrt(3.0) * a5[1] / dist[0];
  double a[40];
#pragma unroll
  for (int q = 0; q < 40; ++q) a[q] = 0.0;
  for (int n = tid; n < N; n += kPRThreads) {
    double m[5], w;
    if (!row(n, m, w)) continue;
    const double xn[4] = {sc * (m[0] - c[0]), sc * (m[1] - c[1]), sc * (m[2] - c[2]), 1.0};
    const double k[4] = {w, w * m[3], w * m[4], w * (m[3] * m[3] + m[4] * m[4])};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) {
        const double xx = xn[i] * xn[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) a[10 * b + e] += k[b] * xx;
        ++e;
      }
  }
  block_sum_f64<40>(a, reinterpret_cast<double(*)[40]>(s_red));
#pragma unroll
  for (int q = 0; q < 40; ++q) ok = ok && is_finite(a[q]);
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < 40; ++q) s_red[q] = a[q];
  }
  __syncthreads();
  if (tid < 144) {
    const int i = tid / 12, j = tid % 12, bi = i / 4, bj = j / 4, qi = min(i % 4, j % 4), qj = max(i % 4, j % 4);
    const int e = qi * 4 - qi * (qi - 1) / 2 + (qj - qi);      // (qi, qj) of the 4x4 upper triangle, row-major
    const int lo = min(bi, bj), hi = max(bi, bj);
    double g = 0.0;
    if (lo == hi) g = s_red[(lo == 2 ? 30 : 0) + e];
    else if (hi == 2) g = -s_red[(lo == 0 ? 10 : 20) + e];
    s_gram[tid] = ok ? g : (i == j ? 1.0 : 0.0);
  }
  __syncthreads();
  if (tid < 64) jacobi_eig12_wave(s_gram, s_vec, s_cs, tid);
  __syncthreads();
  // the two smallest eigenvalues and the largest (every thread: the same LDS values)
  int best = 0;
  double l0 = INFINITY, l1 = INFINITY, lmax = -INFINITY;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const double d = s_gram[13 * i];
    lmax = fmax(lmax, d);
    if (d < l0) {
      l1 = l0;
      l0 = d;
      best = i;
    } else if (d < l1) {
      l1 = d;
    }
  }
  ok = ok && (l1 - l0) > kDltGap * lmax;      // (false for NaN)
  double h[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) h[q] = s_vec[q * 12 + best];
  // One refinement step on the equations themselves.  The Gram matrix is known to eps lambda_max, which leaves h at
  // eps lambda_max / (lambda_1 - lambda_0): the square of what the equations allow.  g = A^T (A h), summed over the rows, is known to
  // eps sigma_max |A h| instead, and with the eigenpairs at hand  h <- h - sum_{k != 0} v_k (v_k . g) / (lambda_k - h . g)  is the
  // first-order correction of the eigenvector (v_k . h = 0).  A term with a non-finite coefficient is not taken.
  double g[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) g[q] = 0.0;
  for (int n = tid; n < N; n += kPRThreads) {
    double m[5], w;
    if (!row(n, m, w)) continue;
    const double xn[4] = {sc * (m[0] - c[0]), sc * (m[1] - c[1]), sc * (m[2] - c[2]), 1.0};
    double d[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) d[b] = h[4 * b] * xn[0] + h[4 * b + 1] * xn[1] + h[4 * b + 2] * xn[2] + h[4 * b + 3];
    const double e1 = w * (d[0] - m[3] * d[2]), e2 = w * (d[1] - m[4] * d[2]), e3 = -(m[3] * e1 + m[4] * e2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      g[q] += e1 * xn[q];
      g[4 + q] += e2 * xn[q];
      g[8 + q] += e3 * xn[q];
    }
  }
  block_sum_f64<12>(g, reinterpret_cast<double(*)[12]>(s_red));
  {
    double l0r = 0.0, hn[12], nrm = 0.0;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      l0r += h[q] * g[q];
      hn[q] = h[q];
    }
#pragma unroll 1
    for (int k = 0; k < 12; ++k) {
      if (k == best) continue;
      double vg = 0.0;
#pragma unroll
      for (int q = 0; q < 12; ++q) vg += s_vec[q * 12 + k] * g[q];
      const double coef = vg / (s_gram[13 * k] - l0r);
      if (!is_finite(coef)) continue;
#pragma unroll
      for (int q = 0; q < 12; ++q) hn[q] -= coef * s_vec[q * 12 + k];
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) nrm += hn[q] * hn[q];
    const double rn = 1.0 / sqrt(nrm);
#pragma unroll
    for (int q = 0; q < 12; ++q) h[q] = is_finite(rn) ? hn[q] * rn : h[q];
  }
  double front[1] = {0.0};
  for (int n = tid; n < N; n += kPRThreads) {
    double m[5], w;
    if (!row(n, m, w)) continue;
    const double z = h[8] * (sc * (m[0] - c[0])) + h[9] * (sc * (m[1] - c[1])) + h[10] * (sc * (m[2] - c[2])) + h[11];
    front[0] += z > 0.0 ? w : -w;
  }
  block_sum_f64<1>(front, reinterpret_cast<double(*)[1]>(s_red));
  const double sg = front[0] < 0.0 ? -1.0 : 1.0;
  double M[3][3], mt[3], R[3][3], t[3], msv;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = sg * sc * h[4 * i + j];
    mt[i] = sg * h[4 * i + 3] - (M[i][0] * c[0] + M[i][1] * c[1] + M[i][2] * c[2]);
  }
  ok = nearest_rotation3(M, R, msv) && ok;
  ok = ok && msv > 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = mt[i] / msv;
    ok = ok && is_finite(t[i]);
  }
  if (tid == 0) {
    if (!ok) set_identity(R, t);
    store_rigid_model(model + (size_t)p * 16, R, t);
    valid[p] = ok;
  }
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                              \
  int dr_p3p_gather_##sfx(const T *matches, const int32_t *idx, int P, int B, int N, T *models, uint8_t *valid, void *stream) {     \
    DR_REQUIRE(matches && idx && models && valid, "null pointer");                                                                  \
    DR_REQUIRE(P > 0 && B > 0 && N > 0 && (long)P * B < (1l << 29), "need P, B, N > 0 and P * B < 2^29");                           \
    return dr::launch("p3p_gather_kernel", dr::p3p_gather_kernel<T>, dim3((P * B + 63) / 64), 64, stream, matches, idx, P * B, B,   \
                      N, models, valid);                                                                                            \
  }                                                                                                                                 \
  int dr_p3p_##sfx(const T *samples, int Bt, T *models, uint8_t *valid, void *stream) {                                             \
    DR_REQUIRE(samples && models && valid, "null pointer");                                                                         \
    DR_REQUIRE(Bt > 0 && Bt < (1 << 29), "need 0 < Bt < 2^29");                                                                     \
    return dr::launch("p3p_kernel", dr::p3p_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples, Bt, models, valid);               \
  }                                                                                                                                 \
  int dr_p3p_bwd_##sfx(const T *samples, const T *grad_models, int Bt, T *grad_samples, void *stream) {                             \
    DR_REQUIRE(samples && grad_models && grad_samples, "null pointer");                                                             \
    DR_REQUIRE(Bt > 0 && Bt < (1 << 29), "need 0 < Bt < 2^29");                                                                     \
    return dr::launch("p3p_bwd_kernel", dr::p3p_bwd_kernel<T>, dim3((Bt + 63) / 64), 64, stream, samples, grad_models, Bt,          \
                      grad_samples);                                                                                                \
  }                                                                                                                                 \
  int dr_pnp_score_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *thr2, int P, int M, int N, T *scores,    \
                         int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream) {                 \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535, "bad sizes");                                                                 \
    DR_REQUIRE((gate_iters == nullptr) == (gate_max_iters == nullptr), "gate: both pointers or neither");                           \
    return dr::launch_pair_score<T, dr::PnPGeom, dr::TransferMsacTerm<T>>(matches, models, valid, thr2, P, M, N, scores, inliers,   \
                                                                          gate_iters, gate_max_iters, stream);                      \
  }                                                                                                                                 \
  int dr_pnp_update_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *scores, const T *thr2, int P, int M,    \
                          int N, int B, double confidence, double eps, int max_iterations, T *best_score, T *best_model,            \
                          uint8_t *best_mask, int32_t *best_inliers, int32_t *iters, double *max_iters, void *stream) {             \
    DR_REQUIRE(matches && models && scores && thr2 && best_score && best_model && best_mask && best_inliers && iters && max_iters,  \
               "null pointer");                                                                                                     \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && B > 0 && max_iterations > 0, "bad sizes");                                                \
    return dr::launch("pair_update_kernel", dr::pair_update_kernel<T, dr::PnPGeom>, dim3(P), dr::kPairThreads, stream, matches,     \
                      models, valid, scores, thr2, M, N, B, confidence, eps, max_iterations, best_score, best_model, best_mask,     \
                      best_inliers, iters, max_iters);                                                                              \
  }                                                                                                                                 \
  int dr_refit_pnp_##sfx(const T *matches, const uint8_t *mask, const T *init_model, int P, int N, int iters, T *model,             \
                         uint8_t *valid, void *stream) {                                                                            \
    DR_REQUIRE(matches && init_model && model && valid, "null pointer");                                                            \
    DR_REQUIRE(P > 0 && N > 0 && (long)N * 5 < (1l << 31), "bad sizes");                                                            \
    DR_REQUIRE(iters >= 0, "iters must be at least 0");                                                                             \
    return dr::launch("refit_pnp_kernel", dr::refit_pnp_kernel<T, false>, dim3(P), dr::kPRThreads, stream, matches, mask,           \
                      (const T *)nullptr, init_model, N, iters, model, valid);                                                      \
  }                                                                                                                                 \
  int dr_refit_pnp_weighted_##sfx(const T *matches, const uint8_t *mask, const T *weights, const T *init_model, int P, int N,       \
                                  int iters, T *model, uint8_t *valid, void *stream) {                                              \
    DR_REQUIRE(matches && init_model && model && valid, "null pointer");                                                            \
    DR_REQUIRE(P > 0 && N > 0 && (long)N * 5 < (1l << 31), "bad sizes");                                                            \
    DR_REQUIRE(iters >= 0, "iters must be at least 0");                                                                             \
    return dr::launch("refit_pnp_kernel", weights ? dr::refit_pnp_kernel<T, true> : dr::refit_pnp_kernel<T, false>, dim3(P),        \
                      dr::kPRThreads, stream, matches, mask, weights, init_model, N, iters, model, valid);                          \
  }                                                                                                                                 \
  int dr_refit_pnp_bwd_##sfx(const T *matches, const uint8_t *mask, const T *weights, const T *model, const T *grad_model, int P,   \
                             int N, T *grad_matches, T *grad_weights, void *stream) {                                               \
    DR_REQUIRE(matches && model && grad_model, "null pointer");                                                                     \
    DR_REQUIRE(grad_matches || grad_weights, "no gradient asked for");                                                              \
    DR_REQUIRE(P > 0 && N > 0 && (long)N * 5 < (1l << 31), "bad sizes");                                                            \
    return dr::launch("refit_pnp_bwd_kernel", dr::refit_pnp_bwd_kernel<T>, dim3(P), dr::kPRThreads, stream, matches, mask, weights, \
                      model, grad_model, N, grad_matches, grad_weights);                                                            \
  }                                                                                                                                 \
  int dr_pnp_dlt_##sfx(const T *matches, const uint8_t *mask, const T *weights, int P, int N, T *model, uint8_t *valid,             \
                       void *stream) {                                                                                              \
    DR_REQUIRE(matches && model && valid, "null pointer");                                                                          \
    DR_REQUIRE(P > 0 && N > 0 && (long)N * 5 < (1l << 31), "bad sizes");                                                            \
    return dr::launch("pnp_dlt_kernel", dr::pnp_dlt_kernel<T>, dim3(P), dr::kPRThreads, stream, matches, mask, weights, N, model,   \
                      valid);                                                                                                       \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
