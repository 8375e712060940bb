// The soft-inlier score of the homography path (ops.homography_soft_score, loss.HomographyExpectedLoss): every model scored by a
// sigmoid of its squared symmetric transfer error on every match, with a reverse pass to the models AND to the matches.
// include/dransac.h states the maths; the residual is homography_loss.hip's:
//     h = sign(det H) H, A = adj(H), y = h (x1, 1), z = A (x2, 1), e = x2 - y_xy / y_w, f = x1 - z_xy / z_w, d2 = |e|^2 + |f|^2
//     a = beta (1 - d2 / thr2),   live = y_w > 0 and z_w > 0 and d2 finite and a >= -40,   w = live ? 1 / (1 + exp(-a)) : 0
//     score[m] = sum_{n in mask} w[m,n]
// A model is 9 values with adj(H) beside it, its reverse pass goes through the adjugate and all four columns of a match get a
// gradient, so these are kernels of their own and not a Term of soft_score_device.hpp; the mappings, the constants (kSoftTile,
// kSoftWaves, kSoftCutoff) and the rules are that scaffold's.  Three launches, no [P,M,N] tensor, no atomics, no workspace:
//   homography_soft_score_kernel<T, false>   the scores: one LANE per model (prepare_h: 9 + 9 registers), one wave per block, grid
//     (ceil(M / 64), P); the masked points compacted tile by tile (kSoftTile) into LDS in ascending order, each read as a broadcast;
//     the sum in the order of the points, with TwoSum.
//   homography_soft_score_kernel<T, true>    grad_models: the same walk with homography_loss_kernel's 9 + 9 accumulators gh, ga of the
//     two outer products, weighted by w (1 - w); adjugate3_vjp once per model after the point loop, then the sign of the determinant
//     and the model's factor 2 grad_scores[m] (-beta / thr2):  grad = sign c (gh + J_adj(h)^T ga).
//   homography_soft_score_points_kernel<T>   grad_matches, the TRANSPOSED mapping: a lane owns a point, grid (ceil(N / 64), P), a block
//     of kSoftWaves waves that share its 64 points and split the models.  Threads 0 .. kHSoftModels - 1 stage one model each per
//     tile: h AND adj(h) as prepare_h leaves them, c = 2 grad_scores (-beta / thr2) and a use flag; wave k walks models k,
//     k + kSoftWaves, ... of the tile reading each as a broadcast (a model that keep drops, one that prepare_h does not call scored,
//     a pair without a threshold: flag off, skipped by a wave-uniform branch, so a NaN there reaches nothing); at the end the waves'
//     partial sums are added in wave order through LDS.
//     The tile.  A staged model is h, adj(h) beyond the type's precision (below) and c: a row of 112 bytes in f32 and of 224 in f64.
//     512 models, one per thread, would be 112 KB in f64, above the 64 KB of static LDS.  Staging h alone and recomputing the
//     adjugate would add 18 vector instructions (90 in f64) per (wave, model) to the ~90 of a (model, point) term, in every lane
//     alike.  So the tile is kHSoftModels = 256 models in either type: 29 KB of static LDS in f32 and 57 KB in f64 (the flags
//     included; two blocks of eight waves on a CU in f64, which is what its registers allow as well); the two extra barriers per 256
//     models are nothing next to 32 terms per wave between them.
// The order of every sum depends on (M, N) and these constants alone: a repeated launch repeats its bytes.  Every barrier sits under
// a block-uniform branch (the tile loops' trip counts depend on M, N alone).
//
// Precision.  e cancels from |x2| ~ 10^2..10^3 pixels down to a few.  The loss kernel's treatment in the type itself (every linear form
// two fma, the f32 reciprocal Newton-refined, the quotient folded into the subtraction by one fma) leaves e with the rounding of the
// forms, about what rounding the inputs to f32 costs -- and missed the tests' bound, eight times what that rounding moves the
// reference, on the rows where the input roundings happen to cancel (docs/LOG.md: worst error / bound 1.96 on the scores).  So the
// f32 kernels form adj(h), y, z, the two reciprocals and the quotients in f64 and round e, f once, as the rigid term does for its
// residual; everything behind e, f stays in f32.  The f64 kernels missed the bound in the same way with the loss kernel's text (worst
// error / bound 1.69 on the scores, 38 on a grad_models row of 4e-21), so they form every linear form and every adjugate entry as
// hi + lo (TwoProduct by fma, TwoSum) and correct the quotient by its remainder: e, f are good to an eps of themselves in either
// type.  1 - w is formed as exp(-a) w: no cancellation on the sigmoid's flat top.
#include "homography_device.hpp"
#include "soft_score_device.hpp"

namespace dr {

constexpr int kHSoftModels = 256;      // models staged per tile of the point-lane kernel (see above)

// adj(h) as the residual takes it, beyond the type's precision.  f32: computed from the f32 entries in f64 and not rounded back (an
// adjugate rounded to f32 moves every point of its model by the same 1e-5 px, as much as rounding H itself does).  f64: every entry
// a b - c d as hi + lo, the two products by TwoProduct (fma) and their difference by TwoSum.
template <typename T>
struct WideAdj;
template <>
struct WideAdj<float> {
  double a[9];
};
template <>
struct WideAdj<double> {
  double a[9], lo[9];
};

__device__ __forceinline__ void wide_adjugate(const float (&h)[9], WideAdj<float> &A) {
  double hd[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) hd[q] = (double)h[q];
  adjugate3(hd, A.a);
}

// a product that no later sum may absorb: -ffp-contract=fast lets the backend fuse a * b + c across a contract(off) scope once the
// scope is inlined, and an error-free transformation needs the ROUNDED product (the empty asm only hides where the value came from)
__device__ __forceinline__ double rounded_product(double a, double b) {
  double p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ void diff_of_products(double a, double b, double c, double d, double &hi, double &lo) {
#pragma clang fp contract(off)
  const double p = rounded_product(a, b), ep = fma(a, b, -p), q = rounded_product(c, d), eq = fma(c, d, -q);
  double es;
  two_sum(p, -q, hi, es);
  lo = es + (ep - eq);
}

__device__ __forceinline__ void wide_adjugate(const double (&h)[9], WideAdj<double> &A) {      // (adjugate3's entries)
  diff_of_products(h[4], h[8], h[5], h[7], A.a[0], A.lo[0]);
  diff_of_products(h[2], h[7], h[1], h[8], A.a[1], A.lo[1]);
  diff_of_products(h[1], h[5], h[2], h[4], A.a[2], A.lo[2]);
  diff_of_products(h[5], h[6], h[3], h[8], A.a[3], A.lo[3]);
  diff_of_products(h[0], h[8], h[2], h[6], A.a[4], A.lo[4]);
  diff_of_products(h[2], h[3], h[0], h[5], A.a[5], A.lo[5]);
  diff_of_products(h[3], h[7], h[4], h[6], A.a[6], A.lo[6]);
  diff_of_products(h[1], h[6], h[0], h[7], A.a[7], A.lo[7]);
  diff_of_products(h[0], h[4], h[1], h[3], A.a[8], A.lo[8]);
}

// What one (model, point) pair's transfers hand on, rounded to T once: e = x2 - y_xy / y_w, f = x1 - z_xy / z_w, the reciprocals,
// the quotients t, and whether both third coordinates are positive
template <typename T>
struct TransferRes {
  T e0, e1, f0, f1, ry, rz, ty0, ty1, tz0, tz1;
  bool front;
};

// f32: y, z, the two reciprocals (v_rcp_f32 and one Newton step in f64: 1e-14) and the quotients in f64
__device__ __forceinline__ void transfer_res(const float (&h)[9], const WideAdj<float> &A, const float (&x)[4], TransferRes<float> &r) {
  const double(&a)[9] = A.a;
  const double x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
  const double yx = fma((double)h[0], x0, fma((double)h[1], x1, (double)h[2]));
  const double yy = fma((double)h[3], x0, fma((double)h[4], x1, (double)h[5]));
  const double yw = fma((double)h[6], x0, fma((double)h[7], x1, (double)h[8]));
  const double zx = fma(a[0], x2, fma(a[1], x3, a[2]));
  const double zy = fma(a[3], x2, fma(a[4], x3, a[5]));
  const double zw = fma(a[6], x2, fma(a[7], x3, a[8]));
  const double r0 = (double)__builtin_amdgcn_rcpf((float)yw), r1 = (double)__builtin_amdgcn_rcpf((float)zw);
  const double ry = fma(r0, fma(-yw, r0, 1.0), r0), rz = fma(r1, fma(-zw, r1, 1.0), r1);      // (0 or inf gives NaN: not `front`, or
                                                                                              // not finite in d2)
  r.e0 = (float)fma(-yx, ry, x2), r.e1 = (float)fma(-yy, ry, x3);
  r.f0 = (float)fma(-zx, rz, x0), r.f1 = (float)fma(-zy, rz, x1);
  r.ry = (float)ry, r.rz = (float)rz;
  r.ty0 = (float)(yx * ry), r.ty1 = (float)(yy * ry), r.tz0 = (float)(zx * rz), r.tz1 = (float)(zy * rz);
  r.front = yw > 0.0 && zw > 0.0;
}

// c0 u + c1 v + c2 as hi + lo: TwoProduct by fma, TwoSum
__device__ __forceinline__ void form2(double c0, double c1, double c2, double u, double v, double &hi, double &lo) {
#pragma clang fp contract(off)
  const double p0 = rounded_product(c0, u), e0 = fma(c0, u, -p0), p1 = rounded_product(c1, v), e1 = fma(c1, v, -p1);
  double s, es0, es1;
  two_sum(p0, p1, s, es0);
  two_sum(s, c2, hi, es1);
  lo = (e0 + e1) + (es0 + es1);
}

// x - (nh + nl) / (dh + dl) and the quotient: q = nh rd, its remainder exactly by fma, one correction; x - q is exact wherever the
// residual is small (Sterbenz), so e is good to an eps of ITSELF
__device__ __forceinline__ double residual2(double nh, double nl, double dh, double dl, double rd, double x, double &t) {
#pragma clang fp contract(off)
  const double q = rounded_product(nh, rd);
  const double rem = fma(-q, dh, nh) + (nl - q * dl);
  const double qc = rem * rd;
  t = q + qc;
  return (x - q) - qc;
}

// f64: every linear form as hi + lo (the adjugate's lo parts included), the quotient corrected by its remainder
__device__ __forceinline__ void transfer_res(const double (&h)[9], const WideAdj<double> &A, const double (&x)[4],
                                             TransferRes<double> &r) {
  double yxh, yxl, yyh, yyl, ywh, ywl, zxh, zxl, zyh, zyl, zwh, zwl;
  form2(h[0], h[1], h[2], x[0], x[1], yxh, yxl);
  form2(h[3], h[4], h[5], x[0], x[1], yyh, yyl);
  form2(h[6], h[7], h[8], x[0], x[1], ywh, ywl);
  form2(A.a[0], A.a[1], A.a[2], x[2], x[3], zxh, zxl);
  form2(A.a[3], A.a[4], A.a[5], x[2], x[3], zyh, zyl);
  form2(A.a[6], A.a[7], A.a[8], x[2], x[3], zwh, zwl);
  zxl += fma(A.lo[0], x[2], fma(A.lo[1], x[3], A.lo[2]));
  zyl += fma(A.lo[3], x[2], fma(A.lo[4], x[3], A.lo[5]));
  zwl += fma(A.lo[6], x[2], fma(A.lo[7], x[3], A.lo[8]));
  r.ry = 1.0 / ywh, r.rz = 1.0 / zwh;
  r.e0 = residual2(yxh, yxl, ywh, ywl, r.ry, x[2], r.ty0);
  r.e1 = residual2(yyh, yyl, ywh, ywl, r.ry, x[3], r.ty1);
  r.f0 = residual2(zxh, zxl, zwh, zwl, r.rz, x[0], r.tz0);
  r.f1 = residual2(zyh, zyl, zwh, zwl, r.rz, x[1], r.tz1);
  r.front = ywh > 0.0 && zwh > 0.0;
}

// One (model, point) term.  -> live; s = w (1 - w); (e, f) the two residuals; u = s d d2 / d y / 2 = (s / y_w) (-e_0, -e_1, e . t) with
// t = y_xy / y_w, and v the same for z.  Everything but `w` is an exact 0 where the point is not live.  nbt = -beta / thr2.
template <typename T>
struct TransferSoft {
  bool live;
  T w, s, e[2], f[2], u[3], v[3];
};

template <typename T>
__device__ __forceinline__ void transfer_soft(const T (&h)[9], const WideAdj<T> &A, const T (&x)[4], T nbt, T beta,
                                              TransferSoft<T> &o) {
  TransferRes<T> r;
  transfer_res(h, A, x, r);
  const T e0 = r.e0, e1 = r.e1, f0 = r.f0, f1 = r.f1;
  const T d2 = fma(e0, e0, fma(e1, e1, fma(f0, f0, f1 * f1)));
  const T arg = fma(d2, nbt, beta);                   // beta (1 - d2 / thr2)
  const bool live = r.front && is_finite(d2) && arg >= T(kSoftCutoff);      // (false for a NaN anywhere)
  const T ex = exp(-arg);
  const T w = live ? T(1) / (T(1) + ex) : T(0);
  const T s = live ? w * (ex * w) : T(0);
  o.live = live, o.w = w, o.s = s;
  o.e[0] = live ? e0 : T(0), o.e[1] = live ? e1 : T(0);
  o.f[0] = live ? f0 : T(0), o.f[1] = live ? f1 : T(0);
  const T sy = live ? s * r.ry : T(0), sz = live ? s * r.rz : T(0);
  o.u[0] = live ? -(e0 * sy) : T(0), o.u[1] = live ? -(e1 * sy) : T(0);
  o.u[2] = live ? fma(e0, r.ty0, e1 * r.ty1) * sy : T(0);
  o.v[0] = live ? -(f0 * sz) : T(0), o.v[1] = live ? -(f1 * sz) : T(0);
  o.v[2] = live ? fma(f0, r.tz0, f1 * r.tz1) * sz : T(0);
}

// a staged model of the point-lane kernel: adj(h) as above, h, c = 2 grad_scores (-beta / thr2); 112 bytes in f32, 224 in f64
template <typename T>
struct alignas(16) HSoftRow {
  WideAdj<T> A;
  T h[9], c;
};

// kGrad = false: out = scores [P,M].  kGrad = true: out = grad_models [P,M,9] for the upstream grad_scores [P,M].
template <typename T, bool kGrad>
__global__ __launch_bounds__(64) void homography_soft_score_kernel(const T *__restrict__ matches, const uint8_t *__restrict__ mask,
                                                                   const T *__restrict__ models, const uint8_t *__restrict__ keep,
                                                                   const T *__restrict__ thr2, T beta,
                                                                   const T *__restrict__ grad_scores, int M, int N,
                                                                   T *__restrict__ out) {
  __shared__ Match4<T> s_pt[kSoftTile];
  const int p = blockIdx.y, lane = threadIdx.x, m = blockIdx.x * 64 + lane;
  const Match4<T> *pt = reinterpret_cast<const Match4<T> *>(matches) + (size_t)p * N;
  const uint8_t *mk = mask ? mask + (size_t)p * N : nullptr;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);                      // (false for NaN too: the pair then scores 0 and passes nothing)
  const T nbt = thr_ok ? -beta / t2 : T(0);
  // a slot that keep drops is SKIPPED (its model, possibly NaN, is never read); a kept model that prepare_h does not call scored (a
  // non-finite entry, det == 0, a non-finite det) scores 0 and passes nothing
  const bool kept = m < M && (!keep || keep[(size_t)p * M + m] != 0);
  T raw[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) raw[q] = kept ? models[((size_t)p * M + m) * 9 + q] : T(0);
  ScoredH<T> s;
  prepare_h(raw, kept, s);
  const bool scored = s.kind == kModelScored;
  // prepare_h has turned h to det > 0; the gradient is turned back at the end (adj(-H) = adj(H): a needs no sign)
  const bool neg = fma(raw[0], s.a[0], fma(raw[1], s.a[3], raw[2] * s.a[6])) < T(0);
  if (!scored) {
#pragma unroll
    for (int q = 0; q < 9; ++q) s.h[q] = s.a[q] = T(0);      // y_w = z_w = 0: no point is live, nothing non-finite is accumulated
  }
  WideAdj<T> adj;
  wide_adjugate(s.h, adj);

  T acc = T(0), acc_lo = T(0), gh[9], ga[9];          // acc + acc_lo: the score, summed with TwoSum (soft_score_kernel says why)
#pragma unroll
  for (int q = 0; q < 9; ++q) gh[q] = ga[q] = T(0);

  for (int n0 = 0; n0 < N; n0 += kSoftTile) {
    // the tile's masked points, compacted in ascending order (ballot + prefix count: the wave is the block)
    int count = 0;
#pragma unroll
    for (int j = 0; j < kSoftTile / 64; ++j) {
      const int n = n0 + j * 64 + lane;
      const bool on = n < N && (!mk || mk[n] != 0);
      const unsigned long long b = __ballot(on);
      const int pos = count + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
      if (on) s_pt[pos] = pt[n];
      count += __popcll(b);
    }
    __syncthreads();
#pragma unroll 2
    for (int i = 0; i < count; ++i) {
      const Match4<T> xv = s_pt[i];
      const T(&x)[4] = xv.v;
      TransferSoft<T> o;
      transfer_soft(s.h, adj, x, nbt, beta, o);
      if (!kGrad) {
        T err;
        two_sum(acc, o.w, acc, err);
        acc_lo += err;
      } else {
        gh[0] = fma(o.u[0], x[0], gh[0]), gh[1] = fma(o.u[0], x[1], gh[1]), gh[2] += o.u[0];
        gh[3] = fma(o.u[1], x[0], gh[3]), gh[4] = fma(o.u[1], x[1], gh[4]), gh[5] += o.u[1];
        gh[6] = fma(o.u[2], x[0], gh[6]), gh[7] = fma(o.u[2], x[1], gh[7]), gh[8] += o.u[2];
        ga[0] = fma(o.v[0], x[2], ga[0]), ga[1] = fma(o.v[0], x[3], ga[1]), ga[2] += o.v[0];
        ga[3] = fma(o.v[1], x[2], ga[3]), ga[4] = fma(o.v[1], x[3], ga[4]), ga[5] += o.v[1];
        ga[6] = fma(o.v[2], x[2], ga[6]), ga[7] = fma(o.v[2], x[3], ga[7]), ga[8] += o.v[2];
      }
    }
    __syncthreads();
  }

  if (m >= M) return;
  const size_t slot = (size_t)p * M + m;
  const bool good = kept && scored && thr_ok;
  if (!kGrad) {
    out[slot] = good ? acc + acc_lo : T(0);
  } else {
    T back[9];
    adjugate3_vjp(s.h, ga, back);
    // (a dropped slot's grad_scores, possibly NaN, reaches nothing)
    const T sc = good ? (neg ? T(-2) : T(2)) * nbt * grad_scores[slot] : T(0);
    T *g = out + slot * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) g[q] = good ? sc * (gh[q] + back[q]) : T(0);
  }
}

// grad_matches [P,N,4]: d / d x1 = c (s f + h[:, :2]^T u), d / d x2 = c (s e + A[:, :2]^T v) summed over the kept models
template <typename T>
__global__ __launch_bounds__(64 * kSoftWaves) void homography_soft_score_points_kernel(
    const T *__restrict__ matches, const uint8_t *__restrict__ mask, const T *__restrict__ models, const uint8_t *__restrict__ keep,
    const T *__restrict__ thr2, T beta, const T *__restrict__ grad_scores, int M, int N, T *__restrict__ grad_matches) {
  __shared__ HSoftRow<T> s_md[kHSoftModels];
  __shared__ int s_use[kHSoftModels];
  static_assert(sizeof(HSoftRow<T>) * kHSoftModels >= sizeof(T) * kSoftWaves * 4 * 64, "the waves' partial sums reuse the model tile");
  static_assert(kHSoftModels <= 64 * kSoftWaves, "one thread stages one model");
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = blockIdx.x * 64 + lane;
  const T t2 = thr2[p];
  const bool thr_ok = t2 > T(0);
  const T nbt = thr_ok ? -beta / t2 : T(0);
  const bool have = n < N;
  const bool on = have && (!mask || mask[(size_t)p * N + n] != 0);
  const bool wave_on = __ballot(on) != 0ull;          // a wave without a masked point only keeps the barriers
  Match4<T> xv;
#pragma unroll
  for (int d = 0; d < 4; ++d) xv.v[d] = T(0);
  if (have) xv = reinterpret_cast<const Match4<T> *>(matches)[(size_t)p * N + n];
  const T(&x)[4] = xv.v;
  T acc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) acc[d] = T(0);

  for (int m0 = 0; m0 < M; m0 += kHSoftModels) {
    if (tid < kHSoftModels) {
      const int m = m0 + tid;
      const size_t slot = (size_t)p * M + m;
      const bool kept = m < M && (!keep || keep[slot] != 0);
      T raw[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) raw[q] = kept ? models[slot * 9 + q] : T(0);
      ScoredH<T> s;
      prepare_h(raw, kept, s);
      const bool use = s.kind == kModelScored && thr_ok;
      T c = T(0);
      if (use) c = T(2) * nbt * grad_scores[slot];
      WideAdj<T> adj;
      wide_adjugate(s.h, adj);
      if (!use) adj = WideAdj<T>{};
#pragma unroll
      for (int q = 0; q < 9; ++q) s_md[tid].h[q] = use ? s.h[q] : T(0);
      s_md[tid].A = adj;
      s_md[tid].c = c;
      s_use[tid] = use ? 1 : 0;
    }
    __syncthreads();
    const int count = wave_on ? min(kHSoftModels, M - m0) : 0;
    for (int i = wv; i < count; i += kSoftWaves) {
      if (!s_use[i]) continue;                        // (the same word in every lane: the wave skips the model as one)
      T h[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) h[q] = s_md[i].h[q];
      const WideAdj<T> A = s_md[i].A;
      const double(&a)[9] = A.a;
      const T c = s_md[i].c;
      TransferSoft<T> o;
      transfer_soft(h, A, x, nbt, beta, o);
      acc[0] = fma(c, fma(h[0], o.u[0], fma(h[3], o.u[1], fma(h[6], o.u[2], o.s * o.f[0]))), acc[0]);
      acc[1] = fma(c, fma(h[1], o.u[0], fma(h[4], o.u[1], fma(h[7], o.u[2], o.s * o.f[1]))), acc[1]);
      acc[2] = fma(c, fma((T)a[0], o.v[0], fma((T)a[3], o.v[1], fma((T)a[6], o.v[2], o.s * o.e[0]))), acc[2]);
      acc[3] = fma(c, fma((T)a[1], o.v[0], fma((T)a[4], o.v[1], fma((T)a[7], o.v[2], o.s * o.e[1]))), acc[3]);
    }
    __syncthreads();
  }

  // the waves' partial sums, added in wave order
  T *red = reinterpret_cast<T *>(s_md);
#pragma unroll
  for (int d = 0; d < 4; ++d) red[(wv * 4 + d) * 64 + lane] = acc[d];
  __syncthreads();
  if (wv == 0 && have) {
    Match4<T> g;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      T t = T(0);
#pragma unroll
      for (int k = 0; k < kSoftWaves; ++k) t += red[(k * 4 + d) * 64 + lane];
      g.v[d] = on ? t : T(0);                         // an unmasked point: exact zeros
    }
    reinterpret_cast<Match4<T> *>(grad_matches)[(size_t)p * N + n] = g;
  }
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                                 \
  int dr_homography_soft_score_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,      \
                                     T beta, int P, int M, int N, T *scores, void *stream) {                                          \
    DR_REQUIRE(matches && models && thr2 && scores, "null pointer");                                                                  \
    DR_PAIR_LOSS_SIZES;                                                                                                               \
    DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite");                                                \
    return dr::launch("homography_soft_score_kernel", dr::homography_soft_score_kernel<T, false>, dim3((M + 63) / 64, P), 64, stream, \
                      matches, mask, models, keep, thr2, beta, (const T *)nullptr, M, N, scores);                                     \
  }                                                                                                                                   \
  int dr_homography_soft_score_bwd_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,  \
                                         T beta, const T *grad_scores, int P, int M, int N, T *grad_models, T *grad_matches,          \
                                         void *stream) {                                                                              \
    DR_REQUIRE(matches && models && thr2 && grad_scores && grad_models, "null pointer");                                              \
    DR_PAIR_LOSS_SIZES;                                                                                                               \
    DR_REQUIRE(beta > T(0) && beta < T(INFINITY), "beta must be positive and finite");                                                \
    if (int rc = dr::launch("homography_soft_score_kernel", dr::homography_soft_score_kernel<T, true>, dim3((M + 63) / 64, P), 64,    \
                            stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_models))                         \
      return rc;                                                                                                                      \
    if (!grad_matches) return DR_OK;                  /* matches that need no gradient: the point pass is not launched */            \
    return dr::launch("homography_soft_score_points_kernel", dr::homography_soft_score_points_kernel<T>, dim3((N + 63) / 64, P),      \
                      64 * dr::kSoftWaves, stream, matches, mask, models, keep, thr2, beta, grad_scores, M, N, grad_matches);         \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
