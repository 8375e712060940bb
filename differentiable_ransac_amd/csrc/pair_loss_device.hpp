// What the training losses of the pair families share (registration_loss.hip: rigid models, homography_loss.hip: plane-induced
// homographies): the ground-truth mask on the families' Geom policies (pair_state_device.hpp), the per-pair / mean reduction of the
// per-model sums, the elementwise backward of that mean, the launch and the C entries.
// A family's file keeps its loss kernel <family>_loss_kernel<T, kGrad> whole: staging, model, point arithmetic, accumulators and the
// final scaling stay one function body.  (The simplification passes run on a callee before it is inlined: behind force-inlined
// functions the same arithmetic is vectorised and allocated differently, which costs the fused homography kernel 74 -> 86 VGPRs and a
// wave of occupancy; the staging alone behind a function moves every instance by a few registers: docs/LOG.md.)
// The mean and the scale kernels do not know the model's width: the mean reads sums, mask and keep; the scale takes the per-pair width
// as an argument.
#pragma once
#include "pair_state_device.hpp"

namespace dr {

// ---- mask[p,n] = Geom::inlier under the pair's ground-truth model (the score kernels' and the state step's test), count[p] ---------
template <typename T, typename Geom>
__global__ __launch_bounds__(256) void pair_gt_mask_kernel(const T *__restrict__ matches, const T *__restrict__ gt_model,
                                                          const T *__restrict__ thr2, int N, uint8_t *__restrict__ mask,
                                                          int32_t *__restrict__ count) {
  __shared__ int s_cnt[4];
  const int p = blockIdx.x, tid = threadIdx.x;
  typename Geom::template Slot<T> s;
  const bool scored = Geom::prepare(gt_model + (size_t)p * Geom::kModel, s) == kModelScored;
  const T t2 = thr2[p];
  int c = 0;
  for (int n = tid; n < N; n += 256) {
    const auto x = Geom::template Point<T>::load(matches, (size_t)p * N + n);
    const bool on = scored && Geom::inlier(s, x.v, t2);
    mask[(size_t)p * N + n] = on ? 1 : 0;
    c += on ? 1 : 0;
  }
  c = wave_sum(c);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) count[p] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

constexpr int kPairLossMeanT = 1024;

// per_pair[p] = sum_m sums[p,m] / max(#kept_p #mask_p, 1), coef[p] = 1 / that denominator, mean = sum_p per_pair[p] / P: ONE block whose
// sixteen waves take the pairs in turn; lane partials, wave butterfly, waves in order -- a fixed order.  It reads P (5 M + N) bytes
// on one CU: microseconds at a train step's shape, hence the entries' bound P M < 2^22 (16 MB of sums)
template <typename T>
__global__ __launch_bounds__(kPairLossMeanT) void pair_loss_mean_kernel(const T *__restrict__ sums, const uint8_t *__restrict__ mask,
                                                                       const uint8_t *__restrict__ keep, int P, int M, int N,
                                                                       T *__restrict__ per_pair, T *__restrict__ coef,
                                                                       T *__restrict__ mean) {
  __shared__ T s_tot[kPairLossMeanT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T wave_total = T(0);
  for (int p = wv; p < P; p += kPairLossMeanT / 64) {
    T acc = T(0);
    int n_in = 0, n_kept = 0;
    for (int m = lane; m < M; m += 64) {
      acc += sums[(size_t)p * M + m];
      if (keep) n_kept += keep[(size_t)p * M + m] != 0;
    }
    if (mask)
      for (int n = lane; n < N; n += 64) n_in += mask[(size_t)p * N + n] != 0;
    acc = wave_sum(acc);
    n_in = mask ? wave_sum(n_in) : N;
    n_kept = keep ? wave_sum(n_kept) : M;
    const T den = fmax((T)n_in * (T)n_kept, T(1));
    if (lane == 0) {
      per_pair[p] = acc / den;
      coef[p] = T(1) / den;
    }
    wave_total += acc / den;
  }
  if (lane == 0) s_tot[wv] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    T t = T(0);
    for (int w = 0; w < kPairLossMeanT / 64; ++w) t += s_tot[w];
    mean[0] = t / (T)P;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pair_loss_scale_kernel(const T *__restrict__ grad_unscaled, const T *__restrict__ coef,
                                                             const T *__restrict__ grad_mean, T inv_pairs, size_t per_pair,
                                                             size_t total, T *__restrict__ grad_models) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) grad_models[i] = grad_unscaled[i] * (coef[i / per_pair] * grad_mean[0] * inv_pairs);
}

// the loss value (and, with a gradient kernel, its unscaled gradient) per model by the family's `kernel`, then the means
template <typename T, typename Kernel>
int pair_loss_launch(const char *name, Kernel kernel, const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep,
                     const T *thr2, int P, int M, int N, T *sums, T *grad_unscaled, T *per_pair, T *coef, T *mean, void *stream) {
  if (int rc = launch(name, kernel, dim3((M + 63) / 64, P), 64, stream, matches, mask, models, keep, thr2, M, N, sums, grad_unscaled))
    return rc;
  return launch("pair_loss_mean_kernel", pair_loss_mean_kernel<T>, dim3(1), kPairLossMeanT, stream, sums, mask, keep, P, M, N,
                per_pair, coef, mean);
}

}  // namespace dr

// ---- the C entries of one family: dr_<family>_loss_fused / _loss_fwd / _loss_scale and dr_<family>_gt_mask --------------------------
// A family's file stamps them, inside extern "C", with  #define DR_OP(sfx, T) DR_PAIR_LOSS_OP(<family>, dr::<Geom>, sfx, T)  under
// DR_F32_F64(DR_OP); its loss kernel is dr::<family>_loss_kernel<T, kGrad>.
#define DR_PAIR_LOSS_SIZES \
  DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535 && (long)P * M < (1l << 22), "need P, M, N > 0, P <= 65535 and P M < 2^22")

#define DR_PAIR_LOSS_OP(family, Geom, sfx, T)                                                                                      \
  int dr_##family##_loss_fused_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,    \
                                     int P, int M, int N, T *sums, T *grad_unscaled, T *per_pair, T *coef, T *mean,                 \
                                     void *stream) {                                                                                \
    DR_REQUIRE(matches && models && thr2 && sums && grad_unscaled && per_pair && coef && mean, "null pointer");                     \
    DR_PAIR_LOSS_SIZES;                                                                                                             \
    return dr::pair_loss_launch(#family "_loss_kernel", dr::family##_loss_kernel<T, true>, matches, mask, models, keep, thr2, P, M, \
                                N, sums, grad_unscaled, per_pair, coef, mean, stream);                                              \
  }                                                                                                                                 \
  int dr_##family##_loss_fwd_##sfx(const T *matches, const uint8_t *mask, const T *models, const uint8_t *keep, const T *thr2,      \
                                   int P, int M, int N, T *sums, T *per_pair, T *coef, T *mean, void *stream) {                     \
    DR_REQUIRE(matches && models && thr2 && sums && per_pair && coef && mean, "null pointer");                                      \
    DR_PAIR_LOSS_SIZES;                                                                                                             \
    return dr::pair_loss_launch(#family "_loss_kernel", dr::family##_loss_kernel<T, false>, matches, mask, models, keep, thr2, P,   \
                                M, N, sums, (T *)nullptr, per_pair, coef, mean, stream);                                            \
  }                                                                                                                                 \
  int dr_##family##_loss_scale_##sfx(const T *grad_unscaled, const T *coef, const T *grad_mean, int P, int M, T *grad_models,       \
                                     void *stream) {                                                                                \
    DR_REQUIRE(grad_unscaled && coef && grad_mean && grad_models, "null pointer");                                                  \
    DR_REQUIRE(P > 0 && M > 0 && (long)P * M < (1l << 22), "need P, M > 0 and P M < 2^22");                                         \
    const size_t total = (size_t)P * M * Geom::kModel;                                                                              \
    return dr::launch("pair_loss_scale_kernel", dr::pair_loss_scale_kernel<T>, dim3((unsigned)((total + 255) / 256)), 256, stream,  \
                      grad_unscaled, coef, grad_mean, T(1) / (T)P, (size_t)M * Geom::kModel, total, grad_models);                   \
  }                                                                                                                                 \
  int dr_##family##_gt_mask_##sfx(const T *matches, const T *gt_model, const T *thr2, int P, int N, uint8_t *mask, int32_t *count,  \
                                  void *stream) {                                                                                   \
    DR_REQUIRE(matches && gt_model && thr2 && mask && count, "null pointer");                                                       \
    DR_REQUIRE(P > 0 && N > 0, "need P, N > 0");                                                                                    \
    return dr::launch("pair_gt_mask_kernel", dr::pair_gt_mask_kernel<T, Geom>, dim3(P), 256, stream, matches, gt_model, thr2, N,    \
                      mask, count);                                                                                                 \
  }
