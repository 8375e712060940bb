// What the training-loss kernels of the pair families share (registration_loss.hip, homography_loss.hip): the per-pair / mean
// reduction of the per-model sums and the elementwise backward of that mean.  Neither knows the model's width: the mean reads sums,
// mask and keep; the scale takes the per-pair width as an argument.
#pragma once
#include "dr_common.hpp"

namespace dr {

constexpr int kRLMeanT = 1024;

// per_pair[p] = sum_m sums[p,m] / max(#kept_p #mask_p, 1), coef[p] = 1 / that denominator, mean = sum_p per_pair[p] / P: ONE block whose
// sixteen waves take the pairs in turn; lane partials, wave butterfly, waves in order -- a fixed order.  It reads P (5 M + N) bytes
// on one CU: microseconds at a train step's shape, hence the entries' bound P M < 2^22 (16 MB of sums)
template <typename T>
__global__ __launch_bounds__(kRLMeanT) void registration_loss_mean_kernel(const T *__restrict__ sums, const uint8_t *__restrict__ mask,
                                                                         const uint8_t *__restrict__ keep, int P, int M, int N,
                                                                         T *__restrict__ per_pair, T *__restrict__ coef,
                                                                         T *__restrict__ mean) {
  __shared__ T s_tot[kRLMeanT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T wave_total = T(0);
  for (int p = wv; p < P; p += kRLMeanT / 64) {
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
    for (int w = 0; w < kRLMeanT / 64; ++w) t += s_tot[w];
    mean[0] = t / (T)P;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void registration_loss_scale_kernel(const T *__restrict__ grad_unscaled, const T *__restrict__ coef,
                                                                     const T *__restrict__ grad_mean, T inv_pairs, size_t per_pair,
                                                                     size_t total, T *__restrict__ grad_models) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < total) grad_models[i] = grad_unscaled[i] * (coef[i / per_pair] * grad_mean[0] * inv_pairs);
}

}  // namespace dr
