// What the per-pair test-mode families with their state on the device share (registration.hip: rigid models, homography.hip:
// plane-induced homographies): the kernel that scores every model against every point, the state step, the block-wide f64 sum
// of their refits, and the polish of the state behind the step (pair_block_score, pair_polish).  A family enters as a policy struct
// Geom (RigidGeom in rigid_device.hpp, HomographyGeom in homography_device.hpp):
//   kModel, kWidth, kSample        values per model (16 / 9) and per match (6 / 4), sample size of the adaptive stop (3 / 4)
//   kFirstRoundTakes               does the state step take the first round's best even when it is not strictly higher
//   Slot<T>, prepare(m, slot)      a model ready to be evaluated -> its kind (ransac_device.hpp's ModelKind); wave-uniform
//   kind(m, live)                  the kind of a slot whose valid byte is `live`; dead_score<T>(kind) = what a slot that is not scored gets
//   Chunk<T>                       a lane's kPairPts points of a chunk: load(pt, c0, tid, N), live(j), point(j)
//   Point<T>                       one match of the state step: load(matches, row), v[kWidth]
//   d2(slot, x, d2)                the squared residual of one point -> may the point count at all (in front of both cameras)
//   inlier(slot, x, thr2)          the inlier decision of the state step's mask: d2's expression behind the term's d2 < thr2
#pragma once
#include "ransac_device.hpp"

namespace dr {

constexpr int kPairThreads = 256, kPairPts = 8, kPairChunk = kPairThreads * kPairPts, kPairModels = 16;

// ---- score and inlier count of every model against every point, under a per-point term ---------------------------------------------
// One block = (pair, tile of kPairModels model slots) and walks ALL the pair's points in chunks of kPairChunk.  A lane keeps
// kPairPts points of the chunk in registers across the tile (which ones is the family's: Geom::Chunk); the model is wave-uniform: its
// values are read through a uniform address and prepared once per (model, chunk), and a slot that is not valid is left before
// anything of it is loaded.  The sum of a (pair, model) is reduced in one fixed order -- a lane's points in order, the wave butterfly,
// chunk after chunk into the wave's LDS slot, the four slots in order -- so a repeated launch gives the same bits (scores are compared
// strictly downstream).  No [P,M,N] tensor, no floating-point atomics.
// A term is built from thr2 once per block and has inlier(d2) and contrib(d2, live), the point's part of the score: 0 where it adds
// nothing, so 0 for a NaN distance too, and 0 where `live` is false: a slot past the end of the row, or a point Geom::d2 refuses.
template <typename T, typename Geom, typename Term>
__global__ __launch_bounds__(kPairThreads) void pair_score_kernel(const T *__restrict__ matches, const T *__restrict__ models,
                                                                  const uint8_t *__restrict__ valid, const T *__restrict__ thr2, int M,
                                                                  int N, T *__restrict__ scores, int32_t *__restrict__ inliers,
                                                                  PairGate gate) {
  __shared__ T part[kPairThreads / 64][kPairModels];
  __shared__ int pcnt[kPairThreads / 64][kPairModels];
  const int p = blockIdx.y, m0 = blockIdx.x * kPairModels;
  if (gate.closed(p)) return;   // a terminated pair of a multi-round call (block-uniform): its scores keep their contents
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int mcount = min(kPairModels, M - m0);
  const T *pt = matches + (size_t)p * N * Geom::kWidth;
  const T *md = models + ((size_t)p * M + m0) * Geom::kModel;
  const uint8_t *vd = valid ? valid + (size_t)p * M + m0 : nullptr;
  const Term term(thr2[p]);
  if (tid < (kPairThreads / 64) * kPairModels) {
    (&part[0][0])[tid] = T(0);
    (&pcnt[0][0])[tid] = 0;
  }
  __syncthreads();
  for (int c0 = 0; c0 < N; c0 += kPairChunk) {
    typename Geom::template Chunk<T> x;
    x.load(pt, c0, tid, N);
    for (int ml = 0; ml < mcount; ++ml) {
      if (vd && !vd[ml]) continue;   // (wave-uniform)
      typename Geom::template Slot<T> s;
      if (Geom::prepare(md + ml * Geom::kModel, s) != kModelScored) continue;
      T acc = T(0);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < kPairPts; ++j) {
        T d2;
        const bool live = Geom::d2(s, x.point(j), d2) && x.live(j);
        acc += term.contrib(d2, live);
        cnt += (live && term.inlier(d2)) ? 1 : 0;
      }
      acc = wave_sum(acc);
      cnt = wave_sum(cnt);
      if (lane == 0) {
        part[wv][ml] += acc;
        pcnt[wv][ml] += cnt;
      }
    }
  }
  __syncthreads();
  if (tid < mcount) {
    const int kind = Geom::kind(md + tid * Geom::kModel, !vd || vd[tid]);
    T v = T(0);
    int n = 0;
#pragma unroll
    for (int w = 0; w < kPairThreads / 64; ++w) {
      v += part[w][tid];
      n += pcnt[w][tid];
    }
    scores[(size_t)p * M + m0 + tid] = kind == kModelScored ? v : Geom::template dead_score<T>(kind);
    if (inliers) inliers[(size_t)p * M + m0 + tid] = kind == kModelScored ? n : 0;
  }
}

template <typename T, typename Geom, typename Term>
int launch_pair_score(const T *matches, const T *models, const uint8_t *valid, const T *thr2, int P, int M, int N, T *scores,
                      int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream) {
  PairGate gate;
  gate.iters = gate_iters;
  gate.max_iters = gate_max_iters;
  return launch("pair_score_kernel", pair_score_kernel<T, Geom, Term>, dim3((M + kPairModels - 1) / kPairModels, P), kPairThreads,
                stream, matches, models, valid, thr2, M, N, scores, inliers, gate);
}

// ---- the state step ------------------------------------------------------------------------------------------------------------------
// One block per pair: the block is the only writer of the pair's state (no ping-pong needed).  A terminated pair returns at once, its
// state, iters included, untouched.  The first arg-max over valid, non-NaN scores replaces the state on a STRICTLY higher score (or,
// with Geom::kFirstRoundTakes, in the first round whatever it scores); mask and inlier count of a new best come from Geom::inlier, the
// score kernel's expression, so the count is the mask's count (no floating-point sum in this kernel); the bound from adaptive_max_iters
// with the family's sample size; iters += B.
template <typename T, typename Geom>
__global__ __launch_bounds__(kPairThreads) void pair_update_kernel(
    const T *__restrict__ matches, const T *__restrict__ models, const uint8_t *__restrict__ valid, const T *__restrict__ scores,
    const T *__restrict__ thr2, int M, int N, int B, double confidence, double eps, int max_iterations, T *__restrict__ best_score,
    T *__restrict__ best_model, uint8_t *__restrict__ best_mask, int32_t *__restrict__ best_inliers, int32_t *__restrict__ iters,
    double *__restrict__ max_iters) {
  __shared__ T s_val[kPairThreads / 64];
  __shared__ int s_idx[kPairThreads / 64];
  __shared__ int s_cnt[kPairThreads / 64];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int it = iters[p];
  if ((double)it >= max_iters[p]) return;   // this pair has terminated (uniform across the block)
  const T bs = best_score[p];
  T bv;
  int bi;
  // (its barrier comes after every thread has read iters / max_iters / best_score above: thread 0 may write them below)
  block_arg_best<T, kPairThreads, true>(scores + (size_t)p * M, valid ? valid + (size_t)p * M : nullptr, M, s_val, s_idx, bv, bi);
  const bool have = bi != 0x7fffffff;              // (a -inf score of a valid model has an index too)
  if (have && (bv > bs || (Geom::kFirstRoundTakes && it == 0))) {      // (block-uniform)
    const T *win = models + ((size_t)p * M + bi) * Geom::kModel;
    typename Geom::template Slot<T> s;
    const bool scored = Geom::prepare(win, s) == kModelScored;
    const T t2 = thr2[p];
    int cnt = 0;
    for (int n = tid; n < N; n += kPairThreads) {
      const auto x = Geom::template Point<T>::load(matches, (size_t)p * N + n);
      const bool in = scored && Geom::inlier(s, x.v, t2);
      best_mask[(size_t)p * N + n] = in;
      cnt += in;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (tid < Geom::kModel) best_model[(size_t)p * Geom::kModel + tid] = win[tid];
    if (tid == 0) {
      int inl = 0;
#pragma unroll
      for (int w = 0; w < kPairThreads / 64; ++w) inl += s_cnt[w];
      best_inliers[p] = inl;
      best_score[p] = bv;
      max_iters[p] = adaptive_max_iters(inl, N, Geom::kSample, confidence, eps, max_iterations);
    }
  }
  if (tid == 0) iters[p] = it + B;
}

// ---- K block-wide f64 sums of the refits: lane, wave butterfly, the four waves in order ---------------------------------------------
// s: shared [kPairThreads / 64][K].  block_partials_f64 leaves the wave sums there behind a barrier, block_total_f64 adds the four of
// one sum; block_sum_f64 = both for every sum -> every thread holds the K totals, and s is free again.
template <int K>
__device__ __forceinline__ void block_partials_f64(const double *v, double (*s)[K]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double w = wave_sum(v[i]);
    if (lane == 0) s[wv][i] = w;
  }
  __syncthreads();
}

template <int K>
__device__ __forceinline__ double block_total_f64(const double (*s)[K], int i) {
  double a = s[0][i];
#pragma unroll
  for (int w = 1; w < kPairThreads / 64; ++w) a += s[w][i];
  return a;
}

template <int K>
__device__ __forceinline__ void block_sum_f64(double *v, double (*s)[K]) {
  block_partials_f64<K>(v, s);
#pragma unroll
  for (int i = 0; i < K; ++i) v[i] = block_total_f64<K>(s, i);
  __syncthreads();   // (the buffer may be reused)
}

// ---- the score of ONE prepared slot over the N rows of a pair (pt = the pair's first row), by the whole block, under the scoring
// kernel's term -> the score in every thread, and through `count` (with its slots s_cnt) the number of inliers; a caller that passes
// neither pays nothing for the count: the function is forced inline, so `count` is a constant there, and term.inlier has no side
// effect, so the row loop's count is dead code.  Thread n owns rows n, n + 256, ...; sums: lane, wave butterfly, the four waves in order.
// Two barriers; s_part / s_cnt (kPairThreads / 64 entries each) are free again on return.
template <typename T, typename Geom, typename Term>
__device__ __forceinline__ T pair_block_score(const T *pt, int N, const typename Geom::template Slot<T> &s, const Term &term, T *s_part,
                                              int *s_cnt = nullptr, int *count = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  T acc = T(0);
  int cnt = 0;
  for (int n = tid; n < N; n += kPairThreads) {
    const auto x = Geom::template Point<T>::load(pt, n);
    T d2;
    const bool live = Geom::d2(s, x.v, d2);
    acc += term.contrib(d2, live);
    cnt += (live && term.inlier(d2)) ? 1 : 0;
  }
  acc = wave_sum(acc);
  if (count) cnt = wave_sum(cnt);
  if (lane == 0) {
    s_part[wv] = acc;
    if (count) s_cnt[wv] = cnt;
  }
  __syncthreads();
  T sc = s_part[0];
#pragma unroll
  for (int w = 1; w < kPairThreads / 64; ++w) sc += s_part[w];
  if (count) {
    cnt = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kPairThreads / 64; ++w) cnt += s_cnt[w];
    *count = cnt;
  }
  __syncthreads();
  return sc;
}

// ---- the polish of a pair's (best_score, best_model) behind the state step: one accept loop under a family's fit ---------------------
// One block per pair.  Every thread reads the state; behind a barrier (thread 0 writes it at the end) up to `iters` times:
//   fit(current model, candidate) -> kFitStop: nothing was fitted, the loop ends and the step is not counted; otherwise a fit has run
//   and counts, and the candidate holds its model rounded to T as the family's refit stores it.  The loop ends there on kFitInvalid
//   and on a candidate that Geom::prepare does not call scored or that holds a non-finite value (RigidGeom::prepare classifies
//   nothing, so the values are tested here; for HomographyGeom the test repeats what prepare_h has folded into the kind);
//   the candidate's score over all N rows with the scoring kernel's term (pair_block_score), so that it compares with a best_score
//   that kernel produced; it is taken only if it scores STRICTLY higher (the state step and the drivers' final refits use > too), and
//   a candidate that does not win ends the loop.
// Thread 0 then stores score and model if a candidate was taken, and adds the fits run to the pair's counter.  Nothing else of the
// state is read or written.  A latency kernel: the steps of a pair are serial, each one a few block-stride passes over rows that stay
// in L2 -- they are not staged in LDS, so there is one path for every N.  `fit` is called by every thread of the block and returns
// the same value and the same candidate in each, so every exit is block-uniform; all sums go lane, wave butterfly, the four waves in
// order: no atomics, no read-back, a repeated launch gives the same bits.
enum { kFitStop, kFitValid, kFitInvalid };

template <typename T, typename Geom, typename Term, typename Fit>
__device__ __forceinline__ void pair_polish(const T *pt, int N, int iters, const Term &term, const Fit &fit, T *s_part,
                                            T *__restrict__ best_score, T *__restrict__ best_model, int32_t *__restrict__ fit_count) {
  T bs = *best_score;
  T bm[Geom::kModel];
#pragma unroll
  for (int q = 0; q < Geom::kModel; ++q) bm[q] = best_model[q];
  __syncthreads();      // (every thread has read the state: thread 0 writes it below)
  bool taken = false;
  int fits = 0;
  for (int it = 0; it < iters; ++it) {
    T cm[Geom::kModel];
    const int fitted = fit(bm, cm);
    if (fitted == kFitStop) break;
    ++fits;
    typename Geom::template Slot<T> cs;
    bool ok = Geom::prepare(cm, cs) == kModelScored && fitted == kFitValid;
#pragma unroll
    for (int q = 0; q < Geom::kModel; ++q) ok = ok && is_finite(cm[q]);
    if (!ok) break;
    const T sc = pair_block_score<T, Geom>(pt, N, cs, term, s_part);
    if (!(sc > bs)) break;
    bs = sc;
    taken = true;
#pragma unroll
    for (int q = 0; q < Geom::kModel; ++q) bm[q] = cm[q];
  }
  if (threadIdx.x == 0) {
    if (taken) {
      *best_score = bs;
#pragma unroll
      for (int q = 0; q < Geom::kModel; ++q) best_model[q] = bm[q];
    }
    *fit_count += fits;
  }
}

}  // namespace dr
