// K4m -- two-view MAGSAC++ scoring on the Sampson distance: scores [P,M] and, optionally, inlier counts [P,M]; no mask
// stream.  dr_ransac_update (K6) takes the scores as it takes K4's and recomputes the winner's mask from the matches.
//
// Mapping: K4's skeleton.  One block = (pair p, tile of 32 model slots); a lane owns 8 CONSECUTIVE points of a 2048-point chunk in VGPRs
// and the block walks ALL chunks of the row itself, so a (pair, model) is owned by one block.  The model index is wave-uniform: the nine
// coefficients arrive through the scalar cache.  f32 evaluates the Sampson part two points at a time (v_pk_fma_f32), as K4's fast
// kernels do (sampson_d2_pair of ransac_device.hpp, theirs).  One compare, s < 1, serves the term and the count.  Slots the solver marked
// invalid are never evaluated (score exactly 0, count 0); a non-finite or all-zero model scores NaN (count 0) (model_kind); the blocks
// of a gated pair return at once.
// Rows of at most 256 points take a wave per model (1, 2 or 4 consecutive points per lane), where the first mapping would idle lanes.
// Reduction order, fixed: a lane's points in order, the DPP wave tree, the chunks in order onto the wave's LDS partial, the four waves in
// order.  No atomics, no [P,M,N] tensor: a repeated launch gives the same bits.
#include "magsac_device.hpp"

namespace dr {

constexpr int kMgThreads = 256, kMgPts = 8, kMgChunk = kMgThreads * kMgPts, kMgTile = 32;
constexpr int kMgWaveMaxN = 256, kMgWaves = 4, kMgPerWave = 4, kMgWaveTile = kMgWaves * kMgPerWave;

// d2 of the lane's 8 points under model m (wave-uniform)
__device__ __forceinline__ void magsac_d2_8(const float (&x1)[kMgPts], const float (&y1)[kMgPts], const float (&x2)[kMgPts],
                                            const float (&y2)[kMgPts], const float (&m)[9], float (&d2)[kMgPts]) {
  v2f ms[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) ms[q] = splat(m[q]);
#pragma unroll
  for (int j = 0; j < kMgPts; j += 2) {
    const v2f d = sampson_d2_pair((v2f){x1[j], x1[j + 1]}, (v2f){y1[j], y1[j + 1]}, (v2f){x2[j], x2[j + 1]}, (v2f){y2[j], y2[j + 1]}, ms);
    d2[j] = d[0];
    d2[j + 1] = d[1];
  }
}
__device__ __forceinline__ void magsac_d2_8(const double (&x1)[kMgPts], const double (&y1)[kMgPts], const double (&x2)[kMgPts],
                                            const double (&y2)[kMgPts], const double (&m)[9], double (&d2)[kMgPts]) {
#pragma unroll
  for (int j = 0; j < kMgPts; ++j) d2[j] = sampson_d2<double>(m, x1[j], y1[j], x2[j], y2[j]);
}

template <typename T>
__global__ __launch_bounds__(kMgThreads) void magsac_score_kernel(const T *__restrict__ matches, const T *__restrict__ models,
                                                                  const uint8_t *__restrict__ valid, const T *__restrict__ thr, int M,
                                                                  int N, T *__restrict__ scores, int32_t *__restrict__ inliers,
                                                                  PairGate gate) {
  __shared__ T part[kMgThreads / kWave][kMgTile];
  __shared__ int pcnt[kMgThreads / kWave][kMgTile];
  __shared__ int kind[kMgTile];
  const int p = blockIdx.y, m0 = blockIdx.x * kMgTile;
  if (gate.closed(p)) return;   // a terminated pair of a multi-round call (block-uniform): its outputs keep their contents
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int mcount = min(kMgTile, M - m0);
  const T *mt = matches + (size_t)p * N * 4;
  const T *md = models + ((size_t)p * M + m0) * 9;
  const Magsac4Term<T> term(thr[p]);
  if (tid < (kMgThreads / kWave) * kMgTile) {
    (&part[0][0])[tid] = T(0);
    (&pcnt[0][0])[tid] = 0;
  }
  if (tid < mcount) kind[tid] = model_kind<T>(md + tid * 9, !valid || valid[(size_t)p * M + m0 + tid] != 0);
  __syncthreads();
  for (int c0 = 0; c0 < N; c0 += kMgChunk) {
    const int n0 = c0 + tid * kMgPts;
    const int nvalid = min(kMgPts, max(0, N - n0));
    T x1[kMgPts], y1[kMgPts], x2[kMgPts], y2[kMgPts];
#pragma unroll
    for (int j = 0; j < kMgPts; ++j) {
      x1[j] = y1[j] = x2[j] = y2[j] = T(0);   // a padding point: excluded below by j < nvalid
      if (j < nvalid) {
        if constexpr (sizeof(T) == 4) {
          const float4 v = reinterpret_cast<const float4 *>(mt)[n0 + j];
          x1[j] = v.x; y1[j] = v.y; x2[j] = v.z; y2[j] = v.w;
        } else {
          const T *q = mt + 4 * (size_t)(n0 + j);
          x1[j] = q[0]; y1[j] = q[1]; x2[j] = q[2]; y2[j] = q[3];
        }
      }
    }
#pragma unroll 1
    for (int ml = 0; ml < mcount; ++ml) {
      if (__builtin_amdgcn_readfirstlane(kind[ml]) != kModelScored) continue;   // block-uniform
      T m[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) m[q] = md[ml * 9 + q];
      T d2[kMgPts];
      magsac_d2_8(x1, y1, x2, y2, m, d2);
      T acc = T(0);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < kMgPts; ++j) {
        const T s = term.ratio(d2[j]);
        const bool in = (j < nvalid) && term.inlier(s);
        acc += in ? term.gain(s) : T(0);
        cnt += in;
      }
      acc = wave_sum_lane63(acc);
      if (inliers) cnt = wave_sum_lane63(cnt);
      if (lane == 63) {   // the wave's own LDS words: the chunks accumulate in order
        part[wv][ml] += acc;
        pcnt[wv][ml] += cnt;
      }
    }
  }
  __syncthreads();
  if (tid < mcount) {
    const int k = kind[tid];
    const T v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const size_t slot = (size_t)p * M + m0 + tid;
    scores[slot] = k == kModelScored ? v : (k == kModelNan ? T(NAN) : T(0));
    if (inliers) inliers[slot] = k == kModelScored ? pcnt[0][tid] + pcnt[1][tid] + pcnt[2][tid] + pcnt[3][tid] : 0;
  }
}

// short rows: a wave per model, kPtsS consecutive points per lane (64 kPtsS >= N)
template <typename T, int kPtsS>
__global__ __launch_bounds__(kMgWaves * 64) void magsac_score_wave_kernel(const T *__restrict__ matches, const T *__restrict__ models,
                                                                          const uint8_t *__restrict__ valid, const T *__restrict__ thr,
                                                                          int M, int N, T *__restrict__ scores,
                                                                          int32_t *__restrict__ inliers, PairGate gate) {
  const int p = blockIdx.y;
  if (gate.closed(p)) return;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const T *mt = matches + (size_t)p * N * 4;
  const Magsac4Term<T> term(thr[p]);
  const int n0 = lane * kPtsS;
  const int nvalid = min(kPtsS, max(0, N - n0));
  T x1[kPtsS], y1[kPtsS], x2[kPtsS], y2[kPtsS];
#pragma unroll
  for (int j = 0; j < kPtsS; ++j) {
    x1[j] = y1[j] = x2[j] = y2[j] = T(0);
    if (j < nvalid) {
      const T *q = mt + 4 * (size_t)(n0 + j);
      x1[j] = q[0]; y1[j] = q[1]; x2[j] = q[2]; y2[j] = q[3];
    }
  }
#pragma unroll 1
  for (int r = 0; r < kMgPerWave; ++r) {
    const int mi = blockIdx.x * kMgWaveTile + r * kMgWaves + wv;   // wave-uniform
    if (mi >= M) break;
    const size_t slot = (size_t)p * M + mi;
    T m[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] = models[slot * 9 + q];
    const int k = model_kind<T>(m, !valid || valid[slot] != 0);
    T acc = T(0);
    int cnt = 0;
    if (k == kModelScored) {
#pragma unroll
      for (int j = 0; j < kPtsS; ++j) {
        const T s = term.ratio(sampson_d2<T>(m, x1[j], y1[j], x2[j], y2[j]));
        const bool in = (j < nvalid) && term.inlier(s);
        acc += in ? term.gain(s) : T(0);
        cnt += in;
      }
    }
    acc = wave_sum_lane63(acc);
    if (inliers) cnt = wave_sum_lane63(cnt);
    if (lane == 63) {
      scores[slot] = k == kModelScored ? acc : (k == kModelNan ? T(NAN) : T(0));
      if (inliers) inliers[slot] = cnt;
    }
  }
}

template <typename T>
int magsac_score_launch(const T *matches, const T *models, const uint8_t *valid, const T *thr, int P, int M, int N, T *scores,
                        int32_t *inliers, PairGate gate, void *stream) {
  if (N <= kMgWaveMaxN) {
    const dim3 g((M + kMgWaveTile - 1) / kMgWaveTile, P);
    const auto kernel = N <= 64 ? magsac_score_wave_kernel<T, 1> : N <= 128 ? magsac_score_wave_kernel<T, 2> : magsac_score_wave_kernel<T, 4>;
    return launch("magsac_score_wave_kernel", kernel, g, kMgWaves * 64, stream, matches, models, valid, thr, M, N, scores, inliers, gate);
  }
  return launch("magsac_score_kernel", magsac_score_kernel<T>, dim3((M + kMgTile - 1) / kMgTile, P), kMgThreads, stream, matches, models,
                valid, thr, M, N, scores, inliers, gate);
}

}  // namespace dr

extern "C" {

#define DR_OP(sfx, T)                                                                                                              \
  int dr_magsac_score_##sfx(const T *matches, const T *models, const uint8_t *valid, const T *thr, int P, int M, int N, T *scores,  \
                            int32_t *inliers, const int32_t *gate_iters, const double *gate_max_iters, void *stream) {              \
    DR_REQUIRE(P > 0 && M > 0 && N > 0 && P <= 65535, "bad sizes");                                                                 \
    DR_REQUIRE(matches && models && thr && scores, "null pointer");                                                                 \
    DR_REQUIRE((gate_iters == nullptr) == (gate_max_iters == nullptr), "gate: both pointers or neither");                           \
    dr::PairGate gate;                                                                                                              \
    gate.iters = gate_iters;                                                                                                        \
    gate.max_iters = gate_max_iters;                                                                                                \
    return dr::magsac_score_launch<T>(matches, models, valid, thr, P, M, N, scores, inliers, gate, stream);                         \
  }
DR_F32_F64(DR_OP)
#undef DR_OP

}  // extern "C"
