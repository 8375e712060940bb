// K1p -- PROSAC sampler (Chum & Matas, "Matching with PROSAC", CVPR 2005) for the test-mode drivers: index sets only, drawn from the
// points in the order of their predicted inlier probability.  Where the Gumbel top-k sampler makes one Philox word and one or two
// logarithms per (hypothesis, point), a PROSAC draw needs at most k <= 8 random words whatever N is: O(B k) instead of O(B N).
//
// The sampler is stated by its mathematics.  growth[i] = T'_{k+i} is the draw number up to which the sampler works on the
// k + i best-ranked points; draw t (1-based, t = t0 + b + 1 for row b of a launch) takes
//   t <= T'_N :  n = min{ n in [k, N] : T'_n >= t };  the sample's ranks are { n - 1 } and k - 1 distinct ranks uniform in [0, n - 2]
//   t >  T'_N :  k distinct ranks uniform in [0, N - 1]
// so draw 1 is exactly the ranks 0 .. k-1 (the paper's listing starts its first draw at n = m + 1 already).  Distinct ranks come from
// Floyd's algorithm: c ranks out of a pool of s with exactly c random words and no rejection loop.
#include "dr_common.hpp"

namespace dr {

constexpr int kProsacMaxK = 8;

// compare-exchange of two registers (ascending)
__device__ __forceinline__ void prosac_cx(int &a, int &b) {
  const int lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

// One lane per (pair, hypothesis): the lanes of a wave hold consecutive draw numbers, so their binary searches walk the same lines of
// the growth table; the `order` reads are scattered 4-byte loads.  The k <= 8 ranks stay in registers: every loop over them is
// unrolled to kProsacMaxK with predicates, nothing is indexed dynamically.
// Philox4x32-7(key = seed, counter = (word / 4, b, p, 3)); word i of a draw is word i & 3 of block i >> 2.
__global__ __launch_bounds__(256) void prosac_sample_kernel(const int32_t *__restrict__ order, const int64_t *__restrict__ growth,
                                                           uint64_t seed, const uint64_t *__restrict__ seed_ptr, int64_t t0, int B,
                                                           int N, int k, int32_t *__restrict__ idx) {
  if (seed_ptr) seed = *seed_ptr;
  const int p = blockIdx.y, b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t t = t0 + (int64_t)b + 1;
  const int last = N - k;           // growth has N - k + 1 entries
  int pool = N, c = k, top = -1;    // tail: k ranks out of all N points
  if (t <= growth[last]) {          // growth regime: rank n - 1 and k - 1 ranks below it
    int lo = 0, hi = last;
    while (lo < hi) {               // smallest i with growth[i] >= t
      const int mid = (lo + hi) >> 1;
      if (growth[mid] >= t) hi = mid; else lo = mid + 1;
    }
    top = k + lo - 1;
    pool = top;
    c = k - 1;
  }
  uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (c > 0) Philox::gen(seed, 0u, (uint32_t)b, (uint32_t)p, 3u, w);
  if (c > 4) Philox::gen(seed, 1u, (uint32_t)b, (uint32_t)p, 3u, w + 4);
  // Floyd: for j = pool - c .. pool - 1 draw r in [0, j]; take j when r is already chosen, else r (bias <= (j + 1) / 2^32 per draw)
  int sel[kProsacMaxK];
#pragma unroll
  for (int i = 0; i < kProsacMaxK; ++i) sel[i] = -1;
#pragma unroll
  for (int i = 0; i < kProsacMaxK; ++i) {
    const int j = pool - c + i;
    const int r = (int)(((uint64_t)w[i] * (uint64_t)(uint32_t)(j + 1)) >> 32);
    bool dup = false;
#pragma unroll
    for (int q = 0; q < i; ++q) dup = dup || (sel[q] == r);
    if (i < c) sel[i] = dup ? j : r;
  }
  // the forced rank of the growth regime goes into the one free slot (c = k - 1 there)
#pragma unroll
  for (int i = 0; i < kProsacMaxK; ++i)
    if (top >= 0 && i == c) sel[i] = top;
  // rank -> point index; unused slots sort to the end
  const int32_t *ord = order ? order + (size_t)p * N : nullptr;
#pragma unroll
  for (int i = 0; i < kProsacMaxK; ++i) {
    int v = 0x7fffffff;
    if (i < k) v = ord ? ord[sel[i]] : sel[i];
    sel[i] = v;
  }
  // ascending point index, the contract of the index samplers: the 19-comparator network for eight keys
  prosac_cx(sel[0], sel[1]); prosac_cx(sel[2], sel[3]); prosac_cx(sel[4], sel[5]); prosac_cx(sel[6], sel[7]);
  prosac_cx(sel[0], sel[2]); prosac_cx(sel[1], sel[3]); prosac_cx(sel[4], sel[6]); prosac_cx(sel[5], sel[7]);
  prosac_cx(sel[1], sel[2]); prosac_cx(sel[5], sel[6]); prosac_cx(sel[0], sel[4]); prosac_cx(sel[3], sel[7]);
  prosac_cx(sel[1], sel[5]); prosac_cx(sel[2], sel[6]);
  prosac_cx(sel[1], sel[4]); prosac_cx(sel[3], sel[6]);
  prosac_cx(sel[2], sel[4]); prosac_cx(sel[3], sel[5]);
  prosac_cx(sel[3], sel[4]);
  int32_t *dst = idx + ((size_t)p * B + b) * k;
#pragma unroll
  for (int i = 0; i < kProsacMaxK; ++i)
    if (i < k) dst[i] = sel[i];
}

}  // namespace dr

extern "C" {

int dr_prosac_sample(const int32_t *order, const int64_t *growth, uint64_t seed, const uint64_t *seed_dev, int64_t t0, int P, int B,
                     int N, int k, int32_t *idx, void *stream) {
  DR_REQUIRE(idx && growth, "null pointer");
  DR_REQUIRE(k >= 1 && k <= dr::kProsacMaxK, "k must be in [1, 8]");
  DR_REQUIRE(N >= k, "N must be at least k");
  DR_REQUIRE(P >= 1 && B >= 1 && P <= 65535, "bad sizes");
  DR_REQUIRE(t0 >= 0, "t0 must not be negative");
  return dr::launch("prosac_sample_kernel", dr::prosac_sample_kernel, dim3((B + 255) / 256, P), 256, stream, order, growth, seed,
                    seed_dev, t0, B, N, k, idx);
}

}  // extern "C"
