// Streaming top-K selection over a [N][nq] score slab: the pieces avid_cma_topk (cma_topk.hip) and avid_knn_search
// (knn.hip) share.  Lanes = 64 consecutive queries, so a score row is one coalesced 256-B read.  Ties are ordered
// (value desc, index asc).  The kernels are `static`: each of the two files launches its own copy.
#pragma once
#include <math.h>

#include "common.h"

namespace avid {

constexpr int TK_MAX = 64;       // pos_k + 1 <= 64
constexpr int TK_SPLITS = 64;    // row splits per query group

__device__ __forceinline__ bool better(float v, int i, float ev, int ei) { return v > ev || (v == ev && i < ei); }

constexpr int TK_CAP = 1024;     // candidate slots per query of the threshold filter

// grid = (nq / 64, splits); block = 256 = 4 waves; wave w takes rows r0 + w, r0 + w + 4, ... of its split.
// pmax[(split * 4 + wave)][nq]
static __global__ __launch_bounds__(256) void topk_max_kernel(const float* __restrict__ sim, long long N, int nq,
                                                       float* __restrict__ pmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane;
  const long long per = (N + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * per;
  const long long r1 = r0 + per < N ? r0 + per : N;
  float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
  long long r = r0 + wave;
  for (; r + 12 < r1; r += 16) {
    m0 = fmaxf(m0, sim[r * nq + q]);
    m1 = fmaxf(m1, sim[(r + 4) * nq + q]);
    m2 = fmaxf(m2, sim[(r + 8) * nq + q]);
    m3 = fmaxf(m3, sim[(r + 12) * nq + q]);
  }
  for (; r < r1; r += 4) m0 = fmaxf(m0, sim[r * nq + q]);
  pmax[((long long)blockIdx.y * 4 + wave) * nq + q] = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
}

// one block (256 threads) per query: T = K-th largest of its P <= 256 lane maxima; resets the query's
// candidate counter (and, block 0, the overflow flag)
static __global__ __launch_bounds__(256) void topk_thresh_kernel(const float* __restrict__ pmax, int P, int nq, int K,
                                                          float* __restrict__ thr, int* __restrict__ count,
                                                          int* __restrict__ flag) {
  __shared__ float v[256];
  const int q = blockIdx.x, i = threadIdx.x;
  v[i] = i < P ? pmax[(long long)i * nq + q] : -INFINITY;
  __syncthreads();
  if (i < P) {
    const float vi = v[i];
    int rank = 0;
    for (int j = 0; j < P; ++j) rank += (v[j] > vi || (v[j] == vi && j < i)) ? 1 : 0;
    if (rank == K - 1) thr[q] = vi;
  }
  if (i == 0) count[q] = 0;
  if (q == 0 && i == 0) *flag = 0;
}

// same traversal as topk_max_kernel: rows with score >= T[q] go to the query's candidate list
static __global__ __launch_bounds__(256) void topk_collect_kernel(const float* __restrict__ sim, long long N, int nq,
                                                           const float* __restrict__ thr, int* __restrict__ count,
                                                           float* __restrict__ cval, int* __restrict__ cidx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane;
  const long long per = (N + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * per;
  const long long r1 = r0 + per < N ? r0 + per : N;
  const float t = thr[q];
  auto take = [&](float v, long long r) {
    if (v >= t) {
      const int slot = atomicAdd(&count[q], 1);
      if (slot < TK_CAP) {
        cval[(long long)q * TK_CAP + slot] = v;
        cidx[(long long)q * TK_CAP + slot] = (int)r;
      }
    }
  };
  long long r = r0 + wave;
  for (; r + 12 < r1; r += 16) {
    const float v0 = sim[r * nq + q], v1 = sim[(r + 4) * nq + q], v2 = sim[(r + 8) * nq + q],
                v3 = sim[(r + 12) * nq + q];
    if (__any((v0 >= t) | (v1 >= t) | (v2 >= t) | (v3 >= t))) {
      take(v0, r); take(v1, r + 4); take(v2, r + 8); take(v3, r + 12);
    }
  }
  for (; r < r1; r += 4) take(sim[r * nq + q], r);
}

// grid = (nq / 64, TK_SPLITS); block = 256 = 4 waves; wave w scans rows r0 + w, r0 + w + 4, ...
// (`flag`: when given and clear, the threshold filter above already produced this batch — nothing to do)
static __global__ __launch_bounds__(256) void topk_scan_kernel(const float* __restrict__ sim, long long N, int nq, int K,
                                                        float* __restrict__ pval, int* __restrict__ pidx,
                                                        const int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (flag && *flag == 0) return;
  float* lv = smem;                                         // [4][K][64]
  int* li = reinterpret_cast<int*>(smem + 4 * K * 64);      // [4][K][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane;
  float* mv = lv + wave * K * 64 + lane;
  int* mi = li + wave * K * 64 + lane;
  for (int k = 0; k < K; ++k) {
    mv[k * 64] = -INFINITY;
    mi[k * 64] = 0x7fffffff;
  }
  const long long per = (N + gridDim.y - 1) / gridDim.y;
  const long long r0 = (long long)blockIdx.y * per;
  const long long r1 = r0 + per < N ? r0 + per : N;
  float thr_v = -INFINITY;   // current K-th best of this lane's list
  int thr_i = 0x7fffffff;
  for (long long r = r0 + wave; r < r1; r += 4) {
    const float v = sim[r * nq + q];
    const int idx = (int)r;
    if (better(v, idx, thr_v, thr_i)) {
      // insertion into the descending list (position K-1 is evicted)
      int k = K - 1;
      while (k > 0 && better(v, idx, mv[(k - 1) * 64], mi[(k - 1) * 64])) {
        mv[k * 64] = mv[(k - 1) * 64];
        mi[k * 64] = mi[(k - 1) * 64];
        --k;
      }
      mv[k * 64] = v;
      mi[k * 64] = idx;
      thr_v = mv[(K - 1) * 64];
      thr_i = mi[(K - 1) * 64];
    }
  }
  const long long slot = ((long long)blockIdx.y * 4 + wave) * nq + q;   // [P][nq][K]
  for (int k = 0; k < K; ++k) {
    pval[slot * K + k] = mv[k * 64];
    pidx[slot * K + k] = mi[k * 64];
  }
}

}  // namespace avid
