// k-nearest-neighbour search and the similarity-weighted vote (k-NN / retrieval evaluation of a frozen tower).
//
// avid_knn_search: for nq queries against a gallery [N][D], sim[n][q] = <gallery[n], query[q]> from one fp32-MFMA GEMM
// (sim_gemm_nt, the cache-resident [N][nq] slab of the CMA search), then the best K = k (+ 1 with `exclude`) rows per
// query in the order (similarity desc, gallery index asc), with their scores.  The selection is the streaming one of
// cma_topk.hip (topk_select.h: lane maxima -> threshold -> candidate lists for N >= 4096; per-lane insertion lists below
// that and as the fallback of a batch whose candidate list overflowed); what differs is the end of it: the queries are
// not rows of the gallery, nothing is assumed to be "self", the rows keep their rank order and their scores.
// `exclude[q]` names a gallery row that must not be returned (leave-one-out): K = k + 1 rows are selected, the named
// row is removed where it is among them, the last one otherwise.
//
// avid_knn_vote: one wave per query.  scores[q][c] = sum over ranks j (in rank order) of exp(sim[q][j] / T) with
// label(idx[q][j]) == c, the five best classes, and the first rank whose label is the query's.
#include <math.h>

#include "common.h"
#include "topk_select.h"

namespace avid {

constexpr int VOTE_MAX_CLASSES = 8192;   // double accumulators in LDS: 64 KiB

// chosen rows of one query in rank order [K] -> out rows [k]: position p is skipped (p = the excluded row's position, K - 1
// when it is not among them, K (nothing) without an exclude vector).  Called by all 256 threads, after a barrier.
__device__ __forceinline__ void knn_emit(const int* chosen_i, const float* chosen_v, int* pos, int K, int k,
                                         const int32_t* __restrict__ exclude, int q, int32_t* __restrict__ out_idx,
                                         float* __restrict__ out_sim) {
  const int t = threadIdx.x;
  if (t == 0) *pos = exclude ? K - 1 : K;
  __syncthreads();
  if (exclude && t < K && chosen_i[t] == exclude[q]) *pos = t;     // gallery indices are distinct: at most one writer
  __syncthreads();
  if (t < k) {
    const int src = t < *pos ? t : t + 1;
    out_idx[(long long)q * k + t] = chosen_i[src];
    out_sim[(long long)q * k + t] = chosen_v[src];
  }
}

// one block per query: rank the candidates of the threshold filter by (value desc, index asc), keep ranks 0..K-1.
// A list that overflowed raises the flag instead (the exact scan then redoes the batch).
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ cval, const int* __restrict__ cidx,
                                                         const int* __restrict__ count, int K, int k,
                                                         const int32_t* __restrict__ exclude, int* __restrict__ flag,
                                                         int32_t* __restrict__ out_idx, float* __restrict__ out_sim) {
  __shared__ float sv[TK_CAP];
  __shared__ int si[TK_CAP];
  __shared__ int chosen_i[TK_MAX + 1];
  __shared__ float chosen_v[TK_MAX + 1];
  __shared__ int pos;
  const int q = blockIdx.x;
  const int n = count[q];
  if (n > TK_CAP || n < K) {      // (n < K cannot happen: K lane maxima reach the threshold)
    if (threadIdx.x == 0) atomicOr(flag, 1);
    return;
  }
  for (int c = threadIdx.x; c < n; c += 256) {
    sv[c] = cval[(long long)q * TK_CAP + c];
    si[c] = cidx[(long long)q * TK_CAP + c];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < n; c += 256) {
    const float v = sv[c];
    const int i = si[c];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += better(sv[j], si[j], v, i) ? 1 : 0;
    if (rank < K) {
      chosen_i[rank] = i;
      chosen_v[rank] = v;
    }
  }
  __syncthreads();
  knn_emit(chosen_i, chosen_v, &pos, K, k, exclude, q, out_idx, out_sim);
}

// one block per query: K rounds of block-wide arg-best over the P * K candidates of the per-lane lists (topk_scan_kernel).
// With `flag`: the fallback of the threshold filter — returns at once when no list of the batch overflowed.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ pval, const int* __restrict__ pidx, int P,
                                                        int nq, int K, int k, const int32_t* __restrict__ exclude,
                                                        int32_t* __restrict__ out_idx, float* __restrict__ out_sim,
                                                        const int* __restrict__ flag, int32_t* __restrict__ fallbacks) {
  if (flag && *flag == 0) return;
  if (flag && fallbacks && blockIdx.x == 0 && threadIdx.x == 0) *fallbacks += 1;   // this batch overflowed its filter
  __shared__ float sv[256];
  __shared__ int si[256], sp[256];
  __shared__ int chosen_i[TK_MAX + 1];
  __shared__ float chosen_v[TK_MAX + 1];
  __shared__ int pos;
  __shared__ unsigned char taken[TK_SPLITS * 4 * TK_MAX];
  const int q = blockIdx.x;
  const int ncand = P * K;
  for (int c = threadIdx.x; c < ncand; c += 256) taken[c] = 0;
  __syncthreads();
  for (int round = 0; round < K; ++round) {
    float bv = -INFINITY;
    int bi = 0x7fffffff, bp = -1;
    for (int c = threadIdx.x; c < ncand; c += 256) {
      if (taken[c]) continue;
      const int pslot = c / K, kk = c - pslot * K;
      const long long o = ((long long)pslot * nq + q) * K + kk;
      const float v = pval[o];
      const int i = pidx[o];
      if (bp < 0 || better(v, i, bv, bi)) {
        bv = v; bi = i; bp = c;
      }
    }
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi; sp[threadIdx.x] = bp;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (threadIdx.x < s) {
        const int o = threadIdx.x + s;
        if (sp[o] >= 0 && (sp[threadIdx.x] < 0 || better(sv[o], si[o], sv[threadIdx.x], si[threadIdx.x]))) {
          sv[threadIdx.x] = sv[o]; si[threadIdx.x] = si[o]; sp[threadIdx.x] = sp[o];
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      chosen_i[round] = si[0];
      chosen_v[round] = sv[0];
      if (sp[0] >= 0) taken[sp[0]] = 1;
    }
    __syncthreads();
  }
  knn_emit(chosen_i, chosen_v, &pos, K, k, exclude, q, out_idx, out_sim);
}

// grid = nq, block = 64 (one wave per query); dynamic LDS: double acc[n_classes].
__global__ __launch_bounds__(64) void knn_vote_kernel(int k, const int32_t* __restrict__ idx, const float* __restrict__ sim,
                                                      const int32_t* __restrict__ gallery_labels, long long N, int n_classes,
                                                      float inv_T, const int32_t* __restrict__ query_labels,
                                                      float* __restrict__ scores, int32_t* __restrict__ pred5,
                                                      int32_t* __restrict__ first_match) {
  extern __shared__ __attribute__((aligned(16))) double acc[];
  __shared__ int lab[TK_MAX];
  __shared__ double term[TK_MAX];
  const int q = blockIdx.x, lane = threadIdx.x;
  for (int c = lane; c < n_classes; c += 64) acc[c] = 0.0;
  if (lane < k) {
    const int i = idx[(long long)q * k + lane];
    int c = -1;                                            // a row or a label out of range takes no part
    if (i >= 0 && i < N) c = gallery_labels[i];
    lab[lane] = c >= 0 && c < n_classes ? c : -1;
    // the product and exp in double: at |x| <= 14.3 the fp32 rounding of x alone is 8.5e-7 of the term
    term[lane] = exp((double)sim[(long long)q * k + lane] * (double)inv_T);
  }
  __syncthreads();
  if (lane == 0) {                                         // rank order: deterministic
    const int ql = query_labels ? query_labels[q] : -1;
    int first = k;
    for (int j = 0; j < k; ++j) {
      const int c = lab[j];
      if (c < 0) continue;
      acc[c] += term[j];
      if (query_labels && c == ql && first == k) first = j;
    }
    if (query_labels) first_match[q] = first;
  }
  __syncthreads();
  for (int c = lane; c < n_classes; c += 64) scores[(long long)q * n_classes + c] = (float)acc[c];
  // five rounds of wave arg-best by (score desc, class asc) over the fp32 scores, as they were written
  int p0 = -1, p1 = -1, p2 = -1, p3 = -1;
  for (int r = 0; r < 5; ++r) {
    float bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int c = lane; c < n_classes; c += 64) {
      if (c == p0 || c == p1 || c == p2 || c == p3) continue;
      const float v = (float)acc[c];
      if (bc == 0x7fffffff || better(v, c, bv, bc)) {
        bv = v; bc = c;
      }
    }
    for (int s = 32; s > 0; s >>= 1) {
      const float ov = __shfl_xor(bv, s, 64);
      const int oc = __shfl_xor(bc, s, 64);
      if (oc != 0x7fffffff && (bc == 0x7fffffff || better(ov, oc, bv, bc))) {
        bv = ov; bc = oc;
      }
    }
    const int pick = bc == 0x7fffffff ? -1 : bc;
    if (lane == 0) pred5[(long long)q * 5 + r] = pick;
    p3 = p2; p2 = p1; p1 = p0; p0 = pick;
  }
}

}  // namespace avid

using namespace avid;

static int knn_scan_splits(int64_t N) {
  int s = (int)(N / 2048);
  if (s < 1) s = 1;
  return s > TK_SPLITS ? TK_SPLITS : s;
}

// threshold filter: row splits (0 = gallery too small for it: P = 4 * splits lane maxima must cover K)
static int knn_filter_splits(int64_t N) {
  if (N < 4096) return 0;
  const int s = (int)(N / 256);
  return s > TK_SPLITS ? TK_SPLITS : s;
}

// Layout of the workspace, in 4-byte words: score slab [N][nq] | list values [P][nq][K] | list indices [P][nq][K] |
// lane maxima [FP][nq] | thresholds [nq] | counters [nq] | flag (64) | candidate values [nq][CAP] | candidate indices
static size_t knn_words(int64_t N, int nq, int K) {
  const size_t P = (size_t)knn_scan_splits(N) * 4, FS = (size_t)knn_filter_splits(N);
  size_t w = (size_t)N * nq + 2 * P * nq * K;
  if (FS) w += FS * 4 * nq + 2 * (size_t)nq + 64 + 2 * (size_t)nq * TK_CAP;
  return w;
}

extern "C" size_t avid_knn_workspace_bytes(int64_t N, int nq, int k) {
  if (N < 64 || N >= (1ll << 31) || nq <= 0 || nq % 64 || k <= 0 || k > TK_MAX) return 0;
  const int K = k < TK_MAX ? k + 1 : k;       // room for the extra row of an exclude vector
  return 4 * knn_words(N, nq, K) + 256;
}

extern "C" int avid_knn_search(int64_t N, int D, const float* gallery, const float* queries, int nq, int k,
                               const int32_t* exclude, int32_t* out_idx, float* out_sim, int32_t* fallbacks, void* ws,
                               size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(gallery && queries && out_idx && out_sim && ws, AVID_E_BADARG, "knn_search: null pointer");
  AVID_REQUIRE(D > 0 && D % 32 == 0 && nq > 0 && nq % 64 == 0, AVID_E_UNSUPPORTED,
               "knn_search: D %% 32 and nq %% 64 required (D=%d nq=%d)", D, nq);
  AVID_REQUIRE(N >= 64 && N < (1ll << 31), AVID_E_UNSUPPORTED, "knn_search: the gallery needs 64 <= N < 2^31 rows (N=%lld)",
               (long long)N);
  const int K = k + (exclude ? 1 : 0);
  AVID_REQUIRE(k >= 1 && K <= TK_MAX, AVID_E_UNSUPPORTED, "knn_search: k%s must be in [1, %d] (k=%d)",
               exclude ? " + 1 (exclude)" : "", TK_MAX, k);
  AVID_REQUIRE(ws_bytes >= avid_knn_workspace_bytes(N, nq, k), AVID_E_BADARG, "knn_search: workspace too small (%zu < %zu)",
               ws_bytes, avid_knn_workspace_bytes(N, nq, k));
  hipStream_t s = (hipStream_t)stream;
  const int S = knn_scan_splits(N), P = S * 4;
  float* sim = static_cast<float*>(ws);
  float* pval = sim + (size_t)N * nq;
  int* pidx = reinterpret_cast<int*>(pval + (size_t)P * nq * K);
  int rc = sim_gemm_nt(gallery, queries, sim, nullptr, 0, N, nq, D, s);
  if (rc) return rc;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(topk_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)((sizeof(float) + sizeof(int)) * 4 * TK_MAX * 64));
    attr_set = true;
  }
  const int* flag = nullptr;
  const int FS = knn_filter_splits(N);
  if (FS) {
    float* pmax = reinterpret_cast<float*>(pidx + (size_t)P * nq * K);
    float* thr = pmax + (size_t)FS * 4 * nq;
    int* count = reinterpret_cast<int*>(thr + nq);
    int* fl = count + nq;
    float* cval = reinterpret_cast<float*>(fl + 64);
    int* cidx = reinterpret_cast<int*>(cval + (size_t)nq * TK_CAP);
    hipLaunchKernelGGL(topk_max_kernel, dim3(nq / 64, FS), dim3(256), 0, s, sim, (long long)N, nq, pmax);
    hipLaunchKernelGGL(topk_thresh_kernel, dim3(nq), dim3(256), 0, s, pmax, FS * 4, nq, K, thr, count, fl);
    hipLaunchKernelGGL(topk_collect_kernel, dim3(nq / 64, FS), dim3(256), 0, s, sim, (long long)N, nq, thr, count, cval,
                       cidx);
    hipLaunchKernelGGL(knn_select_kernel, dim3(nq), dim3(256), 0, s, cval, cidx, count, K, k, exclude, fl, out_idx, out_sim);
    rc = check_launch("knn_filter");
    if (rc) return rc;
    flag = fl;
  }
  const size_t lds = (sizeof(float) + sizeof(int)) * 4 * K * 64;
  hipLaunchKernelGGL(topk_scan_kernel, dim3(nq / 64, S), dim3(256), lds, s, sim, (long long)N, nq, K, pval, pidx, flag);
  rc = check_launch("knn_scan");
  if (rc) return rc;
  hipLaunchKernelGGL(knn_merge_kernel, dim3(nq), dim3(256), 0, s, pval, pidx, P, nq, K, k, exclude, out_idx, out_sim, flag,
                     fallbacks);
  return check_launch("knn_merge");
}

extern "C" int avid_knn_vote(int nq, int k, const int32_t* idx, const float* sim, const int32_t* gallery_labels, int64_t N,
                             int n_classes, float inv_T, const int32_t* query_labels, float* scores, int32_t* pred5,
                             int32_t* first_match, avid_stream_t stream) {
  AVID_REQUIRE(idx && sim && gallery_labels && scores && pred5, AVID_E_BADARG, "knn_vote: null pointer");
  AVID_REQUIRE(!query_labels || first_match, AVID_E_BADARG, "knn_vote: query labels need a first_match output");
  AVID_REQUIRE(nq > 0 && N > 0 && N < (1ll << 31) && inv_T == inv_T, AVID_E_BADARG, "knn_vote: bad argument (nq=%d N=%lld)", nq,
               (long long)N);
  AVID_REQUIRE(k >= 1 && k <= TK_MAX, AVID_E_UNSUPPORTED, "knn_vote: k must be in [1, %d] (k=%d)", TK_MAX, k);
  AVID_REQUIRE(n_classes >= 1 && n_classes <= VOTE_MAX_CLASSES, AVID_E_UNSUPPORTED,
               "knn_vote: n_classes must be in [1, %d] (n_classes=%d)", VOTE_MAX_CLASSES, n_classes);
  hipLaunchKernelGGL(knn_vote_kernel, dim3(nq), dim3(64), sizeof(double) * n_classes, (hipStream_t)stream, k, idx, sim,
                     gallery_labels, (long long)N, n_classes, inv_T, query_labels, scores, pred5, first_match);
  return check_launch("knn_vote");
}
