// Multi-label ranking metrics on the device: per-class average precision and ROC-AUC of scores [N][C] against targets [N][C]
// (scikit-learn's average_precision_score / roc_auc_score per column; the reference has no multi-label evaluation).
//
// Counting forms, positives being t >= 0.5, ties handled, no sort:
//   ap_c  = (1 / P) sum over positives i, in ascending sample index, of TP_i / (TP_i + FP_i)     (double)
//           TP_i / FP_i = the positives / negatives with score >= score_i
//   auc_c = U2 / (2 P Nn),  U2 = sum over positives of 2 #{neg < s_i} + #{neg == s_i}             (int64, one double division)
// The work is P x N compares per class, and P is small for almost every class of a tagging set (AudioSet: ~2 of 527 per clip).
//
// Four launches, all integer counts reduced through registers and LDS, no atomics on any result:
//   rank_transpose_kernel   [N][C] x 2 -> st [C][N] of (score if negative else NaN, score if positive else NaN): one float2
//                           per sample carries the score and the positive bit, and every later compare is a plain float
//                           compare that is false for the other kind; a positive's first half is the NaN of payload 1
//                           (RK_POS_BITS), so that the positive bit survives a NaN score, which makes both halves NaN
//   rank_count_kernel       one workgroup per class: P, the NaN-score flag, n_pos
//   rank_pairs_kernel       grid (class, z): workgroup z takes the class's rounds z, z + Z, ...; a round is RK_SLAB positives in
//                           ascending sample index, compacted into LDS (ballot prefix over the class's row), then the row is
//                           staged through LDS in tiles that every lane reads as broadcasts.  Lanes are (positive, N-slice)
//                           pairs: slice s of S = 256 / P' (P' the round's positives) takes the samples s, s + S, ... of a
//                           tile, the slices' counts meet in LDS.  The round's terms are summed in index order by one thread.
//                           (A dense class — P = N / 2 — spreads over up to RK_MAX_Z workgroups; almost every class is one round.)
//   rank_final_kernel       one thread per class: the rounds' sums in order, the two divisions, the NaN cases
#include <math.h>

#include "common.h"

namespace avid {

constexpr int RK_THREADS = 256;
constexpr int RK_SLAB = RK_THREADS;               // positives per round: at most one per lane
constexpr int RK_TILE = 1024;                     // samples staged per tile
constexpr int RK_MAX_Z = 64;
constexpr unsigned RK_POS_BITS = 0x7fc00001u;     // the "not a negative" half of a positive sample (never computed with)

struct RankWs {
  float2* st;
  int *P, *bad;
  double* part_ap;
  long long* part_u2;
  int R;
  size_t bytes;
};

static size_t rk_align(size_t n) { return (n + 255) / 256 * 256; }

static RankWs rank_ws(void* ws, int64_t N, int C) {
  RankWs w;
  char* p = static_cast<char*>(ws);
  w.R = (int)ceil_div(N, RK_SLAB);
  size_t off = 0;
  w.st = reinterpret_cast<float2*>(p + off);
  off += rk_align(sizeof(float2) * (size_t)N * C);
  w.P = reinterpret_cast<int*>(p + off);
  off += rk_align(sizeof(int) * (size_t)C);
  w.bad = reinterpret_cast<int*>(p + off);
  off += rk_align(sizeof(int) * (size_t)C);
  w.part_ap = reinterpret_cast<double*>(p + off);
  off += rk_align(sizeof(double) * (size_t)C * w.R);
  w.part_u2 = reinterpret_cast<long long*>(p + off);
  off += rk_align(sizeof(long long) * (size_t)C * w.R);
  w.bytes = off;
  return w;
}

static bool rank_supported(int64_t N, int C) { return N >= 1 && C >= 1 && N < (1ll << 31) - RK_TILE && C <= 65535 * 32; }

__global__ __launch_bounds__(256) void rank_transpose_kernel(long long N, int C, const float* __restrict__ scores,
                                                             const float* __restrict__ targets, float2* __restrict__ st) {
  __shared__ float2 tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long long n0 = (long long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const long long n = n0 + r;
    const int c = c0 + tx;
    if (n < N && c < C) {
      const float s = scores[n * C + c];
      tile[r][tx] = targets[n * C + c] >= 0.5f ? make_float2(__uint_as_float(RK_POS_BITS), s) : make_float2(s, NAN);
    }
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r;
    const long long n = n0 + tx;
    if (n < N && c < C) st[(long long)c * N + n] = tile[tx][r];
  }
}

__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(long long N, const float2* __restrict__ st, int* __restrict__ P,
                                                                int* __restrict__ bad, long long* __restrict__ n_pos,
                                                                int* __restrict__ err) {
  __shared__ int s_p[RK_THREADS / 64], s_b[RK_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float2* row = st + (long long)c * N;
  int p = 0, b = 0;
  for (long long n = tid; n < N; n += RK_THREADS) {
    const float2 e = row[n];
    const bool pos = __float_as_uint(e.x) == RK_POS_BITS;
    p += pos ? 1 : 0;
    b |= (pos ? e.y != e.y : e.x != e.x) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    p += __shfl_xor(p, o, 64);
    b |= __shfl_xor(b, o, 64);
  }
  if (lane == 0) {
    s_p[wave] = p;
    s_b[wave] = b;
  }
  __syncthreads();
  if (tid == 0) {
    p = b = 0;
    for (int w = 0; w < RK_THREADS / 64; ++w) {
      p += s_p[w];
      b |= s_b[w];
    }
    P[c] = p;
    bad[c] = b;
    if (n_pos) n_pos[c] = p;
    if (b && err) atomicOr(err, AVID_DEVERR_RANK_SCORE);
  }
}

__global__ __launch_bounds__(RK_THREADS) void rank_pairs_kernel(long long N, const float2* __restrict__ st, const int* __restrict__ P,
                                                                const int* __restrict__ bad, double* __restrict__ part_ap,
                                                                long long* __restrict__ part_u2, int R) {
  __shared__ float s_pos[RK_SLAB];
  __shared__ float2 s_tile[RK_TILE];
  __shared__ double s_term[RK_SLAB];
  __shared__ int s_cnt[3][RK_THREADS];
  __shared__ int s_wsum[RK_THREADS / 64];
  __shared__ long long s_u2[RK_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Pc = P[c];
  if (bad[c] || Pc == 0) return;
  const float2* row = st + (long long)c * N;
  const long long Nn = N - Pc;
  const int rounds = (Pc + RK_SLAB - 1) / RK_SLAB;
  for (int round = blockIdx.y; round < rounds; round += gridDim.y) {
    const int lo = round * RK_SLAB, Pr = min(RK_SLAB, Pc - lo);
    // ---- the round's positives, in ascending sample index, into s_pos
    int base = 0;                                    // positives in front of this chunk (the same in every thread)
    for (long long n0 = 0; n0 < N && base < lo + Pr; n0 += RK_THREADS) {
      const long long n = n0 + tid;
      const float y = n < N ? row[n].y : NAN;
      const bool pos = y == y;
      const unsigned long long mask = __ballot(pos);
      if (lane == 0) s_wsum[wave] = __popcll(mask);
      __syncthreads();
      int off = base, tot = 0;
#pragma unroll
      for (int w = 0; w < RK_THREADS / 64; ++w) {
        off += w < wave ? s_wsum[w] : 0;
        tot += s_wsum[w];
      }
      const int rank = off + __popcll(mask & ((1ull << lane) - 1ull));
      if (pos && rank >= lo && rank < lo + Pr) s_pos[rank - lo] = y;
      base += tot;
      __syncthreads();
    }
    // ---- counts per positive: positives >= it, negatives >= it, negatives > it.  Lane (k, s) of S = 256 / Pr slices per positive
    //      takes the samples s, s + S, ... of every tile: lanes of one slice read one address (a broadcast), the slices neighbours
    const int S = RK_THREADS / Pr;
    const int k = tid / S, s = tid - k * S;
    const float sk = k < Pr ? s_pos[k] : NAN;
    int ge_p = 0, ge_n = 0, gt_n = 0;
    for (long long t0 = 0; t0 < N; t0 += RK_TILE) {
      const int len = (int)min((long long)RK_TILE, N - t0);
      __syncthreads();
      for (int j = tid; j < len; j += RK_THREADS) s_tile[j] = row[t0 + j];
      __syncthreads();
      for (int j = s; j < len; j += S) {
        const float2 e = s_tile[j];
        ge_n += e.x >= sk ? 1 : 0;
        gt_n += e.x > sk ? 1 : 0;
        ge_p += e.y >= sk ? 1 : 0;
      }
    }
    s_cnt[0][tid] = ge_p;
    s_cnt[1][tid] = ge_n;
    s_cnt[2][tid] = gt_n;
    __syncthreads();
    long long u2 = 0;
    if (k < Pr && s == 0) {
      for (int j = 1; j < S; ++j) {
        ge_p += s_cnt[0][tid + j];
        ge_n += s_cnt[1][tid + j];
        gt_n += s_cnt[2][tid + j];
      }
      s_term[k] = (double)ge_p / (double)(ge_p + ge_n);
      u2 = 2 * Nn - ge_n - gt_n;
    }
    // ---- the round's sums: U2 over the lanes (integers), the terms in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) u2 += __shfl_xor(u2, o, 64);
    if (lane == 0) s_u2[wave] = u2;
    __syncthreads();
    if (tid == 0) {
      double ap = 0.0;
      for (int j = 0; j < Pr; ++j) ap += s_term[j];
      u2 = 0;
      for (int w = 0; w < RK_THREADS / 64; ++w) u2 += s_u2[w];
      part_ap[(long long)c * R + round] = ap;
      part_u2[(long long)c * R + round] = u2;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rank_final_kernel(long long N, int C, const int* __restrict__ P, const int* __restrict__ bad,
                                                         const double* __restrict__ part_ap, const long long* __restrict__ part_u2,
                                                         int R, double* __restrict__ ap, double* __restrict__ auc) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long long Pc = P[c], Nn = N - Pc;
  double a = NAN, u = NAN;
  if (!bad[c] && Pc > 0) {
    const int rounds = (int)((Pc + RK_SLAB - 1) / RK_SLAB);
    double sa = 0.0;
    long long su = 0;
    for (int r = 0; r < rounds; ++r) {
      sa += part_ap[(long long)c * R + r];
      su += part_u2[(long long)c * R + r];
    }
    a = sa / (double)Pc;
    if (Nn > 0) u = (double)su / (double)(2 * Pc * Nn);
  }
  if (ap) ap[c] = a;
  if (auc) auc[c] = u;
}

}  // namespace avid

using namespace avid;

extern "C" size_t avid_rank_metrics_workspace_bytes(int64_t N, int C) {
  if (!rank_supported(N, C)) return 0;
  return rank_ws(nullptr, N, C).bytes;
}

extern "C" int avid_rank_metrics(int64_t N, int C, const float* scores, const float* targets, double* ap, double* auc,
                                 int64_t* n_pos, void* ws, size_t ws_bytes, int32_t* err, avid_stream_t stream) {
  AVID_REQUIRE(N >= 1 && C >= 1 && scores && targets && ws, AVID_E_BADARG, "rank_metrics: bad arguments (N %lld, C %d)",
               (long long)N, C);
  AVID_REQUIRE(rank_supported(N, C), AVID_E_UNSUPPORTED, "rank_metrics: N %lld / C %d beyond the kernels' index range", (long long)N, C);
  const RankWs w = rank_ws(ws, N, C);
  AVID_REQUIRE(ws_bytes >= w.bytes, AVID_E_BADARG, "rank_metrics: workspace too small (%zu < %zu)", ws_bytes, w.bytes);
  AVID_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, AVID_E_BADARG, "rank_metrics: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)N * C;
  {
    ScopedTimer t(s, "rank_transpose_kernel", 0.0, 16.0 * elems);
    hipLaunchKernelGGL(rank_transpose_kernel, dim3((unsigned)ceil_div(N, 32), (unsigned)ceil_div(C, 32)), dim3(256), 0, s,
                       (long long)N, C, scores, targets, w.st);
  }
  int rc = check_launch("rank_metrics (transpose)");
  if (rc != AVID_OK) return rc;
  {
    ScopedTimer t(s, "rank_count_kernel", 0.0, 8.0 * elems);
    hipLaunchKernelGGL(rank_count_kernel, dim3(C), dim3(RK_THREADS), 0, s, (long long)N, w.st, w.P, w.bad, (long long*)n_pos, err);
  }
  if ((rc = check_launch("rank_metrics (count)")) != AVID_OK) return rc;
  {
    const int Z = w.R < RK_MAX_Z ? w.R : RK_MAX_Z;
    ScopedTimer t(s, "rank_pairs_kernel", 0.0, 16.0 * elems);
    hipLaunchKernelGGL(rank_pairs_kernel, dim3(C, Z), dim3(RK_THREADS), 0, s, (long long)N, w.st, w.P, w.bad, w.part_ap, w.part_u2,
                       w.R);
  }
  if ((rc = check_launch("rank_metrics (pairs)")) != AVID_OK) return rc;
  ScopedTimer t(s, "rank_final_kernel", 0.0, 24.0 * C);
  hipLaunchKernelGGL(rank_final_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, s, (long long)N, C, w.P, w.bad, w.part_ap,
                     w.part_u2, w.R, ap, auc);
  return check_launch("rank_metrics (final)");
}
