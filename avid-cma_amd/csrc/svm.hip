// Linear one-vs-all SVM on frozen features (the sound-classification protocol of the paper and of L3 / XDC: ESC-50, DCASE):
// the two skinny products over a tall feature matrix X [N][F] that every pass of a full-batch solver needs, and the
// element-wise work between them.  The solver itself (truncated Newton, all classes in lock-step) is avid_hip/ops.py:svm_fit.
//
//   scores  Z [N][C] = X . W^T + b          one 64 x 64 tile per workgroup, the WHOLE reduction over F inside it
//   xt      G [C][F] = D^T . X,  gb = column sums of D      rows cut into slices of SVM_SLICE, partial tiles added in order
//
// Products are exact fp32 (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  Every result is one sum in a fixed order that
// depends on (N, F, C) only — never on the CU count, the CU budget or the scheduling: no atomics on any result.
#include <math.h>

#include "common.h"

namespace avid {

constexpr int SVM_T = 64;          // tile edge
constexpr int SVM_KT = 32;         // reduction steps per LDS stage
constexpr int SVM_SLICE = 512;     // rows of X per slice of avid_svm_xt
constexpr int SVM_LSLICE = 256;    // rows per partial sum of avid_svm_loss
constexpr int SVM_LADDER = 16;     // step sizes 2^0 .. 2^-15 of avid_svm_loss

// ---------------------------------------------------------------------------------------------
// out[m][n] = sum_k A(m, k) * Bm(n, k) on four waves (a wave: 32 x 32).
//   KC = true  (scores): A = X (m = row, k = feature contiguous), Bm = W (n = class, k contiguous), k = 0 .. F
//   KC = false (xt):     A = D (k = row, m = class contiguous),   Bm = X (k = row, n = feature contiguous), k = the slice's rows
// Operand tiles go through LDS as [k][m] / [k][n]; the next stage's loads are in flight during the products.  A wave
// alternates between two accumulators — acc0 takes k = 0, 1 (mod 4), acc1 k = 2, 3 (mod 4), each in ascending k — and the
// tile is (acc0 + acc1) (+ bias): the order tests/_svm_ref.py restates.  Rows, columns and k outside the matrices are zeros.
// ---------------------------------------------------------------------------------------------
template <bool KC>
struct SvmTile {
  static constexpr int LD = KC ? SVM_T + 2 : SVM_T + 4;     // conflict-free transposing writes / 16-byte rows
};

// the 2 x 4 elements thread t stages of one operand tile.  KC: row t / 8 + 32 j, k = 4 (t % 8) + i; else k = t / 16 + 16 j,
// rows 4 (t % 16) + i
template <bool KC>
__device__ __forceinline__ void svm_load(const float* __restrict__ P, long long ld, int rows, int r0, int k0, int kend, bool vec,
                                         int tid, float (&v)[2][4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = KC ? r0 + (tid >> 3) + 32 * j : r0 + ((tid & 15) << 2);
    const int k = KC ? k0 + ((tid & 7) << 2) : k0 + (tid >> 4) + 16 * j;
    if (KC) {
      if (vec && r < rows && k + 3 < kend) {
        const float4 q = *reinterpret_cast<const float4*>(P + (long long)r * ld + k);
        v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[j][i] = (r < rows && k + i < kend) ? P[(long long)r * ld + k + i] : 0.f;
      }
    } else {
      if (vec && k < kend && r + 3 < rows) {
        const float4 q = *reinterpret_cast<const float4*>(P + (long long)k * ld + r);
        v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[j][i] = (k < kend && r + i < rows) ? P[(long long)k * ld + r + i] : 0.f;
      }
    }
  }
}

template <bool KC>
__device__ __forceinline__ void svm_store(float (*S)[SvmTile<KC>::LD], int tid, const float (&v)[2][4]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (KC) {
      const int r = (tid >> 3) + 32 * j, k = (tid & 7) << 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) S[k + i][r] = v[j][i];
    } else {
      const int k = (tid >> 4) + 16 * j, r = (tid & 15) << 2;
      *reinterpret_cast<float4*>(&S[k][r]) = make_float4(v[j][0], v[j][1], v[j][2], v[j][3]);
    }
  }
}

// grid: tiles_m * tiles_n * slices workgroups, the slice outermost.  sliced == 0: the scores form (k = 0 .. K, out + bias);
// else partial tiles out[slice][M][N] of the rows slice * SVM_SLICE ...
// Stages of 64 steps and a second stage of loads in flight were measured and change nothing (within 5 % either way at
// 16 000 x 8 192 x 50): DESIGN.md 6h.
template <bool KC>
__global__ __launch_bounds__(256) void svm_gemm_kernel(int M, int N, int K, const float* __restrict__ A, long long lda, int vecA,
                                                       const float* __restrict__ Bm, long long ldb, int vecB,
                                                       const float* __restrict__ bias, float* __restrict__ out, int tiles_m,
                                                       int tiles_n, int sliced) {
  constexpr int LD = SvmTile<KC>::LD;
  __shared__ __align__(16) float As[SVM_KT][LD];
  __shared__ __align__(16) float Bs[SVM_KT][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned tiles = (unsigned)tiles_m * (unsigned)tiles_n;
  const unsigned tile = blockIdx.x % tiles, slice = blockIdx.x / tiles;
  const int m0 = (int)(tile % (unsigned)tiles_m) * SVM_T, n0 = (int)(tile / (unsigned)tiles_m) * SVM_T;
  const int kbeg = sliced ? (int)slice * SVM_SLICE : 0;
  const int kend = sliced ? (int)min((long long)K, (long long)kbeg + SVM_SLICE) : K;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int li = lane & 31, lk = lane >> 5;
  floatx16 acc0 = {0}, acc1 = {0};
  float ra[2][4], rb[2][4];
  svm_load<KC>(A, lda, M, m0, kbeg, kend, vecA != 0, tid, ra);
  svm_load<KC>(Bm, ldb, N, n0, kbeg, kend, vecB != 0, tid, rb);
  for (int k0 = kbeg; k0 < kend; k0 += SVM_KT) {
    svm_store<KC>(As, tid, ra);
    svm_store<KC>(Bs, tid, rb);
    __syncthreads();
    if (k0 + SVM_KT < kend) {
      svm_load<KC>(A, lda, M, m0, k0 + SVM_KT, kend, vecA != 0, tid, ra);
      svm_load<KC>(Bm, ldb, N, n0, k0 + SVM_KT, kend, vecB != 0, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < SVM_KT; kk += 4) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + lk][wm + li], Bs[kk + lk][wn + li], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + 2 + lk][wm + li], Bs[kk + 2 + lk][wn + li], acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  // accumulator element r of a lane: row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32
  const int n = n0 + wn + li;
  if (n >= N) return;
  const float bv = (!sliced && bias) ? bias[n] : 0.f;
  float* dst = sliced ? out + (long long)slice * M * N : out;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm + (r >> 2) * 8 + lk * 4 + (r & 3);
    if (m < M) dst[(long long)m * N + n] = (acc0[r] + acc1[r]) + bv;
  }
}

// colpart[slice][c] = sum over the slice's rows of d[i][c]: thread (class, one of four row groups) sums its rows in double in
// ascending order, the four groups are added in group order
__global__ __launch_bounds__(256) void svm_colsum_kernel(int N, int C, int ncb, const float* __restrict__ d,
                                                         double* __restrict__ colpart) {
  __shared__ double red[4][64];
  const int fl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = (int)(blockIdx.x % (unsigned)ncb) * 64 + fl;
  const long long slice = blockIdx.x / (unsigned)ncb;
  const long long kbeg = slice * SVM_SLICE, kend = min((long long)N, kbeg + SVM_SLICE);
  double s = 0.0;
  if (c < C)
    for (long long i = kbeg + g; i < kend; i += 4) s += (double)d[i * C + c];
  red[g][fl] = s;
  __syncthreads();
  if (g == 0 && c < C) colpart[slice * C + c] = ((red[0][fl] + red[1][fl]) + red[2][fl]) + red[3][fl];
}

// g[i] = the slices' partial tiles added in slice order in double, rounded once; gb[c] likewise from the column partials
__global__ __launch_bounds__(256) void svm_reduce_kernel(long long MN, int C, int slices, const float* __restrict__ part,
                                                         const double* __restrict__ colpart, float* __restrict__ g,
                                                         float* __restrict__ gb) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = first; i < MN; i += stride) {
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double)part[(long long)k * MN + i];
    g[i] = (float)s;
  }
  if (gb)
    for (long long c = first; c < C; c += stride) {
      double s = 0.0;
      for (int k = 0; k < slices; ++k) s += colpart[(long long)k * C + c];
      gb[c] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------
// Element-wise over [N][C].  y = +1 where labels[i] == c, else -1; cost_ic = y > 0 ? cost * pos_weight[c] : cost (the product
// rounded to fp32 once).  A label outside [0, C) sets AVID_DEVERR_SVM_LABEL and counts as no class (y = -1 everywhere).
// ---------------------------------------------------------------------------------------------
// xv == NULL: the hinge residual out = (y * m) * cost_ic where m = fma(-y, z, 1) > 0, else 0
// xv != NULL: the active mask applied to a product X.V: out = cost_ic * xv where m > 0, else 0
__global__ __launch_bounds__(256) void svm_hinge_kernel(long long NC, int C, const float* __restrict__ z,
                                                        const int* __restrict__ labels, float cost,
                                                        const float* __restrict__ pos_weight, const float* __restrict__ xv,
                                                        float* __restrict__ out, int* __restrict__ err) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < NC; idx += stride) {
    const long long i = idx / C;
    const int c = (int)(idx - i * C);
    const int lb = labels[i];
    if ((lb < 0 || lb >= C) && err && c == 0) atomicOr(err, AVID_DEVERR_SVM_LABEL);
    const float y = lb == c ? 1.f : -1.f;
    const float ci = lb == c ? cost * (pos_weight ? pos_weight[c] : 1.f) : cost;
    const float m = fmaf(-y, z[idx], 1.f);
    float v = 0.f;
    if (m > 0.f) v = xv ? ci * xv[idx] : (y * m) * ci;
    out[idx] = v;
  }
}

// part[slice][k][c] = sum over the slice's rows of cost_ic * max(0, 1 - y (z + 2^-k zd))^2, k < K, evaluated in double from
// the fp32 z, zd and cost_ic: thread (class, one of four row groups), rows ascending, groups added in order
__global__ __launch_bounds__(256) void svm_loss_kernel(int N, int C, int K, int ncb, const float* __restrict__ z,
                                                       const float* __restrict__ zd, const int* __restrict__ labels, float cost,
                                                       const float* __restrict__ pos_weight, double* __restrict__ part,
                                                       int* __restrict__ err) {
  __shared__ double red[4][64];
  const int fl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int cb = (int)(blockIdx.x % (unsigned)ncb);
  const int c = cb * 64 + fl;
  const long long slice = blockIdx.x / (unsigned)ncb;
  const long long kbeg = slice * SVM_LSLICE, kend = min((long long)N, kbeg + SVM_LSLICE);
  double acc[SVM_LADDER];
#pragma unroll
  for (int k = 0; k < SVM_LADDER; ++k) acc[k] = 0.0;
  const bool live = c < C;
  const float cw = live ? cost * (pos_weight ? pos_weight[c] : 1.f) : 0.f;
  for (long long i = kbeg + g; i < kend; i += 4) {
    const int lb = labels[i];
    if ((lb < 0 || lb >= C) && err && cb == 0 && fl == 0) atomicOr(err, AVID_DEVERR_SVM_LABEL);
    if (!live) continue;
    const double y = lb == c ? 1.0 : -1.0;
    const double ci = (double)(lb == c ? cw : cost);
    const double zz = (double)z[i * C + c], dd = zd ? (double)zd[i * C + c] : 0.0;
    double a = 1.0;
#pragma unroll
    for (int k = 0; k < SVM_LADDER; ++k) {
      if (k < K) {
        const double m = 1.0 - y * (zz + a * dd);
        if (m > 0.0) acc[k] += ci * (m * m);
      }
      a *= 0.5;
    }
  }
#pragma unroll
  for (int k = 0; k < SVM_LADDER; ++k) {
    if (k < K) {     // (K is uniform over the workgroup)
      __syncthreads();
      red[g][fl] = acc[k];
      __syncthreads();
      if (g == 0 && live) part[(slice * K + k) * C + c] = ((red[0][fl] + red[1][fl]) + red[2][fl]) + red[3][fl];
    }
  }
}

__global__ __launch_bounds__(256) void svm_loss_finish_kernel(int KC, long long slices, const double* __restrict__ part,
                                                              double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= KC) return;
  double s = 0.0;
  for (long long k = 0; k < slices; ++k) s += part[k * KC + i];
  out[i] = s;
}

static inline bool svm_aligned16(const void* p, long long ld) { return (((uintptr_t)p) & 15) == 0 && (ld & 3) == 0; }
static inline bool svm_shape_ok(int64_t N, int F, int C) { return N >= 1 && N < (1ll << 31) && F >= 1 && C >= 1; }
static inline int64_t svm_slices(int64_t N) { return ceil_div(N, SVM_SLICE); }
static inline int64_t svm_lslices(int64_t N) { return ceil_div(N, SVM_LSLICE); }
static inline size_t svm_xt_bytes(int64_t N, int F, int C) {
  return (size_t)svm_slices(N) * (size_t)C * (sizeof(double) + sizeof(float) * (size_t)F);
}
static inline size_t svm_loss_bytes(int64_t N, int C) {
  return (size_t)svm_lslices(N) * SVM_LADDER * (size_t)C * sizeof(double);
}

}  // namespace avid

using namespace avid;

extern "C" size_t avid_svm_workspace_bytes(int64_t N, int F, int C) {
  if (!svm_shape_ok(N, F, C)) return 0;
  const size_t a = svm_xt_bytes(N, F, C), b = svm_loss_bytes(N, C);
  return a > b ? a : b;
}

extern "C" int avid_svm_scores(int64_t N, int F, int C, const float* x, const float* w, const float* bias, float* z,
                               avid_stream_t stream) {
  AVID_REQUIRE(x && w && z, AVID_E_BADARG, "svm_scores: null pointer (x, w and z are required)");
  AVID_REQUIRE(svm_shape_ok(N, F, C), AVID_E_SHAPE, "svm_scores: N %lld, F %d, C %d outside 1 <= N < 2^31, F >= 1, C >= 1",
               (long long)N, F, C);
  const int64_t tiles_m = ceil_div(N, SVM_T), tiles_n = ceil_div(C, SVM_T);
  AVID_REQUIRE(tiles_m * tiles_n < (1ll << 31), AVID_E_SHAPE, "svm_scores: grid too large");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "svm_gemm_kernel<true>", 2.0 * (double)N * F * C, 4.0 * ((double)N * F + (double)C * F + (double)N * C));
  hipLaunchKernelGGL((svm_gemm_kernel<true>), dim3((unsigned)(tiles_m * tiles_n)), dim3(256), 0, s, (int)N, C, F, x, (long long)F,
                     svm_aligned16(x, F) ? 1 : 0, w, (long long)F, svm_aligned16(w, F) ? 1 : 0, bias, z, (int)tiles_m, (int)tiles_n, 0);
  return check_launch("svm_scores");
}

extern "C" int avid_svm_xt(int64_t N, int F, int C, const float* x, const float* d, float* g, float* gb, void* ws,
                           size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(x && d && g, AVID_E_BADARG, "svm_xt: null pointer (x, d and g are required)");
  AVID_REQUIRE(svm_shape_ok(N, F, C), AVID_E_SHAPE, "svm_xt: N %lld, F %d, C %d outside 1 <= N < 2^31, F >= 1, C >= 1",
               (long long)N, F, C);
  const size_t need = svm_xt_bytes(N, F, C);
  AVID_REQUIRE(ws && ws_bytes >= need && (((uintptr_t)ws) & 7) == 0, AVID_E_BADARG,
               "svm_xt: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
  const int64_t slices = svm_slices(N), tiles_m = ceil_div(C, SVM_T), tiles_n = ceil_div(F, SVM_T), ncb = tiles_m;
  AVID_REQUIRE(tiles_m * tiles_n * slices < (1ll << 31), AVID_E_SHAPE, "svm_xt: grid too large");
  hipStream_t s = (hipStream_t)stream;
  double* colpart = (double*)ws;
  float* part = (float*)(colpart + slices * C);
  const long long MN = (long long)C * F;
  {
    ScopedTimer t(s, "svm_gemm_kernel<false>", 2.0 * (double)N * F * C,
                  4.0 * ((double)N * F + (double)N * C * (double)tiles_n + (double)MN * slices));
    hipLaunchKernelGGL((svm_gemm_kernel<false>), dim3((unsigned)(tiles_m * tiles_n * slices)), dim3(256), 0, s, C, F, (int)N, d,
                       (long long)C, svm_aligned16(d, C) ? 1 : 0, x, (long long)F, svm_aligned16(x, F) ? 1 : 0, nullptr, part,
                       (int)tiles_m, (int)tiles_n, 1);
  }
  int rc = check_launch("svm_xt");
  if (rc != AVID_OK) return rc;
  if (gb) {
    ScopedTimer t(s, "svm_colsum_kernel", (double)N * C, 4.0 * (double)N * C);
    hipLaunchKernelGGL(svm_colsum_kernel, dim3((unsigned)(ncb * slices)), dim3(256), 0, s, (int)N, C, (int)ncb, d, colpart);
    rc = check_launch("svm_colsum");
    if (rc != AVID_OK) return rc;
  }
  long long blocks = ceil_div(MN, 256);
  if (blocks > 4096) blocks = 4096;
  ScopedTimer t(s, "svm_reduce_kernel", (double)MN * slices, 4.0 * (double)MN * (slices + 1));
  hipLaunchKernelGGL(svm_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, MN, C, (int)slices, part, colpart, g, gb);
  return check_launch("svm_reduce");
}

extern "C" int avid_svm_hinge(int64_t N, int C, const float* z, const int32_t* labels, float cost, const float* pos_weight,
                              const float* xv, float* out, int32_t* err, avid_stream_t stream) {
  AVID_REQUIRE(z && labels && out, AVID_E_BADARG, "svm_hinge: null pointer (z, labels and out are required)");
  AVID_REQUIRE(N >= 1 && N < (1ll << 31) && C >= 1, AVID_E_SHAPE, "svm_hinge: N %lld, C %d outside 1 <= N < 2^31, C >= 1",
               (long long)N, C);
  AVID_REQUIRE(cost > 0.f && isfinite(cost), AVID_E_BADARG, "svm_hinge: cost must be positive and finite");
  const long long NC = (long long)N * C;
  long long blocks = ceil_div(NC, 256);
  if (blocks > 8192) blocks = 8192;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "svm_hinge_kernel", 4.0 * (double)NC, 4.0 * (double)NC * (xv ? 3 : 2));
  hipLaunchKernelGGL(svm_hinge_kernel, dim3((unsigned)blocks), dim3(256), 0, s, NC, C, z, (const int*)labels, cost, pos_weight, xv,
                     out, (int*)err);
  return check_launch("svm_hinge");
}

extern "C" int avid_svm_loss(int64_t N, int C, int K, const float* z, const float* zd, const int32_t* labels, float cost,
                             const float* pos_weight, double* out, void* ws, size_t ws_bytes, int32_t* err,
                             avid_stream_t stream) {
  AVID_REQUIRE(z && labels && out, AVID_E_BADARG, "svm_loss: null pointer (z, labels and out are required)");
  AVID_REQUIRE(N >= 1 && N < (1ll << 31) && C >= 1, AVID_E_SHAPE, "svm_loss: N %lld, C %d outside 1 <= N < 2^31, C >= 1",
               (long long)N, C);
  AVID_REQUIRE(K >= 1 && K <= SVM_LADDER && (zd || K == 1), AVID_E_BADARG,
               "svm_loss: K %d outside [1, %d] (or more than one step without a direction)", K, SVM_LADDER);
  AVID_REQUIRE(cost > 0.f && isfinite(cost), AVID_E_BADARG, "svm_loss: cost must be positive and finite");
  const int64_t slices = svm_lslices(N), ncb = ceil_div(C, 64);
  const size_t need = (size_t)slices * K * C * sizeof(double);
  AVID_REQUIRE(ws && ws_bytes >= need && (((uintptr_t)ws) & 7) == 0, AVID_E_BADARG,
               "svm_loss: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
  AVID_REQUIRE(ncb * slices < (1ll << 31) && (int64_t)K * C < (1ll << 31), AVID_E_SHAPE, "svm_loss: grid too large");
  hipStream_t s = (hipStream_t)stream;
  {
    ScopedTimer t(s, "svm_loss_kernel", 4.0 * (double)N * C * K, 4.0 * (double)N * C * (zd ? 2 : 1));
    hipLaunchKernelGGL(svm_loss_kernel, dim3((unsigned)(ncb * slices)), dim3(256), 0, s, (int)N, C, K, (int)ncb, z, zd,
                       (const int*)labels, cost, pos_weight, (double*)ws, (int*)err);
  }
  int rc = check_launch("svm_loss");
  if (rc != AVID_OK) return rc;
  ScopedTimer t(s, "svm_loss_finish_kernel", (double)slices * K * C, 8.0 * (double)slices * K * C);
  hipLaunchKernelGGL(svm_loss_finish_kernel, dim3((unsigned)ceil_div((int64_t)K * C, 256)), dim3(256), 0, s, K * C,
                     (long long)slices, (const double*)ws, out);
  return check_launch("svm_loss_finish");
}
