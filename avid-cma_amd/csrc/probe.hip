// Linear-probe heads (MOSTModel / Classifier): adaptive max pooling of a channels-last tap into the reference's flatten
// order, BatchNorm1d over [B, F], and the probe's Linear(F, C) on the matrix pipe.
//
// Reference ops replaced: utils/eval_utils.py:231-242 (Classifier.forward: nn.AdaptiveMaxPool3d under no_grad, view(B, -1),
// nn.BatchNorm1d, nn.Linear) for the taps of utils/eval_utils.py:322-329 (MOSTModel.forward) and their autograd backward in
// eval-action-recg-linear.py.  Sizes of the shipped config (configs/benchmark/kinetics/8x224x224-linear.yaml): batch 128,
// features 8192 / 9216, 400 classes — avid_bn_fwd_* stops at 1024 channels and avid_cls_linear_* is one wave per output.
//
// Every result is one sum in a fixed order: no atomics, bit-reproducible from run to run (as classify.hip promises).
#include <math.h>

#include "common.h"

namespace avid {

// ---------------------------------------------------------------------------------------------
// Adaptive max pooling.  One workgroup per (b, to, chunk of CC channels); thread = (channel c of the chunk, group g); group g
// owns the output columns wo = g, g + G, ...  The workgroup walks the input rows h of its t-window once; for each row a thread
// takes the maximum over its (t, w) window and folds it into every output row ho whose window holds h.  acc[(ho, wo)][c] lives
// in LDS, each slot touched by ONE thread only (no synchronisation inside the walk).  CC >= 32 where the tap has that many
// channels: a thread group reads whole 128-byte lines, and a line is fetched by one workgroup only.
// No argmax, no backward (the reference pools under no_grad).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adaptive_maxpool_kernel(int B, int T, int H, int W, int C, int To, int Ho, int Wo, int CC,
                                                               int nchunks, const float* __restrict__ x, float* __restrict__ y) {
  extern __shared__ float acc[];      // [Ho * Wo][CC]
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % nchunks;
  const int to = (blockIdx.x / nchunks) % To;
  const int b = blockIdx.x / (nchunks * To);
  const int cl = tid % CC, g = tid / CC, G = 256 / CC;
  const int c = chunk * CC + cl;
  const int HW = Ho * Wo;
  for (int i = tid; i < HW * CC; i += 256) acc[i] = -INFINITY;
  __syncthreads();
  const int ts = (int)(((long long)to * T) / To), te = (int)((((long long)to + 1) * T + To - 1) / To);
  if (c < C) {
    for (int h = 0; h < H; ++h) {
      for (int wo = g; wo < Wo; wo += G) {
        const int ws = (int)(((long long)wo * W) / Wo), we = (int)((((long long)wo + 1) * W + Wo - 1) / Wo);
        float m = -INFINITY;
        for (int t = ts; t < te; ++t) {
          const float* row = x + ((((long long)b * T + t) * H + h) * W) * C + c;
#pragma unroll 4
          for (int w = ws; w < we; ++w) {
            const float v = row[(long long)w * C];
            if (v > m || v != v) m = v;
          }
        }
        for (int ho = 0; ho < Ho; ++ho) {
          const int hs = (int)(((long long)ho * H) / Ho), he = (int)((((long long)ho + 1) * H + Ho - 1) / Ho);
          if (h >= hs && h < he) {
            float* a = acc + (ho * Wo + wo) * CC + cl;
            const float cur = *a;
            if (m > cur || m != m) *a = m;
          }
        }
      }
    }
  }
  __syncthreads();
  // y [B][C][To][Ho][Wo]: consecutive threads write consecutive (ho, wo) of one channel
  for (int i = tid; i < HW * CC; i += 256) {
    const int ci = i / HW, r = i % HW;
    const int cc = chunk * CC + ci;
    if (cc < C) y[(((long long)b * C + cc) * To + to) * HW + r] = acc[r * CC + ci];
  }
}

// The same for taps whose channel count is a multiple of four (all of R(2+1)D's): a thread owns FOUR channels (one 16-byte
// load per position), so CC / 4 lanes cover a position and the workgroup has 1024 / CC groups — more than output columns.
// Per input row h the groups therefore share out the (wo, t) pairs: stage 1, a group takes the maximum over the w window of
// one (wo, t) into LDS (every thread has a window of independent 16-byte loads in flight); stage 2, thread (wo, c) reduces its
// column over t and folds it into the output rows whose window holds h — again ONE owner thread per accumulator slot.  Same
// values as the kernel above (a maximum does not depend on the order), same one-pass walk over the input.
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void adaptive_maxpool4_kernel(int B, int T, int H, int W, int C, int To, int Ho, int Wo, int CC,
                                                                int nchunks, const float* __restrict__ x, float* __restrict__ y) {
  extern __shared__ __align__(16) float lds4[];      // acc [Ho * Wo][CC] | tmp [Wo * nt][CC]
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % nchunks;
  const int to = (blockIdx.x / nchunks) % To;
  const int b = blockIdx.x / (nchunks * To);
  const int L = CC >> 2, cl4 = (tid % L) << 2, g = tid / L, G = 256 / L;
  const int c = chunk * CC + cl4;
  const int HW = Ho * Wo;
  const int ts = (int)(((long long)to * T) / To), te = (int)((((long long)to + 1) * T + To - 1) / To);
  const int nt = te - ts, items = Wo * nt;
  float* acc = lds4;
  float* tmp = lds4 + HW * CC;
  for (int i = tid; i < HW * CC; i += 256) acc[i] = -INFINITY;
  __syncthreads();
  for (int h = 0; h < H; ++h) {
    for (int it = g; it < items; it += G) {
      const int wo = it / nt, t = ts + it % nt;
      const int ws = (int)(((long long)wo * W) / Wo), we = (int)((((long long)wo + 1) * W + Wo - 1) / Wo);
      float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      if (c < C) {
        const float* row = x + ((((long long)b * T + t) * H + h) * W) * C + c;
#pragma unroll 6
        for (int w = ws; w < we; ++w) {
          const float4 v = *reinterpret_cast<const float4*>(row + (long long)w * C);
          m.x = nanmax(m.x, v.x); m.y = nanmax(m.y, v.y); m.z = nanmax(m.z, v.z); m.w = nanmax(m.w, v.w);
        }
      }
      *reinterpret_cast<float4*>(tmp + it * CC + cl4) = m;
    }
    __syncthreads();
    for (int i = tid; i < Wo * CC; i += 256) {
      const int wo = i / CC, cl = i % CC;
      float m = -INFINITY;
      for (int k = 0; k < nt; ++k) m = nanmax(m, tmp[(wo * nt + k) * CC + cl]);
      for (int ho = 0; ho < Ho; ++ho) {
        const int hs = (int)(((long long)ho * H) / Ho), he = (int)((((long long)ho + 1) * H + Ho - 1) / Ho);
        if (h >= hs && h < he) {
          float* a = acc + (ho * Wo + wo) * CC + cl;
          *a = nanmax(*a, m);
        }
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < HW * CC; i += 256) {
    const int ci = i / HW, r = i % HW;
    const int cc = chunk * CC + ci;
    if (cc < C) y[(((long long)b * C + cc) * To + to) * HW + r] = acc[r * CC + ci];
  }
}

// ---------------------------------------------------------------------------------------------
// BatchNorm1d over x [B, F].  One workgroup owns 64 features; thread = (feature, one of four batch groups): group g sums the
// rows g, g + 4, ... in double, the four partial sums are added in group order.  Mean first, then the sum of squared
// deviations from it (two passes over a column that is in cache), so activations far off zero lose nothing.  The element-wise
// maps are evaluated in double and rounded once (1.2 M elements at the shipped sizes: the kernels stay bound by their loads).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double bn1d_sum4(double (*red)[64], int fl, int g, double v) {
  __syncthreads();      // the previous use of red is over
  red[g][fl] = v;
  __syncthreads();
  return ((red[0][fl] + red[1][fl]) + red[2][fl]) + red[3][fl];
}

__global__ __launch_bounds__(256) void bn1d_fwd_train_kernel(int B, int F, const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ running_mean,
                                                             float* __restrict__ running_var, float momentum, float eps,
                                                             float* __restrict__ y, float* __restrict__ save2,
                                                             long long* __restrict__ counter) {
  __shared__ double red[4][64];
  const int fl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + fl;
  const bool live = f < F;
  double s = 0.0;
  if (live)
    for (int b = g; b < B; b += 4) s += (double)x[(long long)b * F + f];
  const double mean = bn1d_sum4(red, fl, g, s) / (double)B;
  double q = 0.0;
  if (live)
    for (int b = g; b < B; b += 4) {
      const double d = (double)x[(long long)b * F + f] - mean;
      q += d * d;
    }
  const double var = bn1d_sum4(red, fl, g, q) / (double)B;
  if (!live) return;
  const float meanf = (float)mean, invstd = (float)(1.0 / sqrt(var + (double)eps));
  if (g == 0) {
    save2[f] = meanf;
    save2[F + f] = invstd;
    running_mean[f] = (float)((1.0 - (double)momentum) * (double)running_mean[f] + (double)momentum * mean);
    running_var[f] = (float)((1.0 - (double)momentum) * (double)running_var[f] + (double)momentum * var * ((double)B / (double)(B - 1)));
    if (counter && f == 0) *counter += 1;
  }
  // applied in double from the unrounded statistics: with two or three rows x - mean cancels almost everything
  const double ga = gamma ? (double)gamma[f] : 1.0, be = beta ? (double)beta[f] : 0.0, istd = 1.0 / sqrt(var + (double)eps);
  for (int b = g; b < B; b += 4) {
    const long long i = (long long)b * F + f;
    y[i] = (float)((((double)x[i] - mean) * istd) * ga + be);
  }
}

__global__ __launch_bounds__(256) void bn1d_fwd_eval_kernel(int B, int F, const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ running_mean,
                                                            const float* __restrict__ running_var, float eps, float* __restrict__ y,
                                                            float* __restrict__ save2) {
  const int fl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + fl;
  if (f >= F) return;
  const float meanf = running_mean[f], invstd = (float)(1.0 / sqrt((double)running_var[f] + (double)eps));
  if (save2 && g == 0) {
    save2[f] = meanf;
    save2[F + f] = invstd;
  }
  const float ga = gamma ? gamma[f] : 1.f, be = beta ? beta[f] : 0.f;
  for (int b = g; b < B; b += 4) {
    const long long i = (long long)b * F + f;
    y[i] = fmaf((x[i] - meanf) * invstd, ga, be);
  }
}

// Training mode: the batch statistics are rebuilt here in double from x (two more passes over a cached column) instead of
// read back from save2: dx = gamma invstd (dy - mean(dy) - xhat mean(dy xhat)) cancels to eps / (var + eps) of its terms when
// the batch is two rows, which float32 statistics cannot carry.  frozen: save2's (running) statistics are the constants.
__global__ __launch_bounds__(256) void bn1d_bwd_kernel(int B, int F, const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ gamma, const float* __restrict__ save2, float eps,
                                                       int frozen, float* __restrict__ dx, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta) {
  __shared__ double red[4][64];
  const int fl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int f = blockIdx.x * 64 + fl;
  const bool live = f < F;
  double mean, istd;
  if (frozen) {
    mean = live ? (double)save2[f] : 0.0;
    istd = live ? (double)save2[F + f] : 0.0;
  } else {
    double s = 0.0;
    if (live)
      for (int b = g; b < B; b += 4) s += (double)x[(long long)b * F + f];
    mean = bn1d_sum4(red, fl, g, s) / (double)B;
    double q = 0.0;
    if (live)
      for (int b = g; b < B; b += 4) {
        const double d = (double)x[(long long)b * F + f] - mean;
        q += d * d;
      }
    istd = 1.0 / sqrt(bn1d_sum4(red, fl, g, q) / (double)B + (double)eps);
  }
  double s1 = 0.0, s2 = 0.0;
  if (live)
    for (int b = g; b < B; b += 4) {
      const long long i = (long long)b * F + f;
      const double d = (double)dy[i];
      s1 += d;
      s2 += d * (((double)x[i] - mean) * istd);
    }
  const double sum_dy = bn1d_sum4(red, fl, g, s1);
  const double sum_dy_xhat = bn1d_sum4(red, fl, g, s2);
  if (!live) return;
  if (g == 0) {
    if (dgamma) dgamma[f] = (float)sum_dy_xhat;
    if (dbeta) dbeta[f] = (float)sum_dy;
  }
  if (!dx) return;
  const double k = (gamma ? (double)gamma[f] : 1.0) * istd;
  const double m1 = frozen ? 0.0 : sum_dy / (double)B, m2 = frozen ? 0.0 : sum_dy_xhat / (double)B;
  for (int b = g; b < B; b += 4) {
    const long long i = (long long)b * F + f;
    const double xhat = ((double)x[i] - mean) * istd;
    dx[i] = (float)(k * ((double)dy[i] - m1 - xhat * m2));
  }
}

// ---------------------------------------------------------------------------------------------
// The probe's Linear on the matrix pipe: out[m][n] = sum_k A(m, k) * Bm(n, k), one kernel for the three products of a layer:
//   forward  y  = x . w^T   A = x  (k contiguous), Bm = w (k contiguous), K = Fin
//   dx       dx = dy . w    A = dy (k contiguous), Bm = w (n contiguous), K = C
//   dw       dw = dy^T . x  A = dy (m contiguous), Bm = x (n contiguous), K = B
// Workgroup = four waves = a 64 x 64 output tile (a wave: 32 x 32, v_mfma_f32_32x32x2_f32), blockIdx.y = a slice of KC = 512
// of the reduction axis.  Both operand tiles go through LDS as [k][m] / [k][n] (a lane's operand element is then a
// conflict-free read), loaded from memory as float4 where alignment allows, the next tile's loads in flight during the
// products.  Within a slice each wave alternates between two accumulators, so one rounding chain is at most 256 products
// long: against float64 the rms error is below a float32 sum's.  One slice: the tile (+ bias) is the output;
// several: partial tiles [slice][M][N] in the workspace, added in slice order (in double) by probe_reduce_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int PG_T = 64;        // tile edge
constexpr int PG_KT = 16;       // k per LDS stage
constexpr int PG_LD = PG_T + 4; // LDS row pitch
constexpr int PG_KC = 512;      // k per slice

// the four elements thread t of the workgroup stages of one operand tile: KC (k contiguous in memory): row t / 4, k = 4 (t % 4) + j;
// else (row index contiguous): k = t / 16, rows 4 (t % 16) + j
template <bool KC>
__device__ __forceinline__ void pg_load(const float* __restrict__ P, long long ld, int rows, int r0, int k0, int kend, bool vec,
                                        int tid, float (&v)[4]) {
  if (KC) {
    const int r = r0 + (tid >> 2), k = k0 + ((tid & 3) << 2);
    if (vec && r < rows && k + 3 < kend) {
      const float4 q = *reinterpret_cast<const float4*>(P + (long long)r * ld + k);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (r < rows && k + j < kend) ? P[(long long)r * ld + k + j] : 0.f;
    }
  } else {
    const int k = k0 + (tid >> 4), r = r0 + ((tid & 15) << 2);
    if (vec && k < kend && r + 3 < rows) {
      const float4 q = *reinterpret_cast<const float4*>(P + (long long)k * ld + r);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (k < kend && r + j < rows) ? P[(long long)k * ld + r + j] : 0.f;
    }
  }
}

template <bool KC>
__device__ __forceinline__ void pg_store(float (*S)[PG_LD], int tid, const float (&v)[4]) {
  if (KC) {
    const int r = tid >> 2, k = (tid & 3) << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) S[k + j][r] = v[j];
  } else {
    const int k = tid >> 4, r = (tid & 15) << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) S[k][r + j] = v[j];
  }
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void probe_gemm_kernel(int M, int N, int K, const float* __restrict__ A, long long lda, int vecA,
                                                         const float* __restrict__ Bm, long long ldb, int vecB,
                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                         float* __restrict__ part, int tiles_m) {
  __shared__ float As[PG_KT][PG_LD];
  __shared__ float Bs[PG_KT][PG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = (blockIdx.x % tiles_m) * PG_T, n0 = (blockIdx.x / tiles_m) * PG_T;
  const int slice = blockIdx.y;
  const int kbeg = slice * PG_KC, kend = min(K, kbeg + PG_KC);
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int li = lane & 31, lk = lane >> 5;
  floatx16 acc0 = {0}, acc1 = {0};
  float ra[4], rb[4];
  pg_load<A_KC>(A, lda, M, m0, kbeg, kend, vecA != 0, tid, ra);
  pg_load<B_KC>(Bm, ldb, N, n0, kbeg, kend, vecB != 0, tid, rb);
  for (int k0 = kbeg; k0 < kend; k0 += PG_KT) {
    pg_store<A_KC>(As, tid, ra);
    pg_store<B_KC>(Bs, tid, rb);
    __syncthreads();
    if (k0 + PG_KT < kend) {
      pg_load<A_KC>(A, lda, M, m0, k0 + PG_KT, kend, vecA != 0, tid, ra);
      pg_load<B_KC>(Bm, ldb, N, n0, k0 + PG_KT, kend, vecB != 0, tid, rb);
    }
#pragma unroll
    for (int kk = 0; kk < PG_KT; kk += 4) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + lk][wm + li], Bs[kk + lk][wn + li], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + 2 + lk][wm + li], Bs[kk + 2 + lk][wn + li], acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  // accumulator element r of a lane: row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32
  const int n = n0 + wn + li;
  if (n >= N) return;
  const bool direct = gridDim.y == 1;
  const float bv = (direct && bias) ? bias[n] : 0.f;
  float* dst = direct ? out : part + (long long)slice * M * N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm + (r >> 2) * 8 + lk * 4 + (r & 3);
    if (m < M) dst[(long long)m * N + n] = (acc0[r] + acc1[r]) + bv;
  }
}

__global__ __launch_bounds__(256) void probe_reduce_kernel(long long MN, int N, int slices, const float* __restrict__ part,
                                                           const float* __restrict__ bias, float* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < MN; i += stride) {
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double)part[(long long)k * MN + i];
    if (bias) s += (double)bias[i % N];
    out[i] = (float)s;
  }
}

// db[c] = sum_b dy[b][c], in batch order
__global__ __launch_bounds__(256) void probe_colsum_kernel(int B, int C, const float* __restrict__ dy, float* __restrict__ db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += (double)dy[(long long)b * C + c];
  db[c] = (float)s;
}

static inline bool aligned16(const void* p, long long ld) { return (((uintptr_t)p) & 15) == 0 && (ld & 3) == 0; }

static inline int pg_slices(int K) { return (int)ceil_div(K, PG_KC); }

// out [M][N] = A . Bm^T (+ bias); ws holds the slices' partial tiles when K > PG_KC
template <bool A_KC, bool B_KC>
static int probe_gemm(const char* name, int M, int N, int K, const float* A, long long lda, const float* Bm, long long ldb,
                      const float* bias, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
  const int slices = pg_slices(K);
  const long long MN = (long long)M * N;
  AVID_REQUIRE(slices == 1 || (ws && ws_bytes >= (size_t)slices * MN * sizeof(float)), AVID_E_BADARG,
               "%s: workspace of %zu bytes, %zu needed", name, ws_bytes, (size_t)slices * MN * sizeof(float));
  const int tiles_m = (int)ceil_div(M, PG_T), tiles_n = (int)ceil_div(N, PG_T);
  {
    ScopedTimer t(s, name, 2.0 * MN * K, 4.0 * ((double)M * K + (double)N * K + (double)MN * (slices > 1 ? slices : 1)));
    hipLaunchKernelGGL((probe_gemm_kernel<A_KC, B_KC>), dim3((unsigned)(tiles_m * tiles_n), (unsigned)slices), dim3(256), 0, s, M, N, K,
                       A, lda, aligned16(A, lda) ? 1 : 0, Bm, ldb, aligned16(Bm, ldb) ? 1 : 0, bias, out, (float*)ws, tiles_m);
  }
  int rc = check_launch(name);
  if (rc != AVID_OK || slices == 1) return rc;
  long long g = ceil_div(MN, 256);
  if (g > 2048) g = 2048;
  ScopedTimer t(s, "probe_reduce_kernel", (double)MN * slices, 4.0 * MN * (slices + 1));
  hipLaunchKernelGGL(probe_reduce_kernel, dim3((unsigned)g), dim3(256), 0, s, MN, N, slices, (const float*)ws, bias, out);
  return check_launch("probe_reduce");
}

}  // namespace avid

using namespace avid;

extern "C" int avid_adaptive_maxpool_fwd(int B, int T, int H, int W, int C, int To, int Ho, int Wo, const float* x, float* y,
                                         avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && To > 0 && Ho > 0 && Wo > 0 && x && y, AVID_E_BADARG,
               "adaptive_maxpool_fwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const double in = (double)B * T * H * W * C, outn = (double)B * C * To * Ho * Wo;
  const size_t LDS_MAX = 48 * 1024;
  if ((C & 3) == 0 && (((uintptr_t)x) & 15) == 0) {
    // four channels per thread: 32 channels (one 128-byte line per position) per workgroup, fewer while the accumulators
    // [Ho * Wo][CC] and the row stage [Wo * nt][CC] do not fit 48 KB of LDS
    int nt_max = 1;
    for (int to = 0; to < To; ++to) {
      const int nt = (int)((((long long)to + 1) * T + To - 1) / To - ((long long)to * T) / To);
      if (nt > nt_max) nt_max = nt;
    }
    int CC = 32;
    while (CC > 4 && CC / 2 >= C) CC /= 2;
    const size_t per_c = ((size_t)Ho * Wo + (size_t)Wo * nt_max) * sizeof(float);
    while (CC > 4 && per_c * CC > LDS_MAX) CC /= 2;
    if (per_c * CC <= LDS_MAX) {
      const long long nchunks = ceil_div(C, CC), blocks = (long long)B * To * nchunks;
      AVID_REQUIRE(blocks < (1ll << 31), AVID_E_SHAPE, "adaptive_maxpool_fwd: grid too large");
      ScopedTimer t(s, "adaptive_maxpool4_kernel", 0.0, 4.0 * (in + outn));
      hipLaunchKernelGGL(adaptive_maxpool4_kernel, dim3((unsigned)blocks), dim3(256), per_c * CC, s, B, T, H, W, C, To, Ho, Wo, CC,
                         (int)nchunks, x, y);
      return check_launch("adaptive_maxpool_fwd");
    }
  }
  // any channel count: about 256 / Wo threads' worth of channels per workgroup (a power of two that divides 256, whole
  // 128-byte lines where the tap has them), the accumulators [Ho * Wo][CC] within 48 KB of LDS
  int CC = Wo <= 4 ? 64 : 32;
  while (CC > 1 && CC / 2 >= C) CC /= 2;
  while (CC > 1 && (size_t)Ho * Wo * CC * sizeof(float) > LDS_MAX) CC /= 2;
  const size_t lds = (size_t)Ho * Wo * CC * sizeof(float);
  AVID_REQUIRE(lds <= LDS_MAX, AVID_E_UNSUPPORTED, "adaptive_maxpool_fwd: %d x %d outputs per frame exceed the LDS accumulators", Ho, Wo);
  const long long nchunks = ceil_div(C, CC);
  const long long blocks = (long long)B * To * nchunks;
  AVID_REQUIRE(blocks < (1ll << 31), AVID_E_SHAPE, "adaptive_maxpool_fwd: grid too large");
  ScopedTimer t(s, "adaptive_maxpool_kernel", 0.0, 4.0 * (in + outn));
  hipLaunchKernelGGL(adaptive_maxpool_kernel, dim3((unsigned)blocks), dim3(256), lds, s, B, T, H, W, C, To, Ho, Wo, CC, (int)nchunks, x, y);
  return check_launch("adaptive_maxpool_fwd");
}

extern "C" int avid_bn1d_fwd_train(int B, int F, const float* x, const float* gamma, const float* beta, float* running_mean,
                                   float* running_var, float momentum, float eps, float* y, float* save2,
                                   int64_t* num_batches_tracked, avid_stream_t stream) {
  AVID_REQUIRE(F > 0 && x && y && save2 && running_mean && running_var, AVID_E_BADARG, "bn1d_fwd_train: bad arguments");
  AVID_REQUIRE(B >= 2, AVID_E_SHAPE, "bn1d_fwd_train: a batch of %d (training-mode statistics need more than one value per feature)", B);
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "bn1d_fwd_train_kernel", 0.0, 8.0 * (double)B * F);
  hipLaunchKernelGGL(bn1d_fwd_train_kernel, dim3((unsigned)ceil_div(F, 64)), dim3(256), 0, s, B, F, x, gamma, beta, running_mean,
                     running_var, momentum, eps, y, save2, (long long*)num_batches_tracked);
  return check_launch("bn1d_fwd_train");
}

extern "C" int avid_bn1d_fwd_eval(int B, int F, const float* x, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* y, float* save2, avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && F > 0 && x && y && running_mean && running_var, AVID_E_BADARG, "bn1d_fwd_eval: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "bn1d_fwd_eval_kernel", 0.0, 8.0 * (double)B * F);
  hipLaunchKernelGGL(bn1d_fwd_eval_kernel, dim3((unsigned)ceil_div(F, 64)), dim3(256), 0, s, B, F, x, gamma, beta, running_mean,
                     running_var, eps, y, save2);
  return check_launch("bn1d_fwd_eval");
}

extern "C" int avid_bn1d_bwd(int B, int F, const float* x, const float* dy, const float* gamma, const float* save2, float eps,
                             int frozen, float* dx, float* dgamma, float* dbeta, avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && F > 0 && x && dy && (save2 || !frozen) && (dx || dgamma || dbeta), AVID_E_BADARG, "bn1d_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "bn1d_bwd_kernel", 0.0, (dx ? 20.0 : 8.0) * (double)B * F);
  hipLaunchKernelGGL(bn1d_bwd_kernel, dim3((unsigned)ceil_div(F, 64)), dim3(256), 0, s, B, F, x, dy, gamma, save2, eps, frozen, dx,
                     dgamma, dbeta);
  return check_launch("bn1d_bwd");
}

static bool probe_linear_shape_ok(int B, int Fin, int C) { return B > 0 && B <= 256 && Fin > 0 && Fin <= 16384 && C > 0; }

extern "C" size_t avid_probe_linear_workspace_bytes(int B, int Fin, int C) {
  if (!probe_linear_shape_ok(B, Fin, C)) return 0;
  const size_t fwd = pg_slices(Fin) > 1 ? (size_t)pg_slices(Fin) * B * C : 0;
  const size_t dx = pg_slices(C) > 1 ? (size_t)pg_slices(C) * B * Fin : 0;
  return sizeof(float) * (fwd > dx ? fwd : dx);
}

extern "C" int avid_probe_linear_fwd(int B, int Fin, int C, const float* x, const float* w, const float* bias, float* y, void* ws,
                                     size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(x && w && y, AVID_E_BADARG, "probe_linear_fwd: bad arguments");
  AVID_REQUIRE(probe_linear_shape_ok(B, Fin, C), AVID_E_SHAPE, "probe_linear_fwd: B %d, Fin %d, C %d outside B <= 256, Fin <= 16384", B, Fin, C);
  return probe_gemm<true, true>("probe_gemm_kernel<true, true>", B, C, Fin, x, Fin, w, Fin, bias, y, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int avid_probe_linear_bwd(int B, int Fin, int C, const float* x, const float* w, const float* dy, float* dx, float* dw,
                                     float* db, void* ws, size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(x && w && dy && dw, AVID_E_BADARG, "probe_linear_bwd: bad arguments");
  AVID_REQUIRE(probe_linear_shape_ok(B, Fin, C), AVID_E_SHAPE, "probe_linear_bwd: B %d, Fin %d, C %d outside B <= 256, Fin <= 16384", B, Fin, C);
  hipStream_t s = (hipStream_t)stream;
  // dw [C][Fin] = dy^T . x: A(m = c, k = b) = dy[b][c], Bm(n = f, k = b) = x[b][f]; K = B <= 256: one slice
  int rc = probe_gemm<false, false>("probe_gemm_kernel<false, false>", C, Fin, B, dy, C, x, Fin, nullptr, dw, nullptr, 0, s);
  if (rc != AVID_OK) return rc;
  if (db) {
    ScopedTimer t(s, "probe_colsum_kernel", (double)B * C, 4.0 * ((double)B * C + C));
    hipLaunchKernelGGL(probe_colsum_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, s, B, C, dy, db);
    rc = check_launch("probe_colsum");
    if (rc != AVID_OK) return rc;
  }
  if (dx)   // dx [B][Fin] = dy . w: A(m = b, k = c) = dy[b][c], Bm(n = f, k = c) = w[c][f]
    rc = probe_gemm<true, false>("probe_gemm_kernel<true, false>", B, Fin, C, dy, C, w, Fin, nullptr, dx, ws, ws_bytes, s);
  return rc;
}
