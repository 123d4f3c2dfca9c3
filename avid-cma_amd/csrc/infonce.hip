// In-batch cross-modal InfoNCE (CLIP / GDT style) on the unit-norm embeddings of the GLOBAL batch: include/avid_hip.h,
// avid_infonce.  Three launches, no [G][G] matrix in memory, no floating-point atomics:
//
//   infonce_lse_kernel   grid (ceil(G / 64), 2 directions): a workgroup owns 64 query rows and walks the key tiles
//                        0, 64, 128, ... in order; every score is ONE accumulator fed by fmaf over d = 0 .. D-1 (so
//                        v_i . a_j has the same bits as a_j . v_i, wherever the pair sits in a tile); running
//                        maximum / rescaled sum per row (the row's true running maximum — never a fixed shift), the
//                        lowest index among the maxima, the diagonal score.  Writes lse[2][G], diag[G], hit[2][G].
//   infonce_grad_kernel  grid (ceil(b / 64), ceil(D / 128) column slabs, 2 directions): recomputes the score tile,
//                        forms the weights W from BOTH log-sum-exps (the query-role and the key-role term), and adds
//                        W . keys into one accumulator per output element, key index ascending 0 .. G-1.
//   infonce_final_kernel one workgroup, in double, index order: the two direction means, the total, the hit counts.
//
// The key tiles are cut at absolute key indices and nothing depends on where a query row sits in its tile, so the
// gradient rows and the loss have the same bits for every (row0, b), every grid and every CU budget (the kernels are not
// persistent: no grid is sized from the CU count).
#include <math.h>

#include "common.h"

// Only the fused multiply-adds written out below are fused: a score is the ROUNDED product acc * inv_T in both kernels (a
// contracted s - lse would subtract from the unrounded product, and G = 1 would no longer give exp(0) - 1 = 0 exactly).
#pragma clang fp contract(off)

namespace avid {
namespace {

constexpr int IN_QT = 64;          // query rows of a workgroup
constexpr int IN_KT = 64;          // keys of a tile
constexpr int IN_DC = 32;          // embedding columns staged per round
constexpr int IN_LDP = IN_DC + 4;  // row pitch of a staged chunk (floats): 16-byte rows, conflict-free 16-byte reads
constexpr int IN_SW = 128;         // output columns of a gradient workgroup
constexpr int IN_WP = IN_KT + 4;   // row pitch of the weight tile
constexpr int IN_NT = 256;

// rows [base, base + 64) x columns [d0, d0 + 32) of src[G][D] -> dst[64][IN_LDP]; rows past G - 1 read row G - 1
// (their scores are masked by the callers)
__device__ __forceinline__ void in_stage(float* dst, const float* __restrict__ src, int base, int G, int D, int d0, int tid) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int idx = tid + IN_NT * u, r = idx >> 3, q = idx & 7;
    int gr = base + r;
    gr = gr < G ? gr : G - 1;
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t)gr * D + d0 + 4 * q);
    *reinterpret_cast<float4*>(dst + r * IN_LDP + 4 * q) = v;
  }
}

// acc[a][e] = Q[q_base + 4 ty + a] . K[k_base + tx + 16 e], one accumulator per pair, d ascending.  Begins with a
// barrier (the staging buffers may still be read — also under their alias as the weight tile).
__device__ __forceinline__ void in_scores(float (&acc)[4][4], const float* __restrict__ Q, const float* __restrict__ K,
                                          int q_base, int k_base, int G, int D, float* Qc, float* Kc, int tid) {
  const int ty = tid >> 4, tx = tid & 15;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[a][e] = 0.f;
  for (int d0 = 0; d0 < D; d0 += IN_DC) {
    __syncthreads();
    in_stage(Qc, Q, q_base, G, D, d0, tid);
    in_stage(Kc, K, k_base, G, D, d0, tid);
    __syncthreads();
#pragma unroll
    for (int d = 0; d < IN_DC; d += 4) {
      float4 q[4], k[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) q[a] = *reinterpret_cast<const float4*>(Qc + (4 * ty + a) * IN_LDP + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) k[e] = *reinterpret_cast<const float4*>(Kc + (tx + 16 * e) * IN_LDP + d);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float s = acc[a][e];
          s = __builtin_fmaf(q[a].x, k[e].x, s);
          s = __builtin_fmaf(q[a].y, k[e].y, s);
          s = __builtin_fmaf(q[a].z, k[e].z, s);
          s = __builtin_fmaf(q[a].w, k[e].w, s);
          acc[a][e] = s;
        }
    }
  }
}

__global__ __launch_bounds__(IN_NT) void infonce_lse_kernel(const float* __restrict__ v, const float* __restrict__ a_, int G,
                                                            int D, float inv_T, float* __restrict__ lse,
                                                            float* __restrict__ diag, int* __restrict__ hit) {
  __shared__ __attribute__((aligned(16))) float Qc[IN_QT * IN_LDP];
  __shared__ __attribute__((aligned(16))) float Kc[IN_KT * IN_LDP];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, dir = blockIdx.y;
  const float* Q = dir ? a_ : v;
  const float* K = dir ? v : a_;
  const int q_base = blockIdx.x * IN_QT;
  float m[4], l[4];
  int am[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    m[a] = -INFINITY;
    l[a] = 0.f;
    am[a] = 0;
  }
  for (int k_base = 0; k_base < G; k_base += IN_KT) {
    float acc[4][4];
    in_scores(acc, Q, K, q_base, k_base, G, D, Qc, Kc, tid);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = q_base + 4 * ty + a;
      float s[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = k_base + tx + 16 * e;
        s[e] = c < G ? acc[a][e] * inv_T : -INFINITY;
        if (dir == 0 && c == row && row < G) diag[row] = s[e];
      }
      // the tile's maximum and the lowest key index that reaches it
      float tm = s[0];
      int ti = k_base + tx;
#pragma unroll
      for (int e = 1; e < 4; ++e)
        if (s[e] > tm) {
          tm = s[e];
          ti = k_base + tx + 16 * e;
        }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const float om = __shfl_xor(tm, o, 64);
        const int oi = __shfl_xor(ti, o, 64);
        if (om > tm || (om == tm && oi < ti)) {
          tm = om;
          ti = oi;
        }
      }
      if (tm > m[a]) am[a] = ti;          // strictly greater: an earlier tile keeps a tie
      const float mn = fmaxf(m[a], tm);
      float p = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) p += expf(s[e] - mn);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) p += __shfl_xor(p, o, 64);
      l[a] = l[a] * expf(m[a] - mn) + p;
      m[a] = mn;
    }
  }
  if (tx == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = q_base + 4 * ty + a;
      if (row < G) {
        lse[(size_t)dir * G + row] = m[a] + logf(l[a]);
        hit[(size_t)dir * G + row] = am[a] == row ? 1 : 0;
      }
    }
  }
}

__global__ __launch_bounds__(IN_NT) void infonce_grad_kernel(const float* __restrict__ v, const float* __restrict__ a_, int G,
                                                             int D, int row0, int b, float inv_T, float w_v2a, float w_a2v,
                                                             float scale, const float* __restrict__ lse,
                                                             float* __restrict__ dv, float* __restrict__ da) {
  // the staged chunks (2 x 64 x 36 floats) and, once the scores are in registers, the weight tile (64 x 68) share `buf`
  __shared__ __attribute__((aligned(16))) float buf[2 * IN_QT * IN_LDP];
  __shared__ __attribute__((aligned(16))) float Ks[IN_KT * IN_SW];
  static_assert(IN_QT * IN_WP <= 2 * IN_QT * IN_LDP, "the weight tile must fit the staging buffers");
  float* Qc = buf;
  float* Kc = buf + IN_QT * IN_LDP;
  float* Wt = buf;
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, dir = blockIdx.z;
  const float* Q = dir ? a_ : v;
  const float* K = dir ? v : a_;
  const float* lse_own = lse + (size_t)dir * G;
  const float* lse_oth = lse + (size_t)(1 - dir) * G;
  const float w_own = dir ? w_a2v : w_v2a, w_oth = dir ? w_v2a : w_a2v;
  float* out = dir ? da : dv;
  const int q_base = row0 + blockIdx.x * IN_QT, q_end = row0 + b, col0 = blockIdx.y * IN_SW;
  float own[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = q_base + 4 * ty + a;
    own[a] = lse_own[row < G ? row : G - 1];
  }
  float o[4][8];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int u = 0; u < 8; ++u) o[a][u] = 0.f;
  for (int k_base = 0; k_base < G; k_base += IN_KT) {
    float acc[4][4];
    in_scores(acc, Q, K, q_base, k_base, G, D, Qc, Kc, tid);
    __syncthreads();                       // every wave has read its last chunk: `buf` becomes the weight tile
#pragma unroll
    for (int u = 0; u < 8; ++u) {          // this slab's columns of the tile's keys (zeros past D)
      const int idx = tid + IN_NT * u, r = idx >> 5, col = col0 + 4 * (idx & 31);
      int gr = k_base + r;
      gr = gr < G ? gr : G - 1;
      float4 kv = {0.f, 0.f, 0.f, 0.f};
      if (col < D) kv = *reinterpret_cast<const float4*>(K + (size_t)gr * D + col);
      *reinterpret_cast<float4*>(Ks + r * IN_SW + 4 * (idx & 31)) = kv;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = k_base + tx + 16 * e;
      const float oth = lse_oth[c < G ? c : G - 1];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int row = q_base + 4 * ty + a;
        const float s = acc[a][e] * inv_T;
        // p - delta: on the diagonal through expm1 (a trained pair has p -> 1)
        const float t_own = c == row ? expm1f(s - own[a]) : expf(s - own[a]);
        const float t_oth = c == row ? expm1f(s - oth) : expf(s - oth);
        const float w = scale * (w_own * t_own + w_oth * t_oth);
        Wt[(4 * ty + a) * IN_WP + tx + 16 * e] = c < G ? w : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int c4 = 0; c4 < IN_KT; c4 += 4) {
      float4 w[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) w[a] = *reinterpret_cast<const float4*>(Wt + (4 * ty + a) * IN_WP + c4);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const float4 k0 = *reinterpret_cast<const float4*>(Ks + (c4 + cc) * IN_SW + 4 * tx);
        const float4 k1 = *reinterpret_cast<const float4*>(Ks + (c4 + cc) * IN_SW + 64 + 4 * tx);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const float wv = cc == 0 ? w[a].x : cc == 1 ? w[a].y : cc == 2 ? w[a].z : w[a].w;
          o[a][0] = __builtin_fmaf(wv, k0.x, o[a][0]);
          o[a][1] = __builtin_fmaf(wv, k0.y, o[a][1]);
          o[a][2] = __builtin_fmaf(wv, k0.z, o[a][2]);
          o[a][3] = __builtin_fmaf(wv, k0.w, o[a][3]);
          o[a][4] = __builtin_fmaf(wv, k1.x, o[a][4]);
          o[a][5] = __builtin_fmaf(wv, k1.y, o[a][5]);
          o[a][6] = __builtin_fmaf(wv, k1.z, o[a][6]);
          o[a][7] = __builtin_fmaf(wv, k1.w, o[a][7]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = q_base + 4 * ty + a;
    if (row >= q_end) continue;
    float* dst = out + (size_t)(row - row0) * D + col0;
    if (col0 + 4 * tx < D) *reinterpret_cast<float4*>(dst + 4 * tx) = make_float4(o[a][0], o[a][1], o[a][2], o[a][3]);
    if (col0 + 64 + 4 * tx < D) *reinterpret_cast<float4*>(dst + 64 + 4 * tx) = make_float4(o[a][4], o[a][5], o[a][6], o[a][7]);
  }
}

__global__ __launch_bounds__(IN_NT) void infonce_final_kernel(int G, const float* __restrict__ lse, const float* __restrict__ diag,
                                                              const int* __restrict__ hit, float w_v2a, float w_a2v,
                                                              float* __restrict__ loss, long long* __restrict__ hits) {
  __shared__ double sd[2][IN_NT];
  __shared__ long long sh[2][IN_NT];
  const int tid = threadIdx.x;
  double sv = 0.0, sa = 0.0;
  long long hv = 0, ha = 0;
  for (int i = tid; i < G; i += IN_NT) {
    const double dg = (double)diag[i];
    sv += (double)lse[i] - dg;
    sa += (double)lse[(size_t)G + i] - dg;
    hv += hit[i];
    ha += hit[(size_t)G + i];
  }
  sd[0][tid] = sv;
  sd[1][tid] = sa;
  sh[0][tid] = hv;
  sh[1][tid] = ha;
  __syncthreads();
  for (int st = IN_NT / 2; st > 0; st >>= 1) {
    if (tid < st) {
      sd[0][tid] += sd[0][tid + st];
      sd[1][tid] += sd[1][tid + st];
      sh[0][tid] += sh[0][tid + st];
      sh[1][tid] += sh[1][tid + st];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double lv = sd[0][0] / (double)G, la = sd[1][0] / (double)G;
    loss[0] = (float)((double)w_v2a * lv + (double)w_a2v * la);
    loss[1] = (float)lv;
    loss[2] = (float)la;
    if (hits) {
      hits[0] = sh[0][0];
      hits[1] = sh[1][0];
    }
  }
}

inline size_t in_ws_bytes(int G) {       // lse[2][G], diag[G] (float) + hit[2][G] (int32), rounded up to 256 bytes
  return ((size_t)G * 20 + 255) / 256 * 256;
}

}  // namespace
}  // namespace avid

using namespace avid;

extern "C" size_t avid_infonce_workspace_bytes(int G) { return G >= 1 ? in_ws_bytes(G) : 0; }

extern "C" int avid_infonce(int G, int D, int row0, int b, const float* v_hat, const float* a_hat, float inv_T, float w_v2a,
                            float w_a2v, float grad_scale, float* loss, int64_t* hits, float* dv, float* da, void* ws,
                            size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(G >= 1 && row0 >= 0 && b >= 0 && (long long)row0 + b <= G, AVID_E_BADARG,
               "infonce: rows [%d, %d + %d) outside the global batch of %d", row0, row0, b, G);
  AVID_REQUIRE(D >= 32 && D <= 512 && D % 32 == 0, AVID_E_UNSUPPORTED, "infonce: D = %d (a multiple of 32 up to 512 expected)", D);
  AVID_REQUIRE(v_hat && a_hat && loss && ws, AVID_E_BADARG, "infonce: null pointer");
  AVID_REQUIRE((dv == nullptr) == (da == nullptr), AVID_E_BADARG, "infonce: dv and da are given together or not at all");
  AVID_REQUIRE(((uintptr_t)v_hat | (uintptr_t)a_hat | (uintptr_t)dv | (uintptr_t)da) % 16 == 0 && (uintptr_t)ws % 8 == 0,
               AVID_E_BADARG, "infonce: embeddings and gradients must be 16-byte aligned, the workspace 8-byte aligned");
  AVID_REQUIRE(inv_T > 0.f && inv_T < INFINITY && w_v2a >= 0.f && w_v2a < INFINITY && w_a2v >= 0.f && w_a2v < INFINITY,
               AVID_E_BADARG, "infonce: 1 / T = %g, weights (%g, %g): finite, 1 / T > 0 and weights >= 0 expected",
               (double)inv_T, (double)w_v2a, (double)w_a2v);
  AVID_REQUIRE(ws_bytes >= in_ws_bytes(G), AVID_E_BADARG, "infonce: workspace of %zu bytes, %zu needed", ws_bytes,
               in_ws_bytes(G));
  hipStream_t s = (hipStream_t)stream;
  float* lse = (float*)ws;
  float* diag = lse + 2 * (size_t)G;
  int* hit = (int*)(diag + G);
  const int qt = (int)ceil_div(G, IN_QT);
  const double gg = (double)G * G * D;
  {
    ScopedTimer t(s, "infonce_lse_kernel", 4.0 * gg, 8.0 * G * D * (1.0 + qt));
    hipLaunchKernelGGL(infonce_lse_kernel, dim3(qt, 2), dim3(IN_NT), 0, s, v_hat, a_hat, G, D, inv_T, lse, diag, hit);
  }
  int rc = check_launch("infonce (lse)");
  if (rc != AVID_OK) return rc;
  if (dv && b > 0) {
    const int bt = (int)ceil_div(b, IN_QT), slabs = (int)ceil_div(D, IN_SW);
    const float scale = grad_scale * inv_T / (float)G;
    ScopedTimer t(s, "infonce_grad_kernel", 4.0 * (double)b * G * D * (1.0 + slabs), 8.0 * G * D * bt * slabs + 8.0 * b * D);
    hipLaunchKernelGGL(infonce_grad_kernel, dim3(bt, slabs, 2), dim3(IN_NT), 0, s, v_hat, a_hat, G, D, row0, b, inv_T, w_v2a,
                       w_a2v, scale, lse, dv, da);
    rc = check_launch("infonce (gradient)");
    if (rc != AVID_OK) return rc;
  }
  ScopedTimer t(s, "infonce_final_kernel", 0.0, 20.0 * G);
  hipLaunchKernelGGL(infonce_final_kernel, dim3(1), dim3(IN_NT), 0, s, G, lse, diag, hit, w_v2a, w_a2v, loss, (long long*)hits);
  return check_launch("infonce (final)");
}
