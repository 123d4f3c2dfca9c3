// Action-recognition fine-tuning head: dropout and the classifier's softmax cross-entropy / clip-averaged confidence, and its
// multi-label sibling (binary cross-entropy with logits: the reference has no multi-label code; torch's expression is the contract),
// and the softmax cross-entropy against a distribution (label smoothing, mixup / CutMix targets, distillation; torch's again).
//
// Reference ops replaced: utils/eval_utils.py:203-213 (torch.nn.Dropout inside ClassificationWrapper),
// eval-action-recg.py:150-165 (CrossEntropyLoss, Softmax, .view(V, clips, -1).mean(1), metrics_utils.accuracy top-1 / top-5).
// The classifier Linear(F, C) has kernels of its own below: the heads' igemm (avid_conv_fwd) takes C in multiples of 64 only.
// No MFMA: the head is a few MFLOP per step; what matters is that it costs few launches and no host synchronisation.
#include <math.h>

#include <atomic>

#include "common.h"

namespace avid {

// ---------------------------------------------------------------------------------------------
// Dropout.  Element i (= b * F + f) is kept iff word i % 4 of Philox4x32-10(counter = (i/4 lo, i/4 hi, off lo, off hi),
// key = seed) is >= thresh = floor(p * 2^32); y = kept ? x * scale : 0, scale = 1 / (1 - p) in fp32.  One thread per four
// consecutive elements (one Philox call), the keep-mask stored as one byte per element for the backward.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_fwd_kernel(long long n, const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ mask, uint32_t thresh, float scale,
                                                          uint64_t seed, uint64_t offset,
                                                          const unsigned long long* __restrict__ offset_dev) {
  if (offset_dev) offset = *offset_dev;
  const long long groups = (n + 3) >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r[0], r[1], r[2], r[3]);
    const long long i0 = g << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i0 + j;
      if (i < n) {
        const bool keep = r[j] >= thresh;
        y[i] = keep ? x[i] * scale : 0.f;
        mask[i] = keep ? 1 : 0;
      }
    }
  }
}

__global__ __launch_bounds__(256) void dropout_bwd_kernel(long long n, const uint8_t* __restrict__ mask,
                                                          const float* __restrict__ dy, float* __restrict__ dx, float scale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dx[i] = mask[i] ? dy[i] * scale : 0.f;
}

// ---------------------------------------------------------------------------------------------
// Softmax cross-entropy over logits [V * clips][C] (C <= 1024), labels [V]: one block of CLS_WAVES waves, wave w takes the
// videos w, w + CLS_WAVES, ... and each of their clips' rows in order (three passes over a row: max, sum of exponentials,
// probabilities; lane l owns columns l, l + 64, ... and accumulates their confidence in its wave's slice of LDS).  Per video:
// the confidence (mean over its clips of the softmax), the rank of its label in it, the sum of its rows' cross-entropies.
// The wave sums its videos' terms in order (double), the block sums the waves' in order: a fixed summation order and no
// atomics on the results, so every output is bit-reproducible.
// ---------------------------------------------------------------------------------------------
constexpr int CLS_WAVES = 16;
constexpr int CLS_MAX_C = 1024;

__global__ __launch_bounds__(CLS_WAVES * 64) void cls_loss_kernel(int V, int clips, int C, const float* __restrict__ logits,
                                                                  const long long* __restrict__ labels, float grad_scale,
                                                                  float* __restrict__ loss, float* __restrict__ conf,
                                                                  long long* __restrict__ hits, float* __restrict__ dlogits,
                                                                  int* __restrict__ err) {
  __shared__ float s_acc[CLS_WAVES][CLS_MAX_C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* acc = s_acc[wave];
  const long long rows = (long long)V * clips;
  const float dscale = grad_scale / (float)rows;
  const float inv_clips = 1.f / (float)clips;
  double wloss = 0.0;
  long long wtop1 = 0, wtop5 = 0;
  for (int v = wave; v < V; v += CLS_WAVES) {
    const long long lab = labels[v];
    const bool bad = lab < 0 || lab >= C;
    if (bad && err && lane == 0) atomicOr(err, AVID_DEVERR_CLS_LABEL);
    const int label = bad ? 0 : (int)lab;
    for (int c = lane; c < C; c += 64) acc[c] = 0.f;
    double vloss = 0.0;
    for (int k = 0; k < clips; ++k) {
      const long long row = (long long)v * clips + k;
      const float* src = logits + row * C;
      float m = -INFINITY;
      for (int c = lane; c < C; c += 64) m = fmaxf(m, src[c]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      float s = 0.f;
      for (int c = lane; c < C; c += 64) s += expf(src[c] - m);
      s = wave_sum(s);
      const float inv_s = 1.f / s;
      vloss += (double)(logf(s) + m - src[label]);
      for (int c = lane; c < C; c += 64) {
        const float pr = expf(src[c] - m) * inv_s;
        acc[c] += pr;
        if (dlogits) dlogits[row * C + c] = (pr - (c == label ? 1.f : 0.f)) * dscale;
      }
    }
    // confidence, and the label's rank in it: classes with strictly greater confidence, plus equal confidence at a lower index
    // (a lane reads back only the columns it wrote itself, and the label's column, written by lane label % 64 of this wave)
    int above = 0;
    for (int c = lane; c < C; c += 64) acc[c] *= inv_clips;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const float cl = acc[label];
    for (int c = lane; c < C; c += 64) {
      const float a = acc[c];
      if (conf) conf[(long long)v * C + c] = a;
      above += (a > cl || (a == cl && c < label)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (!bad) {
      wtop1 += above < 1 ? 1 : 0;
      wtop5 += above < 5 ? 1 : 0;
    }
    wloss += vloss;
    __builtin_amdgcn_wave_barrier();     // every lane has read acc[label] before the next video clears it
  }
  __shared__ double s_loss[CLS_WAVES];
  __shared__ long long s_hits[2][CLS_WAVES];
  if (lane == 0) {
    s_loss[wave] = wloss;
    s_hits[0][wave] = wtop1;
    s_hits[1][wave] = wtop5;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    long long h1 = 0, h5 = 0;
    for (int w = 0; w < CLS_WAVES; ++w) {
      t += s_loss[w];
      h1 += s_hits[0][w];
      h5 += s_hits[1][w];
    }
    if (loss) loss[0] = (float)(t / (double)rows);
    if (hits) {
      hits[0] = h1;
      hits[1] = h5;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Multi-label loss: binary cross-entropy with logits over logits [V * clips][C] (C <= 1024) against targets [V][C], torch's
// expression l = (1 - t) x + w (log1p(exp(-|x|)) + max(-x, 0)), w = 1 + (pos_weight_c - 1) t.  A dense evaluation hands
// this kernel 10^7 elements, so it is a grid: workgroup g takes the videos g, g + G, ... (G = min(V, ML_MAX_GRID), a
// function of V alone), thread i the columns i, i + 256, ... of each and all of that video's clips (the clip sum of the
// sigmoids stays in a register).  A thread sums its elements' losses in double, in the order it meets them; the workgroup
// sums its threads' (wave butterfly, then the waves in order) into one MlPart; mlabel_final_kernel sums the G parts in
// index order.  No floating-point atomics, nothing depends on the CU count: the same bits on every run.
// Both tails of the sigmoid come from e = exp(-|x|): 1 / (1 + e) and e / (1 + e), so 1 - sigmoid(x) does not cancel.
// The parts live in one of ML_RING slabs of device memory owned by the library, drawn round-robin per call (the event
// pool's contract, program.hip): a slab is written again after ML_RING further calls on the same device.
// ---------------------------------------------------------------------------------------------
constexpr int ML_THREADS = 256;
constexpr int ML_COLS = CLS_MAX_C / ML_THREADS;
constexpr int ML_MAX_GRID = 1024;
constexpr int ML_RING = 16;

struct MlPart {
  double loss;
  long long top, pairs, pad;
};
__device__ MlPart g_ml_part[ML_RING][ML_MAX_GRID];

__global__ __launch_bounds__(ML_THREADS) void mlabel_loss_kernel(int V, int clips, int C, const float* __restrict__ logits,
                                                                 const float* __restrict__ targets,
                                                                 const float* __restrict__ pos_weight, float grad_scale,
                                                                 float* __restrict__ conf, float* __restrict__ dlogits,
                                                                 int* __restrict__ err, MlPart* __restrict__ part) {
  __shared__ float s_bv[ML_THREADS / 64];
  __shared__ int s_bi[ML_THREADS / 64], s_bt[ML_THREADS / 64];
  __shared__ double s_loss[ML_THREADS / 64];
  __shared__ long long s_pairs[ML_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float dscale = grad_scale / (float)((long long)V * clips * C);
  double tloss = 0.0;
  long long tpairs = 0, top = 0;      // (top: thread 0's)
  bool bad = false;
  for (int v = blockIdx.x; v < V; v += gridDim.x) {
    float bv = -INFINITY;
    int bi = 0x7fffffff, bt = 0;
#pragma unroll
    for (int j = 0; j < ML_COLS; ++j) {
      const int c = tid + j * ML_THREADS;
      if (c >= C) break;
      const float t = targets[(long long)v * C + c];
      bad = bad || !(t >= 0.f && t <= 1.f);
      const float w = 1.f + ((pos_weight ? pos_weight[c] : 1.f) - 1.f) * t, a = 1.f - t;
      float acc = 0.f;
      for (int k = 0; k < clips; ++k) {
        const long long o = ((long long)v * clips + k) * C + c;
        const float x = logits[o];
        const float e = expf(-fabsf(x));
        tloss += (double)(a * x + w * (log1pf(e) + fmaxf(-x, 0.f)));
        const float r = 1.f / (1.f + e), er = e * r;
        acc += x >= 0.f ? r : er;
        if (dlogits) dlogits[o] = (a - w * (x >= 0.f ? er : r)) * dscale;
      }
      const float cf = acc / (float)clips;
      if (conf) conf[(long long)v * C + c] = cf;
      const int tp = t >= 0.5f ? 1 : 0;
      tpairs += ((cf >= 0.5f ? 1 : 0) == tp) ? 1 : 0;
      if (cf > bv) {                  // (a thread meets its columns in ascending order: strict > keeps the lower index)
        bv = cf;
        bi = c;
        bt = tp;
      }
    }
    // the video's highest-confidence class, ties to the lower index: lanes, then the waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
        bt = ot;
      }
    }
    if (lane == 0) {
      s_bv[wave] = bv;
      s_bi[wave] = bi;
      s_bt[wave] = bt;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w2 = 1; w2 < ML_THREADS / 64; ++w2)
        if (s_bv[w2] > bv || (s_bv[w2] == bv && s_bi[w2] < bi)) {
          bv = s_bv[w2];
          bi = s_bi[w2];
          bt = s_bt[w2];
        }
      top += bt;
    }
    __syncthreads();
  }
  if (bad && err) atomicOr(err, AVID_DEVERR_MLABEL_TARGET);
  tloss = wave_sum_d(tloss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tpairs += __shfl_xor(tpairs, o, 64);
  if (lane == 0) {
    s_loss[wave] = tloss;
    s_pairs[wave] = tpairs;
  }
  __syncthreads();
  if (tid == 0) {
    double l = 0.0;
    long long p = 0;
    for (int w2 = 0; w2 < ML_THREADS / 64; ++w2) {
      l += s_loss[w2];
      p += s_pairs[w2];
    }
    part[blockIdx.x].loss = l;
    part[blockIdx.x].top = top;
    part[blockIdx.x].pairs = p;
  }
}

// The G parts in index order: lane i sums the parts [16 i, 16 i + 16) in order, lane 0 the lanes' sums in order.
__global__ __launch_bounds__(64) void mlabel_final_kernel(int G, const MlPart* __restrict__ part, double elems,
                                                          float* __restrict__ loss, long long* __restrict__ hits) {
  __shared__ double s_l[64];
  __shared__ long long s_h[2][64];
  constexpr int PER = ML_MAX_GRID / 64;
  const int lane = threadIdx.x;
  double l = 0.0;
  long long h0 = 0, h1 = 0;
  for (int g = lane * PER; g < min(G, lane * PER + PER); ++g) {
    l += part[g].loss;
    h0 += part[g].top;
    h1 += part[g].pairs;
  }
  s_l[lane] = l;
  s_h[0][lane] = h0;
  s_h[1][lane] = h1;
  __syncthreads();
  if (lane == 0) {
    l = 0.0;
    h0 = h1 = 0;
    for (int i = 0; i < 64; ++i) {
      l += s_l[i];
      h0 += s_h[0][i];
      h1 += s_h[1][i];
    }
    if (loss) loss[0] = (float)(l / elems);
    if (hits) {
      hits[0] = h0;
      hits[1] = h1;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Soft-target softmax cross-entropy: logits [V * clips][C] (C <= 1024) against a DISTRIBUTION per video, targets [V][C] —
// torch's F.cross_entropy(logits, target_probs, label_smoothing = eps), mean reduction: t' = t (1 - eps) + eps / C, row loss
// = sum_c t'[c] (lse(row) - x[c]), d/dx[c] = softmax[c] * S - t'[c] with S = sum_c t'[c] (the targets are NOT renormalised,
// as torch does not).  mlabel_loss_kernel's shape: workgroup g takes the videos g, g + G, ... (G = min(V, ML_MAX_GRID)),
// thread i the columns i, i + 256, ... (in registers: a row is read once); per video one workgroup reduction for S, the
// argmax of the targets (the video's label; ties to the lower index) and the validity of the row, per clip row one for the
// max and one for the sum of exponentials (log-softmax goes through the row max), then one for the label's rank in the
// confidence (cls_loss_kernel's rule).  A workgroup reduction is a wave butterfly, then the waves in order: every float sum
// has one fixed order.  The element losses are added in double per thread in the order met, the threads' sums as in
// mlabel_loss_kernel into one MlPart (top = top-1 hits, pairs = top-5 hits), and mlabel_final_kernel adds the parts in
// index order out of a slab of the same ring.  No floating-point atomics; the same bits on every run.
// A video with a negative or non-finite target sets AVID_DEVERR_SOFT_TARGET and counts no hit.
// ---------------------------------------------------------------------------------------------
constexpr int SC_WAVES = ML_THREADS / 64;

__device__ __forceinline__ float sc_block_sum(float v, float* s, int lane, int wave) {
  v = wave_sum(v);
  if (lane == 0) s[wave] = v;
  __syncthreads();
  float r = s[0];
#pragma unroll
  for (int w = 1; w < SC_WAVES; ++w) r += s[w];
  return r;
}

__global__ __launch_bounds__(ML_THREADS) void soft_ce_loss_kernel(int V, int clips, int C, const float* __restrict__ logits,
                                                                  const float* __restrict__ targets, float eps, float grad_scale,
                                                                  float* __restrict__ conf, float* __restrict__ dlogits,
                                                                  int* __restrict__ err, MlPart* __restrict__ part) {
  // one slot per reduction site: a slot is written again only behind a later site's barrier, which every reader has reached
  __shared__ float s_sum[SC_WAVES], s_tv[SC_WAVES], s_max[SC_WAVES], s_den[SC_WAVES], s_cl;
  __shared__ int s_ti[SC_WAVES], s_above[SC_WAVES];
  __shared__ double s_loss[SC_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float dscale = grad_scale / (float)((long long)V * clips);
  const float keep = 1.f - eps, spread = eps / (float)C, inv_clips = 1.f / (float)clips;
  double tloss = 0.0;
  long long top1 = 0, top5 = 0;      // (thread 0's)
  bool bad = false;
  for (int v = blockIdx.x; v < V; v += gridDim.x) {
    float tp[ML_COLS], acc[ML_COLS];
    float ssum = 0.f, bv = -INFINITY;
    int bi = 0x7fffffff;
    bool vbad = false;
#pragma unroll
    for (int j = 0; j < ML_COLS; ++j) {
      const int c = tid + j * ML_THREADS;
      tp[j] = acc[j] = 0.f;
      if (c < C) {
        const float t = targets[(long long)v * C + c];
        vbad = vbad || !(t >= 0.f && t < INFINITY);
        tp[j] = fmaf(t, keep, spread);
        ssum += tp[j];
        if (t > bv) {                 // (ascending columns: strict > keeps the lower index)
          bv = t;
          bi = c;
        }
      }
    }
    const float S = sc_block_sum(ssum, s_sum, lane, wave);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_tv[wave] = bv;
      s_ti[wave] = bi;
    }
    vbad = __syncthreads_or(vbad ? 1 : 0) != 0;
    bv = s_tv[0];
    bi = s_ti[0];
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w)
      if (s_tv[w] > bv || (s_tv[w] == bv && s_ti[w] < bi)) {
        bv = s_tv[w];
        bi = s_ti[w];
      }
    bad = bad || vbad;
    const int label = (vbad || bi >= C) ? -1 : bi;
    for (int k = 0; k < clips; ++k) {
      const long long row = (long long)v * clips + k;
      float x[ML_COLS], m = -INFINITY;
#pragma unroll
      for (int j = 0; j < ML_COLS; ++j) {
        const int c = tid + j * ML_THREADS;
        x[j] = c < C ? logits[row * C + c] : -INFINITY;
        m = fmaxf(m, x[j]);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      if (lane == 0) s_max[wave] = m;
      __syncthreads();
      m = s_max[0];
#pragma unroll
      for (int w = 1; w < SC_WAVES; ++w) m = fmaxf(m, s_max[w]);
      float e[ML_COLS], den = 0.f;
#pragma unroll
      for (int j = 0; j < ML_COLS; ++j) {
        e[j] = tid + j * ML_THREADS < C ? expf(x[j] - m) : 0.f;
        den += e[j];
      }
      den = sc_block_sum(den, s_den, lane, wave);
      const float lse = logf(den) + m, inv_den = 1.f / den;
#pragma unroll
      for (int j = 0; j < ML_COLS; ++j) {
        const int c = tid + j * ML_THREADS;
        if (c < C) {
          tloss += (double)(tp[j] * (lse - x[j]));
          const float pr = e[j] * inv_den;
          acc[j] += pr;
          if (dlogits) dlogits[row * C + c] = (pr * S - tp[j]) * dscale;
        }
      }
    }
    // the confidence, and the label's rank in it: classes strictly above, plus equal ones at a lower index
#pragma unroll
    for (int j = 0; j < ML_COLS; ++j) {
      const int c = tid + j * ML_THREADS;
      acc[j] *= inv_clips;
      if (c < C) {
        if (conf) conf[(long long)v * C + c] = acc[j];
        if (c == label) s_cl = acc[j];
      }
    }
    __syncthreads();
    const float cl = s_cl;
    int above = 0;
#pragma unroll
    for (int j = 0; j < ML_COLS; ++j) {
      const int c = tid + j * ML_THREADS;
      if (c < C && label >= 0) above += (acc[j] > cl || (acc[j] == cl && c < label)) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o, 64);
    if (lane == 0) s_above[wave] = above;
    __syncthreads();
    if (tid == 0 && label >= 0) {
      above = 0;
      for (int w = 0; w < SC_WAVES; ++w) above += s_above[w];
      top1 += above < 1 ? 1 : 0;
      top5 += above < 5 ? 1 : 0;
    }
  }
  if (bad && err && tid == 0) atomicOr(err, AVID_DEVERR_SOFT_TARGET);
  tloss = wave_sum_d(tloss);
  if (lane == 0) s_loss[wave] = tloss;
  __syncthreads();
  if (tid == 0) {
    double l = 0.0;
    for (int w = 0; w < SC_WAVES; ++w) l += s_loss[w];
    part[blockIdx.x].loss = l;
    part[blockIdx.x].top = top1;
    part[blockIdx.x].pairs = top5;
  }
}

// ---------------------------------------------------------------------------------------------
// The classifier Linear(F, C) for any C (the heads' igemm takes C in multiples of 64; 101 / 51 classes are not).
// Forward: one wave per output (b, c), a dot product over F.  Backward: one thread per dW / db / dx element, each a sum
// over the batch (dW, db) or over the classes (dx) in index order.  Deterministic; a few MFLOP per step.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cls_linear_fwd_kernel(int B, int Fin, int C, const float* __restrict__ x,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= (long long)B * C) return;
  const int b = (int)(o / C), c = (int)(o % C);
  const float* xr = x + (long long)b * Fin;
  const float* wr = w + (long long)c * Fin;
  float acc = 0.f;
  for (int f = lane; f < Fin; f += 64) acc = fmaf(xr[f], wr[f], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[o] = acc + (bias ? bias[c] : 0.f);
}

__global__ __launch_bounds__(256) void cls_linear_bwd_kernel(int B, int Fin, int C, const float* __restrict__ x,
                                                             const float* __restrict__ w, const float* __restrict__ dy,
                                                             float* __restrict__ dx, float* __restrict__ dw,
                                                             float* __restrict__ db) {
  const long long nw = (long long)C * Fin, nb = C, nx = dx ? (long long)B * Fin : 0;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nw + nb + nx; i += stride) {
    if (i < nw) {
      const int c = (int)(i / Fin), f = (int)(i % Fin);
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc = fmaf(dy[(long long)b * C + c], x[(long long)b * Fin + f], acc);
      dw[i] = acc;
    } else if (i < nw + nb) {
      const int c = (int)(i - nw);
      float acc = 0.f;
      for (int b = 0; b < B; ++b) acc += dy[(long long)b * C + c];
      if (db) db[c] = acc;
    } else {
      const long long j = i - nw - nb;
      const int b = (int)(j / Fin), f = (int)(j % Fin);
      float acc = 0.f;
      for (int c = 0; c < C; ++c) acc = fmaf(dy[(long long)b * C + c], w[(long long)c * Fin + f], acc);
      dx[j] = acc;
    }
  }
}

}  // namespace avid

using namespace avid;

extern "C" int avid_cls_linear_fwd(int B, int Fin, int C, const float* x, const float* w, const float* bias, float* y,
                                   avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && Fin > 0 && C > 0 && x && w && y, AVID_E_BADARG, "cls_linear_fwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long long outs = (long long)B * C;
  ScopedTimer t(s, "cls_linear_fwd_kernel", 2.0 * outs * Fin, 4.0 * ((double)B * Fin + (double)C * Fin + outs));
  hipLaunchKernelGGL(cls_linear_fwd_kernel, dim3((unsigned)ceil_div(outs, 4)), dim3(256), 0, s, B, Fin, C, x, w, bias, y);
  return check_launch("cls_linear_fwd");
}

extern "C" int avid_cls_linear_bwd(int B, int Fin, int C, const float* x, const float* w, const float* dy, float* dx, float* dw,
                                   float* db, avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && Fin > 0 && C > 0 && x && w && dy && dw, AVID_E_BADARG, "cls_linear_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)C * Fin + C + (dx ? (long long)B * Fin : 0);
  long long g = ceil_div(n, 256);
  if (g > 4096) g = 4096;
  ScopedTimer t(s, "cls_linear_bwd_kernel", 2.0 * B * (double)C * Fin * (dx ? 2.0 : 1.0), 4.0 * (double)n);
  hipLaunchKernelGGL(cls_linear_bwd_kernel, dim3((unsigned)g), dim3(256), 0, s, B, Fin, C, x, w, dy, dx, dw, db);
  return check_launch("cls_linear_bwd");
}

static uint32_t dropout_threshold(float p) { return (uint32_t)floor((double)p * 4294967296.0); }

extern "C" int avid_dropout_fwd(int64_t B, int64_t F, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                const float* x, float* y, uint8_t* mask, avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && F > 0 && x && y && mask, AVID_E_BADARG, "dropout_fwd: bad arguments");
  AVID_REQUIRE(p >= 0.f && p < 1.f, AVID_E_BADARG, "dropout_fwd: p = %g outside [0, 1)", (double)p);
  const long long n = (long long)B * F;
  long long g = ceil_div(ceil_div(n, 4), 256);
  if (g > 4096) g = 4096;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "dropout_fwd_kernel", 0.0, 9.0 * n);
  hipLaunchKernelGGL(dropout_fwd_kernel, dim3((unsigned)g), dim3(256), 0, s, n, x, y, mask, dropout_threshold(p),
                     1.0f / (1.0f - p), seed, offset, (const unsigned long long*)offset_dev);
  return check_launch("dropout_fwd");
}

extern "C" int avid_dropout_bwd(int64_t n, float p, const uint8_t* mask, const float* dy, float* dx, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && mask && dy && dx, AVID_E_BADARG, "dropout_bwd: bad arguments");
  AVID_REQUIRE(p >= 0.f && p < 1.f, AVID_E_BADARG, "dropout_bwd: p = %g outside [0, 1)", (double)p);
  long long g = ceil_div(n, 256);
  if (g > 4096) g = 4096;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer t(s, "dropout_bwd_kernel", 0.0, 9.0 * n);
  hipLaunchKernelGGL(dropout_bwd_kernel, dim3((unsigned)g), dim3(256), 0, s, (long long)n, mask, dy, dx, 1.0f / (1.0f - p));
  return check_launch("dropout_bwd");
}

extern "C" int avid_cls_loss(int V, int clips, int C, const float* logits, const int64_t* labels, float grad_scale,
                             float* loss, float* conf, int64_t* hits, float* dlogits, int32_t* err, avid_stream_t stream) {
  AVID_REQUIRE(V > 0 && clips > 0 && C > 0 && C <= CLS_MAX_C && logits && labels, AVID_E_BADARG,
               "cls_loss: bad arguments (V %d, clips %d, C %d: C must be in [1, %d])", V, clips, C, CLS_MAX_C);
  hipStream_t s = (hipStream_t)stream;
  const double elems = (double)V * clips * C;
  ScopedTimer t(s, "cls_loss_kernel", 0.0, elems * (dlogits ? 8.0 : 4.0));
  hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(CLS_WAVES * 64), 0, s, V, clips, C, logits, (const long long*)labels,
                     grad_scale, loss, conf, (long long*)hits, dlogits, err);
  return check_launch("cls_loss");
}

// The next slab of the ring of partial sums (avid_mlabel_loss and avid_soft_ce_loss draw from the one ring), or nullptr.
static MlPart* ml_next_slab(const char* who) {
  static std::atomic<unsigned> ring{0};
  MlPart* slabs = nullptr;
  hipError_t he = hipGetSymbolAddress(reinterpret_cast<void**>(&slabs), HIP_SYMBOL(g_ml_part));
  if (he != hipSuccess) {
    set_error("%s: %s", who, hipGetErrorString(he));
    return nullptr;
  }
  return slabs + (size_t)(ring.fetch_add(1) % ML_RING) * ML_MAX_GRID;
}

extern "C" int avid_mlabel_loss(int V, int clips, int C, const float* logits, const float* targets, const float* pos_weight,
                                float grad_scale, float* loss, float* conf, int64_t* hits, float* dlogits, int32_t* err,
                                avid_stream_t stream) {
  AVID_REQUIRE(V > 0 && clips > 0 && C > 0 && C <= CLS_MAX_C && logits && targets && loss, AVID_E_BADARG,
               "mlabel_loss: bad arguments (V %d, clips %d, C %d: C must be in [1, %d])", V, clips, C, CLS_MAX_C);
  MlPart* part = ml_next_slab("mlabel_loss");
  if (!part) return AVID_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int G = V < ML_MAX_GRID ? V : ML_MAX_GRID;
  const double elems = (double)V * clips * C;
  {
    ScopedTimer t(s, "mlabel_loss_kernel", 0.0, elems * (dlogits ? 8.0 : 4.0) + 4.0 * (double)V * C * (conf ? 2.0 : 1.0));
    hipLaunchKernelGGL(mlabel_loss_kernel, dim3(G), dim3(ML_THREADS), 0, s, V, clips, C, logits, targets, pos_weight, grad_scale,
                       conf, dlogits, err, part);
  }
  int rc = check_launch("mlabel_loss");
  if (rc != AVID_OK) return rc;
  ScopedTimer t(s, "mlabel_final_kernel", 0.0, 32.0 * G);
  hipLaunchKernelGGL(mlabel_final_kernel, dim3(1), dim3(64), 0, s, G, part, elems, loss, (long long*)hits);
  return check_launch("mlabel_loss (final)");
}

extern "C" int avid_soft_ce_loss(int V, int clips, int C, const float* logits, const float* targets, float label_smoothing,
                                 float grad_scale, float* loss, float* conf, int64_t* hits, float* dlogits, int32_t* err,
                                 avid_stream_t stream) {
  AVID_REQUIRE(V > 0 && clips > 0 && C > 0 && C <= CLS_MAX_C && logits && targets && loss, AVID_E_BADARG,
               "soft_ce_loss: bad arguments (V %d, clips %d, C %d: C must be in [1, %d])", V, clips, C, CLS_MAX_C);
  AVID_REQUIRE(label_smoothing >= 0.f && label_smoothing < 1.f, AVID_E_BADARG, "soft_ce_loss: label_smoothing = %g outside [0, 1)",
               (double)label_smoothing);
  MlPart* part = ml_next_slab("soft_ce_loss");
  if (!part) return AVID_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  const int G = V < ML_MAX_GRID ? V : ML_MAX_GRID;
  const double rows = (double)V * clips, elems = rows * C;
  {
    ScopedTimer t(s, "soft_ce_loss_kernel", 0.0, elems * (dlogits ? 8.0 : 4.0) + 4.0 * (double)V * C * (conf ? 2.0 : 1.0));
    hipLaunchKernelGGL(soft_ce_loss_kernel, dim3(G), dim3(ML_THREADS), 0, s, V, clips, C, logits, targets, label_smoothing,
                       grad_scale, conf, dlogits, err, part);
  }
  int rc = check_launch("soft_ce_loss");
  if (rc != AVID_OK) return rc;
  ScopedTimer t(s, "mlabel_final_kernel", 0.0, 32.0 * G);
  hipLaunchKernelGGL(mlabel_final_kernel, dim3(1), dim3(64), 0, s, G, part, rows, loss, (long long*)hits);
  return check_launch("soft_ce_loss (final)");
}
