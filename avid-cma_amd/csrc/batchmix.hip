// Batch-level input mixing on the GPU: mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) of a channel-first batch
// x [B][Cin][T][H][W] with a partner permutation, and the mixed targets, in ONE launch.  The reference has no such code; the
// contract is torch's float32 expression, bit for bit:
//   mixup    y[b] = lam[b] * x[b] + (1 - lam[b]) * x[perm[b]]      four operations, each rounded on its own (no fma)
//   cutmix   y[b][.., h, w] = x[perm[b]][.., h, w] inside box[b] = (h0, h1, w0, w1), x[b][.., h, w] outside: a copy
//   targets  t_out[b] = lam[b] * t[b] + (1 - lam[b]) * t[perm[b]]  (t: t_in, or the one-hot of labels_in), the same rule
//
//   batch_mix_kernel   a work item is 2048 consecutive floats of one sample's 16-byte-aligned body (the sample is split into
//                      a head of 0..3 floats up to the first 16-byte boundary of its OUTPUT row, the body, and a tail of
//                      0..3 floats; item 0 of a sample also does its head and tail, one float per thread).  A thread stores
//                      one 16-byte vector per round; a source whose address is 16-byte aligned at the same element (x[b]
//                      is when x and y are congruent modulo 16, as two tensors of the allocator are; x[perm[b]] is when
//                      (b - perm[b]) * n is a multiple of 4) is read as one 16-byte vector, any other as four dwords, which
//                      a wave still reads as 1 KB of consecutive bytes.  CutMix: a vector whose four elements lie on one side
//                      of the box takes one 16-byte read of that source, one that straddles an edge four dword reads.
//                      The items behind the last data item are the rows of the targets, one workgroup per sample.
// Memory-bound: mixup reads 8 and writes 4 bytes per element, CutMix reads 4 and writes 4.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace avid {

constexpr int MIX_THREADS = 256;
constexpr int MIX_ROUNDS = 2;   // 16-byte vectors per thread and work item: an item is 256 * 2 * 4 floats

// Four operations, each rounded to nearest on its own.  Plain operators under this file's `fp contract(off)`: the header's
// __fmul_rn / __fadd_rn are inline `x * y` / `x + y` parsed under the default contraction mode, and once inlined the
// compiler fuses them into an fma (seen: lam = 0.314159 differed from torch in the last bit).
__device__ __forceinline__ float mix4(float l, float a, float b) {
  const float pa = l * a;
  const float k = 1.f - l;
  const float pb = k * b;
  return pa + pb;
}

__device__ __forceinline__ float4 load4(const float* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__global__ __launch_bounds__(MIX_THREADS) void batch_mix_kernel(int mode, long long B, long long n, int H, int W,
                                                                long long items_per_sample, long long data_items,
                                                                const float* __restrict__ x, const long long* __restrict__ perm,
                                                                const float* __restrict__ lam, const int* __restrict__ box,
                                                                float* __restrict__ y, long long n_classes,
                                                                const float* __restrict__ t_in,
                                                                const long long* __restrict__ labels_in,
                                                                float* __restrict__ t_out, int* __restrict__ err) {
  const int tid = threadIdx.x;
  const long long total = data_items + (t_out ? B : 0);
  for (long long item = blockIdx.x; item < total; item += gridDim.x) {
    const bool data = item < data_items;
    const long long b = data ? item / items_per_sample : item - data_items;
    long long p = perm ? perm[b] : b;
    const bool stray = p < 0 || p >= B;
    if (stray) {
      p = b;   // nothing out of bounds is read: the sample is copied unmixed
      if (err && tid == 0) atomicOr(err, AVID_DEVERR_MIX_INDEX);
    }
    const float l = (lam && !stray) ? lam[b] : 1.f;
    if (!data) {
      // ---- the targets' row of sample b
      long long lb = 0, lp = 0;
      if (labels_in) {
        lb = labels_in[b];
        lp = labels_in[p];
        if ((lb < 0 || lb >= n_classes) && err && tid == 0) atomicOr(err, AVID_DEVERR_CLS_LABEL);
      }
      for (long long c = tid; c < n_classes; c += MIX_THREADS) {
        const float tb = t_in ? t_in[b * n_classes + c] : (lb == c ? 1.f : 0.f);
        const float tp = t_in ? t_in[p * n_classes + c] : (lp == c ? 1.f : 0.f);
        t_out[b * n_classes + c] = stray ? tb : mix4(l, tb, tp);
      }
      continue;
    }
    const long long ch = item - b * items_per_sample;
    const float* xb = x + b * n;
    const float* xp = x + p * n;
    float* yb = y + b * n;
    const bool copy = stray || (mode == AVID_MIX_CUTMIX && p == b);
    int h0 = 0, h1 = 0, w0 = 0, w1 = 0;
    if (mode == AVID_MIX_CUTMIX && !copy) {
      h0 = box[b * 4 + 0];
      h1 = box[b * 4 + 1];
      w0 = box[b * 4 + 2];
      w1 = box[b * 4 + 3];
    }
    const bool cut = mode == AVID_MIX_CUTMIX && !copy && h0 < h1 && w0 < w1;
    // head: the floats in front of the first 16-byte boundary of the output row (n < 4: everything is head)
    long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(yb) & 15)) & 15) >> 2;
    if (head > n) head = n;
    const long long nvec = (n - head) >> 2;
    const long long tail0 = head + (nvec << 2);
    if (ch == 0 && tid < 8) {
      // head (threads 0..3) and tail (threads 4..7), one float each
      const long long i = tid < 4 ? tid : tail0 + (tid - 4);
      if (tid < 4 ? i < head : i < n) {
        float v;
        if (copy) {
          v = xb[i];
        } else if (mode == AVID_MIX_MIXUP) {
          v = mix4(l, xb[i], xp[i]);
        } else {
          const int w = (int)(i % W), h = (int)((i / W) % H);
          v = (cut && h >= h0 && h < h1 && w >= w0 && w < w1) ? xp[i] : xb[i];
        }
        yb[i] = v;
      }
    }
    const bool ab = ((reinterpret_cast<uintptr_t>(xb + head)) & 15) == 0;
    const bool ap = ((reinterpret_cast<uintptr_t>(xp + head)) & 15) == 0;
#pragma unroll
    for (int r = 0; r < MIX_ROUNDS; ++r) {
      const long long vi = ch * (MIX_THREADS * MIX_ROUNDS) + r * MIX_THREADS + tid;
      if (vi >= nvec) break;
      const long long i = head + (vi << 2);
      float4 o;
      if (copy) {
        o = load4(xb + i, ab);
      } else if (mode == AVID_MIX_MIXUP) {
        const float4 a = load4(xb + i, ab), c = load4(xp + i, ap);
        o = make_float4(mix4(l, a.x, c.x), mix4(l, a.y, c.y), mix4(l, a.z, c.z), mix4(l, a.w, c.w));
      } else {
        // the side of the box of each of the four elements (n < 2^31: 32-bit divisions)
        const unsigned iu = (unsigned)i;
        unsigned q = iu / (unsigned)W;
        int w = (int)(iu - q * (unsigned)W), h = (int)(q % (unsigned)H);
        bool in[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          in[e] = cut && h >= h0 && h < h1 && w >= w0 && w < w1;
          if (++w == W) {
            w = 0;
            if (++h == H) h = 0;
          }
        }
        if (in[0] == in[1] && in[1] == in[2] && in[2] == in[3]) {
          o = in[0] ? load4(xp + i, ap) : load4(xb + i, ab);
        } else {
          o.x = in[0] ? xp[i] : xb[i];
          o.y = in[1] ? xp[i + 1] : xb[i + 1];
          o.z = in[2] ? xp[i + 2] : xb[i + 2];
          o.w = in[3] ? xp[i + 3] : xb[i + 3];
        }
      }
      *reinterpret_cast<float4*>(yb + i) = o;
    }
  }
}

}  // namespace avid

using namespace avid;

extern "C" int avid_batch_mix(int mode, int64_t B, int64_t Cin, int64_t T, int64_t H, int64_t W, const float* x,
                              const int64_t* perm, const float* lam, const int32_t* box, float* y, int64_t n_classes,
                              const float* t_in, const int64_t* labels_in, float* t_out, int32_t* err, avid_stream_t stream) {
  AVID_REQUIRE(mode == AVID_MIX_MIXUP || mode == AVID_MIX_CUTMIX, AVID_E_BADARG, "batch_mix: mode %d is neither mixup nor cutmix", mode);
  AVID_REQUIRE(B > 0 && (x != nullptr) == (y != nullptr) && (x || t_out), AVID_E_BADARG,
               "batch_mix: bad arguments (B %lld; x and y go together; without them t_out is needed)", (long long)B);
  long long n = 0;
  if (x) {
    AVID_REQUIRE(Cin > 0 && T > 0 && H > 0 && W > 0, AVID_E_BADARG, "batch_mix: bad geometry [%lld][%lld][%lld][%lld][%lld]",
                 (long long)B, (long long)Cin, (long long)T, (long long)H, (long long)W);
    const double nd = (double)Cin * (double)T * (double)H * (double)W;
    AVID_REQUIRE(nd < 2147483648.0 && nd * (double)B < 9.0e18, AVID_E_UNSUPPORTED,
                 "batch_mix: a sample of %g floats is beyond the kernel's 32-bit index range", nd);
    n = (long long)Cin * T * H * W;
    AVID_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0, AVID_E_BADARG,
                 "batch_mix: x and y must be 4-byte aligned");
    const float* xe = x + (size_t)B * n;
    const float* ye = y + (size_t)B * n;
    AVID_REQUIRE(ye <= x || xe <= y, AVID_E_BADARG, "batch_mix: y must not overlap x");
    AVID_REQUIRE(mode != AVID_MIX_CUTMIX || box, AVID_E_BADARG, "batch_mix: cutmix needs the boxes");
  }
  if (t_out) {
    AVID_REQUIRE(n_classes > 0 && (t_in != nullptr) != (labels_in != nullptr), AVID_E_BADARG,
                 "batch_mix: targets need n_classes >= 1 and exactly one of t_in and labels_in");
    AVID_REQUIRE(t_out != t_in, AVID_E_BADARG, "batch_mix: t_out must not be t_in");
  }
  const long long ips = x ? ceil_div(n >> 2 > 0 ? n >> 2 : 1, MIX_THREADS * MIX_ROUNDS) : 0;
  const long long data_items = (long long)B * ips;
  const long long total = data_items + (t_out ? B : 0);
  long long g = (long long)device_cus() * 16;
  if (g > total) g = total;
  hipStream_t s = (hipStream_t)stream;
  const double bytes = 4.0 * (double)B * (double)n * (mode == AVID_MIX_MIXUP ? 3.0 : 2.0) +
                       (t_out ? 4.0 * (double)B * (double)n_classes * (t_in ? 3.0 : 1.0) : 0.0);
  ScopedTimer t(s, "batch_mix_kernel", mode == AVID_MIX_MIXUP ? 3.0 * (double)B * (double)n : 0.0, bytes);
  hipLaunchKernelGGL(batch_mix_kernel, dim3((unsigned)g), dim3(MIX_THREADS), 0, s, mode, (long long)B, n, (int)H, (int)W, ips,
                     data_items, x, (const long long*)perm, lam, box, y, (long long)n_classes, t_in,
                     (const long long*)labels_in, t_out, err);
  return check_launch("batch_mix");
}
