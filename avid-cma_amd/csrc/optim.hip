// Flat fused Adam (torch.optim.Adam semantics: L2 weight decay folded into the gradient, bias
// correction as in torch's single-tensor path) over ONE contiguous fp32 buffer holding every
// parameter — replaces the 141 per-tensor optimizer launches of utils/main_utils.py:250-261.
// Flat SGD with momentum (torch.optim.SGD semantics, utils/main_utils.py:242-248) over the same buffers: one state buffer.
// Flat gradient accumulation (dst = a + b) over the same buffers: what sums the shards of a virtual-rank step.
#include <math.h>

#include "common.h"

namespace avid {

__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long long n4,
                                                        long long n, float b1, float b2, float eps, float wd,
                                                        float step_size, double inv_bc1, float inv_sqrt_bc2,
                                                        float grad_scale, float lr, const long long* __restrict__ step_dev,
                                                        const float* __restrict__ lr_dev) {
  if (lr_dev) {   // graph-replay safe learning rate (scheduler writes the device word); the host's lr is not used
    lr = *lr_dev;
    step_size = (float)((double)lr * inv_bc1);   // (recomputed below when step_dev is given)
  }
  if (step_dev) {  // graph-replay safe: bias corrections from the device-resident step counter
    const double t = (double)*step_dev;
    step_size = (float)((double)lr / (1.0 - pow((double)b1, t)));
    inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, t)));
  }
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    floatx4 pv = reinterpret_cast<floatx4*>(p)[i];
    floatx4 gv = reinterpret_cast<const floatx4*>(g)[i];
    floatx4 mv = reinterpret_cast<floatx4*>(m)[i];
    floatx4 vv = reinterpret_cast<floatx4*>(v)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = gv[j] * grad_scale + wd * pv[j];
      mv[j] = b1 * mv[j] + (1.f - b1) * gg;
      vv[j] = b2 * vv[j] + (1.f - b2) * gg * gg;
      const float denom = sqrtf(vv[j]) * inv_sqrt_bc2 + eps;
      pv[j] -= step_size * (mv[j] / denom);
    }
    reinterpret_cast<floatx4*>(p)[i] = pv;
    reinterpret_cast<floatx4*>(m)[i] = mv;
    reinterpret_cast<floatx4*>(v)[i] = vv;
  }
  // tail (n % 4) handled by block 0
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    const float gg = g[i] * grad_scale + wd * p[i];
    m[i] = b1 * m[i] + (1.f - b1) * gg;
    v[i] = b2 * v[i] + (1.f - b2) * gg * gg;
    p[i] -= step_size * (m[i] / (sqrtf(v[i]) * inv_sqrt_bc2 + eps));
  }
}

// torch's single-tensor SGD (dampening 0) for one element, in torch's order, every product and every sum rounded to fp32 on
// its own: hipcc contracts a * b + c into one fused multiply-add by default, torch's kernels (and the numpy restatement the
// tests hold this against, bit for bit) do not.  A zero-initialised buffer makes the first step torch's ``buf = clone(d)``.
__device__ __forceinline__ float sgd_element(float& p, float g, float* buf, float lr, float momentum, float wd, bool nesterov,
                                             float grad_scale) {
#pragma clang fp contract(off)
  float d = g * grad_scale;
  if (wd != 0.f) {
    const float t = wd * p;
    d = d + t;
  }
  float b = 0.f;
  if (buf) {
    const float t = momentum * *buf;
    b = t + d;
    if (nesterov) {
      const float u = momentum * b;
      d = d + u;
    } else {
      d = b;
    }
  }
  const float s = lr * d;
  p = p - s;
  return b;
}

__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ buf, long long n4, long long n, float lr,
                                                       float momentum, float wd, int nesterov, float grad_scale,
                                                       const float* __restrict__ lr_dev) {
  if (lr_dev) lr = *lr_dev;   // graph-replay safe learning rate, as adam_flat_kernel's
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    floatx4 pv = reinterpret_cast<floatx4*>(p)[i];
    floatx4 gv = reinterpret_cast<const floatx4*>(g)[i];
    floatx4 bv = {0.f, 0.f, 0.f, 0.f};
    if (buf) bv = reinterpret_cast<floatx4*>(buf)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], bj = bv[j];
      bj = sgd_element(pj, gv[j], buf ? &bj : nullptr, lr, momentum, wd, nesterov != 0, grad_scale);
      pv[j] = pj;
      bv[j] = bj;
    }
    reinterpret_cast<floatx4*>(p)[i] = pv;
    if (buf) reinterpret_cast<floatx4*>(buf)[i] = bv;
  }
  // tail (n % 4) handled by block 0
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    float pi = p[i], bi = buf ? buf[i] : 0.f;
    bi = sgd_element(pi, g[i], buf ? &bi : nullptr, lr, momentum, wd, nesterov != 0, grad_scale);
    p[i] = pi;
    if (buf) buf[i] = bi;
  }
}

// dst[i] = a[i] + b[i]: one fp32 rounding per element, every element written by exactly one thread from the two values at
// its own index — the result does not depend on the launch geometry, and dst may BE a or b (no __restrict__: an element is
// read before it is written, by the thread that writes it).  vec: the three pointers are 16-byte aligned (n4 = n / 4
// vectors, then the tail); otherwise n4 = 0 and the scalar loop takes all n elements.
__global__ __launch_bounds__(256) void grad_accum_flat_kernel(float* dst, const float* a, const float* b, long long n4,
                                                              long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = tid; i < n4; i += stride) {
    const floatx4 av = reinterpret_cast<const floatx4*>(a)[i];
    const floatx4 bv = reinterpret_cast<const floatx4*>(b)[i];
    reinterpret_cast<floatx4*>(dst)[i] = av + bv;
  }
  // scalar elements: the tail (n % 4) behind the vectors, or everything when the buffers are not 16-byte aligned
  for (long long i = n4 * 4 + tid; i < n; i += stride) dst[i] = a[i] + b[i];
}

}  // namespace avid

using namespace avid;

extern "C" int avid_adam_flat(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                              const float* lr_dev, float grad_scale, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && p && g && m && v && (step >= 1 || step_dev), AVID_E_BADARG, "adam_flat: bad argument");
  if (step < 1) step = 1;
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, AVID_E_BADARG,
               "adam_flat: buffers must be 16-byte aligned");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const double inv_bc1 = 1.0 / bc1;
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const long long n4 = n / 4;
  long long grid = ceil_div(n4 > 0 ? n4 : 1, 256);
  if (grid > 4096) grid = 4096;
  ScopedTimer t((hipStream_t)stream, "adam_flat_kernel", 0.0, 28.0 * n);
  hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4,
                     (long long)n, beta1, beta2, eps, weight_decay, step_size, inv_bc1, inv_sqrt_bc2, grad_scale, lr,
                     (const long long*)step_dev, lr_dev);
  return check_launch("adam_flat");
}

extern "C" int avid_sgd_flat(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                             int nesterov, const float* lr_dev, float grad_scale, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && p && g, AVID_E_BADARG, "sgd_flat: bad argument");
  AVID_REQUIRE(buf || momentum == 0.f, AVID_E_BADARG, "sgd_flat: momentum needs its buffer");
  if (momentum == 0.f) buf = nullptr;   // (the kernel takes the buffer as the switch)
  AVID_REQUIRE(!nesterov || momentum != 0.f, AVID_E_BADARG, "sgd_flat: nesterov needs momentum");
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0, AVID_E_BADARG,
               "sgd_flat: buffers must be 16-byte aligned");
  const long long n4 = n / 4;
  long long grid = ceil_div(n4 > 0 ? n4 : 1, 256);
  if (grid > 4096) grid = 4096;
  ScopedTimer t((hipStream_t)stream, "sgd_flat_kernel", 0.0, (buf ? 20.0 : 12.0) * n);
  hipLaunchKernelGGL(sgd_flat_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, buf, n4, (long long)n,
                     lr, momentum, weight_decay, nesterov, grad_scale, lr_dev);
  return check_launch("sgd_flat");
}

extern "C" int avid_grad_accum_flat(int64_t n, float* dst, const float* a, const float* b, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && dst && a && b, AVID_E_BADARG, "grad_accum_flat: bad argument");
  // dst is exactly a, exactly b, or disjoint from both: a partly overlapping dst would be read after it was written
  const uintptr_t d0 = (uintptr_t)dst, bytes = (uintptr_t)n * 4;
  const uintptr_t src[2] = {(uintptr_t)a, (uintptr_t)b};
  for (int k = 0; k < 2; ++k)
    AVID_REQUIRE(src[k] == d0 || src[k] + bytes <= d0 || d0 + bytes <= src[k], AVID_E_BADARG,
                 "grad_accum_flat: dst overlaps an input without being that input");
  const bool vec = ((d0 | src[0] | src[1]) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  const long long work = vec ? (n4 > 0 ? n4 : 1) : (long long)n;
  long long grid = ceil_div(work, 256);
  if (grid > 4096) grid = 4096;
  ScopedTimer t((hipStream_t)stream, "grad_accum_flat_kernel", 0.0, 12.0 * n);
  hipLaunchKernelGGL(grad_accum_flat_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, dst, a, b, n4,
                     (long long)n);
  return check_launch("grad_accum_flat");
}
