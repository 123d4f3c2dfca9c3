// Flat fused Adam (torch.optim.Adam semantics: L2 weight decay folded into the gradient, bias
// correction as in torch's single-tensor path) over ONE contiguous fp32 buffer holding every
// parameter — replaces the 141 per-tensor optimizer launches of utils/main_utils.py:250-261.
// Flat SGD with momentum (torch.optim.SGD semantics, utils/main_utils.py:242-248) over the same buffers: one state buffer.
// Flat gradient accumulation (dst = a + b) over the same buffers: what sums the shards of a virtual-rank step.
// The step guard (avid_grad_guard): one deterministic pass over the flat gradient -> norm, clip coefficient, skip word in a
// device record; guarded forms of the two optimizers and of the counter that obey it, and the row restore of a skipped step.
#include <math.h>

#include "common.h"

namespace avid {

// ---- the flat optimizers ----------------------------------------------------------------------------------------------------
// Eight kernels — {Adam, SGD} x {plain, under a guard record} x {alone, with the weight average} — are the instantiations of
// adam_flat_body / sgd_flat_body<GUARD, EMA>: a kernel holds no code of a form it is not.  Every rounding is spelled out: the
// element functions are compiled with contraction off and say __builtin_fmaf where a product and a sum round once.  Which pairs
// Adam fuses — and that its vector loop, its n % 4 tail and its clipped forms do not fuse the same ones — is how the compiler once
// contracted the first kernels, an accident, kept because a step has to keep its bits.  The specification is this source and
// the recorded bits of tests/golden/optim_flat_bits.npz (tests/test_gpu_optim_bits.py), not a code object.

// The weight average: e = e + w * (p - e), the difference, the product and the sum each rounded to fp32 on its own (torch's
// unfused `e + (p - e) * w`; the numpy restatement of tests/_ema_ref.py, bit for bit).
__device__ __forceinline__ float ema_element(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float t = w * d;
  return e + t;
}

// w = (float)(1 - d), formed once per launch in double: d is the decay, or — warm-up — min(decay, (1 + k) / (10 + k)) with k
// the averaging updates applied so far, read from the device counter (a captured graph freezes by-value arguments).
__device__ __forceinline__ float ema_weight(double decay, int warmup, const long long* __restrict__ updates_dev) {
  double d = decay;
  if (warmup) {
    const double k = (double)*updates_dev;
    const double r = (1.0 + k) / (10.0 + k);
    if (r < d) d = r;
  }
  return (float)(1.0 - d);
}

// d of the SGD family up to the weight-decay term, (g * grad_scale) * coef + wd * p: what LARS takes the norm of, and what
// the update goes on from — the same operations in both places.
__device__ __forceinline__ float sgd_d(float g, float p, float grad_scale, float coef, float wd) {
#pragma clang fp contract(off)
  float d = g * grad_scale;
  d = d * coef;
  if (wd != 0.f) {
    const float t = wd * p;
    d = d + t;
  }
  return d;
}

// torch's single-tensor SGD (dampening 0) for one element on q * d, in torch's order, every product and every sum rounded to fp32
// on its own: torch's kernels (and the numpy restatement the tests hold this against, bit for bit) do not fuse.  coef is the
// guard's clip coefficient, q the trust factor of a segment: the unguarded kernels pass coef = 1.0f, the flat ones q = 1.0f, and
// times 1.0f is exact.  A zero-initialised buffer makes the first step torch's ``buf = clone(d)``.  The momentum value travels
// by reference, not behind a nullable pointer, so that nothing of it lives in a private segment.
__device__ __forceinline__ void sgd_element(float& p, float g, float& b, bool has_buf, float lr, float momentum, float wd,
                                            bool nesterov, float grad_scale, float coef, float q) {
#pragma clang fp contract(off)
  float d = sgd_d(g, p, grad_scale, coef, wd);
  d = q * d;
  if (has_buf) {
    const float t = momentum * b;
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
}

// The gradient term gg of the Adam family (L2 weight decay folded into the gradient); t = (g * grad_scale) * coef, the two
// products rounded one after the other:
//   GRAD_UNCLIPPED    fma(g, grad_scale, wd * p)    every step whose clip coefficient is 1.0f (which is not applied)
//   GRAD_CLIPPED_FMA  fma(wd, p, t)                 the flat kernels' vector loop
//   GRAD_CLIPPED_SUM  wd * p + t, unfused           the flat kernels' n % 4 tail; adam_flat_table_kernel throughout
enum { GRAD_UNCLIPPED, GRAD_CLIPPED_FMA, GRAD_CLIPPED_SUM };

template <int FORM>
__device__ __forceinline__ float adam_grad_term(float g, float p, float grad_scale, float wd, float coef) {
#pragma clang fp contract(off)
  if (FORM == GRAD_UNCLIPPED) {
    const float u = wd * p;
    return __builtin_fmaf(g, grad_scale, u);
  }
  float t = g * grad_scale;
  t = t * coef;
  if (FORM == GRAD_CLIPPED_FMA) return __builtin_fmaf(wd, p, t);
  const float u = wd * p;
  return u + t;
}

// Adam's moments.  Vector loop: m = fma(b1, m, (1 - b1) * gg), v = fma(b2, v, ((1 - b2) * gg) * gg); n % 4 tail: m = fma(1 - b1,
// gg, b1 * m), v = b2 * v + ((1 - b2) * gg) * gg, unfused.  (The segment kernels use the vector-loop form for their tails too.)
template <bool TAIL>
__device__ __forceinline__ void adam_moments(float gg, float& m, float& v, float b1, float b2) {
#pragma clang fp contract(off)
  const float c1 = 1.f - b1, c2 = 1.f - b2;
  const float s = c2 * gg;
  const float d = s * gg;
  if (TAIL) {
    const float t = b1 * m;
    m = __builtin_fmaf(c1, gg, t);
    const float u = b2 * v;
    v = u + d;
  } else {
    const float a = c1 * gg;
    m = __builtin_fmaf(b1, m, a);
    v = __builtin_fmaf(b2, v, d);
  }
}

// One element of Adam behind its gradient term: the moments, denom = fma(sqrt(v), inv_sqrt_bc2, eps), p = fma(-step_size,
// m / denom, p) (torch's single-tensor path: bias correction 1 in the step size, 2 in the denominator).
template <bool TAIL>
__device__ __forceinline__ void adam_element(float& p, float gg, float& m, float& v, float b1, float b2, float eps,
                                             float step_size, float inv_sqrt_bc2) {
#pragma clang fp contract(off)
  adam_moments<TAIL>(gg, m, v, b1, b2);
  const float denom = __builtin_fmaf(sqrtf(v), inv_sqrt_bc2, eps);
  const float q = m / denom;
  p = __builtin_fmaf(-step_size, q, p);
}

// Adam's bias corrections from the device-resident step counter (graph-replay safe): bc1 = 1 - beta1^t, (float)(1 / sqrt(1 - beta2^t)).
__device__ __forceinline__ void adam_bias_dev(float b1, float b2, const long long* __restrict__ step_dev, double& bc1,
                                              float& inv_sqrt_bc2) {
  const double t = (double)*step_dev;
  bc1 = 1.0 - pow((double)b1, t);
  inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, t)));
}

// The block size of the eight kernels, a constant in the walks: read from the dispatch (blockDim.x) inside a device function
// it costs every wave a vector load and a wait in front of its loop.
constexpr int FLAT_THREADS = 256;

// What a flat kernel takes: its optimizer's arguments, then — only in the forms that have them — the average's and the guard
// record, so that a kernel's argument block holds nothing of a form it is not (the plain kernels' is the one they always had).
struct AdamFlatArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n4, n;               // 16-byte vectors, elements
  float b1, b2, eps, wd, step_size;   // step_size, inv_bc1, inv_sqrt_bc2: from the host's step
  double inv_bc1;
  float inv_sqrt_bc2, grad_scale, lr;
  const long long* step_dev;     // nullable
  const float* lr_dev;           // nullable: the learning rate a scheduler writes (a captured graph freezes lr)
};

struct SgdFlatArgs {
  float* p;
  const float* g;
  float* buf;                    // the momentum buffer, nullptr exactly when momentum == 0 (the kernels' switch)
  long long n4, n;
  float lr, momentum, wd;
  int nesterov;
  float grad_scale;
  const float* lr_dev;
};

struct EmaFlatArgs {
  float* e;
  double decay;
  int warmup;
  const long long* updates_dev;
};

// The step size and 1 / sqrt(bias correction 2) of a launch.  By value: the host's.  lr_dev alone: lr times the host's 1 / bc1
// (the host's lr is not used).  step_dev: lr / bc1 with both corrections from the device counter.
__device__ __forceinline__ void adam_step_terms(const AdamFlatArgs& a, float& step_size, float& inv_sqrt_bc2) {
  float lr = a.lr;
  step_size = a.step_size;
  inv_sqrt_bc2 = a.inv_sqrt_bc2;
  if (a.lr_dev) {
    lr = *a.lr_dev;
    step_size = (float)((double)lr * a.inv_bc1);
  }
  if (a.step_dev) {
    double bc1;
    adam_bias_dev(a.b1, a.b2, a.step_dev, bc1, inv_sqrt_bc2);
    step_size = (float)((double)lr / bc1);
  }
}

// The walk of a flat kernel: grid-stride over the 16-byte vectors, the n % 4 tail by block 0.  With the average, e[i] comes
// from the p[i] just computed — one more 4-byte read and write per element instead of a pass of its own that reads p again.
template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_flat_walk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, float* __restrict__ e, const AdamFlatArgs& a, float step_size,
                                               float inv_sqrt_bc2, float coef, float w) {
  const long long n4 = a.n4, stride = (long long)gridDim.x * FLAT_THREADS;
  for (long long i = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n4; i += stride) {
    floatx4 pv = reinterpret_cast<floatx4*>(p)[i];
    floatx4 gv = reinterpret_cast<const floatx4*>(g)[i];
    floatx4 mv = reinterpret_cast<floatx4*>(m)[i];
    floatx4 vv = reinterpret_cast<floatx4*>(v)[i];
    floatx4 ev = {0.f, 0.f, 0.f, 0.f};
    if (EMA) ev = reinterpret_cast<floatx4*>(e)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], mj = mv[j], vj = vv[j];
      const float gg = adam_grad_term<CLIP ? GRAD_CLIPPED_FMA : GRAD_UNCLIPPED>(gv[j], pj, a.grad_scale, a.wd, coef);
      adam_element<false>(pj, gg, mj, vj, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
      pv[j] = pj;
      mv[j] = mj;
      vv[j] = vj;
      if (EMA) ev[j] = ema_element(ev[j], pj, w);
    }
    reinterpret_cast<floatx4*>(p)[i] = pv;
    reinterpret_cast<floatx4*>(m)[i] = mv;
    reinterpret_cast<floatx4*>(v)[i] = vv;
    if (EMA) reinterpret_cast<floatx4*>(e)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(a.n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    float pi = p[i], mi = m[i], vi = v[i];
    const float gg = adam_grad_term<CLIP ? GRAD_CLIPPED_SUM : GRAD_UNCLIPPED>(g[i], pi, a.grad_scale, a.wd, coef);
    adam_element<true>(pi, gg, mi, vi, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (EMA) e[i] = ema_element(e[i], pi, w);
  }
}

// GUARD: nothing is written when guard->skip, e included; the gradient is scaled by guard->clip_coef on the way in, and a
// coefficient of 1.0f takes the unclipped form, so that an unclipped step has the unguarded kernel's bits.
template <bool GUARD, bool EMA>
__device__ __forceinline__ void adam_flat_body(const AdamFlatArgs& a, const EmaFlatArgs& avg, const avid_step_guard* guard) {
  if (GUARD && guard->skip) return;
  const float coef = GUARD ? guard->clip_coef : 1.f;
  float step_size, inv_sqrt_bc2;
  adam_step_terms(a, step_size, inv_sqrt_bc2);
  const float w = EMA ? ema_weight(avg.decay, avg.warmup, avg.updates_dev) : 0.f;
  if (coef == 1.f)
    adam_flat_walk<false, EMA>(a.p, a.g, a.m, a.v, avg.e, a, step_size, inv_sqrt_bc2, coef, w);
  else
    adam_flat_walk<true, EMA>(a.p, a.g, a.m, a.v, avg.e, a, step_size, inv_sqrt_bc2, coef, w);
}

template <bool EMA>
__device__ __forceinline__ void sgd_flat_walk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                              float* __restrict__ e, const SgdFlatArgs& a, float lr, float coef, float w) {
  const bool has_buf = buf != nullptr, nesterov = a.nesterov != 0;
  const long long n4 = a.n4, stride = (long long)gridDim.x * FLAT_THREADS;
  for (long long i = (long long)blockIdx.x * FLAT_THREADS + threadIdx.x; i < n4; i += stride) {
    floatx4 pv = reinterpret_cast<floatx4*>(p)[i];
    floatx4 gv = reinterpret_cast<const floatx4*>(g)[i];
    floatx4 bv = {0.f, 0.f, 0.f, 0.f}, ev = {0.f, 0.f, 0.f, 0.f};
    if (EMA) ev = reinterpret_cast<floatx4*>(e)[i];
    if (has_buf) bv = reinterpret_cast<floatx4*>(buf)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], bj = bv[j];
      sgd_element(pj, gv[j], bj, has_buf, lr, a.momentum, a.wd, nesterov, a.grad_scale, coef, 1.f);
      pv[j] = pj;
      bv[j] = bj;
      if (EMA) ev[j] = ema_element(ev[j], pj, w);
    }
    reinterpret_cast<floatx4*>(p)[i] = pv;
    if (has_buf) reinterpret_cast<floatx4*>(buf)[i] = bv;
    if (EMA) reinterpret_cast<floatx4*>(e)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(a.n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    float pi = p[i], bi = has_buf ? buf[i] : 0.f;
    sgd_element(pi, g[i], bi, has_buf, lr, a.momentum, a.wd, nesterov, a.grad_scale, coef, 1.f);
    p[i] = pi;
    if (has_buf) buf[i] = bi;
    if (EMA) e[i] = ema_element(e[i], pi, w);
  }
}

template <bool GUARD, bool EMA>
__device__ __forceinline__ void sgd_flat_body(const SgdFlatArgs& a, const EmaFlatArgs& avg, const avid_step_guard* guard) {
  if (GUARD && guard->skip) return;
  const float coef = GUARD ? guard->clip_coef : 1.f;
  const float lr = a.lr_dev ? *a.lr_dev : a.lr;
  const float w = EMA ? ema_weight(avg.decay, avg.warmup, avg.updates_dev) : 0.f;
  sgd_flat_walk<EMA>(a.p, a.g, a.buf, avg.e, a, lr, coef, w);
}

__global__ __launch_bounds__(FLAT_THREADS) void adam_flat_kernel(AdamFlatArgs a) {
  adam_flat_body<false, false>(a, EmaFlatArgs{}, nullptr);
}
__global__ __launch_bounds__(FLAT_THREADS) void adam_flat_guarded_kernel(AdamFlatArgs a, const avid_step_guard* guard) {
  adam_flat_body<true, false>(a, EmaFlatArgs{}, guard);
}
__global__ __launch_bounds__(FLAT_THREADS) void adam_flat_ema_kernel(AdamFlatArgs a, EmaFlatArgs avg) {
  adam_flat_body<false, true>(a, avg, nullptr);
}
__global__ __launch_bounds__(FLAT_THREADS) void adam_flat_ema_guarded_kernel(AdamFlatArgs a, EmaFlatArgs avg,
                                                                             const avid_step_guard* guard) {
  adam_flat_body<true, true>(a, avg, guard);
}
__global__ __launch_bounds__(FLAT_THREADS) void sgd_flat_kernel(SgdFlatArgs a) {
  sgd_flat_body<false, false>(a, EmaFlatArgs{}, nullptr);
}
__global__ __launch_bounds__(FLAT_THREADS) void sgd_flat_guarded_kernel(SgdFlatArgs a, const avid_step_guard* guard) {
  sgd_flat_body<true, false>(a, EmaFlatArgs{}, guard);
}
__global__ __launch_bounds__(FLAT_THREADS) void sgd_flat_ema_kernel(SgdFlatArgs a, EmaFlatArgs avg) {
  sgd_flat_body<false, true>(a, avg, nullptr);
}
__global__ __launch_bounds__(FLAT_THREADS) void sgd_flat_ema_guarded_kernel(SgdFlatArgs a, EmaFlatArgs avg,
                                                                            const avid_step_guard* guard) {
  sgd_flat_body<true, true>(a, avg, guard);
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

// ---- the step guard ---------------------------------------------------------------------------------------------------
// Sum of squares of g[0, n) in a FIXED order, whatever the scheduling: grid-stride 16-byte vectors into four double
// accumulators per thread (the product of two floats is exact in double), the up to three scalar elements in front of the
// first 16-byte boundary and the up to three behind the last vector added by threads of block 0, (a0 + a1) + (a2 + a3), the
// xor butterfly over the wave, the four waves left to right: one double per block.  No atomics.
constexpr int GUARD_THREADS = 256;
constexpr int GUARD_MAX_BLOCKS = 1024;

__device__ __forceinline__ double guard_block_sum(double s, double* lds) {
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(GUARD_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, long long n, int head,
                                                                   long long n4, double* __restrict__ partials) {
  __shared__ double lds[GUARD_THREADS / 64];
  const floatx4* body = reinterpret_cast<const floatx4*>(g + head);
  const long long stride = (long long)gridDim.x * blockDim.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const floatx4 v = body[i];
    a0 += (double)v[0] * (double)v[0];
    a1 += (double)v[1] * (double)v[1];
    a2 += (double)v[2] * (double)v[2];
    a3 += (double)v[3] * (double)v[3];
  }
  if (blockIdx.x == 0) {   // scalar head (threads 0 .. head-1) and tail (the threads behind them)
    const int tail = (int)(n - head - n4 * 4), t = threadIdx.x;
    if (t < head) {
      a0 += (double)g[t] * (double)g[t];
    } else if (t < head + tail) {
      const float x = g[head + n4 * 4 + (t - head)];
      a0 += (double)x * (double)x;
    }
  }
  const double s = guard_block_sum((a0 + a1) + (a2 + a3), lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One block: thread t sums partials t, t + 256, ... in that order, then the same block sum; thread 0 judges and writes the
// record (plain stores).  The sum is judged as the float it would have been: a double sum above FLT_MAX is an overflow.
__global__ __launch_bounds__(GUARD_THREADS) void grad_guard_finish_kernel(const double* __restrict__ partials, int nparts,
                                                                          float grad_scale, float max_norm, int skip_nonfinite,
                                                                          avid_step_guard* __restrict__ guard) {
  __shared__ double lds[GUARD_THREADS / 64];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += GUARD_THREADS) a += partials[i];
  const double sum = guard_block_sum(a, lds);
  if (threadIdx.x != 0) return;
  const float sum_f = (float)sum;
  const bool finite = sum_f - sum_f == 0.f;
  const float norm = (float)(sqrt(finite ? sum : (double)sum_f) * (double)grad_scale);
  float coef = 1.f;
  if (max_norm > 0.f) {   // torch.nn.utils.clip_grad_norm_: min(1, max_norm / (total_norm + 1e-6)), rounded once
    const double c = (double)max_norm / ((double)norm + (double)1e-6f);
    if (c < 1.0) coef = (float)c;
  }
  const int skip = (skip_nonfinite && !finite) ? 1 : 0;
  guard->grad_norm = norm;
  guard->clip_coef = skip ? 1.f : coef;
  guard->skip = skip;
  guard->reserved = 0;
  guard->skipped_total += skip;
  guard->steps_total += 1;
}

// One block over a SMALL buffer (the 78 KB of BatchNorm running statistics): any element that is not finite turns the record
// into a skip — clip_coef 1.0f, skipped_total advanced unless the gradient's verdict was a skip already.
__global__ __launch_bounds__(256) void guard_nonfinite_kernel(const float* __restrict__ x, long long n,
                                                              avid_step_guard* __restrict__ guard) {
  int bad = 0;
  for (long long i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = x[i];
    bad |= (v - v == 0.f) ? 0 : 1;
  }
  const int any = __syncthreads_or(bad);
  if (threadIdx.x == 0 && any && !guard->skip) {
    guard->skip = 1;
    guard->clip_coef = 1.f;
    guard->skipped_total += 1;
  }
}

__global__ void counter_add_unless_kernel(unsigned long long* ctr, unsigned long long inc, const avid_step_guard* guard) {
  if (!guard->skip) *ctr += inc;
}

// dst[idx[r]][0, D) = saved[r][0, D) for every row when guard->skip (idx == nullptr: row r itself); nothing otherwise.
// Duplicate ids carry identical saved rows: the writes race on equal values.
__global__ __launch_bounds__(256) void guard_restore_kernel(long long rows, long long D, float* __restrict__ dst,
                                                            const long long* __restrict__ idx, const float* __restrict__ saved,
                                                            const avid_step_guard* __restrict__ guard) {
  if (!guard->skip) return;
  const long long total = rows * D, stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long r = i / D, c = i - r * D;
    dst[(idx ? idx[r] : r) * D + c] = saved[i];
  }
}

// ---- the weight average (EMA) ----------------------------------------------------------------------------------------------
// ema_element in a pass of its own: e from a p that somebody else wrote (the BatchNorm running statistics; a caller's
// own optimizer).  guard: nullable; a skip writes nothing.
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ e, const float* __restrict__ p, long long n4,
                                                       long long n, double decay, int warmup,
                                                       const long long* __restrict__ updates_dev,
                                                       const avid_step_guard* __restrict__ guard) {
  if (guard && guard->skip) return;
  const float w = ema_weight(decay, warmup, updates_dev);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    floatx4 ev = reinterpret_cast<floatx4*>(e)[i];
    const floatx4 pv = reinterpret_cast<const floatx4*>(p)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) ev[j] = ema_element(ev[j], pv[j], w);
    reinterpret_cast<floatx4*>(e)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) {
    const long long i = n4 * 4 + threadIdx.x;
    e[i] = ema_element(e[i], p[i], w);
  }
}

// a <-> b: every element read from both buffers and written to both by one thread.  n4 vectors (0 unless both pointers are
// 16-byte aligned), then the scalar elements: the tail, or everything.  The buffers are disjoint (the host checks).
__global__ __launch_bounds__(256) void swap_flat_kernel(float* __restrict__ a, float* __restrict__ b, long long n4,
                                                        long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long i = tid; i < n4; i += stride) {
    const floatx4 av = reinterpret_cast<floatx4*>(a)[i];
    const floatx4 bv = reinterpret_cast<floatx4*>(b)[i];
    reinterpret_cast<floatx4*>(a)[i] = bv;
    reinterpret_cast<floatx4*>(b)[i] = av;
  }
  for (long long i = n4 * 4 + tid; i < n; i += stride) {
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

// ---- segment tables: per-tensor hyper-parameters, per-segment norms, LARS / LAMB ------------------------------------------
// A workgroup takes CHUNKS (AVID_SEG_CHUNK floats of one segment: chunk c, c + gridDim.x, ...), finds its segment in the chunk
// record and walks the chunk's 16-byte vectors (a segment starts on a 16-byte boundary, a chunk is a multiple of it); the up to
// three elements behind a segment's last vector are scalar accesses of threads 0..2, so that nothing outside a segment — the
// padding between tensors — is read into a sum or written.  What an element becomes depends on its own index only.
constexpr int SEG_THREADS = 256;

struct SegArgs {
  const avid_segment* segs;
  const avid_seg_chunk* chunks;
  int n_chunks;
  float* p;            // (the plain sums: x)
  const float* g;      // (the plain sums: y, nullable)
  float* m;
  float* v;
  float* buf;
  float* e;            // the weight average, nullable
  float lr, momentum, b1, b2, eps, grad_scale;
  int nesterov;
  double bc1, inv_bc1;           // 1 - beta1^step and its reciprocal, from the host's step
  float inv_sqrt_bc2;            // (float)(1 / sqrt(1 - beta2^step))
  const long long* step_dev;
  const float* lr_dev;
  const avid_step_guard* guard;
  const float* trust;            // per-segment factor the update applies, nullable (1.0f)
  double decay;
  int warmup;
  const long long* updates_dev;
  double* partials;              // [n_chunks][2]
};

// What a launch reads once: the skip word, the clip coefficient, the learning rate and Adam's bias corrections as
// adam_step_terms forms them (step_case 0: by value, 1: lr_dev alone, 2: step_dev), the averaging weight.
struct SegTerms {
  float coef, lr, inv_sqrt_bc2, c1, w;
  double bc1, inv_bc1;
  int step_case;
};

__device__ __forceinline__ bool seg_terms(const SegArgs& a, bool adam, SegTerms& t) {
  if (a.guard && a.guard->skip) return false;
  t.coef = a.guard ? a.guard->clip_coef : 1.f;
  t.lr = a.lr_dev ? *a.lr_dev : a.lr;
  t.bc1 = a.bc1;
  t.inv_bc1 = a.inv_bc1;
  t.inv_sqrt_bc2 = a.inv_sqrt_bc2;
  t.step_case = a.lr_dev ? 1 : 0;
  if (adam && a.step_dev) {
    adam_bias_dev(a.b1, a.b2, a.step_dev, t.bc1, t.inv_sqrt_bc2);
    t.inv_bc1 = 1.0 / t.bc1;
    t.step_case = 2;
  }
  t.c1 = (float)t.inv_bc1;
  t.w = a.e ? ema_weight(a.decay, a.warmup, a.updates_dev) : 0.f;
  return true;
}

// The learning rate of a segment: one fp32 product (times 1.0f is exact).
__device__ __forceinline__ float seg_lr(float lr, float lr_scale) {
#pragma clang fp contract(off)
  const float s = lr * lr_scale;
  return s;
}

// adam_flat_kernel's step size for a segment's learning rate, in the case the launch is in.
__device__ __forceinline__ float seg_adam_step_size(float lr_s, const SegTerms& t) {
  return t.step_case == 1 ? (float)((double)lr_s * t.inv_bc1) : (float)((double)lr_s / t.bc1);
}

// Two block sums at once, guard_block_sum's order each; thread 0 stores the chunk's pair.  (Ends in a barrier: the next chunk
// of the same workgroup writes the same LDS words.)
__device__ __forceinline__ void seg_store_partial(double sa, double sb, double* lds, double* __restrict__ partials, int c) {
  sa = wave_sum_d(sa);
  sb = wave_sum_d(sb);
  if ((threadIdx.x & 63) == 0) {
    lds[threadIdx.x >> 6] = sa;
    lds[4 + (threadIdx.x >> 6)] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (long long)c] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
    partials[2 * (long long)c + 1] = ((lds[4] + lds[5]) + lds[6]) + lds[7];
  }
  __syncthreads();
}

__global__ __launch_bounds__(SEG_THREADS) void seg_sumsq_kernel(SegArgs a) {
  __shared__ double lds[8];
  if (a.guard && a.guard->skip) return;
  const float* __restrict__ x = a.p;
  const float* __restrict__ y = a.g;
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const int nv = ck.len >> 2, tail = ck.len & 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      const floatx4 xv = reinterpret_cast<const floatx4*>(x + ck.start)[i];
      a0 += (double)xv[0] * (double)xv[0];
      a1 += (double)xv[1] * (double)xv[1];
      a2 += (double)xv[2] * (double)xv[2];
      a3 += (double)xv[3] * (double)xv[3];
      if (y) {
        const floatx4 yv = reinterpret_cast<const floatx4*>(y + ck.start)[i];
        b0 += (double)yv[0] * (double)yv[0];
        b1 += (double)yv[1] * (double)yv[1];
        b2 += (double)yv[2] * (double)yv[2];
        b3 += (double)yv[3] * (double)yv[3];
      }
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      a0 += (double)x[i] * (double)x[i];
      if (y) b0 += (double)y[i] * (double)y[i];
    }
    seg_store_partial((a0 + a1) + (a2 + a3), (b0 + b1) + (b2 + b3), lds, a.partials, c);
  }
}

// The norm pass of LARS: per chunk the sums of p^2 and of d^2.
__global__ __launch_bounds__(SEG_THREADS) void sgd_table_norm_kernel(SegArgs a) {
  __shared__ double lds[8];
  SegTerms t;
  if (!seg_terms(a, false, t)) return;
  const float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const float wd = a.segs[ck.seg].weight_decay;
    const int nv = ck.len >> 2, tail = ck.len & 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      const floatx4 pv = reinterpret_cast<const floatx4*>(p + ck.start)[i];
      const floatx4 gv = reinterpret_cast<const floatx4*>(g + ck.start)[i];
      const float d0 = sgd_d(gv[0], pv[0], a.grad_scale, t.coef, wd), d1 = sgd_d(gv[1], pv[1], a.grad_scale, t.coef, wd);
      const float d2 = sgd_d(gv[2], pv[2], a.grad_scale, t.coef, wd), d3 = sgd_d(gv[3], pv[3], a.grad_scale, t.coef, wd);
      a0 += (double)pv[0] * (double)pv[0];
      a1 += (double)pv[1] * (double)pv[1];
      a2 += (double)pv[2] * (double)pv[2];
      a3 += (double)pv[3] * (double)pv[3];
      b0 += (double)d0 * (double)d0;
      b1 += (double)d1 * (double)d1;
      b2 += (double)d2 * (double)d2;
      b3 += (double)d3 * (double)d3;
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      const float pi = p[i], d = sgd_d(g[i], pi, a.grad_scale, t.coef, wd);
      a0 += (double)pi * (double)pi;
      b0 += (double)d * (double)d;
    }
    seg_store_partial((a0 + a1) + (a2 + a3), (b0 + b1) + (b2 + b3), lds, a.partials, c);
  }
}

// One wave per segment adds its chunks' pairs in index order; sums (nullable) takes them, trust (nullable) the factor
// (float)(eta * (sqrt(sum a) / sqrt(sum b))) of an adapted segment whose two sums are > 0, 1.0f otherwise.
// The adds are one dependent chain per sum — pair 0, 1, 2, ... exactly as a single thread would add them, which every lane does
// redundantly — but the loads are not: lane l fetches pair k0 + l of a tile of 64 (the next tile while this one is added) and
// the chain reads them lane by lane.  (One thread with one pair per round trip took 107 us over the 21.3 M parameters' 5 282
// partials — the largest tensor alone has 576 — three times the norm pass in front of it.)
__device__ __forceinline__ void seg_finish_tile(double a, double b, int cnt, double& sa, double& sb) {
  if (cnt == 64) {
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      sa += __shfl(a, j, 64);
      sb += __shfl(b, j, 64);
    }
    return;
  }
  for (int j = 0; j < cnt; ++j) {
    sa += __shfl(a, j, 64);
    sb += __shfl(b, j, 64);
  }
}

__global__ __launch_bounds__(64) void seg_finish_kernel(const avid_segment* __restrict__ segs, int S,
                                                        const double* __restrict__ partials, double eta,
                                                        double* __restrict__ sums, float* __restrict__ trust,
                                                        const avid_step_guard* __restrict__ guard) {
  if (guard && guard->skip) return;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= S) return;
  const avid_segment sg = segs[s];
  const long long nck = (sg.numel + AVID_SEG_CHUNK - 1) / AVID_SEG_CHUNK;
  const double* __restrict__ mine = partials + 2 * (long long)sg.first_chunk;
  double sa = 0.0, sb = 0.0, a = 0.0, b = 0.0;
  if (lane < nck) {
    a = mine[2 * lane];
    b = mine[2 * lane + 1];
  }
  for (long long k0 = 0; k0 < nck; k0 += 64) {
    const long long next = k0 + 64 + lane;
    double na = 0.0, nb = 0.0;
    if (next < nck) {
      na = mine[2 * next];
      nb = mine[2 * next + 1];
    }
    const long long left = nck - k0;
    seg_finish_tile(a, b, left < 64 ? (int)left : 64, sa, sb);
    a = na;
    b = nb;
  }
  if (lane != 0) return;
  if (sums) {
    sums[2 * s] = sa;
    sums[2 * s + 1] = sb;
  }
  if (trust) {
    float q = 1.f;
    if (sg.adapt && sa > 0.0 && sb > 0.0) q = (float)(eta * (sqrt(sa) / sqrt(sb)));
    trust[s] = q;
  }
}

__global__ __launch_bounds__(SEG_THREADS) void sgd_flat_table_kernel(SegArgs a) {
  SegTerms t;
  if (!seg_terms(a, false, t)) return;
  float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  float* __restrict__ buf = a.buf;
  float* __restrict__ e = a.e;
  const bool has_buf = buf != nullptr, nesterov = a.nesterov != 0;
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const avid_segment sg = a.segs[ck.seg];
    const float lr = seg_lr(t.lr, sg.lr_scale), wd = sg.weight_decay, q = a.trust ? a.trust[ck.seg] : 1.f;
    const int nv = ck.len >> 2, tail = ck.len & 3;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      floatx4 pv = reinterpret_cast<floatx4*>(p + ck.start)[i];
      const floatx4 gv = reinterpret_cast<const floatx4*>(g + ck.start)[i];
      floatx4 bv = {0.f, 0.f, 0.f, 0.f}, ev = {0.f, 0.f, 0.f, 0.f};
      if (has_buf) bv = reinterpret_cast<floatx4*>(buf + ck.start)[i];
      if (e) ev = reinterpret_cast<floatx4*>(e + ck.start)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], bj = bv[j];
        sgd_element(pj, gv[j], bj, has_buf, lr, a.momentum, wd, nesterov, a.grad_scale, t.coef, q);
        pv[j] = pj;
        bv[j] = bj;
        if (e) ev[j] = ema_element(ev[j], pj, t.w);
      }
      reinterpret_cast<floatx4*>(p + ck.start)[i] = pv;
      if (has_buf) reinterpret_cast<floatx4*>(buf + ck.start)[i] = bv;
      if (e) reinterpret_cast<floatx4*>(e + ck.start)[i] = ev;
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      float pi = p[i], bi = has_buf ? buf[i] : 0.f;
      sgd_element(pi, g[i], bi, has_buf, lr, a.momentum, wd, nesterov, a.grad_scale, t.coef, q);
      p[i] = pi;
      if (has_buf) buf[i] = bi;
      if (e) e[i] = ema_element(e[i], pi, t.w);
    }
  }
}

__global__ __launch_bounds__(SEG_THREADS) void adam_flat_table_kernel(SegArgs a) {
  SegTerms t;
  if (!seg_terms(a, true, t)) return;
  float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  float* __restrict__ m = a.m;
  float* __restrict__ v = a.v;
  float* __restrict__ e = a.e;
  const bool clip = t.coef != 1.f;   // (the clipped form is the unfused one here, vectors and tail; both use the vector-loop moments)
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const avid_segment sg = a.segs[ck.seg];
    const float step_size = seg_adam_step_size(seg_lr(t.lr, sg.lr_scale), t), wd = sg.weight_decay;
    const int nv = ck.len >> 2, tail = ck.len & 3;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      floatx4 pv = reinterpret_cast<floatx4*>(p + ck.start)[i];
      const floatx4 gv = reinterpret_cast<const floatx4*>(g + ck.start)[i];
      floatx4 mv = reinterpret_cast<floatx4*>(m + ck.start)[i];
      floatx4 vv = reinterpret_cast<floatx4*>(v + ck.start)[i];
      floatx4 ev = {0.f, 0.f, 0.f, 0.f};
      if (e) ev = reinterpret_cast<floatx4*>(e + ck.start)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        const float gg = clip ? adam_grad_term<GRAD_CLIPPED_SUM>(gv[j], pj, a.grad_scale, wd, t.coef)
                              : adam_grad_term<GRAD_UNCLIPPED>(gv[j], pj, a.grad_scale, wd, t.coef);
        adam_element<false>(pj, gg, mj, vj, a.b1, a.b2, a.eps, step_size, t.inv_sqrt_bc2);
        pv[j] = pj;
        mv[j] = mj;
        vv[j] = vj;
        if (e) ev[j] = ema_element(ev[j], pj, t.w);
      }
      reinterpret_cast<floatx4*>(p + ck.start)[i] = pv;
      reinterpret_cast<floatx4*>(m + ck.start)[i] = mv;
      reinterpret_cast<floatx4*>(v + ck.start)[i] = vv;
      if (e) reinterpret_cast<floatx4*>(e + ck.start)[i] = ev;
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      float pi = p[i], mi = m[i], vi = v[i];
      const float gg = clip ? adam_grad_term<GRAD_CLIPPED_SUM>(g[i], pi, a.grad_scale, wd, t.coef)
                            : adam_grad_term<GRAD_UNCLIPPED>(g[i], pi, a.grad_scale, wd, t.coef);
      adam_element<false>(pi, gg, mi, vi, a.b1, a.b2, a.eps, step_size, t.inv_sqrt_bc2);
      p[i] = pi;
      m[i] = mi;
      v[i] = vi;
      if (e) e[i] = ema_element(e[i], pi, t.w);
    }
  }
}

// LAMB.  The moments: Adam's vector-loop recurrences on gg = fma(g, grad_scale, 0 * p), which is (g * grad_scale) + 0.0f.
__device__ __forceinline__ void lamb_moments(float g, float& m, float& v, float b1, float b2, float grad_scale, float coef) {
#pragma clang fp contract(off)
  float gg = g * grad_scale;
  gg = gg * coef;
  gg = gg + 0.f;
  adam_moments<false>(gg, m, v, b1, b2);
}

// u = (m * c1) / (sqrt(v) * c2 + eps) + wd * p: the same operations in both passes.
__device__ __forceinline__ float lamb_u(float p, float m, float v, float c1, float c2, float eps, float wd) {
#pragma clang fp contract(off)
  const float mh = m * c1;
  float den = sqrtf(v) * c2;
  den = den + eps;
  float u = mh / den;
  if (wd != 0.f) {
    const float t = wd * p;
    u = u + t;
  }
  return u;
}

__global__ __launch_bounds__(SEG_THREADS) void lamb_moments_kernel(SegArgs a) {
  __shared__ double lds[8];
  SegTerms t;
  if (!seg_terms(a, true, t)) return;
  const float* __restrict__ p = a.p;
  const float* __restrict__ g = a.g;
  float* __restrict__ m = a.m;
  float* __restrict__ v = a.v;
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const float wd = a.segs[ck.seg].weight_decay;
    const int nv = ck.len >> 2, tail = ck.len & 3;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      const floatx4 pv = reinterpret_cast<const floatx4*>(p + ck.start)[i];
      const floatx4 gv = reinterpret_cast<const floatx4*>(g + ck.start)[i];
      floatx4 mv = reinterpret_cast<floatx4*>(m + ck.start)[i];
      floatx4 vv = reinterpret_cast<floatx4*>(v + ck.start)[i];
      float u[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float mj = mv[j], vj = vv[j];
        lamb_moments(gv[j], mj, vj, a.b1, a.b2, a.grad_scale, t.coef);
        mv[j] = mj;
        vv[j] = vj;
        u[j] = lamb_u(pv[j], mj, vj, t.c1, t.inv_sqrt_bc2, a.eps, wd);
      }
      reinterpret_cast<floatx4*>(m + ck.start)[i] = mv;
      reinterpret_cast<floatx4*>(v + ck.start)[i] = vv;
      a0 += (double)pv[0] * (double)pv[0];
      a1 += (double)pv[1] * (double)pv[1];
      a2 += (double)pv[2] * (double)pv[2];
      a3 += (double)pv[3] * (double)pv[3];
      b0 += (double)u[0] * (double)u[0];
      b1 += (double)u[1] * (double)u[1];
      b2 += (double)u[2] * (double)u[2];
      b3 += (double)u[3] * (double)u[3];
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      const float pi = p[i];
      float mi = m[i], vi = v[i];
      lamb_moments(g[i], mi, vi, a.b1, a.b2, a.grad_scale, t.coef);
      m[i] = mi;
      v[i] = vi;
      const float u = lamb_u(pi, mi, vi, t.c1, t.inv_sqrt_bc2, a.eps, wd);
      a0 += (double)pi * (double)pi;
      b0 += (double)u * (double)u;
    }
    seg_store_partial((a0 + a1) + (a2 + a3), (b0 + b1) + (b2 + b3), lds, a.partials, c);
  }
}

__device__ __forceinline__ float lamb_apply(float p, float u, float step) {
#pragma clang fp contract(off)
  const float s = step * u;
  return p - s;
}

__global__ __launch_bounds__(SEG_THREADS) void lamb_update_kernel(SegArgs a) {
  SegTerms t;
  if (!seg_terms(a, true, t)) return;
  float* __restrict__ p = a.p;
  const float* __restrict__ m = a.m;
  const float* __restrict__ v = a.v;
  float* __restrict__ e = a.e;
  for (int c = blockIdx.x; c < a.n_chunks; c += gridDim.x) {
    const avid_seg_chunk ck = a.chunks[c];
    const avid_segment sg = a.segs[ck.seg];
    const float step = seg_lr(seg_lr(t.lr, sg.lr_scale), a.trust[ck.seg]), wd = sg.weight_decay;
    const int nv = ck.len >> 2, tail = ck.len & 3;
    for (int i = threadIdx.x; i < nv; i += SEG_THREADS) {
      floatx4 pv = reinterpret_cast<floatx4*>(p + ck.start)[i];
      const floatx4 mv = reinterpret_cast<const floatx4*>(m + ck.start)[i];
      const floatx4 vv = reinterpret_cast<const floatx4*>(v + ck.start)[i];
      floatx4 ev = {0.f, 0.f, 0.f, 0.f};
      if (e) ev = reinterpret_cast<floatx4*>(e + ck.start)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float u = lamb_u(pv[j], mv[j], vv[j], t.c1, t.inv_sqrt_bc2, a.eps, wd);
        pv[j] = lamb_apply(pv[j], u, step);
        if (e) ev[j] = ema_element(ev[j], pv[j], t.w);
      }
      reinterpret_cast<floatx4*>(p + ck.start)[i] = pv;
      if (e) reinterpret_cast<floatx4*>(e + ck.start)[i] = ev;
    }
    if ((int)threadIdx.x < tail) {
      const long long i = ck.start + nv * 4 + threadIdx.x;
      const float u = lamb_u(p[i], m[i], v[i], t.c1, t.inv_sqrt_bc2, a.eps, wd);
      const float pi = lamb_apply(p[i], u, step);
      p[i] = pi;
      if (e) e[i] = ema_element(e[i], pi, t.w);
    }
  }
}

}  // namespace avid

using namespace avid;

// Blocks of 256 threads over `work` items (16-byte vectors, or scalar elements), one at least and 4096 at most: the kernels stride.
static unsigned flat_grid(long long work) {
  const long long grid = ceil_div(work > 0 ? work : 1, 256);
  return (unsigned)(grid > 4096 ? 4096 : grid);
}

// Adam's bias corrections from a step given by value (the kernels form them again from step_dev, where there is one).
struct AdamBias {
  double bc1, inv_bc1;     // 1 - beta1^step and its reciprocal
  float inv_sqrt_bc2;      // (float)(1 / sqrt(1 - beta2^step))
};

static AdamBias adam_bias(float beta1, float beta2, int64_t step) {
  if (step < 1) step = 1;
  AdamBias b;
  b.bc1 = 1.0 - pow((double)beta1, (double)step);
  b.inv_bc1 = 1.0 / b.bc1;
  b.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
  return b;
}

static int ema_desc_check(const char* who, const avid_ema_desc* ema, char* msg, size_t cap) {
  const char* bad = nullptr;
  if (!ema || !ema->ema) bad = "needs its average buffer";
  else if (((uintptr_t)ema->ema & 15) != 0) bad = "the average must be 16-byte aligned";
  else if (!(ema->decay >= 0.0 && ema->decay < 1.0)) bad = "decay must be in [0, 1)";
  else if (ema->warmup && !ema->updates_dev) bad = "warm-up needs the device counter of updates";
  else if (((uintptr_t)ema->updates_dev & 7) != 0) bad = "the counter of updates must be 8-byte aligned";
  if (!bad) return 0;
  snprintf(msg, cap, "%s: %s", who, bad);
  return 1;
}

// ---- the flat optimizers
// The three entry points of an optimizer differ in what they take besides the buffers: nothing; a guard record, required (its
// alignment is not looked at); with `averaging`, a record that may be null and an averaging descriptor, both checked here.
static int flat_average(const char* who, bool averaging, const avid_step_guard* guard, const avid_ema_desc* ema, EmaFlatArgs& avg) {
  memset(&avg, 0, sizeof avg);
  if (!averaging) return AVID_OK;
  AVID_REQUIRE(((uintptr_t)guard & 7) == 0, AVID_E_BADARG, "%s: the guard record must be 8-byte aligned", who);
  char msg[128];
  AVID_REQUIRE(!ema_desc_check(who, ema, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  avg.e = ema->ema;
  avg.decay = ema->decay;
  avg.warmup = (int)ema->warmup;
  avg.updates_dev = (const long long*)ema->updates_dev;
  return AVID_OK;
}

static int adam_flat_launch(const char* who, bool guarded, bool averaging, int64_t n, float* p, const float* g, float* m, float* v,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                            const int64_t* step_dev, const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                            const avid_ema_desc* ema, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && p && g && m && v && (guard || !guarded) && (step >= 1 || step_dev), AVID_E_BADARG, "%s: bad argument", who);
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, AVID_E_BADARG,
               "%s: buffers must be 16-byte aligned", who);
  EmaFlatArgs avg;
  if (int rc = flat_average(who, averaging, guard, ema, avg)) return rc;
  const AdamBias bias = adam_bias(beta1, beta2, step);
  const AdamFlatArgs a = {p, g, m, v, n / 4, n, beta1, beta2, eps, weight_decay, (float)((double)lr / bias.bc1), bias.inv_bc1,
                          bias.inv_sqrt_bc2, grad_scale, lr, (const long long*)step_dev, lr_dev};
  const dim3 grid(flat_grid(a.n4)), block(FLAT_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const double bytes = (averaging ? 36.0 : 28.0) * n;
  if (averaging && guard) {
    ScopedTimer t(s, "adam_flat_ema_guarded_kernel", 0.0, bytes);
    hipLaunchKernelGGL(adam_flat_ema_guarded_kernel, grid, block, 0, s, a, avg, guard);
  } else if (averaging) {
    ScopedTimer t(s, "adam_flat_ema_kernel", 0.0, bytes);
    hipLaunchKernelGGL(adam_flat_ema_kernel, grid, block, 0, s, a, avg);
  } else if (guard) {
    ScopedTimer t(s, "adam_flat_guarded_kernel", 0.0, bytes);
    hipLaunchKernelGGL(adam_flat_guarded_kernel, grid, block, 0, s, a, guard);
  } else {
    ScopedTimer t(s, "adam_flat_kernel", 0.0, bytes);
    hipLaunchKernelGGL(adam_flat_kernel, grid, block, 0, s, a);
  }
  return check_launch(who);
}

static int sgd_flat_launch(const char* who, bool guarded, bool averaging, int64_t n, float* p, const float* g, float* buf, float lr,
                           float momentum, float weight_decay, int nesterov, const float* lr_dev, float grad_scale,
                           const avid_step_guard* guard, const avid_ema_desc* ema, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && p && g && (guard || !guarded), AVID_E_BADARG, "%s: bad argument", who);
  AVID_REQUIRE(buf || momentum == 0.f, AVID_E_BADARG, "%s: momentum needs its buffer", who);
  if (momentum == 0.f) buf = nullptr;   // (the kernels take the buffer as the switch)
  AVID_REQUIRE(!nesterov || momentum != 0.f, AVID_E_BADARG, "%s: nesterov needs momentum", who);
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0, AVID_E_BADARG, "%s: buffers must be 16-byte aligned",
               who);
  EmaFlatArgs avg;
  if (int rc = flat_average(who, averaging, guard, ema, avg)) return rc;
  const SgdFlatArgs a = {p, g, buf, n / 4, n, lr, momentum, weight_decay, nesterov, grad_scale, lr_dev};
  const dim3 grid(flat_grid(a.n4)), block(FLAT_THREADS);
  hipStream_t s = (hipStream_t)stream;
  const double bytes = ((buf ? 20.0 : 12.0) + (averaging ? 8.0 : 0.0)) * n;
  if (averaging && guard) {
    ScopedTimer t(s, "sgd_flat_ema_guarded_kernel", 0.0, bytes);
    hipLaunchKernelGGL(sgd_flat_ema_guarded_kernel, grid, block, 0, s, a, avg, guard);
  } else if (averaging) {
    ScopedTimer t(s, "sgd_flat_ema_kernel", 0.0, bytes);
    hipLaunchKernelGGL(sgd_flat_ema_kernel, grid, block, 0, s, a, avg);
  } else if (guard) {
    ScopedTimer t(s, "sgd_flat_guarded_kernel", 0.0, bytes);
    hipLaunchKernelGGL(sgd_flat_guarded_kernel, grid, block, 0, s, a, guard);
  } else {
    ScopedTimer t(s, "sgd_flat_kernel", 0.0, bytes);
    hipLaunchKernelGGL(sgd_flat_kernel, grid, block, 0, s, a);
  }
  return check_launch(who);
}

extern "C" int avid_adam_flat(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                              const float* lr_dev, float grad_scale, avid_stream_t stream) {
  return adam_flat_launch("adam_flat", false, false, n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, step_dev, lr_dev,
                          grad_scale, nullptr, nullptr, stream);
}

extern "C" int avid_adam_flat_guarded(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                                      float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                                      const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                                      avid_stream_t stream) {
  return adam_flat_launch("adam_flat_guarded", true, false, n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, step_dev,
                          lr_dev, grad_scale, guard, nullptr, stream);
}

extern "C" int avid_adam_flat_ema(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, int64_t step, const int64_t* step_dev, const float* lr_dev,
                                  float grad_scale, const avid_step_guard* guard, const avid_ema_desc* ema,
                                  avid_stream_t stream) {
  return adam_flat_launch("adam_flat_ema", false, true, n, p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, step_dev, lr_dev,
                          grad_scale, guard, ema, stream);
}

extern "C" int avid_sgd_flat(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                             int nesterov, const float* lr_dev, float grad_scale, avid_stream_t stream) {
  return sgd_flat_launch("sgd_flat", false, false, n, p, g, buf, lr, momentum, weight_decay, nesterov, lr_dev, grad_scale, nullptr,
                         nullptr, stream);
}

extern "C" int avid_sgd_flat_guarded(int64_t n, float* p, const float* g, float* buf, float lr, float momentum,
                                     float weight_decay, int nesterov, const float* lr_dev, float grad_scale,
                                     const avid_step_guard* guard, avid_stream_t stream) {
  return sgd_flat_launch("sgd_flat_guarded", true, false, n, p, g, buf, lr, momentum, weight_decay, nesterov, lr_dev, grad_scale,
                         guard, nullptr, stream);
}

extern "C" int avid_sgd_flat_ema(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                                 int nesterov, const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                                 const avid_ema_desc* ema, avid_stream_t stream) {
  return sgd_flat_launch("sgd_flat_ema", false, true, n, p, g, buf, lr, momentum, weight_decay, nesterov, lr_dev, grad_scale, guard,
                         ema, stream);
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

// ---- the step guard
static long long guard_blocks(int64_t n) {
  long long b = ceil_div(n, GUARD_THREADS * 4);
  return b < 1 ? 1 : (b > GUARD_MAX_BLOCKS ? GUARD_MAX_BLOCKS : b);
}

extern "C" size_t avid_grad_guard_workspace_bytes(int64_t n) { return n > 0 ? (size_t)guard_blocks(n) * sizeof(double) : 0; }

extern "C" int avid_grad_guard(int64_t n, const float* g, float grad_scale, float max_norm, int skip_nonfinite,
                               avid_step_guard* guard_dev, void* ws, size_t ws_bytes, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && g && guard_dev && ws, AVID_E_BADARG, "grad_guard: bad argument");
  AVID_REQUIRE(ws_bytes >= avid_grad_guard_workspace_bytes(n), AVID_E_BADARG, "grad_guard: workspace too small");
  AVID_REQUIRE(((uintptr_t)g & 3) == 0 && (((uintptr_t)guard_dev | (uintptr_t)ws) & 7) == 0, AVID_E_BADARG,
               "grad_guard: the gradient must be 4-byte, the record and the workspace 8-byte aligned");
  long long head = (long long)(((16 - ((uintptr_t)g & 15)) & 15) / 4);   // scalar elements in front of the first 16-byte boundary
  if (head > n) head = n;
  const long long n4 = (n - head) / 4;
  const int blocks = (int)guard_blocks(n);
  {
    ScopedTimer t((hipStream_t)stream, "grad_sumsq_kernel", 2.0 * n, 4.0 * n);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(GUARD_THREADS), 0, (hipStream_t)stream, g, (long long)n,
                       (int)head, n4, (double*)ws);
  }
  int rc = check_launch("grad_guard");
  if (rc != AVID_OK) return rc;
  ScopedTimer t((hipStream_t)stream, "grad_guard_finish_kernel", 0.0, 8.0 * blocks);
  hipLaunchKernelGGL(grad_guard_finish_kernel, dim3(1), dim3(GUARD_THREADS), 0, (hipStream_t)stream, (const double*)ws, blocks,
                     grad_scale, max_norm, skip_nonfinite, guard_dev);
  return check_launch("grad_guard");
}

extern "C" int avid_guard_nonfinite(int64_t n, const float* x, avid_step_guard* guard, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && x && guard, AVID_E_BADARG, "guard_nonfinite: bad argument");
  AVID_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)guard & 7) == 0, AVID_E_BADARG, "guard_nonfinite: misaligned pointer");
  ScopedTimer t((hipStream_t)stream, "guard_nonfinite_kernel", 0.0, 4.0 * n);
  hipLaunchKernelGGL(guard_nonfinite_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, (long long)n, guard);
  return check_launch("guard_nonfinite");
}

extern "C" int avid_counter_add_unless(uint64_t* counter, uint64_t inc, const avid_step_guard* guard, avid_stream_t stream) {
  AVID_REQUIRE(counter && guard, AVID_E_BADARG, "counter_add_unless: null pointer");
  hipLaunchKernelGGL(counter_add_unless_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)counter,
                     (unsigned long long)inc, guard);
  return check_launch("counter_add_unless");
}

extern "C" int avid_guard_restore(int64_t rows, int64_t D, float* dst, const int64_t* idx, const float* saved,
                                  const avid_step_guard* guard, avid_stream_t stream) {
  AVID_REQUIRE(rows > 0 && D > 0 && dst && saved && guard, AVID_E_BADARG, "guard_restore: bad argument");
  long long grid = ceil_div(rows * D, 256);
  if (grid > 1024) grid = 1024;
  ScopedTimer t((hipStream_t)stream, "guard_restore_kernel", 0.0, 0.0);
  hipLaunchKernelGGL(guard_restore_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (long long)rows,
                     (long long)D, dst, (const long long*)idx, saved, guard);
  return check_launch("guard_restore");
}

// ---- the weight average (EMA)
extern "C" int avid_ema_flat(int64_t n, float* e, const float* p, double decay, int warmup, const int64_t* updates_dev,
                             const avid_step_guard* guard, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && e && p, AVID_E_BADARG, "ema_flat: bad argument");
  AVID_REQUIRE((((uintptr_t)e | (uintptr_t)p) & 15) == 0, AVID_E_BADARG, "ema_flat: buffers must be 16-byte aligned");
  AVID_REQUIRE(decay >= 0.0 && decay < 1.0, AVID_E_BADARG, "ema_flat: decay must be in [0, 1)");
  AVID_REQUIRE(!warmup || updates_dev, AVID_E_BADARG, "ema_flat: warm-up needs the device counter of updates");
  AVID_REQUIRE((((uintptr_t)updates_dev | (uintptr_t)guard) & 7) == 0, AVID_E_BADARG,
               "ema_flat: the counter and the guard record must be 8-byte aligned");
  const long long n4 = n / 4;
  ScopedTimer t((hipStream_t)stream, "ema_flat_kernel", 0.0, 12.0 * n);
  hipLaunchKernelGGL(ema_flat_kernel, dim3(flat_grid(n4)), dim3(256), 0, (hipStream_t)stream, e, p, n4, (long long)n, decay,
                     warmup, (const long long*)updates_dev, guard);
  return check_launch("ema_flat");
}

extern "C" int avid_swap_flat(int64_t n, float* a, float* b, avid_stream_t stream) {
  AVID_REQUIRE(n > 0 && a && b, AVID_E_BADARG, "swap_flat: bad argument");
  AVID_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, AVID_E_BADARG, "swap_flat: buffers must be 4-byte aligned");
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  AVID_REQUIRE(a0 + bytes <= b0 || b0 + bytes <= a0, AVID_E_BADARG, "swap_flat: the two buffers overlap");
  const bool vec = ((a0 | b0) & 15) == 0;
  const long long n4 = vec ? n / 4 : 0;
  const long long work = vec ? (n4 > 0 ? n4 : 1) : (long long)n;
  long long grid = ceil_div(work, 256);
  if (grid > 4096) grid = 4096;
  ScopedTimer t((hipStream_t)stream, "swap_flat_kernel", 0.0, 16.0 * n);
  hipLaunchKernelGGL(swap_flat_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, n4, (long long)n);
  return check_launch("swap_flat");
}

// ---- segment tables
extern "C" int avid_segment_chunks(int32_t S, avid_segment* segs, avid_seg_chunk* chunks, int32_t cap) {
  AVID_REQUIRE(S > 0 && segs, AVID_E_BADARG, "segment_chunks: bad argument");
  long long c = 0;
  for (int s = 0; s < S; ++s) {
    AVID_REQUIRE(segs[s].numel > 0, AVID_E_BADARG, "segment_chunks: segment %d has numel %lld", s, (long long)segs[s].numel);
    const long long nck = (segs[s].numel + AVID_SEG_CHUNK - 1) / AVID_SEG_CHUNK;
    AVID_REQUIRE(c + nck < (1ll << 31), AVID_E_BADARG, "segment_chunks: too many chunks");
    segs[s].first_chunk = (int32_t)c;
    if (chunks) {
      AVID_REQUIRE(c + nck <= cap, AVID_E_BADARG, "segment_chunks: the chunk list holds %d records, segment %d ends at %lld",
                   cap, s, c + nck);
      for (long long k = 0; k < nck; ++k) {
        const long long left = segs[s].numel - k * AVID_SEG_CHUNK;
        chunks[c + k].start = segs[s].offset + k * AVID_SEG_CHUNK;
        chunks[c + k].len = (int32_t)(left < AVID_SEG_CHUNK ? left : AVID_SEG_CHUNK);
        chunks[c + k].seg = s;
      }
    }
    c += nck;
  }
  return (int)c;
}

// The host copy of a table against the n of the call: a message (and 1) for the first thing that is wrong.  total: the
// elements the segments hold.
static int table_check(const char* who, const avid_segment_table* t, int64_t n, long long* total, char* msg, size_t cap) {
  *total = 0;
  if (!t || t->S <= 0 || t->n_chunks <= 0 || !t->seg_host || !t->seg_dev || !t->chunk_host || !t->chunk_dev || n <= 0) {
    snprintf(msg, cap, "%s: bad segment table (null pointer, S <= 0 or n <= 0)", who);
    return 1;
  }
  if ((((uintptr_t)t->seg_dev | (uintptr_t)t->chunk_dev) & 7) != 0) {
    snprintf(msg, cap, "%s: the device copies of the segment table must be 8-byte aligned", who);
    return 1;
  }
  long long end = 0, c = 0;
  for (int s = 0; s < t->S; ++s) {
    const avid_segment& g = t->seg_host[s];
    const char* bad = nullptr;
    if (g.offset < 0 || (g.offset & 3) != 0) bad = "offset is negative or not 16-byte aligned";
    else if (g.offset < end) bad = "offset lies inside or in front of the segment before (not increasing, or overlapping)";
    else if (g.numel <= 0) bad = "numel <= 0";
    else if (g.numel > n || g.offset > n - g.numel) bad = "offset + numel exceeds n";
    else if (!(g.lr_scale - g.lr_scale == 0.f) || !(g.weight_decay - g.weight_decay == 0.f)) bad = "lr_scale or weight_decay is not finite";
    else if (g.adapt != 0 && g.adapt != 1) bad = "adapt is neither 0 nor 1";
    else if (g.first_chunk != c) bad = "first_chunk is not what avid_segment_chunks gives";
    if (bad) {
      snprintf(msg, cap, "%s: segment %d: %s", who, s, bad);
      return 1;
    }
    const long long nck = (g.numel + AVID_SEG_CHUNK - 1) / AVID_SEG_CHUNK;
    if (c + nck > t->n_chunks) {
      snprintf(msg, cap, "%s: the chunk list is shorter than segment %d needs", who, s);
      return 1;
    }
    for (long long k = 0; k < nck; ++k) {
      const avid_seg_chunk& ck = t->chunk_host[c + k];
      const long long left = g.numel - k * AVID_SEG_CHUNK;
      if (ck.start != g.offset + k * AVID_SEG_CHUNK || ck.len != (left < AVID_SEG_CHUNK ? left : AVID_SEG_CHUNK) || ck.seg != s) {
        snprintf(msg, cap, "%s: chunk %lld is not what avid_segment_chunks gives for segment %d", who, c + k, s);
        return 1;
      }
    }
    c += nck;
    end = g.offset + g.numel;
    *total += g.numel;
  }
  if (c != t->n_chunks) {
    snprintf(msg, cap, "%s: the chunk list holds %d records, the segments need %lld", who, t->n_chunks, c);
    return 1;
  }
  return 0;
}

static unsigned seg_grid(int n_chunks) {
  const long long cap = 4ll * device_cus();
  return (unsigned)(n_chunks < cap ? n_chunks : cap);
}

static SegArgs seg_args(const avid_segment_table* t) {
  SegArgs a;
  memset(&a, 0, sizeof a);
  a.segs = t->seg_dev;
  a.chunks = t->chunk_dev;
  a.n_chunks = t->n_chunks;
  a.grad_scale = 1.f;
  a.bc1 = a.inv_bc1 = 1.0;
  a.inv_sqrt_bc2 = 1.f;
  return a;
}

static void seg_args_ema(SegArgs& a, const avid_ema_desc* ema) {
  if (!ema) return;
  a.e = ema->ema;
  a.decay = ema->decay;
  a.warmup = (int)ema->warmup;
  a.updates_dev = (const long long*)ema->updates_dev;
}

static void seg_args_adam(SegArgs& a, float beta1, float beta2, float eps, int64_t step, const int64_t* step_dev) {
  const AdamBias bias = adam_bias(beta1, beta2, step);
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.bc1 = bias.bc1;
  a.inv_bc1 = bias.inv_bc1;
  a.inv_sqrt_bc2 = bias.inv_sqrt_bc2;
  a.step_dev = (const long long*)step_dev;
}

extern "C" size_t avid_segment_sumsq_workspace_bytes(const avid_segment_table* table) {
  return table && table->n_chunks > 0 ? (size_t)table->n_chunks * 2 * sizeof(double) : 0;
}

static int seg_finish(const char* who, const avid_segment_table* t, const double* partials, double eta, double* sums,
                      float* trust, const avid_step_guard* guard, hipStream_t s) {
  ScopedTimer tm(s, "seg_finish_kernel", 0.0, 16.0 * t->n_chunks);
  hipLaunchKernelGGL(seg_finish_kernel, dim3((unsigned)t->S), dim3(64), 0, s, t->seg_dev, (int)t->S, partials, eta,
                     sums, trust, guard);
  return check_launch(who);
}

extern "C" int avid_segment_sumsq(const avid_segment_table* table, int64_t n, const float* x, const float* y, double* sums,
                                  const avid_step_guard* guard, void* ws, size_t ws_bytes, avid_stream_t stream) {
  char msg[192];
  long long total;
  AVID_REQUIRE(!table_check("segment_sumsq", table, n, &total, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  AVID_REQUIRE(x && sums && ws, AVID_E_BADARG, "segment_sumsq: null pointer");
  AVID_REQUIRE(ws_bytes >= avid_segment_sumsq_workspace_bytes(table), AVID_E_BADARG, "segment_sumsq: workspace too small");
  AVID_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0 && (((uintptr_t)sums | (uintptr_t)ws | (uintptr_t)guard) & 7) == 0,
               AVID_E_BADARG, "segment_sumsq: x and y must be 16-byte, sums, the workspace and the guard record 8-byte aligned");
  SegArgs a = seg_args(table);
  a.p = const_cast<float*>(x);
  a.g = y;
  a.guard = guard;
  a.partials = (double*)ws;
  {
    ScopedTimer t((hipStream_t)stream, "seg_sumsq_kernel", 2.0 * total, (y ? 8.0 : 4.0) * total);
    hipLaunchKernelGGL(seg_sumsq_kernel, dim3(seg_grid(table->n_chunks)), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
  }
  int rc = check_launch("segment_sumsq");
  if (rc != AVID_OK) return rc;
  return seg_finish("segment_sumsq", table, (const double*)ws, 1.0, sums, nullptr, guard, (hipStream_t)stream);
}

extern "C" int avid_sgd_flat_table(const avid_segment_table* table, int64_t n, float* p, const float* g, float* buf, float lr,
                                   float momentum, int nesterov, const float* lr_dev, float grad_scale, float trust_coefficient,
                                   float* trust, const avid_step_guard* guard, const avid_ema_desc* ema, void* ws,
                                   size_t ws_bytes, avid_stream_t stream) {
  char msg[192];
  long long total;
  AVID_REQUIRE(!table_check("sgd_flat_table", table, n, &total, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  AVID_REQUIRE(p && g, AVID_E_BADARG, "sgd_flat_table: null pointer");
  AVID_REQUIRE(buf || momentum == 0.f, AVID_E_BADARG, "sgd_flat_table: momentum needs its buffer");
  if (momentum == 0.f) buf = nullptr;
  AVID_REQUIRE(!nesterov || momentum != 0.f, AVID_E_BADARG, "sgd_flat_table: nesterov needs momentum");
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0, AVID_E_BADARG,
               "sgd_flat_table: buffers must be 16-byte aligned");
  AVID_REQUIRE((((uintptr_t)guard | (uintptr_t)ws) & 7) == 0 && ((uintptr_t)trust & 3) == 0, AVID_E_BADARG,
               "sgd_flat_table: the guard record and the workspace must be 8-byte, the trust array 4-byte aligned");
  if (ema) AVID_REQUIRE(!ema_desc_check("sgd_flat_table", ema, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  if (trust) {
    AVID_REQUIRE(trust_coefficient > 0.f && trust_coefficient - trust_coefficient == 0.f, AVID_E_BADARG,
                 "sgd_flat_table: the trust coefficient must be finite and > 0");
    AVID_REQUIRE(ws && ws_bytes >= avid_segment_sumsq_workspace_bytes(table), AVID_E_BADARG,
                 "sgd_flat_table: the trust factors need the workspace of avid_segment_sumsq_workspace_bytes");
  }
  SegArgs a = seg_args(table);
  a.p = p;
  a.g = g;
  a.buf = buf;
  a.lr = lr;
  a.momentum = momentum;
  a.nesterov = nesterov;
  a.lr_dev = lr_dev;
  a.grad_scale = grad_scale;
  a.guard = guard;
  a.trust = trust;
  a.partials = (double*)ws;
  seg_args_ema(a, ema);
  const unsigned grid = seg_grid(table->n_chunks);
  if (trust) {
    {
      ScopedTimer t((hipStream_t)stream, "sgd_table_norm_kernel", 4.0 * total, 8.0 * total);
      hipLaunchKernelGGL(sgd_table_norm_kernel, dim3(grid), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
    }
    int rc = check_launch("sgd_flat_table");
    if (rc != AVID_OK) return rc;
    rc = seg_finish("sgd_flat_table", table, (const double*)ws, (double)trust_coefficient, nullptr, trust, guard,
                    (hipStream_t)stream);
    if (rc != AVID_OK) return rc;
  }
  ScopedTimer t((hipStream_t)stream, "sgd_flat_table_kernel", 0.0, ((buf ? 20.0 : 12.0) + (ema ? 8.0 : 0.0)) * total);
  hipLaunchKernelGGL(sgd_flat_table_kernel, dim3(grid), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("sgd_flat_table");
}

extern "C" int avid_adam_flat_table(const avid_segment_table* table, int64_t n, float* p, const float* g, float* m, float* v,
                                    float lr, float beta1, float beta2, float eps, int64_t step, const int64_t* step_dev,
                                    const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                                    const avid_ema_desc* ema, avid_stream_t stream) {
  char msg[192];
  long long total;
  AVID_REQUIRE(!table_check("adam_flat_table", table, n, &total, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  AVID_REQUIRE(p && g && m && v && (step >= 1 || step_dev), AVID_E_BADARG, "adam_flat_table: bad argument");
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, AVID_E_BADARG,
               "adam_flat_table: buffers must be 16-byte aligned");
  AVID_REQUIRE((((uintptr_t)guard | (uintptr_t)step_dev) & 7) == 0, AVID_E_BADARG,
               "adam_flat_table: the guard record and the step counter must be 8-byte aligned");
  if (ema) AVID_REQUIRE(!ema_desc_check("adam_flat_table", ema, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  SegArgs a = seg_args(table);
  a.p = p;
  a.g = g;
  a.m = m;
  a.v = v;
  a.lr = lr;
  a.lr_dev = lr_dev;
  a.grad_scale = grad_scale;
  a.guard = guard;
  seg_args_adam(a, beta1, beta2, eps, step, step_dev);
  seg_args_ema(a, ema);
  ScopedTimer t((hipStream_t)stream, "adam_flat_table_kernel", 0.0, (ema ? 36.0 : 28.0) * total);
  hipLaunchKernelGGL(adam_flat_table_kernel, dim3(seg_grid(table->n_chunks)), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("adam_flat_table");
}

extern "C" int avid_lamb_flat(const avid_segment_table* table, int64_t n, float* p, const float* g, float* m, float* v, float lr,
                              float beta1, float beta2, float eps, int64_t step, const int64_t* step_dev, const float* lr_dev,
                              float grad_scale, float* trust, const avid_step_guard* guard, const avid_ema_desc* ema, void* ws,
                              size_t ws_bytes, avid_stream_t stream) {
  char msg[192];
  long long total;
  AVID_REQUIRE(!table_check("lamb_flat", table, n, &total, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  AVID_REQUIRE(p && g && m && v && trust && ws && (step >= 1 || step_dev), AVID_E_BADARG, "lamb_flat: bad argument");
  AVID_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, AVID_E_BADARG,
               "lamb_flat: buffers must be 16-byte aligned");
  AVID_REQUIRE((((uintptr_t)guard | (uintptr_t)step_dev | (uintptr_t)ws) & 7) == 0 && ((uintptr_t)trust & 3) == 0, AVID_E_BADARG,
               "lamb_flat: the guard record, the step counter and the workspace must be 8-byte, the trust array 4-byte aligned");
  AVID_REQUIRE(ws_bytes >= avid_segment_sumsq_workspace_bytes(table), AVID_E_BADARG, "lamb_flat: workspace too small");
  if (ema) AVID_REQUIRE(!ema_desc_check("lamb_flat", ema, msg, sizeof msg), AVID_E_BADARG, "%s", msg);
  SegArgs a = seg_args(table);
  a.p = p;
  a.g = g;
  a.m = m;
  a.v = v;
  a.lr = lr;
  a.lr_dev = lr_dev;
  a.grad_scale = grad_scale;
  a.guard = guard;
  a.trust = trust;
  a.partials = (double*)ws;
  seg_args_adam(a, beta1, beta2, eps, step, step_dev);
  seg_args_ema(a, ema);
  const unsigned grid = seg_grid(table->n_chunks);
  {
    ScopedTimer t((hipStream_t)stream, "lamb_moments_kernel", 4.0 * total, 24.0 * total);
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(grid), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
  }
  int rc = check_launch("lamb_flat");
  if (rc != AVID_OK) return rc;
  rc = seg_finish("lamb_flat", table, (const double*)ws, 1.0, nullptr, trust, guard, (hipStream_t)stream);
  if (rc != AVID_OK) return rc;
  ScopedTimer t((hipStream_t)stream, "lamb_update_kernel", 0.0, (ema ? 24.0 : 16.0) * total);
  hipLaunchKernelGGL(lamb_update_kernel, dim3(grid), dim3(SEG_THREADS), 0, (hipStream_t)stream, a);
  return check_launch("lamb_flat");
}
