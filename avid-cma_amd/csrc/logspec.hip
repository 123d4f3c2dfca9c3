// Log-spectrogram front end on the GPU: the reference computes it per clip on CPU
// workers with librosa (datasets/preprocessing.py:158-186); here a whole batch of mono clips goes
//     frames (reflect-centred, Hann-windowed)  ->  DFT as one fp32-MFMA GEMM against a cos | -sin basis
//     ->  power, bin-pair mean, dB, per-clip top_db floor, optional z-score          -> [B, 1, T, n_fft/2 + 1]
// The DFT-by-GEMM costs 2*T*n*(n+2) FLOP per clip (0.42 GFLOP at n = 1024, T = 200) — 100x an FFT's count
// but one launch of the convolution kernel, with no FFT library or twiddle plumbing; at batch 64 it is
// 27 GFLOP, a fraction of a millisecond next to the 16 ms training step.
#include <math.h>

#include "common.h"

namespace avid {

// basis[j][k]: j < F: cos(2 pi j k / n);  F <= j < 2F: -sin(2 pi (j - F) k / n);  else 0  (rows = GEMM N, [N][K])
__global__ void logspec_basis_kernel(float* __restrict__ basis, int n, int F, int Npad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Npad * n) return;
  const int k = (int)(i % n), j = (int)(i / n);
  float v = 0.f;
  if (j < 2 * F) {
    const int bin = j < F ? j : j - F;
    const int m = (int)(((long long)bin * k) % n);                 // exact argument reduction
    const double a = 2.0 * M_PI * (double)m / (double)n;
    v = j < F ? (float)cos(a) : (float)(-sin(a));
  }
  basis[i] = v;
}

// A[(b*T + t)][k] = hann[k] * x[b][reflect(t*hop + k - n/2)]
__global__ void logspec_frames_kernel(const float* __restrict__ sig, float* __restrict__ A, int B, int L, int n, int hop,
                                      int T) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * T * n) return;
  const int k = (int)(i % n);
  const long long r = i / n;
  const int t = (int)(r % T), b = (int)(r / T);
  int p = t * hop + k - n / 2;
  if (p < 0) p = -p;
  if (p >= L) p = 2 * (L - 1) - p;
  const float w = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)n));
  A[i] = w * sig[(long long)b * L + p];
}

// ---- the same front end from the decoder's int16 samples (include/avid_hip.h: avid_pcm_desc) ----------------------------
// The reference's AudioPrep (datasets/preprocessing.py:116-155) on what av_laod_audio returns (data / np.iinfo(int16).max,
// float64): .mean(0).astype(float32), trim / zero-pad to L, sig *= gain.  numpy sums the channels one after the other in
// float64 and divides by their count; the in-place gain is a float32 multiply.  pcm_prepared is that arithmetic, in one place:
// audio_prep_kernel writes it out, logspec_frames_pcm_kernel windows it where logspec_frames_kernel windows sig[b][p].
struct PcmDev {
  const int16_t* s;   // planar [channels][n], 2-byte aligned
  int channels, n;
  float gain;
};

__device__ __forceinline__ float pcm_prepared(const PcmDev& c, int p) {
  float v = 0.f;
  if (p < c.n) {
    double acc = (double)c.s[p] / 32767.0;
    for (int ch = 1; ch < c.channels; ++ch) acc += (double)c.s[(long long)ch * c.n + p] / 32767.0;
    v = (float)(acc / (double)c.channels);
  }
  return v * c.gain;
}

// out[b][p] = prepared(b, p): one thread per output sample
__global__ void audio_prep_kernel(const PcmDev* __restrict__ clips, float* __restrict__ out, int B, int L) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * L) return;
  out[i] = pcm_prepared(clips[i / L], (int)(i % L));
}

// A[(b*T + t)][k] = hann[k] * prepared(b, reflect(t*hop + k - n/2)): logspec_frames_kernel without the waveform in between
__global__ void logspec_frames_pcm_kernel(const PcmDev* __restrict__ clips, float* __restrict__ A, int B, int L, int n, int hop,
                                          int T) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * T * n) return;
  const int k = (int)(i % n);
  const long long r = i / n;
  const int t = (int)(r % T), b = (int)(r / T);
  int p = t * hop + k - n / 2;
  if (p < 0) p = -p;
  if (p >= L) p = 2 * (L - 1) - p;
  const float w = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)k / (double)n));
  A[i] = w * pcm_prepared(clips[b], p);
}

__device__ __forceinline__ int float_order(float v) {   // monotone float -> int map (for atomicMax)
  const int i = __float_as_int(v);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float order_float(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void logspec_init_kernel(int* __restrict__ mx, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) mx[i] = float_order(-INFINITY);
}

// C[(b*T + t)][Npad] (re | im) -> db[b][t][fo], per-clip maximum
__global__ void logspec_db_kernel(const float* __restrict__ C, float* __restrict__ db, int* __restrict__ mx, int B, int T,
                                  int F, int Fo, int Npad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float v = -INFINITY;
  int b = 0;
  if (i < (long long)B * T * Fo) {
    const int fo = (int)(i % Fo);
    const long long r = i / Fo;
    b = (int)(r / T);
    const float* row = C + r * Npad;
    auto power = [&](int f) { return row[f] * row[f] + row[F + f] * row[F + f]; };
    const float S = fo == 0 ? power(0) : 0.5f * (power(2 * fo - 1) + power(2 * fo));
    v = 10.f * log10f(fmaxf(1e-10f, S));
    db[i] = v;
  }
  // one atomic per wave when the wave sits inside one clip (the common case), else per lane
  const int b0 = __shfl(b, 0, 64);
  const bool uniform = __all(b == b0 || v == -INFINITY);
  if (uniform) {
    float m = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m != -INFINITY) atomicMax(&mx[b0], float_order(m));
  } else if (v != -INFINITY) {
    atomicMax(&mx[b], float_order(v));
  }
}

__global__ void logspec_finish_kernel(float* __restrict__ out, const int* __restrict__ mx, const float* __restrict__ mean,
                                      const float* __restrict__ stdv, int B, int T, int Fo, float top_db) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * T * Fo) return;
  const int fo = (int)(i % Fo);
  const int b = (int)(i / ((long long)T * Fo));
  float v = fmaxf(out[i], order_float(mx[b]) - top_db);
  if (mean) v = (v - mean[fo]) / (stdv[fo] + 1e-5f);
  out[i] = v;
}

}  // namespace avid

using namespace avid;

static int logspec_npad(int n) { return (2 * (n / 2 + 1) + 63) / 64 * 64; }

extern "C" size_t avid_logspec_basis_floats(int n_stft) {
  if (n_stft < 64 || n_stft % 32) return 0;
  return (size_t)logspec_npad(n_stft) * n_stft;
}

extern "C" int avid_logspec_basis(int n_stft, float* basis, avid_stream_t stream) {
  AVID_REQUIRE(n_stft >= 64 && n_stft % 32 == 0 && basis, AVID_E_BADARG, "logspec_basis: n_stft must be a multiple of 32");
  const int Npad = logspec_npad(n_stft);
  const long long tot = (long long)Npad * n_stft;
  hipLaunchKernelGGL(logspec_basis_kernel, dim3((unsigned)ceil_div(tot, 256)), dim3(256), 0, (hipStream_t)stream, basis, n_stft,
                     n_stft / 2 + 1, Npad);
  return check_launch("logspec_basis");
}

extern "C" size_t avid_logspec_workspace_bytes(int B, int n_stft, int T) {
  if (B <= 0 || T <= 0 || n_stft < 64) return 0;
  const size_t rows = (size_t)B * T;
  return sizeof(float) * rows * ((size_t)n_stft + logspec_npad(n_stft)) + sizeof(int) * (((size_t)B + 63) / 64 * 64);
}

extern "C" int avid_logspec(int B, int L, const float* sig, int n_stft, int hop, int T, const float* basis,
                            const float* mean, const float* stdv, float top_db, float* out, void* ws, size_t ws_bytes,
                            avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && L > n_stft / 2 && hop > 0 && T > 0 && sig && basis && out && ws, AVID_E_BADARG,
               "logspec: bad argument");
  AVID_REQUIRE(n_stft >= 64 && n_stft % 64 == 0, AVID_E_UNSUPPORTED, "logspec: the STFT size must be a multiple of 64");
  AVID_REQUIRE(T <= 1 + L / hop, AVID_E_SHAPE, "logspec: %d frames requested, the signal has %d", T, 1 + L / hop);
  AVID_REQUIRE((mean == nullptr) == (stdv == nullptr), AVID_E_BADARG, "logspec: mean and std go together");
  AVID_REQUIRE(ws_bytes >= avid_logspec_workspace_bytes(B, n_stft, T), AVID_E_BADARG, "logspec: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int F = n_stft / 2 + 1, Fo = n_stft / 4 + 1, Npad = logspec_npad(n_stft);
  const long long rows = (long long)B * T;
  float* A = static_cast<float*>(ws);
  float* Cm = A + rows * n_stft;
  int* mx = reinterpret_cast<int*>(Cm + rows * Npad);
  {
    ScopedTimer t(s, "logspec_frames_kernel", 0.0, 4.0 * rows * n_stft);
    hipLaunchKernelGGL(logspec_frames_kernel, dim3((unsigned)ceil_div(rows * n_stft, 256)), dim3(256), 0, s, sig, A, B, L,
                       n_stft, hop, T);
  }
  int rc = check_launch("logspec_frames");
  if (rc) return rc;
  rc = sim_gemm_nt(A, basis, Cm, nullptr, 0, rows, Npad, n_stft, s);
  if (rc) return rc;
  hipLaunchKernelGGL(logspec_init_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, s, mx, B);
  const long long no = rows * Fo;
  {
    ScopedTimer t(s, "logspec_db_kernel", 0.0, 4.0 * rows * (2.0 * F + Fo));
    hipLaunchKernelGGL(logspec_db_kernel, dim3((unsigned)ceil_div(no, 256)), dim3(256), 0, s, Cm, out, mx, B, T, F, Fo, Npad);
  }
  hipLaunchKernelGGL(logspec_finish_kernel, dim3((unsigned)ceil_div(no, 256)), dim3(256), 0, s, out, mx, mean, stdv, B, T, Fo,
                     top_db);
  return check_launch("logspec");
}

// ---- from int16 clips -------------------------------------------------------------------------------------------------------
static size_t pcm_table_bytes(int B) { return (sizeof(PcmDev) * (size_t)B + 15) / 16 * 16; }

static int validate_pcm(const char* what, int B, const avid_pcm_desc* descs) {
  AVID_REQUIRE(descs, AVID_E_BADARG, "%s: null descriptors", what);
  for (int b = 0; b < B; ++b) {
    const avid_pcm_desc& d = descs[b];
    AVID_REQUIRE(d.channels >= 1 && d.channels <= 8, AVID_E_UNSUPPORTED, "%s: clip %d: %d channels (1 to 8)", what, b, d.channels);
    AVID_REQUIRE(d.n >= 0, AVID_E_SHAPE, "%s: clip %d: negative length %d", what, b, d.n);
    AVID_REQUIRE(d.n == 0 || d.samples, AVID_E_BADARG, "%s: clip %d: null samples pointer with %d samples", what, b, d.n);
    AVID_REQUIRE(((uintptr_t)d.samples & 1) == 0, AVID_E_BADARG, "%s: clip %d: samples pointer is not 2-byte aligned", what, b);
    AVID_REQUIRE(d.gain - d.gain == 0.f, AVID_E_BADARG, "%s: clip %d: gain is not finite", what, b);
  }
  return AVID_OK;
}

// the descriptor table into `table` (device, pcm_table_bytes(B)) on the stream; *src_bytes: int16 bytes the clips hold
static int stage_pcm(const char* what, int B, const avid_pcm_desc* descs, void* table, hipStream_t s, double* src_bytes) {
  std::lock_guard<std::mutex> lock(g_stage_mu);
  Stage* st = take_stage(sizeof(PcmDev) * (size_t)B);
  AVID_REQUIRE(st, AVID_E_HIP, "%s: pinned staging allocation failed", what);
  PcmDev* pd = static_cast<PcmDev*>(st->host);
  *src_bytes = 0;
  for (int b = 0; b < B; ++b) {
    pd[b] = PcmDev{descs[b].samples, descs[b].channels, descs[b].n, descs[b].gain};
    *src_bytes += 2.0 * descs[b].channels * descs[b].n;
  }
  hipError_t e = hipMemcpyAsync(table, st->host, sizeof(PcmDev) * (size_t)B, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(st->done, s);
  st->used = true;
  if (e != hipSuccess) {
    set_error("%s: staging the descriptors: %s", what, hipGetErrorString(e));
    return AVID_E_HIP;
  }
  return AVID_OK;
}

extern "C" size_t avid_audio_prep_workspace_bytes(int B) { return B > 0 ? pcm_table_bytes(B) : 0; }

extern "C" int avid_audio_prep(int B, const avid_pcm_desc* descs, int L, float* out, void* ws, size_t ws_bytes,
                               avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && L > 0 && out && ws, AVID_E_BADARG, "audio_prep: bad argument");
  int rc = validate_pcm("audio_prep", B, descs);
  if (rc) return rc;
  AVID_REQUIRE(ws_bytes >= avid_audio_prep_workspace_bytes(B), AVID_E_BADARG, "audio_prep: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  double src_bytes;
  rc = stage_pcm("audio_prep", B, descs, ws, s, &src_bytes);
  if (rc) return rc;
  const long long tot = (long long)B * L;
  {
    ScopedTimer t(s, "audio_prep_kernel", 0.0, src_bytes + 4.0 * tot);
    hipLaunchKernelGGL(audio_prep_kernel, dim3((unsigned)ceil_div(tot, 256)), dim3(256), 0, s, static_cast<const PcmDev*>(ws), out,
                       B, L);
  }
  return check_launch("audio_prep");
}

extern "C" size_t avid_logspec_pcm_workspace_bytes(int B, int n_stft, int T) {
  const size_t base = avid_logspec_workspace_bytes(B, n_stft, T);
  return base ? (base + 15) / 16 * 16 + pcm_table_bytes(B) : 0;
}

extern "C" int avid_logspec_pcm(int B, const avid_pcm_desc* descs, int L, int n_stft, int hop, int T, const float* basis,
                                const float* mean, const float* stdv, float top_db, float* out, void* ws, size_t ws_bytes,
                                avid_stream_t stream) {
  AVID_REQUIRE(B > 0 && L > n_stft / 2 && hop > 0 && T > 0 && basis && out && ws, AVID_E_BADARG, "logspec_pcm: bad argument");
  AVID_REQUIRE(n_stft >= 64 && n_stft % 64 == 0, AVID_E_UNSUPPORTED, "logspec_pcm: the STFT size must be a multiple of 64");
  AVID_REQUIRE(T <= 1 + L / hop, AVID_E_SHAPE, "logspec_pcm: %d frames requested, the signal has %d", T, 1 + L / hop);
  AVID_REQUIRE((mean == nullptr) == (stdv == nullptr), AVID_E_BADARG, "logspec_pcm: mean and std go together");
  int rc = validate_pcm("logspec_pcm", B, descs);
  if (rc) return rc;
  AVID_REQUIRE(ws_bytes >= avid_logspec_pcm_workspace_bytes(B, n_stft, T), AVID_E_BADARG, "logspec_pcm: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int F = n_stft / 2 + 1, Fo = n_stft / 4 + 1, Npad = logspec_npad(n_stft);
  const long long rows = (long long)B * T;
  float* A = static_cast<float*>(ws);
  float* Cm = A + rows * n_stft;
  int* mx = reinterpret_cast<int*>(Cm + rows * Npad);
  PcmDev* table = reinterpret_cast<PcmDev*>(static_cast<char*>(ws) + (avid_logspec_workspace_bytes(B, n_stft, T) + 15) / 16 * 16);
  double src_bytes;
  rc = stage_pcm("logspec_pcm", B, descs, table, s, &src_bytes);
  if (rc) return rc;
  {
    ScopedTimer t(s, "logspec_frames_pcm_kernel", 0.0, src_bytes + 4.0 * rows * n_stft);
    hipLaunchKernelGGL(logspec_frames_pcm_kernel, dim3((unsigned)ceil_div(rows * n_stft, 256)), dim3(256), 0, s, table, A, B, L,
                       n_stft, hop, T);
  }
  rc = check_launch("logspec_frames_pcm");
  if (rc) return rc;
  rc = sim_gemm_nt(A, basis, Cm, nullptr, 0, rows, Npad, n_stft, s);
  if (rc) return rc;
  hipLaunchKernelGGL(logspec_init_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, s, mx, B);
  const long long no = rows * Fo;
  {
    ScopedTimer t(s, "logspec_db_kernel", 0.0, 4.0 * rows * (2.0 * F + Fo));
    hipLaunchKernelGGL(logspec_db_kernel, dim3((unsigned)ceil_div(no, 256)), dim3(256), 0, s, Cm, out, mx, B, T, F, Fo, Npad);
  }
  hipLaunchKernelGGL(logspec_finish_kernel, dim3((unsigned)ceil_div(no, 256)), dim3(256), 0, s, out, mx, mean, stdv, B, T, Fo,
                     top_db);
  return check_launch("logspec_pcm");
}
