// Clip augmentation on the GPU: the part of the reference's video preprocessing that ran per frame in PIL inside the DataLoader
// workers (datasets/preprocessing.py:15-113 -> utils/videotransforms/video_transforms.py: RandomResizedCrop / Resize +
// CenterCrop / RandomCrop, RandomHorizontalFlip, ColorJitter), fused with the ClipToTensor + Normalize tail of clipprep.hip.
// Every step is integer or short float arithmetic and is reproduced bit for bit (tests/_augment_ref.py is the numpy
// restatement, pinned against Pillow itself; tests/test_gpu_augment.py holds this file to it with torch.equal).
//
//   clip_augment_kernel   one workgroup = one 8 x 32 tile of one output frame.  Pillow resamples in two passes and rounds
//                         the horizontal result to uint8 before the vertical pass: the workgroup computes the horizontal
//                         pass for the source rows its tile needs, 32 rows at a time, into LDS (one packed RGB word per
//                         pixel) and accumulates the vertical taps from there, so the intermediate never reaches HBM and
//                         any scale fits (the row loop is as long as the scale asks).  Then flip, the colour operations up
//                         to (not including) contrast, and either the normalised fp32 output or, for a clip that uses
//                         contrast, a uint8 intermediate + the frame's integer grey sum (one 32-bit vector atomic per wave:
//                         exact and order independent; 255 * ch * cw fits).
//   clip_contrast_kernel  clips with contrast only: blend with the frame's rounded mean grey, the operations after it,
//                         normalise.
// The coefficient tables are Pillow's (precompute_coeffs + normalize_coeffs_8bpc: double, sequential normalising sum, 22
// fraction bits), built on the host for the window's rows and columns only; a pass Pillow skips (size unchanged) is the
// identity table (one tap of 2^22), which rounds to the source byte exactly.
//
// Pillow is built without floating-point contraction and hipcc contracts by default: a fused multiply-add in blend() or in
// the HSV arithmetic changes results (tests: every factor outside the exactly representable ones catches it).
#include <math.h>

#include <mutex>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

namespace avid {

constexpr int AUG_TH = 8, AUG_TW = 32, AUG_ROWS = 32;   // output tile, source rows staged per round
constexpr int AUG_BITS = 22;

struct ClipDev {
  const uint8_t* src;
  long long inter_off;   // byte offset of this clip's intermediate (one RGB word per pixel), -1: no contrast
  int T, H, W, i, j, flip;
  int hoff, hstride, voff, vstride;   // tables (in ints): per output column / row {first tap, taps, coefficients...}
  int nops, cpos;                     // cpos: index of contrast in ops, -1 without
  int ops[4];
  float f[4];
  int shift;                          // hue: the uint8 added to H
  int pad;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int grey8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// Image.blend(degenerate d, image a, f) for one channel
__device__ __forceinline__ int blend8(int d, int a, float f) {
  const float t = (float)d + f * (float)(a - d);
  if (f >= 0.f && f <= 1.f) return (int)t & 255;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int round8(double x) { return clip8((int)floor(x + 0.5)); }

// convert("HSV"), H += shift (mod 256), convert("RGB"): Pillow's rgb2hsv_row / hsv2rgb_row, double where C promotes to double
__device__ __forceinline__ void hue_op(int shift, int& r, int& g, int& b) {
  const int maxc = max(max(r, g), b), minc = min(min(r, g), b);
  int H = 0, S = 0;
  const int V = maxc;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    double hd = (double)h / 6.0 + 1.0;        // in [5/6, 11/6): fmod(., 1) = . - floor(.)
    hd = hd - floor(hd);
    h = (float)hd;
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const float fs = (float)((double)S / 255.0);
  const double hf = (double)H * 6.0 / 255.0;
  const double fi = floor(hf);
  const float f = (float)(hf - fi);
  const double v = (double)V;
  const int p = round8(v * (1.0 - (double)fs));
  const int q = round8(v * (1.0 - (double)(fs * f)));
  const int t = round8(v * (1.0 - (double)fs * (1.0 - (double)f)));
  switch ((int)fi % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// operations [first, last) of the clip, contrast excluded (the callers place it)
__device__ __forceinline__ void colour_ops(const ClipDev& c, int first, int last, int& r, int& g, int& b) {
  for (int k = first; k < last; ++k) {
    const int op = c.ops[k];
    const float f = c.f[k];
    if (op == AVID_AUG_BRIGHTNESS) {
      r = blend8(0, r, f); g = blend8(0, g, f); b = blend8(0, b, f);
    } else if (op == AVID_AUG_SATURATION) {
      const int d = grey8(r, g, b);
      r = blend8(d, r, f); g = blend8(d, g, f); b = blend8(d, b, f);
    } else if (op == AVID_AUG_HUE) {
      hue_op(c.shift, r, g, b);
    }
  }
}

struct NormArgs { float m0, m1, m2, s0, s1, s2; };

__device__ __forceinline__ void store_normalized(float* __restrict__ o, long long plane, int r, int g, int b, const NormArgs& n) {
  o[0] = ((float)r / 255.f - n.m0) / n.s0;
  o[plane] = ((float)g / 255.f - n.m1) / n.s1;
  o[2 * plane] = ((float)b / 255.f - n.m2) / n.s2;
}

__global__ __launch_bounds__(256) void clip_augment_kernel(const ClipDev* __restrict__ clips, const int* __restrict__ tabs,
                                                           uint8_t* __restrict__ inter, unsigned* __restrict__ sums,
                                                           float* __restrict__ out, int nf, int ch, int cw, int tiles_x,
                                                           NormArgs nrm) {
  __shared__ unsigned hrow[AUG_ROWS][AUG_TW];
  const int b = blockIdx.z, t = blockIdx.y;
  const ClipDev& c = clips[b];
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int tid = threadIdx.x, ty = tid / AUG_TW, tx = tid % AUG_TW;
  const int oy = tile_y * AUG_TH + ty, xs = tile_x * AUG_TW + tx;   // xs: column of the resampled window (before the flip)
  const bool valid = oy < ch && xs < cw;
  const uint8_t* frame = c.src + (long long)(t % c.T) * c.H * c.W * 3;

  const int row0 = tile_y * AUG_TH, rowl = min(row0 + AUG_TH, ch) - 1;
  const int* v0 = tabs + c.voff + (long long)row0 * c.vstride;
  const int* vl = tabs + c.voff + (long long)rowl * c.vstride;
  const int ylo = v0[0], yhi = vl[0] + vl[1];      // Pillow's bounds never decrease along an axis
  const int* vk = tabs + c.voff + (long long)(valid ? oy : row0) * c.vstride;
  const int ymin = vk[0], ycnt = vk[1];

  int ar = 1 << (AUG_BITS - 1), ag = ar, ab = ar;
  for (int y0 = ylo; y0 < yhi; y0 += AUG_ROWS) {
    const int nr = min(AUG_ROWS, yhi - y0);
    for (int it = tid; it < nr * AUG_TW; it += 256) {
      const int rr = it / AUG_TW, cx = it % AUG_TW, col = tile_x * AUG_TW + cx;
      if (col < cw) {
        const int* hk = tabs + c.hoff + (long long)col * c.hstride;
        const int xmin = hk[0], cnt = hk[1];
        const uint8_t* p = frame + ((long long)(c.i + y0 + rr) * c.W + c.j + xmin) * 3;
        int s0 = 1 << (AUG_BITS - 1), s1 = s0, s2 = s0;
        for (int k = 0; k < cnt; ++k) {
          const int w = hk[2 + k];
          s0 += (int)p[3 * k] * w;
          s1 += (int)p[3 * k + 1] * w;
          s2 += (int)p[3 * k + 2] * w;
        }
        hrow[rr][cx] = (unsigned)clip8(s0 >> AUG_BITS) | ((unsigned)clip8(s1 >> AUG_BITS) << 8) |
                       ((unsigned)clip8(s2 >> AUG_BITS) << 16);
      }
    }
    __syncthreads();
    if (valid) {
      const int ya = max(ymin, y0), yb = min(ymin + ycnt, y0 + nr);
      for (int yy = ya; yy < yb; ++yy) {
        const int w = vk[2 + yy - ymin];
        const unsigned px = hrow[yy - y0][tx];
        ar += (int)(px & 255u) * w;
        ag += (int)((px >> 8) & 255u) * w;
        ab += (int)((px >> 16) & 255u) * w;
      }
    }
    __syncthreads();
  }
  int r = clip8(ar >> AUG_BITS), g = clip8(ag >> AUG_BITS), bl = clip8(ab >> AUG_BITS);
  const int ox = c.flip ? cw - 1 - xs : xs;
  const long long plane = (long long)nf * ch * cw;
  if (c.cpos < 0) {
    if (valid) {
      colour_ops(c, 0, c.nops, r, g, bl);
      store_normalized(out + (long long)b * 3 * plane + ((long long)t * ch + oy) * cw + ox, plane, r, g, bl, nrm);
    }
    return;
  }
  int gsum = 0;
  if (valid) {
    colour_ops(c, 0, c.cpos, r, g, bl);
    // one packed word per pixel: a coalesced 32-bit store here and load in clip_contrast_kernel
    *reinterpret_cast<unsigned*>(inter + c.inter_off + (((long long)t * ch + oy) * cw + ox) * 4) =
        (unsigned)r | ((unsigned)g << 8) | ((unsigned)bl << 16);
    gsum = grey8(r, g, bl);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o, 64);
  if ((tid & 63) == 0 && gsum) atomicAdd(&sums[b * nf + t], (unsigned)gsum);
}

__global__ __launch_bounds__(256) void clip_contrast_kernel(const ClipDev* __restrict__ clips, const uint8_t* __restrict__ inter,
                                                            const unsigned* __restrict__ sums, float* __restrict__ out,
                                                            int nf, int ch, int cw, NormArgs nrm) {
  const int b = blockIdx.z, t = blockIdx.y;
  const ClipDev& c = clips[b];
  if (c.cpos < 0) return;
  const int npix = ch * cw;
  const int mean = (int)((double)sums[b * nf + t] / (double)npix + 0.5);
  const float fc = c.f[c.cpos];
  const long long plane = (long long)nf * npix;
  const unsigned* src = reinterpret_cast<const unsigned*>(inter + c.inter_off) + (long long)t * npix;
  float* o = out + (long long)b * 3 * plane + (long long)t * npix;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    const unsigned px = src[i];
    int r = blend8(mean, px & 255u, fc), g = blend8(mean, (px >> 8) & 255u, fc), bl = blend8(mean, (px >> 16) & 255u, fc);
    colour_ops(c, c.cpos + 1, c.nops, r, g, bl);
    store_normalized(o + i, plane, r, g, bl, nrm);
  }
}

// ---- host: Pillow's coefficient tables -----------------------------------------------------------------------------------
struct AxisTab {
  int stride = 0;            // 2 + the largest tap count of the rows kept
  std::vector<int> rows;     // [n][stride]
};

// rows first .. first + n - 1 of the `in` -> `out` bilinear table (ImagingResample: precompute_coeffs, normalize_coeffs_8bpc)
static void axis_table(int in, int out, int first, int n, AxisTab& tab, std::vector<double>& tmp) {
  if (in == out) {           // Pillow skips the pass
    tab.stride = 3;
    tab.rows.resize((size_t)n * 3);
    for (int r = 0; r < n; ++r) {
      tab.rows[3 * r] = first + r;
      tab.rows[3 * r + 1] = 1;
      tab.rows[3 * r + 2] = 1 << AUG_BITS;
    }
    return;
  }
  const double scale = (double)in / (double)out;
  const double fscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / fscale;
  tab.stride = 2 + ksize;
  tab.rows.assign((size_t)n * tab.stride, 0);
  tmp.resize(ksize);
  int most = 1;
  for (int r = 0; r < n; ++r) {
    const int xx = first + r;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      const double w = a < 1.0 ? 1.0 - a : 0.0;
      tmp[x] = w;
      ww += w;
    }
    int* row = &tab.rows[(size_t)r * tab.stride];
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
      const double w = ww != 0.0 ? tmp[x] / ww : tmp[x];
      row[2 + x] = w < 0 ? (int)(-0.5 + w * (1 << AUG_BITS)) : (int)(0.5 + w * (1 << AUG_BITS));
    }
    if (xmax > most) most = xmax;
  }
  if (2 + most < tab.stride) {      // keep only the taps some row uses
    const int ns = 2 + most;
    for (int r = 0; r < n; ++r)
      for (int k = 0; k < ns; ++k) tab.rows[(size_t)r * ns + k] = tab.rows[(size_t)r * tab.stride + k];
    tab.stride = ns;
    tab.rows.resize((size_t)n * ns);
  }
}

static int table_stride(int in, int out) {     // an upper bound of axis_table's stride that needs no table
  if (in == out) return 3;
  const double scale = (double)in / (double)out;
  return 2 + (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

static int validate(int B, const avid_aug_desc* descs, int nf, int ch, int cw) {
  AVID_REQUIRE(descs, AVID_E_BADARG, "clip_augment: null descriptors");
  AVID_REQUIRE(B > 0 && B <= 65535 && nf > 0 && nf <= 65535 && ch > 0 && cw > 0 && (long long)ch * cw <= (1 << 24),
               AVID_E_SHAPE, "clip_augment: bad shape (B %d, num_frames %d, output %d x %d)", B, nf, ch, cw);
  for (int b = 0; b < B; ++b) {
    const avid_aug_desc& d = descs[b];
    AVID_REQUIRE(d.frames, AVID_E_BADARG, "clip_augment: clip %d: null frames pointer", b);
    AVID_REQUIRE(d.T > 0 && d.H > 0 && d.W > 0, AVID_E_SHAPE, "clip_augment: clip %d: bad source shape %d x %d x %d", b, d.T,
                 d.H, d.W);
    AVID_REQUIRE(d.i >= 0 && d.j >= 0 && d.h > 0 && d.w > 0 && (long long)d.i + d.h <= d.H && (long long)d.j + d.w <= d.W,
                 AVID_E_BADARG, "clip_augment: clip %d: crop box (%d, %d, %d, %d) outside the %d x %d frame", b, d.i, d.j,
                 d.h, d.w, d.H, d.W);
    AVID_REQUIRE(d.RH > 0 && d.RW > 0 && d.y1 >= 0 && d.x1 >= 0 && (long long)d.y1 + ch <= d.RH &&
                     (long long)d.x1 + cw <= d.RW,
                 AVID_E_BADARG, "clip_augment: clip %d: window (%d, %d, %d, %d) outside the resampled %d x %d image", b, d.y1,
                 d.x1, ch, cw, d.RH, d.RW);
    AVID_REQUIRE(d.nops >= 0 && d.nops <= 4, AVID_E_BADARG, "clip_augment: clip %d: %d colour operations (at most 4)", b,
                 d.nops);
    int contrasts = 0;
    for (int k = 0; k < d.nops; ++k) {
      AVID_REQUIRE(d.ops[k] >= AVID_AUG_BRIGHTNESS && d.ops[k] <= AVID_AUG_CONTRAST, AVID_E_BADARG,
                   "clip_augment: clip %d: unknown colour operation %d", b, d.ops[k]);
      AVID_REQUIRE(d.factor[k] == d.factor[k], AVID_E_BADARG, "clip_augment: clip %d: factor %d is not a number", b, k);
      if (d.ops[k] == AVID_AUG_HUE)
        AVID_REQUIRE(d.factor[k] >= -0.5 && d.factor[k] <= 0.5, AVID_E_BADARG,
                     "clip_augment: clip %d: hue factor %g outside [-0.5, 0.5]", b, d.factor[k]);
      contrasts += d.ops[k] == AVID_AUG_CONTRAST;
    }
    AVID_REQUIRE(contrasts <= 1, AVID_E_UNSUPPORTED, "clip_augment: clip %d: contrast more than once", b);
  }
  return AVID_OK;
}

struct AugLayout {
  size_t clips, tabs, sums, inter, total;   // byte offsets; [clips, sums) is what the host stages
};

static bool uses_contrast(const avid_aug_desc& d) {
  for (int k = 0; k < d.nops; ++k)
    if (d.ops[k] == AVID_AUG_CONTRAST) return true;
  return false;
}

static AugLayout layout(int B, const avid_aug_desc* descs, int nf, int ch, int cw) {
  AugLayout L;
  size_t ints = 0, inter = 0;
  for (int b = 0; b < B; ++b) {
    ints += (size_t)cw * table_stride(descs[b].w, descs[b].RW) + (size_t)ch * table_stride(descs[b].h, descs[b].RH);
    if (uses_contrast(descs[b])) inter += ((size_t)nf * ch * cw * 4 + 15) / 16 * 16;
  }
  L.clips = 0;
  L.tabs = (sizeof(ClipDev) * B + 15) / 16 * 16;
  L.sums = (L.tabs + ints * 4 + 15) / 16 * 16;
  L.inter = (L.sums + (size_t)B * nf * 4 + 15) / 16 * 16;
  L.total = L.inter + inter;
  return L;
}

}  // namespace avid

using namespace avid;

extern "C" size_t avid_clip_augment_workspace_bytes(int B, const avid_aug_desc* descs, int num_frames, int ch, int cw) {
  if (validate(B, descs, num_frames, ch, cw) != AVID_OK) return 0;
  return layout(B, descs, num_frames, ch, cw).total;
}

extern "C" int avid_clip_augment(int B, const avid_aug_desc* descs, int num_frames, int ch, int cw, const float* mean3,
                                 const float* std3, float* out, void* ws, size_t ws_bytes, avid_stream_t stream) {
  const int rc = validate(B, descs, num_frames, ch, cw);
  if (rc != AVID_OK) return rc;
  AVID_REQUIRE(mean3 && std3 && out && ws, AVID_E_BADARG, "clip_augment: null pointer");
  AVID_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, AVID_E_BADARG, "clip_augment: zero std");
  const AugLayout L = layout(B, descs, num_frames, ch, cw);
  AVID_REQUIRE(ws_bytes >= L.total, AVID_E_BADARG, "clip_augment: workspace too small (%zu < %zu)", ws_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;

  std::lock_guard<std::mutex> lock(g_stage_mu);
  Stage* st = take_stage(L.sums);
  AVID_REQUIRE(st, AVID_E_HIP, "clip_augment: pinned staging allocation failed");
  ClipDev* cd = reinterpret_cast<ClipDev*>(st->host);
  int* tabs = reinterpret_cast<int*>(static_cast<char*>(st->host) + L.tabs);
  size_t at = 0, inter = 0;
  bool any_contrast = false;
  double src_bytes = 0;
  AxisTab tab;
  std::vector<double> tmp;
  for (int b = 0; b < B; ++b) {
    const avid_aug_desc& d = descs[b];
    ClipDev& c = cd[b];
    memset(&c, 0, sizeof(c));
    c.src = d.frames;
    c.T = d.T; c.H = d.H; c.W = d.W; c.i = d.i; c.j = d.j; c.flip = d.flip ? 1 : 0;
    axis_table(d.w, d.RW, d.x1, cw, tab, tmp);
    c.hoff = (int)at; c.hstride = tab.stride;
    memcpy(tabs + at, tab.rows.data(), tab.rows.size() * sizeof(int));
    at += tab.rows.size();
    axis_table(d.h, d.RH, d.y1, ch, tab, tmp);
    c.voff = (int)at; c.vstride = tab.stride;
    memcpy(tabs + at, tab.rows.data(), tab.rows.size() * sizeof(int));
    at += tab.rows.size();
    c.nops = d.nops;
    c.cpos = -1;
    c.inter_off = -1;
    for (int k = 0; k < d.nops; ++k) {
      c.ops[k] = d.ops[k];
      c.f[k] = (float)d.factor[k];
      if (d.ops[k] == AVID_AUG_CONTRAST) c.cpos = k;
      if (d.ops[k] == AVID_AUG_HUE) c.shift = (int)(d.factor[k] * 255.0) & 255;   // truncation toward zero, modulo 256
    }
    if (c.cpos >= 0) {
      c.inter_off = (long long)inter;
      inter += ((size_t)num_frames * ch * cw * 4 + 15) / 16 * 16;
      any_contrast = true;
    }
    src_bytes += 3.0 * num_frames * d.h * d.w * ((double)ch / d.RH) * ((double)cw / d.RW);
  }
  char* wsb = static_cast<char*>(ws);
  hipError_t e = hipMemcpyAsync(wsb, st->host, L.tabs + at * sizeof(int), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(st->done, s);
  st->used = true;
  if (e == hipSuccess && any_contrast) e = hipMemsetAsync(wsb + L.sums, 0, (size_t)B * num_frames * 4, s);
  if (e != hipSuccess) {
    set_error("clip_augment: staging the tables: %s", hipGetErrorString(e));
    return AVID_E_HIP;
  }
  const NormArgs nrm{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
  const double out_px = (double)B * num_frames * ch * cw;
  const int tiles_x = (int)ceil_div(cw, AUG_TW), tiles_y = (int)ceil_div(ch, AUG_TH);
  {
    ScopedTimer t(s, "clip_augment_kernel", 0.0, src_bytes + 12.0 * out_px);
    hipLaunchKernelGGL(clip_augment_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)num_frames, (unsigned)B), dim3(256),
                       0, s, reinterpret_cast<const ClipDev*>(wsb), reinterpret_cast<const int*>(wsb + L.tabs),
                       reinterpret_cast<uint8_t*>(wsb + L.inter), reinterpret_cast<unsigned*>(wsb + L.sums), out, num_frames,
                       ch, cw, tiles_x, nrm);
  }
  if (any_contrast) {
    ScopedTimer t(s, "clip_contrast_kernel", 0.0, 16.0 * out_px);
    long long gx = ceil_div((long long)ch * cw, 256);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(clip_contrast_kernel, dim3((unsigned)gx, (unsigned)num_frames, (unsigned)B), dim3(256), 0, s,
                       reinterpret_cast<const ClipDev*>(wsb), reinterpret_cast<const uint8_t*>(wsb + L.inter),
                       reinterpret_cast<const unsigned*>(wsb + L.sums), out, num_frames, ch, cw, nrm);
  }
  return check_launch("clip_augment");
}
