/*
 * avid_hip.h — C-ABI of libavid_hip.so: the MI355X (gfx950) kernels behind the AVID / AVID-CMA
 * training step.  Plain C types only; no torch / C++ types cross this boundary.
 *
 * The reference (facebookresearch/AVID-CMA) is pure Python and has no FFI of its own: every entry
 * point below replaces the ATen/cuDNN op that a reference line dispatches to.  Each declaration
 * cites that line (paths relative to the reference root).  The Python side that binds these symbols
 * with ctypes lives in avid-cma_amd/avid_hip/lib.py; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - All device pointers are fp32 unless stated; indices are int64 (reference: default collate of
 *     Python ints, datasets/video_db.py:263) except positive_set (int32, criterions/avid_cma.py:223).
 *   - Activations are channels-last: [B, T, H, W, C] (2-D audio uses T = 1).  Conv weights are
 *     [Cout][kt][kh][kw][Cin] — the memory of a torch tensor of logical shape [Cout,Cin,kt,kh,kw]
 *     held in torch.channels_last_3d format, so state_dict keys *and shapes* equal the reference's.
 *   - The stem convs read the reference's NCDHW / NCHW input directly (x_channel_first = 1).
 *   - Every call is asynchronous on `stream` (a hipStream_t); nothing here synchronises the host.
 *   - The library never allocates persistent device memory: scratch is passed in by the caller
 *     (sizes from the *_workspace_bytes queries); torch owns every buffer.
 *   - Return value: 0 = AVID_OK, negative = error; avid_last_error() gives the message
 *     (thread-local).  Kernels never abort.
 */
#ifndef AVID_HIP_H
#define AVID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVID_OK 0
#define AVID_E_BADARG (-1)
#define AVID_E_SHAPE (-2)
#define AVID_E_HIP (-3)
#define AVID_E_UNSUPPORTED (-4)

typedef void* avid_stream_t; /* hipStream_t */

const char* avid_last_error(void);
int avid_version(void);
/* CU count / LDS per CU / arch name of `device` ("gfx950" expected). */
int avid_device_info(int device, int* cu_count, int* lds_bytes, char* arch, int arch_len);

/* Per-kernel timing with HIP events recorded on the launch stream.  enable(1) clears old records and
 * starts bracketing every hot kernel launch with two events; report() synchronises them and writes
 * one line per kernel: "name;launches;total_ms;algorithmic_flops;algorithmic_bytes\n". */
int avid_timing_enable(int on);
int avid_timing_report(char* buf, size_t len);

/* ------------------------------------------------------------------------------------------------
 * Convolution: fp32 in, fp32 out, fp32 accumulation, fp32-accurate products.  Which kernel a layer runs on is the library's
 * business (avid_conv_kernel_name tells): implicit GEMM, Winograd F(2x2,3x3) for the stride-1 3x3 layers, LDS-patch kernels for
 * the stems, a tap-sharing kernel for conv2x's (3,1,1) layers.  Since version 110 most of them assemble every fp32 product
 * from SIX bf16 matrix instructions (v_mfma_f32_32x32x16_bf16 on operands split into three bf16 terms: error against float64
 * at or below the fp32 instruction's, tests/test_gpu_precision.py; a non-finite input becomes NaN where the fp32 instruction
 * would keep an infinity); wino_kernel, wino_wgrad_kernel and the bias / ReLU epilogues of the linear layers issue the fp32
 * instruction v_mfma_f32_32x32x2_f32 itself.
 * Replaces nn.Conv3d / nn.Conv2d / nn.Linear forward+backward:
 *   models/video.py:20, models/network_blocks.py:18,20,35,37,40,42,49, models/audio.py:22,
 *   models/av_wrapper.py:25 (Linear == 1x1x1 conv over a [B,1,1,1,C] tensor).
 * ---------------------------------------------------------------------------------------------- */
typedef struct avid_conv_desc {
  int32_t B, Ti, Hi, Wi, Cin; /* input  [B,Ti,Hi,Wi,Cin] */
  int32_t To, Ho, Wo, Cout;   /* output [B,To,Ho,Wo,Cout] */
  int32_t kt, kh, kw;         /* kernel extent */
  int32_t st, sh, sw;         /* stride */
  int32_t pt, ph, pw;         /* zero padding */
  int32_t x_channel_first;    /* 1: x (and the dx of avid_conv_dgrad) is [B,Cin,Ti,Hi,Wi] (stems only; Cin in {1,3}) */
} avid_conv_desc;

/* y = conv(x, w) [+ addend] [+ bias] [relu].  addend: [B,To,Ho,Wo,Cout] or NULL (residual add of
 * models/network_blocks.py:59 fused into tmp_conv2/res_conv); bias: [Cout] or NULL.
 * ws: scratch for the split-K partial slabs of small-M layers (may be NULL: single pass, slower).
 * Large (1,3,3) stride-1 layers with <= 256 output channels run as a fused Winograd F(2x2,3x3) kernel (forward and
 * input gradient; csrc/wino.hip, AVID_WINO=0 to switch it off): same contract, results within 1e-6 of the direct
 * form; its transformed weights live in ws, so BatchNorm partials / the fused BatchNorm-backward sums of such a
 * layer need the planned workspace. */
size_t avid_conv_fwd_workspace_bytes(const avid_conv_desc* d);
/* bn_partials (or NULL): BatchNorm partial sums of the output y, [rows][2][Cout] with rows =
 * avid_conv_fwd_stats_rows(d) (0 = this layer cannot produce them), written by the conv epilogue so that
 * avid_bn_fwd_train can skip its statistics pass over y.  Needs bias == NULL and relu == 0. */
int avid_conv_fwd_stats_rows(const avid_conv_desc* d);
/* u (or NULL): for a layer on the Winograd path (v = avid_conv_uses_wino(d, 0) != 0), its weights already transformed by
 * avid_weight_transpose_batched (a descriptor of mode 1 if v == 1, mode 3 if v == 2; current for this w): the call then
 * skips its own transform launch.  For a layer with avid_conv_uses_split(d, 0) != 0 (version >= 120): its mode-5 table
 * (the weights pre-split into bf16 terms).  Ignored by every other layer. */
int avid_conv_fwd(const avid_conv_desc* d, const float* x, const float* w, const float* u, const float* addend,
                  const float* bias, int relu, float* y, float* bn_partials, void* ws, size_t ws_bytes,
                  avid_stream_t stream);

/* The same convolution reading the INPUT of a BatchNorm (+ReLU) instead of its output (version >= 130): x is the tensor the
 * BatchNorm normalises (the previous convolution's output), `in` its saved scale / shift ([Cin] each, avid_bn_fwd_train's
 * save_scale / save_shift) — the kernel applies fma(x, scale[c], shift[c]) (+ max(., 0) if relu) to every element it stages,
 * the expression of avid_bn_fwd_train's own apply pass, bit for bit; padding stays zero.  The normalised tensor is then never
 * written: avid_bn_fwd_train(y = NULL) makes the statistics only.  Replaces the `x = ReLU(bn(x))` round trip through memory
 * between models/network_blocks.py:36 / 41 and :37 / 42 (spt_bn1 -> tmp_conv1, spt_bn2 -> tmp_conv2).  in = NULL: avid_conv_fwd.
 * Only layers for which avid_conv_takes_in_affine() answers 1 (conv2x's temporal layers: tconv64_kernel / twgrad64_kernel, given
 * their pre-split weights as u); anything else returns AVID_E_UNSUPPORTED.  A layer that takes it must be given the same pair
 * in its weight gradient (avid_conv_wgrad_in); its input gradient does not read x. */
typedef struct avid_in_affine {
  const float* scale;
  const float* shift;
  int32_t relu;
} avid_in_affine;
int avid_conv_takes_in_affine(const avid_conv_desc* d);
int avid_conv_fwd_in(const avid_conv_desc* d, const float* x, const avid_in_affine* in, const float* w, const float* u,
                     const float* addend, const float* bias, int relu, float* y, float* bn_partials, void* ws, size_t ws_bytes,
                     avid_stream_t stream);
/* Launches of tconv64_kernel's forward / twgrad64_kernel since the library was loaded that read their input as it is
 * (fused = 0) or applied a BatchNorm to it while staging (fused = 1): tests assert which form ran. */
long long avid_debug_in_affine_launches(int fused);

/* Inference (version >= 160): the same convolution with the eval-mode BatchNorm (+ReLU) of its OUTPUT applied in the epilogue:
 * y = [max(., 0)](fma(conv(x) [+ addend], out->scale[c], out->shift[c])), scale / shift [Cout] from the running statistics
 * (avid_bn_eval_coeffs_batched, or avid_bn_fwd_eval's save4 rows 2 and 3).  Bit-identical to avid_conv_fwd[_in] followed by
 * avid_bn_fwd_eval(save4) with the same vectors: the same fma on the same fp32 value, the addend added in front of it as a
 * separate operation.  The un-normalised tensor is never written, so there are no BatchNorm partial sums of it: bn_partials
 * (and bias, relu) must be NULL / 0 when out is given.  `in` (nullable) as in avid_conv_fwd_in; out = NULL: avid_conv_fwd_in.
 * Only layers for which avid_conv_takes_out_affine() answers 1 (those whose forward runs on tconv64_kernel: (3,1,1), stride 1,
 * 64 -> 64 channels, 8 frames, given their pre-split weights as u); anything else returns AVID_E_UNSUPPORTED. */
typedef struct avid_out_affine {
  const float* scale;
  const float* shift;
  int32_t relu;
} avid_out_affine;
int avid_conv_takes_out_affine(const avid_conv_desc* d);
int avid_conv_fwd_out(const avid_conv_desc* d, const float* x, const avid_in_affine* in, const float* w, const float* u,
                      const float* addend, const float* bias, int relu, const avid_out_affine* out, float* y,
                      float* bn_partials, void* ws, size_t ws_bytes, avid_stream_t stream);
/* Launches of tconv64_kernel's forward since the library was loaded that applied a BatchNorm to their output. */
long long avid_debug_out_affine_launches(void);

/* dx = conv_transpose(dy, w) [+ addend].  ws: scratch for the transposed weights (+ split-K slabs).
 * wt (nullable): the weights already repacked as [Cin][taps][Cout] by avid_weight_transpose_batched (mode 0, current
 * for this w); NULL = repack inside the call (one extra small launch per layer).
 * u (nullable, version >= 110: its own argument): for a layer whose input gradient runs on the Winograd path
 * (v = avid_conv_uses_wino(d, 1) != 0) its mode-2 (v == 1) or mode-4 (v == 2) transform from
 * avid_weight_transpose_batched; NULL = transform inside the call.  Each pointer is read only by the path it belongs
 * to: a Winograd-eligible layer that falls through to the implicit GEMM (compact addend) reads wt, never u.
 * A layer with avid_conv_uses_split(d, 1) != 0 (version >= 120) takes its mode-6 table as u and then reads neither wt
 * nor the repack scratch.
 * x_channel_first = 1 (version >= 166): the input gradient of the two stems — Cin 3, kernel (3,7,7), padding (1,3,3) and
 * Cin 1, kernel (1,7,7), padding (0,3,3), both Cout 64 and stride (1,2,2), any input size.  dy is channels-last
 * [B,To,Ho,Wo,64], w the parameter's memory, dx channel-first [B,Cin,Ti,Hi,Wi] like the x the forward read
 * (stem_dgrad_kernel: plain fp32 multiply-adds in one fixed order per element — the same bits on every run and under
 * every CU budget).  wt, u, addend, addend_stride and bn must be NULL (AVID_E_BADARG otherwise); no workspace
 * (avid_conv_dgrad_workspace_bytes == 0, ws may be NULL) and avid_conv_dgrad_bn_rows == 0.  Any other channel-first
 * geometry: AVID_E_UNSUPPORTED before anything is launched.
 * What avid_conv_dgrad_workspace_bytes contains: the transposed weights (Cout * taps * Cin floats, rounded up to 256 bytes)
 * + the K-split slabs of the kernel the layer runs on — for a strided layer on the persistent kernel up to 8 dx-shaped slabs
 * of its K-split parity classes.  A strided layer whose dx has 2^31 bytes or more does not run on the persistent kernel
 * (igemm_kernel<..,1>s2 splits nothing): since version 172 the answer for it is the transposed weights alone. */
size_t avid_conv_dgrad_workspace_bytes(const avid_conv_desc* d);
/* bn (or NULL): dx is the COMPLETE gradient of the output of a training-mode BatchNorm(+ReLU) whose input was
 * bn->x (shape of dx) — the usual conv <- ReLU <- BN chain of models/network_blocks.py:30-60.  The dgrad epilogue
 * then also writes that BatchNorm's backward partial sums ([rows][2][Cin]: sum dy_m, sum dy_m * xhat with dy_m the
 * gradient masked by the recomputed ReLU; rows = avid_conv_dgrad_bn_rows(d), 0 = this layer cannot), which
 * avid_bn_bwd takes instead of making its own pass over dy and x.  scale / shift / mean / invstd: the tensors
 * avid_bn_fwd_train saved. */
typedef struct {
  const float* x;
  const float* scale;
  const float* shift;
  const float* mean;
  const float* invstd;
  int32_t relu;
  float* partials;
} avid_bn_bwd_fuse;
int avid_conv_dgrad_bn_rows(const avid_conv_desc* d);
/* addend_stride (nullable = {1,1,1}): strides (1 or 2 per axis) of a COMPACT addend — the gradient of the
 * sub-sampled view x[:, ::st, ::sh, ::sw] that a block's 1x1x1 strided residual convolution reads
 * (models/network_blocks.py:47-51,58), shape [B][ceil(Ti/st)][ceil(Hi/sh)][ceil(Wi/sw)][Cin]: it is added at the
 * positions divisible by the strides only, instead of being scattered into a dx-shaped tensor of mostly zeros
 * first.  Strided layers on the persistent kernel only. */
int avid_conv_dgrad(const avid_conv_desc* d, const float* dy, const float* w, const float* wt, const float* u,
                    const float* addend, const int32_t* addend_stride, float* dx, const avid_bn_bwd_fuse* bn,
                    void* ws, size_t ws_bytes, avid_stream_t stream);

/* One launch that repacks every conv / linear weight of a model for its input-gradient pass:
 * w[Cout][taps][Cin] -> wt[Cin][taps][Cout] for each descriptor.  descs_dev: n descriptors in DEVICE
 * memory (they do not change between steps); max_elems = max over descriptors of Cout*taps*Cin.
 * Call it once after each optimizer step (the autograd.Function of torch's conv does this per call). */
typedef struct avid_wt_desc {
  const float* w;
  float* wt;
  int32_t Cout, ntaps, Cin;
  int32_t mode; /* 0: wt[Cin][taps][Cout]; 3x3 layers on the Winograd path (ntaps = 9): wt = the 16 x Cout x Cin transformed
                   weights U in the operand-fragment order (and element format: fp32, or three bf16 terms) of the kernel that
                   will read them, a buffer of 96 * Cout * Cin bytes whatever the format — 1 / 3: for the forward
                   (pass it as `u` to avid_conv_fwd), 2 / 4: with flipped taps and swapped channel roles for the input
                   gradient (pass it as `u` to avid_conv_dgrad); 1, 2 for wino_kernel, 3, 4 for wino2_kernel
                   (avid_conv_uses_wino says which of the two a layer runs on);
                   5 / 6: the weights (5) / their [Cin][taps][Cout] transpose (6) split into three bf16 terms (hi, mid, lo:
                   w = hi + mid + lo to fp32 accuracy) in the operand-fragment order of igemm_pk_kernel's 128 x 64 tile,
                   6 bytes per weight (avid_conv_split_bytes) — pass it as `u` to avid_conv_fwd (5) / avid_conv_dgrad (6)
                   of a layer for which avid_conv_uses_split answers 1; needs Cout % 64 == 0 and Cin % 32 == 0 (5) or
                   Cin % 64 == 0 and Cout % 32 == 0 (6) */
} avid_wt_desc;
int avid_weight_transpose_batched(int n, const avid_wt_desc* descs_dev, int64_t max_elems, avid_stream_t stream);
/* The same for ONE descriptor in HOST memory (passed to the kernel by value: nothing to upload, legal inside a stream
 * capture) — what a per-layer caller without a per-step table uses. */
int avid_weight_transform(const avid_wt_desc* desc, avid_stream_t stream);

/* Which kernel instantiation a descriptor dispatches to (which: 0 fwd, 1 dgrad, 2 wgrad), e.g.
 * "igemm_kernel<4,1,1,2,1>" — lets bench.py attribute HIP-event timings to rocprofv3 kernel names.  The answer follows the
 * launch at every size: a strided input gradient is "igemm_pk_kernel<..,1>s2 (stride-parity classes)" while dx is below
 * 2^31 bytes and "igemm_kernel<4,1,1,2,1>s2 ..." / "igemm_kernel<2,2,2,2,1>s2 ..." from there on (version >= 172; earlier
 * versions named the persistent kernel whatever the size). */
int avid_conv_kernel_name(const avid_conv_desc* d, int which, char* buf, int len);
/* Nonzero if this layer's forward (which 0) / input gradient (1) / weight gradient (2) runs on the Winograd kernels;
 * for which 0 / 1: 1 = wino_kernel, 2 = wino2_kernel (layers with >= 1.5 rounds of 64-tile units for the CUs). */
int avid_conv_uses_wino(const avid_conv_desc* d, int which);
/* Nonzero if this layer's forward (which 0) / input gradient (1) runs on the implicit-GEMM tile that reads its weights
 * pre-split into bf16 terms: `u` of avid_conv_fwd / avid_conv_dgrad is then the avid_wt_desc mode 5 / 6 table of this
 * layer (avid_conv_split_bytes bytes).  Without it (u = NULL) the same layer runs with the fp32 matrix instruction on the
 * weights as they are (and avid_conv_dgrad on wt): both forms are fp32-accurate, their roundings differ. */
int avid_conv_uses_split(const avid_conv_desc* d, int which);
size_t avid_conv_split_bytes(const avid_conv_desc* d);
/* Launches of igemm_pk_kernel that consumed a pre-split weight table since the library was loaded (tests assert that
 * avid_conv_uses_split and the kernel that ran agree; the HIP-event log names both forms igemm_pk_kernel<...>). */
long long avid_debug_presplit_launches(void);

/* Dispatch switches of the Winograd path (defaults: on, layers of >= 6000 output pixels, <= 256 output channels and
 * pixels x max(Cin, Cout) >= 1e6; environment AVID_WINO / AVID_WINO_MIN_M / AVID_WINO_MAXC / AVID_WINO_MIN_WORK — an
 * explicit min_pixels here drops the pixels x channels rule).  A negative argument returns that switch to its
 * environment / default value.  Changes what avid_conv_fwd / avid_conv_dgrad / avid_conv_wgrad dispatch to and what
 * the *_workspace_bytes / *_rows queries answer from the next call on: callers that cache those answers per layer
 * must drop them (ops.wino_configure does).  Parity tests use it to send the reference-generated small fixtures
 * (tests/golden) through the Winograd kernels (models/network_blocks.py:35,40 at 2 clips). */
int avid_wino_configure(int enabled, int64_t min_pixels, int max_channels);
/* Which of the two forward / input-gradient kernels a Winograd layer takes: wino2_kernel (one workgroup per CU, 64-tile
 * units, one instruction stream per SIMD) where the layer has at least min_rounds_x10 / 10 rounds of units for the CUs
 * (default 15, environment AVID_WINO2_MIN_ROUNDS; AVID_WINO2=0: never), wino_kernel otherwise.  0 sends every Winograd
 * layer through wino2_kernel (tests), negative restores the environment / default. */
int avid_wino2_configure(int min_rounds_x10);
/* wino2_kernel's two forms: 1 (default; environment AVID_WINO2_PRE) = wino2p_kernel — the transformed input V is split into its
 * three bf16 terms ONCE, by the thread that transforms it, and kept in LDS as the fragments the products read (a ring of three
 * half-stages of 8 transform points); 0 = every product wave splits the fragments it multiplies.  Same split, same products,
 * same order: bit-identical results (tests/test_gpu_ops.py::test_wino2_presplit_is_bit_identical).  Negative: environment /
 * default.  Takes effect from the next launch. */
int avid_wino2_pre_configure(int on);
/* wgrad_group_kernel's two forms (the grouped weight gradients of the 128-wide layers, backward of models/network_blocks.py:37-49,
 * models/audio.py:27-30): 1 (default; environment AVID_WGRAD_PRE) = every dy / x fragment is split into its three bf16 terms ONCE, by
 * the thread that stages it (one k-step of 16 pixel rows per LDS stage, fragments kept as three planes); 0 = each of the two waves
 * that share a fragment gathers and splits it itself.  Same split, same products, same order: bit-identical results
 * (tests/test_gpu_ops.py::test_grouped_weight_gradients_presplit_is_bit_identical).  Negative: environment / default. */
int avid_wgrad_pre_configure(int on);
/* The video stem's forward (models/video.py:20) in its split-bf16 form: 1 (default; environment AVID_STEM_FWD_PRE) =
 * stem_fwd3p_kernel — the input patch is split into its three bf16 terms ONCE, when it is committed to LDS (three planes), and a
 * lane's operand fragment is eight consecutive patch columns of one row, read as it is; 0 = stem_fwd3_kernel (fp32 patch, every lane
 * gathers and splits its taps per k-step).  Same products per (row, tap), assigned to other k indices of the matrix instruction:
 * results agree to rounding (tests/test_gpu_ops.py::test_stem_fwd_presplit_patch).  Inputs whose split patch does not fit in LDS
 * (224 x 224) keep stem_fwd3_kernel.  Negative: environment / default. */
int avid_stem_fwd_pre_configure(int on);

/* Which launches take tconv64_kernel — the (3,1,1) stride-1 pad-1 layers with 64 -> 64 channels and 8 frames
 * (models/network_blocks.py:37,42 in conv2x), forward and input gradient, when the layer's pre-split weights are passed
 * (`u`): every input row staged once for its three taps, the weights resident in LDS.  0: never (igemm_pk_kernel as
 * before); 1: layers with at least three rounds of 32-position tiles for the CUs (the default; environment AVID_TCONV);
 * 2: every layer it can run (tests send small fixtures through it); anything else: back to the environment / default.
 * Returns the mode in force.  Does not change any *_workspace_bytes / *_rows answer. */
int avid_tconv_configure(int mode);

/* CU budget of the persistent kernels.  igemm_pk_kernel, the stem kernels, the Winograd kernels and the grouped weight
 * gradient size their grids for — and deal their tiles over — every CU of the device; a workgroup that cannot be placed
 * (another kernel's long-lived workgroups hold the CU: RCCL's, when the gradient all-reduce of
 * utils/main_utils.py:112 runs beside the backward pass) costs such a kernel a whole extra round.  cus > 0: plan for that
 * many CUs (rounded down to a multiple of 8 = whole CUs per XCD, at least 8); cus <= 0: every CU (the default; the
 * environment variable AVID_CU_RESERVE = n starts the process at device CUs - n).  Returns the effective count, as does
 * avid_cu_budget().  Like the Winograd switches it changes what the *_workspace_bytes / *_rows queries answer: callers
 * that cache them must drop the cache (ops.set_cu_budget does).  Results stay deterministic at any budget; they are
 * bit-identical across budgets only for layers whose K-split / slab plan does not depend on the CU count. */
int avid_set_cu_budget(int cus);
int avid_cu_budget(void);

/* dw[Cout][kt][kh][kw][Cin] = sum_m dy[m][:]^T x_col[m][:]  (deterministic split-M + tree reduce). */
size_t avid_conv_wgrad_workspace_bytes(const avid_conv_desc* d);
int avid_conv_wgrad(const avid_conv_desc* d, const float* x, const float* dy, float* dw, void* ws,
                    size_t ws_bytes, avid_stream_t stream);
/* ... with x the input of the BatchNorm (+ReLU) whose output the layer convolved (avid_conv_fwd_in's twin; in = NULL:
 * avid_conv_wgrad).  Needs the layer's workspace. */
int avid_conv_wgrad_in(const avid_conv_desc* d, const float* x, const avid_in_affine* in, const float* dy, float* dw, void* ws,
                       size_t ws_bytes, avid_stream_t stream);

/* The weight gradients of up to 12 layers in ONE persistent launch (+ one grouped reduce): the small layers of a stage
 * (conv3x-5x temporal / strided / residual convolutions, audio blocks, heads — backward of models/network_blocks.py:
 * 18,20,37,42,49 and models/av_wrapper.py:25).  A launch per layer has to K-split every layer until it fills the chip
 * alone; in a group the items of all layers share one size and most layers need no split (their dw is written
 * directly).  Only layers for which avid_conv_wgrad_groupable() is 1 (128-wide dw tiles, not a stem, not on the
 * Winograd path).  Every dw is fully written (dead temporal taps as zeros).  Results equal avid_conv_wgrad's up to the
 * summation order over pixel chunks. */
typedef struct avid_wgrad_item {
  avid_conv_desc d;
  const float* x;
  const float* dy;
  float* dw;
} avid_wgrad_item;
int avid_conv_wgrad_groupable(const avid_conv_desc* d);
size_t avid_conv_wgrad_group_workspace_bytes(int n, const avid_wgrad_item* items);
int avid_conv_wgrad_group(int n, const avid_wgrad_item* items, void* ws, size_t ws_bytes, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm (train / eval) over a channels-last [M, C] view, fused ReLU.
 * Replaces nn.BatchNorm3d/2d + nn.ReLU: models/network_blocks.py:19,21,36,38,41,43,54-59,
 * models/video.py:21-22, models/audio.py:23-24.
 * ---------------------------------------------------------------------------------------------- */
size_t avid_bn_workspace_bytes(int64_t M, int C);
/* Train: batch mean / biased var -> save_mean, save_invstd [C]; running stats updated in place
 * (momentum, unbiased var); y = [relu](fma(x, scale, shift)) with scale = gamma * invstd,
 * shift = beta - mean * scale, both also saved ([C]) so backward can recompute the ReLU mask bit-exactly.
 * num_batches_tracked: device int64 counter bumped by one (nn.BatchNorm's buffer), or NULL.
 * partials / nparts: [nparts][2][C] partial sums of x from avid_conv_fwd (skips the statistics pass), or NULL / 0.
 * y = NULL (version >= 130): statistics only — the saved vectors and the running statistics are made, the normalised tensor
 * is not; its consumer applies the map while it stages x (avid_conv_fwd_in / avid_conv_wgrad_in). */
int avid_bn_fwd_train(int64_t M, int C, const float* x, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, int relu,
                      float* y, float* save_mean, float* save_invstd, float* save_scale,
                      float* save_shift, int64_t* num_batches_tracked, const float* partials, int nparts,
                      void* ws, size_t ws_bytes, avid_stream_t stream);
/* Eval: uses running stats.  save4 (nullable, [4][C]): a backward will follow (frozen-BatchNorm fine-tuning) —
 * mean (= running_mean) / invstd / scale / shift are written there and y = fma(x, scale, shift), the expression
 * avid_bn_bwd(frozen = 1) recomputes the ReLU mask with. */
int avid_bn_fwd_eval(int64_t M, int C, const float* x, const float* gamma, const float* beta,
                     const float* running_mean, const float* running_var, float eps, int relu,
                     float* y, float* save4, avid_stream_t stream);
/* Inference (version >= 160).  The two halves of avid_bn_fwd_eval(save4) as calls of their own:
 * avid_bn_eval_coeffs_batched — ONE launch that writes the [4][C] vectors (mean = running_mean, invstd = 1 / sqrt(var + eps),
 * scale = gamma * invstd, shift = beta - mean * scale: the bits avid_bn_fwd_eval writes to save4) of n BatchNorms from a table
 * in DEVICE memory; every C a power of two in [4, 1024];
 * avid_bn_apply_eval — y = [relu](fma(x, scale[c], shift[c])) with such vectors (x == y allowed). */
typedef struct avid_bn_eval_item {
  const float* gamma;
  const float* beta;
  const float* running_mean;
  const float* running_var;
  float* out;                 /* [4][C] */
  float eps;
  int32_t C;
} avid_bn_eval_item;
int avid_bn_eval_coeffs_batched(int n, const avid_bn_eval_item* items_dev, avid_stream_t stream);
int avid_bn_apply_eval(int64_t M, int C, const float* x, const float* scale, const float* shift, int relu, float* y,
                       avid_stream_t stream);
/* Backward of train-mode BN(+ReLU).  The ReLU mask is fma(x, scale, shift) > 0 recomputed from the conv
 * output x (the forward's exact expression), so the saved activation is not re-read: 2 + 3 passes.
 * partials / nparts: the partial sums the dgrad that produced dy already made (avid_conv_dgrad's `bn`), or
 * NULL / 0 — then the 2-read statistics pass runs here.
 * frozen != 0: backward of an EVAL-mode BatchNorm (statistics are constants): dx = gamma * invstd * dy_m,
 * dgamma = sum dy_m * xhat, dbeta = sum dy_m. */
int avid_bn_bwd(int64_t M, int C, const float* x, const float* dy, const float* gamma,
                const float* save_mean, const float* save_invstd, const float* save_scale,
                const float* save_shift, int relu, float* dx, float* dgamma, float* dbeta,
                const float* partials, int nparts, int frozen, void* ws, size_t ws_bytes,
                avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling.  MaxPool3d((1,3,3),(1,2,2),(0,1,1)) — models/video.py:23;  AdaptiveMaxPool{3,2}d(1) —
 * models/video.py:41, models/audio.py:31.  Ties: first maximum in (t,h,w) scan order (ATen CPU).
 * ---------------------------------------------------------------------------------------------- */
/* Stem tail fused (models/video.py:21-23): y = maxpool(relu(bn_train(x))) with x [B,T,H,W,C] the stem conv
 * output, y / argmax [B,T,Ho,Wo,C]; the normalised activation is never materialised.  Backward rebuilds the
 * un-pooled gradient from (dy, argmax) on the fly.  Same saved tensors / workspace / `partials` (the stem
 * convolution's own BatchNorm partial sums, avid_conv_fwd) as avid_bn_fwd_train. */
int avid_bn_relu_maxpool_fwd(int B, int T, int H, int W, int C, const float* x, const float* gamma,
                             const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                             float* y, uint8_t* argmax, float* save_mean, float* save_invstd, float* save_scale,
                             float* save_shift, int64_t* num_batches_tracked, const float* partials, int nparts,
                             void* ws, size_t ws_bytes, avid_stream_t stream);
int avid_bn_relu_maxpool_bwd(int B, int T, int H, int W, int C, const float* x, const float* dy,
                             const uint8_t* argmax, const float* gamma, const float* save_mean,
                             const float* save_invstd, const float* save_scale, const float* save_shift, float* dx,
                             float* dgamma, float* dbeta, void* ws, size_t ws_bytes, avid_stream_t stream);
/* The stem tail in eval mode (version >= 160): y = maxpool(relu(fma(x, scale[c], shift[c]))) in one pass, scale / shift [C]
 * from the running statistics (avid_bn_eval_coeffs_batched).  No argmax, no saved vectors.  The values of
 * avid_bn_fwd_eval(save4, relu = 1) followed by avid_maxpool_hw3s2_fwd, bit for bit (signed zeros and ties included). */
int avid_bn_relu_maxpool_fwd_eval(int B, int T, int H, int W, int C, const float* x, const float* scale, const float* shift,
                                  float* y, avid_stream_t stream);
int avid_maxpool_hw3s2_fwd(int B, int T, int H, int W, int C, const float* x, float* y,
                           uint8_t* argmax, avid_stream_t stream);
int avid_maxpool_hw3s2_bwd(int B, int T, int H, int W, int C, const float* dy,
                           const uint8_t* argmax, float* dx, avid_stream_t stream);
/* x [B, S, C] -> y [B, C], argmax [B, C] (int32 position in S). */
int avid_global_maxpool_fwd(int B, int S, int C, const float* x, float* y, int32_t* argmax,
                            avid_stream_t stream);
int avid_global_maxpool_bwd(int B, int S, int C, const float* dy, const int32_t* argmax, float* dx,
                            avid_stream_t stream);

/* Small helpers for the projection heads (models/av_wrapper.py:23-29). */
int avid_relu_bwd(int64_t n, const float* y, const float* dy, float* dx, avid_stream_t stream);
int avid_colsum(int64_t M, int C, const float* x, float* out, avid_stream_t stream); /* bias grad */

/* ------------------------------------------------------------------------------------------------
 * Criterion path (criterions/avid.py, criterions/nce.py, utils/alias_method.py).
 * ---------------------------------------------------------------------------------------------- */
/* F.normalize(x, p=2, dim=1) — criterions/avid.py:52-53.  norm_out [bs] = max(||x||, 1e-12). */
int avid_l2norm_fwd(int bs, int D, const float* x, float* y, float* norm_out, avid_stream_t stream);
int avid_l2norm_bwd(int bs, int D, const float* y, const float* norm, const float* dy, float* dx,
                    avid_stream_t stream);

/* AliasMethod.draw + "avoid self" — utils/alias_method.py:56-71, criterions/avid.py:82-86.
 * out[i] = alias_select(prob, alias, kk_i, u_i) with (kk_i, u_i) from Philox4x32-10
 * (counter = (i, offset), key = seed); if y != NULL: out[i] += (out[i] >= y[i / per_row]).
 * uniform != 0 short-circuits the table lookup for the all-ones table (prob == 1, alias == 0).
 * offset_dev != NULL: the offset is read from device memory instead of the by-value argument. */
int avid_alias_draw(int64_t n, int64_t K, const float* prob, const int64_t* alias, int uniform,
                    uint64_t seed, uint64_t offset, const uint64_t* offset_dev, const int64_t* y,
                    int64_t per_row, int64_t* out, avid_stream_t stream);
/* *counter += inc on the stream.  offset_dev (above) / step_dev (avid_adam_flat) point at such device
 * counters so a captured hipGraph of the whole step advances its RNG stream / Adam step on replay. */
int avid_counter_add(uint64_t* counter, uint64_t inc, avid_stream_t stream);

/* Device-side index errors.  The reference's gathers / index_copy_ raise an IndexError for an id outside
 * [0, N) (criterions/avid.py:57-62,124; avid_cma.py:199).  A kernel cannot raise: the three entry points below
 * take `err` (nullable), one int32 word in device memory that they OR a code into while staying inside the
 * table themselves (gathers clamp, the update skips the sample).  The host polls the word without a
 * synchronisation (avid_hip/ops.py: DeviceErrors) and raises IndexError at most one step late. */
#define AVID_DEVERR_BANK_INDEX 1   /* avid_bank_scores_fwd: idx outside [0, N) */
#define AVID_DEVERR_UPDATE_INDEX 2 /* avid_bank_update: y outside [0, N) */
#define AVID_DEVERR_CMA_INDEX 4    /* avid_cma_negatives: y outside [0, N) */
#define AVID_DEVERR_CLS_LABEL 8    /* avid_cls_loss: label outside [0, C) */
#define AVID_DEVERR_MLABEL_TARGET 16 /* avid_mlabel_loss: target outside [0, 1] or not finite */
#define AVID_DEVERR_RANK_SCORE 32  /* avid_rank_metrics: NaN score */
#define AVID_DEVERR_SOFT_TARGET 64 /* avid_soft_ce_loss: target negative or not finite */
#define AVID_DEVERR_MIX_INDEX 128  /* avid_batch_mix: perm[b] outside [0, B) */
#define AVID_DEVERR_SVM_LABEL 256  /* avid_svm_hinge / avid_svm_loss: label outside [0, C) */

/* Action-recognition fine-tuning head (utils/eval_utils.py:193-214, eval-action-recg.py:150-165) — classify.hip.
 *
 * Dropout over x [B, F]: element i = b * F + f is kept iff word i % 4 of Philox4x32-10 with counter
 * (i / 4 lo, i / 4 hi, offset lo, offset hi) and key seed is >= floor(p * 2^32); y = x * mask * (1 / (1 - p)), the scale
 * computed in fp32.  mask [B * F] bytes (0 / 1) is kept for the backward.  offset_dev != NULL: the offset is read from
 * device memory, as avid_alias_draw does.  The masks follow torch.nn.Dropout's distribution, not its bits.  0 <= p < 1. */
int avid_dropout_fwd(int64_t B, int64_t F, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                     const float* x, float* y, uint8_t* mask, avid_stream_t stream);
/* dx = dy * mask * (1 / (1 - p)) over n elements. */
int avid_dropout_bwd(int64_t n, float p, const uint8_t* mask, const float* dy, float* dx, avid_stream_t stream);
/* Softmax cross-entropy of logits [V * clips][C] (1 <= C <= 1024; rows v * clips .. v * clips + clips - 1 are video v's
 * clips) against labels [V] (int64), one launch:
 *   loss[0]     = mean over all V * clips rows of -log softmax(row)[labels[v]]  (clips = 1: the train / test loss)
 *   conf [V][C] = mean over each video's clips of softmax(row)                 (nullable)
 *   hits[2]     = (top-1, top-5) hit counts of conf, int64                      (nullable; written on the device, no sync)
 *   dlogits     = (softmax(row) - onehot(label)) * grad_scale / (V * clips)     (nullable: the training case)
 * Rank rule of the hit counts: a label's rank is the number of classes with strictly greater confidence plus the number
 * with equal confidence at a lower class index; top-k hits rank < k.  A label outside [0, C) ORs AVID_DEVERR_CLS_LABEL into
 * err (nullable) and scores no hit.  The summation order is fixed and no result is accumulated with atomics: every output
 * is bit-reproducible from run to run. */
int avid_cls_loss(int V, int clips, int C, const float* logits, const int64_t* labels, float grad_scale, float* loss,
                  float* conf, int64_t* hits, float* dlogits, int32_t* err, avid_stream_t stream);
/* Multi-label sibling of avid_cls_loss (version >= 167): binary cross-entropy with logits, torch's
 * binary_cross_entropy_with_logits, of logits [V * clips][C] (1 <= C <= 1024) against targets [V][C] in [0, 1] (a video's
 * clips share its targets); pos_weight [C] nullable (all ones).  Per element, with w = 1 + (pos_weight[c] - 1) t:
 *   l           = (1 - t) x + w (log1p(exp(-|x|)) + max(-x, 0))             (the stable softplus is part of the contract)
 *   loss[0]     = mean of l over all V * clips * C elements
 *   dlogits     = ((1 - t) - w (1 - sigmoid(x))) * grad_scale / (V * clips * C)   (nullable)
 *   conf [V][C] = mean over each video's clips of sigmoid(x) — not the sigmoid of the mean   (nullable)
 *   hits[2]     (nullable; a class is positive iff t >= 0.5): hits[0] = videos whose highest-confidence class is positive
 *                (ties to the lower class index, avid_cls_loss's rank rule), hits[1] = (video, class) pairs with
 *                (conf >= 0.5) == (t >= 0.5)
 * A target outside [0, 1] or not finite ORs AVID_DEVERR_MLABEL_TARGET into err (nullable).  A grid over the videos
 * (min(V, 1024) workgroups), a partial sum per workgroup, the partial sums added in index order by a second small launch:
 * no floating-point atomics, every output has the same bits on every run and under every avid_set_cu_budget.  The partial
 * sums live in device memory the library owns: 16 slabs per device drawn round-robin per call, so a call's slab is written
 * again by the 16th later call on that device (the contract of the event pool below). */
int avid_mlabel_loss(int V, int clips, int C, const float* logits, const float* targets, const float* pos_weight,
                     float grad_scale, float* loss, float* conf, int64_t* hits, float* dlogits, int32_t* err,
                     avid_stream_t stream);
/* Softmax cross-entropy against a DISTRIBUTION (version >= 168): label smoothing, mixup / CutMix targets, distillation —
 * torch's F.cross_entropy(logits, target_probs, label_smoothing = eps) with mean reduction, of logits [V * clips][C]
 * (1 <= C <= 1024) against targets [V][C] float32 (a video's clips share its targets), 0 <= label_smoothing < 1
 * (AVID_E_BADARG otherwise).  The targets are NOT renormalised (torch does not): with t'[c] = t[c] (1 - eps) + eps / C and
 * S = sum_c t'[c] (not assumed to be 1),
 *   row loss    = sum_c t'[c] (lse(row) - x[c]), lse = log(sum_c exp(x[c] - max)) + max   (log-softmax through the row max)
 *   loss[0]     = mean of the row losses over the V * clips rows
 *   dlogits     = (softmax(row)[c] * S - t'[c]) * grad_scale / (V * clips)                 (nullable)
 *   conf [V][C] = mean over each video's clips of softmax(row), as avid_cls_loss's         (nullable)
 *   hits[2]     (nullable) = top-1 / top-5 hits by avid_cls_loss's rank rule; a video's label is the argmax of its target
 *                row, ties in the targets and in the confidences to the lower class index
 * A target that is negative or not finite ORs AVID_DEVERR_SOFT_TARGET into err (nullable); such a video counts no hit and
 * its outputs are whatever the arithmetic gives.  A grid over the videos (min(V, 1024) workgroups of 256 threads, a thread
 * holds its columns of a row in registers), every float sum of a row in one fixed order, the element losses added in double,
 * one partial sum per workgroup, the partial sums added in index order by a second small launch (avid_mlabel_loss's, out
 * of a slab of the same ring: 16 slabs per device drawn round-robin per call of either function).  No floating-point
 * atomics: every output has the same bits on every run and under every avid_set_cu_budget. */
int avid_soft_ce_loss(int V, int clips, int C, const float* logits, const float* targets, float label_smoothing,
                      float grad_scale, float* loss, float* conf, int64_t* hits, float* dlogits, int32_t* err,
                      avid_stream_t stream);
/* Mixup and CutMix of a batch in one launch (version >= 168) — batchmix.hip.  x, y: [B][Cin][T][H][W] float32, channel-first
 * as the stems read them (a spectrogram [B][1][T][F] is Cin = 1, T = 1, H = T, W = F); y must not overlap x (AVID_E_BADARG).
 * perm [B] int64: the partner of every sample (NULL: the identity); lam [B] float32 in [0, 1] (NULL: all ones).
 *   mode AVID_MIX_MIXUP    y[b] = lam[b] * x[b] + (1 - lam[b]) * x[perm[b]]: two products, one difference and one sum, each
 *                          rounded on its own (never contracted into an fma) — torch's float32 expression bit for bit
 *   mode AVID_MIX_CUTMIX   box [B][4] int32 = (h0, h1, w0, w1), half-open: y[b][.., h, w] = x[perm[b]][.., h, w] inside the
 *                          box (all channels and frames), x[b][.., h, w] outside — an exact copy; an empty box copies x[b];
 *                          lam enters the targets only
 *   targets (t_out [B][n_classes] nullable: skipped)   t_out[b][c] = lam[b] * t[b][c] + (1 - lam[b]) * t[perm[b]][c] by the
 *                          same four roundings; t is t_in [B][n_classes], or the one-hot of labels_in [B] int64 — exactly one
 *                          of the two is non-NULL
 * x and y may both be NULL: the targets alone (with perm and lam NULL: the one-hot rows of labels_in).
 * A perm[b] outside [0, B) ORs AVID_DEVERR_MIX_INDEX into err (nullable); nothing out of bounds is read, that sample and its
 * targets are copied unmixed.  A label outside [0, n_classes) ORs AVID_DEVERR_CLS_LABEL and is a zero row.
 * Any H, W; a sample of fewer than 2^31 floats.  16-byte vectors over the aligned body of every output sample, a source that
 * is not 16-byte aligned at the same element is read in dwords; memory-bound (mixup 12, CutMix 8 bytes per element).
 * Every output element is computed by one thread from its own inputs: the same bits on every run. */
#define AVID_MIX_MIXUP 0
#define AVID_MIX_CUTMIX 1
int avid_batch_mix(int mode, int64_t B, int64_t Cin, int64_t T, int64_t H, int64_t W, const float* x, const int64_t* perm,
                   const float* lam, const int32_t* box, float* y, int64_t n_classes, const float* t_in,
                   const int64_t* labels_in, float* t_out, int32_t* err, avid_stream_t stream);
/* The classifier Linear(Fin, C) for any C (avid_conv_fwd's igemm takes Cout in multiples of 64):
 * y [B][C] = x [B][Fin] . w [C][Fin]^T + bias (bias nullable).  Backward: dw = dy^T . x, db = column sums of dy (nullable),
 * dx = dy . w (nullable).  Each output is one sum in index order: deterministic. */
int avid_cls_linear_fwd(int B, int Fin, int C, const float* x, const float* w, const float* bias, float* y,
                        avid_stream_t stream);
int avid_cls_linear_bwd(int B, int Fin, int C, const float* x, const float* w, const float* dy, float* dx, float* dw,
                        float* db, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Linear-probe heads (utils/eval_utils.py:217-242, 298-329: Classifier / MOSTModel; eval-action-recg-linear.py) — probe.hip.
 * Version >= 140.
 * ---------------------------------------------------------------------------------------------- */
/* nn.AdaptiveMaxPool3d((To, Ho, Wo)) of a channels-last tap x [B,T,H,W,C] straight into the reference's flatten order:
 * y [B][C][To][Ho][Wo] (= pooling(x_ncdhw).view(B, -1), utils/eval_utils.py:237-239), so classifier weights interchange with
 * the reference's.  Output index i of an axis covers floor(i * In / Out) .. ceil((i + 1) * In / Out) (torch's rule), for any
 * output size, Out > In included.  A NaN in a window makes its output NaN, as torch's does.  One workgroup owns a (b, to,
 * channel chunk) and walks its rows once: every input element is fetched from HBM once (overlapping windows re-read it from
 * cache).  NO argmax and NO backward: the reference pools under torch.no_grad(), nothing ever differentiates through it. */
int avid_adaptive_maxpool_fwd(int B, int T, int H, int W, int C, int To, int Ho, int Wo, const float* x, float* y,
                              avid_stream_t stream);
/* nn.BatchNorm1d(F) over x [B, F] (utils/eval_utils.py:225,241), any F, B >= 2 in training mode.
 * Train: batch mean / biased variance per feature (accumulated in double) -> save2 [2][F] = mean | invstd; running statistics
 * updated in place (momentum, unbiased variance); num_batches_tracked (device int64, nullable) bumped by one;
 * y = (x - mean) * invstd * gamma + beta.
 * Eval: the running statistics; save2 (nullable) receives running_mean | invstd for a backward with frozen = 1.
 * Backward: dx, dgamma, dbeta from (x, dy, gamma); dx nullable (the probe's input takes no gradient).  In training mode it
 * rebuilds the batch statistics in double from x and eps (with two rows dx cancels to eps / (var + eps) of its terms, more
 * than float32 statistics carry; save2 is then not read and may be NULL).
 * frozen != 0: the statistics were constants (eval mode), read from save2: dx = gamma * invstd * dy.
 * One workgroup owns 64 features and sums over the batch in a fixed order: bit-reproducible. */
int avid_bn1d_fwd_train(int B, int F, const float* x, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float momentum, float eps, float* y, float* save2,
                        int64_t* num_batches_tracked, avid_stream_t stream);
int avid_bn1d_fwd_eval(int B, int F, const float* x, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* y, float* save2, avid_stream_t stream);
int avid_bn1d_bwd(int B, int F, const float* x, const float* dy, const float* gamma, const float* save2, float eps,
                  int frozen, float* dx, float* dgamma, float* dbeta, avid_stream_t stream);
/* The probe's Linear(Fin, C) on the matrix pipe (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation), B <= 256,
 * Fin <= 16384, any C:  y [B][C] = x [B][Fin] . w [C][Fin]^T + bias (nullable);  backward: dw [C][Fin] = dy^T . x,
 * db [C] = column sums of dy (nullable), dx [B][Fin] = dy . w (nullable).  64 x 64 output tiles; the reduction axis is cut
 * into slices of 512 (the forward has only ceil(B/64) * ceil(C/64) tiles), each slice's partial tile goes to ws and a second
 * launch adds the slices in index order — no atomics, every output bit-reproducible from run to run.
 * ws: avid_probe_linear_workspace_bytes(B, Fin, C) bytes (covers the forward and the backward). */
size_t avid_probe_linear_workspace_bytes(int B, int Fin, int C);
int avid_probe_linear_fwd(int B, int Fin, int C, const float* x, const float* w, const float* bias, float* y, void* ws,
                          size_t ws_bytes, avid_stream_t stream);
int avid_probe_linear_bwd(int B, int Fin, int C, const float* x, const float* w, const float* dy, float* dx, float* dw,
                          float* db, void* ws, size_t ws_bytes, avid_stream_t stream);

/* scores[b][j] = <bank[idx[b][j]], emb[b]> * inv_T — the gather + bmm of criterions/avid.py:57-71.
 * idx [bs][R] int64, bank [N][D], emb [bs][D], D in {64,128,256,512}.  rows_out (nullable,
 * [bs][R][D]) receives a snapshot of the gathered rows: the reference's autograd keeps the
 * PRE-update rows for backward (the bank is updated inside forward, avid.py:78). */
int avid_bank_scores_fwd(int bs, int R, int D, int64_t N, const int64_t* idx, const float* bank,
                         const float* emb, float inv_T, float* scores, float* rows_out, int32_t* err,
                         avid_stream_t stream);
/* demb[b] (+)= inv_T * sum_j dscores[b][j] * row(b,j)  (autograd of torch.bmm, avid.py:66), where
 * row(b,j) = rows[b][j] if rows != NULL (the snapshot) else bank[idx[b][j]]. */
int avid_bank_scores_bwd(int bs, int R, int D, int64_t N, const float* rows, const int64_t* idx,
                         const float* bank, const float* dscores, float inv_T, int accumulate,
                         float* demb, avid_stream_t stream);

/* NCE — criterions/nce.py:38-58.  Score matrices are row-major with leading dimension ld_* so the
 * positive / negative column blocks of one [bs][P+K] score buffer can be passed without a copy.
 * mean_exp: out[0] = mean(exp(s[rows][cols])) (first-call Z, nce.py:27).
 * fwd: loss[0] (+)= scale * mean_b( -mean_p log Pmt - sum_k log Pon ); Z is read from device memory.
 * bwd: dpos [bs][P], dneg [bs][K] (dense) = dloss[0] * scale * dL/ds. */
int avid_mean_exp(int rows, int cols, int ld, const float* s, float* out, avid_stream_t stream);
size_t avid_nce_workspace_bytes(void);
/* ws: optional scratch of avid_nce_workspace_bytes(), ZERO-FILLED ONCE by the caller and then left to this op
 * (per-block partial sums + a ticket counter the kernel re-arms itself); NULL -> single-block kernel. */
int avid_nce_fwd(int bs, int P, int K, const float* spos, int ld_pos, const float* sneg, int ld_neg,
                 const float* Z, float scale, int accumulate, float* loss, void* ws, size_t ws_bytes,
                 avid_stream_t stream);
int avid_nce_bwd(int bs, int P, int K, const float* spos, int ld_pos, const float* sneg, int ld_neg,
                 const float* Z, const float* dloss, float scale, float* dpos, float* dneg,
                 avid_stream_t stream);

/* update_memory — criterions/avid.py:118-129: bank[y[i]] = normalize(m*bank[y[i]] + (1-m)*emb[i]).
 * Duplicate ids: the LAST occurrence wins (the reference's index_copy_ order is unspecified). */
int avid_bank_update(int B, int D, int64_t N, float* bank, const int64_t* y, const float* emb,
                     float momentum, int32_t* err, avid_stream_t stream);

/* Fused cross-modal criterion for the steady state (partition constant Z already frozen, criterions/nce.py:22-24):
 * criterions/avid.py:52-71 (F.normalize of both embeddings; gather of row y and of the K negative rows idx from BOTH
 * banks; bmm / T: v2a = video embedding . audio bank, a2v = audio embedding . video bank) + criterions/nce.py:38-58 for
 * both score sets + the backward of all of it with respect to the two raw embeddings, formed in the same pass while a
 * gathered row is in registers (the banks are updated before backward runs, avid.py:78 — the unfused ops keep a
 * snapshot of the gathered rows for that; here none is needed).
 *   v_emb, a_emb [bs][128] raw embeddings; y [bs], idx [bs][K] int64; bank_v = view1_mem, bank_a = view2_mem;
 *   v_hat, a_hat [bs][128]: the normalised embeddings (input of the bank update / its all-gather);
 *   losses [4]: L_v2a, L_a2v, L_v2a / 2 + L_a2v / 2 (avid.py:221-222), coeff * that (the total loss);
 *   dv, da [bs][128]: d(total) / d(v_emb), d(total) / d(a_emb) for an upstream gradient of 1.
 * ws: avid_xmodal_fused_workspace_bytes(bs, K) bytes, ZERO-FILLED ONCE by the caller and then owned by this op (device
 * tickets that re-arm themselves); one per stream that may run the op concurrently.  Fixed summation order, no
 * floating-point atomics.  D must be 128.  err: device error word (AVID_DEVERR_BANK_INDEX), may be NULL. */
size_t avid_xmodal_fused_workspace_bytes(int bs, int K);
int avid_xmodal_fused(int bs, int K, int D, int64_t N, const float* v_emb, const float* a_emb, const int64_t* y,
                      const int64_t* idx, const float* bank_v, const float* bank_a, float inv_T, const float* Z,
                      float coeff, float* v_hat, float* a_hat, float* losses, float* dv, float* da, void* ws,
                      size_t ws_bytes, int32_t* err, avid_stream_t stream);
/* The same for the AVID+CMA criterion in its stock form — cross-modal instance terms + within-modal positive terms
 * (criterions/avid_cma.py:150-194, 338-358 with xModalInst and wModalPos on; Z frozen): rows gathered once from both
 * banks = the sample's own row y | its P positives pos[bs][P] (avid_cma_negatives) | the K negatives idx[bs][K]; four
 * score sets per row pair (inst-v2a / inst-a2v over self + K negatives, pos-v2v / pos-a2a over the P positives — mean
 * over P, criterions/nce.py:44 — and the first Kw negatives, avid_cma.py:184-190), their NCE terms, and the gradient of
 *   total = coeff_inst (L_inst-v2a + L_inst-a2v) / 2 + coeff_pos (L_pos-v2v + L_pos-a2a) / 2
 * with respect to both raw embeddings (each receives gradient through rows of BOTH banks).
 *   losses [8]: L_inst-v2a, L_inst-a2v, L_pos-v2v, L_pos-a2a, the two group means, the total, (unused).
 * Everything else as avid_xmodal_fused (ws: avid_cma_fused_workspace_bytes(bs, P, K), zero-filled once). */
size_t avid_cma_fused_workspace_bytes(int bs, int P, int K);
int avid_cma_fused(int bs, int P, int K, int Kw, int D, int64_t N, const float* v_emb, const float* a_emb, const int64_t* y,
                   const int64_t* pos, const int64_t* idx, const float* bank_v, const float* bank_a, float inv_T,
                   const float* Z, float coeff_inst, float coeff_pos, float* v_hat, float* a_hat, float* losses, float* dv,
                   float* da, void* ws, size_t ws_bytes, int32_t* err, avid_stream_t stream);
/* The general form of the two entry points above: ANY term set of criterions/avid.py and criterions/avid_cma.py with Z
 * frozen, in the same two launches.  Rows gathered once from both banks = the sample's own row y | its P positives
 * pos[bs][P] (P may be 0) | the K negatives idx[bs][K]; a row pair gives four dot products (v_hat . bank_a row,
 * a_hat . bank_v row, v_hat . bank_v row, a_hat . bank_a row) and `mask` says which NCE terms they enter:
 *   AVID_CRIT_X_INST  v2a / a2v: positive = row y, negatives = all K        (avid.py xModal; avid_cma.py xModalInst / wModalInst)
 *   AVID_CRIT_W_INST  v2v / a2a: positive = row y, negatives = all K        (avid.py wModal)
 *   AVID_CRIT_X_POS   pos-v2a / pos-a2v: the P positives (mean over P, nce.py:44), negatives = all K       (xModalPos)
 *   AVID_CRIT_W_POS   pos-v2v / pos-a2a: the P positives, negatives = the first Kw                           (wModalPos)
 *   total = sum over the groups g of the mask, in the order above, of coeff[g] * (L_g,first / 2 + L_g,second / 2)
 * A score that serves two terms (a negative's v2a score under X_INST | X_POS) carries the sum of both dL/ds.  A set bit
 * with coeff 0 reports its losses and contributes no gradient.
 *   losses [16], every element written: [0..7] the term losses in the order X_INST (v2a, a2v), W_INST (v2v, a2a), X_POS,
 *   W_POS — 0 for a term that is off; [8..11] the four group means; [12] the total; [13..15] 0.
 *   v_hat, a_hat, dv, da, err, Z: as avid_xmodal_fused.  pos may be NULL when P = 0.
 * Limits: D = 128 (AVID_E_UNSUPPORTED otherwise); mask in 1..15, bs, K > 0, P >= 0 and P >= 1 with a *_POS bit,
 * 1 <= Kw <= K, ws_bytes >= avid_crit_fused_workspace_bytes(bs, P, K) (ws zero-filled once by the caller, then owned by
 * this op), no null pointer: AVID_E_BADARG otherwise, before anything is launched. */
#define AVID_CRIT_X_INST 1
#define AVID_CRIT_W_INST 2
#define AVID_CRIT_X_POS 4
#define AVID_CRIT_W_POS 8
typedef struct avid_crit_desc {
  int32_t bs, P, K, Kw, D, mask;
  int64_t N;
  const float* v_emb;
  const float* a_emb;
  const int64_t* y;
  const int64_t* pos;
  const int64_t* idx;
  const float* bank_v;
  const float* bank_a;
  const float* Z;
  float inv_T;
  float coeff[4];
  int32_t reserved;
  float* v_hat;
  float* a_hat;
  float* losses;
  float* dv;
  float* da;
} avid_crit_desc;
size_t avid_crit_fused_workspace_bytes(int bs, int P, int K);
int avid_crit_fused(const avid_crit_desc* d, void* ws, size_t ws_bytes, int32_t* err, avid_stream_t stream);
/* In-batch cross-modal InfoNCE (the symmetric CLIP / GDT loss; version >= 171) — infonce.hip.  No memory bank: the keys
 * are the other modality's embeddings of the GLOBAL batch.  v_hat, a_hat [G][D]: the unit-norm embeddings of the global
 * batch (every process holds all of them); rows [row0, row0 + b) are the ones this process owns.  With
 * S_ij = v_hat_i . a_hat_j * inv_T, lse_v[i] = logsumexp_j S_ij and lse_a[j] = logsumexp_i S_ij, all over the G keys:
 *   loss[1]  = mean_i (lse_v[i] - S_ii)            (video -> audio)
 *   loss[2]  = mean_j (lse_a[j] - S_jj)            (audio -> video)
 *   loss[0]  = w_v2a loss[1] + w_a2v loss[2]       — over the global batch, the same on every process
 *   hits[2]  (int64, nullable): rows i whose lowest-index maximum of S_i. is i; columns j likewise for S_.j
 *   W_ij     = grad_scale (w_v2a (exp(S_ij - lse_v[i]) - delta_ij) + w_a2v (exp(S_ij - lse_a[j]) - delta_ij)) inv_T / G
 *   dv [b][D]: d(grad_scale loss[0]) / d v_hat_i = sum_j W_ij a_hat_j, i = row0 .. row0 + b - 1
 *   da [b][D]: d(grad_scale loss[0]) / d a_hat_j = sum_i W_ij v_hat_i, j = row0 .. row0 + b - 1
 * — the exact gradient of the global loss for the local rows, the key-role term (a local sample as a negative of every
 * other process's queries) included; dv and da are both NULL (loss and hits only) or both given.
 * Products are fp32 FMAs, one accumulator per score fed in the order d = 0 .. D-1: a score has the same bits wherever its
 * pair sits in a tile and whichever side is the query, so bit-identical key rows give bit-identical scores.  The softmax
 * shifts by the row's true running maximum.  Every sum over keys runs in key order with tiles cut at absolute key
 * indices, the loss is added up in double in index order; no floating-point atomics, no grid sized from the CU count:
 * dv / da rows and the loss have the same bits on every run, under every avid_set_cu_budget and for every (row0, b).
 * No [G][G] matrix is stored: ws holds lse_v, lse_a, the diagonal and the hit flags, avid_infonce_workspace_bytes(G) =
 * 20 G bytes rounded up to 256, written before it is read (no zero-fill).  Three launches on `stream`, no host
 * synchronisation (capturable).  Refused before anything is launched: G < 1, row0 < 0, b < 0, row0 + b > G, a null v_hat /
 * a_hat / loss / ws, embeddings or gradients not 16-byte aligned, inv_T <= 0, a negative or non-finite weight, a short
 * workspace (AVID_E_BADARG); D not a multiple of 32 in [32, 512] (AVID_E_UNSUPPORTED).  G = 1: loss 0, gradients 0. */
size_t avid_infonce_workspace_bytes(int G);
int avid_infonce(int G, int D, int row0, int b, const float* v_hat, const float* a_hat, float inv_T, float w_v2a, float w_a2v,
                 float grad_scale, float* loss, int64_t* hits, float* dv, float* da, void* ws, size_t ws_bytes,
                 avid_stream_t stream);
/* avid_bank_update for both banks in one launch (criterions/avid.py:118-129): bank0 <- emb0 (momentum0), bank1 <- emb1; bit-identical to two avid_bank_update calls. */
int avid_bank_update2(int B, int D, int64_t N, float* bank0, float* bank1, const int64_t* y, const float* emb0,
                      const float* emb1, float momentum0, float momentum1, int32_t* err, avid_stream_t stream);

/* memory_sampling remap — criterions/avid_cma.py:196-209.  positive_set int32 [N][P] (rows sorted);
 * pos_out [bs][P] = positive_set[y];  neg_out[b][k] = r + #{j : r >= pos_j - j}, r = rand_idx[b][k]. */
int avid_cma_negatives(int bs, int K, int P, int64_t N, const int32_t* positive_set, const int64_t* y,
                       const int64_t* rand_idx, int64_t* pos_out, int64_t* neg_out, int32_t* err,
                       avid_stream_t stream);

/* CMA correspondence search — criterions/avid_cma.py:42-73: for queries q in [q0, q0+nq):
 * sim = combine(V V[q]^T, A A[q]^T) (kind 0 consensus=min, 1 union=max, 2 video, 3 audio);
 * top-(pos_k+1) by similarity, drop the best (self), sort ascending -> out [nq][pos_k] int32. */
size_t avid_cma_topk_workspace_bytes(int64_t N, int nq, int pos_k);
/* fallbacks (nullable): device int32 counter, += 1 when this batch overflowed the threshold filter's candidate
 * lists (heavy score ties) and was redone by the exact scan — diagnostics, the result is exact either way. */
int avid_cma_topk(int64_t N, int D, const float* view1, const float* view2, int64_t q0, int nq,
                  int pos_k, int kind, int32_t* out, int32_t* fallbacks, void* ws, size_t ws_bytes,
                  avid_stream_t stream);

/* k-nearest-neighbour search (k-NN / retrieval evaluation of a frozen tower): for nq query rows [nq][D] against a
 * gallery [N][D] (fp32, row-major) the k gallery rows of largest dot product per query, ordered by (similarity
 * descending, gallery index ascending) -> out_idx int32 [nq][k], out_sim fp32 [nq][k].
 * exclude (nullable): int32 [nq], a gallery row that must not be returned for that query (-1: none) — leave-one-out
 * when the queries are gallery rows: k + 1 rows are selected, the named one removed where it is among them, the last one
 * otherwise.  Nothing is assumed to be "self".
 * Limits: D % 32 == 0, nq % 64 == 0, 64 <= N < 2^31, 1 <= k, k + (exclude ? 1 : 0) <= 64 (AVID_E_UNSUPPORTED otherwise).
 * fallbacks (nullable): as avid_cma_topk.  ws: avid_knn_workspace_bytes(N, nq, k) bytes (0 = unsupported arguments). */
size_t avid_knn_workspace_bytes(int64_t N, int nq, int k);
int avid_knn_search(int64_t N, int D, const float* gallery, const float* queries, int nq, int k, const int32_t* exclude,
                    int32_t* out_idx, float* out_sim, int32_t* fallbacks, void* ws, size_t ws_bytes,
                    avid_stream_t stream);
/* Similarity-weighted vote over the rows of avid_knn_search: scores[q][c] = sum over ranks j, in rank order, of
 * exp(sim[q][j] * inv_T) with gallery_labels[idx[q][j]] == c (fp32 [nq][n_classes]; a row or a label out of range takes no
 * part); pred5 int32 [nq][5]: the five best classes by (score descending, class ascending), padded with -1 when
 * n_classes < 5; with query_labels (nullable, int32 [nq]) first_match[q] = the smallest rank whose gallery label is the
 * query's, k if none (recall@r = first_match < r).  1 <= k <= 64, 1 <= n_classes <= 8192; labels int32 [N]. */
int avid_knn_vote(int nq, int k, const int32_t* idx, const float* sim, const int32_t* gallery_labels, int64_t N,
                  int n_classes, float inv_T, const int32_t* query_labels, float* scores, int32_t* pred5,
                  int32_t* first_match, avid_stream_t stream);

/* Multi-label ranking metrics (version >= 167) — rank_metrics.hip: per class c of scores [N][C] against targets [N][C]
 * (fp32, row-major; positive iff t >= 0.5; P positives, Nn negatives), scikit-learn's average_precision_score and
 * roc_auc_score in their counting forms — ties handled, no sort:
 *   ap[c]  = (1 / P) sum over positives i of TP_i / (TP_i + FP_i), TP_i / FP_i = the positives / negatives with score >=
 *            score_i; the sum runs in ascending sample index in double (a class with more than 256 positives: 256 at
 *            a time, those sums then in order)
 *   auc[c] = U2 / (2 P Nn), U2 = sum over positives of 2 #{neg < s_i} + #{neg == s_i} as int64, then one double division
 *   n_pos[c] = P (nullable)
 * ap = NaN if P == 0; auc = NaN if P == 0 or Nn == 0.  A NaN score ORs AVID_DEVERR_RANK_SCORE into err (nullable) and makes
 * that class's ap and auc NaN.  Plain float comparisons: -0.0 == +0.0, +-inf are scores like any other.  Any N >= 1, C >= 1
 * (N < 2^31 - 1024).  Work: P x N compares per class.  No atomics on any result: the same bits on every run.
 * ws: avid_rank_metrics_workspace_bytes(N, C) bytes, 8-byte aligned (0 = unsupported arguments). */
size_t avid_rank_metrics_workspace_bytes(int64_t N, int C);
int avid_rank_metrics(int64_t N, int C, const float* scores, const float* targets, double* ap, double* auc, int64_t* n_pos,
                      void* ws, size_t ws_bytes, int32_t* err, avid_stream_t stream);

/* Linear one-vs-all SVM on frozen features (version >= 173) — svm.hip: the passes of a full-batch solver of the L2-regularised
 * L2-loss primal (liblinear's, scikit-learn's LinearSVC default; ops.svm_fit is the solver) over x [N][F] fp32 row-major,
 * 1 <= N < 2^31 (N * F may pass 2^31: 64-bit offsets), any F >= 1, any C >= 1 (more than 64 classes: blocks of 64).
 * Products are exact fp32 (v_mfma_f32_32x32x2_f32); every result is one sum in an order fixed by (N, F, C): no atomics, the
 * same bits on every run, under every CU budget, and for a row of x whatever block of rows it is passed in.
 *   avid_svm_scores: z [N][C] = x . w^T + bias (w [C][F], bias [C] nullable).  One workgroup owns 64 rows x 64 classes and
 *     the whole reduction over F: element = (s0 + s1) + bias, s0 / s1 the fmaf chains over the features f with f % 4 in
 *     {0, 1} / {2, 3} in ascending f.  Also serves the Hessian-vector products (w = a direction) and prediction.
 *   avid_svm_xt: g [C][F] = d^T . x and gb [C] = column sums of d (nullable) for d [N][C].  Rows are cut into slices of 512
 *     (their count depends on N only); a slice's partial element is (s0 + s1) as above over its rows (row index % 4), the
 *     partial tiles go to ws and are added in slice order in double, rounded once.  gb: double sums, rows r % 4 == j of a
 *     slice in ascending order, j = 0..3 in order, slices in order, rounded once.
 *   avid_svm_hinge: with y = +1 where labels[i] == c else -1, cost_ic = y > 0 ? cost * pos_weight[c] : cost (pos_weight
 *     nullable), m = fma(-y, z, 1): xv == NULL: out = (y * m) * cost_ic where m > 0, else 0 (the hinge residual; the
 *     gradient is w - 2 x^T out); xv != NULL: out = cost_ic * xv where m > 0, else 0 (the active set applied to x . v).
 *   avid_svm_loss: out [K][C] double, out[k][c] = sum_i cost_ic max(0, 1 - y (z + 2^-k zd))^2 evaluated in double from the
 *     fp32 inputs, 1 <= K <= 16 (zd nullable when K == 1: the loss at z); rows in partial sums of 256 (in ws), then in order.
 * labels: int32 [N]; one outside [0, C) ORs AVID_DEVERR_SVM_LABEL into err (nullable) and counts as no class.
 * ws: avid_svm_workspace_bytes(N, F, C) bytes, 8-byte aligned, covers avid_svm_xt and avid_svm_loss (0 = unsupported
 * arguments).  Null pointers, shapes outside the limits and a short workspace are refused before any launch. */
size_t avid_svm_workspace_bytes(int64_t N, int F, int C);
int avid_svm_scores(int64_t N, int F, int C, const float* x, const float* w, const float* bias, float* z,
                    avid_stream_t stream);
int avid_svm_xt(int64_t N, int F, int C, const float* x, const float* d, float* g, float* gb, void* ws, size_t ws_bytes,
                avid_stream_t stream);
int avid_svm_hinge(int64_t N, int C, const float* z, const int32_t* labels, float cost, const float* pos_weight,
                   const float* xv, float* out, int32_t* err, avid_stream_t stream);
int avid_svm_loss(int64_t N, int C, int K, const float* z, const float* zd, const int32_t* labels, float cost,
                  const float* pos_weight, double* out, void* ws, size_t ws_bytes, int32_t* err, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer: torch.optim.Adam semantics (L2 weight decay folded into the gradient; bias-corrected)
 * over one flat fp32 buffer — utils/main_utils.py:250-261.
 * ---------------------------------------------------------------------------------------------- */
/* lr_dev (nullable): the learning rate is read from this device float instead of `lr` — a captured hipGraph
 * freezes by-value arguments, a scheduler then writes the device word (utils/main_utils.py:258 MultiStepLR). */
int avid_adam_flat(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                   const float* lr_dev, float grad_scale, avid_stream_t stream);
/* torch.optim.SGD semantics (utils/main_utils.py:242-248; dampening 0, L2 weight decay folded into the gradient) over
 * one flat fp32 buffer, in torch's single-tensor order with every product and sum rounded to fp32 on its own:
 *   d = g * grad_scale;  if (weight_decay != 0) d += weight_decay * p;
 *   if (momentum != 0) { buf = momentum * buf + d;  d = nesterov ? d + momentum * buf : buf; }   p -= lr * d
 * A zero-filled buf makes the first step torch's buf = clone(d): there is no step counter.  buf may be NULL exactly when
 * momentum == 0 (it is not touched then); nesterov needs momentum.  lr_dev as above.  Buffers 16-byte aligned. */
int avid_sgd_flat(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                  int nesterov, const float* lr_dev, float grad_scale, avid_stream_t stream);
/* dst[i] = a[i] + b[i] in fp32 over one flat buffer of n elements: what accumulates the gradients of the shards of a
 * virtual-rank step (parallel.TrainStep(virtual_ranks=R)) in rank order.  One rounding per element, no atomics, the same
 * bits whatever the launch geometry; inf / nan propagate as IEEE addition has them.  dst may be exactly a or exactly b
 * (in place); any other overlap of dst with an input, n <= 0 or a null pointer is AVID_E_BADARG.  16-byte vectors where
 * all three pointers are 16-byte aligned, a scalar path otherwise: any 4-byte aligned addresses are taken. */
int avid_grad_accum_flat(int64_t n, float* dst, const float* a, const float* b, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Step guard: skip a non-finite step, clip the gradient norm — decided on the device, obeyed by the
 * launches behind it without a host synchronisation (avid_hip/parallel.py: AdamStep(max_grad_norm=,
 * skip_nonfinite=)).  One 32-byte record in device memory per engine; zero it once.
 * ---------------------------------------------------------------------------------------------- */
typedef struct avid_step_guard {
    float   grad_norm;      /* grad_scale * sqrt(sum g^2): the norm of the AVERAGED gradient; inf / nan when not finite */
    float   clip_coef;      /* factor the optimizer applies; exactly 1.0f when nothing is clipped */
    int32_t skip;           /* 1: this step must leave no trace */
    int32_t reserved;
    int64_t skipped_total;  /* steps skipped since the record was zeroed */
    int64_t steps_total;    /* steps the record has judged */
} avid_step_guard;

/* Judge the flat gradient g[0, n): sum of squares in a fixed order (no floating-point atomics: the same bits run to run,
 * whatever the block scheduling), accumulated in double — the product of two floats is exact there, subnormal gradients
 * count — then the record is filled:
 *   grad_norm = (float)(sqrt(sum) * grad_scale)
 *   clip_coef = max_norm > 0 ? min(1, max_norm / (grad_norm + 1e-6f)) : 1.0f   (torch.nn.utils.clip_grad_norm_'s rule,
 *               evaluated in double from the stored grad_norm and rounded once)
 *   skip      = skip_nonfinite && !isfinite((float)sum);  on a skip clip_coef = 1.0f
 *   skipped_total += skip;  steps_total += 1
 * The sum is judged as a float: one that exceeds FLT_MAX from finite gradients (a single 3e19) counts as non-finite and
 * grad_norm is inf — torch's fp32 norm is inf there too.  With skip_nonfinite == 0 a non-finite gradient gives skip == 0
 * and an inf / nan grad_norm.  16-byte vector loads between a scalar head and tail: any 4-byte aligned g.  ws: device
 * scratch of avid_grad_guard_workspace_bytes(n) bytes, 8-byte aligned (so guard_dev).  n <= 0, a null pointer or a short
 * workspace is AVID_E_BADARG, before anything is launched. */
size_t avid_grad_guard_workspace_bytes(int64_t n);
int avid_grad_guard(int64_t n, const float* g, float grad_scale, float max_norm, int skip_nonfinite,
                    avid_step_guard* guard_dev, void* ws, size_t ws_bytes, avid_stream_t stream);
/* A second witness for the same record, behind avid_grad_guard: if any of x[0, n) is not finite, the record becomes a skip
 * (skip = 1, clip_coef = 1.0f, skipped_total advanced unless it was a skip already); a finite x changes nothing.  One block:
 * meant for a small buffer — the BatchNorm running statistics, which a non-finite activation poisons even where a ReLU
 * (max(NaN, 0) = 0) keeps it out of the gradient.  n <= 0 or a null pointer: AVID_E_BADARG. */
int avid_guard_nonfinite(int64_t n, const float* x, avid_step_guard* guard, avid_stream_t stream);
/* avid_adam_flat / avid_sgd_flat under a record: with guard->skip nothing is written (p, m, v, buf untouched); otherwise
 * the gradient term is (g * grad_scale) * guard->clip_coef, the two products rounded to fp32 one after the other, in that
 * order.  With clip_coef == 1.0f the results are the unguarded kernels', bit for bit. */
int avid_adam_flat_guarded(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                           float beta2, float eps, float weight_decay, int64_t step, const int64_t* step_dev,
                           const float* lr_dev, float grad_scale, const avid_step_guard* guard, avid_stream_t stream);
int avid_sgd_flat_guarded(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                          int nesterov, const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                          avid_stream_t stream);
/* avid_counter_add unless guard->skip: Adam's device step counter stands still on a skipped step. */
int avid_counter_add_unless(uint64_t* counter, uint64_t inc, const avid_step_guard* guard, avid_stream_t stream);
/* When guard->skip: dst[idx[r]][0, D) = saved[r][0, D) for r in [0, rows) (idx == NULL: row r itself, a flat copy);
 * nothing is written otherwise.  Every idx[r] must be a row of dst (the kernel does not know its height); duplicates
 * must carry the same saved row, as rows saved before one update do. */
int avid_guard_restore(int64_t rows, int64_t D, float* dst, const int64_t* idx, const float* saved,
                       const avid_step_guard* guard, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight averaging (EMA), fused into the optimizer launch — avid_hip/parallel.py: AdamStep(ema_decay=).
 * The rule, per element and in fp32 with the difference, the product and the sum each rounded on its own:
 *   e = e + w * (p_new - e)          (torch's unfused e + (p - e) * w; within one ulp of torch.lerp)
 *   w = (float)(1.0 - d), formed once per launch in double; d = decay, or with warmup
 *   d = min(decay, (1 + k) / (10 + k)), k = *updates_dev: the averaging updates applied before this one.
 * The kernels read k and never write it: the caller advances the counter once per applied step, behind every
 * launch of that step (avid_counter_add, or avid_counter_add_unless under a guard).
 * ---------------------------------------------------------------------------------------------- */
typedef struct avid_ema_desc {
    float*         ema;          /* the average: n floats laid out like p, 16-byte aligned */
    double         decay;        /* in [0, 1) */
    int            warmup;       /* nonzero: the warm-up rule above; needs updates_dev */
    const int64_t* updates_dev;  /* device counter k (nullable without warmup), 8-byte aligned */
} avid_ema_desc;
/* avid_adam_flat / avid_sgd_flat (guard == NULL) or their guarded forms (guard != NULL), then e[i] from the p[i] just
 * computed, in the same launch: p, m, v, buf come out with the bits of those entry points.  Under guard->skip nothing is
 * written, the average included.  n <= 0, a null or misaligned buffer, a decay outside [0, 1) or warmup without its
 * counter is AVID_E_BADARG, before anything is launched. */
int avid_adam_flat_ema(int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int64_t step, const int64_t* step_dev, const float* lr_dev,
                       float grad_scale, const avid_step_guard* guard, const avid_ema_desc* ema, avid_stream_t stream);
int avid_sgd_flat_ema(int64_t n, float* p, const float* g, float* buf, float lr, float momentum, float weight_decay,
                      int nesterov, const float* lr_dev, float grad_scale, const avid_step_guard* guard,
                      const avid_ema_desc* ema, avid_stream_t stream);
/* The same rule in a pass of its own over p as somebody else left it (the BatchNorm running statistics, a caller's own
 * optimizer).  guard: nullable; with guard->skip nothing is written.  e and p 16-byte aligned. */
int avid_ema_flat(int64_t n, float* e, const float* p, double decay, int warmup, const int64_t* updates_dev,
                  const avid_step_guard* guard, avid_stream_t stream);
/* a <-> b over n floats, in place: every element is read from both buffers and written to both by one thread.  16-byte
 * vectors where both pointers are 16-byte aligned, a scalar path otherwise (any 4-byte aligned addresses).  a == b or any
 * overlap of the two buffers, n <= 0 or a null pointer is AVID_E_BADARG. */
int avid_swap_flat(int64_t n, float* a, float* b, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Per-tensor hyper-parameters and trust ratios (LARS / LAMB) over the flat buffers — avid_hip/parallel.py:
 * AdamStep(param_rules=, optimizer="lars" / "lamb").  A segment table says, for every tensor of a flat fp32 buffer,
 * where it lies and which hyper-parameters it takes; elements outside every segment (the padding between tensors) are
 * neither read into a norm nor written.  The kernels deal CHUNKS of AVID_SEG_CHUNK floats to workgroups, never segments:
 * a host-built list says for every chunk which segment it belongs to, where it starts and how long it is.
 * ---------------------------------------------------------------------------------------------- */
#define AVID_SEG_CHUNK 4096
typedef struct avid_segment {
    int64_t offset;        /* first element; a multiple of 4 (16 bytes), not below the end of the segment before */
    int64_t numel;         /* > 0; offset + numel <= n of the call */
    float   lr_scale;      /* the segment's learning rate is the single fp32 product lr * lr_scale; finite */
    float   weight_decay;  /* finite */
    int32_t adapt;         /* 0 / 1: takes the trust ratio (LARS / LAMB); ignored by the plain table kernels */
    int32_t first_chunk;   /* index of its first chunk; it owns ceil(numel / AVID_SEG_CHUNK) consecutive ones */
} avid_segment;
typedef struct avid_seg_chunk {
    int64_t start;         /* first element: offset + k * AVID_SEG_CHUNK */
    int32_t len;           /* AVID_SEG_CHUNK, or what is left of the segment */
    int32_t seg;
} avid_seg_chunk;
typedef struct avid_segment_table {
    int32_t S, n_chunks;
    const avid_segment*   seg_host;    /* S records in host memory: validated on every call, before anything is launched */
    const avid_segment*   seg_dev;     /* the same S records in device memory (uploaded once), 8-byte aligned */
    const avid_seg_chunk* chunk_host;  /* n_chunks records, host and device alike */
    const avid_seg_chunk* chunk_dev;
} avid_segment_table;
/* Fill first_chunk of segs[0, S) and, unless chunks is NULL, chunks[0, cap) with the list the kernels expect; returns
 * the number of chunks, or AVID_E_BADARG (S <= 0, a null segs, a numel <= 0, cap too small).  Host only. */
int avid_segment_chunks(int32_t S, avid_segment* segs, avid_seg_chunk* chunks, int32_t cap);
/* Every entry point below validates the host copy of its table first and returns AVID_E_BADARG — the message names the
 * entry point, nothing is launched — for: S <= 0 or a null pointer; an offset that is negative or no multiple of 4;
 * segments that are not increasing or overlap; numel <= 0 or offset + numel > n; an lr_scale or weight_decay that is not
 * finite; adapt outside {0, 1}; a chunk list other than avid_segment_chunks' for these segments.
 *
 * Per-segment sums of squares: sums[2 s] = sum of x^2 over segment s, sums[2 s + 1] = the same of y (0.0 with y == NULL).
 * The rule of avid_grad_guard: every product exact in double, accumulated in double in a FIXED order — four accumulators
 * per thread over its vectors of a chunk, (a0 + a1) + (a2 + a3), the xor butterfly over the wave, the four waves left to
 * right: one double per chunk into ws; then a segment's chunk partials are added in index order, one chain per segment.  No atomics;
 * the same bits whatever the grid, the CU budget or the scheduling.  ws: avid_segment_sumsq_workspace_bytes(table), 8-byte
 * aligned (so sums).  guard (nullable): with guard->skip nothing is written to sums. */
size_t avid_segment_sumsq_workspace_bytes(const avid_segment_table* table);
int avid_segment_sumsq(const avid_segment_table* table, int64_t n, const float* x, const float* y, double* sums,
                       const avid_step_guard* guard, void* ws, size_t ws_bytes, avid_stream_t stream);
/* avid_sgd_flat with the segment's lr (lr * lr_scale, lr read from lr_dev when given) and weight_decay, and an optional
 * trust factor (LARS as the FAIR self-supervised code bases have it).  Per element, every product and sum rounded to fp32
 * on its own:
 *   d = g * grad_scale;  d = d * clip_coef (1.0f without a guard);  if (wd_s != 0) d = d + wd_s * p;
 *   d = q_s * d;  if (momentum != 0) { buf = momentum * buf + d;  d = nesterov ? d + momentum * buf : buf; }
 *   p = p - lr_s * d;  ema as avid_sgd_flat_ema
 * trust == NULL: q_s = 1 — with lr_scale 1 and one weight_decay the bits of avid_sgd_flat(_guarded, _ema).
 * trust != NULL (float[S] in device memory; needs ws of avid_segment_sumsq_workspace_bytes(table)): a norm pass in front of
 * the update — the sums of p^2 and of d^2, d as above up to the weight-decay term, by avid_segment_sumsq's rule — writes
 *   trust[s] = q_s = (float)(trust_coefficient * (sqrt(sum p^2) / sqrt(sum d^2)))  if adapt_s and both sums > 0, else 1.0f
 * (formed in double, rounded once), which the update then reads.  guard / ema: nullable; with guard->skip nothing is
 * written, trust included. */
int avid_sgd_flat_table(const avid_segment_table* table, int64_t n, float* p, const float* g, float* buf, float lr,
                        float momentum, int nesterov, const float* lr_dev, float grad_scale, float trust_coefficient,
                        float* trust, const avid_step_guard* guard, const avid_ema_desc* ema, void* ws, size_t ws_bytes,
                        avid_stream_t stream);
/* avid_adam_flat with the segment's lr and weight_decay: every element is computed as avid_adam_flat's 16-byte vector
 * loop computes it (a flat buffer whose n is a multiple of 4 has no other elements), step size (float)(lr_s / (1 - beta1^t))
 * formed as avid_adam_flat forms it in each of its three cases (by value, lr_dev, step_dev).  Under a guard with
 * clip_coef != 1.0f the gradient term is ((g * grad_scale) * clip_coef) + wd_s * p, each operation rounded on its own. */
int avid_adam_flat_table(const avid_segment_table* table, int64_t n, float* p, const float* g, float* m, float* v, float lr,
                         float beta1, float beta2, float eps, int64_t step, const int64_t* step_dev, const float* lr_dev,
                         float grad_scale, const avid_step_guard* guard, const avid_ema_desc* ema, avid_stream_t stream);
/* LAMB in two passes (g is never written).  With gt = (g * grad_scale) * clip_coef + 0.0f:
 *   pass 1:  m, v as avid_adam_flat(weight_decay = 0) leaves them (the same bits);
 *            u = (m * c1) / (sqrt(v) * c2 + eps) + wd_s * p, each operation rounded to fp32 on its own,
 *            c1 = (float)(1 / (1 - beta1^t)), c2 = (float)(1 / sqrt(1 - beta2^t));  the sums of p^2 and u^2 per segment
 *   finish:  trust[s] = r_s = (float)(sqrt(sum p^2) / sqrt(sum u^2))  if adapt_s and both sums > 0, else 1.0f
 *   pass 2:  u again from the new m and v (the same operations: the same bits);  p = p - (lr_s * r_s) * u;  ema
 * About 40 bytes per parameter against avid_adam_flat's 28.  trust: float[S] in device memory, required.  step / step_dev
 * / lr_dev as avid_adam_flat's; with guard->skip nothing is written. */
int avid_lamb_flat(const avid_segment_table* table, int64_t n, float* p, const float* g, float* m, float* v, float lr,
                   float beta1, float beta2, float eps, int64_t step, const int64_t* step_dev, const float* lr_dev,
                   float grad_scale, float* trust, const avid_step_guard* guard, const avid_ema_desc* ema, void* ws,
                   size_t ws_bytes, avid_stream_t stream);

/* Video clip front end: frames [B][T][H][W][3] uint8 (what the decoder / augmentation hands over)
 * -> out [B][3][T][H][W] fp32 = ((u / 255) - mean[c]) / std[c], the reference's ClipToTensor + Normalize
 * (utils/videotransforms/volume_transforms.py:14-66, tensor_transforms.py:13-37; datasets/preprocessing.py:45-48)
 * in the same fp32 operation order (bit-identical).  mean3 / std3: HOST pointers to 3 floats. */
int avid_clip_normalize(int B, int T, int H, int W, const uint8_t* frames, const float* mean3, const float* std3,
                        float* out, avid_stream_t stream);

/* Clip augmentation on the GPU: the reference's per-frame PIL chain (datasets/preprocessing.py:15-113 through
 * utils/videotransforms/video_transforms.py) for a ragged batch of decoded clips, bit-identical to Pillow:
 *   crop box (i, j, h, w) of the source -> Pillow's two-pass BILINEAR resize to RH x RW (horizontal first, rounded to uint8)
 *   -> window (y1, x1, ch, cw) of that image -> optional horizontal flip -> nops colour operations in the given order
 *   (ImageEnhance.Brightness / Color / Contrast = Image.blend in unfused fp32; torchvision's hue shift through Pillow's
 *   RGB <-> HSV) -> ((u / 255) - mean) / std as avid_clip_normalize.  Output frame t reads source frame t % T.
 * One descriptor per clip; frames: DEVICE pointer to uint8 [T][H][W][3]; factor[k] belongs to ops[k]. */
enum { AVID_AUG_BRIGHTNESS = 0, AVID_AUG_SATURATION = 1, AVID_AUG_HUE = 2, AVID_AUG_CONTRAST = 3 };
typedef struct avid_aug_desc {
  const uint8_t* frames;
  double factor[4];
  int32_t T, H, W;
  int32_t i, j, h, w;
  int32_t RH, RW;
  int32_t y1, x1;
  int32_t flip;
  int32_t nops, ops[4];
  int32_t reserved;
} avid_aug_desc;
/* descs: HOST array of B descriptors; out [B][3][num_frames][ch][cw] fp32; mean3 / std3: HOST pointers to 3 floats.
 * The resample tables are built on the host in double, staged in pinned memory and copied into ws on the stream (no host
 * synchronisation); ws also holds the uint8 intermediate and the per-frame grey sums of the clips that use contrast. */
size_t avid_clip_augment_workspace_bytes(int B, const avid_aug_desc* descs, int num_frames, int ch, int cw);
int avid_clip_augment(int B, const avid_aug_desc* descs, int num_frames, int ch, int cw, const float* mean3,
                      const float* std3, float* out, void* ws, size_t ws_bytes, avid_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Audio front end on the GPU — datasets/preprocessing.py:158-186 LogSpectrogram:
 * out[b][0][t][f] = z-score( top_db-floored dB( bin-pair mean( |STFT(sig[b])|^2 ) ) ), STFT = librosa.stft
 * defaults (centred / reflect-padded frames, periodic Hann, n_stft = 2 * n_fft, hop samples).
 * sig [B][L] mono fp32; out [B][1][T][n_stft/4 + 1], T <= 1 + L/hop (the reference truncates to
 * int(duration * rate) frames before the dB floor).  basis: avid_logspec_basis_floats(n_stft) floats filled
 * once by avid_logspec_basis.  mean / std: [n_stft/4 + 1] or both NULL.
 * ---------------------------------------------------------------------------------------------- */
size_t avid_logspec_basis_floats(int n_stft);
int avid_logspec_basis(int n_stft, float* basis, avid_stream_t stream);
size_t avid_logspec_workspace_bytes(int B, int n_stft, int T);
int avid_logspec(int B, int L, const float* sig, int n_stft, int hop, int T, const float* basis,
                 const float* mean, const float* std, float top_db, float* out, void* ws, size_t ws_bytes,
                 avid_stream_t stream);

/* The same front end from the decoder's samples: the reference's AudioPrep (datasets/preprocessing.py:116-155: downmix, trim /
 * zero-pad to L samples, volume jitter) for a ragged batch of int16 clips, bit for bit.  One descriptor per clip; samples:
 * DEVICE pointer to planar int16 [channels][n], 2-byte aligned (clips may be views into one packed upload); 1 <= channels <= 8;
 * n == 0 is a missing clip (samples may then be NULL); gain: the float32 the waveform is multiplied by, 1.0f when not
 * augmenting.  The prepared sample p of a clip, 0 <= p < L:
 *     p <  n:  (float)((s[0][p] / 32767.0 + s[1][p] / 32767.0 + ...) / channels)   summed in channel order, in double
 *     p >= n:  0.0f
 *     then one float32 multiply by gain
 * (numpy's arithmetic for  data / np.iinfo(int16).max -> .mean(0).astype(float32) -> np.pad -> sig *= float).
 * descs: HOST array of B descriptors, checked before anything is launched (an error names the clip), then copied into ws on
 * the stream through pinned staging (no host synchronisation).
 * avid_audio_prep: out [B][L] fp32.  avid_logspec_pcm: avid_logspec of that waveform (same arguments and checks, bit-identical
 * output) with the frame matrix filled straight from the clips: no waveform is written. */
typedef struct avid_pcm_desc {
  const int16_t* samples;
  int32_t channels;
  int32_t n;
  float gain;
} avid_pcm_desc;
size_t avid_audio_prep_workspace_bytes(int B);
int avid_audio_prep(int B, const avid_pcm_desc* descs, int L, float* out, void* ws, size_t ws_bytes, avid_stream_t stream);
size_t avid_logspec_pcm_workspace_bytes(int B, int n_stft, int T);
int avid_logspec_pcm(int B, const avid_pcm_desc* descs, int L, int n_stft, int hop, int T, const float* basis,
                     const float* mean, const float* std, float top_db, float* out, void* ws, size_t ws_bytes,
                     avid_stream_t stream);


/* ------------------------------------------------------------------------------------------------
 * Collectives: NOT part of this library.  SURVEY.md 8(b) sketched avid_comm_init / avid_allreduce_f32 /
 * avid_allgather_bytes / avid_broadcast; they were deliberately not built.  The reference itself speaks to
 * torch.distributed (utils/distributed_utils.py:12-19, utils/main_utils.py:105-117: DistributedDataParallel;
 * criterions/avid.py:99-111, criterions/nce.py:27-33), whose "nccl" backend IS RCCL on ROCm — a second communicator
 * behind this ABI would duplicate rendezvous, error handling and the process group the driver already owns.
 * What the step needs from the collectives' side lives in the binding: avid-cma_amd/avid_hip/parallel.py (bucketed
 * all-reduce over one flat gradient buffer issued on a placed stream, one fused bank all-gather, one flat buffer
 * broadcast), with avid_stream_wait / avid_probe_spin below as the only native pieces (stream ordering and placement).
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * Launch programs: the host side of a whole forward / backward pass as ONE call.
 *
 * The reference drives its step from Python, one ATen call per layer (main-avid.py:155-180 ->
 * models/av_wrapper.py:50-61 -> models/video.py:44-54, models/audio.py:33-44, models/network_blocks.py:23-27,
 * 52-60, and autograd's mirror image of that for loss.backward()).  A binding that does the same with the
 * entry points above issues ~330 launches per step through its interpreter.  A program is that launch
 * sequence compiled once per (model, input shape): an array of avid_instr records — opcode, stream index,
 * geometry, tensor references — that avid_program_run() walks, calling the SAME entry points above with the
 * SAME arguments (results are bit-identical to issuing the calls one by one), plus the cross-stream
 * dependencies (AVID_OP_WAIT) that keep the four-stream arrangement of the step (two towers, each with a
 * trailing weight-gradient stream).
 *
 * A tensor reference is (slot, byte offset): slots[] is an array of base pointers the caller fills for each
 * run (activation arenas, the parameter / gradient / BatchNorm-buffer tensors, the inputs), so the compiled
 * program never holds an address and the caller's allocator stays in charge.  slot < 0 = NULL.
 * The program owns nothing on the device; the only state of the executor is a pool of hipEvents for the waits.
 * ---------------------------------------------------------------------------------------------- */
typedef struct avid_ref {
  int32_t slot;
  int32_t reserved;
  int64_t off;
} avid_ref;

enum {
  AVID_OP_NOP = 0,
  AVID_OP_WAIT = 1,          /* stream i[0] waits for everything issued so far on stream i[1] (event record + wait) */
  AVID_OP_MEMSET0 = 2,       /* t0 <- zeros, n[0] bytes */
  AVID_OP_CONV_FWD = 3,      /* d; t: x w u addend bias y bn_partials [in_s4]; i0 relu, i1 input BatchNorm (0 none, 1 affine, 2 + ReLU:
                                x is then that BatchNorm's input and t7 its saved [4][C] vectors, i2 = C: avid_conv_fwd_in);
                                inference programs: [... out_s4], i3 output BatchNorm (0 none, 1 affine, 2 + ReLU: t8 = the eval-mode
                                BatchNorm's [4][Cout] vectors, y its OUTPUT: avid_conv_fwd_out) */
  AVID_OP_CONV_DGRAD = 4,    /* d; t: dy w wt u addend dx bn.x bn.scale bn.shift bn.mean bn.invstd bn.partials;
                                i0..2 addend strides (0 = dense addend), i3 bn.relu, i4 bn present */
  AVID_OP_CONV_WGRAD = 5,    /* d; t: x dy dw [in_s4]; i0 input BatchNorm as AVID_OP_CONV_FWD's i1 (t3, i1 = C: avid_conv_wgrad_in) */
  AVID_OP_WGRAD_GROUP = 6,   /* i0 = n, followed by n AVID_OP_WGRAD_ITEM records (d; t: x dy dw) */
  AVID_OP_WGRAD_ITEM = 7,
  AVID_OP_BN_FWD = 8,        /* n0 M; i0 C, i1 relu, i2 nparts; f0 momentum, f1 eps;
                                t: x gamma beta running_mean running_var y save4 counter partials
                                (save4 = mean | invstd | scale | shift, C floats each) */
  AVID_OP_BN_BWD = 9,        /* n0 M; i0 C, i1 relu, i2 nparts, i3 frozen; t: x dy gamma save4 dx dgamma dbeta partials */
  AVID_OP_BN_POOL_FWD = 10,  /* i0..4 B T H W C, i5 nparts; f0 momentum, f1 eps;
                                t: x gamma beta running_mean running_var y argmax save4 counter partials */
  AVID_OP_BN_POOL_BWD = 11,  /* i0..4 B T H W C; t: x dy argmax gamma save4 dx dgamma dbeta */
  AVID_OP_GPOOL_FWD = 12,    /* i0 B, i1 S, i2 C; t: x y argmax */
  AVID_OP_GPOOL_BWD = 13,    /* i0 B, i1 S, i2 C; t: dy argmax dx */
  AVID_OP_RELU_BWD = 14,     /* n0 elements; t: y dy dx */
  AVID_OP_COLSUM = 15,       /* n0 M; i0 C; t: x out */
  AVID_OP_WT_BATCH = 16,     /* i0 descriptors, n0 max_elems; t: table (avid_wt_desc[] in device memory) */
  AVID_OP_ADAM = 17,         /* n0 elements; f0 lr, f1 beta1, f2 beta2, f3 eps, f4 weight_decay, f5 grad_scale; n1 step;
                                t: p g m v step_dev lr_dev (step_dev, if given, is advanced by one first) */
  AVID_OP_DROPOUT_FWD = 18,  /* n0 B, n1 offset; i0 F, i1 seed lo, i2 seed hi; f0 p; t: x y mask offset_dev */
  AVID_OP_DROPOUT_BWD = 19,  /* n0 elements; f0 p; t: mask dy dx */
  AVID_OP_CLS_LOSS = 20,     /* i0 V, i1 clips, i2 C; f0 grad_scale; t: logits labels loss conf hits dlogits err */
  AVID_OP_CLS_LINEAR_FWD = 21, /* i0 B, i1 Fin, i2 C; t: x w bias y */
  AVID_OP_CLS_LINEAR_BWD = 22, /* i0 B, i1 Fin, i2 C; t: x w dy dx dw db */
  AVID_OP_ADAPTIVE_MAXPOOL = 23, /* i0..4 B T H W C; d.To d.Ho d.Wo the output size; t: x y */
  AVID_OP_BN1D_FWD = 24,      /* i0 B, i1 F, i2 training; f0 momentum, f1 eps; t: x gamma beta running_mean running_var y save2 counter */
  AVID_OP_BN1D_BWD = 25,      /* i0 B, i1 F, i2 frozen; f1 eps; t: x dy gamma save2 dx dgamma dbeta */
  AVID_OP_PROBE_LINEAR_FWD = 26, /* i0 B, i1 Fin, i2 C; t: x w bias y */
  AVID_OP_PROBE_LINEAR_BWD = 27, /* i0 B, i1 Fin, i2 C; t: x w dy dx dw db */
  /* inference programs (version >= 160); no training program holds a record of these kinds */
  AVID_OP_BN_EVAL_COEFFS = 28,   /* i0 n; t: table (avid_bn_eval_item[] in device memory): avid_bn_eval_coeffs_batched */
  AVID_OP_BN_EVAL_APPLY = 29,    /* n0 M; i0 C, i1 relu; t: x coeffs4 y (coeffs4 = mean | invstd | scale | shift): avid_bn_apply_eval */
  AVID_OP_BN_POOL_FWD_EVAL = 30, /* i0..4 B T H W C; t: x coeffs4 y: avid_bn_relu_maxpool_fwd_eval */
  AVID_OP_BN_EVAL_DIRECT = 31,   /* n0 M; i0 C, i1 relu; f1 eps; t: x gamma beta running_mean running_var y: avid_bn_fwd_eval WITHOUT save4 —
                                    what the per-layer path calls for a BatchNorm whose parameters take no gradient (another expression
                                    than fma(x, scale, shift): such a BatchNorm is never fused) */
  AVID_OP_MAXPOOL_FWD = 32,      /* i0..4 B T H W C; t: x y argmax: avid_maxpool_hw3s2_fwd (the stem's pool behind such a BatchNorm) */
  /* multi-label fine-tuning / probing (version >= 167) */
  AVID_OP_MLABEL_LOSS = 33,      /* i0 V, i1 clips, i2 C; f0 grad_scale; t: logits targets pos_weight loss conf hits dlogits err */
  /* soft-target fine-tuning / probing: label smoothing, mixup / CutMix targets (version >= 168) */
  AVID_OP_SOFT_CE_LOSS = 34,     /* i0 V, i1 clips, i2 C; f0 grad_scale, f1 label_smoothing; t: logits targets loss conf hits dlogits err */
  AVID_OP_COUNT_
};

#define AVID_INSTR_REFS 12
typedef struct avid_instr {
  int32_t op;
  int32_t stream; /* index into the run's stream table (ignored by AVID_OP_WAIT) */
  int32_t mark;   /* free for the caller (segment labels) */
  int32_t reserved;
  avid_conv_desc d;
  int32_t i[6];
  int64_t n[2];
  float f[6];
  avid_ref t[AVID_INSTR_REFS];
} avid_instr;

/* Scratch of one stream of a run (what the *_workspace_bytes queries ask for, maximum over the stream's records). */
typedef struct avid_stream_ws {
  void* ptr;
  size_t bytes;
} avid_stream_ws;

/* One single-wave kernel that spins for about `us` microseconds on `stream`: the probe with which a binding finds out
 * which of its streams the hardware serialises (streams that share a hardware queue, or queues that share a dispatch
 * pipe: 4 pipes serve GPU_MAX_HW_QUEUES queues) before it places the step's four streams — avid_hip/streams.py. */
int avid_probe_spin(int us, avid_stream_t stream);
/* The shader clock while other work runs: one wave on `stream` spins for `us` microseconds of the constant 100 MHz clock
 * and writes out2[0] = shader-clock cycles elapsed (s_memtime), out2[1] = 100 MHz ticks elapsed (device int64 x 2):
 * GHz = out2[0] / out2[1] / 10.  bench.py runs it beside the timed region (roofline.shader_clock_ghz). */
int avid_clock_probe(int us, long long* out2, avid_stream_t stream);
/* Everything issued to `waiter` after this call runs behind everything issued to `waited` before it (one event of the
 * executor's pool: record + wait) — what AVID_OP_WAIT does inside a program, for a binding that orders its collectives'
 * stream behind the streams that produced a gradient bucket.
 * The event pool's contract: 64 events per device, drawn round-robin through an atomic index by avid_stream_wait and by
 * every AVID_OP_WAIT record (the forward's thread and autograd's backward thread may both draw).  An event is re-recorded
 * after 64 further draws whether or not the GPU has passed the earlier wait: that is safe because hipStreamWaitEvent
 * captures the record that is current WHEN IT IS CALLED (a later hipEventRecord on the same event does not move an
 * earlier wait), and the pair record + wait is issued back to back on the calling thread.  It would NOT be safe for a
 * caller to keep an event of its own across calls, and none is handed out.  Under a stream capture the same pair
 * becomes a graph dependency. */
int avid_stream_wait(avid_stream_t waiter, avid_stream_t waited);
/* sizeof(avid_instr) as the library was compiled: a binding checks its mirror of the record against it. */
size_t avid_program_instr_bytes(void);
/* Scratch bytes records [begin, end) need on each of n_streams streams (out_bytes[n_streams]). */
int avid_program_workspace_bytes(const avid_instr* prog, int begin, int end, int n_streams, size_t* out_bytes);
/* Issue records [begin, end) of prog.  streams[n_streams]: hipStream_t handles, ws[n_streams]: their scratch.
 * Asynchronous like every other entry point.  On error the message names the failing record. */
int avid_program_run(const avid_instr* prog, int begin, int end, void* const* slots, int n_slots,
                     const avid_stream_t* streams, const avid_stream_ws* ws, int n_streams);

#ifdef __cplusplus
}
#endif
#endif /* AVID_HIP_H */
