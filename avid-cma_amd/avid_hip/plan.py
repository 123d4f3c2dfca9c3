"""Launch programs for the two-tower model: the whole forward / backward pass of ``AV_Wrapper`` as ONE C call each.

The reference drives its step from Python, one ATen call per layer (main-avid.py:167,179 -> models/av_wrapper.py:50-61
-> models/video.py:44-54, models/audio.py:33-44, models/network_blocks.py:23-27,52-60).  Doing the same with this
library's entry points (``avid_hip.ops``: one ``torch.autograd.Function`` per layer) costs ~330 launches per step through
the interpreter — 7.7 ms of host time against 11.2 ms of GPU time in round 3, and the reference's own loop, which
synchronises on ``loss.item()`` every step, saw all of it.  Here the launch sequence is COMPILED once per (model, input
shape, stream arrangement) into an ``avid_instr`` array (include/avid_hip.h, "Launch programs") and executed by
``avid_program_run`` in C: same entry points, same arguments, same order per stream as the per-layer path — bit-identical
results (tests/test_gpu_plan.py) — and the whole model is one autograd node.

* ``Builder`` walks the module tree (R2Plus1D / Conv2D / Head, i.e. models/*.py of this package) ONCE for every kind of
  program: ``video_fwd`` / ``audio_fwd`` / ``head_fwd`` call the per-mode layer emitters (``stem_fwd``, ``conv_bn_fwd``,
  ``r2p1d_block_fwd``) of ``TrainBuilder`` (training-mode BatchNorm, everything kept for the backward) or ``EvalBuilder``
  (running statistics, a recycled arena).  ``TrainBuilder`` then emits the backward records in autograd's order, with every
  fusion decision of the per-layer path taken at compile time: BatchNorm statistics from the convolution epilogue,
  BatchNorm-backward sums from the consumer's input-gradient kernel, residual add in the epilogue, compact gradient of the
  strided 1x1x1 residual convolution, grouped weight gradients, weight gradients on trailing streams, the audio tower on
  its own stream.
* ``Programs`` seals what a builder emitted (weight-transform table, record arrays, workspaces, slots) and runs it;
  ``TrainPrograms`` adds the forward / backward pair over a flat gradient buffer (``Plan``, ``ClsPlan``, ``ProbePlan``),
  ``EvalPlan`` is a single forward program.
* tensors are ``(slot, byte offset)`` references: activations live in ONE arena per pass (a torch tensor the autograd
  node keeps alive), parameters / buffers / inputs are slots re-read from the tensors on every run — the program holds
  no address, so re-seated parameters (``FlatParams``), a new batch or a different allocator block just work.
* ``NetFn`` is the autograd node; parameter gradients go straight into a flat gradient buffer (the step engine's, or a
  fresh one whose slices are handed to autograd so that ``torch.optim.Adam`` / DDP see ordinary ``.grad`` tensors).
"""
from __future__ import annotations

import ctypes as C
import os
import struct

import torch

from . import lib, ops
from .lib import ConvDesc

# ---- ctypes mirrors of include/avid_hip.h ------------------------------------------------------------------------
OP_WAIT, OP_MEMSET0, OP_CONV_FWD, OP_CONV_DGRAD, OP_CONV_WGRAD, OP_WGRAD_GROUP, OP_WGRAD_ITEM = 1, 2, 3, 4, 5, 6, 7
OP_BN_FWD, OP_BN_BWD, OP_BN_POOL_FWD, OP_BN_POOL_BWD, OP_GPOOL_FWD, OP_GPOOL_BWD = 8, 9, 10, 11, 12, 13
OP_RELU_BWD, OP_COLSUM, OP_WT_BATCH, OP_ADAM = 14, 15, 16, 17
OP_DROPOUT_FWD, OP_DROPOUT_BWD, OP_CLS_LOSS, OP_CLS_LINEAR_FWD, OP_CLS_LINEAR_BWD = 18, 19, 20, 21, 22
OP_ADAPTIVE_MAXPOOL, OP_BN1D_FWD, OP_BN1D_BWD, OP_PROBE_LINEAR_FWD, OP_PROBE_LINEAR_BWD = 23, 24, 25, 26, 27
OP_BN_EVAL_COEFFS, OP_BN_EVAL_APPLY, OP_BN_POOL_FWD_EVAL, OP_BN_EVAL_DIRECT, OP_MAXPOOL_FWD = 28, 29, 30, 31, 32   # inference programs only
OP_MLABEL_LOSS = 33                                  # the "bce" plans' loss record
OP_SOFT_CE_LOSS = 34                                 # the "soft_ce" plans' loss record
_OP_NAMES = {0: "nop", **{v: k[3:].lower() for k, v in list(globals().items()) if k.startswith("OP_")}}   # (``dump``)
NREF = lib.INSTR_REFS
Ref, Instr, StreamWs = lib.Ref, lib.Instr, lib.StreamWs
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t

# ---- slots ---------------------------------------------------------------------------------------------------------
S_FWD, S_BWD, S_GRAD, S_AUX, S_VIDEO, S_AUDIO, S_DV, S_DA, S_FIRST_TENSOR = 0, 1, 2, 3, 4, 5, 6, 7, 8
S_LABELS, S_DLOGITS, S_OUT = S_AUDIO, S_DV, S_DA     # the single-tower plans' use of the two-tower plan's input slots
OUT_BYTES = 32                                       # S_OUT of a classifier step: loss (f32) at 0, hits (2 x i64) at 8
PROBE_OUT_BYTES = 32                                 # the same per tap of a probe step
NULL = (-1, 0)
# streams of a run (avid_hip/streams.py: one per dispatch pipe): compute (video tower), audio tower, the trailing
# weight-gradient stream of both, the collectives' stream (not used by the programs themselves)
ST_MAIN, ST_AUDIO, ST_TRAIL, ST_COMM = 0, 1, 2, 3

ENABLED = os.environ.get("AVID_PLAN", "1") == "1"
EVAL_ENABLED = os.environ.get("AVID_EVAL_PLAN", "1") != "0"      # 0: parallel.Inference always takes the per-layer path


class Unsupported(Exception):
    """The module tree holds something the compiler does not know: the caller falls back to the per-layer path."""


def _align(n, a=256):
    return (n + a - 1) // a * a


class Arena:
    """Bump allocator of one pass (no reuse: a trailing weight gradient may still read a tensor long after the chain
    has moved on, and 288 GB of HBM hold the ~3 GB per pass of a 64-clip batch many times over)."""

    def __init__(self, slot):
        self.slot, self.size = slot, 0

    def alloc(self, nbytes):
        off = self.size
        self.size += _align(max(int(nbytes), 4))
        return (self.slot, off)


class EvalArena:
    """The activation arena of an inference program while it is compiled: ``alloc`` hands out VIRTUAL offsets that never
    overlap; ``EvalPlan._recycle`` then maps every buffer to a physical offset, re-using the bytes of buffers whose last
    reader has been emitted on the same stream (nothing runs backward, nothing trails on another stream)."""

    def __init__(self, slot):
        self.slot, self.size, self.bufs = slot, 0, []

    def alloc(self, nbytes):
        off, n = self.size, _align(max(int(nbytes), 4))
        self.size += n
        self.bufs.append((off, n))
        return (self.slot, off)


class Sym:
    """A tensor known to the compiler: reference, channels-last shape, and — for the output of a training-mode
    BatchNorm(+ReLU) whose only consumer is the next convolution — that BatchNorm's record (``ops.BnSource``)."""
    __slots__ = ("ref", "shape", "bn", "affine")

    def __init__(self, ref, shape, bn=None, affine=None):
        """``affine`` = (reference of the BatchNorm's saved [4][C] vectors, relu, C): ``ref`` is then the BatchNorm's INPUT and
        the tensor this Sym stands for — ReLU(bn(ref)) — exists nowhere: its consumers apply the map themselves
        (OP_CONV_FWD's i1 / OP_CONV_WGRAD's i0)."""
        self.ref, self.shape, self.bn, self.affine = ref, tuple(shape), bn, affine

    @property
    def numel(self):
        n = 1
        for v in self.shape:
            n *= v
        return n


class BnRec:
    __slots__ = ("x", "s4", "relu", "C", "partials", "rows")

    def __init__(self, x, s4, relu, Cc):
        self.x, self.s4, self.relu, self.C, self.partials, self.rows = x, s4, relu, Cc, None, 0


def _off(ref, nbytes):
    return (ref[0], ref[1] + nbytes)


_STAGES = ("conv2x", "conv3x", "conv4x", "conv5x")   # R2Plus1D's stages: the linear probe's taps


def _classifier(model):
    """The classifier of a ``ClassificationWrapper`` in the compiled pattern: pooled features -> [dropout ->] ``ClsLinear``."""
    from models.classification import ClassificationWrapper, ClsLinear
    if type(model) is not ClassificationWrapper or model.feat_name != "pool" or model.pooling is not None:
        raise Unsupported("classification wrapper outside the compiled pattern")
    if type(model.classifier) is not ClsLinear:
        raise Unsupported("classifier")
    return model.classifier


def _audio_tower(model):
    """The model's single tower — the model itself, or the ``feature_extractor`` of a wrapper — is this package's ``Conv2D``: its
    input is a spectrogram batch [B, 1, T, F] (in slot ``S_VIDEO``, as every single-tower plan's input), its taps are 2-D."""
    from models.audio import Conv2D
    return type(getattr(model, "feature_extractor", model)) is Conv2D


def _tower_input(tower_is_audio, shape):
    """The Sym of a single-tower plan's input in slot ``S_VIDEO``: a clip batch [B, 3, T, H, W] as it is, a spectrogram batch
    [B, 1, T, F] as [B, 1, 1, T, F] (a 2-D convolution is a 3-D one with T = kt = 1, as the two-tower plan builds it)."""
    if len(shape) != (4 if tower_is_audio else 5):
        raise Unsupported("input rank")
    if not tower_is_audio:
        return Sym((S_VIDEO, 0), shape)
    return Sym((S_VIDEO, 0), (shape[0], shape[1], 1, shape[2], shape[3]))


def _probe_heads(model):
    """The heads of a ``MOSTModel`` in its stock form: per tap adaptive max pool -> BatchNorm1d -> Linear, no dropout, no l2 norm.
    The pool is an ``AdaptiveMaxPool3d((t, h, w))`` on an ``R2Plus1D`` tower and an ``AdaptiveMaxPool2d((h, w))`` on a ``Conv2D``
    tower (``pool_size`` (1, h, w)); the other pairing — whose torch module would refuse the tap's rank — is not compiled."""
    from models.linear_probe import MOSTModel, Classifier, ProbeBatchNorm1d, ProbeLinear
    if type(model) is not MOSTModel or not len(model.classifiers):
        raise Unsupported("linear probe outside the compiled pattern")
    pool_type = torch.nn.AdaptiveMaxPool2d if _audio_tower(model) else torch.nn.AdaptiveMaxPool3d
    for c in model.classifiers:
        if (type(c) is not Classifier or c.pool_size is None or c.use_dropout or c.l2_norm or not c.use_bn
                or type(c.pooling) is not pool_type or c.feat_name not in _STAGES
                or type(c.bn) is not ProbeBatchNorm1d or c.bn.momentum is None or not c.bn.affine
                or not c.bn.track_running_stats or type(c.classifier) is not ProbeLinear or c.classifier.bias is None):
            raise Unsupported("probe head outside the compiled pattern")
    if list(model.feat_names) != [c.feat_name for c in model.classifiers]:
        raise Unsupported("feat_names")
    return list(model.classifiers)


class Builder:
    """What every compiler shares: the forward records, the references of external tensors, the weight-transform table, the
    emitters that do not depend on the BatchNorm mode (linear, pools, the classifier and probe heads) and the MODULE WALKERS —
    ``video_fwd``, ``audio_fwd``, ``head_fwd`` — which decide what the compiler accepts and call the mode's layer emitters:

    * ``stem_fwd(w, bn, x, d, srows, psh)`` -> (stem record, reference of the pooled output [psh]),
    * ``conv_bn_fwd(conv, bn, x, addend=None, next_conv=None, ...)`` -> layer record with at least ``"h"``,
    * ``r2p1d_block_fwd(blk, x)`` -> (the block's layer records, Sym of its output)."""

    trailing = False                               # (TrainBuilder: weight gradients and weight tables on the trailing stream)

    def __init__(self, device, arena):
        self.device = device
        self.fa = arena
        self.fwd = []
        self.cur = self.fwd
        self.tensors, self.tslot = [], {}          # external tensors (parameters, buffers) -> slot
        self.S = ST_MAIN                           # compute stream of the records being emitted
        self.tables_waited = set()                 # streams whose forward has waited for the weight-transform launch
        self.wt_off = {}                           # transposed weights / Winograd transforms: (id(param), mode) -> aux offset
        self.aux_size = 0
        self.wt_recs = []                          # (param tensor, aux offset, Cout, taps, Cin, mode)

    # ---- references
    def ext(self, t):
        """Slot of an external tensor (parameter / buffer), registered on first use."""
        key = id(t)
        s = self.tslot.get(key)
        if s is None:
            s = self.tslot[key] = S_FIRST_TENSOR + len(self.tensors)
            self.tensors.append(t)
        return (s, 0)

    def emit(self, op, stream=None, d=None, i=(), n=(), f=(), t=()):
        ins = Instr()
        ins.op = op
        ins.stream = self.S if stream is None else stream
        if d is not None:
            ins.d = d
        for k, v in enumerate(i):
            ins.i[k] = int(v)
        for k, v in enumerate(n):
            ins.n[k] = int(v)
        for k, v in enumerate(f):
            ins.f[k] = float(v)
        for k in range(NREF):
            r = t[k] if k < len(t) else NULL
            if r is None:
                r = NULL
            ins.t[k].slot, ins.t[k].off = int(r[0]), int(r[1])
        self.cur.append(ins)
        return ins

    def wait(self, waiter, waited):
        if waiter != waited:
            self.emit(OP_WAIT, stream=0, i=(waiter, waited))

    # ---- transposed weights / Winograd transforms / pre-split weights (ops.TransposedWeights): one table entry per form
    def _want(self, w, mode, taps, nbytes):
        key = (id(w), mode)
        if key not in self.wt_off:
            self.wt_off[key] = self.aux_size
            self.wt_recs.append((w, self.aux_size, w.shape[0], taps, w.shape[1], mode))
            self.aux_size += _align(nbytes)
        return (S_AUX, self.wt_off[key])

    def want_wt(self, w):
        if not (w.shape[1] % 64 == 0 and w.shape[0] % 32 == 0):
            return None
        k = ops._kdims(w)
        return self._want(w, 0, k[0] * k[1] * k[2], 4 * w.numel())

    def want_u(self, w, variant, forward=False):
        code = (1 if forward else 2) + 2 * (variant - 1)   # forward (1 / 3) or input gradient (2 / 4), wino_kernel's / wino2_kernel's order
        return self._want(w, code, 9, 4 * ops.U_FLOATS * w.shape[0] * w.shape[1])

    def want_split(self, w, mode):
        """The weights pre-split into bf16 terms for igemm_pk_kernel's 128 x 64 tile (mode 5: forward, 6: input gradient)."""
        k = ops._kdims(w)
        return self._want(w, mode, k[0] * k[1] * k[2], 6 * w.numel())

    def fwd_u(self, w, d):
        """`u` of a forward convolution on stream self.S.  The pre-split weights (want_split mode 5) come out of the step's
        weight-transform launch on the trailing stream, which is issued beside the video stem and starves behind its
        persistent workgroups (parallel.py: forward_backward): the FIRST layer of a stream that reads a table waits for
        that launch — on the video tower that is conv2x's temporal convolution, 0.2 ms behind the stem, and costs nothing;
        a wait right behind the stem stalled the compute stream for the time the tables were late (10.07-10.3 against
        10.03-10.09 ms per step on one box).  (An inference program has no trailing stream: its tables come out of record 1.)"""
        if d.wino_fwd:
            # a Winograd layer behind that wait takes its transformed weights from the same launch (mode 1 / 3) instead of
            # transforming them in front of its own kernel (one 6 us launch per layer on the compute stream); the first
            # one of the video tower sits right behind the stem and keeps its own
            if self.trailing and self.S in self.tables_waited:
                return self.want_u(w, d.wino_fwd, forward=True)
            return None
        if not d.split_fwd:
            return None
        if self.trailing and self.S not in self.tables_waited:
            self.wait(self.S, ST_TRAIL)
            self.tables_waited.add(self.S)
        return self.want_split(w, 5)

    # ---- forward emitters of both modes ----------------------------------------------------------------------------
    def desc(self, x_shape, conv_w, stride, pad, channel_first):
        if channel_first:
            B, c, Ti, Hi, Wi = x_shape
        else:
            B, Ti, Hi, Wi, c = x_shape
        cout, cin = conv_w.shape[0], conv_w.shape[1]
        if c != cin:
            raise Unsupported("channel mismatch")
        if not ops.weight_layout_ok(conv_w) or conv_w.dtype != torch.float32:
            raise Unsupported("weight layout")
        return ops._desc_cached((B, Ti, Hi, Wi), cin, cout, ops._kdims(conv_w), tuple(stride), tuple(pad), channel_first)

    def applies_bn(self, next_conv, ysh):
        """``next_conv``, the only consumer of a layer's output [ysh], can apply that layer's BatchNorm (+ReLU) to its input while
        it stages it (``d.in_affine``: conv2x's temporal layers)."""
        if next_conv is None:
            return False
        nw = next_conv.weight
        return bool(ops.weight_layout_ok(nw) and nw.dtype == torch.float32 and nw.shape[1] == ysh[-1] and not next_conv.channel_first
                    and self.desc(ysh, nw, next_conv.stride3, next_conv.padding3, False)[0].in_affine)

    def linear_fwd(self, lin, x, relu, arena=None):
        """nn.Linear (+ReLU) as a 1x1x1 convolution over [B,1,1,1,C] (ops.linear).  ``arena``: where the output goes (default:
        the forward arena)."""
        w = lin.weight
        B, Cin = x.shape
        d = ops._desc_cached((B, 1, 1, 1), w.shape[1], w.shape[0], (1, 1, 1), (1, 1, 1), (0, 0, 0), False)[0]
        if Cin != w.shape[1] or not ops.weight_layout_ok(w):
            raise Unsupported("linear")
        y = (arena or self.fa).alloc(4 * B * d.Cout)
        self.emit(OP_CONV_FWD, d=d, i=(1 if relu else 0,), t=(x.ref, self.ext(w), None, None, self.ext(lin.bias), y, None))
        return {"lin": lin, "d": d, "x": x, "y": Sym(y, (B, d.Cout)), "relu": relu, "w": w}

    def gpool_fwd(self, x, arena=None):
        B, Cc = x.shape[0], x.shape[-1]
        S = x.numel // (B * Cc)
        y = (arena or self.fa).alloc(4 * B * Cc)
        am = self.fa.alloc(4 * B * Cc)
        self.emit(OP_GPOOL_FWD, i=(B, S, Cc), t=(x.ref, y, am))
        return {"x": x, "y": Sym(y, (B, Cc)), "am": am, "S": S}

    def cls_linear_fwd(self, cls, feat, arena=None):
        """The classifier of ``_classifier`` (``avid_cls_linear_fwd``: any number of classes) on features [B, Fd]; returns the logits."""
        B, Fd = feat.shape
        Cn = cls.weight.shape[0]
        if cls.weight.shape[1] != Fd or not cls.weight.is_contiguous():
            raise Unsupported("classifier")
        logits = (arena or self.fa).alloc(4 * B * Cn)
        self.emit(OP_CLS_LINEAR_FWD, i=(B, Fd, Cn), t=(feat.ref, self.ext(cls.weight), self.ext(cls.bias), logits))
        return Sym(logits, (B, Cn))

    def probe_head_fwd(self, c, h, Cn, training, arena=None):
        """One head of ``_probe_heads`` on its tap ``h``: ``avid_adaptive_maxpool_fwd`` (channels-last tap -> the reference's flatten
        order), BatchNorm1d on batch (``training``) or running statistics, ``avid_probe_linear_fwd`` into ``arena``.  Returns the
        head record (``"logits"``: Sym [B, Cn])."""
        B, T, H, W, Cc = h.shape
        To, Ho, Wo = c.pool_size
        Fd = Cc * To * Ho * Wo
        bn, lin = c.bn, c.classifier
        if tuple(lin.weight.shape) != (Cn, Fd) or not lin.weight.is_contiguous() or bn.num_features != Fd or B > 256 or Fd > 16384:
            raise Unsupported("probe head geometry")
        pooled, normed, save2 = self.fa.alloc(4 * B * Fd), self.fa.alloc(4 * B * Fd), self.fa.alloc(8 * Fd)
        d = ConvDesc()
        d.To, d.Ho, d.Wo = To, Ho, Wo
        self.emit(OP_ADAPTIVE_MAXPOOL, d=d, i=(B, T, H, W, Cc), t=(h.ref, pooled))
        self.emit(OP_BN1D_FWD, i=(B, Fd, 1 if training else 0), f=(bn.momentum, bn.eps),
                  t=(pooled, self.ext(bn.weight), self.ext(bn.bias), self.ext(bn.running_mean), self.ext(bn.running_var), normed, save2,
                     self.ext(bn.num_batches_tracked) if training else None))
        logits = (arena or self.fa).alloc(4 * B * Cn)
        self.emit(OP_PROBE_LINEAR_FWD, i=(B, Fd, Cn), t=(normed, self.ext(lin.weight), self.ext(lin.bias), logits))
        return {"c": c, "Fd": Fd, "pooled": pooled, "normed": normed, "save2": save2, "logits": Sym(logits, (B, Cn))}

    # ---- module walkers --------------------------------------------------------------------------------------------
    def video_fwd(self, vm, x, after_stem=None, arena=None):
        """The tower; ``after_stem()`` runs behind the stem's records, ``arena``: where the pooled output goes (default: the forward
        arena).  Returns ({"stem", "blocks": the blocks' layer records, "stages": {stage name: Sym of its output}, "pool"},
        Sym of the pooled features)."""
        from models.video import R2Plus1D
        from models.network_blocks import BasicR2P1DBlock, BatchNormCL, ConvCL
        if type(vm) is not R2Plus1D:
            raise Unsupported(type(vm).__name__)
        conv, bn = vm.conv1[0], vm.conv1[1]
        if type(conv) is not ConvCL or type(bn) is not BatchNormCL:
            raise Unsupported("video stem")
        d, _, _, _, srows = self.desc(x.shape, conv.weight, conv.stride3, conv.padding3, True)
        psh = (d.B, d.To, (d.Ho + 2 - 3) // 2 + 1, (d.Wo + 2 - 3) // 2 + 1, d.Cout)     # behind the stem's (1,3,3) / (1,2,2) max pool
        stem, p = self.stem_fwd(conv.weight, bn, x, d, srows, psh)
        h = Sym(p, psh)
        if after_stem is not None:
            after_stem()
        blocks, stages = [], {}
        for name in _STAGES:
            stage = getattr(vm, name)
            for blk in (stage if isinstance(stage, torch.nn.Sequential) else [stage]):
                if type(blk) is not BasicR2P1DBlock:
                    raise Unsupported(type(blk).__name__)
                Ls, h = self.r2p1d_block_fwd(blk, h)
                blocks.append(Ls)
            stages[name] = h
        pool = self.gpool_fwd(h, arena=arena)
        return {"stem": stem, "blocks": blocks, "stages": stages, "pool": pool}, pool["y"]

    def audio_fwd(self, am, x, arena=None):
        """The audio tower on x [B, 1, 1, T, F]; ``arena``: where the pooled output goes (default: the forward arena).  Returns
        ({"layers": the layer records, "stages": {stage name: Sym of block1..block4's output — the names ``Conv2D.forward`` gives
        them under ``return_embs``}, "pool"}, Sym of the pooled features)."""
        from models.audio import Conv2D
        from models.network_blocks import Basic2DBlock, BatchNormCL, ConvCL
        if type(am) is not Conv2D:
            raise Unsupported(type(am).__name__)
        if type(am.conv1[0]) is not ConvCL or type(am.conv1[1]) is not BatchNormCL:
            raise Unsupported("audio stem")
        Ls = [self.conv_bn_fwd(am.conv1[0], am.conv1[1], x)]
        stages = {}
        for name, blk in zip(_STAGES, (am.block1, am.block2, am.block3, am.block4)):
            if type(blk) is not Basic2DBlock:
                raise Unsupported(type(blk).__name__)
            for conv, bn in ((blk.conv1, blk.bn1), (blk.conv2, blk.bn2)):
                Ls.append(self.conv_bn_fwd(conv, bn, Ls[-1]["h"]))
            stages[name] = Ls[-1]["h"]
        pool = self.gpool_fwd(Ls[-1]["h"], arena=arena)
        return {"layers": Ls, "stages": stages, "pool": pool}, pool["y"]

    def tower_fwd(self, tower, shape, arena=None):
        """The single tower of a fine-tuning, probe or inference plan on the input of slot ``S_VIDEO``: ``video_fwd`` for an
        ``R2Plus1D`` on clips [B, 3, T, H, W], ``audio_fwd`` for a ``Conv2D`` on spectrograms [B, 1, T, F]; anything else is
        ``video_fwd``'s refusal.  Returns (the walker's record with "stages" and "pool", Sym of the pooled features)."""
        if _audio_tower(tower):
            return self.audio_fwd(tower, _tower_input(True, shape), arena=arena)
        return self.video_fwd(tower, _tower_input(False, shape), arena=arena)

    def head_fwd(self, head, x, arena=None):
        """The projection head; ``arena``: where the LAST layer's output goes (default: the forward arena)."""
        from models.av_wrapper import Head, LinearCL
        if type(head) is not Head:
            raise Unsupported(type(head).__name__)
        mods = list(head.projection)
        Ls, k = [], 0
        while k < len(mods):
            if type(mods[k]) is not LinearCL:
                raise Unsupported("head")
            relu = k + 1 < len(mods) and isinstance(mods[k + 1], torch.nn.ReLU)
            k_next = k + (2 if relu else 1)
            L = self.linear_fwd(mods[k], x, relu, arena=arena if k_next >= len(mods) else None)
            Ls.append(L)
            x, k = L["y"], k_next
        return Ls, x


class TrainBuilder(Builder):
    """The training form: BatchNorms on batch statistics, every activation kept in a bump arena, then the backward records,
    the flat gradient buffer's layout and the order in which its slices complete."""

    def __init__(self, device, overlap_towers, trailing, group):
        super().__init__(device, Arena(S_FWD))
        self.overlap, self.trailing, self.group = overlap_towers, trailing, group
        self.ba = Arena(S_BWD)
        self.bwd = []
        self.params, self.pindex = [], {}          # trainable parameters in gradient-buffer order
        self.pending = {ST_MAIN: [], ST_AUDIO: []}  # queued weight gradients per compute stream
        self.trail_used = set()
        self.grad_ready = []                       # (index of the backward record that completes them, [param index])
        self._err = None

    def grad(self, p):
        """Reference of parameter p's slice of the flat gradient buffer."""
        return (S_GRAD, 4 * self.goff[self.pindex[id(p)]])

    def set_params(self, params):
        """Gradient-buffer layout = ``parallel.FlatParams``': reverse registration order, 16-byte aligned slices."""
        self.params = list(reversed(params))
        self.goff, off = [], 0
        for k, p in enumerate(self.params):
            self.pindex[id(p)] = k
            self.goff.append(off)
            off += (p.numel() + 3) // 4 * 4
        self.gnumel = off

    def dgrad_wt_u(self, w, d):
        """(wt, u) of an input gradient: the Winograd transform, the pre-split transpose, or the plain transpose."""
        if d.wino_dgrad:
            return self.want_wt(w), self.want_u(w, d.wino_dgrad)
        if d.split_dgrad:
            return None, self.want_split(w, 6)
        return self.want_wt(w), None

    # ---- forward emitters ------------------------------------------------------------------------------------------
    def stem_fwd(self, w, bn, x, d, srows, psh):
        """The video stem: convolution with BatchNorm partial sums, then BatchNorm + ReLU + max pool in one pass."""
        B, T, H, W, Cc = d.B, d.To, d.Ho, d.Wo, d.Cout
        n = B * psh[1] * psh[2] * psh[3] * Cc
        y = self.fa.alloc(4 * B * T * H * W * Cc)
        stats = self.fa.alloc(4 * srows * 2 * Cc) if srows > 0 else None
        self.emit(OP_CONV_FWD, d=d, i=(0,), t=(x.ref, self.ext(w), None, None, None, y, stats))
        p = self.fa.alloc(4 * n)
        am = self.fa.alloc(n)
        s4 = self.fa.alloc(16 * Cc)
        self.emit(OP_BN_POOL_FWD, i=(B, T, H, W, Cc, srows if stats is not None else 0), f=(bn.momentum, bn.eps),
                  t=(y, self.ext(bn.weight), self.ext(bn.bias), self.ext(bn.running_mean), self.ext(bn.running_var), p, am, s4,
                     self.ext(bn.num_batches_tracked), stats))
        return {"d": d, "w": w, "x": x, "y": y, "am": am, "s4": s4, "bn": bn, "dims": (B, T, H, W, Cc)}, p

    def conv_bn_fwd(self, conv, bn, x, addend=None, next_conv=None, res=None, sole=True):
        """ReLU(bn(conv(x) [+ addend])) (network_blocks._conv_bn in training mode).  Returns the layer record.

        ``next_conv``: the ONLY consumer of this layer's output, if that is known to be a convolution.  When its kernels can apply
        a BatchNorm (+ReLU) to their input while they stage it (``applies_bn``), this layer's
        BatchNorm makes its statistics only and the returned ``h`` is the convolution's OUTPUT tagged with the map
        (``Sym.affine``): the normalised tensor is never written or read."""
        w = conv.weight
        d, _, _, _, srows = self.desc(x.shape, w, conv.stride3, conv.padding3, conv.channel_first)
        ysh = (d.B, d.To, d.Ho, d.Wo, d.Cout)
        M = d.B * d.To * d.Ho * d.Wo
        y = self.fa.alloc(4 * M * d.Cout)
        stats = self.fa.alloc(4 * srows * 2 * d.Cout) if srows > 0 else None
        xa = x.affine
        if xa is not None and not (d.in_affine and res is None):
            raise Unsupported("a tensor with a pending BatchNorm reached a layer that cannot apply it")
        self.emit(OP_CONV_FWD, d=d, i=(0,) if xa is None else (0, 2 if xa[1] else 1, xa[2]),
                  t=(x.ref, self.ext(w), self.fwd_u(w, d), addend.ref if addend is not None else None, None, y, stats) +
                    (() if xa is None else (xa[0],)))
        L = {"conv": conv, "bn": bn, "d": d, "x": x, "y": y, "w": w, "sole": sole, "res": None, "M": M}
        if res is not None:
            rconv = res
            rw = rconv.weight
            if conv.channel_first or ops._kdims(rw) != (1, 1, 1) or rw.shape[1] != d.Cin:
                raise Unsupported("residual convolution")
            dr = self.desc(x.shape, rw, rconv.stride3, (0, 0, 0), False)[0]
            y_res = self.fa.alloc(4 * d.B * dr.To * dr.Ho * dr.Wo * dr.Cout)
            self.emit(OP_CONV_FWD, d=dr, i=(0,), t=(x.ref, self.ext(rw), self.fwd_u(rw, dr), None, None, y_res, None))
            L["res"] = {"conv": rconv, "d": dr, "w": rw, "y": Sym(y_res, (d.B, dr.To, dr.Ho, dr.Wo, dr.Cout))}
        Cc = d.Cout
        defer = addend is None and res is None and self.applies_bn(next_conv, ysh)
        h = None if defer else self.fa.alloc(4 * M * Cc)
        s4 = self.fa.alloc(4 * 4 * Cc)
        self.emit(OP_BN_FWD, n=(M,), i=(Cc, 1, srows if stats is not None else 0), f=(bn.momentum, bn.eps),
                  t=(y, self.ext(bn.weight), self.ext(bn.bias), self.ext(bn.running_mean), self.ext(bn.running_var), h, s4,
                     self.ext(bn.num_batches_tracked), stats))
        rec = BnRec(y, s4, 1, Cc)
        L["bnrec"] = rec
        L["h"] = Sym(y, ysh, bn=rec, affine=(s4, 1, Cc)) if defer else Sym(h, ysh, bn=rec)
        return L

    def r2p1d_block_fwd(self, blk, x):
        """The strided 1x1x1 residual convolution is emitted right behind ``spt_conv1`` (the same input, ``conv_bn_fwd(res=...)``)."""
        from models.network_blocks import res_fusable
        if blk.res and not res_fusable(blk, x.numel):
            raise Unsupported("residual convolution outside the fused pattern")
        # (spt_bn1 -> tmp_conv1 and spt_bn2 -> tmp_conv2: each BatchNorm's output has exactly one reader, the next convolution)
        L1 = self.conv_bn_fwd(blk.spt_conv1, blk.spt_bn1, x, res=blk.res_conv if blk.res else None,
                              next_conv=None if blk.res else blk.tmp_conv1)
        L2 = self.conv_bn_fwd(blk.tmp_conv1, blk.tmp_bn1, L1["h"])
        L3 = self.conv_bn_fwd(blk.spt_conv2, blk.spt_bn2, L2["h"], next_conv=blk.tmp_conv2)
        addend = L1["res"]["y"] if blk.res else x
        L4 = self.conv_bn_fwd(blk.tmp_conv2, blk.out_bn, L3["h"], addend=addend)
        return (L1, L2, L3, L4), L4["h"]

    def cls_loss(self, logits, tap=0):
        """``AVID_OP_CLS_LOSS`` of head ``tap`` (run by the step engine only): loss and hits into its OUT_BYTES of S_OUT, its
        [B, C] of ``dlogits``; a label outside [0, C) is reported in the device error word (ops.DeviceErrors)."""
        B, Cn = logits.shape
        if self._err is None:
            dry = self.device.type != "cuda"
            self._err = self.ext(torch.zeros((), dtype=torch.int32) if dry else ops.DeviceErrors.get(self.device).flag)
        self.emit(OP_CLS_LOSS, i=(B, 1, Cn), f=(1.0,),
                  t=(logits.ref, (S_LABELS, 0), (S_OUT, OUT_BYTES * tap), None, (S_OUT, OUT_BYTES * tap + 8),
                     (S_DLOGITS, 4 * B * Cn * tap), self._err))

    def mlabel_loss(self, logits, tap=0, pos_weight=None):
        """``AVID_OP_MLABEL_LOSS`` of head ``tap`` (run by the step engine only), the multi-label sibling of ``cls_loss``: the
        label slot holds float32 targets [B, C]; ``pos_weight`` (a float32 [C] tensor, or None) is an external slot; a target
        outside [0, 1] is reported in the device error word."""
        B, Cn = logits.shape
        if self._err is None:
            dry = self.device.type != "cuda"
            self._err = self.ext(torch.zeros((), dtype=torch.int32) if dry else ops.DeviceErrors.get(self.device).flag)
        self.emit(OP_MLABEL_LOSS, i=(B, 1, Cn), f=(1.0,),
                  t=(logits.ref, (S_LABELS, 0), None if pos_weight is None else self.ext(pos_weight), (S_OUT, OUT_BYTES * tap), None,
                     (S_OUT, OUT_BYTES * tap + 8), (S_DLOGITS, 4 * B * Cn * tap), self._err))

    def soft_ce_loss(self, logits, tap=0, label_smoothing=0.0):
        """``AVID_OP_SOFT_CE_LOSS`` of head ``tap`` (run by the step engine only), ``cls_loss`` against a distribution: the label
        slot holds float32 targets [B, C]; ``label_smoothing`` is the record's f1; a negative or non-finite target is reported
        in the device error word."""
        B, Cn = logits.shape
        if self._err is None:
            dry = self.device.type != "cuda"
            self._err = self.ext(torch.zeros((), dtype=torch.int32) if dry else ops.DeviceErrors.get(self.device).flag)
        self.emit(OP_SOFT_CE_LOSS, i=(B, 1, Cn), f=(1.0, float(label_smoothing)),
                  t=(logits.ref, (S_LABELS, 0), (S_OUT, OUT_BYTES * tap), None, (S_OUT, OUT_BYTES * tap + 8),
                     (S_DLOGITS, 4 * B * Cn * tap), self._err))

    def loss(self, kind, logits, tap=0, pos_weight=None, label_smoothing=0.0):
        """The loss record of a supervised plan: ``"ce"`` (``cls_loss``), ``"bce"`` (``mlabel_loss``) or ``"soft_ce"``
        (``soft_ce_loss``)."""
        if kind == "ce":
            self.cls_loss(logits, tap=tap)
        elif kind == "soft_ce":
            self.soft_ce_loss(logits, tap=tap, label_smoothing=label_smoothing)
        else:
            self.mlabel_loss(logits, tap=tap, pos_weight=pos_weight)

    # ---- backward emitters -----------------------------------------------------------------------------------------
    def _ready(self, stream, *ps):
        """The records emitted so far complete the gradients of ``ps`` (written on ``stream``)."""
        self.grad_ready.append((len(self.bwd), stream, [self.pindex[id(p)] for p in ps]))

    def flush_group(self, S=None):
        S = self.S if S is None else S
        lst, self.pending[S] = self.pending[S], []
        if not lst:
            return
        stream = S
        if self.trailing:
            stream = ST_TRAIL
            self.wait(stream, S)                      # every dy of the group is complete on its compute stream
            self.trail_used.add(stream)
        self.emit(OP_WGRAD_GROUP, stream=stream, i=(len(lst),))
        for d, xr, dyr, w in lst:
            self.emit(OP_WGRAD_ITEM, stream=stream, d=d, t=(xr, dyr, self.grad(w)))
        self._ready(stream, *[t[3] for t in lst])

    def wgrad(self, d, xr, dyr, w, flush_check=True, xa=None):
        """The weight gradient of one layer: queued for a grouped launch (small layers), or its own launch on the
        trailing stream; False = the caller emits it on the compute stream (behind the input gradient)."""
        if self.group and d.groupable:
            if xa is not None:
                raise Unsupported("a grouped weight gradient cannot apply its input's BatchNorm")
            self.pending[self.S].append((d, xr, dyr, w))
            if len(self.pending[self.S]) >= ops.GROUP_MAX:
                self.flush_group()
            return True
        if flush_check and self.group and len(self.pending[self.S]) >= ops.GROUP_MIN_FLUSH:
            self.flush_group()                        # the small layers queued so far go first
        if self.trailing:
            self.wait(ST_TRAIL, self.S)
            self.emit(OP_CONV_WGRAD, stream=ST_TRAIL, d=d, **self._wgrad_args(xr, dyr, w, xa))
            self._ready(ST_TRAIL, w)
            self.trail_used.add(ST_TRAIL)
            return True
        return False                                   # the caller emits it behind the input gradient

    def _wgrad_args(self, xr, dyr, w, xa):
        """i / t of an OP_CONV_WGRAD record; xa = Sym.affine of the layer's input (None: x is read as it is)."""
        if xa is None:
            return {"t": (xr, dyr, self.grad(w))}
        return {"i": (2 if xa[1] else 1, xa[2]), "t": (xr, dyr, self.grad(w), xa[0])}

    def wgrad_inline(self, d, xr, dyr, w, xa=None):
        self.emit(OP_CONV_WGRAD, d=d, **self._wgrad_args(xr, dyr, w, xa))
        self._ready(self.S, w)

    def conv_bwd(self, d, w, x, g, need_dx, add=None, add_stride=None, res=None, g_res=None):
        """Backward of one convolution given g = d(loss)/d(conv output): weight gradient, [residual branch,] input
        gradient (ops._ConvCL.backward, same order of launches per stream).  Returns the reference of dx."""
        done = self.wgrad(d, x.ref, g, w, xa=x.affine)
        if res is not None:
            if x.affine is not None:
                raise Unsupported("residual convolution on a tensor with a pending BatchNorm")
            dr, rw = res["d"], res["w"]
            if need_dx:
                # compact input gradient of the residual convolution: a dense 1x1x1 dgrad over the sub-sampled grid
                dc = ops._desc_cached((d.B, dr.To, dr.Ho, dr.Wo), d.Cin, dr.Cout, (1, 1, 1), (1, 1, 1), (0, 0, 0), False)[0]
                add = self.ba.alloc(4 * d.B * dr.To * dr.Ho * dr.Wo * d.Cin)
                self.emit(OP_CONV_DGRAD, d=dc, i=(0, 0, 0, 0, 0), t=(g_res, self.ext(rw), *self.dgrad_wt_u(rw, dc), None, add))
                rs = res["conv"].stride3
                add_stride = tuple(rs) if any(v != 1 for v in rs) else None
            if not self.wgrad(dr, x.ref, g_res, rw, flush_check=False):
                self.wgrad_inline(dr, x.ref, g_res, rw)
        dx = None
        if need_dx:
            dx = self.ba.alloc(4 * x.numel)
            src = x.bn
            fuse = src is not None and ops.FUSE_BN_BWD and d.bn_bwd_rows > 0
            t = [g, self.ext(w), *self.dgrad_wt_u(w, d), add, dx]
            iv = list(add_stride) if add_stride is not None else [0, 0, 0]
            if fuse:
                src.rows = d.bn_bwd_rows
                src.partials = self.ba.alloc(4 * src.rows * 2 * d.Cin)
                Cc = src.C
                t += [src.x, _off(src.s4, 8 * Cc), _off(src.s4, 12 * Cc), src.s4, _off(src.s4, 4 * Cc), src.partials]
                iv += [src.relu, 1]
            else:
                iv += [0, 0]
            self.emit(OP_CONV_DGRAD, d=d, i=iv, t=t)
        if not done:
            self.wgrad_inline(d, x.ref, g, w, xa=x.affine)
        return dx

    def conv_bn_bwd(self, L, dh, need_dx=True, add=None, g_res=None):
        """Backward of a conv_bn_fwd layer given dh = d(loss)/d(h).  Returns (g, dx): g = gradient at the convolution's
        output (== gradient of its addend), dx = gradient of its input (None if not needed)."""
        d, bn, rec = L["d"], L["bn"], L["bnrec"]
        g = self.ba.alloc(4 * L["M"] * d.Cout)
        self.emit(OP_BN_BWD, n=(L["M"],), i=(d.Cout, 1, rec.rows if rec.partials is not None else 0, 0),
                  t=(L["y"], dh, self.ext(bn.weight), rec.s4, g, self.grad(bn.weight), self.grad(bn.bias), rec.partials))
        self._ready(self.S, bn.weight, bn.bias)
        x = L["x"]
        if not L["sole"]:
            x = Sym(x.ref, x.shape, affine=x.affine)  # not the only consumer: no BatchNorm hand-over
        dx = self.conv_bwd(d, L["w"], x, g, need_dx, add=add, res=L["res"], g_res=g_res)
        return g, dx

    def linear_bwd(self, L, dy):
        d, lin = L["d"], L["lin"]
        B = d.B
        if L["relu"]:
            g = self.ba.alloc(4 * B * d.Cout)
            self.emit(OP_RELU_BWD, n=(B * d.Cout,), t=(L["y"].ref, dy, g))
            dy = g
        dx = self.conv_bwd(d, L["w"], L["x"], dy, True)
        self.emit(OP_COLSUM, n=(B,), i=(d.Cout,), t=(dy, self.grad(lin.bias)))
        self._ready(self.S, lin.bias)
        return dx

    def gpool_bwd(self, P, dy):
        x = P["x"]
        dx = self.ba.alloc(4 * x.numel)
        self.emit(OP_GPOOL_BWD, i=(x.shape[0], P["S"], x.shape[-1]), t=(dy, P["am"], dx))
        return dx

    def r2p1d_block_bwd(self, Ls, dout):
        L1, L2, L3, L4 = Ls
        g4, dh3 = self.conv_bn_bwd(L4, dout)
        _, dh2 = self.conv_bn_bwd(L3, dh3)
        _, dh1 = self.conv_bn_bwd(L2, dh2)
        if L1["res"] is not None:
            _, dx = self.conv_bn_bwd(L1, dh1, g_res=g4)
        else:
            _, dx = self.conv_bn_bwd(L1, dh1, add=g4)       # identity residual: its gradient rides in the dgrad's addend
        return dx

    def video_bwd(self, V, dy):
        dh = self.gpool_bwd(V["pool"], dy)
        for Ls in reversed(V["blocks"]):
            dh = self.r2p1d_block_bwd(Ls, dh)
        return dh

    def video_stem_bwd(self, V, dh):
        st = V["stem"]
        B, T, H, W, Cc = st["dims"]
        bn = st["bn"]
        dx = self.ba.alloc(4 * B * T * H * W * Cc)
        self.emit(OP_BN_POOL_BWD, i=(B, T, H, W, Cc),
                  t=(st["y"], dh, st["am"], self.ext(bn.weight), st["s4"], dx, self.grad(bn.weight), self.grad(bn.bias)))
        self._ready(self.S, bn.weight, bn.bias)
        self.conv_bwd(st["d"], st["w"], st["x"], dx, False)

    def audio_bwd(self, A, dy):
        dh = self.gpool_bwd(A["pool"], dy)
        Ls = A["layers"]
        for k in range(len(Ls) - 1, -1, -1):
            _, dh = self.conv_bn_bwd(Ls[k], dh, need_dx=k > 0)

    def tower_bwd(self, V, dy):
        """The backward of ``tower_fwd``'s record from the pooled features' gradient: ``audio_bwd``, or ``video_bwd`` with the
        stem behind the queued weight-gradient group."""
        if "layers" in V:
            return self.audio_bwd(V, dy)
        dh = self.video_bwd(V, dy)
        self.flush_group(ST_MAIN)
        self.video_stem_bwd(V, dh)

    def head_bwd(self, Ls, dy):
        for L in reversed(Ls):
            dy = self.linear_bwd(L, dy)
        return dy


class EvalBuilder(Builder):
    """The eval form of the layer emitters: BatchNorms use their running statistics — every coefficient vector comes out of ONE
    launch at the head of the program (``AVID_OP_BN_EVAL_COEFFS``), a (3,1,1) layer of conv2x applies its own BatchNorm in its
    epilogue (``d.out_affine``) and the one in front of it while staging (``d.in_affine``), everything else is a convolution
    followed by ``AVID_OP_BN_EVAL_APPLY``; the stem's tail is one pass.  No statistics, no argmax of the stem's pool, no saved
    vectors for a backward.  Each record is the call the per-layer path makes in eval mode with trainable BatchNorm parameters
    (``avid_bn_fwd_eval`` with ``save4``: y = fma(x, scale, shift)) or a fusion that is bit-identical to it.
    A BatchNorm whose weight and bias take NO gradient (the linear probe's frozen tower) is another case: the per-layer path then
    calls ``avid_bn_fwd_eval`` without ``save4``, which evaluates ``(x - mean) * invstd * gamma + beta`` — other bits than the
    fma.  Such a BatchNorm is never fused: it is one ``AVID_OP_BN_EVAL_DIRECT`` record (the same call), the stem's pool behind it
    an ``AVID_OP_MAXPOOL_FWD`` record, and it has no entry in the coefficient table.
    Activations go to an ``EvalArena`` (``self.fa``), what leaves the program to ``self.oa`` (slot ``S_OUT``)."""

    def __init__(self, device):
        super().__init__(device, EvalArena(S_FWD))
        self.oa = Arena(S_OUT)
        self.bn_recs, self.bn_off = [], {}         # (BatchNorm module, aux offset of its [4][C] vectors)

    @staticmethod
    def frozen(bn):
        """The per-layer path computes this BatchNorm without coefficient vectors (ops._BatchNormCL.forward: no gradient can flow)."""
        return not (bn.weight.requires_grad or bn.bias.requires_grad)

    def bn_direct(self, bn, x, M, Cc, relu=1):
        """The unfused eval-mode BatchNorm (+ReLU) of a frozen BatchNorm: x -> a new tensor."""
        from models.network_blocks import BatchNormCL
        if type(bn) is not BatchNormCL or bn.weight.dtype != torch.float32:
            raise Unsupported("BatchNorm")
        h = self.fa.alloc(4 * M * Cc)
        self.emit(OP_BN_EVAL_DIRECT, n=(M,), i=(Cc, relu), f=(0.0, bn.eps),
                  t=(x, self.ext(bn.weight), self.ext(bn.bias), self.ext(bn.running_mean), self.ext(bn.running_var), h))
        return h

    def coeffs(self, bn):
        from models.network_blocks import BatchNormCL
        off = self.bn_off.get(id(bn))
        if off is None:
            if type(bn) is not BatchNormCL or bn.weight.dtype != torch.float32:
                raise Unsupported("BatchNorm")
            off = self.bn_off[id(bn)] = self.aux_size
            self.bn_recs.append((bn, off))
            self.aux_size += _align(16 * bn.num_features)
        return (S_AUX, off)

    def stem_fwd(self, w, bn, x, d, srows, psh):
        """The video stem: convolution, then BatchNorm + ReLU + max pool in one pass (no partial sums, no argmax)."""
        B, T, H, W, Cc = d.B, d.To, d.Ho, d.Wo, d.Cout
        n = B * psh[1] * psh[2] * psh[3] * Cc
        y = self.fa.alloc(4 * B * T * H * W * Cc)
        self.emit(OP_CONV_FWD, d=d, i=(0,), t=(x.ref, self.ext(w), None, None, None, y, None))
        p = self.fa.alloc(4 * n)
        if self.frozen(bn):                        # bn -> maxpool as the per-layer path runs them (its pool writes an argmax)
            am = self.fa.alloc(n)
            self.emit(OP_MAXPOOL_FWD, i=(B, T, H, W, Cc), t=(self.bn_direct(bn, y, B * T * H * W, Cc), p, am))
        else:
            self.emit(OP_BN_POOL_FWD_EVAL, i=(B, T, H, W, Cc), t=(y, self.coeffs(bn), p))
        return None, p

    def conv_bn_fwd(self, conv, bn, x, addend=None, next_conv=None):
        """ReLU(bn_eval(conv(x) [+ addend])); returns {"h": Sym of the result} (``affine`` set: its only consumer applies the map)."""
        w = conv.weight
        d = self.desc(x.shape, w, conv.stride3, conv.padding3, conv.channel_first)[0]
        ysh = (d.B, d.To, d.Ho, d.Wo, d.Cout)
        M, Cc = d.B * d.To * d.Ho * d.Wo, d.Cout
        xa = x.affine
        if xa is not None and not d.in_affine:
            raise Unsupported("a tensor with a pending BatchNorm reached a layer that cannot apply it")
        iv = (0, 0, 0) if xa is None else (0, 2 if xa[1] else 1, xa[2])
        t = [x.ref, self.ext(w), self.fwd_u(w, d), addend.ref if addend is not None else None, None]
        xr = None if xa is None else xa[0]
        if self.frozen(bn):                        # convolution, then the call the per-layer path makes: nothing fused
            y = self.fa.alloc(4 * M * Cc)
            self.emit(OP_CONV_FWD, d=d, i=iv, t=t + [y, None, xr])
            return {"h": Sym(self.bn_direct(bn, y, M, Cc), ysh)}
        c4 = self.coeffs(bn)
        if d.out_affine:
            h = self.fa.alloc(4 * M * Cc)
            self.emit(OP_CONV_FWD, d=d, i=iv + (2,), t=t + [h, None, xr, c4])
            return {"h": Sym(h, ysh)}
        y = self.fa.alloc(4 * M * Cc)
        self.emit(OP_CONV_FWD, d=d, i=iv, t=t + [y, None, xr])
        if addend is None and self.applies_bn(next_conv, ysh):
            return {"h": Sym(y, ysh, affine=(c4, 1, Cc))}
        h = self.fa.alloc(4 * M * Cc)
        self.emit(OP_BN_EVAL_APPLY, n=(M,), i=(Cc, 1), t=(y, c4, h))
        return {"h": Sym(h, ysh)}

    def r2p1d_block_fwd(self, blk, x):
        """The strided 1x1x1 residual convolution is a record of its own in front of ``tmp_conv2``, which adds it: its output
        lives for one record, which keeps the recycled arena small."""
        h = self.conv_bn_fwd(blk.spt_conv1, blk.spt_bn1, x, next_conv=blk.tmp_conv1)["h"]
        h = self.conv_bn_fwd(blk.tmp_conv1, blk.tmp_bn1, h)["h"]
        h = self.conv_bn_fwd(blk.spt_conv2, blk.spt_bn2, h, next_conv=blk.tmp_conv2)["h"]
        res = x
        if blk.res:
            rc = blk.res_conv
            dr = self.desc(x.shape, rc.weight, rc.stride3, rc.padding3, False)[0]
            yr = self.fa.alloc(4 * dr.B * dr.To * dr.Ho * dr.Wo * dr.Cout)
            self.emit(OP_CONV_FWD, d=dr, i=(0,), t=(x.ref, self.ext(rc.weight), self.fwd_u(rc.weight, dr), None, None, yr, None))
            res = Sym(yr, (dr.B, dr.To, dr.Ho, dr.Wo, dr.Cout))
        return None, self.conv_bn_fwd(blk.tmp_conv2, blk.out_bn, h, addend=res)["h"]


# Least size of a stream's workspace in a sealed program.  Every record that takes scratch is counted by
# avid_program_workspace_bytes; the floor only keeps small programs from each holding an odd-sized allocation of its own.
# The tests set it to 0, so that the size function alone decides what the records get.
WS_FLOOR = 1 << 20


class Programs:
    """Launch programs sealed and ready to run: the record arrays of what a ``Builder`` emitted, the aux buffer with the
    weight-transform tables, the streams' workspaces, the slot table — and the per-run plumbing that fills them."""

    def _seal(self, b, *programs):
        """Patch the weight-transform record (``self._wt_rec``) now that the table is known, then freeze each record list of
        ``programs`` into an ``Instr`` array (returned, in order) and size the aux buffer and the streams' workspaces for all."""
        self.wt_recs = b.wt_recs
        self.table_off = _align(b.aux_size)
        self.aux_bytes = self._aux_layout(b)
        self._wt_rec.i[0] = len(b.wt_recs)
        self._wt_rec.n[0] = max([r[2] * r[3] * r[4] for r in b.wt_recs] + [1])
        self._wt_rec.t[0].off = self.table_off
        if not b.wt_recs:
            self._wt_rec.op = 0
        progs = [(Instr * max(1, len(recs)))(*recs) for recs in programs]
        self.ws_bytes = [int(WS_FLOOR)] * 4
        for prog, recs in zip(progs, programs):
            need = (_sz * 4)()
            lib.call("avid_program_workspace_bytes", prog, 0, len(recs), 4, need)
            self.ws_bytes = [max(have, int(n)) for have, n in zip(self.ws_bytes, need)]
        self.ws = [torch.empty(n, dtype=torch.uint8, device=self.device) for n in self.ws_bytes]
        self.ws_arr = (StreamWs * 4)()
        for k in range(4):
            self.ws_arr[k].ptr, self.ws_arr[k].bytes = self.ws[k].data_ptr(), self.ws_bytes[k]
        self.aux = torch.empty(self.aux_bytes, dtype=torch.uint8, device=self.device)
        self._table_ptrs = None
        self.tensors = b.tensors
        self.n_slots = S_FIRST_TENSOR + len(self.tensors)
        self.slots = (_vp * self.n_slots)()
        self.streams = (_vp * 4)()
        return progs

    def _aux_layout(self, b):
        """Bytes of the aux buffer: the builder's transformed weights, then the weight-transform table at ``table_off``."""
        return self.table_off + 32 * len(b.wt_recs) + 256

    # ---- per-run plumbing ------------------------------------------------------------------------------------------
    def _fill_slots(self, fa, ba, grad, inputs):
        """``inputs``: the tensors of slots S_VIDEO, S_AUDIO, S_DV, S_DA (None: unused by the records run)."""
        s = self.slots
        for k, t in enumerate((fa, ba, grad, self.aux) + tuple(inputs)):     # S_FWD .. S_DA
            s[k] = t.data_ptr() if t is not None else None
        s[S_FIRST_TENSOR:self.n_slots] = [t.data_ptr() for t in self.tensors]

    def _refresh_table(self):
        """The device table of weight-transform descriptors follows the parameters' current addresses."""
        ptrs = tuple(r[0].data_ptr() for r in self.wt_recs)
        if ptrs != self._table_ptrs and self.wt_recs:
            base = self.aux.data_ptr()
            recs = b"".join(struct.pack("<QQiiii", p, base + r[1], r[2], r[3], r[4], r[5]) for p, r in zip(ptrs, self.wt_recs))
            host = torch.frombuffer(bytearray(recs), dtype=torch.uint8)
            self.aux[self.table_off:self.table_off + len(recs)].copy_(host)
            self._table_ptrs = ptrs

    def _streams(self):
        """Raw handles of the run's streams: the current stream and the helper streams placed for it."""
        from . import streams
        ss = streams.current_set(self.device)
        st = self.streams
        st[0], st[1], st[2], st[3] = ss.main.cuda_stream, ss.side.cuda_stream, ss.trail.cuda_stream, ss.comm.cuda_stream
        self.stream_objs = (ss.main, ss.side, ss.trail, ss.comm)

    def _run(self, prog, begin, end):
        """Issue records [begin, end) of ``prog`` with the slots and streams set."""
        lib.call("avid_program_run", prog, begin, end, self.slots, self.n_slots, self.streams, self.ws_arr, 4)


class TrainPrograms(Programs):
    """A compiled pair of launch programs — forward and backward — over all of one model's parameters: what the two-tower
    ``Plan``, the classifier's ``ClsPlan`` and the probe's ``ProbePlan`` share.  A subclass compiles its own graph between
    ``_open`` (the checks, the forward's leading records), ``_backward_begins`` and ``_close`` (the backward's tail), and
    issues its own forward; the backward program runs the same way for all (``backward``)."""

    adam_early = None        # gradient offset from which the optimizer may start before the backward program ends (Plan)

    def _open(self, model, device, overlap_towers, trailing, group, frozen_ok=False):
        """The TrainBuilder of the model's parameters and the forward's leading records: what the backward needs but the forward
        does not — the gradient fill, the transposed / Winograd-transformed weights — runs on the trailing stream beside
        the forward; the table is known only after the backward is compiled, so ``_seal`` patches it in.
        ``frozen_ok``: parameters without ``requires_grad`` are allowed (the linear probe's tower); the gradient buffer
        then holds the trainable ones only, as ``parallel.FlatParams`` lays them out."""
        params = [p for p in model.parameters()]
        dry = device.type != "cuda"                  # (compile only: tests/test_plan_compile.py, no GPU)
        if not all((p.requires_grad or frozen_ok) and (p.is_cuda or dry) and p.dtype == torch.float32 for p in params):
            raise Unsupported("frozen / non-fp32 parameters")
        params = [p for p in params if p.requires_grad]
        b = TrainBuilder(device, overlap_towers, trailing, group)
        b.set_params(params)
        self.device, self.params_fwd = device, params
        helper = ST_TRAIL if trailing else ST_MAIN
        if trailing:
            b.wait(helper, ST_MAIN)
        self._zero_index = len(b.fwd)
        b.emit(OP_MEMSET0, stream=helper, n=(4 * b.gnumel,), t=((S_GRAD, 0),))
        self._wt_index = len(b.fwd)
        self._wt_rec = b.emit(OP_WT_BATCH, stream=helper, i=(0,), n=(0,), t=((S_AUX, 0),))
        b.S = ST_MAIN
        return b

    def _backward_begins(self, b):
        """The forward program ends here; the backward starts once the transposed weights are complete."""
        b.cur = b.bwd
        if b.trailing:
            b.wait(ST_MAIN, ST_TRAIL)
        b.S = ST_MAIN

    def _close(self, b, *joined):
        """The backward's last weight-gradient group, then the compute stream joins ``joined`` and every trailing stream."""
        b.flush_group(ST_MAIN)
        for S in joined + tuple(sorted(b.trail_used)):
            b.wait(ST_MAIN, S)
        self.n_fwd, self.n_bwd = len(b.fwd), len(b.bwd)
        self.fa_bytes, self.ba_bytes = max(b.fa.size, 256), max(b.ba.size, 256)
        self.params, self.goff, self.gnumel, self.grad_ready = b.params, b.goff, b.gnumel, b.grad_ready
        self.fwd_prog, self.bwd_prog = self._seal(b, b.fwd, b.bwd)
        self._wt_op = int(self.fwd_prog[self._wt_index].op)      # (0: the model has no weight in a derived form)

    def _forward_arena(self, grad_flat, zero_grad, inputs, tables=True):
        """A run of the forward program set up: weight table, arena, slots, streams, gradient fill on or off.  Returns the arena.
        ``tables=False``: the derived weight tables in the aux buffer (transposed, Winograd-transformed, pre-split) are those
        of an earlier run of THIS program with the same weights — a later shard of a virtual-rank step — and are not rebuilt."""
        self._refresh_table()
        self.fwd_prog[self._wt_index].op = self._wt_op if tables else 0
        fa = torch.empty(self.fa_bytes, dtype=torch.uint8, device=self.device)
        self._fill_slots(fa, None, grad_flat, inputs)
        self._streams()
        self.fwd_prog[self._zero_index].op = OP_MEMSET0 if (zero_grad and grad_flat is not None) else 0
        return fa

    def _view(self, fa, lg):
        """The tensor of a Sym (logits, embeddings) in the forward arena ``fa``."""
        n = 4 * lg.numel
        return fa[lg.ref[1]:lg.ref[1] + n].view(torch.float32).view(lg.shape)

    def backward(self, fa, inputs, grad_flat, begin=0, end=None, ba=None):
        """Issue records [begin, end) of the backward program (default: all of them) after the forward that returned ``fa``;
        ``inputs`` as ``_fill_slots``'.  Returns the backward arena (pass it back as ``ba`` for the next segment)."""
        if ba is None:
            ba = torch.empty(self.ba_bytes, dtype=torch.uint8, device=self.device)
        self._fill_slots(fa, ba, grad_flat, inputs)
        self._streams()
        self._run(self.bwd_prog, begin, self.n_bwd if end is None else end)
        return ba

    def grad_views(self, g):
        """{id(parameter): its gradient in the flat buffer ``g``}."""
        out = {}
        for p, o in zip(self.params, self.goff):
            out[id(p)] = g[o:o + p.numel()].as_strided(p.shape, p.stride())
        return out

    def segments(self, bucket_of, counts):
        """Cut the backward program where a gradient bucket becomes complete: [(end record, [(param index, stream)])] —
        the engine runs the records up to ``end``, reports those gradients (which launches the bucket's all-reduce) and
        goes on.  ``bucket_of[i]`` = bucket of parameter i (the plan's order), ``counts[b]`` = parameters in bucket b."""
        key = (tuple(bucket_of), tuple(counts))
        hit = self.__dict__.setdefault("_segments", {}).get(key)
        if hit is not None:
            return hit
        left = list(counts)
        segs, cur = [], []
        for end, stream, ps in self.grad_ready:
            cut = False
            for i in ps:
                cur.append((i, stream))
                left[bucket_of[i]] -= 1
                cut |= left[bucket_of[i]] == 0
            if cut:
                segs.append((end, cur))
                cur = []
        if cur or not segs or segs[-1][0] != self.n_bwd:
            segs.append((self.n_bwd, cur))
        self._segments[key] = segs
        return segs


class Plan(TrainPrograms):
    """The compiled forward / backward programs of one ``AV_Wrapper`` for one input geometry and stream arrangement."""

    def __init__(self, model, vshape, ashape, device, overlap_towers, trailing, group):
        if not model.use_linear_proj:
            raise Unsupported("no projection heads")
        b = self._open(model, device, overlap_towers, trailing, group)
        self.vshape, self.ashape = tuple(vshape), tuple(ashape)
        video = Sym((S_VIDEO, 0), vshape)
        audio = Sym((S_AUDIO, 0), (ashape[0], ashape[1], 1, ashape[2], ashape[3]))   # [B,1,1,H,W]: T = kt = 1
        A_S = ST_AUDIO if overlap_towers else ST_MAIN
        # ------------------------------------------------------------------ forward
        # the video stem first, then the audio tower starts on its own stream (beside conv2x.., not beside the stem:
        # models/av_wrapper.py AUDIO_AFTER)
        V, vfeat = self._video_with_audio(b, model, video, audio, A_S)
        A = self._A
        b.S = ST_MAIN
        VH, self.vemb = b.head_fwd(model.video_proj, vfeat)
        if A_S != ST_MAIN:
            b.wait(ST_MAIN, A_S)
        self.aemb = self._aemb
        # ------------------------------------------------------------------ backward (autograd's order: the video
        # tower from its head down to conv2x, the audio tower, the video stem last — sequence numbers of the forward)
        self._backward_begins(b)
        if A_S != ST_MAIN:
            b.wait(A_S, ST_MAIN)                      # the criterion's gradients (and the transposed weights)
        dv = b.head_bwd(VH, (S_DV, 0))
        dh = b.video_bwd(V, dv)
        b.S = A_S
        da = b.head_bwd(self._AH, (S_DA, 0))
        b.audio_bwd(A, da)
        # Everything but the video stem's three parameters has its gradient here: the engine's optimizer can update those
        # (nearly all of the 134 MB) on the fourth stream WHILE the stem's backward — one LDS-bound full-chip kernel of
        # 0.57 ms on the trailing stream, the step's last — still runs (parallel.TrainStep.step; the HBM-bound Adam pass and
        # that kernel overlap).  The fourth stream waits here for the three streams that hold those gradients.
        for S in (ST_MAIN, ST_AUDIO):
            b.S = S
            b.flush_group(S)
        b.S = ST_MAIN
        if trailing and A_S != ST_MAIN:
            stem_conv, stem_bn = model.video_model.conv1[0], model.video_model.conv1[1]
            idx = sorted(b.pindex[id(p)] for p in (stem_conv.weight, stem_bn.weight, stem_bn.bias))
            n = len(b.params)
            if idx == [n - 3, n - 2, n - 1]:                   # (the engine's flat layout: parameters in reverse order)
                for S in (ST_MAIN, A_S, ST_TRAIL):
                    b.wait(ST_COMM, S)
                self.adam_early = b.goff[n - 3]
        b.video_stem_bwd(V, dh)
        self._close(b, A_S)

    def _video_with_audio(self, b, model, video, audio, A_S):
        """The video tower with the audio tower (and its head) started behind the video stem on stream A_S."""
        def start_audio():
            S0 = b.S
            if A_S != ST_MAIN:
                b.wait(A_S, ST_MAIN)
            b.S = A_S
            self._A, afeat = b.audio_fwd(model.audio_model, audio)
            self._AH, self._aemb = b.head_fwd(model.audio_proj, afeat)
            b.S = S0
        return b.video_fwd(model.video_model, video, after_stem=start_audio)

    def forward(self, video, audio, grad_flat, zero_grad, tables=True):
        """Issue the forward program; returns (v_emb, a_emb, arena).  ``tables``: see ``_forward_arena``."""
        fa = self._forward_arena(grad_flat, zero_grad, (video, audio, None, None), tables)
        self._run(self.fwd_prog, 0, self.n_fwd)
        return self._view(fa, self.vemb), self._view(fa, self.aemb), fa


# ------------------------------------------------------------------------------------------------------------------
# autograd node + dispatch
# ------------------------------------------------------------------------------------------------------------------
_ENGINE = None          # the parallel.EngineCore driving the current step (flat gradient buffer, buckets), or None


class engine:
    """``with plan.engine(eng): ...`` — model calls inside write their parameter gradients into the engine's
    flat gradient buffer (and report them to its gradient buckets) instead of handing tensors to autograd."""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        global _ENGINE
        self.prev, _ENGINE = _ENGINE, self.eng
        return self

    def __exit__(self, *exc):
        global _ENGINE
        _ENGINE = self.prev
        return False


def _engine_flat(eng, pl):
    """The engine's flat gradient buffer if its layout is the plan's (same parameters, same offsets), else None."""
    flat = eng.flat
    ok = getattr(pl, "_engine_ok", None)
    if ok is None or ok[0] is not flat:
        same = (len(flat.params) == len(pl.params) and all(a is b for a, b in zip(flat.params, pl.params))
                and list(flat.offsets) == list(pl.goff))
        pl._engine_ok = ok = (flat, same)
    return eng.grad_target() if ok[1] else None


def _remember(ctx, pl, fa, params):
    ctx.pl, ctx.fa, ctx.params = pl, fa, params
    ctx.versions = sum(p._version for p in params)


def _check_backward(ctx):
    """The guards of a backward pass through a launch program: the forward's activations are still there, and no parameter
    the programs read was modified in place since."""
    if ctx.fa is None:
        raise RuntimeError("avid_hip.plan: backward through the same forward pass a second time (its activations "
                           "were released)")
    if sum(p._version for p in ctx.params) != ctx.versions:
        raise RuntimeError("avid_hip.plan: a parameter was modified in place between the forward and the backward pass")


def _autograd_backward(ctx, inputs, n_inputs):
    """The backward program outside a step engine: into a fresh flat gradient buffer whose slices go to autograd as the
    parameters' gradients, behind ``n_inputs`` Nones for the node's other inputs.  Releases the forward's arena."""
    pl = ctx.pl
    g = torch.empty(pl.gnumel, dtype=torch.float32, device=inputs[2].device)
    pl.backward(ctx.fa, inputs, g)
    ctx.fa = None
    views = pl.grad_views(g)
    return (None,) * n_inputs + tuple(views[id(p)] for p in ctx.params)


class NetFn(torch.autograd.Function):
    """(video, audio) -> (video_emb, audio_emb): models/av_wrapper.py:50-61 with both towers, both heads and all of
    their backward as two launch programs."""

    @staticmethod
    def forward(ctx, video, audio, pl, *params):
        eng = _ENGINE
        gflat = _engine_flat(eng, pl) if eng is not None else None
        ve, ae, fa = pl.forward(video, audio, gflat, zero_grad=gflat is not None, tables=eng is None or eng.rebuild_tables(pl))
        _remember(ctx, pl, fa, params)
        ctx.video, ctx.audio = video, audio
        ctx.in_engine = gflat is not None
        # the engine of THIS forward pass: the reference's loop calls loss.backward() itself, outside any `with plan.engine`
        # (parallel.DistributedDataParallel), and the gradients still have to land in the flat buffer this forward zeroed
        ctx.eng = eng if gflat is not None else None
        return ve, ae

    @staticmethod
    def backward(ctx, dv, da):
        _check_backward(ctx)
        pl, params = ctx.pl, ctx.params
        inputs = (ctx.video, ctx.audio, dv.contiguous(), da.contiguous())
        eng = ctx.eng
        gflat = _engine_flat(eng, pl) if eng is not None else None
        if gflat is not None:
            eng._plan_backward(pl, ctx.fa, inputs)
            ctx.fa = None
            return (None, None, None) + (None,) * len(params)
        return _autograd_backward(ctx, inputs, 3)


def _cached(model, name, make):
    """``model.__dict__[name]``, made by ``make()`` on first use (the module / parameter lists the per-call checks walk)."""
    v = model.__dict__.get(name)
    if v is None:
        v = model.__dict__[name] = make()
    return v


def _tree_ok(model, training=True):
    """No module hooked (a hook on any of them sends the call to the per-layer path, where each module's own ``__call__`` runs
    its hooks) and, for a ``training`` call, every module in training mode."""
    for m in _cached(model, "_avid_modules", lambda: list(model.modules())):
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks or (training and not m.training):
            return False
    return True


def _inputs_ok(inputs, audio_tower=False):
    """float32 GPU inputs — video [B,3,T,H,W], then audio [B,1,F,T] if there is one; the one spectrogram batch [B,1,T,F] of a
    single ``Conv2D`` tower (``audio_tower``) — and no graph being captured."""
    ranks = (4,) if audio_tower else (5, 4)
    if len(inputs) > len(ranks) or not all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == rank
                                           for x, rank in zip(inputs, ranks)):
        return False
    return not torch.cuda.is_current_stream_capturing()


def eligible(model, *inputs, need_grad=True):
    """The launch-program path applies: a training call (gradients on, unless ``need_grad`` is False: ``FinetuneStep`` runs
    the programs itself) on inputs the programs take (``_inputs_ok``) through the stock module tree, nothing hooked.  An
    input that requires a gradient sends the call to the per-layer path: the backward programs stop at the stems' weight
    gradients, ``ops._ConvCL.backward`` goes on to the clip / the spectrogram (``stem_dgrad_kernel``)."""
    if not ENABLED or not model.training or (need_grad and not torch.is_grad_enabled()):
        return False
    if need_grad and any(torch.is_tensor(x) and x.requires_grad for x in inputs):
        return False
    return _inputs_ok(inputs, _audio_tower(model)) and _tree_ok(model)


def _bn_identity(model):
    """The identity of the BatchNorm buffers a compiled plan's slot table points at: the address of the model's flat buffer
    when it keeps one (``AV_Wrapper._bn_flat``: the buffers are re-seated as its views), else every buffer's address
    (`.to()` / `.cuda()` re-create them)."""
    flat = getattr(model, "_bn_flat", None)
    if flat is not None:
        return flat.data_ptr()
    return tuple(b.data_ptr() for m in _cached(model, "_avid_modules", lambda: list(model.modules()))
                 for b in m._buffers.values() if b is not None)


def _plan_for(model, key, make):
    """The model's compiled plan for ``key`` (``make()`` compiles it on first use), or None: the caller takes the per-layer
    path.  (what a compiled plan froze besides shapes and switches — which parameters take gradients, their dtype,
    and the identity of the BatchNorm buffers its slot table points at: parameters frozen after the first step, `.double()`,
    `.cpu().cuda()` must not meet a stale program.  ~20 us per call for 141 parameters.)"""
    fp, dt_ok = 0, True
    for p in _cached(model, "_avid_param_list", lambda: list(model.parameters())):
        fp = (fp << 1) | int(p.requires_grad)
        dt_ok = dt_ok and p.dtype == torch.float32 and p.is_cuda
    if not dt_ok:
        return None
    key += (bool(ops.GROUP_WGRAD), ops.FUSE_BN_BWD, ops.wino_epoch(), fp, _bn_identity(model))
    plans = model.__dict__.setdefault("_avid_plans", {})
    pl = plans.get(key)
    if pl is None:
        try:
            pl = make()
        except Unsupported:
            pl = False
        plans[key] = pl
    return pl or None


def run(model, video, audio):
    """``AV_Wrapper.forward`` through the launch programs, or None when the model / call is outside what the compiler
    knows (the caller then takes the per-layer path)."""
    if not eligible(model, video, audio):
        return None
    eng = _ENGINE
    timing = lib.TIMING
    overlap = (not timing) and os.environ.get("AVID_OVERLAP_TOWERS", "1") == "1" and (eng is None or model.overlap_towers)
    trailing = (not timing) and bool(ops.DEFER_WGRAD)
    video, audio = video.contiguous(), audio.contiguous()
    pl = _plan_for(model, (tuple(video.shape), tuple(audio.shape), video.device.index, overlap, trailing),
                   lambda: Plan(model, video.shape, audio.shape, video.device, overlap, trailing, bool(ops.GROUP_WGRAD)))
    if pl is None or (eng is not None and _engine_flat(eng, pl) is None):
        return None                                   # (or the engine's gradient buffer is laid out differently)
    return NetFn.apply(video, audio, pl, *pl.params_fwd)


def dump(prog, n):
    """Readable listing of a program (debugging / tests)."""
    lines = []
    for k in range(n):
        r = prog[k]
        d = r.d
        geo = (f" [{d.B}x{d.Ti}x{d.Hi}x{d.Wi}x{d.Cin} -> {d.To}x{d.Ho}x{d.Wo}x{d.Cout} k{d.kt}{d.kh}{d.kw} s{d.st}{d.sh}{d.sw}]"
               if r.op in (3, 4, 5, 7) else "")
        refs = " ".join(f"{r.t[j].slot}:{r.t[j].off}" if r.t[j].slot >= 0 else "-" for j in range(NREF))
        lines.append(f"{k:4d} s{r.stream} {_OP_NAMES.get(r.op, r.op):12s}{geo} i={list(r.i)} n={list(r.n)} | {refs}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------
# fine-tuning: models.classification.ClassificationWrapper (utils/eval_utils.py:193-214 of the reference)
# ------------------------------------------------------------------------------------------------------------------
def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


class ClsPlan(TrainPrograms):
    """The compiled programs of one ``ClassificationWrapper`` around this package's ``R2Plus1D`` for one clip geometry, or around
    its ``Conv2D`` for one spectrogram geometry [B, 1, T, F] (``Builder.tower_fwd``; the input stays in slot ``S_VIDEO``, because
    the labels alias ``S_AUDIO``).

    Forward: the tower (``Builder.video_fwd`` / ``audio_fwd``), dropout, the classifier (``Builder.cls_linear_fwd``)
    — records [0, n_logits) — then ``AVID_OP_CLS_LOSS`` with ``dlogits`` (record n_logits, run by the step engine only).
    Backward, from ``dlogits``: the classifier's weight, bias and input gradients (one ``avid_cls_linear_bwd``), dropout's
    backward, the tower's backward (``TrainBuilder.tower_bwd``: ``video_bwd`` / ``video_stem_bwd``, or ``audio_bwd``).  ``classifier_only``: the reference's warm-up epochs — the
    tower still runs in training mode (its BatchNorm running statistics move) but no tower backward is compiled, the
    classifier's input gradient neither, and only the classifier's slice of the gradient buffer is zeroed."""

    def __init__(self, model, vshape, device, trailing, group, classifier_only=False, loss="ce", pos_weight=None,
                 label_smoothing=0.0):
        from models.classification import HipDropout
        cls = _classifier(model)
        self.loss, self.pos_weight = _loss_kind(loss, pos_weight, cls.weight.shape[0], label_smoothing), pos_weight
        self.label_smoothing = float(label_smoothing)
        if model.use_dropout and type(model.dropout) is not HipDropout:
            raise Unsupported("classifier / dropout")
        b = self._open(model, device, False, trailing, group)
        self.classifier_only = classifier_only
        self.vshape, self.ashape = tuple(vshape), None
        self.p = float(model.dropout.p) if model.use_dropout else 0.0
        # (parameters in reverse order: the classifier's bias and weight lead the gradient buffer)
        self.n_cls = b.goff[2] if len(b.params) > 2 else b.gnumel
        if classifier_only:
            b.fwd[self._zero_index].n[0] = 4 * self.n_cls
        # ------------------------------------------------------------------ forward
        V, feat = b.tower_fwd(model.feature_extractor, self.vshape)
        B, Fd = feat.shape
        self.drop_index = None
        if self.p > 0.0:
            y = b.fa.alloc(4 * B * Fd)
            self.mask = b.fa.alloc(B * Fd)
            self.drop_index = len(b.fwd)
            b.emit(OP_DROPOUT_FWD, n=(B, 0), i=(Fd, 0, 0), f=(self.p,), t=(feat.ref, y, self.mask, None))
            feat = Sym(y, (B, Fd))
        self.logits = b.cls_linear_fwd(cls, feat)
        self.n_classes = C = self.logits.shape[1]
        self.n_logits = len(b.fwd)
        b.loss(self.loss, self.logits, pos_weight=pos_weight, label_smoothing=label_smoothing)
        # ------------------------------------------------------------------ backward
        self._backward_begins(b)
        dlog = (S_DLOGITS, 0)
        dx = None if classifier_only else b.ba.alloc(4 * B * Fd)
        b.emit(OP_CLS_LINEAR_BWD, i=(B, Fd, C), t=(feat.ref, b.ext(cls.weight), dlog, dx, b.grad(cls.weight), b.grad(cls.bias)))
        b._ready(b.S, cls.weight, cls.bias)
        if not classifier_only:
            if self.p > 0.0:
                df = b.ba.alloc(4 * B * Fd)
                b.emit(OP_DROPOUT_BWD, n=(B * Fd,), f=(self.p,), t=(self.mask, dx, df))
                dx = df
            b.tower_bwd(V, dx)
        self._close(b)

    def forward(self, video, grad_flat, zero_grad, seed=0, offset=0, labels=None, out=None, dlogits=None, grad_scale=1.0,
                tables=True):
        """Issue the forward program — with ``labels`` also the loss record, which writes ``out`` (OUT_BYTES: loss, hits)
        and ``dlogits``; returns (logits, arena).  ``tables``: see ``_forward_arena``."""
        fa = self._forward_arena(grad_flat, zero_grad, (video, labels, dlogits, out), tables)
        if self.drop_index is not None:
            r = self.fwd_prog[self.drop_index]
            r.i[1], r.i[2], r.n[1] = _i32(seed), _i32(seed >> 32), int(offset)
        end = self.n_logits
        if labels is not None:
            self.fwd_prog[self.n_logits].f[0] = float(grad_scale)
            end = self.n_fwd
        self._run(self.fwd_prog, 0, end)
        return self._view(fa, self.logits), fa


class ClsFn(torch.autograd.Function):
    """video -> logits: ClassificationWrapper.forward in training mode with the tower, dropout, the classifier and all of
    their backward as two launch programs (``NetFn``'s shape with a single input)."""

    @staticmethod
    def forward(ctx, video, pl, seed, offset, *params):
        logits, fa = pl.forward(video, None, False, seed, offset)
        _remember(ctx, pl, fa, params)
        ctx.video = video
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        _check_backward(ctx)
        return _autograd_backward(ctx, (ctx.video, None, dlogits.contiguous(), None), 4)


def _loss_kind(loss, pos_weight, n_classes, label_smoothing=0.0):
    """The checked loss kind of a supervised plan: ``"ce"`` (softmax cross-entropy, int64 labels [B]), ``"bce"`` (binary
    cross-entropy with logits, float32 targets [B, C]; ``pos_weight``: float32 [C] on the parameters' device, or None) or
    ``"soft_ce"`` (softmax cross-entropy against float32 distributions [B, C]; ``label_smoothing`` in [0, 1))."""
    if loss not in ("ce", "bce", "soft_ce"):
        raise ValueError(f"loss must be 'ce', 'bce' or 'soft_ce' (got {loss!r})")
    if not isinstance(label_smoothing, (int, float)) or not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"label_smoothing must be a number in [0, 1) (got {label_smoothing!r})")
    if float(label_smoothing) != 0.0 and loss != "soft_ce":
        raise ValueError("label_smoothing belongs to loss='soft_ce'")
    if pos_weight is not None:
        if loss != "bce":
            raise ValueError("pos_weight belongs to loss='bce'")
        if (not isinstance(pos_weight, torch.Tensor) or pos_weight.dtype != torch.float32 or tuple(pos_weight.shape) != (n_classes,)
                or not pos_weight.is_contiguous()):
            raise ValueError(f"pos_weight must be a contiguous float32 tensor [{n_classes}]")
    return loss


def _loss_key(loss, pos_weight, label_smoothing=0.0):
    """What the loss kind adds to a plan's cache key: nothing for ``"ce"`` (the key of every plan compiled so far), the kind
    and the identity of the ``pos_weight`` tensor (an external slot of the program, which keeps it alive) for ``"bce"``, the
    kind and the smoothing (a constant of the loss record) for ``"soft_ce"``."""
    if loss == "soft_ce":
        return (loss, float(label_smoothing))
    return () if loss == "ce" else (loss, None if pos_weight is None else id(pos_weight))


def cls_plan(model, video, classifier_only=False, need_grad=True, loss="ce", pos_weight=None, label_smoothing=0.0):
    """The cached ``ClsPlan`` of this call (same staleness rules as ``run``), or None: the caller takes the per-layer path."""
    if not eligible(model, video, need_grad=need_grad):
        return None
    trailing = (not lib.TIMING) and bool(ops.DEFER_WGRAD)
    drop = model.dropout.p if model.use_dropout else 0.0
    return _plan_for(model, ("cls", tuple(video.shape), video.device.index, trailing, bool(classifier_only), drop)
                     + _loss_key(loss, pos_weight, label_smoothing),
                     lambda: ClsPlan(model, tuple(video.shape), video.device, trailing, bool(ops.GROUP_WGRAD), classifier_only,
                                     loss, pos_weight, label_smoothing))


def run_cls(model, video):
    """``ClassificationWrapper.forward`` through the launch programs, or None (the caller takes the per-layer path)."""
    if not eligible(model, video):
        return None
    video = video.contiguous()
    pl = cls_plan(model, video)
    if pl is None:
        return None
    seed, offset = (model.dropout.seed, model.dropout.next_offset()) if pl.drop_index is not None else (0, 0)
    return ClsFn.apply(video, pl, seed, offset, *pl.params_fwd)


# ------------------------------------------------------------------------------------------------------------------
# linear probe: models.linear_probe.MOSTModel (utils/eval_utils.py:217-242, 298-329 of the reference)
# ------------------------------------------------------------------------------------------------------------------
class ProbePlan(TrainPrograms):
    """The compiled programs of one ``MOSTModel`` in its stock form around this package's ``R2Plus1D`` for one clip geometry, or
    around its ``Conv2D`` for one spectrogram geometry (``AdaptiveMaxPool2d((h, w))`` heads: the taps are [B, 1, H, W, C] and pool
    with T = To = 1 into the reference's (C, h, w) flatten order).

    Forward: the training-mode tower (``Builder.tower_fwd``; the stage outputs it materialises anyway are the taps), then per
    tap ``Builder.probe_head_fwd`` — records [0, n_logits) — then one ``AVID_OP_CLS_LOSS`` with ``dlogits`` per tap (run by the step
    engine only).  Backward, from ``dlogits``, per tap: ``avid_probe_linear_bwd`` (weight, bias and input gradient),
    ``avid_bn1d_bwd`` (no input gradient: the pooled features are constants).  No tower record: the tower is frozen.  The
    gradient buffer holds the classifiers' parameters only (``FlatParams`` over the trainable ones)."""

    def __init__(self, model, vshape, device, trailing, group, loss="ce", pos_weight=None, label_smoothing=0.0):
        classifiers = _probe_heads(model)
        self.loss = _loss_kind(loss, pos_weight, classifiers[0].classifier.weight.shape[0], label_smoothing)
        self.pos_weight, self.label_smoothing = pos_weight, float(label_smoothing)
        if any(p.requires_grad for p in model.feature_extractor.parameters()):
            raise Unsupported("the probe's tower is not frozen")
        b = self._open(model, device, False, trailing, group, frozen_ok=True)
        self.vshape, self.ashape = tuple(vshape), None
        # ------------------------------------------------------------------ forward
        V, _ = b.tower_fwd(model.feature_extractor, self.vshape)
        B = vshape[0]
        self.n_classes = C = classifiers[0].classifier.weight.shape[0]
        if C > 1024:
            raise Unsupported("more classes than avid_cls_loss takes")
        if B < 2:
            raise Unsupported("probe head geometry")          # (BatchNorm1d on batch statistics)
        heads = []
        for c in classifiers:
            h = V["stages"][c.feat_name]
            if h.affine is not None:
                raise Unsupported("tap not materialised")
            heads.append(b.probe_head_fwd(c, h, C, True))
        self.logits = [hd["logits"] for hd in heads]
        self.n_logits = len(b.fwd)
        for i, lg in enumerate(self.logits):
            b.loss(self.loss, lg, tap=i, pos_weight=pos_weight, label_smoothing=label_smoothing)
        # ------------------------------------------------------------------ backward
        self._backward_begins(b)
        for i, hd in enumerate(heads):
            bn, lin, Fd = hd["c"].bn, hd["c"].classifier, hd["Fd"]
            dn = b.ba.alloc(4 * B * Fd)
            b.emit(OP_PROBE_LINEAR_BWD, i=(B, Fd, C),
                   t=(hd["normed"], b.ext(lin.weight), (S_DLOGITS, 4 * B * C * i), dn, b.grad(lin.weight), b.grad(lin.bias)))
            b._ready(b.S, lin.weight, lin.bias)
            b.emit(OP_BN1D_BWD, i=(B, Fd, 0), f=(0.0, bn.eps),
                   t=(hd["pooled"], dn, b.ext(bn.weight), hd["save2"], None, b.grad(bn.weight), b.grad(bn.bias)))
            b._ready(b.S, bn.weight, bn.bias)
        self._close(b)

    def forward(self, video, grad_flat, zero_grad, labels=None, out=None, dlogits=None, tables=True):
        """Issue the forward program — with ``labels`` also the loss records, which write ``out`` ([n_taps] x PROBE_OUT_BYTES:
        loss, hits) and ``dlogits [n_taps, B, C]``; returns ([logits per tap], arena).  ``tables``: see ``_forward_arena``."""
        fa = self._forward_arena(grad_flat, zero_grad, (video, labels, dlogits, out), tables)
        self._run(self.fwd_prog, 0, self.n_fwd if labels is not None else self.n_logits)
        return [self._view(fa, lg) for lg in self.logits], fa


class ProbeFn(torch.autograd.Function):
    """video -> logits of every tap: ``MOSTModel.forward`` in training mode with the tower, the pools, the heads and the heads'
    backward as two launch programs."""

    @staticmethod
    def forward(ctx, video, pl, *params):
        logits, fa = pl.forward(video, None, False)
        _remember(ctx, pl, fa, params)
        ctx.video = video
        return tuple(logits)

    @staticmethod
    def backward(ctx, *dlogits):
        _check_backward(ctx)
        B, C = ctx.pl.vshape[0], ctx.pl.n_classes
        dl = torch.stack([d.contiguous() if d is not None else torch.zeros((B, C), dtype=torch.float32, device=ctx.video.device)
                          for d in dlogits])
        return _autograd_backward(ctx, (ctx.video, None, dl, None), 2)


def probe_plan(model, video, need_grad=True, loss="ce", pos_weight=None, label_smoothing=0.0):
    """The cached ``ProbePlan`` of this call (same staleness rules as ``run``), or None: the caller takes the per-layer path."""
    if not eligible(model, video, need_grad=need_grad):
        return None
    trailing = (not lib.TIMING) and bool(ops.DEFER_WGRAD)
    return _plan_for(model, ("probe", tuple(video.shape), video.device.index, trailing) + _loss_key(loss, pos_weight, label_smoothing),
                     lambda: ProbePlan(model, tuple(video.shape), video.device, trailing, bool(ops.GROUP_WGRAD), loss, pos_weight,
                                       label_smoothing))


def run_probe(model, video):
    """``MOSTModel.forward`` through the launch programs: {feat_name: logits}, or None (the caller takes the per-layer path)."""
    if not eligible(model, video):
        return None
    video = video.contiguous()
    pl = probe_plan(model, video)
    if pl is None:
        return None
    logits = ProbeFn.apply(video, pl, *pl.params_fwd)
    return dict(zip(model.feat_names, logits))


# ------------------------------------------------------------------------------------------------------------------
# inference: eval-mode forward programs (parallel.Inference, the engines' evaluate())
# ------------------------------------------------------------------------------------------------------------------
class EvalPlan(Programs):
    """The compiled inference program of one model for one input geometry: ``R2Plus1D`` or ``Conv2D`` (pooled features; wherever
    ``R2Plus1D`` stands as a wrapper's tower below, ``Conv2D`` on spectrograms [B, 1, T, F] is compiled too), ``AV_Wrapper`` (the two
    embeddings; the audio tower on its own stream and its own buffers), ``ClassificationWrapper(R2Plus1D, feat_name='pool',
    pooling_op=None)`` (logits; dropout is the identity in eval mode) or the stock ``MOSTModel`` (every tap's logits:
    ``Builder.probe_head_fwd`` with training = 0).  Record 0 is the batched BatchNorm-coefficient launch — it
    runs on every call, because running statistics move between evaluations — record 1 the weight-transform launch (the
    pre-split weights of the layers that read them).  Activations live in a RECYCLED arena (``_recycle``); what leaves the program
    lives in a buffer of its own (slot ``S_OUT``), so the caller's results do not keep the arena alive.  There is no backward
    program and no gradient buffer: this is ``Programs``, not ``TrainPrograms``."""

    def __init__(self, model, vshape, ashape, device):
        from models.av_wrapper import AV_Wrapper
        from models.classification import ClassificationWrapper
        from models.linear_probe import MOSTModel
        from models.audio import Conv2D
        from models.video import R2Plus1D
        dry = device.type != "cuda"
        if not all((p.is_cuda or dry) and p.dtype == torch.float32 for p in model.parameters()):
            raise Unsupported("non-fp32 / CPU parameters")
        self.device, self.vshape, self.ashape = device, tuple(vshape), None if ashape is None else tuple(ashape)
        b = EvalBuilder(device)
        self._coef_rec = b.emit(OP_BN_EVAL_COEFFS, i=(0,), t=((S_AUX, 0),))
        self._wt_rec = b.emit(OP_WT_BATCH, i=(0,), n=(0,), t=((S_AUX, 0),))
        video = Sym((S_VIDEO, 0), vshape)
        if type(model) in (R2Plus1D, Conv2D):
            _, feat = b.tower_fwd(model, self.vshape, arena=b.oa)
            # [B, C, 1, 1, 1] (R2Plus1D) / [B, C, 1, 1] (Conv2D), as the module returns them
            outs = [Sym(feat.ref, feat.shape + ((1, 1) if type(model) is Conv2D else (1, 1, 1)))]
        elif type(model) is ClassificationWrapper:
            cls = _classifier(model)
            _, feat = b.tower_fwd(model.feature_extractor, self.vshape)
            outs = [b.cls_linear_fwd(cls, feat, arena=b.oa)]
        elif type(model) is AV_Wrapper:
            if not model.use_linear_proj or ashape is None:
                raise Unsupported("no projection heads")
            audio = Sym((S_AUDIO, 0), (ashape[0], ashape[1], 1, ashape[2], ashape[3]))
            A_S = ST_MAIN if lib.TIMING else ST_AUDIO
            outs = [None, None]

            def start_audio():                      # behind the video stem, as in training (models/av_wrapper.py AUDIO_AFTER)
                b.wait(A_S, ST_MAIN)
                b.S = A_S
                _, afeat = b.audio_fwd(model.audio_model, audio)
                outs[1] = b.head_fwd(model.audio_proj, afeat, arena=b.oa)[1]
                b.S = ST_MAIN
            _, vfeat = b.video_fwd(model.video_model, video, after_stem=start_audio)
            outs[0] = b.head_fwd(model.video_proj, vfeat, arena=b.oa)[1]
            b.wait(ST_MAIN, A_S)
        elif type(model) is MOSTModel:
            heads = _probe_heads(model)
            V, _ = b.tower_fwd(model.feature_extractor, self.vshape)
            Cn = heads[0].classifier.weight.shape[0]
            self.out_names = list(model.feat_names)
            outs = [b.probe_head_fwd(c, V["stages"][c.feat_name], Cn, False, arena=b.oa)["logits"] for c in heads]
        else:
            raise Unsupported(type(model).__name__)
        self.outputs = [(o.ref[1], o.shape) for o in outs]
        # ------------------------------------------------------------------ the arena, then the tables and the record array
        self.n_fwd = len(b.fwd)
        self.virtual_bytes = b.fa.size                       # what a bump allocator would take
        self.fa_bytes, self.buffers = self._recycle(b.fwd, b.fa.bufs, S_FWD)
        self.fa_bytes = max(self.fa_bytes, 256)
        self.out_bytes = max(b.oa.size, 256)
        (self.fwd_prog,) = self._seal(b, b.fwd)
        self._bn_ptrs = None

    def _aux_layout(self, b):
        """aux: transformed weights | BatchNorm vectors (both at the builder's offsets) | weight-transform table | BatchNorm table,
        which the coefficient record (record 0) reads."""
        self.bn_recs = b.bn_recs
        self.bn_table_off = self.table_off + _align(32 * len(b.wt_recs) + 32)
        self._coef_rec.i[0] = len(b.bn_recs)
        self._coef_rec.t[0].off = self.bn_table_off
        if not b.bn_recs:
            self._coef_rec.op = 0
        return self.bn_table_off + C.sizeof(lib.BnEvalItem) * len(b.bn_recs) + 256

    @staticmethod
    def _recycle(recs, bufs, slot):
        """Map the virtual buffers of ``slot`` to physical offsets: a buffer takes the bytes of an earlier one of the same aligned
        size whose last record has been emitted on the same stream, else new bytes.  A record's outputs are placed BEFORE the
        buffers it reads last are released.  Returns (arena bytes, [(physical offset, bytes, stream, first, last record)])."""
        import bisect
        starts = [o for o, _ in bufs]
        first, last, streams = {}, {}, {}
        refs = []
        for k, r in enumerate(recs):
            if r.op in (0, OP_WAIT):
                continue
            for j in range(NREF):
                if r.t[j].slot == slot:
                    bi = bisect.bisect_right(starts, r.t[j].off) - 1
                    refs.append((k, j, bi))
                    first.setdefault(bi, k)
                    last[bi] = k
                    streams.setdefault(bi, set()).add(r.stream)
        release = {}
        for bi, k in last.items():
            release.setdefault(k, []).append(bi)
        last_ref = {k: j for k, j, _ in refs}                # a record's last reference into the slot
        free, phys, top = {}, {}, 0
        for k, j, bi in refs:
            if bi not in phys:
                n = bufs[bi][1]
                pool = free.get((recs[k].stream, n)) if len(streams[bi]) == 1 else None
                if pool:
                    phys[bi] = pool.pop()
                else:
                    phys[bi], top = top, top + n
            recs[k].t[j].off = phys[bi] + (recs[k].t[j].off - bufs[bi][0])
            if j == last_ref[k] and k in release:            # every buffer of the record is placed: release what it read last
                for b2 in release[k]:
                    if len(streams[b2]) == 1:
                        free.setdefault((recs[k].stream, bufs[b2][1]), []).append(phys[b2])
        return top, [(phys[bi], bufs[bi][1], min(streams[bi]), first[bi], last[bi]) for bi in sorted(phys)]

    def _refresh_bn_table(self):
        """The device table of the coefficient launch follows the BatchNorms' current parameter and buffer addresses."""
        ptrs = tuple(t.data_ptr() for bn, _ in self.bn_recs for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        if ptrs != self._bn_ptrs and self.bn_recs:
            base = self.aux.data_ptr()
            recs = [lib.BnEvalItem(ptrs[4 * k], ptrs[4 * k + 1], ptrs[4 * k + 2], ptrs[4 * k + 3], base + off, float(bn.eps),
                                   bn.num_features) for k, (bn, off) in enumerate(self.bn_recs)]
            ops.bn_eval_table(recs, self.device, out=self.aux[self.bn_table_off:])
            self._bn_ptrs = ptrs

    def forward(self, video, audio=None):
        """Issue the program; returns the outputs (views of a fresh output buffer)."""
        self._refresh_table()
        self._refresh_bn_table()
        fa = torch.empty(self.fa_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(self.out_bytes, dtype=torch.uint8, device=self.device)
        self._fill_slots(fa, None, None, (video, audio, None, out))
        self._streams()
        self._run(self.fwd_prog, 0, self.n_fwd)
        res = []
        for off, shape in self.outputs:
            n = 1
            for v in shape:
                n *= v
            res.append(out[off:off + 4 * n].view(torch.float32).view(shape))
        return res


def eval_plan(model, *inputs):
    """The cached ``EvalPlan`` of this call, or None: the caller takes the per-layer path.  Staleness as the training plans'
    (``_plan_for``: dtype, device, which parameters take gradients, BatchNorm buffer identity, the dispatch epoch that
    ``ops.wino_configure`` / ``tconv_configure`` / ``set_cu_budget`` bump); the key's leading "eval" keeps it apart from theirs."""
    if not EVAL_ENABLED or not ENABLED or not inputs or len(inputs) > 2:
        return None
    if not _inputs_ok(inputs, _audio_tower(model)) or not _tree_ok(model, training=False):
        return None
    shapes = tuple(tuple(x.shape) for x in inputs)
    dev = inputs[0].device
    return _plan_for(model, ("eval",) + shapes + (dev.index, bool(lib.TIMING)),
                     lambda: EvalPlan(model, shapes[0], shapes[1] if len(shapes) > 1 else None, dev))


def run_eval(model, *inputs):
    """``model.eval()(*inputs)`` under ``torch.no_grad()`` through an inference program: the output tensor (``R2Plus1D``, ``Conv2D``,
    ``ClassificationWrapper``), the tuple of embeddings (``AV_Wrapper``) or the dict of logits (``MOSTModel``); None when the model / call is outside what the
    compiler knows.  Reached only from ``parallel.Inference``: ``model(x)`` in eval mode stays on the per-layer path."""
    pl = eval_plan(model, *inputs)
    if pl is None:
        return None
    seat = getattr(model, "_seat_flat_buffers", None)
    if seat is not None:
        seat()
    with torch.no_grad():
        res = pl.forward(*[x.contiguous() for x in inputs])
    names = getattr(pl, "out_names", None)
    if names is not None:                          # MOSTModel: {feat_name: logits}
        return dict(zip(names, res))
    return res[0] if len(res) == 1 else tuple(res)
