"""Linear-probe evaluation model on gfx950 kernels (reference: utils/eval_utils.py:217-242 ``Classifier``, 298-329 ``MOSTModel``;
driven by eval-action-recg-linear.py with configs/benchmark/kinetics/8x224x224-linear.yaml, model ``MOSTWrapper``).

``MOSTModel(feature_extractor, n_classes, feat_names, feat_dims, pooling_ops, l2_norm=None, use_bn=False, use_dropout=False)``
has the reference's constructor, attribute names, ``state_dict`` keys and shapes (``feature_extractor.*``,
``classifiers.<i>.bn.*``, ``classifiers.<i>.classifier.*``) and ``forward(video) -> {feat_name: logits}``.  The tower is
frozen (``requires_grad=False``) and runs under ``no_grad``; the constructor puts it in eval mode and — exactly as in the
reference — ``model.train()`` puts it back in training mode, so during probe training its BatchNorms use batch statistics
and move their running statistics.  That quirk is the published protocol; ``train()`` is ``nn.Module``'s.

* The stock case — every pooling op an ``AdaptiveMaxPool3d((t, h, w))`` string, no ``l2_norm``, no dropout, GPU float32
  taps — pools each channels-last tap straight into the reference's flatten order (``avid_adaptive_maxpool_fwd``: no NCDHW
  copy of the tap), then ``avid_bn1d_*`` and ``avid_probe_linear_*`` (matrix pipe, any number of classes).
* A training call of that stock model around this package's ``R2Plus1D`` — every module in training mode, nothing hooked,
  gradients on — runs the tower, the pools and the heads as one forward launch program and the heads' backward as another
  (``avid_hip.plan.ProbePlan``); so does one around this package's ``Conv2D`` on spectrograms ``[B, 1, T, F]`` whose pooling
  ops are ``AdaptiveMaxPool2d((h, w))`` strings (sound classification: the taps are 2-D); ``avid_hip.parallel.ProbeStep``
  adds the four losses and Adam.  Every other call (eval, a hook, a tower put in eval mode by hand) walks the modules, the
  tower with ``return_embs``.
* Any other pooling string, ``l2_norm``, ``use_dropout`` or ``use_bn=False`` takes the torch ops exactly as the reference
  builds them (correct, not fast), and so do CPU tensors; the BatchNorm1d and Linear of a GPU batch still run on the
  kernels above.
"""
import re

import torch
import torch.nn as nn

from avid_hip import ops

__all__ = ["MOSTModel", "Classifier", "ProbeBatchNorm1d", "ProbeLinear"]

_ADAPTIVE = re.compile(r"^\s*AdaptiveMaxPool3d\(\s*\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)\s*\)\s*$")
_ADAPTIVE_2D = re.compile(r"^\s*AdaptiveMaxPool2d\(\s*\(\s*(\d+)\s*,\s*(\d+)\s*\)\s*\)\s*$")


def _pool_size(pooling):
    """(t, h, w) of an ``AdaptiveMaxPool3d((t, h, w))`` string, (1, h, w) of an ``AdaptiveMaxPool2d((h, w))`` string (the audio
    tower's taps have no time axis of their own), None for anything else."""
    if not isinstance(pooling, str):
        return None
    m = _ADAPTIVE.match(pooling)
    if m:
        return tuple(int(v) for v in m.groups())
    m = _ADAPTIVE_2D.match(pooling)
    return (1,) + tuple(int(v) for v in m.groups()) if m else None


class ProbeBatchNorm1d(nn.BatchNorm1d):
    """``nn.BatchNorm1d(feat_dim)`` — its parameters, buffers and defaults — computed by ``avid_bn1d_fwd_train`` / ``_eval`` /
    ``_bwd`` for a float32 GPU batch ``[B, F]`` (the tower's BatchNorm kernels stop at 1024 channels; the heads have 8192 / 9216)."""

    def forward(self, x):
        if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and self.affine and self.track_running_stats
                and self.momentum is not None):
            return super().forward(x)
        return ops.bn1d(x, self.weight, self.bias, self.running_mean, self.running_var, self.training, self.momentum, self.eps,
                        self.num_batches_tracked if self.training else None)


class ProbeLinear(nn.Linear):
    """``nn.Linear(feat_dim, n_classes)`` — its keys and initialisation — computed by ``avid_probe_linear_fwd`` / ``_bwd`` for a
    float32 GPU batch (B <= 256, feat_dim <= 16384; anything larger is an error, not a fall-back)."""

    def forward(self, x):
        if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32):
            return super().forward(x)
        return ops.probe_linear(x, self.weight, self.bias)


class Classifier(nn.Module):
    def __init__(self, n_classes, feat_name, feat_dim, pooling, l2_norm=False, use_bn=True, use_dropout=False):
        super().__init__()
        self.use_bn = use_bn
        self.feat_name = feat_name
        self.pooling = eval("nn." + pooling, {"nn": nn, "torch": torch}) if pooling is not None else None
        self.pool_size = _pool_size(pooling)
        self.l2_norm = l2_norm
        if use_bn:
            self.bn = ProbeBatchNorm1d(feat_dim)
        self.use_dropout = use_dropout
        if use_dropout:
            self.dropout = nn.Dropout()
        self.classifier = ProbeLinear(feat_dim, n_classes)

    def on_kernels(self, x):
        """The pooling of this tap runs as ``avid_adaptive_maxpool_fwd``: the stock head on a float32 GPU tap, pooling unhooked."""
        p = self.pooling
        return (self.pool_size is not None and not self.use_dropout and not self.l2_norm and x.is_cuda and x.dim() == 5
                and x.dtype == torch.float32 and type(p) is nn.AdaptiveMaxPool3d
                and not (p._forward_hooks or p._forward_pre_hooks))

    def pooled(self, x):
        """The reference's no_grad block: dropout, normalize, pooling, ``view(B, -1)`` in NCDHW order."""
        with torch.no_grad():
            if self.on_kernels(x):
                # the tower hands out the NCDHW view of a channels-last tensor: pooled where it lies
                x = ops.adaptive_maxpool(x.permute(0, 2, 3, 4, 1).contiguous(), self.pool_size)
                return x.detach()
            if self.use_dropout:
                x = self.dropout(x)
            if self.l2_norm:
                x = nn.functional.normalize(x, p=2, dim=-1)
            if self.pooling is not None and len(x.shape) > 2:
                x = self.pooling(x)
            return x.reshape(x.shape[0], -1).contiguous().detach()

    def forward(self, x):
        x = self.pooled(x)
        if self.use_bn:
            x = self.bn(x)
        return self.classifier(x)


class MOSTModel(nn.Module):
    def __init__(self, feature_extractor, n_classes, feat_names, feat_dims, pooling_ops, l2_norm=None, use_bn=False,
                 use_dropout=False):
        super().__init__()
        assert len(feat_dims) == len(pooling_ops) == len(feat_names)
        n_outputs = len(feat_dims)
        self.feat_names = feat_names
        self.feat_dims = feat_dims
        self.pooling_ops = pooling_ops
        if l2_norm is None:
            l2_norm = [False] * len(feat_names)
        if not isinstance(l2_norm, list):
            l2_norm = [l2_norm] * len(feat_names)
        self.l2_norm = l2_norm

        feature_extractor.train(False)
        self.feature_extractor = feature_extractor

        self.classifiers = nn.ModuleList([
            Classifier(n_classes, feat_name=feat_names[i], feat_dim=feat_dims[i], pooling=pooling_ops[i], l2_norm=l2_norm[i],
                       use_bn=use_bn, use_dropout=use_dropout) for i in range(n_outputs)])

        for p in self.feature_extractor.parameters():
            p.requires_grad = False

    def forward(self, *x):
        if len(x) == 1 and torch.is_tensor(x[0]):
            from avid_hip import plan
            out = plan.run_probe(self, x[0])       # a training call of the stock model: two launch programs
            if out is not None:
                return out
        with torch.no_grad():
            embs = self.feature_extractor(*x, return_embs=self.feat_names)
            embs = {ft: embs[ft] for ft in self.feat_names}
        for classifier, ft in zip(self.classifiers, self.feat_names):
            embs[ft] = classifier(embs[ft])
        return embs
