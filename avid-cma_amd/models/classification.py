"""Action-recognition fine-tuning model on gfx950 kernels (reference: utils/eval_utils.py:193-214).

``ClassificationWrapper(feature_extractor, n_classes, feat_name, feat_dim, pooling_op=None, use_dropout=False, dropout=0.5)``
has the reference's constructor, ``state_dict`` keys and shapes (``feature_extractor.*``, ``classifier.weight``,
``classifier.bias``) and ``forward(video) -> logits [B, n_classes]``.

* A training call on the GPU through the stock tree (``feat_name="pool"``, no pooling op, this package's ``R2Plus1D`` on
  clips or its ``Conv2D`` on spectrograms ``[B, 1, T, F]``, fp32 trainable parameters, nothing hooked) runs as two launch
  programs: the tower, dropout and the classifier forward, and their mirror image backward (``avid_hip.plan.ClsPlan``), one
  autograd node.
* The classifier is a ``ClsLinear`` (``nn.Linear``'s keys and initialisation) computed by ``avid_cls_linear_fwd`` / ``_bwd``,
  which take any number of classes (the heads' igemm takes multiples of 64; UCF-101 and HMDB-51 have 101 and 51).
* Everything else takes the per-layer path with the HIP ops: evaluation, other ``feat_name`` values (the tower is asked
  for ``return_embs``), a pooling op (built from torch, as the reference does), hooks.  For ``feat_name="pool"`` the tower
  is called without ``return_embs``, so its BatchNorm hand-over stays on.

Dropout (``HipDropout``) draws its keep-mask from Philox4x32-10 with a seed taken from torch's CPU generator at
construction — so ``torch.manual_seed`` reproduces it — and an offset that advances by one per training forward.  The
masks follow ``torch.nn.Dropout``'s distribution (each element kept with probability 1 - p, scaled by 1 / (1 - p)) but
not its bits.  Neither the seed nor the offset is a ``state_dict`` entry.  In eval mode dropout is the identity.
"""
import torch
import torch.nn as nn

from avid_hip import ops
from .av_wrapper import LinearCL

__all__ = ["ClassificationWrapper", "ClsLinear", "HipDropout"]


class ClsLinear(LinearCL):
    """The classifier: ``nn.Linear(in_features, n_classes)``'s keys and default initialisation (``LinearCL``'s), computed by
    ``avid_cls_linear_fwd`` / ``_bwd``, which take any number of classes — the heads' igemm takes multiples of 64, and
    UCF-101 / HMDB-51 have 101 / 51.  A module, so that hooks registered on ``model.classifier`` run as in the reference."""

    def forward(self, x):
        return ops.cls_linear(x, self.weight, self.bias)


class HipDropout(nn.Module):
    """``torch.nn.Dropout(p)`` on ``avid_dropout_fwd`` / ``avid_dropout_bwd`` (see the module docstring for the masks)."""

    def __init__(self, p=0.5):
        super().__init__()
        if not 0.0 <= p < 1.0:
            raise ValueError(f"dropout probability {p} outside [0, 1)")
        self.p = float(p)
        self.seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        self.offset = 0

    def next_offset(self):
        off = self.offset
        self.offset += 1
        return off

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        return ops.dropout(x, self.p, self.seed, self.next_offset())

    def extra_repr(self):
        return f"p={self.p}"


class ClassificationWrapper(nn.Module):
    def __init__(self, feature_extractor, n_classes, feat_name, feat_dim, pooling_op=None, use_dropout=False, dropout=0.5):
        super().__init__()
        self.feature_extractor = feature_extractor
        self.feat_name = feat_name
        self.use_dropout = use_dropout
        self.pooling = eval("torch.nn." + pooling_op, {"torch": torch}) if pooling_op is not None else None
        self.classifier = ClsLinear(feat_dim, n_classes)
        if use_dropout:
            # (the seed is drawn AFTER the classifier's initialisation: the classifier starts from the same weights as the
            #  reference's under the same torch.manual_seed)
            self.dropout = HipDropout(dropout)

    def forward(self, *inputs):
        from avid_hip import plan
        out = plan.run_cls(self, inputs[0]) if len(inputs) == 1 else None
        if out is not None:
            return out
        video = inputs[0]
        if self.feat_name == "pool" and self.pooling is None:
            emb = self.feature_extractor(*inputs)
        else:
            emb = self.feature_extractor(*inputs, return_embs=True)[self.feat_name]
        emb_pool = self.pooling(emb) if self.pooling is not None else emb
        emb_pool = emb_pool.reshape(video.shape[0], -1)
        if self.use_dropout:
            emb_pool = self.dropout(emb_pool)
        return self.classifier(emb_pool)
