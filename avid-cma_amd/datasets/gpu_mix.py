"""Mixup (Zhang et al. 2018) and CutMix (Yun et al. 2019) of a batch that is already on the GPU: the sampler of
``avid_batch_mix`` (``avid_hip.ops.batch_mix``).  The reference has no batch-level augmentation; the conventions are the
published ones (timm's ``Mixup``: one switch between the two, ``lam ~ Beta(alpha, alpha)``, CutMix's ``lam`` recomputed from the
clipped box).

Every random number is drawn on the HOST from one ``numpy.random.Generator(PCG64(seed))``, in this order per call:

1. ``u = random()``: the batch is mixed iff ``u < prob``.  A batch that is not mixed draws nothing more.
2. only when both alphas are positive, ``s = random()``: CutMix iff ``s < switch_prob`` (otherwise the one positive alpha decides).
3. ``lam = beta(alpha, alpha)`` — one draw, or ``beta(alpha, alpha, size=B)`` with ``per_sample``.
4. ``perm = permutation(B)``.
5. CutMix only, per box (one, or B with ``per_sample``): ``cy = integers(H)`` (all boxes), then ``cx = integers(W)`` (all boxes).
   The cut is ``int(H * r)`` x ``int(W * r)`` with ``r = sqrt(1 - lam)``, centred on (cy, cx) and clipped to the plane;
   ``lam`` is then RECOMPUTED as ``1 - box_area / (H * W)`` (a clipped box covers less than ``1 - lam`` of the plane).

The device sees three small arrays (``perm`` int64 [B], ``lam`` float32 [B], ``box`` int32 [B, 4]) and one launch; nothing
waits for the GPU.  A batch that is not mixed still goes through the kernel (the identity permutation, ``lam = 1``, empty boxes:
an exact copy), so the output is always a fresh tensor and the targets always float32 [B, n_classes]."""
import math

import numpy as np
import torch


class GpuBatchMix:
    """``GpuBatchMix(n_classes, ...)(x, labels_or_targets) -> (x_mixed, targets [B, n_classes] float32)``.

    ``x``: clips [B, C, T, H, W] or spectrograms [B, 1, T, F] (float32, on the GPU); the (H, W) plane of CutMix is the last two
    dimensions.  ``labels_or_targets``: int64 labels [B] or float32 targets [B, n_classes] on the same device.
    ``mixup_alpha`` / ``cutmix_alpha``: the Beta parameters, 0 switches the mode off (both 0: no batch is ever mixed);
    ``prob``: the probability that a batch is mixed; ``switch_prob``: that of CutMix when both modes are on; ``per_sample``: one
    ``lam`` (and box) per sample instead of one per batch.  ``state_dict()`` / ``load_state_dict()`` carry the generator's state:
    a restored sampler continues the sequence.  ``last`` holds the host arrays of the last call (mode, perm, lam, box)."""

    def __init__(self, n_classes, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5, per_sample=False, seed=0):
        if int(n_classes) < 1:
            raise ValueError("GpuBatchMix: n_classes must be >= 1")
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0 and math.isfinite(mixup_alpha) and math.isfinite(cutmix_alpha)):
            raise ValueError(f"GpuBatchMix: the alphas must be finite and >= 0 (got {mixup_alpha!r}, {cutmix_alpha!r})")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError(f"GpuBatchMix: prob and switch_prob must be in [0, 1] (got {prob!r}, {switch_prob!r})")
        self.n_classes = int(n_classes)
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.per_sample = float(prob), float(switch_prob), bool(per_sample)
        self.seed = int(seed)
        self.rng = np.random.Generator(np.random.PCG64(self.seed))
        self.last = None

    # ---- the draws (host only)
    def draw(self, B, H, W):
        """The draws of one call, in the documented order: ``(mode, perm int64 [B], lam float32 [B], box int32 [B, 4])`` with
        mode ``None`` (not mixed), ``"mixup"`` or ``"cutmix"``."""
        rng = self.rng
        perm = np.arange(B, dtype=np.int64)
        lam = np.ones(B, np.float32)
        box = np.zeros((B, 4), np.int32)
        u = rng.random()
        if not (u < self.prob) or (self.mixup_alpha <= 0.0 and self.cutmix_alpha <= 0.0):
            return None, perm, lam, box
        if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
            cut = bool(rng.random() < self.switch_prob)
        else:
            cut = self.cutmix_alpha > 0.0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        k = B if self.per_sample else 1
        lam64 = np.broadcast_to(np.asarray(rng.beta(alpha, alpha, size=k), np.float64), (k,)).copy()
        perm = rng.permutation(B).astype(np.int64)
        if cut:
            cy, cx = rng.integers(H, size=k), rng.integers(W, size=k)
            r = np.sqrt(1.0 - lam64)
            ch, cw = (H * r).astype(np.int64), (W * r).astype(np.int64)
            h0, h1 = np.clip(cy - ch // 2, 0, H), np.clip(cy - ch // 2 + ch, 0, H)
            w0, w1 = np.clip(cx - cw // 2, 0, W), np.clip(cx - cw // 2 + cw, 0, W)
            lam64 = 1.0 - ((h1 - h0) * (w1 - w0)).astype(np.float64) / float(H * W)
            box[:] = np.stack([h0, h1, w0, w1], 1).astype(np.int32)          # (k = 1: the one box for every sample)
        lam[:] = lam64.astype(np.float32)
        return ("cutmix" if cut else "mixup"), perm, lam, box

    def __call__(self, x, labels_or_targets):
        from avid_hip import ops
        if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
            raise ValueError("GpuBatchMix: x must be clips [B, C, T, H, W] or spectrograms [B, 1, T, F]")
        B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        y = labels_or_targets
        if not isinstance(y, torch.Tensor) or y.shape[0] != B or not (
                (y.dtype == torch.int64 and y.dim() == 1) or (y.dtype == torch.float32 and tuple(y.shape) == (B, self.n_classes))):
            raise ValueError(f"GpuBatchMix: labels int64 [{B}] or targets float32 [{B}, {self.n_classes}] expected")
        mode, perm, lam, box = self.draw(B, H, W)
        self.last = (mode, perm, lam, box)
        dev = x.device
        up = lambda a: torch.from_numpy(a).to(dev, non_blocking=True)         # noqa: E731
        # (not mixed: CutMix with empty boxes, an exact copy whatever x holds)
        box_d = None if mode == "mixup" else up(box)
        if y.dtype == torch.int64:
            return ops.batch_mix(x, up(perm), up(lam), box=box_d, labels=y, n_classes=self.n_classes)
        return ops.batch_mix(x, up(perm), up(lam), box=box_d, targets=y, n_classes=self.n_classes)

    # ---- checkpoints
    def state_dict(self):
        return {"bit_generator": self.rng.bit_generator.state, "seed": self.seed}

    def load_state_dict(self, sd):
        self.rng.bit_generator.state = sd["bit_generator"]
        self.seed = int(sd.get("seed", self.seed))
