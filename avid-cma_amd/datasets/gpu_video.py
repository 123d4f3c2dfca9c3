"""GPU-side tail of the reference's video preprocessing (datasets/preprocessing.py:45-48):
``volume_transforms.ClipToTensor()`` + ``tensor_transforms.Normalize(mean, std)`` for a whole batch of decoded,
already cropped / augmented uint8 clips in ONE HBM-bound kernel (avid_clip_normalize), bit-identical to the CPU
transform.  With it the DataLoader workers hand over uint8 frames (a quarter of the bytes of the fp32 tensor over
PCIe) and the float conversion happens on the training stream right before ``model(video, audio)``."""
import collections
import math
import numbers
import random

import numpy as np
import torch

from avid_hip import lib, ops

__all__ = ["ClipToTensorNormalize", "ClipAugParams", "GpuVideoPrep_MSC_CJ", "GpuVideoPrep_Crop_CJ", "RawFrames",
           "collate_raw_clips"]


class ClipToTensorNormalize:
    """``__call__(frames)``: ``frames`` uint8 ``[B, T, H, W, 3]`` (or one clip ``[T, H, W, 3]``) on the GPU ->
    fp32 ``[B, 3, T, H, W]`` (``[3, T, H, W]``): ((u / 255) - mean) / std per channel."""

    def __init__(self, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.mean, self.std = tuple(mean), tuple(std)

    def __call__(self, frames):
        single = frames.dim() == 4
        if single:
            frames = frames.unsqueeze(0)
        out = ops.clip_normalize(frames.contiguous(), self.mean, self.std)
        return out[0] if single else out

    def __repr__(self):
        return f"ClipToTensorNormalize(mean={self.mean}, std={self.std})"


# ------------------------------------------------------------------------------------------------------------------------
# The augmentation in front of that tail (datasets/preprocessing.py:15-113), also on the GPU: the DataLoader workers only
# decode (RawFrames, collate_raw_clips) and ONE avid_clip_augment call per batch produces the model's input, bit-identical to
# the reference's per-frame PIL chain.  The random parameters are drawn on the host from Python's ``random`` in the
# reference's call order, so a seeded run draws the crops, flips, factors and operation orders the reference's classes draw.
# ------------------------------------------------------------------------------------------------------------------------
BRIGHTNESS, SATURATION, HUE, CONTRAST = lib.AUG_BRIGHTNESS, lib.AUG_SATURATION, lib.AUG_HUE, lib.AUG_CONTRAST
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

ClipAugParams = collections.namedtuple("ClipAugParams", "box resize window flip ops")
ClipAugParams.__doc__ = """One clip's geometry and colour parameters: crop ``box`` (i, j, h, w) of the source frame, resampled
to ``resize`` (RH, RW); ``window`` (y1, x1) of that image (its size is the transform's crop); ``flip``; ``ops`` = the colour
operations in the order they are applied, [(BRIGHTNESS | SATURATION | HUE | CONTRAST, factor), ...]."""


def _resized_crop_params(H, W, scale, ratio=(3. / 4., 4. / 3.)):
    """video_transforms.RandomResizedCrop.get_params (utils/videotransforms/video_transforms.py:331-371)."""
    area = W * H
    for _ in range(10):
        target_area = random.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect_ratio = math.exp(random.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if w <= W and h <= H:
            i = random.randint(0, H - h)
            j = random.randint(0, W - w)
            return i, j, h, w
    in_ratio = W / H                                   # fallback to the central crop
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def _jitter_ops(brightness, contrast, saturation, hue):
    """ColorJitter.get_params + the shuffled transform list of ColorJitter.__call__ (video_transforms.py:413-463)."""
    b = random.uniform(max(0, 1 - brightness), 1 + brightness) if brightness > 0 else None
    c = random.uniform(max(0, 1 - contrast), 1 + contrast) if contrast > 0 else None
    s = random.uniform(max(0, 1 - saturation), 1 + saturation) if saturation > 0 else None
    h = random.uniform(-hue, hue) if hue > 0 else None
    ops_ = [(code, f) for code, f in ((BRIGHTNESS, b), (SATURATION, s), (HUE, h), (CONTRAST, c)) if f is not None]
    random.shuffle(ops_)
    return ops_


def _resize_sizes(H, W, size):
    """videotransforms.functional.resize_clip's target (functional.py:47-57, 69-76): a number scales the shorter side (and
    leaves a clip whose shorter side already matches alone), a pair is (height, width)."""
    if isinstance(size, numbers.Number):
        if (W <= H and W == size) or (H <= W and H == size):
            return H, W
        if W < H:
            return int(size * H / W), size
        return size, int(size * W / H)
    return int(size[0]), int(size[1])


def _check_crop(RH, RW, crop):
    if crop[1] > RW or crop[0] > RH:                   # RandomCrop / CenterCrop raise the same way
        raise ValueError(f"Initial image size should be larger then cropped size but got cropped sizes : ({crop[1]}, "
                         f"{crop[0]}) while initial image is ({RW}, {RH})")


def _center_window(RH, RW, crop):
    _check_crop(RH, RW, crop)
    x1 = int(round((RW - crop[1]) / 2.))
    y1 = int(round((RH - crop[0]) / 2.))
    return y1, x1


class _GpuVideoPrep:
    def _init(self, crop, color, num_frames, pad_missing, augment, normalize, totensor):
        if isinstance(crop, numbers.Number):
            crop = (crop, crop)
        if normalize:
            assert totensor
        if not totensor:
            raise ValueError("the GPU front end produces the tensor: totensor=False is the CPU classes' business")
        self.crop, self.color = (int(crop[0]), int(crop[1])), tuple(color)
        self.num_frames, self.pad_missing, self.augment, self.normalize = num_frames, pad_missing, augment, normalize

    def sample(self, sizes):
        """Draw one ClipAugParams per clip from Python's ``random``; ``sizes``: (H, W) of every clip's frames, in batch
        order (the order a single-process reference loader would have transformed them in)."""
        return [self._sample_one(int(H), int(W)) for H, W in sizes]

    def __call__(self, clips, params=None):
        """``clips``: list of uint8 ``[T_b, H_b, W_b, 3]`` GPU tensors (or one clip, or a dense ``[B, T, H, W, 3]`` tensor)
        -> fp32 ``[B, 3, frames, ch, cw]`` (``[3, frames, ch, cw]`` for one clip); ``params``: what ``sample`` returned
        (drawn here when omitted)."""
        single = isinstance(clips, torch.Tensor) and clips.dim() == 4
        if single:
            clips = [clips]
        elif isinstance(clips, torch.Tensor):
            clips = list(clips.unbind(0))
        if params is None:
            params = self.sample([(c.shape[1], c.shape[2]) for c in clips])
        # the reference's pad_missing loop repeats a short clip up to num_frames and leaves a long one alone
        lengths = {max(c.shape[0], self.num_frames) if self.pad_missing else c.shape[0] for c in clips}
        if len(lengths) != 1:
            raise ValueError(f"the clips of one batch come out with different frame counts: {sorted(lengths)}")
        mean, std = (MEAN, STD) if self.normalize else ((0., 0., 0.), (1., 1., 1.))
        out = ops.clip_augment([c.contiguous() for c in clips], params, lengths.pop(), self.crop, mean, std)
        return out[0] if single else out


class GpuVideoPrep_MSC_CJ(_GpuVideoPrep):
    """``VideoPrep_MSC_CJ`` (datasets/preprocessing.py:15-60) on the GPU: RandomResizedCrop + flip + ColorJitter, or
    Resize(int(crop[0] / 0.875)) + CenterCrop with ``augment=False``; then ClipToTensor + Normalize."""

    def __init__(self, crop=(224, 224), color=(0.4, 0.4, 0.4, 0.2), min_area=0.08, augment=True, normalize=True,
                 totensor=True, num_frames=8, pad_missing=False):
        self._init(crop, color, num_frames, pad_missing, augment, normalize, totensor)
        self.min_area = min_area

    def _sample_one(self, H, W):
        if self.augment:
            box = _resized_crop_params(H, W, (self.min_area, 1.))
            flip = random.random() < 0.5
            return ClipAugParams(box, self.crop, (0, 0), flip, _jitter_ops(*self.color))
        RH, RW = _resize_sizes(H, W, int(self.crop[0] / 0.875))
        return ClipAugParams((0, 0, H, W), (RH, RW), _center_window(RH, RW, self.crop), False, [])


class GpuVideoPrep_Crop_CJ(_GpuVideoPrep):
    """``VideoPrep_Crop_CJ`` (datasets/preprocessing.py:63-113) on the GPU: Resize(resize) + RandomCrop + flip +
    ColorJitter, or Resize + CenterCrop with ``augment=False``; then ClipToTensor + Normalize."""

    def __init__(self, resize=(256, 256), crop=(224, 224), color=(0.4, 0.4, 0.4, 0.2), num_frames=8, pad_missing=False,
                 augment=True, normalize=True, totensor=True):
        self._init(crop, color, num_frames, pad_missing, augment, normalize, totensor)
        self.resize = resize

    def _sample_one(self, H, W):
        RH, RW = _resize_sizes(H, W, self.resize)
        if not self.augment:
            return ClipAugParams((0, 0, H, W), (RH, RW), _center_window(RH, RW, self.crop), False, [])
        _check_crop(RH, RW, self.crop)
        x1 = random.randint(0, RW - self.crop[1])       # video_transforms.py:220-221: x before y
        y1 = random.randint(0, RH - self.crop[0])
        flip = random.random() < 0.5
        return ClipAugParams((0, 0, H, W), (RH, RW), (y1, x1), flip, _jitter_ops(*self.color))


class RawFrames:
    """``video_transform`` for the DataLoader workers: the decoder's list of RGB PIL images -> one uint8 ``[T, H, W, 3]``
    tensor (no resampling, no float conversion)."""

    def __call__(self, frames):
        arr = np.stack([np.asarray(f) for f in frames])
        if arr.ndim != 4 or arr.shape[-1] != 3 or arr.dtype != np.uint8:
            raise TypeError(f"RawFrames expects RGB 8-bit frames, got an array of shape {arr.shape} {arr.dtype}")
        return torch.from_numpy(np.ascontiguousarray(arr))


def collate_raw_clips(batch):
    """``collate_fn``: the default collation for every key but ``frames``, which stays a list of ``[T, H, W, 3]`` tensors
    (decoded sizes differ from video to video)."""
    from torch.utils.data import default_collate
    out = default_collate([{k: v for k, v in s.items() if k != "frames"} for s in batch])
    out["frames"] = [s["frames"] for s in batch]
    return out
