#!/usr/bin/env python
"""Generate tests/golden/augment.npz by IMPORTING the reference's VideoPrep_MSC_CJ / VideoPrep_Crop_CJ and running them under
seeded ``random`` (build container only; needs Pillow).

    python tools/make_golden_augment.py --ref <reference checkout> [--out tests/golden]

torchvision is not installed where this runs and the reference's video_transforms imports it, so an in-process stand-in for
``torchvision.transforms.functional`` is installed first: the six functions the reference calls (resized_crop, the four
adjust_* and to_grayscale), written with PIL as torchvision's PIL backend writes them.  The composition, the RNG call order
and the pad_missing loop are the reference's own.  Stored per case: the input frames, the constructor arguments and seed, the
parameters the reference drew (logged at the stand-in and at the reference's crop helper) and its output; no reference source
is copied."""
import argparse
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np
from PIL import Image, ImageEnhance

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRIGHTNESS, SATURATION, HUE, CONTRAST = 0, 1, 2, 3
LOG = {}


def _standin():
    vF = types.ModuleType("torchvision.transforms.functional")

    def resized_crop(img, i, j, h, w, size, interpolation=Image.BILINEAR):
        LOG["box"] = (i, j, h, w)
        LOG["resize"] = tuple(size)
        img = img.crop((j, i, j + w, i + h))
        return img.resize(tuple(size[::-1]), interpolation)

    def _once(code, factor):
        if LOG["frame"] == 0:
            LOG["ops"].append((code, float(factor)))

    def adjust_brightness(img, f):
        _once(BRIGHTNESS, f)
        return ImageEnhance.Brightness(img).enhance(f)

    def adjust_contrast(img, f):
        _once(CONTRAST, f)
        return ImageEnhance.Contrast(img).enhance(f)

    def adjust_saturation(img, f):
        _once(SATURATION, f)
        return ImageEnhance.Color(img).enhance(f)

    def adjust_hue(img, f):
        _once(HUE, f)
        if not -0.5 <= f <= 0.5:
            raise ValueError(f"hue_factor ({f}) is not in [-0.5, 0.5].")
        if img.mode in {"L", "1", "I", "F"}:
            return img
        h, s, v = img.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(int(f * 255) % 256)               # uint8 arithmetic wraps, as the backend's does
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert(img.mode)

    def to_grayscale(img, num_output_channels=1):
        img = img.convert("L")
        return img if num_output_channels == 1 else Image.merge("RGB", (img, img, img))

    for f in (resized_crop, adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue, to_grayscale):
        setattr(vF, f.__name__, f)
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tv.transforms, tr.functional = tr, vF
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": vF})
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))      # preprocessing.py's audio classes: not run here


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    _standin()
    sys.path.insert(0, args.ref)
    spec = importlib.util.spec_from_file_location("ref_preprocessing", os.path.join(args.ref, "datasets", "preprocessing.py"))
    prep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prep)                                        # the reference
    from utils.videotransforms import functional as F, video_transforms

    crop_clip = F.crop_clip

    def logged_crop(clip, y1, x1, h, w):
        LOG["resize"] = clip[0].size[::-1]
        LOG["window"] = (y1, x1)
        return crop_clip(clip, y1, x1, h, w)
    F.crop_clip = logged_crop

    flip_cls = video_transforms.RandomHorizontalFlip
    flip_call = flip_cls.__call__

    def logged_flip(self, clip):
        out = flip_call(self, clip)
        LOG["flip"] = out is not clip
        return out
    flip_cls.__call__ = logged_flip

    jitter_cls = video_transforms.ColorJitter
    jitter_call = jitter_cls.__call__

    class _Frames(list):
        def __iter__(self):
            for n, img in enumerate(list.__iter__(self)):
                LOG["frame"] = n
                yield img

    def logged_jitter(self, clip):
        return jitter_call(self, _Frames(clip))
    jitter_cls.__call__ = logged_jitter

    cases = {
        # tag: (class, kwargs, (T, H, W), seed)
        "msc_aug": ("MSC", dict(crop=(12, 16), num_frames=2), (2, 30, 40), 11),
        "msc_eval": ("MSC", dict(crop=(12, 16), augment=False, num_frames=2), (2, 30, 40), 13),
        "msc_fallback": ("MSC", dict(crop=(10, 12), min_area=0.9, num_frames=2), (2, 8, 48), 14),
        "msc_pad": ("MSC", dict(crop=(12, 12), num_frames=5, pad_missing=True), (2, 24, 34), 15),
        "msc_nocontrast": ("MSC", dict(crop=(12, 16), color=(0.4, 0.0, 0.4, 0.2), num_frames=2), (2, 23, 33), 16),
        "msc_contrast_only": ("MSC", dict(crop=(12, 16), color=(0.0, 0.4, 0.0, 0.0), num_frames=2), (2, 23, 33), 17),
        "crop_aug": ("Crop", dict(resize=(18, 24), crop=(12, 16), num_frames=2), (2, 23, 33), 18),
        "crop_aug_up": ("Crop", dict(resize=(40, 44), crop=(14, 14), num_frames=2, pad_missing=True), (1, 18, 25), 19),
        "crop_eval": ("Crop", dict(resize=(18, 24), crop=(12, 16), augment=False, num_frames=2), (2, 36, 48), 20),
    }
    rng = np.random.RandomState(20261017)
    out, meta = {}, {}
    for tag, (cls, kw, (T, H, W), seed) in cases.items():
        # smooth structure + sparse noise, so that resampling, saturation and hue all have something to act on
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([(yy * 5 + xx * 2) % 256, (xx * 7 + 40) % 256, (yy * 3 + xx * 3 + 90) % 256], -1)
        noise = rng.randint(-40, 41, (T, H, W, 3)) * (rng.rand(T, H, W, 1) < 0.12)
        frames = np.clip(base[None] + noise, 0, 255).astype(np.uint8)
        frames[0, 0, :2] = [[0, 0, 0], [255, 255, 255]]
        LOG.clear()
        LOG.update(box=(0, 0, H, W), window=(0, 0), flip=False, ops=[], frame=0)
        random.seed(seed)
        t = (prep.VideoPrep_MSC_CJ if cls == "MSC" else prep.VideoPrep_Crop_CJ)(**kw)
        ref = t([Image.fromarray(f) for f in frames]).numpy()
        out[f"{tag}_frames"] = frames
        out[f"{tag}_out"] = ref.astype(np.float32)
        meta[tag] = {"cls": cls, "kwargs": kw, "seed": seed, "box": list(LOG["box"]), "resize": list(LOG["resize"]),
                     "window": list(LOG["window"]), "flip": bool(LOG["flip"]), "ops": [[c, f] for c, f in LOG["ops"]]}
        print(tag, ref.shape, meta[tag])
    out["meta"] = np.array(json.dumps(meta))         # floats round-trip exactly through repr
    path = os.path.join(args.out, "augment.npz")
    np.savez_compressed(path, **out)
    print("augment.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
