#!/usr/bin/env python
"""Throughput of the GPU clip augmentation (avid_clip_augment) on one GPU.  One JSON line:

    python tools/augment_bench.py [--batch 64] [--iters 20] [--rounds 5] [--pil-batches 2] [--workers 16]

A batch of 8-frame uint8 clips at a spread of decoded sizes (240 x 320 ... 360 x 640) goes through
``GpuVideoPrep_MSC_CJ`` (RandomResizedCrop + flip + the four colour operations in a random order per clip, parameters drawn
once from a seed) to 224 x 224 and to 112 x 112.  The two paths and ``clip_normalize_kernel`` on the same output shapes
alternate (``rounds`` rounds of ``iters`` calls each, HIP events around each group of calls, same process, same box); the
figures are medians over the rounds, with the min-max spread.
  ``ms_per_batch`` / ``clips_per_s``   one call = the whole batch
  ``gbytes_per_s``                     over the ALGORITHMIC bytes: the crop boxes read once (3 B per source pixel of every output
                                       frame) + the fp32 output written once (12 B per pixel); the uint8 intermediate of the
                                       contrast path and re-read taps are not counted
  ``augment_*_geometry_only`` / ``_no_hue``  the same crops and flips with no colour operation / without the hue shift
  ``kernels_224_ms``                   HIP-event time of each kernel of the 224 path, per launch (the library's timers)
  ``normalize``                        ``avid_clip_normalize`` producing the same output from a dense uint8 batch (3 + 12 B)
  ``pil_16_workers``                   the same batch and parameters through Pillow (crop + resize, transpose, ImageEnhance,
                                       HSV hue shift, float conversion + normalisation) on a pool of worker processes; null
                                       where Pillow is not importable.  No decoding on either side."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(240, 320), (240, 426), (256, 340), (288, 512), (360, 480), (360, 640)]
MEAN = np.array([0.485, 0.456, 0.406], np.float32).reshape(3, 1, 1, 1)
STD = np.array([0.229, 0.224, 0.225], np.float32).reshape(3, 1, 1, 1)


def make_clips(batch, T=8, seed=0):
    rng = np.random.RandomState(seed)
    clips = []
    for b in range(batch):
        H, W = SIZES[b % len(SIZES)]
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([(yy + xx * 2) % 256, (xx * 3 + 40) % 256, (yy * 2 + xx + 90) % 256], -1)
        clips.append(np.clip(base[None] + rng.randint(-50, 51, (T, H, W, 3)), 0, 255).astype(np.uint8))
    return clips


def _pil_clip(job):
    """One clip through Pillow, as the reference's transforms + torchvision's PIL backend do it per frame."""
    from PIL import Image, ImageEnhance
    frames, (box, resize, window, flip, ops_), crop = job
    i, j, h, w = box
    out = []
    for f in frames:
        img = Image.fromarray(f).crop((j, i, j + w, i + h)).resize((resize[1], resize[0]), Image.BILINEAR)
        img = img.crop((window[1], window[0], window[1] + crop[1], window[0] + crop[0]))
        if flip:
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        for code, fac in ops_:
            if code == 0:
                img = ImageEnhance.Brightness(img).enhance(fac)
            elif code == 1:
                img = ImageEnhance.Color(img).enhance(fac)
            elif code == 3:
                img = ImageEnhance.Contrast(img).enhance(fac)
            else:
                hh, s, v = img.convert("HSV").split()
                np_h = np.array(hh, dtype=np.uint8)
                np_h += np.uint8(int(fac * 255) % 256)
                img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        out.append(np.asarray(img))
    t = np.stack(out).transpose(3, 0, 1, 2).astype(np.float32) / np.float32(255)
    return (t - MEAN) / STD


def pil_rate(clips, params, crop, workers, batches):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return None
    import multiprocessing as mp
    jobs = [(c, tuple(p), crop) for c, p in zip(clips, params)]
    with mp.get_context("fork").Pool(workers) as pool:
        pool.map(_pil_clip, jobs[:workers], chunksize=1)            # start-up
        t0 = time.perf_counter()
        for _ in range(batches):
            pool.map(_pil_clip, jobs, chunksize=1)
        dt = (time.perf_counter() - t0) / batches
    return {"workers": workers, "s_per_batch": round(dt, 4), "clips_per_s": round(len(clips) / dt, 1),
            "frames_per_s": round(len(clips) * clips[0].shape[0] / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pil-batches", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()

    import torch                                                     # (the library import initialises nothing on the GPU)
    from datasets.gpu_video import GpuVideoPrep_MSC_CJ
    clips = make_clips(args.batch)
    paths = {}
    for side in (224, 112):
        t = GpuVideoPrep_MSC_CJ(crop=(side, side), num_frames=8)
        random.seed(side)
        paths[side] = (t, t.sample([c.shape[1:3] for c in clips]))
    # the worker pool forks: it runs before this process opens the GPU
    pil = {side: pil_rate(clips, params, (side, side), args.workers, args.pil_batches) if args.pil_batches > 0 else None
           for side, (t, params) in paths.items()}

    assert torch.cuda.is_available(), "augment_bench needs a GPU"
    from avid_hip import ops
    dev = torch.device("cuda:0")
    gclips = [torch.from_numpy(c).to(dev) for c in clips]
    dense = {side: torch.randint(0, 256, (args.batch, 8, side, side, 3), dtype=torch.uint8, device=dev) for side in paths}
    work = {}
    for side, (t, params) in paths.items():
        work[f"augment_{side}"] = (lambda t=t, params=params: t(gclips, params),
                                   sum(3.0 * 8 * p.box[2] * p.box[3] for p in params) + 12.0 * args.batch * 8 * side * side)
        # where the time goes: the same geometry without colour operations, and with the three blends but no hue
        for tag, keep in (("geometry_only", ()), ("no_hue", (0, 1, 3))):
            sub = [p._replace(ops=[o for o in p.ops if o[0] in keep]) for p in params]
            work[f"augment_{side}_{tag}"] = (lambda t=t, sub=sub: t(gclips, sub), work[f"augment_{side}"][1])
        work[f"normalize_{side}"] = (lambda side=side: ops.clip_normalize(dense[side]), 15.0 * args.batch * 8 * side * side)
    for fn, _ in work.values():                                       # warm-up: code objects, workspace, staging buffers
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, _) in work.items():                               # the paths alternate inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.iters)
    out = {"batch": args.batch, "frames": 8, "sizes": SIZES, "iters": args.iters, "rounds": args.rounds}
    for k, (fn, nbytes) in work.items():
        med = statistics.median(ms[k])
        out[k] = {"ms_per_batch": round(med, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                  "clips_per_s": round(args.batch / med * 1e3, 1), "gbytes_per_s": round(nbytes / med / 1e6, 1),
                  "algorithmic_mbytes": round(nbytes / 1e6, 2)}
    # the kernels alone (the library's HIP-event timers around each launch): a call's GPU time without the host's share
    from avid_hip import lib
    t, params = paths[224]
    lib.timing_enable(True)
    for _ in range(5):
        t(gclips, params)
    torch.cuda.synchronize()
    out["kernels_224_ms"] = {k: round(v["ms"] / v["launches"], 4) for k, v in lib.timing_report().items()}
    lib.timing_enable(False)
    # host time of one call (descriptor marshalling + the coefficient tables): what the training loop's thread pays
    t, params = paths[224]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        t(gclips, params)
    out["host_ms_per_call_224"] = round((time.perf_counter() - t0) * 1e3 / args.iters, 3)
    torch.cuda.synchronize()
    out["pil_16_workers"] = {str(k): v for k, v in pil.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
