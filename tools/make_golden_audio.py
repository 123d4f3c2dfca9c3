#!/usr/bin/env python
"""Generate tests/golden/audio_prep.npz by IMPORTING the reference's AudioPrep and running it on seeded int16 clips (build
container only).

    python tools/make_golden_audio.py --ref <reference checkout> [--out tests/golden]

librosa is not installed where this runs and the reference's datasets/preprocessing.py imports it (for LogSpectrogram, which is
not run here), so an empty stand-in module is registered under that name first; torchvision likewise (the video classes).
Each clip is handed over the way the decoder hands it over (int16 / np.iinfo(int16).max, float64; ``None`` for the missing
clip).  The cases run in order on ONE seeded ``random``, so the gains are the sequence a single-process loader would draw.
Stored: the int16 inputs, the seed, the reference's constructor arguments and defaults (read from its signature), per case the
constructor keywords, the gain the reference drew (logged at ``random.uniform``) and its float32 output; no reference source is
copied."""
import argparse
import importlib.util
import inspect
import json
import os
import random
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, DURATION, SEED = 8000, 0.25, 20261019                  # L = int(0.25 * 8000) = 2000

# tag: (channels, samples or None = missing, augment)
CASES = {
    "missing": (1, None, False),
    "n1_c1_aug": (1, 1, True),
    "n1999_c2_aug": (2, 1999, True),
    "n1999_c3": (3, 1999, False),
    "n2000_c3": (3, 2000, False),
    "n2000_c1_aug": (1, 2000, True),
    "n2001_c2": (2, 2001, False),
    "n2001_c1_aug": (1, 2001, True),
    "n3500_c3_aug": (3, 3500, True),
    "n3500_c1": (1, 3500, False),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    for name in ("librosa", "torchvision", "torchvision.transforms", "torchvision.transforms.functional"):
        sys.modules.setdefault(name, types.ModuleType(name))
    import PIL.Image  # noqa: F401  (the reference's video transforms, imported alongside, expect the submodule loaded)
    sys.path.insert(0, args.ref)
    spec = importlib.util.spec_from_file_location("ref_preprocessing", os.path.join(args.ref, "datasets", "preprocessing.py"))
    prep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prep)                                        # the reference

    drawn = []
    uniform = random.uniform

    def logged_uniform(a, b):
        drawn.append(uniform(a, b))
        return drawn[-1]

    sig = inspect.signature(prep.AudioPrep.__init__)
    ctor = [[n, p.default] for n, p in sig.parameters.items() if n != "self"]
    rng = np.random.RandomState(SEED)
    out, meta = {}, {"sr": SR, "duration": DURATION, "seed": SEED, "constructor": ctor, "cases": {}}
    random.seed(SEED)
    random.uniform = logged_uniform
    try:
        for tag, (C, n, augment) in CASES.items():
            kw = dict(trim_pad=True, duration=DURATION, augment=augment, missing_as_zero=n is None)
            drawn.clear()
            if n is None:
                clip, given = np.zeros((1, 0), np.int16), None
            else:
                clip = rng.randint(-32768, 32768, (C, n)).astype(np.int16)
                clip[0, 0] = 32767                                      # the extremes, and a sum that cancels
                clip[-1, -1] = -32768
                if n > 2:
                    clip[:, 1] = -32768
                    clip[:, 2] = 32767
                given = clip / np.iinfo(clip.dtype).max                  # what the decoder returns: float64
            ref, sr = prep.AudioPrep(**kw)(given, SR)
            assert sr == SR and ref.dtype == np.float32 and ref.shape == (1, int(DURATION * SR)) and len(drawn) == int(augment)
            out[f"{tag}_pcm"] = clip
            out[f"{tag}_out"] = ref
            meta["cases"][tag] = {"kwargs": kw, "gain": drawn[0] if augment else None}
            print(tag, clip.shape, meta["cases"][tag])
    finally:
        random.uniform = uniform
    out["meta"] = np.array(json.dumps(meta))         # floats round-trip exactly through repr
    path = os.path.join(args.out, "audio_prep.npz")
    np.savez_compressed(path, **out)
    print("audio_prep.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
