#!/usr/bin/env python
"""The audio front end from int16 against the float32 path it replaces, on one GPU.  One JSON line:

    python tools/audio_bench.py [--batch 64] [--iters 50] [--rounds 7]

A batch of 2 s mono clips at 24 kHz (48000 int16 samples each, seeded noise), ``n_fft=512``, hop 0.01 -> ``[B, 1, 200, 257]``.
  ``front_end_int16``       (a) ``GpuAudioFrontEnd`` on int16 clips already on the device (descriptor marshalling, one
                            ``avid_logspec_pcm`` call)
  ``logspec_float32``       (b) ``LogSpectrogram`` on a float32 ``[B, 1, L]`` already on the device
  ``host_prep_upload_logspec``  (c) what the float32 loader pays per batch: the numpy restatement of ``AudioPrep`` per clip on
                            the host (ONE thread here; the reference spreads it over its workers), the float32 upload from
                            pinned memory, then (b).  Host clock around work that ends in a synchronise.
  ``upload_int16`` / ``upload_float32``   the pinned host-to-device copy alone, 96 KB against 192 KB per clip
  ``kernels_ms``            HIP-event time per launch of each kernel of (a) and (b) (the library's timers, a pass of their own)
(a), (b) and the uploads alternate inside every round (``rounds`` rounds of ``iters`` calls, HIP events around each group, same
process, same box); figures are medians over the rounds with the min-max spread.  ``sclk_ghz``: mean shader clock over the
timed rounds where the box exposes it.  A report, not a gate."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SR, DURATION, N_FFT, HOP = 24000, 2.0, 512, 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "audio_bench needs a GPU"
    import _audio_ref as R
    from avid_hip import lib
    from bench import ClockSampler
    from datasets.gpu_audio import GpuAudioFrontEnd, GpuAudioPrep, LogSpectrogram
    dev = torch.device("cuda:0")
    B, L = args.batch, int(DURATION * SR)
    rng = np.random.RandomState(0)
    pcm = [np.clip(rng.standard_normal((1, L)) * 3000.0, -32768, 32767).astype(np.int16) for _ in range(B)]
    spec = LogSpectrogram(SR, n_fft=N_FFT, hop_size=HOP, device=dev)
    front = GpuAudioFrontEnd(GpuAudioPrep(duration=DURATION, device=dev), spec)
    pin16 = torch.from_numpy(np.concatenate(pcm)).pin_memory()                                    # [B, L] int16
    pin32 = torch.from_numpy(R.prepared_batch(pcm, L)).unsqueeze(1).pin_memory()                  # [B, 1, L] float32
    dev16 = torch.empty(pin16.shape, dtype=pin16.dtype, device=dev)
    dev32 = torch.empty(pin32.shape, dtype=pin32.dtype, device=dev)
    dev16.copy_(pin16)
    dev32.copy_(pin32)
    clips = [c.unsqueeze(0) for c in dev16.unbind(0)]                                             # B views [1, L]

    got, want = front(clips, SR, DURATION)[0], spec(dev32, SR, DURATION)[0]
    same = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))                       # what is timed agrees

    def host_path():
        wave = torch.from_numpy(np.stack([R.prepared(c, L) for c in pcm])).unsqueeze(1)
        out, _ = spec(wave.to(dev), SR, DURATION)
        return out

    work = {"front_end_int16": lambda: front(clips, SR, DURATION),
            "logspec_float32": lambda: spec(dev32, SR, DURATION),
            "upload_int16": lambda: dev16.copy_(pin16, non_blocking=True),
            "upload_float32": lambda: dev32.copy_(pin32, non_blocking=True)}
    for fn in work.values():                                            # warm-up: code objects, basis, workspace, staging
        for _ in range(5):
            fn()
    host_path()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    clock = ClockSampler(0)
    clock.start()
    for _ in range(args.rounds):
        for k, fn in work.items():                                      # the paths alternate inside every round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.iters)
    sclk = clock.stop()
    host = []
    for _ in range(max(3, args.rounds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_path()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    ms["host_prep_upload_logspec"] = host

    out = {"batch": B, "samples": L, "sr": SR, "n_fft": N_FFT, "hop": HOP, "frames": int(got.shape[2]), "iters": args.iters,
           "rounds": args.rounds, "bit_identical": same, "sclk_ghz": sclk,
           "bytes_per_clip": {"int16": 2 * L, "float32": 4 * L}}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"ms_per_batch": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "clips_per_s": round(B / med * 1e3, 1)}
    lib.timing_enable(True)
    for _ in range(5):
        front(clips, SR, DURATION)
        spec(dev32, SR, DURATION)
    torch.cuda.synchronize()
    out["kernels_ms"] = {k: round(v["ms"] / v["launches"], 4) for k, v in lib.timing_report().items()}
    lib.timing_enable(False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
