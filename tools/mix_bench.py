#!/usr/bin/env python
"""What mixup, CutMix and the soft-target loss cost on the GPU.

    python tools/mix_bench.py [--batch 64] [--steps 20] [--warmup 5] [--rounds 5] [--parts mix,loss,step] [--json PATH]

Three measurements of the SAME tree in ONE process (other work shares the host, so a difference is read within a round):

* ``mix``: ``ops.batch_mix`` on a batch of clips 3 x 8 x 224 x 224 and of log-spectrograms 1 x 200 x 257, mixup and CutMix (one
  box per sample, about a quarter of the plane), against the same mix written in torch ops on the GPU (``lam * x + (1 - lam) *
  x[perm]``; ``x.clone()`` plus one slice assignment per sample), alternating round by round.  Each timing is a host clock around
  ``steps`` calls that end in a device synchronise; reported: ms per call and GB/s of ALGORITHMIC bytes (mixup: two reads and one
  write per element; CutMix: one read and one write), next to the 6.3 TB/s a float4 copy reaches on this chip.  The two agree
  bit for bit or the script fails.
* ``loss``: ``ops.soft_ce_loss`` at V x clips x C = 9 900 x 10 x 101 (10^7 logits), with and without ``dlogits``: kernel time
  from device events against the bytes it moves.
* ``step``: ``parallel.FinetuneStep.step`` with ``loss="soft_ce"``, ``label_smoothing=0.1`` and a ``GpuBatchMix`` in front of it
  (mixup and CutMix, per sample) against the plain ``loss="ce"`` step of the same model and batch, for the video tower (clips 3 x 8
  x 112 x 112) and the audio tower (log-spectrograms 1 x 200 x 257), alternating round by round.

Needs a GPU: without one this fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))

HBM_ACHIEVABLE_GBS = 6300.0
N_CLASSES = 101


def _timed(fn, steps, warmup, torch):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, out


def _summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def _torch_mixup(x, perm, lam):
    l = lam.view(-1, *([1] * (x.dim() - 1)))
    return l * x + (1 - l) * x[perm]


def _torch_cutmix(x, perm, boxes):
    y = x.clone()
    for b, (h0, h1, w0, w1) in enumerate(boxes):
        y[b, ..., h0:h1, w0:w1] = x[perm[b], ..., h0:h1, w0:w1]
    return y


def bench_mix(args, torch, dev):
    import numpy as np
    from avid_hip import ops
    rng = np.random.default_rng(0)
    res = {}
    for name, shape in (("video", (args.batch, 3, 8, 224, 224)), ("audio", (args.batch, 1, 200, 257))):
        B, H, W = shape[0], shape[-2], shape[-1]
        x = torch.randn(shape, device=dev)
        perm = torch.from_numpy(rng.permutation(B)).to(dev)
        lam = torch.from_numpy(rng.beta(0.8, 0.8, size=B).astype(np.float32)).to(dev)
        h0, w0 = rng.integers(0, H // 2, size=B), rng.integers(0, W // 2, size=B)
        boxes = np.stack([h0, h0 + H // 2, w0, w0 + W // 2], 1).astype(np.int32)
        box = torch.from_numpy(boxes).to(dev)
        perm_h = perm.tolist()
        loops = {"mixup": lambda i: ops.batch_mix(x, perm, lam)[0], "mixup_torch": lambda i: _torch_mixup(x, perm, lam),
                 "cutmix": lambda i: ops.batch_mix(x, perm, lam, box=box)[0],
                 "cutmix_torch": lambda i: _torch_cutmix(x, perm_h, boxes.tolist())}
        times, last = {k: [] for k in loops}, {}
        for _ in range(args.rounds):
            for k, fn in loops.items():
                ms, out = _timed(fn, args.steps, args.warmup, torch)
                times[k].append(ms)
                last[k] = out
        assert torch.equal(last["mixup"].view(torch.int32), last["mixup_torch"].view(torch.int32)), name
        assert torch.equal(last["cutmix"].view(torch.int32), last["cutmix_torch"].view(torch.int32)), name
        nbytes = {"mixup": 12 * x.numel(), "cutmix": 8 * x.numel()}
        out = {"shape": list(shape), "ms": {k: _summary(v) for k, v in times.items()}}
        for k in ("mixup", "cutmix"):
            gbs = nbytes[k] / (statistics.median(times[k]) * 1e-3) / 1e9
            out[k + "_GBs"] = round(gbs, 1)
            out[k + "_of_achievable_hbm"] = round(gbs / HBM_ACHIEVABLE_GBS, 3)
            out[k + "_torch_over_ours"] = round(statistics.median(times[k + "_torch"]) / statistics.median(times[k]), 2)
        res[name] = out
        del x, last
        torch.cuda.empty_cache()
    from avid_hip import lib
    lib.timing_enable(True)
    x = torch.randn((args.batch, 3, 8, 224, 224), device=dev)
    perm, lam = torch.randperm(args.batch, device=dev), torch.rand(args.batch, device=dev)
    for _ in range(5):
        ops.batch_mix(x, perm, lam)
    torch.cuda.synchronize()
    res["kernels"] = {k: v for k, v in lib.timing_report().items() if k.startswith("batch_mix")}
    lib.timing_enable(False)
    ops.check_device_errors(dev)
    return res


def bench_loss(args, torch, dev):
    from avid_hip import lib, ops
    V, clips, C = 9900, 10, N_CLASSES
    g = torch.Generator().manual_seed(2)
    x = (3.0 * torch.randn((V * clips, C), generator=g)).to(dev)
    t = torch.softmax(4.0 * torch.randn((V, C), generator=g), 1).to(dev)
    n = V * clips * C
    res = {"V": V, "clips": clips, "C": C, "logits": n}
    for name, gs in (("eval", None), ("train", 1.0)):
        ts = [_timed(lambda i: ops.soft_ce_loss(x, t, clips, 0.1, grad_scale=gs), 20, 5, torch)[0] for _ in range(args.rounds)]
        nbytes = 4 * n * (2 if gs is not None else 1) + 4 * V * C * 2
        res[name] = {"ms_per_call": _summary(ts), "bytes": nbytes,
                     "GBs": round(nbytes / (statistics.median(ts) * 1e-3) / 1e9, 1)}
    lib.timing_enable(True)
    for gs in (None, 1.0):
        for _ in range(5):
            ops.soft_ce_loss(x, t, clips, 0.1, grad_scale=gs)
    torch.cuda.synchronize()
    res["kernels"] = {k: v for k, v in lib.timing_report().items() if k.startswith(("soft_ce", "mlabel_final"))}
    lib.timing_enable(False)
    ops.check_device_errors(dev)
    return res


def bench_step(args, torch, dev):
    import models
    from avid_hip import parallel
    from datasets.gpu_mix import GpuBatchMix
    g = torch.Generator().manual_seed(1)
    shapes = {"video": (args.batch, 3, 8, 112, 112), "audio": (args.batch, 1, 200, 257)}
    res = {}
    for tower, shape in shapes.items():
        make = (lambda: models.R2Plus1D(18)) if tower == "video" else models.Conv2D
        xs = [torch.randn(shape, generator=g).to(dev) for _ in range(2)]
        ys = [torch.randint(0, N_CLASSES, (args.batch,), generator=g).to(dev) for _ in range(2)]
        engines = {}
        for kind in ("ce", "soft_ce"):
            torch.manual_seed(0)
            m = models.ClassificationWrapper(make(), N_CLASSES, "pool", 512, use_dropout=True).to(dev).train()
            engines[kind] = parallel.FinetuneStep(m, loss=kind, label_smoothing=0.1 if kind == "soft_ce" else 0.0)
        mix = GpuBatchMix(N_CLASSES, mixup_alpha=0.8, cutmix_alpha=1.0, per_sample=True, seed=0)

        def mixed(i):
            xm, t = mix(xs[i % 2], ys[i % 2])
            return engines["soft_ce"].step(xm, t)[0]
        loops = {"ce": lambda i: engines["ce"].step(xs[i % 2], ys[i % 2])[0], "mix_soft_ce": mixed}
        times, last = {k: [] for k in loops}, {}
        for _ in range(args.rounds):
            for name, fn in loops.items():
                ms, loss = _timed(fn, args.steps, args.warmup, torch)
                times[name].append(ms)
                last[name] = float(loss)
        res[tower] = {"shape": list(shape), "ms_per_step": {k: _summary(v) for k, v in times.items()}, "last_loss": last,
                      "mix_soft_ce_minus_ce_ms": round(statistics.median(times["mix_soft_ce"]) - statistics.median(times["ce"]), 4)}
        del engines
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="mix,loss,step")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU")
    dev = torch.device("cuda", 0)
    parts = {"mix": bench_mix, "loss": bench_loss, "step": bench_step}
    unknown = [p for p in args.parts.split(",") if p not in parts]
    if unknown:
        raise SystemExit(f"mix_bench: unknown part(s) {unknown}; known: {list(parts)}")
    result = {"batch": args.batch, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    for p in args.parts.split(","):
        result[p] = parts[p](args, torch, dev)
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
