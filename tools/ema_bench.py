"""Dev tool: what the weight average (``ema_decay``) costs, on the GPU, the configurations alternating in one process.

1. kernel:  over a flat buffer of the two-tower model's size (21.3 M fp32 elements), by the library's HIP-event timers, in turns
   within every round: ``adam_flat_kernel`` (28 B per element), ``adam_flat_ema_kernel`` (the fused form, 36 B), ``ema_flat_kernel``
   (the separate pass, 12 B: plain + separate is the two-launch form, 40 B and a second launch), ``swap_flat_kernel`` (16 B), and
   the SGD pair.  ``blocks`` windows of ``rounds`` rounds each: the median window and the spread (min .. max) per kernel.
2. step:    ``TrainStep.step`` at bench.py's default shapes (batch 64, 3x8x112x112 video, 240 000-row banks, 1024 negatives) and
   ``FinetuneStep.step`` (batch 32, 101 classes) with ``ema_decay`` off and on, taking turns; ms per step and, with the mean
   shader clock over each window (bench.py's sampler), shader cycles per step; the yardstick is the average off in the same run.

One JSON line per part.    python tools/ema_bench.py [--rounds 20] [--steps 30] [--warmup 8] [--blocks 5] [--parts kernel,step,finetune] [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
from avid_hip import lib, ops, parallel  # noqa: E402
from guard_bench import BANK, BS, alternate, fresh  # noqa: E402

KERNELS = ("adam_flat_kernel", "adam_flat_ema_kernel", "sgd_flat_kernel", "sgd_flat_ema_kernel", "ema_flat_kernel", "swap_flat_kernel")


def kernel_part(dev, n, rounds, blocks):
    g = torch.Generator().manual_seed(1)

    def buf(scale):
        return (scale * torch.randn(n, generator=g)).to(dev)
    p, gr, m, v, e, other = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_(), buf(1.0), buf(1.0)
    k = torch.zeros((), dtype=torch.int64, device=dev)

    def one(step):
        ops.adam_flat(p, gr, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, step)
        ops.adam_flat_ema(p, gr, m, v, e, 2e-4, 0.9, 0.999, 1e-8, 1e-5, step, 0.999, warmup=True, updates_dev=k)
        ops.sgd_flat(p, gr, m, 1e-3, 0.9, 1e-4, True)
        ops.sgd_flat_ema(p, gr, m, e, 1e-3, 0.9, 1e-4, 0.999, nesterov=True, warmup=True, updates_dev=k)
        ops.ema_flat(e, p, 0.999, True, k)
        ops.swap_flat(e, other)
    for s in range(3):                                             # warm up outside the timers
        one(1 + s)
    torch.cuda.synchronize()
    windows = {name: [] for name in KERNELS}
    nbytes = {}
    for b in range(blocks):
        lib.timing_enable(True)
        for r in range(rounds):
            one(4 + b * rounds + r)
        torch.cuda.synchronize()
        rep = lib.timing_report()
        lib.timing_enable(False)
        for name in KERNELS:
            windows[name].append(rep[name]["ms"] / rep[name]["launches"])
            nbytes[name] = rep[name]["bytes"] / rep[name]["launches"]
    rec = {"part": "kernel", "elements": n, "rounds": rounds, "blocks": blocks}
    med = {}
    for name in KERNELS:
        w = sorted(windows[name])
        med[name] = w[len(w) // 2]
        rec[name] = {"ms": round(med[name], 4), "min": round(w[0], 4), "max": round(w[-1], 4), "bytes": nbytes[name],
                     "GB_s": round(nbytes[name] / med[name] / 1e6, 1)}
    for opt in ("adam", "sgd"):
        plain, fused = med[f"{opt}_flat_kernel"], med[f"{opt}_flat_ema_kernel"]
        rec[f"{opt}_fused_over_plain"] = round(fused / plain, 4)
        rec[f"{opt}_fused_over_two_launches"] = round(fused / (plain + med["ema_flat_kernel"]), 4)
    return rec


def fresh_finetune(dev):
    import models
    torch.manual_seed(0)
    return models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5).to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parts", default="kernel,step,finetune")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ema_bench measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    g = torch.Generator().manual_seed(1234)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def over_off(res):
        return {n: round(r["ms_per_step"] / res["off"]["ms_per_step"], 4) for n, r in res.items()}

    if "kernel" in parts:
        m, _ = fresh(dev)
        n = parallel.FlatParams(m).numel
        del m
        emit(kernel_part(dev, n, a.rounds, a.blocks))
    if "step" in parts:
        video = torch.randn(BS, 3, 8, 112, 112, generator=g).to(dev)
        audio = torch.randn(BS, 1, 40, 100, generator=g).to(dev)
        ids = torch.stack([torch.randperm(BANK, generator=g)[:BS] for _ in range(64)]).to(dev)
        engines = {}
        for name, kw in (("off", {}), ("ema", dict(ema_decay=0.999, ema_warmup=True))):
            m, c = fresh(dev)
            engines[name] = parallel.TrainStep(m, c, **kw)
        res = alternate({n: (lambda i, e=e: e.step(video, audio, ids[i % 64])) for n, e in engines.items()}, a.steps, a.warmup,
                        a.blocks, dev)
        emit({"part": "step", "batch": BS, "TrainStep": res, "over_off": over_off(res), "ema_updates": int(engines["ema"].ema_updates)})
        del engines
    if "finetune" in parts:
        B = 32
        clips = torch.randn(B, 3, 8, 112, 112, generator=g).to(dev)
        labels = torch.randint(0, 101, (B,), generator=g).to(dev)
        engines = {name: parallel.FinetuneStep(fresh_finetune(dev), **kw)
                   for name, kw in (("off", {}), ("ema", dict(ema_decay=0.999, ema_warmup=True)))}
        res = alternate({n: (lambda i, e=e: e.step(clips, labels)) for n, e in engines.items()}, a.steps, a.warmup, a.blocks, dev)
        emit({"part": "finetune", "batch": B, "FinetuneStep": res, "over_off": over_off(res),
              "ema_updates": int(engines["ema"].ema_updates)})
        del engines
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
