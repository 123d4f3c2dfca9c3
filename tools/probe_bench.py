#!/usr/bin/env python
"""Linear-probe training throughput on one GPU at the shipped config (configs/benchmark/kinetics/8x224x224-linear.yaml:
clips 3x8x224x224, 400 classes, four AdaptiveMaxPool3d heads with BatchNorm1d).  One JSON line:

    python tools/probe_bench.py [--steps 6] [--warmup 2] [--rounds 3] [--virtual-ranks R]

The batch is the largest of 128 (the shipped one), 64, 32 that both paths run without exhausting memory (``batch``).
  ``probe_step``      clips/s of ``parallel.ProbeStep`` (the launch programs + flat Adam)
  ``head_kernels_ms`` HIP-event time of every head kernel in one step (launch log on, everything on one stream)
  ``peak_memory_mb``  torch's peak allocated memory of each path
  ``baseline``        clips/s of what the package gave a user before: this package's R2Plus1D called with ``return_embs=True``
                      under ``no_grad`` (the per-layer path), then ``nn.AdaptiveMaxPool3d``, ``nn.BatchNorm1d`` and ``nn.Linear``
                      heads, the summed ``CrossEntropyLoss`` and ``torch.optim.Adam``
The two paths alternate (``rounds`` times ``steps`` steps each, same process, same box); the rates are the medians over the
rounds.  ``linear_128x9216x400_ms``: forward + backward of one head's Linear on ``avid_probe_linear_*``, on the fine-tuning
classifier's ``avid_cls_linear_*`` and on torch's ``F.linear``.

``--virtual-ranks R`` (default 1, the output is then what it was): ``probe_step`` is ``ProbeStep(virtual_ranks=R)`` on the same
global batch — R = 8 at batch 128 is the shipped eight-replica job, 16 rows per BatchNorm1d; the baseline stays the whole-batch
step.  The output then also says ``virtual_ranks``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ARGS = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
            pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                         "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)
HEAD_KERNELS = ("adaptive_maxpool", "bn1d_", "probe_gemm_kernel", "probe_reduce_kernel", "probe_colsum_kernel",
                "cls_loss_kernel", "adam_flat_kernel")


class _TorchProbe(nn.Module):
    """The baseline: the reference's MOSTModel restated from torch modules over this package's tower."""

    def __init__(self, fe):
        super().__init__()
        fe.train(False)
        self.feature_extractor = fe
        self.pools = [eval("nn." + p, {"nn": nn}) for p in ARGS["pooling_ops"]]
        self.bns = nn.ModuleList([nn.BatchNorm1d(d) for d in ARGS["feat_dims"]])
        self.fcs = nn.ModuleList([nn.Linear(d, ARGS["n_classes"]) for d in ARGS["feat_dims"]])
        for p in fe.parameters():
            p.requires_grad = False

    def forward(self, x):
        with torch.no_grad():
            embs = self.feature_extractor(x, return_embs=True)
        out = []
        for ft, pool, bn, fc in zip(ARGS["feat_names"], self.pools, self.bns, self.fcs):
            with torch.no_grad():
                f = pool(embs[ft]).view(x.shape[0], -1).contiguous()
            out.append(fc(bn(f)))
        return out


def _steps(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def _event_ms(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _linear_compare(dev):
    from avid_hip import ops
    B, Fin, C = 128, 9216, 400
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, Fin), generator=g).to(dev).requires_grad_(True)
    w = (torch.randn((C, Fin), generator=g) / 96).to(dev).requires_grad_(True)
    b = torch.zeros(C, device=dev, requires_grad=True)
    gy = torch.randn((B, C), generator=g).to(dev)

    def both(f):
        def run():
            x.grad = w.grad = b.grad = None
            f(x, w, b).backward(gy)
        return run
    return {"probe_linear": round(_event_ms(both(ops.probe_linear)), 4), "cls_linear": round(_event_ms(both(ops.cls_linear)), 4),
            "torch_F_linear": round(_event_ms(both(F.linear)), 4)}


def _run(B, args, dev):
    import models
    from avid_hip import lib, parallel
    g = torch.Generator().manual_seed(0)
    video = torch.randn((B, 3, 8, 224, 224), generator=g).to(dev)
    labels = torch.randint(0, ARGS["n_classes"], (B,), generator=g).to(dev)
    torch.manual_seed(0)
    model = models.MOSTModel(models.R2Plus1D(18), **ARGS).to(dev).train()
    eng = parallel.ProbeStep(model, lr=1e-4, **({"virtual_ranks": args.virtual_ranks} if args.virtual_ranks != 1 else {}))
    torch.manual_seed(0)
    base = _TorchProbe(models.R2Plus1D(18)).to(dev).train()
    opt = torch.optim.Adam(base.parameters(), lr=1e-4, weight_decay=0)

    def new_step():
        eng.step(video, labels)

    def base_step():
        loss = sum(F.cross_entropy(o, labels) for o in base(video))
        opt.zero_grad()
        loss.backward()
        opt.step()
    peak = {}
    for tag, fn in (("probe_step", new_step), ("baseline", base_step)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        start = torch.cuda.memory_allocated(dev)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        peak[tag] = {"peak_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1), "resident_before_mb": round(start / 2 ** 20, 1)}
    ms = {"probe_step": [], "baseline": []}
    for _ in range(args.rounds):
        ms["probe_step"].append(_steps(new_step, args.steps))
        ms["baseline"].append(_steps(base_step, args.steps))
    lib.timing_enable(True)
    new_step()
    torch.cuda.synchronize()
    rep = lib.timing_report()
    lib.timing_enable(False)
    heads = {k: {"launches": v["launches"], "ms": round(v["ms"], 4)} for k, v in sorted(rep.items()) if k.startswith(HEAD_KERNELS)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"batch": B,
            "probe_step": {"clips_per_s": round(B / med["probe_step"] * 1e3, 2), "ms_per_step": round(med["probe_step"], 3),
                           "rounds_ms": [round(v, 3) for v in ms["probe_step"]]},
            "head_kernels_ms": heads, "head_kernels_total_ms": round(sum(v["ms"] for v in heads.values()), 4),
            "tower_and_rest_ms": round(sum(v["ms"] for k, v in rep.items() if not k.startswith(HEAD_KERNELS)), 3),
            "peak_memory_mb": peak,
            "baseline": {"clips_per_s": round(B / med["baseline"] * 1e3, 2), "ms_per_step": round(med["baseline"], 3),
                         "rounds_ms": [round(v, 3) for v in ms["baseline"]]},
            "probe_step_over_baseline": round(med["baseline"] / med["probe_step"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="128,64,32")
    ap.add_argument("--virtual-ranks", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "linear-probe training clips/s (MOSTModel on R(2+1)D-18, 3x8x224x224, 400 classes, 1 GPU)", "unit": "clips/s"}
    res, skipped = None, {}
    for B in (int(v) for v in args.batches.split(",")):
        try:
            res = _run(B, args, dev)
            break
        except torch.cuda.OutOfMemoryError as e:
            skipped[str(B)] = str(e).splitlines()[0][:120]
            torch.cuda.empty_cache()
    if res is None:
        raise SystemExit(f"no batch fits: {skipped}")
    out.update(res)
    out["batches_skipped"] = skipped
    if args.virtual_ranks != 1:
        out["virtual_ranks"] = args.virtual_ranks
    out["linear_128x9216x400_ms"] = _linear_compare(dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
