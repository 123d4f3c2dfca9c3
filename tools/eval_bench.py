#!/usr/bin/env python
"""Dense-evaluation throughput on one GPU: ``parallel.FinetuneStep.evaluate`` (eval-action-recg.py's ``test_dense`` phase) through the
inference programs (``plan.EvalPlan``) against the per-layer path, alternating in one process.  One JSON line:

    python tools/eval_bench.py [--calls 4] [--warmup 2] [--rounds 5] [--cases ...] [--repo DIR]

  ``8x10_8f``   8 videos x 10 clips of 3x8x224x224 in chunks of 8 clips (configs/benchmark/ucf/8at16-fold1.yaml's dense test)
  ``1x10_32f``  1 video x 10 clips of 3x32x224x224 in chunks of 10 (the 32-frame configs)
  ``probe_16x10`` ``parallel.ProbeStep.evaluate``: 16 videos x 10 clips of 3x8x224x224 in chunks of 128, the shipped probe batch
                (configs/benchmark/kinetics/8x224x224-linear.yaml; chunks of 128 and 32 clips)
For each: clips/s and ms per ``evaluate`` call of either path (median over ``rounds`` rounds of ``calls`` calls; ``rounds_ms`` and
``spread`` = (max - min) / median show the run-to-run variation), ``programs_over_per_layer`` (> 1: the programs are faster), torch's
peak allocated memory of either path, and the records per chunk program.  ``AVID_EVAL_PLAN=0`` is what the per-layer rows run
under (``plan.EVAL_ENABLED``, flipped in-process here).  The results of the two paths are compared bit for bit before anything is
timed.  ``--repo DIR`` imports the package from another checkout (its own built library): a checkout from before the inference
programs has no switch to flip and gets one row, ``evaluate`` — run this file once per checkout, alternating, to compare commits
on one box."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--repo" in sys.argv:
    REPO = os.path.abspath(sys.argv[sys.argv.index("--repo") + 1])
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = {"8x10_8f": ((8, 10, 3, 8, 224, 224), 8), "1x10_32f": ((1, 10, 3, 32, 224, 224), 10),
         "probe_16x10": ((16, 10, 3, 8, 224, 224), 128)}
PROBE = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
             pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                          "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)


def _calls(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def _run(name, args, dev):
    import models
    from avid_hip import parallel, plan
    shape, chunk = CASES[name]
    g = torch.Generator().manual_seed(0)
    video = torch.randn(shape, generator=g).to(dev)
    torch.manual_seed(0)
    if name.startswith("probe"):
        labels = torch.randint(0, 400, (shape[0],), generator=g).to(dev)
        model = models.MOSTModel(models.R2Plus1D(18), **PROBE).to(dev).train()
        eng = parallel.ProbeStep(model)
    else:
        labels = torch.randint(0, 101, (shape[0],), generator=g).to(dev)
        model = models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5).to(dev).train()
        eng = parallel.FinetuneStep(model)
    has_switch = hasattr(plan, "EVAL_ENABLED")
    paths = (("programs", True), ("per_layer", False)) if has_switch else (("evaluate", None),)

    def run(on):
        if on is not None:
            plan.EVAL_ENABLED = on
        return eng.evaluate(video, labels, chunk)
    same = None
    if has_switch:
        a, b = run(True), run(False)
        same = all(torch.equal(x, y) for x, y in zip(a, b))
    peak = {}
    for tag, on in paths:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        start = torch.cuda.memory_allocated(dev)
        for _ in range(args.warmup):
            run(on)
        torch.cuda.synchronize()
        peak[tag] = {"peak_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1), "resident_before_mb": round(start / 2 ** 20, 1)}
    ms = {tag: [] for tag, _ in paths}
    for _ in range(args.rounds):
        for tag, on in paths:
            ms[tag].append(_calls(lambda: run(on), args.calls))
    if has_switch:
        plan.EVAL_ENABLED = True
    clips = shape[0] * shape[1]
    out = {"clips_per_call": clips, "chunk": chunk, "bit_identical": same, "peak_memory_mb": peak}
    for tag, v in ms.items():
        med = statistics.median(v)
        out[tag] = {"clips_per_s": round(clips / med * 1e3, 1), "ms_per_call": round(med, 3), "rounds_ms": [round(x, 3) for x in v],
                    "spread": round((max(v) - min(v)) / med, 4)}
    if has_switch:
        out["programs_over_per_layer"] = round(statistics.median(ms["per_layer"]) / statistics.median(ms["programs"]), 4)
    pls = [v for k, v in model.__dict__.get("_avid_plans", {}).items() if k[0] == "eval" and v]
    out["program_records"] = sorted(sum(1 for k in range(pl.n_fwd) if pl.fwd_prog[k].op not in (0, plan.OP_WAIT)) for pl in pls)
    out["arena_mb"] = sorted(round(pl.fa_bytes / 2 ** 20, 1) for pl in pls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--repo", default=None, help="import the package from this checkout (default: the one this file lies in)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "dense evaluation clips/s (FinetuneStep.evaluate / ProbeStep.evaluate on R(2+1)D-18, 1 GPU)",
           "unit": "clips/s"}
    for name in args.cases.split(","):
        out[name] = _run(name, args, dev)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
