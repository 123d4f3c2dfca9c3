#!/usr/bin/env python
"""Per-step time of fine-tuning and linear-probe training around the audio tower, launch programs against the per-layer path.

    python tools/audio_downstream_bench.py [--batch 64] [--steps 30] [--warmup 5] [--rounds 5] [--loops A,B] [--json PATH]

The shipped audio shape: log-spectrograms 1 x 200 x 257, batch 64; 50 classes; the probe with the shipped-style heads
``AdaptiveMaxPool2d((12,12))``, ``((8,8))``, ``((6,6))``, ``((4,4))`` on conv2x..conv5x.  Four loops of the SAME tree in ONE
process, alternating round by round (other work shares the host, so a difference is read within a round):

* ``finetune / programs``: ``parallel.FinetuneStep.step`` — forward program ending in ``avid_cls_loss``, backward program, flat Adam.
* ``finetune / per-layer``: what an audio user had before the programs compiled this tower — ``model(spect)`` walking the modules
  (one autograd node per layer), ``ops.cls_loss``, ``backward``, ``parallel.Adam`` (the one-launch optimizer).
* ``probe / programs`` and ``probe / per-layer``: the same pair for ``parallel.ProbeStep`` / ``MOSTModel``.

Each timing is a host clock around ``steps`` steps that end in a device synchronise, after ``warmup`` steps of the same loop;
the figure reported per loop is the median over the rounds, with the spread.  Both loops of a pair start from the same weights and
see the same batches and dropout masks; the last loss of every loop is reported next to the times (the two paths agree bit for
bit up to the grouped weight-gradient launch, tests/test_gpu_audio_downstream.py).  Needs a GPU: without one this fails, it does
not fall back.  ``--loops probe/programs`` (a comma list) runs only the named loops — one loop at a time under a kernel trace."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))

POOLS = ["AdaptiveMaxPool2d((12,12))", "AdaptiveMaxPool2d((8,8))", "AdaptiveMaxPool2d((6,6))", "AdaptiveMaxPool2d((4,4))"]
DIMS = [64 * 144, 128 * 64, 256 * 36, 512 * 16]
STAGES = ["conv2x", "conv3x", "conv4x", "conv5x"]
N_CLASSES = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loops", default=None, help="comma list of loops to run (default: all four)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("audio_downstream_bench: no GPU")
    import models
    from avid_hip import ops, parallel, plan
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    n_batches = 4
    xs = [torch.randn((args.batch, 1, 200, 257), generator=g).to(dev) for _ in range(n_batches)]
    ys = [torch.randint(0, N_CLASSES, (args.batch,), generator=g).to(dev) for _ in range(n_batches)]

    ft = models.ClassificationWrapper(models.Conv2D(), N_CLASSES, "pool", 512, use_dropout=True).to(dev).train()
    ft_ref = copy.deepcopy(ft)
    pr = models.MOSTModel(models.Conv2D(), N_CLASSES, STAGES, DIMS, POOLS, use_bn=True).to(dev).train()
    pr_ref = copy.deepcopy(pr)

    ft_eng = parallel.FinetuneStep(ft)
    pr_eng = parallel.ProbeStep(pr)
    ft_opt = parallel.Adam(list(ft_ref.parameters()), lr=1e-4)
    pr_opt = parallel.Adam([p for p in pr_ref.parameters() if p.requires_grad], lr=1e-4)

    def per_layer(model, x):
        prev, plan.ENABLED = plan.ENABLED, False
        try:
            return model(x)
        finally:
            plan.ENABLED = prev

    def ft_programs(i):
        return ft_eng.step(xs[i], ys[i])[0]

    def ft_per_layer(i):
        ft_opt.zero_grad()
        logits = per_layer(ft_ref, xs[i])
        loss, _, _, d = ops.cls_loss(logits.detach(), ys[i], grad_scale=1.0)
        logits.backward(d)
        ft_opt.step()
        return loss

    def pr_programs(i):
        return pr_eng.step(xs[i], ys[i])[0].sum()

    def pr_per_layer(i):
        pr_opt.zero_grad()
        out = per_layer(pr_ref, xs[i])
        res = [ops.cls_loss(v.detach(), ys[i], grad_scale=1.0) for v in out.values()]
        torch.autograd.backward(list(out.values()), [r[3] for r in res])
        pr_opt.step()
        return sum(r[0] for r in res)

    loops = {"finetune/programs": ft_programs, "finetune/per-layer": ft_per_layer,
             "probe/programs": pr_programs, "probe/per-layer": pr_per_layer}
    if args.loops:
        want = args.loops.split(",")
        unknown = [k for k in want if k not in loops]
        if unknown:
            raise SystemExit(f"audio_downstream_bench: unknown loop(s) {unknown}; known: {list(loops)}")
        loops = {k: loops[k] for k in want}
    times = {k: [] for k in loops}
    last = {}
    for rnd in range(args.rounds):
        for name, fn in loops.items():
            for i in range(args.warmup):
                fn(i % n_batches)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                loss = fn(i % n_batches)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            last[name] = float(loss)
    ops.check_device_errors(dev)
    result = {"shape": [args.batch, 1, 200, 257], "n_classes": N_CLASSES, "steps": args.steps, "warmup": args.warmup,
              "rounds": args.rounds, "ms_per_step": {}, "last_loss": last}
    for name, ts in times.items():
        result["ms_per_step"][name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}
    for kind in ("finetune", "probe"):
        if kind + "/per-layer" not in times or kind + "/programs" not in times:
            continue
        a, b = result["ms_per_step"][kind + "/per-layer"]["median"], result["ms_per_step"][kind + "/programs"]["median"]
        result[kind + "_speedup"] = round(a / b, 3)
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
