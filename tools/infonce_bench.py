#!/usr/bin/env python
"""What the in-batch InfoNCE criterion costs on the GPU.

    python tools/infonce_bench.py [--sizes 64,256,1024,4096] [--dim 128] [--iters 20] [--warmup 5] [--rounds 5]
                                  [--parts criterion,step] [--batch 64] [--steps 10] [--json PATH]

Two measurements of the SAME tree in ONE process (other work shares the host, so a difference is read within a round):

* ``criterion``: ``criterions.InfoNCE`` alone, forward + backward, on unnormalised embeddings [G, D] with b = G (one
  process owns the whole batch), against the same loss written in torch ops — ``normalize``, one ``matmul``, two
  ``cross_entropy`` and the autograd backward — alternating round by round.  Each timing is a host clock around ``iters``
  forward + backward pairs that end in a device synchronise, after ``warmup`` pairs of the same loop; the median over the
  rounds is reported with the spread.  The two losses must agree to 1e-4 relative or the script fails.
* ``step``: ``parallel.TrainStep.step`` at batch ``--batch`` (3 x 8 x 112 x 112 clips, 1 x 200 x 257 spectrograms) under
  ``InfoNCE`` against the same step under ``AVID`` (65 536-row banks, 1024 negatives), alternating likewise.

Needs a GPU: without one this fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))


def _timed(fn, iters, warmup, torch):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        out = fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, out


def _summary(ts):
    return {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def bench_criterion(args, torch, dev):
    import criterions
    F = torch.nn.functional
    res = {}
    for G in args.sizes:
        g = torch.Generator().manual_seed(G)
        e1 = torch.randn((G, args.dim), generator=g).to(dev).requires_grad_(True)
        e2 = (0.7 * e1.detach().cpu() + 0.7 * torch.randn((G, args.dim), generator=g)).to(dev).requires_grad_(True)
        crit = criterions.InfoNCE(args.dim, device=dev.index, temperature=0.07)
        tgt = torch.arange(G, device=dev)

        def hip(i):
            e1.grad = e2.grad = None
            loss, _ = crit(e1, e2, tgt)
            loss.backward()
            return loss.detach()

        def chain(i):
            e1.grad = e2.grad = None
            S = F.normalize(e1, dim=1) @ F.normalize(e2, dim=1).t() / 0.07
            loss = 0.5 * F.cross_entropy(S, tgt) + 0.5 * F.cross_entropy(S.t(), tgt)
            loss.backward()
            return loss.detach()
        loops = {"hip": hip, "torch": chain}
        times, last = {k: [] for k in loops}, {}
        for _ in range(args.rounds):
            for name, fn in loops.items():
                ms, loss = _timed(fn, args.iters, args.warmup, torch)
                times[name].append(ms)
                last[name] = float(loss)
        if abs(last["hip"] - last["torch"]) > 1e-4 * abs(last["torch"]):
            raise SystemExit(f"G = {G}: the kernel's loss {last['hip']!r} and the torch chain's {last['torch']!r} disagree")
        res[str(G)] = {"ms": {k: _summary(v) for k, v in times.items()}, "loss": last,
                       "hip_over_torch": round(statistics.median(times["hip"]) / statistics.median(times["torch"]), 3)}
    return res


def bench_step(args, torch, dev):
    import criterions
    import models
    from avid_hip import parallel
    g = torch.Generator().manual_seed(1)
    B = args.batch
    vids = [torch.randn((B, 3, 8, 112, 112), generator=g).to(dev) for _ in range(2)]
    auds = [torch.randn((B, 1, 200, 257), generator=g).to(dev) for _ in range(2)]
    ids = [torch.randperm(65536, generator=g)[:B].to(dev) for _ in range(2)]
    engines = {}
    for kind in ("avid", "infonce"):
        torch.manual_seed(0)
        m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(dev).train()
        crit = (criterions.AVID(num_data=65536, embedding_dim=128, num_negatives=1024, momentum=0.5, device=dev.index)
                if kind == "avid" else criterions.InfoNCE(128, device=dev.index, temperature=0.07))
        engines[kind] = parallel.TrainStep(m, crit)
    loops = {k: (lambda i, e=e: e.step(vids[i % 2], auds[i % 2], ids[i % 2])) for k, e in engines.items()}
    times, last = {k: [] for k in loops}, {}
    for _ in range(args.rounds):
        for name, fn in loops.items():
            ms, loss = _timed(fn, args.steps, args.warmup, torch)
            times[name].append(ms)
            last[name] = float(loss)
    return {"batch": B, "ms_per_step": {k: _summary(v) for k, v in times.items()}, "last_loss": last,
            "infonce_minus_avid_ms": round(statistics.median(times["infonce"]) - statistics.median(times["avid"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parts", default="criterion,step")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    args.sizes = [int(s) for s in args.sizes.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/infonce_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "dim": args.dim}
    for part in args.parts.split(","):
        res[part] = {"criterion": bench_criterion, "step": bench_step}[part](args, torch, dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
