"""Dev tool: what the step guard costs, on the GPU, the configurations alternating in one process.

1. kernel:  ``avid_grad_guard`` alone (the library's HIP-event timers: ``grad_sumsq_kernel`` + ``grad_guard_finish_kernel``) over
   a flat buffer of the two-tower model's size (21.3 M fp32 elements, 85 MB read once), next to ``adam_flat_kernel`` and
   ``adam_flat_guarded_kernel`` over the same buffers.
2. step:    ``TrainStep.step`` at bench.py's default shapes (batch 64, 3x8x112x112 video, 240 000-row banks, 1024 negatives)
   three ways, taking turns: guard off (the step as it always was, the overlapped two-slice Adam), ``max_grad_norm`` only,
   ``max_grad_norm`` + ``skip_nonfinite``.  ms per step and, with the mean shader clock over each window (bench.py's sampler),
   shader cycles per step; the yardstick is guard off in the same run.

One JSON line per part.    python tools/guard_bench.py [--rounds 50] [--steps 30] [--warmup 8] [--blocks 5] [--parts kernel,step] [--out FILE]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
import torch  # noqa: E402
from avid_hip import lib, ops, parallel  # noqa: E402

BS, BANK, NEG = 64, 240000, 1024
CONFIGS = (("off", {}), ("clip", dict(max_grad_norm=1e3)), ("clip_skip", dict(max_grad_norm=1e3, skip_nonfinite=True)))


def fresh(dev):
    import criterions
    import models
    torch.manual_seed(0)
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(dev).train()
    c = criterions.AVID(num_data=BANK, embedding_dim=m.out_dim, num_negatives=NEG, momentum=0.5, xModal_coeff=1., wModal_coeff=0.,
                        device=dev.index)
    return m, c


def kernel_part(dev, n, rounds):
    g = torch.Generator().manual_seed(1)

    def buf(scale):
        return (scale * torch.randn(n, generator=g)).to(dev)
    p, gr, m, v = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_()
    guard = ops.StepGuard(dev)

    def one(step):
        ops.grad_guard(gr, guard, 1.0, 1e3, True)
        ops.adam_flat_guarded(p, gr, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, step, guard)
        ops.adam_flat(p, gr, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, step)
    for s in range(3):                                             # warm up outside the timers
        one(1 + s)
    torch.cuda.synchronize()
    lib.timing_enable(True)
    for r in range(rounds):
        one(4 + r)
    torch.cuda.synchronize()
    rep = lib.timing_report()
    lib.timing_enable(False)
    rec = {"part": "kernel", "elements": n, "rounds": rounds, "skipped_total": int(guard.skipped_total)}
    for k in ("grad_sumsq_kernel", "grad_guard_finish_kernel", "adam_flat_guarded_kernel", "adam_flat_kernel"):
        ms = rep[k]["ms"] / rep[k]["launches"]
        rec[k] = {"ms": round(ms, 4), "bytes": rep[k]["bytes"] / rep[k]["launches"],
                  "GB_s": round(rep[k]["bytes"] / rep[k]["launches"] / ms / 1e6, 1), "launches": rep[k]["launches"]}
    guard_ms = rec["grad_sumsq_kernel"]["ms"] + rec["grad_guard_finish_kernel"]["ms"]
    rec["avid_grad_guard"] = {"ms": round(guard_ms, 4), "GB_s": round(4.0 * n / guard_ms / 1e6, 1)}
    return rec


def alternate(runs, steps, warmup, blocks, dev):
    """{name: ms, shader clock and shader cycles per step}: the runs take turns, ``blocks`` windows of ``steps`` steps each, every
    window ended by a synchronise; medians over the windows."""
    from bench import ClockSampler
    for one in runs.values():
        for i in range(warmup):
            one(i)
    torch.cuda.synchronize()
    ms, ghz = {n: [] for n in runs}, {n: [] for n in runs}
    for b in range(blocks):
        for n, one in runs.items():
            torch.cuda.synchronize()
            sampler = ClockSampler(dev.index or 0)
            sampler.start()
            t0 = time.perf_counter()
            for i in range(steps):
                one(warmup + b * steps + i)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / steps * 1e3)
            ghz[n].append(sampler.stop())

    def med(v):
        v = sorted(x for x in v if x is not None)
        return v[len(v) // 2] if v else None
    out = {}
    for n in runs:
        m, c = med(ms[n]), med(ghz[n])
        cyc = [a * b for a, b in zip(ms[n], ghz[n]) if b is not None]
        out[n] = {"ms_per_step": round(m, 3), "windows": [round(x, 3) for x in ms[n]], "shader_clock_ghz": None if c is None else round(c, 3),
                  "mcycles_per_step": round(med(cyc), 2) if cyc else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parts", default="kernel,step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "guard_bench measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    g = torch.Generator().manual_seed(1234)
    video = torch.randn(BS, 3, 8, 112, 112, generator=g).to(dev)
    audio = torch.randn(BS, 1, 40, 100, generator=g).to(dev)
    ids = torch.stack([torch.randperm(BANK, generator=g)[:BS] for _ in range(64)]).to(dev)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if "kernel" in parts:
        m, _ = fresh(dev)
        n = parallel.FlatParams(m).numel
        del m
        emit(kernel_part(dev, n, a.rounds))
    if "step" in parts:
        engines = {}
        for name, kw in CONFIGS:
            m, c = fresh(dev)
            engines[name] = parallel.TrainStep(m, c, **kw)
        res = alternate({n: (lambda i, e=e: e.step(video, audio, ids[i % 64])) for n, e in engines.items()}, a.steps, a.warmup,
                        a.blocks, dev)
        off = res["off"]["ms_per_step"]
        emit({"part": "step", "batch": BS, "TrainStep": res,
              "over_guard_off": {n: round(r["ms_per_step"] / off, 4) for n, r in res.items()},
              "skipped_total": {n: (None if e.guard is None else int(e.guard.skipped_total)) for n, e in engines.items()},
              "grad_norm": {n: (None if e.guard is None else round(float(e.guard.grad_norm), 6)) for n, e in engines.items()}})
        del engines
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
