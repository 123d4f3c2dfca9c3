"""Dev tool: what ``TrainStep(virtual_ranks=R)`` costs, on the GPU.

1. kernel:  ``grad_accum_flat_kernel`` (12 bytes per element: two reads, one write) next to ``adam_flat_kernel`` (28) on the same
   flat buffers of the two-tower model's size, the library's HIP-event timers, the two alternating; both forms the engine
   launches (``acc = acc + g`` and ``g = acc + g``).  The yardstick is Adam's achieved bytes/s in the same run.
2. step:    ``TrainStep.step`` at bench.py's shapes (3x8x112x112 + 1x40x100, GLOBAL batch 64, 240 000-row banks, 1024 negatives)
   for R = 1, 2, 4, 8, one engine alive at a time: ms per step (median of the windows), clips/s and
   ``torch.cuda.max_memory_allocated`` over the timed windows.  R = 1 runs first and last (the spread of the same command).
3. parent:  with ``--parent DIR`` (a checkout of the parent commit with its library built) the R = 1 step of THAT tree, in a
   process of its own before and after part 2: the default path did not move.

One JSON line per record.   python tools/virtual_ranks_bench.py [--steps 30] [--warmup 8] [--windows 3] [--parent DIR] [--out FILE]"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BS, BANK, NEG = 64, 240000, 1024


def _import(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "avid-cma_amd"))


def fresh(dev):
    import criterions
    import models
    import torch
    torch.manual_seed(0)
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(dev).train()
    c = criterions.AVID(num_data=BANK, embedding_dim=m.out_dim, num_negatives=NEG, momentum=0.5, xModal_coeff=1., wModal_coeff=0.,
                        device=dev.index)
    return m, c


def kernel_part(dev, n, rounds):
    import torch
    from avid_hip import lib, ops
    g = torch.Generator().manual_seed(1)

    def buf(scale):
        return (scale * torch.randn(n, generator=g)).to(dev)
    p, grad, m, v, acc = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_(), buf(0.0)
    for _ in range(3):                                             # warm both up outside the timers
        ops.grad_accum_flat(acc, acc, grad)
        ops.adam_flat(p, grad, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, 1)
    torch.cuda.synchronize()
    rec = {"part": "kernel", "elements": n, "rounds": rounds}
    for form, dst in (("acc=acc+g", acc), ("g=acc+g", grad)):
        acc.zero_()
        grad.normal_(0.0, 0.01, generator=None)
        lib.timing_enable(True)
        for r in range(rounds):
            ops.grad_accum_flat(dst, acc, grad)
            ops.adam_flat(p, grad, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, 4 + r)
            if dst is grad:
                grad.mul_(0.5)                                     # (keeps the in-place sum finite; not under a library timer)
        torch.cuda.synchronize()
        rep = lib.timing_report()
        lib.timing_enable(False)
        one = {}
        for k in ("grad_accum_flat_kernel", "adam_flat_kernel"):
            ms = rep[k]["ms"] / rep[k]["launches"]
            one[k] = {"ms": round(ms, 4), "bytes": rep[k]["bytes"] / rep[k]["launches"],
                      "TB_s": round(rep[k]["bytes"] / rep[k]["launches"] / ms / 1e9, 3), "launches": rep[k]["launches"]}
        one["accum_bytes_s_over_adam"] = round(one["grad_accum_flat_kernel"]["TB_s"] / one["adam_flat_kernel"]["TB_s"], 3)
        rec[form] = one
    return rec


def step_record(dev, R, steps, warmup, windows, tag):
    """One engine: warm-up, then ``windows`` timed windows of ``steps`` steps, each ended by a synchronise."""
    import torch
    from avid_hip import parallel
    g = torch.Generator().manual_seed(1234)
    video = torch.randn(BS, 3, 8, 112, 112, generator=g).to(dev)
    audio = torch.randn(BS, 1, 40, 100, generator=g).to(dev)
    ids = torch.stack([torch.randperm(BANK, generator=g)[:BS] for _ in range(64)]).to(dev)
    m, c = fresh(dev)
    eng = parallel.TrainStep(m, c, **({"virtual_ranks": R} if R > 1 else {}))
    for i in range(warmup):
        loss = eng.step(video, audio, ids[i % 64])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for w in range(windows):
        t0 = time.perf_counter()
        for i in range(steps):
            loss = eng.step(video, audio, ids[(warmup + w * steps + i) % 64])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    med = sorted(ms)[len(ms) // 2]
    rec = {"part": "step", "tree": tag, "virtual_ranks": R, "global_batch": BS, "shard_batch": BS // R, "ms_per_step": round(med, 3),
           "windows": [round(x, 3) for x in ms], "clips_s": round(BS / med * 1e3, 1),
           "max_memory_allocated_MiB": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
           "memory_allocated_MiB": round(torch.cuda.memory_allocated(dev) / 2 ** 20, 1), "loss": round(float(loss), 5)}
    del eng, m, c, loss
    gc.collect()                                                   # (engine and plans refer to each other: nothing of this run stays)
    torch.cuda.empty_cache()
    return rec


def child(tree, a):
    """The R = 1 step of the tree at ``tree`` (its own package and library), in this process."""
    _import(tree)
    import torch
    assert torch.cuda.is_available(), "virtual_ranks_bench measures on the GPU: there is nothing to report without one"
    print(json.dumps(step_record(torch.device("cuda:0"), 1, a.steps, a.warmup, a.windows, a.tag)), flush=True)


def run_parent(a, lines, tag):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(a.parent), "--tag", tag,
                          "--steps", str(a.steps), "--warmup", str(a.warmup), "--windows", str(a.windows)],
                         capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(f"the parent tree's run failed ({out.returncode}):\n{out.stderr[-2000:]}")
    lines.append(out.stdout.strip().splitlines()[-1])
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--ranks", default="1,2,4,8,1")
    ap.add_argument("--parts", default="kernel,step")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a)
    lines = []
    if a.parent:
        run_parent(a, lines, "parent:first")
    _import(REPO)
    import torch
    from avid_hip import parallel
    assert torch.cuda.is_available(), "virtual_ranks_bench measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda:0")

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    parts = a.parts.split(",")
    if "kernel" in parts:
        n = parallel.FlatParams(fresh(dev)[0]).numel
        emit(kernel_part(dev, n, a.rounds))
        gc.collect()
        torch.cuda.empty_cache()
    if "step" in parts:
        base = None
        for R in [int(x) for x in a.ranks.split(",")]:
            rec = step_record(dev, R, a.steps, a.warmup, a.windows, "this")
            base = rec["ms_per_step"] if base is None else base
            rec["over_R1"] = round(rec["ms_per_step"] / base, 4)
            emit(rec)
    if a.parent:
        run_parent(a, lines, "parent:last")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
