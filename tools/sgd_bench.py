"""Dev tool: what SGD with momentum costs next to Adam, on the GPU, alternating the two in one process.

1. kernel:  ``sgd_flat_kernel`` against ``adam_flat_kernel`` (the library's HIP-event timers) over flat buffers of the two-tower
   model's size (21.3 M fp32 elements): SGD moves 20 bytes per element (p, g, buf read; p, buf written), Adam 28.
2. step:    ``TrainStep.step`` at bench.py's default shapes (batch 64, 3x8x112x112 video, 240 000-row banks, 1024 negatives)
   with ``optimizer="sgd"`` against ``"adam"``.
3. loop:    the reference's loop shape (main-avid.py:169-178, ``loss.item()`` included) over ``parallel.DistributedDataParallel``
   with ``parallel.SGD`` against ``torch.optim.SGD`` — the same wrapper, the optimizer is the only difference — and both as a
   fraction of the SGD engine's rate (the figures utils/main_utils.py quotes for Adam are 0.79 / 0.93).

One JSON line per part.    python tools/sgd_bench.py [--rounds 50] [--steps 30] [--warmup 8] [--parts kernel,step,loop] [--out FILE]"""
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
SGD = dict(momentum=0.9, nesterov=True, weight_decay=1e-5)


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
    sp, sg, sb = buf(1.0), buf(0.01), buf(0.01)
    ap, ag, am, av = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_()
    for _ in range(3):                                             # warm both up outside the timers
        ops.sgd_flat(sp, sg, sb, 1e-3, 0.9, 1e-5, True)
        ops.adam_flat(ap, ag, am, av, 2e-4, 0.9, 0.999, 1e-8, 1e-5, 1)
    torch.cuda.synchronize()
    lib.timing_enable(True)
    for r in range(rounds):
        ops.sgd_flat(sp, sg, sb, 1e-3, 0.9, 1e-5, True)
        ops.adam_flat(ap, ag, am, av, 2e-4, 0.9, 0.999, 1e-8, 1e-5, 4 + r)
    torch.cuda.synchronize()
    rep = lib.timing_report()
    lib.timing_enable(False)
    rec = {"part": "kernel", "elements": n, "rounds": rounds}
    for k in ("sgd_flat_kernel", "adam_flat_kernel"):
        ms = rep[k]["ms"] / rep[k]["launches"]
        rec[k] = {"ms": round(ms, 4), "bytes": rep[k]["bytes"] / rep[k]["launches"],
                  "TB_s": round(rep[k]["bytes"] / rep[k]["launches"] / ms / 1e9, 2), "launches": rep[k]["launches"]}
    rec["sgd_over_adam"] = round(rec["sgd_flat_kernel"]["ms"] / rec["adam_flat_kernel"]["ms"], 3)
    return rec


def alternate(runs, steps, warmup, blocks=3):
    """{name: ms per step}: the runs take turns, ``blocks`` windows of ``steps`` steps each, every window ended by a synchronise."""
    for one in runs.values():
        for i in range(warmup):
            one(i)
    torch.cuda.synchronize()
    ms = {n: [] for n in runs}
    for b in range(blocks):
        for n, one in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                one(warmup + b * steps + i)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / steps * 1e3)
    return {n: {"ms_per_step": round(sorted(v)[len(v) // 2], 3), "windows": [round(x, 3) for x in v]} for n, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--parts", default="kernel,step,loop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sgd_bench measures on the GPU: there is nothing to report without one"
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
    sgd_ms = None
    if "step" in parts:
        engines = {}
        for name, kw in (("sgd", dict(lr=1e-3, optimizer="sgd", **SGD)), ("adam", dict(lr=2e-4, weight_decay=1e-5))):
            m, c = fresh(dev)
            engines[name] = parallel.TrainStep(m, c, **kw)
        res = alternate({n: (lambda i, e=e: e.step(video, audio, ids[i % 64])) for n, e in engines.items()}, a.steps, a.warmup)
        sgd_ms = res["sgd"]["ms_per_step"]
        emit({"part": "step", "batch": BS, "TrainStep": res, "sgd_over_adam": round(sgd_ms / res["adam"]["ms_per_step"], 4),
              "clips_s": {n: round(BS / r["ms_per_step"] * 1e3, 1) for n, r in res.items()}})
        del engines
    if "loop" in parts:
        runs = {}
        for name, make in (("parallel.SGD", parallel.SGD), ("torch.optim.SGD", torch.optim.SGD)):
            m, c = fresh(dev)
            net = parallel.DistributedDataParallel(m, device_ids=[dev.index])
            opt = make(net.parameters(), lr=1e-3, **SGD)

            def one(i, net=net, c=c, opt=opt):
                v, au = net(video, audio)
                loss, _ = c(v, au, ids[i % 64])
                loss.item()                                        # main-avid.py:174, before the backward pass
                opt.zero_grad()
                loss.backward()
                opt.step()
            runs[name] = one
        res = alternate(runs, a.steps, a.warmup)
        rec = {"part": "loop", "batch": BS, "wrapper": "avid_hip.parallel.DistributedDataParallel, no process group", "loop": res,
               "dropin_over_torch_time": round(res["parallel.SGD"]["ms_per_step"] / res["torch.optim.SGD"]["ms_per_step"], 4)}
        if sgd_ms is not None:
            rec["rate_against_the_sgd_engine"] = {n: round(sgd_ms / r["ms_per_step"], 3) for n, r in res.items()}
        emit(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
