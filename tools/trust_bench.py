"""Dev tool: what per-tensor hyper-parameters and trust ratios (LARS / LAMB) cost, on the GPU, the forms alternating in one process.

1. kernel:  over the flat layout of the pretraining model (141 tensors, 21.3 M fp32 elements, the usual exclusion of 1-d tensors as
   the table), by the library's HIP-event timers, in turns within every round: the plain kernels (``sgd_flat_kernel`` 20 B per
   element, ``adam_flat_kernel`` 28 B), the norm pass alone (``seg_sumsq_kernel`` over p and g, 8 B), ``sgd_flat_table_kernel`` (20 B),
   the LARS pair (``sgd_table_norm_kernel`` 8 B + ``sgd_flat_table_kernel`` 20 B), ``adam_flat_table_kernel`` (28 B) and the two LAMB
   passes (``lamb_moments_kernel`` 24 B + ``lamb_update_kernel`` 16 B), with ``seg_finish_kernel`` behind every norm pass.  ``blocks``
   windows of ``rounds`` rounds each: the median window and the spread per kernel, achieved bytes per second, and against the
   yardstick — the plain kernel's byte rate in the same run times the form's bytes.
2. step:    ``TrainStep.step`` at bench.py's default shapes (batch 64) under "adam", "adam" with an empty list of rules (the table
   kernel in one piece: what the lost optimizer overlap costs on top of the kernel), "lamb", "sgd", "sgd" with rules and "lars",
   taking turns; ms and shader cycles per step.
3. parent:  ``bench.py --gpus 1`` of this tree and of another checkout (``--parent-tree``: the parent commit, built) in child
   processes that take turns: the default step did not move.

One JSON line per part.    python tools/trust_bench.py [--rounds 20] [--steps 30] [--warmup 8] [--blocks 5] [--parts kernel,step]
                                                       [--parent-tree DIR --parent-rounds 3] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
from avid_hip import lib, ops, parallel  # noqa: E402
from guard_bench import BANK, BS, alternate, fresh  # noqa: E402

# form -> (kernels whose times add up to it, the plain kernel it is held against)
FORMS = {"norms(p, g)": (("seg_sumsq_kernel", "seg_finish_kernel"), "sgd_flat_kernel"),
         "sgd_flat_table": (("sgd_flat_table_kernel",), "sgd_flat_kernel"),
         "lars": (("sgd_table_norm_kernel", "seg_finish_kernel", "sgd_flat_table_kernel"), "sgd_flat_kernel"),
         "adam_flat_table": (("adam_flat_table_kernel",), "adam_flat_kernel"),
         "lamb": (("lamb_moments_kernel", "seg_finish_kernel", "lamb_update_kernel"), "adam_flat_kernel")}


def kernel_part(dev, rounds, blocks):
    m, _ = fresh(dev)
    flat = parallel.FlatParams(m)
    n = flat.numel
    decay = [0.0 if p.ndim <= 1 else 1e-5 for p in flat.params]
    tab = ops.SegmentTable(flat, 1.0, decay, [p.ndim > 1 for p in flat.params])
    numels = sorted(tab.numels)
    g = torch.Generator().manual_seed(1)

    def buf(scale):
        return (scale * torch.randn(n, generator=g)).to(dev)
    p, gr, mo, v = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_()
    # every form runs alone between two timing reports: the kernels' names are shared between forms
    runs = {"sgd_flat_kernel": lambda s: ops.sgd_flat(p, gr, mo, 1e-3, 0.9, 1e-5, True),
            "adam_flat_kernel": lambda s: ops.adam_flat(p, gr, mo, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, s),
            "norms(p, g)": lambda s: ops.segment_sumsq(tab, p, gr),
            "sgd_flat_table": lambda s: ops.sgd_flat_table(tab, p, gr, mo, 1e-3, 0.9, True),
            "lars": lambda s: ops.sgd_flat_table(tab, p, gr, mo, 1e-3, 0.9, True, trust_coefficient=0.001),
            "adam_flat_table": lambda s: ops.adam_flat_table(tab, p, gr, mo, v, 2e-4, 0.9, 0.999, 1e-8, s),
            "lamb": lambda s: ops.lamb_flat(tab, p, gr, mo, v, 2e-4, 0.9, 0.999, 1e-8, s)}
    for s in range(3):
        for run in runs.values():
            run(1 + s)
    torch.cuda.synchronize()
    windows = {name: [] for name in runs}
    parts, nbytes = {}, {}
    for b in range(blocks):
        acc = {name: 0.0 for name in runs}
        for r in range(rounds):
            for name, run in runs.items():          # the forms take turns within a round
                lib.timing_enable(True)
                run(4 + b * rounds + r)
                torch.cuda.synchronize()
                rep = lib.timing_report()
                lib.timing_enable(False)
                acc[name] += sum(k["ms"] for k in rep.values())
                nbytes[name] = sum(k["bytes"] for k in rep.values())
                parts[name] = {k: round(x["ms"], 4) for k, x in rep.items()}
        for name in runs:
            windows[name].append(acc[name] / rounds)
    rec = {"part": "kernel", "elements": n, "segments": tab.S, "chunks": tab.n_chunks,
           "segments_under_one_chunk": sum(1 for x in numels if x < lib.SEG_CHUNK), "smallest": numels[0], "largest": numels[-1],
           "rounds": rounds, "blocks": blocks}
    med = {}
    for name in runs:
        w = sorted(windows[name])
        med[name] = w[len(w) // 2]
        rec[name] = {"ms": round(med[name], 4), "min": round(w[0], 4), "max": round(w[-1], 4), "bytes": nbytes[name],
                     "GB_s": round(nbytes[name] / med[name] / 1e6, 1), "last_round_kernels_ms": parts[name]}
    for name, (_, plain) in FORMS.items():
        yard = nbytes[name] / (nbytes[plain] / med[plain])
        rec[name]["yardstick_ms"] = round(yard, 4)
        rec[name]["over_yardstick"] = round(med[name] / yard, 3)
        rec[name]["over_plain"] = round(med[name] / med[plain], 3)
    return rec


def parent_part(parent_tree, rounds, steps, warmup):
    """bench.py of the two trees in child processes that take turns; clips/s of each run."""
    out = {"this": [], "parent": []}
    cmd = ["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-extra"]
    for r in range(rounds):
        for name, tree in (("parent", parent_tree), ("this", REPO)):
            proc = subprocess.run([sys.executable, os.path.join(tree, "bench.py")] + cmd, capture_output=True, text=True, cwd=tree,
                                  timeout=600)
            if proc.returncode != 0:
                raise RuntimeError(f"bench.py of {tree} failed: {proc.stderr[-2000:]}")
            line = json.loads(proc.stdout.strip().splitlines()[-1])
            out[name].append(line["value"])
    med = {k: sorted(v)[len(v) // 2] for k, v in out.items()}
    return {"part": "parent", "rounds": rounds, "steps": steps, "clips_per_s": out, "median": med,
            "this_over_parent": round(med["this"] / med["parent"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--parts", default="kernel,step")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--parent-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trust_bench measures on the GPU: there is nothing to report without one"
    dev = torch.device("cuda:0")
    parts = a.parts.split(",")
    g = torch.Generator().manual_seed(1234)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            open(a.out, "w").write("\n".join(lines) + "\n")

    if "kernel" in parts:
        emit(kernel_part(dev, a.rounds, a.blocks))
    if "step" in parts:
        video = torch.randn(BS, 3, 8, 112, 112, generator=g).to(dev)
        audio = torch.randn(BS, 1, 40, 100, generator=g).to(dev)
        ids = torch.stack([torch.randperm(BANK, generator=g)[:BS] for _ in range(64)]).to(dev)
        sgd = dict(lr=1e-3, momentum=0.9, nesterov=True)
        engines = {}
        for name, kw in (("adam", {}), ("adam_rules", dict(param_rules=[])), ("lamb", dict(optimizer="lamb")),
                         ("sgd", dict(optimizer="sgd", **sgd)), ("sgd_rules", dict(optimizer="sgd", param_rules=[], **sgd)),
                         ("lars", dict(optimizer="lars", **sgd))):
            m, c = fresh(dev)
            if name in ("lamb", "lars"):
                kw = dict(kw, param_rules=parallel.rules_no_decay_1d(m))
            engines[name] = parallel.TrainStep(m, c, **kw)
        res = alternate({n: (lambda i, e=e: e.step(video, audio, ids[i % 64])) for n, e in engines.items()}, a.steps, a.warmup,
                        a.blocks, dev)
        over = {n: round(r["ms_per_step"] / res["adam" if n in ("adam_rules", "lamb") else "sgd"]["ms_per_step"], 4)
                for n, r in res.items() if n not in ("adam", "sgd")}
        emit({"part": "step", "batch": BS, "TrainStep": res, "over_plain_engine": over})
        del engines
    if a.parent_tree:
        emit(parent_part(os.path.abspath(a.parent_tree), a.parent_rounds, a.steps, a.warmup))


if __name__ == "__main__":
    main()
