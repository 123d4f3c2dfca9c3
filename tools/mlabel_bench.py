#!/usr/bin/env python
"""What multi-label fine-tuning and evaluation cost on the GPU.

    python tools/mlabel_bench.py [--batch 64] [--steps 20] [--warmup 5] [--rounds 5] [--parts step,metric,loss] [--json PATH]

Three measurements of the SAME tree in ONE process (other work shares the host, so a difference is read within a round):

* ``step``: ``parallel.FinetuneStep.step`` with ``loss="bce"`` (527 classes, float32 targets [B, 527], a ``pos_weight``) against
  the ``loss="ce"`` step of the same model and batch, for the video tower (clips 3 x 8 x 112 x 112) and the audio tower
  (log-spectrograms 1 x 200 x 257), alternating round by round.  Each timing is a host clock around ``steps`` steps that end in a
  device synchronise, after ``warmup`` steps of the same loop; the median over the rounds is reported with the spread.
* ``metric``: ``ops.rank_metrics`` at AudioSet's evaluation size — N = 20 371 clips, C = 527 classes, about 2 positives per clip
  spread over 526 classes, and one dense class with P = N / 2 — against (a) a torch-on-GPU sort-and-cumsum formulation of the
  same two definitions (per class: sort descending, cumulative positives, the last index of every tie group) and (b)
  scikit-learn's ``average_precision_score`` / ``roc_auc_score`` on the host, the copy of [N, C] to the host included.  The
  three agree to 1e-9 or the script fails.
* ``loss``: ``ops.mlabel_loss`` at V x clips x C = 1900 x 10 x 527 (10^7 elements), with and without ``dlogits``: kernel time
  from device events against the bytes it moves (logits, gradient; targets and confidences once per video).

Needs a GPU: without one this fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))

N_CLASSES = 527
EVAL_N = 20371


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


def bench_step(args, torch, dev):
    import models
    from avid_hip import parallel
    g = torch.Generator().manual_seed(1)
    shapes = {"video": (args.batch, 3, 8, 112, 112), "audio": (args.batch, 1, 200, 257)}
    res = {}
    for tower, shape in shapes.items():
        make = (lambda: models.R2Plus1D(18)) if tower == "video" else models.Conv2D
        xs = [torch.randn(shape, generator=g).to(dev) for _ in range(2)]
        ys = [torch.randint(0, N_CLASSES, (args.batch,), generator=g).to(dev) for _ in range(2)]
        ts = [(torch.rand((args.batch, N_CLASSES), generator=g) < 2.0 / N_CLASSES).float().to(dev) for _ in range(2)]
        pw = torch.linspace(1.0, 20.0, N_CLASSES)
        engines = {}
        for kind in ("ce", "bce"):
            torch.manual_seed(0)
            m = models.ClassificationWrapper(make(), N_CLASSES, "pool", 512, use_dropout=True).to(dev).train()
            engines[kind] = parallel.FinetuneStep(m, loss=kind, pos_weight=pw if kind == "bce" else None)
        loops = {"ce": lambda i: engines["ce"].step(xs[i % 2], ys[i % 2])[0],
                 "bce": lambda i: engines["bce"].step(xs[i % 2], ts[i % 2])[0]}
        times, last = {k: [] for k in loops}, {}
        for _ in range(args.rounds):
            for name, fn in loops.items():
                ms, loss = _timed(fn, args.steps, args.warmup, torch)
                times[name].append(ms)
                last[name] = float(loss)
        res[tower] = {"shape": list(shape), "ms_per_step": {k: _summary(v) for k, v in times.items()}, "last_loss": last,
                      "bce_minus_ce_ms": round(statistics.median(times["bce"]) - statistics.median(times["ce"]), 4)}
        del engines
        torch.cuda.empty_cache()
    return res


def _torch_metrics(scores, targets, torch):
    """Per-class AP and AUC by one descending sort per class (all classes at once): the step-wise AP over the tie groups and the
    tie-aware AUC, in float64 on the device."""
    N, C = scores.shape
    s, order = torch.sort(scores.t().contiguous(), dim=1, descending=True)
    pos = torch.gather((targets.t() >= 0.5).to(torch.float64), 1, order)
    P = pos.sum(1)
    Nn = N - P
    tp = pos.cumsum(1)
    idx = torch.arange(N, device=scores.device)
    last = torch.ones((C, N), dtype=torch.bool, device=scores.device)
    last[:, :-1] = s[:, 1:] != s[:, :-1]                                 # the last sample of every tie group
    # the counts at the END of a sample's tie group: TP and TP + FP among the scores >= its own
    end = torch.where(last, idx.expand(C, N), torch.full((C, N), N, device=scores.device)).flip(1).cummin(1).values.flip(1)
    tp_ge = torch.gather(tp, 1, end)
    n_ge = (end + 1).to(torch.float64)
    ap = (pos * tp_ge / n_ge).sum(1) / P
    first = torch.ones((C, N), dtype=torch.bool, device=scores.device)
    first[:, 1:] = last[:, :-1]
    start = torch.where(first, idx.expand(C, N), torch.zeros((C, N), dtype=idx.dtype, device=scores.device)).cummax(1).values
    neg_ge = n_ge - tp_ge                                                # negatives >= s
    tp_before = torch.gather(tp, 1, start) - torch.gather(pos, 1, start)
    neg_gt = start.to(torch.float64) - tp_before                         # negatives > s
    u2 = (pos * (2.0 * (Nn[:, None] - neg_ge) + (neg_ge - neg_gt))).sum(1)
    return ap, u2 / (2.0 * P * Nn)


def bench_metric(args, torch, dev):
    import numpy as np
    from avid_hip import ops
    rng = np.random.default_rng(0)
    N, C = args.eval_n, N_CLASSES
    t = (rng.random((N, C)) < 2.0 / (C - 1)).astype(np.float32)
    t[:, 0] = (rng.random(N) < 0.5)
    s = (rng.standard_normal((N, C)) + 1.5 * t).astype(np.float32)
    s[:, 1] = np.round(s[:, 1], 1)                                       # one class of heavy ties
    sd, td = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
    res = {"N": N, "C": C, "positives_per_sample": round(float(t[:, 1:].sum(1).mean()), 3), "dense_class_P": int(t[:, 0].sum())}
    ours, torch_ms = [], []
    for _ in range(args.rounds):
        ms, out = _timed(lambda i: ops.rank_metrics(sd, td), 5, 2, torch)
        ours.append(ms)
        ms, ref = _timed(lambda i: _torch_metrics(sd, td, torch), 5, 2, torch)
        torch_ms.append(ms)
    ops.check_device_errors(dev)
    ap, auc, n_pos = (v.cpu().numpy() for v in out)
    res["ms"] = {"rank_metrics": _summary(ours), "torch_sort_cumsum": _summary(torch_ms)}
    res["max_diff_vs_torch"] = [float(np.nanmax(np.abs(ap - ref[0].cpu().numpy()))), float(np.nanmax(np.abs(auc - ref[1].cpu().numpy())))]
    assert max(res["max_diff_vs_torch"]) < 1e-9, res
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        res["ms"]["sklearn_host"] = None
    else:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sh, th = sd.cpu().numpy(), td.cpu().numpy() >= 0.5
        sk_ap = average_precision_score(th, sh, average=None)
        sk_auc = roc_auc_score(th, sh, average=None)
        res["ms"]["sklearn_host"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["max_diff_vs_sklearn"] = [float(np.abs(ap - sk_ap).max()), float(np.abs(auc - sk_auc).max())]
        assert max(res["max_diff_vs_sklearn"]) < 1e-9, res
    res["mAP"], res["mAUC"] = float(np.nanmean(ap)), float(np.nanmean(auc))
    # per kernel, from the library's device-event timers
    from avid_hip import lib
    lib.timing_enable(True)
    for _ in range(3):
        ops.rank_metrics(sd, td)
    torch.cuda.synchronize()
    res["kernels"] = {k: v for k, v in lib.timing_report().items() if k.startswith("rank_")}
    lib.timing_enable(False)
    return res


def bench_loss(args, torch, dev):
    from avid_hip import lib, ops
    V, clips, C = 1900, 10, N_CLASSES
    g = torch.Generator().manual_seed(2)
    x = (3.0 * torch.randn((V * clips, C), generator=g)).to(dev)
    t = (torch.rand((V, C), generator=g) < 2.0 / C).float().to(dev)
    n = V * clips * C
    res = {"V": V, "clips": clips, "C": C, "elements": n}
    for name, gs in (("eval", None), ("train", 1.0)):
        ts = [_timed(lambda i: ops.mlabel_loss(x, t, clips, None, grad_scale=gs), 20, 5, torch)[0] for _ in range(args.rounds)]
        nbytes = 4 * n * (2 if gs is not None else 1) + 4 * V * C * 2
        res[name] = {"ms_per_call": _summary(ts), "bytes": nbytes}
    lib.timing_enable(True)
    for gs in (None, 1.0):
        for _ in range(5):
            ops.mlabel_loss(x, t, clips, None, grad_scale=gs)
    torch.cuda.synchronize()
    res["kernels"] = {k: v for k, v in lib.timing_report().items() if k.startswith("mlabel_")}
    lib.timing_enable(False)
    ops.check_device_errors(dev)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--eval-n", type=int, default=EVAL_N)
    ap.add_argument("--parts", default="step,metric,loss")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mlabel_bench: no GPU")
    dev = torch.device("cuda", 0)
    parts = {"step": bench_step, "metric": bench_metric, "loss": bench_loss}
    unknown = [p for p in args.parts.split(",") if p not in parts]
    if unknown:
        raise SystemExit(f"mlabel_bench: unknown part(s) {unknown}; known: {list(parts)}")
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
