#!/usr/bin/env python
"""Time of the stems' input gradient (stem_dgrad_kernel) on one GPU.  One JSON line:

    python tools/input_grad_bench.py [--iters 10] [--rounds 5] [--shapes 64,3,8,112,112 ...]

For each input shape (default: the pretraining clip batch [64,3,8,112,112], the fine-tuning clip batch [32,3,8,224,224] and
the spectrogram batch [64,1,200,257]) three things alternate in one process (``rounds`` rounds of ``iters`` calls each, HIP
events around each group of calls; medians over the rounds with the min-max spread):
  ``dgrad_ms``       ``avid_conv_dgrad`` of the channel-first stem descriptor: dx from dy and the parameter
  ``forward_ms``     the project's stem forward at the same shape (``ops.conv_cl``: the weight repack / split and the
                     convolution kernel) — the same multiply-adds, on the matrix pipe
  ``torch_ms``       ``torch.nn.grad.conv3d_input`` on the GPU, dy and w in torch's own NCDHW layout (null if it raises)
  ``dgrad_tflops``   2 * B*To*Ho*Wo * 64 * Cin*kt*49 operations over ``dgrad_ms`` (the forward's operation count)
and the ratios ``dgrad_over_forward`` / ``dgrad_over_torch``.  The new kernel's result is checked against torch's on the
first shape's data before anything is timed (max |difference| relative to max |dx|)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEFAULT_SHAPES = ["64,3,8,112,112", "32,3,8,224,224", "64,1,200,257"]
STRIDE = (1, 2, 2)


def timed(fn, iters, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def bench_shape(shape, iters, rounds, torch, lib, ops, dev):
    if len(shape) == 4:
        xs, k, pad = (shape[0], shape[1], 1, shape[2], shape[3]), (1, 7, 7), (0, 3, 3)
    else:
        xs, k, pad = tuple(shape), (3, 7, 7), (1, 3, 3)
    B, cin, Ti, Hi, Wi = xs
    d = ops._desc_cached((B, Ti, Hi, Wi), cin, 64, k, STRIDE, pad, True)[0]
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(xs, device=dev, generator=g)
    dy = torch.randn((B, d.To, d.Ho, d.Wo, 64), device=dev, generator=g)
    w = ops.make_weight(64, cin, *k).to(dev)
    w.copy_(0.05 * torch.randn(w.shape, device=dev, generator=g))
    dx = torch.empty(xs, device=dev)
    dy_t, w_t = dy.permute(0, 4, 1, 2, 3).contiguous(), w.contiguous()

    def dgrad():
        lib.call("avid_conv_dgrad", C.byref(d), ops._p(dy), ops._p(w), None, None, None, None, ops._p(dx), None, None, 0,
                 ops._stream())

    def forward():
        with torch.no_grad():
            ops.conv_cl(x, w, STRIDE, pad, channel_first=True)

    def torch_dgrad():
        return torch.nn.grad.conv3d_input(xs, w_t, dy_t, stride=STRIDE, padding=pad)

    runs = {"dgrad_ms": dgrad, "forward_ms": forward, "torch_ms": torch_dgrad}
    out = {"shape": list(shape)}
    try:
        ref = torch_dgrad()
        dgrad()
        out["max_diff_vs_torch_rel"] = float((dx - ref).abs().max() / ref.abs().max())
        del ref
    except RuntimeError as e:
        out["torch_error"] = str(e)[:200]
        del runs["torch_ms"]
    for fn in runs.values():                      # warm up every path at this shape
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, iters, torch))
    for name, v in times.items():
        out[name] = summary(v)
    out.setdefault("torch_ms", None)
    ms = out["dgrad_ms"]["median"]
    out["dgrad_tflops"] = round(2.0 * B * d.To * d.Ho * d.Wo * 64 * cin * k[0] * 49 / (ms * 1e-3) / 1e12, 2)
    out["dgrad_over_forward"] = round(ms / out["forward_ms"]["median"], 3)
    out["dgrad_over_torch"] = round(ms / out["torch_ms"]["median"], 3) if out["torch_ms"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES, help="B,C,T,H,W (video stem) or B,1,T,F (audio stem)")
    args = ap.parse_args()
    import torch
    from avid_hip import lib, ops
    if not torch.cuda.is_available():
        sys.exit("input_grad_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    res = [bench_shape(tuple(int(v) for v in s.split(",")), args.iters, args.rounds, torch, lib, ops, dev) for s in args.shapes]
    print(json.dumps({"tool": "input_grad_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters,
                      "rounds": args.rounds, "library_version": lib.version(), "results": res}))


if __name__ == "__main__":
    main()
