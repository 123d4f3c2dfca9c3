"""Linear SVM evaluation (csrc/svm.hip, ops.svm_fit) on the GPU: one avid_svm_scores pass and one avid_svm_xt pass against
torch.matmul on the same tensors (X @ W.T, D.T @ X), alternating in one process, and a whole ops.svm_fit with its pass counts:
    python tools/svm_bench.py [--reps 20] [--fit-reps 2] [--shapes 16000x512x50,16000x8192x50,4000x8192x10]
Device events around each call, after warm-up.  Bytes and FLOPs are computed from the shapes (what the algorithm needs: X once,
the small operands once, for xt the partial tiles written and read once); one JSON line per shape."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

HBM_BYTES_S, FP32_MATRIX_FLOPS = 6.3e12, 155e12        # achievable HBM rate, measured fp32 MFMA rate (MI355X)


def _time(fns, reps):
    """Median milliseconds of each function, the functions alternating inside every repetition."""
    times = [[] for _ in fns]
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in times]


def _roof(ms, flops, nbytes):
    t_mem, t_mat = nbytes / HBM_BYTES_S, flops / FP32_MATRIX_FLOPS
    return {"ms": round(ms, 4), "TB_s": round(nbytes / ms / 1e9, 3), "TFLOP_s": round(flops / ms / 1e9, 2),
            "bound": "hbm" if t_mem >= t_mat else "fp32 matrix", "share_of_roof": round(max(t_mem, t_mat) * 1e3 / ms, 3)}


def run(N, F, C, reps, fit_reps):
    from avid_hip import lib, ops
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(N + F + C)
    labels = torch.randint(0, C, (N,), generator=gen, device=dev)
    means = torch.randn((C, F), generator=gen, device=dev) * (0.8 / F ** 0.5)
    X = (means[labels] + torch.randn((N, F), generator=gen, device=dev) / F ** 0.5).contiguous()
    W = torch.randn((C, F), generator=gen, device=dev)
    b = torch.randn(C, generator=gen, device=dev)
    D = torch.randn((N, C), generator=gen, device=dev)
    slices = -(-N // ops.SVM_SLICE_ROWS)
    s_ms, s_ref = _time([lambda: ops.svm_scores(X, W, b), lambda: torch.addmm(b, X, W.t())], reps)
    x_ms, x_ref = _time([lambda: ops.svm_xt(X, D), lambda: (torch.matmul(D.t(), X), D.sum(0))], reps)
    flops = 2.0 * N * F * C
    out = {"shape": [N, F, C],
           "scores": dict(_roof(s_ms, flops, 4.0 * (N * F + C * F + N * C)), torch_ms=round(s_ref, 4)),
           "xt": dict(_roof(x_ms, flops, 4.0 * (N * F + N * C + C * F * (2 * slices + 1))), torch_ms=round(x_ref, 4))}
    if fit_reps < 1:
        return out
    # the whole fit: passes counted at the C ABI
    counts, call = {}, lib.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return call(name, *a)
    lib.call = counting
    try:
        coef, icpt, info = ops.svm_fit(X, labels, C)
    finally:
        lib.call = call
    torch.cuda.synchronize()
    fit_ms = []
    for _ in range(fit_reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.svm_fit(X, labels, C)
        e.record()
        e.synchronize()
        fit_ms.append(a.elapsed_time(e))
    n_s, n_x = counts.get("avid_svm_scores", 0), counts.get("avid_svm_xt", 0)
    out["fit"] = {"ms": round(min(fit_ms), 2), "newton_steps": int(info["iterations"].max()), "converged": bool(info["converged"].all()),
                  "scores_passes": n_s, "xt_passes": n_x, "passes_x_pass_ms": round(n_s * s_ms + n_x * x_ms, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fit-reps", type=int, default=2)
    ap.add_argument("--shapes", default="16000x512x50,16000x8192x50,4000x8192x10")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("svm_bench: no GPU (a timing needs the device)")
    for spec in args.shapes.split(","):
        N, F, C = (int(v) for v in spec.split("x"))
        print(json.dumps(run(N, F, C, args.reps, args.fit_reps)), flush=True)


if __name__ == "__main__":
    main()
