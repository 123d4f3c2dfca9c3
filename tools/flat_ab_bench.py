"""Dev tool: the eight flat optimizer kernels of TWO builds of the library in ONE process, over the same buffers.

Separate processes are no yardstick for a 1 % question: the same library's median moves by 3 % from process to process (where
the buffers land).  Here the other build (``--other``: the libavid_hip.so of another worktree, e.g. the parent commit's) and this
tree's are loaded side by side through ctypes and launched in turns, kernel by kernel, the order rotating from window to window;
the other build is loaded a second time from a copy, and the distance between its two copies is the noise band.  ms per launch by
each library's own HIP-event timers (the launch gaps and the host stay outside); median / min / max of the windows per kernel
over the two-tower model's 21 286 784 elements (momentum SGD with nesterov, the guarded forms clipped).  One JSON line.

    python tools/flat_ab_bench.py --other ../parent/avid-cma_amd/avid_hip/libavid_hip.so [--windows 18] [--rounds 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import shutil
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 21286784
_i, _i64, _f, _vp = C.c_int, C.c_int64, C.c_float, C.c_void_p


class EmaDesc(C.Structure):
    _fields_ = [("ema", C.c_void_p), ("decay", C.c_double), ("warmup", C.c_int), ("updates_dev", C.c_void_p)]


_ADAM, _SGD = [_i64, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f, _i64, _vp, _vp, _f], [_i64, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _f]
SIG = {
    "avid_adam_flat": _ADAM + [_vp], "avid_adam_flat_guarded": _ADAM + [_vp, _vp], "avid_adam_flat_ema": _ADAM + [_vp, C.POINTER(EmaDesc), _vp],
    "avid_sgd_flat": _SGD + [_vp], "avid_sgd_flat_guarded": _SGD + [_vp, _vp], "avid_sgd_flat_ema": _SGD + [_vp, C.POINTER(EmaDesc), _vp],
    "avid_timing_enable": [_i], "avid_timing_report": [C.c_char_p, C.c_size_t],
}


def load(path):
    lib = C.CDLL(path)
    for fn, sig in SIG.items():
        getattr(lib, fn).restype = _i
        getattr(lib, fn).argtypes = sig
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="libavid_hip.so of the build to compare with")
    ap.add_argument("--windows", type=int, default=18)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flat_ab_bench measures on the GPU"
    tmp = tempfile.mkdtemp(prefix="avid_ab_")
    again = os.path.join(tmp, "libavid_hip_again.so")       # the same file under another name is a second library to dlopen
    shutil.copy(a.other, again)
    libs = {"other": load(os.path.abspath(a.other)), "other_again": load(again),
            "this": load(os.path.join(REPO, "avid-cma_amd", "avid_hip", "libavid_hip.so"))}
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)

    def buf(scale):
        return (scale * torch.randn(N, generator=g)).to(dev)
    p, gr, m, v, e = buf(1.0), buf(0.01), buf(0.01), buf(0.01).abs_(), buf(1.0)
    k = torch.zeros((), dtype=torch.int64, device=dev)
    rec = torch.zeros(8, dtype=torch.int32, device=dev)
    rec.view(torch.float32)[1] = 0.37                       # the guard record of a clipped step
    desc = EmaDesc(e.data_ptr(), 0.999, 1, k.data_ptr())
    P, G, M, V, R, D = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), rec.data_ptr(), C.byref(desc)
    A, S = (2e-4, 0.9, 0.999, 1e-8, 1e-5), (1e-3, 0.9, 1e-4, 1, None, 1.0)
    calls = {
        "adam_flat_kernel": lambda L, s: L.avid_adam_flat(N, P, G, M, V, *A, s, None, None, 1.0, None),
        "adam_flat_guarded_kernel": lambda L, s: L.avid_adam_flat_guarded(N, P, G, M, V, *A, s, None, None, 1.0, R, None),
        "adam_flat_ema_kernel": lambda L, s: L.avid_adam_flat_ema(N, P, G, M, V, *A, s, None, None, 1.0, None, D, None),
        "adam_flat_ema_guarded_kernel": lambda L, s: L.avid_adam_flat_ema(N, P, G, M, V, *A, s, None, None, 1.0, R, D, None),
        "sgd_flat_kernel": lambda L, s: L.avid_sgd_flat(N, P, G, M, *S, None),
        "sgd_flat_guarded_kernel": lambda L, s: L.avid_sgd_flat_guarded(N, P, G, M, *S, R, None),
        "sgd_flat_ema_kernel": lambda L, s: L.avid_sgd_flat_ema(N, P, G, M, *S, None, D, None),
        "sgd_flat_ema_guarded_kernel": lambda L, s: L.avid_sgd_flat_ema(N, P, G, M, *S, R, D, None),
    }

    def timed(name, L, step):
        assert L.avid_timing_enable(1) == 0
        for r in range(a.rounds):
            assert calls[name](L, step + r) == 0
        torch.cuda.synchronize()
        out = C.create_string_buffer(1 << 16)
        assert L.avid_timing_report(out, len(out)) == 0
        L.avid_timing_enable(0)
        for line in out.value.decode().splitlines():
            kernel, n, ms, _, _ = line.split(";")
            if kernel == name:
                assert int(n) == a.rounds, line
                return float(ms) / int(n)
        raise KeyError(name)

    try:
        for name in calls:                                      # warm up outside the windows
            for L in libs.values():
                timed(name, L, 1)
        win = {name: {side: [] for side in libs} for name in calls}
        sides = list(libs)
        for w in range(a.windows):
            order = sides[w % 3:] + sides[:w % 3]
            if (w // 3) % 2:
                order = order[::-1]
            for name in calls:
                for side in order:
                    win[name][side].append(timed(name, libs[side], 30 + w * a.rounds))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rec = {"elements": N, "windows": a.windows, "rounds": a.rounds, "other": os.path.abspath(a.other)}
    for name in calls:
        rec[name] = {}
        for side in libs:
            x = sorted(win[name][side])
            rec[name][side] = {"ms": round(x[len(x) // 2], 4), "min": round(x[0], 4), "max": round(x[-1], 4)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
