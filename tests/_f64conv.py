"""Test helpers shared by tests/test_bs64_table.py (host) and tests/test_gpu_bs64_layers.py (GPU).

* A float64 reference of one 3-D convolution — forward, input gradient, weight gradient — by explicit im2col and float64
  matmul over channels-last tensors [B,T,H,W,C].  It calls no avid_hip op (torch only), runs wherever its inputs live, and
  is chunked over clips so that a batch-64 layer never materialises its whole column matrix.
* The convolution geometries of the benchmark's batch-64 step, read from the compiled launch programs (avid_hip/plan.py,
  compiled on the host), with what the step fuses into each: the layer table the batch-64 tests run."""
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_PATH = os.path.join(HERE, "golden", "bs64_conv_layers.json")
BENCH_VIDEO = (64, 3, 8, 112, 112)
BENCH_AUDIO = (64, 1, 40, 100)


# ---- float64 reference ----------------------------------------------------------------------------------------------
def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _cols(xp, k, stride, osz):
    """im2col of a padded chunk [b,Tp,Hp,Wp,C] -> [b*To*Ho*Wo, taps*C], taps in (kt,kh,kw) order, channel fastest."""
    (kt, kh, kw), (st, sh, sw), (To, Ho, Wo) = k, stride, osz
    taps = []
    for a in range(kt):
        for b in range(kh):
            for c in range(kw):
                taps.append(xp[:, a:a + st * (To - 1) + 1:st, b:b + sh * (Ho - 1) + 1:sh, c:c + sw * (Wo - 1) + 1:sw, :])
    return torch.stack(taps, dim=4).reshape(-1, len(taps) * xp.shape[-1])


def _pad(x, pad):
    pt, ph, pw = pad
    return torch.nn.functional.pad(x, (0, 0, pw, pw, ph, ph, pt, pt))


def _wmat(w):
    """[Cout, Cin, kt, kh, kw] -> [Cout, taps*Cin] matching _cols's column order."""
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)


def conv_ref(x, w, stride, pad, dy=None, want=("y", "dx", "dw"), chunk=8, dtype=torch.float64):
    """Float64 y = conv(x, w), dx = d<y, dy>/dx, dw = d<y, dy>/dw for channels-last x [B,T,H,W,Cin] and logical
    w [Cout,Cin,kt,kh,kw] (any float dtype; computed in float64 on x's device).  Returns a dict of the requested
    results, channels-last for y / dx, logical [Cout,Cin,k...] for dw.  (``dtype=torch.float32``: the same contraction in
    plain float32 arithmetic, a yardstick for what fp32 itself makes of a long contraction.)"""
    x = x.to(dtype)
    W = _wmat(w.to(dtype).to(x.device))
    k = tuple(w.shape[2:])
    B, Ti, Hi, Wi, Cin = x.shape
    osz = tuple(out_size(n, kk, s, p) for n, kk, s, p in zip((Ti, Hi, Wi), k, stride, pad))
    out = {}
    if "y" in want:
        out["y"] = torch.empty((B,) + osz + (W.shape[0],), dtype=dtype, device=x.device)
    if "dx" in want:
        out["dx"] = torch.zeros_like(x)
    dW = torch.zeros_like(W) if "dw" in want else None
    for b0 in range(0, B, chunk):
        xs = x[b0:b0 + chunk]
        nb = xs.shape[0]
        if "y" in want or "dw" in want:
            cols = _cols(_pad(xs, pad), k, stride, osz)
            if "y" in want:
                out["y"][b0:b0 + nb] = (cols @ W.t()).reshape((nb,) + osz + (W.shape[0],))
            if dW is not None:
                dW += dy[b0:b0 + nb].to(dtype).to(x.device).reshape(-1, W.shape[0]).t() @ cols
            del cols
        if "dx" in want:
            dcols = (dy[b0:b0 + nb].to(dtype).to(x.device).reshape(-1, W.shape[0]) @ W).reshape((nb,) + osz + (-1, Cin))
            dxp = torch.zeros_like(_pad(xs, pad))                 # col2im: every tap's slice back onto the padded grid
            (kt, kh, kw), (st, sh, sw), (To, Ho, Wo) = k, stride, osz
            j = 0
            for a in range(kt):
                for bb in range(kh):
                    for c in range(kw):
                        dxp[:, a:a + st * (To - 1) + 1:st, bb:bb + sh * (Ho - 1) + 1:sh, c:c + sw * (Wo - 1) + 1:sw, :] += \
                            dcols[:, :, :, :, j, :]
                        j += 1
            pt, ph, pw = pad
            out["dx"][b0:b0 + nb] = dxp[:, pt:pt + Ti, ph:ph + Hi, pw:pw + Wi, :]
    if dW is not None:
        out["dw"] = dW.reshape((W.shape[0],) + k + (Cin,)).permute(0, 4, 1, 2, 3).contiguous()
    return out


# ---- the batch-64 step's layer table --------------------------------------------------------------------------------
def _geom(d):
    return {"Cin": d.Cin, "Cout": d.Cout, "k": [d.kt, d.kh, d.kw], "stride": [d.st, d.sh, d.sw], "pad": [d.pt, d.ph, d.pw],
            "x": [d.B, d.Ti, d.Hi, d.Wi], "channel_first": bool(d.x_channel_first)}


def _key(g):
    return json.dumps([g[n] for n in ("Cin", "Cout", "k", "stride", "pad", "x", "channel_first")])


def trace_bs64_table():
    """Every distinct convolution geometry of the benchmark's batch-64 step (the launch programs of
    models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]) at the benchmark's
    input shapes), each with what the step does with it:
      fwd: list of epilogue forms [addend, bn_stats, bias, relu, in_affine] the forward launches use;
      dgrad: list of forms [bn_bwd_sums, addend, st, sh, sw] — (st, sh, sw): the strides of a compact addend (the gradient
        of the block's strided 1x1x1 residual convolution of the same input), 0 0 0 for a dense one or none;
      wgrad: "own", "grouped" or "in_affine" launches;
    and "groups": the table indices of the items of each grouped weight-gradient launch, in program order."""
    import models
    from avid_hip import plan
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).train()
    pl = plan.Plan(m, BENCH_VIDEO, BENCH_AUDIO, torch.device("cpu"), True, True, True)
    table, index = [], {}

    def entry(d):
        g = _geom(d)
        kk = _key(g)
        if kk not in index:
            index[kk] = len(table)
            table.append(dict(g, fwd=[], dgrad=[], wgrad=[]))
        return index[kk]

    def add(lst, v):
        if v not in lst:
            lst.append(v)
            lst.sort()

    for k in range(pl.n_fwd):
        r = pl.fwd_prog[k]
        if r.op == plan.OP_CONV_FWD:
            e = table[entry(r.d)]
            add(e["fwd"], [int(r.t[3].slot >= 0), int(r.t[6].slot >= 0), int(r.t[4].slot >= 0), int(r.i[0]), int(r.i[1])])
    groups = []
    k = 0
    while k < pl.n_bwd:
        r = pl.bwd_prog[k]
        if r.op == plan.OP_CONV_DGRAD:
            e = table[entry(r.d)]
            add(e["dgrad"], [int(r.i[4]), int(r.t[4].slot >= 0), int(r.i[0]), int(r.i[1]), int(r.i[2])])
        elif r.op == plan.OP_CONV_WGRAD:
            add(table[entry(r.d)]["wgrad"], "in_affine" if r.i[0] else "own")
        elif r.op == plan.OP_WGRAD_GROUP:
            members = []
            for j in range(r.i[0]):
                i = entry(pl.bwd_prog[k + 1 + j].d)
                add(table[i]["wgrad"], "grouped")
                members.append(i)
            groups.append(members)
            k += r.i[0]
        k += 1
    return {"model": 'av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])',
            "video": list(BENCH_VIDEO), "audio": list(BENCH_AUDIO), "layers": table, "groups": groups}


def load_bs64_table():
    with open(TABLE_PATH) as f:
        return json.load(f)


def layer_id(e):
    cf = "_cf" if e["channel_first"] else ""
    return (f"{e['Cin']}to{e['Cout']}_k{''.join(map(str, e['k']))}_s{''.join(map(str, e['stride']))}"
            f"_x{'x'.join(map(str, e['x'][1:]))}{cf}")
