"""Test helpers shared by tests/test_bs64_table.py, tests/test_ft_table.py (host) and tests/test_gpu_bs64_layers.py,
tests/test_gpu_ft_layers.py (GPU).

* A float64 reference of one 3-D convolution — forward, input gradient, weight gradient — by explicit im2col and float64
  matmul over channels-last tensors [B,T,H,W,C].  It calls no avid_hip op (torch only), runs wherever its inputs live, and
  is chunked over clips so that a batch-64 layer never materialises its whole column matrix.
* The convolution geometries of the benchmark's batch-64 step, read from the compiled launch programs (avid_hip/plan.py,
  compiled on the host), with what the step fuses into each: the layer table the batch-64 tests run.  The same trace of the
  fine-tuning programs (plan.ClsPlan) at the two shipped per-GPU clip shapes: the tables tests/test_gpu_ft_layers.py runs.
* A float64 reference of training-mode BatchNorm (+ReLU): forward, backward and the running-statistics update.
* Every other launch of the same programs — BatchNorm, the stem's BatchNorm + max-pool, global max-pool, the heads' ReLU
  backward and bias sums — and the flat Adam buffer with its split: the table tests/test_gpu_bs64_norm.py runs."""
import functools
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_PATH = os.path.join(HERE, "golden", "bs64_conv_layers.json")
NORM_TABLE_PATH = os.path.join(HERE, "golden", "bs64_norm_ops.json")
MODEL = 'av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])'
BENCH_VIDEO = (64, 3, 8, 112, 112)
BENCH_AUDIO = (64, 1, 40, 100)
FT_TABLE_PATH = os.path.join(HERE, "golden", "ft_conv_layers.json")
FT_MODEL = ('ClassificationWrapper(R2Plus1D(18), 101, feat_name="pool", feat_dim=512, pooling_op=None, use_dropout=True, '
            'dropout=0.5)')
# the per-GPU clip shapes of the shipped fine-tuning configs, by the key of their table in the fixture
FT_SHAPES = {"8x8x224": (8, 3, 8, 224, 224), "4x32x224": (4, 3, 32, 224, 224)}


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


@functools.lru_cache(maxsize=1)
def _bs64_plan():
    """The launch programs of the benchmark's batch-64 step, compiled on the host (the same records on any device)."""
    import models
    from avid_hip import plan
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).train()
    return plan.Plan(m, BENCH_VIDEO, BENCH_AUDIO, torch.device("cpu"), True, True, True)


def trace_conv_table(pl):
    """Every distinct convolution geometry of a compiled plan's launch programs, each with what the programs do with it:
      fwd: list of epilogue forms [addend, bn_stats, bias, relu, in_affine] the forward launches use;
      dgrad: list of forms [bn_bwd_sums, addend, st, sh, sw] — (st, sh, sw): the strides of a compact addend (the gradient
        of the block's strided 1x1x1 residual convolution of the same input), 0 0 0 for a dense one or none;
      wgrad: "own", "grouped" or "in_affine" launches;
    and the table indices of the items of each grouped weight-gradient launch, in program order: (layers, groups)."""
    from avid_hip import plan
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
    return table, groups


def trace_bs64_table():
    """The convolution table (trace_conv_table) of the benchmark's batch-64 step: the launch programs of
    models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]) at the benchmark's
    input shapes."""
    table, groups = trace_conv_table(_bs64_plan())
    return {"model": MODEL, "video": list(BENCH_VIDEO), "audio": list(BENCH_AUDIO), "layers": table, "groups": groups}


def load_bs64_table():
    with open(TABLE_PATH) as f:
        return json.load(f)


# ---- the fine-tuning programs' layer tables -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ft_plan(shape):
    """The full-mode launch programs of the shipped fine-tuning configs' wrapper at one per-GPU clip shape, compiled on
    the host."""
    import models
    from avid_hip import plan
    m = models.ClassificationWrapper(models.R2Plus1D(18), 101, feat_name="pool", feat_dim=512, pooling_op=None,
                                     use_dropout=True, dropout=0.5).train()
    return plan.ClsPlan(m, tuple(shape), torch.device("cpu"), True, True, False)


def trace_ft_table(shape):
    """The convolution table (trace_conv_table) of the fine-tuning programs at one of FT_SHAPES' clip shapes."""
    table, groups = trace_conv_table(ft_plan(tuple(shape)))
    return {"model": FT_MODEL, "video": list(shape), "layers": table, "groups": groups}


def load_ft_tables():
    with open(FT_TABLE_PATH) as f:
        return json.load(f)


def layer_id(e):
    cf = "_cf" if e["channel_first"] else ""
    return (f"{e['Cin']}to{e['Cout']}_k{''.join(map(str, e['k']))}_s{''.join(map(str, e['stride']))}"
            f"_x{'x'.join(map(str, e['x'][1:]))}{cf}")


# ---- float64 BatchNorm reference ------------------------------------------------------------------------------------
def bn_ref(x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, relu=False, dy=None, mask=None):
    """Training-mode BatchNorm (+ReLU) over the rows of x [M, C], in float64 on x's device: the forward (mean, biased
    variance, invstd, scale = gamma * invstd, shift = beta - mean * scale, y), the running statistics after one update
    (momentum; unbiased variance M / (M - 1)), and with ``dy`` the backward (dx, dgamma, dbeta).  ``mask``: the ReLU's
    pass pattern to use instead of y > 0 (a device's own, where a pre-activation sits within rounding of 0)."""
    f = lambda t: t.to(torch.float64).to(x.device)                          # noqa: E731
    xd = f(x)
    M = xd.shape[0]
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = f(gamma) * invstd
    shift = f(beta) - mean * scale
    xhat = (xd - mean) * invstd
    y = xhat * f(gamma) + f(beta)
    if relu:
        keep = (y > 0) if mask is None else mask.to(torch.bool).to(x.device)
        y = torch.where(keep, y, torch.zeros_like(y))
    out = {"mean": mean, "var": var, "invstd": invstd, "scale": scale, "shift": shift, "y": y,
           "running_mean": (1 - momentum) * f(running_mean) + momentum * mean,
           "running_var": (1 - momentum) * f(running_var) + momentum * var * (M / (M - 1) if M > 1 else 1.0)}
    if dy is not None:
        dym = f(dy)
        if relu:
            dym = torch.where(keep, dym, torch.zeros_like(dym))
        out["dbeta"] = dym.sum(0)
        out["dgamma"] = (dym * xhat).sum(0)
        out["dx"] = f(gamma) * invstd * (dym - out["dbeta"] / M - xhat * (out["dgamma"] / M))
    return out


# ---- the batch-64 step's other launches -----------------------------------------------------------------------------
def _ref(r):
    return (int(r.slot), int(r.off))


def _conv_form(r):
    """A convolution record's epilogue form, as in trace_bs64_table: forward [addend, bn_stats, bias, relu, in_affine],
    input gradient [bn_bwd_sums, addend, st, sh, sw]."""
    from avid_hip import plan
    if r.op == plan.OP_CONV_FWD:
        return [int(r.t[3].slot >= 0), int(r.t[6].slot >= 0), int(r.t[4].slot >= 0), int(r.i[0]), int(r.i[1])]
    return [int(r.i[4]), int(r.t[4].slot >= 0), int(r.i[0]), int(r.i[1]), int(r.i[2])]


def trace_bs64_norm_table():
    """Every distinct launch of the batch-64 programs that is not a convolution, and the optimizer's flat buffer:
      bn_fwd: M, C, relu, nparts (partial rows handed over by the producing convolution; 0: its own statistics pass),
        y (the normalised tensor is written; false: statistics only, its consumer applies them), running (the running
        statistics are updated), momentum, eps, and "producer": the convolution-table entry and forward form whose epilogue
        wrote the partial rows (the record's t[8] is that convolution's t[6]);
      bn_bwd: M, C, relu, frozen, nparts, "fwd": the bn_fwd entry whose saved state it reads, and "producer": the
        convolution-table entry and input-gradient form whose fused sums are its partial rows (its t[7] is that record's
        t[11]), or null with "dy": "gpool_bwd" when its gradient comes from the global max-pool (nparts 0);
      bn_pool_fwd / bn_pool_bwd: the video stem's BatchNorm + ReLU + max-pool; gpool_fwd / gpool_bwd: B, S, C;
      relu_bwd: n; colsum: M, C;
    each with "count", the number of records it stands for; and "adam": the flat buffer's length and the split of the
    overlapped optimizer step (parallel.TrainStep._optimizer_step_overlapped: [0, early) then [early, n))."""
    from avid_hip import plan
    pl = _bs64_plan()
    conv_index = {_key(e): i for i, e in enumerate(trace_bs64_table()["layers"])}
    fwd = [pl.fwd_prog[k] for k in range(pl.n_fwd)]
    bwd = [pl.bwd_prog[k] for k in range(pl.n_bwd)]
    stats_of = {_ref(r.t[6]): r for r in fwd if r.op == plan.OP_CONV_FWD and r.t[6].slot >= 0}
    sums_of = {_ref(r.t[11]): r for r in bwd if r.op == plan.OP_CONV_DGRAD and r.i[4]}
    table = {k: [] for k in ("bn_fwd", "bn_bwd", "bn_pool_fwd", "bn_pool_bwd", "gpool_fwd", "gpool_bwd", "relu_bwd", "colsum")}

    def add(kind, e):
        lst = table[kind]
        for i, o in enumerate(lst):
            if {k: v for k, v in o.items() if k != "count"} == e:
                o["count"] += 1
                return i
        lst.append(dict(e, count=1))
        return len(lst) - 1

    def producer(conv_rec, key):
        return {"conv": conv_index[_key(_geom(conv_rec.d))], key: _conv_form(conv_rec)}

    bn_fwd_of = {}          # the BatchNorm input's reference -> bn_fwd entry
    for r in fwd:
        if r.op == plan.OP_BN_FWD:
            nparts = int(r.i[2])
            e = {"M": int(r.n[0]), "C": int(r.i[0]), "relu": int(r.i[1]), "nparts": nparts, "y": r.t[5].slot >= 0,
                 "running": r.t[3].slot >= 0, "momentum": round(float(r.f[0]), 6), "eps": round(float(r.f[1]), 9),
                 "producer": producer(stats_of[_ref(r.t[8])], "fwd") if nparts else None}
            bn_fwd_of[_ref(r.t[0])] = add("bn_fwd", e)
        elif r.op == plan.OP_BN_POOL_FWD:
            nparts = int(r.i[5])
            add("bn_pool_fwd", {"B": int(r.i[0]), "T": int(r.i[1]), "H": int(r.i[2]), "W": int(r.i[3]), "C": int(r.i[4]),
                                "nparts": nparts, "running": r.t[3].slot >= 0, "momentum": round(float(r.f[0]), 6),
                                "eps": round(float(r.f[1]), 9),
                                "producer": producer(stats_of[_ref(r.t[9])], "fwd") if nparts else None})
        elif r.op == plan.OP_GPOOL_FWD:
            add("gpool_fwd", {"B": int(r.i[0]), "S": int(r.i[1]), "C": int(r.i[2])})
    gpool_out = {_ref(r.t[2]) for r in bwd if r.op == plan.OP_GPOOL_BWD}
    for r in bwd:
        if r.op == plan.OP_BN_BWD:
            nparts = int(r.i[2])
            e = {"M": int(r.n[0]), "C": int(r.i[0]), "relu": int(r.i[1]), "frozen": int(r.i[3]), "nparts": nparts,
                 "fwd": bn_fwd_of[_ref(r.t[0])], "producer": producer(sums_of[_ref(r.t[7])], "dgrad") if nparts else None}
            if not nparts:
                assert _ref(r.t[1]) in gpool_out, "a BatchNorm backward without partial rows that no global pool feeds"
                e["dy"] = "gpool_bwd"
            add("bn_bwd", e)
        elif r.op == plan.OP_BN_POOL_BWD:
            add("bn_pool_bwd", {"B": int(r.i[0]), "T": int(r.i[1]), "H": int(r.i[2]), "W": int(r.i[3]), "C": int(r.i[4])})
        elif r.op == plan.OP_GPOOL_BWD:
            add("gpool_bwd", {"B": int(r.i[0]), "S": int(r.i[1]), "C": int(r.i[2])})
        elif r.op == plan.OP_RELU_BWD:
            add("relu_bwd", {"n": int(r.n[0])})
        elif r.op == plan.OP_COLSUM:
            add("colsum", {"M": int(r.n[0]), "C": int(r.i[0])})
    return {"model": MODEL, "video": list(BENCH_VIDEO), "audio": list(BENCH_AUDIO), "ops": table,
            "adam": {"n": int(pl.gnumel), "early": int(pl.adam_early)}}


def load_bs64_norm_table():
    with open(NORM_TABLE_PATH) as f:
        return json.load(f)


def norm_id(kind, e):
    if kind in ("bn_fwd", "bn_bwd"):
        tag = f"{kind}_M{e['M']}_C{e['C']}_p{e['nparts']}"
        tag += "" if kind == "bn_bwd" or e["y"] else "_stats_only"
        return tag + (f"_conv{e['producer']['conv']}" if e["producer"] else "_gpool")
    return kind + "_" + "x".join(str(e[k]) for k in ("B", "T", "H", "W", "S", "C", "M", "n") if k in e)
