"""Where the kernels write, and what their results depend on (tests/_guards.py).

Every case runs three times: plain, under ``guarded(0xFF)`` and under ``guarded(0x5A)``.  In the guarded runs every device
allocation of the Python layer has a guard band on both sides and starts out as the fill byte, ``ops.workspace`` hands out
exactly the bytes the size function asked for, a sealed launch program gives each stream exactly what
``avid_program_workspace_bytes`` reports (no 1 MiB floor), and the inputs sit in guarded buffers of their own.  Asserted:

(a) no guard byte changed (an overrun of an output, a partials table, a mask or a workspace; an under-counting size function);
(b) every returned tensor (gradients, running statistics, banks, Adam state, index outputs included) is the same BITS under
    the two fills: every returned byte was written, and nothing read from unwritten scratch, a guard or past an input
    reached a result (0xFF reads as NaN / -1, 0x5A as 1.5e16 / a large positive integer);
(c) they are the plain run's bits, which the float64 tests of the same inputs pin.

The inputs and shapes are those of the float64 tests named at each case: the smallest that reach each kernel path.
No op here is documented as irreproducible between runs, so all comparisons are bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _width_ref as W
from _guards import FILLS, guarded
from oracle import avid_oracle as O
from oracle import detgen

pytestmark = pytest.mark.gpu

# Bytes an op's contract leaves undefined: (case prefix, result name) -> (index expression that IS compared, contract line).
EXCLUSIONS = {
    ("cma_fused", "losses"): (slice(0, 7), "include/avid_hip.h:539 'losses [8]: ... the total, (unused)': losses[7] is never written"),
}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


@functools.lru_cache(maxsize=None)
def gen(kind, tag, shape):
    """Deterministic CPU inputs, made once and shared by the three runs of a case (never modified: callers copy)."""
    return T(getattr(detgen, "det_" + kind)(tag, shape))


def weight(dev, tag, cout, cin, *k):
    from avid_hip import ops
    w = ops.make_weight(cout, cin, *k)
    w.copy_(gen("param", tag, (cout, cin) + tuple(k)))
    return w.to(dev)


CASES = {}


def case(name, backward=False, ws=False, in_place=False):
    """Register ``fn(dev, P) -> {name: tensor}``; ``P`` places an input (identity in the plain run).  ``backward``: the case
    runs an autograd backward (allocations must be seen there); ``ws``: it must have been handed a workspace of non-zero size (a tuple: one below each of these functions of the package); ``in_place``: the op
    allocates nothing, it updates its (placed, guarded) arguments."""
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (fn, backward, ws, in_place)
        return fn
    return deco


# ------------------------------------------------------------------------------------------------------------ convolutions
def _conv(name, cin, cout, k, stride, pad, shp, tag="conv", wino2=False, bn_stats=False, budget=0):
    """``budget``: the CUs the persistent kernels plan for while the case runs (ops.set_cu_budget; set before, restored in
    ``finally``): the guarded runs size every workspace under that budget too, so a size function that plans for another
    budget than the launch shows as a changed guard byte."""
    def fn(dev, P):
        from avid_hip import ops
        B, Ti, Hi, Wi = shp
        To, Ho, Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((Ti, Hi, Wi), pad, k, stride)]
        x = cl(gen("normalish", f"{tag}:{name}:x", (B, cin, Ti, Hi, Wi)))
        gy = cl(gen("uniform", f"{tag}:{name}:gy", (B, cout, To, Ho, Wo)))
        if budget:
            full = torch.cuda.get_device_properties(dev).multi_processor_count
            if budget >= full:
                pytest.skip(f"a budget of {budget} CUs is no reduction on a device of {full}")
        if wino2:
            ops.wino2_configure(0)
        try:
            if budget:
                assert ops.set_cu_budget(budget) == budget
            xd = P(x.to(dev).requires_grad_(True))
            wd = P(weight(dev, f"{tag}:{name}:w.weight", cout, cin, *k).requires_grad_(True))
            out = ops.conv_cl(xd, wd, stride, pad, bn_stats=bn_stats)
            y, part = out if bn_stats else (out, None)
            y.backward(P(gy.to(dev)))
        finally:
            if budget:
                ops.set_cu_budget(0)
            if wino2:
                ops.wino2_configure(-1)
        res = {"y": y, "dx": xd.grad, "dw": wd.grad}
        if bn_stats:
            assert part.numel() > 0
            res["partials"] = part
        return res
    return fn


def _register_convs():
    import test_gpu_ops as G
    import test_gpu_precision as PR
    want = ("spt_s1", "spt_s2_odd", "tmp_s2_odd", "res_s2", "late_small_m", "dead_taps_T1", "dead_taps_T2_s2", "dead_taps_333_T1",
            "big_ragged_333", "wino_128x128_odd", "wino_256x256", "wino_64x64_audio")
    by_name = {c[0]: c for c in G.CONV_CASES}
    for n in want:
        c = by_name[n]
        case(f"conv:{n}", backward=True)(_conv(*c))
        if n in G.WINO_CASES:
            case(f"conv:{n}:wino2", backward=True)(_conv(*c, wino2=True))
    for c in PR.CASES:                       # K-split partials + the reduce
        if c[0] in ("pk_128x128_ksplit", "pk_K4608"):
            case(f"conv:{c[0]}", backward=True, ws=("forward", "backward"))(_conv(*c[:7], tag="prec"))
    for shp in ((2, 3, 9, 11), (5, 7, 45, 47)):
        nm = "x".join(map(str, shp))
        case(f"conv:bn_stats:{nm}", backward=True)(
            _conv(f"bnstats{nm}", 64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), shp, tag="cbp", bn_stats=True))
    # under a reduced CU budget (tests/_budget_ref.py, inputs of tests/test_gpu_cu_budget.py): whole rounds + an unsplit tail,
    # whole rounds + a K-split tail (slabs of the rows >= tail_row0 only), a weight-stationary tail, three column blocks (its
    # input gradient weight-stationary), a Winograd grid of 8 CUs, and the K-split layer with the BatchNorm-statistics epilogue
    import _budget_ref as R
    rows = {R.row_id(r): r for r in R.ROWS}
    for rid, ws, stats in (("s64@24", False, False), ("s64@16", ("forward", "backward"), False), ("s64_small@16", ("forward", "backward"), False),
                           ("s64_192@16", ("backward",), False), ("wino256@8", ("forward", "backward"), False),
                           ("s64@16", ("forward", "backward"), True)):
        layer, budget = rows[rid][:2]
        case(f"conv:budget:{rid}" + (":bn_stats" if stats else ""), backward=True, ws=ws)(
            _conv(layer, *R.LAYERS[layer], tag="budget", bn_stats=stats, budget=budget))


_register_convs()


@case("conv:addend", backward=True)
def _conv_addend(dev, P):
    """test_conv_fused_addend"""
    from avid_hip import ops
    x, r = cl(gen("normalish", "fa:x", (2, 64, 3, 5, 6))), cl(gen("normalish", "fa:r", (2, 64, 3, 5, 6)))
    xd, rd = P(x.to(dev).requires_grad_(True)), P(r.to(dev).requires_grad_(True))
    wd = P(weight(dev, "fa:w.weight", 64, 64, 3, 1, 1).requires_grad_(True))
    y = ops.conv_cl(xd, wd, (1, 1, 1), (1, 0, 0), addend=rd)
    y.backward(P(cl(gen("uniform", "fa:gy", (2, 64, 3, 5, 6))).to(dev)))
    return {"y": y, "dx": xd.grad, "dr": rd.grad, "dw": wd.grad}


@case("conv:bn_backward_partials_from_dgrad", backward=True, ws=True)
def _bn_from_dgrad(dev, P):
    """test_bn_backward_partials_from_dgrad, smallest case, hand-over on, with and without the tap"""
    from avid_hip import ops
    shape, cmid, cout, k, pad, stride = (2, 4, 12, 12), 64, 64, (1, 3, 3), (0, 1, 1), (1, 1, 1)
    B, Ti, Hi, Wi = shape
    res = {}
    for tap in (False, True):
        xx = P(gen("normalish", f"bnb:{shape}:x", (B, Ti, Hi, Wi, 64)).to(dev).requires_grad_(True))
        w1 = P(weight(dev, f"bnb:{cmid}:w1.weight", cmid, 64, 1, 3, 3))
        w2 = P(weight(dev, f"bnb:{cout}:{k}:w2.weight", cout, cmid, *k))
        g_ = P((gen("uniform", f"bnb:{cmid}:g", (cmid,)) + 1.5).to(dev).requires_grad_(True))
        b_ = P(gen("uniform", f"bnb:{cmid}:b", (cmid,)).to(dev).requires_grad_(True))
        rm, rv = P(torch.zeros(cmid).to(dev)), P(torch.ones(cmid).to(dev))
        y1 = ops.conv_cl(xx, w1, (1, 1, 1), (0, 1, 1))
        src = ops.BnSource(None, None, True)
        h = ops.batch_norm_cl(y1, g_, b_, rm, rv, True, relu=True, src=src)
        out = ops.conv_cl(h, w2, stride, pad, tap=tap, bn_src=src)
        y2, alias = (out[0], out[-1]) if tap else (out, None)
        gy = P(gen("uniform", f"bnb:{shape}:{cout}:gy", tuple(y2.shape)).to(dev))
        loss = (y2 * gy).sum()
        if tap:
            loss = loss + (alias * alias).sum() * 0.25
        loss.backward()
        assert src.partials is None
        res.update({f"y2:{tap}": y2, f"dx:{tap}": xx.grad, f"dg:{tap}": g_.grad, f"db:{tap}": b_.grad, f"rm:{tap}": rm, f"rv:{tap}": rv})
    return res


def _grouped(count):
    def fn(dev, P):
        """test_grouped_weight_gradients"""
        import test_gpu_ops as G
        from avid_hip import lib, ops
        layers = G.GROUP_LAYERS[:count]
        items = (lib.WgradItem * count)()
        keep, outs = [], {}
        for i, (cin, cout, k, stride, pad, (B, Ti, Hi, Wi)) in enumerate(layers):
            To, Ho, Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip((Ti, Hi, Wi), pad, k, stride)]
            xd = P(cl(gen("normalish", f"grp:{i}:x", (B, cin, Ti, Hi, Wi))).to(dev))
            gyd = P(cl(gen("uniform", f"grp:{i}:gy", (B, cout, To, Ho, Wo))).to(dev))
            d = ops._desc_cached((B, Ti, Hi, Wi), cin, cout, k, stride, pad, False)[0]
            assert d.groupable
            dw = torch.empty(cout, *k, cin, device=dev).movedim(-1, 1)
            items[i].d = d
            items[i].x, items[i].dy, items[i].dw = xd.data_ptr(), gyd.data_ptr(), dw.data_ptr()
            keep += [xd, gyd]
            outs[f"dw{i}"] = dw
        nb = lib.raw("avid_conv_wgrad_group_workspace_bytes")(count, items)
        ws = ops.workspace(dev, nb)
        lib.call("avid_conv_wgrad_group", count, items, ops._p(ws), ws.numel(), ops._stream())
        torch.cuda.synchronize()
        return outs
    return fn


case("conv:wgrad_group:5", ws=True)(_grouped(5))
case("conv:wgrad_group:1", ws=True)(_grouped(1))


def _affine(kind):
    def fn(dev, P):
        """tests/test_gpu_inference_layers.py, smallest shape (1, 3, 5): the input-side map (forward and weight gradient) and
        the output-side map"""
        import test_gpu_inference_layers as IL
        from avid_hip import ops
        shape = (1, 3, 5)
        B, Hi, Wi = shape
        assert ops.tconv_configure(2) == 2
        try:
            x = P(gen("normalish", f"oaff:{shape}:x", (B, 8, Hi, Wi, 64)).to(dev))
            w = P(IL._weight(f"oaff:{shape}:w", dev, 64, 64, 3, 1, 1))
            bn_in = [P(t) for t in IL._bn(f"oaff:{shape}:in", 64, dev)]
            bn_out = [P(t) for t in IL._bn(f"oaff:{shape}:out", 64, dev)]
            s_in = ops.bn_eval_coeffs([tuple(bn_in) + (1e-5,)])[0]
            s_out = ops.bn_eval_coeffs([tuple(bn_out) + (1e-5,)])[0]
            stride, pad = (1, 1, 1), (1, 0, 0)
            if kind == "in":
                y, part = ops.conv_fwd_in(x, w, stride, pad, s_in[2], s_in[3], relu=True, bn_stats=True)
                dy = P(gen("uniform", f"oaff:{shape}:gy", tuple(y.shape)).to(dev))
                dw = ops.conv_wgrad_in(x, dy, w, stride, pad, s_in[2], s_in[3], relu=True)
                res = {"y": y, "dw": dw, "s4": s_in}
                if part is not None:
                    res["partials"] = part
                return res
            add = P(gen("normalish", f"oaff:{shape}:add", (B, 8, Hi, Wi, 64)).to(dev))
            y0 = ops.conv_fwd_out(x, w, stride, pad, s_out[2], s_out[3], out_relu=True)
            y1 = ops.conv_fwd_out(x, w, stride, pad, s_out[2], s_out[3], out_relu=False, addend=add, in_scale=s_in[2],
                                  in_shift=s_in[3], in_relu=True)
            return {"y0": y0, "y1": y1, "s4": s_out}
        finally:
            ops.tconv_configure(-1)
    return fn


case("conv:in_affine")(_affine("in"))
case("conv:out_affine")(_affine("out"))


# ------------------------------------------------------------------------------------------------------------------- stems
def _stem(shp, pre):
    def fn(dev, P):
        """test_stem_fwd_presplit_patch / test_stem_bn_partials shapes, BatchNorm partials and the weight gradient"""
        from avid_hip import lib, ops
        audio = shp[1] == 1
        cin, k, stride, pad = (1, (1, 7, 7), (1, 2, 2), (0, 3, 3)) if audio else (3, (3, 7, 7), (1, 2, 2), (1, 3, 3))
        To, Ho, Wo = [(n + 2 * p - kk) // s + 1 for n, p, kk, s in zip(shp[2:], pad, k, stride)]
        switch = lib.raw("avid_stem_fwd_pre_configure")
        if pre is not None:
            switch(pre)
        try:
            x = P(gen("normalish", f"stemp:{shp}:x", shp).to(dev))
            wd = P(weight(dev, f"stemp:{shp}:w.weight", 64, cin, *k).requires_grad_(True))
            y, part = ops.conv_cl(x, wd, stride, pad, channel_first=True, bn_stats=True)
            y.backward(P(gen("uniform", f"stemp:{shp}:gy", (shp[0], To, Ho, Wo, 64)).to(dev)))
        finally:
            switch(-1)
        assert part.numel() > 0
        return {"y": y, "partials": part, "dw": wd.grad}
    return fn


for _shp in ((2, 3, 4, 24, 28), (5, 3, 2, 38, 44), (1, 3, 1, 112, 112)):
    for _pre in (1, 0):
        case(f"stem:video:{'x'.join(map(str, _shp))}:pre{_pre}", backward=True)(_stem(_shp, _pre))
case("stem:audio:3x1x1x40x100", backward=True)(_stem((3, 1, 1, 40, 100), None))


# ------------------------------------------------------------------------------------------- BatchNorm, pooling and linear
def _bn_train(M, Cc, relu):
    def fn(dev, P):
        """test_batchnorm_train"""
        from avid_hip import ops
        x = gen("normalish", f"bn:{M}:{Cc}:x", (M, Cc)) * 1.7 + 0.3
        xd = P(x.to(dev).requires_grad_(True))
        gd = P(gen("param", f"bn:{M}:{Cc}:bn.weight", (Cc,)).to(dev).requires_grad_(True))
        bd = P(gen("param", f"bn:{M}:{Cc}:bn.bias", (Cc,)).to(dev).requires_grad_(True))
        rm = P(gen("param", f"bn:{M}:{Cc}:bn.running_mean", (Cc,)).to(dev))
        rv = P(gen("param", f"bn:{M}:{Cc}:bn.running_var", (Cc,)).to(dev))
        cnt = P(torch.zeros((), dtype=torch.int64).to(dev))
        y = ops.batch_norm_cl(xd.view(1, 1, 1, M, Cc), gd, bd, rm, rv, True, 0.1, 1e-5, relu, cnt)
        y.backward(P(gen("uniform", f"bn:{M}:{Cc}:gy", (M, Cc)).to(dev)).view(1, 1, 1, M, Cc))
        return {"y": y, "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "running_mean": rm, "running_var": rv, "count": cnt}
    return fn


for _M, _C in ((2, 64), (777, 128), (40, 512), (140000, 64)):
    for _relu in (False, True):
        case(f"bn:train:{_M}x{_C}:{'relu' if _relu else 'plain'}", backward=True, ws=True)(_bn_train(_M, _C, _relu))


@case("bn:eval:500x128")
def _bn_eval(dev, P):
    """test_batchnorm_eval"""
    from avid_hip import ops
    M, Cc = 500, 128
    args = [P(gen(kind, f"bne:{n}", shape).to(dev)) for kind, n, shape in (
        ("normalish", "x", (M, Cc)), ("param", "bn.weight", (Cc,)), ("param", "bn.bias", (Cc,)),
        ("param", "bn.running_mean", (Cc,)), ("param", "bn.running_var", (Cc,)))]
    with torch.no_grad():
        y = ops.batch_norm_cl(args[0].view(1, 1, 1, M, Cc), *args[1:], False, 0.1, 1e-5, True)
    return {"y": y, "running_mean": args[3], "running_var": args[4]}


def _bn_pool(shape):
    def fn(dev, P):
        """test_bn_relu_maxpool_fused"""
        from avid_hip import ops
        Cc = shape[-1]
        xx = P(gen("normalish", f"bnpool:{shape}:x", shape).to(dev).requires_grad_(True))
        gg = P((gen("uniform", f"bnpool:{shape}:g", (Cc,)) + 1.5).to(dev).requires_grad_(True))
        bb = P(gen("uniform", f"bnpool:{shape}:b", (Cc,)).to(dev).requires_grad_(True))
        rm, rv = P(torch.zeros(Cc).to(dev)), P(torch.ones(Cc).to(dev))
        cnt = P(torch.zeros((), dtype=torch.int64).to(dev))
        y = ops.bn_relu_maxpool(xx, gg, bb, rm, rv, 0.1, 1e-5, cnt)
        gy = P(gen("uniform", f"bnpool:{shape}:gy", tuple(y.shape)).to(dev))
        (y * gy).sum().backward()
        return {"y": y, "dx": xx.grad, "dgamma": gg.grad, "dbeta": bb.grad, "running_mean": rm, "running_var": rv, "count": cnt}
    return fn


case("pool:bn_relu_maxpool:1x2x7x9x64", backward=True, ws=True)(_bn_pool((1, 2, 7, 9, 64)))
case("pool:bn_relu_maxpool:2x3x10x12x64", backward=True, ws=True)(_bn_pool((2, 3, 10, 12, 64)))


@case("pool:maxpool_hw3s2:1x64x2x7x9", backward=True)
def _maxpool(dev, P):
    """test_maxpool_hw3s2"""
    from avid_hip import ops
    shp = (1, 64, 2, 7, 9)
    xd = P(cl(F.relu(gen("normalish", f"mp:{shp}:x", shp))).to(dev).requires_grad_(True))
    y = ops.maxpool_hw3s2(xd)
    y.backward(P(gen("uniform", f"mp:{shp}:gcl", tuple(y.shape)).to(dev)))
    return {"y": y, "dx": xd.grad}


@case("pool:global_maxpool:2x512x1x3x7", backward=True)
def _global_maxpool(dev, P):
    """test_global_maxpool"""
    from avid_hip import ops
    shp = (2, 512, 1, 3, 7)
    xd = P(cl(F.relu(gen("normalish", f"gp:{shp}:x", shp))).to(dev).requires_grad_(True))
    y = ops.global_maxpool(xd)
    y.backward(P(gen("uniform", f"gp:{shp}:g", (2, 512)).to(dev)))
    return {"y": y, "dx": xd.grad}


def _linear(B, cin, cout, relu):
    def fn(dev, P):
        """test_linear_bias_relu"""
        from avid_hip import ops
        xd = P(gen("normalish", f"lin:{B}:x", (B, cin)).to(dev).requires_grad_(True))
        wd = P(gen("param", f"lin:{B}:w.weight", (cout, cin)).to(dev).requires_grad_(True))
        bd = P(gen("param", f"lin:{B}:w.bias", (cout,)).to(dev).requires_grad_(True))
        y = ops.linear(xd, wd, bd, relu)
        y.backward(P(gen("uniform", f"lin:{B}:g", (B, cout)).to(dev)))
        return {"y": y, "dx": xd.grad, "dw": wd.grad, "db": bd.grad}
    return fn


case("linear:5x512x128", backward=True)(_linear(5, 512, 128, False))
case("linear:4x512x512:relu", backward=True)(_linear(4, 512, 512, True))


# ------------------------------------------------------------------------------------------------- criterion and optimiser
def _l2norm(bs, D):
    def fn(dev, P):
        """test_l2norm (with its zero row)"""
        from avid_hip import ops
        x = (gen("normalish", f"l2:{bs}:{D}:x", (bs, D)) * 3).clone()
        x[3] = 0
        xd = P(x.to(dev).requires_grad_(True))
        y = ops.l2_normalize(xd)
        y.backward(P(gen("uniform", f"l2:{bs}:{D}:g", (bs, D)).to(dev)))
        return {"y": y, "dx": xd.grad}
    return fn


case("crit:l2_normalize:7x128", backward=True)(_l2norm(7, 128))
case("crit:l2_normalize:5x512", backward=True)(_l2norm(5, 512))
case("crit:l2norm:D1000", backward=True)(_l2norm(5, 1000))       # 16 trips, the last one ragged (40 of 64 lanes)


@case("crit:bank_scores+mean_exp", backward=True)
def _bank_scores(dev, P):
    """test_bank_scores_and_backward; mean_exp of the scores and of a column slice"""
    from avid_hip import ops
    N, bs, R = 5000, 6, 1025
    bank = P(F.normalize(gen("normalish", "bs:bank", (N, 128)), dim=1).to(dev))
    ed = P(F.normalize(gen("normalish", "bs:emb", (bs, 128)), dim=1).to(dev).requires_grad_(True))
    idx = P(T(detgen.det_indices("bs:idx", bs * R, N)).view(bs, R).to(dev))
    s = ops.bank_scores(ed, bank, idx, 1 / 0.07)
    z0, z1 = ops.mean_exp(s.detach() * 0.1), ops.mean_exp((s.detach() * 0.1)[:, 1:])
    s.backward(P(gen("uniform", "bs:g", (bs, R)).to(dev)))
    return {"s": s, "demb": ed.grad, "mean_exp": z0, "mean_exp_sliced": z1}


def _bank_scores_width(D):
    def fn(dev, P):
        """test_bank_scores_widths at (3, 65): one row past a 64-row block; the snapshot [3, 65, D] is guarded at pitch D"""
        from avid_hip import ops
        bank, emb, idx, ds = W.score_inputs(D, 3, 65)
        bank_d, idx_d = P(bank.to(dev)), P(idx.to(dev))
        ed = P(emb.to(dev).requires_grad_(True))
        s = ops.bank_scores(ed, bank_d, idx_d, W.INV_T)
        s.backward(P(ds.to(dev)))
        ops.check_device_errors(dev)
        return {"s": s, "demb": ed.grad}
    return fn


case("crit:bank_scores:D64", backward=True)(_bank_scores_width(64))
case("crit:bank_scores:D512", backward=True)(_bank_scores_width(512))


def _nce(bs, Pn, K, joint=False):
    def fn(dev, P):
        """test_nce_multi_block_path / test_nce_joint_score_tensor_path"""
        from avid_hip import ops
        g = torch.Generator().manual_seed(bs + Pn + K)
        base = torch.rand(bs, Pn + K, generator=g) * 12 - 6
        Z = P(torch.tensor(0.37).to(dev))
        if joint:
            s = P(base.to(dev).requires_grad_(True))
            pos, neg = ops.split_scores(s * 1.0, Pn)
            loss = ops.nce_loss(pos, neg, Z)
            assert type(loss.grad_fn).__name__.startswith("_NCELossJoint")
            (loss * 0.5).backward()
            return {"loss": loss, "ds": s.grad}
        sp = P(base[:, :Pn].contiguous().to(dev).requires_grad_(True))
        sn = P(base[:, Pn:].contiguous().to(dev).requires_grad_(True))
        loss = ops.nce_loss(sp, sn, Z)
        loss2 = ops.nce_loss(sp, sn, Z)               # the re-armed ticket
        loss2.backward()
        return {"loss": loss, "loss2": loss2, "dpos": sp.grad, "dneg": sn.grad}
    return fn


case("crit:nce:4x1x64", backward=True)(_nce(4, 1, 64))
case("crit:nce:64x32x1000", backward=True)(_nce(64, 32, 1000))
case("crit:nce_joint:16x32x64", backward=True)(_nce(16, 32, 64, joint=True))


@case("crit:bank_update")
def _bank_update(dev, P):
    """test_bank_update: duplicate ids, the last occurrence wins; and both banks in one launch"""
    from avid_hip import ops
    N, B = 3000, 40
    bank = F.normalize(gen("normalish", "bu:bank", (N, 128)), dim=1)
    emb = P(F.normalize(gen("normalish", "bu:emb", (B, 128)), dim=1).to(dev))
    emb2 = P(F.normalize(gen("normalish", "bu:emb2", (B, 128)), dim=1).to(dev))
    y = T(detgen.det_indices("bu:y", B, N)).clone()
    y[7] = y[3]
    y[30] = y[3]
    yd = P(y.to(dev))
    b1, b2, p1, p2 = (P(bank.to(dev)) for _ in range(4))
    ops.bank_update(b1, yd, emb, 0.5)
    ops.bank_update(b2, yd, emb, 0.9)
    ops.bank_update_pair(p1, p2, yd, emb, emb2, 0.5, 0.9)
    ops.check_device_errors(dev)
    return {"b1": b1, "b2": b2, "p1": p1, "p2": p2}


def _bank_update_width(D):
    def fn(dev, P):
        """test_bank_update_widths at B = 5 (ragged against 4 samples per block, a triple duplicate): in place, single and pair"""
        from avid_hip import ops
        bank, emb0, emb1, y = W.update_inputs(D, 5)
        e0, e1, yd = P(emb0.to(dev)), P(emb1.to(dev)), P(y.to(dev))
        b0, b1, p0, p1 = (P(bank.to(dev)) for _ in range(4))
        ops.bank_update(b0, yd, e0, 0.5)
        ops.bank_update(b1, yd, e1, 0.9)
        ops.bank_update_pair(p0, p1, yd, e0, e1, 0.5, 0.9)
        ops.check_device_errors(dev)
        return {"b0": b0, "b1": b1, "p0": p0, "p1": p1}
    return fn


case("crit:bank_update:D100")(_bank_update_width(100))
case("crit:bank_update:D512")(_bank_update_width(512))


def _fused_inputs(bs, K, N, P_=None):
    gen_ = torch.Generator().manual_seed(bs * 1000 + K + (P_ or 0))
    v1 = F.normalize(torch.randn(N, 128, generator=gen_), dim=1)
    v2 = F.normalize(torch.randn(N, 128, generator=gen_), dim=1)
    ve, ae = torch.randn(bs, 128, generator=gen_) * 2, torch.randn(bs, 128, generator=gen_) * 0.5
    y = torch.randperm(N, generator=gen_)[:bs]
    return gen_, v1, v2, ve, ae, y


def _xmodal(bs, K, N):
    def fn(dev, P):
        """test_xmodal_fused_vs_unfused_ops_and_fp64 (the backward only scales the gradient the forward stored: it allocates
        through no factory function, so no allocation count is asked of it)"""
        from avid_hip import ops
        g, v1, v2, ve, ae, y = _fused_inputs(bs, K, N)
        idx = torch.randint(0, N - 1, (bs, K), generator=g)
        idx = idx + (idx >= y[:, None]).long()
        b1, b2 = P(v1.to(dev)), P(v2.to(dev))
        vd, ad = P(ve.to(dev).requires_grad_(True)), P(ae.to(dev).requires_grad_(True))
        ws = ops.xmodal_fused_workspace(dev, bs, K)
        yd, idd, Z = P(y.to(dev)), P(idx.to(dev)), P(torch.tensor(0.83).to(dev))
        first = ops.xmodal_fused(vd, ad, yd, idd, b1, b2, Z, 1 / 0.07, 0.75, ws)
        total, losses, hats = ops.xmodal_fused(vd, ad, yd, idd, b1, b2, Z, 1 / 0.07, 0.75, ws)      # re-armed tickets
        (total * 2.0).backward()
        ops.check_device_errors(dev)
        return {"total0": first[0], "total": total, "losses": losses, "hats": hats, "dv": vd.grad, "da": ad.grad}
    return fn


case("crit:xmodal_fused:3x70x300")(_xmodal(3, 70, 300))
case("crit:xmodal_fused:6x1024x5000")(_xmodal(6, 1024, 5000))


def _cma(bs, Pn, K, Kw, N):
    def fn(dev, P):
        """test_cma_fused_vs_fp64_and_the_criterion_it_replaces"""
        from avid_hip import ops
        g, v1, v2, ve, ae, y = _fused_inputs(bs, K, N, Pn)
        pos = torch.randint(0, N, (bs, Pn), generator=g)
        idx = torch.randint(0, N, (bs, K), generator=g)
        b1, b2 = P(v1.to(dev)), P(v2.to(dev))
        vd, ad = P(ve.to(dev).requires_grad_(True)), P(ae.to(dev).requires_grad_(True))
        ws = ops.cma_fused_workspace(dev, bs, Pn, K)
        args = (P(y.to(dev)), P(pos.to(dev)), P(idx.to(dev)), b1, b2, P(torch.tensor(0.83).to(dev)), 1 / 0.07, Kw, 0.4, 0.6, ws)
        first = ops.cma_fused(vd, ad, *args)
        total, losses, hats = ops.cma_fused(vd, ad, *args)
        (total * 2.0).backward()
        ops.check_device_errors(dev)
        return {"total0": first[0], "total": total, "losses": losses, "hats": hats, "dv": vd.grad, "da": ad.grad}
    return fn


case("cma_fused:4x1x33x7x200")(_cma(4, 1, 33, 7, 200))
case("cma_fused:6x32x1024x64x5000")(_cma(6, 32, 1024, 64, 5000))


@functools.lru_cache(maxsize=None)
def _golden(name):
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False))


@case("crit:cma_negatives")
def _cma_negatives(dev, P):
    """test_cma_negatives_bit_exact"""
    from avid_hip import ops
    g = _golden("cma")
    pos, neg = ops.cma_negatives(P(T(g["topk_consensus"]).int().to(dev)), P(T(g["ms_y"]).to(dev)), P(T(g["ms_rand"]).to(dev)))
    ops.check_device_errors(dev)
    return {"pos": pos, "neg": neg}


@case("crit:alias_draw")
def _alias(dev, P):
    """test_alias_draw_bit_exact: the 50-entry table, and the fused avoid-self form (per_row) on it"""
    from avid_hip import ops
    prob, alias = O.alias_build(np.abs(detgen.det_uniform("alias:det50", (50,))) + 0.01)
    pd, ad = P(T(prob).to(dev)), P(T(alias).to(dev))
    a = ops.alias_draw(30000, len(prob), pd, ad, False, 2 ** 40 + 5, 2 ** 33, device=dev)
    y = P(T(detgen.det_indices("alias:y50", 30, 51)).to(dev))
    off = P(torch.full((), 11, dtype=torch.int64).to(dev))
    b = ops.alias_draw(30 * 1000, len(prob), pd, ad, False, 5, 0, y=y, per_row=1000, offset_dev=off)
    return {"draw": a, "draw_per_row": b, "offset": off}


def _adam(n):
    def fn(dev, P):
        """test_adam_flat: by-value step, and the device-resident step counter and learning rate"""
        from avid_hip import ops
        p0 = gen("normalish", f"adam:{n}:p", (n,))
        pd, pd2 = P(p0.to(dev)), P(p0.to(dev))
        m, v, m2, v2 = (P(torch.zeros(n).to(dev)) for _ in range(4))
        t_dev = P(torch.zeros((), dtype=torch.int64).to(dev))
        lr_dev = P(torch.full((), 2e-4, dtype=torch.float32).to(dev))
        for step in (1, 2):
            g = P(gen("normalish", f"adam:{n}:g{step}", (n,)).to(dev))
            ops.adam_flat(pd, g, m, v, 2e-4, 0.9, 0.999, 1e-8, 1e-5, step)
            ops.adam_flat(pd2, g, m2, v2, 0.0, 0.9, 0.999, 1e-8, 1e-5, 0, step_dev=t_dev, lr_dev=lr_dev)
        return {"p": pd, "m": m, "v": v, "p_dev": pd2, "m_dev": m2, "v_dev": v2, "t": t_dev, "lr": lr_dev}
    return fn


case("optim:adam_flat:5", in_place=True)(_adam(5))
case("optim:adam_flat:100003", in_place=True)(_adam(100003))


# ------------------------------------------------------------------------------------------------------------------ search
@case("search:cma_topk:scan_500", ws=True)
def _topk_scan(dev, P):
    """test_cma_topk_vs_reference_golden: the 500-row banks (exact scan), all four kinds, a sharded range"""
    import test_gpu_model as GM
    from avid_hip import topk
    v1, v2 = P(GM.det_bank("cma:v1", 500).to(dev)), P(GM.det_bank("cma:v2", 500).to(dev))
    res = {f"kind{k}": topk.cma_topk(v1, v2, 0, 500, 32, k, batch=128) for k in range(4)}
    res["shard"] = topk.cma_topk(v1, v2, 250, 500, 32, 0, batch=64)
    return res


@case("search:cma_topk:filter_6000", ws=True)
def _topk_filter(dev, P):
    """test_cma_topk_filter_path_vs_oracle"""
    from avid_hip import topk
    N = 6000
    g = torch.Generator().manual_seed(11)
    v1 = F.normalize(torch.randn(N, 128, generator=g), dim=1)
    v2 = F.normalize(torch.randn(N, 128, generator=g), dim=1)
    d1, d2 = P(v1.to(dev)), P(v2.to(dev))
    fb = P(torch.zeros((), dtype=torch.int32).to(dev))
    res = {f"kind{k}": topk.cma_topk(d1, d2, 0, N, 32, k, batch=1024, fallbacks=fb) for k in range(4)}
    res["shard"] = topk.cma_topk(d1, d2, 2500, N, 32, 0, batch=256)
    res["fallbacks"] = fb
    return res


def _knn(N, Q, k, excl, batch=128, nq=None, overflow=False):
    def fn(dev, P):
        """tests/test_gpu_knn.py: lattice features (every score exact, ties abound)"""
        import test_gpu_knn as KN
        from avid_hip import ops
        if overflow:
            rng = np.random.default_rng(7)
            g = rng.integers(-4, 5, (N, 32)).astype(np.float32) / 8
            dup = np.sort(rng.permutation(N)[:1500])
            g[dup] = 0.5
            q = rng.integers(1, 5, (Q, 32)).astype(np.float32) / 8
            ex = np.where(np.arange(Q) % 2 == 0, dup[np.arange(Q) % 7], -1).astype(np.int32)
        else:
            g, q, ex = KN._lattice(N, Q)
        if nq is not None:
            q, ex = q[:nq], ex[:nq]
        fb = P(torch.zeros((), dtype=torch.int32).to(dev))
        idx, sim = ops.knn_search(P(T(g).to(dev)), P(T(q).contiguous().to(dev)), k,
                                  exclude=P(T(ex).contiguous().to(dev)) if excl else None, batch=batch, fallbacks=fb)
        return {"idx": idx, "sim": sim, "fallbacks": fb}
    return fn


case("search:knn:200x70:k20:exclude", ws=True)(_knn(200, 70, 20, True))
case("search:knn:4133x130:k63:batch64", ws=True)(_knn(4133, 130, 63, False, batch=64))
case("search:knn:4133x130:k63:batch128", ws=True)(_knn(4133, 130, 63, False, batch=128))
case("search:knn:4133x130:k20:exclude:batch128", ws=True)(_knn(4133, 130, 20, True, batch=128))
case("search:knn:4133:5_queries_padded", ws=True)(_knn(4133, 130, 20, True, nq=5))
case("search:knn:overflow_4160x130", ws=True)(_knn(4160, 130, 20, True, overflow=True))


@case("search:knn_vote:101x20")
def _vote(dev, P):
    """test_vote_matches_the_restatement"""
    import test_gpu_knn as KN
    from avid_hip import ops
    g, q, _ = KN._lattice(4133, 130)
    idx, sim = ops.knn_search(P(T(g).to(dev)), P(T(q).to(dev)), 20)
    rng = np.random.default_rng(101)
    gl = P(T(rng.integers(0, 101, 4133).astype(np.int32)).to(dev))
    ql = P(T(rng.integers(0, 101, 130).astype(np.int32)).to(dev))
    scores, pred5, first = ops.knn_vote(P(idx), P(sim), gl, 101, T=0.07, query_labels=ql)
    s2, p2, _ = ops.knn_vote(P(idx), P(sim), gl, 101, T=0.07)
    return {"scores": scores, "pred5": pred5, "first": first, "scores_nolabels": s2, "pred5_nolabels": p2}


# ------------------------------------------------------------------------------------------------------------------- heads
@case("head:cls_linear:1x51x512", backward=True)
def _cls_linear(dev, P):
    """test_cls_linear_against_float64, smallest of LINEAR_CASES"""
    from avid_hip import ops
    B, Cn, Fin = 1, 51, 512
    g = torch.Generator().manual_seed(B * 100000 + Cn * 100 + Fin % 100)
    x = torch.randn(B, Fin, generator=g).abs() * (torch.rand(B, Fin, generator=g) > 0.5) * 2
    w = (torch.rand(Cn, Fin, generator=g) * 2 - 1) * Fin ** -0.5
    b = (torch.rand(Cn, generator=g) * 2 - 1) * Fin ** -0.5
    xd, wd, bd = (P(t.to(dev).requires_grad_(True)) for t in (x, w, b))
    y = ops.cls_linear(xd, wd, bd)
    y.backward(P(torch.randn(B, Cn, generator=g).to(dev)))
    return {"y": y, "dx": xd.grad, "dw": wd.grad, "db": bd.grad}


@case("head:cls_loss:4x101:2clips")
def _cls_loss(dev, P):
    """test_cls_loss_against_float64"""
    from avid_hip import ops
    g = torch.Generator().manual_seed(4 * 1000 + 101)
    logits = P((3 * torch.randn(4, 101, generator=g)).to(dev))
    labels = P(torch.randint(0, 101, (2,), generator=g).to(dev))
    loss, conf, hits, dl = ops.cls_loss(logits, labels, 2, grad_scale=1.0)
    ops.check_device_errors(dev)
    return {"loss": loss, "conf": conf, "hits": hits, "dlogits": dl}


def _dropout(shape):
    def fn(dev, P):
        """tests/test_gpu_finetune.py dropout: (4, 512), and an element count with n mod 4 = 3 (the vector tail)"""
        from avid_hip import ops
        g = torch.Generator().manual_seed(shape[0] * shape[1])
        xd = P(torch.randn(shape, generator=g).to(dev).requires_grad_(True))
        y = ops.dropout(xd, 0.5, 0xC1A5, 3)
        y.backward(P(torch.randn(shape, generator=g).to(dev)))
        return {"y": y, "dx": xd.grad, "mask": ops.dropout_mask(shape[0], shape[1], 0.5, 0xC1A5, 3, dev)}
    return fn


case("head:dropout:4x512", backward=True)(_dropout((4, 512)))
case("head:dropout:3x5_tail", backward=True)(_dropout((3, 5)))


@case("head:adaptive_maxpool:5x3x7x9->2x3x4")
def _adaptive(dev, P):
    """test_adaptive_maxpool_equals_torch, smallest of POOL_CASES"""
    from avid_hip import ops
    g = torch.Generator().manual_seed(5 + 7)
    return {"y": ops.adaptive_maxpool(P(torch.randn((3, 3, 7, 9, 5), generator=g).to(dev)), (2, 3, 4))}


def _bn1d(B, Fd):
    def fn(dev, P):
        """test_bn1d_against_float64"""
        from avid_hip import ops
        g = torch.Generator().manual_seed(B * 7 + Fd)
        x = torch.randn((B, Fd), generator=g).abs() * 1.3 + 0.2
        gy = torch.randn((B, Fd), generator=g)
        gamma, beta = torch.rand(Fd, generator=g) + 0.5, torch.randn(Fd, generator=g) * 0.3
        rm0, rv0 = torch.randn(Fd, generator=g) * 0.1, torch.rand(Fd, generator=g) + 0.5
        xd = P(x.to(dev).requires_grad_(True))
        gd, bd = P(gamma.to(dev).requires_grad_(True)), P(beta.to(dev).requires_grad_(True))
        rm, rv, cnt = P(rm0.to(dev)), P(rv0.to(dev)), P(torch.tensor(3, dtype=torch.int64).to(dev))
        y = ops.bn1d(xd, gd, bd, rm, rv, True, 0.1, 1e-5, cnt)
        y.backward(P(gy.to(dev)))
        xe = P(x.to(dev).requires_grad_(True))
        ye = ops.bn1d(xe, gd.detach(), bd.detach(), rm, rv, False, 0.1, 1e-5)
        ye.backward(P(gy.to(dev)))
        return {"y": y, "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "running_mean": rm, "running_var": rv, "count": cnt,
                "y_eval": ye, "dx_eval": xe.grad}
    return fn


case("head:bn1d:2x4", backward=True)(_bn1d(2, 4))
case("head:bn1d:5x100", backward=True)(_bn1d(5, 100))


@case("head:probe_linear:3x100x7", backward=True)
def _probe_linear(dev, P):
    """test_probe_linear_against_float64"""
    from avid_hip import ops
    B, Fin, Cn = 3, 100, 7
    g = torch.Generator().manual_seed(B + Fin + Cn)
    x, gy = torch.randn((B, Fin), generator=g), torch.randn((B, Cn), generator=g)
    w = (torch.rand((Cn, Fin), generator=g) * 2 - 1) / Fin ** 0.5
    b = (torch.rand(Cn, generator=g) * 2 - 1) / Fin ** 0.5
    xd, wd, bd = (P(t.to(dev).requires_grad_(True)) for t in (x, w, b))
    y = ops.probe_linear(xd, wd, bd)
    y.backward(P(gy.to(dev)))
    return {"y": y, "dx": xd.grad, "dw": wd.grad, "db": bd.grad}


# -------------------------------------------------------------------------------------------------------------- front ends
@case("front:clip_normalize:1x1x1x4")
def _clip_normalize(dev, P):
    """tests/test_clip_prep.py, smallest case"""
    from avid_hip import ops
    frames = torch.randint(0, 256, (1, 1, 1, 4, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    return {"out": ops.clip_normalize(P(frames.to(dev)))}


@case("front:clip_augment:28x36", ws=True)
def _clip_augment(dev, P):
    """test_ragged_batch_frame_mapping_and_flip: a clip with a contrast operation (the per-frame grey sums in the workspace)
    and one with no colour operation, output 28 x 36 (no multiple of the 8 x 32 tile)"""
    import test_gpu_augment as GA
    from avid_hip import ops
    clips = [GA.frames(2, 3, 48, 64), GA.frames(5, 2, 24, 31)]
    params = [GA.P((4, 6, 40, 50), (28, 36), flip=True, ops=[(GA.B, 1.2), (GA.C, 0.8)]), GA.P((1, 1, 20, 29), (28, 36))]
    res = {"both": ops.clip_augment([P(T(c).to(dev)) for c in clips], params, 5, (28, 36))}
    res["plain_only"] = ops.clip_augment([P(T(clips[1]).to(dev))], params[1:], 2, (28, 36))
    return res


@case("front:log_spectrogram:256", ws=True)
def _logspec(dev, P):
    """test_logspec_vs_oracle, config (256, 0.005, 24000 samples): B 3, normalised"""
    import test_logspec as LS
    from avid_hip import ops
    n_fft, hop, nsamp = 256, 120, 24000
    rng = np.random.default_rng(5)
    Fb = n_fft // 2 + 1
    mean = P(T(rng.uniform(-30, -10, Fb).astype(np.float32)).to(dev))
    std = P(T(rng.uniform(5, 15, Fb).astype(np.float32)).to(dev))
    sig = np.stack([np.asarray(LS._signal(10 + i, nsamp, "noise"), dtype=np.float32).reshape(-1) for i in range(3)])
    out = ops.log_spectrogram(P(T(sig).to(dev)), 2 * n_fft, hop, 1 + nsamp // hop, mean, std, top_db=100.)
    return {"spect": out}


# -------------------------------------------------------------------------------------------------------- compiled programs
def _buffers(m):
    return {f"buffer:{n}": b for n, b in m.named_buffers()}


@case("program:trainstep")
def _trainstep(dev, P):
    """tests/test_gpu_engine.py _make / _data: bs 4, video 3x8x64x64, audio 1x40x100, N 5000, K 256.  Two steps: the second
    one runs the fused criterion (Z is frozen by the first)."""
    import test_gpu_engine as E
    video, audio, ids = E._data(dev, steps=2)
    m, crit, eng = E._make(dev)
    video, audio = P(video), P(audio)
    losses = [eng.step(video, audio, P(ids[i].contiguous())) for i in range(2)]
    torch.cuda.synchronize()
    res = {"loss0": losses[0], "loss1": losses[1], "grad": eng.flat.grad, "params": eng.flat.flat, "adam_m": eng.m, "adam_v": eng.v,
           "adam_t": eng.t_dev, "bank1": crit.nce_average.view1_mem, "bank2": crit.nce_average.view2_mem}
    res.update(_buffers(m))
    return res


@case("program:finetune_step")
def _finetune(dev, P):
    """tests/test_gpu_finetune.py test_programs_match_the_per_layer_path, smallest shape (4, 3, 8, 112, 112)"""
    import test_gpu_finetune as FT
    from avid_hip import parallel
    m = FT._wrapper(dev)
    eng = parallel.FinetuneStep(m)
    g = torch.Generator().manual_seed(4 * 8)
    video = P(torch.randn((4, 3, 8, 112, 112), generator=g).to(dev))
    labels = P(torch.randint(0, 101, (4,), generator=g).to(dev))
    loss, hits = eng.step(video, labels)
    torch.cuda.synchronize()
    res = {"loss": loss, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat, "adam_m": eng.m, "adam_v": eng.v}
    res.update(_buffers(m))
    return res


@case("program:probe_step")
def _probe_step(dev, P):
    """tests/_inference_probe.py most_model, 4 clips of 3x8x64x64"""
    from _inference_probe import most_model
    from avid_hip import parallel
    m = most_model(dev)
    eng = parallel.ProbeStep(m)
    g = torch.Generator().manual_seed(1)
    video = P(torch.randn((4, 3, 8, 64, 64), generator=g).to(dev))
    labels = P(torch.randint(0, 400, (4,), generator=g).to(dev))
    losses, hits = eng.step(video, labels)
    torch.cuda.synchronize()
    res = {"losses": losses, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat, "adam_m": eng.m, "adam_v": eng.v}
    res.update(_buffers(m))
    return res


@case("program:inference")
def _inference(dev, P):
    """tests/_inference_probe.py wrapper at 3x8x48x48: the inference program and its recycled arena"""
    from _inference_probe import wrapper
    from avid_hip import parallel
    m = wrapper(dev, seed=21)
    g = torch.Generator().manual_seed(22)
    video = P(torch.randn((4, 3, 8, 48, 48), generator=g).to(dev))
    inf = parallel.Inference(m)
    logits = inf(video)
    assert inf.used_programs, "the inference call did not take the launch program"
    feats = parallel.Inference(m.feature_extractor)(video)
    torch.cuda.synchronize()
    res = {"logits": logits, "features": feats}
    res.update(_buffers(m))
    return res


# ------------------------------------------------------------------------------------------------------------- the one test
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _snapshot(name, res):
    out = {}
    for k, v in res.items():
        assert isinstance(v, torch.Tensor), (name, k, type(v))
        for (prefix, field), (keep, _) in EXCLUSIONS.items():
            if name.startswith(prefix) and k == field:
                v = v[keep]
        out[k] = (tuple(v.shape), v.dtype, _bits(v))
    return out


def _first_difference(a, b):
    d = (a != b).nonzero().flatten()
    return f"{d.numel()} of {a.numel()} bytes differ, first at byte {int(d[0])}"


_DEVICE_ERROR = []          # a case that ended in a device or library error: the cases after it do not touch the GPU


@pytest.mark.parametrize("name", list(CASES))
def test_no_write_outside_and_no_read_of_unwritten_memory(name, gpu_device):
    if _DEVICE_ERROR:
        pytest.fail(f"not run: the earlier case {_DEVICE_ERROR[0]} ended in a device error")
    try:
        _run_case(name, gpu_device)
    except (AssertionError, pytest.skip.Exception):       # (a skip: a CU budget that is no reduction on this device)
        raise
    except BaseException:
        _DEVICE_ERROR.append(name)
        raise


def _run_case(name, gpu_device):
    fn, has_backward, wants_ws, in_place = CASES[name]
    dev = gpu_device
    plain = _snapshot(name, fn(dev, lambda t: t))
    guarded_runs = []
    for fill in FILLS:
        with guarded(fill) as g:
            res = fn(dev, g.place)
            torch.cuda.synchronize()
            g.check()                                                                       # (a)
            snap = _snapshot(name, res)
        # the mechanism was engaged
        assert any(r.kind == "input" for r in g.records), f"{name}: no input was placed"
        if not in_place:
            assert any(r.kind != "input" for r in g.records), f"{name}: no allocation or workspace was intercepted (fill 0x{fill:02X})"
        if has_backward:
            assert g.count_in("backward") > 0, f"{name}: no allocation was intercepted inside an autograd backward"
        # every workspace handed out (each of exactly the bytes asked for: Guards.workspace) was sized by an answer of one of
        # the size functions called in this run; which function is not told apart: a case calls the functions of its own op
        for asked, site, _ in g.workspaces:
            assert asked in g.size_values or (asked == 16 and min(g.size_values, default=16) < 16), \
                f"{name}: workspace of {asked} bytes at {site}, the size functions returned {sorted(g.size_values)}"
        if wants_ws:
            assert any(asked > 0 for asked, _, _ in g.workspaces), f"{name}: no workspace of non-zero size was handed out"
        for fn_name in (wants_ws if isinstance(wants_ws, tuple) else ()):         # a non-zero workspace below each of these
            assert any(asked > 0 and fn_name in callers for asked, _, callers in g.workspaces), \
                f"{name}: no non-zero workspace was handed out in {fn_name}: {[(a, s_) for a, s_, _ in g.workspaces]}"
        if name.startswith("program:"):
            # sealed programs: each stream's workspace is a guarded buffer of exactly the largest answer of
            # avid_program_workspace_bytes for that stream, and that figure is what the C side is told
            assert g.programs, f"{name}: no launch program was sealed"
            for ws_bytes, numel, passed, needs in g.programs:
                assert needs, f"{name}: a program was sealed without asking avid_program_workspace_bytes"
                want = [max(n[k] for n in needs) for k in range(4)]
                assert ws_bytes == want and numel == want and passed == want, (name, ws_bytes, numel, passed, needs)
            assert any(max(w[0]) > 0 for w in g.programs), f"{name}: no program asked for any workspace"
        guarded_runs.append(snap)
    ff, fa = guarded_runs
    assert set(ff) == set(fa) == set(plain)
    for k in plain:
        assert ff[k][:2] == fa[k][:2] == plain[k][:2], (name, k, ff[k][:2], fa[k][:2], plain[k][:2])
        assert torch.equal(ff[k][2], fa[k][2]), \
            f"{name}: '{k}' depends on unwritten memory (0xFF vs 0x5A fill): {_first_difference(ff[k][2], fa[k][2])}"   # (b)
        assert torch.equal(ff[k][2], plain[k][2]), \
            f"{name}: '{k}' differs from the plain run: {_first_difference(ff[k][2], plain[k][2])}"                      # (c)
