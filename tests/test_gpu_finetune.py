"""Action-recognition fine-tuning on the GPU: the new kernels (dropout, softmax cross-entropy, the classifier's linear
layer) against host restatements in float64, the compiled classifier programs against the per-layer path and the float64
oracle, the FinetuneStep engine against a plain torch loop, and the reference's eval script shape through the launcher."""
import copy
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "avid-cma_amd")


def _host_mask(B, Fd, p, seed, offset):
    """The keep-mask restated on the host from oracle.avid_oracle.philox4x32_10 (include/avid_hip.h avid_dropout_fwd)."""
    from oracle import avid_oracle as O
    n = B * Fd
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    U32 = np.uint64(0xFFFFFFFF)
    words = O.philox4x32_10(g & U32, g >> np.uint64(32), np.uint64(offset) & U32, np.uint64(offset) >> np.uint64(32),
                            np.uint64(seed) & U32, np.uint64(seed) >> np.uint64(32))
    w = np.stack(words, 1).reshape(-1)[:n]
    thresh = np.uint64(int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32)))
    return (w >= thresh).reshape(B, Fd)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B", [1, 4, 8, 64, 320])
def test_dropout_mask_is_the_philox_restatement(gpu_device, B, p):
    _dropout_against_the_restatement(gpu_device, B, 512, p, 0x1234_5678_9ABC_DEF1 + B, 7 + B)


def test_dropout_past_the_grid_caps(gpu_device):
    """n = 4099 x 2049 elements: n mod 4 = 3 (a ragged last group of four), more than 4096 x 256 groups of four in the
    forward and more than 4096 x 256 elements in the backward, so both kernels go round their grid-stride loops."""
    B, Fd = 4099, 2049
    assert (B * Fd) % 4 == 3 and (B * Fd + 3) // 4 > 4096 * 256
    _dropout_against_the_restatement(gpu_device, B, Fd, 0.5, 0x0FED_CBA9_8765_4321, 11)


def _dropout_against_the_restatement(gpu_device, B, Fd, p, seed, offset):
    from avid_hip import ops
    x = torch.randn(B, Fd, device=gpu_device, requires_grad=True)
    y = ops.dropout(x, p, seed, offset)
    want = torch.from_numpy(_host_mask(B, Fd, p, seed, offset)).to(gpu_device)
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    assert torch.equal(y.detach(), torch.where(want, x.detach() * scale.item(), torch.zeros_like(x)))
    dy = torch.randn_like(y)
    y.backward(dy)
    assert torch.equal(x.grad, torch.where(want, dy * scale.item(), torch.zeros_like(dy)))
    assert torch.equal(ops.dropout_mask(B, Fd, p, seed, offset, gpu_device).bool(), want)


def test_dropout_keeps_one_minus_p(gpu_device):
    from avid_hip import ops
    B, Fd, p = 2048, 1024, 0.5
    m = ops.dropout_mask(B, Fd, p, 99, 3, gpu_device).double()
    n = B * Fd
    kept = float(m.mean())
    assert abs(kept - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5, kept
    assert not torch.equal(ops.dropout_mask(8, 512, p, 99, 3, gpu_device), ops.dropout_mask(8, 512, p, 99, 4, gpu_device))


def _ref_loss(logits, labels, clips):
    x = logits.double().cpu()
    V = labels.shape[0]
    lab = labels.cpu().repeat_interleave(clips)
    loss = F.cross_entropy(x, lab)
    conf = torch.softmax(x, 1).view(V, clips, -1).mean(1)
    dl = (torch.softmax(x, 1) - F.one_hot(lab, x.shape[1]).double()) / x.shape[0]
    return loss, conf, dl


@pytest.mark.parametrize("C", [51, 101, 400])
@pytest.mark.parametrize("B", [1, 4, 8, 64, 320])
def test_cls_loss_against_float64(gpu_device, B, C):
    from avid_hip import ops
    g = torch.Generator().manual_seed(B * 1000 + C)
    for clips in (1, 5):
        V = max(1, B // clips) if clips > 1 else B
        logits = (3 * torch.randn(V * clips, C, generator=g)).to(gpu_device)
        labels = torch.randint(0, C, (V,), generator=g).to(gpu_device)
        loss, conf, hits, dl = ops.cls_loss(logits, labels, clips, grad_scale=1.0)
        rl, rc, rd = _ref_loss(logits, labels, clips)
        assert abs(float(loss) - float(rl)) <= 1e-6 * abs(float(rl)), (float(loss), float(rl))
        assert float((conf.double().cpu() - rc).abs().max()) <= 1e-6 * float(rc.abs().max())
        assert float((dl.double().cpu() - rd).abs().max()) <= 1e-6 * float(rd.abs().max())
        top = rc.topk(min(5, C), 1).indices
        lab = labels.cpu()
        assert int(hits[0]) == int((top[:, 0] == lab).sum())
        assert int(hits[1]) == int((top == lab[:, None]).any(1).sum())
        # bit-reproducible
        again = ops.cls_loss(logits, labels, clips, grad_scale=1.0)
        assert torch.equal(again[0], loss) and torch.equal(again[1], conf) and torch.equal(again[2], hits)
        assert torch.equal(again[3], dl)
    ops.check_device_errors(gpu_device)


# B, C, Fin: the batch sizes and class counts of test_cls_loss_against_float64 at the tower's 512 features; fewer features
# than lanes (37) and a ragged count (100); one case whose backward (C * Fin + C + B * Fin = 1 474 960 elements, one thread
# each) is past its cap of 4096 blocks of 256
LINEAR_CASES = [(B, C, 512) for B in (1, 4, 8, 64, 320) for C in (51, 101, 400)] + \
               [(8, 101, 37), (8, 101, 100), (320, 400, 2048)]


def _relerr(got, want):
    return float((got.double() - want).abs().max() / (want.abs().max() + 1e-300))


@pytest.mark.parametrize("B,C,Fin", LINEAR_CASES, ids=["%dx%dx%d" % c for c in LINEAR_CASES])
def test_cls_linear_against_float64(gpu_device, B, C, Fin):
    """avid_cls_linear_fwd / avid_cls_linear_bwd on their own, every output filled with NaN first, against float64 F.linear
    and its autograd at the per-op bars (max|err| / max|ref| below 2e-5 for y and dx, 5e-5 for dw and db).  x is what the
    step feeds: positive (post-ReLU, max-pooled) features through dropout, about half of them zero and the rest doubled; w
    and bias at torch.nn.Linear's initial scale; dy the dlogits of ops.cls_loss on the forward's own logits.  bias = NULL,
    dx = NULL (the classifier-only program) and db = NULL leave the other outputs bit-identical; so does a repeated call."""
    from avid_hip import lib, ops
    dev = gpu_device
    assert C * Fin + C + B * Fin > 4096 * 256 or (B, C, Fin) != (320, 400, 2048)
    g = torch.Generator(device=dev).manual_seed(B * 100000 + C * 100 + Fin % 100)
    x = ops.dropout(torch.randn(B, Fin, generator=g, device=dev).abs(), 0.5, 0xC1A5 + B, C).contiguous()
    zeros = float((x == 0).double().mean())
    assert B * Fin < 4096 or 0.4 < zeros < 0.6, zeros
    bound = Fin ** -0.5
    w = ((torch.rand(C, Fin, generator=g, device=dev) * 2 - 1) * bound).contiguous()
    bias = ((torch.rand(C, generator=g, device=dev) * 2 - 1) * bound).contiguous()
    labels = torch.randint(0, C, (B,), generator=g, device=dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)                  # noqa: E731

    def fwd(b):
        y = nan(B, C)
        lib.call("avid_cls_linear_fwd", B, Fin, C, ops._p(x), ops._p(w), ops._p(b), ops._p(y), ops._stream())
        return y

    def bwd(dy, want_dx=True, want_db=True):
        dx, dw, db = nan(B, Fin), nan(C, Fin), nan(C)
        lib.call("avid_cls_linear_bwd", B, Fin, C, ops._p(x), ops._p(w), ops._p(dy), ops._p(dx if want_dx else None),
                 ops._p(dw), ops._p(db if want_db else None), ops._stream())
        return dx, dw, db

    y = fwd(bias)
    assert bool(torch.isfinite(y).all()), "an element of y was never written"
    dy = ops.cls_loss(y, labels, grad_scale=1.0)[3].contiguous()
    dx, dw, db = bwd(dy)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, bias))
    yr = F.linear(xr, wr, br)
    (yr * dy.double()).sum().backward()
    for name, got, want, bar in (("y", y, yr.detach(), 2e-5), ("dx", dx, xr.grad, 2e-5), ("dw", dw, wr.grad, 5e-5),
                                 ("db", db, br.grad, 5e-5)):
        assert bool(torch.isfinite(got).all()), (name, "an element was never written")
        err = _relerr(got, want)
        print(f"  cls_linear {B}x{C}x{Fin} {name:2s} max {err:.2e} / {bar:.0e}")
        assert err < bar, (name, err)
    # bias = NULL
    y0 = fwd(None)
    assert bool(torch.isfinite(y0).all())
    assert _relerr(y0, F.linear(x.double(), w.double())) < 2e-5
    # dx = NULL / db = NULL: the other outputs are the full call's bits, the absent one is not touched
    dx1, dw1, db1 = bwd(dy, want_dx=False)
    assert torch.equal(dw1, dw) and torch.equal(db1, db) and bool(torch.isnan(dx1).all())
    dx2, dw2, db2 = bwd(dy, want_db=False)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw) and bool(torch.isnan(db2).all())
    # bit-reproducible
    assert torch.equal(fwd(bias), y)
    assert all(torch.equal(a, b) for a, b in zip(bwd(dy), (dx, dw, db)))
    ops.check_device_errors(dev)


def test_cls_loss_tie_rule(gpu_device):
    from avid_hip import ops
    # every class equally likely: the label ranks by the number of LOWER class indices
    logits = torch.zeros(3, 10, device=gpu_device)
    labels = torch.tensor([0, 4, 5], device=gpu_device)
    _, _, hits, _ = ops.cls_loss(logits, labels)
    assert hits.tolist() == [1, 2]          # label 0: rank 0; label 4: rank 4 (top-5 hit); label 5: rank 5 (no hit)


@pytest.mark.parametrize("bad", [-1, 101])
def test_cls_loss_bad_label_raises(gpu_device, bad):
    from avid_hip import ops
    logits = torch.randn(4, 101, device=gpu_device)
    labels = torch.tensor([1, bad, 3, 4], device=gpu_device)
    ops.cls_loss(logits, labels)
    with pytest.raises(ops.AvidHipError):
        ops.check_device_errors(gpu_device)
    ops.check_device_errors(gpu_device)        # cleared


# ------------------------------------------------------------------------------------------------------------------
def _wrapper(dev, n_classes=101, seed=0):
    import models
    torch.manual_seed(seed)
    m = models.ClassificationWrapper(models.R2Plus1D(18), n_classes, "pool", 512, use_dropout=True, dropout=0.5)
    with torch.no_grad():           # non-trivial BatchNorm affines
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bn" in n:
                p.add_(0.1 * torch.randn_like(p))
    return m.to(dev).train()


def _grouped_ids(pl):
    from avid_hip import plan
    at = {4 * o: i for i, o in enumerate(pl.goff)}
    return {id(pl.params[at[pl.bwd_prog[k].t[2].off]]) for k in range(pl.n_bwd) if pl.bwd_prog[k].op == plan.OP_WGRAD_ITEM}


def _program_vs_per_layer(dev, shape):
    from avid_hip import ops, plan
    m1 = _wrapper(dev)
    m2 = copy.deepcopy(m1)
    m2.dropout.seed = m1.dropout.seed
    g = torch.Generator().manual_seed(shape[0] * shape[2])
    video = torch.randn(shape, generator=g).to(dev)
    labels = torch.randint(0, 101, (shape[0],), generator=g).to(dev)
    # program path
    m1.dropout.offset = 5
    l1 = m1(video)
    assert type(l1.grad_fn).__name__ == "ClsFnBackward", type(l1.grad_fn).__name__
    loss1, _, _, d1 = ops.cls_loss(l1.detach(), labels, grad_scale=1.0)
    l1.backward(d1)
    # per-layer path
    m2.dropout.offset = 5
    prev = plan.ENABLED
    plan.ENABLED = False
    try:
        l2 = m2(video)
    finally:
        plan.ENABLED = prev
    assert type(l2.grad_fn).__name__ != "ClsFnBackward"
    loss2, _, _, d2 = ops.cls_loss(l2.detach(), labels, grad_scale=1.0)
    l2.backward(d2)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(loss1, loss2)
    pls = [p for p in m1.__dict__["_avid_plans"].values() if p]
    grouped = _grouped_ids(pls[0])
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        if id(p1) in grouped:
            assert float((p1.grad - p2.grad).abs().max() / p2.grad.abs().max()) < 1e-5, n
        else:
            assert torch.equal(p1.grad, p2.grad), n
    for (n, b1), b2 in zip(m1.named_buffers(), m2.buffers()):
        assert torch.equal(b1, b2), n
    return m1, pls[0]


@pytest.mark.parametrize("shape", [(4, 3, 8, 112, 112), (2, 3, 16, 112, 112), (1, 3, 32, 224, 224), (8, 3, 8, 224, 224),
                                   (4, 3, 32, 224, 224)], ids=["4x8", "2x16", "1x32", "8x8x224", "4x32x224"])
def test_programs_match_the_per_layer_path(gpu_device, shape):
    _program_vs_per_layer(gpu_device, shape)


def test_programs_against_the_float64_oracle(gpu_device):
    """The per-layer path (the oracle's hooks pin ReLU signs and pool picks, and a hooked model is not compiled) against
    float64; the compiled programs are the per-layer path's bits at this shape (test_programs_match_the_per_layer_path[4x8])."""
    from avid_hip import ops, plan
    from oracle import avid_oracle as O
    from oracle.hooks import capture_relu_masks, capture_pool_argmax
    dev = gpu_device
    m = _wrapper(dev)
    g = torch.Generator().manual_seed(11)
    video = torch.randn((4, 3, 8, 112, 112), generator=g)
    labels = torch.randint(0, 101, (4,), generator=g)
    P = {("video_model." + k[len("feature_extractor."):] if k.startswith("feature_extractor.") else k): v.detach().double().cpu().clone()
         for k, v in m.state_dict().items()}
    shim = torch.nn.Module()
    shim.video_model = m.feature_extractor
    shim.audio_model = torch.nn.Identity()
    masks, remove = capture_relu_masks(shim)
    picks, remove_picks = capture_pool_argmax(shim)
    seed, offset = m.dropout.seed, m.dropout.offset
    try:
        logits = m(video.to(dev))
        assert type(logits.grad_fn).__name__ != "ClsFnBackward"
    finally:
        remove()
        remove_picks()
    loss, _, _, dl = ops.cls_loss(logits.detach(), labels.to(dev), grad_scale=1.0)
    logits.backward(dl)
    torch.cuda.synchronize()
    keep = ops.dropout_mask(4, 512, 0.5, seed, offset, dev).double().cpu()
    pn = [n for n in P if not ("running" in n or "num_batches" in n)]
    for n in pn:
        P[n].requires_grad_(True)
    O.RELU_MASKS, O.POOL_ARGMAX = masks, picks
    try:
        feat = O.r2plus1d_forward(video.double(), P, "video_model", 18, True).view(4, 512)
    finally:
        O.RELU_MASKS = O.POOL_ARGMAX = None
    ref_logits = F.linear(feat * keep * 2.0, P["classifier.weight"], P["classifier.bias"])
    ref = F.cross_entropy(ref_logits, labels)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    for n, p in m.named_parameters():
        key = "video_model." + n[len("feature_extractor."):] if n.startswith("feature_extractor.") else n
        r = P[key].grad
        err = float((p.grad.double().cpu() - r).abs().max() / (r.abs().max() + 1e-30))
        assert err < 5e-4, (n, err)


# ------------------------------------------------------------------------------------------------------------------
def _plain_step(m, opt, v, y, own_dlogits):
    """eval-action-recg.py's training phase: logits = model(video); cross-entropy; zero_grad / backward / torch.optim.Adam.
    own_dlogits: the backward starts from avid_cls_loss's dlogits instead of F.cross_entropy's."""
    from avid_hip import ops
    logits = m(v)
    opt.zero_grad()
    if own_dlogits:
        loss, _, _, d = ops.cls_loss(logits.detach(), y, grad_scale=1.0)
        logits.backward(d)
    else:
        loss = F.cross_entropy(logits, y)
        loss.backward()
    opt.step()
    return float(loss)


def _off_bar(m_a, m_b):
    """{parameter: (elements outside rtol 1e-4 / atol 1e-6, elements, max |difference|)} (test_gpu_dropin.py's bars)."""
    out = {}
    for (n, a), b in zip(m_a.named_parameters(), m_b.parameters()):
        off = ~torch.isclose(a, b, rtol=1e-4, atol=1e-6)
        if bool(off.any()):
            out[n] = (int(off.sum()), a.numel(), float((a - b).abs().max()))
    return out


def test_engine_against_torch_adam_loop(gpu_device):
    from avid_hip import ops, parallel
    dev, steps, lr = gpu_device, 3, 1e-4
    shape = (4, 3, 8, 112, 112)
    g = torch.Generator().manual_seed(3)
    vids = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 101, (4,), generator=g).to(dev) for _ in range(steps)]
    m0 = _wrapper(dev)
    m_eng, m_ce, m_own, m_chk = (copy.deepcopy(m0) for _ in range(4))
    # the first step's program-path gradient (the autograd node, from avid_cls_loss's dlogits)
    l = m_chk(vids[0])
    _, _, _, d = ops.cls_loss(l.detach(), labs[0], grad_scale=1.0)
    l.backward(d)
    eng = parallel.FinetuneStep(m_eng, lr=lr)
    opt_ce = torch.optim.Adam(m_ce.parameters(), lr=lr, weight_decay=0)
    opt_own = torch.optim.Adam(m_own.parameters(), lr=lr, weight_decay=0)
    le, l_ce, l_own = [], [], []
    for i in range(steps):
        loss, hits = eng.step(vids[i], labs[i])
        le.append(float(loss))
        if i == 0:
            torch.cuda.synchronize()
            for p, pc in zip(eng.flat.params, reversed(list(m_chk.parameters()))):
                assert torch.equal(p.grad, pc.grad)
        l_ce.append(_plain_step(m_ce, opt_ce, vids[i], labs[i], False))
        l_own.append(_plain_step(m_own, opt_own, vids[i], labs[i], True))
        torch.cuda.synchronize()
        if i == 0:
            # the same gradient bits (the loop started from the kernel's dlogits): the flat Adam is torch's Adam to
            # rtol 1e-4 / atol 1e-6 in every element
            assert not _off_bar(m_eng, m_own)
    assert 0 <= int(hits[0]) <= int(hits[1]) <= 4
    np.testing.assert_allclose(le[0], l_ce[0], rtol=2e-5)
    np.testing.assert_allclose(le[0], l_own[0], rtol=2e-5)
    # Later steps: Adam moves an element by about lr * sign(g) whatever |g| is, so where a gradient cancels down to rounding
    # level (a few percent of the stem's and conv2x's weights, sums over millions of pixels) the last-ulp differences of the
    # step before — flat Adam against torch's, F.cross_entropy's backward against avid_cls_loss's dlogits — choose the
    # direction.  Three steps in: the losses to rtol 1e-4 (measured 2.1e-5), at least 95 % of all elements at the bars
    # above, the classifier everywhere.
    total = sum(p.numel() for p in m_eng.parameters())
    for ref_losses, m_ref in ((l_ce, m_ce), (l_own, m_own)):
        np.testing.assert_allclose(le, ref_losses, rtol=1e-4)
        off = _off_bar(m_eng, m_ref)
        assert not any(n.startswith("classifier.") for n in off), off
        assert sum(k for k, _, _ in off.values()) <= 0.05 * total, off


def test_classifier_only_leaves_the_tower_alone(gpu_device):
    from avid_hip import parallel
    dev = gpu_device
    m_full = _wrapper(dev)
    m_warm = copy.deepcopy(m_full)
    before = {n: p.detach().clone() for n, p in m_warm.named_parameters()}
    g = torch.Generator().manual_seed(5)
    video = torch.randn((4, 3, 8, 112, 112), generator=g).to(dev)
    labels = torch.randint(0, 101, (4,), generator=g).to(dev)
    e_full = parallel.FinetuneStep(m_full)
    e_warm = parallel.FinetuneStep(m_warm, classifier_only=True)
    lf, _ = e_full.step(video, labels)
    lw, _ = e_warm.step(video, labels)
    torch.cuda.synchronize()
    assert torch.equal(lf, lw)
    for n, p in m_warm.named_parameters():
        if n.startswith("feature_extractor."):
            assert torch.equal(p, before[n]), n
        else:
            assert not torch.equal(p, before[n]), n
    for (n, a), b in zip(m_warm.named_buffers(), m_full.buffers()):
        assert torch.equal(a, b), n
    sd = e_warm.state_dict()
    assert sorted(sd["state"]) == [0, 1] and sd["param_groups"][0]["params"] == [0, 1]


def test_state_dict_round_trip_resumes_bit_for_bit(gpu_device):
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    vids = [torch.randn((2, 3, 8, 112, 112), generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, 101, (2,), generator=g).to(dev) for _ in range(3)]
    m = _wrapper(dev)
    eng = parallel.FinetuneStep(m)
    for i in range(2):
        eng.step(vids[i], labs[i])
    torch.cuda.synchronize()
    msd = {k: v.clone() for k, v in m.state_dict().items()}
    osd = copy.deepcopy(eng.state_dict())
    seed, off = m.dropout.seed, m.dropout.offset
    la, _ = eng.step(vids[2], labs[2])
    after = {n: p.detach().clone() for n, p in m.named_parameters()}
    m2 = _wrapper(dev, seed=1)
    m2.load_state_dict(msd)
    m2.dropout.seed, m2.dropout.offset = seed, off
    eng2 = parallel.FinetuneStep(m2)
    eng2.load_state_dict(osd)
    lb, _ = eng2.step(vids[2], labs[2])
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for n, p in m2.named_parameters():
        assert torch.equal(p, after[n]), n


def test_evaluate_matches_torch_softmax(gpu_device):
    from avid_hip import parallel
    dev = gpu_device
    m = _wrapper(dev)
    eng = parallel.FinetuneStep(m)
    g = torch.Generator().manual_seed(4)
    V, clips = 3, 4
    video = torch.randn((V, clips, 3, 8, 112, 112), generator=g).to(dev)
    labels = torch.randint(0, 101, (V,), generator=g).to(dev)
    conf, loss, hits = eng.evaluate(video, labels, batch=5)
    assert m.training
    m.eval()
    with torch.no_grad():
        logits = torch.cat([m(video.flatten(0, 1)[i:i + 5]) for i in range(0, V * clips, 5)])
    m.train()
    ref = torch.softmax(logits, 1).view(V, clips, -1).mean(1)
    torch.testing.assert_close(conf, ref, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(loss, F.cross_entropy(logits, labels.repeat_interleave(clips)), rtol=1e-5, atol=1e-6)
    top = ref.topk(5, 1).indices
    assert int(hits[0]) == int((top[:, 0] == labels).sum()) and int(hits[1]) == int((top == labels[:, None]).any(1).sum())


def test_hooked_wrapper_takes_the_per_layer_path(gpu_device):
    """Hooks on the classifier (and inside the tower) run, as they do around the reference's torch.nn.Linear, and the
    logits are the compiled programs' bits."""
    m = _wrapper(gpu_device)
    m_ref = copy.deepcopy(m)
    video = torch.randn(2, 3, 8, 64, 64, device=gpu_device)
    calls = []
    hs = [m.classifier.register_forward_pre_hook(lambda mod, inp: calls.append("pre")),
          m.classifier.register_forward_hook(lambda mod, inp, out: calls.append(("fwd", tuple(out.shape)))),
          m.classifier.register_full_backward_hook(lambda mod, gi, go: calls.append("bwd")),
          m.feature_extractor.conv5x[1].out_bn.register_forward_hook(lambda *a: calls.append("tower"))]
    out = m(video)
    assert type(out.grad_fn).__name__ != "ClsFnBackward"
    out.sum().backward()
    for h in hs:
        h.remove()
    assert calls == ["tower", "pre", ("fwd", (2, 101)), "bwd"], calls
    ref = m_ref(video)
    assert type(ref.grad_fn).__name__ == "ClsFnBackward"
    assert torch.equal(out, ref)


def test_labels_are_checked(gpu_device):
    from avid_hip import parallel
    eng = parallel.FinetuneStep(_wrapper(gpu_device))
    video = torch.randn(2, 3, 8, 64, 64, device=gpu_device)
    for bad in (torch.tensor([1, 2], dtype=torch.int32, device=gpu_device), torch.tensor([1], device=gpu_device),
                torch.tensor([1, 2])):
        with pytest.raises(ValueError):
            eng.step(video, bad)


def test_recreated_buffers_get_a_new_plan(gpu_device):
    """`.cpu().cuda()` re-creates the BatchNorm buffers: the next compiled call updates the new ones (plan.run's rule)."""
    m = _wrapper(gpu_device)
    video = torch.randn(2, 3, 8, 64, 64, device=gpu_device)
    m(video).sum().backward()
    bn = m.feature_extractor.conv1[1]
    assert int(bn.num_batches_tracked) == 1
    m.cpu().cuda()
    before = bn.running_mean.clone()
    out = m(video)
    assert type(out.grad_fn).__name__ == "ClsFnBackward"
    out.sum().backward()
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == 2 and not torch.equal(bn.running_mean, before)
    assert len([p for p in m.__dict__["_avid_plans"].values() if p]) == 2


# ------------------------------------------------------------------------------------------------------------------
def test_standin_eval_loop_through_the_launcher(gpu_device, tmp_path):
    """The shape of eval-action-recg.py's training phase (build_model -> ClassificationWrapper; logits = model(video);
    CrossEntropyLoss; zero_grad / backward / step) restated in a stand-in checkout, run through the launcher."""
    ref = tmp_path / "ref"
    (ref / "utils").mkdir(parents=True)
    (ref / "utils" / "__init__.py").write_text("")
    (ref / "utils" / "eval_utils.py").write_text(textwrap.dedent("""
        import torch

        class ClassificationWrapper(torch.nn.Module):
            pass

        def build_model(feature_extractor, args):
            return ClassificationWrapper(feature_extractor=feature_extractor, **args)
    """))
    (ref / "eval_loop.py").write_text(textwrap.dedent("""
        import json
        import torch
        import models
        from utils import eval_utils
        torch.manual_seed(0)
        net = eval_utils.build_model(models.R2Plus1D(depth=18), dict(n_classes=101, feat_name="pool", feat_dim=512,
                                                                     pooling_op=None, use_dropout=True, dropout=0.5))
        net = net.cuda().train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=0.0)
        crit = torch.nn.CrossEntropyLoss()
        out = []
        for it in range(2):
            video = torch.randn(2, 3, 8, 64, 64, device="cuda")
            target = torch.randint(0, 101, (2,), device="cuda")
            logits = net(video)
            loss = crit(logits, target)
            opt.zero_grad()
            loss.backward()
            opt.step()
            out.append([type(logits.grad_fn).__name__, loss.item()])
        print(json.dumps(out))
    """))
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG
    r = subprocess.run([sys.executable, "-m", "avid_hip.run_reference", str(ref / "eval_loop.py")], cwd=str(ref), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [g[0] for g in got] == ["ClsFnBackward", "ClsFnBackward"]
    assert all(np.isfinite(g[1]) for g in got)
