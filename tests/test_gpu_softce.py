"""Soft-target fine-tuning on the GPU: label smoothing, mixup and CutMix.

1. ``avid_soft_ce_loss`` against the float64 restatement of tests/_softce_ref.py within the bounds tests/test_softce_host.py
   derives (loss, gradient, confidence; the rank rule on the device's own confidences), the same bits on every run and at CU
   budgets 8 and 24, ``ops.cls_loss`` on one-hot targets, the tie rules, bad targets through the device error word, autograd.
2. ``avid_batch_mix``: mixup bit-identical to torch's float32 expression computed on the CPU, CutMix bit-identical to slicing,
   the targets from labels and from rows, a partner out of range, a bad label, what is refused.
3. The engines: ``FinetuneStep`` / ``ProbeStep(loss="soft_ce", label_smoothing=0.1)`` over the launch programs against the
   per-layer path with ``ops.soft_ce_loss``, bit for bit; the step's loss and ``dlogits`` against float64; int64 labels;
   ``virtual_ranks=2``; ``classifier_only``; the step guard; ``evaluate``; ``GpuBatchMix`` in front of the step.
4. One guarded case per new op and per new program (tests/_guards.py)."""
import contextlib
import copy
import math

import numpy as np
import pytest
import torch

import _audio_downstream as AD
import _softce_ref as R
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu

VIDEO = (4, 3, 8, 64, 64)                 # tests/test_gpu_plan.py's clips
EPS = 0.1


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _excess(got, want, bound):
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - np.asarray(want)) / np.asarray(bound)).max())


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


# ---------------------------------------------------------------------------------------------------------- 1. avid_soft_ce_loss
@pytest.mark.parametrize("kind", R.TARGET_KINDS)
@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_soft_ce_loss_against_float64(gpu_device, shape, kind):
    from avid_hip import ops
    dev = gpu_device
    V, clips, C = shape
    x, t = R.loss_inputs(V, clips, C, kind)
    xd, td = _dev(x, dev), _dev(t, dev)
    for eps in (0.0, EPS):
        loss, conf, hits, dl = ops.soft_ce_loss(xd, td, clips, eps, grad_scale=1.0)
        torch.cuda.synchronize()
        rows = [("loss", _excess(float(loss), R.loss(x, t, clips, eps), R.loss_bound(x, t, clips, eps))),
                ("dlogits", _excess(_np(dl), R.grad(x, t, clips, eps), R.grad_bound(x, t, clips, eps))),
                ("conf", _excess(_np(conf), R.confidence(x, t, clips), R.confidence_bound(x, t, clips)))]
        print(f"\n[soft_ce_loss {shape} {kind} eps {eps}] " + ", ".join(f"{k} {e:.3f} of its bound" for k, e in rows))
        for k, e in rows:
            assert e <= 1.0, (k, e, eps)
        assert R.hits(_np(conf).astype(np.float64), t) == tuple(hits.tolist())        # the rule, on the device's own confidences
        assert 0 <= int(hits[0]) <= int(hits[1]) <= V
        # the same bits on every run and under every CU budget
        want = [_bits(v) for v in (loss, conf, hits, dl)]
        try:
            for budget in (0, 8, 24):
                if budget:
                    assert ops.set_cu_budget(budget) == budget
                again = ops.soft_ce_loss(xd, td, clips, eps, grad_scale=1.0)
                assert all(torch.equal(_bits(a), b) for a, b in zip(again, want)), budget
        finally:
            ops.set_cu_budget(0)
        # grad_scale scales dlogits and nothing else; without it no gradient is written
        l2, c2, h2, d2 = ops.soft_ce_loss(xd, td, clips, eps)
        assert d2 is None and torch.equal(l2, loss) and torch.equal(c2, conf) and torch.equal(h2, hits)
        l3, c3, h3, d3 = ops.soft_ce_loss(xd, td, clips, eps, grad_scale=0.5)
        assert torch.equal(l3, loss) and torch.equal(c3, conf) and torch.equal(h3, hits)
        assert _excess(_np(d3), R.grad(x, t, clips, eps, 0.5), R.grad_bound(x, t, clips, eps, 0.5)) <= 1.0
    ops.check_device_errors(dev)


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_hot_targets_without_smoothing_are_cls_loss(gpu_device, shape):
    """With one-hot targets and no smoothing the two kernels compute one quantity: loss, confidence and gradient agree within
    the bounds of tests/_softce_ref.py (around ``cls_loss``'s values), the hits are equal."""
    from avid_hip import ops
    dev = gpu_device
    V, clips, C = shape
    x, t = R.loss_inputs(V, clips, C, "hard")
    xd, td = _dev(x, dev), _dev(t, dev)
    labels = td.argmax(1)
    l1, c1, h1, d1 = ops.soft_ce_loss(xd, td, clips, 0.0, grad_scale=1.0)
    l2, c2, h2, d2 = ops.cls_loss(xd, labels, clips, grad_scale=1.0)
    torch.cuda.synchronize()
    e = [_excess(float(l1), float(l2), R.loss_bound(x, t, clips)), _excess(_np(c1), _np(c2), R.confidence_bound(x, t, clips)),
         _excess(_np(d1), _np(d2), R.grad_bound(x, t, clips))]
    print(f"\n[soft_ce_loss vs cls_loss {shape}] loss {e[0]:.3f} conf {e[1]:.3f} dlogits {e[2]:.3f} of the bound")
    assert max(e) <= 1.0, e
    assert h1.tolist() == h2.tolist()
    ops.check_device_errors(dev)


def test_soft_ce_loss_tie_rules(gpu_device):
    """Equal targets: the lower class index is the video's label.  Equal confidences: the lower index ranks first."""
    from avid_hip import ops
    dev = gpu_device
    x = torch.tensor([[1.0, 2.5, 2.5, 0.0, 0.0, 0.0, 0.0], [2.5, 2.5, 0.0, 0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0],
                      [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]], device=dev).repeat_interleave(2, 0)
    t = torch.tensor([[0.0, 0.5, 0.5, 0, 0, 0, 0],        # label 1 (tie with 2), which wins its confidence tie with 2: top-1
                      [0.0, 0.5, 0.5, 0, 0, 0, 0],        # label 1, behind its equal at index 0: rank 1
                      [0, 0, 0, 0, 0.3, 0.3, 0.0],        # label 4, behind four equals: rank 4, a top-5 hit
                      [0, 0, 0, 0, 0.2, 0.3, 0.0]], device=dev)   # label 5, behind five equals: rank 5, no hit
    _, conf, hits, _ = ops.soft_ce_loss(x, t, clips=2)
    assert conf[0, 1] == conf[0, 2] and conf[1, 0] == conf[1, 1] and conf[2, 0] == conf[2, 5]
    assert hits.tolist() == [1, 3]
    assert R.hits(_np(conf).astype(np.float64), _np(t)) == (1, 3)
    ops.check_device_errors(dev)


@pytest.mark.parametrize("bad", [-0.25, float("nan"), float("inf")])
def test_soft_ce_loss_bad_target_raises(gpu_device, bad):
    from avid_hip import ops
    dev = gpu_device
    x = torch.randn(6, 65, device=dev)
    t = torch.zeros(3, 65, device=dev)
    t[:, 3] = 1.0
    ok = t.clone()
    t[2, 64] = bad
    _, _, hits, _ = ops.soft_ce_loss(x, t, clips=2)
    assert int(hits[1]) <= 2                # the bad video counts no hit
    with pytest.raises(ops.TargetError):
        ops.check_device_errors(dev)
    ops.check_device_errors(dev)            # raised once, then cleared
    ops.soft_ce_loss(x, ok, clips=2)
    ops.soft_ce_loss(x, ok * 1.5, clips=2)  # an unnormalised row is no error
    ops.check_device_errors(dev)


def test_soft_ce_loss_refusals_and_autograd(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    x, t = torch.randn(6, 5, device=dev), torch.full((3, 5), 0.2, device=dev)
    for args in ((x, t[:, :4], 2), (x, t, 3), (x, t.long(), 2), (x.double(), t, 2), (x, t.cpu(), 2), (x, t, 2, 1.0), (x, t, 2, -0.5),
                 (x, torch.zeros(3, dtype=torch.int64, device=dev), 2)):
        with pytest.raises(ops.AvidHipError):
            ops.soft_ce_loss(*args)
    # the autograd form: loss.backward() leaves dlogits in .grad, through a function of the logits too
    t = torch.softmax(torch.randn(3, 5, device=dev), 1)
    w = torch.randn(6, 5, device=dev, requires_grad=True)
    loss, conf, hits, dl = ops.soft_ce_loss(w * 2.0, t, 2, EPS, grad_scale=1.0)
    (3.0 * loss).backward()
    assert not conf.requires_grad and torch.equal(w.grad, dl * 3.0 * 2.0)
    ref = torch.nn.functional.cross_entropy((w.detach() * 2.0).double(), t.repeat_interleave(2, 0).double(), label_smoothing=EPS)
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    with torch.no_grad():
        assert ops.soft_ce_loss(w, t, 2)[0].grad_fn is None
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------------- 2. avid_batch_mix
def _lams(B):
    return {"0": [0.0] * B, "1": [1.0] * B, "0.5": [0.5] * B, "long": [R.LONG_LAM] * B,
            "per_sample": list(np.linspace(0.05, 0.95, B).astype(np.float32))}


@pytest.mark.parametrize("shape", R.MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mixup_is_torch_float32_bit_for_bit(gpu_device, shape):
    from avid_hip import ops
    dev = gpu_device
    x = R.mix_inputs(shape)
    B = shape[0]
    xt = torch.from_numpy(x)
    xd = xt.to(dev)
    fma_seen = False
    for pname, perm in R.perms(B).items():
        pt = torch.from_numpy(perm)
        for lname, lam in _lams(B).items():
            lt = torch.tensor(lam, dtype=torch.float32)
            l5 = lt.view(-1, 1, 1, 1, 1)
            want = l5 * xt + (1 - l5) * xt[pt]                                   # torch's float32 expression, on the CPU
            y, t_out = ops.batch_mix(xd, pt.to(dev), lt.to(dev))
            assert t_out is None and y.data_ptr() != xd.data_ptr()
            assert torch.equal(_bits(y), _bits(want)), (pname, lname)
            assert R.mixup(x, perm, lam).tobytes() == want.numpy().tobytes()
            fma_seen = fma_seen or R.mixup_fma(x, perm, lam).tobytes() != want.numpy().tobytes()
    assert fma_seen or x.size <= 3               # a contracted fma would have shown on this input
    assert torch.equal(xd.cpu(), xt)             # the input is untouched
    # a spectrogram [B, 1, T, F] is the same call
    if shape[1] == 1 and shape[2] == 1:
        lt, pt = torch.full((B,), R.LONG_LAM), torch.from_numpy(R.perms(B)["cycle"])
        y4, _ = ops.batch_mix(xd[:, :, 0], pt.to(dev), lt.to(dev))
        l4 = lt.view(-1, 1, 1, 1)
        assert y4.shape == xd[:, :, 0].shape and torch.equal(_bits(y4), _bits(l4 * xt[:, :, 0] + (1 - l4) * xt[:, :, 0][pt]))
    ops.check_device_errors(dev)


@pytest.mark.parametrize("shape", R.MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cutmix_is_slicing_bit_for_bit(gpu_device, shape):
    from avid_hip import ops
    dev = gpu_device
    x = R.mix_inputs(shape)
    B, _, _, H, W = shape
    xd = torch.from_numpy(x).to(dev)
    lam = torch.full((B,), 0.25, device=dev)
    names = list(R.boxes(H, W))
    for pname, perm in R.perms(B).items():
        pd = torch.from_numpy(perm).to(dev)
        for name, bx in R.boxes(H, W).items():
            box = np.asarray([bx] * B, np.int32)
            y, _ = ops.batch_mix(xd, pd, lam, box=_dev(box, dev))
            assert _np(y).tobytes() == R.cutmix(x, perm, box).tobytes(), (pname, name)
        # a different box per sample
        box = np.asarray([R.boxes(H, W)[names[(b + 2) % len(names)]] for b in range(B)], np.int32)
        y, _ = ops.batch_mix(xd, pd, lam, box=_dev(box, dev))
        assert _np(y).tobytes() == R.cutmix(x, perm, box).tobytes(), pname
    ops.check_device_errors(dev)


def test_batch_mix_targets(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    B, C = 5, 301                                        # more classes than a workgroup has threads
    x = torch.from_numpy(R.mix_inputs(R.MIX_SHAPES[1])).to(dev)
    perm = R.perms(B)["fixed_point"]
    lam = np.asarray([R.LONG_LAM, 0.0, 1.0, 0.5, 0.77], np.float32)
    labels = np.asarray([0, 300, 7, 7, 150], np.int64)
    pd, ld = _dev(perm, dev), _dev(lam, dev)
    y1, t1 = ops.batch_mix(x, pd, ld, labels=_dev(labels, dev), n_classes=C)
    want = R.mix_targets(R.one_hot(labels, C), perm, lam)
    assert t1.shape == (B, C) and _np(t1).tobytes() == want.tobytes()
    lt, t_cpu = torch.from_numpy(lam)[:, None], torch.from_numpy(R.one_hot(labels, C))
    assert want.tobytes() == (lt * t_cpu + (1 - lt) * t_cpu[torch.from_numpy(perm)]).numpy().tobytes()
    rows = np.random.default_rng(2).random((B, C)).astype(np.float32)
    y2, t2 = ops.batch_mix(x, pd, ld, targets=_dev(rows, dev))
    assert _np(t2).tobytes() == R.mix_targets(rows, perm, lam).tobytes()
    y3, t3 = ops.batch_mix(x, pd, ld)
    assert t3 is None and torch.equal(y1, y2) and torch.equal(y1, y3)
    # CutMix mixes the targets by lam as well
    box = _dev(np.asarray([R.boxes(17, 23)["odd"]] * B, np.int32), dev)
    _, t4 = ops.batch_mix(x, pd, ld, box=box, labels=_dev(labels, dev), n_classes=C)
    assert torch.equal(t4, t1)
    # the one-hot rows alone
    assert _np(ops.one_hot(_dev(labels, dev), C)).tobytes() == R.one_hot(labels, C).tobytes()
    ops.check_device_errors(dev)


def test_batch_mix_partner_out_of_range_and_bad_label(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    shape = R.MIX_SHAPES[1]
    B, C = shape[0], 7
    x = R.mix_inputs(shape)
    xd = _dev(x, dev)
    lam = np.full(B, 0.5, np.float32)
    labels = np.arange(B, dtype=np.int64)
    for stray in (B, -1, 2 ** 40):
        perm = R.perms(B)["cycle"].copy()
        perm[2] = stray
        for box in (None, _dev(np.asarray([R.boxes(17, 23)["odd"]] * B, np.int32), dev)):
            y, t = ops.batch_mix(xd, _dev(perm, dev), _dev(lam, dev), box=box, labels=_dev(labels, dev), n_classes=C)
            torch.cuda.synchronize()
            ok = perm.copy()
            ok[2] = 2
            lam_ok = lam.copy()
            want = R.mixup(x, ok, lam_ok) if box is None else R.cutmix(x, ok, _np(box))
            want[2] = x[2]                                       # that sample is copied unmixed
            assert _np(y).tobytes() == want.tobytes(), stray
            wt = R.mix_targets(R.one_hot(labels, C), ok, lam)
            wt[2] = R.one_hot(labels, C)[2]
            assert _np(t).tobytes() == wt.tobytes()
            with pytest.raises(IndexError):
                ops.check_device_errors(dev)
            ops.check_device_errors(dev)                         # raised once, then cleared
    bad = labels.copy()
    bad[1] = C
    _, t = ops.batch_mix(xd, _dev(R.perms(B)["identity"], dev), _dev(np.ones(B, np.float32), dev), labels=_dev(bad, dev), n_classes=C)
    assert not _np(t)[1].any() and _np(t)[0, 0] == 1.0           # a zero row
    with pytest.raises(ops.LabelError):
        ops.check_device_errors(dev)
    ops.check_device_errors(dev)


def test_batch_mix_refusals(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    x = torch.zeros(4, 3, 2, 8, 8, device=dev)
    perm, lam = torch.arange(4, device=dev), torch.ones(4, device=dev)
    box = torch.zeros(4, 4, dtype=torch.int32, device=dev)
    lab = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(ops.AvidHipError):
        ops.batch_mix(x, perm, lam, out=x)                       # y aliasing x
    with pytest.raises(ops.AvidHipError):
        ops.batch_mix(x, perm, lam, out=x.view(-1)[8:].view(-1))  # another shape
    big = torch.zeros(2 * x.numel(), device=dev)
    with pytest.raises(ops.AvidHipError):
        ops.batch_mix(big[:x.numel()].view_as(x), perm, lam, out=big[64:64 + x.numel()].view_as(x))      # overlapping
    y, _ = ops.batch_mix(big[:x.numel()].view_as(x), perm, lam, out=big[x.numel():].view_as(x))           # disjoint halves: fine
    assert y.data_ptr() == big.data_ptr() + 4 * x.numel()
    for kw in (dict(perm=perm.int()), dict(perm=perm[:3]), dict(lam=lam.double()), dict(lam=lam[:3]), dict(box=box.long()),
               dict(box=box[:, :3]), dict(labels=lab), dict(labels=lab.int(), n_classes=3), dict(labels=lab, n_classes=0),
               dict(targets=torch.zeros(4, 3, device=dev), labels=lab, n_classes=3), dict(targets=torch.zeros(3, 3, device=dev)),
               dict(targets=torch.zeros(4, 3, device=dev), n_classes=4), dict(targets=torch.zeros(4, 3)), dict(perm=perm.cpu()),
               dict(x=x.double()), dict(x=x[0]), dict(x=x.cpu())):
        args = dict(x=x, perm=perm, lam=lam)
        args.update(kw)
        with pytest.raises(ops.AvidHipError):
            ops.batch_mix(**args)
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------------------ 3. the engines
@contextlib.contextmanager
def _per_layer():
    from avid_hip import plan
    prev, plan.ENABLED = plan.ENABLED, False
    try:
        yield
    finally:
        plan.ENABLED = prev


@contextlib.contextmanager
def _ungrouped():
    from avid_hip import ops
    prev, ops.GROUP_WGRAD = ops.GROUP_WGRAD, 0
    try:
        yield
    finally:
        ops.GROUP_WGRAD = prev


def _video_model(dev, C, seed=0):
    import models
    torch.manual_seed(seed)
    m = models.ClassificationWrapper(models.R2Plus1D(18), C, "pool", 512, use_dropout=True, dropout=0.5)
    m.dropout.seed = AD.FIXTURE_DROPOUT[0]
    return m.to(dev).train()


def _batch(shape, C, dev, seed, steps=1, B=None):
    """Clips and two-hot targets (mixup's: lam at one class, 1 - lam at another), and the labels of the larger share."""
    g = torch.Generator().manual_seed(seed)
    shape = (B or shape[0],) + tuple(shape[1:])
    xs = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    ts = []
    for _ in range(steps):
        a = torch.randint(0, C, (shape[0],), generator=g)
        b = (a + 1 + torch.randint(0, C - 1, (shape[0],), generator=g)) % C
        lam = 0.55 + 0.4 * torch.rand(shape[0], generator=g)
        t = torch.zeros(shape[0], C)
        t[torch.arange(shape[0]), a] = lam
        t[torch.arange(shape[0]), b] = 1 - lam
        ts.append(t.to(dev))
    return xs, ts


def _cls_per_layer_step(m, x, t, eps, opt=None):
    """The per-layer path: the modules' forward (one autograd node per layer), ``ops.soft_ce_loss`` in its autograd form."""
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        logits = m(x)
    assert type(logits.grad_fn).__name__ != "ClsFnBackward"
    loss, _, hits, dl = ops.soft_ce_loss(logits, t, 1, eps, grad_scale=1.0)
    loss.backward()
    if opt is not None:
        opt.step()
    return logits.detach(), loss.detach(), hits, dl


def _probe_per_layer_step(m, x, t, eps, opt=None):
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        out = m(x)
    assert all(type(v.grad_fn).__name__ != "ProbeFnBackward" for v in out.values())
    res = [ops.soft_ce_loss(v, t, 1, eps, grad_scale=1.0) for v in out.values()]
    sum(r[0] for r in res).backward()
    if opt is not None:
        opt.step()
    return torch.stack([r[0].detach() for r in res]), torch.stack([r[2] for r in res])


def _same(m1, m2, what=("grad", "param", "buffer")):
    if "buffer" in what:
        for (n, a), b in zip(m1.named_buffers(), m2.buffers()):
            assert torch.equal(a, b), n
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        if "param" in what:
            assert torch.equal(p1, p2), n
        if "grad" in what and p1.requires_grad:
            assert torch.equal(p1.grad, p2.grad), n


def _loss_against_float64(logits, t, eps, loss, hits, dl):
    """The step's loss, hits and dlogits against float64 on the step's OWN logits."""
    x, tn = _np(logits), _np(t)
    assert _excess(float(loss), R.loss(x, tn, 1, eps), R.loss_bound(x, tn, 1, eps)) <= 1.0
    assert _excess(_np(dl), R.grad(x, tn, 1, eps), R.grad_bound(x, tn, 1, eps)) <= 1.0
    assert tuple(hits.tolist()) == R.hits(R.confidence(x, tn), tn)


@pytest.mark.parametrize("tower,C", [("video", 10), ("audio", 65)])
def test_finetune_soft_ce_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device, tower, C):
    from avid_hip import ops, parallel, plan
    dev = gpu_device
    shape = VIDEO if tower == "video" else AD.SMALL
    xs, ts = _batch(shape, C, dev, 31 + C, steps=2)
    with _ungrouped():
        m1 = _video_model(dev, C) if tower == "video" else AD.cls_model(n_classes=C).to(dev).train()
        m2 = copy.deepcopy(m1)
        eng = parallel.FinetuneStep(m1, lr=1e-3, loss="soft_ce", label_smoothing=EPS)
        opt = parallel.Adam(list(m2.parameters()), lr=1e-3)
        for i in range(2):
            loss1, hits1 = eng.step(xs[i], ts[i])
            pl = eng._step_plan
            assert pl.loss == "soft_ce" and pl.fwd_prog[pl.n_fwd - 1].op == plan.OP_SOFT_CE_LOSS == 34
            logits2, loss2, hits2, dl2 = _cls_per_layer_step(m2, xs[i], ts[i], EPS, opt)
            torch.cuda.synchronize()
            assert loss1.dtype == torch.float32 and hits1.dtype == torch.int64 and hits1.shape == (2,)
            assert torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist(), i
            _same(m1, m2, ("grad",))
            _loss_against_float64(logits2, ts[i], EPS, loss1, hits1, dl2)
    _same(m1, m2, ("param", "buffer"))
    ops.check_device_errors(dev)


def test_probe_soft_ce_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device):
    from avid_hip import ops, parallel, plan
    dev, C = gpu_device, 10
    xs, ts = _batch(AD.SMALL, C, dev, 41 + C, steps=2)
    m1 = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    m2 = copy.deepcopy(m1)
    eng = parallel.ProbeStep(m1, lr=1e-3, loss="soft_ce", label_smoothing=EPS)
    opt = parallel.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3)
    for i in range(2):
        losses1, hits1 = eng.step(xs[i], ts[i])
        pl = eng._step_plan
        assert [pl.fwd_prog[k].op for k in range(pl.n_logits, pl.n_fwd)] == [plan.OP_SOFT_CE_LOSS] * 4
        losses2, hits2 = _probe_per_layer_step(m2, xs[i], ts[i], EPS, opt)
        torch.cuda.synchronize()
        assert losses1.shape == (4,) and hits1.shape == (4, 2)
        assert torch.equal(losses1, losses2) and torch.equal(hits1, hits2), i
        _same(m1, m2, ("grad",))
    _same(m1, m2, ("param", "buffer"))
    # the taps' losses of the last step against float64, on the per-layer path's own logits (the same bits as the programs')
    with _per_layer(), torch.no_grad():
        m3 = copy.deepcopy(m2)
        out = m3(xs[1])
    for v in out.values():
        l, _, h, d = ops.soft_ce_loss(v, ts[1], 1, EPS, grad_scale=1.0)
        _loss_against_float64(v, ts[1], EPS, l, h, d)
    ops.check_device_errors(dev)


@pytest.mark.parametrize("kind", ["finetune", "probe"])
def test_int64_labels_give_the_bits_of_their_one_hot_rows(gpu_device, kind):
    """``label_smoothing`` alone works with ordinary labels: they become one-hot rows on the device."""
    from avid_hip import ops, parallel
    dev, C = gpu_device, 10
    g = torch.Generator().manual_seed(5)
    x = torch.randn(AD.SMALL, generator=g).to(dev)
    labels = torch.randint(0, C, (AD.SMALL[0],), generator=g).to(dev)
    rows = torch.nn.functional.one_hot(labels, C).float()
    out = []
    for y in (labels, rows):
        if kind == "finetune":
            m = AD.cls_model(n_classes=C).to(dev).train()
            eng = parallel.FinetuneStep(m, lr=1e-3, loss="soft_ce", label_smoothing=EPS)
        else:
            m = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
            eng = parallel.ProbeStep(m, lr=1e-3, loss="soft_ce", label_smoothing=EPS)
        loss, hits = eng.step(x, y)
        torch.cuda.synchronize()
        out.append((loss.clone(), hits.clone(), eng.flat.flat.clone(), eng.flat.grad.clone()))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*out))
    assert math.isfinite(float(out[0][0].sum()))
    ops.check_device_errors(dev)


def _soft_shard(dev, kind, C, **kw):
    import test_gpu_virtual_downstream as VD
    from avid_hip import parallel

    class SoftShard(VD.Shard):
        def __init__(self):
            self.kind = kind
            if kind == "finetune":
                self.m = AD.cls_model(n_classes=C).to(dev).train()
                self.eng = parallel.FinetuneStep(self.m, loss="soft_ce", label_smoothing=EPS, **kw)
            else:
                self.m = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
                self.eng = parallel.ProbeStep(self.m, loss="soft_ce", label_smoothing=EPS, **kw)
    return VD, SoftShard()


@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
def test_virtual_finetune_soft_ce_step_is_the_two_shard_engines_sum(gpu_device, classifier_only):
    """tests/test_gpu_virtual_downstream.py's check: the shards are views of the global, already mixed, batch and its targets;
    per shard the mean over b rows, the shards' gradients summed in rank order and applied with 1 / R in ONE optimizer launch,
    bit for bit the one-shard engines' results."""
    from avid_hip import ops, parallel
    dev, Rk, b, C = gpu_device, 2, 4, 65
    VD, shard = _soft_shard(dev, "finetune", C, classifier_only=classifier_only)
    xs, ts = _batch(AD.SMALL, C, dev, 51, steps=2, B=8)
    m = AD.cls_model(n_classes=C).to(dev).train()
    m.dropout.seed = VD.BASE_SEED
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, virtual_ranks=Rk, loss="soft_ce", label_smoothing=EPS)
    n = eng.n_cls if classifier_only else eng.flat.numel
    VD._check_against_shards(eng, m, shard, xs, ts, Rk, b, n, seeds=VD._seeds(Rk))
    ops.check_device_errors(dev)


def test_virtual_probe_soft_ce_step_is_the_two_shard_engines_sum(gpu_device):
    from avid_hip import ops, parallel
    dev, Rk, b, C = gpu_device, 2, 4, 10
    VD, shard = _soft_shard(dev, "probe", C)
    xs, ts = _batch(AD.SMALL, C, dev, 52, steps=2, B=8)
    m = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    eng = parallel.ProbeStep(m, virtual_ranks=Rk, loss="soft_ce", label_smoothing=EPS)
    VD._check_against_shards(eng, m, shard, xs, ts, Rk, b, eng.flat.numel)
    ops.check_device_errors(dev)


def test_classifier_only_soft_ce_with_sgd_trains_the_classifier_alone(gpu_device):
    from avid_hip import ops, parallel
    dev, C = gpu_device, 10
    (x,), (t,) = _batch(VIDEO, C, dev, 61)
    m1 = _video_model(dev, C)
    m2 = copy.deepcopy(m1)
    before = {n: p.detach().clone() for n, p in m1.named_parameters()}
    eng = parallel.FinetuneStep(m1, lr=1e-2, classifier_only=True, loss="soft_ce", label_smoothing=EPS, optimizer="sgd", momentum=0.9)
    loss1, hits1 = eng.step(x, t)
    _, loss2, hits2, _ = _cls_per_layer_step(m2, x, t, EPS)
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist()
    for n, p in m1.named_parameters():
        assert torch.equal(p, before[n]) == (not n.startswith("classifier.")), n
    g2 = dict(m2.named_parameters())
    for n in ("classifier.weight", "classifier.bias"):
        assert torch.equal(dict(m1.named_parameters())[n].grad, g2[n].grad), n
    _same(m1, m2, ("buffer",))
    sd = eng.state_dict()
    assert len(sd["state"]) == 2 and all("momentum_buffer" in s for s in sd["state"].values())
    ops.check_device_errors(dev)


def test_step_guard_skips_a_step_with_one_non_finite_target(gpu_device):
    from avid_hip import ops, parallel
    dev, C = gpu_device, 10
    xs, ts = _batch(AD.SMALL, C, dev, 71, steps=2)
    m = AD.cls_model(n_classes=C).to(dev).train()
    eng = parallel.FinetuneStep(m, lr=1e-3, loss="soft_ce", label_smoothing=EPS, skip_nonfinite=True, max_grad_norm=1.0)
    eng.step(xs[0], ts[0])
    torch.cuda.synchronize()
    params, bufs = eng.flat.flat.clone(), {n: b.clone() for n, b in m.named_buffers()}
    bad = ts[1].clone()
    bad[2, 7] = float("nan")
    try:
        loss, _ = eng.step(xs[1], bad)
        assert int(eng.guard.skipped) == 1 and not math.isfinite(float(loss))
        assert torch.equal(eng.flat.flat, params) and all(torch.equal(b, bufs[n]) for n, b in m.named_buffers())
        with pytest.raises(ops.TargetError):                         # the same target is also reported through the error word
            ops.check_device_errors(dev)
    finally:
        with contextlib.suppress(ops.AvidHipError):
            ops.check_device_errors(dev)
    loss, _ = eng.step(xs[1], ts[1])
    assert int(eng.guard.skipped) == 0 and math.isfinite(float(loss)) and not torch.equal(eng.flat.flat, params)
    ops.check_device_errors(dev)


def test_dense_evaluation_with_hard_and_with_soft_labels(gpu_device):
    """3 videos x 2 clips.  Hard labels go through ``ops.cls_loss``, soft targets through ``ops.soft_ce_loss``; neither is smoothed."""
    from avid_hip import ops, parallel
    dev, V, clips, C = gpu_device, 3, 2, 65
    g = torch.Generator().manual_seed(81)
    x = torch.randn((V, clips) + AD.SMALL[1:], generator=g).to(dev)
    _, (t,) = _batch((V,) + AD.SMALL[1:], C, dev, 82)
    labels = t.argmax(1)
    m = AD.cls_model(n_classes=C).to(dev).train()
    eng = parallel.FinetuneStep(m, loss="soft_ce", label_smoothing=EPS)
    conf_h, loss_h, hits_h = eng.evaluate(x, labels, batch=4)                       # chunks of 4 and 2 clips
    conf_s, loss_s, hits_s = eng.evaluate(x, t, batch=4)
    assert m.training and conf_h.shape == conf_s.shape == (V, C)
    logits = parallel.Inference(m)(x.flatten(0, 1))
    want = ops.cls_loss(logits, labels, clips)
    torch.cuda.synchronize()
    assert torch.equal(loss_h, want[0]) and torch.equal(conf_h, want[1]) and torch.equal(hits_h, want[2])
    xn, tn = _np(logits), _np(t)
    assert _excess(float(loss_s), R.loss(xn, tn, clips, 0.0), R.loss_bound(xn, tn, clips, 0.0)) <= 1.0
    assert _excess(_np(conf_s), R.confidence(xn, tn, clips), R.confidence_bound(xn, tn, clips)) <= 1.0
    assert tuple(hits_s.tolist()) == R.hits(_np(conf_s).astype(np.float64), tn)
    smoothed = R.loss(xn, tn, clips, EPS)                                # the smoothed loss is another number
    assert abs(smoothed - R.loss(xn, tn, clips, 0.0)) > 100 * R.loss_bound(xn, tn, clips, 0.0)
    pm = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    confs, losses, hitss = parallel.ProbeStep(pm, loss="soft_ce", label_smoothing=EPS).evaluate(x, t, batch=4)
    assert pm.training and confs.shape == (4, V, C) and losses.shape == (4,) and hitss.shape == (4, 2)
    out = parallel.Inference(pm)(x.flatten(0, 1))
    for i, k in enumerate(AD.STAGES):
        xn = _np(out[k])
        assert _excess(float(losses[i]), R.loss(xn, tn, clips, 0.0), R.loss_bound(xn, tn, clips, 0.0)) <= 1.0, k
        assert _excess(_np(confs[i]), R.confidence(xn, tn, clips), R.confidence_bound(xn, tn, clips)) <= 1.0, k
    ops.check_device_errors(dev)


@pytest.mark.parametrize("tower", ["video", "audio"])
def test_batch_mix_then_step_gives_the_same_bits_twice(gpu_device, tower):
    """``GpuBatchMix`` in front of the ``"soft_ce"`` step: the same seed, the same bits — and the targets are what the step saw."""
    from avid_hip import ops, parallel
    from datasets.gpu_mix import GpuBatchMix
    dev, C = gpu_device, 10
    shape = VIDEO if tower == "video" else AD.SMALL
    g = torch.Generator().manual_seed(91)
    xs = [torch.randn(shape, generator=g).to(dev) for _ in range(3)]
    ys = [torch.randint(0, C, (shape[0],), generator=g).to(dev) for _ in range(3)]
    runs = []
    for _ in range(2):
        m = _video_model(dev, C) if tower == "video" else AD.cls_model(n_classes=C).to(dev).train()
        eng = parallel.FinetuneStep(m, lr=1e-3, loss="soft_ce", label_smoothing=EPS)
        mix = GpuBatchMix(C, mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, per_sample=True, seed=17)
        res, modes = [], []
        for x, y in zip(xs, ys):
            xm, t = mix(x, y)
            assert xm.data_ptr() != x.data_ptr() and t.shape == (shape[0], C) and t.dtype == torch.float32
            loss, hits = eng.step(xm, t)
            res += [loss.clone(), hits.clone(), t.clone(), xm[0, 0].clone()]
            modes.append(mix.last[0])
        torch.cuda.synchronize()
        runs.append((res + [eng.flat.flat.clone()], modes))
    assert runs[0][1] == runs[1][1] and any(mo is not None for mo in runs[0][1])
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(runs[0][0], runs[1][0]))
    # the mixed targets are the host arrays' float32 expression
    mode, perm, lam, box = mix.last
    want = R.mix_targets(R.one_hot(_np(ys[-1]), C), perm, lam)
    assert _np(runs[0][0][-3]).tobytes() == want.tobytes()
    assert abs(float(want.sum()) - shape[0]) < 1e-4
    ops.check_device_errors(dev)


# ----------------------------------------------------------------------------------------------------------------------- 4. guards
def _guard_soft_ce_loss(dev, P):
    from avid_hip import ops
    x, t = R.loss_inputs(7, 3, 65, "unnorm")
    loss, conf, hits, dl = ops.soft_ce_loss(P(_dev(x, dev)), P(_dev(t, dev)), 3, EPS, grad_scale=1.0)
    return {"loss": loss, "conf": conf, "hits": hits, "dlogits": dl}


def _guard_batch_mix(dev, P):
    from avid_hip import ops
    shape = R.MIX_SHAPES[1]
    B = shape[0]
    x = P(_dev(R.mix_inputs(shape), dev))
    perm, lam = P(_dev(R.perms(B)["cycle"], dev)), P(_dev(np.linspace(0.1, 0.9, B).astype(np.float32), dev))
    labels = P(_dev(np.arange(B, dtype=np.int64), dev))
    box = P(_dev(np.asarray([R.boxes(17, 23)["odd"]] * B, np.int32), dev))
    y1, t1 = ops.batch_mix(x, perm, lam, labels=labels, n_classes=7)
    y2, t2 = ops.batch_mix(x, perm, lam, box=box, targets=t1)
    return {"mixup": y1, "mixup_targets": t1, "cutmix": y2, "cutmix_targets": t2, "one_hot": ops.one_hot(labels, 7)}


def _guard_finetune(dev, P):
    from avid_hip import parallel
    C = 65
    m = AD.cls_model(n_classes=C).to(dev).train()
    eng = parallel.FinetuneStep(m, loss="soft_ce", label_smoothing=EPS)
    (x,), (t,) = _batch(AD.ODD, C, dev, 91)
    loss, hits = eng.step(P(x), P(t))
    torch.cuda.synchronize()
    res = {"loss": loss, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat}
    res.update({f"buffer:{n}": b for n, b in m.named_buffers()})
    return res


def _guard_probe(dev, P):
    from avid_hip import parallel
    C = 10
    m = AD.probe_model(AD.ODD, n_classes=C).to(dev).train()
    eng = parallel.ProbeStep(m, loss="soft_ce", label_smoothing=EPS)
    (x,), (t,) = _batch(AD.ODD, C, dev, 92)
    losses, hits = eng.step(P(x), P(t))
    torch.cuda.synchronize()
    res = {"losses": losses, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat}
    res.update({f"buffer:{n}": b for n, b in m.named_buffers()})
    return res


@pytest.mark.parametrize("case", [_guard_soft_ce_loss, _guard_batch_mix, _guard_finetune, _guard_probe],
                         ids=["soft_ce_loss", "batch_mix", "finetune_step", "probe_step"])
def test_soft_target_ops_and_programs_under_guards(gpu_device, case):
    """tests/test_gpu_guards.py's rule: (a) no byte of any guard band changes, with every workspace sized exactly by its query,
    (b) every result is the same bits under both fills of unwritten memory, and the same as without guards."""
    dev = gpu_device
    plain = {k: _bits(v) for k, v in case(dev, lambda t: t).items()}
    runs = []
    for fill in FILLS:
        with guarded(fill) as g:
            res = case(dev, g.place)
            torch.cuda.synchronize()
            g.check()
            runs.append({k: _bits(v) for k, v in res.items()})
        assert any(r.kind == "input" for r in g.records) and any(r.kind != "input" for r in g.records)
        if case in (_guard_finetune, _guard_probe):
            assert g.programs, "no launch program was sealed under the guards"
            for ws_bytes, numel, passed, needs in g.programs:
                want = [max(n[k] for n in needs) for k in range(4)]
                assert needs and ws_bytes == want and numel == want and passed == want
    ff, fa = runs
    assert set(ff) == set(fa) == set(plain)
    for k in plain:
        assert torch.equal(ff[k], fa[k]), f"'{k}' depends on unwritten memory"
        assert torch.equal(ff[k], plain[k]), f"'{k}' differs under guards"
