"""Multi-label fine-tuning, probing and evaluation on the GPU.

1. ``avid_mlabel_loss`` against the float64 restatement of tests/_mlabel_ref.py within the bounds tests/test_mlabel_host.py
   derives (loss, gradient, confidence; the hits of the float64 confidences), the same bits on every run and at CU budgets 8
   and 24, bad targets through the device error word, the autograd form.
2. ``avid_rank_metrics`` against the counting restatement at the host file's tolerance, NaN where defined, the same bits on every
   run, ``MultiLabelEval`` fed in three uneven chunks.
3. The engines: ``FinetuneStep(loss="bce")`` / ``ProbeStep(loss="bce")`` over the launch programs against the per-layer path with
   ``ops.mlabel_loss``, bit for bit; the step's loss and ``dlogits`` against float64; ``virtual_ranks=2``; ``classifier_only``;
   the step guard; ``evaluate``.
4. One guarded case per new op and per new program (tests/_guards.py)."""
import contextlib
import copy
import math

import numpy as np
import pytest
import torch

import _audio_downstream as AD
import _mlabel_ref as R
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu

VIDEO = (4, 3, 8, 64, 64)                 # tests/test_gpu_plan.py's clips
CLASSES = (10, 65)


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


# ------------------------------------------------------------------------------------------------------------ 1. avid_mlabel_loss
@pytest.mark.parametrize("with_pw", [False, True], ids=["plain", "pos_weight"])
@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mlabel_loss_against_float64(gpu_device, shape, with_pw):
    from avid_hip import ops
    dev = gpu_device
    V, clips, C = shape
    x, t, pw = R.loss_inputs(V, clips, C, soft=(C % 2 == 1), with_pw=with_pw)
    xd, td, pwd = _dev(x, dev), _dev(t, dev), _dev(pw, dev)
    loss, conf, hits, dl = ops.mlabel_loss(xd, td, clips, pwd, grad_scale=1.0)
    torch.cuda.synchronize()
    rows = [("loss", _excess(float(loss), R.loss(x, t, pw, clips), R.loss_bound(x, t, pw, clips))),
            ("dlogits", _excess(_np(dl), R.grad(x, t, pw, clips), R.grad_bound(x, t, pw, clips))),
            ("conf", _excess(_np(conf), R.confidence(x, t, clips), R.confidence_bound(x, t, clips)))]
    print(f"\n[mlabel_loss {shape} pos_weight {with_pw}] " + ", ".join(f"{k} {e:.3f} of its bound" for k, e in rows))
    for k, e in rows:
        assert e <= 1.0, (k, e)
    # the hits of the float64 confidences; a pair whose float64 confidence lies within the bound of 0.5 (but is not 0.5 itself,
    # as sigmoid(0) is) may fall on either side
    c64, cb = R.confidence(x, t, clips), R.confidence_bound(x, t, clips)
    top, pairs = R.hits(c64, t)
    loose = int(((np.abs(c64 - 0.5) <= cb) & (c64 != 0.5)).sum())
    srt = np.sort(c64, 1)
    clear_top = C == 1 or bool(((srt[:, -1] - srt[:, -2] > 2 * cb.max()) | (srt[:, -1] == srt[:, -2])).all())
    assert abs(int(hits[1]) - pairs) <= loose, (hits.tolist(), pairs, loose)
    if clear_top:
        assert int(hits[0]) == top
    assert R.hits(_np(conf).astype(np.float64), t) == tuple(hits.tolist())           # the rule, on the device's own confidences
    # the same bits on every run and under every CU budget
    want = [_bits(v) for v in (loss, conf, hits, dl)]
    try:
        for budget in (0, 8, 24):
            if budget:
                assert ops.set_cu_budget(budget) == budget
            again = ops.mlabel_loss(xd, td, clips, pwd, grad_scale=1.0)
            assert all(torch.equal(_bits(a), b) for a, b in zip(again, want)), budget
    finally:
        ops.set_cu_budget(0)
    # grad_scale scales dlogits and nothing else; without it no gradient is written
    l2, c2, h2, d2 = ops.mlabel_loss(xd, td, clips, pwd)
    assert d2 is None and torch.equal(l2, loss) and torch.equal(c2, conf) and torch.equal(h2, hits)
    d3 = ops.mlabel_loss(xd, td, clips, pwd, grad_scale=0.5)[3]
    assert _excess(_np(d3), R.grad(x, t, pw, clips, 0.5), R.grad_bound(x, t, pw, clips, 0.5)) <= 1.0
    ops.check_device_errors(dev)


def test_mlabel_loss_tie_rule_and_exact_half(gpu_device):
    """Equal logits give equal confidences: the lower class index is the top class.  sigmoid(0) is exactly 0.5 and counts as >= 0.5."""
    from avid_hip import ops
    dev = gpu_device
    x = torch.tensor([[1.5, 2.5, 2.5, -1.0], [2.5, 1.5, -1.0, 2.5], [0.0, -0.0, -3.0, -3.0]], device=dev).repeat_interleave(2, 0)
    t = torch.tensor([[0, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.float32, device=dev)
    _, conf, hits, _ = ops.mlabel_loss(x, t, clips=2)
    assert conf[0, 1] == conf[0, 2] and conf[1, 0] == conf[1, 3] and float(conf[2, 0]) == float(conf[2, 1]) == 0.5
    # top classes 1, 0, 0 against positives at 2, 0, 0: two videos; the pairs on the right side of 0.5: 2 + 2 + 3
    assert hits.tolist() == [2, 2 + 2 + 3]
    ops.check_device_errors(dev)


@pytest.mark.parametrize("bad", [1.5, -0.25, float("nan"), float("inf")])
def test_mlabel_loss_bad_target_raises(gpu_device, bad):
    from avid_hip import ops
    dev = gpu_device
    x = torch.randn(6, 65, device=dev)
    t = torch.zeros(3, 65, device=dev)
    t[2, 64] = bad
    ops.mlabel_loss(x, t, clips=2)
    with pytest.raises(ops.TargetError):
        ops.check_device_errors(dev)
    ops.check_device_errors(dev)            # cleared
    ops.mlabel_loss(x, torch.zeros(3, 65, device=dev), clips=2)
    ops.check_device_errors(dev)


def test_mlabel_loss_refusals_and_autograd(gpu_device):
    from avid_hip import ops
    dev = gpu_device
    x, t = torch.randn(6, 5, device=dev), torch.zeros(3, 5, device=dev)
    for args in ((x, t[:, :4], 2), (x, t, 3), (x, t.long(), 2), (x.double(), t, 2), (x, t.cpu(), 2),
                 (x, t, 2, torch.ones(4, device=dev)), (x, torch.zeros(3, dtype=torch.int64, device=dev), 2)):
        with pytest.raises(ops.AvidHipError):
            ops.mlabel_loss(*args)
    with pytest.raises(ops.AvidHipError):
        ops.rank_metrics(x, t)
    with pytest.raises(ops.AvidHipError):
        ops.rank_metrics(x, torch.zeros(6, 5, device=dev, dtype=torch.float64))
    # the autograd form: loss.backward() leaves dlogits in .grad, through a function of the logits too
    t = (torch.rand(3, 5, device=dev) < 0.4).float()
    pw = torch.rand(5, device=dev) + 0.5
    w = torch.randn(6, 5, device=dev, requires_grad=True)
    loss, conf, hits, dl = ops.mlabel_loss(w * 2.0, t, 2, pw, grad_scale=1.0)
    (3.0 * loss).backward()
    assert not conf.requires_grad and torch.equal(w.grad, dl * 3.0 * 2.0)
    ref = torch.nn.functional.binary_cross_entropy_with_logits((w.detach() * 2.0).double(), t.repeat_interleave(2, 0).double(),
                                                               pos_weight=pw.double())
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * float(ref)
    with torch.no_grad():
        assert ops.mlabel_loss(w, t, 2)[0].grad_fn is None
    ops.check_device_errors(dev)


# ----------------------------------------------------------------------------------------------------------- 2. avid_rank_metrics
_RANK_REF = {}


def _rank_ref(N, C):
    """The inputs and the restatement of one (N, C), computed once."""
    if (N, C) not in _RANK_REF:
        s, t = R.rank_inputs(N, C)
        _RANK_REF[(N, C)] = (s, t) + R.rank_metrics(s, t)
    return _RANK_REF[(N, C)]


def _check_metrics(got, want, who):
    ap, auc, n_pos = (_np(v) for v in got)
    rap, rauc, rn = want
    assert np.array_equal(n_pos, rn), who
    assert np.array_equal(np.isnan(ap), np.isnan(rap)) and np.array_equal(np.isnan(auc), np.isnan(rauc)), who
    ok = ~np.isnan(rap)
    worst = float((np.abs(ap - rap)[ok] / R.ap_tolerance(rn)[ok]).max()) if ok.any() else 0.0
    print(f"\n[rank_metrics {who}] ap {worst:.3f} of its tolerance, {int(ok.sum())} classes defined")
    assert worst <= 1.0, who
    ok = ~np.isnan(rauc)
    assert np.array_equal(auc[ok], rauc[ok]), who                    # integers and one division: the same double


@pytest.mark.parametrize("C", R.RANK_C)
@pytest.mark.parametrize("N", R.RANK_N)
def test_rank_metrics_against_the_counting_restatement(gpu_device, N, C):
    from avid_hip import ops
    dev = gpu_device
    s, t, rap, rauc, rn = _rank_ref(N, C)
    sd, td = _dev(s, dev), _dev(t, dev)
    got = ops.rank_metrics(sd, td)
    torch.cuda.synchronize()
    _check_metrics(got, (rap, rauc, rn), f"N {N} C {C}")
    if C > 4:
        assert math.isnan(float(got[0][4])) and math.isnan(float(got[1][4]))          # the NaN-score column
        with pytest.raises(ops.ScoreError):
            ops.check_device_errors(dev)
    ops.check_device_errors(dev)
    if C > 3:
        assert math.isnan(float(got[0][2])) and int(got[2][2]) == 0                     # P = 0
        assert math.isnan(float(got[1][3])) and int(got[2][3]) == N                     # P = N: AP defined, AUC not
        assert float(got[0][3]) == 1.0
    again = ops.rank_metrics(sd, td)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, got))
    with contextlib.suppress(ops.ScoreError):
        ops.check_device_errors(dev)


def test_rank_metrics_many_positives_take_rounds(gpu_device):
    """More positives than one round holds (256), continuous and heavily tied; and — the one size at which it shows — more rounds
    than a class has workgroups (64): N = 20 011 with 17 000 positives."""
    from avid_hip import ops
    dev = gpu_device
    rng = np.random.default_rng(3)
    N = 4099
    s = np.stack([rng.standard_normal(N), np.round(rng.standard_normal(N), 1), rng.standard_normal(N)], 1).astype(np.float32)
    t = np.stack([rng.random(N) < 0.8, rng.random(N) < 0.55, rng.random(N) < 0.07], 1).astype(np.float32)
    want = R.rank_metrics(s, t)
    assert want[2][0] > 12 * 256 and 8 * 256 < want[2][1] < 9 * 256 + 256 and 256 < want[2][2] < 2 * 256
    _check_metrics(ops.rank_metrics(_dev(s, dev), _dev(t, dev)), want, "N 4099, classes of 2 to 13 rounds")
    N = 20011
    s = np.stack([rng.standard_normal(N), np.round(rng.standard_normal(N), 1)], 1).astype(np.float32)
    t = np.stack([rng.random(N) < 0.85, rng.random(N) < 0.85], 1).astype(np.float32)
    want = R.rank_metrics(s, t)
    assert want[2].min() > 64 * 256
    _check_metrics(ops.rank_metrics(_dev(s, dev), _dev(t, dev)), want, "N 20011, 66 rounds over 64 workgroups")
    ops.check_device_errors(dev)


def test_multilabel_eval_in_chunks_equals_one_call(gpu_device):
    from avid_hip import ops, parallel
    dev = gpu_device
    N, C = 1000, 65
    s, t, rap, rauc, rn = _rank_ref(N, C)
    s, t = s.copy(), t.copy()
    s[N // 2, 4] = 0.25                                                # (no NaN column here)
    sd, td = _dev(s, dev), _dev(t, dev)
    one = ops.rank_metrics(sd, td)
    ev = parallel.MultiLabelEval(C)
    for a, b in ((0, 7), (7, 600), (600, N)):
        ev.add(sd[a:b], td[a:b].bool() if a == 7 else td[a:b])
    out = ev.compute()
    assert set(out) == {"ap", "auc", "n_pos", "mAP", "mAUC", "d_prime", "n_valid"} and all(v.is_cuda for v in out.values())
    for k, v in zip(("ap", "auc", "n_pos"), one):
        assert torch.equal(_bits(out[k]), _bits(v)), k
    ap, auc, _ = R.rank_metrics(s, t)
    m_ap, m_auc = np.nanmean(ap), np.nanmean(auc)
    assert out["n_valid"].tolist() == [int((~np.isnan(ap)).sum()), int((~np.isnan(auc)).sum())] == [C - 1, C - 2]
    assert abs(float(out["mAP"]) - m_ap) <= 1e-13 and abs(float(out["mAUC"]) - m_auc) <= 1e-13
    assert abs(float(out["d_prime"]) - R.d_prime(m_auc)) <= 1e-11
    with pytest.raises(ValueError):
        ev.add(sd[:, :3], td[:, :3])
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
    g = torch.Generator().manual_seed(seed)
    shape = (B or shape[0],) + tuple(shape[1:])
    xs = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    ts = [(torch.rand((shape[0], C), generator=g) < 0.3).float().to(dev) for _ in range(steps)]
    return xs, ts


def _pos_weight(C, dev):
    return torch.linspace(0.5, 20.0, C).to(dev)


def _cls_per_layer_step(m, x, t, pw, opt=None):
    """The per-layer path: the modules' forward (one autograd node per layer), ``ops.mlabel_loss`` in its autograd form."""
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        logits = m(x)
    assert type(logits.grad_fn).__name__ != "ClsFnBackward"
    loss, _, hits, dl = ops.mlabel_loss(logits, t, 1, pw, grad_scale=1.0)
    loss.backward()
    if opt is not None:
        opt.step()
    return logits.detach(), loss.detach(), hits, dl


def _probe_per_layer_step(m, x, t, pw, opt=None):
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        out = m(x)
    assert all(type(v.grad_fn).__name__ != "ProbeFnBackward" for v in out.values())
    res = [ops.mlabel_loss(v, t, 1, pw, grad_scale=1.0) for v in out.values()]
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


def _loss_against_float64(logits, t, pw, loss, hits, dl):
    """The step's loss, hits and dlogits against float64 on the step's OWN logits."""
    x, tn, pwn = _np(logits), _np(t), None if pw is None else _np(pw)
    assert _excess(float(loss), R.loss(x, tn, pwn), R.loss_bound(x, tn, pwn)) <= 1.0
    assert _excess(_np(dl), R.grad(x, tn, pwn), R.grad_bound(x, tn, pwn)) <= 1.0
    assert tuple(hits.tolist()) == R.hits(R.confidence(x, tn), tn)


@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("tower", ["video", "audio"])
def test_finetune_bce_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device, tower, C):
    from avid_hip import ops, parallel, plan
    dev = gpu_device
    shape = VIDEO if tower == "video" else AD.SMALL
    xs, ts = _batch(shape, C, dev, 31 + C, steps=2)
    pw = _pos_weight(C, dev) if C == 65 else None
    with _ungrouped():
        m1 = _video_model(dev, C) if tower == "video" else AD.cls_model(n_classes=C).to(dev).train()
        m2 = copy.deepcopy(m1)
        eng = parallel.FinetuneStep(m1, lr=1e-3, loss="bce", pos_weight=None if pw is None else pw.tolist())
        opt = parallel.Adam(list(m2.parameters()), lr=1e-3)
        for i in range(2):
            t_in = ts[i].bool() if i == 1 else ts[i]                     # bool targets are converted
            loss1, hits1 = eng.step(xs[i], t_in)
            pl = eng._step_plan
            assert pl.loss == "bce" and pl.fwd_prog[pl.n_fwd - 1].op == plan.OP_MLABEL_LOSS
            logits2, loss2, hits2, dl2 = _cls_per_layer_step(m2, xs[i], ts[i], pw, opt)
            torch.cuda.synchronize()
            assert loss1.dtype == torch.float32 and hits1.dtype == torch.int64 and hits1.shape == (2,)
            assert torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist(), i
            _same(m1, m2, ("grad",))
            _loss_against_float64(logits2, ts[i], pw, loss1, hits1, dl2)
    _same(m1, m2, ("param", "buffer"))
    ops.check_device_errors(dev)


@pytest.mark.parametrize("C", CLASSES)
def test_probe_bce_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device, C):
    from avid_hip import ops, parallel, plan
    dev = gpu_device
    xs, ts = _batch(AD.SMALL, C, dev, 41 + C, steps=2)
    pw = _pos_weight(C, dev) if C == 10 else None
    m1 = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    m2 = copy.deepcopy(m1)
    eng = parallel.ProbeStep(m1, lr=1e-3, loss="bce", pos_weight=pw)
    opt = parallel.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3)
    for i in range(2):
        losses1, hits1 = eng.step(xs[i], ts[i])
        pl = eng._step_plan
        assert [pl.fwd_prog[k].op for k in range(pl.n_logits, pl.n_fwd)] == [plan.OP_MLABEL_LOSS] * 4
        losses2, hits2 = _probe_per_layer_step(m2, xs[i], ts[i], pw, opt)
        torch.cuda.synchronize()
        assert losses1.shape == (4,) and hits1.shape == (4, 2)
        assert torch.equal(losses1, losses2) and torch.equal(hits1, hits2), i
        _same(m1, m2, ("grad",))
    _same(m1, m2, ("param", "buffer"))
    # the taps' losses of the last step against float64, on the per-layer path's own logits (the same bits as the programs')
    with _per_layer(), torch.no_grad():
        m3 = copy.deepcopy(m2)
        out = m3(xs[1])
    for i, v in enumerate(out.values()):
        l, _, h, d = ops.mlabel_loss(v, ts[1], 1, pw, grad_scale=1.0)
        _loss_against_float64(v, ts[1], pw, l, h, d)
    ops.check_device_errors(dev)


def _bce_shard(dev, kind, C, pw, **kw):
    import test_gpu_virtual_downstream as VD
    from avid_hip import parallel

    class BceShard(VD.Shard):
        def __init__(self):
            self.kind = kind
            if kind == "finetune":
                self.m = AD.cls_model(n_classes=C).to(dev).train()
                self.eng = parallel.FinetuneStep(self.m, loss="bce", pos_weight=pw, **kw)
            else:
                self.m = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
                self.eng = parallel.ProbeStep(self.m, loss="bce", pos_weight=pw, **kw)
    return VD, BceShard()


@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
def test_virtual_finetune_bce_step_is_the_two_shard_engines_sum(gpu_device, classifier_only):
    """tests/test_gpu_virtual_downstream.py's check: per shard the mean over b * C, the shards' gradients summed in rank order and
    applied with 1 / R, bit for bit the one-shard engines' results."""
    from avid_hip import ops, parallel
    dev, Rk, b, C = gpu_device, 2, 4, 65
    pw = _pos_weight(C, dev)
    VD, shard = _bce_shard(dev, "finetune", C, pw, classifier_only=classifier_only)
    xs, ts = _batch(AD.SMALL, C, dev, 51, steps=2, B=8)
    m = AD.cls_model(n_classes=C).to(dev).train()
    m.dropout.seed = VD.BASE_SEED
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, virtual_ranks=Rk, loss="bce", pos_weight=pw)
    n = eng.n_cls if classifier_only else eng.flat.numel
    VD._check_against_shards(eng, m, shard, xs, ts, Rk, b, n, seeds=VD._seeds(Rk))
    ops.check_device_errors(dev)


def test_virtual_probe_bce_step_is_the_two_shard_engines_sum(gpu_device):
    from avid_hip import ops, parallel
    dev, Rk, b, C = gpu_device, 2, 4, 10
    VD, shard = _bce_shard(dev, "probe", C, None)
    xs, ts = _batch(AD.SMALL, C, dev, 52, steps=2, B=8)
    m = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    eng = parallel.ProbeStep(m, virtual_ranks=Rk, loss="bce")
    VD._check_against_shards(eng, m, shard, xs, ts, Rk, b, eng.flat.numel)
    ops.check_device_errors(dev)


def test_classifier_only_bce_trains_the_classifier_alone(gpu_device):
    from avid_hip import ops, parallel
    dev, C = gpu_device, 10
    (x,), (t,) = _batch(VIDEO, C, dev, 61)
    m1 = _video_model(dev, C)
    m2 = copy.deepcopy(m1)
    before = {n: p.detach().clone() for n, p in m1.named_parameters()}
    eng = parallel.FinetuneStep(m1, lr=1e-3, classifier_only=True, loss="bce")
    loss1, hits1 = eng.step(x, t)
    _, loss2, hits2, _ = _cls_per_layer_step(m2, x, t, None)
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist()
    for n, p in m1.named_parameters():
        assert torch.equal(p, before[n]) == (not n.startswith("classifier.")), n
    g2 = dict(m2.named_parameters())
    for n in ("classifier.weight", "classifier.bias"):
        assert torch.equal(dict(m1.named_parameters())[n].grad, g2[n].grad), n
    _same(m1, m2, ("buffer",))
    ops.check_device_errors(dev)


def test_step_guard_skips_a_step_with_one_non_finite_target(gpu_device):
    from avid_hip import ops, parallel
    dev, C = gpu_device, 10
    xs, ts = _batch(AD.SMALL, C, dev, 71, steps=2)
    m = AD.cls_model(n_classes=C).to(dev).train()
    eng = parallel.FinetuneStep(m, lr=1e-3, loss="bce", skip_nonfinite=True)
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


def test_dense_evaluation_bce(gpu_device):
    """3 videos x 2 clips: the confidence is the clips' mean sigmoid of the eval-mode logits, the loss their BCE."""
    from avid_hip import ops, parallel
    dev, V, clips, C = gpu_device, 3, 2, 65
    g = torch.Generator().manual_seed(81)
    x = torch.randn((V, clips) + AD.SMALL[1:], generator=g).to(dev)
    t = (torch.rand((V, C), generator=g) < 0.3).float().to(dev)
    pw = _pos_weight(C, dev)
    m = AD.cls_model(n_classes=C).to(dev).train()
    conf, loss, hits = parallel.FinetuneStep(m, loss="bce", pos_weight=pw).evaluate(x, t, batch=4)      # chunks of 4 and 2 clips
    assert m.training and conf.shape == (V, C)
    logits = parallel.Inference(m)(x.flatten(0, 1))
    torch.cuda.synchronize()
    xn, tn, pwn = _np(logits), _np(t), _np(pw)
    assert _excess(float(loss), R.loss(xn, tn, pwn, clips), R.loss_bound(xn, tn, pwn, clips)) <= 1.0
    assert _excess(_np(conf), R.confidence(xn, tn, clips), R.confidence_bound(xn, tn, clips)) <= 1.0
    assert tuple(hits.tolist()) == R.hits(R.confidence(xn, tn, clips), tn)
    one = R.confidence(xn.reshape(V, clips, C).mean(1), tn, 1)          # the sigmoid of the mean logit is another number
    assert np.abs(one - R.confidence(xn, tn, clips)).max() > 100 * R.confidence_bound(xn, tn, clips).max()
    pm = AD.probe_model(AD.SMALL, n_classes=C).to(dev).train()
    confs, losses, hitss = parallel.ProbeStep(pm, loss="bce").evaluate(x, t.bool(), batch=4)
    assert pm.training and confs.shape == (4, V, C) and losses.shape == (4,) and hitss.shape == (4, 2)
    out = parallel.Inference(pm)(x.flatten(0, 1))
    for i, k in enumerate(AD.STAGES):
        xn = _np(out[k])
        assert _excess(float(losses[i]), R.loss(xn, tn, None, clips), R.loss_bound(xn, tn, None, clips)) <= 1.0, k
        assert _excess(_np(confs[i]), R.confidence(xn, tn, clips), R.confidence_bound(xn, tn, clips)) <= 1.0, k
    ops.check_device_errors(dev)


# ----------------------------------------------------------------------------------------------------------------------- 4. guards
def _guard_mlabel_loss(dev, P):
    from avid_hip import ops
    x, t, pw = R.loss_inputs(7, 3, 65, soft=True, with_pw=True)
    loss, conf, hits, dl = ops.mlabel_loss(P(_dev(x, dev)), P(_dev(t, dev)), 3, P(_dev(pw, dev)), grad_scale=1.0)
    return {"loss": loss, "conf": conf, "hits": hits, "dlogits": dl}


def _guard_rank_metrics(dev, P):
    from avid_hip import ops
    s, t = R.rank_inputs(1000, 65)
    s[500, 4] = 0.5
    ap, auc, n_pos = ops.rank_metrics(P(_dev(s, dev)), P(_dev(t, dev)))
    return {"ap": ap, "auc": auc, "n_pos": n_pos}


def _guard_finetune(dev, P):
    from avid_hip import parallel
    C = 65
    m = AD.cls_model(n_classes=C).to(dev).train()
    eng = parallel.FinetuneStep(m, loss="bce", pos_weight=_pos_weight(C, dev))
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
    eng = parallel.ProbeStep(m, loss="bce")
    (x,), (t,) = _batch(AD.ODD, C, dev, 92)
    losses, hits = eng.step(P(x), P(t))
    torch.cuda.synchronize()
    res = {"losses": losses, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat}
    res.update({f"buffer:{n}": b for n, b in m.named_buffers()})
    return res


@pytest.mark.parametrize("case", [_guard_mlabel_loss, _guard_rank_metrics, _guard_finetune, _guard_probe],
                         ids=["mlabel_loss", "rank_metrics", "finetune_step", "probe_step"])
def test_multilabel_ops_and_programs_under_guards(gpu_device, case):
    """tests/test_gpu_guards.py's rule: (a) no byte of any guard band changes, with every workspace sized exactly by its query,
    (b) every result is the same bits under both fills of unwritten memory, and the same as without guards."""
    from avid_hip import lib
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
        if case is _guard_rank_metrics:
            need = int(lib.raw("avid_rank_metrics_workspace_bytes")(1000, 65))
            assert [w[0] for w in g.workspaces] == [need] and need in g.size_values
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
