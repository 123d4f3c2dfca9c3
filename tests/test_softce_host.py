"""Host side of soft-target fine-tuning (no GPU): torch's float32 cross-entropy against probabilities inside the float32 error
bounds of ``avid_soft_ce_loss`` (tests/_softce_ref.py) and every named defect at least ten times outside, the float32
restatement of ``avid_batch_mix`` against torch's expression bit for bit, ``GpuBatchMix``'s draws against a fake
``ops.batch_mix``, the ``"soft_ce"`` launch programs compiled dry, and what is refused before a launch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _softce_ref as R
import _audio_downstream as A

CPU = torch.device("cpu")
SHAPE = (6, 3, 65)                     # (V, clips, C) of the host checks: several clips, a column tail past one wave


def _excess(got, want, bound):
    """max |got - want| / bound (inf for a non-finite result)."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - want) / bound).max())


# ---- the restatement against torch, torch's float32 inside the bounds -------------------------------------------------------------
@pytest.mark.parametrize("kind", R.TARGET_KINDS)
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_restatement_equals_torch_float64_and_torch_float32_is_inside_the_bounds(kind, eps):
    V, clips, C = SHAPE
    x, t = R.loss_inputs(V, clips, C, kind)
    if kind == "unnorm":
        assert np.allclose(t.sum(1)[0::2], 0.7, atol=1e-6) and np.allclose(t.sum(1)[1::2], 1.3, atol=1e-6)
    want_l, want_g = R.loss(x, t, clips, eps), R.grad(x, t, clips, eps)
    for dtype in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        tt = torch.from_numpy(t).to(dtype).repeat_interleave(clips, 0)
        got = F.cross_entropy(xt, tt, label_smoothing=eps)
        got.backward()
        got = got.detach()
        if dtype == torch.float64:
            assert abs(float(got) - want_l) <= 1e-13 * max(abs(want_l), 1.0)
            assert np.abs(xt.grad.numpy() - want_g).max() <= 1e-15
            p = torch.softmax(torch.from_numpy(x).double(), 1).view(V, clips, C).mean(1).numpy()
            assert np.abs(R.confidence(x, t, clips) - p).max() <= 1e-15
        else:
            e_l = _excess(float(got), want_l, R.loss_bound(x, t, clips, eps))
            e_g = _excess(xt.grad.numpy(), want_g, R.grad_bound(x, t, clips, eps))
            p = torch.softmax(torch.from_numpy(x), 1).view(V, clips, C).mean(1).numpy()
            e_c = _excess(p, R.confidence(x, t, clips), R.confidence_bound(x, t, clips))
            print(f"{kind} eps {eps}: torch float32 loss {e_l:.3f} grad {e_g:.3f} conf {e_c:.3f} of the bound")
            assert e_l <= 1 and e_g <= 1 and e_c <= 1


def _f32_restatement(x, t, clips, eps, smooth=True, spread=True, s_is_one=False, mean_over="rows", conf="mean_softmax"):
    """soft_ce_loss_kernel's arithmetic in numpy float32 (the element losses added in double, as the kernel does) — and, by its
    switches, the defects the bounds have to catch."""
    f = np.float32
    V, C = t.shape
    x3 = x.reshape(V, clips, C).astype(f)
    e_ = f(eps if smooth else 0.0)
    tp = (t.astype(f) * (f(1) - e_) + (e_ / f(C) if spread else f(0))).astype(f)[:, None, :]
    m = x3.max(2, keepdims=True)
    e = np.exp((x3 - m).astype(f)).astype(f)
    den = e.sum(2, keepdims=True, dtype=f)
    lse = (np.log(den).astype(f) + m).astype(f)
    rows = V * clips
    n = rows if mean_over == "rows" else V
    loss = f((tp * (lse - x3).astype(f)).astype(f).astype(np.float64).sum() / n)
    p = (e * (f(1) / den).astype(f)).astype(f)
    S = f(1) if s_is_one else tp.sum(2, keepdims=True, dtype=f)
    dl = (((p * S).astype(f) - tp).astype(f) * (f(1) / f(rows))).astype(f).reshape(-1, C)
    if conf == "mean_softmax":
        cf = (p.sum(1, dtype=f) * (f(1) / f(clips))).astype(f)
    else:                                                             # the softmax of the clip-mean logits
        xm = x3.mean(1, dtype=f)
        em = np.exp(xm - xm.max(1, keepdims=True)).astype(f)
        cf = (em / em.sum(1, keepdims=True, dtype=f)).astype(f)
    return float(loss), dl, cf


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", R.TARGET_KINDS)
def test_float32_restatement_is_inside_the_bounds(shape, kind):
    V, clips, C = shape
    x, t = R.loss_inputs(V, clips, C, kind)
    for eps in (0.0, 0.1):
        loss, dl, cf = _f32_restatement(x, t, clips, eps)
        e_l = _excess(loss, R.loss(x, t, clips, eps), R.loss_bound(x, t, clips, eps))
        e_g = _excess(dl, R.grad(x, t, clips, eps), R.grad_bound(x, t, clips, eps))
        e_c = _excess(cf, R.confidence(x, t, clips), R.confidence_bound(x, t, clips))
        print(f"{shape} {kind} eps {eps}: loss {e_l:.3f} grad {e_g:.3f} conf {e_c:.3f} of the bound")
        assert e_l <= 1 and e_g <= 1 and e_c <= 1


def test_defects_are_ten_times_outside_the_bounds():
    V, clips, C = SHAPE
    eps = 0.1
    x, t = R.loss_inputs(V, clips, C, "unnorm")
    want_l, b_l = R.loss(x, t, clips, eps), R.loss_bound(x, t, clips, eps)
    want_g, b_g = R.grad(x, t, clips, eps), R.grad_bound(x, t, clips, eps)
    want_c, b_c = R.confidence(x, t, clips), R.confidence_bound(x, t, clips)
    sane, dl, cf = _f32_restatement(x, t, clips, eps)
    assert _excess(sane, want_l, b_l) <= 1 and _excess(dl, want_g, b_g) <= 1 and _excess(cf, want_c, b_c) <= 1
    out = {}
    l, dl, _ = _f32_restatement(x, t, clips, eps, smooth=False)
    out["smoothing ignored"] = min(_excess(l, want_l, b_l), _excess(dl, want_g, b_g))
    l, dl, _ = _f32_restatement(x, t, clips, eps, spread=False)
    out["eps / C dropped"] = min(_excess(l, want_l, b_l), _excess(dl, want_g, b_g))
    _, dl, _ = _f32_restatement(x, t, clips, eps, s_is_one=True)
    out["S taken as 1"] = _excess(dl, want_g, b_g)
    l, _, _ = _f32_restatement(x, t, clips, eps, mean_over="V")
    out["mean over V"] = _excess(l, want_l, b_l)
    _, _, cf = _f32_restatement(x, t, clips, eps, conf="softmax_of_mean")
    out["softmax of the mean logits"] = _excess(cf, want_c, b_c)
    print(out)
    assert all(v >= 10 for v in out.values()), out


def test_hits_tie_rules():
    """Equal targets: the lower class index is the label.  Equal confidences: the lower index ranks first."""
    conf = np.asarray([[0.1, 0.4, 0.4, 0.1], [0.3, 0.3, 0.2, 0.2]])
    t = np.asarray([[0.0, 0.5, 0.5, 0.0], [0.0, 0.5, 0.5, 0.0]], np.float32)       # label 1 in both rows
    assert R.hits(conf, t) == (1, 2)             # row 0: class 1 wins its tie with 2; row 1: class 0 ties with 1 and ranks first
    t2 = np.asarray([[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]], np.float32)
    assert R.hits(conf, t2) == (1, 2)            # row 0: label 2 is behind its equal at index 1
    six = np.full((1, 6), 1.0 / 6)
    assert R.hits(six, np.eye(6, dtype=np.float32)[[5]]) == (0, 0) and R.hits(six, np.eye(6, dtype=np.float32)[[4]]) == (0, 1)


# ---- the mix restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_restatement_equals_torch_float32_bit_for_bit(shape):
    x = R.mix_inputs(shape)
    B = shape[0]
    xt = torch.from_numpy(x)
    seen_fma = False
    for name, perm in R.perms(B).items():
        for lam in ([0.0] * B, [1.0] * B, [0.5] * B, [R.LONG_LAM] * B, list(np.linspace(0.1, 0.9, B).astype(np.float32))):
            lt = torch.tensor(lam, dtype=torch.float32).view(-1, 1, 1, 1, 1)
            want = lt * xt + (1 - lt) * xt[torch.from_numpy(perm)]
            got = R.mixup(x, perm, lam)
            assert got.tobytes() == want.numpy().tobytes(), (name, lam[0])
            seen_fma = seen_fma or R.mixup_fma(x, perm, lam).tobytes() != got.tobytes()
    # a contracted fma differs somewhere on this input (one element only: nothing to round twice)
    assert seen_fma or x.size <= 3
    t = torch.rand(B, 7)
    perm = R.perms(B)["cycle"]
    lam = torch.full((B,), R.LONG_LAM)
    want_t = lam[:, None] * t + (1 - lam[:, None]) * t[torch.from_numpy(perm)]
    assert R.mix_targets(t.numpy(), perm, lam.numpy()).tobytes() == want_t.numpy().tobytes()


def test_cutmix_restatement_and_boxes():
    x = R.mix_inputs(R.MIX_SHAPES[1])
    B, _, _, H, W = x.shape
    perm = R.perms(B)["cycle"]
    for name, bx in R.boxes(H, W).items():
        h0, h1, w0, w1 = bx
        assert 0 <= h0 <= h1 <= H and 0 <= w0 <= w1 <= W, name
        y = R.cutmix(x, perm, [bx] * B)
        inside = np.zeros((H, W), bool)
        inside[h0:h1, w0:w1] = True
        assert np.array_equal(y[..., inside], x[perm][..., inside]) and np.array_equal(y[..., ~inside], x[..., ~inside]), name
    assert np.array_equal(R.one_hot([2, -1, 7, 0], 7), np.eye(8, 7, dtype=np.float32)[[2, 7, 7, 0]])


# ---- GpuBatchMix's draws, with a fake ops.batch_mix -------------------------------------------------------------------------------------
class _FakeMix:
    def __init__(self):
        self.calls = []

    def __call__(self, x, perm, lam, box=None, labels=None, targets=None, n_classes=None):
        self.calls.append(dict(perm=perm.numpy().copy(), lam=lam.numpy().copy(), box=None if box is None else box.numpy().copy(),
                               labels=labels, targets=targets, n_classes=n_classes))
        return x.clone(), torch.zeros(x.shape[0], n_classes)


@pytest.fixture
def fake_mix(monkeypatch):
    from avid_hip import ops
    fake = _FakeMix()
    monkeypatch.setattr(ops, "batch_mix", fake)
    return fake


def test_sampler_draw_order(fake_mix):
    """The documented order: apply, switch, lam, perm, then the box centres (rows, then columns)."""
    from datasets.gpu_mix import GpuBatchMix
    B, H, W = 6, 20, 33
    x, lab = torch.zeros(B, 1, H, W), torch.arange(B)
    for per_sample in (False, True):
        s = GpuBatchMix(10, mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7, switch_prob=0.5, per_sample=per_sample, seed=11)
        rng = np.random.Generator(np.random.PCG64(11))
        modes = set()
        for _ in range(40):
            y, t = s(x, lab)
            assert y is not x and t.shape == (B, 10)
            call = fake_mix.calls[-1]
            k = B if per_sample else 1
            if not rng.random() < 0.7:
                mode, perm, lam, box = None, np.arange(B), np.ones(B, np.float32), np.zeros((B, 4), np.int32)
            else:
                cut = rng.random() < 0.5
                lam64 = rng.beta(1.0 if cut else 0.8, 1.0 if cut else 0.8, size=k)
                perm = rng.permutation(B)
                mode, box = "cutmix" if cut else "mixup", None
                if cut:
                    cy, cx = rng.integers(H, size=k), rng.integers(W, size=k)
                    r = np.sqrt(1.0 - lam64)
                    ch, cw = (H * r).astype(np.int64), (W * r).astype(np.int64)
                    h0, h1 = np.clip(cy - ch // 2, 0, H), np.clip(cy - ch // 2 + ch, 0, H)
                    w0, w1 = np.clip(cx - cw // 2, 0, W), np.clip(cx - cw // 2 + cw, 0, W)
                    box = np.broadcast_to(np.stack([h0, h1, w0, w1], 1), (B, 4)).astype(np.int32)
                    lam64 = 1.0 - (h1 - h0) * (w1 - w0) / float(H * W)          # recomputed from the clipped box
                lam = np.broadcast_to(lam64.astype(np.float32), (B,))
            modes.add(mode)
            assert s.last[0] == mode and np.array_equal(call["perm"], perm) and np.array_equal(call["lam"], lam)
            assert call["perm"].dtype == np.int64 and call["lam"].dtype == np.float32
            if mode == "mixup":
                assert call["box"] is None
            else:
                assert call["box"].dtype == np.int32 and np.array_equal(call["box"], box)
                bx = call["box"]
                assert (0 <= bx[:, 0]).all() and (bx[:, 0] <= bx[:, 1]).all() and (bx[:, 1] <= H).all()
                assert (0 <= bx[:, 2]).all() and (bx[:, 2] <= bx[:, 3]).all() and (bx[:, 3] <= W).all()
                area = (bx[:, 1] - bx[:, 0]) * (bx[:, 3] - bx[:, 2])
                assert np.array_equal(call["lam"], (1.0 - area / float(H * W)).astype(np.float32))
            if mode is None:                          # identity: lam 1, every sample its own partner, empty boxes
                assert (call["lam"] == 1).all() and np.array_equal(call["perm"], np.arange(B)) and not call["box"].any()
            assert call["labels"] is lab and call["targets"] is None and call["n_classes"] == 10
        assert modes == {None, "mixup", "cutmix"}


def test_sampler_clipped_boxes_lower_the_mixed_share(fake_mix):
    """A box that is clipped covers less than 1 - lam of the plane: the recomputed lam is the drawn one or larger."""
    from datasets.gpu_mix import GpuBatchMix
    s = GpuBatchMix(4, cutmix_alpha=1.0, per_sample=True, seed=3)
    rng = np.random.Generator(np.random.PCG64(3))
    x = torch.zeros(64, 3, 2, 16, 24)
    s(x, torch.zeros(64, 4))
    rng.random()
    drawn = rng.beta(1.0, 1.0, size=64)
    lam, box = fake_mix.calls[-1]["lam"], fake_mix.calls[-1]["box"]
    assert (lam >= drawn.astype(np.float32) - 1e-6).all() and (lam > drawn + 0.01).any()
    assert fake_mix.calls[-1]["targets"] is not None and fake_mix.calls[-1]["labels"] is None


def test_sampler_state_and_seed(fake_mix):
    from datasets.gpu_mix import GpuBatchMix
    x, lab = torch.zeros(5, 3, 2, 8, 8), torch.arange(5)

    def run(s, n):
        out = []
        for _ in range(n):
            s(x, lab)
            c = fake_mix.calls[-1]
            out.append((c["perm"].tobytes(), c["lam"].tobytes(), None if c["box"] is None else c["box"].tobytes()))
        return out
    kw = dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=0.9, seed=5)
    a, b = GpuBatchMix(7, **kw), GpuBatchMix(7, **kw)
    first = run(a, 6)
    assert run(b, 6) == first                                  # the same seed: the same sequence
    assert run(GpuBatchMix(7, **{**kw, "seed": 6}), 6) != first
    sd = a.state_dict()
    nxt = run(a, 5)
    c = GpuBatchMix(7, **{**kw, "seed": 99})
    c.load_state_dict(sd)
    assert run(c, 5) == nxt                                    # a restored sampler continues the sequence
    off = GpuBatchMix(7, seed=1)                               # both alphas 0: never mixed
    off(x, lab)
    assert off.last[0] is None
    for bad in (dict(n_classes=0), dict(n_classes=3, mixup_alpha=-1.0), dict(n_classes=3, prob=1.5), dict(n_classes=3, switch_prob=-0.1)):
        with pytest.raises(ValueError):
            GpuBatchMix(**bad)
    with pytest.raises(ValueError):
        a(x, torch.zeros(5, 6))                                # targets of another width
    with pytest.raises(ValueError):
        a(torch.zeros(5, 8), lab)


# ---- plan compilation, dry ------------------------------------------------------------------------------------------------------
def _records(pl):
    return [pl.fwd_prog[k] for k in range(pl.n_fwd)], [pl.bwd_prog[k] for k in range(pl.n_bwd)]


def _same(a, b):
    return len(a) == len(b) and all(bytes(p) == bytes(q) for p, q in zip(a, b))


def test_soft_ce_cls_plan_ends_in_record_34_and_the_others_are_unchanged():
    from avid_hip import plan
    m = A.cls_model(n_classes=65).train()
    pw = torch.ones(65)
    ce = plan.ClsPlan(m, A.SMALL, CPU, True, True, False)
    ce2 = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "ce", None, 0.0)
    bce = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "bce", pw)
    bce2 = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "bce", pw, 0.0)
    f_ce, b_ce = _records(ce)
    assert _same(f_ce + b_ce, sum(_records(ce2), [])) and f_ce[-1].op == plan.OP_CLS_LOSS
    assert _same(sum(_records(bce), []), sum(_records(bce2), [])) and _records(bce)[0][-1].op == plan.OP_MLABEL_LOSS
    B = A.SMALL[0]
    for eps in (0.0, 0.1):
        pl = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "soft_ce", None, eps)
        fwd, bwd = _records(pl)
        assert pl.loss == "soft_ce" and pl.label_smoothing == eps
        assert pl.n_logits == pl.n_fwd - 1 and fwd[-1].op == plan.OP_SOFT_CE_LOSS == 34
        assert not {plan.OP_CLS_LOSS, plan.OP_MLABEL_LOSS} & {r.op for r in fwd + bwd}
        r = fwd[-1]
        assert list(r.i)[:3] == [B, 1, 65] and r.f[0] == 1.0 and r.f[1] == np.float32(eps)
        assert (r.t[0].slot, r.t[0].off) == tuple(pl.logits.ref)
        assert (r.t[1].slot, r.t[1].off) == (plan.S_LABELS, 0)
        assert (r.t[2].slot, r.t[2].off) == (plan.S_OUT, 0) and r.t[3].slot == -1
        assert (r.t[4].slot, r.t[4].off) == (plan.S_OUT, 8) and (r.t[5].slot, r.t[5].off) == (plan.S_DLOGITS, 0)
        assert r.t[6].slot >= plan.S_FIRST_TENSOR
        # everything in front of the loss record, and the whole backward, is the "ce" program's
        assert _same(fwd[:-1], f_ce[:-1]) and _same(bwd, b_ce)
    assert plan._OP_NAMES[34] == "soft_ce_loss"


def test_soft_ce_probe_plan_has_one_record_34_per_tap():
    from avid_hip import plan
    m = A.probe_model(A.SMALL, n_classes=10).train()
    ce = plan.ProbePlan(m, A.SMALL, CPU, True, True)
    ce2 = plan.ProbePlan(m, A.SMALL, CPU, True, True, "ce", None, 0.0)
    sc = plan.ProbePlan(m, A.SMALL, CPU, True, True, "soft_ce", None, 0.1)
    B, n = A.SMALL[0], 4
    loss = [sc.fwd_prog[k] for k in range(sc.n_logits, sc.n_fwd)]
    assert [r.op for r in loss] == [plan.OP_SOFT_CE_LOSS] * n
    assert [(r.t[2].off, r.t[4].off, r.t[5].off) for r in loss] == [(32 * i, 32 * i + 8, 4 * B * 10 * i) for i in range(n)]
    assert all(r.t[1].slot == plan.S_LABELS and r.t[3].slot == -1 and r.f[1] == np.float32(0.1) for r in loss)
    assert [(r.t[0].slot, r.t[0].off) for r in loss] == [tuple(lg.ref) for lg in sc.logits]
    assert _same(sum(_records(ce), []), sum(_records(ce2), []))
    assert [ce.fwd_prog[k].op for k in range(ce.n_logits, ce.n_fwd)] == [plan.OP_CLS_LOSS] * n
    assert ce.n_fwd == sc.n_fwd and ce.n_bwd == sc.n_bwd


def test_cache_keys():
    from avid_hip import plan
    pw = torch.ones(5)
    # "ce" and "bce": the keys of every plan compiled before, with and without the new argument at its default
    assert plan._loss_key("ce", None) == plan._loss_key("ce", None, 0.0) == ()
    assert plan._loss_key("bce", None) == plan._loss_key("bce", None, 0.0) == ("bce", None)
    assert plan._loss_key("bce", pw) == plan._loss_key("bce", pw, 0.0) == ("bce", id(pw))
    keys = {plan._loss_key("ce", None), plan._loss_key("bce", None), plan._loss_key("soft_ce", None, 0.0),
            plan._loss_key("soft_ce", None, 0.1), plan._loss_key("soft_ce", None, 0.2)}
    assert len(keys) == 5                                      # the smoothing is part of the key
    assert plan._loss_kind("soft_ce", None, 5, 0.1) == "soft_ce" and plan._loss_kind("ce", None, 5) == "ce"
    for bad in (("soft_ce", None, 5, 1.0), ("soft_ce", None, 5, -0.1), ("soft_ce", None, 5, float("nan")), ("ce", None, 5, 0.1),
                ("bce", None, 5, 0.1), ("soft_ce", pw, 5, 0.0), ("focal", None, 5, 0.0), ("soft_ce", None, 5, "0.1")):
        with pytest.raises(ValueError):
            plan._loss_kind(*bad)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_ops_refuse_before_a_launch():
    from avid_hip import ops, lib, AvidHipError
    with pytest.raises(AvidHipError):
        ops.soft_ce_loss(torch.zeros(2, 4), torch.zeros(2, 4))                      # CPU tensors: no fallback
    x, t = torch.zeros(6, 4), torch.zeros(2, 4)
    for bad in ((x, torch.zeros(2, 5), 3, 0.0), (x, t, 2, 0.0), (x, t.long(), 3, 0.0), (x.double(), t, 3, 0.0),
                (x, torch.zeros(2, dtype=torch.int64), 3, 0.0), (x, t, 3, 1.0), (x, t, 3, -0.01), (x, t, 3, float("nan")),
                (x, t, 0, 0.0), (torch.zeros(2, 1025), torch.zeros(2, 1025), 1, 0.0)):
        with pytest.raises(AvidHipError):
            ops._soft_ce_args(*bad)
    clip = torch.zeros(4, 3, 2, 8, 8)
    perm, lam = torch.arange(4), torch.ones(4)
    with pytest.raises(AvidHipError):
        ops.batch_mix(clip, perm, lam)                                              # CPU tensors: no fallback
    with pytest.raises(AvidHipError):
        ops.one_hot(torch.arange(4), 5)
    for s in ("avid_soft_ce_loss", "avid_batch_mix"):
        assert s in lib.SIGNATURES
    assert lib.version() >= 168
    raw = lib.raw("avid_soft_ce_loss")
    assert raw(2, 1, 1025, None, None, 0.0, 1.0, None, None, None, None, None, None) < 0
    assert raw(0, 1, 4, None, None, 0.0, 1.0, None, None, None, None, None, None) < 0
    mix = lib.raw("avid_batch_mix")
    assert mix(2, 4, 3, 2, 8, 8, None, None, None, None, None, 0, None, None, None, None, None) < 0     # no such mode
    assert mix(0, 4, 3, 2, 8, 8, None, None, None, None, None, 0, None, None, None, None, None) < 0     # nothing to do
    assert ops.DeviceErrors._MSG[64].startswith("soft_ce_loss") and ops.DeviceErrors._MSG[128].startswith("batch_mix")
    assert issubclass(ops.TargetError, ValueError)


class _Flat:
    class flat:
        device = CPU


def test_engines_refuse_wrong_arguments():
    from avid_hip import parallel
    eng = parallel.AdamStep.__new__(parallel.FinetuneStep)
    eng.flat = _Flat()
    eng._set_loss("soft_ce", None, 3, 0.1)
    assert eng.loss == "soft_ce" and eng.label_smoothing == 0.1 and eng.pos_weight is None and eng.n_classes == 3
    x = torch.zeros(2, 1, 8, 8)
    v, t = eng._labelled(x, torch.tensor([[0.25, 0.75, 0.0], [0.0, 0.0, 1.0]]))
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3)
    for bad in (torch.zeros(2, 4), torch.zeros(3, 3), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, dtype=torch.int64),
                torch.zeros(2, 3, dtype=torch.bool), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError):
            eng._labelled(x, bad)
    for bad in (("ce", None, 3, 0.1), ("bce", None, 3, 0.1), ("soft_ce", [1.0, 1.0, 1.0], 3, 0.0), ("soft_ce", None, 3, 1.0),
                ("soft_ce", None, None, 0.0)):
        with pytest.raises(ValueError):
            eng._set_loss(*bad)
    eng._set_loss("ce", None, 3)                               # the defaults: as before
    assert eng.loss == "ce" and eng.label_smoothing == 0.0
    with pytest.raises(ValueError):
        eng._labelled(x, torch.zeros(2, 3))                    # "ce" still wants int64 [B]
    # the constructors take the arguments and refuse the same
    import inspect
    for cls in (parallel.FinetuneStep, parallel.ProbeStep):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["loss"].default == "ce" and sig["label_smoothing"].default == 0.0
