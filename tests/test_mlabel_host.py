"""Host side of multi-label fine-tuning and probing (no GPU): the float64 restatements of tests/_mlabel_ref.py against
scikit-learn and torch, the float32 error bounds of ``avid_mlabel_loss`` (a float32 restatement inside them, every named defect
at least ten times outside), the ``"bce"`` launch programs compiled dry, and what is refused before a launch."""
import math

import numpy as np
import pytest
import torch

import _mlabel_ref as R
import _audio_downstream as A

CPU = torch.device("cpu")


# ---- the metrics restatement against scikit-learn ---------------------------------------------------------------------------------
def _metric_cases():
    rng = np.random.default_rng(5)
    N = 257
    tied = np.round(rng.standard_normal(N), 1).astype(np.float32)
    lab = (rng.random(N) < 0.3)
    one = np.zeros(N, bool)
    one[17] = True
    zeros = np.where(rng.random(N) < 0.5, np.float32(0.0), np.float32(-0.0))
    infs = tied.copy()
    infs[::5], infs[1::7] = np.inf, -np.inf
    return {"tied": (tied, lab), "all_equal": (np.full(N, 0.25, np.float32), lab), "P=1": (tied, one), "P=N-1": (tied, ~one),
            "signed_zeros": (zeros, lab), "infinities": (infs, lab),
            "continuous": (rng.standard_normal(N).astype(np.float32), lab)}


@pytest.mark.parametrize("name", list(_metric_cases()))
def test_metrics_restatement_equals_scikit_learn(name):
    skm = pytest.importorskip("sklearn.metrics")
    s, lab = _metric_cases()[name]
    ap, auc, n_pos = R.rank_metrics(s[:, None], lab[:, None].astype(np.float32))
    # scikit-learn refuses infinities: their RANK is all the definitions read, so it is given any strictly monotone finite map
    s_sk = np.clip(s.astype(np.float64), -1e30, 1e30) if name == "infinities" else s.astype(np.float64)
    want_ap, want_auc = skm.average_precision_score(lab, s_sk), skm.roc_auc_score(lab, s_sk)
    P = int(lab.sum())
    assert n_pos[0] == P
    print(f"{name}: P {P} ap {ap[0]!r} (sklearn {want_ap!r}) auc {auc[0]!r} (sklearn {want_auc!r})")
    assert abs(ap[0] - want_ap) <= (2 * P + 8) * R.D
    # the restatement is one rounding of the exact rational; scikit-learn's trapezoid is held to it within one rounding of its own
    from fractions import Fraction
    tp, fp_ge, fp_gt = R._counts(s, lab)
    exact = Fraction(int((2 * ((len(s) - P) - fp_ge) + (fp_ge - fp_gt)).sum()), 2 * P * (len(s) - P))
    assert auc[0] == float(exact)
    assert abs(auc[0] - want_auc) <= 2 * R.D


def test_metrics_undefined_cases_are_nan():
    s = np.asarray([[0.1, 0.2, 0.3, np.nan], [0.4, 0.1, 0.2, 0.5], [0.3, 0.3, 0.9, 0.1]], np.float32)
    t = np.asarray([[0, 1, 1, 1], [0, 1, 0, 0], [0, 1, 1, 0]], np.float32)
    ap, auc, n_pos = R.rank_metrics(s, t)
    assert list(n_pos) == [0, 3, 2, 1]
    assert math.isnan(ap[0]) and math.isnan(auc[0])                    # P = 0
    assert ap[1] == 1.0 and math.isnan(auc[1])                         # Nn = 0
    assert ap[2] == 1.0 and auc[2] == 1.0
    assert math.isnan(ap[3]) and math.isnan(auc[3])                    # a NaN score


def test_metric_defects_are_outside_the_tolerance():
    """AUC without the half-credit for ties, AP on interpolated instead of step precision: each at least 10x outside."""
    s, lab = _metric_cases()["tied"]
    ap, auc, n_pos = R.rank_metrics(s[:, None], lab[:, None].astype(np.float32))
    P, Nn = int(lab.sum()), int((~lab).sum())
    tp, fp_ge, fp_gt = R._counts(s, lab)
    no_half = float((2 * (Nn - fp_ge)).sum()) / (2 * P * Nn)           # ties count nothing
    assert abs(no_half - auc[0]) >= 10 * 2 * R.D
    # interpolated precision: the best precision at any recall at least as high
    order = np.argsort(-s[lab], kind="stable")
    prec = (tp / (tp + fp_ge))[order]
    interp = np.maximum.accumulate(prec[::-1])[::-1]
    assert abs(float(interp.sum()) / P - ap[0]) >= 10 * (2 * P + 8) * R.D


# ---- the loss restatement against torch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_pw", [False, True])
@pytest.mark.parametrize("soft", [False, True])
def test_loss_restatement_equals_torch_float64(with_pw, soft):
    V, clips, C = 7, 3, 65
    x, t, pw = R.loss_inputs(V, clips, C, soft=soft, with_pw=with_pw)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    tt = torch.from_numpy(t).double().repeat_interleave(clips, 0)
    want = torch.nn.functional.binary_cross_entropy_with_logits(xt, tt, pos_weight=None if pw is None else torch.from_numpy(pw).double())
    want.backward()
    want = want.detach()
    got = R.loss(x, t, pw, clips)
    assert abs(got - float(want)) <= 8 * R.D * abs(float(want))
    g = R.grad(x, t, pw, clips)
    assert np.abs(g - xt.grad.numpy()).max() <= 1e-15 * np.abs(g).max()
    conf = torch.sigmoid(torch.from_numpy(x).double()).view(V, clips, C).mean(1).numpy()
    assert np.abs(R.confidence(x, t, clips) - conf).max() <= 4 * R.D


# ---- the float32 error bounds ---------------------------------------------------------------------------------------------------
def _f32_restatement(x, t, pw, clips, softplus="stable", use_pw=True, mean_over="all", conf="mean_sigmoid"):
    """mlabel_loss_kernel's arithmetic in numpy float32 (the element losses added in double, as the kernel does) — and, by its
    switches, the defects the bounds have to catch."""
    f = np.float32
    V, C = t.shape
    x3 = x.reshape(V, clips, C).astype(f)
    t3 = t[:, None, :].astype(f)
    pwv = np.ones(C, f) if (pw is None or not use_pw) else pw.astype(f)
    w = f(1) + (pwv - f(1))[None, None, :] * t3
    a = f(1) - t3
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(x3)).astype(f)
        sp = (np.log1p(e) + np.maximum(-x3, f(0))).astype(f) if softplus == "stable" else np.log(f(1) + np.exp(-x3).astype(f)).astype(f)
        l = (a * x3 + w * sp).astype(f)
        r = (f(1) / (f(1) + e)).astype(f)
        er = (e * r).astype(f)
        n = x3.size if mean_over == "all" else V * C
        loss = np.float32(l.astype(np.float64).sum() / n)
        dl = ((a - w * np.where(x3 >= 0, er, r)) * (f(1) / f(x3.size))).astype(f).reshape(-1, C)
        if conf == "mean_sigmoid":
            cf = (np.where(x3 >= 0, r, er).sum(1, dtype=f) / f(clips)).astype(f)
        else:                                                         # the sigmoid of the clip-mean logit
            m = x3.mean(1, dtype=f)
            cf = (f(1) / (f(1) + np.exp(-m).astype(f))).astype(f)
    return float(loss), dl, cf


def _excess(got, want, bound):
    """max |got - want| / bound (inf for a non-finite result)."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - want) / bound).max())


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_pw", [False, True])
def test_float32_restatement_is_inside_the_bounds(shape, with_pw):
    V, clips, C = shape
    x, t, pw = R.loss_inputs(V, clips, C, soft=(C % 2 == 1), with_pw=with_pw)
    loss, dl, cf = _f32_restatement(x, t, pw, clips)
    e_l = _excess(loss, R.loss(x, t, pw, clips), R.loss_bound(x, t, pw, clips))
    e_g = _excess(dl, R.grad(x, t, pw, clips), R.grad_bound(x, t, pw, clips))
    e_c = _excess(cf, R.confidence(x, t, clips), R.confidence_bound(x, t, clips))
    print(f"{shape} pw {with_pw}: loss {e_l:.3f} grad {e_g:.3f} conf {e_c:.3f} of the bound")
    assert e_l <= 1 and e_g <= 1 and e_c <= 1


def test_loss_defects_are_ten_times_outside_the_bounds():
    V, clips, C = 7, 3, 65
    x, t, pw = R.loss_inputs(V, clips, C, soft=False, with_pw=True)
    want_l, b_l = R.loss(x, t, pw, clips), R.loss_bound(x, t, pw, clips)
    want_c, b_c = R.confidence(x, t, clips), R.confidence_bound(x, t, clips)
    # naive log(1 + exp(-x)): exp overflows at x = -88.8 and -104 (the special logits lead the tensor)
    assert all(np.float32(v) in x.reshape(-1)[:8] for v in (88.8, -88.8, 104.0, -104.0))
    naive, _, _ = _f32_restatement(x, t, pw, clips, softplus="naive")
    assert _excess(naive, want_l, b_l) >= 10
    dropped, dl, _ = _f32_restatement(x, t, pw, clips, use_pw=False)
    assert _excess(dropped, want_l, b_l) >= 10
    assert _excess(dl, R.grad(x, t, pw, clips), R.grad_bound(x, t, pw, clips)) >= 10
    over_vc, _, _ = _f32_restatement(x, t, pw, clips, mean_over="VC")
    assert _excess(over_vc, want_l, b_l) >= 10
    _, _, cf = _f32_restatement(x, t, pw, clips, conf="sigmoid_of_mean")
    assert _excess(cf, want_c, b_c) >= 10


def test_tie_rule_of_the_hits():
    """Equal confidences: the lower class index is the top class; the opposite rule gives another count."""
    conf = np.asarray([[0.5, 0.7, 0.7, 0.1], [0.9, 0.9, 0.2, 0.9]])
    t = np.asarray([[0, 1, 0, 0], [0, 0, 0, 1]], np.float32)
    assert R.hits(conf, t) == (1, 4)
    higher = conf.shape[1] - 1 - np.argmax(conf[:, ::-1], axis=1)           # a tie broken to the higher index
    assert int((t[np.arange(2), higher] >= 0.5).sum()) == 1 and list(higher) == [2, 3] and list(np.argmax(conf, 1)) == [1, 0]
    t2 = np.asarray([[0, 0, 1, 0], [0, 0, 0, 1]], np.float32)               # positives at the HIGHER tied index only
    assert R.hits(conf, t2)[0] == 0 and int((t2[np.arange(2), higher] >= 0.5).sum()) == 2


# ---- plan compilation, dry ------------------------------------------------------------------------------------------------------
def _records(pl):
    return [pl.fwd_prog[k] for k in range(pl.n_fwd)], [pl.bwd_prog[k] for k in range(pl.n_bwd)]


def _same_record(a, b):
    return bytes(a) == bytes(b)


def test_bce_cls_plan_ends_in_the_mlabel_record_and_ce_is_unchanged():
    from avid_hip import plan
    m = A.cls_model(n_classes=65).train()
    pw = torch.ones(65)
    ce = plan.ClsPlan(m, A.SMALL, CPU, True, True, False)
    ce2 = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "ce", None)
    bce = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "bce", None)
    bcw = plan.ClsPlan(m, A.SMALL, CPU, True, True, False, "bce", pw)
    B = A.SMALL[0]
    for pl, has_pw in ((bce, False), (bcw, True)):
        fwd, bwd = _records(pl)
        assert pl.n_logits == pl.n_fwd - 1 and fwd[-1].op == plan.OP_MLABEL_LOSS == 33
        assert plan.OP_CLS_LOSS not in [r.op for r in fwd + bwd]
        r = fwd[-1]
        assert list(r.i)[:3] == [B, 1, 65] and r.f[0] == 1.0
        assert (r.t[0].slot, r.t[0].off) == tuple(pl.logits.ref)
        assert (r.t[1].slot, r.t[1].off) == (plan.S_LABELS, 0)
        assert (r.t[3].slot, r.t[3].off) == (plan.S_OUT, 0) and r.t[4].slot == -1
        assert (r.t[5].slot, r.t[5].off) == (plan.S_OUT, 8) and (r.t[6].slot, r.t[6].off) == (plan.S_DLOGITS, 0)
        assert r.t[7].slot >= plan.S_FIRST_TENSOR
        if has_pw:
            assert r.t[2].slot >= plan.S_FIRST_TENSOR and pl.tensors[r.t[2].slot - plan.S_FIRST_TENSOR] is pw
        else:
            assert r.t[2].slot == -1
        # everything in front of the loss record, and the whole backward, is the "ce" program's
        f_ce, b_ce = _records(ce)
        assert all(_same_record(a, b) for a, b in zip(fwd[:-1], f_ce[:-1])) and len(bwd) == len(b_ce)
    f1, b1 = _records(ce)
    f2, b2 = _records(ce2)
    assert len(f1) == len(f2) and all(_same_record(a, b) for a, b in zip(f1 + b1, f2 + b2))
    assert f1[-1].op == plan.OP_CLS_LOSS
    assert plan._OP_NAMES[33] == "mlabel_loss"


def test_bce_probe_plan_has_one_mlabel_record_per_tap():
    from avid_hip import plan
    m = A.probe_model(A.SMALL, n_classes=10).train()
    pw = torch.full((10,), 2.0)
    ce = plan.ProbePlan(m, A.SMALL, CPU, True, True)
    bce = plan.ProbePlan(m, A.SMALL, CPU, True, True, "bce", pw)
    B, n = A.SMALL[0], 4
    loss = [bce.fwd_prog[k] for k in range(bce.n_logits, bce.n_fwd)]
    assert [r.op for r in loss] == [plan.OP_MLABEL_LOSS] * n
    assert [(r.t[3].off, r.t[5].off, r.t[6].off) for r in loss] == [(32 * i, 32 * i + 8, 4 * B * 10 * i) for i in range(n)]
    assert all(r.t[1].slot == plan.S_LABELS and r.t[4].slot == -1 and bce.tensors[r.t[2].slot - plan.S_FIRST_TENSOR] is pw for r in loss)
    assert [(r.t[0].slot, r.t[0].off) for r in loss] == [tuple(lg.ref) for lg in bce.logits]
    assert [ce.fwd_prog[k].op for k in range(ce.n_logits, ce.n_fwd)] == [plan.OP_CLS_LOSS] * n
    assert ce.n_fwd == bce.n_fwd and ce.n_bwd == bce.n_bwd


def test_the_two_loss_kinds_do_not_share_a_cache_entry():
    from avid_hip import plan
    pw = torch.ones(5)
    assert plan._loss_key("ce", None) == ()                    # the "ce" key is the key of every plan compiled before
    keys = {plan._loss_key("ce", None), plan._loss_key("bce", None), plan._loss_key("bce", pw)}
    assert len(keys) == 3
    with pytest.raises(ValueError):
        plan._loss_kind("focal", None, 5)
    with pytest.raises(ValueError):
        plan._loss_kind("ce", pw, 5)
    with pytest.raises(ValueError):
        plan._loss_kind("bce", torch.ones(4), 5)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_ops_refuse_before_a_launch():
    from avid_hip import ops, lib, AvidHipError
    with pytest.raises(AvidHipError):
        ops.mlabel_loss(torch.zeros(2, 4), torch.zeros(2, 4))                       # CPU tensors: no fallback
    with pytest.raises(AvidHipError):
        ops.rank_metrics(torch.zeros(2, 4), torch.zeros(2, 4))
    x, t = torch.zeros(6, 4), torch.zeros(2, 4)
    for bad in ((x, torch.zeros(2, 5), 3, None), (x, t, 2, None), (x, t.long(), 3, None), (x.double(), t, 3, None),
                (x, t, 3, torch.ones(5)), (x, torch.zeros(2, dtype=torch.int64), 3, None)):
        with pytest.raises(AvidHipError):
            ops._mlabel_args(*bad)
    for s in ("avid_mlabel_loss", "avid_rank_metrics", "avid_rank_metrics_workspace_bytes"):
        assert s in lib.SIGNATURES
    assert lib.version() >= 167
    need = lib.raw("avid_rank_metrics_workspace_bytes")
    assert need(1, 1) > 0 and need(20371, 527) >= 8 * 20371 * 527 and need(0, 5) == 0 and need(1 << 31, 1) == 0
    assert lib.raw("avid_rank_metrics")(4, 2, None, None, None, None, None, None, 0, None, None) < 0
    assert lib.raw("avid_mlabel_loss")(2, 1, 1025, None, None, None, 1.0, None, None, None, None, None, None) < 0
    assert ops.DeviceErrors._MSG[16].startswith("mlabel_loss") and ops.DeviceErrors._MSG[32].startswith("rank_metrics")


class _Flat:
    class flat:
        device = CPU


def test_engines_refuse_wrong_targets():
    from avid_hip import parallel
    eng = parallel.AdamStep.__new__(parallel.FinetuneStep)
    eng.flat = _Flat()
    eng._set_loss("bce", [1.0, 2.0, 3.0], 3)
    assert eng.pos_weight.dtype == torch.float32 and eng.loss == "bce"
    x = torch.zeros(2, 1, 8, 8)
    v, t = eng._labelled(x, torch.tensor([[1, 0, 1], [0, 0, 1]], dtype=torch.bool))
    assert t.dtype == torch.float32 and t.tolist() == [[1.0, 0.0, 1.0], [0.0, 0.0, 1.0]]
    assert eng._labelled(x, torch.zeros(2, 3, dtype=torch.uint8))[1].dtype == torch.float32
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4), torch.zeros(3, 3), torch.zeros(2, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            eng._labelled(x, bad)
    with pytest.raises(ValueError):
        eng._set_loss("bce", [1.0, 2.0], 3)                    # pos_weight of the wrong length
    with pytest.raises(ValueError):
        eng._set_loss("ce", [1.0, 2.0, 3.0], 3)
    eng._set_loss("ce", None, 3)
    with pytest.raises(ValueError):
        eng._labelled(x, torch.zeros(2, 3))                    # "ce" still wants int64 [B]
    ev = parallel.MultiLabelEval(3)
    with pytest.raises(ValueError):
        ev.add(torch.zeros(2, 3), torch.zeros(2, 3))           # CPU tensors
    with pytest.raises(ValueError):
        ev.compute()
