"""Linear-probe evaluation (MOSTModel) on the GPU: the heads' kernels against torch / float64, the module's two paths against
each other and against the reference-generated fixture, and the step engine against the torch loop the reference runs
(eval-action-recg-linear.py: summed cross-entropy over the taps, Adam over model.parameters(), lr 1e-4, weight decay 0)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 6e-7          # rms(err) / rms(output) against float64: the project's bar (tests/test_gpu_precision.py)

SHIPPED = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
               pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                            "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)


def rms_rel(got, want64):
    want64 = want64.double().cpu()
    return float(((got.double().cpu() - want64) ** 2).mean().sqrt() / ((want64 ** 2).mean().sqrt() + 1e-300))


def max_rel(got, want64):
    want64 = want64.double().cpu()
    return float((got.double().cpu() - want64).abs().max() / (want64.abs().max() + 1e-300))


# ------------------------------------------------------------------------------------------------------------------ pool
# (C, T, H, W), output size: the four taps at 224 x 224 clips, the same at 64 x 64 (two of them pool to MORE outputs than
# positions), a pooled time axis, and odd sizes
POOL_CASES = [((64, 8, 56, 56), (1, 12, 12)), ((128, 4, 28, 28), (1, 8, 8)), ((256, 2, 14, 14), (1, 6, 6)),
              ((512, 1, 7, 7), (1, 4, 4)), ((64, 8, 16, 16), (1, 12, 12)), ((128, 4, 8, 8), (1, 8, 8)),
              ((256, 2, 4, 4), (1, 6, 6)), ((512, 1, 2, 2), (1, 4, 4)), ((64, 8, 16, 16), (2, 3, 5)), ((512, 1, 2, 2), (2, 4, 4)),
              ((5, 3, 7, 9), (2, 3, 4))]


@pytest.mark.parametrize("shape,out", POOL_CASES, ids=[f"{s}->{o}".replace(" ", "") for s, o in POOL_CASES])
def test_adaptive_maxpool_equals_torch(gpu_device, shape, out):
    from avid_hip import ops
    Cc, T, H, W = shape
    B = 2 if H > 16 else 3
    g = torch.Generator().manual_seed(Cc + H)
    x = torch.randn((B, T, H, W, Cc), generator=g).to(gpu_device)
    y = ops.adaptive_maxpool(x, out)
    ref = nn.AdaptiveMaxPool3d(out)(x.permute(0, 4, 1, 2, 3)).reshape(B, -1)
    assert y.shape == ref.shape and torch.equal(y, ref)


def test_adaptive_maxpool_full_size_tap_and_nan(gpu_device):
    from avid_hip import ops
    g = torch.Generator().manual_seed(8)
    x = torch.randn((8, 8, 56, 56, 64), generator=g).to(gpu_device)
    y = ops.adaptive_maxpool(x, (1, 12, 12))
    ref = nn.AdaptiveMaxPool3d((1, 12, 12))(x.permute(0, 4, 1, 2, 3)).reshape(8, -1)
    assert torch.equal(y, ref)
    assert torch.equal(y, ops.adaptive_maxpool(x, (1, 12, 12)))
    x[1, 3, 20, 20, 5] = float("nan")                      # a NaN owns its windows, as in torch
    y = ops.adaptive_maxpool(x, (1, 12, 12))
    ref = nn.AdaptiveMaxPool3d((1, 12, 12))(x.permute(0, 4, 1, 2, 3)).reshape(8, -1)
    assert torch.equal(torch.isnan(y), torch.isnan(ref)) and int(torch.isnan(y).sum()) >= 1
    with pytest.raises(ops.AvidHipError):
        ops.adaptive_maxpool(x.permute(0, 4, 1, 2, 3), (1, 12, 12))          # not channels-last memory


# ------------------------------------------------------------------------------------------------------------------ BatchNorm1d
@pytest.mark.parametrize("B,Fd", [(128, 9216), (128, 8192), (2, 4), (5, 100)])
def test_bn1d_against_float64(gpu_device, B, Fd):
    from avid_hip import ops
    dev = gpu_device
    g = torch.Generator().manual_seed(B * 7 + Fd)
    x = torch.randn((B, Fd), generator=g).abs() * 1.3 + 0.2          # pooled ReLU outputs: positive, off zero
    gy = torch.randn((B, Fd), generator=g)
    gamma, beta = torch.rand(Fd, generator=g) + 0.5, torch.randn(Fd, generator=g) * 0.3
    rm0, rv0 = torch.randn(Fd, generator=g) * 0.1, torch.rand(Fd, generator=g) + 0.5

    def torch_bn(dtype):
        bn = nn.BatchNorm1d(Fd).to(dtype)
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
        xi = x.clone().to(dtype).requires_grad_(True)
        y = bn.train()(xi)
        y.backward(gy.to(dtype))
        ye = bn.eval()(x.to(dtype)).detach()
        return {"y": y.detach(), "dx": xi.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
                "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(), "y_eval": ye}

    r64, r32 = torch_bn(torch.float64), torch_bn(torch.float32)
    xd = x.to(dev).requires_grad_(True)
    gd, bd = gamma.to(dev).requires_grad_(True), beta.to(dev).requires_grad_(True)
    rm, rv, cnt = rm0.to(dev), rv0.to(dev), torch.tensor(3, dtype=torch.int64, device=dev)
    y = ops.bn1d(xd, gd, bd, rm, rv, True, 0.1, 1e-5, cnt)
    y.backward(gy.to(dev))
    assert int(cnt) == 4
    ye = ops.bn1d(x.to(dev), gd.detach(), bd.detach(), rm, rv, False, 0.1, 1e-5)
    got = {"y": y.detach(), "dx": xd.grad, "dgamma": gd.grad, "dbeta": bd.grad, "running_mean": rm, "running_var": rv, "y_eval": ye}
    rep = {k: (rms_rel(got[k], r64[k]), rms_rel(r32[k], r64[k])) for k in got}
    print(f"\n[bn1d] ({B}, {Fd}): " + ", ".join(f"{k} {a:.2e} (torch float32 {b:.2e})" for k, (a, b) in rep.items()))
    for k, (e, _) in rep.items():
        assert e <= BAR, (k, e)
    # a second run gives the same bits, and the frozen (eval-mode) backward is gamma * invstd * dy
    rm2, rv2 = rm0.to(dev), rv0.to(dev)
    assert torch.equal(ops.bn1d(x.to(dev), gd.detach(), bd.detach(), rm2, rv2, True, 0.1, 1e-5), y)
    xe = x.to(dev).requires_grad_(True)
    ops.bn1d(xe, gd.detach(), bd.detach(), rm, rv, False, 0.1, 1e-5).backward(gy.to(dev))
    want = gy.double() * (gamma.double() / torch.sqrt(rv.double().cpu() + 1e-5))
    assert rms_rel(xe.grad, want) <= BAR


def test_bn1d_needs_two_rows_in_training(gpu_device):
    from avid_hip import ops
    x = torch.randn(1, 8, device=gpu_device)
    one, zero = torch.ones(8, device=gpu_device), torch.zeros(8, device=gpu_device)
    with pytest.raises(ValueError):
        ops.bn1d(x, one, zero, zero.clone(), one.clone(), True)
    assert ops.bn1d(x, one, zero, zero.clone(), one.clone(), False).shape == (1, 8)


# ------------------------------------------------------------------------------------------------------------------ Linear
@pytest.mark.parametrize("B,Fin,C", [(128, 9216, 400), (128, 8192, 400), (3, 100, 7), (256, 16384, 1000)])
def test_probe_linear_against_float64(gpu_device, kernel_log, B, Fin, C):
    from avid_hip import ops
    dev = gpu_device
    g = torch.Generator().manual_seed(B + Fin + C)
    x, gy = torch.randn((B, Fin), generator=g), torch.randn((B, C), generator=g)
    w = (torch.rand((C, Fin), generator=g) * 2 - 1) / Fin ** 0.5
    b = (torch.rand(C, generator=g) * 2 - 1) / Fin ** 0.5

    def torch_linear(dtype):
        xi, wi, bi = (t.clone().to(dtype).requires_grad_(True) for t in (x, w, b))
        y = F.linear(xi, wi, bi)
        y.backward(gy.to(dtype))
        return {"y": y.detach(), "dw": wi.grad, "db": bi.grad, "dx": xi.grad}

    r64, r32 = torch_linear(torch.float64), torch_linear(torch.float32)

    def run():
        xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
        y = ops.probe_linear(xd, wd, bd)
        y.backward(gy.to(dev))
        return {"y": y.detach(), "dw": wd.grad, "db": bd.grad, "dx": xd.grad}

    with kernel_log() as log:
        got = run()
    assert log.launches("probe_gemm_kernel") == 3 and log.launches("cls_linear") == 0, sorted(log.report)
    again = run()
    for k in got:
        assert torch.equal(got[k], again[k]), k                     # bit-reproducible: fixed summation order, no atomics
    rep = {k: (rms_rel(got[k], r64[k]), rms_rel(r32[k], r64[k]), max_rel(got[k], r64[k])) for k in got}
    print(f"\n[probe_linear] ({B}, {Fin}, {C}): " +
          ", ".join(f"{k} rms {a:.2e} (float32 F.linear {b:.2e}) max {m:.2e}" for k, (a, b, m) in rep.items()))
    for k, (e, e32, m) in rep.items():
        assert e <= BAR, (k, e)
        assert e <= 3.0 * e32, (k, e, e32)
        assert m <= 2e-5, (k, m)


def test_probe_linear_refuses_what_it_cannot_run(gpu_device):
    from avid_hip import ops
    x = torch.zeros(257, 64, device=gpu_device)
    w, b = torch.zeros(5, 64, device=gpu_device), torch.zeros(5, device=gpu_device)
    with pytest.raises(ops.AvidHipError):
        ops.probe_linear(x, w, b)
    with pytest.raises(ops.AvidHipError):
        ops.probe_linear(torch.zeros(2, 16388, device=gpu_device), torch.zeros(5, 16388, device=gpu_device), b)


# ------------------------------------------------------------------------------------------------------------------ module
def _model(dev, seed=0, **kw):
    import models
    torch.manual_seed(seed)
    args = dict(SHIPPED)
    args.update(kw)
    return models.MOSTModel(models.R2Plus1D(18), **args).to(dev).train()


def _head_grads(m):
    return {n: p.grad.clone() for n, p in m.classifiers.named_parameters()}


def test_programs_match_the_per_layer_path(gpu_device, kernel_log):
    dev = gpu_device
    m = _model(dev)
    m_ref = copy.deepcopy(m)
    g = torch.Generator().manual_seed(1)
    video = torch.randn((4, 3, 8, 64, 64), generator=g).to(dev)
    labels = torch.randint(0, 400, (4,), generator=g).to(dev)
    with kernel_log() as log:
        out = m(video)
    assert log.launches("adaptive_maxpool") == 4 and log.launches("bn1d_fwd_train_kernel") == 4
    assert log.launches("probe_gemm_kernel") == 4, sorted(log.report)
    assert all(type(v.grad_fn).__name__ == "ProbeFnBackward" for v in out.values()) and list(out) == SHIPPED["feat_names"]
    sum(F.cross_entropy(out[k], labels) for k in out).backward()
    # the per-layer path: a hook anywhere sends the call there
    h = m_ref.classifiers[0].classifier.register_forward_hook(lambda *a: None)
    ref = m_ref(video)
    h.remove()
    assert all(type(v.grad_fn).__name__ != "ProbeFnBackward" for v in ref.values())
    sum(F.cross_entropy(ref[k], labels) for k in ref).backward()
    for k in out:
        assert torch.equal(out[k], ref[k]), k
    ga, gb = _head_grads(m), _head_grads(m_ref)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert all(p.grad is None for p in m.feature_extractor.parameters())
    assert all(p.grad is None for p in m_ref.feature_extractor.parameters())
    for (n, a), b in zip(m.named_buffers(), m_ref.buffers()):
        assert torch.equal(a, b), n


def test_tower_statistics_move_in_training_and_stand_still_in_eval(gpu_device):
    dev = gpu_device
    m = _model(dev)
    video = torch.randn(2, 3, 8, 64, 64, device=dev)
    before = {n: b.clone() for n, b in m.named_buffers()}
    m(video)
    moved = [n for n, b in m.named_buffers() if not torch.equal(b, before[n])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))
    before = {n: b.clone() for n, b in m.named_buffers()}
    m.eval()
    with torch.no_grad():
        out = m(video)
    assert all(v.shape == (2, 400) for v in out.values())
    assert all(torch.equal(b, before[n]) for n, b in m.named_buffers())
    # a tower put in eval mode by hand under training heads: the per-layer path, avid_bn_fwd_eval in the tower
    m.train()
    m.feature_extractor.eval()
    out = m(video)
    assert all(type(v.grad_fn).__name__ != "ProbeFnBackward" for v in out.values())
    for n, b in m.named_buffers():
        assert torch.equal(b, before[n]) == n.startswith("feature_extractor."), n


def _stub_model(dev, z):
    import models

    class Stub(nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.ones(1))

        def forward(self, x, return_embs=False):
            return {k[4:]: torch.from_numpy(z[k]).to(x.device) for k in z.files if k.startswith("tap.")}

    names = [k[4:] for k in z.files if k.startswith("tap.")]
    pools = {"a": "AdaptiveMaxPool3d((1,2,2))", "b": "AdaptiveMaxPool3d((1,4,4))", "c": "AdaptiveMaxPool3d((2,2,3))"}
    dims = [z[f"init.{i}.classifier.weight"].shape[1] for i in range(len(names))]
    m = models.MOSTModel(Stub(), 7, names, dims, [pools[n] for n in names], use_bn=True)
    m.classifiers.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init.")})
    return m.to(dev).train(), names


def test_heads_reproduce_the_reference_fixture(gpu_device, kernel_log):
    z = np.load(os.path.join(GOLDEN, "most_heads.npz"))
    m, names = _stub_model(gpu_device, z)
    labels = torch.from_numpy(z["labels"]).to(gpu_device)
    with kernel_log() as log:
        out = m(torch.zeros(4, 3, 1, 1, 1, device=gpu_device))
        loss = sum(F.cross_entropy(out[n], labels) for n in names)
        loss.backward()
    assert log.launches("adaptive_maxpool") == 3 and log.launches("bn1d_bwd_kernel") == 3
    np.testing.assert_allclose(float(loss), float(z["loss"]), rtol=1e-5)
    for n in names:
        np.testing.assert_allclose(out[n].detach().cpu().numpy(), z[f"logits.{n}"], rtol=1e-5, atol=1e-6)
    for k, p in m.classifiers.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), z[f"grad.{k}"], rtol=1e-5, atol=1e-7, err_msg=k)
    for k, v in m.classifiers.state_dict().items():
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(v.cpu().numpy(), z[f"after.{k}"], rtol=1e-5, atol=1e-7, err_msg=k)
    assert m.feature_extractor.scale.grad is None


def test_other_heads_take_the_torch_ops(gpu_device, kernel_log):
    """l2_norm / another pooling op / no BatchNorm: the reference's ops, correct against the reference's own expression."""
    dev = gpu_device
    m = _model(dev, l2_norm=True, pooling_ops=["AdaptiveAvgPool3d((1,12,12))"] + SHIPPED["pooling_ops"][1:], use_bn=False)
    video = torch.randn(2, 3, 8, 64, 64, device=dev)
    with kernel_log() as log:
        out = m(video)
    assert log.launches("adaptive_maxpool") == 0 and log.launches("probe_gemm_kernel") == 4
    with torch.no_grad():
        embs = copy.deepcopy(m).feature_extractor(video, return_embs=True)
    for c, ft in zip(m.classifiers, SHIPPED["feat_names"]):
        x = c.pooling(F.normalize(embs[ft], p=2, dim=-1)).reshape(2, -1)
        torch.testing.assert_close(out[ft], F.linear(x, c.classifier.weight, c.classifier.bias), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ ProbeStep
def _torch_step(m, opt, video, labels):
    """One iteration of the reference's loop, restated: tower with return_embs under no_grad, torch heads, summed loss."""
    opt.zero_grad()
    with torch.no_grad():
        embs = m.feature_extractor(video, return_embs=True)
    losses = []
    for c, ft in zip(m.classifiers, m.feat_names):
        x = c.pooling(embs[ft]).reshape(video.shape[0], -1)
        x = nn.BatchNorm1d.forward(c.bn, x)              # torch's own module forward (F.batch_norm, counter bumped)
        losses.append(F.cross_entropy(F.linear(x, c.classifier.weight, c.classifier.bias), labels))
    sum(losses).backward()
    opt.step()
    return [float(l) for l in losses]


def _off_bar(m_a, m_b):
    out = {}
    for (n, a), b in zip(m_a.named_parameters(), m_b.parameters()):
        off = ~torch.isclose(a, b, rtol=1e-4, atol=1e-6)
        if bool(off.any()):
            out[n] = (int(off.sum()), a.numel(), float((a - b).abs().max()))
    return out


def test_probe_step_against_the_torch_loop(gpu_device):
    from avid_hip import parallel
    dev, steps = gpu_device, 3
    g = torch.Generator().manual_seed(3)
    vids = [torch.randn((4, 3, 8, 64, 64), generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 400, (4,), generator=g).to(dev) for _ in range(steps)]
    m_eng = _model(dev)
    m_ref = copy.deepcopy(m_eng)
    tower0 = {n: p.detach().clone() for n, p in m_eng.feature_extractor.named_parameters()}
    eng = parallel.ProbeStep(m_eng, lr=1e-4)
    opt = torch.optim.Adam(m_ref.parameters(), lr=1e-4, weight_decay=0)
    le, lr_ = [], []
    for i in range(steps):
        losses, hits = eng.step(vids[i], labs[i])
        assert losses.shape == (4,) and hits.shape == (4, 2) and hits.dtype == torch.int64
        le.append(losses.cpu().tolist())
        lr_.append(_torch_step(m_ref, opt, vids[i], labs[i]))
    torch.cuda.synchronize()
    assert bool(((0 <= hits[:, 0]) & (hits[:, 0] <= hits[:, 1]) & (hits[:, 1] <= 4)).all())
    print(f"\n[probe step] losses {le} against torch {lr_}")
    np.testing.assert_allclose(le, lr_, rtol=1e-4)
    total = sum(p.numel() for p in m_eng.classifiers.parameters())
    off = _off_bar(m_eng, m_ref)
    assert sum(k for k, _, _ in off.values()) <= 0.05 * total, off
    for n, p in m_eng.feature_extractor.named_parameters():
        assert torch.equal(p, tower0[n]) and not p.requires_grad and p.grad is None, n
    for (n, a), b in zip(m_eng.named_buffers(), m_ref.buffers()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6, msg=n)
    eng.set_lr(5e-5)
    assert float(eng.lr_dev) == pytest.approx(5e-5)


def test_probe_step_state_dict_round_trip(gpu_device):
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    vids = [torch.randn((2, 3, 8, 64, 64), generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, 400, (2,), generator=g).to(dev) for _ in range(3)]
    m = _model(dev)
    eng = parallel.ProbeStep(m)
    for i in range(2):
        eng.step(vids[i], labs[i])
    torch.cuda.synchronize()
    msd = {k: v.clone() for k, v in m.state_dict().items()}
    osd = copy.deepcopy(eng.state_dict())
    n_all, n_tower = len(list(m.parameters())), len(list(m.feature_extractor.parameters()))
    assert osd["param_groups"][0]["params"] == list(range(n_all))            # frozen tower parameters listed ...
    assert sorted(osd["state"]) == list(range(n_tower, n_all))               # ... and without state
    la, _ = eng.step(vids[2], labs[2])
    after = {n: p.detach().clone() for n, p in m.named_parameters()}
    m2 = _model(dev, seed=1)
    m2.load_state_dict(msd)
    eng2 = parallel.ProbeStep(m2)
    eng2.load_state_dict(osd)
    lb, _ = eng2.step(vids[2], labs[2])
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for n, p in m2.named_parameters():
        assert torch.equal(p, after[n]), n
    # into torch.optim.Adam(model.parameters()) and back
    opt = torch.optim.Adam(m2.parameters(), lr=1e-4)
    opt.load_state_dict(copy.deepcopy(osd))
    back = opt.state_dict()
    assert sorted(back["state"]) == sorted(osd["state"])
    eng3 = parallel.ProbeStep(m2)
    eng3.load_state_dict(back)
    sd3 = eng3.state_dict()
    for k in osd["state"]:
        assert torch.equal(sd3["state"][k]["exp_avg"], osd["state"][k]["exp_avg"])
        assert torch.equal(sd3["state"][k]["exp_avg_sq"], osd["state"][k]["exp_avg_sq"])
        assert float(sd3["state"][k]["step"]) == 2.0


def test_probe_step_evaluate_and_labels(gpu_device):
    from avid_hip import ops, parallel
    dev = gpu_device
    m = _model(dev)
    eng = parallel.ProbeStep(m)
    g = torch.Generator().manual_seed(4)
    V, clips = 3, 2
    video = torch.randn((V, clips, 3, 8, 64, 64), generator=g).to(dev)
    labels = torch.randint(0, 400, (V,), generator=g).to(dev)
    conf, loss, hits = eng.evaluate(video, labels, batch=4)
    assert m.training and conf.shape == (4, V, 400) and loss.shape == (4,) and hits.shape == (4, 2)
    m.eval()
    with torch.no_grad():
        outs = [m(video.flatten(0, 1)[i:i + 4]) for i in range(0, V * clips, 4)]
    m.train()
    for t, ft in enumerate(SHIPPED["feat_names"]):
        logits = torch.cat([o[ft] for o in outs])
        ref = torch.softmax(logits, 1).view(V, clips, -1).mean(1)
        torch.testing.assert_close(conf[t], ref, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(loss[t], F.cross_entropy(logits, labels.repeat_interleave(clips)), rtol=1e-5, atol=1e-6)
        top = ref.topk(5, 1).indices
        assert int(hits[t, 0]) == int((top[:, 0] == labels).sum())
        assert int(hits[t, 1]) == int((top == labels[:, None]).any(1).sum())
    # labels: shape / dtype / device are checked on the host, the range through the device error word
    clip = video[:, 0].contiguous()
    for bad in (labels.to(torch.int32), labels[:1], labels.cpu()):
        with pytest.raises(ValueError):
            eng.step(clip, bad)
    ops.check_device_errors(dev)
    bad = labels.clone()
    bad[1] = 400
    eng.step(clip, bad)
    with pytest.raises(ops.LabelError):
        ops.check_device_errors(dev)
