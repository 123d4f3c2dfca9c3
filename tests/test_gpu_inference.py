"""Whole models through the inference programs (``avid_hip.parallel.Inference`` -> ``plan.EvalPlan``): the results are the bits
of ``model.eval()(x)`` under ``torch.no_grad()`` on the per-layer path, the programs are what ran, and nothing about training
moves.  ``ops.tconv_configure(2)`` sends conv2x's temporal layers of these small clips through tconv64_kernel, so that the
fused epilogues run (48 x 48 pixels: 144 positions per clip behind the stem's tail — tiles straddle clips, the last is ragged)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import detgen
from _inference_probe import evaluate_digest, golden_av_wrapper, most_model, probe_digest, wrapper

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture
def tconv_all(gpu_device):
    from avid_hip import ops
    assert ops.tconv_configure(2) == 2
    yield
    ops.tconv_configure(-1)


def _per_layer(m, *inputs):
    flags = [(mod, mod.training) for mod in m.modules()]
    m.eval()
    try:
        with torch.no_grad():
            return m(*inputs)
    finally:
        for mod, f in flags:
            mod.training = f


def _eval_plans(m):
    return [v for k, v in m.__dict__.get("_avid_plans", {}).items() if k[0] == "eval" and v]


@pytest.mark.parametrize("kind", ["tower", "classifier"])
@pytest.mark.parametrize("shape", [(3, 3, 8, 48, 48), (2, 3, 8, 64, 64), (2, 3, 32, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_video_models_equal_the_per_layer_eval_forward(kind, shape, gpu_device, tconv_all):
    from avid_hip import parallel, plan
    m = wrapper(gpu_device, seed=shape[2])
    if kind == "tower":
        m = m.feature_extractor
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    want = _per_layer(m, x)
    infer = parallel.Inference(m)
    got = infer(x)
    assert infer.used_programs is True
    assert all(mod.training for mod in m.modules()), "Inference touched the training flags"
    assert got.shape == want.shape and torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(infer(x), want)                       # the cached program, a second call
    assert not got.requires_grad
    # the program: no BatchNorm record between the stem's tail and conv3x in an 8-frame clip; with 32 frames no layer takes
    # the tconv forms and every BatchNorm behind the stem is an apply record
    pl, = _eval_plans(m)
    ops_ = [pl.fwd_prog[k] for k in range(pl.n_fwd)]
    assert ops_[0].op == plan.OP_BN_EVAL_COEFFS and ops_[0].i[0] == 33
    tail = next(k for k, r in enumerate(ops_) if r.op == plan.OP_BN_POOL_FWD_EVAL)
    conv3x = next(k for k, r in enumerate(ops_) if r.op == plan.OP_CONV_FWD and r.d.Cout == 128)
    between = [r.op for r in ops_[tail + 1:conv3x]]
    n_apply = sum(1 for r in ops_ if r.op == plan.OP_BN_EVAL_APPLY)
    if shape[2] == 8:
        assert between == [plan.OP_CONV_FWD] * 8 and n_apply == 24, plan.dump(pl.fwd_prog, conv3x + 1)
        assert [(r.i[1], r.i[3]) for r in ops_[tail + 1:conv3x]] == [(0, 0), (2, 2)] * 4
    else:
        assert n_apply == 32 and all(r.i[1] == 0 and r.i[3] == 0 for r in ops_ if r.op == plan.OP_CONV_FWD)
    assert pl.fa_bytes < pl.virtual_bytes                     # the arena is recycled


def test_av_wrapper_equals_the_per_layer_eval_forward(gpu_device, tconv_all):
    import models
    from avid_hip import parallel
    torch.manual_seed(3)
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).to(gpu_device).train()
    g = torch.Generator().manual_seed(2)
    video, audio = torch.randn((2, 3, 8, 64, 64), generator=g).to(gpu_device), torch.randn((2, 1, 40, 100), generator=g).to(gpu_device)
    m(video, audio)                                           # one training forward: the running statistics leave their initial values
    want = _per_layer(m, video, audio)
    infer = parallel.Inference(m)
    got = infer(video, audio)
    assert infer.used_programs is True and isinstance(got, tuple) and len(got) == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert m.training


def test_inference_meets_the_reference_golden(golden, gpu_device):
    """tests/golden/av_wrapper.npz: the reference's own eval-mode embeddings after one training forward on the fixture inputs
    (tests/test_gpu_model.py::test_av_wrapper_vs_reference_golden's recipe and its 2e-4 of scale)."""
    from avid_hip import parallel
    g = golden("av_wrapper")
    m = golden_av_wrapper(gpu_device).train()
    video = T(detgen.det_normalish("in:video", (2, 3, 8, 112, 112))).to(gpu_device)
    audio = T(detgen.det_normalish("in:audio", (2, 1, 40, 100))).to(gpu_device)
    m(video, audio)
    infer = parallel.Inference(m)
    ve, ae = infer(video, audio)
    assert infer.used_programs is True

    def err(a, ref):
        a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
        return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-12)
    assert err(ve.cpu().numpy(), g["eval_video_emb"]) < 2e-4
    assert err(ae.cpu().numpy(), g["eval_audio_emb"]) < 2e-4


def test_finetune_evaluate_runs_the_programs_and_keeps_its_bits(gpu_device):
    """FinetuneStep.evaluate with a chunk size that does not divide V x clips: two plans, the per-layer results bit for bit;
    under AVID_EVAL_PLAN=0 (a fresh process) the per-layer path, the same bits."""
    from avid_hip import ops
    info, (m, video, labels, conf, loss, hits) = evaluate_digest(gpu_device)
    assert info == {"sha": info["sha"], "eval_plans": 2, "enabled": True, "training": True}
    ops.tconv_configure(2)
    try:
        x = video.flatten(0, 1)
        logits = torch.cat([_per_layer(m, x[i:i + 4].contiguous()) for i in range(0, 9, 4)], 0)
        loss2, conf2, hits2, _ = ops.cls_loss(logits, labels, 3)
    finally:
        ops.tconv_configure(-1)
    assert torch.equal(conf, conf2) and torch.equal(loss, loss2) and torch.equal(hits, hits2)
    assert _child([]) == {"sha": info["sha"], "eval_plans": 0, "enabled": False, "training": True}


def _child(arg):
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "_inference_probe.py")] + arg, capture_output=True, text=True,
                         env=dict(os.environ, AVID_EVAL_PLAN="0"), timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])


def test_most_model_equals_the_per_layer_eval_forward(gpu_device):
    """The stock linear probe at 4 x 3x8x64x64 (the geometry tests/test_probe_host.py compiles): the dict of logits, bit for bit.
    Its tower is frozen, so the per-layer path computes every BatchNorm without coefficient vectors — the program holds the
    same calls as records (no fused BatchNorm, no coefficient launch), then the heads' pool / BatchNorm1d / Linear records."""
    from avid_hip import parallel, plan
    m = most_model(gpu_device, seed=4)
    x = torch.randn((4, 3, 8, 64, 64), generator=torch.Generator().manual_seed(6)).to(gpu_device)
    flags = [mod.training for mod in m.modules()]
    want = _per_layer(m, x)
    infer = parallel.Inference(m)
    got = infer(x)
    assert infer.used_programs is True and isinstance(got, dict) and list(got) == list(m.feat_names) == list(want)
    for ft in m.feat_names:
        assert got[ft].shape == (4, 400) and torch.equal(got[ft], want[ft]), ft
    assert [mod.training for mod in m.modules()] == flags, "Inference touched the training flags"
    pl, = _eval_plans(m)
    kinds = [pl.fwd_prog[k].op for k in range(pl.n_fwd)]
    assert kinds.count(plan.OP_BN_EVAL_DIRECT) == 33 and kinds.count(plan.OP_MAXPOOL_FWD) == 1
    assert not {plan.OP_BN_EVAL_COEFFS, plan.OP_BN_EVAL_APPLY, plan.OP_BN_POOL_FWD_EVAL} & set(kinds)
    assert all(pl.fwd_prog[k].i[1] == 0 and pl.fwd_prog[k].i[3] == 0 for k in range(pl.n_fwd) if pl.fwd_prog[k].op == plan.OP_CONV_FWD)
    assert kinds[-12:] == [plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_PROBE_LINEAR_FWD] * 4
    # the same tower with trainable BatchNorms takes the coefficient forms — and the per-layer path's other expression with them
    for p in m.feature_extractor.parameters():
        p.requires_grad_(True)
    want2 = _per_layer(m, x)
    got2 = infer(x)
    assert infer.used_programs and all(torch.equal(got2[ft], want2[ft]) for ft in m.feat_names)
    assert len(_eval_plans(m)) == 2


def test_probe_evaluate_runs_the_programs_and_keeps_its_bits(gpu_device):
    """ProbeStep.evaluate with a chunk size that does not divide V x clips: two plans, the per-layer results bit for bit; under
    AVID_EVAL_PLAN=0 (a fresh process) the per-layer path, the same bits."""
    from avid_hip import ops
    info, (m, video, labels, conf, loss, hits) = probe_digest(gpu_device)
    assert info == {"sha": info["sha"], "eval_plans": 2, "enabled": True, "training": True}
    x = video.flatten(0, 1)
    outs = [_per_layer(m, x[i:i + 4].contiguous()) for i in range(0, 9, 4)]
    res = [ops.cls_loss(torch.cat([o[ft] for o in outs], 0), labels, 3) for ft in m.feat_names]
    assert torch.equal(conf, torch.stack([r[1] for r in res])) and torch.equal(loss, torch.stack([r[0] for r in res]))
    assert torch.equal(hits, torch.stack([r[2] for r in res]))
    assert _child(["probe"]) == {"sha": info["sha"], "eval_plans": 0, "enabled": False, "training": True}


def test_staleness_and_fallbacks(gpu_device, tconv_all):
    """A training step between two calls moves the result exactly as it moves the per-layer result (the coefficients are
    recomputed from the moved running statistics, the weights re-read); `.cpu().cuda()` gets a fresh program; a forward hook
    sends the call to the per-layer path."""
    from avid_hip import parallel
    m = wrapper(gpu_device, seed=11)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 8, 48, 48), generator=g).to(gpu_device)
    labels = torch.randint(0, 101, (2,), generator=g).to(gpu_device)
    infer = parallel.Inference(m)
    y0 = infer(x).clone()
    eng = parallel.FinetuneStep(m, lr=1e-3)
    eng.step(x, labels)
    y1 = infer(x)
    assert infer.used_programs and not torch.equal(y0, y1)
    assert torch.equal(y1, _per_layer(m, x))
    n0 = len(_eval_plans(m))
    m = m.cpu().to(gpu_device)
    infer = parallel.Inference(m)
    y2 = infer(x)
    assert infer.used_programs and len(_eval_plans(m)) == n0 + 1 and torch.equal(y2, y1)
    seen = []
    h = m.classifier.register_forward_hook(lambda mod, i, o: seen.append(1))
    y3 = infer(x)
    h.remove()
    assert infer.used_programs is False and seen == [1] and torch.equal(y3, y1)
    assert m.training


def test_training_is_untouched_by_inference_calls(gpu_device, tconv_all):
    """The same FinetuneStep.step with and without Inference calls around it: same loss, same parameters, same running
    statistics (plans, arenas and tables are separate)."""
    from avid_hip import parallel
    g = torch.Generator().manual_seed(9)
    x = torch.randn((2, 3, 8, 48, 48), generator=g).to(gpu_device)
    labels = torch.randint(0, 101, (2,), generator=g).to(gpu_device)
    res = []
    for with_inference in (False, True):
        m = wrapper(gpu_device, seed=13)
        m.dropout.seed = 1234
        eng = parallel.FinetuneStep(m)
        if with_inference:
            parallel.Inference(m)(x)
        loss, _ = eng.step(x, labels)
        if with_inference:
            parallel.Inference(m)(x)
        loss2, _ = eng.step(x, labels)
        res.append((loss.clone(), loss2.clone(), [p.detach().clone() for p in m.parameters()], [b.clone() for b in m.buffers()]))
    a, b = res
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2])) and all(torch.equal(p, q) for p, q in zip(a[3], b[3]))
