"""Fine-tuning, linear-probe and inference programs around the audio tower (``Conv2D``) on the GPU.

Shapes (tests/_audio_downstream.py): (4, 1, 64, 65) — even and odd extents, taps 16x17, 8x9, 4x5, 4x5 —, (3, 1, 50, 33) — an odd
batch, extents the strides do not divide, a fourth head of 512 features — and one case of each kind at (4, 1, 200, 257) with the
shipped-style heads.

1. The programs against the per-layer path of the same tree, bit for bit (``torch.equal``): logits, loss, hits, running
   statistics and counters, and every gradient — except that the per-layer path outside an engine launches every weight gradient
   on its own, where the programs group the small ones: those (``_grouped_ids``) are held to tests/test_gpu_finetune.py's 1e-5,
   and a second run with the grouped launch switched off in both paths holds EVERY gradient and the parameters after two
   optimizer steps (Adam, SGD with momentum) bit for bit.
2. Against a float64 torch restatement of tower and heads (tests/_audio_downstream.py), at the bars tests/test_gpu_finetune.py and
   tests/test_gpu_probe.py use around the video tower — loss 1e-5 (fine-tuning) / 1e-4 (probe), logits and gradients
   max|err| / max|ref| < 5e-4, running statistics rtol 1e-4 / atol 1e-6; the fine-tuning restatement takes the step's ReLU
   signs and pool picks, as that file's oracle does — and against the reference's own float32 results
   (tests/golden/audio_downstream.npz) at the same bars.
3. Dense evaluation, 3 recordings x 5 clips: the clip-averaged hits of the float64 restatement.
4. ``virtual_ranks=2`` on a batch of 8: bit for bit the two one-shard engines' sum (tests/test_gpu_virtual_downstream.py's
   check, fine-tuning and probe), and the two-shard rule of tests/_dp_ref.py in float64 (fine-tuning without dropout, because the
   rule's module sees a shard and not its rank; the probe one tap at a time, the frozen tower held outside the rule's module).
5. ``KNNEval(model=Conv2D(), ...)`` against tests/_knn_ref.py on the features ``Inference`` returns.
6. The three programs under tests/_guards.py: no guard byte changes, the same bits under both fills."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _audio_downstream as AD
import _dp_ref
import _knn_ref
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
SHAPES = [AD.SMALL, AD.ODD, AD.SHIPPED]
IDS = ["4x64x65", "3x50x33", "4x200x257"]
LOSS_FT, LOSS_PROBE, TENSOR, STATS = 1e-5, 1e-4, 5e-4, dict(rtol=1e-4, atol=1e-6)


def _data(shape, dev, seed=0, steps=1):
    g = torch.Generator().manual_seed(1000 * seed + shape[2] + shape[0])
    xs = [torch.randn(shape, generator=g).to(dev) for _ in range(steps)]
    ys = [torch.randint(0, AD.N_CLASSES, (shape[0],), generator=g).to(dev) for _ in range(steps)]
    return xs, ys


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
    """The grouped weight-gradient launch off, in the programs (the plan cache key carries the switch) and in the ops alike."""
    from avid_hip import ops
    prev, ops.GROUP_WGRAD = ops.GROUP_WGRAD, 0
    try:
        yield
    finally:
        ops.GROUP_WGRAD = prev


def _grouped_ids(pl):
    from avid_hip import plan
    at = {4 * o: i for i, o in enumerate(pl.goff)}
    return {id(pl.params[at[pl.bwd_prog[k].t[2].off]]) for k in range(pl.n_bwd) if pl.bwd_prog[k].op == plan.OP_WGRAD_ITEM}


def _same_buffers(m1, m2):
    for (n, a), b in zip(m1.named_buffers(), m2.buffers()):
        assert torch.equal(a, b), n


def _same_grads(m1, m2, grouped=()):
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        if not p1.requires_grad:
            assert p1.grad is None and p2.grad is None, n
        elif id(p1) in grouped:
            err = float((p1.grad - p2.grad).abs().max() / p2.grad.abs().max())
            print(f"  grouped weight gradient {n}: {err:.2e} / 1e-5")
            assert err < 1e-5, (n, err)
        else:
            assert torch.equal(p1.grad, p2.grad), n


def _optimizer(kind, params):
    from avid_hip import parallel
    if kind == "sgd":
        return parallel.SGD(params, lr=1e-2, momentum=0.9)
    return parallel.Adam(params, lr=1e-3)


def _engine_args(kind):
    return dict(lr=1e-2, optimizer="sgd", momentum=0.9) if kind == "sgd" else dict(lr=1e-3)


# ---------------------------------------------------------------------------------------------------- 1. programs == per-layer path
def _cls_per_layer_step(m, x, y, opt=None):
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        logits = m(x)
    assert type(logits.grad_fn).__name__ != "ClsFnBackward"
    loss, _, hits, d = ops.cls_loss(logits.detach(), y, grad_scale=1.0)
    logits.backward(d)
    if opt is not None:
        opt.step()
    return logits.detach(), loss, hits


def _probe_per_layer_step(m, x, y, opt=None):
    from avid_hip import ops
    if opt is not None:
        opt.zero_grad()
    with _per_layer():
        out = m(x)
    assert list(out) == AD.STAGES and all(type(v.grad_fn).__name__ != "ProbeFnBackward" for v in out.values())
    res = [ops.cls_loss(v.detach(), y, grad_scale=1.0) for v in out.values()]
    torch.autograd.backward(list(out.values()), [r[3] for r in res])
    if opt is not None:
        opt.step()
    return {k: v.detach() for k, v in out.items()}, torch.stack([r[0] for r in res]), torch.stack([r[2] for r in res])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_finetune_step_matches_the_per_layer_path(gpu_device, shape):
    from avid_hip import parallel
    dev = gpu_device
    (x,), (y,) = _data(shape, dev, 1)
    m1 = AD.cls_model().to(dev).train()
    m2, m3 = copy.deepcopy(m1), copy.deepcopy(m1)
    eng = parallel.FinetuneStep(m1)
    loss1, hits1 = eng.step(x, y)
    logits1 = m3(x)                                                    # the same programs as an autograd node: the logits
    assert type(logits1.grad_fn).__name__ == "ClsFnBackward"
    logits2, loss2, hits2 = _cls_per_layer_step(m2, x, y)
    torch.cuda.synchronize()
    assert torch.equal(logits1, logits2) and torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist()
    assert m1.dropout.offset == m2.dropout.offset == m3.dropout.offset == 1
    _same_grads(m1, m2, _grouped_ids(eng._step_plan))
    _same_buffers(m1, m2)
    _same_buffers(m3, m2)
    assert {int(b) for n, b in m1.named_buffers() if n.endswith("num_batches_tracked")} == {1}


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_finetune_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device, shape, kind):
    from avid_hip import parallel
    dev = gpu_device
    xs, ys = _data(shape, dev, 2, steps=2)
    with _ungrouped():
        m1 = AD.cls_model().to(dev).train()
        m2 = copy.deepcopy(m1)
        eng = parallel.FinetuneStep(m1, **_engine_args(kind))
        opt = _optimizer(kind, list(m2.parameters()))
        for i in range(2):
            loss1, hits1 = eng.step(xs[i], ys[i])
            assert not _grouped_ids(eng._step_plan)
            _, loss2, hits2 = _cls_per_layer_step(m2, xs[i], ys[i], opt)
            torch.cuda.synchronize()
            assert torch.equal(loss1, loss2) and hits1.tolist() == hits2.tolist(), i
            _same_grads(m1, m2)
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1, p2), n
    _same_buffers(m1, m2)
    before = AD.cls_model().state_dict()
    assert not any(torch.equal(p.detach().cpu(), before[n]) for n, p in m1.named_parameters())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_probe_step_matches_the_per_layer_path(gpu_device, shape):
    from avid_hip import parallel
    dev = gpu_device
    (x,), (y,) = _data(shape, dev, 3)
    m1 = AD.probe_model(shape).to(dev).train()
    m2, m3 = copy.deepcopy(m1), copy.deepcopy(m1)
    eng = parallel.ProbeStep(m1)
    losses1, hits1 = eng.step(x, y)
    out1 = m3(x)
    assert all(type(v.grad_fn).__name__ == "ProbeFnBackward" for v in out1.values()) and list(out1) == AD.STAGES
    out2, losses2, hits2 = _probe_per_layer_step(m2, x, y)
    torch.cuda.synchronize()
    for k in AD.STAGES:
        assert torch.equal(out1[k], out2[k]), k
    assert torch.equal(losses1, losses2) and torch.equal(hits1, hits2)
    _same_grads(m1, m2)
    _same_buffers(m1, m2)
    _same_buffers(m3, m2)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_probe_two_steps_match_the_per_layer_path_bit_for_bit(gpu_device, kind):
    from avid_hip import parallel
    dev, shape = gpu_device, AD.ODD
    xs, ys = _data(shape, dev, 4, steps=2)
    m1 = AD.probe_model(shape).to(dev).train()
    m2 = copy.deepcopy(m1)
    eng = parallel.ProbeStep(m1, **_engine_args(kind))
    opt = _optimizer(kind, [p for p in m2.parameters() if p.requires_grad])
    for i in range(2):
        losses1, _ = eng.step(xs[i], ys[i])
        _, losses2, _ = _probe_per_layer_step(m2, xs[i], ys[i], opt)
        assert torch.equal(losses1, losses2), i
    torch.cuda.synchronize()
    before = AD.probe_model(shape).state_dict()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1, p2), n
        assert torch.equal(p1.detach().cpu(), before[n]) == n.startswith("feature_extractor."), n
    _same_buffers(m1, m2)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inference_programs_match_the_per_layer_path(gpu_device, shape):
    from avid_hip import parallel
    dev = gpu_device
    (x,), _ = _data(shape, dev, 5)
    for m in (AD.tower_model(), AD.cls_model(), AD.probe_model(shape)):
        m = m.to(dev).train()                                         # (Inference leaves the modules' flags alone)
        before = {n: b.clone() for n, b in m.named_buffers()}
        inf = parallel.Inference(m)
        out = inf(x)
        assert inf.used_programs is True, type(m).__name__
        ref = inf._per_layer(x)
        torch.cuda.synchronize()
        if isinstance(ref, dict):
            assert list(out) == list(ref) == AD.STAGES
            for k in ref:
                assert out[k].shape == (shape[0], AD.N_CLASSES) and torch.equal(out[k], ref[k]), k
        else:
            assert out.shape == ref.shape and torch.equal(out, ref), type(m).__name__
        assert all(mod.training for mod in m.modules())
        assert all(torch.equal(b, before[n]) for n, b in m.named_buffers())


# --------------------------------------------------------------------------------------------------------------- 2. against float64
def _report(what, rows):
    print(f"\n[{what}] " + ", ".join(f"{k} {e:.2e} / {bar:.0e}" for k, e, bar in rows))
    for k, e, bar in rows:
        assert e < bar, (what, k, e, bar)


def _stats_close(m, ref):
    rb = dict(ref.named_buffers())
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(rb[n]), n
        else:
            torch.testing.assert_close(b.double().cpu(), rb[n], msg=n, **STATS)


def _decisions(m, x):
    """The tower's ReLU masks and global-max-pool picks (``TorchTower.pins``) as the per-layer path of a copy of ``m`` takes them
    on x: forward hooks on its BatchNorms, whose output is ReLU(bn(.)) — a hooked model is not compiled, and the programs are
    that path's bits (test_finetune_step_matches_the_per_layer_path)."""
    m = copy.deepcopy(m)
    got, mods = {}, dict(m.feature_extractor.named_modules())

    def keep(name):
        def hook(mod, inp, out):
            h = out[:, 0].permute(0, 3, 1, 2)                          # channels-last [B, 1, H, W, C] -> [B, C, H, W]
            got[name] = (h > 0).cpu()
            if name == AD.BN_NAMES[-1]:
                got["pool"] = h.flatten(2).argmax(2).cpu()
        return hook
    hooks = [mods[name].register_forward_hook(keep(name)) for name in AD.BN_NAMES]
    try:
        out = m(x)
    finally:
        for h in hooks:
            h.remove()
    assert type(out.grad_fn).__name__ != "ClsFnBackward" and sorted(got) == sorted(AD.BN_NAMES + ["pool"])
    return got


def _finetune_against(dev, m, x, y, ref_of):
    """One ``FinetuneStep.step`` of ``m`` on (x, y): (loss, logits, {name: gradient}, the restatement after its own pass).  The
    restatement takes the step's ReLU and max-pool decisions (``_decisions``), as tests/test_gpu_finetune.py's oracle does; how
    many of them float64 would have taken differently is printed."""
    from avid_hip import ops, parallel
    seed, offset = m.dropout.seed, m.dropout.offset
    ref = ref_of(m)
    ref.keep = ops.dropout_mask(x.shape[0], 512, 0.5, seed, offset, dev).bool().cpu()
    tower = ref.feature_extractor
    tower.pins = _decisions(m, x)
    m3 = copy.deepcopy(m)
    eng = parallel.FinetuneStep(m)
    loss, _ = eng.step(x, y)
    logits = m3(x).detach()
    torch.cuda.synchronize()
    rl = ref(x.double().cpu())
    rloss = F.cross_entropy(rl, y.cpu())
    rloss.backward()
    flips = {n: int((tower.seen[n] != tower.pins[n]).sum()) for n in tower.pins}
    flips = {n: k for n, k in flips.items() if k}
    print(f"\n  decisions float64 takes differently: {flips} of {sum(v.numel() for v in tower.pins.values())}")
    return loss, logits, {n: p.grad for n, p in m.named_parameters()}, ref, rl.detach(), rloss.detach()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_finetune_step_against_float64(gpu_device, shape):
    dev = gpu_device
    (x,), (y,) = _data(shape, dev, 6)
    m = AD.cls_model().to(dev).train()
    loss, logits, grads, ref, rl, rloss = _finetune_against(dev, m, x, y, AD.restate)
    assert 0.3 < float(ref.keep.double().mean()) < 0.7
    rg = {n: p.grad for n, p in ref.named_parameters()}
    assert list(rg) == list(grads)
    rows = [("loss", abs(float(loss) - float(rloss)) / abs(float(rloss)), LOSS_FT), ("logits", AD.max_rel(logits, rl), TENSOR)]
    rows += [(n, AD.max_rel(grads[n], rg[n]), TENSOR) for n in grads]
    _report(f"finetune {shape} against float64", rows)
    _stats_close(m, ref)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_probe_step_against_float64(gpu_device, shape):
    from avid_hip import parallel
    dev = gpu_device
    (x,), (y,) = _data(shape, dev, 7)
    m = AD.probe_model(shape).to(dev).train()
    ref = AD.restate(m, shape)
    m3 = copy.deepcopy(m)
    eng = parallel.ProbeStep(m)
    losses, hits = eng.step(x, y)
    out = {k: v.detach() for k, v in m3(x).items()}
    torch.cuda.synchronize()
    ro = ref(x.double().cpu())
    rlosses = [F.cross_entropy(ro[k], y.cpu()) for k in AD.STAGES]
    sum(rlosses).backward()
    rows = [(f"loss.{k}", abs(float(losses[i]) - rlosses[i].item()) / abs(rlosses[i].item()), LOSS_PROBE) for i, k in enumerate(AD.STAGES)]
    rows += [(f"logits.{k}", AD.max_rel(out[k], ro[k]), TENSOR) for k in AD.STAGES]
    rg = dict(ref.named_parameters())
    rows += [(n, AD.max_rel(p.grad, rg[n].grad), TENSOR) for n, p in m.named_parameters() if p.requires_grad]
    assert len(rows) == 8 + 16
    _report(f"probe {shape} against float64", rows)
    _stats_close(m, ref)
    for i, k in enumerate(AD.STAGES):                                  # the hits are those of the float64 logits
        top = ro[k].topk(5, 1).indices
        assert hits[i].tolist() == [int((top[:, 0] == y.cpu()).sum()), int((top == y.cpu()[:, None]).any(1).sum())], k


def test_programs_reproduce_the_reference_fixture(gpu_device):
    """tests/golden/audio_downstream.npz: the reference's float32 CPU results for the seeded weight set, HipDropout's mask at
    the stored (seed, offset) standing where its nn.Dropout stood."""
    dev = gpu_device
    z = np.load(os.path.join(GOLDEN, "audio_downstream.npz"))
    x, y = torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["labels"]).to(dev)
    m = AD.cls_model(seed=int(z["weight_seed"])).to(dev).train()
    m.dropout.seed, m.dropout.offset = int(z["dropout_seed"]), int(z["dropout_offset"])
    loss, logits, grads, ref, _, _ = _finetune_against(dev, m, x, y, AD.restate)
    assert np.array_equal(ref.keep.numpy(), z["keep"])
    rows = [("loss", abs(float(loss) - float(z["cls.loss"])) / abs(float(z["cls.loss"])), LOSS_FT),
            ("logits", AD.max_rel(logits, torch.from_numpy(z["cls.logits"])), TENSOR)]
    rows += [(k, AD.max_rel(grads[k], torch.from_numpy(z[f"cls.grad.{k}"])), TENSOR)
             for k in ("classifier.weight", "classifier.bias", "feature_extractor.conv1.0.weight")]
    _report("finetune against the reference fixture", rows)
    pm = AD.probe_model(AD.SMALL, seed=int(z["weight_seed"])).to(dev).train()
    out = pm(x)
    assert all(type(v.grad_fn).__name__ == "ProbeFnBackward" for v in out.values())
    _report("probe against the reference fixture",
            [(k, AD.max_rel(out[k], torch.from_numpy(z[f"probe.logits.{k}"])), TENSOR) for k in AD.STAGES])


# ------------------------------------------------------------------------------------------------------------ 3. dense evaluation
def _dense_hits(logits64, labels, V, clips):
    conf = torch.softmax(logits64, 1).view(V, clips, -1).mean(1)
    top = conf.topk(5, 1).indices
    return conf, [int((top[:, 0] == labels).sum()), int((top == labels[:, None]).any(1).sum())]


def test_dense_evaluation_gives_the_float64_hits(gpu_device):
    from avid_hip import parallel
    dev, V, clips = gpu_device, 3, 5
    g = torch.Generator().manual_seed(8)
    x = torch.randn((V, clips) + AD.SMALL[1:], generator=g).to(dev)
    y = torch.randint(0, AD.N_CLASSES, (V,), generator=g).to(dev)
    x64, y_cpu = x.flatten(0, 1).double().cpu(), y.cpu()
    m = AD.cls_model().to(dev).train()
    conf, loss, hits = parallel.FinetuneStep(m).evaluate(x, y, batch=4)            # chunks of 4, 4, 4 and 3 clips
    assert m.training and conf.shape == (V, AD.N_CLASSES)
    with torch.no_grad():
        rl = AD.restate(m.eval())(x64)
    m.train()
    rconf, rhits = _dense_hits(rl, y_cpu, V, clips)
    rloss = F.cross_entropy(rl, y_cpu.repeat_interleave(clips))
    _report("dense evaluation, fine-tuning", [("conf", AD.max_rel(conf, rconf), TENSOR),
                                              ("loss", abs(float(loss) - float(rloss)) / float(rloss), LOSS_FT)])
    assert hits.tolist() == rhits
    pm = AD.probe_model(AD.SMALL).to(dev).train()
    conf, losses, hits = parallel.ProbeStep(pm).evaluate(x, y, batch=4)
    assert pm.training and conf.shape == (4, V, AD.N_CLASSES) and hits.shape == (4, 2)
    with torch.no_grad():
        ro = AD.restate(pm.eval(), AD.SMALL)(x64)
    pm.train()
    for i, k in enumerate(AD.STAGES):
        rconf, rhits = _dense_hits(ro[k], y_cpu, V, clips)
        rloss = F.cross_entropy(ro[k], y_cpu.repeat_interleave(clips))
        _report(f"dense evaluation, probe {k}", [("conf", AD.max_rel(conf[i], rconf), TENSOR),
                                                 ("loss", abs(float(losses[i]) - float(rloss)) / float(rloss), LOSS_PROBE)])
        assert hits[i].tolist() == rhits, k


# -------------------------------------------------------------------------------------------------------------- 4. virtual_ranks=2
def _shard_engine(dev, kind, **kw):
    """tests/test_gpu_virtual_downstream.py's one-rank ``Shard`` around the audio models."""
    import test_gpu_virtual_downstream as VD
    from avid_hip import parallel

    class AudioShard(VD.Shard):
        def __init__(self):
            self.kind = kind
            if kind == "finetune":
                self.m = AD.cls_model().to(dev).train()
                self.eng = parallel.FinetuneStep(self.m, **kw)
            else:
                self.m = AD.probe_model(AD.SMALL).to(dev).train()
                self.eng = parallel.ProbeStep(self.m, **kw)
    return VD, AudioShard()


def _batch8(dev, seed, steps):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((8,) + AD.SMALL[1:], generator=g).to(dev) for _ in range(steps)]
    ys = [torch.randint(0, AD.N_CLASSES, (8,), generator=g).to(dev) for _ in range(steps)]
    return xs, ys


@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
def test_virtual_finetune_step_is_the_two_shard_engines_sum(gpu_device, classifier_only):
    from avid_hip import ops, parallel
    dev, R, b = gpu_device, 2, 4
    VD, shard = _shard_engine(dev, "finetune", classifier_only=classifier_only)
    xs, ys = _batch8(dev, 9, 2)
    m = AD.cls_model().to(dev).train()
    m.dropout.seed = VD.BASE_SEED
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, virtual_ranks=R)
    n = eng.n_cls if classifier_only else eng.flat.numel
    VD._check_against_shards(eng, m, shard, xs, ys, R, b, n, seeds=VD._seeds(R))
    assert m.dropout.offset == 2
    ops.check_device_errors(dev)


def test_virtual_probe_step_is_the_two_shard_engines_sum(gpu_device):
    from avid_hip import ops, parallel
    dev, R, b = gpu_device, 2, 4
    VD, shard = _shard_engine(dev, "probe")
    xs, ys = _batch8(dev, 10, 2)
    m = AD.probe_model(AD.SMALL).to(dev).train()
    eng = parallel.ProbeStep(m, virtual_ranks=R)
    VD._check_against_shards(eng, m, shard, xs, ys, R, b, eng.flat.numel)
    assert tuple(eng.rank_losses.shape) == (R, 4) and tuple(eng.rank_hits.shape) == (R, 4, 2)
    ops.check_device_errors(dev)


def test_virtual_ranks_follow_the_two_shard_rule_in_float64(gpu_device):
    """tests/_dp_ref.py ``engine_rule``: per-shard BatchNorm statistics, the shards' gradients summed and taken with 1 / R, replica
    0's running statistics.  (Without dropout: the rule's module sees a shard, not its rank.)"""
    from avid_hip import parallel
    dev, R = gpu_device, 2
    (x,), (y,) = _batch8(dev, 11, 1)
    m = AD.cls_model(use_dropout=False).to(dev).train()
    ref = AD.restate(m)
    eng = parallel.FinetuneStep(m, virtual_ranks=R)
    loss, _ = eng.step(x, y)
    torch.cuda.synchronize()
    rgrads, rbufs, rloss = _dp_ref.engine_rule(ref, x.cpu(), y.cpu(), R)
    rows = [("loss", abs(float(loss) - float(rloss)) / abs(float(rloss)), LOSS_FT)]
    rows += [(n, AD.max_rel(p.grad / R, g), TENSOR) for (n, p), g in zip(m.named_parameters(), rgrads)]
    _report("FinetuneStep(virtual_ranks=2) against the two-shard rule", rows)
    whole = _dp_ref.whole_batch(ref, x.cpu(), y.cpu())[1]
    for n, b in m.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1, n
        else:
            torch.testing.assert_close(b.double().cpu(), rbufs[n], msg=n, **STATS)
    # ... which are replica 0's, not the whole batch's
    n = "feature_extractor.block4.bn2.running_mean"
    assert float((rbufs[n] - whole[n]).abs().max()) > 100 * STATS["atol"]


class _Tap(torch.nn.Module):
    """One tap of the float64 probe as the module tests/_dp_ref.py differentiates: the rule sums the gradient of EVERY parameter of
    its module, so the module's parameters are the head's, and the frozen tower (which has none to give) is held outside the module
    tree — already float64 and in training mode; every replica's deep copy gets its own, with its own running statistics."""

    def __init__(self, probe, i):
        super().__init__()
        self.head, self.tap, self._tower = probe.classifiers[i], AD.STAGES[i], (probe.feature_extractor,)

    def forward(self, x):
        with torch.no_grad():
            taps = self._tower[0](x, return_embs=True)
        return self.head(taps[self.tap])


def test_virtual_probe_ranks_follow_the_two_shard_rule_in_float64(gpu_device):
    """The same rule for ``ProbeStep(virtual_ranks=2)``, one tap at a time (the step's loss is the sum of the taps' cross-entropies
    and no head reads another's tap): the tower's BatchNorms AND the heads' BatchNorm1d normalise with their shard's 4 rows."""
    from avid_hip import parallel
    dev, R = gpu_device, 2
    (x,), (y,) = _batch8(dev, 16, 1)
    m = AD.probe_model(AD.SMALL).to(dev).train()
    ref = AD.restate(m, AD.SMALL)
    eng = parallel.ProbeStep(m, virtual_ranks=R)
    losses, _ = eng.step(x, y)
    torch.cuda.synchronize()
    ours, bufs = dict(m.named_parameters()), dict(m.named_buffers())
    for i, k in enumerate(AD.STAGES):
        tap = _Tap(ref, i)
        names = [n for n, _ in tap.named_parameters()]
        assert names == ["head.bn.weight", "head.bn.bias", "head.classifier.weight", "head.classifier.bias"]
        rgrads, rbufs, rloss = _dp_ref.engine_rule(tap, x.cpu(), y.cpu(), R)
        rows = [(f"loss.{k}", abs(float(losses[i]) - float(rloss)) / abs(float(rloss)), LOSS_PROBE)]
        rows += [(n, AD.max_rel(ours[f"classifiers.{i}.{n[5:]}"].grad / R, g), TENSOR) for n, g in zip(names, rgrads)]
        _report(f"ProbeStep(virtual_ranks=2) against the two-shard rule, {k}", rows)
        for n in ("running_mean", "running_var"):                      # replica 0's, of the head's BatchNorm1d
            torch.testing.assert_close(bufs[f"classifiers.{i}.bn.{n}"].double().cpu(), rbufs[f"head.bn.{n}"], msg=f"{k} {n}", **STATS)
        assert int(bufs[f"classifiers.{i}.bn.num_batches_tracked"]) == 1


# -------------------------------------------------------------------------------------------------------------------- 5. KNNEval
def test_knneval_on_the_audio_tower(gpu_device):
    from avid_hip import ops, parallel
    dev = gpu_device
    m = AD.tower_model().to(dev).eval()
    g = torch.Generator().manual_seed(12)
    gal = torch.randn((64,) + AD.SMALL[1:], generator=g).to(dev)
    gal_l = torch.randint(0, 5, (64,), generator=g).to(dev)
    q = torch.randn((8,) + AD.SMALL[1:], generator=g).to(dev)
    ql = torch.randint(0, 5, (8,), generator=g).to(dev)
    ev = parallel.KNNEval(model=m, n_classes=5, k=5)
    for i in range(0, 64, 16):
        ev.add_gallery(gal[i:i + 16], gal_l[i:i + 16])
    out = ev.evaluate(q, ql)
    assert ev._infer.used_programs is True
    infer = parallel.Inference(m)

    def feats(v):
        f = infer(v.contiguous())
        assert infer.used_programs is True and f.shape == (v.shape[0], 512, 1, 1)
        return ops.l2_normalize(f.flatten(1).contiguous())
    G = torch.cat([feats(gal[i:i + 16]) for i in range(0, 64, 16)])
    assert torch.equal(ev.gallery()[0], G) and torch.equal(ev.gallery()[1], gal_l.to(torch.int32))
    Q = feats(q)
    idx, sim = _knn_ref.search(G.cpu().numpy(), Q.cpu().numpy(), 5)
    _, p5, first = _knn_ref.vote(idx, sim, gal_l.cpu().numpy(), 5, T=0.07, query_labels=ql.cpu().numpy())
    lab = ql.cpu().numpy()
    want = (8, int((p5[:, 0] == lab).sum()), int((p5 == lab[:, None]).any(1).sum()), {r: int((first < r).sum()) for r in (1, 5)})
    got = (int(out["n"]), int(out["top1_hits"]), int(out["top5_hits"]), {r: int(v) for r, v in out["recall_hits"].items()})
    assert got == want
    assert not any(mod.training for mod in m.modules())


# --------------------------------------------------------------------------------------------------------------------- 6. guards
def _guard_finetune(dev, P):
    from avid_hip import parallel
    m = AD.cls_model().to(dev).train()
    eng = parallel.FinetuneStep(m)
    (x,), (y,) = _data(AD.ODD, dev, 13)
    loss, hits = eng.step(P(x), P(y))
    torch.cuda.synchronize()
    res = {"loss": loss, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat, "adam_m": eng.m, "adam_v": eng.v}
    res.update({f"buffer:{n}": b for n, b in m.named_buffers()})
    return res


def _guard_probe(dev, P):
    from avid_hip import parallel
    m = AD.probe_model(AD.ODD).to(dev).train()
    eng = parallel.ProbeStep(m)
    (x,), (y,) = _data(AD.ODD, dev, 14)
    losses, hits = eng.step(P(x), P(y))
    torch.cuda.synchronize()
    res = {"losses": losses, "hits": hits, "grad": eng.flat.grad, "params": eng.flat.flat, "adam_m": eng.m, "adam_v": eng.v}
    res.update({f"buffer:{n}": b for n, b in m.named_buffers()})
    return res


def _guard_inference(dev, P):
    from avid_hip import parallel
    (x,), _ = _data(AD.ODD, dev, 15)
    x = P(x)
    res = {}
    for name, m in (("tower", AD.tower_model()), ("cls", AD.cls_model()), ("probe", AD.probe_model(AD.ODD))):
        inf = parallel.Inference(m.to(dev).eval())
        out = inf(x)
        assert inf.used_programs is True, name
        res.update({f"{name}.{k}": v for k, v in out.items()} if isinstance(out, dict) else {name: out})
    torch.cuda.synchronize()
    return res


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


@pytest.mark.parametrize("case", [_guard_finetune, _guard_probe, _guard_inference], ids=["finetune_step", "probe_step", "inference"])
def test_audio_programs_under_guards(gpu_device, case):
    """tests/test_gpu_guards.py's rule for the video programs: (a) no byte of any guard band changes, (b) every result is the
    same bits under both fills of unwritten memory, and the same as without guards."""
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
        assert g.programs, "no launch program was sealed under the guards"
        for ws_bytes, numel, passed, needs in g.programs:
            want = [max(n[k] for n in needs) for k in range(4)]
            assert needs and ws_bytes == want and numel == want and passed == want
    ff, fa = runs
    assert set(ff) == set(fa) == set(plain)
    for k in plain:
        assert torch.equal(ff[k], fa[k]), f"'{k}' depends on unwritten memory"
        assert torch.equal(ff[k], plain[k]), f"'{k}' differs under guards"
