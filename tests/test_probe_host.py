"""Host side of the linear probe (no GPU): MOSTModel's state dict is the reference's, ``train()`` flips the tower as the
reference's does, the probe's launch programs compile at the shipped shape with every reference in bounds and a backward
that holds head records only, a hooked / eval-mode / l2-normalised model yields no plan, the pooling window rule is torch's,
``utils.eval_utils`` resolves MOSTModel here, and the heads reproduce the reference-generated fixture on the torch path."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "avid-cma_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
SHIPPED = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
               pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                            "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)
SHAPE = (128, 3, 8, 224, 224)


def _model(**kw):
    import models
    torch.manual_seed(0)
    args = dict(SHIPPED)
    args.update(kw)
    return models.MOSTModel(models.R2Plus1D(18), **args)


@pytest.fixture(scope="module")
def compiled():
    from avid_hip import plan
    m = _model().train()
    return m, plan.ProbePlan(m, SHAPE, torch.device("cpu"), True, True)


def test_state_dict_keys_match_the_reference_fixture():
    ref = json.load(open(os.path.join(GOLDEN, "most_model_keys.json")))
    assert ref["args"] == SHIPPED
    m = _model()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == ref["state_dict"]
    # the reference's attributes, and its initialisation order under one seed (BatchNorm1d, then Linear, per head)
    assert m.feat_names == SHIPPED["feat_names"] and m.feat_dims == SHIPPED["feat_dims"] and m.l2_norm == [False] * 4
    assert m.pooling_ops == SHIPPED["pooling_ops"] and [c.feat_name for c in m.classifiers] == SHIPPED["feat_names"]
    import models
    torch.manual_seed(0)
    models.R2Plus1D(18)
    lin = [nn.Linear(d, 400) for d in SHIPPED["feat_dims"]]
    for c, l in zip(m.classifiers, lin):
        assert torch.equal(c.classifier.weight, l.weight) and torch.equal(c.classifier.bias, l.bias)
        assert isinstance(c.bn, nn.BatchNorm1d) and isinstance(c.classifier, nn.Linear) and isinstance(c.pooling, nn.AdaptiveMaxPool3d)


def test_train_flips_the_tower_as_the_reference_does():
    m = _model()
    assert not m.feature_extractor.training and m.training            # the constructor: feature_extractor.train(False)
    assert all(not p.requires_grad for p in m.feature_extractor.parameters())
    assert all(p.requires_grad for p in m.classifiers.parameters())
    m.train(True)
    assert all(mod.training for mod in m.modules())                   # nn.Module.train: the tower's BatchNorms are back on batch statistics
    m.train(False)
    assert not any(mod.training for mod in m.modules())
    assert type(m).train is nn.Module.train


def test_programs_stay_in_bounds(compiled):
    from avid_hip import plan
    m, pl = compiled
    B, C, n = SHAPE[0], 400, 4
    size = {plan.S_FWD: pl.fa_bytes, plan.S_BWD: pl.ba_bytes, plan.S_GRAD: 4 * pl.gnumel, plan.S_AUX: pl.aux_bytes,
            plan.S_DLOGITS: 4 * B * C * n, plan.S_OUT: plan.PROBE_OUT_BYTES * n, plan.S_LABELS: 8 * B}
    for prog, cnt in ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)):
        for k in range(cnt):
            r = prog[k]
            assert 0 <= r.op <= 27 and r.op in plan._OP_NAMES and 0 <= r.stream < 4
            for j in range(plan.NREF):
                s, off = r.t[j].slot, r.t[j].off
                assert -1 <= s < pl.n_slots
                if s in size:
                    assert 0 <= off < size[s], (k, j, s, off)
                elif s >= 0:
                    assert off == 0
    # the loss records: one per tap, each with its own 32 bytes of S_OUT and its own [B, C] of dlogits
    loss = [pl.fwd_prog[k] for k in range(pl.n_logits, pl.n_fwd)]
    assert [r.op for r in loss] == [plan.OP_CLS_LOSS] * 4
    assert [(r.t[2].off, r.t[4].off, r.t[5].off) for r in loss] == [(32 * i, 32 * i + 8, 4 * B * C * i) for i in range(4)]
    fwd = [pl.fwd_prog[k].op for k in range(pl.n_logits)]
    for op in (plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_PROBE_LINEAR_FWD):
        assert fwd.count(op) == 4
    assert plan.OP_CLS_LINEAR_FWD not in fwd and plan.OP_GPOOL_FWD in fwd
    pools = [pl.fwd_prog[k] for k in range(pl.n_logits) if pl.fwd_prog[k].op == plan.OP_ADAPTIVE_MAXPOOL]
    assert [(list(r.i)[:5], (r.d.To, r.d.Ho, r.d.Wo)) for r in pools] == [
        ([128, 8, 56, 56, 64], (1, 12, 12)), ([128, 4, 28, 28, 128], (1, 8, 8)), ([128, 2, 14, 14, 256], (1, 6, 6)),
        ([128, 1, 7, 7, 512], (1, 4, 4))]


def test_backward_holds_head_records_only(compiled):
    from avid_hip import plan
    from avid_hip.parallel import FlatParams
    m, pl = compiled
    ops_b = [pl.bwd_prog[k].op for k in range(pl.n_bwd) if pl.bwd_prog[k].op != plan.OP_WAIT]
    assert ops_b == [plan.OP_PROBE_LINEAR_BWD, plan.OP_BN1D_BWD] * 4
    # the gradient buffer is the classifiers' slice: FlatParams over the trainable parameters, every one written once
    heads = list(m.classifiers.parameters())
    assert len(pl.params) == len(heads) == 16 and {id(p) for p in pl.params} == {id(p) for p in heads}
    assert pl.gnumel == sum((p.numel() + 3) // 4 * 4 for p in heads)
    assert sorted(i for _, _, ps in pl.grad_ready for i in ps) == list(range(16))
    flat = FlatParams(_model())
    assert list(flat.offsets) == list(pl.goff) and flat.numel == pl.gnumel
    written = []
    for k in range(pl.n_bwd):
        r = pl.bwd_prog[k]
        if r.op == plan.OP_BN1D_BWD:
            assert r.t[4].slot == -1                                  # no input gradient: the pooled features are constants
        written += [r.t[j].off for j in range(plan.NREF) if r.t[j].slot == plan.S_GRAD]
    assert sorted(written) == [4 * o for o in sorted(pl.goff)]
    assert pl.fwd_prog[pl._zero_index].n[0] == 4 * pl.gnumel


def test_hooked_eval_or_other_heads_yield_no_plan():
    from avid_hip import plan
    dev = torch.device("cpu")
    small = (4, 3, 8, 64, 64)
    plan.ProbePlan(_model().train(), small, dev, True, True)            # the stock model compiles at the test geometry too
    for kw in (dict(l2_norm=True), dict(use_bn=False), dict(use_dropout=True),
               dict(pooling_ops=["AdaptiveAvgPool3d((1,12,12))"] + SHIPPED["pooling_ops"][1:]),
               dict(feat_names=["conv1"] + SHIPPED["feat_names"][1:])):
        with pytest.raises(plan.Unsupported):
            plan.ProbePlan(_model(**kw).train(), small, dev, True, True)
    m = _model().train()
    for p in m.feature_extractor.conv5x.parameters():
        p.requires_grad = True
    with pytest.raises(plan.Unsupported):
        plan.ProbePlan(m, small, dev, True, True)
    m = _model().train()
    assert plan._tree_ok(m)
    assert plan.run_probe(m, torch.zeros(small)) is None                # CPU tensor
    h = m.classifiers[2].bn.register_forward_hook(lambda *a: None)
    assert not plan._tree_ok(m)
    h.remove()
    m.feature_extractor.eval()                                          # a tower put in eval mode by hand
    assert not plan._tree_ok(m)
    m.eval()
    assert not plan.eligible(m, torch.zeros(small))


def test_window_rule_is_torchs():
    from avid_hip import ops

    def pool(x, out):       # x [B, C, T, H, W]
        y = torch.empty(x.shape[:2] + tuple(out))
        for t in range(out[0]):
            t0, t1 = ops.adaptive_window(t, x.shape[2], out[0])
            for h in range(out[1]):
                h0, h1 = ops.adaptive_window(h, x.shape[3], out[1])
                for w in range(out[2]):
                    w0, w1 = ops.adaptive_window(w, x.shape[4], out[2])
                    y[:, :, t, h, w] = x[:, :, t0:t1, h0:h1, w0:w1].amax((2, 3, 4))
        return y
    g = torch.Generator().manual_seed(0)
    for shape, out in (((8, 56, 56), (1, 12, 12)), ((4, 28, 28), (1, 8, 8)), ((2, 14, 14), (1, 6, 6)), ((1, 7, 7), (1, 4, 4)),
                       ((8, 16, 16), (1, 12, 12)), ((4, 8, 8), (1, 8, 8)), ((2, 4, 4), (1, 6, 6)), ((1, 2, 2), (1, 4, 4)),
                       ((1, 2, 2), (2, 4, 4)), ((3, 7, 9), (2, 3, 4))):
        x = torch.randn((2, 3) + shape, generator=g)
        assert torch.equal(pool(x, out), nn.AdaptiveMaxPool3d(out)(x)), (shape, out)
    # 64 x 64 clips give the real head sizes from the same pooling ops (two of them pool to more outputs than positions)
    for (c, t, s), p, d in zip(((64, 8, 16), (128, 4, 8), (256, 2, 4), (512, 1, 2)), SHIPPED["pooling_ops"], SHIPPED["feat_dims"]):
        assert eval("nn." + p)(torch.zeros(1, c, t, s, s)).numel() == d


def _standin(tmp_path):
    ref = tmp_path / "ref"
    (ref / "utils").mkdir(parents=True)
    (ref / "models").mkdir()
    (ref / "utils" / "__init__.py").write_text("")
    (ref / "utils" / "eval_utils.py").write_text(textwrap.dedent("""
        import torch

        class ClassificationWrapper(torch.nn.Module):
            marker = "stand-in"

        class Classifier(torch.nn.Module):
            marker = "stand-in"

        class MOSTModel(torch.nn.Module):
            marker = "stand-in"

        class MOSTCheckpointManager(object):
            marker = "stand-in"

        def build_model():
            return MOSTModel, Classifier, MOSTCheckpointManager
    """))
    (ref / "models" / "__init__.py").write_text("")
    (ref / "eval_script.py").write_text(textwrap.dedent("""
        import json
        from utils import eval_utils
        most, cls, ckp = eval_utils.build_model()
        print(json.dumps({"most": [most.__module__, getattr(most, "marker", None)],
                          "cls": [cls.__module__, getattr(cls, "marker", None)], "ckp": getattr(ckp, "marker", None)}))
    """))
    return ref


def _run_launcher(ref, env_extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-m", "avid_hip.run_reference", str(ref / "eval_script.py")],
                         cwd=str(ref), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_eval_utils_resolves_the_probe_model_here(tmp_path):
    ref = _standin(tmp_path)
    on = _run_launcher(ref, {"AVID_DROPIN": "1"})
    assert on["most"] == ["models.linear_probe", None] and on["cls"] == ["models.linear_probe", None]
    assert on["ckp"] == "stand-in"                                      # the checkpoint manager stays the reference's
    off = _run_launcher(ref, {"AVID_DROPIN": "0"})
    assert off["most"][1] == "stand-in" and off["cls"][1] == "stand-in"


def test_heads_reproduce_the_reference_fixture_on_the_torch_path():
    import models
    z = np.load(os.path.join(GOLDEN, "most_heads.npz"))
    names = [k[4:] for k in z.files if k.startswith("tap.")]

    class Stub(nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = nn.Parameter(torch.ones(1))

        def forward(self, x, return_embs=False):
            return {n: torch.from_numpy(z[f"tap.{n}"]) for n in names}

    pools = {"a": "AdaptiveMaxPool3d((1,2,2))", "b": "AdaptiveMaxPool3d((1,4,4))", "c": "AdaptiveMaxPool3d((2,2,3))"}
    dims = [z[f"init.{i}.classifier.weight"].shape[1] for i in range(len(names))]
    m = models.MOSTModel(Stub(), 7, names, dims, [pools[n] for n in names], use_bn=True)
    m.classifiers.load_state_dict({k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init.")})
    m.train()
    out = m(torch.zeros(4, 3, 1, 1, 1))
    assert list(out) == names
    labels = torch.from_numpy(z["labels"])
    loss = sum(F.cross_entropy(out[n], labels) for n in names)
    loss.backward()
    np.testing.assert_allclose(loss.item(), float(z["loss"]), rtol=1e-5)
    for n in names:
        np.testing.assert_allclose(out[n].detach().numpy(), z[f"logits.{n}"], rtol=1e-4, atol=1e-5)
    for k, p in m.classifiers.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), z[f"grad.{k}"], rtol=1e-4, atol=1e-6, err_msg=k)
    for k, v in m.classifiers.state_dict().items():
        if "running" in k or "num_batches" in k:
            np.testing.assert_allclose(v.numpy(), z[f"after.{k}"], rtol=1e-5, atol=1e-6, err_msg=k)
    assert m.feature_extractor.scale.grad is None and not m.feature_extractor.scale.requires_grad


def test_new_entry_points_opcodes_and_kernels():
    from avid_hip import lib, plan, ops, AvidHipError
    for s in ("avid_adaptive_maxpool_fwd", "avid_bn1d_fwd_train", "avid_bn1d_fwd_eval", "avid_bn1d_bwd",
              "avid_probe_linear_workspace_bytes", "avid_probe_linear_fwd", "avid_probe_linear_bwd"):
        assert s in lib.SIGNATURES
    assert lib.version() >= 140
    assert (plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_BN1D_BWD, plan.OP_PROBE_LINEAR_FWD,
            plan.OP_PROBE_LINEAR_BWD) == (23, 24, 25, 26, 27)
    assert [plan._OP_NAMES[k] for k in range(23, 28)] == ["adaptive_maxpool", "bn1d_fwd", "bn1d_bwd", "probe_linear_fwd",
                                                          "probe_linear_bwd"]
    # the workspace covers the K-split partial tiles of the forward (18 slices of 512 at 9216 features) and of dx
    ws = lib.raw("avid_probe_linear_workspace_bytes")
    assert ws(128, 9216, 400) == 4 * 18 * 128 * 400 and ws(3, 100, 7) == 0 and ws(256, 16384, 1000) == 4 * 2 * 256 * 16384
    assert ws(257, 64, 8) == 0 and lib.raw("avid_probe_linear_fwd")(257, 64, 8, None, None, None, None, None, 0, None) < 0
    # CPU tensors are refused by the ops: there is no fallback inside them
    for call in (lambda: ops.adaptive_maxpool(torch.zeros(1, 1, 2, 2, 4), (1, 1, 1)),
                 lambda: ops.probe_linear(torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(3)),
                 lambda: ops.bn1d(torch.zeros(2, 4), torch.ones(4), torch.zeros(4), torch.zeros(4), torch.ones(4), True)):
        with pytest.raises(AvidHipError):
            call()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_table
    rows = [r for r in kernel_table() if any(k in r["name"] for k in ("adaptive_maxpool", "bn1d_", "probe_gemm_kernel",
                                                                       "probe_reduce_kernel", "probe_colsum_kernel"))]
    assert len(rows) == 10, [r["name"] for r in rows]
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0 and not r["uses_dynamic_stack"], r
