"""Host side of action-recognition fine-tuning (no GPU): the classifier's launch programs compile at the shipped per-GPU
shapes with every reference in bounds and one gradient per parameter in the FlatParams layout, the warm-up programs hold no
tower backward, a hooked or pooled wrapper falls back to the per-layer path, the wrapper's state dict is the reference's,
the launcher puts this package ahead of a script's directory, and the new kernels neither spill nor use scratch."""
import json
import os
import subprocess
import sys
import textwrap

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "avid-cma_amd")
SHAPES = [(8, 3, 8, 224, 224), (4, 3, 32, 224, 224)]


def _wrapper(n_classes=101, **kw):
    import models
    torch.manual_seed(0)
    args = dict(feat_name="pool", feat_dim=512, pooling_op=None, use_dropout=True, dropout=0.5)
    args.update(kw)
    return models.ClassificationWrapper(models.R2Plus1D(18), n_classes, **args).train()


@pytest.fixture(scope="module")
def wrapper():
    return _wrapper()


@pytest.fixture(scope="module", params=SHAPES, ids=["8x8", "4x32"])
def compiled(request, wrapper):
    from avid_hip import plan
    full = plan.ClsPlan(wrapper, request.param, torch.device("cpu"), True, True, False)
    warm = plan.ClsPlan(wrapper, request.param, torch.device("cpu"), True, True, True)
    return wrapper, full, warm


def _ops(pl, prog, n):
    return [prog[k].op for k in range(n)]


def test_programs_stay_in_bounds(compiled):
    from avid_hip import plan
    _, full, warm = compiled
    for pl in (full, warm):
        B, C = pl.vshape[0], pl.n_classes
        size = {plan.S_FWD: pl.fa_bytes, plan.S_BWD: pl.ba_bytes, plan.S_GRAD: 4 * pl.gnumel, plan.S_AUX: pl.aux_bytes,
                plan.S_DLOGITS: 4 * B * C, plan.S_OUT: plan.OUT_BYTES, plan.S_LABELS: 8 * B}
        for prog, n in ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)):
            for k in range(n):
                r = prog[k]
                assert 0 <= r.op <= 22 and 0 <= r.stream < 4
                for j in range(plan.NREF):
                    s, off = r.t[j].slot, r.t[j].off
                    assert -1 <= s < pl.n_slots
                    if s in size:
                        assert 0 <= off < size[s], (k, j, s, off)
                    elif s >= 0:
                        assert off == 0


def test_each_parameter_gets_one_gradient_in_flatparams_layout(compiled):
    from avid_hip.parallel import FlatParams
    m, full, warm = compiled
    seen = [i for _, _, ps in full.grad_ready for i in ps]
    assert sorted(seen) == list(range(len(full.params))) == list(range(sum(1 for _ in m.parameters())))
    m2 = _wrapper()
    flat = FlatParams(m2)
    assert list(flat.offsets) == list(full.goff) and flat.numel == full.gnumel
    # the warm-up programs: the classifier's two parameters only, which lead the buffer
    seen = sorted(i for _, _, ps in warm.grad_ready for i in ps)
    assert seen == [0, 1] and warm.params[0] is m.classifier.bias and warm.params[1] is m.classifier.weight
    assert warm.n_cls == full.goff[2]


def test_one_dropout_and_loss_record_each(compiled):
    from avid_hip import plan
    _, full, _ = compiled
    fwd, bwd = _ops(full, full.fwd_prog, full.n_fwd), _ops(full, full.bwd_prog, full.n_bwd)
    assert fwd.count(plan.OP_DROPOUT_FWD) == 1 and bwd.count(plan.OP_DROPOUT_BWD) == 1
    assert (fwd + bwd).count(plan.OP_CLS_LOSS) == 1
    assert fwd[-1] == plan.OP_CLS_LOSS and full.n_logits == full.n_fwd - 1
    r = full.fwd_prog[full.n_fwd - 1]
    assert r.t[5].slot == plan.S_DLOGITS and r.t[2].slot == plan.S_OUT and r.t[1].slot == plan.S_LABELS
    assert list(r.i)[:3] == [full.vshape[0], 1, 101]
    # the backward starts from dlogits: its first launch reads them
    first = full.bwd_prog[next(k for k in range(full.n_bwd) if full.bwd_prog[k].op != plan.OP_WAIT)]
    assert first.op == plan.OP_CLS_LINEAR_BWD and first.t[2].slot == plan.S_DLOGITS and first.t[3].slot == plan.S_BWD
    assert (fwd + bwd).count(plan.OP_CLS_LINEAR_FWD) == 1 and bwd.count(plan.OP_CLS_LINEAR_BWD) == 1


def test_classifier_only_backward_has_no_tower_convolutions(compiled):
    from avid_hip import plan
    _, full, warm = compiled
    ops_w = _ops(warm, warm.bwd_prog, warm.n_bwd)
    assert plan.OP_CONV_DGRAD not in ops_w and plan.OP_DROPOUT_BWD not in ops_w
    assert plan.OP_BN_BWD not in ops_w and plan.OP_BN_POOL_BWD not in ops_w
    assert plan.OP_CONV_WGRAD not in ops_w and plan.OP_WGRAD_GROUP not in ops_w
    launches = [op for op in ops_w if op != plan.OP_WAIT]
    assert launches == [plan.OP_CLS_LINEAR_BWD]              # the classifier's own weight and bias gradients, no input gradient
    r = next(warm.bwd_prog[k] for k in range(warm.n_bwd) if warm.bwd_prog[k].op == plan.OP_CLS_LINEAR_BWD)
    assert r.t[3].slot == -1 and list(r.i)[:3] == [warm.vshape[0], 512, 101]
    assert warm.fwd_prog[warm._zero_index].n[0] == 4 * warm.n_cls
    assert _ops(warm, warm.fwd_prog, warm.n_fwd) == _ops(full, full.fwd_prog, full.n_fwd)


def test_hooked_eval_pooled_or_other_features_fall_back():
    from avid_hip import plan
    dev = torch.device("cpu")
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(_wrapper(pooling_op="AdaptiveMaxPool3d((1, 1, 1))"), SHAPES[0], dev, True, True)
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(_wrapper(feat_name="conv5x", feat_dim=512 * 7 * 7), SHAPES[0], dev, True, True)
    m = _wrapper()
    assert plan.eligible(m, torch.zeros(1, 3, 8, 16, 16)) is False                      # CPU tensor
    # the module-tree rule (the device checks aside): any hook, on the classifier or inside the tower, or eval mode
    assert plan._tree_ok(m)
    for mod in (m.classifier, m.feature_extractor.conv3x[1].spt_bn1):
        for reg in (mod.register_forward_hook, mod.register_forward_pre_hook):
            h = reg(lambda *a: None)
            assert not plan._tree_ok(m), (type(mod).__name__, reg.__name__)
            h.remove()
            assert plan._tree_ok(m)
    h = m.classifier.register_full_backward_hook(lambda *a: None)
    assert not plan._tree_ok(m)
    h.remove()
    m.eval()
    assert not plan._tree_ok(m)
    assert plan.run_cls(m, torch.zeros(1, 3, 8, 16, 16)) is None                         # evaluation
    m.train()
    # the classifier is a module of its own type: hooks on it run on the per-layer path; anything else is not compiled
    from models.classification import ClsLinear
    from models.av_wrapper import LinearCL
    assert type(m.classifier) is ClsLinear
    m2 = _wrapper()
    m2.classifier = LinearCL(512, 101)
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(m2, SHAPES[0], dev, True, True)


def test_state_dict_keys_match_the_reference_fixture():
    ref = json.load(open(os.path.join(REPO, "tests", "golden", "cls_wrapper_keys.json")))["state_dict"]
    m = _wrapper()
    mine = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert mine == ref
    assert [k for k, _ in m.named_parameters()][-2:] == ["classifier.weight", "classifier.bias"]


def test_classifier_init_and_dropout_seed_follow_torch_manual_seed():
    a, b = _wrapper(), _wrapper()
    assert a.dropout.seed == b.dropout.seed and torch.equal(a.classifier.weight, b.classifier.weight)
    torch.manual_seed(0)
    import models
    fe = models.R2Plus1D(18)
    lin = torch.nn.Linear(512, 101)
    assert torch.equal(lin.weight, a.classifier.weight) and torch.equal(lin.bias, a.classifier.bias)
    assert "dropout.seed" not in a.state_dict() and a.dropout.offset == 0
    assert a.eval().dropout(torch.ones(2, 3)).equal(torch.ones(2, 3))                   # identity in eval mode
    del fe


def _standin(tmp_path):
    """A stand-in reference checkout: utils/eval_utils.py with a ClassificationWrapper of its own, a models package, a script
    that reports what it resolved."""
    ref = tmp_path / "ref"
    (ref / "utils").mkdir(parents=True)
    (ref / "models").mkdir()
    (ref / "utils" / "__init__.py").write_text("")
    (ref / "utils" / "eval_utils.py").write_text(textwrap.dedent("""
        import torch

        class ClassificationWrapper(torch.nn.Module):
            marker = "stand-in"

        def build_model():
            return ClassificationWrapper
    """))
    (ref / "models" / "__init__.py").write_text("")
    (ref / "eval_script.py").write_text(textwrap.dedent("""
        import json, sys
        import models
        from utils import eval_utils
        cls = eval_utils.build_model()
        print(json.dumps({"cls_module": cls.__module__, "marker": getattr(cls, "marker", None), "models": models.__file__,
                          "argv": sys.argv[1:], "name": __name__}))
    """))
    return ref


def _run_launcher(ref, env_extra):
    env = dict(os.environ)
    env["PYTHONPATH"] = PKG
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-m", "avid_hip.run_reference", str(ref / "eval_script.py"), "--cfg", "x"],
                         cwd=str(ref), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_launcher_puts_this_package_first(tmp_path):
    ref = _standin(tmp_path)
    got = _run_launcher(ref, {"AVID_DROPIN": "1"})
    assert got["cls_module"] == "models.classification" and got["marker"] is None
    assert os.path.dirname(os.path.abspath(got["models"])) == os.path.join(PKG, "models")
    assert got["argv"] == ["--cfg", "x"] and got["name"] == "__main__"
    off = _run_launcher(ref, {"AVID_DROPIN": "0"})
    assert off["marker"] == "stand-in"


def test_new_kernels_spill_nothing():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_table
    rows = [r for r in kernel_table() if any(k in r["name"] for k in ("dropout_fwd_kernel", "dropout_bwd_kernel", "cls_loss_kernel",
                                                                       "cls_linear_fwd_kernel", "cls_linear_bwd_kernel"))]
    assert len(rows) == 5, [r["name"] for r in rows]
    for r in rows:
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["private_segment_fixed_size"] == 0 and not r["uses_dynamic_stack"], r


def test_new_entry_points_and_opcodes():
    from avid_hip import lib, plan
    for s in ("avid_dropout_fwd", "avid_dropout_bwd", "avid_cls_loss", "avid_cls_linear_fwd", "avid_cls_linear_bwd"):
        assert s in lib.SIGNATURES
    assert (plan.OP_DROPOUT_FWD, plan.OP_DROPOUT_BWD, plan.OP_CLS_LOSS, plan.OP_CLS_LINEAR_FWD, plan.OP_CLS_LINEAR_BWD) == \
        (18, 19, 20, 21, 22)
    assert plan._OP_NAMES[18] == "dropout_fwd" and plan._OP_NAMES[20] == "cls_loss"
    # a CPU tensor is refused, there is no fallback
    from avid_hip import ops, AvidHipError
    with pytest.raises(AvidHipError):
        ops.dropout(torch.zeros(2, 4), 0.5, 1, 0)
    with pytest.raises(AvidHipError):
        ops.cls_loss(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(AvidHipError):
        ops.cls_linear(torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(3))
