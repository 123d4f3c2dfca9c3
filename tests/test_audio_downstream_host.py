"""Host side of the audio tower's downstream programs (no GPU): fine-tuning, linear-probe and inference plans around ``Conv2D``
compile on the host at the three test geometries with every reference in bounds; the record sequence is tower, dropout,
classifier, loss, and a backward that starts at the classifier and writes every trainable parameter's gradient slice exactly once;
``classifier_only`` leaves one launching backward record; a probe program holds no tower backward; mixed and unknown forms stay
refused; the state dicts are the reference's (tests/golden/audio_downstream_keys.json, tools/make_audio_downstream_golden.py);
and the pure-torch restatement the GPU tests hold the kernels to reproduces the reference's fixture in float64."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _audio_downstream as AD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CPU = torch.device("cpu")
SHAPES = [AD.SMALL, AD.ODD, AD.SHIPPED]
IDS = ["4x64x65", "3x50x33", "4x200x257"]
# tap geometry [H, W, C] per stage behind the 7x7 / 2 stem and the blocks' strides 2, 2, 2, 1
TAPS = {AD.SMALL: [(16, 17, 64), (8, 9, 128), (4, 5, 256), (4, 5, 512)],
        AD.ODD: [(13, 9, 64), (7, 5, 128), (4, 3, 256), (4, 3, 512)],
        AD.SHIPPED: [(50, 65, 64), (25, 33, 128), (13, 17, 256), (13, 17, 512)]}


def _cls_plan(shape, classifier_only=False, **kw):
    from avid_hip import plan
    m = AD.cls_model(**kw).train()
    return m, plan.ClsPlan(m, shape, CPU, True, True, classifier_only)


def _probe_plan(shape, **kw):
    from avid_hip import plan
    m = AD.probe_model(shape, **kw).train()
    return m, plan.ProbePlan(m, shape, CPU, True, True)


def _ops(prog, n, skip_wait=True):
    from avid_hip import plan
    return [prog[k].op for k in range(n) if not (skip_wait and prog[k].op in (0, plan.OP_WAIT))]


def _in_bounds(pl, progs, size):
    from avid_hip import plan
    for prog, cnt in progs:
        for k in range(cnt):
            r = prog[k]
            assert r.op in plan._OP_NAMES and 0 <= r.stream < 4
            for j in range(plan.NREF):
                s, off = r.t[j].slot, r.t[j].off
                assert -1 <= s < pl.n_slots
                if s in size:
                    assert 0 <= off < size[s], (k, j, s, off)
                elif s >= 0:
                    assert off == 0


# ------------------------------------------------------------------------------------------------------------ fine-tuning
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cls_plan_compiles_with_the_record_sequence(shape):
    """The plan of the issue's first case — ``ClsPlan(ClassificationWrapper(Conv2D(), 50, "pool", 512, use_dropout=True).train(),
    (4, 1, 64, 65), cpu, True, True)`` — and of the other two geometries."""
    from avid_hip import plan
    from avid_hip.parallel import FlatParams
    m, pl = _cls_plan(shape)
    B = shape[0]
    assert pl.vshape == shape and pl.ashape is None and pl.n_classes == 50
    size = {plan.S_FWD: pl.fa_bytes, plan.S_BWD: pl.ba_bytes, plan.S_GRAD: 4 * pl.gnumel, plan.S_AUX: pl.aux_bytes,
            plan.S_VIDEO: 4 * B * shape[2] * shape[3], plan.S_LABELS: 8 * B, plan.S_DLOGITS: 4 * B * 50, plan.S_OUT: plan.OUT_BYTES}
    _in_bounds(pl, ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)), size)
    # forward: the tower's nine convolution + BatchNorm pairs and its global max pool, dropout, the classifier; the loss record
    # at n_logits
    fwd = _ops(pl.fwd_prog, pl.n_logits)
    tower = [plan.OP_CONV_FWD, plan.OP_BN_FWD] * 9 + [plan.OP_GPOOL_FWD]
    assert fwd == [plan.OP_MEMSET0, plan.OP_WT_BATCH] + tower + [plan.OP_DROPOUT_FWD, plan.OP_CLS_LINEAR_FWD]
    assert pl.n_fwd == pl.n_logits + 1 and pl.fwd_prog[pl.n_logits].op == plan.OP_CLS_LOSS
    assert pl.drop_index is not None and pl.fwd_prog[pl.drop_index].op == plan.OP_DROPOUT_FWD
    # the input: slot S_VIDEO read as [B, 1, 1, T, F] by the channel-first stem, and by nothing else in the forward
    convs = [pl.fwd_prog[k] for k in range(pl.n_logits) if pl.fwd_prog[k].op == plan.OP_CONV_FWD]
    d = convs[0].d
    assert (convs[0].t[0].slot, convs[0].t[0].off) == (plan.S_VIDEO, 0)
    assert (d.B, d.Ti, d.Hi, d.Wi, d.Cin, d.kt, d.kh, d.kw) == (B, 1, shape[2], shape[3], 1, 1, 7, 7)
    assert all(r.t[0].slot == plan.S_FWD for r in convs[1:])
    assert [(r.d.Ho, r.d.Wo, r.d.Cout) for r in convs[2::2]] == TAPS[shape]
    assert not any(pl.fwd_prog[k].t[j].slot == plan.S_AUDIO for k in range(pl.n_logits) for j in range(plan.NREF))
    loss = pl.fwd_prog[pl.n_logits]
    assert (loss.t[1].slot, loss.t[2].slot, loss.t[5].slot) == (plan.S_LABELS, plan.S_OUT, plan.S_DLOGITS)
    # backward: starts at the classifier, then dropout, the pool, and the tower's layers — every trainable parameter's slice of
    # the gradient buffer is written exactly once
    bwd = _ops(pl.bwd_prog, pl.n_bwd)
    assert bwd[:3] == [plan.OP_CLS_LINEAR_BWD, plan.OP_DROPOUT_BWD, plan.OP_GPOOL_BWD]
    assert bwd.count(plan.OP_BN_BWD) == 9 and bwd.count(plan.OP_CONV_DGRAD) == 8        # (no input gradient of the stem)
    assert bwd.count(plan.OP_CONV_WGRAD) + bwd.count(plan.OP_WGRAD_ITEM) == 9
    flat = FlatParams(AD.cls_model())
    assert list(flat.offsets) == list(pl.goff) and flat.numel == pl.gnumel and len(pl.params) == len(list(m.parameters()))
    written = []
    for k in range(pl.n_bwd):
        r = pl.bwd_prog[k]
        if r.op not in (0, plan.OP_WAIT):
            written += [r.t[j].off for j in range(plan.NREF) if r.t[j].slot == plan.S_GRAD]
    assert sorted(written) == [4 * o for o in sorted(pl.goff)]
    assert sorted(i for _, _, ps in pl.grad_ready for i in ps) == list(range(len(pl.params)))
    assert pl.fwd_prog[pl._zero_index].n[0] == 4 * pl.gnumel


def test_classifier_only_leaves_one_launching_backward_record():
    from avid_hip import plan
    m, pl = _cls_plan(AD.SMALL, classifier_only=True)
    assert _ops(pl.bwd_prog, pl.n_bwd) == [plan.OP_CLS_LINEAR_BWD]
    r = [pl.bwd_prog[k] for k in range(pl.n_bwd) if pl.bwd_prog[k].op == plan.OP_CLS_LINEAR_BWD][0]
    assert r.t[3].slot == -1                                              # no input gradient
    assert pl.n_cls == 50 * 512 + 52 and pl.fwd_prog[pl._zero_index].n[0] == 4 * pl.n_cls
    # the forward is the full step's: the tower still runs in training mode
    _, full = _cls_plan(AD.SMALL)
    assert _ops(pl.fwd_prog, pl.n_fwd) == _ops(full.fwd_prog, full.n_fwd)


def test_no_dropout_no_dropout_record():
    from avid_hip import plan
    _, pl = _cls_plan(AD.SMALL, use_dropout=False)
    assert pl.drop_index is None
    assert plan.OP_DROPOUT_FWD not in _ops(pl.fwd_prog, pl.n_fwd) and plan.OP_DROPOUT_BWD not in _ops(pl.bwd_prog, pl.n_bwd)


# ------------------------------------------------------------------------------------------------------------------ probe
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_probe_plan_compiles_without_a_tower_backward(shape):
    from avid_hip import plan
    from avid_hip.parallel import FlatParams
    m, pl = _probe_plan(shape)
    B, n = shape[0], 4
    size = {plan.S_FWD: pl.fa_bytes, plan.S_BWD: pl.ba_bytes, plan.S_GRAD: 4 * pl.gnumel, plan.S_AUX: pl.aux_bytes,
            plan.S_VIDEO: 4 * B * shape[2] * shape[3], plan.S_DLOGITS: 4 * B * 50 * n, plan.S_OUT: plan.PROBE_OUT_BYTES * n,
            plan.S_LABELS: 8 * B}
    _in_bounds(pl, ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)), size)
    fwd = _ops(pl.fwd_prog, pl.n_logits)
    head = [plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_PROBE_LINEAR_FWD]
    assert fwd == [plan.OP_MEMSET0, plan.OP_WT_BATCH] + [plan.OP_CONV_FWD, plan.OP_BN_FWD] * 9 + [plan.OP_GPOOL_FWD] + head * 4
    assert _ops(pl.fwd_prog, pl.n_fwd)[len(fwd):] == [plan.OP_CLS_LOSS] * 4
    # every tap is a materialised tensor [B, 1, H, W, C] of the forward arena, pooled with T = To = 1 to the head's (h, w)
    pools = [pl.fwd_prog[k] for k in range(pl.n_logits) if pl.fwd_prog[k].op == plan.OP_ADAPTIVE_MAXPOOL]
    assert [(list(r.i)[:5], (r.d.To, r.d.Ho, r.d.Wo)) for r in pools] == [
        ([B, 1, h, w, c], (1,) + hw) for (h, w, c), hw in zip(TAPS[shape], AD.HEADS[shape][0])]
    bns = [pl.fwd_prog[k] for k in range(pl.n_logits) if pl.fwd_prog[k].op == plan.OP_BN_FWD]
    assert [r.t[0].off for r in pools] == [bns[k].t[5].off for k in (2, 4, 6, 8)]     # block1..block4's second BatchNorm output
    assert all(r.t[0].slot == plan.S_FWD for r in pools)
    assert [list(r.i)[:2] for k in range(pl.n_logits) for r in [pl.fwd_prog[k]] if r.op == plan.OP_BN1D_FWD] == \
        [[B, d] for d in AD.HEADS[shape][1]]
    # backward: head records only, over the classifiers' slice of the gradient buffer
    assert _ops(pl.bwd_prog, pl.n_bwd) == [plan.OP_PROBE_LINEAR_BWD, plan.OP_BN1D_BWD] * 4
    heads = list(m.classifiers.parameters())
    assert len(pl.params) == 16 and {id(p) for p in pl.params} == {id(p) for p in heads}
    flat = FlatParams(AD.probe_model(shape))
    assert list(flat.offsets) == list(pl.goff) and flat.numel == pl.gnumel
    written = []
    for k in range(pl.n_bwd):
        r = pl.bwd_prog[k]
        written += [r.t[j].off for j in range(plan.NREF) if r.t[j].slot == plan.S_GRAD and r.op != plan.OP_WAIT]
    assert sorted(written) == [4 * o for o in sorted(pl.goff)]


# -------------------------------------------------------------------------------------------------------------- inference
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eval_plans_compile(shape):
    from avid_hip import plan
    B = shape[0]
    tower = [plan.OP_CONV_FWD, plan.OP_BN_EVAL_APPLY] * 9 + [plan.OP_GPOOL_FWD]
    head = [plan.OP_BN_EVAL_COEFFS, plan.OP_WT_BATCH]
    for m, outputs, want in (
            (AD.tower_model(), [(B, 512, 1, 1)], head + tower),
            (AD.cls_model(), [(B, 50)], head + tower + [plan.OP_CLS_LINEAR_FWD]),
            # the probe's tower is frozen: its BatchNorms are the per-layer path's unfused call, with no coefficient table
            (AD.probe_model(shape), [(B, 50)] * 4,
             [plan.OP_WT_BATCH] + [plan.OP_CONV_FWD, plan.OP_BN_EVAL_DIRECT] * 9 + [plan.OP_GPOOL_FWD] +
             [plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_PROBE_LINEAR_FWD] * 4)):
        pl = plan.EvalPlan(m.eval(), shape, None, CPU)
        assert [s for _, s in pl.outputs] == outputs
        assert _ops(pl.fwd_prog, pl.n_fwd) == want, type(m).__name__
        size = {plan.S_FWD: pl.fa_bytes, plan.S_AUX: pl.aux_bytes, plan.S_VIDEO: 4 * B * shape[2] * shape[3], plan.S_OUT: pl.out_bytes}
        _in_bounds(pl, ((pl.fwd_prog, pl.n_fwd),), size)
        assert not any(pl.fwd_prog[k].t[j].slot in (plan.S_BWD, plan.S_GRAD, plan.S_AUDIO)
                       for k in range(pl.n_fwd) for j in range(plan.NREF))
        assert pl.fa_bytes <= pl.virtual_bytes
    assert getattr(plan.EvalPlan(AD.probe_model(shape).eval(), shape, None, CPU), "out_names") == AD.STAGES


def test_audio_and_video_plans_of_one_shape_family_do_not_collide():
    """The cache key carries the input shape: rank 4 for a spectrogram batch, rank 5 for clips."""
    from avid_hip import plan
    assert plan._audio_tower(AD.tower_model()) and plan._audio_tower(AD.cls_model()) and plan._audio_tower(AD.probe_model(AD.SMALL))
    import models
    assert not plan._audio_tower(models.R2Plus1D(18))
    assert not plan._audio_tower(models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]))
    x = torch.zeros(AD.SMALL)
    assert plan.run_cls(AD.cls_model().train(), x) is None                # a CPU tensor: the per-layer path
    assert plan.run_eval(AD.tower_model().eval(), x) is None


# --------------------------------------------------------------------------------------------------------------- refusals
def test_mixed_and_unknown_forms_stay_refused():
    import models
    from avid_hip import plan
    vshape = (4, 3, 8, 64, 64)
    pools3 = ["AdaptiveMaxPool3d((1,%d,%d))" % hw for hw in AD.HEADS[AD.SMALL][0]]
    args = AD.probe_args(AD.SMALL)
    # a 3-D pool on the audio tower (torch's module would refuse the 4-D tap), in one head or in all of them
    for pools in (pools3, pools3[:1] + args["pooling_ops"][1:]):
        with pytest.raises(plan.Unsupported):
            _probe_plan(AD.SMALL, pooling_ops=pools)
        with pytest.raises(plan.Unsupported):
            plan.EvalPlan(AD.probe_model(AD.SMALL, pooling_ops=pools).eval(), AD.SMALL, None, CPU)
    # a 2-D pool on the video tower
    video_args = dict(args, feat_dims=[1024, 1024, 1024, 1024])
    mv = models.MOSTModel(models.R2Plus1D(18), **video_args).train()
    with pytest.raises(plan.Unsupported):
        plan.ProbePlan(mv, vshape, CPU, True, True)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(mv.eval(), vshape, None, CPU)
    # ... while each tower compiles with its own kind
    plan.ProbePlan(models.MOSTModel(models.R2Plus1D(18), **dict(video_args, pooling_ops=pools3)).train(), vshape, CPU, True, True)
    # the other head forms, as for video
    for kw in (dict(l2_norm=True), dict(use_bn=False), dict(use_dropout=True),
               dict(pooling_ops=["AdaptiveAvgPool2d((4,4))"] + args["pooling_ops"][1:]),
               dict(pooling_ops=["AdaptiveMaxPool2d(4)"] + args["pooling_ops"][1:]),
               dict(feat_names=["conv1"] + AD.STAGES[1:])):
        with pytest.raises(plan.Unsupported):
            _probe_plan(AD.SMALL, **kw)
    # head widths that are not the pooled tap's
    with pytest.raises(plan.Unsupported):
        _probe_plan(AD.ODD, feat_dims=[1024, 1024, 1024, 1024])
    # a probe tower that is not frozen
    m = AD.probe_model(AD.SMALL).train()
    for p in m.feature_extractor.block4.parameters():
        p.requires_grad = True
    with pytest.raises(plan.Unsupported):
        plan.ProbePlan(m, AD.SMALL, CPU, True, True)
    # a fine-tuning model with frozen parameters, another feat_name, a pooling op, torch's dropout
    m = AD.cls_model().train()
    m.feature_extractor.conv1[0].weight.requires_grad = False
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(m, AD.SMALL, CPU, True, True)
    for kw in (dict(feat_name="conv5x", feat_dim=512, pooling_op="AdaptiveMaxPool2d((1,1))"), dict(feat_name="conv5x", feat_dim=512 * 20)):
        with pytest.raises(plan.Unsupported):
            _cls_plan(AD.SMALL, **kw)
    m = AD.cls_model().train()
    m.dropout = torch.nn.Dropout(0.5)
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(m, AD.SMALL, CPU, True, True)
    # the input's rank belongs to the tower: clips into the audio tower, spectrograms into the video one
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(AD.cls_model().train(), vshape, CPU, True, True)
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(models.ClassificationWrapper(models.R2Plus1D(18), 50, "pool", 512).train(), AD.SMALL, CPU, True, True)
    # a tower that is neither, a bare module the inference compiler does not know
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(models.ClassificationWrapper(torch.nn.Conv2d(1, 512, 3), 50, "pool", 512).train(), AD.SMALL, CPU, True, True)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(torch.nn.Linear(4, 4), (4, 4), None, CPU)


def test_a_hooked_or_eval_mode_module_yields_no_plan():
    from avid_hip import plan
    for m in (AD.cls_model().train(), AD.probe_model(AD.SMALL).train()):
        assert plan._tree_ok(m)
        h = m.feature_extractor.block2.bn1.register_forward_hook(lambda *a: None)
        assert not plan._tree_ok(m) and not plan._tree_ok(m, training=False)
        h.remove()
        assert plan._tree_ok(m)
        m.feature_extractor.eval()
        assert not plan._tree_ok(m) and plan._tree_ok(m, training=False)
        m.eval()
        assert not plan.eligible(m, torch.zeros(AD.SMALL))


def test_inputs_of_the_wrong_rank_or_count_are_not_eligible():
    """``_inputs_ok`` on the host: it sees CPU tensors as not eligible whatever their rank, so the rank rule is read off meta
    tensors that claim to be on the GPU."""
    from avid_hip import plan

    class T:
        def __init__(self, rank):
            self.rank, self.is_cuda, self.dtype = rank, True, torch.float32

        def dim(self):
            return self.rank

    real = torch.is_tensor
    mp = pytest.MonkeyPatch()
    mp.setattr(torch, "is_tensor", lambda x: isinstance(x, T) or real(x))
    mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    try:
        assert plan._inputs_ok((T(4),), True) and not plan._inputs_ok((T(5),), True) and not plan._inputs_ok((T(4), T(4)), True)
        assert plan._inputs_ok((T(5),)) and plan._inputs_ok((T(5), T(4))) and not plan._inputs_ok((T(4),))
        assert not plan._inputs_ok((T(5), T(4), T(4)))
    finally:
        mp.undo()


# --------------------------------------------------------------------------------------------------------------- fixtures
def test_state_dicts_match_the_reference_fixture():
    ref = json.load(open(os.path.join(GOLDEN, "audio_downstream_keys.json")))
    assert ref["cls"]["args"] == AD.CLS_ARGS and ref["probe"]["args"] == AD.probe_args(AD.SMALL)
    assert [[k, list(v.shape)] for k, v in AD.cls_model().state_dict().items()] == ref["cls"]["state_dict"]
    assert [[k, list(v.shape)] for k, v in AD.probe_model(AD.SMALL).state_dict().items()] == ref["probe"]["state_dict"]


def test_pooling_strings_are_parsed():
    from models.linear_probe import Classifier
    for s, want in (("AdaptiveMaxPool2d((4,4))", (1, 4, 4)), (" AdaptiveMaxPool2d( ( 12 , 3 ) ) ", (1, 12, 3)),
                    ("AdaptiveMaxPool3d((2,3,4))", (2, 3, 4)), ("AdaptiveMaxPool2d(4)", None), ("AdaptiveAvgPool2d((4,4))", None),
                    ("AdaptiveMaxPool2d((4,4,4))", None), ("AdaptiveMaxPool1d((4))", None)):
        c = Classifier(5, "conv2x", 8, s)
        assert c.pool_size == want, s
        assert type(c.pooling).__name__ == s.strip().split("(")[0]


def test_the_restatement_reproduces_the_reference_fixture():
    """The float64 yardstick of the GPU tests against what the reference computed in float32 on the CPU, at the float32 reference's
    own resolution (the generator prints its distance from float64: at most 1.2e-6 for fine-tuning, 7.9e-6 for the probe)."""
    z = np.load(os.path.join(GOLDEN, "audio_downstream.npz"))
    assert int(z["weight_seed"]) == AD.FIXTURE_SEED and (int(z["dropout_seed"]), int(z["dropout_offset"])) == AD.FIXTURE_DROPOUT
    assert tuple(z["x"].shape) == AD.SMALL
    keep = AD.host_mask(4, 512, 0.5, *AD.FIXTURE_DROPOUT)
    assert np.array_equal(keep, z["keep"]) and 0.4 < keep.mean() < 0.6
    x, labels = torch.from_numpy(z["x"]).double(), torch.from_numpy(z["labels"])
    ref = AD.restate(AD.cls_model().train())
    ref.keep = torch.from_numpy(keep)
    logits = ref(x)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    assert abs(float(loss.detach()) - float(z["cls.loss"])) <= 1e-5 * abs(float(z["cls.loss"]))
    assert AD.max_rel(torch.from_numpy(z["cls.logits"]), logits) < 2e-5
    grads = dict(ref.named_parameters())
    for k in ("classifier.weight", "classifier.bias", "feature_extractor.conv1.0.weight"):
        assert AD.max_rel(torch.from_numpy(z[f"cls.grad.{k}"]), grads[k].grad) < 2e-5, k
    heads = AD.restate(AD.probe_model(AD.SMALL).train(), AD.SMALL)(x)
    for k in AD.STAGES:
        assert AD.max_rel(torch.from_numpy(z[f"probe.logits.{k}"]), heads[k]) < 2e-5, k
