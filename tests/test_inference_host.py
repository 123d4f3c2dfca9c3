"""Host logic of the inference compiler (avid_hip/plan.py: EvalBuilder / EvalPlan), no GPU: the programs compile at the shipped
evaluation shapes, hold only known record kinds, keep every reference inside its buffer, never hand a recycled buffer to a
writer while a reader of its earlier contents is still to come, and take less memory than the training forward."""
import pytest
import torch

CPU = torch.device("cpu")
SHAPES = {"8x8x224": (8, 3, 8, 224, 224), "4x32x224": (4, 3, 32, 224, 224)}


def _cls():
    import models
    return models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5)


@pytest.fixture(scope="module")
def compiled():
    import models
    from avid_hip import plan
    out = {k: plan.EvalPlan(_cls(), s, None, CPU) for k, s in SHAPES.items()}
    av = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])
    out["av"] = plan.EvalPlan(av, (4, 3, 8, 112, 112), (4, 1, 40, 100), CPU)
    return out


def _records(pl):
    return [pl.fwd_prog[k] for k in range(pl.n_fwd)]


def test_programs_compile_with_known_records_and_references_in_bounds(compiled):
    from avid_hip import plan
    size = lambda pl: {plan.S_FWD: pl.fa_bytes, plan.S_AUX: pl.aux_bytes, plan.S_OUT: pl.out_bytes}   # noqa: E731
    for name, pl in compiled.items():
        recs = _records(pl)
        assert recs[0].op == plan.OP_BN_EVAL_COEFFS and recs[0].t[0].off == pl.bn_table_off, name
        assert recs[0].i[0] == len(pl.bn_recs) == (33 + 9 if name == "av" else 33)
        assert recs[1].op in (plan.OP_WT_BATCH, 0)
        for k, r in enumerate(recs):
            assert r.op in plan._OP_NAMES and 0 <= r.stream < 4
            # forward records only: nothing of a backward, no training-mode BatchNorm, no argmax of the stem's pool
            assert r.op in (0, plan.OP_WAIT, plan.OP_CONV_FWD, plan.OP_GPOOL_FWD, plan.OP_WT_BATCH, plan.OP_CLS_LINEAR_FWD,
                            plan.OP_BN_EVAL_COEFFS, plan.OP_BN_EVAL_APPLY, plan.OP_BN_POOL_FWD_EVAL), (name, k, r.op)
            for j in range(plan.NREF):
                s, off = r.t[j].slot, r.t[j].off
                if s in size(pl):
                    assert 0 <= off < size(pl)[s], (name, k, j, s, off)
                elif s >= 0:
                    assert off == 0 and s < pl.n_slots
            if r.op == plan.OP_CONV_FWD:
                assert r.t[6].slot < 0, "BatchNorm partial sums in an inference program"
        # launches per program: every record but the waits
        n = sum(1 for r in recs if r.op not in (0, plan.OP_WAIT))
        assert n == {"8x8x224": 65, "4x32x224": 73, "av": 97}[name], (name, n)
    # 8 frames at 224 x 224: conv2x's four temporal layers carry both maps, and no BatchNorm record stands before conv3x
    recs = _records(compiled["8x8x224"])
    conv3x = next(k for k, r in enumerate(recs) if r.op == plan.OP_CONV_FWD and r.d.Cout == 128)
    assert [r.op for r in recs[2:conv3x]] == [plan.OP_CONV_FWD, plan.OP_BN_POOL_FWD_EVAL] + [plan.OP_CONV_FWD] * 8
    assert sum(1 for r in recs if r.op == plan.OP_CONV_FWD and r.i[3] == 2 and r.i[1] == 2) == 4
    # 32 frames: no layer takes the tconv forms
    assert all(r.i[3] == 0 and r.i[1] == 0 for r in _records(compiled["4x32x224"]) if r.op == plan.OP_CONV_FWD)


def test_no_buffer_is_rewritten_while_its_contents_are_still_read(compiled):
    """Walk the program: every reference into the arena falls into exactly one buffer that is live at that record, and two
    buffers that share bytes are live at disjoint times on the same stream, the later one starting strictly after the earlier
    one's last record (a record's output never aliases one of its inputs)."""
    from avid_hip import plan
    for name, pl in compiled.items():
        recs = _records(pl)
        bufs = pl.buffers                                   # (offset, bytes, stream, first record, last record)
        for k, r in enumerate(recs):
            if r.op in (0, plan.OP_WAIT):
                continue
            for j in range(plan.NREF):
                if r.t[j].slot == plan.S_FWD:
                    live = [b for b in bufs if b[0] <= r.t[j].off < b[0] + b[1] and b[3] <= k <= b[4]]
                    assert len(live) == 1 and live[0][2] == r.stream, (name, k, j, live)
        shared = 0
        for a in range(len(bufs)):
            for b in range(a + 1, len(bufs)):
                x, y = bufs[a], bufs[b]
                if x[0] < y[0] + y[1] and y[0] < x[0] + x[1]:
                    shared += 1
                    first, second = (x, y) if x[3] <= y[3] else (y, x)
                    assert first[2] == second[2] and first[4] < second[3], (name, first, second)
        assert shared > 0, "nothing was recycled"
        assert max(o + n for o, n, *_ in bufs) == pl.fa_bytes < pl.virtual_bytes


def test_audio_tower_keeps_its_own_stream_and_buffers(compiled):
    from avid_hip import plan
    pl = compiled["av"]
    by_stream = {}
    for o, n, s, *_ in pl.buffers:
        by_stream.setdefault(s, []).append((o, o + n))
    assert set(by_stream) == {plan.ST_MAIN, plan.ST_AUDIO}
    for a0, a1 in by_stream[plan.ST_AUDIO]:
        assert all(a1 <= v0 or v1 <= a0 for v0, v1 in by_stream[plan.ST_MAIN])
    assert len(pl.outputs) == 2 and all(off + 4 * 4 * 128 <= pl.out_bytes for off, _ in pl.outputs)


def test_eval_arena_is_smaller_than_the_training_forward_arena(compiled):
    """Same geometry, the fine-tuning step's forward arena (bump allocator, everything kept for the backward) against the
    inference program's recycled one.  DESIGN.md 6c / 6d quote these byte counts."""
    from avid_hip import plan
    want = {"8x8x224": (1251385600, 477708288), "4x32x224": (2867507968, 955367424)}
    for name, shape in SHAPES.items():
        train = plan.ClsPlan(_cls().train(), shape, CPU, True, True)
        ev = compiled[name]
        assert ev.fa_bytes < train.fa_bytes
        assert (train.fa_bytes, ev.fa_bytes) == want[name], (name, train.fa_bytes, ev.fa_bytes)


def test_training_programs_hold_no_inference_record():
    from avid_hip import plan
    pl = plan.ClsPlan(_cls().train(), (2, 3, 8, 64, 64), CPU, True, True)
    for prog, n in ((pl.fwd_prog, pl.n_fwd), (pl.bwd_prog, pl.n_bwd)):
        assert all(prog[k].op < plan.OP_BN_EVAL_COEFFS and not (prog[k].op == plan.OP_CONV_FWD and prog[k].i[3]) for k in range(n))


def test_what_the_compiler_refuses():
    import models
    from avid_hip import plan
    shape = (2, 3, 8, 64, 64)
    m = _cls()
    m.feature_extractor.conv2x[0] = torch.nn.Identity()
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(m, shape, None, CPU)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, pooling_op="AdaptiveMaxPool3d(1)"), shape, None, CPU)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(torch.nn.Linear(4, 4), shape, None, CPU)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(_cls().double(), shape, None, CPU)
    most = models.MOSTModel(models.R2Plus1D(18), 400, ["conv5x"], [8192], ["AdaptiveAvgPool3d((1,4,4))"], use_bn=True)
    with pytest.raises(plan.Unsupported):
        plan.EvalPlan(most, shape, None, CPU)
    # CPU inputs, a hooked module: no plan — parallel.Inference takes the per-layer path
    assert plan.eval_plan(_cls(), torch.zeros(shape)) is None


PROBE = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
             pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                          "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)


def test_probe_program_at_the_shipped_batch():
    """The stock MOSTModel at the shipped probe batch (128 clips of 3x8x224x224): frozen BatchNorms are the per-layer path's own
    call as a record (no coefficient launch, nothing fused), the heads are records, and the arena is smaller than the probe's
    training forward arena (DESIGN.md 6c / 6d quote the figures)."""
    import models
    from avid_hip import plan
    m = models.MOSTModel(models.R2Plus1D(18), **PROBE)
    shape = (128, 3, 8, 224, 224)
    ev = plan.EvalPlan(m, shape, None, CPU)
    recs = _records(ev)
    kinds = [r.op for r in recs]
    assert all(k in plan._OP_NAMES for k in kinds)
    assert sum(1 for k in kinds if k not in (0, plan.OP_WAIT)) == 84
    assert kinds.count(plan.OP_BN_EVAL_DIRECT) == 33 and kinds.count(plan.OP_MAXPOOL_FWD) == 1 and not ev.bn_recs
    assert not {plan.OP_BN_EVAL_COEFFS, plan.OP_BN_EVAL_APPLY, plan.OP_BN_POOL_FWD_EVAL} & set(kinds)
    assert all(r.i[1] == 0 and r.i[3] == 0 for r in recs if r.op == plan.OP_CONV_FWD)
    assert kinds[-12:] == [plan.OP_ADAPTIVE_MAXPOOL, plan.OP_BN1D_FWD, plan.OP_PROBE_LINEAR_FWD] * 4
    assert all(r.i[2] == 0 for r in recs if r.op == plan.OP_BN1D_FWD)          # training = 0
    assert len(ev.outputs) == 4 and ev.out_names == PROBE["feat_names"]
    train = plan.ProbePlan(m.train(), shape, CPU, True, True)
    assert (train.fa_bytes, ev.fa_bytes) == (19394503680, 10949632000)
    # the liveness walk of test_no_buffer_is_rewritten_while_its_contents_are_still_read, on this program: the taps are read by
    # the heads at the end, so their bytes are not handed out in between
    for k, r in enumerate(recs):
        if r.op in (0, plan.OP_WAIT):
            continue
        for j in range(plan.NREF):
            if r.t[j].slot == plan.S_FWD:
                live = [b for b in ev.buffers if b[0] <= r.t[j].off < b[0] + b[1] and b[3] <= k <= b[4]]
                assert len(live) == 1, (k, j, live)
    for a in range(len(ev.buffers)):
        for b in range(a + 1, len(ev.buffers)):
            x, y = ev.buffers[a], ev.buffers[b]
            if x[0] < y[0] + y[1] and y[0] < x[0] + x[1]:
                first, second = (x, y) if x[3] <= y[3] else (y, x)
                assert first[4] < second[3], (first, second)


def test_recycling_places_outputs_before_it_releases_inputs():
    """The allocator on a hand-made chain a -> b -> c -> d of equal sizes on one stream: two physical buffers serve it, and no
    record's output takes the bytes of its own input."""
    from avid_hip import plan
    arena = plan.EvalArena(plan.S_FWD)
    refs = [arena.alloc(1000) for _ in range(4)]
    recs = []
    for k in range(3):
        r = plan.Instr()
        r.op = plan.OP_BN_EVAL_APPLY
        for j in range(plan.NREF):
            r.t[j].slot = -1
        r.t[0].slot, r.t[0].off = refs[k]
        r.t[2].slot, r.t[2].off = refs[k + 1]
        recs.append(r)
    top, bufs = plan.EvalPlan._recycle(recs, arena.bufs, plan.S_FWD)
    assert top == 2 * 1024 and len(bufs) == 4
    assert all(r.t[0].off != r.t[2].off for r in recs)
    assert recs[0].t[2].off == recs[1].t[0].off and recs[1].t[2].off == recs[2].t[0].off
