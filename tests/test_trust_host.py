"""Per-tensor hyper-parameters and LARS / LAMB without a GPU: the segment table and its refusals (Python and C side), the rule
matching of the engines, the numpy restatements (tests/_trust_ref.py) against torch.optim with real ``param_groups`` and against
independent per-tensor loops, the LAMB error bound with its planted faults, and the checkpoint key."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _trust_ref as R

NUMELS = [1, 3, 4, 5, 64, 1027, 4096, 4097]            # tail only, no tail, body + tail, one chunk exactly, one chunk + 1


def _rand(n, seed, scale=1.0):
    return (scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))).numpy()


def _tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Linear(8, 3))


class _Wrapped(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.feature_extractor = torch.nn.Sequential(torch.nn.Linear(6, 6), torch.nn.BatchNorm1d(6))
        self.classifier = torch.nn.Linear(6, 3)


# ------------------------------------------------------------------------------------------------------------------- the table
def test_version_and_mirrors():
    from avid_hip import lib
    assert lib.version() >= 170
    for s in ("avid_segment_chunks", "avid_segment_sumsq_workspace_bytes", "avid_segment_sumsq", "avid_sgd_flat_table",
              "avid_adam_flat_table", "avid_lamb_flat"):
        assert s in lib.SIGNATURES
    assert C.sizeof(lib.Segment) == 32 and C.sizeof(lib.SegChunk) == 16 and C.sizeof(lib.SegmentTable) == 40
    assert lib.Segment.first_chunk.offset == 28 and lib.SegChunk.seg.offset == 12


def test_table_from_flat_params():
    """Built from a FlatParams: one segment per tensor in the flat layout's order, offsets on multiples of 4, the padding in no
    segment, chunks of 4096 floats dealt per segment; a slice of the layout counts its offsets from the slice's start."""
    from avid_hip import lib, ops
    from avid_hip.parallel import FlatParams
    m = torch.nn.Sequential(torch.nn.Linear(100, 90), torch.nn.Linear(90, 3))      # 9000, 90, 270, 3 elements
    flat = FlatParams(m)
    n = len(flat.params)
    tab = ops.SegmentTable(flat, lr_scale=[0.5, 1.0, 2.0, 1.0], weight_decay=1e-4, adapt=[True, False, True, False])
    assert tab.S == n == 4 and tab.numel == flat.numel and tab.offsets == flat.offsets
    assert tab.numels == [p.numel() for p in flat.params] == [3, 270, 90, 9000]
    assert tab.lr_scale == [0.5, 1.0, 2.0, 1.0] and tab.adapt == [True, False, True, False]
    assert all(abs(w - 1e-4) < 1e-11 for w in tab.weight_decay)
    assert tab.n_chunks == 1 + 1 + 1 + 3 and [s.first_chunk for s in tab.segs] == [0, 1, 2, 3]
    last = [(c.start, c.len, c.seg) for c in tab.chunks][3:]
    o = flat.offsets[3]
    assert last == [(o, 4096, 3), (o + 4096, 4096, 3), (o + 8192, 9000 - 8192, 3)]
    assert tab.workspace_bytes() == 6 * 2 * 8 and tab.trust.tolist() == [1.0] * 4
    covered = sum(tab.numels)
    assert covered < tab.numel and tab.numel % 4 == 0                  # 3 -> 4 and 270 -> 272 and 90 -> 92: padding in no segment
    head = ops.SegmentTable(flat, begin=0, end=flat.offsets[2])
    assert head.S == 2 and head.numel == flat.offsets[2] and head.index == [0, 1]
    rest = ops.SegmentTable(flat, begin=flat.offsets[2])
    assert rest.offsets == [0, flat.offsets[3] - flat.offsets[2]] and rest.index == [2, 3]
    assert lib.SEG_CHUNK == 4096


def test_table_refusals_in_python():
    from avid_hip import ops, AvidHipError
    dev = torch.device("cpu")
    good = [(0, 5), (8, 3)]
    ops.SegmentTable(good, device=dev)
    for layout, kw, word in (([], {}, "no tensor"), ([(2, 4)], {}, "aligned"), ([(-4, 4)], {}, "negative"), ([(8, 3), (0, 5)], {}, "increasing"),
                             ([(0, 6), (4, 3)], {}, "overlapping"), ([(0, 0)], {}, "empty"), ([(0, 9)], {"numel": 8}, "straddles"),
                             (good, {"lr_scale": float("nan")}, "finite"), (good, {"weight_decay": float("inf")}, "finite"),
                             (good, {"lr_scale": [1.0]}, "values"), (good, {"begin": 4}, "straddles")):
        with pytest.raises(AvidHipError, match=word):
            ops.SegmentTable(layout, device=dev, **kw)
    with pytest.raises(AvidHipError, match="device"):
        ops.SegmentTable(good)
    tab = ops.SegmentTable(good, device=dev)
    p = torch.zeros(tab.numel)
    for call in (lambda: ops.segment_sumsq(tab, p), lambda: ops.sgd_flat_table(tab, p, p, None, 0.1, 0.0),
                 lambda: ops.adam_flat_table(tab, p, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 1),
                 lambda: ops.lamb_flat(tab, p, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 1)):
        with pytest.raises(AvidHipError, match="device tensors"):                 # no CPU fallback
            call()


def _c_table(pairs, scales=None, decays=None, adapts=None):
    from avid_hip import lib
    S = len(pairs)
    segs = (lib.Segment * S)(*[lib.Segment(o, n, (scales or [1.0] * S)[k], (decays or [0.0] * S)[k], (adapts or [1] * S)[k], 0)
                               for k, (o, n) in enumerate(pairs)])
    count = lib.raw("avid_segment_chunks")(S, segs, None, 0)
    chunks = (lib.SegChunk * max(count, 1))()
    if count > 0:
        assert lib.raw("avid_segment_chunks")(S, segs, chunks, count) == count
    keep = (C.c_double * 8)()                       # stands in for the device copies: nothing is launched
    tab = lib.SegmentTable(S, count, C.addressof(segs), C.addressof(keep), C.addressof(chunks), C.addressof(keep))
    return tab, segs, chunks, keep


def test_table_refusals_in_the_library():
    """Every entry point validates the host copy of the table before it launches anything (there is no GPU here: a launch would
    fail with another code): AVID_E_BADARG, the message names the entry point and the segment."""
    from avid_hip import lib
    BADARG = -1
    buf = (C.c_float * 20000)()
    base = (C.addressof(buf) + 15) & ~15
    P = lambda off=0: C.c_void_p(base + 4 * off)     # noqa: E731
    ws = (C.c_double * 64)()

    def calls(tab, n):
        t = C.byref(tab)
        return {"segment_sumsq": lib.raw("avid_segment_sumsq")(t, n, P(), None, ws, None, ws, 512, None),
                "sgd_flat_table": lib.raw("avid_sgd_flat_table")(t, n, P(), P(5000), None, 0.1, 0.0, 0, None, 1.0, 0.0, None, None,
                                                                 None, None, 0, None),
                "adam_flat_table": lib.raw("avid_adam_flat_table")(t, n, P(), P(5000), P(10000), P(15000), 1e-3, 0.9, 0.999, 1e-8,
                                                                   1, None, None, 1.0, None, None, None),
                "lamb_flat": lib.raw("avid_lamb_flat")(t, n, P(), P(5000), P(10000), P(15000), 1e-3, 0.9, 0.999, 1e-8, 1, None,
                                                        None, 1.0, ws, None, None, ws, 512, None)}

    def all_refuse(tab, n, word):
        for name in ("segment_sumsq", "sgd_flat_table", "adam_flat_table", "lamb_flat"):
            rc = calls(tab, n)[name]
            # (each call sets the message: ask again for this one alone)
            one = {"segment_sumsq": lambda: lib.raw("avid_segment_sumsq")(C.byref(tab), n, P(), None, ws, None, ws, 512, None)}
            assert rc == BADARG, (name, word, rc)
        rc = one["segment_sumsq"]()
        assert rc == BADARG and "segment_sumsq" in lib.last_error() and word in lib.last_error(), (word, lib.last_error())

    nan, inf = float("nan"), float("inf")
    cases = [([(2, 4)], {}, 16, "aligned"), ([(-4, 4)], {}, 16, "negative"), ([(8, 4), (0, 4)], {}, 16, "increasing"),
             ([(0, 6), (4, 4)], {}, 16, "overlapping"), ([(0, 4), (8, 9)], {}, 16, "exceeds n"),
             ([(0, 4)], {"scales": [nan]}, 16, "finite"), ([(0, 4)], {"scales": [inf]}, 16, "finite"),
             ([(0, 4)], {"decays": [-inf]}, 16, "finite"), ([(0, 4)], {"adapts": [2]}, 16, "adapt")]
    for pairs, kw, n, word in cases:
        tab, *keep = _c_table(pairs, **kw)
        all_refuse(tab, n, word)
    tab, segs, chunks, keep = _c_table([(0, 5000), (5000, 8)])
    assert tab.n_chunks == 3
    chunks[1].len += 1
    all_refuse(tab, 5008, "chunk 1")
    chunks[1].len -= 1
    segs[1].first_chunk = 1
    all_refuse(tab, 5008, "first_chunk")
    segs[1].first_chunk = 2
    tab.n_chunks = 4
    all_refuse(tab, 5008, "chunk list")
    tab.n_chunks = 3
    tab.seg_dev = None
    all_refuse(tab, 5008, "null")
    for s, c in ((0, None), (1, None)):
        assert lib.raw("avid_segment_chunks")(s, None, c, 0) == BADARG
    # the other arguments, on a good table
    tab, segs, chunks, keep = _c_table([(0, 8)])
    t = C.byref(tab)
    sgd, lamb = lib.raw("avid_sgd_flat_table"), lib.raw("avid_lamb_flat")
    assert sgd(t, 8, P(), P(5000), None, 0.1, 0.9, 0, None, 1.0, 0.0, None, None, None, None, 0, None) == BADARG
    assert "momentum" in lib.last_error()
    assert sgd(t, 8, P(), P(5000), None, 0.1, 0.0, 1, None, 1.0, 0.0, None, None, None, None, 0, None) == BADARG
    assert sgd(t, 8, P(1), P(5000), None, 0.1, 0.0, 0, None, 1.0, 0.0, None, None, None, None, 0, None) == BADARG
    assert sgd(t, 8, P(), P(5000), None, 0.1, 0.0, 0, None, 1.0, 0.001, ws, None, None, None, 0, None) == BADARG      # trust without workspace
    assert "workspace" in lib.last_error()
    assert sgd(t, 8, P(), P(5000), None, 0.1, 0.0, 0, None, 1.0, 0.0, ws, None, None, ws, 512, None) == BADARG        # trust with eta 0
    assert "trust coefficient" in lib.last_error()
    assert lamb(t, 8, P(), P(5000), P(10000), P(15000), 1e-3, 0.9, 0.999, 1e-8, 1, None, None, 1.0, None, None, None, ws, 512,
                None) == BADARG                                                                                           # no trust array
    assert lamb(t, 8, P(), P(5000), P(10000), P(15000), 1e-3, 0.9, 0.999, 1e-8, 1, None, None, 1.0, ws, None, None, ws, 8,
                None) == BADARG and "workspace" in lib.last_error()
    assert lib.raw("avid_segment_sumsq_workspace_bytes")(t) == 16 and lib.raw("avid_segment_sumsq_workspace_bytes")(None) == 0


# ----------------------------------------------------------------------------------------------------------------- the rules
def test_rule_matching_and_rules_no_decay_1d():
    from avid_hip import parallel
    m = _Wrapped()
    rules = [(r"^feature_extractor\.", {"lr_scale": 0.125})] + parallel.rules_no_decay_1d(m)
    eng = parallel.FinetuneStep(m, weight_decay=1e-4, optimizer="sgd", momentum=0.9, param_rules=rules)
    got = {n: (s, w, a) for n, s, w, a in eng.param_values()}
    assert got == {"feature_extractor.0.weight": (0.125, 1e-4, True), "feature_extractor.0.bias": (0.125, 1e-4, True),
                   "feature_extractor.1.weight": (0.125, 1e-4, True), "feature_extractor.1.bias": (0.125, 1e-4, True),
                   "classifier.weight": (1.0, 1e-4, True), "classifier.bias": (1.0, 0.0, False)}          # the first match wins
    assert [n for n, *_ in eng.param_values()] == ["classifier.bias", "classifier.weight", "feature_extractor.1.bias",
                                                   "feature_extractor.1.weight", "feature_extractor.0.bias",
                                                   "feature_extractor.0.weight"]                          # the flat layout's order
    nd = parallel.rules_no_decay_1d(m)
    assert [p for p, _ in nd] == [r"^feature_extractor\.0\.bias$", r"^feature_extractor\.1\.weight$", r"^feature_extractor\.1\.bias$",
                                  r"^classifier\.bias$"]
    assert all(d == {"weight_decay": 0.0, "adapt": False} for _, d in nd)
    eng = parallel.FinetuneStep(_Wrapped(), weight_decay=1e-4, optimizer="lars", momentum=0.9, param_rules=nd)
    got = {n: (s, w, a) for n, s, w, a in eng.param_values()}
    assert got["feature_extractor.1.weight"] == (1.0, 0.0, False) and got["feature_extractor.0.weight"] == (1.0, 1e-4, True)
    tab = eng.segment_table()
    assert tab.S == 6 and tab.adapt == [False, True, False, False, False, True] and eng.trust is tab.trust
    # the table covers the slice the engine updates: a classifier_only engine's holds the classifier
    warm = parallel.FinetuneStep(_Wrapped(), classifier_only=True, optimizer="lamb", param_rules=nd)
    assert warm.segment_table().S == 2 and warm.segment_table().numel == warm.n_cls
    # engines without rules and without trust ratios keep no table and say so
    plain = parallel.FinetuneStep(_Wrapped())
    assert not plain._table_on and plain.trust is None and sorted(plain.state_dict()) == ["param_groups", "state"]
    assert parallel.FinetuneStep(_Wrapped(), param_rules=[])._table_on          # an empty list of rules is still "with rules"


def test_rule_refusals_leave_the_model_alone():
    from avid_hip import parallel
    for rules, word in (([(r"^classifier", {"lr": 0.1})], "unknown key"), ([(r"^nothing_like_this", {"lr_scale": 0.1})], "matches no"),
                        ([(r"^classifier", {"lr_scale": -1.0})], "finite number >= 0"),
                        ([(r"^classifier", {"weight_decay": float("nan")})], "finite number >= 0"), ([r"^classifier"], "pair"),
                        ([(r"^classifier", 0.1)], "pair")):
        m = _Wrapped()
        before = [p.data_ptr() for p in m.parameters()]
        for make in (lambda: parallel.FinetuneStep(m, param_rules=rules), lambda: parallel.TrainStep(m, None, param_rules=rules),
                     lambda: parallel.ProbeStep(m, param_rules=rules)):
            with pytest.raises(ValueError, match=word):
                make()
        assert [p.data_ptr() for p in m.parameters()] == before        # nothing was flattened
    for kw, word in ((dict(optimizer="lion"), "optimizer must be"), (dict(optimizer="lars", nesterov=True), "Nesterov"),
                     (dict(optimizer="lars", trust_coefficient=0.0), "trust_coefficient"),
                     (dict(optimizer="lars", trust_coefficient=float("nan")), "trust_coefficient")):
        with pytest.raises(ValueError, match=word):
            parallel.FinetuneStep(_Wrapped(), **kw)
    # a rule that matches only a frozen parameter matches nothing the optimizer holds
    m = _Wrapped()
    for p in m.feature_extractor.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="matches no"):
        parallel.FinetuneStep(m, param_rules=[(r"^feature_extractor", {"lr_scale": 0.5})])


def test_dropin_optimizers_still_refuse_param_groups():
    from avid_hip import parallel
    m = _tiny_model()
    groups = [{"params": list(m[0].parameters())}, {"params": list(m[3].parameters()), "lr": 1e-2}]
    for cls in (parallel.Adam, parallel.SGD):
        with pytest.raises((ValueError, NotImplementedError)):
            cls(groups, lr=1e-3)


# -------------------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("optimizer", ["lars", "lamb", "sgd", "adam"])
def test_checkpoint_key_round_trip_and_mismatch(optimizer):
    from avid_hip import parallel
    kw = dict(optimizer=optimizer, weight_decay=1e-4, **({"momentum": 0.9} if optimizer in ("lars", "sgd") else {}))
    rules = lambda m, s=0.125: [(r"^feature_extractor\.0\.weight", {"lr_scale": s})] + parallel.rules_no_decay_1d(m)   # noqa: E731
    m = _Wrapped()
    eng = parallel.FinetuneStep(m, param_rules=rules(m), **kw)
    sd = eng.state_dict()
    assert sorted(sd) == ["avid_param_table", "param_groups", "state"]
    want = "momentum" if optimizer in ("lars", "sgd") else "betas"
    assert want in sd["param_groups"][0]                                  # torch.optim.SGD's / Adam's format, as today
    table = sd["avid_param_table"]
    names = [n for n, _ in m.named_parameters()]
    assert [t["name"] for t in table] == names and all(sorted(t) == ["adapt", "lr_scale", "name", "weight_decay"] for t in table)
    assert table[0] == {"name": "feature_extractor.0.weight", "lr_scale": 0.125, "weight_decay": 1e-4, "adapt": True}
    assert table[1] == {"name": "feature_extractor.0.bias", "lr_scale": 1.0, "weight_decay": 0.0, "adapt": False}
    m2 = _Wrapped()
    parallel.FinetuneStep(m2, param_rules=rules(m2), **kw).load_state_dict(sd)                      # the same rules: loads
    m3 = _Wrapped()
    with pytest.raises(ValueError, match=r"avid_param_table.*'feature_extractor\.0\.weight'"):
        parallel.FinetuneStep(m3, param_rules=rules(m3, 0.5), **kw).load_state_dict(sd)
    m4 = _Wrapped()
    with pytest.raises(ValueError, match=r"avid_param_table.*'feature_extractor\.0\.bias'"):       # the first tensor that differs
        parallel.FinetuneStep(m4, param_rules=[(r"^feature_extractor\.0\.weight", {"lr_scale": 0.125})], **kw).load_state_dict(sd)
    # torch's own checkpoint (no key) loads into a table-driven engine
    plain = {k: v for k, v in sd.items() if k != "avid_param_table"}
    m5 = _Wrapped()
    parallel.FinetuneStep(m5, param_rules=rules(m5), **kw).load_state_dict(plain)
    if optimizer in ("lars", "lamb"):                                      # without rules the key is there too: uniform values
        t = parallel.FinetuneStep(_Wrapped(), **kw).state_dict()["avid_param_table"]
        assert all((e["lr_scale"], e["weight_decay"], e["adapt"]) == (1.0, 1e-4, True) for e in t)


# ------------------------------------------------------------------------------------- the restatements against torch.optim
def _groups(segs, p):
    """One torch parameter per segment (float32) and the param_groups that give each its own lr scale and decay."""
    params = [torch.nn.Parameter(torch.from_numpy(p[s.offset:s.offset + s.numel].copy())) for s in segs]
    return params


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.5, False), (0.5, True)])
def test_grouped_sgd_is_torch_sgd_with_param_groups_bit_for_bit(momentum, nesterov):
    """torch.optim.SGD with one real param_group per tensor, three steps, every element the same bits.  torch's CPU kernels fuse
    their multiply-adds (tests/test_sgd_host.py) and the restatement rounds every product on its own, so the hyper-parameters are
    powers of two — lr 2^-3, momentum 2^-1, decays 2^-10 / 2^-13, lr_scale 2^-3 .. 2 — which makes every product exact and a
    fused multiply-add the same one rounding as the separate sum: what is compared is the order and the grouping of the
    operations, per group.  (Products that DO round are held against separate torch operations in the LARS loop below, whose
    excluded tensor is plain grouped SGD.)  lr * lr_scale is exact in float32 and in the Python floats torch multiplies by."""
    lr = 2.0 ** -3
    scales, decays = [1.0, 0.5, 0.125, 2.0, 1.0, 0.25, 1.0, 0.5], [0.0, 2.0 ** -10, 2.0 ** -13, 0.0, 2.0 ** -10, 2.0 ** -13, 0.0, 2.0 ** -10]
    segs, n = R.padded_table(NUMELS, scales, decays)
    p = np.zeros(n, np.float32)
    for k, s in enumerate(segs):
        p[s.offset:s.offset + s.numel] = _rand(s.numel, 100 + k)
    params = _groups(segs, p)
    opt = torch.optim.SGD([{"params": [q], "lr": lr * s.lr_scale, "weight_decay": s.weight_decay} for q, s in zip(params, segs)],
                          lr=lr, momentum=momentum, nesterov=nesterov)
    buf = np.zeros(n, np.float32) if momentum else None
    pad = R.padding_mask(segs, n)
    for step in range(3):
        g = np.zeros(n, np.float32)
        for k, s in enumerate(segs):
            g[s.offset:s.offset + s.numel] = _rand(s.numel, 1000 * step + k, 0.3)
        for q, s in zip(params, segs):
            q.grad = torch.from_numpy(g[s.offset:s.offset + s.numel].copy())
        opt.step()
        p, buf = R.grouped_sgd_step(p, g, buf, segs, lr, momentum, nesterov)
        for q, s in zip(params, segs):
            assert np.array_equal(q.detach().numpy().view(np.int32), p[s.offset:s.offset + s.numel].view(np.int32)), (step, s)
        assert not p[pad].any() and (buf is None or not buf[pad].any())


def test_grouped_adam_is_torch_adam_with_param_groups_within_the_adam_bar():
    """The bar of tests/test_gpu_finetune.py::_off_bar (rtol 1e-4 / atol 1e-6, every element), three steps."""
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    scales, decays = [1.0, 0.5, 0.1, 2.0, 1.0, 0.3, 1.0, 0.5], [0.0, 1e-4, 1e-4, 0.0, 5e-4, 1e-4, 0.0, 1e-4]
    segs, n = R.padded_table(NUMELS, scales, decays)
    p = np.zeros(n, np.float32)
    for k, s in enumerate(segs):
        p[s.offset:s.offset + s.numel] = _rand(s.numel, 200 + k)
    params = _groups(segs, p)
    opt = torch.optim.Adam([{"params": [q], "lr": R.f32(lr) * R.f32(s.lr_scale), "weight_decay": s.weight_decay}
                            for q, s in zip(params, segs)], lr=lr, betas=betas, eps=eps)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in range(3):
        g = np.zeros(n, np.float32)
        for k, s in enumerate(segs):
            g[s.offset:s.offset + s.numel] = _rand(s.numel, 2000 * (step + 1) + k, 0.3)
        for q, s in zip(params, segs):
            q.grad = torch.from_numpy(g[s.offset:s.offset + s.numel].copy())
        opt.step()
        p, m, v = R.grouped_adam_step(p, g, m, v, segs, lr, betas[0], betas[1], eps, step + 1)
        for q, s in zip(params, segs):
            np.testing.assert_allclose(p[s.offset:s.offset + s.numel], q.detach().numpy(), rtol=1e-4, atol=1e-6)


# --------------------------------------------------------------------------------- LARS / LAMB against independent loops
def _case(seed, wd=1e-4):
    """A table with an excluded (adapt False, no decay) tensor, an all-zero parameter tensor and an all-zero gradient tensor."""
    adapt = [True, True, False, True, True, True, True, True]
    decays = [wd, wd, 0.0, wd, wd, wd, 0.0, wd]
    scales = [1.0, 0.5, 1.0, 1.0, 2.0, 1.0, 1.0, 0.25]
    segs, n = R.padded_table(NUMELS, scales, decays, adapt)
    p = np.zeros(n, np.float32)
    grads = [np.zeros(n, np.float32) for _ in range(3)]
    for k, s in enumerate(segs):
        sl = slice(s.offset, s.offset + s.numel)
        if k != 3:                                        # segment 3: all-zero parameters
            p[sl] = _rand(s.numel, seed + k)
        for t in range(3):
            if k != 4:                                    # segment 4: all-zero gradients
                grads[t][sl] = _rand(s.numel, seed + 100 * (t + 1) + k, 0.3)
    return segs, n, p, grads


@pytest.mark.parametrize("momentum,nesterov", [(0.9, False), (0.9, True)])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_lars_restatement_is_a_per_tensor_torch_loop_bit_for_bit(momentum, nesterov, wd):
    """The loop is written from the formulas: d = g~ + wd p; q = eta |p| / |d| if adapted and both norms > 0 else 1; d = q d;
    buf = mu buf + d; d = d + mu buf (Nesterov) or buf; p = p - lr_s d — torch float32 tensors, one operation per statement."""
    eta, lr, gs = 0.001, 0.1, 0.5
    segs, n, p, grads = _case(300, wd)
    f = lambda x: torch.tensor(np.float32(x))      # noqa: E731
    tp = [torch.from_numpy(p[s.offset:s.offset + s.numel].copy()) for s in segs]
    tb = [torch.zeros(s.numel) for s in segs]
    buf = np.zeros(n, np.float32)
    for t in range(3):
        p, buf, q = R.lars_step(p, grads[t], buf, segs, lr, momentum, nesterov, eta, gs)
        for k, s in enumerate(segs):
            g = torch.from_numpy(grads[t][s.offset:s.offset + s.numel])
            d = g * f(gs)
            if s.weight_decay != 0:
                d = d + f(s.weight_decay) * tp[k]
            pn, dn = math.sqrt(math.fsum((tp[k].double() ** 2).tolist())), math.sqrt(math.fsum((d.double() ** 2).tolist()))
            qk = f(float(np.float32(eta)) * (pn / dn)) if (s.adapt and pn > 0 and dn > 0) else f(1.0)
            d = qk * d
            tb[k] = f(momentum) * tb[k] + d
            d = d + f(momentum) * tb[k] if nesterov else tb[k]
            tp[k] = tp[k] - (f(lr) * f(s.lr_scale)) * d
            sl = slice(s.offset, s.offset + s.numel)
            assert float(qk) == float(q[k]), (t, k)
            assert np.array_equal(tp[k].numpy().view(np.int32), p[sl].view(np.int32)), (t, k)
            assert np.array_equal(tb[k].numpy().view(np.int32), buf[sl].view(np.int32)), (t, k)
        assert float(q[2]) == 1.0                                  # not adapted
        assert t > 0 or float(q[3]) == 1.0                         # all-zero parameters (until the first step moves them)
        assert wd != 0 or float(q[4]) == 1.0                       # all-zero gradient and no decay term: |d| = 0
    assert float(q[0]) != 1.0


def _lamb_loop64(p, grads, segs, lr, b1, b2, eps, gs):
    """LAMB per tensor in float64 torch, straight from the formulas (hyper-parameters: the float32 values)."""
    b1, b2, eps, gs, lr = (R.f32(x) for x in (b1, b2, eps, gs, lr))
    tp = [torch.from_numpy(p[s.offset:s.offset + s.numel].astype(np.float64)) for s in segs]
    tm, tv = [torch.zeros_like(x) for x in tp], [torch.zeros_like(x) for x in tp]
    for t, g_all in enumerate(grads):
        for k, s in enumerate(segs):
            g = torch.from_numpy(g_all[s.offset:s.offset + s.numel].astype(np.float64)) * gs
            tm[k] = b1 * tm[k] + (1 - b1) * g
            tv[k] = b2 * tv[k] + (1 - b2) * g * g
            mhat, vhat = tm[k] / (1 - b1 ** (t + 1)), tv[k] / (1 - b2 ** (t + 1))
            u = mhat / (vhat.sqrt() + eps) + R.f32(s.weight_decay) * tp[k]
            pn, un = float(tp[k].norm()), float(u.norm())
            r = pn / un if (s.adapt and pn > 0 and un > 0) else 1.0
            tp[k] = tp[k] - lr * R.f32(s.lr_scale) * r * u
    return tp, tm, tv


def test_lamb_restatement_bound_and_planted_faults():
    """(1) the float64 restatement is the independent float64 loop (to 1e-12: the loop divides by the bias corrections where the
    restatement multiplies by reciprocals); (2) the float32 restatement lies inside the derived per-element bound of the
    float64 one over three steps, p, m and v; (3) each planted fault lands at least 10 x outside it."""
    lr, b1, b2, eps, gs = 1e-2, 0.9, 0.999, 1e-6, 0.5
    segs, n, p0, grads = _case(500, 1e-2)
    pad = R.padding_mask(segs, n)

    def run32(fault=None):
        p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
        use = segs
        if fault == "decay_on_excluded":
            use = [s._replace(weight_decay=1e-2) if k == 2 else s for k, s in enumerate(segs)]
        if fault == "padding_in_norm":
            p[pad] = 3.0
        for t, g in enumerate(grads):
            kw = {}
            if fault in ("neighbour_ratio", "ratio_one"):
                _, _, _, r = R.lamb_step(p, g, m, v, use, lr, b1, b2, eps, t + 1, gs)
                kw["ratios"] = ([r[(k + 1) % len(r)] for k in range(len(r))] if fault == "neighbour_ratio"
                                else [np.float32(1.0)] * len(r))
            if fault == "padding_in_norm":
                kw["norm_extra"] = [slice(s.offset + s.numel, (s.offset + s.numel + 3) // 4 * 4) for s in segs]
            p, m, v, _ = R.lamb_step(p, g, m, v, use, lr, b1, b2, eps, t + 1, gs, **kw)
        return p, m, v

    bound = R.LambBound(n)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads):
        p64, m64, v64 = bound.step(p64, g.astype(np.float64), m64, v64, segs, lr, b1, b2, eps, t + 1, gs)
    tp, tm, tv = _lamb_loop64(p0, grads, segs, lr, b1, b2, eps, gs)
    for k, s in enumerate(segs):
        sl = slice(s.offset, s.offset + s.numel)
        np.testing.assert_allclose(p64[sl], tp[k].numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m64[sl], tm[k].numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(v64[sl], tv[k].numpy(), rtol=1e-12, atol=1e-18)
    seg_mask = ~pad
    p, m, v = run32()
    worst = {}
    for name, got, ref, e in (("p", p, p64, bound.ep), ("m", m, m64, bound.em), ("v", v, v64, bound.ev)):
        assert (e[seg_mask] > 0).all() or name != "p"
        ratio = np.abs(got.astype(np.float64) - ref)[seg_mask] / np.maximum(e[seg_mask], 1e-300)
        worst[name] = float(ratio.max())
        assert worst[name] <= 1.0, (name, worst)
    print(f"\n[lamb bound] float32 restatement / bound, worst element: {worst}; bound on p relative to |p|: median "
          f"{float(np.median(bound.ep[seg_mask] / np.maximum(np.abs(p64[seg_mask]), 1e-30))):.2e}")
    for fault in ("neighbour_ratio", "ratio_one", "decay_on_excluded", "padding_in_norm"):
        pf, _, _ = run32(fault)
        out = float((np.abs(pf.astype(np.float64) - p64)[seg_mask] / np.maximum(bound.ep[seg_mask], 1e-300)).max())
        print(f"[lamb bound] planted fault {fault}: {out:.1f} x the bound")
        assert out >= 10.0, (fault, out)
