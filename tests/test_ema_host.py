"""The weight average without a GPU: the numpy restatement the averaging kernels are held to (tests/_ema_ref.py) against torch's
unfused expression and ``torch.lerp``, the warm-up sequence, what the default engines look like (nothing new), what the
keyword refuses, the ``ops`` wrappers' refusals, and the ``avid_ema`` checkpoint entry on CPU engines."""
import warnings

import numpy as np
import pytest
import torch

from _ema_ref import ema_decay_at, ema_sequence, ema_update, ema_weight

DECAYS = (0.9, 0.999, 0.9999)


def _bits(a):
    a = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach().contiguous()
    return a.view(torch.int32)


def _pair(seed, n=1 << 16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


# ---------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("decay", (0.0,) + DECAYS)
def test_restatement_is_torchs_unfused_expression(decay):
    e, p = _pair(1)
    w = float(ema_weight(decay))
    want = e + (p - e) * w
    got = ema_update(e.numpy(), p.numpy(), decay)
    assert got.dtype == np.float32 and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("decay", DECAYS)
def test_distance_to_torch_lerp_is_at_most_one_ulp(decay):
    """torch.lerp (what AveragedModel / ModelEmaV2 run: ``_foreach_lerp_``) evaluates e + w * (p - e) for w < 0.5 with a fused
    multiply-add where the CPU has one: not the same bits, and no equality is asserted.  The two forms differ by ONE rounding,
    that of the product t = w * (p - e) (at most half an ulp of t, and |t| <= max(|e|, |result|) up to that rounding), so after
    the sum's own rounding the results differ by at most one unit in the last place at the larger of |e| and |result|: that
    is asserted for every element.  Wherever the sum does not cancel (|result| >= |e|) this is one ulp of the result itself.
    Where it cancels — e and t of opposite sign, the result smaller than both — one ulp OF THE RESULT cannot hold for any
    unfused evaluation (the product's rounding error is not scaled down with the sum); those elements are counted and
    printed.  N(0,1) data, 65536 elements, decay 0.9 / 0.999 / 0.9999: 11 % / 0.27 % / 0.04 % of elements differ from
    torch.lerp, largest difference 2.4e-7 / 2.4e-7 / 6.0e-8; 886 / 7 / 0 elements exceed one ulp of a cancelled result."""
    e, p = _pair(3)
    w = float(ema_weight(decay))
    ours = ema_update(e.numpy(), p.numpy(), decay)
    inplace = [e.clone()]
    torch._foreach_lerp_(inplace, [p], w)
    for name, theirs in (("lerp", torch.lerp(e, p, w)), ("_foreach_lerp_", inplace[0])):
        theirs = theirs.numpy()
        diff = np.abs(ours.astype(np.float64) - theirs.astype(np.float64))
        result = np.maximum(np.abs(ours), np.abs(theirs)).astype(np.float32)
        ulp_result = np.spacing(result).astype(np.float64)
        ulp = np.spacing(np.maximum(result, np.abs(e.numpy()))).astype(np.float64)
        share = float((ours != theirs).mean())
        cancelled = result < np.abs(e.numpy())
        print(f"\n[ema vs torch.{name}] decay {decay}: {100 * share:.4f} % of elements differ, largest difference {diff.max():.2e}; "
              f"{int((diff > ulp_result).sum())} elements beyond one ulp of a cancelled result")
        assert np.all(diff <= ulp)
        assert np.all(diff[~cancelled] <= ulp_result[~cancelled])


def test_warmup_sequence():
    """d = min(decay, (1 + k) / (10 + k)) for k = 0 .. 20 and where the cap takes over: (1 + k) / (10 + k) >= decay from
    k = (10 decay - 1) / (1 - decay) on."""
    for k in range(21):
        want = min(0.999, (1 + k) / (10 + k))
        assert float(ema_decay_at(0.999, k, True)) == want
        assert ema_weight(0.999, k, True) == np.float32(1.0 - want)
        assert float(ema_decay_at(0.999, k, False)) == 0.999
    assert float(ema_decay_at(0.9, 0, True)) == 0.1 and float(ema_decay_at(0.0, 5, True)) == 0.0
    for decay in DECAYS:
        seq = [float(ema_decay_at(decay, k, True)) for k in range(120000)]
        cap = next(k for k, d in enumerate(seq) if d == decay)
        assert abs(cap - (10 * decay - 1) / (1 - decay)) <= 1.0                      # where (1 + k) / (10 + k) reaches the decay
        assert all(a < b < decay for a, b in zip(seq[:cap - 1], seq[1:cap])) and all(d == decay for d in seq[cap:])
        assert float(ema_decay_at(decay, 10 ** 6, True)) == decay
    # a sequence is the updates one after the other with k counting up
    e, p = _pair(4, 257)
    snaps = [p.numpy() * s for s in (1.0, 0.5, 0.25)]
    want = e.numpy()
    for j, s in enumerate(snaps):
        want = ema_update(want, s, 0.999, 7 + j, True)
    assert np.array_equal(ema_sequence(e.numpy(), snaps, 0.999, True, k0=7), want)


# ------------------------------------------------------------------------------------------------------------------ library
def test_version():
    from avid_hip import lib
    assert lib.version() >= 169
    for s in ("avid_adam_flat_ema", "avid_sgd_flat_ema", "avid_ema_flat", "avid_swap_flat"):
        assert s in lib.SIGNATURES
    import ctypes as C
    assert C.sizeof(lib.EmaDesc) == 32 and lib.EmaDesc.updates_dev.offset == 24


def test_ops_refuse_cpu_tensors():
    from avid_hip import ops, AvidHipError
    p, g, m, v, e = (torch.zeros(8) for _ in range(5))
    k = torch.zeros((), dtype=torch.int64)
    with pytest.raises(AvidHipError):
        ops.adam_flat_ema(p, g, m, v, e, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0.999)
    with pytest.raises(AvidHipError):
        ops.sgd_flat_ema(p, g, None, e, 0.1, 0.0, 0.0, 0.999)
    with pytest.raises(AvidHipError):
        ops.ema_flat(e, p, 0.999, True, k)
    with pytest.raises(AvidHipError):
        ops.swap_flat(p, e)


def test_entry_points_refuse_before_they_launch():
    """No GPU here, so nothing can be launched: the refusals come back through the error convention."""
    import ctypes as C
    from avid_hip import lib
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) & ~15
    P = lambda off=0: C.c_void_p(base + off)     # noqa: E731
    BADARG = -1
    ema = lib.raw("avid_ema_flat")
    assert ema(0, P(), P(64), 0.9, 0, None, None, None) == BADARG and "ema_flat" in lib.last_error()
    assert ema(8, None, P(64), 0.9, 0, None, None, None) == BADARG
    assert ema(8, P(4), P(64), 0.9, 0, None, None, None) == BADARG and "aligned" in lib.last_error()
    for decay in (-0.1, 1.0, 1.5, float("nan")):
        assert ema(8, P(), P(64), decay, 0, None, None, None) == BADARG and "decay" in lib.last_error(), decay
    assert ema(8, P(), P(64), 0.9, 1, None, None, None) == BADARG and "counter" in lib.last_error()
    swap = lib.raw("avid_swap_flat")
    assert swap(8, P(), P(), None) == BADARG and "overlap" in lib.last_error()
    assert swap(8, P(), P(16), None) == BADARG and "overlap" in lib.last_error()
    assert swap(8, P(16), P(), None) == BADARG
    assert swap(0, P(), P(64), None) == BADARG and swap(8, None, P(64), None) == BADARG and swap(8, P(2), P(64), None) == BADARG
    adam, sgd = lib.raw("avid_adam_flat_ema"), lib.raw("avid_sgd_flat_ema")
    good = lib.EmaDesc(P(128).value, 0.9, 0, None)
    for desc, word in ((None, "average"), (lib.EmaDesc(None, 0.9, 0, None), "average"), (lib.EmaDesc(P(132).value, 0.9, 0, None), "aligned"),
                       (lib.EmaDesc(P(128).value, 1.0, 0, None), "decay"), (lib.EmaDesc(P(128).value, float("nan"), 0, None), "decay"),
                       (lib.EmaDesc(P(128).value, 0.9, 1, None), "counter")):
        ref = None if desc is None else C.byref(desc)
        assert adam(8, P(), P(32), P(64), P(96), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 1.0, None, ref, None) == BADARG
        assert "adam_flat_ema" in lib.last_error() and word in lib.last_error(), (word, lib.last_error())
        assert sgd(8, P(), P(32), P(64), 0.1, 0.9, 0.0, 0, None, 1.0, None, ref, None) == BADARG
        assert "sgd_flat_ema" in lib.last_error() and word in lib.last_error(), (word, lib.last_error())
    assert adam(0, P(), P(32), P(64), P(96), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 1.0, None, C.byref(good), None) == BADARG
    assert adam(8, P(4), P(32), P(64), P(96), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, 1.0, None, C.byref(good), None) == BADARG
    assert sgd(8, P(), P(32), None, 0.1, 0.9, 0.0, 0, None, 1.0, None, C.byref(good), None) == BADARG


# ------------------------------------------------------------------------------------------------------------------ engines
def _tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.BatchNorm1d(8), torch.nn.ReLU(), torch.nn.Linear(8, 3))


class _Wrapped(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(1)
        self.feature_extractor = torch.nn.Sequential(torch.nn.Linear(6, 6), torch.nn.BatchNorm1d(6))
        self.classifier = torch.nn.Linear(6, 3)


def test_default_engines_carry_nothing_new():
    from avid_hip.parallel import FinetuneStep, TrainStep
    for eng in (TrainStep(_tiny_model(), criterion=None), TrainStep(_tiny_model(), criterion=None, optimizer="sgd", momentum=0.9),
                FinetuneStep(_Wrapped()), FinetuneStep(_Wrapped(), classifier_only=True)):
        assert eng.ema_decay is None and eng.ema is None and eng.ema_updates is None and eng.ema_buffers_flat is None
        assert not any(isinstance(v, torch.Tensor) for k, v in vars(eng).items() if "ema" in k)
        assert sorted(eng.state_dict()) == ["param_groups", "state"]
        for what in (eng.ema_reset, eng.ema_state_dict, lambda: eng.ema_weights().__enter__()):
            with pytest.raises(RuntimeError, match="ema_decay"):
                what()
        # a checkpoint that carries an average loads into an engine without one: the key is ignored
        sd = eng.state_dict()
        sd["avid_ema"] = {"decay": 0.9, "warmup": False, "num_updates": 3, "params": {}, "buffers": None}
        eng.load_state_dict(sd)
        assert eng.ema is None and sorted(eng.state_dict()) == ["param_groups", "state"]


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_bad_decays_are_refused_before_anything_is_flattened(bad):
    from avid_hip.parallel import FinetuneStep, ProbeStep, TrainStep
    for make in (lambda m: TrainStep(m, criterion=None, ema_decay=bad), lambda m: FinetuneStep(m, ema_decay=bad)):
        m = _Wrapped()
        ptrs = [p.data_ptr() for p in m.parameters()]
        with pytest.raises(ValueError, match="ema_decay"):
            make(m)
        assert [p.data_ptr() for p in m.parameters()] == ptrs
    import inspect
    assert "ema_decay" in inspect.signature(ProbeStep.__init__).parameters


def test_engine_with_an_average_starts_as_a_copy():
    from avid_hip.parallel import TrainStep
    eng = TrainStep(_tiny_model(), criterion=None, ema_decay=0.0)          # 0 is a legal decay
    assert eng.ema_decay == 0.0 and eng.ema.data_ptr() != eng.flat.flat.data_ptr() and torch.equal(eng.ema, eng.flat.flat)
    assert eng.ema_updates.dtype == torch.int64 and eng.ema_updates.dim() == 0 and int(eng.ema_updates) == 0
    assert torch.equal(eng.ema_buffers_flat, eng.flat_buffers.flat) and eng.ema_buffers_flat.data_ptr() != eng.flat_buffers.flat.data_ptr()
    assert TrainStep(_tiny_model(), criterion=None, ema_decay=0.9, ema_buffers=False).ema_buffers_flat is None
    with torch.no_grad():
        eng.flat.flat.add_(1.0)
        eng.flat_buffers.flat.add_(2.0)
        eng.ema_updates.fill_(4)
    eng.ema_reset()
    assert torch.equal(eng.ema, eng.flat.flat) and torch.equal(eng.ema_buffers_flat, eng.flat_buffers.flat) and int(eng.ema_updates) == 0


# -------------------------------------------------------------------------------------------------------------- checkpoints
def _disturb(eng, seed):
    """Random values into the average through the parameters' and buffers' own views (the padding between slices stays)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for i, p in enumerate(eng.flat.params):
            eng.flat.view(eng.ema, i).copy_(torch.randn(p.shape, generator=g))
        for _, view in eng._ema_buffer_views():
            view.copy_(torch.randn(view.shape, generator=g))
        eng.ema_updates.fill_(seed)


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_checkpoint_round_trip(optimizer):
    from avid_hip.parallel import TrainStep
    kw = dict(optimizer=optimizer, momentum=0.9) if optimizer == "sgd" else {}
    m = _tiny_model()
    eng = TrainStep(m, criterion=None, ema_decay=0.999, ema_warmup=True, **kw)
    _disturb(eng, 7)
    sd = eng.state_dict()
    assert sorted(sd) == ["avid_ema", "param_groups", "state"]
    saved = sd["avid_ema"]
    assert sorted(saved) == ["buffers", "decay", "num_updates", "params", "warmup"]
    assert (saved["decay"], saved["warmup"], saved["num_updates"]) == (0.999, True, 7)
    params = list(m.parameters())
    assert sorted(saved["params"]) == list(range(len(params)))
    for k, i, p in eng._param_order():
        assert saved["params"][k].shape == p.shape and torch.equal(saved["params"][k], eng.flat.view(eng.ema, i))
        assert saved["params"][k].data_ptr() != eng.flat.view(eng.ema, i).data_ptr()          # a copy, not a view
    assert sorted(saved["buffers"]) == ["1.running_mean", "1.running_var"]                 # no num_batches_tracked
    fresh = TrainStep(_tiny_model(), criterion=None, ema_decay=0.5, **kw)
    fresh.load_state_dict(sd)
    assert (fresh.ema_decay, fresh.ema_warmup, int(fresh.ema_updates)) == (0.999, True, 7)
    assert torch.equal(fresh.ema, eng.ema) and torch.equal(fresh.ema_buffers_flat, eng.ema_buffers_flat)
    # the averaged model: state_dict's keys and shapes, averaged where covered, live elsewhere; loads strictly
    esd = eng.ema_state_dict()
    live = m.state_dict()
    assert list(esd) == list(live) and all(esd[k].shape == live[k].shape and esd[k].dtype == live[k].dtype for k in live)
    names = [n for n, _ in m.named_parameters()]
    for k, i, p in eng._param_order():
        assert torch.equal(esd[names[k]], eng.flat.view(eng.ema, i))
    assert torch.equal(esd["1.running_mean"], saved["buffers"]["1.running_mean"])
    assert torch.equal(esd["1.num_batches_tracked"], live["1.num_batches_tracked"])
    _tiny_model().load_state_dict(esd, strict=True)
    # an engine with an average keeps it when the checkpoint has none, and says so
    plain = TrainStep(_tiny_model(), criterion=None, **kw).state_dict()
    before = fresh.ema.clone()
    with pytest.warns(UserWarning, match="no weight average"):
        fresh.load_state_dict(plain)
    assert torch.equal(fresh.ema, before) and int(fresh.ema_updates) == 7
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fresh.load_state_dict(sd)                          # a checkpoint with the average: no warning


def test_checkpoint_without_averaged_statistics():
    from avid_hip.parallel import TrainStep
    eng = TrainStep(_tiny_model(), criterion=None, ema_decay=0.9, ema_buffers=False)
    sd = eng.state_dict()
    assert sd["avid_ema"]["buffers"] is None
    esd = eng.ema_state_dict()
    assert torch.equal(esd["1.running_var"], eng.model.state_dict()["1.running_var"])      # live statistics
    TrainStep(_tiny_model(), criterion=None, ema_decay=0.9, ema_buffers=False).load_state_dict(sd)


def test_classifier_only_numbering():
    """FinetuneStep(classifier_only=True): the optimizer holds the classifier's two parameters, numbered 0 and 1 — and so does
    the average's checkpoint entry; the tower's slice of the average is the untouched copy."""
    from avid_hip.parallel import FinetuneStep
    m = _Wrapped()
    eng = FinetuneStep(m, classifier_only=True, ema_decay=0.99)
    tower = eng.ema[eng.n_cls:].clone()
    with torch.no_grad():
        eng.ema[:eng.n_cls].mul_(0.5)
    sd = eng.state_dict()
    assert sd["param_groups"][0]["params"] == [0, 1] and sorted(sd["avid_ema"]["params"]) == [0, 1]
    assert torch.equal(sd["avid_ema"]["params"][0], 0.5 * m.classifier.weight) and torch.equal(sd["avid_ema"]["params"][1], 0.5 * m.classifier.bias)
    fresh = FinetuneStep(_Wrapped(), classifier_only=True, ema_decay=0.99)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.ema, eng.ema) and torch.equal(fresh.ema[fresh.n_cls:], tower)
    esd = eng.ema_state_dict()
    assert torch.equal(esd["classifier.weight"], 0.5 * m.classifier.weight)
    assert torch.equal(esd["feature_extractor.0.weight"], m.feature_extractor[0].weight)
    # the full engine numbers every parameter
    full = FinetuneStep(_Wrapped(), ema_decay=0.99)
    assert sorted(full.state_dict()["avid_ema"]["params"]) == list(range(len(list(m.parameters()))))
