"""The ordering between the step's four streams, tested by making one of them late (tests/_delay.py).

A step is deterministic from run to run, so with every wait in place its results cannot depend on when a stream gets to its
work.  Each case runs two consecutive steps with different inputs — the first undisturbed, so that every arena, bank and
buffer holds valid earlier data — and in the second puts a delay of D = max(3 x T0, 5 ms) on one stream (T0: the undisturbed
step, measured here), at every cut of the launch programs (behind each wait record, and evenly spaced) or in front of a launching
call; everything the step leaves must be the bits the undisturbed pair leaves from the same initial state.  A difference is a
missing ordering: the smallest cut and the stream name the records (``plan.dump``).

The control comes first: the same delay on a hand-made three-record program whose wait is switched off DOES change the result,
for every ordered pair of the four streams — the delay really reorders.  No control removes a wait from a model program.

Every test is one GPU step under its own time limit (a watchdog ends the process: a hung kernel cannot be interrupted from
Python), and after a failed step the remaining ones fail without touching the GPU."""
import contextlib
import ctypes as C
import faulthandler
import functools
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delay  # noqa: E402
import _inference_probe as ip  # noqa: E402
import test_gpu_plan as tp  # noqa: E402

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 120
_STATE = {"failed": None}
STREAMS = ["compute", "audio", "trailing", "fourth"]


def gpu_step(fn):
    @functools.wraps(fn)
    def wrapper(*a, **k):
        if _STATE["failed"]:
            pytest.fail(f"not run: the earlier GPU step {_STATE['failed']} failed")
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        try:
            return fn(*a, **k)
        except BaseException:
            _STATE["failed"] = fn.__name__
            raise
        finally:
            faulthandler.cancel_dump_traceback_later()
    return wrapper


# ------------------------------------------------------------------------------------------------------------------ 3a
@gpu_step
def test_control_a_delay_reorders_what_no_wait_orders(gpu_device):
    """MEMSET0 X on stream p | WAIT c <- p | COLSUM X -> out on stream c, with a delay on p in front: with the wait out is 0,
    with the wait record switched off (op 0) the column sums are those of the stale ones, exactly 256 — for all 12 ordered
    pairs of the four placed streams.  Reads only initialised floats, indexes nothing by what it reads."""
    from avid_hip import lib, plan, streams
    dev = gpu_device
    ss = streams.place(dev)
    four = (ss.main, ss.side, ss.trail, ss.comm)
    assert len({s.cuda_stream for s in four}) == 4, streams.report(dev)
    X = torch.empty((256, 64), dtype=torch.float32, device=dev)
    out = torch.empty(64, dtype=torch.float32, device=dev)
    slots = (C.c_void_p * 2)(X.data_ptr(), out.data_ptr())
    handles = (C.c_void_p * 4)(*[s.cuda_stream for s in four])
    ws = [torch.empty(256, dtype=torch.uint8, device=dev) for _ in range(4)]
    ws_arr = (lib.StreamWs * 4)()
    for k in range(4):
        ws_arr[k].ptr, ws_arr[k].bytes = ws[k].data_ptr(), 256

    def program(p, c, wait):
        recs = (lib.Instr * 3)()
        for r in recs:
            for j in range(lib.INSTR_REFS):
                r.t[j].slot = -1
        recs[0].op, recs[0].stream = plan.OP_MEMSET0, p
        recs[0].n[0] = 4 * X.numel()
        recs[0].t[0].slot, recs[0].t[0].off = 0, 0
        recs[1].op = plan.OP_WAIT if wait else 0
        recs[1].i[0], recs[1].i[1] = c, p
        recs[2].op, recs[2].stream = plan.OP_COLSUM, c
        recs[2].n[0], recs[2].i[0] = 256, 64
        recs[2].t[0].slot, recs[2].t[1].slot = 0, 1
        return recs

    def run(recs, p, ms):
        X.fill_(1.0)
        out.fill_(-1.0)
        torch.cuda.synchronize()
        if ms:
            _delay.spin(handles[p], ms)
        lib.call("avid_program_run", recs, 0, 3, slots, 2, handles, ws_arr, 4)
        torch.cuda.synchronize()
        return out.clone()

    recs = program(2, 0, True)
    t0 = _delay.time_ms(lambda: lib.call("avid_program_run", recs, 0, 3, slots, 2, handles, ws_arr, 4))
    D = _delay.delay_ms(t0)
    print(f"\n[stream delays] control: T0 {t0:.3f} ms, D {D:.1f} ms")
    bad = []
    for p in range(4):
        for c in range(4):
            if p == c:
                continue
            ordered, stale = run(program(p, c, True), p, D), run(program(p, c, False), p, D)
            if not bool((ordered == 0).all()):
                bad.append((STREAMS[p], STREAMS[c], "with the wait", ordered[:4].tolist()))
            if not bool((stale == 256).all()):
                bad.append((STREAMS[p], STREAMS[c], "without the wait", stale[:4].tolist()))
    assert not bad, (bad, streams.report(dev))


# ------------------------------------------------------------------------------------------------------------------ 3b
def _clone(t):
    return [x.clone() for x in t] if isinstance(t, (list, tuple)) else t.clone()


def _engine_state(eng, model, crit=None):
    """Everything a step leaves: flat gradient buffer, parameters, optimizer moments and step counter, BatchNorm buffers,
    the criterion's state dict."""
    out = {"grad": eng.flat.grad.clone(), "params": eng.flat.flat.clone(), "m": eng.m.clone(), "v": eng.v.clone(),
           "t": (eng.t, int(eng.t_dev))}
    for n, b in model.named_buffers():
        out["buffer:" + n] = b.clone()
    if crit is not None:
        for k, v in crit.state_dict().items():
            out["criterion:" + k] = v.clone()
    return out


def _differences(a, b):
    assert sorted(a) == sorted(b)
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, list):
            same = len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
        elif torch.is_tensor(x):
            same = torch.equal(x, y)
        else:
            same = x == y
        if not same:
            bad.append(k)
    return bad


def _reset_engine(eng):
    eng.m.zero_()
    eng.v.zero_()
    eng.t_dev.zero_()
    eng.flat.grad.zero_()
    eng.t = 0


class Arrangement:
    """One engine, its saved initial state and a pair of inputs.  ``pair(ctx)``: from the initial state, step 1 undisturbed,
    then step 2 inside ``ctx``; returns (what the pair leaves, what ``ctx`` yielded)."""

    def __init__(self, name, reset, step, collect):
        self.name, self.reset, self.step, self.collect = name, reset, step, collect
        self.reference = self.t0 = self.D = None
        self.runs = 0

    def pair(self, ctx=None):
        self.reset()
        self.step(0)
        with (ctx if ctx is not None else contextlib.nullcontext()) as fired:
            out = self.step(1)
        torch.cuda.synchronize()
        self.runs += 1
        return self.collect(out), fired

    def prepare(self):
        """The reference pair (twice: the step is deterministic, or nothing below means anything), then T0 and D of step 2."""
        self.reference, _ = self.pair()
        again, _ = self.pair()
        assert not _differences(self.reference, again), "two undisturbed runs differ"
        self.reset()
        self.step(0)
        self.t0 = _delay.time_ms(lambda: self.step(1))
        self.D = _delay.delay_ms(self.t0)
        print(f"\n[stream delays] {self.name}: T0 {self.t0:.3f} ms, D {self.D:.1f} ms")
        return self

    def check(self, cases):
        """``cases``: [(label, context manager)] — every one must leave the reference's bits and must have injected its delay."""
        bad = []
        for label, ctx in cases:
            got, fired = self.pair(ctx)
            assert fired.spins == 1, (self.name, label, fired.spins)
            diff = _differences(self.reference, got)
            if diff:
                bad.append((label, diff[:6]))
        assert not bad, f"{self.name}: a delayed stream changed the step's results at {len(bad)} of {len(cases)} injections: {bad[:8]}"


def _av_state():
    """The deterministic two-tower weights of tests/test_gpu_plan.py, generated once."""
    sd = _CACHE.get("av_sd")
    if sd is None:
        sd = _CACHE["av_sd"] = {k: v.cpu().clone() for k, v in tp._model(torch.device("cpu")).state_dict().items()}
    return sd


def _av_model(dev):
    import models
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])
    m.load_state_dict(_av_state())
    return m.to(dev).train()


def _av_inputs(dev, bs):
    video, audio, ids = tp._data(dev, bs=bs, steps=2, hw=64)
    g = torch.Generator().manual_seed(17)
    video2, audio2 = torch.randn(video.shape, generator=g).to(dev), torch.randn(audio.shape, generator=g).to(dev)
    return [(video, audio, ids[0]), (video2, audio2, ids[1])]


def _train_arrangement(name, dev, virtual_ranks=1, whole_step=True):
    from avid_hip.parallel import TrainStep
    m, crit = _av_model(dev), tp._crit(dev)
    eng = TrainStep(m, crit, virtual_ranks=virtual_ranks)
    inputs = _av_inputs(dev, 4 * virtual_ranks)
    sd_m = {k: v.clone() for k, v in m.state_dict().items()}
    sd_c = {k: v.clone() for k, v in crit.state_dict().items()}
    seeds = [s for s, _ in eng._rank_sampler] if virtual_ranks > 1 else None

    def reset():
        m.load_state_dict(sd_m)
        crit.load_state_dict(sd_c)
        _reset_engine(eng)
        if seeds is not None:
            eng.reseed(seeds, 0)
        else:
            crit.nce_average.multinomial.reseed(11, 0)

    def step(i):
        if whole_step:
            return eng.step(*inputs[i])
        loss = eng.forward_backward(*inputs[i])
        eng.optimizer_step()
        return loss.detach()

    def collect(loss):
        return {"loss": loss.clone(), **_engine_state(eng, m, crit)}

    arr = Arrangement(name, reset, step, collect)
    arr.eng, arr.model = eng, m
    return arr


@contextlib.contextmanager
def _tapped(cls, sink):
    """The logits a plan's forward returns (views of the forward arena, which the step releases), copied on the compute stream."""
    original = cls.forward

    def forward(self, *a, **k):
        res = original(self, *a, **k)
        sink.append(_clone(res[0]))
        return res
    cls.forward = forward
    try:
        yield
    finally:
        cls.forward = original


def _supervised_arrangement(name, dev, kind):
    from avid_hip import parallel, plan
    if kind == "finetune":
        m, n_classes, plan_cls = ip.wrapper(dev), 101, plan.ClsPlan
        eng = parallel.FinetuneStep(m)
    else:
        m, n_classes, plan_cls = ip.most_model(dev), 400, plan.ProbePlan
        eng = parallel.ProbeStep(m)
    g = torch.Generator().manual_seed(23)
    inputs = [(torch.randn((4, 3, 8, 64, 64), generator=g).to(dev), torch.randint(0, n_classes, (4,), generator=g).to(dev))
              for _ in range(2)]
    sd_m = {k: v.clone() for k, v in m.state_dict().items()}
    drop = getattr(m, "dropout", None)
    offset0 = drop.offset if hasattr(drop, "offset") else None

    def reset():
        m.load_state_dict(sd_m)
        _reset_engine(eng)
        if offset0 is not None:
            drop.offset = offset0

    def step(i):
        sink = []
        with _tapped(plan_cls, sink):
            loss, hits = eng.step(*inputs[i])
        (logits,) = sink
        return loss, hits, logits

    def collect(out):
        loss, hits, logits = out
        return {"loss": loss.clone(), "hits": hits.clone(), "logits": _clone(logits), **_engine_state(eng, m)}

    arr = Arrangement(name, reset, step, collect)
    arr.eng, arr.model = eng, m
    return arr


def _inference_arrangement(name, dev):
    from avid_hip import parallel
    m = _av_model(dev)
    infer = parallel.Inference(m)
    inputs = [x[:2] for x in _av_inputs(dev, 4)]

    def step(i):
        out = infer(*inputs[i])
        assert infer.used_programs is True
        return out

    arr = Arrangement(name, lambda: None, step, lambda out: {"video": out[0].clone(), "audio": out[1].clone()})
    arr.model = m
    return arr


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines live for this module only: the rest of the suite gets their memory back."""
    yield
    _CACHE.clear()


def _arrangement(key, make):
    """Built once per module: the engine, the undisturbed reference and the measured delay are shared by the four streams' tests
    and left unchanged."""
    arr = _CACHE.get(key)
    if arr is None:
        arr = _CACHE[key] = make().prepare()
    return arr


def _program_cases(pl, stream, D, which=("fwd", "bwd"), visit=None):
    cases = []
    for w in which:
        prog, n = (pl.fwd_prog, pl.n_fwd) if w == "fwd" else (pl.bwd_prog, pl.n_bwd)
        for cut in _delay.program_cuts(prog, n):
            cases.append((f"{w}@{cut}", _delay.delayed_programs(stream, cut, D, w, visit=visit)))
    return cases


def _report(arr, cases, t_start):
    print(f"[stream delays] {arr.name}: {len(cases)} injections, {time.perf_counter() - t_start:.2f} s")


@pytest.mark.parametrize("stream", range(4), ids=STREAMS)
@gpu_step
def test_a_engine_step_over_the_programs(gpu_device, stream):
    """A: TrainStep.step() over the launch programs — four streams, deferred and grouped weight gradients, the overlapped
    optimizer step — delayed at every cut of the forward and of the backward program and at the three phase boundaries (in
    front of the criterion, of the backward, of the optimizer; a delay at cut 0 of the forward is the one between two steps)."""
    t_start = time.perf_counter()
    arr = _arrangement("A", lambda: _train_arrangement("A TrainStep.step, programs", gpu_device))
    pl = arr.eng._step_plan
    assert pl is not None and pl.adam_early, "step() did not take the overlapped optimizer path"
    cases = _program_cases(pl, stream, arr.D)
    _, dry = arr.pair(_delay.delayed_calls(stream, None, 0))
    runs = [k for k, n in enumerate(dry.names) if n == "avid_program_run"]
    assert len(runs) == 2, dry.names
    for label, nth in (("criterion", runs[0] + 1), ("backward", runs[1]), ("optimizer", runs[1] + 1)):
        assert nth < dry.count, (label, dry.names)
        cases.append((f"before the {label} (call {nth})", _delay.delayed_calls(stream, nth, arr.D)))
    arr.check(cases)
    _report(arr, cases, t_start)


@pytest.mark.parametrize("stream", range(4), ids=STREAMS)
@gpu_step
def test_b_engine_step_on_the_per_layer_path(gpu_device, per_layer_path, stream):
    """B: the same step on the per-layer path (``ops.DEFER_WGRAD`` at its default), forward_backward() + optimizer_step(),
    delayed in front of launching call 0 and of 12 evenly spaced ones."""
    from avid_hip import ops
    t_start = time.perf_counter()
    assert ops.DEFER_WGRAD
    arr = _arrangement("B", lambda: _train_arrangement("B forward_backward + optimizer_step, per-layer path", gpu_device,
                                                       whole_step=False))
    assert not [p for p in arr.model.__dict__.get("_avid_plans", {}).values() if p], "the per-layer step compiled a program"
    _, dry = arr.pair(_delay.delayed_calls(stream, None, 0))
    assert dry.count > 100 and "avid_program_run" not in dry.names, dry.count
    nths = sorted({0} | {dry.count * j // 13 for j in range(1, 13)})
    cases = [(f"call {nth} ({dry.names[nth]})", _delay.delayed_calls(stream, nth, arr.D)) for nth in nths]
    arr.check(cases)
    _report(arr, cases, t_start)


@pytest.mark.parametrize("stream", range(4), ids=STREAMS)
@gpu_step
def test_c_second_shard_of_a_virtual_rank_step(gpu_device, stream):
    """C: TrainStep(virtual_ranks=2): the second shard's forward runs with ``tables=False`` and reads the weight tables the
    first shard's built on the trailing stream — delayed at every cut of that second forward."""
    t_start = time.perf_counter()
    arr = _arrangement("C", lambda: _train_arrangement("C TrainStep(virtual_ranks=2)", gpu_device, virtual_ranks=2))
    pl = arr.eng._step_plan
    assert pl is not None and pl.vshape[0] == 4
    cases = _program_cases(pl, stream, arr.D, which=("fwd",), visit=1)
    arr.check(cases)
    _report(arr, cases, t_start)


@pytest.mark.parametrize("stream", range(4), ids=STREAMS)
@pytest.mark.parametrize("kind", ["finetune", "probe"])
@gpu_step
def test_d_supervised_steps(gpu_device, kind, stream):
    """D: FinetuneStep (ClsPlan) and ProbeStep (ProbePlan), one step pair each, delayed at every cut of the forward and of the
    backward program; compared as the others, plus the logits and the hit counts."""
    from avid_hip import plan
    t_start = time.perf_counter()
    name = "D FinetuneStep" if kind == "finetune" else "D ProbeStep"
    arr = _arrangement("D" + kind, lambda: _supervised_arrangement(name, gpu_device, kind))
    pl = arr.eng._step_plan
    assert type(pl) is (plan.ClsPlan if kind == "finetune" else plan.ProbePlan)
    cases = _program_cases(pl, stream, arr.D)
    arr.check(cases)
    _report(arr, cases, t_start)


@pytest.mark.parametrize("stream", range(4), ids=STREAMS)
@gpu_step
def test_e_inference_program(gpu_device, stream):
    """E: parallel.Inference on the two-tower model (EvalPlan: the audio tower on its own stream, activations in a recycled
    arena), two calls with different inputs, the second delayed at every cut of the program; the embeddings are compared."""
    t_start = time.perf_counter()
    arr = _arrangement("E", lambda: _inference_arrangement("E Inference, two-tower EvalPlan", gpu_device))
    (pl,) = [v for k, v in arr.model.__dict__.get("_avid_plans", {}).items() if k[0] == "eval" and v]
    cases = _program_cases(pl, stream, arr.D, which=("fwd",))
    arr.check(cases)
    _report(arr, cases, t_start)
