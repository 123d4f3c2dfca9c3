"""SGD with momentum on a real MI355X: ``avid_sgd_flat`` against the float32 numpy restatement (tests/_sgd_ref.py) BIT FOR BIT —
the kernel is built without floating-point contraction, so every product and sum rounds where numpy's does —, the device-resident
learning rate, guard bands, the three step engines under ``optimizer="sgd"``, a captured graph, checkpoints interchanged with
torch.optim.SGD, and the reference's loop with ``DistributedDataParallel`` + ``parallel.SGD``."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from _sgd_ref import sgd_step

pytestmark = pytest.mark.gpu

SGD = dict(momentum=0.9, nesterov=True, weight_decay=1e-4)          # the engines' configuration below
BIG = 4 * 256 * 4096 + 7      # the grid-stride loop's second round (4096 blocks x 256 threads x 4 floats) and a tail


def _bits(t):
    t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t.detach().cpu()
    return t.contiguous().view(torch.int32)


def _same_bits(got, want):
    return torch.equal(_bits(got), _bits(want))


def _rand(n, seed, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, BIG])
def test_kernel_is_the_float32_restatement(gpu_device, n):
    """Three successive steps, p and buf, over {no momentum (buf=None), momentum, nesterov} x wd {0, 1e-4} x grad_scale {1, 0.5}.
    n: the tail alone (1, 3), no tail (4), body + tail (5, 1027), and a size that enters the grid-stride loop twice."""
    from avid_hip import ops
    dev = gpu_device
    p0 = _rand(n, 1)
    grads = [_rand(n, 10 + s, 0.3) for s in range(3)]
    gd = [g.to(dev) for g in grads]
    bad = []
    for momentum, nesterov in ((0.0, False), (0.9, False), (0.9, True)):
        for wd in (0.0, 1e-4):
            for gs in (1.0, 0.5):
                p = p0.to(dev)
                buf = torch.zeros(n, device=dev) if momentum else None
                wp, wb = p0.numpy(), (np.zeros(n, np.float32) if momentum else None)
                for s in range(3):
                    ops.sgd_flat(p, gd[s], buf, 0.1, momentum, wd, nesterov, grad_scale=gs)
                    wp, wb = sgd_step(wp, grads[s].numpy(), wb, 0.1, momentum, wd, nesterov, gs)
                    ok = _same_bits(p, wp) and (buf is None or _same_bits(buf, wb))
                    if not ok:
                        bad.append((momentum, nesterov, wd, gs, s, float((p.cpu() - torch.from_numpy(wp)).abs().max())))
                        break
    assert not bad, bad


def test_kernel_on_a_slice_leaves_the_rest_alone(gpu_device):
    from avid_hip import ops
    dev, N, off, n = gpu_device, 2048, 8, 1027
    full_p, full_g, full_b = _rand(N, 2), _rand(N, 3, 0.3), _rand(N, 4, 0.1)
    p, g, b = full_p.to(dev), full_g.to(dev), full_b.to(dev)
    s = slice(off, off + n)
    ops.sgd_flat(p[s], g[s], b[s], 0.05, 0.9, 1e-4, True)
    wp, wb = sgd_step(full_p[s].numpy(), full_g[s].numpy(), full_b[s].numpy(), 0.05, 0.9, 1e-4, True)
    assert _same_bits(p[s], wp) and _same_bits(b[s], wb)
    for got, was in ((p, full_p), (b, full_b)):
        assert _same_bits(got[:off], was[:off]) and _same_bits(got[off + n:], was[off + n:])
    assert _same_bits(g, full_g)


def test_bad_arguments_come_back_through_the_error_convention(gpu_device):
    from avid_hip import lib
    dev = gpu_device
    p, g, b = (torch.zeros(64, device=dev) for _ in range(3))
    P = lambda t, byte_off=0: None if t is None else C.c_void_p(t.data_ptr() + byte_off)   # noqa: E731
    call = lib.raw("avid_sgd_flat")
    BADARG = -1                                                            # include/avid_hip.h: AVID_E_BADARG
    cases = {"n == 0": (0, P(p), P(g), P(b), 0.1, 0.9, 0.0, 0), "n < 0": (-4, P(p), P(g), P(b), 0.1, 0.9, 0.0, 0),
             "no p": (16, None, P(g), P(b), 0.1, 0.9, 0.0, 0), "no g": (16, P(p), None, P(b), 0.1, 0.9, 0.0, 0),
             "momentum without buf": (16, P(p), P(g), None, 0.1, 0.9, 0.0, 0),
             "misaligned p": (16, P(p, 4), P(g), P(b), 0.1, 0.9, 0.0, 0), "misaligned g": (16, P(p), P(g, 8), P(b), 0.1, 0.9, 0.0, 0),
             "misaligned buf": (16, P(p), P(g), P(b, 4), 0.1, 0.9, 0.0, 0),
             "nesterov without momentum": (16, P(p), P(g), None, 0.1, 0.0, 0.0, 1)}
    for what, args in cases.items():
        assert call(*args, None, 1.0, None) == BADARG and "sgd_flat" in lib.last_error(), what
    with pytest.raises(lib.AvidHipError, match="sgd_flat"):
        lib.call("avid_sgd_flat", 16, P(p), P(g), None, 0.1, 0.0, 0.0, 1, None, 1.0, None)
    torch.cuda.synchronize()
    assert not p.any() and not b.any()                                     # nothing was launched
    assert call(16, P(p), P(g), None, 0.1, 0.0, 0.0, 0, None, 1.0, None) == 0      # buf may be NULL exactly without momentum


def test_learning_rate_is_read_from_the_device_word(gpu_device):
    from avid_hip import ops
    dev, n = gpu_device, 1027
    p0, g = _rand(n, 5).to(dev), _rand(n, 6, 0.3).to(dev)
    plain_p, plain_b = p0.clone(), torch.zeros(n, device=dev)
    dev_p, dev_b = p0.clone(), torch.zeros(n, device=dev)
    lr_dev = torch.full((), 0.05, dtype=torch.float32, device=dev)
    ops.sgd_flat(plain_p, g, plain_b, 0.05, 0.9, 1e-4, True)
    ops.sgd_flat(dev_p, g, dev_b, 123.0, 0.9, 1e-4, True, lr_dev=lr_dev)   # the host's lr is wrong and not used
    assert _same_bits(dev_p, plain_p) and _same_bits(dev_b, plain_b)
    lr_dev.fill_(0.002)
    ops.sgd_flat(plain_p, g, plain_b, 0.002, 0.9, 1e-4, True)
    ops.sgd_flat(dev_p, g, dev_b, 123.0, 0.9, 1e-4, True, lr_dev=lr_dev)
    assert _same_bits(dev_p, plain_p) and _same_bits(dev_b, plain_b)


def test_no_write_outside_the_buffers(gpu_device):
    """tests/_guards.py: the op under both fills and plain at n = 1027 with momentum and nesterov; no guard byte changes and p /
    buf are the same bits in all three runs."""
    from _guards import FILLS, guarded
    from avid_hip import ops
    dev, n = gpu_device, 1027

    def run(P):
        p, g = P(_rand(n, 7).to(dev)), P(_rand(n, 8, 0.3).to(dev))
        buf, lr_dev = P(_rand(n, 9, 0.1).to(dev)), P(torch.full((), 0.05, dtype=torch.float32).to(dev))
        ops.sgd_flat(p, g, buf, 0.05, 0.9, 1e-4, True, grad_scale=0.5)
        ops.sgd_flat(p, g, buf, 0.0, 0.9, 1e-4, True, grad_scale=0.5, lr_dev=lr_dev)
        torch.cuda.synchronize()
        return _bits(p), _bits(buf), _bits(g)

    plain = run(lambda t: t)
    for fill in FILLS:
        with guarded(fill) as g:
            got = run(g.place)
            g.check()
        assert sum(r.kind == "input" for r in g.records) == 4
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), hex(fill)


# ----------------------------------------------------------------------------------------------------------------- engines
def _trainstep(dev, **kw):
    import test_gpu_engine as E
    from avid_hip.parallel import TrainStep
    import test_gpu_plan as GP
    m, crit = E._model(dev), GP._crit(dev)                 # what E._make builds, with the engine's keywords open
    return m, crit, TrainStep(m, crit, **kw)


def _check_steps(eng, step, n_steps, lr, begin=0, end=None):
    """Before each step clone flat.flat and momentum_buffer, after it read flat.grad: the engine's new buffers are the restatement
    applied to the clones over [begin, end) and untouched elsewhere."""
    end = eng.flat.numel if end is None else end
    for i in range(n_steps):
        p0, b0 = eng.flat.flat.clone(), eng.momentum_buffer.clone()
        step(i)
        torch.cuda.synchronize()
        g = eng.flat.grad
        assert bool(g[begin:end].any()), "the step produced no gradient"
        wp, wb = sgd_step(p0[begin:end].cpu().numpy(), g[begin:end].cpu().numpy(), b0[begin:end].cpu().numpy(), lr,
                          SGD["momentum"], SGD["weight_decay"], SGD["nesterov"], 1.0)
        assert _same_bits(eng.flat.flat[begin:end], wp), ("parameters", i)
        assert _same_bits(eng.momentum_buffer[begin:end], wb), ("momentum buffer", i)
        assert _same_bits(eng.flat.flat[end:], p0[end:]) and _same_bits(eng.momentum_buffer[end:], b0[end:]), i
        assert not np.isnan(wp).any()
    assert eng.t == n_steps and eng.m is None and eng.v is None and eng.t_dev is None


def test_trainstep_sgd_is_the_restatement(gpu_device):
    """Covers the two-slice overlapped update (plan.Plan.adam_early) of the launch-program path."""
    import test_gpu_engine as E
    video, audio, ids = E._data(gpu_device, steps=3)
    m, crit, eng = _trainstep(gpu_device, lr=1e-3, optimizer="sgd", **SGD)
    assert eng.momentum_buffer.shape == eng.flat.flat.shape
    _check_steps(eng, lambda i: eng.step(video, audio, ids[i]), 3, 1e-3)
    assert eng._step_plan is not None, "the step did not run through a launch program"
    print(f"\n[sgd trainstep] two-slice overlapped update from element {eng._step_plan.adam_early} of {eng.flat.numel}")
    sd = eng.state_dict()
    assert len(sd["state"]) == len(list(m.parameters())) and sd["avid_sampler"]["offset"] == 3
    assert set(sd["param_groups"][0]) == set(torch.optim.SGD([torch.zeros(1)], lr=1.0).state_dict()["param_groups"][0])


def _finetune_inputs(dev, steps, seed=3):
    g = torch.Generator().manual_seed(seed)
    vids = [torch.randn((4, 3, 8, 112, 112), generator=g).to(dev) for _ in range(steps)]
    labs = [torch.randint(0, 101, (4,), generator=g).to(dev) for _ in range(steps)]
    return vids, labs


def test_finetunestep_sgd_is_the_restatement(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    vids, labs = _finetune_inputs(gpu_device, 3)
    eng = parallel.FinetuneStep(FT._wrapper(gpu_device), lr=1e-3, optimizer="sgd", **SGD)
    _check_steps(eng, lambda i: eng.step(vids[i], labs[i]), 3, 1e-3)


def test_finetunestep_classifier_only_under_sgd(gpu_device):
    import test_gpu_finetune as FT
    from avid_hip import parallel
    vids, labs = _finetune_inputs(gpu_device, 3)
    m = FT._wrapper(gpu_device)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    eng = parallel.FinetuneStep(m, lr=1e-3, classifier_only=True, optimizer="sgd", **SGD)
    _check_steps(eng, lambda i: eng.step(vids[i], labs[i]), 3, 1e-3, 0, eng.n_cls)
    for n, p in m.named_parameters():
        assert _same_bits(p, before[n]) == n.startswith("feature_extractor."), n
    assert not eng.momentum_buffer[eng.n_cls:].any() and eng.momentum_buffer[:eng.n_cls].any()
    sd = eng.state_dict()
    assert sorted(sd["state"]) == [0, 1] and sd["param_groups"][0]["params"] == [0, 1]
    assert sd["state"][0]["momentum_buffer"].shape == m.classifier.weight.shape


def test_probestep_sgd_is_the_restatement(gpu_device):
    import test_gpu_probe as PR
    from avid_hip import parallel
    dev = gpu_device
    g = torch.Generator().manual_seed(9)
    vids = [torch.randn((2, 3, 8, 64, 64), generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, 400, (2,), generator=g).to(dev) for _ in range(3)]
    m = PR._model(dev)
    eng = parallel.ProbeStep(m, lr=1e-3, optimizer="sgd", **SGD)
    _check_steps(eng, lambda i: eng.step(vids[i], labs[i]), 3, 1e-3)
    sd = eng.state_dict()
    n_all, n_tower = len(list(m.parameters())), len(list(m.feature_extractor.parameters()))
    assert sd["param_groups"][0]["params"] == list(range(n_all)) and sorted(sd["state"]) == list(range(n_tower, n_all))


def test_learning_rate_reaches_a_captured_sgd_graph(gpu_device):
    """The SGD twin of tests/test_gpu_engine.py::test_learning_rate_reaches_a_captured_graph, against an eager twin engine."""
    import test_gpu_engine as E
    dev = gpu_device
    video, audio, ids = E._data(dev)
    m, c, e = _trainstep(dev, lr=1e-3, optimizer="sgd", **SGD)
    m2, c2, twin = _trainstep(dev, lr=1e-3, optimizer="sgd", **SGD)
    for i in range(2):
        e.step(video, audio, ids[i])
        twin.step(video, audio, ids[i])
    e.capture(video, audio, ids[2])
    assert e.t == 2 and c.nce_average.multinomial.offset == 2              # the capture ran nothing
    torch.cuda.synchronize()
    assert _same_bits(e.flat.flat, twin.flat.flat) and _same_bits(e.momentum_buffer, twin.momentum_buffer)
    e.replay(index=ids[2])
    twin.step(video, audio, ids[2])
    before = e.flat.flat.clone()
    for lr, i in ((0.0, 3), (3e-3, 4)):
        e.set_lr(lr)                                       # a scheduler's write: by-value arguments are frozen in the graph
        twin.set_lr(lr)
        e.replay(index=ids[i])
        twin.step(video, audio, ids[i])
        torch.cuda.synchronize()
        assert _same_bits(e.flat.flat, before) == (lr == 0.0), lr
        assert _same_bits(e.flat.flat, twin.flat.flat) and _same_bits(e.momentum_buffer, twin.momentum_buffer), lr
    assert e.t == 5 and int(c.nce_average.multinomial.offset_dev) == 5


# ------------------------------------------------------------------------------------------------------------- checkpoints
def _torch_step_on(params, opt, eng):
    """One torch.optim.SGD step on the gradients the engine's last step produced (through FlatParams' own layout)."""
    for k, i, _ in eng._param_order():
        params[k].grad = eng.flat.view(eng.flat.grad, i).detach().clone()
    opt.step()


def _twin(m, dev):
    """A second model with ``m``'s parameters and buffers (a stepped model carries launch programs: not for deepcopy)."""
    import test_gpu_finetune as FT
    twin = FT._wrapper(dev, seed=1)
    twin.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    return twin


def test_checkpoints_interchange_with_torch_sgd(gpu_device):
    """The engine's state dict after two steps loads into torch.optim.SGD over a copy of its parameters and torch's loads into
    a fresh engine; after one further step on identical gradients both agree to tests/test_gpu_finetune.py::_off_bar's bars
    (rtol 1e-4 / atol 1e-6, every element): what is left is torch's fused arithmetic."""
    import test_gpu_finetune as FT
    from avid_hip import parallel
    dev = gpu_device
    vids, labs = _finetune_inputs(dev, 4, seed=11)
    m = FT._wrapper(dev)
    eng = parallel.FinetuneStep(m, lr=1e-3, optimizer="sgd", **SGD)
    for i in range(2):
        eng.step(vids[i], labs[i])
    torch.cuda.synchronize()
    # engine -> torch
    sd = copy.deepcopy(eng.state_dict())
    assert len(sd["state"]) == len(list(m.parameters()))
    m_t = _twin(m, dev)
    params = list(m_t.parameters())
    opt = torch.optim.SGD(params, lr=1.0)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"], g["dampening"]) == (1e-3, 0.9, 1e-4, True, 0)
    for k, i, p in eng._param_order():
        assert torch.equal(opt.state[params[k]]["momentum_buffer"], eng._slice(eng.momentum_buffer, i))
    eng.step(vids[2], labs[2])
    torch.cuda.synchronize()
    _torch_step_on(params, opt, eng)
    assert not FT._off_bar(m, m_t)
    # torch -> engine: a fresh engine over a copy of torch's parameters, torch's state dict
    m_e = _twin(m_t, dev)
    eng2 = parallel.FinetuneStep(m_e, lr=1.0, optimizer="sgd", momentum=0.5)
    eng2.load_state_dict(opt.state_dict())
    assert (eng2.lr, eng2.momentum, eng2.wd, eng2.nesterov, eng2.t) == (1e-3, 0.9, 1e-4, True, 1)
    for k, i, p in eng2._param_order():
        assert torch.equal(opt.state[params[k]]["momentum_buffer"], eng2._slice(eng2.momentum_buffer, i))
    eng2.step(vids[3], labs[3])
    torch.cuda.synchronize()
    _torch_step_on(params, opt, eng2)
    assert not FT._off_bar(m_e, m_t)
    with pytest.raises(ValueError, match=r"torch\.optim\.SGD.*torch\.optim\.Adam"):
        eng2.load_state_dict(parallel.FinetuneStep(_twin(m_t, dev)).state_dict())


# ------------------------------------------------------------------------------------------------------------ drop-in loop
def test_reference_loop_with_dropin_sgd_is_the_engine_bit_for_bit(gpu_device):
    """main-avid.py:169-178 with DistributedDataParallel(model) + parallel.SGD: zero_grad / backward / step, two steps — the
    parameters are the bits TrainStep(optimizer="sgd") reaches from the same start."""
    import test_gpu_engine as E
    import test_gpu_plan as GP
    from avid_hip import parallel
    dev, steps = gpu_device, 2
    video, audio, ids = E._data(dev, steps=steps)
    m_eng, _, eng = _trainstep(dev, lr=1e-3, optimizer="sgd", **SGD)
    for i in range(steps):
        eng.step(video, audio, ids[i])
    torch.cuda.synchronize()
    m, crit = E._model(dev), GP._crit(dev)
    net = parallel.DistributedDataParallel(m, device_ids=[dev.index])
    opt = parallel.SGD(net.parameters(), lr=1e-3, **SGD)
    assert opt.flat is net._engine.flat, "the optimizer did not adopt the wrapper's flat buffers"
    assert opt.state_dict()["state"] == {}
    for i in range(steps):
        v, a = net(video, audio)
        loss, _ = crit(v, a, ids[i])
        loss.item()
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    assert [p for p in m.__dict__.get("_avid_plans", {}).values() if p], "the loop did not run through a launch program"
    for (n, a), b in zip(m.named_parameters(), m_eng.parameters()):
        assert _same_bits(a, b), n
    assert _same_bits(opt.buf, eng.momentum_buffer)
    got, want = opt.state_dict(), eng.state_dict()
    assert sorted(got["state"]) == sorted(want["state"]) and got["param_groups"] == want["param_groups"]
    for k, st in want["state"].items():
        view = opt.state[list(m.parameters())[k]]["momentum_buffer"]
        assert torch.equal(got["state"][k]["momentum_buffer"], st["momentum_buffer"])
        assert opt.buf.data_ptr() <= view.data_ptr() < opt.buf.data_ptr() + 4 * opt.buf.numel()
