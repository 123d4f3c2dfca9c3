"""SGD with momentum without a GPU: the numpy restatement the kernel is held to (tests/_sgd_ref.py) against torch.optim.SGD,
the drop-in optimizer's constructor / checkpoint behaviour on CPU parameters, the step engines' checkpoint format, and the
``utils.main_utils`` hook."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _sgd_ref import sgd_steps

CONFIGS = [(0.1, 0.9, 1e-4, False), (0.01, 0.9, 1e-5, True), (0.1, 0, 1e-4, False), (1e-3, 0.9, 0, True), (0.02, 0.5, 0, False)]


def _tiny_model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("lr,momentum,wd,nesterov", CONFIGS)
def test_restatement_is_torch_sgd(lr, momentum, wd, nesterov, seed):
    """The float32 restatement is no further from the float64 recurrence than 2x what torch.optim.SGD (foreach=False, whose CPU
    kernels fuse multiply-adds: not the same bits) is, floor 2^-23 max|p|.  Both sides do the same operations, hence 2 where
    tests/test_gpu_precision.py allows 3 against a float32 F.conv3d."""
    n, steps = 4099, 8
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [0.3 * torch.randn(n, generator=g) for _ in range(steps)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, weight_decay=wd, nesterov=nesterov, foreach=False)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
    ours, buf = sgd_steps(p0.numpy(), [gr.numpy() for gr in grads], lr, momentum, wd, nesterov)
    want, buf64 = sgd_steps(p0.numpy(), [gr.numpy() for gr in grads], lr, momentum, wd, nesterov, dtype=np.float64)
    assert ours.dtype == np.float32 and want.dtype == np.float64
    err_ours = np.abs(ours.astype(np.float64) - want).max()
    err_torch = np.abs(p.detach().numpy().astype(np.float64) - want).max()
    floor = 2.0 ** -23 * np.abs(want).max()
    print(f"\n[sgd restatement] lr {lr} momentum {momentum} wd {wd} nesterov {nesterov} seed {seed}: restatement {err_ours:.3e}, "
          f"torch {err_torch:.3e}, ratio {err_ours / max(err_torch, 1e-300):.2f}, floor {floor:.3e}")
    assert err_ours <= max(2 * err_torch, floor)
    if momentum:
        tb = opt.state[p]["momentum_buffer"].numpy().astype(np.float64)
        assert np.abs(buf.astype(np.float64) - buf64).max() <= max(2 * np.abs(tb - buf64).max(), 2.0 ** -23 * np.abs(buf64).max())
    else:
        assert buf is None and not opt.state[p]


def test_version():
    from avid_hip import lib
    assert lib.version() >= 162


def test_ops_sgd_flat_refuses_cpu_tensors():
    from avid_hip import ops, AvidHipError
    p, g, b = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    with pytest.raises(AvidHipError):
        ops.sgd_flat(p, g, b, 0.1, 0.9, 0.0)
    with pytest.raises(AvidHipError):
        ops.sgd_flat(p, g, None, 0.1, 0.0, 0.0)


@pytest.mark.parametrize("kw", [dict(lr=0.1), dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True),
                                dict(lr=0.1, momentum=0.5, foreach=False)])
def test_dropin_state_dict_before_any_step_is_torch_sgds(kw):
    from avid_hip import parallel
    m = _tiny_model()
    ref = torch.optim.SGD(copy.deepcopy(m).parameters(), **kw)
    opt = parallel.SGD(m.parameters(), **kw)
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.state_dict() == ref.state_dict()
    assert all(p.data_ptr() == opt.flat.flat.data_ptr() + 4 * o for p, o in zip(opt.flat.params, opt.flat.offsets))


def test_dropin_refusals():
    from avid_hip import parallel
    lin = torch.nn.Linear(4, 4)
    for kw in (dict(dampening=0.1, momentum=0.9), dict(maximize=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            parallel.SGD(torch.nn.Linear(4, 4).parameters(), lr=0.1, **kw)
    with pytest.raises(NotImplementedError, match="one parameter group"):
        parallel.SGD([{"params": [torch.nn.Parameter(torch.zeros(3))]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}], lr=0.1)
    with pytest.raises(ValueError):                                        # torch's own rule
        parallel.SGD(torch.nn.Linear(4, 4).parameters(), lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        torch.optim.SGD(torch.nn.Linear(4, 4).parameters(), lr=0.1, nesterov=True)
    # a list that shares parameters with a live flat buffer without being exactly its set
    flat = parallel.FlatParams(lin)
    assert parallel.SGD(lin.parameters(), lr=0.1).flat is flat
    with pytest.raises(ValueError, match="not exactly that buffer's parameter set"):
        parallel.SGD([lin.weight], lr=0.1)
    with pytest.raises(ValueError, match="not exactly that buffer's parameter set"):
        parallel.SGD(list(lin.parameters()) + [torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    # step() on CPU parameters is an error of the library, not a quiet torch step
    from avid_hip import AvidHipError
    opt = parallel.SGD(torch.nn.Linear(4, 4).parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(AvidHipError):
        opt.step()


def _stepped_torch_sgd(m, **kw):
    opt = torch.optim.SGD(m.parameters(), **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        for p in m.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_dropin_loads_a_torch_sgd_checkpoint_and_gives_it_back():
    from avid_hip import parallel
    m = _tiny_model()
    ref = _stepped_torch_sgd(m, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    sd = copy.deepcopy(ref.state_dict())
    m2 = copy.deepcopy(m)
    opt = parallel.SGD(m2.parameters(), lr=1.0)
    assert opt.state_dict()["state"] == {}
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.1, 0.9, 1e-4, True)
    for k, p in enumerate(m2.parameters()):
        view = opt.state[p]["momentum_buffer"]
        assert torch.equal(view, sd["state"][k]["momentum_buffer"]) and view.shape == p.shape
        lo, hi = opt.buf.data_ptr(), opt.buf.data_ptr() + 4 * opt.buf.numel()
        assert lo <= view.data_ptr() < hi                                  # a view of the flat buffer, not a copy
    back = opt.state_dict()
    assert back["param_groups"] == sd["param_groups"] and sorted(back["state"]) == sorted(sd["state"])
    for k in sd["state"]:
        assert torch.equal(back["state"][k]["momentum_buffer"], sd["state"][k]["momentum_buffer"])
    torch.optim.SGD(copy.deepcopy(m).parameters(), lr=1.0).load_state_dict(back)      # torch takes it back


def test_adam_format_into_sgd_raises_naming_both_formats():
    from avid_hip import parallel
    m = _tiny_model()
    adam = torch.optim.Adam(m.parameters(), lr=1e-3)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    adam.step()
    adam_sd = adam.state_dict()
    sgd_sd = _stepped_torch_sgd(copy.deepcopy(m), lr=0.1, momentum=0.9).state_dict()
    opt = parallel.SGD(copy.deepcopy(m).parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match=r"torch\.optim\.SGD.*torch\.optim\.Adam"):
        opt.load_state_dict(adam_sd)
    for cls, kw in ((parallel.TrainStep, dict(criterion=None)), (parallel.FinetuneStep, {})):
        eng = cls(copy.deepcopy(m), optimizer="sgd", momentum=0.9, **kw)
        with pytest.raises(ValueError, match=r"torch\.optim\.SGD.*torch\.optim\.Adam"):
            eng.load_state_dict(adam_sd)
        eng = cls(copy.deepcopy(m), **kw)
        with pytest.raises(ValueError, match=r"torch\.optim\.Adam.*torch\.optim\.SGD"):
            eng.load_state_dict(sgd_sd)
        eng.load_state_dict(adam_sd)                                       # its own format still loads


def test_engine_sgd_state_dict_is_torch_sgds():
    """Numbering counts frozen parameters (they have an index and no state), the group carries the keys the installed
    torch.optim.SGD writes, the state is empty before the first step and without momentum, and both directions load."""
    from avid_hip.parallel import TrainStep
    m = _tiny_model()
    m[2].weight.requires_grad_(False)                                      # index 2 of 6 is frozen
    eng = TrainStep(m, criterion=None, lr=0.05, weight_decay=1e-4, optimizer="sgd", momentum=0.9, nesterov=True)
    assert eng.m is None and eng.v is None and eng.t_dev is None and eng.t == 0
    assert eng.momentum_buffer.shape == eng.flat.flat.shape and not eng.momentum_buffer.any()
    ref = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    assert eng.state_dict() == ref.state_dict()                            # before the first step: no state
    g = torch.Generator().manual_seed(2)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g) if p.requires_grad else None
    ref.step()
    rsd = ref.state_dict()
    assert sorted(rsd["state"]) == [0, 1, 3, 4, 5]
    eng.load_state_dict(rsd)
    assert eng.t == 1
    slot = {id(p): j for j, p in enumerate(eng.flat.params)}
    params = list(m.parameters())
    for k, st in rsd["state"].items():
        assert torch.equal(eng._slice(eng.momentum_buffer, slot[id(params[k])]), st["momentum_buffer"])
    sd = eng.state_dict()
    assert sd["param_groups"] == rsd["param_groups"] and sorted(sd["state"]) == sorted(rsd["state"])
    for k, st in rsd["state"].items():
        assert torch.equal(sd["state"][k]["momentum_buffer"], st["momentum_buffer"]) and list(sd["state"][k]) == ["momentum_buffer"]
    torch.optim.SGD(m.parameters(), lr=1.0).load_state_dict(sd)
    # without momentum: no buffer at all, no state
    plain = TrainStep(_tiny_model(), criterion=None, optimizer="sgd")
    assert plain.momentum_buffer is None
    plain.t = 3
    assert plain.state_dict()["state"] == {}
    # the default engine is what it was
    adam = TrainStep(_tiny_model(), criterion=None)
    assert adam.optimizer == "adam" and adam.momentum_buffer is None and adam.m.shape == adam.v.shape == adam.flat.flat.shape
    assert set(adam.state_dict()["param_groups"][0]) >= {"betas", "eps", "amsgrad"}
    with pytest.raises(ValueError):
        TrainStep(_tiny_model(), criterion=None, optimizer="sgd", nesterov=True)
    with pytest.raises(ValueError):
        TrainStep(_tiny_model(), criterion=None, optimizer="rmsprop")


def test_classifier_only_numbering_under_sgd():
    """FinetuneStep(classifier_only=True) numbers the warm-up optimizer's parameters (the classifier's) only, under SGD too."""
    from avid_hip import parallel

    class Wrapped(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.feature_extractor = torch.nn.Linear(6, 6)
            self.classifier = torch.nn.Linear(6, 3)
    m = Wrapped()
    eng = parallel.FinetuneStep(m, classifier_only=True, optimizer="sgd", momentum=0.9)
    eng.t = 1
    eng.momentum_buffer.copy_(torch.arange(eng.flat.numel, dtype=torch.float32))
    sd = eng.state_dict()
    assert sorted(sd["state"]) == [0, 1] and sd["param_groups"][0]["params"] == [0, 1]
    assert sd["state"][0]["momentum_buffer"].shape == m.classifier.weight.shape
    assert sd["state"][1]["momentum_buffer"].shape == m.classifier.bias.shape
    assert eng.n_cls == eng.flat.offsets[2]


def test_hook_forwards_sgd_for_a_flat_buffer_set(tmp_path):
    """avid-cma_amd/utils/main_utils.py with AVID_DROPIN_SGD=1: the reference's ``torch.optim.SGD(params=..., lr=..., momentum=...,
    weight_decay=..., nesterov=...)`` call site (a stand-in with its shape, written here) builds this package's SGD exactly for a
    live flat-buffer set, torch's own for a bare list, for dampening, under AVID_DROPIN=0 and without the opt-in."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref = str(tmp_path / "ref")
    os.makedirs(os.path.join(ref, "utils"))
    open(os.path.join(ref, "utils", "__init__.py"), "w").close()
    with open(os.path.join(ref, "utils", "main_utils.py"), "w") as f:
        f.write("import torch\n\n"
                "def build_optimizer(params, cfg, logger=None):\n"
                "    extra = {'dampening': cfg['dampening']} if 'dampening' in cfg else {}\n"
                "    o = torch.optim.SGD(params=params, lr=cfg['lr']['base_lr'], momentum=cfg['momentum'],\n"
                "                        weight_decay=cfg['weight_decay'], nesterov=cfg['nesterov'], **extra)\n"
                "    return o, torch.optim.lr_scheduler.MultiStepLR(o, milestones=cfg['lr']['milestones'], gamma=cfg['lr']['gamma'])\n")
    code = r'''
import sys, torch
import utils.main_utils as mu
from avid_hip import parallel
on = sys.argv[1] == "1"
assert (mu.torch.optim.SGD is not torch.optim.SGD) == on and mu.torch.optim.RMSprop is torch.optim.RMSprop
cfg = {"name": "sgd", "lr": {"base_lr": 0.05, "milestones": [1], "gamma": 0.1}, "momentum": 0.9, "weight_decay": 1e-4, "nesterov": True}
lin = torch.nn.Linear(8, 4)
opt, sched = mu.build_optimizer(lin.parameters(), cfg)                       # a bare model's parameters: torch's own either way
assert type(opt) is torch.optim.SGD and isinstance(sched, torch.optim.lr_scheduler.MultiStepLR)
assert type(mu.build_optimizer([lin.weight], cfg)[0]) is torch.optim.SGD
net = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))
flat = parallel.FlatParams(net)
opt, sched = mu.build_optimizer(list(net.parameters()), cfg)                 # a live flat-buffer set
assert (type(opt) is parallel.SGD and opt.flat is flat) if on else type(opt) is torch.optim.SGD
g = opt.param_groups[0]
assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (0.05, 0.9, 1e-4, True)
assert type(mu.build_optimizer([net[0].weight], cfg)[0]) is torch.optim.SGD  # a subset of it: torch's, nothing re-seated
damp = dict(cfg, dampening=0.1, nesterov=False)
assert type(mu.build_optimizer(list(net.parameters()), damp)[0]) is torch.optim.SGD
assert all(p.data_ptr() == flat.flat.data_ptr() + 4 * o for p, o in zip(flat.params, flat.offsets))
print("OK")
'''
    for dropin, sgd, on in (("1", "1", "1"), ("0", "1", "0"), ("1", None, "0")):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(repo, "avid-cma_amd"), ref]), AVID_DROPIN=dropin)
        env.pop("AVID_DROPIN_SGD", None)
        if sgd is not None:
            env["AVID_DROPIN_SGD"] = sgd
        out = subprocess.run([sys.executable, "-c", code, on], capture_output=True, text=True, env=env, cwd=str(tmp_path))
        assert out.returncode == 0 and "OK" in out.stdout, (dropin, sgd, out.stderr[-1500:])
