"""``FinetuneStep`` / ``ProbeStep(virtual_ranks=R)``: the step of an R-replica job on one MI355X, shard after shard.

Fine-tuning at the shapes of tests/test_gpu_finetune_two_ranks.py (R(2+1)D-18 + dropout 0.5 + Linear(512, 101), clips
3 x 8 x 64 x 64, b = 2 per replica), the probe at those of tests/test_gpu_probe.py's engine test (the shipped heads, b = 4).
Everything is compared BIT FOR BIT (``torch.equal``) with one-rank engines that run one shard each from the same state —
which tests/test_gpu_finetune.py and tests/test_gpu_probe.py hold to float64 and to the per-layer path — and, for R = 2, with the
real two-process job.  The combination rule itself is held to ``nn.DataParallel`` in float64 by
tests/test_virtual_downstream_host.py.  The one tolerance is the step guard's norm (tests/_guard_ref.py ``norm_bound``)."""
import copy
import math
import os

import pytest
import torch

import _guard_ref as GR
import test_gpu_finetune_two_ranks as FT
import test_gpu_probe as PR

pytestmark = pytest.mark.gpu

B_RANK, SHAPE = FT.B_RANK, FT.SHAPE
STRIDE, U64 = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF
BASE_SEED = 4242


def _seeds(R, base=BASE_SEED):
    return [(base + STRIDE * r) & U64 for r in range(R)]


def _ft_data(R, dev, steps=2, seed=21):
    g = torch.Generator().manual_seed(seed)
    video = [torch.randn((R * B_RANK,) + SHAPE, generator=g).to(dev) for _ in range(steps)]
    labels = [torch.randint(0, 101, (R * B_RANK,), generator=g).to(dev) for _ in range(steps)]
    return video, labels


def _buffers(m):
    return {n: b.detach().clone() for n, b in m.named_buffers()}


def _nbt(m):
    return [int(b) for n, b in m.named_buffers() if n.endswith("num_batches_tracked")]


def _sh(t, r, b):
    return t[r * b:(r + 1) * b]


def _rank_sum(grads):
    """((g0 + g1) + g2) + ... with float32 adds, left to right."""
    acc = grads[0].clone()
    for g in grads[1:]:
        acc = acc + g
    return acc


class Shard:
    """A one-rank engine (no virtual ranks, no process group) that runs ONE replica's shard from a given state."""

    def __init__(self, dev, kind="finetune", **kw):
        from avid_hip import parallel
        self.kind = kind
        if kind == "finetune":
            self.m = FT._model(dev)
            self.eng = parallel.FinetuneStep(self.m, **kw)
        else:
            self.m = PR._model(dev)
            self.eng = parallel.ProbeStep(self.m, **kw)

    def run(self, params, bufs, v, y, seed=None, offset=0):
        """One step on (v, y) from ``params`` (the flat parameter buffer) and ``bufs`` (every buffer by name), dropout at
        (seed, offset): the loss, the hits, the gradient buffer and every buffer as the step leaves them."""
        with torch.no_grad():
            self.eng.flat.flat.copy_(params)
            for n, b in self.m.named_buffers():
                b.copy_(bufs[n])
        if seed is not None:
            self.m.dropout.seed, self.m.dropout.offset = seed, offset
        loss, hits = self.eng.step(v.contiguous(), y.contiguous())
        return {"loss": loss.clone(), "hits": hits.clone(), "grad": self.eng.flat.grad.clone(), "buf": _buffers(self.m)}


def _adam(eng, params, grad, m, v, step_dev, t, n, R):
    from avid_hip import ops
    ops.adam_flat(params[:n], grad[:n], m[:n], v[:n], eng.lr, eng.betas[0], eng.betas[1], eng.eps, eng.wd, t, grad_scale=1.0 / R,
                  step_dev=step_dev)


def _check_against_shards(eng, model, shard, video, labels, R, b, n, seeds=None, steps=2):
    """``steps`` steps of the virtual engine ``eng`` on the global batches against ``shard`` runs of every replica's rows from
    the state the step started in: elements [0, n) of the flat buffers are trained, the rest is not touched."""
    dev = video[0].device
    params, bufs = eng.flat.flat.clone(), _buffers(model)
    params0 = params.clone()
    am, av = torch.zeros_like(params), torch.zeros_like(params)
    step_dev = torch.zeros((), dtype=torch.int64, device=dev)
    for step in range(steps):
        singles = [shard.run(params, bufs, _sh(video[step], r, b), _sh(labels[step], r, b), None if seeds is None else seeds[r], step)
                   for r in range(R)]
        grad_before = eng.flat.grad.clone()
        loss, hits = eng.step(video[step], labels[step])
        assert eng.rank_losses.dtype == torch.float32 and eng.rank_hits.dtype == torch.int64 and eng.rank_losses.is_cuda
        assert eng.rank_losses.shape[0] == R and eng.rank_hits.shape == eng.rank_losses.shape + (2,)
        for r in range(R):
            assert torch.equal(eng.rank_losses[r], singles[r]["loss"]), (step, r)
            assert torch.equal(eng.rank_hits[r], singles[r]["hits"]), (step, r)
        assert torch.equal(loss, eng.rank_losses.mean(0)) and torch.equal(hits, eng.rank_hits.sum(0))
        assert loss.shape == singles[0]["loss"].shape and hits.shape == singles[0]["hits"].shape
        gsum = _rank_sum([s["grad"] for s in singles])
        assert torch.equal(eng.flat.grad[:n], gsum[:n]), step
        assert torch.equal(eng.flat.grad[n:], grad_before[n:])          # (classifier_only: the tower's slice is never written)
        if R == 3:      # the order is visible: another association of the three is other bits somewhere
            other = singles[0]["grad"] + (singles[1]["grad"] + singles[2]["grad"])
            assert not torch.equal(other[:n], gsum[:n])
        for name, buf in model.named_buffers():
            assert torch.equal(buf, singles[0]["buf"][name]), (step, name)
        assert set(_nbt(model)) == {step + 1}
        want = params.clone()
        _adam(eng, want, gsum, am, av, step_dev, step + 1, n, R)
        assert torch.equal(eng.flat.flat, want), step
        assert torch.equal(want[n:], params0[n:]) and not torch.equal(want[:n], params[:n])
        assert eng.t == step + 1 and int(eng.t_dev) == step + 1
        params, bufs = want, singles[0]["buf"]
    return params


# ------------------------------------------------------------------------------------------------------- 1. fine-tuning against shard runs
@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
@pytest.mark.parametrize("R", [2, 3])
def test_virtual_finetune_step_against_single_shard_engines(gpu_device, R, classifier_only):
    from avid_hip import ops, parallel
    dev = gpu_device
    video, labels = _ft_data(R, dev)
    m = FT._model(dev)
    m.dropout.seed = BASE_SEED
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, virtual_ranks=R)
    assert eng.rank_losses is None and eng.rank_hits is None and eng.dropout_seeds == _seeds(R)
    shard = Shard(dev, classifier_only=classifier_only)
    n = eng.n_cls if classifier_only else eng.flat.numel
    assert 0 < eng.n_cls < eng.flat.numel
    tower0 = eng.flat.flat[eng.n_cls:].clone()
    _check_against_shards(eng, m, shard, video, labels, R, B_RANK, n, seeds=_seeds(R))
    assert m.dropout.offset == 2                                       # one offset per step, whatever R
    assert torch.equal(eng.flat.flat[eng.n_cls:], tower0) == classifier_only
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------- 2. R = 2 is the two-process job
def _job(rank, world, out):
    from avid_hip import ops, parallel
    dev = torch.device("cuda", 0)
    m = FT._model(dev)
    m.dropout.seed = _seeds(2)[rank]
    eng = parallel.FinetuneStep(m, bucket_bytes=4 << 20)
    video, labels = _ft_data(2, dev)
    res = {}
    for step in range(2):
        eng.step(_sh(video[step], rank, B_RANK).contiguous(), _sh(labels[step], rank, B_RANK).contiguous())
        torch.cuda.synchronize()
        if step == 0:
            res["grad0"] = eng.flat.grad.clone().cpu()
    res["params_final"] = eng.flat.flat.clone().cpu()
    res["buf"] = {n: b.clone().cpu() for n, b in m.named_buffers()}
    ops.check_device_errors(dev)
    return res


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_job(rank, world, out), os.path.join(out, f"vd_{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _run2(out, timeout=600):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = FT._free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(out))) for r in range(2)]
    [p.start() for p in procs]
    [p.join(timeout) for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [torch.load(os.path.join(str(out), f"vd_{r}.pt"), weights_only=False) for r in range(2)]


def test_two_virtual_ranks_are_the_two_process_job(tmp_path, gpu_device):
    from avid_hip import parallel
    r = _run2(tmp_path)
    dev = gpu_device
    m = FT._model(dev)
    eng = parallel.FinetuneStep(m, virtual_ranks=2)
    eng.reseed_dropout(_seeds(2))
    video, labels = _ft_data(2, dev)
    for step in range(2):
        eng.step(video[step], labels[step])
        if step == 0:
            assert torch.equal(eng.flat.grad.cpu(), r[0]["grad0"]) and torch.equal(r[1]["grad0"], r[0]["grad0"])
    assert torch.equal(eng.flat.flat.cpu(), r[0]["params_final"]) and torch.equal(r[1]["params_final"], r[0]["params_final"])
    for n, b in m.named_buffers():
        assert torch.equal(b.cpu(), r[0]["buf"][n]), n
    assert not torch.equal(r[1]["buf"]["feature_extractor.conv1.1.running_mean"], r[0]["buf"]["feature_extractor.conv1.1.running_mean"])


# ------------------------------------------------------------------------------------------------------- 3. the probe
def test_virtual_probe_step_against_single_shard_engines(gpu_device):
    from avid_hip import ops, parallel
    dev, R, b = gpu_device, 2, 4
    g = torch.Generator().manual_seed(3)
    video = [torch.randn((R * b, 3, 8, 64, 64), generator=g).to(dev) for _ in range(2)]
    labels = [torch.randint(0, 400, (R * b,), generator=g).to(dev) for _ in range(2)]
    m = PR._model(dev)
    tower0 = {n: p.detach().clone() for n, p in m.feature_extractor.named_parameters()}
    eng = parallel.ProbeStep(m, virtual_ranks=R)
    assert eng.rank_losses is None and eng.n_taps == 4
    heads = sum((p.numel() + 3) // 4 * 4 for p in m.classifiers.parameters())
    assert eng.flat.numel == heads                                     # the flat buffers hold the classifiers only
    _check_against_shards(eng, m, Shard(dev, "probe"), video, labels, R, b, eng.flat.numel)
    assert tuple(eng.rank_losses.shape) == (R, 4) and tuple(eng.rank_hits.shape) == (R, 4, 2)
    names = [n for n, _ in m.named_buffers()]
    assert any(n.startswith("classifiers.") and n.endswith("running_var") for n in names)      # the heads' BatchNorm1d were compared
    assert any(n.startswith("feature_extractor.") and n.endswith("running_mean") for n in names)
    for n, p in m.feature_extractor.named_parameters():
        assert torch.equal(p, tower0[n]) and not p.requires_grad and p.grad is None, n
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------- 4. shards matter
def test_the_virtual_step_is_not_the_whole_batch_step(gpu_device):
    from avid_hip import parallel
    dev = gpu_device
    video, labels = _ft_data(2, dev, steps=1)
    res = []
    for kw in ({"virtual_ranks": 2}, {}):
        m = FT._model(dev)
        m.dropout.seed = BASE_SEED
        eng = parallel.FinetuneStep(m, **kw)
        eng.step(video[0], labels[0])
        res.append((eng.flat.grad.clone(), eng._grad_scale(), m.feature_extractor.conv1[1].running_mean.clone()))
    (gv, sv, rv), (g1, s1, r1) = res
    assert (sv, s1) == (0.5, 1.0)
    assert not torch.equal(gv * sv, g1) and not torch.equal(rv, r1)
    # not a matter of rounding: the per-shard statistics give another gradient (the classifier's slice leads the buffer)
    assert float((gv * sv - g1).abs().max()) > 1e-3 * float(g1.abs().max())


# ------------------------------------------------------------------------------------------------------- 5. the launch log
TABLE_KERNELS = ("weight_transpose_batched", "weight_transform", "wino_weight")


def test_launch_log_of_a_virtual_step(gpu_device, kernel_log):
    from avid_hip import ops, parallel
    dev, R = gpu_device, 3
    video, labels = _ft_data(R, dev)
    one = parallel.FinetuneStep(FT._model(dev))
    one.step(_sh(video[0], 0, B_RANK).contiguous(), _sh(labels[0], 0, B_RANK).contiguous())
    with kernel_log() as ref:
        one.step(_sh(video[1], 0, B_RANK).contiguous(), _sh(labels[1], 0, B_RANK).contiguous())
    eng = parallel.FinetuneStep(FT._model(dev), virtual_ranks=R)
    eng.step(video[0], labels[0])
    with kernel_log() as log:
        eng.step(video[1], labels[1])
    assert log.launches("grad_accum_flat") == R - 1 and ref.launches("grad_accum_flat") == 0
    assert log.launches("adam_flat") == 1 and ref.launches("adam_flat") == 1
    assert ref.launches("weight_transpose_batched") == 1
    for k in TABLE_KERNELS:                                   # the derived weight tables: once per step, not once per shard
        assert log.launches(k) == ref.launches(k), (k, log.launches(k), ref.launches(k))
    assert log.launches("cls_loss") == R * ref.launches("cls_loss") and ref.launches("cls_loss") == 1
    ops.check_device_errors(dev)


def test_virtual_step_with_sgd(gpu_device, kernel_log):
    from avid_hip import ops, parallel
    dev, R = gpu_device, 2
    video, labels = _ft_data(R, dev)
    m = FT._model(dev)
    m.dropout.seed = BASE_SEED
    eng = parallel.FinetuneStep(m, lr=1e-3, weight_decay=1e-4, optimizer="sgd", momentum=0.9, virtual_ranks=R)
    params, bufs = eng.flat.flat.clone(), _buffers(m)
    shard = Shard(dev)
    singles = [shard.run(params, bufs, _sh(video[0], r, B_RANK), _sh(labels[0], r, B_RANK), _seeds(R)[r], 0) for r in range(R)]
    eng.step(video[0], labels[0])
    gsum = _rank_sum([s["grad"] for s in singles])
    assert torch.equal(eng.flat.grad, gsum)
    want, buf = params.clone(), torch.zeros_like(params)
    ops.sgd_flat(want, gsum, buf, 1e-3, 0.9, 1e-4, False, grad_scale=1.0 / R)
    assert torch.equal(eng.flat.flat, want) and torch.equal(eng.momentum_buffer, buf) and eng.t == 1
    with kernel_log() as log:
        eng.step(video[1], labels[1])
    assert log.launches("sgd_flat") == 1 and log.launches("adam_flat") == 0 and log.launches("grad_accum_flat") == R - 1


# ------------------------------------------------------------------------------------------------------- 6. the step guard
def test_guard_clips_the_accumulated_gradient(gpu_device):
    from avid_hip import ops, parallel
    dev, R = gpu_device, 2
    video, labels = _ft_data(R, dev, steps=1)
    max_norm = 1e-3
    m = FT._model(dev)
    eng = parallel.FinetuneStep(m, max_grad_norm=max_norm, virtual_ranks=R)
    params = eng.flat.flat.clone()
    eng.step(video[0], labels[0])
    gsum = eng.flat.grad.clone()                                       # (the sum of the shards': test 1)
    ref = GR.guard_ref(gsum.cpu().numpy(), 1.0 / R, max_norm)
    got = float(eng.guard.grad_norm)
    bound = GR.norm_bound(gsum.numel())
    print(f"\n[virtual guard] n {gsum.numel()}: norm {got!r} (float64 {ref['norm']!r}) bound {bound:.3e}, coef "
          f"{float(eng.guard.clip_coef)!r} (float64 {ref['coef']!r})")
    assert ref["norm"] > 10 * max_norm and abs(got - ref["norm"]) <= bound * ref["norm"]
    assert int(eng.guard.skipped) == 0 and 0 < float(eng.guard.clip_coef) < 0.1
    guard = ops.StepGuard(dev)
    ops.grad_guard(gsum, guard, grad_scale=1.0 / R, max_norm=max_norm)
    assert float(guard.grad_norm) == got and float(guard.clip_coef) == float(eng.guard.clip_coef)
    am, av = torch.zeros_like(params), torch.zeros_like(params)
    step_dev = torch.zeros((), dtype=torch.int64, device=dev)
    ops.adam_flat_guarded(params, gsum, am, av, eng.lr, eng.betas[0], eng.betas[1], eng.eps, eng.wd, 1, guard, grad_scale=1.0 / R,
                          step_dev=step_dev)
    assert torch.equal(eng.flat.flat, params) and torch.equal(eng.m, am) and torch.equal(eng.v, av) and int(eng.t_dev) == 1


def _state(eng, m):
    return {"params": eng.flat.flat.clone(), "m": eng.m.clone(), "v": eng.v.clone(), "t": eng.t_dev.clone(),
            **{"buf." + n: b for n, b in _buffers(m).items()}}


@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
def test_guard_skips_a_step_with_a_nan_in_one_shard(gpu_device, classifier_only):
    """The NaN sits in shard 1's clip only.  In the full step it reaches the gradient; in the warm-up step the tower's ReLUs
    turn it into zero features and only shard 1's running statistics — which the step does not keep — give it away."""
    from avid_hip import parallel
    dev, R = gpu_device, 2
    video, labels = _ft_data(R, dev, steps=3)
    engines = []
    for _ in range(2):
        m = FT._model(dev)
        m.dropout.seed = BASE_SEED
        engines.append((parallel.FinetuneStep(m, classifier_only=classifier_only, skip_nonfinite=True, virtual_ranks=R), m))
    (eng, m), (twin, m2) = engines
    for e in (eng, twin):
        e.step(video[0], labels[0])
    assert int(eng.guard.skipped) == 0 and set(_nbt(m)) == {1}
    before = _state(eng, m)
    bad = video[1].clone()
    bad[B_RANK, 1, 3, 5, 7] = float("nan")                             # the first clip of shard 1
    eng.step(bad, labels[1])
    assert int(eng.guard.skipped) == 1 and int(eng.guard.skipped_total) == 1
    # which witness spoke: the gradient in the full step; in the warm-up step its norm is finite and the statistics did
    assert math.isfinite(float(eng.guard.grad_norm)) == classifier_only
    assert bool(torch.isfinite(eng.rank_losses[0])) and eng.t == 2 and int(eng.t_dev) == 1
    after = _state(eng, m)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert set(_nbt(m)) == {1}
    # the next clean step: the one an engine takes that never saw the bad batch, but for the dropout offset
    m2.dropout.offset = m.dropout.offset
    la, ha = eng.step(video[2], labels[2])
    lb, hb = twin.step(video[2], labels[2])
    assert int(eng.guard.skipped) == 0 and torch.equal(la, lb) and torch.equal(ha, hb) and bool(torch.isfinite(la))
    sa, sb = _state(eng, m), _state(twin, m2)
    for k, v in sa.items():
        assert torch.equal(v, sb[k]), k
    assert not torch.equal(sa["params"], before["params"]) and set(_nbt(m)) == {2}


# ------------------------------------------------------------------------------------------------------- 7. checkpoints
def test_checkpoint_between_virtual_steps_resumes_bit_for_bit(gpu_device):
    from avid_hip import parallel
    dev, R = gpu_device, 2
    video, labels = _ft_data(R, dev)
    m = FT._model(dev)
    m.dropout.seed = BASE_SEED
    eng = parallel.FinetuneStep(m, virtual_ranks=R)
    eng.step(video[0], labels[0])
    saved = copy.deepcopy({"opt": eng.state_dict(), "model": m.state_dict()})
    assert set(saved["opt"]) == {"state", "param_groups"}                # torch.optim.Adam's format: no virtual_ranks in it
    loss, hits = eng.step(video[1], labels[1])
    torch.manual_seed(1)
    m2 = FT._model(dev)
    m2.load_state_dict(saved["model"])
    m2.dropout.seed, m2.dropout.offset = BASE_SEED, 1
    eng2 = parallel.FinetuneStep(m2, virtual_ranks=R)
    eng2.load_state_dict(saved["opt"])
    assert eng2.t == 1 and int(eng2.t_dev) == 1
    loss2, hits2 = eng2.step(video[1], labels[1])
    assert torch.equal(loss2, loss) and torch.equal(hits2, hits) and torch.equal(eng2.rank_losses, eng.rank_losses)
    assert torch.equal(eng2.flat.flat, eng.flat.flat) and torch.equal(eng2.m, eng.m) and torch.equal(eng2.v, eng.v)
    for (n, a), b in zip(m2.named_buffers(), m.buffers()):
        assert torch.equal(a, b), n
    # a one-rank engine's checkpoint loads into a two-rank engine, and back
    one = parallel.FinetuneStep(FT._model(dev))
    one.step(_sh(video[0], 0, B_RANK).contiguous(), _sh(labels[0], 0, B_RANK).contiguous())
    sd1 = copy.deepcopy(one.state_dict())
    eng2.load_state_dict(sd1)
    assert eng2.virtual_ranks == R and torch.equal(eng2.m, one.m) and torch.equal(eng2.v, one.v) and int(eng2.t_dev) == 1
    back = eng2.state_dict()
    one.load_state_dict(back)
    assert one.virtual_ranks == 1 and sorted(back["state"]) == sorted(sd1["state"])
    for k, st in sd1["state"].items():
        assert torch.equal(back["state"][k]["exp_avg"], st["exp_avg"]) and torch.equal(back["state"][k]["exp_avg_sq"], st["exp_avg_sq"])
