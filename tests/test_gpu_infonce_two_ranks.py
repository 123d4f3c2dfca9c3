"""criterions.InfoNCE and TrainStep under it with TWO ranks on the one GPU of the box (two processes on ``cuda:0`` over gloo,
spawned as fresh children like tests/test_gpu_two_ranks.py): every rank gathers both modalities' embeddings in one packed
record, reports the loss of the GLOBAL batch and back-propagates world x the exact gradient of that loss for its own rows —
the rows of a single-process call on the concatenated embeddings, bit for bit — so that the engines' 1 / world average
leaves the gradient of the global loss and the replicas stay identical."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, D, TAU = 19, 128, 0.07           # per-rank batch: the global 38 rows sit in one key tile, the blocks start off a tile edge


def _embeddings():
    rng = np.random.RandomState(21)
    e1 = (rng.randn(2 * B, D) * 1.3).astype(np.float32)
    e2 = (0.7 * e1 + 0.7 * rng.randn(2 * B, D) * 1.3).astype(np.float32)
    return torch.from_numpy(e1), torch.from_numpy(e2)


def _criterion_job(rank, world, out):
    import criterions
    dev = torch.device("cuda", 0)
    e1, e2 = _embeddings()
    t1 = e1[rank * B:(rank + 1) * B].to(dev).requires_grad_(True)
    t2 = e2[rank * B:(rank + 1) * B].to(dev).requires_grad_(True)
    crit = criterions.InfoNCE(D, device=0, temperature=TAU, v2a_coeff=1.0, a2v_coeff=3.0)
    loss, log = crit(t1, t2, torch.arange(B, device=dev))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": float(loss.detach()), "log": {k: float(x) for k, x in log.items()}, "g1": t1.grad.cpu(), "g2": t2.grad.cpu()}


def _train_job(rank, world, out):
    import criterions
    import test_gpu_two_ranks as T2
    from avid_hip import ops
    from avid_hip.parallel import TrainStep
    dev = torch.device("cuda", 0)
    m = T2._model(dev)
    if rank == 1:                                    # ranks start DIFFERENT: the construction broadcast must fix it
        with torch.no_grad():
            m.video_model.conv1[0].weight.add_(1.0)
    eng = TrainStep(m, criterions.InfoNCE(128, device=0, temperature=TAU), bucket_bytes=4 << 20)
    video, audio = T2._inputs()
    v = video[rank * T2.BS:(rank + 1) * T2.BS].to(dev)
    a = audio[rank * T2.BS:(rank + 1) * T2.BS].to(dev)
    ids = torch.arange(rank * T2.BS, (rank + 1) * T2.BS, device=dev)
    res = {"loss": [], "params": []}
    for _ in range(2):
        res["loss"].append(float(eng.step(v, a, ids)))
        res["params"].append(eng.flat.flat.clone().cpu())
    ops.check_device_errors(dev)
    return res


_JOBS = {"criterion": _criterion_job, "train": _train_job}


def _worker(rank, world, port, out, job):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _JOBS[job](rank, world, out)
        torch.save(res, os.path.join(out, f"{job}_{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _run2(job, out, timeout=600):
    import torch.multiprocessing as mp
    import test_gpu_two_ranks as T2
    ctx = mp.get_context("spawn")
    port = T2._free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(out), job)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(timeout) for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [torch.load(os.path.join(str(out), f"{job}_{r}.pt"), weights_only=False) for r in range(2)]


def test_two_rank_criterion_is_the_global_loss(tmp_path, gpu_device):
    import criterions
    r = _run2("criterion", tmp_path)
    e1, e2 = _embeddings()
    t1, t2 = e1.to(gpu_device).requires_grad_(True), e2.to(gpu_device).requires_grad_(True)
    crit = criterions.InfoNCE(D, device=0, temperature=TAU, v2a_coeff=1.0, a2v_coeff=3.0)
    loss, log = crit(t1, t2, torch.arange(2 * B, device=gpu_device))
    loss.backward()
    assert r[0]["loss"] == r[1]["loss"] == float(loss.detach()) and np.isfinite(r[0]["loss"])
    assert r[0]["log"] == r[1]["log"] == {k: float(x) for k, x in log.items()}
    for rank in range(2):
        rows = slice(rank * B, (rank + 1) * B)
        # world x the global gradient (the power of two is exact): the 1 / world of the gradient average leaves it
        for got, want in ((r[rank]["g1"], t1.grad[rows]), (r[rank]["g2"], t2.grad[rows])):
            assert torch.equal(got.view(torch.int32), (2.0 * want).cpu().view(torch.int32)), rank
    assert float(t1.grad.abs().max()) > 0


def test_two_rank_trainstep_keeps_the_replicas_identical(tmp_path, gpu_device):
    r = _run2("train", tmp_path)
    assert r[0]["loss"] == r[1]["loss"] and all(np.isfinite(l) for l in r[0]["loss"])
    for step in range(2):
        assert torch.equal(r[0]["params"][step].view(torch.int32), r[1]["params"][step].view(torch.int32)), step
    assert not torch.equal(r[0]["params"][0], r[0]["params"][1])
