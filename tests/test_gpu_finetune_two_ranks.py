"""FinetuneStep with TWO ranks on the one MI355X (backend gloo, two processes sharing cuda:0, as tests/test_gpu_two_ranks.py
does for the pretraining step), against single-process runs of the same programs on each rank's half of the batch.

* construction: both ranks start from rank 0's parameters and buffers;
* step 0: the all-reduced gradient buffer is bit-identical to g(shard 0) + g(shard 1) — the full step through GradBuckets, the
  classifier-only warm-up through one collective over the classifier's slice (the tower's slice is never written or
  reduced) — and the Adam step applies their mean;
* parameters stay bit-identical across ranks; each rank's BatchNorm running statistics after step 0 are the single-process
  statistics of its own shard; rank 0's are broadcast before every step (broadcast_buffers="step").
"""
import os
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

B_RANK = 2
SHAPE = (3, 8, 64, 64)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _model(dev):
    import models
    torch.manual_seed(0)
    m = models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5)
    return m.to(dev).train()


def _data(dev):
    g = torch.Generator().manual_seed(21)
    video = [torch.randn((2 * B_RANK,) + SHAPE, generator=g) for _ in range(2)]
    labels = [torch.randint(0, 101, (2 * B_RANK,), generator=g) for _ in range(2)]
    return video, labels


def _job(rank, world, out, classifier_only):
    from avid_hip import ops, parallel
    dev = torch.device("cuda", 0)
    m = _model(dev)
    if rank == 1:                                   # ranks start DIFFERENT: the construction broadcast must fix it
        with torch.no_grad():
            m.classifier.weight.add_(1.0)
            m.feature_extractor.conv1[1].running_mean.fill_(3.0)
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, bucket_bytes=4 << 20)
    res = {"params_init": eng.flat.flat.clone().cpu(), "rm_init": m.feature_extractor.conv1[1].running_mean.clone().cpu()}
    video, labels = _data(dev)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    res["loss"], res["rm"], res["rm_synced"] = [], [], []
    sync = eng.sync_buffers

    def recorded_sync():                            # what the step's own broadcast leaves in the buffers
        sync()
        res["rm_synced"].append(m.feature_extractor.conv1[1].running_mean.clone().cpu())
    eng.sync_buffers = recorded_sync
    for step in range(2):
        loss, _ = eng.step(video[step][sl].to(dev), labels[step][sl].to(dev))
        torch.cuda.synchronize()
        if step == 0:
            res["grad0"] = eng.flat.grad.clone().cpu()
            res["params0"] = eng.flat.flat.clone().cpu()
            res["buf0"] = {n: b.clone().cpu() for n, b in m.named_buffers()}
        res["loss"].append(float(loss))
        res["rm"].append(m.feature_extractor.conv1[1].running_mean.clone().cpu())
    res["params_final"] = eng.flat.flat.clone().cpu()
    res["n_cls"] = eng.n_cls
    ops.check_device_errors(dev)
    return res


def _worker(rank, world, port, out, classifier_only):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_job(rank, world, out, classifier_only), os.path.join(out, f"ft_{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _run2(out, classifier_only, timeout=600):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(out), classifier_only)) for r in range(2)]
    [p.start() for p in procs]
    [p.join(timeout) for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [torch.load(os.path.join(str(out), f"ft_{r}.pt"), weights_only=False) for r in range(2)]


def _single(dev, rank, classifier_only):
    """Step 0 of one rank's shard in ONE process: loss, gradient buffer, buffers after the forward, the engine."""
    from avid_hip import parallel
    m = _model(dev)
    eng = parallel.FinetuneStep(m, classifier_only=classifier_only, bucket_bytes=4 << 20)
    video, labels = _data(dev)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    flat0 = eng.flat.flat.clone()
    loss, _ = eng.step(video[0][sl].to(dev), labels[0][sl].to(dev))
    torch.cuda.synchronize()
    return {"loss": float(loss), "grad": eng.flat.grad.clone(), "flat0": flat0, "eng": eng,
            "buf": {n: b.clone().cpu() for n, b in m.named_buffers()}}


@pytest.mark.parametrize("classifier_only", [False, True], ids=["full", "classifier_only"])
def test_two_rank_finetune_matches_the_split_batch(tmp_path, gpu_device, classifier_only):
    from avid_hip import ops
    r = _run2(tmp_path, classifier_only)
    # construction: rank 0's state everywhere
    assert torch.equal(r[0]["params_init"], r[1]["params_init"]) and torch.equal(r[0]["rm_init"], r[1]["rm_init"])
    s = [_single(gpu_device, k, classifier_only) for k in range(2)]
    n_cls = r[0]["n_cls"]
    want = (s[0]["grad"] + s[1]["grad"]).cpu()
    for k in range(2):
        assert r[k]["loss"][0] == s[k]["loss"]                       # each rank's loss is its own shard's
        if classifier_only:
            # the classifier's slice reduced; the tower's slice neither written nor reduced
            assert torch.equal(r[k]["grad0"][:n_cls], want[:n_cls])
        else:
            assert torch.equal(r[k]["grad0"], want)
        # each rank's running statistics after step 0 are its own shard's (per-rank statistics, no SyncBN)
        for n, b in s[k]["buf"].items():
            assert torch.equal(r[k]["buf0"][n], b), (k, n)
    # the Adam step applies the MEAN of the two shards' gradients, over all parameters or the classifier's slice
    eng = s[0]["eng"]
    flat = s[0]["flat0"].clone()
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    g = want.to(gpu_device)
    n = n_cls if classifier_only else flat.numel()
    step_dev = torch.zeros((), dtype=torch.int64, device=gpu_device)
    ops.adam_flat(flat[:n], g[:n], m[:n], v[:n], eng.lr, eng.betas[0], eng.betas[1], eng.eps, eng.wd, 1, grad_scale=0.5,
                  step_dev=step_dev)
    torch.cuda.synchronize()
    assert torch.equal(r[0]["params0"], flat.cpu()) and torch.equal(r[1]["params0"], flat.cpu())
    if classifier_only:
        assert torch.equal(r[0]["params0"][n_cls:], s[0]["flat0"][n_cls:].cpu())     # the tower did not move
    # parameters bit-identical across ranks at every step; rank 0's running statistics reach rank 1 before step 1
    assert torch.equal(r[0]["params_final"], r[1]["params_final"])
    assert not torch.equal(r[0]["rm"][0], r[1]["rm"][0])          # per-rank statistics after a step ...
    assert len(r[1]["rm_synced"]) == 2
    assert torch.equal(r[1]["rm_synced"][1], r[0]["rm"][0])      # ... and rank 0's at the start of the next one
    assert torch.equal(r[0]["rm_synced"][1], r[0]["rm"][0])
