"""What one training step of ``torch.nn.DataParallel`` computes, restated in float64 for a pure-torch module on the host, next to
the rule the step engines implement for ``virtual_ranks=R`` and to the whole-batch step they run with one rank.

``nn.DataParallel.forward`` scatters the batch along dimension 0 into contiguous chunks, replicates the module (replica 0
shares the module's buffers, the others get copies that are thrown away), runs every replica on its chunk, and gathers the
outputs on device 0; the loss is taken there over the gathered batch, and the backward pass through ``Broadcast`` SUMS the
replicas' parameter gradients into the module's.  No device is needed to say that: deep copies stand in for the replicas."""
import copy

import torch
import torch.nn.functional as F


def _double(model):
    return copy.deepcopy(model).double().train()


def _buffers(model):
    return {n: b.detach().clone() for n, b in model.named_buffers()}


def data_parallel(model, x, y, R):
    """(parameter gradients, buffers after the step, loss) of ``nn.DataParallel(model)`` over R replicas on the batch (x, y):
    one ``F.cross_entropy`` over the concatenated logits, replica gradients summed in rank order, replica 0's buffers."""
    b = x.shape[0] // R
    assert b * R == x.shape[0]
    replicas = [_double(model) for _ in range(R)]
    logits = torch.cat([rep(x[r * b:(r + 1) * b].double()) for r, rep in enumerate(replicas)])
    loss = F.cross_entropy(logits, y)
    loss.backward()
    grads = []
    for ps in zip(*(rep.parameters() for rep in replicas)):
        g = ps[0].grad.clone()
        for p in ps[1:]:
            g = g + p.grad
        grads.append(g)
    return grads, _buffers(replicas[0]), loss.detach()


def engine_rule(model, x, y, R):
    """The same step as the engines run it: every shard's own mean cross-entropy and its gradient, the gradients summed in
    rank order and scaled by 1 / R (the optimizer's ``grad_scale``), shard 0's buffers; the loss the mean of the shards'."""
    b = x.shape[0] // R
    assert b * R == x.shape[0]
    grads, losses, bufs = None, [], None
    for r in range(R):
        rep = _double(model)
        loss = F.cross_entropy(rep(x[r * b:(r + 1) * b].double()), y[r * b:(r + 1) * b])
        loss.backward()
        g = [p.grad for p in rep.parameters()]
        grads = g if grads is None else [a + c for a, c in zip(grads, g)]
        losses.append(loss.detach())
        if r == 0:
            bufs = _buffers(rep)
    return [g / R for g in grads], bufs, torch.stack(losses).mean()


def whole_batch(model, x, y):
    """The one-rank step: every BatchNorm normalises with the statistics of the whole batch."""
    rep = _double(model)
    loss = F.cross_entropy(rep(x.double()), y)
    loss.backward()
    return [p.grad for p in rep.parameters()], _buffers(rep), loss.detach()


def rel(a, b):
    """max |a - b| / max |b| over two lists of tensors."""
    num = max(float((s - t).abs().max()) for s, t in zip(a, b))
    return num / max(float(t.abs().max()) for t in b)
