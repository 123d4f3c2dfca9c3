"""Data-parallel training step: one process per MI355X, RCCL (torch.distributed "nccl") over xGMI.

What the reference does with ``DistributedDataParallel`` + ``torch.optim.Adam``
(utils/main_utils.py:105-117, :250-261; main-avid.py:155-180) is done here with

* ``FlatParams``   — every parameter (and its gradient) is a strided view into ONE flat fp32 buffer,
                     laid out in reverse registration order so buckets complete front-to-back while
                     backward runs (conv5x / heads first).  Views keep each tensor's memory format,
                     so the channels-last conv weights stay channels-last.
* ``GradBuckets``  — per-bucket async all-reduce (sum) launched from post-accumulate-grad hooks as soon
                     as the bucket's last gradient is written, i.e. overlapped with the rest of
                     backward; ``finish()`` makes the compute stream wait.  The 1/world average is
                     folded into the optimizer kernel's ``grad_scale``.
* ``FlatBuffers``  — the BatchNorm running statistics as views of one flat buffer: DDP's buffer broadcast
                     (``broadcast_buffers=True``, the default of utils/main_utils.py:112) is ONE 78 KB collective.
* ``EngineCore``   — what the step engines share: the model in those buffers, the backward launch program cut at bucket
                     ends.  No optimizer, no criterion (``DistributedDataParallel``'s engine is this and little else).
* ``AdamStep``     — the core + one fused flat-Adam launch; ``state_dict`` / ``load_state_dict`` in torch.optim.Adam's
                     format (the reference's CheckpointManager saves ``optimizer.state_dict()``, main-avid.py:115,127,138).
                     ``optimizer="sgd"``: the other optimizer of ``build_optimizer`` (utils/main_utils.py:242-248) instead —
                     one flat SGD launch, one momentum buffer, torch.optim.SGD's checkpoint format.
                     ``param_rules`` (per-tensor lr scale / weight decay) and ``optimizer="lars"`` / ``"lamb"`` run the
                     table-driven kernels over an ``ops.SegmentTable`` of the flat layout.
* ``TrainStep``    — AdamStep for pretraining: fwd -> criterion -> bwd (+ overlapped all-reduce) -> Adam; hipGraph capture
                     (``FinetuneStep``: for action-recognition fine-tuning).

The comm layer is backend-agnostic (gloo on CPU in tests/test_distributed_cpu.py); only the Adam
kernel needs the GPU.  BatchNorm statistics stay per-rank — the reference has no SyncBN.
"""
from __future__ import annotations

import contextlib
import math
import os
import re
import warnings
import weakref
import torch
import torch.distributed as dist
from . import lib


_FLAT_OF = {}           # id(parameter) -> weakref(FlatParams it is a view of)
_U64 = 0xFFFFFFFFFFFFFFFF
_RANK_SEED_STRIDE = 0x9E3779B97F4A7C15      # rank r's negative sampler: base seed + stride * r (criterions/avid.py)


def flat_of(params):
    """The FlatParams whose parameters are exactly ``params`` (any order), or None."""
    params = [p for p in params if p.requires_grad]
    if not params:
        return None
    ref = _FLAT_OF.get(id(params[0]))
    flat = ref() if ref is not None else None
    if flat is None or len(flat.params) != len(params):
        return None
    mine = {id(p) for p in flat.params}
    if any(id(p) not in mine for p in params) or any(p.data_ptr() != flat.flat.data_ptr() + 4 * o
                                                     for p, o in zip(flat.params, flat.offsets)):
        return None
    return flat


def _dist_on():
    """Collectives are in play: more than one rank (or AVID_FORCE_DIST=1, which drives the RCCL path on a
    single-rank group so it can be exercised on a one-GPU box)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("AVID_FORCE_DIST", "0") == "1"


class FlatParams:
    """Re-seat ``module``'s parameters and gradients as views of two flat buffers."""

    def __init__(self, module):
        """``module``: an nn.Module, or the parameters themselves (an optimizer's: Adam below)."""
        src = module.parameters() if isinstance(module, torch.nn.Module) else module
        params = [p for p in src if p.requires_grad]
        self.params = list(reversed(params))            # backward produces gradients roughly in this order
        dev, dt = self.params[0].device, self.params[0].dtype
        self.offsets, off = [], 0
        for p in self.params:
            if not (p.is_contiguous() or p.movedim(1, -1).is_contiguous()):
                raise ValueError("FlatParams needs dense parameters")
            self.offsets.append(off)
            off += (p.numel() + 3) // 4 * 4             # keep every slice 16-byte aligned
        self.numel = off
        self.flat = torch.zeros(off, dtype=dt, device=dev)
        self.grad = torch.zeros(off, dtype=dt, device=dev)
        self.grad_views = []
        for i, p in enumerate(self.params):
            view = self.view(self.flat, i)
            view.copy_(p.data)
            p.data = view
            p.grad = self.view(self.grad, i)
            self.grad_views.append(p.grad)
            _FLAT_OF[id(p)] = weakref.ref(self)

    def view(self, buf, i):
        """Parameter i's view (its shape and strides) of ``buf``, a flat tensor laid out like ``flat``: a gradient, an Adam moment."""
        p, o = self.params[i], self.offsets[i]
        return buf[o:o + p.numel()].as_strided(p.shape, p.stride())

    def seat_grads(self):
        """`.grad` of every parameter is its view of the flat gradient buffer again (it was None after a
        zero_grad(set_to_none=True), or something pointed it elsewhere: the kernels wrote the buffer, not the attribute)."""
        for p, v in zip(self.params, self.grad_views):
            if p.grad is not v:
                p.grad = v

    def zero_grad(self):
        self.grad.zero_()
        self.seat_grads()

    def load_moments(self, m, v, states):
        """Fill the flat Adam moments ``m`` / ``v`` from ``states``: (slot in the flat layout, that parameter's entry of a
        torch.optim.Adam ``state``, or None: zero moments) pairs.  Returns the largest ``step`` among them."""
        m.zero_()
        v.zero_()
        step = 0
        for i, st in states:
            if st:
                self.view(m, i).copy_(st["exp_avg"])
                self.view(v, i).copy_(st["exp_avg_sq"])
                step = max(step, int(float(st["step"])))
        return step

    def load_momentum(self, buf, states):
        """Fill the flat SGD momentum buffer ``buf`` from ``states``, pairs as above of a torch.optim.SGD ``state`` (an entry
        without a buffer: zeros, which the update takes exactly as torch takes a missing one).  Returns whether any was there."""
        buf.zero_()
        found = False
        for i, st in states:
            if st and st.get("momentum_buffer") is not None:
                self.view(buf, i).copy_(st["momentum_buffer"])
                found = True
        return found


class FlatBuffers:
    """The floating-point buffers of ``module`` (BatchNorm running_mean / running_var) re-seated as views of one
    flat tensor, so that broadcasting rank 0's buffers — what DistributedDataParallel(broadcast_buffers=True)
    does before every forward — is a single small collective.  ``num_batches_tracked`` (int64) advances by one
    per step on every rank and is identical everywhere by construction."""

    def __init__(self, module: torch.nn.Module):
        # ONE owner.  models.AV_Wrapper keeps its floating-point buffers in its own flat tensor (`_bn_flat`, what torch's DDP
        # broadcasts) and re-seats them there on every forward: a second flat tensor here would be orphaned by the first
        # evaluation / per-layer forward, and sync_buffers() would then broadcast a tensor nobody reads.  So the module's
        # buffer is ADOPTED (looked up at every use: `.to()` / `.cuda()` re-create it), and only a module without one gets
        # a flat tensor of this class's making.
        self.module = module if (hasattr(module, "_seat_flat_buffers") and getattr(module, "_bn_flat", None) is not None) else None
        if self.module is not None:
            module._seat_flat_buffers()
            mods = dict(module.named_modules())
            self.bufs, self.offsets = [], []
            for n, off, cnt in module._bn_layout:
                owner, _, leaf = n.rpartition(".")
                self.bufs.append(getattr(mods[owner], leaf))
                self.offsets.append(off)
            self.numel = module._bn_flat.numel()
            self._flat = None
            return
        self.bufs = [b for b in module.buffers() if b.is_floating_point()]
        self.offsets, off = [], 0
        for b in self.bufs:
            self.offsets.append(off)
            off += (b.numel() + 3) // 4 * 4
        self.numel = off
        if not self.bufs:
            self._flat = None
            return
        self._flat = torch.zeros(off, dtype=self.bufs[0].dtype, device=self.bufs[0].device)
        for b, o in zip(self.bufs, self.offsets):
            view = self._flat[o:o + b.numel()].view(b.shape)
            view.copy_(b)
            b.data = view

    @property
    def flat(self):
        if self.module is not None:
            self.module._seat_flat_buffers()             # (no-op unless the buffers were re-created since)
            return self.module._bn_flat
        return self._flat

    def broadcast(self, src=0, async_op=False):
        if self.flat is None or not _dist_on():
            return None
        return dist.broadcast(self.flat, src, async_op=async_op)


class GradBuckets:
    """Bucketed, backward-overlapped gradient all-reduce over a ``FlatParams`` gradient buffer."""

    def __init__(self, flat: FlatParams, bucket_bytes: int = 16 << 20, average: bool = False, hooks=None):
        """``average``: the collective leaves the MEAN over ranks in the buffer (what torch's DDP hands the optimizer) instead
        of the sum (TrainStep folds 1 / world into its Adam launch).  ``hooks``: autograd hooks on every parameter — default:
        only where no kernel reports its gradients itself (CPU tensors)."""
        self.flat = flat
        self.average = average
        self.world = dist.get_world_size() if _dist_on() else 1
        self.comm = _dist_on()
        self.bounds, self.bucket_of = [], []
        start, cur = 0, 0
        for i, (p, o) in enumerate(zip(flat.params, flat.offsets)):
            end = o + (p.numel() + 3) // 4 * 4
            self.bucket_of.append(len(self.bounds))
            if (end - start) * 4 >= bucket_bytes or i == len(flat.params) - 1:
                self.bounds.append((start, end))
                start = end
        self.counts = [0] * len(self.bounds)
        for b in self.bucket_of:
            self.counts[b] += 1
        self.pending = list(self.counts)
        self.launched = [False] * len(self.bounds)        # bucket b's collective has been issued this step
        self.reported = [False] * len(flat.params)        # parameter i's gradient was reported (ready(i)) this step
        self.works = []
        self.hooks = []
        self.comm_used = []           # every collectives' stream a bucket went out on this step (normally one)
        self.step_set = None          # the step's StreamSet, resolved once per step (first bucket)
        self.measure = False          # bench.py: event-time the compute stream's wait for the collectives in finish()
        self.on_autograd = None       # called from every autograd hook (DistributedDataParallel: arm the end-of-backward callback)
        self.wait_events = []
        self.producers = [set() for _ in self.bounds]     # streams that issued gradients of each bucket
        # Autograd hooks only where the kernels do not report their gradients themselves (ops.GradSlots, the
        # CUDA path): 141 tensor hooks cost ~0.4 ms of backward per step on the single-rank check.  A gradient
        # that arrives through autograd anyway (a parameter used twice) is picked up by finish().
        if (self.comm and not flat.grad.is_cuda) if hooks is None else hooks:
            for i, p in enumerate(flat.params):
                self.hooks.append(p.register_post_accumulate_grad_hook(self._make_hook(i)))

    def ready(self, i, stream=None):
        """Gradient of parameter i has been issued on ``stream`` (default: the current one) — autograd hook,
        ops.GradSlots for kernels that write the flat buffer directly, or a launch program's segment end: launch its
        bucket's all-reduce once the bucket is complete."""
        self.reported[i] = True
        if not self.comm:
            return
        b = self.bucket_of[i]
        if self.flat.grad.is_cuda:
            self.producers[b].add(stream if stream is not None else torch.cuda.current_stream(self.flat.grad.device))
        self.pending[b] -= 1
        if self.pending[b] == 0 and not self._capturing():
            self._launch(b)

    def _capturing(self):
        return self.flat.grad.is_cuda and torch.cuda.is_current_stream_capturing()

    def _make_hook(self, i):
        view = self.flat.grad_views[i]

        def hook(param):
            # a gradient that came through autograd into a tensor of its own (`.grad` was None: zero_grad(set_to_none=True))
            # belongs in the flat buffer the collectives and the optimizer read
            g = param.grad
            if g is not None and g.data_ptr() != view.data_ptr():
                view.copy_(g)
                param.grad = view
            if self.on_autograd is not None:
                self.on_autograd()
            self.ready(i)
        return hook

    def _mean_by_division(self):
        """Averaging on a backend without ReduceOp.AVG (gloo: CPU tensors, the two-ranks-on-one-GPU tests; RCCL has it): the
        collective sums, and with more than one rank the sum is divided behind it."""
        return self.average and dist.get_backend() != "nccl"

    def _reduce(self, grad):
        """All-reduce ``grad`` (the flat gradient buffer or a slice) on the current stream: the sum, or the mean with ``average``."""
        divide = self._mean_by_division()
        dist.all_reduce(grad, op=dist.ReduceOp.AVG if self.average and not divide else dist.ReduceOp.SUM)
        if divide and self.world > 1:
            grad.div_(self.world)

    def _launch(self, b):
        self.launched[b] = True
        self._issue(b)

    def _issue(self, b):
        """Issue bucket b's all-reduce on the collectives' stream of the step's StreamSet (avid_hip/streams.py: a stream
        on a dispatch pipe of its own), ordered behind every stream that produced one of the bucket's gradients — the
        compute streams never wait here, and nothing waits for the collective before ``finish()``.  The collective is
        issued as a stream-synchronous op under that stream: torch's NCCL process group then runs it ON that stream
        (c10d: ``asyncOp = false`` uses the current stream) instead of its internal one, whose hardware queue we could
        not choose — two queues on one dispatch pipe serialise, and a queue waiting for an event of its pipe-mate
        stalls both (the 6-8 ms a one-rank group used to add)."""
        s, e = self.bounds[b]
        if not self.flat.grad.is_cuda:
            # (gloo has no AVG: the mean is taken in finish(), behind the wait)
            self.works.append(dist.all_reduce(self.flat.grad[s:e], async_op=True))
            return
        from . import streams
        dev = self.flat.grad.device
        # ONE StreamSet per step: the first bucket resolves it (from whichever of the set's streams is current — the
        # per-layer path reports deferred weight gradients with the trailing stream current), the rest of the step reuses
        # it, so every bucket goes out on the same comm stream of the same RCCL communicator
        ss = self.step_set
        if ss is None:
            ss = self.step_set = streams.current_set(dev)
        prod = self.producers[b] or {ss.main, ss.side, ss.trail}      # unknown producers: everything
        cs = ss.comm
        for st in prod:
            lib.call("avid_stream_wait", cs.cuda_stream, st.cuda_stream)
        with torch.cuda.stream(cs):
            self._reduce(self.flat.grad[s:e])
        if all(cs is not c for c in self.comm_used):
            self.comm_used.append(cs)

    def exposed_wait_ms(self):
        """Mean time per step the compute stream spent waiting for the gradient collectives in ``finish()`` since
        ``measure`` was switched on (synchronises; clears the record)."""
        if not self.wait_events:
            return None
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.wait_events]
        self.wait_events = []
        return sum(ms) / len(ms)

    def finish(self):
        """Launch whatever did not fire (unused parameters, gradients that came through autograd) and make the
        current stream wait for all buckets."""
        if self.comm and self._capturing():
            # Inside a hipGraph capture the bucketed collectives, issued while the backward pass is being recorded, turn
            # into joins of the streams in the graph (round 2: 23.8 ms per replay against 14 ms eager).  A captured step
            # reduces the whole gradient buffer with ONE collective behind the backward pass instead: the all-reduce is
            # exposed (85 MB), the rest of the graph keeps its shape.
            from . import ops
            dev = self.flat.grad.device
            cur = torch.cuda.current_stream(dev)
            cur.wait_stream(ops.side_stream(dev, 1))         # the audio tower's gradients
            self._reduce(self.flat.grad)
            self.launched = [True] * len(self.bounds)
        if self.comm:
            for b, left in enumerate(self.pending):
                if self.launched[b]:
                    continue
                if left > 0:
                    self.producers[b].clear()        # not all producers are known: wait for every stream
                self._launch(b)
            timed = self.measure and self.flat.grad.is_cuda and not self._capturing()
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            for w in self.works:
                w.wait()                             # (CPU tensors: gloo)
            if self.works and self._mean_by_division() and self.world > 1:
                self.flat.grad.div_(self.world)          # (the works are asynchronous: the division _reduce does, deferred)
            for cs in self.comm_used:
                torch.cuda.current_stream(self.flat.grad.device).wait_stream(cs)
            self.comm_used = []
            if timed:
                e1.record()
                self.wait_events.append((e0, e1))
        self.reset()

    def reset(self):
        """The per-step state as a step finds it.  ``finish()`` ends with it; DistributedDataParallel.forward starts with it, so a
        backward pass that raised half-way (out of memory, 'backward a second time') cannot leave counts behind that keep the
        next step's buckets from ever launching — torch's reducer does the same in prepare_for_backward."""
        self.works = []
        self.comm_used = []
        self.step_set = None
        self.pending = list(self.counts)
        self.launched = [False] * len(self.bounds)
        self.reported = [False] * len(self.flat.params)
        for p in self.producers:
            p.clear()


class EngineCore:
    """What every step engine on this rank's GPU shares: the model in flat buffers, the gradient buckets, the backward kernels'
    transposed weights and gradient slots, the hand-over of a backward launch program.  No criterion and no optimizer."""

    def __init__(self, model, bucket_bytes=16 << 20, broadcast_buffers="step", average=False, hooks=None):
        """``broadcast_buffers``: DistributedDataParallel broadcasts rank 0's BatchNorm buffers before EVERY
        forward (utils/main_utils.py:112, default ``broadcast_buffers=True``).  A training-mode forward never
        reads them (it normalises with the batch statistics), and rank 0's own buffers are never overwritten, so
        the only observable effect is what a non-zero rank evaluates / saves with.  ``"step"`` (default) reproduces
        DDP literally with ONE flat 78 KB broadcast per step (the running statistics are views of one buffer);
        ``"lazy"`` broadcasts at ``sync_buffers()`` only — the caller must invoke it before evaluating or saving on a
        rank other than 0 — ``"off"`` never broadcasts.  ``average`` / ``hooks``: ``GradBuckets``'s."""
        self.model = model
        if broadcast_buffers not in ("lazy", "step", "off"):
            raise ValueError("broadcast_buffers must be 'lazy', 'step' or 'off'")
        self.broadcast_buffers = broadcast_buffers
        if _dist_on():                                   # DDP's construction-time parameter broadcast (C3)
            for p in model.parameters():
                dist.broadcast(p.data, 0)
            for b in model.buffers():
                dist.broadcast(b.data, 0)
        self.flat = FlatParams(model)
        self.flat_buffers = FlatBuffers(model)
        # The audio tower runs on a side stream under the video tower (models/av_wrapper.py): on by default
        # here, because GradBuckets below orders every bucket's collective after the streams that produced it.
        if hasattr(model, "overlap_towers") and os.environ.get("AVID_OVERLAP_TOWERS", "1") == "1":
            model.overlap_towers = True
        if os.environ.get("AVID_BUCKET_MB"):             # tuning knob: gradient all-reduce bucket size
            bucket_bytes = int(float(os.environ["AVID_BUCKET_MB"]) * (1 << 20))
        self.buckets = GradBuckets(self.flat, bucket_bytes, average=average, hooks=hooks)
        self._step_plan = None                           # the launch program the current step's backward ran through
        self._grad_target = None                         # where the launch programs write gradients, if not flat.grad
        self._share_tables, self._tables_of = False, None   # a virtual-rank step: the plan whose derived weight tables are current
        self.twt = self.slots = None
        if self.flat.flat.is_cuda:
            from . import ops
            self.twt = ops.TransposedWeights(self.flat.params)   # dgrad weight repack: one launch per step
            # backward kernels write parameter gradients straight into the flat buffer (no per-parameter add)
            self.slots = ops.GradSlots(self.flat.params, self.flat.grad_views, on_ready=self.buckets.ready)

    def sync_buffers(self):
        """Every rank takes rank 0's BatchNorm running statistics (see ``broadcast_buffers``): call before
        evaluating the model or saving it on a rank other than 0."""
        self.flat_buffers.broadcast(0)

    def grad_target(self):
        """The flat buffer the launch programs zero and write this pass's gradients into: ``flat.grad``, unless a virtual-rank
        step has pointed shard 0 at its accumulator (``AdamStep._virtual_pass``, ``TrainStep._virtual_forward_backward``)."""
        return self.flat.grad if self._grad_target is None else self._grad_target

    def rebuild_tables(self, pl):
        """Whether a forward through ``pl`` has to rebuild the derived weight tables: always, except for the later passes of
        a virtual-rank step (``_share_tables``), which run the program that built them a moment ago from the same weights."""
        if not self._share_tables:
            return True
        fresh, self._tables_of = self._tables_of is not pl, pl
        return fresh

    def _plan_backward(self, pl, fa, inputs):
        """A backward launch program into the flat gradient buffer (``pl.backward``'s ``fa`` / ``inputs``; called from the
        model's autograd node or by ``FinetuneStep``): in one piece, or — with gradient collectives — cut where a bucket
        becomes complete, so that its all-reduce starts under the rest of the pass."""
        self._step_plan = pl
        if not self.buckets.comm or self.buckets._capturing():
            pl.backward(fa, inputs, self.grad_target())
            return
        ba, begin = None, 0
        for end, ready in pl.segments(self.buckets.bucket_of, self.buckets.counts):
            ba = pl.backward(fa, inputs, self.grad_target(), begin, end, ba)
            for i, st in ready:
                self.buckets.ready(i, pl.stream_objs[st])
            begin = end

    def _poll_errors(self):
        """Out-of-range sample ids raise here (non-blocking look at the device error word, ops.DeviceErrors): the
        criterion's own polls do not run when a captured graph is replayed.  The error surfaces about one step after
        the offending kernels, i.e. after Adam has applied that step — ``ops.check_device_errors()`` is the blocking
        form for checkpoint time."""
        if self.flat.flat.is_cuda:
            from . import ops
            ops.poll_device_errors(self.flat.flat.device)


def _virtual_ranks_arg(who, virtual_ranks, broadcast_buffers="step"):
    """An engine's ``virtual_ranks`` argument as R >= 1, or the ValueError that names it: R > 1 emulates the ranks (replicas) of a
    job inside one process and keeps rank 0's BatchNorm running statistics.  Raised before anything is broadcast or flattened."""
    R = int(virtual_ranks)
    if R < 1:
        raise ValueError(f"{who}: virtual_ranks must be >= 1 (got {virtual_ranks})")
    if R > 1:
        if _dist_on():
            raise ValueError(f"{who}(virtual_ranks={R}) emulates the ranks of a job inside ONE process: a process group of "
                             "more than one rank (or AVID_FORCE_DIST=1) is not supported with virtual_ranks > 1")
        if broadcast_buffers != "step":
            raise ValueError(f"{who}(virtual_ranks={R}) keeps rank 0's BatchNorm running statistics, which is "
                             f"broadcast_buffers='step'; broadcast_buffers={broadcast_buffers!r} is not supported with "
                             "virtual_ranks > 1")
    return R


def _ema_decay_arg(who, ema_decay):
    """An engine's ``ema_decay`` as a float in [0, 1), None for no weight average, or the ValueError that names it."""
    if ema_decay is None:
        return None
    d = float(ema_decay)
    if not 0.0 <= d < 1.0:                             # (NaN fails both comparisons)
        raise ValueError(f"{who}: ema_decay must be in [0, 1), or None for no weight average (got {ema_decay})")
    return d


def _sgd_param_group(lr, momentum, weight_decay, nesterov):
    """``param_groups[0]`` (without ``params``) as the installed torch.optim.SGD writes it for these hyper-parameters."""
    probe = torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
    return {k: v for k, v in probe.state_dict()["param_groups"][0].items() if k != "params"}


def _require_format(who, sd, want):
    """``sd`` is a state dict of torch.optim.<want>'s format (``"Adam"`` / ``"SGD"``), told by its first parameter group."""
    g = sd["param_groups"][0]
    got = "Adam" if "betas" in g else "SGD" if "momentum" in g else None
    if got != want:
        given = f"torch.optim.{got}'s" if got else "neither"
        raise ValueError(f"{who} loads torch.optim.{want}'s state dict format, the one given is {given} (torch.optim.Adam: "
                         "param_groups with betas / eps, state step / exp_avg / exp_avg_sq; torch.optim.SGD: param_groups with "
                         "momentum / dampening / nesterov, state momentum_buffer)")
    if want == "SGD" and (g.get("dampening", 0) != 0 or g.get("maximize", False)):
        raise NotImplementedError(f"{who}: dampening / maximize")
    return g


_RULE_KEYS = ("lr_scale", "weight_decay", "adapt")


def rules_no_decay_1d(model):
    """``param_rules`` of the usual exclusion: every trainable tensor with ``ndim <= 1`` (BatchNorm weights and biases, the other
    biases) takes ``weight_decay=0`` and ``adapt=False``.  One anchored pattern per tensor; put rules of your own in front of
    them (the first match wins)."""
    return [("^" + re.escape(n) + "$", {"weight_decay": 0.0, "adapt": False})
            for n, p in model.named_parameters() if p.requires_grad and p.ndim <= 1]


def _resolve_param_rules(who, named, rules):
    """{name: {key: value}} of the overrides ``rules`` — (pattern, dict) pairs, the first ``re.search`` match on the name wins —
    give the (name, parameter) pairs ``named``; the ValueError for an unknown key, a value that is not a finite number >= 0,
    or a rule whose pattern matches no name."""
    named = list(named)
    rules = list(rules or [])
    compiled = []
    for k, rule in enumerate(rules):
        if not (isinstance(rule, (tuple, list)) and len(rule) == 2 and isinstance(rule[1], dict)):
            raise ValueError(f"{who}: param_rules[{k}] is not a (pattern, dict) pair")
        pattern, values = rule
        unknown = sorted(set(values) - set(_RULE_KEYS))
        if unknown:
            raise ValueError(f"{who}: param_rules[{k}] ({pattern!r}) has unknown key(s) {unknown}; the keys are {list(_RULE_KEYS)}")
        clean = {}
        for key, val in values.items():
            if key == "adapt":
                clean[key] = bool(val)
                continue
            val = float(val)
            if not (math.isfinite(val) and val >= 0):
                raise ValueError(f"{who}: param_rules[{k}] ({pattern!r}): {key} must be a finite number >= 0 (got {val})")
            clean[key] = val
        rx = re.compile(pattern)
        if not any(rx.search(n) for n, _ in named):
            raise ValueError(f"{who}: param_rules[{k}] ({pattern!r}) matches no trainable parameter")
        compiled.append((rx, clean))
    out = {}
    for n, _ in named:
        for rx, clean in compiled:
            if rx.search(n):
                out[n] = dict(clean)
                break
    return out


class AdamStep(EngineCore):
    """The core plus Adam over the flat buffers: one fused launch per step (or per slice of the buffers), moments ``m`` / ``v``,
    the step count and learning rate in device memory as well (a captured graph reads them there).

    ``optimizer="sgd"`` (with ``momentum``, ``nesterov``; ``betas`` / ``eps`` are ignored): torch.optim.SGD's update instead,
    the same one launch per slice (``ops.sgd_flat``).  Its only state is ``momentum_buffer``, laid out like the flat
    parameters (None without momentum); ``m`` / ``v`` / ``t_dev`` are None — the update needs no step count, a zero buffer
    is torch's first step — and ``t`` just counts steps on the host.  ``state_dict`` is then torch.optim.SGD's.

    ``optimizer="lars"`` (with ``momentum``, ``nesterov``, ``trust_coefficient``) is the SGD family with a trust factor per
    tensor, ``q = trust_coefficient * |p| / |g~ + wd p|`` on the update in front of the momentum; ``optimizer="lamb"`` (with
    ``betas``, ``eps``) is the Adam family with ``r = |p| / |u|`` on ``u = m^ / (sqrt(v^) + eps) + wd p``.  Both run the
    table-driven kernels (``ops.sgd_flat_table`` / ``ops.lamb_flat``): the norms are per-tensor sums in double in a fixed order,
    the factors stay on the device (``trust``), nothing synchronises the host.  Checkpoints are torch.optim.SGD's / Adam's.
    ``param_rules``: (pattern, dict) pairs, the first ``re.search`` match on a parameter's ``named_parameters()`` name wins;
    the dict may set ``lr_scale``, ``weight_decay`` and ``adapt`` (False: no trust ratio) for the tensors it matches, the
    others keep the engine's values (``rules_no_decay_1d(model)``: the usual exclusion of BatchNorm and biases).  An unknown
    key or a rule that matches nothing raises.  With rules ``"adam"`` / ``"sgd"`` run ``ops.adam_flat_table`` /
    ``ops.sgd_flat_table``; without them exactly the kernels they always ran.  A table-driven step runs its optimizer in
    one piece (as a guarded step does).  ``state_dict()`` gains the key ``avid_param_table`` (name, ``lr_scale``,
    ``weight_decay``, ``adapt`` per tensor), which ``load_state_dict`` compares with the engine's own.

    The step guard, off by default (``guard`` is None and nothing below is launched).  ``max_grad_norm`` (> 0, finite):
    ``torch.nn.utils.clip_grad_norm_``'s rule on the norm of the averaged flat gradient; ``skip_nonfinite=True``: a step whose
    gradient is not finite leaves no trace.  Either one puts ``ops.grad_guard`` behind the backward pass — one fixed-order pass
    over the flat gradient that fills a 32-byte device record, ``guard`` (``ops.StepGuard``: ``grad_norm``, ``clip_coef``,
    ``skipped``, ``skipped_total``, ``steps_total`` as 0-d device tensors; reading one is the caller's synchronisation) — and
    runs the optimizer in one piece through the guarded kernels, which read the record: nothing synchronises the host, a
    captured graph replays it.  In one process ``skip_nonfinite`` also skips a step whose BatchNorm running statistics went
    non-finite (``ops.guard_nonfinite``: a ReLU can keep a NaN channel out of the gradient).  A skipped step leaves the parameters, the optimizer state, ``t_dev``, the BatchNorm running
    statistics, ``num_batches_tracked`` (and ``TrainStep``: both memory banks) exactly as it found them; what still advances
    is the host's ``t`` (it counts ATTEMPTED steps: ``t - int(t_dev) == int(guard.skipped_total)`` for Adam; ``state_dict``
    saves ``t_dev``), the negative sampler's position and the dropout offset — the next step draws fresh ones.

    The weight average, off by default (``ema_decay=None``: nothing below is allocated or launched).  ``ema_decay`` in [0, 1):
    ``ema``, laid out like ``flat.flat`` and started as its copy (timm's rule), follows the parameters by ``e = e + w * (p - e)``,
    ``w = (float)(1 - d)``, inside the optimizer launch itself (``ops.adam_flat_ema`` / ``ops.sgd_flat_ema``, over the slice the
    optimizer updates: a ``classifier_only`` engine averages the classifier and keeps the copy elsewhere); ``ema_warmup``:
    ``d = min(ema_decay, (1 + k) / (10 + k))`` with ``k = ema_updates``, a 0-d device int64 that counts the applied updates;
    ``ema_buffers``: ``ema_buffers_flat`` averages the BatchNorm running statistics the step leaves by one ``ops.ema_flat``
    launch behind the optimizer (``num_batches_tracked`` is not averaged; with ``ema_buffers=False`` evaluation under the
    average uses the live statistics).  One update per step — per global step with ``virtual_ranks`` — a skipped step leaves
    ``ema``, ``ema_updates`` and the averaged statistics as it found them, a captured graph carries the update.
    ``with ema_weights():`` makes the model the averaged one in place, ``ema_state_dict()`` returns it, ``ema_reset()``
    restarts it from the current weights; ``state_dict()`` gains the key ``avid_ema``.  The average is per rank and fp32."""

    virtual_ranks = 1        # ranks whose gradients the buffer holds the SUM of, per process (the step engines' virtual_ranks=R)

    def __init__(self, model, lr, betas, eps, weight_decay, optimizer="adam", momentum=0.0, nesterov=False,
                 max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, ema_buffers=True,
                 param_rules=None, trust_coefficient=0.001, **core):
        ema_decay = _ema_decay_arg(type(self).__name__, ema_decay)
        if optimizer not in ("adam", "sgd", "lars", "lamb"):
            raise ValueError("optimizer must be 'adam', 'sgd', 'lars' or 'lamb'")
        if optimizer in ("sgd", "lars") and (momentum < 0 or (nesterov and momentum == 0)):
            raise ValueError("SGD: momentum must be >= 0, and Nesterov momentum requires a momentum")
        trust_coefficient = float(trust_coefficient)
        if optimizer == "lars" and not (trust_coefficient > 0 and math.isfinite(trust_coefficient)):
            raise ValueError(f"LARS: trust_coefficient must be a finite number > 0 (got {trust_coefficient})")
        # resolved before anything is flattened: a bad rule leaves the model as it was
        overrides = _resolve_param_rules(type(self).__name__, ((n, p) for n, p in model.named_parameters() if p.requires_grad),
                                         param_rules)
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (max_grad_norm > 0 and math.isfinite(max_grad_norm)):
                raise ValueError(f"max_grad_norm must be a finite number > 0, or None for no clipping (got {max_grad_norm})")
        super().__init__(model, **core)
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self.guard = None
        self._fb_saved = self._guard_nbt = None
        self._acc = self._bn_keep = self._nbt = None     # a virtual-rank step's accumulator and rank 0's statistics (_virtual_buffers)
        self._bn_seen = None                             # ... and, skip_nonfinite, what witnesses the later shards' statistics
        if self.max_grad_norm is not None or self.skip_nonfinite:
            from . import ops
            self.guard = ops.StepGuard(self.flat.flat.device)
        self.optimizer = optimizer
        self._sgd_family = optimizer in ("sgd", "lars")
        self.trust_coefficient = trust_coefficient
        # the table-driven kernels: with rules, and always under LARS / LAMB (whose trust ratios are per tensor)
        self._table_on = param_rules is not None or optimizer in ("lars", "lamb")
        names = {id(p): n for n, p in model.named_parameters()}
        self._param_names = [names[id(p)] for p in self.flat.params]          # by slot of the flat layout
        self._param_overrides = [overrides.get(n, {}) for n in self._param_names]
        self._tables = {}
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.momentum, self.nesterov = float(momentum), bool(nesterov)
        self.t = 0
        dev = self.flat.flat.device if self.flat.flat.is_cuda else None
        # the learning rate lives in device memory as well: a captured graph freezes by-value arguments
        self.lr_dev = torch.full((), float(lr), dtype=torch.float32, device=dev) if dev is not None else None
        # the weight average (``ema_decay``): laid out like the flat parameters and started as their copy, the counter of
        # applied averaging updates a device word — a captured graph reads and advances it there
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.ema = self.ema_updates = self.ema_buffers_flat = None
        self._ema_swapped = False
        if ema_decay is not None:
            self.ema = self.flat.flat.detach().clone()
            self.ema_updates = torch.zeros((), dtype=torch.int64, device=self.flat.flat.device)
            fb = self.flat_buffers.flat
            if ema_buffers and fb is not None:
                self.ema_buffers_flat = fb.detach().clone()
        self.m = self.v = self.t_dev = self.momentum_buffer = None
        if self._sgd_family:
            if self.momentum != 0:
                self.momentum_buffer = torch.zeros_like(self.flat.flat)
            return
        self.m = torch.zeros_like(self.flat.flat)
        self.v = torch.zeros_like(self.flat.flat)
        self.t_dev = torch.zeros((), dtype=torch.int64, device=dev) if dev is not None else None

    def set_lr(self, lr):
        """Change the learning rate (an LR scheduler's hook; also reaches a captured graph)."""
        self.lr = float(lr)
        if self.lr_dev is not None:
            self.lr_dev.fill_(self.lr)

    def _grad_scale(self):
        return 1.0 / (self.buckets.world * self.virtual_ranks)

    def _guard_begin(self):
        """In front of a guarded step's forward: the snapshot a skipped step is put back from (``skip_nonfinite``) — the flat
        buffer of BatchNorm running statistics, one 78 KB copy."""
        if not self.skip_nonfinite:
            return
        fb = self.flat_buffers.flat
        if fb is not None:
            if self._fb_saved is None or self._fb_saved.shape != fb.shape or self._fb_saved.device != fb.device:
                self._fb_saved = torch.empty_like(fb)
            self._fb_saved.copy_(fb)
        if self._guard_nbt is None:
            self._guard_nbt = [m.num_batches_tracked for m in self.model.modules()
                               if getattr(m, "num_batches_tracked", None) is not None]

    def _guard_judge(self, begin=0, end=None):
        """Behind a guarded step's backward pass (all gradient collectives finished): judge elements [begin, end) of the flat
        gradient into the record, then — ``skip_nonfinite`` — the launches that put the snapshot back if the record says skip
        (``num_batches_tracked`` goes back by the record's skip word).  All on the device."""
        from . import ops
        ops.grad_guard(self.flat.grad[begin:end], self.guard, grad_scale=self._grad_scale(),
                       max_norm=self.max_grad_norm or 0.0, skip_nonfinite=self.skip_nonfinite)
        if not self.skip_nonfinite:
            return
        fb = self.flat_buffers.flat
        if fb is not None:
            # the running statistics are a second witness: a non-finite activation poisons them even where a ReLU (max(NaN, 0)
            # = 0) keeps it out of the gradient — a frozen tower's heads (ProbeStep) never see it.  One process only: they are
            # per-rank, and with gradient collectives every rank must reach the verdict of the all-reduced gradient.
            if not self.buckets.comm:
                ops.guard_nonfinite(fb, self.guard)
                if self._bn_seen is not None:        # (the later shards' statistics of a virtual-rank step: _virtual_pass)
                    ops.guard_nonfinite(self._bn_seen, self.guard)
            ops.guard_restore(fb, None, self._fb_saved, self.guard)
        if self._guard_nbt:
            torch._foreach_sub_(self._guard_nbt, [self.guard.skipped.to(torch.int64)] * len(self._guard_nbt))

    def _update(self, begin=0, end=None, advance=True, last=True):
        """One optimizer launch over elements [begin, end) of the flat buffers with the engine's hyper-parameters (Adam: step
        ``self.t``; ``advance=False``: another slice of the same step, the device step counter stays.  SGD has no counter).
        With the step guard on: the guarded kernels, which obey the record ``_guard_judge`` filled.  With ``ema_decay``: the
        averaging forms of the same kernels (``last=False``: another slice of the same step follows)."""
        from . import ops
        s = slice(begin, end)
        if self._table_on:
            return self._update_table(begin, end, advance, last)
        if self.ema is not None:
            return self._update_averaging(s, advance, last)
        if self.guard is not None:
            if self.optimizer == "sgd":
                buf = self.momentum_buffer
                ops.sgd_flat_guarded(self.flat.flat[s], self.flat.grad[s], None if buf is None else buf[s], self.lr, self.momentum,
                                     self.wd, self.guard, self.nesterov, grad_scale=self._grad_scale(), lr_dev=self.lr_dev)
                return
            ops.adam_flat_guarded(self.flat.flat[s], self.flat.grad[s], self.m[s], self.v[s], self.lr, self.betas[0],
                                  self.betas[1], self.eps, self.wd, self.t, self.guard, grad_scale=self._grad_scale(),
                                  step_dev=self.t_dev, lr_dev=self.lr_dev, advance=advance)
            return
        if self.optimizer == "sgd":
            buf = self.momentum_buffer
            ops.sgd_flat(self.flat.flat[s], self.flat.grad[s], None if buf is None else buf[s], self.lr, self.momentum, self.wd,
                         self.nesterov, grad_scale=1.0 / (self.buckets.world * self.virtual_ranks), lr_dev=self.lr_dev)
            return
        ops.adam_flat(self.flat.flat[s], self.flat.grad[s], self.m[s], self.v[s], self.lr, self.betas[0], self.betas[1],
                      self.eps, self.wd, self.t, grad_scale=1.0 / (self.buckets.world * self.virtual_ranks), step_dev=self.t_dev,
                      lr_dev=self.lr_dev, advance=advance)

    def _update_averaging(self, s, advance, last):
        """``_update`` with the weight average on: the averaging form of the engine's optimizer kernel over the same slice —
        guarded or not — which leaves ``ema[s]`` updated from the parameters it has just written.  Behind the step's last
        slice: one ``ops.ema_flat`` over the BatchNorm running statistics (final by now: rank 0's, after the guard's restore)
        with the same weight and the same guard, then the counter of updates goes up by one — unless the step was skipped.
        Every launch of a step reads the same count."""
        from . import ops
        self._ema_live("step")
        fb = self.flat_buffers.flat if self.ema_buffers_flat is not None else None
        kw = dict(guard=self.guard, grad_scale=self._grad_scale(), lr_dev=self.lr_dev, warmup=self.ema_warmup,
                  updates_dev=self.ema_updates, ema_advance=last and fb is None)
        if self.optimizer == "sgd":
            buf = self.momentum_buffer
            ops.sgd_flat_ema(self.flat.flat[s], self.flat.grad[s], None if buf is None else buf[s], self.ema[s], self.lr,
                             self.momentum, self.wd, self.ema_decay, nesterov=self.nesterov, **kw)
        else:
            ops.adam_flat_ema(self.flat.flat[s], self.flat.grad[s], self.m[s], self.v[s], self.ema[s], self.lr, self.betas[0],
                              self.betas[1], self.eps, self.wd, self.t, self.ema_decay, step_dev=self.t_dev, advance=advance,
                              **kw)
        if last and fb is not None:
            ops.ema_flat(self.ema_buffers_flat, fb, self.ema_decay, self.ema_warmup, self.ema_updates, self.guard)

    # ---- per-tensor hyper-parameters and trust ratios (``param_rules``, ``optimizer="lars"`` / ``"lamb"``)
    def param_values(self):
        """[(name, lr_scale, weight_decay, adapt)] by slot of the flat layout: the engine's base values (``lr_scale`` 1, its
        ``weight_decay``, ``adapt`` True) under the overrides of the first matching rule."""
        return [(n, float(o.get("lr_scale", 1.0)), float(o.get("weight_decay", self.wd)), bool(o.get("adapt", True)))
                for n, o in zip(self._param_names, self._param_overrides)]

    def _update_range(self):
        """[begin, end) of the flat buffers the optimizer updates (``FinetuneStep(classifier_only=True)``: the classifier's)."""
        return 0, self.flat.numel

    def segment_table(self, begin=None, end=None):
        """The ``ops.SegmentTable`` of elements [begin, end) of the flat buffers (default: the slice the optimizer updates),
        built once per slice and per set of values; its ``trust`` holds the factors the last LARS / LAMB step applied."""
        if begin is None:
            begin, end = self._update_range()
        end = self.flat.numel if end is None else end
        key = (begin, end)
        hit = self._tables.get(key)
        if hit is None or hit[0] != self.wd:               # (a loaded checkpoint may change the base weight decay)
            from . import ops
            vals = self.param_values()
            tab = ops.SegmentTable(self.flat, [v[1] for v in vals], [v[2] for v in vals], [v[3] for v in vals], begin=begin, end=end)
            if hit is not None and hit[1].S == tab.S:
                tab.trust.copy_(hit[1].trust)
            hit = (self.wd, tab)
            self._tables[key] = hit
        return hit[1]

    @property
    def trust(self):
        """float32 [S] on the device: the trust factor of every tensor the optimizer updates, in the flat layout's order, as the
        last applied LARS / LAMB step left it (ones before the first; None for an engine without trust ratios)."""
        return self.segment_table().trust if self.optimizer in ("lars", "lamb") else None

    def _update_table(self, begin, end, advance, last):
        """``_update`` through the table-driven kernels (one kernel per family: guard and average are nullable arguments)."""
        from . import ops
        end = self.flat.numel if end is None else end
        s = slice(begin, end)
        tab = self.segment_table(begin, end)
        kw = dict(grad_scale=self._grad_scale(), lr_dev=self.lr_dev, guard=self.guard)
        fb = None
        if self.ema is not None:
            self._ema_live("step")
            fb = self.flat_buffers.flat if self.ema_buffers_flat is not None else None
            kw.update(ema=self.ema[s], decay=self.ema_decay, warmup=self.ema_warmup, updates_dev=self.ema_updates,
                      ema_advance=last and fb is None)
        if self._sgd_family:
            buf = self.momentum_buffer
            ops.sgd_flat_table(tab, self.flat.flat[s], self.flat.grad[s], None if buf is None else buf[s], self.lr, self.momentum,
                               self.nesterov, trust_coefficient=self.trust_coefficient if self.optimizer == "lars" else None, **kw)
        else:
            fn = ops.lamb_flat if self.optimizer == "lamb" else ops.adam_flat_table
            fn(tab, self.flat.flat[s], self.flat.grad[s], self.m[s], self.v[s], self.lr, self.betas[0], self.betas[1], self.eps,
               self.t, step_dev=self.t_dev, advance=advance, **kw)
        if last and fb is not None:
            ops.ema_flat(self.ema_buffers_flat, fb, self.ema_decay, self.ema_warmup, self.ema_updates, self.guard)

    def _param_table_checkpoint(self):
        vals = self.param_values()
        return [{"name": vals[i][0], "lr_scale": vals[i][1], "weight_decay": vals[i][2], "adapt": vals[i][3]}
                for _, i, _ in self._param_order()]

    def _check_param_table(self, saved):
        """``load_state_dict``: the checkpoint's ``avid_param_table`` against this engine's, tensor by tensor."""
        if saved is None:
            return
        mine = self._param_table_checkpoint()
        for a, b in zip(saved, mine):
            if dict(a) != b:
                raise ValueError(f"{type(self).__name__}.load_state_dict: the checkpoint's avid_param_table differs from this "
                                 f"engine's at tensor {b['name']!r}: saved {dict(a)}, here {b}")
        if len(saved) != len(mine):
            k = min(len(saved), len(mine))
            name = (mine[k] if len(mine) > k else saved[k])["name"]
            raise ValueError(f"{type(self).__name__}.load_state_dict: the checkpoint's avid_param_table holds {len(saved)} "
                             f"tensors, this engine's {len(mine)}: the first one without a partner is {name!r}")

    def optimizer_step(self):
        self.t += 1
        self._update()

    # ---- the weight average (``ema_decay``)
    def _ema_on(self, what):
        if self.ema is None:
            raise RuntimeError(f"{type(self).__name__}.{what}: the engine was built without ema_decay, it keeps no average")

    def _ema_live(self, what):
        """Raise inside ``ema_weights()``: the model holds the average there, a step or a checkpoint would take it for the
        live weights."""
        if self._ema_swapped:
            raise RuntimeError(f"{type(self).__name__}.{what} inside `with ema_weights():` — the model holds the averaged "
                               "weights there; leave the block first")

    def ema_reset(self):
        """The average becomes a copy of the current parameters (and running statistics) and the counter of updates zero:
        call it after loading model weights from a checkpoint that carries no average."""
        self._ema_on("ema_reset")
        self._ema_live("ema_reset")
        self.ema.copy_(self.flat.flat)
        if self.ema_buffers_flat is not None:
            self.ema_buffers_flat.copy_(self.flat_buffers.flat)
        self.ema_updates.zero_()

    def _ema_exchange(self):
        """The flat parameters <-> their average (and the running statistics <-> theirs), in place: ``ops.swap_flat``.  No
        address changes — sealed programs, cached plans and inference programs read the exchanged values — and every
        parameter's version counter goes up, as after any in-place write."""
        from . import ops
        ops.swap_flat(self.flat.flat, self.ema)
        if self.ema_buffers_flat is not None:
            ops.swap_flat(self.flat_buffers.flat, self.ema_buffers_flat)
        bump = getattr(torch.autograd.graph, "increment_version", None) or torch._C._increment_version
        for p in self.flat.params:
            bump(p)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with step.ema_weights():`` — inside the block the model IS the averaged model: ``evaluate``, ``Inference(model)``,
        ``KNNEval(model=...)``, a per-layer forward and ``model.state_dict()`` see the average (with ``ema_buffers`` also the
        averaged running statistics, otherwise the live ones).  Two exchange launches on entry, two on exit; on exit — also by
        an exception — the live weights and statistics are bit for bit what they were.  ``step()`` inside the block raises."""
        self._ema_on("ema_weights")
        self._ema_live("ema_weights")
        self._ema_exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_exchange()
            self._ema_swapped = False

    def _ema_buffer_views(self):
        """[(name in ``model.state_dict()``, its view of ``ema_buffers_flat``)] for every buffer the flat statistics buffer
        holds (``num_batches_tracked`` and anything else outside it is not averaged)."""
        fb = self.flat_buffers.flat
        if self.ema_buffers_flat is None or fb is None:
            return []
        lo, size, out = fb.data_ptr(), fb.element_size(), []
        for name, b in self.model.named_buffers():
            off = (b.data_ptr() - lo) // size
            if b.is_floating_point() and b.numel() and 0 <= off and off + b.numel() <= fb.numel():
                out.append((name, self.ema_buffers_flat[off:off + b.numel()].view(b.shape)))
        return out

    def ema_state_dict(self):
        """``model.state_dict()``'s keys and shapes with the averaged tensors where the average covers them — the trainable
        parameters and, with ``ema_buffers``, the running statistics — and copies of the live ones elsewhere (frozen
        parameters, ``num_batches_tracked``): loads into a fresh model with ``load_state_dict(strict=True)``."""
        self._ema_on("ema_state_dict")
        self._ema_live("ema_state_dict")
        sd = type(self.model.state_dict())((k, v.detach().clone()) for k, v in self.model.state_dict().items())
        slot = {id(p): i for i, p in enumerate(self.flat.params)}
        for name, p in self.model.named_parameters():
            if id(p) in slot and name in sd:
                sd[name] = self.flat.view(self.ema, slot[id(p)]).detach().clone()
        for name, view in self._ema_buffer_views():
            if name in sd:
                sd[name] = view.detach().clone()
        return sd

    def _ema_checkpoint(self):
        """The ``avid_ema`` entry of ``state_dict()``: the average of every parameter the optimizer holds under torch's
        parameter index (``_param_order``), the averaged statistics by name, the hyper-parameters and the count of updates."""
        views = self._ema_buffer_views()
        return {"decay": self.ema_decay, "warmup": self.ema_warmup, "num_updates": int(self.ema_updates),
                "params": {k: self._slice(self.ema, i).detach().clone() for k, i, _ in self._param_order()},
                "buffers": {name: v.detach().clone() for name, v in views} if self.ema_buffers_flat is not None else None}

    def _load_ema_checkpoint(self, saved):
        if self.ema is None:
            return                                   # (an engine without an average ignores the checkpoint's)
        if saved is None:
            warnings.warn(f"{type(self).__name__}.load_state_dict: the checkpoint carries no weight average (avid_ema); the "
                          "engine keeps its current one — call ema_reset() to restart it from the loaded weights")
            return
        self._ema_live("load_state_dict")
        self.ema_decay, self.ema_warmup = _ema_decay_arg(type(self).__name__, saved["decay"]), bool(saved["warmup"])
        for k, i, _ in self._param_order():
            self._slice(self.ema, i).copy_(saved["params"].get(k, saved["params"].get(str(k))))
        if self.ema_buffers_flat is not None:
            if saved.get("buffers") is None:
                warnings.warn(f"{type(self).__name__}.load_state_dict: the checkpoint's average carries no running statistics; "
                              "the engine keeps its current averaged statistics")
            else:
                for name, view in self._ema_buffer_views():
                    view.copy_(saved["buffers"][name])
        self.ema_updates.fill_(int(saved["num_updates"]))

    # ---- a virtual-rank step (``virtual_ranks`` = R > 1): the ranks of an R-rank job, shard after shard on this one GPU
    def _virtual_buffers(self):
        """What a virtual-rank step needs beside the engine's own buffers, made at the first one: the gradient accumulator
        (the size of the flat gradient buffer), room for rank 0's BatchNorm running statistics, the ``num_batches_tracked``."""
        if self._acc is None:
            fb = self.flat_buffers.flat
            self._acc = torch.empty_like(self.flat.grad)
            self._bn_keep = torch.empty_like(fb) if fb is not None else None
            self._nbt = [m.num_batches_tracked for m in self.model.modules() if getattr(m, "num_batches_tracked", None) is not None]

    def _virtual_pass(self, shards, run_shard, end=None):
        """Forward, loss and backward of every rank's shard, in rank order: ``run_shard(r, shard)`` runs them for rank r through
        ONE launch program, writing the parameter gradients into ``grad_target()`` and asking ``rebuild_tables(pl)`` whether
        its forward rebuilds the derived weight tables (the first shard's does, the weights do not change in between).
        Shard 0 writes into the accumulator, every later shard into the flat gradient buffer, followed by one
        ``ops.grad_accum_flat`` over elements [0, end): acc = acc + g, and for the last shard g = acc + g — the flat gradient
        buffer ends up holding the SUM over ranks, ((g0 + g1) + g2) + ..., which the optimizer takes with 1 / R
        (``_grad_scale``).  The BatchNorm running statistics the pass leaves are those shard 0's forward left (a replica other
        than the first never keeps its own; DistributedDataParallel broadcasts rank 0's), ``num_batches_tracked`` has advanced
        by one.  Two 78 KB copies, R - 1 accumulations; nothing synchronises the host."""
        from . import ops
        R = len(shards)
        self._virtual_buffers()
        fb = self.flat_buffers.flat
        acc, grad = self._acc[:end], self.flat.grad[:end]
        # skip_nonfinite: the running statistics are the step guard's second witness (``_guard_judge``), and those of a later
        # shard are not kept — a NaN in its clips that a ReLU hides from the gradient would go unseen.  Their sum goes with them
        # to the guard (one more 78 KB pass per later shard): it is not finite if any of them was not.
        witness = self.skip_nonfinite and fb is not None
        if witness and self._bn_seen is None:
            self._bn_seen = torch.empty_like(fb)
        self._share_tables, self._tables_of = True, None
        try:
            for r, shard in enumerate(shards):
                self._grad_target = self._acc if r == 0 else None
                run_shard(r, shard)
                if r == 0 and fb is not None:
                    self._bn_keep.copy_(fb)
                if r > 0:
                    ops.grad_accum_flat(grad if r == R - 1 else acc, acc, grad)
                    if witness and r == 1:
                        self._bn_seen.copy_(fb)
                    elif witness:
                        self._bn_seen.add_(fb)
        finally:
            self._grad_target = None
            self._share_tables, self._tables_of = False, None
        if fb is not None:
            fb.copy_(self._bn_keep)
        if self._nbt:
            torch._foreach_sub_(self._nbt, R - 1)

    def _virtual_shards(self, video, labels):
        """The global batch [R * b, ...] of a supervised virtual-rank step as (b, [(video, labels) of rank r]): rank r holds
        rows [r * b, (r + 1) * b) — DataParallel's scatter of a divisible batch, DistributedDataParallel's per-rank batch."""
        R, B = self.virtual_ranks, video.shape[0]
        if B % R or labels.shape[0] != B:
            raise ValueError(f"{type(self).__name__}(virtual_ranks={R}).step: the global batch must be R * b samples in video and "
                             f"labels alike; virtual_ranks={R} does not divide {B} (labels {labels.shape[0]})")
        video, labels = self._labelled(video, labels)
        b = B // R
        clips = [video[r * b:(r + 1) * b] for r in range(R)]
        # (a shard is a view of the global batch; one that does not start on a 16-byte boundary — an odd clip size — is copied:
        #  the kernels read their input as the allocator hands tensors out)
        clips = [c.clone() if c.data_ptr() % 16 else c for c in clips]
        return b, [(c, labels[r * b:(r + 1) * b]) for r, c in enumerate(clips)]

    # ---- what the supervised steps (FinetuneStep, ProbeStep) share
    def _set_loss(self, loss, pos_weight, n_classes, label_smoothing=0.0):
        """The loss kind of a supervised engine: ``"ce"`` (softmax cross-entropy against int64 labels [B], ``avid_cls_loss``),
        ``"bce"`` (binary cross-entropy with logits against float32 targets [B, C], ``avid_mlabel_loss``; ``pos_weight``: [C]
        values, kept as one float32 device tensor that the compiled programs reference) or ``"soft_ce"`` (softmax cross-entropy
        against float32 distributions [B, C] — or int64 labels [B], made one-hot on the device — ``avid_soft_ce_loss`` with
        ``label_smoothing``)."""
        from . import plan
        try:
            self.n_classes = int(n_classes() if callable(n_classes) else n_classes)
        except (AttributeError, StopIteration, TypeError):
            self.n_classes = None            # (a model outside the compiled patterns: step() says so)
        if loss in ("bce", "soft_ce") and self.n_classes is None:
            raise ValueError(f"{type(self).__name__}: loss={loss!r} needs a model whose classifier says how many classes there are")
        if pos_weight is not None:
            if loss != "bce":
                raise ValueError(f"{type(self).__name__}: pos_weight belongs to loss='bce'")
            pos_weight = torch.as_tensor(pos_weight).detach().to(device=self.flat.flat.device, dtype=torch.float32).contiguous()
            if tuple(pos_weight.shape) != (self.n_classes,):
                raise ValueError(f"{type(self).__name__}: pos_weight must hold {self.n_classes} values (one per class), got "
                                 f"{tuple(pos_weight.shape)}")
        self.loss, self.pos_weight = plan._loss_kind(loss, pos_weight, self.n_classes, label_smoothing), pos_weight
        self.label_smoothing = float(label_smoothing)

    def _labelled(self, video, labels):
        """A supervised step's inputs, contiguous, the labels checked: int64 [B] on the video's device — under ``loss="bce"``
        targets [B, C], float32 (bool / uint8 are converted), under ``loss="soft_ce"`` float32 targets [B, C] or int64 labels
        [B], which become one-hot rows."""
        video, labels = video.contiguous(), labels.contiguous()
        B = video.shape[0]
        if getattr(self, "loss", "ce") == "bce":
            if labels.dtype in (torch.bool, torch.uint8):
                labels = labels.to(torch.float32)
            if labels.dtype != torch.float32 or tuple(labels.shape) != (B, self.n_classes) or labels.device != video.device:
                raise ValueError(f"{type(self).__name__}.step (loss='bce'): targets must be float32 (or bool / uint8) "
                                 f"[{B}, {self.n_classes}] on {video.device} (got {labels.dtype} {tuple(labels.shape)} on "
                                 f"{labels.device})")
            return video, labels
        if getattr(self, "loss", "ce") == "soft_ce":
            if labels.dtype == torch.int64 and tuple(labels.shape) == (B,) and labels.device == video.device:
                from . import ops
                return video, ops.one_hot(labels, self.n_classes)   # (on the device; a label out of range: LabelError at the poll)
            if labels.dtype != torch.float32 or tuple(labels.shape) != (B, self.n_classes) or labels.device != video.device:
                raise ValueError(f"{type(self).__name__}.step (loss='soft_ce'): targets must be float32 [{B}, {self.n_classes}] or "
                                 f"labels int64 [{B}] on {video.device} (got {labels.dtype} {tuple(labels.shape)} on "
                                 f"{labels.device})")
            return video, labels
        if labels.dtype != torch.int64 or tuple(labels.shape) != (B,) or labels.device != video.device:
            raise ValueError(f"{type(self).__name__}.step: labels must be int64 [{B}] on {video.device} "
                             f"(got {labels.dtype} {tuple(labels.shape)} on {labels.device})")
        return video, labels

    def _eval_loss(self, logits, labels, clips):
        """``ops.cls_loss`` / ``ops.mlabel_loss`` (the engine's loss kind) over the V * clips logits of a dense evaluation;
        ``"soft_ce"``: ``ops.cls_loss`` for int64 labels [V], ``ops.soft_ce_loss`` for float32 targets [V, C] — never smoothed."""
        from . import ops
        if self.loss == "soft_ce" and labels.dtype != torch.int64:
            return ops.soft_ce_loss(logits, labels, clips, 0.0)
        if self.loss == "bce":
            if labels.dtype in (torch.bool, torch.uint8):
                labels = labels.to(torch.float32)
            return ops.mlabel_loss(logits, labels, clips, self.pos_weight)
        return ops.cls_loss(logits, labels, clips)

    def _evaluate(self, video, batch, finish):
        """``run_phase('test_dense')``: video [V, clips, 3, T, H, W] (an audio tower: spectrograms [V, clips, 1, T, F]) through the
        model in eval mode, ``batch`` clips at a time (the
        reference's BatchWrapper; ``Inference``: one program per distinct chunk size, cached on the model).  Returns
        ``finish([the chunks' outputs])``, evaluated before the model's mode is restored."""
        x = video.flatten(0, 1)
        was = self.model.training
        self.model.eval()
        try:
            infer = Inference(self.model)
            with torch.no_grad():
                return finish([infer(x[i:i + batch].contiguous()) for i in range(0, x.shape[0], batch)])
        finally:
            self.model.train(was)

    # ---- optimizer state in torch.optim.Adam's format (main-avid.py:115,127,138 save and restore
    # ``optimizer.state_dict()``; utils/main_utils.py:250-261 builds Adam over model.parameters())
    def _param_order(self):
        """[(index in ``list(model.parameters())`` — frozen parameters included, as torch.optim.Adam built over
        ``model.parameters()`` numbers them (utils/main_utils.py:250-261) —, slot in the flat layout, parameter)]
        for the trainable parameters."""
        slot = {id(p): i for i, p in enumerate(self.flat.params)}
        return [(k, slot[id(p)], p) for k, p in enumerate(self.model.parameters()) if id(p) in slot]

    def _slice(self, flat_tensor, i):
        return self.flat.view(flat_tensor, i)

    def _sgd_state_dict(self):
        """torch.optim.SGD's format: a ``momentum_buffer`` per trainable parameter once a step has run (none without momentum)."""
        state = {}
        if self.t > 0 and self.momentum_buffer is not None:
            for k, i, _ in self._param_order():
                state[k] = {"momentum_buffer": self._slice(self.momentum_buffer, i).detach().clone()}
        group = _sgd_param_group(self.lr, self.momentum, self.wd, self.nesterov)
        group["params"] = list(range(sum(1 for _ in self.model.parameters())))
        return {"state": state, "param_groups": [group]}

    def _load_sgd_state_dict(self, sd):
        g = _require_format(type(self).__name__, sd, "SGD")
        self.momentum, self.wd, self.nesterov = float(g["momentum"]), g["weight_decay"], bool(g["nesterov"])
        self.set_lr(g["lr"])
        if self.momentum == 0:
            self.momentum_buffer, self.t = None, 0
            return
        if self.momentum_buffer is None:
            self.momentum_buffer = torch.zeros_like(self.flat.flat)
        self.t = int(self.flat.load_momentum(self.momentum_buffer, ((i, sd["state"].get(k, sd["state"].get(str(k))))
                                                                    for k, i, _ in self._param_order())))

    def state_dict(self):
        """torch.optim.Adam's (SGD's) format.  Adam's ``step`` is the device counter ``t_dev``: the steps APPLIED — with the step
        guard on it lags the host's ``t`` (attempted steps) by ``guard.skipped_total``.  With ``ema_decay`` one more top-level
        key, ``avid_ema`` (``_ema_checkpoint``); without it the dict is the optimizer's alone."""
        sd = self._optimizer_state_dict()
        if self._table_on:
            sd["avid_param_table"] = self._param_table_checkpoint()
        if self.ema is not None:
            self._ema_live("state_dict")
            sd["avid_ema"] = self._ema_checkpoint()
        return sd

    def _optimizer_state_dict(self):
        if self._sgd_family:
            return self._sgd_state_dict()
        step = float(int(self.t_dev) if self.t_dev is not None else self.t)
        state = {}
        if step > 0:
            for k, i, _ in self._param_order():                 # (a frozen parameter has an index but no state, as in torch)
                state[k] = {"step": torch.tensor(step), "exp_avg": self._slice(self.m, i).detach().clone(),
                            "exp_avg_sq": self._slice(self.v, i).detach().clone()}
        nparams = sum(1 for _ in self.model.parameters())
        return {"state": state,
                "param_groups": [{"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd,
                                  "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                                  "differentiable": False, "fused": None, "decoupled_weight_decay": False,
                                  "params": list(range(nparams))}]}

    def load_state_dict(self, sd):
        self._load_optimizer_state_dict(sd)
        self._check_param_table(sd.get("avid_param_table"))
        self._load_ema_checkpoint(sd.get("avid_ema"))

    def _load_optimizer_state_dict(self, sd):
        if self._sgd_family:
            return self._load_sgd_state_dict(sd)
        g = _require_format(type(self).__name__, sd, "Adam")
        self.betas, self.eps, self.wd = tuple(g["betas"]), g["eps"], g["weight_decay"]
        self.set_lr(g["lr"])
        self.t = self.flat.load_moments(self.m, self.v, ((i, sd["state"].get(k, sd["state"].get(str(k))))
                                                         for k, i, _ in self._param_order()))
        if self.t_dev is not None:
            self.t_dev.fill_(self.t)


class TrainStep(AdamStep):
    """One AVID training step (main-avid.py:155-180) on this rank's GPU.

    ``step(video, audio, index)`` returns the (device) loss tensor; nothing synchronises the host.
    Adam hyper-parameters follow the shipped configs (lr 2e-4, betas (0.9, 0.999), L2 wd 1e-5).
    """

    def __init__(self, model, criterion, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5,
                 bucket_bytes=16 << 20, broadcast_buffers="step", optimizer="adam", momentum=0.0, nesterov=False,
                 virtual_ranks=1, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, ema_buffers=True,
                 param_rules=None, trust_coefficient=0.001):
        """``broadcast_buffers``: see ``EngineCore``.  ``optimizer`` / ``momentum`` / ``nesterov``: see ``AdamStep``.
        ``max_grad_norm`` / ``skip_nonfinite``: the step guard, see ``AdamStep``.  Here a skipped step also puts back the bank
        rows it updated, the optimizer gives up its overlapped early slice (it would run before the norm is known), and the
        step that freezes Z reads the skip word back (the one host synchronisation: a skipped first step estimates Z again).
        ``virtual_ranks`` = R > 1: ``step`` takes the GLOBAL batch [R * b, ...] and is the step of an R-rank job of per-rank
        batch b, run on this one GPU shard after shard (``_virtual_forward_backward``): per-shard BatchNorm statistics,
        per-rank negatives, the first step's Z the mean of the ranks', the gradient their mean, one bank update with all
        records in rank order, rank 0's running statistics.  One process only, ``broadcast_buffers="step"``, no ``capture()``."""
        R = _virtual_ranks_arg("TrainStep", virtual_ranks, broadcast_buffers)
        if R > 1 and getattr(criterion, "in_batch_negatives", False):
            raise ValueError(f"TrainStep(virtual_ranks={R}): {type(criterion).__name__} takes its negatives from the batch — the "
                             "exact loss needs every shard's embeddings before any shard's backward, which a shard-after-shard "
                             "step cannot give; virtual_ranks > 1 is not supported with an in-batch criterion")
        super().__init__(model, lr, betas, eps, weight_decay, optimizer=optimizer, momentum=momentum, nesterov=nesterov,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup,
                         ema_buffers=ema_buffers, param_rules=param_rules, trust_coefficient=trust_coefficient,
                         bucket_bytes=bucket_bytes, broadcast_buffers=broadcast_buffers)
        self.criterion = criterion
        self.graph = None
        self.virtual_ranks = R
        self.rank_losses = None      # [R] device tensor: the loss each rank of the emulated job logged in the last step
        self._rank_sampler = None    # per virtual rank: [seed, offset] of its negative-sampler stream
        mult = self._sampler()
        if R > 1 and mult is not None:                   # criterions/avid.py AVIDSimilarityMemoryBank.__init__'s per-rank formula
            self._rank_sampler = [[(int(mult.seed) + _RANK_SEED_STRIDE * r) & _U64, int(mult.offset)] for r in range(R)]

    def reseed(self, seeds, offset=0):
        """Set the seed of every (virtual) rank's negative-sampler stream and the position all of them are at."""
        seeds = [int(s) & _U64 for s in seeds]
        mult = self._sampler()
        if len(seeds) != self.virtual_ranks:
            raise ValueError(f"TrainStep.reseed: {self.virtual_ranks} seed(s) expected, one per virtual rank (got {len(seeds)})")
        if mult is None:
            raise ValueError("TrainStep.reseed: the criterion has no negative sampler")
        mult.reseed(seeds[0], offset)
        if self.virtual_ranks > 1:
            self._rank_sampler = [[s, int(offset)] for s in seeds]

    def _partition_terms(self):
        """The criterion's NCE terms: every module that freezes a partition constant Z on its first call (criterions/nce.py)."""
        return [m for m in self.criterion.modules() if hasattr(m, "avg_exp_score") and hasattr(m, "z_ready")]

    def _shard_forward(self, r, shard):
        """Virtual rank r's forward through the launch programs and the criterion, with ITS sampler stream: (embeddings' loss
        node, where the stream stands afterwards).  The programs are the only path: there is no per-layer form of this step."""
        from . import plan
        mult = self._sampler()
        if mult is not None:
            mult.reseed(*self._rank_sampler[r])
        out = plan.run(self.model, shard[0], shard[1])
        if out is None:
            raise lib.AvidHipError("TrainStep(virtual_ranks > 1) runs through the compiled launch programs only; this model / "
                                   "these inputs are outside them (hooked or frozen modules, non-fp32 or host tensors)")
        return out, mult

    def _partition_pass(self, shards, terms):
        """The first step of an R-rank job: every rank estimates Z from ITS first batch and all take the mean over ranks
        (criterions/nce.py:27-33) — so the R per-shard values are needed before any shard's loss.  A statistics pass: every
        shard's forward and criterion (no backward), its Z noted, Z reset; then Z = ((z0 + z1) + ...) / R, frozen.  It leaves
        no other trace: the BatchNorm buffers and ``num_batches_tracked`` are put back, the bank updates are dropped, the
        samplers' positions are not stored (the real pass draws the same negatives again)."""
        from . import plan
        R = self.virtual_ranks
        fb, bank = self.flat_buffers.flat, self.criterion.nce_average
        saved = fb.clone() if fb is not None else None
        zs = [[] for _ in terms]
        bank.defer_updates()
        try:
            for r, shard in enumerate(shards):
                for m in terms:
                    m.avg_exp_score.fill_(-1.0)
                    m._z_ready = False
                with plan.engine(self):
                    out, _ = self._shard_forward(r, shard)
                    with torch.no_grad():
                        self.criterion(out[0], out[1], shard[2])
                for z, m in zip(zs, terms):
                    z.append(m.avg_exp_score.clone())
        finally:
            bank.flush_updates(apply=False)
        if saved is not None:
            fb.copy_(saved)
        if self._nbt:
            torch._foreach_sub_(self._nbt, R)
        for z, m in zip(zs, terms):
            acc = z[0]
            for other in z[1:]:
                acc += other
            acc /= R
            m.avg_exp_score.copy_(acc)
            m._z_ready = True

    def _virtual_forward_backward(self, video, audio, index):
        """forward_backward of an R-rank job on the global batch: the flat gradient buffer ends up holding the SUM over ranks,
        left to right in rank order, ((g0 + g1) + g2) + ... — what the ranks' all-reduce leaves — ``rank_losses`` the ranks'
        losses; returns their mean.  Shard 0's programs write straight into the accumulator, every later shard's into the
        flat gradient buffer, followed by one ``ops.grad_accum_flat``: acc = acc + g, and for the last shard g = acc + g."""
        from . import ops, plan
        R = self.virtual_ranks
        B = video.shape[0]
        if B % R or audio.shape[0] != B or index.shape[0] != B:
            raise ValueError(f"TrainStep(virtual_ranks={R}).step: the global batch must be R * b samples in video, audio and index "
                             f"alike; virtual_ranks={R} does not divide {B} (audio {audio.shape[0]}, index {index.shape[0]})")
        if not self.flat.grad.is_cuda:
            raise lib.AvidHipError("TrainStep(virtual_ranks > 1) needs the model on a HIP device")
        b = B // R
        video, audio, index = video.contiguous(), audio.contiguous(), index.contiguous()
        shards = [(video[r * b:(r + 1) * b], audio[r * b:(r + 1) * b], index[r * b:(r + 1) * b]) for r in range(R)]
        fb, bank = self.flat_buffers.flat, self.criterion.nce_average
        self._virtual_buffers()
        if self._rank_sampler is None and self._sampler() is not None:
            raise ValueError("TrainStep(virtual_ranks > 1): the criterion's negative sampler appeared after the engine was built; "
                             "call reseed() with one seed per virtual rank")
        terms = self._partition_terms()
        first = [m for m in terms if not m.z_ready()]
        fused = ops.FUSED_CRITERION
        self._share_tables, self._tables_of = True, None
        losses = []
        try:
            if first:
                self._partition_pass(shards, first)
                # every rank of a real job runs its first step through the unfused criterion ops (Z is not frozen when it
                # enters the criterion): so does every shard here — the same launches, the same bits
                ops.FUSED_CRITERION = False
            bank.defer_updates()
            for r, shard in enumerate(shards):
                last = r == R - 1
                self._grad_target = self._acc if r == 0 else None
                with plan.engine(self):
                    out, mult = self._shard_forward(r, shard)
                    # DDP broadcasts rank 0's buffers in front of every forward: what the step leaves is what shard 0's forward left
                    if r == 0 and fb is not None:
                        self._bn_keep.copy_(fb)
                    if last:
                        if fb is not None:
                            fb.copy_(self._bn_keep)
                        if self._nbt:
                            torch._foreach_sub_(self._nbt, R - 1)
                    loss, _ = self.criterion(out[0], out[1], shard[2])
                    loss.backward()
                self.buckets.finish()
                if mult is not None:
                    self._rank_sampler[r][1] = int(mult.offset)
                losses.append(loss.detach())
                if r > 0:
                    ops.grad_accum_flat(self.flat.grad if last else self._acc, self._acc, self.flat.grad)
        except BaseException:
            bank.flush_updates(apply=False)
            raise
        finally:
            ops.FUSED_CRITERION = fused
            self._grad_target = None
            self._share_tables, self._tables_of = False, None
        bank.flush_updates()             # ONE bank update with the R * b records in global order
        self.rank_losses = torch.stack(losses)
        return self.rank_losses.mean()

    def _forward_backward_plan(self, video, audio, index):
        """The step through the compiled launch programs (avid_hip/plan.py); None if the model is outside them."""
        from . import plan
        if not self.flat.grad.is_cuda:
            return None
        with plan.engine(self):
            out = plan.run(self.model, video, audio)
            if out is None:
                return None
            loss, _ = self.criterion(out[0], out[1], index)
            loss.backward()
        self.buckets.finish()
        return loss

    def _bank(self):
        """The criterion's memory banks (``nce_average``) if they can note the rows an update writes, or None."""
        bank = getattr(self.criterion, "nce_average", None)
        return bank if hasattr(bank, "kept_rows") else None

    def _guard_begin(self):
        super()._guard_begin()
        bank = self._bank()
        if self.skip_nonfinite and bank is not None:      # (criterions/avid.py: update_memory notes the rows it writes)
            bank.keep_rows, bank.kept_rows = True, None

    def _guard_judge(self, begin=0, end=None):
        from . import ops
        super()._guard_judge(begin, end)
        bank = self._bank()
        if self.skip_nonfinite and bank is not None:
            kept, bank.keep_rows, bank.kept_rows = bank.kept_rows, False, None
            if kept is not None:
                ops.guard_restore(bank.view1_mem, kept[0], kept[1], self.guard)
                ops.guard_restore(bank.view2_mem, kept[0], kept[2], self.guard)

    def forward_backward(self, video, audio, index):
        """Forward, criterion, backward, gradient collectives.  With the step guard on also its judgement (``guard`` is filled
        when this returns, ``optimizer_step()`` obeys it) and, ``skip_nonfinite``, the restoring launches of a skipped step."""
        if self.guard is None:
            return self._forward_backward(video, audio, index)
        unfrozen = [m for m in self._partition_terms() if not m.z_ready()] if self.skip_nonfinite else []
        self._guard_begin()
        loss = self._forward_backward(video, audio, index)
        self._guard_judge()
        if unfrozen and int(self.guard.skipped):     # the step that froze Z was skipped: the next one estimates it again
            for m in unfrozen:
                m.avg_exp_score.fill_(-1.0)
                m._z_ready = False
        return loss

    def _forward_backward(self, video, audio, index):
        if self.virtual_ranks > 1:
            return self._virtual_forward_backward(video, audio, index)
        if self.broadcast_buffers == "step":
            self.sync_buffers()
        loss = self._forward_backward_plan(video, audio, index)
        if loss is not None:
            return loss
        from . import ops
        helper = None
        if self.twt is not None:
            self.twt.prepare_wino()
            self.twt.uready = False
        if self.twt is not None and self.flat.grad.is_cuda and ops.DEFER_WGRAD and not lib.TIMING:
            # What the backward needs but the forward does not — zeroed gradients, the transposed weight copies, the
            # Winograd transforms of the weights — runs on a helper stream next to the forward instead of in front of /
            # behind it (the weights cannot change in between: this method owns the step).
            # (the helper is the weight-gradient stream, idle during the forward: a FIFTH stream would share one of
            # the runtime's four hardware queues with a busy one and serialise behind it — 4700 -> 3100 clips/s)
            # How this shares the chip with the stem convolution, the forward's first 0.87 ms, decides what it costs
            # (tools/trace_timeline.py on rocprofv3 traces, tools/host_lead.py for the phases):
            #  * issued like this, in front of the model, the gradient fill starts together with the stem kernel, whose
            #    persistent workgroups hold every CU: the fill starves until the stem ends (795 us instead of 22) and the
            #    rest follows in the ~130 us behind it — the stem pays 25 us, the side work nothing else;
            #  * anything that DELAYS the stem's start by ~25 us (a transform launch in front of it on the main stream)
            #    lets the side work win that race: it then runs inside the stem's first 100-150 us and the stem takes
            #    1.35-1.47 ms instead of 0.87 (the forward 4.8 instead of 4.25 ms) — round 3's unexplained "slower with
            #    the transforms hoisted"; a 96 MB fill or copy in front of the model does the same;
            #  * started strictly BEHIND the stem (an event behind its launch) it shares the chip with the pooling pass
            #    and conv2x instead: +0.07 ms.
            # The co-runner that does the damage is the weight transposer, not the fill (tools/corun.py: the stem alone
            # 0.87-0.97 ms; with an 85 MB fill released at the same moment or 30 us earlier 0.90-0.94; with the transposes
            # 1.38-1.44 — their tens of thousands of short 4-wave workgroups leave the stem's persistent waves unevenly
            # spread over the SIMDs, and the slowest workgroup sets the kernel's time; released 30 us later: 0.89).
            # So nothing goes in front of the model on the main stream, and the fill goes first on the helper: it starts
            # with the stem, starves, and keeps everything behind it away from the stem's start.  (Making that explicit —
            # the transposes behind an event recorded after the stem convolution — was measured too: the event's latency
            # moves them from the pooling pass into conv2x, forward 4.25 -> 4.44 ms.)
            cur, helper = ops.wgrad_stream(self.flat.grad.device)
            helper.wait_stream(cur)
            with torch.cuda.stream(helper):
                self.flat.zero_grad()
                self.twt.refresh_wino(False)
                self.twt.refresh()
                self.twt.refresh_wino(True)
        else:
            self.flat.zero_grad()
            if self.twt is not None:
                self.twt.refresh_wino(False)
        if self.twt is not None:
            with self.twt.armed_wino():
                video_emb, audio_emb = self.model(video, audio)
        else:
            video_emb, audio_emb = self.model(video, audio)
        loss, _ = self.criterion(video_emb, audio_emb, index)
        if self.twt is not None:
            if helper is not None:
                torch.cuda.current_stream().wait_stream(helper)
            else:
                self.twt.refresh()                   # after the forward: whatever the weights are now
                self.twt.refresh_wino(True)
            with self.twt.armed(), self.twt.armed_wino(), self.slots.armed(), ops.deferred_wgrads():
                loss.backward()
        else:
            loss.backward()
        self.buckets.finish()
        return loss

    def _optimizer_step_overlapped(self, pl):
        """The same update in two launches: every parameter but the video stem's three on the fourth stream, which the
        backward program made wait for exactly their gradients (plan.Plan: ``adam_early``) — it runs beside the stem's
        weight gradient, the step's last kernel — then the stem's on the compute stream.  Same arithmetic per element."""
        self.t += 1
        main, fourth = torch.cuda.current_stream(), pl.stream_objs[3]
        with torch.cuda.stream(fourth):
            self._update(0, pl.adam_early, last=False)
        main.wait_stream(fourth)
        self._update(pl.adam_early, advance=False)

    def _sampler(self):
        """The criterion's negative sampler (``nce_average.multinomial``), or None."""
        return getattr(getattr(self.criterion, "nce_average", None), "multinomial", None)

    def state_dict(self):
        sd = super().state_dict()
        mult = self._sampler()
        if mult is not None:       # the negative sampler's stream position (not part of the reference's checkpoint:
            off = int(mult.offset_dev) if getattr(mult, "offset_dev", None) is not None else int(mult.offset)
            sd["avid_sampler"] = {"seed": int(mult.seed), "offset": off}   # torch's global RNG is not saved either)
            if self.virtual_ranks > 1:               # every virtual rank's stream: its seed; all stand at one position
                sd["avid_sampler"] = {"seed": self._rank_sampler[0][0], "offset": self._rank_sampler[0][1],
                                      "seeds": [s for s, _ in self._rank_sampler]}
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        mult = self._sampler()
        if mult is not None and "avid_sampler" in sd:
            saved = sd["avid_sampler"]
            if self.virtual_ranks > 1:               # (a one-rank checkpoint: the other ranks' seeds by the per-rank formula)
                seeds = saved.get("seeds") or [int(saved["seed"]) + _RANK_SEED_STRIDE * r for r in range(self.virtual_ranks)]
                self.reseed(seeds, saved["offset"])
            else:
                mult.reseed(saved["seed"], saved["offset"])

    def step(self, video, audio, index):
        self._ema_live("step")
        self._step_plan = None
        loss = self.forward_backward(video, audio, index)
        pl = self._step_plan
        if (pl is not None and pl.adam_early and not self.buckets.comm and not lib.TIMING and self.virtual_ranks == 1
                and self.guard is None and not self._table_on):
            self._optimizer_step_overlapped(pl)
        else:
            self.optimizer_step()
        self._poll_errors()
        return loss.detach()

    # ---- whole-step hipGraph: ~600 launches replayed with one host call (kills the Python launch overhead)
    def capture(self, video, audio, index):
        """Capture one full step into a hipGraph.  Call after >= 2 eager warm-up steps (Z fixed, workspaces
        sized).  Inputs are copied into static buffers on every ``replay``."""
        if self.virtual_ranks > 1:
            raise NotImplementedError("TrainStep.capture: a hipGraph of a virtual-rank step (virtual_ranks > 1) is not supported — "
                                      "the shards' sampler streams and the deferred bank update are driven from the host")
        self._sv, self._sa, self._si = video.clone(), audio.clone(), index.clone()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        t_host = self.t
        mult = self._sampler()
        off_host = mult.offset if mult is not None else None
        # (thread-local capture mode: the NCCL process group's watchdog thread polls the events of earlier collectives with
        #  hipEventQuery — under the default global mode that call is illegal while ANY thread captures and aborts the process)
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self._sloss = self.step(self._sv, self._sa, self._si)
        if self.twt is not None:
            self.twt.frozen = True                   # (the graph holds the table's addresses: ops.prepare_wino)
        self.t = t_host                              # the capture executed nothing: host counters stay where the
        if mult is not None:                         # device counters are
            mult.offset = off_host
        return self

    def replay(self, video=None, audio=None, index=None):
        if video is not None and video.data_ptr() != self._sv.data_ptr():
            self._sv.copy_(video, non_blocking=True)
        if audio is not None and audio.data_ptr() != self._sa.data_ptr():
            self._sa.copy_(audio, non_blocking=True)
        if index is not None:
            self._si.copy_(index, non_blocking=True)
        self._ema_live("replay")
        self.graph.replay()
        self._poll_errors()
        self.t += 1
        mult = self._sampler()
        if mult is not None:
            mult.offset += 1
        return self._sloss


# ---------------------------------------------------------------------------------------------------------------------
# The reference's OWN loop (main-avid.py:155-180: model(...); criterion(...); loss.item(); optimizer.zero_grad(); loss.backward();
# optimizer.step()) on the engine's pieces: the two objects its factories build — utils/main_utils.py:112
# `DistributedDataParallel(model, device_ids=[gpu])` and :250 `torch.optim.Adam(params, lr, weight_decay, betas)` — with the same
# constructors and the same behaviour towards that loop.  Swapping the two names in main_utils.py is the whole change.
class _WrapperEngine(EngineCore):
    """The core under `DistributedDataParallel.forward` and the `loss.backward()` the caller issues later.  The optimizer is
    somebody else's, so the collectives average (``TrainStep`` folds 1 / world into its Adam launch instead) and every
    parameter carries an autograd hook for gradients that do not come out of a launch program."""

    def __init__(self, model, bucket_bytes, broadcast_buffers):
        super().__init__(model, bucket_bytes, "step" if broadcast_buffers else "off", average=True, hooks=True)
        self._armed = False
        self.buckets.on_autograd = self._arm

    def _arm(self):
        """Once per backward pass: when autograd has run every node, finish the collectives (the caller's stream waits for
        them) and give every parameter its `.grad` — torch's reducer queues the same callback (reducer.cpp: finalize_backward)."""
        if not self._armed:
            self._armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self._after_backward)

    def _after_backward(self):
        self._armed = False
        reported = list(self.buckets.reported)
        self.buckets.finish()
        self._seat_reported(reported)

    def _seat_reported(self, reported):
        """`.grad` = the flat view for every parameter whose gradient was produced this step.  A parameter nothing reported
        (frozen for this step, unused) keeps `.grad is None` if the caller's zero_grad(set_to_none=True) left it so — torch's DDP +
        optimizer then skip it, and handing it the view would hand it the previous step's gradient — unless the buffer was
        zeroed (avid_hip.parallel.Adam.zero_grad: the view is then a true zero gradient and stays seated)."""
        flat = self.flat
        if all(reported) or not any(reported):       # (launch programs report per segment: all of them; CPU / hook-less paths: none)
            flat.seat_grads()
            return
        for p, v, r in zip(flat.params, flat.grad_views, reported):
            if r:
                if p.grad is not v:
                    p.grad = v
            elif p.grad is None:
                v.zero_()                            # stale bytes must not reach an optimizer that reads the flat buffer

    def begin_step(self):
        """A new forward in training mode: whatever a failed backward pass left behind is dropped."""
        self._armed = False
        self.buckets.reset()

    def _plan_backward(self, pl, fa, inputs):
        self._arm()
        super()._plan_backward(pl, fa, inputs)


class DistributedDataParallel(torch.nn.Module):
    """`torch.nn.parallel.DistributedDataParallel(module, device_ids=[gpu])` as utils/main_utils.py:112 builds it, for one
    process per GPU: `.module`, `module.`-prefixed state_dict keys (main-avid.py:100, CheckpointManager), rank 0's parameters and
    buffers broadcast at construction, rank 0's buffers before every training forward (`broadcast_buffers=True`: ONE 78 KB
    collective), and after `loss.backward()` every `p.grad` holds the mean over ranks.  Underneath: the parameters and
    gradients are views of flat buffers, the backward launch program writes the gradients in place, the buckets' all-reduces
    (RCCL, mean) start under the rest of the backward pass on the collectives' stream — no per-parameter copy kernel in either
    direction (torch's reducer: 141 `mul_out` + 141 copies back per step, 1.1 ms of the 12.3 ms step on one rank).

    Not reproduced: `no_sync()` / gradient accumulation over several backward passes, `find_unused_parameters`, comm hooks —
    the reference uses none of them; asking for one raises."""

    def __init__(self, module, device_ids=None, output_device=None, dim=0, broadcast_buffers=True, process_group=None,
                 bucket_cap_mb=None, find_unused_parameters=False, gradient_as_bucket_view=False, **unsupported):
        super().__init__()
        if unsupported or find_unused_parameters or process_group is not None:
            raise NotImplementedError("avid_hip.parallel.DistributedDataParallel: unsupported argument(s) "
                                      f"{sorted(unsupported) or ['find_unused_parameters / process_group']}")
        if device_ids is not None and len(device_ids) != 1:
            raise ValueError("one process per GPU: device_ids must name one device")
        self.module = module
        self.device_ids = device_ids
        self.broadcast_buffers = bool(broadcast_buffers)
        cap = int((bucket_cap_mb if bucket_cap_mb is not None else 16) * (1 << 20))
        self._engine = _WrapperEngine(module, cap, self.broadcast_buffers)

    def forward(self, *inputs, **kwargs):
        if not (self.training and torch.is_grad_enabled()):
            return self.module(*inputs, **kwargs)
        from . import plan
        eng = self._engine
        eng.begin_step()
        if eng.broadcast_buffers == "step":
            eng.sync_buffers()
        with plan.engine(eng):
            return self.module(*inputs, **kwargs)

    def no_sync(self):
        raise NotImplementedError("avid_hip.parallel.DistributedDataParallel: no_sync() (gradient accumulation) is not reproduced")


class Adam(torch.optim.Optimizer):
    """`torch.optim.Adam(params, lr, betas, eps, weight_decay)` (utils/main_utils.py:250-256; L2 weight decay, no amsgrad) whose
    `step()` is ONE launch over the flat parameter / gradient / moment buffers.  A `torch.optim.Optimizer`: `param_groups`
    (MultiStepLR writes `lr` there, utils/main_utils.py:258), `state_dict()` / `load_state_dict()` in torch.optim.Adam's own
    format (`state[i] = {step, exp_avg, exp_avg_sq}`), so checkpoints written by either load into the other.

    The parameters are used where they lie if they already are the views of one flat buffer (the model went through
    `DistributedDataParallel` above or `TrainStep`), otherwise they are re-seated into one here.  One parameter group.

    Differences from torch.optim.Adam, by construction of the one-launch step: `zero_grad()` always zero-fills (set_to_none is
    accepted and ignored: `.grad` stays the view of the flat buffer), and `step()` updates EVERY parameter of the buffer — one
    that received no gradient this step is stepped with a zero gradient (its moments decay, L2 weight decay still applies),
    where torch.optim.Adam would skip a parameter whose `.grad` is None.  The reference freezes nothing (main-avid.py:106)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **unsupported):
        if amsgrad or any(unsupported.get(k) for k in ("maximize", "capturable", "differentiable")):
            raise NotImplementedError("avid_hip.parallel.Adam: amsgrad / maximize / capturable / differentiable")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False))
        if len(self.param_groups) != 1:
            raise NotImplementedError("avid_hip.parallel.Adam: one parameter group")
        ps = self.param_groups[0]["params"]
        self.flat = flat_of(ps)
        if self.flat is None:
            # Some of them may already BE views of a live flat buffer (the model went through DistributedDataParallel / TrainStep)
            # while the list is not exactly that buffer's set (extra trainable criterion parameters, a subset): re-seating them
            # into a second buffer here would orphan the first — the launch programs and collectives would keep writing the
            # engine's gradient buffer while this optimizer read its own zeros: a silent no-learning failure.
            owned = [p for p in ps if _FLAT_OF.get(id(p)) is not None and _FLAT_OF[id(p)]() is not None]
            if owned:
                raise ValueError("avid_hip.parallel.Adam: %d of the %d parameters already live in a flat buffer (DistributedDataParallel / "
                                 "TrainStep) but the list is not exactly that buffer's parameter set (or they were moved after it was built); "
                                 "pass exactly the wrapped model's parameters, or use torch.optim.Adam for a different set" % (len(owned), len(ps)))
            self.flat = FlatParams(ps)
        self.m = torch.zeros_like(self.flat.flat)
        self.v = torch.zeros_like(self.flat.flat)
        self._t = 0
        self._step_t = torch.tensor(0.0)

    def _publish_state(self):
        """`self.state` in torch.optim.Adam's shape: views of the flat moments, one shared step tensor."""
        if self.state:
            return
        for i, p in enumerate(self.flat.params):
            self.state[p] = {"step": self._step_t, "exp_avg": self.flat.view(self.m, i), "exp_avg_sq": self.flat.view(self.v, i)}

    def zero_grad(self, set_to_none=True):
        """One fill of the flat gradient buffer; `.grad` stays seated (a launch program writes the buffer, not the attribute)."""
        self.flat.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import ops
        g = self.param_groups[0]
        p0 = self.flat.params[0]
        if p0.data_ptr() != self.flat.flat.data_ptr() + 4 * self.flat.offsets[0]:
            raise RuntimeError("avid_hip.parallel.Adam: the parameters were moved after the optimizer was built (model.cuda() / a "
                               "wrapper constructed later): build the optimizer last, as main-avid.py:95-108 does")
        self.flat.seat_grads()
        self._t += 1
        self._step_t.fill_(float(self._t))
        ops.adam_flat(self.flat.flat, self.flat.grad, self.m, self.v, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                      g["weight_decay"], self._t)
        self._publish_state()
        return loss

    def state_dict(self):
        if self._t > 0:
            self._publish_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)              # (torch: casts, re-keys by parameter, replaces self.state)
        self._t = step = self.flat.load_moments(self.m, self.v, ((i, self.state.get(p)) for i, p in enumerate(self.flat.params)))
        self._step_t = torch.tensor(float(step))
        self.state.clear()
        if step > 0:
            self._publish_state()


class SGD(torch.optim.Optimizer):
    """`torch.optim.SGD(params, lr, momentum, weight_decay, nesterov)` (utils/main_utils.py:242-248; L2 weight decay, dampening 0)
    whose `step()` is ONE launch over the flat parameter / gradient / momentum buffers.  A `torch.optim.Optimizer`: `param_groups`
    (MultiStepLR writes `lr` there, utils/main_utils.py:261), `state_dict()` / `load_state_dict()` in torch.optim.SGD's own format
    (`state[i] = {momentum_buffer}`, nothing without momentum), so checkpoints written by either load into the other.

    The parameters are used where they lie if they already are the views of one flat buffer (the model went through
    `DistributedDataParallel` above or `TrainStep`), otherwise they are re-seated into one here.  One parameter group.

    Differences from torch.optim.SGD, by construction of the one-launch step: `zero_grad()` always zero-fills (set_to_none is
    accepted and ignored: `.grad` stays the view of the flat buffer), and `step()` updates EVERY parameter of the buffer — one
    that received no gradient this step is stepped with a zero gradient (its momentum buffer decays and still moves it, L2
    weight decay still applies), where torch.optim.SGD would skip a parameter whose `.grad` is None.  The reference freezes
    nothing (main-avid.py:106)."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kw):
        if dampening != 0 or kw.get("maximize") or kw.get("differentiable"):
            raise NotImplementedError("avid_hip.parallel.SGD: dampening / maximize / differentiable")
        params = list(params)
        # torch's own constructor checks the values (ValueError: Nesterov momentum requires a momentum) and names the keys
        # this torch's SGD writes into a parameter group
        defaults = dict(torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov, **kw).defaults)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError("avid_hip.parallel.SGD: one parameter group")
        ps = self.param_groups[0]["params"]
        self.flat = flat_of(ps)
        if self.flat is None:
            # (see Adam above: a second flat buffer over parameters that live in an engine's would orphan the engine's)
            owned = [p for p in ps if _FLAT_OF.get(id(p)) is not None and _FLAT_OF[id(p)]() is not None]
            if owned:
                raise ValueError("avid_hip.parallel.SGD: %d of the %d parameters already live in a flat buffer (DistributedDataParallel / "
                                 "TrainStep) but the list is not exactly that buffer's parameter set (or they were moved after it was built); "
                                 "pass exactly the wrapped model's parameters, or use torch.optim.SGD for a different set" % (len(owned), len(ps)))
            self.flat = FlatParams(ps)
        self.buf = None                                  # the flat momentum buffer: made when a step or a checkpoint needs it

    def _buffer(self):
        if self.buf is None:
            self.buf = torch.zeros_like(self.flat.flat)
        return self.buf

    def _publish_state(self):
        """`self.state` in torch.optim.SGD's shape: views of the flat momentum buffer."""
        if self.state or self.buf is None:
            return
        for i, p in enumerate(self.flat.params):
            self.state[p] = {"momentum_buffer": self.flat.view(self.buf, i)}

    def zero_grad(self, set_to_none=True):
        """One fill of the flat gradient buffer; `.grad` stays seated (a launch program writes the buffer, not the attribute)."""
        self.flat.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import ops
        g = self.param_groups[0]
        p0 = self.flat.params[0]
        if p0.data_ptr() != self.flat.flat.data_ptr() + 4 * self.flat.offsets[0]:
            raise RuntimeError("avid_hip.parallel.SGD: the parameters were moved after the optimizer was built (model.cuda() / a "
                               "wrapper constructed later): build the optimizer last, as main-avid.py:95-108 does")
        self.flat.seat_grads()
        ops.sgd_flat(self.flat.flat, self.flat.grad, self._buffer() if g["momentum"] != 0 else None, g["lr"], g["momentum"],
                     g["weight_decay"], g["nesterov"])
        if g["momentum"] != 0:
            self._publish_state()
        return loss

    def load_state_dict(self, state_dict):
        _require_format("avid_hip.parallel.SGD", state_dict, "SGD")
        super().load_state_dict(state_dict)              # (torch: casts, re-keys by parameter, replaces self.state)
        found = self.flat.load_momentum(self._buffer(), ((i, self.state.get(p)) for i, p in enumerate(self.flat.params)))
        self.state.clear()
        if found:
            self._publish_state()


# ---------------------------------------------------------------------------------------------------------------------
# Inference: an eval-mode forward as one launch program
# ---------------------------------------------------------------------------------------------------------------------
class Inference:
    """``Inference(model)(*inputs)`` returns what ``model.eval()(*inputs)`` returns under ``torch.no_grad()`` — a tensor for
    ``R2Plus1D``, ``Conv2D`` and ``ClassificationWrapper``, the tuple of embeddings for ``AV_Wrapper``, the dict of logits for
    ``MOSTModel``, whatever the model returns otherwise —
    bit for bit, without touching the modules' ``training`` flags and without synchronising the host.

    Models the inference compiler knows (``plan.EvalPlan``: the towers, and the two wrappers around either tower — clips
    [B, 3, T, H, W] for ``R2Plus1D``, spectrograms [B, 1, T, F] for ``Conv2D``) run as ONE launch program per input geometry: the eval-mode
    BatchNorms' coefficients from one launch, conv2x's BatchNorms inside the temporal convolutions, the stem's tail in one
    pass, activations in a recycled arena.  Anything else — hooks on a module, frozen BatchNorm parameters, another model,
    CPU or non-fp32 tensors, a stream capture, ``AVID_EVAL_PLAN=0`` — takes the per-layer path.  ``used_programs`` says which
    path the last call took.  ``model(x)`` in eval mode is not affected: the programs are reached through this class (and the
    step engines' ``evaluate``) only."""

    def __init__(self, model):
        self.model = model
        self.used_programs = None

    def __call__(self, *inputs):
        from . import plan
        out = plan.run_eval(self.model, *inputs)
        self.used_programs = out is not None
        return out if out is not None else self._per_layer(*inputs)

    def _per_layer(self, *inputs):
        mods = [m for m in self.model.modules() if m.training]
        for m in mods:
            m.training = False
        try:
            with torch.no_grad():
                return self.model(*inputs)
        finally:
            for m in mods:
                m.training = True


# ---------------------------------------------------------------------------------------------------------------------
# k-nearest-neighbour / retrieval evaluation of a frozen tower
# ---------------------------------------------------------------------------------------------------------------------
class KNNEval:
    """Weighted k-NN classification and retrieval recall over the embeddings of a frozen tower, without training anything:
    embed a labelled gallery, then classify each query by the vote of its ``k`` nearest gallery embeddings, every neighbour
    weighing ``exp(similarity / T)`` (``ops.knn_search`` / ``ops.knn_vote``; no ``[Q, N]`` matrix is ever held).

    ``model``: anything ``Inference`` runs — ``R2Plus1D`` (its ``pool`` output, flattened to ``[B, 512]``), ``Conv2D`` (the audio
    tower: the same on spectrograms ``[B * clips_per_sample, 1, T, F]``, a sample's clips adjacent — the flat form only; nothing
    here is specific to it, the forward is ``Inference``'s inference program), ``AV_Wrapper`` (the video embedding; pass ``(video, audio)`` where a clip batch is
    expected) — or ``None`` to work on features the caller extracted.  The forward is ``Inference(model)``'s and nothing else: frozen towers, hooks and so on take whatever path it
    takes.  ``feat``: only ``"pool"``, the tower's output.  ``normalize``: L2-normalise the (clip-averaged) features, so that
    the similarity is the cosine.  The feature width must be a multiple of 32, the gallery needs 64 rows, ``k <= 63``.

    Clips arrive as ``[B * clips_per_sample, 3, T, H, W]`` in the reference's ``test_dense`` order (a sample's clips are
    adjacent) or as ``[B, clips_per_sample, 3, T, H, W]``; a sample's clip features are averaged before the normalisation
    (``view(B, clips, -1).mean(1)``).  Labels: integer ``[B]`` on the device, in ``[0, n_classes)``.

    ``evaluate`` returns integer counts as device tensors and never synchronises.  Nothing here is distributed: with several
    ranks the caller builds the same gallery on every rank, gives each rank its share of the queries and all-reduces the counts."""

    def __init__(self, model=None, feat="pool", k=20, T=0.07, n_classes=None, normalize=True):
        if feat != "pool":
            raise ValueError(f"KNNEval: feat must be 'pool' (got {feat!r})")
        if n_classes is None or int(n_classes) < 1:
            raise ValueError("KNNEval: n_classes is required")
        if not 1 <= int(k) <= 63:
            raise ValueError(f"KNNEval: k must be in [1, 63] (got {k})")
        self.model, self.k, self.T, self.n_classes, self.normalize = model, int(k), float(T), int(n_classes), bool(normalize)
        self._infer = Inference(model) if model is not None else None
        self._chunks, self._gallery = [], None

    # ---- features
    def _labels(self, labels, n):
        if labels.is_floating_point() or labels.dtype == torch.bool or tuple(labels.shape) != (n,):
            raise ValueError(f"KNNEval: labels must be an integer tensor [{n}] (got {labels.dtype} {tuple(labels.shape)})")
        return labels.to(torch.int32).contiguous()

    def _pooled(self, feats, clips):
        """[B * clips, D] clip features -> [B, D]: the clips' mean, then the normalisation."""
        from . import ops
        feats = feats.flatten(1).float()
        if clips > 1:
            if feats.shape[0] % clips:
                raise ValueError(f"KNNEval: {feats.shape[0]} clips are not a multiple of clips_per_sample = {clips}")
            feats = feats.view(feats.shape[0] // clips, clips, -1).mean(1)
        feats = feats.contiguous()
        return ops.l2_normalize(feats) if self.normalize else feats

    def _embed(self, video, clips):
        if self._infer is None:
            raise ValueError("KNNEval was built without a model: pass features")
        inputs = tuple(video) if isinstance(video, (tuple, list)) else (video,)
        inputs = tuple((x.flatten(0, 1) if x.dim() == 6 else x).contiguous() for x in inputs)
        with torch.no_grad():
            out = self._infer(*inputs)
            if isinstance(out, (tuple, list)):
                out = out[0]
            return self._pooled(out, clips)

    def _features(self, x, clips):
        if isinstance(x, torch.Tensor) and x.dim() == 2:
            with torch.no_grad():
                return self._pooled(x, clips)
        return self._embed(x, clips)

    # ---- gallery
    def add_gallery(self, video, labels, clips_per_sample=1):
        """Embed a batch of gallery clips (``Inference(model)``) and keep the features and labels on the device."""
        feats = self._embed(video, int(clips_per_sample))
        self._chunks.append((feats, self._labels(labels, feats.shape[0])))
        self._gallery = None

    def add_gallery_features(self, feats, labels):
        """Add features ``[B, D]`` the caller extracted (one row per sample)."""
        if feats.dim() != 2:
            raise ValueError("KNNEval.add_gallery_features: feats must be [B, D]")
        with torch.no_grad():
            feats = self._pooled(feats, 1)
        self._chunks.append((feats, self._labels(labels, feats.shape[0])))
        self._gallery = None

    def gallery(self):
        """``(features [N, D], labels int32 [N])``: the chunks, concatenated once."""
        if self._gallery is None:
            if not self._chunks:
                raise ValueError("KNNEval: the gallery is empty")
            self._gallery = (torch.cat([f for f, _ in self._chunks], 0).contiguous(), torch.cat([l for _, l in self._chunks], 0))
            self._chunks = [self._gallery]
        return self._gallery

    # ---- evaluation
    def evaluate(self, video_or_features=None, labels=None, clips_per_sample=1, recall_at=(1, 5, 10, 20, 50), leave_one_out=False):
        """k-NN top-1 / top-5 and retrieval recall of a batch of queries (clips, or features ``[B * clips, D]``) against the
        gallery.  Returns ``{"n", "top1_hits", "top5_hits", "recall_hits": {r: ...}}``: int64 device scalars — counts, so that
        batches and ranks add up; accuracy = hits / n.  ``recall_hits[r]`` (for every ``r <= k`` of ``recall_at``) counts the
        queries with a gallery row of their own label among the ``r`` nearest.  ``leave_one_out=True`` takes no queries: every
        gallery row is evaluated against the others."""
        from . import ops
        gal, gal_labels = self.gallery()
        if leave_one_out:
            if video_or_features is not None or labels is not None:
                raise ValueError("KNNEval.evaluate: leave_one_out evaluates the gallery itself, pass no queries")
            q, q_labels = gal, gal_labels
            exclude = torch.arange(gal.shape[0], dtype=torch.int32, device=gal.device)
        else:
            q = self._features(video_or_features, int(clips_per_sample))
            q_labels, exclude = self._labels(labels, q.shape[0]), None
        idx, sim = ops.knn_search(gal, q, self.k, exclude=exclude)
        _, pred5, first = ops.knn_vote(idx, sim, gal_labels, self.n_classes, T=self.T, query_labels=q_labels)
        return {"n": torch.full((), q.shape[0], dtype=torch.int64, device=q.device),
                "top1_hits": (pred5[:, 0] == q_labels).sum(),
                "top5_hits": (pred5 == q_labels[:, None]).any(1).sum(),
                "recall_hits": {int(r): (first < int(r)).sum() for r in recall_at if int(r) <= self.k}}


# ---------------------------------------------------------------------------------------------------------------------
# Multi-label evaluation: the numbers tagging sets (AudioSet, Charades) are reported in
# ---------------------------------------------------------------------------------------------------------------------
class MultiLabelEval:
    """Accumulates the confidences of a multi-label evaluation — what ``FinetuneStep(loss="bce").evaluate`` returns per batch —
    and computes mAP, mean ROC-AUC and d' over the whole set on the device (``ops.rank_metrics``: scikit-learn's
    ``average_precision_score`` / ``roc_auc_score`` per class, ties handled, no sort, no ``[N, C]`` copy to the host).

    ``add(conf, targets)``: ``[n, n_classes]`` each, on one device; float32 confidences, targets float32 / bool / uint8
    (positive iff >= 0.5).  The tensors are kept as they are; nothing is launched and nothing synchronises.
    ``compute()`` returns device tensors: ``ap`` / ``auc`` float64 [C] (NaN where undefined: a class without positives, for
    ``auc`` also one without negatives), ``n_pos`` int64 [C], and over the classes with a defined value ``mAP``, ``mAUC``,
    ``d_prime`` = sqrt(2) * ndtri(mAUC) (float64 scalars) and ``n_valid`` (int64 [2]: classes behind mAP, behind mAUC).
    Nothing here is distributed: with several ranks the caller gathers the confidences first."""

    def __init__(self, n_classes):
        if int(n_classes) < 1:
            raise ValueError("MultiLabelEval: n_classes must be >= 1")
        self.n_classes = int(n_classes)
        self._chunks = []

    def add(self, conf, targets):
        shape = (conf.shape[0] if conf.dim() == 2 else -1, self.n_classes)
        if (conf.dim() != 2 or tuple(conf.shape) != shape or tuple(targets.shape) != shape or conf.dtype != torch.float32
                or targets.dtype not in (torch.float32, torch.bool, torch.uint8) or conf.device != targets.device
                or not conf.is_cuda or conf.shape[0] < 1):
            raise ValueError(f"MultiLabelEval.add: conf float32 [n, {self.n_classes}] and targets float32 / bool / uint8 of the "
                             f"same shape on one HIP device expected (got {conf.dtype} {tuple(conf.shape)} on {conf.device}, "
                             f"{targets.dtype} {tuple(targets.shape)} on {targets.device})")
        if self._chunks and self._chunks[0][0].device != conf.device:
            raise ValueError("MultiLabelEval.add: every chunk must be on the same device")
        self._chunks.append((conf.detach(), targets.detach()))

    def reset(self):
        self._chunks = []

    def compute(self):
        from . import ops
        if not self._chunks:
            raise ValueError("MultiLabelEval.compute: nothing was added")
        conf = torch.cat([c for c, _ in self._chunks], 0).contiguous()
        targets = torch.cat([t.to(torch.float32) for _, t in self._chunks], 0).contiguous()
        self._chunks = [(conf, targets)]
        ap, auc, n_pos = ops.rank_metrics(conf, targets)
        ok_ap, ok_auc = ~torch.isnan(ap), ~torch.isnan(auc)
        zero = torch.zeros((), dtype=torch.float64, device=ap.device)
        # (the mean over no class is NaN: 0 / 0)
        m_ap = torch.where(ok_ap, ap, zero).sum() / ok_ap.sum()
        m_auc = torch.where(ok_auc, auc, zero).sum() / ok_auc.sum()
        return {"ap": ap, "auc": auc, "n_pos": n_pos, "mAP": m_ap, "mAUC": m_auc,
                "d_prime": math.sqrt(2.0) * torch.special.ndtri(m_auc), "n_valid": torch.stack([ok_ap.sum(), ok_auc.sum()])}


# ---------------------------------------------------------------------------------------------------------------------
# Linear SVM evaluation of frozen features: the sound-classification protocol (ESC-50, DCASE) of the paper, L3 and XDC
# ---------------------------------------------------------------------------------------------------------------------
class SVMEval:
    """A linear one-vs-all SVM (``ops.svm_fit``: liblinear's L2-regularised L2-loss primal) trained on the frozen features of
    a tower, clip predictions averaged per sample — on the device from the embedding to the counts.

    ``model``: anything ``Inference`` runs — ``R2Plus1D`` / ``Conv2D`` (the output, flattened to ``[rows, F]``), ``AV_Wrapper``
    (the first embedding; pass ``(video, audio)`` where a clip batch is expected) — or ``None`` to work on features ``[rows, F]``
    the caller extracted (``MOSTModel``'s pooled taps, say).  A 2-D tensor is always taken as features.

    Training rows are clip-level, as in the protocol: ``add_train(clips, labels, clips_per_sample)`` takes
    ``[B * clips_per_sample, ...]`` (a sample's clips adjacent; video also as ``[B, clips_per_sample, 3, T, H, W]``,
    spectrograms ``[B * clips_per_sample, 1, T, F]`` in the flat form only, as for ``KNNEval``) and integer labels ``[B]`` on
    the device, which are repeated per clip.  ``fit()`` standardises its own copy of the features with the training rows'
    per-feature mean and (biased) standard deviation when ``standardize`` is set (a constant feature is left unscaled),
    after the per-row L2 normalisation when ``normalize`` is set, and solves.  ``decision_function`` returns the clip scores
    ``[rows, n_classes]``; ``evaluate`` averages a sample's clip scores (``view(B, clips, C).mean(1)``) and returns
    ``{"n", "top1_hits", "top5_hits"}`` as int64 device scalars — counts, so that batches and ranks add up.
    ``info`` is ``ops.svm_fit``'s.  Nothing here is distributed."""

    def __init__(self, model=None, n_classes=None, cost=1.0, standardize=True, normalize=False, tol=1e-4, pos_weight=None,
                 intercept_scaling=1.0, max_iter=100):
        if n_classes is None or int(n_classes) < 1:
            raise ValueError("SVMEval: n_classes is required")
        self.model, self.n_classes, self.cost, self.tol = model, int(n_classes), float(cost), float(tol)
        self.standardize, self.normalize = bool(standardize), bool(normalize)
        self.pos_weight, self.intercept_scaling, self.max_iter = pos_weight, float(intercept_scaling), int(max_iter)
        self._infer = Inference(model) if model is not None else None
        self._chunks = []
        self.coef = self.intercept = self.mean = self.std = self.info = None

    # ---- features
    def _features(self, x):
        """Clip-level features [rows, F], fp32 contiguous (L2-normalised per row when ``normalize``)."""
        from . import ops
        with torch.no_grad():
            if not (isinstance(x, torch.Tensor) and x.dim() == 2):
                if self._infer is None:
                    raise ValueError("SVMEval was built without a model: pass features [rows, F]")
                inputs = tuple(x) if isinstance(x, (tuple, list)) else (x,)
                inputs = tuple((t.flatten(0, 1) if t.dim() == 6 else t).contiguous() for t in inputs)
                x = self._infer(*inputs)
                if isinstance(x, (tuple, list)):
                    x = x[0]
            x = x.flatten(1).float().contiguous()
            return ops.l2_normalize(x) if self.normalize else x

    def _labels(self, labels, n):
        if labels.is_floating_point() or labels.dtype == torch.bool or tuple(labels.shape) != (n,):
            raise ValueError(f"SVMEval: labels must be an integer tensor [{n}] (got {labels.dtype} {tuple(labels.shape)})")
        return labels.to(torch.int64)

    def _samples(self, rows, clips):
        if clips < 1 or rows % clips:
            raise ValueError(f"SVMEval: {rows} rows are not a multiple of clips_per_sample = {clips}")
        return rows // clips

    # ---- training
    def add_train(self, clips_or_features, labels, clips_per_sample=1):
        """Embed a batch of training clips (or take features ``[rows, F]``) and keep the rows and their labels on the device."""
        feats = self._features(clips_or_features)
        clips = int(clips_per_sample)
        labels = self._labels(labels, self._samples(feats.shape[0], clips))
        self._chunks.append((feats, labels.repeat_interleave(clips) if clips > 1 else labels))

    def fit(self, init=None):
        """Train on everything added so far; returns ``self``.  ``init=(coef, intercept)`` warm-starts (a sweep over ``cost``)."""
        from . import ops
        if not self._chunks:
            raise ValueError("SVMEval.fit: no training rows")
        with torch.no_grad():
            X = torch.cat([f for f, _ in self._chunks], 0)
            y = torch.cat([l for _, l in self._chunks], 0)
            self._chunks = [(X, y)]
            if self.standardize:
                self.mean = X.mean(0)
                std = X.std(0, unbiased=False)
                self.std = torch.where(std > 0, std, torch.ones_like(std))
            else:
                self.mean = self.std = None
            self.coef, self.intercept, self.info = ops.svm_fit(
                self._scaled(X), y, self.n_classes, cost=self.cost, pos_weight=self.pos_weight,
                intercept_scaling=self.intercept_scaling, tol=self.tol, max_iter=self.max_iter, init=init)
        return self

    def _scaled(self, feats):
        return feats if self.mean is None else ((feats - self.mean) / self.std).contiguous()

    # ---- prediction
    def decision_function(self, clips_or_features):
        """Clip scores ``[rows, n_classes]`` (``ops.svm_scores`` on the standardised features)."""
        from . import ops
        if self.coef is None:
            raise ValueError("SVMEval: fit() or load_state_dict() first")
        with torch.no_grad():
            return ops.svm_scores(self._scaled(self._features(clips_or_features)), self.coef, self.intercept)

    def evaluate(self, clips_or_features, labels, clips_per_sample=1):
        scores = self.decision_function(clips_or_features)
        clips = int(clips_per_sample)
        B = self._samples(scores.shape[0], clips)
        labels = self._labels(labels, B)
        scores = scores.view(B, clips, self.n_classes).mean(1)
        top5 = scores.topk(min(5, self.n_classes), dim=1).indices
        return {"n": torch.full((), B, dtype=torch.int64, device=scores.device),
                "top1_hits": (scores.argmax(1) == labels).sum(),
                "top5_hits": (top5 == labels[:, None]).any(1).sum()}

    # ---- persistence
    def state_dict(self):
        if self.coef is None:
            raise ValueError("SVMEval: fit() first")
        sd = {"coef": self.coef, "intercept": self.intercept}
        if self.mean is not None:
            sd["mean"], sd["std"] = self.mean, self.std
        return sd

    def load_state_dict(self, sd):
        coef, intercept = sd["coef"], sd["intercept"]
        if coef.dim() != 2 or coef.shape[0] != self.n_classes or tuple(intercept.shape) != (self.n_classes,):
            raise ValueError(f"SVMEval.load_state_dict: coef {tuple(coef.shape)} / intercept {tuple(intercept.shape)} do not "
                             f"fit {self.n_classes} classes")
        if ("mean" in sd) != ("std" in sd) or ("mean" in sd) != self.standardize:
            raise ValueError("SVMEval.load_state_dict: mean and std come together, exactly when standardize is set")
        self.coef, self.intercept = coef.float().contiguous(), intercept.float().contiguous()
        self.mean = sd["mean"].float().contiguous() if "mean" in sd else None
        self.std = sd["std"].float().contiguous() if "std" in sd else None


# ---------------------------------------------------------------------------------------------------------------------
# Action-recognition fine-tuning (eval-action-recg.py: run_phase 'train' / 'test_dense', the warm-up epochs of the classifier)
# ---------------------------------------------------------------------------------------------------------------------
class FinetuneStep(AdamStep):
    """One fine-tuning step of a ``models.ClassificationWrapper`` around this package's ``R2Plus1D`` on this rank's GPU:
    the forward launch program ends in ``avid_cls_loss`` (loss, top-1 / top-5 hits and ``dlogits`` on the device), the
    backward program starts from ``dlogits``, then one flat Adam launch (``torch.optim.Adam``'s update; lr 1e-4 and weight
    decay 0 as the shipped benchmark configs).  Nothing synchronises the host.

    ``classifier_only=True``: the reference's warm-up (an optimizer over the classifier's parameters only).  The tower
    still runs in training mode and updates its BatchNorm running statistics; no tower backward is compiled, because the
    reference never applies those gradients; Adam touches only the classifier's slice of the flat buffer.
    The tower may also be this package's ``Conv2D`` (sound classification): ``step`` and ``evaluate`` then take spectrograms
    [B, 1, T, F] / [V, clips, 1, T, F] where they take clips; optimizers, the step guard, checkpoints and ``virtual_ranks`` alike.
    With more than one rank, gradients are averaged as DistributedDataParallel does: through ``GradBuckets`` (the full
    step), or one collective over the classifier's slice (``classifier_only``); Adam's ``grad_scale`` takes the 1 / world.
    Rank 0's BatchNorm running statistics are broadcast before every step (``broadcast_buffers="step"``, DDP's default).
    ``set_lr`` and ``state_dict`` / ``load_state_dict`` (torch.optim.Adam's format) are ``AdamStep``'s, shared with ``TrainStep``.

    ``virtual_ranks`` = R > 1: the step of an R-replica job — the shipped fine-tuning configs are eight-GPU ``nn.DataParallel``
    jobs of batch 64 — on this one GPU.  ``step`` takes the GLOBAL batch [R * b, ...] and runs it shard after shard through one
    ``ClsPlan`` of the shard geometry (``AdamStep._virtual_pass``): every BatchNorm normalises with its replica's b clips,
    every replica draws its own dropout mask (``dropout_seeds``), the flat gradient buffer ends up holding the replicas' sum in
    rank order, the optimizer takes it with 1 / R — the gradient of the cross-entropy over the gathered R * b logits, and the
    all-reduced mean of an R-rank DistributedDataParallel job — the running statistics left are replica 0's.  ``rank_losses``
    [R] / ``rank_hits`` [R, 2] hold every replica's own (None before the first such step).  One process,
    ``broadcast_buffers="step"``, the compiled programs only; ``virtual_ranks`` is not part of a checkpoint."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, classifier_only=False,
                 bucket_bytes=16 << 20, broadcast_buffers="step", optimizer="adam", momentum=0.0, nesterov=False,
                 max_grad_norm=None, skip_nonfinite=False, virtual_ranks=1, loss="ce", pos_weight=None, label_smoothing=0.0,
                 ema_decay=None, ema_warmup=False, ema_buffers=True, param_rules=None, trust_coefficient=0.001):
        """``loss``: ``"ce"`` (default), ``"soft_ce"`` or ``"bce"``.  ``"soft_ce"``: softmax cross-entropy against a distribution
        (mixup / CutMix targets from ``datasets.gpu_mix.GpuBatchMix``, a teacher's probabilities) with ``label_smoothing`` in
        [0, 1): ``step(x, targets)`` takes float32 targets [B, C], ``step(x, labels)`` int64 labels [B] (made one-hot on the
        device, so smoothing alone works with ordinary labels); the forward program ends in ``avid_soft_ce_loss``, ``hits`` are
        top-1 / top-5 against the argmax of each target row; ``evaluate`` is never smoothed (int64 labels: ``avid_cls_loss``,
        float32 targets: ``avid_soft_ce_loss``).  ``"bce"`` — multi-label fine-tuning: ``step(x, targets)`` takes float32 targets [B, C]
        in [0, 1] (bool / uint8 are converted), the forward program ends in ``avid_mlabel_loss`` (``pos_weight``: [C], optional),
        ``hits`` are (videos whose highest-confidence class is positive, (video, class) pairs on the right side of 0.5), and
        ``evaluate`` returns the clip-mean sigmoid as its confidence; everything else as for ``"ce"``.
        ``broadcast_buffers``: as ``TrainStep``'s — ``"step"`` (default, DistributedDataParallel's behaviour) broadcasts rank
        0's BatchNorm running statistics before every step, ``"lazy"`` only at ``sync_buffers()``, ``"off"`` never.
        ``optimizer`` / ``momentum`` / ``nesterov``, ``max_grad_norm`` / ``skip_nonfinite`` (the step guard; it judges the slice
        the optimizer updates — with ``virtual_ranks`` the accumulated gradient, a skipped step puts back the running
        statistics from before shard 0's forward): see ``AdamStep``.  ``virtual_ranks``: see the class."""
        R = _virtual_ranks_arg("FinetuneStep", virtual_ranks, broadcast_buffers)
        super().__init__(model, lr, betas, eps, weight_decay, optimizer=optimizer, momentum=momentum, nesterov=nesterov,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup,
                         ema_buffers=ema_buffers, param_rules=param_rules, trust_coefficient=trust_coefficient,
                         bucket_bytes=bucket_bytes, broadcast_buffers=broadcast_buffers)
        self.classifier_only = bool(classifier_only)
        self.n_cls = self.flat.offsets[2] if len(self.flat.params) > 2 else self.flat.numel   # (reverse order: classifier bias, weight first)
        self._set_loss(loss, pos_weight, lambda: model.classifier.weight.shape[0], label_smoothing)
        self.virtual_ranks = R
        self.rank_losses = self.rank_hits = None     # [R] float32 / [R, 2] int64 device tensors of the last virtual-rank step
        self._dropout_seeds = None                   # reseed_dropout()'s, while the model's own seed is still the first of them

    @property
    def dropout_seeds(self):
        """The seed of every (virtual) rank's dropout stream, or None for a model without dropout: rank 0's is the model's own
        (``model.dropout.seed``), rank r's follows by the per-rank formula of the negative samplers unless ``reseed_dropout``
        set it.  All ranks stand at one offset, ``model.dropout.offset``."""
        drop = getattr(self.model, "dropout", None)
        if not hasattr(drop, "seed"):
            return None
        base = int(drop.seed) & _U64
        if self._dropout_seeds is not None and self._dropout_seeds[0] == base:
            return list(self._dropout_seeds)
        return [(base + _RANK_SEED_STRIDE * r) & _U64 for r in range(self.virtual_ranks)]

    def reseed_dropout(self, seeds, offset=None):
        """Set the seed of every (virtual) rank's dropout stream, and with ``offset`` the position all of them are at."""
        seeds = [int(s) & _U64 for s in seeds]
        if len(seeds) != self.virtual_ranks:
            raise ValueError(f"FinetuneStep.reseed_dropout: {self.virtual_ranks} seed(s) expected, one per virtual rank "
                             f"(got {len(seeds)})")
        drop = getattr(self.model, "dropout", None)
        if not hasattr(drop, "seed"):
            raise ValueError("FinetuneStep.reseed_dropout: the model has no dropout")
        drop.seed = seeds[0]
        if offset is not None:
            drop.offset = int(offset)
        self._dropout_seeds = seeds

    def _plan(self, video):
        from . import plan
        pl = plan.cls_plan(self.model, video, self.classifier_only, need_grad=False, loss=self.loss, pos_weight=self.pos_weight,
                           label_smoothing=self.label_smoothing)
        if pl is None or plan._engine_flat(self, pl) is None:
            raise NotImplementedError("FinetuneStep: the model is outside the compiled fine-tuning programs (plan.ClsPlan: "
                                      "ClassificationWrapper(R2Plus1D, feat_name='pool', pooling_op=None), fp32 CUDA "
                                      "parameters, training mode, no hooks)")
        return pl

    def step(self, video, labels):
        """(loss [], hits [2] int64: top-1 / top-5 hits of the batch) as device tensors.  ``virtual_ranks`` > 1: the mean of the
        ranks' losses and the sum of their hits, over the global batch [R * b, ...]."""
        self._ema_live("step")
        if self.virtual_ranks > 1:
            return self._virtual_step(video, labels)
        video, labels = self._labelled(video, labels)
        B = video.shape[0]
        if self.broadcast_buffers == "step":
            self.sync_buffers()
        pl = self._plan(video)
        if self.guard is not None:
            self._guard_begin()
        drop = self.model.dropout if pl.drop_index is not None else None
        seed, offset = (drop.seed, drop.next_offset()) if drop is not None else (0, 0)
        out = torch.empty(8, dtype=torch.float32, device=video.device)          # plan.OUT_BYTES
        dlogits = torch.empty((B, pl.n_classes), dtype=torch.float32, device=video.device)
        _, fa = pl.forward(video, self.flat.grad, True, seed, offset, labels=labels, out=out, dlogits=dlogits)
        inputs = (video, None, dlogits, None)
        if self.buckets.comm and self.classifier_only:
            # only the classifier's leading slice of the gradient buffer is written (and zeroed): ONE collective over it,
            # behind the backward program (whose streams all join the current one), instead of the buckets over the tower
            pl.backward(fa, inputs, self.flat.grad)
            dist.all_reduce(self.flat.grad[:self.n_cls])
        else:
            self._plan_backward(pl, fa, inputs)
            if self.buckets.comm:
                self.buckets.finish()
        self.t += 1
        end = self.n_cls if self.classifier_only else self.flat.numel
        if self.guard is not None:
            self._guard_judge(0, end)
        self._update(0, end)
        self._poll_errors()
        return out[0], out[2:6].view(torch.int64)

    def _virtual_step(self, video, labels):
        """The step of ``virtual_ranks`` replicas (see the class): per shard the forward program with that replica's dropout
        seed, ``avid_cls_loss`` over its b logits (mean over b) and the backward program; then ONE guard and optimizer pass over
        the accumulated slice — all parameters, or the classifier's [:n_cls] (``classifier_only``: the tower's slice of the
        gradient buffer and of the accumulator is neither written nor read)."""
        b, shards = self._virtual_shards(video, labels)
        pl = self._plan(shards[0][0])
        if self.guard is not None:
            self._guard_begin()                      # (the snapshot a skipped step is put back from: before shard 0's forward)
        drop = self.model.dropout if pl.drop_index is not None else None
        seeds, offset = (self.dropout_seeds, drop.next_offset()) if drop is not None else ([0] * len(shards), 0)
        dev = video.device
        out = torch.empty((len(shards), 8), dtype=torch.float32, device=dev)    # plan.OUT_BYTES per rank
        dlogits = torch.empty((b, pl.n_classes), dtype=torch.float32, device=dev)

        def run_shard(r, shard):
            _, fa = pl.forward(shard[0], self.grad_target(), True, seeds[r], offset, labels=shard[1], out=out[r], dlogits=dlogits,
                               tables=self.rebuild_tables(pl))
            self._plan_backward(pl, fa, (shard[0], None, dlogits, None))
        end = self.n_cls if self.classifier_only else self.flat.numel
        self._virtual_pass(shards, run_shard, end)
        self.t += 1
        if self.guard is not None:
            self._guard_judge(0, end)
        self._update(0, end)
        self._poll_errors()
        self.rank_losses, self.rank_hits = out[:, 0], out[:, 2:6].view(torch.int64)
        return self.rank_losses.mean(), self.rank_hits.sum(0)

    def _update_range(self):
        return 0, (self.n_cls if self.classifier_only else self.flat.numel)

    def _param_order(self):
        order = super()._param_order()
        if self.classifier_only:           # the warm-up optimizer holds the classifier's parameters only
            cls = {id(p) for p in self.model.classifier.parameters()}
            order = [(k, i, p) for k, (_, i, p) in enumerate(o for o in order if id(o[2]) in cls)]
        return order

    def state_dict(self):
        sd = super().state_dict()
        if self.classifier_only:
            sd["param_groups"][0]["params"] = list(range(len(self._param_order())))
        return sd

    def evaluate(self, video, labels, batch):
        """``run_phase('test_dense')``: video [V, clips, 3, T, H, W] in eval mode, fed through the model ``batch`` clips at a
        time (the reference's BatchWrapper), then one ``avid_cls_loss`` over all V * clips logits.  Returns device tensors
        (confidence [V, C], loss [], hits [2] int64)."""
        from . import ops
        clips = video.shape[1]
        loss, conf, hits, _ = self._evaluate(video, batch, lambda outs: self._eval_loss(torch.cat(outs, 0), labels, clips))
        return conf, loss, hits


class ProbeStep(AdamStep):
    """One linear-probe training step of a ``models.MOSTModel`` around this package's ``R2Plus1D`` (eval-action-recg-linear.py:
    the summed cross-entropy of every tap's logits, Adam over ``model.parameters()`` with lr 1e-4 and weight decay 0): the
    forward launch program runs the training-mode tower, pools every tap, runs the heads and ends in one ``avid_cls_loss`` per
    tap (loss, top-1 / top-5 hits and ``dlogits`` on the device); the backward program holds the heads only; then one flat
    Adam launch.  The tower is frozen: the flat parameter, gradient and moment buffers hold the classifiers' parameters only
    (its BatchNorm running statistics still move: the reference trains the probe with the tower in training mode).  Nothing
    synchronises the host.  Single process: the shipped config is not distributed.
    The tower may also be this package's ``Conv2D`` with ``AdaptiveMaxPool2d((h, w))`` heads (sound classification): ``step`` and
    ``evaluate`` then take spectrograms [B, 1, T, F] / [V, clips, 1, T, F] where they take clips, everything else alike.
    ``set_lr`` and ``state_dict`` / ``load_state_dict`` are ``AdamStep``'s — ``torch.optim.Adam(model.parameters())``'s format,
    the frozen tower parameters listed without state.

    ``virtual_ranks`` = R > 1: the step of an R-replica ``nn.DataParallel`` job (the shipped probe config: eight GPUs, batch
    128) on this one GPU, as ``FinetuneStep``'s: ``step`` takes the global batch [R * b, ...], b in the programs' 2..256, and
    runs it shard after shard through one ``ProbePlan`` of the shard geometry — the tower's BatchNorm3d AND the heads'
    BatchNorm1d normalise with their replica's b rows — the classifiers' gradients are summed in rank order and applied with
    1 / R, the running statistics left (tower and heads) are replica 0's.  ``rank_losses`` [R, n_taps] / ``rank_hits``
    [R, n_taps, 2] hold every replica's own (None before the first such step)."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, optimizer="adam", momentum=0.0,
                 nesterov=False, max_grad_norm=None, skip_nonfinite=False, virtual_ranks=1, loss="ce", pos_weight=None,
                 label_smoothing=0.0, ema_decay=None, ema_warmup=False, ema_buffers=True, param_rules=None,
                 trust_coefficient=0.001):
        """``optimizer`` / ``momentum`` / ``nesterov``, ``max_grad_norm`` / ``skip_nonfinite`` (the step guard): see ``AdamStep``.
        ``virtual_ranks``: see the class.  ``loss`` / ``pos_weight`` / ``label_smoothing``: as ``FinetuneStep``'s — ``"bce"`` ends
        every tap in ``avid_mlabel_loss`` against float32 targets [B, C], ``"soft_ce"`` in ``avid_soft_ce_loss`` against float32
        distributions [B, C] (or int64 labels [B], made one-hot on the device)."""
        R = _virtual_ranks_arg("ProbeStep", virtual_ranks)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("ProbeStep runs in a single process (the linear probe's config is not distributed)")
        super().__init__(model, lr, betas, eps, weight_decay, optimizer=optimizer, momentum=momentum, nesterov=nesterov,
                         max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, ema_decay=ema_decay, ema_warmup=ema_warmup,
                         ema_buffers=ema_buffers, param_rules=param_rules, trust_coefficient=trust_coefficient,
                         broadcast_buffers="off")
        self.n_taps = len(model.classifiers)
        self._set_loss(loss, pos_weight, lambda: next(iter(model.classifiers)).classifier.weight.shape[0], label_smoothing)
        self.virtual_ranks = R
        self.rank_losses = self.rank_hits = None     # [R, n_taps] float32 / [R, n_taps, 2] int64 of the last virtual-rank step

    def _plan(self, video):
        from . import plan
        pl = plan.probe_plan(self.model, video, need_grad=False, loss=self.loss, pos_weight=self.pos_weight,
                             label_smoothing=self.label_smoothing)
        if pl is None or plan._engine_flat(self, pl) is None:
            raise NotImplementedError("ProbeStep: the model is outside the compiled probe programs (plan.ProbePlan: MOSTModel("
                                      "R2Plus1D, AdaptiveMaxPool3d heads on conv2x..conv5x, use_bn, no l2_norm / dropout), fp32 "
                                      "CUDA parameters, batch 2..256, training mode, no hooks)")
        return pl

    def step(self, video, labels):
        """(losses [n_taps], hits [n_taps, 2] int64: top-1 / top-5 hits of the batch per tap) as device tensors.
        ``virtual_ranks`` > 1: per tap the mean of the ranks' losses and the sum of their hits, over the global batch."""
        self._ema_live("step")
        if self.virtual_ranks > 1:
            return self._virtual_step(video, labels)
        video, labels = self._labelled(video, labels)
        B = video.shape[0]
        pl = self._plan(video)
        if self.guard is not None:
            self._guard_begin()
        out = torch.empty((self.n_taps, 8), dtype=torch.float32, device=video.device)     # plan.PROBE_OUT_BYTES per tap
        dlogits = torch.empty((self.n_taps, B, pl.n_classes), dtype=torch.float32, device=video.device)
        _, fa = pl.forward(video, self.flat.grad, True, labels=labels, out=out, dlogits=dlogits)
        self._plan_backward(pl, fa, (video, None, dlogits, None))
        self.t += 1
        if self.guard is not None:
            self._guard_judge()
        self._update()
        self._poll_errors()
        return out[:, 0], out[:, 2:6].view(torch.int64)

    def _virtual_step(self, video, labels):
        """The step of ``virtual_ranks`` replicas (see the class): per shard the forward program (tower, pools, heads, one
        ``avid_cls_loss`` per tap over the shard's b rows) and the heads' backward; then ONE guard and optimizer pass."""
        b, shards = self._virtual_shards(video, labels)
        if not 2 <= b <= 256:
            raise ValueError(f"ProbeStep(virtual_ranks={self.virtual_ranks}).step: the per-rank batch must be 2..256 clips "
                             f"(BatchNorm1d on the rank's own rows; the probe programs' limit): a global batch of "
                             f"{video.shape[0]} with virtual_ranks={self.virtual_ranks} leaves {b}")
        pl = self._plan(shards[0][0])
        if self.guard is not None:
            self._guard_begin()
        dev = video.device
        out = torch.empty((len(shards), self.n_taps, 8), dtype=torch.float32, device=dev)   # plan.PROBE_OUT_BYTES per rank and tap
        dlogits = torch.empty((self.n_taps, b, pl.n_classes), dtype=torch.float32, device=dev)

        def run_shard(r, shard):
            _, fa = pl.forward(shard[0], self.grad_target(), True, labels=shard[1], out=out[r], dlogits=dlogits,
                               tables=self.rebuild_tables(pl))
            self._plan_backward(pl, fa, (shard[0], None, dlogits, None))
        self._virtual_pass(shards, run_shard)
        self.t += 1
        if self.guard is not None:
            self._guard_judge()
        self._update()
        self._poll_errors()
        self.rank_losses, self.rank_hits = out[:, :, 0], out[:, :, 2:6].view(torch.int64)
        return self.rank_losses.mean(0), self.rank_hits.sum(0)

    def evaluate(self, video, labels, batch):
        """``run_phase('test_dense')``: video [V, clips, 3, T, H, W] in eval mode, fed through the model ``batch`` clips at a
        time, then one ``avid_cls_loss`` per tap over all V * clips logits.  Returns device tensors
        (confidence [n_taps, V, C], losses [n_taps], hits [n_taps, 2] int64)."""
        from . import ops
        clips = video.shape[1]
        res = self._evaluate(video, batch, lambda outs: [self._eval_loss(torch.cat([o[ft] for o in outs], 0), labels, clips)
                                                         for ft in self.model.feat_names])
        return (torch.stack([r[1] for r in res]), torch.stack([r[0] for r in res]), torch.stack([r[2] for r in res]))
