"""``TrainStep(virtual_ranks=R)``: the step of an R-rank job on one MI355X, shard after shard, and the kernel that sums the
shards' gradients (``avid_grad_accum_flat``).

Sizes, model, banks and ids are those of tests/test_gpu_two_ranks.py (64 x 64 video, 1 x 40 x 100 audio, b = 2 per rank, a
2000-row bank, 64 negatives, everything from ``oracle.detgen``), whose two-process gloo job pins what a two-rank step is:

* R = 2 IS that job, bit for bit: Z, every rank's loss of every step, the all-reduced gradient, the parameters, both banks,
  rank 0's BatchNorm running statistics;
* R = 3 and AVID_CMA with R = 2 against single-process runs of each shard: Z the rank-order mean, the gradient buffer
  ((g0 + g1) + g2), Adam on it with 1/R, ONE bank update with all records in order, shard 0's running statistics, every sampler
  stream one draw further — and no trace of the first step's statistics pass;
* ``virtual_ranks=1`` is the engine as it was; a checkpoint taken between steps resumes bit for bit.

All comparisons are of bits unless a tolerance is named (the oracle's: rtol 2e-5, the two-rank test's)."""
import numpy as np
import pytest
import torch

import test_gpu_two_ranks as TR
from _guards import FILLS, guarded

pytestmark = pytest.mark.gpu

N_BANK, K_NEG, BS, IDS = TR.N_BANK, TR.K_NEG, TR.BS, TR.IDS
T = TR.T


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ------------------------------------------------------------------------------------------------------- the kernel alone
SIZES = (1, 3, 255, 1025, (1 << 20) + 7)


def _operands(n, dev):
    """a, b [n] with a few inf / nan planted where there is room (at every size at least one special value)."""
    from oracle import detgen
    a = T(detgen.det_normalish(f"accum:a:{n}", (n,))).clone()
    b = T(detgen.det_uniform(f"accum:b:{n}", (n,))).clone()
    a[0] = float("inf")
    if n > 2:
        b[1], a[2], b[2] = float("nan"), float("inf"), float("-inf")          # nan + x, inf - inf
    if n > 200:
        a[n - 1], b[n - 2], a[n // 2] = float("nan"), float("-inf"), -0.0
        b[n // 2] = -0.0                                                       # -0 + -0 = -0
    return a.to(dev), b.to(dev)


@pytest.mark.parametrize("n", SIZES)
def test_grad_accum_flat_is_torch_add_bit_for_bit(gpu_device, n):
    from avid_hip import ops
    a, b = _operands(n, gpu_device)
    want = a + b
    assert bool(torch.isnan(want).any()) == (n > 2) and bool(torch.isinf(want).any())
    for shift in (0, 1):                     # 1: every buffer one element off a 16-byte boundary (the scalar path)
        def seat(t):
            buf = torch.full((n + shift,), 7.0, device=gpu_device)
            buf[shift:].copy_(t)
            assert (buf[shift:].data_ptr() % 16 == 0) == (shift == 0)
            return buf, buf[shift:]
        for which in ("third", "a", "b"):
            (abuf, av), (bbuf, bv) = seat(a), seat(b)
            dbuf, dv = seat(torch.zeros(n)) if which == "third" else ((abuf, av) if which == "a" else (bbuf, bv))
            ops.grad_accum_flat(dv, av, bv)
            assert same_bits(dv, want), (n, shift, which)
            if which != "a":
                assert same_bits(av, a)      # an input that is not the destination is not written
            if which != "b":
                assert same_bits(bv, b)
            if shift:
                assert float(dbuf[0]) == 7.0 and float(abuf[0]) == 7.0 and float(bbuf[0]) == 7.0


def test_grad_accum_flat_refuses_partial_overlap_and_bad_arguments(gpu_device):
    from avid_hip import lib, ops
    n = 1024
    buf = torch.zeros(2 * n + 8, device=gpu_device)
    c = torch.ones(n, device=gpu_device)
    for off in (1, 4, n - 1):                # dst overlaps an input without being it, from either side, aligned or not
        with pytest.raises(lib.AvidHipError, match="grad_accum_flat"):
            ops.grad_accum_flat(buf[off:off + n], buf[:n], c)
        with pytest.raises(lib.AvidHipError, match="grad_accum_flat"):
            ops.grad_accum_flat(buf[:n], c, buf[off:off + n])
    ops.grad_accum_flat(buf[n:2 * n], buf[:n], c)          # adjacent is not overlapping
    ops.grad_accum_flat(buf[:n], buf[n:2 * n], buf[n:2 * n])  # a is b
    assert float(buf[:n].min()) == 2.0 and float(buf[:n].max()) == 2.0
    call = lib.raw("avid_grad_accum_flat")
    P = ops._p
    BADARG = call(0, P(buf), P(buf), P(c), None)
    assert BADARG < 0 and "grad_accum_flat" in lib.last_error()
    for args in ((-1, P(buf), P(buf), P(c)), (n, None, P(buf), P(c)), (n, P(buf), None, P(c)), (n, P(buf), P(c), None)):
        assert call(*args, None) == BADARG
    with pytest.raises(lib.AvidHipError, match="one size"):
        ops.grad_accum_flat(buf[:n], buf[:n], c[:n - 1])
    assert float(buf[:n].min()) == 2.0       # nothing above was launched


@pytest.mark.parametrize("shift", (0, 1), ids=("aligned", "unaligned"))
def test_grad_accum_flat_writes_inside_its_buffers(gpu_device, shift):
    """Exactly-sized guarded buffers, both fills (tests/_guards.py): no guard byte changes, the same bits as unguarded.  The
    unaligned case starts one element into its buffers; that leading element keeps the fill."""
    from avid_hip import ops
    n = 1025                                 # vectors and a tail; more than one block
    a, b = _operands(n, gpu_device)
    want = a + b
    for fill in FILLS:
        with guarded(fill) as g:
            av, bv = g.place(torch.cat([a[:shift], a])), g.place(torch.cat([b[:shift], b]))
            dv = torch.empty(n + shift, device=gpu_device)          # guarded, filled with the pattern
            assert dv.data_ptr() % 256 == 0
            ops.grad_accum_flat(dv[shift:], av[shift:], bv[shift:])
            ops.grad_accum_flat(av[shift:], av[shift:], bv[shift:])  # in place on a guarded input
            g.check()
            assert same_bits(dv[shift:], want) and same_bits(av[shift:], want) and same_bits(bv[shift:], b), (fill, shift)
            if shift:
                assert bytes(dv[:1].view(torch.uint8).cpu().tolist()) == bytes([fill] * 4)


# ------------------------------------------------------------------------------------------------------- engines and shards
def _avid(dev):
    crit = TR._criterion(dev, 0)
    TR._set_banks(crit, 0)
    return crit


def _cma(dev):
    import criterions
    crit = criterions.AVID_CMA(num_data=N_BANK, embedding_dim=128, num_negatives=K_NEG, num_negatives_within=16, momentum=0.5,
                               sampling_args={"type": "consensus", "pos_k": 8}, device=dev.index)
    TR._set_banks(crit, 0)
    crit.nce_average.find_correspondences()              # of the deterministic banks
    return crit


def _engine(dev, make_crit=_avid, **kw):
    from avid_hip.parallel import TrainStep
    m = TR._model(dev)
    crit = make_crit(dev)
    return TrainStep(m, crit, bucket_bytes=4 << 20, **kw), m, crit


def _banks(crit):
    return crit.nce_average.view1_mem.clone(), crit.nce_average.view2_mem.clone()


def _global_inputs(n, dev):
    """n samples: the two-rank test's four, then more of the same kind."""
    from oracle import detgen
    video, audio = TR._inputs()
    if n > video.shape[0]:
        more = n - video.shape[0]
        video = torch.cat([video, T(detgen.det_normalish("vr:video", (more, 3, 8, 64, 64)))])
        audio = torch.cat([audio, T(detgen.det_normalish("vr:audio", (more, 1, 40, 100)))])
    return video[:n], audio[:n]


class Shard:
    """A single-process engine (no virtual ranks, no process group) that runs ONE rank's shard from a given state: the
    ``_single`` pattern of tests/test_gpu_two_ranks.py, re-usable for several runs."""

    def __init__(self, dev, make_crit=_avid):
        self.dev = dev
        self.eng, self.model, self.crit = _engine(dev, make_crit)
        self.nbt = [m.num_batches_tracked for m in self.model.modules() if getattr(m, "num_batches_tracked", None) is not None]

    def run(self, v, a, y, seed, offset, Z, banks=None, params=None, fused=False):
        """forward_backward of the shard against ``banks`` / ``params`` (default: the deterministic initial ones) with the
        sampler at (seed, offset) and Z preset (None: estimated from this shard).  ``fused`` off: the criterion ops a first
        step runs (compare like with like)."""
        from avid_hip import ops
        crit, eng = self.crit, self.eng
        if banks is None:
            TR._set_banks(crit, 0)
        else:
            crit.nce_average.view1_mem.copy_(banks[0])
            crit.nce_average.view2_mem.copy_(banks[1])
        if params is not None:
            eng.flat.flat.copy_(params)
        crit.nce_average.multinomial.reseed(seed, offset)
        crit.criterion.avg_exp_score.fill_(-1.0 if Z is None else float(Z))
        crit.criterion._z_ready = Z is not None
        keep, ops.FUSED_CRITERION = ops.FUSED_CRITERION, bool(fused)
        try:
            with TR._RecordUpdates() as rec:
                loss = eng.forward_backward(v.to(self.dev), a.to(self.dev), torch.tensor(y, dtype=torch.int64, device=self.dev))
        finally:
            ops.FUSED_CRITERION = keep
        return {"loss": float(loss.detach()), "grad": eng.flat.grad.clone(), "Z": crit.criterion.avg_exp_score.clone().cpu(),
                "emb": [c[1] for c in rec.calls], "bn": eng.flat_buffers.flat.clone()}


def _expected_banks(before, ids, embs, dev):
    """Both banks after ONE update with the shards' records in rank order."""
    from avid_hip import ops
    out = []
    for b in range(2):
        bank = before[b].clone()
        ops.bank_update(bank, torch.tensor(ids, device=dev), torch.cat([e[b] for e in embs]).to(dev), 0.5)
        out.append(bank)
    return out


# ------------------------------------------------------------------------------------------------------- R = 2: the two-rank job
def test_two_virtual_ranks_are_the_two_rank_job(tmp_path, gpu_device):
    r = TR._run2("train", tmp_path)
    dev = gpu_device
    eng, m, crit = _engine(dev, virtual_ranks=2)
    eng.reseed([100, 101])
    video, audio = TR._inputs()
    v, a = video.to(dev), audio.to(dev)
    assert eng.buckets.world == 1 and not eng.buckets.comm
    for step, ids in enumerate(IDS):
        y = torch.tensor(ids, dtype=torch.int64, device=dev)
        with TR._RecordUpdates() as rec:
            loss = eng.forward_backward(v, a, y)
        if step == 0:
            assert same_bits(crit.criterion.avg_exp_score, r[0]["Z"]) and same_bits(r[1]["Z"], r[0]["Z"])
            assert same_bits(eng.flat.grad, r[0]["grad0"]) and same_bits(r[1]["grad0"], r[0]["grad0"])
        eng.optimizer_step()
        if step == 0:
            assert same_bits(eng.flat.flat, r[0]["params0"])
        assert tuple(eng.rank_losses.shape) == (2,) and eng.rank_losses.is_cuda and loss.dim() == 0
        got = [float(x) for x in eng.rank_losses]
        assert got == [r[0]["loss"][step], r[1]["loss"][step]], (step, got)
        np.testing.assert_allclose(float(loss), np.float32(0.5) * (np.float32(got[0]) + np.float32(got[1])), rtol=1e-6)
        for b, bank in enumerate(_banks(crit)):
            assert same_bits(bank, r[0]["banks"][step][b]), (step, b)
        assert same_bits(m.video_model.conv1[1].running_mean, r[0]["bn_mean"][step]), step
        # one update per step with the four records in global order — what both ranks of the job were handed
        assert len(rec.calls) == 2 and rec.calls[0][0].tolist() == ids
        assert same_bits(rec.calls[0][1], r[0]["updates"][step][0][1])
    assert same_bits(eng.flat.flat, r[0]["params_final"])
    assert eng.t == len(IDS) and int(eng.t_dev) == len(IDS)
    from avid_hip import ops
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------- R = 3 against shard runs
def test_three_virtual_ranks_against_single_process_shard_runs(gpu_device, kernel_log):
    from oracle import avid_oracle as O
    from avid_hip import ops
    dev, R = gpu_device, 3
    ids = [5, 17, 900, 31, 1200, 17]                      # 17 on ranks 0 and 2: the highest global position owns the row
    seeds = [100, 101, 102]
    video, audio = _global_inputs(R * BS, dev)
    sh = lambda t, k: t[k * BS:(k + 1) * BS]
    # ---- the shards on their own: Z of each, then loss / gradient / records with the shared Z (unfused, as a first step runs)
    shard = Shard(dev)
    first = [shard.run(sh(video, k), sh(audio, k), sh(ids, k), seeds[k], 0, None) for k in range(R)]
    bn0 = first[0]["bn"]                                  # ... run 0 was the first forward of that model: shard 0's statistics
    # the mean over ranks as criterions/nce.py takes it in an R-rank job — the ranks' values summed in rank order (all_reduce),
    # then ``Z /= world`` ON THE DEVICE, where torch divides by a host scalar by multiplying with its fp32 reciprocal: for
    # R = 3 that is not the correctly rounded quotient, so the expectation is evaluated where the job evaluates it
    Z = (first[0]["Z"].to(dev) + first[1]["Z"].to(dev)) + first[2]["Z"].to(dev)
    Z /= R
    Z = Z.cpu()
    exact = (float(first[0]["Z"]) + float(first[1]["Z"]) + float(first[2]["Z"])) / R
    np.testing.assert_allclose(float(Z), exact, rtol=2 ** -22)        # (two fp32 sums, a reciprocal, a product: < 4 half-ulps)
    assert len({float(f["Z"]) for f in first}) == R
    single = [shard.run(sh(video, k), sh(audio, k), sh(ids, k), seeds[k], 0, float(Z)) for k in range(R)]
    # ---- the engine
    eng, m, crit = _engine(dev, virtual_ranks=R)
    eng.reseed(seeds)
    before = _banks(crit)
    nbt = [x.num_batches_tracked for x in m.modules() if getattr(x, "num_batches_tracked", None) is not None]
    assert len(nbt) > 30 and all(int(n) == 0 for n in nbt)
    y = torch.tensor(ids, dtype=torch.int64, device=dev)
    keep, ops.FUSED_CRITERION = ops.FUSED_CRITERION, False
    try:
        with TR._RecordUpdates() as rec:
            loss = eng.forward_backward(video.to(dev), audio.to(dev), y)
    finally:
        ops.FUSED_CRITERION = keep
    assert same_bits(crit.criterion.avg_exp_score, Z)
    gsum = (single[0]["grad"] + single[1]["grad"]) + single[2]["grad"]
    assert same_bits(eng.flat.grad, gsum)
    assert [float(x) for x in eng.rank_losses] == [s["loss"] for s in single]
    # the oracle on every shard: its own BatchNorm statistics, its own negatives, the shared Z
    P = O.det_state(O.av_wrapper_spec(18), "w")
    prob, alias = O.alias_build_uniform(N_BANK - 1)
    for k in range(R):
        yk = torch.tensor(sh(ids, k))
        idx = T(O.sample_negatives_from_draw(O.alias_draw_philox(prob, alias, BS * K_NEG, seeds[k], 0), yk.numpy(), K_NEG))
        with torch.no_grad():
            ve, ae = O.av_forward(sh(video, k), sh(audio, k), {n: w.clone() for n, w in P.items()}, 18, True)
            ref, _, _ = O.avid_forward(ve, ae, yk, idx, TR._det_bank("two:v1", N_BANK), TR._det_bank("two:v2", N_BANK),
                                       float(Z), 0.5)
        np.testing.assert_allclose(float(eng.rank_losses[k]), float(ref), rtol=2e-5)
    # one deferred bank update with the six records in order; nothing of the statistics pass in the banks
    assert len(rec.calls) == 2 and rec.calls[0][0].tolist() == ids
    for b, bank in enumerate(_expected_banks(before, ids, [s["emb"] for s in single], dev)):
        assert same_bits(_banks(crit)[b], bank), b
    # shard 0's running statistics, one forward counted, every sampler stream one draw on
    assert same_bits(eng.flat_buffers.flat, bn0)
    assert all(int(n) == 1 for n in nbt)
    assert [off for _, off in eng._rank_sampler] == [1] * R and [s for s, _ in eng._rank_sampler] == seeds
    assert eng.state_dict()["avid_sampler"] == {"seed": 100, "offset": 1, "seeds": seeds}
    # Adam on the accumulated gradient with 1 / R, the step counted once
    e = shard.eng
    ops.adam_flat(e.flat.flat, gsum, e.m, e.v, e.lr, e.betas[0], e.betas[1], e.eps, e.wd, 1, grad_scale=1.0 / R)
    eng.optimizer_step()
    assert same_bits(eng.flat.flat, e.flat.flat)
    assert eng.t == 1 and int(eng.t_dev) == 1
    # ---- a second step: Z is frozen, the shards go through the fused criterion
    p1 = eng.flat.flat.clone()
    with TR._RecordUpdates() as rec:
        loss2 = eng.step(video.to(dev), audio.to(dev), y)
    assert len(rec.calls) == 2 and rec.calls[0][0].tolist() == ids
    assert bool(torch.isfinite(eng.flat.flat).all()) and not torch.equal(eng.flat.flat, p1)
    assert bool(torch.isfinite(loss2)) and bool(torch.isfinite(eng.rank_losses).all())
    assert same_bits(crit.criterion.avg_exp_score, Z) and all(int(n) == 2 for n in nbt) and int(eng.t_dev) == 2
    assert [off for _, off in eng._rank_sampler] == [2] * R
    # ---- the launch log of a step: R - 1 accumulate launches, one optimizer launch
    with kernel_log() as log:
        eng.step(video.to(dev), audio.to(dev), y)
    assert log.launches("grad_accum_flat") == R - 1 and log.launches("adam_flat") == 1
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------- AVID_CMA, R = 2
def test_two_virtual_ranks_with_the_cma_criterion(gpu_device):
    dev, R = gpu_device, 2
    seeds = [7, 8]
    video, audio = _global_inputs(R * BS, dev)
    sh = lambda t, k: t[k * BS:(k + 1) * BS]
    shard = Shard(dev, _cma)
    eng, m, crit = _engine(dev, _cma, virtual_ranks=R)
    eng.reseed(seeds)
    assert torch.equal(crit.nce_average.positive_set, shard.crit.nce_average.positive_set)
    Z = None
    for step, ids in enumerate(IDS[:2]):                  # step 1: id 77 on both ranks
        before, params = _banks(crit), eng.flat.flat.clone()
        if step == 0:
            first = [shard.run(sh(video, k), sh(audio, k), sh(ids, k), seeds[k], 0, None) for k in range(R)]
            Z = (first[0]["Z"] + first[1]["Z"]) / R
        # (step 0 runs the unfused criterion ops on every rank, step 1 the fused kernel)
        single = [shard.run(sh(video, k), sh(audio, k), sh(ids, k), seeds[k], step, float(Z), banks=before, params=params,
                            fused=step > 0) for k in range(R)]
        with TR._RecordUpdates() as rec:
            eng.step(video.to(dev), audio.to(dev), torch.tensor(ids, dtype=torch.int64, device=dev))
        if step == 0:
            assert same_bits(crit.criterion.avg_exp_score, Z)
        assert same_bits(eng.flat.grad, single[0]["grad"] + single[1]["grad"]), step
        assert [float(x) for x in eng.rank_losses] == [s["loss"] for s in single], step
        assert len(rec.calls) == 2 and rec.calls[0][0].tolist() == ids
        for b, bank in enumerate(_expected_banks(before, ids, [s["emb"] for s in single], dev)):
            assert same_bits(_banks(crit)[b], bank), (step, b)
        assert [off for _, off in eng._rank_sampler] == [step + 1] * R
    from avid_hip import ops
    ops.check_device_errors(dev)


# ------------------------------------------------------------------------------------------------------- the default path
def test_one_virtual_rank_is_the_engine_as_it_was(gpu_device, kernel_log):
    dev = gpu_device
    video, audio = TR._inputs()
    v, a = video.to(dev), audio.to(dev)
    runs = []
    for kw in ({}, {"virtual_ranks": 1}):
        eng, m, crit = _engine(dev, **kw)
        losses = []
        for ids in IDS:
            loss = eng.step(v, a, torch.tensor(ids, dtype=torch.int64, device=dev))
            losses.append(loss.clone())
        assert eng.rank_losses is None and eng._acc is None
        runs.append((eng, losses, eng.flat.flat.clone(), _banks(crit), eng.flat_buffers.flat.clone()))
    (_, l0, p0, b0, s0), (eng, l1, p1, b1, s1) = runs
    assert all(same_bits(x, y) for x, y in zip(l0, l1))
    assert same_bits(p0, p1) and same_bits(b0[0], b1[0]) and same_bits(b0[1], b1[1]) and same_bits(s0, s1)
    assert "seeds" not in eng.state_dict()["avid_sampler"]
    with kernel_log() as log:
        eng.step(v, a, torch.tensor(IDS[0], dtype=torch.int64, device=dev))
    assert log.launches("grad_accum_flat") == 0 and log.launches("adam_flat") >= 1


# ------------------------------------------------------------------------------------------------------- checkpoint
def test_checkpoint_between_virtual_rank_steps_resumes_bit_for_bit(gpu_device):
    import copy
    dev = gpu_device
    video, audio = TR._inputs()
    v, a = video.to(dev), audio.to(dev)
    ys = [torch.tensor(ids, dtype=torch.int64, device=dev) for ids in IDS]
    eng, m, crit = _engine(dev, virtual_ranks=2)
    eng.reseed([100, 101])
    for y in ys[:2]:
        eng.step(v, a, y)
    saved = copy.deepcopy({"opt": eng.state_dict(), "model": m.state_dict(), "crit": crit.state_dict()})
    assert saved["opt"]["avid_sampler"] == {"seed": 100, "offset": 2, "seeds": [100, 101]}
    loss = eng.step(v, a, ys[2])
    want = (loss.clone(), eng.rank_losses.clone(), eng.flat.flat.clone(), _banks(crit), eng.flat_buffers.flat.clone())
    # a fresh engine (its own default seeds, Z unset) picks the run up
    eng2, m2, crit2 = _engine(dev, virtual_ranks=2)
    m2.load_state_dict(saved["model"])
    crit2.load_state_dict(saved["crit"])
    eng2.load_state_dict(saved["opt"])
    assert eng2._rank_sampler == [[100, 2], [101, 2]] and eng2.t == 2
    loss2 = eng2.step(v, a, ys[2])
    assert same_bits(loss2, want[0]) and same_bits(eng2.rank_losses, want[1]) and same_bits(eng2.flat.flat, want[2])
    assert same_bits(_banks(crit2)[0], want[3][0]) and same_bits(_banks(crit2)[1], want[3][1])
    assert same_bits(eng2.flat_buffers.flat, want[4])
