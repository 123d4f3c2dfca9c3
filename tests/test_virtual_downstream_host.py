"""``FinetuneStep`` / ``ProbeStep(virtual_ranks=R)`` without a GPU: the defaults, what they refuse and how (every message names the
argument), the per-replica dropout seeds, and — in float64 on a tiny pure-torch model — that the rule the engines implement
(per-shard statistics and mean losses, gradients summed in rank order and taken with 1 / R, shard 0's buffers) IS what
``nn.DataParallel`` computes (tests/_dp_ref.py), and is not what the one-rank whole-batch step computes."""
import os

import pytest
import torch

import _dp_ref as DP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE, U64 = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16), torch.nn.Linear(16, 4))


def _wrapper():
    """A ClassificationWrapper with dropout, on the host (a stand-in tower: the engine's constructor never runs it)."""
    import models
    torch.manual_seed(0)
    return models.ClassificationWrapper(torch.nn.Linear(6, 6), 3, "pool", 6, use_dropout=True, dropout=0.5)


class _Probe(torch.nn.Module):
    """What ProbeStep's constructor asks of a model: a frozen tower and ``classifiers``."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.feature_extractor = torch.nn.Linear(6, 6)
        for p in self.feature_extractor.parameters():
            p.requires_grad = False
        self.classifiers = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.BatchNorm1d(6), torch.nn.Linear(6, 3)) for _ in range(2)])


def _finetune(R, **kw):
    from avid_hip.parallel import FinetuneStep
    return FinetuneStep(_model(), virtual_ranks=R, **kw)


def test_default_is_one_rank():
    from avid_hip.parallel import FinetuneStep, ProbeStep
    for eng in (FinetuneStep(_model()), ProbeStep(_Probe())):
        assert eng.virtual_ranks == 1 and eng.rank_losses is None and eng.rank_hits is None
        assert eng._acc is None and eng._grad_scale() == 1.0
    assert _finetune(4)._grad_scale() == 0.25


@pytest.mark.parametrize("which", ["FinetuneStep", "ProbeStep"])
def test_fewer_than_one_rank_is_refused(which):
    from avid_hip import parallel
    make = (lambda R: _finetune(R)) if which == "FinetuneStep" else (lambda R: parallel.ProbeStep(_Probe(), virtual_ranks=R))
    for bad in (0, -2):
        with pytest.raises(ValueError, match=rf"{which}: virtual_ranks must be >= 1 \(got {bad}\)"):
            make(bad)


def test_lazy_buffer_broadcast_is_refused_with_virtual_ranks():
    for mode in ("lazy", "off"):
        with pytest.raises(ValueError, match=rf"FinetuneStep\(virtual_ranks=2\).*broadcast_buffers='{mode}' is not supported with "
                                             r"virtual_ranks > 1"):
            _finetune(2, broadcast_buffers=mode)
    assert _finetune(1, broadcast_buffers="lazy").virtual_ranks == 1               # one rank: as before


@pytest.mark.parametrize("which", ["FinetuneStep", "ProbeStep"])
def test_forced_collectives_are_refused_with_virtual_ranks(which, monkeypatch):
    """AVID_FORCE_DIST=1 on a one-rank group drives the collectives: not with virtual ranks.  Refused before anything is
    flattened: the parameters are still the module's own tensors."""
    import torch.distributed as dist
    from avid_hip import parallel
    from test_distributed_cpu import _free_port
    monkeypatch.setenv("AVID_FORCE_DIST", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        m = _model() if which == "FinetuneStep" else _Probe()
        before = [(p, p.data_ptr()) for p in m.parameters()]
        with pytest.raises(ValueError, match=rf"{which}\(virtual_ranks=2\).*AVID_FORCE_DIST=1.*virtual_ranks > 1"):
            getattr(parallel, which)(m, virtual_ranks=2)
        assert all(p.data_ptr() == ptr for p, ptr in before) and parallel.flat_of(m.parameters()) is None
    finally:
        dist.destroy_process_group()


def _group_job(rank, world):
    import sys
    sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
    from avid_hip.parallel import FinetuneStep, ProbeStep
    out = []
    for cls, m in ((FinetuneStep, _model()), (ProbeStep, _Probe())):
        if rank == 1:                                   # a construction broadcast would overwrite this with rank 0's
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(1.0)
        before = [p.detach().clone() for p in m.parameters()]
        try:
            cls(m, virtual_ranks=2)
        except ValueError as e:
            out.append((str(e), all(torch.equal(a, b) for a, b in zip(before, m.parameters()))))
        else:
            out.append((None, False))
    return out


def test_a_process_group_of_two_ranks_is_refused_with_virtual_ranks():
    from test_distributed_cpu import run2
    res = run2(_group_job)
    for rank in range(2):
        for who, (msg, untouched) in zip(("FinetuneStep", "ProbeStep"), res[rank]):
            assert msg is not None and msg.startswith(f"{who}(virtual_ranks=2)"), (rank, who, msg)
            assert "process group of more than one rank" in msg and "virtual_ranks > 1" in msg and untouched


def test_step_refuses_a_batch_the_ranks_do_not_divide():
    eng = _finetune(3)
    with pytest.raises(ValueError, match=r"FinetuneStep\(virtual_ranks=3\)\.step.*virtual_ranks=3 does not divide 4"):
        eng.step(torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"virtual_ranks=3 does not divide 6 \(labels 3\)"):    # video and labels are one batch
        eng.step(torch.zeros(6, 8), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"labels must be int64 \[6\]"):                         # ... checked as before
        eng.step(torch.zeros(6, 8), torch.zeros(6, dtype=torch.int32))
    assert eng.t == 0 and eng._acc is None and eng.rank_losses is None


def test_a_model_outside_the_programs_stays_not_implemented():
    """There is no per-layer form of the virtual step: what the one-rank step refuses, it refuses the same way."""
    for R in (1, 2):
        with pytest.raises(NotImplementedError, match="outside the compiled fine-tuning programs"):
            _finetune(R).step(torch.zeros(6, 8), torch.zeros(6, dtype=torch.int64))


def test_dropout_seeds_follow_the_rank_formula_and_reseed_sets_them():
    from avid_hip.parallel import FinetuneStep
    m = _wrapper()
    eng = FinetuneStep(m, virtual_ranks=4)
    base = m.dropout.seed
    assert eng.dropout_seeds == [(base + STRIDE * r) & U64 for r in range(4)] and len(set(eng.dropout_seeds)) == 4
    m.dropout.seed = 1234                                           # rank 0's seed is the model's own, the others follow it
    assert eng.dropout_seeds == [(1234 + STRIDE * r) & U64 for r in range(4)]
    eng.reseed_dropout([100, 101, 102, 103])
    assert eng.dropout_seeds == [100, 101, 102, 103] and m.dropout.seed == 100 and m.dropout.offset == 0
    eng.reseed_dropout([7, 8, 9, 10], offset=5)
    assert eng.dropout_seeds == [7, 8, 9, 10] and (m.dropout.seed, m.dropout.offset) == (7, 5)
    for bad in ([100], [1, 2, 3], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError, match=r"FinetuneStep\.reseed_dropout: 4 seed\(s\) expected, one per virtual rank \(got "
                                             + str(len(bad))):
            eng.reseed_dropout(bad)
    assert eng.dropout_seeds == [7, 8, 9, 10]
    one = FinetuneStep(_wrapper())
    assert one.dropout_seeds == [one.model.dropout.seed]
    with pytest.raises(ValueError, match="1 seed"):
        one.reseed_dropout([1, 2])
    one.reseed_dropout([55])
    assert one.model.dropout.seed == 55 and one.dropout_seeds == [55]
    # a model without dropout has no seeds to set
    assert _finetune(2).dropout_seeds is None
    with pytest.raises(ValueError, match="no dropout"):
        _finetune(2).reseed_dropout([1, 2])


def test_virtual_ranks_is_not_part_of_a_checkpoint():
    a, b = _finetune(1), _finetune(2)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() == {"state", "param_groups"} and sa["param_groups"] == sb["param_groups"]
    b.load_state_dict(sa)
    a.load_state_dict(sb)
    assert (a.virtual_ranks, b.virtual_ranks) == (1, 2)


def test_probe_step_constructs_and_refuses_a_per_rank_batch_outside_the_programs():
    from avid_hip.parallel import ProbeStep
    eng = ProbeStep(_Probe(), virtual_ranks=2)
    assert eng.virtual_ranks == 2 and eng.n_taps == 2 and eng.rank_losses is None and eng._grad_scale() == 0.5
    assert eng.flat.numel == sum((p.numel() + 3) // 4 * 4 for p in eng.model.classifiers.parameters())
    with pytest.raises(ValueError, match=r"ProbeStep\(virtual_ranks=2\)\.step: the per-rank batch must be 2\.\.256.*"
                                         r"virtual_ranks=2 leaves 1"):
        eng.step(torch.zeros(2, 6), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"virtual_ranks=2 leaves 257"):
        eng.step(torch.zeros(514, 6), torch.zeros(514, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"virtual_ranks=2 does not divide 5"):
        eng.step(torch.zeros(5, 6), torch.zeros(5, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="outside the compiled probe programs"):    # a batch in range: the plan decides
        eng.step(torch.zeros(4, 6), torch.zeros(4, dtype=torch.int64))


# ------------------------------------------------------------------------------------------ the rule, in float64
def _batch(R, b=5):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(R * b, 8, generator=g, dtype=torch.float64) * torch.linspace(0.5, 3.0, R * b, dtype=torch.float64)[:, None]
    return x, torch.randint(0, 4, (R * b,), generator=g)


@pytest.mark.parametrize("R", [2, 3])
def test_the_engine_rule_is_data_parallel_and_not_the_whole_batch_step(R):
    m = _model()
    x, y = _batch(R)
    dp_g, dp_buf, dp_loss = DP.data_parallel(m, x, y, R)
    en_g, en_buf, en_loss = DP.engine_rule(m, x, y, R)
    wb_g, wb_buf, wb_loss = DP.whole_batch(m, x, y)
    assert all(g.dtype == torch.float64 for g in dp_g + en_g + wb_g)
    assert DP.rel(en_g, dp_g) <= 1e-12
    assert abs(float(en_loss) - float(dp_loss)) <= 1e-12 * abs(float(dp_loss))
    floats = [n for n, v in dp_buf.items() if v.is_floating_point()]
    assert len(floats) == 2 and DP.rel([en_buf[n] for n in floats], [dp_buf[n] for n in floats]) <= 1e-12
    assert all(int(buf["1.num_batches_tracked"]) == 1 for buf in (dp_buf, en_buf, wb_buf))
    # shard 0's statistics are not the batch's, and the gradient of the per-shard-normalised model is not the whole-batch one
    assert DP.rel(wb_g, dp_g) > 1e-3 and DP.rel(wb_g, en_g) > 1e-3
    assert DP.rel([wb_buf[n] for n in floats], [dp_buf[n] for n in floats]) > 1e-3
    # (the initial state was not touched: every function works on its own copies)
    assert all(p.grad is None for p in m.parameters()) and int(m[1].num_batches_tracked) == 0
