"""``TrainStep(virtual_ranks=R)`` without a GPU: what it refuses and how (every message names the argument), the per-rank seeds,
and the new symbol in the header and the ctypes table."""
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE, U64 = 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16), torch.nn.Linear(16, 4))


def _criterion(seed=1234):
    """What the engine asks of a criterion on the host: ``nce_average.multinomial`` with a seed and a position."""
    from utils.alias_method import AliasMethod
    mult = AliasMethod(torch.ones(9))
    mult.reseed(seed, 0)
    crit = torch.nn.Module()
    crit.nce_average = types.SimpleNamespace(multinomial=mult)
    return crit


def _engine(R, **kw):
    from avid_hip.parallel import TrainStep
    return TrainStep(_model(), _criterion(), virtual_ranks=R, **kw)


def test_default_is_one_rank_and_zero_is_refused():
    from avid_hip.parallel import TrainStep
    eng = TrainStep(_model(), _criterion())
    assert eng.virtual_ranks == 1 and eng.rank_losses is None
    with pytest.raises(ValueError, match="virtual_ranks"):
        _engine(0)


def test_step_refuses_a_batch_the_ranks_do_not_divide():
    eng = _engine(3)
    with pytest.raises(ValueError, match=r"virtual_ranks=3 does not divide 4"):
        eng.step(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"virtual_ranks=3"):            # the three inputs are one global batch
        eng.step(torch.zeros(6, 8), torch.zeros(3, 8), torch.zeros(6, dtype=torch.int64))


def test_lazy_buffer_broadcast_is_refused_with_virtual_ranks():
    for mode in ("lazy", "off"):
        with pytest.raises(ValueError, match=rf"broadcast_buffers='{mode}' is not supported with virtual_ranks > 1"):
            _engine(2, broadcast_buffers=mode)
    from avid_hip.parallel import TrainStep
    assert TrainStep(_model(), _criterion(), broadcast_buffers="lazy").virtual_ranks == 1      # one rank: as before


def test_capture_is_refused_with_virtual_ranks():
    eng = _engine(2)
    with pytest.raises(NotImplementedError, match=r"virtual_ranks > 1"):
        eng.capture(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, dtype=torch.int64))


def _group_job(rank, world):
    import sys
    sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
    from avid_hip.parallel import TrainStep
    m = _model()
    before = [p.detach().clone() for p in m.parameters()]
    try:
        TrainStep(m, _criterion(), virtual_ranks=2)
    except ValueError as e:
        # refused before anything was touched: no broadcast, the parameters are still the module's own tensors
        return str(e), all(torch.equal(a, b) for a, b in zip(before, m.parameters()))
    return None, False


def test_a_process_group_of_two_ranks_is_refused_with_virtual_ranks():
    from test_distributed_cpu import run2
    res = run2(_group_job)
    for rank in range(2):
        msg, untouched = res[rank]
        assert msg is not None and "process group of more than one rank" in msg and "virtual_ranks" in msg and untouched


def test_default_seeds_follow_the_rank_formula_and_reseed_sets_them():
    eng = _engine(4)
    base = 1234
    assert [s for s, _ in eng._rank_sampler] == [(base + STRIDE * r) & U64 for r in range(4)]
    assert all(off == 0 for _, off in eng._rank_sampler)
    sd = eng.state_dict()["avid_sampler"]
    assert sd["seeds"] == [(base + STRIDE * r) & U64 for r in range(4)] and sd["offset"] == 0 and sd["seed"] == base
    eng.reseed([100, 101, 102, 103], offset=7)
    assert eng._rank_sampler == [[100, 7], [101, 7], [102, 7], [103, 7]]
    assert eng.state_dict()["avid_sampler"] == {"seed": 100, "offset": 7, "seeds": [100, 101, 102, 103]}
    for bad in ([100], [1, 2, 3], [1, 2, 3, 4, 5]):
        with pytest.raises(ValueError, match="4 seed"):
            eng.reseed(bad)
    # one rank: no "seeds" key, the checkpoint is what it was
    from avid_hip.parallel import TrainStep
    one = TrainStep(_model(), _criterion())
    assert one.state_dict()["avid_sampler"] == {"seed": 1234, "offset": 0}
    with pytest.raises(ValueError, match="1 seed"):
        one.reseed([1, 2])


def test_checkpoint_restores_every_rank_seed():
    a, b = _engine(2), _engine(2)
    a.reseed([100, 101], 5)
    sd = a.state_dict()
    b.load_state_dict(sd)
    assert b._rank_sampler == [[100, 5], [101, 5]]
    assert (b._sampler().seed, b._sampler().offset) == (100, 5)
    # a checkpoint written by a one-rank engine: the other ranks' seeds by the formula
    sd["avid_sampler"] = {"seed": 9, "offset": 3}
    b.load_state_dict(sd)
    assert b._rank_sampler == [[9, 3], [(9 + STRIDE) & U64, 3]]


def test_grad_accum_flat_is_in_the_header_and_the_ctypes_table():
    import ctypes as C
    from avid_hip import lib, ops
    header = open(os.path.join(REPO, "include", "avid_hip.h")).read()
    decl = re.search(r"int\s+avid_grad_accum_flat\s*\(([^)]*)\)\s*;", header)
    assert decl, "avid_grad_accum_flat is not declared in include/avid_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["int64_t", "float*", "const float*", "const float*", "avid_stream_t"]
    res, argtypes = lib.SIGNATURES["avid_grad_accum_flat"]
    assert res is C.c_int and argtypes == [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.raw("avid_grad_accum_flat").argtypes == argtypes
    with pytest.raises(lib.AvidHipError, match="no CPU fallback"):
        ops.grad_accum_flat(torch.zeros(4), torch.zeros(4), torch.zeros(4))
