"""CPU-only acceptance of the in-batch InfoNCE criterion (avid_infonce): the float32 emulation of the kernel's order lies
inside the bounds of tests/_infonce_ref.py in both input regimes, every named defect lies at least ten times outside them,
the float64 restatement's gradient is torch autograd's, and the C ABI / Python layers agree and refuse bad arguments before
anything is launched.  (Without the feature this module fails at import.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import _infonce_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV_T = 1.0 / 0.07


def _case(regime, G, D, inv_T=INV_T, seed=3):
    return (R.make_unrelated if regime == "unrelated" else R.make_trained)(G, D, seed, inv_T)


@pytest.mark.parametrize("regime", ["unrelated", "trained"])
@pytest.mark.parametrize("G,D,inv_T,w", [(1, 32, INV_T, (0.5, 0.5)), (33, 32, INV_T, (0.3, 0.7)), (130, 128, 5.0, (0.5, 0.5)),
                                         (200, 64, INV_T, (1.0, 0.0))])
def test_emulation_inside_bounds(regime, G, D, inv_T, w):
    v, a = _case(regime, G, D, inv_T)
    r = R.ref64(v, a, inv_T, w)
    bd = R.bounds(r, v, a, inv_T, w)
    e = R.emulate32(v, a, inv_T, w)
    print("excess", R.excess(e, r, bd))
    assert R.excess(e, r, bd) <= 1.0
    assert float(np.abs(e["S"] - r["S"]).max()) <= bd["score"]
    assert float(np.abs(e["lse_v"] - r["lse_v"]).max()) <= bd["lse"] and float(np.abs(e["lse_a"] - r["lse_a"]).max()) <= bd["lse"]
    assert e["hits"] == r["hits"]
    if regime == "trained" and G > 1 and inv_T > 10:
        assert r["hits"][0] > 0.9 * G and float(np.diag(r["Pv"]).min()) > 0.5       # peaked: p_ii - 1 cancels


def test_emulation_inside_bounds_for_a_block():
    v, a = _case("trained", 130, 64)
    w, gs, row0, b = (0.3, 0.7), 2.0, 72, 56
    r = R.ref64(v, a, INV_T, w, gs, row0, b)
    e = R.emulate32(v, a, INV_T, w, gs, row0, b)
    assert R.excess(e, r, R.bounds(r, v, a, INV_T, w, gs, row0, b)) <= 1.0
    full = R.emulate32(v, a, INV_T, w, gs)
    assert np.array_equal(full["dv"][row0:row0 + b], e["dv"]) and np.array_equal(full["da"][row0:row0 + b], e["da"])


# (swapped log-sum-exps are looked for among unrelated rows only: a trained batch has a_i close to v_i, hence S close to
# symmetric and lse_v[i] close to lse_a[i] — there the swap changes little by construction)
@pytest.mark.parametrize("regime,defect", [(r, d) for r in ("unrelated", "trained")
                                           for d in ("no_delta", "swap_lse", "no_key_role", "b_for_G", "tau_twice", "drop_tail")
                                           if (r, d) != ("trained", "swap_lse")])
def test_named_defects_lie_ten_bounds_outside(regime, defect):
    v, a = _case(regime, 130, 64)
    w, gs, row0, b = (0.3, 0.7), 1.0, 32, 67
    r = R.ref64(v, a, INV_T, w, gs, row0, b)
    bd = R.bounds(r, v, a, INV_T, w, gs, row0, b)
    assert R.excess(R.emulate32(v, a, INV_T, w, gs, row0, b), r, bd) <= 1.0
    assert R.excess(R.emulate32(v, a, INV_T, w, gs, row0, b, defect=defect), r, bd) >= 10.0


@pytest.mark.parametrize("case,defect", [(R.extreme_small_tau, "fixed_shift"), (R.extreme_identical_pairs, "no_shift")])
def test_softmax_needs_the_true_running_maximum(case, defect):
    v, a, inv_T = case()
    r = R.ref64(v, a, inv_T)
    bd = R.bounds(r, v, a, inv_T)
    assert R.excess(R.emulate32(v, a, inv_T), r, bd) <= 1.0
    assert R.excess(R.emulate32(v, a, inv_T, defect=defect), r, bd) >= 10.0       # (inf: not finite)


def test_gap_check_fails_loudly():
    v, a = R.make_unrelated(8, 32, 1)
    a[5] = a[2]                                         # two equal keys: every row's scores tie there
    v[0] = a[2]
    assert not R._gap_ok(v, a, INV_T)
    with pytest.raises(AssertionError):
        R._make(16, 32, 0, INV_T, None, factor=1e8)     # no seed opens a gap of 1e8 bounds (more than the scores' range)


def test_restatement_matches_autograd_in_float64():
    rng = np.random.RandomState(11)
    G, D, R_ = 12, 32, 3                                 # three ranks of four: the gradient is the GLOBAL loss's
    v = torch.tensor(R._normalize64(rng.randn(G, D)), requires_grad=True)
    a = torch.tensor(R._normalize64(rng.randn(G, D)), requires_grad=True)
    w = (0.3, 0.7)
    S = v @ a.t() * INV_T
    tgt = torch.arange(G)
    loss = w[0] * torch.nn.functional.cross_entropy(S, tgt) + w[1] * torch.nn.functional.cross_entropy(S.t(), tgt)
    loss.backward()
    for rank in range(R_):
        r = R.ref64(v.detach().numpy(), a.detach().numpy(), INV_T, w, gs=float(R_), row0=4 * rank, b=4)
        assert abs(r["loss"] - float(loss.detach())) < 1e-14
        assert float(np.abs(r["dv"] / R_ - v.grad.numpy()[4 * rank:4 * rank + 4]).max()) < 1e-15
        assert float(np.abs(r["da"] / R_ - a.grad.numpy()[4 * rank:4 * rank + 4]).max()) < 1e-15


def test_header_ctypes_and_exports_agree():
    from avid_hip import lib, ops
    import criterions
    src = open(os.path.join(REPO, "include", "avid_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    proto = re.search(r"int avid_infonce\((.*?)\);", src, flags=re.S).group(1)
    kinds = []
    for arg in proto.split(","):
        arg = " ".join(arg.split())
        kinds.append(C.c_void_p if "*" in arg or "avid_stream_t" in arg else C.c_size_t if arg.startswith("size_t")
                     else C.c_float if arg.startswith("float") else C.c_int)
    assert lib.SIGNATURES["avid_infonce"] == (C.c_int, kinds)
    assert lib.SIGNATURES["avid_infonce_workspace_bytes"] == (C.c_size_t, [C.c_int])
    assert lib.version() >= 171
    ws = lib.raw("avid_infonce_workspace_bytes")
    assert ws(0) == 0 and ws(1) == 256 and ws(1030) == -(-20 * 1030 // 256) * 256 and ws(1 << 20) < 21 << 20     # O(G)
    assert criterions.__dict__["InfoNCE"] is criterions.InfoNCE and callable(ops.infonce) and callable(ops.infonce_workspace)


def test_c_entry_validates_before_any_launch():
    from avid_hip import lib
    call = lib.raw("avid_infonce")
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) // 16 * 16
    BADARG, UNSUPPORTED = -1, -4
    ok = dict(G=4, D=32, row0=0, b=4, v=p, a=p, inv_T=10.0, wv=0.5, wa=0.5, gs=1.0, loss=p, hits=p, dv=p, da=p, ws=p, wsb=256)

    def rc(**kw):
        k = {**ok, **kw}
        return call(k["G"], k["D"], k["row0"], k["b"], k["v"], k["a"], k["inv_T"], k["wv"], k["wa"], k["gs"], k["loss"], k["hits"],
                    k["dv"], k["da"], k["ws"], k["wsb"], None)
    for kw in (dict(G=0), dict(row0=-1), dict(row0=2, b=3), dict(b=-1), dict(v=None), dict(a=None), dict(loss=None), dict(ws=None),
               dict(wsb=255), dict(inv_T=0.0), dict(inv_T=float("inf")), dict(wv=-1.0), dict(wa=float("nan")), dict(dv=None),
               dict(v=p + 4)):
        assert rc(**kw) == BADARG and "infonce" in lib.last_error(), kw
    for D in (0, 16, 48, 544):
        assert rc(D=D) == UNSUPPORTED, D


def test_python_layers_refuse_bad_arguments_before_launch():
    import criterions
    from avid_hip import ops, AvidHipError
    x = torch.zeros(4, 32)
    with pytest.raises(AvidHipError):
        ops.infonce(x, x)                                                      # host tensors
    with pytest.raises(AvidHipError):
        criterions.InfoNCE(32)(x, x, torch.arange(4))
    for kw in (dict(embedding_dim=48), dict(embedding_dim=1024), dict(embedding_dim=128, temperature=0.0),
               dict(embedding_dim=128, v2a_coeff=0.0, a2v_coeff=0.0), dict(embedding_dim=128, v2a_coeff=-1.0)):
        with pytest.raises(ValueError):
            criterions.InfoNCE(**kw)
    # shapes and types are judged before the device: every message names what is wrong with them
    for v, a, match in ((torch.zeros(4, 32), torch.zeros(5, 32), "must be"), (torch.zeros(32), torch.zeros(32), "must be"),
                        (torch.zeros(4, 32, dtype=torch.float64), x, "float32"), (None, x, "tensor")):
        with pytest.raises(AvidHipError, match=match):
            ops.infonce(v, a)
    with pytest.raises(AvidHipError, match="no CPU fallback"):
        ops.infonce(x, x)


def test_criterion_interface():
    import criterions
    c = criterions.InfoNCE(128, device=0, temperature=0.1, v2a_coeff=1.0, a2v_coeff=3.0, num_data=12345)
    assert (c.v2a_coeff, c.a2v_coeff) == (0.25, 0.75) and c.temperature == 0.1
    assert len(c.state_dict()) == 0 and not list(c.parameters()) and not list(c.buffers())
    assert c.set_epoch(3) is None and not hasattr(c, "nce_average")
    # the loss section of a shipped AVID yaml (plus what main-avid.py adds) with only the name swapped
    c = criterions.__dict__["InfoNCE"](num_data=232067, num_negatives=1024, momentum=0.5, xModal_coeff=1., wModal_coeff=0.,
                                       embedding_dim=128, device=0)
    assert (c.v2a_coeff, c.a2v_coeff, c.temperature) == (0.5, 0.5, 0.07)
    with pytest.raises(TypeError):
        criterions.InfoNCE(128, temperatur=0.1)


def test_virtual_ranks_are_refused_with_an_in_batch_criterion():
    import criterions
    from avid_hip.parallel import TrainStep
    with pytest.raises(ValueError, match="in-batch"):
        TrainStep(torch.nn.Linear(4, 4), criterions.InfoNCE(128), virtual_ranks=2)
