"""The general fused criterion (``avid_crit_fused`` / ``ops.crit_fused``) without a GPU: its float64 restatement
(tests/_crit_ref.py) is pinned to tests/_fused_ref.py at the two stock term sets, to the oracle's AVID / AVID+CMA forward at a
joint and an all-groups term set and to the reference's own golden steps; the criterions' dispatch (``fused_ok``) and the
``tb_log`` they fill are compared with the unfused path on CPU tensors; the C-ABI entry refuses bad descriptors before it
launches anything."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _crit_ref as R
import _fused_ref as FR
from oracle import avid_oracle as O
from oracle import detgen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the float64 restatement
def test_stock_masks_reproduce_the_fused_reference():
    c = FR.xmodal_case(3, 70, 300)
    r = R.crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, None, c.idx, c.Z, R.X_INST, (c.coeff, 0., 0., 0.), 70)
    got = [r.losses[0], r.losses[1], r.losses[8], r.losses[12]]
    assert max(abs(g - w) / abs(w) for g, w in zip(got, c.losses)) <= 1e-12
    assert all(v == 0.0 for v in r.losses[2:8] + r.losses[9:12])
    assert max(rel(r.gv, c.gv), rel(r.ga, c.ga), rel(r.vh, c.vh), rel(r.ah, c.ah)) <= 1e-12
    c = FR.cma_case(4, 1, 33, 7, 200)
    r = R.crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, c.pos, c.idx, c.Z, R.X_INST | R.W_POS, (c.cI, 0., 0., c.cP), 7)
    got = [r.losses[0], r.losses[1], r.losses[6], r.losses[7], r.losses[8], r.losses[11], r.losses[12]]
    assert max(abs(g - w) / abs(w) for g, w in zip(got, c.losses)) <= 1e-12
    assert max(rel(r.gv, c.gv), rel(r.ga, c.ga), rel(r.vh, c.vh), rel(r.ah, c.ah)) <= 1e-12


# the bars of the reference-generated golden steps (tests/test_gpu_model.py): float32 rounding of a reference step
LOSS_RTOL, GRAD_RTOL, GRAD_ATOL = 5e-6, 2e-4, 2e-7


def test_joint_and_all_groups_agree_with_the_oracle():
    """float32 oracle (a port of the reference) against the float64 restatement."""
    c = R.crit_inputs(3, 0, 70, 300)
    ve, ae = c.ve.clone().requires_grad_(True), c.ae.clone().requires_grad_(True)
    total, tb, _ = O.avid_forward(ve, ae, c.y, c.idx, c.v1.clone(), c.v2.clone(), Z=c.Z, xModal_coeff=1.0, wModal_coeff=1.0)
    total.backward()
    r = R.crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, None, c.idx, c.Z, R.X_INST | R.W_INST, (0.5, 0.5, 0., 0.), 70)
    want = dict(zip(("v2a", "a2v", "v2v", "a2a"), r.losses[:4]), xModal=r.losses[8], wModal=r.losses[9])
    for k, w in want.items():
        np.testing.assert_allclose(float(tb[f"Loss/{k}"].detach()), w, rtol=LOSS_RTOL)
    np.testing.assert_allclose(float(total.detach()), r.losses[12], rtol=LOSS_RTOL)
    np.testing.assert_allclose(ve.grad.numpy(), r.gv.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(ae.grad.numpy(), r.ga.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)

    N, P, K, Kw, bs = 200, 5, 33, 7, 4
    c = R.crit_inputs(bs, 0, K, N)
    gen = torch.Generator().manual_seed(5)
    pset = torch.stack([torch.randperm(N, generator=gen)[:P].sort().values for _ in range(N)]).int()
    rand = torch.randint(0, N - P, (bs, K), generator=gen)
    coeffs = (1.0, 0.5, 2.0, 1.5)            # wModalInst on: the cross-modal instance scores again, its coefficient unused
    ve, ae = c.ve.clone().requires_grad_(True), c.ae.clone().requires_grad_(True)
    total, tb, _ = O.avid_cma_forward(ve, ae, c.y, rand, pset, c.v1.clone(), c.v2.clone(), Z=c.Z, num_negatives_within=Kw,
                                      coeffs=coeffs)
    total.backward()
    pos, neg = O.cma_memory_sampling(pset, c.y, rand)
    s = sum(coeffs)
    r = R.crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, pos, neg, c.Z, R.X_INST | R.X_POS | R.W_POS,
                   (coeffs[0] / s, 0., coeffs[2] / s, coeffs[3] / s), Kw)
    assert sorted(tb) == sorted(f"Loss/{R.TERMS[k]}" for k in (0, 1, 4, 5, 6, 7))
    for k in (0, 1, 4, 5, 6, 7):
        np.testing.assert_allclose(float(tb[f"Loss/{R.TERMS[k]}"]), r.losses[k], rtol=LOSS_RTOL)
    np.testing.assert_allclose(float(total.detach()), r.losses[12], rtol=LOSS_RTOL)
    np.testing.assert_allclose(ve.grad.numpy(), r.gv.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(ae.grad.numpy(), r.ga.numpy(), rtol=GRAD_RTOL, atol=GRAD_ATOL)


def det_bank(tag, N, D=128):
    return F.normalize(T(detgen.det_normalish(f"bank:{tag}", (N, D))), p=2, dim=1)


def test_reference_golden_second_steps(golden):
    """Step 1 (Z frozen: the step the fused kernel takes) of the reference's Joint-AVID and all-groups AVID+CMA golden runs."""
    g = golden("avid")
    N, bs, K = 300, 3, 16
    v1, v2 = det_bank("joint:v1", N), det_bank("joint:v2", N)
    v0, a0 = (T(detgen.det_normalish(f"avid:joint:{m}0", (bs, 128))) for m in "va")
    O.update_memory(v1, v2, F.normalize(v0, dim=1), F.normalize(a0, dim=1), T(g["joint_y0"]), (0.5, 0.5))
    v, a = (T(detgen.det_normalish(f"avid:joint:{m}1", (bs, 128))) for m in "va")
    r = R.crit_ref(v, a, v1, v2, T(g["joint_y1"]), None, T(g["joint_idx1"]), float(g["joint_Z1"]), R.X_INST | R.W_INST,
                   (0.5, 0.5, 0., 0.), K)
    want = dict(zip(("v2a", "a2v", "v2v", "a2a"), r.losses[:4]), xModal=r.losses[8], wModal=r.losses[9])
    for k, w in want.items():
        np.testing.assert_allclose(w, float(g[f"joint_tb1_Loss_{k}"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(r.losses[12], float(g["joint_loss1"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(r.gv.numpy(), g["joint_gv1"], rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(r.ga.numpy(), g["joint_ga1"], rtol=GRAD_RTOL, atol=GRAD_ATOL)

    g, gc = golden("cma_all"), golden("cma")
    N, K, Kw, bs = 500, 64, 16, 4
    v1, v2 = det_bank("cma:v1", N), det_bank("cma:v2", N)
    pset = T(gc["topk_consensus"]).int()
    v0, a0 = (T(detgen.det_normalish(f"cma_all:{m}0", (bs, 128))) for m in "va")
    O.update_memory(v1, v2, F.normalize(v0, dim=1), F.normalize(a0, dim=1), T(g["y0"]), (0.5, 0.5))
    v, a = (T(detgen.det_normalish(f"cma_all:{m}1", (bs, 128))) for m in "va")
    y = T(g["y1"])
    pos, neg = O.cma_memory_sampling(pset, y, T(g["rand1"]))
    cf = [float(x) for x in g["coeffs"]]
    r = R.crit_ref(v, a, v1, v2, y, pos, neg, float(g["Z1"]), R.X_INST | R.X_POS | R.W_POS, (cf[0], 0., cf[2], cf[3]), Kw)
    for k in (0, 1, 4, 5, 6, 7):
        np.testing.assert_allclose(r.losses[k], float(g[f"tb1_Loss_{R.TERMS[k]}"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(r.losses[12], float(g["loss1"]), rtol=LOSS_RTOL)
    np.testing.assert_allclose(r.gv.numpy(), g["gv1"], rtol=GRAD_RTOL, atol=GRAD_ATOL)
    np.testing.assert_allclose(r.ga.numpy(), g["ga1"], rtol=GRAD_RTOL, atol=GRAD_ATOL)


# ------------------------------------------------------------------------------------------------ the criterions' dispatch
AVID_SETS = ((1., 0.), (0., 1.), (1., 1.))                                        # (xModal_coeff, wModal_coeff)
CMA_SETS = ((1., 0., 0., 1.), (1., 0., 0., 0.), (0., 1., 0., 0.), (0., 0., 1., 0.), (0., 0., 0., 1.), (1., 0., 1., 0.),
            (0., 0., 1., 1.), (1., 0., 1., 1.), (1., 1., 1., 1.), (0.25, 0.25, 0.25, 0.25))      # (xInst, wInst, xPos, wPos)


def _cma(coeffs, N, K, Kw, P, D=128):
    """criterions.AVID_CMA without its constructor's correspondence search (a GPU op): banks on the CPU, a random positive set."""
    import criterions
    from criterions.avid_cma import AVIDSimilarityPositiveExpansion
    from criterions.nce import NCECriterion
    crit = criterions.AVID_CMA.__new__(criterions.AVID_CMA)
    torch.nn.Module.__init__(crit)
    xi, wi, xp, wp = coeffs
    crit.nce_average = AVIDSimilarityPositiveExpansion(memory_size=N, embedding_dim=D, num_negatives=K, num_negatives_within=Kw,
                                                       xModalInst=xi > 0, wModalInst=wi > 0, xModalPos=xp > 0, wModalPos=wp > 0,
                                                       sampling_args={"type": "consensus", "pos_k": P}, momentum=0.5, device=CPU)
    s = sum(coeffs)
    crit.xModalInstCoeff, crit.wModalInstCoeff, crit.xModalPosCoeff, crit.wModalPosCoeff = (c / s for c in coeffs)
    crit.criterion = NCECriterion(N)
    return crit


def _gpu_like(D):
    """What ``fused_ok`` looks at in an embedding: a 2-D float32 tensor on the GPU."""
    return types.SimpleNamespace(is_cuda=True, dim=lambda: 2, shape=(2, D), dtype=torch.float32)


def test_fused_ok_for_every_term_set(monkeypatch):
    import criterions
    from avid_hip import ops
    monkeypatch.setattr(ops, "FUSED_CRITERION", True)
    for D, want in ((128, True), (64, False)):
        e = _gpu_like(D)
        for xc, wc in AVID_SETS:
            crit = criterions.AVID(num_data=50, embedding_dim=D, num_negatives=8, xModal_coeff=xc, wModal_coeff=wc, device=CPU)
            assert bool(crit.nce_average.fused_ok(e, e)) is want, (D, xc, wc)
        for coeffs in CMA_SETS:
            assert bool(_cma(coeffs, 50, 8, 4, 3, D).nce_average.fused_ok(e, e)) is want, (D, coeffs)
    crit = criterions.AVID(num_data=50, embedding_dim=128, num_negatives=8, xModal_coeff=1., wModal_coeff=1., device=CPU)
    monkeypatch.setattr(ops, "FUSED_CRITERION", False)           # AVID_FUSED_CRITERION=0: the unfused chain for every set
    assert not crit.nce_average.fused_ok(_gpu_like(128), _gpu_like(128))
    assert not _cma(CMA_SETS[-1], 50, 8, 4, 3).nce_average.fused_ok(_gpu_like(128), _gpu_like(128))


@pytest.fixture
def cpu_ops(monkeypatch):
    """The ops both criterion paths call, as float64 torch on the CPU: the unfused chain op by op, the fused ops through
    tests/_crit_ref.py.  ``calls`` lists the fused ops that ran."""
    from avid_hip import ops
    calls = []
    monkeypatch.setattr(ops, "poll_device_errors", lambda dev: None)
    monkeypatch.setattr(ops, "l2_normalize", lambda x: F.normalize(x, dim=1))
    monkeypatch.setattr(ops, "bank_scores", lambda e, bank, rows, inv_T: torch.bmm(bank.double()[rows], e.unsqueeze(2)).squeeze(-1) * inv_T)
    monkeypatch.setattr(ops, "nce_loss", lambda sp, sn, Z: O.nce_loss(sp, sn, Z.double())[0])
    monkeypatch.setattr(ops, "bank_update", lambda *a: None)

    def pack(r, picks, n):
        losses = torch.tensor([r.losses[k] for k in picks] + [0.] * (n - len(picks)), dtype=torch.float64)
        return losses[len(picks) - 1], losses, torch.stack([r.vh, r.ah])

    def crit_fused(v, a, y, pos, idx, bv, ba, Z, inv_T, Kw, mask, coeffs, ws):
        calls.append(("crit_fused", mask, tuple(coeffs)))
        return pack(R.crit_ref(v, a, bv, ba, y, pos, idx, Z, mask, coeffs, Kw), range(13), 16)

    def xmodal_fused(v, a, y, idx, bv, ba, Z, inv_T, coeff, ws):
        calls.append(("xmodal_fused",))
        return pack(R.crit_ref(v, a, bv, ba, y, None, idx, Z, R.X_INST, (coeff, 0, 0, 0), idx.shape[1]), (0, 1, 8, 12), 4)

    def cma_fused(v, a, y, pos, idx, bv, ba, Z, inv_T, Kw, cI, cP, ws):
        calls.append(("cma_fused",))
        return pack(R.crit_ref(v, a, bv, ba, y, pos, idx, Z, R.X_INST | R.W_POS, (cI, 0, 0, cP), Kw), (0, 1, 6, 7, 8, 11, 12), 8)

    for f in (crit_fused, xmodal_fused, cma_fused):
        monkeypatch.setattr(ops, f.__name__, f)
    return calls


def _both_paths(crit, v, a, y, monkeypatch, calls):
    from avid_hip import ops
    crit.criterion.avg_exp_score.fill_(0.83)
    crit.criterion._z_ready = None
    monkeypatch.setattr(crit.nce_average, "fused_ok", lambda ve, ae: ops.FUSED_CRITERION, raising=False)
    out = []
    for fused in (False, True):
        monkeypatch.setattr(ops, "FUSED_CRITERION", fused)
        n = len(calls)
        out.append(crit(v, a, y))
        assert len(calls) == n + (1 if fused else 0)
    (t0, tb0), (t1, tb1) = out
    assert list(tb1) == list(tb0), (list(tb1), list(tb0))                 # the same keys in the same order
    for k in tb0:
        np.testing.assert_allclose(float(tb1[k]), float(tb0[k]), rtol=1e-9, atol=0, err_msg=k)
    np.testing.assert_allclose(float(t1), float(t0), rtol=1e-9)
    return calls[-1], tb1


def test_tb_log_and_total_equal_the_unfused_path_for_every_term_set(cpu_ops, monkeypatch):
    import criterions
    N, K, Kw, P, bs = 60, 12, 5, 3, 4
    c = R.crit_inputs(bs, P, K, N)
    v, a = c.ve.double(), c.ae.double()
    for xc, wc in AVID_SETS:
        crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, xModal_coeff=xc, wModal_coeff=wc, device=CPU)
        crit.nce_average.sample_negatives = lambda yy, KK: c.idx
        call, tb = _both_paths(crit, v, a, c.y, monkeypatch, cpu_ops)
        if wc == 0:
            assert call == ("xmodal_fused",)                              # the stock set keeps its own op
        else:
            assert call == ("crit_fused", (R.X_INST if xc else 0) | R.W_INST, (xc / (xc + wc), wc / (xc + wc), 0., 0.))
            assert list(tb) == [f"Loss/{k}" for k in (("v2a", "a2v") if xc else ()) + ("v2v", "a2a", "xModal", "wModal")]
    for coeffs in CMA_SETS:
        crit = _cma(coeffs, N, K, Kw, P)
        crit.nce_average.memory_sampling = lambda yy: (c.pos, c.idx)
        call, tb = _both_paths(crit, v, a, c.y, monkeypatch, cpu_ops)
        xi, wi, xp, wp = (x / sum(coeffs) for x in coeffs)
        if coeffs == (1., 0., 0., 1.):
            assert call == ("cma_fused",)
            continue
        mask = (R.X_INST if xi or wi else 0) | (R.X_POS if xp else 0) | (R.W_POS if wp else 0)
        assert call == ("crit_fused", mask, (xi, 0., xp, wp)), coeffs       # wModalInst: X_INST again, never W_INST
        assert list(tb) == [f"Loss/{R.TERMS[k]}" for k in range(8) if mask >> (k // 2) & 1]


# ------------------------------------------------------------------------------------------------ the C-ABI
BADARG, UNSUPPORTED = -1, -4           # include/avid_hip.h: AVID_E_BADARG, AVID_E_UNSUPPORTED


def test_descriptor_mirror_matches_the_header():
    from avid_hip import lib
    src = open(os.path.join(REPO, "include", "avid_hip.h")).read()
    body = re.search(r"typedef struct avid_crit_desc \{(.*?)\} avid_crit_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"[\s*]|\[\d+\]", "", f) for decl in re.findall(r"(?:const )?\w+\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [n for n, _ in lib.CritDesc._fields_]
    assert C.sizeof(lib.CritDesc) == 160 and lib.CritDesc.N.offset == 24 and lib.CritDesc.v_hat.offset == 120
    for name, bit in (("X_INST", 1), ("W_INST", 2), ("X_POS", 4), ("W_POS", 8)):
        assert re.search(rf"#define AVID_CRIT_{name} {bit}\b", src) and getattr(lib, f"CRIT_{name}") == bit
    assert lib.SIGNATURES["avid_crit_fused"][1][0] == C.POINTER(lib.CritDesc) and lib.version() >= 165


def test_crit_fused_refuses_bad_descriptors_before_launching():
    from avid_hip import lib
    call = lib.raw("avid_crit_fused")
    assert call(None, None, 0, None, None) == BADARG and "crit_fused" in lib.last_error()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)                   # never dereferenced: every call below is refused by the argument checks

    def desc(**kw):
        d = lib.CritDesc(bs=2, P=3, K=8, Kw=4, D=128, mask=13, N=10, v_emb=p, a_emb=p, y=p, pos=p, idx=p, bank_v=p, bank_a=p, Z=p,
                         inv_T=1.0, v_hat=p, a_hat=p, losses=p, dv=p, da=p)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    need = lib.raw("avid_crit_fused_workspace_bytes")(2, 3, 8)
    assert need > 0
    for d, code, word in ((desc(mask=0), BADARG, "mask"), (desc(mask=16), BADARG, "mask"), (desc(D=64), UNSUPPORTED, "D=64"),
                          (desc(Kw=9), BADARG, "Kw"), (desc(Kw=0), BADARG, "Kw"), (desc(P=0, mask=4), BADARG, "P >= 1"),
                          (desc(P=0, mask=9), BADARG, "P >= 1"), (desc(bs=0), BADARG, "bs"), (desc(losses=None), BADARG, "null"),
                          (desc(pos=None), BADARG, "null")):
        assert call(C.byref(d), p, need, None, None) == code, word
        assert word in lib.last_error(), (word, lib.last_error())
    assert call(C.byref(desc()), p, need - 1, None, None) == BADARG and "workspace" in lib.last_error()
    assert call(C.byref(desc()), None, need, None, None) == BADARG
    # the scratch holds what the stock forms' does, with eight loss terms per block and sample
    S = -(-(1 + 3 + 8) // 64)
    assert need == 2 * S * 2 * 128 * 4 + 2 * S * 8 * 8 + 2 * 8 * 8 + 3 * 4 + 2 * 2 * 4 + 64


def test_ops_crit_fused_refuses_cpu_tensors():
    from avid_hip import ops, AvidHipError
    z = torch.zeros(2, 128)
    with pytest.raises(AvidHipError):
        ops.crit_fused(z, z, torch.zeros(2, dtype=torch.int64), None, torch.zeros(2, 4, dtype=torch.int64), torch.zeros(9, 128),
                       torch.zeros(9, 128), torch.tensor(0.5), 1.0, 4, 3, (1., 1., 0., 0.), torch.zeros(8, dtype=torch.uint8))


def test_every_instantiation_is_spill_free_and_the_criterions_masks_keep_four_waves():
    """tools/kernel_resources.py on the built library: no ``crit_fused_kernel<MASK>`` spills or carries a private segment; the
    nine masks the criterions can produce stay within 128 registers (four waves per SIMD, as the stock forms run)."""
    from tools_path import kernel_table
    rows = {r["name"]: r for r in kernel_table() if r["name"].startswith(("crit_fused_kernel<", "crit_finish_kernel"))}
    assert sorted(rows) == sorted([f"crit_fused_kernel<{m}>" for m in range(1, 16)] + ["crit_finish_kernel"])
    for name, r in rows.items():
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"]) == (0, 0, 0), (name, r)
    for m in (1,) + R.AVID_MASKS + R.CMA_MASKS + (R.X_INST | R.W_POS,):
        assert rows[f"crit_fused_kernel<{m}>"]["vgpr_count"] <= 128, (m, rows[f"crit_fused_kernel<{m}>"]["vgpr_count"])


def test_timer_name_is_the_name_the_profiler_shows():
    """The launch is timed as ``crit_fused_kernel`` whatever the mask; tools/kernel_names.py maps rocprofv3's name to it."""
    from tools_path import timer_name
    assert timer_name("void avid::crit_fused_kernel<13>(avid::CritArgs)") == "crit_fused_kernel"
    assert timer_name("avid::crit_finish_kernel(avid::CritArgs)") == "crit_finish_kernel"
    src = open(os.path.join(REPO, "avid-cma_amd", "csrc", "criterion.hip")).read()
    assert 'ScopedTimer t(s, "crit_fused_kernel"' in src


def test_workspace_queries_answer_what_they_answered_when_the_bits_were_recorded(golden):
    """tests/golden/crit_fused_bits.npz (tools/record_crit_bits.py) holds the three workspace-size queries' answers for every
    (bs, P, K) of its cases, from the library the bits were recorded with: the queries answer the same today."""
    import tools_path  # noqa: F401
    import record_crit_bits as B
    want = golden("crit_fused_bits")["ws_queries"]
    assert want.dtype == np.int64 and want.shape == (len({B.bs_p_k(c) for c in B.cases()}), 6) and (want[:, 3:] > 0).all()
    assert np.array_equal(B.ws_queries(), want)
