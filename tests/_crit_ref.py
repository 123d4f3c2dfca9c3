"""The general fused criterion (``avid_crit_fused`` / ``ops.crit_fused``, D = 128) restated in float64 on the CPU: any term set of
criterions/avid.py:52-71 and criterions/avid_cma.py:150-194, 338-358 over criterions/nce.py:38-58 with a frozen Z.  Shared by
tests/test_crit_fused_host.py (pinned there to tests/_fused_ref.py, the oracle and the reference's golden steps) and
tests/test_gpu_crit_fused.py (the kernel against it).

Rows = [self | P positives | K negatives]; mask bits and what they score:
    X_INST  v2a = v_hat . bank_a, a2v = a_hat . bank_v : positive row 0, all K negatives
    W_INST  v2v = v_hat . bank_v, a2a = a_hat . bank_a : positive row 0, all K negatives
    X_POS   pos-v2a / pos-a2v : the P positives (mean over P), all K negatives
    W_POS   pos-v2v / pos-a2a : the P positives, the first Kw negatives
``losses`` (13 figures): the eight terms in that order (0.0 for a term that is off), the four group means, the total
= sum_g coeff_g (L_g,first / 2 + L_g,second / 2)."""
import types

import torch
import torch.nn.functional as F

from oracle import avid_oracle as O

T_ = 0.07
X_INST, W_INST, X_POS, W_POS = 1, 2, 4, 8
TERMS = ("inst-v2a", "inst-a2v", "inst-v2v", "inst-a2a", "pos-v2a", "pos-a2v", "pos-v2v", "pos-a2a")
AVID_MASKS = (W_INST, X_INST | W_INST)                                       # what criterions.AVID adds to the stock X_INST
CMA_MASKS = (X_INST, X_POS, W_POS, X_INST | X_POS, X_POS | W_POS, X_INST | X_POS | W_POS)     # ... AVID_CMA to X_INST | W_POS
STOCK_MASKS = (X_INST, X_INST | W_POS)


def crit_ref(ve, ae, v1, v2, y, pos, idx, Z, mask, coeffs, Kw, T=T_):
    """float64 criterion of one step.  ``ve`` / ``ae`` raw embeddings [bs][128], ``v1`` / ``v2`` the video / audio bank,
    ``pos`` [bs][P] or None, ``idx`` [bs][K].  Returns losses[13], d total / d raw embeddings, the normalised embeddings."""
    bs, K = idx.shape
    P = 0 if pos is None else pos.shape[1]
    vr, ar = ve.double().detach().clone().requires_grad_(True), ae.double().detach().clone().requires_grad_(True)
    vh, ah = F.normalize(vr, dim=1), F.normalize(ar, dim=1)
    rows = torch.cat([y.view(-1, 1)] + ([pos] if P else []) + [idx], 1)
    sc = lambda bank, e: torch.bmm(bank.double()[rows], e.unsqueeze(2)).squeeze(-1) / T     # noqa: E731
    Zd = torch.as_tensor(Z).double().reshape(())
    own, posi, neg, wneg = slice(0, 1), slice(1, 1 + P), slice(1 + P, None), slice(1 + P, 1 + P + Kw)
    zero = torch.zeros((), dtype=torch.float64)
    terms = [zero] * 8
    for bit, first, (cols_p, cols_n) in ((X_INST, 0, (own, neg)), (W_INST, 2, (own, neg)), (X_POS, 4, (posi, neg)),
                                         (W_POS, 6, (posi, wneg))):
        if not mask & bit:
            continue
        cross = bit in (X_INST, X_POS)
        s_v = sc(v2 if cross else v1, vh)        # the video embedding's scores: against the audio bank when cross-modal
        s_a = sc(v1 if cross else v2, ah)
        terms[first] = O.nce_loss(s_v[:, cols_p], s_v[:, cols_n], Zd)[0]
        terms[first + 1] = O.nce_loss(s_a[:, cols_p], s_a[:, cols_n], Zd)[0]
    groups = [terms[2 * g] / 2 + terms[2 * g + 1] / 2 for g in range(4)]
    total = sum(groups[g] * float(coeffs[g]) for g in range(4))
    if total.requires_grad:
        total.backward()
    gv = vr.grad if vr.grad is not None else torch.zeros_like(vr)
    ga = ar.grad if ar.grad is not None else torch.zeros_like(ar)
    return types.SimpleNamespace(losses=[float(t.detach()) for t in terms + groups + [total]], gv=gv, ga=ga, vh=vh.detach(),
                                 ah=ah.detach(), mask=mask, coeffs=tuple(float(c) for c in coeffs), Kw=Kw, P=P, K=K, rows=rows)


def crit_inputs(bs, P, K, N, seed=None):
    """Banks, embeddings (norms far from 1, as tests/_fused_ref.py), ids: a last-row id and — from bs = 3 on — a duplicate id in y."""
    gen = torch.Generator().manual_seed(bs * 1000 + K + P if seed is None else seed)
    v1 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    v2 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    ve = torch.randn(bs, 128, generator=gen) * 2
    ae = torch.randn(bs, 128, generator=gen) * 0.5
    y = torch.randperm(N, generator=gen)[:bs]
    y[0] = N - 1
    if bs >= 3:
        y[2] = y[1]
    pos = torch.randint(0, N, (bs, P), generator=gen) if P else None
    idx = torch.randint(0, N, (bs, K), generator=gen)
    idx[-1, -1] = N - 1
    return types.SimpleNamespace(v1=v1, v2=v2, ve=ve, ae=ae, y=y, pos=pos, idx=idx, Z=torch.tensor(0.83), T=T_, N=N, bs=bs)


COEFFS = (0.4, 0.3, 0.2, 0.1)


def crit_case(mask, bs, P, K, Kw, N, coeffs=COEFFS):
    """Inputs + the float64 figures for one (term set, shape)."""
    c = crit_inputs(bs, P, K, N)
    ref = crit_ref(c.ve, c.ae, c.v1, c.v2, c.y, c.pos, c.idx, c.Z, mask, coeffs, Kw)
    c.__dict__.update(ref.__dict__)
    return c
