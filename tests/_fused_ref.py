"""Inputs of the fused criterion kernels (``avid_xmodal_fused`` / ``avid_cma_fused``, D = 128) and the same arithmetic in float64
on the CPU (criterions/avid.py:52-71, criterions/avid_cma.py:150-194, 338-358, criterions/nce.py:38-58 with a frozen Z): shared
by tests/test_gpu_ops.py (the benchmark and golden sizes) and tests/test_gpu_embedding_widths.py (the block edges)."""
import types

import torch
import torch.nn.functional as F

from oracle import avid_oracle as O

T_ = 0.07


def xmodal_case(bs, K, N):
    """Cross-modal criterion: rows = [self | K negatives].  ``losses`` = [L_v2a, L_a2v, their mean, coeff * mean]; ``gv`` / ``ga``:
    d total / d raw embedding; ``vh`` / ``ah``: the normalised embeddings (all float64)."""
    gen = torch.Generator().manual_seed(bs * 1000 + K)
    v1 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    v2 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    ve = torch.randn(bs, 128, generator=gen) * 2
    ae = torch.randn(bs, 128, generator=gen) * 0.5
    y = torch.randperm(N, generator=gen)[:bs]
    idx = torch.randint(0, N - 1, (bs, K), generator=gen)
    idx = idx + (idx >= y[:, None]).long()
    Z, coeff = torch.tensor(0.83), 0.75
    vr, ar = ve.double().requires_grad_(True), ae.double().requires_grad_(True)
    vh, ah = F.normalize(vr, dim=1), F.normalize(ar, dim=1)
    rows = torch.cat([y[:, None], idx], 1)
    s_v2a = torch.bmm(v2.double()[rows], vh.unsqueeze(2)).squeeze(-1) / T_
    s_a2v = torch.bmm(v1.double()[rows], ah.unsqueeze(2)).squeeze(-1) / T_
    l1, _ = O.nce_loss(s_v2a[:, :1], s_v2a[:, 1:], Z.double())
    l2, _ = O.nce_loss(s_a2v[:, :1], s_a2v[:, 1:], Z.double())
    tot = (l1 / 2 + l2 / 2) * coeff
    tot.backward()
    return types.SimpleNamespace(v1=v1, v2=v2, ve=ve, ae=ae, y=y, idx=idx, rows=rows, Z=Z, coeff=coeff, T=T_, vh=vh.detach(),
                                 ah=ah.detach(), losses=[float(v.detach()) for v in (l1, l2, l1 / 2 + l2 / 2, tot)],
                                 gv=vr.grad, ga=ar.grad)


def cma_case(bs, P, K, Kw, N):
    """AVID+CMA stock term set: rows = [self | P positives | K negatives], the first Kw negatives also serve the within-modal
    terms.  ``losses`` = the four terms, the two group means, the total."""
    gen = torch.Generator().manual_seed(bs * 1000 + K + P)
    v1 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    v2 = F.normalize(torch.randn(N, 128, generator=gen), dim=1)
    ve = torch.randn(bs, 128, generator=gen) * 2
    ae = torch.randn(bs, 128, generator=gen) * 0.5
    y = torch.randperm(N, generator=gen)[:bs]
    pos = torch.randint(0, N, (bs, P), generator=gen)
    idx = torch.randint(0, N, (bs, K), generator=gen)
    Z, cI, cP = torch.tensor(0.83), 0.4, 0.6
    vr, ar = ve.double().requires_grad_(True), ae.double().requires_grad_(True)
    vh, ah = F.normalize(vr, dim=1), F.normalize(ar, dim=1)
    rows = torch.cat([y[:, None], pos, idx], 1)
    sc = lambda bank, e: torch.bmm(bank.double()[rows], e.unsqueeze(2)).squeeze(-1) / T_
    s_v2a, s_a2v, s_v2v, s_a2a = sc(v2, vh), sc(v1, ah), sc(v1, vh), sc(v2, ah)
    neg = slice(1 + P, None)
    wneg = slice(1 + P, 1 + P + Kw)
    l = [O.nce_loss(s_v2a[:, :1], s_v2a[:, neg], Z.double())[0], O.nce_loss(s_a2v[:, :1], s_a2v[:, neg], Z.double())[0],
         O.nce_loss(s_v2v[:, 1:1 + P], s_v2v[:, wneg], Z.double())[0], O.nce_loss(s_a2a[:, 1:1 + P], s_a2a[:, wneg], Z.double())[0]]
    gi, gp = l[0] / 2 + l[1] / 2, l[2] / 2 + l[3] / 2
    tot = gi * cI + gp * cP
    tot.backward()
    return types.SimpleNamespace(v1=v1, v2=v2, ve=ve, ae=ae, y=y, pos=pos, idx=idx, Z=Z, cI=cI, cP=cP, T=T_, vh=vh.detach(),
                                 ah=ah.detach(), losses=[float(v.detach()) for v in l + [gi, gp, tot]],
                                 gv=vr.grad, ga=ar.grad)
