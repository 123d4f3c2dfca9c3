"""End-to-end parity on a real MI355X against the golden vectors produced by the reference itself
(tests/golden/*.npz, tools/make_golden.py) and against the oracle at sizes it finishes in seconds;
plus size-independent properties at the BASELINE.json shapes."""
import numpy as np
import pytest
import torch

from oracle import avid_oracle as O
from oracle import detgen

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def load_det(module, tag):
    sd = module.state_dict()
    module.load_state_dict({k: T(detgen.det_param(f"{tag}:{k}", tuple(v.shape)).copy()).to(v.dtype)
                            for k, v in sd.items()})


BLOCKS = {
    "r2p1d_64_128_s2": ("r3d", 64, 128, (2, 2, 2), (2, 64, 4, 10, 12)),
    "r2p1d_64_64": ("r3d", 64, 64, (1, 1, 1), (2, 64, 3, 6, 7)),
    "b2d_64_128_s2": ("b2d", 64, 128, (2, 2), (2, 64, 9, 13)),
    "b2d_64_64": ("b2d", 64, 64, (1, 1), (2, 64, 5, 7)),
}


@pytest.mark.parametrize("tag", list(BLOCKS))
def test_blocks_vs_reference_golden(tag, golden, gpu_device, wino_mode, kernel_log):
    """BasicR2P1DBlock / Basic2DBlock fwd + bwd + running stats vs the reference's CPU outputs.
    Tolerance: 1e-4 relative to each tensor's scale (fp32 both sides, different summation order).
    ``wino_forced``: the same reference-generated fixtures through the Winograd kernels (every stride-1 (1,3,3) /
    3x3 layer of these blocks: 64 -> 64 with ragged tiles, 128 -> 128 = two column blocks x four chunks)."""
    from models.network_blocks import BasicR2P1DBlock, Basic2DBlock
    g = golden("blocks")
    kind, cin, cout, stride, xs = BLOCKS[tag]
    blk = (BasicR2P1DBlock if kind == "r3d" else Basic2DBlock)(cin, cout, stride=stride)
    load_det(blk, f"blk:{tag}")
    blk = blk.to(gpu_device).train()
    x = T(detgen.det_normalish(f"blk:{tag}:x", xs))
    if kind == "b2d":
        x = x.unsqueeze(2)
    xd = cl(x).to(gpu_device).requires_grad_(True)
    with kernel_log() as log:
        y = blk(xd)
        yl = y.permute(0, 4, 1, 2, 3)
        if kind == "b2d":
            yl = yl[:, :, 0]
        gy = T(detgen.det_uniform(f"blk:{tag}:g", tuple(yl.shape)))
        gyd = gy.unsqueeze(2) if kind == "b2d" else gy
        y.backward(cl(gyd).to(gpu_device))
    # stride-1 3x3 layers of the block: both spatial convs of an unstrided block, the second one of a strided block
    n_s1 = 2 if all(v == 1 for v in stride) else 1
    assert log.launches("wino_kernel") == (2 * n_s1 if wino_mode == "wino_forced" else 0), sorted(log.report)
    assert log.launches("wino2p_kernel") + log.launches("wino2_kernel") == (2 * n_s1 if wino_mode == "wino2_forced" else 0), sorted(log.report)

    def close(a, ref, tol):
        a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert a.shape == ref.shape
        assert np.abs(a - ref).max() <= tol * (np.abs(ref).max() + 1e-12), float(np.abs(a - ref).max())

    close(yl.detach().cpu().numpy(), g[f"{tag}_y"], 1e-4)
    gx = xd.grad.permute(0, 4, 1, 2, 3)
    close((gx[:, :, 0] if kind == "b2d" else gx).cpu().numpy(), g[f"{tag}_gx"], 2e-4)
    for n, p in blk.named_parameters():
        gg = p.grad.contiguous().cpu().numpy().reshape(-1)      # logical (reference) order
        close(gg[:8192], g[f"{tag}_g_{n}"], 5e-4)
        np.testing.assert_allclose(np.linalg.norm(gg.astype(np.float64)), g[f"{tag}_gnorm_{n}"], rtol=2e-4)
    for n, b in blk.named_buffers():
        close(b.cpu().numpy(), g[f"{tag}_buf_{n}"], 1e-5)


from oracle.hooks import capture_relu_masks, relu_flip_report, capture_pool_argmax, pool_pick_report  # noqa: E402


def _build_model(gpu_device, tag="w"):
    import models
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])
    load_det(m, tag)
    return m.to(gpu_device)


def test_return_embs_in_the_loss_keeps_exact_bn_gradients(gpu_device):
    """return_embs hands intermediate activations to the caller; with one of them in the loss a BatchNorm output
    has a second consumer, so the dgrad -> BatchNorm hand-over of the partial sums (ops.BnSource) must be off
    for that forward: gradients are then bit-identical to a run with the hand-over disabled globally, and the
    plain training forward (hand-over on) agrees with both to fp32 summation-order noise."""
    from avid_hip import ops
    m = _build_model(gpu_device).train().video_model
    video = T(detgen.det_normalish("embs:video", (2, 3, 8, 112, 112))).to(gpu_device)

    def run(return_embs, extra):
        for p in m.parameters():
            p.grad = None
        e = m(video, return_embs=True) if return_embs else {"pool": m(video)}
        loss = (e["pool"] ** 2).sum()
        if extra:
            loss = loss + (e["conv3x"] ** 2).sum() * 1e-3
        loss.backward()
        return [p.grad.clone() for p in m.parameters()]

    with_embs = run(True, True)
    saved, ops.FUSE_BN_BWD = ops.FUSE_BN_BWD, False
    try:
        plain_off = run(True, True)
        base_off = run(False, False)
    finally:
        ops.FUSE_BN_BWD = saved
    assert all(torch.equal(a, b) for a, b in zip(with_embs, plain_off))
    base_on = run(False, False)               # the normal training forward: hand-over active
    for a, b in zip(base_on, base_off):
        assert relerr(a, b) < 1e-4


def test_av_wrapper_vs_reference_golden(golden, gpu_device, wino_mode, kernel_log):
    """Config 1/2 parity case: 2 clips of 3x8x112x112 + 1x40x100 through R(2+1)D-18 + Conv2D + heads,
    train mode, against the reference's own CPU forward/backward.  Stated fp32 tolerance:
    embeddings 2e-4 of scale, gradients 2e-3 of scale (17 BN layers amplify summation-order noise).
    ``wino_forced``: conv2x (12544 pixels), conv3x (1568) and the audio blocks' stride-1 64 / 128-channel layers run
    on the Winograd kernels — the reference's own outputs pin them."""
    g = golden("av_wrapper")
    m = _build_model(gpu_device).train()
    video = T(detgen.det_normalish("in:video", (2, 3, 8, 112, 112))).to(gpu_device)
    audio = T(detgen.det_normalish("in:audio", (2, 1, 40, 100))).to(gpu_device)
    with kernel_log() as log:
        ve, ae = m(video, audio)
        gv = T(detgen.det_uniform("in:gv", (2, 128))).to(gpu_device)
        ga = T(detgen.det_uniform("in:ga", (2, 128))).to(gpu_device)
        ((ve * gv).sum() + (ae * ga).sum()).backward()
    # video: 4 (conv2x) + 3 (conv3x) stride-1 spatial layers, audio: one in block 1, one in block 2; x 2 directions
    assert log.launches("wino_kernel") == (2 * 9 if wino_mode == "wino_forced" else 0), sorted(log.report)
    assert log.launches("wino2p_kernel") + log.launches("wino2_kernel") == (2 * 9 if wino_mode == "wino2_forced" else 0), sorted(log.report)

    def err(a, ref):
        a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
        return np.abs(a - ref).max() / (np.abs(ref).max() + 1e-12)

    assert err(ve.detach().cpu().numpy(), g["video_emb"]) < 2e-4
    assert err(ae.detach().cpu().numpy(), g["audio_emb"]) < 2e-4
    # Gradients: the device and the reference's CPU run disagree on ~10 of ~2e7 ReLU signs (pre-activations
    # within fp32 noise of 0, measured by tools/gpu_debug.py mask); every flipped sign perturbs the
    # gradients upstream of it by O(1e-2) of their scale (only 32 samples/channel at conv5x with 2 clips; a
    # flipped hidden unit of a head zeroes one bias-gradient entry), and WHICH signs flip depends on the
    # summation order (tile / split-K plan).  Against the FIXED golden gradients the bound is therefore
    # flip-limited: cosine > 0.99 and norm within 5 %.  test_full_step_vs_oracle_bs4 pins the ReLU pattern
    # and checks every parameter's gradient to fp32 round-off (5e-4 of scale).
    grads = dict(m.named_parameters())
    for key in g.files:
        if key.startswith("grad:"):
            n = key[5:]
            gg = grads[n].grad.contiguous().cpu().numpy().reshape(-1)
            a, r = gg[:4096].astype(np.float64), g[key].astype(np.float64)
            cos = float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r) + 1e-30))
            assert cos > 0.99, (n, cos)
            np.testing.assert_allclose(np.linalg.norm(gg.astype(np.float64)), g[f"gradnorm:{n}"], rtol=5e-2)
        elif key.startswith("buf:"):
            np.testing.assert_allclose(m.state_dict()[key[4:]].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
    m.eval()
    with torch.no_grad():
        ve2, ae2 = m(video, audio)
        assert err(ve2.cpu().numpy(), g["eval_video_emb"]) < 2e-4
        assert err(ae2.cpu().numpy(), g["eval_audio_emb"]) < 2e-4
        e = m.video_model(video, return_embs=True)
        assert tuple(e["conv2x"].shape) == (2, 64, 8, 28, 28) and tuple(e["conv5x"].shape) == (2, 512, 1, 4, 4)
        for k, t in e.items():
            np.testing.assert_allclose(float(t.abs().mean()), g[f"eval_video_{k}_absmean"], rtol=2e-4)
        e = m.audio_model(audio, return_embs=True)
        assert tuple(e["conv5x"].shape) == (2, 512, 3, 7)
        for k, t in e.items():
            np.testing.assert_allclose(float(t.abs().mean()), g[f"eval_audio_{k}_absmean"], rtol=2e-4)


def det_bank(tag, N, D=128):
    return torch.nn.functional.normalize(T(detgen.det_normalish(f"bank:{tag}", (N, D))), p=2, dim=1)


def test_avid_two_steps_vs_reference_golden(golden, gpu_device):
    """criterions.AVID with injected negatives: loss, tb_log, d loss/d emb, Z and the updated bank rows
    for two consecutive steps vs the reference (tests/golden/avid.npz)."""
    import criterions
    g = golden("avid")
    for tag, (N, bs, K, xc, wc) in {"cross": (1000, 4, 64, 1.0, 0.0), "joint": (300, 3, 16, 1.0, 1.0)}.items():
        crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, xModal_coeff=xc,
                               wModal_coeff=wc, device=gpu_device.index)
        assert sorted(crit.state_dict().keys()) == list(g[f"{tag}_state_keys"])
        crit.nce_average.view1_mem.copy_(det_bank(f"{tag}:v1", N))
        crit.nce_average.view2_mem.copy_(det_bank(f"{tag}:v2", N))
        for step in range(2):
            v = T(detgen.det_normalish(f"avid:{tag}:v{step}", (bs, 128))).to(gpu_device).requires_grad_(True)
            a = T(detgen.det_normalish(f"avid:{tag}:a{step}", (bs, 128))).to(gpu_device).requires_grad_(True)
            y = T(g[f"{tag}_y{step}"]).to(gpu_device)
            idx = T(g[f"{tag}_idx{step}"]).to(gpu_device)
            crit.nce_average.sample_negatives = lambda yy, KK, _i=idx: _i
            loss, tb = crit(v, a, y)
            loss.backward()
            np.testing.assert_allclose(loss.item(), g[f"{tag}_loss{step}"], rtol=5e-6)
            np.testing.assert_allclose(float(crit.criterion.avg_exp_score), g[f"{tag}_Z{step}"], rtol=5e-6)
            for k in tb:
                np.testing.assert_allclose(float(tb[k]), g[f"{tag}_tb{step}_{k.replace('/', '_')}"], rtol=5e-6)
            np.testing.assert_allclose(v.grad.cpu().numpy(), g[f"{tag}_gv{step}"], rtol=2e-4, atol=2e-7)
            np.testing.assert_allclose(a.grad.cpu().numpy(), g[f"{tag}_ga{step}"], rtol=2e-4, atol=2e-7)
            np.testing.assert_allclose(crit.nce_average.view1_mem[y].cpu().numpy(), g[f"{tag}_v1rows{step}"],
                                       rtol=2e-6, atol=2e-7)
            np.testing.assert_allclose(crit.nce_average.view2_mem[y].cpu().numpy(), g[f"{tag}_v2rows{step}"],
                                       rtol=2e-6, atol=2e-7)


def test_avid_sampler_contract(gpu_device):
    """Un-injected path at the Kinetics-scale bank: negatives uniform over [0,N) minus {y}."""
    import criterions
    N, bs, K = 240000, 64, 1024
    crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, device=gpu_device.index)
    y = torch.randperm(N)[:bs].to(gpu_device)
    idx = crit.nce_average.sample_negatives(y, K)
    assert idx.shape == (bs, K) and idx.dtype == torch.int64
    assert int(idx.min()) >= 0 and int(idx.max()) < N and not bool((idx == y[:, None]).any())
    idx2 = crit.nce_average.sample_negatives(y, K)
    assert not torch.equal(idx, idx2)                               # the stream advances
    # chi-square over 64 equal bins of [0,N): 65536 draws, dof 63 -> 99.99th percentile ~ 115
    hist = torch.histc(idx.float(), bins=64, min=0, max=N).cpu().numpy()
    chi2 = ((hist - hist.mean()) ** 2 / hist.mean()).sum()
    assert chi2 < 130, chi2
    v = torch.randn(bs, 128, device=gpu_device, requires_grad=True)
    a = torch.randn(bs, 128, device=gpu_device, requires_grad=True)
    before = crit.nce_average.view1_mem.clone()
    loss, tb = crit(v, a, y)
    loss.backward()
    assert torch.isfinite(loss) and set(tb) == {"Loss/v2a", "Loss/a2v", "Loss/xModal", "Loss/wModal"}
    changed = (crit.nce_average.view1_mem != before).any(1).nonzero().flatten()
    assert set(changed.tolist()) == set(y.tolist())                 # only the batch's rows moved
    np.testing.assert_allclose(crit.nce_average.view1_mem[y].norm(dim=1).cpu().numpy(), 1.0, rtol=1e-5)


def test_avid_cma_vs_reference_golden(golden, gpu_device):
    import criterions
    from criterions.avid_cma import AVIDSimilarityPositiveExpansion
    from criterions.nce import NCECriterion
    g = golden("cma")
    N, Pk, K, Kw, bs = 500, 32, 64, 16, 4
    crit = criterions.AVID_CMA.__new__(criterions.AVID_CMA)
    torch.nn.Module.__init__(crit)
    na = AVIDSimilarityPositiveExpansion(memory_size=N, embedding_dim=128, num_negatives=K, num_negatives_within=Kw,
                                         sampling_args={"type": "consensus", "pos_k": Pk}, momentum=0.5,
                                         device=gpu_device.index)
    na.view1_mem.copy_(det_bank("cma:v1", N))
    na.view2_mem.copy_(det_bank("cma:v2", N))
    na.register_buffer("positive_set", T(g["topk_consensus"]).int().to(gpu_device))
    crit.nce_average = na
    crit.xModalInstCoeff, crit.wModalInstCoeff, crit.xModalPosCoeff, crit.wModalPosCoeff = 0.5, 0.0, 0.0, 0.5
    crit.criterion = NCECriterion(N).to(gpu_device)
    y = T(g["ms_y"]).to(gpu_device)
    rand_idx = T(g["ms_rand"]).to(gpu_device)
    na.multinomial.draw = lambda n, _r=rand_idx: _r.reshape(-1)
    v = T(detgen.det_normalish("cma:v", (bs, 128))).to(gpu_device).requires_grad_(True)
    a = T(detgen.det_normalish("cma:a", (bs, 128))).to(gpu_device).requires_grad_(True)
    loss, tb = crit(v, a, y)
    loss.backward()
    np.testing.assert_allclose(loss.item(), g["cma_loss"], rtol=5e-6)
    np.testing.assert_allclose(float(crit.criterion.avg_exp_score), g["cma_Z"], rtol=5e-6)
    for k in tb:
        np.testing.assert_allclose(float(tb[k]), g[f"cma_tb_{k.replace('/', '_')}"], rtol=5e-6)
    np.testing.assert_allclose(v.grad.cpu().numpy(), g["cma_gv"], rtol=2e-4, atol=2e-7)
    np.testing.assert_allclose(a.grad.cpu().numpy(), g["cma_ga"], rtol=2e-4, atol=2e-7)
    np.testing.assert_allclose(na.view1_mem[y].cpu().numpy(), g["cma_v1rows"], rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(na.view2_mem[y].cpu().numpy(), g["cma_v2rows"], rtol=2e-6, atol=2e-7)


def test_avid_cma_all_four_terms_vs_reference_golden(golden, gpu_device):
    """All four score groups active (tests/golden/cma_all.npz, generated from the reference): two steps, six loss
    terms, carried Z, bank rows — the HIP criterion against the reference's own numbers."""
    import criterions
    from criterions.avid_cma import AVIDSimilarityPositiveExpansion
    from criterions.nce import NCECriterion
    g, gc = golden("cma_all"), golden("cma")
    N, Pk, K, Kw, bs = 500, 32, 64, 16, 4
    crit = criterions.AVID_CMA.__new__(criterions.AVID_CMA)
    torch.nn.Module.__init__(crit)
    na = AVIDSimilarityPositiveExpansion(memory_size=N, embedding_dim=128, num_negatives=K, num_negatives_within=Kw,
                                         xModalInst=True, wModalInst=True, xModalPos=True, wModalPos=True,
                                         sampling_args={"type": "consensus", "pos_k": Pk}, momentum=0.5,
                                         device=gpu_device.index)
    na.view1_mem.copy_(det_bank("cma:v1", N))
    na.view2_mem.copy_(det_bank("cma:v2", N))
    na.register_buffer("positive_set", T(gc["topk_consensus"]).int().to(gpu_device))
    crit.nce_average = na
    crit.xModalInstCoeff, crit.wModalInstCoeff, crit.xModalPosCoeff, crit.wModalPosCoeff = (float(c) for c in g["coeffs"])
    crit.criterion = NCECriterion(N).to(gpu_device)
    for step in range(2):
        y = T(g[f"y{step}"]).to(gpu_device)
        rand_idx = T(g[f"rand{step}"]).to(gpu_device)
        na.multinomial.draw = lambda n, _r=rand_idx: _r.reshape(-1)
        v = T(detgen.det_normalish(f"cma_all:v{step}", (bs, 128))).to(gpu_device).requires_grad_(True)
        a = T(detgen.det_normalish(f"cma_all:a{step}", (bs, 128))).to(gpu_device).requires_grad_(True)
        loss, tb = crit(v, a, y)
        loss.backward()
        assert sorted(tb.keys()) == list(g[f"tb_keys{step}"])
        np.testing.assert_allclose(loss.item(), g[f"loss{step}"], rtol=5e-6)
        np.testing.assert_allclose(float(crit.criterion.avg_exp_score), g[f"Z{step}"], rtol=5e-6)
        for k in tb:
            np.testing.assert_allclose(float(tb[k]), g[f"tb{step}_{k.replace('/', '_')}"], rtol=5e-6)
        np.testing.assert_allclose(v.grad.cpu().numpy(), g[f"gv{step}"], rtol=2e-4, atol=2e-7)
        np.testing.assert_allclose(a.grad.cpu().numpy(), g[f"ga{step}"], rtol=2e-4, atol=2e-7)
        np.testing.assert_allclose(na.view1_mem[y].cpu().numpy(), g[f"v1rows{step}"], rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(na.view2_mem[y].cpu().numpy(), g[f"v2rows{step}"], rtol=2e-6, atol=2e-7)


def test_criterion_checkpoint_restore(tmp_path, gpu_device):
    """criterions/avid.py:187-200 / avid_cma.py:308-319: banks and the partition function are restored from the
    'train_criterion' entry of an AVID checkpoint; Z is the MEAN of every '*avg_exp_score' entry and the reference
    stores it with shape (1,) after the first step (the nce.py:35 quirk)."""
    import criterions
    N = 300
    gen = torch.Generator().manual_seed(9)
    v1 = torch.nn.functional.normalize(torch.randn(N, 128, generator=gen), dim=1)
    v2 = torch.nn.functional.normalize(torch.randn(N, 128, generator=gen), dim=1)
    ckp = {"train_criterion": {"nce_average.view1_mem": v1, "nce_average.view2_mem": v2,
                               "criterion.avg_exp_score": torch.tensor([0.25]),
                               "criterion_extra.avg_exp_score": torch.tensor([0.75])}}
    path = str(tmp_path / "avid.pth.tar")
    torch.save(ckp, path)
    crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=32, momentum=0.5, checkpoint=path,
                           device=gpu_device.index)
    assert torch.equal(crit.nce_average.view1_mem.cpu(), v1) and torch.equal(crit.nce_average.view2_mem.cpu(), v2)
    np.testing.assert_allclose(float(crit.criterion.avg_exp_score), 0.5, rtol=1e-7)
    cma = criterions.AVID_CMA(num_data=N, embedding_dim=128, num_negatives=32, num_negatives_within=8, momentum=0.5,
                              sampling_args={"type": "consensus", "pos_k": 8}, checkpoint=path,
                              device=gpu_device.index)
    assert torch.equal(cma.nce_average.view1_mem.cpu(), v1)
    np.testing.assert_allclose(float(cma.criterion.avg_exp_score), 0.5, rtol=1e-7)
    want = O.cma_topk(v1, v2, 8, "consensus")                     # the constructor searched the RESTORED banks
    got = cma.nce_average.positive_set.cpu().numpy()
    assert np.mean([set(got[i]) == set(want[i]) for i in range(N)]) > 0.99
    # a step with the restored Z does not re-estimate it
    v = torch.randn(4, 128, device=gpu_device, requires_grad=True)
    a = torch.randn(4, 128, device=gpu_device, requires_grad=True)
    loss, _ = crit(v, a, torch.tensor([1, 5, 9, 200], device=gpu_device))
    loss.backward()
    np.testing.assert_allclose(float(crit.criterion.avg_exp_score), 0.5, rtol=1e-7)
    sd = crit.state_dict()
    assert sorted(sd) == ["criterion.avg_exp_score", "nce_average.view1_mem", "nce_average.view2_mem"]


def _full_step_vs_oracle(gpu_device, bs, N, K, video, audio, y, idx, v1, v2, min_elements, flip_bound=1e-4):
    """model fwd -> AVID (injected idx) -> bwd on the device against the oracle (free-running, then with the device's
    ReLU pattern pinned).  Returns the kernel log of the device run."""
    import criterions
    from avid_hip import lib
    m = _build_model(gpu_device).train()
    crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, device=gpu_device.index)
    crit.nce_average.view1_mem.copy_(v1)
    crit.nce_average.view2_mem.copy_(v2)
    idx_d = idx.to(gpu_device)
    crit.nce_average.sample_negatives = lambda yy, KK: idx_d
    masks, remove = capture_relu_masks(m)
    picks, remove_picks = capture_pool_argmax(m)
    lib.timing_enable(True)
    e1, e2 = m(video.to(gpu_device), audio.to(gpu_device))
    remove()
    remove_picks()
    assert sorted(picks) == ["audio_model.pool", "video_model.conv1.pool", "video_model.pool"]
    loss, _ = crit(e1, e2, y.to(gpu_device))
    loss.backward()
    torch.cuda.synchronize()
    report = lib.timing_report()
    lib.timing_enable(False)

    # the same step unhooked: the launch program (the benchmark's kernels, AFF forms included) — bit-identical to the hooked
    # per-layer run above, so that every bar below holds for the program path too
    m2 = _build_model(gpu_device).train()
    crit2 = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, device=gpu_device.index)
    crit2.nce_average.view1_mem.copy_(v1)
    crit2.nce_average.view2_mem.copy_(v2)
    crit2.nce_average.sample_negatives = lambda yy, KK: idx_d
    aff = lib.raw("avid_debug_in_affine_launches")
    aff0 = aff(1)
    f1, f2 = m2(video.to(gpu_device), audio.to(gpu_device))
    assert type(f1.grad_fn).__name__.startswith("NetFn"), type(f1.grad_fn).__name__
    loss2, _ = crit2(f1, f2, y.to(gpu_device))
    loss2.backward()
    torch.cuda.synchronize()
    if bs == 64:
        assert aff(1) - aff0 == 8, aff(1) - aff0        # conv2x's four temporal forwards and weight gradients in the AFF forms
    assert torch.equal(f1.detach(), e1.detach()) and torch.equal(f2.detach(), e2.detach())
    assert loss2.item() == loss.item()
    # every gradient bit-identical, except the weights of the small layers the program's grouped weight-gradient launches
    # serve (avid_conv_wgrad_group, read from the compiled program): outside the step engine the per-layer path gives each its
    # own launch, the same products summed in another order over pixel chunks (1e-5: test_gpu_ops.test_grouped_weight_gradients)
    from avid_hip import plan as P_
    pls = [p for p in m2.__dict__.get("_avid_plans", {}).values() if p]
    assert len(pls) == 1
    pl = pls[0]
    at = {4 * o: i for i, o in enumerate(pl.goff)}
    grouped_ids = {id(pl.params[at[pl.bwd_prog[k].t[2].off]]) for k in range(pl.n_bwd) if pl.bwd_prog[k].op == P_.OP_WGRAD_ITEM}
    assert len(grouped_ids) == {4: 39, 64: 33}[bs]
    same = grouped = 0
    for (n, p), p2 in zip(m.named_parameters(), m2.parameters()):
        if id(p2) in grouped_ids:
            assert float((p2.grad - p.grad).abs().max() / p.grad.abs().max()) < 1e-5, n
            grouped += 1
        else:
            assert torch.equal(p.grad, p2.grad), n
            same += 1
    assert (same, grouped) == (141 - len(grouped_ids), len(grouped_ids))
    del m2, crit2, f1, f2, loss2

    P = O.det_state(O.av_wrapper_spec(18), "w")
    pn = [n for n in P if not ("running" in n or "num_batches" in n)]
    for n in pn:
        P[n].requires_grad_(True)
    # (a) free-running oracle: forward quantities agree to fp32 round-off, and the device's ReLU pattern (the one
    # pinned in (b)) differs from the oracle's OWN pattern on at most 2e-6 of the signs, every one of them a
    # pre-activation within 1e-4 of its layer's RMS of zero — a wrong mask in a fused epilogue cannot hide in (b)
    O.PREACT, O.POOL_INPUT = {}, {}
    try:
        with torch.no_grad():
            ve0, ae0 = O.av_forward(video, audio, {k: v.detach().clone() for k, v in P.items()}, 18, True)
        flips, elements, worst = relu_flip_report(masks, O.PREACT)
        pool_dis, pool_n, pool_worst = pool_pick_report(picks, O.POOL_INPUT)
    finally:
        O.PREACT = O.POOL_INPUT = None
    assert float((e1.detach().cpu() - ve0).abs().max() / ve0.abs().max()) < 2e-4
    assert float((e2.detach().cpu() - ae0).abs().max() / ae0.abs().max()) < 2e-4
    assert elements > min_elements and flips <= 2e-6 * elements and worst < flip_bound, \
        (flips, elements, worst, relu_flip_report.worst_layer)
    # the global max-pools' selections: the device and the free-running oracle may pick different positions only
    # between two activations that are equal to within fp32 summation noise (<= 1e-4 of the tensor's RMS), and on at
    # most 1e-5 of the selections (the stem's (1,3,3) pool included: 25.7 M windows at 64 clips)
    assert pool_n == 2 * bs * 512 + bs * 64 * 8 * 28 * 28 and pool_dis <= max(2, 1e-5 * pool_n) and pool_worst < 1e-4, \
        (pool_dis, pool_n, pool_worst)
    # (b) oracle with the device's ReLU pattern and max-pool selections pinned: loss and ALL 141 parameter gradients
    # to 5e-4 of scale
    O.RELU_MASKS, O.POOL_ARGMAX = masks, picks
    try:
        ve, ae = O.av_forward(video, audio, P, 18, True)
        ref_loss, _, _ = O.avid_forward(ve, ae, y, idx, v1.clone(), v2.clone(), None, 0.5)
        ref_loss.backward()
    finally:
        O.RELU_MASKS = O.POOL_ARGMAX = None
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-5)
    worst = ("", 0.0)
    checked = 0
    for n, p in m.named_parameters():
        a, r = p.grad.contiguous().cpu().double(), P[n].grad.double()
        e = float((a - r).abs().max() / (r.abs().max() + 1e-30))
        worst = max(worst, (n, e), key=lambda t: t[1])
        checked += 1
    assert checked == 141 and worst[1] < 5e-4, worst
    return report


def test_full_step_vs_oracle_bs4(gpu_device):
    """BASELINE config 2 parity shape (bs=4, 3x8x112x112 + 1x40x100, K=1024) against the oracle:
    model fwd -> AVID (injected idx) -> bwd.  Loss to 1e-5, embeddings 2e-4, all 141 gradients to 5e-4 of scale."""
    N, bs, K = 1000, 4, 1024
    video = T(detgen.det_normalish("step:video", (bs, 3, 8, 112, 112)))
    audio = T(detgen.det_normalish("step:audio", (bs, 1, 40, 100)))
    y = T(detgen.det_indices("step:y", bs, N))
    draw = detgen.det_indices("step:draw", bs * K, N - 1)
    idx = T(O.sample_negatives_from_draw(draw, y.numpy(), K))
    v1, v2 = det_bank("step:v1", N), det_bank("step:v2", N)
    _full_step_vs_oracle(gpu_device, bs, N, K, video, audio, y, idx, v1, v2, 1.5e7)


def test_full_step_vs_oracle_bs64(gpu_device):
    """BASELINE config 2 at the batch its metric is quoted on (bs = 64 per GPU, 240k-row banks, K = 1024) against
    the oracle — the code paths of the benchmark step, which differ from the bs = 4 case: Winograd at conv2x AND
    conv3x (128 -> 128: two column blocks x four chunks), conv4x (256 -> 256) and audio block 1, the Winograd weight gradients, the bs-64 K-split plans of
    conv4x / conv5x, the grouped small-layer weight gradients, the separate finalize + apply BatchNorm launches of
    the large layers.  Same bars as bs = 4: loss 1e-5, embeddings 2e-4, ReLU pattern vs the free-running oracle
    (<= 2e-6 of 2.9e8 signs, near-zero pre-activations only), all 141 parameter gradients 5e-4 of their scale.
    The "near zero" bound is 2e-4 of the layer RMS here (1e-4 at bs = 4): it is the extreme of 16x more signs
    (measured: 398 flips of 291.9 M, the largest at 1.06e-4 of its layer's RMS), while two fp32 summation orders differ
    by up to 5e-5 of the scale in the late layers (K up to 4608)."""
    N, bs, K = 240_000, 64, 1024
    g = torch.Generator().manual_seed(20260928)
    video = torch.randn(bs, 3, 8, 112, 112, generator=g)
    audio = torch.randn(bs, 1, 40, 100, generator=g)
    y = torch.randperm(N, generator=g)[:bs]
    idx = torch.randint(0, N - 1, (bs, K), generator=g)
    idx = idx + (idx >= y[:, None]).long()                              # criterions/avid.py:85
    v1 = torch.nn.functional.normalize(torch.randn(N, 128, generator=g), dim=1)
    v2 = torch.nn.functional.normalize(torch.randn(N, 128, generator=g), dim=1)
    report = _full_step_vs_oracle(gpu_device, bs, N, K, video, audio, y, idx, v1, v2, 2.5e8, flip_bound=2e-4)
    wino = sum(v["launches"] for k, v in report.items() if k.startswith(("wino_kernel", "wino2_kernel", "wino2p_kernel")))
    assert any(k.startswith("wino2p_kernel") for k in report)     # conv2x / conv3x have the 64-tile units wino2_kernel wants; its default form is wino2p_kernel
    # conv2x 4 + conv3x 3 + conv4x 3 layers of the video tower and the stride-1 layer of audio block 1, forward and
    # input gradient
    assert wino == 22, (wino, sorted(report))


def test_properties_at_baseline_batch(gpu_device):
    """Size-independent properties at the throughput batch (bs=64 per GPU, N=240k, K=1024):
    (1) eval-mode embeddings of a clip do not depend on its batch-mates; (2) two identical train
    steps are bit-identical (deterministic kernels, no atomics); (3) BN outputs are standardised."""
    import criterions
    from avid_hip import ops
    bs = 64
    m = _build_model(gpu_device)
    g = torch.Generator().manual_seed(1234)
    video = torch.randn(bs, 3, 8, 112, 112, generator=g).to(gpu_device)
    audio = torch.randn(bs, 1, 40, 100, generator=g).to(gpu_device)
    m.eval()
    with torch.no_grad():
        v_all, a_all = m(video, audio)
        v_one, a_one = m(video[5:7], audio[5:7])
    assert float((v_all[5:7] - v_one).abs().max() / v_all.abs().max()) < 1e-5
    assert float((a_all[5:7] - a_one).abs().max() / a_all.abs().max()) < 1e-5

    def one_step():
        mm = _build_model(gpu_device).train()
        crit = criterions.AVID(num_data=240000, embedding_dim=128, num_negatives=1024, momentum=0.5,
                               device=gpu_device.index)
        gg = torch.Generator().manual_seed(7)
        crit.nce_average.view1_mem.copy_(torch.nn.functional.normalize(torch.randn(240000, 128, generator=gg), dim=1))
        crit.nce_average.view2_mem.copy_(torch.nn.functional.normalize(torch.randn(240000, 128, generator=gg), dim=1))
        crit.nce_average.multinomial.reseed(42, 0)
        y = torch.randperm(240000, generator=gg)[:bs].to(gpu_device)
        e1, e2 = mm(video, audio)
        loss, _ = crit(e1, e2, y)
        loss.backward()
        return loss.item(), mm.video_model.conv1[0].weight.grad.clone(), crit.nce_average.view1_mem[y].clone()

    l1, g1, r1 = one_step()
    l2, g2, r2 = one_step()
    assert l1 == l2 and torch.equal(g1, g2) and torch.equal(r1, r2)
    assert np.isfinite(l1)

    x = torch.randn(bs * 8 * 28 * 28, 64, generator=g).to(gpu_device) * 3 + 1
    one, zero = torch.ones(64, device=gpu_device), torch.zeros(64, device=gpu_device)
    y = ops.batch_norm_cl(x.view(bs, 8, 28, 28, 64), one, zero, zero.clone(), one.clone(), True, 0.1, 1e-5, False)
    y = y.view(-1, 64)
    assert float(y.mean(0).abs().max()) < 1e-4 and float((y.var(0, unbiased=False) - 1).abs().max()) < 1e-3


def test_graph_replay_equals_eager(gpu_device):
    """A captured hipGraph of the whole step (TrainStep.capture/replay) advances the alias RNG stream and
    the Adam step on the device and reproduces the eager steps bit for bit."""
    import criterions
    from avid_hip.parallel import TrainStep
    bs, N, K = 4, 5000, 256

    def make():
        torch.manual_seed(0)
        m = _build_model(gpu_device).train()
        crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, device=gpu_device.index)
        gg = torch.Generator().manual_seed(3)
        crit.nce_average.view1_mem.copy_(torch.nn.functional.normalize(torch.randn(N, 128, generator=gg), dim=1))
        crit.nce_average.view2_mem.copy_(torch.nn.functional.normalize(torch.randn(N, 128, generator=gg), dim=1))
        crit.nce_average.multinomial.reseed(11, 0)
        return m, crit, TrainStep(m, crit)

    g = torch.Generator().manual_seed(5)
    video = torch.randn(bs, 3, 8, 64, 64, generator=g).to(gpu_device)
    audio = torch.randn(bs, 1, 40, 100, generator=g).to(gpu_device)
    ids = torch.stack([torch.randperm(N, generator=g)[:bs] for _ in range(6)]).to(gpu_device)

    m1, c1, e1 = make()
    eager = [float(e1.step(video, audio, ids[i])) for i in range(6)]
    m2, c2, e2 = make()
    got = [float(e2.step(video, audio, ids[i])) for i in range(3)]
    e2.capture(video, audio, ids[3])                 # the capture itself executes nothing
    got += [float(e2.replay(index=ids[i])) for i in range(3, 6)]
    assert got == eager, (got, eager)
    assert torch.equal(m1.video_model.conv1[0].weight, m2.video_model.conv1[0].weight)
    assert torch.equal(c1.nce_average.view1_mem, c2.nce_average.view1_mem)
    assert int(e2.t_dev) == 6 and int(c2.nce_average.multinomial.offset_dev) == 6


def test_cma_topk_vs_reference_golden(golden, gpu_device):
    """find_correspondences on the 500 x 128 golden banks: all four agreement types vs the reference's
    CMASampler output (sets compared; at most one boundary tie may differ per row), rows sorted, self excluded."""
    from avid_hip import topk
    g = golden("cma")
    N, Pk = 500, 32
    v1, v2 = det_bank("cma:v1", N).to(gpu_device), det_bank("cma:v2", N).to(gpu_device)
    for kind, name in enumerate(["consensus", "union", "video", "audio"]):
        got = topk.cma_topk(v1, v2, 0, N, Pk, kind, batch=128).cpu().numpy()
        ref = g[f"topk_{name}"]
        assert got.shape == ref.shape
        same = [set(got[i]) == set(ref[i]) for i in range(N)]
        assert np.mean(same) > 0.995, (name, np.mean(same))
        for i in range(N):
            assert i not in set(got[i]) and len(set(got[i]) & set(ref[i])) >= Pk - 1
        assert (np.diff(got, axis=1) > 0).all()
    # sharded query ranges give the same rows (multi-GPU path shards [q0, q1) by rank)
    a = topk.cma_topk(v1, v2, 0, 250, Pk, 0, batch=64)
    b = topk.cma_topk(v1, v2, 250, 500, Pk, 0, batch=64)
    full = topk.cma_topk(v1, v2, 0, N, Pk, 0, batch=128)
    assert torch.equal(torch.cat([a, b]), full)


def test_cma_topk_filter_path_vs_oracle(gpu_device):
    """Banks of >= 4096 rows take the threshold-filter selection (csrc/cma_topk.hip): all four agreement types
    against the oracle's dense search; rows sorted, self excluded; a ragged last query batch; sharded ranges."""
    from avid_hip import topk
    N, Pk = 6000, 32
    gen = torch.Generator().manual_seed(11)
    v1 = torch.nn.functional.normalize(torch.randn(N, 128, generator=gen), dim=1)
    v2 = torch.nn.functional.normalize(torch.randn(N, 128, generator=gen), dim=1)
    d1, d2 = v1.to(gpu_device), v2.to(gpu_device)
    for kind, name in enumerate(["consensus", "union", "video", "audio"]):
        got = topk.cma_topk(d1, d2, 0, N, Pk, kind, batch=1024).cpu().numpy()
        want = O.cma_topk(v1, v2, Pk, name)
        same = np.mean([set(got[i]) == set(want[i]) for i in range(N)])
        assert same > 0.998, (name, same)          # fp32 summation order may swap a boundary pair
        for i in range(0, N, 7):
            assert i not in set(got[i]) and len(set(got[i]) & set(want[i])) >= Pk - 1
        assert (np.diff(got, axis=1) > 0).all()
    a = topk.cma_topk(d1, d2, 0, 2500, Pk, 0, batch=512)
    b = topk.cma_topk(d1, d2, 2500, N, Pk, 0, batch=256)
    assert torch.equal(torch.cat([a, b]), topk.cma_topk(d1, d2, 0, N, Pk, 0, batch=1024))


def test_cma_topk_tie_overflow_falls_back_to_exact_scan(gpu_device):
    """Heavy ties overflow the filter's candidate lists; the exact insertion-list scan then redoes the batch.
    All rows identical: every score ties, order is (value desc, index asc) -> top 33 = rows 0..32, rank 0
    (row 0) dropped -> 1..32 for every query.  Half identical / half random: the identical half still resolves
    by index, the random half is still a valid top-K."""
    from avid_hip import topk
    N, Pk = 5000, 32
    row = torch.nn.functional.normalize(torch.randn(1, 128, generator=torch.Generator().manual_seed(3)), dim=1)
    bank = row.repeat(N, 1).contiguous().to(gpu_device)
    got = topk.cma_topk(bank, bank, 0, N, Pk, 0, batch=512).cpu()
    assert torch.equal(got, torch.arange(1, Pk + 1, dtype=got.dtype).repeat(N, 1))
    gen = torch.Generator().manual_seed(5)
    mixed = torch.nn.functional.normalize(torch.randn(N, 128, generator=gen), dim=1)
    mixed[:2000] = row
    got = topk.cma_topk(mixed.to(gpu_device), mixed.to(gpu_device), 0, N, Pk, 2, batch=1024).cpu().numpy()
    assert (got[:2000] == np.arange(1, Pk + 1)[None]).all()       # the 2000 duplicates tie at score 1.0
    # random half: a valid top-(Pk+1) minus self under ties (the 2000 duplicates share one score per query, so
    # set equality with torch.topk's arbitrary tie order is not the criterion)
    sims = (mixed @ mixed[2000::15].t()).numpy()                  # [N, nq']
    for col, q in enumerate(range(2000, N, 15)):
        sc = sims[:, col]
        kth = np.sort(sc)[::-1][Pk]                               # (Pk+1)-th best score
        sel = set(got[q].tolist())
        assert q not in sel and len(sel) == Pk
        assert all(sc[i] >= kth - 2e-6 for i in sel)
        must = set(np.nonzero(sc > kth + 2e-6)[0].tolist()) - {q}
        assert must <= sel


def test_avid_cma_constructor_end_to_end(gpu_device):
    """criterions.AVID_CMA(...) builds its positive_set with the HIP search and trains one step."""
    import criterions
    N, bs = 3000, 8
    crit = criterions.AVID_CMA(num_data=N, embedding_dim=128, num_negatives=256, num_negatives_within=64,
                               momentum=0.5, sampling_args={"type": "consensus", "pos_k": 32},
                               resample_freq=5, device=gpu_device.index)
    ps = crit.nce_average.positive_set
    assert ps.shape == (N, 32) and ps.dtype == torch.int32
    want = O.cma_topk(crit.nce_average.view1_mem.cpu(), crit.nce_average.view2_mem.cpu(), 32, "consensus")
    agree = np.mean([len(set(ps[i].tolist()) & set(want[i])) for i in range(N)]) / 32
    assert agree > 0.999
    assert sorted(crit.state_dict().keys()) == ["criterion.avg_exp_score", "nce_average.positive_set",
                                                "nce_average.view1_mem", "nce_average.view2_mem"]
    v = torch.randn(bs, 128, device=gpu_device, requires_grad=True)
    a = torch.randn(bs, 128, device=gpu_device, requires_grad=True)
    y = torch.randperm(N)[:bs].to(gpu_device)
    loss, tb = crit(v, a, y)
    loss.backward()
    assert torch.isfinite(loss) and set(tb) == {"Loss/inst-v2a", "Loss/inst-a2v", "Loss/pos-v2v", "Loss/pos-a2a"}
    crit.set_epoch(5)                                   # resample
    assert crit.nce_average.positive_set.shape == (N, 32)


def test_real_dataset_shapes_vs_oracle(gpu_device):
    """the shipped configs feed 3x8x224x224 video and 1x200x257 audio
    (configs/main/avid/kinetics/Cross-N1024.yaml:19-25): odd extents (257 -> 129 -> 65 -> 33 -> 17) hit the
    tile-edge paths, 224^2 the stem's fallback selection.  One clip pair, forward + backward vs the oracle
    with the device's ReLU pattern pinned."""
    m = _build_model(gpu_device).train()
    video = T(detgen.det_normalish("real:video", (1, 3, 8, 224, 224)))
    audio = T(detgen.det_normalish("real:audio", (1, 1, 200, 257)))
    video = torch.cat([video, video.flip(4)]); audio = torch.cat([audio, audio.flip(2)])     # 2 clips
    masks, remove = capture_relu_masks(m)
    e1, e2 = m(video.to(gpu_device), audio.to(gpu_device))
    remove()
    gv = T(detgen.det_uniform("real:gv", (2, 128))).to(gpu_device)
    ga = T(detgen.det_uniform("real:ga", (2, 128))).to(gpu_device)
    ((e1 * gv).sum() + (e2 * ga).sum()).backward()
    P = O.det_state(O.av_wrapper_spec(18), "w")
    for n in P:
        if not ("running" in n or "num_batches" in n):
            P[n].requires_grad_(True)
    O.PREACT = {}
    try:         # free-running oracle first: the pinned pattern differs from its own only on near-zero pre-activations
        with torch.no_grad():
            O.av_forward(video, audio, {k: v.detach().clone() for k, v in P.items()}, 18, True)
        flips, elements, worst = relu_flip_report(masks, O.PREACT)
    finally:
        O.PREACT = None
    assert flips <= 2e-6 * elements and worst < 1e-4, (flips, elements, worst)
    O.RELU_MASKS = masks
    try:
        ve, ae = O.av_forward(video, audio, P, 18, True)
        ((ve * gv.cpu()).sum() + (ae * ga.cpu()).sum()).backward()
    finally:
        O.RELU_MASKS = None
    assert float((e1.detach().cpu() - ve.detach()).abs().max() / ve.detach().abs().max()) < 2e-4
    assert float((e2.detach().cpu() - ae.detach()).abs().max() / ae.detach().abs().max()) < 2e-4
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        a, r = p.grad.contiguous().cpu().double(), P[n].grad.double()
        worst = max(worst, (n, float((a - r).abs().max() / (r.abs().max() + 1e-30))), key=lambda t: t[1])
    assert worst[1] < 1e-3, worst


def test_rccl_path_single_rank(gpu_device):
    """Drive the multi-GPU code path on the one GPU we have: a 1-rank RCCL group with AVID_FORCE_DIST=1 makes
    TrainStep broadcast parameters, all-reduce the gradient buckets from the backward hooks (issued from both
    tower streams) and fold 1/world into Adam.  With world == 1 the result must equal the plain run exactly."""
    import os
    import torch.distributed as dist
    import criterions
    from avid_hip.parallel import TrainStep
    bs, N, K = 4, 4000, 128
    g = torch.Generator().manual_seed(9)
    video = torch.randn(bs, 3, 8, 64, 64, generator=g).to(gpu_device)
    audio = torch.randn(bs, 1, 40, 100, generator=g).to(gpu_device)
    ids = torch.stack([torch.randperm(N, generator=g)[:bs] for _ in range(3)]).to(gpu_device)

    def run():
        torch.manual_seed(0)
        m = _build_model(gpu_device).train()
        crit = criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, device=gpu_device.index)
        gg = torch.Generator().manual_seed(3)
        crit.nce_average.view1_mem.copy_(torch.nn.functional.normalize(torch.randn(N, 128, generator=gg), dim=1))
        crit.nce_average.view2_mem.copy_(torch.nn.functional.normalize(torch.randn(N, 128, generator=gg), dim=1))
        crit.nce_average.multinomial.reseed(11, 0)
        e = TrainStep(m, crit, bucket_bytes=4 << 20)
        return [float(e.step(video, audio, ids[i])) for i in range(3)], e

    plain, _ = run()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", AVID_FORCE_DIST="1")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu_device)
    try:
        forced, eng = run()
        assert eng.buckets.comm and len(eng.buckets.bounds) >= 4
    finally:
        dist.destroy_process_group()
        os.environ.pop("AVID_FORCE_DIST")
    assert forced == plain, (forced, plain)
