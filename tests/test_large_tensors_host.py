"""Host side of tests/test_gpu_large_tensors.py (no GPU): what the library's dispatch queries answer for tensors of 2^31
bytes and more, what it refuses, the probe lists of tests/_large_ref.py at the shapes of the GPU test, and the four checks of
that file turned on planted defects in a scaled-down model whose boundary is a parameter.

The plans (grid, K-split, rounds) depend on the CU count, which is a default without a device: the queries pinned here are
the ones that do not — which path a layer takes, which kernel family, what its workspace contains."""
import ctypes as C

import pytest
import torch

import _large_ref as R

CPU = torch.device("cpu")


def _desc(layer, B):
    from avid_hip import ops
    cin, cout, k, s, p, thw, cf = R.LAYERS[layer]
    return ops._desc((B,) + thw, cin, cout, k, s, p, cf)


def _q(name, d, *a):
    from avid_hip import lib
    return lib.raw(name)(C.byref(d), *a)


def _name(d, which):
    from avid_hip import lib
    buf = C.create_string_buffer(256)
    assert lib.raw("avid_conv_kernel_name")(C.byref(d), which, buf, 256) == 0, lib.last_error()
    return buf.value.decode()


def _wt_bytes(layer):
    cin, cout, k, s, p, thw, cf = R.LAYERS[layer]
    return (4 * cout * k[0] * k[1] * k[2] * cin + 255) // 256 * 256


@pytest.fixture
def tconv_all():
    from avid_hip import lib
    conf = lib.raw("avid_tconv_configure")
    assert conf(2) == 2
    yield
    conf(-1)


# ------------------------------------------------------------------------------------------------------------ the shapes
def test_the_shapes_cross_the_lines_they_are_meant_to():
    for layer, B in R.CONV_2G:
        big = max(B * nb for nb in R.item_bytes(layer))
        assert (1 << 31) <= big < (1 << 31) + (1 << 25), (layer, B, big)          # past the line by less than 32 MiB
    for layer, B in R.CONV_4G:
        assert max(B * nb for nb in R.item_bytes(layer)) >= (1 << 32)
    layer, B = R.SPATIAL_2E31
    assert B * R.item_bytes(layer)[0] // 4 > (1 << 31) and B * 2 * 27 * 29 < (1 << 31)      # elements past 2^31, pixels below
    assert R.item_bytes("spatial") == (400896, 400896) and R.item_bytes("strided") == (400896, 215040)
    assert R.item_bytes("strided_wide") == (199680, 114688) and R.item_bytes("video_stem") == (18432, 98304)
    assert R.item_bytes("audio_stem") == (2560, 40960) and R.item_bytes("temporal") == (430080, 430080)
    assert 5400 * 400896 == 2164838400 and 5000 * 430080 == 2150400000 and 10800 * 199680 == 2156544000
    assert 52500 * 40960 == 2150400000 and 21500 * 2 * 27 * 29 * 64 == 2154816000


PROBES = {      # (layer, B) -> the items around every multiple of 2^31 bytes, worked out by hand: floor(k 2^31 / item bytes)
    ("spatial", 5400): [5355, 5356, 5357],                           # 2^31 / 400896 = 5356.7
    ("temporal", 5000): [4992, 4993, 4994],                          # 2^31 / 430080 = 4993.2
    ("temporal_13x15", 5378): [5376, 5377],                          # 2^31 / 399360 = 5377.3: the last item holds it
    ("strided", 5400): [5355, 5356, 5357],                           # x; y stays below 2^31 bytes
    ("strided_wide", 10800): [10753, 10754, 10755],                  # 2^31 / 199680 = 10754.6
    ("video_stem", 22000): [21844, 21845, 21846],                    # y: 2^31 / 98304 = 21845.3
    ("audio_stem", 52500): [52427, 52428, 52429],                    # y: 2^31 / 40960 = 52428.8
    ("spatial", 10800): [5355, 5356, 5357, 10712, 10713, 10714],     # 2^32 / 400896 = 10713.4
    ("video_stem", 44000): [21844, 21845, 21846, 43689, 43690, 43691],
    ("spatial", 21500): [5355, 5356, 5357, 10712, 10713, 10714, 16069, 16070, 16071, 21425, 21426, 21427],
}


@pytest.mark.parametrize("case", list(PROBES), ids=lambda c: f"{c[0]}-{c[1]}")
def test_probe_items(case):
    layer, B = case
    items = R.probe_items(B, R.item_bytes(layer), seed=1)
    assert items == sorted(set(items)) and items[0] == 0 and items[-1] == B - 1 and all(0 <= i < B for i in items)
    assert set(PROBES[case]) <= set(items)
    g = torch.Generator().manual_seed(1)
    rand = {int(v) for v in torch.randint(0, B, (4,), generator=g)}
    assert set(items) == {0, B - 1} | rand | set(PROBES[case])
    assert R.probe_items(B, R.item_bytes(layer), seed=1) == items and R.probe_items(B, R.item_bytes(layer), seed=2) != items
    n = R.chunk_items(R.item_bytes(layer))
    assert n * max(R.item_bytes(layer)) < (1 << 30) <= (n + 1) * max(R.item_bytes(layer))
    assert len(R.chunks(B, n)) >= 3 and R.chunks(B, n)[0][0] == 0 and R.chunks(B, n)[-1][1] == B


def test_probe_items_of_the_norm_and_pool_shapes():
    ib = (4 * 2 * 27 * 29 * 64, 4 * 2 * 14 * 15 * 64)                  # x, pooled y
    assert {5355, 5356, 5357} <= set(R.probe_items(5400, ib, 1))
    # at 21500 items the pooled tensor crosses 2^31 bytes as well: 2^31 / 107520 = 19972.9
    assert {19971, 19972, 19973, 21425, 21426, 21427} <= set(R.probe_items(21500, ib, 1))


# -------------------------------------------------------------------------------------------------------- dispatch queries
def test_spatial_layer_leaves_the_winograd_path_at_2_gib():
    small, big = _desc("spatial", 64), _desc("spatial", 5400)
    assert [_q("avid_conv_uses_wino", small, w) for w in range(3)] == [2, 2, 1]
    assert _name(small, 0).startswith("wino") and _name(small, 2) == "wino_wgrad_kernel"
    for B in (5400, 10800, 21500):
        d = _desc("spatial", B)
        assert [_q("avid_conv_uses_wino", d, w) for w in range(3)] == [0, 0, 0]
        assert _q("avid_conv_uses_split", d, 0) == 1 and _q("avid_conv_uses_split", d, 1) == 1
        assert _q("avid_conv_takes_in_affine", d) == 0 and _q("avid_conv_wgrad_groupable", d) == 0
        assert _q("avid_conv_dgrad_bn_rows", d) > 0
        assert _name(d, 0).startswith("igemm_pk_kernel<4,1,1,2,0>") and _name(d, 1).startswith("igemm_pk_kernel<4,1,1,2,1>")
        assert _name(d, 2).startswith("wgrad_tab_kernel<")
    assert big.To == 2 and big.Ho == 27 and big.Wo == 29


def test_temporal_layers_leave_tconv_at_2_gib(tconv_all):
    for layer, small_b, big_b in (("temporal", 64, 5000), ("temporal_13x15", 3, 5378)):
        small, big = _desc(layer, small_b), _desc(layer, big_b)
        assert _q("avid_conv_takes_in_affine", small) == 1 and _name(small, 0).startswith("tconv64_kernel<0>")
        assert _name(small, 1).startswith("tconv64_kernel<1>") and _name(small, 2).startswith("twgrad64_kernel")
        assert _q("avid_conv_takes_in_affine", big) == 0 and _q("avid_conv_takes_out_affine", big) == 0
        assert _name(big, 0).startswith("igemm_pk_kernel<4,1,1,2,0>") and _name(big, 1).startswith("igemm_pk_kernel<4,1,1,2,1>")
        assert _name(big, 2).startswith("wgrad_tab_kernel<")
        assert _q("avid_conv_uses_split", big, 0) == 1 and _q("avid_conv_uses_wino", big, 0) == 0


@pytest.mark.parametrize("layer,B,tile", [("strided", 5400, "4,1,1,2"), ("strided_wide", 10800, "2,2,2,2")])
def test_strided_input_gradient_follows_dispatch_igemm(layer, B, tile):
    """dx >= 2^31 bytes: dispatch_igemm<1> takes igemm_kernel<..,true>, which splits nothing.  The kernel name says so and the
    workspace holds the transposed weights alone (before library version 172: the persistent kernel's name and 8 dx-shaped
    slabs — 17 GB — that nothing touched)."""
    from avid_hip import lib
    assert lib.version() >= 172
    small, big = _desc(layer, 64), _desc(layer, B)
    assert _name(small, 1).startswith("igemm_pk_kernel<") and "s2 (stride-parity classes)" in _name(small, 1)
    assert _q("avid_conv_dgrad_bn_rows", small) > 0
    # below the line: transposed weights + at least the 8 dx-shaped slabs of the K-split classes
    assert _q("avid_conv_dgrad_workspace_bytes", small) >= _wt_bytes(layer) + 8 * 64 * R.item_bytes(layer)[0]
    assert _name(big, 1).startswith(f"igemm_kernel<{tile},1>s2"), _name(big, 1)
    assert _q("avid_conv_dgrad_bn_rows", big) == 0 and _q("avid_conv_uses_split", big, 1) == 0
    assert _q("avid_conv_uses_split", big, 0) == 1 and _q("avid_conv_wgrad_groupable", big) == 1
    assert _q("avid_conv_dgrad_workspace_bytes", big) == _wt_bytes(layer)
    assert B * R.item_bytes(layer)[0] >= (1 << 31)
    # one item fewer than the line: still the persistent kernel
    edge = (1 << 31) // R.item_bytes(layer)[0]
    below, at = _desc(layer, edge), _desc(layer, edge + 1)
    assert _name(below, 1).startswith("igemm_pk_kernel<") and _name(at, 1).startswith("igemm_kernel<")
    assert _q("avid_conv_dgrad_workspace_bytes", at) == _wt_bytes(layer) < _q("avid_conv_dgrad_workspace_bytes", below)


def test_stems_keep_their_kernels():
    for layer, B, fwd in (("video_stem", 22000, "stem_fwd3p_kernel<3,3>"), ("video_stem", 44000, "stem_fwd3p_kernel<3,3>"),
                          ("audio_stem", 52500, "stem_fwd_kernel<1,1>")):
        d = _desc(layer, B)
        cin, kt = R.LAYERS[layer][0], R.LAYERS[layer][2][0]
        assert _name(d, 0) == fwd and _name(d, 1) == f"stem_dgrad_kernel<{cin},{kt}>"
        assert _name(d, 2).startswith("stem_wgrad_kernel splits=")
        assert _q("avid_conv_dgrad_workspace_bytes", d) == 0 and _q("avid_conv_wgrad_workspace_bytes", d) > 0


# --------------------------------------------------------------------------------------------------------------- refusals
def test_validate_refuses_2_31_pixels_and_items_too_large_for_tile_offsets():
    from avid_hip import lib
    cin, cout, k, s, p, thw, cf = R.LAYERS["spatial"]
    from avid_hip import ops
    B = (1 << 31) // (2 * 27 * 29) + 1
    d = ops._desc((B, 2, 27, 29), cin, cout, k, s, p, False)
    buf = C.create_string_buffer(64)
    assert lib.raw("avid_conv_kernel_name")(C.byref(d), 0, buf, 64) == -4 and "2^31 pixels" in lib.last_error()
    assert _q("avid_conv_fwd_workspace_bytes", d) == 0 and _q("avid_conv_uses_wino", d, 0) == 0
    d = ops._desc((B - 1, 2, 27, 29), cin, cout, k, s, p, False)
    assert lib.raw("avid_conv_kernel_name")(C.byref(d), 0, buf, 64) == 0
    # one item of 64 x 600 x 600 x 64 floats: (128 / pixels + 2) items of 5.9 GB do not fit 32-bit tile offsets
    d = ops._desc((2, 64, 600, 600), cin, cout, k, s, p, False)
    assert lib.raw("avid_conv_kernel_name")(C.byref(d), 0, buf, 64) == -4 and "32-bit tile offsets" in lib.last_error()


def test_res_fusable_ends_at_2_31_bytes():
    import models
    from models import network_blocks as nb
    blk = models.R2Plus1D(18).conv3x.block1 if hasattr(models.R2Plus1D(18).conv3x, "block1") else None
    if blk is None:
        blk = next(m for m in models.R2Plus1D(18).modules() if isinstance(m, nb.BasicR2P1DBlock) and m.res)
    assert nb.res_fusable(blk, (1 << 29) - 1) and not nb.res_fusable(blk, 1 << 29)
    assert not nb.res_fusable(blk, 84 * 64 * 32 * 56 * 56)             # a block input at 84 clips of 32 frames


def test_the_launch_programs_refuse_a_step_with_a_2_gib_block_input():
    import models
    from avid_hip import plan
    torch.manual_seed(0)
    wrapper = models.ClassificationWrapper(models.R2Plus1D(18), 101, feat_name="pool", feat_dim=512, pooling_op=None,
                                           use_dropout=True, dropout=0.5).train()
    with pytest.raises(plan.Unsupported):
        plan.ClsPlan(wrapper, (88, 3, 32, 224, 224), CPU, True, True, False)


# ------------------------------------------------------------------------------- the checks against planted defects
# A scaled-down model: 40 items of 25 floats (100 bytes each), boundary at 2048 bytes (inside item 20), chunks of 9 items.
TOY_B, TOY_N, TOY_BOUNDARY, TOY_CHUNK = 40, 25, 2048, 9


def _toy():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(TOY_B, TOY_N, generator=g)
    items = R.probe_items(TOY_B, (4 * TOY_N,), seed=4, boundary=TOY_BOUNDARY)
    assert {19, 20, 21} <= set(items) and len(items) <= 9
    ref = lambda i: 2.0 * x[i].double() + 1.0                                   # noqa: E731
    chunk = lambda b0, b1: R.toy_op(x[b0:b1], TOY_BOUNDARY, item0=b0, total=TOY_B)   # noqa: E731
    return x, items, ref, chunk


def _verdicts(y, items, ref, chunk):
    """Which of checks 1, 2 and 4 object to ``y``."""
    out = set()
    for k, run in ((1, lambda: R.check_probes(y, ref, items, 2e-5, "toy")), (2, lambda: R.check_chunks(y, chunk, TOY_CHUNK, None, "toy")),
                   (4, lambda: R.assert_written(y, "toy"))):
        try:
            run()
        except AssertionError:
            out.add(k)
    return out


def test_checks_pass_a_correct_op():
    x, items, ref, chunk = _toy()
    assert TOY_CHUNK * 4 * TOY_N < TOY_BOUNDARY                     # a chunk never reaches the boundary, like the GPU test's
    assert _verdicts(R.toy_op(x, TOY_BOUNDARY), items, ref, chunk) == set()
    # and a defect is silent on a tensor that ends below the boundary — the regime the rest of the suite pins
    for defect in ("wrap", "drop", "sign"):
        assert torch.equal(R.toy_op(x[:20], TOY_BOUNDARY, defect), R.toy_op(x[:20], TOY_BOUNDARY))


@pytest.mark.parametrize("defect,meant", [("wrap", 1), ("sign", 1), ("drop", 4), ("swap", 2)])
def test_each_planted_defect_is_caught_by_the_check_meant_for_it(defect, meant):
    x, items, ref, chunk = _toy()
    others = [i for i in range(TOY_B) if i not in items]
    swap = (others[0], others[-1])                                               # two non-probe items of different chunks
    assert swap[0] // TOY_CHUNK != swap[1] // TOY_CHUNK
    y = R.toy_op(x, TOY_BOUNDARY, defect, swap=swap)
    caught = _verdicts(y, items, ref, chunk)
    assert meant in caught, (defect, caught)
    if defect == "swap":
        assert caught == {2}                      # no probe item is wrong, everything was written: only the whole-tensor check sees it
    if defect == "drop":
        assert bool(torch.isnan(y[21:]).all()) and not bool(torch.isnan(y[:20]).any())
    if defect == "wrap":
        # item 21 holds the data of the bytes 2100 - 2048 = 52 ... : another item's values, finite and plausible
        assert bool(torch.isfinite(y).all()) and not torch.equal(y[21], R.toy_op(x, TOY_BOUNDARY)[21])


def test_check_1_alone_would_miss_a_wrong_item_that_is_no_probe_item():
    x, items, ref, chunk = _toy()
    other = next(i for i in range(TOY_B) if i not in items)
    y = R.toy_op(x, TOY_BOUNDARY)
    y[other, 3] += 1.0
    assert _verdicts(y, items, ref, chunk) == {2}
    y = R.toy_op(x, TOY_BOUNDARY)
    y[items[2], 3] *= 1.0 + 1e-3                                               # a probe item off by more than the bar
    assert 1 in _verdicts(y, items, ref, chunk)


def test_float64_helpers_agree_with_autograd():
    """``wgrad64`` and ``conv_item64`` (the references of the GPU test) against torch's own float64 convolution gradient."""
    import torch.nn.functional as F
    for layer in ("spatial", "strided", "temporal", "audio_stem", "video_stem"):
        cin, cout, k, s, p, thw, cf = R.LAYERS[layer]
        thw = tuple(min(v, 6) for v in thw) if not cf else thw
        g = torch.Generator().manual_seed(5)
        xs = (3, cin) + thw if cf else (3,) + thw + (cin,)
        x = torch.randn(xs, generator=g, dtype=torch.float64)
        w = R.weight(layer, 6).double().requires_grad_(True)
        saved = R.LAYERS[layer]
        R.LAYERS[layer] = (cin, cout, k, s, p, thw, cf)
        try:
            y = F.conv3d(R.to_ncdhw(x, cf), w, stride=s, padding=p)
            dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
            (y * dy).sum().backward()
            dy_cl = dy.permute(0, 2, 3, 4, 1).contiguous()
            got = R.wgrad64(layer, x, dy_cl)
            assert float((got - w.grad).abs().max()) < 1e-12 * float(w.grad.abs().max() + 1)
            per_item = sum(R.conv_item64(layer, x[i], w.detach(), dy_cl[i])[2] for i in range(3))
            assert float((per_item - w.grad).abs().max()) < 1e-12 * float(w.grad.abs().max() + 1)
            y0, dx0, _ = R.conv_item64(layer, x[0], w.detach(), dy_cl[0])
            assert float((y0 - y[0].detach().permute(1, 2, 3, 0)).abs().max()) < 1e-12
            assert dx0.shape == x[0].shape
        finally:
            R.LAYERS[layer] = saved
