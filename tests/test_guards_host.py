"""The guarded, poisoned allocator of tests/_guards.py, checked on CPU tensors (no GPU): it intercepts each factory
function, keeps their contracts, and turns each kind of slip the GPU tests look for into a failure; the last test
checks what it patches in the package (the library's host-side size functions only) and that it puts everything back."""
import threading

import pytest
import torch

from _guards import FILLS, GUARD, GuardError, guarded


def cpu_guarded(fill):
    return guarded(fill, device_types=("cpu",), package=False)


def _poison(dtype, fill):
    return torch.full((1,), fill, dtype=torch.uint8).repeat(torch.empty((), dtype=dtype).element_size()).view(dtype)[0]


FACTORIES = {
    "empty": lambda: torch.empty((3, 5), dtype=torch.float32),
    "empty_like": lambda: torch.empty_like(torch.ones(4, 2, dtype=torch.int64)),
    "empty_strided": lambda: torch.empty_strided((2, 3), (1, 2), dtype=torch.float32),
    "zeros": lambda: torch.zeros(7, dtype=torch.int32),
    "zeros_like": lambda: torch.zeros_like(torch.ones(3, 3)),
    "full": lambda: torch.full((2, 2), 2.5),
}


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", sorted(FACTORIES))
def test_each_factory_is_intercepted(name, fill):
    plain = FACTORIES[name]()
    with cpu_guarded(fill) as g:
        before = len(g.records)
        t = FACTORIES[name]()
        assert len(g.records) == before + 1, f"torch.{name} was not intercepted"
        rec = g.records[-1]
        assert rec.kind == name
        assert rec.site.startswith("test_guards_host.py:"), rec.site
        assert t.shape == plain.shape and t.dtype == plain.dtype and t.stride() == plain.stride()
        assert rec.nbytes == plain.untyped_storage().nbytes() or name == "empty_like"
        base = rec.buf.data_ptr()
        assert t.data_ptr() == base + GUARD and GUARD % 256 == 0 and GUARD >= 64 * 1024
        assert rec.buf.numel() - GUARD - rec.nbytes >= GUARD
        if name.startswith("empty"):
            assert bool((t.contiguous().view(torch.uint8) == fill).all()), "an empty* payload must hold the pattern"
        g.check()


@pytest.mark.parametrize("fill", FILLS)
def test_zeros_and_full_keep_their_contract(fill):
    with cpu_guarded(fill) as g:
        z = torch.zeros((5, 3), dtype=torch.float32)
        zl = torch.zeros_like(torch.ones(2, 3, 4).permute(2, 0, 1))
        zs = torch.zeros((), dtype=torch.int64)
        f = torch.full((4,), 7, dtype=torch.int32)
        fs = torch.full((), 0.125, dtype=torch.float32)
        e0 = torch.empty((0, 4))
        assert not z.any() and not zl.any() and int(zs) == 0
        assert f.tolist() == [7] * 4 and float(fs) == 0.125
        assert e0.shape == (0, 4)
        g.check()


@pytest.mark.parametrize("fill", FILLS)
def test_empty_like_of_a_permuted_tensor_keeps_its_strides(fill):
    src = torch.ones(2, 3, 4, 5).permute(0, 3, 1, 2)              # channels-last memory under a channels-first shape
    want = torch.empty_like(src)
    with cpu_guarded(fill) as g:
        got = torch.empty_like(src)
        w = torch.empty(8, 3, 3, 4).movedim(-1, 1)                # ops.make_weight's layout
        assert len(g.records) == 2
    assert got.shape == want.shape and got.stride() == want.stride() and not got.is_contiguous()
    assert w.shape == (8, 4, 3, 3) and w.movedim(1, -1).is_contiguous()


@pytest.mark.parametrize("nbytes", [1, 4, 100, 255, 256, 257, 4097])
def test_payloads_stay_256_byte_aligned(nbytes):
    with cpu_guarded(0xFF) as g:
        for _ in range(3):
            t = torch.empty(nbytes, dtype=torch.uint8)
            base = g.records[-1].buf.data_ptr()
            assert (t.data_ptr() - base) % 256 == 0, "the payload's offset into its allocation is no multiple of 256"
            ws = g.workspace(torch.device("cpu"), nbytes)
            assert ws.numel() == nbytes and (ws.data_ptr() - g.records[-1].buf.data_ptr()) % 256 == 0
        assert [w[:2] for w in g.workspaces] == [(nbytes, g.records[-1].site)] * 3
        g.check()


@pytest.mark.parametrize("fill", FILLS)
def test_one_byte_into_the_leading_guard_is_detected(fill):
    with cpu_guarded(fill) as g:
        torch.empty(10)
        t = torch.empty(6, dtype=torch.float32)
        torch.as_strided(t.view(torch.uint8), (1,), (1,), t.storage_offset() * 4 - 1).fill_(fill ^ 0x01)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert "leading guard" in msg and "1 bytes before the payload" in msg and "test_guards_host.py:" in msg
    assert "buffer of 24 bytes" in msg and msg.count("buffer of") == 1, msg


@pytest.mark.parametrize("fill", FILLS)
def test_one_byte_into_the_trailing_guard_is_detected(fill):
    with cpu_guarded(fill) as g:
        t = torch.empty(6, dtype=torch.float32)
        torch.empty(10)
        torch.as_strided(t.view(torch.uint8), (1,), (1,), t.storage_offset() * 4 + 24).fill_(fill ^ 0x80)
        with pytest.raises(GuardError) as e:
            g.check()
    msg = str(e.value)
    assert "trailing guard" in msg and "first at payload offset 24 (0 bytes past the end" in msg, msg
    assert "test_guards_host.py:" in msg and msg.count("buffer of") == 1, msg


def test_an_overrun_far_into_the_guard_is_detected():
    with cpu_guarded(0x5A) as g:
        ws = g.workspace(torch.device("cpu"), 1000)
        torch.as_strided(ws, (1,), (1,), ws.storage_offset() + 1000 + GUARD - 1).fill_(0)
        with pytest.raises(GuardError, match="workspace buffer of 1000 bytes"):
            g.check()


def _op_that_skips_an_element(x):
    y = torch.empty_like(x)
    y[:-1] = x[:-1] * 2                                           # the last element is never written
    return y


def test_an_unwritten_element_differs_between_the_fills():
    x = torch.arange(9, dtype=torch.float32)
    outs = []
    for fill in FILLS:
        with cpu_guarded(fill) as g:
            outs.append(_op_that_skips_an_element(g.place(x)).clone())
            g.check()
    a, b = (o.view(torch.int32) for o in outs)
    assert torch.equal(a[:-1], b[:-1]) and a[-1] != b[-1]
    assert torch.isnan(outs[0][-1]) and float(outs[1][-1]) > 1e16          # 0xFF: NaN; 0x5A: finite, about 1.5e16
    assert int(_poison(torch.int64, 0xFF)) == -1 and int(_poison(torch.int32, 0x5A)) == 0x5A5A5A5A


def _op_that_reads_one_past_the_end(x):
    win = torch.as_strided(x, (x.numel(), 2), (1, 1))              # the last window reads x[n]
    return win.sum(1)


def test_a_read_past_an_input_differs_between_the_fills():
    x = torch.arange(5, dtype=torch.float32)
    outs = []
    for fill in FILLS:
        with cpu_guarded(fill) as g:
            px = g.place(x)
            assert torch.equal(px, x) and px.stride() == x.stride() and g.records[-1].kind == "input"
            outs.append(_op_that_reads_one_past_the_end(px).clone())
            g.check()
    a, b = (o.view(torch.int32) for o in outs)
    assert torch.equal(a[:-1], b[:-1]) and a[-1] != b[-1]


def test_place_keeps_strides_and_requires_grad():
    x = torch.randn(2, 3, 4).permute(2, 0, 1).requires_grad_(True)
    with cpu_guarded(0xFF) as g:
        px = g.place(x)
        assert g.place(None) is None
        g.check()
    assert px.requires_grad and px.is_leaf and px.stride() == x.stride() and torch.equal(px.detach(), x.detach())


def test_allocations_are_counted_per_call_site_and_thread():
    """The mode itself is thread-local: an allocation on another thread is seen only where the module's ``torch`` name
    is the forwarding proxy.  Both routes feed the same per-site count."""
    from _guards import _TorchProxy

    def backward(t):                                               # (the count is kept by function name)
        return t.empty(3)

    with cpu_guarded(0xFF) as g:
        backward(torch)
        assert g.count_in("backward") == 1 and g.count_off_thread() == 0
        proxy = _TorchProxy(g)
        assert proxy.float32 is torch.float32 and proxy.nn is torch.nn
        th = threading.Thread(target=backward, args=(proxy,))
        th.start()
        th.join()
        assert g.count_in("backward") == 2 and g.count_off_thread() == 1
        backward(proxy)                                            # on the mode's thread: guarded once, not twice
        assert g.count_in("backward") == 3 and len(g.records) == 3
        g.check()


def test_other_devices_and_the_world_outside_are_left_alone():
    with guarded(0xFF, device_types=("cuda",), package=False) as g:
        t = torch.empty(4)                                         # CPU, while only CUDA is guarded
        assert not g.records and t.shape == (4,)
    with cpu_guarded(0xFF) as g:
        pass
    assert torch.zeros(3).untyped_storage().nbytes() == 12         # nothing stays patched


def test_the_package_patches_apply_and_are_undone():
    """With the package: ``ops.workspace`` (also under the name topk imported) hands out exactly the bytes asked for, the size
    functions' answers are noted, allocations made by the package's code are named by their own file and line, the caches start
    empty, and everything is put back on exit."""
    from avid_hip import lib, ops, plan, topk
    real_ws, real_raw, real_torch = ops.workspace, lib.raw, ops.torch
    real_call, real_seal, floor = lib.call, plan.Programs._seal, plan.WS_FLOOR
    assert floor == 1 << 20
    ops._BN_WS_CACHE[("sentinel", 0)] = 123
    try:
        with guarded(0x5A, device_types=("cpu",)) as g:
            assert ops.workspace == g.workspace and topk.workspace == g.workspace and lib.raw is not real_raw
            assert ("sentinel", 0) not in ops._BN_WS_CACHE
            assert plan.WS_FLOOR == 0 and lib.call is not real_call and plan.Programs._seal is not real_seal
            nb = lib.raw("avid_logspec_workspace_bytes")(3, 512, 201)
            assert nb > 0 and g.size_values == {nb}
            assert lib.raw("avid_version")() == lib.version()
            ws = ops.workspace(torch.device("cpu"), nb)
            assert ws.numel() == nb and ws.dtype == torch.uint8 and g.workspaces[-1][0] == nb
            assert bool((ws == 0x5A).all())
            w = ops.make_weight(8, 4, 1, 3, 3)
            site, func = next(k for k in g.sites if k[1] == "make_weight")
            assert site.startswith("avid-cma_amd/avid_hip/ops.py:") and ops.weight_layout_ok(w)
            assert ops._bn_ws_bytes(777, 128) in g.size_values
            g.check()
        assert ops.workspace is real_ws and topk.workspace is real_ws and lib.raw is real_raw and ops.torch is real_torch
        assert plan.WS_FLOOR == floor and lib.call is real_call and plan.Programs._seal is real_seal
        assert ops._BN_WS_CACHE[("sentinel", 0)] == 123 and (777, 128) not in ops._BN_WS_CACHE
    finally:
        ops._BN_WS_CACHE.pop(("sentinel", 0), None)


def test_check_takes_records_on_a_device_that_is_not_guarded():
    """``place`` guards its source wherever it lives: a CPU input while only CUDA allocations are guarded is checked too."""
    with guarded(0xFF, device_types=("cuda",), package=False) as g:
        px = g.place(torch.arange(4, dtype=torch.float32))
        assert len(g.records) == 1 and not px.is_cuda
        g.check()
        torch.as_strided(px, (1,), (1,), px.storage_offset() + 4).fill_(0.0)
        with pytest.raises(GuardError, match="input buffer of 16 bytes"):
            g.check()
