"""Shapes, probe items and checkers of tests/test_gpu_large_tensors.py (tensors of 2^31 bytes, 2^32 bytes and 2^31 elements)
and of tests/test_large_tensors_host.py, which pins the probe lists and turns the checkers on planted defects.

Every big tensor is batch-major ([B, ...]) and the ops under test treat batch items independently (convolutions, pooling)
or couple them only through sums over all rows (BatchNorm statistics, weight gradients).  Four checks per case:

1. ``check_probes``: a few items against float64 on the CPU — item 0, item B-1, four seeded random items and, for every
   multiple of 2^31 bytes inside an input or output tensor, the item that holds that byte and both its neighbours
   (``probe_items``).
2. ``check_chunks``: the WHOLE tensor against the same op run on batch chunks below 1 GiB each (the regime the rest of the
   suite pins): bit equality for per-element ops, a relative bar for convolutions.
3. sums over all rows against a float64 accumulation on the device (``sum64`` / ``wgrad64``) — next to what a float32
   torch reduction of the same data gives (``wgrad64(..., dtype=torch.float32)``).
4. ``assert_written``: the output, allocated as NaN by tests/_guards.py, holds no NaN (a store discarded by a truncated
   buffer descriptor stays NaN).

``toy_op`` is the scaled-down model the host test plants defects in: a per-element op whose byte offsets go wrong at a
``boundary`` that is a parameter."""
import torch
import torch.nn.functional as F

BOUNDARY = 1 << 31          # bytes: where the library changes route, and every further multiple of it
CHUNK_BYTES = (1 << 30) - 1   # check 2 runs the op on chunks in which every tensor is smaller than 1 GiB

# name -> (Cin, Cout, kernel, stride, pad, (T, H, W) of the input, channel_first)
LAYERS = {
    "spatial": (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 27, 29), False),
    "temporal": (64, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (8, 14, 15), False),
    "temporal_13x15": (64, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (8, 13, 15), False),   # tests/test_gpu_tconv.py SHAPES[0], B scaled
    "strided": (64, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 27, 29), False),
    "strided_wide": (128, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 13, 15), False),
    "video_stem": (3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), (2, 24, 32), True),
    "audio_stem": (1, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 20, 32), True),
}
# (layer, B): the smallest batches that cross 2^31 bytes, 2^32 bytes and (spatial only) 2^31 elements
CONV_2G = [("spatial", 5400), ("temporal", 5000), ("temporal_13x15", 5378), ("strided", 5400), ("strided_wide", 10800),
           ("video_stem", 22000), ("audio_stem", 52500)]
CONV_4G = [("spatial", 10800), ("video_stem", 44000)]
SPATIAL_2E31 = ("spatial", 21500)
NORM_B = (5400, 10800, 21500)          # C = 64 over [B, 2, 27, 29, 64]
NORM_ITEM = (2, 27, 29, 64)


def out_extent(layer):
    cin, cout, k, s, p, thw, cf = LAYERS[layer]
    return tuple((thw[a] + 2 * p[a] - k[a]) // s[a] + 1 for a in range(3))


def item_bytes(layer):
    """(bytes of one batch item of x, of y)."""
    cin, cout, k, s, p, thw, cf = LAYERS[layer]
    o = out_extent(layer)
    return 4 * cin * thw[0] * thw[1] * thw[2], 4 * cout * o[0] * o[1] * o[2]


def probe_items(B, item_nbytes, seed, boundary=BOUNDARY):
    """Sorted batch items check 1 looks at.  ``item_nbytes``: bytes of one item in each input / output tensor of the op."""
    items = {0, B - 1}
    g = torch.Generator().manual_seed(seed)
    items.update(int(v) for v in torch.randint(0, B, (4,), generator=g))
    for nb in item_nbytes:
        k = 1
        while k * boundary < B * nb:
            i = k * boundary // nb                   # the item that holds byte k * boundary
            items.update(j for j in (i - 1, i, i + 1) if 0 <= j < B)
            k += 1
    return sorted(items)


def chunk_items(item_nbytes):
    """Items per chunk of check 2: every tensor of a chunk is below 1 GiB."""
    return max(1, min(CHUNK_BYTES // nb for nb in item_nbytes))


def chunks(B, n):
    return [(b0, min(B, b0 + n)) for b0 in range(0, B, n)]


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_probes(got, ref_of, items, bar, what=""):
    """Check 1.  ``got`` [B, ...] (any device); ``ref_of(i)``: float64 CPU tensor shaped like ``got[i]``.  Every element of
    every probe item within ``bar`` of the largest |reference| over the probe items (``bar`` 0: equal values; a NaN fails).
    Returns the worst error as a share of the bar (bar 0: the worst error itself)."""
    refs = {i: ref_of(i) for i in items}
    scale = max(float(r.abs().max()) for r in refs.values())
    worst = 0.0
    for i, r in refs.items():
        err = (got[i].detach().cpu().double() - r).abs()
        ok = err <= bar * scale
        assert bool(ok.all()), (f"{what}: item {i} of {got.shape[0]}: {int((~ok).sum())} of {ok.numel()} elements outside "
                                f"{bar:g} x {scale:.3g}, worst {float(torch.nan_to_num(err, nan=float('inf')).max()):.3g}")
        worst = max(worst, float(err.max()))
    return worst / (bar * scale) if bar else worst


def check_chunks(got, run_chunk, n, bar=None, what=""):
    """Check 2.  ``run_chunk(b0, b1)``: the op on items [b0, b1) alone, shaped like ``got[b0:b1]``.  ``bar`` None: the same
    values everywhere (``torch.equal``); else within ``bar`` of the chunk's largest |value|.  Returns the worst share."""
    worst = 0.0
    for b0, b1 in chunks(got.shape[0], n):
        want = run_chunk(b0, b1)
        have = got[b0:b1]
        assert want.shape == have.shape, (what, want.shape, have.shape)
        if bar is None:
            if not torch.equal(have, want):
                bad = (have != want).flatten(1).any(1).nonzero().flatten()
                raise AssertionError(f"{what}: {bad.numel()} items of [{b0}, {b1}) differ from the chunked run, first item "
                                     f"{b0 + int(bad[0])}")
        else:
            scale = float(want.abs().max())
            err = (have - want).abs()
            ok = err <= bar * scale
            if not bool(ok.all()):
                bad = (~ok).flatten(1).any(1).nonzero().flatten()
                raise AssertionError(f"{what}: {bad.numel()} items of [{b0}, {b1}) outside {bar:g} x {scale:.3g} of the "
                                     f"chunked run, first item {b0 + int(bad[0])}")
            worst = max(worst, float(err.max()) / (bar * scale))
        del want, have
    return worst


def assert_written(t, what=""):
    """Check 4: no element is NaN (the guarded allocator hands every output out as NaN)."""
    flat = t.detach().reshape(-1)
    step = 1 << 28
    for o in range(0, flat.numel(), step):
        bad = torch.isnan(flat[o:o + step])
        if bool(bad.any()):
            first = o + int(bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())}+ elements never written, first at element {first} "
                                 f"(byte {4 * first}, item {first // max(1, flat.numel() // t.shape[0])})")


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------------- data on the device
def fill(shape, seed, device, kind="normal", scale=1.0, shift=0.0):
    """A float32 tensor filled ON ``device`` from a seeded generator, in batch chunks of at most 2^28 elements."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    per = 1
    for s in shape[1:]:
        per *= s
    n = max(1, (1 << 28) // per)
    for b0, b1 in chunks(shape[0], n):
        if kind == "normal":
            out[b0:b1].normal_(generator=g)
        else:
            out[b0:b1].uniform_(-0.5, 0.5, generator=g)
    if scale != 1.0 or shift != 0.0:
        for b0, b1 in chunks(shape[0], n):
            out[b0:b1].mul_(scale).add_(shift)
    return out


def weight(layer, seed):
    """[Cout, Cin, kt, kh, kw] float32 on the CPU, N(0, 1/K)."""
    cin, cout, k, s, p, thw, cf = LAYERS[layer]
    g = torch.Generator().manual_seed(seed)
    return torch.randn((cout, cin) + k, generator=g) / float(cin * k[0] * k[1] * k[2]) ** 0.5


# ------------------------------------------------------------------------------------------------------ float64 references
def to_ncdhw(t, channel_first):
    """One item or a batch, as the logical [.., C, T, H, W] view."""
    if channel_first:
        return t
    return t.movedim(-1, -4)


def conv_item64(layer, x_i, w, dy_i=None):
    """float64 CPU reference of ONE item: y [To,Ho,Wo,Cout] (channels-last, like the op's output), and with ``dy_i`` also dx
    (in x's layout) and this item's term of the weight gradient [Cout,Cin,kt,kh,kw]."""
    cin, cout, k, s, p, thw, cf = LAYERS[layer]
    x = to_ncdhw(x_i.detach().cpu().double(), cf).unsqueeze(0).clone().requires_grad_(dy_i is not None)
    w64 = w.detach().cpu().double().clone().requires_grad_(dy_i is not None)
    y = F.conv3d(x, w64, stride=s, padding=p)
    y_cl = y[0].permute(1, 2, 3, 0)
    if dy_i is None:
        return y_cl.detach(), None, None
    (y_cl * dy_i.detach().cpu().double()).sum().backward()
    dx = x.grad[0] if cf else x.grad[0].permute(1, 2, 3, 0)
    return y_cl.detach(), dx, w64.grad


def _tn(a, b, dtype):
    """a^T b of two [rows, *] matrices, rows cut into 128 batches so that the product parallelises; ``dtype`` float64: the
    reference accumulation, float32: what a float32 torch reduction of the same data makes of it."""
    rows = a.shape[0]
    nb = 128
    r = rows // nb * nb
    a, b = a.to(dtype), b.to(dtype)
    out = torch.zeros(a.shape[1], b.shape[1], dtype=dtype, device=a.device)
    if r:
        out += torch.bmm(a[:r].view(nb, r // nb, -1).transpose(1, 2), b[:r].view(nb, r // nb, -1)).sum(0)
    if r < rows:
        out += a[r:].t() @ b[r:]
    return out


def wgrad64(layer, x, dy, dtype=torch.float64, items=None):
    """The weight gradient [Cout, Cin, kt, kh, kw] accumulated on x's device in ``dtype``, tap by tap over batch chunks."""
    cin, cout, k, s, p, thw, cf = LAYERS[layer]
    To, Ho, Wo = out_extent(layer)
    B = x.shape[0]
    out = torch.zeros((cout, cin) + k, dtype=dtype, device=x.device)
    n = max(1, (1 << 26) // max(x[0].numel(), dy[0].numel()))          # <= 256 MiB of float32 per chunk and tensor
    for b0, b1 in chunks(B, n):
        xc = x[b0:b1].detach()
        if cf:
            xc = xc.permute(0, 2, 3, 4, 1)
        xp = F.pad(xc, (0, 0, p[2], p[2], p[1], p[1], p[0], p[0]))
        dyc = dy[b0:b1].detach().reshape(-1, cout)
        for a in range(k[0]):
            for b in range(k[1]):
                for c in range(k[2]):
                    xs = xp[:, a:a + s[0] * (To - 1) + 1:s[0], b:b + s[1] * (Ho - 1) + 1:s[1], c:c + s[2] * (Wo - 1) + 1:s[2]]
                    out[:, :, a, b, c] += _tn(dyc, xs.reshape(-1, cin), dtype)
    return out


def sum64(t, fn=None, other=None):
    """Column sums over all rows of a [.., C] tensor in float64 on its device, in chunks: sum fn(t[, other])."""
    Cc = t.shape[-1]
    flat = t.detach().reshape(-1, Cc)
    oth = None if other is None else other.detach().reshape(-1, Cc)
    acc = torch.zeros(Cc, dtype=torch.float64, device=t.device)
    step = 1 << 21
    for o in range(0, flat.shape[0], step):
        v = flat[o:o + step].double()
        if fn is not None:
            v = fn(v) if oth is None else fn(v, oth[o:o + step].double())
        acc += v.sum(0)
    return acc


# ------------------------------------------------------------------------------------------------- the scaled-down model
def toy_op(x, boundary, defect=None, swap=None, item0=0, total=None):
    """y = 2 x + 1 over a [B, n] float32 tensor the way a kernel with flat byte offsets would compute it; the output starts as
    NaN (the guarded allocator's fill).  ``item0`` / ``total``: x is items [item0, item0 + B) of a tensor of ``total`` items
    run as a chunk of its own, so its offsets start at 0 again.  Planted defects, all silent on a tensor below ``boundary``:

    * "wrap": the source offset wraps modulo ``boundary`` (a 32-bit offset) — elements past it read another item's data;
    * "drop": rows past ``boundary`` are never stored (a buffer descriptor whose num_records was truncated);
    * "sign": an offset >= ``boundary`` sign-extends to a negative one, out of the descriptor's range: the load returns 0;
    * "swap": the outputs of the two items ``swap`` = (i, j) of the WHOLE tensor trade places (chunked runs are not affected
      unless both items fall into the chunk — the host test picks items of different chunks)."""
    B, n = x.shape
    off = torch.arange(B * n, dtype=torch.int64) * 4
    flat = x.reshape(-1)
    src = flat.clone()
    if defect == "wrap":
        src = flat[(off % boundary) // 4]
    elif defect == "sign":
        src = torch.where(off >= boundary, torch.zeros_like(flat), flat)
    y = 2.0 * src + 1.0
    if defect == "drop":
        y = torch.where(off >= boundary, torch.full_like(y, float("nan")), y)
    y = y.view(B, n).clone()
    if defect == "swap" and total is None:
        i, j = swap
        y[[i, j]] = y[[j, i]]
    return y
