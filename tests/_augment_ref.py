"""CPU restatement (numpy) of the reference's per-frame PIL augmentation, integer for integer and rounding for rounding
(TEST INFRASTRUCTURE ONLY: imported by tests/ and tools/, the product path is avid_clip_augment in csrc/clipaug.hip).

What it restates, all for 8-bit RGB images:
  * ``img.crop((j, i, j + w, i + h)).resize((RW, RH), BILINEAR)``: Pillow's two-pass fixed-point resample (22 fraction bits,
    coefficients normalised in double by their sequential sum, the horizontal pass rounded to uint8 before the vertical one,
    a pass whose size does not change skipped);
  * ``ImageEnhance.Brightness / Color / Contrast``: ``Image.blend(degenerate, image, factor)`` in unfused fp32;
  * ``convert("L")``, ``convert("HSV")`` and back, and the hue shift of torchvision's PIL backend.
tests/test_augment_host.py pins every function here against the installed Pillow (the two colour conversions and the grey over
all 2^24 colours) and against tests/golden/augment.npz, which the reference's own transform classes produced."""
import math

import numpy as np

BRIGHTNESS, SATURATION, HUE, CONTRAST = 0, 1, 2, 3
PRECISION_BITS = 22


def coeffs(in_size, out_size):
    """Bilinear (support 1) coefficients of one axis: bounds int [out, 2] = (xmin, count), kk int32 [out, ksize]."""
    scale = fscale = in_size / out_size
    if fscale < 1.0:
        fscale = 1.0
    support = 1.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws, ww = [], 0.0
        for x in range(xmax):
            a = (x + xmin - center + 0.5) * ss
            w = 1.0 - abs(a) if abs(a) < 1.0 else 0.0
            ws.append(w)
            ww += w                                             # sequential, as the C loop (np.sum is pairwise)
        for x in range(xmax):
            w = ws[x] / ww if ww != 0.0 else ws[x]
            kk[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _pass(img, bounds, kk, axis):
    """One resample pass along ``axis`` of img [H, W, 3] uint8 -> uint8."""
    n_in = img.shape[axis]
    K = np.zeros((bounds.shape[0], n_in), np.int64)
    for xx, (xmin, cnt) in enumerate(bounds):
        K[xx, xmin:xmin + cnt] = kk[xx, :cnt]
    src = img.astype(np.int64)
    acc = np.einsum("ox,hxc->hoc", K, src) if axis == 1 else np.einsum("oy,ywc->owc", K, src)
    return np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample(img, box, RH, RW):
    """img [H, W, 3] uint8; box = (i, j, h, w) -> the box resampled to [RH, RW, 3]."""
    i, j, h, w = box
    out = np.ascontiguousarray(img[i:i + h, j:j + w])
    if w != RW:
        out = _pass(out, *coeffs(w, RW), axis=1)
    if h != RH:
        out = _pass(out, *coeffs(h, RH), axis=0)
    return out


def grey(rgb):
    """convert("L"): [..., 3] uint8 -> [...] uint8."""
    c = rgb.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(d, a, f):
    """Image.blend(degenerate d, image a, f): uint8 arrays (broadcastable) and a Python float."""
    f32 = np.float32(f)
    df = np.asarray(d).astype(np.float32)
    t = df + f32 * (np.asarray(a).astype(np.float32) - df)      # numpy never fuses: two fp32 roundings
    if 0.0 <= float(f32) <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def saturation(img, f):
    return blend(grey(img)[..., None], img, f)


def contrast(img, f):
    """img is ONE frame [H, W, 3]: the degenerate image is its rounded mean grey."""
    g = grey(img)
    mean = int(int(g.astype(np.int64).sum()) / g.size + 0.5)
    return blend(np.full_like(img, mean), img, f)


def rgb2hsv(rgb):
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(np.float32)
    mx = np.where(flat, 1, maxc).astype(np.float32)
    s = cr / mx
    rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
    h_r = bc - gc                                                                            # fp32
    h_g = ((2.0 + rc.astype(np.float64)) - bc.astype(np.float64)).astype(np.float32)         # double, rounded once
    h_b = ((4.0 + gc.astype(np.float64)) - rc.astype(np.float64)).astype(np.float32)
    h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(flat, 0, H), np.where(flat, 0, S), maxc], -1).astype(np.uint8)


def hsv2rgb(hsv):
    H, S, V = (hsv[..., k].astype(np.int32) for k in range(3))
    fs = (S.astype(np.float64) / 255.0).astype(np.float32)
    hf = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(np.float32)
    v = V.astype(np.float64)

    def rnd(x):
        return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)
    p = rnd(v * (1.0 - fs.astype(np.float64)))
    q = rnd(v * (1.0 - (fs * f).astype(np.float64)))
    t = rnd(v * (1.0 - fs.astype(np.float64) * (1.0 - f.astype(np.float64))))
    sel = i.astype(np.int32) % 6
    table = [(V, t, p), (q, V, p), (p, V, t), (p, q, V), (t, p, V), (V, p, q)]
    out = np.zeros(hsv.shape, np.int32)
    for k, trip in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(sel == k, trip[c], out[..., c])
    grey_px = S == 0
    for c in range(3):
        out[..., c] = np.where(grey_px, V, out[..., c])
    return out.astype(np.uint8)


def hue_shift(f):
    """The uint8 the PIL backend adds to H: f * 255 truncated toward zero, modulo 256."""
    return int(f * 255) % 256 if f >= 0 else (-(int(-f * 255))) % 256


def hue(img, f):
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(f)) % 256
    return hsv2rgb(hsv)


_OPS = {BRIGHTNESS: brightness, SATURATION: saturation, HUE: hue, CONTRAST: contrast}


def augment_clip(frames, p, num_frames, out_size):
    """frames uint8 [T, H, W, 3]; p: box (i, j, h, w), resize (RH, RW), window (y1, x1), flip, ops [(code, factor), ...]
    -> uint8 [num_frames, ch, cw, 3] (output frame t = source frame t % T, the reference's pad_missing loop)."""
    ch, cw = out_size
    RH, RW = p.resize
    y1, x1 = p.window
    done = []
    for img in frames:
        o = resample(np.asarray(img), p.box, RH, RW)[y1:y1 + ch, x1:x1 + cw]
        if p.flip:
            o = o[:, ::-1]
        for code, f in p.ops:
            o = _OPS[code](np.ascontiguousarray(o), f)
        done.append(o)
    return np.stack([done[t % len(done)] for t in range(num_frames)])


def augment_batch(clips, params, num_frames, out_size):
    """-> uint8 [B, num_frames, ch, cw, 3]: what oracle.clip_oracle.clip_to_tensor_normalize takes."""
    return np.stack([augment_clip(c, p, num_frames, out_size) for c, p in zip(clips, params)])
