"""avid_clip_augment on the GPU against the numpy restatement of the reference's PIL chain (tests/_augment_ref.py, itself
pinned to Pillow and to the reference in tests/test_augment_host.py) followed by oracle.clip_oracle.clip_to_tensor_normalize,
and against the reference's own outputs (tests/golden/augment.npz).  torch.equal everywhere: no tolerance.

Every test is one GPU step under its own time limit (a watchdog ends the process: a hung kernel cannot be interrupted from
Python), and after a failed step the remaining ones fail without touching the GPU."""
import faulthandler
import functools
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_ref as R  # noqa: E402
from oracle import clip_oracle as CO  # noqa: E402
from test_augment_host import golden_cases, golden_params, golden_transform  # noqa: E402

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = 240
_STATE = {"failed": None}
B, S, H, C = R.BRIGHTNESS, R.SATURATION, R.HUE, R.CONTRAST


def gpu_step(fn):
    @functools.wraps(fn)
    def wrapper(*a, **k):
        if _STATE["failed"]:
            pytest.fail(f"not run: the earlier GPU step {_STATE['failed']} failed")
        faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
        try:
            return fn(*a, **k)
        except BaseException:
            _STATE["failed"] = fn.__name__
            raise
        finally:
            faulthandler.cancel_dump_traceback_later()
    return wrapper


def P(box, resize, window=(0, 0), flip=False, ops=()):
    from datasets.gpu_video import ClipAugParams
    return ClipAugParams(tuple(box), tuple(resize), tuple(window), flip, list(ops))


def frames(seed, T, Hh, W):
    """Smooth colour structure + noise + the extremes: resampling, saturation and hue all have something to act on."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:Hh, 0:W]
    base = np.stack([(yy * 5 + xx * 2) % 256, (xx * 7 + 40) % 256, (yy * 3 + xx * 3 + 90) % 256], -1)
    f = np.clip(base[None] + rng.randint(-70, 71, (T, Hh, W, 3)), 0, 255).astype(np.uint8)
    f[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [3, 3, 3]]
    return f


def check(dev, clips, params, nf, out_size, mean=CO.MEAN, std=CO.STD, dense=False):
    from avid_hip import ops
    want = CO.clip_to_tensor_normalize(R.augment_batch(clips, params, nf, out_size), mean, std)
    src = torch.from_numpy(np.stack(clips)).to(dev) if dense else [torch.from_numpy(c).to(dev) for c in clips]
    got = ops.clip_augment(src, params, nf, out_size, mean, std)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.dtype == torch.float32
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want).flatten(2).any(2).any(1).nonzero().flatten().tolist()
        n = int((got != want).sum())
        raise AssertionError(f"{n} of {want.numel()} values differ, clips {bad}: {[params[b] for b in bad[:3]]}")
    return got


@gpu_step
def test_resample_geometry(gpu_device):
    """Up- and down-scaling, a scale above 8 on both axes (ksize 23 / 21: several staging rounds per tile), one pass or both
    skipped, odd widths, partial tiles, a window inside the resampled image; no colour operation."""
    a = frames(1, 2, 200, 183)
    cases = [
        (P((0, 0, 200, 183), (20, 18)), (20, 18)),                  # scale 10 and 10.2
        (P((3, 5, 190, 170), (19, 17)), (19, 17)),
        (P((10, 20, 40, 50), (96, 130)), (96, 130)),                # up-scaling
        (P((10, 20, 40, 50), (40, 33)), (40, 33)),                  # vertical pass skipped
        (P((10, 20, 40, 50), (61, 50)), (61, 50)),                  # horizontal pass skipped
        (P((7, 9, 33, 41), (33, 41)), (33, 41)),                    # both skipped: a plain crop
        (P((0, 0, 200, 183), (64, 59), (5, 3)), (40, 37)),          # Resize + window, odd sizes
        (P((0, 0, 200, 183), (224, 205), (100, 90)), (9, 33)),      # the last rows and columns of an up-scaled image
        (P((199, 182, 1, 1), (8, 5)), (8, 5)),                      # a one-pixel box
        (P((0, 0, 200, 183), (1, 1)), (1, 1)),
    ]
    for p, size in cases:
        check(gpu_device, [a], [p], 2, size)
        check(gpu_device, [a], [p._replace(flip=True)], 2, size)


@gpu_step
def test_ragged_batch_frame_mapping_and_flip(gpu_device):
    """Clips of differing sizes and frame counts in one call; output frame t = source frame t % T; flips per clip; a
    single-clip call; other mean / std (ClipToTensor alone: mean 0, std 1)."""
    clips = [frames(2, 3, 48, 64), frames(3, 1, 37, 53), frames(4, 5, 90, 61), frames(5, 2, 24, 31)]
    params = [P((4, 6, 40, 50), (28, 36), flip=True, ops=[(B, 1.2), (C, 0.8)]),
              P((0, 0, 37, 53), (28, 36), ops=[(H, 0.1)]),
              P((0, 0, 90, 61), (60, 40), (20, 2), flip=True, ops=[(C, 1.3), (S, 0.4)]),
              P((1, 1, 20, 29), (28, 36))]
    got = check(gpu_device, clips, params, 5, (28, 36))
    assert torch.equal(got[1, :, 0], got[1, :, 4]) and torch.equal(got[3, :, 0], got[3, :, 2])
    assert torch.equal(got[0, :, 1], got[0, :, 4])
    one = check(gpu_device, clips[2:3], params[2:3], 5, (28, 36))
    assert torch.equal(one[0], got[2])
    check(gpu_device, clips, params, 2, (28, 36), mean=(0., 0., 0.), std=(1., 1., 1.))
    check(gpu_device, clips, params, 3, (28, 36), mean=(0.1, 0.5, 0.9), std=(0.3, 1.0, 2.5))


FACTORS = (0.0, 1.0, 0.3, 0.6180339887, 0.8998035936506915, 1.0699078630799175, 1.4, 2.5, 7.0)


@gpu_step
@pytest.mark.parametrize("op", [B, S, C])
def test_each_blend_operation_alone(op, gpu_device):
    """Factors at 0 and 1, inside and outside [0, 1] (a fused multiply-add in the blend shows at the inexact ones)."""
    clips = [frames(10 + n, 2, 40, 56) for n in range(len(FACTORS))]
    params = [P((2, 3, 36, 50), (30, 44), flip=bool(n & 1), ops=[(op, f)]) for n, f in enumerate(FACTORS)]
    check(gpu_device, clips, params, 2, (30, 44))


@gpu_step
def test_hue_alone(gpu_device):
    """Both signs, zero, the ends of the range, shifts that truncate toward zero; every hue sector and the grey axis."""
    fs = (-0.5, -0.150789461747335, -0.0023861283571298963, 0.0, 0.004, 0.05195308808672078, 0.19872677483915963, 0.5)
    clips = [frames(30 + n, 2, 40, 56) for n in range(len(fs))]
    for c in clips:
        c[1, 5, :8] = [[9, 9, 9], [255, 255, 254], [1, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    params = [P((0, 0, 40, 56), (40, 56), ops=[(H, f)]) for f in fs]
    check(gpu_device, clips, params, 2, (40, 56))
    # a dense sweep of colours through the conversions: 64 x 64 x 64 lattice as one 512 x 512 frame
    v = (np.arange(64) * 4 + np.arange(64) % 4).astype(np.uint8)
    lat = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(1, 512, 512, 3)
    for f in (-0.31, 0.07):
        check(gpu_device, [np.ascontiguousarray(lat)], [P((0, 0, 512, 512), (512, 512), ops=[(H, f)])], 1, (512, 512))


@gpu_step
def test_all_orders_of_four_operations(gpu_device):
    """All 24 orders in one ragged call: contrast first, in the middle and last (its grey mean is taken after whatever
    precedes it), plus subsets without contrast, contrast alone and no operation at all."""
    fac = {B: 1.2840365, S: 0.6086883544720544, H: -0.10855610986043351, C: 0.7519216250458975}
    orders = [list(o) for o in itertools.permutations((B, S, H, C))]
    orders += [[B, S, H], [H, S], [C], [], [S, C], [C, H]]
    clips = [frames(50 + n, 2, 30 + n % 5, 41 + n % 7) for n in range(len(orders))]
    params = [P((1, 2, 28, 38), (20, 28), flip=bool(n % 3 == 0), ops=[(o, fac[o] + 0.01 * n * (o != H)) for o in order])
              for n, order in enumerate(orders)]
    check(gpu_device, clips, params, 3, (20, 28))


@gpu_step
def test_kernel_log_names_the_kernels(gpu_device, kernel_log):
    """The library's timers name what ran: the contrast kernel only when a clip uses contrast."""
    a = [frames(70, 2, 30, 40)]
    with kernel_log() as log:
        check(gpu_device, a, [P((0, 0, 30, 40), (16, 16), ops=[(B, 1.1)])], 2, (16, 16))
    assert log.launches("clip_augment_kernel") == 1 and log.launches("clip_contrast_kernel") == 0
    with kernel_log() as log:
        check(gpu_device, a, [P((0, 0, 30, 40), (16, 16), ops=[(B, 1.1), (C, 1.1)])], 2, (16, 16))
    assert log.launches("clip_augment_kernel") == 1 and log.launches("clip_contrast_kernel") == 1


@gpu_step
def test_reference_golden(gpu_device):
    """The reference's own outputs, from the recorded parameters and from sample() under the recorded seed."""
    for tag, (f, want, m) in golden_cases().items():
        t = golden_transform(m)
        nf, ch, cw = want.shape[1:]
        clip = torch.from_numpy(f).to(gpu_device)
        got = t([clip], [golden_params(m)])
        assert tuple(got.shape) == (1,) + want.shape and np.array_equal(got[0].cpu().numpy(), want), tag
        random.seed(m["seed"])
        got = t(clip)                                       # one clip in, one clip out; parameters drawn here
        assert np.array_equal(got.cpu().numpy(), want), tag


@gpu_step
def test_transform_classes_real_shapes_and_dense_form(gpu_device):
    """Resize + CenterCrop (evaluation), Resize + RandomCrop (fine-tuning) and RandomResizedCrop (pretraining) at 112 and 224
    on decoded-size frames; the dense [B, T, H, W, 3] form of the op and of the classes."""
    from datasets.gpu_video import GpuVideoPrep_Crop_CJ, GpuVideoPrep_MSC_CJ
    clips = [frames(80 + n, 2, 120, 160) for n in range(3)]
    dense = torch.from_numpy(np.stack(clips)).to(gpu_device)
    random.seed(7)
    for t in (GpuVideoPrep_MSC_CJ(crop=(112, 112), num_frames=2), GpuVideoPrep_MSC_CJ(crop=(112, 112), augment=False),
              GpuVideoPrep_Crop_CJ(resize=(128, 171), crop=(112, 112), num_frames=4, pad_missing=True),
              GpuVideoPrep_Crop_CJ(resize=(128, 128), crop=(112, 112), augment=False),
              GpuVideoPrep_MSC_CJ(crop=(224, 224), num_frames=2), GpuVideoPrep_Crop_CJ(augment=False)):
        params = t.sample([c.shape[1:3] for c in clips])
        nf = max(2, t.num_frames) if t.pad_missing else 2
        want = check(gpu_device, clips, params, nf, t.crop, dense=True)
        assert torch.equal(t(dense, params).cpu(), want)
        assert torch.equal(t(list(dense.unbind(0)), params).cpu(), want)
    t = GpuVideoPrep_MSC_CJ(crop=(32, 32), normalize=False, augment=False)
    got = t(dense)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0                # ClipToTensor alone
    with pytest.raises(ValueError):
        GpuVideoPrep_MSC_CJ(crop=(32, 32))([dense[0], dense[1, :1]])          # frame counts differ, no padding


@gpu_step
def test_back_to_back_calls_keep_their_tables(gpu_device):
    """Calls issued without a host synchronisation in between: a later call's staging never overwrites tables an earlier
    copy is still reading (each result is checked after all were issued)."""
    from avid_hip import ops
    jobs = []
    for n in range(12):
        clip = frames(90 + n, 2, 60 + n, 80 - n)
        p = P((n, 1, 50, 60), (24 + n, 40 - n), flip=bool(n & 1), ops=[(S, 0.5 + 0.1 * n), (C, 1.2), (H, 0.01 * n)])
        jobs.append((clip, p, (24 + n, 40 - n)))
    outs = [ops.clip_augment([torch.from_numpy(c).to(gpu_device)], [p], 2, size).clone() for c, p, size in jobs]
    torch.cuda.synchronize()
    for (c, p, size), got in zip(jobs, outs):
        assert torch.equal(got.cpu(), CO.clip_to_tensor_normalize(R.augment_batch([c], [p], 2, size)))


@gpu_step
def test_bad_arguments_raise(gpu_device):
    from avid_hip import ops, AvidHipError
    clip = torch.zeros(2, 20, 30, 3, dtype=torch.uint8, device=gpu_device)
    ok = P((0, 0, 20, 30), (16, 16))
    for bad in (ok._replace(box=(0, 0, 21, 30)), ok._replace(resize=(15, 16)), ok._replace(ops=[(7, 1.0)]),
                ok._replace(ops=[(B, 1.0)] * 5), ok._replace(ops=[(H, 0.7)])):
        with pytest.raises(AvidHipError):
            ops.clip_augment([clip], [bad], 2, (16, 16))
    with pytest.raises(AvidHipError):
        ops.clip_augment([clip.float()], [ok], 2, (16, 16))
    with pytest.raises(AvidHipError):
        ops.clip_augment([clip], [ok], 2, (16, 16), std=(1.0, 0.0, 1.0))
    with pytest.raises(AvidHipError):
        ops.clip_augment([clip, clip], [ok], 2, (16, 16))
    assert ops.clip_augment([clip], [ok], 2, (16, 16)).shape == (1, 3, 2, 16, 16)
