"""The GPU audio front end from the decoder's int16 samples (avid_audio_prep, avid_logspec_pcm; datasets/gpu_audio.py).

Two bit-identities and one tolerance:
  * the prepared waveform == the reference's AudioPrep (tests/golden/audio_prep.npz) and, on shapes the golden does not hold, its
    numpy restatement (tests/_audio_ref.py, pinned to that golden on the CPU: tests/test_audio_host.py);
  * the spectrogram from int16 == ``ops.log_spectrogram`` of that waveform: the frame matrix is the same two float32 multiplies
    (gain, window) and everything behind it is the same launch sequence, so this is derivable, not a tolerance;
  * against float64 (oracle/logspec_oracle.py on the restatement's waveform) with tests/test_logspec.py's own tolerances."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _audio_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SR, L_FUZZ = 24000, 24000
# (channels, samples): missing, one sample, shorter than n_stft / 2, L - 1, L, L + 1, much longer.  Packed back to back the clips
# start at element offsets 0, 0, 1, 301, 24300, 72300, 144303: three of them odd (2-byte alignment only)
FUZZ = ((1, 0), (1, 1), (3, 100), (1, 23999), (2, 24000), (3, 24001), (2, 40000))


@functools.lru_cache(maxsize=None)
def _fuzz_host():
    rng = np.random.RandomState(11)
    clips = []
    for C, n in FUZZ:
        c = rng.randint(-32768, 32768, (C, n)).astype(np.int16)
        if n > 2:
            c[:, 0], c[:, 1], c[-1, 2] = 32767, -32768, -32768
        clips.append(c)
    gains = [random.Random(3 + b).uniform(0.9, 1.1) for b in range(len(FUZZ))]
    return clips, gains


@functools.lru_cache(maxsize=None)
def _fuzz_ref(drawn):
    clips, gains = _fuzz_host()
    ref = R.prepared_batch(clips, L_FUZZ, gains if drawn else None)
    ref.setflags(write=False)
    return ref


def _packed(clips, dev):
    """The clips as views into ONE upload, back to back."""
    flat = torch.from_numpy(np.concatenate([c.ravel() for c in clips])).to(dev)
    views, off = [], 0
    for c in clips:
        views.append(flat[off:off + c.size].view(c.shape))
        off += c.size
    return views


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _stats(n_fft, dev):
    rng = np.random.default_rng(5)
    F = n_fft // 2 + 1
    return (torch.from_numpy(rng.uniform(-30, -10, F).astype(np.float32)).to(dev),
            torch.from_numpy(rng.uniform(5, 15, F).astype(np.float32)).to(dev))


# ------------------------------------------------------------------------------------------------------------ waveform bits
def test_audio_prep_equals_the_reference(gpu_device, kernel_log):
    from avid_hip import ops
    meta, cases = R.golden()
    L = int(meta["duration"] * meta["sr"])
    tags = list(cases)
    views = _packed([cases[t][0] for t in tags], gpu_device)
    # the golden's clips one by one with their own augment setting, as the reference ran them ...
    for tag, v in zip(tags, views):
        g = meta["cases"][tag]["gain"]
        got = ops.audio_prep([v], None if g is None else [g], L)
        assert R.same_bits(got.cpu().numpy(), cases[tag][1]), tag
    # ... and as one ragged batch (gain 1.0 = not augmenting: x * 1.0f is x)
    with kernel_log() as log:
        got = ops.audio_prep(views, [1.0 if meta["cases"][t]["gain"] is None else meta["cases"][t]["gain"] for t in tags], L)
    assert log.launches("audio_prep_kernel") == 1
    want = np.concatenate([cases[t][1] for t in tags])
    assert R.same_bits(got.cpu().numpy(), want)


@pytest.mark.parametrize("drawn", [False, True], ids=["gain_one", "gain_drawn"])
def test_audio_prep_equals_the_restatement_on_fuzz(drawn, gpu_device):
    from avid_hip import ops
    clips, gains = _fuzz_host()
    views = _packed(clips, gpu_device)
    assert sum((v.data_ptr() // 2) % 2 for v in views if v.numel()) >= 3          # odd element offsets are exercised
    got = ops.audio_prep(views, gains if drawn else [1.0] * len(views), L_FUZZ)
    assert tuple(got.shape) == (len(FUZZ), L_FUZZ) and R.same_bits(got.cpu().numpy(), _fuzz_ref(drawn))
    if not drawn:
        assert torch.equal(_bits(ops.audio_prep(views, None, L_FUZZ)), _bits(got))


# --------------------------------------------------------------------------------------------------------- spectrogram bits
@pytest.mark.parametrize("normalize", [False, True], ids=["plain", "zscore"])
@pytest.mark.parametrize("cfg", [(256, 0.005, 1.0), (512, 0.01, 1.0)], ids=["256", "512"])
def test_logspec_pcm_is_logspec_of_the_prepared_waveform(cfg, normalize, gpu_device, kernel_log):
    from avid_hip import ops
    n_fft, hop_size, duration = cfg
    clips, gains = _fuzz_host()
    views = _packed(clips, gpu_device)
    L, hop = int(duration * SR), int(hop_size * SR)
    assert L == L_FUZZ
    frames = min(1 + L // hop, int(duration * (1. / hop_size)))       # LogSpectrogram.__call__'s rule
    mean, std = _stats(n_fft, gpu_device) if normalize else (None, None)
    for g in (None, gains):
        want = ops.log_spectrogram(ops.audio_prep(views, g, L), 2 * n_fft, hop, frames, mean, std)
        with kernel_log() as log:
            got = ops.log_spectrogram_pcm(views, g, L, 2 * n_fft, hop, frames, mean, std)
        assert log.launches("logspec_frames_pcm_kernel") == 1 and log.launches("logspec_frames_kernel") == 0
        assert log.launches("audio_prep_kernel") == 0                      # no waveform in between
        assert tuple(got.shape) == (len(FUZZ), 1, frames, n_fft // 2 + 1) and bool(torch.isfinite(got).all())
        assert torch.equal(_bits(got), _bits(want)), (cfg, normalize, g is not None)


# ---------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("kind", ["noise", "chirp", "speech"])
def test_front_end_vs_float64_oracle(kind, gpu_device):
    import test_logspec as LS
    from oracle import logspec_oracle as O
    from datasets.gpu_audio import GpuAudioFrontEnd, GpuAudioPrep, LogSpectrogram
    n_fft, hop_size, duration = 512, 0.01, 1.0
    L = int(duration * SR)
    pcm = [np.clip(np.rint(LS._signal(20 + i, n, kind).astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16)
           for i, n in enumerate((L, L + 1, 31337))]                      # full length: n >= L, mono, gain 1
    front = GpuAudioFrontEnd(GpuAudioPrep(duration=duration, device=gpu_device),
                             LogSpectrogram(SR, n_fft=n_fft, hop_size=hop_size, device=gpu_device))
    got, rate = front([torch.from_numpy(p) for p in pcm], SR, duration)
    for i, p in enumerate(pcm):
        ref, rrate = O.log_spectrogram(R.prepared(p, L)[None], SR, n_fft, hop_size, duration)
        assert rate == rrate and tuple(got[i].shape) == ref.shape
        LS._close_db(got[i].cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------------------------ classes
def test_classes(gpu_device):
    from datasets.gpu_audio import GpuAudioFrontEnd, GpuAudioPrep, LogSpectrogram
    clips, _ = _fuzz_host()
    dev, duration = gpu_device, 1.0
    prep = GpuAudioPrep(duration=duration, missing_as_zero=True, device=dev)
    one, sr = prep(torch.from_numpy(clips[5]), SR)                        # one [C, n] clip -> [1, L], like the reference
    assert sr == SR and tuple(one.shape) == (1, L_FUZZ) and R.same_bits(one.cpu().numpy(), _fuzz_ref(False)[5:6])
    tens, _ = GpuAudioPrep(duration=duration, to_tensor=True, device=dev)(clips[5], SR)        # numpy in, to_tensor: the same
    assert torch.equal(_bits(tens), _bits(one))
    batch, _ = prep([None] + [torch.from_numpy(c) for c in clips[1:]], SR)                     # a missing clip is silence
    assert tuple(batch.shape) == (len(FUZZ), 1, L_FUZZ) and R.same_bits(batch[:, 0].cpu().numpy(), _fuzz_ref(False))
    assert not bool(batch[0].any())
    # duration given at the call wins, as in the reference
    half, _ = prep([torch.from_numpy(clips[4])], SR, duration=0.5)
    assert tuple(half.shape) == (1, 1, 12000) and torch.equal(_bits(half[0, 0]), _bits(batch[4, 0, :12000]))
    # augment: gains drawn per clip in batch order from Python's random, or given
    aug = GpuAudioPrep(duration=duration, missing_as_zero=True, augment=True, device=dev)
    random.seed(9)
    gains = aug.sample(len(FUZZ))
    random.seed(9)
    drawn, _ = aug([torch.from_numpy(c) for c in clips], SR)
    given, _ = aug([torch.from_numpy(c) for c in clips], SR, gains=gains)
    assert torch.equal(_bits(drawn), _bits(given)) and R.same_bits(given[:, 0].cpu().numpy(), R.prepared_batch(clips, L_FUZZ, gains))
    # trim_pad=False: the clips' own length, which they must share
    free = GpuAudioPrep(trim_pad=False, device=dev)
    same, _ = free([torch.from_numpy(clips[4]), torch.from_numpy(clips[4][:1])], SR)
    assert tuple(same.shape) == (2, 1, 24000) and R.same_bits(same[0].cpu().numpy(), _fuzz_ref(False)[4:5])
    with pytest.raises(ValueError):
        free([torch.from_numpy(clips[4]), torch.from_numpy(clips[5])], SR)
    with pytest.raises(TypeError):
        GpuAudioPrep(duration=duration, device=dev)([None], SR)
    # the front end's shape and rate are LogSpectrogram's for the same duration, and its bits LogSpectrogram's of the waveform
    for n_fft, hop_size, dur in ((256, 0.005, 1.0), (512, 0.01, None)):
        spec = LogSpectrogram(SR, n_fft=n_fft, hop_size=hop_size, device=dev)
        spec.mean, spec.std = _stats(n_fft, dev)
        front = GpuAudioFrontEnd(prep, spec)
        want, wrate = spec(batch, SR, dur)
        got, rate = front([torch.from_numpy(c) for c in clips], SR, dur)
        assert rate == wrate and got.shape == want.shape and torch.equal(_bits(got), _bits(want))
        g1, _ = front(torch.from_numpy(clips[5]), SR, dur)
        w1, _ = spec(one, SR, dur)
        assert g1.shape == w1.shape and torch.equal(_bits(g1), _bits(w1))


# ------------------------------------------------------------------------------------------------------------------- guards
def test_no_write_outside_the_buffers(gpu_device):
    """tests/_guards.py: both ops plain and under both fills, every clip in a guarded buffer of its own (a read past a clip's
    end sees the pattern), workspaces of exactly the size functions' answers; no guard byte changes and the outputs are the same
    bits in all three runs."""
    from _guards import FILLS, guarded
    from avid_hip import ops
    dev, n_fft, hop, frames = gpu_device, 256, 120, 200
    clips, gains = _fuzz_host()
    mean, std = _stats(n_fft, dev)

    def run(P):
        views = [P(torch.from_numpy(c).to(dev)) for c in clips]
        wave = ops.audio_prep(views, gains, L_FUZZ)
        spec = ops.log_spectrogram_pcm(views, gains, L_FUZZ, 2 * n_fft, hop, frames, P(mean), P(std))
        torch.cuda.synchronize()
        return _bits(wave), _bits(spec)

    plain = run(lambda t: t)
    assert R.same_bits(plain[0].view(torch.float32).numpy(), _fuzz_ref(True))
    for fill in FILLS:
        with guarded(fill) as g:
            got = run(g.place)
            g.check()
        assert sum(r.kind == "input" for r in g.records) == len(FUZZ) + 2
        assert len(g.workspaces) == 2 and all(asked > 0 and asked in g.size_values for asked, _, _ in g.workspaces), \
            (g.workspaces, sorted(g.size_values))
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), hex(fill)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(gpu_device, kernel_log):
    """Host-side checks only: nothing malformed ever reaches a kernel."""
    import ctypes as C
    from avid_hip import AvidHipError, lib, ops
    dev = gpu_device
    good = torch.zeros((1, 3000), dtype=torch.int16, device=dev)
    nine = torch.zeros((9, 300), dtype=torch.int16, device=dev)
    out = torch.zeros((2, 1, 20, 129), dtype=torch.float32, device=dev)
    ws = torch.zeros(lib.raw("avid_logspec_pcm_workspace_bytes")(2, 512, 20), dtype=torch.uint8, device=dev)
    basis = ops._logspec_basis(dev, 512)
    torch.cuda.synchronize()
    before = out.clone()
    with kernel_log() as log:
        for clips in ([good, nine], [nine]):
            with pytest.raises(AvidHipError, match="9 channels"):
                ops.audio_prep(clips, None, 2000)
            with pytest.raises(AvidHipError, match="9 channels"):
                ops.log_spectrogram_pcm(clips, None, 2000, 512, 80, 20)
        with pytest.raises(AvidHipError):
            ops.log_spectrogram_pcm([good], None, 256, 512, 80, 2)        # L <= n_stft / 2
        arr = (lib.PcmDesc * 2)()
        arr[0].samples, arr[0].channels, arr[0].n, arr[0].gain = good.data_ptr(), 1, 3000, 1.0
        arr[1].samples, arr[1].channels, arr[1].n, arr[1].gain = None, 1, 3000, 1.0                # null with n > 0
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        assert lib.raw("avid_audio_prep")(2, arr, 2000, p(out), p(ws), ws.numel(), None) < 0
        assert "clip 1" in lib.last_error() and "null samples" in lib.last_error()
        assert lib.raw("avid_logspec_pcm")(2, arr, 2000, 512, 80, 20, p(basis), None, None, 100.0, p(out), p(ws), ws.numel(),
                                           None) < 0
        assert "clip 1" in lib.last_error() and "null samples" in lib.last_error()
        arr[1].samples = good.data_ptr()
        assert lib.raw("avid_logspec_pcm")(2, arr, 256, 512, 80, 2, p(basis), None, None, 100.0, p(out), p(ws), ws.numel(),
                                           None) < 0                                                 # L <= n_stft / 2
    assert not log.report, log.report
    assert torch.equal(out, before)
