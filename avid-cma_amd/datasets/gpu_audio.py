"""Batched log-spectrogram on the GPU — drop-in for ``datasets.preprocessing.LogSpectrogram``
(reference ``datasets/preprocessing.py:158-186``).

Same constructor and ``__call__(sig, sr, duration=None) -> (spect, rate)`` contract; additionally accepts a
batch ``[B, 1, nsamples]`` (or ``[B, nsamples]``) of mono clips already on the GPU and then returns
``[B, 1, T, n_fft/2 + 1]`` — the layout ``main-avid.py`` feeds the audio encoder — in one call
(``avid_logspec``: frames -> DFT as one fp32-MFMA GEMM -> power / pair-mean / dB / top_db floor / z-score).
The reference runs librosa per clip on 36-72 CPU workers (Cross-N1024.yaml:3).

The part in front of it, the reference's ``AudioPrep`` (``datasets/preprocessing.py:116-155``: downmix, trim / zero-pad to
``int(duration * sr)`` samples, +-10 % volume jitter), runs on the GPU too: the DataLoader workers hand over the decoder's int16
samples (``RawAudio``, ``collate_raw``) and ONE call per batch on the training stream turns the ragged batch into the
network's input (``GpuAudioFrontEnd`` -> ``avid_logspec_pcm``; ``GpuAudioPrep`` -> ``avid_audio_prep`` where the waveform
itself is wanted).  The waveform is bit-identical to the reference's and the spectrogram is bit-identical to ``LogSpectrogram``
applied to that waveform; the gains are drawn on the host from Python's ``random`` in the reference's call order.
"""
import random

import numpy as np
import torch

from avid_hip import ops

__all__ = ["LogSpectrogram", "RawAudio", "GpuAudioPrep", "GpuAudioFrontEnd", "collate_raw"]

_STATS = {(512, 24000): "datasets/assets/audio-spectDB-24k-513-norm-stats.npz",
          (256, 24000): "datasets/assets/audio-spectDB-24k-257-norm-stats.npz"}


class LogSpectrogram(object):
    def __init__(self, fps, n_fft=512, hop_size=0.005, normalize=False, device="cuda", stats=None):
        self.inp_fps = fps
        self.n_fft = n_fft
        self.hop_size = hop_size
        self.rate = 1. / hop_size
        self.normalize = normalize
        self.device = torch.device(device)
        self.mean = self.std = None
        if self.normalize:
            # the reference reads these files relative to its checkout (preprocessing.py:167-171); ``stats`` may
            # name another .npz with 'mean' / 'std' arrays of n_fft/2 + 1 bins
            path = stats if stats is not None else _STATS[(n_fft, int(fps))]
            st = np.load(path)
            self.mean = torch.as_tensor(st['mean'], dtype=torch.float32, device=self.device).contiguous()
            self.std = torch.as_tensor(st['std'], dtype=torch.float32, device=self.device).contiguous()

    def __call__(self, sig, sr, duration=None):
        single = False
        if isinstance(sig, np.ndarray):
            sig = torch.from_numpy(np.ascontiguousarray(sig, dtype=np.float32))
        if sig.dim() == 2 and sig.shape[0] == 1:           # the reference's [1, nsamples] (AudioPrep output)
            single = True
        elif sig.dim() == 3:                               # [B, 1, nsamples]
            sig = sig[:, 0]
        sig = sig.to(self.device, torch.float32).contiguous()
        hop_length = int(self.hop_size * sr)
        frames = 1 + sig.shape[1] // hop_length
        if duration is not None:
            frames = min(frames, int(duration * self.rate))
        spect = ops.log_spectrogram(sig, 2 * self.n_fft, hop_length, frames, self.mean, self.std, top_db=100.)
        return (spect[0] if single else spect), self.rate


class RawAudio(object):
    """``audio_transform`` for the DataLoader workers: what the decoder returns -> the int16 samples it decoded, ``[C, n]``.

    ``av_laod_audio`` (reference ``utils/ioutils/av_wrappers.py:111``) returns ``data / np.iinfo(int16).max``, float64; the
    integers are recovered with ``rint(sig * 32767)`` and checked (``k / 32767 == sig`` everywhere, else ``TypeError``: the
    array is not the decoder's).  int16 input passes through.  ``None`` (a missing clip) with ``missing_as_zero`` becomes an
    empty ``[1, 0]`` tensor, which the GPU side pads to silence as the reference does."""

    def __init__(self, missing_as_zero=False):
        self.missing_as_zero = missing_as_zero

    def __call__(self, sig, sr, duration=None):
        if sig is None:
            if not self.missing_as_zero:
                raise TypeError("RawAudio: the clip is missing and missing_as_zero is not set")
            return torch.zeros((1, 0), dtype=torch.int16), sr
        if isinstance(sig, torch.Tensor):
            sig = sig.numpy()
        sig = np.asarray(sig)
        if sig.ndim != 2:
            raise TypeError(f"RawAudio expects [channels, samples], got an array of shape {sig.shape}")
        if sig.dtype != np.int16:
            if sig.dtype.kind != "f":
                raise TypeError(f"RawAudio expects int16 samples or the decoder's float64 array, got {sig.dtype}")
            k = np.rint(sig.astype(np.float64) * 32767.0)
            if not (np.all((k >= -32768) & (k <= 32767)) and np.array_equal(k / 32767.0, sig)):
                raise TypeError("RawAudio: the samples are not int16 / 32767 (resampled or rescaled after decoding?)")
            sig = k.astype(np.int16)
        return torch.from_numpy(np.ascontiguousarray(sig)), sr


class GpuAudioPrep(object):
    """``AudioPrep`` (datasets/preprocessing.py:116-155) on the GPU, for a batch: same constructor arguments and defaults (plus
    ``device``).  ``__call__(clips, sr, duration=None, gains=None)``: ``clips`` a list of int16 ``[C_b, n_b]`` tensors (what
    ``RawAudio`` returned; uploaded here when they are on the host) -> (fp32 ``[B, 1, L]`` on the GPU, sr) with
    ``L = int(duration * sr)``; one ``[C, n]`` clip gives ``[1, L]`` like the reference.  ``to_tensor`` is accepted for
    signature parity: the result is a tensor either way."""

    def __init__(self, trim_pad=True, duration=None, missing_as_zero=False, augment=False, to_tensor=False, volume=0.1,
                 device="cuda"):
        self.trim_pad = trim_pad
        self.missing_as_zero = missing_as_zero
        self.augment = augment
        self.to_tensor = to_tensor
        self.volume = volume
        self.device = torch.device(device)
        if trim_pad:
            assert duration is not None
            self.duration = duration

    def sample(self, n_clips):
        """One ``random.uniform(1 - volume, 1 + volume)`` per clip, in batch order (the order a single-process reference loader
        would have drawn them in); ``None`` without ``augment`` (nothing is drawn)."""
        if not self.augment:
            return None
        return [random.uniform(1. - self.volume, 1. + self.volume) for _ in range(n_clips)]

    def _batch(self, clips, sr, duration, gains):
        """(list of int16 [C, n] device tensors, gains, L, whether ``clips`` was one clip)."""
        single = isinstance(clips, (torch.Tensor, np.ndarray)) or clips is None
        if single:
            clips = [clips]
        clips = list(clips)
        for b, c in enumerate(clips):
            if c is None:
                if not self.missing_as_zero:
                    raise TypeError(f"clip {b} is missing and missing_as_zero is not set")
                c = torch.zeros((1, 0), dtype=torch.int16)
            elif isinstance(c, np.ndarray):
                c = torch.from_numpy(np.ascontiguousarray(c))
            clips[b] = c.to(self.device, non_blocking=True).contiguous()
        if self.trim_pad:
            if duration is None:
                duration = self.duration
            length = int(duration * sr)
        else:
            lengths = sorted({int(c.shape[-1]) for c in clips})
            if len(lengths) != 1:
                raise ValueError(f"trim_pad=False and the clips of one batch differ in length: {lengths}")
            length = lengths[0]
        if gains is None:
            gains = self.sample(len(clips))
        return clips, gains, length, single

    def __call__(self, clips, sr, duration=None, gains=None):
        clips, gains, length, single = self._batch(clips, sr, duration, gains)
        out = ops.audio_prep(clips, gains, length)
        return (out if single else out.unsqueeze(1)), sr


class GpuAudioFrontEnd(object):
    """``AudioPrep`` + ``LogSpectrogram`` for a ragged batch of int16 clips in one call on the training stream:
    ``GpuAudioFrontEnd(GpuAudioPrep(...), LogSpectrogram(...))``; ``__call__(clips, sr, duration=None, gains=None) ->
    (spect [B, 1, T, n_fft/2 + 1], rate)`` — the bits of ``spectrogram(prep(clips, sr, duration, gains)[0], sr, duration)``
    (``T`` by the same rule), through ``avid_logspec_pcm``: no waveform is written.  One ``[C, n]`` clip gives ``[1, T, F]``."""

    def __init__(self, prep, spectrogram):
        self.prep, self.spectrogram = prep, spectrogram

    def __call__(self, clips, sr, duration=None, gains=None):
        sp = self.spectrogram
        clips, gains, length, single = self.prep._batch(clips, sr, duration, gains)
        hop_length = int(sp.hop_size * sr)
        frames = 1 + length // hop_length
        if duration is not None:
            frames = min(frames, int(duration * sp.rate))
        spect = ops.log_spectrogram_pcm(clips, gains, length, 2 * sp.n_fft, hop_length, frames, sp.mean, sp.std, top_db=100.)
        return (spect[0] if single else spect), sp.rate


def collate_raw(batch):
    """``collate_fn``: the default collation for every key but ``frames`` and ``audio``, which stay lists where present
    (``[T, H, W, 3]`` uint8 clips for ``datasets.gpu_video``, ``[C, n]`` int16 clips for ``GpuAudioFrontEnd``: decoded sizes
    differ from sample to sample)."""
    from torch.utils.data import default_collate
    raw = ("frames", "audio")
    out = default_collate([{k: v for k, v in s.items() if k not in raw} for s in batch])
    for k in raw:
        if k in batch[0]:
            out[k] = [s[k] for s in batch]
    return out
