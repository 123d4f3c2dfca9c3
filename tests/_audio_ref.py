"""numpy restatement of the audio chain in front of the spectrogram: the decoder's scaling (reference
utils/ioutils/av_wrappers.py:111) and AudioPrep (datasets/preprocessing.py:116-155), written the way include/avid_hip.h states
the prepared sample, so that the statement itself is what tests/golden/audio_prep.npz (the reference's own outputs,
tools/make_golden_audio.py) pins on the CPU (tests/test_audio_host.py).  The GPU tests use it for shapes the golden does not
hold."""
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decoded(pcm):
    """What the decoder hands the transforms: int16 ``[C, n]`` -> float64 ``[C, n]`` = k / 32767."""
    return np.asarray(pcm, dtype=np.int16) / 32767.0


def prepared(pcm, length, gain=None):
    """int16 ``[C, n]`` (n = 0: a missing clip) -> float32 ``[length]``.
        p <  n:  float32( (s[0][p] / 32767 + s[1][p] / 32767 + ...) / C )   summed in channel order, in float64
        p >= n:  0
        then one float32 multiply by float32(gain) (gain None: not augmenting, nothing is multiplied)"""
    pcm = np.asarray(pcm, dtype=np.int16)
    C, n = pcm.shape
    m = min(n, int(length))
    acc = np.zeros(m, np.float64)
    for c in range(C):
        acc = pcm[c, :m].astype(np.float64) / 32767.0 if c == 0 else acc + pcm[c, :m].astype(np.float64) / 32767.0
    out = np.zeros(int(length), np.float32)
    out[:m] = (acc / np.float64(C)).astype(np.float32)
    if gain is not None:
        out = out * np.float32(gain)
    return out


def prepared_batch(clips, length, gains=None):
    """``[B, length]`` float32: ``prepared`` per clip."""
    gains = [None] * len(clips) if gains is None else gains
    return np.stack([prepared(c, length, g) for c, g in zip(clips, gains)])


def golden():
    """(meta, {tag: (int16 input, the reference's float32 [1, L] output)}) of tests/golden/audio_prep.npz."""
    g = np.load(os.path.join(REPO, "tests", "golden", "audio_prep.npz"))
    meta = json.loads(str(g["meta"]))
    return meta, {tag: (g[f"{tag}_pcm"], g[f"{tag}_out"]) for tag in meta["cases"]}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
