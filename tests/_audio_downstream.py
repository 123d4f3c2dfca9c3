"""What tests/test_audio_downstream_host.py, tests/test_gpu_audio_downstream.py and tools/make_audio_downstream_golden.py share:
the audio downstream models (fine-tuning and linear probe around ``Conv2D``) at the test geometries, one seeded weight set that
any module with the reference's state-dict keys can be given, and a pure-torch restatement of the two models — the audio tower
(models/audio.py of the reference: a 7x7 / 2 stem and four blocks of two 3x3 convolutions, each followed by BatchNorm + ReLU,
then a global max pool), ``Linear`` behind a fixed dropout keep-mask, and per tap ``AdaptiveMaxPool2d -> BatchNorm1d -> Linear``
— which ``.double()`` turns into the float64 yardstick.  The restatement calls no avid_hip op and runs on the host."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

STAGES = ["conv2x", "conv3x", "conv4x", "conv5x"]
N_CLASSES = 50
# spectrogram batch [B, 1, T, F] -> (the four heads' AdaptiveMaxPool2d sizes, their feature counts)
HEADS = {(4, 1, 64, 65): ([(4, 4), (2, 4), (2, 2), (1, 2)], [1024, 1024, 1024, 1024]),        # taps 16x17, 8x9, 4x5, 4x5
         (3, 1, 50, 33): ([(3, 2), (2, 2), (2, 1), (1, 1)], [384, 512, 512, 512]),            # taps 13x9, 7x5, 4x3, 4x3
         (4, 1, 200, 257): ([(12, 12), (8, 8), (6, 6), (4, 4)], [9216, 8192, 9216, 8192])}    # taps 50x65, 25x33, 13x17, 13x17
SMALL, ODD, SHIPPED = (4, 1, 64, 65), (3, 1, 50, 33), (4, 1, 200, 257)
CLS_ARGS = dict(n_classes=N_CLASSES, feat_name="pool", feat_dim=512, use_dropout=True)
FIXTURE_SEED, FIXTURE_DROPOUT = 1234, (0x5EED_A0D1_0123_4567, 3)      # the fixture's weight seed, its dropout (seed, offset)


def pool_strings(shape):
    return ["AdaptiveMaxPool2d((%d,%d))" % hw for hw in HEADS[shape][0]]


def probe_args(shape):
    return dict(n_classes=N_CLASSES, feat_names=list(STAGES), feat_dims=list(HEADS[shape][1]), pooling_ops=pool_strings(shape),
                use_bn=True)


def seeded_state(entries, seed):
    """{key: float32 tensor} for ``entries`` = [(key, shape)] in state-dict order, drawn from ONE generator: convolution and
    linear weights N(0, 2 / fan_in), linear biases and BatchNorm shifts N(0, 0.1^2), BatchNorm scales 1 + N(0, 0.1^2), running
    means N(0, 0.1^2), running variances U(0.5, 1.5), counters 0.  The draw depends on the keys' order and shapes only."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shape in entries:
        shape = tuple(shape)
        if key.endswith("num_batches_tracked"):
            out[key] = torch.zeros(shape, dtype=torch.int64)
        elif key.endswith("running_var"):
            out[key] = torch.rand(shape, generator=g) + 0.5
        elif len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            out[key] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif key.endswith("weight"):
            out[key] = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            out[key] = 0.1 * torch.randn(shape, generator=g)
    return out


def load_seeded(model, seed):
    """Give ``model`` the seeded weight set of its own state-dict entries (in place); returns the model."""
    sd = model.state_dict()
    model.load_state_dict(seeded_state([(k, v.shape) for k, v in sd.items()], seed))
    return model


def host_mask(B, Fd, p, seed, offset):
    """``HipDropout``'s keep-mask [B, Fd] (bool) restated on the host from oracle.avid_oracle.philox4x32_10, as
    tests/test_gpu_finetune.py restates it."""
    from oracle import avid_oracle as O
    n = B * Fd
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    U32 = np.uint64(0xFFFFFFFF)
    words = O.philox4x32_10(g & U32, g >> np.uint64(32), np.uint64(offset) & U32, np.uint64(offset) >> np.uint64(32),
                            np.uint64(seed) & U32, np.uint64(seed) >> np.uint64(32))
    w = np.stack(words, 1).reshape(-1)[:n]
    thresh = np.uint64(int(np.floor(np.float64(np.float32(p)) * 2.0 ** 32)))
    return (w >= thresh).reshape(B, Fd)


# ---- this package's models ---------------------------------------------------------------------------------------------
def cls_model(seed=FIXTURE_SEED, **kw):
    import models
    args = dict(CLS_ARGS)
    args.update(kw)
    m = load_seeded(models.ClassificationWrapper(models.Conv2D(), **args), seed)
    if m.use_dropout:
        m.dropout.seed = FIXTURE_DROPOUT[0]          # (HipDropout draws its seed from torch's generator: one model, one mask)
    return m


def probe_model(shape, seed=FIXTURE_SEED, **kw):
    import models
    args = probe_args(shape)
    args.update(kw)
    return load_seeded(models.MOSTModel(models.Conv2D(), **args), seed)


def tower_model(seed=FIXTURE_SEED):
    import models
    return load_seeded(models.Conv2D(), seed)


# ---- the pure-torch restatement ----------------------------------------------------------------------------------------
BN_NAMES = ["conv1.1"] + [f"block{b}.bn{k}" for b in (1, 2, 3, 4) for k in (1, 2)]      # the tower's nine BatchNorm + ReLU pairs


class TorchTower(nn.Module):
    """``pins`` (None: plain ReLU and max): {BatchNorm name: bool mask [B, C, H, W] of the outputs its ReLU lets through, "pool":
    int64 [B, C] position h * W + w the global max pool picks} — the decisions another run of the same tower took.  Float32 and
    float64 disagree on them only where a pre-activation lies within rounding of zero, or two maxima within rounding of each
    other; there a gradient changes by a whole element, not by rounding, which is why tests/test_gpu_finetune.py pins them too.
    ``seen`` holds the decisions of the last forward in the same form."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(1, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU())
        for b, (cin, cout, stride) in enumerate(((64, 64, 2), (64, 128, 2), (128, 256, 2), (256, 512, 1)), 1):
            blk = nn.Module()
            blk.conv1, blk.bn1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout)
            blk.conv2, blk.bn2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout)
            setattr(self, f"block{b}", blk)
        self.pins, self.seen = None, {}

    def _relu(self, name, x):
        self.seen[name] = x.detach() > 0
        if self.pins is None:
            return F.relu(x)
        return x * self.pins[name].to(x.dtype)

    def forward(self, x, return_embs=False):
        taps = {}
        h = self._relu("conv1.1", self.conv1[1](self.conv1[0](x)))
        for b, name in enumerate(STAGES, 1):
            blk = getattr(self, f"block{b}")
            h = self._relu(f"block{b}.bn1", blk.bn1(blk.conv1(h)))
            h = taps[name] = self._relu(f"block{b}.bn2", blk.bn2(blk.conv2(h)))
        flat = h.flatten(2)
        self.seen["pool"] = flat.detach().argmax(2)
        picks = self.seen["pool"] if self.pins is None else self.pins["pool"]
        taps["pool"] = flat.gather(2, picks[:, :, None])[:, :, :, None]
        return taps if return_embs else taps["pool"]


class TorchCls(nn.Module):
    """``ClassificationWrapper(Conv2D(), n, "pool", 512, use_dropout=True)``: ``keep`` (None: no dropout, or eval mode) is the
    keep-mask [B, 512] of the call, kept features scaled by 1 / (1 - p)."""

    def __init__(self, n_classes=N_CLASSES, p=0.5):
        super().__init__()
        self.feature_extractor = TorchTower()
        self.classifier = nn.Linear(512, n_classes)
        self.p, self.keep = p, None

    def forward(self, x):
        f = self.feature_extractor(x).flatten(1)
        if self.keep is not None and self.training:
            f = f * self.keep.to(f.dtype) / (1.0 - self.p)
        return self.classifier(f)


class _TorchHead(nn.Module):
    def __init__(self, hw, feat_dim, n_classes):
        super().__init__()
        self.hw = hw
        self.bn = nn.BatchNorm1d(feat_dim)
        self.classifier = nn.Linear(feat_dim, n_classes)

    def forward(self, x):
        return self.classifier(self.bn(F.adaptive_max_pool2d(x, self.hw).flatten(1)))


class TorchProbe(nn.Module):
    """``MOSTModel(Conv2D(), n, conv2x..conv5x, dims, AdaptiveMaxPool2d strings, use_bn=True)``; the tower takes no gradient."""

    def __init__(self, shape, n_classes=N_CLASSES):
        super().__init__()
        self.feature_extractor = TorchTower()
        self.classifiers = nn.ModuleList([_TorchHead(hw, d, n_classes) for hw, d in zip(*HEADS[shape])])
        for p in self.feature_extractor.parameters():
            p.requires_grad = False

    def forward(self, x):
        with torch.no_grad():
            taps = self.feature_extractor(x, return_embs=True)
        return {name: c(taps[name]) for name, c in zip(STAGES, self.classifiers)}


def restate(model, shape=None):
    """The float64 restatement of one of this package's audio models (or of any module with the same state-dict), in the mode
    ``model`` is in."""
    kind = type(model).__name__
    ref = {"Conv2D": TorchTower, "ClassificationWrapper": TorchCls}[kind]() if kind != "MOSTModel" else TorchProbe(shape)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return ref.double().train(model.training)


def max_rel(got, want):
    """max |got - want| / max |want|, in float64 on the host."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))
