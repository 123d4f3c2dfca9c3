#!/usr/bin/env python
"""Generate the audio downstream fixtures by IMPORTING the reference (runs only in the build container):

    python tools/make_audio_downstream_golden.py [--ref /root/reference] [--out tests/golden]

* ``audio_downstream_keys.json``: state-dict keys and shapes, in order, of the reference's ``ClassificationWrapper`` and
  ``MOSTModel`` (utils/eval_utils.py) around its ``Conv2D`` (models/audio.py) — 50 classes (ESC-50), ``feat_name="pool"`` with
  dropout for fine-tuning, the four stages with ``AdaptiveMaxPool2d`` heads of 1024 features and BatchNorm for the probe.
* ``audio_downstream.npz``: for the seeded weight set of tests/_audio_downstream.py (``seeded_state``; the weights themselves
  are NOT stored, the seed is) and one (4, 1, 64, 65) input, what the reference computes in float32 on the CPU in training mode:
  fine-tuning — logits, cross-entropy, the gradients of the classifier and of ``feature_extractor.conv1.0.weight``, with the
  reference's ``nn.Dropout`` replaced by the fixed keep-mask that ``HipDropout`` draws at the stored (seed, offset) (restated on
  the host by the oracle's Philox) — and the probe — the four heads' logits.  Only arrays and name lists are stored."""
import argparse
import importlib.util
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_eval_utils(ref):
    sys.path.insert(0, ref)
    import torch  # noqa: F401
    # eval_utils.py imports the reference's data pipeline at module level; only the model classes are needed here
    for name in ("datasets", "utils.videotransforms", "utils.videotransforms.video_transforms",
                 "utils.videotransforms.volume_transforms", "utils.videotransforms.tensor_transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("ref_eval_utils", os.path.join(ref, "utils", "eval_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    mod = reference_eval_utils(args.ref)
    sys.path[1:1] = [REPO, os.path.join(REPO, "tests")]          # oracle/ (Philox) and the shared helper, behind the reference
    import numpy as np
    import torch
    import torch.nn.functional as F
    from models.audio import Conv2D  # reference
    import _audio_downstream as AD

    class FixedDropout(torch.nn.Module):
        """Stands where the reference's ``nn.Dropout`` stood: the fixture's keep-mask, kept features scaled by 1 / (1 - p)."""

        def __init__(self, keep, p):
            super().__init__()
            self.keep, self.p = keep, p

        def forward(self, x):
            return x * self.keep.to(x.dtype) / (1.0 - self.p)

    shape = AD.SMALL
    cls = mod.ClassificationWrapper(Conv2D(), pooling_op=None, **AD.CLS_ARGS)
    most = mod.MOSTModel(Conv2D(), **AD.probe_args(shape))
    keys = {"cls": {"model": "ClassificationWrapper(Conv2D(), 50, 'pool', 512, use_dropout=True)", "args": AD.CLS_ARGS,
                    "state_dict": [[k, list(v.shape)] for k, v in cls.state_dict().items()]},
            "probe": {"model": "MOSTModel(Conv2D(), **args)", "args": AD.probe_args(shape),
                      "state_dict": [[k, list(v.shape)] for k, v in most.state_dict().items()]}}
    with open(os.path.join(args.out, "audio_downstream_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print(f"{len(keys['cls']['state_dict'])} + {len(keys['probe']['state_dict'])} keys -> audio_downstream_keys.json")

    g = torch.Generator().manual_seed(AD.FIXTURE_SEED + 1)
    x = torch.randn(shape, generator=g)
    labels = torch.randint(0, AD.N_CLASSES, (shape[0],), generator=g)
    seed, offset = AD.FIXTURE_DROPOUT
    keep = torch.from_numpy(AD.host_mask(shape[0], 512, 0.5, seed, offset))
    out = {"x": x.numpy(), "labels": labels.numpy(), "weight_seed": np.int64(AD.FIXTURE_SEED),
           "dropout_seed": np.uint64(seed), "dropout_offset": np.int64(offset), "keep": keep.numpy()}

    AD.load_seeded(cls, AD.FIXTURE_SEED).train()
    cls.dropout = FixedDropout(keep, 0.5)
    logits = cls(x)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    out["cls.logits"], out["cls.loss"] = logits.detach().numpy(), loss.detach().numpy()
    grads = dict(cls.named_parameters())
    for k in ("classifier.weight", "classifier.bias", "feature_extractor.conv1.0.weight"):
        out[f"cls.grad.{k}"] = grads[k].grad.numpy()

    AD.load_seeded(most, AD.FIXTURE_SEED).train()
    heads = most(x)
    assert list(heads) == AD.STAGES
    for k, v in heads.items():
        out[f"probe.logits.{k}"] = v.detach().numpy()

    # the float32 reference's own distance from float64 (printed: what a comparison with this fixture can resolve)
    ref64 = AD.restate(cls)
    ref64.keep = keep
    l64 = ref64(x.double())
    loss64 = F.cross_entropy(l64, labels)
    loss64.backward()
    g64 = dict(ref64.named_parameters())
    print("float32 reference against float64: loss rel %.2e, logits %.2e, " % (
        abs(loss.item() - loss64.item()) / abs(loss64.item()), AD.max_rel(logits, l64)) + ", ".join(
        "%s %.2e" % (k, AD.max_rel(grads[k].grad, g64[k].grad)) for k in ("classifier.weight", "classifier.bias",
                                                                          "feature_extractor.conv1.0.weight")))
    p64 = AD.restate(most, shape)(x.double())
    print("probe logits: " + ", ".join("%s %.2e" % (k, AD.max_rel(heads[k], p64[k])) for k in AD.STAGES))

    path = os.path.join(args.out, "audio_downstream.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes -> audio_downstream.npz")


if __name__ == "__main__":
    main()
