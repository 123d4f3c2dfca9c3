#!/usr/bin/env python
"""Generate the linear-probe fixtures by IMPORTING the reference (runs only in the build container):

    python tools/make_golden_probe.py [--ref /root/reference] [--out tests/golden]

* ``most_model_keys.json``: state-dict keys and shapes, in order, of the reference's ``MOSTModel`` (utils/eval_utils.py) around
  its ``R2Plus1D`` depth 18 with the arguments of configs/benchmark/kinetics/8x224x224-linear.yaml.
* ``most_heads.npz``: a stub extractor's taps (float32 values) and what the reference's heads make of them in float64 in
  training mode — logits per tap, the summed cross-entropy, the gradient of every classifier parameter, the BatchNorm1d
  running statistics after the pass.  Small sizes: 7 classes, batch 4, at most 256 features per head (one head pools to MORE
  outputs than its tap has positions).  Only data is stored."""
import argparse
import importlib.util
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIPPED = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
               pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                            "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)
# name: (tap shape [B, C, T, H, W], pooling op, features)
HEADS = {"a": ((4, 4, 2, 5, 5), "AdaptiveMaxPool3d((1,2,2))", 16),
         "b": ((4, 8, 1, 3, 3), "AdaptiveMaxPool3d((1,4,4))", 128),
         "c": ((4, 16, 3, 4, 6), "AdaptiveMaxPool3d((2,2,3))", 192)}
N_CLASSES = 7


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
    import numpy as np
    import torch
    from models.video import R2Plus1D  # reference

    m = mod.MOSTModel(R2Plus1D(depth=18), **SHIPPED)
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(args.out, "most_model_keys.json"), "w") as f:
        json.dump({"model": "MOSTModel(R2Plus1D(depth=18), **configs/benchmark/kinetics/8x224x224-linear.yaml model args)",
                   "args": SHIPPED, "state_dict": keys}, f, indent=0)
        f.write("\n")
    print(f"{len(keys)} keys -> most_model_keys.json")

    g = torch.Generator().manual_seed(20)
    taps = {n: (torch.randn(shape, generator=g) * 1.5 + 0.3) for n, (shape, _, _) in HEADS.items()}

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.scale = torch.nn.Parameter(torch.ones(1))

        def forward(self, x, return_embs=False):
            return {n: t.to(x.dtype) for n, t in taps.items()}

    torch.manual_seed(21)
    m = mod.MOSTModel(Stub(), N_CLASSES, list(HEADS), [f for _, _, f in HEADS.values()], [p for _, p, _ in HEADS.values()],
                      use_bn=True)
    for c in m.classifiers:
        with torch.no_grad():
            c.bn.weight.copy_(torch.rand(c.bn.weight.shape, generator=g) + 0.5)
            c.bn.bias.copy_(torch.randn(c.bn.bias.shape, generator=g) * 0.2)
    out = {"labels": torch.randint(0, N_CLASSES, (4,), generator=g).numpy()}
    for n, t in taps.items():
        out[f"tap.{n}"] = t.numpy()
    for k, v in m.classifiers.state_dict().items():
        out[f"init.{k}"] = v.clone().numpy()          # (a copy: the forward below bumps num_batches_tracked in place)
    m = m.double().train()
    logits = m(torch.zeros(4, 3, 1, 1, 1, dtype=torch.float64))
    labels = torch.from_numpy(out["labels"])
    loss = sum(torch.nn.functional.cross_entropy(logits[n], labels) for n in HEADS)
    loss.backward()
    out["loss"] = loss.detach().numpy()
    for n in HEADS:
        out[f"logits.{n}"] = logits[n].detach().numpy()
    for k, p in m.classifiers.named_parameters():
        out[f"grad.{k}"] = p.grad.numpy()
    for k, v in m.classifiers.state_dict().items():
        if "running" in k or "num_batches" in k:
            out[f"after.{k}"] = v.numpy()
    assert all(p.grad is None for p in m.feature_extractor.parameters())
    path = os.path.join(args.out, "most_heads.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out)} arrays, {os.path.getsize(path)} bytes -> most_heads.npz")


if __name__ == "__main__":
    main()
