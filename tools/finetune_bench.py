#!/usr/bin/env python
"""Fine-tuning throughput on one GPU (not bench.py: the flagship workload stays the pretraining step).  One JSON line:

    python tools/finetune_bench.py [--steps 10] [--warmup 3] [--virtual-ranks R] [--batch-scale K]

Per-GPU shapes are the shipped benchmark configs (configs/benchmark/{ucf,hmdb51}/*.yaml) split over 8 GPUs: 8 x 3x8x224^2
(``8at16``, global batch 64) and 4 x 3x32x224^2 (``32at16``, global batch 32), R(2+1)D-18 + dropout 0.5 + Linear(512, 101).
For each shape, clips/s and ms/step of
  (a) ``FinetuneStep``                       the compiled programs + flat Adam
  (b) ``FinetuneStep(classifier_only=True)`` the warm-up epochs
  (c) the path the reference's script took before: this package's R2Plus1D with ``return_embs=True`` (the per-layer path),
      torch ``Dropout``, ``Linear``, ``cross_entropy`` and ``torch.optim.Adam``
  (d) ``FinetuneStep.evaluate`` at 10 clips per video
plus ``mcycles_per_step`` (ms per step x the mean shader clock during the timed steps, bench.py's definition) and the
kernels that served the 32-frame step (launch log of one timed step).

``--virtual-ranks R`` (default 1): (a) and (b) run ``FinetuneStep(virtual_ranks=R)`` on the GLOBAL batch of R per-GPU batches —
R = 8 is the shipped eight-replica job on one GPU; (c) and (d) take that batch whole.  ``--batch-scale K`` (default 1): every
per-GPU batch times K (K = 8, R = 1: the shipped global batch as ONE whole-batch step, what the virtual step is compared with).
With the defaults the output is what it was; otherwise it also says ``virtual_ranks`` and ``batch_scale``."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class _TorchHead(torch.nn.Module):
    """(c): the reference's ClassificationWrapper as it ran here before — its forward restated over this package's tower."""

    def __init__(self, fe, n_classes):
        super().__init__()
        self.feature_extractor = fe
        self.dropout = torch.nn.Dropout(0.5)
        self.classifier = torch.nn.Linear(512, n_classes)

    def forward(self, x):
        emb = self.feature_extractor(x, return_embs=True)["pool"]
        return self.classifier(self.dropout(emb.reshape(x.shape[0], -1)))


def _time(fn, steps, warmup, sampler_cls, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    sampler = sampler_cls(dev.index or 0)
    sampler.start()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    ghz = sampler.stop()
    return ms, ghz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", type=int, default=101)
    ap.add_argument("--virtual-ranks", type=int, default=1)
    ap.add_argument("--batch-scale", type=int, default=1)
    args = ap.parse_args()
    R, K = args.virtual_ranks, args.batch_scale
    import models
    from avid_hip import lib, parallel
    from bench import ClockSampler
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = {"metric": "fine-tuning clips/s (R(2+1)D-18 + dropout + linear, 1 GPU)", "unit": "clips/s", "shapes": {}}
    for name, shape in (("8at16", (8, 3, 8, 224, 224)), ("32at16", (4, 3, 32, 224, 224))):
        shape = (shape[0] * K * R,) + shape[1:]
        B = shape[0]
        g = torch.Generator().manual_seed(0)
        video = torch.randn(shape, generator=g).to(dev)
        labels = torch.randint(0, args.classes, (B,), generator=g).to(dev)
        res = {}

        def wrapper():
            torch.manual_seed(0)
            return models.ClassificationWrapper(models.R2Plus1D(18), args.classes, "pool", 512, use_dropout=True,
                                                dropout=0.5).to(dev).train()
        for tag, co in (("a_finetune_step", False), ("b_classifier_only", True)):
            eng = parallel.FinetuneStep(wrapper(), classifier_only=co, **({"virtual_ranks": R} if R != 1 else {}))
            ms, ghz = _time(lambda: eng.step(video, labels), args.steps, args.warmup, ClockSampler, dev)
            res[tag] = {"ms_per_step": round(ms, 3), "clips_per_s": round(B / ms * 1e3, 2),
                        "mcycles_per_step": None if ghz is None else round(ms * ghz, 2)}
            if tag == "a_finetune_step":
                vid_eval = torch.randn((B, 10) + shape[1:], generator=g).to(dev) if B * 10 * shape[2] <= 80 * 8 else \
                    torch.randn((1, 10) + shape[1:], generator=g).to(dev)
                lab_eval = torch.randint(0, args.classes, (vid_eval.shape[0],), generator=g).to(dev)
                ms_e, ghz_e = _time(lambda: eng.evaluate(vid_eval, lab_eval, B), max(2, args.steps // 3), 1, ClockSampler, dev)
                n_clips = vid_eval.shape[0] * 10
                res["d_evaluate_10clips"] = {"videos": vid_eval.shape[0], "batch": B, "ms_per_call": round(ms_e, 3),
                                             "clips_per_s": round(n_clips / ms_e * 1e3, 2),
                                             "mcycles_per_call": None if ghz_e is None else round(ms_e * ghz_e, 2)}
                if name == "32at16":            # which kernels served the 32-frame step (one step, launch log on)
                    lib.timing_enable(True)
                    eng.step(video, labels)
                    torch.cuda.synchronize()
                    rep = lib.timing_report()
                    lib.timing_enable(False)
                    res["kernels_t32"] = {k: v["launches"] for k, v in sorted(rep.items())}
            del eng
        torch.manual_seed(0)
        ref = _TorchHead(models.R2Plus1D(18), args.classes).to(dev).train()
        opt = torch.optim.Adam(ref.parameters(), lr=1e-4, weight_decay=0.0)

        def torch_step():
            loss = F.cross_entropy(ref(video), labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
        ms, ghz = _time(torch_step, args.steps, args.warmup, ClockSampler, dev)
        res["c_per_layer_torch_head"] = {"ms_per_step": round(ms, 3), "clips_per_s": round(B / ms * 1e3, 2),
                                         "mcycles_per_step": None if ghz is None else round(ms * ghz, 2)}
        res["a_over_c"] = round(res["c_per_layer_torch_head"]["ms_per_step"] / res["a_finetune_step"]["ms_per_step"], 3)
        del ref, opt
        torch.cuda.empty_cache()
        out["shapes"][name] = {"per_gpu_batch": B // R, "clip": list(shape[1:]), **res}
    if (R, K) != (1, 1):
        out["virtual_ranks"], out["batch_scale"] = R, K
    print(json.dumps(out))


if __name__ == "__main__":
    main()
