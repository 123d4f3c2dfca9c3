"""Helper of tests/test_gpu_inference.py: ``FinetuneStep.evaluate`` / ``ProbeStep.evaluate`` (argument ``probe``) on a fixed small
problem, one JSON line with digests of the results and the path the chunks took.  Run in-process (programs on) and in a fresh process under ``AVID_EVAL_PLAN=0`` (the switch
is read once at import)."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "avid-cma_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402


def wrapper(dev, seed=0):
    import models
    torch.manual_seed(seed)
    m = models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5)
    with torch.no_grad():           # non-trivial BatchNorm affines and running statistics
        for n, p in m.named_parameters():
            if p.dim() == 1 and "bn" in n:
                p.add_(0.1 * torch.randn_like(p))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.mul_(1.0 + 0.3 * torch.rand_like(b))
    return m.to(dev).train()


def evaluate_digest(dev):
    """V x clips = 3 x 3 clips of 3x8x48x48 in chunks of 4: two chunk sizes (4 and 1), two plans."""
    from avid_hip import ops, parallel, plan
    ops.tconv_configure(2)
    try:
        m = wrapper(dev)
        eng = parallel.FinetuneStep(m)
        g = torch.Generator().manual_seed(7)
        video = torch.randn((3, 3, 3, 8, 48, 48), generator=g).to(dev)
        labels = torch.randint(0, 101, (3,), generator=g).to(dev)
        conf, loss, hits = eng.evaluate(video, labels, batch=4)
        torch.cuda.synchronize()
        n_plans = sum(1 for k, v in m.__dict__.get("_avid_plans", {}).items() if k[0] == "eval" and v)
    finally:
        ops.tconv_configure(-1)
    sha = hashlib.sha256(conf.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes() + hits.cpu().numpy().tobytes()).hexdigest()
    return {"sha": sha, "eval_plans": n_plans, "enabled": bool(plan.EVAL_ENABLED), "training": bool(m.training)}, (m, video, labels, conf, loss, hits)


SHIPPED = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
               pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                            "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)


def most_model(dev, seed=0):
    """The stock linear probe (shipped heads) with non-trivial running statistics in the tower and the heads."""
    import models
    torch.manual_seed(seed)
    m = models.MOSTModel(models.R2Plus1D(18), **SHIPPED)
    with torch.no_grad():
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.add_(0.1 * torch.randn_like(b))
            elif n.endswith("running_var"):
                b.mul_(1.0 + 0.3 * torch.rand_like(b))
    return m.to(dev).train()


def probe_digest(dev):
    """V x clips = 3 x 3 clips of 3x8x64x64 in chunks of 4 through ``ProbeStep.evaluate``: chunk sizes 4 and 1, two plans."""
    from avid_hip import parallel, plan
    m = most_model(dev)
    eng = parallel.ProbeStep(m)
    g = torch.Generator().manual_seed(8)
    video = torch.randn((3, 3, 3, 8, 64, 64), generator=g).to(dev)
    labels = torch.randint(0, 400, (3,), generator=g).to(dev)
    conf, loss, hits = eng.evaluate(video, labels, batch=4)
    torch.cuda.synchronize()
    n_plans = sum(1 for k, v in m.__dict__.get("_avid_plans", {}).items() if k[0] == "eval" and v)
    sha = hashlib.sha256(conf.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes() + hits.cpu().numpy().tobytes()).hexdigest()
    return {"sha": sha, "eval_plans": n_plans, "enabled": bool(plan.EVAL_ENABLED), "training": bool(m.training)}, (m, video, labels, conf, loss, hits)


def golden_av_wrapper(dev):
    """``AV_Wrapper`` with the deterministic parameters tests/golden/av_wrapper.npz was generated from (tag "w")."""
    import numpy as np
    import models
    from oracle import detgen
    m = models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128])
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(detgen.det_param(f"w:{k}", tuple(v.shape)))).to(v.dtype)
                       for k, v in m.state_dict().items()})
    return m.to(dev)


if __name__ == "__main__":
    fn = probe_digest if sys.argv[1:] == ["probe"] else evaluate_digest
    print("PROBE " + json.dumps(fn(torch.device("cuda:0"))[0]), flush=True)
