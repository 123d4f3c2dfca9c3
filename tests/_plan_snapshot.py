"""What the launch-program compiler (avid_hip/plan.py) emits for a fixed matrix of plans, reduced to a JSON-able snapshot:
shared by tools/plan_snapshot.py (writes tests/golden/plan_programs.json) and tests/test_plan_snapshot.py (compares).

Everything is compiled with ``torch.device("cpu")``: no GPU, no kernel runs.  A record holds geometry, integers and
``(slot, offset)`` references only — no address — so its bytes are the same in every process."""
import functools
import json
import os
import struct
import zlib

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "plan_programs.json")
CPU = torch.device("cpu")

PROBE = dict(n_classes=400, feat_names=["conv2x", "conv3x", "conv4x", "conv5x"], feat_dims=[9216, 8192, 9216, 8192],
             pooling_ops=["AdaptiveMaxPool3d((1,12,12))", "AdaptiveMaxPool3d((1,8,8))", "AdaptiveMaxPool3d((1,6,6))",
                          "AdaptiveMaxPool3d((1,4,4))"], use_bn=True)          # tests/test_probe_host.py: SHIPPED
CLIPS = {"8x8x224": (8, 3, 8, 224, 224), "4x32x224": (4, 3, 32, 224, 224), "2x8x64": (2, 3, 8, 64, 64)}
TOWERS = {"b4": ((4, 3, 8, 112, 112), (4, 1, 40, 100)), "b64": ((64, 3, 8, 112, 112), (64, 1, 40, 100)),
          "b2x64": ((2, 3, 8, 64, 64), (2, 1, 40, 100))}
STREAMS = {"o1t1g1": (True, True, True), "o0t0g0": (False, False, False), "o0t1g0": (False, True, False)}


@functools.lru_cache(maxsize=None)
def _model(kind):
    import models
    torch.manual_seed(0)
    if kind == "av":
        return models.av_wrapper("R2Plus1D", {"depth": 18}, "Conv2D", {"depth": 10}, proj_dim=[512, 512, 128]).train()
    if kind == "tower":
        return models.R2Plus1D(18)
    if kind == "cls":
        return models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=True, dropout=0.5).train()
    if kind == "cls_nodrop":
        return models.ClassificationWrapper(models.R2Plus1D(18), 101, "pool", 512, use_dropout=False).train()
    if kind == "most":
        return models.MOSTModel(models.R2Plus1D(18), **PROBE).train()
    raise KeyError(kind)


def _matrix():
    from avid_hip import plan
    mx = {}
    for tn, (vs, as_) in TOWERS.items():
        for sn, otg in STREAMS.items():
            mx[f"plan/{tn}/{sn}"] = lambda vs=vs, as_=as_, otg=otg: plan.Plan(_model("av"), vs, as_, CPU, *otg)
        if tn != "b2x64":
            mx[f"eval/av/{tn}"] = lambda vs=vs, as_=as_: plan.EvalPlan(_model("av"), vs, as_, CPU)
    for cn, s in CLIPS.items():
        mx[f"cls/{cn}/full"] = lambda s=s: plan.ClsPlan(_model("cls"), s, CPU, True, True, False)
        mx[f"cls/{cn}/classifier_only"] = lambda s=s: plan.ClsPlan(_model("cls"), s, CPU, True, True, True)
        for kind in ("tower", "cls", "most"):
            mx[f"eval/{kind}/{cn}"] = lambda kind=kind, s=s: plan.EvalPlan(_model(kind), s, None, CPU)
    mx["cls/2x8x64/nodrop_t0g0"] = lambda: plan.ClsPlan(_model("cls_nodrop"), CLIPS["2x8x64"], CPU, False, False, False)
    mx["probe/128x8x224"] = lambda: plan.ProbePlan(_model("most"), (128, 3, 8, 224, 224), CPU, True, True)
    mx["probe/4x8x64"] = lambda: plan.ProbePlan(_model("most"), (4, 3, 8, 64, 64), CPU, True, True)
    return mx


def names():
    return sorted(_matrix())


def compile_plan(name):
    return _matrix()[name]()


def programs(pl):
    """[(program name, record array, number of records)] of a compiled plan."""
    out = [("fwd", pl.fwd_prog, pl.n_fwd)]
    if getattr(pl, "bwd_prog", None) is not None:
        out.append(("bwd", pl.bwd_prog, pl.n_bwd))
    return out


def _digest(obj):
    return zlib.crc32(json.dumps(obj, sort_keys=True).encode())


def entry(pl):
    e = {"programs": {n: [zlib.crc32(bytes(prog[k])) for k in range(cnt)] for n, prog, cnt in programs(pl)},
         "fa_bytes": pl.fa_bytes, "ba_bytes": getattr(pl, "ba_bytes", None), "aux_bytes": pl.aux_bytes,
         "ws_bytes": list(pl.ws_bytes), "table_off": pl.table_off, "n_slots": pl.n_slots,
         "wt_recs": [[off, cout, taps, cin, mode] for _, off, cout, taps, cin, mode in pl.wt_recs]}
    if getattr(pl, "bwd_prog", None) is not None:
        e.update(gnumel=pl.gnumel, goff=zlib.crc32(struct.pack(f"<{len(pl.goff)}q", *pl.goff)),
                 grad_ready=_digest([[end, stream, list(ps)] for end, stream, ps in pl.grad_ready]),
                 adam_early=pl.adam_early, n_logits=getattr(pl, "n_logits", None), zero_index=pl._zero_index)
    else:
        e.update(virtual_bytes=pl.virtual_bytes, out_bytes=pl.out_bytes,
                 outputs=[[off, list(shape)] for off, shape in pl.outputs], out_names=getattr(pl, "out_names", None),
                 bn_recs=[off for _, off in pl.bn_recs], bn_table_off=pl.bn_table_off,
                 buffers=_digest([list(b) for b in pl.buffers]))
    return json.loads(json.dumps(e))                     # (as it reads back from the file: lists, no tuples)


def snapshot():
    return {name: entry(compile_plan(name)) for name in names()}


def write(snap, path=GOLDEN):
    """One plan per line, so that a regenerated file shows which plans moved."""
    with open(path, "w") as f:
        f.write("{\n")
        f.write(",\n".join(f"{json.dumps(n)}: {json.dumps(snap[n], sort_keys=True, separators=(',', ':'))}" for n in sorted(snap)))
        f.write("\n}\n")


def load(path=GOLDEN):
    with open(path) as f:
        return json.load(f)
