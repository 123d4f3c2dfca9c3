#!/usr/bin/env python
"""Generate tests/golden/cls_wrapper_keys.json by IMPORTING the reference (runs only in the build container):

    python tools/make_cls_golden.py [--ref /root/reference] [--out tests/golden/cls_wrapper_keys.json]

The reference's ``ClassificationWrapper`` (utils/eval_utils.py) around its ``R2Plus1D`` depth 18 with 101 classes, as the
benchmark configs build it (feat_name "pool", feat_dim 512, use_dropout, dropout 0.5): its state-dict keys and shapes, in
order.  Only that list is stored."""
import argparse
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "cls_wrapper_keys.json"))
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    import importlib.util
    import torch  # noqa: F401
    from models.video import R2Plus1D  # reference
    # eval_utils.py imports the reference's data pipeline at module level; only the wrapper class is needed here
    for name in ("datasets", "utils.videotransforms", "utils.videotransforms.video_transforms",
                 "utils.videotransforms.volume_transforms", "utils.videotransforms.tensor_transforms"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("ref_eval_utils", os.path.join(args.ref, "utils", "eval_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = mod.ClassificationWrapper(R2Plus1D(depth=18), n_classes=101, feat_name="pool", feat_dim=512, pooling_op=None,
                                  use_dropout=True, dropout=0.5)
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(args.out, "w") as f:
        json.dump({"model": "ClassificationWrapper(R2Plus1D(depth=18), n_classes=101, feat_name='pool', feat_dim=512, "
                            "pooling_op=None, use_dropout=True, dropout=0.5)", "state_dict": keys}, f, indent=0)
        f.write("\n")
    print(f"{len(keys)} keys -> {args.out}")


if __name__ == "__main__":
    main()
