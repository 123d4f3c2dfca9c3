"""The recorded bits of the fused criterion: tests/golden/crit_fused_bits.npz.

The fixture is the anchor of the three fused criterion entry points' arithmetic (``ops.xmodal_fused``, ``ops.cma_fused``,
``ops.crit_fused``): the normalisation, every score, the exp / log / divide chains, the fold over groups, waves, blocks and samples,
the finish kernel's scale and the re-armed ticket.  It is recorded ONCE, from the library of the commit named in its metadata
(built outside the tree and selected with AVID_HIP_LIB), and replayed bit for bit by tests/test_gpu_crit_bits.py: a mismatch is a
change of behaviour, never a reason to record again.

    AVID_HIP_LIB=<that library> python tools/record_crit_bits.py --commit <hash of the commit whose library runs> [--out FILE]

The importable half names the cases and runs one (``cases()``, ``make_inputs()``, ``input_hash()``, ``run_case()``); the test uses
the same ``run_case``.  The inputs come from the seeded generators of tests/_fused_ref.py and tests/_crit_ref.py and are not stored
(no banks in the file): per case the file holds the sha256 of their concatenated bytes, which the test asserts first.

Layout of the file: per case ``<name>/sha256`` uint8 [32] and the int32 bits of ``<name>/total`` [1], ``<name>/losses`` [4 | 8 | 16]
(``cma_fused`` never writes its eighth word, "(unused)" in include/avid_hip.h: stored as 0, not compared),
``<name>/hats`` [2, bs, 128], ``<name>/dv`` / ``<name>/da`` [bs, 128] — the embeddings' ``.grad`` after ``(total * 2.0).backward()``.
Every case is called twice on one workspace and the SECOND call is recorded: the re-armed ticket is part of what is pinned.
``ws_queries`` int64 [n, 6]: (bs, P, K) of every case and the answers of the three workspace-size queries for it; ``meta`` — JSON."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "crit_fused_bits.npz")
for _p in (REPO, os.path.join(REPO, "avid-cma_amd"), os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _crit_ref as R  # noqa: E402
import _fused_ref as FR  # noqa: E402

# bs, K, N: K = 1; one block exactly (with the extra unit); a one-row last block; two and three blocks; the benchmark's K (16 blocks)
XMODAL_SHAPES = ((2, 1, 200), (3, 63, 300), (3, 64, 300), (3, 65, 300), (3, 70, 300), (3, 129, 300), (6, 1024, 5000))
# bs, P, K, Kw, N: CMA_SHAPES of tests/test_gpu_crit_fused.py — 1 + P + K = 64 and 65, Kw = 1, Kw = K, Kw inside the first block
CMA_SHAPES = ((3, 5, 70, 70, 300), (4, 1, 33, 7, 200), (2, 3, 60, 1, 200), (2, 3, 61, 61, 200), (6, 32, 1024, 64, 5000))
CRIT_AVID = (R.AVID_MASKS + (R.X_INST,), ((3, 0, 65, 65, 300),))
CRIT_CMA = (R.CMA_MASKS + (R.X_INST | R.W_POS,), ((4, 1, 33, 7, 200), (2, 3, 61, 61, 200)))
ARRAYS = ("total", "losses", "hats", "dv", "da")
# the words of ``losses`` an entry point writes: losses[7] of ``cma_fused`` is "(unused)" (include/avid_hip.h) and holds whatever
# torch.empty found — the file's eighth word of a cma case is such a leftover and is not compared
WRITTEN = {"xmodal": 4, "cma": 7, "crit": 16}


def cases():
    """Every case as a dict: ``name``, ``op`` (xmodal / cma / crit), ``shape`` (the generator's arguments), ``mask`` (crit)."""
    out = [dict(name="xmodal-" + "x".join(map(str, s)), op="xmodal", shape=s) for s in XMODAL_SHAPES]
    out += [dict(name="cma-" + "x".join(map(str, s)), op="cma", shape=s) for s in CMA_SHAPES]
    for masks, shapes in (CRIT_AVID, CRIT_CMA):
        out += [dict(name=f"crit-m{m}-" + "x".join(map(str, s)), op="crit", shape=s, mask=m) for s in shapes for m in masks]
    return out


def bs_p_k(case):
    s = case["shape"]
    return (s[0], 0, s[1]) if case["op"] == "xmodal" else (s[0], s[1], s[2])


def make_inputs(case):
    if case["op"] == "xmodal":
        return FR.xmodal_case(*case["shape"])
    if case["op"] == "cma":
        return FR.cma_case(*case["shape"])
    return R.crit_case(case["mask"], *case["shape"])


def input_hash(c):
    """sha256 over the bytes of ve, ae, y, pos (if any), idx, the two banks and Z, in that order."""
    h = hashlib.sha256()
    for t in (c.ve, c.ae, c.y, getattr(c, "pos", None), c.idx, c.v1, c.v2, c.Z):
        if t is not None:
            h.update(t.contiguous().numpy().tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def run_case(case, c, dev):
    """The case's entry point twice on one workspace -> {array name: int32 bits} of the second call."""
    import torch
    from avid_hip import ops
    vd, ad = c.ve.to(dev).requires_grad_(True), c.ae.to(dev).requires_grad_(True)
    y, idx, b1, b2, Z = c.y.to(dev), c.idx.to(dev), c.v1.to(dev), c.v2.to(dev), c.Z.to(dev)
    bs, P, K = bs_p_k(case)
    if case["op"] == "xmodal":
        ws = ops.xmodal_fused_workspace(dev, bs, K)
        call = lambda: ops.xmodal_fused(vd, ad, y, idx, b1, b2, Z, 1 / c.T, c.coeff, ws)                        # noqa: E731
    elif case["op"] == "cma":
        ws, pos = ops.cma_fused_workspace(dev, bs, P, K), c.pos.to(dev)
        call = lambda: ops.cma_fused(vd, ad, y, pos, idx, b1, b2, Z, 1 / c.T, case["shape"][3], c.cI, c.cP, ws)  # noqa: E731
    else:
        ws, pos = ops.crit_fused_workspace(dev, bs, P, K), None if c.pos is None else c.pos.to(dev)
        call = lambda: ops.crit_fused(vd, ad, y, pos, idx, b1, b2, Z, 1 / c.T, case["shape"][3], case["mask"], R.COEFFS, ws)  # noqa: E731
    call()
    total, losses, hats = call()
    (total * 2.0).backward()
    torch.cuda.synchronize()
    ops.check_device_errors(dev)
    got = dict(total=total.detach().reshape(1), losses=losses[:WRITTEN[case["op"]]], hats=hats, dv=vd.grad, da=ad.grad)
    return {k: v.detach().contiguous().view(torch.int32).cpu().numpy() for k, v in got.items()}


def ws_queries():
    """int64 [n, 6]: the distinct (bs, P, K) of the cases with the answers of avid_xmodal_fused_workspace_bytes(bs, K),
    avid_cma_fused_workspace_bytes(bs, P, K) and avid_crit_fused_workspace_bytes(bs, P, K).  Needs the library, not a GPU."""
    from avid_hip import lib
    rows = []
    for bs, P, K in sorted({bs_p_k(c) for c in cases()}):
        rows.append((bs, P, K, lib.raw("avid_xmodal_fused_workspace_bytes")(bs, K), lib.raw("avid_cma_fused_workspace_bytes")(bs, P, K),
                     lib.raw("avid_crit_fused_workspace_bytes")(bs, P, K)))
    return np.asarray(rows, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded: goes into the metadata")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the bits are the GPU's: there is nothing to record without one"
    dev = torch.device("cuda:0")
    arrays = {}
    for case in cases():
        c = make_inputs(case)
        arrays[case["name"] + "/sha256"] = input_hash(c)
        got = run_case(case, c, dev)
        for k in ARRAYS:
            assert np.isfinite(got[k].view(np.float32)).all(), (case["name"], k)
            arrays[case["name"] + "/" + k] = got[k]
        if case["op"] == "cma":                       # the file keeps the entry point's length; the unused word as 0
            arrays[case["name"] + "/losses"] = np.concatenate([got["losses"], np.zeros(1, np.int32)])
        print(case["name"], "ok", flush=True)
    arrays["ws_queries"] = ws_queries()
    meta = dict(commit=a.commit, device=torch.cuda.get_device_name(0), cases=[c["name"] for c in cases()],
                note="recorded once from the library of `commit`, second call on one workspace; replayed by tests/test_gpu_crit_bits.py")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    size = os.path.getsize(a.out)
    assert size <= 512 * 1000, f"{a.out}: {size} bytes"
    print(f"wrote {a.out}: {size} bytes, {len(cases())} cases", flush=True)


if __name__ == "__main__":
    main()
