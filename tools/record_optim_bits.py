"""The recorded bits of the flat optimizers: tests/golden/optim_flat_bits.npz.

The fixture is the anchor of the flat Adam / SGD kernels' arithmetic: every fused multiply-add, every separately rounded
product, the vector loop and the n % 4 tail, the four ways the step and the learning rate reach the kernel.  It is recorded ONCE,
from the library of the commit named in its metadata, and replayed bit for bit by tests/test_gpu_optim_bits.py: a mismatch is a
change of behaviour, never a reason to record again.

    python tools/record_optim_bits.py --commit <hash of the commit whose library runs> [--out FILE]

The importable half builds the cases and their inputs and runs one case (``cases()``, ``make_inputs()``, ``run_case()``); the
test uses the same ``run_case`` on the inputs the file holds.

Layout of the file: ``inputs`` int32 [6, 1042] — the fp32 bits of p, g, m, v, buf, e for the sizes 3, 8, 1031 one behind the
other; ``out/<case>`` int32 [buffers, 1042] — the case's buffers (``BUFFERS`` order) after three consecutive steps; ``aux/<case>``
int64 — per size the device step counter, the device counter of averaging updates, the bits of the clip coefficient (-1: the
case has none), for the table kernels the bits of the three trust factors behind them; ``meta`` — JSON.  Every size runs once at
the start of an allocation and once 16 bytes into one; the recorder refuses to write unless the two agree, so one copy is kept.
A skipped step changes nothing: its case holds no ``out`` array, the expectation is the inputs."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "optim_flat_bits.npz")

SIZES = (3, 8, 1031)        # the tail alone (n4 = 0); vectors alone; 257 vectors = two workgroups, and a tail of block 0's
COLS = sum(SIZES)
ROWS = ("p", "g", "m", "v", "buf", "e")
LEAD, PAD = 4, 8            # floats in front of a slice placed 16 bytes into its allocation; pattern floats behind every slice
STEPS = 3
MODES = ("value", "step_dev", "lr_dev", "lr_dev+step_dev")
ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)
SGD_LR, DECAY, GRAD_SCALE, CLIP_AT = 1e-3, 0.999, 1.0 / 3.0, 0.37
# three segments of the sizes above in one buffer, each on a 16-byte boundary; elements 3 and 1043 belong to nobody
TABLE = dict(layout=[(0, 3), (4, 8), (12, 1031)], numel=1044, lr_scale=[1.0, 0.5, 2.0], weight_decay=[0.0, 1e-5, 1e-4],
             adapt=[True, False, True], trust_coefficient=0.02)
SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-41, 1e18, -2e18, 3e-18, -1e-18], np.float32)   # +-0, denormals, around 1e+-18


def cases():
    """Every case as a dict: ``name``, ``kind`` (adam / sgd / adam_table / sgd_table / lamb), ``guard`` (None, "one": clip
    coefficient 1, "clip", "skip"), ``ema``, ``mode`` (how the step and the learning rate arrive), ``wd``, ``momentum``,
    ``nesterov``, ``mild`` (the inputs without their largest magnitudes, see ``mild()``)."""
    out = []

    def adam(label, guard, ema, mode, wd):
        out.append(dict(name=f"adam-{label}-{mode}-wd{wd:g}", kind="adam", guard=guard, ema=ema, mode=mode, wd=wd))
    for label, guard, ema in (("plain", None, False), ("ema_clip", "clip", True)):     # all four modes
        for mode in MODES:
            adam(label, guard, ema, mode, 1e-5)
        adam(label, guard, ema, "step_dev", 0.0)
    for label, guard, ema in (("one", "one", False), ("clip", "clip", False), ("ema", None, True)):
        for wd in (0.0, 1e-5):
            adam(label, guard, ema, "step_dev", wd)
    adam("skip", "skip", False, "step_dev", 1e-5)
    for label, guard, ema in (("plain", None, False), ("clip", "clip", False), ("ema_clip", "clip", True)):
        for momentum, nesterov in ((0.0, False), (0.9, False), (0.9, True)):
            for wd in (0.0, 1e-4):
                out.append(dict(name=f"sgd-{label}-m{momentum:g}{'n' if nesterov else ''}-wd{wd:g}", kind="sgd", guard=guard, ema=ema,
                                mode="lr_dev" if ema else "value", wd=wd, momentum=momentum, nesterov=nesterov))
    for kind in ("adam_table", "sgd_table", "lamb"):
        out.append(dict(name=kind, kind=kind, guard="clip", ema=True, mode="lr_dev" if kind == "sgd_table" else "step_dev",
                        wd=None, momentum=0.9, nesterov=True))
    # LAMB once more without the magnitudes around 1e18 and the v near 0 (two of the three trust factors are about 1e-8, p stands still)
    out.append(dict(name="lamb-mild", kind="lamb", guard="clip", ema=True, mode="step_dev", wd=None, momentum=0.9, nesterov=True,
                    mild=True))
    return out


def buffers(case):
    """The names of the buffers a case updates, in the order of its ``out`` rows."""
    if case["kind"] in ("sgd", "sgd_table"):
        names = ["p"] + (["buf"] if case["momentum"] else [])
    else:
        names = ["p", "m", "v"]
    return names + (["e"] if case["ema"] else [])


def make_inputs():
    """float32 [6, 1042]: finite values only.  The first sixteen elements of every size are dense in special values (so that the
    sizes 3 and 8 meet them), one in thirteen behind; v >= 0 with exact zeros; one element with g == m == v == 0."""
    rng = np.random.default_rng(20261021)
    scale = dict(p=1.0, g=0.3, m=0.05, v=0.01, buf=0.1, e=1.0)
    x = np.empty((len(ROWS), COLS), np.float32)
    col = 0
    for n in SIZES:
        for k, name in enumerate(ROWS):
            a = (scale[name] * rng.standard_normal(n)).astype(np.float32)
            for i in range(n):
                if i < 16 and i % 2 == 0:
                    a[i] = SPECIALS[(i + 3 * k) % 8]
                elif i >= 16 and i % 13 == k:
                    a[i] = SPECIALS[(i // 13) % 8]
            if name == "v":
                a = np.abs(a)
            x[k, col:col + n] = a
        if n >= 8:
            x[1:4, col + 1] = 0.0          # sqrt(0) + eps with nothing to add
        col += n
    assert np.isfinite(x).all() and (x[3] >= 0).all()
    return x


def split(row):
    """One row of ``inputs`` / ``out`` -> {n: its columns}."""
    out, col = {}, 0
    for n in SIZES:
        out[n] = row[col:col + n]
        col += n
    return out


def mild(x, floor=0.0):
    """``x`` with every magnitude from 1e17 up replaced by 0.75 of its sign, and nothing below ``floor`` (given for v alone:
    an element with v near 0 and m not has an update of 1e6 and more, which alone makes the trust factor tiny): what a
    ``mild`` case runs on."""
    x = np.where(np.abs(x) >= 1e17, np.copysign(np.float32(0.75), x), x).astype(np.float32)
    return np.maximum(x, np.float32(floor)) if floor else x


def moved(case, inputs, out):
    """The fraction of the elements of p whose bits a case changed."""
    p = inputs[ROWS.index("p")]
    return float(np.mean(out[0] != (mild(p) if case.get("mild") else p).view(np.int32)))


def max_norm_for(g):
    """A clipping threshold below the norm of the scaled gradient, so that the coefficient is about CLIP_AT (no power of two)."""
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) * GRAD_SCALE
    return float(np.float32(CLIP_AT * norm))


def _pattern(count):
    return (1.5 + 0.25 * np.arange(count)).astype(np.float32)


class _Placed:
    """Values inside an allocation whose other floats hold a pattern: ``t`` is the slice the kernels get."""

    def __init__(self, values, placement, dev, holes=()):
        import torch
        lead = LEAD * placement
        host = _pattern(lead + len(values) + PAD)
        self.keep = np.ones(len(host), bool)                 # the floats nobody may write
        self.keep[lead:lead + len(values)] = False
        for i in holes:
            self.keep[lead + i] = True
        host[~self.keep] = np.asarray(values)[~self.keep[lead:lead + len(values)]]
        self.before = host.view(np.int32).copy()
        self.alloc = torch.from_numpy(host).to(dev)
        self.t = self.alloc[lead:lead + len(values)]

    def surroundings_untouched(self):
        now = self.alloc.cpu().numpy().view(np.int32)
        return bool(np.array_equal(now[self.keep], self.before[self.keep]))

    def bits(self):
        return self.t.cpu().numpy().view(np.int32).copy()


def _run(case, vals, placement, dev, table_spec=None):
    """One set of buffers through STEPS steps of ``case``.  vals: {name: fp32 array}.  -> ({name: int32 bits}, aux list)."""
    import torch
    from avid_hip import ops
    holes = ()
    if table_spec:
        covered = np.zeros(table_spec["numel"], bool)
        for o, n in table_spec["layout"]:
            covered[o:o + n] = True
        holes = tuple(np.flatnonzero(~covered))
    names = buffers(case)
    B = {k: _Placed(vals[k], placement, dev, holes) for k in names}
    G = _Placed(vals["g"], placement, dev)
    g = G.t
    t = {k: b.t for k, b in B.items()}
    kind, mode, wd = case["kind"], case["mode"], case["wd"]
    adamish = kind in ("adam", "adam_table", "lamb")
    lr = ADAM["lr"] if adamish else SGD_LR
    step_dev = torch.zeros((), dtype=torch.int64, device=dev) if "step_dev" in mode else None
    lr_dev = torch.tensor(lr, dtype=torch.float32, device=dev) if "lr_dev" in mode else None
    lr_host = lr if lr_dev is None else 1.0                       # with lr_dev the host's value must not matter
    guard = ops.StepGuard(dev) if case["guard"] else None
    updates = torch.zeros((), dtype=torch.int64, device=dev) if (case["ema"] and case["guard"]) else None
    ema_kw = dict(decay=DECAY, warmup=updates is not None, updates_dev=updates) if case["ema"] else {}
    table = None
    if table_spec:
        table = ops.SegmentTable(table_spec["layout"], lr_scale=table_spec["lr_scale"], weight_decay=table_spec["weight_decay"],
                                 adapt=table_spec["adapt"], device=dev, numel=table_spec["numel"])
    for k in range(1, STEPS + 1):
        if case["guard"] == "skip":
            guard.record.zero_()
            guard.record[2] = 1
            guard.clip_coef.fill_(1.0)
        elif guard is not None:
            ops.grad_guard(g, guard, GRAD_SCALE, max_norm_for(vals["g"]) if case["guard"] == "clip" else 0.0, True)
        a = (lr_host, ADAM["b1"], ADAM["b2"], ADAM["eps"])
        skw = dict(grad_scale=GRAD_SCALE, step_dev=step_dev, lr_dev=lr_dev)
        if kind == "adam":
            if case["ema"]:
                ops.adam_flat_ema(t["p"], g, t["m"], t["v"], t["e"], *a, wd, k, guard=guard, **skw, **ema_kw)
            elif guard is not None:
                ops.adam_flat_guarded(t["p"], g, t["m"], t["v"], *a, wd, k, guard, **skw)
            else:
                ops.adam_flat(t["p"], g, t["m"], t["v"], *a, wd, k, **skw)
        elif kind == "sgd":
            m, nest, kw = case["momentum"], case["nesterov"], dict(grad_scale=GRAD_SCALE, lr_dev=lr_dev)
            if case["ema"]:
                ops.sgd_flat_ema(t["p"], g, t.get("buf"), t["e"], lr_host, m, wd, guard=guard, nesterov=nest, **kw, **ema_kw)
            elif guard is not None:
                ops.sgd_flat_guarded(t["p"], g, t.get("buf"), lr_host, m, wd, guard, nesterov=nest, **kw)
            else:
                ops.sgd_flat(t["p"], g, t.get("buf"), lr_host, m, wd, nest, **kw)
        elif kind == "adam_table":
            ops.adam_flat_table(table, t["p"], g, t["m"], t["v"], *a, k, guard=guard, ema=t["e"], **skw, **ema_kw)
        elif kind == "lamb":
            ops.lamb_flat(table, t["p"], g, t["m"], t["v"], *a, k, guard=guard, ema=t["e"], **skw, **ema_kw)
        elif kind == "sgd_table":
            ops.sgd_flat_table(table, t["p"], g, t["buf"], lr_host, case["momentum"], nesterov=case["nesterov"],
                               grad_scale=GRAD_SCALE, lr_dev=lr_dev, trust_coefficient=table_spec["trust_coefficient"], guard=guard,
                               ema=t["e"], **ema_kw)
        else:
            raise ValueError(kind)
    torch.cuda.synchronize()
    for name, b in list(B.items()) + [("g", G)]:
        assert b.surroundings_untouched(), f"{case['name']}: a float outside the slice of {name} changed (placement {placement})"
    assert np.array_equal(G.bits(), np.asarray(vals["g"]).view(np.int32)), f"{case['name']}: the gradient changed"
    aux = [-1 if step_dev is None else int(step_dev), -1 if updates is None else int(updates),
           -1 if guard is None else int(guard.clip_coef.view(torch.int32))]
    if table is not None and kind != "adam_table":
        aux += [int(x) for x in table.trust.cpu().numpy().view(np.int32)]
    return {k: b.bits() for k, b in B.items()}, aux


def run_case(case, inputs, placement, dev):
    """``case`` over ``inputs`` (float32 [6, 1042]) with every slice ``placement`` x 16 bytes into its allocation.
    -> (int32 [buffers, 1042], int64 aux).  Asserts that nothing around a slice, in a table's gaps or in the gradient changed."""
    rows = {name: split(inputs[k]) for k, name in enumerate(ROWS)}
    names = buffers(case)
    out = np.empty((len(names), COLS), np.int32)
    aux = []
    if case["kind"] in ("adam", "sgd"):
        col = 0
        for n in SIZES:
            bits, a = _run(case, {k: rows[k][n] for k in ROWS}, placement, dev)
            for r, k in enumerate(names):
                out[r, col:col + n] = bits[k]
            aux += a
            col += n
    else:
        vals = {}
        for k in ROWS:
            flat = _pattern(TABLE["numel"])
            for (o, n) in TABLE["layout"]:
                flat[o:o + n] = mild(rows[k][n], 1e-4 if k == "v" else 0.0) if case.get("mild") else rows[k][n]
            vals[k] = flat
        bits, aux = _run(case, vals, placement, dev, TABLE)
        for r, k in enumerate(names):
            out[r] = np.concatenate([bits[k][o:o + n] for o, n in TABLE["layout"]])
    return out, np.asarray(aux, np.int64)


def clip_coefs(case, aux):
    """The clip coefficients (float32) a case's aux holds."""
    words = aux[2::3][:len(SIZES)] if case["kind"] in ("adam", "sgd") else aux[2:3]
    return np.asarray(words, np.int64).astype(np.int32).view(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library is loaded: goes into the metadata")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
    import torch
    assert torch.cuda.is_available(), "the bits are the GPU's: there is nothing to record without one"
    dev = torch.device("cuda:0")
    inputs = make_inputs()
    arrays = {"inputs": inputs.view(np.int32)}
    for case in cases():
        got = [run_case(case, inputs, placement, dev) for placement in (0, 1)]
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), \
            f"{case['name']}: the two placements disagree"
        out, aux = got[0]
        if case["guard"] == "clip":
            c = clip_coefs(case, aux)
            assert ((c > 0.25) & (c < 0.5)).all(), (case["name"], c)       # strictly inside a binade: no power of two
        if case["guard"] == "skip":
            want = np.stack([inputs[ROWS.index(k)] for k in buffers(case)]).view(np.int32)
            assert np.array_equal(out, want) and (aux[0::3] == 0).all(), f"{case['name']}: a skipped step wrote something"
        else:
            arrays["out/" + case["name"]] = out
        if case.get("mild"):
            assert moved(case, inputs, out) > 0.9, (case["name"], moved(case, inputs, out))
        arrays["aux/" + case["name"]] = aux
        print(case["name"], "ok", flush=True)
    meta = dict(commit=a.commit, device=torch.cuda.get_device_name(0), steps=STEPS, sizes=SIZES, cases=[c["name"] for c in cases()],
                note="recorded once from the library of `commit`; replayed by tests/test_gpu_optim_bits.py")
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    size = os.path.getsize(a.out)
    assert size <= 512 * 1000, f"{a.out}: {size} bytes"
    print(f"wrote {a.out}: {size} bytes, {len(cases())} cases", flush=True)


if __name__ == "__main__":
    main()
