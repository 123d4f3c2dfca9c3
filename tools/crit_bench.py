"""Dev tool: the criterion alone — forward + backward + bank update — for the term sets that take the general fused kernel
(ops.crit_fused) and the stock AVID+CMA set (ops.cma_fused), against the unfused chain of the same criterion object (ops.FUSED_CRITERION off), at bs 64, K 1024, 240 k-row
banks.  Times are the library's HIP-event timers summed over every library launch of a step (torch's own glue kernels of the
unfused chain — cat, slice copies, the gradient adds — are NOT in them: the unfused figure is a lower bound), plus the step's
wall time between two stream events.  The two paths alternate round by round in one process; per path the median over the
rounds and the spread (min .. max) are printed, and one JSON line at the end.
usage: python tools/crit_bench.py [rounds=15] [steps per round=10]"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "avid-cma_amd"))
import torch  # noqa: E402
import criterions  # noqa: E402
from avid_hip import lib, ops  # noqa: E402
from criterions.avid_cma import AVIDSimilarityPositiveExpansion  # noqa: E402
from criterions.nce import NCECriterion  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device("cuda:0")
B, K, KW, P, N = 64, 1024, 64, 32, 240000


def avid(xc, wc):
    return criterions.AVID(num_data=N, embedding_dim=128, num_negatives=K, momentum=0.5, xModal_coeff=xc, wModal_coeff=wc, device=0)


def cma(coeffs):
    """AVID_CMA without the correspondence search of its constructor (minutes at 240 k rows): a random sorted positive set."""
    crit = criterions.AVID_CMA.__new__(criterions.AVID_CMA)
    torch.nn.Module.__init__(crit)
    xi, wi, xp, wp = coeffs
    na = AVIDSimilarityPositiveExpansion(memory_size=N, embedding_dim=128, num_negatives=K, num_negatives_within=KW,
                                         xModalInst=xi > 0, wModalInst=wi > 0, xModalPos=xp > 0, wModalPos=wp > 0,
                                         sampling_args={"type": "consensus", "pos_k": P}, momentum=0.5, device=0)
    na.register_buffer("positive_set", torch.randint(0, N, (N, P), device=dev).sort(1).values.int())
    crit.nce_average = na
    s = sum(coeffs)
    crit.xModalInstCoeff, crit.wModalInstCoeff, crit.xModalPosCoeff, crit.wModalPosCoeff = (c / s for c in coeffs)
    crit.criterion = NCECriterion(N).to(dev)
    return crit


SETS = {"self-avid": lambda: avid(0., 1.), "joint-avid": lambda: avid(1., 1.), "cma-three-groups": lambda: cma((1., 0., 1., 1.)),
        "cma-stock": lambda: cma((1., 0., 0., 1.))}
result = {}
for name, make in SETS.items():
    crit = make()
    ve = torch.randn(B, 128, device=dev, requires_grad=True)
    ae = torch.randn(B, 128, device=dev, requires_grad=True)
    ids = [torch.randperm(N)[:B].to(dev) for _ in range(steps)]

    def step(y):
        loss, _ = crit(ve, ae, y)
        loss.backward()

    ops.FUSED_CRITERION = False
    for y in ids[:3]:                       # the first step freezes Z; warm both paths
        step(y)
    ops.FUSED_CRITERION = True
    for y in ids[:3]:
        step(y)
    torch.cuda.synchronize()
    per = {True: [], False: []}
    wall = {True: [], False: []}
    launches = {}
    for r in range(rounds):
        for fused in ((True, False) if r % 2 == 0 else (False, True)):
            ops.FUSED_CRITERION = fused
            lib.timing_enable(True)
            for y in ids:
                step(y)
            torch.cuda.synchronize()
            rep = lib.timing_report()
            lib.timing_enable(False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()                     # the wall time without the timers' event pairs
            for y in ids:
                step(y)
            e1.record()
            torch.cuda.synchronize()
            per[fused].append(sum(v["ms"] for v in rep.values()) / steps * 1e3)
            wall[fused].append(e0.elapsed_time(e1) / steps * 1e3)
            launches[fused] = {k: v["launches"] // steps for k, v in sorted(rep.items())}
    ops.FUSED_CRITERION = True
    out = {}
    for fused in (True, False):
        tag = "fused" if fused else "unfused"
        med, lo, hi = statistics.median(per[fused]), min(per[fused]), max(per[fused])
        out[tag] = {"kernel_us_median": round(med, 2), "kernel_us_min": round(lo, 2), "kernel_us_max": round(hi, 2),
                    "wall_us_median": round(statistics.median(wall[fused]), 1), "wall_us_min": round(min(wall[fused]), 1),
                    "wall_us_max": round(max(wall[fused]), 1), "library_launches_per_step": sum(launches[fused].values()),
                    "launches": launches[fused]}
        print(f"{name:18s} {tag:8s} library kernels {med:8.2f} us/step (min {lo:.2f} max {hi:.2f})  wall {out[tag]['wall_us_median']:8.1f} us/step "
              f"(min {out[tag]['wall_us_min']:.1f} max {out[tag]['wall_us_max']:.1f})  {out[tag]['library_launches_per_step']} library launches")
    u, f = out["unfused"], out["fused"]
    out["ratio_kernel"] = round(u["kernel_us_median"] / f["kernel_us_median"], 2)
    out["ratio_wall"] = round(u["wall_us_median"] / f["wall_us_median"], 2)
    out["fused_faster_than_the_unfused_spread"] = bool(
        f["kernel_us_median"] < u["kernel_us_median"] - (u["kernel_us_max"] - u["kernel_us_min"])
        and f["wall_us_median"] < u["wall_us_median"] - (u["wall_us_max"] - u["wall_us_min"]))
    print(f"{name:18s} unfused / fused: library kernels x{out['ratio_kernel']}, wall x{out['ratio_wall']}")
    result[name] = out
    del crit
print(json.dumps({"bs": B, "K": K, "Kw": KW, "P": P, "N": N, "rounds": rounds, "steps": steps, "sets": result}))
