"""Every launch program compiles to the bytes recorded in tests/golden/plan_programs.json (no GPU).

The matrix (tests/_plan_snapshot.py): the two-tower ``Plan`` at three geometries and three stream arrangements, ``ClsPlan`` full /
classifier-only at the shipped fine-tuning shapes and a small one, ``ProbePlan`` at the shipped and a small batch, ``EvalPlan`` of
all four models.  Per plan: the CRC-32 of every record of every program, the arena / aux / workspace sizes, the gradient-buffer
layout, the order in which gradients complete, the weight-transform table, and for inference programs the recycled arena, the
outputs and the BatchNorm table.  A record holds geometry, integers and ``(slot, offset)`` references, no address, so the file
does not depend on the process that wrote it.

The golden is valid for 256 compute units: the library's figure when no device is present, and an MI355X's.  It was written by
tools/plan_snapshot.py; a change that moves records or dispatch on purpose regenerates it with that tool and shows the diff."""
import pytest

import _plan_snapshot as S


@pytest.fixture(scope="module")
def golden_snapshot():
    return S.load()


def test_golden_holds_the_matrix_and_nothing_else(golden_snapshot):
    assert sorted(golden_snapshot) == S.names() and len(S.names()) == 29


@pytest.mark.parametrize("name", S.names())
def test_plan_compiles_to_the_recorded_programs(name, golden_snapshot):
    from avid_hip import plan
    want = golden_snapshot[name]
    pl = S.compile_plan(name)
    got = S.entry(pl)
    assert sorted(got["programs"]) == sorted(want["programs"]), name
    for pname, prog, n in S.programs(pl):
        g, w = got["programs"][pname], want["programs"][pname]
        k = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), None)
        if k is None and len(g) != len(w):
            k = min(len(g), len(w))
        if k is not None:
            line = plan.dump(prog, n).split("\n")[k] if k < n else "(the program ends here)"
            print(f"{name}: program {pname!r} differs first at record {k} ({len(g)} records, golden {len(w)}):\n{line}")
            pytest.fail(f"{name}: program {pname!r}, record {k}: {line}")
    diff = {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if k != "programs" and got.get(k) != want.get(k)}
    assert not diff, (name, diff)
