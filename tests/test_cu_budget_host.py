"""The planner under reduced CU budgets, on the host: tests/_budget_ref.py's table of (layer, budget) -> plans is what the
library reports (``avid_conv_kernel_name``; without a GPU it plans for 256 physical CUs, and a plan for a budget below the
physical count does not depend on the device), and the table reaches every class of plan_pk_tile's decision space for the
forward and for the input gradient.  tests/test_gpu_cu_budget.py runs the same rows against float64.

``avid_set_cu_budget`` is process-global: the library is asked in a process of its own."""
import functools
import json
import os
import subprocess
import sys

import _budget_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _reported():
    out = subprocess.run([sys.executable, os.path.join(HERE, "_budget_ref.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-1500:])
    rows, full, cus = {}, {}, None
    for ln in out.stdout.splitlines():
        if ln.startswith("ROW "):
            v = json.loads(ln[4:])
            rows[(v[0], v[1])] = tuple(v[2:])
        elif ln.startswith("FULL "):
            v = json.loads(ln[5:])
            full[v[0]] = tuple(v[1:])
        elif ln.startswith("CUS "):
            cus = int(ln[4:])
    return rows, full, cus


def test_the_table_is_what_the_library_reports():
    rows, full, cus = _reported()
    assert cus is not None and cus >= 256 and cus % 8 == 0          # (a plan for a budget below the count is the 256-CU plan)
    assert len({R.row_id(r) for r in R.ROWS}) == len(R.ROWS)
    for row in R.ROWS:
        assert rows[tuple(row[:2])] == tuple(row[2:5]), (R.row_id(row), rows[tuple(row[:2])])
    for layer, budget, dgrad in R.CHAIN_ROWS:
        assert rows[(layer, budget)][1] == dgrad, (layer, budget, rows[(layer, budget)])
    if cus == 256:
        assert set(full) == set(R.FULL)
        for layer, names in R.FULL.items():
            assert full[layer] == tuple(names), (layer, full[layer])


def test_every_class_of_plan_has_a_row_for_the_forward_and_for_the_input_gradient():
    for which in (0, 1):
        seen = {}
        for row in R.ROWS:
            for c in R.classes(row[0], row[1], which, row[2 + which]):
                seen.setdefault(c, []).append(R.row_id(row))
        assert set(seen) == set("abcdefghi"), (which, sorted(set("abcdefghi") - set(seen)))
    # the other kernel families whose grids follow the budget
    names = [n for row in R.ROWS for n in row[2:5]]
    for prefix in ("tconv64_kernel<0>", "twgrad64_kernel", "wino_kernel<0>", "wino_kernel<1>", "wino_wgrad_kernel",
                   "igemm_pk_kernel<4,1,1,2,1>s2", "igemm_pk_kernel over the sub-sampled grid"):
        assert any(n.startswith(prefix) for n in names), prefix
    # the chain rows: whole rounds + unsplit tail, whole rounds + K-split tail, weight-stationary, on a 64- and a 128-channel layer
    chain = {}
    for layer, budget, dgrad in R.CHAIN_ROWS:
        chain.setdefault(layer, set()).update(R.classes(layer, budget, 1, dgrad))
    assert set("bcd") <= set().union(*chain.values()) and set(chain) == set(R.CHAIN_LAYERS)


def test_the_class_rules_on_hand_worked_plans():
    """R.classes against plan_pk_tile worked by hand: 64 columns on the 128 x 64 tile are one column block, so C = budget and
    the grid is 2 * budget workgroups; 192 columns are three (C = 15 of 16 CUs, G = 30); 128 columns on the 128 x 128 tile one."""
    pk, pkw = R.PK % 0, R.PKW % 0
    assert R.classes("s64", 8, 0, pk + "full=40 tail_units=0 f=1") == {"a"}             # 40 tiles on G = 16: 2.5 rounds
    assert R.classes("s64", 8, 0, pk + "full=32 tail_units=0 f=1") == set()             # two whole rounds: not ragged
    assert R.classes("s64", 24, 0, pk + "full=24 tail_units=16 f=1") == {"b"}
    assert R.classes("s64", 16, 0, pk + "full=32 tail_units=16 f=2") == {"c"}
    assert R.classes("s64", 16, 0, pk + "full=0 tail_units=15 f=3" + R.WS) == {"d"}
    assert R.classes("s64", 16, 0, pk + "full=0 tail_units=16 f=4") == {"e"}
    assert R.classes("s128", 24, 0, pkw + "full=48 tail_units=24 f=6") == {"c", "f"}
    assert R.classes("s64_192", 16, 0, pk + "full=15 tail_units=9 f=1") == {"b", "g"}
    assert R.classes("s64_192", 16, 1, R.PK % 1 + "full=0 tail_units=16 f=2" + R.WS) == {"d"}    # 64 columns the other way
    assert R.classes("s64", 8, 0, pk + "full=0 tail_units=4 f=1") == {"h"}              # 4 <= 8 / 2
    assert R.classes("s64", 8, 0, pk + "full=0 tail_units=5 f=1") == set()
    assert R.classes("t64", 24, 0, pk + "full=48 tail_units=1 f=1") == {"b", "i"}
    assert R.classes("wino256", 8, 0, "wino_kernel<0> grid=8") == set()
    assert R.family(R.S2) == (["igemm_pk_kernel<4,1,1,2,1>s2"], False)
    assert R.family(pk + "full=32 tail_units=16 f=2") == (["igemm_pk_kernel<4,1,1,2,0>"], True)


def test_rows_held_to_the_full_budget_bits_exist():
    """Bit-identity to the full-budget run is asserted where both plans are unsplit on the same kernel template: the table
    has such rows for y and for dx."""
    got = {R.row_id(r): R.bit_identical_outputs(r) for r in R.ROWS}
    assert got["t64@24"] == {0, 1} and got["t64_tiny@8"] == {0, 1} and got["s2_res@8"] == {0}
    assert got["t64@8"] == set() and got["wino256@8"] == set() and got["s64@24"] == set()
