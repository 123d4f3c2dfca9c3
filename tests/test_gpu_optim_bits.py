"""The flat optimizers against their recorded bits (tests/golden/optim_flat_bits.npz, tools/record_optim_bits.py).

The file was recorded once, from the library of the commit its metadata names — the last one whose flat Adam kernels left
their contractions to the compiler — and is the fixed anchor of the arithmetic: every case is replayed on the inputs the file
holds and compared with ``view(int32)`` equality, no tolerance, at the start of an allocation and 16 bytes into one.  A failure
here is a change of behaviour, not a fixture to record again."""
import json

import numpy as np
import pytest

import tools_path  # noqa: F401  (tests -> tools/)
import record_optim_bits as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.fixture(scope="module")
def recorded(golden):
    f = golden("optim_flat_bits")
    return {k: f[k] for k in f.files}


def test_the_file_holds_every_case(recorded):
    meta = json.loads(bytes(recorded["meta"]).decode())
    assert len(meta["commit"]) == 40 and meta["steps"] == R.STEPS and tuple(meta["sizes"]) == R.SIZES
    assert meta["cases"] == [c["name"] for c in CASES]
    inputs = recorded["inputs"].view(np.float32)
    assert inputs.shape == (len(R.ROWS), R.COLS) and np.isfinite(inputs).all()
    assert np.array_equal(recorded["inputs"], R.make_inputs().view(np.int32))      # the file holds them; the builder agrees
    for c in CASES:
        assert ("out/" + c["name"] in recorded) == (c["guard"] != "skip") and "aux/" + c["name"] in recorded, c["name"]
    # what the inputs were chosen to contain
    p, g, m, v = inputs[:4]
    assert (np.signbit(g) & (g == 0)).any() and (g == 0).any() and (v == 0).any()
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(g) > 0) & (np.abs(g) < tiny)).any() and ((np.abs(p) > 0) & (np.abs(p) < tiny)).any()
    assert (np.abs(g) >= 1e18).any() and ((np.abs(g) > 0) & (np.abs(g) <= 1e-17) & (np.abs(g) >= tiny)).any()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_recorded_bits(gpu_device, recorded, case):
    """Three consecutive steps; every buffer, the step counter, the counter of averaging updates, the clip coefficient and the
    trust factors, bit for bit; the floats around every slice untouched (``run_case`` asserts that)."""
    inputs = recorded["inputs"].view(np.float32)
    names = R.buffers(case)
    if case["guard"] == "skip":           # nothing may change: the expectation is the inputs themselves
        want = np.stack([recorded["inputs"][R.ROWS.index(k)] for k in names])
    else:
        want = recorded["out/" + case["name"]]
    want_aux = recorded["aux/" + case["name"]]
    if case.get("mild"):
        assert R.moved(case, inputs, want) > 0.9          # this case anchors the update of p, not only the moments
    if case["guard"] == "clip":
        c = R.clip_coefs(case, want_aux)
        assert ((c > 0.25) & (c < 0.5)).all(), c          # clipped, by no power of two
    for placement in (0, 1):
        got, aux = R.run_case(case, inputs, placement, gpu_device)
        assert got.dtype == np.int32 and got.shape == want.shape
        for r, k in enumerate(names):
            bad = np.flatnonzero(got[r] != want[r])
            assert bad.size == 0, (case["name"], placement, k, bad[:8].tolist(), got[r][bad[:4]].view(np.float32).tolist(),
                                   want[r][bad[:4]].view(np.float32).tolist())
        assert np.array_equal(aux, want_aux), (case["name"], placement, aux.tolist(), want_aux.tolist())
