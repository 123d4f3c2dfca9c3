"""The three fused criterion entry points against their recorded bits (tests/golden/crit_fused_bits.npz,
tools/record_crit_bits.py).

The file was recorded once on an MI355X from the library of commit a48ddbf877e2087654c6f5f203a46b48333f5cd5 — the last one in
which the stock forms (``xmodal_fused_kernel`` / ``xmodal_finish_kernel``) and the general form (``crit_fused_kernel`` /
``crit_finish_kernel``) were written out separately — and is the fixed anchor of their arithmetic.  Every case first asserts the
sha256 of its regenerated inputs (a mismatch means the seeded generators changed: a failure, never a skip), then calls its entry
point twice on one workspace and compares the second call's total, losses, normalised embeddings and both embeddings' gradients
with ``torch.equal`` on the int32 views, no tolerance.  A failure here is a change of behaviour, not a fixture to record again."""
import json

import numpy as np
import pytest
import torch

import tools_path  # noqa: F401  (tests -> tools/)
import record_crit_bits as R

pytestmark = pytest.mark.gpu

COMMIT = "a48ddbf877e2087654c6f5f203a46b48333f5cd5"
CASES = R.cases()


@pytest.fixture(scope="module")
def recorded(golden):
    f = golden("crit_fused_bits")
    return {k: f[k] for k in f.files}


def test_the_file_holds_every_case(recorded):
    meta = json.loads(bytes(recorded["meta"]).decode())
    assert meta["commit"] == COMMIT and meta["cases"] == [c["name"] for c in CASES]
    n_losses = {"xmodal": 4, "cma": 8, "crit": 16}
    for c in CASES:
        bs = c["shape"][0]
        assert recorded[c["name"] + "/sha256"].shape == (32,), c["name"]
        shapes = {k: recorded[c["name"] + "/" + k].shape for k in R.ARRAYS}
        assert shapes == dict(total=(1,), losses=(n_losses[c["op"]],), hats=(2, bs, 128), dv=(bs, 128), da=(bs, 128)), (c["name"], shapes)
        assert all(recorded[c["name"] + "/" + k].dtype == np.int32 for k in R.ARRAYS), c["name"]
        assert not recorded[c["name"] + "/losses"][R.WRITTEN[c["op"]]:].any(), c["name"]      # the unused word of cma_fused: 0
    assert len(recorded) == 6 * len(CASES) + 2


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_recorded_bits(gpu_device, recorded, case):
    c = R.make_inputs(case)
    assert np.array_equal(R.input_hash(c), recorded[case["name"] + "/sha256"]), f"{case['name']}: inputs changed"
    got = R.run_case(case, c, gpu_device)
    for k in R.ARRAYS:
        want = torch.from_numpy(recorded[case["name"] + "/" + k])
        have = torch.from_numpy(got[k])
        if k == "losses":                 # the words the entry point writes: losses[7] of cma_fused is unused, never written
            assert have.numel() == R.WRITTEN[case["op"]]
            want = want[:have.numel()]
        assert have.dtype == torch.int32 and have.shape == want.shape, (case["name"], k)
        if not torch.equal(have, want):
            bad = torch.nonzero(have.flatten() != want.flatten()).flatten()
            pytest.fail(f"{case['name']}: {k} differs in {bad.numel()} of {want.numel()} words, first at {bad[:4].tolist()}: got "
                        f"{have.flatten()[bad[:4]].view(torch.float32).tolist()}, recorded {want.flatten()[bad[:4]].view(torch.float32).tolist()}")
