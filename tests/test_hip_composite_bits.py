"""-m gpu: the four stand-alone composite kernels give the bits of the commit BEFORE their bodies were merged
(csrc/cfnerf_comp_fwd_body.h, csrc/cfnerf_comp_bwd_body.h).

tests/golden/composite_bits/MANIFEST.json holds the SHA-256 of every output of every call of tests/composite_bits_common.py, written by
tests/golden/make_golden_composite_bits.py from that commit's library (its id is in the manifest) - never from the code under test.
A failure means that an edit of a shared body moved a bit: the fix goes into the body, not into the manifest."""
import json
import os

import pytest

import composite_bits_common as CB

pytestmark = pytest.mark.gpu
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite_bits", "MANIFEST.json")


@pytest.fixture(scope="module")
def golden():
    with open(MANIFEST) as f:
        m = json.load(f)
    assert len(m["commit"]) == 40 and m["scheme"] == "sha256 of the fp32 bytes, C order"
    return m["hashes"]


def test_the_manifest_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(key for key, _ in CB.cases())


@pytest.mark.parametrize("kind", ["fwd", "sparse all", "sparse holes", "bwd"])
def test_outputs_carry_the_bits_of_the_parent_commit(golden, kind):
    import torch
    n, bad = 0, []
    for key, thunk in CB.cases():
        if not key.startswith(kind + " "):
            continue
        out = thunk()
        torch.cuda.synchronize()
        assert sorted(out) == sorted(golden[key]), key
        bad += [f"{key}: {name}" for name, t in out.items() if CB.sha(t) != golden[key][name]]
        n += len(out)
    assert n > 0 and not bad, f"{len(bad)} of {n} outputs differ from the parent commit's, e.g. {bad[:5]}"
