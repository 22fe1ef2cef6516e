"""-m gpu: the fused forward and the geometry-only forward give the bits of the commit BEFORE their shared phases became one text
(csrc/cfnerf_fwd_trunk_body.h, csrc/cfnerf_fwd_halpha_body.h) and their launchers one helper.

tests/golden/fwd_bits/MANIFEST.json holds the SHA-256 of every output of every launch of tests/fwd_bits_common.py, written by
tests/golden/make_golden_fwd_bits.py from that commit's library (its id is in the manifest) - never from the code under test.  For a
launch with an activation stash the flat gradient of the (untouched) backward on that stash is hashed as well: it pins the stash.
A failure means that an edit of a shared body or of the launch helper moved a bit: the fix goes there, not into the manifest."""
import json
import os

import pytest

import fwd_bits_common as FB

pytestmark = pytest.mark.gpu
MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_bits", "MANIFEST.json")


@pytest.fixture(scope="module")
def golden():
    with open(MANIFEST) as f:
        m = json.load(f)
    assert len(m["commit"]) == 40 and m["scheme"] == "sha256 of the fp32 bytes, C order"
    return m["hashes"]


def test_the_manifest_holds_exactly_the_cases(golden):
    keys = FB.keys()
    assert len(set(keys)) == len(keys) and sorted(golden) == sorted(keys)


@pytest.mark.parametrize("name", list(FB.MODELS))
def test_outputs_carry_the_bits_of_the_parent_commit(golden, name):
    net = FB.build(name)
    n, bad = 0, []
    for s in FB.specs(name):
        key = FB.key(name, s)
        out = FB.run(net, s)
        assert sorted(out) == sorted(golden[key]), key
        bad += [f"{key}: {what}" for what, t in out.items() if FB.sha(t) != golden[key][what]]
        n += len(out)
    assert n > 0 and not bad, f"{len(bad)} of {n} outputs differ from the parent commit's, e.g. {bad[:5]}"
