#!/usr/bin/env python3
"""Write tests/golden/composite_bits/MANIFEST.json: the SHA-256 of every output of the calls of tests/composite_bits_common.py, from the
library of the commit BEFORE the bodies of the four stand-alone composite kernels were merged (csrc/cfnerf_comp_*_body.h; needs a GPU).

Run:  CFNERF_LIB=<libcfnerf_hip.so built from that commit> python tests/golden/make_golden_composite_bits.py --commit <its 40-hex id> [--out DIR]

The script refuses to run without CFNERF_LIB: it never hashes what the in-tree build - the code under test - computes.  The manifest
records the commit id; the fixture holds hashes only."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the 40-hex id of the commit CFNERF_LIB was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "composite_bits"))
    a = ap.parse_args()
    lib = os.environ.get("CFNERF_LIB")
    if not lib or not os.path.exists(lib):
        sys.exit("CFNERF_LIB must name the parent commit's build of libcfnerf_hip.so: the in-tree build is the code under test")
    if len(a.commit) != 40 or any(c not in "0123456789abcdef" for c in a.commit):
        sys.exit("--commit takes the full 40-hex commit id")
    import cfnerf_amd  # noqa: F401
    import composite_bits_common as CB
    hashes = CB.run_all()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "MANIFEST.json"), "w") as f:
        json.dump({"commit": a.commit, "scheme": "sha256 of the fp32 bytes, C order", "hashes": hashes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} calls, {sum(len(v) for v in hashes.values())} outputs -> {os.path.join(a.out, 'MANIFEST.json')}")


if __name__ == "__main__":
    main()
