#!/usr/bin/env python3
"""Write tests/golden/fwd_bits/MANIFEST.json: the SHA-256 of every output of the launches of tests/fwd_bits_common.py, from the library of
the commit BEFORE the shared phases of fused_fwd_kernel and geom_fwd_kernel became one text (csrc/cfnerf_fwd_*_body.h; needs a GPU).

Run:  CFNERF_LIB=<libcfnerf_hip.so built from that commit> python tests/golden/make_golden_fwd_bits.py --commit <its 40-hex id> [--out DIR]

The script refuses to run without CFNERF_LIB: it never hashes what the in-tree build - the code under test - computes.  Every launch runs
twice and must hash alike (a manifest of outputs that are not reproducible would be worthless).  The manifest records the commit id;
the fixture holds hashes only."""
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
    ap.add_argument("--out", default=os.path.join(HERE, "fwd_bits"))
    a = ap.parse_args()
    lib = os.environ.get("CFNERF_LIB")
    if not lib or not os.path.exists(lib):
        sys.exit("CFNERF_LIB must name the parent commit's build of libcfnerf_hip.so: the in-tree build is the code under test")
    if len(a.commit) != 40 or any(c not in "0123456789abcdef" for c in a.commit):
        sys.exit("--commit takes the full 40-hex commit id")
    import cfnerf_amd  # noqa: F401
    import fwd_bits_common as FB
    hashes = FB.run_all()
    again = FB.run_all()
    moved = [f"{k}: {n}" for k, v in hashes.items() for n in v if again[k][n] != v[n]]
    if moved:
        sys.exit(f"{len(moved)} outputs are not reproducible between two runs, e.g. {moved[:5]}")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "MANIFEST.json"), "w") as f:
        json.dump({"commit": a.commit, "scheme": "sha256 of the fp32 bytes, C order", "hashes": hashes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} calls, {sum(len(v) for v in hashes.values())} outputs -> {os.path.join(a.out, 'MANIFEST.json')}")


if __name__ == "__main__":
    main()
