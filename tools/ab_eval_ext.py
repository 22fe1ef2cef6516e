#!/usr/bin/env python3
"""Cost of the extended K-statistics (CFNERF_F_KSTATS_EXT) on the fused eval render: ONE process, `render_uncertainty` with
stats="basic" and stats="ext" (ground truth given, so the NLL columns are written) launched alternately on the same model and image,
the fused-forward launch of every call timed by HIP events on the launch stream (cfnerf_timing_enable(m, 2)); median / p10 per mode.
    python tools/ab_eval_ext.py --shape c5|k128 [--steps 8]
c5: bench.py's C5 (800 x 800, K = 32, W = 256, Blender intrinsics, white background).  k128: 200 x 200 at K = 128, same scene."""
import argparse
import contextlib
import json
import statistics
import sys
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="c5", choices=["c5", "k128"])
ap.add_argument("--steps", type=int, default=8)
a = ap.parse_args()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
import cfnerf_amd  # noqa: E402
from cfnerf_amd import _lib as L  # noqa: E402
from cfnerf_amd import evaluate as EV  # noqa: E402

sc = bench.SCENES["blender"]
K, H, W, focal = (32, sc["H"], sc["W"], sc["focal"]) if a.shape == "c5" else (128, 200, 200, sc["focal"] * 200 / sc["W"])
torch.manual_seed(0)
with contextlib.redirect_stdout(sys.stderr):
    kw_train, _, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(netwidth=256, netdepth=bench.D, K_samples=K, h_alpha_size=32, device=dev,
                                                                          no_ndc=True, white_bkgd=True, dataset_type="blender"))
net = kw_train["network_fn"].module
lib = L.lib()
lib.cfnerf_timing_enable(net.handle, 2)
c2w = bench.blender_pose()
gt = torch.rand(H, W, 3, device=dev)
kw = dict(near=sc["near"], far=sc["far"], ndc=False, white_bkgd=True, gt=gt)
acc = {"basic": [], "ext": []}
with torch.no_grad():
    for i in range(2 + a.steps):
        for mode in ("basic", "ext"):
            EV.render_uncertainty(H, W, focal, c2w, net, stats=mode, **kw)
            torch.cuda.synchronize()
            if i >= 2:
                acc[mode].append(lib.cfnerf_timing_last_ms(net.handle, 0))


def summ(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "mean": round(sum(v) / len(v), 4), "p10": round(v[len(v) // 10], 4), "max": round(v[-1], 4)}


b, e = summ(acc["basic"]), summ(acc["ext"])
print(json.dumps({"lib": os.environ.get("CFNERF_LIB", "default").split("/")[-1], "shape": a.shape, "image": [H, W], "K": K, "steps": a.steps,
                  "fwd_ms_basic": b, "fwd_ms_ext": e, "ext_over_basic": round(e["median"] / b["median"], 5)}))
