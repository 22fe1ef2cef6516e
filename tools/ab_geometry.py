#!/usr/bin/env python3
"""Cost of the geometry-only forward (CFNERF_F_GEOMETRY) against the full eval launch: ONE process on one GPU, the two launches
alternating on the same model, rays and latents, every fused-forward launch timed by HIP events on the launch stream
(cfnerf_timing_enable(m, 2) / cfnerf_timing_fwd_mean_ms); median per mode, their ratio and the run-to-run spread.  Then the throughput of
`evaluate.density_grid` (points mode) in points per second.
    python tools/ab_geometry.py [--launches 20] [--grid 128] [--out profiles/r09_geometry_ab.txt]
Shapes: the C2 eval shape (1024 fern-shaped NDC rays x 128 samples, K = 4, W = 256) and 8192 rays of C5 (Blender intrinsics, K = 32,
W = 256).  Both launches write the per-K depth / disparity maps; the full one also its colour map.  Every timed section runs under its
own time limit (SIGALRM): a section that is SLOW - still returning to the interpreter between launches - ends the process when it exceeds
it, and nothing is started after it.  Python runs signal handlers only between bytecodes, so this does NOT end a launch that hangs inside a
synchronising HIP call: run the tool under an outer limit that kills the process (`timeout -k 10 400 python tools/ab_geometry.py ...`)."""
import argparse
import contextlib
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--grid", type=int, default=128)
ap.add_argument("--limit", type=int, default=120, help="seconds per timed section")
ap.add_argument("--out", default=None)
a = ap.parse_args()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
import cfnerf_amd  # noqa: E402
from cfnerf_amd import _lib as L  # noqa: E402
from cfnerf_amd import evaluate as EV  # noqa: E402
from cfnerf_amd.api import _pack_rays, _render_fwd, _render_geometry_fwd, t_vals_table  # noqa: E402


@contextlib.contextmanager
def time_limit(seconds, what):
    def over(signum, frame):
        raise TimeoutError(f"{what}: over its time limit of {seconds} s")
    signal.signal(signal.SIGALRM, over)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def model(K, scene):
    sc = bench.SCENES[scene]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        kw, _, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(netwidth=256, netdepth=bench.D, K_samples=K, h_alpha_size=32, device=dev,
                                                                        no_ndc=not sc["ndc"], white_bkgd=sc["white_bkgd"],
                                                                        dataset_type="llff" if sc["ndc"] else "blender"))
    net = kw["network_fn"].module
    net._sync()
    return net, sc


def summ(v):
    v = sorted(v)
    med = statistics.median(v)
    return {"median": med, "min": v[0], "max": v[-1], "spread_pct": 100.0 * (v[-1] - v[0]) / med}


def ab(name, net, packed, flags, launches):
    lib, tv, eps = L.lib(), t_vals_table(dev), net.eval_eps()
    lib.cfnerf_timing_enable(net.handle, 2)
    acc = {"full": [], "geometry": []}
    with time_limit(a.limit, name), torch.no_grad():
        for i in range(2 + launches):
            for mode in ("full", "geometry"):
                if mode == "full":
                    _render_fwd(net, packed, tv, None, eps, flags, entropy=False)
                else:
                    _render_geometry_fwd(net, packed, tv, eps, flags | L.F_GEOMETRY)
                torch.cuda.synchronize()
                if i >= 2:
                    acc[mode].append(float(lib.cfnerf_timing_fwd_mean_ms(net.handle, 1)))
    f, g = summ(acc["full"]), summ(acc["geometry"])
    return {"shape": name, "rays": int(packed.shape[0]), "K": net.K_samples, "launches": launches, "full_ms": f, "geometry_ms": g,
            "ratio": g["median"] / f["median"]}


rows = []
net, sc = model(4, "fern")
rays = bench.synth_rays(np.random.default_rng(1000), 1024, sc["H"], sc["W"], sc["focal"]).to(dev)
packed = _pack_rays(sc["H"], sc["W"], sc["focal"], rays=rays, ndc=True, near=sc["near"], far=sc["far"], device=dev)
rows.append(ab("C2 eval: 1024 rays x 128 x K=4, W=256", net, packed, 0, a.launches))
del net

net, sc = model(32, "blender")
packed = _pack_rays(sc["H"], sc["W"], sc["focal"], c2w=bench.blender_pose(), n=8192, pixel0=400 * sc["W"], ndc=False, near=sc["near"], far=sc["far"],
                    device=dev)
rows.append(ab("C5: 8192 rays x 128 x K=32, W=256", net, packed, L.F_WHITE_BKGD, a.launches))

with time_limit(a.limit, "density_grid"), torch.no_grad():
    EV.density_grid(net, (-1.5,) * 3, (1.5,) * 3, (32, 32, 32))                       # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    EV.density_grid(net, (-1.5,) * 3, (1.5,) * 3, (a.grid,) * 3)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
pps = a.grid ** 3 / dt

lines = ["# r09: the geometry-only forward (CFNERF_F_GEOMETRY) against the full eval launch, one process, alternating launches, HIP events around",
         "# the fused-forward launch (tools/ab_geometry.py).  Yardstick: the full launch of the same run (run to run +-0.3 %, profiles/r06_ab_runs.txt).",
         "# Expectation from the operation count: ratio <= 0.8135 + 0.1865 x (the non-MFMA share of the launch).", "#"]
for r in rows:
    f, g = r["full_ms"], r["geometry_ms"]
    lines.append(f"{r['shape']}  ({r['launches']} launches each)")
    lines.append(f"  full      median {f['median']:.4f} ms   min {f['min']:.4f}   max {f['max']:.4f}   spread {f['spread_pct']:.2f} %")
    lines.append(f"  geometry  median {g['median']:.4f} ms   min {g['min']:.4f}   max {g['max']:.4f}   spread {g['spread_pct']:.2f} %")
    lines.append(f"  ratio geometry / full = {r['ratio']:.4f}")
lines.append(f"density_grid  res = {a.grid}^3, K = 32, W = 256, chunk = 2^20:  {dt * 1e3:.1f} ms wall  =  {pps / 1e6:.2f} M points / s")
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
