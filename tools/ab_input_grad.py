#!/usr/bin/env python3
"""Cost of the input gradient (CFNERF_F_INPUT_GRAD) on cfnerf_network_bwd: ONE process on one GPU, the same model, points, latents and
cotangents; a stashed forward without the flag and its backward, then a stashed forward with the flag and its backward, alternating.
Each cfnerf_network_bwd call sits between two HIP events on the launch stream (all of its launches, the new stage included); medians
per mode, their difference (= the new stage) and the min-to-max spread.
    python tools/ab_input_grad.py [--launches 20] [--out profiles/r10_input_grad.txt]
    CFNERF_LIB=<another build> python tools/ab_input_grad.py --flagless-only      (the flag-less backward of another build, e.g. the parent's)
Shapes: P = 131072 points at W = 256, K = 4 (the C2 train batch through the unfused seam) and at W = 512, K = 32.
Run it under an outer limit that kills the process (`timeout -k 10 400 python tools/ab_input_grad.py ...`): a launch that hangs inside a
synchronising HIP call is not ended from Python."""
import argparse
import contextlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--points", type=int, default=131072)
ap.add_argument("--flagless-only", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
import cfnerf_amd  # noqa: E402
from cfnerf_amd import _lib as L  # noqa: E402
from cfnerf_amd.api import _network_fwd  # noqa: E402

F_INPUT_GRAD = getattr(L, "F_INPUT_GRAD", 1 << 7)


def summ(v):
    v = sorted(v)
    med = statistics.median(v)
    return {"median": med, "min": v[0], "max": v[-1], "spread_pct": 100.0 * (v[-1] - v[0]) / med}


def ab(W, K, P, launches):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        kw, _, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(netwidth=W, netdepth=8, K_samples=K, h_alpha_size=32, device=dev))
    net = kw["network_fn"].module
    net._sync()
    lib = L.lib()
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.rand(P, 90, generator=g) * 2 - 1).to(dev)
    eps = torch.randn(K, 4, generator=g).to(dev)
    d_raw = (torch.randn(P, K, 4, generator=g) / (P * K)).to(dev)
    d_ent = torch.full((1,), 0.01, device=dev)
    n = net.n_params
    x_off = (n + 63) // 64 * 64
    grad = torch.empty(x_off + P * 90, device=dev)
    net.ensure_workspace(1, P, K)
    modes = ("flagless",) if a.flagless_only else ("flagless", "input_grad")
    acc = {m: [] for m in modes}
    for i in range(2 + launches):                     # two warm-up rounds: code objects, the weight-gradient plan of this binding
        for mode in modes:
            _network_fwd(net, x, eps, K, L.F_TRAIN | L.F_STASH | (F_INPUT_GRAD if mode == "input_grad" else 0))
            gen = lib.cfnerf_model_stash_generation(net.handle)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.cfnerf_network_bwd(net.handle, gen, L.ptr(d_raw), L.ptr(d_ent), L.ptr(grad), L.stream()), "cfnerf_network_bwd")
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                acc[mode].append(e0.elapsed_time(e1))
    net.release_workspace()
    return {"W": W, "K": K, "P": P, "launches": launches, **{m: summ(v) for m, v in acc.items()}}


rows = [ab(256, 4, a.points, a.launches), ab(512, 32, a.points, a.launches)]
lib_note = os.environ.get("CFNERF_LIB") or "the in-tree build"
lines = ["# r10: cfnerf_network_bwd with and without CFNERF_F_INPUT_GRAD, one process, alternating launches, HIP events around the whole call",
         f"# (tools/ab_input_grad.py; library: {lib_note}).  Baseline: the flag-less launch of the same run.", "#"]
for r in rows:
    lines.append(f"P = {r['P']}, W = {r['W']}, K = {r['K']}  ({r['launches']} launches each)")
    for m in ("flagless", "input_grad"):
        if m in r:
            s = r[m]
            lines.append(f"  {m:10s} median {s['median']:.4f} ms   min {s['min']:.4f}   max {s['max']:.4f}   spread {s['spread_pct']:.2f} %")
    if "input_grad" in r:
        d = r["input_grad"]["median"] - r["flagless"]["median"]
        lines.append(f"  input_grad - flagless = {d:.4f} ms  ({100.0 * d / r['flagless']['median']:.2f} % of the flag-less backward)")
text = "\n".join(lines) + "\n"
print(text, end="")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
