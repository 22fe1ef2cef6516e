"""What d_z_vals and d_rays_d cost behind cfnerf_composite_bwd (CFNERF_F_SEAM_GRAD: comp_seam_zgrad_kernel as a second launch after
composite_bwd_kernel): the plain backward - the yardstick, the kernel as it was -, the backward with the request, and the request alone (a
detached raw: no d_raw), alternating in blocks on one box in one run; per-launch times from events around each call.  N = 8192 rays x 128
samples, K = 4 and K = 32, cotangents of rgb_map and depth_map.  Each figure next to its algorithmic bytes: raw read 16 B + d_raw written 16 B
per (sample, latent) for the plain backward, raw read once more (16 B) for the request.

    python tests/tools/seam_zgrad_bench.py [--reps 40] [--block 10] [--out profiles/r13_seam_zgrad_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import cfnerf_amd  # noqa: E402,F401
from cfnerf_amd import _lib as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lib = L.lib()
    N, S = 8192, 128
    lines, results = [], {}
    for K in (4, 32):
        g = torch.Generator().manual_seed(K)
        raw = torch.randn(N, S, K, 4, generator=g).to(dev)
        z = torch.sort(torch.rand(N, S, generator=g) * 4 + 2, -1).values.to(dev).contiguous()
        d = (torch.randn(N, 3, generator=g) * 0.3 + torch.tensor([0.1, -0.2, -1.0])).to(dev).contiguous()
        G, Gd = (torch.randn(N, 3, K, generator=g) / (N * K)).to(dev), (torch.randn(N, K, generator=g) / (N * K)).to(dev)
        d_raw, d_z, d_d = torch.empty_like(raw), torch.empty_like(z), torch.empty_like(d)
        both, alone = L.composite_grads(d_raw, d_z, d_d), L.composite_grads(None, d_z, d_d)
        arms = {"plain": (0, L.ptr(d_raw)), "with the request": (L.F_SEAM_GRAD, L.composite_grads_arg(both)),
                "the request alone": (L.F_SEAM_GRAD, L.composite_grads_arg(alone))}
        times = {k: [] for k in arms}

        def once(arm):
            wb, out = arms[arm]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            L.check(lib.cfnerf_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), N, S, K, wb, L.ptr(G), None, L.ptr(Gd), None, out, L.stream()), "cfnerf_composite_bwd")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)
        for arm in arms:
            for _ in range(5):
                once(arm)
        done = 0
        while done < a.reps:
            for arm in arms:
                times[arm] += [once(arm) for _ in range(a.block)]
            done += a.block
        med = {k: float(np.median(v)) for k, v in times.items()}
        pk = N * S * K
        mb = {"plain": pk * 32 / 1e6, "with the request": pk * 48 / 1e6, "the request alone": pk * 16 / 1e6}
        results[f"K{K}"] = {k: dict(ms=round(med[k], 4), mb=round(mb[k], 1), tb_per_s=round(mb[k] / med[k] / 1e3, 3)) for k in arms}
        results[f"K{K}"]["reps"] = len(times["plain"])
        lines.append(f"K = {K:3d} (N {N}, S {S}; medians of {len(times['plain'])} launches per arm in blocks of {a.block}):")
        for k in arms:
            lines.append(f"    {k:18s} {med[k]:8.4f} ms   {mb[k]:7.1f} MB   {mb[k] / med[k] / 1e3:6.3f} TB/s   {med[k] / med['plain']:5.2f} x the plain backward")
        del raw, d_raw
    text = "\n".join(lines) + "\n" + json.dumps({"tool": "seam_zgrad_bench", "results": results}) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
