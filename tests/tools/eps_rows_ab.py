"""Same-box A/B of the per-netchunk latent mode: the default one-set launch (flag off) against Trainer(latent_draws="netchunk")
(CFNERF_F_EPS_ROWS, one latent row per ray), alternating in blocks, at C2 (1024 rays) and N_rand 8192, W = 256, K = 4.
Medians of the fused forward and of the backward (tail + backward-data + weight gradients) from the library's HIP events
(cfnerf_timing_enable mode 1), over >= 200 timed steps per arm after a warm-up.  Prints one line per (config, arm) and a JSON line.

    python tests/tools/eps_rows_ab.py [--steps 200] [--warmup 20] [--block 25]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cfnerf_amd import _lib as L  # noqa: E402
from cfnerf_amd import api  # noqa: E402
from cfnerf_amd import train as TR  # noqa: E402
from oracle import cfnerf_oracle as O  # noqa: E402
from util_hip import build_model, fern_rays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    a = ap.parse_args()
    K = 4
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    _, _, _, model, _, _ = build_model(cfg, 1)
    net = model.module
    lib = L.lib()
    out = {}
    for name, N in (("C2", 1024), ("N8192", 8192)):
        rng = np.random.default_rng(N)
        rays, (H, W, focal) = fern_rays(rng, N)
        rays = rays.cuda()
        target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32).cuda()
        t_rand = torch.tensor(rng.uniform(0, 1, (N, 128)), dtype=torch.float32).cuda()
        eps = torch.tensor(rng.standard_normal((K, 4)), dtype=torch.float32).cuda()
        C = api.netchunk_count(N, 128, 65536, 1024 * 32)
        chunks = torch.tensor(rng.standard_normal((C, K, 4)), dtype=torch.float32)
        arms = {"flag_off": (TR.Trainer(net, beta1=0.01), dict(eps=eps)),
                "netchunk_rows": (TR.Trainer(net, beta1=0.01, latent_draws="netchunk"), dict(eps_chunks=chunks))}
        times = {k: {"fwd": [], "bwd": []} for k in arms}
        L.check(lib.cfnerf_timing_enable(net.handle, 1), "cfnerf_timing_enable")
        for k, (tr, kw) in arms.items():
            for _ in range(a.warmup):
                tr.forward_backward(H, W, focal, rays, target, t_rand=t_rand, **kw)
        torch.cuda.synchronize()
        done = 0
        while done < a.steps:
            for k, (tr, kw) in arms.items():
                for _ in range(a.block):
                    tr.forward_backward(H, W, focal, rays, target, t_rand=t_rand, **kw)
                    times[k]["fwd"].append(lib.cfnerf_timing_last_ms(net.handle, 0))
                    times[k]["bwd"].append(sum(lib.cfnerf_timing_last_ms(net.handle, i) for i in (1, 2, 3)))
            done += a.block
        L.check(lib.cfnerf_timing_enable(net.handle, 0), "cfnerf_timing_enable")
        out[name] = {}
        for k in arms:
            f, b = np.array(times[k]["fwd"]), np.array(times[k]["bwd"])
            out[name][k] = {"fwd_ms_median": round(float(np.median(f)), 4), "bwd_ms_median": round(float(np.median(b)), 4),
                            "fwd_ms_p10_p90": [round(float(np.percentile(f, 10)), 4), round(float(np.percentile(f, 90)), 4)],
                            "bwd_ms_p10_p90": [round(float(np.percentile(b, 10)), 4), round(float(np.percentile(b, 90)), 4)], "steps": len(f)}
            print(f"{name:6s} {k:14s} fwd {out[name][k]['fwd_ms_median']:.4f} ms  bwd {out[name][k]['bwd_ms_median']:.4f} ms  "
                  f"(p10/p90 fwd {out[name][k]['fwd_ms_p10_p90']}, bwd {out[name][k]['bwd_ms_p10_p90']}; {len(f)} steps)", flush=True)
        net.release_workspace()
    print(json.dumps({"tool": "eps_rows_ab", "W": 256, "K": K, "results": out}))


if __name__ == "__main__":
    main()
