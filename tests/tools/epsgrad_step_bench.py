"""What the latent gradient costs: on one box in one run, the plain C2 and K64 train steps of bench.py and the same steps with
Trainer(latent_grad=True) (CFNERF_F_EPS_GRAD: tail_eps_kernel + reduce_eps_kernel in the backward, d_eps copied out), alternating in
blocks.  Two plain arms run in the same alternation: their difference is the box's own run-to-run spread, the margin any "the plain step
did not move" claim has to be read against.  Per arm: the median step time (two events around Trainer.step) and the median of every stage
(cfnerf_timing_enable mode 1: fwd, bwd_tail, bwd_data, bwd_dw, adam - as tools/ab_kernels.py reads them; the two new launches - tail_eps_kernel
beside the tail kernel and reduce_eps_kernel - sit INSIDE the bwd_tail pair, so they show in that stage, in the sum of the five stages and
in the step time; the copy of d_eps out of the gradient buffer shows in the step time alone) over --steps timed steps after --warmup.

    python tests/tools/epsgrad_step_bench.py [--steps 200] [--warmup 20] [--block 25] [--out profiles/r18_epsgrad_step.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from cfnerf_amd import train as TR  # noqa: E402

STAGES = (("fwd", 0), ("bwd_tail", 1), ("bwd_data", 2), ("bwd_dw", 3), ("adam", 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_epsgrad_step.txt"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines, results = [], {}
    for name in ("C2", "K64"):
        wl = bench.Workload(name, "train", 0, 1, dev)
        sc, n, K = wl.sc, wl.n, wl.K
        H, Wd, focal = sc["H"], sc["W"], sc["focal"]
        geo = dict(near=sc["near"], far=sc["far"], ndc=sc["ndc"], white_bkgd=sc["white_bkgd"])
        trainers = {"plain_a": wl.trainer, "plain_b": wl.trainer,
                    "latent_grad": TR.Trainer(wl.net, lrate=5e-4, lrate_decay=250, beta1=0.01, latent_grad=True)}
        gen = torch.Generator(device=dev).manual_seed(1234)

        def step(arm):
            t_rand = torch.rand(n, bench.S, device=dev)
            eps = torch.randn(K, 4, device=dev, generator=gen)
            return trainers[arm].step(H, Wd, focal, wl.rays, wl.target, t_rand=t_rand, eps=eps, **geo)

        wl.lib.cfnerf_timing_enable(wl.net.handle, 1)
        for arm in trainers:
            for _ in range(a.warmup):
                step(arm)
        torch.cuda.synchronize()
        times = {arm: {"step": [], **{k: [] for k, _ in STAGES}} for arm in trainers}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        done = 0
        while done < a.steps:
            for arm in trainers:
                for _ in range(a.block):
                    ev[0].record()
                    step(arm)
                    ev[1].record()
                    torch.cuda.synchronize()
                    times[arm]["step"].append(ev[0].elapsed_time(ev[1]))
                    for k, i in STAGES:
                        times[arm][k].append(wl.lib.cfnerf_timing_last_ms(wl.net.handle, i))
            done += a.block
        wl.lib.cfnerf_timing_enable(wl.net.handle, 0)
        med = {arm: {k: float(np.median(v)) for k, v in t.items()} for arm, t in times.items()}
        results[name] = {arm: {k: round(v, 4) for k, v in m.items()} for arm, m in med.items()}
        results[name]["steps_per_arm"] = len(times["latent_grad"]["step"])
        lines.append(f"{name}: N_rand {n}, K {K}, W {wl.W}; {len(times['latent_grad']['step'])} timed steps per arm in blocks of {a.block}, medians in ms")
        for arm in trainers:
            m = med[arm]
            lines.append(f"  {arm:11s} step {m['step']:.4f}  " + "  ".join(f"{k} {m[k]:.4f}" for k, _ in STAGES))
        spread = abs(med["plain_a"]["step"] - med["plain_b"]["step"]) / med["plain_a"]["step"]
        plain = 0.5 * (med["plain_a"]["step"] + med["plain_b"]["step"])
        kern = lambda m: sum(m[k] for k, _ in STAGES)
        lines.append(f"  same-run spread of the plain step: {100 * spread:.2f} %")
        lines.append(f"  latent_grad=True: step {med['latent_grad']['step'] - plain:+.4f} ms ({100 * (med['latent_grad']['step'] / plain - 1):+.1f} %), "
                     f"the five timed stages {100 * (kern(med['latent_grad']) / (0.5 * (kern(med['plain_a']) + kern(med['plain_b']))) - 1):+.1f} %")
        results[name]["plain_spread"] = round(spread, 5)
        results[name]["latent_grad_over_plain_step"] = round(med["latent_grad"]["step"] / plain, 4)
        wl.net.release_workspace()
        del wl, trainers
    text = "\n".join(lines) + "\n" + json.dumps({"tool": "epsgrad_step_bench", "results": results}) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
