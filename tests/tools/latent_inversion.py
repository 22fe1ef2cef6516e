"""Latent inversion: which of the model's hypotheses explains an observation.  A small target is rendered with a hidden latent set eps*;
starting from zeros, Adam on eps.grad ALONE (the weights are frozen: CFNERF_F_EPS_GRAD gives the latents their gradient whether or not the
network asks for one) brings the render back to the target.  Prints the loss and max |eps - eps*| every --every steps.

    python tests/tools/latent_inversion.py [--steps 400] [--lr 0.05] [--rays 64] [--K 4] [--W 64] [--out profiles/r18_latent_inversion.txt]

A tool, not a test: the recovered latents need not equal eps* where the render does not depend on them (a colour latent of a sample no ray
sees), so the loss is the figure to read and the latent distance the illustration."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cfnerf_amd  # noqa: E402
from oracle import cfnerf_oracle as O  # noqa: E402
from util_hip import build_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=25)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--seed", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_latent_inversion.txt"))
    a = ap.parse_args()
    dev = "cuda"
    cfg = O.OracleCfg(netwidth=a.W, K_samples=a.K)
    _, _, _, model, _, _ = build_model(cfg, a.seed)
    net = model.module
    net.flat.requires_grad_(False)                         # frozen weights: the latents are the only unknowns
    rng = np.random.default_rng(a.seed)
    o = rng.uniform(-0.3, 0.3, (a.rays, 3))
    d = rng.standard_normal((a.rays, 3)) * 0.3 + np.array([0.1, -0.2, -1.0])
    v = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays = torch.tensor(np.concatenate([o, d, np.full((a.rays, 1), 2.0), np.full((a.rays, 1), 6.0), v], -1), dtype=torch.float32).to(dev)
    hidden = torch.tensor(rng.standard_normal((a.K, 4)), dtype=torch.float32).to(dev)
    render = lambda ea, er: cfnerf_amd.render_rays(rays, model, None, 128, True, False, perturb=0., eps_alpha=ea, eps_rgb=er)
    with torch.no_grad():
        t = render(hidden[:, 3:4], hidden[:, 0:3])
        target = (t["rgb_map"].clone(), t["depth_map"].clone())
    ea = torch.zeros(a.K, 1, device=dev, requires_grad=True)
    er = torch.zeros(a.K, 3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([ea, er], lr=a.lr)
    lines = [f"latent inversion: W {a.W}, K {a.K}, {a.rays} rays x 128 samples, Adam lr {a.lr} on eps.grad alone from zeros, weights frozen",
             f"{'step':>6s} {'loss':>12s} {'max |eps - eps*|':>18s}"]
    for step in range(a.steps + 1):
        opt.zero_grad()
        ret = render(ea, er)
        loss = ((ret["rgb_map"] - target[0]) ** 2).mean() + ((ret["depth_map"] - target[1]) ** 2).mean()
        if step % a.every == 0:
            dist = float((torch.cat([er, ea], -1).detach() - hidden).abs().max())
            lines.append(f"{step:6d} {float(loss.detach()):12.4e} {dist:18.4f}")
        loss.backward()
        assert ea.grad is not None and er.grad is not None and net.flat.grad is None
        opt.step()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
