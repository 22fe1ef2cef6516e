"""Does sampling through an occupancy grid earn its keep?  (A tool, not a test; needs the GPU.)

The procedural stand-in scene has density everywhere, so this tool builds a variant with real empty space: the same procedural radiance
(tools/procedural_scene.py: Gaussian blobs) with ZERO density outside a ball of radius 0.5, seen from the same 20 poses (near 2, far 6),
inside a [-1.5, 1.5]^3 box.  Four runs of C2-sized batches (1024 rays, K = 4, W = 256) from the same initial weights, batches and latents:

    plain S = 128 (the reference's sample table) | plain S = 64 | warped S = 64, the analytic ball as the grid |
    warped S = 64, the grid taken from the network at step 500 (plain S = 64 until then)

and for each the held-out PSNR (3 views; evaluated the way it was trained, and on the plain 128-sample table) and the median step time
(device events around every step).  Separately, with every library stage timed (cfnerf_timing_enable(m, 1)), the warp's own cost per step:
what a step takes beyond its library stages with and without the warp, and the warp call alone.

    python tests/tools/warped_sampling_bench.py [steps=2000] [grid_res=64] [bins=512] [threshold=0.5]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import cfnerf_amd
import procedural_scene as PS
from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O            # deterministic weight generator only
from util_hip import build_model

DEV = "cuda"
H, W, FOCAL, NEAR, FAR = PS.H, PS.W, PS.FOCAL, PS.NEAR, PS.FAR
RADIUS, BOX = 0.5, 1.5
N_RAND, K = 1024, 4


@torch.no_grad()
def render_truth(sc, c2w, n_quad=512):
    """PS.render_truth with the density cut to zero outside the ball |p| <= RADIUS (dense fp64 quadrature; data generation only)"""
    ro, rd = PS.camera_rays(c2w, DEV)
    ro, rd = ro.double(), rd.double()
    t = torch.linspace(NEAR, FAR, n_quad, dtype=torch.float64, device=DEV)
    pts = ro[:, None, :] + rd[:, None, :] * t[None, :, None]
    d2 = ((pts[:, :, None, :] - sc["c"][None, None]) ** 2).sum(-1)
    dens = sc["a"] * torch.exp(-d2 / (2 * sc["s"] ** 2)) * (pts.norm(dim=-1) <= RADIUS)[..., None]
    sigma = dens.sum(-1)
    col = (dens[..., None] * sc["col"]).sum(-2) / (sigma[..., None] + 1e-12)
    delta = (t[1] - t[0]) * rd.norm(dim=-1, keepdim=True)
    alpha = 1 - torch.exp(-sigma * delta)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], -1), -1)[:, :-1]
    return ((alpha * T)[..., None] * col).sum(1).reshape(H, W, 3).float()


def ball_grid(res):
    """cells of the box that touch the ball: the nearest point of the cell to the origin is within RADIUS"""
    h = BOX / res
    c = (torch.arange(res, dtype=torch.float64) + 0.5) * (2 * h) - BOX
    near = (c.abs() - h).clamp_min(0.)
    d2 = near[:, None, None] ** 2 + near[None, :, None] ** 2 + near[None, None, :] ** 2
    return E.OccupancyGrid.from_mask(d2 <= RADIUS ** 2, (-BOX,) * 3, (BOX,) * 3)


def psnr(model, poses, images, idx, t_vals, sampler):
    ps, occ = [], []
    for v in idx:
        out = E.render_uncertainty(H, W, FOCAL, poses[v], model, near=NEAR, far=FAR, ndc=False, t_vals=t_vals, occupancy=sampler)
        ps.append(float(-10 * torch.log10(torch.mean((out["rgb_mean"] - images[v].to(DEV)) ** 2))))
        if sampler is not None:
            occ.append(float(out["occupied_bins"]))
    return float(np.mean(ps)), (float(np.mean(occ)) if occ else None)


def fresh_model():
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    torch.manual_seed(0)
    _, _, _, model, _, _ = build_model(cfg, 0, no_ndc=True)
    model.module.reset_parameters()
    return model


def run(name, steps, S, images, poses, i_train, i_test, sampler=None, grid_at=None, grid_kw=None, bins=512):
    model = fresh_model()
    net = model.module
    pool = cfnerf_amd.RayPool(images, poses, H, W, FOCAL, i_train, N_RAND, generator=torch.Generator(device=DEV).manual_seed(1))
    tr = TR.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01)
    g = torch.Generator(device=DEV).manual_seed(2)
    t_vals = None if S == 128 else torch.linspace(0., 1., S, device=DEV)
    ev = []
    for it in range(1, steps + 1):
        if grid_at is not None and it == grid_at + 1:
            sampler = E.OccupancyGrid.from_network(model, **grid_kw).sampler(bins=bins)
        rays, target = pool.next_batch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tr.step(H, W, FOCAL, rays, target.contiguous(), t_rand=torch.rand(N_RAND, S, device=DEV, generator=g),
                eps=torch.randn(K, 4, device=DEV, generator=g), near=NEAR, far=FAR, ndc=False, t_vals=t_vals, occupancy=sampler)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev[steps // 4:]]               # (past the warm-up and, in the fourth run, past the plain steps)
    own, occ = psnr(model, poses, images, i_test, t_vals, sampler)
    on128, _ = psnr(model, poses, images, i_test, None, None)
    r = {"run": name, "S": S, "steps": steps, "held_out_psnr": round(own, 3), "held_out_psnr_plain_128_eval": round(on128, 3),
         "step_ms_median": round(float(np.median(ms)), 4), "step_ms_p10": round(float(np.percentile(ms, 10)), 4),
         "train_psnr_last_batch": round(float(tr.scalars[3]), 3), "occupied_bins_eval": occ,
         "grid_fraction": None if sampler is None else round(sampler.grid.fraction, 5)}
    print(json.dumps(r), flush=True)
    return r, model, sampler


def warp_cost(model, sampler, images, poses, i_train, S=64, steps=300):
    """with every library stage timed: what a step takes beyond its stages, plain and warped, and the warp call alone"""
    net, lib = model.module, L.lib()
    pool = cfnerf_amd.RayPool(images, poses, H, W, FOCAL, i_train, N_RAND, generator=torch.Generator(device=DEV).manual_seed(3))
    tr = TR.Trainer(net, lrate=0.0, beta1=0.01)
    g = torch.Generator(device=DEV).manual_seed(4)
    t_vals = torch.linspace(0., 1., S, device=DEV)
    L.check(lib.cfnerf_timing_enable(net.handle, 1), "cfnerf_timing_enable")
    out = {}
    try:
        for arm, occ in (("plain", None), ("warped", sampler), ("plain_again", None)):
            wall, stages = [], []
            for it in range(steps):
                rays, target = pool.next_batch()
                t_rand, eps = torch.rand(N_RAND, S, device=DEV, generator=g), torch.randn(K, 4, device=DEV, generator=g)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.step(H, W, FOCAL, rays, target.contiguous(), t_rand=t_rand, eps=eps, near=NEAR, far=FAR, ndc=False, t_vals=t_vals, occupancy=occ)
                e1.record()
                e1.synchronize()
                if it >= steps // 3:
                    wall.append(e0.elapsed_time(e1))
                    stages.append(sum(lib.cfnerf_timing_last_ms(net.handle, i) for i in range(5)))
            out[arm] = {"step_ms_median": round(float(np.median(wall)), 4), "library_stages_ms_median": round(float(np.median(stages)), 4),
                        "beyond_stages_ms_median": round(float(np.median(np.array(wall) - np.array(stages))), 4)}
    finally:
        L.check(lib.cfnerf_timing_enable(net.handle, 0), "cfnerf_timing_enable")
    packed, alone = tr.packed, []
    t_rand = torch.rand(N_RAND, S, device=DEV, generator=g)
    for it in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        A.warp_z_vals(packed, sampler, t_vals, t_rand, False)
        e1.record()
        e1.synchronize()
        if it >= steps // 3:
            alone.append(e0.elapsed_time(e1))
    out["warp_call_alone_ms_median"] = round(float(np.median(alone)), 4)
    out["warp_cost_ms_per_step"] = round(out["warped"]["step_ms_median"] - 0.5 * (out["plain"]["step_ms_median"] + out["plain_again"]["step_ms_median"]), 4)
    out["note"] = "synchronised per step (stage timers are read back): launch gaps are exposed in every arm alike"
    print(json.dumps({"warp_cost": out, "bins": sampler.bins, "N_rand": N_RAND, "S": S}), flush=True)
    return out


def main(steps=2000, res=64, bins=512, threshold=0.5):
    sc = PS.blobs(np.random.default_rng(7), DEV)
    poses = torch.stack([PS.pose_spherical(th, -20.0 - 10.0 * (i % 3), 4.0) for i, th in enumerate(np.linspace(-60, 60, 20))])
    images = torch.stack([render_truth(sc, p) for p in poses]).cpu()
    i_test = list(PS.I_TEST)
    i_train = [i for i in range(20) if i not in i_test]
    print(json.dumps({"scene": "procedural blobs cut to a ball of radius 0.5 in a [-1.5, 1.5]^3 box", "image": [H, W], "N_rand": N_RAND, "K": K, "W": 256,
                      "grid_res": res, "bins": bins, "pad": 1, "threshold": threshold,
                      "lit_pixels": round(float((images.sum(-1) > 1e-3).float().mean()), 4)}), flush=True)
    ball = ball_grid(res)
    common = (images, poses, i_train, i_test)
    run("plain S=128", steps, 128, *common)
    run("plain S=64", steps, 64, *common)
    _, model, sampler = run("warped S=64, analytic ball", steps, 64, *common, sampler=ball.sampler(bins=bins), bins=bins)
    run(f"warped S=64, from_network at step {steps // 4}", steps, 64, *common, grid_at=steps // 4, bins=bins,
        grid_kw=dict(lo=(-BOX,) * 3, hi=(BOX,) * 3, res=(res,) * 3, threshold=threshold, dilate=1))
    warp_cost(model, sampler, images, poses, i_train)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 2000, int(a[1]) if len(a) > 1 else 64, int(a[2]) if len(a) > 2 else 512, float(a[3]) if len(a) > 3 else 0.5)
