"""Evaluation through an occupancy grid (CFNERF_F_CULL) against the dense eval render, on the procedural stand-in scene (a tool, not a test).

Trains the synthetic scene as tests/tools/psnr_procedural.py does (K = 32 and K = 4), builds occupancy grids at a few threshold / res /
dilate settings and, for ONE 800 x 800 view per K, reports

  * the occupied-cell fraction and the kept-sample fraction,
  * the wall time of the dense ``render_uncertainty`` (device events around the call, median of the repeats after a warm-up),
  * the culled path split into cull / embed / network / composite (device events per stage, summed over the ray chunks) and the
    synchronising copy of the kept count (host clock), plus its wall time as ``render_uncertainty(occupancy=)`` runs it,
  * the same with an all-ones grid: the overhead of the route by itself,
  * mean and maximum absolute difference to the dense image in rgb_mean and depth_mean, and the PSNR of both against ground truth.

    python tests/tools/culled_eval_bench.py [--steps 1500] [--size 800] [--repeats 5] [--ks 32,4] [--grids all | all-ones]

--grids all-ones: the all-ones grid alone (an A/B of the route's own kernels, e.g. the sparse composite of two builds)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np, torch
import cfnerf_amd
from cfnerf_amd import api as A, evaluate as E, train as TR
from oracle import cfnerf_oracle as O            # deterministic weight generator only
from util_hip import build_model
import procedural_scene as PS

DEV = "cuda"
BOX_LO, BOX_HI = (-3.5, -3.5, -3.5), (3.5, 3.5, 3.5)          # holds every sample of the view (camera at radius 4, far = 6): nothing is "outside"


def train(K, steps, N_rand=1024):
    poses, images, i_train, _ = PS.make(DEV)
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    torch.manual_seed(0)
    _, _, _, model, _, _ = build_model(cfg, 0, no_ndc=True)
    net = model.module
    net.reset_parameters()
    pool = cfnerf_amd.RayPool(images, poses, PS.H, PS.W, PS.FOCAL, i_train, N_rand, generator=torch.Generator(device=DEV).manual_seed(1))
    tr = TR.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01)
    g = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(steps):
        rays, target = pool.next_batch()
        tr.step(PS.H, PS.W, PS.FOCAL, rays, target.contiguous(), t_rand=torch.rand(N_rand, 128, device=DEV, generator=g),
                eps=torch.randn(K, 4, device=DEV, generator=g), near=PS.NEAR, far=PS.FAR, ndc=False)
    torch.cuda.synchronize()
    return model, net, float(tr.scalars[3])


@torch.no_grad()
def truth(c2w, size, focal, n_quad=512, rows_per=8):
    """the scene's ground truth at size x size: the quadrature of procedural_scene.render_truth on this view's rays"""
    sc = PS.blobs(np.random.default_rng(7), DEV)
    out = []
    for r0 in range(0, size, rows_per):
        n = min(rows_per, size - r0) * size
        packed = A._pack_rays(size, size, focal, c2w=c2w, n=n, pixel0=r0 * size, ndc=False, near=PS.NEAR, far=PS.FAR, device=torch.device(DEV))
        ro, rd = packed[:, 0:3].double(), packed[:, 3:6].double()
        t = torch.linspace(PS.NEAR, PS.FAR, n_quad, dtype=torch.float64, device=DEV)
        pts = ro[:, None, :] + rd[:, None, :] * t[None, :, None]
        d2 = ((pts[:, :, None, :] - sc["c"][None, None]) ** 2).sum(-1)
        dens = sc["a"] * torch.exp(-d2 / (2 * sc["s"] ** 2))
        sigma = dens.sum(-1)
        col = (dens[..., None] * sc["col"]).sum(-2) / (sigma[..., None] + 1e-12)
        alpha = 1 - torch.exp(-sigma * (t[1] - t[0]) * rd.norm(dim=-1, keepdim=True))
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], -1), -1)[:, :-1]
        out.append(((alpha * T)[..., None] * col).sum(1).float())
    return torch.cat(out).reshape(size, size, 3)


def timed(fn, repeats):
    """median over `repeats` of the device time (ms) of fn() between two events, after one warm-up call; also its last result"""
    res = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); res = fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), res


@torch.no_grad()
def staged(model, net, grid, packed, tv, repeats):
    """the steps of api.render_rays_culled per chunk of rays with an event pair around each: medians (ms) of the per-image sums"""
    ic, icv, K = net.input_ch, net.input_ch_views, net.K_samples
    runs = []
    for rep in range(repeats + 1):
        ev, copy_ms, kept = {k: [] for k in ("cull", "embed", "network", "composite")}, 0.0, 0

        def stage(name, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); r = fn(); e1.record()
            ev[name].append((e0, e1))
            return r

        for i in range(0, packed.shape[0], E._CULL_RAY_CHUNK):
            rays = packed[i:i + E._CULL_RAY_CHUNK].contiguous()
            z, slot, ray_start, pts_c, ray_of = stage("cull", lambda: A._cull_launch(rays, grid, tv))
            t0 = time.perf_counter()
            n = int(ray_start[-1].item())
            copy_ms += (time.perf_counter() - t0) * 1e3            # (host clock: the wait for the cull launches is in it)
            kept += n
            if n:
                def embed():
                    x = torch.empty(n, ic + icv, device=DEV)
                    x[:, :ic] = A._embed_fwd(pts_c[:n], (ic - 3) // 6, ic)
                    x[:, ic:] = A._embed_fwd(rays[:, 8:11].contiguous(), (icv - 3) // 6, icv)[ray_of[:n].long()]
                    return x
                x = stage("embed", embed)
                raw_c = stage("network", lambda: model(x, False, True)[0])
            else:
                raw_c = torch.empty(0, K, 4, device=DEV)
            stage("composite", lambda: A.raw2outputs_sparse(raw_c, slot, ray_start, z, rays[:, 3:6].contiguous()))
        torch.cuda.synchronize()
        if rep:                                                    # (the first pass is the warm-up)
            runs.append({**{k: sum(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}, "count_copy_host": copy_ms})
    return {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}, kept


def psnr(img, gt):
    return round(float(-10 * torch.log10(torch.mean((img - gt) ** 2))), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="32,4")
    ap.add_argument("--grids", default="all", choices=("all", "all-ones"))
    a = ap.parse_args()
    size, focal = a.size, PS.FOCAL * a.size / PS.H               # the scene's vertical field of view at size x size
    c2w = PS.pose_spherical(10.0, -25.0, 4.0)                    # a view between the training poses
    gt = truth(c2w, size, focal)
    kw = dict(near=PS.NEAR, far=PS.FAR, ndc=False)
    for K in (int(k) for k in a.ks.split(",")):
        model, net, train_psnr = train(K, a.steps)
        tv = A.t_vals_table(net.device)
        S = tv.shape[0]
        dense_ms, dense = timed(lambda: E.render_uncertainty(size, size, focal, c2w, model, **kw), a.repeats)
        print(json.dumps({"K": K, "image": [size, size], "S": S, "train_steps": a.steps, "train_psnr_last_batch": round(train_psnr, 2),
                          "dense_render_uncertainty_ms": round(dense_ms, 2), "dense_psnr": psnr(dense["rgb_mean"], gt)}), flush=True)
        packed = A._pack_rays(size, size, focal, c2w=c2w, n=size * size, ndc=False, near=PS.NEAR, far=PS.FAR, device=net.device)
        settings = [("all-ones", None, 1, 0)] + [("network", th, res, dil) for th, res, dil in ((0.5, 64, 1), (0.05, 64, 1), (0.05, 128, 1), (0.01, 128, 2))]
        for kind, th, res, dil in settings[:1] if a.grids == "all-ones" else settings:
            if kind == "all-ones":
                grid, build_ms = E.OccupancyGrid.from_mask(torch.ones(1, 1, 1, dtype=torch.bool), BOX_LO, BOX_HI), 0.0      # the route's overhead by itself
            else:
                t0 = time.perf_counter()
                grid = E.OccupancyGrid.from_network(model, BOX_LO, BOX_HI, (res,) * 3, th, dilate=dil)
                torch.cuda.synchronize()
                build_ms = (time.perf_counter() - t0) * 1e3
            wall_ms, out = timed(lambda: E.render_uncertainty(size, size, focal, c2w, model, occupancy=grid, **kw), a.repeats)
            stages, kept = staged(model, net, grid, packed, tv, a.repeats)
            d_rgb, d_depth = (out["rgb_mean"] - dense["rgb_mean"]).abs(), (out["depth_mean"] - dense["depth_mean"]).abs()
            print(json.dumps({"K": K, "grid": kind, "threshold": th, "res": grid.res[0], "dilate": dil, "grid_build_ms": round(build_ms, 1),
                              "occupied_cells": round(grid.fraction, 4), "kept_samples": round(out["kept_samples"] / (size * size * S), 4),
                              "culled_render_uncertainty_ms": round(wall_ms, 2), "vs_dense": round(wall_ms / dense_ms, 3),
                              "stages_ms": stages, "rgb_mean_absdiff_mean_max": [float(f"{d_rgb.mean():.3g}"), float(f"{d_rgb.max():.3g}")],
                              "depth_mean_absdiff_mean_max": [float(f"{d_depth.mean():.3g}"), float(f"{d_depth.max():.3g}")],
                              "culled_psnr": psnr(out["rgb_mean"], gt)}), flush=True)
        del model, net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
