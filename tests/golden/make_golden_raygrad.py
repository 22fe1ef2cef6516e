#!/usr/bin/env python3
"""Generate the ray-gradient fixtures (G26) by running the REAL reference (build container only).

Run:  python tests/golden/make_golden_raygrad.py [--out DIR]
      (writes DIR/*.npz, default tests/golden/raygrad/, and DIR/MANIFEST.json with the digest scheme of
       tests/test_oracle_golden.py::_digest; tests/test_raygrad_cpu.py holds the committed files to it and, where the
       reference exists, re-runs this script and compares every array bit for bit.)

The reference's ``render()`` (RUN:103-170) is ONE autograd graph from ``c2w`` / ``rays_o`` / ``rays_d`` to the loss: pose refinement and
image registration differentiate it.  These fixtures pin that gradient, loss = sum(rgb_map G) + sum(depth_map Gd) + 0.3 mean(entropy):

  G26a  ``render_rays`` on a leaf ``ray_batch [3,11]``, train branch, perturb = 1 with explicit t_rand -> ``rays_grad [3,11]`` (all 11 columns:
        near / far reach the loss through the sampling lines RUN:510-532).
  G26b  ``render(rays=(o, d))``, leaves [4,3], ndc=True, near 0 / far 1 -> ``rays_o_grad``, ``rays_d_grad``.
  G26c  ``render(c2w=leaf [3,4])``, H = W = 4, ndc=False, lindisp=True, white_bkgd=True, near 2 / far 6 -> ``c2w_grad``.

W = 64, K = 4, the reference's 128-sample table, explicit latents through make_golden.ExplicitRandom.  The seed walk and the stored ReLU masks
are make_golden_inputgrad's: the model seed of a case is the FIRST one, walking up from 0, at which the smallest |pre-activation| is
>= MIN_PRE - and where no seed below MAX_SEED gets there (see _walk) the one that comes closest; ``min_abs_pre`` says how close.
Fixtures hold data only.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import torch  # noqa: E402

import make_golden as MG  # noqa: E402
from make_golden import ExplicitRandom, build_reference_model, import_reference, t2n  # noqa: E402
from make_golden_inputgrad import C_ENT, MAX_SEED, MIN_PRE, K, W, _hooks  # noqa: E402

O = MG.O
S = 128


def _walk(R, tmp, run, **over):
    """run(model, kw_train) -> fixture dict of the walk's model seed: the FIRST seed below MAX_SEED whose smallest |pre-activation| clears
    MIN_PRE, else - a ray fixture has 384 .. 2048 points x 544 ReLU units, and no seed keeps ALL of them 2e-5 from zero - the seed with the
    LARGEST smallest |pre-activation| (ties: the lowest seed)"""
    cfg = O.OracleCfg(netwidth=W, K_samples=K)
    best = None
    for seed in range(MAX_SEED):
        _, kw_train, _, model, _, _ = build_reference_model(R, cfg, seed, tmp, K_samples=K, **over)
        rec = {}
        hs = _hooks(model.module, rec)
        g = run(model, kw_train)
        for h in hs:
            h.remove()
        min_pre = min(float(v.abs().min()) for v in rec.values())
        if best is None or min_pre > best[0]:
            g.update(seed=seed, netwidth=W, K=K, min_abs_pre=np.float32(min_pre), c_entropy=np.float32(C_ENT))
            g.update({"mask." + k: (v > 0).to(torch.uint8) for k, v in rec.items()})
            best = (min_pre, g)
        if min_pre >= MIN_PRE:
            break
    return best[1]


def _draws(rng, n):
    t_rand = torch.tensor(rng.uniform(0, 1, (n, S)), dtype=torch.float32)
    ea = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)
    G = torch.tensor(rng.standard_normal((n, 3, K)), dtype=torch.float32) / (n * K)
    Gd = torch.tensor(rng.standard_normal((n, K)), dtype=torch.float32) / (n * K)
    return t_rand, ea, er, G, Gd


def _world_rays(rng, n):
    o = rng.uniform(-0.3, 0.3, (n, 3))
    d = rng.standard_normal((n, 3)) * 0.3 + np.array([0.1, -0.2, -1.0])
    return torch.tensor(o, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)


def _loss(rgb, depth, ent, G, Gd):
    return (rgb * G.reshape(rgb.shape)).sum() + (depth * Gd.reshape(depth.shape)).sum() + C_ENT * ent.mean()


def g26a(R, tmp):
    rng = np.random.default_rng(2611)
    o, d = _world_rays(rng, 3)
    v = d / d.norm(dim=-1, keepdim=True)
    rb0 = torch.cat([o, d, torch.full((3, 1), 2.0), torch.full((3, 1), 6.0), v], -1)
    t_rand, ea, er, G, Gd = _draws(rng, 3)

    def run(model, kw):
        rb = rb0.clone().requires_grad_(True)
        with ExplicitRandom(t_rand=t_rand, normals=[ea, er]) as rnd:
            ret = R.render_rays(rb, model, kw["network_query_fn"], S, True, False, K_samples=K, perturb=1.)
            assert not rnd.normals
        _loss(ret["rgb_map"], ret["depth_map"], ret["loss_entropy"], G, Gd).backward()
        return dict(ray_batch=rb0, t_rand=t_rand, eps_alpha=ea, eps_rgb=er, G=G, Gd=Gd, rgb_map=ret["rgb_map"].detach(),
                    depth_map=ret["depth_map"].detach(), loss_entropy=ret["loss_entropy"].mean().detach(), rays_grad=rb.grad.clone())
    return _walk(R, tmp, run)


def g26b(R, tmp):
    rng = np.random.default_rng(2621)
    rays, (H, Wd, focal) = MG.fern_rays(rng, 4)
    o0, d0 = torch.tensor(rays[0]), torch.tensor(rays[1])
    t_rand, ea, er, G, Gd = _draws(rng, 4)

    def run(model, kw):
        o, d = o0.clone().requires_grad_(True), d0.clone().requires_grad_(True)
        with ExplicitRandom(t_rand=t_rand, normals=[ea, er]) as rnd:
            rgb, disp, depth, ex = R.render(H, Wd, focal, chunk=8192, rays=(o, d), ndc=True, near=0., far=1., **kw)
            assert not rnd.normals
        _loss(rgb, depth, ex["loss_entropy"], G, Gd).backward()
        return dict(H=H, W=Wd, focal=np.float32(focal), rays_o=o0, rays_d=d0, t_rand=t_rand, eps_alpha=ea, eps_rgb=er, G=G, Gd=Gd,
                    rgb_map=rgb.detach(), depth_map=depth.detach(), loss_entropy=ex["loss_entropy"].mean().detach(),
                    rays_o_grad=o.grad.clone(), rays_d_grad=d.grad.clone())
    return _walk(R, tmp, run)


def g26c(R, tmp):
    rng = np.random.default_rng(2631)
    H = Wd = 4
    focal = 3.7
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    c2w0 = torch.tensor(np.concatenate([rot, rng.uniform(-0.3, 0.3, (3, 1))], -1), dtype=torch.float32)
    t_rand, ea, er, G, Gd = _draws(rng, H * Wd)

    def run(model, kw):
        c2w = c2w0.clone().requires_grad_(True)
        with ExplicitRandom(t_rand=t_rand, normals=[ea, er]) as rnd:
            rgb, disp, depth, ex = R.render(H, Wd, focal, chunk=8192, c2w=c2w, near=2., far=6., **kw)
            assert not rnd.normals
        _loss(rgb, depth, ex["loss_entropy"], G, Gd).backward()
        return dict(H=H, W=Wd, focal=np.float32(focal), c2w=c2w0, t_rand=t_rand, eps_alpha=ea, eps_rgb=er, G=G, Gd=Gd,
                    rgb_map=rgb.detach().reshape(H * Wd, 3, K), depth_map=depth.detach().reshape(H * Wd, K),
                    loss_entropy=ex["loss_entropy"].mean().detach(), c2w_grad=c2w.grad.clone())
    return _walk(R, tmp, run, no_ndc=True, lindisp=True, white_bkgd=True)


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(HERE, "raygrad")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    R = import_reference()
    tmp = tempfile.mkdtemp(prefix="cfnerf_golden_raygrad_")
    out = {"g26a_render_rays_rays_grad": g26a(R, tmp), "g26b_render_rays_od_grad": g26b(R, tmp), "g26c_render_c2w_grad": g26c(R, tmp)}
    manifest = {}
    for name, d in out.items():
        arrays = t2n(d)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        manifest[name] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))
                          for k, v in sorted(arrays.items())}
        print(f"{name}: seed {int(d['seed'])}, min |pre-activation| {float(d['min_abs_pre']):.2e}, {os.path.getsize(path)/1024:.1f} KiB")
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
