#!/usr/bin/env python3
"""Generate the depth-supervision fixtures (G24) by running the REAL reference (build container only).

Run:  python tests/golden/make_golden_depth.py [--out DIR]
      (writes DIR/*.npz, default tests/golden/depth/, and DIR/MANIFEST.json with the digest scheme of
       tests/test_oracle_golden.py::_digest; tests/test_depth_cpu.py holds the committed files to it and, where the
       reference exists, re-runs this script and compares every array bit for bit.)

With ``colmap_depth`` the reference's train loop renders the step's colour rays and N_depth rays through COLMAP key points
in ONE render (RUN:1009-1016), takes the K-mean of the depth map, cuts everything else to the colour rays (RUN:1019-1024)
and adds ``depth_lambda * mse(depth of the key-point rays, key-point depth)`` to the loss (RUN:1052-1054).  These fixtures
pin that step:

  G24a  one network call:  W = 64, K = 4, 24 colour + 8 depth rays, netchunk 65536, beta1 0.01, depth_lambda 0.1.
  G24b  two network calls, the boundary inside the colour rays: the same model, 12 + 4 rays, netchunk 1024 (8 rays per call),
        two explicit latent pairs; ``loss_entropy`` is the FIRST call's entropy (the cut of the per-point entropy tensor to its
        first N_c rows lands inside the first call), ``loss_entropy_chunks`` holds both calls' values.
  G24c  full size: W = 256, K = 4, 1024 + 128 rays, netchunk 65536 (three calls, three pairs), depth_lambda 0.01; gradients
        stored like G23b (64 sampled entries, norm, float64 sum, abs-max per tensor; t_rand by seed + sha256).

Only the reference's own ``render`` runs; the loop lines are restated once in ``reference_depth_step`` below, beside
make_golden.reference_kde_nll (the reference's ``train()`` cannot be imported as a function).  Fixtures hold data only.
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
from make_golden import ExplicitRandom, build_reference_model, fern_rays, import_reference, reference_kde_nll, t2n  # noqa: E402

O = MG.O
G24C_TRAND_SEED = 2403
NEAR, FAR = 1.2, 8.0


def reference_depth_step(rgbs, depth, extras, target_s, target_depth, n_batch, nk, beta1, depth_lambda):
    """The loss of the reference's depth-supervised step on the outputs of ONE render of cat(colour rays, depth rays), lines
    RUN:1019-1024, 1045-1054 restated operation for operation (the KDE lines through reference_kde_nll): K-mean of the depth map,
    everything else cut to the first ``n_batch`` (colour) rays - the per-point ``loss_entropy [N*S,K,1]`` included, whose first
    ``n_batch`` rows are points of the first network call - and ``depth_lambda * mse`` on the depth rays."""
    depth = torch.mean(depth, -1)
    rgbs = rgbs[:n_batch, :]
    depth_col = depth[n_batch:]
    extras = {x: extras[x][:n_batch] for x in extras}
    loss_nll = reference_kde_nll(rgbs, target_s, nk)
    loss_entropy = extras["loss_entropy"].mean()
    loss = loss_nll + beta1 * loss_entropy if beta1 else loss_nll
    depth_loss = torch.mean((depth_col - target_depth) ** 2)
    loss = loss + depth_lambda * depth_loss
    return dict(loss=loss, loss_nll=loss_nll, loss_entropy=loss_entropy, depth_loss=depth_loss)


def _grads(model):
    return {k[len("module."):]: v.grad for k, v in model.named_parameters() if v.grad is not None}


def _case(R, tmp, *, netwidth, seed, data_seed, n_c, n_d, netchunk, beta1, depth_lambda, n_pairs, t_rand_seed=None):
    cfg = O.OracleCfg(netwidth=netwidth, K_samples=4)
    _, kw_train, _, model, _, optimizer = build_reference_model(R, cfg, seed, tmp, K_samples=4, no_ndc=True, netchunk_per_gpu=netchunk)
    rng = np.random.default_rng(data_seed)
    n = n_c + n_d
    rays, (H, W, focal) = fern_rays(rng, n)                      # rows [0, n_c): colour rays, [n_c, n): rays through key points
    rays_t = torch.tensor(rays)
    target = torch.tensor(rng.uniform(0, 1, (n_c, 3)), dtype=torch.float32)
    target_depth = torch.tensor(rng.uniform(2.0, 6.0, (n_d,)), dtype=torch.float32)
    if t_rand_seed is None:
        t_rand_np = rng.uniform(0, 1, (n, 128)).astype(np.float32)
    else:
        t_rand_np = np.random.default_rng(t_rand_seed).uniform(0, 1, (n, 128)).astype(np.float32)
    t_rand = torch.tensor(t_rand_np)
    pairs = [(torch.tensor(rng.standard_normal((4, 1)), dtype=torch.float32), torch.tensor(rng.standard_normal((4, 3)), dtype=torch.float32))
             for _ in range(n_pairs)]
    with ExplicitRandom(t_rand=t_rand, normals=[t for p in pairs for t in p]) as er:
        rgbs, disp, depth, extras = R.render(H, W, focal, chunk=8192, rays=rays_t, near=NEAR, far=FAR, verbose=False, retraw=False, **kw_train)
        assert not er.normals, f"the reference did not draw exactly {n_pairs} latent pairs"
    ent = extras["loss_entropy"]
    assert tuple(ent.shape) == (n * 128, 4, 1), tuple(ent.shape)
    L = reference_depth_step(rgbs, depth, extras, target, target_depth, n_c, 4, beta1, depth_lambda)
    optimizer.zero_grad()
    L["loss"].backward()
    g = dict(seed=seed, netwidth=netwidth, K=4, H=H, W=W, focal=focal, near=NEAR, far=FAR, ndc=0, chunk=8192, netchunk=netchunk, beta1=beta1,
             depth_lambda=depth_lambda, n_colour=n_c, n_depth=n_d, rays=rays_t, target=target, target_depth=target_depth,
             eps_alpha=torch.stack([p[0] for p in pairs]), eps_rgb=torch.stack([p[1] for p in pairs]),
             rgb_map=rgbs, disp_map=disp, depth_map=depth, loss_entropy_chunks=ent[::netchunk, 0, 0].detach(),
             loss_entropy_all_points=ent.mean().detach())
    g.update({k: v.detach() for k, v in L.items()})
    return g, model, rng, t_rand_np


def _full_gradients(g, model):
    for k, v in _grads(model).items():
        g["grad." + k] = v.clone()
    return g


def g24a(R, tmp):
    g, model, _, t_rand = _case(R, tmp, netwidth=64, seed=241, data_seed=2411, n_c=24, n_d=8, netchunk=65536, beta1=0.01, depth_lambda=0.1,
                                n_pairs=1)
    g["t_rand"] = t_rand
    return _full_gradients(g, model)


def g24b(R, tmp):
    g, model, _, t_rand = _case(R, tmp, netwidth=64, seed=241, data_seed=2421, n_c=12, n_d=4, netchunk=1024, beta1=0.01, depth_lambda=0.1,
                                n_pairs=2)
    g["t_rand"] = t_rand
    return _full_gradients(g, model)


def g24c(R, tmp):
    g, model, rng, t_rand = _case(R, tmp, netwidth=256, seed=243, data_seed=2431, n_c=1024, n_d=128, netchunk=65536, beta1=0.01,
                                  depth_lambda=0.01, n_pairs=3, t_rand_seed=G24C_TRAND_SEED)
    g["t_rand_seed"] = G24C_TRAND_SEED
    g["t_rand_sha256"] = np.array(hashlib.sha256(t_rand.tobytes()).hexdigest())
    for k, v in _grads(model).items():
        gf = v.reshape(-1)
        idx = np.sort(rng.choice(gf.numel(), size=min(64, gf.numel()), replace=False))
        g["gradidx." + k] = idx
        g["gradsample." + k] = gf[torch.tensor(idx)].clone()
        g["gradnorm." + k] = gf.double().norm()
        g["gradsum." + k] = gf.double().sum()
        g["gradabsmax." + k] = gf.abs().max()
    return g


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(HERE, "depth")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    R = import_reference()
    tmp = tempfile.mkdtemp(prefix="cfnerf_golden_depth_")
    out = {"g24a_depth_one_call": g24a(R, tmp), "g24b_depth_two_calls": g24b(R, tmp), "g24c_depth_c2": g24c(R, tmp)}
    manifest = {}
    for name, d in out.items():
        arrays = t2n(d)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **arrays)
        manifest[name] = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))
                          for k, v in sorted(arrays.items())}
        print(f"{name}: {os.path.getsize(path)/1024:.1f} KiB")
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as f:
        json.dump(manifest, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
