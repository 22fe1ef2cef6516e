#!/usr/bin/env python3
"""Generate the per-netchunk latent fixtures (G23) by running the REAL reference (build container only).

Run:  python tests/golden/make_golden_netchunk.py [--out DIR]
      (writes DIR/*.npz, default tests/golden/netchunk/, and DIR/MANIFEST.json with the digest scheme of
       tests/test_oracle_golden.py::_digest; tests/test_netchunk_cpu.py holds the committed files to it and, where the
       reference exists, re-runs this script and compares every array bit for bit.)

The reference's batchify (RUN:47-64, called from run_network at RUN:82) calls NeRF_Flows.forward once per netchunk points,
and every call draws fresh latents (MOD:234,246).  These fixtures pin what a batch of several netchunks computes:

  G23a  draw order, small: W = 64, K = 4, 6 rays cut into chunk = 4 rays, netchunk = 256 points (2 rays), raw_noise_std = 1,
        perturb = 1, implicit draws under torch.manual_seed - every draw the reference consumed is recorded in order.
  G23b  C2 at full size: W = 256, K = 4, 1024 rays, netchunk = 65536 (two netchunks) with two explicit latent pairs.

Only the reference's own functions run (render -> batchify_rays -> render_rays -> run_network -> batchify -> NeRF_Flows.forward
-> raw2outputs); the loss lines come through make_golden.reference_kde_nll.  Fixtures hold data only.
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
G23B_TRAND_SEED = 2302


class RecordRandom:
    """Record every draw of the reference's three generator call sites (torch.rand RUN:524, Tensor.normal_ MOD:234,246,
    torch.randn RUN:434) while letting the real generator produce them."""

    def __init__(self):
        self.draws = []
        self._rand, self._normal, self._randn = torch.rand, torch.Tensor.normal_, torch.randn

    def __enter__(self):
        outer = self

        def rand(*a, **k):
            v = outer._rand(*a, **k)
            outer.draws.append(("rand", v.clone()))
            return v

        def normal_(t, *a, **k):
            outer._normal(t, *a, **k)
            outer.draws.append(("normal", t.clone()))
            return t

        def randn(*a, **k):
            v = outer._randn(*a, **k)
            outer.draws.append(("randn", v.clone()))
            return v
        torch.rand, torch.Tensor.normal_, torch.randn = rand, normal_, randn
        return self

    def __exit__(self, *exc):
        torch.rand, torch.Tensor.normal_, torch.randn = self._rand, self._normal, self._randn


def _grads(model):
    return {k[len("module."):]: v.grad for k, v in model.named_parameters() if v.grad is not None}


def g23a(R, tmp):
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    seed, draw_seed, n, chunk, netchunk, beta1 = 231, 2310, 6, 4, 256, 0.01
    _, kw_train, _, model, _, optimizer = build_reference_model(R, cfg, seed, tmp, K_samples=4, no_ndc=True, netchunk_per_gpu=netchunk,
                                                                raw_noise_std=1.0)
    rng = np.random.default_rng(2311)
    rays, (H, W, focal) = fern_rays(rng, n)
    rays_t = torch.tensor(rays)
    near, far = 1.2, 8.0
    target = torch.tensor(rng.uniform(0, 1, (n, 3)), dtype=torch.float32)
    torch.manual_seed(draw_seed)
    with RecordRandom() as rec:
        rgbs, disp, depth, extras = R.render(H, W, focal, chunk=chunk, rays=rays_t, near=near, far=far, verbose=False, retraw=False, **kw_train)
    loss_nll = reference_kde_nll(rgbs, target, 4)
    ent = extras["loss_entropy"]
    loss = loss_nll + beta1 * ent.mean()
    optimizer.zero_grad()
    loss.backward()
    g = dict(seed=seed, draw_seed=draw_seed, netwidth=64, K=4, H=H, W=W, focal=focal, near=near, far=far, ndc=0, chunk=chunk,
             netchunk=netchunk, raw_noise_std=1.0, perturb=1.0, beta1=beta1, rays=rays_t, target=target, rgb_map=rgbs, disp_map=disp,
             depth_map=depth, loss=loss.detach(), loss_nll=loss_nll.detach(), loss_entropy=ent.mean().detach(),
             loss_entropy_chunks=ent[::netchunk, 0, 0].detach(), draw_kinds=np.array([k for k, _ in rec.draws]))
    for i, (_, v) in enumerate(rec.draws):
        g[f"draw{i}"] = v
    for k, v in _grads(model).items():
        g["grad." + k] = v.clone()
    return g


def g23b(R, tmp):
    cfg = O.OracleCfg(netwidth=256, K_samples=4)
    seed, n, beta1 = 232, 1024, 0.01
    _, kw_train, _, model, _, optimizer = build_reference_model(R, cfg, seed, tmp, K_samples=4, no_ndc=True)
    rng = np.random.default_rng(2321)
    rays, (H, W, focal) = fern_rays(rng, n)
    rays_t = torch.tensor(rays)
    near, far = 1.2, 8.0
    target = torch.tensor(rng.uniform(0, 1, (n, 3)), dtype=torch.float32)
    t_rand_np = np.random.default_rng(G23B_TRAND_SEED).uniform(0, 1, (n, 128)).astype(np.float32)
    t_rand = torch.tensor(t_rand_np)
    pairs = [(torch.tensor(rng.standard_normal((4, 1)), dtype=torch.float32), torch.tensor(rng.standard_normal((4, 3)), dtype=torch.float32))
             for _ in range(2)]
    with ExplicitRandom(t_rand=t_rand, normals=[pairs[0][0], pairs[0][1], pairs[1][0], pairs[1][1]]) as er:
        rgbs, disp, depth, extras = R.render(H, W, focal, chunk=8192, rays=rays_t, near=near, far=far, verbose=False, retraw=False, **kw_train)
        assert not er.normals, "the reference did not draw exactly two latent pairs"
    loss_nll = reference_kde_nll(rgbs, target, 4)
    ent = extras["loss_entropy"]
    loss = loss_nll + beta1 * ent.mean()
    optimizer.zero_grad()
    loss.backward()
    g = dict(seed=seed, netwidth=256, K=4, H=H, W=W, focal=focal, near=near, far=far, ndc=0, chunk=8192, netchunk=65536, beta1=beta1,
             rays=rays_t, target=target, t_rand_seed=G23B_TRAND_SEED, t_rand_sha256=np.array(hashlib.sha256(t_rand_np.tobytes()).hexdigest()),
             eps_alpha=torch.stack([p[0] for p in pairs]), eps_rgb=torch.stack([p[1] for p in pairs]),
             rgb_map=rgbs, disp_map=disp, depth_map=depth, loss=loss.detach(), loss_nll=loss_nll.detach(), loss_entropy=ent.mean().detach(),
             loss_entropy_chunks=ent[::65536, 0, 0].detach())
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
    out_dir = os.path.join(HERE, "netchunk")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    R = import_reference()
    tmp = tempfile.mkdtemp(prefix="cfnerf_golden_nc_")
    out = {"g23a_netchunk_draw_order": g23a(R, tmp), "g23b_netchunk_c2": g23b(R, tmp)}
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
