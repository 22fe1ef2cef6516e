#!/usr/bin/env python3
"""Generate the latent-gradient fixtures (G28) by running the REAL reference (build container only).

Run:  python tests/golden/make_golden_epsgrad.py [--out DIR]
      (writes DIR/*.npz, default tests/golden/epsgrad/, and DIR/MANIFEST.json with the digest scheme of
       tests/test_oracle_golden.py::_digest; tests/test_epsgrad_cpu.py holds the committed files to it and, where the
       reference exists, re-runs this script and compares every array bit for bit.)

In the reference the base sample ``z0 = eps.mul(std).add_(mean)`` (MOD:239,251) is an ordinary autograd line, so a latent that is a LEAF gets a
gradient: the chain through the flows, plus the direct term of the base log-normal in ``loss_entropy`` (MOD:268,283,286).  The latents reach
the reference through make_golden.ExplicitRandom unchanged - its ``self_t.copy_(v)`` is differentiable when ``v`` is a leaf.

  G28a  ``render_rays`` on 3 rays, train branch, perturb = 1 with explicit t_rand, K = 3.
        loss = sum(rgb_map G) + sum(disp_map Gq) + sum(depth_map Gd) + sum(raw Gr) + 0.3 mean(entropy),  Gr[n,s,k,c] = Gr_a[n,s] Gr_b[k,c]
        -> ``eps_alpha_grad [K,1]``, ``eps_rgb_grad [K,3]`` and the four base-Gaussian gradients.
  G28b  4 rays, ``netchunk_per_gpu = 256``: two network calls, two latent pairs; lindisp, white background; the loss of G28a
        -> the gradients of both pairs, ``[2,K,1]`` / ``[2,K,3]``, and the four base-Gaussian gradients.
  G28c  ``NeRF_Flows.forward(x [5,90])``, train branch.  loss = sum(raw Gr) + 0.3 mean(entropy) -> the latent gradients and the four
        base-Gaussian gradients.

W = 64, netdepth = 3, the reference's 128-sample table; the seed walk and the stored ReLU masks are make_golden_cotangents'.  Fixtures hold
data only.
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
from make_golden_inputgrad import C_ENT, MAX_SEED, MIN_PRE, _encoded  # noqa: E402

O = MG.O
W, DEPTH, S = 64, 3, 128
BASE = ("alpha_mean", "alpha_std", "rgb_mean", "rgb_std")


def _hooks(net, rec):
    """make_golden_inputgrad._hooks for a batch of several network calls: the pre-activations of every ReLU of MOD:168-181, one entry per call"""
    add = lambda k: (lambda m, i, o: rec.setdefault(k, []).append(o.detach().clone()))
    hs = [l.register_forward_hook(add(f"trunk{j}")) for j, l in enumerate(net.pts_linears)]
    hs.append(net.views_linears[0].register_forward_hook(add("views")))
    return hs


def _walk(R, tmp, K, run, **over):
    """make_golden_cotangents._walk, keeping the base-Gaussian gradients only: the first model seed whose smallest |pre-activation| clears
    MIN_PRE, else the one that comes closest"""
    cfg = O.OracleCfg(netwidth=W, K_samples=K, netdepth=DEPTH)
    best = None
    for seed in range(MAX_SEED):
        _, kw_train, _, model, p, _ = build_reference_model(R, cfg, seed, tmp, K_samples=K, **over)
        model.zero_grad()
        rec = {}
        hs = _hooks(model.module, rec)
        g = run(model, kw_train)
        for h in hs:
            h.remove()
        rec = {k: torch.cat(v, 0) for k, v in rec.items()}        # (in call order = point order)
        min_pre = min(float(v.abs().min()) for v in rec.values())
        if best is None or min_pre > best[0]:
            named = dict(model.module.named_parameters())
            g.update({"grad." + k: named[k].grad.detach().clone() for k in BASE})
            g.update(seed=seed, netwidth=W, netdepth=DEPTH, K=K, min_abs_pre=np.float32(min_pre))
            g.update({"mask." + k: (v > 0).to(torch.uint8) for k, v in rec.items()})
            best = (min_pre, g)
        if min_pre >= MIN_PRE:
            break
    return best[1]


def _rays(rng, n):
    o = torch.tensor(rng.uniform(-0.3, 0.3, (n, 3)), dtype=torch.float32)
    d = torch.tensor(rng.standard_normal((n, 3)) * 0.3 + np.array([0.1, -0.2, -1.0]), dtype=torch.float32)
    return torch.cat([o, d, torch.full((n, 1), 2.0), torch.full((n, 1), 6.0), d / d.norm(dim=-1, keepdim=True)], -1)


def _render_rays_case(R, tmp, data_seed, n, K, pairs, **opt):
    rng = np.random.default_rng(data_seed)
    rb = _rays(rng, n)
    rnd_t = lambda *s: torch.tensor(rng.standard_normal(s), dtype=torch.float32)
    t_rand = torch.tensor(rng.uniform(0, 1, (n, S)), dtype=torch.float32)
    ea, er = rnd_t(pairs, K, 1), rnd_t(pairs, K, 3)
    G, Gq, Gd = rnd_t(n, 3, K) / (n * K), rnd_t(n, K) / (n * K), rnd_t(n, K) / (n * K)
    Gr_a, Gr_b = rnd_t(n, S) / (n * K), rnd_t(K, 4)
    flags = {k: v for k, v in opt.items() if k in ("lindisp", "white_bkgd")}

    def run(model, kw):
        la, lr = ea.clone().requires_grad_(True), er.clone().requires_grad_(True)
        normals = [t for c in range(pairs) for t in (la[c], lr[c])]          # per network call: eps_alpha (MOD:234), then eps_rgb (MOD:246)
        with ExplicitRandom(t_rand=t_rand, normals=normals) as rnd:
            ret = R.render_rays(rb, model, kw["network_query_fn"], S, True, False, K_samples=K, perturb=1., **flags)
            assert not rnd.normals
        Gr = Gr_a[:, :, None, None] * Gr_b[None, None]
        loss = ((ret["rgb_map"] * G).sum() + (ret["disp_map"] * Gq).sum() + (ret["depth_map"] * Gd).sum() + (ret["raw"] * Gr).sum()
                + C_ENT * ret["loss_entropy"].mean())
        loss.backward()
        one = pairs == 1
        return dict(ray_batch=rb, t_rand=t_rand, eps_alpha=ea[0] if one else ea, eps_rgb=er[0] if one else er, G=G, Gq=Gq, Gd=Gd, Gr_a=Gr_a, Gr_b=Gr_b,
                    c_entropy=np.float32(C_ENT), rgb_map=ret["rgb_map"].detach(), loss_entropy=ret["loss_entropy"].mean().detach(), loss=loss.detach(),
                    eps_alpha_grad=la.grad[0].clone() if one else la.grad.clone(), eps_rgb_grad=lr.grad[0].clone() if one else lr.grad.clone())
    return _walk(R, tmp, K, run, **opt)


def g28a(R, tmp):
    return _render_rays_case(R, tmp, 2811, 3, 3, 1)


def g28b(R, tmp):
    g = _render_rays_case(R, tmp, 2821, 4, 3, 2, netchunk_per_gpu=256, lindisp=True, white_bkgd=True, no_ndc=True)
    g.update(netchunk=256)
    return g


def g28c(R, tmp):
    K, P = 4, 5
    rng = np.random.default_rng(2831)
    pts = torch.tensor(rng.uniform(-1, 1, (P, 1, 3)), dtype=torch.float32)
    dirs = torch.nn.functional.normalize(torch.tensor(rng.standard_normal((P, 3)), dtype=torch.float32), dim=-1)
    Gr = torch.tensor(rng.standard_normal((P, K, 4)), dtype=torch.float32) / (P * K)
    ea = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)

    def run(model, kw):
        la, lr = ea.clone().requires_grad_(True), er.clone().requires_grad_(True)
        x = _encoded(R, pts, dirs)
        with ExplicitRandom(normals=[la, lr]) as rnd:
            raw, ent = model(x, False, False)
            assert not rnd.normals
        loss = (raw * Gr).sum() + C_ENT * ent.mean()
        loss.backward()
        return dict(x=x.detach(), Gr=Gr, eps_alpha=ea, eps_rgb=er, c_entropy=np.float32(C_ENT), raw=raw.detach(), loss_entropy=ent.mean().detach(),
                    loss=loss.detach(), eps_alpha_grad=la.grad.clone(), eps_rgb_grad=lr.grad.clone())
    return _walk(R, tmp, K, run)


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(HERE, "epsgrad")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    R = import_reference()
    tmp = tempfile.mkdtemp(prefix="cfnerf_golden_epsgrad_")
    out = {"g28a_render_rays_eps_grad": g28a(R, tmp), "g28b_netchunk_pairs_eps_grad": g28b(R, tmp), "g28c_forward_eps_grad": g28c(R, tmp)}
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
