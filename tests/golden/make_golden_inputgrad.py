#!/usr/bin/env python3
"""Generate the input-gradient fixtures (G25) by running the REAL reference (build container only).

Run:  python tests/golden/make_golden_inputgrad.py [--out DIR]
      (writes DIR/*.npz, default tests/golden/inputgrad/, and DIR/MANIFEST.json with the digest scheme of
       tests/test_oracle_golden.py::_digest; tests/test_inputgrad_cpu.py holds the committed files to it and, where the
       reference exists, re-runs this script and compares every array bit for bit.)

In the reference ``NeRF_Flows.forward`` (MOD:188-291) and ``Embedder.embed`` (HLP:21-69) are autograd graphs in their INPUTS too, so a
caller's ``network_query_fn`` can put something learnable in front of the network.  These fixtures pin that gradient:

  G25a  train branch: ``NeRF_Flows.forward(x)`` on 8 pre-embedded points, loss = sum(raw G) + 0.3 mean(entropy) -> ``x_grad [8,90]``.
  G25b  the reference's ``run_network(pts [2,4,3], viewdirs [2,3], ...)`` with the same loss -> ``pts_grad``, ``viewdirs_grad``
        (the embedder's adjoint and the expand-sum of the view direction over a ray's samples).
  G25c  eval branch (``is_test=True``, the module's fixed latents with the last one zeroed), loss = sum(raw G) -> ``x_grad``.

W = 64, K = 4, explicit latents through make_golden.ExplicitRandom.  Every fixture stores the reference's ReLU masks (``mask.trunk<i>``,
``mask.views``) and the smallest absolute pre-activation: the model seed of a case is the FIRST one, walking up from 0, at which that
smallest |pre-activation| is >= MIN_PRE - so that another fp32 implementation of the forward takes the same masks with no exception and
the comparison of the gradients is one of GEMM rounding alone.  Fixtures hold data only.
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

O = MG.O
W, K, C_ENT, MIN_PRE, MAX_SEED = 64, 4, 0.3, 2e-5, 64


def _hooks(net, rec):
    """pre-activations of every ReLU of MOD:168-181: the outputs of pts_linears[i] and views_linears[0]"""
    hs = [l.register_forward_hook(lambda m, i, o, k=f"trunk{j}": rec.__setitem__(k, o.detach().clone())) for j, l in enumerate(net.pts_linears)]
    hs.append(net.views_linears[0].register_forward_hook(lambda m, i, o: rec.__setitem__("views", o.detach().clone())))
    return hs


def _walk(R, tmp, run):
    """run(model, kw_train) -> fixture dict, with the first model seed whose smallest |pre-activation| clears MIN_PRE"""
    cfg = O.OracleCfg(netwidth=W, K_samples=K)
    for seed in range(MAX_SEED):
        _, kw_train, _, model, _, _ = build_reference_model(R, cfg, seed, tmp, K_samples=K)
        rec = {}
        hs = _hooks(model.module, rec)
        g = run(model, kw_train)
        for h in hs:
            h.remove()
        min_pre = min(float(v.abs().min()) for v in rec.values())
        if min_pre >= MIN_PRE:
            g.update(seed=seed, netwidth=W, K=K, min_abs_pre=np.float32(min_pre))
            g.update({"mask." + k: (v > 0).to(torch.uint8) for k, v in rec.items()})
            return g
    raise RuntimeError(f"no model seed below {MAX_SEED} keeps every pre-activation {MIN_PRE} away from zero")


def _data(data_seed, n_rays, n_samples):
    rng = np.random.default_rng(data_seed)
    pts = torch.tensor(rng.uniform(-1, 1, (n_rays, n_samples, 3)), dtype=torch.float32)
    dirs = torch.nn.functional.normalize(torch.tensor(rng.standard_normal((n_rays, 3)), dtype=torch.float32), dim=-1)
    G = torch.tensor(rng.standard_normal((n_rays * n_samples, K, 4)), dtype=torch.float32) / (n_rays * n_samples * K)
    ea = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)
    return pts, dirs, G, ea, er


def _encoded(R, pts, dirs):
    """x [P,90] as run_network builds it (RUN:70-80), handed over as a LEAF: the seam's input"""
    embed_fn, _ = R.get_embedder(10, 0)
    embeddirs_fn, _ = R.get_embedder(4, 0)
    with torch.no_grad():
        d = dirs[:, None].expand(pts.shape).reshape(-1, 3)
        return torch.cat([embed_fn(pts.reshape(-1, 3)), embeddirs_fn(d)], -1)


def g25a(R, tmp):
    pts, dirs, G, ea, er = _data(2511, 8, 1)

    def run(model, kw_train):
        x = _encoded(R, pts, dirs).requires_grad_(True)
        with ExplicitRandom(normals=[ea, er]) as rnd:                 # MOD:234 draws eps_alpha, MOD:246 eps_rgb
            raw, ent = model(x, False, False)
            assert not rnd.normals
        ((raw * G).sum() + C_ENT * ent.mean()).backward()
        return dict(x=x.detach(), G=G, eps_alpha=ea, eps_rgb=er, c_entropy=np.float32(C_ENT), raw=raw.detach(),
                    loss_entropy=ent.mean().detach(), x_grad=x.grad.clone())
    return _walk(R, tmp, run)


def g25b(R, tmp):
    pts0, dirs0, G, ea, er = _data(2521, 2, 4)

    def run(model, kw_train):
        pts, dirs = pts0.clone().requires_grad_(True), dirs0.clone().requires_grad_(True)
        embed_fn, _ = R.get_embedder(10, 0)
        embeddirs_fn, _ = R.get_embedder(4, 0)
        with ExplicitRandom(normals=[ea, er]) as rnd:
            raw, ent = R.run_network(pts, dirs, model, False, False, embed_fn, embeddirs_fn, netchunk=1024 * 64)
            assert not rnd.normals
        assert tuple(raw.shape) == (2, 4, K, 4)
        ((raw.reshape(-1, K, 4) * G).sum() + C_ENT * ent.mean()).backward()
        return dict(pts=pts0, viewdirs=dirs0, G=G, eps_alpha=ea, eps_rgb=er, c_entropy=np.float32(C_ENT), raw=raw.detach(),
                    loss_entropy=ent.mean().detach(), pts_grad=pts.grad.clone(), viewdirs_grad=dirs.grad.clone())
    return _walk(R, tmp, run)


def g25c(R, tmp):
    pts, dirs, G, ea, er = _data(2531, 8, 1)

    def run(model, kw_train):
        net = model.module
        net.sample_alpha, net.sample_rgb = ea.clone(), er.clone()      # the fixed eval latents (MOD:54-55); the branch zeroes the last (MOD:199,205)
        x = _encoded(R, pts, dirs).requires_grad_(True)
        raw, aux = model(x, False, True)
        assert not aux.any()                                           # MOD:223
        (raw * G).sum().backward()
        return dict(x=x.detach(), G=G, sample_alpha=ea, sample_rgb=er, raw=raw.detach(), x_grad=x.grad.clone())
    return _walk(R, tmp, run)


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(HERE, "inputgrad")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
    os.makedirs(out_dir, exist_ok=True)
    R = import_reference()
    tmp = tempfile.mkdtemp(prefix="cfnerf_golden_inputgrad_")
    out = {"g25a_train_x_grad": g25a(R, tmp), "g25b_run_network_grads": g25b(R, tmp), "g25c_eval_x_grad": g25c(R, tmp)}
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
