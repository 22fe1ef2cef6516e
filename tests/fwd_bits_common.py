"""The cases and inputs of tests/test_hip_fwd_bits.py and tests/golden/make_golden_fwd_bits.py: the fused forward (fused_fwd_kernel) and the
geometry-only forward (geom_fwd_kernel), whose shared phases are the texts csrc/cfnerf_fwd_trunk_body.h and csrc/cfnerf_fwd_halpha_body.h,
through cfnerf_render_fwd, cfnerf_render_eval and cfnerf_network_fwd - every output as the SHA-256 of its bytes.  Inputs come from fixed
seeds on the CPU.  The smallest shapes that reach every branch of the shared text:

  models   w64: W = 64 (four waves), default depth, h_alpha_size 96 (the thread count is no multiple of it: the indexed form of the k-split
           sum); w512d5: W = 512 (eight waves), netdepth 5 (the skip layer moves), h_alpha_size 64 (two n-tiles of partial sums).
  rays     N = 3.  S = 1 a single lane (dist = 1e1 only), 65 a ragged second tile, 128 whole tiles (with a stash: the Q4 train variant).
           K = 1, 5 the one-latent path (k wraps the waves), 20 the hardware-math pair path (singles left over at four waves, idle waves
           at eight).  Depths from the table, from the table + t_rand, or explicit z_vals; lindisp on and off (near = 2, far = 6).
  points   P = 1, 65 (ragged) and, for the Q4 stash, 128.
  variants eval | ext: CFNERF_F_KSTATS_EXT through cfnerf_render_fwd (eval and train branch) and, with a target (sqerr), cfnerf_render_eval |
           train (no stash) | stash | rows: stash + CFNERF_F_EPS_ROWS | geom: CFNERF_F_GEOMETRY; fp32 and bf16x3.
A stash case also hashes the flat gradient of the backward of that stash with seeded cotangents (the backward kernels are deterministic,
tests/test_hip_train.py): it pins what the forward stashed."""
import hashlib

import numpy as np
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd.api import _network_fwd, _network_geometry, _pack_rays, _render_fwd, _render_geometry_fwd

N = 3
DEV = "cuda"
NEAR, FAR = 2.0, 6.0
MODELS = {"w64": dict(netwidth=64, h_alpha_size=96), "w512d5": dict(netwidth=512, netdepth=5, h_alpha_size=64)}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def build(name):
    """The model `name` of MODELS with the oracle's seeded weights (tests/util_hip.py); returns the NeRF_Flows module"""
    from oracle import cfnerf_oracle as O
    from util_hip import build_model
    _, _, _, model, _, _ = build_model(O.OracleCfg(K_samples=5, **MODELS[name]), 4100 + len(name))
    net = model.module
    net._sync()
    return net


def _spec(mode, variant, n, K, prec="fp32", samp="table", lindisp=0):
    return dict(mode=mode, variant=variant, n=n, K=K, prec=prec, samp=samp, lindisp=lindisp)


def specs(name):
    """The launches of the model `name`, as plain dicts (no GPU needed to list them); `n` is S in ray mode and P in points mode"""
    out = []
    samp3, k = ("table", "t_rand", "z_vals"), 0
    for S in (1, 65, 128):                                                  # eval and geometry: the S x K grid (at eight waves the half of it
        for K in (1, 5, 20):                                                # in which K = 5 no longer wraps the waves and K = 20 leaves some idle)
            if name == "w64" or k % 2 == 1 or (S, K) == (128, 20):
                out.append(_spec("rays", "eval", S, K, samp=samp3[k % 3], lindisp=(k // 3) % 2))
                out.append(_spec("rays", "geom", S, K, samp=("table", "z_vals")[k % 2], lindisp=(k + 1) % 2))
            k += 1
    out += [_spec("rays", "ext", 65, 20, lindisp=1), _spec("rays", "ext", 128, 5), _spec("rays", "ext-train", 65, 5, samp="t_rand"),
            _spec("rays", "train", 1, 5, samp="t_rand"), _spec("rays", "train", 128, 1, samp="t_rand"),
            _spec("rays", "stash", 65, 5, samp="t_rand"), _spec("rays", "stash", 128, 20, samp="t_rand", lindisp=1),
            _spec("rays", "stash", 128, 1), _spec("rays", "stash", 65, 20, samp="z_vals"),
            _spec("rays", "rows", 65, 5, samp="t_rand"), _spec("rays", "rows", 128, 20),
            _spec("rays", "eval", 65, 5, prec="bf16x3", samp="t_rand"), _spec("rays", "eval", 128, 20, prec="bf16x3", lindisp=1),
            _spec("rays", "geom", 65, 20, prec="bf16x3"), _spec("rays", "geom", 128, 5, prec="bf16x3", samp="z_vals"),
            _spec("rays", "stash", 65, 20, prec="bf16x3", samp="t_rand"), _spec("rays", "rows", 65, 5, prec="bf16x3")]
    out += [_spec("points", "eval", 1, 5), _spec("points", "eval", 65, 20),
            _spec("points", "geom", 1, 20), _spec("points", "geom", 65, 5),
            _spec("points", "train", 1, 5), _spec("points", "train", 65, 20),
            _spec("points", "stash", 65, 5), _spec("points", "stash", 128, 20),
            _spec("points", "rows", 65, 5), _spec("points", "rows", 128, 20),
            _spec("points", "geom", 65, 20, prec="bf16x3"), _spec("points", "stash", 65, 5, prec="bf16x3")]
    return out


def key(name, s):
    return f"{name} {s['mode']} {s['variant']} {s['prec']} n={s['n']} K={s['K']} samp={s['samp']} lindisp={s['lindisp']}"


def keys():
    return [key(name, s) for name in MODELS for s in specs(name)]


def _seeded(seed):
    g = torch.Generator().manual_seed(seed)
    return (lambda *shape: torch.randn(*shape, generator=g)), (lambda *shape: torch.rand(*shape, generator=g))


def _pose():
    th, ph = np.deg2rad(30.0), np.deg2rad(-30.0)
    return torch.tensor([[np.cos(th), -np.sin(th) * np.sin(ph), np.sin(th) * np.cos(ph), 4 * np.sin(th) * np.cos(ph)],
                         [0, np.cos(ph), np.sin(ph), 4 * np.sin(ph)],
                         [-np.sin(th), -np.cos(th) * np.sin(ph), np.cos(th) * np.cos(ph), 4 * np.cos(th) * np.cos(ph)]], dtype=torch.float32)


def _backward(net, call, d_out, d_ent, extra=()):
    """the flat gradient of the model's current stash through cfnerf_render_bwd / cfnerf_network_bwd"""
    lib = L.lib()
    grad = torch.empty(net.n_params, device=DEV)
    gen = lib.cfnerf_model_stash_generation(net.handle)
    L.check(getattr(lib, call)(net.handle, gen, L.ptr(d_out), *extra, L.ptr(d_ent), L.ptr(grad), L.stream()), call)
    return grad


def run_rays(net, s):
    S, K, variant = s["n"], s["K"], s["variant"]
    randn, rand = _seeded(5000 + 100 * S + K)
    packed = _pack_rays(40, 30, 33.3, c2w=_pose(), n=N, pixel0=37, ndc=False, near=NEAR, far=FAR, device=net.device)
    tv = torch.linspace(0., 1., S, device=DEV)
    t_rand = rand(N, S).to(DEV) if s["samp"] == "t_rand" else None
    z = (NEAR + (FAR - NEAR) * torch.sort(rand(N, S), -1)[0]).to(DEV).contiguous() if s["samp"] == "z_vals" else None
    rows = variant == "rows"
    eps = (randn(N, K, 4) if rows else randn(K, 4)).to(DEV)
    gt, d_rgb, d_depth = rand(N, 3).to(DEV), randn(N, 3, K).to(DEV), randn(N, K).to(DEV)
    base = L.F_LINDISP if s["lindisp"] else 0
    ks = K >= 2                                                             # the K-statistics divide by K - 1
    if variant == "geom":
        o = _render_geometry_fwd(net, packed, tv, eps, base | L.F_GEOMETRY, z_vals=z, raw=True, weights=True, pts=True, kstats=ks)
    elif variant == "eval":
        o = _render_fwd(net, packed, tv, t_rand, eps, base, z_vals=z, raw=True, weights=True, pts=True, kstats=ks, entropy=False)
    elif variant in ("ext", "ext-train"):
        train = L.F_TRAIN if variant == "ext-train" else 0
        o = _render_fwd(net, packed, tv, t_rand, eps, base | train | L.F_KSTATS_EXT, z_vals=z, weights=True, kstats=True, entropy=bool(train))
        if not train:                                                       # ... and with a target: sqerr [N,6]
            o["eval_kstats"], o["eval_sqerr"] = torch.empty(N, 12, device=DEV), torch.empty(N, 6, device=DEV)
            L.check(L.lib().cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(tv), L.ptr(eps), N, S, K, base | L.F_KSTATS_EXT, L.ptr(gt),
                                               L.ptr(o["eval_kstats"]), L.ptr(o["eval_sqerr"]), L.stream()), "cfnerf_render_eval")
    elif variant == "train":
        o = _render_fwd(net, packed, tv, t_rand, eps, base | L.F_TRAIN, z_vals=z, raw=True, weights=True)
    else:                                                                   # stash, rows (_render_fwd sets CFNERF_F_EPS_ROWS from the shape)
        net.ensure_workspace(N, S, K)
        o = _render_fwd(net, packed, tv, t_rand, eps, base | L.F_TRAIN | L.F_STASH, z_vals=z, raw=True, weights=True, pts=True)
        o["grad"] = _backward(net, "cfnerf_render_bwd", d_rgb, torch.tensor([0.01], device=DEV), extra=(L.ptr(d_depth),))
    return o


def run_points(net, s):
    P, K, variant = s["n"], s["K"], s["variant"]
    randn, rand = _seeded(6000 + 100 * P + K)
    x = (rand(P, 90) * 2 - 1).to(DEV)
    eps = (randn(P, K, 4) if variant == "rows" else randn(K, 4)).to(DEV)
    d_raw = randn(P, K, 4).to(DEV)
    if variant == "geom":
        return {"raw": _network_geometry(net, x, eps)}
    if variant == "eval":
        return {"raw": _network_fwd(net, x, eps, K, 0)[0]}
    if variant == "train":
        raw, ent = _network_fwd(net, x, eps, K, L.F_TRAIN)
        return {"raw": raw, "entropy": ent}
    net.ensure_workspace(1, P, K)
    raw, ent = _network_fwd(net, x, eps, K, L.F_TRAIN | L.F_STASH)
    return {"raw": raw, "entropy": ent, "grad": _backward(net, "cfnerf_network_bwd", d_raw, torch.tensor([0.01], device=DEV))}


def run(net, s):
    """{output name: tensor} of one launch (the outputs that were asked for)"""
    if getattr(net, "precision", "fp32") != s["prec"]:
        net.set_precision(s["prec"])
        net._sync()
    out = run_rays(net, s) if s["mode"] == "rays" else run_points(net, s)
    torch.cuda.synchronize()
    return {k: v for k, v in out.items() if v is not None}


def run_all():
    """{key: {output name: sha256}} over both models"""
    res = {}
    for name in MODELS:
        net = build(name)
        for s in specs(name):
            res[key(name, s)] = {k: sha(v) for k, v in run(net, s).items()}
    return res
