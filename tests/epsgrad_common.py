"""Shared by tests/test_epsgrad_cpu.py and tests/test_hip_epsgrad.py (CFNERF_F_EPS_GRAD: the render differentiated in its latents): the oracle's
latent gradients of a case - per ray / point row and summed - in a given dtype on given ReLU masks, with the calibration grad_close_tight
reads (the fp32 oracle's own distance from fp64, and std * sum |d z0| per entry), the oracle on the G28 fixtures, and their loaders."""
import json
import os

import numpy as np
import torch

from oracle import cfnerf_oracle as O

import cotangents_common as CC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epsgrad")
NAMES = ["g28a_render_rays_eps_grad", "g28b_netchunk_pairs_eps_grad", "g28c_forward_eps_grad"]
BASE = ("alpha_mean", "alpha_std", "rgb_mean", "rgb_std")
G_TIGHT = CC.G_TIGHT
T = CC.T
# the losses of the fused cases: the plain train loss (no cotangent descriptor), and one over every output of render_rays
USES = {"plain": ("G", "Gd", "ent"), "all": CC.SUBSETS["all"]}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def manifest():
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        return json.load(f)


def _rows_of(inp, dt, n):
    """the case's latents as one row per ray / point (a shared set: n identical rows - what d_eps_rows means, cfnerf.h)"""
    ea, er = inp["ea"].to(dt), inp["er"].to(dt)
    if ea.dim() == 2:
        ea, er = ea[None].expand(n, *ea.shape), er[None].expand(n, *er.shape)
    return ea.clone().requires_grad_(True), er.clone().requires_grad_(True)


def _tapped(fn):
    O.latent_tap = tap = {}
    try:
        return fn(), tap
    finally:
        O.latent_tap = None


def _grads(loss, la, lr, taps, q, std):
    """rows [n,K,4] (rgb then alpha), the base-Gaussian gradients, std * sum_samples |d loss / d z0| per row entry, and that sum without std"""
    leaves = [la, lr] + [t["alpha0"] for t in taps] + [t["rgb0"] for t in taps] + [q[k] for k in BASE]
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    n, K = la.shape[0], la.shape[1]
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    rows = torch.cat([z(gs[1], lr), z(gs[0], la)], -1)
    ca = torch.stack([z(g, t["alpha0"]).reshape(-1, K, 1).abs().sum(0) for g, t in zip(gs[2:2 + n], taps)])
    cr = torch.stack([z(g, t["rgb0"]).reshape(-1, K, 3).abs().sum(0) for g, t in zip(gs[2 + n:2 + 2 * n], taps)])
    sum_abs = torch.cat([cr * std["rgb_std"], ca * std["alpha_std"]], -1)
    base = {k: z(g, q[k]).detach() for k, g in zip(BASE, gs[2 + 2 * n:])}
    return rows.detach(), base, sum_abs.detach(), torch.cat([cr, ca], -1).detach()


def render_rows(p, inp, masks, dt, use):
    """(d_eps_rows [N,K,4], base-Gaussian gradients, sum_abs [N,K,4], sum |d z0| [N,K,4]) of loss_of(render_rays, use): the oracle called per ray with that ray's row,
    the entropy the mean over the rays"""
    q = {k: v.to(dt).clone().requires_grad_(k in BASE) for k, v in p.items()}
    rays, z = inp["rays"].to(dt), inp["z"].to(dt)
    N, S = z.shape
    la, lr = _rows_of(inp, dt, N)
    rets, taps = [], []
    for r in range(N):
        mk = {k: v[r * S:(r + 1) * S] for k, v in masks.items()}
        with O.relu_override(masks=mk):
            ret, tap = _tapped(lambda: O.render_rays(q, rays[r:r + 1], inp["cfg"], la[r], lr[r], True, None, inp["lindisp"], inp["wb"], z_vals=z[r:r + 1]))
        rets.append(ret)
        taps.append(tap)
    ret = {k: torch.cat([x[k] for x in rets], 0) for k in ("rgb_map", "disp_map", "depth_map", "raw", "weights")}
    ret["loss_entropy"] = sum(x["loss_entropy"] for x in rets) / N
    return _grads(CC.loss_of(ret, inp["cot"], use), la, lr, taps, q, {k: q[k].detach() for k in ("alpha_std", "rgb_std")})


def network_rows(p, inp, masks, dt):
    """the same for NeRF_Flows.forward on inp["x"] [P,90]: loss = sum(raw Gr) + C_ENT entropy, the oracle called per point with that point's row"""
    q = {k: v.to(dt).clone().requires_grad_(k in BASE) for k, v in p.items()}
    x = inp["x"].to(dt)
    P = x.shape[0]
    la, lr = _rows_of(inp, dt, P)
    raws, ents, taps = [], [], []
    for i in range(P):
        mk = {k: v[i:i + 1] for k, v in masks.items()}
        with O.relu_override(masks=mk):
            (raw, ent), tap = _tapped(lambda: O.nerf_flows_forward(q, x[i:i + 1], la[i], lr[i], inp["cfg"], False))
        raws.append(raw)
        ents.append(ent)
        taps.append(tap)
    loss = (torch.cat(raws, 0) * inp["Gr"].to(dt)).sum() + CC.C_ENT * sum(ents) / P
    return _grads(loss, la, lr, taps, q, {k: q[k].detach() for k in ("alpha_std", "rgb_std")})


def reference(rows_fn, counts=None):
    """The fp64 reference of a case and what grad_close_tight needs to hold fp32 code to it: {"rows" [n,K,4], "d_eps" [K,4] (the sum of the
    rows), "base": the base-Gaussian gradients} and, given the rows per latent pair `counts`, "pairs" [C,K,4] (the sum of each pair's
    consecutive rows), each tensor with `fp32_noise` (the fp32 CPU oracle's own distance from fp64 on these
    inputs, of the tensor's largest entry), `sum_abs` (std * sum |d z0| per entry) and `global_scale`"""
    r64, b64, s64, z64 = rows_fn(torch.float64)
    r32, b32, _, _ = rows_fn(torch.float32)
    out = {"rows": r64, "d_eps": r64.sum(0), "base": b64}
    s = {"rows": s64, "d_eps": s64.sum(0)}
    g32 = {"rows": r32.double(), "d_eps": r32.double().sum(0)}
    if counts is not None:
        seg = lambda t: torch.stack([x.sum(0) for x in torch.split(t, list(counts))])
        out["pairs"], s["pairs"], g32["pairs"] = seg(r64), seg(s64), seg(r32.double())
    gmax = float(r64.sum(0).abs().max())
    for k in [k for k in ("rows", "d_eps", "pairs") if k in s]:
        m = max(float(out[k].abs().max()), 1e-300)
        out[k].fp32_noise = float((g32[k] - out[k]).abs().max()) / m
        out[k].sum_abs = s[k].numpy()
        out[k].global_scale = gmax
    # the base-Gaussian means: sums over k of the same d z0 (the identity of cfnerf.h)
    for k, cols in (("alpha_mean", slice(3, 4)), ("rgb_mean", slice(0, 3))):
        g = b64[k]
        g.fp32_noise = float((b32[k].double() - g).abs().max()) / max(float(g.abs().max()), 1e-300)
        g.sum_abs = z64.sum((0, 1))[cols].numpy()
        g.global_scale = gmax
        out["base"][k] = g
    return out


def columns(t):
    """the two column blocks a latent gradient is compared on, like the base Gaussians' rgb_* / alpha_* tensors"""
    pick = lambda sl: _sliced(t, sl)
    return (("rgb columns", pick(slice(0, 3))), ("alpha column", pick(slice(3, 4))))


def _sliced(t, sl):
    v = t[..., sl]
    if hasattr(t, "fp32_noise"):
        v = v.clone()
        v.fp32_noise, v.sum_abs, v.global_scale = t.fp32_noise, np.asarray(t.sum_abs)[..., sl], t.global_scale
    return v


def direct_term(eps, d_ent):
    """the base log-normal's direct term of d_eps [K,4] (MOD:268,283,286): -d_entropy eps / K for the density latent, / (3 K) for a colour latent;
    `eps` [K,4] or rows [n,K,4] (then summed over the rows, each 1 / n)"""
    e = eps.double()
    if e.dim() == 3:
        e = e.mean(0)
    K = e.shape[0]
    return -float(d_ent) * e / K * torch.tensor([1 / 3, 1 / 3, 1 / 3, 1.0], dtype=torch.float64)


# ---- the G28 fixtures through the oracle
def oracle_fixture(name, g, dtype=torch.float32):
    """({"eps_alpha_grad", "eps_rgb_grad", "grad.<base Gaussian>"}, loss) of the fixture's loss by the oracle's autograd on the STORED masks"""
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]), netdepth=int(g["netdepth"]))
    c = lambda a: T(a).to(dtype)
    p = {k: v.to(dtype).clone().requires_grad_(k in BASE) for k, v in O.make_params(cfg, int(g["seed"])).items()}
    masks = {k[len("mask."):]: T(v).to(dtype) for k, v in g.items() if k.startswith("mask.")}
    ea, er = c(g["eps_alpha"]).requires_grad_(True), c(g["eps_rgb"]).requires_grad_(True)
    if name == NAMES[2]:
        with O.relu_override(masks=masks):
            raw, ent = O.nerf_flows_forward(p, c(g["x"]), ea, er, cfg, False)
        loss = (raw * c(g["Gr"])).sum() + float(g["c_entropy"]) * ent
    else:
        rb, tr = c(g["ray_batch"]), c(g["t_rand"])
        opt = dict(lindisp=True, white_bkgd=True) if name == NAMES[1] else {}
        S = tr.shape[1]
        if ea.dim() == 2:
            with O.relu_override(masks=masks):
                ret = O.render_rays(p, rb, cfg, ea, er, True, tr, **opt)
        else:                                             # one network call per pair: `per` rays each, the entropy the mean over the points
            per = int(g["netchunk"]) // S
            rets = []
            for ci in range(ea.shape[0]):
                sl = slice(ci * per, (ci + 1) * per)
                with O.relu_override(masks={k: v[ci * per * S:(ci + 1) * per * S] for k, v in masks.items()}):
                    rets.append(O.render_rays(p, rb[sl], cfg, ea[ci], er[ci], True, tr[sl], **opt))
            ret = {k: torch.cat([x[k] for x in rets], 0) for k in ("rgb_map", "disp_map", "depth_map", "raw")}
            ret["loss_entropy"] = sum(x["loss_entropy"] for x in rets) / len(rets)
        Gr = c(g["Gr_a"])[:, :, None, None] * c(g["Gr_b"])[None, None]
        loss = ((ret["rgb_map"] * c(g["G"])).sum() + (ret["disp_map"] * c(g["Gq"])).sum() + (ret["depth_map"] * c(g["Gd"])).sum()
                + (ret["raw"] * Gr).sum() + float(g["c_entropy"]) * ret["loss_entropy"].mean())
    loss.backward()
    grads = {"eps_alpha_grad": ea.grad, "eps_rgb_grad": er.grad}
    grads.update({"grad." + k: p[k].grad for k in BASE})
    return grads, loss.detach()
