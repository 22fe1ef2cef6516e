"""Shared by tests/test_raygrad_cpu.py and tests/test_hip_raygrad.py: a torch restatement of the two CFNERF_F_RAY_GRAD kernels' formulas
(csrc/cfnerf_raygrad.hip) in the dtype of its inputs, the linear loss of the G26 fixtures, and the fixtures' loaders."""
import json
import os

import numpy as np
import torch

from oracle import cfnerf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raygrad")
C_ENT = 0.3


def linear_loss(ret, G, Gd):
    """sum(rgb_map G) + sum(depth_map Gd) + 0.3 mean(entropy): the loss of the fixtures and of the GPU cases"""
    loss = (ret["rgb_map"] * G).sum()
    if Gd is not None:
        loss = loss + (ret["depth_map"] * Gd).sum()
    ent = ret.get("loss_entropy")
    if ent is not None:
        loss = loss + C_ENT * ent.mean()
    return loss


def comp_zgrad_mirror(raw, z, rays_d, G, Gd, white_bkgd=False):
    """comp_zgrad_kernel: raw [N,S,K,4], z [N,S], rays_d [N,3], G [N,3,K] = d loss / d rgb_map, Gd [N,K] or None ->
    (d_z [N,S], d_rays_d [N,3]): the composite's adjoint in the sample depths and in |rays_d| (RUN:424-447)"""
    N, S, K, _ = raw.shape
    dt = raw.dtype
    Gd = torch.zeros(N, K, dtype=dt) if Gd is None else Gd
    dnorm = torch.sqrt((rays_d * rays_d).sum(-1))                                                     # [N]
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 1e1, dtype=dt)], -1)                     # RUN:426-427 (the 1e1 last interval)
    dist = dz * dnorm[:, None]
    sp = torch.nn.functional.softplus(raw[..., 3])                                                    # [N,S,K]
    e = torch.exp(-sp * dist[..., None])
    alpha = 1.0 - e
    x = (1.0 - alpha) + 1e-10
    T = torch.cumprod(torch.cat([torch.ones(N, 1, K, dtype=dt), x], 1), 1)[:, :-1]
    w = alpha * T
    g = (torch.sigmoid(raw[..., :3]) * G.transpose(1, 2)[:, None]).sum(-1) + Gd[:, None] * z[..., None]   # d loss / d w  [N,S,K]
    if white_bkgd:
        g = g - G.sum(1)[:, None]
    # comp_adjoint_D: D_s = (g_s - g_{s+1}) + x_{s+1} D_{s+1} - 1e-10 g_{s+1}, D behind the last sample = 0 (g = x = 0 there)
    D = torch.zeros_like(g)
    gn, xn, Dn = torch.zeros(N, K, dtype=dt), torch.zeros(N, K, dtype=dt), torch.zeros(N, K, dtype=dt)
    for s in range(S - 1, -1, -1):
        D[:, s] = (g[:, s] - gn) + xn * Dn - 1e-10 * gn
        gn, xn, Dn = g[:, s], x[:, s], D[:, s]
    d_dist = ((T * D) * e * sp).sum(-1)                                                               # [N,S]
    d_z = (Gd[:, None] * w).sum(-1)                                                                   # the explicit z of depth_map, RUN:447
    flow = d_dist * dnorm[:, None]
    flow[:, -1] = 0.0
    d_z = d_z - flow
    d_z[:, 1:] = d_z[:, 1:] + flow[:, :-1]
    d_norm = (d_dist * dz).sum(-1)
    return d_z, d_norm[:, None] * rays_d / dnorm[:, None]


def embed_adjoint(dg, enc):
    """the embedder's adjoint from the STASHED encoding: d_p[c] = dg[c] + sum_l 2^l (dg[3+6l+c] enc[6+6l+c] - dg[6+6l+c] enc[3+6l+c])"""
    L = (enc.shape[-1] - 3) // 6
    out = dg[..., :3].clone()
    for l in range(L):
        out = out + (2.0 ** l) * (dg[..., 3 + 6 * l:6 + 6 * l] * enc[..., 6 + 6 * l:9 + 6 * l] - dg[..., 6 + 6 * l:9 + 6 * l] * enc[..., 3 + 6 * l:6 + 6 * l])
    return out


def ray_grad_mirror(dgp, dgd, enc, gd, z, rays_d):
    """ray_grad_kernel's epilogue: dgp [N,S,ic] / dgd [N,S,icv] = d loss / d gamma(p), d gamma(d) per point, enc [N,S,ic] = gamma(p),
    gd [N,icv] = gamma(d) of the ray -> (d_o [N,3], d_d [N,3], d_z [N,S], d_viewdirs [N,3]) through pts = o + d z (RUN:534)"""
    d_p = embed_adjoint(dgp, enc)                                                                     # [N,S,3]
    return d_p.sum(1), (d_p * z[..., None]).sum(1), (d_p * rays_d[:, None]).sum(-1), embed_adjoint(dgd.sum(1), gd)


def mirror_ray_grads(p, ray_batch, cfg, ea, er, G, Gd, z_vals, white_bkgd=False):
    """(d_rays [N,11] with columns 6, 7 zero, d_z [N,S]) of linear_loss by the kernels' formulas, fed what the kernels are fed: the
    oracle's raw and d loss / d [gamma(p) | gamma(d)] (autograd up to the encoded inputs only), z, rays"""
    N, S = z_vals.shape
    rays_o, rays_d, viewdirs = ray_batch[:, 0:3], ray_batch[:, 3:6], ray_batch[:, 8:11]
    pts = (rays_o[:, None] + rays_d[:, None] * z_vals[..., None]).detach()
    enc = O.embed(pts.reshape(-1, 3), cfg.multires)
    gd = O.embed(viewdirs.detach(), cfg.multires_views)
    x = torch.cat([enc, gd[:, None].expand(N, S, gd.shape[-1]).reshape(N * S, -1)], -1).detach().requires_grad_(True)
    raw, ent = O.nerf_flows_forward(p, x, ea, er, cfg, False)
    raw = raw.reshape(N, S, raw.shape[-2], 4)
    rgb_map, _, _, depth_map = O.raw2outputs(raw, z_vals.detach(), rays_d.detach(), white_bkgd)
    loss = linear_loss(dict(rgb_map=rgb_map, depth_map=depth_map, loss_entropy=ent), G, Gd)
    (dx,) = torch.autograd.grad(loss, x)
    ic = enc.shape[-1]
    dz_c, dd_c = comp_zgrad_mirror(raw.detach(), z_vals.detach(), rays_d.detach(), G, Gd, white_bkgd)
    d_o, d_d, dz_n, d_v = ray_grad_mirror(dx[:, :ic].reshape(N, S, ic), dx[:, ic:].reshape(N, S, -1), enc.reshape(N, S, ic), gd,
                                          z_vals.detach(), rays_d.detach())
    d_rays = torch.zeros(N, 11, dtype=raw.dtype)
    d_rays[:, 0:3], d_rays[:, 3:6], d_rays[:, 8:11] = d_o, d_d + dd_c, d_v
    return d_rays, dz_c + dz_n


def random_rays(rng, N, near=2.0, far=6.0, dtype=torch.float32):
    """[N,11] rays with non-unit directions (so that |rays_d| matters) and their own view directions"""
    o = rng.uniform(-0.3, 0.3, (N, 3))
    d = rng.standard_normal((N, 3)) * 0.3 + np.array([0.1, -0.2, -1.0])
    v = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.tensor(np.concatenate([o, d, np.full((N, 1), near), np.full((N, 1), far), v], -1), dtype=dtype)


# ---- fixtures of the real reference (tests/golden/raygrad, G26)
def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def manifest():
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as f:
        return json.load(f)


T = lambda a: torch.tensor(np.asarray(a))
