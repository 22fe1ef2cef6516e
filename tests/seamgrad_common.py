"""Shared by tests/test_seamgrad_cpu.py, tests/test_hip_seamgrad.py and tests/tools/seam_zgrad_bench.py (CFNERF_F_SEAM_GRAD: raw2outputs
differentiated in z_vals and rays_d): a torch restatement of comp_seam_zgrad_kernel's formula (csrc/cfnerf_bwd.hip) with all four cotangents
in the dtype of its inputs, the kernel's cases with their inputs, and fp64 autograd of the oracle's raw2outputs on them."""
import functools

import numpy as np
import torch

from oracle import cfnerf_oracle as O

import raygrad_common as RG


def seam_zgrad_mirror(raw, z, rays_d, G, Gq=None, Gd=None, Gw=None, white_bkgd=False):
    """comp_seam_zgrad_kernel: raw [N,S,K,4], z [N,S], rays_d [N,3], cotangents G [N,3,K] of rgb_map, Gq [N,K] of disp_map, Gd [N,K] of
    depth_map, Gw [N,S,K] of weights (each of the last three or None) -> (d_z [N,S], d_rays_d [N,3]).  RG.comp_zgrad_mirror with the
    disp_map and weights cotangents entering g, Gd' and Ga as they do in composite_bwd_kernel."""
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
    Ga = torch.zeros(N, K, dtype=dt)
    if white_bkgd:
        Ga = Ga - G.sum(1)                                                                            # rgb_map += 1 - acc, RUN:452
    if Gq is not None:                                                                                # disp = 1 / max(2e-10, depth / (acc + 1e-10) + 1e-10), RUN:448
        depth, acc = (w * z[..., None]).sum(1), w.sum(1)
        qq = depth / (acc + 1e-10) + 1e-10
        gq = torch.where(qq > 2e-10, -Gq / (qq * qq), torch.zeros_like(qq))                           # torch.max routes the gradient to the larger argument
        Gd = Gd + gq / (acc + 1e-10)
        Ga = Ga + gq * (-depth / ((acc + 1e-10) * (acc + 1e-10)))
    g = (torch.sigmoid(raw[..., :3]) * G.transpose(1, 2)[:, None]).sum(-1) + Gd[:, None] * z[..., None] + Ga[:, None]   # d loss / d w  [N,S,K]
    if Gw is not None:
        g = g + Gw
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


# (N, S, K, cotangents in use, white_bkgd)                                       what it covers
ALL = ("G", "Gq", "Gd", "Gw")
CASES = [
    (1, 2, 4, ALL, False),                # one real interval plus the 1e1 one; one ray in a workgroup of four waves
    (5, 64, 3, ALL, False),               # one whole chunk; K ragged in a group of 4; N no multiple of the waves per workgroup
    (3, 65, 5, ALL, False),               # flow_{s-1} and the scan carry across a chunk boundary; K ragged in a group of 8; d_weights rows read one by one
    (2, 130, 12, ALL, False),             # three chunks; two latent groups: d_z accumulated across groups
    (3, 130, 16, ALL, False),             # hardware transcendentals
    (1, 64, 128, ALL, False),             # the maximum K: sixteen groups
    (5, 65, 5, ("Gq",), False),           # each optional cotangent alone (rgb_map's is zero)
    (5, 65, 5, ("Gd",), False),
    (5, 65, 12, ("Gw",), False),
    (3, 66, 12, ("G", "Gq", "Gw"), False),  # d_depth NULL
    (3, 65, 16, ALL, True),               # white_bkgd
    (2, 2, 16, ALL, True),                # S = 2 on the fast path
]
IDS = [f"N{n}-S{s}-K{k}-{'+'.join(u)}" + ("-wb" if wb else "") for n, s, k, u, wb in CASES]


@functools.lru_cache(maxsize=None)
def inputs(i):
    """fp32 inputs of case i (shared, never changed): raw, sorted depths in [2, 6], NON-UNIT rays_d, one cotangent per output in use"""
    N, S, K, use, wb = CASES[i]
    rng = np.random.default_rng(2600 + i)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    raw = t(rng.standard_normal((N, S, K, 4)))
    z = torch.sort(t(rng.uniform(2.0, 6.0, (N, S))), -1).values
    rays_d = RG.random_rays(rng, N)[:, 3:6].contiguous()
    cot = dict(G=t(rng.standard_normal((N, 3, K))) / (N * K), Gq=t(rng.standard_normal((N, K))) / (N * K),
               Gd=t(rng.standard_normal((N, K))) / (N * K), Gw=t(rng.standard_normal((N, S, K))) / (N * K))
    cot = {k: (v if k in use else None) for k, v in cot.items()}
    if cot["G"] is None:
        cot["G"] = torch.zeros(N, 3, K)                      # d_rgb_map is a required argument
    return dict(raw=raw, z=z, rays_d=rays_d, wb=wb, **cot)


def oracle_grads(inp, dt=torch.float64):
    """(d_z, d_rays_d) of sum(output . cotangent) by autograd of O.raw2outputs in dtype dt"""
    c = lambda v: None if v is None else v.to(dt)
    z, d = inp["z"].to(dt).requires_grad_(True), inp["rays_d"].to(dt).requires_grad_(True)
    rgb, disp, w, depth = O.raw2outputs(inp["raw"].to(dt), z, d, inp["wb"])
    loss = (rgb * c(inp["G"])).sum()
    for out, key in ((disp, "Gq"), (depth, "Gd"), (w, "Gw")):
        if inp[key] is not None:
            loss = loss + (out * c(inp[key])).sum()
    return torch.autograd.grad(loss, (z, d))


def rel(a, b):
    """max |a - b| as a fraction of b's largest entry, the way tests/test_hip_raygrad.py states an error"""
    b = b.detach().cpu().double()
    return float((a.detach().cpu().double() - b).abs().max() / b.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def fp32_formula_errors(i):
    """(error of d_z, error of d_rays_d, the two fp64 gradients) of case i: the kernel's formula evaluated by torch in fp32 on the CPU against
    fp64 autograd of the oracle - what a correct fp32 evaluation of this formula loses on these inputs"""
    inp = inputs(i)
    z64, d64 = oracle_grads(inp)
    z32, d32 = seam_zgrad_mirror(inp["raw"], inp["z"], inp["rays_d"], inp["G"], inp["Gq"], inp["Gd"], inp["Gw"], inp["wb"])
    return rel(z32, z64), rel(d32, d64), z64, d64
