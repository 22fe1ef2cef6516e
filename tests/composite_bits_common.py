"""The cases and inputs of tests/test_hip_composite_bits.py and tests/golden/make_golden_composite_bits.py: the four stand-alone composite
kernels (csrc/cfnerf_comp_fwd_body.h, csrc/cfnerf_comp_bwd_body.h) through cfnerf_composite_fwd, its CFNERF_F_CULL form and cfnerf_composite_bwd (plain and
CFNERF_F_SEAM_GRAD), every output as the SHA-256 of its bytes.  Inputs come from fixed numpy seeds on the CPU.

  S in {1, 65, 130}: a single lane, a ragged second chunk, three chunks.     N = 5: the second workgroup holds one ray.
  K in {1, 4, 5, 20}: KG = 4; 16-byte rows; KG = 8 with a ragged group and scalar rows; hardware transcendentals with a ragged group.
  K in {70, 72}, forward only: a second pass over kCompKB latents; the 32-latent weights turn-around (K % 4 == 0).
  white_bkgd both ways.  Ray 3 is empty space (density latents -40: acc = depth = 0, the clamp branch of disp_map and of its adjoint).
  forward: with and without `weights`.  sparse: every sample kept, and a table in which every odd ray has an empty chunk.
  adjoint: d_disp, d_depth, d_weights all present / all absent."""
import hashlib

import numpy as np
import torch

from cfnerf_amd import _lib as L

N = 5
S_ALL = (1, 65, 130)
K_ALL = (1, 4, 5, 20)
K_FWD = K_ALL + (70, 72)
DEV = "cuda"


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def inputs(S, K):
    """raw [N,S,K,4], z_vals [N,S] (increasing), rays_d [N,3] and the four cotangents, on the CPU"""
    rng = np.random.default_rng(7000 + 100 * S + K)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    raw = 2.0 * f(N, S, K, 4)
    raw[3, :, :, 3] = -40.0
    z = torch.from_numpy((2.0 + np.cumsum(rng.uniform(0.01, 0.1, (N, S)), -1)).astype(np.float32))
    return dict(raw=raw, z=z, d=f(N, 3), d_rgb=f(N, 3, K), d_disp=f(N, K), d_depth=f(N, K), d_weights=f(N, S, K))


def keep_mask(S, table):
    """[N,S] bool.  "all": every sample kept.  "holes": 60 % kept at random, and ray n = 1, 3 loses its chunk (n // 2) % nch whole."""
    if table == "all":
        return torch.ones(N, S, dtype=torch.bool)
    rng = np.random.default_rng(9000 + S)
    m = torch.from_numpy(rng.uniform(0, 1, (N, S)) < 0.6)
    nch = (S + 63) // 64
    for n in range(1, N, 2):
        ch = (n // 2) % nch
        m[n, ch * 64:(ch + 1) * 64] = False
    return m


def forward_dense(S, K, wb, with_weights):
    x = inputs(S, K)
    raw, z, d = x["raw"].to(DEV), x["z"].to(DEV), x["d"].to(DEV)
    rgb, disp, depth = torch.empty(N, 3, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, K, device=DEV)
    w = torch.empty(N, S, K, device=DEV) if with_weights else None
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(d), N, S, K, wb, L.ptr(rgb), L.ptr(disp), L.ptr(depth), L.ptr(w), L.stream()),
            "cfnerf_composite_fwd")
    out = dict(rgb_map=rgb, disp_map=disp, depth_map=depth)
    if with_weights:
        out["weights"] = w
    return out


def forward_sparse(S, K, wb, with_weights, table):
    x = inputs(S, K)
    m = keep_mask(S, table)
    cnt = m.sum(-1)
    ray_start = torch.zeros(N + 1, dtype=torch.int64)
    ray_start[1:] = torch.cumsum(cnt, 0)
    rows = torch.cumsum(m.reshape(-1).to(torch.int64), 0).reshape(N, S) - 1              # (ray, sample) order: the cull kernel's compaction
    slot = torch.where(m, rows, torch.full_like(rows, -1)).to(torch.int32)
    raw_c = x["raw"][m].contiguous().to(DEV)                                             # [P',K,4]
    z, d, slot, ray_start = x["z"].to(DEV), x["d"].to(DEV), slot.to(DEV), ray_start.to(DEV)
    rgb, disp, depth = torch.empty(N, 3, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, K, device=DEV)
    w = torch.empty(N, S, K, device=DEV) if with_weights else None
    sp = L.SparseRaw(L.dptr(slot), L.dptr(ray_start), L.dptr(w))
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw_c) if raw_c.numel() else None, L.ptr(z), L.ptr(d), N, S, K, wb | L.F_CULL, L.ptr(rgb), L.ptr(disp),
                                         L.ptr(depth), L.struct_arg(sp), L.stream()), "cfnerf_composite_fwd")
    out = dict(rgb_map=rgb, disp_map=disp, depth_map=depth)
    if with_weights:
        out["weights"] = w
    return out


def backward(S, K, wb, cots):
    """d_raw of the plain call; d_raw, d_z_vals and d_rays_d of the CFNERF_F_SEAM_GRAD call.  cots: "all" or "none" of d_disp, d_depth, d_weights"""
    x = inputs(S, K)
    raw, z, d, g_rgb = x["raw"].to(DEV), x["z"].to(DEV), x["d"].to(DEV), x["d_rgb"].to(DEV)
    g = [x[k].to(DEV) if cots == "all" else None for k in ("d_disp", "d_depth", "d_weights")]
    args = (L.ptr(raw), L.ptr(z), L.ptr(d), N, S, K)
    gp = (L.ptr(g_rgb), L.ptr(g[0]), L.ptr(g[1]), L.ptr(g[2]))
    d_raw = torch.empty_like(raw)
    L.check(L.lib().cfnerf_composite_bwd(*args, wb, *gp, L.ptr(d_raw), L.stream()), "cfnerf_composite_bwd")
    d_raw2, d_z, d_d = torch.empty_like(raw), torch.empty_like(z), torch.empty_like(d)
    out = L.composite_grads(d_raw=d_raw2, d_z_vals=d_z, d_rays_d=d_d)
    L.check(L.lib().cfnerf_composite_bwd(*args, wb | L.F_SEAM_GRAD, *gp, L.composite_grads_arg(out), L.stream()), "cfnerf_composite_bwd")
    return dict(d_raw=d_raw, d_raw_seam=d_raw2, d_z_vals=d_z, d_rays_d=d_d)


def cases():
    """(key, thunk) of every call; the thunk returns {output name: tensor}"""
    for S in S_ALL:
        for wb in (0, 1):
            for K in K_FWD:
                for ww in (1, 0):
                    yield f"fwd S={S} K={K} wb={wb} weights={ww}", (lambda S=S, K=K, wb=wb, ww=ww: forward_dense(S, K, wb, bool(ww)))
                    for table in ("all", "holes"):
                        yield (f"sparse {table} S={S} K={K} wb={wb} weights={ww}",
                               (lambda S=S, K=K, wb=wb, ww=ww, table=table: forward_sparse(S, K, wb, bool(ww), table)))
            for K in K_ALL:
                for cots in ("all", "none"):
                    yield f"bwd S={S} K={K} wb={wb} cotangents={cots}", (lambda S=S, K=K, wb=wb, cots=cots: backward(S, K, wb, cots))


def run_all():
    """{key: {output name: sha256}}"""
    res = {}
    for key, thunk in cases():
        out = thunk()
        torch.cuda.synchronize()
        res[key] = {name: sha(t) for name, t in out.items()}
    return res
