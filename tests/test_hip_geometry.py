"""-m gpu: the geometry-only forward (CFNERF_F_GEOMETRY): density queries in points mode, depth / disparity maps, weights and the [N,6]
statistics in ray mode, ``NeRF_Flows.sample``, ``api.render_geometry``, ``evaluate.density_grid`` and
``render_uncertainty(stats="geometry")``.

The yardstick is the launch WITHOUT the flag on the same model and inputs (itself pinned to the real reference by the goldens):
the geometry-only kernel runs the same trunk / h_alpha / density-flow arithmetic in the same order, so every comparison with it is
``torch.equal``.  Two tests go to the reference's own fixtures at the tolerances of tests/util_hip.py."""
import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
from cfnerf_amd.api import _pack_rays, _render_fwd, _render_geometry_fwd, render_geometry
from oracle import cfnerf_oracle as O
from util_hip import ATOL, ATOL_DISP, RTOL, build_model, close

pytestmark = pytest.mark.gpu
T = lambda a: torch.tensor(np.asarray(a))
DEV = "cuda"
G = L.F_GEOMETRY
SENTINEL = -7.0


def _model(W, K, ha=32, seed=77, flow=None, prec=None, **over):
    cfg = O.OracleCfg(netwidth=W, K_samples=K, h_alpha_size=ha, **{k: v for k, v in over.items() if k == "n_flows"})
    _, _, kw_test, model, p, _ = build_model(cfg, seed + W + K, **{k: v for k, v in over.items() if k != "n_flows"})
    net = model.module
    if flow:
        net.set_flow_math(flow)
    if prec:
        net.set_precision(prec)
    net._sync()
    return model, net


def _points_pair(net, x, eps, K):
    """(raw [P,K,4] of the launch without the flag, raw [P,K] of the launch with it) through cfnerf_network_fwd"""
    P = x.shape[0]
    lib = L.lib()
    full = torch.full((P, K, 4), SENTINEL, device=DEV)
    geom = torch.full((P, K), SENTINEL, device=DEV)
    L.check(lib.cfnerf_network_fwd(net.handle, L.ptr(x), L.ptr(eps), P, K, 0, L.ptr(full), None, L.stream()), "network_fwd")
    L.check(lib.cfnerf_network_fwd(net.handle, L.ptr(x), L.ptr(eps), P, K, G, L.ptr(geom), None, L.stream()), "network_fwd geometry")
    return full, geom


def _points_inputs(P, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(P, 90, generator=g) * 2 - 1).to(DEV), torch.randn(K, 4, generator=g).to(DEV)


# ---------------------------------------------------------------------------------------------- 1. points mode
POINT_CASES = [
    (64, 1, 1, 32, {}),                          # the smallest shape
    (64, 5, 65, 32, {}),                         # ragged second tile; k wraps the four waves
    (256, 4, 129, 32, {}),
    (256, 17, 64, 128, {}),                      # hardware-math pair path with a single latent left over
    (512, 33, 70, 64, {}),                       # eight waves; pairs k, k + 8
    (192, 128, 33, 96, {}),
    (256, 4, 129, 32, {"flow": "fast"}),
    (256, 17, 64, 128, {"flow": "libm"}),
    (256, 4, 129, 32, {"prec": "bf16x3"}),
    (64, 5, 65, 32, {"n_flows": 2}),
]


@pytest.mark.parametrize("W,K,P,ha,opt", POINT_CASES, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_points_density_latent_has_the_bits_of_the_full_forward(W, K, P, ha, opt):
    model, net = _model(W, K, ha, **opt)
    x, eps = _points_inputs(P, K, 11 + P)
    full, geom = _points_pair(net, x, eps, K)
    assert not (geom == SENTINEL).any() and bool(torch.isfinite(geom).all())
    assert torch.equal(geom, full[..., 3])
    _, again = _points_pair(net, x, eps, K)                               # 5. determinism
    assert torch.equal(again, geom)


# ---------------------------------------------------------------------------------------------- 2. points mode, the real reference
def test_points_vs_reference_golden_and_sample(golden):
    g = golden("g123_model_w256")
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]), netdepth=int(g.get("netdepth", 8)), n_flows=int(g.get("n_flows", 4)),
                      h_alpha_size=int(g.get("h_alpha_size", 32)), h_rgb_size=int(g.get("h_rgb_size", 64)),
                      multires=int(g.get("multires", 10)), multires_views=int(g.get("multires_views", 4)))
    _, _, _, model, p, _ = build_model(cfg, int(g["seed"]))
    net = model.module
    x = T(g["x90"]).to(DEV).float().contiguous()
    net.sample_alpha = T(g["eps_alpha"]).clone()
    net.sample_rgb = T(g["eps_rgb"]).clone()
    net._sync()
    K = cfg.K_samples
    _, zeroed = _points_pair(net, x, net.eval_eps(), K)                  # the eval branch: last latent zeroed (MOD:199)
    close(zeroed, np.asarray(g["raw_eval"])[..., 3], ATOL, RTOL, what="density latent vs the reference's raw_eval[..., 3]")
    kept = torch.cat([net.sample_rgb, net.sample_alpha], -1).float().to(DEV).contiguous()
    _, unzeroed = _points_pair(net, x, kept, K)
    with torch.no_grad():
        s = net.sample(x)
    assert list(s.shape) == [x.shape[0], K, 1]
    assert torch.equal(s[..., 0], unzeroed)                               # MOD:78: sample_alpha as it is
    assert torch.equal(s[:, :K - 1, 0], zeroed[:, :K - 1])
    with torch.no_grad():
        e = net.sample(x, eps_alpha=kept[:, 3:].cpu() * 0.5)
    _, half = _points_pair(net, x, torch.cat([kept[:, :3], kept[:, 3:] * 0.5], -1).contiguous(), K)
    assert torch.equal(e[..., 0], half)


# ---------------------------------------------------------------------------------------------- 3. ray mode
def _pose(ndc):
    if ndc:
        return torch.tensor([[1, 0, 0, 0.1], [0, 1, 0, -0.1], [0, 0, 1, 0.0]], dtype=torch.float32)
    th, ph = np.deg2rad(30.0), np.deg2rad(-30.0)
    return torch.tensor([[np.cos(th), -np.sin(th) * np.sin(ph), np.sin(th) * np.cos(ph), 4 * np.sin(th) * np.cos(ph)],
                         [0, np.cos(ph), np.sin(ph), 4 * np.sin(ph)],
                         [-np.sin(th), -np.cos(th) * np.sin(ph), np.cos(th) * np.cos(ph), 4 * np.cos(th) * np.cos(ph)]], dtype=torch.float32)


def _rays(net, N, ndc):
    H, Wd = 40, 30
    near, far = (0.0, 1.0) if ndc else (2.0, 6.0)
    return _pack_rays(H, Wd, 33.3, c2w=_pose(ndc), n=N, pixel0=37 if N + 37 <= H * Wd else 0, ndc=ndc, near=near, far=far, device=net.device), (near, far)


RAY_CASES = [
    (64, 2, 3, 128, dict(ndc=True)),
    (256, 4, 5, 100, dict(ndc=False, lindisp=True)),                     # ragged second tile
    (128, 16, 2, 130, dict(ndc=True)),                                   # three tiles, the last with 2 rows
    (512, 32, 2, 64, dict(ndc=True)),                                    # one tile
    (64, 2, 4, 1, dict(ndc=True)),                                       # a single sample: dist = 1e1 only
    (64, 3, 1100, 16, dict(ndc=True)),                                   # more rays than workgroups: the comp rows are re-initialised
    (256, 4, 5, 100, dict(ndc=False, z_vals=True)),                      # explicit z_vals_opt
    (64, 2, 3, 128, dict(ndc=True, white_bkgd=True)),                    # accepted, no effect
    (256, 4, 5, 100, dict(ndc=False, lindisp=True, prec="bf16x3")),
]


@pytest.mark.parametrize("W,K,N,S,opt", RAY_CASES, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_rays_every_output_has_the_bits_of_the_full_render(W, K, N, S, opt):
    model, net = _model(W, K, 64 if W == 512 else 32, prec=opt.get("prec"))
    packed, (near, far) = _rays(net, N, opt["ndc"])
    tv = torch.linspace(0., 1., S, device=DEV)
    z = None
    if opt.get("z_vals"):
        g = torch.Generator().manual_seed(5)
        z = (near + (far - near) * torch.sort(torch.rand(N, S, generator=g), -1)[0]).to(DEV).contiguous()
    eps = net.eval_eps()
    base = L.F_LINDISP if opt.get("lindisp") else 0
    full = _render_fwd(net, packed, tv, None, eps, base, z_vals=z, raw=True, weights=True, pts=True, entropy=False)
    ext = _render_fwd(net, packed, tv, None, eps, base | L.F_KSTATS_EXT, z_vals=z, maps=False, kstats=True, entropy=False)
    gflags = base | G | (L.F_WHITE_BKGD if opt.get("white_bkgd") else 0)
    geo = _render_geometry_fwd(net, packed, tv, eps, gflags, z_vals=z, raw=True, weights=True, pts=True, kstats=True)
    assert list(geo["raw"].shape) == [N, S, K] and list(geo["kstats"].shape) == [N, 6]
    assert torch.equal(geo["depth_map"], full["depth_map"])
    assert torch.equal(geo["disp_map"], full["disp_map"])
    assert torch.equal(geo["weights"], full["weights"])
    assert torch.equal(geo["raw"], full["raw"][..., 3])
    assert torch.equal(geo["pts"], full["pts"])
    assert torch.equal(geo["kstats"], ext["kstats"][:, 6:12])
    # kstats alone (no per-K map), through cfnerf_render_fwd and through cfnerf_render_eval
    only = _render_geometry_fwd(net, packed, tv, eps, gflags, z_vals=z, maps=False, kstats=True)
    assert torch.equal(only["kstats"], geo["kstats"])
    if z is None:
        ks = torch.full((N, 6), SENTINEL, device=DEV)
        L.check(L.lib().cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(tv), L.ptr(eps), N, S, K, gflags, None, L.ptr(ks), None, L.stream()),
                "render_eval geometry")
        assert torch.equal(ks, geo["kstats"])
    again = _render_geometry_fwd(net, packed, tv, eps, gflags, z_vals=z, raw=True, weights=True, kstats=True)          # 5. determinism
    for k in ("depth_map", "disp_map", "weights", "raw", "kstats"):
        assert torch.equal(again[k], geo[k]), k


# ---------------------------------------------------------------------------------------------- 4. ray mode, the real reference
def test_render_geometry_vs_reference_golden(golden):
    g = golden("g6_render_c2w")
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    _, _, kw_test, model, p, _ = build_model(cfg, int(g["seed"]))
    net = model.module
    net.sample_alpha = T(g["eps_alpha"]).clone()
    net.sample_rgb = T(g["eps_rgb"]).clone()
    H, W, focal = int(g["H"]), int(g["W"]), float(g["focal"])
    packed = _pack_rays(H, W, focal, c2w=T(g["c2w"]), n=H * W, pixel0=0, ndc=True, near=0., far=1., device=net.device)
    o = render_geometry(packed, model, weights=True)
    assert set(o) == {"depth_map", "disp_map", "weights"} and list(o["weights"].shape) == [H * W, 128, 4]
    close(o["depth_map"].reshape(H, W, 4), g["depth_map"], ATOL, RTOL, what="depth_map")
    close(o["disp_map"].reshape(H, W, 4), g["disp_map"], atol=ATOL_DISP, rtol=1e-3, what="disp_map")
    with torch.no_grad():
        _, disp, depth, _ = cfnerf_amd.render(H, W, focal, chunk=8192, c2w=T(g["c2w"]), near=0., far=1., **kw_test)
    assert torch.equal(o["depth_map"].reshape(H, W, 4), depth) and torch.equal(o["disp_map"].reshape(H, W, 4), disp)
    assert set(render_geometry(packed, model)) == {"depth_map", "disp_map"}


def test_render_geometry_with_explicit_depths_needs_no_sample_table():
    """``render_geometry(z_vals=...)`` with the default ``t_vals=None``, and with a table of another length: the geometry-only kernel does
    not read the table when depths are given (S comes from ``z_vals``).  Yardstick: the launch without the flag, handed a table of length S."""
    W, K, N, S = 64, 3, 5, 70                                            # a ragged second tile
    model, net = _model(W, K)
    packed, (near, far) = _rays(net, N, True)
    g = torch.Generator().manual_seed(9)
    z = (near + (far - near) * torch.sort(torch.rand(N, S, generator=g), -1)[0]).to(DEV).contiguous()
    full = _render_fwd(net, packed, torch.linspace(0., 1., S, device=DEV), None, net.eval_eps(), 0, z_vals=z, weights=True, entropy=False)
    for tv in (None, torch.linspace(0., 1., 3, device=DEV), torch.linspace(0., 1., 128, device=DEV)):
        o = render_geometry(packed, model, t_vals=tv, z_vals=z, weights=True)
        assert list(o["weights"].shape) == [N, S, K]
        for k in ("depth_map", "disp_map", "weights"):
            assert torch.equal(o[k], full[k]), (k, None if tv is None else tv.shape[0])
    lib, ks = L.lib(), torch.full((N, 6), SENTINEL, device=DEV)                                   # and through the raw ABI: t_vals NULL
    ext = _render_fwd(net, packed, torch.linspace(0., 1., S, device=DEV), None, net.eval_eps(), L.F_KSTATS_EXT, z_vals=z, maps=False, kstats=True,
                      entropy=False)
    L.check(lib.cfnerf_render_fwd(net.handle, L.ptr(packed), None, None, L.ptr(z), L.ptr(net.eval_eps()), N, S, K, G, None, None, None, None, None, None,
                                  L.ptr(ks), None, L.stream()), "render_fwd geometry, z_vals, no t_vals")
    assert torch.equal(ks, ext["kstats"][:, 6:12])
    with pytest.raises(ValueError, match="z_vals"):
        render_geometry(packed, model, z_vals=z[:N - 1])


# ---------------------------------------------------------------------------------------------- 5. tiling
def test_render_uncertainty_geometry_rows_and_ext_maps():
    model, net = _model(256, 4)
    H, W, focal = 7, 6, 11.0
    kw = dict(near=0., far=1., ndc=True)
    c2w = _pose(True)
    one = E.render_uncertainty(H, W, focal, c2w, model, stats="geometry", **kw)
    keys = {"depth_mean", "disp_mean", "depth_unc", "disp_unc", "acc_mean", "acc_unc"}
    assert set(one) == keys and all(list(v.shape) == [H, W] for v in one.values())
    parts = [E.render_uncertainty(H, W, focal, c2w, model, stats="geometry", rows=E.row_shard(H, rk, 2), **kw) for rk in range(2)]
    ext = E.render_uncertainty(H, W, focal, c2w, model, stats="ext", **kw)
    for k in keys:
        assert torch.equal(torch.cat([q[k] for q in parts], 0), one[k]), k
        assert torch.equal(one[k], ext[k]), k


# ---------------------------------------------------------------------------------------------- 6. density_grid
def test_density_grid_chunks_and_statistics():
    K = 4
    model, net = _model(64, K)
    lo, hi, res = (-1.0, -0.5, 0.0), (1.0, 0.75, 0.5), (5, 4, 3)
    out = E.density_grid(model, lo, hi, res, chunk=17, return_raw=True)          # 60 points: three full chunks and a ragged one
    assert list(out["alpha"].shape) == [5, 4, 3, K] and list(out["sigma_mean"].shape) == [5, 4, 3] == list(out["sigma_unc"].shape)
    axes = [torch.linspace(lo[d], hi[d], res[d], device=DEV) for d in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    emb, _ = cfnerf_amd.get_embedder(10)
    x = torch.cat([emb(pts), torch.zeros(pts.shape[0], 27, device=DEV)], -1).contiguous()
    zeroed = net.sample_alpha.clone()
    zeroed[-1] = 0
    with torch.no_grad():
        ref = net.sample(x, eps_alpha=zeroed)
        kept = net.sample(x)
    assert torch.equal(out["alpha"].reshape(-1, K), ref[..., 0])                 # eval latents: the last one zeroed
    own = E.density_grid(model, lo, hi, res, chunk=1 << 20, eps_alpha=net.sample_alpha, return_raw=True)
    assert torch.equal(own["alpha"].reshape(-1, K), kept[..., 0]) and set(E.density_grid(model, lo, hi, res)) == {"sigma_mean", "sigma_unc"}
    a = out["alpha"].cpu().double().numpy()
    sigma = np.where(a > 20, a, np.log1p(np.exp(np.minimum(a, 20))))
    close(out["sigma_mean"], sigma.mean(-1), atol=1e-6, rtol=1e-5, what="sigma_mean")
    close(out["sigma_unc"], np.std(sigma, -1) * K / (K - 1), atol=1e-6, rtol=1e-4, what="sigma_unc")


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_the_flag_and_leave_the_handle_usable():
    W, K, P = 64, 2, 65
    model, net = _model(W, K)
    lib, h, s = L.lib(), net.handle, L.stream()
    x, eps = _points_inputs(P, K, 3)
    _, good = _points_pair(net, x, eps, K)
    N, S = 3, 16
    packed, _ = _rays(net, N, True)
    tv = torch.linspace(0., 1., S, device=DEV)
    buf = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    raw, ent, rows = buf(P, K), buf(1), torch.zeros(P, K, 4, device=DEV)
    rgb, disp, depth, ks, gt, sq = buf(N, 3, K), buf(N, K), buf(N, K), buf(N, 6), buf(N, 3), buf(N, 3)
    P_ = L.ptr

    def refused(rc, *names):
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0, (rc, names)
        for n in ("CFNERF_F_GEOMETRY",) + names:
            assert n in msg, (n, msg)

    for bit, name in ((L.F_TRAIN, "CFNERF_F_TRAIN"), (L.F_STASH, "CFNERF_F_STASH"), (L.F_EPS_ROWS, "CFNERF_F_EPS_ROWS"), (L.F_KSTATS_EXT, "CFNERF_F_KSTATS_EXT")):
        refused(lib.cfnerf_network_fwd(h, P_(x), P_(rows if bit == L.F_EPS_ROWS else eps), P, K, G | bit, P_(raw), P_(ent), s), name)
        refused(lib.cfnerf_render_fwd(h, P_(packed), P_(tv), None, None, P_(eps), N, S, K, G | bit, None, P_(disp), P_(depth), None, None, None, P_(ks),
                                      P_(ent), s), name)
        refused(lib.cfnerf_render_eval(h, P_(packed), P_(tv), P_(eps), N, S, K, G | bit, None, P_(ks), None, s), name)
    fwd = lambda r, di, de, k_: lib.cfnerf_render_fwd(h, P_(packed), P_(tv), None, None, P_(eps), N, S, K, G, r, di, de, None, None, None, k_, None, s)
    refused(fwd(P_(rgb), P_(disp), P_(depth), None), "rgb_map")
    refused(fwd(None, P_(disp), None, P_(ks)), "disp_map", "depth_map")
    refused(fwd(None, None, P_(depth), None), "disp_map", "depth_map")
    refused(lib.cfnerf_render_eval(h, P_(packed), P_(tv), P_(eps), N, S, K, G, P_(gt), P_(ks), P_(sq), s), "gt_opt", "sqerr_opt")
    refused(lib.cfnerf_render_eval(h, P_(packed), P_(tv), P_(eps), N, S, K, G, P_(gt), P_(ks), None, s), "gt_opt")
    # the K-statistics need K >= 2
    _, net1 = _model(64, 1)
    packed1, _ = _rays(net1, N, True)
    e1, k1 = net1.eval_eps(), buf(N, 6)
    refused(lib.cfnerf_render_fwd(net1.handle, P_(packed1), P_(tv), None, None, P_(e1), N, S, 1, G, None, None, None, None, None, None, P_(k1), None, s), "K >= 2")
    refused(lib.cfnerf_render_eval(net1.handle, P_(packed1), P_(tv), P_(e1), N, S, 1, G, None, P_(k1), None, s), "K >= 2")
    # the refusals are argument checks in front of any launch: nothing was written, and the next valid launch gives the bits it gave before
    torch.cuda.synchronize()
    for t in (raw, ent, rgb, disp, depth, ks, sq, k1):
        assert bool((t == SENTINEL).all())
    _, after = _points_pair(net, x, eps, K)
    assert torch.equal(after, good)
