"""-m gpu: rendering through an occupancy grid (CFNERF_F_CULL): the cull kernels of cfnerf_sample_points, the sparse composite of
cfnerf_composite_fwd, ``api.render_rays_culled`` end to end, ``render_uncertainty(occupancy=)`` and the refusals.

Every comparison is ``torch.equal``: the cull path is held to the plain sampling call and to a torch restatement of the cell formula, the
sparse composite to the dense composite on the scattered raw whose culled samples carry the density latent -1e4, the end-to-end render to
the existing unfused pipeline."""
import ctypes as C

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E
from cfnerf_amd.api import _pack_rays, _sample_points
from oracle import cfnerf_oracle as O
from util_hip import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
LO, HI, RES = (-1.0, -0.8, -1.2), (1.0, 0.9, 1.1), (4, 3, 5)


def _mask(seed=0):
    m = torch.rand(RES, generator=torch.Generator().manual_seed(seed)) < 0.5
    m[:, 1, 2] = False                       # an empty column of cells along x ...
    m[:, 0, 0] = True                        # ... and a full one
    return m


def _cull_rays():
    """[6,11]: 0 entirely outside the box; 1 along the empty column (keeps nothing); 2 along the full column (keeps everything), both with
    samples exactly on cell faces; 3..5 cross box faces obliquely.  near = 0.5, far = 2.5 (> 0: CFNERF_F_LINDISP divides by them)."""
    cy = lambda i: LO[1] + (i + 0.5) * (HI[1] - LO[1]) / RES[1]
    cz = lambda i: LO[2] + (i + 0.5) * (HI[2] - LO[2]) / RES[2]
    o = [[5.0, 5.0, 5.0], [-1.5, cy(1), cz(2)], [-1.5, cy(0), cz(0)], [-1.6, -1.0, -1.5], [0.2, 1.5, 0.3], [1.4, -0.1, 1.6]]
    d = [[1.0, 0.5, 0.25], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.7, 0.9], [-0.1, -1.0, -0.2], [-1.2, 0.1, -1.1]]
    o, d = torch.tensor(o), torch.tensor(d)
    rays = torch.cat([o, d, torch.full((6, 1), 0.5), torch.full((6, 1), 2.5), d / d.norm(dim=-1, keepdim=True)], -1)
    return rays.to(DEV).contiguous()


def _keep_restated(pts, mask, outside):
    """the header's cell formula in torch fp32 on the plain call's pts [N,S,3]: floor((p - lo) * scale), inside iff 0 <= t < res"""
    g = E.OccupancyGrid.from_mask(mask, LO, HI)
    lo, scale = torch.tensor(g.lo, device=pts.device), torch.tensor(g.scale, device=pts.device)
    res = torch.tensor(g.res, device=pts.device)
    t = torch.floor((pts - lo) * scale)
    inside = ((t >= 0) & (t < res)).all(-1)
    i = torch.where(inside[..., None], t, torch.zeros_like(t)).long()
    occ = mask.to(pts.device)[i[..., 0], i[..., 1], i[..., 2]]
    on_face = (((pts - lo) * scale) == t).any(-1) & inside
    return torch.where(inside, occ, torch.full_like(occ, outside == 0)), on_face


def _cull_call(rays, tv, tr, lindisp, grid, outside):
    """cfnerf_sample_points with CFNERF_F_CULL into sentinel-filled buffers"""
    N, S = rays.shape[0], tv.shape[0]
    z = torch.full((N, S), SENTINEL, device=DEV)
    slot = torch.full((N, S), -99, dtype=torch.int32, device=DEV)
    ray_start = torch.full((N + 1,), -99, dtype=torch.int64, device=DEV)
    pts_c = torch.full((N * S, 3), SENTINEL, device=DEV)
    ray_of = torch.full((N * S,), -99, dtype=torch.int32, device=DEV)
    f3 = lambda v: (C.c_float * 3)(*(float(x) for x in v))
    d = L.Cull(L.dptr(grid.bits_on(rays.device)), f3(grid.lo), f3(grid.scale), (C.c_int32 * 3)(*grid.res), outside, L.dptr(slot), L.dptr(ray_start),
               L.dptr(pts_c), L.dptr(ray_of))
    L.check(L.lib().cfnerf_sample_points(L.ptr(rays), L.ptr(tv), L.ptr(tr), (L.F_LINDISP if lindisp else 0) | L.F_CULL, N, S, L.ptr(z),
                                         L.struct_arg(d), L.stream()), "cfnerf_sample_points")
    return z, slot, ray_start, pts_c, ray_of


# ---------------------------------------------------------------------------------------------- 1. the cull kernels
@pytest.mark.parametrize("S", [1, 16, 64, 65, 130])
def test_cull_matches_the_plain_call_and_the_restated_cell_formula(S):
    mask = _mask()
    grid = E.OccupancyGrid.from_mask(mask, LO, HI)
    rays = _cull_rays()
    N = rays.shape[0]
    tv = torch.linspace(0., 1., S, device=DEV)
    jitter = torch.rand(N, S, generator=torch.Generator().manual_seed(S)).to(DEV)
    seen_face = False
    for tr in (None, jitter):
        for lindisp in (False, True):
            z0, pts0 = _sample_points(rays, tv, tr, lindisp)
            for outside in (0, 1):
                z, slot, ray_start, pts_c, ray_of = _cull_call(rays, tv, tr, lindisp, grid, outside)
                what = (S, tr is not None, lindisp, outside)
                assert torch.equal(z, z0), what
                keep, on_face = _keep_restated(pts0, mask, outside)
                seen_face |= bool(on_face.any())
                assert torch.equal(slot >= 0, keep), what
                count = int(keep.sum())
                assert torch.equal(slot[keep].long(), torch.arange(count, device=DEV)), what           # (ray, sample) order
                assert torch.equal(slot[~keep], torch.full_like(slot[~keep], -1)), what
                per_ray = keep.sum(1)
                assert torch.equal(ray_start, torch.cat([per_ray.new_zeros(1), per_ray.cumsum(0)])), what
                assert int(ray_start[N]) == count
                assert torch.equal(pts_c[:count], pts0[keep]), what
                assert torch.equal(ray_of[:count].long(), torch.arange(N, device=DEV)[:, None].expand(N, S)[keep]), what
                assert bool((pts_c[count:] == SENTINEL).all()) and bool((ray_of[count:] == -99).all()), what
                assert int(per_ray[0]) == (S if outside == 0 else 0), what                             # entirely outside the box
                if outside == 1:
                    assert int(per_ray[1]) == 0, what                                                  # inside: empty cells; outside: culled
                else:
                    assert int(per_ray[2]) == S, what                                                  # inside: full cells; outside: kept
    if S == 65:
        assert seen_face                     # samples exactly on cell faces took part (rays 1 and 2 without jitter: x = -1 + i / 32)


def test_cull_points_returns_the_kernels_outputs():
    mask = _mask(3)
    grid = E.OccupancyGrid.from_mask(mask, LO, HI)               # (bits on the CPU: uploaded by cull_points)
    rays, tv = _cull_rays(), torch.linspace(0., 1., 65, device=DEV)
    z, slot, ray_start, pts_c, ray_of = _cull_call(rays, tv, None, False, grid, 1)
    c = A.cull_points(rays, grid, t_vals=tv, outside="cull")
    n = c['count']
    assert n == int(ray_start[-1]) and 0 < n < rays.shape[0] * 65
    assert torch.equal(c['z_vals'], z) and torch.equal(c['slot'], slot) and torch.equal(c['ray_start'], ray_start)
    assert list(c['pts'].shape) == [n, 3] and torch.equal(c['pts'], pts_c[:n]) and torch.equal(c['ray_of'], ray_of[:n])
    with pytest.raises(ValueError, match="outside"):
        A.cull_points(rays, grid, t_vals=tv, outside=1)
    empty = A.cull_points(rays[:0], grid, t_vals=tv)
    assert empty['count'] == 0 and list(empty['ray_start'].shape) == [1]


# ---------------------------------------------------------------------------------------------- 2. the sparse composite
def _sparse_case(N, S, K, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(N, S, generator=g) < 0.4
    mask[0] = False                                              # an empty ray
    mask[1] = True                                               # a full ray
    count = int(mask.sum())
    raw_c = torch.randn(count, K, 4, generator=g) * 2
    z = torch.sort(torch.rand(N, S, generator=g) * 4 + 2, -1).values
    rays_d = torch.randn(N, 3, generator=g)
    slot = torch.full((N, S), -1, dtype=torch.int32)
    slot[mask] = torch.arange(count, dtype=torch.int32)
    per_ray = mask.sum(1)
    ray_start = torch.cat([per_ray.new_zeros(1), per_ray.cumsum(0)])
    dense = torch.zeros(N, S, K, 4)
    dense[..., 3] = -1e4
    dense[mask] = raw_c
    return [t.to(DEV).contiguous() for t in (raw_c, slot, ray_start, z, rays_d, dense)]


def _dense_composite(raw, z, rays_d, white, want_w):
    N, S, K = raw.shape[:3]
    o = [torch.full((N, 3, K), SENTINEL, device=DEV), torch.full((N, K), SENTINEL, device=DEV), torch.full((N, K), SENTINEL, device=DEV),
         torch.full((N, S, K), SENTINEL, device=DEV) if want_w else None]
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw), L.ptr(z), L.ptr(rays_d), N, S, K, white, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]),
                                         L.stream()), "cfnerf_composite_fwd")
    return o


def _sparse_composite(raw_c, slot, ray_start, z, rays_d, K, white, want_w):
    N, S = z.shape
    o = [torch.full((N, 3, K), SENTINEL, device=DEV), torch.full((N, K), SENTINEL, device=DEV), torch.full((N, K), SENTINEL, device=DEV),
         torch.full((N, S, K), SENTINEL, device=DEV) if want_w else None]
    sp = L.SparseRaw(L.dptr(slot), L.dptr(ray_start), L.dptr(o[3]))
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw_c), L.ptr(z), L.ptr(rays_d), N, S, K, white | L.F_CULL, L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]),
                                         L.struct_arg(sp), L.stream()), "cfnerf_composite_fwd")
    return o


@pytest.mark.parametrize("K", [1, 4, 20, 70])                   # libm (K = 1, 4), hardware transcendentals (20, 70), two passes over the chunks (70)
@pytest.mark.parametrize("S", [1, 65, 130])
def test_sparse_composite_has_the_bits_of_the_dense_composite(S, K):
    N = 4
    raw_c, slot, ray_start, z, rays_d, dense = _sparse_case(N, S, K, 100 * S + K)
    for white in (0, 1):
        for want_w in (False, True):
            ref = _dense_composite(dense, z, rays_d, white, want_w)
            got = _sparse_composite(raw_c, slot, ray_start, z, rays_d, K, white, want_w)
            for name, a, b in zip(("rgb_map", "disp_map", "depth_map", "weights"), got, ref):
                if a is None:
                    assert b is None
                    continue
                assert not bool((a == SENTINEL).any()), (name, white, want_w)
                assert torch.equal(a, b), (name, white, want_w)
            assert bool((got[0][0] == float(white)).all())       # the empty ray is the background
    rgb, disp, w, depth = A.raw2outputs_sparse(raw_c, slot, ray_start, z, rays_d, white_bkgd=True, retweights=True)
    ref = _dense_composite(dense, z, rays_d, 1, True)
    assert torch.equal(rgb, ref[0]) and torch.equal(disp, ref[1]) and torch.equal(depth, ref[2]) and torch.equal(w, ref[3])
    assert A.raw2outputs_sparse(raw_c, slot, ray_start, z, rays_d)[2] is None


def test_raw2outputs_sparse_is_inference_only_and_names_raw2outputs():
    raw_c, slot, ray_start, z, rays_d, _ = _sparse_case(4, 16, 2, 1)
    with torch.enable_grad(), pytest.raises(RuntimeError, match="raw2outputs"):
        A.raw2outputs_sparse(raw_c.requires_grad_(True), slot, ray_start, z, rays_d)


# ---------------------------------------------------------------------------------------------- 3. end to end
W_, K_, S_, N_ = 64, 4, 65, 7
BOX_LO, BOX_HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)


@pytest.fixture(scope="module")
def scene():
    cfg = O.OracleCfg(netwidth=W_, K_samples=K_)
    _, _, _, model, _, _ = build_model(cfg, 4242)
    net = model.module
    net._sync()
    th, ph = np.deg2rad(30.0), np.deg2rad(-30.0)
    c2w = torch.tensor([[np.cos(th), -np.sin(th) * np.sin(ph), np.sin(th) * np.cos(ph), 4 * np.sin(th) * np.cos(ph)],
                        [0, np.cos(ph), np.sin(ph), 4 * np.sin(ph)],
                        [-np.sin(th), -np.cos(th) * np.sin(ph), np.cos(th) * np.cos(ph), 4 * np.cos(th) * np.cos(ph)]], dtype=torch.float32)
    rays = _pack_rays(6, 5, 7.0, c2w=c2w, n=N_, pixel0=11, ndc=False, near=2., far=6., device=net.device)
    return model, net, c2w, rays, torch.linspace(0., 1., S_, device=DEV)


def _embed_points(net, pts, viewdirs):
    """x [P,90] of points [P,3] and their view directions [P,3], through the embedders of the unfused path"""
    emb, _ = cfnerf_amd.get_embedder((net.input_ch - 3) // 6)
    embd, _ = cfnerf_amd.get_embedder((net.input_ch_views - 3) // 6)
    return torch.cat([emb(pts), embd(viewdirs)], -1).contiguous()


@pytest.mark.parametrize("white", [False, True])
def test_all_ones_grid_has_the_bits_of_the_unfused_pipeline(scene, white):
    model, net, _, rays, tv = scene
    grid = E.OccupancyGrid.from_mask(torch.ones(3, 4, 2, dtype=torch.bool), BOX_LO, BOX_HI)
    got = A.render_rays_culled(rays, model, grid, t_vals=tv, white_bkgd=white, retweights=True)
    assert got['count'] == N_ * S_                               # the compact list is the dense list in the same order
    with torch.no_grad():
        z, pts = _sample_points(rays, tv, None, False)
        x = _embed_points(net, pts.reshape(-1, 3), rays[:, None, 8:11].expand(N_, S_, 3).reshape(-1, 3))
        raw = model(x, False, True)[0].reshape(N_, S_, K_, 4)
        rgb, disp, w, depth = A.raw2outputs(raw, z, rays[:, 3:6], 0., white)
    assert torch.equal(got['rgb_map'], rgb) and torch.equal(got['disp_map'], disp) and torch.equal(got['depth_map'], depth)
    assert torch.equal(got['weights'], w)


def test_random_grid_has_the_bits_of_the_scatter_oracle(scene):
    model, net, _, rays, tv = scene
    mask = torch.rand(5, 6, 4, generator=torch.Generator().manual_seed(9)) < 0.5
    grid = E.OccupancyGrid.from_mask(mask.to(DEV), BOX_LO, BOX_HI)            # (a GPU mask: bits packed on the device)
    got = A.render_rays_culled(rays, model, grid, t_vals=tv, outside="cull", retweights=True)
    c = A.cull_points(rays, grid, t_vals=tv, outside="cull")
    keep = c['slot'] >= 0
    assert 0 < got['count'] == c['count'] < N_ * S_
    with torch.no_grad():
        x_c = _embed_points(net, c['pts'], rays[c['ray_of'].long(), 8:11])
        raw_c = model(x_c, False, True)[0]
        dense = torch.zeros(N_, S_, K_, 4, device=DEV)
        dense[..., 3] = -1e4
        dense[keep] = raw_c
        rgb, disp, w, depth = A.raw2outputs(dense, c['z_vals'], rays[:, 3:6], 0., False)
    assert torch.equal(got['rgb_map'], rgb) and torch.equal(got['disp_map'], disp) and torch.equal(got['depth_map'], depth)
    assert torch.equal(got['weights'], w) and bool((w[~keep] == 0).all())


@pytest.mark.parametrize("white", [False, True])
def test_all_zero_grid_is_the_background_without_a_network_launch(scene, white, monkeypatch):
    model, net, _, rays, tv = scene
    calls = []
    forward = net.forward
    monkeypatch.setattr(net, "forward", lambda *a, **k: (calls.append(1), forward(*a, **k))[1])
    grid = E.OccupancyGrid.from_mask(torch.zeros(3, 4, 2, dtype=torch.bool), BOX_LO, BOX_HI)
    got = A.render_rays_culled(rays, model, grid, t_vals=tv, white_bkgd=white, outside="cull")
    assert got['count'] == 0 and not calls
    assert bool((got['rgb_map'] == float(white)).all()) and bool((got['depth_map'] == 0).all())
    z, _ = _sample_points(rays, tv, None, False)
    dense = torch.zeros(N_, S_, K_, 4, device=DEV)
    dense[..., 3] = -1e4
    rgb, disp, _, depth = A.raw2outputs(dense, z, rays[:, 3:6], 0., white)
    assert torch.equal(got['rgb_map'], rgb) and torch.equal(got['disp_map'], disp) and torch.equal(got['depth_map'], depth)


# ---------------------------------------------------------------------------------------------- 4. render_uncertainty(occupancy=)
def test_render_uncertainty_through_a_grid(scene, monkeypatch):
    model, net, c2w, _, tv = scene
    H, Wd, focal, rows = 6, 5, 7.0, (1, 4)
    mask = torch.rand(5, 6, 4, generator=torch.Generator().manual_seed(2)) < 0.6
    grid = E.OccupancyGrid.from_mask(mask, BOX_LO, BOX_HI)
    gt = torch.rand(rows[1] - rows[0], Wd, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(near=2., far=6., ndc=False, t_vals=tv, rows=rows, occupancy=grid)
    out = E.render_uncertainty(H, Wd, focal, c2w, model, gt=gt, want_maps=True, **kw)
    n = (rows[1] - rows[0]) * Wd
    rays = _pack_rays(H, Wd, focal, c2w=c2w, n=n, pixel0=rows[0] * Wd, ndc=False, near=2., far=6., device=net.device)
    ref = A.render_rays_culled(rays, model, grid, t_vals=tv)
    assert 0 < out['kept_samples'] == ref['count'] < n * S_
    m, u, dm, zm = E.k_stats(ref['rgb_map'], ref['disp_map'], ref['depth_map'])
    h = rows[1] - rows[0]
    assert torch.equal(out['rgb_mean'], m.reshape(h, Wd, 3)) and torch.equal(out['rgb_unc'], u.reshape(h, Wd, 3))
    assert torch.equal(out['disp_mean'], dm.reshape(h, Wd)) and torch.equal(out['depth_mean'], zm.reshape(h, Wd))
    assert torch.equal(out['rgb_map'], ref['rgb_map'].reshape(h, Wd, 3, K_)) and torch.equal(out['depth_map'], ref['depth_map'].reshape(h, Wd, K_))
    sq = (m.reshape(h, Wd, 3) - gt) ** 2
    assert torch.equal(out['sq_err'], sq) and torch.equal(out['mse'], sq.mean())
    plain = E.render_uncertainty(H, Wd, focal, c2w, model, **kw)
    assert set(plain) == {"rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "kept_samples"} and torch.equal(plain['rgb_mean'], out['rgb_mean'])
    # bounded chunks: the rays are walked 7 at a time, each chunk one render_rays_culled call
    monkeypatch.setattr(E, "_CULL_RAY_CHUNK", 7)
    parts = [A.render_rays_culled(rays[i:i + 7], model, grid, t_vals=tv) for i in range(0, n, 7)]
    chunked = E.render_uncertainty(H, Wd, focal, c2w, model, want_maps=True, **kw)
    assert torch.equal(chunked['rgb_map'].reshape(n, 3, K_), torch.cat([p['rgb_map'] for p in parts]))
    assert chunked['kept_samples'] == sum(p['count'] for p in parts) == ref['count']
    for stats in ("ext", "geometry"):
        with pytest.raises(ValueError, match="acc_map"):
            E.render_uncertainty(H, Wd, focal, c2w, model, stats=stats, **kw)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_the_flag_and_leave_the_handle_usable(scene):
    model, net, _, rays, tv = scene
    lib, h, s, P_ = L.lib(), net.handle, L.stream(), L.ptr
    N, S, K = N_, S_, K_
    eps = net.eval_eps()
    x = (torch.rand(33, 90, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)

    def network():
        raw = torch.full((33, K, 4), SENTINEL, device=DEV)
        L.check(lib.cfnerf_network_fwd(h, P_(x), P_(eps), 33, K, 0, P_(raw), None, s), "cfnerf_network_fwd")
        return raw

    good = network()
    raw_c, slot, ray_start, z, rays_d, dense = _sparse_case(4, 16, K, 8)
    good_c = _sparse_composite(raw_c, slot, ray_start, z, rays_d, K, 0, False)
    buf = lambda *shape: torch.full(shape, SENTINEL, device=DEV)
    raw, rgb, disp, depth, ks = buf(33, K, 4), buf(N, 3, K), buf(N, K), buf(N, K), buf(N, 8)

    def refused(rc, *names):
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0, (rc, names)
        for n in ("CFNERF_F_CULL",) + names:
            assert n in msg, (n, msg)

    refused(lib.cfnerf_render_fwd(h, P_(rays), P_(tv), None, None, P_(eps), N, S, K, L.F_CULL, P_(rgb), P_(disp), P_(depth), None, None, None, None,
                                  None, s), "cfnerf_render_fwd")
    refused(lib.cfnerf_render_eval(h, P_(rays), P_(tv), P_(eps), N, S, K, L.F_CULL, None, P_(ks), None, s), "cfnerf_render_eval")
    refused(lib.cfnerf_network_fwd(h, P_(x), P_(eps), 33, K, L.F_CULL, P_(raw), None, s), "cfnerf_network_fwd")
    o = [buf(4, 3, K), buf(4, K), buf(4, K)]
    sp = L.SparseRaw(None, L.dptr(ray_start), None)
    refused(lib.cfnerf_composite_fwd(P_(raw_c), P_(z), P_(rays_d), 4, 16, K, L.F_CULL, P_(o[0]), P_(o[1]), P_(o[2]), L.struct_arg(sp), s), "slot")
    refused(lib.cfnerf_composite_fwd(P_(raw_c), P_(z), P_(rays_d), 4, 16, K, L.F_CULL | 1, P_(o[0]), P_(o[1]), P_(o[2]), None, s), "cfnerf_sparse_raw")
    # argument checks in front of any launch: nothing was written, and the next valid launches give the bits they gave before
    torch.cuda.synchronize()
    for t in [raw, rgb, disp, depth, ks] + o:
        assert bool((t == SENTINEL).all())
    assert torch.equal(network(), good)
    again = _sparse_composite(raw_c, slot, ray_start, z, rays_d, K, 0, False)
    assert all(torch.equal(a, b) for a, b in zip(again[:3], good_c[:3]))
    # the background is white iff (white_bkgd & ~0x800) != 0: the dense call ignores nothing a caller passes today
    assert torch.equal(_dense_composite(dense, z, rays_d, 4, False)[0], _dense_composite(dense, z, rays_d, 1, False)[0])
    assert torch.equal(_sparse_composite(raw_c, slot, ray_start, z, rays_d, K, 4, False)[0], _dense_composite(dense, z, rays_d, 1, False)[0])
