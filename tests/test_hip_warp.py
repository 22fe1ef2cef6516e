"""-m gpu: sampling through an occupancy grid on the fused path (``evaluate.OccupancySampler``): the probes and the depth warp of
``api.warp_z_vals`` against their CPU restatements, ``api.render_rays_warped`` and ``Trainer.forward_backward(occupancy=)`` against the fp64
oracle composed on the depths they used (``oracle.render_rays(z_vals=)``, the fine pass of ``oracle.render_rays_hierarchical``),
``render_uncertainty(occupancy=sampler)`` against the per-K maps, and the refusal."""
import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E
from cfnerf_amd import train as TR
from cfnerf_amd.api import _pack_rays, _sample_points
from oracle import cfnerf_oracle as O
from test_hip_cull import HI, LO, _cull_rays
from util_hip import ATOL_DISP, build_model, close, grad_close_tight, hip_relu_masks
from warp_common import check_warp

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_, K_ = 64, 4
NEAR, FAR = 0.5, 2.5                                  # of the six-ray set


def _slab_mask():
    """8 x 8 x 8 cells on the box of tests/test_hip_cull.py: a slab two cells thick across x, with a hole along the column that ray 1 of the
    six-ray set travels in (the ray runs on the face between cells 3 and 4 in y and in z: all four columns around it are empty)"""
    m = torch.zeros(8, 8, 8, dtype=torch.bool)
    m[3:5] = True
    m[:, 3:5, 3:5] = False
    return m


def _grid(mask=None):
    return E.OccupancyGrid.from_mask(_slab_mask() if mask is None else mask, LO, HI)


def _rays8():
    """rays_o, rays_d [8,3]: the six-ray set and two more oblique rays through the slab"""
    six = _cull_rays().cpu()
    o = torch.cat([six[:, 0:3], torch.tensor([[-1.4, 0.85, -0.9], [0.1, -0.7, -1.6]])])
    d = torch.cat([six[:, 3:6], torch.tensor([[1.0, -0.3, 0.5], [-0.4, 0.3, 1.0]])])
    return o.contiguous(), d.contiguous()


# ---------------------------------------------------------------------------------------------- 1. probes and warp
@pytest.mark.parametrize("S", [16, 65])
def test_probes_bins_and_warp_against_the_cpu_restatements(S):
    rays = _cull_rays()
    N = rays.shape[0]
    grid = _grid()
    tv = torch.linspace(0., 1., S, device=DEV)
    jitter = torch.rand(N, S, generator=torch.Generator().manual_seed(S)).to(DEV)
    seen_face = False
    for bins, pad, outside in ((16, 1, "cull"), (64, 0, "cull"), (16, 0, "keep"), (512, 2, "cull")):
        sampler = grid.sampler(bins=bins, pad=pad, outside=outside)
        # the CPU restatement: the cell rule in fp32 torch on the probe points of the plain sampling call, then the bin rule
        _, pts = _sample_points(rays, torch.linspace(0., 1., 2 * bins + 1).to(DEV), None, False)
        pts = pts.cpu()
        occ = A.probe_occupancy_reference(pts, grid, outside)
        want = A.bins_from_probes(occ, pad)
        assert np.array_equal(want.numpy(), A.bins_from_probes_reference(occ.numpy(), pad))
        cellf = (pts - torch.tensor(grid.lo)) * torch.tensor(grid.scale)
        seen_face |= bool(((cellf == torch.floor(cellf)).any(-1) & occ).any())
        for tr in (None, jitter):
            for lindisp in (False, True):
                what = f"S={S} bins={bins} pad={pad} outside={outside} jitter={tr is not None} lindisp={lindisp}"
                w = A.warp_z_vals(rays, sampler, tv, tr, lindisp)
                assert w['bins'].dtype == torch.bool and torch.equal(w['bins'].cpu(), want), what
                z_plain, _ = _sample_points(rays, tv, tr, lindisp)
                warped = check_warp(w['z_vals'], w['n_occ'], z_plain, rays[:, 6], rays[:, 7], w['bins'], what)
                if outside == "cull":
                    assert not warped[0] and not warped[1], what            # outside the box / along the empty column: the plain depths' bits
                    assert int(w['n_occ'][0]) == 0 and int(w['n_occ'][1]) == 0
                    assert warped[2:].all(), what                          # the others cross the slab: some bins, not all
                else:
                    assert int(w['n_occ'][0]) == bins and not warped[0], what
                again = A.warp_z_vals(rays, sampler, tv, tr, lindisp)
                assert torch.equal(again['z_vals'], w['z_vals']) and torch.equal(again['n_occ'], w['n_occ'])
    assert seen_face                                   # occupied probes exactly on cell faces took part (ray 2: x = -1 + j / bins)
    # an all-ones grid: every ray inside it keeps the plain depths; with outside="keep" every ray does
    full = _grid(torch.ones(8, 8, 8, dtype=torch.bool)).sampler(bins=16, outside="keep")
    for tr in (None, jitter):
        z_plain, _ = _sample_points(rays, tv, tr, True)
        w = A.warp_z_vals(rays, full, tv, tr, True)
        assert torch.equal(w['z_vals'], z_plain) and bool((w['n_occ'] == 16).all()) and bool(w['bins'].all())
    empty = A.warp_z_vals(rays[:0], full, tv)
    assert list(empty['z_vals'].shape) == [0, S] and list(empty['bins'].shape) == [0, 16]


def test_probe_launches_are_chunked_under_the_byte_bound(monkeypatch):
    rays = torch.cat([_cull_rays()] * 3)
    sampler = _grid().sampler(bins=16)
    tv = torch.linspace(0., 1., 16, device=DEV)
    one = A.warp_z_vals(rays, sampler, tv)
    monkeypatch.setattr(A, "_WARP_PROBE_BYTES", 4 * 33 * 24)                 # four rays per probe launch: 18 rays in five launches
    assert A.warp_probe_chunk(16) == 4
    parts = A.warp_z_vals(rays, sampler, tv)
    assert all(torch.equal(one[k], parts[k]) for k in one)


# ---------------------------------------------------------------------------------------------- 2. render_rays_warped against the oracle
@pytest.fixture(scope="module")
def scene():
    cfg = O.OracleCfg(netwidth=W_, K_samples=K_)
    _, kw_train, _, model, p, optimizer = build_model(cfg, 1515, no_ndc=True)
    g = torch.Generator().manual_seed(15)
    d = dict(ea=torch.randn(K_, 1, generator=g), er=torch.randn(K_, 3, generator=g), target=torch.rand(8, 3, generator=g),
             t_rand=torch.rand(8, 65, generator=g), target_depth=0.8 + torch.rand(3, generator=g))
    return cfg, model, model.module, p, optimizer, d


def _oracle64(p, packed, cfg, ea, er, is_train, z, white=False, masks=None, leaves=False):
    """the fp64 oracle composed on the depths ``z`` the launch used: run_network + raw2outputs on pts = o + d z (``O.render_rays(z_vals=)``)"""
    q = {k: v.double().clone().requires_grad_(leaves) for k, v in p.items()}
    import contextlib
    with (O.relu_override(masks=masks) if masks is not None else contextlib.nullcontext()):
        ret = O.render_rays(q, packed.double(), cfg, ea.double(), er.double(), is_train, None, False, white, z_vals=z.detach().cpu().double())
    return q, ret


def _check_grads(net, g_hip, q):
    g_hip = g_hip.detach().cpu()
    n = 0
    for key, (off, cnt) in net.layout.items():
        if q[key].grad is None:
            assert not g_hip[off:off + cnt].any(), key
        else:
            grad_close_tight(g_hip[off:off + cnt].reshape(q[key].grad.shape), q[key].grad.numpy(), "grad " + key)
            n += 1
    assert n >= 30


@pytest.mark.parametrize("S,white", [(16, True), (65, False)])
def test_eval_render_matches_the_oracle_on_the_returned_depths(scene, S, white):
    cfg, model, net, p, _, d = scene
    rays = _cull_rays()
    sampler = _grid().sampler(bins=16)
    tv = torch.linspace(0., 1., S, device=DEV)
    with torch.no_grad():
        got = A.render_rays_warped(rays, model, sampler, False, white_bkgd=white, t_vals=tv, retweights=True)
    assert set(got) == {"rgb_map", "disp_map", "depth_map", "weights", "z_vals", "n_occ"}
    w = A.warp_z_vals(rays, sampler, tv)
    assert torch.equal(got['z_vals'], w['z_vals']) and torch.equal(got['n_occ'], w['n_occ']) and 0 < int(got['n_occ'][2]) < 16
    ea, er = net.sample_alpha.clone(), net.sample_rgb.clone()
    ea[-1] = 0
    er[-1] = 0
    _, ref = _oracle64(p, rays.cpu(), cfg, ea, er, False, got['z_vals'], white)
    close(got['rgb_map'], ref['rgb_map'], what="rgb_map")
    close(got['depth_map'], ref['depth_map'], what="depth_map")
    close(got['disp_map'], ref['disp_map'], atol=ATOL_DISP, rtol=1e-3, what="disp_map")
    close(got['weights'], ref['weights'], what="weights")
    # not the plain render: the budget went into the slab
    with torch.no_grad():
        plain = cfnerf_amd.render_rays(rays, model, None, S, False, False, white_bkgd=white, t_vals=tv)
    close(got['rgb_map'][:2], plain['rgb_map'][:2], what="rays 0, 1 keep the plain depths")
    assert float((got['depth_map'][2:] - plain['depth_map'][2:]).abs().max()) > 1e-3


def test_train_render_under_autograd_matches_the_oracle_maps_and_gradients(scene):
    cfg, model, net, p, optimizer, d = scene
    rays = _cull_rays()
    N, S = rays.shape[0], 65
    sampler = _grid().sampler(bins=16)
    tv = torch.linspace(0., 1., S, device=DEV)
    ret = A.render_rays_warped(rays, model, sampler, True, perturb=1., t_rand=d["t_rand"][:N], eps_alpha=d["ea"], eps_rgb=d["er"], t_vals=tv)
    assert set(ret) == {"rgb_map", "disp_map", "depth_map", "raw", "loss_entropy", "pts", "z_vals", "n_occ"}
    assert ret["rgb_map"].requires_grad and not ret["z_vals"].requires_grad
    z_plain, _ = _sample_points(rays, tv, d["t_rand"][:N].to(DEV), False)
    check_warp(ret['z_vals'], ret['n_occ'], z_plain, rays[:, 6], rays[:, 7], A.warp_z_vals(rays, sampler, tv)['bins'], "train")

    def loss_of(r, dev):
        return torch.mean((r["rgb_map"].mean(-1) - d["target"][:N].to(dev)) ** 2) + 0.05 * torch.mean(r["depth_map"]) + 0.01 * r["loss_entropy"].mean()
    loss = loss_of(ret, DEV)
    optimizer.zero_grad()
    loss.backward()
    g_hip = net.flat.grad.clone()
    optimizer.zero_grad()
    _, masks = hip_relu_masks(net, N * S)
    q, ref = _oracle64(p, rays.cpu(), cfg, d["ea"], d["er"], True, ret['z_vals'], masks=masks, leaves=True)
    loss_o = loss_of(ref, "cpu")
    loss_o.backward()
    close(ret["rgb_map"], ref["rgb_map"], what="rgb_map")
    close(ret["depth_map"], ref["depth_map"], what="depth_map")
    close(ret["pts"], ref["pts"], what="pts")
    close(ret["raw"], ref["raw"], atol=1e-4, rtol=1e-4, what="raw")
    close(loss, loss_o, atol=1e-6, rtol=1e-5, what="loss")
    _check_grads(net, g_hip, q)


def test_rays_that_ask_for_a_gradient_get_one(scene):
    cfg, model, net, p, optimizer, d = scene
    rays = _cull_rays().clone().requires_grad_(True)
    ret = A.render_rays_warped(rays, model, _grid().sampler(bins=16), True, eps_alpha=d["ea"], eps_rgb=d["er"], t_vals=torch.linspace(0., 1., 16, device=DEV))
    ret["rgb_map"].sum().backward()
    optimizer.zero_grad()
    assert rays.grad is not None and bool(torch.isfinite(rays.grad).all()) and float(rays.grad[2:, 0:6].abs().max()) > 0
    assert not rays.grad[:, 6:8].any()                # near / far: not computed by the fused node; the warp's depths are constants


# ---------------------------------------------------------------------------------------------- 3. Trainer.forward_backward(occupancy=)
HWF = (8, 8, 7.0)
GEO = dict(near=NEAR, far=FAR, ndc=False)


def _oracle_step(net, p, cfg, d, z, S, beta1, n_colour=8, depth_lambda=0.0, o_d=None):
    """the train step's loss and gradient on the fp64 oracle at depths ``z`` and on the ReLU masks of the HIP forward just run"""
    o, dd = _rays8() if o_d is None else o_d
    packed = O.pack_rays(*HWF, o, dd, False, NEAR, FAR)
    _, masks = hip_relu_masks(net, packed.shape[0] * S)
    q, ret = _oracle64(p, packed, cfg, d["ea"], d["er"], True, z, masks=masks, leaves=True)
    L = O.train_loss(ret["rgb_map"][:n_colour], d["target"][:n_colour].double(), ret["loss_entropy"], K_, beta1)
    loss, depth_loss = L["loss"], None
    if depth_lambda:
        depth_loss = ((ret["depth_map"][n_colour:].mean(-1) - d["target_depth"].double()) ** 2).mean()
        loss = loss + depth_lambda * depth_loss
    loss.backward()
    return q, ret, dict(loss=loss.detach(), loss_nll=L["loss_nll"].detach(), mse=L["mse"].detach(), psnr=L["psnr"].detach(),
                        depth_loss=depth_loss)


def _fb(tr, d, S, occupancy=None, rays=None, n=8, **kw):
    o, dd = _rays8()
    rays = torch.stack([o, dd])[:, :n].to(DEV) if rays is None else rays
    eps = torch.cat([d["er"], d["ea"]], -1).to(DEV)
    return tr.forward_backward(*HWF, rays, d["target"][:n].to(DEV), t_rand=d["t_rand"][:, :S].contiguous().to(DEV), eps=eps,
                               t_vals=torch.linspace(0., 1., S, device=DEV), occupancy=occupancy, **GEO, **kw).clone()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_trainer_step_through_the_grid_matches_the_oracle(scene, precision):
    cfg, model, net, p, _, d = scene
    S, beta1 = 65, 0.01
    sampler = _grid().sampler(bins=16)
    net.set_precision(precision)
    try:
        tr = TR.Trainer(net, beta1=beta1)
        plain_before = _fb(tr, d, S)
        sc_before = tr.scalars.clone()
        grad = _fb(tr, d, S, occupancy=sampler)
        assert list(tr.z_vals.shape) == [8, S] and list(tr.n_occ.shape) == [8] and tr.n_occ.dtype == torch.int32
        assert int(tr.n_occ[0]) == 0 and int(tr.n_occ[1]) == 0 and bool(((tr.n_occ[2:] > 0) & (tr.n_occ[2:] < 16)).all())
        w = A.warp_z_vals(tr.packed, sampler, torch.linspace(0., 1., S, device=DEV), d["t_rand"][:, :S].contiguous().to(DEV))
        assert torch.equal(tr.z_vals, w['z_vals'])
        q, ret, sc = _oracle_step(net, p, cfg, d, tr.z_vals, S, beta1)
        close(tr.rgb_map, ret["rgb_map"], what="rgb_map")
        close(tr.depth, ret["depth_map"], what="depth_map")
        for i, k in enumerate(("loss", "loss_nll", "mse", "psnr")):
            close(tr.scalars[i].cpu(), sc[k], what=k)
        close(tr.entropy.cpu().reshape(()), ret["loss_entropy"].detach(), what="entropy")
        _check_grads(net, grad, q)
        assert float((grad - plain_before).abs().max()) > 1e-2 * float(grad.abs().max())            # not the plain step
        # a plain step after the warped one has the bits of the plain step before it: the shared buffers carry nothing over
        assert torch.equal(_fb(tr, d, S), plain_before) and torch.equal(tr.scalars, sc_before)
    finally:
        net.set_precision("fp32")


def test_sliced_step_equals_the_unsliced_step(scene):
    cfg, model, net, p, _, d = scene
    S = 65
    sampler = _grid().sampler(bins=16)
    whole = TR.Trainer(net, beta1=0.01)
    g_whole = _fb(whole, d, S, occupancy=sampler)
    sliced = TR.Trainer(net, beta1=0.01, max_rays_per_launch=4)
    g_sliced = _fb(sliced, d, S, occupancy=sampler)
    assert sliced.n_slices(8) == 2 and torch.equal(sliced.z_vals, whole.z_vals)
    grad_close_tight(g_sliced, g_whole.cpu().numpy(), "sliced against unsliced")
    close(sliced.scalars[:3].cpu(), whole.scalars[:3].cpu(), what="scalars")
    close(sliced.rgb_map, whole.rgb_map, what="rgb_map")
    # ray_grad=True: the same parameter gradient, and the ray blocks of the explicit-depth launch (d_z: to the warped depths)
    rg = TR.Trainer(net, beta1=0.01, ray_grad=True)
    g_rg = _fb(rg, d, S, occupancy=sampler)
    grad_close_tight(g_rg, g_whole.cpu().numpy(), "ray_grad=True against the default")
    assert list(rg.d_rays.shape) == [8, 11] and list(rg.d_z.shape) == [8, S] and bool(torch.isfinite(rg.d_rays).all())
    assert float(rg.d_rays[2:, 0:6].abs().max()) > 0 and float(rg.d_z.abs().max()) > 0 and not rg.d_rays[:, 6:8].any()


def test_depth_rays_through_the_grid_match_the_oracles_depth_term(scene):
    cfg, model, net, p, _, d = scene
    S, beta1, lam = 16, 0.01, 0.1
    sampler = _grid().sampler(bins=16)
    o, dd = _rays8()
    tr = TR.Trainer(net, beta1=beta1, depth_lambda=lam)
    eps = torch.cat([d["er"], d["ea"]], -1).to(DEV)
    # five colour rays, then rays 5..7 as depth rays: one launch of eight rows, the order of _rays8
    grad = tr.forward_backward(*HWF, torch.stack([o, dd])[:, :5].to(DEV), d["target"][:5].to(DEV), t_rand=d["t_rand"][:, :S].contiguous().to(DEV), eps=eps,
                               t_vals=torch.linspace(0., 1., S, device=DEV), depth_rays=torch.stack([o, dd])[:, 5:].to(DEV),
                               target_depth=d["target_depth"].to(DEV), occupancy=sampler, **GEO).clone()
    assert list(tr.z_vals.shape) == [8, S]
    q, ret, sc = _oracle_step(net, p, cfg, d, tr.z_vals, S, beta1, n_colour=5, depth_lambda=lam)
    close(tr.depth, ret["depth_map"], what="depth_map")
    close(tr.depth_loss.cpu().reshape(()), sc["depth_loss"], what="depth_loss")
    close(tr.scalars[0].cpu(), sc["loss"], what="loss")
    _check_grads(net, grad, q)


def test_netchunk_latents_follow_the_rays_through_the_grid(scene):
    """two network calls of four rays each, each with its own latent pair: the gradient is the mean of the two launch-mode steps on the
    halves (every loss term is a mean over the rays; beta1 = 0), at the depths the whole batch was warped to"""
    cfg, model, net, p, _, d = scene
    S = 16
    sampler = _grid().sampler(bins=16)
    o, dd = _rays8()
    rays = torch.stack([o, dd]).to(DEV)
    tv = torch.linspace(0., 1., S, device=DEV)
    t_rand = d["t_rand"][:, :S].contiguous().to(DEV)
    g2 = torch.Generator().manual_seed(2)
    pairs = torch.randn(2, K_, 4, generator=g2)
    nc = TR.Trainer(net, latent_draws="netchunk", netchunk=4 * S, chunk=None)
    g_nc = nc.forward_backward(*HWF, rays, d["target"].to(DEV), t_rand=t_rand, eps_chunks=pairs, t_vals=tv, occupancy=sampler, **GEO).clone()
    halves = []
    for c in range(2):
        tr = TR.Trainer(net)
        halves.append(tr.forward_backward(*HWF, rays[:, 4 * c:4 * c + 4].contiguous(), d["target"][4 * c:4 * c + 4].to(DEV),
                                          t_rand=t_rand[4 * c:4 * c + 4].contiguous(), eps=pairs[c].to(DEV), t_vals=tv, occupancy=sampler, **GEO).clone())
        assert torch.equal(tr.z_vals, nc.z_vals[4 * c:4 * c + 4])
    grad_close_tight(g_nc, (0.5 * (halves[0] + halves[1])).cpu().numpy(), "netchunk rows against the two launches")
    assert float((halves[0] - halves[1]).abs().max()) > 1e-2 * float(g_nc.abs().max())


# ---------------------------------------------------------------------------------------------- 4. render_uncertainty(occupancy=sampler)
def test_render_uncertainty_through_a_sampler(scene, monkeypatch):
    cfg, model, net, p, _, d = scene
    H, Wd, focal = 8, 8, 7.0
    th, ph = np.deg2rad(30.0), np.deg2rad(-30.0)
    c2w = torch.tensor([[np.cos(th), -np.sin(th) * np.sin(ph), np.sin(th) * np.cos(ph), 4 * np.sin(th) * np.cos(ph)],
                        [0, np.cos(ph), np.sin(ph), 4 * np.sin(ph)],
                        [-np.sin(th), -np.cos(th) * np.sin(ph), np.cos(th) * np.cos(ph), 4 * np.cos(th) * np.cos(ph)]], dtype=torch.float32)
    grid = E.OccupancyGrid.from_mask(_slab_mask(), (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    sampler = grid.sampler(bins=32)
    tv = torch.linspace(0., 1., 33, device=DEV)
    gt = torch.rand(H, Wd, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    kw = dict(near=2., far=6., ndc=False, t_vals=tv, occupancy=sampler)
    out = E.render_uncertainty(H, Wd, focal, c2w, model, gt=gt, **kw)
    assert set(out) == {"rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "occupied_bins", "sq_err", "mse"}
    rays = _pack_rays(H, Wd, focal, c2w=c2w, ndc=False, near=2., far=6., device=net.device)
    with torch.no_grad():
        ref = A.render_rays_warped(rays, model, sampler, False, t_vals=tv)
    n_occ = ref['n_occ']
    assert int((n_occ == 0).sum()) > 0 and int(((n_occ > 0) & (n_occ < 32)).sum()) > 0            # rays that miss the slab, rays that cross it
    m, u, dm, zm = E.k_stats(ref['rgb_map'], ref['disp_map'], ref['depth_map'])
    # (the tolerances of tests/test_hip_evaluate.py for the fused statistics against the per-K maps)
    close(out['rgb_mean'], m.reshape(H, Wd, 3), atol=1e-6, rtol=1e-5, what="rgb_mean")
    close(out['rgb_unc'], u.reshape(H, Wd, 3), atol=1e-6, rtol=1e-4, what="rgb_unc")
    close(out['disp_mean'], dm.reshape(H, Wd), atol=1e-5, rtol=1e-5, what="disp_mean")
    close(out['depth_mean'], zm.reshape(H, Wd), atol=1e-6, rtol=1e-5, what="depth_mean")
    assert torch.equal(out['occupied_bins'], (n_occ.to(torch.float32) / 32).mean()) and 0 < float(out['occupied_bins']) < 1
    close(out['sq_err'], (out['rgb_mean'] - gt) ** 2, atol=1e-7, rtol=1e-6, what="sq_err")
    assert torch.equal(out['mse'], out['sq_err'].mean())
    maps = E.render_uncertainty(H, Wd, focal, c2w, model, want_maps=True, **kw)
    assert torch.equal(maps['rgb_map'].reshape(H * Wd, 3, K_), ref['rgb_map']) and torch.equal(maps['rgb_mean'], out['rgb_mean'])
    part = E.render_uncertainty(H, Wd, focal, c2w, model, gt=gt[2:5], rows=(2, 5), **kw)
    for k in ("rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "sq_err"):
        assert torch.equal(part[k], out[k][2:5]), k
    assert torch.equal(part['occupied_bins'], (n_occ[16:40].to(torch.float32) / 32).mean())
    # bounded chunks: 7 rays per probe launch and render launch
    monkeypatch.setattr(A, "_WARP_PROBE_BYTES", 7 * 65 * 24)
    chunked = E.render_uncertainty(H, Wd, focal, c2w, model, gt=gt, **kw)
    for k in ("rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "sq_err", "occupied_bins"):
        assert torch.equal(chunked[k], out[k]), k
    for stats in ("ext", "geometry"):
        with pytest.raises(ValueError, match="acc_map"):
            E.render_uncertainty(H, Wd, focal, c2w, model, stats=stats, **kw)


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_the_hierarchical_step_refuses_a_sampler(scene):
    cfg, model, net, p, _, d = scene
    o, dd = _rays8()
    tr = TR.Trainer(net)
    before = net.flat.detach().clone()
    with pytest.raises(NotImplementedError, match="occupancy.*step_hierarchical"):
        tr.step_hierarchical(*HWF, torch.stack([o, dd]).to(DEV), d["target"].to(DEV), occupancy=_grid().sampler(), **GEO)
    with pytest.raises(NotImplementedError, match="occupancy"):
        tr.forward_backward_hierarchical(*HWF, torch.stack([o, dd]).to(DEV), d["target"].to(DEV), occupancy=_grid().sampler(), **GEO)
    assert tr.t == 0 and torch.equal(net.flat.detach(), before)
