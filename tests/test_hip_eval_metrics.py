"""-m gpu: the paper's evaluation metrics fused into the eval render (CFNERF_F_KSTATS_EXT): kstats [N,12], sqerr [N,6],
``render_uncertainty(stats="ext")``, ``image_metrics``.  The reference of every new column is the fp64 restatement of
tests/eval_metrics_common.py (pinned to the oracle by tests/test_eval_metrics_cpu.py) evaluated on the kernel's OWN per-K maps.

The NLL test prints its figures per case (kernel error, fp32-reference error, their ratio, the bound); they belong in
profiles/r08_eval_metrics.txt, which says whether they have been measured."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
from cfnerf_amd.api import _pack_rays, _render_fwd, t_vals_table
from eval_metrics_common import nll_terms, spread
from oracle import cfnerf_oracle as O
from util_hip import ATOL, ATOL_DISP, RTOL, build_model, close, fern_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(True, False, 32), (False, True, 4), (False, False, 128), (False, True, 2)]        # (white_bkgd, ndc, K)
H_, W_, FOCAL_ = 20, 24, 33.3                                                               # as tests/test_hip_evaluate.py
NEW_KEYS = ("disp_unc", "depth_unc", "acc_mean", "acc_unc")


def _pose(ndc):
    if ndc:
        return torch.tensor([[1, 0, 0, 0.1], [0, 1, 0, -0.1], [0, 0, 1, 0.0]], dtype=torch.float32)
    th, ph = np.deg2rad(30.0), np.deg2rad(-30.0)
    return torch.tensor([[np.cos(th), -np.sin(th) * np.sin(ph), np.sin(th) * np.cos(ph), 4 * np.sin(th) * np.cos(ph)],
                         [0, np.cos(ph), np.sin(ph), 4 * np.sin(ph)],
                         [-np.sin(th), -np.cos(th) * np.sin(ph), np.cos(th) * np.cos(ph), 4 * np.cos(th) * np.cos(ph)]], dtype=torch.float32)


def _case(white_bkgd, ndc, K, seed=55):
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    _, _, kw_test, model, p, _ = build_model(cfg, seed, white_bkgd=white_bkgd, no_ndc=not ndc)
    near, far = (2.0, 6.0) if not ndc else (0.0, 1.0)
    return cfg, model, p, _pose(ndc), dict(near=near, far=far, ndc=ndc, white_bkgd=white_bkgd)


def _raw_launch(net, kw, ext, maps=False, weights=False, train=False, H=H_, W=W_):
    """cfnerf_render_fwd on the whole H x W image: the per-K maps / weights / kstats of ONE launch"""
    n = H * W
    packed = _pack_rays(H, W, FOCAL_, c2w=kw["c2w"], n=n, pixel0=0, ndc=kw["ndc"], near=kw["near"], far=kw["far"], device=net.device)
    net._sync()
    flags = (L.F_WHITE_BKGD if kw["white_bkgd"] else 0) | (L.F_KSTATS_EXT if ext else 0) | (L.F_TRAIN if train else 0)
    return _render_fwd(net, packed, t_vals_table(net.device), None, net.eval_eps(), flags, maps=maps, weights=weights, kstats=True, entropy=train)


def _gt_from_maps(rgb_mean, rgb_unc, seed):
    """gt = rgb_mean + u rgb_unc, u ~ U(-2, 2), on the even pixels (the integrand is then not saturated); U(0, 1) noise on the odd
    ones (they exercise the + 1e-5 floor, where nll -> -log 1e-5)."""
    g = torch.Generator().manual_seed(seed)
    n = rgb_mean.shape[0]
    u = torch.rand(n, 3, generator=g) * 4 - 2
    gt = rgb_mean.cpu() + u * rgb_unc.cpu()
    gt[1::2] = torch.rand(gt[1::2].shape, generator=g)
    return gt.contiguous()


@pytest.mark.parametrize("white_bkgd,ndc,K", CASES)
def test_old_columns_keep_their_bits(white_bkgd, ndc, K):
    cfg, model, p, c2w, kw = _case(white_bkgd, ndc, K)
    gt = torch.tensor(np.random.default_rng(3).uniform(0, 1, (H_, W_, 3)), dtype=torch.float32)
    base = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt, **kw)
    ext = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt, stats="ext", **kw)
    for k in ("rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "sq_err", "mse"):
        assert torch.equal(base[k], ext[k]), k
    assert set(ext) - set(base) == set(NEW_KEYS) | {"nll", "loss_nll"}
    # and on the raw buffers: kstats_ext[:, :8] / sqerr_ext[:, :3] against the flag-less launch
    net = model.module
    n = H_ * W_
    lib = L.lib()
    packed = _pack_rays(H_, W_, FOCAL_, c2w=c2w, n=n, pixel0=0, ndc=ndc, near=kw["near"], far=kw["far"], device=net.device)
    tv, eps, g = t_vals_table(net.device), net.eval_eps(), gt.to(DEV).reshape(n, 3).contiguous()
    flags = L.F_WHITE_BKGD if white_bkgd else 0
    k8, s3 = torch.full((n, 8), -7.0, device=DEV), torch.full((n, 3), -7.0, device=DEV)
    k12, s6 = torch.full((n, 12), -7.0, device=DEV), torch.full((n, 6), -7.0, device=DEV)
    L.check(lib.cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(tv), L.ptr(eps), n, 128, K, flags, L.ptr(g), L.ptr(k8), L.ptr(s3), L.stream()), "eval")
    L.check(lib.cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(tv), L.ptr(eps), n, 128, K, flags | L.F_KSTATS_EXT, L.ptr(g), L.ptr(k12), L.ptr(s6),
                                   L.stream()), "eval ext")
    assert torch.equal(k12[:, :8], k8) and torch.equal(s6[:, :3], s3)
    assert not (k12 == -7.0).any() and not (s6 == -7.0).any()                               # every new column was written
    # without gt the kstats are the same bits and nothing else is touched
    k12b = torch.full((n, 12), -7.0, device=DEV)
    L.check(lib.cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(tv), L.ptr(eps), n, 128, K, flags | L.F_KSTATS_EXT, None, L.ptr(k12b), None,
                                   L.stream()), "eval ext, no gt")
    assert torch.equal(k12b, k12)


@pytest.mark.parametrize("white_bkgd,ndc,K", CASES)
def test_new_columns_match_the_kernels_own_per_k_maps(white_bkgd, ndc, K):
    """disp_map, depth_map, rgb_map and the weights (their sum over the samples = acc_map, RUN:449) of ONE launch; the fp64 restatement
    on them against columns 8 .. 11 of that launch's kstats.  Bounds: those tests/test_hip_evaluate.py uses for rgb_unc."""
    cfg, model, p, c2w, kw = _case(white_bkgd, ndc, K)
    net = model.module
    o = _raw_launch(net, dict(kw, c2w=c2w), ext=True, maps=True, weights=True)
    ks = o["kstats"]
    assert list(ks.shape) == [H_ * W_, 12]
    disp, depth, acc = o["disp_map"].cpu().double(), o["depth_map"].cpu().double(), o["weights"].cpu().double().sum(1)
    close(ks[:, 8], spread(disp), atol=ATOL_DISP, rtol=1e-3, what="disp_unc")
    close(ks[:, 9], spread(depth), atol=1e-6, rtol=1e-4, what="depth_unc")
    close(ks[:, 10], acc.mean(-1), atol=1e-6, rtol=1e-5, what="acc_mean")
    close(ks[:, 11], spread(acc), atol=1e-6, rtol=1e-4, what="acc_unc")
    close(ks[:, 3:6], spread(o["rgb_map"].cpu().double()), atol=1e-6, rtol=1e-4, what="rgb_unc")
    # the fused eval launch (no per-K map anywhere) gives the same columns bit for bit
    fe = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, stats="ext", **kw)
    fm = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, stats="ext", want_maps=True, **kw)
    for i, k in zip((8, 9, 10, 11), NEW_KEYS):
        assert torch.equal(fe[k].reshape(-1), ks[:, i]), k
        assert torch.equal(fm[k].reshape(-1), ks[:, i]), k                                  # want_maps: still the kernel's kstats
    if K == 4:                                                                              # and against the CPU oracle
        ea, er = net.sample_alpha.clone(), net.sample_rgb.clone()
        ea[-1] = 0
        er[-1] = 0
        r = O.render(p, H_, W_, FOCAL_, cfg, ea, er, False, c2w=c2w, ndc=ndc, near=kw["near"], far=kw["far"], white_bkgd=white_bkgd)
        flat = lambda t: t.reshape(H_ * W_, -1).double()
        close(ks[:, 8], spread(flat(r["disp_map"])), atol=ATOL_DISP, rtol=1e-3, what="disp_unc vs oracle")
        close(ks[:, 9], spread(flat(r["depth_map"])), atol=ATOL, rtol=RTOL, what="depth_unc vs oracle")
        acc_o = r["weights"].double().sum(-2).reshape(H_ * W_, K)                           # [.., S, K] -> acc_map, RUN:449
        close(ks[:, 10], acc_o.mean(-1), atol=ATOL, rtol=RTOL, what="acc_mean vs oracle")
        close(ks[:, 11], spread(acc_o), atol=ATOL, rtol=RTOL, what="acc_unc vs oracle")


@pytest.mark.parametrize("white_bkgd,ndc,K", CASES)
def test_nll_map_against_the_restatement_and_the_loss_kernel(white_bkgd, ndc, K):
    """nll [h,W,3] of the fused launch against the fp64 restatement on the launch's own per-K colours.  The quantity is ill-conditioned
    in the bandwidth (d nll / d rgb_k ~ delta / h^2), so the bound is calibrated per case, in the form of util_hip.density_path_tol:
    the error of the REFERENCE's own arithmetic - the same expression evaluated by torch on the CPU in fp32 on the same maps - against
    fp64, times 8, with a floor of 1e-5, of the largest entry."""
    cfg, model, p, c2w, kw = _case(white_bkgd, ndc, K)
    net = model.module
    n = H_ * W_
    full = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, stats="ext", want_maps=True, **kw)
    rgbs = full["rgb_map"].reshape(n, 3, K).cpu()
    gt = _gt_from_maps(full["rgb_mean"].reshape(n, 3), full["rgb_unc"].reshape(n, 3), seed=K)
    ref, lik = nll_terms(rgbs.double(), gt.double())
    # condition (not a measurement): the even pixels are NOT on the floor - a test that only ever sees -log 1e-5 cannot pass
    frac = float((lik[0::2] > 1e-3).double().mean())
    assert frac >= 0.95, f"only {frac:.3f} of the even pixel-channels have a likelihood above 1e-3"
    floor_frac = float((lik[1::2] < 1e-5).double().mean())                                  # (how many odd pixel-channels sit on the floor: printed)
    ref32, _ = nll_terms(rgbs, gt)
    scale = float(ref.abs().max())
    e32 = float((ref32.double() - ref).abs().max()) / scale
    fe = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt.reshape(H_, W_, 3), stats="ext", **kw)
    got = fe["nll"].reshape(n, 3).cpu().double()
    assert torch.isfinite(got).all()
    err = float((got - ref).abs().max()) / scale
    bound = max(1e-5, 8.0 * e32)
    print(f"\nNLL white_bkgd={white_bkgd} ndc={ndc} K={K}: kernel err {err:.3e}  fp32 reference err {e32:.3e}  ratio {err / max(e32, 1e-30):.2f}  "
          f"bound {bound:.3e}  (of the largest entry {scale:.4f}; {frac:.3f} of the even pixel-channels above 1e-3, {floor_frac:.3f} of the odd ones below 1e-5)", file=sys.stderr, flush=True)
    assert err <= bound, f"nll: error {err:.3e} of the largest entry exceeds max(1e-5, 8 x {e32:.3e})"
    close(fe["loss_nll"], ref.mean(), atol=max(1e-5, bound * scale), rtol=1e-4, what="loss_nll vs restatement")
    # want_maps + gt: nll from the per-K maps that were asked for - the same numbers to the same bound
    fm = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt.reshape(H_, W_, 3), stats="ext", want_maps=True, **kw)
    assert float((fm["nll"].reshape(n, 3).cpu().double() - ref).abs().max()) / scale <= bound
    # independent cross-check: loss_nll is scalars_out[1] of cfnerf_loss_fwd_bwd on the same rgb_map and gt (n_total = N, beta1 = 0)
    rg, g = full["rgb_map"].reshape(n, 3, K).contiguous(), gt.to(DEV)
    d_rgb, scal = torch.empty(n, 3, K, device=DEV), torch.zeros(4, device=DEV)
    L.check(L.lib().cfnerf_loss_fwd_bwd(L.ptr(rg), L.ptr(g), None, n, K, C.c_float(0.0), n, L.ptr(d_rgb), L.ptr(scal), L.stream()), "cfnerf_loss_fwd_bwd")
    close(fe["loss_nll"], scal[1], atol=ATOL, rtol=RTOL, what="loss_nll vs cfnerf_loss_fwd_bwd")
    close(fe["mse"], scal[2], atol=1e-7, rtol=1e-5, what="mse vs cfnerf_loss_fwd_bwd")


def test_row_shards_and_two_launches_give_identical_bits():
    white_bkgd, ndc, K = True, False, 32
    cfg, model, p, c2w, kw = _case(white_bkgd, ndc, K)
    gt = torch.tensor(np.random.default_rng(5).uniform(0, 1, (H_, W_, 3)), dtype=torch.float32)
    full = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt, stats="ext", **kw)
    again = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt, stats="ext", **kw)
    keys = NEW_KEYS + ("nll",)
    parts = []
    for rk in range(3):
        r0, r1 = E.row_shard(H_, rk, 3)
        parts.append(E.render_uncertainty(H_, W_, FOCAL_, c2w, model, gt=gt[r0:r1], rows=(r0, r1), stats="ext", **kw))
    for k in keys:
        assert torch.equal(full[k], again[k]), k
        assert torch.equal(torch.cat([q[k] for q in parts], 0), full[k]), k


def test_full_size_config5_tiles_equal_the_image_and_the_maps_are_in_range():
    """800 x 800, K = 32, white background, no NDC: 8 row tiles equal the one-launch image bit for bit for every new map; all new maps
    are finite, uncertainties >= 0, 0 <= acc_mean <= 1 + 1e-5."""
    K = 32
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    _, _, _, model, _, _ = build_model(cfg, 9, white_bkgd=True, no_ndc=True)
    H = W = 800
    focal = 1111.1
    c2w = _pose(False)
    kw = dict(near=2.0, far=6.0, ndc=False, white_bkgd=True)
    gt = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    full = E.render_uncertainty(H, W, focal, c2w, model, gt=gt, stats="ext", **kw)
    keys = NEW_KEYS + ("nll",)
    parts = []
    for rk in range(8):
        r0, r1 = E.row_shard(H, rk, 8)
        parts.append(E.render_uncertainty(H, W, focal, c2w, model, gt=gt[r0:r1], rows=(r0, r1), stats="ext", **kw))
    for k in keys:
        assert torch.equal(torch.cat([q[k] for q in parts], 0), full[k]), k
        assert torch.isfinite(full[k]).all(), k
    for k in ("disp_unc", "depth_unc", "acc_unc"):
        assert float(full[k].min()) >= 0, k
    assert float(full["acc_mean"].min()) >= 0 and float(full["acc_mean"].max()) <= 1 + 1e-5
    assert float(full["nll"].max()) <= -np.log(1e-5) + 1e-4


@pytest.mark.parametrize("train", [False, True])
def test_render_fwd_takes_the_flag_on_both_branches(train):
    white_bkgd, ndc, K = False, True, 4
    cfg, model, p, c2w, kw = _case(white_bkgd, ndc, K)
    net = model.module
    kwc = dict(kw, c2w=c2w)
    o = _raw_launch(net, kwc, ext=True, maps=True, train=train)
    base = _raw_launch(net, kwc, ext=False, maps=True, train=train)
    assert list(o["kstats"].shape) == [H_ * W_, 12]
    assert torch.equal(o["kstats"][:, :8], base["kstats"]) and torch.equal(o["rgb_map"], base["rgb_map"])
    only = _raw_launch(net, kwc, ext=True, maps=False, train=train)                         # kstats alone, no per-K map
    assert torch.equal(only["kstats"], o["kstats"])
    if train:
        assert torch.equal(o["entropy"], base["entropy"]) and bool(torch.isfinite(o["entropy"]).all())
        close(o["kstats"][:, 9], spread(o["depth_map"].cpu().double()), atol=1e-6, rtol=1e-4, what="depth_unc (train branch)")
    else:                                                                                   # eval branch: the columns of cfnerf_render_eval
        fe = E.render_uncertainty(H_, W_, FOCAL_, c2w, model, stats="ext", **kw)
        for i, k in zip((8, 9, 10, 11), NEW_KEYS):
            assert torch.equal(fe[k].reshape(-1), o["kstats"][:, i]), k


def test_refusals_name_the_flag():
    lib = L.lib()
    cfg = O.OracleCfg(netwidth=64, K_samples=3)
    _, _, _, model, _, _ = build_model(cfg, 3)
    net = model.module
    net._sync()
    h, s, P = net.handle, L.stream(), L.ptr
    N, S, K = 8, 128, 3
    rays, (H, W, focal) = fern_rays(np.random.default_rng(0), N)
    packed = torch.empty(N, 11, device=DEV)
    L.check(lib.cfnerf_rays_setup(H, W, focal, None, P(rays[0].contiguous().to(DEV)), P(rays[1].contiguous().to(DEV)), N, 0, 1, 0., 1., P(packed), s), "rays")
    tv, eps = t_vals_table(DEV), torch.randn(K, 4, device=DEV)
    ks, sq, gt = torch.empty(N, 12, device=DEV), torch.empty(N, 6, device=DEV), torch.rand(N, 3, device=DEV)
    X = L.F_KSTATS_EXT

    def refused(rc, *words):
        msg = lib.cfnerf_last_error().decode(errors="replace")
        assert rc < 0 and all(w in msg for w in words), (rc, msg)

    assert lib.cfnerf_render_eval(h, P(packed), P(tv), P(eps), N, S, K, X, P(gt), P(ks), P(sq), s) == 0          # the valid call
    x, raw = torch.randn(16, 90, device=DEV), torch.empty(16, K, 4, device=DEV)
    refused(lib.cfnerf_network_fwd(h, P(x), P(eps), 16, K, X, P(raw), None, s), "cfnerf_network_fwd", "CFNERF_F_KSTATS_EXT")
    z, pts = torch.empty(N, S, device=DEV), torch.empty(N, S, 3, device=DEV)
    refused(lib.cfnerf_sample_points(P(packed), P(tv), None, X, N, S, P(z), P(pts), s), "cfnerf_sample_points", "CFNERF_F_KSTATS_EXT")
    wts, u, zo = torch.rand(N, S, K, device=DEV), torch.rand(N, 16, device=DEV), torch.empty(N, S + 16, device=DEV)
    refused(lib.cfnerf_sample_pdf(P(packed), P(tv), None, X, P(wts), P(u), N, S, K, 16, P(zo), s), "cfnerf_sample_pdf", "CFNERF_F_KSTATS_EXT")
    refused(lib.cfnerf_render_eval(h, P(packed), P(tv), P(eps[:1]), N, S, 1, X, None, P(ks), None, s), "K >= 2")            # the flag with K = 1
    refused(lib.cfnerf_render_eval(h, P(packed), P(tv), P(eps), N, S, K, X, P(gt), P(ks), None, s), "gt_opt", "sqerr_opt")   # gt without sqerr
    rgb, disp, depth, ent = torch.empty(N, 3, K, device=DEV), torch.empty(N, K, device=DEV), torch.empty(N, K, device=DEV), torch.zeros(1, device=DEV)
    fwd = lambda flags, kst, e=None: lib.cfnerf_render_fwd(h, P(packed), P(tv), None, None, P(eps), N, S, K, flags, P(rgb), P(disp), P(depth), None, None,
                                                         None, P(kst), P(e), s)
    refused(fwd(X, None), "CFNERF_F_KSTATS_EXT", "kstats_opt")                                                   # nothing to widen
    refused(fwd(X | L.F_STASH, ks, ent), "CFNERF_F_KSTATS_EXT", "CFNERF_F_STASH")                                 # not built for stash launches
    assert fwd(X, ks) == 0 and fwd(X | L.F_TRAIN, ks, ent) == 0                                                  # the handle stays usable
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ks).all())


def test_image_metrics_on_a_trained_model():
    """A few hundred steps on the procedural stand-in scene (fixed seeds), then the per-view numbers of the paper's tables from one launch."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import procedural_scene as PS
    from cfnerf_amd import train as TR
    K, N_rand, steps = 4, 1024, 300
    poses, images, i_train, i_test = PS.make(DEV, 7)
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    torch.manual_seed(0)
    _, _, _, model, _, _ = build_model(cfg, 0, no_ndc=True)
    net = model.module
    net.reset_parameters()
    pool = cfnerf_amd.RayPool(images, poses, PS.H, PS.W, PS.FOCAL, i_train, N_rand, generator=torch.Generator(device=DEV).manual_seed(1))
    tr = TR.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01)
    g = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(steps):
        rays, target = pool.next_batch()
        tr.step(PS.H, PS.W, PS.FOCAL, rays, target.contiguous(), t_rand=torch.rand(N_rand, 128, device=DEV, generator=g),
                eps=torch.randn(K, 4, device=DEV, generator=g), near=PS.NEAR, far=PS.FAR, ndc=False)
    v = i_test[0]
    H, W = PS.H, PS.W
    kw = dict(near=PS.NEAR, far=PS.FAR, ndc=False)
    gt = images[v].to(DEV).contiguous()
    ref = E.render_uncertainty(H, W, PS.FOCAL, poses[v], model, gt=gt, stats="ext", **kw)
    # no depth truth exists for the stand-in scene: a fixed perturbation of the rendered depth plays it (the comparison below is helper against helper)
    gt_depth = (ref["depth_mean"] * (1 + 0.2 * (torch.rand(H, W, generator=torch.Generator().manual_seed(3)).to(DEV) - 0.5))).contiguous()
    del pool, tr
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    m = E.image_metrics(H, W, PS.FOCAL, poses[v], model, gt, gt_depth=gt_depth, **kw)
    peak = torch.cuda.max_memory_allocated() - base
    budget = 2 * 84 * H * W + 44 * H * W                                                     # 2 x 84 B per pixel + the [N,11] ray pack
    print(f"\nimage_metrics: {m}\npeak device memory of the call {peak} B = {peak / (H * W):.1f} B per pixel (budget {budget / (H * W):.0f}; "
          f"one [N,K] fp32 map would be {4 * K} B per pixel, the per-K maps {20 * K})", file=sys.stderr, flush=True)
    assert peak <= budget, (peak, budget)
    assert set(m) == {"mse", "psnr", "loss_nll", "ause_rgb_rmse", "ause_rgb_mae", "ause_depth_rmse", "ause_depth_mae"}
    assert all(np.isfinite(x) for x in m.values()), m
    close(torch.tensor(m["psnr"]), cfnerf_amd.mse2psnr(cfnerf_amd.img2mse(ref["rgb_mean"], gt)).reshape(()), atol=1e-5, rtol=1e-5, what="psnr")
    assert m["psnr"] > 12.0, m                                                              # the model did train
    close(torch.tensor(m["loss_nll"]), ref["loss_nll"], atol=0, rtol=1e-6, what="loss_nll")
    var = (ref["rgb_unc"] ** 2).mean(-1).reshape(-1)
    sq = ref["sq_err"]
    d = ref["depth_mean"] - gt_depth
    dvar = (ref["depth_unc"] ** 2).reshape(-1)
    for name, vv, ee, et in (("ause_rgb_rmse", var, sq.mean(-1).reshape(-1), "rmse"), ("ause_rgb_mae", var, torch.sqrt(sq).mean(-1).reshape(-1), "mae"),
                             ("ause_depth_rmse", dvar, (d * d).reshape(-1), "rmse"), ("ause_depth_mae", dvar, d.abs().reshape(-1), "mae")):
        want = E.ause(vv, ee, err_type=et)
        assert abs(m[name] - want) <= 1e-5 * abs(want), (name, m[name], want)
    no_depth = E.image_metrics(H, W, PS.FOCAL, poses[v], model, gt, **kw)
    assert set(no_depth) == {"mse", "psnr", "loss_nll", "ause_rgb_rmse", "ause_rgb_mae"} and no_depth["psnr"] == m["psnr"]
