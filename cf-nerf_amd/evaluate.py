"""Full-image evaluation on the HIP path (reference: render_path_train RUN:247-314, the
uncertainty maps of RUN:1117-1131, sparsification_plot HLP:382-438).

* ``render_path_train`` mirrors the reference's working single-pose branch and returns numpy ``rgbs [1,H,W,3,K]``,
  ``disps [1,H,W,K]``.
* ``render_uncertainty`` is the MI355X-first form of what the training loop derives from those maps: the K-mean
  prediction, the ``np.std * n/(n-1)`` uncertainty, mean disparity/depth are reduced INSIDE the fused kernel
  (32 B per pixel leave the chip instead of 20*K B), optionally on a row slice of the image so an image is
  tiled across ranks with no exchange.
* ``render_uncertainty(stats="ext")`` / ``image_metrics``: the four numbers of the paper's tables (PSNR, NLL, AUSE of the colour and of
  the depth uncertainty) from ONE launch per image (CFNERF_F_KSTATS_EXT: 48 + 24 B per pixel, + 12 B of ground truth, no per-K map),
  with ``sparsification_curves`` / ``ause_fused`` as the device-side form of the reference's sparsification helper.
* ``render_uncertainty(scores=levels)`` / ``calibration`` / ``image_metrics(calibration=True)``: the K samples of a pixel scored as an ENSEMBLE
  (CFNERF_F_KSCORES, ``api.k_scores``) - quantile maps (median colour and depth, credible intervals), the CRPS, the rank of the truth among
  the samples and, from the ranks, the coverage of the central intervals and the area under the calibration error.
* ``render_uncertainty(stats="geometry")`` / ``density_grid``: depth and disparity maps with their uncertainty, and density /
  density-uncertainty volumes, from launches that skip the colour branch (CFNERF_F_GEOMETRY).
"""
from __future__ import annotations


import math

import numpy as np
import torch

from . import _lib as L
from .api import _network_geometry, _pack_rays, _render_fwd, _unwrap, k_scores, render, render_rays_culled, t_vals_table, warp_probe_chunk, warp_z_vals
from .api import ssim as _ssim      # (image_metrics has an argument of that name)


def render_path_train(render_poses, hwf, chunk, render_kwargs, gt_imgs=None, savedir=None, render_factor=0):
    """RUN:247-314.  Only the single-pose branch works in the reference (the multi-pose branch reads an undefined
    ``var`` and unpacks 3 of render()'s 4 results, RUN:279-282 / SURVEY R11); it is rejected here."""
    H, W, focal = hwf
    if render_factor != 0:
        H, W, focal = H // render_factor, W // render_factor, focal / render_factor          # RUN:251-255
    poses = torch.as_tensor(render_poses)
    if poses.ndim == 3:
        raise NotImplementedError("the reference's multi-pose branch of render_path_train cannot run (undefined `var`, "
                                  "RUN:279-282); call it once per pose")
    c2w = poses[:3, :4]                                                                      # RUN:304
    rgb, disp, depth, extras = render(int(H), int(W), float(focal), chunk=chunk, c2w=c2w, **render_kwargs)
    return np.stack([rgb.cpu().numpy()], 0), np.stack([disp.cpu().numpy()], 0)              # RUN:307-314


def row_shard(H: int, rank: int, world: int):
    """Rows [r0, r1) of an H-row image for this rank (contiguous, sizes differ by at most one)."""
    base, rem = divmod(H, world)
    r0 = rank * base + min(rank, rem)
    return r0, r0 + base + (1 if rank < rem else 0)


# what travels in gather_rows: the maps of render_uncertainty, then those of stats="ext" (52 more bytes per pixel with ground truth)
# (stats="geometry" produces a subset of the same keys: depth_mean, disp_mean, depth_unc, disp_unc, acc_mean, acc_unc)
_ROW_KEYS = ("rgb_mean", "rgb_unc", "disp_mean", "depth_mean", "sq_err", "disp_unc", "depth_unc", "acc_mean", "acc_unc", "nll")


def gather_rows(local: dict, H: int, world: int, rank: int, group=None, dst: int = 0):
    """The optional exchange of the row-tiled evaluation: every rank rendered rows ``row_shard(H, rank, world)`` of one
    image with ``render_uncertainty``; rank ``dst`` gets the full-image maps (``rgb_mean [H,W,3]``, ``rgb_unc``, ``disp_mean``,
    ``depth_mean``, and ``sq_err`` when present), the others ``None``.  32 B per pixel travel (20 MB for 800 x 800), once per image;
    the render itself needs no exchange.  Shards differ by at most one row: they are padded to the largest for ``all_gather``.
    A gloo group (CPU tests, ranks sharing one GPU) is served through host copies.  The maps of ``stats="ext"`` (``disp_unc``,
    ``depth_unc``, ``acc_mean``, ``acc_unc``, ``nll``) travel too when present; a gathered ``nll`` gives ``loss_nll`` as ``sq_err`` gives ``mse``."""
    import torch.distributed as dist
    keys = [k for k in _ROW_KEYS if k in local]
    hmax = max(row_shard(H, r, world)[1] - row_shard(H, r, world)[0] for r in range(world))
    via_host = dist.get_backend(group) == "gloo"
    out = {}
    for k in keys:
        t = local[k].contiguous()
        dev = t.device
        if via_host:
            t = t.cpu()
        pad = torch.zeros((hmax,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        pad[:t.shape[0]] = t
        parts = [torch.empty_like(pad) for _ in range(world)]
        dist.all_gather(parts, pad, group=group)
        if rank == dst:
            rows = [parts[r][:row_shard(H, r, world)[1] - row_shard(H, r, world)[0]] for r in range(world)]
            out[k] = torch.cat(rows, 0).to(dev)
    if rank != dst:
        return None
    if "sq_err" in out:
        out["mse"] = out["sq_err"].mean()
    if "nll" in out:
        out["loss_nll"] = out["nll"].mean()
    return out


def kde_nll(rgb_map, gt):
    """Per-pixel, per-channel integrand of the loss's negative log-likelihood (RUN:1034-1042) from per-K colours ``rgb_map [...,3,K]`` and
    ``gt [...,3]``, in the dtype of ``rgb_map``: the TRAIN estimator - bandwidth from ``torch.std`` (unbiased) times ``n/(n-1)`` - not the
    ``np.std * n/(n-1)`` of ``rgb_unc``.  What CFNERF_F_KSTATS_EXT evaluates inside the kernel; used here only where the per-K maps were
    asked for anyway (``want_maps=True`` with ``gt``)."""
    n = rgb_map.shape[-1]
    h = (torch.std(rgb_map, -1) * n / (n - 1) * torch.pow(torch.tensor(0.8 / n), torch.tensor(-1 / 7)).to(rgb_map) + 1e-05)[..., None]
    r1 = torch.exp(-((rgb_map - gt[..., None]) ** 2) / (2 * h * h))
    r2 = torch.pow(torch.tensor(2 * math.pi), -1.5).to(rgb_map) / h
    return -torch.log((r1 * r2).mean(-1) + 1e-05)


@torch.no_grad()
def render_uncertainty(H, W, focal, c2w, network_fn, near=0., far=1., ndc=True, lindisp=False, white_bkgd=False,
                       rows=None, want_maps=False, t_vals=None, gt=None, stats="basic", occupancy=None, **_ignored):
    """Eval render of rows ``rows=(r0, r1)`` (default: all) of the image seen from ``c2w`` with the reductions over the
    K latent samples fused into the kernel.  Returns a dict with ``rgb_mean [h,W,3]``, ``rgb_unc [h,W,3]``
    (= ``np.std(rgbs,-1) * n/(n-1)``, RUN:1129-1130), ``disp_mean [h,W]`` (RUN:1124), ``depth_mean [h,W]`` and, if
    ``want_maps``, the per-K ``rgb_map [h,W,3,K]``, ``disp_map``, ``depth_map`` as render() returns them.  With ``gt``
    (ground-truth colours of those rows, ``[h,W,3]``) the per-pixel squared error of the K-mean prediction is produced by the
    same launch (``sq_err [h,W,3]``; ``mse`` = its mean = ``img2mse(rgb_mean, gt)``, RUN:1028).

    ``stats="ext"`` (CFNERF_F_KSTATS_EXT; every key above keeps its bits) adds, from the same launch, ``disp_unc`` / ``depth_unc [h,W]`` -
    the depth-uncertainty maps, same estimator as ``rgb_unc`` - and ``acc_mean`` / ``acc_unc [h,W]`` (accumulated opacity, RUN:449); with
    ``gt`` also ``nll [h,W,3]``, the per-pixel integrand of the loss's KDE negative log-likelihood (RUN:1034-1042: the train estimator,
    see ``kde_nll``), and ``loss_nll`` = its mean.  84 B per pixel stay on the device (48 + 24 + the 12 of ``gt``).  With ``want_maps``
    the extended statistics still come from the kernel's ``kstats``; ``nll`` is then taken from the per-K maps that were asked for.

    ``stats="geometry"`` (CFNERF_F_GEOMETRY: the launch skips the colour branch) returns ``depth_mean``, ``disp_mean``, ``depth_unc``,
    ``disp_unc``, ``acc_mean``, ``acc_unc [h,W]`` only - 24 B per pixel, each with the bits ``stats="ext"`` gives it; ``white_bkgd`` has no
    effect on them, ``want_maps`` / ``gt`` are refused.

    ``occupancy=`` an ``OccupancyGrid`` (``stats="basic"`` only) renders through the grid instead (CFNERF_F_CULL, ``api.render_rays_culled``):
    samples in empty cells never reach the network.  The rays are walked in bounded chunks, each with one synchronising copy of its kept
    count, and the keys above are derived in torch from the per-K maps of the sparse composite, with the same estimators.

    ``occupancy=`` an ``OccupancySampler`` (``grid.sampler()``; ``stats="basic"`` only) SAMPLES through the grid on the fused path instead:
    per ray chunk ``api.warp_z_vals`` places all S depths inside the occupied part of the ray and one explicit-depth fused launch writes
    the ``[n,8]`` statistics (no per-K map leaves the chip unless ``want_maps``; nothing synchronises).  Adds ``occupied_bins``, the mean of
    ``n_occ / bins`` over the rays (a device scalar).

    ``scores=levels`` (keyword; a sequence of at most 16 quantile levels in [0,1]; ``stats="basic"`` or ``"ext"``) also scores the K samples of every
    pixel as an ensemble (``api.k_scores``, CFNERF_F_KSCORES): ``rgb_q [h,W,3,Q]`` and ``depth_q [h,W,Q]``, the quantile maps (level 0.5: the
    median colour and the median depth); with ``gt`` also ``rgb_crps``, ``rgb_pit [h,W,3]`` and ``rgb_rank [h,W,3]`` (int32), with
    ``gt_depth [h,W]`` ``depth_crps``, ``depth_pit`` and ``depth_rank [h,W]`` (``calibration`` turns the ranks into coverage figures).  The
    rows are walked in chunks of ``_SCORES_RAY_CHUNK`` rays: a chunk is one fused forward that also writes its per-K maps, then the scoring
    launch on ``rgb_map`` and ``depth_map``; the maps of a chunk are dropped before the next one, so no whole-image per-K map exists unless
    ``want_maps`` asks for it.  Every key the call returns without ``scores=`` keeps its bits (rays are independent).  One combination pays
    a second forward per chunk: ``stats="ext"`` with ``gt`` and without ``want_maps``, where ``nll`` is the fused kernel's own
    (cfnerf_render_eval) and the per-K maps come from a maps-only launch.  Refused with ``stats="geometry"`` and with ``occupancy=``."""
    if stats not in ("basic", "ext", "geometry"):
        raise ValueError(f"stats must be 'basic', 'ext' or 'geometry', got {stats!r}")
    # (keyword-only, taken from the catch-all: tests/test_cull_cpu.py pins the named parameters of this function)
    scores, gt_depth = _ignored.get("scores"), _ignored.get("gt_depth")
    if scores is not None and (occupancy is not None or stats == "geometry"):
        raise ValueError("scores= is not supported with occupancy= or stats='geometry' (it scores the per-K maps of the plain fused forward, "
                         "stats='basic' or 'ext')")
    if gt_depth is not None and scores is None:
        raise ValueError("gt_depth= is the target of the depth scores: it needs scores=levels")
    if occupancy is not None:
        if stats != "basic":
            raise ValueError(f"occupancy= supports stats='basic' only, got {stats!r}: the culled path ends in the standalone composite, which has "
                             "no acc_map (the accumulated opacity of stats='ext' / 'geometry' exists in the fused kernels alone)")
        route = _render_uncertainty_warped if isinstance(occupancy, OccupancySampler) else _render_uncertainty_culled
        return route(H, W, focal, c2w, network_fn, occupancy, near, far, ndc, lindisp, white_bkgd, rows, want_maps, t_vals, gt)
    if stats == "geometry":
        if want_maps or gt is not None:
            raise ValueError("stats='geometry' renders no colour: want_maps / gt are not arguments of it (api.render_geometry gives the per-K maps)")
        return _render_uncertainty_geometry(H, W, focal, c2w, network_fn, near, far, ndc, lindisp, rows, t_vals)
    ext = stats == "ext"
    net = _unwrap(network_fn)
    dev = net.device
    r0, r1 = rows if rows is not None else (0, H)
    n = (r1 - r0) * W
    K = net.K_samples
    if t_vals is None:
        t_vals = t_vals_table(dev)
    S = t_vals.shape[0]
    packed = _pack_rays(H, W, focal, c2w=c2w, n=n, pixel0=r0 * W, ndc=ndc, near=near, far=far, device=dev)
    net._sync()
    eps = net.eval_eps()
    flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0) | (L.F_KSTATS_EXT if ext else 0)
    if scores is not None:
        return _render_uncertainty_scored(net, packed, t_vals, eps, flags, ext, r1 - r0, W, want_maps, gt, gt_depth, scores)
    sq = nll = None
    if want_maps:
        o = _render_fwd(net, packed, t_vals, None, eps, flags, kstats=True, entropy=False)
        kst = o['kstats']
        if gt is not None:
            g = gt.to(dev, torch.float32).reshape(n, 3)
            sq = (kst[:, 0:3] - g) ** 2
            if ext:
                nll = kde_nll(o['rgb_map'], g)
    else:
        kst = torch.empty(n, 12 if ext else 8, device=dev)
        g = None
        if gt is not None:
            g = gt.to(dev, torch.float32).reshape(n, 3).contiguous()
            sq = torch.empty(n, 6 if ext else 3, device=dev)
        L.check(L.lib().cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(t_vals), L.ptr(eps), n, S, K, flags, L.ptr(g), L.ptr(kst), L.ptr(sq),
                                           L.stream()), "cfnerf_render_eval")
    h = r1 - r0
    out = dict(rgb_mean=kst[:, 0:3].reshape(h, W, 3), rgb_unc=kst[:, 3:6].reshape(h, W, 3), disp_mean=kst[:, 6].reshape(h, W),
               depth_mean=kst[:, 7].reshape(h, W))
    if want_maps:
        out.update(rgb_map=o['rgb_map'].reshape(h, W, 3, K), disp_map=o['disp_map'].reshape(h, W, K), depth_map=o['depth_map'].reshape(h, W, K))
    if ext:
        out.update(disp_unc=kst[:, 8].reshape(h, W), depth_unc=kst[:, 9].reshape(h, W), acc_mean=kst[:, 10].reshape(h, W),
                   acc_unc=kst[:, 11].reshape(h, W))
        if sq is not None and nll is None:
            sq, nll = sq[:, 0:3].contiguous(), sq[:, 3:6]           # (sq_err contiguous: ``mse`` then reduces exactly as in "basic")
    if sq is not None:
        out.update(sq_err=sq.reshape(h, W, 3), mse=sq.mean())
    if nll is not None:
        out.update(nll=nll.reshape(h, W, 3), loss_nll=nll.mean())
    return out


_SCORES_RAY_CHUNK = 1 << 14    # rays per forward + scoring round of render_uncertainty(scores=): bounds the per-K maps (20 K bytes per ray)


def _render_uncertainty_scored(net, packed, t_vals, eps, flags, ext, h, W, want_maps, gt, gt_depth, levels):
    """``render_uncertainty(scores=levels)``: the rays in chunks of ``_SCORES_RAY_CHUNK``; per chunk the fused forward with its per-K maps, then
    ``k_scores`` on ``rgb_map`` and ``depth_map``.  The keys of the call without ``scores=`` are produced the way that call produces them."""
    dev = net.device
    n, K, S = packed.shape[0], net.K_samples, t_vals.shape[0]
    levels = list(levels)
    Q = len(levels)
    L.quantile_levels(levels, K)                                  # (refuses a level outside [0,1] before anything is rendered)
    if not 1 <= Q <= 16:
        raise ValueError(f"scores= takes 1 to 16 quantile levels, got {Q}")
    g = None if gt is None else gt.to(dev, torch.float32).reshape(n, 3).contiguous()
    gd = None if gt_depth is None else gt_depth.to(dev, torch.float32).reshape(n).contiguous()
    fused_nll = ext and g is not None and not want_maps          # nll is then the fused kernel's own: statistics from cfnerf_render_eval
    kst = torch.empty(n, 12 if ext else 8, device=dev)
    sqn = torch.empty(n, 6, device=dev) if fused_nll else None
    maps = [torch.empty(n, 3, K, device=dev), torch.empty(n, K, device=dev), torch.empty(n, K, device=dev)] if want_maps else None
    out = dict(rgb_q=torch.empty(n, 3, Q, device=dev), depth_q=torch.empty(n, Q, device=dev))
    if g is not None:
        out.update(rgb_crps=torch.empty(n, 3, device=dev), rgb_pit=torch.empty(n, 3, device=dev), rgb_rank=torch.empty(n, 3, dtype=torch.int32, device=dev))
    if gd is not None:
        out.update(depth_crps=torch.empty(n, device=dev), depth_pit=torch.empty(n, device=dev), depth_rank=torch.empty(n, dtype=torch.int32, device=dev))
    for i in range(0, n, _SCORES_RAY_CHUNK):
        j = min(n, i + _SCORES_RAY_CHUNK)
        rays = packed[i:j]
        if fused_nll:
            L.check(L.lib().cfnerf_render_eval(net.handle, L.ptr(rays), L.ptr(t_vals), L.ptr(eps), j - i, S, K, flags, L.ptr(g[i:j]), L.ptr(kst[i:j]),
                                               L.ptr(sqn[i:j]), L.stream()), "cfnerf_render_eval")
            o = _render_fwd(net, rays, t_vals, None, eps, flags & ~L.F_KSTATS_EXT, entropy=False)
        else:
            o = _render_fwd(net, rays, t_vals, None, eps, flags, kstats=True, entropy=False)
            kst[i:j] = o['kstats']
        if want_maps:
            maps[0][i:j], maps[1][i:j], maps[2][i:j] = o['rgb_map'], o['disp_map'], o['depth_map']
        c = k_scores(o['rgb_map'], target=None if g is None else g[i:j], levels=levels)
        d = k_scores(o['depth_map'], target=None if gd is None else gd[i:j], levels=levels)
        out['rgb_q'][i:j], out['depth_q'][i:j] = c['quantiles'], d['quantiles']
        if g is not None:
            out['rgb_crps'][i:j], out['rgb_pit'][i:j], out['rgb_rank'][i:j] = c['crps'], c['pit'], c['rank_code']
        if gd is not None:
            out['depth_crps'][i:j], out['depth_pit'][i:j], out['depth_rank'][i:j] = d['crps'], d['pit'], d['rank_code']
        del o, c, d
    out = {k: v.reshape((h, W) + tuple(v.shape[1:])) for k, v in out.items()}
    # the keys of the call without scores=, assembled as render_uncertainty assembles them
    sq = nll = None
    if g is not None:
        if fused_nll:
            sq, nll = sqn[:, 0:3].contiguous(), sqn[:, 3:6]
        else:
            sq = (kst[:, 0:3] - g) ** 2
            if ext:
                nll = kde_nll(maps[0], g)
    out.update(rgb_mean=kst[:, 0:3].reshape(h, W, 3), rgb_unc=kst[:, 3:6].reshape(h, W, 3), disp_mean=kst[:, 6].reshape(h, W),
               depth_mean=kst[:, 7].reshape(h, W))
    if want_maps:
        out.update(rgb_map=maps[0].reshape(h, W, 3, K), disp_map=maps[1].reshape(h, W, K), depth_map=maps[2].reshape(h, W, K))
    if ext:
        out.update(disp_unc=kst[:, 8].reshape(h, W), depth_unc=kst[:, 9].reshape(h, W), acc_mean=kst[:, 10].reshape(h, W),
                   acc_unc=kst[:, 11].reshape(h, W))
    if sq is not None:
        out.update(sq_err=sq.reshape(h, W, 3), mse=sq.mean())
    if nll is not None:
        out.update(nll=nll.reshape(h, W, 3), loss_nll=nll.mean())
    return out


def _render_uncertainty_geometry(H, W, focal, c2w, network_fn, near, far, ndc, lindisp, rows, t_vals):
    """``render_uncertainty(stats="geometry")``: one cfnerf_render_eval launch with CFNERF_F_GEOMETRY, kstats [n,6]."""
    net = _unwrap(network_fn)
    dev = net.device
    r0, r1 = rows if rows is not None else (0, H)
    n, h = (r1 - r0) * W, r1 - r0
    if t_vals is None:
        t_vals = t_vals_table(dev)
    packed = _pack_rays(H, W, focal, c2w=c2w, n=n, pixel0=r0 * W, ndc=ndc, near=near, far=far, device=dev)
    net._sync()
    kst = torch.empty(n, 6, device=dev)
    flags = L.F_GEOMETRY | (L.F_LINDISP if lindisp else 0)
    L.check(L.lib().cfnerf_render_eval(net.handle, L.ptr(packed), L.ptr(t_vals), L.ptr(net.eval_eps()), n, t_vals.shape[0], net.K_samples, flags,
                                       None, L.ptr(kst), None, L.stream()), "cfnerf_render_eval")
    keys = ("disp_mean", "depth_mean", "disp_unc", "depth_unc", "acc_mean", "acc_unc")
    return {k: kst[:, i].reshape(h, W) for i, k in enumerate(keys)}


_CULL_RAY_CHUNK = 1 << 14      # rays per cull / network / composite round of render_uncertainty(occupancy=): bounds x_c and raw_c (dense worst case)


def k_stats(rgb_map, disp_map, depth_map):
    """The evaluation loop's reductions over the K latent samples (RUN:1122-1131) of per-K maps ``rgb_map [...,3,K]``, ``disp_map`` /
    ``depth_map [...,K]`` in torch: ``(rgb_mean, rgb_unc = np.std * n/(n-1), disp_mean, depth_mean)`` - what the fused kernels write as kstats."""
    K = rgb_map.shape[-1]
    return rgb_map.mean(-1), rgb_map.std(-1, unbiased=False) * K / (K - 1), disp_map.mean(-1), depth_map.mean(-1)


def _render_uncertainty_culled(H, W, focal, c2w, network_fn, grid, near, far, ndc, lindisp, white_bkgd, rows, want_maps, t_vals, gt):
    """``render_uncertainty(occupancy=grid)``: ``api.render_rays_culled`` on chunks of the rays, the K-statistics in torch (``k_stats``)."""
    net = _unwrap(network_fn)
    dev = net.device
    K = net.K_samples
    if K < 2:
        raise ValueError("render_uncertainty needs K_samples >= 2 (std * n/(n-1))")
    r0, r1 = rows if rows is not None else (0, H)
    n, h = (r1 - r0) * W, r1 - r0
    packed = _pack_rays(H, W, focal, c2w=c2w, n=n, pixel0=r0 * W, ndc=ndc, near=near, far=far, device=dev)
    rgb_map, disp_map, depth_map = torch.empty(n, 3, K, device=dev), torch.empty(n, K, device=dev), torch.empty(n, K, device=dev)
    kept = 0
    for i in range(0, n, _CULL_RAY_CHUNK):
        o = render_rays_culled(packed[i:i + _CULL_RAY_CHUNK], network_fn, grid, t_vals=t_vals, lindisp=lindisp, white_bkgd=white_bkgd)
        rgb_map[i:i + _CULL_RAY_CHUNK], disp_map[i:i + _CULL_RAY_CHUNK], depth_map[i:i + _CULL_RAY_CHUNK] = o['rgb_map'], o['disp_map'], o['depth_map']
        kept += o['count']
    rgb_mean, rgb_unc, disp_mean, depth_mean = k_stats(rgb_map, disp_map, depth_map)
    out = dict(rgb_mean=rgb_mean.reshape(h, W, 3), rgb_unc=rgb_unc.reshape(h, W, 3), disp_mean=disp_mean.reshape(h, W),
               depth_mean=depth_mean.reshape(h, W), kept_samples=kept)
    if want_maps:
        out.update(rgb_map=rgb_map.reshape(h, W, 3, K), disp_map=disp_map.reshape(h, W, K), depth_map=depth_map.reshape(h, W, K))
    if gt is not None:
        sq = (rgb_mean - gt.to(dev, torch.float32).reshape(n, 3)) ** 2
        out.update(sq_err=sq.reshape(h, W, 3), mse=sq.mean())
    return out


def _render_uncertainty_warped(H, W, focal, c2w, network_fn, sampler, near, far, ndc, lindisp, white_bkgd, rows, want_maps, t_vals, gt):
    """``render_uncertainty(occupancy=sampler)``: per ray chunk ``api.warp_z_vals``, then one fused explicit-depth launch with kstats.  The
    chunk keeps the probe buffers of the warp under 256 MiB (``api.warp_probe_chunk``)."""
    net = _unwrap(network_fn)
    dev = net.device
    K = net.K_samples
    r0, r1 = rows if rows is not None else (0, H)
    n, h = (r1 - r0) * W, r1 - r0
    t_vals = t_vals_table(dev) if t_vals is None else t_vals.to(dev, torch.float32).contiguous()
    packed = _pack_rays(H, W, focal, c2w=c2w, n=n, pixel0=r0 * W, ndc=ndc, near=near, far=far, device=dev)
    net._sync()
    eps = net.eval_eps()
    flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0)
    kst, n_occ = torch.empty(n, 8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    maps = [torch.empty(n, 3, K, device=dev), torch.empty(n, K, device=dev), torch.empty(n, K, device=dev)] if want_maps else None
    step = warp_probe_chunk(sampler.bins)
    for i in range(0, n, step):
        w = warp_z_vals(packed[i:i + step], sampler, t_vals, None, lindisp)
        o = _render_fwd(net, packed[i:i + step], t_vals, None, eps, flags, z_vals=w['z_vals'], maps=want_maps, kstats=True, entropy=False)
        kst[i:i + step], n_occ[i:i + step] = o['kstats'], w['n_occ']
        if want_maps:
            maps[0][i:i + step], maps[1][i:i + step], maps[2][i:i + step] = o['rgb_map'], o['disp_map'], o['depth_map']
    out = dict(rgb_mean=kst[:, 0:3].reshape(h, W, 3), rgb_unc=kst[:, 3:6].reshape(h, W, 3), disp_mean=kst[:, 6].reshape(h, W),
               depth_mean=kst[:, 7].reshape(h, W), occupied_bins=(n_occ.to(torch.float32) / float(sampler.bins)).mean())
    if want_maps:
        out.update(rgb_map=maps[0].reshape(h, W, 3, K), disp_map=maps[1].reshape(h, W, K), depth_map=maps[2].reshape(h, W, K))
    if gt is not None:
        sq = (kst[:, 0:3] - gt.to(dev, torch.float32).reshape(n, 3)) ** 2
        out.update(sq_err=sq.reshape(h, W, 3), mse=sq.mean())
    return out


def sigma_stats(alpha):
    """Density statistics over the K latent samples (last axis) of the density latents ``alpha [...,K]``: sigma = softplus(alpha_k) (RUN:424),
    its mean and ``np.std * n/(n-1)`` (RUN:1130, the estimator of every other uncertainty map here).  Returns ``(sigma_mean, sigma_unc)``."""
    K = alpha.shape[-1]
    sigma = torch.nn.functional.softplus(alpha)
    return sigma.mean(-1), sigma.std(-1, unbiased=False) * K / (K - 1)


@torch.no_grad()
def density_grid(network_fn, lo, hi, res, chunk=1 << 20, eps_alpha=None, return_raw=False):
    """Density and density-uncertainty volume on the axis-aligned grid of ``res = (X, Y, Z)`` points from corner ``lo`` to corner ``hi``
    (both included), queried ``chunk`` points at a time with geometry-only launches (``NeRF_Flows.sample``'s kernel: no colour branch).
    Returns ``{"sigma_mean", "sigma_unc"}`` ``[X,Y,Z]`` (``sigma_stats`` over K; K >= 2) and, with ``return_raw``, ``"alpha" [X,Y,Z,K]``, the
    pre-softplus density latents.  Eval latents (``eval_eps()``: the last one zeroed) unless ``eps_alpha [K,1]`` is given."""
    net = _unwrap(network_fn)
    dev = net.device
    K = net.K_samples
    if K < 2:
        raise ValueError("density_grid needs K_samples >= 2 (std * n/(n-1))")
    X, Y, Z = (int(r) for r in res)
    P = X * Y * Z
    net._sync()
    if eps_alpha is None:
        eps = net.eval_eps()
    else:
        if tuple(eps_alpha.shape) != (K, 1):
            raise ValueError(f"eps_alpha must be [K,1] = [{K},1], got {tuple(eps_alpha.shape)}")
        eps = torch.zeros(K, 4)
        eps[:, 3:] = eps_alpha.detach().to("cpu", torch.float32)
        eps = eps.to(dev)
    axes = [torch.linspace(float(lo[d]), float(hi[d]), n, device=dev) for d, n in enumerate((X, Y, Z))]
    ic, icv = net.input_ch, net.input_ch_views
    chunk = max(1, min(int(chunk), P))
    xbuf = torch.zeros(chunk, ic + icv, device=dev)         # (the view columns are not read by the geometry-only launch)
    emb = torch.empty(chunk, ic, device=dev)
    abuf = torch.empty(chunk, K, device=dev)
    mean, unc = torch.empty(P, device=dev), torch.empty(P, device=dev)
    alpha = torch.empty(P, K, device=dev) if return_raw else None
    lib = L.lib()
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        idx = torch.arange(p0, p0 + n, device=dev)
        pts = torch.stack([axes[0][idx // (Y * Z)], axes[1][(idx // Z) % Y], axes[2][idx % Z]], -1).contiguous()
        L.check(lib.cfnerf_embed(L.ptr(pts), n, (ic - 3) // 6, L.ptr(emb), L.stream()), "cfnerf_embed")
        xbuf[:n, :ic] = emb[:n]
        a = _network_geometry(net, xbuf[:n], eps, out=abuf[:n])
        mean[p0:p0 + n], unc[p0:p0 + n] = sigma_stats(a)
        if return_raw:
            alpha[p0:p0 + n] = a
    out = {"sigma_mean": mean.reshape(X, Y, Z), "sigma_unc": unc.reshape(X, Y, Z)}
    if return_raw:
        out["alpha"] = alpha.reshape(X, Y, Z, K)
    return out


class OccupancyGrid:
    """A bit per cell of the axis-aligned box ``lo .. hi`` cut into ``res = (X, Y, Z)`` cells: what ``api.cull_points`` /
    ``render_uncertainty(occupancy=)`` skip empty space with (CFNERF_F_CULL).  Cell ``(ix, iy, iz)`` is bit ``c & 31`` of word ``c >> 5`` of
    ``bits`` (int32 words holding the 32-bit patterns), ``c = (ix * Y + iy) * Z + iz``; the cell of a point is ``floor((p - lo) * scale)`` per
    axis with ``scale = res / (hi - lo)`` computed ONCE, here, in fp32 - the kernel uses this ``scale``, so host and device agree on every
    cell face.  ``lo``, ``hi``, ``scale`` are numpy fp32 ``[3]``, ``res`` a tuple of ints, ``fraction`` the share of occupied cells."""

    def __init__(self, bits, lo, hi, res, fraction):
        self.bits = bits
        self.lo, self.hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        self.res = tuple(int(r) for r in res)
        if min(self.res) < 1 or not (self.hi > self.lo).all():
            raise ValueError(f"an occupancy grid needs res >= 1 and hi > lo on every axis, got res={self.res} lo={self.lo} hi={self.hi}")
        self.scale = np.asarray(self.res, np.float32) / (self.hi - self.lo)           # fp32 / fp32: the number the kernel multiplies by
        self.fraction = float(fraction)
        self._dev = {}

    def bits_on(self, device):
        """``bits`` on ``device`` (uploaded once per device)"""
        device = torch.device(device)
        if self.bits.device == device:
            return self.bits
        if device not in self._dev:
            self._dev[device] = self.bits.to(device)
        return self._dev[device]

    @staticmethod
    def pack_mask(mask):
        """``mask [X,Y,Z]`` bool -> int32 words ``[ceil(XYZ / 32)]`` in the layout above (on the mask's device)"""
        flat = mask.reshape(-1).to(torch.int64)
        pad = (-flat.numel()) % 32
        if pad:
            flat = torch.cat([flat, flat.new_zeros(pad)])
        w = (flat.reshape(-1, 32) << torch.arange(32, device=flat.device)).sum(1)                # in [0, 2^32)
        return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)                         # the same 32 bits as a signed word

    @staticmethod
    def dilate_mask(mask, n):
        """``mask [X,Y,Z]`` grown by ``n`` cells along each axis (a cell is set iff a cell within ``n`` steps on every axis is)"""
        n = int(n)
        if n <= 0:
            return mask
        m = torch.nn.functional.max_pool3d(mask[None, None].to(torch.float32), kernel_size=2 * n + 1, stride=1, padding=n)
        return m[0, 0] > 0

    @classmethod
    def from_mask(cls, mask, lo, hi):
        """The grid of a bool ``mask [X,Y,Z]`` (a CPU or a GPU tensor; ``bits`` stays on its device) on the box ``lo .. hi``"""
        mask = torch.as_tensor(mask)
        if mask.dim() != 3 or mask.dtype != torch.bool:
            raise ValueError(f"mask must be a bool tensor [X,Y,Z], got {mask.dtype} {tuple(mask.shape)}")
        return cls(cls.pack_mask(mask), lo, hi, mask.shape, mask.float().mean().item() if mask.numel() else 0.)

    @classmethod
    @torch.no_grad()
    def from_network(cls, net, lo, hi, res, threshold, dilate=1, chunk=1 << 20, eps_alpha=None):
        """The grid of a trained network: ``density_grid(..., return_raw=True)`` on the ``(X+1, Y+1, Z+1)`` lattice of cell corners; a cell
        is occupied iff any of its 8 corners has ``softplus(max_k alpha) > threshold`` (the largest density over the K latents); the mask
        is then grown by ``dilate`` cells along each axis, which covers surfaces that pass between corners."""
        X, Y, Z = (int(r) for r in res)
        alpha = density_grid(net, lo, hi, (X + 1, Y + 1, Z + 1), chunk=chunk, eps_alpha=eps_alpha, return_raw=True)["alpha"]
        c = torch.nn.functional.softplus(alpha.max(-1).values) > float(threshold)
        cell = torch.zeros(X, Y, Z, dtype=torch.bool, device=c.device)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    cell |= c[dx:dx + X, dy:dy + Y, dz:dz + Z]
        return cls.from_mask(cls.dilate_mask(cell, dilate), lo, hi)

    def sampler(self, **kw):
        """An ``OccupancySampler`` on this grid (``bins``, ``pad``, ``outside``)"""
        return OccupancySampler(self, **kw)


class OccupancySampler:
    """How rays are SAMPLED through an ``OccupancyGrid`` (``api.warp_z_vals``, ``api.render_rays_warped``, ``Trainer.step(occupancy=)``,
    ``render_uncertainty(occupancy=)``): every ray is cut into ``bins`` equal depth bins between its own near and far (columns 6, 7 of the
    packed ray), a bin is occupied iff one of three probe depths in it lies in an occupied cell, occupied runs are grown by ``pad`` bins on
    both sides along the ray (a 1-D max-pool; 0 = none), and all S depths of the ray are placed in the occupied bins.  ``outside`` =
    ``"cull"`` / ``"keep"`` is the probe's answer outside the grid's box, as in ``api.cull_points``.  ``1 <= bins <= 4096``."""

    def __init__(self, grid, bins=512, pad=1, outside="cull"):
        if not isinstance(grid, OccupancyGrid):
            raise TypeError("OccupancySampler needs an OccupancyGrid")
        if int(bins) != bins or not 1 <= int(bins) <= 4096:
            raise ValueError(f"bins must be an integer in [1, 4096], got {bins!r}")
        if int(pad) != pad or int(pad) < 0:
            raise ValueError(f"pad must be an integer >= 0, got {pad!r}")
        if outside not in ("keep", "cull"):
            raise ValueError(f"outside must be 'keep' or 'cull', got {outside!r}")
        self.grid, self.bins, self.pad, self.outside = grid, int(bins), int(pad), outside


def sparsification_plot(var_vec, err_vec, uncert_type='c', err_type='rmse'):
    """HLP:382-438: error of the pixels that remain after removing the top r% by (a) error itself - the oracle
    curve - and (b) predicted uncertainty; r = 0, 1, ..., 99 %.  Returns ``(ause_err, ause_err_by_var)`` as numpy."""
    ratio_removed = np.linspace(0, 1, 100, endpoint=False)
    n = len(err_vec)
    agg = (lambda e: torch.sqrt(e.mean())) if err_type == 'rmse' else (lambda e: e.mean())
    err_sorted, _ = torch.sort(err_vec)
    oracle = np.array([agg(err_sorted[0:int((1 - r) * n)]).cpu().numpy() for r in ratio_removed])
    std = torch.sqrt(var_vec)
    _, idx = torch.sort(std, descending=(uncert_type == 'c'))
    by_var_sorted = err_vec[idx]
    by_var = np.array([agg(by_var_sorted[0:int((1 - r) * n)]).cpu().numpy() for r in ratio_removed])
    return oracle, by_var


def ause(var_vec, err_vec, err_type='rmse'):
    """Area under the sparsification error (mean gap between the by-uncertainty curve and the oracle curve).
    NOTE the reference's ``uncert_type='c'`` sorts DESCENDING and then keeps the head, i.e. it keeps the MOST
    uncertain pixels (HLP:414-416,424); AUSE as usually defined removes them, which is ``uncert_type='v'``."""
    o, v = sparsification_plot(var_vec, err_vec, uncert_type='v', err_type=err_type)
    return float(np.mean(v - o))


def sparsification_curves(var_vec, err_vec, uncert_type='c', err_type='rmse'):
    """``sparsification_plot`` (same arguments, same return) without its 200 device-to-host round trips: one sort of the errors, one of
    the uncertainties, ONE fp64 cumulative sum over both orderings, the reference's 100 prefix lengths ``int((1 - r) * n)`` computed on
    the host exactly as HLP:405-406 computes them, the 200 prefix means gathered on the device and ONE copy to the host.  Differs from
    ``sparsification_plot`` only in that a prefix mean is accumulated in fp64 instead of fp32 (a prefix of length 0 is nan in both)."""
    ratio_removed = np.linspace(0, 1, 100, endpoint=False)
    n = len(err_vec)
    counts = torch.tensor([int((1 - r) * n) for r in ratio_removed], dtype=torch.int64)
    err_sorted, _ = torch.sort(err_vec)
    _, idx = torch.sort(torch.sqrt(var_vec), descending=(uncert_type == 'c'))
    both = torch.stack([err_sorted, err_vec[idx]]).double()
    del err_sorted, idx
    both.cumsum_(1)
    counts = counts.to(both.device)
    sums = both[:, (counts - 1).clamp_(min=0)]
    means = torch.where(counts > 0, sums, torch.zeros_like(sums)) / counts         # (0 / 0 = nan: the mean of an empty prefix)
    if err_type == 'rmse':
        means = torch.sqrt(means)
    curves = means.to(err_vec.dtype).cpu().numpy()
    return curves[0], curves[1]


def ause_fused(var_vec, err_vec, err_type='rmse'):
    """``ause`` on ``sparsification_curves``: same ``uncert_type='v'`` (ascending sort of the uncertainty, head kept = the most uncertain
    pixels REMOVED, AUSE as usually defined; the reference's ``'c'`` keeps them, see ``ause``)."""
    o, v = sparsification_curves(var_vec, err_vec, uncert_type='v', err_type=err_type)
    return float(np.mean(v - o))


def _central_inside(levels, K):
    """For each central level p (a fraction a/b, b <= 1000) the 2K+1 flags ``b |code - K| <= a K`` over code = 0..2K, and ``ideal``: the same
    rule over the K+1 equally likely values of #below of a calibrated ensemble (code = 2 #below)."""
    from fractions import Fraction
    codes, below = np.arange(2 * K + 1), 2 * np.arange(K + 1)
    inside, ideal = [], []
    for p in levels:
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"a central level must lie in [0, 1], got {p!r}")
        f = Fraction(float(p)).limit_denominator(1000)
        a, b = f.numerator, f.denominator
        inside.append(b * np.abs(codes - K) <= a * K)
        ideal.append(float(np.count_nonzero(b * np.abs(below - K) <= a * K)) / (K + 1))
    return np.stack(inside), np.asarray(ideal)


@torch.no_grad()
def calibration(rank_code, K, levels=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9), group=None, n_groups=None):
    """Calibration of a K-member ensemble from the ranks of the truth among its samples: ``rank_code`` (any shape, integer) as
    ``api.k_scores`` / ``render_uncertainty(scores=)`` give it, ``2 #{x_k < y} + #{x_k == y}`` in [0, 2K], -1 = not scored (a NaN).
    One ``bincount`` on the device and one copy of its 2K+2 integers (per group) to the host.  Returns a dict of host values:

    * ``pit_hist [2K+1]`` (int64): how many rows have each code; ``n`` their number, ``n_invalid`` the rows with code -1 (left out);
    * ``coverage [len(levels)]``: the share of rows whose truth lies inside the central interval of level p.  Defined from the rank, in
      integers, so it is exact: with p = j/10 a row is inside iff ``10 |rank_code - K| <= j K`` (in general p = a/b: ``b |rank_code - K| <= a K``);
    * ``ideal``: the coverage a perfectly calibrated K-member ensemble shows under that rule - the truth is exchangeable with the samples,
      so #below is uniform on 0..K: ``ideal_j = #{b in 0..K : 10 |2b - K| <= j K} / (K + 1)`` (not p itself: K + 1 ranks are a coarse grid);
    * ``auce`` = ``mean_j |coverage_j - ideal_j|``, the area under the calibration error (nan without a valid row).

    ``group`` (an integer tensor of the shape of ``rank_code``, values 0..G-1, e.g. the channel) gives every result a leading ``[G]`` axis (``n_groups`` = G saves the copy of ``group.max()``)."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be at least 1, got {K}")
    code = rank_code.reshape(-1).to(torch.int64)
    width = 2 * K + 2
    G = 1
    idx = code + 1
    if group is not None:
        if tuple(group.shape) != tuple(rank_code.shape):
            raise ValueError(f"group must have the shape of rank_code {tuple(rank_code.shape)}, got {tuple(group.shape)}")
        grp = group.reshape(-1).to(code.device, torch.int64)
        G = int(n_groups) if n_groups is not None else (int(grp.max().item()) + 1 if grp.numel() else 1)
        idx = idx + grp * width
    counts = torch.bincount(idx, minlength=G * width)
    if counts.numel() != G * width:
        raise ValueError(f"rank_code must lie in [-1, 2K] = [-1, {2 * K}] (and group in [0, {G - 1}])")
    counts = counts.cpu().numpy().astype(np.int64).reshape(G, width)
    inside, ideal = _central_inside(levels, K)
    hist, n_invalid = counts[:, 1:], counts[:, 0]
    n = hist.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        coverage = (hist[:, None, :] * inside[None]).sum(-1) / n[:, None].astype(np.float64)
    auce = np.abs(coverage - ideal[None]).mean(1)
    ideal_g = np.broadcast_to(ideal, coverage.shape).copy()
    if group is None:
        return dict(pit_hist=hist[0], coverage=coverage[0], ideal=ideal_g[0], auce=float(auce[0]), n=int(n[0]), n_invalid=int(n_invalid[0]))
    return dict(pit_hist=hist, coverage=coverage, ideal=ideal_g, auce=auce, n=n, n_invalid=n_invalid)


_calibration = calibration      # (image_metrics has an argument of that name)


@torch.no_grad()
def image_metrics(H, W, focal, c2w, network_fn, gt, gt_depth=None, calibration=False, ssim=False, **render_kw):
    """The per-view numbers of the paper's tables for the image seen from ``c2w`` against ``gt [H,W,3]`` (and ``gt_depth [H,W]``): one
    ``render_uncertainty(stats="ext", gt=gt)`` launch - no per-K map exists anywhere - plus the sorts of ``ause_fused``.  Returns floats:

    * ``mse``, ``psnr`` = ``mse2psnr(img2mse(rgb_mean, gt))`` (RUN:1028-1029), ``loss_nll`` (RUN:1042);
    * ``ause_rgb_rmse`` / ``ause_rgb_mae``: uncertainty = mean over the channels of ``rgb_unc ** 2`` (a variance: the helpers take its
      root), error = mean over the channels of the squared / absolute error of the K-mean colour, per pixel;
    * with ``gt_depth``: ``ause_depth_rmse`` / ``ause_depth_mae`` from ``depth_mean`` and ``depth_unc ** 2`` likewise.

    All AUSE figures use ``uncert_type='v'`` like ``ause`` (the most uncertain pixels are removed first; the reference's ``'c'`` keeps
    them, HLP:414-416,424).  ``render_kw``: near, far, ndc, lindisp, white_bkgd, t_vals of ``render_uncertainty``.

    ``calibration=True`` also scores the K samples of every pixel as an ensemble (``render_uncertainty(scores=)``: the rows are walked in
    chunks, each with a second, maps-only forward): ``crps_rgb`` (the mean CRPS over pixels and channels), ``auce_rgb`` and ``coverage_rgb``
    (a list: the coverage of the central 10 % .. 90 % intervals, see ``calibration``); with ``gt_depth`` also ``crps_depth``, ``auce_depth``
    and ``coverage_depth``.  With the default the returned dict is what it was.

    ``ssim=True`` adds ``ssim`` (skimage's default: 7 x 7 uniform window, ``data_range=1``) and ``ssim_gaussian`` (Wang et al.: 11 x 11,
    sigma = 1.5) of the K-mean image that the one launch already returns against ``gt`` (``cfnerf_amd.ssim``): no second render.  With the
    default the returned dict is what it was."""
    for k in ("rows", "want_maps", "stats", "gt", "scores"):
        if k in render_kw:
            raise TypeError(f"image_metrics renders the whole image with stats='ext' and its own gt: {k}= is not an argument")
    if calibration:
        r = render_uncertainty(H, W, focal, c2w, network_fn, gt=gt, stats="ext", scores=(0.5,), gt_depth=gt_depth, **render_kw)
    else:
        r = render_uncertainty(H, W, focal, c2w, network_fn, gt=gt, stats="ext", **render_kw)
    mse = r["mse"]
    out = dict(mse=float(mse), psnr=float(-10. * torch.log(mse) / math.log(10.)), loss_nll=float(r["loss_nll"]))
    var = (r["rgb_unc"] ** 2).mean(-1).reshape(-1)
    sq = r["sq_err"]
    out["ause_rgb_rmse"] = ause_fused(var, sq.mean(-1).reshape(-1), 'rmse')
    out["ause_rgb_mae"] = ause_fused(var, torch.sqrt(sq).mean(-1).reshape(-1), 'mae')
    if gt_depth is not None:
        d = r["depth_mean"] - gt_depth.to(sq.device, torch.float32).reshape(H, W)
        var = (r["depth_unc"] ** 2).reshape(-1)
        out["ause_depth_rmse"] = ause_fused(var, (d * d).reshape(-1), 'rmse')
        out["ause_depth_mae"] = ause_fused(var, d.abs().reshape(-1), 'mae')
    if calibration:
        K = _unwrap(network_fn).K_samples
        for what in ("rgb",) + (("depth",) if gt_depth is not None else ()):
            c = _calibration(r[what + "_rank"], K)
            out["crps_" + what] = float(r[what + "_crps"].mean())
            out["auce_" + what] = c["auce"]
            out["coverage_" + what] = [float(v) for v in c["coverage"]]
    if ssim:
        img, ref = r["rgb_mean"], gt.to(sq.device, torch.float32).reshape(H, W, 3)
        out["ssim"] = float(_ssim(img, ref))
        out["ssim_gaussian"] = float(_ssim(img, ref, window="gaussian"))
    return out
