"""GPU: the image similarity (CFNERF_MODE_SSIM, cfnerf_ssim.hip) - ssim_kernel against the fp64 yardstick of ssim_common on the same fp32
images, ``cfnerf_amd.ssim`` and ``image_metrics(ssim=True)``.

The shapes (ssim_common.SHAPES) sit on and one past the edges of the kernel's 32 x 32 output tile.  Bounds, none taken from what the kernel
gives (they come from a numpy probe of fp32 arithmetic on the CPU):
* per pixel, every case and shape: max |kernel - fp64| <= max(the same maximum of ``naive32``, 4 x 2^-24); on ``bright_flat`` also <= 1/100
  of ``naive32``'s;
* the image mean within 1e-6 of fp64;
* ``ssim(x, x)`` is 1.0 bit for bit, map and mean;
* ``one_nan``: NaN exactly on the win x win footprint clipped to the interior and in that image's mean, every other output the clean run's
  bits;
* two runs bit-equal; an image of a batch bit-equal to the same image alone; nothing is written outside the outputs.
The measured maxima are kept in profiles/r22_ssim_errors.txt (CFNERF_SSIM_ERRORS=<file> appends them)."""
import os

import numpy as np
import pytest
import torch

import cfnerf_amd
import ssim_common as SC
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
from oracle import cfnerf_oracle as O
from util_hip import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = os.environ.get("CFNERF_SSIM_ERRORS")          # development aid: append every measured error to this file
POISON = -12345.0
GUARD = 64                                              # poisoned floats behind every output: nothing may be written there
FLOOR = 4 * 2.0 ** -24


def _record(line):
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit for bit (NaN payloads and the sign of zero included)"""
    return torch.equal(_bits(a), _bits(b))


def launch(x, y, win, want_map=True, want_mean=True):
    """one call on device tensors x, y [B,H,W,C] with the window of the shape table -> (map [B,Hi,Wi,C], mean [B,C]), every buffer poisoned
    first and followed by a guard that must come back untouched"""
    B, H, W, C_ = x.shape
    taps, cov = L.ssim_window(SC.window_kind(win), win)
    n_map, n_mean = B * (H - win + 1) * (W - win + 1) * C_, B * C_
    n_scr = L.ssim_scratch_floats(B, C_, H, W, win)
    bmap, bmean = torch.full((n_map + GUARD,), POISON, device=DEV), torch.full((n_mean + GUARD,), POISON, device=DEV)
    bscr = torch.full((n_scr + GUARD,), POISON, device=DEV)
    L.ssim(x, y, B, H, W, C_, taps, cov, 1e-4, 9e-4, ssim_map=bmap if want_map else None, mean=bmean if want_mean else None,
           scratch=bscr if want_mean else None)
    for buf, n, used in ((bmap, n_map, want_map), (bmean, n_mean, want_mean), (bscr, n_scr, want_mean)):
        assert bool((buf[n if used else 0:] == POISON).all()), "written outside an output"
    assert not want_mean or bool((bscr[:n_scr] != POISON).all()), "a tile's partial sum was not written"
    return bmap[:n_map].reshape(B, H - win + 1, W - win + 1, C_), bmean[:n_mean].reshape(B, C_)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared cases are read-only)


def _image_mean(mean_bc):
    """[B,C] fp32 channel means -> one fp64 number per image, as ``cfnerf_amd.ssim`` forms it"""
    return mean_bc.double().mean(-1).cpu().numpy()


@pytest.mark.parametrize("name", SC.CASES)
@pytest.mark.parametrize("H, W, C_, win", SC.SHAPES)
def test_kernel_against_the_fp64_yardstick(H, W, C_, win, name):
    x, y = SC.make_case(name, H, W, C_)
    (ref, ref_mean), (naive, naive_mean) = SC.reference(name, H, W, C_, win)
    xd, yd = _dev(x)[None], _dev(y)[None]
    smap, mean = launch(xd, yd, win)
    again_map, again_mean = launch(xd, yd, win)
    assert _same(smap, again_map) and _same(mean, again_mean), "two runs differ"
    got = smap[0].cpu().numpy()
    err, err_naive = SC.max_err(got, ref), SC.max_err(naive, ref)          # (asserts that the NaN entries are the yardstick's)
    got_mean = float(_image_mean(mean)[0])
    mean_err = abs(got_mean - ref_mean)
    _record(f"{H:3d}x{W:2d}x{C_} win {win:2d} {name:12s} map: kernel {err:.2e} naive32 {err_naive:.2e}   mean: kernel {mean_err:.1e} "
            f"naive32 {abs(naive_mean - ref_mean):.1e}")
    print(f"\n{name} {H}x{W}x{C_} win {win}: map error {err:.3e} (naive32 {err_naive:.3e}), mean error {mean_err:.3e}")
    assert err <= max(err_naive, FLOOR), (err, err_naive)
    if name == "bright_flat":
        assert err <= err_naive / 100, (err, err_naive)
    if name == "one_nan":
        assert np.isnan(got_mean) and np.isnan(ref_mean)
    else:
        assert mean_err <= 1e-6, (got_mean, ref_mean)
    # the mean is the mean of the map as written: fp64 over the fp32 values, rounded once - within one fp32 unit of numpy's (the kernel adds
    # in another fixed order, so a rounding tie may fall the other way)
    want = got.astype(np.float64).mean(axis=(0, 1)).astype(np.float32)
    have = mean[0].cpu().numpy()
    assert np.array_equal(np.isnan(have), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(have[ok] - want[ok]) <= np.spacing(np.abs(want[ok]))).all(), (have, want)
    # the public entry point: the same launch, with and without the map
    value, full = cfnerf_amd.ssim(xd[0], yd[0], window=SC.window_kind(win), win_size=win, full=True)
    alone = cfnerf_amd.ssim(xd[0], yd[0], window=SC.window_kind(win), win_size=win)
    assert _same(full, smap[0]) and value.shape == () and _same(value, alone)
    assert np.array_equal(value.cpu().numpy(), np.float32(_image_mean(mean)[0]), equal_nan=True)
    only_mean = launch(xd, yd, win, want_map=False)[1]
    only_map = launch(xd, yd, win, want_mean=False)[0]
    assert _same(only_mean, mean) and _same(only_map, smap)


@pytest.mark.parametrize("H, W, C_, win", SC.SHAPES)
def test_ssim_of_an_image_with_itself_is_exactly_one(H, W, C_, win):
    for name in ("identical", "render", "bright_flat"):
        x = _dev(SC.make_case(name, H, W, C_)[0])[None]
        smap, mean = launch(x, x.clone(), win)
        assert bool((smap == 1.0).all()) and bool((mean == 1.0).all()), name
    value, full = cfnerf_amd.ssim(x[0], x[0], window=SC.window_kind(win), win_size=win, full=True)
    assert float(value) == 1.0 and bool((full == 1.0).all())


@pytest.mark.parametrize("H, W, C_, win", SC.SHAPES)
def test_one_nan_reaches_its_footprint_and_its_mean_and_nothing_else(H, W, C_, win):
    x, y = SC.make_case("one_nan", H, W, C_)
    cx, cy = SC.make_case("render", H, W, C_)
    r, c, ch = SC.NAN_AT(H, W, C_)
    assert np.isnan(x[r, c, ch]) and np.array_equal(y, cy) and int(np.isnan(x).sum()) == 1 and np.array_equal(np.isnan(x) | (x == cx), np.ones(x.shape, bool))
    smap, mean = launch(_dev(x)[None], _dev(y)[None], win)
    clean_map, clean_mean = launch(_dev(cx)[None], _dev(cy)[None], win)
    want = torch.zeros(smap.shape, dtype=torch.bool, device=DEV)
    want[0, max(r - win + 1, 0):r + 1, max(c - win + 1, 0):c + 1, ch] = True
    assert bool(want.any()) and not bool(torch.isnan(clean_map).any())
    assert torch.equal(torch.isnan(smap), want)
    assert torch.equal(_bits(smap)[~want], _bits(clean_map)[~want])
    nan_mean = torch.zeros(1, C_, dtype=torch.bool, device=DEV)
    nan_mean[0, ch] = True
    assert torch.equal(torch.isnan(mean), nan_mean) and torch.equal(_bits(mean)[~nan_mean], _bits(clean_mean)[~nan_mean])
    assert bool(torch.isnan(cfnerf_amd.ssim(_dev(x), _dev(y), window=SC.window_kind(win), win_size=win)))


def test_an_image_of_a_batch_equals_the_same_image_alone():
    H, W, C_, win = 45, 70, 3, 7
    pairs = [SC.make_case("render", H, W, C_), SC.make_case("identical", H, W, C_), SC.make_case("one_nan", H, W, C_)]
    x, y = _dev(np.stack([p[0] for p in pairs])), _dev(np.stack([p[1] for p in pairs]))
    smap, mean = launch(x, y, win)
    again_map, again_mean = launch(x, y, win)
    assert _same(smap, again_map) and _same(mean, again_mean), "two runs differ"
    for b in range(3):
        one_map, one_mean = launch(x[b:b + 1].contiguous(), y[b:b + 1].contiguous(), win)
        assert _same(smap[b], one_map[0]) and _same(mean[b], one_mean[0]), b
    assert bool((smap[1] == 1.0).all()) and bool((mean[1] == 1.0).all())
    assert not bool(torch.isnan(smap[0]).any()) and bool(torch.isnan(mean[2]).any())
    value, full = cfnerf_amd.ssim(x, y, full=True)
    assert value.shape == (3,) and _same(full, smap) and float(value[1]) == 1.0 and bool(torch.isnan(value[2]))
    assert np.array_equal(value.cpu().numpy(), _image_mean(mean).astype(np.float32), equal_nan=True)
    assert cfnerf_amd.ssim(x[:0], y[:0]).shape == (0,)


def test_the_public_entry_point_takes_three_layouts_and_a_data_range():
    H, W, C_ = 45, 70, 3
    x, y = (_dev(a) for a in SC.make_case("render", H, W, C_))
    v3, m3 = cfnerf_amd.ssim(x, y, full=True)
    v4, m4 = cfnerf_amd.ssim(x[None], y[None], full=True)
    assert v3.shape == () and m3.shape == (H - 6, W - 6, C_) and v4.shape == (1,) and m4.shape == (1, H - 6, W - 6, C_)
    assert _same(v3, v4[0]) and _same(m3, m4[0])
    v2, m2 = cfnerf_amd.ssim(x[..., 1], y[..., 1], full=True)          # [H,W], and not contiguous
    assert v2.shape == () and m2.shape == (H - 6, W - 6) and _same(m2, m3[..., 1])
    vg, mg = cfnerf_amd.ssim(x, y, window="gaussian", full=True)
    assert mg.shape == (H - 10, W - 10, C_)
    ref = SC.yardstick(x.cpu().numpy(), y.cpu().numpy(), "gaussian", 11)
    assert SC.max_err(mg.cpu().numpy(), ref[0]) <= FLOOR and abs(float(vg) - ref[1]) <= 1e-6
    # 8-bit levels: the constants follow data_range
    x8, y8 = torch.round(x * 255), torch.round(y * 255)
    v8, m8 = cfnerf_amd.ssim(x8, y8, data_range=255.0, full=True)
    ref8 = SC.yardstick(x8.cpu().numpy(), y8.cpu().numpy(), "uniform", 7, data_range=255.0)
    assert SC.max_err(m8.cpu().numpy(), ref8[0]) <= FLOOR and abs(float(v8) - ref8[1]) <= 1e-6
    with pytest.raises(RuntimeError):
        cfnerf_amd.ssim(x.cpu(), y.cpu())
    for bad in (lambda: cfnerf_amd.ssim(x, y[:-1]), lambda: cfnerf_amd.ssim(x[:6], y[:6]), lambda: cfnerf_amd.ssim(x, y, win_size=8),
                lambda: cfnerf_amd.ssim(x, y, data_range=0.0), lambda: cfnerf_amd.ssim(x, y, window="hann"),
                lambda: cfnerf_amd.ssim(x[None, None], y[None, None]), lambda: cfnerf_amd.ssim(x[:, :, :1].expand(H, W, 5), y[:, :, :1].expand(H, W, 5))):
        with pytest.raises(ValueError):
            bad()


def test_model_entry_points_refuse_the_bit_by_name():
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    _, _, _, model, _, _ = build_model(cfg, 5)
    net, lib = model.module, L.lib()
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_network_fwd(net.handle, None, None, 4, 4, L.F_TRAIN | L.F_STASH | L.MODE_SSIM, None, None, L.stream())
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_MODE_SSIM" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 128, 4, L.MODE_SSIM, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_MODE_SSIM" in err(), err()
    rc = lib.cfnerf_render_fwd(net.handle, None, None, None, None, None, 4, 128, 4, L.F_TRAIN | L.F_STASH | L.MODE_SSIM, *([None] * 8), L.stream())
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_MODE_SSIM" in err(), err()


def test_image_metrics_with_ssim():
    H_, W_, focal, S_ = 12, 16, 14.0, 8
    pose = torch.tensor([[1, 0, 0, 0.1], [0, 1, 0, -0.1], [0, 0, 1, 4.0]], dtype=torch.float32)
    cfg = O.OracleCfg(netwidth=64, K_samples=3)
    _, _, _, model, _, _ = build_model(cfg, 22, no_ndc=True)
    kw = dict(near=2.0, far=6.0, ndc=False, t_vals=torch.linspace(0., 1., S_, device=DEV))
    gt = torch.tensor(np.random.default_rng(0).uniform(0, 1, (H_, W_, 3)), dtype=torch.float32)
    base = E.image_metrics(H_, W_, focal, pose, model, gt, **kw)
    assert set(base) == {"mse", "psnr", "loss_nll", "ause_rgb_rmse", "ause_rgb_mae"}
    got = E.image_metrics(H_, W_, focal, pose, model, gt, ssim=True, **kw)
    assert set(got) == set(base) | {"ssim", "ssim_gaussian"}
    for k in base:
        assert got[k] == base[k] or (np.isnan(got[k]) and np.isnan(base[k])), k
    r = E.render_uncertainty(H_, W_, focal, pose, model, gt=gt, stats="ext", **kw)
    assert got["ssim"] == float(cfnerf_amd.ssim(r["rgb_mean"], gt.to(DEV)))
    assert got["ssim_gaussian"] == float(cfnerf_amd.ssim(r["rgb_mean"], gt.to(DEV), window="gaussian"))
    ref = SC.yardstick(r["rgb_mean"].cpu().numpy(), gt.numpy(), "uniform", 7)[1]
    assert abs(got["ssim"] - ref) <= 1e-6 and -1.0 <= got["ssim"] <= 1.0 and got["ssim"] != got["ssim_gaussian"]
