"""GPU: the ensemble scores (CFNERF_F_KSCORES, cfnerf_kscores.hip) - k_scores_kernel against the fp64 yardstick of kscores_common on the same
fp32 inputs, ``cfnerf_amd.k_scores``, ``render_uncertainty(scores=)`` and ``image_metrics(calibration=True)``.

Bounds (set with the kernel, none taken from what it gives):
* ``sorted``: non-decreasing, equal to torch.sort as floats, and a permutation of the row's 32-bit patterns; ``rank_code`` and ``pit`` exact;
* ``quantiles`` at (0, 0.05, 0.25, 0.5, 0.75, 0.95, 1): bit-equal to the order statistic where frac == 0, elsewhere
  |err| <= 4 x 2^-24 max(|x_(lo)|, |x_(hi)|) against fp64 numpy.quantile (three roundings and the rounding of frac; the same expression in
  fp32 numpy stays within 2.05 of those units on these inputs);
* ``crps``: |err| <= 16 x 2^-24 (A + B), A and B from fp64 (<= 128 non-negative terms in a tree of depth 7, three roundings per term, two
  divisions, the final difference; fp32 numpy on the same form reaches 7.9 of those units).
On the row of denormals both scales are floored at the smallest normal number, 2^-126: below it the spacing of fp32 is absolute (2^-149), so no
fp32 result can follow a bound relative to a denormal magnitude.
Rows whose fp64 reference is not finite (the +-inf row) must be non-finite in the kernel too.  The measured maxima per case are kept in
profiles/r21_kscores_errors.txt (CFNERF_KSCORES_ERRORS=<file> appends them)."""
import os

import numpy as np
import pytest
import torch

import cfnerf_amd
import kscores_common as KS
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
from oracle import cfnerf_oracle as O
from util_hip import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = os.environ.get("CFNERF_KSCORES_ERRORS")          # development aid: append every measured error to this file
KS_ALL = [1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 127, 128]
MS_ALL = [1, 5, 64, 1000]
POISON = -12345.0
FLT_MIN = 2.0 ** -126          # below it fp32 is spaced absolutely, 2^-149 = 2^-23 FLT_MIN: a bound relative to a denormal magnitude is floored there


def _record(case, what, units):
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(f"{case:16s} {what:10s} max error {units:7.3f} units of its bound's 2^-24 scale\n")


def launch(x, y=None, levels=KS.LEVELS, want=("sorted", "quantiles", "rank_code", "pit", "crps")):
    """one launch on device tensors x [M,K], y [M] -> every output buffer, poisoned first; the ones in ``want`` are passed to the kernel"""
    M, K = x.shape
    lv = L.quantile_levels(levels, K)
    o = dict(sorted=torch.full((M, K), POISON, device=DEV), quantiles=torch.full((M, len(lv)), POISON, device=DEV),
             rank_code=torch.full((M,), -777, dtype=torch.int32, device=DEV), pit=torch.full((M,), POISON, device=DEV),
             crps=torch.full((M,), POISON, device=DEV))
    g = lambda k: o[k] if k in want else None
    L.k_scores(x, M, K, target=y, sorted_out=g("sorted"), quantiles=g("quantiles"), levels=lv, rank_code=g("rank_code"), pit=g("pit"), crps=g("crps"))
    return o


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """bit for bit (NaN payloads and the sign of zero included)"""
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("M", MS_ALL)
@pytest.mark.parametrize("K", KS_ALL)
def test_kernel_against_the_fp64_yardstick(K, M):
    x, y = KS.make_rows(M, K, seed=1000 * K + M)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    got = launch(xd, yd)
    again = launch(xd, yd)
    for k in got:
        assert _same(got[k], again[k]), k + ": two runs differ"
    case = f"K={K} M={M}"
    # ---- sorted
    s = got["sorted"]
    assert bool((s[:, 1:] >= s[:, :-1]).all())
    assert torch.equal(s, torch.sort(xd, dim=1).values)
    assert torch.equal(torch.sort(_bits(s), dim=1).values, torch.sort(_bits(xd), dim=1).values), "not a permutation of the bit patterns"
    s_np = s.cpu().numpy()
    # ---- rank_code, pit
    code = KS.rank_code(x, y)
    assert np.array_equal(got["rank_code"].cpu().numpy(), code)
    assert np.array_equal(got["pit"].cpu().numpy().view(np.int32), KS.pit_of(code, K).view(np.int32))
    # ---- quantiles
    q64, lo, hi, exact = KS.quantiles64(x)
    q = got["quantiles"].cpu().numpy()
    worst = 0.0
    for t in range(len(KS.LEVELS)):
        xl, xh = s_np[:, lo[t]], s_np[:, hi[t]]
        if exact[t]:
            assert np.array_equal(q[:, t].view(np.int32), xl.view(np.int32)), f"{case} level {KS.LEVELS[t]}: not the order statistic's bits"
            continue
        fin = np.isfinite(xl) & np.isfinite(xh)
        assert not np.isfinite(q[~fin, t]).any()
        scale = np.maximum(np.maximum(np.abs(xl[fin]), np.abs(xh[fin])).astype(np.float64), FLT_MIN * ((xl[fin] != 0) | (xh[fin] != 0)))
        err = np.abs(q[fin, t].astype(np.float64) - q64[fin, t])
        units = (err[scale > 0] / (KS.U24 * scale[scale > 0])).max() if (scale > 0).any() else 0.0
        worst = max(worst, units)
        assert (err <= 4 * KS.U24 * scale).all(), f"{case} level {KS.LEVELS[t]}: {units:.2f} units"
    _record(case, "quantiles", worst)
    # ---- crps
    A, B = KS.crps_terms(x, y)
    c = got["crps"].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = A - B
    fin = np.isfinite(ref)
    assert not np.isfinite(c[~fin]).any()
    err, scale = np.abs(c[fin] - ref[fin]), (A + B)[fin]
    scale = np.maximum(scale, FLT_MIN * (scale > 0))
    assert (err[scale == 0] == 0).all()
    units = (err[scale > 0] / (KS.U24 * scale[scale > 0])).max() if (scale > 0).any() else 0.0
    _record(case, "crps", units)
    assert (err <= 16 * KS.U24 * scale).all(), f"{case}: crps {units:.2f} units"
    if K == 1:
        assert np.array_equal(got["crps"].cpu().numpy()[fin], np.abs(x[fin, 0] - y[fin]))


@pytest.mark.parametrize("K", [3, 4, 33, 64, 65])
def test_a_nan_row_gets_nan_scores_and_leaves_its_neighbours_alone(K):
    M = 70
    x, y = KS.make_rows(M, K, seed=K, special=False)
    clean = launch(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    xn, yn = x.copy(), y.copy()
    xn[5, K // 2] = np.nan                   # a NaN sample (rows 4..7 share a wave segment group at K <= 16; every row a wave's neighbour otherwise)
    xn[6, 0] = -np.nan
    yn[9] = np.nan                           # a NaN target
    got = launch(torch.from_numpy(xn).to(DEV), torch.from_numpy(yn).to(DEV))
    bad = np.array([5, 6, 9])
    ok = np.setdiff1d(np.arange(M), bad)
    for k in ("quantiles", "pit", "crps"):
        assert bool(torch.isnan(got[k][bad]).all()), k
        assert torch.equal(_bits(got[k][ok]), _bits(clean[k][ok])), k
    assert got["rank_code"][bad].tolist() == [-1, -1, -1] and torch.equal(got["rank_code"][ok], clean["rank_code"][ok])
    assert torch.equal(_bits(got["sorted"][ok]), _bits(clean["sorted"][ok])) and torch.equal(_bits(got["sorted"][9]), _bits(clean["sorted"][9]))
    # NaN orders after +inf, as torch.sort does, and keeps its bits
    for r in (5, 6):
        s = got["sorted"][r]
        assert bool(torch.isnan(s[-1])) and not bool(torch.isnan(s[:-1]).any()) and bool((s[1:-1] >= s[:-2]).all())
        assert torch.equal(torch.sort(_bits(s)).values, torch.sort(_bits(torch.from_numpy(xn[r]).to(DEV))).values)
    # without a target: the NaN rows' quantiles alone
    q = launch(torch.from_numpy(xn).to(DEV), None, want=("quantiles",))["quantiles"]
    assert bool(torch.isnan(q[[5, 6]]).all()) and torch.equal(_bits(q[9]), _bits(clean["quantiles"][9]))


@pytest.mark.parametrize("K", [2, 4, 5, 33, 128])
def test_rows_scored_alone_have_the_bits_of_the_full_launch(K):
    M, a, b = 1000, 3, 778                   # neither a multiple of the 64 / Kp rows of a wave (Kp <= 32), nor of the 4 waves of a workgroup
    x, y = KS.make_rows(M, K, seed=7 * K)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    full = launch(xd, yd)
    part = launch(xd[a:b].contiguous(), yd[a:b].contiguous())
    for k in full:
        assert _same(full[k][a:b], part[k]), k


def test_an_unrequested_output_is_never_written():
    x, y = KS.make_rows(100, 33, seed=2)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    full = launch(xd, yd)
    for tgt in (yd, None):
        o = launch(xd, tgt, want=("quantiles",))
        assert torch.equal(_bits(o["quantiles"]), _bits(full["quantiles"]))
        assert bool((o["sorted"] == POISON).all()) and bool((o["pit"] == POISON).all()) and bool((o["crps"] == POISON).all())
        assert bool((o["rank_code"] == -777).all())
    o = launch(xd, yd, want=("crps",))
    assert torch.equal(_bits(o["crps"]), _bits(full["crps"])) and bool((o["quantiles"] == POISON).all()) and bool((o["rank_code"] == -777).all())


def test_k_scores_is_the_launch_on_any_leading_shape():
    x, y = KS.make_rows(6 * 5 * 3, 33, seed=4, special=False)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    flat = launch(xd, yd)
    r = cfnerf_amd.k_scores(xd.reshape(6, 5, 3, 33), target=yd.reshape(6, 5, 3), levels=KS.LEVELS, return_sorted=True)
    assert set(r) == {"quantiles", "sorted", "crps", "pit", "rank_code"}
    assert tuple(r["quantiles"].shape) == (6, 5, 3, 7) and tuple(r["sorted"].shape) == (6, 5, 3, 33) and tuple(r["crps"].shape) == (6, 5, 3)
    assert r["rank_code"].dtype == torch.int32
    for k in r:
        assert torch.equal(r[k].reshape(flat[k].shape), flat[k]), k
    assert set(cfnerf_amd.k_scores(xd, levels=(0.5,))) == {"quantiles"}
    assert set(cfnerf_amd.k_scores(xd, target=yd)) == {"crps", "pit", "rank_code"}
    with pytest.raises(ValueError, match="nothing to compute"):
        cfnerf_amd.k_scores(xd)
    with pytest.raises(ValueError, match="target"):
        cfnerf_amd.k_scores(xd, target=yd[:5])
    with pytest.raises(RuntimeError, match="GPU"):
        cfnerf_amd.k_scores(xd.cpu(), levels=(0.5,))
    empty = cfnerf_amd.k_scores(xd[:0], target=yd[:0], levels=(0.5,))
    assert tuple(empty["quantiles"].shape) == (0, 1) and tuple(empty["crps"].shape) == (0,)
    # the median of the calibrated coverage path: codes of an i.i.d. truth are calibrated (a smoke of calibration() on device codes)
    g = torch.Generator().manual_seed(1)
    z = torch.rand(20000, 9, generator=g).to(DEV)
    c = E.calibration(cfnerf_amd.k_scores(z[:, 1:].contiguous(), target=z[:, 0].contiguous())["rank_code"], 8)
    assert c["n"] == 20000 and c["auce"] <= 4 * 0.5 / np.sqrt(20000)


def test_model_entry_points_refuse_the_bit_by_name():
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    _, _, _, model, _, _ = build_model(cfg, 3)
    net, lib = model.module, L.lib()
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_render_fwd(net.handle, None, None, None, None, None, 4, 8, 4, L.F_KSCORES, None, None, None, None, None, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_F_KSCORES" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 8, 4, L.F_KSCORES, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_F_KSCORES" in err(), err()
    rc = lib.cfnerf_network_fwd(net.handle, None, None, 4, 4, L.F_KSCORES, None, None, L.stream())
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_F_KSCORES" in err(), err()


# ---------------------------------------------------------------- render_uncertainty(scores=), image_metrics(calibration=True)
H_, W_, FOCAL_, S_ = 5, 7, 9.0, 8
POSE = torch.tensor([[1, 0, 0, 0.1], [0, 1, 0, -0.1], [0, 0, 1, 4.0]], dtype=torch.float32)
RKW = dict(near=2.0, far=6.0, ndc=False)
_MODELS = {}


def _model(K):
    if K not in _MODELS:
        cfg = O.OracleCfg(netwidth=64, K_samples=K)
        _, _, _, model, _, _ = build_model(cfg, 21 + K, no_ndc=True)
        _MODELS[K] = model
    return _MODELS[K]


def _targets(seed):
    rng = np.random.default_rng(seed)
    return (torch.tensor(rng.uniform(0, 1, (H_, W_, 3)), dtype=torch.float32), torch.tensor(rng.uniform(2, 6, (H_, W_)), dtype=torch.float32))


@pytest.mark.parametrize("stats, want_maps", [("basic", False), ("ext", False), ("ext", True)])
@pytest.mark.parametrize("K", [3, 33])
def test_render_uncertainty_scores_in_chunks(K, stats, want_maps, monkeypatch):
    model = _model(K)
    tv = torch.linspace(0., 1., S_, device=DEV)
    gt, gtd = _targets(K)
    kw = dict(RKW, t_vals=tv, stats=stats, want_maps=want_maps)
    monkeypatch.setattr(E, "_SCORES_RAY_CHUNK", 16)              # 35 rays: chunks of 16, 16 and 3
    got = E.render_uncertainty(H_, W_, FOCAL_, POSE, model, gt=gt, gt_depth=gtd, scores=KS.LEVELS, **kw)
    plain = E.render_uncertainty(H_, W_, FOCAL_, POSE, model, gt=gt, **kw)
    added = {"rgb_q", "depth_q", "rgb_crps", "rgb_pit", "rgb_rank", "depth_crps", "depth_pit", "depth_rank"}
    assert set(got) == set(plain) | added
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    maps = E.render_uncertainty(H_, W_, FOCAL_, POSE, model, **dict(kw, want_maps=True))          # the per-K maps of a single launch
    c = cfnerf_amd.k_scores(maps["rgb_map"], target=gt.to(DEV), levels=KS.LEVELS)
    d = cfnerf_amd.k_scores(maps["depth_map"], target=gtd.to(DEV), levels=KS.LEVELS)
    assert tuple(got["rgb_q"].shape) == (H_, W_, 3, 7) and tuple(got["depth_q"].shape) == (H_, W_, 7) and got["rgb_rank"].dtype == torch.int32
    for name, ref in (("rgb", c), ("depth", d)):
        assert torch.equal(got[name + "_q"], ref["quantiles"]) and torch.equal(got[name + "_crps"], ref["crps"])
        assert torch.equal(got[name + "_pit"], ref["pit"]) and torch.equal(got[name + "_rank"], ref["rank_code"])
    assert bool(torch.isfinite(got["rgb_crps"]).all()) and bool((got["rgb_rank"] >= 0).all())
    # without targets: the quantile maps alone; the median lies between the extremes
    q = E.render_uncertainty(H_, W_, FOCAL_, POSE, model, scores=(0, 0.5, 1), **kw)
    assert set(q) == (set(plain) - {"sq_err", "mse", "nll", "loss_nll"}) | {"rgb_q", "depth_q"}
    assert bool((q["depth_q"][..., 0] <= q["depth_q"][..., 1]).all()) and bool((q["depth_q"][..., 1] <= q["depth_q"][..., 2]).all())
    assert torch.equal(q["depth_q"][..., 2], maps["depth_map"].max(-1).values)


def test_render_uncertainty_scores_refusals():
    model = _model(3)
    with pytest.raises(ValueError, match="scores="):
        E.render_uncertainty(H_, W_, FOCAL_, POSE, model, stats="geometry", scores=(0.5,), **RKW)
    grid = E.OccupancyGrid.from_mask(torch.ones(2, 2, 2, dtype=torch.bool), (-4, -4, -4), (4, 4, 8))
    for occ in (grid, grid.sampler(bins=8)):
        with pytest.raises(ValueError, match="scores="):
            E.render_uncertainty(H_, W_, FOCAL_, POSE, model, occupancy=occ, scores=(0.5,), **RKW)
    with pytest.raises(ValueError):
        E.render_uncertainty(H_, W_, FOCAL_, POSE, model, scores=[0.1] * 17, **RKW)


@pytest.mark.parametrize("K", [3, 33])
def test_image_metrics_with_calibration(K):
    model = _model(K)
    tv = torch.linspace(0., 1., S_, device=DEV)
    gt, gtd = _targets(50 + K)
    kw = dict(RKW, t_vals=tv)
    base = E.image_metrics(H_, W_, FOCAL_, POSE, model, gt, gt_depth=gtd, **kw)
    assert set(base) == {"mse", "psnr", "loss_nll", "ause_rgb_rmse", "ause_rgb_mae", "ause_depth_rmse", "ause_depth_mae"}
    cal = E.image_metrics(H_, W_, FOCAL_, POSE, model, gt, gt_depth=gtd, calibration=True, **kw)
    new = {"crps_rgb", "auce_rgb", "coverage_rgb", "crps_depth", "auce_depth", "coverage_depth"}
    assert set(cal) == set(base) | new
    for k in base:
        assert cal[k] == base[k] or (np.isnan(cal[k]) and np.isnan(base[k])), k
    r = E.render_uncertainty(H_, W_, FOCAL_, POSE, model, gt=gt, gt_depth=gtd, stats="ext", scores=(0.5,), **kw)
    assert cal["crps_rgb"] == float(r["rgb_crps"].mean()) and cal["crps_depth"] == float(r["depth_crps"].mean())
    cr = E.calibration(r["rgb_rank"], K)
    assert cal["auce_rgb"] == cr["auce"] and cal["coverage_rgb"] == [float(v) for v in cr["coverage"]] and len(cal["coverage_rgb"]) == 9
    assert cal["crps_rgb"] >= 0 and 0 <= cal["auce_rgb"] <= 1
    no_depth = E.image_metrics(H_, W_, FOCAL_, POSE, model, gt, calibration=True, **kw)
    assert set(no_depth) == (set(base) - {"ause_depth_rmse", "ause_depth_mae"}) | {"crps_rgb", "auce_rgb", "coverage_rgb"}
