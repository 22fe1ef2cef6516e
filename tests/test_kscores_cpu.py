"""CPU: the ensemble scores (CFNERF_F_KSCORES) - everything that needs no GPU.

* the flag in the header (a hex literal) and in the Python mirror, the struct's member order and layout, 34 exports as before;
* every refusal of the contract names the flag and the member or argument, before anything touches a device;
* the yardstick itself (kscores_common, fp64): the gap form of B against the brute-force double sum, CRPS >= 0 and = |x - y| at K = 1, the
  ideal coverage, and - truth and samples drawn from ONE skewed distribution - every coverage within 4 binomial standard deviations of it,
  while an ensemble with its spread halved is far outside;
* ``evaluate.calibration`` on hand-written codes, -1 rows and groups included."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import kscores_common as KS
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["samples", "target", "sorted", "quantiles", "rank_code", "pit", "crps", "n_levels", "level_lo", "level_frac"]


def _header():
    with open(os.path.join(ROOT, "include", "cfnerf.h")) as f:
        return f.read()


# ---------------------------------------------------------------- flag, exports, struct
def test_flag_is_the_hex_literal_0x4000_in_the_header_and_in_the_mirror():
    hdr = _header()
    assert re.search(r"\bCFNERF_F_KSCORES\s*=\s*0x4000\b", hdr)
    assert not re.search(r"CFNERF_F_KSCORES\s*=\s*1\s*<<", hdr)
    assert L.F_KSCORES == 0x4000 == 1 << 14
    values = {m.group(1): (1 << int(m.group(3))) if m.group(3) else int(m.group(2), 16)
              for m in re.finditer(r"^\s+CFNERF_F_(\w+)\s*=\s*(?:(0x[0-9a-fA-F]+)|1\s*<<\s*(\d+))", hdr, re.M)}
    assert len(values) == 15 and values["TRAIN"] == 1 and values["RAY_REG"] == 0x2000
    assert [n for n, v in values.items() if v & 0x4000] == ["KSCORES"]


def test_the_declared_names_are_still_34_and_equal_the_mirrors():
    names = re.findall(r"^CFNERF_API\s+[\w\s\*]+?\b(cfnerf_\w+)\s*\(", _header(), re.M)
    assert len(names) == 34 and sorted(names) == sorted(L.EXPORTS)


def test_struct_has_the_headers_member_order_and_layout():
    body = re.search(r"typedef struct cfnerf_kscores \{(.*?)\} cfnerf_kscores;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", body) == MEMBERS == [f[0] for f in L.KScores._fields_]
    assert re.search(r"level_lo\[16\]", body) and re.search(r"level_frac\[16\]", body)
    P = C.sizeof(C.c_void_p)
    assert L.KScores.n_levels.offset == 7 * P and L.KScores.level_lo.offset == 7 * P + 4 and L.KScores.level_frac.offset == 7 * P + 68
    assert C.sizeof(L.KScores) == (7 * P + 132 + P - 1) // P * P


def test_quantile_levels_are_floor_and_fraction_of_q_times_k_minus_1():
    assert L.quantile_levels(KS.LEVELS, 33) == [(0, 0.0), (1, float(np.float32(0.6))), (8, 0.0), (16, 0.0), (24, 0.0), (30, float(np.float32(0.4))), (32, 0.0)]
    assert L.quantile_levels((0, 0.5, 1), 1) == [(0, 0.0)] * 3
    assert L.quantile_levels((0.5,), 4) == [(1, 0.5)]
    for K in (2, 3, 5, 31, 64, 127, 128):
        for q, (lo, fr) in zip(KS.LEVELS, L.quantile_levels(KS.LEVELS, K)):
            assert 0 <= lo <= K - 1 and 0.0 <= fr < 1.0 and abs(lo + fr - q * (K - 1)) <= 2.0 ** -24
    with pytest.raises(ValueError):
        L.quantile_levels((1.5,), 4)


# ---------------------------------------------------------------- refusals, before anything touches a device
FAKE = 0x1000          # a non-NULL "device pointer": every call below is refused before anything could read it


def _call(white=None, N=4, S=1, K=4, ks="ok", raw=None, z=None, rays_d=None, rgb=None, disp=None, depth=None, levels=((1, 0.5),), **members):
    lib = L.lib()
    m = dict(samples=FAKE, target=FAKE, sorted=FAKE, quantiles=FAKE, rank_code=FAKE, pit=FAKE, crps=FAKE, n_levels=len(levels))
    m.update(members)
    st = L.KScores(*(m[k] for k in MEMBERS[:8]))
    for t, (lo, fr) in enumerate(levels[:16]):
        st.level_lo[t], st.level_frac[t] = lo, fr
    arg = None if ks is None else L.struct_arg(st)
    rc = lib.cfnerf_composite_fwd(raw, z, rays_d, N, S, K, L.F_KSCORES if white is None else white, rgb, disp, depth, arg, None)
    return rc, lib.cfnerf_last_error().decode()


def test_a_null_struct_is_refused_by_name():
    rc, msg = _call(ks=None)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and "cfnerf_kscores" in msg


def test_null_samples_are_refused_by_name():
    rc, msg = _call(samples=None)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and re.search(r"\bsamples\b", msg), msg


def test_no_output_requested_is_refused():
    rc, msg = _call(sorted=None, quantiles=None, rank_code=None, pit=None, crps=None)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and "no output" in msg, msg


@pytest.mark.parametrize("member", ["crps", "pit", "rank_code"])
def test_a_score_without_target_is_refused_by_name(member):
    others = {m: None for m in ("crps", "pit", "rank_code") if m != member}
    rc, msg = _call(target=None, **others)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and re.search(r"\b%s\b" % member, msg) and re.search(r"\btarget\b", msg), msg


@pytest.mark.parametrize("n", [0, 17, -1])
def test_quantiles_with_a_bad_n_levels_are_refused_by_name(n):
    rc, msg = _call(n_levels=n)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and "n_levels" in msg, msg


@pytest.mark.parametrize("level, what", [((-1, 0.0), "level_lo"), ((4, 0.0), "level_lo"), ((1, 1.0), "level_frac"), ((1, -0.25), "level_frac"),
                                         ((1, float("nan")), "level_frac")])
def test_a_level_out_of_range_is_refused_by_name(level, what):
    rc, msg = _call(levels=((0, 0.0), level))
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and what + "[1]" in msg, msg


def test_levels_are_not_read_without_quantiles():
    """(the call then gets as far as the launch check of an N = 0 launch: accepted, nothing runs)"""
    rc, msg = _call(N=0, quantiles=None, n_levels=99)
    assert rc == 0, msg


@pytest.mark.parametrize("arg", ["raw", "z", "rays_d", "rgb", "disp", "depth"])
def test_a_forbidden_argument_is_refused_by_name(arg):
    rc, msg = _call(**{arg: FAKE})
    name = {"z": "z_vals", "rgb": "rgb_map", "disp": "disp_map", "depth": "depth_map"}.get(arg, arg)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and re.search(r"\b%s\b" % name, msg), msg


@pytest.mark.parametrize("kw, what", [(dict(S=2), "S"), (dict(S=0), "S"), (dict(K=0), "K"), (dict(K=129), "K"), (dict(N=-1), "N")])
def test_bad_sizes_are_refused_by_name(kw, what):
    rc, msg = _call(**kw)
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and re.search(r"\b%s\b" % what, msg), msg


@pytest.mark.parametrize("other", ["F_CULL", "F_RAY_REG"])
def test_the_bit_together_with_another_mode_is_refused(other):
    rc, msg = _call(white=L.F_KSCORES | getattr(L, other))
    assert rc < 0 and "CFNERF_F_KSCORES" in msg and "CFNERF_" + other in msg, msg


def test_every_other_entry_point_that_takes_flags_refuses_the_bit_by_name():
    lib = L.lib()
    f = L.F_KSCORES
    calls = {
        "cfnerf_sample_points": lambda: lib.cfnerf_sample_points(None, None, None, f, 4, 8, None, None, None),
        "cfnerf_sample_pdf": lambda: lib.cfnerf_sample_pdf(None, None, None, f, None, None, 4, 8, 2, 4, None, None),
    }
    for who, call in calls.items():
        rc = call()
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0 and who in msg and "CFNERF_F_KSCORES" in msg, msg


# ---------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("K", [1, 2, 3, 5, 33, 128])
def test_the_gap_form_equals_the_brute_force_double_sum(K):
    x, y = KS.make_rows(40, K, seed=K, special=False)
    A, B = KS.crps_terms(x, y)
    brute = KS.crps_brute(x, y)
    assert np.abs((A - B) - brute).max() <= 1e-13 * np.abs(A + B).max()
    assert (B >= 0).all() and (A - B >= -1e-13 * (A + B)).all()
    if K == 1:
        assert np.array_equal(A - B, np.abs(x[:, 0].astype(np.float64) - y.astype(np.float64)))


def test_rank_code_and_pit_of_a_hand_written_row():
    x = np.array([[0.25, 0.5, 0.5, 1.0]], np.float32)
    for y, code in ((0.0, 0), (0.25, 1), (0.3, 2), (0.5, 4), (0.75, 6), (1.0, 7), (2.0, 8)):
        c = KS.rank_code(x, np.array([y], np.float32))
        assert int(c[0]) == code and float(KS.pit_of(c, 4)[0]) == code / 8


@pytest.mark.parametrize("K", [1, 2, 3, 8, 33])
def test_ideal_coverage_counts_the_ranks_inside(K):
    ideal = KS.ideal_coverage(K)
    _, mine = E._central_inside([j / 10 for j in range(1, 10)], K)
    assert np.array_equal(ideal, mine)
    assert (np.diff(ideal) >= 0).all() and ideal[-1] <= 1.0
    for j, v in zip(range(1, 10), ideal):                          # by hand: b is inside iff |b - K/2| <= j K / 20
        assert v == sum(1 for b in range(K + 1) if abs(20 * b - 10 * K) <= j * K) / (K + 1)
    # level 1 holds every rank, level 0 the middle one of an even K alone
    assert KS.ideal_coverage(K, [10])[0] == 1.0 and KS.ideal_coverage(K, [0])[0] == (1 / (K + 1) if K % 2 == 0 else 0.0)


@pytest.mark.parametrize("K", [8, 33])
def test_an_exchangeable_ensemble_is_calibrated_and_a_narrow_one_is_not(K):
    M = 200_000
    rng = np.random.default_rng(K)
    z = rng.gamma(2.0, 1.0, (M, K + 1)).astype(np.float32)        # skewed; truth and samples i.i.d.
    code = KS.rank_code(z[:, 1:], z[:, 0])
    cov, ideal = KS.coverage_of(code, K), KS.ideal_coverage(K)
    band = 4 * np.sqrt(ideal * (1 - ideal) / M)
    assert (np.abs(cov - ideal) <= band).all(), (cov, ideal, band)
    got = E.calibration(torch.from_numpy(code), K)
    assert np.array_equal(got["coverage"], cov) and np.array_equal(got["ideal"], ideal) and got["n"] == M and got["n_invalid"] == 0
    assert got["auce"] == pytest.approx(np.abs(cov - ideal).mean(), abs=1e-15) and got["auce"] <= band.mean()
    assert int(got["pit_hist"].sum()) == M and np.array_equal(got["pit_hist"], np.bincount(code, minlength=2 * K + 1))
    # a Gaussian ensemble with its spread halved: over-confident, far outside that band
    g = rng.standard_normal((M, K + 1)).astype(np.float32)
    g[:, 1:] *= 0.5
    narrow = E.calibration(torch.from_numpy(KS.rank_code(g[:, 1:], g[:, 0])), K)
    assert narrow["auce"] > 0.1 > 20 * band.max()
    assert (narrow["coverage"] < narrow["ideal"]).all()


# ---------------------------------------------------------------- evaluate.calibration
def test_calibration_on_hand_written_codes():
    K = 2                                                           # codes 0..4; inside level j/10 iff 10 |c - 2| <= 2 j: c = 2 always, c = 1, 3 from j = 5
    code = torch.tensor([[0, 1, 2], [3, 4, -1], [2, 2, -1]], dtype=torch.int32)
    c = E.calibration(code, K)
    assert c["n"] == 7 and c["n_invalid"] == 2 and c["pit_hist"].tolist() == [1, 1, 3, 1, 1]
    assert c["coverage"].tolist() == [3 / 7] * 4 + [5 / 7] * 5
    assert c["ideal"].tolist() == [1 / 3] * 9                      # #below = 1 of 0..2 (code 2) is inside below level 1; codes 1, 3 are no value of 2 #below
    assert c["auce"] == pytest.approx((4 * (3 / 7 - 1 / 3) + 5 * (5 / 7 - 1 / 3)) / 9)
    one = E.calibration(code, K, levels=(1.0, 0.0))
    assert one["coverage"].tolist() == [1.0, 3 / 7] and one["ideal"].tolist() == [1.0, 1 / 3]


def test_calibration_with_groups_is_calibration_of_each_group():
    rng = np.random.default_rng(5)
    K = 5
    code = torch.from_numpy(rng.integers(-1, 2 * K + 1, (50, 3)).astype(np.int32))
    group = torch.arange(3).expand(50, 3)
    both = E.calibration(code, K, group=group)
    fixed = E.calibration(code, K, group=group, n_groups=3)
    for ch in range(3):
        one = E.calibration(code[:, ch], K)
        for k in ("pit_hist", "coverage", "ideal"):
            assert np.array_equal(both[k][ch], one[k]) and np.array_equal(fixed[k][ch], one[k]), k
        assert both["auce"][ch] == one["auce"] and both["n"][ch] == one["n"] and both["n_invalid"][ch] == one["n_invalid"]


def test_calibration_without_a_valid_row_is_nan_and_bad_codes_raise():
    c = E.calibration(torch.tensor([-1, -1]), 3)
    assert c["n"] == 0 and c["n_invalid"] == 2 and np.isnan(c["auce"]) and np.isnan(c["coverage"]).all()
    with pytest.raises(ValueError):
        E.calibration(torch.tensor([7]), 3)
    with pytest.raises((ValueError, RuntimeError)):
        E.calibration(torch.tensor([-2]), 3)


def test_scores_are_refused_where_they_are_not_supported():
    eye = torch.eye(4)[:3]
    with pytest.raises(ValueError, match="scores="):
        E.render_uncertainty(4, 4, 1.0, eye, None, stats="geometry", scores=(0.5,))
    with pytest.raises(ValueError, match="scores="):
        E.render_uncertainty(4, 4, 1.0, eye, None, occupancy=object(), scores=(0.5,))
    with pytest.raises(ValueError, match="gt_depth"):
        E.render_uncertainty(4, 4, 1.0, eye, None, gt_depth=torch.zeros(4, 4))
