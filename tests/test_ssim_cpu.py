"""CPU: the image similarity (CFNERF_MODE_SSIM) - everything that needs no GPU.

* the mode bit in the header (a hex literal, an enum of its own) and in the Python mirror, the struct's member order and layout, the
  scratch macro against its mirror (compiled with the host compiler), 34 exports and 15 CFNERF_F_* enumerators as before;
* every refusal of the contract names the mode and the member or argument, before anything touches a device;
* ``ssim_window``: 7 equal taps, and the 11 Gaussian taps of scipy's own kernel;
* the yardstick itself (ssim_common, fp64) against the scipy.ndimage route that skimage takes, exactly 1 on identical images, the closed form
  on constant ones."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ssim_common as SC
from cfnerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["x", "y", "ssim_map", "mean", "scratch", "H", "W", "win", "cov_norm", "c1", "c2", "taps"]


def _header():
    with open(os.path.join(ROOT, "include", "cfnerf.h")) as f:
        return f.read()


# ---------------------------------------------------------------- mode bit, exports, struct, macro
def test_mode_is_the_hex_literal_0x8000_in_an_enum_of_its_own_and_in_the_mirror():
    hdr = _header()
    assert re.search(r"enum cfnerf_mode \{\s*CFNERF_MODE_SSIM\s*=\s*0x8000\s*\};", hdr)
    assert L.MODE_SSIM == 0x8000 == 1 << 15
    assert len(re.findall(r"^\s+CFNERF_F_\w+\s*=", hdr, re.M)) == 15
    values = {m.group(1): (1 << int(m.group(3))) if m.group(3) else int(m.group(2), 16)
              for m in re.finditer(r"^\s+CFNERF_F_(\w+)\s*=\s*(?:(0x[0-9a-fA-F]+)|1\s*<<\s*(\d+))", hdr, re.M)}
    assert len(values) == 15 and not [n for n, v in values.items() if v & 0x8000]
    assert not [n for n in dir(L) if n.startswith(("F_", "FLAG_")) and isinstance(getattr(L, n), int) and getattr(L, n) & 0x8000]


def test_the_declared_names_are_still_34_and_equal_the_mirrors():
    names = re.findall(r"^CFNERF_API\s+[\w\s\*]+?\b(cfnerf_\w+)\s*\(", _header(), re.M)
    assert len(names) == 34 and sorted(names) == sorted(L.EXPORTS)


def test_struct_has_the_headers_member_order_and_layout():
    body = re.search(r"typedef struct cfnerf_ssim \{(.*?)\} cfnerf_ssim;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", body) == MEMBERS == [f[0] for f in L.SSim._fields_]
    assert re.search(r"float\s+taps\[15\]", body) and len(re.findall(r"\bdouble\s+(?:cov_norm|c1|c2)\b", body)) == 3
    P = C.sizeof(C.c_void_p)
    assert L.SSim.H.offset == 5 * P and L.SSim.win.offset == 5 * P + 8
    assert L.SSim.cov_norm.offset == (5 * P + 12 + 7) // 8 * 8 and L.SSim.c2.offset == L.SSim.cov_norm.offset + 16
    assert L.SSim.taps.offset == L.SSim.cov_norm.offset + 24 and C.sizeof(L.SSim) == (L.SSim.taps.offset + 60 + 7) // 8 * 8


SHAPES_FOR_SCRATCH = [(1, 1, 7, 7, 7), (1, 3, 38, 39, 7), (1, 3, 39, 40, 7), (3, 3, 45, 70, 7), (2, 4, 45, 70, 11), (1, 4, 20, 20, 15), (5, 2, 12, 12, 3),
                      (1, 3, 800, 800, 11), (100000, 4, 4000, 4000, 3)]


def test_the_scratch_macro_equals_its_mirror(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no host C compiler: the macro of include/cfnerf.h cannot be checked against its mirror")
    lines = "".join('    printf("%%lld\\n", (long long)CFNERF_SSIM_SCRATCH_FLOATS(%d, %d, %d, %d, %d));\n' % s for s in SHAPES_FOR_SCRATCH)
    src = tmp_path / "scratch_floats.c"
    src.write_text('#include <stdio.h>\n#include "cfnerf.h"\nint main(void) {\n' + lines + "    return sizeof(cfnerf_ssim) == %d ? 0 : 1;\n}\n" % C.sizeof(L.SSim))
    exe = tmp_path / "scratch_floats"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, "sizeof(cfnerf_ssim) differs from the mirror's"
    assert [int(v) for v in r.stdout.split()] == [L.ssim_scratch_floats(*s) for s in SHAPES_FOR_SCRATCH]
    # two floats (one double) per 32 x 32 tile, image and channel
    assert L.ssim_scratch_floats(1, 3, 38, 39, 7) == 2 * 3 * 1 * 2 and L.ssim_scratch_floats(3, 3, 45, 70, 7) == 2 * 9 * 2 * 2


# ---------------------------------------------------------------- refusals, before anything touches a device
FAKE = 0x1000          # a non-NULL, 8-byte aligned "device pointer": every call below is refused before anything could read it


def _call(white=None, N=2, S=1, K=3, ss="ok", raw=None, z=None, rays_d=None, rgb=None, disp=None, depth=None, taps=None, **members):
    lib = L.lib()
    m = dict(x=FAKE, y=FAKE, ssim_map=FAKE, mean=FAKE, scratch=FAKE, H=20, W=24, win=7, cov_norm=49 / 48, c1=1e-4, c2=9e-4)
    m.update(members)
    st = L.SSim(*(m[k] for k in MEMBERS[:11]))
    for i, t in enumerate([1 / 7] * 15 if taps is None else taps):
        st.taps[i] = t
    arg = None if ss is None else L.struct_arg(st)
    rc = lib.cfnerf_composite_fwd(raw, z, rays_d, N, S, K, L.MODE_SSIM if white is None else white, rgb, disp, depth, arg, None)
    return rc, lib.cfnerf_last_error().decode()


def test_a_null_struct_is_refused_by_name():
    rc, msg = _call(ss=None)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and "cfnerf_ssim" in msg


@pytest.mark.parametrize("member", ["x", "y"])
def test_a_null_image_is_refused_by_name(member):
    rc, msg = _call(**{member: None})
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"member %s\b" % member, msg), msg


def test_no_output_requested_is_refused():
    rc, msg = _call(ssim_map=None, mean=None)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and "no output" in msg, msg


def test_mean_without_scratch_is_refused_by_name():
    rc, msg = _call(scratch=None)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\bmean\b", msg) and re.search(r"\bscratch\b", msg), msg
    rc, msg = _call(scratch=FAKE + 4)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\bscratch\b", msg) and "aligned" in msg, msg


def test_scratch_is_not_needed_without_mean():
    """(the call then gets as far as the launch of N = 0 images: accepted, nothing runs)"""
    rc, msg = _call(N=0, mean=None, scratch=None)
    assert rc == 0, msg
    rc, msg = _call(N=0)
    assert rc == 0, msg


@pytest.mark.parametrize("win", [6, 8, 1, 2, 17, 16, 0, -7])
def test_a_bad_win_is_refused_by_name(win):
    rc, msg = _call(win=win)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\bwin\b", msg), msg


@pytest.mark.parametrize("kw, what", [(dict(H=6), "H"), (dict(W=6), "W"), (dict(H=0), "H"), (dict(W=-3), "W"), (dict(H=10, win=11), "H")])
def test_an_image_smaller_than_the_window_is_refused_by_name(kw, what):
    rc, msg = _call(**kw)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"member %s\b" % what, msg), msg


@pytest.mark.parametrize("kw, what", [(dict(K=0), "K"), (dict(K=5), "K"), (dict(K=-1), "K"), (dict(S=2), "S"), (dict(S=0), "S"), (dict(N=-1), "N")])
def test_bad_sizes_are_refused_by_name(kw, what):
    rc, msg = _call(**kw)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\b%s\b" % what, msg), msg


@pytest.mark.parametrize("value", [0.0, -1e-4, float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("member", ["c1", "c2", "cov_norm"])
def test_a_constant_that_is_not_finite_and_positive_is_refused_by_name(member, value):
    rc, msg = _call(**{member: value})
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"member %s\b" % member, msg), msg


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_tap_that_is_not_finite_is_refused_by_name(value):
    taps = [1 / 7] * 15
    taps[6] = value
    rc, msg = _call(taps=taps)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and "taps[6]" in msg, msg
    taps[6], taps[7] = 1 / 7, value                       # behind the window: not read
    rc, msg = _call(N=0, taps=taps)
    assert rc == 0, msg
    rc, msg = _call(taps=[0.0] * 15)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\btaps\b", msg), msg


@pytest.mark.parametrize("arg", ["raw", "z", "rays_d", "rgb", "disp", "depth"])
def test_a_forbidden_argument_is_refused_by_name(arg):
    rc, msg = _call(**{arg: FAKE})
    name = {"z": "z_vals", "rgb": "rgb_map", "disp": "disp_map", "depth": "depth_map"}.get(arg, arg)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and re.search(r"\b%s\b" % name, msg), msg


@pytest.mark.parametrize("other", ["F_CULL", "F_RAY_REG", "F_KSCORES"])
def test_the_bit_together_with_another_mode_is_refused(other):
    rc, msg = _call(white=L.MODE_SSIM | getattr(L, other))
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and "CFNERF_" + other in msg, msg


def test_too_many_tiles_are_refused():
    rc, msg = _call(N=1 << 40, K=4)
    assert rc < 0 and "CFNERF_MODE_SSIM" in msg and "2^31" in msg, msg


def test_composite_bwd_does_not_take_the_bit():
    """there the background is white iff (white_bkgd & ~CFNERF_F_SEAM_GRAD) != 0, whatever other bits are set: an existing test pins a
    value with every other bit set (tests/test_hip_seamgrad.py), so the bit cannot be refused in the backward - it selects nothing there"""
    lib = L.lib()
    for wb in (1, L.MODE_SSIM, -1 & ~L.F_SEAM_GRAD):                # (N = 0: accepted, nothing runs)
        assert lib.cfnerf_composite_bwd(None, None, None, 0, 1, 1, wb, None, None, None, None, None, None) == 0, wb


def test_every_entry_point_that_takes_flags_refuses_the_bit_by_name():
    lib = L.lib()
    f = L.MODE_SSIM
    calls = {
        "cfnerf_sample_points": lambda: lib.cfnerf_sample_points(None, None, None, f, 4, 8, None, None, None),
        "cfnerf_sample_pdf": lambda: lib.cfnerf_sample_pdf(None, None, None, f, None, None, 4, 8, 2, 4, None, None),
    }
    for who, call in calls.items():
        rc = call()
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0 and who in msg and "CFNERF_MODE_SSIM" in msg, msg
    # the three that check their model handle first share the same refusal (refuse_mode_flags): it is in every one of them
    with open(os.path.join(ROOT, "cf-nerf_amd", "csrc", "cfnerf_abi.hip")) as fh:
        src = fh.read()
    users = set(re.findall(r'refuse_mode_flags\(flags, [^;]*?"(cfnerf_\w+)"\)', src))
    assert users == {"cfnerf_sample_points", "cfnerf_sample_pdf", "cfnerf_render_fwd", "cfnerf_render_eval", "cfnerf_network_fwd"}
    takes_flags = set(re.findall(r"^int (cfnerf_\w+)\([^)]*\bint flags\b", src, re.M))
    assert takes_flags == users


# ---------------------------------------------------------------- ssim_window
def test_the_uniform_window_is_7_equal_taps_with_the_sample_covariance():
    taps, cov = L.ssim_window("uniform")
    assert len(taps) == 7 and len(set(taps)) == 1 and taps[0] == float(np.float32(1 / 7)) and cov == 49 / 48
    taps, cov = L.ssim_window("uniform", 3)
    assert taps == [float(np.float32(1 / 3))] * 3 and cov == 9 / 8
    for bad in (4, 1, 17):
        with pytest.raises(ValueError):
            L.ssim_window("uniform", bad)
    with pytest.raises(ValueError):
        L.ssim_window("box")


def test_the_gaussian_window_is_scipys_kernel_rounded_once():
    taps, cov = L.ssim_window("gaussian")
    assert len(taps) == 11 and cov == 1.0 and taps == taps[::-1]
    assert all(t == float(np.float32(t)) for t in taps) and abs(sum(taps) - 1) < 11 * 2.0 ** -25
    assert np.array_equal(np.array(taps, np.float32), SC.gaussian_taps(11).astype(np.float32))
    filters = pytest.importorskip("scipy.ndimage._filters")
    assert np.array_equal(np.array(taps, np.float32), filters._gaussian_kernel1d(1.5, 0, 5).astype(np.float32))
    assert len(L.ssim_window("gaussian", sigma=0.8)[0]) == 2 * int(3.5 * 0.8 + 0.5) + 1 == 7
    assert len(L.ssim_window("gaussian", 5)[0]) == 5


# ---------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("name", ["uniform", "render", "bright_flat", "identical"])
@pytest.mark.parametrize("H, W, C_, win", [(45, 70, 3, 7), (45, 70, 3, 11)])
def test_the_yardstick_agrees_with_the_scipy_route_of_skimage(name, H, W, C_, win):
    ndi = pytest.importorskip("scipy.ndimage")
    x, y = (a.astype(np.float64) for a in SC.make_case(name, H, W, C_))
    (S, mean), _ = SC.reference(name, H, W, C_, win)
    p = (win - 1) // 2
    worst, means = 0.0, []
    for ch in range(C_):
        a, b = x[..., ch], y[..., ch]
        if win == 11:
            f, cov = (lambda im: ndi.gaussian_filter(im, sigma=1.5, truncate=3.5, mode="reflect")), 1.0
        else:
            f, cov = (lambda im: ndi.uniform_filter(im, size=win, mode="reflect")), win * win / (win * win - 1.0)
        ux, uy = f(a), f(b)
        vx, vy, vxy = cov * (f(a * a) - ux * ux), cov * (f(b * b) - uy * uy), cov * (f(a * b) - ux * uy)
        sk = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
        sk = sk[p:H - p, p:W - p]
        worst = max(worst, float(np.abs(sk - S[..., ch]).max()))
        means.append(sk.mean())
    assert worst <= 1e-11, worst
    assert abs(np.mean(means) - mean) <= 1e-11


@pytest.mark.parametrize("H, W, C_, win", SC.SHAPES)
def test_the_yardstick_gives_exactly_1_on_identical_images(H, W, C_, win):
    (S, mean), _ = SC.reference("identical", H, W, C_, win)
    assert S.shape == (H - win + 1, W - win + 1, C_) and (S == 1.0).all() and mean == 1.0


@pytest.mark.parametrize("H, W, C_, win", SC.SHAPES)
def test_the_yardstick_gives_the_luminance_term_on_constant_images(H, W, C_, win):
    (S, mean), _ = SC.reference("constant", H, W, C_, win)
    x, y = SC.make_case("constant", H, W, C_)
    mx, my = float(x[0, 0, 0]), float(y[0, 0, 0])              # (the fp32 values of 0.3 and 0.7)
    want = (2 * mx * my + 1e-4) / (mx * mx + my * my + 1e-4)
    assert np.abs(S - want).max() <= 1e-12 and abs(mean - want) <= 1e-12


def test_the_naive_fp32_form_loses_the_variance_of_a_bright_flat_image():
    """what the kernel is for: E[x^2] - mu^2 in fp32 cancels against C2 = 9e-4"""
    for H, W, C_, win in [(45, 70, 3, 7), (45, 70, 3, 11)]:
        (S, _), (N, _) = SC.reference("bright_flat", H, W, C_, win)
        assert SC.max_err(N, S) > 1e-4
        (S, _), (N, _) = SC.reference("uniform", H, W, C_, win)
        assert SC.max_err(N, S) < 4e-6


def test_one_nan_makes_nan_exactly_its_footprint_in_the_yardstick():
    H, W, C_, win = 45, 70, 3, 7
    (S, mean), _ = SC.reference("one_nan", H, W, C_, win)
    (clean, _), _ = SC.reference("render", H, W, C_, win)
    r, c, ch = SC.NAN_AT(H, W, C_)
    want = np.zeros(S.shape, bool)
    want[max(r - win + 1, 0):r + 1, max(c - win + 1, 0):c + 1, ch] = True
    assert np.array_equal(np.isnan(S), want) and np.isnan(mean) and np.array_equal(S[~want], clean[~want])
