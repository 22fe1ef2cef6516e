"""CPU: the ray regularisers (CFNERF_F_RAY_REG) - everything that needs no GPU.

* the yardstick itself: rayreg_common's fp64 closed forms (the Q/R arrangement) against fp64 autograd of the quadratic definition;
* the flag in the header (a hex literal) and in the Python mirror, the struct's member order and layout, 34 exports as before;
* every refusal of the contract names the flag and the member or argument, before anything touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

import rayreg_common as R
from cfnerf_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["weights", "rays", "lambda_dist", "lambda_ent", "acc_min", "n_total", "d_weights", "d_z_opt", "scalars_out"]


def _header():
    with open(os.path.join(ROOT, "include", "cfnerf.h")) as f:
        return f.read()


# ---------------------------------------------------------------- the yardstick
def _inputs(S):
    """five rays: composited weights with a tie z_3 = z_2 (where S allows), ray 1 at A ~ 1e-3 (masked), ray 2 all zero"""
    w, z = R.composite_weights(5, S, 3, seed=S, tie=2)
    w[1] *= 1e-3
    w[2] = 0
    return w, z


@pytest.mark.parametrize("rays", [None, (2., 6.)], ids=["s=z", "near-far"])
@pytest.mark.parametrize("S", [1, 2, 130])
def test_closed_forms_equal_autograd_of_the_quadratic_definition(S, rays):
    """1e-12 of the largest entry per tensor.  The entropy's gradient (g_i - sum_j p_j g_j) / (A + 1e-10) is a difference of terms of size
    U = max |g| / (A + 1e-10): both sides carry its fp64 rounding, a few 2^-53 U, whatever the size of the result - at S = 1 the exact
    gradient is ~1e-10 U (p = 1 - 1e-10: only the 1e-10 guards keep it from 0), so that floor is all there is to compare."""
    lam_d, lam_e, acc_min, n_total = 0.7, 0.3, 0.1, 15
    w, z = _inputs(S)
    assert R.mask_margin(w, acc_min) > 1e-3
    A = w.sum(1)
    assert bool((A[1] < acc_min).all()) and bool((A[2] == 0).all()) and bool((A[0] > acc_min).all())
    if S > 3:
        assert bool((z[:, 3] == z[:, 2]).all())
    w.requires_grad_()
    z.requires_grad_()
    reg, dist, ent, frac = R.quadratic(w, z, rays, lam_d, lam_e, acc_min, n_total)
    gw, gz = torch.autograd.grad(reg, [w, z], allow_unused=True)
    gz = torch.zeros_like(z) if gz is None else gz
    c = R.closed_forms(w.detach(), z.detach(), rays, lam_d, lam_e, acc_min, n_total)
    ref = torch.stack([reg, dist, ent, frac]).detach()
    assert (c["scalars"] - ref).abs().max() <= 1e-12 * ref.abs().max()
    p = (w / (A[:, None] + 1e-10)).detach()
    on = (A > acc_min)[:, None].expand_as(p)
    U = (lam_e / (n_total * 3) * (torch.log(p + 1e-10).abs() + 1) / (A[:, None] + 1e-10))[on].max().item()
    assert (c["d_weights"] - gw).abs().max() <= 1e-12 * gw.abs().max() + 8 * 2.0 ** -53 * U
    assert (c["d_z"] - gz).abs().max() <= 1e-12 * gz.abs().max()
    assert float(frac) == pytest.approx(3 * 3 / (15 * 3))                  # rays 0, 3, 4 (x K = 3) over n_total = 15 rays


def test_the_entropy_part_is_the_snippet_of_the_integration_guide():
    """INTEGRATION.md section 12 (c), verbatim, on rays that are all above acc_min"""
    w, _ = R.composite_weights(4, 33, 2, seed=7)
    snippet = re.search(r"p = w / \(w\.sum\(1, keepdim=True\) \+ 1e-10\)\n.*?\(-\(p \* torch\.log\(p \+ 1e-10\)\)\.sum\(1\)\)\.mean\(\)",
                        open(os.path.join(ROOT, "INTEGRATION.md")).read(), re.S)
    assert snippet is not None, "INTEGRATION.md section 12 (c) changed"
    p = w / (w.sum(1, keepdim=True) + 1e-10)
    want = (-(p * torch.log(p + 1e-10)).sum(1)).mean()
    assert torch.equal(R.entropy_12c(w), -(p * torch.log(p + 1e-10)).sum(1))
    z = torch.zeros(4, 33, dtype=torch.float64)
    assert torch.equal(R.quadratic(w, z, None, 0., 1., 0.0)[2], want)
    assert torch.equal(R.closed_forms(w, z, None, 0., 1., 0.0)["scalars"][2], want)


# ---------------------------------------------------------------- flag, exports, struct
def test_flag_is_the_hex_literal_0x2000_in_the_header_and_in_the_mirror():
    hdr = _header()
    assert re.search(r"\bCFNERF_F_RAY_REG\s*=\s*0x2000\b", hdr)
    assert not re.search(r"CFNERF_F_RAY_REG\s*=\s*1\s*<<", hdr)
    assert L.F_RAY_REG == 0x2000 == 1 << 13
    values = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"\bCFNERF_F_(\w+)\s*=\s*(0x[0-9a-fA-F]+)", hdr)}
    assert [n for n, v in values.items() if v & 0x2000] == ["RAY_REG"]


def test_the_declared_names_are_still_34_and_equal_the_mirrors():
    names = re.findall(r"^CFNERF_API\s+[\w\s\*]+?\b(cfnerf_\w+)\s*\(", _header(), re.M)
    assert len(names) == 34 and sorted(names) == sorted(L.EXPORTS)


def test_struct_has_the_headers_member_order_and_layout():
    body = re.search(r"typedef struct cfnerf_ray_reg \{(.*?)\} cfnerf_ray_reg;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == MEMBERS == [f[0] for f in L.RayReg._fields_]
    P = C.sizeof(C.c_void_p)
    assert L.RayReg.lambda_dist.offset == 2 * P and L.RayReg.n_total.offset == 2 * P + 16 and L.RayReg.d_weights.offset == 2 * P + 24
    assert C.sizeof(L.RayReg) == 5 * P + 24


# ---------------------------------------------------------------- refusals, before anything touches a device
FAKE = 0x1000          # a non-NULL "device pointer": every call below is refused before anything could read it


def _call(white=None, raw=None, z=FAKE, rays_d=None, N=4, S=8, K=2, rgb=None, disp=None, depth=None, rr="ok", **members):
    lib = L.lib()
    m = dict(weights=FAKE, rays=None, lambda_dist=1.0, lambda_ent=1.0, acc_min=0.1, n_total=0, d_weights=FAKE, d_z_opt=None, scalars_out=FAKE)
    m.update(members)
    st = L.RayReg(*(m[k] for k in MEMBERS))
    arg = None if rr is None else L.struct_arg(st)
    rc = lib.cfnerf_composite_fwd(raw, z, rays_d, N, S, K, L.F_RAY_REG if white is None else white, rgb, disp, depth, arg, None)
    return rc, lib.cfnerf_last_error().decode()


def test_a_null_struct_is_refused_by_name():
    rc, msg = _call(rr=None)
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and "cfnerf_ray_reg" in msg


@pytest.mark.parametrize("member", ["weights", "d_weights", "scalars_out"])
def test_a_null_member_is_refused_by_name(member):
    rc, msg = _call(**{member: None})
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and re.search(r"\b%s\b" % member, msg), msg


def test_a_null_z_vals_is_refused_by_name():
    rc, msg = _call(z=None)
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and "z_vals" in msg


@pytest.mark.parametrize("arg", ["raw", "rays_d", "rgb", "disp", "depth"])
def test_a_forbidden_argument_is_refused_by_name(arg):
    rc, msg = _call(**{arg: FAKE})
    name = {"rgb": "rgb_map", "disp": "disp_map", "depth": "depth_map"}.get(arg, arg)
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and re.search(r"\b%s\b" % name, msg), msg


def test_the_bit_together_with_cull_is_refused():
    rc, msg = _call(white=L.F_RAY_REG | L.F_CULL)
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and "CFNERF_F_CULL" in msg


@pytest.mark.parametrize("kw, what", [(dict(S=0), "S"), (dict(K=0), "K"), (dict(N=-1), "N")])
def test_bad_sizes_are_refused_by_name(kw, what):
    rc, msg = _call(**kw)
    assert rc < 0 and "CFNERF_F_RAY_REG" in msg and re.search(r"\b%s\b" % what, msg), msg


def test_every_other_entry_point_that_takes_flags_refuses_the_bit_by_name():
    lib = L.lib()
    f = L.F_RAY_REG
    calls = {
        "cfnerf_sample_points": lambda: lib.cfnerf_sample_points(None, None, None, f, 4, 8, None, None, None),
        "cfnerf_sample_pdf": lambda: lib.cfnerf_sample_pdf(None, None, None, f, None, None, 4, 8, 2, 4, None, None),
    }
    for who, call in calls.items():
        rc = call()
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0 and who in msg and "CFNERF_F_RAY_REG" in msg, msg
