"""CFNERF_F_SEAM_GRAD on the CPU: the closed form the unfused seam's sampling node differentiates (api.sample_points_reference) against the
oracle's sampling lines, a torch restatement of comp_seam_zgrad_kernel's formula with all four cotangents against fp64 autograd of the
oracle's raw2outputs in z_vals and rays_d, and the boundary: the header's flag and struct, the refusals by name.  No kernel runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import api
from oracle import cfnerf_oracle as O

import raygrad_common as RG
import seamgrad_common as SG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the sampling lines (RUN:510-534)
@pytest.mark.parametrize("lindisp", [False, True], ids=["lin", "lindisp"])
@pytest.mark.parametrize("jitter", [False, True], ids=["t_rand-None", "t_rand"])
def test_sample_points_reference_equals_the_oracles_sampling_in_value_and_gradient(lindisp, jitter):
    N, S = 5, 33
    rng = np.random.default_rng(31)
    rb = RG.random_rays(rng, N, dtype=torch.float64)
    rb[:, 6] = torch.tensor(rng.uniform(0.5, 2.0, N))          # per-ray near / far
    rb[:, 7] = torch.tensor(rng.uniform(4.0, 7.0, N))
    tv = torch.sort(torch.tensor(rng.uniform(0, 1, S))).values
    tr = torch.tensor(rng.uniform(0, 1, (N, S))) if jitter else None
    Gz, Gp = torch.tensor(rng.standard_normal((N, S))), torch.tensor(rng.standard_normal((N, S, 3)))
    a, b = rb.clone().requires_grad_(True), rb.clone().requires_grad_(True)
    z, pts = api.sample_points_reference(a, tv, tr, lindisp)
    z_o = O.sample_z(b[:, 6:7], b[:, 7:8], tv, lindisp, tr)
    pts_o = b[:, None, 0:3] + b[:, None, 3:6] * z_o[..., None]
    assert z.dtype == torch.float64 and tuple(z.shape) == (N, S) and tuple(pts.shape) == (N, S, 3)
    np.testing.assert_allclose(z.detach().numpy(), z_o.detach().numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(pts.detach().numpy(), pts_o.detach().numpy(), rtol=1e-14, atol=1e-14)
    ((z * Gz).sum() + (pts * Gp).sum()).backward()
    ((z_o * Gz).sum() + (pts_o * Gp).sum()).backward()
    assert tuple(a.grad.shape) == (N, 11)
    assert float(b.grad[:, 0:8].abs().min()) > 0, "every one of origin, direction, near and far must be on the oracle's graph"
    assert float(a.grad[:, 8:11].abs().max()) == 0 and float(b.grad[:, 8:11].abs().max()) == 0      # the view directions are not sampled
    np.testing.assert_allclose(a.grad.numpy(), b.grad.numpy(), rtol=1e-12, atol=1e-12 * float(b.grad.abs().max()))


def test_sample_points_reference_keeps_the_dtype_and_takes_an_fp32_table():
    rb = RG.random_rays(np.random.default_rng(32), 3)
    z, pts = api.sample_points_reference(rb, O.t_vals_table(torch.float64))
    assert z.dtype == torch.float32 and pts.dtype == torch.float32 and tuple(z.shape) == (3, 128)
    assert torch.equal(z, O.sample_z(rb[:, 6:7], rb[:, 7:8], O.t_vals_table(), False, None))


# ---------------------------------------------------------------- 2. the kernel's formula against fp64 autograd of raw2outputs
@pytest.mark.parametrize("i", range(len(SG.CASES)), ids=SG.IDS)
def test_formula_mirror_in_fp64_equals_autograd_of_raw2outputs_in_z_and_rays_d(i):
    """every kernel case (white_bkgd, S = 2 and a cotangent on disp_map alone among them) in fp64: 1e-9 of the largest entry - the
    recurrence for D and the suffix form of torch's cumprod backward are the same number in exact arithmetic, not in fp64"""
    inp = {k: (v.double() if torch.is_tensor(v) else v) for k, v in SG.inputs(i).items()}
    z64, d64 = SG.oracle_grads(inp)
    dz, dd = SG.seam_zgrad_mirror(inp["raw"], inp["z"], inp["rays_d"], inp["G"], inp["Gq"], inp["Gd"], inp["Gw"], inp["wb"])
    assert float(z64.abs().max()) > 0 and float(d64.abs().max()) > 0
    assert SG.rel(dz, z64) < 1e-9 and SG.rel(dd, d64) < 1e-9, (SG.rel(dz, z64), SG.rel(dd, d64))


def test_formula_mirror_without_the_new_cotangents_is_the_fused_paths_mirror():
    inp = SG.inputs(2)
    a = SG.seam_zgrad_mirror(inp["raw"].double(), inp["z"].double(), inp["rays_d"].double(), inp["G"].double(), None, inp["Gd"].double(), None, True)
    b = RG.comp_zgrad_mirror(inp["raw"].double(), inp["z"].double(), inp["rays_d"].double(), inp["G"].double(), inp["Gd"].double(), True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_case_table_covers_what_the_kernel_can_get_wrong():
    shapes = {(s, k) for _, s, k, _, _ in SG.CASES}
    assert {2, 64, 65, 130} <= {s for s, _ in shapes} and {3, 5, 12, 16} <= {k for _, k in shapes} and (64, 128) in shapes
    assert {1, 5} <= {n for n, *_ in SG.CASES}
    uses = {u for _, _, _, u, _ in SG.CASES}
    assert {("Gq",), ("Gd",), ("Gw",)} <= uses and any("Gd" not in u and len(u) > 1 for u in uses) and any(wb for *_, wb in SG.CASES)
    for i in range(len(SG.CASES)):
        d = SG.inputs(i)["rays_d"]
        assert float(((d * d).sum(-1).sqrt() - 1).abs().min()) > 1e-3          # non-unit directions: |rays_d| matters


# ---------------------------------------------------------------- 3. the boundary
def test_header_flag_struct_and_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    assert re.search(r"\bCFNERF_F_SEAM_GRAD\s*=\s*0x400\b", hdr) and L.F_SEAM_GRAD == 0x400
    m = re.search(r"typedef struct cfnerf_composite_grads \{(.*?)\} cfnerf_composite_grads;", hdr, flags=re.S)
    assert m, "cfnerf_composite_grads is not declared"
    members = re.findall(r"float\*\s*(\w+);", m.group(1))
    assert members == ["d_raw", "d_z_vals", "d_rays_d"] == [f[0] for f in L.CompositeGrads._fields_]
    assert C.sizeof(L.CompositeGrads) == 3 * C.sizeof(C.c_void_p)
    g = L.composite_grads()
    assert g.d_raw is None and g.d_z_vals is None and g.d_rays_d is None
    assert not (L.F_SEAM_GRAD & (L.F_TRAIN | L.F_LINDISP | L.F_WHITE_BKGD | L.F_STASH | L.F_EPS_ROWS | L.F_KSTATS_EXT | L.F_GEOMETRY | L.F_INPUT_GRAD
                                 | L.F_RAY_GRAD | L.F_COTANGENTS))


def test_no_new_symbol():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cfnerf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bCFNERF_API\b[^;(]*?\b(cfnerf_[a-z_0-9]+)\s*\(", hdr))
    assert len(declared) == 34 and declared == set(L.EXPORTS)


def test_flags_taking_entry_points_refuse_the_bit_by_name():
    lib = L.lib()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_sample_points(None, None, None, L.F_SEAM_GRAD, 4, 128, None, None, None)
    assert rc != 0 and "cfnerf_sample_points does not take CFNERF_F_SEAM_GRAD" in err(), err()
    rc = lib.cfnerf_sample_pdf(None, None, None, L.F_SEAM_GRAD | L.F_LINDISP, None, None, 4, 128, 4, 8, None, None)
    assert rc != 0 and "cfnerf_sample_pdf does not take CFNERF_F_SEAM_GRAD" in err(), err()
    # (the entry points that take a model check the handle first: tests/test_hip_seamgrad.py refuses the bit there)


def test_composite_bwd_with_the_bit_and_nothing_to_write_is_refused():
    lib = L.lib()
    err = lambda: lib.cfnerf_last_error().decode()
    out = L.composite_grads()
    for wb in (0, 1):
        rc = lib.cfnerf_composite_bwd(None, None, None, 4, 8, 4, wb | L.F_SEAM_GRAD, None, None, None, None, L.composite_grads_arg(out), None)
        assert rc != 0 and "CFNERF_F_SEAM_GRAD" in err() and "d_raw, d_z_vals and d_rays_d are all NULL" in err(), err()
    rc = lib.cfnerf_composite_bwd(None, None, None, 4, 8, 4, L.F_SEAM_GRAD, None, None, None, None, None, None)
    assert rc != 0 and "CFNERF_F_SEAM_GRAD" in err() and "cfnerf_composite_grads" in err(), err()
    # with something to write the call goes on to its ordinary argument checks (no launch here: raw is NULL)
    one = L.CompositeGrads(None, 64, None)
    rc = lib.cfnerf_composite_bwd(None, None, None, 4, 8, 4, L.F_SEAM_GRAD, None, None, None, None, L.composite_grads_arg(one), None)
    assert rc != 0 and "NULL argument" in err(), err()
