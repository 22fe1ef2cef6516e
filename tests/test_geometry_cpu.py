"""CPU: the geometry-only forward (CFNERF_F_GEOMETRY) - everything that needs no GPU.

* the flag's bit in the header and in the Python mirror;
* the stateless entry points refuse the flag by name before anything touches a device;
* tools/kernel_regs.py of the built library: 32 ``geom_fwd_kernel`` instantiations without a VGPR spill or scratch, and every kernel of
  profiles/r08_kernel_regs.txt (and of the committed profiles/r09_kernel_regs.txt) with the figures recorded there;
* ``render_uncertainty`` refuses an unknown ``stats``; ``NeRF_Flows.sample`` raises under grad mode;
* ``evaluate.sigma_stats``, the reduction of ``density_grid``, against numpy."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(\S.*?)\s+vgpr=\s*(\d+) agpr=\s*(\d+) vgpr_spill=\s*(\d+) sgpr=\s*(\d+) sgpr_spill=\s*(\d+) scratch=\s*(\d+) lds=\s*(\d+)\s*$")


def _table(text):
    """{kernel name: (vgpr, agpr, vgpr_spill, sgpr, sgpr_spill, scratch, lds)} of the kernel lines of a tools/kernel_regs.py listing"""
    out = {}
    for l in text.splitlines():
        m = LINE.match(l)
        if m:
            assert m.group(1) not in out, l
            out[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return out


@pytest.fixture(scope="module")
def built():
    return _table(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], capture_output=True, text=True, check=True).stdout)


def test_header_and_python_mirror_agree_on_bit_6():
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"CFNERF_F_(\w+)\s*=\s*1\s*<<\s*(\d+)", hdr)}
    assert flags["GEOMETRY"] == 6 and L.F_GEOMETRY == 1 << 6
    assert sorted(flags.values()) == list(range(7))                                        # seven public flags, one bit each


def test_stateless_entry_points_refuse_the_flag_by_name():
    lib = L.lib()
    rc = lib.cfnerf_sample_points(None, None, None, L.F_GEOMETRY, 4, 8, None, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "cfnerf_sample_points" in msg and "CFNERF_F_GEOMETRY" in msg
    rc = lib.cfnerf_sample_pdf(None, None, None, L.F_GEOMETRY, None, None, 4, 8, 2, 4, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "cfnerf_sample_pdf" in msg and "CFNERF_F_GEOMETRY" in msg
    rc = lib.cfnerf_sample_points(None, None, None, L.F_GEOMETRY | L.F_KSTATS_EXT, 4, 8, None, None, None)
    assert rc < 0 and "cfnerf_sample_points" in lib.cfnerf_last_error().decode()


def test_the_library_carries_32_geometry_kernels_without_spill_or_scratch(built):
    geom = {k: v for k, v in built.items() if k.startswith("geom_fwd_kernel<")}
    assert len(geom) == 32, sorted(geom)
    assert {k for k in geom} == {f"geom_fwd_kernel<{w}, {m}, {p}>" for w in range(64, 513, 64) for m in (0, 1) for p in (0, 1)}
    for k, (vgpr, agpr, vspill, sgpr, sspill, scratch, lds) in geom.items():
        assert vspill == 0 and scratch == 0, (k, vspill, scratch)


@pytest.mark.parametrize("committed", ["r08_kernel_regs.txt", "r09_kernel_regs.txt"])
def test_every_recorded_kernel_keeps_its_registers(built, committed):
    text = open(os.path.join(ROOT, "profiles", committed)).read()
    rec = _table(text)
    assert len(rec) >= 32
    for k, v in rec.items():
        # (r08 prints the kernels of ITS parent under that parent's names: fused_fwd_kernel had six template arguments then, EXT = false today)
        if re.fullmatch(r"fused_fwd_kernel<[^,>]+(, [^,>]+){5}>", k):
            k = k[:-1] + ", false>"
        assert k in built, k
        assert built[k] == v, (k, v, built[k])
    assert "(none)" in text.split("## changed")[1].split("## new")[0]


def test_r09_records_every_kernel_of_the_parent_and_the_new_ones(built):
    """the r09 table holds the 202 kernels of the parent commit (its `## unchanged` section) and the 32 new ones, all of them in the library
    (which may have gained others since)"""
    text = open(os.path.join(ROOT, "profiles", "r09_kernel_regs.txt")).read()
    new = _table(text.split("## new")[1].split("## unchanged")[0])
    old = _table(text.split("## unchanged")[1])
    assert len(new) == 32 and all(k.startswith("geom_fwd_kernel<") for k in new)
    assert len(old) == 202 and not any(k.startswith("geom_fwd_kernel<") for k in old)
    assert set(new) | set(old) <= set(built)


def test_render_uncertainty_refuses_an_unknown_stats_mode_and_lists_the_three():
    with pytest.raises(ValueError, match="'basic', 'ext' or 'geometry'"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="depth")
    with pytest.raises(ValueError, match="geometry"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="geometry", want_maps=True)


def test_sample_raises_under_grad_mode_and_names_forward():
    class Stub:                                                   # (what sample() looks at before anything touches a device)
        flat = torch.nn.Parameter(torch.zeros(3))
    assert hasattr(A.NeRF_Flows, "sample")
    with torch.enable_grad(), pytest.raises(RuntimeError, match=r"forward\(\)"):
        A.NeRF_Flows.sample(Stub(), torch.zeros(2, 90))


@pytest.mark.parametrize("K", [2, 4, 32, 128])
def test_sigma_stats_against_numpy(K):
    """sigma = softplus(alpha_k) (RUN:424), mean and np.std * n/(n-1) over K (RUN:1130).  fp32 against numpy fp64 on the same alpha: the
    bounds tests/test_hip_evaluate.py uses for rgb_mean / rgb_unc; in fp64 to rounding."""
    rng = np.random.default_rng(K)
    a = rng.standard_normal((5, 7, K)) * 3 + rng.uniform(-2, 2, (5, 7, 1))
    a[0, 0, 0] = 25.0                                             # past torch's softplus threshold
    sigma = np.where(a > 20, a, np.log1p(np.exp(np.minimum(a, 20))))
    m64, u64 = E.sigma_stats(torch.tensor(a))
    np.testing.assert_allclose(m64.numpy(), sigma.mean(-1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(u64.numpy(), np.std(sigma, -1) * K / (K - 1), rtol=1e-10, atol=0)
    a32 = torch.tensor(a, dtype=torch.float32)
    s32 = a32.double().numpy()
    sigma = np.where(s32 > 20, s32, np.log1p(np.exp(np.minimum(s32, 20))))
    m, u = E.sigma_stats(a32)
    assert m.dtype == torch.float32 and list(m.shape) == [5, 7] == list(u.shape)
    np.testing.assert_allclose(m.double().numpy(), sigma.mean(-1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(u.double().numpy(), np.std(sigma, -1) * K / (K - 1), rtol=1e-4, atol=1e-6)
