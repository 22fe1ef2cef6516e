"""The latent gradient (CFNERF_F_EPS_GRAD) on the CPU: the G28 fixtures of the real reference, the oracle's autograd against them (so that the
fixtures mean what tests/test_hip_epsgrad.py assumes), the layout helper against the header's rule, the deterministic pairs -> rows adjoint,
and the register / scratch figures of the new kernels in the built code object.  No kernel runs."""
import glob
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import latents as LT

import epsgrad_common as EC
from util_hip import RTOL, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))


def test_epsgrad_fixtures_match_their_manifest():
    man = EC.manifest()
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(EC.GOLDEN, "*.npz")))
    assert names == sorted(man) == sorted(EC.NAMES)
    for name in names:
        g = EC.load(name)
        assert sorted(g) == sorted(man[name]), name
        for k, v in g.items():
            assert _digest(v) == man[name][k], (name, k)
        assert os.path.getsize(os.path.join(EC.GOLDEN, name + ".npz")) <= 64 * 1024


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="the reference only exists in the build container")
def test_committed_epsgrad_generator_reproduces_the_fixtures(tmp_path):
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_epsgrad.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(os.path.join(str(tmp_path), "MANIFEST.json")) as f:
        assert json.load(f) == EC.manifest()


def test_fixture_shapes():
    a, b, c = (EC.load(n) for n in EC.NAMES)
    assert a["ray_batch"].shape == (3, 11) and int(a["K"]) == 3 and a["eps_alpha_grad"].shape == (3, 1) and a["eps_rgb_grad"].shape == (3, 3)
    assert b["ray_batch"].shape == (4, 11) and int(b["netchunk"]) == 256 and b["eps_alpha"].shape == (2, 3, 1)
    assert b["eps_alpha_grad"].shape == (2, 3, 1) and b["eps_rgb_grad"].shape == (2, 3, 3)
    assert c["x"].shape == (5, 90) and int(c["K"]) == 4 and c["eps_alpha_grad"].shape == (4, 1) and c["eps_rgb_grad"].shape == (4, 3)
    for g in (a, b, c):
        assert int(g["netwidth"]) == 64 and int(g["netdepth"]) == 3 and float(g["min_abs_pre"]) > 0
        assert sorted(k[5:] for k in g if k.startswith("grad.")) == sorted(EC.BASE)
        for k in ("eps_alpha_grad", "eps_rgb_grad"):
            assert np.isfinite(g[k]).all() and float(np.abs(g[k]).max()) > 0, k


@pytest.mark.parametrize("name", EC.NAMES)
def test_oracle_autograd_reproduces_the_reference_latent_gradients(name):
    """the fp32 oracle differentiated in its latents: the reference's eps gradients (one set, both pairs of a two-netchunk batch, NeRF_Flows.forward)
    and the four base-Gaussian gradients, on the reference's masks, within G_TIGHT of each tensor's largest entry (both sides fp32)"""
    g = EC.load(name)
    grads, loss = EC.oracle_fixture(name, g)
    close(loss, g["loss"], what=f"{name} loss")
    for k, v in grads.items():
        scale = float(np.abs(g[k]).max())
        assert scale > 0, k
        close(v, g[k], atol=EC.G_TIGHT * scale, rtol=RTOL, what=f"{name} {k}")


# ---------------------------------------------------------------- the layout of cfnerf.h and its mirror
def _header():
    with open(os.path.join(ROOT, "include", "cfnerf.h")) as f:
        return f.read()


def test_flag_value_and_symbol_count():
    m = re.search(r"CFNERF_F_EPS_GRAD\s*=\s*(0x[0-9a-fA-F]+|\d+)\b", _header())
    assert m and int(m.group(1), 0) == 1 << 12 == L.FLAG_EPS_GRAD
    assert len(L.EXPORTS) == 34
    if os.path.exists(L.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert len([ln for ln in out.splitlines() if " T " in ln]) == 34


@pytest.mark.parametrize("K", [1, 3, 16, 17, 128])
@pytest.mark.parametrize("block", ["params", "ray_grad", "input_grad"])
def test_eps_grad_offsets_follow_the_headers_rule(block, K):
    """e_off = (base_end + 63) / 64 * 64, er_off = e_off + (4 K + 63) / 64 * 64, for every block the stash may already ask for"""
    n_params, N, S, P, C = 29058, 5, 70, 11, 90
    up = lambda v: (v + 63) // 64 * 64
    if block == "params":
        base_end, n = n_params, N
    elif block == "ray_grad":
        base_end, n = up(n_params) + up(N * 11) + N * S, N
        assert base_end == L.ray_grad_offsets(n_params, N, S)[2]
    else:
        base_end, n = up(n_params) + P * C, P
        assert base_end == L.input_grad_offset(n_params) + P * C
    e_off, er_off, total = L.eps_grad_offsets(base_end, n, K)
    assert e_off == up(base_end) and e_off % 64 == 0 and e_off >= base_end
    assert er_off == e_off + up(4 * K) and er_off % 64 == 0 and er_off >= e_off + 4 * K
    assert total == er_off + n * K * 4


# ---------------------------------------------------------------- pairs -> rows
@pytest.mark.parametrize("N,S,netchunk,chunk", [(4, 128, 256, None), (7, 64, 128, 4), (5, 1, 2, None), (3, 128, 1024, None)])
def test_pairs_to_rows_adjoint_equals_index_selects(N, S, netchunk, chunk):
    """the deterministic adjoint of netchunk_eps_rows (segment sums) against torch's own index_select backward on the CPU; the cotangent holds
    small integers, so both sums are exact and the comparison is bit for bit"""
    C = LT.netchunk_count(N, S, netchunk, chunk)
    gen = torch.Generator().manual_seed(N * 1000 + S)
    pairs = torch.randn(C, 3, 4, generator=gen)
    cot = torch.randint(-8, 9, (N, 3, 4), generator=gen).float()
    a = pairs.clone().requires_grad_(True)
    rows = LT.netchunk_eps_rows(a, N, S, netchunk, chunk)
    assert type(rows.grad_fn).__name__.startswith("_PairsToRows")
    (rows * cot).sum().backward()
    b = pairs.clone().requires_grad_(True)
    idx = LT.netchunk_row_index(N, S, netchunk, chunk)
    ref = b.index_select(0, idx)
    assert torch.equal(rows.detach(), ref.detach()) and torch.equal(rows.detach(), LT.netchunk_eps_rows(pairs, N, S, netchunk, chunk))
    (ref * cot).sum().backward()
    assert torch.equal(a.grad, b.grad)
    # pack is a cat: the gradient reaches eps_alpha / eps_rgb
    ea, er = torch.randn(C, 3, 1, requires_grad=True), torch.randn(C, 3, 3, requires_grad=True)
    (LT.netchunk_eps_rows(LT.pack(ea, er), N, S, netchunk, chunk) * cot).sum().backward()
    assert ea.grad is not None and er.grad is not None and torch.equal(torch.cat([er.grad, ea.grad], -1), a.grad)


# ---------------------------------------------------------------- the new kernels in the built code object
def test_new_kernels_use_no_scratch():
    """tail_eps_kernel, flows_eps_kernel and reduce_eps_kernel: no scratch and no vector spill to memory, like their siblings; the tail variant's
    LDS is tail_cot_kernel's without the merge rows (dead there: it writes no g_theta) + the 8 KB of its accumulators; tail_bwd_kernel,
    tail_cot_kernel and flows_bwd_kernel keep their own figures"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    rows = {}
    for name in ("tail_eps_kernel", "flows_eps_kernel", "reduce_eps_kernel", "tail_bwd_kernel", "tail_cot_kernel", "flows_bwd_kernel"):
        row = [ln for ln in out.splitlines() if name in ln]
        assert len(row) == 1, (name, out[-500:])
        rows[name] = {k: int(v) for k, v in re.findall(r"(\w+)=\s*(\d+)", row[0])}
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0, row[0]
    assert rows["tail_eps_kernel"]["lds"] == rows["tail_cot_kernel"]["lds"] - 3 * 84 * 64 * 4 + 8192
    assert rows["tail_eps_kernel"]["vgpr"] <= 256 and rows["tail_eps_kernel"]["agpr"] == 0
    assert rows["tail_cot_kernel"]["vgpr"] <= 256 and rows["tail_bwd_kernel"]["vgpr"] <= 256 and rows["tail_cot_kernel"]["agpr"] == 0
    assert rows["flows_eps_kernel"]["lds"] == 0
