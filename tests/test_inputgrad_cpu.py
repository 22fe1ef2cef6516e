"""The input gradient of the seam on the CPU: the G25 fixtures of the real reference (x.grad of NeRF_Flows.forward, pts.grad / viewdirs.grad
of run_network), the oracle's autograd against them, the layout of the widened grad_flat (x_off) and the embedder's adjoint.  No kernel runs."""
import ctypes as C
import glob
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import api
from oracle import cfnerf_oracle as O

import inputgrad_common as IG
from util_hip import ATOL, RTOL, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _digest(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))


def _manifest(path=IG.DIR):
    with open(os.path.join(path, "MANIFEST.json")) as f:
        return json.load(f)


def test_inputgrad_fixtures_match_their_manifest():
    man = _manifest()
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(IG.DIR, "*.npz")))
    assert names == sorted(man) == sorted(IG.NAMES)
    for name in names:
        g = IG.load(name)
        assert sorted(g) == sorted(man[name]), name
        for k, v in g.items():
            assert _digest(v) == man[name][k], (name, k)
        assert os.path.getsize(os.path.join(IG.DIR, name + ".npz")) < 32 * 1024


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="the reference only exists in the build container")
def test_committed_inputgrad_generator_reproduces_the_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_inputgrad.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _manifest(str(tmp_path)) == _manifest()


def test_fixture_shapes_masks_and_the_seed_rule():
    a, b, c = (IG.load(n) for n in IG.NAMES)
    assert a["x"].shape == (8, 90) and a["x_grad"].shape == (8, 90) and a["raw"].shape == (8, 4, 4)
    assert b["pts"].shape == (2, 4, 3) and b["pts_grad"].shape == (2, 4, 3) and b["viewdirs_grad"].shape == (2, 3) and b["raw"].shape == (2, 4, 4, 4)
    assert c["x_grad"].shape == (8, 90) and c["sample_alpha"].shape == (4, 1) and c["sample_rgb"].shape == (4, 3)
    for g in (a, b, c):
        assert float(g["min_abs_pre"]) >= 2e-5 and int(g["netwidth"]) == 64 and int(g["K"]) == 4
        m = IG.masks_of(g)
        assert sorted(m) == sorted([f"trunk{i}" for i in range(8)] + ["views"])
        assert m["trunk0"].shape == (8, 64) and m["views"].shape == (8, 32)
        for k in ("x_grad", "pts_grad", "viewdirs_grad"):
            if k in g:
                assert np.isfinite(g[k]).all() and np.abs(g[k]).max() > 0


@pytest.mark.parametrize("name", IG.NAMES)
def test_oracle_autograd_reproduces_the_reference_input_gradients(name):
    """oracle.nerf_flows_forward / run_network are differentiable in their inputs: the same gradients as the reference's autograd, on the
    oracle's OWN masks (which are the reference's: the fixture's seed keeps every pre-activation >= 2e-5 from zero)"""
    g = IG.load(name)
    cfg, rec = IG.cfg_of(g), {}
    grads, raw = IG.oracle_grads(name, g)
    close(raw, g["raw"], what=f"{name} raw")
    with torch.no_grad(), O.relu_override(record=rec):
        x = IG.T(g["x"]) if "x" in g else torch.cat([O.embed(IG.T(g["pts"]).reshape(-1, 3), cfg.multires),
                                                     O.embed(IG.T(g["viewdirs"])[:, None].expand(2, 4, 3).reshape(-1, 3), cfg.multires_views)], -1)
        O.mlp_encode(O.make_params(cfg, int(g["seed"])), x, cfg)
    for k, m in IG.masks_of(g).items():
        assert torch.equal((rec[k] > 0).float(), m), f"{name}: the oracle's ReLU mask of {k} differs from the reference's"
    for k, v in grads.items():
        close(v, g[k], atol=ATOL * float(np.abs(g[k]).max()), rtol=RTOL, what=f"{name} {k}")


@pytest.mark.parametrize("kw", [dict(), dict(netwidth=64, multires=6, multires_views=2), dict(netwidth=512, netdepth=5, h_alpha_size=64)])
def test_x_off_formula_is_the_headers(kw):
    """d_x starts at x_off = (param_count + 63) / 64 * 64 floats: the header states it at the flag and at cfnerf_network_bwd, the host
    mirror computes it in ONE place (_lib.input_grad_offset) and api._NetworkFn sizes its buffer with that function"""
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    found = re.findall(r"x_off = \(cfnerf_param_count\(cfg\) \+ (\d+)\) / (\d+) \* (\d+)", hdr)
    assert len(found) == 2 and len(set(found)) == 1, found
    add, div, mul = (int(v) for v in found[0])
    m = re.search(r"CFNERF_F_INPUT_GRAD\s*=\s*(0x[0-9a-fA-F]+|\d+)\b", hdr)
    assert m and int(m.group(1), 0) == 1 << 7 == L.F_INPUT_GRAD
    oc = O.OracleCfg(**kw)
    cfg = api._cfg_struct(oc.netdepth, oc.netwidth, oc.multires, oc.multires_views, oc.h_alpha_size, oc.h_rgb_size, oc.n_flows)
    n = L.lib().cfnerf_param_count(C.byref(cfg))
    assert n > 0 and api.param_layout(cfg)[1] == n
    x_off = L.input_grad_offset(n)
    assert x_off == (n + add) // div * mul and x_off % 64 == 0 and 0 <= x_off - n < 64
    import inspect
    src = inspect.getsource(api._NetworkFn.backward)
    assert "L.input_grad_offset(ctx.n_params)" in src and "+ 63" not in src      # no second copy of the formula


@pytest.mark.parametrize("multires,P", [(10, 7), (4, 5), (1, 3)])
def test_embed_backward_formula_equals_autograd(multires, P):
    """d_in = d_out[:, :3] + sum_l f_l (cos_l d_sin_l - sin_l d_cos_l), sin / cos read from the forward's own output"""
    rng = np.random.default_rng(multires)
    x = torch.tensor(rng.uniform(-1, 1, (P, 3)), dtype=torch.float64, requires_grad=True)
    out = O.embed(x, multires)
    d_out = torch.tensor(rng.standard_normal(tuple(out.shape)), dtype=torch.float64)
    (ref,) = torch.autograd.grad(out, x, d_out)
    got = api.embed_backward(out.detach(), d_out, api.Embedder(multires).freq_bands)
    assert got.shape == (P, 3)
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-12, atol=1e-12 * float(ref.abs().max()))
    # ... and in fp32, as the node runs it
    got32 = api.embed_backward(out.detach().float(), d_out.float(), api.Embedder(multires).freq_bands)
    close(got32, ref.float(), atol=ATOL * float(ref.abs().max()), rtol=RTOL, what="embed backward fp32")
