"""The ray gradient of the fused render on the CPU: the G26 fixtures of the real reference (rays.grad of render_rays, rays_o / rays_d / c2w
grads of render), the oracle's autograd against them, the layout of the widened grad_flat (r_off, z_off), a torch restatement of the two
kernels' formulas against fp64 autograd, and the closed form pack_rays differentiates.  No kernel runs."""
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

import raygrad_common as RG
from util_hip import ATOL, RTOL, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["g26a_render_rays_rays_grad", "g26b_render_rays_od_grad", "g26c_render_c2w_grad"]
T = RG.T


def _digest(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))


def _manifest(path=RG.GOLDEN):
    with open(os.path.join(path, "MANIFEST.json")) as f:
        return json.load(f)


def test_raygrad_fixtures_match_their_manifest():
    man = _manifest()
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(RG.GOLDEN, "*.npz")))
    assert names == sorted(man) == sorted(NAMES)
    for name in names:
        g = RG.load(name)
        assert sorted(g) == sorted(man[name]), name
        for k, v in g.items():
            assert _digest(v) == man[name][k], (name, k)
        assert os.path.getsize(os.path.join(RG.GOLDEN, name + ".npz")) < 160 * 1024


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="the reference only exists in the build container")
def test_committed_raygrad_generator_reproduces_the_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_raygrad.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _manifest(str(tmp_path)) == _manifest()


def _oracle_fixture(name, g, dtype=torch.float32):
    """{name: gradient} of the fixture's loss by the oracle's autograd on the STORED masks, + the oracle's render dict"""
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    c = lambda a: T(a).to(dtype)
    p = {k: v.to(dtype) for k, v in O.make_params(cfg, int(g["seed"])).items()}
    masks = {k[len("mask."):]: T(v).to(dtype) for k, v in g.items() if k.startswith("mask.")}
    ea, er, tr, G, Gd = c(g["eps_alpha"]), c(g["eps_rgb"]), c(g["t_rand"]), c(g["G"]), c(g["Gd"])
    with O.relu_override(masks=masks):
        if name == NAMES[0]:
            leaves = {"rays_grad": c(g["ray_batch"]).requires_grad_(True)}
            ret = O.render_rays(p, leaves["rays_grad"], cfg, ea, er, True, tr)
        elif name == NAMES[1]:
            leaves = {"rays_o_grad": c(g["rays_o"]).requires_grad_(True), "rays_d_grad": c(g["rays_d"]).requires_grad_(True)}
            ret = O.render(p, int(g["H"]), int(g["W"]), float(g["focal"]), cfg, ea, er, True, rays=(leaves["rays_o_grad"], leaves["rays_d_grad"]),
                           ndc=True, near=0., far=1., t_rand=tr)
        else:
            leaves = {"c2w_grad": c(g["c2w"]).requires_grad_(True)}
            ret = O.render(p, 4, 4, float(g["focal"]), cfg, ea, er, True, c2w=leaves["c2w_grad"], ndc=False, near=2., far=6., t_rand=tr,
                           lindisp=True, white_bkgd=True)
            ret = dict(ret, rgb_map=ret["rgb_map"].reshape(16, 3, -1), depth_map=ret["depth_map"].reshape(16, -1))
    RG.linear_loss(ret, G, Gd).backward()
    return {k: v.grad for k, v in leaves.items()}, ret


@pytest.mark.parametrize("name", NAMES)
def test_oracle_autograd_reproduces_the_reference_ray_gradients(name):
    """oracle.render_rays / render are differentiable in rays, z_vals and c2w: the reference's gradients on the reference's masks - all 11
    columns of G26a, near / far (6, 7) included, which only the oracle covers (the kernels do not compute them, cfnerf.h)"""
    g = RG.load(name)
    grads, ret = _oracle_fixture(name, g)
    close(ret["rgb_map"], g["rgb_map"], what=f"{name} rgb_map")
    close(ret["depth_map"], g["depth_map"], what=f"{name} depth_map")
    close(ret["loss_entropy"], g["loss_entropy"], what=f"{name} entropy")
    for k, v in grads.items():
        assert np.abs(g[k]).max() > 0 and np.isfinite(g[k]).all()
        close(v, g[k], atol=2e-4 * float(np.abs(g[k]).max()), rtol=RTOL, what=f"{name} {k}")
    if name == NAMES[0]:
        assert np.abs(g["rays_grad"][:, 6:8]).min() > 0
        close(grads["rays_grad"][:, 6:8], g["rays_grad"][:, 6:8], atol=2e-4 * float(np.abs(g["rays_grad"][:, 6:8]).max()), rtol=RTOL, what="near / far")


def test_fixture_shapes_and_masks():
    a, b, c = (RG.load(n) for n in NAMES)
    assert a["ray_batch"].shape == (3, 11) and a["rays_grad"].shape == (3, 11) and a["t_rand"].shape == (3, 128)
    assert b["rays_o"].shape == (4, 3) and b["rays_o_grad"].shape == (4, 3) and b["rays_d_grad"].shape == (4, 3)
    assert c["c2w"].shape == (3, 4) and c["c2w_grad"].shape == (3, 4) and int(c["H"]) == int(c["W"]) == 4
    for g, P in ((a, 384), (b, 512), (c, 2048)):
        assert int(g["netwidth"]) == 64 and int(g["K"]) == 4 and float(g["min_abs_pre"]) > 0
        assert g["mask.trunk0"].shape == (P, 64) and g["mask.views"].shape == (P, 32)


@pytest.mark.parametrize("n,N,S", [(100, 3, 5), (0, 64, 1), (64, 128, 7), (12345, 1, 2), (595844, 1024, 128), (63, 5, 64), (65, 6, 130)])
def test_ray_grad_offsets_are_the_headers(n, N, S):
    """r_off = (param_count + 63) / 64 * 64, z_off = r_off + (N * 11 + 63) / 64 * 64, total = z_off + N * S: the header's formulas, computed
    in ONE place (_lib.ray_grad_offsets), which api._RenderFn and train.Trainer size their buffers with"""
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    m = re.search(r"r_off = \(cfnerf_param_count\(cfg\) \+ (\d+)\) / (\d+) \* (\d+),\s+z_off = r_off \+ \(N \* (\d+) \+ (\d+)\) / (\d+) \* (\d+)", hdr)
    assert m, "the header does not state the layout"
    a, b, c, cols, d, e, f = (int(v) for v in m.groups())
    m = re.search(r"CFNERF_F_RAY_GRAD\s*=\s*(0x[0-9a-fA-F]+|\d+)\b", hdr)
    assert m and int(m.group(1), 0) == 1 << 8 == L.F_RAY_GRAD
    r_off, z_off, total = L.ray_grad_offsets(n, N, S)
    assert r_off == (n + a) // b * c and z_off == r_off + (N * cols + d) // e * f and total == z_off + N * S and cols == 11
    assert r_off % 64 == 0 and z_off % 64 == 0 and 0 <= r_off - n < 64 and 0 <= z_off - (r_off + N * 11) < 64
    if (N * 11) % 64 == 0:
        assert z_off == r_off + N * 11                    # (no pad between the blocks)
    import inspect
    from cfnerf_amd import train
    assert "L.ray_grad_offsets(" in inspect.getsource(api._RenderFn.backward) and "L.ray_grad_offsets(" in inspect.getsource(train.Trainer._pass)


MIRROR_CASES = [(64, 3, 2, 5, False, {}), (64, 2, 3, 7, True, dict(multires=6, multires_views=2)), (64, 4, 1, 2, False, dict(netdepth=5)),
                (64, 2, 2, 66, False, {})]


@pytest.mark.parametrize("W,K,N,S,wb,kw", MIRROR_CASES)
def test_kernel_formulas_equal_fp64_autograd(W, K, N, S, wb, kw):
    """raygrad_common's torch restatement of comp_zgrad_kernel (the composite's z / |d| adjoint with the 1e1 last interval, the D recurrence)
    and of ray_grad_kernel's epilogue (the embedder's adjoint from stashed sin / cos, reduced through pts = o + d z) against autograd of
    O.render_rays in rays and z_vals, fp64, to 1e-10 of the largest entry"""
    cfg = O.OracleCfg(netwidth=W, K_samples=K, **kw)
    p = {k: v.double() for k, v in O.make_params(cfg, 5).items()}
    rng = np.random.default_rng(S)
    rays = RG.random_rays(rng, N, dtype=torch.float64).requires_grad_(True)
    z = torch.sort(torch.tensor(rng.uniform(2, 6, (N, S)))).values.requires_grad_(True)
    ea, er = torch.tensor(rng.standard_normal((K, 1))), torch.tensor(rng.standard_normal((K, 3)))
    G, Gd = torch.tensor(rng.standard_normal((N, 3, K))), torch.tensor(rng.standard_normal((N, K)))
    RG.linear_loss(O.render_rays(p, rays, cfg, ea, er, True, None, False, wb, z_vals=z), G, Gd).backward()
    d_rays, d_z = RG.mirror_ray_grads(p, rays.detach(), cfg, ea, er, G, Gd, z.detach(), wb)
    assert float(rays.grad[:, 6:8].abs().max()) == 0 and float(d_rays[:, 6:8].abs().max()) == 0
    for a, b in ((d_rays[:, 0:3], rays.grad[:, 0:3]), (d_rays[:, 3:6], rays.grad[:, 3:6]), (d_rays[:, 8:11], rays.grad[:, 8:11]), (d_z, z.grad)):
        assert float(b.abs().max()) > 0
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())


@pytest.mark.parametrize("mode", ["rays", "rays-ndc", "c2w", "c2w-ndc", "rays-near-far-tensors"])
def test_pack_rays_closed_form_equals_the_oracles_autograd(mode):
    """what pack_rays' backward differentiates (api.pack_rays_reference) against autograd of O.get_rays / O.ndc_rays / O.pack_rays, fp64"""
    rng = np.random.default_rng(len(mode))
    H, Wd, focal = 3, 5, 4.2
    ndc = mode.endswith("ndc")
    n = H * Wd
    D = torch.tensor(rng.standard_normal((n, 11)))
    near, far = (0., 1.) if ndc else (2., 6.)
    if mode.startswith("c2w"):
        pose = np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(-0.3, 0.3, (3, 1))], -1)
        a, b = torch.tensor(pose, requires_grad=True), torch.tensor(pose, requires_grad=True)
        got = api.pack_rays_reference(H, Wd, focal, c2w=a, ndc=ndc, near=near, far=far)
        ro, rd = O.get_rays(H, Wd, focal, b)
        ref = O.pack_rays(H, Wd, focal, ro, rd, ndc, near, far)
        leaves = [(a, b)]
    else:
        o, d = rng.uniform(-0.3, 0.3, (n, 3)), rng.standard_normal((n, 3)) * 0.3 + np.array([0.1, -0.2, -1.0])
        a = [torch.tensor(o, requires_grad=True), torch.tensor(d, requires_grad=True)]
        b = [torch.tensor(o, requires_grad=True), torch.tensor(d, requires_grad=True)]
        if mode == "rays-near-far-tensors":
            nt, ft = torch.tensor(rng.uniform(1, 2, n)), torch.tensor(rng.uniform(5, 6, n))
            got = api.pack_rays_reference(H, Wd, focal, rays=(a[0], a[1]), ndc=ndc, near=nt, far=ft)
            ref = O.pack_rays(H, Wd, focal, b[0], b[1], ndc, nt[:, None], ft[:, None])
        else:
            got = api.pack_rays_reference(H, Wd, focal, rays=(a[0], a[1]), ndc=ndc, near=near, far=far)
            ref = O.pack_rays(H, Wd, focal, b[0], b[1], ndc, near, far)
        leaves = list(zip(a, b))
    np.testing.assert_allclose(got.detach().numpy(), ref.detach().numpy(), rtol=1e-13, atol=1e-13)
    (got * D).sum().backward()
    (ref * D).sum().backward()
    for x, y in leaves:
        assert float(y.grad.abs().max()) > 0
        np.testing.assert_allclose(x.grad.numpy(), y.grad.numpy(), rtol=1e-11, atol=1e-11 * float(y.grad.abs().max()))
