"""-m gpu: the unfused seam is differentiable in the RAYS, like the reference's render_rays whatever network_query_fn is: raw2outputs in
z_vals and rays_d (CFNERF_F_SEAM_GRAD: comp_seam_zgrad_kernel behind cfnerf_composite_bwd), the sampling lines through their closed form,
the points handed to the query function.  Held to the G26 fixtures of the real reference in ALL ELEVEN columns (near / far included, which
no kernel path held before), to fp64 autograd of the oracle's raw2outputs, to the fused path's CFNERF_F_RAY_GRAD, and to "nothing else moved".

The kernel's bound is not fixed in advance: per tensor (d_z, d_rays_d) it is four times the LARGEST error, over the cases of
seamgrad_common.CASES, of the same formula evaluated by torch in fp32 on the CPU against the fp64 oracle (hardware transcendentals at K >= 16
and the wave scan's order differ from torch's).  The largest over the table and not the case's own figure, because d_rays_d of a ray is ONE
sum times the ray's direction: a case's own fp32 figure is a single draw of that sum's rounding noise, not its size.  Every measured figure
goes to the file named by CFNERF_SEAMGRAD_ERRORS (how profiles/r13_seamgrad_errors.txt is made)."""
import functools
import os

import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import api
from oracle import cfnerf_oracle as O

import raygrad_common as RG
import seamgrad_common as SG
from util_hip import RTOL, build_model, close, grad_close_tight, hip_relu_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE_X = 4.0             # the kernel may lose four times what torch's fp32 evaluation of its formula loses


def _record(case, what, rel, ref=None):
    line = f"{case:40s} {what:12s} {rel:.3e}" + ("" if ref is None else f"   fp32 formula on the CPU {ref:.3e}")
    print(line)
    path = os.environ.get("CFNERF_SEAMGRAD_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _passthrough(kw_train):
    """a plain network_query_fn of the caller's: run_network through create_nerf's closure, NOT marked fused"""
    q = kw_train["network_query_fn"]
    fn = lambda *a, **k: q(*a, **k)
    assert not getattr(fn, "_cfnerf_fused", False)
    return fn


# ---------------------------------------------------------------- 1. the reference's numbers (G26), through the seam
def _fixture_net(g):
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    _, kw_train, _, model, _, _ = build_model(cfg, int(g["seed"]))
    return cfg, kw_train, model, model.module


def _masks_equal_the_references(net, P, g, name):
    _, masks = hip_relu_masks(net, P)
    for k, m in masks.items():
        ref = RG.T(g["mask." + k]).float()
        assert torch.equal(m, ref), f"{name}: the HIP forward's ReLU mask of {k} differs from the reference's in {int((m != ref).sum())} units"


def test_g26a_ray_batch_grad_through_a_custom_query_fn_equals_the_references_in_all_eleven_columns():
    """Before CFNERF_F_SEAM_GRAD only columns 8..10 were filled here.  Bounds: columns 0..5 and 8..10 as the fused G26a test holds them
    (grad_close_tight: 2e-4 of the block's largest entry); near / far as tests/test_raygrad_cpu.py holds the fp32 oracle to the same fixture."""
    g = RG.load("g26a_render_rays_rays_grad")
    cfg, kw, model, net = _fixture_net(g)
    rb = RG.T(g["ray_batch"]).to(DEV).requires_grad_(True)
    ret = cfnerf_amd.render_rays(rb, model, _passthrough(kw), 128, True, False, perturb=1., t_rand=RG.T(g["t_rand"]), eps_alpha=RG.T(g["eps_alpha"]),
                                 eps_rgb=RG.T(g["eps_rgb"]))
    loss = (ret["rgb_map"] * RG.T(g["G"]).to(DEV)).sum() + (ret["depth_map"] * RG.T(g["Gd"]).to(DEV)).sum() + RG.C_ENT * ret["loss_entropy"].mean()
    loss.backward()
    _masks_equal_the_references(net, 3 * 128, g, "G26a")
    close(ret["rgb_map"], g["rgb_map"], what="G26a rgb_map")
    assert rb.grad is not None and tuple(rb.grad.shape) == (3, 11)
    for what, sl in (("rays_o", slice(0, 3)), ("rays_d", slice(3, 6)), ("near/far", slice(6, 8)), ("viewdirs", slice(8, 11))):
        _record("G26a through the seam", what, SG.rel(rb.grad[:, sl], RG.T(g["rays_grad"][:, sl])))
    for what, sl in (("rays_o", slice(0, 3)), ("rays_d", slice(3, 6)), ("viewdirs", slice(8, 11))):
        grad_close_tight(rb.grad[:, sl], g["rays_grad"][:, sl], "G26a seam rays.grad " + what)
    nf = g["rays_grad"][:, 6:8]
    assert abs(nf).min() > 0
    close(rb.grad[:, 6:8], nf, atol=2e-4 * float(abs(nf).max()), rtol=RTOL, what="G26a seam near / far")
    net.flat.grad = None


def test_g26b_rays_o_d_grads_through_a_custom_query_fn_equal_the_references():
    g = RG.load("g26b_render_rays_od_grad")
    cfg, kw, model, net = _fixture_net(g)
    ro, rd = RG.T(g["rays_o"]).to(DEV).requires_grad_(True), RG.T(g["rays_d"]).to(DEV).requires_grad_(True)
    rgb, _, depth, ex = cfnerf_amd.render(int(g["H"]), int(g["W"]), float(g["focal"]), rays=(ro, rd), ndc=True, near=0., far=1.,
                                          t_rand=RG.T(g["t_rand"]), eps_alpha=RG.T(g["eps_alpha"]), eps_rgb=RG.T(g["eps_rgb"]),
                                          **dict(kw, network_query_fn=_passthrough(kw)))
    ((rgb * RG.T(g["G"]).to(DEV)).sum() + (depth * RG.T(g["Gd"]).to(DEV)).sum() + RG.C_ENT * ex["loss_entropy"].mean()).backward()
    _masks_equal_the_references(net, 4 * 128, g, "G26b")
    close(rgb, g["rgb_map"], what="G26b rgb_map")
    _record("G26b through the seam", "rays_o", SG.rel(ro.grad, RG.T(g["rays_o_grad"])))
    _record("G26b through the seam", "rays_d", SG.rel(rd.grad, RG.T(g["rays_d_grad"])))
    grad_close_tight(ro.grad, g["rays_o_grad"], "G26b seam rays_o.grad")
    grad_close_tight(rd.grad, g["rays_d_grad"], "G26b seam rays_d.grad")
    net.flat.grad = None


def test_g26c_c2w_grad_through_a_custom_query_fn_equals_the_references():
    g = RG.load("g26c_render_c2w_grad")
    cfg, kw, model, net = _fixture_net(g)
    kw = dict(kw, ndc=False, lindisp=True, white_bkgd=True, network_query_fn=_passthrough(kw))
    pose = RG.T(g["c2w"]).to(DEV).requires_grad_(True)
    rgb, _, depth, ex = cfnerf_amd.render(4, 4, float(g["focal"]), c2w=pose, near=2., far=6., t_rand=RG.T(g["t_rand"]),
                                          eps_alpha=RG.T(g["eps_alpha"]), eps_rgb=RG.T(g["eps_rgb"]), **kw)
    ((rgb * RG.T(g["G"]).to(DEV).reshape(rgb.shape)).sum() + (depth * RG.T(g["Gd"]).to(DEV).reshape(depth.shape)).sum()
     + RG.C_ENT * ex["loss_entropy"].mean()).backward()
    _masks_equal_the_references(net, 16 * 128, g, "G26c")
    _record("G26c through the seam", "c2w", SG.rel(pose.grad, RG.T(g["c2w_grad"])))
    grad_close_tight(pose.grad, g["c2w_grad"], "G26c seam c2w.grad")
    net.flat.grad = None


# ---------------------------------------------------------------- 2. the kernel against the fp64 oracle
def _composite_bwd(inp, want_raw=True, want_z=True, want_d=True, seam=True, fill=None):
    """cfnerf_composite_bwd at the C ABI on the case's inputs -> (d_raw, d_z_vals, d_rays_d), None where not asked for"""
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    raw, z, d = dev(inp["raw"]), dev(inp["z"]), dev(inp["rays_d"])
    N, S, K = raw.shape[:3]
    cots = [dev(inp[k]) for k in ("G", "Gq", "Gd", "Gw")]
    new = lambda like: torch.empty_like(like) if fill is None else torch.full_like(like, fill)
    d_raw, d_z, d_d = (new(raw) if want_raw else None), (new(z) if want_z else None), (new(d) if want_d else None)
    if seam:
        out = L.composite_grads(d_raw=d_raw, d_z_vals=d_z, d_rays_d=d_d)
        arg, wb = L.composite_grads_arg(out), int(inp["wb"]) | L.F_SEAM_GRAD
    else:
        arg, wb = L.ptr(d_raw), int(inp["wb"])
    L.check(L.lib().cfnerf_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), N, S, K, wb, *[L.ptr(c) for c in cots], arg, L.stream()), "cfnerf_composite_bwd")
    torch.cuda.synchronize()
    return d_raw, d_z, d_d


@functools.lru_cache(maxsize=None)
def _kernel(i):
    return _composite_bwd(SG.inputs(i))


@functools.lru_cache(maxsize=None)
def _bounds():
    errs = [SG.fp32_formula_errors(i)[:2] for i in range(len(SG.CASES))]
    return NOISE_X * max(e[0] for e in errs), NOISE_X * max(e[1] for e in errs)


@pytest.mark.parametrize("i", range(len(SG.CASES)), ids=SG.IDS)
def test_kernel_d_z_vals_and_d_rays_d_vs_fp64_autograd_of_raw2outputs(i):
    ez32, ed32, z64, d64 = SG.fp32_formula_errors(i)
    _, d_z, d_d = _kernel(i)
    assert torch.isfinite(d_z).all() and torch.isfinite(d_d).all()
    ez, ed = SG.rel(d_z, z64), SG.rel(d_d, d64)
    _record(SG.IDS[i], "d_z_vals", ez, ez32)
    _record(SG.IDS[i], "d_rays_d", ed, ed32)
    bz, bd = _bounds()
    assert ez <= bz, f"d_z_vals: {ez:.3e} of the largest entry, beyond {NOISE_X:g} x the fp32 formula's worst over the cases ({bz:.3e})"
    assert ed <= bd, f"d_rays_d: {ed:.3e} of the largest entry, beyond {NOISE_X:g} x the fp32 formula's worst over the cases ({bd:.3e})"


# ---------------------------------------------------------------- 3. nothing else moved, bit-reproducible
@pytest.mark.parametrize("i", [1, 3, 4, 10], ids=[SG.IDS[j] for j in (1, 3, 4, 10)])
def test_d_raw_keeps_its_bits_and_two_runs_agree_bit_for_bit(i):
    inp = SG.inputs(i)
    d_raw, d_z, d_d = _kernel(i)
    plain, _, _ = _composite_bwd(inp, seam=False)                       # the call as it was: no bit, d_raw a device array
    assert torch.equal(plain, d_raw), "d_raw changed with CFNERF_F_SEAM_GRAD"
    SENT = 12345.0
    r2, z2, d2 = _composite_bwd(inp, fill=SENT)                         # into sentinel-filled buffers: every element is written
    assert torch.equal(r2, d_raw) and torch.equal(z2, d_z) and torch.equal(d2, d_d), "not bit-reproducible"
    assert not bool((z2 == SENT).any()) and not bool((d2 == SENT).any())
    # each output on its own: the same bits, and what is not asked for is not touched
    _, z3, none_d = _composite_bwd(inp, want_raw=False, want_d=False)
    assert none_d is None and torch.equal(z3, d_z)
    _, none_z, d3 = _composite_bwd(inp, want_raw=False, want_z=False)
    assert none_z is None and torch.equal(d3, d_d)
    r4, _, _ = _composite_bwd(inp, want_z=False, want_d=False)
    assert torch.equal(r4, d_raw)


def test_a_background_value_with_other_bits_set_is_still_white():
    """the background is white iff (white_bkgd & ~0x400) != 0: every value a caller passes today means what it meant"""
    inp = dict(SG.inputs(10))
    d_raw, _, _ = _kernel(10)
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    raw, z, d = dev(inp["raw"]), dev(inp["z"]), dev(inp["rays_d"])
    cots = [dev(inp[k]) for k in ("G", "Gq", "Gd", "Gw")]               # (kept alive across the launches)
    for wb in (1, 2, -1 & ~L.F_SEAM_GRAD):
        out = torch.empty_like(raw)
        L.check(L.lib().cfnerf_composite_bwd(L.ptr(raw), L.ptr(z), L.ptr(d), *raw.shape[:3], wb, *[L.ptr(c) for c in cots], L.ptr(out), L.stream()),
                "cfnerf_composite_bwd")
        assert torch.equal(out, d_raw), wb


def test_model_entry_points_refuse_the_bit_by_name():
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    _, _, _, model, _, _ = build_model(cfg, 5)
    net, lib = model.module, L.lib()
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_network_fwd(net.handle, None, None, 4, 4, L.F_TRAIN | L.F_STASH | L.F_SEAM_GRAD, None, None, L.stream())
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_F_SEAM_GRAD" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 128, 4, L.F_SEAM_GRAD, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_F_SEAM_GRAD" in err(), err()
    rc = lib.cfnerf_render_fwd(net.handle, None, None, None, None, None, 4, 128, 4, L.F_TRAIN | L.F_STASH | L.F_SEAM_GRAD, *([None] * 8), L.stream())
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_F_SEAM_GRAD" in err(), err()


# ---------------------------------------------------------------- 4. raw2outputs alone
def test_raw2outputs_differentiates_in_z_vals_with_a_detached_raw_and_asks_for_no_d_raw(monkeypatch):
    inp = SG.inputs(3)
    asked = []
    real = L.composite_grads
    monkeypatch.setattr(L, "composite_grads", lambda **kw: asked.append(kw) or real(**kw))
    raw, d = inp["raw"].to(DEV), inp["rays_d"].to(DEV)
    z = inp["z"].to(DEV).requires_grad_(True)
    rgb, disp, w, depth = cfnerf_amd.raw2outputs(raw, z, d, 0., inp["wb"])
    assert rgb.requires_grad and w.requires_grad
    ((rgb * inp["G"].to(DEV)).sum() + (disp * inp["Gq"].to(DEV)).sum() + (depth * inp["Gd"].to(DEV)).sum() + (w * inp["Gw"].to(DEV)).sum()).backward()
    assert len(asked) == 1 and asked[0]["d_raw"] is None and asked[0]["d_z_vals"] is not None and asked[0]["d_rays_d"] is None, asked
    assert torch.equal(z.grad, _kernel(3)[1])
    # all three at once: raw.grad is the plain backward's, bit for bit
    raw_l, z_l, d_l = raw.clone().requires_grad_(True), inp["z"].to(DEV).requires_grad_(True), d.clone().requires_grad_(True)
    rgb, disp, w, depth = cfnerf_amd.raw2outputs(raw_l, z_l, d_l, 0., inp["wb"])
    ((rgb * inp["G"].to(DEV)).sum() + (disp * inp["Gq"].to(DEV)).sum() + (depth * inp["Gd"].to(DEV)).sum() + (w * inp["Gw"].to(DEV)).sum()).backward()
    k_raw, k_z, k_d = _kernel(3)
    assert torch.equal(raw_l.grad, k_raw) and torch.equal(z_l.grad, k_z) and torch.equal(d_l.grad, k_d)
    # raw alone: the call as it was, no descriptor
    n = len(asked)
    raw_l = raw.clone().requires_grad_(True)
    rgb, _, _, _ = cfnerf_amd.raw2outputs(raw_l, inp["z"].to(DEV), d, 0., inp["wb"])
    (rgb * inp["G"].to(DEV)).sum().backward()
    assert len(asked) == n and raw_l.grad is not None


# ---------------------------------------------------------------- 5. the seam and the fused path agree
def test_seam_ray_gradient_and_d_z_agree_with_the_fused_paths_ray_grad(monkeypatch):
    """columns 0..5 and 8..10 of ray_batch.grad and the total d loss / d z_vals: through a pass-through network_query_fn, and from
    cfnerf_render_bwd of a CFNERF_F_RAY_GRAD stash.  Bound: grad_close_tight's 2e-4 of the block's largest entry, as the existing seam cross-check
    of tests/test_hip_raygrad.py.  The seam's d_z is read off the graph: the cotangent of the z_vals raw2outputs is handed + that of the
    points along the ray direction (pts = o + d z)."""
    import numpy as np
    N, S, K = 5, 66, 4
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    _, kw, _, model, p, _ = build_model(cfg, 78)
    net = model.module
    rng = np.random.default_rng(78)
    rb = RG.random_rays(rng, N)
    tv = torch.linspace(0., 1., S)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32)
    ea, er = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32), torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)
    G, Gd = (torch.tensor(rng.standard_normal((N, 3, K)), dtype=torch.float32) / N).to(DEV), (torch.tensor(rng.standard_normal((N, K)), dtype=torch.float32) / N).to(DEV)
    got = {}
    q, real_r2o = kw["network_query_fn"], api.raw2outputs

    def query(inputs, viewdirs, network_fn, is_val, is_test):
        inputs.register_hook(lambda g: got.__setitem__("d_pts", g.clone()))
        return q(inputs, viewdirs, network_fn, is_val, is_test)

    def r2o(raw, z_vals, rays_d, *a, **k):
        z_vals.register_hook(lambda g: got.__setitem__("d_z", g.clone()))
        return real_r2o(raw, z_vals, rays_d, *a, **k)
    monkeypatch.setattr(api, "raw2outputs", r2o)
    rbs = rb.to(DEV).requires_grad_(True)
    ret = cfnerf_amd.render_rays(rbs, model, query, S, True, False, perturb=1., t_rand=t_rand, eps_alpha=ea, eps_rgb=er, t_vals=tv)
    ((ret["rgb_map"] * G).sum() + (ret["depth_map"] * Gd).sum() + RG.C_ENT * ret["loss_entropy"].mean()).backward()
    seam_dz = got["d_z"] + (got["d_pts"] * rbs.detach()[:, None, 3:6]).sum(-1)
    net.flat.grad = None
    # the fused path at the C ABI: STASH | RAY_GRAD, then d_rays / d_z behind the parameter gradient
    rays = rb.to(DEV).contiguous()
    eps = torch.cat([er, ea], -1).to(DEV).contiguous()
    net._sync()
    net.ensure_workspace(N, S, K)
    api._render_fwd(net, rays, tv.to(DEV), t_rand.to(DEV), eps, L.F_TRAIN | L.F_STASH | L.F_RAY_GRAD)
    gen = L.lib().cfnerf_model_stash_generation(net.handle)
    r_off, z_off, total = L.ray_grad_offsets(net.n_params, N, S)
    buf = torch.empty(total, device=DEV)
    d_ent = torch.full((1,), RG.C_ENT, device=DEV)
    L.check(L.lib().cfnerf_render_bwd(net.handle, gen, L.ptr(G.contiguous()), L.ptr(Gd.contiguous()), L.ptr(d_ent), L.ptr(buf), L.stream()), "cfnerf_render_bwd")
    f_rays, f_dz = buf[r_off:r_off + N * 11].view(N, 11), buf[z_off:z_off + N * S].view(N, S)
    for what, sl in (("rays_o", slice(0, 3)), ("rays_d", slice(3, 6)), ("viewdirs", slice(8, 11))):
        _record("seam vs fused", what, SG.rel(rbs.grad[:, sl], f_rays[:, sl]))
        grad_close_tight(rbs.grad[:, sl], f_rays[:, sl].cpu().numpy(), "seam vs fused " + what)
    _record("seam vs fused", "d_z", SG.rel(seam_dz, f_dz))
    grad_close_tight(seam_dz, f_dz.cpu().numpy(), "seam vs fused d_z")
    assert float(rbs.grad[:, 6:8].abs().min()) > 0 and bool((f_rays[:, 6:8] == 0).all())      # near / far: the seam's alone


# ---------------------------------------------------------------- 6. the eval branch, and no request = the code as it was
def test_eval_branch_through_a_custom_query_fn_is_a_graph_in_the_rays_and_returns_the_eval_forward():
    N, K = 3, 4
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    _, kw, kw_test, model, _, _ = build_model(cfg, 80)
    net = model.module
    rb = RG.random_rays(__import__("numpy").random.default_rng(80), N).to(DEV)
    query = _passthrough(kw)
    with torch.no_grad():
        plain = cfnerf_amd.render_rays(rb, model, query, 128, False, False)
    same = cfnerf_amd.render_rays(rb, model, query, 128, False, False)          # grad mode on, nothing asks: the same code, the same bits
    assert not same["rgb_map"].requires_grad and torch.equal(same["rgb_map"], plain["rgb_map"])
    rbg = rb.clone().requires_grad_(True)
    ret = cfnerf_amd.render_rays(rbg, model, query, 128, False, False)
    assert sorted(ret) == sorted(plain) and ret["rgb_map"].requires_grad
    close(ret["rgb_map"], plain["rgb_map"], what="eval rgb_map with ray_batch.requires_grad")
    close(ret["depth_map"], plain["depth_map"], what="eval depth_map with ray_batch.requires_grad")
    (ret["rgb_map"].sum() + ret["depth_map"].sum()).backward()
    assert rbg.grad is not None and torch.isfinite(rbg.grad).all() and float(rbg.grad.abs().min()) > 0, rbg.grad
    net.flat.grad = None
