"""-m gpu: NeRF_Flows.forward and Embedder.embed are differentiable in their INPUTS, like the reference's (MOD:188-291, HLP:21-69 are
ordinary autograd graphs): cfnerf_network_fwd with CFNERF_F_STASH | CFNERF_F_INPUT_GRAD, then cfnerf_network_bwd writes d loss / d x
behind the parameter gradient (input_grad_kernel).  Held to the oracle's autograd on the ReLU masks the HIP forward took, to the G25
fixtures of the real reference, and to "nothing else moved"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import api
from oracle import cfnerf_oracle as O

import inputgrad_common as IG
from util_hip import build_model, close, grad_close_tight, hip_relu_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
C_ENT = 0.3

# (W, K, P, OracleCfg extras, mode)                                               what it covers
CASES = [
    (64, 3, 1, {}, None),                                                       # one row
    (64, 8, 64, {}, None),                                                      # one whole tile: Q4 streams
    (128, 3, 65, {}, None),                                                     # a partial second tile: row-major
    (192, 4, 130, {}, None),
    (256, 16, 257, {}, None),                                                   # fast flow math
    (512, 2, 96, dict(h_alpha_size=64), None),
    (256, 4, 70, dict(netdepth=5), None),                                       # skip elsewhere (odd depth: no skip concat at all)
    (64, 4, 100, dict(multires=6, multires_views=2), "layout"),                 # row stride 54
    (256, 4, 128, {}, "bf16x3"),
    (128, 4, 130, {}, "rows"),                                                  # per-point latent rows (CFNERF_F_EPS_ROWS)
    (64, 4, 70, dict(netdepth=6), None),                                        # an even depth other than 8: the skip concat feeds layer 4
]
IDS = [f"W{w}-K{k}-P{p}" + ("-" + "-".join(f"{a}{b}" for a, b in kw.items()) if kw else "") + (f"-{m}" if m else "") for w, k, p, kw, m in CASES]
ROWS_NETCHUNK = 64


def _loss(raw, ent, G):
    return (raw * G).sum() + C_ENT * ent.mean()


@functools.lru_cache(maxsize=None)
def _case(i):
    """One HIP forward + backward of case i with x.requires_grad and the oracle's gradient on the masks that forward took: computed once,
    shared by the tests below (none of them changes what is kept here)."""
    W, K, P, kw, mode = CASES[i]
    cfg = O.OracleCfg(netwidth=W, K_samples=K, **kw)
    _, _, _, model, p, _ = build_model(cfg, 900 + W + K)
    net = model.module
    if mode == "bf16x3":
        net.set_precision("bf16x3")
    rng = np.random.default_rng(P + K)
    pts = torch.tensor(rng.uniform(-1, 1, (P, 3)), dtype=torch.float32)
    dirs = torch.nn.functional.normalize(torch.tensor(rng.standard_normal((P, 3)), dtype=torch.float32), dim=-1)
    x = torch.cat([O.embed(pts, cfg.multires), O.embed(dirs, cfg.multires_views)], -1)
    n_sets = -(-P // ROWS_NETCHUNK) if mode == "rows" else None
    shape = (lambda d: (n_sets, K, d)) if n_sets else (lambda d: (K, d))
    ea = torch.tensor(rng.standard_normal(shape(1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal(shape(3)), dtype=torch.float32)
    if n_sets:
        net.netchunk = ROWS_NETCHUNK                     # explicit [C,K,.] latents: one pair per 64 points -> one latent row per point
    G = torch.tensor(rng.standard_normal((P, K, 4)), dtype=torch.float32) / (P * K)
    net.flat.grad = None
    xg = x.to(DEV).requires_grad_(True)
    raw, ent = net(xg, False, False, eps_alpha=ea, eps_rgb=er)
    assert raw.requires_grad and list(ent.shape) == [P, K, 1]
    _loss(raw, ent, G.to(DEV)).backward()
    assert xg.grad is not None and xg.grad.shape == x.shape, "NeRF_Flows.forward gave no input gradient"
    dx, grad = xg.grad.detach().clone(), net.flat.grad.detach().clone()
    # the oracle on the ReLU masks the HIP forward took (tests/util_hip.py)
    _, masks = hip_relu_masks(net, P)
    xo = x.clone().requires_grad_(True)
    with O.relu_override(masks=masks):
        if n_sets:                                       # one oracle call per latent pair; the entropy is the point-weighted mean
            raws, ent_o = [], 0.
            for c in range(n_sets):
                lo, hi = c * ROWS_NETCHUNK, min((c + 1) * ROWS_NETCHUNK, P)
                with O.relu_override(masks={k: v[lo:hi] for k, v in masks.items()}):
                    r, e = O.nerf_flows_forward(p, xo[lo:hi], ea[c], er[c], cfg, False)
                raws.append(r)
                ent_o = ent_o + e * ((hi - lo) / P)
            raw_o = torch.cat(raws, 0)
        else:
            raw_o, ent_o = O.nerf_flows_forward(p, xo, ea, er, cfg, False)
    ((raw_o * G).sum() + C_ENT * ent_o).backward()
    return dict(cfg=cfg, net=net, model=model, p=p, x=x, ea=ea, er=er, G=G, raw=raw.detach(), ent=ent.mean().detach(), dx=dx, grad=grad,
                raw_o=raw_o.detach(), ent_o=ent_o.detach(), dx_o=xo.grad.clone(), masks=masks)


# ---------------------------------------------------------------- 1. against the oracle, on the masks the HIP forward took
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_input_gradient_vs_oracle_autograd(i):
    c = _case(i)
    close(c["raw"], c["raw_o"], what="raw")
    close(c["ent"], c["ent_o"], what="entropy")
    rel = float((c["dx"].cpu().double() - c["dx_o"].double()).abs().max() / c["dx_o"].double().abs().max())
    print(f"{IDS[i]}: d_x max error {rel:.3e} of the largest entry ({float(c['dx_o'].abs().max()):.3e})")
    grad_close_tight(c["dx"], c["dx_o"].numpy(), f"d_x {IDS[i]}")
    if CASES[i][4] == "layout":
        _check_layout_at_the_c_abi(c)


def _check_layout_at_the_c_abi(c):
    """row stride ic + icv = 54: the 64- / 32-wide padded outputs of the kernel store nothing past column 54 (it would be the next row) or
    past row P, and the floats between param_count and x_off are not written"""
    net, (P, Cx), K = c["net"], c["x"].shape, c["cfg"].K_samples
    assert Cx == 54
    n = net.n_params
    x_off = L.input_grad_offset(n)
    xf = c["x"].to(DEV).contiguous()
    eps = api.LT.pack(c["ea"], c["er"]).to(DEV)
    net._sync()
    net.ensure_workspace(1, P, K)
    api._network_fwd(net, xf, eps, K, L.F_TRAIN | L.F_STASH | L.F_INPUT_GRAD)
    gen = L.lib().cfnerf_model_stash_generation(net.handle)
    SENT, extra = 12345.0, 3 * Cx + 7
    buf = torch.full((x_off + P * Cx + extra,), SENT, device=DEV)
    d_raw, d_ent = c["G"].to(DEV).contiguous(), torch.full((1,), C_ENT, device=DEV)
    L.check(L.lib().cfnerf_network_bwd(net.handle, gen, L.ptr(d_raw), L.ptr(d_ent), L.ptr(buf), L.stream()), "cfnerf_network_bwd")
    assert torch.equal(buf[:n], c["grad"]), "parameter gradient at the C ABI"
    assert bool((buf[n:x_off] == SENT).all()), "pad floats before x_off were written"
    assert bool((buf[x_off + P * Cx:] == SENT).all()), "rows past P were written"
    assert torch.equal(buf[x_off:x_off + P * Cx].view(P, Cx), c["dx"]), "d_x at the C ABI"
    assert not bool((buf[x_off:x_off + P * Cx] == SENT).any())


# ---------------------------------------------------------------- 2. against the reference
def _hip_masks_equal_the_references(net, P, g, name):
    _, masks = hip_relu_masks(net, P)
    ref = IG.masks_of(g)
    assert sorted(masks) == sorted(ref)
    for k in ref:
        assert torch.equal(masks[k], ref[k]), f"{name}: the HIP forward's ReLU mask of {k} differs from the reference's in {int((masks[k] != ref[k]).sum())} units"


def _fixture_model(g):
    _, _, _, model, _, _ = build_model(IG.cfg_of(g), int(g["seed"]))
    return model, model.module


def test_g25a_train_branch_x_grad_equals_the_references():
    g = IG.load("g25a_train_x_grad")
    _, net = _fixture_model(g)
    x = IG.T(g["x"]).to(DEV).requires_grad_(True)
    raw, ent = net(x, False, False, eps_alpha=IG.T(g["eps_alpha"]), eps_rgb=IG.T(g["eps_rgb"]))
    ((raw * IG.T(g["G"]).to(DEV)).sum() + float(g["c_entropy"]) * ent.mean()).backward()
    _hip_masks_equal_the_references(net, 8, g, "G25a")
    close(raw, g["raw"], what="G25a raw")
    close(ent.mean(), g["loss_entropy"], what="G25a entropy")
    grad_close_tight(x.grad, g["x_grad"], "G25a x.grad")


def test_g25b_run_network_pts_and_viewdirs_grads_equal_the_references():
    """the embedder's adjoint and the expand-sum of a ray's view direction over its samples"""
    g = IG.load("g25b_run_network_grads")
    model, net = _fixture_model(g)
    embed_fn, _ = cfnerf_amd.get_embedder(10)
    embeddirs_fn, _ = cfnerf_amd.get_embedder(4)
    ea, er = IG.T(g["eps_alpha"]), IG.T(g["eps_rgb"])
    pts, dirs = IG.T(g["pts"]).to(DEV).requires_grad_(True), IG.T(g["viewdirs"]).to(DEV).requires_grad_(True)
    fn = lambda e, is_val, is_test: model(e, is_val, is_test, eps_alpha=ea, eps_rgb=er)
    raw, ent = cfnerf_amd.run_network(pts, dirs, fn, False, False, embed_fn, embeddirs_fn, netchunk=1024 * 64)
    assert tuple(raw.shape) == (2, 4, 4, 4)
    ((raw.reshape(8, 4, 4) * IG.T(g["G"]).to(DEV)).sum() + float(g["c_entropy"]) * ent.mean()).backward()
    _hip_masks_equal_the_references(net, 8, g, "G25b")
    close(raw, g["raw"], what="G25b raw")
    grad_close_tight(pts.grad, g["pts_grad"], "G25b pts.grad")
    grad_close_tight(dirs.grad, g["viewdirs_grad"], "G25b viewdirs.grad")


def test_g25c_eval_branch_x_grad_equals_the_references():
    g = IG.load("g25c_eval_x_grad")
    _, net = _fixture_model(g)
    net.sample_alpha, net.sample_rgb = IG.T(g["sample_alpha"]), IG.T(g["sample_rgb"])
    x = IG.T(g["x"]).to(DEV).requires_grad_(True)
    raw, aux = net(x, False, True)
    assert raw.requires_grad and aux.shape == raw.shape and not aux.any()          # MOD:223
    (raw * IG.T(g["G"]).to(DEV)).sum().backward()
    _hip_masks_equal_the_references(net, 8, g, "G25c")
    close(raw, g["raw"], what="G25c raw")
    grad_close_tight(x.grad, g["x_grad"], "G25c x.grad")


# ---------------------------------------------------------------- 3. a frozen network still gives x.grad
@pytest.mark.parametrize("i", [1, 2], ids=[IDS[1], IDS[2]])
def test_frozen_network_gives_the_same_input_gradient(i):
    c = _case(i)
    net = c["net"]
    net.flat.requires_grad_(False)
    try:
        xg = c["x"].to(DEV).requires_grad_(True)
        raw, ent = net(xg, False, False, eps_alpha=c["ea"], eps_rgb=c["er"])
        assert raw.requires_grad, "a frozen network with x.requires_grad returned a tensor with no graph"
        _loss(raw, ent, c["G"].to(DEV)).backward()
    finally:
        net.flat.requires_grad_(True)
    assert torch.equal(raw.detach(), c["raw"])
    assert torch.equal(xg.grad, c["dx"])


# ---------------------------------------------------------------- 4. nothing else moved
@pytest.mark.parametrize("i", [1, 2, 8, 9], ids=[IDS[1], IDS[2], IDS[8], IDS[9]])
def test_without_an_input_gradient_nothing_moved(i):
    c = _case(i)
    net, (W, K, P, _, _) = c["net"], CASES[i]
    lib = L.lib()
    ws_flagged = (lib.cfnerf_model_workspace_bytes(net.handle), net._ws.numel())
    G = c["G"].to(DEV)
    # the same launch without x.requires_grad: parameter gradient, raw and entropy keep their bits
    net.flat.grad = None
    raw, ent = net(c["x"].to(DEV), False, False, eps_alpha=c["ea"], eps_rgb=c["er"])
    _loss(raw, ent, G).backward()
    assert torch.equal(net.flat.grad, c["grad"]), "the parameter gradient changed with x.requires_grad"
    assert torch.equal(raw.detach(), c["raw"]) and torch.equal(ent.mean().detach(), c["ent"])
    # the workspace is what it was: d_x goes to the caller's buffer
    assert (lib.cfnerf_model_workspace_bytes(net.handle), net._ws.numel()) == ws_flagged
    assert net._ws.numel() == lib.cfnerf_workspace_bytes(C.byref(net.cfg), 1, P, K)
    # two backwards of one forward: bit-equal d_x (no atomics)
    xg = c["x"].to(DEV).requires_grad_(True)
    raw, ent = net(xg, False, False, eps_alpha=c["ea"], eps_rgb=c["er"])
    loss = _loss(raw, ent, G)
    (d1,) = torch.autograd.grad(loss, xg, retain_graph=True)
    (d2,) = torch.autograd.grad(loss, xg)
    assert torch.equal(d1, d2) and torch.equal(d1, c["dx"])
    net.flat.grad = None


def test_eval_branch_with_an_input_gradient_returns_the_eval_forward():
    c = _case(2)
    net = c["net"]
    with torch.no_grad():
        raw0, aux0 = net(c["x"].to(DEV), False, True)
    xg = c["x"].to(DEV).requires_grad_(True)
    raw1, aux1 = net(xg, False, True)
    assert not raw0.requires_grad and raw1.requires_grad and not aux1.any() and aux1.shape == raw1.shape
    close(raw1, raw0, what="eval raw with x.requires_grad")
    print("is_test=True with x.requires_grad: raw bit-equal to the no-grad eval forward:", bool(torch.equal(raw1.detach(), raw0)))
    raw1.sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0
    net.flat.grad = None


# ---------------------------------------------------------------- 5. refusals at the C ABI, each by message
def test_refusals_name_the_flags():
    c = _case(0)
    net, lib = c["net"], L.lib()
    P, K = c["x"].shape[0], c["cfg"].K_samples
    xf, eps = c["x"].to(DEV).contiguous(), api.LT.pack(c["ea"], c["er"]).to(DEV)
    raw, ent = torch.empty(P, K, 4, device=DEV), torch.zeros(1, device=DEV)
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_network_fwd(net.handle, L.ptr(xf), L.ptr(eps), P, K, L.F_TRAIN | L.F_INPUT_GRAD, L.ptr(raw), L.ptr(ent), L.stream())
    assert rc != 0 and "CFNERF_F_INPUT_GRAD" in err() and "CFNERF_F_STASH" in err(), err()
    rc = lib.cfnerf_network_fwd(net.handle, L.ptr(xf), L.ptr(eps), P, K, L.F_GEOMETRY | L.F_INPUT_GRAD, L.ptr(raw), None, L.stream())
    assert rc != 0 and "CFNERF_F_INPUT_GRAD" in err() and "CFNERF_F_GEOMETRY" in err(), err()
    rc = lib.cfnerf_render_fwd(net.handle, None, None, None, None, None, 4, 128, K, L.F_INPUT_GRAD, None, None, None, None, None, None, None, None,
                               L.stream())
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_F_INPUT_GRAD" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 128, max(K, 2), L.F_INPUT_GRAD, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_F_INPUT_GRAD" in err(), err()
    rc = lib.cfnerf_sample_points(None, None, None, L.F_INPUT_GRAD, 4, 128, None, None, L.stream())
    assert rc != 0 and "cfnerf_sample_points does not take CFNERF_F_INPUT_GRAD" in err(), err()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. a learnable front end trains through a custom network_query_fn
def test_a_learnable_point_offset_trains_through_a_custom_query_fn():
    """8 rays x 16 samples, W = 64: a 3-vector added to every sample point inside the caller's network_query_fn; its gradient through
    run_network + raw2outputs + the reference's loss against the oracle's (fp64, on the HIP forward's masks), and one SGD step."""
    N, S, K, beta1 = 8, 16, 4, 0.05
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    _, _, _, model, p, _ = build_model(cfg, 61)
    net = model.module
    rng = np.random.default_rng(6)
    rays_o = torch.tensor(rng.uniform(-0.3, 0.3, (N, 3)), dtype=torch.float32)
    rays_d = torch.tensor(rng.standard_normal((N, 3)) * 0.3 + np.array([0, 0, -1.]), dtype=torch.float32)
    viewdirs = torch.nn.functional.normalize(rays_d, dim=-1)
    z_vals = torch.sort(torch.tensor(rng.uniform(0.2, 1.5, (N, S)), dtype=torch.float32), -1).values
    pts = rays_o[:, None] + rays_d[:, None] * z_vals[..., None]
    target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32)
    ea = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)
    delta0 = torch.tensor([0.02, -0.01, 0.03])
    embed_fn, _ = cfnerf_amd.get_embedder(10)
    embeddirs_fn, _ = cfnerf_amd.get_embedder(4)
    network_fn = lambda e, is_val, is_test: model(e, is_val, is_test, eps_alpha=ea, eps_rgb=er)

    def hip_loss(delta):
        def my_query_fn(inputs, viewdirs, network_fn, is_val, is_test):          # the caller's: something learnable in front of the network
            return cfnerf_amd.run_network(inputs + delta, viewdirs, network_fn, is_val, is_test, embed_fn=embed_fn, embeddirs_fn=embeddirs_fn)
        raw, ent = my_query_fn(pts.to(DEV), viewdirs.to(DEV), network_fn, False, False)
        rgb, _, _, _ = cfnerf_amd.raw2outputs(raw, z_vals.to(DEV), rays_d.to(DEV))
        # (the loss lines in fp64 on the fp32 maps: the SGD step below moves the loss by ~1e-6 of its value)
        return O.train_loss(rgb.double(), target.to(DEV).double(), ent.mean().double(), K, beta1)["loss"]

    delta = delta0.to(DEV).requires_grad_(True)
    net.flat.grad = None
    loss = hip_loss(delta)
    loss.backward()
    assert delta.grad is not None, "no gradient reached the front end"
    _, masks = hip_relu_masks(net, N * S)
    d = lambda t: t.double()
    do = d(delta0).requires_grad_(True)
    with O.relu_override(masks=masks):
        raw_o, ent_o = O.run_network({k: d(v) for k, v in p.items()}, d(pts) + do, d(viewdirs), d(ea), d(er), cfg, False)
    rgb_o = O.raw2outputs(raw_o, d(z_vals), d(rays_d))[0]
    loss_o = O.train_loss(rgb_o, d(target), ent_o, K, beta1)["loss"]
    loss_o.backward()
    close(loss, loss_o, atol=1e-5, rtol=1e-4, what="loss")
    print("d loss / d delta:", delta.grad.cpu().numpy(), "oracle:", do.grad.numpy())
    grad_close_tight(delta.grad, do.grad.numpy(), "d loss / d delta")
    # one SGD step of a length far below the encoding's shortest period (2 pi / 2^9) lowers the loss
    lr = 1e-3 / float(delta.grad.norm())
    with torch.no_grad():
        after = hip_loss(delta - lr * delta.grad)
    print(f"loss {float(loss.detach()):.8f} -> {float(after):.8f}")
    assert float(after) < float(loss.detach())
    net.flat.grad = None
