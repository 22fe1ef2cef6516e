"""-m gpu: the depth-supervised train step (the reference's colmap_depth: colour rays + key-point rays in ONE render, RUN:1009-1024,
1052-1054) - the d_depth_map path of the fused backward pinned against the real reference (G24a / G24b / G24c, tests/golden/depth/):
in one launch, as the first network call + the rest (netchunk mode), in slices, in shards, and in the opt-in bf16x3 precision."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O
from util_hip import G_TIGHT, build_model, close, fern_rays, hip_relu_masks

import depth_common as DC
from depth_common import S, T, load

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_depth import reference_depth_step  # noqa: E402  (the reference's loop lines, restated once; imports no reference code)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(name, **over):
    g = load(name)
    cfg = DC.cfg_of(g)
    _, kw_train, _, model, p, _ = build_model(cfg, int(g["seed"]), no_ndc=True, netchunk_per_gpu=int(g["netchunk"]), **over)
    geo = dict(near=float(g["near"]), far=float(g["far"]), ndc=False)
    n_c = int(g["n_colour"])
    rays = T(g["rays"]).to(DEV)
    inputs = dict(rays=rays[:, :n_c].contiguous(), depth_rays=rays[:, n_c:].contiguous(), target=T(g["target"]).to(DEV),
                  target_depth=T(g["target_depth"]).to(DEV), t_rand=DC.t_rand_of(g).to(DEV), all_rays=rays,
                  chunks=torch.cat([T(g["eps_rgb"]), T(g["eps_alpha"])], -1))
    return g, cfg, kw_train, model.module, p, (int(g["H"]), int(g["W"]), float(g["focal"])), geo, inputs


def _hip_masks_per_call(net, g, hwf, geo, x):
    """The ReLU masks the HIP forward takes on the rays of every network call: a plain one-set launch of those rays (the masks belong to
    the trunk, which sees the points alone)."""
    out = []
    for c, (lo, hi) in enumerate(DC.calls_of(g)):
        tc = TR.Trainer(net)
        tc.forward_backward(*hwf, (x["all_rays"][0, lo:hi], x["all_rays"][1, lo:hi]), torch.zeros(hi - lo, 3, device=DEV),
                            t_rand=x["t_rand"][lo:hi].contiguous(), eps=x["chunks"][c].to(DEV), **geo)
        out.append(hip_relu_masks(net, (hi - lo) * S)[1])
    return out


def _mask_correction(net, p, g, hwf, geo, x):
    """Per tensor: (the oracle's depth-supervised step on the HIP forward's ReLU masks) - (the same on its own masks), fp32 on both
    sides like the fixture; the masks may differ on a rounding-sized share of the units only."""
    masks = _hip_masks_per_call(net, g, hwf, geo, x)
    t_rand = x["t_rand"].cpu()
    scal, g_own, _ = DC.oracle_depth_step(p, g, t_rand, flips_against=masks)
    n_flips, n_units = scal["flips"]
    assert n_flips <= max(2, 2e-4 * n_units), f"{n_flips} of {n_units} ReLU masks differ"
    _, g_hip, _ = DC.oracle_depth_step(p, g, t_rand, masks=masks)
    return {k: (None if g_own[k] is None else (g_hip[k] - g_own[k]).double().numpy().reshape(-1)) for k in g_own}


def _check_maps_and_scalars(tr, g, entropy):
    close(tr.rgb_map, g["rgb_map"], what="rgb_map")
    close(tr.depth, g["depth_map"], what="depth_map")
    close(tr.disp, g["disp_map"], atol=1e-4, rtol=1e-3, what="disp_map")
    close(tr.scalars[0].cpu(), g["loss"], what="loss")
    close(tr.scalars[1].cpu(), g["loss_nll"], what="loss_nll")
    close(tr.entropy.cpu().reshape(()), entropy, what="entropy")
    close(tr.depth_loss.cpu().reshape(()), g["depth_loss"], what="depth_loss")


def _check_gradients(net, grad, g, corr):
    """Every stored entry of the reference's gradient, moved onto the HIP forward's ReLU masks, within G_TIGHT of the tensor's largest."""
    grad = grad.detach().cpu().double().numpy()
    n_checked = 0
    for key, (off, cnt) in net.layout.items():
        gk = grad[off:off + cnt]
        fx = DC.fixture_gradient(g, key)
        if fx is None:
            assert not gk.any(), f"{key} must get a zero gradient"
            continue
        ref, idx, scale, norm = fx
        sel = slice(None) if idx is None else idx
        ref = ref + corr[key][sel]
        err = float(np.abs(gk[sel] - ref).max())
        assert err <= G_TIGHT * scale + 1e-4 * np.abs(ref).max(), f"grad {key}: {err / scale:.2e} of the largest entry"
        assert abs(float(np.linalg.norm(gk)) - norm) <= 2e-3 * norm + float(np.linalg.norm(corr[key])), "gradnorm " + key
        n_checked += 1
    assert n_checked >= 30


def _g24a_through_the_trainer(precision=None):
    g, cfg, kw_train, net, p, hwf, geo, x = _case("g24a_depth_one_call")
    if precision:
        net.set_precision(precision)
    tr = TR.Trainer(net, beta1=float(g["beta1"]))
    tr.depth_lambda = float(g["depth_lambda"])          # (= Trainer(depth_lambda=); as an attribute the VALUES below judge any Trainer)
    eps = x["chunks"][0].to(DEV)
    grad = tr.forward_backward(*hwf, x["rays"], x["target"], t_rand=x["t_rand"], eps=eps, depth_rays=x["depth_rays"],
                               target_depth=x["target_depth"], **geo).clone()
    assert tr.rgb_map.shape[0] == tr.depth.shape[0] == int(g["n_colour"]) + int(g["n_depth"]), "the launch is colour rays + depth rays"
    _check_maps_and_scalars(tr, g, g["loss_entropy"])
    _check_gradients(net, grad, g, _mask_correction(net, p, g, hwf, geo, x))
    # the depth term is no correction: the same call without the depth rays gives another gradient
    n_c = int(g["n_colour"])
    plain = TR.Trainer(net, beta1=float(g["beta1"])).forward_backward(*hwf, x["rays"], x["target"], t_rand=x["t_rand"][:n_c].contiguous(),
                                                                      eps=eps, **geo)
    assert float((grad - plain).abs().max()) > 10 * G_TIGHT * float(grad.abs().max())
    return g, kw_train, net, hwf, geo, x, grad


def test_g24a_trainer_depth_step_matches_the_reference():
    """G24a (24 colour + 8 depth rays, one network call) through Trainer.forward_backward(depth_rays=, target_depth=): maps, loss terms,
    depth_loss and every gradient entry of the real reference.  A Trainer that drops the two arguments renders 24 rays and misses the
    depth term, which carries most of this gradient."""
    g, kw_train, net, hwf, geo, x, grad = _g24a_through_the_trainer()
    # the reference's loop lines, unchanged, on render() of the concatenated rays under autograd: the same gradient
    rgb, disp, depth, extras = cfnerf_amd.render(*hwf, chunk=int(g["chunk"]), rays=x["all_rays"], near=geo["near"], far=geo["far"],
                                                 t_rand=x["t_rand"], eps_alpha=T(g["eps_alpha"][0]), eps_rgb=T(g["eps_rgb"][0]), **kw_train)
    L = reference_depth_step(rgb, depth, extras, x["target"], x["target_depth"], int(g["n_colour"]), 4, float(g["beta1"]),
                             float(g["depth_lambda"]))
    close(L["loss"], g["loss"], what="loss of the loop lines")
    L["loss"].backward()
    gd = net.flat.grad.detach()
    assert float((gd - grad).abs().max()) <= 1e-4 * float(grad.abs().max())


def test_g24a_depth_step_in_bf16x3_precision():
    """The same step with cfnerf_model_set_precision(m, 1), at the same tolerances."""
    _g24a_through_the_trainer("bf16x3")


@pytest.mark.parametrize("name", ["g24b_depth_two_calls", "g24c_depth_c2"])
def test_netchunk_depth_step_takes_the_first_calls_entropy(name):
    """G24b (two network calls, the boundary inside the colour rays) and G24c (1024 + 128 rays, three calls) through
    Trainer(latent_draws="netchunk"): the reference's entropy term is the FIRST network call's alone - not the all-point mean."""
    g, cfg, kw_train, net, p, hwf, geo, x = _case(name, latent_draws="netchunk")
    ent_first, ent_all = float(g["loss_entropy_chunks"][0]), float(g["loss_entropy_all_points"])
    assert abs(ent_first - ent_all) > 10 * (1e-5 + 1e-4 * abs(ent_first)), "the fixture cannot tell the two entropy rules apart"
    tr = TR.Trainer(net, beta1=float(g["beta1"]), latent_draws="netchunk", netchunk=int(g["netchunk"]), chunk=int(g["chunk"]),
                    depth_lambda=float(g["depth_lambda"]))
    grad = tr.forward_backward(*hwf, x["rays"], x["target"], t_rand=x["t_rand"], eps_chunks=x["chunks"], depth_rays=x["depth_rays"],
                               target_depth=x["target_depth"], **geo).clone()
    _check_maps_and_scalars(tr, g, g["loss_entropy"])
    close(tr.entropy.cpu().reshape(()), ent_first, what="entropy of the first call")
    _check_gradients(net, grad, g, _mask_correction(net, p, g, hwf, geo, x))
    net.release_workspace()


def _g24c_launch_mode(**trainer_kw):
    g, cfg, kw_train, net, p, hwf, geo, x = _case("g24c_depth_c2")
    tr = TR.Trainer(net, beta1=float(g["beta1"]), depth_lambda=float(g["depth_lambda"]), **trainer_kw)
    return g, net, tr, hwf, geo, x, x["chunks"][0].to(DEV)


def test_depth_batch_walked_in_slices_equals_the_one_launch_step():
    """G24c's 1152 rays with max_rays_per_launch=384 (launch mode, one latent set): slices of colour rows only and one of 256 colour +
    128 depth rows - gradient within the suite's slice bound of the one-launch step, scalars and depth_loss equal."""
    out = {}
    for form, mx in (("sliced", 384), ("one launch", None)):
        g, net, tr, hwf, geo, x, eps = _g24c_launch_mode(max_rays_per_launch=mx)
        grad = tr.forward_backward(*hwf, x["rays"], x["target"], t_rand=x["t_rand"], eps=eps, depth_rays=x["depth_rays"],
                                   target_depth=x["target_depth"], **geo).clone()
        out[form] = (grad, tr.depth.clone(), tr.scalars.clone(), tr.entropy.clone(), tr.depth_loss.clone(), tr.n_slices(1152))
        net.release_workspace()
    a, b = out["sliced"], out["one launch"]
    assert (a[5], b[5]) == (3, 1)
    assert torch.equal(a[1], b[1])
    assert float((a[0] - b[0]).abs().max()) <= 2e-5 * float(b[0].abs().max())
    for i, what in ((2, "scalars"), (3, "entropy"), (4, "depth_loss")):
        close(a[i].cpu(), b[i].cpu(), atol=1e-5, rtol=1e-5, what=what)


def test_depth_shards_add_up_to_the_full_step():
    """Two half shards (512 colour + 64 depth rays each) with world_size=2 semantics sum to the 1024 + 128 step: gradient, loss, nll,
    mse and depth_loss."""
    g, net, _, hwf, geo, x, eps = _g24c_launch_mode()
    n_c, n_d, beta1, lam = 1024, 128, float(g["beta1"]), float(g["depth_lambda"])

    def step(c0, c1, d0, d1, world):
        tr = TR.Trainer(net, beta1=beta1, depth_lambda=lam, world_size=world)
        t_rand = torch.cat([x["t_rand"][c0:c1], x["t_rand"][n_c + d0:n_c + d1]])
        grad = tr.forward_backward(*hwf, x["rays"][:, c0:c1].contiguous(), x["target"][c0:c1].contiguous(), t_rand=t_rand, eps=eps,
                                   depth_rays=x["depth_rays"][:, d0:d1].contiguous(), target_depth=x["target_depth"][d0:d1], **geo).clone()
        return grad, torch.cat([tr.scalars[:3], tr.depth_loss]).clone()
    g1, s1 = step(0, n_c, 0, n_d, 1)
    ga, sa = step(0, n_c // 2, 0, n_d // 2, 2)
    gb, sb = step(n_c // 2, n_c, n_d // 2, n_d, 2)
    scale = float(g1.abs().max())
    assert float((ga + gb - g1).abs().max()) <= 2e-5 * scale, float((ga + gb - g1).abs().max()) / scale
    close((sa + sb).cpu(), s1.cpu(), atol=1e-5, rtol=1e-5, what="loss, nll, mse, depth_loss: shard sums")
    assert torch.isfinite(s1).all() and float(s1[3]) > 0
    net.release_workspace()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_depth_step_equals_the_one_process_step():
    """World 2 on one GPU over gloo: every rank renders its shard of the colour rays and of the depth rays; the exchanged gradient
    and the summed contributions are the one-process step's on the whole batch with the same latents."""
    from conftest import FORKSERVER_CTX as ctx
    assert ctx is not None
    import depth_workers
    spec = dict(W=64, K=4, n_colour=48, n_depth=16, seed=29, data_seed=8, beta1=0.01, depth_lambda=0.1)
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=depth_workers.depth_trainer_rank, args=(r, 2, port, q, spec)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = {}
    for _ in range(2):
        rank, status, *rest = q.get(timeout=600)
        assert status == "ok", f"rank {rank} failed:\n{rest[0]}"
        got[rank] = rest
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    (e0, g0, s0, f0), (e1, g1, s1, f1) = got[0], got[1]
    assert np.array_equal(e0, e1) and np.array_equal(g0, g1) and np.array_equal(f0, f1)
    cfg = O.OracleCfg(netwidth=spec["W"], K_samples=spec["K"])
    _, _, _, model, _, _ = build_model(cfg, spec["seed"], no_ndc=True)
    rng = np.random.default_rng(spec["data_seed"])
    n_c, n_d = spec["n_colour"], spec["n_depth"]
    rays, (H, Wd, focal) = fern_rays(rng, n_c + n_d)
    target = torch.tensor(rng.uniform(0, 1, (n_c, 3)), dtype=torch.float32)
    td = torch.tensor(rng.uniform(2, 6, (n_d,)), dtype=torch.float32)
    t_rand = torch.tensor(rng.uniform(0, 1, (n_c + n_d, 128)), dtype=torch.float32)
    # the ranks' launches hold [colour shard | depth shard]: the same rays in another order, so t_rand follows its rays
    tr = TR.Trainer(model, beta1=spec["beta1"], depth_lambda=spec["depth_lambda"])
    grad = tr.forward_backward(H, Wd, focal, rays[:, :n_c].to(DEV), target.to(DEV), t_rand=t_rand.to(DEV), eps=T(e0).to(DEV), near=1.2, far=8.0,
                               ndc=False, depth_rays=rays[:, n_c:].to(DEV), target_depth=td.to(DEV)).cpu().numpy()
    assert np.abs(g0 - grad).max() <= 2e-5 * np.abs(grad).max()
    one = torch.cat([tr.scalars[:3], tr.depth_loss]).cpu().numpy()
    close(s0 + s1, one, atol=1e-5, rtol=1e-5, what="loss, nll, mse, depth_loss: rank sums")


def test_plain_step_is_untouched_and_the_refusals():
    """A Trainer(depth_lambda=0.1) stepped WITHOUT depth rays is the plain Trainer bit for bit over three steps (also after a
    depth-supervised step has used its buffers); every refusal raises what it says."""
    K, N = 4, 40
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    rng = np.random.default_rng(31)
    rays, (H, Wd, focal) = fern_rays(rng, N + 8)
    rays = rays.to(DEV)
    colour, drays = rays[:, :N].contiguous(), rays[:, N:].contiguous()
    target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32, device=DEV)
    td = torch.tensor(rng.uniform(2, 6, (8,)), dtype=torch.float32, device=DEV)
    t_rand = torch.tensor(rng.uniform(0, 1, (3, N, 128)), dtype=torch.float32, device=DEV)
    eps = torch.tensor(rng.standard_normal((3, K, 4)), dtype=torch.float32, device=DEV)
    out = {}
    for form, kw in (("plain", {}), ("depth_lambda", dict(depth_lambda=0.1))):
        _, _, _, model, _, _ = build_model(cfg, 11)
        tr = TR.Trainer(model, beta1=0.01, **kw)
        rec = []
        for i in range(3):
            sc = tr.step(H, Wd, focal, colour, target, t_rand=t_rand[i], eps=eps[i])
            rec.append((tr.grad.clone(), sc.clone(), model.module.flat.detach().clone()))
        out[form] = rec
    for a, b in zip(out["plain"], out["depth_lambda"]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    # a plain launch of N + 8 rays after a depth-supervised one of N + 8 (same buffers), then the depth-supervised one again
    both = rays.contiguous()
    tgt2 = torch.cat([target, target[:8]])
    t2 = torch.cat([t_rand[0], t_rand[1][:8]])
    kwd = dict(t_rand=t2, eps=eps[0], depth_rays=drays, target_depth=td)
    d1 = tr.forward_backward(H, Wd, focal, colour, target, **kwd).clone()
    p1 = tr.forward_backward(H, Wd, focal, both, tgt2, t_rand=t2, eps=eps[0]).clone()
    p0 = TR.Trainer(model, beta1=0.01).forward_backward(H, Wd, focal, both, tgt2, t_rand=t2, eps=eps[0]).clone()
    d2 = tr.forward_backward(H, Wd, focal, colour, target, **kwd).clone()
    assert torch.equal(p1, p0) and torch.equal(d1, d2) and not torch.equal(d1, p1)
    tr.forward_backward_hierarchical(H, Wd, focal, both, tgt2, eps=eps[0])                     # (the extension's passes share those buffers too)
    assert torch.equal(tr.forward_backward(H, Wd, focal, colour, target, **kwd), d1)

    with pytest.raises(ValueError):
        tr.forward_backward(H, Wd, focal, colour, target, depth_rays=drays)
    with pytest.raises(ValueError):
        tr.step(H, Wd, focal, colour, target, target_depth=td)
    with pytest.raises(ValueError):
        TR.Trainer(model, beta1=0.01).step(H, Wd, focal, colour, target, depth_rays=drays, target_depth=td)
    with pytest.raises(NotImplementedError):
        tr.step_hierarchical(H, Wd, focal, colour, target, depth_rays=drays, target_depth=td)
    nc = dict(latent_draws="netchunk", netchunk=1024, chunk=1024, depth_lambda=0.1)           # 8 rays per network call: 6 calls
    with pytest.raises(NotImplementedError):
        TR.Trainer(model, world_size=2, **nc).forward_backward(H, Wd, focal, colour, target, depth_rays=drays, target_depth=td)
    with pytest.raises(NotImplementedError):
        TR.Trainer(model, max_rays_per_launch=16, **nc).forward_backward(H, Wd, focal, colour, target, depth_rays=drays, target_depth=td)
    one_call = dict(nc, netchunk=65536)                                                        # ... one network call: sliced as ever
    TR.Trainer(model, max_rays_per_launch=16, **one_call).forward_backward(H, Wd, focal, colour, target, depth_rays=drays, target_depth=td)
    torch.cuda.synchronize()
