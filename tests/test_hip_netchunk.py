"""-m gpu: per-netchunk latents (CFNERF_F_EPS_ROWS).  The reference draws fresh latents for every netchunk points
(RUN:47-64,82; MOD:234,246); in latent_draws="netchunk" mode every ray (fused path) or point (unfused seam) reads its own
latent row.  Pinned against the real reference (G23a / G23b, tests/golden/netchunk/), against the oracle, and against the
default one-set launch."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import api
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O
from util_hip import G_TIGHT, build_model, close, fern_rays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden import reference_kde_nll  # noqa: E402  (the reference's loss lines, restated once; imports no reference code)
from test_hip_train import mask_corrected  # noqa: E402

pytestmark = pytest.mark.gpu
T = lambda a: torch.tensor(np.asarray(a))
DEV = "cuda"
NC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "netchunk")


def load(name):
    return dict(np.load(os.path.join(NC, name + ".npz"), allow_pickle=False))


def _g23b_inputs(g):
    n = g["rays"].shape[1]
    import hashlib
    t_np = np.random.default_rng(int(g["t_rand_seed"])).uniform(0, 1, (n, 128)).astype(np.float32)
    assert hashlib.sha256(t_np.tobytes()).hexdigest() == str(g["t_rand_sha256"])
    return n, T(t_np)


def test_g23b_trainer_netchunk_matches_the_reference_c2_batch():
    """G23b (C2: 1024 rays = two netchunks, two latent pairs) through Trainer(latent_draws="netchunk"): maps, loss, entropy and the
    sampled gradients at G21's tolerances (mask-corrected per chunk with weights N_c / N).  The default mode reads one latent set
    for every ray and misses the second chunk's latents: this is the test that needs the feature."""
    g = load("g23b_netchunk_c2")
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    _, kw_train, _, model, p, _ = build_model(cfg, int(g["seed"]), no_ndc=True, latent_draws="netchunk")
    net = model.module
    n, t_rand = _g23b_inputs(g)
    H, W, focal, near, far, beta1 = int(g["H"]), int(g["W"]), float(g["focal"]), float(g["near"]), float(g["far"]), float(g["beta1"])
    chunks = torch.cat([T(g["eps_rgb"]), T(g["eps_alpha"])], -1)
    tr = TR.Trainer(net, beta1=beta1, latent_draws="netchunk", netchunk=int(g["netchunk"]), chunk=int(g["chunk"]))
    rays = T(g["rays"]).to(DEV)
    grad = tr.forward_backward(H, W, focal, rays, T(g["target"]).to(DEV), t_rand=t_rand.to(DEV), eps_chunks=chunks, near=near, far=far,
                               ndc=False).cpu().clone()
    close(tr.rgb_map, g["rgb_map"], what="rgb_map")
    close(tr.depth, g["depth_map"], what="depth_map")
    close(tr.disp, g["disp_map"], atol=1e-4, rtol=1e-3, what="disp_map")
    close(tr.scalars[0].cpu(), g["loss"], atol=1e-5, rtol=1e-4, what="loss")
    close(tr.scalars[1].cpu(), g["loss_nll"], atol=1e-5, rtol=1e-4, what="loss_nll")
    close(tr.entropy.cpu().reshape(()), g["loss_entropy"], atol=1e-5, rtol=1e-4, what="entropy")
    rgb_t, disp_t, depth_t, ent_t = tr.rgb_map.clone(), tr.disp.clone(), tr.depth.clone(), tr.entropy.clone()

    # mask correction per netchunk: a one-set HIP launch of the chunk alone takes the same masks as the chunk's rays in the batch
    packed = O.pack_rays(H, W, focal, T(g["rays"])[0], T(g["rays"])[1], False, near, far)
    per = int(g["netchunk"]) // 128
    corr = None
    for c in range(2):
        s = slice(c * per, (c + 1) * per)
        tc = TR.Trainer(net, beta1=beta1)
        tc.forward_backward(H, W, focal, (rays[0, s], rays[1, s]), T(g["target"])[s].to(DEV), t_rand=t_rand[s].to(DEV), eps=chunks[c].to(DEV),
                            near=near, far=far, ndc=False)
        cc, _ = mask_corrected(net, p, packed[s], T(g["target"])[s], cfg, T(g["eps_alpha"][c]), T(g["eps_rgb"][c]), t_rand[s], beta1)
        w = per / n
        corr = {k: (None if v is None else w * v) for k, v in cc.items()} if corr is None else \
            {k: (None if v is None else corr[k] + w * v) for k, v in cc.items()}
    n_checked = 0
    for key, (off, cnt) in net.layout.items():
        gk = grad[off:off + cnt].double().numpy()
        if ("gradsample." + key) not in g:
            assert not gk.any(), f"{key} must get a zero gradient"
            continue
        idx = g["gradidx." + key]
        scale = max(float(g["gradabsmax." + key]), 1e-12)
        ref = g["gradsample." + key].astype(np.float64) + corr[key].reshape(-1)[idx]
        assert np.abs(gk[idx] - ref).max() <= G_TIGHT * scale + 1e-4 * np.abs(ref).max(), \
            f"gradsample {key}: {np.abs(gk[idx] - ref).max() / scale:.2e} of the largest entry"
        corr_norm = float(np.linalg.norm(corr[key].astype(np.float64)))
        assert abs(float(np.linalg.norm(gk)) - float(g["gradnorm." + key])) <= 2e-3 * float(g["gradnorm." + key]) + corr_norm, "gradnorm " + key
        n_checked += 1
    assert n_checked >= 30

    # the same batch through render() with explicit per-netchunk latents [C,K,1] / [C,K,3], under autograd: the same launch
    rgb, disp, depth, extras = cfnerf_amd.render(H, W, focal, chunk=int(g["chunk"]), rays=rays, near=near, far=far, t_rand=t_rand.to(DEV),
                                                 eps_alpha=T(g["eps_alpha"]), eps_rgb=T(g["eps_rgb"]), **kw_train)
    assert torch.equal(rgb, rgb_t) and torch.equal(depth, depth_t) and torch.equal(disp, disp_t)
    assert torch.equal(extras["loss_entropy"].mean().reshape(1), ent_t)
    (reference_kde_nll(rgb, T(g["target"]).to(DEV), 4) + beta1 * extras["loss_entropy"].mean()).backward()
    gd = net.flat.grad.detach().cpu()
    assert float((gd - grad).abs().max()) <= 1e-4 * float(grad.abs().max())


def test_g23a_render_netchunk_mode_matches_the_reference_draws():
    """G23a: render() in netchunk mode under the fixture's seed (implicit draws: two ray cuts, three latent pairs, two thrown-away
    noise draws) gives the reference's maps, entropy and - through autograd of the reference's loss - its gradients."""
    g = load("g23a_netchunk_draw_order")
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    _, kw_train, _, model, p, _ = build_model(cfg, int(g["seed"]), no_ndc=True, netchunk_per_gpu=int(g["netchunk"]),
                                              raw_noise_std=float(g["raw_noise_std"]), latent_draws="netchunk")
    net = model.module
    H, W, focal, near, far = int(g["H"]), int(g["W"]), float(g["focal"]), float(g["near"]), float(g["far"])
    torch.manual_seed(int(g["draw_seed"]))
    rgb, disp, depth, extras = cfnerf_amd.render(H, W, focal, chunk=int(g["chunk"]), rays=T(g["rays"]).to(DEV), near=near, far=far, **kw_train)
    close(rgb, g["rgb_map"], what="rgb_map")
    close(depth, g["depth_map"], what="depth_map")
    close(disp, g["disp_map"], atol=1e-4, rtol=1e-3, what="disp_map")
    ent = extras["loss_entropy"].mean()
    close(ent, g["loss_entropy"], atol=1e-5, rtol=1e-4, what="entropy")
    nll = reference_kde_nll(rgb, T(g["target"]).to(DEV), int(g["K"]))
    loss = nll + float(g["beta1"]) * ent
    close(loss, g["loss"], atol=1e-5, rtol=1e-4, what="loss")
    loss.backward()
    grad = net.flat.grad.detach().cpu()
    n = 0
    for key, (off, cnt) in net.layout.items():
        if ("grad." + key) not in g:
            continue
        ref = g["grad." + key].astype(np.float64).reshape(-1)
        scale = max(float(np.abs(ref).max()), 1e-12)
        err = float(np.abs(grad[off:off + cnt].double().numpy() - ref).max())
        assert err <= 1e-3 * scale + 1e-7, f"grad {key}: {err / scale:.2e} of the largest entry"
        n += 1
    assert n >= 30


def _rand_case(W, K, N, seed, precision="fp32", S=None):
    cfg = O.OracleCfg(netwidth=W, K_samples=K, h_alpha_size=64 if W == 512 else 32)
    _, kw_train, _, model, p, _ = build_model(cfg, seed)
    net = model.module
    if precision != "fp32":
        net.set_precision(precision)
    rng = np.random.default_rng(seed)
    rays, (H, Wd, focal) = fern_rays(rng, N)
    S = 128 if S is None else S
    target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32, device=DEV)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32, device=DEV)
    return cfg, kw_train, model, net, p, rays.to(DEV), (H, Wd, focal), target, t_rand, rng


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("W", [64, 256, 512])
def test_rows_equal_to_one_set_are_bit_identical_to_the_default_launch(W, K, precision):
    """CFNERF_F_EPS_ROWS with every row equal to one [K,4] set: forward maps, entropy and gradient equal the flag-off launch bit for
    bit (K = 16 takes the hardware-transcendental two-latent flow path)."""
    cfg, _, model, net, p, rays, (H, Wd, focal), target, t_rand, rng = _rand_case(W, K, 37, 300 + W + K, precision)
    eps = torch.tensor(rng.standard_normal((K, 4)), dtype=torch.float32, device=DEV)
    out = {}
    for form, e in (("set", eps), ("rows", eps.expand(37, K, 4).contiguous())):
        tr = TR.Trainer(net, beta1=0.01)
        g = tr.forward_backward(H, Wd, focal, rays, target, t_rand=t_rand, eps=e, ndc=True).clone()
        out[form] = (tr.rgb_map.clone(), tr.disp.clone(), tr.depth.clone(), tr.entropy.clone(), tr.scalars.clone(), g)
    for a, b, what in zip(out["set"], out["rows"], ("rgb", "disp", "depth", "entropy", "scalars", "grad")):
        assert torch.equal(a, b), what


def test_independent_rows_on_a_ragged_batch_match_the_oracle_per_ray():
    """Independent random latents for EVERY ray of a ragged batch (a 100-entry sample table: two tiles per ray, the second partly
    filled): each ray's maps equal the oracle run with that ray's latents, the entropy is the mean of the rays' entropies, and the
    gradient is the mean of the per-ray oracle gradients (each taken on the ReLU masks the HIP forward took for that ray's points) -
    this pins the per-ray row addressing of the forward and of tail_bwd against an independent reference."""
    from util_hip import hip_relu_masks
    K, N, S, beta1 = 4, 40, 100, 0.01
    cfg, kw_train, model, net, p, rays, (H, Wd, focal), target, _, rng = _rand_case(64, K, N, 77, S=S)
    t_vals = torch.linspace(0., 1., S)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32)
    rows = torch.tensor(rng.standard_normal((N, K, 4)), dtype=torch.float32)
    tr = TR.Trainer(net, beta1=beta1)
    grad = tr.forward_backward(H, Wd, focal, rays, target, t_rand=t_rand.to(DEV), eps=rows.to(DEV), t_vals=t_vals.to(DEV), ndc=True)
    grad = grad.cpu().double()
    _, masks = hip_relu_masks(net, N * S)
    packed = O.pack_rays(H, Wd, focal, rays[0].cpu(), rays[1].cpu(), True, 0., 1.)
    tgt = target.cpu()
    ents, ref = [], {}
    for i in range(N):
        s = slice(i, i + 1)
        with O.relu_override(masks={k: m[i * S:(i + 1) * S].cpu() for k, m in masks.items()}):
            scal, g, ret = O.train_step(p, packed[s], tgt[s], cfg, rows[i, :, 3:], rows[i, :, :3], t_rand[s], beta1, t_vals=t_vals)
        close(tr.rgb_map[s], ret["rgb_map"], what=f"rgb ray {i}")
        close(tr.depth[s], ret["depth_map"], what=f"depth ray {i}")
        ents.append(scal["loss_entropy"])
        for k, v in g.items():
            if v is not None:
                ref[k] = ref.get(k, 0) + v.double() / N
    close(tr.entropy.cpu().reshape(()), np.mean(ents), atol=1e-5, rtol=1e-4, what="entropy")
    n = 0
    for key, (off, cnt) in net.layout.items():
        if key not in ref:
            continue
        r = ref[key].reshape(-1)
        scale = max(float(r.abs().max()), 1e-12)
        err = float((grad[off:off + cnt] - r).abs().max())
        assert err <= 5e-4 * scale + 1e-7, f"grad {key}: {err / scale:.2e} of the largest entry"
        n += 1
    assert n >= 30


def test_trainer_step_with_implicit_netchunk_draws():
    """Trainer(latent_draws="netchunk").step() on one process with nothing explicit: t_rand and the latent pairs come from torch's CPU
    generator in the reference's order (draw_train_randomness) and reach the device - the step equals one given those draws."""
    K, N, netchunk, chunk = 4, 64, 1024, 32
    out = {}
    for form in ("implicit", "explicit"):
        cfg, _, model, net, p, rays, (H, Wd, focal), target, _, _ = _rand_case(64, K, N, 41)
        tr = TR.Trainer(net, beta1=0.01, latent_draws="netchunk", netchunk=netchunk, chunk=chunk)
        torch.manual_seed(4242)
        if form == "implicit":
            tr.step(H, Wd, focal, rays, target)
        else:
            t_rand, chunks = api.draw_train_randomness(N, 128, K, chunk, netchunk, 1.0)
            tr.forward_backward(H, Wd, focal, rays, target, t_rand=t_rand.to(DEV), eps_chunks=chunks)
        torch.cuda.synchronize()
        out[form] = (tr.rgb_map.clone(), tr.grad.clone(), tr.entropy.clone(), tr.last_eps_chunks.cpu().clone())
    a, b = out["implicit"], out["explicit"]
    assert a[3].shape == (api.netchunk_count(N, 128, netchunk, chunk), K, 4) and torch.equal(a[3], b[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_explicit_per_netchunk_latents_mean_the_same_in_both_modes_and_rows_are_counted():
    """Explicit eps_alpha [C,K,1] / eps_rgb [C,K,3] are per-netchunk latents whether the model is in "launch" or "netchunk" mode; a
    launch reading latent rows is refused unless it has one row per ray (per point); the eval branch refuses per-netchunk latents."""
    K, N = 4, 8
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    rng = np.random.default_rng(12)
    rays, (H, Wd, focal) = fern_rays(rng, N)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, 128)), dtype=torch.float32)
    ea, er = (torch.tensor(rng.standard_normal((4, K, d)), dtype=torch.float32) for d in (1, 3))
    res = {}
    for mode in ("launch", "netchunk"):
        _, kw_train, kw_test, model, p, _ = build_model(cfg, 13, netchunk_per_gpu=256, latent_draws=mode)
        with torch.no_grad():
            rgb, _, depth, extras = cfnerf_amd.render(H, Wd, focal, chunk=1024, rays=rays.to(DEV), t_rand=t_rand, eps_alpha=ea, eps_rgb=er, **kw_train)
        res[mode] = (rgb, depth, extras["loss_entropy"].mean())
        with pytest.raises(ValueError):
            cfnerf_amd.render(H, Wd, focal, chunk=1024, rays=rays.to(DEV), eps_alpha=ea, eps_rgb=er, **kw_test)
    assert all(torch.equal(x, y) for x, y in zip(res["launch"], res["netchunk"]))
    net = model.module
    net._sync()
    packed = torch.zeros(N, 11, device=DEV)
    packed[:, 5], packed[:, 7] = -1., 1.
    with pytest.raises(ValueError):
        api._render_fwd(net, packed, api.t_vals_table(DEV), None, torch.zeros(4, K, 4, device=DEV), L.F_TRAIN)
    with pytest.raises(ValueError):
        api._network_fwd(net, torch.zeros(16, 90, device=DEV), torch.zeros(4, K, 4, device=DEV), K, L.F_TRAIN)
    torch.cuda.synchronize()


def test_sliced_batch_with_netchunk_rows_matches_one_launch():
    """N_rand 8192 in 8 slices of 1024 (max_rays_per_launch) with the 16 netchunk pairs of the reference's defaults: the rows pointer
    moves with every slice, so the sliced step equals one 8192-ray launch up to summation order (the suite's slice bound)."""
    K, N = 4, 8192
    cfg, _, model, net, p, rays, (H, Wd, focal), target, t_rand, rng = _rand_case(64, K, N, 88)
    C_ = api.netchunk_count(N, 128, 65536, 1024 * 32)
    assert C_ == 16
    chunks = torch.tensor(rng.standard_normal((C_, K, 4)), dtype=torch.float32)
    out = {}
    for form, mx in (("sliced", 1024), ("one shot", None)):
        tr = TR.Trainer(net, beta1=0.01, max_rays_per_launch=mx, latent_draws="netchunk")
        g = tr.forward_backward(H, Wd, focal, rays, target, t_rand=t_rand, eps_chunks=chunks).clone()
        out[form] = (g, tr.rgb_map.clone(), tr.entropy.clone(), tr.scalars.clone(), tr.n_slices(N))
        net.release_workspace()
    a, b = out["sliced"], out["one shot"]
    assert a[4] == 8 and b[4] == 1
    assert torch.equal(a[1], b[1])
    assert float((a[0] - b[0]).abs().max()) <= 2e-5 * float(b[0].abs().max())
    close(a[2].cpu(), b[2].cpu(), atol=1e-5, rtol=1e-5, what="entropy")
    close(a[3].cpu(), b[3].cpu(), atol=1e-5, rtol=1e-5, what="scalars")


def test_unfused_seam_with_point_rows_trains_like_the_fused_path():
    """A caller's own network_query_fn in netchunk mode: the seam hands one latent row per point to NeRF_Flows.forward
    (cfnerf_network_fwd / _bwd with CFNERF_F_EPS_ROWS) and trains with the fused path's outputs and gradients."""
    K, N = 4, 8
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    rng = np.random.default_rng(5)
    rays, (H, Wd, focal) = fern_rays(rng, N)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, 128)), dtype=torch.float32)
    ea, er = (torch.tensor(rng.standard_normal((4, K, d)), dtype=torch.float32) for d in (1, 3))
    res = {}
    for form in ("fused", "unfused"):
        args, kw_train, _, model, p, _ = build_model(cfg, 9, netchunk_per_gpu=256, latent_draws="netchunk")
        kw = dict(kw_train)
        if form == "unfused":
            kw["network_query_fn"] = lambda inputs, viewdirs, fn, is_val, is_test: api.run_network(
                inputs, viewdirs, fn, is_val, is_test, args.embed_fn, args.embeddirs_fn, netchunk=256)
        rgb, disp, depth, extras = cfnerf_amd.render(H, Wd, focal, chunk=1024, rays=rays.to(DEV), t_rand=t_rand, eps_alpha=ea, eps_rgb=er, **kw)
        (rgb.square().mean() + 0.01 * extras["loss_entropy"].mean()).backward()
        res[form] = (rgb.detach(), extras["loss_entropy"].mean().detach(), model.module.flat.grad.detach().clone())
    close(res["unfused"][0], res["fused"][0], what="rgb")
    close(res["unfused"][1], res["fused"][1], atol=1e-5, rtol=1e-5, what="entropy")
    gu, gf = res["unfused"][2], res["fused"][2]
    assert float((gu - gf).abs().max()) <= 1e-4 * float(gf.abs().max())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_consume_identical_latents_and_their_shards_add_up():
    """World 2 on one GPU in netchunk mode, the ranks seeded differently: both use rank 0's latent pairs of the GLOBAL batch, and the
    exchanged (summed) shard gradient is the one-process gradient of the full batch with the same pairs."""
    from conftest import FORKSERVER_CTX as ctx
    assert ctx is not None
    import netchunk_workers
    spec = dict(W=64, K=4, N=64, seed=23, data_seed=6, beta1=0.01, netchunk=1024, chunk=32)
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=netchunk_workers.netchunk_trainer_rank, args=(r, 2, port, q, spec)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = {}
    for _ in range(2):
        rank, status, a, b, c = q.get(timeout=600)
        assert status == "ok", f"rank {rank} failed:\n{a}"
        got[rank] = (a, b, c)
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    (ch0, g0, f0), (ch1, g1, f1) = got[0], got[1]
    assert ch0.shape == (api.netchunk_count(64, 128, 1024, 32), 4, 4) == (8, 4, 4)
    assert np.array_equal(ch0, ch1) and np.array_equal(f0, f1)
    cfg = O.OracleCfg(netwidth=spec["W"], K_samples=spec["K"])
    _, _, _, model, _, _ = build_model(cfg, spec["seed"])
    rng = np.random.default_rng(spec["data_seed"])
    rays, (H, Wd, focal) = fern_rays(rng, spec["N"])
    target = torch.tensor(rng.uniform(0, 1, (spec["N"], 3)), dtype=torch.float32)
    t_rand = torch.tensor(rng.uniform(0, 1, (spec["N"], 128)), dtype=torch.float32)
    tr = TR.Trainer(model, beta1=spec["beta1"], latent_draws="netchunk", netchunk=spec["netchunk"], chunk=spec["chunk"])
    g = tr.forward_backward(H, Wd, focal, rays.to(DEV), target.to(DEV), t_rand=t_rand.to(DEV), eps_chunks=T(ch0)).cpu().numpy()
    assert np.abs(g0 - g).max() <= 2e-5 * np.abs(g).max()


def test_refusals():
    """cfnerf_render_eval refuses CFNERF_F_EPS_ROWS (the eval branch uses the fixed latents); the hierarchical extension refuses
    netchunk mode."""
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    _, kw_train, _, model, p, _ = build_model(cfg, 3, latent_draws="netchunk")
    net = model.module
    net._sync()
    N, S, K = 4, 128, 4
    rays = torch.zeros(N, 11, device=DEV)
    rays[:, 5] = -1.
    rays[:, 7] = 1.
    tv = api.t_vals_table(DEV)
    eps = torch.zeros(N, K, 4, device=DEV)
    kst = torch.empty(N, 8, device=DEV)
    rc = L.lib().cfnerf_render_eval(net.handle, L.ptr(rays), L.ptr(tv), L.ptr(eps), N, S, K, L.F_EPS_ROWS, None, L.ptr(kst), None, L.stream())
    assert rc == -1 and b"EPS_ROWS" in L.lib().cfnerf_last_error()
    with pytest.raises(NotImplementedError):
        api.render_rays(rays, network_query_fn=kw_train["network_query_fn"], network_fn=model, N_samples=64, N_importance=32, is_train=True,
                        uniformsample=False, hierarchical_extension=True)
    tr = TR.Trainer(net, latent_draws="netchunk")
    with pytest.raises(NotImplementedError):
        tr.forward_backward_hierarchical(4, 4, 1., (rays[:, :3], rays[:, 3:6]), torch.zeros(N, 3, device=DEV))
    torch.cuda.synchronize()
