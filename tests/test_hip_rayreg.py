"""GPU: the ray regularisers (CFNERF_F_RAY_REG, cfnerf_rayreg.hip) - ray_reg_kernel against the fp64 yardstick of rayreg_common on the same
fp32-rounded inputs, the autograd node ``ray_regularizers``, and ``Trainer(distortion_lambda=, ray_entropy_lambda=)`` against the autograd route.

Bound of the kernel, per output tensor (scalars, d_weights, d_z): error = max abs error over the largest reference entry; at most 4 x the
error of fp32 torch evaluating the same closed forms on the same inputs on the device (the 4 covers a scan tree against torch's sequential
cumsum), and never less than 1e-6 allowed.  Both errors are computed here; measured values: profiles/r20_rayreg_errors.txt
(MI355X: the kernel 1e-8 .. 1.9e-7, fp32 torch 1e-8 .. 4.2e-7).  At S = 1 the entropy's gradient is ~1e-10 of its own terms - exactly 0 in
fp32, for the kernel and for torch alike: both "errors" are the whole (tiny) reference entry there, 1.0."""
import os

import numpy as np
import pytest
import torch

import cfnerf_amd
import cotangents_common as CC
import rayreg_common as R
from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O
from util_hip import build_model, grad_close_tight

pytestmark = pytest.mark.gpu
DEV = "cuda"
RECORD = os.environ.get("CFNERF_RAYREG_ERRORS")          # development aid: append every measured error to this file


def _record(case, what, err, torch32=None):
    if RECORD:
        with open(RECORD, "a") as f:
            f.write(f"{case:58s} {what:10s} kernel {err:.3e}" + (f"   torch fp32 {torch32:.3e}" if torch32 is not None else "") + "\n")


def kernel(w, z, rays=None, distortion=0., entropy=0., acc_min=0.1, n_total=0, want_z=True):
    """one launch on device tensors -> scalars [4], d_weights, d_z"""
    d_w = torch.full_like(w, float("nan"))
    d_z = torch.full_like(z, float("nan")) if want_z else None
    sc = torch.full((8,), float("nan"), device=DEV)
    L.ray_reg(w, z, d_w, sc, rays=rays, d_z=d_z, lambda_dist=distortion, lambda_ent=entropy, acc_min=acc_min, n_total=n_total)
    return {"scalars": sc[:4], "d_weights": d_w, "d_z": d_z, "tail": sc[4:]}


def _packed(N, near, far):
    rays = torch.zeros(N, 11)
    rays[:, 6], rays[:, 7] = near, far
    return rays


# (name, N, S, K, maker, rays, kwargs): every S of {1, 2, 63, 64, 65, 130}, K of {1, 3, 4, 5, 32}, N of {1, 3, 70} once, + (130, 5, 70)
def _random(N, S, K, seed, **kw):
    return R.composite_weights(N, S, K, seed, **kw)


def _tied(N, S, K, seed):
    w, z = R.composite_weights(N, S, K, seed)
    z[:, 1::3] = z[:, 0::3][:, :z[:, 1::3].shape[1]]             # every third depth repeats its predecessor
    return w, z


def _sparse(N, S, K, seed):
    w, z = R.composite_weights(N, S, K, seed)
    w[0] = 0                                                       # an all-zero ray
    w[1] *= 1e-3 / w[1].sum(0, keepdim=True)                       # a ray at A = 1e-3
    return w, z


CASES = [
    ("random S1 K1 N1", 1, 1, 1, _random, None, {}),
    ("random S2 K3 N3 near-far", 3, 2, 3, _random, (2., 6.), {}),
    ("random S63 K4 N3 n_total=3N", 3, 63, 4, _random, (2., 6.), dict(n_total=9)),
    ("random S64 K5 N3", 3, 64, 5, _random, None, {}),
    ("random S65 K32 N3 near-far", 3, 65, 32, _random, (2., 6.), {}),
    ("random S130 K5 N70 near-far", 70, 130, 5, _random, (2., 6.), {}),
    ("peaked S130 K3 N3", 3, 130, 3, R.peaked_weights, None, {}),
    ("tied S65 K4 N3 near-far", 3, 65, 4, _tied, (2., 6.), {}),
    ("zero + 1e-3 rays S130 K4 N3 near-far", 3, 130, 4, _sparse, (2., 6.), {}),
    ("zero + 1e-3 rays S64 K3 N3 acc_min=0", 3, 64, 3, _sparse, None, dict(acc_min=0.0)),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_kernel_against_the_fp64_closed_forms(case):
    name, N, S, K, make, rays, kw = case
    lam = dict(distortion=0.7, entropy=0.3)
    acc_min = kw.get("acc_min", 0.1)
    w64, z64 = make(N, S, K, seed=len(name) + S)
    w32, z32 = w64.float(), z64.float()
    w64, z64 = w32.double(), z32.double()                          # the yardstick sees the fp32-rounded inputs
    if acc_min > 0:
        assert R.mask_margin(w64, acc_min) >= 1e-3, "a (ray, latent) sits on the mask threshold: fp32 and fp64 may disagree"
    else:                                                          # acc_min = 0: the margin is the all-zero ray's exact 0 (0 > 0 is false in both)
        A64 = w64.sum(1)
        assert bool(((A64 == 0) | (A64 >= 1e-3 - 1e-9)).all())
    ref = R.closed_forms(w64, z64, rays, acc_min=acc_min, n_total=kw.get("n_total"), **lam)
    wd, zd = w32.to(DEV), z32.to(DEV)
    t32 = R.closed_forms(wd, zd, rays, acc_min=acc_min, n_total=kw.get("n_total"), **lam)
    packed = None if rays is None else _packed(N, *rays).to(DEV)
    got = kernel(wd, zd, packed, acc_min=acc_min, n_total=kw.get("n_total", 0), **lam)
    assert bool((got["tail"] == 0).all())
    again = kernel(wd, zd, packed, acc_min=acc_min, n_total=kw.get("n_total", 0), **lam)
    for k in ("scalars", "d_weights", "d_z"):
        assert torch.equal(got[k], again[k]), k + ": two runs differ"
        assert bool(torch.isfinite(got[k]).all()), k
        if float(ref[k].abs().max()) == 0.0:                        # (S = 1: no interval, d_z is exactly zero)
            assert float(got[k].abs().max()) == 0.0, k
            continue
        e_k, e_t = R.rel_err(got[k], ref[k]), R.rel_err(t32[k], ref[k])
        _record(name, k, e_k, e_t)
        assert e_k <= max(4 * e_t, 1e-6), f"{name} {k}: kernel {e_k:.3e}, torch fp32 {e_t:.3e}"


def test_one_lambda_at_zero_gives_the_other_terms_bits():
    N, S, K = 3, 130, 5
    w64, z64 = R.composite_weights(N, S, K, seed=5)
    w, z, rays = w64.float().to(DEV), z64.float().to(DEV), _packed(N, 2., 6.).to(DEV)
    both = kernel(w, z, rays, 0.7, 0.3)
    d = kernel(w, z, rays, 0.7, 0.0)
    e = kernel(w, z, rays, 0.0, 0.3)
    # a term alone is that term of the yardstick (so "the other term's gradient alone" is not vacuous) ...
    r_d = R.closed_forms(w.double(), z.double(), (2., 6.), 0.7, 0.0)
    r_e = R.closed_forms(w.double(), z.double(), (2., 6.), 0.0, 0.3)
    assert R.rel_err(d["d_weights"], r_d["d_weights"]) <= 1e-5 and R.rel_err(e["d_weights"], r_e["d_weights"]) <= 1e-5
    assert float(d["scalars"][2]) == 0.0 and float(e["scalars"][1]) == 0.0 and float(e["d_z"].abs().max()) == 0.0
    assert torch.equal(d["d_z"], both["d_z"])
    # ... and the two-term call is their sum, to 1 ulp of the larger
    s = d["d_weights"].double() + e["d_weights"].double()
    big = torch.maximum(torch.maximum(d["d_weights"].abs(), e["d_weights"].abs()), both["d_weights"].abs())
    ulp = torch.nextafter(big, torch.full_like(big, float("inf"))) - big
    assert bool(((both["d_weights"].double() - s).abs() <= ulp.double()).all())
    assert float(both["scalars"][1]) == float(d["scalars"][1]) and float(both["scalars"][2]) == float(e["scalars"][2])


def test_ray_regularizers_backward_is_the_kernels_buffers_times_the_cotangent():
    N, S, K = 3, 65, 4
    w64, z64 = R.composite_weights(N, S, K, seed=11)
    rays = _packed(N, 2., 6.).to(DEV)
    w = w64.float().to(DEV).requires_grad_()
    z = z64.float().to(DEV).requires_grad_()
    k = kernel(w.detach(), z.detach(), rays, 0.7, 0.3, n_total=9)
    reg, parts = cfnerf_amd.ray_regularizers(w, z, rays=rays, distortion=0.7, entropy=0.3, n_total=9)
    assert reg.dim() == 0 and reg.grad_fn is not None and set(parts) == {"dist", "ent", "frac"}
    assert float(reg.detach()) == float(k["scalars"][0])
    assert [float(parts[n]) for n in ("dist", "ent", "frac")] == [float(v) for v in k["scalars"][1:]]
    (0.37 * reg).backward()
    assert torch.equal(w.grad, k["d_weights"] * torch.tensor(0.37, device=DEV))
    assert torch.equal(z.grad, k["d_z"] * torch.tensor(0.37, device=DEV))
    # (near, far) in place of the packed rays; z_vals without requires_grad gets no gradient
    w2 = w.detach().clone().requires_grad_()
    reg2, _ = cfnerf_amd.ray_regularizers(w2, z.detach(), rays=(2., 6.), distortion=0.7, entropy=0.3, n_total=9)
    reg2.backward()
    assert float(reg2.detach()) == float(reg.detach()) and torch.equal(w2.grad, k["d_weights"])
    # on the seam: through raw2outputs to raw
    raw = torch.randn(N, S, K, 4, device=DEV).requires_grad_()
    _, _, weights, _ = cfnerf_amd.raw2outputs(raw, z.detach(), torch.randn(N, 3, device=DEV))
    assert weights.grad_fn is not None
    cfnerf_amd.ray_regularizers(weights, z.detach(), rays=rays, distortion=0.7, entropy=0.3)[0].backward()
    assert raw.grad is not None and float(raw.grad[..., 3].abs().max()) > 0 and bool(torch.isfinite(raw.grad).all())


def test_model_entry_points_refuse_the_bit_by_name():
    cfg = O.OracleCfg(netwidth=64, K_samples=4)
    _, _, _, model, _, _ = build_model(cfg, 3)
    net, lib = model.module, L.lib()
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    rc = lib.cfnerf_render_fwd(net.handle, None, None, None, None, None, 4, 8, 4, L.F_RAY_REG, None, None, None, None, None, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_F_RAY_REG" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 8, 4, L.F_RAY_REG, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_F_RAY_REG" in err(), err()
    rc = lib.cfnerf_network_fwd(net.handle, None, None, 4, 4, L.F_RAY_REG, None, None, L.stream())
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_F_RAY_REG" in err(), err()


# ---------------------------------------------------------------- Trainer
LAM = dict(distortion_lambda=0.01, ray_entropy_lambda=0.001)
_STEP = {}


def _step():
    """netwidth 64, K = 4, 16 rays x S = 128: the model, the step's inputs, and the unsliced Trainer step with the regularisers - shared"""
    if not _STEP:
        N, S, K = 16, 128, 4
        cfg = O.OracleCfg(netwidth=64, K_samples=K)
        _, _, _, model, _, _ = build_model(cfg, 91)
        rng = np.random.default_rng(91)
        rb = CC.random_rays(rng, N)
        rays = torch.stack([rb[:, 0:3], rb[:, 3:6]], 0).to(DEV)
        target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32).to(DEV)
        kw = dict(t_rand=torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32).to(DEV),
                  eps=torch.tensor(rng.standard_normal((K, 4)), dtype=torch.float32).to(DEV), near=2., far=6., ndc=False)
        tr = TR.Trainer(model.module, beta1=0.05, ray_grad=True, **LAM)
        grad = tr.forward_backward(4, 4, 3., rays, target, **kw).clone()
        _STEP.update(N=N, S=S, K=K, model=model, net=model.module, rays=rays, target=target, kw=kw, grad=grad, scalars=tr.scalars.clone(),
                     reg=tr.reg_scalars.clone(), d_z=tr.d_z.clone(), packed=tr.packed.clone())
    return _STEP


def _per_tensor(net, g, ref, what):
    for key, (off, cnt) in net.layout.items():
        grad_close_tight(g[off:off + cnt], ref[off:off + cnt].cpu().numpy(), f"{what} {key}", tol=CC.G_TIGHT)


def test_trainer_with_lambdas_against_the_autograd_route():
    c = _step()
    net, N, S, K, kw = c["net"], c["N"], c["S"], c["K"], c["kw"]
    net.flat.grad = None
    ret = cfnerf_amd.render_rays(c["packed"], c["model"], None, S, True, False, perturb=1., t_rand=kw["t_rand"], eps_alpha=kw["eps"][:, 3:4],
                                 eps_rgb=kw["eps"][:, 0:3], retweights=True)
    z, _ = A._sample_points(c["packed"], cfnerf_amd.t_vals_table(DEV), kw["t_rand"], False)
    loss = O.train_loss(ret["rgb_map"], c["target"], ret["loss_entropy"].mean(), K, 0.05)["loss"]
    reg, parts = cfnerf_amd.ray_regularizers(ret["weights"], z, rays=c["packed"], distortion=LAM["distortion_lambda"],
                                             entropy=LAM["ray_entropy_lambda"])
    (loss + reg).backward()
    g_auto = net.flat.grad.clone()
    net.flat.grad = None
    _per_tensor(net, c["grad"], g_auto, "Trainer vs autograd")
    want = torch.stack([reg.detach(), parts["dist"], parts["ent"], parts["frac"]])
    assert torch.equal(c["reg"], want), (c["reg"], want)
    assert float(c["reg"][0]) > 0 and float(c["reg"][1]) > 0 and float(c["reg"][2]) > 0
    total = float((loss + reg).detach())
    assert abs(float(c["scalars"][0]) - total) <= 1e-5 * abs(total)
    # the regularisers moved the gradient (without them this comparison would hold for any Trainer)
    plain = TR.Trainer(net, beta1=0.05)
    g_plain = plain.forward_backward(4, 4, 3., c["rays"], c["target"], **kw)
    assert float((g_plain - c["grad"]).abs().max()) > 1e-3 * float(c["grad"].abs().max())


def test_trainer_ray_grad_adds_the_direct_depth_gradient():
    """Trainer.d_z against the autograd route's z_vals.grad: the explicit-depth launch, where z_vals is a leaf of both terms"""
    c = _step()
    net, S, K, kw = c["net"], c["S"], c["K"], c["kw"]
    z, _ = A._sample_points(c["packed"], cfnerf_amd.t_vals_table(DEV), kw["t_rand"], False)
    zl = z.clone().requires_grad_()
    net.flat.grad = None
    eps = kw["eps"]
    net._sync()
    o = A._RenderFn.apply(net.flat, net, c["packed"], cfnerf_amd.t_vals_table(DEV), None, eps, L.F_TRAIN, False, zl, True)
    rgb_map, ent, weights = o[0], o[3], o[6]
    loss = O.train_loss(rgb_map, c["target"], ent, K, 0.05)["loss"]
    reg, _ = cfnerf_amd.ray_regularizers(weights, zl, rays=c["packed"], distortion=LAM["distortion_lambda"], entropy=LAM["ray_entropy_lambda"])
    (loss + reg).backward()
    net.flat.grad = None
    grad_close_tight(c["d_z"], zl.grad.cpu().numpy(), "Trainer.d_z vs autograd", tol=CC.G_TIGHT)
    off = TR.Trainer(net, beta1=0.05, ray_grad=True)
    off.forward_backward(4, 4, 3., c["rays"], c["target"], **kw)
    assert float((off.d_z - c["d_z"]).abs().max()) > 0


def test_trainer_slices_against_the_unsliced_step():
    c = _step()
    sl = TR.Trainer(c["net"], beta1=0.05, ray_grad=True, max_rays_per_launch=8, **LAM)
    g = sl.forward_backward(4, 4, 3., c["rays"], c["target"], **c["kw"])
    assert sl.n_slices(c["N"]) == 2
    _per_tensor(c["net"], g, c["grad"], "Trainer 2 slices vs 1")
    grad_close_tight(sl.d_z, c["d_z"].cpu().numpy(), "Trainer 2 slices vs 1 d_z", tol=CC.G_TIGHT)
    assert torch.allclose(sl.reg_scalars, c["reg"], rtol=1e-6, atol=0), (sl.reg_scalars, c["reg"])
    assert abs(float(sl.scalars[0]) - float(c["scalars"][0])) <= 1e-5 * abs(float(c["scalars"][0]))


def test_trainer_without_lambdas_is_bit_equal_to_the_parents_argument_list():
    c = _step()
    net, kw = c["net"], c["kw"]
    a = TR.Trainer(net, 5e-4, 250, 0.05, 1, None, 0, False, False, False, None, "launch", 1024 * 64, 1024 * 32, 0.0, False, False)
    ga, sa = a.forward_backward(4, 4, 3., c["rays"], c["target"], **kw).clone(), a.scalars.clone()
    b = TR.Trainer(net, beta1=0.05, distortion_lambda=0., ray_entropy_lambda=0.)
    gb = b.forward_backward(4, 4, 3., c["rays"], c["target"], **kw)
    assert torch.equal(ga, gb) and torch.equal(sa, b.scalars)
    assert b._reg_n is None and b.gbuf.numel() == a.gbuf.numel() and float(b.reg_scalars.abs().max()) == 0.0


def test_step_hierarchical_with_lambdas_raises():
    c = _step()
    tr = TR.Trainer(c["net"], beta1=0.05, **LAM)
    with pytest.raises(NotImplementedError, match="distortion_lambda"):
        tr.step_hierarchical(4, 4, 3., c["rays"], c["target"], near=2., far=6., ndc=False)
    with pytest.raises(NotImplementedError, match="distortion_lambda"):
        tr.forward_backward_hierarchical(4, 4, 3., c["rays"], c["target"], near=2., far=6., ndc=False)
