"""-m gpu: ``cfnerf_sample_pdf`` (sample_pdf_kernel, the hierarchical resampler) called directly through the C ABI on synthetic weights and held
to the fp64 inverse-CDF bracket of tests/sample_pdf_common.py: every slot written, rows sorted, the coarse depths of ``cfnerf_sample_points``
in the output bit for bit (the header's "exactly as cfnerf_render_fwd samples them"), every resampled depth inside its bracket.  The
shapes cross the 64-entry chunk of the cumulative sum (its carry), reach S + N_importance = 1024 and go down to one inner weight; the weights
go from uniform to one-hot (the ``denom < 1e-5`` clamp on most bins); ``u`` holds exact 0 and 1, ties and CDF knots.  Then the entry's
refusals, and one end-to-end case through ``render_rays(hierarchical_extension=True)`` and ``Trainer.forward_backward_hierarchical``."""
import numpy as np
import pytest
import torch

import cfnerf_amd
import sample_pdf_common as SP
from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O
from util_hip import build_model, fern_rays

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def sample_pdf(rays, tv, tr, lindisp, w, u, flags=0):
    """the raw entry into a NaN-filled z_out [N,S+Ni] (device tensors in, device tensor out)"""
    N, S, K = w.shape
    Ni = u.shape[1]
    z = torch.full((N, S + Ni), NAN, device=DEV)
    L.check(L.lib().cfnerf_sample_pdf(L.ptr(rays), L.ptr(tv), L.ptr(tr), flags | (L.F_LINDISP if lindisp else 0), L.ptr(w), L.ptr(u), N, S, K, Ni,
                                      L.ptr(z), L.stream()), "cfnerf_sample_pdf")
    return z


def hip_cases(S, Ni, K):
    """every (weight kind, what, z_out, z_coarse, w, u) of a shape: geometries x weight kinds x u kinds, N_RAYS rays each"""
    rng = np.random.default_rng(1000 * S + Ni)
    N = SP.N_RAYS
    for ndc, lindisp, jitter, uniform in SP.geometries(S):
        rays = SP.make_rays(rng, N, ndc).to(DEV)
        tv = SP.make_t_vals(S, uniform).to(DEV)
        tr = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32).to(DEV) if jitter else None
        z_coarse = A._sample_points(rays, tv, tr, lindisp)[0].cpu()        # (held to the oracle by test_sample_points_kernel_vs_oracle_ragged)
        for wk in SP.W_KINDS:
            w = SP.make_weights(rng, wk, N, S, K)
            w_d = w.to(DEV)
            for uk in SP.U_KINDS:
                u = SP.make_u(rng, uk, N, Ni, z_coarse, w)
                z = sample_pdf(rays, tv, tr, lindisp, w_d, u.to(DEV))
                yield wk, f"S={S} Ni={Ni} K={K} ndc={ndc} lindisp={lindisp} jitter={jitter} table={uniform} w={wk} u={uk}", z, z_coarse, w, u


@pytest.mark.parametrize("S,Ni,K", SP.SHAPES)
def test_sample_pdf_kernel_inside_the_fp64_bracket(S, Ni, K):
    worst, wide = {}, {}
    for wk, what, z, z_coarse, w, u in hip_cases(S, Ni, K):
        r = SP.judge(z, z_coarse, w, u)
        worst[wk], wide[wk] = max(worst.get(wk, 0.0), r["max_cdf_err"]), max(wide.get(wk, 0.0), r["wide_share"])
        if r["n_nan"] or r["n_unsorted"] or r["n_coarse_missing"] or r["n_outside"]:
            print(f"{what}: {r}")
        SP.assert_judged(r, what)
    for wk in SP.W_KINDS:
        print(f"S={S} Ni={Ni} K={K} {wk}: max |F(z) - u| {worst[wk]:.3e}, widest share of wide brackets {wide[wk]:.4f}")


def test_sample_pdf_refusals_leave_z_out_untouched():
    """S < 3, S + N_importance > 1024, K < 1, N_importance < 1, N < 0, each NULL pointer, a mode flag of another entry: a negative status, a
    message, and not one store; N = 0 is fine; the entry works afterwards"""
    lib, s, P = L.lib(), L.stream(), L.ptr
    rng = np.random.default_rng(11)
    N, S, K, Ni = SP.N_RAYS, 66, 3, 63
    rays, tv = SP.make_rays(rng, N, False).to(DEV), SP.make_t_vals(S).to(DEV)
    tr = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32).to(DEV)
    w = SP.make_weights(rng, "surface", N, S, K)
    u = SP.make_u(rng, "rep4", N, Ni)
    w_d, u_d = w.to(DEV), u.to(DEV)
    z = torch.full((N, 1100), NAN, device=DEV)            # (room for every size asked for below)

    def call(rays_=rays, tv_=tv, w_=w_d, u_=u_d, z_=z, n=N, s_=S, k=K, ni=Ni, flags=0):
        return lib.cfnerf_sample_pdf(P(rays_), P(tv_), P(tr), flags, P(w_), P(u_), n, s_, k, ni, P(z_), s)

    for kw in (dict(s_=2), dict(s_=959, ni=66), dict(k=0), dict(ni=0), dict(n=-1), dict(rays_=None), dict(tv_=None), dict(w_=None), dict(u_=None),
               dict(z_=None), dict(flags=L.F_GEOMETRY), dict(flags=L.F_KSTATS_EXT), dict(flags=L.F_RAY_GRAD)):
        rc = call(**kw)
        msg = lib.cfnerf_last_error().decode(errors="replace")
        assert rc < 0 and len(msg) > 0, (kw, rc, msg)
        torch.cuda.synchronize()
        assert bool(torch.isnan(z).all()), kw
    assert call(n=0) == 0 and call(n=0, rays_=None, z_=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(z).all())
    z_coarse = A._sample_points(rays, tv, tr, False)[0]
    SP.check_sample_pdf(sample_pdf(rays, tv, tr, False, w_d, u_d), z_coarse, w, u, "after the refusals")


def test_python_paths_hand_the_kernel_their_rays_flags_jitter_and_weights():
    """End to end at S = 96, Ni = 70, W = 64, K = 3, N = 12 with lindisp, non-NDC rays, white_bkgd and perturb = 1: the ``z_vals`` of
    ``render_rays(hierarchical_extension=True)`` and ``Trainer.z_vals`` after ``forward_backward_hierarchical`` pass the bracket on the coarse
    weights of a plain ``render_rays(..., retweights=True)`` with the same ``t_rand`` and latents"""
    W, K, N, S, Ni = 64, 3, 12, 96, 70
    near, far = 2.0, 6.0
    cfg = O.OracleCfg(netwidth=W, K_samples=K)
    _, kw_train, _, model, _, _ = build_model(cfg, 77, no_ndc=True, lindisp=True, white_bkgd=True)
    net = model.module
    rng = np.random.default_rng(17)
    rays, (H, Wd, focal) = fern_rays(rng, N)
    packed = O.pack_rays(H, Wd, focal, rays[0], rays[1], False, near, far).to(DEV)
    t_rand = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32)
    u = torch.tensor(rng.uniform(0, 1, (N, Ni)), dtype=torch.float32)
    ea, er = torch.tensor(rng.standard_normal((K, 1)), dtype=torch.float32), torch.tensor(rng.standard_normal((K, 3)), dtype=torch.float32)
    target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32)
    kw = {k: v for k, v in kw_train.items() if k not in ("use_viewdirs", "N_samples", "N_importance", "perturb", "ndc")}
    assert kw["lindisp"] and kw["white_bkgd"] and kw["is_train"]
    tv = torch.linspace(0., 1., steps=S).to(DEV)
    with torch.no_grad():
        ret = cfnerf_amd.render_rays(packed, N_samples=S, N_importance=Ni, perturb=1., hierarchical_extension=True, t_rand=t_rand, u_fine=u,
                                     eps_alpha=ea, eps_rgb=er, **kw)
        coarse = cfnerf_amd.render_rays(packed, N_samples=S, perturb=1., t_rand=t_rand, eps_alpha=ea, eps_rgb=er, t_vals=tv, retweights=True, **kw)
    z_coarse = A._sample_points(packed, tv, t_rand.to(DEV), True)[0]
    assert ret["z_vals"].shape == (N, S + Ni) and coarse["weights"].shape == (N, S, K)
    SP.check_sample_pdf(ret["z_vals"], z_coarse, coarse["weights"], u, "render_rays(hierarchical_extension=True)")
    tr = TR.Trainer(net, beta1=0.01)
    tr.forward_backward_hierarchical(H, Wd, focal, rays.to(DEV), target.to(DEV), N_samples=S, N_importance=Ni, t_rand=t_rand.to(DEV), u_fine=u.to(DEV),
                                     eps=torch.cat([er, ea], -1).to(DEV), near=near, far=far, ndc=False, lindisp=True, white_bkgd=True, perturb=1.)
    with torch.no_grad():
        coarse_t = cfnerf_amd.render_rays(tr.packed.clone(), N_samples=S, perturb=1., t_rand=t_rand, eps_alpha=ea, eps_rgb=er, t_vals=tv,
                                          retweights=True, **kw)
    z_coarse_t = A._sample_points(tr.packed.clone(), tv, t_rand.to(DEV), True)[0]
    SP.check_sample_pdf(tr.z_vals, z_coarse_t, coarse_t["weights"], u, "Trainer.forward_backward_hierarchical")
