"""-m gpu: the render is differentiable in its latents, like the reference's (eps.mul(std).add_(mean), MOD:239,251, is an ordinary autograd
line): cfnerf_render_fwd / cfnerf_network_fwd with CFNERF_F_STASH | CFNERF_F_EPS_GRAD, then the backward writes d_eps [K,4] and d_eps_rows
[n,K,4] behind the blocks it already writes (tail_eps_kernel, flows_eps_kernel, reduce_eps_kernel).  Held to the fp64 oracle's autograd on the
ReLU masks the HIP forward took, to the G28 fixtures of the real reference, and to "nothing else moved".

Every measured error is appended to the file named by CFNERF_EPSGRAD_ERRORS (how profiles/r18_epsgrad_errors.txt is made)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cfnerf_amd
from cfnerf_amd import _lib as L
from cfnerf_amd import api
from cfnerf_amd import evaluate as E
from cfnerf_amd import latents as LT
from cfnerf_amd import train as TR
from oracle import cfnerf_oracle as O

import cotangents_common as CC
import epsgrad_common as EC
from util_hip import build_model, close, grad_close_tight, hip_relu_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (W, K, N, S, options, first model seed tried)                                        what it covers
CASES = [
    (64, 4, 1, 2, {}, 2100),                                                          # 62 idle lanes
    (64, 3, 5, 64, {}, 2110),                                                         # odd K, dead waves in the last workgroup
    (128, 4, 3, 65, {}, 2120),                                                        # the accumulators span two chunks, ragged
    (64, 128, 1, 64, {}, 2161),                                                       # four k-parts, K beyond one lane pass
    (64, 65, 2, 70, {}, 2150),                                                        # uneven parts
    (64, 5, 1, 64, {}, 2190),                                                         # four parts, the last one empty
    (192, 4, 3, 64, dict(lindisp=True, white_bkgd=True, perturb=False, near=0.2), 2160),
    (256, 4, 4, 128, dict(bf16x3=True), 2170),
    (128, 4, 6, 66, dict(rows=True), 2180),                                           # CFNERF_F_EPS_ROWS, different rows per ray
]
IDS = [f"W{w}-K{k}-N{n}-S{s}" + "".join(f"-{a}" for a in opt) for w, k, n, s, opt, _ in CASES]
ALL = 2                                                                               # the case that also runs with COTANGENTS and RAY_GRAD together
# the unfused seam: (W, K, P, options, model seed)
SEAM = [
    (64, 3, 1, {}, 2200),
    (64, 3, 70, {}, 2201),
    (64, 65, 1, {}, 2202),
    (64, 65, 70, dict(rows=True), 2203),
    (128, 4, 70, dict(rows=True, input_grad=True), 2204),
]
SEAM_IDS = [f"W{w}-K{k}-P{p}" + "".join(f"-{a}" for a in opt) for w, k, p, opt, _ in SEAM]


def _record(case, what, rel):
    print(f"{case}: {what} max error {rel:.3e} of the largest entry")
    path = os.environ.get("CFNERF_EPSGRAD_ERRORS")
    if path:
        with open(path, "a") as f:
            f.write(f"{case:60s} {what:40s} {rel:.3e}\n")


def _hold(hip, ref, case, what):
    """a latent gradient against its reference, by column block (rgb, alpha), with the bound of the base-Gaussian gradients"""
    for (cname, g), (_, r) in zip(EC.columns(hip.detach().cpu()), EC.columns(ref)):
        _record(case, f"{what} {cname}", CC.rel(g, r))
    for (cname, g), (_, r) in zip(EC.columns(hip.detach().cpu()), EC.columns(ref)):
        grad_close_tight(g, r, f"{case} {what} {cname}")


# ---------------------------------------------------------------- the C ABI, fused
def abi_fwd(net, inp, extra=L.FLAG_EPS_GRAD):
    """cfnerf_render_fwd (STASH | extra) at the C ABI, every output asked for"""
    rays = inp["rays"].to(DEV).contiguous()
    N, S = inp["z"].shape
    K = inp["cfg"].K_samples
    eps = torch.cat([inp["er"], inp["ea"]], -1).to(DEV).contiguous()
    flags = L.F_TRAIN | L.F_STASH | extra | (L.F_LINDISP if inp["lindisp"] else 0) | (L.F_WHITE_BKGD if inp["wb"] else 0)
    net._sync()
    net.ensure_workspace(N, S, K)
    tr = None if inp["t_rand"] is None else inp["t_rand"].to(DEV).contiguous()
    o = api._render_fwd(net, rays, inp["tv"].to(DEV).contiguous(), tr, eps, flags, None, raw=True, weights=True)
    return dict(o=o, gen=L.lib().cfnerf_model_stash_generation(net.handle), eps=eps, extra=extra, NS=(N, S))


def abi_bwd(net, inp, f, use, bwd="cfnerf_render_bwd", buf=None, ent_scale=1.0):
    """the backward of the forward `f` with the cotangents named by `use`; the blocks of cfnerf.h as views of the one buffer"""
    lib, n = L.lib(), net.n_params
    N, S = f["NS"]
    K = inp["cfg"].K_samples
    t = {k: v.to(DEV).contiguous() for k, v in inp["cot"].items()}
    G = t["G"] if "G" in use else torch.zeros(N, 3, K, device=DEV)
    pick = lambda c: t[c] if c in use else None
    d_ent = torch.full((1,), CC.C_ENT * ent_scale, device=DEV) if "ent" in use else None
    ray_grad, eps_grad = bool(f["extra"] & L.F_RAY_GRAD), bool(f["extra"] & L.FLAG_EPS_GRAD)
    r_off, z_off, total = L.ray_grad_offsets(n, N, S) if ray_grad else (n, n, n)
    e_off, er_off, total = L.eps_grad_offsets(total, N, K) if eps_grad else (total, total, total)
    if buf is None:
        buf = torch.full((total + 64,), float("nan"), device=DEV)       # (64 floats past the end: never written)
    if f["extra"] & L.F_COTANGENTS:
        desc = L.cotangents(G, pick("Gq"), pick("Gw"), pick("Gr"))
        first = L.cotangents_arg(desc)
    else:
        assert not any(c in use for c in ("Gq", "Gw", "Gr"))
        first = L.ptr(G)
    L.check(getattr(lib, bwd)(net.handle, f["gen"], first, L.ptr(pick("Gd")), L.ptr(d_ent), L.ptr(buf), L.stream()), bwd)
    torch.cuda.synchronize()
    out = dict(buf=buf, grad=buf[:n], total=total)
    if ray_grad:
        out.update(d_rays=buf[r_off:r_off + N * 11].view(N, 11), d_z=buf[z_off:z_off + N * S].view(N, S))
    if eps_grad:
        out.update(d_eps=buf[e_off:e_off + K * 4].view(K, 4), rows=buf[er_off:er_off + N * K * 4].view(N, K, 4), pad=buf[e_off + K * 4:er_off])
    return out


@functools.lru_cache(maxsize=None)
def _case(i):
    """The model of case i (seed picked on the CPU), the ReLU masks its HIP forward takes, the fp64 oracle's latent gradients on those masks with
    their calibration, and the HIP backward with and without the flag: computed once, shared by the tests below (none changes what is kept)."""
    W, K, N, S, opt, base = CASES[i]
    inp = CC.make_inputs(W, K, N, S, {}, opt, seed=2800 + i)
    seed = CC.pick_seed(inp, base)
    _, _, _, model, p, _ = build_model(inp["cfg"], seed)
    net = model.module
    if opt.get("bf16x3"):
        net.set_precision("bf16x3")
    f = abi_fwd(net, inp)
    torch.cuda.synchronize()
    _, masks = hip_relu_masks(net, N * S)
    rec = CC.oracle_records(p, inp, torch.float64)
    n_flips = sum(int(((rec[k] > 0).float() != masks[k]).sum()) for k in rec)
    units = sum(v.numel() for v in rec.values())
    assert n_flips <= max(2, CC.FLIP_FRAC * units), f"{n_flips} of {units} ReLU masks differ"
    ref = {"plain": EC.reference(lambda dt: EC.render_rows(p, inp, masks, dt, EC.USES["plain"]))}
    if i == ALL:
        ref["all"] = EC.reference(lambda dt: EC.render_rows(p, inp, masks, dt, EC.USES["all"]))
    hip = abi_bwd(net, inp, f, EC.USES["plain"])
    f0 = abi_fwd(net, inp, extra=0)
    hip0 = abi_bwd(net, inp, f0, EC.USES["plain"])
    return dict(inp=inp, net=net, model=model, p=p, masks=masks, ref=ref, f=f, f0=f0, hip=hip, hip0=hip0, eps=f["eps"])


# ---------------------------------------------------------------- 1. against the fp64 oracle, on the masks the HIP forward took
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_latent_gradient_vs_fp64_oracle_autograd(i):
    """d_eps and d_eps_rows of the plain train loss (rgb_map, depth_map, 0.3 entropy).  The rows reference is the oracle called per ray with that
    ray's row (a shared set: identical rows).  Bound: grad_close_tight as the base-Gaussian gradients are held - fp32_noise = the fp32 CPU
    oracle's own distance from fp64 on these inputs, sum_abs = std * sum |d z0| per entry - by column block (rgb, alpha)."""
    c = _case(i)
    _hold(c["hip"]["d_eps"], c["ref"]["plain"]["d_eps"], IDS[i], "d_eps")
    _hold(c["hip"]["rows"], c["ref"]["plain"]["rows"], IDS[i], "d_eps_rows")


def test_latent_gradient_with_cotangents_and_ray_grad_together():
    """COTANGENTS (disp, weights, raw) | RAY_GRAD | EPS_GRAD in one stash: the latent gradient of the loss over every output, and the parameter
    gradient, d_rays and d_z bit for bit what they are without EPS_GRAD"""
    c = _case(ALL)
    net, inp = c["net"], c["inp"]
    both = L.F_COTANGENTS | L.F_RAY_GRAD
    hip = abi_bwd(net, inp, abi_fwd(net, inp, extra=both | L.FLAG_EPS_GRAD), EC.USES["all"])
    _hold(hip["d_eps"], c["ref"]["all"]["d_eps"], IDS[ALL], "all+ray_grad d_eps")
    _hold(hip["rows"], c["ref"]["all"]["rows"], IDS[ALL], "all+ray_grad d_eps_rows")
    plain = abi_bwd(net, inp, abi_fwd(net, inp, extra=both), EC.USES["all"])
    for k in ("grad", "d_rays", "d_z"):
        assert torch.equal(hip[k], plain[k]), k + " changed with CFNERF_F_EPS_GRAD"
    # cotangent stash, optional members NULL: tail_eps_kernel with a null TailCot is the plain loss's latent gradient
    nul = abi_bwd(net, inp, abi_fwd(net, inp, extra=L.F_COTANGENTS | L.FLAG_EPS_GRAD), EC.USES["plain"])
    assert torch.equal(nul["d_eps"], c["hip"]["d_eps"]) and torch.equal(nul["rows"], c["hip"]["rows"])


# ---------------------------------------------------------------- 3. d_eps is the sum of the rows
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_d_eps_is_the_fp64_sum_of_the_rows_rounded_once(i):
    h = _case(i)["hip"]
    want = h["rows"].double().sum(0).float()
    ulp = torch.maximum(want.abs(), torch.tensor(1e-37, device=DEV)).log2().floor().exp2() * 2.0 ** -23
    assert bool(((h["d_eps"] - want).abs() <= ulp).all()), float(((h["d_eps"] - want).abs() / ulp).max())
    assert bool(torch.isnan(h["pad"]).all()) and bool(torch.isnan(h["buf"][h["total"]:]).all()), "a pad float was written"
    n = _case(i)["net"].n_params
    assert bool(torch.isnan(h["buf"][n:(n + 63) // 64 * 64]).all())


# ---------------------------------------------------------------- 4. the identity with the base-Gaussian means
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sum_over_k_without_the_direct_term_is_the_mean_gradient(i):
    """sum_k (d_eps[k,3] - direct) / alpha_std = d loss / d alpha_mean, the colour columns likewise with rgb_mean: against the fp64 oracle's
    gradient of the means, under the bound of test 1 (sum_abs = sum |d z0|)"""
    c = _case(i)
    p, ref = c["p"], c["ref"]["plain"]
    d = c["hip"]["d_eps"].detach().cpu().double() - EC.direct_term(c["eps"].cpu(), CC.C_ENT)
    std = torch.cat([p["rgb_std"], p["alpha_std"]]).double()
    got = (d / std).sum(0)
    for key, sl in (("alpha_mean", slice(3, 4)), ("rgb_mean", slice(0, 3))):
        _record(IDS[i], "identity " + key, CC.rel(got[sl], ref["base"][key]))
        grad_close_tight(got[sl], ref["base"][key], f"{IDS[i]} identity grad {key}")
    # ... and the library's own gradient of the means, from the same launch
    lay = c["net"].layout
    for key, sl in (("alpha_mean", slice(3, 4)), ("rgb_mean", slice(0, 3))):
        off, cnt = lay[key]
        grad_close_tight(c["hip"]["grad"][off:off + cnt], ref["base"][key], f"{IDS[i]} grad {key}")


# ---------------------------------------------------------------- 5. / 6. nothing else moved; reproducible
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_nothing_else_moved_and_two_runs_are_bit_equal(i):
    c = _case(i)
    net, inp, lib = c["net"], c["inp"], L.lib()
    N, S = inp["z"].shape
    for k in ("rgb_map", "disp_map", "depth_map", "raw", "weights", "entropy"):
        assert torch.equal(c["f"]["o"][k], c["f0"]["o"][k]), k + " changed with CFNERF_F_EPS_GRAD"
    assert torch.equal(c["hip"]["grad"], c["hip0"]["grad"]), "the parameter gradient changed with CFNERF_F_EPS_GRAD"
    assert net._ws.numel() == lib.cfnerf_workspace_bytes(C.byref(net.cfg), N, S, inp["cfg"].K_samples)
    again = abi_bwd(net, inp, abi_fwd(net, inp), EC.USES["plain"])
    for k in ("grad", "d_eps", "rows"):
        assert torch.equal(again[k], c["hip"][k]), k + " is not bit-reproducible"
    # _accumulate ADDS the parameter gradient and OVERWRITES the two latent blocks
    acc = abi_bwd(net, inp, abi_fwd(net, inp), EC.USES["plain"], bwd="cfnerf_render_bwd_accumulate", buf=again["buf"].clone())
    close(acc["grad"], 2 * again["grad"].double(), atol=1e-12, rtol=1e-6, what="accumulated parameter gradient")
    assert torch.equal(acc["d_eps"], again["d_eps"]) and torch.equal(acc["rows"], again["rows"])


# ---------------------------------------------------------------- 7. slices
@pytest.mark.parametrize("i", [7, 8], ids=[IDS[7], IDS[8]])
def test_two_slices_sum_to_the_one_shot_total(i):
    """cfnerf_render_bwd for the first half of the rays, cfnerf_render_bwd_accumulate for the second, each with d_entropy / 2: the per-slice
    d_eps add up to the one launch's (not bit for bit: the k-split depends on N), the slices' rows are the one launch's rows"""
    c = _case(i)
    net, inp = c["net"], c["inp"]
    N = inp["z"].shape[0]
    h = N // 2
    total, rows = 0, []
    for j, sl in enumerate((slice(0, h), slice(h, N))):
        part = dict(inp, rays=inp["rays"][sl], t_rand=inp["t_rand"][sl], z=inp["z"][sl], cot={k: v[sl] for k, v in inp["cot"].items()})
        if inp["rows"]:
            part.update(ea=inp["ea"][sl], er=inp["er"][sl])
        o = abi_bwd(net, part, abi_fwd(net, part), EC.USES["plain"], bwd="cfnerf_render_bwd" if j == 0 else "cfnerf_render_bwd_accumulate",
                    ent_scale=0.5)
        total = total + o["d_eps"].double()
        rows.append(o["rows"].clone())
    _hold(total.float(), c["ref"]["plain"]["d_eps"], IDS[i], "two slices d_eps")
    _hold(torch.cat(rows, 0), c["ref"]["plain"]["rows"], IDS[i], "two slices d_eps_rows")
    one = c["ref"]["plain"]["d_eps"]
    ref = c["hip"]["d_eps"].detach().cpu().double()
    ref.fp32_noise, ref.sum_abs, ref.global_scale = one.fp32_noise, one.sum_abs, one.global_scale
    _hold(total.float(), ref, IDS[i], "two slices vs one launch d_eps")


# ---------------------------------------------------------------- the unfused seam
def _seam_inputs(W, K, P, opt, seed):
    cfg = O.OracleCfg(netwidth=W, K_samples=K)
    rng = np.random.default_rng(seed)
    pts = torch.tensor(rng.uniform(-1, 1, (P, 3)), dtype=torch.float32)
    dirs = torch.nn.functional.normalize(torch.tensor(rng.standard_normal((P, 3)), dtype=torch.float32), dim=-1)
    x = torch.cat([O.embed(pts, cfg.multires), O.embed(dirs, cfg.multires_views)], -1)
    shape = (lambda d: (P, K, d)) if opt.get("rows") else (lambda d: (K, d))
    ea = torch.tensor(rng.standard_normal(shape(1)), dtype=torch.float32)
    er = torch.tensor(rng.standard_normal(shape(3)), dtype=torch.float32)
    Gr = torch.tensor(rng.standard_normal((P, K, 4)), dtype=torch.float32) / (P * K)
    return dict(cfg=cfg, x=x, ea=ea, er=er, Gr=Gr, rows=bool(opt.get("rows")))


def seam_run(net, inp, extra, ent=True):
    """cfnerf_network_fwd (STASH | extra) + cfnerf_network_bwd at the C ABI"""
    lib, n = L.lib(), net.n_params
    x = inp["x"].to(DEV).contiguous()
    P, Cx = x.shape
    K = inp["cfg"].K_samples
    eps = torch.cat([inp["er"], inp["ea"]], -1).to(DEV).contiguous()
    net._sync()
    net.ensure_workspace(1, P, K)
    raw, entropy = api._network_fwd(net, x, eps, K, L.F_TRAIN | L.F_STASH | extra)
    gen = lib.cfnerf_model_stash_generation(net.handle)
    x_off = L.input_grad_offset(n)
    base_end = x_off + P * Cx if extra & L.F_INPUT_GRAD else n
    e_off, er_off, total = L.eps_grad_offsets(base_end, P, K) if extra & L.FLAG_EPS_GRAD else (base_end, base_end, base_end)
    buf = torch.full((total + 64,), float("nan"), device=DEV)
    d_ent = torch.full((1,), CC.C_ENT, device=DEV) if ent else None
    L.check(lib.cfnerf_network_bwd(net.handle, gen, L.ptr(inp["Gr"].to(DEV).contiguous()), L.ptr(d_ent), L.ptr(buf), L.stream()), "cfnerf_network_bwd")
    torch.cuda.synchronize()
    out = dict(raw=raw, entropy=entropy, buf=buf, grad=buf[:n], total=total, eps=eps)
    if extra & L.F_INPUT_GRAD:
        out["d_x"] = buf[x_off:x_off + P * Cx].view(P, Cx)
    if extra & L.FLAG_EPS_GRAD:
        out.update(d_eps=buf[e_off:e_off + K * 4].view(K, 4), rows=buf[er_off:er_off + P * K * 4].view(P, K, 4), pad=buf[e_off + K * 4:er_off])
    return out


@functools.lru_cache(maxsize=None)
def _seam(i):
    W, K, P, opt, seed = SEAM[i]
    inp = _seam_inputs(W, K, P, opt, seed)
    _, _, _, model, p, _ = build_model(inp["cfg"], seed)
    net = model.module
    extra = L.F_INPUT_GRAD if opt.get("input_grad") else 0
    hip = seam_run(net, inp, extra | L.FLAG_EPS_GRAD)
    _, masks = hip_relu_masks(net, P)
    rec = {}
    with torch.no_grad(), O.relu_override(record=rec):
        O.nerf_flows_forward({k: v.double() for k, v in p.items()}, inp["x"].double(), inp["ea"].double()[0] if inp["rows"] else inp["ea"].double(),
                             inp["er"].double()[0] if inp["rows"] else inp["er"].double(), inp["cfg"], False)
    n_flips = sum(int(((rec[k] > 0).float() != masks[k]).sum()) for k in rec)
    assert n_flips <= max(2, CC.FLIP_FRAC * sum(v.numel() for v in rec.values())), f"{n_flips} ReLU masks differ"
    ref = EC.reference(lambda dt: EC.network_rows(p, inp, masks, dt))
    hip0 = seam_run(net, inp, extra)
    return dict(inp=inp, net=net, model=model, p=p, ref=ref, hip=hip, hip0=hip0, extra=extra)


@pytest.mark.parametrize("i", range(len(SEAM)), ids=SEAM_IDS)
def test_seam_latent_gradient_vs_fp64_oracle_autograd(i):
    """cfnerf_network_fwd / cfnerf_network_bwd: d_eps and d_eps_rows [P,K,4] of sum(raw Gr) + 0.3 entropy under the bound of the fused cases;
    d_eps the fp64 sum of the rows; the parameter gradient, d_x and raw bit for bit what they are without the flag; two runs bit-equal"""
    c = _seam(i)
    h, h0 = c["hip"], c["hip0"]
    _hold(h["d_eps"], c["ref"]["d_eps"], SEAM_IDS[i], "seam d_eps")
    _hold(h["rows"], c["ref"]["rows"], SEAM_IDS[i], "seam d_eps_rows")
    want = h["rows"].double().sum(0).float()
    ulp = torch.maximum(want.abs(), torch.tensor(1e-37, device=DEV)).log2().floor().exp2() * 2.0 ** -23
    assert bool(((h["d_eps"] - want).abs() <= ulp).all())
    assert bool(torch.isnan(h["pad"]).all()) and bool(torch.isnan(h["buf"][h["total"]:]).all()), "a pad float was written"
    for k in ("raw", "entropy", "grad") + (("d_x",) if c["extra"] else ()):
        assert torch.equal(h[k], h0[k]), k + " changed with CFNERF_F_EPS_GRAD"
    again = seam_run(c["net"], c["inp"], c["extra"] | L.FLAG_EPS_GRAD)
    for k in ("grad", "d_eps", "rows"):
        assert torch.equal(again[k], h[k]), k + " is not bit-reproducible"
    # the identity with the means
    p = c["p"]
    d = h["d_eps"].detach().cpu().double() - EC.direct_term(h["eps"].cpu(), CC.C_ENT)
    got = (d / torch.cat([p["rgb_std"], p["alpha_std"]]).double()).sum(0)
    for key, sl in (("alpha_mean", slice(3, 4)), ("rgb_mean", slice(0, 3))):
        _record(SEAM_IDS[i], "seam identity " + key, CC.rel(got[sl], c["ref"]["base"][key]))
        grad_close_tight(got[sl], c["ref"]["base"][key], f"{SEAM_IDS[i]} seam identity grad {key}")


# ---------------------------------------------------------------- 8. refusals at the C ABI, each by message
def test_refusals_name_the_flag():
    c = _case(0)
    net, lib, inp = c["net"], L.lib(), c["inp"]
    K = inp["cfg"].K_samples
    rays, tv = inp["rays"].to(DEV), inp["tv"].to(DEV)
    eps = torch.cat([inp["er"], inp["ea"]], -1).to(DEV).contiguous()
    o = [torch.empty(1, 3, K, device=DEV), torch.empty(1, K, device=DEV), torch.empty(1, K, device=DEV)]
    ks, ent = torch.empty(1, 12, device=DEV), torch.zeros(1, device=DEV)
    net._sync()
    err = lambda: lib.cfnerf_last_error().decode()
    fwd = lambda flags, maps=True, kstats=None: lib.cfnerf_render_fwd(
        net.handle, L.ptr(rays), L.ptr(tv), None, None, L.ptr(eps), 1, 2, K, flags, *([L.ptr(t) for t in o] if maps else [None, L.ptr(o[1]), L.ptr(o[2])]),
        None, None, None, L.ptr(kstats), L.ptr(ent), L.stream())
    rc = fwd(L.F_TRAIN | L.FLAG_EPS_GRAD)
    assert rc != 0 and "CFNERF_F_EPS_GRAD needs CFNERF_F_STASH" in err(), err()
    rc = fwd(L.F_GEOMETRY | L.FLAG_EPS_GRAD, maps=False)
    assert rc != 0 and "CFNERF_F_EPS_GRAD" in err() and "CFNERF_F_GEOMETRY" in err(), err()
    rc = fwd(L.F_STASH | L.F_KSTATS_EXT | L.FLAG_EPS_GRAD, kstats=ks)
    assert rc != 0 and "CFNERF_F_EPS_GRAD" in err() and "CFNERF_F_KSTATS_EXT" in err(), err()
    rc = fwd(L.F_STASH | L.F_CULL | L.FLAG_EPS_GRAD)
    assert rc != 0 and "cfnerf_render_fwd does not take CFNERF_F_CULL" in err(), err()
    x, raw = torch.zeros(4, 90, device=DEV), torch.empty(4, K, 4, device=DEV)
    nf = lambda flags: lib.cfnerf_network_fwd(net.handle, L.ptr(x), L.ptr(eps), 4, K, flags, L.ptr(raw), L.ptr(ent), L.stream())
    rc = nf(L.F_TRAIN | L.FLAG_EPS_GRAD)
    assert rc != 0 and "CFNERF_F_EPS_GRAD needs CFNERF_F_STASH" in err(), err()
    rc = nf(L.F_GEOMETRY | L.FLAG_EPS_GRAD)
    assert rc != 0 and "CFNERF_F_EPS_GRAD" in err() and "CFNERF_F_GEOMETRY" in err(), err()
    rc = nf(L.F_STASH | L.F_KSTATS_EXT | L.FLAG_EPS_GRAD)
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_F_KSTATS_EXT" in err(), err()
    rc = nf(L.F_STASH | L.F_CULL | L.FLAG_EPS_GRAD)
    assert rc != 0 and "cfnerf_network_fwd does not take CFNERF_F_CULL" in err(), err()
    rc = lib.cfnerf_render_eval(net.handle, None, None, None, 4, 128, max(K, 2), L.FLAG_EPS_GRAD, None, None, None, L.stream())
    assert rc != 0 and "cfnerf_render_eval does not take CFNERF_F_EPS_GRAD" in err(), err()
    rc = lib.cfnerf_sample_points(None, None, None, L.FLAG_EPS_GRAD, 4, 128, None, None, L.stream())
    assert rc != 0 and "cfnerf_sample_points does not take CFNERF_F_EPS_GRAD" in err(), err()
    rc = lib.cfnerf_sample_pdf(None, None, None, L.FLAG_EPS_GRAD, None, None, 4, 128, K, 8, None, L.stream())
    assert rc != 0 and "cfnerf_sample_pdf does not take CFNERF_F_EPS_GRAD" in err(), err()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. against the reference's numbers (G28)
def _fixture_net(g, **over):
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]), netdepth=int(g["netdepth"]))
    args, kw_train, _, model, _, _ = build_model(cfg, int(g["seed"]), **over)
    model.module.flat.grad = None
    return cfg, args, model, model.module


def _masks_equal_the_references(net, P, g, name):
    _, masks = hip_relu_masks(net, P)
    for k, m in masks.items():
        ref = EC.T(g["mask." + k]).float()
        assert torch.equal(m, ref), f"{name}: the HIP forward's ReLU mask of {k} differs from the reference's in {int((m != ref).sum())} units"


def _equal_the_references(name, g, ea, er, net):
    for what, leaf in (("eps_alpha_grad", ea), ("eps_rgb_grad", er)):
        assert leaf.grad is not None, f"{name}: no gradient reached {what[:-5]}"
        _record(name, what, CC.rel(leaf.grad, EC.T(g[what])))
        grad_close_tight(leaf.grad, g[what], f"{name} {what}")
    grad = net.flat.grad.detach().cpu()
    for key in EC.BASE:
        off, cnt = net.layout[key]
        grad_close_tight(grad[off:off + cnt].reshape(g["grad." + key].shape), g["grad." + key], f"{name} grad {key}")
    net.flat.grad = None


def _g28_loss(ret, g):
    dv = lambda k: EC.T(g[k]).to(DEV)
    Gr = dv("Gr_a")[:, :, None, None] * dv("Gr_b")[None, None]
    return ((ret["rgb_map"] * dv("G")).sum() + (ret["disp_map"] * dv("Gq")).sum() + (ret["depth_map"] * dv("Gd")).sum() + (ret["raw"] * Gr).sum()
            + float(g["c_entropy"]) * ret["loss_entropy"].mean())


def test_g28a_render_rays_latent_gradient_equals_the_references():
    """through the Python surface (leaf eps_alpha / eps_rgb on the device) and through the C ABI (the d_eps block of cfnerf_render_bwd)"""
    g = EC.load(EC.NAMES[0])
    cfg, _, model, net = _fixture_net(g)
    ea, er = EC.T(g["eps_alpha"]).to(DEV).requires_grad_(True), EC.T(g["eps_rgb"]).to(DEV).requires_grad_(True)
    rb = EC.T(g["ray_batch"]).to(DEV)
    ret = cfnerf_amd.render_rays(rb, model, None, 128, True, False, perturb=1., t_rand=EC.T(g["t_rand"]), eps_alpha=ea, eps_rgb=er)
    loss = _g28_loss(ret, g)
    loss.backward()
    _masks_equal_the_references(net, 3 * 128, g, "G28a")
    close(ret["rgb_map"], g["rgb_map"], what="G28a rgb_map")
    close(loss, g["loss"], what="G28a loss")
    surface = torch.cat([er.grad, ea.grad], -1).clone()
    _equal_the_references("G28a", g, ea, er, net)
    # the C ABI: the same stash flags by hand
    K = int(g["K"])
    t = lambda k: EC.T(g[k])
    inp = dict(cfg=cfg, rays=t("ray_batch"), tv=O.t_vals_table(), t_rand=t("t_rand"), z=torch.zeros(3, 128), lindisp=False, wb=False, ea=t("eps_alpha"),
               er=t("eps_rgb"), cot=dict(G=t("G"), Gd=t("Gd"), Gq=t("Gq"), Gr=t("Gr_a")[:, :, None, None] * t("Gr_b")[None, None]))
    o = abi_bwd(net, inp, abi_fwd(net, inp, extra=L.F_COTANGENTS | L.FLAG_EPS_GRAD), ("G", "Gd", "Gq", "Gr", "ent"))
    want = np.concatenate([g["eps_rgb_grad"], g["eps_alpha_grad"]], -1)
    _record("G28a", "C ABI d_eps", CC.rel(o["d_eps"], EC.T(want)))
    grad_close_tight(o["d_eps"], want, "G28a C ABI d_eps")
    _record("G28a", "Python surface vs C ABI d_eps", CC.rel(surface, o["d_eps"]))
    grad_close_tight(surface, o["d_eps"].cpu().numpy(), "G28a Python surface vs C ABI d_eps")
    assert K == 3


def test_g28b_both_pairs_of_a_two_netchunk_batch_equal_the_references():
    g = EC.load(EC.NAMES[1])
    _, _, model, net = _fixture_net(g, netchunk_per_gpu=int(g["netchunk"]), latent_draws="netchunk")
    ea, er = EC.T(g["eps_alpha"]).to(DEV).requires_grad_(True), EC.T(g["eps_rgb"]).to(DEV).requires_grad_(True)
    assert tuple(ea.shape) == (2, 3, 1)
    run = lambda: cfnerf_amd.render_rays(EC.T(g["ray_batch"]).to(DEV), model, None, 128, True, False, perturb=1., t_rand=EC.T(g["t_rand"]), eps_alpha=ea,
                                         eps_rgb=er, lindisp=True, white_bkgd=True)
    ret = run()
    loss = _g28_loss(ret, g)
    loss.backward()
    _masks_equal_the_references(net, 4 * 128, g, "G28b")
    close(ret["rgb_map"], g["rgb_map"], what="G28b rgb_map")
    close(loss, g["loss"], what="G28b loss")
    first = (ea.grad.clone(), er.grad.clone())
    _equal_the_references("G28b", g, ea, er, net)
    # the whole chain - pack, pairs -> rows, the kernels, the segment sums - is bit-reproducible
    ea.grad = er.grad = None
    _g28_loss(run(), g).backward()
    assert torch.equal(ea.grad, first[0]) and torch.equal(er.grad, first[1])
    net.flat.grad = None


def test_g28c_forward_latent_gradient_equals_the_references():
    """NeRF_Flows.forward(x, eps_alpha=, eps_rgb=) with leaf latents, and cfnerf_network_bwd's d_eps block"""
    g = EC.load(EC.NAMES[2])
    cfg, _, model, net = _fixture_net(g)
    ea, er = EC.T(g["eps_alpha"]).to(DEV).requires_grad_(True), EC.T(g["eps_rgb"]).to(DEV).requires_grad_(True)
    raw, ent = net(EC.T(g["x"]).to(DEV), False, False, eps_alpha=ea, eps_rgb=er)
    loss = (raw * EC.T(g["Gr"]).to(DEV)).sum() + float(g["c_entropy"]) * ent.mean()
    loss.backward()
    _masks_equal_the_references(net, 5, g, "G28c")
    close(raw, g["raw"], what="G28c raw")
    close(loss, g["loss"], what="G28c loss")
    _equal_the_references("G28c", g, ea, er, net)
    inp = dict(cfg=cfg, x=EC.T(g["x"]), ea=EC.T(g["eps_alpha"]), er=EC.T(g["eps_rgb"]), Gr=EC.T(g["Gr"]), rows=False)
    o = seam_run(net, inp, L.FLAG_EPS_GRAD)
    want = np.concatenate([g["eps_rgb_grad"], g["eps_alpha_grad"]], -1)
    _record("G28c", "C ABI d_eps", CC.rel(o["d_eps"], EC.T(want)))
    grad_close_tight(o["d_eps"], want, "G28c C ABI d_eps")


# ---------------------------------------------------------------- 9. the Python surface (each of these is None without the feature)
def _leaves(inp):
    return inp["ea"].to(DEV).requires_grad_(True), inp["er"].to(DEV).requires_grad_(True)


def _surface_kw(inp, ea, er):
    return dict(perturb=1. if inp["t_rand"] is not None else 0., t_rand=inp["t_rand"], eps_alpha=ea, eps_rgb=er, t_vals=inp["tv"],
                lindisp=inp["lindisp"], white_bkgd=inp["wb"])


def test_leaf_latents_get_the_c_abis_gradient_frozen_network_or_not():
    c = _case(2)
    inp, net, model = c["inp"], c["net"], c["model"]
    S = inp["z"].shape[1]
    got = {}
    for frozen in (False, True):
        net.flat.requires_grad_(not frozen)
        net.flat.grad = None
        try:
            ea, er = _leaves(inp)
            ret = cfnerf_amd.render_rays(inp["rays"].to(DEV), model, None, S, True, False, **_surface_kw(inp, ea, er))
            CC.loss_of(ret, inp["cot"], EC.USES["plain"]).backward()
            assert ea.grad is not None and er.grad is not None, "no gradient reached the latents"
            assert (net.flat.grad is None) == frozen
            got[frozen] = torch.cat([er.grad, ea.grad], -1)
        finally:
            net.flat.requires_grad_(True)
            net.flat.grad = None
    assert torch.equal(got[True], got[False]), "a frozen network gives another latent gradient"
    _hold(got[True], c["ref"]["plain"]["d_eps"], IDS[2], "render_rays leaf latents")


def test_ray_rows_as_leaves_get_one_row_each():
    c = _case(8)
    inp, net = c["inp"], c["net"]
    rows = torch.cat([inp["er"], inp["ea"]], -1).to(DEV).requires_grad_(True)
    f = api._RenderFn.apply(net.flat, net, inp["rays"].to(DEV), inp["tv"].to(DEV), inp["t_rand"].to(DEV), rows,
                            L.F_TRAIN, False, None, False)
    ret = dict(rgb_map=f[0], disp_map=f[1], depth_map=f[2], loss_entropy=f[3])
    CC.loss_of(ret, inp["cot"], EC.USES["plain"]).backward()
    assert rows.grad is not None and tuple(rows.grad.shape) == tuple(rows.shape)
    _hold(rows.grad, c["ref"]["plain"]["rows"], IDS[8], "leaf ray rows")
    net.flat.grad = None


def test_a_custom_network_query_fn_reaches_the_latents():
    """the unfused route: render_rays hands the latents to NeRF_Flows.forward, whose node returns their gradient; against the fused route's
    under the suite's fused-vs-unfused bound, and rows through the seam bit-reproducibly"""
    c = _case(1)
    inp, net, model = c["inp"], c["net"], c["model"]
    S = inp["z"].shape[1]
    embed_fn, _ = cfnerf_amd.get_embedder(inp["cfg"].multires)
    embeddirs_fn, _ = cfnerf_amd.get_embedder(inp["cfg"].multires_views)
    qf = lambda inputs, viewdirs, fn, is_val, is_test: api.run_network(inputs, viewdirs, fn, is_val, is_test, embed_fn, embeddirs_fn)
    ea, er = _leaves(inp)
    ret = cfnerf_amd.render_rays(inp["rays"].to(DEV), model, qf, S, True, False, **_surface_kw(inp, ea, er))
    CC.loss_of(ret, inp["cot"], EC.USES["plain"]).backward()
    assert ea.grad is not None and er.grad is not None, "no gradient reached the latents through the custom network_query_fn"
    _hold(torch.cat([er.grad, ea.grad], -1), c["ref"]["plain"]["d_eps"], IDS[1], "custom network_query_fn d_eps")
    net.flat.grad = None


def test_the_eval_branch_is_a_graph_in_the_latents_too():
    """is_train=False with explicit latents that require grad: the stashed train-branch launch on them, no entropy cotangent, the eval structure;
    against the fp64 oracle's eval branch on the HIP forward's masks, under the fixed bound of the fixtures"""
    c = _case(2)
    inp, net, model, p = c["inp"], c["net"], c["model"], c["p"]
    S = inp["z"].shape[1]
    ea, er = _leaves(inp)
    ret = cfnerf_amd.render_rays(inp["rays"].to(DEV), model, None, S, False, False, **_surface_kw(inp, ea, er))
    assert sorted(ret) == ["depth_map", "disp_map", "rgb_map"]
    CC.loss_of(ret, inp["cot"], ("G", "Gd")).backward()
    assert ea.grad is not None and er.grad is not None, "the eval branch gave the latents no gradient"
    d = lambda t: t.double()
    la, lr = d(inp["ea"]).requires_grad_(True), d(inp["er"]).requires_grad_(True)
    with O.relu_override(masks=c["masks"]):
        ro = O.render_rays({k: d(v) for k, v in p.items()}, d(inp["rays"]), inp["cfg"], la, lr, False, None, inp["lindisp"], inp["wb"], z_vals=d(inp["z"]))
    CC.loss_of(ro, inp["cot"], ("G", "Gd")).backward()
    for what, g, r in (("eval eps_alpha", ea.grad, la.grad), ("eval eps_rgb", er.grad, lr.grad)):
        _record(IDS[2], what, CC.rel(g, r))
        grad_close_tight(g, r.numpy(), f"{IDS[2]} {what}", tol=EC.G_TIGHT)
    net.flat.grad = None


def test_forward_with_leaf_latents_and_a_frozen_network():
    c = _seam(1)
    inp, net = c["inp"], c["net"]
    net.flat.requires_grad_(False)
    try:
        ea, er = _leaves(inp)
        raw, ent = net(inp["x"].to(DEV), False, False, eps_alpha=ea, eps_rgb=er)
        ((raw * inp["Gr"].to(DEV)).sum() + CC.C_ENT * ent.mean()).backward()
        assert ea.grad is not None and er.grad is not None and net.flat.grad is None
        _hold(torch.cat([er.grad, ea.grad], -1), c["ref"]["d_eps"], SEAM_IDS[1], "forward leaf latents, frozen network")
        # the eval branch of forward
        ea, er = _leaves(inp)
        raw, aux = net(inp["x"].to(DEV), False, True, eps_alpha=ea, eps_rgb=er)
        (raw * inp["Gr"].to(DEV)).sum().backward()
        assert ea.grad is not None and float(ea.grad.abs().max()) > 0 and not bool(aux.any())
    finally:
        net.flat.requires_grad_(True)
        net.flat.grad = None


def _explicit_depth_reference(c, ret, use):
    """the fp64 oracle at the depths an explicit-depth launch used (constants of the graph), on the ReLU masks of that launch - the model's last
    STASH forward - with the calibration of test 1"""
    inp, net = c["inp"], c["net"]
    z = ret["z_vals"].detach().cpu()
    _, masks = hip_relu_masks(net, z.shape[0] * z.shape[1])
    at = dict(inp, z=z)
    return EC.reference(lambda dt: EC.render_rows(c["p"], at, masks, dt, use))


@pytest.mark.parametrize("is_train", [True, False], ids=["train", "eval"])
def test_the_hierarchical_fine_pass_reaches_the_latents(is_train):
    """render_rays(hierarchical_extension=True) with leaf latents: the fine pass - the explicit-depth stashed launch, on the eval branch too -
    returns their gradient (the resampled depths are constants); frozen network"""
    c = _case(2)
    inp, net, model = c["inp"], c["net"], c["model"]
    N, S = inp["z"].shape
    use = EC.USES["plain"] if is_train else ("G", "Gd")
    u = torch.rand(N, 8, generator=torch.Generator().manual_seed(5))
    net.flat.requires_grad_(False)
    try:
        ea, er = _leaves(inp)
        ret = cfnerf_amd.render_rays(inp["rays"].to(DEV), model, None, S, is_train, False, N_importance=8, hierarchical_extension=True, u_fine=u,
                                     **_surface_kw(inp, ea, er))
        assert tuple(ret["z_vals"].shape) == (N, S + 8) and ("loss_entropy" in ret) == is_train
        CC.loss_of(ret, inp["cot"], use).backward()
        assert ea.grad is not None and er.grad is not None, "the fine pass gave the latents no gradient"
        ref = _explicit_depth_reference(c, ret, use)
        _hold(torch.cat([er.grad, ea.grad], -1), ref["d_eps"], IDS[2], "hierarchical fine pass d_eps, " + ("train" if is_train else "eval"))
    finally:
        net.flat.requires_grad_(True)
        net.flat.grad = None


@pytest.mark.parametrize("is_train", [True, False], ids=["train", "eval"])
def test_render_rays_warped_reaches_the_latents(is_train):
    """render_rays_warped with leaf latents: the depths warped into the occupied bins of a half-full grid are constants, the latents get
    the gradient of the explicit-depth launch on either branch; frozen network"""
    c = _case(2)
    inp, net, model = c["inp"], c["net"], c["model"]
    use = EC.USES["plain"] if is_train else ("G", "Gd")
    mask = torch.zeros(4, 4, 4, dtype=torch.bool)
    mask[:, :, ::2] = True                                 # every other layer along z: each ray crosses occupied and empty runs
    sampler = E.OccupancyGrid.from_mask(mask, (-3.0, -3.0, -7.0), (3.0, 3.0, 0.0)).sampler(bins=16, pad=0)
    net.flat.requires_grad_(False)
    try:
        ea, er = _leaves(inp)
        ret = api.render_rays_warped(inp["rays"].to(DEV), model, sampler, is_train, perturb=1., t_rand=inp["t_rand"], eps_alpha=ea, eps_rgb=er,
                                     t_vals=inp["tv"])
        assert not torch.equal(ret["z_vals"].cpu(), inp["z"]), "the grid did not move a depth: the case tests nothing"
        CC.loss_of(ret, inp["cot"], use).backward()
        assert ea.grad is not None and er.grad is not None, "render_rays_warped gave the latents no gradient"
        ref = _explicit_depth_reference(c, ret, use)
        _hold(torch.cat([er.grad, ea.grad], -1), ref["d_eps"], IDS[2], "render_rays_warped d_eps, " + ("train" if is_train else "eval"))
    finally:
        net.flat.requires_grad_(True)
        net.flat.grad = None


def test_pairs_reach_the_seam_as_rows_through_a_custom_network_query_fn():
    """per-netchunk pairs that require grad on the unfused route: render_rays hands NeRF_Flows.forward one row per POINT (an expand of the ray
    rows, whose adjoint is a plain sum), the seam returns d_eps_rows [P,K,4], and the sums arrive at the pairs; against the fp64 oracle called
    per ray with that ray's pair, and twice bit for bit"""
    c = _case(8)
    inp, net, model, p = c["inp"], c["net"], c["model"], c["p"]
    N, S = inp["z"].shape
    K = inp["cfg"].K_samples
    embed_fn, _ = cfnerf_amd.get_embedder(inp["cfg"].multires)
    embeddirs_fn, _ = cfnerf_amd.get_embedder(inp["cfg"].multires_views)
    qf = lambda inputs, viewdirs, fn, is_val, is_test: api.run_network(inputs, viewdirs, fn, is_val, is_test, embed_fn, embeddirs_fn)
    rng = np.random.default_rng(288)
    pa, pr = (torch.tensor(rng.standard_normal((3, K, d)), dtype=torch.float32) for d in (1, 3))
    net.netchunk, keep = 2 * S, net.netchunk               # two rays per network call: three pairs for the six rays
    got = []
    try:
        for _ in range(2):
            ea, er = pa.to(DEV).requires_grad_(True), pr.to(DEV).requires_grad_(True)
            ret = cfnerf_amd.render_rays(inp["rays"].to(DEV), model, qf, S, True, False, perturb=1., t_rand=inp["t_rand"], eps_alpha=ea, eps_rgb=er,
                                         t_vals=inp["tv"])
            CC.loss_of(ret, inp["cot"], EC.USES["plain"]).backward()
            assert ea.grad is not None and er.grad is not None, "no gradient reached the pairs through the custom network_query_fn"
            got.append(torch.cat([er.grad, ea.grad], -1))
        _, masks = hip_relu_masks(net, N * S)
    finally:
        net.netchunk = keep
        net.flat.grad = None
    assert torch.equal(got[0], got[1]), "the pairs' gradient through the seam is not bit-reproducible"
    idx = LT.netchunk_row_index(N, S, 2 * S)
    counts = torch.bincount(idx, minlength=3).tolist()
    assert counts == [2, 2, 2]
    at = dict(inp, ea=pa[idx], er=pr[idx], rows=True)
    ref = EC.reference(lambda dt: EC.render_rows(p, at, masks, dt, EC.USES["plain"]), counts=counts)
    _hold(got[0], ref["pairs"], IDS[8], "pairs through a custom network_query_fn")


def test_trainer_latent_grad_equals_the_autograd_routes():
    """Trainer(latent_grad=True).d_eps against eps.grad of render_rays fed the step's own cotangent (Trainer.d_rgb) and beta1 on the entropy: the
    same launches, bit for bit; a sliced step sums its slices; netchunk mode leaves one gradient per pair; world_size > 1 is refused"""
    N, S, K = 8, 66, 4
    cfg = O.OracleCfg(netwidth=64, K_samples=K)
    _, _, _, model, p, _ = build_model(cfg, 281)
    net = model.module
    rng = np.random.default_rng(281)
    rb = CC.random_rays(rng, N)
    rays = torch.stack([rb[:, 0:3], rb[:, 3:6]], 0).to(DEV)
    target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32).to(DEV)
    eps = torch.tensor(rng.standard_normal((K, 4)), dtype=torch.float32).to(DEV)
    tv = torch.linspace(0., 1., S).to(DEV)
    kw = dict(t_rand=torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32).to(DEV), near=2., far=6., ndc=False, t_vals=tv)
    plain = TR.Trainer(net, beta1=0.05)
    g0 = plain.forward_backward(4, 2, 3., rays, target, eps=eps, **kw).clone()
    assert plain.d_eps is None and plain.gbuf.numel() == net.n_params + 4 * TR.MAX_K
    one = TR.Trainer(net, beta1=0.05, latent_grad=True)
    g1 = one.forward_backward(4, 2, 3., rays, target, eps=eps, **kw).clone()
    assert torch.equal(g1, g0), "latent_grad=True moved the parameter gradient"
    assert tuple(one.d_eps.shape) == (K, 4) and float(one.d_eps.abs().max()) > 0
    ea, er = eps[:, 3:4].clone().requires_grad_(True), eps[:, 0:3].clone().requires_grad_(True)
    ret = cfnerf_amd.render_rays(one.packed.clone(), model, None, S, True, False, perturb=1., t_rand=kw["t_rand"], eps_alpha=ea, eps_rgb=er, t_vals=tv)
    ((ret["rgb_map"] * one.d_rgb).sum() + 0.05 * ret["loss_entropy"][0, 0, 0]).backward()      # (one element of the expanded scalar: d_entropy = beta1 itself)
    assert torch.equal(torch.cat([er.grad, ea.grad], -1), one.d_eps)
    net.flat.grad = None
    sl = TR.Trainer(net, beta1=0.05, latent_grad=True, max_rays_per_launch=4)
    sl.forward_backward(4, 2, 3., rays, target, eps=eps, **kw)
    err = CC.rel(sl.d_eps, one.d_eps)
    _record("Trainer slices 2x4 vs 8", "d_eps", err)
    grad_close_tight(sl.d_eps, one.d_eps.cpu().numpy(), "Trainer slices d_eps")
    nc = TR.Trainer(net, beta1=0.05, latent_grad=True, latent_draws="netchunk", netchunk=4 * S, chunk=None)
    pairs = torch.tensor(rng.standard_normal((2, K, 4)), dtype=torch.float32)
    nc.forward_backward(4, 2, 3., rays, target, eps_chunks=pairs, **kw)
    assert tuple(nc.d_eps.shape) == (2, K, 4) and float(nc.d_eps[1].abs().max()) > 0
    ea, er = pairs[..., 3:4].to(DEV).requires_grad_(True), pairs[..., 0:3].to(DEV).requires_grad_(True)
    net.netchunk, keep = 4 * S, net.netchunk
    try:
        ret = cfnerf_amd.render_rays(nc.packed.clone(), model, None, S, True, False, perturb=1., t_rand=kw["t_rand"], eps_alpha=ea, eps_rgb=er, t_vals=tv)
        ((ret["rgb_map"] * nc.d_rgb).sum() + 0.05 * ret["loss_entropy"][0, 0, 0]).backward()
    finally:
        net.netchunk = keep
    assert torch.equal(torch.cat([er.grad, ea.grad], -1), nc.d_eps)
    net.flat.grad = None
    with pytest.raises(NotImplementedError, match="latent_grad"):
        TR.Trainer(net, latent_grad=True, world_size=2)
    # the hierarchical step is refused before any launch (its passes would carry no room for the latent blocks), and leaves the trainer usable
    hkw = dict(N_samples=16, N_importance=8, near=2., far=6., ndc=False)
    with pytest.raises(NotImplementedError, match=r"latent_grad=True\) is not supported by forward_backward_hierarchical"):
        one.forward_backward_hierarchical(4, 2, 3., rays, target, **hkw)
    with pytest.raises(NotImplementedError, match=r"latent_grad=True\) is not supported by forward_backward_hierarchical"):
        one.step_hierarchical(4, 2, 3., rays, target, **hkw)
    torch.cuda.synchronize()
    assert torch.equal(one.forward_backward(4, 2, 3., rays, target, eps=eps, **kw), g0)
    # ... and a trainer without the option runs it with the plain flags: gradient buffers of before, no latent block written
    plain.forward_backward_hierarchical(4, 2, 3., rays, target, **hkw)
    torch.cuda.synchronize()
    assert plain.d_eps is None and plain.gbuf.numel() == net.n_params + 4 * TR.MAX_K
