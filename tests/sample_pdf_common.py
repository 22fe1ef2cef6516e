"""Shared by tests/test_sample_pdf_cpu.py and tests/test_hip_sample_pdf.py: the fp64 inverse-CDF BRACKET that every output of the hierarchical
resampler (``cfnerf_sample_pdf``, include/cfnerf.h; ``oracle.cfnerf_oracle.sample_pdf``) is held to, and the inputs both tests run it on.

Why a bracket and not a distance: the inverse CDF is steep where a bin has little mass, and with the ``denom < 1e-5`` clamp it JUMPS (a
clamped bin maps to its left edge, the next bin starts at its right edge), so an fp32 CDF entry that rounds to the other side of ``u`` moves
a sample by a whole coarse bin.  What survives rounding is monotonicity.  With ``Finv(u; thr)`` the fp64 restatement below (searchsorted
right, below / above, ``denom < thr -> 1``, linear interpolation) - non-decreasing in ``u`` for every ``thr``, and lowering ``thr`` can only
raise it - the acceptable interval of the sample drawn for ``u`` is

    lo(u) = Finv(max(u - T_u, 0); 1e-5 + 2 T_u) - T_z          hi(u) = Finv(u + T_u; 1e-5 - 2 T_u) + T_z

T_U = 2e-6: the worst-case fp32 error of ONE CDF entry of the kernel - a sum at most 6 scan levels + 15 carry additions deep whose terms carry
the rounding of the division and of the wave-summed total: about 30 roundings of 2^-24 on values <= 1.  The clamp band is 2 T_u because
``denom`` is a difference of two such entries.  T_z = 4 * 2^-24 * max|z| of the ray: one rounding of the fp32 midpoint, three of
``b0 + t * (b1 - b0)``.  Derived, not tuned: an output that needs more is a finding."""
import numpy as np
import torch

T_U = 2e-6
T_Z_ROUNDINGS = 4.0
CLAMP = 1e-5
WIDE_SHARE_MAX = 0.10       # non-vacuity: at most this share of a case's brackets may be wider than half their local coarse bin

# (S, Ni, K): no inner weight but one; one scan chunk of 64; the chunk boundary from both sides (S - 2 = 64, 65); several chunks; the 1024 limit
SHAPES = [(3, 5, 1), (4, 64, 2), (64, 128, 3), (66, 63, 3), (67, 65, 4), (130, 70, 3), (200, 128, 16), (512, 512, 2), (959, 65, 1)]
N_RAYS = 8
W_KINDS = ("uniform", "zero", "random", "surface", "onehot", "two")
U_KINDS = ("uniform", "linspace", "half", "rep4", "knots")


# ---- the fp64 restatement ------------------------------------------------------------------------------------------------------------
def pdf_tables(z, w, mutation=None):
    """fp32 coarse depths ``z [N,S]`` and weights ``w [N,S,K]`` -> fp64 ``(bins [N,S-1], cdf [N,S-1])``: bins = mids of consecutive depths,
    cdf = [0, cumsum(pdf)] of the K-mean of the INNER weights + 1e-5.  ``mutation``: one of the four wrong restatements the CPU test shows
    the bracket catches (never used by a check).
    The two order-dependent reductions - the mean over K and the total - are torch's on the whole batch, everything else is numpy: two
    libraries add in different orders, and one rounding of fp64 in the total is all that would keep the fp64 oracle from passing with
    T_u = T_z = 0, bit for bit."""
    z = np.asarray(z, dtype=np.float64)
    w = torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float64)))
    bins = 0.5 * (z[:, 1:] + z[:, :-1])
    wm = w.mean(-1)
    wm = (wm[:, 0:-2] if mutation == "slice" else wm[:, 1:-1]) + (0.0 if mutation == "no_eps" else 1e-5)
    pdf = (wm / torch.sum(wm, -1, keepdim=True)).numpy()
    if mutation == "no_carry":          # a chunked scan (64 entries per chunk) that forgets what the chunks before it summed to
        csum = np.concatenate([np.cumsum(pdf[:, b:b + 64], -1) for b in range(0, pdf.shape[1], 64)], -1)
    else:
        csum = np.cumsum(pdf, -1)
    cdf = np.concatenate([np.zeros_like(csum[:, :1]), csum], -1)
    if mutation == "bins_shift":
        bins = np.concatenate([bins[:, 1:], bins[:, -1:]], -1)
    return bins, cdf


def finv(bins, cdf, u, thr=CLAMP):
    """Inverse-CDF sampling of nerf-pytorch's sample_pdf in fp64, with the clamp threshold as a parameter"""
    u = np.asarray(u, dtype=np.float64)
    inds = np.searchsorted(cdf, u, side="right")
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, cdf.shape[0] - 1)
    denom = cdf[above] - cdf[below]
    denom = np.where(denom < thr, 1.0, denom)
    t = (u - cdf[below]) / denom
    return bins[below] + t * (bins[above] - bins[below])


def resample64(z, w, u, mutation=None):
    """[N,S], [N,S,K], [N,Ni] -> the merged, sorted fp64 depths [N,S+Ni] of the restatement (or of one of its mutations)"""
    z, u = _np(z).astype(np.float64), _np(u)
    bins, cdf = pdf_tables(z, _np(w), mutation)
    return np.stack([np.sort(np.concatenate([z[n], finv(bins[n], cdf[n], u[n])])) for n in range(z.shape[0])])


# ---- the check ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def judge(z_out, z_coarse, w, u, t_u=T_U, t_z_roundings=T_Z_ROUNDINGS):
    """Measure ``z_out [N,S+Ni]`` (fp32 from a kernel or the fp32 oracle, fp64 from the fp64 oracle) against the coarse depths ``z_coarse
    [N,S]`` (fp32), the weights ``w [N,S,K]`` and ``u [N,Ni]``.  Returns a dict of what ``check_sample_pdf`` asserts on; rows that fail checks
    1 - 3 take no part in the bracket statistics (``rows_judged``)."""
    z_out, z_coarse, w, u = _np(z_out), _np(z_coarse), _np(w), _np(u)
    N, S = z_coarse.shape
    Ni = u.shape[1]
    assert z_out.shape == (N, S + Ni) and w.shape[:2] == (N, S) and z_coarse.dtype == np.float32, (z_out.shape, z_coarse.shape, w.shape)
    zc = z_coarse.astype(z_out.dtype)                 # (exact: fp32 -> fp32 or fp32 -> fp64)
    r = dict(n_nan=int(np.isnan(z_out).sum()), n_unsorted=0, n_coarse_missing=0, n_outside=0, n_wide=0, n_samples=0, rows_judged=0,
             max_cdf_err=0.0, worst=None)
    bins_all, cdf_all = pdf_tables(z_coarse, w)
    for n in range(N):
        row = z_out[n]
        if np.isnan(row).any():
            continue
        if (row[1:] < row[:-1]).any():
            r["n_unsorted"] += int((row[1:] < row[:-1]).sum())
            continue
        # check 3: the S coarse depths are in the row bit for bit, as a multiset - the k-th copy of a value takes the k-th slot that holds it
        cs = np.sort(zc[n])
        idx = np.searchsorted(row, cs, side="left") + (np.arange(S) - np.searchsorted(cs, cs, side="left"))
        ok = idx < S + Ni
        ok[ok] = _bits(row[idx[ok]]) == _bits(cs[ok])
        if not ok.all():
            r["n_coarse_missing"] += int((~ok).sum())
            continue
        keep = np.ones(S + Ni, dtype=bool)
        keep[idx] = False
        samples = row[keep].astype(np.float64)        # sorted, like the row
        us = np.sort(u[n].astype(np.float64))
        bins, cdf = bins_all[n], cdf_all[n]
        t_z = t_z_roundings * 2.0 ** -24 * float(np.abs(z_coarse[n]).max())
        lo = finv(bins, cdf, np.maximum(us - t_u, 0.0), CLAMP + 2 * t_u) - t_z
        hi = finv(bins, cdf, us + t_u, CLAMP - 2 * t_u) + t_z
        assert (lo <= hi).all() and (lo[1:] >= lo[:-1]).all() and (hi[1:] >= hi[:-1]).all()      # (the reference's own monotonicity)
        out = (samples < lo) | (samples > hi)
        # the local coarse bin of a sample: the interval of bins the exact search lands in (the last / first one beyond the ends) - for a
        # bracket that straddles a knot, the wider of the bins that u - T_u and u + T_u land in
        i0 = np.clip(np.searchsorted(cdf, np.maximum(us - t_u, 0.0), side="right"), 1, cdf.shape[0] - 1)
        i1 = np.clip(np.searchsorted(cdf, us + t_u, side="right"), 1, cdf.shape[0] - 1)
        local = np.maximum(bins[i0] - bins[i0 - 1], bins[i1] - bins[i1 - 1])
        wide = (hi - lo) > 0.5 * local
        if out.any() and r["worst"] is None:
            i = int(np.argmax(out))
            r["worst"] = dict(ray=n, i=i, u=float(us[i]), z=float(samples[i]), lo=float(lo[i]), hi=float(hi[i]))
        r["n_outside"] += int(out.sum())
        r["n_wide"] += int(wide.sum())
        r["n_samples"] += Ni
        r["rows_judged"] += 1
        r["max_cdf_err"] = max(r["max_cdf_err"], float(np.abs(np.interp(samples, bins, cdf) - us).max()))
    r["wide_share"] = r["n_wide"] / max(r["n_samples"], 1)
    r["outside_share"] = r["n_outside"] / max(r["n_samples"], 1)
    r["rows"] = N
    return r


def check_sample_pdf(z_out, z_coarse, w, u, what="", t_u=T_U, t_z_roundings=T_Z_ROUNDINGS):
    """The five checks on a whole ``z_out [N,S+Ni]`` that was filled with NaN before the call: (1) no NaN is left - every rank was written;
    (2) every row is non-decreasing; (3) every row holds its S coarse depths bit for bit; (4) the other Ni values, in order, lie in the
    brackets of the sorted ``u``; (5) the brackets mean something: at most WIDE_SHARE_MAX of them are wider than half their coarse bin."""
    return assert_judged(judge(z_out, z_coarse, w, u, t_u, t_z_roundings), what)


def assert_judged(r, what=""):
    """the assertions of ``check_sample_pdf`` on what ``judge`` measured"""
    assert r["n_nan"] == 0, f"{what}: {r['n_nan']} slots of z_out were never written (NaN left)"
    assert r["n_unsorted"] == 0, f"{what}: {r['n_unsorted']} descents in the merged rows"
    assert r["n_coarse_missing"] == 0, f"{what}: {r['n_coarse_missing']} coarse depths are not in z_out bit for bit"
    assert r["rows_judged"] == r["rows"]
    assert r["n_outside"] == 0, f"{what}: {r['n_outside']} of {r['n_samples']} samples outside their fp64 bracket, first {r['worst']}"
    assert r["wide_share"] <= WIDE_SHARE_MAX, f"{what}: {r['wide_share']:.3f} of the brackets are wider than half their coarse bin (vacuous)"
    return r


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def make_rays(rng, N, ndc):
    """packed rays [N,11]: random origins / directions; NDC (0, 1) or per-ray near in [1.5, 2.5], far in [5, 7]"""
    o, d = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
    near = np.zeros((N, 1)) if ndc else rng.uniform(1.5, 2.5, (N, 1))
    far = np.ones((N, 1)) if ndc else rng.uniform(5.0, 7.0, (N, 1))
    return torch.tensor(np.concatenate([o, d, near, far, d / np.linalg.norm(d, axis=-1, keepdims=True)], -1), dtype=torch.float32)


def make_t_vals(S, uniform=True):
    if uniform:
        return torch.linspace(0., 1., steps=S)
    t = torch.linspace(0., 1., steps=S, dtype=torch.float64)
    return (0.35 * t + 0.65 * t ** 3).float()          # increasing, 0 and 1 at the ends, steps that differ by a factor of ~7


def make_weights(rng, kind, N, S, K):
    """fp32 ``[N,S,K]`` coarse weights as a compositing pass makes them: non-negative, at most 1 in total along a ray"""
    w = np.zeros((N, S, K))
    if kind == "uniform":
        w[:] = 1.0 / S
    elif kind == "zero":
        pass                                            # the pdf is uniform through the 1e-5 alone
    elif kind == "random":                              # heavy-tailed, a total between 0.2 and 1: many bins near and below the 1e-5
        w = rng.uniform(0, 1, (N, S, K)) ** 6
        w *= rng.uniform(0.2, 1.0, (N, 1, 1)) / w.sum(1, keepdims=True)
    elif kind == "surface":                             # alpha compositing of a sharp sigmoid density: a trained ray, most bins clamped
        t = np.linspace(0., 1., S)[None, :, None]
        t0 = rng.uniform(0.3, 0.85, (N, 1, 1)) + 0.01 * rng.standard_normal((N, 1, K))
        sigma = 400.0 * S / (1.0 + np.exp(np.minimum(-(t - t0) * 4.0 * S, 700.0)))
        alpha = 1.0 - np.exp(-sigma / S)
        trans = np.cumprod(np.concatenate([np.ones((N, 1, K)), 1.0 - alpha[:, :-1] + 1e-10], 1), 1)
        w = alpha * trans
    elif kind == "onehot":
        j = rng.integers(1, S - 1, N)
        w[np.arange(N), j] = 1.0
    elif kind == "two":                                 # mass at samples 1 and S - 2, split unevenly (u = 0.5 lands inside one of them)
        a = rng.choice([-1.0, 1.0], N) * rng.uniform(0.1, 0.35, N) + 0.5
        w[:, 1] += a[:, None]
        w[:, S - 2] += (1.0 - a)[:, None]
    else:
        raise ValueError(kind)
    return torch.tensor(w, dtype=torch.float32)


def cdf_knots32(z, w):
    """the oracle's own fp32 CDF [N,S-1] (the lines of ``oracle.cfnerf_oracle.sample_pdf`` up to the search)"""
    wm = w.mean(-1)[..., 1:-1] + 1e-5
    cdf = torch.cumsum(wm / torch.sum(wm, -1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)


def make_u(rng, kind, N, Ni, z=None, w=None):
    """fp32 ``[N,Ni]`` in [0, 1]"""
    if kind == "uniform":
        u = np.sort(rng.uniform(0, 1, (N, Ni)), -1)
    elif kind == "linspace":                            # what perturb == 0 sends: exact 0 and exact 1
        u = np.broadcast_to(np.linspace(0., 1., Ni, dtype=np.float32), (N, Ni))
    elif kind == "half":
        u = np.full((N, Ni), 0.5)
    elif kind == "rep4":                                # ties in the rank sort: every value four times, in shuffled order
        u = rng.permuted(np.repeat(rng.uniform(0, 1, (N, (Ni + 3) // 4)), 4, -1)[:, :Ni], axis=-1)
    elif kind == "knots":                               # u ON a CDF entry (the `<=` of the search): the knot that closes the bin of a uniform draw
        cdf = cdf_knots32(z, w)
        d = torch.tensor(rng.uniform(0, 1, (N, Ni)), dtype=torch.float32)
        inds = torch.searchsorted(cdf, d, right=True).clamp(max=cdf.shape[-1] - 1)
        return torch.gather(cdf, -1, inds).clamp(0., 1.).contiguous()
    else:
        raise ValueError(kind)
    return torch.tensor(np.ascontiguousarray(u), dtype=torch.float32)


def geometries(S):
    """(ndc, lindisp, jitter, uniform table) of a shape.  ``lindisp`` goes with per-ray near / far only: it divides by near, which NDC sets
    to 0 (the reference's own depths are NaN there).  The non-uniform sample table is run at one shape."""
    g = [(True, False, True, True), (True, False, False, True), (False, False, True, True), (False, False, False, True),
         (False, True, True, True), (False, True, False, True)]
    if S == 130:
        g += [(False, False, True, False), (False, True, False, False)]
    return g
