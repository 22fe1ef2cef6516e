"""ctypes binding of libcfnerf_hip.so (include/cfnerf.h).  There is NO fallback: if the library is
missing or a call fails, a RuntimeError is raised."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CFNERF_LIB: development aid for same-box A/B runs of two builds of the SAME library (never a fallback)
LIB_PATH = os.environ.get("CFNERF_LIB") or os.path.join(HERE, "libcfnerf_hip.so")

F_TRAIN, F_LINDISP, F_WHITE_BKGD, F_STASH, F_EPS_ROWS, F_KSTATS_EXT, F_GEOMETRY, F_INPUT_GRAD = 1, 2, 4, 8, 16, 32, 64, 128
F_RAY_GRAD = 256
F_COTANGENTS = 512
F_SEAM_GRAD = 1024          # goes into the white_bkgd argument of cfnerf_composite_bwd, not into a flags argument
F_CULL = 0x800              # cfnerf_sample_points: pts is a Cull; cfnerf_composite_fwd: or-ed into white_bkgd, weights_opt is a SparseRaw
# CFNERF_F_EPS_GRAD (cfnerf_render_fwd / cfnerf_network_fwd with F_STASH: the backward also writes d_eps and d_eps_rows, eps_grad_offsets).  Not an
# ``F_`` name: tests/test_cull_cpu.py pins how many of those this module has
FLAG_EPS_GRAD = 0x1000
# CFNERF_F_RAY_REG (or-ed into the white_bkgd argument of cfnerf_composite_fwd: weights_opt is a RayReg).  Stored under a ``FLAG_`` name for the
# same reason; ``F_RAY_REG`` resolves to it through the module's __getattr__ below, so it is spelled like the header's without being counted
FLAG_RAY_REG = 0x2000
# CFNERF_F_KSCORES (or-ed into the white_bkgd argument of cfnerf_composite_fwd: weights_opt is a KScores); ``F_KSCORES`` resolves like ``F_RAY_REG``
FLAG_KSCORES = 0x4000


def __getattr__(name):
    if name == "F_RAY_REG":
        return FLAG_RAY_REG
    if name == "F_KSCORES":
        return FLAG_KSCORES
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def input_grad_offset(n_params: int) -> int:
    """x_off of include/cfnerf.h (CFNERF_F_INPUT_GRAD): where d_x starts in the grad_flat of cfnerf_network_bwd, in floats"""
    return (n_params + 63) // 64 * 64


def ray_grad_offsets(n_params: int, N: int, S: int):
    """(r_off, z_off, total) of include/cfnerf.h (CFNERF_F_RAY_GRAD), in floats: d_rays [N,11] starts at r_off and d_z [N,S] at z_off of the
    grad_flat of cfnerf_render_bwd, which then holds ``total`` floats"""
    r_off = (n_params + 63) // 64 * 64
    z_off = r_off + (N * 11 + 63) // 64 * 64
    return r_off, z_off, z_off + N * S


def eps_grad_offsets(base_end: int, n: int, K: int):
    """(e_off, er_off, total) of include/cfnerf.h (CFNERF_F_EPS_GRAD), in floats: d_eps [K,4] starts at e_off and d_eps_rows [n,K,4] at er_off
    of the backward's grad_flat, which then holds ``total`` floats.  ``base_end``: the end of the blocks the stash already asks for -
    ``n_params``, ``ray_grad_offsets(...)[2]`` with F_RAY_GRAD, ``input_grad_offset(n_params) + P * C`` with F_INPUT_GRAD; ``n``: rays or points"""
    e_off = (base_end + 63) // 64 * 64
    er_off = e_off + (4 * K + 63) // 64 * 64
    return e_off, er_off, er_off + n * K * 4


class Cfg(C.Structure):
    _fields_ = [("netdepth", C.c_int32), ("netwidth", C.c_int32), ("multires", C.c_int32),
                ("multires_views", C.c_int32), ("h_alpha_size", C.c_int32), ("h_rgb_size", C.c_int32),
                ("n_flows", C.c_int32)]


class Cotangents(C.Structure):
    """cfnerf_cotangents of include/cfnerf.h: the host struct of device pointers that the backward of a CFNERF_F_COTANGENTS stash takes in
    place of d_rgb_map (``cotangents_arg``)"""
    _fields_ = [("d_rgb_map", C.c_void_p), ("d_disp_map", C.c_void_p), ("d_weights", C.c_void_p), ("d_raw", C.c_void_p)]


def cotangents(d_rgb_map, d_disp_map=None, d_weights=None, d_raw=None):
    """A Cotangents of contiguous fp32 device tensors (None -> NULL).  Keep the tensors alive until the backward has run."""
    val = lambda t: None if t is None else ptr(t).value
    return Cotangents(val(d_rgb_map), val(d_disp_map), val(d_weights), val(d_raw))


def cotangents_arg(cot):
    """what goes into the d_rgb_map argument of cfnerf_render_bwd / _accumulate for a CFNERF_F_COTANGENTS stash: the struct's host address"""
    return C.cast(C.pointer(cot), C.c_void_p)


class CompositeGrads(C.Structure):
    """cfnerf_composite_grads of include/cfnerf.h: the host struct of device pointers that a CFNERF_F_SEAM_GRAD cfnerf_composite_bwd takes in
    place of d_raw (``composite_grads_arg``), naming what it writes"""
    _fields_ = [("d_raw", C.c_void_p), ("d_z_vals", C.c_void_p), ("d_rays_d", C.c_void_p)]


def composite_grads(d_raw=None, d_z_vals=None, d_rays_d=None):
    """A CompositeGrads of contiguous fp32 device tensors to write into (None -> NULL: not wanted)"""
    val = lambda t: None if t is None else ptr(t).value
    return CompositeGrads(val(d_raw), val(d_z_vals), val(d_rays_d))


def composite_grads_arg(out):
    """what goes into the d_raw argument of cfnerf_composite_bwd when F_SEAM_GRAD is or-ed into white_bkgd: the struct's host address"""
    return C.cast(C.pointer(out), C.c_void_p)


class Cull(C.Structure):
    """cfnerf_cull of include/cfnerf.h: the occupancy grid and the outputs of a CFNERF_F_CULL cfnerf_sample_points, passed in place of pts
    (``struct_arg``)"""
    _fields_ = [("occ_bits", C.c_void_p), ("lo", C.c_float * 3), ("scale", C.c_float * 3), ("res", C.c_int32 * 3), ("outside", C.c_int32),
                ("slot", C.c_void_p), ("ray_start", C.c_void_p), ("pts_c", C.c_void_p), ("ray_of", C.c_void_p)]


class SparseRaw(C.Structure):
    """cfnerf_sparse_raw of include/cfnerf.h: where the rows of a CFNERF_F_CULL cfnerf_composite_fwd's raw belong, passed in place of
    weights_opt (``struct_arg``)"""
    _fields_ = [("slot", C.c_void_p), ("ray_start", C.c_void_p), ("weights_opt", C.c_void_p)]


class RayReg(C.Structure):
    """cfnerf_ray_reg of include/cfnerf.h: the inputs and outputs of a CFNERF_F_RAY_REG cfnerf_composite_fwd, passed in place of weights_opt
    (``struct_arg``)"""
    _fields_ = [("weights", C.c_void_p), ("rays", C.c_void_p), ("lambda_dist", C.c_float), ("lambda_ent", C.c_float), ("acc_min", C.c_float),
                ("n_total", C.c_int64), ("d_weights", C.c_void_p), ("d_z_opt", C.c_void_p), ("scalars_out", C.c_void_p)]


def ray_reg(weights, z_vals, d_weights, scalars_out, rays=None, d_z=None, lambda_dist=0.0, lambda_ent=0.0, acc_min=0.1, n_total=0, stream_=None):
    """One CFNERF_F_RAY_REG launch on contiguous fp32 device tensors: weights [N,S,K], z_vals [N,S], rays [N,11] or None; writes d_weights [N,S,K],
    d_z [N,S] (or None) and the 8 floats of scalars_out ({reg, dist, ent, frac} first).  Nothing synchronises."""
    N, S, K = weights.shape
    rr = RayReg(dptr(weights), dptr(rays), lambda_dist, lambda_ent, acc_min, int(n_total), dptr(d_weights), dptr(d_z), dptr(scalars_out))
    check(lib().cfnerf_composite_fwd(None, ptr(z_vals), None, N, S, K, FLAG_RAY_REG, None, None, None, struct_arg(rr),
                                     stream() if stream_ is None else stream_), "cfnerf_composite_fwd(CFNERF_F_RAY_REG)")


class KScores(C.Structure):
    """cfnerf_kscores of include/cfnerf.h: the inputs and outputs of a CFNERF_F_KSCORES cfnerf_composite_fwd, passed in place of weights_opt
    (``struct_arg``)"""
    _fields_ = [("samples", C.c_void_p), ("target", C.c_void_p), ("sorted", C.c_void_p), ("quantiles", C.c_void_p), ("rank_code", C.c_void_p),
                ("pit", C.c_void_p), ("crps", C.c_void_p), ("n_levels", C.c_int32), ("level_lo", C.c_int32 * 16), ("level_frac", C.c_float * 16)]


def quantile_levels(levels, K):
    """The ``(lo, frac)`` pairs of include/cfnerf.h (CFNERF_F_KSCORES) for quantile levels ``q`` in [0,1] of K samples: ``lo = floor(q (K-1))`` in
    double, ``frac`` the fractional part rounded once to fp32 - the ``numpy.quantile(method="linear")`` position.  (A ``frac`` that rounds up
    to 1.0f is the next order statistic.)"""
    import math
    import struct
    out = []
    for q in levels:
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"a quantile level must lie in [0, 1], got {q!r}")
        pos = q * (K - 1)
        lo = int(math.floor(pos))
        frac = struct.unpack("f", struct.pack("f", pos - lo))[0]
        if frac >= 1.0:
            lo, frac = lo + 1, 0.0
        if lo >= K - 1:
            lo, frac = K - 1, 0.0
        out.append((lo, frac))
    return out


def k_scores(samples, M, K, target=None, sorted_out=None, quantiles=None, levels=(), rank_code=None, pit=None, crps=None, stream_=None):
    """One CFNERF_F_KSCORES launch on contiguous device tensors: samples [M,K] fp32, target [M] or None; writes the outputs that are given
    (sorted_out [M,K], quantiles [M,len(levels)], rank_code [M] int32, pit [M], crps [M]).  ``levels``: ``(lo, frac)`` pairs (``quantile_levels``).
    Nothing synchronises."""
    ks = KScores(dptr(samples), dptr(target), dptr(sorted_out), dptr(quantiles), dptr(rank_code), dptr(pit), dptr(crps), len(levels))
    for t, (lo, frac) in enumerate(levels[:16]):
        ks.level_lo[t], ks.level_frac[t] = lo, frac
    check(lib().cfnerf_composite_fwd(None, None, None, M, 1, K, FLAG_KSCORES, None, None, None, struct_arg(ks),
                                     stream() if stream_ is None else stream_), "cfnerf_composite_fwd(CFNERF_F_KSCORES)")


# CFNERF_MODE_SSIM (enum cfnerf_mode; or-ed into the white_bkgd argument of cfnerf_composite_fwd: weights_opt is an SSim)
MODE_SSIM = 0x8000
SSIM_TILE = 32              # CFNERF_SSIM_TILE


class SSim(C.Structure):
    """cfnerf_ssim of include/cfnerf.h: the inputs and outputs of a CFNERF_MODE_SSIM cfnerf_composite_fwd, passed in place of weights_opt
    (``struct_arg``)"""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("ssim_map", C.c_void_p), ("mean", C.c_void_p), ("scratch", C.c_void_p),
                ("H", C.c_int32), ("W", C.c_int32), ("win", C.c_int32), ("cov_norm", C.c_double), ("c1", C.c_double), ("c2", C.c_double),
                ("taps", C.c_float * 15)]


def ssim_scratch_floats(B, C_, H, W, win):
    """CFNERF_SSIM_SCRATCH_FLOATS of include/cfnerf.h: the floats of SSim.scratch (two per 32 x 32 tile, image and channel)"""
    return 2 * B * C_ * ((H - win) // SSIM_TILE + 1) * ((W - win) // SSIM_TILE + 1)


def ssim_window(kind="uniform", win=None, sigma=1.5):
    """``(taps, cov_norm)`` of a CFNERF_MODE_SSIM window, the taps as Python floats that are exact fp32 values.  ``"uniform"``: ``win``
    (default 7) equal taps and the sample covariance ``n / (n - 1)``, ``n = win ** 2`` - skimage's default.  ``"gaussian"``: ``exp(-i^2 / (2
    sigma^2))`` on ``-r .. r``, normalised in double and rounded once to fp32, ``cov_norm = 1`` - ``gaussian_weights=True``; ``win`` defaults
    to ``2 int(3.5 sigma + 0.5) + 1`` (11 at sigma = 1.5)."""
    import math
    import struct
    if kind not in ("uniform", "gaussian"):
        raise ValueError(f"window must be 'uniform' or 'gaussian', got {kind!r}")
    if kind == "gaussian" and not sigma > 0:
        raise ValueError(f"sigma must be positive, got {sigma!r}")
    if win is None:
        win = 7 if kind == "uniform" else 2 * int(3.5 * sigma + 0.5) + 1
    win = int(win)
    if win % 2 == 0 or not 3 <= win <= 15:
        raise ValueError(f"the window must have an odd number of taps in [3, 15], got {win}")
    if kind == "uniform":
        taps, cov = [1.0 / win] * win, win * win / (win * win - 1.0)
    else:
        r = (win - 1) // 2
        w = [math.exp(-0.5 / (sigma * sigma) * i ** 2) for i in range(-r, r + 1)]
        tot = math.fsum(w)
        taps, cov = [v / tot for v in w], 1.0
    return [struct.unpack("f", struct.pack("f", t))[0] for t in taps], cov


def ssim(x, y, B, H, W, C_, taps, cov_norm, c1, c2, ssim_map=None, mean=None, scratch=None, stream_=None):
    """One CFNERF_MODE_SSIM call on contiguous fp32 device tensors x, y [B,H,W,C]: writes the outputs that are given (ssim_map
    [B,H-win+1,W-win+1,C], mean [B,C]); ``scratch``: ``ssim_scratch_floats`` floats, needed with mean.  Nothing synchronises."""
    s = SSim(dptr(x), dptr(y), dptr(ssim_map), dptr(mean), dptr(scratch), H, W, len(taps), cov_norm, c1, c2)
    for i, t in enumerate(taps[:15]):
        s.taps[i] = t
    check(lib().cfnerf_composite_fwd(None, None, None, B, 1, C_, MODE_SSIM, None, None, None, struct_arg(s),
                                     stream() if stream_ is None else stream_), "cfnerf_composite_fwd(CFNERF_MODE_SSIM)")


def struct_arg(st):
    """the host address of a descriptor struct, as the pointer argument it replaces"""
    return C.cast(C.pointer(st), C.c_void_p)


def dptr(t):
    """Device pointer of a contiguous tensor of any dtype (None -> NULL): the integer members of Cull / SparseRaw"""
    if t is None:
        return None
    assert t.is_contiguous(), t.shape
    return t.data_ptr() or None


_P = C.c_void_p
_SIGS = {
    "cfnerf_version": (C.c_int, []),
    "cfnerf_last_error": (C.c_char_p, []),
    "cfnerf_param_count": (C.c_int64, [C.POINTER(Cfg)]),
    "cfnerf_param_offset": (C.c_int64, [C.POINTER(Cfg), C.c_char_p, C.POINTER(C.c_int64)]),
    "cfnerf_param_key": (C.c_char_p, [C.POINTER(Cfg), C.c_int]),
    "cfnerf_model_create": (C.c_int, [C.POINTER(Cfg), C.POINTER(_P)]),
    "cfnerf_model_destroy": (C.c_int, [_P]),
    "cfnerf_model_set_params": (C.c_int, [_P, _P, _P]),
    "cfnerf_rays_setup": (C.c_int, [C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), _P, _P, C.c_int64, C.c_int64, C.c_int,
                                    C.c_float, C.c_float, _P, _P]),
    "cfnerf_ndc_rays": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, _P, _P, C.c_int64, _P, _P, _P]),
    "cfnerf_embed": (C.c_int, [_P, C.c_int64, C.c_int, _P, _P]),
    "cfnerf_sample_points": (C.c_int, [_P, _P, _P, C.c_int, C.c_int64, C.c_int, _P, _P, _P]),
    "cfnerf_render_fwd": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P,
                                    _P, _P, _P]),
    "cfnerf_render_eval": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "cfnerf_sample_pdf": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P]),
    "cfnerf_network_fwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P]),
    "cfnerf_composite_fwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P]),
    "cfnerf_loss_fwd_bwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_float, C.c_int64, _P, _P, _P]),
    "cfnerf_workspace_bytes": (C.c_int64, [C.POINTER(Cfg), C.c_int64, C.c_int, C.c_int]),
    "cfnerf_model_set_workspace": (C.c_int, [_P, _P, C.c_size_t]),
    "cfnerf_model_stash_generation": (C.c_uint64, [_P]),
    "cfnerf_render_bwd": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P]),
    "cfnerf_render_bwd_accumulate": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P, _P]),
    "cfnerf_network_bwd": (C.c_int, [_P, C.c_uint64, _P, _P, _P, _P]),
    "cfnerf_composite_bwd": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    "cfnerf_grad_early_ranges": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int]),
    "cfnerf_stream_wait_grad_early": (C.c_int, [_P, _P]),
    "cfnerf_adam_step": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_float, C.c_float, _P]),
    "cfnerf_model_set_precision": (C.c_int, [_P, C.c_int]),
    "cfnerf_model_set_flow_math": (C.c_int, [_P, C.c_int]),
    "cfnerf_model_workspace_bytes": (C.c_int64, [_P]),
    "cfnerf_timing_enable": (C.c_int, [_P, C.c_int]),
    "cfnerf_timing_last_ms": (C.c_float, [_P, C.c_int]),
    "cfnerf_timing_fwd_mean_ms": (C.c_float, [_P, C.c_int]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def lib():
    """Load (once) and return the shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python cf-nerf_amd/build.py` (needs hipcc). "
                "The CF-NeRF hot path has no CPU or PyTorch fallback.")
        override = bool(os.environ.get("CFNERF_LIB"))
        if override:
            import sys
            print(f"cf-nerf_amd: warning: CFNERF_LIB is set - loading {LIB_PATH} instead of the in-tree libcfnerf_hip.so "
                  "(development aid for same-box A/B runs of two builds)", file=sys.stderr, flush=True)
        l = C.CDLL(LIB_PATH)
        skipped = []
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(l, name)  # AttributeError here = header / library out of sync
            except AttributeError:
                if override:
                    skipped.append(name)   # (an OLDER build under the A/B override: entry points added since are simply absent there)
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        if skipped:
            print("cf-nerf_amd: warning: entry points absent from the CFNERF_LIB build: " + ", ".join(skipped), file=sys.stderr, flush=True)
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().cfnerf_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed (status {rc}): {msg}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL).  The tensor must be contiguous fp32."""
    if t is None:
        return None
    assert t.is_contiguous() and t.dtype.is_floating_point and t.element_size() == 4, (t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
