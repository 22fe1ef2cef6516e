"""Host-side mirror of the reference's hot-path interface, backed by libcfnerf_hip.so.

Same names, argument order, defaults and return structure as the reference
(RUN = run_nerf_uncertainty_NF.py, HLP = run_nerf_helpers.py, MOD = model/models.py):

    render            RUN:103-170      render_rays     RUN:457-553
    run_network       RUN:67-85        raw2outputs     RUN:411-454
    batchify(_rays)   RUN:47-64,88-100 create_nerf     RUN:317-409
    NeRF_Flows        MOD:13-291       get_embedder    HLP:54-69
    get_rays/ndc_rays HLP:288-297,360-377   img2mse/mse2psnr HLP:15-16

All arithmetic of the path runs in hand-written HIP kernels; PyTorch only owns device memory,
streams, autograd plumbing and the optimiser.  There is no CPU / eager fallback: every function
raises if the library is missing or the tensors are not on a GPU.

Extra (new) keyword arguments make the reference's hidden randomness explicit:
``t_rand [N,S]``, ``eps_alpha [K,1]``, ``eps_rgb [K,3]``.  When left ``None`` they are drawn with
torch in the reference's order.  ``latents.py`` is the one description of that order, of the ``[K,4]`` layout and of the
reference-exact per-netchunk latents (opt-in, ``create_nerf`` with ``args.latent_draws = "netchunk"``; explicit latents are then
``eps_alpha [C,K,1]`` / ``eps_rgb [C,K,3]``, one pair per netchunk); every train launch here takes its latents from
``latents.train_latents``.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib as L
from . import latents as LT
from .latents import LATENT_DRAWS, draw_train_randomness, netchunk_count, netchunk_eps_point_rows, netchunk_eps_rows    # noqa: F401  (public here too)

# --------------------------------------------------------------------------------------------
# misc helpers (HLP:15-16)
img2mse = lambda x, y: torch.mean((x - y) ** 2)
mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))


def _need_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on the GPU: the CF-NeRF hot path is HIP-only (no CPU fallback)")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


# --------------------------------------------------------------------------------------------
# positional encoding (HLP:21-69).  Used only by the unfused run_network path and by callers that
# want the embedding itself; the fused kernels encode on-chip.
def _embed_fwd(x, multires, out_dim):
    out = torch.empty(x.shape[0], out_dim, device=x.device)
    L.check(L.lib().cfnerf_embed(L.ptr(x), x.shape[0], multires, L.ptr(out), L.stream()), "cfnerf_embed")
    return out


class _EmbedFn(torch.autograd.Function):
    """Embedder.embed as an autograd node (the reference's is a torch graph, HLP:21-69): the cfnerf_embed kernel forward; the adjoint is a
    few torch ops on the SAVED output, no second transcendental pass - with out = [x | sin(f_l x), cos(f_l x) ...],
    d_in = d_out[:, :3] + sum_l f_l (cos_l d_sin_l - sin_l d_cos_l)."""

    @staticmethod
    def forward(ctx, x, multires, out_dim, freq_bands):
        out = _embed_fwd(_f32c(x), multires, out_dim)
        ctx.save_for_backward(out)
        ctx.freq_bands = freq_bands
        return out

    @staticmethod
    def backward(ctx, d_out):
        (out,) = ctx.saved_tensors
        return embed_backward(out, d_out, ctx.freq_bands), None, None, None


def embed_backward(out, d_out, freq_bands):
    """d loss / d inputs [P,3] of the positional encoding from its own output ``out [P, 3 + 6 L]`` and ``d_out`` (any device)"""
    P, n = out.shape[0], freq_bands.numel()
    o = out[:, 3:].reshape(P, n, 2, 3)                             # [:, l, 0] = sin(f_l x), [:, l, 1] = cos(f_l x)  (HLP:40-44)
    g = d_out[:, 3:].reshape(P, n, 2, 3)
    f = freq_bands.to(device=out.device, dtype=out.dtype)[None, :, None]
    return d_out[:, :3] + ((o[:, :, 1] * g[:, :, 0] - o[:, :, 0] * g[:, :, 1]) * f).sum(1)


class Embedder:
    def __init__(self, multires: int, input_dims: int = 3):
        self.multires = multires
        self.input_dims = input_dims
        self.out_dim = input_dims * (1 + 2 * multires)
        self.freq_bands = 2. ** torch.linspace(0., multires - 1, steps=multires)     # HLP:38

    def embed(self, inputs: torch.Tensor) -> torch.Tensor:
        _need_gpu(inputs, "Embedder input")                                           # HIP kernel only (cfnerf_embed)
        if inputs.shape[-1] != self.input_dims or self.input_dims != 3:
            raise ValueError("Embedder encodes 3-vectors (HLP:57-64: input_dims = 3)")
        if torch.is_grad_enabled() and inputs.requires_grad:      # a learnable front end (pose, deformation ...) trains through the encoding
            out = _EmbedFn.apply(inputs.reshape(-1, 3).to(torch.float32), self.multires, self.out_dim, self.freq_bands)
        else:
            out = _embed_fwd(_f32c(inputs.reshape(-1, 3)), self.multires, self.out_dim)
        return out.reshape(list(inputs.shape[:-1]) + [self.out_dim])


def get_embedder(multires, i=0):
    if i == -1:
        return nn.Identity(), 3                                                       # HLP:55-56
    eo = Embedder(multires)
    fn = lambda x, eo=eo: eo.embed(x)
    fn.multires = multires
    return fn, eo.out_dim


# --------------------------------------------------------------------------------------------
# ray helpers (HLP:288-297, 360-377) as standalone calls: the same kernels render() uses (cfnerf_rays_setup with a pose,
# cfnerf_ndc_rays).  GPU only, like everything else here.
def _pose_arg(c2w):
    """A [3,4] pose as the `const float* c2w_host` argument.  A pose that already lives on the host is passed as it is
    (no copy when it is contiguous fp32); a device pose is fetched once (the call needs it on the host: it travels in
    the kernel arguments).  Returns (ctypes pointer, keep-alive tensor)."""
    t = torch.as_tensor(c2w)
    if t.is_cuda:
        t = t.detach().cpu()
    t = t.detach()[:3, :4].to(torch.float32).contiguous()
    return C.cast(t.data_ptr(), C.POINTER(C.c_float)), t


def _device_of(*ts, default=None):
    for t in ts:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device()) if default is None else default


def _pack_rays(H, W, focal, c2w=None, rays=None, n=None, pixel0=0, ndc=False, near=0., far=1., out=None, device=None):
    """The packed ray batch every launch reads, ``[n, 11]`` = o3, d3, near, far, viewdir3 (RUN:504-507), on
    ``cfnerf_rays_setup``: from a pose (pixels ``pixel0 .. pixel0 + n`` of the H x W image, default all of it) or from
    explicit ``rays=(rays_o, rays_d)``.  ``near`` / ``far`` are numbers or per-ray tensors.  Written into ``out`` when given
    (a persistent [n, 11] buffer), else into a new tensor on ``device`` (rays mode: the rays' device)."""
    if c2w is not None:
        arr, _keep = _pose_arg(c2w)
        ro = rd = None
        n = int(H) * int(W) if n is None else n
    else:
        arr = None
        ro, rd = _f32c(rays[0].reshape(-1, 3)), _f32c(rays[1].reshape(-1, 3))
        n, device = rd.shape[0], rd.device
    if out is None:
        out = torch.empty(n, 11, device=device)
    nf, ff = (near if not torch.is_tensor(near) else 0.), (far if not torch.is_tensor(far) else 1.)
    L.check(L.lib().cfnerf_rays_setup(int(H), int(W), float(focal), arr, L.ptr(ro), L.ptr(rd), n, pixel0, int(bool(ndc)), float(nf), float(ff),
                                      L.ptr(out), L.stream()), "cfnerf_rays_setup")
    if torch.is_tensor(near):
        out[:, 6] = near.reshape(-1).to(out)
    if torch.is_tensor(far):
        out[:, 7] = far.reshape(-1).to(out)
    return out


def pack_rays_reference(H, W, focal, rays=None, c2w=None, ndc=False, near=0., far=1.):
    """RUN:129-158 with get_rays (HLP:288-297) and ndc_rays (HLP:360-377, near = 1 as RUN:149 calls it) in plain torch, in the dtype and on
    the device of its inputs: the closed form ``pack_rays`` differentiates (and what the CPU tests hold to the oracle).  ``[n,11]``."""
    if c2w is not None:
        dt, dev = c2w.dtype, c2w.device
        i, j = torch.meshgrid(torch.arange(int(W), dtype=dt, device=dev), torch.arange(int(H), dtype=dt, device=dev), indexing="xy")
        dirs = torch.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -torch.ones_like(i)], -1)          # HLP:292
        rays_d = torch.sum(dirs[..., None, :] * c2w[:3, :3], -1)                                             # HLP:294
        rays_o = c2w[:3, -1].expand(rays_d.shape)                                                            # HLP:296
    else:
        rays_o, rays_d = rays
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)                                             # RUN:143 (before NDC)
    if ndc:
        t = -(1. + rays_o[..., 2]) / rays_d[..., 2]                                                          # HLP:362
        rays_o = rays_o + t[..., None] * rays_d
        cw, chh = -1. / (W / (2. * focal)), -1. / (H / (2. * focal))
        oz = rays_o[..., 2]
        o = torch.stack([cw * rays_o[..., 0] / oz, chh * rays_o[..., 1] / oz, 1. + 2. / oz], -1)             # HLP:366-368
        d = torch.stack([cw * (rays_d[..., 0] / rays_d[..., 2] - rays_o[..., 0] / oz),
                         chh * (rays_d[..., 1] / rays_d[..., 2] - rays_o[..., 1] / oz), -2. / oz], -1)       # HLP:370-372
        rays_o, rays_d = o, d
    one = torch.ones_like(rays_d[..., :1])
    nr = near.reshape(-1, 1).to(one) if torch.is_tensor(near) else near * one                                # RUN:155
    fr = far.reshape(-1, 1).to(one) if torch.is_tensor(far) else far * one
    return torch.cat([rays_o, rays_d, nr, fr, viewdirs], -1)                                                 # RUN:156-158


class _PackRaysFn(torch.autograd.Function):
    """``pack_rays`` as an autograd node: the forward is the cfnerf_rays_setup kernel (the bits every launch reads), the backward the
    closed form above differentiated by torch in fp32 on the device - a few elementwise ops per ray, once per step."""

    @staticmethod
    def forward(ctx, a, b, H, W, focal, from_pose, ndc, near, far):
        ctx.cfg = (H, W, focal, from_pose, ndc, near, far)
        ctx.save_for_backward(a, b) if not from_pose else ctx.save_for_backward(a)
        if from_pose:
            dev = a.device if a.is_cuda else torch.device("cuda", torch.cuda.current_device())
            with torch.cuda.device(dev):
                return _pack_rays(H, W, focal, c2w=a, ndc=ndc, near=near, far=far, device=dev)
        return _pack_rays(H, W, focal, rays=(a, b), ndc=ndc, near=near, far=far)

    @staticmethod
    def backward(ctx, d_packed):
        H, W, focal, from_pose, ndc, near, far = ctx.cfg
        leaves = [t.detach().to(d_packed.device, torch.float32).requires_grad_(True) for t in ctx.saved_tensors]
        with torch.enable_grad():
            out = pack_rays_reference(H, W, focal, c2w=leaves[0], ndc=ndc, near=near, far=far) if from_pose else \
                pack_rays_reference(H, W, focal, rays=(leaves[0], leaves[1]), ndc=ndc, near=near, far=far)
        g = torch.autograd.grad(out, leaves, d_packed.to(out.dtype))
        g = [gi.to(t.device).reshape(t.shape) for gi, t in zip(g, ctx.saved_tensors)]
        return (g[0], None if from_pose else g[1]) + (None,) * 7


def pack_rays(H, W, focal, rays=None, c2w=None, ndc=False, near=0., far=1.):
    """The packed ray batch ``[n,11]`` = o3, d3, near, far, viewdir3 that every launch reads (RUN:129-158), from explicit
    ``rays=(rays_o, rays_d)`` or from a pose ``c2w [3,4]`` (all H x W pixels, row-major), DIFFERENTIABLE in them: the forward is the ray
    set-up kernel with its unchanged bits; gradients reach ``rays_o`` / ``rays_d`` / ``c2w`` through ``get_rays``, the view-direction
    normalisation and ``ndc_rays`` in closed form.  ``packed.backward(d_rays)`` chains a ``d_rays [n,11]`` (``render_rays``' gradient, or
    ``train.Trainer(ray_grad=True).d_rays``) into a pose.  ``near`` / ``far``: numbers or per-ray tensors (constants)."""
    if (rays is None) == (c2w is None):
        raise ValueError("pack_rays takes either rays=(rays_o, rays_d) or c2w=")
    if c2w is not None:
        c2w = torch.as_tensor(c2w)
        pose = c2w[:3, :4].to(torch.float32)
        return _PackRaysFn.apply(pose, None, int(H), int(W), float(focal), True, bool(ndc), near, far)
    _need_gpu(rays[1], "rays")
    ro, rd = rays[0].reshape(-1, 3).to(torch.float32), rays[1].reshape(-1, 3).to(torch.float32)
    return _PackRaysFn.apply(ro, rd, int(H), int(W), float(focal), False, bool(ndc), near, far)


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts)


def sample_points_reference(ray_batch, t_vals, t_rand=None, lindisp=False):
    """RUN:510-534 in plain torch, in the dtype and on the device of ``ray_batch [N,11]``: near / far -> ``z_vals [N,S]`` (both ``lindisp``
    forms, the jitter lines when ``t_rand [N,S]`` is given) and ``pts [N,S,3] = o + d z``.  The closed form the unfused seam's sampling node
    differentiates (and what the CPU tests hold to the oracle); returns ``(z_vals, pts)``."""
    rays_o, rays_d = ray_batch[:, 0:3], ray_batch[:, 3:6]
    near, far = ray_batch[:, 6:7], ray_batch[:, 7:8]
    t = t_vals.to(ray_batch)
    if not lindisp:
        z_vals = near * (1. - t) + far * t                                                                   # RUN:512
    else:
        z_vals = 1. / (1. / near * (1. - t) + 1. / far * t)                                                  # RUN:514
    z_vals = z_vals.expand([ray_batch.shape[0], t.shape[0]])                                                 # RUN:516
    if t_rand is not None:
        mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])                                                     # RUN:520
        upper = torch.cat([mids, z_vals[..., -1:]], -1)
        lower = torch.cat([z_vals[..., :1], mids], -1)
        z_vals = lower + (upper - lower) * t_rand.to(ray_batch)                                              # RUN:532
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]                                 # RUN:534
    return z_vals, pts


def _sample_points(rays, t_vals, t_rand, lindisp):
    """cfnerf_sample_points of the packed fp32 ``rays [N,11]`` into new ``z_vals [N,S], pts [N,S,3]`` (RUN:510-534)"""
    N, S = rays.shape[0], t_vals.shape[0]
    z_vals = torch.empty(N, S, device=rays.device)
    pts = torch.empty(N, S, 3, device=rays.device)
    L.check(L.lib().cfnerf_sample_points(L.ptr(rays), L.ptr(t_vals), L.ptr(t_rand), L.F_LINDISP if lindisp else 0, N, S, L.ptr(z_vals),
                                         L.ptr(pts), L.stream()), "cfnerf_sample_points")
    return z_vals, pts


class _SamplePointsFn(torch.autograd.Function):
    """The unfused seam's sampling as an autograd node: the forward is the cfnerf_sample_points kernel (its unchanged bits), the backward
    ``sample_points_reference`` differentiated by torch in fp32 on the device - N S 3 floats, elementwise.  ``(d_z, d_pts)`` reach all
    eleven columns of ``d ray_batch``, near and far included (the view directions' three get zeros here: they are sliced off the rays)."""

    @staticmethod
    def forward(ctx, rays, t_vals, t_rand, lindisp):
        ctx.lindisp = lindisp
        ctx.t_rand = t_rand
        ctx.save_for_backward(rays, t_vals)
        return _sample_points(_f32c(rays), t_vals, t_rand, lindisp)

    @staticmethod
    def backward(ctx, d_z, d_pts):
        rays, t_vals = ctx.saved_tensors
        leaf = rays.detach().to(torch.float32).requires_grad_(True)
        with torch.enable_grad():
            z, pts = sample_points_reference(leaf, t_vals, ctx.t_rand, ctx.lindisp)
        (g,) = torch.autograd.grad((z, pts), (leaf,), (d_z.to(z.dtype), d_pts.to(pts.dtype)))
        return g.to(rays.dtype), None, None, None


def get_rays(H, W, focal, c2w):
    """HLP:288-297 on the ray set-up kernel: ``rays_o, rays_d [H,W,3]`` on the GPU (of ``c2w`` if it lives on one, else the
    current device)."""
    H, W = int(H), int(W)
    dev = _device_of(c2w)
    with torch.cuda.device(dev):
        packed = _pack_rays(H, W, focal, c2w=c2w, device=dev)
    return packed[:, 0:3].reshape(H, W, 3), packed[:, 3:6].reshape(H, W, 3)


def get_rays_by_coord(H, W, focal, c2w, coords):
    """Rays through FRACTIONAL pixel coordinates ``coords [n,2] = (x, y)`` of the view ``c2w [3,>=4]`` (HLP:440-445, the key-point rays
    of depth supervision): ``rays_o, rays_d [n,3]`` fp32 on ``coords``' device.  Plain torch: it runs once per view when a
    data.DepthRayPool is built, never per step."""
    coords = torch.as_tensor(coords)
    dev = coords.device
    coords = coords.to(torch.float32)
    c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
    x, y = (coords[:, 0] - W * .5) / focal, -(coords[:, 1] - H * .5) / focal
    dirs = torch.stack([x, y, -torch.ones_like(x)], -1)
    rays_d = torch.sum(dirs[:, None, :] * c2w[:3, :3], -1)
    return c2w[:3, -1].expand(rays_d.shape), rays_d


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """HLP:360-377 on ``cfnerf_ndc_rays``."""
    _need_gpu(rays_d, "rays_d")
    ro, rd = _f32c(rays_o.reshape(-1, 3)), _f32c(rays_d.reshape(-1, 3))
    o, d = torch.empty_like(ro), torch.empty_like(rd)
    L.check(L.lib().cfnerf_ndc_rays(int(H), int(W), float(focal), float(near), L.ptr(ro), L.ptr(rd), ro.shape[0], L.ptr(o), L.ptr(d),
                                    L.stream()), "cfnerf_ndc_rays")
    return o.reshape(rays_o.shape), d.reshape(rays_d.shape)


_T_VALS_CACHE = {}


def t_vals_table(device=None) -> torch.Tensor:
    """The hard-coded 96 + 32 = 128 sample table of RUN:510 (computed on the CPU like the reference; the device copy
    is made once per device - treat it as read-only)."""
    key = str(torch.device(device)) if device is not None else "cpu"
    t = _T_VALS_CACHE.get(key)
    if t is None:
        t = torch.cat([torch.linspace(0., 0.5, steps=97)[:-1], torch.linspace(0.5, 1., steps=32)], 0)
        if device is not None:
            t = t.to(device)
        _T_VALS_CACHE[key] = t
    return t


# --------------------------------------------------------------------------------------------
# parameter layout (mirror of cfnerf_param_key / cfnerf_param_offset)
def _cfg_struct(netdepth, netwidth, multires, multires_views, h_alpha_size, h_rgb_size, n_flows) -> L.Cfg:
    return L.Cfg(int(netdepth), int(netwidth), int(multires), int(multires_views), int(h_alpha_size),
                 int(h_rgb_size), int(n_flows))


def param_layout(cfg: L.Cfg):
    """OrderedDict key -> (offset, shape) in the flat parameter buffer, as the C ABI defines it."""
    lib = L.lib()
    total = lib.cfnerf_param_count(C.byref(cfg))
    if total < 0:
        raise RuntimeError("unsupported configuration: " + lib.cfnerf_last_error().decode())
    out = OrderedDict()
    i = 0
    W, D = cfg.netwidth, cfg.netdepth
    while True:
        k = lib.cfnerf_param_key(C.byref(cfg), i)
        if k is None:
            break
        key = k.decode()
        n = C.c_int64(0)
        off = lib.cfnerf_param_offset(C.byref(cfg), k, C.byref(n))
        out[key] = (int(off), int(n.value))
        i += 1
    return out, int(total)


def _shape_of(key: str, numel: int, cfg: L.Cfg):
    if key.endswith(".weight"):
        W, ic, icv = cfg.netwidth, 3 + 6 * cfg.multires, 3 + 6 * cfg.multires_views
        rows = {"views_linears.0.weight": W // 2, "feature_linear.weight": W, "alpha_linear.weight": 1,
                "alpha_std_linear.weight": 1, "h_alpha_linear.weight": cfg.h_alpha_size,
                "h_rgb_linear.weight": cfg.h_rgb_size}.get(key)
        if rows is None:
            if key.startswith("pts_linears."):
                rows = W
            elif key.startswith("flows_rgb."):
                rows = cfg.n_flows * (9 if ".amor_d." in key else 3)
            else:
                rows = cfg.n_flows
        return (rows, numel // rows)
    return (numel,)


# --------------------------------------------------------------------------------------------
def flow_buffers(n_flows, device="cpu"):
    """The registered buffers of the reference's two flow stacks (MOD:323-333, FLW:180-181), which its ``state_dict()`` carries next to
    the parameters: key -> tensor.  Device-free host logic (a checkpoint this build writes holds exactly the reference's key set:
    ``param_layout`` keys + these)."""
    out = OrderedDict()
    for name, z in (("flows_rgb", 3), ("flows_alpha", 1)):
        out[f"{name}.flip_idx"] = torch.arange(z - 1, -1, -1, device=device).long()             # MOD:323
        out[f"{name}.triu_mask"] = torch.triu(torch.ones(z, z, device=device), diagonal=1)[None, :, :, None]
        out[f"{name}.diag_idx"] = torch.arange(0, z, device=device).long()
        for k in range(n_flows):
            out[f"{name}.flow_{k}.diag_idx"] = torch.arange(0, z, device=device).long()         # FLW:180-181
    return out


@torch.no_grad()
def reference_init(shapes, netdepth, K_samples=None):
    """Initial values exactly as ``NeRF_Flows.__init__`` produces them under the same ``torch.manual_seed``
    (MOD:38-67, 339-350).  Throw-away CPU ``nn.Linear``s are created in the reference's construction order, so torch's
    own default init (U(+-1/sqrt(fan_in)) for weight and bias) consumes the CPU generator identically, and the fixed
    latents are drawn at the same point of the stream (MOD:50-55: after ``views_linears``, before ``feature_linear``).

    ``shapes``: key -> shape in state_dict order.  Returns ``(values, (sample_alpha, sample_rgb) | None)``; with
    ``K_samples=None`` the latent draws are skipped (re-initialisation of an existing module)."""
    vals = OrderedDict()

    def lin(prefix):
        out_f, in_f = shapes[prefix + ".weight"]
        l = nn.Linear(in_f, out_f)
        vals[prefix + ".weight"], vals[prefix + ".bias"] = l.weight.detach(), l.bias.detach()

    for i in range(netdepth):
        lin(f"pts_linears.{i}")                                            # MOD:38-39
    lin("views_linears.0")                                                 # MOD:42
    vals["alpha_mean"], vals["alpha_std"] = torch.zeros(1), torch.ones(1)  # MOD:44-45
    vals["rgb_mean"], vals["rgb_std"] = torch.zeros(3), torch.ones(3)      # MOD:47-48
    latents = None
    if K_samples is not None:
        # MOD:50-51: two `intepolation_*` latents come first.  They only feed NeRF_Flows.interpolation, which - like
        # .sample - cannot run in the reference (both call the flows without the required is_test argument), so the
        # draws are made for the RNG stream and dropped.
        torch.empty([2, 1]).normal_()
        torch.empty([2, 3]).normal_()
        latents = (torch.empty([K_samples, 1]).normal_(), torch.empty([K_samples, 3]).normal_())     # MOD:54-55
    for name in ("feature_linear", "alpha_linear", "alpha_std_linear", "h_alpha_linear", "h_rgb_linear"):
        lin(name)                                                          # MOD:58-62
    for flow in ("flows_rgb", "flows_alpha"):                              # MOD:66-67
        for name in ("amor_d", "amor_diag1.0", "amor_diag2.0", "amor_b"):
            lin(f"{flow}.{name}")                                          # MOD:339-350
    missing = set(shapes) - set(vals)
    if missing:
        raise RuntimeError(f"reference_init: no rule for {sorted(missing)}")
    return vals, latents


# --------------------------------------------------------------------------------------------
def _latents(model, explicit, train, device):
    """[K,4] latents of a launch that takes ONE set: the packed explicit one when given, else fresh train draws or the fixed eval ones."""
    if explicit is not None and explicit.dim() == 3:
        raise ValueError("per-netchunk latents [C,K,1] / [C,K,3] cannot be one launch's [K,4] set (train branch of render_rays / "
                         "NeRF_Flows.forward only; the eval branch uses the fixed latents)")
    if explicit is not None:
        return explicit.to(device).contiguous()
    return model.draw_eps() if train else model.eval_eps()


class NeRF_Flows(nn.Module):
    """Drop-in for the reference's ``NeRF_Flows`` (MOD:13-291).

    All parameters live in ONE flat fp32 tensor ``self.flat`` (the layout of ``state_dict()``),
    which is what the kernels, the gradient all-reduce and the fused Adam work on.
    ``state_dict()`` / ``load_state_dict()`` speak the reference's key names (with the buffers
    ``flip_idx`` / ``triu_mask`` / ``diag_idx``), so released checkpoints load unchanged.
    """

    def __init__(self, args):
        super().__init__()
        self.D = args.netdepth
        self.W = args.netwidth
        self.input_ch = args.input_ch
        self.input_ch_views = args.input_ch_views
        self.K_samples = args.K_samples
        self.skips = args.skips
        self.use_viewdirs = args.use_viewdirs
        self.h_alpha_size = args.h_alpha_size
        self.h_rgb_size = args.h_rgb_size
        args.z_size = 3                                            # MOD:31
        self.z_size = 3
        self.n_flows = args.n_flows
        self.type_flows = getattr(args, "type_flows", "triangular")
        self.n_hidden = getattr(args, "n_hidden", 128)
        dev = torch.device(getattr(args, "device", "cuda"))
        if dev.type != "cuda":
            raise RuntimeError("NeRF_Flows needs a GPU device: the CF-NeRF hot path is HIP-only")
        self.device = dev
        if not self.use_viewdirs:
            # the reference crashes later with an AttributeError (MOD:63-64,183-186); reject up front
            raise ValueError("use_viewdirs=False is not supported (the reference's NeRF_Flows cannot run it either)")
        if list(self.skips) != [self.D / 2]:
            # the float division matters: for an odd netdepth nothing matches `i in skips` and there is no skip concat
            raise ValueError(f"skips must be [netdepth / 2] (RUN:327), got {self.skips}")
        if (self.input_ch - 3) % 6 or (self.input_ch_views - 3) % 6:
            raise ValueError("input_ch / input_ch_views must come from get_embedder (3 + 6*multires)")
        self.cfg = _cfg_struct(self.D, self.W, (self.input_ch - 3) // 6, (self.input_ch_views - 3) // 6,
                               self.h_alpha_size, self.h_rgb_size, self.n_flows)
        self.layout, n_params = param_layout(self.cfg)
        self.n_params = n_params
        self.flat = nn.Parameter(torch.zeros(n_params, dtype=torch.float32, device=dev))
        self.sample_size = args.K_samples
        self._replay_reference_init(draw_latents=True)
        h = C.c_void_p()
        L.check(L.lib().cfnerf_model_create(C.byref(self.cfg), C.byref(h)), "cfnerf_model_create")
        self._h = h
        self._packed_version = None
        self._next_eps = None          # the launch's latents, handed from render_rays through an unfused network_query_fn to forward()
        self.latent_draws = "launch"   # "netchunk": per-netchunk train latents like the reference (create_nerf: args.latent_draws)
        self.netchunk = 1024 * 64      # points per network call of the reference (netchunk_per_gpu * n_gpus, RUN:82,384)
        self._ws = None                # train-step workspace: a torch-owned block lent to the library

    # ---- parameters ------------------------------------------------------------------------
    def view(self, key: str) -> torch.Tensor:
        off, n = self.layout[key]
        return self.flat.data[off:off + n].view(_shape_of(key, n, self.cfg))

    @torch.no_grad()
    def _replay_reference_init(self, draw_latents: bool):
        shapes = OrderedDict((k, tuple(self.view(k).shape)) for k in self.layout)
        vals, latents = reference_init(shapes, self.D, self.sample_size if draw_latents else None)
        for k, v in vals.items():
            self.view(k).copy_(v)
        if draw_latents:
            self.sample_alpha, self.sample_rgb = latents    # eval latents: plain attributes, NOT in state_dict
        self._dirty = True
        self.params_serial += 1             # (writes through .data views do not move flat._version)

    def reset_parameters(self):
        """Fresh nn.Linear default init (U(+-1/sqrt(fan_in)) for weight and bias), base Gaussians mean 0 / std 1; the
        fixed eval latents are kept."""
        self._replay_reference_init(draw_latents=False)

    def _buffers_ref(self):
        return flow_buffers(self.n_flows, self.device)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for key in self.layout:
            v = self.view(key)
            destination[prefix + key] = v if keep_vars else v.detach().clone()
        for k, v in self._buffers_ref().items():
            destination[prefix + k] = v

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        bufs = self._buffers_ref()
        with torch.no_grad():
            for key in self.layout:
                k = prefix + key
                if k in state_dict:
                    src = state_dict[k]
                    dst = self.view(key)
                    if tuple(src.shape) != tuple(dst.shape):
                        error_msgs.append(f"size mismatch for {k}: {tuple(src.shape)} vs {tuple(dst.shape)}")
                        continue
                    dst.copy_(src.to(dst.device, torch.float32))
                elif strict:
                    missing_keys.append(k)
        self._dirty = True                  # re-pack before the next launch
        self.params_serial += 1             # (writes through .data views do not move flat._version): a pending backward must notice
        if strict:
            for k in state_dict:
                if k.startswith(prefix) and k[len(prefix):] not in self.layout and k[len(prefix):] not in bufs:
                    unexpected_keys.append(k)

    def _sync(self):
        """Re-pack the MFMA-ordered weight copies if ``flat`` changed (optimizer.step, load_state_dict)."""
        if (getattr(self, "_dirty", True) or self.flat.data_ptr() != getattr(self, "_packed_ptr", None)
                or self.flat._version != self._packed_version):
            L.check(L.lib().cfnerf_model_set_params(self._h, L.ptr(self.flat.data), L.stream()), "cfnerf_model_set_params")
            self.mark_packed()

    def mark_packed(self):
        """Tell the module that the library already re-packed (cfnerf_adam_step does)."""
        self._packed_version = self.flat._version
        self._packed_ptr = self.flat.data_ptr()
        self._dirty = False
        self.pack_serial += 1               # identifies the packed weights the library holds: a backward must meet its forward's

    pack_serial = 0

    def mark_dirty(self):
        """Call after writing into ``flat.data`` / ``view(key)`` directly."""
        self._dirty = True
        self.params_serial += 1

    # bumped by every parameter update that does not go through a torch in-place op on ``flat`` (the fused Adam kernel of
    # train.Trainer writes through the raw pointer; mark_dirty): with ``flat._version`` it identifies "the weights of a forward"
    params_serial = 0

    @property
    def handle(self):
        return self._h

    def ensure_workspace(self, N: int, S: int, K: int):
        """Lend the library a torch-owned block big enough for a STASH forward + backward of an (N,S,K) batch
        (``cfnerf_workspace_bytes`` / ``cfnerf_model_set_workspace``): the library itself never allocates on the train
        path.  The block only grows; a pending backward of an earlier forward is invalidated when it does."""
        lib = L.lib()
        need = lib.cfnerf_workspace_bytes(C.byref(self.cfg), N, S, K)
        if need < 0:
            raise RuntimeError("cfnerf_workspace_bytes: " + lib.cfnerf_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            if self._ws is not None:
                # growth is rare: wait for every kernel that may still use the old block (whatever stream it ran on) before the
                # block goes back to torch's caching allocator
                torch.cuda.synchronize(self.device)
            L.check(lib.cfnerf_model_set_workspace(self._h, None, 0), "cfnerf_model_set_workspace")   # drop the old block first
            self._ws = None
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            L.check(lib.cfnerf_model_set_workspace(self._h, C.c_void_p(ws.data_ptr()), ws.numel()), "cfnerf_model_set_workspace")
            self._ws = ws

    def release_workspace(self):
        """Give the block back (e.g. before a large evaluation render)."""
        if self._ws is not None:
            torch.cuda.synchronize(self.device)
            L.check(L.lib().cfnerf_model_set_workspace(self._h, None, 0), "cfnerf_model_set_workspace")
            self._ws = None

    def set_precision(self, mode: str):
        """'fp32' (default: exact-fp32 MFMA) or 'bf16x3' (opt-in split-bf16 MFMA in the forward's dense layers)."""
        code = {"fp32": 0, "bf16x3": 1}[mode]
        L.check(L.lib().cfnerf_model_set_precision(self._h, code), "cfnerf_model_set_precision")
        self.precision = mode

    def set_flow_math(self, mode: str):
        """Arithmetic of the flows + composite inside the fused kernels: 'libm' (correctly rounded routines), 'fast' (hardware
        exp2 / log2 / rcp forms, same parity bounds) or 'auto' (default: libm below 16 latent samples, fast from 16 on)."""
        L.check(L.lib().cfnerf_model_set_flow_math(self._h, {"auto": 0, "libm": 1, "fast": 2}[mode]), "cfnerf_model_set_flow_math")
        self.flow_math = mode

    def eval_eps(self):
        """[K,4] eval latents: the fixed buffers with the LAST sample zeroed (MOD:199,205)."""
        # the device copy is rebuilt only when the (plain-attribute) latents were replaced or edited in place
        key = (id(self.sample_rgb), self.sample_rgb._version, id(self.sample_alpha), self.sample_alpha._version)
        if getattr(self, "_eval_eps_key", None) != key:
            e = LT.pack(self.sample_alpha, self.sample_rgb)
            e[-1] = 0
            self._eval_eps_dev, self._eval_eps_key = e.to(self.device), key
        return self._eval_eps_dev

    def draw_eps(self):
        """One fresh train pair ``[K,4]`` on the device (latents.draw_pairs: the reference's order; the upload does not block the host)."""
        return LT.to_device(LT.draw_pairs(1, self.K_samples)[0], self.device)

    def _one_call_only(self, is_test, x=None):
        """True when a batch of points must reach forward() in ONE call, not in batchify's chunks."""
        if torch.is_grad_enabled() and ((self.flat.requires_grad and not is_test) or (x is not None and x.requires_grad)):
            # one launch = the model's one stash; chunks would each replace it and the backward would re-run their forwards
            return True
        # latent rows of the whole batch (render_rays' hand-over): its network calls are already in them
        return self._next_eps is not None and self._next_eps.dim() == 3

    # ---- forward (MOD:188-291) ---------------------------------------------------------------
    def forward(self, x, is_val=False, is_test=False, eps_alpha=None, eps_rgb=None):
        _need_gpu(x, "x")
        if x.shape[-1] != self.input_ch + self.input_ch_views:
            raise ValueError(f"x must have {self.input_ch + self.input_ch_views} channels, got {x.shape[-1]}")
        self._sync()
        xf = _f32c(x.reshape(-1, x.shape[-1]))
        P, K = xf.shape[0], self.K_samples
        explicit = LT.pack(eps_alpha, eps_rgb)
        if self._next_eps is not None and explicit is None:
            eps = self._next_eps                                    # latents chosen by the enclosing render_rays call
        elif is_test:
            eps = _latents(self, explicit, False, self.device)
        else:                                                       # P points = P rays of one sample (batchify, RUN:47-64)
            eps = LT.to_device(LT.train_latents(self.latent_draws, explicit, N=P, S=1, K=K, netchunk=self.netchunk)[1], self.device)
        # (point rows from render_rays cover the whole batch: a network_query_fn of its own must hand all of it to ONE call)
        LT.check_rows(eps, P, "points", hint=": in netchunk mode render_rays hands one latent row per point of the whole batch, so a custom "
                                             "network_query_fn must evaluate all of them in one NeRF_Flows call")
        want_x = torch.is_grad_enabled() and x.requires_grad
        want_eps = torch.is_grad_enabled() and eps.requires_grad      # explicit latents that ask for a gradient (CFNERF_F_EPS_GRAD), either branch
        if ((torch.is_grad_enabled() and self.flat.requires_grad and not is_test) or want_x or want_eps) and P > 0:
            # the reference's forward is an autograd graph (MOD:188-291): so is this one - cfnerf_network_fwd with the
            # activation stash, differentiated by cfnerf_network_bwd.  Gradients reach the parameters and - when x asks for
            # one (CFNERF_F_INPUT_GRAD: a frozen network still gives x.grad) - the inputs.  The eval branch is a graph in the
            # reference too: with an input gradient wanted it runs the same node on the eval latents.
            xin = x.reshape(-1, x.shape[-1]).to(torch.float32) if want_x else xf
            raw, ent = _NetworkFn.apply(self.flat, self, xin, eps)
            if is_test:
                return raw, torch.zeros_like(raw)                    # MOD:223
            return raw, ent.reshape(1, 1, 1).expand(P, K, 1)         # MOD:291
        raw, ent = _network_fwd(self, xf, eps, K, 0 if is_test else L.F_TRAIN)
        if is_test:
            return raw, torch.zeros_like(raw)                        # MOD:223
        return raw, ent.reshape(1, 1, 1).expand(P, K, 1)             # MOD:291

    # ---- sample (MOD:69-96): the density latents of a batch of points, geometry only -----------------
    def sample(self, x, eps_alpha=None):
        """``alpha_k [P,K,1]``: the pre-softplus density latent of every (point, latent sample) of the pre-embedded ``x [P, input_ch +
        input_ch_views]`` (the view columns are not read) - trunk -> ``h_alpha`` -> density flow, what the reference's ``sample`` evidently
        means (its colour half is commented out, and as shipped it calls the flows without ``is_test`` and cannot run).  The latents are
        ``self.sample_alpha`` AS THEY ARE (MOD:78 does not zero the last one, unlike the eval branch of ``forward``) or an explicit
        ``eps_alpha [K,1]``.  One CFNERF_F_GEOMETRY launch: the colour branch is not computed; every value has the bits of
        ``forward(x, is_test=True)[0][..., 3]`` with the same density latents.  Inference only."""
        if torch.is_grad_enabled() and self.flat.requires_grad:
            raise RuntimeError("NeRF_Flows.sample is inference only (a geometry-only launch keeps no activations): call it under "
                               "torch.no_grad(), or use forward() for a differentiable density")
        _need_gpu(x, "x")
        if x.shape[-1] != self.input_ch + self.input_ch_views:
            raise ValueError(f"x must have {self.input_ch + self.input_ch_views} channels, got {x.shape[-1]}")
        ea = self.sample_alpha if eps_alpha is None else eps_alpha
        if tuple(ea.shape) != (self.K_samples, 1):
            raise ValueError(f"eps_alpha must be [K,1] = [{self.K_samples},1], got {tuple(ea.shape)}")
        self._sync()
        eps = torch.zeros(self.K_samples, 4)
        eps[:, 3:] = ea.detach().to("cpu", torch.float32)
        xf = _f32c(x.reshape(-1, x.shape[-1]))
        return _network_geometry(self, xf, eps.to(self.device)).unsqueeze(-1)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                L.lib().cfnerf_model_destroy(h)      # synchronises the device before the lent workspace tensor is freed
            except Exception:
                pass
            try:
                object.__setattr__(self, "_h", None)     # (nn.Module.__setattr__ may already be torn down at interpreter exit)
            except Exception:
                pass


def _params_token(model):
    """Identifies "the weights of a forward": torch in-place ops on ``flat`` (optimizer.step) move ``flat._version``; everything that
    writes through the raw pointer or a ``.data`` view (the fused Adam kernel, load_state_dict, mark_dirty) bumps ``params_serial``."""
    return (model.flat._version, model.params_serial)


def _mark_forward(ctx, model):
    """What a backward must meet again (``_check_backward``): its forward's stash generation, weights and the library's packed copy of them."""
    ctx.generation = L.lib().cfnerf_model_stash_generation(model.handle)
    ctx.params_at, ctx.pack_serial = _params_token(model), model.pack_serial


def _check_backward(ctx, model, packed=True):
    """A backward differentiates the stashed activations of ITS forward against what the library holds NOW: the packed weights AND -
    for the base Gaussians (alpha_mean / alpha_std / rgb_mean / rgb_std) - the flat parameter buffer itself, which the flow-adjoint
    kernels read live.  If either changed since the forward (optimizer.step(), Trainer.step() through the same handle,
    load_state_dict(), mark_dirty(); or a re-pack by a later launch) the result would be silently inconsistent whether or not the
    activation stash is still the forward's (round-4 advisor) - torch autograd raises in this situation, so do we."""
    if _params_token(model) != ctx.params_at or (packed and model.pack_serial != ctx.pack_serial):
        raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation: the "
                           "parameters of NeRF_Flows changed between this forward and its backward (call backward() before "
                           "optimizer.step() / Trainer.step() / load_state_dict())")


def _network_fwd(model, xf, eps, K, flags):
    """cfnerf_network_fwd of the encoded points ``xf [P,90]`` into new ``raw [P,K,4]`` and a zeroed entropy accumulator ``[1]``.
    ``eps`` is the launch's ``[K,4]`` or one row per point ``[P,K,4]`` (CFNERF_F_EPS_ROWS)."""
    if LT.check_rows(eps, xf.shape[0], "points"):
        flags |= L.F_EPS_ROWS
    raw = torch.empty(xf.shape[0], K, 4, device=xf.device)
    ent = torch.zeros(1, device=xf.device)
    L.check(L.lib().cfnerf_network_fwd(model.handle, L.ptr(xf), L.ptr(eps), xf.shape[0], K, flags, L.ptr(raw), L.ptr(ent), L.stream()),
            "cfnerf_network_fwd")
    return raw, ent


def _network_geometry(model, xf, eps, out=None):
    """cfnerf_network_fwd with CFNERF_F_GEOMETRY: the density latents ``[P,K]`` of the encoded points ``xf [P,90]`` for the ``[K,4]`` latents
    ``eps`` (column 3 is read), into ``out`` or a new tensor."""
    P, K = xf.shape[0], eps.shape[0]
    if out is None:
        out = torch.empty(P, K, device=xf.device)
    L.check(L.lib().cfnerf_network_fwd(model.handle, L.ptr(xf), L.ptr(eps), P, K, L.F_GEOMETRY, L.ptr(out), None, L.stream()),
            "cfnerf_network_fwd")
    return out


class _NetworkFn(torch.autograd.Function):
    """NeRF_Flows.forward as an autograd node: cfnerf_network_fwd with the activation stash + cfnerf_network_bwd.  The model has
    ONE stash.  If a later grad-enabled forward replaced it before this node's backward runs (several chunks of one batch through
    a caller's own batchify loop), the node re-runs its forward from the inputs it kept (x, latents - the parameters cannot
    have changed in between) and then differentiates: chunked callers train, at the price of one extra forward per chunk."""

    @staticmethod
    def _forward_stash(model, xf, eps, extra=0):
        K = eps.shape[-2]
        model.ensure_workspace(1, xf.shape[0], K)
        return _network_fwd(model, xf, eps, K, L.F_TRAIN | L.F_STASH | extra)

    @staticmethod
    def forward(ctx, flat, model, xf, eps):
        # xf asks for a gradient: the stash remembers CFNERF_F_INPUT_GRAD and the backward also writes d_x behind the parameter gradient;
        # the latents ask for one: CFNERF_F_EPS_GRAD, d_eps / d_eps_rows behind that (a frozen network still gives either)
        ctx.extra = (L.F_INPUT_GRAD if ctx.needs_input_grad[2] else 0) | (L.FLAG_EPS_GRAD if ctx.needs_input_grad[3] else 0)
        xf, eps = _f32c(xf), _f32c(eps)
        raw, ent = _NetworkFn._forward_stash(model, xf, eps, ctx.extra)
        ctx.model, ctx.xf, ctx.eps, ctx.n_params = model, xf, eps, flat.numel()
        _mark_forward(ctx, model)
        return raw, ent.reshape(())

    @staticmethod
    def backward(ctx, d_raw, d_ent):
        model, lib = ctx.model, L.lib()
        stash_kept = lib.cfnerf_model_stash_generation(model.handle) == ctx.generation
        _check_backward(ctx, model, packed=stash_kept)             # the stash is this forward's: so must the packed weights be
        if not stash_kept:
            # the stash is gone (a later grad-enabled forward replaced it): re-run the forward - the SAME forward, the parameters being the
            # ones it was taken at (checked above; a re-pack of unchanged parameters in between is harmless here)
            model._sync()
            _NetworkFn._forward_stash(model, ctx.xf, ctx.eps, ctx.extra)
            ctx.generation = lib.cfnerf_model_stash_generation(model.handle)
        dr = _f32c(d_raw) if d_raw is not None else None
        de = _f32c(d_ent.reshape(1)) if d_ent is not None else None
        want_x, want_eps = bool(ctx.extra & L.F_INPUT_GRAD), bool(ctx.extra & L.FLAG_EPS_GRAD)
        if dr is None and de is None:
            return (torch.zeros(ctx.n_params, device=model.flat.device), None, (torch.zeros_like(ctx.xf) if want_x else None),
                    (torch.zeros_like(ctx.eps) if want_eps else None))
        if want_eps:
            # CFNERF_F_EPS_GRAD layout of grad_flat (cfnerf.h): d_eps [K,4] from e_off and d_eps_rows [P,K,4] from er_off, behind the blocks of before
            (P, Cx), K = ctx.xf.shape, ctx.eps.shape[-2]
            x_off = L.input_grad_offset(ctx.n_params)
            e_off, er_off, total = L.eps_grad_offsets(x_off + P * Cx if want_x else ctx.n_params, P, K)
            grad = torch.empty(total, device=model.flat.device)
            L.check(lib.cfnerf_network_bwd(model.handle, ctx.generation, L.ptr(dr), L.ptr(de), L.ptr(grad), L.stream()), "cfnerf_network_bwd")
            d_eps = grad[er_off:].view(P, K, 4) if ctx.eps.dim() == 3 else grad[e_off:e_off + K * 4].view(K, 4)
            return grad[:ctx.n_params], None, (grad[x_off:x_off + P * Cx].view(P, Cx) if want_x else None), d_eps
        if not ctx.extra:
            grad = torch.empty(ctx.n_params, device=model.flat.device)
            L.check(lib.cfnerf_network_bwd(model.handle, ctx.generation, L.ptr(dr), L.ptr(de), L.ptr(grad), L.stream()), "cfnerf_network_bwd")
            return grad, None, None, None
        # CFNERF_F_INPUT_GRAD layout of grad_flat (cfnerf.h): [0, n_params) the parameter gradient, d_x [P, C] from x_off on
        x_off, (P, Cx) = L.input_grad_offset(ctx.n_params), ctx.xf.shape
        grad = torch.empty(x_off + P * Cx, device=model.flat.device)
        L.check(lib.cfnerf_network_bwd(model.handle, ctx.generation, L.ptr(dr), L.ptr(de), L.ptr(grad), L.stream()), "cfnerf_network_bwd")
        return grad[:ctx.n_params], None, grad[x_off:].view(P, Cx), None


def _composite_fwd(raw, z_vals, rays_d, white_bkgd):
    """cfnerf_composite_fwd into new ``rgb_map [N,3,K], disp_map [N,K], weights [N,S,K], depth_map [N,K]`` (raw2outputs' order)."""
    N, S, K = raw.shape[0], raw.shape[1], raw.shape[2]
    dev = raw.device
    rgb_map = torch.empty(N, 3, K, device=dev)
    disp_map = torch.empty(N, K, device=dev)
    depth_map = torch.empty(N, K, device=dev)
    weights = torch.empty(N, S, K, device=dev)
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw), L.ptr(z_vals), L.ptr(rays_d), N, S, K, int(bool(white_bkgd)), L.ptr(rgb_map),
                                         L.ptr(disp_map), L.ptr(depth_map), L.ptr(weights), L.stream()), "cfnerf_composite_fwd")
    return rgb_map, disp_map, weights, depth_map


class _CompositeFn(torch.autograd.Function):
    """raw2outputs (RUN:411-454) as an autograd node: cfnerf_composite_fwd + cfnerf_composite_bwd (stateless; differentiable with
    respect to raw, z_vals and rays_d through every output: rgb_map, disp_map, weights, depth_map).  The library is asked only for what
    ``needs_input_grad`` asks: d_raw alone is the plain call; d_z_vals / d_rays_d are CFNERF_F_SEAM_GRAD, without d_raw for a detached raw."""

    @staticmethod
    def forward(ctx, raw, z_vals, rays_d, white_bkgd):
        ctx.save_for_backward(raw, z_vals, rays_d)
        ctx.white_bkgd = int(bool(white_bkgd))
        return _composite_fwd(raw, z_vals, rays_d, white_bkgd)

    @staticmethod
    def backward(ctx, d_rgb, d_disp, d_weights, d_depth):
        raw, z_vals, rays_d = ctx.saved_tensors
        N, S, K = raw.shape[0], raw.shape[1], raw.shape[2]
        want_raw, want_z, want_d = ctx.needs_input_grad[:3]
        if N == 0 or (d_rgb is None and d_disp is None and d_weights is None and d_depth is None):
            return (torch.zeros_like(raw) if want_raw else None, torch.zeros_like(z_vals) if want_z else None,
                    torch.zeros_like(rays_d) if want_d else None, None)
        d_raw = torch.empty_like(raw) if want_raw else None
        g_rgb = _f32c(d_rgb) if d_rgb is not None else torch.zeros(N, 3, K, device=raw.device)
        c = lambda t: _f32c(t) if t is not None else None
        g_disp, g_depth, g_weights = c(d_disp), c(d_depth), c(d_weights)         # (named: a converted copy must outlive the allocations below)
        cots = (L.ptr(g_rgb), L.ptr(g_disp), L.ptr(g_depth), L.ptr(g_weights))
        if not (want_z or want_d):
            L.check(L.lib().cfnerf_composite_bwd(L.ptr(raw), L.ptr(z_vals), L.ptr(rays_d), N, S, K, ctx.white_bkgd, *cots, L.ptr(d_raw), L.stream()),
                    "cfnerf_composite_bwd")
            return d_raw, None, None, None
        d_z = torch.empty_like(z_vals) if want_z else None
        d_d = torch.empty_like(rays_d) if want_d else None
        out = L.composite_grads(d_raw=d_raw, d_z_vals=d_z, d_rays_d=d_d)
        L.check(L.lib().cfnerf_composite_bwd(L.ptr(raw), L.ptr(z_vals), L.ptr(rays_d), N, S, K, ctx.white_bkgd | L.F_SEAM_GRAD, *cots,
                                             L.composite_grads_arg(out), L.stream()), "cfnerf_composite_bwd")
        return d_raw, d_z, d_d, None


class _DataParallelShim(nn.Module):
    """Stands where the reference puts ``nn.DataParallel(model)`` (RUN:330): same ``.module`` attribute and
    the same ``module.``-prefixed ``state_dict`` keys, but no replication - multi-GPU is one process per
    GPU with ray sharding (see cf-nerf_amd/train.py)."""

    def __init__(self, module: NeRF_Flows):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


def _unwrap(network_fn) -> NeRF_Flows:
    m = network_fn.module if isinstance(network_fn, _DataParallelShim) else network_fn
    if not isinstance(m, NeRF_Flows):
        raise TypeError("network_fn must be the NeRF_Flows returned by create_nerf")
    return m


# --------------------------------------------------------------------------------------------
def batchify(fn, chunk):
    """RUN:47-64.  The kernels tile internally, so chunking only bounds the size of one launch."""
    if chunk is None:
        return fn

    def ret(inputs, is_val, is_test):
        m = getattr(fn, "module", fn)
        if isinstance(m, NeRF_Flows) and m._one_call_only(is_test, inputs):
            return fn(inputs, is_val, is_test)
        A, B = [], []
        for i in range(0, inputs.shape[0], chunk):
            a, b = fn(inputs[i:i + chunk], is_val, is_test)
            A.append(a)
            B.append(b)
        return torch.cat(A, 0), torch.cat(B, 0)
    return ret


def run_network(inputs, viewdirs, fn, is_val, is_test, embed_fn, embeddirs_fn, netchunk=1024 * 64):
    """RUN:67-85 (the unfused query: embed with torch, then the network kernel)."""
    inputs_flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
    embedded = embed_fn(inputs_flat)
    if viewdirs is not None:
        input_dirs = viewdirs[:, None].expand(inputs.shape) if viewdirs.ndim == inputs.ndim - 1 else viewdirs
        input_dirs_flat = torch.reshape(input_dirs, [-1, input_dirs.shape[-1]])
        embedded = torch.cat([embedded, embeddirs_fn(input_dirs_flat)], -1)
    outputs_flat, loss_entropy = batchify(fn, netchunk)(embedded, is_val, is_test)
    outputs = torch.reshape(outputs_flat, list(inputs.shape[:-1]) + list(outputs_flat.shape[-2:]))
    return outputs, loss_entropy


def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False, pytest=False):
    """RUN:411-454 on the standalone composite kernel.  ``raw_noise_std`` is accepted and has no effect,
    exactly like the reference (the noise is generated but never added, RUN:432-442)."""
    _need_gpu(raw, "raw")
    if _wants_grad(raw, z_vals, rays_d):                             # differentiable like the reference's: in raw, z_vals and rays_d
        f = lambda t: t.to(torch.float32).contiguous() if t.requires_grad else _f32c(t)
        return _CompositeFn.apply(f(raw), f(z_vals), f(rays_d), bool(white_bkgd))
    return _composite_fwd(_f32c(raw), _f32c(z_vals), _f32c(rays_d), white_bkgd)


# --------------------------------------------------------------------------------------------
class _RayRegFn(torch.autograd.Function):
    """The ray regularisers as an autograd node over ONE CFNERF_F_RAY_REG launch: the forward keeps the kernel's (scaled) ``d_weights`` and,
    when ``z_vals`` asks for a gradient, its direct ``d_z``; the backward multiplies them by the incoming cotangent.  Output: the launch's
    8 scalars, ``[0]`` = reg - the one entry whose cotangent is read."""

    @staticmethod
    def forward(ctx, weights, z_vals, rays, lambda_dist, lambda_ent, acc_min, n_total):
        w, z = _f32c(weights), _f32c(z_vals)
        want_z = ctx.needs_input_grad[1]
        d_w, d_z = torch.empty_like(w), (torch.empty_like(z) if want_z else None)
        out = torch.empty(8, device=w.device)
        L.ray_reg(w, z, d_w, out, rays=rays, d_z=d_z, lambda_dist=lambda_dist, lambda_ent=lambda_ent, acc_min=acc_min, n_total=n_total)
        ctx.d_w, ctx.d_z = d_w, d_z
        ctx.dtypes = (weights.dtype, z_vals.dtype)
        return out

    @staticmethod
    def backward(ctx, d_out):
        g = d_out[0]
        d_w = (ctx.d_w * g).to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        d_z = (ctx.d_z * g).to(ctx.dtypes[1]) if ctx.d_z is not None else None
        return d_w, d_z, None, None, None, None, None


def ray_regularizers(weights, z_vals, rays=None, distortion=0., entropy=0., acc_min=0.1, n_total=None):
    """The two ray regularisers of few-view training on the composite's ``weights [N,S,K]`` (``render_rays(retweights=True)`` on the fused
    path, ``raw2outputs`` on the seam) and the depths ``z_vals [N,S]``, in ONE launch (CFNERF_F_RAY_REG, include/cfnerf.h has the formulas):
    ``reg = distortion * dist + entropy * ent`` with ``dist`` the distortion loss of mip-NeRF 360 on the intervals' normalised midpoints,
    ``ent`` the ray entropy of InfoNeRF over the (ray, latent) pairs whose weights sum above ``acc_min``, both means over ``n_total``
    (default N) rays and the K latents.  ``rays``: the packed ``ray_batch [N,11]`` or ``(near, far)`` - the depths are normalised to
    ``(z - near) / (far - near)``; None: taken as they are.  A weight of 0 skips that term.

    Returns ``(reg, parts)``: ``reg`` a 0-dim tensor on the graph - ``weights.grad`` and, when ``z_vals`` requires grad, the direct
    ``z_vals.grad`` (the path through the weights is the composite's own backward) - and ``parts = {'dist', 'ent', 'frac'}``, 0-dim
    tensors off the graph (``frac``: the fraction of pairs above ``acc_min``).  Nothing synchronises with the host."""
    _need_gpu(weights, "weights")
    if weights.dim() != 3 or z_vals.dim() != 2 or tuple(z_vals.shape) != tuple(weights.shape[:2]):
        raise ValueError(f"weights must be [N,S,K] and z_vals [N,S], got {tuple(weights.shape)} and {tuple(z_vals.shape)}")
    N = weights.shape[0]
    if rays is not None:
        if isinstance(rays, (tuple, list)):
            near, far = rays
            packed = torch.zeros(N, 11, device=weights.device)
            packed[:, 6] = torch.as_tensor(near, dtype=torch.float32, device=weights.device).reshape(-1)
            packed[:, 7] = torch.as_tensor(far, dtype=torch.float32, device=weights.device).reshape(-1)
            rays = packed
        else:
            rays = _f32c(rays)
            if rays.dim() != 2 or tuple(rays.shape) != (N, 11):
                raise ValueError(f"rays must be the packed ray_batch [N,11] or (near, far), got {tuple(rays.shape)}")
    out = _RayRegFn.apply(weights, z_vals.to(weights.device), rays, float(distortion), float(entropy), float(acc_min), int(n_total or 0))
    parts = out.detach()
    return out[0], {'dist': parts[1], 'ent': parts[2], 'frac': parts[3]}


@torch.no_grad()
def k_scores(samples, target=None, levels=None, return_sorted=False):
    """The K latent samples ``samples [...,K]`` (fp32, on the GPU; K <= 128) scored as an ensemble, row by row, in ONE launch
    (CFNERF_F_KSCORES, include/cfnerf.h has the definitions).  Returns a dict with

    * ``quantiles [...,Q]`` at the ``levels`` (a sequence of at most 16 numbers in [0,1]; ``numpy.quantile(method="linear")``), when given;
    * ``sorted [...,K]``, the samples ascending (a permutation of their bits; NaN last), with ``return_sorted``;
    * with ``target [...]``: ``crps [...]`` (the CRPS of the K-member ensemble against the target), ``rank_code [...]`` int32
      (``2 #{x_k < y} + #{x_k == y}``) and ``pit [...]`` = ``rank_code / (2K)``.

    A row that holds a NaN (or whose target is NaN) gets NaN quantiles / crps / pit and ``rank_code`` -1.  Every output of a row depends on
    that row alone; nothing synchronises with the host."""
    _need_gpu(samples, "samples")
    if samples.dim() < 1 or samples.shape[-1] < 1:
        raise ValueError(f"samples must be [...,K] with K >= 1, got {tuple(samples.shape)}")
    lead, K = tuple(samples.shape[:-1]), samples.shape[-1]
    x = _f32c(samples).reshape(-1, K)
    M, dev = x.shape[0], x.device
    y = None
    if target is not None:
        if tuple(target.shape) != lead:
            raise ValueError(f"target must be {lead} (samples without the last axis), got {tuple(target.shape)}")
        y = _f32c(target).to(dev).reshape(-1)
    lv = [] if levels is None else L.quantile_levels(levels, K)
    if len(lv) > 16:
        raise ValueError(f"at most 16 quantile levels per launch, got {len(lv)}")
    if not lv and y is None and not return_sorted:
        raise ValueError("k_scores: nothing to compute - give levels=, target= or return_sorted=True")
    out = {}
    if lv:
        out["quantiles"] = torch.empty(M, len(lv), device=dev)
    if return_sorted:
        out["sorted"] = torch.empty(M, K, device=dev)
    if y is not None:
        out["crps"], out["pit"] = torch.empty(M, device=dev), torch.empty(M, device=dev)
        out["rank_code"] = torch.empty(M, dtype=torch.int32, device=dev)
    if M > 0:
        L.k_scores(x, M, K, target=y, sorted_out=out.get("sorted"), quantiles=out.get("quantiles"), levels=lv, rank_code=out.get("rank_code"),
                   pit=out.get("pit"), crps=out.get("crps"))
    return {k: v.reshape(lead + tuple(v.shape[1:])) for k, v in out.items()}


@torch.no_grad()
def ssim(img, gt, data_range=1.0, window="uniform", win_size=None, sigma=1.5, full=False):
    """The structural similarity of ``img`` and ``gt`` - ``[H,W]``, ``[H,W,C]`` or ``[B,H,W,C]`` fp32 tensors on the GPU, C <= 4 - as
    ``skimage.metrics.structural_similarity(img, gt, data_range=data_range, channel_axis=-1)`` computes it, in ONE call of the fused kernel
    (CFNERF_MODE_SSIM, include/cfnerf.h has the definitions): ``window="uniform"`` is skimage's default (7 x 7 box, sample covariance),
    ``window="gaussian"`` its ``gaussian_weights=True`` (sigma = 1.5: 11 x 11); ``win_size`` overrides the number of taps (odd, 3..15).
    Returns the mean over the valid interior and the channels, one value per image (a 0-dim tensor without a batch axis); with
    ``full=True`` also the map on the interior, ``[..., H-win+1, W-win+1(, C)]`` - there is no boundary mode, where skimage's full map
    carries a border that its own mean crops.  The window moments are accumulated in fp64, so a bright, flat render does not lose its
    variance against C2 as ``E[x^2] - mu^2`` does in fp32.  Nothing synchronises with the host."""
    _need_gpu(img, "img")
    _need_gpu(gt, "gt")
    if tuple(img.shape) != tuple(gt.shape):
        raise ValueError(f"img and gt must have one shape, got {tuple(img.shape)} and {tuple(gt.shape)}")
    if img.dim() not in (2, 3, 4):
        raise ValueError(f"img must be [H,W], [H,W,C] or [B,H,W,C], got {tuple(img.shape)}")
    if not data_range > 0:
        raise ValueError(f"data_range must be positive, got {data_range!r}")
    taps, cov = L.ssim_window(window, win_size, sigma)
    win = len(taps)
    x, y = _f32c(img), _f32c(gt)
    shape = {2: (1,) + tuple(x.shape) + (1,), 3: (1,) + tuple(x.shape), 4: tuple(x.shape)}[x.dim()]
    B, H, W, C_ = shape
    if not 1 <= C_ <= 4:
        raise ValueError(f"at most 4 channels (channel-last), got {C_}")
    if H < win or W < win:
        raise ValueError(f"the image ({H} x {W}) is smaller than the window ({win} taps): the valid interior is empty")
    dev = x.device
    mean = torch.empty(B, C_, device=dev)
    smap = torch.empty(B, H - win + 1, W - win + 1, C_, device=dev) if full else None
    if B > 0:
        scratch = torch.empty(L.ssim_scratch_floats(B, C_, H, W, win) // 2, dtype=torch.float64, device=dev)
        L.ssim(x, y, B, H, W, C_, taps, cov, (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, ssim_map=smap, mean=mean, scratch=scratch)
    value = mean.double().mean(-1).float()
    if img.dim() < 4:
        value = value[0]
    if not full:
        return value
    return value, smap.reshape(tuple(img.shape[:-2]) + (H - win + 1, W - win + 1) if img.dim() == 2 else
                               tuple(img.shape[:-3]) + (H - win + 1, W - win + 1, C_))


def _render_fwd(model, rays, t_vals, t_rand, eps, flags, z_vals=None, maps=True, raw=False, weights=False, pts=False, kstats=False,
                entropy=True):
    """cfnerf_render_fwd of the packed ``rays [N,11]`` into newly allocated outputs.  Returns a dict with ``rgb_map [N,3,K]``,
    ``disp_map`` / ``depth_map [N,K]`` (``maps``), ``raw [N,S,K,4]``, ``weights [N,S,K]``, ``pts [N,S,3]``, ``kstats [N,8]`` ([N,12] with ``L.F_KSTATS_EXT`` in ``flags``) and the
    zeroed accumulator ``entropy [1]``; an output that was not asked for is None.  S is that of ``z_vals [N,S]`` (explicit depths,
    which the library then prefers to ``t_rand``) or of the sample table ``t_vals``."""
    N, K = rays.shape[0], eps.shape[-2]
    if LT.check_rows(eps, N, "rays"):
        flags |= L.F_EPS_ROWS
    S = z_vals.shape[1] if z_vals is not None else t_vals.shape[0]
    dev = rays.device
    new = lambda want, *shape: torch.empty(*shape, device=dev) if want else None
    o = {'rgb_map': new(maps, N, 3, K), 'disp_map': new(maps, N, K), 'depth_map': new(maps, N, K), 'raw': new(raw, N, S, K, 4),
         'weights': new(weights, N, S, K), 'pts': new(pts, N, S, 3), 'kstats': new(kstats, N, 12 if flags & L.F_KSTATS_EXT else 8),
         'entropy': torch.zeros(1, device=dev) if entropy else None}
    L.check(L.lib().cfnerf_render_fwd(model.handle, L.ptr(rays), L.ptr(t_vals), L.ptr(t_rand), L.ptr(z_vals), L.ptr(eps), N, S, K, flags,
                                      *(L.ptr(t) for t in o.values()), L.stream()), "cfnerf_render_fwd")
    return o


@torch.no_grad()
def render_geometry(ray_batch, network_fn, t_vals=None, lindisp=False, z_vals=None, weights=False):
    """Geometry of the packed rays ``ray_batch [N,11]`` (o3, d3, near, far, viewdir3; the view direction is not read) on the eval branch, in
    ONE CFNERF_F_GEOMETRY launch that skips the colour branch: ``{"depth_map" [N,K], "disp_map" [N,K]}`` and, with ``weights``,
    ``"weights" [N,S,K]`` - each with the bits ``render_rays`` gives it on the eval branch.  ``t_vals [S]`` defaults to the reference's
    sample table; ``z_vals [N,S]`` are explicit depths (what a hierarchical coarse pass hands on): with them ``t_vals`` is not needed and
    not read, whatever its length."""
    net = _unwrap(network_fn)
    _need_gpu(ray_batch, "ray_batch")
    rays = _f32c(ray_batch)
    if rays.dim() != 2 or rays.shape[1] != 11:
        raise ValueError(f"ray_batch must be [N,11], got {tuple(rays.shape)}")
    if t_vals is None and z_vals is None:
        t_vals = t_vals_table(rays.device)
    net._sync()
    flags = L.F_GEOMETRY | (L.F_LINDISP if lindisp else 0)
    o = _render_geometry_fwd(net, rays, t_vals, net.eval_eps(), flags, z_vals=None if z_vals is None else _f32c(z_vals), weights=weights)
    out = {"depth_map": o["depth_map"], "disp_map": o["disp_map"]}
    if weights:
        out["weights"] = o["weights"]
    return out


def _render_geometry_fwd(model, rays, t_vals, eps, flags, z_vals=None, maps=True, raw=False, weights=False, pts=False, kstats=False):
    """cfnerf_render_fwd with CFNERF_F_GEOMETRY (in ``flags``) into newly allocated outputs: ``disp_map`` / ``depth_map [N,K]`` (``maps``),
    ``raw [N,S,K]`` (the density latent), ``weights [N,S,K]``, ``pts [N,S,3]``, ``kstats [N,6]``; an output not asked for is None."""
    N, K = rays.shape[0], eps.shape[-2]
    if z_vals is not None:
        if z_vals.dim() != 2 or z_vals.shape[0] != N:
            raise ValueError(f"z_vals must be [N,S] with N = {N} rays, got {tuple(z_vals.shape)}")
        t_vals = None                       # explicit depths: the geometry-only kernel does not read the sample table (any length, or none)
    S = z_vals.shape[1] if z_vals is not None else t_vals.shape[0]
    dev = rays.device
    new = lambda want, *shape: torch.empty(*shape, device=dev) if want else None
    o = {'disp_map': new(maps, N, K), 'depth_map': new(maps, N, K), 'raw': new(raw, N, S, K), 'weights': new(weights, N, S, K),
         'pts': new(pts, N, S, 3), 'kstats': new(kstats, N, 6)}
    L.check(L.lib().cfnerf_render_fwd(model.handle, L.ptr(rays), L.ptr(t_vals), None, L.ptr(z_vals), L.ptr(eps), N, S, K, flags, None,
                                      *(L.ptr(t) for t in o.values()), None, L.stream()), "cfnerf_render_fwd")
    return o


class _RenderFn(torch.autograd.Function):
    """Fused render (forward with activation stash) + cfnerf_render_bwd.  The model has ONE stash: the node remembers
    the generation of its forward and the backward is refused (loudly) if a later grad-enabled forward replaced it.
    When ``rays`` or an explicit ``z_vals`` asks for a gradient the stash carries CFNERF_F_RAY_GRAD and the backward also returns
    ``d_rays [N,11]`` (columns 6, 7 - near / far - are zero: not computed, cfnerf.h) and ``d_z [N,S]``.
    Every differentiable output carries a loss, as in the reference's one autograd graph: the stash carries CFNERF_F_COTANGENTS and the
    backward hands the library whichever of ``d_disp``, ``d_raw`` and ``d_weights`` autograd delivers (none of them: the kernels of a stash
    without the flag).  ``weights [N,S,K]`` is allocated and returned only with ``want_weights`` (else an empty tensor)."""

    @staticmethod
    def forward(ctx, flat, model, rays, t_vals, t_rand, eps, flags, want_pts, z_vals, want_weights=False):
        N, K = rays.shape[0], eps.shape[-2]
        flags |= L.F_COTANGENTS
        ctx.set_materialize_grads(False)        # an output without a loss arrives as None, not as a tensor of zeros: its kernel work is skipped
        ctx.want_rays, ctx.want_z = ctx.needs_input_grad[2], z_vals is not None and ctx.needs_input_grad[8]
        if ctx.want_rays or ctx.want_z:
            flags |= L.F_RAY_GRAD
        ctx.want_eps = ctx.needs_input_grad[5]      # the latents ask for a gradient: CFNERF_F_EPS_GRAD, d_eps / d_eps_rows behind the other blocks
        if ctx.want_eps:
            flags |= L.FLAG_EPS_GRAD
        rays, eps = _f32c(rays), _f32c(eps)
        z_vals = None if z_vals is None else _f32c(z_vals)
        S = z_vals.shape[1] if z_vals is not None else t_vals.shape[0]
        model.ensure_workspace(N, S, K)
        o = _render_fwd(model, rays, t_vals, t_rand, eps, flags | L.F_STASH, z_vals, raw=True, weights=want_weights, pts=want_pts)
        ctx.NS = (N, S)
        ctx.model = model
        ctx.eps = eps               # latent rows: the stash reads the caller's buffer until the backward (cfnerf.h, CFNERF_F_EPS_ROWS)
        ctx.n_params = flat.numel()
        _mark_forward(ctx, model)
        ctx.shape = (N, 3, K)
        pts = o['pts'] if want_pts else torch.empty(0, device=rays.device)
        weights = o['weights'] if want_weights else torch.empty(0, device=rays.device)
        # (torch keeps only the LAST mark_non_differentiable call's tensors: one call names them all)
        ctx.mark_non_differentiable(*([pts] if want_weights else [pts, weights]))
        return o['rgb_map'], o['disp_map'], o['depth_map'], o['entropy'].reshape(()), o['raw'], pts, weights

    @staticmethod
    def backward(ctx, d_rgb, d_disp, d_depth, d_ent, d_raw, d_pts, d_weights):
        model = ctx.model
        _check_backward(ctx, model)                                # (a replaced STASH is refused by the library itself: generation id)
        dev = model.flat.device
        ray_grad = ctx.want_rays or ctx.want_z
        # CFNERF_F_RAY_GRAD layout of grad_flat (cfnerf.h): the parameter gradient, then d_rays [N,11] from r_off and d_z [N,S] from z_off
        (N, S), n = ctx.NS, ctx.n_params
        r_off, z_off, total = L.ray_grad_offsets(n, N, S) if ray_grad else (n, n, n)
        K = ctx.shape[2]
        # CFNERF_F_EPS_GRAD: then d_eps [K,4] from e_off and d_eps_rows [N,K,4] from er_off
        e_off, er_off, total = L.eps_grad_offsets(total, N, K) if ctx.want_eps else (total, total, total)
        grad = torch.empty(total, device=dev)
        d_rgb = _f32c(d_rgb) if d_rgb is not None else torch.zeros(ctx.shape, device=dev)
        dd = _f32c(d_depth) if d_depth is not None else None
        de = _f32c(d_ent.reshape(1)) if d_ent is not None else None
        # CFNERF_F_COTANGENTS: the d_rgb_map argument is the host descriptor (cfnerf.h, cfnerf_cotangents); a member that is None stays NULL
        c = lambda t: None if t is None else _f32c(t)
        keep = (d_rgb, c(d_disp), c(d_weights), c(d_raw))
        cot = L.cotangents(*keep)
        L.check(L.lib().cfnerf_render_bwd(model.handle, ctx.generation, L.cotangents_arg(cot), L.ptr(dd), L.ptr(de), L.ptr(grad), L.stream()),
                "cfnerf_render_bwd")
        d_rays = grad[r_off:r_off + N * 11].view(N, 11) if ctx.want_rays else None
        d_z = grad[z_off:z_off + N * S].view(N, S) if ctx.want_z else None
        d_eps = None
        if ctx.want_eps:        # one set: its gradient; rows: one row per ray
            d_eps = grad[er_off:er_off + N * K * 4].view(N, K, 4) if ctx.eps.dim() == 3 else grad[e_off:e_off + K * 4].view(K, 4)
        return (grad[:n] if ctx.needs_input_grad[0] else None), None, d_rays, None, None, d_eps, None, None, d_z, None


def render_rays(ray_batch, network_fn, network_query_fn, N_samples, is_train, uniformsample, retraw=False,
                lindisp=False, K_samples=0, perturb=0., N_importance=0, network_fine=None, white_bkgd=False,
                raw_noise_std=0., verbose=False, pytest=False, t_rand=None, eps_alpha=None, eps_rgb=None,
                t_vals=None, retweights=False, hierarchical_extension=False, u_fine=None, chunk=None):
    """Volumetric rendering of a ray batch (RUN:457-553) in ONE fused launch.

    Returns ``{'rgb_map' [N,3,K], 'disp_map' [N,K], 'depth_map' [N,K]}`` plus ``raw``, ``loss_entropy``
    and ``pts`` when ``is_train`` (RUN:542-547).  ``retraw``, ``uniformsample``, ``K_samples``, ``verbose``
    are accepted and never read, like the reference; ``N_importance > 0`` / ``network_fine`` - which the
    reference silently ignores (there is no fine pass) - are rejected.  ``retweights=True`` adds ``weights [N,S,K]``
    (the ``weights`` of raw2outputs, RUN:443).  Under autograd every returned map is on the graph, as in the reference: a loss on
    ``disp_map``, ``raw`` or ``weights`` trains like one on ``rgb_map`` (CFNERF_F_COTANGENTS).  With a
    ``network_query_fn`` of the caller's the graph reaches ``ray_batch`` as well - all eleven columns, near / far included (section 13).

    A model in ``latent_draws = "netchunk"`` mode takes its train latents per netchunk (latents.py): ``chunk`` is then the
    ray cut of the reference's batchify_rays that the draw layout follows (``render`` passes its own; None = one cut).
    """
    _need_gpu(ray_batch, "ray_batch")
    if hierarchical_extension and N_importance and N_importance > 0:
        if is_train and _unwrap(network_fn).latent_draws == "netchunk":
            raise NotImplementedError("latent_draws='netchunk' is not supported by the hierarchical-sampling extension")
        return _render_rays_hierarchical(ray_batch, network_fn, N_samples, N_importance, is_train, lindisp, perturb, white_bkgd,
                                         t_rand, eps_alpha, eps_rgb, t_vals, u_fine)
    if N_importance and N_importance > 0 or network_fine is not None:
        raise NotImplementedError("the reference has no hierarchical/fine pass (N_importance is dead there); refusing to ignore it "
                                  "(pass hierarchical_extension=True for the coarse+fine EXTENSION of this build)")
    if ray_batch.shape[-1] != 11:
        raise ValueError("ray_batch must be [N,11] = o3,d3,near,far,viewdir3 (use_viewdirs=True)")
    model = _unwrap(network_fn)
    dev = ray_batch.device
    if t_vals is None:
        t_vals = t_vals_table(dev)
        if N_samples != t_vals.shape[0]:
            # the reference's z_vals.expand([N_rays, N_samples]) raises for any other value (RUN:510,516)
            raise ValueError(f"N_samples must be {t_vals.shape[0]} (hard-coded sample table, RUN:510); pass t_vals= to override")
    else:
        t_vals = t_vals.to(dev, torch.float32).contiguous()
    N, S, K = ray_batch.shape[0], t_vals.shape[0], model.K_samples
    rays = _f32c(ray_batch)
    # the reference's render_rays is an autograd graph in the rays too (pose refinement, registration): the fused node differentiates it
    want_rays = torch.is_grad_enabled() and ray_batch.requires_grad
    explicit = LT.pack(eps_alpha, eps_rgb)
    # ... and in its latents (eps.mul(std).add_(mean), MOD:239,251): explicit ones that ask for a gradient get it, CFNERF_F_EPS_GRAD
    want_eps = torch.is_grad_enabled() and explicit is not None and explicit.requires_grad
    if is_train:
        # latents.train_latents: the mode's draws in the reference's order (a t_rand of the CPU generator included, unless there is one)
        tr, eps, _ = LT.train_latents(model.latent_draws, explicit, N=N, S=S, K=K, netchunk=model.netchunk, chunk=chunk, perturb=perturb,
                                      raw_noise_std=raw_noise_std, own_t_rand=t_rand is not None or pytest)
        t_rand, eps = (tr if t_rand is None else t_rand), LT.to_device(eps, dev)
    else:
        eps = _latents(model, explicit, False, dev)
    if perturb > 0.:
        if t_rand is None:                                  # RUN:524 (eval branch; pytest: RUN:527-529)
            t_rand = torch.rand([N, S]) if not pytest else torch.tensor(__import__("numpy").random.rand(N, S), dtype=torch.float32)
        t_rand = _f32c(t_rand.to(dev))
    else:
        t_rand = None
    flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0) | (L.F_TRAIN if is_train else 0)
    model._sync()

    fused = network_query_fn is None or getattr(network_query_fn, "_cfnerf_fused", False)
    if not fused:
        # the reference's graph runs from ray_batch to the loss whatever the query function is: rays that ask for a gradient stay on it
        return _render_rays_unfused(ray_batch.to(torch.float32) if want_rays else rays, model, network_fn, network_query_fn, t_vals, t_rand, eps, is_train, lindisp, white_bkgd)

    if (want_rays or want_eps) and fused and N > 0:
        # CFNERF_F_RAY_GRAD: gradients reach ray_batch (columns 6, 7 - near / far - get zeros) whether or not the network is frozen.  The eval
        # branch is a graph in the reference too: it runs the stashed train-branch launch on the fixed eval latents (no jitter unless asked
        # for) and returns the eval structure, like NeRF_Flows.forward(is_test=True) with an input gradient wanted.
        # CFNERF_F_EPS_GRAD likewise: explicit latents that ask for a gradient get it from either branch, frozen network or not.
        rgb_map, disp, depth, ent, raw, pts, wts = _RenderFn.apply(model.flat, model, ray_batch.to(torch.float32) if want_rays else rays, t_vals, t_rand, eps,
                                                                   flags | L.F_TRAIN, is_train, None, bool(retweights))
        ret = {'rgb_map': rgb_map, 'disp_map': disp, 'depth_map': depth}
        if is_train:
            ret.update(raw=raw, loss_entropy=ent.reshape(1, 1, 1).expand(N * S, K, 1), pts=pts)
        if retweights:
            ret['weights'] = wts                 # on the graph: a distortion / ray-entropy regulariser trains through it
        return ret

    if is_train and N > 0 and torch.is_grad_enabled() and model.flat.requires_grad:
        rgb_map, disp, depth, ent, raw, pts, wts = _RenderFn.apply(model.flat, model, rays, t_vals, t_rand, eps, flags, True, None, bool(retweights))
        ret = {'rgb_map': rgb_map, 'disp_map': disp, 'depth_map': depth, 'raw': raw,
               'loss_entropy': ent.reshape(1, 1, 1).expand(N * S, K, 1), 'pts': pts}
        if retweights:
            ret['weights'] = wts                 # on the graph: a distortion / ray-entropy regulariser trains through it
        return ret

    o = _render_fwd(model, rays, t_vals, t_rand, eps, flags, raw=is_train, weights=retweights, pts=is_train)
    ret = {k: o[k] for k in ('rgb_map', 'disp_map', 'depth_map')}
    if is_train:
        ret['raw'] = o['raw']
        ret['loss_entropy'] = o['entropy'].reshape(1, 1, 1).expand(N * S, K, 1)
        ret['pts'] = o['pts']
    if retweights:
        ret['weights'] = o['weights']
    return ret


def _render_rays_hierarchical(ray_batch, network_fn, N_samples, N_importance, is_train, lindisp, perturb, white_bkgd, t_rand,
                              eps_alpha, eps_rgb, t_vals, u_fine):
    """EXTENSION, not in the reference: classic coarse+fine sampling through the single CF-NeRF network.
    Coarse pass on ``t_vals`` (default ``linspace(0,1,N_samples)``), ``cfnerf_sample_pdf`` on the K-mean coarse weights,
    fine pass on the merged depths.  Under autograd the FINE pass is differentiated (explicit-depth STASH launch +
    ``cfnerf_render_bwd``); the resampled depths are constants, as nerf-pytorch detaches ``z_samples``, and the coarse
    pass only provides the sampling distribution (one network, one stash: its outputs ``rgb0`` / ``disp0`` / ``depth0``
    are returned detached - ``train.Trainer.step_hierarchical`` adds a coarse loss term with a second stashed pass).
    Parity is pinned against the build's own CPU restatement of nerf-pytorch's ``sample_pdf`` only - the reference has
    nothing to compare with."""
    model = _unwrap(network_fn)
    dev = ray_batch.device
    rays = _f32c(ray_batch)
    N, K = rays.shape[0], model.K_samples
    tv = torch.linspace(0., 1., steps=N_samples).to(dev) if t_vals is None else t_vals.to(dev, torch.float32).contiguous()
    S = tv.shape[0]
    tr = None
    if perturb > 0.:
        tr = _f32c((torch.rand([N, S]) if t_rand is None else t_rand).to(dev))
    eps = _latents(model, LT.pack(eps_alpha, eps_rgb), is_train, dev)
    if u_fine is None:      # det=(perturb == 0.) in nerf-pytorch
        u_fine = torch.linspace(0., 1., steps=N_importance).expand(N, N_importance) if not perturb > 0. else torch.rand(N, N_importance)
    u = _f32c(u_fine.to(dev))
    flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0) | (L.F_TRAIN if is_train else 0)
    model._sync()
    with torch.no_grad():
        c = _render_fwd(model, rays, tv, tr, eps, flags, weights=True)
        z_all = torch.empty(N, S + N_importance, device=dev)
        L.check(L.lib().cfnerf_sample_pdf(L.ptr(rays), L.ptr(tv), L.ptr(tr), flags, L.ptr(c['weights']), L.ptr(u), N, S, K, N_importance,
                                          L.ptr(z_all), L.stream()), "cfnerf_sample_pdf")
    want_eps = torch.is_grad_enabled() and eps.requires_grad       # explicit latents that ask for a gradient: the fine pass gives it (CFNERF_F_EPS_GRAD)
    if N > 0 and torch.is_grad_enabled() and ((is_train and model.flat.requires_grad) or want_eps):
        rgb, disp, depth, ent, _raw, _pts, _wts = _RenderFn.apply(model.flat, model, rays, tv, None, eps, flags | L.F_TRAIN, False, z_all)
        ent = ent.reshape(1)
    else:
        f = _render_fwd(model, rays, tv, None, eps, flags, z_all)
        rgb, disp, depth, ent = f['rgb_map'], f['disp_map'], f['depth_map'], f['entropy']
    ret = {'rgb_map': rgb, 'disp_map': disp, 'depth_map': depth, 'rgb0': c['rgb_map'], 'disp0': c['disp_map'], 'depth0': c['depth_map'],
           'z_vals': z_all}
    if is_train:
        ret['loss_entropy'] = ent.reshape(1, 1, 1).expand(N * (S + N_importance), K, 1)
    return ret


def _render_rays_unfused(rays, model, network_fn, network_query_fn, t_vals, t_rand, eps, is_train, lindisp, white_bkgd):
    """A caller-supplied network_query_fn: sample with the sampling kernel, query through it, composite kernel.  ``rays`` that ask for a
    gradient (render_rays hands over the caller's ray_batch then) keep the reference's graph whole: z_vals and the points handed to the
    query function are on it (_SamplePointsFn), rays_d and viewdirs are slices of it, raw2outputs differentiates in all three arguments."""
    rays_d, viewdirs = rays[:, 3:6], rays[:, 8:11]
    S = t_vals.shape[0]
    if _wants_grad(rays):
        z_vals, pts0 = _SamplePointsFn.apply(rays, t_vals, t_rand, bool(lindisp))                     # RUN:510-534
    else:
        z_vals, pts0 = _sample_points(rays, t_vals, t_rand, lindisp)                                  # RUN:510-534
    # NeRF_Flows.forward consumes it (a custom query fn honours the launch's latents too); the network sees points: one row per point
    if eps.dim() == 3 and _wants_grad(eps):     # (the same rows; an expand's adjoint is a plain sum - no atomics, unlike repeat_interleave's)
        model._next_eps = eps[:, None].expand(eps.shape[0], S, *eps.shape[1:]).reshape(-1, *eps.shape[1:])
    else:
        model._next_eps = eps.repeat_interleave(S, 0) if eps.dim() == 3 else eps
    try:
        raw, loss_entropy = network_query_fn(pts0, viewdirs, network_fn, is_val=False, is_test=not is_train)
    finally:
        model._next_eps = None               # never leaks into a later direct call
    rgb_map, disp_map, weights, depth_map = raw2outputs(raw, z_vals, rays_d, 0., white_bkgd)
    ret = {'rgb_map': rgb_map, 'disp_map': disp_map, 'depth_map': depth_map}
    if is_train:
        ret.update(raw=raw, loss_entropy=loss_entropy, pts=pts0)
    return ret


# --------------------------------------------------------------------------------------------
# Rendering through an occupancy grid (CFNERF_F_CULL): an opt-in EVALUATION path over the unfused seam.  Samples in empty cells never
# reach the network; the composite takes raw rows for the kept samples only.  Inference only; one synchronising device-to-host copy per
# call (the kept count) - the train step's "nothing synchronises" contract is about the train step and is not affected.
@torch.no_grad()
def cull_points(ray_batch, grid, t_vals=None, t_rand=None, lindisp=False, outside="keep"):
    """cfnerf_sample_points with CFNERF_F_CULL on the packed ``ray_batch [N,11]`` and an ``evaluate.OccupancyGrid``: the sampling lines of
    render_rays (RUN:510-534) + the keep / skip decision of every sample + the compact list of the kept points, in (ray, sample) order.
    A sample is kept iff the cell ``floor((p - lo) * scale)`` of its point is occupied; ``outside`` = ``"keep"`` / ``"cull"`` decides for
    points outside the box.  Returns ``z_vals [N,S]`` (the bits of the plain call), ``slot [N,S]`` int32 (row in the compact list, -1 =
    culled), ``ray_start [N+1]`` int64, ``pts [P',3]``, ``ray_of [P']`` int32 and ``count`` = P' (read back from the device: this call
    synchronises)."""
    z_vals, slot, ray_start, pts_c, ray_of = _cull_launch(ray_batch, grid, t_vals, t_rand, lindisp, outside)
    count = int(ray_start[-1].item())                                # the one device-to-host copy: it synchronises
    return {'z_vals': z_vals, 'slot': slot, 'ray_start': ray_start, 'pts': pts_c[:count], 'ray_of': ray_of[:count], 'count': count}


def _cull_launch(ray_batch, grid, t_vals=None, t_rand=None, lindisp=False, outside="keep"):
    """the launches of ``cull_points`` without the copy of the kept count: ``(z_vals, slot, ray_start, pts_c [N*S,3], ray_of [N*S])``"""
    _need_gpu(ray_batch, "ray_batch")
    if outside not in ("keep", "cull"):
        raise ValueError(f"outside must be 'keep' or 'cull', got {outside!r}")
    rays = _f32c(ray_batch)
    dev = rays.device
    t_vals = t_vals_table(dev) if t_vals is None else t_vals.to(dev, torch.float32).contiguous()
    t_rand = None if t_rand is None else _f32c(t_rand.to(dev))
    N, S = rays.shape[0], t_vals.shape[0]
    bits = grid.bits_on(dev)
    z_vals = torch.empty(N, S, device=dev)
    slot = torch.empty(N, S, dtype=torch.int32, device=dev)
    ray_start = torch.empty(N + 1, dtype=torch.int64, device=dev)
    pts_c = torch.empty(N * S, 3, device=dev)
    ray_of = torch.empty(N * S, dtype=torch.int32, device=dev)
    if N == 0:                                                       # (empty batch: no buffer to describe, nothing to launch)
        return z_vals, slot, ray_start.zero_(), pts_c, ray_of
    f3 = lambda v: (C.c_float * 3)(*(float(x) for x in v))           # (fp32 values: exact through Python's float)
    d = L.Cull(L.dptr(bits), f3(grid.lo), f3(grid.scale), (C.c_int32 * 3)(*(int(r) for r in grid.res)), int(outside == "cull"),
               L.dptr(slot), L.dptr(ray_start), L.dptr(pts_c), L.dptr(ray_of))
    L.check(L.lib().cfnerf_sample_points(L.ptr(rays), L.ptr(t_vals), L.ptr(t_rand), (L.F_LINDISP if lindisp else 0) | L.F_CULL, N, S,
                                         L.ptr(z_vals), L.struct_arg(d), L.stream()), "cfnerf_sample_points")
    return z_vals, slot, ray_start, pts_c, ray_of


def raw2outputs_sparse(raw_c, slot, ray_start, z_vals, rays_d, white_bkgd=False, retweights=False):
    """raw2outputs (RUN:411-454) on ``raw_c [P',K,4]``, the rows of the kept samples of ``cull_points`` alone: the tuple raw2outputs returns,
    ``(rgb_map [N,3,K], disp_map [N,K], weights [N,S,K] or None without retweights, depth_map [N,K])`` - bit for bit what raw2outputs gives
    on the dense raw in which every culled sample has the density latent -1e4.  Inference only."""
    _need_gpu(raw_c, "raw_c")
    if _wants_grad(raw_c):
        raise RuntimeError("raw2outputs_sparse is inference only (the sparse composite has no backward): call it under torch.no_grad(), or "
                           "scatter the rows into a dense raw and use raw2outputs for a differentiable composite")
    raw_c, z_vals, rays_d = _f32c(raw_c), _f32c(z_vals), _f32c(rays_d)
    N, S = z_vals.shape
    if raw_c.dim() != 3 or raw_c.shape[2] != 4:
        raise ValueError(f"raw_c must be [P',K,4], got {tuple(raw_c.shape)}")
    if tuple(slot.shape) != (N, S) or slot.dtype != torch.int32 or tuple(ray_start.shape) != (N + 1,) or ray_start.dtype != torch.int64:
        raise ValueError("slot must be int32 [N,S] and ray_start int64 [N+1], as cull_points returns them")
    K, dev = raw_c.shape[1], z_vals.device
    rgb_map = torch.empty(N, 3, K, device=dev)
    disp_map = torch.empty(N, K, device=dev)
    depth_map = torch.empty(N, K, device=dev)
    weights = torch.empty(N, S, K, device=dev) if retweights else None
    sp = L.SparseRaw(L.dptr(slot.contiguous()), L.dptr(ray_start.contiguous()), L.dptr(weights))
    L.check(L.lib().cfnerf_composite_fwd(L.ptr(raw_c) if raw_c.numel() else None, L.ptr(z_vals), L.ptr(rays_d), N, S, K,
                                         int(bool(white_bkgd)) | L.F_CULL, L.ptr(rgb_map), L.ptr(disp_map), L.ptr(depth_map), L.struct_arg(sp),
                                         L.stream()), "cfnerf_composite_fwd")
    return rgb_map, disp_map, weights, depth_map


@torch.no_grad()
def render_rays_culled(ray_batch, network_fn, grid, t_vals=None, lindisp=False, white_bkgd=False, retweights=False, outside="keep"):
    """Eval render of ``ray_batch [N,11]`` through an ``evaluate.OccupancyGrid`` (eval branch, eval latents): ``cull_points`` -> cfnerf_embed
    of the kept points -> the view-direction embedding gathered by ``ray_of`` -> ``NeRF_Flows.forward(x_c, is_test=True)`` on the P' kept
    points -> ``raw2outputs_sparse``.  Returns ``{'rgb_map' [N,3,K], 'disp_map' [N,K], 'depth_map' [N,K], 'count': P'}`` (+ ``weights``).
    With P' = 0 the network is not called: an empty ray is the background.  With an all-ones grid the result has the bits of the unfused
    pipeline (sample, embed, forward, raw2outputs)."""
    model = _unwrap(network_fn)
    c = cull_points(ray_batch, grid, t_vals=t_vals, lindisp=lindisp, outside=outside)
    rays = _f32c(ray_batch)
    K, count = model.K_samples, c['count']
    if count > 0:
        ic, icv = model.input_ch, model.input_ch_views
        x_c = torch.empty(count, ic + icv, device=rays.device)
        x_c[:, :ic] = _embed_fwd(c['pts'], (ic - 3) // 6, ic)
        x_c[:, ic:] = _embed_fwd(rays[:, 8:11].contiguous(), (icv - 3) // 6, icv)[c['ray_of'].long()]
        raw_c = network_fn(x_c, False, True)[0]
    else:
        raw_c = torch.empty(0, K, 4, device=rays.device)
    rgb_map, disp_map, weights, depth_map = raw2outputs_sparse(raw_c, c['slot'], c['ray_start'], c['z_vals'], rays[:, 3:6].contiguous(),
                                                               white_bkgd=white_bkgd, retweights=retweights)
    ret = {'rgb_map': rgb_map, 'disp_map': disp_map, 'depth_map': depth_map, 'count': count}
    if retweights:
        ret['weights'] = weights
    return ret


# --------------------------------------------------------------------------------------------
# Sampling through an occupancy grid (evaluate.OccupancySampler): the grid as a SAMPLING AID on the fused path, train and eval.  All S
# depths of a ray are placed inside the occupied part of it; the render is the existing explicit-depth launch (z_vals), so stash, backward,
# ray gradient and slices are the ones the hierarchical extension uses.  The ray probes are the cull kernel (no synchronising copy); the
# depth warp is elementwise torch on N x (2 bins + 1 + S) values, like the sampling adjoint of the unfused seam - no kernel, flag or
# struct member is added.
_WARP_PROBE_BYTES = 256 << 20      # bound of the buffers of one probe launch: _cull_launch allocates 24 bytes per probe
_PROBE_T_CACHE = {}


def _probe_t_vals(bins, device):
    """``linspace(0, 1, 2 bins + 1)`` (made on the CPU, one device copy per ``(bins, device)`` - read-only)"""
    key = (int(bins), str(torch.device(device)))
    t = _PROBE_T_CACHE.get(key)
    if t is None:
        t = _PROBE_T_CACHE[key] = torch.linspace(0., 1., steps=2 * int(bins) + 1).to(device)
    return t


def warp_probe_chunk(bins):
    """Rays of one probe launch of ``warp_z_vals``: as many as keep its buffers (24 bytes per probe) under 256 MiB"""
    return max(1, (_WARP_PROBE_BYTES // 24) // (2 * int(bins) + 1))


def bins_from_probes(probes, pad=0):
    """The bin rule of ``warp_z_vals`` in torch (any device): ``probes [N, 2 bins + 1]`` bool -> ``[N, bins]`` bool.  Bin ``b`` is occupied iff
    probe ``2b``, ``2b + 1`` or ``2b + 2`` is (its two ends and its middle); the result is grown by ``pad`` bins on both sides along the ray
    (a 1-D max-pool)."""
    b = probes[:, 0:-1:2] | probes[:, 1::2] | probes[:, 2::2]
    pad = int(pad)
    if pad > 0 and b.shape[1] > 0:
        b = torch.nn.functional.max_pool1d(b[:, None].to(torch.float32), kernel_size=2 * pad + 1, stride=1, padding=pad)[:, 0] > 0
    return b


def bins_from_probes_reference(probes, pad=0):
    """``bins_from_probes`` as a plain numpy loop (tests)"""
    import numpy as np
    probes = np.asarray(probes, dtype=bool)
    N, B = probes.shape[0], (probes.shape[1] - 1) // 2
    raw = np.zeros((N, B), dtype=bool)
    for n in range(N):
        for b in range(B):
            raw[n, b] = probes[n, 2 * b] or probes[n, 2 * b + 1] or probes[n, 2 * b + 2]
    out = raw.copy()
    for n in range(N):
        for b in range(B):
            if raw[n, b]:
                out[n, max(b - int(pad), 0):b + int(pad) + 1] = True
    return out


def probe_occupancy_reference(pts, grid, outside="cull"):
    """The cell rule of the cull kernel restated in fp32 torch on the CPU (tests): ``pts [N,P,3]`` -> ``[N,P]`` bool.  The cell of a point is
    ``floor((p - lo) * scale)`` per axis (subtract, multiply, floor - each rounded to fp32), inside iff ``0 <= cell < res``, occupied iff its
    bit of ``grid.bits`` is set; a point outside the box is occupied iff ``outside == "keep"``.  A point on a cell face belongs to the upper cell."""
    pts = pts.detach().to("cpu", torch.float32)
    lo, scale = torch.tensor(grid.lo), torch.tensor(grid.scale)
    res = torch.tensor(grid.res, dtype=torch.float32)
    t = torch.floor((pts - lo) * scale)
    inside = ((t >= 0) & (t < res)).all(-1)
    i = torch.where(inside[..., None], t, torch.zeros_like(t)).long()
    cell = (i[..., 0] * grid.res[1] + i[..., 1]) * grid.res[2] + i[..., 2]
    words = grid.bits.detach().to("cpu", torch.int64)
    occ = ((words[cell >> 5] >> (cell & 31)) & 1).bool()
    return torch.where(inside, occ, torch.full_like(occ, outside == "keep"))


def warp_from_bins(z_plain, near, far, bins):
    """The depth warp of ``warp_z_vals`` as a pure torch function (any device; fp32): ``z_plain [N,S]`` (non-decreasing along a ray),
    ``near`` / ``far [N]``, ``bins [N,B]`` bool -> ``(z_vals [N,S], n_occ [N] int32)``.  With ``n`` = occupied bins of the ray:

        f = clamp((z_plain - near) / (far - near), 0, 1);  target = f n;  i = min(floor(target), n - 1);  r = target - i
        b = index of the i-th occupied bin (0-based, ascending);  z = near + (far - near) (b + r) / B

    i.e. the share ``f`` of the ray's length becomes the same share of its OCCUPIED length.  A ray with ``n == 0`` or ``n == B`` keeps
    ``z_plain`` bit for bit.  Every step is monotone, so ``z`` is non-decreasing like ``z_plain``."""
    N, B = bins.shape
    near, far = near.reshape(N, 1).to(torch.float32), far.reshape(N, 1).to(torch.float32)
    z_plain = z_plain.to(torch.float32)
    csum = bins.to(torch.int64).cumsum(1)                            # occupied bins up to and including b
    n = csum[:, -1:] if B > 0 else csum.new_zeros(N, 1)
    nf = n.to(torch.float32)
    target = ((z_plain - near) / (far - near)).clamp(0., 1.) * nf
    i = torch.minimum(torch.floor(target), (nf - 1.).clamp_min(0.))
    r = target - i
    b = torch.searchsorted(csum, i.to(torch.int64) + 1).clamp_max(max(B - 1, 0))       # the first bin with i + 1 occupied bins up to it
    z = near + (far - near) * ((b.to(torch.float32) + r) / float(B))
    return torch.where((n == 0) | (n == B), z_plain, z), n.reshape(N).to(torch.int32)


def warp_z_vals_reference(z_plain, near, far, bins):
    """The rules of ``warp_from_bins`` as a plain fp64 numpy loop (tests): ``(z_vals [N,S] float64, n_occ [N])``.  ``z_plain`` / ``near`` /
    ``far`` are read as they are given (the fp32 values of the device, widened)."""
    import numpy as np
    z_plain = np.asarray(z_plain, dtype=np.float64)
    near, far = np.asarray(near, dtype=np.float64).reshape(-1), np.asarray(far, dtype=np.float64).reshape(-1)
    bins = np.asarray(bins, dtype=bool)
    (N, S), B = z_plain.shape, bins.shape[1]
    out, n_occ = z_plain.copy(), np.zeros(N, dtype=np.int64)
    for k in range(N):
        occ = np.flatnonzero(bins[k])
        n = n_occ[k] = len(occ)
        if n == 0 or n == B:
            continue
        for s in range(S):
            f = min(max((z_plain[k, s] - near[k]) / (far[k] - near[k]), 0.0), 1.0)
            target = f * n
            i = min(int(np.floor(target)), n - 1)
            out[k, s] = near[k] + (far[k] - near[k]) * (occ[i] + (target - i)) / B
    return out, n_occ


@torch.no_grad()
def warp_z_vals(ray_batch, sampler, t_vals=None, t_rand=None, lindisp=False):
    """Depths of the packed rays ``ray_batch [N,11]`` placed inside the occupied part of every ray, for an ``evaluate.OccupancySampler``:
    ``{'z_vals' [N,S], 'n_occ' [N] int32, 'bins' [N,bins] bool}``.  Nothing is copied to the host and nothing synchronises.

    * Probes: ``2 bins + 1`` depths per ray, ``near (1 - t) + far t`` for ``t = linspace(0, 1, 2 bins + 1)`` (no jitter, never ``lindisp``),
      tested by the cull kernel (cfnerf_sample_points with CFNERF_F_CULL: its cell rule, faces included); a probe is occupied iff its
      ``slot >= 0``.  Rays are probed ``warp_probe_chunk(bins)`` at a time so that the probe buffers stay under 256 MiB.
    * Bins: ``bins_from_probes`` - bin ``b`` is occupied iff probe ``2b``, ``2b + 1`` or ``2b + 2`` is, then grown by ``sampler.pad``.
    * Plain depths: ``z_plain [N,S]`` = what cfnerf_sample_points writes for ``t_vals`` / ``t_rand`` / ``lindisp`` (RUN:510-532), bit for bit.
    * Warp: ``warp_from_bins``.  A ray with no occupied bin, or with all of them, keeps ``z_plain`` bit for bit: a full grid reproduces the
      dense sampling, an empty ray renders as before.

    The depths are CONSTANTS of the graph, as ``sample_pdf``'s are: nothing is differentiated through the warp.

    Quadrature.  The composite gives a sample the interval up to the NEXT sample (``dists``, RUN:426), so the last sample before a gap
    integrates its density over the whole gap.  With ``pad >= 1``, or a grid that was dilated (``OccupancyGrid.from_network(dilate >= 1)``),
    that sample sits in the low-density margin of an occupied run and the gap contributes next to nothing; with ``pad = 0`` on a tight grid
    it sits inside the object and the gap is rendered as solid.  Use one of the two (the sampler's default is ``pad = 1``)."""
    _need_gpu(ray_batch, "ray_batch")
    rays = _f32c(ray_batch)
    if rays.dim() != 2 or rays.shape[1] != 11:
        raise ValueError(f"ray_batch must be [N,11], got {tuple(rays.shape)}")
    dev = rays.device
    t_vals = t_vals_table(dev) if t_vals is None else t_vals.to(dev, torch.float32).contiguous()
    t_rand = None if t_rand is None else _f32c(t_rand.to(dev))
    N, B = rays.shape[0], int(sampler.bins)
    if N == 0:
        return {'z_vals': torch.empty(0, t_vals.shape[0], device=dev), 'n_occ': torch.empty(0, dtype=torch.int32, device=dev),
                'bins': torch.empty(0, B, dtype=torch.bool, device=dev)}
    z_plain, _ = _sample_points(rays, t_vals, t_rand, lindisp)
    tp, step = _probe_t_vals(B, dev), warp_probe_chunk(B)
    parts = [bins_from_probes(_cull_launch(rays[i:i + step], sampler.grid, tp, None, False, sampler.outside)[1] >= 0, sampler.pad)
             for i in range(0, N, step)]
    bins = parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    z, n_occ = warp_from_bins(z_plain, rays[:, 6], rays[:, 7], bins)
    return {'z_vals': z, 'n_occ': n_occ, 'bins': bins}


def render_rays_warped(ray_batch, network_fn, sampler, is_train, lindisp=False, perturb=0., white_bkgd=False, t_rand=None, eps_alpha=None,
                       eps_rgb=None, t_vals=None, retweights=False, chunk=None):
    """``render_rays`` with its depths warped into the occupied part of every ray (``warp_z_vals`` with an ``evaluate.OccupancySampler``), in
    ONE fused explicit-depth launch - the launches of the hierarchical extension's fine pass: ``_RenderFn`` under autograd (parameter
    gradients, and ``ray_batch.grad`` when the rays ask for one, as for any explicit-depth launch; the depths are constants), the plain
    forward otherwise.  Returns the dict of the fused ``render_rays`` (``rgb_map [N,3,K]``, ``disp_map`` / ``depth_map [N,K]``; ``raw``,
    ``loss_entropy``, ``pts`` when ``is_train``; ``weights`` with ``retweights``) plus ``z_vals [N,S]`` and ``n_occ [N]``.  Latents as in
    ``render_rays``, ``latent_draws = "netchunk"`` (with its ray cut ``chunk``) included; ``t_rand`` / ``perturb`` jitter the plain depths the
    warp starts from."""
    _need_gpu(ray_batch, "ray_batch")
    if ray_batch.dim() != 2 or ray_batch.shape[-1] != 11:
        raise ValueError("ray_batch must be [N,11] = o3,d3,near,far,viewdir3 (use_viewdirs=True)")
    model = _unwrap(network_fn)
    dev = ray_batch.device
    t_vals = t_vals_table(dev) if t_vals is None else t_vals.to(dev, torch.float32).contiguous()
    N, S, K = ray_batch.shape[0], t_vals.shape[0], model.K_samples
    rays = _f32c(ray_batch)
    want_rays = torch.is_grad_enabled() and ray_batch.requires_grad
    explicit = LT.pack(eps_alpha, eps_rgb)
    if is_train:
        tr, eps, _ = LT.train_latents(model.latent_draws, explicit, N=N, S=S, K=K, netchunk=model.netchunk, chunk=chunk, perturb=perturb,
                                      own_t_rand=t_rand is not None)
        t_rand, eps = (tr if t_rand is None else t_rand), LT.to_device(eps, dev)
    else:
        eps = _latents(model, explicit, False, dev)
    if perturb > 0.:
        t_rand = _f32c((torch.rand([N, S]) if t_rand is None else t_rand).to(dev))
    else:
        t_rand = None
    w = warp_z_vals(rays, sampler, t_vals, t_rand, lindisp)
    z = w['z_vals']
    flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0) | (L.F_TRAIN if is_train else 0)
    model._sync()
    want_eps = _wants_grad(eps)                  # explicit latents that ask for a gradient (CFNERF_F_EPS_GRAD), either branch
    if N > 0 and (want_rays or want_eps or (is_train and torch.is_grad_enabled() and model.flat.requires_grad)):
        # (rays that ask for a gradient on the eval branch: the stashed train-branch launch on the eval latents, as in render_rays)
        rgb_map, disp, depth, ent, raw, pts, wts = _RenderFn.apply(model.flat, model, ray_batch.to(torch.float32) if want_rays else rays, t_vals,
                                                                   None, eps, flags | L.F_TRAIN, is_train, z, bool(retweights))
        o = {'rgb_map': rgb_map, 'disp_map': disp, 'depth_map': depth, 'raw': raw, 'entropy': ent, 'pts': pts, 'weights': wts}
    else:
        o = _render_fwd(model, rays, t_vals, None, eps, flags, z_vals=z, raw=is_train, weights=retweights, pts=is_train)
    ret = {k: o[k] for k in ('rgb_map', 'disp_map', 'depth_map')}
    if is_train:
        ret.update(raw=o['raw'], loss_entropy=o['entropy'].reshape(1, 1, 1).expand(N * S, K, 1), pts=o['pts'])
    if retweights:
        ret['weights'] = o['weights']
    ret.update(z_vals=z, n_occ=w['n_occ'])
    return ret


def batchify_rays(rays_flat, chunk=1024 * 32, **kwargs):
    """RUN:88-100."""
    all_ret = {}
    for i in range(0, rays_flat.shape[0], chunk):
        ret = render_rays(rays_flat[i:i + chunk], **kwargs)
        for k in ret:
            all_ret.setdefault(k, []).append(ret[k])
    return {k: (torch.cat(v, 0) if len(v) > 1 else v[0]) for k, v in all_ret.items()}


def render(H, W, focal, chunk=1024 * 32, rays=None, c2w=None, ndc=True, near=0., far=1., use_viewdirs=False,
           c2w_staticcam=None, **kwargs):
    """Render rays (RUN:103-170).  Returns ``[rgb_map [..,3,K], disp_map [..,K], depth_map [..,K], extras]``.

    ``chunk`` does not affect results (RUN:112-113); here it does not even split the launch: the fused
    kernel tiles rays internally and keeps nothing per-point in HBM, so one launch renders the batch.
    """
    if not use_viewdirs:
        raise ValueError("use_viewdirs=False is not supported (the reference's model cannot run it, SURVEY R8)")
    if c2w_staticcam is None and (_wants_grad(c2w) if c2w is not None else _wants_grad(*rays)):
        # a pose or rays that ask for a gradient (pose refinement, registration): the differentiable pack, then the fused node's ray gradient
        sh = (H, W, 3) if c2w is not None else tuple(rays[1].shape)
        packed = pack_rays(H, W, focal, rays=rays if c2w is None else None, c2w=c2w, ndc=ndc, near=near, far=far)
    elif c2w is not None:                        # a host pose goes into the kernel arguments as it is: no device round trip
        dev = kwargs["network_fn"].module.device if hasattr(kwargs.get("network_fn"), "module") else _unwrap(kwargs["network_fn"]).device
        sh = (H, W, 3)
        packed = _pack_rays(H, W, focal, c2w=c2w, ndc=ndc and c2w_staticcam is None, near=near, far=far, device=dev)
        if c2w_staticcam is not None:   # RUN:139-141: view directions from c2w, geometry from the static camera
            vd = packed[:, 8:11].clone()
            _pack_rays(H, W, focal, c2w=c2w_staticcam, ndc=ndc, near=near, far=far, out=packed)
            packed[:, 8:11] = vd
    else:
        _need_gpu(rays[1], "rays")
        sh = tuple(rays[1].shape)
        packed = _pack_rays(H, W, focal, rays=rays, ndc=ndc, near=near, far=far)

    kwargs.setdefault("chunk", chunk)                 # (read only by per-netchunk latents: their layout follows the ray cuts, RUN:88-100)
    all_ret = render_rays(packed, **kwargs)                                   # one launch (see docstring)
    for k in all_ret:
        if k != 'loss_entropy' and k != 'loss_entropy_uniformsample':         # RUN:163
            all_ret[k] = torch.reshape(all_ret[k], list(sh[:-1]) + list(all_ret[k].shape[1:]))
    k_extract = ['rgb_map', 'disp_map', 'depth_map']
    return [all_ret[k] for k in k_extract] + [{k: all_ret[k] for k in all_ret if k not in k_extract}]


# --------------------------------------------------------------------------------------------
def default_args(**over):
    """argparse.Namespace with the reference's defaults for every flag create_nerf() reads (config_parser, RUN:556-719;
    ``use_viewdirs`` on, as every shipped config sets it).  Keyword arguments override."""
    import argparse
    a = argparse.Namespace(
        multires=10, multires_views=4, i_embed=0, use_viewdirs=True, N_importance=0, netdepth=8, netwidth=256, K_samples=4,
        h_alpha_size=32, h_rgb_size=64, z_size=4, n_flows=4, type_flows="triangular", n_hidden=128, netchunk_per_gpu=1024 * 64,
        n_gpus=1, lrate=5e-4, lrate_decay=250, ft_path=None, basedir="./logs/", dataname="leaves", expname="cfnerf", no_reload=True,
        index_step=-1, is_train=True, uniformsample=False, perturb=1.0, N_samples=128, white_bkgd=False, raw_noise_std=0.0,
        dataset_type="llff", no_ndc=False, lindisp=False, beta1=0.0, device=torch.device("cuda"), latent_draws="launch")
    for k, v in over.items():
        setattr(a, k, v)
    return a


def save_checkpoint(path, global_step, network_fn, optimizer=None, trainer=None):
    """The reference's checkpoint dict (RUN:1085-1100): ``global_step``, ``network_fn_state_dict`` with the
    DataParallel ``module.`` key prefix, ``optimizer_state_dict``.  Like the reference's loader (RUN:360, commented
    out) create_nerf never restores the optimiser state; for a fused ``Trainer`` the flat Adam moments are saved."""
    sd = network_fn.state_dict()
    if not any(k.startswith("module.") for k in sd):
        sd = OrderedDict(("module." + k, v) for k, v in sd.items())
    if trainer is not None:
        opt = {"exp_avg": trainer.exp_avg.detach().cpu(), "exp_avg_sq": trainer.exp_avg_sq.detach().cpu(), "t": trainer.t}
    else:
        opt = optimizer.state_dict() if optimizer is not None else {}
    torch.save({'global_step': global_step, 'network_fn_state_dict': {k: v.detach().cpu() for k, v in sd.items()},
                'optimizer_state_dict': opt}, path)
    return path


def _checkpoint_to_reload(args):
    """The checkpoint create_nerf() resumes from, by the reference's rules (RUN:345-357): an explicit ``ft_path`` wins;
    otherwise the log directory ``basedir/dataname/type_flows/expname`` is searched for ``*tar*`` files and either the
    newest one (``index_step == -1``) or ``<index_step>_01.tar`` is taken.  ``no_reload`` disables all of it."""
    if getattr(args, "no_reload", False):
        return None
    ft = getattr(args, "ft_path", None)
    logdir = os.path.join(args.basedir, args.dataname, args.type_flows, args.expname)
    found = [ft] if ft is not None and ft != 'None' else (
        [os.path.join(logdir, f) for f in sorted(os.listdir(logdir)) if 'tar' in f] if os.path.isdir(logdir) else [])
    if not found:
        return None
    return found[-1] if args.index_step == -1 else os.path.join(logdir, '{:06d}_{:02d}.tar'.format(args.index_step, 1))


def _maybe_reload(args, model) -> int:
    """Load network weights from a reference-format checkpoint (RUN:358-378): keys the model does not have are dropped,
    the optimiser state is NOT restored (that line is commented out in the reference).  Returns the global step."""
    path = _checkpoint_to_reload(args)
    if path is None:
        print('No reloading')
        return 0
    print('Reloading from', path)
    ckpt = torch.load(path, map_location="cpu")
    own = model.state_dict()
    own.update({k: v for k, v in ckpt['network_fn_state_dict'].items() if k in own})
    model.load_state_dict(own)
    return ckpt['global_step']


def create_nerf(args):
    """Instantiate the CF-NeRF model (RUN:317-409).  Returns
    ``(render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer)``."""
    args.embed_fn, args.input_ch = get_embedder(args.multires, args.i_embed)
    args.input_ch_views = 0
    args.embeddirs_fn = None
    if args.use_viewdirs:
        args.embeddirs_fn, args.input_ch_views = get_embedder(args.multires_views, args.i_embed)
    args.output_ch = 5 if args.N_importance > 0 else 4
    args.skips = [args.netdepth / 2]                                          # RUN:327
    if not hasattr(args, "device") or args.device is None:
        args.device = torch.device("cuda")
    model = _DataParallelShim(NeRF_Flows(args))
    latent_draws = getattr(args, "latent_draws", "launch")       # not a reference flag: "netchunk" = the reference's per-netchunk latents
    if latent_draws not in LATENT_DRAWS:
        raise ValueError(f"latent_draws must be one of {LATENT_DRAWS}, got {latent_draws!r}")
    model.module.latent_draws = latent_draws
    model.module.netchunk = args.netchunk_per_gpu * max(1, getattr(args, "n_gpus", 1))
    grad_vars = list(model.parameters())

    def network_query_fn(inputs, viewdirs, network_fn, is_val, is_test):
        return run_network(inputs, viewdirs, network_fn, is_val, is_test, embed_fn=args.embed_fn,
                           embeddirs_fn=args.embeddirs_fn, netchunk=args.netchunk_per_gpu * max(1, getattr(args, "n_gpus", 1)))
    network_query_fn._cfnerf_fused = True        # render_rays may replace query + composite by the fused launch

    optimizer = torch.optim.Adam(params=grad_vars, lr=args.lrate, betas=(0.9, 0.999))
    start = _maybe_reload(args, model)

    render_kwargs_train = {
        'is_train': args.is_train, 'uniformsample': args.uniformsample, 'network_query_fn': network_query_fn,
        'perturb': args.perturb, 'N_importance': args.N_importance, 'N_samples': args.N_samples,
        'K_samples': args.K_samples, 'network_fn': model, 'use_viewdirs': args.use_viewdirs,
        'white_bkgd': args.white_bkgd, 'raw_noise_std': args.raw_noise_std,
    }
    if args.dataset_type != 'llff' or args.no_ndc:                            # RUN:397-400
        print('Not ndc!')
        render_kwargs_train['ndc'] = False
        render_kwargs_train['lindisp'] = args.lindisp
    render_kwargs_test = {k: render_kwargs_train[k] for k in render_kwargs_train}
    render_kwargs_test['perturb'] = False
    render_kwargs_test['raw_noise_std'] = 0.
    render_kwargs_test['is_train'] = False
    render_kwargs_test['uniformsample'] = False
    render_kwargs_test['retraw'] = True
    return render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer
