"""Train step of the CF-NeRF hot path on the HIP kernels (reference: train() inner loop, RUN:1013-1077).

One process per GPU.  A step is: ray set-up -> fused forward (activations stashed) -> KDE-NLL loss
(+ beta1 * entropy) -> backward -> ONE all-reduce (sum) of the flat gradient over RCCL when
world_size > 1 -> fused Adam on the flat buffers -> re-pack.  Rays are sharded by the caller
(rank r renders its own N_rand rays); every rank holds the full weights and applies the same update.

Gradient normalisation across ranks: the reference's losses are means over rays / points
(RUN:1042,1045).  Each rank computes the gradient of  nll_local_sum / (3 * N_total) + (beta1 / world) *
entropy_local, so the SUM over ranks is the gradient of the global means for equal shards.

Depth supervision (the reference's ``colmap_depth``, RUN:1009-1024,1052-1054): a step may carry N_d extra rays through key
points of known depth; they are rendered in the SAME launch behind the N colour rays and add
``depth_lambda * mean_i (mean_K depth_map[N + i] - target_depth[i])^2`` to the loss.  The rule above extends by one term: each
rank differentiates  nll_local / (3 N world) + depth_lambda * sq_local / (N_d world) + (beta1 / world) * entropy_local.
``depth_term`` forms that term and its cotangent ``d_depth_map`` on the device from the forward's depth map.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib as L
from . import latents as LT
from .api import NeRF_Flows, _f32c, _pack_rays, _unwrap, t_vals_table, warp_z_vals


def backward_available() -> bool:
    """True when libcfnerf_hip.so carries the real backward (an empty batch is accepted)."""
    rc = L.lib().cfnerf_loss_fwd_bwd(None, None, None, 0, 2, C.c_float(0.0), 0, None, None, None)
    return rc == 0


def shard_bounds(n_rays: int, rank: int, world: int):
    """Contiguous equal shards (the reference's DataParallel splits the same way along dim 0)."""
    if n_rays % world:
        raise ValueError(f"N_rand ({n_rays}) must be divisible by world_size ({world})")
    per = n_rays // world
    return rank * per, (rank + 1) * per


def lr_at(lrate: float, lrate_decay: int, start: int, t: int) -> float:
    """Learning rate used by the t-th optimiser step of this run (RUN:1073-1077: the decayed rate is
    written to the param groups AFTER optimizer.step(), computed from the current global_step)."""
    if t == 0:
        return lrate
    return lrate * (0.1 ** ((start + t - 1) / (lrate_decay * 1000)))


def _collective_(op, t: torch.Tensor, group=None):
    """The in-place collective ``op(tensor)`` on ``t``; a gloo group (CPU tests, ranks sharing one GPU) gets a GPU tensor through a host copy."""
    import torch.distributed as dist
    if t.is_cuda and dist.get_backend(group) == "gloo":
        host = t.cpu()
        op(host)
        t.copy_(host)
    else:
        op(t)
    return t


def allreduce_sum_(grad: torch.Tensor, world: int, group=None, force: bool = False):
    """ONE sum all-reduce of the flat buffer (RCCL over xGMI when the group's backend is "nccl")."""
    if world > 1 or force:
        import torch.distributed as dist
        _collective_(lambda t: dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group), grad, group)
    return grad


MAX_K = 128     # kMaxK of the kernels


def depth_term(depth_rows: torch.Tensor, target_depth: torch.Tensor, depth_lambda: float, n_depth_total: int):
    """The depth-supervision term of ``n`` key-point rays (RUN:1020,1023,1053-1054) and its cotangent:
    ``contribution [1] = depth_lambda * sum_i (mean_k depth_rows[i,:] - target_depth[i])^2 / n_depth_total`` and
    ``d_depth_rows [n,K] = d contribution / d depth_rows = 2 depth_lambda (mean_k depth_rows[i,:] - target_depth[i]) / (n_depth_total K)``.
    ``n_depth_total`` is the step's number of depth rays over all ranks and slices, so contributions add up to
    ``depth_lambda * img2mse`` and cotangents concatenate.  Tensors in and out on the inputs' device, no host synchronisation.
    (The one place the term is formed: ``cfnerf_loss_fwd_bwd`` has no argument that could carry it.)"""
    K = depth_rows.shape[-1]
    diff = depth_rows.mean(-1) - target_depth
    d_rows = (diff * (2.0 * depth_lambda / (n_depth_total * K)))[:, None].expand(-1, K).contiguous()
    return d_rows, ((diff * diff).sum() * (depth_lambda / n_depth_total)).reshape(1)


class Trainer:
    """Fused train step on one rank.  Multi-GPU: construct with ``world_size`` (and ``group``) after
    ``torch.distributed.init_process_group``; every rank renders its own shard of the step's rays.

    Latent samples (latents.py describes draw order and layout): the reference draws eps once per forward call; here every rank must
    use the SAME eps in a step.  That is enforced, not assumed: rank 0 draws the latents of step t+1 and they travel in a 4*K-float tail of
    the step-t gradient all-reduce (the other ranks contribute zeros there), so no extra collective and no reliance on
    identical seeding; step 0 uses one broadcast.  An explicit ``eps=`` argument overrides this (tests, benchmarks): ``[K,4]`` for
    the whole step or ``[N,K,4]``, one row per ray of this rank's shard.

    ``latent_draws="netchunk"``: the reference's per-netchunk latents (latents.py has the draw order and the row layout).  A step
    draws the ``C = netchunk_count(N_global, S, netchunk, chunk)`` latent pairs of the GLOBAL batch (on one process together with t_rand),
    every rank takes the rows of its own ray range (shard_bounds), and the ``C*K*4`` latents travel in the all-reduce tail like the one
    set of the default mode.  ``eps_chunks=[C,K,4]`` gives them explicitly.

    ``depth_lambda > 0``: ``step`` / ``forward_backward`` accept ``depth_rays=`` / ``target_depth=`` (data.DepthRayPool feeds them) and
    add the reference's depth-supervision term (module docstring; forward_backward has the entropy rule).  Without depth rays a step is
    the plain step whatever ``depth_lambda`` is.

    ``ray_grad=True`` (one rank): ``forward_backward`` / ``step`` also leave ``self.d_rays [N,11]`` = d loss / d (the packed rays) and
    ``self.d_z [N,S]`` = d loss / d z_vals of the step's WHOLE loss (means over the full batch), rows in launch order - colour rays, then
    depth rays (CFNERF_F_RAY_GRAD; columns 6, 7 of ``d_rays`` - near / far - are zero, cfnerf.h).  ``api.pack_rays(...).backward(trainer.d_rays)``
    chains them into a pose.  The default changes nothing: same buffers, same launches.

    ``latent_grad=True`` (one rank): ``forward_backward`` / ``step`` also leave ``self.d_eps`` = d loss / d (the step's latents) of the step's
    WHOLE loss, summed over the slices of a sliced step (CFNERF_F_EPS_GRAD): ``[K,4]`` for one latent set, ``[C,K,4]`` - one per pair, in
    draw order - in netchunk mode, ``[N,K,4]`` for explicit per-ray rows; columns rgb then alpha, like the latents.  The default changes
    nothing: same buffers, same launches.  ``forward_backward_hierarchical`` / ``step_hierarchical`` refuse the option (their passes never
    carry the flag: the blocks behind the parameter gradient are sized by ``forward_backward`` alone).

    ``distortion_lambda`` / ``ray_entropy_lambda`` > 0: the step's loss gains ``api.ray_regularizers`` of every ray of the launch (depth
    rays included; means over the step's rays of all ranks; ``ray_entropy_acc_min`` is its ``acc_min``) - the distortion loss of mip-NeRF 360
    and the ray entropy of InfoNeRF on the composite's weights.  ``self.scalars[0]`` includes the term and ``self.reg_scalars`` holds
    ``[reg, dist, ent, frac]`` of the step; with ``ray_grad`` the direct gradient in the depths is added to ``self.d_z``.  Works with slices,
    depth rays, ``occupancy=`` (the warped depths), netchunk latents and both precisions; the hierarchical extension refuses it.  With both
    at 0 (the default) a step launches what it launched and writes the bits it wrote."""

    def __init__(self, net, lrate=5e-4, lrate_decay=250, beta1=0.0, world_size=1, group=None, start=0, force_allreduce=False,
                 overlap_comm=False, time_comm=False, max_rays_per_launch=None, latent_draws="launch", netchunk=1024 * 64, chunk=1024 * 32,
                 depth_lambda=0.0, ray_grad=False, latent_grad=False, distortion_lambda=0.0, ray_entropy_lambda=0.0, ray_entropy_acc_min=0.1):
        if latent_draws not in LT.LATENT_DRAWS:
            raise ValueError(f"latent_draws must be one of {LT.LATENT_DRAWS}, got {latent_draws!r}")
        if ray_grad and (int(world_size) > 1 or force_allreduce):
            raise NotImplementedError("Trainer(ray_grad=True) with world_size > 1 / force_allreduce: the ray blocks of CFNERF_F_RAY_GRAD lie behind "
                                      "the parameter gradient in the buffer whose tail the gradient exchange uses for the next step's latents")
        if latent_grad and (int(world_size) > 1 or force_allreduce):
            raise NotImplementedError("Trainer(latent_grad=True) with world_size > 1 / force_allreduce: the latent blocks of CFNERF_F_EPS_GRAD lie behind "
                                      "the parameter gradient in the buffer whose tail the gradient exchange uses for the next step's latents")
        if distortion_lambda < 0 or ray_entropy_lambda < 0:
            raise ValueError("distortion_lambda and ray_entropy_lambda must not be negative")
        self.ray_grad = bool(ray_grad)
        self.d_rays = self.d_z = None
        # the ray regularisers (CFNERF_F_RAY_REG): weights of the two terms, and whether a pass runs them at all
        self.distortion_lambda, self.ray_entropy_lambda = float(distortion_lambda), float(ray_entropy_lambda)
        self.ray_entropy_acc_min = float(ray_entropy_acc_min)
        self._reg = self.distortion_lambda > 0.0 or self.ray_entropy_lambda > 0.0
        self._reg_n = None
        self.latent_grad = bool(latent_grad)
        self.d_eps = None
        self.latent_draws, self.netchunk, self.chunk = latent_draws, int(netchunk), (int(chunk) if chunk else None)
        # max_rays_per_launch: a step's shard larger than this is walked in EQUAL slices (forward -> loss -> backward per slice, the
        # gradient accumulated by cfnerf_render_bwd_accumulate, ONE exchange and ONE Adam step at the end): the train-step workspace
        # is sized for a slice (3 MiB per ray at W = 256), not for the batch - the reference trains any N_rand (RUN:88-100,602)
        self.max_rays = None if not max_rays_per_launch else int(max_rays_per_launch)
        self.force_allreduce = bool(force_allreduce)
        self.overlap_comm = bool(overlap_comm)
        # time_comm: two events on the compute stream around every gradient exchange - what the exchange EXPOSES on that stream
        # (an exchange that ran entirely under compute would read ~0); read back with comm_stats()
        self._comm_ev = [] if time_comm else None
        self.net: NeRF_Flows = _unwrap(net)
        dev = self.net.flat.device
        self.lrate, self.lrate_decay, self.beta1 = float(lrate), int(lrate_decay), float(beta1)
        self.world, self.group, self.start = int(world_size), group, int(start)
        self.rank = 0
        import torch.distributed as dist
        if (self.world > 1 or self.force_allreduce) and dist.is_available() and dist.is_initialized():
            self.rank = dist.get_rank(group)       # (world_size > 1 without a process group: shard semantics only, see forward_backward)
        n = self.net.n_params
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        self.gbuf = torch.zeros(n + 4 * MAX_K, device=dev)      # flat gradient | next step's latents (rank 0's, via the all-reduce)
        self.grad = self.gbuf[:n]
        self._eps_next = None
        self.d_ent = torch.tensor([self.beta1 / self.world], device=dev)
        # loss, loss_nll, mse, psnr of the local shard; loss and loss_nll are CONTRIBUTIONS (nll / (3 N_total) and
        # beta1 / world on the shard's entropy): their sum over ranks is the global value (RUN:1042-1050)
        self.scalars = torch.zeros(4, device=dev)
        self.entropy = torch.zeros(1, device=dev)
        # depth supervision: weight of the term, and this rank's contribution to the step's depth_loss (the reference's train/depth_loss)
        self.depth_lambda = float(depth_lambda)
        self.depth_loss = torch.zeros(1, device=dev)
        self._d_depth_n = None
        # [reg, dist, ent, frac] of the step's ray regularisers on the local shard (contributions: means over the step's rays of all ranks)
        self.reg_scalars = torch.zeros(4, device=dev)
        self.t = 0
        self._buf_n = None
        self._eps_rows = None           # this step's latent rows (netchunk mode): the stash reads them until the backward

    # ---- gradient exchange ---------------------------------------------------------------------------------------
    def _exchange_plan(self):
        """Index tensors of the two buckets: `early` = flat ranges that are final before the backward's last launch
        (cfnerf_grad_early_ranges), `late` = the rest + the latents tail.  Built once, after the first backward."""
        if getattr(self, "_xplan", None) is None:
            lib, n = L.lib(), self.net.n_params
            offs, cnts = (C.c_int64 * 64)(), (C.c_int64 * 64)()
            k = lib.cfnerf_grad_early_ranges(self.net.handle, offs, cnts, 64)
            if k < 0:
                raise RuntimeError("cfnerf_grad_early_ranges: " + lib.cfnerf_last_error().decode())
            dev = self.gbuf.device
            mask = torch.zeros(self.gbuf.numel(), dtype=torch.bool, device=dev)
            for i in range(k):
                mask[offs[i]:offs[i] + cnts[i]] = True
            idx = torch.arange(self.gbuf.numel(), device=dev)
            self._xplan = (idx[mask], idx[~mask])
            self._comm = torch.cuda.Stream(device=dev)
        return self._xplan

    def _exchange(self):
        """Sum the gradient (and the latents tail) over the ranks.  Default: ONE all-reduce of the whole flat buffer
        (2.47 MB at W = 256).  `overlap_comm=True` (RCCL groups): two buckets - the early one (every bias, the base
        Gaussians and the weights fed by the big dW launch alone: ~3/4 of the bytes) is gathered and all-reduced on a side
        stream as soon as those tensors are final, i.e. UNDER the small-job launch that ends the backward (~0.23 ms);
        the late one follows on the main stream.  On ONE GPU, where the exchange itself costs nothing, the gathers,
        scatters and the second launch of the two-bucket form cost ~0.13 ms per step, more than a 2.5 MB all-reduce is
        expected to expose on 8 GPUs - hence opt-in until it can be measured on a multi-GPU node."""
        import torch.distributed as dist
        if not self.overlap_comm or not self.gbuf.is_cuda or dist.get_backend(self.group) != "nccl":
            allreduce_sum_(self.gbuf, self.world, self.group, self.force_allreduce)
            return
        early, late = self._exchange_plan()
        main = torch.cuda.current_stream(self.gbuf.device)
        L.check(L.lib().cfnerf_stream_wait_grad_early(self.net.handle, C.c_void_p(self._comm.cuda_stream)), "cfnerf_stream_wait_grad_early")
        with torch.cuda.stream(self._comm):
            e_buf = self.gbuf.index_select(0, early)
            w_early = dist.all_reduce(e_buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        l_buf = self.gbuf.index_select(0, late)
        dist.all_reduce(l_buf, op=dist.ReduceOp.SUM, group=self.group)
        self.gbuf.index_copy_(0, late, l_buf)
        w_early.wait()                              # the main stream waits for the side stream's all-reduce
        main.wait_stream(self._comm)
        self.gbuf.index_copy_(0, early, e_buf)
        e_buf.record_stream(main)

    def _timed_exchange(self, fn):
        if self._comm_ev is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        self._comm_ev.append((e0, e1))
        if len(self._comm_ev) > 4096:
            del self._comm_ev[:2048]

    def comm_stats(self, last_n=None):
        """Exposed time of the gradient exchange over the last ``last_n`` steps (device-synchronising), its payload and what
        torch.distributed reports about the group - the self-diagnosis block of a multi-GPU bench line."""
        import torch.distributed as dist
        out = {"payload_bytes": int(self.gbuf.numel() * 4), "form": "two buckets (overlap_comm)" if self.overlap_comm else "one all-reduce",
               "backend": None, "world_size_reported": None}
        if dist.is_available() and dist.is_initialized():
            out["backend"] = dist.get_backend(self.group)
            out["world_size_reported"] = dist.get_world_size(self.group)
        ev = (self._comm_ev or [])[-(last_n or 0):]
        if ev:
            ev[-1][1].synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            out.update(exposed_ms_mean=sum(ms) / len(ms), exposed_ms_max=max(ms), exposed_ms_min=min(ms), steps=len(ms))
        return out

    # ---- the latents that ride in the all-reduce tail: shape (K,4), or the (C,K,4) netchunk pairs of the step's global batch ----------
    def _draw(self, shape):
        """Fresh pairs of ``shape`` on the device (pinned, non-blocking: the host keeps running ahead)."""
        return LT.to_device(LT.draw_pairs(math.prod(shape[:-2]), shape[-2]).reshape(shape), self.net.flat.device)

    def _tail(self, shape):
        """The latents tail of the all-reduce buffer, grown (with the gradient view) when a netchunk step needs more than 4*MAX_K."""
        n, numel = self.net.n_params, math.prod(shape)
        if self.gbuf.numel() < n + numel:
            self.gbuf = torch.zeros(n + numel, device=self.gbuf.device)
            self.grad = self.gbuf[:n]
            self._xplan = None
        return self.gbuf[n:n + numel]

    def _step_eps(self, shape=None):
        """Latents of the coming step (default shape: "launch" mode's ``[K,4]``), identical on every rank and on every call before it."""
        shape = (self.net.K_samples, 4) if shape is None else tuple(shape)
        if self.world == 1 and not self.force_allreduce:
            return self._draw(shape)
        if self._eps_next is None or tuple(self._eps_next.shape) != shape:             # first step: one broadcast from rank 0
            import torch.distributed as dist
            eps = self._draw(shape) if self.rank == 0 else torch.zeros(*shape, device=self.net.flat.device)
            src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
            self._eps_next = _collective_(lambda t: dist.broadcast(t, src=src, group=self.group), eps, self.group)
        return self._eps_next

    def _buffers(self, N, K):
        if self._buf_n != (N, K):
            dev = self.net.flat.device
            self.packed = torch.empty(N, 11, device=dev)
            self.rgb_map = torch.empty(N, 3, K, device=dev)
            self.disp = torch.empty(N, K, device=dev)
            self.depth = torch.empty(N, K, device=dev)
            self.d_rgb = torch.empty(N, 3, K, device=dev)
            self._buf_n = (N, K)
            self._d_depth_n = None

    def _depth_buffers(self, n_colour, N, K):
        """The cotangent buffers of a depth-supervised launch of ``n_colour`` colour rows then ``N - n_colour`` depth rows: ``d_rgb`` of the
        depth rows and ``d_depth`` of the colour rows are zero and stay zero (the loss writes colour rows of ``d_rgb`` only, depth_term depth
        rows of ``d_depth`` only), so they are cleared when the buffers or the split change, not per step."""
        if self._d_depth_n != (n_colour, N, K):
            self.d_rgb[n_colour:].zero_()
            self.d_depth = torch.zeros(N, K, device=self.d_rgb.device)
            self._d_depth_n = (n_colour, N, K)

    def _check_depth(self, depth_rays, target_depth, n_colour, S):
        """Refusals of a depth-supervised step; returns None (no depth rays) or ``(depth_rays, target_depth [N_d], first)`` where ``first``
        is None or, in netchunk mode when the batch is several network calls, the rays of the first one."""
        if depth_rays is None and target_depth is None:
            return None
        if depth_rays is None or target_depth is None:
            raise ValueError("depth_rays and target_depth go together")
        if self.depth_lambda == 0.0:
            raise ValueError("depth rays given to a Trainer with depth_lambda = 0: the depth term would be dropped")
        n_d = depth_rays[1].reshape(-1, 3).shape[0]
        target_depth = target_depth.reshape(-1)
        if target_depth.shape[0] != n_d or n_d == 0:
            raise ValueError(f"{n_d} depth rays, {target_depth.shape[0]} depth targets")
        first = None
        if self.latent_draws == "netchunk":
            N = n_colour + n_d
            if self.world > 1:
                raise NotImplementedError("latent_draws='netchunk' with depth rays on several ranks: the reference's ray order puts all colour "
                                          "rays before all depth rays, the ranks' shards interleave them")
            if LT.netchunk_count(N, S, self.netchunk, self.chunk) > 1:
                # the reference cuts the per-POINT entropy tensor to its first n_colour rows (RUN:1024): points of the first network call
                if self.n_slices(N) > 1:
                    raise NotImplementedError("latent_draws='netchunk' with depth rays and max_rays_per_launch on a batch of several network "
                                              "calls: the entropy term is the first network call's alone")
                first = min(self.netchunk // S, LT.ray_cuts(N, self.chunk)[0][1])
        return depth_rays, target_depth, first

    def _ray_grad_buffers(self, N, S, n_max):
        """``d_rays`` / ``d_z`` of a step of N rays, and the gradient buffer grown to hold the ray blocks of its largest pass (``n_max``
        rays) behind the parameter gradient (cfnerf.h, CFNERF_F_RAY_GRAD)"""
        dev = self.net.flat.device
        if self.d_rays is None or tuple(self.d_z.shape) != (N, S):
            self.d_rays, self.d_z = torch.zeros(N, 11, device=dev), torch.zeros(N, S, device=dev)
        need = L.ray_grad_offsets(self.net.n_params, n_max, S)[2]
        if self.gbuf.numel() < need:
            self.gbuf = torch.zeros(need, device=dev)
            self.grad = self.gbuf[:self.net.n_params]
            self._xplan = None

    def _reg_buffers(self, N, S, K, z_vals, t_vals, t_rand, lindisp):
        """The persistent buffers of a step with ray regularisers - the forward's ``weights`` and their cotangent ``[N,S,K]``, the launch's
        8 scalars, the direct ``d_z`` with ``ray_grad`` - and the step's depths: the explicit ``z_vals``, else what the fused forward
        samples for ``t_vals`` / ``t_rand`` / ``lindisp`` (cfnerf_sample_points: the same lines)"""
        dev = self.net.flat.device
        if self._reg_n != (N, S, K):
            self._reg_w, self._reg_dw = torch.empty(N, S, K, device=dev), torch.empty(N, S, K, device=dev)
            self._reg_sc = torch.zeros(8, device=dev)
            self._reg_zbuf = torch.empty(N, S, device=dev)
            self._reg_dz = torch.empty(N, S, device=dev) if self.ray_grad else None
            self._reg_n = (N, S, K)
        self.reg_scalars.zero_()
        if z_vals is not None:
            self._reg_z = z_vals
        else:
            L.check(L.lib().cfnerf_sample_points(L.ptr(self.packed), L.ptr(t_vals), L.ptr(t_rand), L.F_LINDISP if lindisp else 0, N, S,
                                                 L.ptr(self._reg_zbuf), None, L.stream()), "cfnerf_sample_points")
            self._reg_z = self._reg_zbuf

    def _latent_grad_buffers(self, eps, S, n_max):
        """The step's latent gradient, zeroed (``[K,4]`` or one row per ray), and the gradient buffer grown to hold the latent blocks of its
        largest pass (``n_max`` rays) behind the parameter gradient and the ray blocks (cfnerf.h, CFNERF_F_EPS_GRAD)"""
        dev, n = self.net.flat.device, self.net.n_params
        self._d_eps_acc = torch.zeros(eps.shape, device=dev)
        need = L.eps_grad_offsets(L.ray_grad_offsets(n, n_max, S)[2] if self.ray_grad else n, n_max, eps.shape[-2])[2]
        if self.gbuf.numel() < need:
            self.gbuf = torch.zeros(need, device=dev)
            self.grad = self.gbuf[:n]
            self._xplan = None

    def _latent_grad_finish(self, N, S):
        """``self.d_eps`` of the step: the one set's gradient, the rows' - or, in netchunk mode, the pairs': the rows of a pair are one
        contiguous segment of the step's rows, summed in a fixed order (no atomics: bit-reproducible like the blocks themselves)"""
        acc, pairs = self._d_eps_acc, getattr(self, "_step_pairs", None)
        if acc.dim() == 3 and pairs is not None:
            idx = LT.netchunk_row_index(N, S, self.netchunk, self.chunk)
            acc = LT.rows_to_pairs_sum(acc, torch.bincount(idx, minlength=pairs.shape[0]).tolist())
        self.d_eps = acc

    def _pass(self, a, b, t_vals, t_rand, eps, S, flags, target, beta, scalars, entropy, d_ent, grad=None, accumulate=False, z_vals=None,
              weights=None, depth=None, ray_grad=False, latent_grad=False):
        """One pass over rows [a, b) of the packed rays into the persistent buffers: the fused forward (``t_rand`` / ``z_vals`` and the
        optional ``weights [N,S,K]`` output are per-ray too and sliced alike) and, given a ``grad`` buffer, a STASH forward followed by the
        KDE-NLL loss (+ ``beta`` * entropy; means over the step's whole shard) into ``scalars`` and the backward into ``grad``
        (``accumulate``: added to what it holds).  ``depth = (n_colour, target_depth)``: rows from ``n_colour`` on are depth rays - the
        loss runs on the pass's colour rows, depth_term on its depth rows, and the backward gets ``d_depth_map``.
        With ray regularisers (``distortion_lambda`` / ``ray_entropy_lambda``) the stash carries CFNERF_F_COTANGENTS, the forward also writes
        the pass's rows of the persistent ``weights``, one CFNERF_F_RAY_REG launch turns them into ``reg`` (added to ``scalars[0]`` and
        ``self.reg_scalars``) and ``d_weights``, and the backward takes a cotangent descriptor."""
        net, lib, st = self.net, L.lib(), L.stream()
        reg = self._reg and grad is not None
        if reg:
            weights, flags = self._reg_w, flags | L.F_COTANGENTS
        rows = lambda t: t[a:b] if t is not None else None
        n, K = b - a, net.K_samples
        if LT.check_rows(eps, self.packed.shape[0], "rays of the shard"):         # CFNERF_F_EPS_ROWS: the slice's rows
            eps, flags = eps[a:b], flags | L.F_EPS_ROWS
        L.check(lib.cfnerf_render_fwd(net.handle, L.ptr(self.packed[a:b]), L.ptr(t_vals), L.ptr(rows(t_rand)), L.ptr(rows(z_vals)), L.ptr(eps),
                                      n, S, K, flags | (L.F_STASH if grad is not None else 0) | (L.F_RAY_GRAD if ray_grad else 0)
                                      | (L.FLAG_EPS_GRAD if latent_grad and grad is not None else 0),
                                      L.ptr(self.rgb_map[a:b]), L.ptr(self.disp[a:b]),
                                      L.ptr(self.depth[a:b]), None, L.ptr(rows(weights)), None, None, L.ptr(entropy), st), "cfnerf_render_fwd")
        if grad is None:
            return
        d_depth = None
        if depth is None:
            self._d_depth_n = None                                               # (a plain pass writes every row of d_rgb it covers)
            L.check(lib.cfnerf_loss_fwd_bwd(L.ptr(self.rgb_map[a:b]), L.ptr(target[a:b]), L.ptr(entropy), n, K, C.c_float(beta),
                                            self.packed.shape[0] * self.world, L.ptr(self.d_rgb[a:b]), L.ptr(scalars), st), "cfnerf_loss_fwd_bwd")
        else:
            n_colour, target_depth = depth
            hi, lo = max(a, min(b, n_colour)), max(a, n_colour)                  # colour rows [a, hi), depth rows [lo, b) of this pass
            if hi > a:
                L.check(lib.cfnerf_loss_fwd_bwd(L.ptr(self.rgb_map[a:hi]), L.ptr(target[a:hi]), L.ptr(entropy), hi - a, K, C.c_float(beta),
                                                n_colour * self.world, L.ptr(self.d_rgb[a:hi]), L.ptr(scalars), st), "cfnerf_loss_fwd_bwd")
            else:                                                                # no colour row: the entropy term is all the loss kernel would add
                scalars.zero_()
                if beta:
                    scalars[0:1] = beta * entropy
            if b > lo:
                n_d = self.packed.shape[0] - n_colour
                self.d_depth[lo:b], part = depth_term(self.depth[lo:b], target_depth[lo - n_colour:b - n_colour], self.depth_lambda,
                                                      n_d * self.world)
                scalars[0:1] += part
                self.depth_loss += part / self.depth_lambda
                d_depth = self.d_depth[a:b]
        d_rgb_arg = L.ptr(self.d_rgb[a:b])
        if reg:                                 # every ray of the launch, depth rays included; means over the step's rays of all ranks
            L.ray_reg(self._reg_w[a:b], self._reg_z[a:b], self._reg_dw[a:b], self._reg_sc, rays=self.packed[a:b],
                      d_z=self._reg_dz[a:b] if ray_grad else None, lambda_dist=self.distortion_lambda, lambda_ent=self.ray_entropy_lambda,
                      acc_min=self.ray_entropy_acc_min, n_total=self.packed.shape[0] * self.world, stream_=st)
            scalars[0:1] += self._reg_sc[0:1]
            self.reg_scalars += self._reg_sc[:4]
            cot = L.cotangents(self.d_rgb[a:b], None, self._reg_dw[a:b], None)
            d_rgb_arg = L.cotangents_arg(cot)
        gen = lib.cfnerf_model_stash_generation(net.handle)
        bwd = lib.cfnerf_render_bwd_accumulate if accumulate else lib.cfnerf_render_bwd
        L.check(bwd(net.handle, gen, d_rgb_arg, L.ptr(d_depth), L.ptr(d_ent) if self.beta1 and d_ent is not None else None,
                    L.ptr(grad), st), "cfnerf_render_bwd_accumulate" if accumulate else "cfnerf_render_bwd")
        if ray_grad:                            # the pass's ray blocks (per-launch quantities: the next pass overwrites them) -> the step's rows
            r_off, z_off, _ = L.ray_grad_offsets(net.n_params, n, S)
            self.d_rays[a:b] = self.gbuf[r_off:r_off + n * 11].view(n, 11)
            self.d_z[a:b] = self.gbuf[z_off:z_off + n * S].view(n, S)
            if reg:                             # + the regularisers' direct gradient in the depths (the path through the weights is in the block)
                self.d_z[a:b] += self._reg_dz[a:b]
        if latent_grad:                         # the pass's latent blocks (per-launch quantities too) -> the step's sum / the step's rows
            e_off, er_off, _ = L.eps_grad_offsets(L.ray_grad_offsets(net.n_params, n, S)[2] if ray_grad else net.n_params, n, K)
            if eps.dim() == 3:
                self._d_eps_acc[a:b] = self.gbuf[er_off:er_off + n * K * 4].view(n, K, 4)
            else:
                self._d_eps_acc += self.gbuf[e_off:e_off + K * 4].view(K, 4)

    def forward_backward(self, H, W, focal, rays, target, t_rand=None, eps=None, near=0., far=1., ndc=True,
                         lindisp=False, white_bkgd=False, perturb=1., t_vals=None, eps_chunks=None, depth_rays=None, target_depth=None,
                         occupancy=None, **_ignored):
        """Forward + loss + backward of this rank's shard.  Leaves the (un-reduced) gradient in ``self.grad``.

        ``depth_rays [2,N_d,3]`` / ``target_depth [N_d]`` (this rank's shard of the step's key-point rays, ``depth_lambda > 0``): the launch
        is the colour rays followed by the depth rays - ``t_rand`` / ``eps`` rows cover all ``N + N_d`` rays, the output buffers too -,
        the KDE-NLL runs on the colour rows, the depth term on the depth rows; ``self.depth_loss`` holds the rank's contribution to the
        step's ``depth_loss`` and ``self.scalars[0]`` includes ``depth_lambda`` times it.  The entropy term is the launch's (all rays);
        in netchunk mode on a batch of several network calls it is the FIRST call's alone, as in the reference (RUN:1024 cuts the
        per-point entropy tensor to its first N rows): that call is one launch, the rest a second one without an entropy cotangent.

        ``occupancy=`` an ``evaluate.OccupancySampler``: the depths of all the step's rays (depth rays included) are warped ONCE into the
        occupied part of every ray (``api.warp_z_vals`` on the plain depths of ``t_vals`` / ``t_rand`` / ``lindisp``; constants of the graph)
        and every pass is the explicit-depth launch on its rows of them - slices, depth rays, ``ray_grad``, both precisions and netchunk
        latents as without.  ``self.z_vals [N,S]`` and ``self.n_occ [N]`` are left for the caller.  Without it nothing changes."""
        net = self.net
        dev = net.flat.device
        t_vals = t_vals_table(dev) if t_vals is None else t_vals            # (cached per device)
        S = t_vals.shape[0]
        N, K = rays[1].reshape(-1, 3).shape[0], net.K_samples
        depth = self._check_depth(depth_rays, target_depth, N, S)
        first = None
        if depth is not None:
            depth_rays, target_depth, first = depth
            rays = tuple(torch.cat([_f32c(rays[i].reshape(-1, 3)), _f32c(depth_rays[i].reshape(-1, 3)).to(rays[i].device)], 0) for i in (0, 1))
            depth = (N, _f32c(target_depth).to(dev))                        # (colour rows, targets of the depth rows behind them)
            N += target_depth.shape[0]
            self.depth_loss.zero_()
        self._buffers(N, K)
        if depth is not None:
            self._depth_buffers(depth[0], N, K)
        _pack_rays(H, W, focal, rays=rays, ndc=ndc, near=near, far=far, out=self.packed)
        self._step_pairs = None
        if eps is None:
            if self.latent_draws == "netchunk" and eps_chunks is None and (self.world > 1 or self.force_allreduce):
                raise RuntimeError("netchunk latents of a sharded step come from Trainer.step (or pass eps_chunks=)")
            # the GLOBAL batch's latents; of rows this rank takes its own range (the union of the shards is the one-process batch).  As ever:
            # an implicit netchunk draw brings the CPU generator's t_rand, any other t_rand is drawn on the DEVICE below; no raw_noise_std
            tr, eps, pairs = LT.train_latents(self.latent_draws, None if eps_chunks is None else _f32c(eps_chunks), N=N * self.world, S=S, K=K,
                                              netchunk=self.netchunk, chunk=self.chunk, perturb=perturb)
            t_rand = tr if t_rand is None else t_rand
            self._step_pairs = pairs
            if pairs is not None:
                self.last_eps_chunks = pairs                                # (the step's pairs: identical on every rank)
                eps = eps[self.rank * N:(self.rank + 1) * N]
        t_rand = None if perturb <= 0. else _f32c(torch.rand(N, S, device=dev) if t_rand is None else t_rand).to(dev)
        eps = LT.to_device(_f32c(eps), dev)
        self._eps_rows = eps if eps.dim() == 3 else None
        z_vals = None
        if occupancy is not None:                                           # grid-guided sampling: the jitter went into the plain depths
            w = warp_z_vals(self.packed, occupancy, t_vals, t_rand, lindisp)
            self.z_vals, self.n_occ = w['z_vals'], w['n_occ']
            z_vals, t_rand = self.z_vals, None
        if self._reg:
            self._reg_buffers(N, S, K, z_vals, t_vals, t_rand, lindisp)
        net._sync()
        flags = L.F_TRAIN | (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0)
        n_sl = self.n_slices(N)
        target = _f32c(target)
        # the shard in n_sl equal slices: every loss term is taken with n_total = the FULL batch and beta1 / (world n_sl) on the slice's
        # entropy (equal slices: the mean of the slice means is the batch mean), so the slice gradients and the scalar contributions ADD.
        # One slice writes its scalars and entropy straight into the step's own buffers.
        if self.ray_grad:
            self._ray_grad_buffers(N, S, max(first, N - first) if first is not None else N // n_sl)
        if self.latent_grad:
            self._latent_grad_buffers(eps, S, max(first, N - first) if first is not None else N // n_sl)
        if first is not None:
            self._first_call_and_rest(first, N, t_vals, t_rand, eps, S, flags, target, depth, z_vals)
            if self.latent_grad:
                self._latent_grad_finish(N, S)
            return self.grad
        Ns = N // n_sl
        net.ensure_workspace(Ns, S, K)
        if n_sl == 1:
            sc, ent, d_ent = self.scalars, self.entropy, self.d_ent
        else:
            if getattr(self, "_sl_n", None) != n_sl:
                self._d_ent_sl = torch.tensor([self.beta1 / (self.world * n_sl)], device=dev)
                self._sc_sl, self._ent_sl = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
                self._sl_n = n_sl
            sc, ent, d_ent = self._sc_sl, self._ent_sl, self._d_ent_sl
            sc_sum, ent_sum = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
        for i in range(n_sl):
            self._pass(i * Ns, (i + 1) * Ns, t_vals, t_rand, eps, S, flags, target, self.beta1 / (self.world * n_sl), sc, ent, d_ent,
                       grad=self.grad, accumulate=i > 0, depth=depth, ray_grad=self.ray_grad, latent_grad=self.latent_grad, z_vals=z_vals)
            if n_sl > 1:
                sc_sum += sc
                ent_sum += ent
        if n_sl > 1:
            self.scalars[:3] = sc_sum[:3]
            self.scalars[3] = -10.0 * torch.log10(sc_sum[2])                # HLP:16 on the batch's mse
            self.entropy.copy_(ent_sum / n_sl)
        if self.latent_grad:
            self._latent_grad_finish(N, S)
        return self.grad

    def _first_call_and_rest(self, first, N, t_vals, t_rand, eps, S, flags, target, depth, z_vals=None):
        """Depth-supervised netchunk step on a batch of several network calls (one process): rows [0, first) - the first network call -
        with the entropy term ``beta1`` * (that call's entropy), rows [first, N) without one; the second launch's gradient is added
        to the first's and the colour rows' scalar contributions add like slices'."""
        dev = self.net.flat.device
        self.net.ensure_workspace(max(first, N - first), S, self.net.K_samples)
        sc, ent = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
        self._pass(0, first, t_vals, t_rand, eps, S, flags, target, self.beta1, self.scalars, self.entropy, self.d_ent, grad=self.grad,
                   depth=depth, ray_grad=self.ray_grad, latent_grad=self.latent_grad, z_vals=z_vals)
        self._pass(first, N, t_vals, t_rand, eps, S, flags, target, 0.0, sc, ent, None, grad=self.grad, accumulate=True, depth=depth,
                   ray_grad=self.ray_grad, latent_grad=self.latent_grad, z_vals=z_vals)
        sc[:3] += self.scalars[:3]
        self.scalars[:3] = sc[:3]
        self.scalars[3] = -10.0 * torch.log10(sc[2])                        # HLP:16 on the batch's mse
        return self.grad

    def n_slices(self, N):
        """Slices a shard of N rays is walked in: the fewest EQUAL ones of at most max_rays_per_launch rays (1 without a limit)."""
        if not self.max_rays or N <= self.max_rays:
            return 1
        n = -(-N // self.max_rays)
        while N % n:
            n += 1
        return n

    def _step(self, forward_backward, exchange, H, W, focal, rays, target, kw):
        """Body of step / step_hierarchical: the step's latents, forward + backward, the gradient exchange, Adam, re-pack."""
        dist_on = self.world > 1 or self.force_allreduce
        shape = (self.net.K_samples, 4)             # what the ranks exchange for the next step: one set, or the global batch's pairs
        if self.latent_draws == "netchunk":
            S = (kw.get("t_vals").shape[0] if kw.get("t_vals") is not None else t_vals_table().shape[0])
            n_depth = 0 if kw.get("depth_rays") is None else kw["depth_rays"][1].reshape(-1, 3).shape[0]
            shape = (LT.netchunk_count((rays[1].reshape(-1, 3).shape[0] + n_depth) * self.world, S, self.netchunk, self.chunk), *shape)
        if dist_on:
            tail = self._tail(shape)                                        # (grown BEFORE the backward writes the gradient view)
            if kw.get("eps") is None and kw.get("eps_chunks") is None:
                kw["eps_chunks" if len(shape) == 3 else "eps"] = self._step_eps(shape)
        forward_backward(H, W, focal, rays, target, **kw)
        if dist_on:
            # rank 0 writes the NEXT step's latents behind the gradient, everyone else zeros; after the sum every rank holds them
            tail.copy_(self._draw(shape).reshape(-1)) if self.rank == 0 else tail.zero_()
            self._timed_exchange(exchange)
            self._eps_next = tail.reshape(shape).clone()
        lr = lr_at(self.lrate, self.lrate_decay, self.start, self.t)
        self.t += 1
        net = self.net
        L.check(L.lib().cfnerf_adam_step(net.handle, L.ptr(net.flat.data), L.ptr(self.grad), L.ptr(self.exp_avg),
                                         L.ptr(self.exp_avg_sq), self.t, C.c_float(lr), C.c_float(1.0), L.stream()),
                "cfnerf_adam_step")
        net.mark_packed()
        net.params_serial += 1
        return self.scalars

    def step(self, H, W, focal, rays, target, **kw):
        """One full train step.  Returns the device tensor [loss, loss_nll, mse, psnr] of the local shard (``depth_rays=`` /
        ``target_depth=``: the depth-supervised step; ``occupancy=`` a sampler: sampling through an occupancy grid - see forward_backward)."""
        kw = {k: v for k, v in kw.items() if k in ("t_rand", "eps", "eps_chunks", "near", "far", "ndc", "lindisp", "white_bkgd", "perturb",
                                                     "t_vals", "depth_rays", "target_depth", "occupancy")}
        return self._step(self.forward_backward, self._exchange, H, W, focal, rays, target, kw)

    # ---- EXTENSION (not in the reference): coarse + fine sampling through the single network -----
    def forward_backward_hierarchical(self, H, W, focal, rays, target, N_samples=64, N_importance=128, coarse_loss=True, t_rand=None,
                                      u_fine=None, eps=None, near=0., far=1., ndc=True, lindisp=False, white_bkgd=False, perturb=1.,
                                      depth_rays=None, target_depth=None, **_ignored):
        """Coarse pass on ``linspace(0,1,N_samples)`` -> ``cfnerf_sample_pdf`` (depths are constants, as nerf-pytorch
        detaches ``z_samples``) -> fine pass on the merged N_samples + N_importance depths, loss and backward.  With
        ``coarse_loss`` the coarse pass keeps a stash and its own loss term is differentiated too
        (nerf-pytorch adds img2mse(rgb0); here the same KDE-NLL as the fine term), so ``self.grad`` is the gradient of
        loss_fine + loss_coarse.  Returns it; ``self.scalars`` holds the fine pass's [loss, nll, mse, psnr]."""
        if self.latent_draws == "netchunk":
            raise NotImplementedError("latent_draws='netchunk' is not supported by the hierarchical-sampling extension")
        if self.latent_grad:
            raise NotImplementedError("Trainer(latent_grad=True) is not supported by forward_backward_hierarchical / step_hierarchical: the latent "
                                      "blocks of CFNERF_F_EPS_GRAD are sized and collected by forward_backward / step alone (the fine pass under "
                                      "autograd, render_rays(hierarchical_extension=True), gives eps.grad)")
        if depth_rays is not None or target_depth is not None:
            raise NotImplementedError("depth rays are not supported by the hierarchical-sampling extension")
        if self._reg:
            raise NotImplementedError("Trainer(distortion_lambda= / ray_entropy_lambda=) is not supported by forward_backward_hierarchical / "
                                      "step_hierarchical: the ray regularisers run on the passes of forward_backward / step alone")
        if _ignored.get("occupancy") is not None:
            raise NotImplementedError("occupancy= (sampling through an occupancy grid) is not supported by forward_backward_hierarchical / "
                                      "step_hierarchical: both choose the depths of the pass; use step(occupancy=)")
        net = self.net
        dev = net.flat.device
        N, K, S, Ni = rays[1].reshape(-1, 3).shape[0], net.K_samples, int(N_samples), int(N_importance)
        self._buffers(N, K)
        _pack_rays(H, W, focal, rays=rays, ndc=ndc, near=near, far=far, out=self.packed)
        tv = torch.linspace(0., 1., steps=S).to(dev)
        if perturb > 0.:
            t_rand = _f32c(torch.rand(N, S, device=dev) if t_rand is None else t_rand)
            u = _f32c(torch.rand(N, Ni, device=dev) if u_fine is None else u_fine)
        else:
            t_rand = None
            u = _f32c(torch.linspace(0., 1., steps=Ni).expand(N, Ni).to(dev) if u_fine is None else u_fine)
        eps = _f32c(net.draw_eps() if eps is None else eps)
        net._sync()
        net.ensure_workspace(N, S + Ni, K)
        flags = (L.F_LINDISP if lindisp else 0) | (L.F_WHITE_BKGD if white_bkgd else 0) | L.F_TRAIN
        target = _f32c(target)
        loss = (target, self.beta1 / self.world, self.scalars, self.entropy, self.d_ent)
        # 1. coarse pass -> per-sample weights -> resampled depths.  With a coarse loss term the same launch also stashes its
        #    activations and its loss and backward follow at once (before the fine pass replaces the stash), so the coarse term
        #    costs one backward, not a second forward.
        w0 = torch.empty(N, S, K, device=dev)
        grad_c = torch.empty_like(self.grad) if coarse_loss else None
        self._pass(0, N, tv, t_rand, eps, S, flags, *loss, grad=grad_c, weights=w0)
        if coarse_loss:
            self.scalars_coarse = self.scalars.clone()
        z_all = torch.empty(N, S + Ni, device=dev)
        L.check(L.lib().cfnerf_sample_pdf(L.ptr(self.packed), L.ptr(tv), L.ptr(t_rand), flags, L.ptr(w0), L.ptr(u), N, S, K, Ni, L.ptr(z_all),
                                          L.stream()), "cfnerf_sample_pdf")
        # 2. fine pass on the merged depths, loss, backward
        self._pass(0, N, tv, None, eps, S + Ni, flags, *loss, grad=self.grad, z_vals=z_all)
        if grad_c is not None:
            self.grad.add_(grad_c)
        self.z_vals = z_all
        return self.grad

    def step_hierarchical(self, H, W, focal, rays, target, **kw):
        """One full train step of the coarse + fine EXTENSION (see forward_backward_hierarchical)."""
        if self.latent_draws == "netchunk":
            raise NotImplementedError("latent_draws='netchunk' is not supported by the hierarchical-sampling extension")
        if self.latent_grad:
            raise NotImplementedError("Trainer(latent_grad=True) is not supported by forward_backward_hierarchical / step_hierarchical "
                                      "(refused before the step draws or launches anything; see forward_backward_hierarchical)")
        if kw.get("occupancy") is not None:
            raise NotImplementedError("occupancy= (sampling through an occupancy grid) is not supported by step_hierarchical: both choose "
                                      "the depths of the pass; use step(occupancy=)")
        if self._reg:
            raise NotImplementedError("Trainer(distortion_lambda= / ray_entropy_lambda=) is not supported by step_hierarchical "
                                      "(refused before the step draws or launches anything; see forward_backward_hierarchical)")
        # always the plain one-bucket all-reduce: this gradient is grad_fine + grad_c, added by torch after the last backward, while
        # the early-range event that overlap_comm's first bucket waits for fires inside that backward, before the add
        return self._step(self.forward_backward_hierarchical, lambda: allreduce_sum_(self.gbuf, self.world, self.group, self.force_allreduce),
                          H, W, focal, rays, target, kw)

    @property
    def global_step(self):
        return self.start + self.t
