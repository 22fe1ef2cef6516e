#!/usr/bin/env python3
"""bench.py - headline benchmark of the MI355X-native CF-NeRF ray-batch hot path.

    python bench.py --gpus N --steps K --warmup W [--config C2|C3|C4|C5|C1|W512|K64] [--full] [--dump-outputs DIR]
    N > 1: one rank per GPU.  Either the driver starts the ranks (python -m torch.distributed.run --nproc-per-node N
    bench.py --gpus N ...: WORLD_SIZE is set) or - plain `python bench.py --gpus N` - this process, which has not touched
    the GPU, starts them itself as a child torch.distributed.run and relays rank 0's JSON line.

A "step" is one pass of the hot path over one batch of synthetic rays of a BASELINE.json config:
  C2  (default at EVERY N: the config the metric is quoted on)  N_rand 1024 per GPU, K 4, W 256, fern-shaped NDC rays - train
      step, rays sharded, ONE all-reduce of the flat gradient per step when N > 1
  C4  N_rand 1024 per GPU (8192 over 8), K 16 - train step (at N > 1 the default run reports it as `config4_k16` next to the line)
  C3  N_rand 4096, K 8, africa-like (no NDC, near 1.2 / far 8) - train step
  C5  800 x 800 full-image eval, K 32, white background, rows tiled across ranks, fused uncertainty maps - eval
  C1  N_rand 256, K 1 - forward only (the reference's K = 1 train loss is NaN)
  W512  the authors' recipe (train_NF.sh): W 512, h_alpha 64, K 32, N_rand 512 - train step ("stress row" of SURVEY 8d)
  K64   the reference's DEFAULT latent count (--K_samples 64, RUN:631): N_rand 1024, W 256 - train step
S = 128 samples always (the reference's hard-coded table; single pass - it has no fine network).
  --mode train: forward + KDE-NLL loss + backward + Adam;  --mode eval: fused forward render only.
A plain run sets up, warms up, times the K steps and prints the line; everything else it can measure or check (rocprofv3 counter
passes, per-stage kernel times, other precisions / configs, the eval and PSNR blocks, the CPU leg) runs only with --full.
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy, before anything else runs.
Rays are sharded across ranks (weak scaling: rays per GPU fixed); the only exchange is one RCCL all-reduce of the flat
gradient per train step.  Prints ONE JSON line on rank 0.  At N > 1 the line explains itself: `comm` (exposed exchange time
per step from two HIP events around the all-reduce on the compute stream, payload, the backend and world size torch.distributed
reports), `rank_skew` (min / max over ranks of the step and forward-kernel times) and, with --full, `psnr` (the sharded ray pool +
Trainer on the stand-in scene, with `vs_single_process`), `cpu_baseline` (rank 0).  Exit codes: 2 = fewer GPUs than --gpus, 3 = the process
group could not be initialised or does not span --gpus ranks.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

FP32_MFMA_PEAK_TF = 157.3          # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz
S, D = 128, 8

CONFIGS = {
    # name: rays per GPU, K, width, h_alpha, mode, scene
    "C1": dict(n=256, K=1, W=256, ha=32, mode="eval", scene="fern", what="LLFF-fern-shaped NDC rays, forward only (K=1)"),
    "C2": dict(n=1024, K=4, W=256, ha=32, mode="train", scene="fern", what="LLFF-fern-shaped NDC rays"),
    "C3": dict(n=4096, K=8, W=256, ha=32, mode="train", scene="africa", what="africa-like rays (no NDC, near 1.2 / far 8, 512x512, f=600)"),
    "C4": dict(n=1024, K=16, W=256, ha=32, mode="train", scene="fern", what="LLFF-fern-shaped NDC rays, 1024 rays per GPU (8192 over 8 GPUs)"),
    "C5": dict(n=None, K=32, W=256, ha=32, mode="eval", scene="blender", what="800x800 full-image eval (Blender intrinsics, near 2 / far 6, white background, "
                                                                               "no NDC), rows tiled across ranks, fused K-statistics (uncertainty maps)"),
    "W512": dict(n=512, K=32, W=512, ha=64, mode="train", scene="fern", what="the authors' recipe (train_NF.sh): W=512, h_alpha=64, K=32, N_rand=512"),
    "K64": dict(n=1024, K=64, W=256, ha=32, mode="train", scene="fern", what="LLFF-fern-shaped NDC rays at the reference's default K_samples=64 (RUN:631)"),
    "N8192": dict(n=8192, K=4, W=256, ha=32, mode="train", scene="fern", max_rays=1024,
                  what="C2's rays, 8192 per optimiser step walked in 8 slices of 1024 (Trainer(max_rays_per_launch=1024), cfnerf_render_bwd_accumulate): "
                       "the workspace of a 1024-ray step"),
}


def gemm_flops_per_point(W=256, ha=32, hr=64, ic=63, icv=27, F=4):
    """Algorithmic MACs per point (deduplicated flow heads) x 2."""
    macs = ic * W + 4 * W * W + (W + ic) * W + 2 * W * W          # trunk (D = 8: layers 0, 1-4, 5 (skip), 6-7)
    macs += W * ha + W * W + (W + icv) * (W // 2) + (W // 2) * hr  # h_alpha, feature, views, h_rgb
    macs += hr * 18 * F + ha * 3 * F                               # live flow-parameter heads
    return 2 * macs


def synth_rays(rng, n, H, Wd, focal):
    """n random pixels of a near-identity pose."""
    c2w = np.eye(4, dtype=np.float32)[:3]
    c2w[:, 3] = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    pix = rng.choice(H * Wd, size=n, replace=False)
    j, i = np.divmod(pix, Wd)
    dirs = np.stack([(i - Wd * .5) / focal, -(j - H * .5) / focal, -np.ones_like(i, dtype=np.float64)], -1)
    rays_d = (dirs[:, None, :] * c2w[:3, :3]).sum(-1).astype(np.float32)
    rays_o = np.broadcast_to(c2w[:3, 3], rays_d.shape).astype(np.float32)
    return torch.tensor(np.stack([rays_o, rays_d], 0))


def fern_rays(rng, n, H=378, W=504, focal=407.5658):
    return synth_rays(rng, n, H, W, focal), (H, W, focal)


SCENES = {
    "fern": dict(H=378, W=504, focal=407.5658, ndc=True, near=0., far=1., white_bkgd=False),
    "africa": dict(H=512, W=512, focal=600.0, ndc=False, near=1.2, far=8.0, white_bkgd=False),
    "blender": dict(H=800, W=800, focal=1111.1, ndc=False, near=2.0, far=6.0, white_bkgd=True),
}


def blender_pose(theta=30., phi=-30., radius=4.):
    """pose_spherical of the Blender loader (load_blender.py:29-34)."""
    t = np.eye(4); t[2, 3] = radius
    p = phi / 180. * np.pi
    rp = np.array([[1, 0, 0, 0], [0, np.cos(p), -np.sin(p), 0], [0, np.sin(p), np.cos(p), 0], [0, 0, 0, 1.]])
    th = theta / 180. * np.pi
    rt = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1.]])
    c2w = rt @ rp @ t
    c2w = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1.]]) @ c2w
    return torch.tensor(c2w[:3, :4], dtype=torch.float32)


def cpu_baseline(mode, cfg, budget_s=30.0):
    """The CPU oracle (op-for-op PyTorch-CPU restatement of the reference, oracle/) timed on this box's
    host cores on a bounded sample of the same workload.  The thread count is swept (all usable
    cores is NOT the fastest for these GEMM sizes) and the best setting is reported with its count."""
    from oracle import cfnerf_oracle as O      # oracle/ is used by the cpu_baseline leg only: timed here as the CPU baseline, and as the checker of psnr_oracle_agreement
    K, W = cfg["K"], cfg["W"]
    n_rays = min(cfg["n"] or 1024, 1024)        # bounded sample: at most 1024 rays of the per-GPU workload
    sc = SCENES[cfg["scene"]]
    ocfg = O.OracleCfg(netwidth=W, K_samples=K, h_alpha_size=cfg["ha"])
    p = O.make_params(ocfg, 0)
    rng = np.random.default_rng(5)
    rays = synth_rays(rng, n_rays, sc["H"], sc["W"], sc["focal"])
    packed = O.pack_rays(sc["H"], sc["W"], sc["focal"], rays[0], rays[1], sc["ndc"], sc["near"], sc["far"])
    t_rand = torch.rand(n_rays, S)
    ea, er = torch.randn(K, 1), torch.randn(K, 3)
    target = torch.rand(n_rays, 3)
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1

    def one():
        t0 = time.perf_counter()
        if mode == "train":
            scal, grads, _ = O.train_step(p, packed, target, ocfg, ea, er, t_rand, 0.01, white_bkgd=sc["white_bkgd"])
            O.adam_step({k: v.clone() for k, v in p.items()}, grads, {}, 1, 5e-4)
        else:
            with torch.no_grad():
                O.render_rays(p, packed, ocfg, ea, er, False, white_bkgd=sc["white_bkgd"])
        return time.perf_counter() - t0

    t_start = time.perf_counter()
    best, best_thr, tried = float("inf"), 1, []
    torch.set_num_threads(min(usable, 16))
    one()                                       # warm-up (thread pool, allocator, autograd graph caches)
    for thr in (16, 32, 8, 64):                 # more threads than 64 only thrash on these GEMM sizes
        if thr > usable or time.perf_counter() - t_start > budget_s:
            continue
        torch.set_num_threads(thr)
        dt = one()
        tried.append(thr)
        if dt < best:
            best, best_thr = dt, thr
    out = {"value": n_rays / best, "unit": "rays/s", "cores": best_thr, "kind": "port",
           "sample": f"{n_rays} rays x {S} samples x K={K}, W={W}: one {mode} step of the PyTorch-CPU oracle per thread count, best at "
                     f"{best_thr} threads (tried {tried}; {usable} usable cores; anomaly detection off)"}
    if mode == "train" and time.perf_counter() - t_start < budget_s:
        # the reference ships with torch.autograd.set_detect_anomaly(True) (HLP:2, MOD:5): one more step that way
        torch.set_num_threads(best_thr)
        with torch.autograd.set_detect_anomaly(True):
            out["value_anomaly_on"] = n_rays / one()
    return out


class Workload:
    """One config on this rank: model, synthetic inputs resident in HBM, step()."""

    def __init__(self, name, mode, rank, world, dev, precision="fp32", force_dist=False, hierarchical=0):
        import contextlib
        import cfnerf_amd
        from cfnerf_amd import _lib as L
        self.name, self.cfg = name, CONFIGS[name]
        cfg = self.cfg
        self.mode = mode or cfg["mode"]
        self.K, self.W, self.world, self.rank, self.dev = cfg["K"], cfg["W"], world, rank, dev
        sc = self.sc = SCENES[cfg["scene"]]
        torch.manual_seed(0)                    # same random-init weights on every rank (nn.Linear-style init of the product)
        with contextlib.redirect_stdout(sys.stderr):            # create_nerf prints the reference's "No reloading" notice
            kw_train, kw_test, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(
                netwidth=self.W, netdepth=D, K_samples=self.K, h_alpha_size=cfg["ha"], device=dev, no_ndc=not sc["ndc"],
                white_bkgd=sc["white_bkgd"], dataset_type="llff" if sc["ndc"] else "blender"))
        self.kw_train, self.kw_test = kw_train, kw_test
        self.net = kw_train["network_fn"].module
        self.lib = L.lib()
        # mode 2: HIP events around the fused forward launch only (2 per step).  Timing every stage (10 events) costs ~1 % of the
        # step, so the per-stage breakdown is taken in a few extra steps AFTER the timed region (stage_ms)
        self.lib.cfnerf_timing_enable(self.net.handle, 2)
        self.net.set_precision(precision)
        if os.environ.get("CFNERF_BENCH_FLOW_MATH"):            # development A/B only: auto (default) | libm | fast
            self.net.set_flow_math(os.environ["CFNERF_BENCH_FLOW_MATH"])
        self.cfnerf = cfnerf_amd
        self.g = torch.Generator(device=dev).manual_seed(1234)  # explicit latents: same on every rank (Trainer enforces it otherwise)
        H, Wd, focal = sc["H"], sc["W"], sc["focal"]
        if name == "C5":
            from cfnerf_amd import evaluate as EV
            self.EV = EV
            self.c2w = blender_pose()
            self.r0, self.r1 = EV.row_shard(H, rank, world)
            self.n = (self.r1 - self.r0) * Wd
        else:
            self.n = cfg["n"]
            rng = np.random.default_rng(1000 + rank)
            self.rays = synth_rays(rng, self.n, H, Wd, focal).to(dev)
            self.target = torch.tensor(rng.uniform(0, 1, (self.n, 3)), dtype=torch.float32).to(dev)
        if self.mode == "train":
            from cfnerf_amd import train as T
            self.trainer = T.Trainer(self.net, lrate=5e-4, lrate_decay=250, beta1=0.01, world_size=world, force_allreduce=force_dist,
                                     overlap_comm=os.environ.get("CFNERF_BENCH_OVERLAP", "0") == "1", time_comm=world > 1 or force_dist,
                                     max_rays_per_launch=cfg.get("max_rays"))
        self.hier = hierarchical

    def step(self):
        sc, dev = self.sc, self.dev
        H, Wd, focal = sc["H"], sc["W"], sc["focal"]
        if self.name == "C5":
            with torch.no_grad():
                return self.EV.render_uncertainty(H, Wd, focal, self.c2w, self.net, near=sc["near"], far=sc["far"], ndc=False,
                                                  white_bkgd=True, rows=(self.r0, self.r1))
        if self.mode == "train":
            t_rand = torch.rand(self.n, S, device=dev)
            eps = torch.randn(self.K, 4, device=dev, generator=self.g)
            return self.trainer.step(H, Wd, focal, self.rays, self.target, t_rand=t_rand, eps=eps, near=sc["near"], far=sc["far"],
                                     ndc=sc["ndc"], white_bkgd=sc["white_bkgd"])
        with torch.no_grad():
            return self.cfnerf.render(H, Wd, focal, rays=self.rays, near=sc["near"], far=sc["far"], **self.kw_test)

    def fwd_mean_ms(self, n):
        """mean duration of the last n fused-forward launches (HIP events on the launch stream, recorded inside the timed region)"""
        return float(self.lib.cfnerf_timing_fwd_mean_ms(self.net.handle, int(n)))

    def kernel_ms(self, sync, extra_steps=3):
        """per-stage durations of one step: a few extra steps with every stage timed (outside the timed region)"""
        h = self.net.handle
        self.lib.cfnerf_timing_enable(h, 1)
        for _ in range(extra_steps):
            self.step()
        sync()
        names = (("fwd", 0),) + ((("bwd_tail", 1), ("bwd_data", 2), ("bwd_dw", 3), ("adam", 4)) if self.mode == "train" else ())
        out = {k: self.lib.cfnerf_timing_last_ms(h, i) for k, i in names}
        self.lib.cfnerf_timing_enable(h, 2)
        return out

    def describe(self, precision):
        c = self.cfg
        n = f"N_rand={self.n}/GPU" if self.name != "C5" else f"{self.n} rays/GPU (rows {self.r0}..{self.r1} of 800)"
        return (f"{self.name}: {c['what']}; {n}, S={S} (reference table, single pass), K={self.K}, W={self.W}, D={D}, h_alpha={c['ha']}, "
                f"mode={self.mode}, precision={precision}")

    def launches_per_step(self):
        return -(-self.n // (self.cfg.get("max_rays") or self.n))

    def fwd_flops(self):
        return gemm_flops_per_point(self.W, self.cfg["ha"]) * min(self.n, self.cfg.get("max_rays") or self.n) * S       # per LAUNCH (a slice of the step)


def timed(wl, steps, warmup, sync, per_step=None):
    """W untimed steps, then exactly K steps between two (barrier + device sync) points.  `per_step` (a list) receives the
    K step durations in ms from one HIP event per step on the launch stream (no host sync inside the region).  What the last
    step returned is kept in `wl.last`."""
    for _ in range(warmup):
        wl.step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] if per_step is not None else None
    sync()
    t0 = time.perf_counter()
    if ev:
        ev[0].record()
    for i in range(steps):
        wl.last = wl.step()
        if ev:
            ev[i + 1].record()
    sync()
    dt = time.perf_counter() - t0
    if ev:
        per_step.extend(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    return dt


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(wl, out_dir):
    """--dump-outputs: what the timed path handed its caller in its LAST step, one DIR/<name>.npy per array (float32 / float64), so that
    two builds run with the same arguments (same seeded inputs) can be compared output for output.  A train step returns the
    scalars [loss, loss_nll, mse, psnr] and leaves the updated parameters, their gradient and the forward's per-latent maps in place;
    an eval step returns the maps (C5: the fused K-statistics of the image rows)."""
    ret = wl.last
    if isinstance(ret, dict):
        arrays = dict(ret)
    elif wl.mode == "train":
        tr = wl.trainer
        arrays = {"scalars": ret, "params": wl.net.flat, "grad": tr.grad, "rgb_map": tr.rgb_map, "disp_map": tr.disp,
                  "depth_map": tr.depth, "entropy": tr.entropy}
    else:
        rgb, disp, depth, extras = ret
        arrays = {"rgb_map": rgb, "disp_map": disp, "depth_map": depth, **extras}
    arrays = {k: v.detach().cpu().numpy() for k, v in arrays.items() if torch.is_tensor(v)}
    arrays = {k: v if v.dtype == np.float64 else v.astype(np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs: {total} bytes of outputs exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: THIS process has only imported torch (no GPU call), so it may start
    the N ranks as a child `python -m torch.distributed.run` (the driver's own launch line), relay rank 0's JSON line as
    the last line of stdout and return the child's exit code."""
    import socket
    import subprocess
    same_gpu = os.environ.get("CFNERF_BENCH_SAME_GPU") == "1"
    # count devices WITHOUT initialising HIP in this process (it is about to fork + exec the launcher): the amdsmi path only; a negative
    # answer means "unknown" (torch.cuda.device_count() would then fall back to hipGetDeviceCount) - the ranks report a missing device
    try:
        have = int(torch.cuda._device_count_amdsmi())
    except Exception:
        have = -1
    if not same_gpu and 0 <= have < n:         # (negative = amdsmi could not tell: let the ranks find out)
        print(f"bench.py: --gpus {n} but only {have} GPU(s) visible (CFNERF_BENCH_SAME_GPU=1 runs the N-rank code path on one GPU over gloo)",
              file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    lines = r.stdout.splitlines()
    js = [i for i, l in enumerate(lines) if l.startswith("{") and '"metric"' in l]
    for i, l in enumerate(lines):
        if not js or i != js[-1]:
            print(l, file=sys.stderr)
    if r.returncode != 0 or not js:
        print(f"bench.py: the {n}-rank run failed (exit code {r.returncode}, JSON line {'found' if js else 'missing'})", file=sys.stderr)
        return r.returncode or 1
    print(lines[js[-1]], flush=True)
    return 0


def live_pmc(mode, budget_s=150.0):
    """HBM traffic and matrix-pipe occupancy of the fused forward kernel OBSERVED BY THIS RUN: before this process touches the GPU it
    runs the same workload (3 steps) as a CHILD under `rocprofv3 --kernel-trace --pmc ...`, one pass per counter group (FETCH_SIZE;
    WRITE_SIZE; SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE - counters in their own passes, no other trace domain, the program itself
    after `--`), and reads the per-dispatch means of the kernel from the counter CSV.  Corrections as MI355X_MICROARCH.md prescribes
    (FETCH_SIZE / WRITE_SIZE are KB; gfx950 reports half of a wide coalesced read: FETCH doubled).  Returns None - and the line falls
    back to the committed profiles/ figures, saying so - when rocprofv3 is absent, a pass fails or the time budget runs out."""
    import csv
    import glob
    import shutil
    import signal
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    # under a profiler this process may already hold the GPU (its preloaded tool library initialises it): starting children is off limits
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any(k.upper().startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    t_end = time.monotonic() + budget_s
    env = dict(os.environ, CFNERF_BENCH_LIVE_PMC="0", TMPDIR="/tmp")
    got = {}
    for group in (("FETCH_SIZE",), ("WRITE_SIZE",), ("SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE")):
        left = t_end - time.monotonic()
        if left < 25:
            return None
        with tempfile.TemporaryDirectory(prefix="cfnerf_pmc_", dir="/tmp") as d:
            cmd = [exe, "--kernel-trace", "--pmc", *group, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable,
                   os.path.abspath(__file__), "--steps", "3", "--warmup", "1", "--no-alt", "--no-cpu-baseline", "--mode", mode]
            try:
                proc = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            except OSError:
                return None
            try:
                proc.wait(timeout=min(left, 90.0))
            except subprocess.TimeoutExpired:
                try:
                    os.killpg(proc.pid, signal.SIGKILL)          # exactly the process group started above
                except OSError:
                    pass
                proc.wait()
                return None
            if proc.returncode != 0:
                return None
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                return None
            acc = {}
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    if "fused_fwd_kernel" in r["Kernel_Name"]:
                        acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
            for c in group:
                if not acc.get(c):
                    return None
                got[c] = sum(acc[c]) / len(acc[c])
    return {"hbm_bytes_per_launch": (2.0 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024.0,
            "FETCH_SIZE_KB": got["FETCH_SIZE"], "WRITE_SIZE_KB": got["WRITE_SIZE"],
            "mfma_busy_frac": got["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * got["GRBM_GUI_ACTIVE"] / 8.0)}


PSNR_NOTE = ("the end value of this chaotic trajectory re-rolls by a few dB with any change of arithmetic (35.1 / 36.3 / 38.2 dB at 2000 steps over "
             "round 3's builds, same seeds): it shows that the path trains; the PINS are vs_reference_run (the real reference's own run, fixture "
             "G19), vs_oracle and - at N > 1 - vs_single_process")


def _psnr_net(dev, K):
    import contextlib
    import cfnerf_amd
    torch.manual_seed(0)                        # the reference constructor's RNG stream is replayed on the CPU: same weights on every rank
    with contextlib.redirect_stdout(sys.stderr):
        kw_train, _, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(netwidth=256, K_samples=K, device=dev, no_ndc=True,
                                                                             dataset_type="blender"))
    return kw_train["network_fn"].module


def psnr_block(dev, steps, n_rand=1024, K=4, rank=0, world=1):
    """PSNR half of the headline metric (RUN:1027-1029: mse2psnr(img2mse(mean_K rgb, target))).  No LLFF-fern data exists
    here, so the scene is the procedural stand-in of tools/procedural_scene.py, trained through the device ray pool +
    the fused Trainer; held-out PSNR of the K-mean prediction at a few checkpoints.  N > 1: the pool is SHARDED (one permutation for
    all ranks, rank r takes its N_rand rows of the step's world x N_rand window), the global batch is world x n_rand rays, the Trainer
    all-reduces the gradient and enforces one set of latents per step; rank 0 evaluates."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import procedural_scene as PS
    import cfnerf_amd
    from cfnerf_amd import train as T
    poses, images, i_train, i_test = PS.make(dev)
    net = _psnr_net(dev, K)
    if world == 1:
        pool = cfnerf_amd.RayPool(images, poses, PS.H, PS.W, PS.FOCAL, i_train, n_rand, generator=torch.Generator(device=dev).manual_seed(1))
    else:
        pool = cfnerf_amd.RayPool(images, poses, PS.H, PS.W, PS.FOCAL, i_train, n_rand, rank=rank, world=world,
                                  generator=torch.Generator(device=dev).manual_seed(1))      # sync="auto": rank 0's permutation, broadcast per epoch
    tr = T.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01, world_size=world)
    g = torch.Generator(device=dev).manual_seed(2 + rank)                                    # jitter: independent per ray
    marks = sorted({0, min(250, steps), min(1000, steps), steps})
    curve = {0: PS.held_out_psnr(net, poses, images, i_test, dev)} if rank == 0 else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, steps + 1):
        rays, target = pool.next_batch()
        n = rays.shape[1]
        # one rank: explicit latents from the seeded generator (as rounds 1-3); several: the Trainer's own mechanism (rank 0 draws,
        # the latents of step t + 1 ride in the tail of step t's gradient all-reduce)
        eps = torch.randn(K, 4, device=dev, generator=g) if world == 1 else None
        sc = tr.step(PS.H, PS.W, PS.FOCAL, rays, target.contiguous(), t_rand=torch.rand(n, S, device=dev, generator=g), eps=eps,
                     near=PS.NEAR, far=PS.FAR, ndc=False)
        if it in marks and rank == 0:
            curve[it] = PS.held_out_psnr(net, poses, images, i_test, dev)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = None
    if rank == 0:
        out = {"scene": PS.LABEL, "what": "held-out PSNR of the K-mean prediction, mse2psnr(img2mse(mean_K rgb_map, target)) as RUN:1027-1029",
               "views": f"{len(i_train)} train / {len(i_test)} held out, {PS.H}x{PS.W}", "N_rand": n_rand, "n_gpus": world,
               "global_batch": n_rand * world, "K": K, "W": 256, "steps": steps, "epochs_crossed": pool.epoch,
               "feeder": "RayPool" + (f"(rank, world={world}): one permutation per epoch for all ranks ({pool.sync}), rank r takes rows "
                                      f"[i + r N_rand, i + (r+1) N_rand) of the step's window" if world > 1 else ""),
               "held_out_psnr_db_by_step": {str(k): round(v, 3) for k, v in curve.items()}, "value": round(curve[steps], 3), "unit": "dB",
               "train_batch_psnr_db_last_step": round(float(sc[3]), 3), "wall_s_incl_eval": round(wall, 2),
               "lrate": 5e-4, "lrate_decay": 250, "beta1": 0.01, "precision": "fp32", "note": PSNR_NOTE}
    net.release_workspace()
    return out


def psnr_vs_single_process(dev, rank, world, barrier, steps=25, n_rand=1024, K=4, tol_db=0.05):
    """Pass/fail at N > 1: the N-rank run (sharded pool, gradient all-reduce) reproduces ONE process training the same global batches -
    same initial weights, same permutation (seed form of the pool), the same jitter row for every ray and the same latents every step;
    their held-out PSNR after `steps` steps must agree within `tol_db` (what differs is the summation order of the gradient)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import procedural_scene as PS
    import cfnerf_amd
    from cfnerf_amd import train as T
    poses, images, i_train, i_test = PS.make(dev)

    def run(r, w, nr):
        net = _psnr_net(dev, K)
        pool = cfnerf_amd.RayPool(images, poses, PS.H, PS.W, PS.FOCAL, i_train, nr, rank=r, world=w, seed=11, sync="seed")
        tr = T.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01, world_size=w)
        gj, ge = torch.Generator().manual_seed(12), torch.Generator().manual_seed(13)
        for _ in range(steps):
            rays, target = pool.next_batch()
            n = rays.shape[1]
            t_all = torch.rand(n * w, S, generator=gj)              # jitter of the GLOBAL batch; a rank keeps its rows
            eps = torch.randn(K, 4, generator=ge)
            tr.step(PS.H, PS.W, PS.FOCAL, rays, target.contiguous(), t_rand=t_all[r * n:(r + 1) * n].to(dev), eps=eps.to(dev),
                    near=PS.NEAR, far=PS.FAR, ndc=False)
        ps = PS.held_out_psnr(net, poses, images, i_test, dev) if r == 0 else None
        flat = net.flat.detach().clone()
        net.release_workspace()
        return ps, flat, pool.epoch

    p_multi, flat_multi, ep = run(rank, world, n_rand)
    out = None
    if rank == 0:
        p_single, flat_single, _ = run(0, 1, n_rand * world)
        dw = float((flat_multi - flat_single).abs().max() / flat_single.abs().max())
        out = {"what": f"{world}-rank run (sharded RayPool, gradient all-reduce) vs ONE process on the same global batches of {n_rand * world} rays: "
                       f"same weights / permutation / jitter / latents for {steps} steps; held-out PSNR of both",
               "psnr_db_ranks": p_multi, "psnr_db_single_process": p_single, "abs_psnr_diff_db": abs(p_multi - p_single),
               "max_abs_param_diff_rel": dw, "epochs_crossed": ep, "tolerance_db": tol_db, "agree": bool(abs(p_multi - p_single) <= tol_db)}
    barrier()                                   # the other ranks wait here while rank 0 trains the one-process run
    return out


def psnr_reference_run_agreement():
    """Pass/fail against the REFERENCE ITSELF: fixture tests/golden/g19_psnr_curve.npz is the real reference trained in the build
    container for 120 steps with its own loop lines (RUN:1013-1077) on a tiny procedural scene (data only: scene, seeds, its loss /
    PSNR curves).  The HIP path re-runs those 120 steps with the same weights, batches, jitter and latents; its per-step loss,
    train-batch PSNR and held-out K-mean PSNR (steps 0 / 40 / 80 / 120) must stay inside the bounds of the -m gpu test
    (tests/g19_common.py).  Part of the cpu_baseline leg (the weights come from the oracle's deterministic generator)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import contextlib
    import numpy as np
    import g19_common as GC
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g19_psnr_curve.npz")))
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(sys.stderr):
        dl, dp, held = GC.hip_curve(g)
    ok = all(dl[a:b].max() <= tl and dp[a:b].max() <= tp for a, b, tl, tp in GC.CURVE_BOUNDS) and \
        all(float(np.abs(held[k]).max()) <= tol for k, tol in GC.HELD_OUT_BOUNDS.items())
    last = int(g["n_steps"])
    return {"what": "HIP path vs the real reference's own 120-step training run (fixture G19: its loop lines RUN:1013-1077, N_rand 128, K 4, "
                    "W 64, procedural 24x32 scene), same weights / batches / jitter / latents",
            "reference_held_out_psnr_db": {str(int(s)): round(float(np.mean(v)), 3) for s, v in zip(g["test_steps"], g["psnr_test"])},
            "max_abs_held_out_psnr_diff_db": {str(k): float(np.abs(v).max()) for k, v in held.items()},
            "max_abs_train_psnr_diff_db": float(dp.max()), "max_rel_loss_diff": float(dl.max()),
            "tolerance_db_at_last_step": GC.HELD_OUT_BOUNDS[last], "agree": bool(ok), "seconds": round(time.perf_counter() - t0, 2)}


def psnr_oracle_agreement(dev, steps=25, n_rand=256, K=4, tol_db=0.05):
    """Pass/fail: the HIP path and the CPU oracle train on the procedural scene from IDENTICAL weights with identical rays,
    targets, jitter and latents every step; their held-out PSNR must agree at step 0 and after `steps` steps (studied over 300
    steps in tests/tools/psnr_curve_vs_oracle.py: 1e-5 dB at step 0, 5e-6 at 25, then fp32 chaos separates any two runs).
    Part of the cpu_baseline leg: the oracle is the checker here, nothing it computes is reported as performance."""
    import contextlib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import procedural_scene as PS
    import cfnerf_amd
    from cfnerf_amd import train as T
    from oracle import cfnerf_oracle as O
    poses, images, i_train, i_test = PS.make(dev)
    view = i_test[1]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        kw_train, kw_test, _, _, _ = cfnerf_amd.create_nerf(cfnerf_amd.default_args(netwidth=256, K_samples=K, device=dev, no_ndc=True,
                                                                                   dataset_type="blender"))
    net = kw_train["network_fn"].module
    cfg = O.OracleCfg(netwidth=256, K_samples=K)
    shapes = O.param_shapes(cfg)
    sd = net.state_dict()
    p = {k: sd[k].detach().cpu().clone().reshape(shapes[k]) for k in shapes}
    ev = net.eval_eps().cpu()
    ea_eval, er_eval = ev[:, 3:4].clone(), ev[:, 0:3].clone()

    def psnr_hip():
        return PS.held_out_psnr(net, poses, images, [view], dev)

    def psnr_oracle():
        with torch.no_grad():
            out = O.render(p, PS.H, PS.W, PS.FOCAL, cfg, ea_eval, er_eval, False, c2w=poses[view], ndc=False, near=PS.NEAR, far=PS.FAR)
        return float(-10 * torch.log10(torch.mean((out["rgb_map"].mean(-1) - images[view]) ** 2)))

    ro_all, rd_all, tg_all = [], [], []
    for v in i_train:
        ro, rd = PS.camera_rays(poses[v], dev)
        ro_all.append(ro.cpu()); rd_all.append(rd.cpu()); tg_all.append(images[v].reshape(-1, 3))
    ro_all, rd_all, tg_all = torch.cat(ro_all), torch.cat(rd_all), torch.cat(tg_all)
    tr = T.Trainer(net, lrate=5e-4, lrate_decay=250, beta1=0.01)
    g = torch.Generator().manual_seed(3)
    state = {}
    d0 = abs(psnr_hip() - psnr_oracle())
    t_cpu = 0.0
    for it in range(1, steps + 1):
        sel = torch.randint(0, ro_all.shape[0], (n_rand,), generator=g)
        ro, rd, tg = ro_all[sel], rd_all[sel], tg_all[sel]
        t_rand = torch.rand(n_rand, S, generator=g)
        eps = torch.randn(K, 4, generator=g)
        tr.step(PS.H, PS.W, PS.FOCAL, (ro.to(dev), rd.to(dev)), tg.to(dev).contiguous(), t_rand=t_rand.to(dev), eps=eps.to(dev),
                near=PS.NEAR, far=PS.FAR, ndc=False)
        t0 = time.perf_counter()
        packed = O.pack_rays(PS.H, PS.W, PS.FOCAL, ro, rd, False, PS.NEAR, PS.FAR)
        _, grads, _ = O.train_step(p, packed, tg, cfg, eps[:, 3:4], eps[:, 0:3], t_rand, 0.01)
        p = O.adam_step(p, grads, state, it, O.lr_schedule(5e-4, 250, it - 1))
        t_cpu += time.perf_counter() - t0
    ph, po = psnr_hip(), psnr_oracle()
    net.release_workspace()
    return {"what": f"HIP path vs CPU oracle, same weights / rays / jitter / latents for {steps} steps of N_rand={n_rand} on the procedural scene",
            "abs_psnr_diff_db_step0": d0, f"abs_psnr_diff_db_step{steps}": abs(ph - po), "hip_psnr_db": ph, "oracle_psnr_db": po,
            "tolerance_db": tol_db, "agree": bool(d0 <= tol_db and abs(ph - po) <= tol_db), "oracle_cpu_s_per_step": round(t_cpu / steps, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None, help="default: C2 (1024 rays per GPU, K=4) at every GPU count")
    ap.add_argument("--mode", choices=["train", "eval"], default=None)
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline figure: the rocprofv3 counter "
                                                        "passes, per-stage kernel times, the extra measurements (see --no-alt) and the CPU leg "
                                                        "(see --no-cpu-baseline).  Off: set up, warm up, time the steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (rank 0; same arguments = same inputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the PSNR agreement checks")
    ap.add_argument("--no-alt", action="store_true", help="with --full: skip the extra measurements reported next to the main line (bf16x3, "
                                                          "W512 stress row, sliced batch, eval block, PSNR block, coarse+fine extension, "
                                                          "config 4 at N > 1)")
    ap.add_argument("--precision", choices=["fp32", "bf16x3"], default="fp32",
                    help="fp32 = exact-fp32 MFMA (default, the measured parity path); bf16x3 = opt-in split-bf16 MFMA mode")
    ap.add_argument("--psnr-steps", type=int, default=2000, help="train steps of the PSNR block (procedural stand-in scene)")
    ap.add_argument("--extension", action="store_true", help="also time the coarse + fine sampling EXTENSION (`alt_config`; not in the reference, "
                                                             "parity unpinned - off by default since round 5: the default line carries `eval` instead)")
    args = ap.parse_args()
    alt_on = args.full and not args.no_alt

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher above us: start the ranks ourselves (nothing in this process has touched the GPU yet)
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))

    # counters of the dominant kernel observed by this very run (--full one-GPU C2 line only; child passes BEFORE the first GPU call here)
    live = None
    if (args.gpus == 1 and "WORLD_SIZE" not in os.environ and alt_on and args.config is None and args.precision == "fp32"
            and os.environ.get("CFNERF_BENCH_LIVE_PMC", "1") != "0"):
        live = live_pmc(args.mode or "train")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node must equal --gpus")
    # CFNERF_BENCH_SAME_GPU=1 (testing the N > 1 code path on a one-GPU box): every rank uses cuda:0 and the ranks talk over gloo
    same_gpu = os.environ.get("CFNERF_BENCH_SAME_GPU") == "1"
    dev_index = 0 if same_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    force_dist = os.environ.get("CFNERF_BENCH_FORCE_DIST") == "1"      # exercise the RCCL path on one GPU (tests)
    dist = None
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if force_dist and "RANK" not in os.environ:
            os.environ.update(RANK="0", WORLD_SIZE="1")
        # a run that cannot be what --gpus asked for ends HERE with one line and a non-zero code, not with a number for fewer GPUs
        backend = "gloo" if same_gpu else "nccl"
        try:
            if same_gpu:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=dev)
        except Exception as e:
            print(f"bench.py: rank {rank}: init_process_group({backend!r}) failed: {type(e).__name__}: {str(e).splitlines()[0] if str(e) else ''}",
                  file=sys.stderr, flush=True)
            raise SystemExit(3)
        if dist.get_world_size() != (args.gpus if world > 1 else 1):
            print(f"bench.py: rank {rank}: the {backend} group spans {dist.get_world_size()} rank(s), --gpus asked for {args.gpus}", file=sys.stderr, flush=True)
            raise SystemExit(3)

    from cfnerf_amd import train as T
    if not T.backward_available():
        raise SystemExit("the backward kernels are not built")
    name = args.config or "C2"                 # the SAME workload per GPU at every N: the driver's scaling efficiency compares like with like
    wl = Workload(name, args.mode, rank, world, dev, args.precision, force_dist)
    mode = wl.mode

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(dt):
        if dist is None:
            return dt
        t = torch.tensor([dt], device="cpu" if same_gpu else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    step_ms = []
    dt_own = timed(wl, args.steps, args.warmup, sync, step_ms)
    if args.dump_outputs and rank == 0:
        dump_outputs(wl, args.dump_outputs)      # before anything below steps the model again
    dt = max_over_ranks(dt_own)
    # duration of the dominant kernel: mean over the launches of the timed region, HIP events on the launch stream
    fwd_ms = wl.fwd_mean_ms(args.steps)
    # N > 1: what the exchange exposed on the compute stream during the timed steps (this rank), then ONE more all-reduce (MAX of
    # [x, -x] pairs) for the spread over the ranks of the step time, the forward kernel and the exposed exchange
    comm, skew = None, None
    if dist is not None and mode == "train" and name != "C5":
        comm = wl.trainer.comm_stats(args.steps)
        own = [dt_own / args.steps * 1e3, fwd_ms, comm.get("exposed_ms_mean", 0.0), comm.get("exposed_ms_max", 0.0)]
        t = torch.tensor([v for x in own for v in (x, -x)], device="cpu" if same_gpu else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        t = t.tolist()
        skew = {"ms_per_step_max": t[0], "ms_per_step_min": -t[1], "fwd_launch_ms_max": t[2], "fwd_launch_ms_min": -t[3],
                "what": "over the ranks: each rank's own wall time per step of the timed region (between the same two barriers) and its mean "
                        "fused-forward launch duration"}
        comm.update(exposed_ms_mean_max_over_ranks=t[4], exposed_ms_mean_min_over_ranks=-t[5], exposed_ms_max_over_ranks=t[6],
                    what="gradient exchange of one train step (flat gradient + 4 K_max latents tail): time between two HIP events recorded on the "
                         "compute stream right before and right after Trainer._exchange, i.e. what the exchange EXPOSES there (the compute "
                         "stream waits for the collective); rank 0's mean / max / min over the timed steps, then the spread of the means over ranks",
                    frac_of_step=comm.get("exposed_ms_mean", 0.0) / (dt / args.steps * 1e3),
                    overlap_comm_pays_if="exposed_ms_mean > ~0.15 ms: the two-bucket form costs ~0.13 ms of gathers / scatters / a second "
                                         "launch per step (measured on one GPU) and can hide at most the early bucket's ~3/4 of the payload "
                                         "under the last ~0.2 ms of the backward (CFNERF_BENCH_OVERLAP=1 measures it)")
    kms = wl.kernel_ms(sync) if args.full else None
    extras = world == 1 and alt_on and name == "C2" and args.precision == "fp32" and mode == "train"

    # the opt-in split-bf16 mode, measured the same way right after (every rank runs it: the all-reduce is inside)
    alt = None
    if args.precision == "fp32" and alt_on and name != "C5":
        wl.net.set_precision("bf16x3")
        dta = max_over_ranks(timed(wl, args.steps, min(3, args.warmup) or 1, sync))
        alt_fwd_ms = wl.fwd_mean_ms(args.steps)
        wl.net.set_precision("fp32")
        alt = {"precision": "bf16x3 (opt-in): fp32 operands carried as hi+lo bf16, product = hi*hi + hi*lo + lo*hi on "
                            "v_mfma_f32_32x32x16_bf16, fp32 accumulate; forward, backward-data and the large weight-gradient GEMMs; "
                            "held to the same parity tolerances (tests/test_hip_bf16x3.py)",
               "value": wl.n * world * args.steps / dta, "unit": "rays/s", "ms_per_step": dta / args.steps * 1e3,
               "fwd_launch_ms": alt_fwd_ms, "fwd_fp32_equiv_tflops": wl.fwd_flops() / (alt_fwd_ms * 1e-3) / 1e12}
        # its own roofline: three bf16 MFMAs per fp32 product on the 2.5 PFLOP/s dense bf16 matrix pipe
        alt["roofline"] = {"bound": "mfma (bf16 pipe, 3 MFMAs per fp32 product)", "peak": 2500.0 / 3, "unit": "fp32-equivalent TFLOP/s",
                           "achieved": alt["fwd_fp32_equiv_tflops"], "frac": alt["fwd_fp32_equiv_tflops"] / (2500.0 / 3),
                           "note": "PMC (train forward, per tile and wave): 1 809 MFMAs = 38 % of the time, 7 970 other vector instructions "
                                   "(hi/lo split of every epilogue element, mask bits, flows) = 23 % - the bf16 MFMA does not co-issue with them "
                                   "either - and 38 % stalls at the 2.07 GHz this kernel clocks; costed in round 3: a free activation stash "
                                   "would give 0.40, the remaining candidates sum to 0.42-0.45 (profiles/r03_pmc_summary.txt section pmc_b16, "
                                   "profiles/EXPERIMENTS.md, round 3)"}

    # BASELINE config 4 (K = 16, 1024 rays per GPU) next to the line when the job spans several GPUs (--full default-config run only)
    cfg4 = None
    if world > 1 and alt_on and args.config is None and args.precision == "fp32" and mode == "train":
        wl.__dict__.pop("trainer", None)
        wl.net.release_workspace()
        w4 = Workload("C4", "train", rank, world, dev, "fp32", force_dist)
        s4 = max(5, min(20, args.steps))
        dt4 = max_over_ranks(timed(w4, s4, 3, sync))
        f4 = w4.fwd_mean_ms(s4)
        cfg4 = {"workload": w4.describe("fp32"), "value": w4.n * world * s4 / dt4, "unit": "rays/s", "ms_per_step": dt4 / s4 * 1e3, "steps": s4,
                "fwd_launch_ms": f4, "step_frac_of_peak": 3 * w4.fwd_flops() / (dt4 / s4) / 1e12 / FP32_MFMA_PEAK_TF}
        w4.net.release_workspace()
        del w4

    # SURVEY 8d "stress row": the authors' own recipe, next to the headline line (one GPU, --full default train run only)
    stress = None
    if extras:
        wl.__dict__.pop("trainer", None)
        wl.net.release_workspace()
        ws = Workload("W512", "train", rank, world, dev, "fp32", False)
        st_steps = max(5, min(20, args.steps))
        dts = timed(ws, st_steps, 3, sync)
        sk_fwd = ws.fwd_mean_ms(st_steps)
        sk = ws.kernel_ms(sync)
        sk["fwd"] = sk_fwd                      # the roofline figure: mean over the timed steps
        fl = ws.fwd_flops()
        stress = {"workload": ws.describe("fp32"), "value": ws.n * st_steps / dts, "unit": "rays/s", "ms_per_step": dts / st_steps * 1e3,
                  "kernel_ms": sk, "flops_per_ray_fwd": fl / ws.n,
                  "roofline": {"bound": "mfma", "kernel": "fused_fwd_kernel<512,rays,train>", "achieved": fl / (sk["fwd"] * 1e-3) / 1e12,
                               "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": fl / (sk["fwd"] * 1e-3) / 1e12 / FP32_MFMA_PEAK_TF},
                  "step_frac_of_peak": 3 * fl / (dts / st_steps) / 1e12 / FP32_MFMA_PEAK_TF}
        ws.net.release_workspace()
        del ws

    # a batch larger than the workspace the caller lends: N_rand 8192 walked in 8 slices of 1024 (Trainer(max_rays_per_launch=1024),
    # cfnerf_render_bwd_accumulate) - the reference trains any N_rand (RUN:88-100,602).  One rank, a second of run time; guarded like `eval`
    sliced = None
    if extras and world == 1:
        try:
            wl.__dict__.pop("trainer", None)
            wl.net.release_workspace()
            w8 = Workload("N8192", "train", rank, world, dev, "fp32", False)
            n8 = max(3, min(10, args.steps))
            dt8 = timed(w8, n8, 2, sync)
            sliced = {"workload": w8.describe("fp32"), "value": w8.n * n8 / dt8, "unit": "rays/s", "ms_per_step": dt8 / n8 * 1e3,
                      "slices": w8.launches_per_step(), "workspace_bytes": int(w8.net._ws.numel()),
                      "step_frac_of_peak": 3 * w8.fwd_flops() * w8.launches_per_step() / (dt8 / n8) / 1e12 / FP32_MFMA_PEAK_TF}
            w8.net.release_workspace()
            del w8
        except Exception as e:
            sliced = {"error": f"{type(e).__name__}: {e}"}

    # the coarse + fine sampling EXTENSION (BASELINE configs 2/3/5 are worded "64 + 128"; the reference has no second pass, so
    # this is NOT the parity path and never the headline): coarse 64 -> sample_pdf -> fine 64 + 128, both loss terms
    hier = None
    if extras and args.extension:
        wh = Workload("C2", "train", rank, world, dev, "fp32", False)
        sc = wh.sc

        def hstep():
            return wh.trainer.step_hierarchical(sc["H"], sc["W"], sc["focal"], wh.rays, wh.target, N_samples=64, N_importance=128, coarse_loss=True,
                                                eps=torch.randn(wh.K, 4, device=dev, generator=wh.g), near=sc["near"], far=sc["far"], ndc=sc["ndc"])
        for _ in range(3):
            hstep()
        sync()
        h_steps = max(5, min(20, args.steps))
        t1 = time.perf_counter()
        for _ in range(h_steps):
            hstep()
        sync()
        dth = time.perf_counter() - t1
        hier = {"workload": f"EXTENSION (not in the reference; parity unpinned): coarse 64 samples -> inverse-CDF resampling -> fine 64 + 128 samples "
                            f"through the one network, coarse + fine KDE-NLL terms both differentiated; N_rand={wh.n}, K={wh.K}, W={wh.W}",
                "value": wh.n * h_steps / dth, "unit": "rays/s", "ms_per_step": dth / h_steps * 1e3,
                "points_per_ray": "64 (coarse pass: sampling weights + its loss term) + 192 (fine pass)"}
        wh.net.release_workspace()
        del wh

    # The OTHER half of SURVEY 8(d)'s metric, "rays/sec of eval render" (the reference's render_path_train / uncertainty maps, RUN:247-314,
    # 1117-1131), in the --full line at every GPU count, after the timed region: the C2 batch in eval mode (perturb off, fixed latents
    # with the last one zeroed: one fused forward launch per step, rays per GPU fixed) and BASELINE config 5 - one 800 x 800 image at
    # K = 32 with the K-statistics (mean / uncertainty / disparity / depth) reduced inside the kernel, rows tiled across the ranks
    # with no exchange.  Both timed like the headline: barrier + device sync on both sides, max over ranks.
    evalb = None
    if alt_on and name == "C2" and args.precision == "fp32" and mode == "train" and not force_dist:
        try:                                   # (like the PSNR block: nothing here may take the headline line down with it - ADVICE r5)
            wl.__dict__.pop("trainer", None)
            wl.net.release_workspace()
            we = Workload("C2", "eval", rank, world, dev, "fp32", False)
            e_steps = max(10, min(50, args.steps))
            dte = max_over_ranks(timed(we, e_steps, 3, sync))
            e_fwd = we.fwd_mean_ms(e_steps)
            fle = we.fwd_flops()
            evalb = {"metric": "rays/sec (eval render, fused forward)",
                     "config2_eval": {"workload": we.describe("fp32"), "value": we.n * world * e_steps / dte, "unit": "rays/s", "steps": e_steps,
                                      "ms_per_step": dte / e_steps * 1e3, "fwd_launch_ms": e_fwd,
                                      "roofline": {"bound": "mfma", "kernel": "fused_fwd_kernel<256,rays,eval>", "achieved": fle / (e_fwd * 1e-3) / 1e12,
                                                   "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": fle / (e_fwd * 1e-3) / 1e12 / FP32_MFMA_PEAK_TF,
                                                   "flops_per_launch": fle}}}
            del we
            w5 = Workload("C5", "eval", rank, world, dev, "fp32", False)
            n_img = 2
            dt5 = max_over_ranks(timed(w5, n_img, 1, sync))
            f5 = w5.fwd_mean_ms(n_img)
            sc5 = w5.sc
            fl5 = w5.fwd_flops()
            evalb["config5_full_image"] = {"workload": w5.describe("fp32"), "value": sc5["H"] * sc5["W"] * n_img / dt5, "unit": "rays/s", "images": n_img,
                                           "s_per_image": dt5 / n_img, "fwd_launch_ms": f5,
                                           "outputs": "fused K-statistics per pixel: K-mean rgb, uncertainty std_K n/(n-1) (RUN:1129-1130), mean disparity, mean depth",
                                           "roofline": {"bound": "mfma", "kernel": "fused_fwd_kernel<256,rays,eval>", "achieved": fl5 / (f5 * 1e-3) / 1e12,
                                                        "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": fl5 / (f5 * 1e-3) / 1e12 / FP32_MFMA_PEAK_TF,
                                                        "flops_per_launch": fl5, "note": "this rank's launch (its rows of the image)"}}
            del w5
        except Exception as e:
            if world > 1:
                raise                          # a rank that fell out of max_over_ranks cannot be papered over
            evalb = dict(evalb or {}, error=f"{type(e).__name__}: {e}")

    # PSNR, the second half of the headline metric, on the synthetic stand-in scene - at EVERY GPU count (--full default train run only): one rank
    # trains 1024-ray batches, N ranks train world x 1024-ray global batches through the sharded ray pool + the Trainer's all-reduce.
    # Nothing here may take the headline line down with it: a failure is reported inside the psnr object.
    psnr = None
    if alt_on and name == "C2" and args.precision == "fp32" and mode == "train" and args.psnr_steps > 0 and not force_dist:
        wl.__dict__.pop("trainer", None)
        wl.net.release_workspace()
        try:
            psnr = psnr_block(dev, args.psnr_steps, rank=rank, world=world)
        except Exception as e:
            if world > 1:
                raise                          # a rank that fell out of a collective cannot be papered over
            psnr = {"value": None, "error": f"{type(e).__name__}: {e}"}
        if world > 1:
            vs = psnr_vs_single_process(dev, rank, world, sync)
            if rank == 0:
                psnr["vs_single_process"] = vs

    out = None
    if rank == 0:
        rays_per_s = wl.n * world * args.steps / dt
        fl = wl.fwd_flops()                     # forward GEMM FLOPs of one launch of the fused forward kernel
        # HBM bytes per launch of that kernel from the committed PMC passes (rocprofv3 cannot run inside the bench)
        traffic, mfma_busy, src = None, None, None
        for prof in ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json"):
            try:
                with open(os.path.join(ROOT, "profiles", prof)) as f:
                    tj = json.load(f)[f"{name}:{mode}"]
                traffic, mfma_busy, src = tj["hbm_bytes_per_launch"], tj.get("mfma_busy_frac"), prof
                break
            except Exception:
                continue
        traffic_unit = (f"bytes/launch (PMC FETCH_SIZE x2 + WRITE_SIZE of the committed rocprofv3 --pmc passes, profiles/{src}; not "
                        f"re-measured by this run)") if src else None
        if live is not None:
            traffic, mfma_busy = live["hbm_bytes_per_launch"], live["mfma_busy_frac"]
            traffic_unit = ("bytes/launch, OBSERVED BY THIS RUN: rocprofv3 --kernel-trace --pmc child passes of the same workload (3 steps each: "
                            "FETCH_SIZE; WRITE_SIZE; SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE) before the timed region; FETCH_SIZE x2 per "
                            "MI355X_MICROARCH.md (gfx950 reports half of a wide coalesced read), KB -> bytes")
        roof = {"bound": "mfma", "kernel": f"fused_fwd_kernel<{wl.W},rays,{'train' if mode == 'train' else 'eval'}>",
                "achieved": fl / (fwd_ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s", "traffic": traffic,
                "traffic_unit": traffic_unit, "traffic_source": "live" if live is not None else ("profiles/" + src if src else None),
                "mfma_busy_frac_pmc": mfma_busy, "launch_ms": fwd_ms, "flops_per_launch": fl}
        if live is not None:
            roof["pmc_live"] = {"FETCH_SIZE_KB": live["FETCH_SIZE_KB"], "WRITE_SIZE_KB": live["WRITE_SIZE_KB"]}
        roof["frac"] = roof["achieved"] / roof["peak"]
        sm = sorted(step_ms)
        out = {
            "metric": "rays/sec (train step)" if mode == "train" else "rays/sec (eval render, fused forward)",
            "value": rays_per_s, "unit": "rays/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if args.precision == "fp32" else "bf16x3-split MFMA, f32 accumulate (opt-in mode)", "data": "synthetic",
            "config": {"workload": wl.describe(args.precision),
                       "parallelism": f"ray-sharded dp{world}" + (", 1 RCCL all-reduce of flat grads/step" if mode == "train" and world > 1 else "")},
            "roofline": roof,
            # per-step durations of rank 0 from one HIP event per step inside the timed region (value uses the wall clock over all K)
            "ms_per_step_median": sm[len(sm) // 2] if len(sm) % 2 else 0.5 * (sm[len(sm) // 2 - 1] + sm[len(sm) // 2]),
            "ms_per_step_min": sm[0], "ms_per_step_max": sm[-1],
        }
        if same_gpu and world > 1:
            out["config"]["parallelism"] += " [CFNERF_BENCH_SAME_GPU=1: all ranks share cuda:0 and exchange over gloo - a code-path test, not a scaling number]"
        if mode == "train":
            if kms is not None:
                out["kernel_ms"] = kms
            out["step_frac_of_peak"] = 3 * fl * wl.launches_per_step() / (dt / args.steps) / 1e12 / FP32_MFMA_PEAK_TF
        if psnr is not None:
            out["psnr"] = psnr
        if evalb is not None:
            out["eval"] = evalb
        if alt is not None:
            out["alt_precision"] = alt
        if cfg4 is not None:
            out["config4_k16"] = cfg4
        if stress is not None:
            out["stress_w512"] = stress
        if sliced is not None:
            out["sliced_batch_n8192"] = sliced
        if hier is not None:
            out["alt_config"] = hier
        if comm is not None:
            out["comm"] = comm
            out["rank_skew"] = skew

    # the JSON line is the LAST thing on stdout: RCCL prints its version banner through libc's buffered stdout (it would
    # otherwise surface at process exit, after the line), so every rank flushes that before the final barrier
    def flush_c_stdio():
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
    flush_c_stdio()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    flush_c_stdio()
    # the CPU leg - at every N, on rank 0, AFTER the final barrier (the other ranks are done; nothing waits in a collective while the host
    # cores are timed): the oracle as the CPU baseline and as the checker of the two PSNR agreements.  A failure in here is reported
    # inside the object it belongs to; the headline line is printed regardless.
    if rank == 0 and args.full and not args.no_cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline(mode, wl.cfg)
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "error": f"{type(e).__name__}: {e}"}
        if psnr is not None and psnr.get("value") is not None:
            wl.__dict__.pop("trainer", None)
            wl.net.release_workspace()
            for key, fn in (("vs_oracle", lambda: psnr_oracle_agreement(dev)), ("vs_reference_run", psnr_reference_run_agreement)):
                try:
                    psnr[key] = fn()
                except Exception as e:
                    psnr[key] = {"agree": None, "error": f"{type(e).__name__}: {e}"}
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
