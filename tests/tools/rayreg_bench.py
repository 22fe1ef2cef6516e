"""The ray regularisers (CFNERF_F_RAY_REG, cfnerf_rayreg.hip) on the clock, at the train batch's shapes:

1. one ``ray_reg_kernel`` call (the accumulator memset + the launch: forward, gradient and direct d_z) against fp32 torch evaluating the same
   O(S) closed forms, forward + autograd (tests/rayreg_common.py), on the same inputs, alternating; with the achieved GB/s over the call's
   ALGORITHMIC bytes, 2 N S K 4 (weights in, d_weights out) + N S 4 (1 or 2) (z_vals in, d_z out) - context, not a target: a ray's block is
   walked three times out of L2;
2. the C2 and K64 train step of bench.py with both lambdas > 0 against the same step with both at 0, alternating - the delta holds the
   ``weights`` write of the forward, this kernel and the backward's cotangent route (tail_cot_kernel).

    python tests/tools/rayreg_bench.py            (MI355X; summary kept in profiles/r20_rayreg.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import statistics
import torch
import cfnerf_amd                                    # noqa: F401  (package alias for the hyphenated directory)
from cfnerf_amd import _lib as L
from cfnerf_amd import train as TR
import rayreg_common as R

DEV = "cuda"
LAM = dict(distortion=0.01, entropy=0.001)


def ev_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(n):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def alternate(fa, fb, rounds=9, n=40, warm=20):
    """medians (and min .. max) of `rounds` windows of n calls each, a window of fa then a window of fb"""
    for _ in range(warm):
        fa(); fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(ev_ms(fa, n)); tb.append(ev_ms(fb, n))
    f = lambda t: (statistics.median(t), min(t), max(t))
    return f(ta), f(tb)


def kernel_block():
    print("== one call: ray_reg_kernel vs fp32 torch closed forms (forward + autograd), same inputs, alternating windows; us per call, median (min .. max)")
    for name, N, S, K in (("C2", 1024, 128, 4), ("K64", 1024, 128, 64)):
        w64, z64 = R.composite_weights(N, S, K, seed=K)
        w, z = w64.float().to(DEV), z64.float().to(DEV)
        rays = torch.zeros(N, 11, device=DEV); rays[:, 6] = 2.; rays[:, 7] = 6.
        d_w, d_z, sc = torch.empty_like(w), torch.empty_like(z), torch.empty(8, device=DEV)

        def hip():
            L.ray_reg(w, z, d_w, sc, rays=rays, d_z=d_z, lambda_dist=LAM["distortion"], lambda_ent=LAM["entropy"])

        wl, zl = w.clone().requires_grad_(), z.clone().requires_grad_()

        def torch_fp32():                            # forward + backward of the same O(S) forms, by autograd
            _, m, dl, _ = R.geometry(zl, (2., 6.))
            m, dl = m[..., None], dl[..., None]
            dm = torch.cat([m[:, 1:] - m[:, :-1], torch.zeros_like(m[:, :1])], 1)
            Wi = torch.cumsum(wl, 1)
            zero = torch.zeros_like(wl[:, :1])
            Q = torch.cat([zero, torch.cumsum(Wi * dm, 1)[:, :-1]], 1)
            D = (2 * wl * Q).sum(1) + (wl * wl * dl).sum(1) / 3
            A = wl.sum(1)
            mask = (A.detach() > 0.1).to(wl.dtype)
            reg = (LAM["distortion"] * D.sum() + LAM["entropy"] * (mask * R.entropy_12c(wl)).sum()) / (N * K)
            wl.grad = zl.grad = None
            reg.backward()

        hip(); torch_fp32()
        ref = R.closed_forms(w.double(), z.double(), (2., 6.), **LAM)
        print(f"   (same function: kernel d_weights {R.rel_err(d_w, ref['d_weights']):.1e}, torch autograd d_weights {R.rel_err(wl.grad, ref['d_weights']):.1e}, "
              f"kernel d_z {R.rel_err(d_z, ref['d_z']):.1e}, torch d_z {R.rel_err(zl.grad, ref['d_z']):.1e} of the largest fp64 entry)")
        (h, hlo, hhi), (t, tlo, thi) = alternate(hip, torch_fp32)
        nbytes = 2 * N * S * K * 4 + N * S * 4 * 2
        print(f"{name:4s} N={N} S={S} K={K:3d}  kernel {h * 1e3:8.1f} ({hlo * 1e3:.1f} .. {hhi * 1e3:.1f})   torch fp32 {t * 1e3:8.1f} ({tlo * 1e3:.1f} .. {thi * 1e3:.1f})   "
              f"x{t / h:.1f}   {nbytes / 1e6:.2f} MB algorithmic -> {nbytes / (h * 1e-3) / 1e9:.0f} GB/s", flush=True)


def step_block():
    import bench
    print("== train step of bench.py: both lambdas > 0 against both at 0, alternating windows; ms per step, median (min .. max)")
    for name in ("C2", "K64"):
        wl = bench.Workload(name, "train", 0, 1, torch.device(DEV))
        plain = wl.trainer
        reg = TR.Trainer(wl.net, lrate=5e-4, lrate_decay=250, beta1=0.01, distortion_lambda=LAM["distortion"], ray_entropy_lambda=LAM["entropy"])

        def run(tr):
            def f():
                wl.trainer = tr
                wl.step()
            return f
        (p, plo, phi), (r, rlo, rhi) = alternate(run(plain), run(reg), rounds=7, n=30, warm=10)
        print(f"{name:4s} lambda = 0 {p:7.3f} ({plo:.3f} .. {phi:.3f})   lambda > 0 {r:7.3f} ({rlo:.3f} .. {rhi:.3f})   delta {1e3 * (r - p):+7.1f} us "
              f"({100 * (r - p) / p:+.1f} %)   reg_scalars {[round(v, 6) for v in reg.reg_scalars.tolist()]}", flush=True)
        del wl, plain, reg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    kernel_block()
    step_block()
