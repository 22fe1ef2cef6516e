"""The image similarity (CFNERF_MODE_SSIM, cfnerf_ssim.hip) on the clock: one ``ssim_kernel`` call (map and mean: the tile launch and the small
mean launch) on 800 x 800 x 3 and 378 x 504 x 3 images, uniform 7 x 7 and Gaussian 11 x 11 windows, against fp32 torch evaluating the same
closed form with ``F.conv2d`` (grouped, separable) on the same images, alternating; with the achieved GB/s over the call's ALGORITHMIC
bytes - the two images read once, the map written once.  A batch of 16 such images in one call tells the launch latency of a single view
from the kernel's throughput.

    python tests/tools/ssim_bench.py           (MI355X; summary kept in profiles/r22_ssim.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import statistics
import numpy as np
import torch
import torch.nn.functional as F
import cfnerf_amd                                    # noqa: F401  (package alias for the hyphenated directory)
from cfnerf_amd import _lib as L
import ssim_common as SC

DEV = "cuda"


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


def torch_ssim(x, y, taps, cov):
    """the same closed form in fp32 torch on [B,C,H,W]: separable grouped conv2d, E[x^2] - mu^2"""
    C_ = x.shape[1]
    t = torch.tensor(taps, device=x.device)
    kh, kv = t.reshape(1, 1, 1, -1).repeat(C_, 1, 1, 1), t.reshape(1, 1, -1, 1).repeat(C_, 1, 1, 1)
    f = lambda a: F.conv2d(F.conv2d(a, kh, groups=C_), kv, groups=C_)
    mx, my = f(x), f(y)
    vx, vy, vxy = cov * (f(x * x) - mx * mx), cov * (f(y * y) - my * my), cov * (f(x * y) - mx * my)
    S = ((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    return S, S.mean(dim=(2, 3))


def main():
    print("== one call: ssim_kernel (map + mean) vs fp32 torch (separable grouped conv2d, the same closed form), same images, alternating windows; "
          "us per call, median (min .. max)")
    rng = np.random.default_rng(0)
    for H, W in ((800, 800), (378, 504)):
        for kind, win in (("uniform", 7), ("gaussian", 11)):
            for B in (1, 16):
                C_ = 3
                x = np.clip(0.9 + 0.05 * rng.standard_normal((B, H, W, C_)), 0, 1).astype(np.float32)
                y = np.clip(x + 0.02 * rng.standard_normal(x.shape), 0, 1).astype(np.float32)
                xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
                xt, yt = xd.permute(0, 3, 1, 2).contiguous(), yd.permute(0, 3, 1, 2).contiguous()
                taps, cov = L.ssim_window(kind, win)
                smap, mean = torch.empty(B, H - win + 1, W - win + 1, C_, device=DEV), torch.empty(B, C_, device=DEV)
                scratch = torch.empty(L.ssim_scratch_floats(B, C_, H, W, win) // 2, dtype=torch.float64, device=DEV)

                def hip():
                    L.ssim(xd, yd, B, H, W, C_, taps, cov, 1e-4, 9e-4, ssim_map=smap, mean=mean, scratch=scratch)

                def torch_fp32():
                    torch_ssim(xt, yt, taps, cov)

                hip()
                if B == 1:
                    ref = SC.yardstick(x[0], y[0], kind, win)[0]
                    tm = torch_ssim(xt, yt, taps, cov)[0][0].permute(1, 2, 0)
                    print(f"   (same function: max error against fp64 kernel {SC.max_err(smap[0].cpu().numpy(), ref):.2e} / torch fp32 {SC.max_err(tm.cpu().numpy(), ref):.2e})")
                (h, hlo, hhi), (t, tlo, thi) = alternate(hip, torch_fp32, n=40 if B == 1 else 10)
                nbytes = (2 * B * H * W * C_ + smap.numel()) * 4
                print(f"{H}x{W}x{C_} B={B:2d} {kind:8s} win {win:2d}  kernel {h * 1e3:8.1f} ({hlo * 1e3:.1f} .. {hhi * 1e3:.1f})   torch fp32 {t * 1e3:8.1f} "
                      f"({tlo * 1e3:.1f} .. {thi * 1e3:.1f})   x{t / h:.1f}   {nbytes / 1e6:.2f} MB algorithmic -> {nbytes / (h * 1e-3) / 1e9:.0f} GB/s   "
                      f"{h * 1e3 / B:.1f} us per image", flush=True)


if __name__ == "__main__":
    main()
