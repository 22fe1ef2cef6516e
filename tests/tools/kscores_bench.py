"""The ensemble scores (CFNERF_F_KSCORES, cfnerf_kscores.hip) on the clock:

1. one ``k_scores_kernel`` call with every output and Q = 7 quantile levels at 49 152 rows (a 128 x 128 tile's 3 colour rows per pixel) x
   K = 4, 32, 64, 128, against fp32 torch evaluating the same closed forms (``torch.sort`` and the reductions) on the same inputs,
   alternating; with the achieved GB/s over the call's ALGORITHMIC bytes: M K 4 (samples in) + M 4 (target in) + M K 4 (sorted out) +
   M (Q + 3) 4 (quantiles, rank_code, pit, crps out);
2. ``image_metrics`` of one 800 x 800 view at S = 128, K = 32 with ``calibration=True`` against the default (whose code path is the one from
   before the scores existed), alternating.

    python tests/tools/kscores_bench.py [--kernel-only]           (MI355X; summary kept in profiles/r21_kscores.txt)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import statistics
import time
import numpy as np
import torch
import cfnerf_amd                                    # noqa: F401  (package alias for the hyphenated directory)
from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
import kscores_common as KS

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


def torch_scores(x, y, lv):
    """the same closed forms in fp32 torch: sort, interpolated order statistics, rank counts, the gap form of the CRPS"""
    K = x.shape[1]
    s = torch.sort(x, dim=1).values
    lo = torch.tensor([l for l, _ in lv], device=x.device)
    fr = torch.tensor([f for _, f in lv], device=x.device)
    xl, xh = s[:, lo], s[:, torch.clamp(lo + 1, max=K - 1)]
    q = xl + fr * (xh - xl)
    code = 2 * (x < y[:, None]).sum(1) + (x == y[:, None]).sum(1)
    pit = code.float() / (2 * K)
    g = torch.arange(K - 1, device=x.device)
    wgt = ((g + 1) * (K - 1 - g)).float()
    crps = (x - y[:, None]).abs().sum(1) / K - ((s[:, 1:] - s[:, :-1]) * wgt).sum(1) / (K * K)
    return s, q, code, pit, crps


def kernel_block():
    print("== one call: k_scores_kernel (all outputs, Q = 7) vs fp32 torch (torch.sort + the same closed forms), same inputs, alternating windows; "
          "us per call, median (min .. max)")
    M = 49152
    for K in (4, 32, 64, 128):
        x, y = KS.make_rows(M, K, seed=K, special=False)
        xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
        lv = L.quantile_levels(KS.LEVELS, K)
        so, q = torch.empty(M, K, device=DEV), torch.empty(M, len(lv), device=DEV)
        rc, pit, crps = torch.empty(M, dtype=torch.int32, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)

        def hip():
            L.k_scores(xd, M, K, target=yd, sorted_out=so, quantiles=q, levels=lv, rank_code=rc, pit=pit, crps=crps)

        def torch_fp32():
            torch_scores(xd, yd, lv)

        hip()
        ts, tq, tc, tp, tcr = torch_scores(xd, yd, lv)
        A, B = KS.crps_terms(x, y)
        pos = (A + B) > 0                         # (a row of ties with its target among them has A = B = 0)
        ek = np.abs(crps.cpu().numpy() - (A - B))[pos] / (KS.U24 * (A + B)[pos])
        et = np.abs(tcr.cpu().numpy() - (A - B))[pos] / (KS.U24 * (A + B)[pos])
        print(f"   (same function: sorted equal {torch.equal(so, ts)}, rank_code equal {torch.equal(rc.long(), tc)}, crps error kernel {ek.max():.2f} / torch {et.max():.2f} "
              f"units of 2^-24 (A + B))")
        (h, hlo, hhi), (t, tlo, thi) = alternate(hip, torch_fp32)
        nbytes = 2 * M * K * 4 + M * 4 + M * (len(lv) + 3) * 4
        print(f"M={M} K={K:3d}  kernel {h * 1e3:8.1f} ({hlo * 1e3:.1f} .. {hhi * 1e3:.1f})   torch fp32 {t * 1e3:8.1f} ({tlo * 1e3:.1f} .. {thi * 1e3:.1f})   "
              f"x{t / h:.1f}   {nbytes / 1e6:.2f} MB algorithmic -> {nbytes / (h * 1e-3) / 1e9:.0f} GB/s", flush=True)


def metrics_block(rounds=3):
    from oracle import cfnerf_oracle as O
    from util_hip import build_model
    print("== image_metrics of one 800 x 800 view, S = 128, K = 32, netwidth 256: calibration=True against the default, alternating; s per view", flush=True)
    H = W = 800
    cfg = O.OracleCfg(netwidth=256, K_samples=32)
    _, _, _, model, _, _ = build_model(cfg, 7, no_ndc=True)
    pose = torch.tensor([[1, 0, 0, 0.1], [0, 1, 0, -0.1], [0, 0, 1, 4.0]], dtype=torch.float32)
    rng = np.random.default_rng(0)
    gt = torch.tensor(rng.uniform(0, 1, (H, W, 3)), dtype=torch.float32).to(DEV)
    gtd = torch.tensor(rng.uniform(2, 6, (H, W)), dtype=torch.float32).to(DEV)
    kw = dict(near=2.0, far=6.0, ndc=False)

    def run(cal):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = E.image_metrics(H, W, 1111.0, pose, model, gt, gt_depth=gtd, calibration=cal, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, m

    run(False); run(True)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(run(False)[0]); tb.append(run(True)[0])
        print(f"   default {ta[-1]:.3f} s   calibration=True {tb[-1]:.3f} s", flush=True)
    a, b = statistics.median(ta), statistics.median(tb)
    m = run(True)[1]
    print(f"default {a:.3f} s   calibration=True {b:.3f} s   delta {b - a:+.3f} s ({100 * (b - a) / a:+.1f} %)")
    print("   " + ", ".join(f"{k} {v:.4g}" for k, v in m.items() if not isinstance(v, list)))


if __name__ == "__main__":
    kernel_block()
    if "--kernel-only" not in sys.argv:
        metrics_block()
