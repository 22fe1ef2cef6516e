"""Pure-torch restatement of the two reductions CFNERF_F_KSTATS_EXT adds to the fused eval render, shared by
tests/test_eval_metrics_cpu.py (which pins it to the oracle's train_loss and to np.std * n/(n-1)) and tests/test_hip_eval_metrics.py
(which holds the kernel to it).  Works in the dtype of its inputs; the two constants of RUN:1036,1039 are made in fp32 as the
reference makes them."""
import math

import torch


def spread(x):
    """np.std(x, -1) * n / (n - 1) (RUN:1129-1130): biased standard deviation over the last axis, times n/(n-1).  x [..., K]."""
    n = x.shape[-1]
    return torch.sqrt(((x - x.mean(-1, keepdim=True)) ** 2).mean(-1)) * n / (n - 1)


def nll_terms(rgbs, gt):
    """rgbs [n,3,K], gt [n,3] -> (nll [n,3], lik [n,3]): the per-pixel, per-channel integrand of loss_nll (RUN:1034-1042) and the
    likelihood mean_k[exp(-(rgb_k - gt)^2 / (2 h^2))] * (2 pi)^(-1.5) / h it is the -log(. + 1e-5) of."""
    n = rgbs.shape[-1]
    d = rgbs - gt[..., None]
    mean = rgbs.mean(-1, keepdim=True)
    std_unbiased = torch.sqrt(((rgbs - mean) ** 2).sum(-1) / (n - 1))                         # torch.std
    bw = float(torch.pow(torch.tensor(0.8 / n), torch.tensor(-1 / 7)))                        # RUN:1036 (fp32 constant)
    c2pi = float(torch.pow(torch.tensor(2 * math.pi), -1.5))                                  # RUN:1039 (fp32 constant)
    h = (std_unbiased * n / (n - 1) * bw + 1e-05)[..., None]                                  # RUN:1034,1036
    lik = (torch.exp(-(d * d) / (2 * h * h)) * (c2pi / h)).mean(-1)                           # RUN:1038-1040
    return -torch.log(lik + 1e-05), lik                                                       # RUN:1041-1042


def gather_problem():
    """The full-image maps of the world-size-2 gather test: H = 7 rows (shards of 4 and 3), every key of stats='ext' with gt."""
    H, W = 7, 5
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.rand(*s, generator=g)
    full = {"rgb_mean": r(H, W, 3), "rgb_unc": r(H, W, 3), "disp_mean": r(H, W), "depth_mean": r(H, W), "sq_err": r(H, W, 3),
            "disp_unc": r(H, W), "depth_unc": r(H, W), "acc_mean": r(H, W), "acc_unc": r(H, W), "nll": r(H, W, 3) * 11 - 3}
    return H, W, full
