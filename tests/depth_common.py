"""Shared by tests/test_depth_cpu.py and tests/test_hip_depth.py: the G24 fixtures (tests/golden/depth/) and the depth-supervised
step composed on the CPU oracle - one render_rays per network call of the reference's batch, the loss lines of RUN:1019-1054 on top."""
import contextlib
import hashlib
import os

import numpy as np
import torch

from oracle import cfnerf_oracle as O

DEPTH_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth")
T = lambda a: torch.tensor(np.asarray(a))
S = 128


def load(name):
    return dict(np.load(os.path.join(DEPTH_DIR, name + ".npz"), allow_pickle=False))


def cfg_of(g):
    return O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))


def t_rand_of(g):
    if "t_rand" in g:
        return T(g["t_rand"])
    n = g["rays"].shape[1]
    t_np = np.random.default_rng(int(g["t_rand_seed"])).uniform(0, 1, (n, S)).astype(np.float32)
    assert hashlib.sha256(t_np.tobytes()).hexdigest() == str(g["t_rand_sha256"])
    return T(t_np)


def calls_of(g):
    """(first ray, end ray) of every network call of the fixture's batch (one cut: chunk >= N)."""
    n, per = g["rays"].shape[1], int(g["netchunk"]) // S
    return [(lo, min(lo + per, n)) for lo in range(0, n, per)]


def packed_of(g):
    rays = T(g["rays"])
    return O.pack_rays(int(g["H"]), int(g["W"]), float(g["focal"]), rays[0], rays[1], False, float(g["near"]), float(g["far"]))


def oracle_depth_step(p, g, t_rand, masks=None, flips_against=None):
    """The reference's depth-supervised step on the oracle: every network call rendered with its own latent pair, the KDE-NLL over the
    colour rays, beta1 times the FIRST call's entropy, depth_lambda * mse of the K-mean depth of the depth rays.  ``masks``: per call,
    ReLU masks to impose (tests on the GPU: those of the HIP forward); ``flips_against``: per call, masks to count the oracle's own
    against (``scalars["flips"]`` = (differing units, units)).  Returns (scalars, gradients, per-call entropies)."""
    cfg = cfg_of(g)
    K, n_c, n_d = cfg.K_samples, int(g["n_colour"]), int(g["n_depth"])
    packed, target, td = packed_of(g), T(g["target"]), T(g["target_depth"])
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    nll, sq, ents, flips = 0., 0., [], [0, 0]
    for c, (lo, hi) in enumerate(calls_of(g)):
        rec = {} if flips_against is not None else None
        with (O.relu_override(masks=masks[c]) if masks is not None else
              O.relu_override(record=rec) if rec is not None else contextlib.nullcontext()):
            ret = O.render_rays(q, packed[lo:hi], cfg, T(g["eps_alpha"][c]), T(g["eps_rgb"][c]), True, t_rand[lo:hi])
        for k, pre in (rec or {}).items():
            flips[0] += int(((pre > 0).float() != flips_against[c][k]).sum())
            flips[1] += pre.numel()
        ents.append(ret["loss_entropy"])
        hc, ld = min(hi, n_c), max(lo, n_c)
        if hc > lo:                                     # colour rows of this call: their share of the mean over n_c rays
            nll = nll + O.train_loss(ret["rgb_map"][:hc - lo], target[lo:hc], ret["loss_entropy"], K, 0.)["loss_nll"] * ((hc - lo) / n_c)
        if hi > ld:
            sq = sq + ((ret["depth_map"][ld - lo:].mean(-1) - td[ld - n_c:hi - n_c]) ** 2).sum()
    depth_loss = sq / n_d
    loss = nll + float(g["beta1"]) * ents[0] + float(g["depth_lambda"]) * depth_loss
    loss.backward()
    scal = dict(loss=float(loss.detach()), loss_nll=float(nll.detach()), loss_entropy=float(ents[0].detach()),
                depth_loss=float(depth_loss.detach()), flips=tuple(flips))
    return scal, {k: v.grad for k, v in q.items()}, [float(e.detach()) for e in ents]


def fixture_gradient(g, key):
    """(reference gradient entries, their flat indices or None for "all", largest entry, norm or None) of one tensor, or None when the
    reference gave it no gradient."""
    if ("grad." + key) in g:
        ref = g["grad." + key].astype(np.float64).reshape(-1)
        return ref, None, max(float(np.abs(ref).max()), 1e-12), float(np.linalg.norm(ref))
    if ("gradsample." + key) in g:
        return (g["gradsample." + key].astype(np.float64), g["gradidx." + key], max(float(g["gradabsmax." + key]), 1e-12),
                float(g["gradnorm." + key]))
    return None
