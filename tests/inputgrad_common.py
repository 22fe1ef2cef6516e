"""Shared by tests/test_inputgrad_cpu.py and tests/test_hip_inputgrad.py: the G25 fixtures of the real reference (tests/golden/inputgrad/)
and the oracle's own autograd for the same cases - the gradient with respect to the INPUTS of NeRF_Flows.forward / run_network."""
import os

import numpy as np
import torch

from oracle import cfnerf_oracle as O

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputgrad")
NAMES = ["g25a_train_x_grad", "g25b_run_network_grads", "g25c_eval_x_grad"]
T = lambda a: torch.tensor(np.asarray(a))


def load(name):
    return dict(np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False))


def cfg_of(g):
    return O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))


def masks_of(g):
    """the reference's ReLU masks as O.relu_override / hip_relu_masks name them"""
    return {k[len("mask."):]: T(v).float() for k, v in g.items() if k.startswith("mask.")}


def eval_latents(g):
    """(eps_alpha, eps_rgb) of the eval branch: the fixed latents with the LAST sample zeroed (MOD:199,205)"""
    ea, er = T(g["sample_alpha"]).clone(), T(g["sample_rgb"]).clone()
    ea[-1], er[-1] = 0, 0
    return ea, er


def oracle_grads(name, g, masks=None):
    """{tensor name: gradient} of the fixture's loss on the oracle (fp32 CPU autograd), optionally on imposed ReLU masks; + raw"""
    cfg = cfg_of(g)
    p = O.make_params(cfg, int(g["seed"]))
    G = T(g["G"])
    with O.relu_override(masks=masks):
        if name == "g25b_run_network_grads":
            pts, dirs = T(g["pts"]).clone().requires_grad_(True), T(g["viewdirs"]).clone().requires_grad_(True)
            raw, ent = O.run_network(p, pts, dirs, T(g["eps_alpha"]), T(g["eps_rgb"]), cfg, False)
            ((raw.reshape(G.shape) * G).sum() + float(g["c_entropy"]) * ent).backward()
            return {"pts_grad": pts.grad, "viewdirs_grad": dirs.grad}, raw.detach()
        x = T(g["x"]).clone().requires_grad_(True)
        if name == "g25a_train_x_grad":
            raw, ent = O.nerf_flows_forward(p, x, T(g["eps_alpha"]), T(g["eps_rgb"]), cfg, False)
            ((raw * G).sum() + float(g["c_entropy"]) * ent).backward()
        else:
            ea, er = eval_latents(g)
            raw, _ = O.nerf_flows_forward(p, x, ea, er, cfg, True)
            (raw * G).sum().backward()
        return {"x_grad": x.grad}, raw.detach()
