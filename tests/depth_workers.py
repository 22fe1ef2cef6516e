"""Rank body of the two-rank depth-supervision test (importable by name from a fork-server child)."""
import os


def depth_trainer_rank(rank, world, port, q, spec):
    """One rank of a world-2 depth-supervised Trainer.step on cuda:0 over a gloo group: its shard of the colour rays and of the depth
    rays.  Reports the step's latents, the exchanged (summed) gradient, its loss / depth_loss contributions and the parameters."""
    import numpy as np
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import contextlib
        import io

        import cfnerf_amd                                      # noqa: F401
        from cfnerf_amd import train as TR
        from oracle import cfnerf_oracle as O
        from util_hip import build_model, fern_rays
        cfg = O.OracleCfg(netwidth=spec["W"], K_samples=spec["K"])
        with contextlib.redirect_stdout(io.StringIO()):
            _, _, _, model, _, _ = build_model(cfg, spec["seed"], no_ndc=True)
        rng = np.random.default_rng(spec["data_seed"])
        n_c, n_d = spec["n_colour"], spec["n_depth"]
        rays, (H, Wd, focal) = fern_rays(rng, n_c + n_d)
        target = torch.tensor(rng.uniform(0, 1, (n_c, 3)), dtype=torch.float32)
        td = torch.tensor(rng.uniform(2, 6, (n_d,)), dtype=torch.float32)
        t_rand = torch.tensor(rng.uniform(0, 1, (n_c + n_d, 128)), dtype=torch.float32)
        (lo, hi), (dlo, dhi) = TR.shard_bounds(n_c, rank, world), TR.shard_bounds(n_d, rank, world)
        tr = TR.Trainer(model, beta1=spec["beta1"], world_size=world, overlap_comm=False, depth_lambda=spec["depth_lambda"])
        torch.manual_seed(1000 + rank)                        # DIFFERENT seeds per rank: the latents must still agree
        eps = tr._step_eps().cpu().numpy().copy()             # what step() is about to use (idempotent)
        sc = tr.step(H, Wd, focal, (rays[0, lo:hi].cuda(), rays[1, lo:hi].cuda()), target[lo:hi].cuda(),
                     t_rand=torch.cat([t_rand[lo:hi], t_rand[n_c + dlo:n_c + dhi]]).cuda(), near=1.2, far=8.0, ndc=False,
                     depth_rays=rays[:, n_c + dlo:n_c + dhi].cuda(), target_depth=td[dlo:dhi].cuda())
        torch.cuda.synchronize()
        q.put((rank, "ok", eps, tr.grad.cpu().numpy(), np.concatenate([sc[:3].cpu().numpy(), tr.depth_loss.cpu().numpy()]),
               model.module.flat.detach().cpu().numpy()))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None, None, None))
        raise
