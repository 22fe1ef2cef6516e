"""Rank body of the two-rank netchunk-latent test (importable by name from a fork-server child)."""
import os


def netchunk_trainer_rank(rank, world, port, q, spec):
    """One rank of a world-2 Trainer(latent_draws="netchunk") step on cuda:0 over a gloo group, seeded differently from the other
    rank: reports the step's latent pairs, the exchanged (summed) gradient and the parameters after the step."""
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
            _, _, _, model, _, _ = build_model(cfg, spec["seed"])
        rng = np.random.default_rng(spec["data_seed"])
        N = spec["N"]
        rays, (H, Wd, focal) = fern_rays(rng, N)
        target = torch.tensor(rng.uniform(0, 1, (N, 3)), dtype=torch.float32)
        t_rand = torch.tensor(rng.uniform(0, 1, (N, 128)), dtype=torch.float32)
        lo, hi = TR.shard_bounds(N, rank, world)
        tr = TR.Trainer(model, beta1=spec["beta1"], world_size=world, overlap_comm=False, latent_draws="netchunk",
                        netchunk=spec["netchunk"], chunk=spec["chunk"])
        torch.manual_seed(1000 + rank)                        # DIFFERENT seeds per rank: the latents must still agree
        tr.step(H, Wd, focal, (rays[0, lo:hi].cuda(), rays[1, lo:hi].cuda()), target[lo:hi].cuda(), t_rand=t_rand[lo:hi].cuda())
        torch.cuda.synchronize()
        q.put((rank, "ok", tr.last_eps_chunks.cpu().numpy(), tr.grad.cpu().numpy(), model.module.flat.detach().cpu().numpy()))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc(), None, None))
        raise
