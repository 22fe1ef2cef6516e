"""Worker of tests/test_eval_metrics_cpu.py (a module of its own: spawned children import it by name)."""
import os

import torch
import torch.distributed as dist


def gather_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cfnerf_amd import evaluate as E
    from eval_metrics_common import gather_problem
    H, W, full = gather_problem()
    r0, r1 = E.row_shard(H, rank, world)
    got = E.gather_rows({k: v[r0:r1].clone() for k, v in full.items()}, H, world, rank)
    if rank == 0:
        q.put({k: (v.numpy() if torch.is_tensor(v) and v.ndim else float(v)) for k, v in got.items()})
    else:
        assert got is None
    dist.destroy_process_group()
