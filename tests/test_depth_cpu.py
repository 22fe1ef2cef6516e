"""Depth supervision (the reference's colmap_depth) on the CPU: the G24 fixtures of the real reference, train.depth_term against
autograd of the reference's loop lines, the depth-supervised step composed on the oracle, the key-point ray formula and the
DepthRayPool feeder, and the unchanged C ABI.  No kernel runs."""
import glob
import hashlib
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cfnerf_amd import _lib as L
from cfnerf_amd import api
from cfnerf_amd import train as TR
from cfnerf_amd.data import DepthRayPool, RayPool
from oracle import cfnerf_oracle as O

import depth_common as DC
from depth_common import T, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _digest(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))


def _manifest(path=DC.DEPTH_DIR):
    with open(os.path.join(path, "MANIFEST.json")) as f:
        return json.load(f)


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------------------

def test_depth_fixtures_match_their_manifest():
    man = _manifest()
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(DC.DEPTH_DIR, "*.npz")))
    assert names == sorted(man) == ["g24a_depth_one_call", "g24b_depth_two_calls", "g24c_depth_c2"]
    for name in names:
        g = load(name)
        assert sorted(g) == sorted(man[name]), name
        for k, v in g.items():
            assert _digest(v) == man[name][k], (name, k)
        assert os.path.getsize(os.path.join(DC.DEPTH_DIR, name + ".npz")) < 512 * 1024


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="the reference only exists in the build container")
def test_committed_depth_generator_reproduces_the_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_depth.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _manifest(str(tmp_path)) == _manifest()


def test_fixture_shapes_and_the_first_call_entropy():
    """What the reference's cut of the per-point entropy tensor to its first N_c rows yields: the FIRST network call's entropy."""
    a, b, c = load("g24a_depth_one_call"), load("g24b_depth_two_calls"), load("g24c_depth_c2")
    for g, (n_c, n_d, calls) in ((a, (24, 8, 1)), (b, (12, 4, 2)), (c, (1024, 128, 3))):
        assert (int(g["n_colour"]), int(g["n_depth"])) == (n_c, n_d) and g["rays"].shape == (2, n_c + n_d, 3)
        assert g["rgb_map"].shape == (n_c + n_d, 3, 4) and g["depth_map"].shape == (n_c + n_d, 4) and g["target_depth"].shape == (n_d,)
        assert g["eps_alpha"].shape == (calls, 4, 1) and g["loss_entropy_chunks"].shape == (calls,) and len(DC.calls_of(g)) == calls
        assert 2.0 <= g["target_depth"].min() and g["target_depth"].max() <= 6.0
        assert abs(float(g["loss_entropy"]) - float(g["loss_entropy_chunks"][0])) <= 1e-6 * float(g["loss_entropy"])
        want = float(g["loss_nll"]) + float(g["beta1"]) * float(g["loss_entropy"]) + float(g["depth_lambda"]) * float(g["depth_loss"])
        assert abs(float(g["loss"]) - want) <= 1e-6 * want
    assert abs(float(b["loss_entropy_all_points"]) - float(b["loss_entropy"])) > 1e-3 * float(b["loss_entropy"])


# ---- 2. train.depth_term against autograd of the reference's lines --------------------------------------------------------------------

def _reference_depth_lines(depth_map, target_depth, n_batch, depth_lambda):
    from make_golden_depth import reference_depth_step
    K = depth_map.shape[-1]
    z = torch.zeros(depth_map.shape[0], 3, K)                      # (the colour and entropy terms do not touch depth_map)
    out = reference_depth_step(z + torch.arange(K) * 0.1, depth_map, {"loss_entropy": torch.zeros(depth_map.shape[0], K, 1)},
                               torch.zeros(n_batch, 3), target_depth, n_batch, K, 0.0, depth_lambda)
    return out["loss"] - out["loss_nll"], out["depth_loss"]


def test_depth_term_equals_autograd_of_the_reference_lines():
    g = load("g24a_depth_one_call")
    n_c, n_d, lam = int(g["n_colour"]), int(g["n_depth"]), float(g["depth_lambda"])
    depth = T(g["depth_map"]).clone().requires_grad_(True)
    td = T(g["target_depth"])
    term, depth_loss = _reference_depth_lines(depth, td, n_c, lam)
    np.testing.assert_allclose(float(depth_loss.detach()), float(g["depth_loss"]), rtol=1e-6)
    (cot,) = torch.autograd.grad(term, depth)
    assert not cot[:n_c].any()
    rows = depth.detach()[n_c:]
    d_rows, part = TR.depth_term(rows, td, lam, n_d)
    assert d_rows.shape == (n_d, 4) and part.shape == (1,) and d_rows.is_contiguous()
    np.testing.assert_allclose(d_rows.numpy(), cot[n_c:].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(float(part), float(term.detach()), rtol=1e-6)
    # world 2: two half shards, normalised by the step's total - cotangents concatenate, contributions add
    h = n_d // 2
    (d0, p0), (d1, p1) = TR.depth_term(rows[:h], td[:h], lam, n_d), TR.depth_term(rows[h:], td[h:], lam, n_d)
    np.testing.assert_allclose(torch.cat([d0, d1]).numpy(), cot[n_c:].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(float(p0 + p1), float(term.detach()), rtol=1e-6)


# ---- 3. the step composed on the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["g24a_depth_one_call", "g24b_depth_two_calls"])
def test_oracle_depth_step_reproduces_the_reference(name):
    """One oracle render per network call with that call's latents, the entropy cotangent on the first call only, the depth loss on
    the oracle's depth_map: the reference's loss terms and every gradient entry."""
    g = load(name)
    cfg = DC.cfg_of(g)
    p = O.make_params(cfg, int(g["seed"]))
    scal, grads, ents = DC.oracle_depth_step(p, g, DC.t_rand_of(g))
    for c, e in enumerate(ents):
        assert abs(e - float(g["loss_entropy_chunks"][c])) <= 2e-5 * abs(float(g["loss_entropy_chunks"][c])) + 2e-6
    for k in ("loss", "loss_nll", "depth_loss"):
        assert abs(scal[k] - float(g[k])) <= 2e-5 * abs(float(g[k])), k
    assert abs(scal["loss_entropy"] - float(g["loss_entropy"])) <= 2e-5 * abs(float(g["loss_entropy"])) + 2e-6
    n_checked = 0
    for k in p:
        fx = DC.fixture_gradient(g, k)
        if fx is None:
            assert grads[k] is None or not grads[k].any(), k
            continue
        ref, _, scale, norm = fx
        np.testing.assert_allclose(grads[k].double().reshape(-1).numpy(), ref, atol=2e-4 * scale, rtol=1e-3, err_msg=k)
        np.testing.assert_allclose(float(grads[k].double().norm()), norm, rtol=2e-4, err_msg=k)
        n_checked += 1
    assert n_checked >= 30


# ---- 4. key-point rays and the feeder ---------------------------------------------------------------------------------------------------

def test_get_rays_by_coord_is_the_formula_and_meets_get_rays_on_pixels():
    rng = np.random.default_rng(4)
    H, W, focal = 20, 30, 25.5
    c2w = np.concatenate([np.linalg.qr(rng.standard_normal((3, 3)))[0], rng.uniform(-1, 1, (3, 1))], 1)
    coords = rng.uniform(0, [W - 1, H - 1], (50, 2))
    ro, rd = api.get_rays_by_coord(H, W, focal, torch.tensor(c2w), torch.tensor(coords))
    assert ro.dtype == rd.dtype == torch.float32 and ro.shape == rd.shape == (50, 3)
    dirs = np.stack([(coords[:, 0] - W * .5) / focal, -(coords[:, 1] - H * .5) / focal, -np.ones(50)], -1)
    np.testing.assert_allclose(rd.numpy(), (dirs[:, None, :] * c2w[:3, :3]).sum(-1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ro.numpy(), np.broadcast_to(c2w[:, 3], (50, 3)), rtol=1e-6)
    # integer coordinates (x, y) = (column, row): the pixel's ray of get_rays
    o_all, d_all = O.get_rays(H, W, focal, torch.tensor(c2w, dtype=torch.float32))
    xy = np.stack([rng.integers(0, W, 40), rng.integers(0, H, 40)], -1)
    ro, rd = api.get_rays_by_coord(H, W, focal, torch.tensor(c2w), torch.tensor(xy))
    np.testing.assert_allclose(rd.numpy(), d_all[xy[:, 1], xy[:, 0]].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ro.numpy(), o_all[xy[:, 1], xy[:, 0]].numpy(), rtol=1e-6)


def _depth_gts(rng, n_views, H, W):
    out = []
    for v in range(n_views):
        n = 20 + 7 * v
        out.append(dict(coord=rng.uniform(0, [W - 1, H - 1], (n, 2)), depth=rng.uniform(2, 6, n), weight=rng.uniform(0, 1, n)))
    return out


def test_depth_ray_pool_table_layout():
    """RUN:890-900: per key point origin, direction, depth x3, weight x3, the training views concatenated in order."""
    rng = np.random.default_rng(8)
    H, W, focal = 20, 30, 25.5
    gts = _depth_gts(rng, 4, H, W)
    poses = rng.standard_normal((4, 3, 5)).astype(np.float32)
    i_train = [0, 2, 3]
    pool = DepthRayPool(gts, poses, H, W, focal, i_train, N_depth=16, shuffle=False)
    M = sum(len(gts[v]["depth"]) for v in i_train)
    assert pool.rays_depth.shape == (M, 4, 3) and len(pool) == M and pool.N_depth == 16 and pool.rays_depth.dtype == torch.float32
    row = 0
    for v in i_train:
        n = len(gts[v]["depth"])
        ro, rd = api.get_rays_by_coord(H, W, focal, torch.tensor(poses[v, :3, :4]), torch.tensor(gts[v]["coord"]))
        blk = pool.rays_depth[row:row + n]
        assert torch.equal(blk[:, 0], ro) and torch.equal(blk[:, 1], rd)
        for j in range(3):
            np.testing.assert_array_equal(blk[:, 2, j].numpy(), gts[v]["depth"].astype(np.float32))
            np.testing.assert_array_equal(blk[:, 3, j].numpy(), gts[v]["weight"].astype(np.float32))
        row += n
    rays, td, w = pool.next_batch()
    assert rays.shape == (2, 16, 3) and td.shape == w.shape == (16,)
    assert torch.equal(rays[0], pool.rays_depth[:16, 0]) and torch.equal(td, pool.rays_depth[:16, 2, 0]) and torch.equal(w, pool.rays_depth[:16, 3, 0])
    # a colour pool is untouched by the shared feeder: same attributes, same two-tuple
    cp = RayPool.from_rays_rgb(torch.arange(90, dtype=torch.float32).reshape(10, 3, 3), 4, shuffle=False)
    r, t = cp.next_batch()
    assert r.shape == (2, 4, 3) and t.shape == (4, 3) and cp.i_batch == 4 and len(cp) == 10


_M, _ND, _STEPS = 300, 128, 7


def _table():
    return torch.arange(_M * 12, dtype=torch.float32).reshape(_M, 4, 3)


def test_depth_ray_pool_windows_and_reshuffle_one_process():
    """RUN:966-977 on 300 rows with N_depth = 128: windows [0,128), [128,256), the short [256,300), then a re-shuffle and [0,128)."""
    pool = DepthRayPool.from_rays_depth(_table(), _ND, seed=5)
    first = pool.rays_depth.clone()
    assert sorted(first[:, 0, 0].tolist()) == _table()[:, 0, 0].tolist() and not torch.equal(first, _table())
    sizes, cursors = [], []
    for step in range(4):
        before = pool.rays_depth
        rays, td, w = pool.next_batch()
        sizes.append(td.shape[0])
        cursors.append((pool.epoch, pool.i_batch))
        lo = step * _ND if step < 3 else 0
        assert torch.equal(td, before[lo:lo + td.shape[0], 2, 0]) and torch.equal(rays, before[lo:lo + td.shape[0], :2].transpose(0, 1))
        assert torch.equal(w, before[lo:lo + td.shape[0], 3, 0])
    assert sizes == [128, 128, 44, 128] and cursors == [(0, 128), (0, 256), (1, 0), (1, 128)]
    assert not torch.equal(pool.rays_depth, first) and sorted(pool.rays_depth[:, 0, 0].tolist()) == _table()[:, 0, 0].tolist()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _depth_pool_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)
    pool = DepthRayPool.from_rays_depth(_table(), _ND // world, rank=rank, world=world, sync="broadcast",
                                        generator=torch.Generator().manual_seed(77 + rank))
    out = []
    for _ in range(_STEPS):
        rays, td, w = pool.next_batch()
        out.append((rays.clone().numpy(), td.clone().numpy(), w.clone().numpy(), pool.epoch, pool.i_batch))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_depth_ray_pool_two_ranks_union_of_shards_is_the_one_process_batch():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_depth_pool_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    one = DepthRayPool.from_rays_depth(_table(), _ND, generator=torch.Generator().manual_seed(77))
    for step in range(_STEPS):
        rays1, td1, w1 = one.next_batch()
        (r0, t0, w0, ep0, ib0), (r1, t1, w1_, ep1, ib1) = got[0][step], got[1][step]
        assert (ep0, ib0) == (ep1, ib1) == (one.epoch, one.i_batch), step
        assert t0.shape[0] == t1.shape[0] == td1.shape[0] // 2 and t0.shape[0] in (_ND // 2, (_M % _ND) // 2)
        np.testing.assert_array_equal(np.concatenate([r0, r1], 1), rays1.numpy())
        np.testing.assert_array_equal(np.concatenate([t0, t1]), td1.numpy())
        np.testing.assert_array_equal(np.concatenate([w0, w1_]), w1.numpy())
    assert one.epoch == 2


# ---- 5. the C ABI did not grow -------------------------------------------------------------------------------------------------------------

def test_the_c_abi_still_declares_the_same_34_names():
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bCFNERF_API\b[^;(]*?\b(cfnerf_[a-z_0-9]+)\s*\(", stripped))
    assert len(declared) == 34 and declared == set(L.EXPORTS)
    vmap = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "cf-nerf_amd", "csrc", "cfnerf_exports.map")).read(), flags=re.S)
    assert vmap.split() == ["{", "global:", "cfnerf_*;", "local:", "*;", "};"]        # the header's names and nothing else, as before
    assert not any("depth_lambda" in s or "depth_term" in s for s in declared)


def test_trainer_signature_names_the_depth_arguments():
    """step() used to filter its keywords and forward_backward to swallow the rest: depth arguments must be named parameters of both."""
    import inspect
    fb = inspect.signature(TR.Trainer.forward_backward).parameters
    assert "depth_rays" in fb and "target_depth" in fb and fb["depth_rays"].default is None
    assert inspect.signature(TR.Trainer.__init__).parameters["depth_lambda"].default == 0.0
    src = inspect.getsource(TR.Trainer.step)
    assert '"depth_rays"' in src and '"target_depth"' in src
