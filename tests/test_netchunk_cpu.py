"""Per-netchunk latents (CFNERF_F_EPS_ROWS) on the CPU: the G23 fixtures of the real reference, the draw order and row layout of
the host helpers, the "per-netchunk = chunk-weighted sum" composition on the oracle, and the flag in the header.  No kernel runs."""
import glob
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import api
from cfnerf_amd import latents as LT
from oracle import cfnerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = os.path.join(ROOT, "tests", "golden", "netchunk")
T = lambda a: torch.tensor(np.asarray(a))


def _digest(v):
    return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16] + ":" + str(v.dtype) + str(list(v.shape))


def _manifest(path=NC):
    with open(os.path.join(path, "MANIFEST.json")) as f:
        return json.load(f)


def load(name):
    return dict(np.load(os.path.join(NC, name + ".npz"), allow_pickle=False))


def test_netchunk_fixtures_match_their_manifest():
    man = _manifest()
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(NC, "*.npz")))
    assert names == sorted(man)
    for name in names:
        g = load(name)
        assert sorted(g) == sorted(man[name]), name
        for k, v in g.items():
            assert _digest(v) == man[name][k], (name, k)


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="the reference only exists in the build container")
def test_committed_netchunk_generator_reproduces_the_fixtures(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_netchunk.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _manifest(str(tmp_path)) == _manifest()


def test_draw_train_randomness_is_the_reference_draw_order():
    """G23a: 6 rays in cuts of 4, netchunk = 2 rays, raw_noise_std = 1: the reference consumed t_rand, two latent pairs, a noise
    draw, then t_rand, one pair, a noise draw.  The helper draws the same numbers from the same seed, bit for bit."""
    g = load("g23a_netchunk_draw_order")
    kinds = list(g["draw_kinds"])
    assert kinds == ["rand", "normal", "normal", "normal", "normal", "randn", "rand", "normal", "normal", "randn"]
    torch.manual_seed(int(g["draw_seed"]))
    t_rand, eps = api.draw_train_randomness(6, 128, int(g["K"]), int(g["chunk"]), int(g["netchunk"]), float(g["perturb"]),
                                            float(g["raw_noise_std"]))
    np.testing.assert_array_equal(t_rand.numpy(), np.concatenate([g["draw0"], g["draw6"]], 0))
    pairs = [(1, 2), (3, 4), (7, 8)]
    assert eps.shape == (3, 4, 4)
    for c, (ia, ir) in enumerate(pairs):
        np.testing.assert_array_equal(eps[c, :, 3:].numpy(), g[f"draw{ia}"])
        np.testing.assert_array_equal(eps[c, :, :3].numpy(), g[f"draw{ir}"])
    # and the generator stands where the reference left it (the thrown-away noise draws were made)
    torch.manual_seed(int(g["draw_seed"]))
    api.draw_train_randomness(6, 128, 4, 4, 256, 1.0, 1.0)
    after = torch.rand(3)
    torch.manual_seed(int(g["draw_seed"]))
    for k, name in zip(kinds, range(len(kinds))):
        v = g[f"draw{name}"]
        {"rand": torch.rand, "randn": torch.randn}.get(k, lambda *s: torch.empty(*s).normal_())(*v.shape)
    np.testing.assert_array_equal(after.numpy(), torch.rand(3).numpy())


def test_netchunk_eps_rows_layout_of_ragged_cuts():
    """Cuts of `chunk` rays restart batchify's count; a ragged last network call of a cut still draws its own pair."""
    C = api.netchunk_count(10, 4, 8, chunk=5)        # cuts of 5 rays = 20 points -> calls of 2 rays: 3 + 3 pairs
    assert C == 6
    chunks = torch.arange(C, dtype=torch.float32)[:, None, None].expand(C, 2, 4).contiguous()
    rows = api.netchunk_eps_rows(chunks, 10, 4, 8, chunk=5)
    assert rows.shape == (10, 2, 4)
    assert rows[:, 0, 0].tolist() == [0, 0, 1, 1, 2, 3, 3, 4, 4, 5]
    # one cut (chunk None or larger than N)
    assert api.netchunk_eps_rows(chunks[:5], 10, 4, 8)[:, 0, 0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # point rows of the unfused seam
    assert api.netchunk_eps_point_rows(chunks[:3], 5, 2)[:, 0, 0].tolist() == [0, 0, 1, 1, 2]
    with pytest.raises(ValueError):
        api.netchunk_eps_rows(chunks[:4], 10, 4, 8, chunk=5)
    with pytest.raises(NotImplementedError):
        api.netchunk_eps_rows(chunks, 10, 3, 8, chunk=5)
    # the reference's defaults: 65536 points = 512 rays of 128 samples; N_rand 8192 in cuts of 32768 rays -> 16 pairs
    assert api.netchunk_count(8192, 128, 65536, 1024 * 32) == 16
    assert api.netchunk_count(1024, 128, 65536, 8192) == 2


def test_oracle_per_chunk_steps_compose_to_the_reference_c2_batch():
    """G23b: the oracle run once per netchunk with that chunk's latents, combined with weights N_c / N, is the reference's full
    batch - loss, entropy and the sampled gradients (what the kernels' point-weighted entropy and ray rows must reproduce)."""
    g = load("g23b_netchunk_c2")
    cfg = O.OracleCfg(netwidth=int(g["netwidth"]), K_samples=int(g["K"]))
    p = O.make_params(cfg, int(g["seed"]))
    n = g["rays"].shape[1]
    t_np = np.random.default_rng(int(g["t_rand_seed"])).uniform(0, 1, (n, 128)).astype(np.float32)
    assert hashlib.sha256(t_np.tobytes()).hexdigest() == str(g["t_rand_sha256"])
    rays = T(g["rays"])
    packed = O.pack_rays(int(g["H"]), int(g["W"]), float(g["focal"]), rays[0], rays[1], False, float(g["near"]), float(g["far"]))
    per = int(g["netchunk"]) // 128
    loss = ent = 0.
    grads = {}
    for c in range(2):
        s = slice(c * per, (c + 1) * per)
        w = per / n
        scal, gr, _ = O.train_step(p, packed[s], T(g["target"])[s], cfg, T(g["eps_alpha"][c]), T(g["eps_rgb"][c]), T(t_np)[s], float(g["beta1"]))
        assert abs(scal["loss_entropy"] - float(g["loss_entropy_chunks"][c])) <= 2e-5 * abs(float(g["loss_entropy_chunks"][c])) + 2e-6
        loss += w * scal["loss"]
        ent += w * scal["loss_entropy"]
        for k, v in gr.items():
            if v is not None:
                grads[k] = grads.get(k, 0) + w * v.double()
    assert abs(loss - float(g["loss"])) <= 2e-5 * abs(float(g["loss"]))
    assert abs(ent - float(g["loss_entropy"])) <= 2e-5 * abs(float(g["loss_entropy"])) + 2e-6
    n_checked = 0
    for k in p:
        if ("gradsample." + k) not in g:
            assert k not in grads or not grads[k].any(), k
            continue
        idx = T(g["gradidx." + k]).long()
        scale = max(1e-7, float(g["gradabsmax." + k]))
        np.testing.assert_allclose(grads[k].reshape(-1)[idx].numpy(), g["gradsample." + k], atol=2e-4 * scale, rtol=1e-3, err_msg=k)
        np.testing.assert_allclose(float(grads[k].norm()), float(g["gradnorm." + k]), rtol=2e-4, err_msg=k)
        n_checked += 1
    assert n_checked >= 30


def test_eps_rows_flag_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    m = re.search(r"CFNERF_F_EPS_ROWS\s*=\s*1\s*<<\s*(\d+)", hdr)
    assert m and (1 << int(m.group(1))) == L.F_EPS_ROWS == 16
    assert L.F_EPS_ROWS not in (L.F_TRAIN, L.F_LINDISP, L.F_WHITE_BKGD, L.F_STASH)
    stripped = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bCFNERF_API\b[^;(]*?\b(cfnerf_[a-z_0-9]+)\s*\(", stripped))
    assert len(declared) == 34 and declared == set(L.EXPORTS)


def test_latent_draws_option_defaults_to_launch():
    assert api.default_args().latent_draws == "launch"
    assert api.LATENT_DRAWS == ("launch", "netchunk")


# ---- latents.train_latents: the one resolver behind render_rays, NeRF_Flows.forward and Trainer.forward_backward -------------------


def _pair_as_the_model_drew_it(K):
    """One launch's pair the way NeRF_Flows.draw_eps spelled it before latents.py: eps_alpha, then eps_rgb (MOD:234,246), rgb | alpha."""
    ea = torch.empty([K, 1]).normal_()
    er = torch.empty([K, 3]).normal_()
    return torch.cat([er, ea], -1)


def _same(new, old):
    """(t_rand, eps) of the resolver against the building blocks, bit for bit, and the generator stands where they left it."""
    (t_new, e_new, nxt_new), (t_old, e_old, nxt_old) = new, old
    assert (t_new is None) == (t_old is None)
    if t_old is not None:
        assert t_new.dtype == t_old.dtype and torch.equal(t_new, t_old)
    assert e_new.dtype == torch.float32 and e_new.shape == e_old.shape and torch.equal(e_new, e_old)
    assert torch.equal(nxt_new, nxt_old)


@pytest.mark.parametrize("own_t_rand", [False, True])
def test_resolver_launch_mode_implicit_is_t_rand_then_one_pair(own_t_rand):
    """render_rays' shape (no t_rand of its own: the CPU generator's, BEFORE the pair) and the Trainer's (it has its own: only the pair)."""
    N, S, K = 6, 128, 4
    torch.manual_seed(77)
    t_old = None if own_t_rand else torch.rand([N, S])
    old = (t_old, _pair_as_the_model_drew_it(K), torch.rand(3))
    torch.manual_seed(77)
    t, eps, pairs = LT.train_latents("launch", None, N=N, S=S, K=K, netchunk=256, chunk=4, perturb=1.0, raw_noise_std=1.0, own_t_rand=own_t_rand)
    assert pairs is None and eps.shape == (K, 4)
    _same((t, eps, torch.rand(3)), old)
    torch.manual_seed(77)                               # perturb = 0: no t_rand either way
    t, eps, _ = LT.train_latents("launch", None, N=N, S=S, K=K, netchunk=256, own_t_rand=False)
    assert t is None
    torch.manual_seed(77)
    assert torch.equal(eps, _pair_as_the_model_drew_it(K))


@pytest.mark.parametrize("own_t_rand", [False, True])
def test_resolver_netchunk_mode_implicit_on_ragged_cuts_is_the_reference_order(own_t_rand):
    """The G23a shape (6 rays, cuts of 4, netchunk = 2 rays, raw_noise_std > 0): draw_train_randomness + netchunk_eps_rows, and through
    them the reference's recorded draws; the t_rand comes with the pairs whether or not the caller has one."""
    g = load("g23a_netchunk_draw_order")
    N, S, K, chunk, netchunk = 6, 128, int(g["K"]), int(g["chunk"]), int(g["netchunk"])
    torch.manual_seed(int(g["draw_seed"]))
    t_old, chunks = api.draw_train_randomness(N, S, K, chunk, netchunk, float(g["perturb"]), float(g["raw_noise_std"]))
    old = (t_old, api.netchunk_eps_rows(chunks, N, S, netchunk, chunk), torch.rand(3))
    torch.manual_seed(int(g["draw_seed"]))
    t, eps, pairs = LT.train_latents("netchunk", None, N=N, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=float(g["perturb"]),
                                     raw_noise_std=float(g["raw_noise_std"]), own_t_rand=own_t_rand)
    _same((t, eps, torch.rand(3)), old)
    assert torch.equal(pairs, chunks) and eps.shape == (N, K, 4)
    np.testing.assert_array_equal(t.numpy(), np.concatenate([g["draw0"], g["draw6"]], 0))
    for ray, (ia, ir) in zip(range(N), [(1, 2), (1, 2), (3, 4), (3, 4), (7, 8), (7, 8)]):      # rays 0-3: first cut's two calls; 4-5: the second cut's one
        np.testing.assert_array_equal(eps[ray, :, 3:].numpy(), g[f"draw{ia}"])
        np.testing.assert_array_equal(eps[ray, :, :3].numpy(), g[f"draw{ir}"])


def test_resolver_trainer_shape_is_the_global_batch_and_a_rank_slices_its_rows():
    """Trainer.forward_backward: N * world rays, no raw_noise_std, its own t_rand; rank r keeps rows [r N, (r + 1) N)."""
    N, world, S, K, chunk, netchunk = 4, 2, 4, 3, 5, 8
    torch.manual_seed(5)
    t_old, chunks = api.draw_train_randomness(N * world, S, K, chunk, netchunk, 1.0)
    old = (t_old, api.netchunk_eps_rows(chunks, N * world, S, netchunk, chunk), torch.rand(3))
    torch.manual_seed(5)
    t, eps, pairs = LT.train_latents("netchunk", None, N=N * world, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=1.0)
    _same((t, eps, torch.rand(3)), old)
    assert pairs.shape == (api.netchunk_count(N * world, S, netchunk, chunk), K, 4)
    # the pairs as they arrive in the all-reduce tail: explicit, nothing drawn
    torch.manual_seed(5)
    nxt = torch.rand(3)
    torch.manual_seed(5)
    t2, eps2, pairs2 = LT.train_latents("netchunk", chunks, N=N * world, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=1.0)
    assert t2 is None and pairs2 is chunks and torch.equal(eps2, eps) and torch.equal(torch.rand(3), nxt)
    for r in range(world):
        assert torch.equal(eps2[r * N:(r + 1) * N], old[1][r * N:(r + 1) * N])


@pytest.mark.parametrize("mode", api.LATENT_DRAWS)
def test_resolver_explicit_latents_mean_the_same_in_both_modes_and_consume_no_draw(mode):
    """An explicit [K,*] set is one set (also in netchunk mode), explicit [C,K,*] pairs are rows (also in launch mode)."""
    N, S, K, chunk, netchunk = 10, 4, 2, 5, 8
    rng = np.random.default_rng(3)
    torch.manual_seed(9)
    nxt = torch.rand(3)
    ea, er = (torch.tensor(rng.standard_normal((K, d)), dtype=torch.float32) for d in (1, 3))
    torch.manual_seed(9)
    t, eps, pairs = LT.train_latents(mode, LT.pack(ea, er), N=N, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=1.0, raw_noise_std=1.0)
    assert t is None and pairs is None
    _same((None, eps, torch.rand(3)), (None, torch.cat([er, ea], -1), nxt))
    C = api.netchunk_count(N, S, netchunk, chunk)
    ea, er = (torch.tensor(rng.standard_normal((C, K, d)), dtype=torch.float32) for d in (1, 3))
    chunks = torch.cat([er, ea], -1)
    torch.manual_seed(9)
    t, eps, pairs = LT.train_latents(mode, LT.pack(ea, er), N=N, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=1.0, raw_noise_std=1.0)
    assert t is None and torch.equal(pairs, chunks)
    _same((None, eps, torch.rand(3)), (None, api.netchunk_eps_rows(chunks, N, S, netchunk, chunk), nxt))
    # ... and with no t_rand of the caller's the CPU generator yields one [N,S], nothing else
    torch.manual_seed(9)
    t_old = torch.rand([N, S])
    nxt = torch.rand(3)
    torch.manual_seed(9)
    t, eps, _ = LT.train_latents(mode, chunks, N=N, S=S, K=K, netchunk=netchunk, chunk=chunk, perturb=1.0, own_t_rand=False)
    _same((t, eps, torch.rand(3)), (t_old, api.netchunk_eps_rows(chunks, N, S, netchunk, chunk), nxt))
    with pytest.raises(ValueError):
        LT.train_latents(mode, chunks[:-1], N=N, S=S, K=K, netchunk=netchunk, chunk=chunk)
    with pytest.raises(ValueError):
        LT.pack(ea, er[0])
    with pytest.raises(ValueError):
        LT.pack(ea, None)
    assert LT.pack(None, None) is None


def test_resolver_points_mode_with_a_ragged_last_network_call():
    """NeRF_Flows.forward: P points as N = P rays of one sample, no cuts, no jitter.  Netchunk mode draws ceil(P / netchunk) pairs (each
    eps_alpha then eps_rgb) and nothing else; launch mode one pair."""
    P, K, netchunk = 5, 4, 2
    torch.manual_seed(21)
    chunks = torch.stack([_pair_as_the_model_drew_it(K) for _ in range(3)])
    old = (None, api.netchunk_eps_point_rows(chunks, P, netchunk), torch.rand(3))
    torch.manual_seed(21)
    t, eps, pairs = LT.train_latents("netchunk", None, N=P, S=1, K=K, netchunk=netchunk)
    _same((t, eps, torch.rand(3)), old)
    assert eps.shape == (P, K, 4) and eps[:, 0, 0].tolist() == chunks[[0, 0, 1, 1, 2], 0, 0].tolist() and torch.equal(pairs, chunks)
    torch.manual_seed(21)
    old = (None, _pair_as_the_model_drew_it(K), torch.rand(3))
    torch.manual_seed(21)
    t, eps, _ = LT.train_latents("launch", None, N=P, S=1, K=K, netchunk=netchunk)
    _same((t, eps, torch.rand(3)), old)
    with pytest.raises(ValueError):
        api.netchunk_eps_point_rows(chunks[:2], P, netchunk)
    with pytest.raises(ValueError):
        LT.train_latents("per_ray", None, N=P, S=1, K=K, netchunk=netchunk)


def test_check_rows_counts_the_rows_of_a_launch():
    assert LT.check_rows(torch.zeros(4, 4), 7, "rays") is False
    assert LT.check_rows(torch.zeros(7, 4, 4), 7, "rays") is True
    with pytest.raises(ValueError, match="latent rows for 4 points, the launch has 16"):
        LT.check_rows(torch.zeros(4, 4, 4), 16, "points")
