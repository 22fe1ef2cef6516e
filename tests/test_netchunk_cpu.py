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
