"""CPU: the evaluation metrics fused into the eval render (CFNERF_F_KSTATS_EXT) - everything that needs no GPU.

* ``sparsification_curves`` / ``ause_fused`` against the reference-shaped ``sparsification_plot`` / ``ause`` (HLP:382-438);
* the torch restatement of the kernel's two new reductions (tests/eval_metrics_common.py) against the oracle's ``train_loss`` and
  ``np.std * n/(n-1)`` - the GPU tests compare the kernel with that restatement, so it is pinned here to the oracle, which the
  fixtures G15-G18 pin to the reference;
* the flag's value in the Python mirror against the header;
* ``gather_rows`` with the new keys over a world-size-2 gloo group."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from cfnerf_amd import _lib as L
from cfnerf_amd import evaluate as E
from eval_metrics_common import gather_problem, nll_terms, spread
from oracle import cfnerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectors(n, seed):
    """continuous random values: no ties (the existing helper's sort is not stable, so the order of ties is unspecified)"""
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.uniform(0.01, 1, n) ** 2, dtype=torch.float32), torch.tensor(rng.uniform(0.01, 1, n) ** 2, dtype=torch.float32)


@pytest.mark.parametrize("n", [1, 7, 100, 12345])
@pytest.mark.parametrize("ut", ["c", "v"])
@pytest.mark.parametrize("et", ["rmse", "mae"])
def test_sparsification_curves_equal_sparsification_plot(n, ut, et):
    """rtol 1e-5: the only difference is the fp64 against fp32 accumulation of a prefix mean; an empty prefix is nan in both."""
    var, err = _vectors(n, 100 + n)
    a0, b0 = E.sparsification_plot(var, err, uncert_type=ut, err_type=et)
    a1, b1 = E.sparsification_curves(var, err, uncert_type=ut, err_type=et)
    assert a1.shape == (100,) and b1.shape == (100,) and a1.dtype == a0.dtype
    assert np.array_equal(np.isnan(a0), np.isnan(a1)) and np.array_equal(np.isnan(b0), np.isnan(b1))
    assert np.isfinite(a1[0]) and np.isfinite(b1[0])
    np.testing.assert_allclose(a1, a0, rtol=1e-5, atol=0, equal_nan=True)
    np.testing.assert_allclose(b1, b0, rtol=1e-5, atol=0, equal_nan=True)


@pytest.mark.parametrize("et", ["rmse", "mae"])
def test_ause_fused_equals_ause(et):
    for n in (100, 12345):
        var, err = _vectors(n, 7 + n)
        a, b = E.ause(var, err, err_type=et), E.ause_fused(var, err, err_type=et)
        assert abs(a - b) <= 1e-5 * abs(a), (n, a, b)
    assert E.ause_fused(err.clone(), err) < 1e-6                          # perfect uncertainty = the oracle ordering


@pytest.mark.parametrize("K", [2, 4, 32, 128])
def test_restatement_of_the_new_reductions_is_the_oracles(K):
    """The fp64 restatement against (a) the oracle's own loss lines evaluated in fp64 - the same formula, to rounding - and (b) the
    oracle's fp32 evaluation, the reference's arithmetic, at the fp32 tolerance of the path (tests/util_hip.py: atol 1e-5, rtol 1e-4);
    the spread against np.std * n/(n-1) (RUN:1129-1130)."""
    rng = np.random.default_rng(K)
    n = 257
    centre = rng.uniform(0.1, 0.9, (n, 3, 1))
    rgbs = torch.tensor(np.clip(centre + rng.standard_normal((n, 3, K)) * rng.uniform(0.005, 0.2, (n, 3, 1)), 0, 1), dtype=torch.float64)
    gt = torch.tensor(centre[..., 0] + rng.uniform(-0.1, 0.1, (n, 3)), dtype=torch.float64)
    gt[::5] = torch.tensor(rng.uniform(0, 1, gt[::5].shape))                               # some pixels on the + 1e-5 floor
    nll, lik = nll_terms(rgbs, gt)
    assert nll.shape == (n, 3) and float((lik > 1e-3).double().mean()) > 0.5               # the integrand is exercised, not only its floor
    ent = torch.zeros(())
    o64 = O.train_loss(rgbs, gt, ent.double(), K, 0.0)
    assert abs(float(nll.mean()) - float(o64["loss_nll"])) <= 1e-12 * abs(float(o64["loss_nll"])) + 1e-13
    o32 = O.train_loss(rgbs.float(), gt.float(), ent, K, 0.0)
    assert abs(float(nll.mean()) - float(o32["loss_nll"])) <= 1e-5 + 1e-4 * abs(float(o32["loss_nll"]))
    mse = ((rgbs.mean(-1) - gt) ** 2).mean()
    assert abs(float(mse) - float(o64["mse"])) <= 1e-14
    x = torch.tensor(rng.uniform(0, 5, (n, K)), dtype=torch.float64)
    np.testing.assert_allclose(spread(x).numpy(), np.std(x.numpy(), -1) * K / (K - 1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(spread(rgbs).numpy(), np.std(rgbs.numpy(), -1) * K / (K - 1), rtol=1e-12, atol=1e-18)
    # the package's own restatement (used where the per-K maps were asked for anyway) is the same expression
    np.testing.assert_allclose(E.kde_nll(rgbs, gt).numpy(), nll.numpy(), rtol=1e-12, atol=1e-12)


def test_flag_value_in_the_python_mirror_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "cfnerf.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"CFNERF_F_(\w+)\s*=\s*1\s*<<\s*(\d+)", hdr)}
    assert flags["KSTATS_EXT"] == 5 and L.F_KSTATS_EXT == 1 << flags["KSTATS_EXT"]
    for name, bit in flags.items():                                                        # and no two flags share a bit
        assert getattr(L, "F_" + name) == 1 << bit, name
    assert len(set(flags.values())) == len(flags)


def test_gather_rows_carries_the_new_keys_over_unequal_shards():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    import eval_metrics_workers as WK
    procs = [ctx.Process(target=WK.gather_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = q.get(timeout=300)
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    H, W, full = gather_problem()
    assert E.row_shard(H, 0, world) == (0, 4) and E.row_shard(H, 1, world) == (4, 7)      # shards of unequal height
    assert set(got) == set(full) | {"mse", "loss_nll"}
    for k, v in full.items():
        np.testing.assert_array_equal(got[k], v.numpy(), err_msg=k)                        # = the concatenation of the shards
    assert abs(got["loss_nll"] - float(full["nll"].mean())) < 1e-6 and abs(got["mse"] - float(full["sq_err"].mean())) < 1e-7


def test_render_uncertainty_refuses_an_unknown_stats_mode():
    with pytest.raises(ValueError, match="stats"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="all")


def test_stateless_entry_points_refuse_the_flag_by_name():
    """cfnerf_sample_points / cfnerf_sample_pdf check their flags before anything touches a device (the model-bound refusals are GPU tests)."""
    lib = L.lib()
    rc = lib.cfnerf_sample_points(None, None, None, L.F_KSTATS_EXT, 4, 8, None, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "cfnerf_sample_points" in msg and "CFNERF_F_KSTATS_EXT" in msg
    rc = lib.cfnerf_sample_pdf(None, None, None, L.F_KSTATS_EXT, None, None, 4, 8, 2, 4, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "cfnerf_sample_pdf" in msg and "CFNERF_F_KSTATS_EXT" in msg


def test_the_library_carries_the_ext_variants_and_leaves_every_other_kernel_alone():
    """tools/kernel_regs.py of the built library: one EXT variant per (width, branch, precision) in ray mode, none of them with a VGPR
    spill or scratch (the committed table, profiles/r08_kernel_regs.txt, holds the comparison with the parent commit)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], capture_output=True, text=True, check=True).stdout
    ext = [l for l in out.splitlines() if re.match(r"fused_fwd_kernel<\d+, 0, (true|false), [01], false, false, true>", l)]
    assert len(ext) == 32, len(ext)
    for l in ext:
        assert re.search(r"vgpr_spill=\s+0 ", l) and re.search(r"scratch=\s+0 ", l), l
    committed = open(os.path.join(ROOT, "profiles", "r08_kernel_regs.txt")).read()
    assert "(none)" in committed.split("## changed")[1].split("## new")[0]
