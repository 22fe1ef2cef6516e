"""No GPU: sampling through an occupancy grid - the depth warp (``api.warp_from_bins``) against its fp64 numpy restatement, the bin rule and
``pad`` against theirs, the probe cell rule on hand-made points, and the signatures and refusals of the new entry points."""
import inspect

import numpy as np
import pytest
import torch

from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E
from cfnerf_amd import train as TR

from warp_common import check_warp


def _case(bins, S, jitter, lindisp, seed, N=24):
    """(z_plain [N,S] fp32 from the sampling lines RUN:510-532 in torch, near [N], far [N], mask [N,bins]): rows 0 / 1 empty / full, row 2
    one occupied bin, row 3 all but one, the rest random at densities from sparse to dense."""
    g = torch.Generator().manual_seed(seed)
    near = 0.5 + 1.5 * torch.rand(N, generator=g)
    far = near + 1.0 + 3.0 * torch.rand(N, generator=g)
    rays = torch.zeros(N, 11)
    rays[:, 6], rays[:, 7] = near, far
    t_rand = torch.rand(N, S, generator=g) if jitter else None
    z_plain, _ = A.sample_points_reference(rays, torch.linspace(0., 1., S), t_rand, lindisp)
    mask = torch.rand(N, bins, generator=g) < torch.linspace(0.05, 0.95, N)[:, None]
    mask[0], mask[1] = False, True
    mask[2] = False
    mask[2, bins // 3] = True
    mask[3] = True
    mask[3, bins // 2] = False
    return z_plain.contiguous(), near, far, mask


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("S", [16, 65])
@pytest.mark.parametrize("bins", [8, 512])
def test_warp_against_the_fp64_reference(bins, S, jitter, lindisp):
    z_plain, near, far, mask = _case(bins, S, jitter, lindisp, seed=1000 * bins + 10 * S + 2 * jitter + lindisp)
    z, n = A.warp_from_bins(z_plain, near, far, mask)
    assert set(n.tolist()) >= {0, 1, bins - 1, bins}
    warped = check_warp(z, n, z_plain, near, far, mask, what=f"bins={bins} S={S} jitter={jitter} lindisp={lindisp}")
    assert int((~warped).sum()) >= 2 and not torch.equal(z[torch.tensor(warped)], z_plain[torch.tensor(warped)])
    z2, n2 = A.warp_from_bins(z_plain, near, far, mask)
    assert torch.equal(z2, z) and torch.equal(n2, n)                              # two calls are bit-equal


def test_warp_uses_the_whole_sample_budget_inside_the_occupied_bins():
    """one occupied run in the middle of the ray: the first sample sits at its start, the last at its end, equal spacing in between"""
    bins, S = 8, 9
    mask = torch.zeros(1, bins, dtype=torch.bool)
    mask[0, 2:4] = True
    z_plain = torch.linspace(2., 6., S)[None]
    z, n = A.warp_from_bins(z_plain, torch.tensor([2.]), torch.tensor([6.]), mask)
    assert int(n) == 2
    np.testing.assert_allclose(z[0].numpy(), np.linspace(3., 4., S), rtol=0, atol=1e-6)


def _probe_rows():
    B = 8
    rows = np.zeros((6, 2 * B + 1), dtype=bool)
    rows[1] = True                                   # the full row
    rows[2, 5] = True                                # a single middle probe: bin 2 alone
    rows[3, 6] = True                                # a single end probe: the two bins that share it (2 and 3)
    rows[4, 0::2] = True                             # alternating, ends: every bin
    rows[5, 3::4] = True                             # alternating, every other middle: bins 1, 3, 5, 7
    return B, rows


@pytest.mark.parametrize("pad", [0, 1, 2, 20])
def test_bin_rule_and_pad_against_numpy(pad):
    B, rows = _probe_rows()
    got = A.bins_from_probes(torch.tensor(rows), pad)
    want = A.bins_from_probes_reference(rows, pad)
    assert got.dtype == torch.bool and tuple(got.shape) == (6, B)
    assert np.array_equal(got.numpy(), want)
    assert not want[0].any() and want[1].all() and want[4].all()
    if pad == 0:
        assert list(np.flatnonzero(want[2])) == [2] and list(np.flatnonzero(want[3])) == [2, 3] and list(np.flatnonzero(want[5])) == [1, 3, 5, 7]
    if pad == 1:
        assert list(np.flatnonzero(want[2])) == [1, 2, 3] and list(np.flatnonzero(want[3])) == [1, 2, 3, 4] and want[5].all()
    if pad == 20:
        assert want[2].all() and not want[0].any()
    rng = np.random.default_rng(pad)
    rnd = rng.random((9, 2 * 33 + 1)) < 0.1
    assert np.array_equal(A.bins_from_probes(torch.tensor(rnd), pad).numpy(), A.bins_from_probes_reference(rnd, pad))


def test_probe_cell_rule_on_hand_made_points():
    mask = torch.zeros(2, 2, 2, dtype=torch.bool)
    mask[1, 0, 1] = True
    grid = E.OccupancyGrid.from_mask(mask, (0., 0., 0.), (2., 2., 2.))
    pts = torch.tensor([[[1.5, 0.5, 1.5], [1.0, 0.0, 1.0], [0.999, 0.5, 1.5], [1.5, 1.0, 1.5], [2.0, 0.5, 1.5], [-0.1, 0.5, 1.5],
                         [float("nan"), 0.5, 1.5]]])
    #                    inside the cell, on its lower faces (its own), below it, on its upper y face (the next cell's), on the box's upper face
    #                    and beyond its lower face (outside), not a number (outside)
    assert A.probe_occupancy_reference(pts, grid, "cull")[0].tolist() == [True, True, False, False, False, False, False]
    assert A.probe_occupancy_reference(pts, grid, "keep")[0].tolist() == [True, True, False, False, True, True, True]
    full = E.OccupancyGrid.from_mask(torch.ones(3, 11, 2, dtype=torch.bool), (0., 0., 0.), (2., 2., 2.))           # (66 cells: three words)
    assert bool(A.probe_occupancy_reference(torch.rand(4, 9, 3, generator=torch.Generator().manual_seed(0)) * 2, full).all())


def test_signatures_and_refusals():
    fb = inspect.signature(TR.Trainer.forward_backward).parameters
    assert "occupancy" in fb and fb["occupancy"].default is None and fb["occupancy"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert '"occupancy"' in inspect.getsource(TR.Trainer.step)
    assert list(inspect.signature(E.render_uncertainty).parameters)[-2:] == ["occupancy", "_ignored"]
    assert list(inspect.signature(A.render_rays_warped).parameters) == [
        "ray_batch", "network_fn", "sampler", "is_train", "lindisp", "perturb", "white_bkgd", "t_rand", "eps_alpha", "eps_rgb", "t_vals",
        "retweights", "chunk"]
    assert list(inspect.signature(A.warp_z_vals).parameters) == ["ray_batch", "sampler", "t_vals", "t_rand", "lindisp"]
    grid = E.OccupancyGrid.from_mask(torch.ones(2, 2, 2, dtype=torch.bool), (0, 0, 0), (1, 1, 1))
    s = grid.sampler()
    assert isinstance(s, E.OccupancySampler) and (s.grid, s.bins, s.pad, s.outside) == (grid, 512, 1, "cull")
    s = grid.sampler(bins=4096, pad=0, outside="keep")
    assert (s.bins, s.pad, s.outside) == (4096, 0, "keep") and E.OccupancySampler(grid, bins=1).bins == 1
    for bad in (0, 4097, -3, 2.5):
        with pytest.raises(ValueError, match="bins"):
            E.OccupancySampler(grid, bins=bad)
    with pytest.raises(ValueError, match="pad"):
        E.OccupancySampler(grid, pad=-1)
    with pytest.raises(ValueError, match="outside"):
        E.OccupancySampler(grid, outside=1)
    with pytest.raises(ValueError, match="acc_map"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="ext", occupancy=grid.sampler())
    # the probe buffers of one launch stay under 256 MiB at 24 bytes per probe
    for bins in (1, 512, 4096):
        c = A.warp_probe_chunk(bins)
        assert c >= 1 and c * (2 * bins + 1) * 24 <= 256 << 20 < (c + 1) * (2 * bins + 1) * 24
