"""Shared by tests/test_warp_cpu.py and tests/test_hip_warp.py: the properties every warped depth set must have, judged in fp64 numpy."""
import numpy as np
import torch

from cfnerf_amd import api as A

# fp32 error of target = f n for n <= 4096 is about 2.5e-4 bins (a few ulp of a number below 4096); the bound gives that a margin of four
LEN_TOL = 1e-3


def occupied_length_before(z, near, far, mask):
    """fp64: the number of occupied bins (fractions included) of every ray that lie in front of depth z [N,S]"""
    B = mask.shape[1]
    u = np.clip((z - near[:, None]) / (far - near)[:, None] * B, 0.0, float(B))
    b = np.minimum(np.floor(u).astype(np.int64), B - 1)
    csum = np.concatenate([np.zeros((mask.shape[0], 1)), np.cumsum(mask, 1)], 1)
    return np.take_along_axis(csum, b, 1) + np.take_along_axis(mask, b, 1) * (u - b)


def check_warp(z, n, z_plain, near, far, mask, what=""):
    """``z [N,S]`` / ``n [N]`` (fp32 / int32 tensors, any device) are the warp of ``z_plain`` through the bin ``mask [N,B]``: the reference's
    counts; the occupied length in front of every sample is f n within LEN_TOL bins; every sample lies in the closed interval of an occupied
    bin; depths do not decrease; rays with no or with every bin occupied keep the bits of ``z_plain``.  Returns the rows that were warped."""
    z, n, z_plain, near, far, mask = (t.detach().cpu() for t in (z, n, z_plain, near, far, mask))
    bins = mask.shape[1]
    assert z.dtype == torch.float32 and n.dtype == torch.int32 and tuple(z.shape) == tuple(z_plain.shape), what
    zp64, nr64, fr64, m = z_plain.double().numpy(), near.double().numpy(), far.double().numpy(), mask.numpy()
    z_ref, n_ref = A.warp_z_vals_reference(zp64, nr64, fr64, m)
    assert np.array_equal(n.numpy(), n_ref) and np.array_equal(n_ref, m.sum(1)), what
    warped = (n_ref > 0) & (n_ref < bins)
    same = torch.tensor(~warped)
    assert torch.equal(z[same], z_plain[same]), what                              # bit for bit
    assert bool((z[:, 1:] >= z[:, :-1]).all()) and bool((z_plain[:, 1:] >= z_plain[:, :-1]).all()), what
    if not warped.any():
        return warped
    # depths are not compared directly: one ulp of `target` at an integer moves a sample across a gap.  The occupied length in front of a
    # sample, in bin units, is continuous there: it must be f n, for the depths under test and (to fp64) for the reference's own
    f = np.clip((zp64 - nr64[:, None]) / (fr64 - nr64)[:, None], 0.0, 1.0)
    want = (f * n_ref[:, None])[warped]
    assert np.abs(occupied_length_before(z_ref, nr64, fr64, m)[warped] - want).max() < 1e-9, what
    err = np.abs(occupied_length_before(z.double().numpy(), nr64, fr64, m)[warped] - want).max()
    print(f"{what}: occupied-length error {err:.3e} bins")
    assert err < LEN_TOL, (what, err)
    # every depth lies in the closed interval of an occupied bin (to the rounding of z itself: 4 ulp of the ray's far end, in bin units)
    zz = z.double().numpy()[warped]
    slack = (4 * np.spacing(far.numpy()).astype(np.float64) * bins / (fr64 - nr64))[warped][:, None]
    u = (zz - nr64[warped][:, None]) / (fr64 - nr64)[warped][:, None] * bins
    mw = m[warped]
    lo_bin = np.clip(np.floor(u + slack).astype(np.int64), 0, bins - 1)          # the bin z is in, or - on a boundary - the one above ...
    hi_bin = np.clip(np.ceil(u - slack).astype(np.int64) - 1, 0, bins - 1)       # ... or the one below
    assert (np.take_along_axis(mw, lo_bin, 1) | np.take_along_axis(mw, hi_bin, 1)).all(), what
    return warped
