"""CPU: the fp64 inverse-CDF bracket of tests/sample_pdf_common.py, before it judges the HIP resampler (tests/test_hip_sample_pdf.py):
the oracle's ``sample_pdf`` passes it - in fp64 with no tolerance at all, in fp32 with the derived constants - on every shape, weight
kind, ``u`` kind and ray geometry of the case list, and four one-line mistakes in the restatement each fail it on most samples."""
import numpy as np
import pytest
import torch

import sample_pdf_common as SP
from oracle import cfnerf_oracle as O


def _inputs(S, Ni, K, seed=0):
    """every (what, z [N,S] fp32, w [N,S,K], u [N,Ni]) of a shape: geometries x weight kinds x u kinds"""
    rng = np.random.default_rng(1000 * S + Ni + seed)
    N = SP.N_RAYS
    for ndc, lindisp, jitter, uniform in SP.geometries(S):
        rays = SP.make_rays(rng, N, ndc)
        tv = SP.make_t_vals(S, uniform)
        tr = torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32) if jitter else None
        z = O.sample_z(rays[:, 6:7], rays[:, 7:8], tv, lindisp, tr).contiguous()
        for wk in SP.W_KINDS:
            w = SP.make_weights(rng, wk, N, S, K)
            for uk in SP.U_KINDS:
                yield f"S={S} Ni={Ni} K={K} ndc={ndc} lindisp={lindisp} jitter={jitter} table={uniform} w={wk} u={uk}", z, w, SP.make_u(rng, uk, N, Ni, z, w)


def _oracle(z, w, u, dtype):
    z, w, u = z.to(dtype), w.to(dtype), u.to(dtype)
    zs = O.sample_pdf(0.5 * (z[..., 1:] + z[..., :-1]), w.mean(-1)[..., 1:-1], u)
    return torch.sort(torch.cat([z, zs], -1), -1)[0]


@pytest.mark.parametrize("S,Ni,K", SP.SHAPES)
def test_oracle_passes_the_bracket_fp64_exactly_and_fp32_with_the_derived_constants(S, Ni, K):
    wide = []
    for what, z, w, u in _inputs(S, Ni, K):
        SP.check_sample_pdf(_oracle(z, w, u, torch.float64), z, w, u, what + " fp64", t_u=0.0, t_z_roundings=0.0)     # lo = hi: bit for bit
        r = SP.check_sample_pdf(_oracle(z, w, u, torch.float32), z, w, u, what + " fp32")
        wide.append(r["wide_share"])
    print(f"S={S}: wide brackets, largest share of a case {max(wide):.4f}, mean {np.mean(wide):.4f}, cases {len(wide)}")


@pytest.mark.parametrize("mutation", ["slice", "no_carry", "bins_shift", "no_eps"])
@pytest.mark.parametrize("S,Ni,K", [s for s in SP.SHAPES if s[0] >= 130])
def test_the_bracket_has_teeth(S, Ni, K, mutation):
    """w[0:-2] for w[1:-1]; the carry dropped after the first 64 entries; bins shifted by one; the +1e-5 omitted: each puts more than half of
    a case's samples outside their brackets - and the unmutated restatement none"""
    rng = np.random.default_rng(S + len(mutation))
    N = SP.N_RAYS
    rays = SP.make_rays(rng, N, True)
    z = O.sample_z(rays[:, 6:7], rays[:, 7:8], SP.make_t_vals(S), False, torch.tensor(rng.uniform(0, 1, (N, S)), dtype=torch.float32))
    for wk in ("random", "surface"):
        w = SP.make_weights(rng, wk, N, S, K)
        u = SP.make_u(rng, "uniform", N, Ni)
        good = SP.judge(SP.resample64(z, w, u).astype(np.float32), z, w, u)
        bad = SP.judge(SP.resample64(z, w, u, mutation).astype(np.float32), z, w, u)
        print(f"S={S} {wk} {mutation}: outside {bad['outside_share']:.3f} (unmutated {good['n_outside']} of {good['n_samples']})")
        assert good["n_outside"] == 0 and good["rows_judged"] == N
        assert bad["rows_judged"] == N and bad["outside_share"] > 0.5, (wk, mutation, bad)


def test_the_helper_sees_a_lost_slot_a_descent_and_a_moved_coarse_depth():
    """checks 1 - 3 on a passing output with one element spoilt"""
    rng = np.random.default_rng(5)
    S, Ni, K, N = 66, 63, 3, SP.N_RAYS
    rays = SP.make_rays(rng, N, False)
    z = O.sample_z(rays[:, 6:7], rays[:, 7:8], SP.make_t_vals(S), False, None).contiguous()
    w, u = SP.make_weights(rng, "random", N, S, K), SP.make_u(rng, "rep4", N, Ni)
    good = _oracle(z, w, u, torch.float32)
    SP.check_sample_pdf(good, z, w, u, "unspoilt")
    lost = good.clone(); lost[3, 17] = float("nan")
    assert SP.judge(lost, z, w, u)["n_nan"] == 1
    i = int(torch.nonzero(good[2, 1:] > good[2, :-1])[20])                # two neighbours that differ, swapped
    desc = good.clone(); desc[2, i], desc[2, i + 1] = good[2, i + 1], good[2, i]
    assert SP.judge(desc, z, w, u)["n_unsorted"] == 1
    moved = good.clone()
    k = int(torch.searchsorted(good[5], z[5, 30]))
    moved[5, k] = torch.nextafter(good[5, k], good[5, k + 1])             # one ulp: still sorted, no longer the coarse depth
    assert SP.judge(moved, z, w, u)["n_coarse_missing"] >= 1
    for spoilt in (lost, desc, moved):
        with pytest.raises(AssertionError):
            SP.check_sample_pdf(spoilt, z, w, u, "spoilt")
