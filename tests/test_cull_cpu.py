"""CPU: rendering through an occupancy grid (CFNERF_F_CULL) - everything that needs no GPU.

* the flag in the header (a hex literal: the `1 << n` flags are pinned to bits 0..6) and in the Python mirror, 34 exports as before;
* the two host structs: member order in the header, size and offsets of the ctypes mirrors against a C99 compiler's;
* host-side refusals that name the flag before anything touches a device;
* ``evaluate.OccupancyGrid``: bit packing, dilation, ``fraction`` and ``scale`` against numpy restatements;
* tools/kernel_regs.py of the built library: the new kernels without VGPR spill or scratch, and profiles/r14_kernel_regs.txt with the built figures."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfnerf_amd import _lib as L
from cfnerf_amd import api as A
from cfnerf_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(\S.*?)\s+vgpr=\s*(\d+) agpr=\s*(\d+) vgpr_spill=\s*(\d+) sgpr=\s*(\d+) sgpr_spill=\s*(\d+) scratch=\s*(\d+) lds=\s*(\d+)\s*$")


def _table(text):
    """{kernel name: (vgpr, agpr, vgpr_spill, sgpr, sgpr_spill, scratch, lds)} of the kernel lines of a tools/kernel_regs.py listing"""
    out = {}
    for l in text.splitlines():
        m = LINE.match(l)
        if m:
            assert m.group(1) not in out, l
            out[m.group(1)] = tuple(int(v) for v in m.groups()[1:])
    return out



NEW_KERNELS = ["cull_kernel<false>", "cull_kernel<true>", "cfnerf::cull_scan_kernel","composite_sparse_kernel<4, false>",
               "composite_sparse_kernel<8, false>", "composite_sparse_kernel<8, true>"]
CULL_MEMBERS = ["occ_bits", "lo", "scale", "res", "outside", "slot", "ray_start", "pts_c", "ray_of"]
SPARSE_MEMBERS = ["slot", "ray_start", "weights_opt"]


def _header():
    with open(os.path.join(ROOT, "include", "cfnerf.h")) as f:
        return f.read()


# ---------------------------------------------------------------- flag, exports, structs
def test_flag_is_a_hex_literal_on_bit_11_and_overlaps_no_other():
    hdr = _header()
    assert re.search(r"\bCFNERF_F_CULL\s*=\s*0x800\b", hdr)
    assert not re.search(r"CFNERF_F_CULL\s*=\s*1\s*<<", hdr)
    assert L.F_CULL == 0x800 == 1 << 11
    others = {n: getattr(L, n) for n in dir(L) if n.startswith("F_") and n != "F_CULL"}
    assert len(others) == 11
    for n, v in others.items():
        assert v & L.F_CULL == 0, n
    assert len(L.EXPORTS) == 34


def _members(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*;", body)


def test_structs_have_the_headers_member_order_and_the_c_compilers_layout(tmp_path):
    hdr = _header()
    assert _members(hdr, "cfnerf_cull") == CULL_MEMBERS == [f[0] for f in L.Cull._fields_]
    assert _members(hdr, "cfnerf_sparse_raw") == SPARSE_MEMBERS == [f[0] for f in L.SparseRaw._fields_]
    cc = shutil.which("gcc") or shutil.which("cc")
    assert C.sizeof(L.SparseRaw) == 3 * C.sizeof(C.c_void_p) and L.Cull.lo.offset == C.sizeof(C.c_void_p) and L.Cull.outside.offset == L.Cull.lo.offset + 36
    if not cc:                                             # the C compiler's own layout, where there is one
        return
    fields = ["sizeof(cfnerf_cull)"] + [f"offsetof(cfnerf_cull, {m})" for m in CULL_MEMBERS]
    fields += ["sizeof(cfnerf_sparse_raw)"] + [f"offsetof(cfnerf_sparse_raw, {m})" for m in SPARSE_MEMBERS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cfnerf.h"\nint main(void) { printf("' + " ".join(["%zu"] * len(fields))
                   + '\\n", ' + ", ".join("(size_t)" + f for f in fields) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(L.Cull)] + [getattr(L.Cull, m).offset for m in CULL_MEMBERS]
    want += [C.sizeof(L.SparseRaw)] + [getattr(L.SparseRaw, m).offset for m in SPARSE_MEMBERS]
    assert got == want


def test_struct_arg_is_the_structs_host_address():
    sp = L.SparseRaw(None, None, None)
    assert L.struct_arg(sp).value == C.addressof(sp)
    assert L.dptr(None) is None and L.dptr(torch.zeros(3, dtype=torch.int32)) != 0


# ---------------------------------------------------------------- refusals on a machine without a device
def test_host_side_refusals_name_the_flag():
    lib = L.lib()
    rc = lib.cfnerf_sample_points(None, None, None, L.F_CULL, 4, 8, None, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "CFNERF_F_CULL" in msg and "cfnerf_cull" in msg
    rc = lib.cfnerf_sample_pdf(None, None, None, L.F_CULL, None, None, 4, 8, 2, 4, None, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "cfnerf_sample_pdf" in msg and "CFNERF_F_CULL" in msg
    # the flag does not unlock the others: GEOMETRY on cfnerf_sample_points is refused as before
    rc = lib.cfnerf_sample_points(None, None, None, L.F_CULL | L.F_GEOMETRY, 4, 8, None, None, None)
    assert rc < 0 and "CFNERF_F_GEOMETRY" in lib.cfnerf_last_error().decode()


def _desc(**over):
    """a Cull whose pointers are non-NULL dummies (never dereferenced: every call below is refused on the host)"""
    d = dict(occ_bits=8, lo=(C.c_float * 3)(0, 0, 0), scale=(C.c_float * 3)(1, 1, 1), res=(C.c_int32 * 3)(2, 2, 2), outside=0, slot=8, ray_start=8,
             pts_c=8, ray_of=8)
    d.update(over)
    return L.Cull(*(d[k] for k in CULL_MEMBERS))


@pytest.mark.parametrize("member", ["occ_bits", "slot", "ray_start", "pts_c", "ray_of"])
def test_a_null_member_of_the_descriptor_is_refused_by_name(member):
    lib = L.lib()
    d = _desc(**{member: None})
    rc = lib.cfnerf_sample_points(None, None, None, L.F_CULL, 4, 8, None, L.struct_arg(d), None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "CFNERF_F_CULL" in msg and member in msg, msg


def test_a_res_below_one_and_a_null_sparse_descriptor_are_refused():
    lib = L.lib()
    d = _desc(res=(C.c_int32 * 3)(2, 0, 2))
    rc = lib.cfnerf_sample_points(None, None, None, L.F_CULL, 4, 8, None, L.struct_arg(d), None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "CFNERF_F_CULL" in msg and "res[1]" in msg
    comp = lambda wb, w: lib.cfnerf_composite_fwd(None, None, None, 4, 8, 2, wb, None, None, None, w, None)
    rc = comp(L.F_CULL | 1, None)
    msg = lib.cfnerf_last_error().decode()
    assert rc < 0 and "CFNERF_F_CULL" in msg and "cfnerf_sparse_raw" in msg
    for member in ("slot", "ray_start"):
        sp = L.SparseRaw(**{"slot": 8, "ray_start": 8, "weights_opt": None, member: None})
        rc = comp(L.F_CULL, L.struct_arg(sp))
        msg = lib.cfnerf_last_error().decode()
        assert rc < 0 and "CFNERF_F_CULL" in msg and member in msg, msg


def test_python_entry_points_refuse_what_they_cannot_do():
    with pytest.raises(ValueError, match="acc_map"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="ext", occupancy=object())
    with pytest.raises(ValueError, match="acc_map"):
        E.render_uncertainty(4, 4, 1.0, torch.eye(4)[:3], None, stats="geometry", occupancy=object())
    import inspect
    names = list(inspect.signature(E.render_uncertainty).parameters)
    assert names[-2:] == ["occupancy", "_ignored"]
    assert list(inspect.signature(A.cull_points).parameters) == ["ray_batch", "grid", "t_vals", "t_rand", "lindisp", "outside"]
    assert list(inspect.signature(A.raw2outputs_sparse).parameters) == ["raw_c", "slot", "ray_start", "z_vals", "rays_d", "white_bkgd", "retweights"]
    assert list(inspect.signature(A.render_rays_culled).parameters)[:7] == ["ray_batch", "network_fn", "grid", "t_vals", "lindisp", "white_bkgd", "retweights"]


# ---------------------------------------------------------------- OccupancyGrid against numpy
def _np_pack(mask):
    flat = mask.reshape(-1).astype(np.uint64)
    words = np.zeros((flat.size + 31) // 32, np.uint64)
    for c in np.nonzero(flat)[0]:
        words[c >> 5] |= np.uint64(1) << np.uint64(c & 31)
    return words.astype(np.uint32)


@pytest.mark.parametrize("shape,kind", [((4, 3, 5), "random"), ((4, 3, 5), "empty"), ((4, 3, 5), "full"), ((8, 4, 2), "random"), ((1, 1, 1), "full"),
                                        ((3, 11, 2), "random")])
def test_from_mask_packs_the_bits_as_laid_out(shape, kind):
    rng = np.random.default_rng(sum(shape))
    mask = {"random": rng.random(shape) < 0.4, "empty": np.zeros(shape, bool), "full": np.ones(shape, bool)}[kind]
    lo, hi = (-1.0, 0.5, 2.0), (1.5, 3.5, 2.75)
    g = E.OccupancyGrid.from_mask(torch.tensor(mask), lo, hi)
    assert g.bits.dtype == torch.int32 and g.bits.numel() == (mask.size + 31) // 32
    assert np.array_equal(g.bits.numpy().view(np.uint32), _np_pack(mask))
    assert g.res == shape and g.fraction == pytest.approx(mask.mean())
    assert g.lo.dtype == g.hi.dtype == g.scale.dtype == np.float32
    assert np.array_equal(g.lo, np.float32(lo)) and np.array_equal(g.hi, np.float32(hi))
    assert np.array_equal(g.scale, np.float32(shape) / (np.float32(hi) - np.float32(lo)))      # fp32 / fp32, once
    # cell (ix, iy, iz) is bit c & 31 of word c >> 5, c = (ix * Y + iy) * Z + iz
    w = g.bits.numpy().view(np.uint32)
    for ix, iy, iz in zip(*np.nonzero(np.ones(shape, bool))):
        c = (ix * shape[1] + iy) * shape[2] + iz
        assert bool((w[c >> 5] >> np.uint32(c & 31)) & 1) == bool(mask[ix, iy, iz])


def test_from_mask_refuses_what_is_not_a_bool_volume():
    with pytest.raises(ValueError):
        E.OccupancyGrid.from_mask(torch.zeros(4, 3, 5), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        E.OccupancyGrid.from_mask(torch.zeros(4, 3, dtype=torch.bool), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        E.OccupancyGrid.from_mask(torch.zeros(4, 3, 5, dtype=torch.bool), (0, 0, 0), (1, 0, 1))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_dilate_against_numpy(n):
    rng = np.random.default_rng(5 + n)
    mask = rng.random((6, 5, 7)) < 0.08
    mask[0, 0, 0] = mask[5, 4, 6] = True                       # corners: the growth stops at the box
    want = np.zeros_like(mask)
    X, Y, Z = mask.shape
    for ix, iy, iz in zip(*np.nonzero(mask)):
        want[max(ix - n, 0):ix + n + 1, max(iy - n, 0):iy + n + 1, max(iz - n, 0):iz + n + 1] = True
    got = E.OccupancyGrid.dilate_mask(torch.tensor(mask), n)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)


def test_k_stats_are_the_evaluation_loops_estimators():
    rng = np.random.default_rng(3)
    K = 5
    rgb, disp, depth = rng.random((7, 3, K)), rng.random((7, K)), rng.random((7, K))
    m, u, dm, zm = E.k_stats(torch.tensor(rgb), torch.tensor(disp), torch.tensor(depth))
    np.testing.assert_allclose(m.numpy(), rgb.mean(-1), rtol=1e-12)
    np.testing.assert_allclose(u.numpy(), np.std(rgb, -1) * K / (K - 1), rtol=1e-12)          # RUN:1129-1130
    np.testing.assert_allclose(dm.numpy(), disp.mean(-1), rtol=1e-12)
    np.testing.assert_allclose(zm.numpy(), depth.mean(-1), rtol=1e-12)


# ---------------------------------------------------------------- the new kernels in the built code object
@pytest.fixture(scope="module")
def built():
    return _table(subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py")], capture_output=True, text=True, check=True).stdout)


def test_new_kernels_are_built_without_spill_or_scratch(built):
    for k in NEW_KERNELS:
        assert k in built, k
        vgpr, agpr, vspill, sgpr, sspill, scratch, lds = built[k]
        assert vspill == 0 and scratch == 0, (k, built[k])
    # the sparse composite keeps the dense composite's occupancy: four workgroups per CU need <= 128 registers and <= 40 KB of LDS
    for k in NEW_KERNELS[3:]:
        assert built[k][0] <= 128 + (40 if "false" in k else 0) and built[k][6] <= 40 * 1024, (k, built[k])


def test_r14_table_lists_the_new_kernels_with_the_built_figures(built):
    text = open(os.path.join(ROOT, "profiles", "r14_kernel_regs.txt")).read()
    assert "(none)" in text.split("## changed")[1].split("## new")[0]
    new = _table(text.split("## new")[1].split("## unchanged")[0])
    old = _table(text.split("## unchanged")[1])
    assert sorted(new) == sorted(NEW_KERNELS)
    for k, v in list(new.items()) + list(old.items()):
        assert built[k] == v, (k, v, built.get(k))
    assert set(new) | set(old) == set(built)
