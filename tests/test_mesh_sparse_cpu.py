"""CPU tier of the sparse mesh extractor (include/rnb_mesh.h): the numpy statement of tests/mesh_sparse_reference.py on the analytic sphere (nothing dropped under
the band bitfield, exactly the bricks without a set cell dropped under a half-cleared one, empty and ragged cases), and the C-ABI of the mesh header (exports,
version, defaults, struct layout against the Python declarations). No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_checks
from tests import mesh_sparse_reference as ms
from tests import render_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh.h")


def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


def _sphere_lattice(res):
    """sdf of the analytic sphere on the lattice of rnb_sdf_lattice over [0, 1): [rz, ry, rx] float32."""
    g = [np.arange(r, dtype=np.float64) / r for r in res]
    z, y, x = np.meshgrid(g[2], g[1], g[0], indexing="ij")
    return rr.sphere_sdf()(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))[0].reshape(res[2], res[1], res[0]).astype(np.float32)


_CACHE = {}


def _dense(res):
    if res not in _CACHE:
        d = _sphere_lattice(res)
        _CACHE[res] = (d,) + tuple(mesh_checks.host_marching_cubes(d))
    return _CACHE[res]


def _half_cleared(bits):
    """The band bitfield with every cascade-0 cell beyond x = 0.5 cleared."""
    occ = ms.occupancy_cells(bits, 0)
    occ[:, :, 65:] = False
    g = np.arange(128, dtype=np.uint32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    flat = np.zeros(128 ** 3, bool)
    flat[rr.morton3d(x.ravel(), y.ravel(), z.ravel()).astype(np.int64)] = occ.ravel()
    out = bits.copy()
    out[: 128 ** 3 // 8] = np.packbits(flat.reshape(-1, 8)[:, ::-1], axis=1).ravel()
    return out


@pytest.mark.parametrize("res,brick", [((64, 64, 64), 8), ((64, 64, 64), 16), ((40, 50, 70), 16), ((40, 50, 70), 64)])
def test_band_bitfield_drops_nothing(res, brick):
    """A cell the surface crosses has |sdf(centre of its occupancy cell)| <= 0.87 cell < the band of 2.5 cells: the culled triangle set is the dense one."""
    d, v, i = _dense(res)
    assert len(i) > 3000
    bits = rr.bitfield_from_sdf(rr.sphere_sdf())
    e = ms.expected(d, v, i, bits, brick)
    assert (~e["keep"]).sum() == 0
    assert np.array_equal(e["triangles"], ms.triangle_keys(v, i))
    # each vertex of D once (the analytic sphere passes exactly through lattice points, where D itself has coincident vertices: compare with D's own count)
    assert len(e["verts"]) == len(v) and len(np.unique(e["verts"], axis=0)) == len(np.unique(v, axis=0))
    assert e["kept"].sum() <= e["evaluated"].sum() and e["sign_change"].sum() <= e["evaluated"].sum()
    assert not (e["sign_change"] & ~e["evaluated"]).any()
    none = ms.expected(d, v, i, None, brick)
    assert none["kept"].all() and none["evaluated"].all() and np.array_equal(none["triangles"], e["triangles"])
    # every brick that holds a triangle's cell sees a sign change, with or without culling
    b = np.unique(e["cells"] // brick, axis=0)
    assert e["sign_change"][b[:, 2], b[:, 1], b[:, 0]].all() and none["sign_change"][b[:, 2], b[:, 1], b[:, 0]].all()


def test_half_cleared_bitfield_drops_exactly_the_bricks_without_a_set_cell():
    res, brick = (64, 64, 64), 8
    d, v, i = _dense(res)
    bits = _half_cleared(rr.bitfield_from_sdf(rr.sphere_sdf()))
    e = ms.expected(d, v, i, bits, brick)
    n_all, n_keep = len(e["keep"]), int(e["keep"].sum())
    assert 0 < n_keep < n_all
    assert len(e["triangles"]) == n_keep and len(e["indices"]) == 3 * n_keep
    dense_keys = ms.triangle_keys(v, i)
    assert len(np.unique(np.concatenate([dense_keys, e["triangles"]]), axis=0)) == len(np.unique(dense_keys, axis=0))  # a subset of D
    # per triangle, independently of the mask's index arithmetic: the grown box of a dropped triangle's brick meets no set cell, that of a kept one's does
    boxes = ms.set_cell_boxes(bits)
    bricks = e["cells"] // brick
    verdict = {}
    for (bx, by, bz), keep in zip(map(tuple, bricks), e["keep"]):
        if (bx, by, bz) not in verdict:
            verdict[(bx, by, bz)] = ms.brick_meets_a_set_cell(bx, by, bz, res, brick, boxes)
        assert verdict[(bx, by, bz)] == bool(keep)
    assert e["cells"][~e["keep"]][:, 0].min() * (1.0 / 64) > 0.5  # what is dropped lies beyond x = 0.5


def test_empty_bitfield_and_bricks_larger_than_the_lattice():
    res = (40, 50, 70)
    d, v, i = _dense(res)
    e = ms.expected(d, v, i, np.zeros(128 ** 3 // 8 * 8, np.uint8), 16)
    assert not e["kept"].any() and not e["evaluated"].any() and not e["sign_change"].any()
    assert len(e["verts"]) == 0 and len(e["indices"]) == 0 and e["triangles"].shape == (0, 9)
    assert ms.n_bricks(res, 16) == (3, 4, 5) and e["kept"].shape == (5, 4, 3)
    one = ms.expected(d, v, i, rr.bitfield_from_sdf(rr.sphere_sdf()), 128)  # one brick holds everything
    assert one["kept"].shape == (1, 1, 1) and one["kept"].all() and one["keep"].all() and one["sign_change"].all()


def test_coarser_cascades_and_their_shadowed_cells():
    """A set cell of cascade 1 outside the unit cube keeps the bricks it touches; one inside the cube of cascade 0 is never consulted."""
    bits = np.zeros(128 ** 3 // 8 * 8, np.uint8)
    idx = int(rr.morton3d(np.array([64], np.uint32), np.array([64], np.uint32), np.array([64], np.uint32))[0])  # cascade-1 cell at the centre: shadowed
    bits[128 ** 3 // 8 + idx // 8] |= 1 << (idx % 8)
    assert not ms.kept_mask((64, 64, 64), 8, bits, -0.5, 1.5).any()
    idx = int(rr.morton3d(np.array([100], np.uint32), np.array([64], np.uint32), np.array([64], np.uint32))[0])  # x in [1.0625, 1.078]: outside cascade 0
    bits[128 ** 3 // 8 + idx // 8] |= 1 << (idx % 8)
    k = ms.kept_mask((64, 64, 64), 8, bits, -0.5, 1.5)  # a lattice step is 1 / 32: the cell lies inside brick x = 6 (points 48..55 = 1.0 .. 1.22)
    assert k.any() and k[:, :, 6].any() and not k[:, :, :5].any()
    boxes = ms.set_cell_boxes(bits)
    assert all(ms.brick_meets_a_set_cell(bx, by, bz, (64, 64, 64), 8, boxes, -0.5, 1.5) == k[bz, by, bx] for bz in range(8) for by in range(8) for bx in range(8))


def test_mesh_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = _functions(HEADER)
    assert names == ["rnb_extract_mesh", "rnb_mesh_abi_version", "rnb_mesh_default_options", "rnb_mesh_free"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_PROTOTYPES) == set(names)
    assert not set(_abi.MESH_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.RENDER_PROTOTYPES))  # a table of its own
    # rnb_neus2.h is unchanged: its 54 functions and ABI 5
    assert len(_functions(os.path.join(ROOT, "include", "rnb_neus2.h"))) == 54
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5
    assert fns.mesh_abi_version() == _abi.MESH_ABI_VERSION == 1
    opt = _abi.MeshOptions()
    assert fns.mesh_default_options(C.byref(opt)) == 0
    assert opt.abi_version == 1 and list(opt.res) == [256, 256, 256] and (opt.lattice_min, opt.lattice_max, opt.thresh) == (0.0, 1.0, 0.0)
    assert list(opt.aabb_min) == [0.0] * 3 and list(opt.aabb_max) == [1.0] * 3
    assert opt.use_inference_params == 1 and opt.cull == _abi.MESH_CULL_OCCUPANCY == 1 and opt.brick == 0 and opt.attributes == 0
    assert opt.max_points_in_flight == 0 and opt.max_active_points == 0 and list(opt.reserved) == [0] * 4
    assert fns.mesh_default_options(None) == _abi.ERR_INVALID
    # rnb_extract_mesh validates its arguments before it touches a context or the device
    m = _abi.Mesh()
    assert fns.extract_mesh(None, None, C.byref(opt), C.byref(m), None) == _abi.ERR_INVALID
    assert fns.mesh_free(None, C.byref(m)) == _abi.ERR_INVALID
    assert hasattr(api.Context, "extract_mesh")


def test_mesh_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    src = tmp_path / "layout.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "rnb_mesh.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh_options), offsetof(rnb_mesh_options, lattice_min), offsetof(rnb_mesh_options, aabb_max),
         offsetof(rnb_mesh_options, thresh), offsetof(rnb_mesh_options, brick), offsetof(rnb_mesh_options, max_points_in_flight),
         offsetof(rnb_mesh_options, max_active_points), offsetof(rnb_mesh_options, reserved));
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh), offsetof(rnb_mesh, normals), offsetof(rnb_mesh, n_indices), sizeof(rnb_mesh_stats),
         offsetof(rnb_mesh_stats, peak_workspace), offsetof(rnb_mesh_stats, ms));
  printf("%d %d %d %u %u %u\\n", RNB_MESH_ABI_VERSION, RNB_MESH_CULL_NONE, RNB_MESH_CULL_OCCUPANCY, RNB_MESH_ATTR_COLORS, RNB_MESH_ATTR_NORMALS, RNB_MESH_MAX_RES);
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    O, M, S = _abi.MeshOptions, _abi.Mesh, _abi.MeshStats
    assert out[:8] == [C.sizeof(O), O.lattice_min.offset, O.aabb_max.offset, O.thresh.offset, O.brick.offset, O.max_points_in_flight.offset, O.max_active_points.offset, O.reserved.offset]
    assert out[8:14] == [C.sizeof(M), M.normals.offset, M.n_indices.offset, C.sizeof(S), S.peak_workspace.offset, S.ms.offset]
    assert out[14:] == [_abi.MESH_ABI_VERSION, _abi.MESH_CULL_NONE, _abi.MESH_CULL_OCCUPANCY, _abi.MESH_ATTR_COLORS, _abi.MESH_ATTR_NORMALS, _abi.MESH_MAX_RES]
