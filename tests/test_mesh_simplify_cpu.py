"""CPU tier of the mesh simplifier (include/rnb_mesh_simplify.h): the C-ABI of the new header (exports, version, defaults, struct layout, argument validation without a
device), the numpy statement of tests/mesh_simplify_reference.py on hand-made cases and its own properties on marching-cubes meshes, and the command-line / pipeline
surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_simplify_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_simplify.h")


def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_simplify_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = _functions(HEADER)
    assert names == ["rnb_mesh_simplify", "rnb_mesh_simplify_abi_version", "rnb_mesh_simplify_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_SIMPLIFY_PROTOTYPES) == set(names)
    assert not set(_abi.MESH_SIMPLIFY_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.RENDER_PROTOTYPES) | set(_abi.MESH_PROTOTYPES) | set(_abi.MESH_CLEAN_PROTOTYPES))
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_abi_version() == 1 and fns.mesh_clean_abi_version() == 1  # the others are as they were
    assert fns.mesh_simplify_abi_version() == _abi.MESH_SIMPLIFY_ABI_VERSION == 1
    opt = _abi.MeshSimplifyOptions()
    assert fns.mesh_simplify_default_options(C.byref(opt)) == 0
    assert (opt.abi_version, list(opt.origin), opt.cell, list(opt.dims), opt.placement, list(opt.reserved)) == (1, [0.0] * 3, 1.0 / 256, [256] * 3, _abi.MESH_PLACE_QUADRIC, [0] * 4)
    assert fns.mesh_simplify_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.Context, "simplify_mesh")
    from rnb_neus2_amd import build
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_simplify.cuh") in build.DEPS


def test_simplify_validates_its_arguments_without_a_device():
    """Null pointers, a wrong version, an unknown placement, a bad cell / origin / dims, n_indices % 3 and null buffers are refused before the context or the device is
    touched: the context handed in here is not one (a block of zeros), and no device exists where this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good():
        o = _abi.MeshSimplifyOptions()
        assert fns.mesh_simplify_default_options(C.byref(o)) == 0
        return o

    def call(ctx_, m_in, o, m_out):
        return fns.mesh_simplify(ctx_, None, m_in, o, m_out, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    assert call(None, C.byref(src), C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, None, C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), None, C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), C.byref(good()), None) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), C.byref(good()), C.byref(src)) == _abi.ERR_INVALID  # in place
    nan, inf = float("nan"), float("inf")
    cases = [("abi_version", 2), ("abi_version", 0), ("placement", 2), ("placement", 0xFFFFFFFF), ("cell", 0.0), ("cell", -1.0), ("cell", nan), ("cell", inf),
             ("origin", (0.0, nan, 0.0)), ("origin", (inf, 0.0, 0.0)), ("dims", (0, 4, 4)), ("dims", (4, 4097, 4)), ("dims", (4096, 4096, 4096)), ("dims", (1024, 1024, 1025))]
    for field, value in cases:
        o = good()
        if isinstance(value, tuple):
            getattr(o, field)[:] = value
        else:
            setattr(o, field, value)
        dst.n_verts = 7
        assert call(ctx, C.byref(src), C.byref(o), C.byref(dst)) == _abi.ERR_INVALID, (field, value)
        assert dst.n_verts == 0 and not dst.verts  # zeroed on failure
        assert fns.last_error()
    o = good()
    o.dims[:] = (1024, 1024, 1024)  # exactly the cap passes the option checks: what is refused next is the mesh
    src.n_indices, src.n_verts = 4, 3  # not a multiple of 3
    assert call(ctx, C.byref(src), C.byref(o), C.byref(dst)) == _abi.ERR_INVALID and b"multiple of 3" in fns.last_error()
    src.n_indices = 3  # null buffers
    assert call(ctx, C.byref(src), C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    assert fake.raw == b"\0" * 4096


def test_simplify_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    src = tmp_path / "layout.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "rnb_mesh_simplify.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh_simplify_options), offsetof(rnb_mesh_simplify_options, origin), offsetof(rnb_mesh_simplify_options, cell),
         offsetof(rnb_mesh_simplify_options, dims), offsetof(rnb_mesh_simplify_options, placement), offsetof(rnb_mesh_simplify_options, reserved));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh_simplify_stats), offsetof(rnb_mesh_simplify_stats, n_verts_in), offsetof(rnb_mesh_simplify_stats, n_tris_in),
         offsetof(rnb_mesh_simplify_stats, n_clusters), offsetof(rnb_mesh_simplify_stats, n_verts_out), offsetof(rnb_mesh_simplify_stats, n_tris_out),
         offsetof(rnb_mesh_simplify_stats, n_tris_collapsed), offsetof(rnb_mesh_simplify_stats, n_clamped), offsetof(rnb_mesh_simplify_stats, n_fallback),
         offsetof(rnb_mesh_simplify_stats, peak_workspace), offsetof(rnb_mesh_simplify_stats, ms));
  printf("%d %d %d %u %llu %d %d\\n", RNB_MESH_SIMPLIFY_ABI_VERSION, RNB_MESH_PLACE_QUADRIC, RNB_MESH_PLACE_MEAN, RNB_MESH_SIMPLIFY_MAX_DIM,
         (unsigned long long)RNB_MESH_SIMPLIFY_MAX_CELLS, RNB_MESH_SIMPLIFY_Q_SHIFT, RNB_MESH_SIMPLIFY_Q_TERM_LOG2);
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    O, S = _abi.MeshSimplifyOptions, _abi.MeshSimplifyStats
    assert out[:6] == [C.sizeof(O), O.origin.offset, O.cell.offset, O.dims.offset, O.placement.offset, O.reserved.offset]
    assert out[6:17] == [C.sizeof(S), S.n_verts_in.offset, S.n_tris_in.offset, S.n_clusters.offset, S.n_verts_out.offset, S.n_tris_out.offset, S.n_tris_collapsed.offset,
                         S.n_clamped.offset, S.n_fallback.offset, S.peak_workspace.offset, S.ms.offset]
    assert out[17:] == [_abi.MESH_SIMPLIFY_ABI_VERSION, _abi.MESH_PLACE_QUADRIC, _abi.MESH_PLACE_MEAN, _abi.MESH_SIMPLIFY_MAX_DIM, _abi.MESH_SIMPLIFY_MAX_CELLS,
                        _abi.MESH_SIMPLIFY_Q_SHIFT, _abi.MESH_SIMPLIFY_Q_TERM_LOG2]
    assert (sr.Q_SHIFT, sr.Q_TERM_LOG2, sr.MAX_DIM, sr.MAX_CELLS) == (_abi.MESH_SIMPLIFY_Q_SHIFT, _abi.MESH_SIMPLIFY_Q_TERM_LOG2, _abi.MESH_SIMPLIFY_MAX_DIM, _abi.MESH_SIMPLIFY_MAX_CELLS)
    # the other headers stay as they are: none of them mentions this one
    for name in ("rnb_neus2.h", "rnb_render.h", "rnb_mesh.h", "rnb_mesh_clean.h"):
        assert "simplify" not in open(os.path.join(ROOT, "include", name)).read()


# ------------------------------------------------------------------------------------------------------------------------ hand-made cases of the rules
TETRA_T = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2], np.uint32)


def _tetra(scale=1.0, shift=(0.0, 0.0, 0.0)):
    return (np.array([(0.1, 0.1, 0.1), (0.7, 0.2, 0.15), (0.2, 0.8, 0.25), (0.3, 0.3, 0.9)], np.float64) * scale + shift).astype(np.float32)


def test_one_tetrahedron_in_one_cell_gives_an_empty_mesh():
    for pl in ("quadric", "mean"):
        e = sr.expected(_tetra(), TETRA_T, origin=(0, 0, 0), cell=1.0, dims=4, placement=pl)
        assert e["verts"].shape == (0, 3) and e["indices"].shape == (0,)
        assert e["stats"] == dict(n_verts_in=4, n_tris_in=4, n_clusters=1, n_verts_out=0, n_tris_out=0, n_tris_collapsed=4, n_clamped=0, n_fallback=0)
    e = sr.expected(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), colors=np.zeros((5, 3), np.float32))  # an empty input: an empty output
    assert e["verts"].shape == (0, 3) and e["colors"].shape == (0, 3) and e["stats"]["n_clusters"] == 0


def test_each_vertex_in_its_own_cell_gives_the_same_mesh_ordered_by_key():
    v = _tetra(4.0)  # cells of edge 1: (0,0,0), (2,0,0), (0,3,1), (1,1,3)
    col = np.arange(12, dtype=np.float32).reshape(4, 3) / 16
    nrm = np.array([(0, 0, 2), (0, -3, 0), (1, 1, 0), (0, 0, 0)], np.float32)
    for pl in ("quadric", "mean"):
        e = sr.expected(v, TETRA_T, colors=col, normals=nrm, origin=(0, 0, 0), cell=1.0, dims=4, placement=pl)
        keys = sr.locate(v, (0, 0, 0), 1.0, 4)[2]
        order = np.argsort(keys)
        assert list(e["vertex_keys"]) == sorted(keys) and e["stats"]["n_verts_out"] == 4 and e["stats"]["n_tris_out"] == 4 and e["stats"]["n_fallback"] == 0
        # every corner lies on all the planes that touch it, so the quadric's minimiser is the vertex itself (and so is the mean of one member)
        assert np.abs(e["verts"].astype(np.float64) - v[order]).max() <= 1e-6
        new_of_old = np.argsort(order)
        assert np.array_equal(e["indices"], new_of_old[TETRA_T].astype(np.uint32))  # same triangles, same order, same winding
        assert np.array_equal(e["colors"], col[order])  # one member: its own colour, exactly (multiples of 2^-4)
        want_n = np.array([(0, 0, 1), (0, -1, 0), (np.sqrt(0.5), np.sqrt(0.5), 0), (0, 0, 0)])[order]
        assert np.abs(e["normals"] - want_n).max() < 1e-7 and np.array_equal(e["normals"][new_of_old[3]], [0, 0, 0])  # normalised; a zero sum stays zero


def test_a_vertex_on_a_cell_face_outside_the_grid_and_dims_of_one():
    # exactly on the face between cells 1 and 2 along x: floor puts it into the upper cell, local coordinate -0.5
    p, i, key = sr.locate(np.array([(0.5, 0.3, 0.3)], np.float32), (0, 0, 0), 0.25, 4)
    assert list(i[0]) == [2, 1, 1] and p[0, 0] - (i[0, 0] + 0.5) == -0.5
    # outside the grid: clamped into the border cell, local coordinate beyond [-0.5, 0.5)
    p, i, key = sr.locate(np.array([(-0.3, 1.7, 0.3)], np.float32), (0, 0, 0), 0.25, 4)
    assert list(i[0]) == [0, 3, 1] and p[0, 0] - 0.5 < -0.5 and p[0, 1] - 3.5 > 0.5
    # a tetrahedron with one corner outside: that corner's cluster is placed on its cell's box (mean placement is cut, and counted)
    v = _tetra(4.0)
    v[1] = (5.5, 0.5, 0.5)
    e = sr.expected(v, TETRA_T, origin=(0, 0, 0), cell=1.0, dims=4, placement="mean")
    assert e["stats"]["n_clamped"] == 1 and e["stats"]["n_verts_out"] == 4
    assert [4.0, 0.5, 0.5] in e["verts"].tolist()
    # dims of 1 along z: everything shares iz = 0, keys are ix + 4 * iy, z is clamped into the slab
    e = sr.expected(_tetra(4.0), TETRA_T, origin=(0, 0, 0), cell=1.0, dims=(4, 4, 1), placement="mean")
    assert list(e["cluster_keys"]) == [0, 2, 5, 12] and e["stats"]["n_verts_out"] == 4 and e["stats"]["n_clamped"] == 1  # z = 0.4, 0.6, 1.0 lie in the closed slab, 3.6 is cut
    assert e["verts"][:, 2].max() <= 1.0
    # a flat mesh in one plane: the quadric is singular along the plane and the regularisation pulls to the mean; never a fallback, always finite
    g = np.arange(9)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    fv = np.stack([gx.ravel() / 8.0, gy.ravel() / 8.0, np.full(81, 0.3)], 1).astype(np.float32)
    q = (gy[:-1, :-1] * 9 + gx[:-1, :-1]).ravel()
    ft = np.concatenate([np.stack([q, q + 1, q + 9], 1), np.stack([q + 1, q + 10, q + 9], 1)]).astype(np.uint32)
    e = sr.expected(fv, ft.ravel(), origin=(0, 0, 0), cell=0.25, dims=5)
    assert e["stats"]["n_fallback"] == 0 and np.isfinite(e["verts"]).all() and np.abs(e["verts"][:, 2] - 0.3).max() < 1e-6
    with pytest.raises(ValueError):
        sr.expected(_tetra(), [0, 1, 4])  # index out of range
    with pytest.raises(ValueError):
        sr.expected(_tetra(), [0, 1])  # n_indices % 3
    bad = _tetra()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        sr.expected(bad, TETRA_T)
    sr.expected(np.concatenate([_tetra(), [[np.nan] * 3]]).astype(np.float32), TETRA_T)  # an unused vertex may hold anything
    with pytest.raises(ValueError):
        sr.expected(_tetra(), TETRA_T, cell=0.0)
    with pytest.raises(ValueError):
        sr.expected(_tetra(), TETRA_T, dims=(4096, 4096, 4096))
    with pytest.raises(ValueError):
        sr.expected(_tetra(2.0 ** 23), TETRA_T, cell=1.0, dims=4)  # 2^23 cells outside the grid: the local position is over the term bound


# ------------------------------------------------------------------------------------------------------------------------ the statement's own properties
def _inside_its_cell(e, origin, cell, dims):
    """Every output vertex lies in the closed box of its cell, up to the rounding of the final conversion to float (half an ulp of the coordinate)."""
    d = np.array([dims] * 3 if np.isscalar(dims) else dims, np.int64)
    k = e["vertex_keys"]
    i = np.stack([k % d[0], (k // d[0]) % d[1], k // (d[0] * d[1])], 1).astype(np.float64)
    c, o = np.float64(np.float32(cell)), np.asarray(origin, np.float32).astype(np.float64)
    v = e["verts"].astype(np.float64)
    slack = np.spacing(np.abs(e["verts"])).astype(np.float64)
    return bool(np.all(v >= i * c + o - slack) and np.all(v <= (i + 1) * c + o + slack))


def _surface_rms_radial(verts, indices, centre, radius):
    """Root of the area-weighted mean of (|x - centre| - radius)^2 over the surface, by the edge-midpoint rule per triangle (exact for quadratics)."""
    v, t = np.asarray(verts, np.float64), np.asarray(indices, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    e2 = sum((np.linalg.norm(m - centre, axis=1) - radius) ** 2 for m in ((a + b) / 2, (b + c) / 2, (c + a) / 2)) / 3.0
    return float(np.sqrt((area * e2).sum() / area.sum()))


def test_three_spheres_keep_their_boundary_zero_and_their_vertices_inside_their_cells():
    v, i = mc.three_spheres(64)
    assert sr.directed_edge_balance(i) == 0
    for n in (16, 8):
        for pl in ("quadric", "mean"):
            e = sr.expected(v, i, origin=(0, 0, 0), cell=1.0 / n, dims=n, placement=pl)
            assert 0 < e["stats"]["n_tris_out"] < len(i) // 3 and e["stats"]["n_tris_out"] + e["stats"]["n_tris_collapsed"] == len(i) // 3
            assert sr.directed_edge_balance(e["indices"]) == 0  # clustering a closed oriented mesh keeps the boundary zero
            assert _inside_its_cell(e, (0, 0, 0), 1.0 / n, n)
            assert e["stats"]["n_verts_out"] == len(np.unique(e["indices"])) == len(e["verts"])
    # the sums are integers: a permutation of the triangles permutes the output's triangles, a renumbering of the vertices changes nothing
    rng = np.random.default_rng(4)
    t = i.reshape(-1, 3)
    e = sr.expected(v, i, cell=1.0 / 16, dims=16)
    perm = rng.permutation(len(t))
    p = sr.expected(v, t[perm].ravel(), cell=1.0 / 16, dims=16)
    pos = np.cumsum(e["tri_kept"]) - 1
    assert p["verts"].tobytes() == e["verts"].tobytes() and np.array_equal(p["indices"].reshape(-1, 3), e["indices"].reshape(-1, 3)[pos[perm[e["tri_kept"][perm]]]])
    new_of_old = rng.permutation(len(v))
    w = np.empty_like(v)
    w[new_of_old] = v
    r = sr.expected(w, new_of_old[t].ravel(), cell=1.0 / 16, dims=16)
    assert r["verts"].tobytes() == e["verts"].tobytes() and r["indices"].tobytes() == e["indices"].tobytes()


@pytest.mark.parametrize("lattice,n", [(64, 16), (64, 8), (96, 24), (128, 16)])
def test_quadric_placement_beats_mean_placement_on_a_sphere(lattice, n):
    """A marching-cubes sphere (radius 0.3 around the centre of the unit box). Quadric placement has the smaller rms radial error and the smaller relative volume error.
    The radial error is that of the SURFACE (area-weighted over the triangles, edge-midpoint rule), which is what a simplified mesh is judged by: the mean of a cap's
    vertices lies inside the sphere and the chords between such vertices lie deeper still, while the quadric's minimiser lies slightly outside, so that the chords
    straddle the sphere. Measured over the vertices alone the two are about equal in size and opposite in sign ((64, 16): +0.96e-3 mean signed error for quadric,
    -0.83e-3 for the mean; rms 1.10e-3 against 0.91e-3; the other cases quadric / mean 3.95e-3 / 3.39e-3, 5.1e-4 / 4.3e-4, 1.05e-3 / 0.90e-3: over the vertices the quadric
    is the WORSE by a fifth, and this test does not assert otherwise), which says nothing about the surface between them. Figures of the statement, surface rms quadric / mean:
    (64, 16) 1.03e-3 / 2.99e-3, (64, 8) 4.14e-3 / 1.16e-2, (96, 24) 4.7e-4 / 1.39e-3, (128, 16) 1.01e-3 / 2.89e-3; volume error -0.7 % / -2.8 %, -2.7 % / -10.2 %,
    -0.3 % / -1.3 %, -0.7 % / -2.7 %."""
    centre, radius = np.array([0.5, 0.5, 0.5]), 0.3
    v, i = sr.sphere_mesh(lattice, centre, radius)
    vol = 4.0 / 3.0 * np.pi * radius ** 3
    res = {}
    for pl in ("quadric", "mean"):
        e = sr.expected(v, i, origin=(0, 0, 0), cell=1.0 / n, dims=n, placement=pl)
        assert sr.directed_edge_balance(e["indices"]) == 0 and _inside_its_cell(e, (0, 0, 0), 1.0 / n, n)
        res[pl] = (_surface_rms_radial(e["verts"], e["indices"], centre, radius), abs(sr.signed_volume(e["verts"], e["indices"]) / vol - 1.0))
        print(lattice, n, pl, "surface rms %.3e, volume error %.2f %%, %d triangles" % (res[pl][0], 100 * res[pl][1], e["stats"]["n_tris_out"]))
    assert res["quadric"][0] < res["mean"][0] and res["quadric"][1] < res["mean"][1]


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_simplify_flags():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--simplify" in r.stdout and "--placement" in r.stdout
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--simplify", "0"], ["--simplify", "1025"], ["--simplify", "many"], ["--simplify"], ["--simplify", "-4"], ["--placement", "mean"],
                ["--simplify", "64", "--placement", "median"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255 and "--simplify" in r.stderr, bad  # the help text follows the message
    for good in (["--simplify", "64"], ["--simplify", "1024", "--placement", "mean"], ["--keep", "largest", "--simplify", "32", "--placement", "quadric"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr  # the flags parse; the snapshot is what is missing


def test_plan_device_postprocess_with_and_without_simplify(tmp_path):
    from rnb_neus2_amd import api, pipeline
    import run_pipeline
    today = ["/b/build/mesh", "--snapshot", "/d/prepared_data/output/snapshot_10000.msgpack", "--scene", "/d/prepared_data", "--out", "/out/mesh.obj",
             "--resolution", "1024", "--keep", "largest", "--orient", "outward"]
    assert pipeline.plan_device_postprocess("/d/prepared_data", 10000, 1024, "/out/mesh.obj", "/b/build/mesh") == today
    assert pipeline.plan_device_postprocess("/d/prepared_data", 10000, 1024, "/out/mesh.obj", "/b/build/mesh", simplify=None) == today
    assert pipeline.plan_device_postprocess("/d/prepared_data", 10000, 1024, "/out/mesh.obj", "/b/build/mesh", simplify=256) == today + ["--simplify", "256"]
    stub = str(tmp_path / "testbed")
    common = ["-i", "in", "-t", stub, "-o", str(tmp_path / "out")]
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert kw["device_postprocess"] is True and "simplify" not in kw
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--simplify", "128"]))
    assert kw["device_postprocess"] is True and kw["simplify"] == 128
    assert "simplify" not in run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common))
    for bad in (["--simplify", "128"], ["--device-postprocess", "--simplify", "0"], ["--device-postprocess", "--simplify", "x"]):
        with pytest.raises(SystemExit):  # only valid with --device-postprocess, and only a count the mesh program accepts
            run_pipeline.main(common + bad)
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", stub, str(tmp_path / "out"), simplify=64)
    # the grid build/mesh --simplify N and extract_mesh(simplify=N) lay over a box
    assert api.Context.simplify_grid((0, 0, 0), (1, 1, 1), 32) == ((0.0, 0.0, 0.0), 1.0 / 32, (32, 32, 32))
    assert api.Context.simplify_grid((-0.5, 0, 0), (1.5, 1, 0.25), 8) == ((-0.5, 0.0, 0.0), 0.25, (8, 8, 8))  # dims = N on every axis, as build/mesh
    assert api.Context.simplify_grid((0, 0, 0), (1, 1, 1), 1024)[2] == (1024, 1024, 1024)
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            api.Context.simplify_grid((0, 0, 0), (1, 1, 1), bad)
