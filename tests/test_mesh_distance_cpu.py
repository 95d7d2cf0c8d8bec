"""CPU tier of the mesh-to-mesh distance (include/rnb_mesh_distance.h): the C-ABI of the new header (exports, version, defaults, struct layout, argument validation
without a device), the numpy statement of tests/mesh_distance_reference.py on hand-made cases, and the search of the header (cell lists, shells, stop rule) against the
exhaustive definition, bit for bit. No GPU needed."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_distance_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_distance.h")
UNIT_TRI = (np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32), np.array([0, 1, 2], np.uint32))


@pytest.fixture(autouse=True, scope="module")
def _the_header_exists():
    """Every test here follows the rules as include/rnb_mesh_distance.h states them, the ones that need nothing but numpy too: none of them stands without it."""
    assert os.path.exists(HEADER), HEADER


def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_distance_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi, build
    names = _functions(HEADER)
    assert names == ["rnb_mesh_distance", "rnb_mesh_distance_abi_version", "rnb_mesh_distance_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_DISTANCE_PROTOTYPES) == set(names)
    assert not set(_abi.MESH_DISTANCE_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.RENDER_PROTOTYPES) | set(_abi.MESH_PROTOTYPES) | set(_abi.MESH_CLEAN_PROTOTYPES) | set(_abi.MESH_SIMPLIFY_PROTOTYPES))
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_abi_version() == 1 and fns.mesh_clean_abi_version() == 1 and fns.mesh_simplify_abi_version() == 1  # as they were
    assert fns.mesh_distance_abi_version() == _abi.MESH_DISTANCE_ABI_VERSION == 1
    opt = _abi.MeshDistanceOptions()
    opt.level, opt.cells, opt.reserved[2] = 3, 9, 5
    assert fns.mesh_distance_default_options(C.byref(opt)) == 0
    assert (opt.abi_version, opt.level, opt.max_distance, opt.unit, list(opt.tau), opt.cells, list(opt.reserved)) == (1, 1, 0.0, 2.0 ** -10, [0.0] * 4, 0, [0] * 4)
    assert fns.mesh_distance_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.Context, "mesh_distance")
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_distance.cuh") in build.DEPS
    for name in os.listdir(os.path.join(ROOT, "include")):  # no other header mentions this one
        assert name == "rnb_mesh_distance.h" or "distance.h" not in open(os.path.join(ROOT, "include", name)).read()


def test_distance_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the context or the device is touched: the context handed in here is a block of zeros, and no device exists where
    this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good():
        o = _abi.MeshDistanceOptions()
        assert fns.mesh_distance_default_options(C.byref(o)) == 0
        return o

    def call(ctx_, a, b, o, dist=None, near=None, stats=None):
        return fns.mesh_distance(ctx_, None, a, b, o, dist, near, stats)

    def mesh(nv=3, ni=3):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, 0x1000, 0x2000  # never dereferenced
        return m

    A, B = mesh(), mesh()
    assert call(None, C.byref(A), C.byref(B), C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, None, C.byref(B), C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(A), None, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(A), C.byref(B), None) == _abi.ERR_INVALID
    assert call(ctx, C.byref(A), C.byref(A), C.byref(good())) == _abi.ERR_INVALID and b"different" in fns.last_error()  # aliased meshes
    assert call(ctx, C.byref(A), C.byref(B), C.byref(good()), 0x3000, 0x3000) == _abi.ERR_INVALID and b"different" in fns.last_error()  # aliased outputs
    nan, inf = float("nan"), float("inf")
    cases = [("abi_version", 2), ("abi_version", 0), ("level", 4), ("level", 0xFFFFFFFF), ("unit", 0.0), ("unit", -1.0), ("unit", nan), ("unit", inf), ("max_distance", -1.0),
             ("max_distance", nan), ("max_distance", inf), ("tau", (0.0, -1.0, 0.0, 0.0)), ("tau", (nan, 0.0, 0.0, 0.0)), ("tau", (0.0, 0.0, 0.0, inf)), ("cells", 257)]
    st = _abi.MeshDistanceStats()
    for field, value in cases:
        o = good()
        if isinstance(value, tuple):
            getattr(o, field)[:] = value
        else:
            setattr(o, field, value)
        st.n_tris_to = 7
        assert call(ctx, C.byref(A), C.byref(B), C.byref(o), stats=C.byref(st)) == _abi.ERR_INVALID, (field, value)
        assert st.n_tris_to == 0 and fns.last_error()  # zeroed on failure
    for side in (0, 1):
        ms = [mesh(), mesh()]
        ms[side].n_indices = 4
        assert call(ctx, C.byref(ms[0]), C.byref(ms[1]), C.byref(good())) == _abi.ERR_INVALID and b"multiple of 3" in fns.last_error()
        ms[side].n_indices, ms[side].n_verts = 3, 0
        assert call(ctx, C.byref(ms[0]), C.byref(ms[1]), C.byref(good())) == _abi.ERR_INVALID and b"no vertices" in fns.last_error()  # indices without vertices
        ms[side].n_verts, ms[side].indices = 3, None
        assert call(ctx, C.byref(ms[0]), C.byref(ms[1]), C.byref(good())) == _abi.ERR_INVALID and b"null" in fns.last_error()
    empty_b = mesh(3, 0)
    assert call(ctx, C.byref(A), C.byref(empty_b), C.byref(good())) == _abi.ERR_INVALID and b"non-degenerate" in fns.last_error()  # a B without triangles needs no device to refuse
    assert fake.raw == b"\0" * 4096


def test_distance_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    O, S = _abi.MeshDistanceOptions, _abi.MeshDistanceStats
    of = [n for n, _ in O._fields_]
    sf = [n for n, _ in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_distance.h\"\nint main(void) {\n"
                   + "  printf(\"%zu\\n\", sizeof(rnb_mesh_distance_options));\n" + "".join("  printf(\"%%zu\\n\", offsetof(rnb_mesh_distance_options, %s));\n" % n for n in of)
                   + "  printf(\"%zu\\n\", sizeof(rnb_mesh_distance_stats));\n" + "".join("  printf(\"%%zu\\n\", offsetof(rnb_mesh_distance_stats, %s));\n" % n for n in sf)
                   + "  printf(\"%d %u %d %u %u %u %u %llu %d %d\\n\", RNB_MESH_DISTANCE_ABI_VERSION, RNB_MESH_DISTANCE_MAX_LEVEL, RNB_MESH_DISTANCE_MAX_TAUS, RNB_MESH_DISTANCE_NONE,\n"
                   "         RNB_MESH_DISTANCE_MAX_CELLS, RNB_MESH_DISTANCE_LARGE_CELLS, RNB_MESH_DISTANCE_MAX_LARGE, (unsigned long long)RNB_MESH_DISTANCE_MAX_ENTRIES, RNB_MESH_DISTANCE_Q_SHIFT,\n"
                   "         RNB_MESH_DISTANCE_Q_TERM_LOG2);\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = [C.sizeof(O)] + [getattr(O, n).offset for n in of] + [C.sizeof(S)] + [getattr(S, n).offset for n in sf]
    assert out[:len(want)] == want
    assert out[len(want):] == [_abi.MESH_DISTANCE_ABI_VERSION, _abi.MESH_DISTANCE_MAX_LEVEL, _abi.MESH_DISTANCE_MAX_TAUS, _abi.MESH_DISTANCE_NONE, _abi.MESH_DISTANCE_MAX_CELLS,
                                _abi.MESH_DISTANCE_LARGE_CELLS, _abi.MESH_DISTANCE_MAX_LARGE, _abi.MESH_DISTANCE_MAX_ENTRIES, _abi.MESH_DISTANCE_Q_SHIFT, _abi.MESH_DISTANCE_Q_TERM_LOG2]
    assert (dr.Q_SHIFT, dr.Q_TERM_LOG2) == (_abi.MESH_DISTANCE_Q_SHIFT, _abi.MESH_DISTANCE_Q_TERM_LOG2)
    assert (dr.MAX_LEVEL, dr.MAX_TAUS, dr.NONE, dr.MAX_CELLS, dr.LARGE_CELLS, dr.MAX_LARGE) == (_abi.MESH_DISTANCE_MAX_LEVEL, _abi.MESH_DISTANCE_MAX_TAUS, _abi.MESH_DISTANCE_NONE,
                                                                                               _abi.MESH_DISTANCE_MAX_CELLS, _abi.MESH_DISTANCE_LARGE_CELLS, _abi.MESH_DISTANCE_MAX_LARGE)


# ------------------------------------------------------------------------------------------------------------------------ rule 2
def test_rule_2_on_one_triangle_in_each_region_and_on_the_boundaries():
    v, _ = UNIT_TRI
    a, b, c = v.astype(np.float64)
    cases = [  # point, s, region (0 a, 1 b, 2 ab, 3 c, 4 ac, 5 bc, 6 face): every answer is exactly representable
        ((0.25, 0.25, 2), 4, 6), ((-1, -1, 0), 2, 0), ((0.5, -3, 0), 9, 2), ((2, 2, 0), 4.5, 5), ((3, -1, 0), 5, 1), ((-1, 3, 0), 5, 3), ((-2, 0.5, 0), 4, 4),
        ((0.25, 0.25, 0), 0, 6), ((0.5, -3, 4), 25, 2), ((2, 2, 1), 5.5, 5),
        # on region boundaries: the first test that holds decides
        ((0, 0, 1), 1, 0),        # above a: the vertex test comes first
        ((1, 0, 1), 1, 1),        # above b
        ((0, 1, 1), 1, 3),        # above c
        ((0.5, 0, 1), 1, 2),      # above the edge ab (vc == 0): the edge test comes before the face
        ((0, 0.5, 1), 1, 4),      # above ac
        ((0.5, 0.5, 1), 1, 5),    # above bc
        ((-1, 0, 0), 1, 0),       # d1 < 0, d2 == 0: between the regions of a and of ac
        ((1, -1, 0), 1, 1),       # d3 == 0: between the regions of b and of ab
        ((2, 0, 0), 1, 1),        # d4 == d3... beyond b along ab
    ]
    for p, s, region in cases:
        got, reg = dr.point_triangle(np.array(p, np.float64), a, b, c)
        assert float(got) == float(s) and int(reg) == region, (p, float(got), int(reg))
    # a permutation of the corners is another triangle to rule 2, but the same set of points: equal s on these exactly representable cases
    for p, s, _ in cases:
        assert float(dr.point_triangle(np.array(p, np.float64), b, c, a)[0]) == float(s) == float(dr.point_triangle(np.array(p, np.float64), c, a, b)[0])


# ------------------------------------------------------------------------------------------------------------------------ rule 4
def test_rule_4_weights_sum_to_the_area_and_points_to_the_centroid():
    v = np.array([(0.125, 0.25, 0.5), (1.75, 0.5, 0.25), (0.5, 2.25, 1.5), (0.125, 0.25, 0.5)], np.float32)
    idx = np.array([0, 1, 2, 0, 3, 1], np.uint32)  # the second one is degenerate (two equal corners)
    a, b, c = v[:3].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a))
    for level in range(4):
        p, w, tri, n_deg = dr.samples(v, idx, level)
        n = 1 << level
        assert len(p) == n * n == len(w) and n_deg == 1 and set(tri) == {0}
        assert abs(w.sum() - area) <= 4 * np.spacing(area) and np.all(w == w[0])
        assert np.abs((w[:, None] * p).sum(0) - area * (a + b + c) / 3).max() <= 1e-14
        assert len(np.unique(p, axis=0)) == n * n
        # every sample lies strictly inside the triangle: s to it is 0 up to rounding and the face decides
        s, region = dr.point_triangle(p, a, b, c)
        assert s.max() < 1e-28 and np.all(region == 6)
    assert np.array_equal(dr.samples(v, idx, 0)[0][0], (a * (1 / 3) + b * (1 / 3)) + c * (1 / 3))


# ------------------------------------------------------------------------------------------------------------------------ (ii) == (i)
spheres = dr.concentric_spheres


def _same(x, y):
    return np.asarray(x, np.float64).tobytes() == np.asarray(y, np.float64).tobytes()


def test_shell_search_equals_the_definition_on_spheres():
    (ov, oi), (iv, ii) = spheres()
    rng = np.random.default_rng(11)
    sub = dr.samples(ov, oi, 1)[0]
    pts = np.concatenate([sub[rng.choice(len(sub), 300, replace=False)], iv[rng.choice(len(iv), 100, replace=False)].astype(np.float64),
                          rng.uniform(-1, 2, (150, 3)), rng.uniform(-20, 20, (50, 3))])
    tgt, n_deg = dr.target(iv, ii)
    assert n_deg == 0
    s, t = dr.nearest(pts, tgt, prune=False)
    fast = dr.nearest(pts, tgt)
    assert _same(fast[0], s) and np.array_equal(fast[1], t)  # the pruning of the reference's exhaustive minimum changes no bit
    assert np.all(s[300:400] == 0)  # the vertices of B lie on B
    for cells in (1, 4, 16):
        g = dr.Grid(iv, ii, cells)
        assert g.dims.max() == cells and g.n_entries >= len(tgt[3]) and not g.large
        res = [g.query(p) for p in pts]
        assert _same([r[0] for r in res], s), cells
        assert np.array_equal([r[1] for r in res], t), cells
        if cells == 16:  # the samples on B stop after shell 1
            assert max(r[3] for r in res[300:400]) == 1


@pytest.mark.parametrize("case", dr.stop_rule_cases(), ids=lambda c: c[0])
def test_shell_search_equals_the_definition_on_hand_made_cases(case):
    _, bv, bi, cells, pts = case
    s, t = dr.nearest(pts, dr.target(bv, bi)[0])
    for n in (cells, 2 * cells, 1):
        g = dr.Grid(bv, bi, n)
        res = [g.query(p) for p in pts]
        assert _same([r[0] for r in res], s) and np.array_equal([r[1] for r in res], t), n
    if case[0] == "diagonal":
        assert t[0] == 4 and s[0] == 3 * 1.0625 ** 2  # the quad of shell 2 wins over the triangles of shell 1; its two triangles tie in their shared corner
        assert dr.Grid(bv, bi, 4).query(pts[0])[3] == 2
    if case[0] == "exactly r cells":
        assert list(s) == [4.0, 1.0, 6.25, 9.0] and list(t) == [4, 4, 4, 4]


# ------------------------------------------------------------------------------------------------------------------------ the metric on two concentric spheres
@functools.lru_cache(maxsize=None)
def sphere_distances():
    (ov, oi), (iv, ii) = spheres()
    return dr.expected(ov, oi, iv, ii, level=0), dr.expected(iv, ii, ov, oi, level=0)


def test_concentric_spheres_are_their_radius_difference_apart():
    """Radii 0.30 and 0.25: the mean distance in each direction is within 3e-3 of 0.05 -- the sagitta e^2 / 8r = 1.5e-3 of a chord of at most sqrt(3) / 32 on the smaller
    sphere, once per mesh -- and every sample lies in [0.0489, 0.0513]."""
    for e in sphere_distances():
        m = dr.summary(e["stats"])
        print("mean %.5f rms %.5f max %.5f, samples %.5f .. %.5f" % (m["mean"], m["rms"], e["stats"]["max_distance"], e["sample_d"].min(), e["sample_d"].max()))
        assert abs(m["mean"] - 0.05) <= 3e-3 and abs(m["rms"] - 0.05) <= 3e-3
        used = e["vert_nearest"] != dr.NONE
        assert 0.0489 <= min(e["sample_d"].min(), e["vert_dist"][used].min()) and max(e["sample_d"].max(), e["vert_dist"][used].max()) <= 0.0513
        assert e["stats"]["max_distance"] == max(e["sample_d"].max(), np.sqrt(e["vert_s"][used]).max())
        # the quantisation bound of rule 5 against the float sum
        exact = float((e["sample_w"] * (e["sample_d"] / 2.0 ** -10)).sum())
        assert 0 <= exact - e["stats"]["sum_wd"] * 2.0 ** -48 <= e["stats"]["n_samples"] * 2.0 ** -48 + 1e-12 * exact


def test_the_cap_on_concentric_spheres():
    (ov, oi), (iv, ii) = spheres()
    free = sphere_distances()[0]
    low = dr.expected(ov, oi, iv, ii, level=0, max_distance=0.04, taus=(0.04, 0.039))
    st = low["stats"]
    assert st["n_beyond"] == st["n_samples"] == 3456 and st["n_verts_beyond"] == st["n_verts_from_used"] and np.all(low["vert_nearest"] == dr.NONE)
    D = float(np.float32(0.04))
    assert st["max_distance"] == D and np.all(low["vert_dist"] == np.float32(0.04))
    w = low["sample_w"]
    assert st["sum_w"] == free["stats"]["sum_w"] == dr._q(w) and st["sum_wd"] == dr._q(w * (D / 2.0 ** -10)) and st["sum_wd2"] == dr._q((w * (D / 2.0 ** -10)) * (D / 2.0 ** -10))
    assert st["sum_within"] == [st["sum_w"], 0, 0, 0]  # d == D is within tau == D; nothing is within 0.039
    high = dr.expected(ov, oi, iv, ii, level=0, max_distance=0.06)
    assert high["stats"] == free["stats"] and high["vert_dist"].tobytes() == free["vert_dist"].tobytes() and np.array_equal(high["vert_nearest"], free["vert_nearest"])
    # the search with the cap: the same capped results from every grid
    sub = slice(0, None, 37)
    for cells in (1, 16):
        g = dr.Grid(iv, ii, cells)
        for cap, ref in ((0.04, low), (0.06, high)):
            used = np.nonzero(ref["vert_nearest"] != dr.NONE if cap > 0.05 else np.ones(len(ov), bool))[0][sub]
            s, t = g.search(cap)(ov[used].astype(np.float64))
            d, t, _ = dr.capped(s, t, cap)
            assert d.astype(np.float32).tobytes() == ref["vert_dist"][used].tobytes() and np.array_equal(t, ref["vert_nearest"][used])


def test_reference_refuses_what_the_call_refuses():
    v, i = UNIT_TRI
    with pytest.raises(ValueError):
        dr.expected(v, [0, 1, 3], v, i)
    with pytest.raises(ValueError):
        dr.expected(v, i, v, [0, 1])
    with pytest.raises(ValueError):
        dr.expected(v, i, v, [0, 0, 1])  # B of only degenerate triangles
    bad = v.copy()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError):
        dr.expected(v, i, bad, i)
    with pytest.raises(ValueError):
        dr.expected(v * 8, i, v + np.float32(64), i)  # w = 8 per sample, d' about 1e5: over the term bound -- a larger unit
    assert dr.expected(v * 8, i, v + np.float32(64), i, unit=64.0)["stats"]["sum_w"] == 32 << 48
    e = dr.expected(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), v, i)  # an empty A: zero sums
    assert e["stats"]["sum_w"] == 0 and e["stats"]["n_samples"] == 0 and np.all(e["vert_nearest"] == dr.NONE) and np.all(e["vert_dist"] == 0)
    e = dr.expected(np.concatenate([v, [[np.nan] * 3]]).astype(np.float32), [0, 1, 2, 0, 0, 1], v + np.float32(1), [0, 1, 2, 2, 2, 1], level=2, unit=1.0)  # degenerate ones on both sides
    assert (e["stats"]["n_degenerate_from"], e["stats"]["n_degenerate_to"], e["stats"]["n_samples"], e["stats"]["n_verts_from_used"]) == (1, 1, 16, 3)
    assert e["vert_nearest"].tolist() == [0, 0, 0, dr.NONE]


# ------------------------------------------------------------------------------------------------------------------------ the tools' own arithmetic
def test_mesh_eval_chooses_its_unit_and_checks_its_arguments():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mesh_eval
    finally:
        sys.path.pop(0)
    assert [mesh_eval.choose_unit(x) for x in (1.0, 1.7, 2.0, 300.0, 0.75)] == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.25, 2.0 ** -11]
    for bad in (0.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            mesh_eval.choose_unit(bad)
    for bad in (["--tau", "-1"], ["--tau", "1", "2", "3", "4", "5"], []):
        with pytest.raises(SystemExit):
            mesh_eval.main(["--mesh", "a.obj"] + (["--reference", "b.obj"] + bad if bad else []))
