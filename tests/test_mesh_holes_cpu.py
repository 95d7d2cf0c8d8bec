"""CPU tier of the hole stage (include/rnb_mesh_holes.h): the numpy statement of tests/mesh_holes_reference.py against numbers known by hand, the C-ABI of the new
header (exports, version, defaults, struct layout, argument validation without a device), the calls the Python layer makes (through a recording stand-in of the function
table), and the command-line / pipeline surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_holes_reference as hr
from tests import mesh_topology_reference as tr

from rnb_neus2_amd import _abi as _ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_holes.h")
assert (hr.MAX_EDGES, hr.NONE) == (_ABI.MESH_HOLES_MAX_EDGES, _ABI.MESH_TOPOLOGY_NONE)  # the statement and the Python layer speak of the same stage


def _walk(r, label):
    """The half-edges of a simple loop in the order next gives them, from its label."""
    out, h = [], int(label)
    while True:
        out.append(h)
        h = int(r["next"][h])
        if h == label:
            return out


def _topology(f):
    return tr.expected_topology(len(f["verts"]), f["indices"])["stats"]


# ------------------------------------------------------------------------------------------------------------------------ the statement
def test_loops_known_by_hand():
    v, t = tr.disc(9)
    r = hr.expected_boundary_loops(v, t)
    assert r["stats"] == dict(n_boundary_edges=9, n_loops=1, n_simple=1, n_irregular_vertices=0, max_loop_edges=9, n_too_long=0)
    rec = r["table"][0]
    assert (rec["label"], rec["n_edges"], rec["simple"], rec["n_irregular"], rec["component"]) == (1, 9, 1, 0, 0)  # half-edge 1: triangle 0, from vertex 1 to vertex 2
    loop = _walk(r, 1)
    assert loop == [3 * k + 1 for k in range(9)] and list(r["pos"][loop]) == list(range(9)) and (r["loop"][loop] == 1).all()
    rest = np.setdiff1d(np.arange(27), loop)
    assert (r["loop"][rest] == hr.NONE).all() and (r["next"][rest] == hr.NONE).all() and (r["pos"][rest] == hr.NONE).all()
    # a regular nonagon of radius 0.3 around (.5, .5, .5) in the plane z = .5, run counter-clockwise by the faces: the fill side looks down
    assert np.allclose(rec["centroid"], [0.5, 0.5, 0.5], atol=1e-7) and np.allclose(rec["normal"], [0, 0, -1], atol=1e-7)
    assert abs(rec["area"] - 4.5 * 0.09 * np.sin(2 * np.pi / 9)) < 1e-7 and abs(rec["perimeter"] - 18 * 0.3 * np.sin(np.pi / 9)) < 1e-6
    v, t = tr.annulus(12)
    r = hr.expected_boundary_loops(v, t)
    assert r["stats"]["n_loops"] == 2 and r["stats"]["n_simple"] == 2 and list(r["table"]["n_edges"]) == [12, 12] and list(r["table"]["component"]) == [0, 0]
    assert np.allclose(r["table"]["normal"], [[0, 0, -1], [0, 0, 1]], atol=1e-6)  # the inner rim and the outer rim face opposite ways
    assert np.allclose(r["table"]["area"], [6 * 0.04 * np.sin(np.pi / 6), 6 * 0.09 * np.sin(np.pi / 6)], atol=1e-7)
    for label in r["table"]["label"]:
        assert len(_walk(r, label)) == 12
    v, t = tr.moebius(16)
    r = hr.expected_boundary_loops(v, t)  # one boundary component of 32 edges; the closing cell is wound against its neighbours, so two of its vertices are irregular
    assert r["stats"]["n_loops"] == 1 and list(r["table"]["n_edges"]) == [32] and r["stats"]["n_simple"] == 0 and r["stats"]["n_irregular_vertices"] == 2
    assert (r["next"] == hr.NONE).all() and (r["pos"] == hr.NONE).all() and (r["loop"] != hr.NONE).sum() == 32
    f = hr.expected_fill(v, t)
    assert f["stats"]["n_filled"] == 0 and f["stats"]["n_skipped_not_simple"] == 1 and f["indices"].tobytes() == t.astype(np.uint32).tobytes()
    for v, t in (tr.cube(), tr.torus_grid(8), (np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int64))):
        r = hr.expected_boundary_loops(v, t)
        assert r["stats"]["n_loops"] == 0 and len(r["table"]) == 0 and (r["loop"] == hr.NONE).all()
        f = hr.expected_fill(v, t)
        assert f["verts"].tobytes() == v.tobytes() and len(f["indices"]) == 3 * len(t) and f["stats"]["n_tris_added"] == 0


def test_the_cube_gets_its_face_back():
    v, t = tr.cube()
    pv, pt = hr.punch(v, t, [3])
    r = hr.expected_boundary_loops(pv, pt)
    assert list(r["table"]["n_edges"]) == [3] and r["stats"]["n_simple"] == 1
    f = hr.expected_fill(pv, pt)
    assert f["stats"]["n_verts_added"] == 0 and f["stats"]["n_tris_added"] == 1 and len(f["verts"]) == 8 and len(f["indices"]) == 36
    new = f["indices"].reshape(-1, 3)[-1]
    assert sorted(new) == sorted(t[3]) and tr._vertex_sets(np.array([new, t[3]], np.int64), np.ones(2, bool))[2].tolist() in ([0, 0], [1, 1])  # the same triangle, the same winding
    s = _topology(f)
    assert (s["closed"], s["oriented"], s["euler"], s["n_tris"]) == (1, 1, 2, 12)
    pv, pt = hr.punch(v, t, [4, 5])  # the face y = 0.25
    r = hr.expected_boundary_loops(pv, pt)
    assert list(r["table"]["n_edges"]) == [4]
    f = hr.expected_fill(pv, pt)
    assert (f["stats"]["n_verts_added"], f["stats"]["n_tris_added"], f["stats"]["n_verts_out"], f["stats"]["n_tris_out"]) == (1, 4, 9, 14)
    assert f["verts"][8].tolist() == [0.5, 0.25, 0.5] and (f["indices"].reshape(-1, 3)[-4:, 2] == 8).all()
    assert np.allclose(r["table"]["normal"][0], [0, -1, 0]) and abs(r["table"]["area"][0] - 0.25) < 1e-12 and abs(r["table"]["perimeter"][0] - 2.0) < 1e-12
    s = _topology(f)
    assert (s["closed"], s["oriented"], s["euler"]) == (1, 1, 2)
    assert (f["loop_of_tri"][:10] == hr.NONE).all() and (f["loop_of_tri"][10:] == r["table"]["label"][0]).all()
    col, nrm = hr.coloured(pv, 2)
    f = hr.expected_fill(pv, pt, col, nrm)
    rim = np.unique(t[[4, 5]])
    assert np.allclose(f["colors"][8], col[rim].mean(0), atol=1e-6) and np.allclose(f["normals"][8], [0, -1, 0]) and f["colors"][:8].tobytes() == col.tobytes()


def test_a_pinch_and_an_inconsistent_rim_are_reported_and_left_open():
    v, t = tr.sphere(32)
    p, q, r_ = hr.touching_fans(t)
    shared = np.intersect1d(hr.neighbours(t, p), hr.neighbours(t, q))
    assert len(shared) == 1
    pv, pt = hr.punch_vertex_fans(v, t, [p, q, r_])
    r = hr.expected_boundary_loops(pv, pt)
    assert r["stats"]["n_loops"] == 2 and r["stats"]["n_simple"] == 1 and r["stats"]["n_irregular_vertices"] == 1
    pinch = r["table"][r["table"]["simple"] == 0][0]
    assert pinch["n_irregular"] == 1 and pinch["n_edges"] == len(hr.neighbours(t, p)) + len(hr.neighbours(t, q))
    f = hr.expected_fill(pv, pt)
    assert (f["stats"]["n_filled"], f["stats"]["n_skipped_not_simple"]) == (1, 1) and f["stats"]["n_tris_added"] == len(hr.neighbours(t, r_))
    s = _topology(f)
    assert s["n_boundary_edges"] == pinch["n_edges"] and s["n_boundary_components"] == 1  # the third fan is closed, the pinched pair is as it was
    sv, st = tr.strip(40)
    st = tr.flip_some(st, 0.4, 40)
    r = hr.expected_boundary_loops(sv, st)
    assert r["stats"]["n_loops"] == 1 and r["stats"]["n_simple"] == 0 and r["stats"]["n_irregular_vertices"] > 0
    assert hr.expected_fill(sv, st)["stats"]["n_filled"] == 0
    fixed = tr.expected_repair(sv, st, orient="consistent")  # what the header tells the user to run first
    r = hr.expected_boundary_loops(fixed["verts"], fixed["indices"])
    assert r["stats"]["n_simple"] == 1 and r["stats"]["max_loop_edges"] == 42


def test_skip_largest_and_max_edges():
    v, t = tr.disc(9)
    f = hr.expected_fill(v, t, skip_largest=True)
    assert f["stats"]["n_filled"] == 0 and f["stats"]["n_skipped_largest"] == 1 and len(f["indices"]) == 27
    v, t, k = hr.grid_sheet_with_holes(24, 24)
    r = hr.expected_boundary_loops(v, t)
    assert r["stats"]["n_loops"] == k + 1 == 50 and sorted(set(r["table"]["n_edges"])) == [3, 4, 6, 96]
    f = hr.expected_fill(v, t, skip_largest=True)
    assert f["stats"]["n_filled"] == k and f["stats"]["n_skipped_largest"] == 1
    s = _topology(f)
    assert s["n_boundary_components"] == 1 and s["n_boundary_edges"] == 96  # exactly the rim
    for limit, filled in ((3, 17), (4, 33), (6, 49), (95, 49), (96, 50)):
        st = hr.expected_fill(v, t, max_edges=limit)["stats"]
        assert (st["n_filled"], st["n_skipped_over_max"]) == (filled, 50 - filled), limit
    st = hr.expected_fill(v, t, max_edges=4, skip_largest=True)["stats"]  # the rim is over the limit: it is counted there, and no other loop is the largest
    assert (st["n_filled"], st["n_skipped_over_max"], st["n_skipped_largest"]) == (33, 17, 0)


FILLABLE = {
    "disc": lambda: tr.disc(9), "annulus": lambda: tr.annulus(12), "cube_minus_1": lambda: hr.punch(*tr.cube(), [3]), "cube_minus_face": lambda: hr.punch(*tr.cube(), [4, 5]),
    "sphere_fans": lambda: hr.punch_vertex_fans(*tr.sphere(32), [5, 900, 1500]), "sphere_tris": lambda: hr.punch(*tr.sphere(32), [0, 1000, 2000]),
    "sheet": lambda: hr.grid_sheet_with_holes(24, 24)[:2], "disc_257": lambda: tr.disc(257), "torus_minus_cell": lambda: hr.punch(*tr.torus_grid(8), [9, 64 + 9]),
}


@pytest.mark.parametrize("name", sorted(FILLABLE))
def test_a_fill_closes_what_is_fillable(name):
    """A condition, not a measurement: where every boundary component is a simple loop, the filled mesh is closed and consistently wound, and every fill is a disc: the
    Euler number rises by one per filled loop."""
    v, t = FILLABLE[name]()
    before = tr.expected_topology(len(v), t)["stats"]
    assert before["oriented"] == 0 and before["n_inconsistent_edges"] == 0 and before["n_boundary_edges"] > 0
    loops = hr.expected_boundary_loops(v, t)["stats"]
    assert loops["n_simple"] == loops["n_loops"] == before["n_boundary_components"]
    f = hr.expected_fill(v, t)
    after = _topology(f)
    assert after["closed"] == 1 and after["oriented"] == 1 and after["euler"] == before["euler"] + f["stats"]["n_filled"] and f["stats"]["n_filled"] == loops["n_loops"]
    assert f["indices"][:3 * len(t)].tobytes() == np.asarray(t, np.uint32).tobytes() and f["verts"][:len(v)].tobytes() == v.tobytes()  # the input comes first, unchanged


def test_the_statement_does_not_depend_on_the_order_of_the_triangles():
    v, t, _ = hr.grid_sheet_with_holes(12, 12)
    col, _n = hr.coloured(v, 4)
    a = hr.expected_boundary_loops(v, t, col)
    perm = np.random.default_rng(3).permutation(len(t))
    b = hr.expected_boundary_loops(v, t[perm], col)
    # the labels move with the triangles, and with them the order of the records and the anchor o: what does not involve o is equal, the rest equal to rounding
    drop = lambda tab: np.sort(tab[["n_edges", "simple", "n_irregular", "component", "perimeter"]], axis=0)
    assert a["stats"] == b["stats"] and np.array_equal(drop(a["table"]), drop(b["table"]))
    # (every term of a sum is truncated to 2^-32 and the longest loop has 48 edges: the area vectors agree to 48 * 2^-32 per axis, the areas to less than that)
    assert np.allclose(np.sort(a["table"]["area"]), np.sort(b["table"]["area"]), rtol=0, atol=48 * 2.0 ** -32)
    with pytest.raises(ValueError):
        far = v.copy()
        far[0, 0] = 2.0 ** 11
        hr.expected_boundary_loops(far, t)
    with pytest.raises(ValueError):
        nan = v.copy()
        nan[0, 2] = np.nan
        hr.expected_boundary_loops(nan, t)


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


def test_holes_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = _functions(HEADER)
    assert names == ["rnb_mesh_boundary_loops", "rnb_mesh_boundary_loops_default_options", "rnb_mesh_boundary_loops_free", "rnb_mesh_fill_holes", "rnb_mesh_fill_holes_default_options",
                     "rnb_mesh_holes_abi_version"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_HOLES_PROTOTYPES) == set(names)
    others = [getattr(_abi, n) for n in dir(_abi) if n.endswith("PROTOTYPES") and n != "MESH_HOLES_PROTOTYPES"]
    assert len(others) >= 11 and not any(set(_abi.MESH_HOLES_PROTOTYPES) & set(o) for o in others)  # a table of its own
    fns = api.load_library()
    assert fns.mesh_holes_abi_version() == _abi.MESH_HOLES_ABI_VERSION == 1
    o = _abi.MeshBoundaryLoopsOptions()
    assert fns.mesh_boundary_loops_default_options(C.byref(o)) == 0 and (o.abi_version, o.buckets_log2, list(o.reserved)) == (1, 0, [0] * 4)
    f = _abi.MeshFillHolesOptions()
    assert fns.mesh_fill_holes_default_options(C.byref(f)) == 0 and (f.abi_version, f.max_edges, f.skip_largest, f.buckets_log2, list(f.reserved)) == (1, 0, 0, 0, [0] * 4)
    assert fns.mesh_boundary_loops_default_options(None) == _abi.ERR_INVALID and fns.mesh_fill_holes_default_options(None) == _abi.ERR_INVALID
    for name in ("mesh_boundary_loops", "fill_mesh_holes"):
        assert hasattr(api.Context, name)
    for name in ("boundary_loops", "fill_holes"):
        assert hasattr(api.DeviceMesh, name)
    from rnb_neus2_amd import build
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS


def test_holes_validate_their_arguments_without_a_device():
    """Null pointers, a wrong version, skip_largest > 1, reserved words, buckets_log2 outside 0, 4 .. 30, n_indices % 3, null buffers and in == out are refused before the
    context or the device is touched: the context handed in here is a block of zeros, and no device exists where this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def lopt(**kw):
        o = _abi.MeshBoundaryLoopsOptions()
        assert fns.mesh_boundary_loops_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def fopt(**kw):
        o = _abi.MeshFillHolesOptions()
        assert fns.mesh_fill_holes_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def census(ctx_, m, o, tab=None):
        return fns.mesh_boundary_loops(ctx_, None, m, o, None, None, None, tab, None)

    def fill(ctx_, m, o, out):
        return fns.mesh_fill_holes(ctx_, None, m, o, out, None, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    E = _abi.ERR_INVALID
    assert census(None, C.byref(src), C.byref(lopt())) == E and census(ctx, None, C.byref(lopt())) == E and census(ctx, C.byref(src), None) == E
    assert b"rnb_mesh_boundary_loops" in fns.last_error()
    assert fill(None, C.byref(src), C.byref(fopt()), C.byref(dst)) == E and fill(ctx, None, C.byref(fopt()), C.byref(dst)) == E
    assert fill(ctx, C.byref(src), None, C.byref(dst)) == E and fill(ctx, C.byref(src), C.byref(fopt()), None) == E and b"rnb_mesh_fill_holes" in fns.last_error()
    assert fill(ctx, C.byref(src), C.byref(fopt()), C.byref(src)) == E and b"different objects" in fns.last_error() and b"rnb_mesh_fill_holes" in fns.last_error()  # in place
    res4 = (C.c_uint32 * 4)(0, 0, 1, 0)
    for kw in (dict(abi_version=2), dict(abi_version=0), dict(buckets_log2=3), dict(buckets_log2=1), dict(buckets_log2=31), dict(reserved=res4)):
        tab = C.c_void_p(1)
        assert census(ctx, C.byref(src), C.byref(lopt(**kw)), C.byref(tab)) == E and not tab.value, kw
        assert b"rnb_mesh_boundary_loops" in fns.last_error()
    for kw in (dict(abi_version=2), dict(abi_version=0), dict(skip_largest=2), dict(skip_largest=0xFFFFFFFF), dict(buckets_log2=3), dict(buckets_log2=31), dict(reserved=res4)):
        dst.n_verts = 7
        assert fill(ctx, C.byref(src), C.byref(fopt(**kw)), C.byref(dst)) == E, kw
        assert dst.n_verts == 0 and not dst.verts and b"rnb_mesh_fill_holes" in fns.last_error()  # zeroed on failure
    src.n_indices, src.n_verts = 4, 3  # not a multiple of 3
    assert census(ctx, C.byref(src), C.byref(lopt())) == E and b"multiple of 3" in fns.last_error() and fill(ctx, C.byref(src), C.byref(fopt()), C.byref(dst)) == E
    src.n_indices = 3  # null buffers
    assert census(ctx, C.byref(src), C.byref(lopt())) == E and fill(ctx, C.byref(src), C.byref(fopt()), C.byref(dst)) == E
    assert fns.mesh_boundary_loops_free(None, None) == E
    assert fake.raw == b"\0" * 4096


def test_holes_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = {"rnb_mesh_boundary_loops_options": _abi.MeshBoundaryLoopsOptions, "rnb_mesh_boundary_loop": _abi.MeshBoundaryLoop, "rnb_mesh_boundary_loops_stats": _abi.MeshBoundaryLoopsStats,
               "rnb_mesh_fill_holes_options": _abi.MeshFillHolesOptions, "rnb_mesh_fill_holes_stats": _abi.MeshFillHolesStats}
    lines, want = [], []
    for cname, S in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(S))
        for field, _ in S._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
            want.append(getattr(S, field).offset)
    for name in ("RNB_MESH_HOLES_ABI_VERSION", "RNB_MESH_HOLES_MAX_EDGES", "RNB_MESH_HOLES_Q_SHIFT", "RNB_MESH_HOLES_Q_TERM_LOG2"):
        lines.append('printf("%%llu\\n", (unsigned long long)%s);' % name)
        want.append(getattr(_abi, name[4:]))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnb_mesh_holes.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want
    dt, T = np.dtype(_abi.MESH_BOUNDARY_LOOP_DTYPE), _abi.MeshBoundaryLoop
    assert dt == hr.TABLE_DTYPE and dt.itemsize == C.sizeof(T) == 64 and [dt.fields[n][1] for n in dt.names] == [getattr(T, n).offset for n in dt.names]
    assert (hr.MAX_EDGES, hr.Q_SCALE, hr.TERM_LIMIT) == (_abi.MESH_HOLES_MAX_EDGES, 2.0 ** _abi.MESH_HOLES_Q_SHIFT, 2.0 ** _abi.MESH_HOLES_Q_TERM_LOG2)
    assert set(hr.LOOPS_STATS) | {"peak_workspace", "ms"} == set(_abi.MeshBoundaryLoopsStats().as_dict())
    assert set(hr.FILL_STATS) | {"peak_workspace", "ms"} == set(_abi.MeshFillHolesStats().as_dict())


# ------------------------------------------------------------------------------------------------------------------------ the calls of the Python layer
DEVICE_CALLS = ("extract_mesh", "mesh_clean", "mesh_simplify", "mesh_distance", "mesh_topology", "mesh_repair", "mesh_boundary_loops", "mesh_fill_holes", "mesh_visibility",
                "mesh_visibility_select", "device_malloc", "device_free", "memcpy", "mesh_free", "mesh_clean_table_free", "mesh_topology_table_free", "mesh_boundary_loops_free")
MESH_ARGS = dict(extract_mesh=((), 3), mesh_clean=((2,), 4), mesh_simplify=((2,), 4), mesh_repair=((2,), 4), mesh_fill_holes=((2,), 4), mesh_topology=((2,), None),
                 mesh_boundary_loops=((2,), None), mesh_distance=((2, 3), None), mesh_free=((1,), None))


class RecordingLibrary:
    """A stand-in for the library's function table, after the one of tests/test_mesh_topology_cpu.py: every entry point returns 0 (`fail` names the one that returns
    ERR_INVALID instead); a call that returns a mesh fills it with made-up pointers; device_malloc and a table hand out made-up pointers; a download reads zeros. `log`
    holds (name, the `verts` pointers of the meshes passed, inputs then output); `buffers` and `meshes` what is handed out and not yet released, `errors` every release
    of something that is not."""

    def __init__(self, fail=None):
        self.fail, self.log, self.buffers, self.meshes, self.errors, self._next = fail, [], set(), set(), [], 0x1000

    def _ptr(self):
        self._next += 0x100
        return self._next

    def device_log(self):
        return [e for e in self.log if e[0] in DEVICE_CALLS]

    def names(self):
        return [e[0] for e in self.device_log()]

    def last_error(self):
        return b"made to fail"

    def __getattr__(self, name):
        from rnb_neus2_amd import _abi

        def call(*args):
            obj = lambda k: args[k]._obj
            if name == self.fail:
                self.log.append((name, ()))
                return _abi.ERR_INVALID
            ins, out = MESH_ARGS.get(name, ((), None))
            seen = tuple(obj(k).verts for k in ins)
            if name == "create":
                obj(1).value = self._ptr()
            elif name == "device_malloc":
                obj(2).value = self._ptr()
                self.buffers.add(obj(2).value)
            elif name == "memcpy" and args[4] == _abi.D2H:
                C.memset(args[1], 0, args[3])
            elif name in ("device_free", "mesh_clean_table_free", "mesh_topology_table_free", "mesh_boundary_loops_free"):
                self._release(self.buffers, args[1].value, name)
            elif name == "mesh_free":
                m = obj(1)
                if m.verts:
                    self._release(self.meshes, m.verts, name)
                C.memset(C.byref(m), 0, C.sizeof(_abi.Mesh))
            if out is not None:
                m = obj(out)
                src = obj(ins[0]) if ins else None
                m.verts, m.indices, m.n_indices = self._ptr(), self._ptr(), 9
                _abi.Mesh.n_verts.__set__(m, 5)
                if src.colors if src is not None else obj(2).attributes & _abi.MESH_ATTR_COLORS:
                    m.colors = self._ptr()
                self.meshes.add(m.verts)
                seen += (m.verts,)
                obj(len(args) - 1).ms = 0.5
            if name == "mesh_fill_holes":
                obj(6).n_filled = 3
                seen += (int(args[5] is not None), obj(3).max_edges, obj(3).skip_largest)
            if name in ("mesh_topology", "mesh_boundary_loops"):
                if name == "mesh_boundary_loops":
                    obj(8).n_loops = 2
                if args[7] is not None:
                    obj(7).value = self._ptr()
                    self.buffers.add(obj(7).value)
                seen += tuple(int(a is not None) for a in args[4:8])
            self.log.append((name, seen))
            return 0
        return call

    def _release(self, held, ptr, name):
        if ptr in held:
            held.remove(ptr)
        else:
            self.errors.append((name, ptr))


def _context(fail=None):
    from rnb_neus2_amd import _abi, api
    fake = RecordingLibrary(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
I = np.uint32([0, 1, 2, 0, 2, 3])
COL = np.full((4, 3), 0.5, np.float32)
UP = ["device_malloc", "memcpy"]

CALLS = {
    "mesh_boundary_loops": lambda c: c.mesh_boundary_loops(V, I, edges=True),
    "mesh_boundary_loops_stats_only": lambda c: c.mesh_boundary_loops(V, I, table=False),
    "fill_mesh_holes": lambda c: c.fill_mesh_holes(V, I, colors=COL, max_edges=7, skip_largest=True, loop_of_tri=True),
    "extract_mesh": lambda c: c.extract_mesh(16, simplify=8, error=True, colors=True, repair=dict(duplicates="cancel"), fill_holes=dict(max_edges=5), topology=True),
    "extract_mesh_defaults": lambda c: c.extract_mesh(16, fill_holes=True),
}
EXPECTED = {
    "mesh_boundary_loops": UP * 2 + ["device_malloc"] * 3 + ["mesh_boundary_loops"] + ["memcpy"] * 4 + ["mesh_boundary_loops_free"] + ["device_free"] * 3 + ["device_free"] * 2,
    "mesh_boundary_loops_stats_only": UP * 2 + ["mesh_boundary_loops"] + ["device_free"] * 2,
    "fill_mesh_holes": UP * 3 + ["device_malloc", "mesh_fill_holes", "memcpy", "device_free"] + ["device_free"] * 3 + ["memcpy"] * 3 + ["mesh_free"],
    "extract_mesh": ["extract_mesh", "mesh_simplify", "mesh_repair", "mesh_fill_holes", "mesh_distance", "mesh_distance", "mesh_topology"] + ["memcpy"] * 3 + ["mesh_free"] * 4,
    "extract_mesh_defaults": ["extract_mesh", "mesh_fill_holes"] + ["memcpy"] * 2 + ["mesh_free"] * 2,
}


def test_the_python_calls_make_the_expected_c_calls_in_order():
    for name, call in CALLS.items():
        c, fake = _context()
        call(c)
        assert fake.names() == EXPECTED[name], (name, fake.names())
        assert not fake.buffers and not fake.meshes and not fake.errors, name
    c, fake = _context()
    out = CALLS["mesh_boundary_loops"](c)
    assert out["n_loops"] == 2 and out["table"].dtype == hr.TABLE_DTYPE and len(out["table"]) == 2 and all(len(out[k]) == 6 for k in ("loop", "next", "pos"))
    assert [e for e in fake.log if e[0] == "mesh_boundary_loops"][0][1][1:] == (1, 1, 1, 1)  # the three arrays and the table were asked for
    c, fake = _context()
    out = CALLS["mesh_boundary_loops_stats_only"](c)
    assert [e for e in fake.log if e[0] == "mesh_boundary_loops"][0][1][1:] == (0, 0, 0, 0) and "table" not in out and "pos" not in out and "n_simple" in out
    c, fake = _context()
    out = CALLS["fill_mesh_holes"](c)
    assert [e for e in fake.log if e[0] == "mesh_fill_holes"][0][1][2:] == (1, 7, 1)  # loop_of_tri asked for; the options reach the C struct
    assert out["stats"]["n_filled"] == 3 and out["fill_stats"] is out["stats"] and len(out["loop_of_tri"]) == 3 and "colors" in out
    c, fake = _context()
    out = CALLS["extract_mesh"](c)
    log = {e[0]: e[1] for e in fake.device_log() if e[0].startswith("mesh_") and e[0] not in ("mesh_distance", "mesh_free")}
    assert log["mesh_fill_holes"][0] == log["mesh_repair"][1] and log["mesh_topology"][0] == log["mesh_fill_holes"][1]  # repair -> fill -> the census of the result
    assert log["mesh_fill_holes"][2:] == (0, 5, 0)
    dist = [e[1] for e in fake.device_log() if e[0] == "mesh_distance"]
    assert dist == [(log["mesh_simplify"][0], log["mesh_fill_holes"][1]), (log["mesh_fill_holes"][1], log["mesh_simplify"][0])]  # the error: simplifier's input <-> the filled mesh
    assert {"repair_stats", "simplify_stats", "fill_stats", "topology", "simplify_error"} <= set(out) and out["fill_stats"]["n_filled"] == 3
    # left off, extract_mesh makes the calls it made before
    c, fake = _context()
    out = c.extract_mesh(16, simplify=8, repair=dict(duplicates="cancel"), topology=True)
    assert fake.names() == ["extract_mesh", "mesh_simplify", "mesh_repair", "mesh_topology"] + ["memcpy"] * 2 + ["mesh_free"] * 3 and "fill_stats" not in out
    c, fake = _context()
    o = c._fill_holes_options(max_edges=12, skip_largest=True, buckets_log2=9)
    assert (o.max_edges, o.skip_largest, o.buckets_log2) == (12, 1, 9) and c._boundary_loops_options(5).buckets_log2 == 5
    for bad in (dict(fill_holes=dict(keep="largest")), dict(fill_holes=False), dict(fill_holes=3)):
        with pytest.raises(ValueError):
            c.extract_mesh(16, **bad)
    with pytest.raises(ValueError):
        c._fill_holes_options(max_edges=-1)
    assert not fake.device_log()


@pytest.mark.parametrize("stage", ["extract_mesh", "mesh_simplify", "mesh_repair", "mesh_fill_holes", "mesh_distance", "mesh_topology", "mesh_boundary_loops"])
def test_a_failing_stage_leaves_nothing_allocated(stage):
    from rnb_neus2_amd import _abi, api
    reached = 0
    for name, call in CALLS.items():
        c, fake = _context(fail=stage)
        try:
            call(c)
        except api.RnbError as e:
            assert e.code == _abi.ERR_INVALID
            reached += 1
            assert stage in [e[0] for e in fake.log], name
        else:
            assert stage not in [e[0] for e in fake.log], name
        assert not fake.buffers and not fake.meshes and not fake.errors, (name, fake.buffers, fake.meshes, fake.errors)
    assert reached >= 1
    c, fake = _context(fail=stage)
    with pytest.raises(api.RnbError):
        with c.extract_mesh_device(16, colors=True) as m, m.simplify((0, 0, 0), 0.25, 4) as sm, sm.repair() as rm, rm.fill_holes(loop_of_tri=True) as fm:
            fm.boundary_loops(edges=True)
            fm.topology()
            sm.distance_to(fm)
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_a_freed_handle_stops_in_python():
    c, fake = _context()
    m = c.upload_mesh(V, I, COL)
    f = m.fill_holes(loop_of_tri=True)
    assert isinstance(f.loop_of_tri, np.ndarray) and len(f.loop_of_tri) == 3 and f.has_colors and f.stats["ms"] == 0.5 and m.loop_of_tri is None
    assert m.boundary_loops()["n_loops"] == 2
    m.free()
    n = len(fake.log)
    for call in (lambda: m.boundary_loops(), lambda: m.boundary_loops(edges=True), lambda: m.fill_holes(), lambda: m.fill_holes(loop_of_tri=True)):
        with pytest.raises(ValueError):
            call()
    assert len(fake.log) == n
    f.free()
    with pytest.raises(ValueError):
        f.boundary_loops()
    assert not fake.buffers and not fake.meshes and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--fill-holes", "--fill-max-edges", "--fill-skip-largest"):
        assert flag in r.stdout, flag
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--fill-max-edges", "8"], ["--fill-skip-largest"], ["--fill-holes=1"], ["--fill-holes", "--fill-max-edges"], ["--fill-holes", "--fill-max-edges", "2"],
                ["--fill-holes", "--fill-max-edges", "x"], ["--fill-holes", "--fill-skip-largest=1"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    for good in (["--fill-holes"], ["--fill-holes", "--fill-max-edges", "64", "--fill-skip-largest"], ["--keep-seen", "faces", "--fill-holes", "--report-topology"],
                 ["--simplify", "8", "--repair", "--duplicates", "cancel", "--fill-holes", "--keep", "largest", "--orient", "outward", "--texture", "64"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, good  # the flags parse; the snapshot is what is missing


def test_the_pipeline_passes_the_flags_through():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    plain = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces")
    assert "--fill-holes" not in plain
    argv = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces", fill_holes=dict(max_edges=64, skip_largest=True))
    assert argv[:len(plain)] == plain and argv[len(plain):] == ["--fill-holes", "--fill-max-edges", "64", "--fill-skip-largest"]
    assert pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", fill_holes=True)[-1] == "--fill-holes"
    for bad in (dict(max_edges=2), dict(largest=True)):
        with pytest.raises(ValueError):
            pipeline.fill_holes_flags(bad)
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "tb", "out", fill_holes=True)
    common = ["-i", "in", "-t", "tb", "-o", "out"]
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--keep-seen", "faces", "--fill-holes", "--fill-max-edges", "64", "--fill-skip-largest"])
    assert run_pipeline.pipeline_kwargs(ns)["fill_holes"] == dict(max_edges=64, skip_largest=True)
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--fill-holes"])
    assert run_pipeline.pipeline_kwargs(ns)["fill_holes"] == dict(skip_largest=False)
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert "fill_holes" not in kw and "fill_max_edges" not in kw and "fill_skip_largest" not in kw
    for bad in (["--fill-holes"], ["--device-postprocess", "--fill-max-edges", "8"], ["--device-postprocess", "--fill-skip-largest"], ["--device-postprocess", "--fill-holes", "--fill-max-edges", "2"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(common + bad)


def test_the_bench_tool_uses_the_public_interface():
    with open(os.path.join(ROOT, "tools", "bench_mesh_holes.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and 'cull_unseen(' in text and 'unit="faces"' in text and ".boundary_loops(" in text and ".fill_holes(" in text and ".topology(" in text
    assert "mesh_holes_reference" in text and "Not measured" in text
