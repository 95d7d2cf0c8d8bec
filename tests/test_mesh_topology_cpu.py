"""CPU tier of the mesh topology stage (include/rnb_mesh_topology.h): the numpy statement of tests/mesh_topology_reference.py against numbers known by hand, the
C-ABI of the new header (exports, versions, defaults, struct layout, argument validation without a device), the calls the Python layer makes (through a recording
stand-in of the function table), and the command-line / pipeline surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_topology_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_topology.h")


def _stats(v, t):
    return tr.expected_topology(len(v), t)


# ------------------------------------------------------------------------------------------------------------------------ the statement
def test_closed_surfaces():
    for v, t in (tr.cube(), tr.tetrahedron()):
        r = _stats(v, t)
        s = r["stats"]
        assert (s["closed"], s["oriented"], s["euler"], s["n_components"], s["n_patches"], s["n_boundary_components"]) == (1, 1, 2, 1, 1, 0)
        assert s["n_edges"] == 3 * len(t) // 2 == s["n_manifold_edges"] and s["max_faces_on_edge"] == 2
        assert list(r["table"]["genus"]) == [0] and list(r["table"]["euler"]) == [2]
        assert (r["n_faces"] == 2).all() and (r["n_same"] == 1).all() and np.array_equal(r["mate"][r["mate"]], np.arange(3 * len(t)))
    v, t = tr.cube()
    assert (len(v), len(t)) == (8, 12)
    n = 16
    v, t = tr.torus_grid(n)
    r = _stats(v, t)
    assert (len(v), r["stats"]["n_edges"], len(t)) == (n * n, 3 * n * n, 2 * n * n)
    assert r["stats"]["euler"] == 0 and r["stats"]["oriented"] == 1 and list(r["table"]["genus"]) == [1]


def test_open_and_unorientable_surfaces():
    v, t = tr.moebius(16)
    r = _stats(v, t)
    s = r["stats"]
    assert len(t) == 32 and (s["n_patches"], s["n_unorientable_patches"], s["n_boundary_components"], s["closed"]) == (1, 1, 1, 0) and list(r["table"]["genus"]) == [-1]
    rep = tr.expected_repair(v, t, orient="consistent")  # reported and left as it came
    assert rep["stats"]["n_unorientable_patches"] == 1 and rep["stats"]["n_flipped"] == 0 and np.array_equal(rep["indices"].reshape(-1, 3), t)
    v, t = tr.annulus(12)
    s = _stats(v, t)["stats"]
    assert (s["n_boundary_components"], s["n_patches"], s["n_unorientable_patches"], s["n_inconsistent_edges"], s["euler"]) == (2, 1, 0, 0, 0)
    rep = tr.expected_repair(v, t, orient="consistent")
    assert rep["stats"]["n_flipped"] == 0 and np.array_equal(rep["indices"].reshape(-1, 3), t)
    v, t = tr.disc(9)
    s = _stats(v, t)["stats"]
    assert (s["n_boundary_components"], s["n_boundary_edges"], s["euler"]) == (1, 9, 1)
    v, t = tr.strip(257)
    s = _stats(v, t)["stats"]
    assert (s["n_inconsistent_edges"], s["n_manifold_edges"], s["n_boundary_edges"], s["n_boundary_components"]) == (0, 256, 259, 1)


def test_non_manifold_edges():
    v, t = tr.two_cubes_sharing_an_edge()
    r = _stats(v, t)
    s = r["stats"]
    assert (len(v), len(t)) == (14, 24)
    assert (s["n_nonmanifold_edges"], s["max_faces_on_edge"], s["euler"], s["n_patches"], s["n_components"], s["closed"]) == (1, 4, 3, 2, 1, 0)
    assert list(r["table"]["genus"]) == [-1] and (r["mate"][r["n_faces"] == 4] == tr.NONE).all() and (r["n_faces"] == 4).sum() == 4
    v, t = tr.book(7)
    r = _stats(v, t)
    assert r["stats"]["max_faces_on_edge"] == 7 and r["stats"]["n_patches"] == 7 and r["stats"]["n_boundary_edges"] == 14
    assert sorted(r["n_same"][r["n_faces"] == 7]) == [7] * 7  # every page runs the spine the same way


def test_degenerate_and_duplicate_triangles_by_hand():
    v = np.zeros((5, 3), np.float32)
    t = np.array([[0, 1, 2], [1, 2, 0], [0, 2, 1], [3, 3, 4], [2, 1, 0], [0, 1, 2]])  # even, even, odd, degenerate, odd, even
    r = _stats(v, t)
    s = r["stats"]
    assert (s["n_degenerate"], s["n_duplicate_tris"], s["n_folded_pairs"], s["n_edges"], s["max_faces_on_edge"], s["n_verts_used"], s["n_components"]) == (1, 4, 2, 3, 5, 5, 2)
    assert (r["n_faces"][9:12] == 0).all() and (r["mate"][9:12] == tr.NONE).all() and list(r["table"]["n_triangles"]) == [5, 0]
    assert s["euler"] == 5 - 3 + 5
    first = tr.expected_repair(v, t, duplicates="first")
    assert list(np.flatnonzero(first["tri_kept"])) == [0] and first["stats"]["n_degenerate_dropped"] == 1 and first["stats"]["n_duplicates_dropped"] == 4
    cancel = tr.expected_repair(v, t, duplicates="cancel")  # p = 3, m = 2: the lowest-numbered even one stays
    assert list(np.flatnonzero(cancel["tri_kept"])) == [0] and list(cancel["vertex_map"]) == [0, 1, 2, tr.NONE, tr.NONE]
    cancel = tr.expected_repair(v, t[[2, 4, 0]], duplicates="cancel", drop_degenerate=False)  # m = 2, p = 1: the lowest-numbered odd one
    assert list(np.flatnonzero(cancel["tri_kept"])) == [0]
    keep = tr.expected_repair(v, t, duplicates="keep", drop_degenerate=False)
    assert keep["tri_kept"].all() and np.array_equal(keep["indices"].reshape(-1, 3), t) and keep["stats"]["n_verts_out"] == 5


def test_the_clustered_thin_shapes():
    """The numbers of the thin slab and the thin torus after vertex clustering on 8^3 cells (tests/mesh_simplify_reference.expected)."""
    v, t = tr.clustered_slab()
    s = _stats(v, t)["stats"]
    assert (s["n_tris"], s["n_duplicate_tris"], s["n_folded_pairs"], s["n_nonmanifold_edges"], s["n_edges"], s["max_faces_on_edge"]) == (100, 50, 50, 65, 85, 4)
    cancel, first = tr.expected_repair(v, t, duplicates="cancel"), tr.expected_repair(v, t, duplicates="first")
    assert cancel["stats"]["n_tris_out"] == 0 and cancel["stats"]["n_verts_out"] == 0 and len(cancel["indices"]) == 0
    assert first["stats"]["n_tris_out"] == 50 and tr.expected_topology(len(first["verts"]), first["indices"])["stats"]["n_duplicate_tris"] == 0
    v, t = tr.clustered_thin_torus()
    s = _stats(v, t)["stats"]
    assert (s["n_tris"], s["n_duplicate_tris"], s["n_nonmanifold_edges"], s["n_edges"]) == (32, 10, 5, 43)
    v, t = tr.clustered_thin_torus(16)
    s = _stats(v, t)["stats"]
    assert (s["n_duplicate_tris"], s["n_nonmanifold_edges"], s["max_faces_on_edge"]) == (0, 11, 4)


def test_consistent_orientation_restores_a_sphere_and_weld_a_soup():
    v, t = tr.sphere(32)
    assert _stats(v, t)["stats"]["oriented"] == 1
    f = tr.flip_some(t, 0.3, 1)
    n_flipped = int((f != t).any(1).sum())
    assert 0.25 * len(t) < n_flipped < 0.35 * len(t) and _stats(v, f)["stats"]["n_inconsistent_edges"] > 0
    r = tr.expected_repair(v, f, orient="consistent")
    assert np.array_equal(r["indices"].reshape(-1, 3), t) and r["stats"]["n_flipped"] == n_flipped and r["stats"]["n_patches"] == 1
    # more than half flipped: the sheet that flips fewer turns the whole sphere inside out instead
    f = tr.flip_some(t, 0.7, 2)
    r = tr.expected_repair(v, f, orient="consistent")
    assert np.array_equal(r["indices"].reshape(-1, 3), t[:, [0, 2, 1]]) and r["stats"]["n_flipped"] == len(t) - int((f != t).any(1).sum())
    # a tie leaves the lowest-numbered triangle alone
    tv, tt = tr.tetrahedron()
    for flipped in ([0, 1], [2, 3]):
        f = tt.copy()
        f[flipped] = f[flipped][:, [0, 2, 1]]
        r = tr.expected_repair(tv, f, orient="consistent")
        assert np.array_equal(r["tri_flipped"], ~np.isin(np.arange(4), flipped) if 0 in flipped else np.isin(np.arange(4), flipped))
    sv, st = tr.soup(v, t)
    w = tr.expected_repair(sv, st, weld=True, duplicates="keep", drop_degenerate=False)
    assert w["stats"]["n_welded"] == len(sv) - len(v) and w["stats"]["n_verts_out"] == len(v)
    assert tr.expected_topology(len(w["verts"]), w["indices"])["stats"] == _stats(v, t)["stats"]
    assert np.array_equal(w["verts"][w["indices"]], v[t.ravel()])
    pv = np.float32([[0.0, 1, 2], [-0.0, 1, 2], [0, 1, 3], [0.0, 1, 2], [5, 5, 5], [6, 6, 6]])  # -0 equals +0
    w = tr.expected_repair(pv, np.array([[0, 2, 4], [1, 5, 3]]), weld=True)
    assert list(w["vertex_map"]) == [0, 0, 1, 0, 2, tr.NONE] and w["stats"]["n_welded"] == 2 and w["stats"]["n_degenerate_dropped"] == 1  # (1, 5, 3) became (0, 5, 0)
    with pytest.raises(ValueError, match="not finite"):
        tr.expected_repair(np.float32([[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]), weld=True)


def test_permutations_change_what_the_header_says_they_change():
    rng = np.random.default_rng(4)
    v, t = tr.two_cubes_sharing_an_edge()
    t = np.concatenate([tr.flip_some(t, 0.3, 3), [[0, 0, 1]]])
    a = tr.expected_topology(len(v), t)
    perm = rng.permutation(len(t))
    p = tr.expected_topology(len(v), t[perm])
    assert p["stats"] == a["stats"] and p["table"].tobytes() == a["table"].tobytes()
    hperm = (3 * perm[:, None] + np.arange(3)).ravel()  # half-edge h of the permuted mesh is half-edge hperm[h] of the original
    new_of_old = np.empty(3 * len(t), np.int64)
    new_of_old[hperm] = np.arange(3 * len(t))
    assert np.array_equal(p["n_faces"], a["n_faces"][hperm]) and np.array_equal(p["n_same"], a["n_same"][hperm])
    am = a["mate"][hperm].astype(np.int64)
    assert np.array_equal(p["mate"], np.where(am == tr.NONE, tr.NONE, new_of_old[np.minimum(am, 3 * len(t) - 1)]))
    rv, rt, new = tr.renumber(v, t, rng)
    r = tr.expected_topology(len(rv), rt)
    assert r["stats"] == a["stats"]
    drop = lambda table: np.sort(table[[n for n in table.dtype.names if n != "label"]], axis=0)
    assert np.array_equal(drop(r["table"]), drop(a["table"]))


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


def test_topology_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = _functions(HEADER)
    assert names == ["rnb_mesh_repair", "rnb_mesh_repair_default_options", "rnb_mesh_topology", "rnb_mesh_topology_abi_version", "rnb_mesh_topology_default_options",
                     "rnb_mesh_topology_table_free"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_TOPOLOGY_PROTOTYPES) == set(names)
    others = [getattr(_abi, n) for n in dir(_abi) if n.endswith("PROTOTYPES") and n != "MESH_TOPOLOGY_PROTOTYPES"]
    assert len(others) >= 10 and not any(set(_abi.MESH_TOPOLOGY_PROTOTYPES) & set(o) for o in others)  # a table of its own
    fns = api.load_library()
    assert fns.mesh_topology_abi_version() == _abi.MESH_TOPOLOGY_ABI_VERSION == 1
    o = _abi.MeshTopologyOptions()
    assert fns.mesh_topology_default_options(C.byref(o)) == 0 and (o.abi_version, o.buckets_log2, list(o.reserved)) == (1, 0, [0] * 4)
    r = _abi.MeshRepairOptions()
    assert fns.mesh_repair_default_options(C.byref(r)) == 0
    assert (r.abi_version, r.weld, r.drop_degenerate, r.duplicates, r.orient, r.buckets_log2, list(r.reserved)) == (1, 0, 1, _abi.MESH_DUPLICATES_FIRST, _abi.MESH_REPAIR_ORIENT_NONE, 0, [0] * 4)
    assert fns.mesh_topology_default_options(None) == _abi.ERR_INVALID and fns.mesh_repair_default_options(None) == _abi.ERR_INVALID
    for name in ("mesh_topology", "repair_mesh"):
        assert hasattr(api.Context, name)
    for name in ("topology", "repair"):
        assert hasattr(api.DeviceMesh, name)
    from rnb_neus2_amd import build
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS


def test_topology_validates_its_arguments_without_a_device():
    """Null pointers, a wrong version, unknown enums, reserved words, buckets_log2 outside 0, 4 .. 30, n_indices % 3, null buffers and in == out are refused before the
    context or the device is touched: the context handed in here is a block of zeros, and no device exists where this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def topt(**kw):
        o = _abi.MeshTopologyOptions()
        assert fns.mesh_topology_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def ropt(**kw):
        o = _abi.MeshRepairOptions()
        assert fns.mesh_repair_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def census(ctx_, m, o, tab=None):
        return fns.mesh_topology(ctx_, None, m, o, None, None, None, tab, None)

    def repair(ctx_, m, o, out):
        return fns.mesh_repair(ctx_, None, m, o, out, None, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    E = _abi.ERR_INVALID
    assert census(None, C.byref(src), C.byref(topt())) == E and census(ctx, None, C.byref(topt())) == E and census(ctx, C.byref(src), None) == E
    assert repair(None, C.byref(src), C.byref(ropt()), C.byref(dst)) == E and repair(ctx, None, C.byref(ropt()), C.byref(dst)) == E
    assert repair(ctx, C.byref(src), None, C.byref(dst)) == E and repair(ctx, C.byref(src), C.byref(ropt()), None) == E
    assert repair(ctx, C.byref(src), C.byref(ropt()), C.byref(src)) == E and b"different objects" in fns.last_error()  # in place
    res4 = (C.c_uint32 * 4)(0, 0, 1, 0)
    for kw in (dict(abi_version=2), dict(abi_version=0), dict(buckets_log2=3), dict(buckets_log2=1), dict(buckets_log2=31), dict(reserved=res4)):
        tab = C.c_void_p(1)
        assert census(ctx, C.byref(src), C.byref(topt(**kw)), C.byref(tab)) == E and not tab.value, kw
        assert fns.last_error()
    assert b"buckets_log2" in [fns.last_error() for _ in [census(ctx, C.byref(src), C.byref(topt(buckets_log2=3)))]][0]
    for kw in (dict(abi_version=2), dict(weld=2), dict(drop_degenerate=2), dict(duplicates=3), dict(orient=2), dict(orient=0xFFFFFFFF), dict(buckets_log2=3), dict(buckets_log2=31),
               dict(reserved=res4)):
        dst.n_verts = 7
        assert repair(ctx, C.byref(src), C.byref(ropt(**kw)), C.byref(dst)) == E, kw
        assert dst.n_verts == 0 and not dst.verts  # zeroed on failure
    src.n_indices, src.n_verts = 4, 3  # not a multiple of 3
    assert census(ctx, C.byref(src), C.byref(topt())) == E and repair(ctx, C.byref(src), C.byref(ropt()), C.byref(dst)) == E
    src.n_indices = 3  # null buffers
    assert census(ctx, C.byref(src), C.byref(topt())) == E and repair(ctx, C.byref(src), C.byref(ropt()), C.byref(dst)) == E
    assert fns.mesh_topology_table_free(None, None) == E
    assert fake.raw == b"\0" * 4096


def test_topology_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = {"rnb_mesh_topology_options": _abi.MeshTopologyOptions, "rnb_mesh_topology_component": _abi.MeshTopologyComponent, "rnb_mesh_topology_stats": _abi.MeshTopologyStats,
               "rnb_mesh_repair_options": _abi.MeshRepairOptions, "rnb_mesh_repair_stats": _abi.MeshRepairStats}
    lines, want = [], []
    for cname, S in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(S))
        for field, _ in S._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
            want.append(getattr(S, field).offset)
    consts = ["RNB_MESH_TOPOLOGY_ABI_VERSION", "RNB_MESH_TOPOLOGY_NONE", "RNB_MESH_TOPOLOGY_MAX_BUCKET", "RNB_MESH_DUPLICATES_KEEP", "RNB_MESH_DUPLICATES_FIRST", "RNB_MESH_DUPLICATES_CANCEL",
              "RNB_MESH_REPAIR_ORIENT_NONE", "RNB_MESH_REPAIR_ORIENT_CONSISTENT"]
    for name in consts:
        lines.append('printf("%%llu\\n", (unsigned long long)%s);' % name)
        want.append(getattr(_abi, name[4:]))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnb_mesh_topology.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want
    dt, T = np.dtype(_abi.MESH_TOPOLOGY_COMPONENT_DTYPE), _abi.MeshTopologyComponent
    assert dt == tr.TABLE_DTYPE and dt.itemsize == C.sizeof(T) and [dt.fields[n][1] for n in dt.names] == [getattr(T, n).offset for n in dt.names]
    assert (tr.NONE, tr.MAX_BUCKET) == (_abi.MESH_TOPOLOGY_NONE, _abi.MESH_TOPOLOGY_MAX_BUCKET)
    assert set(tr.TOPOLOGY_STATS) | {"peak_workspace", "ms"} == set(_abi.MeshTopologyStats().as_dict())
    assert set(tr.REPAIR_STATS) | {"peak_workspace", "ms"} == set(_abi.MeshRepairStats().as_dict())


# ------------------------------------------------------------------------------------------------------------------------ the calls of the Python layer
DEVICE_CALLS = ("extract_mesh", "mesh_clean", "mesh_simplify", "mesh_distance", "mesh_topology", "mesh_repair", "device_malloc", "device_free", "memcpy", "mesh_free",
                "mesh_clean_table_free", "mesh_topology_table_free")
MESH_ARGS = dict(extract_mesh=((), 3), mesh_clean=((2,), 4), mesh_simplify=((2,), 4), mesh_repair=((2,), 4), mesh_topology=((2,), None), mesh_distance=((2, 3), None), mesh_free=((1,), None))


class RecordingLibrary:
    """A stand-in for the library's function table, after FakeLibrary of tests/test_device_mesh_cpu.py: every entry point returns 0 (`fail` names the one that returns
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
            elif name in ("device_free", "mesh_clean_table_free", "mesh_topology_table_free"):
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
            if name == "mesh_topology":
                obj(8).n_components = 2
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
    "mesh_topology": lambda c: c.mesh_topology(V, I, edges=True, table=True),
    "mesh_topology_stats_only": lambda c: c.mesh_topology(V, I),
    "repair_mesh": lambda c: c.repair_mesh(V, I, colors=COL, weld=True, duplicates="cancel", orient="consistent", vertex_map=True),
    "extract_mesh": lambda c: c.extract_mesh(16, keep="largest", simplify=8, error=True, colors=True, repair=dict(duplicates="cancel", orient="consistent"), topology=True),
}
EXPECTED = {
    "mesh_topology": UP * 2 + ["device_malloc"] * 3 + ["mesh_topology"] + ["memcpy"] * 4 + ["mesh_topology_table_free"] + ["device_free"] * 3 + ["device_free"] * 2,
    "mesh_topology_stats_only": UP * 2 + ["mesh_topology"] + ["device_free"] * 2,
    "repair_mesh": UP * 3 + ["device_malloc", "mesh_repair", "memcpy", "device_free"] + ["device_free"] * 3 + ["memcpy"] * 3 + ["mesh_free"],
    "extract_mesh": ["extract_mesh", "mesh_clean", "mesh_simplify", "mesh_repair", "mesh_distance", "mesh_distance", "mesh_topology"] + ["memcpy"] * 3 + ["mesh_free"] * 4,
}


def test_the_python_calls_make_the_expected_c_calls_in_order():
    from rnb_neus2_amd import _abi
    for name, call in CALLS.items():
        c, fake = _context()
        out = call(c)
        assert fake.names() == EXPECTED[name], (name, fake.names())
        assert not fake.buffers and not fake.meshes and not fake.errors, name
    c, fake = _context()
    out = CALLS["mesh_topology"](c)
    assert out["n_components"] == 2 and out["table"].dtype == tr.TABLE_DTYPE and len(out["table"]) == 2 and all(len(out[k]) == 6 for k in ("n_faces", "n_same", "mate"))
    assert [e for e in fake.log if e[0] == "mesh_topology"][0][1][1:] == (1, 1, 1, 1)  # the three arrays and the table were asked for
    c, fake = _context()
    out = CALLS["mesh_topology_stats_only"](c)
    assert [e for e in fake.log if e[0] == "mesh_topology"][0][1][1:] == (0, 0, 0, 0) and "table" not in out and "mate" not in out and "n_edges" in out
    c, fake = _context()
    out = CALLS["extract_mesh"](c)
    log = {e[0]: e[1] for e in fake.device_log() if e[0].startswith("mesh_") and e[0] not in ("mesh_distance", "mesh_free")}
    assert log["mesh_repair"][0] == log["mesh_simplify"][1] and log["mesh_topology"][0] == log["mesh_repair"][1]  # simplify -> repair -> the census of the result
    dist = [e[1] for e in fake.device_log() if e[0] == "mesh_distance"]
    assert dist == [(log["mesh_simplify"][0], log["mesh_repair"][1]), (log["mesh_repair"][1], log["mesh_simplify"][0])]  # the error: simplifier's input <-> the repaired mesh
    assert {"repair_stats", "simplify_stats", "clean_stats", "topology", "simplify_error"} <= set(out) and "n_flipped" in out["repair_stats"] and "n_edges" in out["topology"]
    # the options reach the C struct
    c, fake = _context()
    o = c._repair_options(weld=True, drop_degenerate=False, duplicates="cancel", orient="consistent", buckets_log2=12)
    assert (o.weld, o.drop_degenerate, o.duplicates, o.orient, o.buckets_log2) == (1, 0, _abi.MESH_DUPLICATES_CANCEL, _abi.MESH_REPAIR_ORIENT_CONSISTENT, 12)
    assert c._topology_options(5).buckets_log2 == 5
    for bad in (dict(duplicates="all"), dict(orient="outward")):
        with pytest.raises(ValueError):
            c._repair_options(**bad)
    with pytest.raises(ValueError):
        c.extract_mesh(16, repair=dict(keep="largest"))
    with pytest.raises(ValueError):
        c.extract_mesh(16, repair=True)
    assert not fake.device_log()


@pytest.mark.parametrize("stage", ["extract_mesh", "mesh_clean", "mesh_simplify", "mesh_repair", "mesh_distance", "mesh_topology"])
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
        with c.extract_mesh_device(16, colors=True) as m, m.clean() as cm, cm.simplify((0, 0, 0), 0.25, 4) as sm, sm.repair(weld=True, vertex_map=True) as rm:
            rm.topology(edges=True, table=True)
            sm.distance_to(rm)
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_a_freed_handle_stops_in_python():
    c, fake = _context()
    m = c.upload_mesh(V, I, COL)
    r = m.repair(vertex_map=True)
    assert isinstance(r.vertex_map, np.ndarray) and len(r.vertex_map) == 4 and r.has_colors and r.stats["ms"] == 0.5 and m.vertex_map is None
    assert m.topology()["n_components"] == 2
    m.free()
    n = len(fake.log)
    for call in (lambda: m.topology(), lambda: m.topology(edges=True, table=True), lambda: m.repair(), lambda: m.repair(weld=True, vertex_map=True)):
        with pytest.raises(ValueError):
            call()
    assert len(fake.log) == n
    r.free()
    with pytest.raises(ValueError):
        r.topology()
    assert not fake.buffers and not fake.meshes and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--repair", "--weld", "--duplicates", "--orient-consistent", "--report-topology"):
        assert flag in r.stdout, flag
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--repair", "--duplicates", "all"], ["--repair", "--duplicates"], ["--weld"], ["--duplicates", "first"], ["--orient-consistent"], ["--repair=1"], ["--repair", "--weld=1"],
                ["--report-topology=1"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    for good in (["--repair"], ["--repair", "--weld", "--duplicates", "cancel", "--orient-consistent", "--report-topology"], ["--report-topology"],
                 ["--simplify", "8", "--repair", "--keep", "largest", "--orient", "outward"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, good  # the flags parse; the snapshot is what is missing


def test_the_pipeline_passes_the_flags_through():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    plain = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8)
    assert "--repair" not in plain and "--report-topology" not in plain
    argv = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, repair=dict(weld=True, duplicates="cancel", orient_consistent=True), report_topology=True)
    assert argv[:len(plain)] == plain and argv[len(plain):] == ["--repair", "--weld", "--duplicates", "cancel", "--orient-consistent", "--report-topology"]
    assert pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", repair=True)[-1] == "--repair"
    with pytest.raises(ValueError):
        pipeline.repair_flags(dict(duplicates="all"))
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "tb", "out", repair=True)
    common = ["-i", "in", "-t", "tb", "-o", "out"]
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--simplify", "8", "--repair", "--duplicates", "cancel", "--orient-consistent", "--report-topology"])
    kw = run_pipeline.pipeline_kwargs(ns)
    assert kw["repair"] == dict(weld=False, orient_consistent=True, duplicates="cancel") and kw["report_topology"] is True
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert "repair" not in kw and "report_topology" not in kw and "weld" not in kw
    for bad in (["--repair"], ["--device-postprocess", "--weld"], ["--device-postprocess", "--repair", "--duplicates", "all"], ["--report-topology"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(common + bad)


def test_the_test_meshes_stay_far_below_the_bucket_guard():
    """The GPU tests (tests/test_gpu_mesh_topology.py) run these meshes: none may put more than 1024 items on one key, so that only the guard's own test meets the cap."""
    rng = np.random.default_rng(0)
    meshes = [tr.cube(), tr.tetrahedron(), tr.torus_grid(16), tr.moebius(16), tr.disc(9), tr.annulus(12), tr.two_cubes_sharing_an_edge(), tr.book(7), tr.book(1024), tr.clustered_slab(),
              tr.clustered_thin_torus(), tr.sphere(32), tr.soup(*tr.sphere(32))] + [tr.strip(n) for n in (255, 256, 257, 1023)]
    for v, t in meshes:
        assert tr.max_key_multiplicity(v, t) <= 1024
    v, t = tr.cube()
    assert tr.max_key_multiplicity(v, np.tile(t[:1], (70000, 1))) == 70000 > tr.MAX_BUCKET


def test_the_tools_use_the_public_interface():
    with open(os.path.join(ROOT, "tools", "bench_mesh_topology.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and "fix_normals" in text and ".topology(edges=True, table=True)" in text and '.repair(duplicates="cancel", orient="consistent")' in text
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mesh_eval
    finally:
        sys.path.pop(0)

    class Ctx:  # --weld: both meshes through repair(weld=True, duplicates="keep", drop_degenerate=False) before the distance
        def __init__(self):
            self.calls = []

        def repair_mesh(self, v, i, **kw):
            self.calls.append(kw)
            return dict(verts=np.asarray(v, np.float32), indices=np.asarray(i, np.uint32).ravel(), stats=dict(n_welded=3))

        def mesh_distance(self, av, ai, bv, bi, **kw):
            one = dict(mean=0.0, rms=0.0, within=[1.0, 1.0], n_samples=1, n_beyond=0, quantisation=0.0, ms=0.0)
            return dict(one, chamfer=0.0, hausdorff=0.0, fscore=[1.0, 1.0], reverse=dict(one))

    v, t = tr.cube()
    c = Ctx()
    out = mesh_eval.evaluate(c, (v, t), (v, t), weld=True)
    assert c.calls == [dict(weld=True, duplicates="keep", drop_degenerate=False)] * 2 and out["welded"] == [3, 3]
    c = Ctx()
    assert "welded" not in mesh_eval.evaluate(c, (v, t), (v, t)) and not c.calls
