"""CPU tier of the self-intersection stage (include/rnb_mesh_intersect.h): the Python statement of tests/mesh_intersect_reference.py against the same rules evaluated
in exact rationals, brute force over all pairs, on meshes whose counts are known; the select rule; the C-ABI and the Python layer over a recording stand-in for the
library; the command line and the pipeline's flags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_intersect_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_intersect.h")


# ------------------------------------------------------------------------------------------------------------------------ the rules against exact rationals
def _against_exact(v, i):
    """Every float-proper pair is exact-proper; every float-apart pair that took no in-plane branch is exact-apart. -> (float census, exact census)."""
    flt, _ = ir.classify_pairs(v, i)
    exa, _ = ir.classify_pairs(v, i, exact=True)
    assert set(flt) == set(exa)  # the candidates are decided on the floats
    for key, (cls, _, inplane) in flt.items():
        if cls == ir.PROPER:
            assert exa[key][0] == ir.PROPER, key
        if cls == ir.APART and not inplane:
            assert exa[key][0] == ir.APART, key
    return ir.census(v, i), ir.census(v, i, exact=True)


def test_one_sphere_reports_nothing():
    v, i = ir.uv_sphere()
    assert len(i) // 3 == 120 and v.dtype == np.float32
    flt, exa = _against_exact(v, i)
    for r in (flt, exa):
        assert r["stats"]["n_pairs_proper"] == r["stats"]["n_pairs_contact"] == 0 and len(r["pairs"]) == 0 and r["stats"]["n_candidates"] > 0


def test_two_crossing_spheres_are_the_generic_case():
    v, i = ir.two_spheres()
    assert len(i) // 3 == 240
    flt, exa = _against_exact(v, i)
    assert flt["stats"]["n_pairs_proper"] == 54 and flt["stats"]["n_pairs_contact"] == 0
    assert np.array_equal(flt["pairs"], exa["pairs"]) and (flt["pairs"][:, 2] == ir.PROPER).all()
    assert (flt["pairs"][:, 0] < 120).all() and (flt["pairs"][:, 1] >= 120).all()  # every pair joins the two shells
    assert flt["n_proper"].sum() == 108 and flt["stats"]["n_tris_proper"] == int((flt["n_proper"] > 0).sum())


def test_a_flat_grid_reports_nothing():
    """Collinear neighbours, shared corners and shared edges in one plane: the in-plane rule is not strict, so touching along boundaries is apart."""
    v, i = ir.flat_grid()
    assert len(i) // 3 == 18
    flt, exa = _against_exact(v, i)
    for r in (flt, exa):
        assert len(r["pairs"]) == 0
    assert flt["stats"]["n_coplanar_pairs"] == flt["stats"]["n_candidates"] > 0  # every candidate was decided in the plane


def test_two_overlapping_grids_are_contact_through_step_2():
    v, i = ir.two_grids()
    flt, exa = _against_exact(v, i)
    assert flt["stats"]["n_pairs_contact"] == 67 and flt["stats"]["n_pairs_proper"] == 0 and np.array_equal(flt["pairs"], exa["pairs"])
    classes, _ = ir.classify_pairs(v, i)
    t = i.reshape(-1, 3)
    for (s, u), (cls, coplanar, _) in classes.items():
        if cls == ir.CONTACT:
            assert coplanar and not set(t[s]) & set(t[u]) and s < 18 <= u  # step 2: no index shared, one triangle of each grid


@pytest.mark.parametrize("name", sorted(ir.hand_cases()))
def test_hand_cases(name):
    v, i, want, stats = ir.hand_cases()[name]
    flt, exa = _against_exact(v, np.uint32(i))
    for r in (flt, exa):
        assert r["pairs"].tolist() == ([[0, 1, want]] if want else []), (name, r["pairs"])
        for key, value in stats.items():
            assert r["stats"][key] == value, (name, key)
    assert flt["stats"]["n_candidates"] == (0 if want is None else 1)


def test_disjoint_shells_report_nothing():
    v, i = mc.three_spheres(32)
    r = ir.census(v, i)
    assert r["stats"]["n_tris"] == 1988 and r["stats"]["n_candidates"] > 1988 and len(r["pairs"]) == 0 and r["stats"]["n_degenerate"] == 0


def test_the_sign_rules_on_their_thresholds():
    R = ir.Rules()
    a, b, c = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    assert R.orient(a, b, c, (0.3, 0.3, 1.0)) == 1 and R.orient(a, b, c, (0.3, 0.3, -1.0)) == -1 and R.orient(a, b, c, (0.3, 0.3, 0.0)) == 0
    # far from the origin: a clear offset is decided; a point a hair off a tilted plane is either not decided or right, never wrong
    far = [tuple(x + 1024.0 for x in q) for q in (a, b, c)]
    off = (1024.25, 1024.25, 1024.0 + 2.0 ** -42)
    exact = ir.Rules(exact=True)
    assert R.orient(*far, off) == 1 and exact.orient(*[exact.point(q) for q in far + [off]]) == 1  # 2^-42 of 2^10: decided
    tilted = [(1024.0, 1024.0, 1024.0), (1025.0, 1024.0, 1024.0 + 2.0 ** -30), (1024.0, 1025.0, 1024.0 - 2.0 ** -31)]
    on = (1024.5, 1024.5, 1024.0 + 2.0 ** -31 - 2.0 ** -32 + 2.0 ** -42)
    assert exact.orient(*[exact.point(q) for q in tilted + [on]]) != 0 and R.orient(*tilted, on) in (0, exact.orient(*[exact.point(q) for q in tilted + [on]]))  # never the wrong sign
    assert R.orient2(a, b, (0.5, 1e-300, 0.0), 2) == 1 and R.orient2(a, b, (0.5, 0.0, 7.0), 2) == 0 and R.orient2(a, b, (0.5, -1.0, 0.0), 2) == -1
    assert ir.Rules.axis(((0, 0, 0), (1, 0, 0), (0, 1, 0))) == 2 and ir.Rules.axis(((0, 0, 0), (0, 1, 0), (0, 0, 1))) == 0
    assert ir.Rules.axis(((0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.0, 1.0, 1.0))) == 0  # |n| = (1, 1, 1): of equals the lowest


# ------------------------------------------------------------------------------------------------------------------------ the select rule
def test_select_removes_the_right_triangles_and_rings_grow_by_vertices():
    v, i = ir.two_spheres()
    r = ir.census(v, i)
    t = i.reshape(-1, 3)
    hit = r["n_proper"] > 0
    out = ir.select(v, i, r["n_proper"], r["n_contact"])
    assert out["n_tris_removed"] == 53 == hit.sum() and len(out["indices"]) == 3 * (240 - 53)
    assert np.array_equal(out["verts"][out["indices"].reshape(-1, 3)], v[t[~hit]])  # the others, in input order, the same corners
    assert ir.census(out["verts"], out["indices"])["stats"]["n_pairs_proper"] == 0  # removing triangles makes no new pair
    none = ir.select(v, i, r["n_proper"], r["n_contact"], classes=ir.CONTACT)
    assert none["n_tris_removed"] == 0 and np.array_equal(none["indices"], i)
    one = ir.select(v, i, r["n_proper"], r["n_contact"], rings=1)
    touched = np.isin(t, np.unique(t[hit])).any(1)
    assert one["n_tris_removed"] == touched.sum() > 53
    two = ir.select(v, i, r["n_proper"], r["n_contact"], rings=2)
    assert two["n_tris_removed"] == np.isin(t, np.unique(t[touched])).any(1).sum() > one["n_tris_removed"]
    kept = ir.select(v, i, r["n_proper"], r["n_contact"], rings=2, drop_unused_vertices=False)
    assert len(kept["verts"]) == len(v) and kept["n_verts_removed"] == 0 and two["n_verts_removed"] > 0
    col = np.arange(3 * len(v), dtype=np.float32).reshape(-1, 3)
    with_col = ir.select(v, i, r["n_proper"], r["n_contact"], rings=2, colors=col)
    assert np.array_equal(with_col["colors"][:, 0] // 3, np.flatnonzero(np.isin(np.arange(len(v)), t[~np.isin(t, np.unique(t[touched])).any(1)])))
    d = ir.two_grids()
    rd = ir.census(*d)
    everything = ir.select(*d, rd["n_proper"], rd["n_contact"], classes=ir.PROPER | ir.CONTACT)
    assert len(everything["indices"]) == 0 and len(everything["verts"]) == 0 and everything["n_tris_removed"] == 36  # everything selected: an empty mesh


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_the_header_the_library_and_the_python_tables_agree(tmp_path):
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import _abi, api
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)))
    assert names == ["rnb_mesh_intersect_abi_version", "rnb_mesh_intersect_default_options", "rnb_mesh_intersections", "rnb_mesh_intersections_select",
                     "rnb_mesh_intersections_select_default_options"], names
    assert set("rnb_" + k for k in _abi.MESH_INTERSECT_PROTOTYPES) == set(names)
    others = [getattr(_abi, n) for n in dir(_abi) if n.endswith("PROTOTYPES") and n != "MESH_INTERSECT_PROTOTYPES"]
    assert len(others) >= 12 and not any(set(_abi.MESH_INTERSECT_PROTOTYPES) & set(o) for o in others)  # a table of its own
    fns = api.load_library()
    assert fns.mesh_intersect_abi_version() == _abi.MESH_INTERSECT_ABI_VERSION == 1
    opt, sel = _abi.MeshIntersectOptions(), _abi.MeshIntersectSelectOptions()
    assert fns.mesh_intersect_default_options(C.byref(opt)) == 0 and (opt.abi_version, opt.cells, list(opt.reserved)) == (1, 0, [0] * 4)
    assert fns.mesh_intersections_select_default_options(C.byref(sel)) == 0
    assert (sel.abi_version, sel.classes, sel.rings, sel.drop_unused_vertices) == (1, _abi.MESH_INTERSECT_PROPER, 0, 1)
    assert fns.mesh_intersect_default_options(None) == _abi.ERR_INVALID and fns.mesh_intersections_select_default_options(None) == _abi.ERR_INVALID
    # failures before the device is touched (this machine has none)
    m = _abi.Mesh()
    st = _abi.MeshIntersectStats()
    st.n_tris = 7
    assert fns.mesh_intersections(None, None, C.byref(m), C.byref(opt), None, None, None, 0, C.byref(st)) == _abi.ERR_INVALID and st.n_tris == 0
    assert (ir.PROPER, ir.CONTACT) == (_abi.MESH_INTERSECT_PROPER, _abi.MESH_INTERSECT_CONTACT)
    # the structs, against a C program compiled from the header
    structs = {"rnb_mesh_intersect_options": _abi.MeshIntersectOptions, "rnb_mesh_intersect_stats": _abi.MeshIntersectStats, "rnb_mesh_intersect_pair": np.dtype(_abi.MESH_INTERSECT_PAIR_DTYPE),
               "rnb_mesh_intersect_select_options": _abi.MeshIntersectSelectOptions, "rnb_mesh_intersect_select_stats": _abi.MeshIntersectSelectStats}
    lines, want = [], []
    for cname, py in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(py.itemsize if isinstance(py, np.dtype) else C.sizeof(py))
        for field in (py.names if isinstance(py, np.dtype) else [f[0] for f in py._fields_]):
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
            want.append(py.fields[field][1] if isinstance(py, np.dtype) else getattr(py, field).offset)
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnb_mesh_intersect.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(tmp_path / "t")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()] == want


# ------------------------------------------------------------------------------------------------------------------------ the Python layer
DEVICE_CALLS = ("extract_mesh", "mesh_simplify", "mesh_repair", "mesh_fill_holes", "mesh_topology", "mesh_intersections", "mesh_intersections_select", "device_malloc", "device_free", "memcpy", "mesh_free")
MESH_ARGS = dict(extract_mesh=((), 3), mesh_simplify=((2,), 4), mesh_repair=((2,), 4), mesh_fill_holes=((2,), 4), mesh_topology=((2,), None), mesh_intersections=((2,), None),
                 mesh_intersections_select=((2,), 6), mesh_free=((1,), None))


class RecordingLibrary:
    """A stand-in for the library's function table, after the one of tests/test_device_mesh_cpu.py: every entry point returns 0 (`fail` names the one that returns
    ERR_INVALID instead); a call that returns a mesh fills it with made-up pointers; device_malloc hands out made-up pointers; a download reads zeros. `log` holds
    (name, the `verts` pointers of the meshes passed, inputs then output, then what the test looks at); `buffers` and `meshes` what is handed out and not yet released,
    `errors` every release of something that is not. mesh_intersections reports `would_be` pairs."""

    def __init__(self, fail=None, would_be=0):
        self.fail, self.would_be, self.log, self.buffers, self.meshes, self.errors, self._next = fail, would_be, [], set(), set(), [], 0x1000

    def _ptr(self):
        self._next += 0x100
        return self._next

    def names(self):
        return [e[0] for e in self.log if e[0] in DEVICE_CALLS]

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
            elif name == "device_free":
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
            if name == "mesh_intersections":
                st = obj(8)
                st.n_pairs_proper, st.n_pairs_written_would_be = self.would_be, (self.would_be if args[6] is not None else 0)
                seen += (int(args[4] is not None), int(args[5] is not None), int(args[6] is not None), int(args[7]), obj(3).cells)
            if name == "mesh_intersections_select":
                obj(7).n_selected = 2
                seen += (int(args[3] is not None), int(args[4] is not None), obj(5).classes, obj(5).rings, obj(5).drop_unused_vertices)
            self.log.append((name, seen))
            return 0
        return call

    def _release(self, held, ptr, name):
        if ptr in held:
            held.remove(ptr)
        else:
            self.errors.append((name, ptr))


def _context(fail=None, would_be=0):
    from rnb_neus2_amd import _abi, api
    fake = RecordingLibrary(fail, would_be)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
I = np.uint32([0, 1, 2, 0, 2, 3])
COL = np.full((4, 3), 0.5, np.float32)
UP = ["device_malloc", "memcpy"]

CALLS = {
    "mesh_self_intersections": lambda c: c.mesh_self_intersections(V, I),
    "mesh_self_intersections_pairs": lambda c: c.mesh_self_intersections(V, I, pairs=True, cells=7),
    "drop_intersecting_mesh": lambda c: c.drop_intersecting_mesh(V, I, colors=COL, classes="all", rings=2),
    "extract_mesh_report": lambda c: c.extract_mesh(16, simplify=8, fill_holes=True, self_intersections=True),
    "extract_mesh_drop": lambda c: c.extract_mesh(16, simplify=8, repair=dict(duplicates="cancel"), fill_holes=True, topology=True, self_intersections="drop"),
    "extract_mesh_both": lambda c: c.extract_mesh(16, self_intersections=dict(drop="all", rings=1, report=True, cells=5)),
}
CENSUS = ["device_malloc"] * 2 + ["mesh_intersections"]
EXPECTED = {
    "mesh_self_intersections": UP * 2 + CENSUS + ["memcpy"] * 2 + ["device_free"] * 2 + ["device_free"] * 2,
    "mesh_self_intersections_pairs": UP * 2 + ["device_malloc"] * 3 + ["mesh_intersections"] + ["memcpy"] * 2 + ["device_free"] * 3 + ["device_free"] * 2,
    "drop_intersecting_mesh": UP * 3 + CENSUS + ["mesh_intersections_select"] + ["device_free"] * 2 + ["device_free"] * 3 + ["memcpy"] * 3 + ["mesh_free"],
    "extract_mesh_report": ["extract_mesh", "mesh_simplify", "mesh_fill_holes"] + CENSUS + ["memcpy"] * 2 + ["device_free"] * 2 + ["memcpy"] * 2 + ["mesh_free"] * 3,
    "extract_mesh_drop": ["extract_mesh", "mesh_simplify", "mesh_repair"] + CENSUS + ["mesh_intersections_select"] + ["device_free"] * 2 + ["mesh_fill_holes", "mesh_topology"] + ["memcpy"] * 2 + ["mesh_free"] * 5,
    "extract_mesh_both": ["extract_mesh"] + CENSUS + ["mesh_intersections_select"] + ["device_free"] * 2 + CENSUS + ["memcpy"] * 2 + ["device_free"] * 2 + ["memcpy"] * 2 + ["mesh_free"] * 2,
}


def test_the_python_calls_make_the_expected_c_calls_in_order():
    for name, call in CALLS.items():
        c, fake = _context()
        call(c)
        assert fake.names() == EXPECTED[name], (name, fake.names())
        assert not fake.buffers and not fake.meshes and not fake.errors, name
    c, fake = _context()
    out = CALLS["mesh_self_intersections"](c)
    assert [e for e in fake.log if e[0] == "mesh_intersections"][0][1][1:] == (1, 1, 0, 0, 0)  # the two count arrays, no pair list, automatic cells
    assert len(out["n_proper"]) == len(out["n_contact"]) == 2 and "pairs" not in out and "n_candidates" in out and out["dims"] == [0, 0, 0]
    c, fake = _context()
    out = CALLS["mesh_self_intersections_pairs"](c)
    assert [e for e in fake.log if e[0] == "mesh_intersections"][0][1][1:] == (1, 1, 1, 256, 7) and out["pairs"].shape == (0, 3)
    # the first guess was short: the list is released and the call repeated with the exact capacity
    c, fake = _context(would_be=1000)
    out = c.mesh_self_intersections(V, I, pairs=True)
    assert [e[1][4] for e in fake.log if e[0] == "mesh_intersections"] == [256, 1000] and out["pairs"].shape == (1000, 3) and out["pairs"].dtype == np.uint32
    assert fake.names() == UP * 2 + ["device_malloc"] * 3 + ["mesh_intersections", "device_free", "device_malloc", "mesh_intersections"] + ["memcpy"] * 3 + ["device_free"] * 3 + ["device_free"] * 2
    assert not fake.buffers and not fake.errors
    c, fake = _context()
    out = CALLS["drop_intersecting_mesh"](c)
    from rnb_neus2_amd import _abi
    sel = [e for e in fake.log if e[0] == "mesh_intersections_select"][0][1]
    assert sel[2:] == (1, 1, _abi.MESH_INTERSECT_PROPER | _abi.MESH_INTERSECT_CONTACT, 2, 1) and "colors" in out
    assert out["stats"]["n_selected"] == 2 and out["drop_stats"] is out["stats"] and "n_candidates" in out["stats"]["census"] and "n_proper" not in out["stats"]["census"]
    c, fake = _context()
    out = CALLS["extract_mesh_drop"](c)
    log = {e[0]: e[1] for e in fake.log if e[0].startswith("mesh_") and e[0] != "mesh_free"}
    assert log["mesh_intersections"][0] == log["mesh_intersections_select"][0] == log["mesh_repair"][1]  # after the repair,
    assert log["mesh_fill_holes"][0] == log["mesh_intersections_select"][1] and log["mesh_topology"][0] == log["mesh_fill_holes"][1]  # before the fill
    assert log["mesh_intersections_select"][4] == _abi.MESH_INTERSECT_PROPER and "drop_stats" in out and "self_intersections" not in out
    c, fake = _context()
    out = CALLS["extract_mesh_report"](c)
    log = {e[0]: e[1] for e in fake.log if e[0].startswith("mesh_") and e[0] != "mesh_free"}
    assert log["mesh_intersections"][0] == log["mesh_fill_holes"][1] and "n_pairs_proper" in out["self_intersections"] and "drop_stats" not in out  # the final mesh
    c, fake = _context()
    out = CALLS["extract_mesh_both"](c)
    runs = [e[1] for e in fake.log if e[0] == "mesh_intersections"]
    sel = [e[1] for e in fake.log if e[0] == "mesh_intersections_select"][0]
    assert runs[1][0] == sel[1] and runs[0][5] == runs[1][5] == 5 and sel[4:6] == (3, 1) and {"drop_stats", "self_intersections"} <= set(out)
    # left off, extract_mesh makes the calls it made before
    c, fake = _context()
    out = c.extract_mesh(16, simplify=8, repair=dict(duplicates="cancel"), fill_holes=True, topology=True)
    assert fake.names() == ["extract_mesh", "mesh_simplify", "mesh_repair", "mesh_fill_holes", "mesh_topology"] + ["memcpy"] * 2 + ["mesh_free"] * 4
    assert "drop_stats" not in out and "self_intersections" not in out
    c, fake = _context()
    for bad in (dict(self_intersections=False), dict(self_intersections="all"), dict(self_intersections=dict(drop="contact")), dict(self_intersections=dict(rings=9, drop="proper")),
                dict(self_intersections=dict(cells=257, report=True)), dict(self_intersections=dict(pairs=True))):
        with pytest.raises(ValueError):
            c.extract_mesh(16, **bad)
    for bad in (lambda: c._intersect_options(-1), lambda: c._intersect_select_options("both"), lambda: c._intersect_select_options(rings=-1)):
        with pytest.raises(ValueError):
            bad()
    assert not fake.names()


@pytest.mark.parametrize("stage", ["extract_mesh", "mesh_simplify", "mesh_fill_holes", "mesh_intersections", "mesh_intersections_select"])
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
    c, fake = _context(fail=stage, would_be=1000)
    with pytest.raises(api.RnbError):
        with c.extract_mesh_device(16, colors=True) as m, m.simplify((0, 0, 0), 0.25, 4) as sm:
            sm.self_intersections(pairs=True)
            counts = sm.self_intersections(on_device=True)
            try:
                with sm.drop_intersecting(counts=counts) as dm, dm.fill_holes() as fm:
                    fm.self_intersections()
            finally:
                c.device_free(counts["n_proper"])
                c.device_free(counts["n_contact"])
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_a_freed_handle_stops_in_python():
    c, fake = _context()
    m = c.upload_mesh(V, I, COL)
    counts = m.self_intersections(on_device=True)
    assert isinstance(counts["n_proper"], int) and counts["n_proper"] in fake.buffers and counts["n_contact"] in fake.buffers  # they stay, and are the caller's
    d = m.drop_intersecting("all", rings=1, counts=counts)
    assert d.has_colors and d.stats["n_selected"] == 2 and d.stats["ms"] == 0.5 and "census" not in d.stats
    assert [e[0] for e in fake.log].count("mesh_intersections") == 1  # counts given: no census of its own
    c.device_free(counts["n_proper"])
    c.device_free(counts["n_contact"])
    m.free()
    n = len(fake.log)
    for call in (lambda: m.self_intersections(), lambda: m.self_intersections(pairs=True, on_device=True), lambda: m.drop_intersecting(), lambda: m.drop_intersecting(counts=counts)):
        with pytest.raises(ValueError):
            call()
    assert len(fake.log) == n
    d.free()
    with pytest.raises(ValueError):
        d.self_intersections()
    assert not fake.buffers and not fake.meshes and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--report-intersections", "--drop-intersecting", "--drop-rings"):
        assert flag in r.stdout, flag
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--drop-intersecting", "contact"], ["--drop-intersecting"], ["--drop-rings", "1"], ["--drop-intersecting", "proper", "--drop-rings", "9"],
                ["--drop-intersecting", "all", "--drop-rings", "x"], ["--report-intersections=1"], ["--drop-intersecting", "proper", "--drop-rings"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    for good in (["--report-intersections"], ["--drop-intersecting", "proper"], ["--drop-intersecting", "all", "--drop-rings", "8", "--fill-holes", "--report-intersections", "--report-topology"],
                 ["--simplify", "8", "--repair", "--drop-intersecting", "proper", "--drop-rings", "0", "--fill-holes", "--keep", "largest"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, good  # the flags parse; the snapshot is what is missing


def test_the_pipeline_passes_the_flags_through():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    plain = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, fill_holes=True)
    assert "--drop-intersecting" not in plain and "--report-intersections" not in plain
    argv = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, fill_holes=True, drop_intersecting=dict(classes="all", rings=2), report_intersections=True)
    assert argv[:len(plain)] == plain and argv[len(plain):] == ["--drop-intersecting", "all", "--drop-rings", "2", "--report-intersections"]
    assert pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", drop_intersecting="proper")[-2:] == ["--drop-intersecting", "proper"]
    for bad in ("contact", dict(classes="proper", rings=9), dict(rings=1), dict(classes="all", ring=1)):
        with pytest.raises(ValueError):
            pipeline.drop_intersecting_flags(bad)
    for kw in (dict(drop_intersecting="proper"), dict(report_intersections=True)):
        with pytest.raises(ValueError):
            pipeline.run_full_pipeline("in", "tb", "out", **kw)
    common = ["-i", "in", "-t", "tb", "-o", "out"]
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--drop-intersecting", "all", "--drop-rings", "3", "--report-intersections"])
    kw = run_pipeline.pipeline_kwargs(ns)
    assert kw["drop_intersecting"] == dict(classes="all", rings=3) and kw["report_intersections"] is True
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--drop-intersecting", "proper"])
    assert run_pipeline.pipeline_kwargs(ns)["drop_intersecting"] == dict(classes="proper")
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert not {"drop_intersecting", "drop_rings", "report_intersections"} & set(kw)
    for bad in (["--drop-intersecting", "proper"], ["--report-intersections"], ["--device-postprocess", "--drop-rings", "1"], ["--device-postprocess", "--drop-intersecting", "some"],
                ["--device-postprocess", "--drop-intersecting", "all", "--drop-rings", "9"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(common + bad)


def test_the_bench_tool_uses_the_public_interface():
    with open(os.path.join(ROOT, "tools", "bench_mesh_intersections.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".self_intersections(" in text and ".drop_intersecting(" in text and ".fill_holes(" in text and ".topology(" in text
