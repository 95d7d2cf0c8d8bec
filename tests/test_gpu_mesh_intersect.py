"""The self-intersection stage on the MI355X (include/rnb_mesh_intersect.h) against the Python statement of tests/mesh_intersect_reference.py, bit for bit: n_proper,
n_contact, the pair list and every statistic outside the grid block. On the meshes of the CPU tier, on crossing shells of a few thousand triangles, across search grids,
under permutations and renumberings, at sizes around the wavefront and the workgroup, with the large list, with short pair lists, on empty and invalid input; the
selection against the statement, and drop -> census -> fill; through the model, beside training, and through build/mesh."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_intersect_reference as ir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
GRID_KEYS = ("dims", "cell", "n_cell_entries", "n_large", "n_visited", "peak_workspace", "ms", "ms_grid")
_WANT = {}


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def _want(name, v, i):
    """The statement's census, computed once per named mesh and left as it is."""
    if name not in _WANT:
        _WANT[name] = ir.census(v, i)
    return _WANT[name]


def _assert_equal(got, want):
    for key in ir.STAT_KEYS:
        assert got[key] == want["stats"][key], (key, got[key], want["stats"][key])
    assert np.array_equal(got["n_proper"], want["n_proper"]) and np.array_equal(got["n_contact"], want["n_contact"])
    assert got["n_proper"].dtype == got["n_contact"].dtype == np.uint32
    if "pairs" in got:
        assert np.array_equal(got["pairs"].astype(np.int64), want["pairs"]) and got["n_pairs_written_would_be"] == len(want["pairs"])


def _check(c, v, i, name=None, cells=0):
    got = c.mesh_self_intersections(v, i, pairs=True, cells=cells)
    _assert_equal(got, _want(name, v, i) if name else ir.census(v, i))
    return got


def _rule_bytes(got):
    """Everything outside the grid block, as bytes."""
    return repr([(k, got[k]) for k in sorted(got) if k not in GRID_KEYS + ("n_proper", "n_contact", "pairs")]).encode() + got["n_proper"].tobytes() + got["n_contact"].tobytes() + got["pairs"].tobytes()


MESHES = {"two_spheres": ir.two_spheres, "flat_grid": ir.flat_grid, "two_grids": ir.two_grids}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_the_meshes_of_the_cpu_tier(ctx, name):
    got = _check(ctx, *MESHES[name](), name=name)
    want = {"two_spheres": (54, 0), "flat_grid": (0, 0), "two_grids": (0, 67)}[name]
    assert (got["n_pairs_proper"], got["n_pairs_contact"]) == want


@pytest.mark.parametrize("name", sorted(ir.hand_cases()))
def test_hand_cases(ctx, name):
    v, i, want, _ = ir.hand_cases()[name]
    got = _check(ctx, v, np.uint32(i))
    assert got["pairs"].tolist() == ([[0, 1, want]] if want else [])


def _crossing_shells():
    v, i = mc.three_spheres(32)
    return ir.join((v, i), (v + np.float32([0.11, 0.07, 0.05]), i))


def test_crossing_shells_of_four_thousand_triangles(ctx):
    v, i = _crossing_shells()
    got = _check(ctx, v, i, name="crossing_shells")
    assert got["n_tris"] == 3976 and got["n_pairs_proper"] > 100 and max(got["dims"]) == 44 and got["n_large"] == 0
    print("crossing shells: %d candidates, %d proper, %d contact, %d visited, %.3f ms" % (got["n_candidates"], got["n_pairs_proper"], got["n_pairs_contact"], got["n_visited"], got["ms"]))


def _tilted_strips():
    from tests.test_gpu_mesh_distance import _flat
    v, i = _flat()
    a = 0.05
    rot = np.float32([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    w = (v - np.float32([0, 3 / 64, 0])) @ rot.T + np.float32([0.004, 3 / 64, 0.001])
    return ir.join((v, i), (w.astype(np.float32), i))


def test_the_grid_changes_no_bit(ctx):
    for name, (v, i) in (("two_spheres", ir.two_spheres()), ("tilted_strips", _tilted_strips())):
        want, seen = None, set()
        for cells in (1, 3, 16, 64, 0):
            got = ctx.mesh_self_intersections(v, i, pairs=True, cells=cells)
            if want is None:  # cells = 1 is the device's own exhaustive search: every pair of triangles that take part is looked at once
                want = got
                _assert_equal(got, _want(name, v, i))
                n = got["n_tris"] - got["n_degenerate"]
                assert got["dims"] == [1, 1, 1] and got["n_visited"] == n * (n - 1) // 2
            assert _rule_bytes(got) == _rule_bytes(want), (name, cells)
            seen.add(tuple(got["dims"]))
        assert len(seen) >= 4
        if name == "tilted_strips":
            assert got["n_pairs_proper"] > 50 and got["dims"][1] < got["dims"][0] and got["dims"][2] < got["dims"][0]


def test_permuted_triangles_and_renumbered_vertices(ctx):
    rng = np.random.default_rng(11)
    v, i = ir.two_spheres()
    t = i.reshape(-1, 3)
    base = _check(ctx, v, i, name="two_spheres")
    perm = rng.permutation(len(t))  # new triangle k is old triangle perm[k]
    got = _check(ctx, v, t[perm].ravel())
    assert np.array_equal(got["n_proper"], base["n_proper"][perm]) and np.array_equal(got["n_contact"], base["n_contact"][perm])  # the counts follow their triangles
    old = np.sort(perm[got["pairs"][:, :2].astype(np.int64)], axis=1)
    order = np.lexsort((old[:, 1], old[:, 0]))
    assert np.array_equal(old[order], base["pairs"][:, :2]) and np.array_equal(got["pairs"][order, 2], base["pairs"][:, 2])
    vperm = rng.permutation(len(v))  # new vertex k is old vertex vperm[k]
    inv = np.argsort(vperm)
    got = _check(ctx, v[vperm], inv[t].astype(np.uint32).ravel())
    assert _rule_bytes(got) == _rule_bytes(base)
    rolled = _check(ctx, v, t[:, [1, 2, 0]].ravel())  # another first corner: the statement follows; here no class depends on it
    assert np.array_equal(rolled["pairs"], base["pairs"])


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_sizes_around_the_wavefront_and_the_workgroup(ctx, n):
    """Prefixes of the two spheres' triangle list, interleaved so that every prefix holds triangles of both shells."""
    v, i = ir.two_spheres()
    t = i.reshape(-1, 3)
    mixed = np.stack([t[:120], t[120:]], 1).reshape(-1, 3)
    mixed = np.concatenate([mixed, mixed[:17][:, [1, 2, 0]]])  # 257 triangles: the last 17 are second copies, same-set pairs
    got = _check(ctx, v, mixed[:n].ravel())
    assert got["n_pairs_proper"] == {63: 0, 64: 2, 65: 2, 255: 63, 256: 63, 257: 64}[n] and got["n_same_set"] == max(n - 240, 0)
    one = _check(ctx, v, mixed[:n].ravel(), cells=1)  # one list of n triangles: tiles of 32 + 32, the last ones part full
    assert _rule_bytes(one) == _rule_bytes(got)


def test_the_large_list(ctx):
    """Triangles that span the box overlap more than 2048 cells of a 64^3 grid and go into the large list: met by a pass of their own, each pair once."""
    v, i = ir.two_spheres()
    big = np.float32([[0.15, 0.15, 0.48], [1.05, 0.2, 0.52], [0.3, 1.0, 0.5], [0.2, 0.5, 0.15], [0.9, 0.45, 0.2], [0.55, 0.6, 1.0]])
    for n_big in (1, 2):
        vv, ii = ir.join((v, i), (big[:3 * n_big], np.arange(3 * n_big)))
        got = _check(ctx, vv, ii, name="large_%d" % n_big, cells=64)
        assert got["n_large"] == n_big and got["n_proper"][240] > 10
        auto = _check(ctx, vv, ii, name="large_%d" % n_big)
        assert auto["n_large"] == 0 and _rule_bytes(auto) == _rule_bytes(got)
    assert got["n_proper"][241] > 10 and [240, 241, ir.PROPER] in got["pairs"].tolist()  # the two cross each other: large against large


def test_pairs_capacity(ctx):
    from rnb_neus2_amd import _abi
    v, i = ir.two_spheres()
    want = _want("two_spheres", v, i)
    rec = np.dtype(_abi.MESH_INTERSECT_PAIR_DTYPE)
    n = len(want["pairs"])
    with ctx.upload_mesh(v, i) as m:
        opt = ctx._intersect_options()
        for cap in (0, n, n - 1):
            buf = ctx.upload(np.full(n + 1, 0xAB, np.uint8).repeat(rec.itemsize))
            st = _abi.MeshIntersectStats()
            try:
                ctx._check(ctx.f.mesh_intersections(ctx._h, None, C.byref(m), C.byref(opt), None, None, buf, cap, C.byref(st)))
                got = ctx.download(buf, n + 1, rec)
            finally:
                ctx.device_free(buf)
            assert st.n_pairs_written_would_be == n == st.n_pairs_proper and st.n_tris_proper == want["stats"]["n_tris_proper"]  # the counts need no output array
            assert np.array_equal(np.stack([got["s"], got["t"], got["cls"]], 1)[:cap].astype(np.int64), want["pairs"][:cap])
            assert got[cap:].tobytes() == b"\xAB" * (rec.itemsize * (n + 1 - cap))  # nothing beyond the capacity
        st = _abi.MeshIntersectStats()
        ctx._check(ctx.f.mesh_intersections(ctx._h, None, C.byref(m), C.byref(opt), None, None, None, 0, C.byref(st)))
        assert st.n_pairs_written_would_be == 0 and st.n_pairs_proper == n


def test_invalid_input_fails_cleanly_and_leaves_the_context_usable(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    v, i = ir.two_spheres()
    bad = i.copy()
    bad[7] = len(v)  # checked by a kernel before any index is used as an address
    nan = v.copy()
    nan[3, 1] = np.inf
    calls = (lambda vv, ii: ctx.mesh_self_intersections(vv, ii, pairs=True), lambda vv, ii: ctx.drop_intersecting_mesh(vv, ii))
    for call in calls:
        for vv, ii, what in ((v, bad, "out of range"), (nan, i, "not finite")):
            with pytest.raises(rnb.RnbError, match=what) as e:
                call(vv, ii)
            assert e.value.code == _abi.ERR_INVALID and "rnb_mesh_intersections" in str(e.value)
            _check(ctx, v, i, name="two_spheres")
    unused = np.concatenate([v, np.float32([[np.nan, 0, 0]])])  # a vertex no triangle uses is never read
    _check(ctx, unused, i, name="two_spheres")
    f = ctx.f
    with ctx.upload_mesh(v, i) as m:
        opt, sel, st, sst, out = ctx._intersect_options(), ctx._intersect_select_options(), _abi.MeshIntersectStats(), _abi.MeshIntersectSelectStats(), _abi.Mesh()
        counts = ctx.device_malloc(4 * 240)
        try:
            def census(mesh, o, pairs=None, cap=0):
                st.n_tris = 7
                rc = f.mesh_intersections(ctx._h, None, C.byref(mesh) if mesh is not None else None, C.byref(o) if o is not None else None, None, None, pairs, cap, C.byref(st))
                assert st.n_tris == 0  # zeroed on failure
                return rc, f.last_error()

            def select(mesh, o, np_=counts, nc=counts, dst=out):
                sst.n_tris_in = 7
                rc = f.mesh_intersections_select(ctx._h, None, C.byref(mesh), np_, nc, C.byref(o), C.byref(dst), C.byref(sst))
                assert sst.n_tris_in == (0 if rc else len(i) // 3)  # zeroed on failure
                return rc, f.last_error()

            short = _abi.Mesh.from_buffer_copy(bytes(m))
            short.n_indices = len(i) - 2
            wrong, cells, reserved = ctx._intersect_options(), ctx._intersect_options(), ctx._intersect_options()
            wrong.abi_version, cells.cells, reserved.reserved[2] = 2, 257, 1
            for args, what in (((None, opt), b"null"), ((m, None), b"null"), ((m, wrong), b"abi_version"), ((m, reserved), b"reserved"), ((m, cells), b"cells"), ((short, opt), b"multiple of 3"),
                               ((m, opt, None, 5), b"pairs_capacity")):
                rc, err = census(*args)
                assert rc == _abi.ERR_INVALID and what in err and b"rnb_mesh_intersections" in err, (what, err)
            for key, value, what in (("abi_version", 2, b"abi_version"), ("classes", 0, b"classes"), ("classes", 4, b"classes"), ("rings", 9, b"rings"), ("drop_unused_vertices", 2, b"drop_unused")):
                o = ctx._intersect_select_options()
                setattr(o, key, value)
                out.n_indices = 9
                rc, err = select(m, o)
                assert rc == _abi.ERR_INVALID and what in err and b"rnb_mesh_intersections_select" in err and bytes(out) == b"\0" * C.sizeof(out), (what, err)
            assert select(m, sel, np_=None)[0] == _abi.ERR_INVALID and select(short, sel)[0] == _abi.ERR_INVALID
            rc, err = select(m, sel, dst=m)
            assert rc == _abi.ERR_INVALID and b"different objects" in err and m.n_indices == len(i) and m.verts  # in == out: refused, the input untouched
            both = ctx._intersect_select_options("all")
            assert select(m, both, nc=None)[0] == _abi.ERR_INVALID and select(m, sel, nc=None)[0] == 0  # a class that is not selected needs no counts
            ctx._check(f.mesh_free(ctx._h, C.byref(out)))
        finally:
            ctx.device_free(counts)
    _check(ctx, v, i, name="two_spheres")
    # a mesh without triangles, and one whose triangles all take no part
    e, z = np.zeros(0, np.uint32), np.zeros((5, 3), np.float32)
    got = _check(ctx, z, e)
    assert got["n_tris"] == 0 and got["dims"] == [0, 0, 0] and len(got["n_proper"]) == 0 and got["pairs"].shape == (0, 3)
    assert len(ctx.drop_intersecting_mesh(z, e, colors=z)["indices"]) == 0
    got = _check(ctx, z, np.uint32([0, 1, 2, 2, 3, 4]))
    assert got["n_degenerate"] == 2 and got["dims"] == [0, 0, 0] and got["n_candidates"] == 0


def _select_equal(got, want, v_in, t_in):
    assert got["verts"].tobytes() == want["verts"].tobytes() and got["indices"].tobytes() == want["indices"].tobytes()
    for key in ("colors", "normals"):
        assert (key in got) == (key in want) and (key not in got or got[key].tobytes() == want[key].tobytes())
    st = got["stats"]
    assert (st["n_tris_removed"], st["n_verts_removed"], st["n_tris_in"], st["n_verts_in"]) == (want["n_tris_removed"], want["n_verts_removed"], t_in, v_in)
    assert st["n_tris_out"] == t_in - want["n_tris_removed"] and st["n_verts_out"] == v_in - want["n_verts_removed"]


@pytest.mark.parametrize("classes", ["proper", "all"])
@pytest.mark.parametrize("rings", [0, 1])
def test_select_against_the_statement(ctx, classes, rings):
    mask = ir.PROPER if classes == "proper" else ir.PROPER | ir.CONTACT
    for name, (v, i) in (("two_spheres", ir.two_spheres()), ("two_grids", ir.two_grids()), ("tilted_strips", _tilted_strips())):
        r = _want(name, v, i)
        col = np.random.default_rng(5).random(v.shape).astype(np.float32)
        got = ctx.drop_intersecting_mesh(v, i, colors=col, normals=-col, classes=classes, rings=rings)
        _select_equal(got, ir.select(v, i, r["n_proper"], r["n_contact"], mask, rings, True, col, -col), len(v), len(i) // 3)
        assert got["stats"]["n_selected"] == int((((r["n_proper"] > 0) & bool(mask & ir.PROPER)) | ((r["n_contact"] > 0) & bool(mask & ir.CONTACT))).sum())
        got = ctx.drop_intersecting_mesh(v, i, classes=classes, rings=rings, drop_unused_vertices=False)
        _select_equal(got, ir.select(v, i, r["n_proper"], r["n_contact"], mask, rings, False), len(v), len(i) // 3)
    if classes == "all":  # everything selected: an empty mesh, no error
        assert len(ctx.drop_intersecting_mesh(*ir.two_grids(), classes="all")["indices"]) == 0


def test_drop_then_census_then_fill(ctx):
    v, i = ir.two_spheres()
    with ctx.upload_mesh(v, i) as m:
        assert m.topology()["closed"] == 1
        counts = m.self_intersections(on_device=True)
        try:
            with m.drop_intersecting(counts=counts) as a, m.drop_intersecting() as b:
                assert a.download()["indices"].tobytes() == b.download()["indices"].tobytes() and b.stats["census"]["n_pairs_proper"] == 54 and "census" not in a.stats
                after = a.self_intersections(pairs=True)
                assert after["n_pairs_proper"] == 0 and after["n_tris"] == 240 - 53 and len(after["pairs"]) == after["n_pairs_contact"]
                assert a.topology()["closed"] == 0
                with a.fill_holes() as f:
                    census, loops = f.topology(), f.boundary_loops()
                    filled = f.self_intersections()
                    print("after the fill: closed %d, %d loops filled of %d, %d open loops of which %d simple; %d proper and %d contact pairs" % (
                        census["closed"], f.stats["n_filled"], f.stats["n_loops"], loops["n_loops"], loops["n_simple"], filled["n_pairs_proper"], filled["n_pairs_contact"]))
                    assert census["closed"] == 1 or loops["n_loops"] > 0  # closed, or it states its open loops
                    _assert_equal(filled, ir.census(**{k: f.download()[k] for k in ("verts", "indices")}))
        finally:
            ctx.device_free(counts["n_proper"])
            ctx.device_free(counts["n_contact"])


def test_through_the_model():
    """extract_mesh(self_intersections=True) returns the census of the mesh it returns; with "drop" the mesh re-examined has no proper pair; left off, nothing changes."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(16, 128, 1400.0 * 128 / 800.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(60):
            c.train_step()
        for res, simplify in ((16, None), (64, 16), (64, 8)):
            kw = dict(res=res, cull="none", colors=True, simplify=simplify)
            plain = c.extract_mesh(**kw)
            seen = c.extract_mesh(self_intersections=True, **kw)
            assert sorted(set(seen) - set(plain)) == ["self_intersections"] and all(seen[k].tobytes() == plain[k].tobytes() for k in ("verts", "indices", "colors"))
            census = seen["self_intersections"]
            _assert_equal(census, ir.census(plain["verts"], plain["indices"]))
            dropped = c.extract_mesh(self_intersections=dict(drop="proper", report=True), fill_holes=True, **kw)
            again = c.mesh_self_intersections(dropped["verts"], dropped["indices"])
            assert dropped["drop_stats"]["census"]["n_pairs_proper"] == census["n_pairs_proper"] and dropped["drop_stats"]["n_selected"] == census["n_tris_proper"]
            assert {k: again[k] for k in ir.STAT_KEYS} == {k: dropped["self_intersections"][k] for k in ir.STAT_KEYS}
            only = c.extract_mesh(self_intersections="drop", **kw)
            assert c.mesh_self_intersections(only["verts"], only["indices"])["n_pairs_proper"] == 0 and "self_intersections" not in only
            print("res %d simplify %s: %d triangles, %d candidates, %d proper and %d contact pairs; after drop + fill %d proper, %d contact" % (
                res, simplify, census["n_tris"], census["n_candidates"], census["n_pairs_proper"], census["n_pairs_contact"], again["n_pairs_proper"], again["n_pairs_contact"]))


def test_the_calls_leave_training_untouched():
    """deterministic = 1: 20 steps, a census with pairs, a drop and an extract_mesh with both, 20 steps == 40 steps, bit for bit."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    v, i = ir.two_spheres()
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(40):
            if interrupt and s == 20:
                c.mesh_self_intersections(v, i, pairs=True)
                c.drop_intersecting_mesh(v, i, classes="all", rings=1)
                c.extract_mesh(64, cull="none", simplify=16, fill_holes=True, self_intersections=dict(drop="proper", report=True))
            stats.append(c.train_step().as_dict())
        state = {k: c.get(k).copy() for k in ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID", "DENSITY_BITFIELD")}
        for st in stats:
            st.pop("prep_ms"), st.pop("step_ms")
        runs.append((state, stats))
        c.close()
    (sa, ta), (sb, tb) = runs
    assert ta == tb
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def test_build_mesh_reports_the_numbers_of_the_python_call(tmp_path):
    """`build/mesh --resolution 128 --simplify 16 --report-intersections` on a snapshot trained here for 100 steps prints one JSON line whose numbers are those of
    Context.extract_mesh(res=128, simplify=16, self_intersections=True) on a context holding the same snapshot; with --drop-intersecting proper --fill-holes the
    `drop intersecting:` line appears and the line describes the refilled mesh; without the flags neither line appears."""
    from rnb_neus2_amd import synthetic
    from tests.test_gpu_mesh_simplify import _context_of
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--simplify", "16", "--out", str(tmp_path / "m.obj")]
    keys = ("n_tris", "n_degenerate", "n_same_set", "n_candidates", "n_pairs_proper", "n_pairs_contact", "n_tris_proper", "n_tris_contact", "n_coplanar_pairs", "dims", "n_large",
            "n_cell_entries", "n_visited")
    with _context_of(snap) as c:
        for flags, kw in (([], dict(self_intersections=True)), (["--drop-intersecting", "proper", "--fill-holes"], dict(self_intersections=dict(drop="proper", report=True), fill_holes=True))):
            r = subprocess.run(base + ["--report-intersections"] + flags, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
            lines = [l for l in r.stdout.splitlines() if l.startswith('{"intersections"')]
            assert len(lines) == 1 and len([l for l in r.stdout.splitlines() if l.startswith("drop intersecting:")]) == (1 if flags else 0), r.stdout
            print(lines[0])
            said = json.loads(lines[0])["intersections"]
            want = c.extract_mesh(res=128, colors=True, simplify=16, **kw)["self_intersections"]
            assert {k: said[k] for k in keys} == {k: want[k] for k in keys} and said["n_tris"] > 0
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "intersections" not in r.stdout and "drop intersecting" not in r.stdout
