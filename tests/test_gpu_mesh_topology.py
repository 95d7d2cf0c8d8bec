"""The mesh topology stage on the MI355X (include/rnb_mesh_topology.h) against the numpy statement of tests/mesh_topology_reference.py, bit for bit: the per-half-edge
arrays, the component table, the statistics and the repaired mesh, on hand-made meshes of every kind (closed, open, unorientable, non-manifold, folded, soup), at the
workgroup and scan boundaries, for every bucket count, under permutations and renumberings, on a strip of 2^20 triangles, on invalid input, at the bucket guard, on the
mesh of a model and through build/mesh."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_topology_reference as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def _census(c, v, t, **kw):
    """DeviceMesh.topology(edges, table) == the statement; returns the device's dict."""
    got = c.mesh_topology(v, np.asarray(t, np.uint32).ravel(), edges=True, table=True, **kw)
    tr.assert_equal_bits(got, tr.expected_topology(len(v), t))
    return got


REPAIRS = (dict(), dict(duplicates="cancel", orient="consistent"), dict(duplicates="keep", drop_degenerate=False, orient="consistent"), dict(weld=True, duplicates="first", orient="consistent"),
           dict(weld=True, duplicates="cancel"))


def _repair(c, v, t, colors=None, normals=None, buckets_log2=0, **kw):
    got = c.repair_mesh(v, np.asarray(t, np.uint32).ravel(), colors=colors, normals=normals, vertex_map=True, buckets_log2=buckets_log2, **kw)
    want = tr.expected_repair(v, t, colors=colors, normals=normals, **kw)
    tr.assert_equal_bits(got, want)
    return got, want


def _flipped_strip(n):
    v, t = tr.strip(n)
    return v, tr.flip_some(t, 0.4, n)


def _with_junk(v, t):
    """Degenerate triangles, a duplicate of either winding and an unused vertex added to a mesh."""
    t = np.asarray(t, np.int64)
    extra = np.array([[t[0, 0], t[0, 0], t[0, 1]], t[1], t[2][[0, 2, 1]], [t[3, 2], t[3, 1], t[3, 2]], t[1][[1, 2, 0]]])
    return np.concatenate([v, [[9, 9, 9]]]).astype(np.float32), np.concatenate([t[:5], extra, t[5:]])


MESHES = {
    "cube": tr.cube, "tetrahedron": tr.tetrahedron, "torus_grid": lambda: tr.torus_grid(16), "moebius": lambda: tr.moebius(16), "disc": lambda: tr.disc(9), "annulus": lambda: tr.annulus(12),
    "two_cubes": tr.two_cubes_sharing_an_edge, "book": lambda: tr.book(7), "soup": lambda: tr.soup(*tr.torus_grid(8)), "slab": tr.clustered_slab, "thin_torus": tr.clustered_thin_torus,
    "thin_torus_16": lambda: tr.clustered_thin_torus(16), "torus_flipped": lambda: (tr.torus_grid(16)[0], tr.flip_some(tr.torus_grid(16)[1], 0.3, 5)),
    "two_cubes_junk": lambda: _with_junk(*tr.two_cubes_sharing_an_edge()), "moebius_flipped": lambda: (tr.moebius(16)[0], tr.flip_some(tr.moebius(16)[1], 0.5, 6)),
    # the 256-thread workgroup and the 1024-element scan: the mate of a half-edge lies in another workgroup
    "strip_255": lambda: _flipped_strip(255), "strip_256": lambda: _flipped_strip(256), "strip_257": lambda: _flipped_strip(257), "strip_1023": lambda: _flipped_strip(1023),
    "book_1024": lambda: tr.book(1024),  # the quadratic path: 1024 half-edges on one edge
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_kind_of_mesh(ctx, name):
    v, t = MESHES[name]()
    assert tr.max_key_multiplicity(v, t) <= 1024
    _census(ctx, v, t)
    rng = np.random.default_rng(len(name))
    col, nrm = rng.random((len(v), 3), dtype=np.float32), rng.standard_normal((len(v), 3)).astype(np.float32)
    for kw in REPAIRS:
        got, want = _repair(ctx, v, t, **kw)
        assert "colors" not in got and "normals" not in got
        _repair(ctx, v, t, colors=col, normals=nrm, **kw)
        if kw.get("orient") == "consistent" and len(want["indices"]):  # what the repair promises: no manifold edge of an orientable patch is left inconsistent
            after = ctx.mesh_topology(got["verts"], got["indices"])
            assert (after["n_inconsistent_edges"] == 0) == (after["n_unorientable_patches"] == 0)
        if kw.get("duplicates") != "keep" and len(want["indices"]):  # first leaves one triangle per vertex set, cancel one winding per vertex set
            after = ctx.mesh_topology(got["verts"], got["indices"])
            assert after["n_folded_pairs"] == 0 and after["n_degenerate"] == 0 and (kw.get("duplicates") == "cancel" or after["n_duplicate_tris"] == 0)


def test_weld_turns_a_soup_back_into_its_mesh(ctx):
    v, t = tr.sphere(32)
    v = v.copy()
    v[t[0, 0], 0] = 0.0  # one vertex with a zero coordinate; its copies in the soup get either sign
    sv, st = tr.soup(v, t)
    sv = sv.copy()
    copies = np.flatnonzero((sv == v[t[0, 0]]).all(1))
    assert len(copies) >= 4
    sv[copies[1::2], 0] = -0.0
    assert np.signbit(sv[copies[1], 0]) and not np.signbit(sv[copies[0], 0])
    assert ctx.mesh_topology(sv, st.ravel())["n_components"] == len(t)  # the cleaner's view of a soup: one component per triangle
    got, want = _repair(ctx, sv, st, weld=True, duplicates="keep", drop_degenerate=False)
    assert got["stats"]["n_welded"] == len(sv) - len(v) and got["stats"]["n_verts_out"] == len(v)
    welded = ctx.mesh_topology(got["verts"], got["indices"], edges=True, table=True)
    tr.assert_equal_bits(welded, tr.expected_topology(len(want["verts"]), want["indices"]))
    original = tr.expected_topology(len(v), t)
    assert {k: welded[k] for k in tr.TOPOLOGY_STATS} == original["stats"] and welded["closed"] == 1 and welded["oriented"] == 1 and list(welded["table"]["genus"]) == [0]
    # a NaN no triangle uses does not matter, with or without weld; a used one fails with weld only
    import rnb_neus2_amd as rnb
    w = np.concatenate([sv, np.full((1, 3), np.nan, np.float32)])
    _repair(ctx, w, st, weld=True)
    w = sv.copy()
    w[7, 1] = np.nan
    _repair(ctx, w, st)
    with pytest.raises(rnb.RnbError, match="not finite"):
        ctx.repair_mesh(w, st.ravel(), weld=True)
    w[7, 1] = np.inf
    with pytest.raises(rnb.RnbError, match="not finite"):
        ctx.repair_mesh(w, st.ravel(), weld=True)
    _repair(ctx, sv, st, weld=True)


def test_the_result_does_not_depend_on_the_bucket_count(ctx):
    """buckets_log2 = 4 puts 10 536 half-edges into 16 buckets: every bucket is long and filled in an order that changes from run to run."""
    v, t = tr.sphere(32)
    f = tr.flip_some(t, 0.3, 1)
    kw = dict(duplicates="cancel", orient="consistent", weld=True)
    base_c = _census(ctx, v, f)
    base_r, want = _repair(ctx, v, f, **kw)
    assert np.array_equal(base_r["indices"].reshape(-1, 3), t) and base_r["stats"]["n_flipped"] == int((f != t).any(1).sum())  # the sphere comes back
    for b in (4, 12, 4):
        c = _census(ctx, v, f, buckets_log2=b)
        r, _ = _repair(ctx, v, f, buckets_log2=b, **kw)
        for key in ("n_faces", "n_same", "mate", "table"):
            assert c[key].tobytes() == base_c[key].tobytes(), (b, key)
        assert {k: c[k] for k in tr.TOPOLOGY_STATS} == {k: base_c[k] for k in tr.TOPOLOGY_STATS}
        for key in ("verts", "indices", "vertex_map"):
            assert r[key].tobytes() == base_r[key].tobytes(), (b, key)
        assert {k: r["stats"][k] for k in tr.REPAIR_STATS} == {k: base_r["stats"][k] for k in tr.REPAIR_STATS}


def test_permuted_triangles_and_renumbered_vertices(ctx):
    rng = np.random.default_rng(4)
    v, t = _with_junk(*tr.two_cubes_sharing_an_edge())
    t = tr.flip_some(t, 0.3, 3)
    a = _census(ctx, v, t)
    perm = rng.permutation(len(t))
    p = _census(ctx, v, t[perm])
    assert {k: p[k] for k in tr.TOPOLOGY_STATS} == {k: a[k] for k in tr.TOPOLOGY_STATS} and p["table"].tobytes() == a["table"].tobytes()
    hperm = (3 * perm[:, None] + np.arange(3)).ravel()
    new_of_old = np.empty(3 * len(t), np.int64)
    new_of_old[hperm] = np.arange(3 * len(t))
    assert np.array_equal(p["n_faces"], a["n_faces"][hperm]) and np.array_equal(p["n_same"], a["n_same"][hperm])
    am = a["mate"][hperm].astype(np.int64)
    assert np.array_equal(p["mate"], np.where(am == tr.NONE, tr.NONE, new_of_old[np.minimum(am, 3 * len(t) - 1)]))
    rv, rt, _ = tr.renumber(v, t, rng)
    r = _census(ctx, rv, rt)
    assert {k: r[k] for k in tr.TOPOLOGY_STATS} == {k: a[k] for k in tr.TOPOLOGY_STATS}
    drop = lambda table: np.sort(table[[n for n in table.dtype.names if n != "label"]], axis=0)
    assert np.array_equal(drop(r["table"]), drop(a["table"]))
    for kw in REPAIRS:
        sa, sp, sr = (_repair(ctx, *m, **kw)[0]["stats"] for m in ((v, t), (v, t[perm]), (rv, rt)))
        for key in ("n_welded", "n_degenerate_dropped", "n_duplicates_dropped", "n_patches", "n_unorientable_patches", "n_verts_out", "n_tris_out"):
            assert sa[key] == sp[key] == sr[key], (kw, key)
    again = ctx.repair_mesh(v, t.ravel(), duplicates="cancel", orient="consistent", vertex_map=True)  # the same input: the same bits
    first = ctx.repair_mesh(v, t.ravel(), duplicates="cancel", orient="consistent", vertex_map=True)
    for key in ("verts", "indices", "vertex_map"):
        assert again[key].tobytes() == first[key].tobytes()


def test_a_strip_of_a_million_triangles_under_a_random_numbering(ctx):
    """The long union-find chain of the double cover: one patch of 2^20 triangles, every third one flipped, vertices numbered at random."""
    rng = np.random.default_rng(7)
    v, t = tr.strip(1 << 20)
    t = t.copy()
    t[::3] = t[::3][:, [0, 2, 1]]
    v, t, _ = tr.renumber(v, t, rng)
    want = tr.expected_repair(v, t, orient="consistent")
    got = ctx.repair_mesh(v, t.astype(np.uint32).ravel(), orient="consistent")
    print("strip of 2^20 triangles: repair %.2f ms, peak workspace %.1f MB" % (got["stats"]["ms"], got["stats"]["peak_workspace"] / 1e6))
    tr.assert_equal_bits(got, {k: want[k] for k in ("verts", "indices", "stats")})
    assert got["stats"]["n_flipped"] == want["stats"]["n_flipped"] == 349526 and got["stats"]["n_patches"] == 1
    after = ctx.mesh_topology(got["verts"], got["indices"])
    print("its census: %.2f ms" % after["ms"])
    assert (after["n_inconsistent_edges"], after["n_manifold_edges"], after["n_patches"], after["n_unorientable_patches"], after["n_boundary_components"]) == (0, (1 << 20) - 1, 1, 0, 1)
    before = ctx.mesh_topology(v, t.astype(np.uint32).ravel())
    assert before["n_inconsistent_edges"] == tr.expected_topology(len(v), t)["stats"]["n_inconsistent_edges"] > 0


def test_invalid_input_fails_cleanly_and_the_context_stays_usable(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    v, t = tr.two_cubes_sharing_an_edge()
    i = t.astype(np.uint32).ravel()
    for bad_value in (len(v), 0xFFFFFFFF):
        bad = i.copy()
        bad[len(bad) // 2] = bad_value
        for call in (lambda: ctx.mesh_topology(v, bad, edges=True, table=True), lambda: ctx.repair_mesh(v, bad, weld=True, orient="consistent", vertex_map=True)):
            with pytest.raises(rnb.RnbError, match="out of range"):
                call()
        _census(ctx, v, t)
    for call in (lambda: ctx.mesh_topology(v, i, buckets_log2=3), lambda: ctx.repair_mesh(v, i, buckets_log2=3), lambda: ctx.repair_mesh(v, i, buckets_log2=31)):
        with pytest.raises(rnb.RnbError, match="buckets_log2"):
            call()
    f = ctx.f
    with ctx.upload_mesh(v, i) as m:
        out, tab = _abi.Mesh(), C.c_void_p(1)

        def census(opt, mesh=m):
            return f.mesh_topology(ctx._h, None, C.byref(mesh), C.byref(opt), None, None, None, C.byref(tab), None)

        def repair(opt, mesh=m):
            out.n_indices = 9
            return f.mesh_repair(ctx._h, None, C.byref(mesh), C.byref(opt), C.byref(out), None, None)

        topt, ropt = ctx._topology_options(), ctx._repair_options()
        assert f.mesh_repair(ctx._h, None, C.byref(m), C.byref(ropt), C.byref(m), None, None) == _abi.ERR_INVALID  # in == out: refused, the input untouched
        assert b"different objects" in f.last_error() and m.n_indices == len(i) and m.verts
        short = _abi.Mesh.from_buffer_copy(bytes(m))
        short.n_indices = len(i) - 2
        assert census(topt, short) == _abi.ERR_INVALID and not tab.value and b"multiple of 3" in f.last_error()
        assert repair(ropt, short) == _abi.ERR_INVALID and bytes(out) == b"\0" * C.sizeof(out)
        for field, value in (("abi_version", 2), ("buckets_log2", 3)):
            o = ctx._topology_options()
            setattr(o, field, value)
            tab.value = 1
            assert census(o) == _abi.ERR_INVALID and not tab.value, field
        o = ctx._topology_options()
        o.reserved[1] = 1
        assert census(o) == _abi.ERR_INVALID and b"reserved" in f.last_error()
        for field, value in (("abi_version", 0), ("weld", 2), ("drop_degenerate", 7), ("duplicates", 3), ("orient", 2), ("buckets_log2", 3)):
            o = ctx._repair_options()
            setattr(o, field, value)
            assert repair(o) == _abi.ERR_INVALID and bytes(out) == b"\0" * C.sizeof(out), field
        o = ctx._repair_options()
        o.reserved[3] = 5
        assert repair(o) == _abi.ERR_INVALID and b"reserved" in f.last_error()
    _census(ctx, v, t)
    _repair(ctx, v, t, orient="consistent")
    # an empty input succeeds and gives an empty output
    e = np.zeros(0, np.uint32)
    z = np.zeros((5, 3), np.float32)
    got = ctx.mesh_topology(z, e, edges=True, table=True)
    tr.assert_equal_bits(got, tr.expected_topology(5, e))
    assert got["closed"] == 1 and got["oriented"] == 1 and len(got["table"]) == 0 and len(got["mate"]) == 0
    got, _ = _repair(ctx, z, e, colors=z, weld=True, orient="consistent")
    assert got["verts"].shape == (0, 3) and got["colors"].shape == (0, 3) and list(got["vertex_map"]) == [tr.NONE] * 5


def test_the_bucket_guard_refuses_a_pathological_mesh(ctx):
    """70 000 copies of one triangle: 70 000 half-edges on each of three edges, 4.9e9 bucket reads each if they were walked. A clean refusal, before any walk."""
    import rnb_neus2_amd as rnb
    v, t = tr.cube()
    many = np.tile(t[:1], (70000, 1)).astype(np.uint32).ravel()
    for call in (lambda: ctx.mesh_topology(v, many), lambda: ctx.repair_mesh(v, many), lambda: ctx.repair_mesh(v, many, duplicates="keep", orient="consistent")):
        with pytest.raises(rnb.RnbError, match="repeated that often") as e:
            call()
        assert e.value.code == rnb._abi.ERR_INVALID and "65536" in str(e.value)
    ok = np.tile(t[:1], (1000, 1))
    got = _census(ctx, v, ok)  # below the cap the same shape goes through
    assert got["max_faces_on_edge"] == 1000 and got["n_duplicate_tris"] == 999
    _repair(ctx, v, ok, duplicates="cancel")
    _census(ctx, v, t)


def test_on_the_mesh_of_a_model():
    """extract_mesh(simplify, repair, topology) == the statement applied to what extract_mesh(simplify) returns; without the new arguments the call is what it was.
    The model is the one tests/test_gpu_mesh_clean.py and tests/test_gpu_mesh_simplify.py use, trained for 60 steps: seen on the MI355X, a context that is only
    initialised has no surface at threshold 0 on a 64^3 lattice (the mesh is empty, asserted against below), which would compare nothing."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(16, 128, 1400.0 * 128 / 800.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(60):
            c.train_step()
        kw = dict(res=64, cull="none", colors=True, normals=True, simplify=8)
        raw = c.extract_mesh(**kw)
        assert "repair_stats" not in raw and "topology" not in raw and len(raw["indices"]) > 0
        again = c.extract_mesh(**kw)
        for key in ("verts", "indices", "colors", "normals"):
            assert again[key].tobytes() == raw[key].tobytes()
        census = tr.expected_topology(len(raw["verts"]), raw["indices"])["stats"]
        print("the model's mesh clustered on 8^3 cells: %d triangles, %d duplicates, %d non-manifold edges" % (census["n_tris"], census["n_duplicate_tris"], census["n_nonmanifold_edges"]))
        got = c.extract_mesh(repair=dict(duplicates="cancel", orient="consistent"), topology=True, **kw)
        want = tr.expected_repair(raw["verts"], raw["indices"], colors=raw["colors"], normals=raw["normals"], duplicates="cancel", orient="consistent")
        tr.assert_equal_bits(got, {k: val for k, val in want.items() if k != "vertex_map"})
        assert all(got["simplify_stats"][k] == raw["simplify_stats"][k] for k in ("n_tris_out", "n_verts_out", "n_clusters"))  # the simplifier's, not the repair's
        assert {k: got["topology"][k] for k in tr.TOPOLOGY_STATS} == tr.expected_topology(len(want["verts"]), want["indices"])["stats"]
        only = c.extract_mesh(topology=True, **kw)
        assert {k: only["topology"][k] for k in tr.TOPOLOGY_STATS} == census and only["indices"].tobytes() == raw["indices"].tobytes()


def _obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.uint32).reshape(-1, 3)


def test_build_mesh_repairs_and_reports_the_topology(ctx, tmp_path):
    """`build/mesh --simplify 8 --repair --duplicates cancel --report-topology` on a snapshot trained here for 100 steps: the JSON line is DeviceMesh.topology() of the
    OBJ it wrote, the repaired mesh holds no duplicate, and without the flags neither line appears."""
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--cull", "none", "--simplify", "8"]
    out = str(tmp_path / "repaired.obj")
    r = subprocess.run(base + ["--out", out, "--repair", "--duplicates", "cancel", "--report-topology"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"topology"')]
    assert len(lines) == 1 and len([l for l in r.stdout.splitlines() if l.startswith("repair:")]) == 1, r.stdout
    print(lines[0])
    said = json.loads(lines[0])["topology"]
    v, f = _obj(out)
    census = ctx.mesh_topology(v, f.ravel())
    assert set(said) == set(tr.TOPOLOGY_STATS) and said == {k: census[k] for k in tr.TOPOLOGY_STATS}
    assert said["n_duplicate_tris"] == 0 and said["n_degenerate"] == 0 and said["n_tris"] == len(f) > 0
    plain = str(tmp_path / "plain.obj")
    r = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "repair:" not in r.stdout and "topology" not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
    pv, pf = _obj(plain)
    want = tr.expected_repair(pv, pf.ravel(), duplicates="cancel")
    assert (len(want["verts"]), len(want["indices"]) // 3) == (len(v), len(f))
    # with --keep / --orient as well the cleaning acts on the repaired mesh: one `clean:` line, after the `repair:` line
    r = subprocess.run(base + ["--out", out, "--repair", "--orient-consistent", "--keep", "largest", "--orient", "outward"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    heads = [l.split(":")[0] for l in r.stdout.splitlines() if l.startswith(("repair:", "clean:", "simplify:"))]
    assert heads == ["simplify", "repair", "clean"], r.stdout
