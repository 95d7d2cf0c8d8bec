"""The hole stage on the MI355X (include/rnb_mesh_holes.h) against the numpy statement of tests/mesh_holes_reference.py, bit for bit: the per-half-edge arrays, the loop
table, the statistics and the filled mesh with its colours and normals, on hand-made meshes of every kind (simple loops, pinches, inconsistent rims, unorientable), at the
wavefront, workgroup and scan boundaries, on one cycle of 2^17 + 1 edges, for every bucket count, against the topology stage's census, for every option, on invalid
input, and through build/mesh."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_holes_reference as hr
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


def _check(c, v, t, colors=None, normals=None, buckets_log2=0, **kw):
    """The census and the fill == the statement; n_loops == the topology stage's boundary components. Returns (the device's census, the device's filled mesh, the expected fill)."""
    i = np.asarray(t, np.uint32).ravel()
    census = c.mesh_boundary_loops(v, i, colors=colors, edges=True, table=True, buckets_log2=buckets_log2)
    hr.assert_equal_bits(census, hr.expected_boundary_loops(v, t, colors))
    assert census["n_loops"] == c.mesh_topology(v, i)["n_boundary_components"]
    got = c.fill_mesh_holes(v, i, colors=colors, normals=normals, loop_of_tri=True, buckets_log2=buckets_log2, **kw)
    want = hr.expected_fill(v, t, colors, normals, **kw)
    hr.assert_equal_bits(got, want)
    return census, got, want


def _closed_after(c, got):
    after = c.mesh_topology(got["verts"], got["indices"])
    assert after["closed"] == 1 and after["oriented"] == 1, after
    return after


def _cube_minus(tris):
    return hr.punch(*tr.cube(), tris)


def _sphere_with_disc_hole(n):
    """sphere(32) with the fan of one vertex removed, beside a separate disc(n) turned over: loops of the fan's valence and of n edges in two components."""
    v, t = tr.sphere(32)
    v, t = hr.punch_vertex_fans(v, t, [5])
    dv, dt = tr.disc(n)
    return np.concatenate([v, dv]), np.concatenate([t, dt[:, [0, 2, 1]] + len(v)])


def _touching_fans():
    v, t = tr.sphere(32)
    return hr.punch_vertex_fans(v, t, hr.touching_fans(t))


def _flipped_strip(n):
    v, t = tr.strip(n)
    return v, tr.flip_some(t, 0.4, n)


# fillable: every boundary component is a simple loop, so the fill closes the mesh
MESHES = {
    "disc": (lambda: tr.disc(9), True), "annulus": (lambda: tr.annulus(12), True), "moebius": (lambda: tr.moebius(16), False), "cube_minus_1": (lambda: _cube_minus([3]), True),
    "cube_minus_face": (lambda: _cube_minus([4, 5]), True), "touching_fans": (_touching_fans, False), "flipped_strip": (lambda: _flipped_strip(40), False),
    "cube": (tr.cube, True), "torus": (lambda: tr.torus_grid(8), True), "sphere_fans": (lambda: hr.punch_vertex_fans(*tr.sphere(32), [5, 900, 1500]), True),
    "sphere_tris": (lambda: hr.punch(*tr.sphere(32), [0, 1000, 2000]), True), "disc_1000": (lambda: tr.disc(1000), True),  # 10 ranking rounds
}
MESHES.update({"sphere_disc_%d" % n: ((lambda n=n: _sphere_with_disc_hole(n)), True) for n in (3, 4, 64, 65, 255, 256, 257)})  # one wavefront, one workgroup


@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_kind_of_mesh(ctx, name):
    make, fillable = MESHES[name]
    v, t = make()
    census, got, want = _check(ctx, v, t)
    assert "colors" not in got and "normals" not in got
    col, nrm = hr.coloured(v, len(name))
    _check(ctx, v, t, colors=col, normals=nrm)
    if fillable:
        assert census["n_simple"] == census["n_loops"] == got["stats"]["n_filled"]
        after = _closed_after(ctx, got)
        assert after["euler"] == ctx.mesh_topology(v, np.asarray(t, np.uint32).ravel())["euler"] + got["stats"]["n_filled"]
    else:
        assert got["stats"]["n_skipped_not_simple"] >= 1 and census["n_irregular_vertices"] >= 1


def test_a_thousand_loops_of_mixed_sizes(ctx):
    """The offsets of the appended vertices and triangles come from two exclusive sums over the table: 962 loops of 3, 4, 6 and 384 edges."""
    v, t, k = hr.grid_sheet_with_holes(96, 96)
    assert k == 961
    census, got, _ = _check(ctx, v, t)
    assert census["n_loops"] == 962 and sorted(set(census["table"]["n_edges"])) == [3, 4, 6, 384]
    _closed_after(ctx, got)
    col, nrm = hr.coloured(v, 3)
    _, got, _ = _check(ctx, v, t, colors=col, normals=nrm, skip_largest=True)
    assert got["stats"]["n_skipped_largest"] == 1 and got["stats"]["n_filled"] == 961
    after = ctx.mesh_topology(got["verts"], got["indices"])
    assert after["n_boundary_components"] == 1 and after["n_boundary_edges"] == 384  # exactly the rim is left


def test_one_long_cycle(ctx):
    """disc(2^17 + 1) under a random order of its triangles and a random numbering of its vertices: 18 ranking rounds; the loop is ordered exactly."""
    n = 2 ** 17 + 1
    v, t = tr.disc(n)
    rng = np.random.default_rng(17)
    v, t, _ = tr.renumber(v, t[rng.permutation(n)], rng)
    census, got, _ = _check(ctx, v, t)
    assert census["n_loops"] == 1 and census["max_loop_edges"] == n
    on = np.flatnonzero(census["loop"] != hr.NONE)
    assert len(on) == n and np.array_equal(np.sort(census["pos"][on]), np.arange(n))
    assert np.array_equal(census["pos"][census["next"][on]], (census["pos"][on].astype(np.int64) + 1) % n)  # pos rises by one along next
    _closed_after(ctx, got)


def test_the_bucket_count_changes_nothing(ctx):
    v, t, _ = hr.grid_sheet_with_holes(24, 24)
    col, nrm = hr.coloured(v, 1)
    i = t.astype(np.uint32).ravel()
    runs = [(ctx.mesh_boundary_loops(v, i, colors=col, edges=True, buckets_log2=b), ctx.fill_mesh_holes(v, i, col, nrm, loop_of_tri=True, buckets_log2=b)) for b in (4, 12, 0)]
    want_c, want_f = hr.expected_boundary_loops(v, t, col), hr.expected_fill(v, t, col, nrm)
    for census, fill in runs:
        hr.assert_equal_bits(census, want_c)
        hr.assert_equal_bits(fill, want_f)


def test_the_options(ctx):
    v, t, _ = hr.grid_sheet_with_holes(24, 24)
    for kw in (dict(max_edges=3), dict(max_edges=4), dict(max_edges=6), dict(max_edges=95), dict(max_edges=96), dict(skip_largest=True), dict(max_edges=4, skip_largest=True)):
        _, got, want = _check(ctx, v, t, **kw)
        st = got["stats"]
        assert st["n_filled"] + st["n_skipped_over_max"] + st["n_skipped_largest"] + st["n_skipped_not_simple"] == st["n_loops"]
    # skip_largest on two components: each keeps its own longest loop open, whatever the other holds
    sv, st_ = tr.sphere(32)
    sv, st_ = hr.punch_vertex_fans(sv, st_, [5, 900])
    st_ = hr.punch(sv, st_, [2000])[1]
    dv, dt = tr.annulus(12)
    both_v, both_t = np.concatenate([sv, dv]), np.concatenate([st_, dt + len(sv)])
    census, got, want = _check(ctx, both_v, both_t, skip_largest=True)
    assert len(set(census["table"]["component"])) == 2 and got["stats"]["n_skipped_largest"] == 2 and got["stats"]["n_filled"] == 3
    lot = got["loop_of_tri"]
    assert (lot[:len(both_t)] == hr.NONE).all() and set(lot[len(both_t):]) == set(want["filled"]) and len(lot) == got["stats"]["n_tris_out"]
    with ctx.upload_mesh(both_v, both_t.astype(np.uint32).ravel()) as m, m.fill_holes() as f:
        assert f.loop_of_tri is None and f.stats["n_filled"] == 5 and f.n_triangles == f.stats["n_tris_out"] and f.topology()["closed"] == 1


def test_invalid_input_fails_cleanly_and_leaves_the_context_usable(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    v, t = _cube_minus([4, 5])
    i = t.astype(np.uint32).ravel()
    calls = (lambda vv, ii: ctx.mesh_boundary_loops(vv, ii), lambda vv, ii: ctx.fill_mesh_holes(vv, ii))
    names = ("rnb_mesh_boundary_loops", "rnb_mesh_fill_holes")
    bad = i.copy()
    bad[7] = len(v)  # checked by a kernel before any index is used as an address
    nan = v.copy()
    nan[0, 1] = np.nan  # vertex 0 is on the hole's rim
    far = v.copy()
    far[0, 0] = 2.0 ** 11 + 0.25  # the anchor of the loop, 2^11 from the others: a - o is over the bound
    for call, name in zip(calls, names):
        for vv, ii, what in ((v, bad, "out of range"), (nan, i, "not finite"), (far, i, "2\\^10")):
            with pytest.raises(rnb.RnbError, match=what) as e:
                call(vv, ii)
            assert e.value.code == _abi.ERR_INVALID and name in str(e.value)
            _check(ctx, v, t)
    on_rim = np.unique(tr.cube()[1][[4, 5]])
    inside = v.copy()
    inside[[k for k in range(8) if k not in on_rim][0]] = np.nan  # not on the boundary: never read
    assert 0 in on_rim and ctx.mesh_boundary_loops(inside, i)["n_loops"] == 1
    f = ctx.f
    with ctx.upload_mesh(v, i) as m:
        out, tab = _abi.Mesh(), C.c_void_p(1)
        lopt, fopt = ctx._boundary_loops_options(), ctx._fill_holes_options()
        assert f.mesh_fill_holes(ctx._h, None, C.byref(m), C.byref(fopt), C.byref(m), None, None) == _abi.ERR_INVALID  # in == out: refused, the input untouched
        assert b"rnb_mesh_fill_holes" in f.last_error() and b"different objects" in f.last_error() and m.n_indices == len(i) and m.verts
        short = _abi.Mesh.from_buffer_copy(bytes(m))
        short.n_indices = len(i) - 2
        assert f.mesh_boundary_loops(ctx._h, None, C.byref(short), C.byref(lopt), None, None, None, C.byref(tab), None) == _abi.ERR_INVALID and not tab.value
        assert b"rnb_mesh_boundary_loops" in f.last_error() and b"multiple of 3" in f.last_error()
        out.n_indices = 9
        assert f.mesh_fill_holes(ctx._h, None, C.byref(short), C.byref(fopt), C.byref(out), None, None) == _abi.ERR_INVALID and bytes(out) == b"\0" * C.sizeof(out)
        assert b"rnb_mesh_fill_holes" in f.last_error() and b"multiple of 3" in f.last_error()
        lopt.abi_version = fopt.abi_version = 2
        tab.value = 1
        assert f.mesh_boundary_loops(ctx._h, None, C.byref(m), C.byref(lopt), None, None, None, C.byref(tab), None) == _abi.ERR_INVALID and not tab.value
        assert b"rnb_mesh_boundary_loops" in f.last_error() and b"abi_version" in f.last_error()
        assert f.mesh_fill_holes(ctx._h, None, C.byref(m), C.byref(fopt), C.byref(out), None, None) == _abi.ERR_INVALID and b"rnb_mesh_fill_holes" in f.last_error() and b"abi_version" in f.last_error()
    _check(ctx, v, t)
    # a mesh without triangles, and one without boundary
    e, z = np.zeros(0, np.uint32), np.zeros((5, 3), np.float32)
    _, got, _ = _check(ctx, z, e, colors=z)
    assert got["verts"].shape == (5, 3) and got["colors"].shape == (5, 3) and len(got["indices"]) == 0
    census, got, _ = _check(ctx, *tr.cube())
    assert census["n_loops"] == 0 and len(census["table"]) == 0 and (census["loop"] == hr.NONE).all() and got["stats"]["n_tris_added"] == 0


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


def test_build_mesh_fills_the_holes_keep_seen_faces_leaves(ctx, tmp_path):
    """`build/mesh --keep-seen faces --fill-holes --report-topology` on a snapshot trained here for 100 steps (the scene of the topology stage's command-line test): the
    mesh written is closed, where --keep-seen faces alone leaves boundary edges; the `fill:` line says what was closed."""
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--keep-seen", "faces", "--report-topology"]
    said = {}
    for name, flags in (("open", []), ("filled", ["--fill-holes"])):
        out = str(tmp_path / (name + ".obj"))
        r = subprocess.run(base + ["--out", out] + flags, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"topology"')]
        assert len(lines) == 1 and len([l for l in r.stdout.splitlines() if l.startswith("fill:")]) == len(flags), r.stdout
        print(name, lines[0])
        said[name] = json.loads(lines[0])["topology"]
        v, f = _obj(out)
        census = ctx.mesh_topology(v, f.ravel())
        assert said[name] == {k: census[k] for k in tr.TOPOLOGY_STATS}  # the line describes the mesh as written
    assert said["open"]["n_boundary_edges"] > 0 and said["open"]["closed"] == 0  # the views really left holes
    loops = ctx.mesh_boundary_loops(*[a.ravel() if a.dtype == np.uint32 else a for a in _obj(str(tmp_path / "open.obj"))])
    print("loops --keep-seen faces left: %d, %d simple, longest %d edges" % (loops["n_loops"], loops["n_simple"], loops["max_loop_edges"]))
    assert loops["n_simple"] == loops["n_loops"]  # else the filled mesh could not be closed: choose other views
    assert said["filled"]["closed"] == 1 and said["filled"]["n_boundary_edges"] == 0 and said["filled"]["n_tris"] > said["open"]["n_tris"]
