"""The smoothing stage on the MI355X (include/rnb_mesh_smooth.h) against the numpy statement of tests/mesh_smooth_reference.py, bit for bit: vertices, normals, the
census arrays, the displacement and the statistics, on every kind of mesh of the hole stage's table under each boundary mode, on fans whose centre crosses the per-vertex
path threshold and the wavefront and workgroup sizes, for odd and even pass counts, with a selection, for every bucket count, on invalid input, and through build/mesh."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_holes_reference as hr
from tests import mesh_smooth_reference as sr
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


def _check(c, v, t, colors=None, normals_in=None, buckets_log2=0, **kw):
    """The smoothed mesh with its census and displacement == the statement. Returns (the device's dict, the expected one)."""
    i = np.asarray(t, np.uint32).ravel()
    got = c.smooth_mesh(v, i, colors=colors, normals_in=normals_in, displacement=True, census=True, buckets_log2=buckets_log2, **kw)
    want = sr.expected_smooth(v, t, colors, normals_in, **kw)
    sr.assert_equal_bits(got, want)
    return got, want


def _check_normals(c, v, t, flip=False):
    got = c.mesh_vertex_normals(v, np.asarray(t, np.uint32).ravel(), flip=flip)
    sr.assert_equal_bits(got, sr.expected_normals(v, t, flip))
    return got


def _cube_minus(tris):
    return hr.punch(*tr.cube(), tris)


def _sphere_with_disc_hole(n):
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


def _duplicates_on_an_edge():
    """The cube with one triangle three times and a degenerate one: an edge with 4 faces beside manifold ones."""
    v, t = tr.cube()
    return v, np.concatenate([t, t[[3, 3]], [[1, 1, 5]]])


# the kinds of the hole stage's table (tests/test_gpu_mesh_holes.py), and a mesh with duplicate triangles on one edge
MESHES = {
    "disc": lambda: tr.disc(9), "annulus": lambda: tr.annulus(12), "moebius": lambda: tr.moebius(16), "cube_minus_1": lambda: _cube_minus([3]),
    "cube_minus_face": lambda: _cube_minus([4, 5]), "touching_fans": _touching_fans, "flipped_strip": lambda: _flipped_strip(40),
    "cube": tr.cube, "torus": lambda: tr.torus_grid(8), "sphere_fans": lambda: hr.punch_vertex_fans(*tr.sphere(32), [5, 900, 1500]),
    "sphere_tris": lambda: hr.punch(*tr.sphere(32), [0, 1000, 2000]), "disc_1000": lambda: tr.disc(1000), "book": lambda: tr.book(5),
    "two_cubes": tr.two_cubes_sharing_an_edge, "duplicates": _duplicates_on_an_edge,
}
MESHES.update({"sphere_disc_%d" % n: (lambda n=n: _sphere_with_disc_hole(n)) for n in (3, 4, 64, 65, 255, 256, 257)})


@pytest.mark.parametrize("name", sorted(MESHES))
def test_every_kind_of_mesh(ctx, name):
    v, t = MESHES[name]()
    col, nrm = hr.coloured(v, len(name))
    for boundary in ("pin", "slide", "free"):
        got, want = _check(ctx, v, t, boundary=boundary)
        assert "colors" not in got and "normals" not in got
        got, _ = _check(ctx, v, t, colors=col, normals_in=nrm, boundary=boundary)
        assert got["colors"].tobytes() == col.tobytes() and got["normals"].tobytes() == nrm.tobytes()
        still = ~want["moving"]
        assert got["verts"][still].tobytes() == np.asarray(v, np.float32)[still].tobytes() and (got["displacement"][still] == 0).all()
    st = got["stats"]
    assert st["n_interior"] + st["n_boundary"] + st["n_nonmanifold"] + st["n_unused"] == len(v) and st["n_edges"] == ctx.mesh_topology(v, np.asarray(t, np.uint32).ravel())["n_edges"]
    _check_normals(ctx, v, t)
    _check_normals(ctx, v, t, flip=True)


@pytest.mark.parametrize("n", [31, 32, 33, 63, 64, 65, 255, 256, 257, 2 ** 17 + 1])
def test_a_fan_centre_on_every_path(ctx, n):
    """disc(n) under a random order of its triangles and a random numbering of its vertices, 20 passes with boundary="slide": the centre has n neighbours, which crosses
    the threshold between a thread and a workgroup per vertex (32), the wavefront (64) and the workgroup (256); the rim vertices have 2."""
    v, t = tr.disc(n)
    rng = np.random.default_rng(n)
    v, t, _ = tr.renumber(v, t[rng.permutation(n)], rng)
    v = (v + rng.normal(0, 0.002, v.shape)).astype(np.float32)
    got, want = _check(ctx, v, t, passes=20, boundary="slide")
    assert got["stats"]["max_valence"] == n and got["stats"]["n_moving"] == n + 1 and got["stats"]["n_wide"] == (1 if n > 32 else 0)
    assert got["stats"]["max_displacement"] > 0
    normals = _check_normals(ctx, v, t)
    assert normals["max_corners"] == n


def test_odd_and_even_passes_and_plain_laplacian(ctx):
    v, t = hr.punch_vertex_fans(*tr.sphere(32), [5, 900])
    rng = np.random.default_rng(2)
    v = (v + rng.normal(0, 0.003, v.shape)).astype(np.float32)
    seen = []
    for passes in (0, 1, 2, 3):
        got, _ = _check(ctx, v, t, passes=passes)
        seen.append(got["verts"].tobytes())
        assert got["stats"]["passes"] == passes
    assert seen[0] == v.tobytes() and len(set(seen)) == 4
    a, _ = _check(ctx, v, t, passes=4, mu=0.0)
    b, _ = _check(ctx, v, t, passes=4)
    assert a["verts"].tobytes() != b["verts"].tobytes()
    _check(ctx, v, t, passes=7, lam=1.0, mu=-1.5, boundary="free")


def test_a_selection_moves_only_what_it_selects(ctx):
    """grid_sheet_with_holes(24, 24) after fill_holes, only the appended vertices selected, rings 0, 1, 5: every unselected vertex is bit-equal to the input."""
    v, t, _ = hr.grid_sheet_with_holes(24, 24)
    f = ctx.fill_mesh_holes(v, t.astype(np.uint32).ravel())
    fv, ft = f["verts"], f["indices"].reshape(-1, 3)
    select = np.arange(len(fv)) >= len(v)
    assert f["stats"]["n_verts_added"] == select.sum() > 0
    moved = []
    for rings in (0, 1, 5):
        got, want = _check(ctx, fv, ft, select=select, select_rings=rings, boundary="free")
        sel = sr.selection(len(fv), sr.edges(len(fv), ft.astype(np.int64))[0], select, rings)
        assert got["stats"]["n_selected"] == sel.sum() and got["verts"][~sel].tobytes() == fv[~sel].tobytes() and (got["displacement"][~sel] == 0).all()
        moved.append(int((got["displacement"] > 0).sum()))
    assert 0 < moved[0] < moved[1] < moved[2]
    with ctx.upload_mesh(fv, f["indices"]) as m, m.smooth(select=select.astype(np.uint8), select_rings=1) as s:
        assert s.displacement is None and s.kind is None and s.stats["n_selected"] > select.sum() and s.n_verts == len(fv)


def test_the_bucket_count_changes_nothing(ctx):
    v, t, _ = hr.grid_sheet_with_holes(24, 24)
    col, nrm = hr.coloured(v, 1)
    want = sr.expected_smooth(v, t, col, nrm, boundary="slide")
    for b in (4, 12, 0):
        got = ctx.smooth_mesh(v, t.astype(np.uint32).ravel(), colors=col, normals_in=nrm, boundary="slide", displacement=True, census=True, buckets_log2=b)
        sr.assert_equal_bits(got, want)


def test_recomputed_normals_are_those_of_the_output(ctx):
    v, t = hr.punch_vertex_fans(*tr.sphere(32), [5])
    _, nrm = hr.coloured(v, 5)
    for given in (None, nrm):
        got, _ = _check(ctx, v, t, normals_in=given, normals="recompute", passes=4)
        again = ctx.mesh_vertex_normals(got["verts"], got["indices"])
        assert got["normals"].tobytes() == again["normals"].tobytes()
        lengths = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
        assert (lengths == 0).sum() == 1 and lengths[5] == 0 and np.abs(lengths[lengths > 0] - 1).max() < 1e-6  # vertex 5 lost its fan: no triangle uses it
    with ctx.upload_mesh(v, t.astype(np.uint32).ravel()) as m:
        on = m.vertex_normals(on_device=True)  # the caller's from here on
        try:
            want = sr.expected_normals(v, t)
            assert ctx.download(on["normals"], len(v) * 3, np.float32).tobytes() == want["normals"].tobytes() and on["n_zero"] == want["stats"]["n_zero"]
        finally:
            ctx.device_free(on["normals"])


def test_invalid_input_fails_cleanly_and_leaves_the_context_usable(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    v, t = _cube_minus([4, 5])  # the rim of the missing face: vertices 0, 1, 4, 5; the others are interior
    i = t.astype(np.uint32).ravel()
    on_rim = np.unique(tr.cube()[1][[4, 5]])
    inner = [k for k in range(8) if k not in on_rim]
    bad = i.copy()
    bad[7] = len(v)  # checked by a kernel before any index is used as an address
    nan = v.copy()
    nan[inner[0], 1] = np.nan  # an interior vertex: it moves
    far = v.copy()
    far[inner[0], 0] = 2.0 ** 11 + 0.25
    for vv, ii, what in ((v, bad, "out of range"), (nan, i, "2\\^10"), (far, i, "2\\^10")):
        with pytest.raises(rnb.RnbError, match=what) as e:
            ctx.smooth_mesh(vv, ii)
        assert e.value.code == _abi.ERR_INVALID and "rnb_mesh_smooth" in str(e.value)
        _check(ctx, v, t)
    with pytest.raises(rnb.RnbError, match="out of range"):
        ctx.mesh_vertex_normals(v, bad)
    with pytest.raises(rnb.RnbError, match="2\\^3"):
        ctx.mesh_vertex_normals(far, i)
    # a NaN on a pinned vertex that neighbours nothing moving is copied, and is no error: a strip has boundary vertices only
    sv, st = tr.strip(12)
    sv[3, 2] = np.nan
    got, _ = _check(ctx, sv, st)
    assert got["stats"]["n_moving"] == 0 and np.isnan(got["verts"][3, 2])
    with pytest.raises(ValueError):
        sr.expected_smooth(nan, t)
    f = ctx.f
    with ctx.upload_mesh(v, i) as m:
        out = _abi.Mesh()
        opt = ctx._smooth_options()
        assert f.mesh_smooth(ctx._h, None, C.byref(m), C.byref(opt), None, C.byref(m), None, None, None, None) == _abi.ERR_INVALID  # in == out: refused, the input untouched
        assert b"rnb_mesh_smooth" in f.last_error() and b"different objects" in f.last_error() and m.n_indices == len(i) and m.verts
        for field, value, what in (("abi_version", 2, b"abi_version"), ("passes", 10001, b"passes"), ("lambda_", 0.0, b"lambda"), ("mu", 0.5, b"mu"), ("boundary", 3, b"boundary")):
            opt = ctx._smooth_options()
            setattr(opt, field, value)
            out.n_indices = 9
            assert f.mesh_smooth(ctx._h, None, C.byref(m), C.byref(opt), None, C.byref(out), None, None, None, None) == _abi.ERR_INVALID and bytes(out) == b"\0" * C.sizeof(out), field
            assert b"rnb_mesh_smooth" in f.last_error() and what in f.last_error()
        nopt = ctx._vertex_normals_options()
        nopt.abi_version = 2
        assert f.mesh_vertex_normals(ctx._h, None, C.byref(m), C.byref(nopt), None, None) == _abi.ERR_INVALID
    _check(ctx, v, t)
    # a mesh without triangles, and one without vertices
    e, z = np.zeros(0, np.uint32), np.zeros((5, 3), np.float32)
    got, _ = _check(ctx, z, e, colors=z)
    assert got["verts"].shape == (5, 3) and got["colors"].shape == (5, 3) and got["stats"]["n_unused"] == 5
    assert _check_normals(ctx, z, e)["n_zero"] == 5
    got, _ = _check(ctx, np.zeros((0, 3), np.float32), e, normals="recompute")
    assert got["verts"].shape == (0, 3) and got["normals"].shape == (0, 3)


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


def test_build_mesh_smooths_what_the_fill_leaves(ctx, tmp_path):
    """`build/mesh --keep-seen faces --fill-holes --smooth 10 --report-topology` on a snapshot trained here for 100 steps (the scene of the hole stage's command-line
    test): the `smooth:` line is there, the topology line is the one of the run without --smooth, and the vertices differ."""
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "64", "--keep-seen", "faces", "--fill-holes", "--report-topology"]
    said, meshes = {}, {}
    for name, flags in (("filled", []), ("smoothed", ["--smooth", "10"])):
        out = str(tmp_path / (name + ".obj"))
        r = subprocess.run(base + ["--out", out] + flags, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"topology"')]
        smooth_lines = [l for l in r.stdout.splitlines() if l.startswith("smooth:")]
        assert len(lines) == 1 and len(smooth_lines) == len(flags) // 2, r.stdout
        print(name, lines[0], smooth_lines)
        said[name] = json.loads(lines[0])["topology"]
        meshes[name] = _obj(out)
    assert said["filled"] == said["smoothed"]
    (v0, f0), (v1, f1) = meshes["filled"], meshes["smoothed"]
    assert f0.tobytes() == f1.tobytes() and v0.shape == v1.shape and (v0 != v1).any()
