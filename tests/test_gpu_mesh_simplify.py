"""The mesh simplifier on the MI355X (include/rnb_mesh_simplify.h) against the numpy statement of tests/mesh_simplify_reference.py, bit for bit: vertices, indices,
colours, normals and the counts of the statistics, on uploaded meshes (three spheres, a fan of 2^16 triangles in one cluster, 4096 components under a random numbering,
a strip alternating between two clusters, triangle counts that are no multiple of the wavefront or the workgroup), under permutations and renumberings, on degenerate
and invalid input, on the mesh of a model, beside training, and through build/mesh."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_simplify_reference as sr

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


@pytest.fixture(scope="module")
def spheres():
    v, i = mc.three_spheres(64)
    rng = np.random.default_rng(5)
    return v, i, rng.random((len(v), 3), dtype=np.float32), rng.standard_normal((len(v), 3)).astype(np.float32)


def _check(c, v, i, colors=None, normals=None, **grid):
    got = c.simplify_mesh(v, i, colors=colors, normals=normals, **grid)
    want = sr.expected(v, i, colors=colors, normals=normals, **grid)
    sr.assert_equal_bits(got, want)
    return got, want


@pytest.mark.parametrize("n", [16, 8])
@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_three_spheres(ctx, spheres, n, placement):
    v, i, col, nrm = spheres
    got, want = _check(ctx, v, i, col, nrm, origin=(0, 0, 0), cell=1.0 / n, dims=n, placement=placement)
    assert 0 < got["stats"]["n_tris_out"] < len(i) // 3 and sr.directed_edge_balance(got["indices"]) == 0
    got, _ = _check(ctx, v, i, origin=(0, 0, 0), cell=1.0 / n, dims=n, placement=placement)  # without attributes
    assert "colors" not in got and "normals" not in got
    cut = i[: 3 * (len(i) // 3 - 37)]  # 7899 triangles: no multiple of 64 or 256 (the full mesh has 31 * 256)
    assert (len(cut) // 3) % 64 and len(i) // 3 % 256 == 0
    _check(ctx, v, cut, col, nrm, origin=(0.01, -0.02, 0.03), cell=1.0 / n, dims=(n, n + 1, n - 1), placement=placement)


def test_permuted_triangles_renumbered_vertices_and_repeated_calls(ctx, spheres):
    v, i, col, nrm = spheres
    grid = dict(origin=(0, 0, 0), cell=1.0 / 16, dims=16)
    a = ctx.simplify_mesh(v, i, col, nrm, **grid)
    b = ctx.simplify_mesh(v, i, col, nrm, **grid)
    for key in ("verts", "indices", "colors", "normals"):
        assert a[key].tobytes() == b[key].tobytes(), key  # two calls in a row: the same bits
    rng = np.random.default_rng(2)
    t = i.reshape(-1, 3)
    perm = rng.permutation(len(t))
    p, want = _check(ctx, v, t[perm].ravel(), col, nrm, **grid)
    kept = sr.expected(v, i, **grid)["tri_kept"]
    pos = np.cumsum(kept) - 1
    for key in ("verts", "colors", "normals"):
        assert p[key].tobytes() == a[key].tobytes(), key
    assert np.array_equal(p["indices"].reshape(-1, 3), a["indices"].reshape(-1, 3)[pos[perm[kept[perm]]]])  # the triangles permuted accordingly, nothing else
    new_of_old = rng.permutation(len(v))
    w, wc, wn = np.empty_like(v), np.empty_like(col), np.empty_like(nrm)
    w[new_of_old], wc[new_of_old], wn[new_of_old] = v, col, nrm
    r, _ = _check(ctx, w, new_of_old[t].ravel(), wc, wn, **grid)
    for key in ("verts", "indices", "colors", "normals"):
        assert r[key].tobytes() == a[key].tobytes(), key  # a renumbering changes nothing at all


def _renumber(v, t, rng):
    new_of_old = rng.permutation(len(v))
    out = np.empty_like(v)
    out[new_of_old] = v
    return out, new_of_old[t]


def test_wavefront_reduction_corners(ctx):
    rng = np.random.default_rng(11)
    # a fan of 2^16 triangles inside ONE cell, tied to two other cells by one more triangle: the cluster's sums (2^16 + 1 quadrics, 2^16 + 2 members) are in the output
    n = 1 << 16
    ang = 2 * np.pi * np.arange(n + 1) / n
    rim = np.stack([1.5 + 0.4 * np.cos(ang), 1.5 + 0.4 * np.sin(ang), 1.5 + 0.1 * np.sin(3 * ang)], 1)
    v = np.concatenate([[(1.5, 1.5, 1.7)], rim, [(3.2, 1.4, 1.5), (1.6, 3.3, 1.4)]]).astype(np.float32)
    k = np.arange(n)
    t = np.concatenate([np.stack([np.zeros(n, np.int64), 1 + k, 2 + k], 1), [[0, n + 2, n + 3]]])
    got, _ = _check(ctx, v, t.astype(np.uint32).ravel(), origin=(0, 0, 0), cell=1.0, dims=4)
    assert got["stats"]["n_clusters"] == 3 and got["stats"]["n_tris_out"] == 1 and got["stats"]["n_tris_collapsed"] == n
    fv, ft = _renumber(v, t, rng)
    _check(ctx, fv, ft[rng.permutation(len(ft))].astype(np.uint32).ravel(), colors=rng.random((len(v), 3), dtype=np.float32), origin=(0, 0, 0), cell=1.0, dims=4, placement="mean")
    # 4096 tetrahedra, each with its corners in four cells of its own 2 x 2 x 2 block of a 32^3 grid, numbered at random: no two lanes of a wavefront share a cluster
    corner = np.array([(0.3, 0.4, 0.2), (1.6, 0.3, 0.4), (0.4, 1.7, 0.6), (1.3, 1.4, 1.8)])
    b = np.arange(4096)
    block = np.stack([b % 16, (b // 16) % 16, b // 256], 1) * 2.0
    jitter = rng.random((4096, 4, 3)) * 0.1
    tv = ((block[:, None, :] + corner[None, :, :] + jitter) / 32.0).reshape(-1, 3).astype(np.float32)
    tt = (np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)])[None, :, :] + 4 * b[:, None, None]).reshape(-1, 3)
    tv, tt = _renumber(tv, tt, rng)
    got, _ = _check(ctx, tv, tt[rng.permutation(len(tt))].astype(np.uint32).ravel(), normals=rng.standard_normal((len(tv), 3)).astype(np.float32), origin=(0, 0, 0), cell=1.0 / 32, dims=32)
    assert got["stats"]["n_clusters"] == 16384 and got["stats"]["n_tris_out"] == 16384
    got, _ = _check(ctx, tv, tt.astype(np.uint32).ravel(), origin=(0, 0, 0), cell=1.0 / 16, dims=16)  # one block = one cell: 4096 components in 4096 cells, all collapse
    assert got["stats"]["n_clusters"] == 4096 and got["stats"]["n_tris_out"] == 0 and got["verts"].shape == (0, 3)
    # a strip whose lower row lies in one cell and whose upper row in the next: consecutive triangles alternate between the two clusters (1999 triangles)
    m = 1000
    x = 0.05 + 0.9 * np.arange(m) / m
    lo = np.stack([x, np.full(m, 0.9), 0.5 + 0.1 * np.sin(7 * x)], 1)
    hi = np.stack([x + 0.0004, np.full(m, 1.1), 0.5 + 0.1 * np.cos(5 * x)], 1)
    sv = np.concatenate([lo, hi, [(2.5, 1.0, 0.5)]]).astype(np.float32)
    a = np.arange(m - 1)
    st = np.stack([np.stack([a, a + 1, a + m], 1), np.stack([a + 1, a + m + 1, a + m], 1)], 1).reshape(-1, 3)  # interleaved: lower-led, upper-led, ...
    st = np.concatenate([st, [[m - 1, 2 * m, 2 * m - 1]]])
    assert len(st) == 1999
    got, _ = _check(ctx, sv, st.astype(np.uint32).ravel(), origin=(0, 0, 0), cell=1.0, dims=4)
    assert got["stats"]["n_clusters"] == 3 and got["stats"]["n_tris_out"] == 1


TETRA_T = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2], np.uint32)


def _tetra(scale=1.0):
    return (np.array([(0.1, 0.1, 0.1), (0.7, 0.2, 0.15), (0.2, 0.8, 0.25), (0.3, 0.3, 0.9)], np.float64) * scale).astype(np.float32)


def test_degenerate_and_boundary_cases(ctx):
    col = np.arange(12, dtype=np.float32).reshape(4, 3) / 16
    nrm = np.array([(0, 0, 2), (0, -3, 0), (1, 1, 0), (0, 0, 0)], np.float32)
    for pl in ("quadric", "mean"):
        got, _ = _check(ctx, _tetra(), TETRA_T, col, nrm, origin=(0, 0, 0), cell=1.0, dims=4, placement=pl)  # one cell: an empty mesh
        assert got["verts"].shape == (0, 3) and got["indices"].shape == (0,) and got["colors"].shape == (0, 3)
        got, _ = _check(ctx, _tetra(4.0), TETRA_T, col, nrm, origin=(0, 0, 0), cell=1.0, dims=4, placement=pl)  # each vertex in its own cell
        assert got["stats"]["n_verts_out"] == 4 and got["stats"]["n_tris_out"] == 4
        v = _tetra(4.0)
        v[1] = (5.5, 0.5, 0.5)  # outside the grid
        v[2] = (1.0, 3.0, 1.0)  # exactly on cell faces
        _check(ctx, v, TETRA_T, col, nrm, origin=(0, 0, 0), cell=1.0, dims=4, placement=pl)
        _check(ctx, _tetra(4.0), TETRA_T, origin=(0, 0, 0), cell=1.0, dims=(4, 4, 1), placement=pl)  # dims of 1 on an axis
        _check(ctx, _tetra(4.0), TETRA_T, origin=(-1, -1, -1), cell=8.0, dims=1, placement=pl)  # one cell in all
    g = np.arange(9)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    fv = np.stack([gx.ravel() / 8.0, gy.ravel() / 8.0, np.full(81, 0.3)], 1).astype(np.float32)
    q = (gy[:-1, :-1] * 9 + gx[:-1, :-1]).ravel()
    ft = np.concatenate([np.stack([q, q + 1, q + 9], 1), np.stack([q + 1, q + 10, q + 9], 1), [[0, 0, 5], [3, 4, 5]]]).astype(np.uint32)  # flat, + a repeated corner, + zero area
    got, _ = _check(ctx, fv, ft.ravel(), origin=(0, 0, 0), cell=0.25, dims=5)
    assert got["stats"]["n_fallback"] == 0
    got = ctx.simplify_mesh(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), colors=np.zeros((5, 3), np.float32))  # an empty input: an empty mesh
    sr.assert_equal_bits(got, sr.expected(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), colors=np.zeros((5, 3), np.float32)))


def test_invalid_input_fails_cleanly_and_the_context_stays_usable(ctx, spheres):
    from rnb_neus2_amd import _abi
    v, i, col, nrm = spheres
    grid = dict(origin=(0, 0, 0), cell=1.0 / 16, dims=16)
    f = ctx.f
    pv = ctx.upload(v)
    try:
        for bad_value in (len(v), 0xFFFFFFFF):
            bad = i.copy()
            bad[len(bad) // 2] = bad_value
            pi = ctx.upload(bad)
            try:
                m, out = _abi.Mesh(), _abi.Mesh()
                m.verts, m.indices, m.n_verts, m.n_indices = pv, pi, len(v), len(bad)
                out.n_verts, out.verts = 5, 64
                opt = ctx._simplify_options((0, 0, 0), 1.0 / 16, 16, "quadric")
                assert f.mesh_simplify(ctx._h, None, C.byref(m), C.byref(opt), C.byref(out), None) == _abi.ERR_INVALID
                assert bytes(out) == b"\0" * C.sizeof(out) and b"out of range" in f.last_error()
                m.n_indices = len(bad) - 2  # not a multiple of 3
                out.n_indices = 9
                assert f.mesh_simplify(ctx._h, None, C.byref(m), C.byref(opt), C.byref(out), None) == _abi.ERR_INVALID
                assert bytes(out) == b"\0" * C.sizeof(out)
                m.n_indices = len(bad)
                for field, value in (("cell", 0.0), ("dims", (4096, 4096, 4096))):  # cell = 0, a dims product over the cap
                    opt = ctx._simplify_options((0, 0, 0), 1.0 / 16, 16, "quadric")
                    if field == "dims":
                        opt.dims[:] = value
                    else:
                        opt.cell = value
                    out.n_verts = 3
                    assert f.mesh_simplify(ctx._h, None, C.byref(m), C.byref(opt), C.byref(out), None) == _abi.ERR_INVALID
                    assert bytes(out) == b"\0" * C.sizeof(out)
            finally:
                ctx.device_free(pi)
            _check(ctx, v, i, **grid)  # a following valid call succeeds
    finally:
        ctx.device_free(pv)
    # a NaN no triangle uses is accepted; one a triangle uses fails the call, in a coordinate or in a carried attribute
    w = np.concatenate([v, np.full((1, 3), np.nan, np.float32)])
    _check(ctx, w, i, np.concatenate([col, np.full((1, 3), np.nan, np.float32)]), **grid)
    w = v.copy()
    w[i[7], 1] = np.nan
    with pytest.raises(Exception, match="not finite"):
        ctx.simplify_mesh(w, i, **grid)
    _check(ctx, v, i, **grid)
    wc = col.copy()
    wc[i[100], 2] = np.inf
    with pytest.raises(Exception, match="not finite"):
        ctx.simplify_mesh(v, i, colors=wc, **grid)
    with pytest.raises(Exception, match="below"):  # a vertex 2^23 cells outside the grid: its local position is over the term bound
        ctx.simplify_mesh(_tetra(2.0 ** 23), TETRA_T, origin=(0, 0, 0), cell=1.0, dims=4)
    _check(ctx, v, i, col, nrm, **grid)


MODEL_STEPS = 60


def test_on_the_mesh_of_a_model():
    """A model trained for MODEL_STEPS steps (the size tests/test_gpu_mesh_clean.py uses): extract_mesh(res=128, simplify=32) equals the statement applied to the
    extracted mesh, simplify_mesh on the downloaded mesh gives the same, keep="largest" combined with simplify equals the two calls in sequence, and extract_mesh without
    the new arguments returns what it did."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(16, 128, 1400.0 * 128 / 800.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(MODEL_STEPS):
            c.train_step()
        kw = dict(res=128, cull="none", colors=True, normals=True)
        raw = c.extract_mesh(**kw)
        assert "simplify_stats" not in raw and len(raw["indices"]) > 3000
        origin, cell, dims = c.simplify_grid((0, 0, 0), (1, 1, 1), 32)
        assert (origin, cell, dims) == ((0.0, 0.0, 0.0), 1.0 / 32, (32, 32, 32))
        for pl in ("quadric", "mean"):
            want = sr.expected(raw["verts"], raw["indices"], raw["colors"], raw["normals"], origin=origin, cell=cell, dims=dims, placement=pl)
            direct = c.extract_mesh(simplify=32, placement=pl, **kw)
            sr.assert_equal_bits(direct, want)
            assert direct["stats"]["n_bricks"] == raw["stats"]["n_bricks"] and "clean_stats" not in direct
            sr.assert_equal_bits(c.simplify_mesh(raw["verts"], raw["indices"], raw["colors"], raw["normals"], origin=origin, cell=cell, dims=dims, placement=pl), want)
        print("the model's mesh: %d -> %d triangles, %d clamped, %d at the mean" % (len(raw["indices"]) // 3, want["stats"]["n_tris_out"], want["stats"]["n_clamped"], want["stats"]["n_fallback"]))
        assert 0 < want["stats"]["n_tris_out"] < len(raw["indices"]) // 3
        cleaned = c.extract_mesh(keep="largest", orient="outward", **kw)
        both = c.extract_mesh(keep="largest", orient="outward", simplify=32, **kw)
        sr.assert_equal_bits(both, sr.expected(cleaned["verts"], cleaned["indices"], cleaned["colors"], cleaned["normals"], origin=origin, cell=cell, dims=dims))
        assert both["clean_stats"]["n_tris_out"] == cleaned["clean_stats"]["n_tris_out"] == both["simplify_stats"]["n_tris_in"]
        again = c.extract_mesh(**kw)
        for key in ("verts", "indices", "colors", "normals"):
            assert again[key].tobytes() == raw[key].tobytes()  # the default call is what it was


def test_simplifying_leaves_training_untouched(spheres):
    """deterministic = 1: 40 steps, a simplify_mesh and an extract_mesh(simplify=...), 40 steps == 80 steps, bit for bit."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    v, i, col, nrm = spheres
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(80):
            if interrupt and s == 40:
                c.simplify_mesh(v, i, col, nrm, origin=(0, 0, 0), cell=1.0 / 16, dims=16)
                c.extract_mesh(64, cull="none", keep="largest", colors=True, simplify=16)
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


def _obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append(p[1:4])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, object).reshape(-1, 3), np.asarray(f, np.uint32).reshape(-1, 3)


def _context_of(path):
    """A context holding what build/mesh loads from a snapshot (as tests/test_gpu_render_cli.py builds one): the EMA weights, the occupancy grid, the step."""
    import msgpack
    import rnb_neus2_amd as rnb
    with open(path, "rb") as f:
        root = msgpack.unpackb(f.read(), raw=False)
    enc, snap = root["encoding"], root["snapshot"]
    c = rnb.Context(n_levels=enc["n_levels"], log2_hashmap_size=enc["log2_hashmap_size"], base_resolution=enc["base_resolution"], per_level_scale=enc["per_level_scale"],
                    valid_level_scale=enc["valid_level_scale"], base_valid_level_scale=enc["base_valid_level_scale"], base_training_step=enc["base_training_step"],
                    sdf_bias=root["network"]["sdf_bias"], apply_no_albedo=1, aabb_scale=int(snap["nerf"]["aabb_scale"]))
    c.set_params(np.frombuffer(snap["params_binary"], np.float16).astype(np.float32))
    c.put("DENSITY_GRID", np.frombuffer(snap["density_grid_binary"], np.float16).astype(np.float32))
    c.update_density_bitfield()
    c.set_training_step(snap["training_step"])
    return c


def test_build_mesh_simplify_writes_the_counts_of_the_python_call(tmp_path):
    """`build/mesh --resolution 128 --simplify 32 [--keep largest --orient outward] [--placement mean]` on a snapshot the testbed wrote, against
    Context.extract_mesh(res=128, simplify=32, ...) on a context that holds the same snapshot: the OBJ has the vertex and face counts of the Python call, which are also
    the counts of the program's `simplify:` line, and without the flag nothing of it runs."""
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128"]
    r = subprocess.run(base + ["--out", str(tmp_path / "full.obj")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "simplify:" not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
    fv, ff = _obj(str(tmp_path / "full.obj"))
    with _context_of(snap) as c:
        assert c.cfg.aabb_scale == 1  # the scene box build/mesh lays the cells over is the unit cube
        for flags, kw in (([], {}), (["--keep", "largest", "--orient", "outward"], dict(keep="largest", orient="outward")), (["--placement", "mean"], dict(placement="mean"))):
            r = subprocess.run(base + ["--out", str(tmp_path / "small.obj"), "--simplify", "32"] + flags, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
            line = [l for l in r.stdout.splitlines() if l.startswith("simplify:")]
            assert len(line) == 1, r.stdout
            print(line[0])
            m = re.match(r"simplify: (\d+) clusters, (\d+) -> (\d+) triangles \((\d+) collapsed\), (\d+) -> (\d+) vertices", line[0])
            n_clusters, tris_in, tris_out, collapsed, verts_in, verts_out = (int(x) for x in m.groups())
            sv, sf = _obj(str(tmp_path / "small.obj"))
            assert (len(sv), len(sf)) == (verts_out, tris_out) and tris_in - tris_out == collapsed and 0 < tris_out < tris_in
            if not flags:
                assert (len(fv), len(ff)) == (verts_in, tris_in)
            got = c.extract_mesh(res=128, colors=True, simplify=32, **kw)
            st = got["simplify_stats"]
            assert (len(sv), len(sf)) == (len(got["verts"]), len(got["indices"]) // 3) == (st["n_verts_out"], st["n_tris_out"])
            assert (st["n_clusters"], st["n_tris_in"], st["n_verts_in"]) == (n_clusters, tris_in, verts_in)
