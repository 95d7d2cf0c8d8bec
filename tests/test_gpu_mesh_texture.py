"""The texture baker on the MI355X (include/rnb_mesh_texture.h) against the numpy statement of tests/mesh_texture_reference.py and against the network itself: the
atlas, the position map and the footprint bit for bit; no bit depends on the batching; the albedo is the network's at the texel's position; a corner texel holds what
the extractor gives the vertex; the texels along a shared edge are equal in both triangles; training is left alone; bad arguments are refused; build/mesh --texture
end to end. The model is the 500-step sphere of tests/test_gpu_mesh_sparse.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_texture_reference as tr
from tests.test_gpu_mesh_sparse import KW, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("albedo", "normal", "position")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def trained():
    """A sphere trained for 500 steps on 16 views at 128 x 128 (the model of tests/test_gpu_mesh_sparse.py)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene()
    c = rnb.Context(**KW)
    c.init_params()
    c.set_dataset(views, normals, albedos)
    for _ in range(500):
        c.train_step()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere32(trained):
    """The res-32 extraction without culling, with the vertex attributes, and its bake at S = 512 with every map (computed once, shared, left unchanged)."""
    with trained.extract_mesh_device(32, cull="none", colors=True, normals=True) as m:
        mesh = m.download()
        baked = m.bake_texture(512, maps=ALL)
    tris = mesh["indices"].reshape(-1, 3)
    assert 1000 < len(tris) < 10000 and baked["block"] >= 6
    return mesh, tris, baked


def test_the_statement_bit_for_bit(trained):
    c = trained
    verts, tris8 = tr.octahedron()
    rng = np.random.default_rng(5)
    verts = (verts + rng.uniform(-0.02, 0.02, verts.shape)).astype(np.float32)
    for tris in (tris8, tris8[:7], tris8[:1], tris8[:0]):
        nt = len(tris)
        for size, block in ((64, 0), (67, 5), (16, 4), (64, 16)):
            lay = tr.layout(nt, size, block)
            b, bpr = lay["block"], lay["blocks_per_row"]
            out = c.bake_texture(verts, tris, size, block, maps=ALL)
            assert (out["block"], out["blocks_per_row"]) == (b, bpr), (nt, size, block)
            assert out["uv"].shape == (nt, 3, 2) and np.array_equal(_bits(out["uv"]), _bits(tr.uvs(nt, size, b, bpr)))
            assert np.array_equal(_bits(out["position"]), _bits(tr.positions(verts, tris, size, b, bpr))), (nt, size, block)
            owner, _ = tr.ownership(nt, size, b, bpr)
            assert (owner >= 0).sum() == (nt // 2) * b * b + (nt % 2) * (b * (b + 1) // 2)
            for name in ALL:
                assert out[name].shape == (size, size, 4) and out[name].dtype == np.float32
                assert np.array_equal(out[name][..., 3], (owner >= 0).astype(np.float32)), (name, nt, size, block)
                assert not _bits(out[name])[owner < 0].any(), (name, nt, size, block)  # all zeros outside, -0 included
                assert np.isfinite(out[name]).all()
            st = out["stats"]
            assert st["n_texels"] == lay["n_blocks"] * b * b and st["n_batches"] == (1 if nt else 0) and st["peak_workspace"] >= 3 * size * size * 16 and st["ms"] > 0
            only = c.bake_texture(verts, tris, size, block, maps=("position",))  # without the network
            assert sorted(only) == ["block", "blocks_per_row", "position", "stats", "uv"] and only["stats"]["n_texels"] == 0 and only["stats"]["n_batches"] == 0
            assert np.array_equal(_bits(only["position"]), _bits(out["position"]))
    assert c.texture_layout(8, 64) == dict(block=32, blocks_per_row=2, n_blocks=4)


def test_batching_cannot_show(trained, sphere32):
    c = trained
    mesh, tris, first = sphere32
    b = first["block"]
    with c.upload_mesh(mesh["verts"], mesh["indices"]) as m:
        runs = [m.bake_texture(512, maps=ALL, max_texels_in_flight=k) for k in (0, 0, 1000, b * b)]
    assert 1000 % (b * b) != 0
    n_texels = first["stats"]["n_texels"]
    assert [r["stats"]["n_batches"] for r in runs] == [1, 1, -(-n_texels // 1000), n_texels // (b * b)]
    for r in runs:
        assert r["block"] == b
        for name in ALL + ("uv",):
            assert np.array_equal(_bits(r[name]), _bits(first[name])), name


def test_values_are_the_networks(trained, sphere32):
    """The albedo of every owned texel against the recipe of test_colours_and_gradient_normals (tests/test_gpu_mesh_sparse.py): Context.forward_infer at coordinates built
    in numpy from the downloaded position map, EMA weights, a float64 logistic. The same half outputs, so the difference is the device's float expf and one float
    division: bound 1e-6, the bound that test carries for the same kernels and the same arithmetic (measured there on an MI355X: 6.0e-8; here the maximum is printed).
    Normal texels are unit length or zero."""
    c = trained
    _, _, baked = sphere32
    own = baked["position"][..., 3] == 1
    v = baked["position"][own][:, :3]
    assert len(v) > 100000
    d = v - np.float32(0.5)
    l = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32)
    coords = np.zeros((len(v), 7), np.float32)
    coords[:, 0:3] = np.clip((v - np.float32(0.0)) / np.float32(1.0), np.float32(0.0), np.float32(1.0))  # (the header's clamp: every texel of this mesh is inside the box)
    assert np.array_equal(coords[:, 0:3], v)
    coords[:, 4:7] = (d / l[:, None] + np.float32(1.0)) * np.float32(0.5)
    chunk = KW["target_batch_size"] * 8
    out = np.concatenate([c.forward_infer(coords[k:k + chunk], inference=True) for k in range(0, len(coords), chunk)]).astype(np.float64)
    want = 1.0 / (1.0 + np.exp(-out[:, 0:3]))
    got = baked["albedo"][own][:, :3]
    err = np.abs(got.astype(np.float64) - want).max()
    print("albedo: max |d| %.3e over %d texels" % (err, len(v)))
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert err < 1e-6
    n = baked["normal"][own][:, :3].astype(np.float64)
    length = np.sqrt((n * n).sum(1))
    nz = np.linalg.norm(out[:, 4:7], axis=1) > 0
    print("normal: %d of %d texels with a zero gradient, max | |n| - 1 | %.3e" % ((~nz).sum(), len(n), np.abs(length[nz] - 1.0).max()))
    assert np.abs(length[nz] - 1.0).max() < 1e-5 and not n[~nz].any()
    assert nz.mean() > 0.99


def test_corners_are_the_vertices(sphere32):
    """The albedo and the normal at the three corner texels of every triangle are, bit for bit, the colour and the normal extract_mesh_device gave the vertex; the position
    is the vertex."""
    mesh, tris, baked = sphere32
    size, b, bpr = 512, baked["block"], baked["blocks_per_row"]
    t = np.arange(len(tris))
    k = t // 2
    corner = tr.corners(b)[t & 1]  # [nt, 3, 2]
    x, y = ((k % bpr) * b)[:, None] + corner[..., 0], ((k // bpr) * b)[:, None] + corner[..., 1]
    for name, attr in (("position", "verts"), ("albedo", "colors"), ("normal", "normals")):
        got = baked[name][y, x]  # [nt, 3, 4]
        assert (got[..., 3] == 1).all()
        assert np.array_equal(_bits(got[..., :3]), _bits(mesh[attr][tris])), name
    assert mesh["colors"].min() > 0 and np.abs(np.linalg.norm(mesh["normals"], axis=1) - 1).max() < 1e-5  # (the attributes are there)


def test_no_seams_at_edge_texels(sphere32):
    """The mesh is closed; for every edge, the n + 1 texels along it in its two triangles are equal bit for bit in all three maps (b >= 6: there are interior edge texels)."""
    mesh, tris, baked = sphere32
    size, b, bpr = 512, baked["block"], baked["blocks_per_row"]
    assert b >= 6
    edges = {}
    for t, tri in enumerate(tris):
        for q in range(3):
            v0, v1 = int(tri[q]), int(tri[(q + 1) % 3])
            edges.setdefault((min(v0, v1), max(v0, v1)), []).append((t, q, v0 < v1))
    assert all(len(e) == 2 for e in edges.values()), "the mesh is not closed"
    rows, cols = [[], []], [[], []]
    for pair in edges.values():
        for side, (t, q, forward) in enumerate(pair):
            r, c = tr.edge_texels(size, b, bpr, t, q, (q + 1) % 3) if forward else tr.edge_texels(size, b, bpr, t, (q + 1) % 3, q)  # from the lower vertex number up
            rows[side].append(r), cols[side].append(c)
    r0, c0, r1, c1 = (np.concatenate(a) for a in (rows[0], cols[0], rows[1], cols[1]))
    assert len(r0) == len(edges) * (b - 2) and ((r0 != r1) | (c0 != c1)).all()
    for name in ALL:
        a, bb = baked[name][r0, c0], baked[name][r1, c1]
        assert (a[:, 3] == 1).all()
        assert np.array_equal(_bits(a), _bits(bb)), name


def test_the_bake_leaves_training_untouched():
    """deterministic = 1: 50 steps, bakes with both sets of weights, 50 steps == 100 steps, bit for bit (the per-step statistics and the weights)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene(8, 96)
    verts, tris = tr.octahedron(2)
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(100):
            if interrupt and s == 50:
                c.bake_texture(verts, tris, 256, maps=ALL)
                c.bake_texture(verts, tris, 64, maps=("albedo",), inference=False, max_texels_in_flight=500)
            stats.append(c.train_step().as_dict())
        state = {k: c.get(k).copy() for k in ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID")}
        for st in stats:
            st.pop("prep_ms"), st.pop("step_ms")
        runs.append((state, stats))
        c.close()
    (sa, ta), (sb, tb) = runs
    assert ta == tb
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def test_refusals(trained):
    import ctypes as C
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    c = trained
    verts, tris = tr.octahedron(1)
    good = c.bake_texture(verts, tris, 64)
    bad = tris.copy()
    bad[5, 1] = len(verts)  # found by the range-check kernel, not by a fault
    for kw in (dict(size=3), dict(size=8193), dict(size=64, maps=0), dict(size=64, maps=()), dict(size=16, block=8), dict(size=64, block=3), dict(size=64, tris=bad)):
        with pytest.raises(rnb.RnbError) as err:
            c.bake_texture(verts, kw.pop("tris", tris), **kw)
        assert err.value.code == _abi.ERR_INVALID, kw
    assert "out of range" in str(err.value)
    with c.upload_mesh(verts, bad) as m:  # the raw call: the result and the statistics come back zeroed
        opt = c._texture_options(64, 0, ALL, True, 0)
        tex, st = _abi.MeshTexture(), _abi.MeshTextureStats()
        tex.uv, tex.n_tris, st.n_batches = 0x40, 7, 3
        assert c.f.mesh_bake_texture(c._h, None, C.byref(m), C.byref(opt), C.byref(tex), C.byref(st)) == _abi.ERR_INVALID
        assert bytes(tex) == bytes(C.sizeof(tex)) and bytes(st) == bytes(C.sizeof(st))
    again = c.bake_texture(verts, tris, 64)  # the context still works
    assert np.array_equal(_bits(again["albedo"]), _bits(good["albedo"])) and (good["albedo"][..., 3] == 1).sum() == len(tris) // 2 * good["block"] ** 2


def test_build_mesh_texture_end_to_end(tmp_path):
    """`build/mesh --texture 128 --texture-maps albedo,normal --simplify 16` on a snapshot the testbed wrote: the four files, 3 nt `vt` records that are the statement's
    for nt triangles, and an albedo image that is zero exactly where channel 3 of a bake of the OBJ's own geometry through the Python API is zero. (The footprint only:
    the OBJ's printed decimals move the positions, and with them the values.)"""
    from rnb_neus2_amd import hostlib, meshproc, synthetic
    from tests.test_gpu_mesh_simplify import _context_of
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    out = str(tmp_path / "baked.obj")
    r = subprocess.run([os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--out", out, "--resolution", "128", "--keep", "largest", "--orient", "outward",
                        "--simplify", "16", "--texture", "128", "--texture-maps", "albedo,normal"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    print(r.stdout)
    assert len([l for l in r.stdout.splitlines() if l.startswith("texture: 128^2 texels")]) == 1
    for name in ("baked.obj", "baked.mtl", "baked_albedo.png", "baked_normal.png"):
        assert os.path.exists(tmp_path / name), name
    m = meshproc.load_obj(out)
    nt = len(m.faces)
    assert nt > 100
    lines = open(out).read().splitlines()
    vt = np.float32([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("vt ")])
    lay = tr.layout(nt, 128)
    assert vt.shape == (3 * nt, 2) and np.array_equal(vt.reshape(nt, 3, 2), tr.uvs(nt, 128, lay["block"], lay["blocks_per_row"]))
    faces = [[w.split("/") for w in l.split()[1:]] for l in lines if l.startswith("f ")]
    assert all(int(w[1]) == 3 * t + q + 1 and w[0] == w[2] for t, f in enumerate(faces) for q, w in enumerate(f))  # written as they are (--orient outward)
    mtl = open(tmp_path / "baked.mtl").read()
    assert "map_Kd baked_albedo.png" in mtl and "baked_normal.png" in mtl
    a8, n16 = hostlib.png_read(str(tmp_path / "baked_albedo.png")), hostlib.png_read(str(tmp_path / "baked_normal.png"))
    assert a8.shape == (128, 128, 3) and a8.dtype == np.uint8 and n16.shape == (128, 128, 3) and n16.dtype == np.uint16
    with _context_of(snap) as c:
        api_bake = c.bake_texture(m.vertices.astype(np.float32), m.faces.astype(np.uint32), 128)
    assert (api_bake["block"], api_bake["blocks_per_row"]) == (lay["block"], lay["blocks_per_row"])
    owned = api_bake["albedo"][..., 3] == 1
    assert np.array_equal(a8.any(axis=2), owned) and 0 < owned.sum() < owned.size
    assert (n16[~owned] == 32768).all()  # n = 0 outside
    r = subprocess.run([os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--out", out, "--texture", "8"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "the smallest size that would fit" in r.stderr  # a mesh the texture cannot hold fails the run, with the library's message
