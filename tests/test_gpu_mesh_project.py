"""The view projection on the MI355X (include/rnb_mesh_project.h: DeviceMesh.project_views and the Context forms) against the numpy statement of
tests/mesh_project_reference.py: uv, color and info bit for bit over modes, normals, exponents, formats and fallbacks; occlusion with a known answer; nothing about the
cut shows; the consequences P7 of the header on the 500-step sphere of tests/test_gpu_mesh_sparse.py; the views' content arrives; the model as the fallback; refusals;
build/mesh --texture-from end to end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_project_reference as pr
from tests import mesh_texture_reference as tr
from tests.test_gpu_mesh_sparse import KW, _scene
from tests.test_mesh_project_cpu import front_view, quad, refusals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTER = np.array([0.5, 0.5, 0.5])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def _view(w, h, f, eye, target=CENTER):
    from rnb_neus2_amd import synthetic
    return dict(width=w, height=h, focal_length=(f, f * 1.03), principal_point=(0.5, 0.48), xform=synthetic.look_at_c2w(np.asarray(eye, np.float64), np.asarray(target, np.float64)).astype(np.float32))


def small_scene():
    """The perturbed octahedron of mesh_texture_reference (split once: 32 triangles) and a two-triangle blocker between it and the last camera; vertex normals (radial, +z on
    the blocker, perturbed); four views: one that the object overflows (off-screen), one from inside the object (behind, flat), one plain, one of 300 x 200 in which a
    triangle's box holds thousands of pixels (the large fill path) and the blocker hides a part of the object (occluded)."""
    verts, tris = tr.octahedron(1)
    rng = np.random.default_rng(11)
    verts = (verts + rng.uniform(-0.02, 0.02, verts.shape)).astype(np.float32)
    qv = np.float32([[0.45, 0.40, 1.1], [0.62, 0.40, 1.1], [0.45, 0.62, 1.1], [0.62, 0.62, 1.1]])
    qt = np.uint32([[0, 1, 2], [2, 1, 3]]) + len(verts)
    normals = np.concatenate([verts - np.float32(0.5), np.tile(np.float32([0, 0, 1]), (4, 1))]) + rng.uniform(-0.05, 0.05, (len(verts) + 4, 3)).astype(np.float32)
    views = [_view(24, 20, 60.0, CENTER + 1.2 * np.array([1.0, 0.2, 0.1])), _view(33, 47, 30.0, CENTER + np.array([0.1, 0.02, 0.03]), CENTER + np.array([1.0, 0.0, 0.0])),
             _view(64, 48, 70.0, CENTER + np.array([-0.35, -1.1, 0.45])), _view(300, 200, 400.0, CENTER + np.array([0.0, 0.2, 1.3]))]
    return np.concatenate([verts, qv]), np.concatenate([tris, qt]), normals.astype(np.float32), views


def random_images(fmt, seed):
    """Random RGBA of sizes that are not the views', a band of alpha 0 across the middle third of the rows."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(((17, 23), (40, 31), (50, 70), (128, 96))):
        kind = fmt if fmt != "mixed" else ("float32", "uint16", "uint8", "uint16")[k]
        if kind == "float32":
            a = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
            a[..., 3] = rng.uniform(0.2, 1.0, (h, w)).astype(np.float32)
        else:
            a = rng.integers(0, np.iinfo(kind).max + 1, (h, w, 4)).astype(kind)
            a[..., 3] = np.maximum(a[..., 3], np.iinfo(kind).max // 5)
        a[h // 3:2 * h // 3, :, 3] = 0
        out.append(a)
    return out


CASES = [  # size, block, mode, normals, weight_power, format, fallback
    (32, 0, "blend", "face", 2, "float32", False), (64, 0, "best", "vertex", 0, "uint16", True), (67, 9, "blend", "vertex", 5, "uint8", False), (64, 9, "best", "face", 2, "mixed", True),
    (67, 0, "blend", "face", 0, "uint16", True), (32, 0, "best", "vertex", 5, "float32", False)]


def test_the_statement_bit_for_bit(ctx):
    """color, info, uv and the four counts equal the statement in every bit over CASES; the case set reaches every way a (texel, view) pair can end, by the statement's
    own tallies."""
    v, t, n, views = small_scene()
    assert len(t) == 34
    total = dict.fromkeys(pr.SKIPS + ("contributed",), 0)
    for k, (size, block, mode, normals, power, fmt, fb) in enumerate(CASES):
        images = random_images(fmt, 100 + k)
        fallback = np.random.default_rng(k).uniform(0, 1, (size, size, 4)).astype(np.float32) if fb else None
        kw = dict(size=size, block=block, mode=mode, weight_power=power, fallback=fallback)
        want = pr.project(v, t, views, images, normals=normals, vnormals=n, **kw)
        got = ctx.project_views(v, t, views, images, normals=n, shading=normals, **kw)
        pr.assert_equal_bits(got, want)
        assert got["stats"]["peak_workspace"] >= size * size * 24 and got["stats"]["ms"] > 0
        for key in total:
            total[key] += want["tallies"][key]
        assert 0 < want["stats"]["n_textured"] < want["stats"]["n_texels"], CASES[k]
    print("pairs:", total)
    for key in total:
        assert total[key] > 0, key
    with ctx.upload_mesh(v, t, normals=n) as m:  # normals=None on the handle: the vertex normals when the mesh has them
        a = m.project_views(views, random_images("uint16", 3), size=64)
    pr.assert_equal_bits(a, pr.project(v, t, views, random_images("uint16", 3), 64, normals="vertex", vnormals=n))
    e = ctx.project_views(v[:0], t[:0], views, random_images("uint8", 3), size=16)  # a mesh without triangles: zero maps
    assert not e["color"].any() and not e["info"].any() and e["uv"].shape == (0, 3, 2) and e["stats"]["n_texels"] == 0


def test_occlusion_with_a_known_answer(ctx):
    """One camera, a plane and a smaller blocker in front of it (the scene of the CPU tier): every plane texel whose projection lies at least one pixel inside the
    blocker's outline has count 0, every one at least one pixel outside has count 1."""
    v0, t0 = quad(0.2, 0.8, 0.5)
    v1, t1 = quad(0.4, 0.6, 0.0)  # its shadow on the plane z = 0.5, seen from z = -1, is [0.35, 0.65]^2
    v, t = np.concatenate([v0, v1]), np.concatenate([t0, t1 + 4])
    r = ctx.project_views(v, t, [front_view(256, 192, 240.0)], [np.full((8, 8, 4), 255, np.uint8)], size=64)
    pos = tr.positions(v, t, 64, r["block"], r["blocks_per_row"])
    tri, _ = tr.ownership(4, 64, r["block"], r["blocks_per_row"])
    plane = (tri >= 0) & (tri < 2)
    far = np.maximum(np.abs(pos[..., 0] - 0.5), np.abs(pos[..., 1] - 0.5))
    pixel = 1.5 / 240.0
    inside, outside = plane & (far < 0.15 - pixel), plane & (far > 0.15 + pixel)
    assert inside.sum() > 50 and outside.sum() > 500
    assert (r["info"][inside, 0] == 0).all() and (r["info"][inside, 1] == 0xFFFFFFFF).all() and (r["info"][outside, 0] == 1).all() and (r["info"][outside, 1] == 0).all()
    assert (r["color"][outside] == 1).all() and (r["color"][inside] == [0, 0, 0, 1]).all() and r["stats"]["n_occluded"] >= inside.sum()


def test_nothing_about_the_cut_shows(ctx):
    """The driver batches neither texels nor views (one launch per view over all texels): two calls, and a call on a second upload, give the same bits."""
    v, t, n, views = small_scene()
    images = random_images("mixed", 5)
    runs = [ctx.project_views(v, t, views, images, normals=n, size=67, block=9) for _ in range(2)]
    with ctx.upload_mesh(v, t, normals=n) as m:
        runs.append(m.project_views(views, images, size=67, block=9))
    for r in runs[1:]:
        for key in ("uv", "color", "info"):
            assert np.array_equal(_bits(r[key]), _bits(runs[0][key])), key
        assert {k: x for k, x in r["stats"].items() if k != "ms"} == {k: x for k, x in runs[0]["stats"].items() if k != "ms"}


# ------------------------------------------------------------------------------------------------------------------------ the sphere
L_FIELD = 1.0


def field(p):
    """f(p) = 0.5 + (p - 0.5) per channel: |f_c(p) - f_c(q)| <= |p - q|, Lipschitz constant L = 1 in every channel."""
    return 0.5 + (np.asarray(p, np.float64) - 0.5)


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
    yield c, views
    c.close()


@pytest.fixture(scope="module")
def sphere32(trained):
    """The res-32 extraction without culling, with normals; per view an image of the field: the mesh rasterised into the view, the world point of every covered pixel
    rebuilt from its depth and the camera in numpy, image = f(point), alpha = coverage. The statement at S = 512 on these, computed once and left unchanged."""
    c, views = trained
    images, z_far = [], 0.0
    with c.extract_mesh_device(32, cull="none", normals=True) as m:
        mesh = m.download()
        for view in views:
            img = m.rasterize(view)["image"]
            h, w = img.shape[:2]
            x = np.asarray(view["xform"], np.float64).reshape(3, 4)
            j, i = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
            z = img[..., 7].astype(np.float64)
            xc = (i - view["principal_point"][0] * w) / view["focal_length"][0] * z
            yc = (j - view["principal_point"][1] * h) / view["focal_length"][1] * z
            point = x[:, 3] + xc[..., None] * x[:, 0] + yc[..., None] * x[:, 1] + z[..., None] * x[:, 2]
            rgba = np.zeros((h, w, 4), np.float32)
            rgba[..., :3] = field(point) * (img[..., 6:7] > 0)
            rgba[..., 3] = img[..., 6]
            images.append(rgba)
            z_far = max(z_far, float(z.max()))
    tris = mesh["indices"].reshape(-1, 3)
    assert 1000 < len(tris) < 10000
    want = pr.project(mesh["verts"], tris, views, images, 512, normals="vertex", vnormals=mesh["normals"])
    assert want["block"] >= 6
    return mesh, tris, images, z_far, want


def test_the_views_content_arrives(trained, sphere32):
    """On texels with count > 0: |rgb - f(p)| <= L * F, F the worst footprint of a pixel on the surface in world units.
    Derivation. rgb is a convex combination (bilinear weights times alpha >= 0 within a view, cos^k * q_a > 0 across views) of the values f(P) at the surface points P
    that the rays of the covered taps meet, so |rgb - f(p)| <= L * max |P - p|. The taps are pixel centres within one pixel of p's projection in each axis (the images
    have the views' resolution), so their rays pass within r = sqrt(2) * z_far / f of p, z_far the greatest depth any view sees. A texel reaches at most two texel steps
    = 2 / n of an edge beyond its triangle (the gutter), g = 2 / n * the longest edge. Seen at a cosine above min_cos, a distance r + g across the ray is at most
    (r + g) / min_cos along the plane of the texel's triangle; the surface leaves that plane by at most the sagitta s = ((r + g) / min_cos)^2 / (2 R), R the smallest
    distance of a vertex from the centre; and p may lie behind the nearest surface of its pixel by depth_tolerance * z_far. F = (r + g) / min_cos + s + tol * z_far.
    2e-6 is added for the float32 storage of depth, image and result. Measured on an MI355X: max |rgb - f(p)| = 3.3e-3 against a bound of 2.7e-1 (r = g = 9.6e-3, z_far 1.51; the
    division by min_cos = 0.1 is what makes the bound loose: most texels are seen at cosines near 1), all 234416 owned texels textured; printed below. The textured fraction is printed; asserted are only that
    count equals the statement's (in every bit, with color and uv), and a floor of one half."""
    c, views = trained
    mesh, tris, images, z_far, want = sphere32
    got = c.project_views(mesh["verts"], tris, views, images, normals=mesh["normals"], size=512)
    pr.assert_equal_bits(got, want)
    own = want["own"]
    count = got["info"][own][:, 0]
    seen = count > 0
    err = np.abs(got["color"][own][seen][:, :3].astype(np.float64) - field(want["positions"][seen].astype(np.float64))).max()
    v = mesh["verts"].astype(np.float64)
    edge = max(np.linalg.norm(v[tris[:, a]] - v[tris[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    min_cos, tol, f = 0.1, 2.0 ** -8, min(min(vw["focal_length"]) for vw in views)
    r, g, radius = np.sqrt(2.0) * z_far / f, 2.0 / (want["block"] - 3) * edge, np.linalg.norm(v - CENTER, axis=1).min()
    lateral = (r + g) / min_cos
    bound = L_FIELD * (lateral + lateral * lateral / (2.0 * radius) + tol * z_far) + 2e-6
    print("textured %d of %d owned texels (%.4f); max |rgb - f(p)| = %.3e, bound %.3e (r %.3e, g %.3e, z_far %.3f)" % (seen.sum(), len(seen), seen.mean(), err, bound, r, g, z_far))
    assert err <= bound
    assert seen.mean() >= 0.5


def test_consequences_on_the_sphere(trained, sphere32):
    """P7 with normals = VERTEX: views that all hold one constant opaque colour give (float) c on every texel with count > 0 (within 1 ulp, expected 0); the n + 1 texels
    along an edge are equal bit for bit, color and info, in the two triangles that share it; a permutation of the views leaves count unchanged."""
    c, views = trained
    mesh, tris, images, _, want = sphere32
    size, b, bpr = 512, want["block"], want["blocks_per_row"]
    with c.upload_mesh(mesh["verts"], tris, normals=mesh["normals"]) as m:
        const = np.tile(np.uint16([12345, 40000, 65535, 65535]), (9, 7, 1))
        flat = m.project_views(views, [const] * len(views), size=size)
        perm = np.random.default_rng(3).permutation(len(views))
        moved = m.project_views([views[k] for k in perm], [images[k] for k in perm], size=size)
        best = m.project_views(views, images, size=size, mode="best")
        blend = m.project_views(views, images, size=size)
    seen = flat["info"][..., 0] > 0
    assert seen.sum() > 100000
    target = (const[0, 0, :3].astype(np.float64) / 65535.0).astype(np.float32)
    ulps = np.abs(_bits(flat["color"][seen][:, :3]).astype(np.int64) - _bits(target).astype(np.int64))
    print("constant colour: %d of %d values off by one ulp, none by more" % ((ulps == 1).sum(), ulps.size))
    assert ulps.max() <= 1 and (flat["color"][seen][:, 3] == 1).all()
    assert np.array_equal(moved["info"][..., 0], want["info"][..., 0]) and (moved["info"][..., 1] != want["info"][..., 1]).any()
    edges = {}
    for t, tri in enumerate(tris):
        for q in range(3):
            v0, v1 = int(tri[q]), int(tri[(q + 1) % 3])
            edges.setdefault((min(v0, v1), max(v0, v1)), []).append((t, q, v0 < v1))
    assert all(len(e) == 2 for e in edges.values()), "the mesh is not closed"
    rows, cols = [[], []], [[], []]
    for pair in edges.values():
        for side, (t, q, forward) in enumerate(pair):
            r, cc = tr.edge_texels(size, b, bpr, t, q, (q + 1) % 3) if forward else tr.edge_texels(size, b, bpr, t, (q + 1) % 3, q)  # from the lower vertex number up
            rows[side].append(r), cols[side].append(cc)
    r0, c0, r1, c1 = (np.concatenate(a) for a in (rows[0], cols[0], rows[1], cols[1]))
    assert len(r0) == len(edges) * (b - 2) and ((r0 != r1) | (c0 != c1)).all()
    for name, res in (("blend", blend), ("best", best), ("constant", flat)):
        for key in ("color", "info"):
            assert np.array_equal(_bits(res[key][r0, c0]), _bits(res[key][r1, c1])), (name, key)
    assert (blend["info"][r0, c0, 0] > 0).mean() > 0.9


def test_the_model_as_the_fallback(trained, sphere32):
    """Three views leave the far side without a view: every owned texel with count 0 is, bit for bit, the baker's albedo texel; the others are the projection without a
    fallback; the training state is the same before and after."""
    c, views = trained
    mesh, tris, images, _, _ = sphere32
    names = ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID")
    before = {k: c.get(k).copy() for k in names}
    with c.upload_mesh(mesh["verts"], tris, normals=mesh["normals"]) as m:
        baked = m.bake_texture(512)
        plain = m.project_views(views[:3], images[:3], size=512)
        filled = m.project_views(views[:3], images[:3], size=512, fallback="model")
    for k in names:
        assert np.array_equal(c.get(k).view(np.uint8), before[k].view(np.uint8)), k
    own, none = baked["albedo"][..., 3] == 1, plain["info"][..., 0] == 0
    assert np.array_equal(own, plain["color"][..., 3] == 1) and 10000 < (own & none).sum() < own.sum() - 10000
    assert np.array_equal(filled["info"], plain["info"]) and np.array_equal(_bits(filled["uv"]), _bits(baked["uv"]))
    assert np.array_equal(_bits(filled["color"][own & none]), _bits(baked["albedo"][own & none]))
    assert np.array_equal(_bits(filled["color"][~none]), _bits(plain["color"][~none])) and not _bits(filled["color"][~own]).any()
    assert (plain["color"][own & none] == [0, 0, 0, 1]).all()


def test_refusals(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi, api
    v, t, n, views = small_scene()
    images = random_images("uint8", 9)
    good = ctx.project_views(v, t, views, images, size=64)
    res = refusals(ctx.f, _abi, api, ctx._h)  # the list of the header, on a live context (nothing of it reaches the device)
    for label, rc, msg in res:
        assert rc == _abi.ERR_INVALID and msg, label
    bad = t.copy()
    bad[5, 1] = len(v)  # found by the range-check kernel, not by a fault
    for kw in (dict(tris=bad), dict(size=16), dict(size=64, block=3), dict(size=3)):
        with pytest.raises(rnb.RnbError) as err:
            ctx.project_views(v, kw.pop("tris", t), views, images, **dict(dict(size=64), **kw))
        assert err.value.code == _abi.ERR_INVALID, kw
    with ctx.upload_mesh(v, bad) as m:  # the raw call: the result and the statistics come back zeroed
        opt = ctx._project_options(64, 0, "blend", "face", 2, 0.1, 2.0 ** -8, 2.0 ** -10, "none")
        arr, arrays = ctx._project_views(views, images)
        held = [ctx.upload(a) for a in arrays]
        try:
            for e, p in zip(arr, held):
                e.image_dev = p
            pj, st = _abi.MeshProjection(), _abi.MeshProjectStats()
            pj.uv, pj.n_tris, st.n_occluded = 0x40, 7, 3
            assert ctx.f.mesh_project_views(ctx._h, None, C.byref(m), arr, len(arr), C.byref(opt), C.byref(pj), C.byref(st)) == _abi.ERR_INVALID
            assert b"out of range" in ctx.f.last_error() and bytes(pj) == bytes(C.sizeof(pj)) and bytes(st) == bytes(C.sizeof(st))
        finally:
            for p in held:
                ctx.device_free(p)
    again = ctx.project_views(v, t, views, images, size=64)  # the context still works
    for key in ("uv", "color", "info"):
        assert np.array_equal(_bits(again[key]), _bits(good[key])), key


def test_build_mesh_texture_from_views_end_to_end(tmp_path):
    """`build/mesh --texture 256 --texture-from views` on a snapshot the testbed wrote: OBJ, MTL and PNG exist, the vt records are those of the run without
    --texture-from, and the albedo image differs from that run's (the scene's albedo maps are white: the projected texels are 255)."""
    from rnb_neus2_amd import hostlib, synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    outs = {}
    for name, extra in (("model", []), ("views", ["--texture-from", "views", "--texture-mode", "blend", "--texture-depth-tolerance", "0.00390625", "--texture-min-cos", "0.1"])):
        out = str(tmp_path / (name + ".obj"))
        r = subprocess.run([os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--out", out, "--resolution", "128", "--keep", "largest", "--orient", "outward",
                            "--simplify", "16", "--texture", "256"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        print(r.stdout)
        assert len([l for l in r.stdout.splitlines() if l.startswith("texture from 12 views (blend)")]) == (1 if extra else 0)
        for suffix in (".obj", ".mtl", "_albedo.png"):
            assert os.path.exists(tmp_path / (name + suffix)), name + suffix
        outs[name] = ([l for l in open(out).read().splitlines() if l.startswith("vt ")], hostlib.png_read(str(tmp_path / (name + "_albedo.png"))))
    assert outs["views"][0] == outs["model"][0] and len(outs["views"][0]) > 300
    a, b = outs["views"][1], outs["model"][1]
    assert a.shape == b.shape == (256, 256, 3) and np.array_equal(a.any(axis=2), b.any(axis=2))  # the same footprint
    assert (a != b).any() and (a == 255).all(axis=2).sum() > 1000
