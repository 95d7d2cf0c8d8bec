"""The textured draw on the MI355X (include/rnb_mesh_draw.h: DeviceMesh.draw_textured and the Context forms) against the numpy statement of
tests/mesh_draw_reference.py: image, faces and counts bit for bit over sizes, blocks, filters, maps, shadings and culls; the fill is the rasteriser's; the baker's
position map comes back as the point under the pixel; a constant map gives the constant; the normal-mapped, simplified sphere through mesh_view_metrics; permutation;
training untouched; refusals; build/mesh --texture --report-views end to end."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_draw_reference as dr
from tests import mesh_texture_reference as tr
from tests.test_gpu_mesh_project import small_scene
from tests.test_gpu_mesh_sparse import KW, _scene
from tests.test_mesh_draw_cpu import position_bound, random_maps, refusals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def awkward_texture(size, block, seed):
    """random_maps of the CPU tier (alpha 0 on the texels no triangle owns, a few all-zero normal texels) with one NaN uv corner and one triangle whose uv leaves [0, 1]."""
    uv, color, normal, lay = random_maps(size, seed, block=block)
    uv = uv.copy()
    uv[3, 1, 0] = np.nan
    uv[8] = uv[8] * 3.0 - 1.0
    return uv, color, normal, lay


CASES = [  # size, block, filter, maps, shading, cull
    (32, 0, "bilinear", "both", "face", "none"), (64, 9, "nearest", "color", "vertex", "back"), (67, 9, "bilinear", "normal", "vertex", "none"), (64, 0, "nearest", "both", "face", "back"),
    (67, 0, "bilinear", "color", "face", "none"), (32, 0, "nearest", "normal", "vertex", "back"), (64, 9, "bilinear", "both", "vertex", "none")]


def test_the_statement_bit_for_bit(ctx):
    """Image, faces, the rasteriser's counts and the three counts of the draw equal the statement in every bit over CASES and the four views; the case set reaches every
    branch, by the statement's own tallies."""
    v, t, n, views = small_scene()
    assert len(t) == 34
    vcol = np.random.default_rng(5).uniform(0, 1, (len(v), 3)).astype(np.float32)
    total = dict.fromkeys(dr.BRANCHES, 0)
    for k, (size, block, filt, maps, shading, cull) in enumerate(CASES):
        uv, color, normal, _ = awkward_texture(size, block, 20 + k)
        color, normal = (color if maps != "normal" else None), (normal if maps != "color" else None)
        with ctx.upload_mesh(v, t, vcol, n) as m:
            for view in views:
                want = dr.draw(v, t, view, uv, color, normal, colors=vcol, normals=n, cull=cull, shading=shading, filter=filt)
                got = m.draw_textured(view, uv, color, normal, cull=cull, shading=shading, filter=filt, faces=True)
                dr.assert_equal_bits(got, want)
                assert got["peak_workspace"] >= 12 * view["width"] * view["height"] and got["ms"] > 0
                for key in total:
                    total[key] += want["tallies"][key]
    print("branches:", total)
    for key in total:
        assert total[key] > 0, key
    uv, color, _, _ = awkward_texture(32, 0, 1)
    e = ctx.draw_textured_mesh(v[:0], t[:0], views[0], uv[:0], color, faces=True)  # a mesh without triangles: an empty image
    assert not e["image"].any() and (e["faces"] == 0xFFFFFFFF).all() and e["n_tris"] == 0 and e["n_covered"] == 0 and e["n_bad_uv"] == 0


def test_the_fill_is_the_rasterisers(ctx):
    v, t, n, views = small_scene()
    uv, color, normal, _ = awkward_texture(64, 0, 2)
    with ctx.upload_mesh(v, t, None, n) as m:
        for cull, shading in (("none", "face"), ("back", "vertex"), ("front", "face")):
            for view in views:
                a = m.rasterize(view, cull=cull, shading=shading, faces=True)
                b = m.draw_textured(view, uv, color, normal, cull=cull, shading=shading, faces=True)
                assert np.array_equal(_bits(a["image"][..., 6:9]), _bits(b["image"][..., 6:9])) and np.array_equal(a["faces"], b["faces"])
                for key in a:
                    if key not in ("image", "faces", "ms", "peak_workspace"):
                        assert a[key] == b[key], key


def test_position_round_trip(ctx):
    """The baker's position map drawn as the colour map with the baker's uv: every covered pixel shows (m_a v_a + m_b v_b) + m_c v_c of the statement's weights within
    position_bound (tests/test_mesh_draw_cpu.py), computed from the inputs."""
    v, t, n, views = small_scene()
    worst = 0.0
    for size, block in ((64, 0), (67, 9)):
        baked = ctx.bake_texture(v, t, size, block, maps=("position",))
        bound = position_bound(v, t, size, baked["block"])
        for view in views:
            r = ctx.draw_textured_mesh(v, t, view, baked["uv"], baked["position"], faces=True)
            pix, want = dr.surface_points(v, t, view, r["faces"])
            assert len(pix) == r["n_covered"] and r["n_bad_uv"] == 0 and r["n_unowned_taps"] == 0
            if len(pix):
                err = np.abs(r["image"].reshape(-1, 9)[pix, 3:6].astype(np.float64) - want).max()
                worst = max(worst, err / bound)
                assert err <= bound, (size, block, err, bound)
    print("position round trip: worst error / bound = %.3f" % worst)


def test_constant_colour(ctx):
    """A colour map that is c on every texel of alpha 1 gives c within 1 ulp on every covered pixel whose unowned flag is clear in the statement: a made-up map, and the
    map project_views blends from constant opaque images (the same constant as the fallback of the texels no view reaches)."""
    v, t, n, views = small_scene()
    uv, color, _, _ = random_maps(67, 3, block=9)
    const = np.float32([0.3, 0.7123, 0.05])
    color[color[..., 3] == 1, :3] = const
    color[color[..., 3] == 0, :3] = 9.0
    eight = np.uint8([77, 200, 255, 255])
    target = (eight[:3].astype(np.float64) / 255.0).astype(np.float32)
    fallback = np.tile(np.append(target, np.float32(1.0)), (67, 67, 1)).astype(np.float32)
    proj = ctx.project_views(v, t, views, [np.tile(eight, (5, 7, 1))] * len(views), size=67, block=9, fallback=fallback)
    assert (proj["info"][..., 0] > 0).sum() > 500 and np.array_equal(_bits(proj["uv"]), _bits(uv))
    for name, cmap, c in (("made up", color, const), ("projected", proj["color"], target)):
        for filt in ("bilinear", "nearest"):
            for view in views:
                got = ctx.draw_textured_mesh(v, t, view, uv, cmap, filter=filt)
                want = dr.draw(v, t, view, uv, cmap, filter=filt)
                clean = (got["image"][..., 6] == 1) & ~want["unowned"]
                assert got["n_unowned_taps"] == want["n_unowned_taps"]
                if clean.any():
                    ulps = np.abs(_bits(got["image"][clean][:, 3:6]).astype(np.int64) - _bits(c).astype(np.int64))
                    assert ulps.max() <= 1, (name, filt, ulps.max())


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
    yield c, views, normals, albedos
    c.close()


def test_normal_map_from_the_model(trained):
    """Extract, simplify, bake albedo + normal, then mesh_view_metrics(texture=, albedo_maps=) on the fixture's views: finite numbers for every key, unit normals where
    covered and zeros elsewhere. The bare and the normal-mapped angles are printed, not compared: that is a measurement (profiles/mesh_draw.md)."""
    c, views, normals, albedos = trained
    with c.extract_mesh_device(64, cull="none", normals=True) as full:
        with full.simplify(*c.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 16)) as m:
            mesh = m.download()
            baked = m.bake_texture(512, maps=("albedo", "normal"))
            tris = mesh["indices"].reshape(-1, 3)
            assert 100 < len(tris) < 5000
            for view in views:
                r = m.draw_textured(view, baked["uv"], baked["albedo"], baked["normal"])
                covered = r["image"][..., 6] == 1
                length = np.linalg.norm(r["image"][..., :3].astype(np.float64), axis=2)
                assert covered.sum() > 1000 and (np.abs(length[covered] - 1.0) <= 2.0 ** -22).all() and not r["image"][~covered].any()
                assert r["n_bad_uv"] == 0
    texture = dict(uv=baked["uv"], color=baked["albedo"], normal=baked["normal"])
    bare = c.mesh_view_metrics(mesh["verts"], tris, views, normals)
    got = c.mesh_view_metrics(mesh["verts"], tris, views, normals, texture=texture, albedo_maps=albedos)
    keys = ("mean_angle_deg", "median_angle_deg", "mask_iou", "albedo_mae", "albedo_rmse", "albedo_psnr_db")
    assert sorted(got["mean"]) == sorted(keys) and len(got["views"]) == len(views)
    for e in got["views"] + [got["mean"]]:
        assert all(math.isfinite(e[k]) for k in keys), e
    assert all(e["pixels_compared"] > 1000 for e in got["views"])
    assert [e["mask_iou"] for e in got["views"]] == [e["mask_iou"] for e in bare["views"]]  # the fill is the rasteriser's
    print("mean angle: bare %.3f deg, normal-mapped %.3f deg; albedo psnr %.2f dB, mae %.4f" % (bare["mean"]["mean_angle_deg"], got["mean"]["mean_angle_deg"],
                                                                                                got["mean"]["albedo_psnr_db"], got["mean"]["albedo_mae"]))


def test_permutation(ctx):
    """The triangles and the rows of uv permuted alike: channels 6-8 unchanged; colours and normals unchanged at every pixel where the statement finds a single triangle
    at the winner's float depth."""
    v, t, n, views = small_scene()
    uv, color, normal, _ = awkward_texture(64, 0, 4)
    perm = np.random.default_rng(6).permutation(len(t))
    for view in views:
        a = ctx.draw_textured_mesh(v, t, view, uv, color, normal, normals=n, shading="vertex")
        b = ctx.draw_textured_mesh(v, t[perm], view, uv[perm], color, normal, normals=n, shading="vertex")
        assert np.array_equal(_bits(a["image"][..., 6:9]), _bits(b["image"][..., 6:9]))
        single = dr.draw(v, t, view, uv, color, normal, normals=n, shading="vertex")["ties"] == 1
        assert np.array_equal(_bits(a["image"][single]), _bits(b["image"][single]))
        assert single.sum() > 0.9 * a["n_covered"] or a["n_covered"] == 0


def test_the_draw_leaves_training_untouched():
    """deterministic = 1: 50 steps, draws with both filters and map sets, 50 steps == 100 steps, bit for bit (the per-step statistics and the weights)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene(8, 96)
    verts, tris = tr.octahedron(2)
    uv, color, normal, _ = random_maps(128, 7, tris=len(tris))
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(100):
            if interrupt and s == 50:
                c.draw_textured_mesh(verts, tris, views[0], uv, color, normal)
                c.draw_textured_mesh(verts, tris, views[1], uv, None, normal, filter="nearest", faces=True)
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


def test_refusals(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi, api
    v, t, n, views = small_scene()
    uv, color, normal, _ = awkward_texture(64, 0, 8)
    good = ctx.draw_textured_mesh(v, t, views[3], uv, color, normal, faces=True)
    res = refusals(ctx.f, _abi, api, ctx._h)  # the list of the header, on a live context (nothing of it reaches the device)
    for label, rc, msg in res:
        assert rc == _abi.ERR_INVALID and msg, label
    bad = t.copy()
    bad[5, 1] = len(v)  # found by the range-check kernel, not by a fault
    with pytest.raises(rnb.RnbError) as err:
        ctx.draw_textured_mesh(v, bad, views[3], uv, color, normal)
    assert err.value.code == _abi.ERR_INVALID and "out of range" in str(err.value)
    again = ctx.draw_textured_mesh(v, t, views[3], uv, color, normal, faces=True)  # the context still works
    assert np.array_equal(_bits(again["image"]), _bits(good["image"])) and np.array_equal(again["faces"], good["faces"])
    dr.assert_equal_bits(again, dr.draw(v, t, views[3], uv, color, normal))


def test_build_mesh_reports_the_textured_views(tmp_path):
    """`build/mesh --simplify 16 --texture 256 --texture-maps albedo,normal --report-views` on a snapshot the testbed wrote: <out>.views.json carries the textured_* and
    albedo_* keys per view and in `mean`, and they are the numbers Context.mesh_view_metrics(texture=, albedo_maps=) gives for the same mesh and the same bake made
    through the Python interface on a context that holds the snapshot (the data the OBJ and its maps are written from, before save_obj's mapping and the 8- and 16-bit
    image files), to 1e-9 relative: both sides sum the same pixels in double, in row-major order. The existing keys are those of the run without --texture; and without
    --texture two runs write the same report byte for byte, timing fields apart."""
    from rnb_neus2_amd import synthetic
    from tests.test_gpu_mesh_simplify import _context_of
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--keep", "largest", "--orient", "outward", "--simplify", "16", "--report-views"]
    reports, lines = {}, {}
    for name, extra in (("plain", []), ("again", []), ("textured", ["--texture", "256", "--texture-maps", "albedo,normal"])):
        out = str(tmp_path / (name + ".obj"))
        r = subprocess.run(base + ["--out", out] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        with open(out + ".views.json") as f:
            reports[name] = f.read()
        lines[name] = r.stdout.splitlines()
    strip = lambda text: __import__("re").sub(r'"frame_ms": [^,}]+', '"frame_ms": 0', text)
    assert strip(reports["plain"]) == strip(reports["again"])
    assert not [l for l in lines["plain"] if "textured" in l] and "textured" not in reports["plain"] and "albedo" not in reports["plain"]
    assert len([l for l in lines["textured"] if l.startswith("  textured:")]) == 12 and len([l for l in lines["textured"] if l.startswith("views textured:")]) == 1
    print("\n".join(l for l in lines["textured"] if "views" in l))
    rep, plain = json.loads(reports["textured"]), json.loads(reports["plain"])
    new = ["textured_mean_angle_deg", "textured_median_angle_deg", "albedo_mae", "albedo_rmse", "albedo_psnr_db"]
    for e, p in zip(rep["views"] + [rep["mean"]], plain["views"] + [plain["mean"]]):
        assert sorted(e) == sorted(list(p) + new + ["textured_frame_ms"])
        assert all(e[k] == p[k] for k in p if k != "frame_ms")  # the bare geometry's numbers are what they were
    with _context_of(snap) as c:
        m = c.extract_mesh(res=128, colors=True, keep="largest", orient="outward", simplify=16, texture=256, texture_maps=("albedo", "normal"))
        tex = m["texture"]
        want = c.mesh_view_metrics(m["verts"], m["indices"], views, normals, texture=dict(uv=tex["uv"], color=tex["albedo"], normal=tex["normal"]), albedo_maps=albedos)
    assert rep["n_triangles"] == len(m["indices"]) // 3
    names = dict(textured_mean_angle_deg="mean_angle_deg", textured_median_angle_deg="median_angle_deg", albedo_mae="albedo_mae", albedo_rmse="albedo_rmse", albedo_psnr_db="albedo_psnr_db")
    for e, w in zip(rep["views"] + [rep["mean"]], want["views"] + [want["mean"]]):
        for key, other in names.items():
            if e[key] is None:  # what is not finite is written as null: a PSNR of equal images
                assert key == "albedo_psnr_db" and w[other] == math.inf, (key, w[other])
            else:
                assert math.isfinite(e[key]) and abs(e[key] - w[other]) <= 1e-9 * abs(w[other]), (key, e[key], w[other])
