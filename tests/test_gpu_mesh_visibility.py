"""The visibility stage (include/rnb_mesh_visibility.h: DeviceMesh.visibility, select_seen, cull_unseen and the Context forms) on the MI355X against the numpy statement
of tests/mesh_visibility_reference.py. Everything is integers: every record, every flag and every count is compared with np.array_equal, the culled meshes bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_visibility_cases as mc
from tests import mesh_visibility_reference as vr
from tests.test_mesh_raster_cpu import axis_view, fibonacci_view

pytestmark = pytest.mark.gpu

KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
COUNTS = ("n_tris", "n_views", "n_pixels", "n_faces_seen", "n_faces_off_mask") + vr.CLASSES


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def _same_records(got, want):
    assert got.dtype == vr.RECORD and got.shape == want.shape
    for name in vr.RECORD.names:
        assert np.array_equal(got[name], want[name]), (name, np.nonzero(got[name] != want[name])[0][:8])


def _measure(c, v, i, views, want, masks=None, **kw):
    """mesh_visibility against (records, stats) of the statement."""
    rec, st = c.mesh_visibility(v, i, views, masks, **kw)
    _same_records(rec, want[0])
    for key in COUNTS:
        assert st[key] == want[1][key], (key, st[key], want[1][key])
    assert st["peak_workspace"] >= 12 * max(x["width"] * x["height"] for x in views) + 12 * (len(i) // 3) and st["ms"] > 0
    return rec, st


def _cull(c, v, i, views, rec, masks=None, colors=None, min_pixels=1, **sel):
    """cull_unseen_mesh against select + compact of the statement on the records `rec`."""
    api_kw = dict(unit=sel.get("unit", "component"), rings=sel.get("rings", 1), min_views=sel.get("min_views_seen", 1),
                  max_off_mask=None if sel.get("max_views_off_mask", 0xFFFFFFFF) == 0xFFFFFFFF else sel["max_views_off_mask"])
    got = c.cull_unseen_mesh(v, i, views, masks, colors=colors, min_pixels=min_pixels, **api_kw)
    kept, st = vr.select(len(v), i, rec, **sel)
    want = vr.compact(v, i, kept, colors)
    assert np.array_equal(got["kept"], kept)
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    for key, val in st.items():
        assert got["stats"][key] == val, (key, got["stats"][key], val)
    s = got["stats"]
    assert (s["n_verts_in"], s["n_tris_in"], s["n_verts_out"], s["n_tris_out"]) == (len(v), len(i) // 3, len(want["verts"]), int(kept.sum())) and s["ms"] > 0
    return got, kept


def _parts(flags, part):
    return [int(np.asarray(flags)[part == k].astype(bool).sum()) for k in range(3)]


# ------------------------------------------------------------------------------------------------------------------------ the scene, without masks
def test_six_views_without_masks(ctx):
    """96 x 72, f = 110: the numbers the statement gives on the CPU tier, on the device."""
    v, i, part = mc.scene()
    views, want = mc.views(96, 72, 110.0), mc.reference(96, 72, 110.0)
    rec, st = _measure(ctx, v, i, views, want)
    assert _parts(rec["n_seen"] >= 1, part) == [2983, 0, 118] and st["n_faces_seen"] == 3101
    col = np.random.default_rng(5).uniform(0, 1, v.shape).astype(np.float32)
    got, kept = _cull(ctx, v, i, views, rec, colors=col)
    assert _parts(kept, part) == [mc.N_OUTER, 0, mc.N_FLOATER] and np.array_equal(kept != 0, part != 1)
    assert (got["stats"]["n_components"], got["stats"]["n_components_kept"]) == (3, 2)
    _, kept = _cull(ctx, v, i, views, rec, unit="face", rings=1)
    assert _parts(kept, part) == [mc.N_OUTER, 0, 174]
    _, kept = _cull(ctx, v, i, views, rec, unit="face", rings=2)
    assert _parts(kept, part) == [mc.N_OUTER, 0, mc.N_FLOATER]
    _, kept = _cull(ctx, v, i, views, rec, unit="face", rings=0)
    assert np.array_equal(kept != 0, rec["n_seen"] >= 1)
    _cull(ctx, v, i, views, rec, min_views_seen=3)
    _cull(ctx, v, i, views, rec, unit="face", min_views_seen=2, rings=3)


@pytest.mark.parametrize("size", [(192, 144, 220.0), (67, 45, 77.0)], ids=lambda s: "%dx%d" % s[:2])
def test_both_fill_paths_and_an_odd_size(ctx, size):
    """192 x 144: 500-900 large triangles per view, filled by a wavefront each, the rest by their threads. 67 x 45: no multiple of anything. Both on a triangle count that
    is no multiple of 64 (the last five dropped)."""
    v, i, part = mc.scene()
    i = i[:-15]
    views, want = mc.views(*size), mc.reference(*size, drop=5)
    if size[0] == 192:
        assert 3000 < want[1]["n_large"] < 5400 and want[1]["n_small"] > 20000
    rec, _ = _measure(ctx, v, i, views, want)
    assert not (rec["n_seen"][part[:-5] == 1]).any()
    _, kept = _cull(ctx, v, i, views, rec)
    assert not kept[part[:-5] == 1].any()
    _cull(ctx, v, i, views, rec, unit="face")


# ------------------------------------------------------------------------------------------------------------------------ masks
def test_masks_at_the_views_resolution(ctx):
    """The masks are the coverage of the ball without the floater: the floater is seen nowhere on the mask and lies off it wherever it covers a pixel centre."""
    v, i, part = mc.scene()
    views, masks, want = mc.views(96, 72, 110.0), mc.ball_masks(96, 72, 110.0), mc.reference(96, 72, 110.0, masks=(96, 72, 110.0))
    rec, st = _measure(ctx, v, i, views, want, masks)
    assert _parts(rec["n_seen"] >= 1, part) == [2983, 0, 0]
    assert _parts(rec["n_off_mask"] >= 1, part) == [0, 0, 150] and int((rec["n_pixels_covered"][part == 2] > 0).sum()) == 150 and st["n_faces_off_mask"] == 150
    _, kept = _cull(ctx, v, i, views, rec, masks)
    assert np.array_equal(kept != 0, part == 0)
    _cull(ctx, v, i, views, rec, masks, max_views_off_mask=0)
    _cull(ctx, v, i, views, rec, masks, unit="face", max_views_off_mask=0, rings=2)
    mixed = [masks[0], None, masks[2], None, None, masks[5]]  # views with and without a mask in one call
    _measure(ctx, v, i, views, vr.measure(v, i, views, mixed), mixed)


def test_masks_of_half_the_resolution(ctx):
    """48 x 36 masks under 96 x 72 views: the lookup rule. Silhouette faces of the ball now lie off the mask in a view or two."""
    v, i, part = mc.scene()
    views, masks, want = mc.views(96, 72, 110.0), mc.ball_masks(48, 36, 55.0), mc.reference(96, 72, 110.0, masks=(48, 36, 55.0))
    rec, _ = _measure(ctx, v, i, views, want, masks)
    assert (rec["n_off_mask"][part == 0] == 1).any()
    for limit in (0, 1):
        _cull(ctx, v, i, views, rec, masks, max_views_off_mask=limit)
        _cull(ctx, v, i, views, rec, masks, unit="face", max_views_off_mask=limit)
    odd = [np.ascontiguousarray(m[:35, :47]) for m in masks]  # a size that divides nothing
    _measure(ctx, v, i, views, vr.measure(v, i, views, odd), odd)


# ------------------------------------------------------------------------------------------------------------------------ the header's consequences
def test_permuted_triangles_and_permuted_views(ctx):
    v, i, part = mc.scene()
    views, masks = mc.views(96, 72, 110.0), mc.ball_masks(48, 36, 55.0)
    base, _ = mc.reference(96, 72, 110.0, masks=(48, 36, 55.0))
    rng = np.random.default_rng(11)
    p = rng.permutation(len(i) // 3)
    ip = i.reshape(-1, 3)[p].ravel()
    rec, _ = _measure(ctx, v, ip, views, vr.measure(v, ip, views, masks), masks)
    for name in ("n_drawn", "n_pixels_covered", "n_off_mask"):  # never changed by the order of the triangles
        assert np.array_equal(rec[name], base[name][p]), name
    assert rec["n_pixels_won"].sum() == base["n_pixels_won"].sum()  # a pixel changes hands between triangles of equal float depth, it is not lost
    _cull(ctx, v, ip, views, rec, masks, max_views_off_mask=1)
    q = [3, 0, 5, 1, 4, 2]
    vq, mq = [views[k] for k in q], [masks[k] for k in q]
    rec, _ = _measure(ctx, v, i, vq, vr.measure(v, i, vq, mq), mq)
    for name in vr.RECORD.names:
        if name != "best_view":
            assert np.array_equal(rec[name], base[name]), name
    won = rec["best_view"] != vr.NONE
    assert np.array_equal(won, base["best_view"] != vr.NONE)
    per_view = np.stack([vr.view_counts(v, i, views[k], masks[k])["won"] for k in range(6)])  # [view, triangle]
    t = np.nonzero(won)[0]
    assert np.array_equal(per_view[np.array(q)[rec["best_view"][t]], t], per_view[base["best_view"][t], t])  # the view named wins as many pixels as the one named before


def test_supersample_equals_hand_scaled_views(ctx):
    from rnb_neus2_amd import api
    v, i, _ = mc.scene()
    views, masks = mc.views(96, 72, 110.0), mc.ball_masks(96, 72, 110.0)
    scaled = [api.scaled_view(x, 2) for x in views]
    assert (scaled[0]["width"], scaled[0]["height"]) == (192, 144)
    a, sa = ctx.mesh_visibility(v, i, views, masks, supersample=2)
    _same_records(a, vr.measure(v, i, scaled, masks)[0])
    b, sb = ctx.mesh_visibility(v, i, scaled, masks)
    assert a.tobytes() == b.tobytes() and all(sa[k] == sb[k] for k in COUNTS) and sa["n_pixels"] == 6 * 192 * 144
    with pytest.raises(ValueError):
        ctx.mesh_visibility(v, i, views, supersample=171)  # 96 * 171 > 16384
    with pytest.raises(ValueError):
        ctx.mesh_visibility(v, i, views, supersample=0)


def test_min_pixels_three(ctx):
    v, i, part = mc.scene()
    views, want = mc.views(96, 72, 110.0), mc.reference(96, 72, 110.0, min_pixels=3)
    rec, st = _measure(ctx, v, i, views, want, min_pixels=3)
    assert 0 < st["n_faces_seen"] < 3101
    _cull(ctx, v, i, views, rec, unit="face", min_pixels=3)


# ------------------------------------------------------------------------------------------------------------------------ single triangles, camera positions
def test_single_triangles_and_camera_positions(ctx):
    view = axis_view(64, 64, 32.0)
    big = np.float32([[-30, -10, 2], [30, -10, 2], [0, 40, 2]])  # covers the whole 64 x 64 screen
    tri = np.uint32([0, 1, 2])
    rec, st = _measure(ctx, big, tri, [view], vr.measure(big, tri, [view]))
    assert (rec["n_pixels_won"][0], rec["n_pixels_covered"][0], rec["best_view"][0], rec["best_pixels"][0], rec["n_seen"][0], rec["n_drawn"][0]) == (4096, 4096, 0, 4096, 1, 1)
    assert st["n_large"] == 1
    behind = big * np.float32([1, 1, -1])
    rec, st = _measure(ctx, behind, tri, [view, view], vr.measure(behind, tri, [view, view]))
    assert (rec["n_drawn"][0], rec["n_seen"][0], rec["best_view"][0], st["n_behind"]) == (0, 0, vr.NONE, 2)
    two = np.concatenate([big, big + np.float32([0, 0, 1])])  # a second triangle behind the first: covered, never the winner
    idx = np.uint32([3, 4, 5, 0, 1, 2])
    rec, _ = _measure(ctx, two, idx, [view], vr.measure(two, idx, [view]))
    assert rec["n_pixels_won"].tolist() == [0, 4096] and rec["n_pixels_covered"][0] > 1000 and rec["n_drawn"].tolist() == [1, 1]
    half = np.zeros((2, 2), np.uint8)
    half[:, 0] = 1  # the left half of the screen is on the mask
    rec, _ = _measure(ctx, big, tri, [view], vr.measure(big, tri, [view], [half]), [half])
    assert (rec["n_pixels_won"][0], rec["n_pixels_covered"][0], rec["n_off_mask"][0]) == (2048, 4096, 0)  # exactly half is on: 2 * on < cov is false
    # a camera inside the cavity sees the cavity, and nothing of the outer surface
    v, i, part = mc.scene()
    from rnb_neus2_amd import synthetic
    inside = dict(width=80, height=60, focal_length=(40.0, 40.0), principal_point=(0.5, 0.5),
                  xform=synthetic.look_at_c2w(np.array(mc.BALL), np.array(mc.BALL) + np.array([0.3, 0.2, 0.1])).astype(np.float32))
    rec, _ = _measure(ctx, v, i, [inside], vr.measure(v, i, [inside]))
    assert _parts(rec["n_seen"], part)[1] > 50 and _parts(rec["n_seen"], part)[0] == 0 and _parts(rec["n_seen"], part)[2] == 0


# ------------------------------------------------------------------------------------------------------------------------ refusals
def test_invalid_arguments(ctx):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi, api
    v, i, part = mc.scene()
    views = mc.views(96, 72, 110.0)
    want = mc.reference(96, 72, 110.0)
    f, h = ctx.f, ctx._h
    rec_size = vr.RECORD.itemsize
    with ctx.upload_mesh(v, i) as m:
        faces = ctx.device_malloc(m.n_triangles * rec_size)
        mask = ctx.upload(np.ones((4, 4), np.uint8))
        try:
            def vis(mesh=m, n=6, opt=None, out=faces, arr=None, stats=None):
                arr = ctx._visibility_views(views, None, 1) if arr is None else arr
                opt = ctx._visibility_options(2.0 ** -10, "none", 1) if opt is None else opt
                return f.mesh_visibility(h, None, C.byref(mesh) if mesh is not None else None, arr, n, C.byref(opt), out, stats)

            def opt_with(**kw):
                o = ctx._visibility_options(2.0 ** -10, "none", 1)
                for k, val in kw.items():
                    setattr(o, k, val)
                return o

            st = _abi.MeshVisibilityStats()
            st.n_tris = 9
            assert vis(n=0, stats=C.byref(st)) == _abi.ERR_INVALID and b"n_views" in f.last_error() and st.n_tris == 0
            assert vis(out=None) == _abi.ERR_INVALID and b"null" in f.last_error()
            assert vis(mesh=None) == _abi.ERR_INVALID
            assert f.mesh_visibility(h, None, C.byref(m), None, 6, C.byref(opt_with()), faces, None) == _abi.ERR_INVALID
            for kw in (dict(abi_version=2), dict(near=0.0), dict(near=float("nan")), dict(cull=3), dict(min_pixels=0)):
                assert vis(opt=opt_with(**kw)) == _abi.ERR_INVALID, kw
            o = opt_with()
            o.reserved[1] = 1
            assert vis(opt=o) == _abi.ERR_INVALID and b"reserved" in f.last_error()
            arr = ctx._visibility_views(views, None, 1)
            arr[4].mask_dev, arr[4].mask_width, arr[4].mask_height = mask, 4, 0
            assert vis(arr=arr) == _abi.ERR_INVALID and b"mask" in f.last_error()
            arr[4].mask_width, arr[4].mask_height = 0, 4
            assert vis(arr=arr) == _abi.ERR_INVALID
            for kw in (dict(width=0), dict(height=16385), dict(focal_length=(0.0, 1.0)), dict(principal_point=(float("inf"), 0.5))):
                arr = ctx._visibility_views(views, None, 1)
                arr[2].view = api._view_struct(dict(views[2], **kw))
                assert vis(arr=arr) == _abi.ERR_INVALID, kw
            # the selection
            _, _ = ctx.mesh_visibility(v, i, views)
            ctx._check(vis())
            out = _abi.Mesh()

            def sel(mesh=m, recs=faces, opt=None, dst=out):
                opt = ctx._visibility_select_options("component", 1, None, 1) if opt is None else opt
                dst.verts, dst.n_indices = 0x1000, 3  # what a failure must zero
                return f.mesh_visibility_select(h, None, C.byref(mesh), recs, C.byref(opt), C.byref(dst), None, None)

            def sel_with(**kw):
                o = ctx._visibility_select_options("component", 1, None, 1)
                for k, val in kw.items():
                    setattr(o, k, val)
                return o

            for kw in (dict(abi_version=0), dict(unit=2), dict(rings=65)):
                assert sel(opt=sel_with(**kw)) == _abi.ERR_INVALID and not out.verts and out.n_indices == 0, kw
            assert sel(recs=None) == _abi.ERR_INVALID and b"faces_dev" in f.last_error() and not out.verts
            assert f.mesh_visibility_select(h, None, C.byref(m), faces, C.byref(sel_with()), C.byref(m), None, None) == _abi.ERR_INVALID and b"different" in f.last_error()
            assert m.n_triangles == 4992  # (in == out: nothing was zeroed)
            bad = i.copy()
            bad[3000] = len(v)
            with ctx.upload_mesh(v, bad) as mb:
                assert vis(mesh=mb) == _abi.ERR_INVALID and b"out of range" in f.last_error()
                assert sel(mesh=mb) == _abi.ERR_INVALID and b"out of range" in f.last_error() and not out.verts and out.n_indices == 0
        finally:
            ctx.device_free(faces)
            ctx.device_free(mask)
    with pytest.raises(rnb.RnbError) as e:
        ctx.mesh_visibility(v, bad, views)
    assert e.value.code == _abi.ERR_INVALID
    with pytest.raises(ValueError):
        ctx.mesh_visibility(v, i, [])
    with pytest.raises(ValueError):
        ctx.cull_unseen_mesh(v, i, views, unit="edge")
    # an empty mesh: no record, an empty mesh out
    e0, e1 = np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
    rec, st = ctx.mesh_visibility(e0, e1, views)
    assert len(rec) == 0 and st["n_tris"] == 0 and st["n_views"] == 6 and st["n_faces_seen"] == 0
    got = ctx.cull_unseen_mesh(e0, e1, views)
    assert len(got["verts"]) == 0 and len(got["indices"]) == 0 and len(got["kept"]) == 0
    # vertices no triangle uses go, as in the cleaner
    got = ctx.cull_unseen_mesh(np.concatenate([np.float32([[9, 9, 9]]), v]), i + np.uint32(1), views)
    assert np.array_equal(got["indices"], vr.compact(v, i, part != 1)["indices"])
    _measure(ctx, v, i, views, want)  # the context stays usable


# ------------------------------------------------------------------------------------------------------------------------ reproducible, and beside training
def test_two_calls_give_the_same_bytes(ctx):
    v, i, _ = mc.scene()
    views, masks = mc.views(192, 144, 220.0), mc.ball_masks(48, 36, 55.0)
    a, sa = ctx.mesh_visibility(v, i, views, masks)
    b, sb = ctx.mesh_visibility(v, i, views, masks)
    assert a.tobytes() == b.tobytes() and all(sa[k] == sb[k] for k in COUNTS)
    ca, cb = (ctx.cull_unseen_mesh(v, i, views, masks, unit="face", max_off_mask=1) for _ in range(2))
    assert all(ca[k].tobytes() == cb[k].tobytes() for k in ("verts", "indices", "kept"))


def test_the_calls_leave_a_training_context_as_it_was():
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    v, i, _ = mc.scene()
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    names = ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID", "DENSITY_BITFIELD")
    with rnb.Context(deterministic=1, **KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(5):
            c.train_step()
        before = {k: c.get(k).tobytes() for k in names}
        step = c.training_step
        c.mesh_visibility(v, i, mc.views(96, 72, 110.0), mc.ball_masks(96, 72, 110.0))
        c.cull_unseen_mesh(v, i, mc.views(96, 72, 110.0))
        c.cull_unseen_mesh(v, i, mc.views(96, 72, 110.0), unit="face", rings=2)
        assert c.training_step == step
        for k in names:
            assert c.get(k).tobytes() == before[k], k
        c.train_step()


# ------------------------------------------------------------------------------------------------------------------------ build/mesh --keep-seen
def _obj_triangles(path):
    """The triangles of an OBJ as tuples of their corners' position strings, in file order."""
    pos, tris = [], []
    with open(path) as f:
        for line in f:
            w = line.split()
            if w and w[0] == "v":
                pos.append(tuple(w[1:4]))
            elif w and w[0] == "f":
                tris.append(tuple(pos[int(x.split("/")[0]) - 1] for x in w[1:4]))
    return tris


def test_build_mesh_keep_seen(tmp_path):
    """`build/mesh --orient outward --keep-seen component [--seen-masks]` on the small model of test_build_mesh_reports_the_views: the triangles written are a subset of
    those written without the flag, in the same order; the report lines are there, and their counts are those of Context.cull_unseen_mesh on the same mesh."""
    import os
    import re
    import subprocess
    from rnb_neus2_amd import synthetic
    from tests.test_gpu_mesh_simplify import _context_of
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(root, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(root, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--orient", "outward"]
    plain = str(tmp_path / "plain.obj")
    r = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "seen: " not in r.stdout and "keep-seen " not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
    all_tris = _obj_triangles(plain)
    with _context_of(snap) as c:
        m = c.extract_mesh(res=128, colors=True, orient="outward")
        assert len(m["indices"]) // 3 == len(all_tris)
        masks = [n[..., 3] > 0 for n in normals]
        for name, extra, kw in (("component", [], {}), ("masked", ["--seen-masks", "--seen-max-off", "3"], dict(masks=masks, max_off_mask=3))):
            out = str(tmp_path / (name + ".obj"))
            r = subprocess.run(base + ["--out", out, "--keep-seen", "component"] + extra, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
            print(r.stdout)
            want = c.cull_unseen_mesh(m["verts"], m["indices"], views, **kw)
            vs, ss = want["visibility_stats"], want["stats"]
            seen = re.search(r"^seen: (\d+) views, (\d+) pixels, (\d+) of (\d+) triangles seen, (\d+) off the mask", r.stdout, re.M)
            kept = re.search(r"^keep-seen component: (\d+) seeds, (\d+) candidates, (\d+) components of which (\d+) kept, (\d+) -> (\d+) triangles, (\d+) -> (\d+) vertices", r.stdout, re.M)
            assert seen and kept, r.stdout
            assert [int(x) for x in seen.groups()] == [12, 12 * 160 * 160, vs["n_faces_seen"], vs["n_tris"], vs["n_faces_off_mask"]]
            assert [int(x) for x in kept.groups()] == [ss["n_seeds"], ss["n_candidates"], ss["n_components"], ss["n_components_kept"], ss["n_tris_in"], ss["n_tris_out"], ss["n_verts_in"],
                                                       ss["n_verts_out"]]
            tris = _obj_triangles(out)
            assert len(tris) == ss["n_tris_out"] == int(want["kept"].sum()) and 0 < len(tris) <= len(all_tris)
            assert tris == [t for t, k in zip(all_tris, want["kept"]) if k]  # the kept triangles of the plain run, in its order
    r = subprocess.run(base + ["--out", plain, "--seen-masks"], capture_output=True, text=True)
    assert r.returncode == 255 and "--keep-seen" in r.stderr
