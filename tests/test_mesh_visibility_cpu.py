"""CPU tier of the visibility stage (include/rnb_mesh_visibility.h): the C-ABI of the new header (exports, versions, defaults, struct layout, argument validation
without a device), the numpy statement of tests/mesh_visibility_reference.py on the scene the GPU tier uses and on its own properties, the calls the Python layer makes,
and the command lines. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_visibility_cases as mc
from tests import mesh_visibility_reference as vr
from tests.test_mesh_raster_cpu import axis_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_visibility.h")
NAMES = ["rnb_mesh_visibility", "rnb_mesh_visibility_abi_version", "rnb_mesh_visibility_default_options", "rnb_mesh_visibility_select", "rnb_mesh_visibility_select_default_options"]


def _parts(flags, part):
    return [int(np.asarray(flags)[part == k].astype(bool).sum()) for k in range(3)]


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_visibility_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"}) == NAMES
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in NAMES)
    assert set("rnb_" + k for k in _abi.MESH_VISIBILITY_PROTOTYPES) == set(NAMES)
    others = (_abi.PROTOTYPES, _abi.RENDER_PROTOTYPES, _abi.MESH_PROTOTYPES, _abi.MESH_CLEAN_PROTOTYPES, _abi.MESH_SIMPLIFY_PROTOTYPES, _abi.MESH_DISTANCE_PROTOTYPES,
              _abi.MESH_RASTER_PROTOTYPES, _abi.MESH_TEXTURE_PROTOTYPES)
    assert not set(_abi.MESH_VISIBILITY_PROTOTYPES) & set().union(*others)
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_raster_abi_version() == 1 and fns.mesh_clean_abi_version() == 1  # as they were
    assert fns.mesh_visibility_abi_version() == _abi.MESH_VISIBILITY_ABI_VERSION == 1
    o = _abi.MeshVisibilityOptions()
    o.cull, o.min_pixels, o.reserved[3] = 2, 9, 4
    assert fns.mesh_visibility_default_options(C.byref(o)) == 0
    assert (o.abi_version, o.near, o.cull, o.min_pixels, list(o.reserved)) == (1, 2.0 ** -10, _abi.MESH_RASTER_CULL_NONE, 1, [0] * 4)
    s = _abi.MeshVisibilitySelectOptions()
    s.unit, s.reserved[0] = 1, 3
    assert fns.mesh_visibility_select_default_options(C.byref(s)) == 0
    assert (s.abi_version, s.unit, s.min_views_seen, s.max_views_off_mask, s.rings, list(s.reserved)) == (1, _abi.MESH_VISIBILITY_UNIT_COMPONENT, 1, 0xFFFFFFFF, 1, [0] * 3)
    assert fns.mesh_visibility_default_options(None) == _abi.ERR_INVALID and fns.mesh_visibility_select_default_options(None) == _abi.ERR_INVALID
    for name in ("mesh_visibility", "cull_unseen_mesh"):
        assert hasattr(api.Context, name), name
    for name in ("visibility", "select_seen", "cull_unseen"):
        assert hasattr(api.DeviceMesh, name), name
    assert HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_visibility.cuh") in build.DEPS
    assert re.findall(r'#include\s+"([^"]+)"', open(HEADER).read()) == ["rnb_mesh.h"]
    for name in os.listdir(os.path.join(ROOT, "include")):  # no other header mentions this one
        assert name == "rnb_mesh_visibility.h" or "visibility" not in open(os.path.join(ROOT, "include", name)).read()


def test_the_fill_is_one_piece_of_code_with_two_callers():
    """rnb_mesh_raster and rnb_mesh_visibility both go through raster_fill; the fill kernels are launched nowhere else, and the new kernel file defines none of its own."""
    drv = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "driver_mesh.hpp")).read()
    assert len(re.findall(r"\braster_fill<(?:true|false)>\(", drv)) == 2 and "raster_fill<false>(\"rnb_mesh_raster\"" in drv and "raster_fill<true>(\"rnb_mesh_visibility\"" in drv
    assert len(re.findall(r"hipLaunchKernelGGL\(\(?k_mr_bin<", drv)) == 2 and len(re.findall(r"hipLaunchKernelGGL\(k_mr_fill_large<", drv)) == 1
    new = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_visibility.cuh")).read()
    assert "mr_edge" not in new and "mr_setup" not in new and "mr_cover" not in new and "atomicMin" not in new and "atomicCAS" not in new
    for k in ("k_cl_init", "k_cl_hook", "k_cl_flatten"):  # the cleaner's components, reused
        assert len(re.findall(r"hipLaunchKernelGGL\(%s," % k, drv)) == 2, k


def test_visibility_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = [("rnb_mesh_visibility_view", _abi.MeshVisibilityView), ("rnb_mesh_visibility_options", _abi.MeshVisibilityOptions), ("rnb_mesh_face_visibility", _abi.MeshFaceVisibility),
               ("rnb_mesh_visibility_stats", _abi.MeshVisibilityStats), ("rnb_mesh_visibility_select_options", _abi.MeshVisibilitySelectOptions),
               ("rnb_mesh_visibility_select_stats", _abi.MeshVisibilitySelectStats)]
    consts = ["ABI_VERSION", "NONE", "MAX_RINGS", "UNIT_COMPONENT", "UNIT_FACE"]
    body, want = "", []
    for cname, S in structs:
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % cname + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, n) for n, _ in S._fields_)
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    body += "".join("  printf(\"%%llu\\n\", (unsigned long long)RNB_MESH_VISIBILITY_%s);\n" % c for c in consts)
    body += "  printf(\"%llu\\n\", (unsigned long long)RNB_MESH_RASTER_NONE);\n"
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_raster.h\"\n#include \"rnb_mesh_visibility.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:len(want)] == want
    assert out[len(want):] == [getattr(_abi, "MESH_VISIBILITY_" + c) for c in consts] + [_abi.MESH_VISIBILITY_NONE]
    assert C.sizeof(_abi.MeshFaceVisibility) == 40 == vr.RECORD.itemsize == np.dtype(_abi.MESH_FACE_VISIBILITY_DTYPE).itemsize
    assert np.dtype(_abi.MESH_FACE_VISIBILITY_DTYPE) == vr.RECORD
    assert [(n, vr.RECORD.fields[n][1]) for n in vr.RECORD.names] == [(n, getattr(_abi.MeshFaceVisibility, n).offset) for n, _ in _abi.MeshFaceVisibility._fields_]
    assert (vr.NONE, vr.MAX_RINGS) == (_abi.MESH_VISIBILITY_NONE, _abi.MESH_VISIBILITY_MAX_RINGS)


def test_visibility_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the context or the device is touched: the context handed in is a block of zeros, and no device exists here."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good():
        o = _abi.MeshVisibilityOptions()
        assert fns.mesh_visibility_default_options(C.byref(o)) == 0
        return o

    def mesh(nv=3, ni=3):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, 0x1000, 0x2000  # never dereferenced
        return m

    def views(n=2, **kw):
        arr = (_abi.MeshVisibilityView * n)()
        for e in arr:
            e.view = api._view_struct(axis_view(8, 6, 10.0))
        if kw:
            arr[n - 1].view = api._view_struct(dict(axis_view(8, 6, 10.0), **kw))
        return arr

    def call(ctx_, m, arr, n, o, out=0x3000, stats=None):
        return fns.mesh_visibility(ctx_, None, m, arr, n, o, out, stats)

    M = mesh()
    assert call(None, C.byref(M), views(), 2, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, None, views(), 2, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), None, 2, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), views(), 2, None) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), views(), 2, C.byref(good()), out=None) == _abi.ERR_INVALID and b"null" in fns.last_error()
    assert call(ctx, C.byref(M), views(), 0, C.byref(good())) == _abi.ERR_INVALID and b"n_views" in fns.last_error()
    st = _abi.MeshVisibilityStats()
    for field, value in [("abi_version", 2), ("abi_version", 0), ("near", 0.0), ("near", -1.0), ("near", float("nan")), ("near", float("inf")), ("cull", 3), ("min_pixels", 0)]:
        o = good()
        setattr(o, field, value)
        st.n_tris = 7
        assert call(ctx, C.byref(M), views(), 2, C.byref(o), stats=C.byref(st)) == _abi.ERR_INVALID, (field, value)
        assert st.n_tris == 0 and fns.last_error()
    o = good()
    o.reserved[0] = 1
    assert call(ctx, C.byref(M), views(), 2, C.byref(o)) == _abi.ERR_INVALID
    for kw in (dict(focal_length=(0.0, 10.0)), dict(focal_length=(10.0, float("inf"))), dict(principal_point=(float("nan"), 0.5)), dict(width=0), dict(height=0), dict(width=16385)):
        assert call(ctx, C.byref(M), views(**kw), 2, C.byref(good())) == _abi.ERR_INVALID, kw  # the bad view is the last one
    arr = views()
    arr[1].mask_dev, arr[1].mask_width, arr[1].mask_height = 0x4000, 0, 5
    assert call(ctx, C.byref(M), arr, 2, C.byref(good())) == _abi.ERR_INVALID and b"mask" in fns.last_error()
    arr[1].mask_width, arr[1].mask_height = 5, 0
    assert call(ctx, C.byref(M), arr, 2, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(mesh(3, 4)), views(), 2, C.byref(good())) == _abi.ERR_INVALID and b"multiple of 3" in fns.last_error()
    assert call(ctx, C.byref(mesh(0, 3)), views(), 2, C.byref(good())) == _abi.ERR_INVALID and b"no vertices" in fns.last_error()

    # the selection
    def sgood():
        o = _abi.MeshVisibilitySelectOptions()
        assert fns.mesh_visibility_select_default_options(C.byref(o)) == 0
        return o

    out = _abi.Mesh()

    def sel(ctx_, m, recs, o, dst):
        if dst is not None:
            out.verts, out.n_indices = 0x5000, 3
        return fns.mesh_visibility_select(ctx_, None, m, recs, o, dst, None, None)

    assert sel(None, C.byref(M), 0x3000, C.byref(sgood()), C.byref(out)) == _abi.ERR_INVALID
    assert sel(ctx, None, 0x3000, C.byref(sgood()), C.byref(out)) == _abi.ERR_INVALID
    assert sel(ctx, C.byref(M), 0x3000, None, C.byref(out)) == _abi.ERR_INVALID
    assert sel(ctx, C.byref(M), 0x3000, C.byref(sgood()), None) == _abi.ERR_INVALID
    assert sel(ctx, C.byref(M), 0x3000, C.byref(sgood()), C.byref(M)) == _abi.ERR_INVALID and b"different" in fns.last_error() and M.n_indices == 3
    for field, value in [("abi_version", 2), ("unit", 2), ("rings", 65)]:
        o = sgood()
        setattr(o, field, value)
        assert sel(ctx, C.byref(M), 0x3000, C.byref(o), C.byref(out)) == _abi.ERR_INVALID and not out.verts and out.n_indices == 0, field  # *out zeroed
    o = sgood()
    o.reserved[2] = 1
    assert sel(ctx, C.byref(M), 0x3000, C.byref(o), C.byref(out)) == _abi.ERR_INVALID
    assert sel(ctx, C.byref(M), None, C.byref(sgood()), C.byref(out)) == _abi.ERR_INVALID and b"faces_dev" in fns.last_error() and not out.verts
    assert sel(ctx, C.byref(mesh(3, 5)), 0x3000, C.byref(sgood()), C.byref(out)) == _abi.ERR_INVALID and b"multiple of 3" in fns.last_error()
    assert fake.raw == b"\0" * 4096


# ------------------------------------------------------------------------------------------------------------------------ the statement on the scene
def test_the_scene_in_six_views():
    """96 x 72, f = 110, no masks: what the GPU tier asserts on the device."""
    v, i, part = mc.scene()
    rec, st = mc.reference(96, 72, 110.0)
    assert _parts(rec["n_seen"] >= 1, part) == [2983, 0, 118]  # a closed outward mesh seen from outside never shows its cavity
    assert st["n_faces_seen"] == 3101 and st["n_faces_off_mask"] == 0 and st["n_pixels"] == 6 * 96 * 72
    assert sum(st[c] for c in vr.CLASSES) == 6 * 4992
    assert not rec["n_pixels_won"][part == 1].any() and rec["n_pixels_covered"][part == 1].any()  # covered, behind the outer surface
    assert (rec["best_view"] == vr.NONE).sum() == 4992 - 3101 and not rec["best_pixels"][rec["best_view"] == vr.NONE].any() and (rec["best_view"][rec["n_seen"] >= 1] < 6).all()
    assert np.all(rec["n_seen"] <= rec["n_drawn"]) and np.all(rec["n_pixels_won"] <= rec["n_pixels_covered"]) and np.all(rec["best_pixels"] <= rec["n_pixels_won"])
    kept, s = vr.select(len(v), i, rec)
    assert np.array_equal(kept != 0, part != 1) and (s["n_components"], s["n_components_kept"], s["n_seeds"], s["n_candidates"]) == (3, 2, 3101, 4992)
    out = vr.compact(v, i, kept)
    assert len(out["indices"]) // 3 == mc.N_OUTER + mc.N_FLOATER and np.array_equal(out["verts"][out["indices"]], v[i.reshape(-1, 3)[kept != 0].ravel()])
    assert _parts(vr.select(len(v), i, rec, "face", rings=1)[0], part) == [mc.N_OUTER, 0, 174]
    assert _parts(vr.select(len(v), i, rec, "face", rings=2)[0], part) == [mc.N_OUTER, 0, mc.N_FLOATER]
    assert np.array_equal(vr.select(len(v), i, rec, "face", rings=0)[0] != 0, rec["n_seen"] >= 1)
    assert 500 * 6 < mc.reference(192, 144, 220.0)[1]["n_large"] < 900 * 6


def test_the_scene_with_masks():
    v, i, part = mc.scene()
    rec, st = mc.reference(96, 72, 110.0, masks=(96, 72, 110.0))
    assert _parts(rec["n_seen"] >= 1, part) == [2983, 0, 0]
    assert _parts(rec["n_off_mask"] >= 1, part) == [0, 0, 150] and int((rec["n_pixels_covered"][part == 2] > 0).sum()) == 150 and st["n_faces_off_mask"] == 150
    assert np.array_equal(vr.select(len(v), i, rec)[0] != 0, part == 0)
    half, _ = mc.reference(96, 72, 110.0, masks=(48, 36, 55.0))
    assert (half["n_off_mask"][part == 0] == 1).any() and not half["n_off_mask"][part == 1].any()
    k0, k1 = (vr.select(len(v), i, half, max_views_off_mask=m)[0] for m in (0, 1))
    assert k0.sum() < k1.sum() and not k1[part == 1].any() and np.all(k0 <= k1)  # a looser limit keeps more, and never the cavity


def test_permuting_the_views_permutes_best_view_only():
    v, i, _ = mc.scene()
    views, masks = mc.views(96, 72, 110.0), mc.ball_masks(48, 36, 55.0)
    base, sb = mc.reference(96, 72, 110.0, masks=(48, 36, 55.0))
    q = [3, 0, 5, 1, 4, 2]
    rec, sq = vr.measure(v, i, [views[k] for k in q], [masks[k] for k in q])
    assert sq == sb
    for name in vr.RECORD.names:
        if name != "best_view":
            assert np.array_equal(rec[name], base[name]), name
    assert np.array_equal(rec["best_view"] == vr.NONE, base["best_view"] == vr.NONE) and (rec["best_view"] != base["best_view"]).any()


def test_the_mask_lookup_rule():
    m = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(vr.on_mask(m, 4, 3), m != 0)  # the same resolution: the pixel itself
    on = vr.on_mask(np.uint8([[0, 1]]), 5, 2)  # 5 pixels over 2: centres 0.5 .. 4.5 scaled by 2 / 5 -> 0 0 1 1 1
    assert on.tolist() == [[False, False, True, True, True]] * 2
    assert vr.on_mask(None, 3, 2).all()
    big = np.zeros((8, 8), np.uint8)
    big[4:, :] = 1
    assert vr.on_mask(big, 2, 2).tolist() == [[False, False], [True, True]]  # (2 j + 1) * 8 // 4 = 2, 6


# ------------------------------------------------------------------------------------------------------------------------ the Python layer
def test_extract_mesh_makes_the_calls_it_made_unless_seen_by_is_given(monkeypatch):
    from tests import test_device_mesh_cpu as dm
    c, fake = dm.context()
    dm.CALLS["extract_mesh"](c)
    assert fake.device_log() == dm.RECORDED["extract_mesh"]
    c, fake = dm.context()
    c.extract_mesh(16, keep="largest", simplify=8, error=True, colors=True, seen_by=None, seen_masks=None)
    assert fake.device_log() == dm.RECORDED["extract_mesh"] and not [e for e in fake.log if "visibility" in e[0]]
    with pytest.raises(ValueError):
        c.extract_mesh(16, seen_masks=[None])
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_visibility", ((2,), None))
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_visibility_select", ((2,), 5))
    c, fake = dm.context()
    out = c.extract_mesh(16, keep="largest", simplify=8, colors=True, seen_by=[dm.VIEW, dm.VIEW], seen_masks=[np.ones((2, 3), np.uint8), None])
    names = [e[0] for e in fake.log if e[0] in dm.STAGES or "visibility" in e[0]]
    assert names == ["extract_mesh", "mesh_clean", "mesh_visibility_default_options", "mesh_visibility_select_default_options", "mesh_visibility",
                     "mesh_visibility_select_default_options", "mesh_visibility_select", "mesh_simplify"] or \
        [n for n in names if not n.endswith("default_options")] == ["extract_mesh", "mesh_clean", "mesh_visibility", "mesh_visibility_select", "mesh_simplify"]
    log = {e[0]: e[1] for e in fake.log}
    assert log["mesh_visibility"] == (log["mesh_clean"][1],) and log["mesh_visibility_select"][0] == log["mesh_clean"][1] and log["mesh_simplify"][0] == log["mesh_visibility_select"][1]
    assert "seen_stats" in out and "visibility_stats" in out and "kept" not in out["seen_stats"]
    assert not fake.buffers and not fake.meshes and not fake.errors
    for stage in ("mesh_visibility", "mesh_visibility_select"):  # a failing stage leaves nothing allocated
        c, fake = dm.context(fail=stage)
        with pytest.raises(api_error()):
            c.extract_mesh(16, keep="largest", seen_by=[dm.VIEW], seen_masks=[np.ones((2, 3), np.uint8)])
        assert not fake.buffers and not fake.meshes and not fake.errors, stage
        c, fake = dm.context(fail=stage)
        with pytest.raises(api_error()):
            c.cull_unseen_mesh(dm.V, dm.I, [dm.VIEW, dm.VIEW], colors=dm.COL)
        assert not fake.buffers and not fake.meshes and not fake.errors, stage


def api_error():
    from rnb_neus2_amd import api
    return api.RnbError


def test_the_python_arguments_are_checked_before_anything_is_uploaded():
    from tests import test_device_mesh_cpu as dm
    c, fake = dm.context()
    bad = [dict(views=[]), dict(views=[dm.VIEW], masks=[None, None]), dict(views=[dm.VIEW], masks=[np.ones(4, np.uint8)]), dict(views=[dm.VIEW], supersample=0),
           dict(views=[dm.VIEW], supersample=1.5), dict(views=[dict(dm.VIEW, width=9000)], supersample=2), dict(views=[dm.VIEW], cull="both"), dict(views=[dm.VIEW], min_pixels=0)]
    with c.upload_mesh(dm.V, dm.I) as m:
        n = len(fake.device_log())
        for kw in bad:
            with pytest.raises(ValueError):
                m.visibility(**kw)
        for kw in (dict(unit="edge"), dict(rings=65), dict(rings=-1), dict(min_views=-1)):
            with pytest.raises(ValueError):
                m.cull_unseen([dm.VIEW], **kw)
        assert len(fake.device_log()) == n
    m.free()
    with pytest.raises(ValueError):
        m.visibility([dm.VIEW])
    with pytest.raises(ValueError):
        m.cull_unseen([dm.VIEW])
    assert not fake.buffers and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ the command lines
def test_build_mesh_lists_the_flags_and_refuses_their_misuse():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    text = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert text.returncode == 0
    for flag in ("--keep-seen=[MODE]", "--seen-min-views=[N]", "--seen-rings=[R]", "--seen-masks\n", "--seen-max-off=[N]", "--seen-supersample=[K]"):
        assert flag in text.stdout, flag
    need = ["--snapshot", "/nonexistent/s.msgpack", "--scene", "/nonexistent", "--out", "/nonexistent/o.obj"]
    for extra, word in ((["--seen-min-views", "2"], "--keep-seen"), (["--seen-rings", "2"], "--keep-seen"), (["--seen-masks"], "--keep-seen"), (["--seen-max-off", "1"], "--keep-seen"),
                        (["--seen-supersample", "2"], "--keep-seen"), (["--keep-seen", "edges"], "keep-seen"), (["--keep-seen", "component", "--seen-rings", "2"], "faces"),
                        (["--keep-seen", "faces", "--seen-rings", "65"], "seen-rings"), (["--keep-seen", "component", "--seen-max-off", "1"], "--seen-masks"),
                        (["--keep-seen", "component", "--seen-supersample", "0"], "seen-supersample"), (["--keep-seen", "component", "--seen-masks=1"], "seen-masks"),
                        (["--keep-seen"], "keep-seen")):
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)
        assert r.returncode == 255 and word in r.stderr.splitlines()[0], (extra, r.returncode, r.stderr[:200])
    for extra in (["--keep-seen", "component"], ["--keep-seen=faces", "--seen-rings", "0", "--seen-masks", "--seen-max-off", "0", "--seen-min-views", "2", "--seen-supersample", "2"]):
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)  # parsed: the next complaint is the missing snapshot
        assert r.returncode == 1 and "does not exist" in r.stderr, (extra, r.returncode, r.stderr[:200])


def test_the_pipeline_forwards_the_flags_and_leaves_the_argv_alone_without_them():
    import inspect
    import run_pipeline
    from rnb_neus2_amd import pipeline
    args = ("data", 1000, 256, "out/mesh.obj", "build/mesh")
    plain = pipeline.plan_device_postprocess(*args)
    assert plain == ["build/mesh", "--snapshot", pipeline.snapshot_candidates("data", 1000)[0], "--scene", "data", "--out", "out/mesh.obj", "--resolution", "256", "--keep", "largest",
                     "--orient", "outward"]
    assert pipeline.plan_device_postprocess(*args, keep_seen=None) == plain
    assert pipeline.plan_device_postprocess(*args, keep_seen="component") == plain + ["--keep-seen", "component"]
    full = dict(unit="faces", min_views=2, rings=3, masks=True, max_off=1, supersample=2)
    assert pipeline.plan_device_postprocess(*args, simplify=64, texture=512, keep_seen=full) == pipeline.plan_device_postprocess(*args, simplify=64, texture=512) + [
        "--keep-seen", "faces", "--seen-min-views", "2", "--seen-rings", "3", "--seen-masks", "--seen-max-off", "1", "--seen-supersample", "2"]
    for bad in ("edges", dict(unit="component", rings=1), dict(unit="faces", max_off=1), dict(unit="faces", foo=1), dict(min_views=1)):
        with pytest.raises(ValueError):
            pipeline.plan_device_postprocess(*args, keep_seen=bad)
    for fn in (pipeline.plan_device_postprocess, pipeline.run_device_postprocess, pipeline.run_full_pipeline):
        assert inspect.signature(fn).parameters["keep_seen"].default is None
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("i", "t", "o", keep_seen="component")
    base = ["--input", "i", "--testbed", "build/testbed", "--output", "o"]
    p = run_pipeline.build_parser()
    assert "keep_seen" not in run_pipeline.pipeline_kwargs(p.parse_args(base)) and "keep_seen" not in run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess"]))
    assert run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess"])) == dict(run_pipeline.pipeline_kwargs(p.parse_args(base)), device_postprocess=True, mesh_exe=None)
    assert run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess", "--keep-seen", "component"]))["keep_seen"] == dict(unit="component")
    kw = run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess", "--keep-seen", "faces", "--seen-min-views", "2", "--seen-rings", "3", "--seen-masks", "--seen-max-off", "1",
                                                           "--seen-supersample", "2"]))
    assert kw["keep_seen"] == full
    for bad in (["--keep-seen", "component"], ["--device-postprocess", "--seen-masks"], ["--device-postprocess", "--seen-rings", "1"], ["--device-postprocess", "--keep-seen", "edges"],
                ["--device-postprocess", "--keep-seen", "component", "--seen-rings", "1"], ["--device-postprocess", "--keep-seen", "faces", "--seen-max-off", "1"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(base + bad)


def test_the_bench_tool_holds_no_private_plumbing():
    """The rule tests/test_device_mesh_cpu.py applies to the other mesh tools: the public mesh interface and mesh_bench_common only."""
    with open(os.path.join(ROOT, "tools", "bench_mesh_visibility.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref", "_abi"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".visibility(" in text and ".cull_unseen(" in text and "rasterize(view, faces=True" in text
