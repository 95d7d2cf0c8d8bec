"""CPU tier of the textured draw (include/rnb_mesh_draw.h): the C-ABI of the new header (exports, version, defaults, struct layout, argument validation without a device),
the numpy statement of tests/mesh_draw_reference.py on its own properties, view_albedo_metrics on known answers, the calls the Python layer makes on a recording stand-in
for the library, and mesh_view_metrics unchanged without the new keywords. No test here needs a GPU."""
import ctypes as C
import inspect
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_draw_reference as dr
from tests import mesh_raster_reference as mr
from tests import mesh_texture_reference as tr
from tests.test_mesh_project_cpu import front_view, quad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_draw.h")
KERNELS = os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_draw.cuh")
NAMES = ["rnb_mesh_draw_abi_version", "rnb_mesh_draw_default_options", "rnb_mesh_draw_textured"]


def _built():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    return api, _abi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_draw_header_is_exported_by_the_hip_library():
    api, _abi = _built()
    from rnb_neus2_amd import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"}) == NAMES
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in NAMES)
    assert set("rnb_" + k for k in _abi.MESH_DRAW_PROTOTYPES) == set(NAMES)
    others = (_abi.PROTOTYPES, _abi.RENDER_PROTOTYPES, _abi.MESH_PROTOTYPES, _abi.MESH_CLEAN_PROTOTYPES, _abi.MESH_SIMPLIFY_PROTOTYPES, _abi.MESH_DISTANCE_PROTOTYPES,
              _abi.MESH_RASTER_PROTOTYPES, _abi.MESH_TEXTURE_PROTOTYPES, _abi.MESH_VISIBILITY_PROTOTYPES, _abi.MESH_PROJECT_PROTOTYPES)
    assert not set(_abi.MESH_DRAW_PROTOTYPES) & set().union(*others)
    assert "mesh_draw" in inspect.signature(_abi.declare).parameters
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_raster_abi_version() == 1 and fns.mesh_texture_abi_version() == 1 and fns.mesh_project_abi_version() == 1  # as they were
    assert fns.mesh_draw_abi_version() == _abi.MESH_DRAW_ABI_VERSION == 1
    o = _abi.MeshDrawOptions()
    o.cull, o.normals, o.filter, o.reserved[1] = 2, 1, 0, 7
    assert fns.mesh_draw_default_options(C.byref(o)) == 0
    assert (o.abi_version, o.near, o.cull, o.normals, o.filter, list(o.reserved)) == (1, 2.0 ** -10, _abi.MESH_RASTER_CULL_NONE, _abi.MESH_RASTER_NORMALS_FACE,
                                                                                     _abi.MESH_DRAW_FILTER_BILINEAR, [0] * 4)
    assert fns.mesh_draw_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.DeviceMesh, "draw_textured") and hasattr(api.Context, "draw_textured_mesh") and hasattr(api, "view_albedo_metrics")
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and KERNELS in build.DEPS


def test_the_draw_shares_the_fill_and_the_winners_weights():
    """The new kernel file has no fill and no coverage arithmetic of its own: it calls the rasteriser's device functions; the driver launches the fill from the one place
    the rasteriser launches it from."""
    new = open(KERNELS).read()
    code = re.sub(r"//[^\n]*", "", new)
    for needle in ("mr_edge", "atomicMin", "atomicCAS", "k_mr_bin", "k_mr_fill_large"):
        assert needle not in code, needle
    for needle in ("mr_setup(", "mr_cover(", "mr_depth(", "fp contract(off)", "wave_sum("):
        assert needle in code, needle
    assert not re.search(r"__device__[^\n(]*\b(mr_\w+)\s*\(", code)  # called, not defined
    assert len(re.findall(r"__global__", code)) == 1 and "k_md_resolve" in code
    drv = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "driver_mesh.hpp")).read()
    body = drv.split("int rnb_mesh_draw_textured(")[1].split("RNB_GUARD")[0]
    assert "raster_image(" in body and "raster_fill" not in body and "hipLaunchKernelGGL" not in body


def test_draw_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = [("rnb_mesh_draw_texture", _abi.MeshDrawTexture), ("rnb_mesh_draw_options", _abi.MeshDrawOptions), ("rnb_mesh_draw_stats", _abi.MeshDrawStats)]
    consts = ["ABI_VERSION", "FILTER_NEAREST", "FILTER_BILINEAR"]
    body, want = "", []
    for cname, S in structs:
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % cname + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, n) for n, _ in S._fields_)
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    body += "  printf(\"%zu\\n\", sizeof(((rnb_mesh_draw_stats*)0)->raster));\n"
    body += "".join("  printf(\"%%llu\\n\", (unsigned long long)RNB_MESH_DRAW_%s);\n" % c for c in consts)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_raster.h\"\n#include \"rnb_mesh_draw.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:len(want)] == want
    assert out[len(want)] == C.sizeof(_abi.MeshRasterStats)
    assert out[len(want) + 1:] == [getattr(_abi, "MESH_DRAW_" + c) for c in consts]
    assert dr.FILTERS == dict(nearest=_abi.MESH_DRAW_FILTER_NEAREST, bilinear=_abi.MESH_DRAW_FILTER_BILINEAR) and dr.MAX_TEXTURE_SIZE == 8192
    st = _abi.MeshDrawStats()
    assert sorted(st.as_dict()) == sorted(list(_abi.MeshRasterStats().as_dict()) + ["n_bad_uv", "n_normal_fallback", "n_unowned_taps"])
    alone = tmp_path / "alone.c"  # without the rasteriser's header first the header says what it needs
    alone.write_text("#include \"rnb_mesh_draw.h\"\nint main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(alone), "-o", str(tmp_path / "alone")], capture_output=True, text=True)
    assert r.returncode != 0 and "rnb_mesh_raster" in r.stderr


def refusals(fns, _abi, api, ctx, ptrs=(0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000)):
    """Every call the header lists as refused before the device is touched, as (label, status, message): shared with the GPU tier, which hands in a live context."""
    p_verts, p_idx, p_normals, p_uv, p_color, p_normal, p_out = ptrs

    def good(**kw):
        o = _abi.MeshDrawOptions()
        assert fns.mesh_draw_default_options(C.byref(o)) == 0
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def mesh(nv=3, ni=3, normals=False):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, p_verts, p_idx
        if normals:
            m.normals = p_normals
        return m

    def texture(**kw):
        t = _abi.MeshDrawTexture()
        t.uv_dev, t.color_dev, t.normal_dev, t.size, t.n_tris = p_uv, p_color, p_normal, 16, 1
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def view(**kw):
        return api._view_struct(dict(front_view(), **kw))

    st = _abi.MeshDrawStats()

    def call(label, ctx_, m, t, v, o, out=p_out, faces=None):
        st.raster.n_tris, st.n_bad_uv = 7, 7
        rc = fns.mesh_draw_textured(ctx_, None, m, t, v, o, out, faces, C.byref(st))
        msg = fns.last_error()
        assert bytes(st) == bytes(C.sizeof(st)), label  # *stats zeroed
        return label, rc, msg

    M, T, V = mesh(), texture(), view()
    b = C.byref
    res = [call("null ctx", None, b(M), b(T), b(V), b(good())), call("null mesh", ctx, None, b(T), b(V), b(good())), call("null tex", ctx, b(M), None, b(V), b(good())),
           call("null view", ctx, b(M), b(T), None, b(good())), call("null opt", ctx, b(M), b(T), b(V), None), call("null out", ctx, b(M), b(T), b(V), b(good()), out=None),
           call("out == faces", ctx, b(M), b(T), b(V), b(good()), out=p_out, faces=p_out)]
    nan, inf = float("nan"), float("inf")
    for field, value in [("abi_version", 2), ("abi_version", 0), ("near", 0.0), ("near", -1.0), ("near", nan), ("near", inf), ("cull", 3), ("normals", 2), ("filter", 2),
                         ("filter", 0xFFFFFFFF)]:
        res.append(call("%s=%r" % (field, value), ctx, b(M), b(T), b(V), b(good(**{field: value}))))
    o = good()
    o.reserved[2] = 1
    res.append(call("reserved", ctx, b(M), b(T), b(V), b(o)))
    res.append(call("no map", ctx, b(M), b(texture(color_dev=None, normal_dev=None)), b(V), b(good())))
    res.append(call("misaligned map", ctx, b(M), b(texture(color_dev=p_color + 8)), b(V), b(good())))
    res.append(call("null uv", ctx, b(M), b(texture(uv_dev=None)), b(V), b(good())))
    for size in (0, 8193):
        res.append(call("size=%d" % size, ctx, b(M), b(texture(size=size)), b(V), b(good())))
    res.append(call("n_tris", ctx, b(M), b(texture(n_tris=2)), b(V), b(good())))
    res.append(call("vertex normals", ctx, b(M), b(T), b(V), b(good(normals=_abi.MESH_RASTER_NORMALS_VERTEX))))
    for kw in (dict(focal_length=(0.0, 10.0)), dict(focal_length=(10.0, inf)), dict(principal_point=(nan, 0.5)), dict(width=0), dict(height=0), dict(width=16385)):
        res.append(call("view %r" % (kw,), ctx, b(M), b(T), b(view(**kw)), b(good())))
    x = np.array(front_view()["xform"], np.float32)
    x[1, 2] = nan
    res.append(call("xform", ctx, b(M), b(T), b(view(xform=x)), b(good())))
    res.append(call("multiple of 3", ctx, b(mesh(3, 4)), b(T), b(V), b(good())))
    res.append(call("no vertices", ctx, b(mesh(0, 3)), b(T), b(V), b(good())))
    return res


def test_draw_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the context or the device is touched: the context handed in is a block of zeros, and no device exists here."""
    api, _abi = _built()
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    res = refusals(fns, _abi, api, C.cast(fake, C.c_void_p))
    assert len(res) >= 30
    for label, rc, msg in res:
        assert rc == _abi.ERR_INVALID and msg.startswith(b"rnb_mesh_draw_textured"), (label, rc, msg)
    msgs = {label: msg for label, rc, msg in res}
    assert b"no map" in msgs["no map"] and b"multiple of 3" in msgs["multiple of 3"] and b"no vertices" in msgs["no vertices"] and b"needs a mesh with normals" in msgs["vertex normals"]
    assert b"filter" in msgs["filter=2"] and b"reserved" in msgs["reserved"] and b"uv_dev" in msgs["null uv"] and b"16 bytes" in msgs["misaligned map"] and b"2 triangles" in msgs["n_tris"]
    assert fake.raw == b"\0" * 4096


# ------------------------------------------------------------------------------------------------------------------------ the statement's own properties
def _scene():
    from tests.test_gpu_mesh_project import small_scene
    return small_scene()


def random_maps(size, seed, tris=34, block=0):
    """Random float maps: alpha 1 on owned texels and 0 elsewhere (the baker's), a few all-zero normal texels among the owned ones."""
    lay = tr.layout(tris, size, block)
    tri, _ = tr.ownership(tris, size, lay["block"], lay["blocks_per_row"])
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 1.0, (size, size, 4)).astype(np.float32)
    normal = rng.uniform(-1.0, 1.0, (size, size, 4)).astype(np.float32)
    color[..., 3] = normal[..., 3] = tri >= 0
    dead = (tri >= 0) & (rng.uniform(0, 1, (size, size)) < 0.05)
    normal[dead, :3] = 0.0
    return tr.uvs(tris, size, lay["block"], lay["blocks_per_row"]), color, normal, lay


def test_the_statement_keeps_the_fill_and_reaches_every_branch():
    v, t, n, views = _scene()
    uv, color, normal, _ = random_maps(64, 1)
    uv = uv.copy()
    uv[3, 1, 0] = np.nan  # a NaN corner
    uv[8] = uv[8] * 3.0 - 1.0  # outside [0, 1]: the clamp
    total = dict.fromkeys(dr.BRANCHES, 0)
    for filt in ("bilinear", "nearest"):
        for view in views:
            want = mr.rasterize(v, t, view, normals=n, shading="vertex")
            got = dr.draw(v, t, view, uv, color, normal, normals=n, shading="vertex", filter=filt)
            assert np.array_equal(_bits(got["image"][..., 6:9]), _bits(want["image"][..., 6:9])) and np.array_equal(got["faces"], want["faces"]) and got["stats"] == want["stats"]
            covered = got["image"][..., 6] == 1
            assert not got["image"][~covered].any()
            length = np.linalg.norm(got["image"][covered][:, :3].astype(np.float64), axis=1)
            assert (np.abs(length - 1.0) <= 2.0 ** -22).all()
            assert got["n_unowned_taps"] == got["unowned"].sum() and not got["unowned"][~covered].any()
            for key in total:
                total[key] += got["tallies"][key]
            only_n = dr.draw(v, t, view, uv, None, normal, filter=filt)  # without a colour map: rule 6's colour (ones), the normal map's alpha decides unowned
            assert np.array_equal(_bits(only_n["image"][..., 3:6]), _bits(mr.rasterize(v, t, view)["image"][..., 3:6]))
            only_c = dr.draw(v, t, view, uv, color, None, filter=filt)
            assert np.array_equal(_bits(only_c["image"][..., 0:3]), _bits(mr.rasterize(v, t, view)["image"][..., 0:3])) and only_c["n_normal_fallback"] == 0
    assert all(total[key] > 0 for key in total), total


def test_a_constant_map_gives_the_constant():
    v, t, n, views = _scene()
    uv, color, _, _ = random_maps(67, 2, block=9)
    const = np.float32([0.3, 0.7123, 0.05])
    color[color[..., 3] == 1, :3] = const
    color[color[..., 3] == 0, :3] = 9.0  # what an unowned texel would bring in
    for filt in ("bilinear", "nearest"):
        for view in views[2:]:
            r = dr.draw(v, t, view, uv, color, filter=filt)
            clean = (r["image"][..., 6] == 1) & ~r["unowned"]
            assert clean.sum() > 100
            ulps = np.abs(_bits(r["image"][clean][:, 3:6]).astype(np.int64) - _bits(const).astype(np.int64))
            assert ulps.max() <= 1 and (ulps == 0).mean() > 0.99


def position_bound(verts, tris, size, block):
    """(S / n + 4) * 2^-24 * (longest edge + max |coordinate|), n = block - 3: a float uv is off by at most 2^-24, that is S * 2^-24 texels, of which one is edge / n; the
    texel values and the output are each rounded to float once (2 * 2^-24 * max |coordinate|), and the double arithmetic between them is far below one more."""
    v = np.asarray(verts, np.float64)
    edge = max(np.linalg.norm(v[tris[:, a]] - v[tris[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    return (size / (block - 3) + 4) * 2.0 ** -24 * (edge + np.abs(v).max())


def test_the_position_map_gives_the_point_under_the_pixel():
    v, t, n, views = _scene()
    for size, block in ((64, 0), (67, 9)):
        lay = tr.layout(len(t), size, block)
        uv = tr.uvs(len(t), size, lay["block"], lay["blocks_per_row"])
        pos = tr.positions(v, t, size, lay["block"], lay["blocks_per_row"])
        bound = position_bound(v, t, size, lay["block"])
        for view in views:
            r = dr.draw(v, t, view, uv, pos)
            pix, want = dr.surface_points(v, t, view, r["faces"])
            if len(pix):
                err = np.abs(r["image"].reshape(-1, 9)[pix, 3:6].astype(np.float64) - want).max()
                assert err <= bound, (size, block, err, bound)


# ------------------------------------------------------------------------------------------------------------------------ view_albedo_metrics
def test_view_albedo_metrics_on_known_answers():
    from rnb_neus2_amd import api
    rng = np.random.default_rng(4)
    h, w = 12, 20
    amap = rng.integers(0, 65536, (h, w, 4)).astype(np.uint16)
    amap[..., 3] = 65535
    amap[:3, :, 3] = 0
    img = np.zeros((h, w, 9), np.float32)
    img[..., 6] = 1.0
    img[:, :4, 6] = 0.0
    exact = amap[..., :3].astype(np.float64) / 65535.0
    img[..., 3:6] = exact  # rounded to float: mae of the order of 2^-25
    r = api.view_albedo_metrics(img, front_view(w, h), amap)
    assert r["pixels_compared"] == (h - 3) * (w - 4) and r["albedo_mae"] < 2.0 ** -24 and r["albedo_psnr_db"] > 140
    eight = (np.arange(h * w * 4).reshape(h, w, 4) % 256).astype(np.uint8)
    eight[..., 3] = 255
    img[..., 3:6] = (eight[..., :3].astype(np.float64) / 255.0).astype(np.float32)
    r = api.view_albedo_metrics(img, front_view(w, h), eight)
    assert r["albedo_mae"] < 2.0 ** -24
    # an equal image: values a float holds exactly
    half = np.full((h, w, 4), 255, np.uint8)
    img[..., 3:6] = 1.0
    r = api.view_albedo_metrics(img, front_view(w, h), half)
    assert r["albedo_mae"] == 0.0 and r["albedo_rmse"] == 0.0 and r["albedo_psnr_db"] == math.inf and r["pixels_compared"] == h * (w - 4)
    d = 0.125
    img[..., 3:6] = 1.0 - d
    r = api.view_albedo_metrics(img, front_view(w, h), half)
    assert r["albedo_mae"] == d and r["albedo_rmse"] == d and abs(r["albedo_psnr_db"] + 20.0 * math.log10(d)) < 1e-12
    img[..., 6] = 0.0
    img[:2, :, 6] = 1.0
    half[:2, :, 3] = 0  # disjoint masks
    r = api.view_albedo_metrics(img, front_view(w, h), half)
    assert r == dict(albedo_mae=0.0, albedo_rmse=0.0, albedo_psnr_db=0.0, pixels_compared=0)
    small = np.full((h // 2, w // 2, 4), 255, np.uint8)  # another resolution: the input pixel whose area holds the pixel's centre
    small[0, 0, :3] = 0
    img[..., 6] = 1.0
    img[..., 3:6] = 1.0
    r = api.view_albedo_metrics(img, front_view(w, h), small)
    assert r["pixels_compared"] == h * w and r["albedo_mae"] == 4.0 / (h * w)
    for bad in (np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.uint8)):
        with pytest.raises(ValueError):
            api.view_albedo_metrics(img, front_view(w, h), bad)


# ------------------------------------------------------------------------------------------------------------------------ the Python layer
def _fake(fail=None):
    from rnb_neus2_amd import _abi, api
    from tests import test_device_mesh_cpu as dm
    fake = dm.FakeLibrary(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake, dm


def test_draw_textured_makes_its_calls_in_order_and_releases_everything(monkeypatch):
    from rnb_neus2_amd import api
    c, fake, dm = _fake()
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_draw_textured", ((2,), None))
    names = lambda f: [e[0] for e in f.log if not e[0].endswith("default_options") and e[0] != "create"]
    uv, color, normal = np.zeros((2, 3, 2), np.float32), np.zeros((8, 8, 4), np.float32), np.ones((8, 8, 4), np.float32)
    up = ["device_malloc", "memcpy"]
    out = c.draw_textured_mesh(dm.V, dm.I, dm.VIEW, uv, color, normal, faces=True)
    assert names(fake) == up * 2 + up * 3 + ["device_malloc"] * 2 + ["mesh_draw_textured"] + ["memcpy"] * 2 + ["device_free"] * 2 + ["device_free"] * 3 + ["device_free"] * 2
    assert out["image"].shape == (4, 6, 9) and out["faces"].shape == (4, 6) and {"n_bad_uv", "n_normal_fallback", "n_unowned_taps", "n_covered", "ms"} <= set(out)
    assert not fake.buffers and not fake.meshes and not fake.errors
    with c.upload_mesh(dm.V, dm.I) as m:
        log = len(fake.log)
        m.draw_textured(dm.VIEW, uv, normal=normal, filter="nearest", out_ptr=0x9000)
        assert names(fake)[-7:] == up * 2 + ["mesh_draw_textured"] + ["device_free"] * 2 and [e for e in fake.log[log:] if e[0] == "mesh_draw_textured"] == [("mesh_draw_textured", (m.verts,))]
        held = set(fake.buffers)
        for kw in (dict(filter="trilinear"), dict(uv=uv[:1]), dict(color=None, normal=None), dict(shading="vertex"), dict(cull="both"), dict(color=np.zeros((8, 4, 4), np.float32)),
                   dict(color=np.zeros((8, 8, 3), np.float32)), dict(color=color, normal=np.zeros((4, 4, 4), np.float32))):
            n = len(fake.device_log())
            with pytest.raises(ValueError):
                m.draw_textured(dm.VIEW, **dict(dict(uv=uv, color=color), **kw))
            assert len(fake.device_log()) == n and fake.buffers == held, kw  # checked before anything is uploaded
    with pytest.raises(ValueError):
        m.draw_textured(dm.VIEW, uv, color)  # freed
    for stage in ("mesh_draw_textured", "device_malloc"):  # a failing step leaves nothing allocated
        c, fake, dm = _fake(fail=stage)
        with pytest.raises(api.RnbError):
            c.draw_textured_mesh(dm.V, dm.I, dm.VIEW, uv, color, normal)
        assert not fake.buffers and not fake.meshes and not fake.errors, stage


def test_mesh_view_metrics_is_what_it_was_without_the_new_keywords(monkeypatch):
    """With texture and albedo_maps left at None every view goes through DeviceMesh.rasterize with the arguments it got before, draw_textured is not reached, and the
    result has the keys it had; with a texture the views go through the draw, the texture uploaded once."""
    from rnb_neus2_amd import api
    sig = inspect.signature(api.Context.mesh_view_metrics).parameters
    assert sig["texture"].default is None and sig["albedo_maps"].default is None and list(sig)[-2:] == ["texture", "albedo_maps"]
    c, fake, dm = _fake()
    calls = []
    image = np.zeros((4, 6, 9), np.float32)

    def rasterize(self, view, near=2.0 ** -10, cull="none", shading="face", faces=False, stream=None, out_ptr=None):
        calls.append((near, cull, shading, faces, stream, out_ptr))
        return dict(image=image, n_back_pixels=3, ms=0.25)

    def never(self, *a, **kw):
        raise AssertionError("the draw was reached")

    monkeypatch.setattr(api.DeviceMesh, "rasterize", rasterize)
    monkeypatch.setattr(api.DeviceMesh, "_draw", never)
    monkeypatch.setattr(api.DeviceMesh, "draw_textured", never)
    out = c.mesh_view_metrics(dm.V, dm.I, [dm.VIEW, dm.VIEW], [dm.NORMAL_MAP, dm.NORMAL_MAP], cull="back")
    assert calls == [(2.0 ** -10, "back", "face", False, None, None)] * 2
    assert sorted(out["mean"]) == ["mask_iou", "mean_angle_deg", "median_angle_deg"]
    assert [sorted(e) for e in out["views"]] == [["mask_iou", "mean_angle_deg", "median_angle_deg", "ms", "n_back_pixels", "odd_count_pixels", "pixels_compared"]] * 2
    assert not [e for e in fake.log if "draw" in e[0]] and not fake.buffers and not fake.meshes and not fake.errors
    monkeypatch.undo()
    c, fake, dm = _fake()
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_draw_textured", ((2,), None))
    tex = dict(uv=np.zeros((2, 3, 2), np.float32), color=np.zeros((8, 8, 4), np.float32), normal=None)
    amap = np.full((4, 6, 4), 255, np.uint8)
    out = c.mesh_view_metrics(dm.V, dm.I, [dm.VIEW, dm.VIEW], [dm.NORMAL_MAP, dm.NORMAL_MAP], texture=tex, albedo_maps=[amap, amap])
    stages = [e[0] for e in fake.log if e[0] in ("mesh_raster", "mesh_draw_textured")]
    assert stages == ["mesh_draw_textured"] * 2 and len([e for e in fake.log if e[0] == "device_malloc"]) == 2 + 2 + 2  # the mesh, uv and colour once, an image per view
    assert sorted(out["mean"]) == ["albedo_mae", "albedo_psnr_db", "albedo_rmse", "mask_iou", "mean_angle_deg", "median_angle_deg"]
    assert all({"albedo_mae", "albedo_rmse", "albedo_psnr_db", "mean_angle_deg"} <= set(e) for e in out["views"])
    assert not fake.buffers and not fake.meshes and not fake.errors
    for bad in (dict(albedo_maps=[amap, amap]), dict(texture=dict(uv=tex["uv"], normal=tex["color"]), albedo_maps=[amap, amap]), dict(texture=tex, albedo_maps=[amap])):
        with pytest.raises(ValueError):
            c.mesh_view_metrics(dm.V, dm.I, [dm.VIEW, dm.VIEW], [dm.NORMAL_MAP, dm.NORMAL_MAP], **bad)
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_the_bench_tool_holds_no_private_plumbing():
    """The rule tests/test_device_mesh_cpu.py applies to the other mesh tools: the public mesh interface and mesh_bench_common only."""
    with open(os.path.join(ROOT, "tools", "bench_mesh_draw.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "m._", "_abi.Mesh(", "C.byref", "_abi"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".draw_textured(" in text and ".rasterize(" in text and ".mesh_view_metrics(" in text and ".project_views(" in text


def test_the_command_lines_albedo_comparison_is_the_python_one(tmp_path):
    """view_metrics::compare_albedo (host/view_metrics.hpp, what build/mesh --report-views writes) on a random image against api.view_albedo_metrics on the same data, to
    1e-12 relative (the same sums in the same order); num_full writes every digit, and null for what is not finite (a PSNR of equal images), never a number."""
    from rnb_neus2_amd import api
    rng = np.random.default_rng(9)
    h, w, ih, iw = 11, 14, 7, 9
    img = rng.uniform(0, 1, (h, w, 9)).astype(np.float32)
    img[..., 6] = rng.uniform(0, 1, (h, w)) > 0.3
    amap = rng.integers(0, 65536, (ih, iw, 4)).astype(np.uint16)
    amap[1, :, 3] = 0
    img.tofile(tmp_path / "img.bin")
    amap.tofile(tmp_path / "map.bin")
    src = tmp_path / "cmp.cpp"
    src.write_text('''#include "view_metrics.hpp"
#include <limits>
int main(int, char** argv) {
	std::vector<float> img(%d); std::vector<uint16_t> map(%d);
	FILE* f = std::fopen(argv[1], "rb"); if (std::fread(img.data(), 4, img.size(), f) != img.size()) return 1; std::fclose(f);
	f = std::fopen(argv[2], "rb"); if (std::fread(map.data(), 2, map.size(), f) != map.size()) return 1; std::fclose(f);
	const view_metrics::AlbedoResult r = view_metrics::compare_albedo(img.data(), 9, %d, %d, map.data(), %d, %d);
	std::printf("%%s %%s %%s %%zu\\n", view_metrics::num_full(r.mae).c_str(), view_metrics::num_full(r.rmse).c_str(), view_metrics::num_full(r.psnr_db).c_str(), r.pixels_compared);
	std::printf("%%s %%s %%s\\n", view_metrics::num_full(std::numeric_limits<double>::infinity()).c_str(), view_metrics::num_full(std::nan("")).c_str(), view_metrics::num_full(0.1).c_str());
	return 0;
}
''' % (img.size, amap.size, w, h, iw, ih))
    exe = tmp_path / "cmp"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rnb-neus2_amd", "host"), str(src), "-o", str(exe)])
    first, second = subprocess.check_output([str(exe), str(tmp_path / "img.bin"), str(tmp_path / "map.bin")]).decode().splitlines()
    want = api.view_albedo_metrics(img, front_view(w, h), amap)
    mae, rmse, psnr, n = first.split()
    assert int(n) == want["pixels_compared"] > 50
    for got, key in ((mae, "albedo_mae"), (rmse, "albedo_rmse"), (psnr, "albedo_psnr_db")):
        assert abs(float(got) - want[key]) <= 1e-12 * abs(want[key]), key
    assert second.split()[:2] == ["null", "null"] and float(second.split()[2]) == 0.1 and json.loads("[%s]" % second.split()[0]) == [None]
