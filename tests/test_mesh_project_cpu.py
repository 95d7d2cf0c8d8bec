"""CPU tier of the view projection (include/rnb_mesh_project.h): the C-ABI of the new header (exports, versions, defaults, struct layout, argument validation without a
device), the numpy statement of tests/mesh_project_reference.py on cases with known answers, the calls the Python layer makes on a recording stand-in for the library,
the command line and the pipeline's argv. No test here needs a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_project_reference as pr
from tests import mesh_texture_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_project.h")
NAMES = ["rnb_mesh_project_abi_version", "rnb_mesh_project_default_options", "rnb_mesh_project_views", "rnb_mesh_projection_free"]


def _built():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    return api, _abi


def front_view(w=64, h=48, f=60.0):
    """A camera at (0.5, 0.5, -1) that looks along +z: right = +x, down = +y."""
    return dict(width=w, height=h, focal_length=(f, f), principal_point=(0.5, 0.5), xform=np.float32([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, -1.0]]))


def quad(lo, hi, z, toward_camera=True):
    """Two triangles over [lo, hi]^2 at depth z; their face normal is -z (towards front_view's camera) or +z."""
    v = np.float32([[lo, lo, z], [lo, hi, z], [hi, lo, z], [hi, hi, z]])
    t = np.uint32([[0, 1, 2], [2, 1, 3]])
    return v, (t if toward_camera else t[:, ::-1].copy())


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_project_header_is_exported_by_the_hip_library():
    api, _abi = _built()
    from rnb_neus2_amd import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"}) == NAMES
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in NAMES)
    assert set("rnb_" + k for k in _abi.MESH_PROJECT_PROTOTYPES) == set(NAMES)
    others = (_abi.PROTOTYPES, _abi.RENDER_PROTOTYPES, _abi.MESH_PROTOTYPES, _abi.MESH_CLEAN_PROTOTYPES, _abi.MESH_SIMPLIFY_PROTOTYPES, _abi.MESH_DISTANCE_PROTOTYPES,
              _abi.MESH_RASTER_PROTOTYPES, _abi.MESH_TEXTURE_PROTOTYPES, _abi.MESH_VISIBILITY_PROTOTYPES)
    assert not set(_abi.MESH_PROJECT_PROTOTYPES) & set().union(*others)
    assert "mesh_project" in inspect.signature(_abi.declare).parameters
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_raster_abi_version() == 1 and fns.mesh_texture_abi_version() == 1 and fns.mesh_visibility_abi_version() == 1  # as they were
    assert fns.mesh_project_abi_version() == _abi.MESH_PROJECT_ABI_VERSION == 1
    o = _abi.MeshProjectOptions()
    o.block, o.mode, o.cull, o.fallback_dev, o.reserved[2] = 9, 1, 2, 0x1000, 4
    assert fns.mesh_project_default_options(C.byref(o)) == 0
    assert (o.abi_version, o.size, o.block, o.mode, o.normals, o.weight_power, o.min_cos, o.depth_tolerance, o.near, o.cull, o.fallback_dev, list(o.reserved)) == (
        1, 1024, 0, _abi.MESH_PROJECT_MODE_BLEND, _abi.MESH_PROJECT_NORMALS_FACE, 2, np.float32(0.1), 2.0 ** -8, 2.0 ** -10, _abi.MESH_RASTER_CULL_NONE, None, [0] * 4)
    assert fns.mesh_project_default_options(None) == _abi.ERR_INVALID
    for name in ("project_views", "_project_options"):
        assert hasattr(api.Context, name), name
    assert hasattr(api.DeviceMesh, "project_views")
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_project.cuh") in build.DEPS
    assert re.findall(r'#include\s+"([^"]+)"', open(HEADER).read()) == ["rnb_mesh.h"]
    for name in os.listdir(os.path.join(ROOT, "include")):  # no other header mentions this one, and the training header gained no function
        assert name == "rnb_mesh_project.h" or "project" not in open(os.path.join(ROOT, "include", name)).read().lower(), name


def test_the_projection_shares_the_fill_and_the_texel_function():
    """The fill kernels are launched by raster_fill alone, which the projection calls; the texel's owner, weights and position come from the baker's device functions."""
    drv = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "driver_mesh.hpp")).read()
    assert len(re.findall(r"\braster_fill<\w+>\(", drv)) == 3 and "raster_fill<MP_FILL_TALLIES>(\"rnb_mesh_project_views\"" in drv
    assert len(re.findall(r"hipLaunchKernelGGL\(\(?k_mr_bin<", drv)) == 2 and len(re.findall(r"hipLaunchKernelGGL\(k_mr_fill_large<", drv)) == 1
    new = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_project.cuh")).read()
    for needle in ("mr_edge", "mr_setup", "mr_cover", "atomicMin", "atomicCAS"):
        assert needle not in new, needle
    assert "mt_texel(" in new and "mt_position(" in new and "mt_corner_uv(" in new and "fp contract(off)" in new
    baker = open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_texture.cuh")).read()
    assert baker.count("void mt_position(") == 1 and "mt_position(A, t, verts, idx" in baker.split("void k_mt_texels")[1]


def test_project_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = [("rnb_mesh_project_view", _abi.MeshProjectView), ("rnb_mesh_project_options", _abi.MeshProjectOptions), ("rnb_mesh_projection", _abi.MeshProjection),
               ("rnb_mesh_project_stats", _abi.MeshProjectStats)]
    consts = ["ABI_VERSION", "NONE", "MAX_WEIGHT_POWER", "FORMAT_F32", "FORMAT_U16", "FORMAT_U8", "MODE_BLEND", "MODE_BEST", "NORMALS_FACE", "NORMALS_VERTEX"]
    body, want = "", []
    for cname, S in structs:
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % cname + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, n) for n, _ in S._fields_)
        want += [C.sizeof(S)] + [getattr(S, n).offset for n, _ in S._fields_]
    body += "".join("  printf(\"%%llu\\n\", (unsigned long long)RNB_MESH_PROJECT_%s);\n" % c for c in consts)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_project.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:len(want)] == want
    assert out[len(want):] == [getattr(_abi, "MESH_PROJECT_" + c) for c in consts]
    assert (pr.NONE, pr.MAX_WEIGHT_POWER) == (_abi.MESH_PROJECT_NONE, _abi.MESH_PROJECT_MAX_WEIGHT_POWER)
    assert _abi.MESH_PROJECT_FORMATS == dict(float32=0, uint16=1, uint8=2)
    assert sorted(_abi.MeshProjectStats().as_dict()) == ["ms", "n_occluded", "n_pairs_tested", "n_texels", "n_textured", "peak_workspace"]


def refusals(fns, _abi, api, ctx, mesh_ptrs=(0x1000, 0x2000, 0x3000), image=0x4000):
    """Every call the header lists as refused before the device is touched, as (label, status, message): shared with the GPU tier, which hands in a live context."""
    def good(**kw):
        o = _abi.MeshProjectOptions()
        assert fns.mesh_project_default_options(C.byref(o)) == 0
        o.size = 64
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def mesh(nv=3, ni=3, normals=False):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, mesh_ptrs[0], mesh_ptrs[1]
        if normals:
            m.normals = mesh_ptrs[2]
        return m

    def views(n=2, view=None, **kw):
        arr = (_abi.MeshProjectView * n)()
        for e in arr:
            e.view = api._view_struct(front_view())
            e.image_dev, e.image_width, e.image_height, e.format = image, 4, 4, _abi.MESH_PROJECT_FORMAT_U8
        if view:
            arr[n - 1].view = api._view_struct(dict(front_view(), **view))
        for k, v in kw.items():
            setattr(arr[n - 1], k, v)  # the bad view is the last one
        return arr

    out, st = _abi.MeshProjection(), _abi.MeshProjectStats()

    def call(label, ctx_, m, arr, n, o, dst=True):
        out.uv, out.size, st.n_texels = 0x5000, 7, 7
        rc = fns.mesh_project_views(ctx_, None, m, arr, n, o, C.byref(out) if dst else None, C.byref(st))
        msg = fns.last_error()
        assert st.n_texels == 0 and (not dst or (not out.uv and out.size == 0)), label  # *stats and *out zeroed
        return label, rc, msg

    M = mesh()
    res = [call("null ctx", None, C.byref(M), views(), 2, C.byref(good())), call("null mesh", ctx, None, views(), 2, C.byref(good())),
           call("null views", ctx, C.byref(M), None, 2, C.byref(good())), call("null opt", ctx, C.byref(M), views(), 2, None),
           call("null out", ctx, C.byref(M), views(), 2, C.byref(good()), dst=False), call("n_views", ctx, C.byref(M), views(), 0, C.byref(good()))]
    for field, value in [("abi_version", 2), ("abi_version", 0), ("size", 3), ("size", 8193), ("mode", 2), ("normals", 2), ("weight_power", 9), ("min_cos", -0.1), ("min_cos", 1.0),
                         ("min_cos", float("nan")), ("depth_tolerance", -1.0), ("depth_tolerance", float("inf")), ("depth_tolerance", float("nan")), ("near", 0.0), ("near", float("nan")),
                         ("near", float("inf")), ("cull", 3), ("fallback_dev", 0x6008)]:
        res.append(call("%s=%r" % (field, value), ctx, C.byref(M), views(), 2, C.byref(good(**{field: value}))))
    o = good()
    o.reserved[3] = 1
    res.append(call("reserved", ctx, C.byref(M), views(), 2, C.byref(o)))
    res.append(call("vertex normals", ctx, C.byref(M), views(), 2, C.byref(good(normals=_abi.MESH_PROJECT_NORMALS_VERTEX))))
    for kw in (dict(focal_length=(0.0, 10.0)), dict(focal_length=(10.0, float("inf"))), dict(principal_point=(float("nan"), 0.5)), dict(width=0), dict(height=0), dict(width=16385)):
        res.append(call("view %r" % (kw,), ctx, C.byref(M), views(view=kw), 2, C.byref(good())))
    for kw in (dict(image_dev=None), dict(image_width=0), dict(image_height=0), dict(format=3), dict(reserved=1), dict(format=_abi.MESH_PROJECT_FORMAT_F32, image_dev=image + 8),
               dict(format=_abi.MESH_PROJECT_FORMAT_U16, image_dev=image + 4)):
        res.append(call("image %r" % (kw,), ctx, C.byref(M), views(**kw), 2, C.byref(good())))
    res.append(call("multiple of 3", ctx, C.byref(mesh(3, 4)), views(), 2, C.byref(good())))
    res.append(call("no vertices", ctx, C.byref(mesh(0, 3)), views(), 2, C.byref(good())))
    res.append(call("layout", ctx, C.byref(mesh(3, 3 * 600)), views(), 2, C.byref(good())))  # 300 blocks of 4 need 18 per row: 72 texels
    res.append(call("block", ctx, C.byref(M), views(), 2, C.byref(good(block=3))))
    return res


def test_project_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the context or the device is touched: the context handed in is a block of zeros, and no device exists here."""
    api, _abi = _built()
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    res = refusals(fns, _abi, api, C.cast(fake, C.c_void_p))
    assert len(res) >= 40
    for label, rc, msg in res:
        assert rc == _abi.ERR_INVALID and msg, label
    msgs = {label: msg for label, rc, msg in res}
    assert b"n_views" in msgs["n_views"] and b"multiple of 3" in msgs["multiple of 3"] and b"no vertices" in msgs["no vertices"] and b"needs a mesh with normals" in msgs["vertex normals"]
    assert re.search(rb"the smallest size that would fit is 72$", msgs["layout"]) and b"rnb_mesh_texture_layout" in msgs["layout"]  # the baker's message
    assert fake.raw == b"\0" * 4096
    pj = _abi.MeshProjection()
    assert fns.mesh_projection_free(None, C.byref(pj)) == _abi.ERR_INVALID and fns.mesh_projection_free(C.cast(fake, C.c_void_p), None) == _abi.ERR_INVALID
    assert fns.mesh_projection_free(C.cast(fake, C.c_void_p), C.byref(pj)) == 0  # nothing to release


# ------------------------------------------------------------------------------------------------------------------------ the statement on known answers
def test_a_quad_facing_the_camera_takes_the_constant_of_its_image():
    v, t = quad(0.2, 0.8, 0.5)
    const = np.float32([0.25, 0.5, 0.8125, 1.0])
    for image in (np.tile(const, (5, 7, 1)), np.tile(np.uint16([1000, 30000, 65535, 65535]), (9, 4, 1)), np.tile(np.uint8([3, 128, 255]), (6, 6, 1))):
        for mode in ("blend", "best"):
            r = pr.project(v, t, [front_view()], [image], 16, mode=mode)
            assert r["block"] == 16 and r["stats"]["n_texels"] == 256 == r["stats"]["n_textured"] and r["stats"]["n_occluded"] == 0
            assert (r["info"][..., 0] == 1).all() and (r["info"][..., 1] == 0).all() and r["tallies"]["contributed"] == 256 and not any(r["tallies"][k] for k in pr.SKIPS)
            want = pr.decode(image)[0, 0, :3].astype(np.float32)
            assert np.array_equal(r["color"][..., :3].view(np.uint32), np.broadcast_to(want, (16, 16, 3)).view(np.uint32)) and (r["color"][..., 3] == 1).all()  # expected: 0 ulp
    r = pr.project(v, t, [front_view()], [np.zeros((4, 4, 4), np.uint8)], 16, fallback=np.full((16, 16, 4), 0.5, np.float32))  # alpha 0 everywhere: q_a == 0
    assert r["tallies"]["empty"] == 256 and r["stats"]["n_textured"] == 0 and r["stats"]["n_pairs_tested"] == 256 and (r["color"] == 0.5).all()
    assert (r["info"][..., 0] == 0).all() and (r["info"][..., 1] == pr.NONE).all()


def test_a_blocker_in_front_leaves_count_zero_in_its_shadow():
    v0, t0 = quad(0.2, 0.8, 0.5)
    v1, t1 = quad(0.4, 0.6, 0.0)  # its shadow on the plane z = 0.5, seen from z = -1, is [0.35, 0.65]^2
    v, t = np.concatenate([v0, v1]), np.concatenate([t0, t1 + 4])
    view = front_view(256, 192, 240.0)
    r = pr.project(v, t, [view], [np.full((8, 8, 4), 255, np.uint8)], 64)
    pos, own = tr.positions(v, t, 64, r["block"], r["blocks_per_row"]), r["own"]
    tri, _ = tr.ownership(4, 64, r["block"], r["blocks_per_row"])
    plane = own & (tri < 2)
    x, y = pos[..., 0], pos[..., 1]
    pixel = 1.5 / 240.0  # one pixel at depth 1.5, in world units
    inside = plane & (np.maximum(np.abs(x - 0.5), np.abs(y - 0.5)) < 0.15 - pixel)
    outside = plane & (np.maximum(np.abs(x - 0.5), np.abs(y - 0.5)) > 0.15 + pixel)
    assert inside.sum() > 50 and outside.sum() > 500
    assert (r["info"][inside, 0] == 0).all() and (r["info"][inside, 1] == pr.NONE).all() and (r["color"][inside] == [0, 0, 0, 1]).all()
    assert (r["info"][outside, 0] == 1).all() and (r["color"][outside] == 1).all()
    assert (r["info"][own & (tri >= 2), 0] == 1).all()  # the blocker itself is seen
    assert r["tallies"]["occluded"] == r["stats"]["n_occluded"] >= inside.sum()
    loose = pr.project(v, t, [view], [np.full((8, 8, 4), 255, np.uint8)], 64, depth_tolerance=0.6)  # 1.5 <= 1.0 * 1.6: the slack swallows the blocker
    assert loose["stats"]["n_occluded"] == 0 and (loose["info"][plane, 0] == 1).all()


def test_a_quad_that_faces_away_takes_no_view():
    v, t = quad(0.2, 0.8, 0.5, toward_camera=False)
    r = pr.project(v, t, [front_view(), front_view(32, 32, 30.0)], [np.full((4, 4, 4), 255, np.uint8)] * 2, 16, min_cos=0.0)
    assert r["stats"]["n_textured"] == 0 and r["tallies"]["flat"] == 2 * 256 and r["stats"]["n_pairs_tested"] == 0
    assert (r["info"][..., 0] == 0).all() and (r["info"][..., 1] == pr.NONE).all() and (r["color"] == [0, 0, 0, 1]).all()
    n = np.tile(np.float32([0, 0, -1]), (4, 1))  # vertex normals that do face the camera, on the same triangles
    r = pr.project(v, t, [front_view()], [np.full((4, 4, 4), 255, np.uint8)], 16, normals="vertex", vnormals=n, cull="front")
    assert r["stats"]["n_textured"] == 256


# ------------------------------------------------------------------------------------------------------------------------ the Python layer
def _fake(dm, fail=None):
    class Fake(dm.FakeLibrary):
        """FakeLibrary whose projection and bake hand out device buffers: the two free calls must release them."""
        def __getattr__(self, name):
            base = super().__getattr__(name)

            def call(*args):
                rc = base(*args)
                owned = dict(mesh_project_views=(6, ("uv", "color", "info")), mesh_bake_texture=(4, ("uv", "albedo")))
                freed = dict(mesh_projection_free=("uv", "color", "info"), mesh_texture_free=("uv", "albedo", "normal", "position"))
                if rc == 0 and name in owned:
                    k, fields = owned[name]
                    s = args[k]._obj
                    for f in fields:
                        setattr(s, f, self._ptr())
                        self.buffers.add(getattr(s, f))
                    s.size, s.block, s.blocks_per_row, s.n_tris = 8, 8, 1, 2
                if name in freed:
                    s = args[1]._obj
                    for f in freed[name]:
                        if getattr(s, f):
                            self._release(self.buffers, getattr(s, f), name)
                    C.memset(C.byref(s), 0, C.sizeof(s))
                return rc
            return call
    from rnb_neus2_amd import _abi, api
    fake = Fake(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


def test_project_views_makes_its_calls_in_order_and_releases_everything(monkeypatch):
    from rnb_neus2_amd import api
    from tests import test_device_mesh_cpu as dm
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_project_views", ((2,), None))
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_bake_texture", ((2,), None))
    images = [np.zeros((3, 5, 4), np.uint16), np.zeros((2, 2, 3), np.uint8)]
    names = lambda fake: [e[0] for e in fake.log if not e[0].endswith("default_options") and e[0] != "create"]
    c, fake = _fake(dm)
    out = c.project_views(dm.V, dm.I, [dm.VIEW, dm.VIEW], images, size=8)
    up = ["device_malloc", "memcpy"]
    assert names(fake) == up * 2 + up * 2 + ["mesh_project_views"] + ["memcpy"] * 3 + ["mesh_projection_free", "mesh_texture_free"] + ["device_free"] * 2 + ["device_free"] * 2
    assert sorted(out) == ["block", "blocks_per_row", "color", "info", "stats", "uv"] and out["color"].shape == (8, 8, 4) and out["info"].shape == (8, 8, 2) and out["uv"].shape == (2, 3, 2)
    assert out["info"].dtype == np.uint32 and sorted(out["stats"]) == ["ms", "n_occluded", "n_pairs_tested", "n_texels", "n_textured", "peak_workspace"]
    assert not fake.buffers and not fake.meshes and not fake.errors
    # the model as the fallback: one bake before the projection, on the same mesh; an array: one more upload
    c, fake = _fake(dm)
    with c.upload_mesh(dm.V, dm.I, normals=dm.COL) as m:
        m.project_views([dm.VIEW], images[:1], size=8, fallback="model")
        log = {e[0]: e[1] for e in fake.log}
        assert log["mesh_bake_texture"] == log["mesh_project_views"] == (m.verts,)
        assert names(fake)[6:] == up + ["mesh_bake_texture", "mesh_project_views"] + ["memcpy"] * 3 + ["mesh_projection_free", "mesh_texture_free", "device_free"]
        k = len(names(fake))
        m.project_views([dm.VIEW], images[:1], size=8, mode="best", fallback=np.zeros((8, 8, 4), np.float32))
        assert names(fake)[k:] == up * 2 + ["mesh_project_views"] + ["memcpy"] * 3 + ["mesh_projection_free", "mesh_texture_free"] + ["device_free"] * 2
        held = set(fake.buffers)
        for kw in (dict(mode="mean"), dict(normals="ring"), dict(weight_power=9), dict(weight_power=1.5), dict(min_cos=1.0), dict(depth_tolerance=-1.0), dict(cull="both"),
                   dict(fallback=np.zeros((4, 4, 4), np.float32)), dict(images=[]), dict(images=[np.zeros((2, 2), np.uint8)]), dict(images=[np.zeros((2, 2, 4), np.int32)]),
                   dict(images=[np.zeros((0, 2, 4), np.uint8)]), dict(views=[])):
            n = len(fake.device_log())
            with pytest.raises(ValueError):
                m.project_views(**dict(dict(views=[dm.VIEW], images=images[:1], size=8), **kw))
            assert len(fake.device_log()) == n and fake.buffers == held, kw  # checked before anything is uploaded
    with c.upload_mesh(dm.V, dm.I) as m:
        with pytest.raises(ValueError):
            m.project_views([dm.VIEW], images[:1], size=8, normals="vertex")
    with pytest.raises(ValueError):
        m.project_views([dm.VIEW], images[:1], size=8)  # freed
    assert not fake.buffers and not fake.meshes and not fake.errors
    for stage in ("mesh_project_views", "mesh_bake_texture", "device_malloc"):  # a failing stage leaves nothing allocated
        c, fake = _fake(dm, fail=stage)
        with pytest.raises(api.RnbError):
            c.project_views(dm.V, dm.I, [dm.VIEW, dm.VIEW], images, size=8, fallback="model")
        assert not fake.buffers and not fake.meshes and not fake.errors, stage


def test_extract_mesh_makes_the_calls_it_made_unless_texture_from_is_given(monkeypatch):
    from rnb_neus2_amd import api
    from tests import test_device_mesh_cpu as dm
    for name, call in dm.CALLS.items():  # the recorded sequences of the existing stages, with the projection bound
        c, fake = _fake(dm)
        call(c)
        assert fake.device_log() == dm.RECORDED[name], name
        assert not [e for e in fake.log if "project" in e[0]] and not fake.buffers and not fake.meshes and not fake.errors
    c, fake = _fake(dm)
    c.extract_mesh(16, keep="largest", simplify=8, error=True, colors=True, texture_from=None)
    assert fake.device_log() == dm.RECORDED["extract_mesh"]
    with pytest.raises(ValueError):
        c.extract_mesh(16, texture_from=([dm.VIEW], [np.zeros((2, 2, 4), np.uint8)]))  # needs texture
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_project_views", ((2,), None))
    monkeypatch.setitem(dm.MESH_ARGS, "mesh_bake_texture", ((2,), None))
    c, fake = _fake(dm)
    out = c.extract_mesh(16, keep="largest", simplify=8, texture=8, texture_from=([dm.VIEW], [np.zeros((2, 2, 4), np.uint8)]))
    stages = [e[0] for e in fake.log if e[0] in dm.STAGES or e[0] in ("mesh_bake_texture", "mesh_project_views")]
    assert stages == ["extract_mesh", "mesh_clean", "mesh_simplify", "mesh_bake_texture", "mesh_project_views"]
    log = {e[0]: e[1] for e in fake.log}
    assert log["mesh_bake_texture"] == log["mesh_project_views"] == (log["mesh_simplify"][1],)  # the final mesh
    assert sorted(out["texture"]) == ["block", "blocks_per_row", "color", "info", "stats", "uv"]
    assert not fake.buffers and not fake.meshes and not fake.errors
    for stage in ("mesh_project_views", "mesh_bake_texture"):
        c, fake = _fake(dm, fail=stage)
        with pytest.raises(api.RnbError):
            c.extract_mesh(16, keep="largest", texture=8, texture_from=([dm.VIEW], [np.zeros((2, 2, 4), np.uint8)]))
        assert not fake.buffers and not fake.meshes and not fake.errors, stage


# ------------------------------------------------------------------------------------------------------------------------ the command lines
def test_build_mesh_lists_the_flags_and_refuses_bad_values():
    _built()
    exe = os.path.join(ROOT, "build", "mesh")
    text = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert text.returncode == 0
    for flag in ("--texture-from=[SOURCE]", "--texture-mode=[MODE]", "--texture-depth-tolerance=[T]", "--texture-min-cos=[C]"):
        assert flag in text.stdout, flag
    need = ["--snapshot", "/nonexistent/s.msgpack", "--scene", "/nonexistent", "--out", "/nonexistent/o.obj"]
    tf = ["--texture", "64", "--texture-from", "views"]
    for extra, word in ((["--texture-from", "views"], "--texture"), (["--texture", "64", "--texture-from", "model"], "texture-from"), (["--texture", "64", "--texture-mode", "best"], "--texture-from"),
                        (["--texture", "64", "--texture-min-cos", "0.2"], "--texture-from"), (["--texture", "64", "--texture-depth-tolerance", "0.1"], "--texture-from"),
                        (tf + ["--texture-mode", "mean"], "texture-mode"), (tf + ["--texture-min-cos", "1"], "texture-min-cos"), (tf + ["--texture-min-cos", "-0.5"], "texture-min-cos"),
                        (tf + ["--texture-min-cos", "x"], "texture-min-cos"), (tf + ["--texture-depth-tolerance", "-1"], "texture-depth-tolerance"),
                        (tf + ["--texture-depth-tolerance", "inf"], "texture-depth-tolerance"), (["--texture", "64", "--texture-from"], "texture-from")):
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)
        assert r.returncode == 255 and word in r.stderr.splitlines()[0], (extra, r.returncode, r.stderr[:200])
    for extra in (tf, tf + ["--texture-mode=best", "--texture-depth-tolerance", "0.015625", "--texture-min-cos", "0.3", "--texture-maps", "normal"]):
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)  # parsed: the next complaint is the missing snapshot
        assert r.returncode == 1 and "does not exist" in r.stderr, (extra, r.returncode, r.stderr[:200])


def test_the_pipeline_forwards_the_flag_and_leaves_the_argv_alone_without_it():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    args = ("data", 1000, 256, "out/mesh.obj", "build/mesh")
    plain = pipeline.plan_device_postprocess(*args, texture=512)
    assert pipeline.plan_device_postprocess(*args, texture=512, texture_from=None) == plain and "--texture-from" not in plain
    assert pipeline.plan_device_postprocess(*args, texture=512, texture_from="views") == plain + ["--texture-from", "views"]
    assert pipeline.plan_device_postprocess(*args, simplify=64, texture=512, texture_from="views", keep_seen="faces") == pipeline.plan_device_postprocess(*args, simplify=64, texture=512) + [
        "--texture-from", "views", "--keep-seen", "faces"]
    for bad in (dict(texture_from="views"), dict(texture=512, texture_from="model")):
        with pytest.raises(ValueError):
            pipeline.plan_device_postprocess(*args, **bad)
    for fn in (pipeline.plan_device_postprocess, pipeline.run_device_postprocess, pipeline.run_full_pipeline):
        assert inspect.signature(fn).parameters["texture_from"].default is None
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("i", "t", "o", device_postprocess=True, texture_from="views")
    base = ["--input", "i", "--testbed", "build/testbed", "--output", "o"]
    p = run_pipeline.build_parser()
    for argv in (base, base + ["--device-postprocess"], base + ["--device-postprocess", "--texture", "256"]):
        assert "texture_from" not in run_pipeline.pipeline_kwargs(p.parse_args(argv))
    kw = run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess", "--texture", "256", "--texture-from", "views"]))
    assert kw["texture_from"] == "views" and kw["texture"] == 256
    for bad in (["--device-postprocess", "--texture-from", "views"], ["--texture-from", "views"], ["--device-postprocess", "--texture", "256", "--texture-from", "model"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(base + bad)


def test_the_bench_tool_holds_no_private_plumbing():
    """The rule tests/test_device_mesh_cpu.py applies to the other mesh tools: the public mesh interface and mesh_bench_common only."""
    with open(os.path.join(ROOT, "tools", "bench_mesh_project.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref", "_abi"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".project_views(" in text and ".visibility(" in text and ".bake_texture(" in text
