"""CPU tests of the texture baker (include/rnb_mesh_texture.h): the layout through the real library against the numpy statement (tests/mesh_texture_reference.py), the
properties the header promises of that statement (texel ownership, the bilinear footprint, corner and edge texels, the orientation of the UV triangles), the ctypes
mirrors against the header, the lifecycle of DeviceMesh.bake_texture on a recording stand-in for the library, the writers, the command line and the pipeline's argv.
No test here needs a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_texture_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_texture.h")
NAMES = ["rnb_mesh_bake_texture", "rnb_mesh_texture_abi_version", "rnb_mesh_texture_default_options", "rnb_mesh_texture_free", "rnb_mesh_texture_layout"]


def _built():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    return api, _abi


# ------------------------------------------------------------------------------------------------------------------------ layout
def test_layout_of_the_library_equals_the_statement():
    api, _abi = _built()
    seen_ok = seen_bad = 0
    for n_tris in (0, 1, 2, 3, 7, 8, 9, 1000):
        for size in (4, 64, 67, 8192):
            for block in (0, 4, 5, 16):
                try:
                    want = tr.layout(n_tris, size, block)
                except tr.LayoutError as e:
                    with pytest.raises(api.RnbError) as got:
                        api.Context.texture_layout(n_tris, size, block)
                    assert got.value.code == _abi.ERR_INVALID, (n_tris, size, block)
                    found = re.search(r"the smallest size that would fit is (\d+)", str(got.value))  # only this is read of the message
                    assert found and int(found.group(1)) == e.smallest, (n_tris, size, block, str(got.value))
                    if e.smallest <= tr.MAX_SIZE:  # and it is the smallest: it fits, one texel less does not
                        tr.layout(n_tris, e.smallest, block)
                        if e.smallest > tr.MIN_SIZE:
                            with pytest.raises(tr.LayoutError):
                                tr.layout(n_tris, e.smallest - 1, block)
                    seen_bad += 1
                else:
                    assert api.Context.texture_layout(n_tris, size, block) == want, (n_tris, size, block)
                    assert want["n_blocks"] <= want["blocks_per_row"] ** 2 and tr.MIN_BLOCK <= want["block"] <= size
                    seen_ok += 1
    assert seen_ok >= 60 and seen_bad >= 20, (seen_ok, seen_bad)
    assert api.Context.texture_layout(1000, 8192) == dict(block=8192 // 23, blocks_per_row=23, n_blocks=500)
    for size in (3, 0, 8193):
        with pytest.raises(api.RnbError):
            api.Context.texture_layout(2, size)
    with pytest.raises(api.RnbError):
        api.Context.texture_layout(2, 64, 3)


@pytest.mark.parametrize("b", range(4, 13))
def test_ownership_and_the_bilinear_footprint(b):
    """Every texel of a block is owned by exactly one of its two triangles; a bilinear lookup anywhere inside a UV triangle, edges included, gives a non-zero weight only to
    texels of the footprint the header names (i + j <= b - 2 for the lower triangle, i + j >= b for the upper one), all of them inside the block and owned by that
    triangle. (A lookup at a whole texel centre has neighbours of weight exactly zero; those are not read.)"""
    size, bpr = 3 * b + 1, 3
    tri, a = tr.ownership(2 * bpr * bpr, size, b, bpr)
    assert (tri[:bpr * b, :bpr * b] >= 0).all() and (tri[bpr * b:] == -1).all() and (tri[:, bpr * b:] == -1).all()
    n = b - 3
    for k in (0, 4, 8):
        ox, oy = (k % bpr) * b, (k // bpr) * b
        blk = tri[oy:oy + b, ox:ox + b]
        j, i = np.meshgrid(np.arange(b), np.arange(b), indexing="ij")
        assert np.array_equal(blk, np.where(i + j <= b - 1, 2 * k, 2 * k + 1))  # exactly one owner each
        assert (a[oy:oy + b, ox:ox + b].sum(-1) == n).all()  # the weights of a texel add up to n
        for upper in (0, 1):
            c = tr.corners(b)[upper].astype(np.float64)
            steps = 4 * n + 3  # a grid that is no multiple of the texel grid, so most lookups are between centres; the corners and edges are on it
            for p in range(steps + 1):
                for q in range(steps + 1 - p):
                    l1, l2 = p / steps, q / steps
                    x, y = c[0] + l1 * (c[1] - c[0]) + l2 * (c[2] - c[0])
                    taps = tr.bilinear_taps(x, y)
                    assert taps and abs(sum(t[2] for t in taps) - 1) < 1e-12
                    for ti, tj, _ in taps:
                        assert 0 <= ti < b and 0 <= tj < b, (b, upper, x, y)
                        assert (ti + tj >= b) if upper else (ti + tj <= b - 2), (b, upper, x, y, ti, tj)
                        assert blk[tj, ti] == 2 * k + upper
    # the corners sit on the centres of owned texels, and the UVs are those centres
    uv = tr.uvs(2 * bpr * bpr, size, b, bpr)
    for t in (0, 1, 8, 9, 17):
        k = t // 2
        c = tr.corners(b)[t & 1]
        for q in range(3):
            x, y = (k % bpr) * b + c[q, 0], (k // bpr) * b + c[q, 1]
            assert tri[y, x] == t
            assert uv[t, q, 0] == np.float32((x + 0.5) / size) and uv[t, q, 1] == np.float32(1.0 - (y + 0.5) / size)


def test_the_statement_on_a_closed_mesh_in_random_order():
    """A subdivided octahedron with its triangles shuffled and their corners rotated at random: the corner texel is the vertex, bit for bit; the texels along an edge are
    equal, bit for bit, in the two triangles that share it, whatever roles its ends have in each; all UV triangles turn the same way."""
    verts, tris = tr.octahedron(2)
    rng = np.random.default_rng(7)
    verts = (verts + rng.uniform(-0.01, 0.01, verts.shape)).astype(np.float32)
    tris = tris[rng.permutation(len(tris))]
    tris = np.stack([np.roll(t, rng.integers(3)) for t in tris])
    nt = len(tris)
    assert nt == 128
    for size, block in ((128, 0), (101, 7)):
        lay = tr.layout(nt, size, block)
        b, bpr = lay["block"], lay["blocks_per_row"]
        pos = tr.positions(verts, tris, size, b, bpr)
        tri, _ = tr.ownership(nt, size, b, bpr)
        assert np.array_equal(pos[..., 3] == 1, tri >= 0) and not pos[tri < 0].any()
        edges = {}
        for t in range(nt):
            for q in range(3):
                r, c = tr.edge_texels(size, b, bpr, t, q, (q + 1) % 3)
                assert (tri[r, c] == t).all()
                assert np.array_equal(pos[r[0], c[0], :3].view(np.uint32), verts[tris[t, q]].view(np.uint32))  # corner = vertex
                edges.setdefault((min(tris[t, q], tris[t, (q + 1) % 3]), max(tris[t, q], tris[t, (q + 1) % 3])), []).append((t, q))
        assert all(len(e) == 2 for e in edges.values())  # closed
        for (t0, q0), (t1, q1) in edges.values():
            r0, c0 = tr.edge_texels(size, b, bpr, t0, q0, (q0 + 1) % 3)
            r1, c1 = tr.edge_texels(size, b, bpr, t1, (q1 + 1) % 3, q1)  # the same edge, walked from the same vertex
            assert tris[t0, q0] == tris[t1, (q1 + 1) % 3]
            assert np.array_equal(pos[r0, c0].view(np.uint32), pos[r1, c1].view(np.uint32)), (t0, t1)
        uv = tr.uvs(nt, size, b, bpr).astype(np.float64)
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        area = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        assert (area < 0).all() or (area > 0).all()  # a half-turn keeps the orientation, a mirror image would flip every other one
        assert np.allclose(np.abs(area), ((b - 3) / size) ** 2)


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_texture_header_is_exported_by_the_hip_library():
    api, _abi = _built()
    from rnb_neus2_amd import build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})
    assert names == NAMES, names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_TEXTURE_PROTOTYPES) == set(names)
    others = [_abi.PROTOTYPES, _abi.RENDER_PROTOTYPES, _abi.MESH_PROTOTYPES, _abi.MESH_CLEAN_PROTOTYPES, _abi.MESH_SIMPLIFY_PROTOTYPES, _abi.MESH_DISTANCE_PROTOTYPES, _abi.MESH_RASTER_PROTOTYPES]
    assert not any(set(_abi.MESH_TEXTURE_PROTOTYPES) & set(t) for t in others)
    assert "mesh_texture" in inspect.signature(_abi.declare).parameters
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_abi_version() == 1 and fns.mesh_clean_abi_version() == 1 and fns.mesh_simplify_abi_version() == 1 \
        and fns.mesh_distance_abi_version() == 1 and fns.mesh_raster_abi_version() == 1  # as they were
    assert fns.mesh_texture_abi_version() == _abi.MESH_TEXTURE_ABI_VERSION == 1
    opt = _abi.MeshTextureOptions()
    opt.block, opt.maps, opt.reserved[1] = 9, 7, 5
    assert fns.mesh_texture_default_options(C.byref(opt)) == 0
    assert (opt.abi_version, opt.size, opt.block, opt.maps, opt.use_inference_params, opt.max_texels_in_flight, list(opt.reserved)) == (1, 1024, 0, _abi.MESH_TEXTURE_ALBEDO, 1, 0, [0] * 4)
    assert fns.mesh_texture_default_options(None) == _abi.ERR_INVALID
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_texture.cuh") in build.DEPS
    assert re.findall(r'#include\s+"([^"]+)"', open(HEADER).read()) == ["rnb_mesh.h"]


def test_texture_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = [("rnb_mesh_texture_options", _abi.MeshTextureOptions), ("rnb_mesh_texture", _abi.MeshTexture), ("rnb_mesh_texture_stats", _abi.MeshTextureStats)]
    consts = ["ABI_VERSION", "MIN_SIZE", "MAX_SIZE", "MIN_BLOCK", "MAX_IN_FLIGHT", "ALBEDO", "NORMAL", "POSITION"]
    body, want = "", []
    for cname, T in structs:
        fields = [n for n, _ in T._fields_]
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % cname + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, n) for n in fields)
        want += [C.sizeof(T)] + [getattr(T, n).offset for n in fields]
    body += "".join("  printf(\"%%llu\\n\", (unsigned long long)RNB_MESH_TEXTURE_%s);\n" % c for c in consts)
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_texture.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[:len(want)] == want
    assert out[len(want):] == [getattr(_abi, "MESH_TEXTURE_" + c) for c in consts]
    assert (tr.MIN_SIZE, tr.MAX_SIZE, tr.MIN_BLOCK) == (_abi.MESH_TEXTURE_MIN_SIZE, _abi.MESH_TEXTURE_MAX_SIZE, _abi.MESH_TEXTURE_MIN_BLOCK)
    assert list(_abi.MESH_TEXTURE_MAPS.items()) == [("albedo", 1), ("normal", 2), ("position", 4)]
    assert sorted(_abi.MeshTextureStats().as_dict()) == ["ms", "n_batches", "n_texels", "peak_workspace"]


def test_bake_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the device is touched: the context handed in here is a block of zeros, and no device exists where this test runs."""
    api, _abi = _built()
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good(**kw):
        o = _abi.MeshTextureOptions()
        assert fns.mesh_texture_default_options(C.byref(o)) == 0
        o.size = 64
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def mesh(nv=3, ni=3):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, 0x1000, 0x2000  # never dereferenced
        return m

    tex, st = _abi.MeshTexture(), _abi.MeshTextureStats()

    def refused(ctx_, m, o, needle=None):
        tex.uv, tex.size, st.n_batches = 0x4000, 9, 7
        rc = fns.mesh_bake_texture(ctx_, None, m, o, C.byref(tex), C.byref(st))
        assert (tex.uv, tex.size, st.n_batches) == (None, 0, 0)  # zeroed on failure
        return rc == _abi.ERR_INVALID and (needle is None or needle in fns.last_error())

    M = mesh()
    assert refused(None, C.byref(M), C.byref(good())) and refused(ctx, None, C.byref(good())) and refused(ctx, C.byref(M), None)
    assert fns.mesh_bake_texture(ctx, None, C.byref(M), C.byref(good()), None, None) == _abi.ERR_INVALID
    for kw in (dict(abi_version=0), dict(abi_version=2), dict(size=3), dict(size=8193), dict(size=0), dict(maps=0), dict(maps=8), dict(maps=0xFFFFFFFF), dict(block=3), dict(block=65)):
        assert refused(ctx, C.byref(M), C.byref(good(**kw))), kw
    o = good()
    o.reserved[3] = 1
    assert refused(ctx, C.byref(M), C.byref(o), b"reserved")
    assert refused(ctx, C.byref(mesh(3, 4)), C.byref(good()), b"multiple of 3")
    assert refused(ctx, C.byref(mesh(0, 3)), C.byref(good()), b"no vertices")
    m = mesh()
    m.verts = None
    assert refused(ctx, C.byref(m), C.byref(good()), b"null")
    assert refused(ctx, C.byref(mesh(9, 3 * 1000)), C.byref(good(size=64)), b"the smallest size that would fit is 92")  # capacity
    assert refused(ctx, C.byref(mesh(9, 3 * 9)), C.byref(good(size=64, block=32)), b"the smallest size that would fit is 96")
    assert fns.mesh_texture_free(None, C.byref(tex)) == _abi.ERR_INVALID and fns.mesh_texture_free(ctx, None) == _abi.ERR_INVALID
    assert fake.raw == b"\0" * 4096


# ------------------------------------------------------------------------------------------------------------------------ DeviceMesh.bake_texture on a stand-in
class FakeTextureLibrary:
    """Every entry point returns 0, except the `nth` call (from 0) of the one named `fail`, which returns ERR_INVALID. device_malloc and mesh_bake_texture hand out
    made-up pointers (the bake: uv and the maps the options ask for, for mesh.n_indices / 3 triangles); memcpy copies nothing (a download reads zeros). `log` holds the
    names in call order; `held` what is handed out and not yet released, `errors` every release of something that is not."""

    def __init__(self, fail=None, nth=0):
        self.fail, self.nth, self.log, self.held, self.errors, self._next, self._count = fail, nth, [], set(), [], 0x1000, {}

    def _ptr(self):
        self._next += 0x100
        self.held.add(self._next)
        return self._next

    def _release(self, ptr, name):
        if ptr in self.held:
            self.held.remove(ptr)
        else:
            self.errors.append((name, ptr))

    def last_error(self):
        return b"made to fail"

    def __getattr__(self, name):
        def call(*args):
            from rnb_neus2_amd import _abi
            obj = lambda k: args[k]._obj
            kind = name + ("_d2h" if name == "memcpy" and args[4] == _abi.D2H else "")
            k = self._count.get(kind, 0)
            self._count[kind] = k + 1
            self.log.append(kind)
            if kind == self.fail and k == self.nth:
                return _abi.ERR_INVALID
            if name == "create":
                obj(1).value = 0x10
            elif name == "device_malloc":
                obj(2).value = self._ptr()
            elif name == "device_free":
                self._release(args[1].value, name)
            elif kind == "memcpy_d2h":
                C.memset(args[1], 0, args[3])
            elif name == "mesh_texture_default_options":
                obj(0).abi_version, obj(0).maps, obj(0).use_inference_params = 1, 1, 1
            elif name == "mesh_bake_texture":
                m, o, t = obj(2), obj(3), obj(4)
                t.uv = self._ptr()
                for field, bit in _abi.MESH_TEXTURE_MAPS.items():
                    if o.maps & bit:
                        setattr(t, field, self._ptr())
                t.size, t.block, t.blocks_per_row, t.n_tris = o.size, 4, o.size // 4, m.n_indices // 3
                obj(5).n_batches = 1
            elif name == "mesh_texture_free":
                t = obj(1)
                for field in ("uv", "albedo", "normal", "position"):
                    if getattr(t, field):
                        self._release(getattr(t, field), name)
                C.memset(C.byref(t), 0, C.sizeof(t))
            return 0
        return call


V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
I = np.uint32([0, 1, 2, 0, 2, 3])
ALL = ("albedo", "normal", "position")


def _context(fail=None, nth=0):
    from rnb_neus2_amd import _abi, api
    fake = FakeTextureLibrary(fail, nth)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


def test_bake_texture_calls_in_order_and_releases_everything():
    c, fake = _context()
    out = c.bake_texture(V, I, 16, maps=ALL)
    assert fake.log == ["create"] + ["device_malloc", "memcpy"] * 2 + ["mesh_texture_default_options", "mesh_bake_texture"] + ["memcpy_d2h"] * 4 + ["mesh_texture_free"] + ["device_free"] * 2
    assert not fake.held and not fake.errors
    assert sorted(out) == sorted(ALL + ("uv", "block", "blocks_per_row", "stats"))
    assert out["uv"].shape == (2, 3, 2) and out["uv"].dtype == np.float32 and all(out[k].shape == (16, 16, 4) and out[k].dtype == np.float32 for k in ALL)
    assert (out["block"], out["blocks_per_row"], out["stats"]["n_batches"]) == (4, 4, 1)
    c, fake = _context()
    out = c.bake_texture(V, I, 8)  # the default: the albedo alone
    assert "albedo" in out and "normal" not in out and "position" not in out and fake.log.count("memcpy_d2h") == 2 and not fake.held and not fake.errors
    with pytest.raises(ValueError):
        c.bake_texture(V, I, 8, maps=("albedo", "depth"))


@pytest.mark.parametrize("fail, nth", [("mesh_bake_texture", 0)] + [("memcpy_d2h", k) for k in range(4)] + [("device_malloc", 1)])
def test_a_failing_step_of_bake_texture_leaves_nothing_allocated(fail, nth):
    from rnb_neus2_amd import _abi, api
    c, fake = _context(fail, nth)
    with pytest.raises(api.RnbError) as e:
        c.bake_texture(V, I, 16, maps=ALL)
    assert e.value.code == _abi.ERR_INVALID and fail in fake.log
    assert not fake.held and not fake.errors, (fake.held, fake.errors)
    assert fake.log.count("mesh_texture_free") == (1 if "mesh_bake_texture" in fake.log else 0)


def test_a_freed_handle_raises_before_any_call():
    c, fake = _context()
    m = c.upload_mesh(V, I)
    m.free()
    n = len(fake.log)
    with pytest.raises(ValueError):
        m.bake_texture(16)
    assert len(fake.log) == n and not fake.held and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ writers
def test_save_obj_textured_writes_obj_mtl_and_pngs(tmp_path):
    _built()
    from rnb_neus2_amd import hostlib, meshproc
    verts, tris = tr.octahedron(1)
    nt, size = len(tris), 32
    lay = tr.layout(nt, size)
    uv = tr.uvs(nt, size, lay["block"], lay["blocks_per_row"])
    rng = np.random.default_rng(3)
    albedo = rng.uniform(-0.2, 1.2, (size, size, 4)).astype(np.float32)
    albedo[0, :4, :3] = np.float32([[0.0, 1.0, 0.5], [0.6 / 255, 1.6 / 255, 254.6 / 255], [-1.0, 2.0, 0.25], [0.1, 0.2, 0.3]])
    normal = rng.uniform(-1.1, 1.1, (size, size, 4)).astype(np.float32)
    normal[1, :2, :3] = np.float32([[0.0, 1.0, -1.0], [0.5, -0.5, 2.0]])
    path = tmp_path / "out" / "baked.obj"
    os.makedirs(path.parent)
    meshproc.save_obj_textured(str(path), meshproc.Mesh(verts, tris), uv, dict(albedo=albedo, normal=normal, position=normal))
    assert sorted(os.listdir(path.parent)) == ["baked.mtl", "baked.obj", "baked_albedo.png", "baked_normal.png"]
    lines = open(path).read().splitlines()
    vt = [l for l in lines if l.startswith("vt ")]
    assert len(vt) == 3 * nt and "mtllib baked.mtl" in lines and "usemtl baked" in lines
    assert np.array_equal(np.float32([[float(x) for x in l.split()[1:]] for l in vt]).reshape(nt, 3, 2), uv)  # nine digits bring a float32 back
    faces = [l.split()[1:] for l in lines if l.startswith("f ")]
    assert len(faces) == nt
    for t, f in enumerate(faces):
        for corner, word in enumerate(f):
            a, tt, n = (int(x) for x in word.split("/"))
            assert (a, tt, n) == (tris[t, corner] + 1, 3 * t + corner + 1, tris[t, corner] + 1)
    mtl = open(path.parent / "baked.mtl").read()
    assert "map_Kd baked_albedo.png" in mtl and "baked_normal.png" in mtl and "newmtl baked" in mtl
    a8 = hostlib.png_read(str(path.parent / "baked_albedo.png"))
    n16 = hostlib.png_read(str(path.parent / "baked_normal.png"))
    assert a8.dtype == np.uint8 and a8.shape == (size, size, 3) and n16.dtype == np.uint16 and n16.shape == (size, size, 3)
    assert np.array_equal(a8, np.floor(255.0 * np.clip(albedo[..., :3].astype(np.float64), 0, 1) + 0.5).astype(np.uint8))
    assert np.array_equal(n16, np.floor(65535.0 * np.clip(normal[..., :3].astype(np.float64) * 0.5 + 0.5, 0, 1) + 0.5).astype(np.uint16))
    assert a8[0, :3].tolist() == [[0, 255, 128], [1, 2, 255], [0, 255, 64]] and n16[1, 0].tolist() == [32768, 65535, 0]
    # the albedo alone: no normal image, and the .mtl does not name one
    meshproc.save_obj_textured(str(tmp_path / "a.obj"), meshproc.Mesh(verts, tris), uv, dict(albedo=albedo))
    assert not os.path.exists(tmp_path / "a_normal.png") and "normal" not in open(tmp_path / "a.mtl").read()
    with pytest.raises(ValueError):
        meshproc.save_obj_textured(str(tmp_path / "b.obj"), meshproc.Mesh(verts, tris), uv[:-1], dict(albedo=albedo))


def test_the_host_writer_keeps_vt_with_its_corner(tmp_path):
    """mesh::save_obj_textured (host/mesh.hpp), compiled into a small program: with the faces as they are and reversed, corner q of triangle t names vt 3 t + q + 1, the
    .mtl names the images, and the PNGs hold the quantisation rule."""
    _built()
    from rnb_neus2_amd import hostlib
    src = tmp_path / "w.cpp"
    src.write_text('''#include "mesh.hpp"
#include "png16.hpp"
int main(int argc, char** argv) {
	mesh::Mesh m;
	m.verts = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
	m.colors = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}};
	m.indices = {0, 1, 2, 0, 2, 3};
	mesh::compute_normals(m);
	mesh::Texture t;
	t.size = 4;
	for (int k = 0; k < 12; ++k) t.uv.push_back((float)k / 16.0f);
	for (int p = 0; p < 16; ++p) for (int k = 0; k < 4; ++k) { t.albedo.push_back((float)(p * 4 + k) / 48.0f - 0.1f); t.normal.push_back((float)(p * 4 + k) / 30.0f - 1.05f); }
	const float off[3] = {0.5f, 0.5f, 0.5f}, tr[3] = {1.f, 2.f, 3.f};
	mesh::save_obj_textured(argv[1], m, t, png16::save, 0.5f, off, 2.0f, tr, argv[2][0] == '1');
	mesh::save_obj(std::string(argv[1]) + ".plain", m, 0.5f, off, 2.0f, tr, argv[2][0] == '1');
	return 0;
}
''')
    exe = tmp_path / "w"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rnb-neus2_amd", "host"), str(src), "-o", str(exe), "-lz"])
    idx = [[0, 1, 2], [0, 2, 3]]
    for as_they_are in (1, 0):
        out = tmp_path / ("m%d.obj" % as_they_are)
        subprocess.check_call([str(exe), str(out), str(as_they_are)])
        lines = open(out).read().splitlines()
        plain = open(str(out) + ".plain").read().splitlines()
        assert [l for l in lines if l.startswith(("v ", "vn "))] == [l for l in plain if l.startswith(("v ", "vn "))]  # the same transform
        assert [l.split()[1:] for l in lines if l.startswith("vt ")] == [["%.9g" % (k / 16.0), "%.9g" % ((k + 1) / 16.0)] for k in range(0, 12, 2)]
        faces = [l.split()[1:] for l in lines if l.startswith("f ")]
        plain_faces = [[w.split("/")[0] for w in l.split()[1:]] for l in plain if l.startswith("f ")]
        for t, f in enumerate(faces):
            order = [0, 1, 2] if as_they_are else [2, 1, 0]
            assert [w.split("/") for w in f] == [[str(idx[t][q] + 1), str(3 * t + q + 1), str(idx[t][q] + 1)] for q in order]
            assert [w.split("/")[0] for w in f] == plain_faces[t]  # the same reversal rule
        assert "map_Kd m%d_albedo.png" % as_they_are in open(tmp_path / ("m%d.mtl" % as_they_are)).read()
        a = np.float32([(p * 4 + k) / 48.0 for p in range(16) for k in range(4)]).reshape(4, 4, 4) - np.float32(0.1)
        n = np.float32([(p * 4 + k) / 30.0 for p in range(16) for k in range(4)]).reshape(4, 4, 4) - np.float32(1.05)
        assert np.array_equal(hostlib.png_read(str(tmp_path / ("m%d_albedo.png" % as_they_are))), np.floor(255.0 * np.clip(a[..., :3].astype(np.float64), 0, 1) + 0.5).astype(np.uint8))
        assert np.array_equal(hostlib.png_read(str(tmp_path / ("m%d_normal.png" % as_they_are))),
                              np.floor(65535.0 * np.clip(n[..., :3].astype(np.float64) * 0.5 + 0.5, 0, 1) + 0.5).astype(np.uint16))


# ------------------------------------------------------------------------------------------------------------------------ command line, pipeline
def test_mesh_cli_knows_the_texture_flags():
    _built()
    exe = os.path.join(ROOT, "build", "mesh")
    h = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert h.returncode == 0 and "--texture=[S]" in h.stdout and "--texture-maps=[LIST]" in h.stdout
    need = ["--snapshot", "missing.msgpack", "--scene", "missing", "--out", "x.obj"]
    for extra, word in ((["--texture", "0"], "'texture'"), (["--texture", "9000"], "'texture'"), (["--texture", "3"], "'texture'"), (["--texture", "x"], "'texture'"),
                        (["--texture-maps", "normal"], "only used with --texture"), (["--texture", "64", "--texture-maps", "albedo,depth"], "'texture-maps'"),
                        (["--texture", "64", "--texture-maps", ""], "'texture-maps'")):
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)
        assert r.returncode == 255 and word in r.stderr.splitlines()[0], (extra, r.returncode, r.stderr[:200])
    for extra in (["--texture", "4"], ["--texture", "8192", "--texture-maps", "albedo,normal"], ["--texture=64", "--texture-maps=normal"]):  # parsed: the next complaint is the missing snapshot
        r = subprocess.run([exe] + need + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, (extra, r.returncode, r.stderr[:200])


def test_plan_device_postprocess_with_and_without_texture():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    args = ("data", 1000, 256, "out/mesh.obj", "build/mesh")
    plain = pipeline.plan_device_postprocess(*args)
    assert pipeline.plan_device_postprocess(*args, texture=None) == plain
    assert pipeline.plan_device_postprocess(*args, texture=512) == plain + ["--texture", "512"]
    assert pipeline.plan_device_postprocess(*args, simplify=64, report_views=True, texture=2048) == pipeline.plan_device_postprocess(*args, simplify=64, report_views=True) + ["--texture", "2048"]
    for fn in (pipeline.plan_device_postprocess, pipeline.run_device_postprocess, pipeline.run_full_pipeline):
        assert inspect.signature(fn).parameters["texture"].default is None
    base = ["--input", "i", "--testbed", "build/testbed", "--output", "o"]
    p = run_pipeline.build_parser()
    assert run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess", "--texture", "512"]))["texture"] == 512
    assert "texture" not in run_pipeline.pipeline_kwargs(p.parse_args(base + ["--device-postprocess"])) and "texture" not in run_pipeline.pipeline_kwargs(p.parse_args(base))
    for bad in (base + ["--texture", "512"], base + ["--device-postprocess", "--texture", "3"], base + ["--device-postprocess", "--texture", "8193"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(bad)
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("i", "t", "o", texture=64)


def test_the_bench_tool_holds_no_private_plumbing():
    """The rule tests/test_device_mesh_cpu.py applies to the other mesh tools: the public mesh interface and mesh_bench_common only."""
    with open(os.path.join(ROOT, "tools", "bench_mesh_texture.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref", "_abi"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and "bake_texture" in text and "forward_infer_staged" in text
