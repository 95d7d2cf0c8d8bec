"""CPU tier of the mesh rasteriser (include/rnb_mesh_raster.h): the C-ABI of the new header (exports, version, defaults, struct layout, argument validation without a
device), the numpy statement of tests/mesh_raster_reference.py on hand-made cases, the view metrics in Python against host/view_metrics.hpp, and the planned command
line. No GPU needed."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import mesh_raster_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_raster.h")
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


@pytest.fixture(autouse=True, scope="module")
def _the_header_exists():
    """Every test here follows the rules as include/rnb_mesh_raster.h states them, the ones that need nothing but numpy too: none of them stands without it."""
    assert os.path.exists(HEADER), HEADER


def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


def axis_view(w, h, f):
    """A camera at the origin that looks along +z, x right, y down."""
    return dict(width=w, height=h, focal_length=(f, f), principal_point=(0.5, 0.5), xform=IDENTITY.copy())


def fibonacci_view(k, n, w, h, f, radius=1.6):
    from rnb_neus2_amd import synthetic
    centre = np.array([0.5, 0.5, 0.5])
    return dict(width=w, height=h, focal_length=(f, f), principal_point=(0.5, 0.5),
                xform=synthetic.look_at_c2w(centre + radius * synthetic.fibonacci_sphere(n)[k], centre).astype(np.float32))


def plane_on_pixel_centres(n=24, z=2.0, seed=3):
    """n x n quads at depth z whose vertices all project onto pixel centres of a 64 x 64 image (focal length 32: sx = 8.5 + 2 k), two triangles each, the diagonal
    alternating and every winding drawn at random. Returns verts, indices, the view."""
    g = np.arange(n + 1)
    xs, ys = np.meshgrid(g, g, indexing="xy")
    sx, sy = 8.5 + 2 * xs, 8.5 + 2 * ys
    v = np.stack([(sx - 32) * z / 32.0, (sy - 32) * z / 32.0, np.full(sx.shape, z)], -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(seed)
    tris = []
    for y in range(n):
        for x in range(n):
            a, b, c, d = y * (n + 1) + x, y * (n + 1) + x + 1, (y + 1) * (n + 1) + x + 1, (y + 1) * (n + 1) + x
            for tr in ([[a, b, c], [a, c, d]] if (x + y) % 2 else [[a, b, d], [b, c, d]]):
                tris.append([tr[0], tr[2], tr[1]] if rng.integers(2) else tr)
    return v, np.array(tris, np.uint32).ravel(), axis_view(64, 64, 32.0)


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_raster_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi, build
    names = _functions(HEADER)
    assert names == ["rnb_mesh_raster", "rnb_mesh_raster_abi_version", "rnb_mesh_raster_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_RASTER_PROTOTYPES) == set(names)
    assert not set(_abi.MESH_RASTER_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.RENDER_PROTOTYPES) | set(_abi.MESH_PROTOTYPES) | set(_abi.MESH_CLEAN_PROTOTYPES)
                                                   | set(_abi.MESH_SIMPLIFY_PROTOTYPES) | set(_abi.MESH_DISTANCE_PROTOTYPES))
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_abi_version() == 1 and fns.mesh_clean_abi_version() == 1 and fns.mesh_simplify_abi_version() == 1 \
        and fns.mesh_distance_abi_version() == 1  # as they were
    assert fns.mesh_raster_abi_version() == _abi.MESH_RASTER_ABI_VERSION == 1
    opt = _abi.MeshRasterOptions()
    opt.cull, opt.normals, opt.reserved[2] = 2, 1, 5
    assert fns.mesh_raster_default_options(C.byref(opt)) == 0
    assert (opt.abi_version, opt.near, opt.cull, opt.normals, list(opt.reserved)) == (1, 2.0 ** -10, _abi.MESH_RASTER_CULL_NONE, _abi.MESH_RASTER_NORMALS_FACE, [0] * 4)
    assert fns.mesh_raster_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.Context, "rasterize_mesh") and hasattr(api.Context, "mesh_view_metrics")
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS and os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_raster.cuh") in build.DEPS
    assert os.path.join(ROOT, "rnb-neus2_amd", "host", "view_metrics.hpp") in build.MESH_DEPS and os.path.join(ROOT, "rnb-neus2_amd", "host", "view_metrics.hpp") in build.RENDER_DEPS
    text = open(HEADER).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["rnb_mesh.h"]
    for other in ("clean.h", "simplify.h", "distance.h", "render.h"):  # it names no other stage's header ...
        assert other not in text, other
    for name in os.listdir(os.path.join(ROOT, "include")):  # ... and no other header mentions this one
        assert name == "rnb_mesh_raster.h" or "raster.h" not in open(os.path.join(ROOT, "include", name)).read()


def test_raster_validates_its_arguments_without_a_device():
    """Every refusal the header lists as made before the context or the device is touched: the context handed in here is a block of zeros, and no device exists where
    this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good():
        o = _abi.MeshRasterOptions()
        assert fns.mesh_raster_default_options(C.byref(o)) == 0
        return o

    def view(**kw):
        d = axis_view(8, 6, 10.0)
        d.update(kw)
        return api._view_struct(d)

    def mesh(nv=3, ni=3):
        m = _abi.Mesh()
        m.n_verts, m.n_indices, m.verts, m.indices = nv, ni, 0x1000, 0x2000  # never dereferenced
        return m

    def call(ctx_, m, v, o, out=0x3000, faces=None, stats=None):
        return fns.mesh_raster(ctx_, None, m, v, o, out, faces, stats)

    M, V = mesh(), view()
    assert call(None, C.byref(M), C.byref(V), C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, None, C.byref(V), C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), None, C.byref(good())) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), C.byref(V), None) == _abi.ERR_INVALID
    assert call(ctx, C.byref(M), C.byref(V), C.byref(good()), out=None) == _abi.ERR_INVALID and b"null" in fns.last_error()
    assert call(ctx, C.byref(M), C.byref(V), C.byref(good()), out=0x3000, faces=0x3000) == _abi.ERR_INVALID and b"different" in fns.last_error()
    nan, inf = float("nan"), float("inf")
    st = _abi.MeshRasterStats()
    for field, value in [("abi_version", 2), ("abi_version", 0), ("near", 0.0), ("near", -1.0), ("near", nan), ("near", inf), ("cull", 3), ("cull", 0xFFFFFFFF), ("normals", 2)]:
        o = good()
        setattr(o, field, value)
        st.n_tris = 7
        assert call(ctx, C.byref(M), C.byref(V), C.byref(o), stats=C.byref(st)) == _abi.ERR_INVALID, (field, value)
        assert st.n_tris == 0 and fns.last_error()  # zeroed on failure
    bad_x = IDENTITY.copy()
    bad_x[1, 3] = nan
    for kw in (dict(focal_length=(0.0, 10.0)), dict(focal_length=(10.0, -1.0)), dict(focal_length=(nan, 10.0)), dict(focal_length=(10.0, inf)), dict(principal_point=(nan, 0.5)),
               dict(principal_point=(0.5, inf)), dict(xform=bad_x), dict(width=0), dict(height=0), dict(width=16385), dict(height=16385)):
        assert call(ctx, C.byref(M), C.byref(view(**kw)), C.byref(good())) == _abi.ERR_INVALID, kw
    assert b"16384" in fns.last_error()
    m = mesh(3, 4)
    assert call(ctx, C.byref(m), C.byref(V), C.byref(good())) == _abi.ERR_INVALID and b"multiple of 3" in fns.last_error()
    m = mesh(0, 3)
    assert call(ctx, C.byref(m), C.byref(V), C.byref(good())) == _abi.ERR_INVALID and b"no vertices" in fns.last_error()
    m = mesh()
    m.indices = None
    assert call(ctx, C.byref(m), C.byref(V), C.byref(good())) == _abi.ERR_INVALID and b"null" in fns.last_error()
    o = good()
    o.normals = _abi.MESH_RASTER_NORMALS_VERTEX
    assert call(ctx, C.byref(M), C.byref(V), C.byref(o)) == _abi.ERR_INVALID and b"normals" in fns.last_error()  # VERTEX without normals
    assert fake.raw == b"\0" * 4096


def test_raster_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    O, S = _abi.MeshRasterOptions, _abi.MeshRasterStats
    of = [n for n, _ in O._fields_]
    sf = [n for n, _ in S._fields_]
    src = tmp_path / "layout.c"
    consts = ["ABI_VERSION", "CHANNELS", "NONE", "MAX_SIZE", "SUBPIXEL_BITS", "MAX_COORD_LOG2", "SMALL_PIXELS", "MAX_COUNT", "CULL_NONE", "CULL_BACK", "CULL_FRONT", "NORMALS_FACE",
              "NORMALS_VERTEX"]
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"rnb_mesh_raster.h\"\nint main(void) {\n"
                   + "  printf(\"%zu\\n\", sizeof(rnb_mesh_raster_options));\n" + "".join("  printf(\"%%zu\\n\", offsetof(rnb_mesh_raster_options, %s));\n" % n for n in of)
                   + "  printf(\"%zu\\n\", sizeof(rnb_mesh_raster_stats));\n" + "".join("  printf(\"%%zu\\n\", offsetof(rnb_mesh_raster_stats, %s));\n" % n for n in sf)
                   + "".join("  printf(\"%%llu\\n\", (unsigned long long)RNB_MESH_RASTER_%s);\n" % c for c in consts) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    want = [C.sizeof(O)] + [getattr(O, n).offset for n in of] + [C.sizeof(S)] + [getattr(S, n).offset for n in sf]
    assert out[:len(want)] == want
    assert out[len(want):] == [getattr(_abi, "MESH_RASTER_" + c) for c in consts]
    assert (rr.CHANNELS, rr.NONE, rr.MAX_SIZE, rr.SMALL_PIXELS, rr.MAX_COUNT, rr.MAX_COORD_LOG2) == (_abi.MESH_RASTER_CHANNELS, _abi.MESH_RASTER_NONE, _abi.MESH_RASTER_MAX_SIZE,
                                                                                                   _abi.MESH_RASTER_SMALL_PIXELS, _abi.MESH_RASTER_MAX_COUNT, _abi.MESH_RASTER_MAX_COORD_LOG2)
    assert _abi.MESH_RASTER_CHANNELS == 9  # the render's layout
    assert sorted(S().as_dict()) == sorted(["n_tris", "n_behind", "n_out_of_range", "n_degenerate", "n_culled", "n_offscreen", "n_small", "n_large", "n_covered", "n_back_pixels",
                                            "n_fragments", "peak_workspace", "ms"])


# ------------------------------------------------------------------------------------------------------------------------ the statement on hand-made cases
def test_one_triangle_against_exact_rationals():
    """Coverage of a single triangle against a brute-force point-in-triangle test in exact rationals on the snapped vertices, with the tie rule of rule 4 on the edges;
    both windings cover the same pixels."""
    v = np.array([(-0.61, -0.37, 2.0), (0.83, -0.11, 2.5), (0.0625, 0.8125, 3.0)], np.float32)  # the last vertex lands on a pixel centre: (32 + 24 * 0.0625 / 3, 24 + 24 * 0.8125 / 3) = (32.5, 30.5)
    view = axis_view(64, 48, 24.0)
    for order in ([0, 1, 2], [0, 2, 1]):
        r = rr.rasterize(v, np.array(order, np.uint32), view)
        s = rr.setup(v, np.array(order, np.uint32), view)
        assert s["cls"].tolist() == [6] and bool(s["back"][0]) == (order == [0, 1, 2])
        X, Y = [Fraction(int(x), 256) for x in s["X"][0]], [Fraction(int(y), 256) for y in s["Y"][0]]

        def inside(px, py):
            ok = True
            for k in range(3):
                p, q = (k + 1) % 3, (k + 2) % 3
                dx, dy = X[q] - X[p], Y[q] - Y[p]
                e = dx * (py - Y[p]) - dy * (px - X[p])
                ok = ok and (e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dx > 0))))
            return ok

        assert (X[2], Y[2]) == (Fraction(65, 2), Fraction(61, 2))
        want = np.array([[inside(Fraction(2 * i + 1, 2), Fraction(2 * j + 1, 2)) for i in range(64)] for j in range(48)])
        assert want.sum() > 40
        assert np.array_equal(r["counts"] == 1, want) and np.array_equal(r["image"][..., 6] == 1, want) and r["counts"].max() == 1
        assert r["stats"]["n_back_pixels"] == (want.sum() if order == [0, 1, 2] else 0)
        assert np.all(r["faces"][want] == 0) and np.all(r["faces"][~want] == rr.NONE) and not r["image"][~want].any()


def test_a_plane_of_mixed_windings_covers_every_pixel_once():
    v, idx, view = plane_on_pixel_centres()
    r = rr.rasterize(v, idx, view)
    c = r["counts"]
    assert c.sum() == 48 * 48 and set(np.unique(c)) == {0, 1}  # 24 x 24 quads of 2 x 2 pixels; every vertex and every edge runs through pixel centres
    rows, cols = np.nonzero(c.any(1))[0], np.nonzero(c.any(0))[0]
    assert len(rows) == 48 and len(cols) == 48 and np.all(c[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] == 1)
    assert r["stats"]["n_small"] == 1152 and r["stats"]["n_large"] == 0 and 0 < r["stats"]["n_back_pixels"] < 48 * 48
    # depth of a plane z = const: that constant's float at every covered pixel
    assert np.all(r["image"][..., 7][c == 1].view(np.uint32) == np.float32(2.0).view(np.uint32)) and not r["image"][c == 0].any()
    for z in (0.7, 3.1, 1e-2):
        v2, idx2, view2 = plane_on_pixel_centres(n=6, z=z)
        r2 = rr.rasterize(v2, idx2, view2)
        assert r2["stats"]["n_covered"] >= 100
        assert np.all(r2["image"][..., 7][r2["counts"] > 0].view(np.uint32) == np.float32(z).view(np.uint32)), z


@functools.lru_cache(maxsize=None)
def spheres_outward():
    from tests import mesh_clean_reference as cr
    v, i = cr.three_spheres(32)
    t = i.reshape(-1, 3)
    p = v.astype(np.float64)
    assert np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() > 0  # turned outward as it comes
    return v, i


def test_three_spheres_have_even_counts_and_the_sign_convention():
    v, i = spheres_outward()
    inward = i.reshape(-1, 3)[:, [0, 2, 1]].ravel()  # `reverse` on all three spheres
    for k in range(3):
        view = fibonacci_view(k, 3, 96, 96, 150.0)
        r = rr.rasterize(v, i, view)
        assert r["stats"]["n_covered"] > 1000 and not (r["counts"] & 1).any() and r["stats"]["n_back_pixels"] == 0
        assert r["stats"]["n_fragments"] == int(r["counts"].sum()) == int(r["image"][..., 8].sum())
        q = rr.rasterize(v, inward, view)
        assert q["stats"]["n_back_pixels"] == q["stats"]["n_covered"] == r["stats"]["n_covered"]
        assert np.array_equal(q["counts"], r["counts"]) and np.array_equal(q["image"][..., 6:9], r["image"][..., 6:9]) and np.array_equal(q["faces"], r["faces"])
        assert np.array_equal(q["image"][..., 0:3], -r["image"][..., 0:3])
        # the face normal of an outward sphere looks at the camera: dot(n, p - o) < 0 at every covered pixel
        o = np.asarray(view["xform"], np.float64)[:, 3]
        cov = r["image"][..., 6] == 1
        centre = v[i.reshape(-1, 3)[r["faces"][cov]]].mean(axis=1).astype(np.float64)
        assert np.all(np.einsum("ij,ij->i", r["image"][..., 0:3][cov].astype(np.float64), centre - o) < 0)
        # cull back / front partition the fragments of cull none
        b, f = rr.rasterize(v, i, view, cull="back"), rr.rasterize(v, i, view, cull="front")
        assert np.array_equal(b["counts"] + f["counts"], r["counts"]) and b["counts"].any() and f["counts"].any()
        assert b["stats"]["n_culled"] + f["stats"]["n_culled"] == r["stats"]["n_small"] + r["stats"]["n_large"] + r["stats"]["n_offscreen"]
        assert b["stats"]["n_back_pixels"] == 0 and f["stats"]["n_back_pixels"] == f["stats"]["n_covered"]
        assert np.array_equal(b["image"][..., :8], r["image"][..., :8]) and np.array_equal(b["faces"], r["faces"])  # seen from outside, the front faces are all one sees


def test_a_tilted_plane_against_the_analytic_depth():
    """The plane z = z0 + s * x seen along +z: the ray through pixel centre (i + 0.5, j + 0.5) has x = u * z with u = (i + 0.5 - cx W) / f, so z = z0 / (1 - s u).
    Bound: the vertices are snapped by at most 1/512 pixel in x and y, which moves the surface a ray meets, in depth, by at most |dz/du| * (1/512) / f per vertex shift;
    the interpolation of 1/z between shifted vertices is exact for a plane, so the error is that of the shifted plane. |dz/du| = z0 s / (1 - s u)^2 = s z^2 / z0. A shift
    of all three vertices by up to 1/512 pixel each can tilt the plane as well: over a triangle that spans L pixels the tilt adds at most 2 / (512 L) relative to the
    pixel offset within the triangle, i.e. at most another 2/512 pixel of equivalent shift. Allowed: 3/512 pixel of shift plus float rounding of the stored depth."""
    z0, s, f, W, H = 2.0, 0.6, 40.0, 48, 40
    xs = np.array([-0.9, 1.1])
    ys = np.array([-0.8, 0.7])
    v = np.array([(x, y, z0 + s * x) for y in ys for x in xs], np.float32)
    idx = np.array([0, 1, 3, 0, 3, 2], np.uint32)
    view = axis_view(W, H, f)
    r = rr.rasterize(v, idx, view)
    cov = r["counts"] > 0
    assert cov.sum() > 500 and r["counts"].max() == 1
    jj, ii = np.nonzero(cov)
    u = (ii + 0.5 - 0.5 * W) / f
    want = z0 / (1.0 - s * u)
    got = r["image"][..., 7][cov].astype(np.float64)
    slope = s * want ** 2 / z0  # |dz/du|
    bound = slope * (3.0 / 512.0) / f + np.spacing(np.float32(want.max())) + 4e-7 * want  # (the float vertices z0 + s * x are themselves rounded: 2^-23 relative twice)
    err = np.abs(got - want)
    print("tilted plane: max error %.3g, bound at that pixel %.3g" % (err.max(), bound[err.argmax()]))
    assert np.all(err <= bound)


def test_skipped_triangles_are_counted_and_draw_nothing():
    view = axis_view(32, 32, 16.0)
    tri = np.array([(-0.5, -0.5, 2.0), (0.5, -0.5, 2.0), (0.0, 0.5, 2.0)], np.float32)
    idx = np.array([0, 1, 2], np.uint32)
    assert rr.rasterize(tri, idx, view)["stats"]["n_covered"] > 20
    behind = tri.copy()
    behind[2, 2] = 2.0 ** -11  # nearer than near = 2^-10
    r = rr.rasterize(behind, idx, view)
    assert (r["stats"]["n_behind"], r["stats"]["n_covered"], r["stats"]["n_fragments"]) == (1, 0, 0) and not r["image"].any() and np.all(r["faces"] == rr.NONE)
    assert rr.rasterize(behind, idx, view, near=2.0 ** -12)["stats"]["n_behind"] == 0
    on_near = tri.copy()
    on_near[:, 2] = 2.0 ** -10  # zc == near is in front
    assert rr.rasterize(on_near * np.float32([2.0 ** -11, 2.0 ** -11, 1]), idx, view)["stats"]["n_behind"] == 0
    far = tri.copy()
    far[1, 0] = 2.0 ** 22  # sx = 16 * 2^22 / 2 * 256 > 2^28
    r = rr.rasterize(far, idx, view)
    assert (r["stats"]["n_out_of_range"], r["stats"]["n_covered"]) == (1, 0) and not r["image"].any()
    edge = tri.copy()
    edge[1, 0] = (2.0 ** 20 - 16) / 16 * 2  # X = 2^28 exactly: still in range
    assert rr.rasterize(edge, idx, view)["stats"]["n_out_of_range"] == 0
    nonfinite = tri.copy()
    for bad in (np.inf, -np.inf, np.nan):  # a coordinate that is not finite: behind (0 * inf in zc) or out of range, never drawn
        for k in range(3):
            nonfinite[0] = tri[0]
            nonfinite[0, k] = bad
            st = rr.rasterize(nonfinite, idx, view)["stats"]
            assert st["n_behind"] + st["n_out_of_range"] == 1 and st["n_covered"] == 0, (bad, k)
    assert rr.rasterize(tri, np.array([0, 1, 1], np.uint32), view)["stats"]["n_degenerate"] == 1
    assert rr.rasterize(tri + np.float32([40, 0, 0]), idx, view)["stats"]["n_offscreen"] == 1
    tiny = tri * np.float32([1e-3, 1e-3, 1]) + np.float32([0.01, 0.01, 0])  # between pixel centres: a box without a centre
    assert rr.rasterize(tiny, idx, view)["stats"]["n_offscreen"] == 1
    e = rr.rasterize(np.zeros((4, 3), np.float32), np.zeros(0, np.uint32), view)  # an empty mesh: an empty image
    assert e["stats"]["n_tris"] == 0 and not e["image"].any() and np.all(e["faces"] == rr.NONE)
    both = rr.rasterize(np.concatenate([tri, behind]), np.array([0, 1, 2, 3, 4, 5], np.uint32), view)  # the skipped one leaves the other as it was
    assert both["stats"]["n_behind"] == 1 and np.array_equal(both["image"], rr.rasterize(tri, idx, view)["image"])


def test_duplicates_permutations_and_renumbering():
    v, i = spheres_outward()
    view = fibonacci_view(1, 3, 96, 72, 140.0)
    r = rr.rasterize(v, i, view)
    t = i.reshape(-1, 3)
    twice = rr.rasterize(v, np.concatenate([t, t]).ravel(), view)  # every triangle again: the lowest index wins, the counts double
    assert np.array_equal(twice["faces"], r["faces"]) and np.array_equal(twice["counts"], 2 * r["counts"]) and np.array_equal(twice["image"][..., :8], r["image"][..., :8])
    assert np.all(twice["ties"][r["counts"] > 0] >= 2)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(t))
    p = rr.rasterize(v, t[perm].ravel(), view)
    assert np.array_equal(p["image"][..., 6:9], r["image"][..., 6:9]) and p["stats"] == r["stats"]
    free = r["ties"] <= 1
    assert np.array_equal(p["image"][free], r["image"][free]) and np.array_equal(perm[p["faces"][free & (r["counts"] > 0)]], r["faces"][free & (r["counts"] > 0)])
    ren = rng.permutation(len(v))
    inv = np.empty_like(ren)
    inv[ren] = np.arange(len(v))
    q = rr.rasterize(v[ren], inv[t].astype(np.uint32).ravel(), view)
    assert np.array_equal(q["image"], r["image"]) and np.array_equal(q["faces"], r["faces"]) and q["stats"] == r["stats"]
    # vertex shading and colours follow their vertices
    col = rng.uniform(0, 1, v.shape).astype(np.float32)
    nrm = (v - v.mean(0)).astype(np.float32)
    a = rr.rasterize(v, i, view, colors=col, normals=nrm, shading="vertex")
    b = rr.rasterize(v[ren], inv[t].astype(np.uint32).ravel(), view, colors=col[ren], normals=nrm[ren], shading="vertex")
    assert np.array_equal(a["image"], b["image"])
    cov = a["image"][..., 6] == 1
    assert np.abs(np.linalg.norm(a["image"][..., 0:3][cov].astype(np.float64), axis=1) - 1).max() < 1e-6 and np.array_equal(a["image"][..., 6:9], r["image"][..., 6:9])
    assert a["image"][..., 3:6][cov].min() >= 0 and a["image"][..., 3:6][cov].max() <= 1 and np.all(r["image"][..., 3:6][cov] == 1)


# ------------------------------------------------------------------------------------------------------------------------ the view metrics
def test_view_normal_metrics_equal_the_host_header(tmp_path):
    from rnb_neus2_amd import api, synthetic
    rng = np.random.default_rng(17)
    w, h, iw, ih = 37, 29, 74, 58  # the input map at twice the size: the pixel lookup of the header
    view = fibonacci_view(2, 5, w, h, 50.0)
    img = np.zeros((h, w, 9), np.float32)
    n = rng.normal(size=(h, w, 3))
    img[..., 0:3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    img[..., 6] = (rng.uniform(size=(h, w)) > 0.3).astype(np.float32)
    img[3, 4, 0:3] = 0  # a masked pixel with a zero normal: not compared
    img[3, 4, 6] = 1
    nm = np.zeros((ih, iw, 4), np.uint16)
    nm[..., :3] = rng.integers(0, 65536, (ih, iw, 3))
    nm[..., 3] = np.where(rng.uniform(size=(ih, iw)) > 0.4, 65535, 0)
    got = api.view_normal_metrics(img, view, nm)
    src = tmp_path / "vm.cpp"
    src.write_text('#include "view_metrics.hpp"\n#include <cstdio>\n#include <vector>\nint main(int argc, char** argv) {\n'
                   '  unsigned w, h, iw, ih; float x[12];\n  std::FILE* f = std::fopen(argv[1], "rb");\n  if (!f || std::fscanf(f, "%u %u %u %u", &w, &h, &iw, &ih) != 4) return 1;\n'
                   '  std::fgetc(f);\n  if (std::fread(x, 4, 12, f) != 12) return 1;\n  std::vector<float> img((size_t)w * h * 9); std::vector<uint16_t> in((size_t)iw * ih * 4);\n'
                   '  if (std::fread(img.data(), 4, img.size(), f) != img.size() || std::fread(in.data(), 2, in.size(), f) != in.size()) return 1;\n'
                   '  const view_metrics::Result r = view_metrics::compare(img.data(), 9, w, h, x, in.data(), iw, ih);\n'
                   '  std::printf("%.17g %.17g %.17g %zu\\n{%s}\\n", r.mean_angle_deg, r.median_angle_deg, r.mask_iou, r.pixels_compared, view_metrics::json_fields(r).c_str());\n  return 0;\n}\n')
    exe = tmp_path / "vm"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "rnb-neus2_amd", "host"), str(src), "-o", str(exe)])
    data = tmp_path / "vm.bin"
    with open(data, "wb") as f:
        f.write(b"%d %d %d %d\n" % (w, h, iw, ih))
        f.write(np.asarray(view["xform"], np.float32).tobytes() + img.tobytes() + nm.tobytes())
    lines = subprocess.check_output([str(exe), str(data)]).decode().splitlines()
    mean, median, iou, k = lines[0].split()
    assert got["pixels_compared"] == int(k) > 300 and got["mask_iou"] == float(iou)
    # acos and the square roots are the platform's libm on both sides, numpy's may differ from it in the last place: 1e-12 degrees relative is far below any digit reported
    assert abs(got["mean_angle_deg"] - float(mean)) <= 1e-12 * float(mean) and abs(got["median_angle_deg"] - float(median)) <= 1e-12 * float(median)
    assert 60 < got["mean_angle_deg"] < 120  # random normals: about 90 degrees
    assert sorted(json.loads(lines[1])) == ["mask_iou", "mean_angle_deg", "median_angle_deg", "pixels_compared"]  # the fields of render_metrics.json
    # the number nobody can compare: empty masks
    empty = api.view_normal_metrics(np.zeros((h, w, 9), np.float32), view, np.zeros((ih, iw, 4), np.uint16))
    assert empty == dict(mean_angle_deg=0.0, median_angle_deg=0.0, mask_iou=1.0, pixels_compared=0)
    # a sphere's input map against the map itself, decoded: zero angle up to the 16-bit quantisation, IoU 1
    views, normals, _ = synthetic.make_scene(2, 48, 84.0)
    t = normals[0].astype(np.float64)
    ncam = (t[..., :3] / 65535.0 * 2.0 - 1.0) * np.array([1.0, -1.0, -1.0])
    world = ncam @ np.asarray(views[0]["xform"], np.float64)[:, :3].T
    self_img = np.zeros((48, 48, 9), np.float32)
    self_img[..., 0:3] = world
    self_img[..., 6] = t[..., 3] > 0
    same = api.view_normal_metrics(self_img, views[0], normals[0])
    assert same["mask_iou"] == 1.0 and same["pixels_compared"] == int((t[..., 3] > 0).sum()) > 100 and same["mean_angle_deg"] < 0.05


# ------------------------------------------------------------------------------------------------------------------------ the pipeline's command line
def test_plan_device_postprocess_with_and_without_report_views():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    args = ("/d/prepared_data", 10000, 1024, "/out/mesh.obj", "/b/build/mesh")
    today = ["/b/build/mesh", "--snapshot", pipeline.snapshot_candidates("/d/prepared_data", 10000)[0], "--scene", "/d/prepared_data", "--out", "/out/mesh.obj", "--resolution", "1024",
             "--keep", "largest", "--orient", "outward"]
    assert pipeline.plan_device_postprocess(*args) == today == pipeline.plan_device_postprocess(*args, report_views=False)
    assert pipeline.plan_device_postprocess(*args, report_views=True) == today + ["--report-views"]
    assert pipeline.plan_device_postprocess(*args, simplify=256, report_views=True) == today + ["--simplify", "256", "--report-views"]
    with open(os.path.join(ROOT, "tests", "golden", "pipeline_argv.json")) as f:
        assert "--report-views" not in f.read()  # the reference's command lines know nothing of it: the default path is theirs
    base = ["--input", "in", "--testbed", "/b/build/testbed", "--output", "out"]
    parser = run_pipeline.build_parser()
    assert "report_views" not in run_pipeline.pipeline_kwargs(parser.parse_args(base))
    assert "report_views" not in run_pipeline.pipeline_kwargs(parser.parse_args(base + ["--device-postprocess"]))
    kw = run_pipeline.pipeline_kwargs(parser.parse_args(base + ["--device-postprocess", "--report-views"]))
    assert kw["device_postprocess"] is True and kw["report_views"] is True
    with pytest.raises(SystemExit):
        run_pipeline.main(base + ["--report-views"])
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "/b/build/testbed", "out", report_views=True)
