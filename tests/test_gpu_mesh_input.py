"""The input checks every mesh stage shares (check_mesh_input and the index check of the drivers' call scope), on one tetrahedron (4 vertices, 4 triangles), for the
entries with an output mesh (clean, simplify, visibility_select), those without (raster, draw_textured, visibility, bake_texture, project_views) and distance with the
bad mesh as `from` and as `to`: an index equal to n_verts, an index of 0xFFFFFFFF, n_indices = 11, n_verts = 0 with indices present and, where there is an output mesh,
in == out. Each returns ERR_INVALID with its text and the entry's name in last_error, leaves what the entry zeroes on entry zeroed (the output mesh, texture or
projection, the statistics; in == out: the call returns before it touches the object, which is the input) and the input as it was; the next valid call on the same
context gives the bits of that stage's numpy statement. Views are 8 x 8, the atlas 8 texels per side."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_distance_reference as dr
from tests import mesh_draw_reference as dw
from tests import mesh_project_reference as pr
from tests import mesh_raster_reference as rr
from tests import mesh_simplify_reference as sr
from tests import mesh_texture_reference as tr
from tests import mesh_visibility_reference as vr

pytestmark = pytest.mark.gpu

TETRA_V = np.array([(0.3, 0.4, 0.2), (1.6, 0.3, 0.4), (0.4, 1.7, 0.6), (1.3, 1.4, 1.8)], np.float32)  # one corner per cell of GRID
TETRA_T = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2], np.uint32)
GRID = dict(origin=(0.0, 0.0, 0.0), cell=1.0, dims=2)
SIZE = 8  # the atlas: 4 triangles in 2 x 2 blocks of 4 texels
#        name: (index to overwrite, its value, n_verts, n_indices, in == out, text in last_error)
CASES = {"index_equals_n_verts": (7, 4, 4, 12, False, b"out of range"),
         "index_all_ones": (4, 0xFFFFFFFF, 4, 12, False, b"out of range"),
         "eleven_indices": (None, None, 4, 11, False, b"not a multiple of 3"),
         "in_is_out": (None, None, 4, 12, True, b"different objects"),
         "no_vertices": (None, None, 0, 12, False, b"out of range")}
WITH_OUT = ("clean", "simplify", "visibility_select")
ENTRIES = WITH_OUT + ("raster", "draw_textured", "visibility", "bake_texture", "project_views", "distance_from", "distance_to")
NAMES = dict(raster=b"rnb_mesh_raster", distance_from=b"rnb_mesh_distance", distance_to=b"rnb_mesh_distance")  # the others: rnb_mesh_<entry>


def _view():
    from rnb_neus2_amd import synthetic
    eye, target = np.array([1.1, 0.8, 5.0]), np.array([0.9, 0.9, 0.8])
    return dict(width=8, height=8, focal_length=(9.0, 9.5), principal_point=(0.5, 0.45), xform=synthetic.look_at_c2w(eye, target).astype(np.float32))


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
    c.init_params()
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    """The view, the texture and the image the entries that need them are given, and the statement of every entry on the valid tetrahedron."""
    rng = np.random.default_rng(3)
    view = _view()
    lay = tr.layout(4, SIZE)
    uv = tr.uvs(4, SIZE, lay["block"], lay["blocks_per_row"])
    color = rng.uniform(0, 1, (SIZE, SIZE, 4)).astype(np.float32)
    image = rng.uniform(0.2, 1, (8, 8, 4)).astype(np.float32)
    records, vis_stats = vr.measure(TETRA_V, TETRA_T, [view])
    kept, sel_stats = vr.select(4, TETRA_T, records)
    want = dict(clean=mc.expected(TETRA_V, TETRA_T), simplify=sr.expected(TETRA_V, TETRA_T, **GRID),
                raster=rr.rasterize(TETRA_V, TETRA_T, view), draw_textured=dw.draw(TETRA_V, TETRA_T, view, uv, color),
                visibility=(records, vis_stats), visibility_select=(kept, sel_stats, vr.compact(TETRA_V, TETRA_T, kept)),
                bake_texture=(lay, uv, tr.positions(TETRA_V, TETRA_T.reshape(-1, 3), SIZE, lay["block"], lay["blocks_per_row"])),
                project_views=pr.project(TETRA_V, TETRA_T.reshape(-1, 3), [view], [image], SIZE),
                distance=dr.expected(TETRA_V, TETRA_T, TETRA_V, TETRA_T))
    return dict(view=view, uv=uv, color=color, image=image, want=want)


def _garbage(struct):
    C.memset(C.byref(struct), 0xAB, C.sizeof(struct))
    return struct


def _refused(ctx, scene, entry, m, dst, own):
    """The raw call of `entry` on the mesh struct m (dst: the output mesh where there is one) -> (status, what the entry zeroes on entry). Device buffers go to `own`."""
    from rnb_neus2_amd import _abi
    from rnb_neus2_amd.api import _view_struct
    f, h, view = ctx.f, ctx._h, scene["view"]

    def dev(x):
        own.append(ctx.upload(x) if isinstance(x, np.ndarray) else ctx.device_malloc(x))
        return own[-1]
    if entry == "clean":
        opt, tab = ctx._clean_options("largest", "outward"), C.c_void_p(1)
        rc = f.mesh_clean(h, None, C.byref(m), C.byref(opt), C.byref(dst), C.byref(tab), None)
        assert not tab.value
        return rc, [dst]
    if entry == "simplify":
        opt = ctx._simplify_options(GRID["origin"], GRID["cell"], GRID["dims"], "quadric")
        return f.mesh_simplify(h, None, C.byref(m), C.byref(opt), C.byref(dst), None), [dst]
    if entry == "visibility_select":
        opt, st = ctx._visibility_select_options("component", 1, None, 1), _garbage(_abi.MeshVisibilitySelectStats())
        records = dev(np.zeros(4, np.dtype(_abi.MESH_FACE_VISIBILITY_DTYPE)))
        return f.mesh_visibility_select(h, None, C.byref(m), records, C.byref(opt), C.byref(dst), dev(16), C.byref(st)), [dst, st]
    if entry == "raster":
        opt, st = ctx._raster_options(2.0 ** -10, "none", "face"), _garbage(_abi.MeshRasterStats())
        return f.mesh_raster(h, None, C.byref(m), C.byref(_view_struct(view)), C.byref(opt), dev(64 * 9 * 4), dev(64 * 4), C.byref(st)), [st]
    if entry == "draw_textured":
        opt, st, tex = ctx._draw_options(2.0 ** -10, "none", "face", "bilinear"), _garbage(_abi.MeshDrawStats()), _abi.MeshDrawTexture()
        tex.size, tex.n_tris, tex.uv_dev, tex.color_dev = SIZE, 4, dev(scene["uv"]), dev(scene["color"])
        return f.mesh_draw_textured(h, None, C.byref(m), C.byref(tex), C.byref(_view_struct(view)), C.byref(opt), dev(64 * 9 * 4), dev(64 * 4), C.byref(st)), [st]
    if entry == "visibility":
        opt, varr, st = ctx._visibility_options(2.0 ** -10, "none", 1), ctx._visibility_views([view], None, 1), _garbage(_abi.MeshVisibilityStats())
        return f.mesh_visibility(h, None, C.byref(m), varr, len(varr), C.byref(opt), dev(4 * 40), C.byref(st)), [st]
    if entry == "bake_texture":
        opt, tex, st = ctx._texture_options(SIZE, 0, ("position",), True, 0), _garbage(_abi.MeshTexture()), _garbage(_abi.MeshTextureStats())
        return f.mesh_bake_texture(h, None, C.byref(m), C.byref(opt), C.byref(tex), C.byref(st)), [tex, st]
    if entry == "project_views":
        opt = ctx._project_options(SIZE, 0, "blend", "face", 2, 0.1, 2.0 ** -8, 2.0 ** -10, "none")
        (varr, arrays), proj, st = ctx._project_views([view], [scene["image"]]), _garbage(_abi.MeshProjection()), _garbage(_abi.MeshProjectStats())
        varr[0].image_dev = dev(arrays[0])
        return f.mesh_project_views(h, None, C.byref(m), varr, len(varr), C.byref(opt), C.byref(proj), C.byref(st)), [proj, st]
    good, opt, st = _abi.Mesh(), ctx._distance_options(), _garbage(_abi.MeshDistanceStats())
    good.verts, good.indices, good.n_verts, good.n_indices = dev(TETRA_V), dev(TETRA_T), 4, 12
    a, b = (m, good) if entry == "distance_from" else (good, m)
    return f.mesh_distance(h, None, C.byref(a), C.byref(b), C.byref(opt), dev(16), dev(16), C.byref(st)), [st]


def _same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _valid(ctx, scene, entry):
    """One valid call of `entry` on the tetrahedron against its statement, bit for bit."""
    view, want = scene["view"], scene["want"]
    if entry == "clean":
        got = ctx.clean_mesh(TETRA_V, TETRA_T, table=True)
        mc.assert_equal_bits(got, want["clean"])
        assert got["stats"]["n_tris_out"] == 4
    elif entry == "simplify":
        got = ctx.simplify_mesh(TETRA_V, TETRA_T, **GRID)
        sr.assert_equal_bits(got, want["simplify"])
        assert got["stats"]["n_tris_out"] == 4 and got["stats"]["n_clusters"] == 4
    elif entry == "visibility_select":
        kept, stats, mesh = want["visibility_select"]
        got = ctx.cull_unseen_mesh(TETRA_V, TETRA_T, [view])
        assert np.array_equal(got["kept"], kept) and kept.sum() == 4
        for key in mesh:
            _same_bits(got[key], mesh[key])
        for key, val in stats.items():
            assert got["stats"][key] == val, key
    elif entry == "raster":
        rr.assert_equal_bits(ctx.rasterize_mesh(TETRA_V, TETRA_T, view, faces=True), want["raster"])
        assert want["raster"]["stats"]["n_covered"] > 0
    elif entry == "draw_textured":
        with ctx.upload_mesh(TETRA_V, TETRA_T) as m:
            dw.assert_equal_bits(m.draw_textured(view, scene["uv"], scene["color"], faces=True), want["draw_textured"])
    elif entry == "visibility":
        rec, st = ctx.mesh_visibility(TETRA_V, TETRA_T, [view])
        assert rec.dtype == vr.RECORD
        for name in vr.RECORD.names:
            assert np.array_equal(rec[name], want["visibility"][0][name]), name
        for key in ("n_tris", "n_views", "n_pixels", "n_faces_seen", "n_faces_off_mask") + vr.CLASSES:
            assert st[key] == want["visibility"][1][key], key
        assert st["n_faces_seen"] >= 1
    elif entry == "bake_texture":
        lay, uv, pos = want["bake_texture"]
        got = ctx.bake_texture(TETRA_V, TETRA_T.reshape(-1, 3), SIZE, maps=("position",))
        assert (got["block"], got["blocks_per_row"]) == (lay["block"], lay["blocks_per_row"]) == (4, 2)
        _same_bits(got["uv"], uv)
        _same_bits(got["position"], pos)
    elif entry == "project_views":
        got = ctx.project_views(TETRA_V, TETRA_T.reshape(-1, 3), [view], [scene["image"]], size=SIZE)
        pr.assert_equal_bits(got, want["project_views"])
        assert got["stats"]["n_textured"] > 0
    else:
        got = ctx.mesh_distance(TETRA_V, TETRA_T, TETRA_V, TETRA_T, per_vertex=True)
        dr.assert_equal_bits(got, want["distance"], TETRA_V, TETRA_V, TETRA_T)


@pytest.mark.parametrize("entry,case", [(e, k) for e in ENTRIES for k in CASES if e in WITH_OUT or not CASES[k][4]])  # in == out only where there is an out
def test_invalid_mesh_is_refused_and_the_next_call_is_right(ctx, scene, entry, case):
    from rnb_neus2_amd import _abi
    at, value, n_verts, n_indices, same, text = CASES[case]
    idx = TETRA_T.copy()
    if at is not None:
        idx[at] = value
    own = [ctx.upload(TETRA_V), ctx.upload(idx)]
    try:
        m, out = _abi.Mesh(), _abi.Mesh()
        m.verts, m.indices, m.n_verts, m.n_indices = own[0], own[1], n_verts, n_indices
        out.n_verts, out.verts, out.n_indices = 5, 64, 9
        before = bytes(m)
        rc, zeroed = _refused(ctx, scene, entry, m, m if same else out, own)
        err = ctx.f.last_error()
        assert rc == _abi.ERR_INVALID and text in err and NAMES.get(entry, b"rnb_mesh_" + entry.encode()) in err, (rc, err)
        if entry.startswith("distance"):  # which of the two meshes: "an index of from is ..." from the device check, "rnb_mesh_distance (from): ..." from the host's
            which = entry[9:].encode()
            assert (b"of " + which + b" " if at is not None else b"(" + which + b")") in err, err
        assert bytes(m) == before
        for z in zeroed:
            if z is not m:
                assert bytes(z) == b"\0" * C.sizeof(z), type(z).__name__
    finally:
        for p in own:
            ctx.device_free(p)
    _valid(ctx, scene, entry)
