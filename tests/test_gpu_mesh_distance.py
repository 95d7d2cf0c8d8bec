"""The mesh-to-mesh distance on the MI355X (include/rnb_mesh_distance.h) against the numpy statement of tests/mesh_distance_reference.py, bit for bit: vert_dist, the raw
sums, the maximum and the counts; vert_nearest through s of the reported triangle, and by index where the case has no tie. Against a simplification, across search grids,
on the stop-rule cases of the CPU tier, far outside and deep inside B's box, with the cap, on ties, under permutations and renumberings, at sizes around the wavefront and
the workgroup, with the large list, on degenerate and invalid input, on the mesh of a model, beside training, and through build/mesh."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_distance_reference as dr
from tests import mesh_simplify_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


@pytest.fixture(scope="module")
def pair():
    """three_spheres(32) (1988 triangles) and its simplification on 16^3 cells, as the statement of the simplifier gives it."""
    v, i = mc.three_spheres(32)
    assert len(i) // 3 == 1988
    e = sr.expected(v, i, origin=(0, 0, 0), cell=1.0 / 16, dims=16)
    return (v, i), (e["verts"], e["indices"])


def _check(c, a, b, by_index=True, cells=0, **kw):
    """One call against the statement; kw: level, max_distance, unit, thresholds."""
    got = c.mesh_distance(a[0], a[1], b[0], b[1], per_vertex=True, cells=cells, **kw)
    ref = dict(kw)
    ref["taus"] = ref.pop("thresholds", ())
    want = dr.expected(a[0], a[1], b[0], b[1], **ref)
    dr.assert_equal_bits(got, want, a[0], b[0], b[1], by_index=by_index)
    return got, want


def _rule_bytes(got):
    """Everything rules 1-5 define, as bytes."""
    return repr([got[k] for k in dr.RULE_KEYS]).encode() + np.float64(got["max"]).tobytes() + got["vert_dist"].tobytes() + got["vert_nearest"].tobytes()


# ------------------------------------------------------------------------------------------------------------------------ against the simplification
@pytest.mark.parametrize("level", [0, 1, 2])
def test_against_the_simplification(ctx, pair, level):
    a, b = pair
    for x, y in ((a, b), (b, a)):
        got, want = _check(ctx, x, y, by_index=False, level=level, thresholds=(0.01, 0.002))
        assert got["n_samples"] == (len(x[1]) // 3 - got["n_degenerate_from"]) * 4 ** level and 0 < got["mean"] < got["rms"] < got["max"] < 0.05
        assert 0 < got["within"][1] < got["within"][0] <= 1 and got["quantisation"] < 1e-9
    cut = a[1][: 3 * (len(a[1]) // 3 - 37)]  # 1951 triangles: no multiple of 64 or 256
    assert (len(cut) // 3) % 64 and (len(b[1]) // 3) % 64
    _check(ctx, (a[0], cut), b, by_index=False, level=level)
    _check(ctx, b, (a[0], cut), by_index=False, level=level)


# ------------------------------------------------------------------------------------------------------------------------ grid independence
def _flat(nx=96, ny=3):
    """A flat, strongly non-cubic strip: nx x ny quads over [0, 3] x [0, 3 / 32] with a gentle ripple in z."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([gx / 32.0, gy / 32.0, 0.01 * np.sin(gx * 0.7) * np.cos(gy * 1.3)], -1).reshape(-1, 3).astype(np.float32)
    q = (gx[:-1, :-1] * (ny + 1) + gy[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([q, q + ny + 1, q + 1], 1), np.stack([q + 1, q + ny + 1, q + ny + 2], 1)]).astype(np.uint32)
    return v, t.ravel()


def test_the_grid_changes_no_bit(ctx, pair):
    a, b = pair
    flat = _flat()
    lifted = (flat[0] * np.float32([0.9, 1.5, 1.0]) + np.float32([0.1, -0.02, 0.03]), flat[1])
    for x, y in ((a, b), (lifted, flat), (a, flat)):
        want = None
        seen = set()
        for cells in (1, 3, 16, 64, 0):
            got = ctx.mesh_distance(x[0], x[1], y[0], y[1], per_vertex=True, cells=cells, level=1, unit=2.0 ** -6, thresholds=(0.01,))
            if want is None:  # cells = 1 is the device's own exhaustive search: every sample tries every triangle once
                want = got
                dr.assert_equal_bits(got, dr.expected(x[0], x[1], y[0], y[1], level=1, unit=2.0 ** -6, taus=(0.01,)), x[0], y[0], y[1], by_index=False)
                assert got["dims"] == [1, 1, 1] and got["n_pairs"] == (got["n_samples"] + got["n_verts_from_used"]) * (got["n_tris_to"] - got["n_degenerate_to"])
            assert _rule_bytes(got) == _rule_bytes(want), cells
            assert max(got["dims"]) == (cells or dr.auto_cells(got["n_tris_to"] - got["n_degenerate_to"]))
            seen.add(tuple(got["dims"]))
        assert len(seen) >= 4
        if y is flat:
            assert got["dims"][1] < got["dims"][0] and got["dims"][2] < got["dims"][0]


# ------------------------------------------------------------------------------------------------------------------------ stop rule and geometry
@pytest.mark.parametrize("case", dr.stop_rule_cases(), ids=lambda c: c[0])
def test_stop_rule_cases(ctx, case):
    _, bv, bi, cells, pts = case
    a = dr.points_mesh(pts)
    for n in (cells, 2 * cells, 1, 0):
        got, want = _check(ctx, a, (bv, bi), by_index=False, cells=n, level=1, unit=1.0)
    s, t = dr.nearest(pts, dr.target(bv, bi)[0])
    assert want["vert_s"][::3].tobytes() == s.tobytes() and np.array_equal(got["vert_nearest"][::3], t)  # the points themselves, lowest index on their ties


def test_outside_far_away_and_inside_one_cell(ctx):
    (ov, oi), (iv, ii) = dr.concentric_spheres()
    b = (iv, ii)
    small = (((ov - np.float32(dr.CENTRE)) * np.float32(0.125)).astype(np.float32), oi[: 3 * 300])  # 300 triangles of a sphere of radius 0.0375 about the origin
    lo, hi = iv.min(0), iv.max(0)
    for axis in range(3):  # entirely outside B's box, on each side
        for side in (-1.0, 1.0):
            shift = np.array(dr.CENTRE, np.float32)
            shift[axis] += np.float32(side * 0.75)
            a = (small[0] + shift, small[1])
            assert (a[0][:, axis].max() < lo[axis]) if side < 0 else (a[0][:, axis].min() > hi[axis])
            _check(ctx, a, b, level=0, cells=16, unit=2.0 ** -4)
    got, _ = _check(ctx, (small[0] + np.float32(dr.CENTRE), small[1]), b, level=1, cells=4, unit=2.0 ** -4)  # inside one cell of B (cells of edge 0.125 around the centre)
    assert abs(got["mean"] - (0.25 - 0.0375)) < 3e-3
    # 40 box diagonals away, above a flat patch: the search ends, and after a few shells -- it does not visit the whole grid
    g = np.arange(33)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    pv = np.stack([gx / 32.0, gy / 32.0, np.zeros_like(gx, float)], -1).reshape(-1, 3).astype(np.float32)
    q = (gx[:-1, :-1] * 33 + gy[:-1, :-1]).ravel()
    pt = np.concatenate([np.stack([q, q + 33, q + 1], 1), np.stack([q + 1, q + 33, q + 34], 1)]).astype(np.uint32).ravel()
    far = (pv * np.float32([0.5, 0.5, 1.0]) + np.float32([0.25, 0.25, 40 * np.sqrt(2.0)]), pt[: 3 * 100])
    got, _ = _check(ctx, far, (pv, pt), by_index=False, level=0, cells=32, unit=1.0)
    n_queries = got["n_samples"] + got["n_verts_from_used"]
    print("far away: %.1f pairs per sample of %d triangles, grid %s" % (got["n_pairs"] / n_queries, len(pt) // 3, got["dims"]))
    assert got["dims"] == [32, 32, 1] and got["n_pairs"] < n_queries * (len(pt) // 3) / 8
    assert abs(got["mean"] - 40 * np.sqrt(2.0)) < 1e-5
    grid = dr.Grid(pv, pt, 32)  # the search restated in Python makes the same evaluations, pair for pair
    used = np.unique(far[1])
    queries = np.concatenate([far[0][used].astype(np.float64), dr.samples(far[0], far[1], 0)[0]])
    assert got["n_pairs"] == sum(grid.query(p)[2] for p in queries) and got["n_cell_entries"] == grid.n_entries and list(grid.dims) == got["dims"] and got["cell"] == grid.cell


# ------------------------------------------------------------------------------------------------------------------------ the cap
def test_the_cap(ctx):
    outer, inner = dr.concentric_spheres()
    free, _ = _check(ctx, outer, inner, level=0, by_index=False)
    low, _ = _check(ctx, outer, inner, level=0, max_distance=0.04, thresholds=(0.04, 0.039))
    assert low["n_beyond"] == low["n_samples"] == 3456 and low["n_verts_beyond"] == low["n_verts_from_used"] and low["max"] == float(np.float32(0.04))
    assert low["sum_w"] == free["sum_w"] and low["within"] == [1.0, 0.0] and low["n_pairs"] < free["n_pairs"]
    high, _ = _check(ctx, outer, inner, level=0, max_distance=0.06, by_index=False)
    assert _rule_bytes(high) == _rule_bytes(free) and high["n_beyond"] == 0
    for e in (free, ctx.mesh_distance(inner[0], inner[1], outer[0], outer[1], level=0)):
        assert abs(e["mean"] - 0.05) <= 3e-3  # the sagitta bound of the CPU tier
    # d == D exactly: a triangle half a unit above the unit triangle
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
    a = ((v * np.float32(0.25) + np.float32([0.125, 0.125, 0.5])).astype(np.float32), np.array([0, 1, 2], np.uint32))
    b = (v, np.array([0, 1, 2], np.uint32))
    got, _ = _check(ctx, a, b, level=2, max_distance=0.5, unit=1.0, thresholds=(0.5,))
    assert got["n_beyond"] == 0 and got["n_verts_beyond"] == 0 and got["max"] == 0.5 and got["vert_nearest"].tolist() == [0, 0, 0] and got["within"] == [1.0]
    got, _ = _check(ctx, a, b, level=2, max_distance=0.25, unit=1.0)
    assert got["n_beyond"] == 16 and got["n_verts_beyond"] == 3 and got["max"] == 0.25 and got["mean"] == 0.25


# ------------------------------------------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_lowest_index(ctx):
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], np.float32)  # two coplanar triangles sharing the edge (1,0,0)-(0,1,0)
    tris = np.array([0, 1, 2, 1, 3, 2], np.uint32)
    a = dr.points_mesh([(0.5, 0.5, 0.25), (0.25, 0.75, 1.0)], e=2.0 ** -3)  # above the shared edge
    for t in (tris, tris.reshape(2, 3)[::-1].ravel()):
        got, want = _check(ctx, a, (v, t), level=0, unit=1.0)
        assert got["vert_nearest"][0] == 0 and got["vert_nearest"][3] == 0 and got["vert_dist"][0] == 0.25 and got["vert_dist"][3] == 1.0
        assert want["vert_s"][0] == 0.0625


# ------------------------------------------------------------------------------------------------------------------------ permutations, renumberings, repeated calls
def test_permutations_renumberings_and_repeated_calls(ctx, pair):
    a, b = pair
    kw = dict(per_vertex=True, level=1, thresholds=(0.01,))
    first = ctx.mesh_distance(a[0], a[1], b[0], b[1], **kw)
    again = ctx.mesh_distance(a[0], a[1], b[0], b[1], **kw)
    assert _rule_bytes(first) == _rule_bytes(again) and first["n_pairs"] == again["n_pairs"]  # two calls in a row: the same bits
    rng = np.random.default_rng(3)

    def permuted(m):
        t = m[1].reshape(-1, 3)
        return m[0], t[rng.permutation(len(t))].ravel()

    def renumbered(m):
        new_of_old = rng.permutation(len(m[0]))
        w = np.empty_like(m[0])
        w[new_of_old] = m[0]
        return (w, new_of_old[m[1]].astype(np.uint32)), new_of_old

    got = ctx.mesh_distance(*permuted(a), b[0], b[1], **kw)  # A's triangles permuted: nothing changes
    assert _rule_bytes(got) == _rule_bytes(first)
    ra, new_of_old = renumbered(a)  # A's vertices renumbered: the per-vertex outputs follow their vertices
    got = ctx.mesh_distance(ra[0], ra[1], b[0], b[1], **kw)
    assert [got[k] for k in dr.RULE_KEYS] == [first[k] for k in dr.RULE_KEYS] and got["max"] == first["max"]
    assert got["vert_dist"][new_of_old].tobytes() == first["vert_dist"].tobytes() and np.array_equal(got["vert_nearest"][new_of_old], first["vert_nearest"])
    rb, _ = renumbered(b)  # B's vertices renumbered: nothing changes
    assert _rule_bytes(ctx.mesh_distance(a[0], a[1], rb[0], rb[1], **kw)) == _rule_bytes(first)
    pb = permuted(b)  # B's triangles permuted: vert_nearest only
    got = ctx.mesh_distance(a[0], a[1], pb[0], pb[1], **kw)
    assert [got[k] for k in dr.RULE_KEYS] == [first[k] for k in dr.RULE_KEYS] and got["max"] == first["max"] and got["vert_dist"].tobytes() == first["vert_dist"].tobytes()
    dr.assert_equal_bits(got, dr.expected(a[0], a[1], pb[0], pb[1], level=1, taus=(0.01,)), a[0], pb[0], pb[1], by_index=False)


# ------------------------------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_a_of_n_triangles_and_b_of_one(ctx, pair, n):
    a, b = pair
    _check(ctx, (a[0], a[1][: 3 * n]), b, by_index=False, level=3 if n == 1 else 1)
    one = (np.array([(0.2, 0.2, 0.5), (0.9, 0.3, 0.4), (0.4, 0.8, 0.6)], np.float32), np.array([0, 1, 2], np.uint32))
    got, _ = _check(ctx, (a[0], a[1][: 3 * n]), one, level=1, unit=2.0 ** -4)
    assert got["dims"] == [1, 1, 1] and got["n_cell_entries"] == 1


def test_a_fan_of_65536_triangles_in_one_cell_and_the_large_list(ctx):
    n = 1 << 16
    ang = np.arange(n + 1) * (2 * np.pi / n)
    fan_v = np.concatenate([[(0.625, 0.625, 0.625)], np.stack([0.625 + 0.05 * np.cos(ang), 0.625 + 0.05 * np.sin(ang), 0.625 + 0.01 * np.sin(5 * ang)], 1)]).astype(np.float32)
    fan_i = np.stack([np.zeros(n, np.uint32), np.arange(1, n + 1, dtype=np.uint32), np.arange(2, n + 2, dtype=np.uint32)], 1).ravel()
    anchors = dr.join(dr.quad(0.0, 0.0, 0.0, 0.03125), dr.quad(1.0, 0.96875, 0.96875, 0.03125))  # they stretch B's box to the unit cube: the fan sits inside the cell [0.5, 0.75]^3 of 4^3
    b = dr.join((fan_v, fan_i), anchors)
    a = dr.points_mesh(np.random.default_rng(9).uniform(0.4, 0.8, (40, 3)), e=2.0 ** -5)
    got, _ = _check(ctx, a, b, by_index=False, level=0, cells=4, unit=2.0 ** -4)
    assert got["dims"] == [4, 4, 4] and got["n_degenerate_to"] == len(b[1]) // 3 - got["n_cell_entries"] and got["n_large"] == 0
    # a 32^3 sphere and the 12 triangles of a box around it at cells = 64: each of the 12 overlaps 64 x 64 cells or more and goes into the large list
    (ov, oi), _ = dr.concentric_spheres()
    corners = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box_i = np.array([k for q in quads for k in (q[0], q[1], q[2], q[0], q[2], q[3])], np.uint32)
    b = dr.join((ov, oi), (corners, box_i))
    inner = dr.concentric_spheres()[1]
    got, _ = _check(ctx, (inner[0], inner[1][: 3 * 600]), b, by_index=False, level=1, cells=64)
    assert got["n_large"] == 12 and got["dims"] == [64, 64, 64] and abs(got["mean"] - 0.05) < 3e-3
    assert got["n_pairs"] >= 12 * (got["n_samples"] + got["n_verts_from_used"])  # every query tests the large list in full


# ------------------------------------------------------------------------------------------------------------------------ invalid input and recovery
def test_invalid_input_fails_cleanly_and_the_context_stays_usable(ctx, pair):
    from rnb_neus2_amd import _abi
    a, b = pair
    ok = lambda: _check(ctx, (a[0], a[1][:300]), b, by_index=False, level=0)
    # degenerate triangles on both sides are counted and ignored; a NaN no triangle uses is accepted
    a2 = (np.concatenate([a[0], np.full((1, 3), np.nan, np.float32)]), np.concatenate([a[1][:300], a[1][[0, 0, 1]], a[1][[5, 5, 5]]]).astype(np.uint32))
    b2 = (np.concatenate([b[0], np.full((2, 3), np.inf, np.float32)]), np.concatenate([b[1][[0, 1, 1]], b[1], b[1][[7, 7, 7]]]).astype(np.uint32))
    got, _ = _check(ctx, a2, b2, by_index=False, level=1)
    assert got["n_degenerate_from"] == 2 and got["n_degenerate_to"] >= 2 and got["vert_nearest"][-1] == dr.NONE and got["vert_dist"][-1] == 0
    for side in (0, 1):
        for bad_value in (None, np.nan, -np.inf):
            ms = [(a[0].copy(), a[1][:300].copy()), (b[0].copy(), b[1].copy())]
            if bad_value is None:
                ms[side][1][11] = len(ms[side][0])  # an index out of range
            else:
                ms[side][0][ms[side][1][11], 2] = bad_value  # a coordinate of a used vertex that is not finite
            with pytest.raises(Exception, match="out of range" if bad_value is None else "not finite"):
                ctx.mesh_distance(ms[0][0], ms[0][1], ms[1][0], ms[1][1])
            ok()
    with pytest.raises(Exception, match="non-degenerate"):  # a B of only degenerate triangles
        ctx.mesh_distance(a[0], a[1][:300], b[0], b[1][[0, 0, 1, 2, 2, 2]])
    ok()
    with pytest.raises(Exception, match="larger unit"):  # d' about 1e5 with w = 8: over the term bound
        ctx.mesh_distance(a[0] * np.float32(64), a[1][:3], b[0] + np.float32(4096), b[1], unit=2.0 ** -10)
    ok()
    e = ctx.mesh_distance(a[0][:5], np.zeros(0, np.uint32), b[0], b[1], per_vertex=True)  # an empty A: zero sums
    assert e["sum_w"] == 0 and e["n_samples"] == 0 and e["mean"] == 0 and e["max"] == 0 and np.all(e["vert_nearest"] == dr.NONE) and np.all(e["vert_dist"] == 0)
    assert e["dims"] == [0, 0, 0]
    # too many large triangles: a coarser grid is asked for
    n = 4097
    strip = (np.concatenate([np.stack([np.zeros(n), np.arange(n) / n, np.zeros(n)], 1), np.stack([np.ones(n), np.arange(n) / n, np.ones(n)], 1), [(0, 0, 1.0)]]).astype(np.float32),
             np.stack([np.arange(n), np.arange(n) + n, np.full(n, 2 * n)], 1).astype(np.uint32).ravel())
    with pytest.raises(Exception, match="coarser grid"):
        ctx.mesh_distance(a[0], a[1][:3], strip[0], strip[1], cells=64)
    _check(ctx, (a[0], a[1][:30]), strip, by_index=False, level=0, cells=8, unit=2.0 ** -4)
    ok()
    # the raw call: stats are zeroed on a failure
    st = _abi.MeshDistanceStats()
    st.n_tris_to = 9
    with ctx.upload_mesh(a[0], a[1][:300], None, None) as ma, ctx.upload_mesh(b[0], b[1], None, None) as mb:
        opt = ctx._distance_options()
        opt.level = 4
        assert ctx.f.mesh_distance(ctx._h, None, C.byref(ma), C.byref(mb), C.byref(opt), None, None, C.byref(st)) == _abi.ERR_INVALID and st.n_tris_to == 0
        opt.level = 1
        assert ctx.f.mesh_distance(ctx._h, None, C.byref(ma), C.byref(mb), C.byref(opt), None, None, None) == 0  # every output is optional


# ------------------------------------------------------------------------------------------------------------------------ on a model, beside training, build/mesh
MODEL_STEPS = 60


def _same_report(x, y):
    keys = dr.RULE_KEYS + ("max", "mean", "rms", "n_pairs", "dims")
    return all(x[k] == y[k] for k in keys) and all(x["reverse"][k] == y["reverse"][k] for k in keys) and all(x[k] == y[k] for k in ("chamfer", "hausdorff"))


def test_extract_mesh_reports_the_error_of_its_simplification():
    """A model trained for MODEL_STEPS steps: extract_mesh(res=128, simplify=32, error=True) returns under simplify_error what mesh_distance(symmetric=True) gives for the
    mesh before and the mesh after, and otherwise what it returns without error=True."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(16, 128, 1400.0 * 128 / 800.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(MODEL_STEPS):
            c.train_step()
        kw = dict(res=128, cull="none", colors=True)
        raw = c.extract_mesh(**kw)
        plain = c.extract_mesh(simplify=32, **kw)
        both = c.extract_mesh(simplify=32, error=True, **kw)
        assert "simplify_error" not in plain and sorted(set(both) - set(plain)) == ["simplify_error"]
        for key in ("verts", "indices", "colors"):
            assert both[key].tobytes() == plain[key].tobytes()
        apart = c.mesh_distance(raw["verts"], raw["indices"], plain["verts"], plain["indices"], symmetric=True)
        err = both["simplify_error"]
        assert _same_report(err, apart)
        print("the model's mesh, %d -> %d triangles: in -> out mean %.3e rms %.3e max %.3e, out -> in mean %.3e rms %.3e max %.3e" % (
            len(raw["indices"]) // 3, len(plain["indices"]) // 3, err["mean"], err["rms"], err["max"], err["reverse"]["mean"], err["reverse"]["rms"], err["reverse"]["max"]))
        assert 0 < err["mean"] < err["rms"] < err["max"] <= np.sqrt(3.0) / 32 and err["chamfer"] == err["mean"] + err["reverse"]["mean"]  # no vertex leaves its cell of edge 1 / 32
        assert err["hausdorff"] == max(err["max"], err["reverse"]["max"])
        dr.assert_equal_bits(c.mesh_distance(plain["verts"], plain["indices"], raw["verts"], raw["indices"], per_vertex=True),
                             dr.expected(plain["verts"], plain["indices"], raw["verts"], raw["indices"]), plain["verts"], raw["verts"], raw["indices"], by_index=False)
        with pytest.raises(ValueError):
            c.extract_mesh(error=True, **kw)


def test_measuring_leaves_training_untouched(pair):
    """deterministic = 1: 40 steps, two mesh_distance calls and an extract_mesh(simplify=..., error=True), 40 steps == 80 steps, bit for bit."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    a, b = pair
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(80):
            if interrupt and s == 40:
                c.mesh_distance(a[0], a[1], b[0], b[1], symmetric=True, per_vertex=True)
                c.extract_mesh(64, cull="none", simplify=16, error=True)
            stats.append(c.train_step().as_dict())
        state = {k: c.get(k).copy() for k in ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID", "DENSITY_BITFIELD")}
        for st in stats:
            st.pop("prep_ms"), st.pop("step_ms")
        runs.append((state, stats))
        c.close()
    (sa, ta), (sb, tb) = runs
    assert ta == tb
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def test_build_mesh_reports_the_numbers_of_the_python_call(tmp_path):
    """`build/mesh --resolution 128 --simplify 32 --report-error` on a snapshot the testbed wrote prints the mean, rms and max of both directions that
    Context.extract_mesh(res=128, simplify=32, error=True) returns on a context holding the same snapshot; without the flag the line is absent."""
    from rnb_neus2_amd import synthetic
    from tests.test_gpu_mesh_simplify import _context_of
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "128", "--out", str(tmp_path / "m.obj"), "--simplify", "32"]
    r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "simplify:" in r.stdout and "simplify error:" not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
    r = subprocess.run(base + ["--report-error"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("simplify error:")]
    assert len(line) == 1, r.stdout
    print(line[0])
    m = re.match(r"simplify error: in -> out mean (\S+) rms (\S+) max (\S+), out -> in mean (\S+) rms (\S+) max (\S+), (\S+) ms$", line[0])
    with _context_of(snap) as c:
        err = c.extract_mesh(res=128, colors=True, simplify=32, error=True)["simplify_error"]
    want = [err["mean"], err["rms"], err["max"], err["reverse"]["mean"], err["reverse"]["rms"], err["reverse"]["max"]]
    assert [x.rstrip(",") for x in m.groups()[:6]] == ["%.9g" % x for x in want]
    r = subprocess.run(base[:-2] + ["--report-error"], capture_output=True, text=True)
    assert r.returncode == 255 and "--simplify" in r.stderr


def test_mesh_eval_prints_the_symmetric_measures(ctx, tmp_path):
    """tools/mesh_eval.py on two OBJ files (the concentric spheres, 0.05 apart) prints one JSON line whose figures are those of Context.mesh_distance(symmetric=True) on the
    meshes load_obj reads, with the unit chosen from the reference's box."""
    import json
    import sys
    from rnb_neus2_amd import meshproc
    outer, inner = dr.concentric_spheres()
    paths = []
    for name, (v, i) in (("outer.obj", outer), ("inner.obj", inner)):
        paths.append(str(tmp_path / name))
        meshproc.save_obj(paths[-1], meshproc.Mesh(v, i.reshape(-1, 3)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mesh_eval.py"), "--mesh", paths[0], "--reference", paths[1], "--tau", "0.049", "0.052", "--level", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    a, b = meshproc.load_obj(paths[0]), meshproc.load_obj(paths[1])
    assert out["unit"] == 2.0 ** -11 and abs(out["diagonal"] - 0.5 * np.sqrt(3.0)) < 0.02  # a box of edge 0.5: diagonal / 1024 lies between 2^-11 and 2^-10
    want = ctx.mesh_distance(a.vertices, a.faces, b.vertices, b.faces, level=0, unit=out["unit"], thresholds=(0.049, 0.052), symmetric=True)
    assert (out["chamfer"], out["hausdorff"], out["accuracy"], out["completeness"]) == (want["chamfer"], want["hausdorff"], want["mean"], want["reverse"]["mean"])
    assert (out["precision"], out["recall"], out["fscore"]) == (want["within"], want["reverse"]["within"], want["fscore"])
    assert abs(out["chamfer"] - 0.1) < 6e-3 and out["hausdorff"] <= 0.0513 and out["fscore"][1] == 1.0 and 0 <= out["fscore"][0] < 1
    p, q = out["precision"][0], out["recall"][0]
    assert out["fscore"][0] == (2 * p * q / (p + q) if p + q else 0.0)
