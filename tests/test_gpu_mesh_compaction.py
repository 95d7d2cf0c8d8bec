"""The one compaction of the mesh drivers (MeshCall::compact; k_compact_verts, k_compact_tris of mesh_common.cuh) through both of its callers on one mesh: three closed
components of 200 triangles each (600 triangles: three workgroups, a component boundary inside two of them), one wound inward, the vertices in shuffled numbering, five
vertices no triangle uses, colours and normals. rnb_mesh_clean keeps by component and flips the inward one; rnb_mesh_visibility_select keeps by triangle, on records
that leave one component unseen. Every output is compared bit for bit with the numpy statements, and peak_workspace with the value of the build before the two stages
shared their compaction."""
import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_visibility_reference as vr

pytestmark = pytest.mark.gpu

# peak_workspace of the four calls below as the parent of the change that introduced the shared compaction returned them on an MI355X for this mesh (311 vertices, 600
# triangles; it is also what its allocation sequence adds up to: the workspace of the stage less `used` where it is released, plus the output mesh).
PEAK = dict(clean_all=20860, clean_largest=8716, select_component=19568, select_face=18324)


def bipyramid(n, centre, radius, height):
    """A closed surface of 2n triangles wound outward: an n-gon equator, one apex above and one below."""
    a = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(a), radius * np.sin(a), np.zeros(n)], axis=1)
    v = np.concatenate([ring, [[0, 0, height], [0, 0, -height]]]) + np.asarray(centre)
    k, nxt = np.arange(n), (np.arange(n) + 1) % n
    top = np.stack([k, nxt, np.full(n, n)], axis=1)
    bottom = np.stack([nxt, k, np.full(n, n + 1)], axis=1)
    return v.astype(np.float32), np.concatenate([top, bottom]).astype(np.uint32)


@pytest.fixture(scope="module")
def mesh():
    parts = [bipyramid(100, (0.3, 0.3, 0.5), 0.10, 0.12), bipyramid(100, (0.7, 0.3, 0.5), 0.18, 0.20), bipyramid(100, (0.5, 0.7, 0.5), 0.14, 0.10)]
    parts[2] = (parts[2][0], parts[2][1][:, [0, 2, 1]])  # wound inward
    v = np.concatenate([p[0] for p in parts] + [np.full((5, 3), 0.9, np.float32)])  # ... and five vertices no triangle uses
    t = np.concatenate([p[1] + 102 * k for k, p in enumerate(parts)])
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(v))  # old -> new number
    vs = np.empty_like(v)
    vs[perm] = v
    t = perm[t].astype(np.uint32)
    assert vs.shape == (311, 3) and t.shape == (600, 3) and len(np.unique(t)) == 306
    colors, normals = rng.uniform(0, 1, vs.shape).astype(np.float32), rng.uniform(-1, 1, vs.shape).astype(np.float32)
    part = np.repeat(np.arange(3), 200)
    return vs, t.ravel(), colors, normals, part


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
    c.init_params()
    yield c
    c.close()


@pytest.mark.parametrize("keep,orient,peak,n_tris,n_verts", [("all", "outward", "clean_all", 600, 306), ("largest", "outward", "clean_largest", 200, 102)])
def test_clean_compacts_by_component(ctx, mesh, keep, orient, peak, n_tris, n_verts):
    v, t, colors, normals, part = mesh
    want = mc.expected(v, t, colors, normals, keep=keep, orient=orient)
    assert len(want["indices"]) == 3 * n_tris and len(want["verts"]) == n_verts and want["stats"]["n_components"] == 3
    if keep == "all":  # the inward component comes out flipped, the other two as they were
        tri_in, tri_out = t.reshape(-1, 3), want["indices"].reshape(-1, 3)
        assert np.array_equal(want["verts"][tri_out[part == 2][:, [0, 2, 1]]], v[tri_in[part == 2]]) and np.array_equal(want["verts"][tri_out[part != 2]], v[tri_in[part != 2]])
    got = ctx.clean_mesh(v, t, colors, normals, keep=keep, orient=orient, table=True)
    mc.assert_equal_bits(got, want)
    assert got["stats"]["peak_workspace"] == PEAK[peak]


@pytest.mark.parametrize("unit,rings,peak", [("component", 1, "select_component"), ("face", 0, "select_face")])
def test_select_seen_compacts_by_triangle(ctx, mesh, unit, rings, peak):
    v, t, colors, normals, part = mesh
    records = np.zeros(600, vr.RECORD)
    records["n_seen"] = part != 1  # the largest component is seen by no view
    records["n_drawn"] = 1
    records["best_view"][part == 1] = 0xFFFFFFFF
    kept, stats = vr.select(len(v), t, records, unit=unit, rings=rings)
    want = vr.compact(v, t, kept, colors, normals)
    assert np.array_equal(kept != 0, part != 1) and len(want["verts"]) == 204
    ptr = ctx.upload(records)
    try:
        with ctx.upload_mesh(v, t, colors, normals) as m, m.select_seen(ptr, unit=unit, rings=rings, kept=True) as out:
            got, st = out.download(), out.stats
    finally:
        ctx.device_free(ptr)
    assert np.array_equal(st["kept"], kept)
    for key in ("verts", "indices", "colors", "normals"):
        assert got[key].dtype == want[key].dtype and got[key].size == want[key].size and got[key].tobytes() == want[key].tobytes(), key
    for key, val in stats.items():
        assert st[key] == val, (key, st[key], val)
    assert (st["n_verts_in"], st["n_tris_in"], st["n_verts_out"], st["n_tris_out"]) == (311, 600, 204, 400)
    assert st["peak_workspace"] == PEAK[peak]
