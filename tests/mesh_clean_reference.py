"""The statement of include/rnb_mesh_clean.h in numpy / scipy: components of the vertex graph labelled by their smallest vertex, the fixed-point area and signed
volume of each (the header's scale and rounding, every double operation on its own), keep / orient / order rules, the table and the counts of the statistics.
The device has to reproduce `expected` bit for bit."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

Q_SHIFT, Q_TERM_LOG2 = 44, 18  # RNB_MESH_Q_SHIFT, RNB_MESH_Q_TERM_LOG2
NO_LABEL = 0xFFFFFFFF
TABLE_DTYPE = np.dtype([("label", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("kept", "<u4"), ("area_q", "<i8"), ("volume_q", "<i8")])


def labels(n_verts, tris):
    """Per vertex: the smallest vertex of its component, NO_LABEL for a vertex no triangle uses."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(t) and (t.min() < 0 or t.max() >= n_verts):
        raise ValueError("index out of range")
    if n_verts == 0:
        return np.empty(0, np.uint32)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]]])
    g = sparse.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(n_verts, n_verts))
    _, comp = csgraph.connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1 if n_verts else 0, n_verts, np.int64)
    np.minimum.at(smallest, comp, np.arange(n_verts))
    out = smallest[comp].astype(np.uint32) if n_verts else np.empty(0, np.uint32)
    used = np.zeros(n_verts, bool)
    used[t.ravel()] = True
    out[~used] = NO_LABEL
    return out


def terms_q(verts, tris):
    """(area_q, volume_q) per triangle, int64: the header's formulas in double precision, one rounding per operation, times 2^44, truncated towards zero."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(all="ignore"):  # a non-finite term is reported below
        return _terms_q(a, b, c)


def _terms_q(a, b, c):
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    my = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    mz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    vol = ((a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz) / 6.0
    lim = float(1 << Q_TERM_LOG2)
    if not (np.all(area < lim) and np.all(np.abs(vol) < lim)):
        raise ValueError("a term is not finite or too large")
    scale = float(1 << Q_SHIFT)
    return np.trunc(area * scale).astype(np.int64), np.trunc(vol * scale).astype(np.int64)


def expected(verts, indices, colors=None, normals=None, keep="largest", orient="outward"):
    """What rnb_mesh_clean returns: dict(verts, indices, [colors], [normals], table, stats) + `labels` (per input vertex) and `tri_kept` (per input triangle)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nt = len(v), len(t)
    lab = labels(nv, t)
    used = lab != NO_LABEL
    roots = np.unique(lab[used])  # ascending label = table order
    cid_of_vertex = np.searchsorted(roots, lab[used])
    table = np.zeros(len(roots), TABLE_DTYPE)
    table["label"] = roots
    table["n_vertices"] = np.bincount(cid_of_vertex, minlength=len(roots))
    tri_c = np.searchsorted(roots, lab[t[:, 0]]) if nt else np.empty(0, np.int64)
    aq, vq = terms_q(v, t)
    table["n_triangles"] = np.bincount(tri_c, minlength=len(roots))
    area = np.zeros(len(roots), np.int64)
    vol = np.zeros(len(roots), np.int64)
    np.add.at(area, tri_c, aq)
    np.add.at(vol, tri_c, vq)
    table["area_q"], table["volume_q"] = area, vol
    best = int(np.argmax(area)) if len(roots) else -1  # argmax returns the first of equal values = the smallest label
    kept = np.ones(len(roots), bool) if keep == "all" else (np.arange(len(roots)) == best)
    assert keep in ("all", "largest") and orient in ("none", "outward")
    table["kept"] = kept
    flip = kept & (vol < 0) & (orient == "outward")
    vkeep = np.zeros(nv, bool)
    vkeep[used] = kept[cid_of_vertex]
    vmap = np.cumsum(vkeep) - vkeep
    tkeep = kept[tri_c] if nt else np.empty(0, bool)
    tk = t[tkeep]
    fl = flip[tri_c[tkeep]] if nt else np.empty(0, bool)
    tk = np.where(fl[:, None], tk[:, [0, 2, 1]], tk)
    out = dict(verts=v[vkeep], indices=vmap[tk].astype(np.uint32).ravel(), table=table, labels=lab, tri_kept=tkeep)
    if colors is not None:
        out["colors"] = np.asarray(colors, np.float32).reshape(-1, 3)[vkeep]
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(-1, 3)[vkeep]
    out["stats"] = dict(n_components=len(roots), n_kept=int(kept.sum()), n_verts_in=nv, n_verts_out=int(vkeep.sum()), n_tris_in=nt, n_tris_out=int(tkeep.sum()),
                        largest_label=int(roots[best]) if len(roots) else NO_LABEL, area_q_in=int(area.sum()), area_q_out=int(area[kept].sum()))
    return out


def assert_equal_bits(got, want, table=True):
    """A dict Context.clean_mesh / extract_mesh returned against `expected`: arrays bit for bit, the counts of the statistics."""
    for key in ("verts", "indices", "colors", "normals"):
        assert (key in got) == (key in want), key
        if key in want:
            g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert g.shape == w.shape, (key, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), key
    if table:
        assert got["table"].dtype == TABLE_DTYPE and got["table"].tobytes() == want["table"].tobytes()
    st = got.get("clean_stats", got["stats"])
    for key, val in want["stats"].items():
        assert st[key] == val, (key, st[key], val)


def three_spheres(res=64, reverse=None):
    """The marching-cubes mesh (tests.mesh_checks.host_marching_cubes) of three disjoint spheres of clearly different radii on a res^3 lattice over [0, 1): no lattice
    value is exactly 0, so no sphere falls apart into unwelded pieces. reverse = k: the triangles of the k-th sphere (by label order) have their winding reversed."""
    from tests import mesh_checks
    g = np.arange(res, dtype=np.float64) / res
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = None
    for (cx, cy, cz), r in (((0.27, 0.31, 0.29), 0.171), ((0.71, 0.33, 0.37), 0.123), ((0.47, 0.77, 0.69), 0.083)):
        s = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r
        d = s if d is None else np.minimum(d, s)
    assert not (d.astype(np.float32) == 0).any()
    v, i = mesh_checks.host_marching_cubes(d.astype(np.float32))
    i = i.reshape(-1, 3).copy()
    if reverse is not None:
        lab = labels(len(v), i)
        sel = lab[i[:, 0]] == np.unique(lab[lab != NO_LABEL])[reverse]
        i[sel] = i[sel][:, [0, 2, 1]]
    return v, i.ravel()
