"""The statement of include/rnb_mesh_smooth.h in numpy, written from the header: the edges by np.unique over the half-edges of the non-degenerate triangles, the kinds,
the selection ring by ring, the passes with the sums as integers of np.trunc(term * 2**32) added by np.add.at, the normals with 2**40. The device has to reproduce
`expected_smooth` and `expected_normals` bit for bit."""
import numpy as np

MAX_RING, MAX_PASSES, MAX_SELECT_RINGS = 1 << 20, 10000, 1024  # RNB_MESH_SMOOTH_MAX_*
Q_SCALE, TERM_LIMIT = 2.0 ** 32, 2.0 ** 10
NORMAL_Q_SCALE, NORMAL_TERM_LIMIT = 2.0 ** 40, 2.0 ** 3
UNUSED, INTERIOR, BOUNDARY, NONMANIFOLD = 0, 1, 2, 3
SMOOTH_STATS = ("n_edges", "n_interior", "n_boundary", "n_nonmanifold", "n_unused", "n_selected", "n_moving", "max_valence", "passes", "max_displacement")
NORMALS_STATS = ("n_zero", "max_corners")


def _q(term, scale, limit, what):
    """The fixed point of an array of terms, int64; a term that is not finite or not below the bound is refused."""
    term = np.asarray(term, np.float64)
    if not (np.abs(term) < limit).all():  # (a NaN compares false)
        raise ValueError("a term is not below %s in magnitude" % what)
    return np.trunc(term * scale).astype(np.int64)


def _unq(s, scale):
    """int64 sums as the doubles the header reads them as: the conversion rounds to nearest even (the C cast numpy makes, in the default rounding mode)."""
    return s.astype(np.float64) * (1.0 / scale)


def _mesh(verts, indices):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    if len(t) and t.max() >= len(v):
        raise ValueError("index out of range")
    return v, t


def edges(n_verts, t):
    """E: (ends int64[n, 2] with a < b, faces int64[n]) of the non-degenerate triangles of t."""
    live = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    a, b = live.ravel(), live[:, [1, 2, 0]].ravel()
    if not len(a):
        return np.empty((0, 2), np.int64), np.empty(0, np.int64)
    n = max(int(n_verts), 1)
    keys, faces = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    return np.stack([keys // n, keys % n], 1), faces


def census(n_verts, t):
    """-> (ends, faces, valence, boundary edges per vertex, kind)"""
    ends, faces = edges(n_verts, t)
    deg = np.bincount(ends.ravel(), minlength=n_verts)
    bdeg = np.bincount(ends[faces == 1].ravel(), minlength=n_verts)
    nm = np.bincount(ends[faces >= 3].ravel(), minlength=n_verts)
    kind = np.where(deg == 0, UNUSED, np.where(nm > 0, NONMANIFOLD, np.where(bdeg > 0, BOUNDARY, INTERIOR)))
    return ends, faces, deg, bdeg, kind


def selection(n_verts, ends, select, rings):
    """D_rings as a bool per vertex."""
    d = np.ones(n_verts, bool) if select is None else (np.asarray(select).ravel() != 0)
    assert len(d) == n_verts
    for _ in range(int(rings)):
        nxt = d.copy()
        nxt[ends[d[ends[:, 1]], 0]] = True
        nxt[ends[d[ends[:, 0]], 1]] = True
        if (nxt == d).all():
            break
        d = nxt
    return d


def expected_smooth(verts, indices, colors=None, normals_in=None, passes=2, lam=0.5, mu=-0.53, boundary="pin", select=None, select_rings=0, normals="keep"):
    """What rnb_mesh_smooth returns: dict(verts, indices, [colors], [normals], valence, kind, displacement, stats) + `moving`, bool per vertex."""
    assert boundary in ("pin", "slide", "free") and normals in ("keep", "recompute") and 0 <= passes <= MAX_PASSES and 0 < lam <= 1 and -1.5 <= mu <= 0
    v, t = _mesh(verts, indices)
    nv = len(v)
    ends, faces, deg, bdeg, kind = census(nv, t)
    sel = selection(nv, ends, select, select_rings)
    moving = sel & ((kind == INTERIOR) | ((kind == BOUNDARY) & (boundary != "pin")))
    slide = moving & (kind == BOUNDARY) & (boundary == "slide")
    # the directed neighbour lists of the moving vertices: (v, u) for u in M(v)
    both = np.concatenate([ends, ends[:, ::-1]])
    bface = np.concatenate([faces, faces])
    take = moving[both[:, 0]] & (~slide[both[:, 0]] | (bface == 1))
    src, dst = both[take, 0], both[take, 1]
    m = np.bincount(src, minlength=nv)
    assert (m[moving] >= 1).all()
    if passes and (m > MAX_RING).any():
        raise ValueError("a moving vertex has more than 2^20 neighbours")
    p0 = v.astype(np.float64)
    p = p0.copy()
    mv = np.flatnonzero(moving)
    for k in range(1, int(passes) + 1):
        f = lam if (k % 2 == 1 or mu == 0) else mu
        s = np.zeros((nv, 3), np.int64)
        np.add.at(s, src, _q(p[dst] - p[src], Q_SCALE, TERM_LIMIT, "2^10"))
        L = _unq(s[mv], Q_SCALE) / m[mv].astype(np.float64)[:, None]
        nxt = p.copy()
        nxt[mv] = p[mv] + np.float64(f) * L
        p = nxt
    out_v = v.copy()
    out_v[mv] = p[mv].astype(np.float32)
    d = p - p0
    disp = np.zeros(nv, np.float32)
    disp[mv] = np.sqrt((d[mv, 0] * d[mv, 0] + d[mv, 1] * d[mv, 1]) + d[mv, 2] * d[mv, 2]).astype(np.float32)
    out = dict(verts=out_v, indices=t.astype(np.uint32).ravel(), valence=deg.astype(np.uint32), kind=kind.astype(np.uint32), displacement=disp, moving=moving)
    if colors is not None:
        out["colors"] = np.asarray(colors, np.float32).reshape(-1, 3)
    if normals == "recompute":
        out["normals"] = expected_normals(out_v, t)["normals"]
    elif normals_in is not None:
        out["normals"] = np.asarray(normals_in, np.float32).reshape(-1, 3)
    out["stats"] = dict(n_edges=len(ends), n_interior=int((kind == INTERIOR).sum()), n_boundary=int((kind == BOUNDARY).sum()), n_nonmanifold=int((kind == NONMANIFOLD).sum()),
                        n_unused=int((kind == UNUSED).sum()), n_selected=int(sel.sum()), n_moving=int(moving.sum()), max_valence=int(deg.max()) if nv else 0, passes=int(passes),
                        max_displacement=float(disp.max()) if nv else 0.0)
    return out


def expected_normals(verts, indices, flip=False):
    """What rnb_mesh_vertex_normals returns: dict(normals float32[n, 3], stats)."""
    v, t = _mesh(verts, indices)
    nv = len(v)
    p = v.astype(np.float64)
    u, w = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    q = _q(n, NORMAL_Q_SCALE, NORMAL_TERM_LIMIT, "2^3")
    corners = np.bincount(t.ravel(), minlength=nv)
    if (corners > MAX_RING).any():
        raise ValueError("a vertex has more than 2^20 corners")
    s = np.zeros((nv, 3), np.int64)
    for k in range(3):
        np.add.at(s, t[:, k], q)
    A = _unq(s, NORMAL_Q_SCALE)
    ln = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        x = A / ln[:, None]
        out = np.where((ln == 0.0)[:, None], np.float32(0), (-x if flip else x).astype(np.float32)).astype(np.float32)
    return dict(normals=out, stats=dict(n_zero=int((ln == 0.0).sum()), max_corners=int(corners.max()) if nv else 0))


def assert_equal_bits(got, want):
    """A dict of the Python layer (Context.smooth_mesh, Context.mesh_vertex_normals / DeviceMesh.vertex_normals) against expected_smooth / expected_normals: every array
    `want` holds bit for bit (the attributes of a smoothed mesh must be there exactly when `want` has them), the counts and max_displacement of the statistics."""
    for key in ("verts", "indices", "colors", "normals", "valence", "kind", "displacement"):
        if "verts" in want and key in ("colors", "normals"):
            assert (key in got) == (key in want), key
        if key in want:
            assert key in got, key
            g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (key, int((g.view(np.uint32) != w.view(np.uint32)).sum()))
    st = got.get("smooth_stats", got.get("stats", got)) if "verts" in want else got.get("stats", got)
    for key, val in want["stats"].items():
        assert st[key] == val, (key, st[key], val)
