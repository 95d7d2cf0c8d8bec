"""The statement of include/rnb_mesh_simplify.h in numpy: vertex clustering on a uniform cell grid with quadric (or mean) placement, operation by operation as the
header writes it -- double precision, every operation rounded on its own, 64-bit fixed-point sums added as integers, the solve by the adjugate written out (no
np.linalg). The device has to reproduce `expected` bit for bit."""
import numpy as np

Q_SHIFT, Q_TERM_LOG2 = 40, 22  # RNB_MESH_SIMPLIFY_Q_SHIFT, RNB_MESH_SIMPLIFY_Q_TERM_LOG2
MAX_DIM, MAX_CELLS = 4096, 1 << 30
SCALE, LIMIT = float(1 << Q_SHIFT), float(1 << Q_TERM_LOG2)


def _q(term):
    """Fixed point of an array of terms (truncation); a term that is not finite or not below the bound is an error."""
    term = np.asarray(term, np.float64)
    if not np.all(np.abs(term) < LIMIT):
        raise ValueError("a term is not finite or too large")
    return np.trunc(term * SCALE).astype(np.int64)


def _unq(s):
    return s.astype(np.float64) * (1.0 / SCALE)


def _grid(origin, cell, dims):
    o = np.asarray(origin, np.float32).astype(np.float64).reshape(3)
    c = np.float64(np.float32(cell))
    d = np.array([int(dims)] * 3 if np.isscalar(dims) else [int(x) for x in dims], np.int64)
    if not (np.isfinite(c) and c > 0 and np.all(np.isfinite(o))):
        raise ValueError("cell must be finite and > 0, origin finite")
    if np.any(d < 1) or np.any(d > MAX_DIM) or int(d[0]) * int(d[1]) * int(d[2]) > MAX_CELLS:
        raise ValueError("dims out of range")
    return o, c, d


def locate(verts, origin, cell, dims):
    """Rule 1: (p, i, key) of every vertex: cell-unit coordinates (float64[n,3]), cell indices (int64[n,3]), keys (int64[n])."""
    o, c, d = _grid(origin, cell, dims)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    p = (v - o) / c
    i = np.minimum(np.maximum(np.floor(p), 0.0), (d - 1).astype(np.float64)).astype(np.int64)
    return p, i, i[:, 0] + d[0] * (i[:, 1] + d[1] * i[:, 2])


def _quadric_terms(a, b, c):
    """Rule 3 for triangles with corners a, b, c (float64[n,3], in the cluster's frame): (has_area bool[n], terms float64[n,9])."""
    u, v = b - a, c - a
    nx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    ny = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    nz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
    ok = ln != 0.0
    safe = np.where(ok, ln, 1.0)
    w = 0.5 * ln
    hx, hy, hz = nx / safe, ny / safe, nz / safe
    d = -((hx * a[:, 0] + hy * a[:, 1]) + hz * a[:, 2])
    gx, gy, gz = w * hx, w * hy, w * hz
    return ok, np.stack([gx * hx, gx * hy, gx * hz, gy * hy, gy * hz, gz * hz, gx * d, gy * d, gz * d], 1)


def expected(verts, indices, colors=None, normals=None, origin=(0.0, 0.0, 0.0), cell=1.0 / 256.0, dims=256, placement="quadric"):
    """What rnb_mesh_simplify returns: dict(verts, indices, [colors], [normals], stats) + `cluster_of_vertex` (per input vertex, -1: unused), `cluster_keys` (ascending),
    `vertex_keys` (key of every output vertex) and `tri_kept` (per input triangle). Invalid input raises ValueError."""
    assert placement in ("quadric", "mean")
    o, cw, d = _grid(origin, cell, dims)
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    idx = np.asarray(indices, np.uint32).ravel().astype(np.int64)
    if len(idx) % 3:
        raise ValueError("n_indices is not a multiple of 3")
    t = idx.reshape(-1, 3)
    nv, nt = len(v), len(t)
    attrs = {k: np.asarray(a, np.float32).reshape(-1, 3) for k, a in (("colors", colors), ("normals", normals)) if a is not None}
    if nt and t.max() >= nv:
        raise ValueError("index out of range")
    used = np.zeros(nv, bool)
    used[t.ravel()] = True
    for a in [v] + list(attrs.values()):
        if not np.all(np.isfinite(a[used])):
            raise ValueError("a coordinate or attribute of a used vertex is not finite")
    with np.errstate(all="ignore"):  # unused vertices may hold anything
        p, ci, key = locate(v, origin, cell, dims)
    keys = np.unique(key[used])  # ascending: cluster id = rank
    nc = len(keys)
    cl = np.full(nv, -1, np.int64)
    cl[used] = np.searchsorted(keys, key[used])
    centre = ci.astype(np.float64) + 0.5  # per vertex: the centre of its own cell = of its cluster's cell
    # member sums
    um = np.nonzero(used)[0]
    count = np.bincount(cl[um], minlength=nc).astype(np.int64)
    sx = np.zeros((nc, 3), np.int64)
    np.add.at(sx, cl[um], _q(p[um] - centre[um]))
    asum = {}
    for k, a in attrs.items():
        asum[k] = np.zeros((nc, 3), np.int64)
        np.add.at(asum[k], cl[um], _q(a[um].astype(np.float64)))
    # quadric sums: per triangle and distinct cluster of its corners, in that cluster's frame
    quad = np.zeros((nc, 9), np.int64)
    tc = cl[t] if nt else np.empty((0, 3), np.int64)
    for s in range(3):
        sel = np.ones(nt, bool)
        if s >= 1:
            sel &= tc[:, s] != tc[:, 0]
        if s >= 2:
            sel &= tc[:, s] != tc[:, 1]
        tt = t[sel]
        if not len(tt):
            continue
        ctr = centre[tt[:, s]]
        ok, terms = _quadric_terms(p[tt[:, 0]] - ctr, p[tt[:, 1]] - ctr, p[tt[:, 2]] - ctr)
        np.add.at(quad, tc[sel][:, s][ok], _q(terms[ok]))
    # triangles
    tkeep = (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (tc[:, 0] != tc[:, 2]) if nt else np.empty(0, bool)
    cused = np.zeros(nc, bool)
    cused[tc[tkeep].ravel()] = True
    cmap = np.cumsum(cused) - cused
    out_idx = cmap[tc[tkeep]].astype(np.uint32).ravel()
    # placement of the output vertices
    oc = np.nonzero(cused)[0]
    cnt = count[oc].astype(np.float64)
    m = _unq(sx[oc]) / cnt[:, None]
    x = m.copy()
    n_fallback = 0
    if placement == "quadric" and len(oc):
        with np.errstate(all="ignore"):
            A = _unq(quad[oc])
            axx, axy, axz, ayy, ayz, azz, bx, by, bz = (A[:, k] for k in range(9))
            tr = (axx + ayy) + azz
            e = tr * 2.0 ** -10
            m00, m11, m22, m01, m02, m12 = axx + e, ayy + e, azz + e, axy, axz, ayz
            r0, r1, r2 = e * m[:, 0] - bx, e * m[:, 1] - by, e * m[:, 2] - bz
            c00 = m11 * m22 - m12 * m12
            c01 = m02 * m12 - m01 * m22
            c02 = m01 * m12 - m02 * m11
            c11 = m00 * m22 - m02 * m02
            c12 = m01 * m02 - m00 * m12
            c22 = m00 * m11 - m01 * m01
            det = (m00 * c00 + m01 * c01) + m02 * c02
            y = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
            good = (tr != 0.0) & (det > 0.0) & np.all(np.isfinite(y), axis=1)
        x = np.where(good[:, None], y, m)
        n_fallback = int((~good).sum())
    clamped = np.any((x < -0.5) | (x > 0.5), axis=1)
    x = np.minimum(np.maximum(x, -0.5), 0.5)
    k = keys[oc]
    cell_i = np.stack([k % d[0], (k // d[0]) % d[1], k // (d[0] * d[1])], 1)
    out = dict(verts=(((cell_i.astype(np.float64) + 0.5) + x) * cw + o).astype(np.float32).reshape(-1, 3), indices=out_idx,
               cluster_of_vertex=cl, cluster_keys=keys, vertex_keys=k, tri_kept=tkeep)
    if "colors" in attrs:
        out["colors"] = (_unq(asum["colors"][oc]) / cnt[:, None]).astype(np.float32).reshape(-1, 3)
    if "normals" in attrs:
        s = _unq(asum["normals"][oc])
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        out["normals"] = np.where(ln[:, None] == 0.0, 0.0, s / np.where(ln == 0.0, 1.0, ln)[:, None]).astype(np.float32).reshape(-1, 3)
    out["stats"] = dict(n_verts_in=nv, n_tris_in=nt, n_clusters=nc, n_verts_out=len(oc), n_tris_out=int(tkeep.sum()), n_tris_collapsed=nt - int(tkeep.sum()),
                        n_clamped=int(clamped.sum()), n_fallback=n_fallback)
    return out


def assert_equal_bits(got, want):
    """A dict Context.simplify_mesh / extract_mesh(simplify=) returned against `expected`: arrays bit for bit, the counts of the statistics."""
    for key in ("verts", "indices", "colors", "normals"):
        assert (key in got) == (key in want), key
        if key in want:
            g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert g.shape == w.shape, (key, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (key, int((g != w).sum()))
    st = got["simplify_stats"]
    for key, val in want["stats"].items():
        assert st[key] == val, (key, st[key], val)


def directed_edge_balance(indices):
    """Every directed edge minus its reverse, counted with multiplicity: the number of unmatched directed edges (0 for the image of a closed oriented surface)."""
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(e.max()) + 1 if len(e) else 1
    fwd = np.sort(e[:, 0] * n + e[:, 1])
    rev = np.sort(e[:, 1] * n + e[:, 0])
    return int((fwd != rev).sum())


def signed_volume(verts, indices):
    v = np.asarray(verts, np.float64)
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def sphere_mesh(res, centre=(0.5, 0.5, 0.5), radius=0.3):
    """Marching-cubes sphere on a res^3 lattice over [0, 1)."""
    from tests import mesh_checks
    g = np.arange(res, dtype=np.float64) / res
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    dist = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    assert not (dist.astype(np.float32) == 0).any()
    return mesh_checks.host_marching_cubes(dist.astype(np.float32))
