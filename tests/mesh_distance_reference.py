"""The numpy statement of include/rnb_mesh_distance.h, operation for operation: (i) the definition, rules 1-5 by an exhaustive minimum over all triangles of B, and (ii)
the search of the header (cell lists over B's box, Chebyshev shells, the stop rule) restated with Python loops, so that the stop rule can be checked without a device.
numpy rounds every operation on its own (no fused multiply-add), which is what the library is compiled to do."""
import functools
import math

import numpy as np

Q_SHIFT, Q_TERM_LOG2 = 48, 12
MAX_LEVEL, MAX_TAUS, NONE = 3, 4, 0xFFFFFFFF
MAX_CELLS, LARGE_CELLS, MAX_LARGE = 256, 2048, 4096


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def normal_length(a, b, c):
    """l of rule 1 (a, b, c: float64[..., 3])."""
    u, v = b - a, c - a
    n = np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)
    return np.sqrt(_dot(n, n))


def point_triangle(p, a, b, c):
    """Rule 2: s(p, T) and the number of the region that decided (0 a, 1 b, 2 ab, 3 c, 4 ac, 5 bc, 6 face); the arguments broadcast against each other."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        g, h = d4 - d3, d5 - d6
        k = (va + vb) + vc
        y, z = vb / k, vc / k
        q = (a + ab * y[..., None]) + ac * z[..., None]
        region = np.full(q.shape[:-1], 6)
        cases = [  # in reverse order: the first test of the header that holds is applied last
            (5, (va <= 0) & (g >= 0) & (h >= 0), lambda: b + (c - b) * (g / (g + h))[..., None]),
            (4, (vb <= 0) & (d2 >= 0) & (d6 <= 0), lambda: a + ac * (d2 / (d2 - d6))[..., None]),
            (3, (d6 >= 0) & (d5 <= d6), lambda: c + np.zeros_like(q)),
            (2, (vc <= 0) & (d1 >= 0) & (d3 <= 0), lambda: a + ab * (d1 / (d1 - d3))[..., None]),
            (1, (d3 >= 0) & (d4 <= d3), lambda: b + np.zeros_like(q)),
            (0, (d1 <= 0) & (d2 <= 0), lambda: a + np.zeros_like(q)),
        ]
        for number, cond, value in cases:
            q = np.where(cond[..., None], value(), q)
            region = np.where(cond, number, region)
        e = p - q
        return _dot(e, e), region


def _mesh(verts, indices, what):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(indices).ravel()
    if len(i) % 3:
        raise ValueError("%s: n_indices is not a multiple of 3" % what)
    if len(i) and (len(v) == 0 or i.max() >= len(v) or i.min() < 0):
        raise ValueError("%s: an index is out of range" % what)
    t = i.astype(np.int64).reshape(-1, 3)
    used = np.zeros(len(v), bool)
    used[t.ravel()] = True
    if not np.isfinite(v[used]).all():
        raise ValueError("%s: a coordinate of a used vertex is not finite" % what)
    return v.astype(np.float64), t, used


def target(b_verts, b_indices):
    """Rule 1: (a, b, c, index) of the non-degenerate triangles of B, float64[m, 3] each and their positions in B's triangle list; the number of degenerate ones."""
    v, t, _ = _mesh(b_verts, b_indices, "to")
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    keep = normal_length(a, b, c) != 0 if len(t) else np.zeros(0, bool)
    return (a[keep], b[keep], c[keep], np.nonzero(keep)[0]), int(len(t) - keep.sum())


def nearest(points, tgt, chunk=1 << 22, prune=True):
    """Rule 3 without the cap: s(p) and nearest(p) for float64[n, 3] points, the minimum of rule 2 over ALL the triangles of tgt. prune=False evaluates every pair. prune=True
    (the default, some twenty times faster) leaves out the pairs that cannot hold the minimum and changes no bit: with m and R the centre and the radius of a ball around a
    triangle, every point of it is at least |p - m| - R from p; a triangle is left out only if that bound, lowered by 1e-6 (1 + |p - m|) against every rounding here and
    in rule 2, still lies above the computed s(p, T0) of the triangle T0 with the nearest centre."""
    a, b, c, index = tgt
    p = np.asarray(points, np.float64).reshape(-1, 3)
    s, t = np.full(len(p), np.inf), np.full(len(p), NONE, np.int64)
    if not len(p) or not len(index):
        return s, t
    step = max(1, chunk // len(index))
    if prune:
        m = (a + b + c) / 3.0
        rad = np.sqrt(np.maximum(np.maximum(((a - m) ** 2).sum(1), ((b - m) ** 2).sum(1)), ((c - m) ** 2).sum(1)))
    for lo in range(0, len(p), step):
        q = p[lo:lo + step]
        if prune:
            dist = np.sqrt(np.maximum((q * q).sum(1)[:, None] - 2.0 * (q @ m.T) + (m * m).sum(1)[None, :], 0.0))
            k0 = np.argmin(dist, axis=1)
            upper = point_triangle(q, a[k0], b[k0], c[k0])[0]
            lower = np.maximum(dist - rad[None, :] - 1e-6 * (1.0 + dist), 0.0)
            rows, cols = np.nonzero(~(lower * lower > upper[:, None]))  # (a NaN upper bound keeps every triangle); row-major: ascending triangle within a point
            st = point_triangle(q[rows], a[cols], b[cols], c[cols])[0]
            st = np.where(np.isnan(st), np.inf, st)
            first = np.nonzero(np.diff(rows, prepend=-1))[0]  # every point keeps at least T0
            smin = np.minimum.reduceat(st, first)
            hit = np.nonzero(st == smin[rows])[0]
            _, where = np.unique(rows[hit], return_index=True)  # the first pair of each point that attains its minimum: the lowest index
            s[lo:lo + step] = smin
            t[lo:lo + step] = np.where(np.isinf(smin), NONE, index[cols[hit[where]]])
            continue
        st = point_triangle(q[:, None, :], a[None], b[None], c[None])[0]
        st = np.where(np.isnan(st), np.inf, st)
        k = np.argmin(st, axis=1)  # the first minimum: the lowest index (the triangles are in ascending order)
        s[lo:lo + step] = st[np.arange(len(k)), k]
        t[lo:lo + step] = np.where(np.isinf(s[lo:lo + step]), NONE, index[k])
    return s, t


def capped(s, t, max_distance):
    """d, nearest, beyond of rule 3 from s and the uncapped nearest."""
    d = np.sqrt(s)
    D = np.float64(np.float32(max_distance))
    beyond = (d > D) if D > 0 else np.zeros(len(d), bool)
    return np.where(beyond, D, d), np.where(beyond, NONE, t), beyond


def samples(a_verts, a_indices, level):
    """Rule 4 (b): points float64[n, 3], weights, the triangle of each sample; the number of degenerate triangles of A. Triangle-major, upward ones first."""
    v, t, _ = _mesh(a_verts, a_indices, "from")
    n = 1 << level
    num = [(3 * i + 1, 3 * j + 1, 3 * n - 3 * i - 3 * j - 2) for i in range(n) for j in range(n - i)] + [(3 * i + 2, 3 * j + 2, 3 * n - 3 * i - 3 * j - 4) for i in range(n - 1) for j in range(n - 1 - i)]
    bary = np.array(num, np.float64) / np.float64(3 * n)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    l = normal_length(a, b, c) if len(t) else np.zeros(0)
    keep = l != 0
    a, b, c, l = a[keep], b[keep], c[keep], l[keep]
    p = (a[:, None, :] * bary[None, :, 0, None] + b[:, None, :] * bary[None, :, 1, None]) + c[:, None, :] * bary[None, :, 2, None]
    w = np.repeat((0.5 * l) / np.float64(n * n), n * n)
    return p.reshape(-1, 3), w, np.repeat(np.nonzero(keep)[0], n * n), int(len(t) - keep.sum())


def _q(term):
    if not np.all(np.isfinite(term) & (term >= 0) & (term < 2.0 ** Q_TERM_LOG2)):
        raise ValueError("a term is not finite or not below 2^12")
    return sum(int(x) for x in np.trunc(term * 2.0 ** Q_SHIFT))  # Python integers: exact


def expected(a_verts, a_indices, b_verts, b_indices, level=1, max_distance=0.0, unit=2.0 ** -10, taus=(), search=None):
    """What rnb_mesh_distance returns: vert_dist, vert_nearest, vert_s (s of every used vertex, before the cap) and stats with the fields of rnb_mesh_distance_stats that
    rules 1-5 define. search = None: the exhaustive minimum; else a function (points) -> (s, nearest), e.g. one made by shell_search."""
    if not 0 <= level <= MAX_LEVEL:
        raise ValueError("level")
    unit, D = np.float64(np.float32(unit)), np.float64(np.float32(max_distance))
    tau = [np.float64(np.float32(x)) for x in taus] + [np.float64(0)] * (MAX_TAUS - len(taus))
    if len(tau) > MAX_TAUS or not (np.isfinite(unit) and unit > 0 and np.isfinite(D) and D >= 0 and all(np.isfinite(x) and x >= 0 for x in tau)):
        raise ValueError("options")
    va, ta, used_a = _mesh(a_verts, a_indices, "from")
    st = dict(n_verts_from_used=int(used_a.sum()), n_verts_to_used=0, n_tris_from=len(ta), n_tris_to=len(np.asarray(b_indices).ravel()) // 3, n_degenerate_from=0, n_degenerate_to=0,
              n_verts_beyond=0, n_samples=0, n_beyond=0, sum_w=0, sum_wd=0, sum_wd2=0, sum_within=[0] * MAX_TAUS, max_distance=0.0)
    out = dict(vert_dist=np.zeros(len(va), np.float32), vert_nearest=np.full(len(va), NONE, np.uint32), vert_s=np.zeros(len(va)), stats=st)
    if not len(ta):
        return out
    tgt, st["n_degenerate_to"] = target(b_verts, b_indices)
    st["n_verts_to_used"] = int(_mesh(b_verts, b_indices, "to")[2].sum())
    if not len(tgt[3]):
        raise ValueError("to has no non-degenerate triangle")
    find = search or (lambda pts: nearest(pts, tgt))
    # (a) the used vertices
    s, t = find(va[used_a])
    d, t, beyond = capped(s, t, D)
    out["vert_dist"][used_a], out["vert_nearest"][used_a], out["vert_s"][used_a] = d.astype(np.float32), t.astype(np.uint32), s
    st["n_verts_beyond"] = int(beyond.sum())
    dmax = d.max()
    # (b) the sub-centroids
    p, w, _, st["n_degenerate_from"] = samples(a_verts, a_indices, level)
    st["n_samples"] = len(p)
    if len(p):
        s, t = find(p)
        d, t, beyond = capped(s, t, D)
        st["n_beyond"] = int(beyond.sum())
        dmax = max(dmax, d.max())
        dp = d / unit
        wd = w * dp
        st["sum_w"], st["sum_wd"], st["sum_wd2"] = _q(w), _q(wd), _q(wd * dp)
        st["sum_within"] = [_q(w[d <= x]) if x != 0 else 0 for x in tau]
        if max([st["sum_w"], st["sum_wd"], st["sum_wd2"]] + st["sum_within"]) >= 1 << 63:
            raise ValueError("a sum reaches 2^15")
        out["sample_d"], out["sample_w"] = d, w
    st["max_distance"] = float(dmax)
    return out


def summary(st, unit=2.0 ** -10):
    """mean, rms and the within fractions from the raw sums, as api.Context.mesh_distance computes them."""
    unit = float(np.float32(unit))
    if not st["sum_w"]:
        return dict(mean=0.0, rms=0.0, within=[0.0] * MAX_TAUS)
    return dict(mean=st["sum_wd"] / st["sum_w"] * unit, rms=math.sqrt(st["sum_wd2"] / st["sum_w"]) * unit, within=[x / st["sum_w"] for x in st["sum_within"]])


# ------------------------------------------------------------------------------------------------------------------------ (ii) the search of the header
def auto_cells(m):
    return min(max(math.isqrt(m // 2), 1), MAX_CELLS)


class Grid:
    """The cell lists over the box of B's used vertices; cells = N along the longest axis (0: automatic)."""

    def __init__(self, b_verts, b_indices, cells=0):
        v, t, used = _mesh(b_verts, b_indices, "to")
        self.tgt, _ = target(b_verts, b_indices)
        a, b, c, index = self.tgt
        self.lo, self.hi = v[used].min(0), v[used].max(0)
        n = cells or auto_cells(len(index))
        self.cell = (self.hi - self.lo).max() / np.float64(n)
        self.dims = np.minimum(n, np.floor((self.hi - self.lo) / self.cell) + 1).astype(np.int64)
        self.lists, self.large, self.n_entries = {}, [], 0
        c0, c1 = self.cell_of(np.minimum(np.minimum(a, b), c)), self.cell_of(np.maximum(np.maximum(a, b), c))
        for k in range(len(index)):
            if np.prod(c1[k] - c0[k] + 1) > LARGE_CELLS:
                self.large.append(k)
                continue
            for z in range(c0[k, 2], c1[k, 2] + 1):
                for y in range(c0[k, 1], c1[k, 1] + 1):
                    for x in range(c0[k, 0], c1[k, 0] + 1):
                        self.lists.setdefault((x, y, z), []).append(k)
                        self.n_entries += 1
        if len(self.large) > MAX_LARGE:
            raise ValueError("the large list is full")

    def cell_of(self, x):
        return np.minimum(np.maximum(np.floor((x - self.lo) / self.cell), 0), self.dims - 1).astype(np.int64)

    def query(self, p, max_distance=0.0):
        """s(p), nearest(p) (before the cap), the number of point-triangle evaluations and the last shell visited."""
        a, b, c, index = self.tgt
        D = np.float64(np.float32(max_distance))
        best_s, best_t, pairs = np.inf, NONE, 0

        def visit(ks):
            nonlocal best_s, best_t, pairs
            if not len(ks):
                return
            ks = np.asarray(ks)
            s = point_triangle(p[None], a[ks], b[ks], c[ks])[0]
            pairs += len(ks)
            s = np.where(np.isnan(s), np.inf, s)
            sk = s.min()
            tk = int(index[ks][s == sk].min())
            if sk < best_s or (sk == best_s and tk < best_t):
                best_s, best_t = float(sk), tk

        visit(self.large)
        q = np.minimum(np.maximum(p, self.lo), self.hi)
        o = p - q
        ctr = self.cell_of(q)
        o2 = _dot(o, o) * (1.0 - 2.0 ** -20)
        rmax = int(np.maximum(ctr, self.dims - 1 - ctr).max())
        r = 0
        for r in range(rmax + 1):
            z0, z1 = max(ctr[2] - r, 0), min(ctr[2] + r, self.dims[2] - 1)
            y0, y1 = max(ctr[1] - r, 0), min(ctr[1] + r, self.dims[1] - 1)
            x0, x1 = max(ctr[0] - r, 0), min(ctr[0] + r, self.dims[0] - 1)
            shell = []
            for z in range(z0, z1 + 1):
                for y in range(y0, y1 + 1):
                    if abs(z - ctr[2]) == r or abs(y - ctr[1]) == r:
                        xs = range(x0, x1 + 1)
                    else:
                        xs = [x for x in (ctr[0] - r, ctr[0] + r) if 0 <= x <= self.dims[0] - 1]
                    for x in xs:
                        shell += self.lists.get((x, y, z), [])
            visit(shell)  # (one evaluation per shell: the order inside a shell decides nothing)
            if r >= 1:
                e = (np.float64(r) - 0.0625) * self.cell
                bound = e * e + o2
                if best_s <= bound or (D > 0 and bound >= D * D):
                    break
        return best_s, best_t, pairs, r

    def search(self, max_distance=0.0):
        """A `search` argument of expected(). Keeps the number of evaluations in self.n_pairs."""
        self.n_pairs = 0

        def find(points):
            res = [self.query(np.asarray(p, np.float64), max_distance) for p in points]
            self.n_pairs += sum(x[2] for x in res)
            return np.array([x[0] for x in res], np.float64), np.array([x[1] for x in res], np.int64)
        return find


# ------------------------------------------------------------------------------------------------------------------------ meshes the CPU and the GPU tier share
CENTRE = (0.47, 0.49, 0.48)


@functools.lru_cache(maxsize=None)
def concentric_spheres():
    """Marching-cubes spheres of radii 0.30 (outer) and 0.25 (inner) about CENTRE on a 32^3 lattice: ((verts, indices), (verts, indices)), 3456 and 2408 triangles."""
    from tests import mesh_simplify_reference as sr
    outer, inner = sr.sphere_mesh(32, np.array(CENTRE), 0.30), sr.sphere_mesh(32, np.array(CENTRE), 0.25)
    assert (len(outer[1]) // 3, len(inner[1]) // 3) == (3456, 2408)
    return outer, inner


def quad(z, x0=0.0, y0=0.0, e=0.25):
    """Two triangles over the square [x0, x0 + e] x [y0, y0 + e] at height z."""
    return np.array([(x0, y0, z), (x0 + e, y0, z), (x0 + e, y0 + e, z), (x0, y0 + e, z)], np.float32), np.array([0, 1, 2, 0, 2, 3], np.uint32)


def join(*meshes):
    vs, is_, base = [], [], 0
    for v, i in meshes:
        vs.append(v)
        is_.append(i + base)
        base += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(is_).astype(np.uint32)


def stop_rule_cases():
    """Hand-made cases with dyadic coordinates: (name, B verts, B indices, cells, points). The box of every B is [0, 4]^3 through two tiny corner triangles."""
    corner = join(quad(0.0, 0.0, 0.0, 0.125), quad(4.0, 3.875, 3.875, 0.125))
    cases = []
    # a sample on a cell corner (cells of edge 1), triangles in the cells around it
    b = join(corner, quad(2.5, 1.5, 1.5, 0.25), quad(1.5, 2.25, 2.25, 0.25))
    cases.append(("cell corner", b[0], b[1], 4, np.array([(2.0, 2.0, 2.0), (1.0, 2.0, 3.0), (2.0, 2.0, 1.5)])))
    # the nearest triangle two shells away on the diagonal while a farther one sits in shell 1: p in cell (1, 1, 1); shell 1 holds the corner triangles at the origin
    # (s = 10.32...), cell (3, 3, 3) of shell 2 a quad whose corner (3, 3, 3) is 1.0625 away per axis
    b = join(corner, quad(3.0, 3.0, 3.0, 0.125))
    cases.append(("diagonal", b[0], b[1], 4, np.array([(1.9375, 1.9375, 1.9375), (1.0, 1.0, 1.0)])))
    # a sample at exactly r * cell from a triangle: p at x = 0.5, the triangle in the plane x = 2.5 (two cells away), another at x = 3.5
    wall = lambda x: (np.array([(x, 2.25, 2.25), (x, 2.75, 2.25), (x, 2.25, 2.75)], np.float32), np.array([0, 1, 2], np.uint32))
    b = join(corner, wall(2.5), wall(3.5))
    cases.append(("exactly r cells", b[0], b[1], 4, np.array([(0.5, 2.375, 2.375), (1.5, 2.375, 2.375), (0.0, 2.375, 2.375), (-0.5, 2.375, 2.375)])))
    return cases


def points_mesh(points, e=2.0 ** -6):
    """A mesh that has the given points among its used vertices: one small triangle (p, p + (e, 0, 0), p + (0, e, 0)) per point; vertex 3k is point k."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.stack([p, p + np.float32([e, 0, 0]), p + np.float32([0, e, 0])], 1).reshape(-1, 3)
    return v.astype(np.float32), np.arange(len(v), dtype=np.uint32)


RULE_KEYS = ("n_verts_from_used", "n_verts_to_used", "n_tris_from", "n_tris_to", "n_degenerate_from", "n_degenerate_to", "n_verts_beyond", "n_samples", "n_beyond", "sum_w", "sum_wd",
             "sum_wd2", "sum_within")


def assert_equal_bits(got, want, a_verts, b_verts, b_indices, by_index=True):
    """got: the dict of api.Context.mesh_distance(per_vertex=True); want: expected(). vert_dist, the raw sums, the maximum and the counts bit for bit; vert_nearest through
    s of the reported triangle, and by index where the case has no tie (by_index)."""
    for key in RULE_KEYS:
        assert got[key] == want["stats"][key], (key, got[key], want["stats"][key])
    assert np.float64(got["max"]).tobytes() == np.float64(want["stats"]["max_distance"]).tobytes(), (got["max"], want["stats"]["max_distance"])
    assert got["vert_dist"].tobytes() == want["vert_dist"].tobytes()
    near = got["vert_nearest"]
    assert np.array_equal(near == NONE, want["vert_nearest"] == NONE)
    k = np.nonzero(near != NONE)[0]
    if len(k):
        v = np.asarray(b_verts, np.float32).reshape(-1, 3).astype(np.float64)
        t = np.asarray(b_indices).astype(np.int64).reshape(-1, 3)[near[k]]
        s = point_triangle(np.asarray(a_verts, np.float32).reshape(-1, 3).astype(np.float64)[k], v[t[:, 0]], v[t[:, 1]], v[t[:, 2]])[0]
        assert s.tobytes() == want["vert_s"][k].tobytes()
    if by_index:
        assert np.array_equal(near, want["vert_nearest"])
