"""The statement of include/rnb_mesh_intersect.h in Python: the rules of the self-intersection census of a triangle mesh, operation for operation what
rnb_mesh_intersections computes (Python floats are IEEE doubles and every operation below is rounded on its own), and of rnb_mesh_intersections_select.
exact=True evaluates the SAME rules with the signs of orient and orient2 taken from fractions.Fraction, which are exact on float inputs: what the float rules may
only approximate (a sign of 0 means "not decided in double") the rational rules decide. Brute force over all pairs: nothing here knows of a search grid."""
from fractions import Fraction

import numpy as np

APART, PROPER, CONTACT = 0, 1, 2  # the class of a pair (rnb_mesh_intersect_pair.cls; PROPER and CONTACT are also the bits of the select mask)
EPS3, EPS2 = 2.0 ** -48, 2.0 ** -50
AXES = ((1, 2), (2, 0), (0, 1))  # (i, j) of orient2 for axis x, y, z
STAT_KEYS = ("n_tris", "n_degenerate", "n_same_set", "n_candidates", "n_pairs_proper", "n_pairs_contact", "n_tris_proper", "n_tris_contact", "n_coplanar_pairs")


def _sign(x):
    return (x > 0) - (x < 0)


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


class Rules:
    """The sign routines, in double (exact=False) or in rationals (exact=True). `inplane` is set by every orient2 call: the caller clears and reads it."""

    def __init__(self, exact=False):
        self.exact, self.inplane = exact, False

    def point(self, p):
        return tuple(Fraction(float(x)) for x in p) if self.exact else tuple(float(x) for x in p)

    def orient(self, a, b, c, d):
        u, v, w = _sub(b, a), _sub(c, a), _sub(d, a)
        det = _dot(_cross(u, v), w)
        if self.exact:
            return _sign(det)
        m = (abs(u[1] * v[2]) + abs(u[2] * v[1]), abs(u[2] * v[0]) + abs(u[0] * v[2]), abs(u[0] * v[1]) + abs(u[1] * v[0]))
        P = (m[0] * abs(w[0]) + m[1] * abs(w[1])) + m[2] * abs(w[2])
        return 0 if abs(det) <= EPS3 * P else _sign(det)

    def orient2(self, a, b, c, axis):
        self.inplane = True
        i, j = AXES[axis]
        l, r = (b[i] - a[i]) * (c[j] - a[j]), (b[j] - a[j]) * (c[i] - a[i])
        d = l - r
        if self.exact:
            return _sign(d)
        return 0 if abs(d) <= EPS2 * (abs(l) + abs(r)) else _sign(d)

    @staticmethod
    def axis(t):
        n = _cross(_sub(t[1], t[0]), _sub(t[2], t[0]))
        n = (abs(n[0]), abs(n[1]), abs(n[2]))
        k = 0
        if n[1] > n[k]:
            k = 1
        if n[2] > n[k]:
            k = 2
        return k

    # ---- the in-plane separation tests (non-strict: on the line counts as outside) ----
    def tri_tri_separated(self, S, T, eS, eT, axis):
        for X, Y, eY in ((T, S, eS), (S, T, eT)):
            for k in range(3):
                e0, e1, e2 = X[k], X[(k + 1) % 3], X[(k + 2) % 3]
                ref = self.orient2(e0, e1, e2, axis)
                if ref == 0:
                    continue  # an edge line whose own triangle has no side in double separates nothing
                if all(self.orient2(e0, e1, Y[j], axis) * ref <= 0 for j in range(3) if j != eY):
                    return True
        return False

    def seg_tri_separated(self, p, q, F, axis):
        for k in range(3):
            e0, e1, e2 = F[k], F[(k + 1) % 3], F[(k + 2) % 3]
            ref = self.orient2(e0, e1, e2, axis)
            if ref == 0:
                continue
            if self.orient2(e0, e1, p, axis) * ref <= 0 and self.orient2(e0, e1, q, axis) * ref <= 0:
                return True
        t = [self.orient2(p, q, F[k], axis) for k in range(3)]
        return all(x >= 0 for x in t) or all(x <= 0 for x in t)

    def edge(self, p, q, sp, sq, F):
        """Step 3 for one edge (p, q) with endpoint signs sp, sq against the triangle F: APART (nothing), CONTACT or PROPER."""
        if sp * sq > 0:
            return APART
        if sp == 0 and sq == 0:
            return APART if self.seg_tri_separated(p, q, F, self.axis(F)) else CONTACT
        s = (self.orient(p, q, F[0], F[1]), self.orient(p, q, F[1], F[2]), self.orient(p, q, F[2], F[0]))
        if any(x > 0 for x in s) and any(x < 0 for x in s):
            return APART
        if sp * sq < 0 and s[0] == s[1] == s[2] != 0:
            return PROPER
        return CONTACT

    def classify(self, S, T, iS, iT):
        """(class, coplanar): S, T three points each, iS, iT their index triples; S is the lower triangle. The pair is a candidate (not the same set)."""
        shared = [(a, b) for a in range(3) for b in range(3) if iS[a] == iT[b]]
        if len(shared) == 2:
            kS = 3 - shared[0][0] - shared[1][0]
            kT = 3 - shared[0][1] - shared[1][1]
            if self.orient(T[0], T[1], T[2], S[kS]) != 0:
                return APART, False
            axis = self.axis(T)
            p, q = T[(kT + 1) % 3], T[(kT + 2) % 3]
            a, b = self.orient2(p, q, S[kS], axis), self.orient2(p, q, T[kT], axis)
            return (APART if a * b < 0 else CONTACT), True
        eS, eT = (shared[0] if shared else (-1, -1))
        sS = [None if k == eS else self.orient(T[0], T[1], T[2], S[k]) for k in range(3)]
        live = [x for x in sS if x is not None]
        if live[0] != 0 and all(x == live[0] for x in live):
            return APART, False
        sT = [None if k == eT else self.orient(S[0], S[1], S[2], T[k]) for k in range(3)]
        live_t = [x for x in sT if x is not None]
        if live_t[0] != 0 and all(x == live_t[0] for x in live_t):
            return APART, False
        if all(x == 0 for x in live) or all(x == 0 for x in live_t):
            return (APART if self.tri_tri_separated(S, T, eS, eT, self.axis(T)) else CONTACT), True
        proper = contact = False
        for X, F, sX, eX in ((S, T, sS, eS), (T, S, sT, eT)):
            for k in range(3):
                k1 = (k + 1) % 3
                if eX in (k, k1):
                    continue
                r = self.edge(X[k], X[k1], sX[k], sX[k1], F)
                proper |= r == PROPER
                contact |= r == CONTACT
        return (PROPER if proper else CONTACT if contact else APART), False


def _tris(verts, indices):
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    return v, t


def degenerate(verts, indices):
    """l == 0 of rule 1 of rnb_mesh_distance.h, per triangle."""
    v, t = _tris(verts, indices)
    p = v.astype(np.float64)[t.astype(np.int64)]
    u, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) == 0.0


def box_pairs(verts, indices):
    """(s, t), s < t, of the triangles that take part and whose closed float boxes overlap on every axis (same-set pairs included), ascending."""
    v, t = _tris(verts, indices)
    live = ~degenerate(v, t)
    p = v[t.astype(np.int64)]
    lo, hi = p.min(1), p.max(1)
    out = []
    n = len(t)
    for s0 in range(0, n, 512):
        s1 = min(s0 + 512, n)
        ov = np.ones((s1 - s0, n), bool)
        for k in range(3):
            ov &= (lo[s0:s1, None, k] <= hi[None, :, k]) & (lo[None, :, k] <= hi[s0:s1, None, k])
        ov &= live[s0:s1, None] & live[None, :]
        a, b = np.nonzero(ov)
        keep = a + s0 < b
        out.append(np.stack([a[keep] + s0, b[keep]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def classify_pairs(verts, indices, exact=False):
    """{(s, t): (class, coplanar, inplane)} over the candidate pairs, and the number of same-set pairs."""
    v, t = _tris(verts, indices)
    R = Rules(exact)
    pts = [R.point(p) for p in v]
    tl = [tuple(int(x) for x in row) for row in t]
    out, same = {}, 0
    for s, u in box_pairs(v, t):
        s, u = int(s), int(u)
        if set(tl[s]) == set(tl[u]):
            same += 1
            continue
        R.inplane = False
        cls, cop = R.classify([pts[i] for i in tl[s]], [pts[i] for i in tl[u]], tl[s], tl[u])
        out[(s, u)] = (cls, cop, R.inplane)
    return out, same


def census(verts, indices, exact=False):
    """What rnb_mesh_intersections reports: n_proper, n_contact (uint32 per triangle), pairs (int64[n, 3]: s, t, class; ascending) and the stats outside the grid block."""
    v, t = _tris(verts, indices)
    classes, same = classify_pairs(v, t, exact)
    n = len(t)
    n_proper, n_contact = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    pairs, cop = [], 0
    for (s, u), (cls, coplanar, _) in sorted(classes.items()):
        cop += coplanar
        if cls == APART:
            continue
        pairs.append((s, u, cls))
        for x in (s, u):
            (n_proper if cls == PROPER else n_contact)[x] += 1
    pairs = np.array(pairs, np.int64).reshape(-1, 3)
    stats = dict(n_tris=n, n_degenerate=int(degenerate(v, t).sum()), n_same_set=same, n_candidates=len(classes), n_pairs_proper=int((pairs[:, 2] == PROPER).sum()),
                 n_pairs_contact=int((pairs[:, 2] == CONTACT).sum()), n_tris_proper=int((n_proper > 0).sum()), n_tris_contact=int((n_contact > 0).sum()), n_coplanar_pairs=cop)
    return dict(n_proper=n_proper, n_contact=n_contact, pairs=pairs, stats=stats)


def select(verts, indices, n_proper, n_contact, classes=PROPER, rings=0, drop_unused_vertices=True, colors=None, normals=None):
    """rnb_mesh_intersections_select: the mesh without the triangles with a partner in one of `classes`, the selection grown `rings` times by the triangles that
    share a vertex with it; input order; -> dict(verts, indices, [colors, normals], n_tris_removed, n_verts_removed)."""
    v, t = _tris(verts, indices)
    ti = t.astype(np.int64)
    sel = np.zeros(len(t), bool)
    if classes & PROPER:
        sel |= np.asarray(n_proper) > 0
    if classes & CONTACT:
        sel |= np.asarray(n_contact) > 0
    for _ in range(rings):
        mark = np.zeros(len(v), bool)
        mark[ti[sel].ravel()] = True
        sel = sel | mark[ti].any(1)
    kept = ti[~sel]
    keep_v = np.ones(len(v), bool)
    if drop_unused_vertices:
        keep_v[:] = False
        keep_v[kept.ravel()] = True
    vmap = np.cumsum(keep_v) - 1
    out = dict(verts=v[keep_v], indices=vmap[kept].astype(np.uint32).ravel(), n_tris_removed=int(sel.sum()), n_verts_removed=int((~keep_v).sum()))
    for key, a in (("colors", colors), ("normals", normals)):
        if a is not None:
            out[key] = np.ascontiguousarray(a, np.float32).reshape(-1, 3)[keep_v]
    return out


# ---- the meshes of the tests ----
def uv_sphere(centre=(0.5, 0.5, 0.5), radius=0.3, rings=5, seg=12):
    """Poles plus `rings` rings of `seg` vertices: 2 * seg * rings triangles (120), float32 vertices, outward winding."""
    c = np.float64(centre)
    v = [c + [0, 0, radius]]
    for r in range(1, rings + 1):
        th = np.pi * r / (rings + 1)
        for k in range(seg):
            ph = 2 * np.pi * k / seg
            v.append(c + radius * np.float64([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    v.append(c - [0, 0, radius])
    t = []
    ring = lambda r, k: 1 + r * seg + k % seg
    for k in range(seg):
        t.append((0, ring(0, k), ring(0, k + 1)))
        for r in range(rings - 1):
            t.append((ring(r, k), ring(r + 1, k), ring(r + 1, k + 1)))
            t.append((ring(r, k), ring(r + 1, k + 1), ring(r, k + 1)))
        t.append((len(v) - 1, ring(rings - 1, k + 1), ring(rings - 1, k)))
    return np.float32(v), np.uint32(t).ravel()


def join(*meshes):
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(np.float32(v))
        ts.append(np.uint32(t).ravel() + np.uint32(off))
        off += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def two_spheres():
    return join(uv_sphere(), uv_sphere((0.72, 0.55, 0.47), 0.25))


def flat_grid(n=3, shift=(0.0, 0.0, 0.0)):
    """n x n quads on multiples of 1/4 in the plane z = 0.25, two triangles each."""
    g = np.arange(n + 1)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    v = np.stack([gx / 4.0, gy / 4.0, np.full(gx.shape, 0.25)], -1).reshape(-1, 3) + np.float64(shift)
    q = (gx[:-1, :-1] * (n + 1) + gy[:-1, :-1]).ravel()
    t = np.concatenate([np.stack([q, q + n + 1, q + 1], 1), np.stack([q + 1, q + n + 1, q + n + 2], 1)])
    return np.float32(v), np.uint32(t).ravel()


def two_grids():
    return join(flat_grid(), flat_grid(shift=(0.125, 0.0625, 0.0)))


def hand_cases():
    """name -> (verts, indices, expected class of the pair (0, 1) or None where there is no candidate pair, expected stats subset)."""
    f = np.float32
    base = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    return {
        "edge_through_interior": (f(base + [[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 1]]), [0, 1, 2, 3, 4, 5], PROPER, {}),
        "vertex_on_face": (f(base + [[0.25, 0.25, 0], [0.25, 0.25, 1], [0.75, 0.5, 1]]), [0, 1, 2, 3, 4, 5], CONTACT, {}),
        "edge_along_edge": (f(base + [[0.25, 0, 0], [0.75, 0, 0], [0.5, -0.5, 1]]), [0, 1, 2, 3, 4, 5], CONTACT, {}),
        "fold": (f(base + [[0.25, 0.5, 0]]), [0, 1, 2, 1, 0, 3], CONTACT, {"n_coplanar_pairs": 1}),
        "hinge": (f(base + [[0.25, 0.5, 1]]), [0, 1, 2, 1, 0, 3], APART, {"n_coplanar_pairs": 0}),
        "shared_vertex_pierced": (f(base + [[0.25, 0.25, -1], [0.25, 0.25, 1]]), [0, 1, 2, 0, 3, 4], PROPER, {}),
        "shared_vertex_only": (f(base + [[-1, 0, 1], [0, -1, 1]]), [0, 1, 2, 0, 3, 4], APART, {}),
        "degenerate": (f(base + [[0.25, 0.25, -1], [0.25, 0.25, 1], [0.25, 0.25, 3]]), [0, 1, 2, 3, 4, 5], None, {"n_degenerate": 1, "n_candidates": 0}),
        "same_set": (f(base), [0, 1, 2, 2, 1, 0], None, {"n_same_set": 1, "n_candidates": 0}),
    }
