"""The statement of include/rnb_mesh_holes.h in numpy, written from the header: the boundary half-edges from tests/mesh_topology_reference.py, the boundary components as
classes of vertices, the cycles walked one step at a time in Python, the sums as integers of np.trunc(term * 2**32), the fill appended loop by loop. The device has to
reproduce `expected_boundary_loops` and `expected_fill` bit for bit. Also the meshes with holes the tests run on."""
import numpy as np

from tests import mesh_clean_reference as mc
from tests import mesh_topology_reference as tr

NONE = tr.NONE
MAX_EDGES = 1 << 20  # RNB_MESH_HOLES_MAX_EDGES
Q_SCALE, TERM_LIMIT = 2.0 ** 32, 2.0 ** 10
TABLE_DTYPE = np.dtype([("label", "<u4"), ("n_edges", "<u4"), ("simple", "<u4"), ("n_irregular", "<u4"), ("component", "<u4"), ("centroid", "<f4", (3,)), ("normal", "<f4", (3,)),
                        ("reserved", "<u4"), ("perimeter", "<f8"), ("area", "<f8")])
LOOPS_STATS = ("n_boundary_edges", "n_loops", "n_simple", "n_irregular_vertices", "max_loop_edges", "n_too_long")
FILL_STATS = ("n_loops", "n_filled", "n_skipped_not_simple", "n_skipped_over_max", "n_skipped_largest", "n_verts_added", "n_tris_added", "n_verts_out", "n_tris_out")


def _q(term):
    """The fixed point of an array of terms, int64; a term that is not finite or not below 2^10 is refused."""
    term = np.asarray(term, np.float64)
    if not (np.abs(term) < TERM_LIMIT).all():  # (a NaN compares false)
        raise ValueError("a term is not below 2^10 in magnitude")
    return np.trunc(term * Q_SCALE).astype(np.int64)


def _sum(q, loop, n_loops):
    """Per loop the integer sum of q (|q| < 2^42 and at most 2^20 terms per loop that is summed: no int64 wraps), as the double the header reads it as."""
    s = np.zeros(n_loops, np.int64)
    np.add.at(s, loop, q)
    return np.array([float(int(x)) for x in s], np.float64) * (1.0 / Q_SCALE), s  # int -> float rounds to nearest even


def _loops(verts, indices, colors=None):
    """Everything both entry points need: per boundary half-edge its loop, successor and position; per loop its record and its colour sums."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nt = len(v), len(t)
    if nt and t.max() >= nv:
        raise ValueError("index out of range")
    he = tr._half_edges(t, tr._nondegenerate(t))
    frm, to = t.ravel(), t[:, [1, 2, 0]].ravel()
    bh = np.flatnonzero(he["n_faces"] == 1)  # ascending
    a, b = frm[bh], to[bh]
    loop_of, nxt, pos = np.full(3 * nt, NONE, np.int64), np.full(3 * nt, NONE, np.int64), np.full(3 * nt, NONE, np.int64)
    if not len(bh):
        return dict(v=v, t=t, bh=bh, a=a, b=b, loop=loop_of, next=nxt, pos=pos, table=np.zeros(0, TABLE_DTYPE), item_loop=np.empty(0, np.int64), colour=np.zeros((0, 3)))
    root = tr._roots(nv, a, b)[a]  # per item: the smallest vertex of its component
    roots, first, inv = np.unique(root, return_index=True, return_inverse=True)  # first: the lowest item = the lowest half-edge of the component
    labels = bh[first]
    order = np.argsort(labels)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    item_loop = rank[inv.ravel()]
    labels = labels[order]
    nl = len(labels)
    table = np.zeros(nl, TABLE_DTYPE)
    table["label"] = labels
    table["n_edges"] = n_edges = np.bincount(item_loop, minlength=nl)
    outc, inc = np.bincount(a, minlength=nv), np.bincount(b, minlength=nv)
    bv = np.unique(np.concatenate([a, b]))
    vert_loop = np.zeros(nv, np.int64)
    vert_loop[a] = item_loop
    vert_loop[b] = item_loop
    irregular = bv[(outc[bv] != 1) | (inc[bv] != 1)]
    table["n_irregular"] = np.bincount(vert_loop[irregular], minlength=nl)
    table["simple"] = simple = table["n_irregular"] == 0
    table["component"] = mc.labels(nv, t)[frm[labels]]
    loop_of[bh] = labels[item_loop]
    outh = np.full(nv, NONE, np.int64)
    np.minimum.at(outh, a, bh)  # the lowest half-edge that starts at a vertex (the only one at a regular vertex)
    for l in np.flatnonzero(simple):  # the cycle walked from the label
        h = int(labels[l])
        for k in range(int(n_edges[l])):
            pos[h] = k
            nxt[h] = outh[to[h]]
            h = int(nxt[h])
        assert h == labels[l]
    # the sums
    if not np.isfinite(v[bv]).all():
        raise ValueError("a coordinate of a boundary vertex is not finite")
    d = v.astype(np.float64)
    o = d[frm[labels]]
    pa, pb, po = d[a], d[b], o[item_loop]
    u, w, e = pb - po, pa - po, pb - pa
    cross = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    length = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    qs = [_q(w[:, k]) for k in range(3)] + [_q(length)] + [_q(cross[:, k]) for k in range(3)]
    if colors is not None:
        col = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
        qs += [_q(col[a][:, k]) for k in range(3)]
    summed = n_edges <= MAX_EDGES
    s = [np.where(summed, _sum(q, item_loop, nl)[0], 0.0) for q in qs]
    n = n_edges.astype(np.float64)
    A = np.stack(s[4:7], 1)
    ln = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            table["centroid"][:, k] = np.where(summed, (s[k] / n + o[:, k]).astype(np.float32), np.float32(0))
            table["normal"][:, k] = np.where(ln == 0.0, np.float32(0), (A[:, k] / ln).astype(np.float32))
        colour = np.stack([(s[7 + k] / n).astype(np.float32) for k in range(3)], 1) if colors is not None else np.zeros((nl, 3), np.float32)
    table["perimeter"] = s[3]
    table["area"] = 0.5 * ln
    return dict(v=v, t=t, bh=bh, a=a, b=b, loop=loop_of, next=nxt, pos=pos, table=table, item_loop=item_loop, colour=colour)


def expected_boundary_loops(verts, indices, colors=None):
    """What rnb_mesh_boundary_loops returns: dict(loop, next, pos uint32[n_indices], table, stats)."""
    L = _loops(verts, indices, colors)
    tab = L["table"]
    stats = dict(n_boundary_edges=len(L["bh"]), n_loops=len(tab), n_simple=int(tab["simple"].sum()), n_irregular_vertices=int(tab["n_irregular"].sum()),
                 max_loop_edges=int(tab["n_edges"].max()) if len(tab) else 0, n_too_long=int((tab["n_edges"] > MAX_EDGES).sum()))
    return dict(loop=L["loop"].astype(np.uint32), next=L["next"].astype(np.uint32), pos=L["pos"].astype(np.uint32), table=tab, stats=stats)


def expected_fill(verts, indices, colors=None, normals=None, max_edges=0, skip_largest=False):
    """What rnb_mesh_fill_holes returns: dict(verts, indices, [colors], [normals], loop_of_tri, stats) + `filled`, the labels of the loops that were filled."""
    L = _loops(verts, indices, colors)
    v, t, tab = L["v"], L["t"], L["table"]
    nv, nt, nl = len(v), len(t), len(tab)
    limit = min(int(max_edges), MAX_EDGES) if max_edges else MAX_EDGES
    largest = {}
    for l in np.flatnonzero(tab["simple"]):  # per connected component: the most edges, then the lowest label (ascending l = ascending label)
        c = int(tab["component"][l])
        if c not in largest or tab["n_edges"][l] > tab["n_edges"][largest[c]]:
            largest[c] = l
    why = np.zeros(nl, np.int64)  # 0 filled, 1 not simple, 2 over the limit, 3 the largest
    for l in range(nl):
        why[l] = 1 if not tab["simple"][l] else 2 if tab["n_edges"][l] > limit else 3 if skip_largest and largest[int(tab["component"][l])] == l else 0
    new_v, new_c, new_n, new_t, lot = [], [], [], [], []
    pos_items = L["pos"][L["bh"]]
    for l in np.flatnonzero(why == 0):
        n = int(tab["n_edges"][l])
        items = _items_of(L, l)
        byk = items[np.argsort(pos_items[items])]
        a, b = L["a"][byk], L["b"][byk]
        if n == 3:
            new_t.append([b[0], a[0], a[2]])
            lot.append(tab["label"][l])
        else:
            c = nv + len(new_v)
            new_v.append(tab["centroid"][l])
            new_c.append(L["colour"][l])
            new_n.append(tab["normal"][l])
            new_t += [[b[k], a[k], c] for k in range(n)]
            lot += [tab["label"][l]] * n
    L.pop("_by_loop", None)
    add = lambda base, rows: np.concatenate([np.asarray(base, np.float32).reshape(-1, 3), np.asarray(rows, np.float32).reshape(-1, 3)])
    out = dict(verts=add(v, new_v), indices=np.concatenate([t, np.asarray(new_t, np.int64).reshape(-1, 3)]).astype(np.uint32).ravel(),
               loop_of_tri=np.concatenate([np.full(nt, NONE, np.int64), np.asarray(lot, np.int64)]).astype(np.uint32), filled=tab["label"][why == 0])
    if colors is not None:
        out["colors"] = add(colors, new_c)
    if normals is not None:
        out["normals"] = add(normals, new_n)
    out["stats"] = dict(n_loops=nl, n_filled=int((why == 0).sum()), n_skipped_not_simple=int((why == 1).sum()), n_skipped_over_max=int((why == 2).sum()),
                        n_skipped_largest=int((why == 3).sum()), n_verts_added=len(new_v), n_tris_added=len(new_t), n_verts_out=nv + len(new_v), n_tris_out=nt + len(new_t))
    return out


def _items_of(L, l):
    """The items of loop l, from one grouping of all items made on first use (a mesh with a thousand loops)."""
    if "_by_loop" not in L:
        order = np.argsort(L["item_loop"], kind="stable")
        counts = np.bincount(L["item_loop"], minlength=len(L["table"]))
        L["_by_loop"] = np.split(order, np.cumsum(counts)[:-1])
    return L["_by_loop"][l]


def assert_equal_bits(got, want):
    """A dict of the Python layer (DeviceMesh.boundary_loops / Context.mesh_boundary_loops, Context.fill_mesh_holes) against expected_boundary_loops / expected_fill: every
    array `want` holds bit for bit (the fill's attributes must be there exactly when `want` has them), the table, the counts of the statistics."""
    for key in ("verts", "indices", "colors", "normals", "loop_of_tri", "loop", "next", "pos"):
        if "verts" in want and key in ("colors", "normals"):
            assert (key in got) == (key in want), key
        if key in want:
            assert key in got, key
            g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (key, int((g != w).sum()))
    if "table" in want:
        assert got["table"].dtype == TABLE_DTYPE, got["table"].dtype
        for name in TABLE_DTYPE.names:
            assert got["table"][name].tobytes() == want["table"][name].tobytes(), (name, got["table"][name], want["table"][name])
    st = got.get("fill_stats", got.get("stats", got)) if "verts" in want else got.get("stats", got)
    for key, val in want["stats"].items():
        assert st[key] == val, (key, st[key], val)


# ---------------------------------------------------------------------------------------------------------------------------- meshes
def punch(v, t, tris):
    """The mesh without the triangles numbered `tris` (the vertices all stay)."""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    keep = np.ones(len(t), bool)
    keep[np.asarray(tris, np.int64)] = False
    return v, t[keep]


def punch_vertex_fans(v, t, verts):
    """The mesh without every triangle that has one of `verts` as a corner."""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    return v, t[~np.isin(t, np.asarray(verts, np.int64)).any(1)]


def neighbours(t, p):
    t = np.asarray(t, np.int64).reshape(-1, 3)
    return np.setdiff1d(np.unique(t[(t == p).any(1)]), [p])


def touching_fans(t):
    """Three vertices (p, q, r) of a closed mesh: the fans of p and q share exactly one rim vertex and no triangle; r's fan touches neither. The first found, p ascending."""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    nv = int(t.max()) + 1
    nb = [None] * nv
    for p in range(nv):
        nb[p] = neighbours(t, p)
        for w in nb[p]:
            for q in neighbours(t, w):
                if q <= p or q in nb[p]:
                    continue
                if len(np.intersect1d(nb[p], neighbours(t, q))) == 1:
                    near = np.unique(np.concatenate([nb[p], neighbours(t, q), [p, q]]))
                    for r in range(nv):
                        if not len(np.intersect1d(np.concatenate([neighbours(t, r), [r]]), near)):
                            return int(p), int(q), int(r)
    raise AssertionError("no two fans touch in one vertex")


def grid_sheet_with_holes(n, m):
    """An open sheet of n x m cells (two triangles each, consistently wound, gently curved) with a hole every third cell both ways, none touching another or the rim:
    in turn one triangle (a loop of 3 edges), both triangles of a cell (4), the fan of a vertex (6). -> (verts, tris, number of holes)"""
    rows, cols, t = tr._grid_tris(n, m, False, False)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    x, y = 0.1 + 0.8 * i / n, 0.1 + 0.8 * j / m
    v = np.stack([x, y, 0.5 + 0.05 * np.sin(7.0 * x) * np.cos(5.0 * y)], -1).reshape(-1, 3).astype(np.float32)
    gone, fans, k = [], [], 0
    for ci in range(2, n - 2, 3):
        for cj in range(2, m - 2, 3):
            cell = ci * m + cj
            if k % 3 == 0:
                gone.append(cell)
            elif k % 3 == 1:
                gone += [cell, n * m + cell]
            else:
                fans.append(ci * cols + cj)
            k += 1
    keep = np.ones(len(t), bool)
    keep[gone] = False
    keep &= ~np.isin(t, fans).any(1)
    return v, t[keep], k


def coloured(v, seed=0):
    """Per-vertex colours in [0, 1) and unit-ish normals for a mesh, float32."""
    rng = np.random.default_rng(seed)
    return rng.random((len(v), 3), dtype=np.float32), rng.standard_normal((len(v), 3)).astype(np.float32)
