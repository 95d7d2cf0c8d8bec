"""The statement of include/rnb_mesh_topology.h in numpy / scipy, written from the header: half-edges grouped by np.unique on edge keys, triangles on their ascending
triples, vertices on their coordinates; patches and the double cover as connected components with the smallest node per class; the duplicate rules, the sheet
rule and the compaction. The device has to reproduce `expected_topology` and `expected_repair` bit for bit. Also the meshes the tests run on."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

from tests import mesh_clean_reference as mc

NONE = 0xFFFFFFFF  # RNB_MESH_TOPOLOGY_NONE
MAX_BUCKET = 65536  # RNB_MESH_TOPOLOGY_MAX_BUCKET
TABLE_DTYPE = np.dtype([("label", "<u4"), ("n_vertices", "<u4"), ("n_edges", "<u4"), ("n_triangles", "<u4"), ("n_boundary_edges", "<u4"), ("n_nonmanifold_edges", "<u4"),
                        ("n_inconsistent_edges", "<u4"), ("n_patches", "<u4"), ("euler", "<i4"), ("genus", "<i4")])
TOPOLOGY_STATS = ("n_verts_used", "n_tris", "n_degenerate", "n_edges", "n_boundary_edges", "n_manifold_edges", "n_nonmanifold_edges", "n_inconsistent_edges",
                  "max_faces_on_edge", "n_duplicate_tris", "n_folded_pairs", "n_components", "n_patches", "n_unorientable_patches", "n_boundary_components", "closed",
                  "oriented", "euler")
REPAIR_STATS = ("n_welded", "n_degenerate_dropped", "n_duplicates_dropped", "n_flipped", "n_patches", "n_unorientable_patches", "n_verts_in", "n_verts_out", "n_tris_in",
                "n_tris_out")


def _roots(n, a, b):
    """Per node 0 .. n-1: the smallest node of its class under the unions a[i] ~ b[i]."""
    if n == 0:
        return np.empty(0, np.int64)
    g = sparse.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, comp = csgraph.connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp]


def _half_edges(t, live):
    """t int64[nt,3], live bool[nt] (the triangles that take part). Per half-edge h = 3t + k: faces on its edge, faces in its direction, mate, the id of its edge
    (-1 for a half-edge that takes no part); per edge: its face count, its two ends, its lowest half-edge."""
    nt = len(t)
    frm, to = t.ravel(), t[:, [1, 2, 0]].ravel()
    part = np.repeat(live, 3)
    n_faces, n_same, mate, eid = np.zeros(3 * nt, np.int64), np.zeros(3 * nt, np.int64), np.full(3 * nt, NONE, np.int64), np.full(3 * nt, -1, np.int64)
    h = np.flatnonzero(part)
    if not len(h):
        z = np.empty(0, np.int64)
        return dict(n_faces=n_faces, n_same=n_same, mate=mate, eid=eid, edge_faces=z, edge_ends=np.empty((0, 2), np.int64), edge_first=z, pairs=(z, z), frm=frm)
    lo, hi = np.minimum(frm[h], to[h]), np.maximum(frm[h], to[h])
    n = int(t.max()) + 1  # (indices are below 2^32: lo * n + hi fits an int64 key up to n = 2^31)
    keys, first, inv, counts = np.unique(lo * n + hi, return_index=True, return_inverse=True, return_counts=True)
    keys = np.stack([keys // n, keys % n], 1)
    eid[h] = inv
    n_faces[h] = counts[inv]
    _, dinv, dcounts = np.unique(frm[h] * n + to[h], return_inverse=True, return_counts=True)
    n_same[h] = dcounts[dinv]
    order = np.argsort(inv, kind="stable")  # half-edges edge by edge, ascending inside an edge
    starts = np.cumsum(counts) - counts
    two = np.flatnonzero(counts == 2)
    h1, h2 = h[order[starts[two]]], h[order[starts[two] + 1]]
    mate[h1], mate[h2] = h2, h1
    return dict(n_faces=n_faces, n_same=n_same, mate=mate, eid=eid, edge_faces=counts, edge_ends=keys.reshape(-1, 2), edge_first=h[first], pairs=(h1, h2), frm=frm)


def _cover(t, live, he):
    """The double cover: root per node (2t, 2t+1), int64[2 nt]."""
    h1, h2 = he["pairs"]
    t1, t2 = h1 // 3, h2 // 3
    same = (he["frm"][h1] == he["frm"][h2]).astype(np.int64)  # inconsistent: 2t ~ 2u+1, 2t+1 ~ 2u
    return _roots(2 * len(t), np.concatenate([2 * t1, 2 * t1 + 1]), np.concatenate([2 * t2 + same, 2 * t2 + 1 - same]))


def _nondegenerate(t):
    return (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])


def _vertex_sets(t, live):
    """Per live triangle: group id of its vertex set, whether its winding is odd. -> (ids of the live triangles, group per live triangle, odd per live triangle)"""
    ids = np.flatnonzero(live)
    tl = t[ids]
    odd = ((tl[:, 0] > tl[:, 1]).astype(np.int64) + (tl[:, 0] > tl[:, 2]) + (tl[:, 1] > tl[:, 2])) & 1
    if not len(tl):
        return ids, np.empty(0, np.int64), odd
    n, srt = int(tl.max()) + 1, np.sort(tl, axis=1)
    if n ** 3 < 2 ** 62:  # the ascending triple as one int64 key (much the faster np.unique)
        _, group = np.unique((srt[:, 0] * n + srt[:, 1]) * n + srt[:, 2], return_inverse=True)
    else:
        _, group = np.unique(srt, axis=0, return_inverse=True)
    return ids, group.ravel(), odd


def expected_topology(n_verts, indices):
    """What rnb_mesh_topology returns: dict(n_faces, n_same, mate uint32[n_indices], table, stats)."""
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nt = int(n_verts), len(t)
    if nt and t.max() >= nv:
        raise ValueError("index out of range")
    live = _nondegenerate(t)
    he = _half_edges(t, live)
    lab = mc.labels(nv, t)
    used = lab != mc.NO_LABEL
    roots = np.unique(lab[used])
    table = np.zeros(len(roots), TABLE_DTYPE)
    table["label"] = roots
    cid = lambda verts: np.searchsorted(roots, lab[verts])
    nc = len(roots)
    table["n_vertices"] = np.bincount(cid(np.flatnonzero(used)), minlength=nc)
    table["n_triangles"] = np.bincount(cid(t[live, 0]), minlength=nc)
    faces, ends = he["edge_faces"], he["edge_ends"]
    ec = cid(ends[:, 0]) if len(ends) else np.empty(0, np.int64)
    h1, h2 = he["pairs"]
    inconsistent_pair = he["frm"][h1] == he["frm"][h2]
    inc_edge = np.zeros(len(faces), bool)
    inc_edge[he["eid"][h1[inconsistent_pair]]] = True
    table["n_edges"] = np.bincount(ec, minlength=nc)
    table["n_boundary_edges"] = np.bincount(ec[faces == 1], minlength=nc)
    table["n_nonmanifold_edges"] = np.bincount(ec[faces >= 3], minlength=nc)
    table["n_inconsistent_edges"] = np.bincount(ec[inc_edge], minlength=nc)
    # patches: the live triangles joined across manifold edges; unorientable through the double cover
    proot = _roots(nt, h1 // 3, h2 // 3)
    patch_first = np.flatnonzero(live & (proot == np.arange(nt)))
    cover = _cover(t, live, he)
    unorientable = cover[2 * patch_first] == cover[2 * patch_first + 1]
    table["n_patches"] = np.bincount(cid(t[patch_first, 0]), minlength=nc)
    euler = table["n_vertices"].astype(np.int64) - table["n_edges"] + table["n_triangles"]
    table["euler"] = euler
    surface = (table["n_boundary_edges"] == 0) & (table["n_nonmanifold_edges"] == 0) & (table["n_inconsistent_edges"] == 0) & (table["n_patches"] == 1) & (euler <= 2) & ((2 - euler) % 2 == 0)
    table["genus"] = np.where(surface, (2 - euler) // 2, -1)
    # boundary components: boundary edges joined at shared vertices
    b = ends[faces == 1]
    on_boundary = np.zeros(nv, bool)
    on_boundary[b.ravel()] = True
    broot = _roots(nv, b[:, 0], b[:, 1])
    n_bc = int((on_boundary & (broot == np.arange(nv))).sum())
    # duplicates
    _, group, odd = _vertex_sets(t, live)
    ng = group.max() + 1 if len(group) else 0
    p, m = np.bincount(group[odd == 0], minlength=ng), np.bincount(group[odd == 1], minlength=ng)
    n_b, n_nm, n_inc = int((faces == 1).sum()), int((faces >= 3).sum()), int(inc_edge.sum())
    stats = dict(n_verts_used=int(used.sum()), n_tris=nt, n_degenerate=int((~live).sum()), n_edges=len(faces), n_boundary_edges=n_b, n_manifold_edges=int((faces == 2).sum()),
                 n_nonmanifold_edges=n_nm, n_inconsistent_edges=n_inc, max_faces_on_edge=int(faces.max()) if len(faces) else 0, n_duplicate_tris=int(live.sum()) - int(ng),
                 n_folded_pairs=int(np.minimum(p, m).sum()), n_components=nc, n_patches=len(patch_first), n_unorientable_patches=int(unorientable.sum()),
                 n_boundary_components=n_bc, closed=int(n_b == 0 and n_nm == 0), oriented=int(n_b == 0 and n_nm == 0 and n_inc == 0),
                 euler=int(used.sum()) - len(faces) + int(live.sum()))
    return dict(n_faces=he["n_faces"].astype(np.uint32), n_same=he["n_same"].astype(np.uint32), mate=he["mate"].astype(np.uint32), table=table, stats=stats)


def expected_repair(verts, indices, colors=None, normals=None, weld=False, drop_degenerate=True, duplicates="first", orient="none"):
    """What rnb_mesh_repair returns: dict(verts, indices, [colors], [normals], vertex_map, stats) + `tri_kept` and `tri_flipped` per input triangle."""
    assert duplicates in ("keep", "first", "cancel") and orient in ("none", "consistent")
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    nv, nt = len(v), len(t)
    if nt and t.max() >= nv:
        raise ValueError("index out of range")
    rep = np.arange(nv)
    n_welded = 0
    if weld:  # 1. used vertices at one position become the lowest-indexed of them (-0 equals +0)
        used = np.zeros(nv, bool)
        used[t.ravel()] = True
        u = np.flatnonzero(used)
        if not np.isfinite(v[u]).all():
            raise ValueError("a used vertex is not finite")
        pos = v[u] + np.float32(0.0)  # -0 + 0 = +0
        _, first, inv = np.unique(pos.view(np.uint32).reshape(-1, 3), axis=0, return_index=True, return_inverse=True)  # first: of each position the lowest row = the lowest index
        rep[u] = u[first[inv.ravel()]]
        n_welded = int((rep != np.arange(nv)).sum())
        t = rep[t]
    nondeg = _nondegenerate(t)
    there = nondeg | (not drop_degenerate)  # 2.
    n_deg = int((~there).sum())
    live = there & nondeg
    n_dup = 0
    if duplicates != "keep":  # 3.
        ids, group, odd = _vertex_sets(t, live)
        ng = group.max() + 1 if len(group) else 0
        stay = np.zeros(len(ids), bool)
        if duplicates == "first":
            first = np.full(ng, nt, np.int64)
            np.minimum.at(first, group, ids)
            stay = first[group] == ids
        else:
            p, m = np.bincount(group[odd == 0], minlength=ng), np.bincount(group[odd == 1], minlength=ng)
            majority_odd = m > p
            left = np.abs(p - m)
            order = np.lexsort((ids, odd, group))  # group by group, winding by winding, ascending number
            g, o = group[order], odd[order]
            start = np.r_[True, (g[1:] != g[:-1]) | (o[1:] != o[:-1])] if len(order) else np.empty(0, bool)
            rank = np.arange(len(order)) - np.maximum.accumulate(np.where(start, np.arange(len(order)), 0)) if len(order) else np.empty(0, np.int64)
            stay[order] = (o == majority_odd[g]) & (p[g] != m[g]) & (rank < left[g])
        gone = ids[~stay]
        n_dup = len(gone)
        there = there.copy()
        there[gone] = False
        live = there & nondeg
    flip = np.zeros(nt, bool)
    n_patches = n_unorientable = 0
    if orient == "consistent":  # 4.
        he = _half_edges(t, live)
        cover = _cover(t, live, he)
        h1, h2 = he["pairs"]
        proot = _roots(nt, h1 // 3, h2 // 3)
        r0, r1 = cover[0::2], cover[1::2]
        firsts = np.flatnonzero(live & (proot == np.arange(nt)))  # a patch is named by its lowest-numbered triangle
        n_patches, n_unorientable = len(firsts), int((r0[firsts] == r1[firsts]).sum())
        members = np.flatnonzero(live & (r0 != r1))  # the triangles of the orientable patches
        in_a = r0 > r1  # sheet A of a patch: "flip exactly these"; sheet B: the other triangles of the patch
        size_a = np.bincount(proot[members][in_a[members]], minlength=nt)
        size_b = np.bincount(proot[members][~in_a[members]], minlength=nt)
        take_a = (size_a < size_b) | ((size_a == size_b) & ~in_a)  # per patch (indexed by its first triangle): A flips fewer, or as many and leaves the first alone
        flip[members] = in_a[members] == take_a[proot[members]]
    tk = t[there]
    fl = flip[there]
    tk = np.where(fl[:, None], tk[:, [0, 2, 1]], tk)
    vkeep = np.zeros(nv, bool)
    vkeep[tk.ravel()] = True
    vmap = np.cumsum(vkeep) - vkeep
    out = dict(verts=v[vkeep], indices=vmap[tk].astype(np.uint32).ravel(), tri_kept=there, tri_flipped=flip,
               vertex_map=np.where(vkeep[rep], vmap[rep], NONE).astype(np.uint32))
    if colors is not None:
        out["colors"] = np.asarray(colors, np.float32).reshape(-1, 3)[vkeep]
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(-1, 3)[vkeep]
    out["stats"] = dict(n_welded=n_welded, n_degenerate_dropped=n_deg, n_duplicates_dropped=n_dup, n_flipped=int(flip.sum()), n_patches=n_patches,
                        n_unorientable_patches=n_unorientable, n_verts_in=nv, n_verts_out=int(vkeep.sum()), n_tris_in=nt, n_tris_out=int(there.sum()))
    return out


def assert_equal_bits(got, want):
    """A dict DeviceMesh.topology / Context.mesh_topology or Context.repair_mesh returned against expected_topology / expected_repair: every array `want` holds bit
    for bit (the repair's attributes must be there exactly when `want` has them), the table, the counts of the statistics."""
    for key in ("verts", "indices", "colors", "normals", "vertex_map", "n_faces", "n_same", "mate"):
        if "verts" in want and key in ("colors", "normals"):
            assert (key in got) == (key in want), key
        if key in want:
            assert key in got, key
            g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
            assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (key, int((g != w).sum()))
    if "table" in want:
        assert got["table"].dtype == TABLE_DTYPE and got["table"].tobytes() == want["table"].tobytes(), (got["table"], want["table"])
    st = got.get("repair_stats", got.get("stats", got)) if "verts" in want else got.get("stats", got)
    for key, val in want["stats"].items():
        assert st[key] == val, (key, st[key], val)


def max_key_multiplicity(verts, indices):
    """The most items any grouping of the header puts on one key: half-edges per edge, triangles per vertex set, used vertices per position."""
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    if not len(t):
        return 0
    e = np.sort(np.stack([t.ravel(), t[:, [1, 2, 0]].ravel()], 1), axis=1)
    used = np.unique(t)
    pos = (np.asarray(verts, np.float32).reshape(-1, 3)[used] + np.float32(0)).view(np.uint32).reshape(-1, 3)
    return max(int(np.unique(x, axis=0, return_counts=True)[1].max()) for x in (e, np.sort(t, axis=1), pos))


# ---------------------------------------------------------------------------------------------------------------------------- meshes
def cube():
    """8 vertices, 12 triangles, closed, wound outward."""
    v = np.float32([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]) * np.float32(0.5) + np.float32(0.25)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = np.array([tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))], np.int64)
    return v, t


def tetrahedron():
    v = np.float32([[0.2, 0.2, 0.2], [0.8, 0.2, 0.2], [0.2, 0.8, 0.2], [0.2, 0.2, 0.8]])
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int64)


def _grid_tris(nu, nv_, wrap_u, wrap_v):
    """Two triangles per cell of a grid of nu x nv_ cells, vertex (i, j) = i * cols + j; a wrapped axis has as many vertex rows as cells, an open one more."""
    rows, cols = (nu if wrap_u else nu + 1), (nv_ if wrap_v else nv_ + 1)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv_), indexing="ij")
    i, j = i.ravel(), j.ravel()
    a, b = i * cols + j, ((i + 1) % rows) * cols + j
    c, d = ((i + 1) % rows) * cols + (j + 1) % cols, i * cols + (j + 1) % cols
    return rows, cols, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])


def torus_grid(n):
    """V = n^2, E = 3 n^2, F = 2 n^2, genus 1."""
    rows, cols, t = _grid_tris(n, n, True, True)
    u, w = np.meshgrid(np.arange(rows) * 2 * np.pi / n, np.arange(cols) * 2 * np.pi / n, indexing="ij")
    r = 0.3 + 0.1 * np.cos(w)
    v = np.stack([0.5 + r * np.cos(u), 0.5 + r * np.sin(u), 0.5 + 0.1 * np.sin(w)], -1).reshape(-1, 3).astype(np.float32)
    return v, t


def annulus(n):
    """A ring of n cells, one cell wide: 2 n vertices, 2 n triangles, two boundary loops."""
    rows, cols, t = _grid_tris(n, 1, True, False)
    u = np.arange(rows) * 2 * np.pi / n
    v = np.stack([np.stack([0.5 + r * np.cos(u), 0.5 + r * np.sin(u), np.full(n, 0.5)], -1) for r in (0.2, 0.3)], 1).reshape(-1, 3).astype(np.float32)
    return v, t


def moebius(n):
    """The annulus of n cells (2 n triangles) closed with a half twist: one boundary loop, unorientable."""
    v, t = annulus(n)
    u = np.arange(n) * 2 * np.pi / n
    w = np.stack([0.1 * np.cos(u / 2), 0.1 * np.sin(u / 2)], 0)
    v = np.stack([np.stack([0.5 + (0.3 + s * w[0]) * np.cos(u), 0.5 + (0.3 + s * w[0]) * np.sin(u), 0.5 + s * w[1]], -1) for s in (-1, 1)], 1).reshape(-1, 3).astype(np.float32)
    t = t.copy()
    last = (t >= 2 * (n - 1)).any(1) & (t < 2).any(1)  # the triangles of the closing cell: their vertices 0 and 1 change places
    swap = np.array([1, 0] + list(range(2, 2 * n)))
    t[last] = np.where(t[last] < 2, swap[t[last]], t[last])
    return v, t


def disc(n):
    """A fan of n triangles around vertex 0: n + 1 vertices, one boundary loop."""
    u = np.arange(n) * 2 * np.pi / n
    v = np.concatenate([[[0.5, 0.5, 0.5]], np.stack([0.5 + 0.3 * np.cos(u), 0.5 + 0.3 * np.sin(u), np.full(n, 0.5)], 1)]).astype(np.float32)
    k = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + k, 1 + (k + 1) % n], 1)


def two_cubes_sharing_an_edge():
    """14 vertices, 24 triangles: two cubes that touch along one edge, which then carries four faces."""
    v, t = cube()
    w = v + np.float32([0.5, 0.5, 0.0])  # the second cube's vertices 0 and 4 (x, y low) are the first's 3 and 7 (x, y high)
    new = np.array([3, 8, 9, 10, 7, 11, 12, 13])
    keep = [1, 2, 3, 5, 6, 7]
    return np.concatenate([v, w[keep]]), np.concatenate([t, new[t]])


def book(m):
    """m triangles around the edge (0, 1): m + 2 vertices."""
    u = np.arange(m) * 2 * np.pi / m
    v = np.concatenate([[[0.5, 0.5, 0.3], [0.5, 0.5, 0.7]], np.stack([0.5 + 0.3 * np.cos(u), 0.5 + 0.3 * np.sin(u), np.full(m, 0.5)], 1)]).astype(np.float32)
    return v, np.stack([np.zeros(m, np.int64), np.ones(m, np.int64), 2 + np.arange(m)], 1)


def strip(n):
    """A zigzag strip of n triangles, consistently wound: n + 2 vertices along x."""
    k = np.arange(n + 2)
    v = np.stack([k / (n + 2.0), 0.01 * (k % 2), np.full(n + 2, 0.5)], 1).astype(np.float32)
    a = np.arange(n)
    return v, np.where((a % 2 == 0)[:, None], np.stack([a, a + 1, a + 2], 1), np.stack([a + 1, a, a + 2], 1))


def sphere(res=32):
    """The marching-cubes sphere of tests.mesh_simplify_reference.sphere_mesh: closed, consistently wound, genus 0."""
    from tests import mesh_simplify_reference as msr
    v, i = msr.sphere_mesh(res)
    return v, np.asarray(i, np.int64).reshape(-1, 3)


def soup(v, t):
    """Every corner its own vertex: 3 nt vertices, triangle k = (3k, 3k+1, 3k+2)."""
    t = np.asarray(t, np.int64).reshape(-1, 3)
    return np.asarray(v, np.float32)[t.ravel()], np.arange(3 * len(t)).reshape(-1, 3)


def flip_some(t, fraction, seed):
    """A copy of t with a random `fraction` of the triangles reversed (second and third index swapped)."""
    t = np.asarray(t, np.int64).reshape(-1, 3).copy()
    sel = np.random.default_rng(seed).random(len(t)) < fraction
    t[sel] = t[sel][:, [0, 2, 1]]
    return t


def renumber(v, t, rng):
    """The same mesh under a random numbering of its vertices -> (verts, tris, new_of_old)."""
    new_of_old = rng.permutation(len(v))
    out = np.empty_like(v)
    out[new_of_old] = v
    return out, new_of_old[np.asarray(t, np.int64)], new_of_old


def _clustered(dist, dims=8):
    from tests import mesh_checks, mesh_simplify_reference as msr
    v, i = mesh_checks.host_marching_cubes(dist.astype(np.float32))
    out = msr.expected(v, i, origin=(0.0, 0.0, 0.0), cell=1.0 / dims, dims=dims)
    return out["verts"], out["indices"].reshape(-1, 3).astype(np.int64)


def _lattice(res=64):
    g = np.arange(res, dtype=np.float64) / res
    return np.meshgrid(g, g, g, indexing="ij")  # z, y, x


def clustered_slab(dims=8):
    """The 64^3 marching-cubes surface of the slab |x-.5|, |y-.5| <= .3, |z-.5603| <= .011 after vertex clustering on dims^3 cells: folded pairs throughout."""
    z, y, x = _lattice()
    return _clustered(np.maximum(np.maximum(np.abs(x - 0.5) - 0.3, np.abs(y - 0.5) - 0.3), np.abs(z - 0.5603) - 0.011), dims)


def clustered_thin_torus(dims=8):
    """Likewise for the torus of major radius .3 and tube radius .031 in the plane z = .5603."""
    z, y, x = _lattice()
    ring = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2) - 0.3
    return _clustered(np.sqrt(ring ** 2 + (z - 0.5603) ** 2) - 0.031, dims)
