"""The plain numpy statement of what rnb_extract_mesh returns (include/rnb_mesh.h): given the dense lattice, the dense mesh D of that lattice, the occupancy
bitfield, the brick size and the lattice's placement, which bricks are kept / evaluated / keep an edge table, and which triangles of D remain.

Lattices are arrays [rz, ry, rx] (x fastest), brick masks [nbz, nby, nbx]. The brick / cell intersection is float64, in the order of operations of the device's
classification kernel (which is double precision too), so the two agree exactly. Meshes are compared order-free: a triangle is the three position bit patterns of
its corners, rotated so that the smallest corner comes first (orientation kept); a mesh is the sorted list of those."""
import numpy as np

from tests import mc_numpy
from tests.render_reference import CASCADES, GRIDSIZE, morton3d


def n_bricks(res, brick):
    """res = (rx, ry, rz) -> bricks per axis (nbx, nby, nbz)."""
    return tuple((int(r) + brick - 1) // brick for r in res)


def occupancy_cells(bitfield, mip):
    """bool [128, 128, 128] indexed [z, y, x]: the cells of cascade `mip` whose bit is set and that the march can consult (a cell of cascade m >= 1 inside the cube of
    cascade m - 1 is shadowed by it: mip_from_pos sends every position in there to a finer cascade)."""
    g = np.arange(GRIDSIZE, dtype=np.uint32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    idx = morton3d(x.ravel(), y.ravel(), z.ravel()).astype(np.int64)
    byte = np.asarray(bitfield, np.uint8)[idx // 8 + (GRIDSIZE ** 3 // 8) * mip]
    occ = ((byte >> (idx % 8).astype(np.uint8)) & 1).astype(bool).reshape(GRIDSIZE, GRIDSIZE, GRIDSIZE)
    if mip:
        q = GRIDSIZE // 4
        occ[q:3 * q, q:3 * q, q:3 * q] = False
    return occ


def _integral(a):
    """Summed-volume table with a zero border: S[k, j, i] = a[:k, :j, :i].sum()."""
    s = np.zeros(tuple(n + 1 for n in a.shape), np.int64)
    s[1:, 1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    return s


def _box_sums(s, lo, hi):
    """Sums of the table's array over the boxes [lo_k, hi_k) per axis (z, y, x), every combination of the per-axis interval lists -> [nz, ny, nx]."""
    (z0, y0, x0), (z1, y1, x1) = lo, hi
    ix = np.ix_
    return (s[ix(z1, y1, x1)] - s[ix(z0, y1, x1)] - s[ix(z1, y0, x1)] - s[ix(z1, y1, x0)]
            + s[ix(z0, y0, x1)] + s[ix(z0, y1, x0)] + s[ix(z1, y0, x0)] - s[ix(z0, y0, x0)])


def brick_interval(res_k, brick, lattice_min, lattice_max):
    """Per brick along one axis: the closed interval of its lattice points grown by one step, in the lattice's own space (float64)."""
    lmin, size = np.float64(np.float32(lattice_min)), np.float64(np.float32(lattice_max)) - np.float64(np.float32(lattice_min))
    first = np.arange(0, res_k, brick, dtype=np.float64)
    last = np.minimum(first + brick, res_k) - 1.0
    return lmin + (first - 1.0) / np.float64(res_k) * size, lmin + (last + 1.0) / np.float64(res_k) * size


def kept_mask(res, brick, bitfield, lattice_min=0.0, lattice_max=1.0):
    """bool [nbz, nby, nbx]. bitfield None = cull NONE: every brick."""
    nb = n_bricks(res, brick)
    kept = np.zeros(nb[::-1], bool)
    if bitfield is None:
        kept[:] = True
        return kept
    iv = [brick_interval(res[k], brick, lattice_min, lattice_max) for k in range(3)]  # x, y, z
    for mip in range(CASCADES):
        occ = occupancy_cells(bitfield, mip)
        if not occ.any():
            continue
        h = np.float64(1 << mip) / np.float64(GRIDSIZE)
        lo, hi, ok = [], [], []
        for k in (2, 1, 0):  # z, y, x
            ua = np.clip((iv[k][0] - 0.5) / h + 0.5 * GRIDSIZE, -1e6, 1e6)
            ub = np.clip((iv[k][1] - 0.5) / h + 0.5 * GRIDSIZE, -1e6, 1e6)
            f = np.maximum(np.ceil(ua).astype(np.int64) - 1, 0)       # cells i with i + 1 >= ua ...
            l = np.minimum(np.floor(ub).astype(np.int64), GRIDSIZE - 1)  # ... and i <= ub: closed boxes, touching counts
            ok.append(l >= f)
            lo.append(np.where(l >= f, f, 0))
            hi.append(np.where(l >= f, l + 1, 0))
        n = _box_sums(_integral(occ), lo, hi)
        kept |= (n > 0) & ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    return kept


def evaluated_mask(kept):
    """A brick is evaluated if it or a brick at -1 along any subset of the axes is kept (the far corners of a kept brick's cells)."""
    ev = kept.copy()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ev[dz:, dy:, dx:] |= kept[:kept.shape[0] - dz, :kept.shape[1] - dy, :kept.shape[2] - dx]
    return ev


def _per_point(mask, shape, brick):
    """A brick mask expanded to the lattice points."""
    rz, ry, rx = shape
    return np.repeat(np.repeat(np.repeat(mask, brick, 0), brick, 1), brick, 2)[:rz, :ry, :rx]


def sign_change_mask(density, evaluated, brick, thresh=0.0):
    """Evaluated bricks whose box grown by one step towards +x, +y, +z holds, among the lattice points of evaluated bricks, values on both sides of thresh."""
    d = np.asarray(density, np.float32)
    rz, ry, rx = d.shape
    avail = _per_point(evaluated, d.shape, brick)
    above = (d > np.float32(thresh)) & avail
    below = ~(d > np.float32(thresh)) & avail
    lo = [np.arange(0, r, brick) for r in (rz, ry, rx)]
    hi = [np.minimum(l + brick + 1, r) for l, r in zip(lo, (rz, ry, rx))]
    return evaluated & (_box_sums(_integral(above), lo, hi) > 0) & (_box_sums(_integral(below), lo, hi) > 0)


def triangle_cells(density, thresh=0.0):
    """int [n_triangles, 3] (x, y, z): the cell of every triangle of the dense mesh, in the dense path's order (cells ascending in lattice order, then table order)."""
    table = mc_numpy.triangle_table()
    per_case = np.array([len(t) // 3 for t in table], np.int64)
    d = np.asarray(density, np.float32)
    rz, ry, rx = d.shape
    if min(rz, ry, rx) < 2:
        return np.zeros((0, 3), np.int64)
    inside = d > np.float32(thresh)
    mask = np.zeros((rz - 1, ry - 1, rx - 1), np.int32)
    for c, (cx, cy, cz) in enumerate(mc_numpy.CORNER):
        mask |= inside[cz:cz + rz - 1, cy:cy + ry - 1, cx:cx + rx - 1].astype(np.int32) << c
    mask[mask == 255] = 0
    z, y, x = np.nonzero(mask)
    return np.repeat(np.stack([x, y, z], axis=1), per_case[mask[z, y, x]], axis=0)


def triangle_keys(verts, idx):
    """uint32 [n, 9], rows sorted: the corners' position bit patterns, each triangle rotated so that its smallest corner (lexicographically, as unsigned bit patterns)
    comes first (of two equal corners, the rotation with the smaller row). Two meshes hold the same triangles, with multiplicity, iff these arrays are equal."""
    v = np.ascontiguousarray(verts, np.float32).view(np.uint32).reshape(-1, 3)
    t = v[np.asarray(idx, np.int64).reshape(-1, 3)].astype(np.uint64)  # [n, 3 corners, 3 coords]
    if len(t) == 0:
        return np.zeros((0, 9), np.uint32)
    n = len(t)
    rots = [t[:, [r, (r + 1) % 3, (r + 2) % 3]].reshape(n, 9).astype(np.uint32) for r in range(3)]

    def less(a, b):  # rows of a lexicographically below rows of b
        diff = a != b
        first = diff.argmax(1)
        rows = np.arange(n)
        return diff.any(1) & (a[rows, first] < b[rows, first])

    keys = rots[0]
    for r in rots[1:]:
        keys = np.where(less(r, keys)[:, None], r, keys)
    return keys[np.lexsort(keys.T[::-1])]


def vertex_keys(verts):
    """uint32 [n, 3], rows sorted: the positions' bit patterns."""
    v = np.ascontiguousarray(verts, np.float32).view(np.uint32).reshape(-1, 3)
    return v[np.lexsort(v.T[::-1])] if len(v) else v


def expected(density, dense_verts, dense_idx, bitfield, brick, lattice_min=0.0, lattice_max=1.0, thresh=0.0):
    """The statement. density [rz, ry, rx]; (dense_verts, dense_idx) the dense mesh D of that lattice and threshold (marching cubes in lattice order); bitfield None
    for cull NONE. Returns dict: kept / evaluated / sign_change (brick masks), keep (bool per triangle of D), verts / indices (D restricted to the kept triangles, its
    vertices renumbered in D's order), triangles / vertices (the order-free keys)."""
    d = np.asarray(density, np.float32)
    rz, ry, rx = d.shape
    kept = kept_mask((rx, ry, rz), brick, bitfield, lattice_min, lattice_max)
    ev = evaluated_mask(kept)
    cells = triangle_cells(d, thresh)
    tri = np.asarray(dense_idx, np.int64).reshape(-1, 3)
    assert len(cells) == len(tri), "the dense mesh is not the marching cubes of this lattice (%d triangles, %d expected)" % (len(tri), len(cells))
    keep = kept[cells[:, 2] // brick, cells[:, 1] // brick, cells[:, 0] // brick] if len(cells) else np.zeros(0, bool)
    used = np.unique(tri[keep])
    remap = np.full(len(dense_verts), -1, np.int64)
    remap[used] = np.arange(len(used))
    verts = np.asarray(dense_verts, np.float32)[used]
    idx = remap[tri[keep]].astype(np.uint32).ravel()
    return dict(kept=kept, evaluated=ev, sign_change=sign_change_mask(d, ev, brick, thresh), keep=keep, cells=cells, verts=verts, indices=idx,
                triangles=triangle_keys(verts, idx), vertices=vertex_keys(verts))


def set_cell_boxes(bitfield):
    """float64 [n, 3] lower and upper corners (x, y, z) of every consultable set cell of every cascade: the cull rule's other operand, spelled out cell by cell
    (used to check kept_mask independently of its index arithmetic)."""
    lo, hi = [], []
    for mip in range(CASCADES):
        z, y, x = np.nonzero(occupancy_cells(bitfield, mip))
        i = np.stack([x, y, z], axis=1).astype(np.float64)
        h = float(1 << mip) / GRIDSIZE
        lo.append(0.5 + (i - GRIDSIZE // 2) * h)
        hi.append(0.5 + (i + 1 - GRIDSIZE // 2) * h)
    return np.concatenate(lo), np.concatenate(hi)


def brick_meets_a_set_cell(bx, by, bz, res, brick, boxes, lattice_min=0.0, lattice_max=1.0):
    """The cull rule for one brick by direct comparison of its grown box with every set cell's box (closed)."""
    lo, hi = boxes
    ok = np.ones(len(lo), bool)
    for k, b in enumerate((bx, by, bz)):
        a0, a1 = brick_interval(res[k], brick, lattice_min, lattice_max)
        ok &= (lo[:, k] <= a1[b]) & (hi[:, k] >= a0[b])
    return bool(ok.any())
