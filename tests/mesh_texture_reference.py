"""The numpy statement of include/rnb_mesh_texture.h: the layout of the per-triangle atlas, the corners' UVs, which triangle owns a texel, and the texel positions
(float64 with every operation rounded on its own and one rounding to float32 at the end, operation for operation the header's formula). What the library's host
function and kernels are compared with, bit for bit; nothing here calls the library."""
import numpy as np

MIN_SIZE, MAX_SIZE, MIN_BLOCK = 4, 8192, 4


class LayoutError(ValueError):
    """The mesh does not fit (or the block is out of range); `smallest` is the smallest size that would hold it with that block (with blocks of 4 for block = 0)."""

    def __init__(self, smallest):
        super().__init__("the smallest size that would fit is %d" % smallest)
        self.smallest = smallest


def _ceil_sqrt(n):
    m = int(np.sqrt(float(n)))
    while m * m > n:
        m -= 1
    while m * m < n:
        m += 1
    return m


def layout(n_tris, size, block=0):
    """-> dict(block, blocks_per_row, n_blocks). Block k holds the triangles 2k and 2k + 1; blocks_per_row = size // b; n_blocks = ceil(n_tris / 2) <= blocks_per_row^2;
    block = 0: the largest b in [4, size] for which that holds."""
    assert MIN_SIZE <= size <= MAX_SIZE
    n_blocks = (n_tris + 1) // 2
    m = _ceil_sqrt(n_blocks)  # the blocks per row the mesh needs
    if block == 0:
        fits = [b for b in range(MIN_BLOCK, size + 1) if (size // b) ** 2 >= n_blocks] if size <= 128 else None  # the definition, where it is cheap to spell out
        b = (size // m if m else size)
        if fits is not None:
            assert (max(fits) if fits else 0) == (b if b >= MIN_BLOCK else 0)
        if b < MIN_BLOCK:
            raise LayoutError(max(MIN_BLOCK * max(m, 1), MIN_SIZE))
    else:
        b = block
        if b < MIN_BLOCK:
            raise LayoutError(max(MIN_BLOCK * max(m, 1), MIN_SIZE))
        if b > size or (size // b) ** 2 < n_blocks:
            raise LayoutError(max(b * max(m, 1), MIN_SIZE))
    return dict(block=b, blocks_per_row=size // b, n_blocks=n_blocks)


def corners(b):
    """Texel-centre indices (ci, cj) of v0, v1, v2 within a block: [0] of the lower triangle, [1] of the upper one (a half-turn of the lower)."""
    n = b - 3
    return np.array([[[0, 0], [n, 0], [0, n]], [[b - 1, b - 1], [b - 1 - n, b - 1], [b - 1, b - 1 - n]]], np.int64)


def uvs(n_tris, size, b, bpr):
    """float32[n_tris, 3, 2]: U = (ox + ci + 0.5) / S, V = 1 - (oy + cj + 0.5) / S in float64, rounded once."""
    t = np.arange(n_tris, dtype=np.int64)
    k = t // 2
    ox, oy = (k % bpr) * b, (k // bpr) * b
    c = corners(b)[t & 1]  # [nt, 3, 2]
    u = ((ox[:, None] + c[..., 0]).astype(np.float64) + 0.5) / np.float64(size)
    v = 1.0 - ((oy[:, None] + c[..., 1]).astype(np.float64) + 0.5) / np.float64(size)
    return np.stack([u, v], axis=-1).astype(np.float32)


def ownership(n_tris, size, b, bpr):
    """-> (tri int64[S, S]: the triangle that owns texel (row y, column x), -1 for none; a int64[S, S, 3]: its integer weights (a0, a1, a2))."""
    y, x = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing="ij")
    bx, by, i, j = x // b, y // b, x % b, y % b
    upper = i + j > b - 1
    tri = 2 * (by * bpr + bx) + upper
    tri = np.where((bx < bpr) & (by < bpr) & (tri < n_tris), tri, -1)
    n = b - 3
    ii, jj = np.where(upper, b - 1 - i, i), np.where(upper, b - 1 - j, j)
    return tri, np.stack([n - ii - jj, ii, jj], axis=-1)


def positions(verts, indices, size, b, bpr):
    """The position map float32[S, S, 4]: p = (float32) (((a0 * v0 + a1 * v1) + a2 * v2) / n) per component in float64, channel 3 = 1; zeros where no triangle owns the texel."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    tri, a = ownership(len(idx), size, b, bpr)
    out = np.zeros((size, size, 4), np.float32)
    own = tri >= 0
    v = verts[idx[tri[own]]].astype(np.float64)  # [m, 3 corners, 3]
    w = a[own].astype(np.float64)  # [m, 3]
    p = ((w[:, 0:1] * v[:, 0] + w[:, 1:2] * v[:, 1]) + w[:, 2:3] * v[:, 2]) / np.float64(b - 3)
    out[own, :3] = p.astype(np.float32)
    out[own, 3] = 1.0
    return out


def edge_texels(size, b, bpr, t, c0, c1):
    """(rows, columns) of the n + 1 texels along the edge from corner c0 to corner c1 (0, 1 or 2) of triangle t, in that direction."""
    k = t // 2
    ox, oy = (k % bpr) * b, (k // bpr) * b
    c = corners(b)[t & 1]
    n = b - 3
    s = np.arange(n + 1, dtype=np.int64)
    ci = c[c0, 0] + (c[c1, 0] - c[c0, 0]) // max(n, 1) * s
    cj = c[c0, 1] + (c[c1, 1] - c[c0, 1]) // max(n, 1) * s
    return oy + cj, ox + ci


def bilinear_taps(x, y):
    """The texels a bilinear lookup at (x, y), in texel-centre coordinates, gives a non-zero weight: [(i, j, weight)]."""
    i0, j0 = int(np.floor(x)), int(np.floor(y))
    fx, fy = x - i0, y - j0
    taps = [(i0, j0, (1 - fx) * (1 - fy)), (i0 + 1, j0, fx * (1 - fy)), (i0, j0 + 1, (1 - fx) * fy), (i0 + 1, j0 + 1, fx * fy)]
    return [t for t in taps if t[2] != 0]


def octahedron(subdivisions=0):
    """A closed, outward-turned mesh around (0.5, 0.5, 0.5), radius 0.3: the octahedron, each triangle split in four `subdivisions` times, the new vertices pushed onto the
    sphere. -> (verts float32[n, 3], tris uint32[m, 3])."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, np.float64) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt((p * p).sum()))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = g
    return (np.array(v) * 0.3 + 0.5).astype(np.float32), np.array(f, np.uint32)
