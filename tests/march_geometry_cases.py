"""Inputs of the march-geometry tests (test_march_geometry_cpu.py, test_gpu_march_geometry.py), as plain numpy: camera families the ring of
synthetic.make_scene never produces, caller-written occupancy shapes, and the predicates -- computed from the ORACLE's outputs only -- that say
a case exercises what it claims. A helper module: no test lives here.

Single-cascade cases (aabb_scale 1, box [0, 1]^3). A family is (views, normal maps, albedo maps); in the maps red is 0 over the left half of the
image and 65535 elsewhere, alpha 65535, so that the reference's "red <= 0" draw (testbed_nerf.cu:1264) is taken by some rays of every view and not
by others. Images are 9 to 33 pixels wide; the reference's snap of an image position does not floor, so the rays of a view are spread continuously over it.
"""
import numpy as np

from rnb_neus2_amd.synthetic import look_at_c2w

STEP = float(np.float32(np.sqrt(np.float32(3.0)) / np.float32(1024.0)))  # MIN_CONE_STEPSIZE: the constant march step of a single-cascade scene
MAX_STEPS = 1024                                                         # RNB_MAX_STEPS
N0 = 128 ** 3 // 8                                                       # bytes of one cascade of the bitfield
CENTRE = np.array([0.5, 0.5, 0.5])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# views
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _view(eye, target, w, h=None, fx=None, fy=None, pp=(0.5, 0.5)):
    h = w if h is None else h
    fx = 0.8 * w if fx is None else fx
    fy = fx * h / w if fy is None else fy
    c2w = look_at_c2w(np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64))
    return dict(width=int(w), height=int(h), focal_length=(float(fx), float(fy)), principal_point=(float(pp[0]), float(pp[1])), xform=c2w.astype(np.float32))


def _axis_view(eye, axis, sign, w, fx, fy, h=None):
    """A camera whose rotation has only 0 and +-1 entries: forward = sign * e_axis, right and down the two other axes."""
    fwd = np.zeros(3)
    fwd[axis] = sign
    right = np.zeros(3)
    right[(axis + 1) % 3] = 1.0
    down = np.cross(fwd, right)
    m = np.zeros((3, 4))
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = right, down, fwd, eye
    h = w if h is None else h
    return dict(width=int(w), height=int(h), focal_length=(float(fx), float(fy)), principal_point=(0.5, 0.5), xform=m.astype(np.float32))


def maps_for(views):
    normals, albedos = [], []
    for v in views:
        m = np.full((v["height"], v["width"], 4), 65535, dtype=np.uint16)
        m[:, : v["width"] // 2, 0] = 0
        normals.append(m)
        albedos.append(m.copy())
    return normals, albedos


def _inside():
    # in empty space and inside cells that the shapes below occupy (the shell at radius 0.27, cell (64,64,64), a blob of two_blobs), looking across the box
    return [_view((0.5, 0.5, 0.5), (1.0, 0.62, 0.41), 17),
            _view((0.1, 0.2, 0.3), (0.9, 0.8, 0.7), 21),
            _view((0.77, 0.5, 0.5), (0.0, 0.3, 0.4), 9),
            _view((0.503, 0.504, 0.505), (0.45, 0.55, 1.0), 33),
            _view((0.999, 0.52, 0.47), (0.0, 0.5, 0.5), 13),
            _view((0.36, 0.5, 0.5), (1.0, 0.5, 0.52), 15)]


def _near_face():
    # 1e-4, 0.01, 0.1 and 0.24 outside a face; the last one narrow, so that even its corner rays enter the box below t = 0.25
    return [_view((-1e-4, 0.45, 0.55), (0.5, 0.5, 0.5), 17, fx=0.7 * 17),
            _view((0.52, 1.01, 0.47), (0.5, 0.5, 0.5), 21, fx=0.7 * 21),
            _view((0.55, 0.48, -0.1), (0.5, 0.5, 0.5), 13, fx=1.0 * 13),
            _view((1.24, 0.5, 0.5), (0.5, 0.5, 0.5), 25, fx=4.0 * 25)]


def _binade_edges():
    # the box entry 4 steps below t = 0.25, 0.5, 1, 2, 4 (a start offset of up to one step on top): the first round of 16 positions crosses the binade boundary.
    # Narrow views (focal length (6 + 6 T) widths: the corner pixel's 1 / cos - 1 stays below 3 steps / T), one per face
    out = []
    for k, (T, axis, sign) in enumerate(((0.25, 0, 1), (0.5, 1, 1), (1.0, 2, 1), (2.0, 0, -1), (4.0, 1, -1))):
        d = T - 4.0 * STEP
        eye = CENTRE.copy()
        eye[axis] = -d if sign > 0 else 1.0 + d
        eye[(axis + 1) % 3] += 0.013 * (k + 1)
        tgt = eye.copy()
        tgt[axis] = 0.5
        w = (9, 13, 17, 21, 11)[k]
        out.append(_view(eye, tgt, w, fx=(6.0 + 6.0 * T) * w))
    return out


def _far():
    # distance 3 .. 20 from the centre; the focal length grows with it so that the image still covers the box. The first one looks along the x axis (two_blobs' axis)
    out = []
    for k, (dist, d) in enumerate(((3.0, (-1, 0, 0)), (6.0, (1, 1, 0.3)), (9.0, (0.2, -1, 0.5)), (14.0, (0.1, 0.05, 1)), (20.0, (-1, 0.4, -0.7)))):
        d = np.asarray(d, dtype=np.float64)
        eye = CENTRE + dist * d / np.linalg.norm(d)
        w = (33, 17, 21, 25, 29)[k]
        out.append(_view(eye, CENTRE, w, fx=w * dist / 1.2))
    return out


def _axis():
    # all six axis directions through the centre from distance 1.5. Finite focal lengths: a telephoto view of the centre (a pixel is 1/1024 of the box there: the 10 x 10
    # image is 1.25 cells wide -- a quarter of its rays go through cell (64,64,64), all of them along the axis of two_blobs or through its gap). focal_length[0] = inf:
    # (xy - pp) * w / inf is exactly 0, so one direction component is an exact zero on every ray; 1e38: a component of ~1e-37, non-zero and below the 1e-12f of the
    # bounding-box stop's axis branch. Those two fan out in the other image axis by +-7 degrees (12 rows: none through the centre itself).
    out = []
    for fx_kind in ("finite", "inf", "tiny"):
        for axis in range(3):
            for sign in (1, -1):
                eye = CENTRE.copy()
                eye[axis] -= sign * 1.5
                if fx_kind == "finite":
                    out.append(_axis_view(eye, axis, sign, 10, 1.5 * 1024, 1.5 * 1024))
                else:
                    out.append(_axis_view(eye, axis, sign, 11 if fx_kind == "inf" else 13, np.inf if fx_kind == "inf" else 1e38, 4.0 * 12, h=12))
    return out


def _graze():
    # eyes in the plane of the face x = 0 and 1e-6 / 1e-3 to either side of it, looking along the face (odd widths: the centre column of pixels lies in the eye's plane);
    # and along the edge x = 0, y = 0
    out = []
    for k, dx in enumerate((0.0, 1e-6, -1e-6, 1e-3, -1e-3)):
        out.append(_view((dx, -0.3, 0.5), (dx, 0.5, 0.5), (17, 13, 15, 21, 19)[k], fx=1.1 * (17, 13, 15, 21, 19)[k]))
    out.append(_view((0.0, 0.0, -0.3), (0.0, 0.0, 0.5), 23, fx=1.1 * 23))
    # ... and a view whose rays run IN the low face x = 0: looking along +y with an infinite focal length in the image axis that is the world's x, so that the x component of
    # every direction is an exact zero, from an eye at x = 2^-27 (at x = 0 itself the reference's slab test divides 0 by 0 and the ray misses the box). Every position of
    # every ray has x = 2^-27: |fl(x - 0.5)| = 0.5, the positions the reference looks up in cascade 1
    out.append(_axis_view(np.array([2.0 ** -27, -0.3, 0.5]), 1, 1, 17, 1.1 * 17, np.inf))
    return out


def _diagonal():
    # just outside a corner, looking at the opposite one, both ways, and from further out. The snap of the image position does not floor, so no pixel is exactly the
    # principal axis: the last two views have both focal lengths infinite, every ray of theirs IS the diagonal (three equal direction components), 1024.9 steps long
    return [_view((-0.01, -0.01, -0.01), (1.0, 1.0, 1.0), 9, fx=1.5 * 9),
            _view((1.01, 1.01, 1.01), (0.0, 0.0, 0.0), 9, fx=1.5 * 9),
            _view((-0.002, -0.002, -0.002), (1.0, 1.0, 1.0), 11, fx=2.5 * 11),
            _view((-0.3, -0.3, -0.3), (1.0, 1.0, 1.0), 13, fx=2.0 * 13),
            _view((-0.01, -0.01, -0.01), (1.0, 1.0, 1.0), 9, fx=np.inf),
            _view((1.01, 1.01, 1.01), (0.0, 0.0, 0.0), 9, fx=np.inf)]


def _wide():
    # focal = 0.3 x width from distance 1.2: many rays miss the box, others cut a corner in less than a step; one non-square view with fx != fy and an off-centre principal point
    out = []
    for k, d in enumerate(((1, 0.2, 0.1), (0.3, -0.5, -0.8))):
        d = np.asarray(d, dtype=np.float64)
        w = (21, 33)[k]
        out.append(_view(CENTRE + 1.2 * d / np.linalg.norm(d), CENTRE, w, fx=0.3 * w))
    d = np.array([-0.4, -0.8, 0.45])
    out.append(_view(CENTRE + 1.2 * d / np.linalg.norm(d), CENTRE, 33, h=17, fx=0.3 * 33, fy=0.45 * 17, pp=(0.31, 0.64)))
    return out


FAMILIES = {"inside": _inside, "near_face": _near_face, "binade_edges": _binade_edges, "far": _far, "axis": _axis, "graze": _graze, "diagonal": _diagonal, "wide": _wide}
OUTSIDE = ("far", "axis", "diagonal", "wide")  # "the outside cameras" of the skip properties (eyes at 0.3 and more from the box among their views)


def family(name):
    views = FAMILIES[name]()
    normals, albedos = maps_for(views)
    return views, normals, albedos


# multi-cascade cameras: the box is [0.5 - s/2, 0.5 + s/2]^3 in the same coordinates
def multi_cascade_family(name, aabb_scale):
    s = float(aabb_scale)
    if name == "inside":  # inside the big box: outside the unit cube, on its face, inside it
        views = [_view((0.5 - 0.45 * s, 0.5 + 0.1 * s, 0.5), (0.5, 0.5, 0.5), 17), _view((0.0, 0.3, 0.6), (1.0, 0.6, 0.5), 21), _view((0.5, 0.5, 0.5), (0.5 + s, 0.7, 0.3), 13),
                 _view((0.5 + 0.49 * s, 0.5 - 0.3 * s, 0.5 + 0.2 * s), (0.5, 0.5, 0.5), 25, fx=0.5 * 25)]
    elif name == "far":
        views = []
        for k, (dist, d) in enumerate(((3.0, (-1, 0, 0)), (6.0, (1, 1, 0.3)), (9.0, (0.2, -1, 0.5)), (14.0, (0.1, 0.05, 1)), (20.0, (-1, 0.4, -0.7)))):
            d = np.asarray(d, dtype=np.float64)
            w = (33, 17, 21, 25, 29)[k]
            views.append(_view(CENTRE + dist * d / np.linalg.norm(d), CENTRE, w, fx=w * dist / (1.2 * s)))
    elif name == "axis":
        views = []
        for fx_kind in ("finite", "inf", "tiny"):
            for axis in range(3):
                for sign in (1, -1):
                    eye = CENTRE.copy()
                    eye[axis] -= sign * 1.5 * s
                    fx = {"finite": 1.3 * 11, "inf": np.inf, "tiny": 1e38}[fx_kind]
                    views.append(_axis_view(eye, axis, sign, 11, fx, 1.3 * 11))
    else:
        raise KeyError(name)
    normals, albedos = maps_for(views)
    return views, normals, albedos


# ---------------------------------------------------------------------------------------------------------------------------------------------
# occupancy shapes: cascade 0 of DENSITY_BITFIELD in Morton order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _spread(v):
    v = v.astype(np.uint32)
    v = (v * 0x00010001) & 0xFF0000FF
    v = (v * 0x00000101) & 0x0F00F00F
    v = (v * 0x00000011) & 0xC30C30C3
    v = (v * 0x00000005) & 0x49249249
    return v


def morton_bits(occ):
    """occ[z, y, x] (128^3 booleans) -> the 128^3 / 8 bytes of one cascade of the bitfield (bit i of the field = the cell with Morton code i)."""
    i = np.arange(128)
    morton = _spread(i)[None, None, :] | (_spread(i)[None, :, None] << 1) | (_spread(i)[:, None, None] << 2)
    bits = np.zeros(128 ** 3, dtype=np.uint8)
    bits[morton.ravel()] = np.asarray(occ, dtype=bool).ravel()
    return np.packbits(bits, bitorder="little")


def _cell_centres():
    g = (np.arange(128) + 0.5) / 128 - 0.5
    return np.meshgrid(g, g, g, indexing="ij")  # z, y, x


def shell_bitfield(radius, half_width):
    """Cascade-0 bitfield (Morton order, 128^3 cells) of a spherical shell around the cube's centre."""
    z, y, x = _cell_centres()
    return morton_bits(np.abs(np.sqrt(x * x + y * y + z * z) - radius) < half_width)


def _cells(*cells):
    occ = np.zeros((128, 128, 128), dtype=bool)
    for (x, y, z) in cells:
        occ[z, y, x] = True
    return occ


def _sheets(axis):
    occ = np.zeros((128, 128, 128), dtype=bool)
    for k in (0, 63, 64, 127):
        if axis == "x":
            occ[:, :, k] = True
        else:
            occ[:, k, :] = True
    return occ


def _blocks_checker():
    b = np.indices((32, 32, 32)).sum(axis=0) % 2 == 0
    return np.repeat(np.repeat(np.repeat(b, 4, axis=0), 4, axis=1), 4, axis=2)


def _cells_checker():
    z, y, x = _cell_centres()
    cube = (np.abs(x) < 0.15) & (np.abs(y) < 0.15) & (np.abs(z) < 0.15)
    return cube & (np.indices((128, 128, 128)).sum(axis=0) % 2 == 0)


def _two_blobs(gap_steps):
    """Two spheres of radius 0.05 on the x axis through the centre, `gap_steps` march steps of empty space between their surfaces."""
    z, y, x = _cell_centres()
    half = 0.05 + 0.5 * gap_steps * STEP
    return ((x + half) ** 2 + y * y + z * z < 0.05 ** 2) | ((x - half) ** 2 + y * y + z * z < 0.05 ** 2)


def _noise():
    rng = np.random.default_rng(20240607)
    b = np.zeros(N0, dtype=np.uint8)
    idx = rng.choice(N0, size=N0 // 100, replace=False)
    b[idx] = rng.integers(1, 256, size=idx.size, dtype=np.uint8)
    return b


def _planes_1():
    occ = np.zeros((128, 128, 128), dtype=bool)
    occ[:, :, 1] = occ[:, 1, :] = occ[1, :, :] = True  # one cell in from the low faces: a position ON such a face lies in an EMPTY cell of cascade 0, under an occupied one of cascade 1
    return occ


# Shapes whose coarser cascades are the max-pool pyramid that update_density_bitfield builds (bitfield_max_pool: cascade k + 1 holds, in its central 64^3 cells, the 2x2x2
# maxima of cascade k; the rest of it stays empty at aabb_scale 1). Every other shape leaves cascades 1 .. 7 empty.
POOLED = {"pooled_dense": lambda: np.ones((128, 128, 128), dtype=bool), "pooled_planes_1": _planes_1}


def pyramid(occ, n_cascades):
    """occ[z, y, x] of cascade 0 -> the bytes of n_cascades cascades."""
    out = [morton_bits(occ)]
    for _ in range(1, n_cascades):
        nxt = np.zeros((128, 128, 128), dtype=bool)
        nxt[32:96, 32:96, 32:96] = occ.reshape(64, 2, 64, 2, 64, 2).any(axis=(1, 3, 5))
        occ = nxt
        out.append(morton_bits(occ))
    return np.concatenate(out)


TWO_BLOB_GAPS = (30, 60, 120)
SHAPES = {
    "pooled_dense": lambda: morton_bits(POOLED["pooled_dense"]()),
    "pooled_planes_1": lambda: morton_bits(POOLED["pooled_planes_1"]()),
    "dense": lambda: np.full(N0, 0xFF, dtype=np.uint8),
    "one_cell_mid": lambda: morton_bits(_cells((64, 64, 64))),
    "one_cell_lo": lambda: morton_bits(_cells((0, 0, 0))),
    "one_cell_hi": lambda: morton_bits(_cells((127, 127, 127))),
    "sheets_x": lambda: morton_bits(_sheets("x")),
    "sheets_y": lambda: morton_bits(_sheets("y")),
    "blocks_checker": lambda: morton_bits(_blocks_checker()),
    "cells_checker": lambda: morton_bits(_cells_checker()),
    "two_blobs_30": lambda: morton_bits(_two_blobs(30)),
    "two_blobs_60": lambda: morton_bits(_two_blobs(60)),
    "two_blobs_120": lambda: morton_bits(_two_blobs(120)),
    "thin_shell": lambda: shell_bitfield(0.27, 0.012),
    "noise": _noise,
}
_shape_cache = {}


def shape(name):
    """The cascade-0 bytes of a shape (cached, read-only)."""
    if name not in _shape_cache:
        b = np.ascontiguousarray(SHAPES[name](), dtype=np.uint8)
        assert b.size == N0
        b.setflags(write=False)
        _shape_cache[name] = b
    return _shape_cache[name]


def bitfield(name, total_bytes):
    """A whole DENSITY_BITFIELD: the shape in cascade 0; the other cascades empty, or (POOLED) its max-pool pyramid."""
    if name in POOLED:
        if (name, total_bytes) not in _shape_cache:
            _shape_cache[(name, total_bytes)] = pyramid(POOLED[name](), total_bytes // N0)
        return _shape_cache[(name, total_bytes)].copy()
    bf = np.zeros(total_bytes, dtype=np.uint8)
    bf[:N0] = shape(name)
    return bf


def multi_cascade_shell(total_bytes):
    """thin_shell in cascade 0 under coarser cascades that are all ones. ALL of them, not cascade 1 alone: the cascade consulted is max(mip of the position, mip of dt), and
    dt = t / 256 puts every position beyond t = 2 into cascade 2 or coarser wherever it lies -- under an empty cascade 2 the cameras outside the box would march nothing."""
    bf = bitfield("thin_shell", total_bytes)
    bf[N0:] = 0xFF
    return bf


def n_blocks(name):
    """Non-empty 4^3 blocks of a shape (a block is 8 consecutive bytes of the Morton-ordered field); the march kernels hold at most 4096 of them in LDS."""
    return int(np.count_nonzero(shape(name).reshape(-1, 8).any(axis=1)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# What each view of each (family, shape) pair is declared to yield at 4200 rays, n_rays_total 0. Written down here, not computed: the CPU tier holds every view of every
# pair to its class. Every view NOT listed in EXPECTS_NONE is `expects_samples`: at least MIN_RAYS kept rays with a sample. EXPECTS_NONE: not one.
# The image position of a ray is continuous (the reference's snap does not floor), so a view that merely has a small target somewhere in its field -- one cell, a blob of radius
# 0.05 under a wide lens -- gets a handful of rays onto it whatever the inputs, neither 0 nor 20. A pair with such a view cannot be declared in these two classes and is NOT
# part of the tests: EXCLUDED_PAIRS, 25 of the 120 pairs (every family and every shape still runs in the others; the small targets are met by the families that aim at them:
# `axis` with its telephoto views, `diagonal` through the corner cells, `inside` from within them).
# ---------------------------------------------------------------------------------------------------------------------------------------------
MIN_RAYS = 20
N_RAYS = 4200
BIG_SHAPES = ("dense", "pooled_dense", "pooled_planes_1", "blocks_checker", "cells_checker", "sheets_x", "sheets_y")  # more than 16 << 14 samples at 4200 rays from some family: these run in contexts with target_batch_size 1 << 18
EXPECTS_NONE = {
    ("inside", "pooled_planes_1"): (1, 3, 5),
    ("inside", "one_cell_mid"): (1, 4, 5),
    ("inside", "one_cell_lo"): (0, 1, 2, 3, 4, 5),
    ("inside", "one_cell_hi"): (0, 1, 2, 3, 4, 5),
    ("inside", "two_blobs_30"): (3,),
    ("inside", "two_blobs_60"): (3,),
    ("inside", "two_blobs_120"): (3,),
    ("near_face", "one_cell_mid"): (0, 1, 2),
    ("near_face", "one_cell_lo"): (0, 1, 2, 3),
    ("near_face", "one_cell_hi"): (1, 2, 3),
    ("binade_edges", "one_cell_lo"): (0, 1, 2, 3, 4),
    ("binade_edges", "one_cell_hi"): (0, 1, 2, 3, 4),
    ("binade_edges", "two_blobs_60"): (1,),
    ("binade_edges", "two_blobs_120"): (1, 2, 4),
    ("far", "one_cell_mid"): (0, 1, 2, 3, 4),
    ("far", "one_cell_lo"): (0, 1, 2, 3, 4),
    ("far", "one_cell_hi"): (0, 1, 2, 3, 4),
    ("axis", "one_cell_lo"): (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17),
    ("axis", "one_cell_hi"): (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17),
    ("axis", "two_blobs_30"): (2, 3, 4, 5, 10, 11, 16, 17),
    ("axis", "two_blobs_60"): (2, 3, 4, 5, 10, 11, 16, 17),
    ("axis", "two_blobs_120"): (2, 3, 4, 5, 10, 11, 16, 17),
    ("axis", "noise"): (2, 3),
    ("graze", "dense"): (6,),
    ("graze", "one_cell_mid"): (0, 1, 2, 3, 4, 5, 6),
    ("graze", "one_cell_lo"): (0, 1, 2, 3, 4, 5, 6),
    ("graze", "one_cell_hi"): (0, 1, 2, 3, 4, 5, 6),
    ("graze", "sheets_x"): (6,),
    ("graze", "sheets_y"): (6,),
    ("graze", "blocks_checker"): (6,),
    ("graze", "cells_checker"): (6,),
    ("graze", "two_blobs_30"): (0, 1, 2, 3, 4, 5, 6),
    ("graze", "two_blobs_60"): (1, 2, 4, 5, 6),
    ("graze", "two_blobs_120"): (5, 6),
    ("graze", "thin_shell"): (6,),
    ("graze", "noise"): (6,),
    ("diagonal", "one_cell_mid"): (2, 3),
    ("diagonal", "one_cell_lo"): (1,),
    ("diagonal", "one_cell_hi"): (0, 2, 3),
    ("diagonal", "two_blobs_30"): (4, 5),
    ("diagonal", "two_blobs_60"): (4, 5),
    ("diagonal", "two_blobs_120"): (4, 5),
    ("wide", "one_cell_mid"): (0, 1, 2),
    ("wide", "one_cell_lo"): (0, 1, 2),
    ("wide", "one_cell_hi"): (0, 1, 2),
    ("wide", "two_blobs_120"): (1,),
}
EXCLUDED_PAIRS = (
    ("inside", "pooled_planes_1"),
    ("inside", "one_cell_mid"),
    ("inside", "two_blobs_30"),
    ("inside", "two_blobs_60"),
    ("near_face", "one_cell_mid"),
    ("near_face", "one_cell_hi"),
    ("binade_edges", "one_cell_mid"),
    ("far", "two_blobs_30"),
    ("far", "two_blobs_60"),
    ("far", "two_blobs_120"),
    ("axis", "one_cell_mid"),
    ("axis", "sheets_x"),
    ("axis", "sheets_y"),
    ("graze", "cells_checker"),
    ("graze", "two_blobs_60"),
    ("graze", "two_blobs_120"),
    ("graze", "thin_shell"),
    ("diagonal", "one_cell_mid"),
    ("diagonal", "one_cell_lo"),
    ("diagonal", "two_blobs_120"),
    ("wide", "cells_checker"),
    ("wide", "two_blobs_30"),
    ("wide", "two_blobs_60"),
    ("wide", "two_blobs_120"),
    ("wide", "thin_shell"),
)
PAIRS = [(f, s) for f in FAMILIES for s in SHAPES if (f, s) not in EXCLUDED_PAIRS]


def view_classes(family_name, shape_name, n_views):
    none = EXPECTS_NONE.get((family_name, shape_name), ())
    return ["none" if v in none else "samples" for v in range(n_views)]


def class_of(count):
    return "none" if count == 0 else "undeclarable" if count < MIN_RAYS else "samples"


def own_density_grid(aabb_scale, _cache={}):
    """The density grid the oracle builds itself at step 0 (every cell sampled; the initial weights alone decide, not the views). Once per aabb_scale."""
    from tests import oracle_lib
    if aabb_scale not in _cache:
        c = oracle_lib.context(target_batch_size=1 << 14, aabb_scale=aabb_scale, max_rays_per_batch=1 << 13, initial_rays_per_batch=512, apply_no_albedo=1)
        try:
            c.init_params()
            c.set_dataset(*multi_cascade_family("inside", aabb_scale))
            c.set_training_step(0)
            c.update_density_grid()
            _cache[aabb_scale] = c.get("DENSITY_GRID").copy()
        finally:
            c.close()
    return _cache[aabb_scale]


def on_face(xyz):
    """|p - 0.5| = 0.5 in some coordinate, as the reference's float subtraction rounds it (mip_from_pos: frexp exponent 0): the position is looked up in cascade 1."""
    return np.abs(np.asarray(xyz, dtype=np.float32) - np.float32(0.5)).max(axis=-1) >= np.float32(0.5)


OVERFLOW_SHAPE = "thin_shell"  # the one case per family that overflows on purpose
SKIP_PAIRS = [("far", "thin_shell"), ("axis", "thin_shell"), ("diagonal", "thin_shell"), ("axis", "two_blobs_30"), ("axis", "two_blobs_60"), ("axis", "two_blobs_120"),
              ("diagonal", "one_cell_hi")]  # pairs of an outside family and a small target: long empty stretches
MULTI_CASCADE_FAMILIES = ("inside", "far", "axis")


def batch_size(big):
    return 1 << 18 if big else 1 << 14


def overflow_max_samples(marched):
    return int(0.6 * marched)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's march, and predicates over its outputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Marched:
    """The outputs of one generate_training_samples call, copied out of a context."""

    def __init__(self, ctx, n_rays, n_rays_total, n_views):
        c = ctx.get("COUNTERS")
        self.counters = c.copy()
        self.n_rays, self.n_rays_total, self.n_views = n_rays, n_rays_total, n_views
        kept, written = int(c[2]), int(c[3])
        self.kept, self.written = kept, written
        self.ray_indices = ctx.get("RAY_INDICES", kept)
        self.numsteps = ctx.get("NUMSTEPS", kept * 2).reshape(kept, 2)
        self.rays = ctx.get("RAYS", kept * 6).reshape(kept, 6)  # origin, UNNORMALISED direction
        d = self.rays[:, 3:].astype(np.float64)
        self.origins, self.dirs = self.rays[:, :3].astype(np.float64), d / np.linalg.norm(d, axis=1, keepdims=True)
        self.coords = ctx.get("COORDS", written * 7).reshape(written, 7)

    def view_of_ray(self):
        """image_idx of every kept ray: ((i + n_rays_total) * n_images / n_rays) % n_images in uint32 (testbed_nerf.cu:1213)."""
        i = self.ray_indices.astype(np.uint64)
        return ((((i + np.uint64(self.n_rays_total)) * np.uint64(self.n_views)) % np.uint64(1 << 32)) // np.uint64(self.n_rays) % np.uint64(self.n_views)).astype(np.int64)

    def rays_with_samples_per_view(self):
        return np.bincount(self.view_of_ray()[self.numsteps[:, 0] > 0], minlength=self.n_views)

    def sample_t(self):
        """t of every sample = (pos - o) . dir in float64 (warping is the identity at aabb_scale 1), and the index of its ray among the kept ones."""
        n = self.numsteps[:, 0].astype(np.int64)
        ray = np.repeat(np.arange(self.kept), n)
        assert np.array_equal(self.numsteps[:, 1].astype(np.int64), np.concatenate([[0], np.cumsum(n)[:-1]])) and ray.size == self.written
        o, d = self.origins[ray], self.dirs[ray]
        return ((self.coords[:, :3].astype(np.float64) - o) * d).sum(axis=1), ray

    def first_sample_t(self):
        """Distance of each kept ray's first sample from the eye."""
        t, _ = self.sample_t()
        return t[self.numsteps[:, 1].astype(np.int64)]

    def box_entry_t(self):
        o, d = self.origins, self.dirs
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (0.0 - o) / d, (1.0 - o) / d
        lo = np.where(d == 0, -np.inf, np.minimum(ta, tb))
        return np.maximum(lo.max(axis=1), 0.0)

    def longest_empty_run(self):
        """Per kept ray, in lattice steps: (the stretch from the box entry to the first sample, the longest stretch between two consecutive samples; 0 with one sample)."""
        t, ray = self.sample_t()
        first = (t[self.numsteps[:, 1].astype(np.int64)] - self.box_entry_t()) / STEP
        gap = np.zeros(self.kept)
        if t.size > 1:
            dt = np.diff(t) / STEP - 1.0
            same = ray[1:] == ray[:-1]
            np.maximum.at(gap, ray[1:][same], dt[same])
        return first, gap

    def n_exact_zero_component(self):
        return int(np.count_nonzero((self.rays[:, 3:] == 0).any(axis=1)))

    def n_full_length(self):
        return int(np.count_nonzero(self.numsteps[:, 0] == MAX_STEPS))


def march(ctx, bf, n_rays, n_rays_total, max_samples, n_views):
    ctx.put("DENSITY_BITFIELD", bf)
    ctx.generate_training_samples(n_rays, n_rays_total, max_samples)
    return Marched(ctx, n_rays, n_rays_total, n_views)
