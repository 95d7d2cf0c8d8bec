"""The numpy statement of include/rnb_mesh_draw.h, T1-T6, operation for operation, on the statement of the rasteriser (tests/mesh_raster_reference.py: its fill, its
rule 6 and its setup / _weights / _depth for the winner's weights) and the conventions of the texture baker (tests/mesh_texture_reference.py: V = 1 at the top row, texel
centres at integers). float64 everywhere, every operation rounded on its own."""
import numpy as np

from tests import mesh_raster_reference as mr
from tests import mesh_texture_reference as tr

FILTERS = {"nearest": 0, "bilinear": 1}
MAX_TEXTURE_SIZE = tr.MAX_SIZE
BRANCHES = ("bad_uv", "normal_fallback", "clamped_tap", "unowned_tap", "small_fill", "large_fill")


def winner_weights(verts, indices, view, faces, near=2.0 ** -10, cull="none"):
    """For the covered pixels of `faces` (uint32 [H,W], NONE where nothing covers): (pix flat indices, m float64 [n,3] of rule 6, vid int64 [n,3] the vertices in the
    swapped order, back bool [n], cls of the winners' triangles (5 small, 6 large))."""
    s = mr.setup(verts, indices, view, near, cull)
    w = s["w"]
    f = np.asarray(faces).reshape(-1)
    pix = np.nonzero(f != mr.NONE)[0]
    tri = f[pix].astype(np.int64)
    k = np.searchsorted(s["live"], tri)
    wk, cov = mr._weights(s, k, pix % w, pix // w)
    assert cov.all()
    z, l = mr._depth(s, k, wk)
    m = (l * s["r"][k]) * z[:, None]
    return pix, m, s["vid"][k], s["back"][k], s["cls"][tri]


def draw(verts, indices, view, uv, color=None, normal=None, colors=None, normals=None, near=2.0 ** -10, cull="none", shading="face", filter="bilinear"):
    """Returns dict(image float32 [H,W,9], faces uint32 [H,W], ties (the rasteriser's), stats (the rasteriser's), n_bad_uv, n_normal_fallback, n_unowned_taps,
    unowned bool [H,W] (the pixels n_unowned_taps counts), tallies: per name of BRANCHES the number of covered pixels that took it; for the two fills the
    number of triangles each path filled)."""
    assert (color is not None or normal is not None) and filter in FILTERS
    base = mr.rasterize(verts, indices, view, colors=colors, normals=normals, near=near, cull=cull, shading=shading)  # T1, and rule 6 for what no map decides
    h, w = base["faces"].shape
    image = base["image"].reshape(-1, mr.CHANNELS).copy()
    maps = [None if a is None else np.asarray(a, np.float32).astype(np.float64) for a in (color, normal)]
    size = next(a for a in maps if a is not None).shape[0]
    assert all(a is None or a.shape == (size, size, 4) for a in maps) and 1 <= size <= MAX_TEXTURE_SIZE
    S = np.float64(size)
    pix, m, _, back, cls = winner_weights(verts, indices, view, base["faces"], near, cull)
    tri = base["faces"].reshape(-1)[pix].astype(np.int64)
    uv = np.asarray(uv, np.float32).reshape(-1, 3, 2).astype(np.float64)
    assert len(uv) == len(np.asarray(indices).reshape(-1, 3))
    order = np.where(back[:, None], np.array([0, 1, 2]), np.array([0, 2, 1]))  # T2: the corners move with their vertices
    c = uv[tri[:, None], order]  # [n,3,2]
    with np.errstate(all="ignore"):
        U = (m[:, 0] * c[:, 0, 0] + m[:, 1] * c[:, 1, 0]) + m[:, 2] * c[:, 2, 0]
        V = (m[:, 0] * c[:, 0, 1] + m[:, 1] * c[:, 1, 1]) + m[:, 2] * c[:, 2, 1]
        x = U * S - 0.5  # T3
        y = (1.0 - V) * S - 0.5
    bad = ~(np.isfinite(x) & np.isfinite(y))
    ok = ~bad
    xo, yo = x[ok], y[ok]
    xc, yc = np.minimum(np.maximum(xo, -1.0), S), np.minimum(np.maximum(yo, -1.0), S)
    last = size - 1
    clip = lambda a: np.minimum(np.maximum(a, 0), last)
    if filter == "nearest":
        i, j = np.floor(xc + 0.5).astype(np.int64), np.floor(yc + 0.5).astype(np.int64)
        taps = [(clip(j), clip(i))]
        b = [np.ones(len(xc))]
        clamped = (xc != xo) | (yc != yo) | (clip(i) != i) | (clip(j) != j)
    else:
        fi, fj = np.floor(xc), np.floor(yc)
        fu, fv = xc - fi, yc - fj
        i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
        taps = [(clip(j0), clip(i0)), (clip(j0), clip(i0 + 1)), (clip(j0 + 1), clip(i0)), (clip(j0 + 1), clip(i0 + 1))]
        b = [(1.0 - fu) * (1.0 - fv), fu * (1.0 - fv), (1.0 - fu) * fv, fu * fv]
        clamped = (xc != xo) | (yc != yo) | (clip(i0) != i0) | (clip(i0 + 1) != i0 + 1) | (clip(j0) != j0) | (clip(j0 + 1) != j0 + 1)

    def sample(a):
        t = [a[r, q] for r, q in taps]  # [n,4] each
        if filter == "nearest":
            val = t[0][:, :3]
        else:
            with np.errstate(all="ignore"):
                val = ((b[0][:, None] * t[0][:, :3] + b[1][:, None] * t[1][:, :3]) + b[2][:, None] * t[2][:, :3]) + b[3][:, None] * t[3][:, :3]
        un = np.zeros(len(xc), bool)
        for bk, tk in zip(b, t):
            un |= (bk != 0.0) & (tk[:, 3] == 0.0)
        return val, un

    unowned = np.zeros(len(xc), bool)
    good = pix[ok]
    if maps[0] is not None:  # T4
        val, unowned = sample(maps[0])
        image[pix[bad], 3:6] = 0.0
        with np.errstate(all="ignore"):
            image[good, 3:6] = val.astype(np.float32)
    fallback = np.zeros(len(xc), bool)
    if maps[1] is not None:  # T5
        val, un = sample(maps[1])
        if maps[0] is None:
            unowned = un
        with np.errstate(all="ignore"):
            ln = np.sqrt(mr._dot(val, val))
            has = np.isfinite(ln) & (ln > 0.0)
            unit = (val / ln[:, None]).astype(np.float32)
        image[good[has], 0:3] = unit[has]
        fallback = ~has
    flag = np.zeros(h * w, bool)
    flag[good[unowned]] = True
    tallies = dict(bad_uv=int(bad.sum()), normal_fallback=int(fallback.sum()), clamped_tap=int(clamped.sum()), unowned_tap=int(unowned.sum()), small_fill=base["stats"]["n_small"],
                   large_fill=base["stats"]["n_large"])
    return dict(image=image.reshape(h, w, mr.CHANNELS), faces=base["faces"], ties=base["ties"], stats=base["stats"], n_bad_uv=int(bad.sum()), n_normal_fallback=int(fallback.sum()),
                n_unowned_taps=int(unowned.sum()), unowned=flag.reshape(h, w), tallies=tallies)


def surface_points(verts, indices, view, faces, near=2.0 ** -10, cull="none"):
    """(pix, points float64 [n,3]): (m_a * v_a + m_b * v_b) + m_c * v_c of every covered pixel, the point of the winner under the pixel's centre."""
    pix, m, vid, _, _ = winner_weights(verts, indices, view, faces, near, cull)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    return pix, (m[:, 0, None] * v[vid[:, 0]] + m[:, 1, None] * v[vid[:, 1]]) + m[:, 2, None] * v[vid[:, 2]]


def assert_equal_bits(got, want, faces=True):
    """A dict DeviceMesh.draw_textured returned against draw(): the image, the faces and the rasteriser's counts as mesh_raster_reference.assert_equal_bits compares them,
    and the three counts of the draw."""
    mr.assert_equal_bits(got, want, faces)
    for key in ("n_bad_uv", "n_normal_fallback", "n_unowned_taps"):
        assert got[key] == want[key], (key, got[key], want[key])
