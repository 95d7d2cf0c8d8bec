"""The numpy statement of include/rnb_mesh_raster.h, rules 1-7, operation for operation: int64 edge functions, float64 everywhere else (numpy rounds every operation on
its own, and never fuses a multiply with an add). All (triangle, pixel) candidates of the pixel boxes are laid out flat, so a mesh of tens of thousands of small
triangles and a pair of screen-filling ones cost the same few array operations."""
import numpy as np

CHANNELS, NONE, MAX_SIZE, SMALL_PIXELS, MAX_COUNT, MAX_COORD_LOG2 = 9, 0xFFFFFFFF, 16384, 16, 1 << 24, 28
CULL = {"none": 0, "back": 1, "front": 2}
CHUNK = 1 << 21  # candidates per pass


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _edge(px, py, qx, qy, x, y):
    return (qx - px) * (y - py) - (qy - py) * (x - px)


def setup(verts, indices, view, near=2.0 ** -10, cull="none"):
    """Rules 1-4 up to the pixel box, for every triangle at once. Returns a dict: cls (0 behind, 1 out of range, 2 degenerate, 3 culled, 4 offscreen, 5 small, 6 large),
    and for the triangles of class 5 and 6 (`live`, ascending) X, Y int64 [n,3], r = 1 / zc [n,3], vid [n,3] (swapped where front-facing), A2 > 0, back, box (i0, i1, j0, j1)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)
    w, h = int(view["width"]), int(view["height"])
    x = np.asarray(view["xform"], np.float32).reshape(3, 4).astype(np.float64)
    fx, fy = (np.float64(np.float32(f)) for f in view["focal_length"])
    cxw = np.float64(np.float32(view["principal_point"][0])) * np.float64(w)
    cyh = np.float64(np.float32(view["principal_point"][1])) * np.float64(h)
    nt = len(t)
    cls = np.full(nt, -1, np.int64)
    with np.errstate(all="ignore"):
        e = v[t] - x[:, 3]  # [nt,3,3]
        xc, yc, zc = (_dot(x[:, k], e) for k in range(3))
        front = (zc >= np.float64(np.float32(near))).all(axis=1)
        sx = fx * (xc / zc) + cxw
        sy = fy * (yc / zc) + cyh
        r = 1.0 / zc
        fX, fY = np.floor(sx * 256.0 + 0.5), np.floor(sy * 256.0 + 0.5)
        lim = float(1 << MAX_COORD_LOG2)
        ok = (np.isfinite(sx) & np.isfinite(sy) & (np.abs(fX) <= lim) & (np.abs(fY) <= lim)).all(axis=1)
    cls[~front] = 0
    cls[front & ~ok] = 1
    go = front & ok
    X = np.where(go[:, None], fX, 0.0).astype(np.int64)
    Y = np.where(go[:, None], fY, 0.0).astype(np.int64)
    a2 = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    cls[go & (a2 == 0)] = 2
    go &= a2 != 0
    back = a2 > 0
    culled = go & (back if CULL[cull] == 1 else ~back if CULL[cull] == 2 else np.zeros(nt, bool))
    cls[culled] = 3
    go &= ~culled
    order = np.where(back[:, None], np.array([0, 1, 2]), np.array([0, 2, 1]))  # b and c swapped where front-facing
    rows = np.arange(nt)[:, None]
    X, Y, r, vid = X[rows, order], Y[rows, order], r[rows, order], t[rows, order]
    a2 = np.abs(a2)
    i0 = np.maximum(0, (X.min(axis=1) - 128 + 255) >> 8)
    i1 = np.minimum(w - 1, (X.max(axis=1) - 128) >> 8)
    j0 = np.maximum(0, (Y.min(axis=1) - 128 + 255) >> 8)
    j1 = np.minimum(h - 1, (Y.max(axis=1) - 128) >> 8)
    empty = (i0 > i1) | (j0 > j1)
    cls[go & empty] = 4
    go &= ~empty
    area = np.where(go, (i1 - i0 + 1) * (j1 - j0 + 1), 0)
    cls[go & (area <= SMALL_PIXELS)] = 5
    cls[go & (area > SMALL_PIXELS)] = 6
    live = np.nonzero(go)[0]
    return dict(cls=cls, live=live, X=X[live], Y=Y[live], r=r[live], vid=vid[live], a2=a2[live], back=back[live], box=(i0[live], i1[live], j0[live], j1[live]), area=area[live], w=w, h=h)


def _weights(s, k, i, j):
    """Rule 4 for triangles s[...][k] at pixels (i, j): the weights [n,3] and the coverage."""
    px, py = 256 * i + 128, 256 * j + 128
    X, Y = s["X"][k], s["Y"][k]
    ws, cov = [], np.ones(len(k), bool)
    for c in range(3):
        p, q = (c + 1) % 3, (c + 2) % 3
        wc = _edge(X[:, p], Y[:, p], X[:, q], Y[:, q], px, py)
        dx, dy = X[:, q] - X[:, p], Y[:, q] - Y[:, p]
        cov &= (wc > 0) | ((wc == 0) & ((dy > 0) | ((dy == 0) & (dx > 0))))
        ws.append(wc)
    return np.stack(ws, axis=1), cov


def _depth(s, k, wk):
    l = wk.astype(np.float64) / s["a2"][k].astype(np.float64)[:, None]
    r = s["r"][k]
    iz = (l[:, 0] * r[:, 0] + l[:, 1] * r[:, 1]) + l[:, 2] * r[:, 2]
    return 1.0 / iz, l


def rasterize(verts, indices, view, colors=None, normals=None, near=2.0 ** -10, cull="none", shading="face"):
    """Returns dict(image float32 [H,W,9], faces uint32 [H,W], counts uint32 [H,W] (unsaturated), ties uint32 [H,W] (covering triangles with the winner's float depth),
    stats)."""
    s = setup(verts, indices, view, near, cull)
    w, h = s["w"], s["h"]
    n_pix = w * h
    keys = np.full(n_pix, np.iinfo(np.uint64).max, np.uint64)
    counts = np.zeros(n_pix, np.int64)
    i0, i1, j0, j1 = s["box"]
    area = s["area"]
    n_live = len(s["live"])
    frag_pix, frag_bits = [], []
    start = 0
    while start < n_live:  # whole triangles per pass, CHUNK candidates at most (one triangle at least)
        stop = start + max(1, int(np.searchsorted(np.cumsum(area[start:]), CHUNK, side="right")))
        k = np.repeat(np.arange(start, stop), area[start:stop])
        off = np.arange(len(k)) - np.repeat(np.cumsum(area[start:stop]) - area[start:stop], area[start:stop])
        bw = (i1 - i0 + 1)[k]
        i, j = i0[k] + off % bw, j0[k] + off // bw
        wk, cov = _weights(s, k, i, j)
        k, i, j, wk = k[cov], i[cov], j[cov], wk[cov]
        z, _ = _depth(s, k, wk)
        bits = z.astype(np.float32).view(np.uint32).astype(np.uint64)
        pix = j * w + i
        np.minimum.at(keys, pix, (bits << np.uint64(32)) | s["live"][k].astype(np.uint64))
        np.add.at(counts, pix, 1)
        frag_pix.append(pix)
        frag_bits.append(bits)
        start = stop
    covered = keys != np.iinfo(np.uint64).max
    ties = np.zeros(n_pix, np.int64)
    if frag_pix:
        fp, fb = np.concatenate(frag_pix), np.concatenate(frag_bits)
        np.add.at(ties, fp[fb == (keys[fp] >> np.uint64(32))], 1)
    # rule 6
    image = np.zeros((n_pix, CHANNELS), np.float32)
    faces = np.full(n_pix, NONE, np.uint32)
    pix = np.nonzero(covered)[0]
    tri = (keys[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    faces[pix] = tri
    k = np.searchsorted(s["live"], tri)
    wk, cov = _weights(s, k, pix % w, pix // w)
    assert cov.all()
    z, l = _depth(s, k, wk)
    m = (l * s["r"][k]) * z[:, None]
    vid = s["vid"][k]
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        if shading == "face":
            t = np.asarray(indices, np.uint32).reshape(-1, 3).astype(np.int64)[tri]
            a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
            u, q = b - a, c - a
            n = np.stack([u[:, 1] * q[:, 2] - u[:, 2] * q[:, 1], u[:, 2] * q[:, 0] - u[:, 0] * q[:, 2], u[:, 0] * q[:, 1] - u[:, 1] * q[:, 0]], axis=1)
        else:
            vn = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
            n = (m[:, 0, None] * vn[vid[:, 0]] + m[:, 1, None] * vn[vid[:, 1]]) + m[:, 2, None] * vn[vid[:, 2]]
        ln = np.sqrt(_dot(n, n))
        image[pix, 0:3] = np.where((ln != 0)[:, None], n / ln[:, None], 0.0).astype(np.float32)
    if colors is not None:
        col = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
        image[pix, 3:6] = ((m[:, 0, None] * col[vid[:, 0]] + m[:, 1, None] * col[vid[:, 1]]) + m[:, 2, None] * col[vid[:, 2]]).astype(np.float32)
    else:
        image[pix, 3:6] = 1.0
    image[pix, 6] = 1.0
    image[pix, 7] = z.astype(np.float32)
    image[pix, 8] = np.minimum(counts[pix], MAX_COUNT).astype(np.float32)
    cls = s["cls"]
    stats = dict(n_tris=len(cls), n_behind=int((cls == 0).sum()), n_out_of_range=int((cls == 1).sum()), n_degenerate=int((cls == 2).sum()), n_culled=int((cls == 3).sum()),
                 n_offscreen=int((cls == 4).sum()), n_small=int((cls == 5).sum()), n_large=int((cls == 6).sum()), n_covered=int(covered.sum()),
                 n_back_pixels=int(s["back"][k].sum()), n_fragments=int(np.minimum(counts, MAX_COUNT).sum()))
    return dict(image=image.reshape(h, w, CHANNELS), faces=faces.reshape(h, w), counts=counts.astype(np.uint32).reshape(h, w), ties=ties.astype(np.uint32).reshape(h, w), stats=stats)


def assert_equal_bits(got, want, faces=True):
    """A dict Context.rasterize_mesh returned against rasterize(): the nine channels and the faces bit for bit, every count of the statistics."""
    g, w = np.ascontiguousarray(got["image"]), want["image"]
    assert g.shape == w.shape and g.dtype == np.float32, (g.shape, w.shape)
    for c in range(CHANNELS):
        bad = np.nonzero(g[..., c].view(np.uint32) != w[..., c].view(np.uint32))
        assert len(bad[0]) == 0, ("channel", c, len(bad[0]), [(int(j), int(i), float(g[j, i, c]), float(w[j, i, c])) for j, i in zip(*bad)][:4])
    if faces:
        assert np.array_equal(got["faces"], want["faces"])
    for key, val in want["stats"].items():
        assert got[key] == val, (key, got[key], val)
