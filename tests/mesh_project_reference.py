"""The numpy statement of include/rnb_mesh_project.h, rules P1-P6, operation for operation in float64 (numpy rounds every operation on its own and never fuses a
multiply with an add): ownership, weights and positions from tests/mesh_texture_reference.py, the winner's float depth of every pixel from tests/mesh_raster_reference.py.
What the library's kernels are compared with, bit for bit; nothing here calls the library."""
import numpy as np

from tests import mesh_raster_reference as rr
from tests import mesh_texture_reference as tr

NONE, MAX_WEIGHT_POWER = 0xFFFFFFFF, 8
SKIPS = ("behind", "flat", "offscreen", "occluded", "empty")  # the five ways a (texel, view) pair ends without contributing, in the order P2-P4 decide them


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def decode(image):
    """An image as the kernels read it: float64 [h, w, 4]; a 3-channel image gets alpha 1."""
    a = np.asarray(image)
    assert a.ndim == 3 and a.shape[2] in (3, 4)
    if a.dtype == np.float32:
        d = a.astype(np.float64)
    elif a.dtype == np.uint16:
        d = a.astype(np.float64) / 65535.0
    elif a.dtype == np.uint8:
        d = a.astype(np.float64) / 255.0
    else:
        raise ValueError(a.dtype)
    if d.shape[2] == 3:
        d = np.concatenate([d, np.ones(d.shape[:2] + (1,))], axis=2)
    return d


def texel_normals(verts, indices, tri, a, own, normals="face", vnormals=None):
    """P1: N float64 [m, 3] of the owned texels and valid [m] (a length that is neither 0 nor not finite)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)[tri[own]]
    with np.errstate(all="ignore"):
        if normals == "face":
            p0, p1, p2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
            u, q = p1 - p0, p2 - p0
            s = np.stack([u[:, 1] * q[:, 2] - u[:, 2] * q[:, 1], u[:, 2] * q[:, 0] - u[:, 0] * q[:, 2], u[:, 0] * q[:, 1] - u[:, 1] * q[:, 0]], axis=1)
        else:
            vn = np.asarray(vnormals, np.float32).reshape(-1, 3).astype(np.float64)
            w = a[own].astype(np.float64)
            s = (w[:, 0:1] * vn[idx[:, 0]] + w[:, 1:2] * vn[idx[:, 1]]) + w[:, 2:3] * vn[idx[:, 2]]
        ln = np.sqrt(_dot(s, s))
        valid = (ln != 0) & np.isfinite(ln)
        n = np.where(valid[:, None], s / ln[:, None], 0.0)
    return n, valid


def project(verts, indices, views, images, size, block=0, mode="blend", normals="face", vnormals=None, weight_power=2, min_cos=0.1, depth_tolerance=2.0 ** -8, near=2.0 ** -10,
            cull="none", fallback=None):
    """rnb_mesh_project_views -> dict(uv, color float32[S,S,4], info uint32[S,S,2], block, blocks_per_row, stats, tallies). `tallies` counts, over all (texel, view) pairs
    of texels with a valid normal, how each pair ended: the five SKIPS and `contributed`."""
    assert mode in ("blend", "best") and normals in ("face", "vertex") and 0 <= weight_power <= MAX_WEIGHT_POWER and len(views) == len(images) > 0
    idx = np.asarray(indices, np.uint32).reshape(-1, 3)
    nt = len(idx)
    lay = tr.layout(nt, size, block)
    b, bpr = lay["block"], lay["blocks_per_row"]
    tri, a = tr.ownership(nt, size, b, bpr)
    own = tri >= 0
    m = int(own.sum())
    p = tr.positions(verts, idx, size, b, bpr)[own][:, :3].astype(np.float64)
    N, valid = texel_normals(verts, idx, tri, a, own, normals, vnormals)
    near64, cos64, slack = np.float64(np.float32(near)), np.float64(np.float32(min_cos)), 1.0 + np.float64(np.float32(depth_tolerance))
    A, Q = np.zeros((m, 3)), np.zeros(m)
    bq_c, bq_a = np.zeros((m, 3)), np.zeros(m)
    w_best = np.full(m, -np.inf)
    count, best = np.zeros(m, np.int64), np.full(m, NONE, np.int64)
    tallies = dict.fromkeys(SKIPS + ("contributed",), 0)
    n_tested = n_occluded = 0
    for v, (view, image) in enumerate(zip(views, images)):
        W, H = int(view["width"]), int(view["height"])
        x = np.asarray(view["xform"], np.float32).reshape(3, 4).astype(np.float64)
        fx, fy = (np.float64(np.float32(f)) for f in view["focal_length"])
        cxw = np.float64(np.float32(view["principal_point"][0])) * np.float64(W)
        cyh = np.float64(np.float32(view["principal_point"][1])) * np.float64(H)
        img = decode(image)
        ih, iw = img.shape[:2]
        if nt:
            ras = rr.rasterize(verts, idx, view, near=near, cull=cull)["image"]
            covered, z_win = ras[..., 6] > 0, ras[..., 7].astype(np.float64)
        else:
            covered, z_win = np.zeros((H, W), bool), np.zeros((H, W))
        with np.errstate(all="ignore"):
            e = p - x[:, 3]
            xc, yc, zc = (_dot(x[:, k], e) for k in range(3))
            go = valid.copy()
            behind = go & (zc < near64)
            go &= ~behind
            d = -e
            c = _dot(N, d) / np.sqrt(_dot(d, d))
            flat = go & ~(c > cos64)
            go &= ~flat
            sx, sy = fx * (xc / zc) + cxw, fy * (yc / zc) + cyh
            fi, fj = np.floor(sx), np.floor(sy)
            inside = np.isfinite(sx) & np.isfinite(sy) & (fi >= 0) & (fi < W) & (fj >= 0) & (fj < H)
            off = go & ~inside
            go &= inside
            i, j = np.where(go, fi, 0).astype(np.int64), np.where(go, fj, 0).astype(np.int64)
            occluded = go & covered[j, i] & (zc > z_win[j, i] * slack)
            n_tested += int(go.sum())
            n_occluded += int(occluded.sum())
            go &= ~occluded
            u, w = sx * np.float64(iw) / np.float64(W) - 0.5, sy * np.float64(ih) / np.float64(H) - 0.5
            u, w = np.where(go, u, 0.0), np.where(go, w, 0.0)
            fu0, fv0 = np.floor(u), np.floor(w)
            fu, fv = u - fu0, w - fv0
            i0, j0 = fu0.astype(np.int64), fv0.astype(np.int64)
            x0, x1 = np.clip(i0, 0, iw - 1), np.clip(i0 + 1, 0, iw - 1)
            y0, y1 = np.clip(j0, 0, ih - 1), np.clip(j0 + 1, 0, ih - 1)
            t = [img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]]
            bw = [(1.0 - fu) * (1.0 - fv), fu * (1.0 - fv), (1.0 - fu) * fv, fu * fv]
            qa = ((bw[0] * t[0][:, 3] + bw[1] * t[1][:, 3]) + bw[2] * t[2][:, 3]) + bw[3] * t[3][:, 3]
            qc = np.stack([((bw[0] * (t[0][:, 3] * t[0][:, k]) + bw[1] * (t[1][:, 3] * t[1][:, k])) + bw[2] * (t[2][:, 3] * t[2][:, k])) + bw[3] * (t[3][:, 3] * t[3][:, k])
                           for k in range(3)], axis=1)
            empty = go & (qa == 0)
            go &= ~empty
            g = np.ones(m)
            for _ in range(weight_power):
                g = g * c
            wv = g * qa
            A[go] += (g[:, None] * qc)[go]
            Q[go] += wv[go]
            count[go] += 1
            better = go & (wv > w_best)
            best[better], w_best[better] = v, wv[better]
            bq_c[better], bq_a[better] = qc[better], qa[better]
        for name, mask in zip(SKIPS, (behind, flat, off, occluded, empty)):
            tallies[name] += int(mask.sum())
        tallies["contributed"] += int(go.sum())
    color = np.zeros((size, size, 4), np.float32)
    info = np.zeros((size, size, 2), np.uint32)
    with np.errstate(all="ignore"):
        rgb = (A / Q[:, None] if mode == "blend" else bq_c / bq_a[:, None]).astype(np.float32)
    got = count > 0
    c4 = np.zeros((m, 4), np.float32)
    c4[:, 3] = 1.0
    if fallback is not None:
        c4[:] = np.asarray(fallback, np.float32)[own]
    c4[got, :3] = rgb[got]
    c4[got, 3] = 1.0
    color[own] = c4
    info[own] = np.stack([count, best], axis=1).astype(np.uint32)
    stats = dict(n_texels=m, n_textured=int(got.sum()), n_pairs_tested=n_tested, n_occluded=n_occluded)
    return dict(uv=tr.uvs(nt, size, b, bpr), color=color, info=info, block=b, blocks_per_row=bpr, stats=stats, tallies=tallies, count=count, own=own,
                positions=p.astype(np.float32))


def assert_equal_bits(got, want):
    """A dict DeviceMesh.project_views returned against project(): uv, color and info in every bit, the four counts of the statistics."""
    assert (got["block"], got["blocks_per_row"]) == (want["block"], want["blocks_per_row"])
    assert np.array_equal(np.ascontiguousarray(got["uv"]).view(np.uint32), want["uv"].view(np.uint32))
    assert np.array_equal(got["info"], want["info"]), int((got["info"] != want["info"]).any(-1).sum())
    g, w = np.ascontiguousarray(got["color"]).view(np.uint32), want["color"].view(np.uint32)
    bad = np.nonzero((g != w).any(-1))
    assert len(bad[0]) == 0, (len(bad[0]), [(int(y), int(x), got["color"][y, x].tolist(), want["color"][y, x].tolist()) for y, x in zip(*bad)][:4])
    for key, val in want["stats"].items():
        assert got["stats"][key] == val, (key, got["stats"][key], val)
