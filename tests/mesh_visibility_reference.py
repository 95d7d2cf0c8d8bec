"""The numpy statement of include/rnb_mesh_visibility.h, both calls, on top of tests/mesh_raster_reference.py (rules 1-5 of the rasteriser are its `setup`, `_weights` and
the winners of `rasterize`; nothing of them is restated here) and the component labels of tests/mesh_clean_reference.py. Integers only: the device has to equal
`measure` and `select` bit for bit."""
import numpy as np

from tests import mesh_clean_reference as cr
from tests import mesh_raster_reference as rr

NONE, MAX_RINGS = 0xFFFFFFFF, 64
RECORD = np.dtype([("n_drawn", "<u4"), ("n_seen", "<u4"), ("n_off_mask", "<u4"), ("best_view", "<u4"), ("best_pixels", "<u4"), ("reserved", "<u4"),
                   ("n_pixels_won", "<u8"), ("n_pixels_covered", "<u8")])
CLASSES = ("n_behind", "n_out_of_range", "n_degenerate", "n_culled", "n_offscreen", "n_small", "n_large")


def on_mask(mask, w, h):
    """bool [h, w]: the pixels of a w x h view that are on `mask` (2-D, any size, non-zero = object; None: all)."""
    if mask is None:
        return np.ones((h, w), bool)
    m = np.asarray(mask)
    mh, mw = m.shape
    mi = np.minimum(mw - 1, ((2 * np.arange(w, dtype=np.int64) + 1) * mw) // (2 * w))
    mj = np.minimum(mh - 1, ((2 * np.arange(h, dtype=np.int64) + 1) * mh) // (2 * h))
    return m[mj][:, mi] != 0


def view_counts(verts, indices, view, mask=None, near=2.0 ** -10, cull="none"):
    """One view: per triangle drawn (bool), cov, on, won (int64), and the classes."""
    s = rr.setup(verts, indices, view, near, cull)
    w, h = s["w"], s["h"]
    nt = len(s["cls"])
    onm = on_mask(mask, w, h).ravel()
    cov, on = np.zeros(nt, np.int64), np.zeros(nt, np.int64)
    i0, i1, j0, j1 = s["box"]
    area = s["area"]
    n_live, start = len(s["live"]), 0
    while start < n_live:  # the candidates of rule 4, laid out flat as the rasteriser's statement does
        stop = start + max(1, int(np.searchsorted(np.cumsum(area[start:]), rr.CHUNK, side="right")))
        k = np.repeat(np.arange(start, stop), area[start:stop])
        off = np.arange(len(k)) - np.repeat(np.cumsum(area[start:stop]) - area[start:stop], area[start:stop])
        bw = (i1 - i0 + 1)[k]
        i, j = i0[k] + off % bw, j0[k] + off // bw
        _, c = rr._weights(s, k, i, j)
        t = s["live"][k[c]]
        np.add.at(cov, t, 1)
        np.add.at(on, t[onm[(j[c] * w + i[c])]], 1)
        start = stop
    faces = rr.rasterize(verts, indices, view, near=near, cull=cull)["faces"].ravel()  # rule 5: the winner of every pixel
    win = faces[(faces != rr.NONE) & onm].astype(np.int64)
    won = np.bincount(win, minlength=nt).astype(np.int64)
    return dict(drawn=s["cls"] >= 5, cov=cov, on=on, won=won, cls=s["cls"], n_pix=w * h)


def measure(verts, indices, views, masks=None, near=2.0 ** -10, cull="none", min_pixels=1):
    """rnb_mesh_visibility: (records RECORD[nt], stats dict)."""
    nt = len(np.asarray(indices).ravel()) // 3
    rec = np.zeros(nt, RECORD)
    rec["best_view"] = NONE
    stats = dict(n_tris=nt, n_views=len(views), n_pixels=0, **{c: 0 for c in CLASSES})
    for v, view in enumerate(views):
        mask = None if masks is None else masks[v]
        c = view_counts(verts, indices, view, mask, near, cull)
        rec["n_drawn"] += c["drawn"].astype(np.uint32)
        rec["n_seen"] += (c["won"] >= min_pixels).astype(np.uint32)
        if mask is not None:
            rec["n_off_mask"] += ((c["cov"] > 0) & (2 * c["on"] < c["cov"])).astype(np.uint32)
        better = c["won"] > rec["best_pixels"]
        rec["best_view"][better] = v
        rec["best_pixels"][better] = c["won"][better]
        rec["n_pixels_won"] += c["won"].astype(np.uint64)
        rec["n_pixels_covered"] += c["cov"].astype(np.uint64)
        for k, name in enumerate(CLASSES):
            stats[name] += int((c["cls"] == k).sum())
        stats["n_pixels"] += c["n_pix"]
    stats["n_faces_seen"] = int((rec["n_seen"] >= 1).sum())
    stats["n_faces_off_mask"] = int((rec["n_off_mask"] >= 1).sum())
    return rec, stats


def select(n_verts, indices, records, unit="component", min_views_seen=1, max_views_off_mask=0xFFFFFFFF, rings=1):
    """rnb_mesh_visibility_select, the decision: (kept uint32[nt], stats dict without the vertex and triangle counts)."""
    t = np.asarray(indices, np.int64).reshape(-1, 3)
    cand = records["n_off_mask"].astype(np.int64) <= max_views_off_mask
    seed = cand & (records["n_seen"].astype(np.int64) >= min_views_seen)
    stats = dict(n_seeds=int(seed.sum()), n_candidates=int(cand.sum()), n_components=0, n_components_kept=0)
    if unit == "face":
        kept = seed.copy()
        for _ in range(rings):
            vm = np.zeros(n_verts, bool)
            vm[t[kept].ravel()] = True
            kept = kept | (cand & vm[t].any(axis=1))
    else:
        lab = cr.labels(n_verts, t)
        tl = lab[t[:, 0]] if len(t) else np.empty(0, np.uint32)
        with_seed = np.unique(tl[seed])
        kept = cand & np.isin(tl, with_seed)
        stats["n_components"] = len(np.unique(tl))
        stats["n_components_kept"] = len(with_seed)
    return kept.astype(np.uint32), stats


def compact(verts, indices, kept, colors=None, normals=None):
    """The output mesh: the vertices a kept triangle uses and the kept triangles, both in input order, renumbered. A dict like the cleaner's."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    t = np.asarray(indices, np.uint32).reshape(-1, 3)[np.asarray(kept) != 0]
    vk = np.zeros(len(v), bool)
    vk[t.ravel()] = True
    vmap = np.cumsum(vk) - vk
    out = dict(verts=v[vk], indices=vmap[t].astype(np.uint32).ravel())
    if colors is not None:
        out["colors"] = np.asarray(colors, np.float32).reshape(-1, 3)[vk]
    if normals is not None:
        out["normals"] = np.asarray(normals, np.float32).reshape(-1, 3)[vk]
    return out
