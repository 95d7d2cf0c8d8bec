"""The scene the visibility tests share (CPU and GPU tier): a hollow ball with a floater beside it, as a marching-cubes mesh in three components, and its cameras."""
import functools

import numpy as np

from tests import mesh_clean_reference as cr
from tests import mesh_raster_reference as rr
from tests import mesh_visibility_reference as vr

BALL, R_OUTER, R_CAVITY = (0.47, 0.52, 0.49), 0.31, 0.17
FLOATER, R_FLOATER = (0.12, 0.14, 0.85), 0.07
N_OUTER, N_CAVITY, N_FLOATER = 3708, 1108, 176


@functools.lru_cache(maxsize=None)
def scene():
    """(verts float32[2502,3], indices uint32[4992*3], part int[4992]: 0 the outer surface, 1 the cavity, 2 the floater) of host_marching_cubes on a 32^3 lattice over
    [0, 1). No lattice value is 0."""
    from tests import mesh_checks
    g = np.arange(32, dtype=np.float64) / 32
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    dist = lambda c: np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    d = np.minimum(np.maximum(dist(BALL) - R_OUTER, R_CAVITY - dist(BALL)), dist(FLOATER) - R_FLOATER)
    assert not (d.astype(np.float32) == 0).any()
    v, i = mesh_checks.host_marching_cubes(d.astype(np.float32))
    t = i.reshape(-1, 3)
    assert (len(v), len(t)) == (2502, 4992)
    lab = cr.labels(len(v), t)[t[:, 0]]
    centre = v[t].astype(np.float64).mean(axis=1)
    far = np.sqrt(((centre - np.array(BALL)) ** 2).sum(axis=1))
    part = np.where(np.sqrt(((centre - np.array(FLOATER)) ** 2).sum(axis=1)) < 2 * R_FLOATER, 2, np.where(far < 0.5 * (R_OUTER + R_CAVITY), 1, 0))
    assert [int((part == k).sum()) for k in range(3)] == [N_OUTER, N_CAVITY, N_FLOATER]
    for k in range(3):  # three components, one per part
        assert len(np.unique(lab[part == k])) == 1
    assert len(np.unique(lab)) == 3
    v.setflags(write=False), i.setflags(write=False), part.setflags(write=False)
    return v, i, part


def views(w, h, f, n=6):
    from tests.test_mesh_raster_cpu import fibonacci_view
    return [fibonacci_view(k, n, w, h, f) for k in range(n)]


@functools.lru_cache(maxsize=None)
def ball_masks(w, h, f, n=6):
    """Per view the coverage of the ball without the floater, by the reference rasteriser: uint8 [h, w]."""
    v, i, part = scene()
    t = i.reshape(-1, 3)[part != 2]
    return tuple((rr.rasterize(v, t.ravel(), view)["faces"] != rr.NONE).astype(np.uint8) for view in views(w, h, f, n))


@functools.lru_cache(maxsize=None)
def reference(w, h, f, masks=None, min_pixels=1, drop=0):
    """measure() of the scene (without its last `drop` triangles) in views(w, h, f); masks: None or the (mw, mh, mf) of ball_masks. Computed once, never modified."""
    v, i, _ = scene()
    i = i[:len(i) - 3 * drop]
    rec, st = vr.measure(v, i, views(w, h, f), None if masks is None else ball_masks(*masks), min_pixels=min_pixels)
    rec.setflags(write=False)
    return rec, st
