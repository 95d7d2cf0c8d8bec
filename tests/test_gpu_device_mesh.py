"""DeviceMesh on the MI355X: a chain of stages on the handle gives, bit for bit, what the same stages give through the host-array calls of Context (which are themselves an
upload, the stage and a download on the handle), on three_spheres(32), in one 64 x 48 view, and on the mesh of a small trained model; and a freed handle stops in Python."""
import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_distance_reference as dr
from tests.test_mesh_raster_cpu import fibonacci_view

pytestmark = pytest.mark.gpu

KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
TIMES = ("ms", "ms_grid")


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


@pytest.fixture(scope="module")
def spheres():
    v, i = mc.three_spheres(32)
    assert len(i) // 3 == 1988
    return v, i


@pytest.fixture(scope="module")
def through_the_host(ctx, spheres):
    """clean_mesh, then simplify_mesh on 16^3 cells of the unit box: the two result dicts."""
    cleaned = ctx.clean_mesh(*spheres)
    return cleaned, ctx.simplify_mesh(cleaned["verts"], cleaned["indices"], origin=(0, 0, 0), cell=1.0 / 16, dims=16)


def _timeless(d):
    return {k: (_timeless(v) if isinstance(v, dict) else v) for k, v in d.items() if k not in TIMES}


def test_a_chain_on_the_device_equals_the_chain_through_the_host(ctx, spheres, through_the_host):
    cleaned, simplified = through_the_host
    with ctx.upload_mesh(*spheres) as m, m.clean("largest", "outward") as cm, cm.simplify((0, 0, 0), 1.0 / 16, 16) as sm:
        got = sm.download()
        assert (m.stats, m.n_verts, m.n_triangles, m.has_colors, m.has_normals) == (None, len(spheres[0]), 1988, False, False)
        assert (cm.n_verts, cm.n_triangles, sm.n_verts, sm.n_triangles) == (len(cleaned["verts"]), len(cleaned["indices"]) // 3, len(got["verts"]), len(got["indices"]) // 3)
        assert _timeless(cm.stats) == _timeless(cleaned["stats"]) and _timeless(sm.stats) == _timeless(simplified["stats"])
        assert cm.download()["verts"].tobytes() == cleaned["verts"].tobytes()
    assert sorted(got) == ["indices", "verts"] and 0 < len(got["indices"]) < len(cleaned["indices"]) < len(spheres[1])
    assert got["verts"].tobytes() == simplified["verts"].tobytes() and got["indices"].tobytes() == simplified["indices"].tobytes()


def test_distance_between_two_handles(ctx, spheres):
    b = ctx.simplify_mesh(*spheres, origin=(0, 0, 0), cell=1.0 / 16, dims=16)  # all three spheres on 16^3 cells: the pair of tests/test_gpu_mesh_distance.py
    want = ctx.mesh_distance(*spheres, b["verts"], b["indices"], symmetric=True, per_vertex=True)
    with ctx.upload_mesh(*spheres) as ma, ctx.upload_mesh(b["verts"], b["indices"]) as mb:
        got = ma.distance_to(mb, symmetric=True, per_vertex=True)
    assert sorted(got) == sorted(want) and sorted(got["reverse"]) == sorted(want["reverse"]) and want["mean"] > 0 and want["reverse"]["mean"] > 0
    for g, w in ((got, want), (got["reverse"], want["reverse"])):
        for k in dr.RULE_KEYS + ("max", "mean", "rms"):
            assert g[k] == w[k], k
        for k in ("vert_dist", "vert_nearest"):
            assert g[k].dtype == w[k].dtype and g[k].tobytes() == w[k].tobytes(), k
    assert (got["chamfer"], got["hausdorff"]) == (want["chamfer"], want["hausdorff"])


def test_raster_of_a_handle(ctx, spheres):
    view = fibonacci_view(0, 3, 64, 48, 2.5 * 64)
    want = ctx.rasterize_mesh(*spheres, view, faces=True)
    with ctx.upload_mesh(*spheres) as m:
        got = m.rasterize(view, faces=True)
    assert want["n_covered"] > 100 and got["image"].shape == (48, 64, 9)
    assert got["image"].tobytes() == want["image"].tobytes() and got["faces"].tobytes() == want["faces"].tobytes()
    assert {k: v for k, v in got.items() if k not in ("image", "faces", "ms")} == {k: v for k, v in want.items() if k not in ("image", "faces", "ms")}


def test_extract_mesh_is_the_chain_written_out():
    """A model of 40 steps: extract_mesh with every post-processing argument against extract_mesh_device and the methods, on the one context, one after the other."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    with rnb.Context(deterministic=1, **KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(40):
            c.train_step()
        got = c.extract_mesh(64, cull="none", colors=True, keep="largest", orient="outward", simplify=16, error=True)
        with c.extract_mesh_device(64, cull="none", colors=True) as m, m.clean("largest", "outward") as cm:
            with cm.simplify(*c.simplify_grid((0, 0, 0), (1, 1, 1), 16)) as sm:
                want = sm.download()
                want.update(stats=m.stats, simplify_error=cm.distance_to(sm, symmetric=True), clean_stats=cm.stats, simplify_stats=sm.stats)
    assert sorted(got) == sorted(want) == ["clean_stats", "colors", "indices", "simplify_error", "simplify_stats", "stats", "verts"]
    assert len(got["indices"]) > 300
    for k in ("verts", "indices", "colors"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    for k in ("stats", "clean_stats", "simplify_stats", "simplify_error"):
        assert _timeless(got[k]) == _timeless(want[k]) and sorted(got[k]) == sorted(want[k]), k


def test_a_freed_handle_stops_in_python_on_the_device_too(ctx, spheres):
    view = fibonacci_view(0, 3, 64, 48, 2.5 * 64)
    with ctx.upload_mesh(*spheres) as other:
        m = ctx.upload_mesh(*spheres)
        cm = m.clean()
        for x in (m, cm):
            x.free()
            x.free()
            for call in (lambda: x.clean(), lambda: x.simplify((0, 0, 0), 1.0 / 16, 16), lambda: x.distance_to(other), lambda: other.distance_to(x), lambda: x.rasterize(view),
                         lambda: x.download(), lambda: x.__enter__()):
                with pytest.raises(ValueError, match="freed"):
                    call()
            assert (x.n_verts, x.n_triangles) == (0, 0) and not x.verts
        assert other.rasterize(view)["n_covered"] > 100  # the context and the live handle go on
