"""The inference tracer on the MI355X (include/rnb_render.h; the reference's NerfTracer, src/testbed_nerf.cu:822-1118, 2248-2770): parity with the numpy
statement of tests/render_reference.py on the CPU checker's network, the geometry of a trained sphere, bit-reproducibility across renders and tilings,
no effect on training, and the edge cases of the ray set."""
import numpy as np
import pytest

from tests import render_reference as rr

pytestmark = pytest.mark.gpu

KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)


def _scene(n_views=16, res=128):
    from rnb_neus2_amd import synthetic
    return synthetic.make_scene(n_views, res, 1400.0 * res / 800.0)


@pytest.fixture(scope="module")
def trained():
    """A sphere trained for 500 steps on 16 views at 128 x 128."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene()
    c = rnb.Context(**KW)
    c.init_params()
    c.set_dataset(views, normals, albedos)
    for _ in range(500):
        c.train_step()
    yield c, views, normals
    c.close()


def _view(base, w, h):
    """The camera of `base` with a w x h image (focal length scaled with the width, centred principal point)."""
    f = float(base["focal_length"][0]) * w / float(base["width"])
    return dict(width=w, height=h, focal_length=(f, f), principal_point=(0.5, 0.5), xform=np.asarray(base["xform"], np.float32).reshape(3, 4))


def _angle_deg(a, b):
    cos = np.clip((a * b).sum(-1) / np.maximum(np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1), 1e-30), -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def _stack(r):
    return np.concatenate([r["normal"], r["albedo"], r["opacity"][..., None], r["depth"][..., None], r["n_samples"][..., None].astype(np.float32)], axis=-1)


def test_parity_with_the_numpy_tracer(trained):
    """The same weights (EMA) and grid in the CPU checker; its forward_infer is the network of the numpy tracer, the bitfield the library's own.
    min_transmittance 0: every pixel's sample count equals the numpy march's (the march depends on the ray and the bitfield only, and is float32 in the same
    operation order). Default: the maps agree within what half-precision network outputs allow (the two networks round differently)."""
    from tests import oracle_lib
    c, views, _ = trained
    cpu = oracle_lib.context(**KW)
    cpu.init_params()
    cpu.set_params(c.get("PARAMS_FP32"))
    cpu.put("PARAMS_EMA", c.get("PARAMS_EMA"))
    cpu.put("DENSITY_GRID", c.get("DENSITY_GRID"))
    cpu.update_density_bitfield()
    bits = c.get("DENSITY_BITFIELD")
    chunk = KW["target_batch_size"] * 8

    def net(coords):
        return np.concatenate([cpu.forward_infer(coords[k:k + chunk], inference=True) for k in range(0, len(coords), chunk)])

    v = _view(views[3], 48, 40)
    full = c.render(v, min_transmittance=0.0)
    ref_full, _ = rr.render(v, net, bitfield=bits, min_transmittance=0.0)
    assert np.array_equal(full["n_samples"], ref_full[..., 8].astype(np.uint32))
    assert full["n_samples"].max() > 0

    g = c.render(v)
    ref, n_net = rr.render(v, net, bitfield=bits)
    gi = _stack(g)
    d_op = np.abs(gi[..., 6] - ref[..., 6])
    both = (gi[..., 6] > 0.5) & (ref[..., 6] > 0.5)
    ang = _angle_deg(gi[both][:, 0:3], ref[both][:, 0:3])
    d_alb = np.abs(gi[both][:, 3:6] - ref[both][:, 3:6])
    dep = (gi[..., 6] > 0.2) & (ref[..., 6] > 0.2)
    d_dep = np.abs(gi[dep][:, 7] - ref[dep][:, 7])
    print("parity: opacity |d| mean %.2e max %.2e; normal angle mean %.3f max %.3f deg; albedo |d| max %.2e; depth |d| median %.2e max %.2e; hit %d of %d"
          % (d_op.mean(), d_op.max(), ang.mean(), ang.max(), d_alb.max(), np.median(d_dep), d_dep.max(), both.sum(), both.size))
    # observed on the first MI355X run (500 steps, view 3 at 48 x 40, 631 pixels hit): opacity |d| mean 9.1e-7, max 1.7e-4; normal angle mean 0.001, max 0.028 deg;
    # albedo |d| max 6.0e-7; depth |d| median 0, max 3.4e-3 (a max-weight sample that changed places)
    assert both.sum() > 0.2 * both.size
    assert d_op.mean() < 2e-5 and d_op.max() < 5e-3
    assert ang.mean() < 0.02 and ang.max() < 0.5
    assert d_alb.max() < 1e-4
    assert np.median(d_dep) < 1e-5 and d_dep.max() < 0.02
    cpu.close()


def test_geometry_of_the_trained_sphere(trained):
    """Training views against the analytic maps of synthetic.render_view: a frame, sign or axis error of the normals costs tens of degrees."""
    c, views, normals = trained
    for k in (0, 5, 11):
        r = c.render(views[k])
        nm = normals[k]
        mask_in, mask_r = nm[..., 3] > 0, r["opacity"] > 0.5
        iou = (mask_in & mask_r).sum() / (mask_in | mask_r).sum()
        R = np.asarray(views[k]["xform"], np.float64).reshape(3, 4)[:, :3]
        m = nm[..., :3].astype(np.float64) / 65535.0 * 2.0 - 1.0
        n_in = np.stack([m[..., 0], -m[..., 1], -m[..., 2]], axis=-1)
        both = mask_in & mask_r
        ang = _angle_deg(n_in[both], r["normal"].astype(np.float64)[both] @ R)
        print("view %d: IoU %.4f, normal angle mean %.2f median %.2f deg, depth %.3f..%.3f, %d rounds, %d samples"
              % (k, iou, ang.mean(), np.median(ang), r["depth"][both].min(), r["depth"][both].max(), r["stats"]["rounds"], r["stats"]["n_samples"]))
        # observed (first MI355X run): IoU 0.985-0.990, mean angle 3.0-4.3 deg, median 2.8-3.9 deg
        assert iou > 0.97
        assert ang.mean() < 7.0 and np.median(ang) < 6.0
        assert r["depth"][both].min() > 1.2 and r["depth"][both].max() < 1.5  # the sphere (radius 0.25) seen from 1.5
        assert r["stats"]["n_rays"] == 128 * 128 and r["stats"]["n_hit"] >= mask_r.sum()


def test_renders_are_bit_identical_across_runs_and_tilings(trained):
    c, views, _ = trained
    v = _view(views[7], 160, 120)
    a = _stack(c.render(v))
    b = _stack(c.render(v))
    t = c.render(v, max_rays_in_flight=4096)
    assert t["stats"]["rounds"] > c.render(v)["stats"]["rounds"]  # five tiles: a different round schedule
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), _stack(t).view(np.uint32))


@pytest.mark.parametrize("overlap", [1, 0])
def test_rendering_leaves_training_untouched(overlap):
    """deterministic = 1: 50 steps, a render, 50 steps == 100 steps, bit for bit (weights, EMA, Adam moments, occupancy grid, step statistics)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene(8, 96)
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, overlap=overlap, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(100):
            if interrupt and s == 50:
                r = c.render(_view(views[2], 64, 48))
                assert r["stats"]["n_hit"] > 0
                c.render(_view(views[4], 33, 17), inference=False, min_transmittance=0.0)
            stats.append(c.train_step().as_dict())
        state = {k: c.get(k).copy() for k in ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID")}
        for st in stats:
            st.pop("prep_ms"), st.pop("step_ms")
        runs.append((state, stats))
        c.close()
    (sa, ta), (sb, tb) = runs
    assert ta == tb
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def test_edge_views(trained):
    import rnb_neus2_amd as rnb
    c, views, _ = trained
    bits = c.get("DENSITY_BITFIELD")
    # a 1 x 1 view and widths that are not multiples of 64: the sample counts of the numpy march (min_transmittance 0 composites every sample)
    for w, h in ((1, 1), (100, 37), (65, 3)):
        v = _view(views[1], w, h)
        r = c.render(v, min_transmittance=0.0)
        o, d = rr.camera_rays(v)
        _, _, cnt = rr.march(o, d, bits)
        assert r["normal"].shape == (h, w, 3) and r["stats"]["n_rays"] == w * h
        assert np.array_equal(r["n_samples"].ravel(), cnt.astype(np.uint32))
        assert np.all(np.isfinite(_stack(r)))
    # a camera looking away from the box: nothing
    away = _view(views[1], 64, 64)
    m = np.asarray(away["xform"], np.float32).reshape(3, 4).copy()
    m[:, 0:3] = -m[:, 0:3]
    away["xform"] = m
    r = c.render(away)
    assert not _stack(r).any() and r["stats"]["n_hit"] == 0 and r["stats"]["n_samples"] == 0
    # more pixels than one default tile (2^19): the same bits as one tile
    big = _view(views[1], 1600, 1200)
    r1 = c.render(big)
    r2 = c.render(big, max_rays_in_flight=1 << 21)
    assert r1["stats"]["rounds"] > r2["stats"]["rounds"]
    assert np.array_equal(_stack(r1).view(np.uint32), _stack(r2).view(np.uint32))
    assert r1["stats"]["n_hit"] > 0.1 * 1600 * 1200
    # without the occupancy grid every step of the box is a sample
    r_all = c.render(_view(views[1], 32, 32), occupancy=False, min_transmittance=0.0)
    r_occ = c.render(_view(views[1], 32, 32), min_transmittance=0.0)
    assert np.all(r_all["n_samples"] >= r_occ["n_samples"]) and r_all["n_samples"].sum() > r_occ["n_samples"].sum()
    # an all-empty bitfield: no samples (a context of its own: the trained one keeps its grid)
    e = rnb.Context(**KW)
    e.init_params()
    e.put("DENSITY_BITFIELD", np.zeros(len(bits), np.uint8))
    r = e.render(_view(views[1], 64, 64))
    assert r["stats"]["n_samples"] == 0 and not _stack(r).any()
    e.close()
    # bad arguments
    with pytest.raises(rnb.RnbError, match="empty view"):
        c.render(_view(views[1], 0, 5))
    with pytest.raises(rnb.RnbError, match="min_transmittance"):
        c.render(_view(views[1], 4, 4), min_transmittance=1.0)
    with pytest.raises(rnb.RnbError, match="null"):
        c.render_into(_view(views[1], 4, 4), 0)


def test_both_accumulate_modes(trained):
    """RNB_ACCUM_HALF selects the half-accumulating network kernel; the tracer around it is the same: the maps agree with the fp32 mode's within half rounding."""
    import rnb_neus2_amd as rnb
    c, views, _ = trained
    v = _view(views[9], 96, 80)
    ref = c.render(v)
    from rnb_neus2_amd import _abi
    h = rnb.Context(accumulate=_abi.ACCUM_HALF, **KW)
    h.init_params()
    h.set_params(c.get("PARAMS_FP32"))
    h.put("PARAMS_EMA", c.get("PARAMS_EMA"))
    h.put("DENSITY_GRID", c.get("DENSITY_GRID"))
    h.update_density_bitfield()
    r = h.render(v)
    both = (r["opacity"] > 0.5) & (ref["opacity"] > 0.5)
    ang = _angle_deg(r["normal"][both], ref["normal"][both])
    print("half vs fp32 accumulators: normal angle mean %.3f deg, opacity |d| mean %.2e" % (ang.mean(), np.abs(r["opacity"] - ref["opacity"]).mean()))
    assert both.sum() > 0.2 * both.size
    assert ang.mean() < 1.0
    assert np.abs(r["opacity"] - ref["opacity"]).mean() < 0.01
    r2 = h.render(v, max_rays_in_flight=1024)
    assert np.array_equal(_stack(r).view(np.uint32), _stack(r2).view(np.uint32))
    h.close()
