"""`build/render` on the MI355X, end to end: `testbed --maxiter 600 --save-snapshot` on a synthetic scene, then `render` on the snapshot. The outputs have
the input sizes, the normal PNGs decode (as the loss decodes the inputs) to the camera-frame normals of Context.render on the same snapshot within one
quantisation step, and render_metrics.json agrees with a recomputation from the written PNGs."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = (0, 4, 9)


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    from rnb_neus2_amd import synthetic
    tmp = tmp_path_factory.mktemp("render_cli")
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp / "scene")
    synthetic.write_scene(scene, views, normals, albedos)  # scale 1, offset 0: the loader's cameras are the views' float32 matrices
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "600", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_600.msgpack")
    out = str(tmp / "maps")
    r = subprocess.run([os.path.join(ROOT, "build", "render"), "--snapshot", snap, "--scene", scene, "--out", out, "--views", ",".join(map(str, VIEWS))],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    print(r.stdout)
    return views, normals, snap, out


def _context_from_snapshot(path):
    import msgpack
    import rnb_neus2_amd as rnb
    with open(path, "rb") as f:
        root = msgpack.unpackb(f.read(), raw=False)
    enc, snap = root["encoding"], root["snapshot"]
    c = rnb.Context(n_levels=enc["n_levels"], log2_hashmap_size=enc["log2_hashmap_size"], base_resolution=enc["base_resolution"], per_level_scale=enc["per_level_scale"],
                    valid_level_scale=enc["valid_level_scale"], base_valid_level_scale=enc["base_valid_level_scale"], base_training_step=enc["base_training_step"],
                    sdf_bias=root["network"]["sdf_bias"], apply_no_albedo=1, aabb_scale=int(snap["nerf"]["aabb_scale"]))
    c.set_params(np.frombuffer(snap["params_binary"], np.float16).astype(np.float32))
    c.put("DENSITY_GRID", np.frombuffer(snap["density_grid_binary"], np.float16).astype(np.float32))
    c.update_density_bitfield()
    c.set_training_step(snap["training_step"])
    return c


def _png(path):
    from rnb_neus2_amd import image_io
    a = image_io.read_unchanged(path)
    assert a is not None and a.dtype == np.uint16, path
    return a


def test_outputs_have_the_input_sizes(rendered):
    views, normals, _, out = rendered
    for k in VIEWS:
        h, w = normals[k].shape[:2]
        assert _png(os.path.join(out, "normals", "%05d.png" % k)).shape == (h, w, 4)
        assert _png(os.path.join(out, "albedos", "%05d.png" % k)).shape == (h, w, 4)
        d = np.load(os.path.join(out, "depth", "%05d.npy" % k))
        assert d.shape == (h, w) and d.dtype == np.float32 and np.all(np.isfinite(d))
        hit = d > 0
        assert hit.sum() > 0.1 * hit.size and d[hit].min() > 1.2 and d[hit].max() < 1.5  # the sphere (radius 0.25) seen from 1.5
    assert sorted(os.listdir(os.path.join(out, "normals"))) == ["%05d.png" % k for k in VIEWS]


def test_normal_pngs_decode_to_the_rendered_normals(rendered):
    views, _, snap, out = rendered
    c = _context_from_snapshot(snap)
    for k in VIEWS:
        r = c.render(views[k])
        png = _png(os.path.join(out, "normals", "%05d.png" % k)).astype(np.int64)
        mask = r["opacity"] > 0.5
        assert np.array_equal(png[..., 3] == 65535, mask) and np.all(png[..., 3][~mask] == 0)
        R = np.asarray(views[k]["xform"], np.float32).reshape(3, 4)[:, :3].astype(np.float64)
        ncam = r["normal"].astype(np.float64) @ R  # R^T n
        m = np.stack([ncam[..., 0], -ncam[..., 1], -ncam[..., 2]], axis=-1)
        want = np.rint((m + 1.0) * 0.5 * 65535.0)
        assert np.abs(png[..., :3][mask] - want[mask]).max() <= 1  # one quantisation step
        dec = png[..., :3][mask] / 65535.0 * 2.0 - 1.0  # the loss's decoding (ray_targets): (x, -y, -z) back to the camera frame
        dec = np.stack([dec[:, 0], -dec[:, 1], -dec[:, 2]], axis=-1)
        assert np.abs(dec - ncam[mask]).max() < 2.0 / 65535.0
    c.close()


def test_metrics_agree_with_the_written_pngs(rendered):
    views, normals, _, out = rendered
    with open(os.path.join(out, "render_metrics.json")) as f:
        met = json.load(f)
    assert [v["view"] for v in met["views"]] == list(VIEWS)
    for v in met["views"]:
        k = v["view"]
        png = _png(os.path.join(out, "normals", "%05d.png" % k)).astype(np.float64)
        inp = normals[k].astype(np.float64)
        m_r, m_i = png[..., 3] > 0, inp[..., 3] > 0
        both = m_r & m_i
        def cam(a):
            d = a[..., :3] / 65535.0 * 2.0 - 1.0
            return np.stack([d[..., 0], -d[..., 1], -d[..., 2]], axis=-1)
        a, b = cam(png)[both], cam(inp)[both]
        ang = np.degrees(np.arccos(np.clip((a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1), -1, 1)))
        iou = both.sum() / (m_r | m_i).sum()
        # the program measures with the float normals before quantisation: the PNGs give them back to ~1e-3 degrees
        assert abs(v["mask_iou"] - iou) < 2e-6
        assert abs(v["mean_angle_deg"] - ang.mean()) < 0.01 and abs(v["median_angle_deg"] - np.median(ang)) < 0.01
        assert v["width"] == 160 and v["height"] == 160 and v["frame_ms"] > 0
        assert v["mask_iou"] > 0.95 and v["mean_angle_deg"] < 10.0
    assert abs(met["mean"]["mask_iou"] - np.mean([v["mask_iou"] for v in met["views"]])) < 2e-6
    assert abs(met["mean"]["mean_angle_deg"] - np.mean([v["mean_angle_deg"] for v in met["views"]])) < 1e-5
