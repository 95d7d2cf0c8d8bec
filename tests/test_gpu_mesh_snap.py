"""The snapping stage on the MI355X (include/rnb_mesh_snap.h) against the numpy statement of tests/mesh_snap_reference.py with Context.forward_infer as the network,
bit for bit: vertices, residuals, states, displacement, resampled normals and the statistics; no bit depends on the batching or on the order of the vertices; no vertex
ends worse than it began; without a step the attributes are the extractor's; a selection; training is left alone; refusals; build/mesh --snap end to end. The model is
the 500-step sphere of tests/test_gpu_mesh_sparse.py, the mesh its res-32 extraction."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_snap_reference as sr
from tests import mesh_texture_reference as tr
from tests.test_gpu_mesh_sparse import KW, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = ("colors", "normals")
COMPARED = [k for k in sr.SNAP_STATS]  # every stat but n_network_points, peak_workspace, ms and ms_network


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def trained():
    """A sphere trained for 500 steps on 16 views at 128 x 128 (the model of tests/test_gpu_mesh_sparse.py)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene()
    c = rnb.Context(**KW)
    c.init_params()
    c.set_dataset(views, normals, albedos)
    for _ in range(500):
        c.train_step()
    yield c
    c.close()


@pytest.fixture(scope="module")
def sphere32(trained):
    """The res-32 extraction without culling, with the vertex attributes (computed once, shared, left unchanged)."""
    mesh = trained.extract_mesh(32, cull="none", colors=True, normals=True)
    assert 1000 < len(mesh["verts"]) < 10000
    return mesh


@pytest.fixture(scope="module")
def perturbed(sphere32):
    """Its vertices pushed about by a seeded uniform +-0.01, and three placed by hand: one outside the box, one on the box face, one 0.2 further from the centre."""
    v = sphere32["verts"]
    rng = np.random.default_rng(11)
    p = (v + rng.uniform(-0.01, 0.01, v.shape)).astype(np.float32)
    p[0] = (1.2, 0.5, 0.5)
    p[1] = (1.0, 0.5, 0.5)
    d = v[2].astype(np.float64) - 0.5
    p[2] = (0.5 + d * (1 + 0.2 / np.linalg.norm(d))).astype(np.float32)
    return p


def _evaluate(c, inference=True):
    chunk = KW["target_batch_size"] * 8  # what forward_infer's scratch holds

    def net(coords):
        return np.concatenate([c.forward_infer(coords[k:k + chunk], inference=inference) for k in range(0, len(coords), chunk)]) if len(coords) else np.zeros((0, 16), np.float16)
    return net


def _assert_equal(got, want, attributes=()):
    """Every per-vertex array and every compared stat, bit for bit; the resampled colours as far as numpy can state them (see test_the_statement_bit_for_bit)."""
    for key in ("verts", "residual_before", "residual_after", "displacement"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (key, int((_bits(got[key]) != _bits(want[key])).sum()))
    assert np.array_equal(got["state"], want["state"])
    for key in COMPARED:
        assert got["stats"][key] == want["stats"][key], (key, got["stats"][key], want["stats"][key])
    if "normals" in attributes:
        assert np.array_equal(_bits(got["normals"]), _bits(want["normals"]))
    if "colors" in attributes:
        assert np.abs(got["colors"].astype(np.float64) - want["colors"]).max() < 1e-6


def test_the_statement_bit_for_bit(trained, sphere32, perturbed):
    """Verts, residuals, states, displacement, the resampled normals and every stat except n_network_points, ms* and peak_workspace equal expected_snap with
    evaluate = forward_infer(inference=True), for 0, 1 and 3 iterations. The colours pass through the device's float expf, which numpy does not have: they are the
    float64 logistic of the SAME half outputs to within 1e-6 (the bound tests/test_gpu_mesh_texture.py::test_values_are_the_networks carries for the same arithmetic),
    one colour per half value, and bit-equal to the extractor's where nothing moves (test_without_a_step_the_attributes_are_the_extractors). Fails without the
    feature."""
    c = trained
    net = _evaluate(c)
    shares = {}
    for it in (0, 1, 3):
        got = c.snap_mesh(perturbed, sphere32["indices"], iterations=it, attributes=BOTH, residuals=True, states=True, displacement=True)
        want = sr.expected_snap(perturbed, None, net, 0.0, 1.0, iterations=it, attributes=BOTH)
        _assert_equal(got, want, BOTH)
        assert np.array_equal(got["indices"], sphere32["indices"]) and got["colors"].dtype == np.float32
        # one colour per half value: the colour is a function of the half output alone
        halves, colours = want["out"][:, 0:3].view(np.uint16).ravel(), _bits(got["colors"]).ravel()
        order = np.argsort(halves, kind="stable")
        same_half = halves[order][1:] == halves[order][:-1]
        assert (colours[order][1:][same_half] == colours[order][:-1][same_half]).all()
        st = got["stats"]
        assert st["n_network_points"] >= 2 * st["n_selected"] and st["ms"] > 0 and st["ms_network"] > 0 and st["peak_workspace"] > len(perturbed) * 12
        shares[it] = {s: st["n_" + s] for s in sr.STATE_NAMES if st["n_" + s]}
        print("iterations %d: %s, mean |sdf| %.3e -> %.3e" % (it, shares[it], st["sum_before_q"] / 2.0 ** 24 / st["n_selected"], st["sum_after_q"] / 2.0 ** 24 / st["n_selected"]))
    # the hand-placed vertices: from outside the box no step of 1 / 128 leads into it; 0.2 away the leash holds
    print("placed by hand: states %s" % [sr.STATE_NAMES[k] for k in got["state"][:3]])
    assert got["verts"][0].tobytes() == perturbed[0].tobytes() and got["displacement"][2] <= np.float32(1.0 / 64.0)


def test_batching_and_vertex_order_cannot_show(trained, sphere32, perturbed):
    c = trained
    kw = dict(iterations=3, attributes=BOTH, residuals=True, states=True, displacement=True)
    first = c.snap_mesh(perturbed, sphere32["indices"], **kw)
    for per_launch in (0, 1000, 64):
        again = c.snap_mesh(perturbed, sphere32["indices"], max_points_in_flight=per_launch, **kw)
        for key in ("verts", "residual_before", "residual_after", "displacement", "state", "colors", "normals"):
            assert np.array_equal(_bits(again[key]), _bits(first[key])), (per_launch, key)
        assert {k: again["stats"][k] for k in COMPARED} == {k: first["stats"][k] for k in COMPARED}
    perm = np.random.default_rng(12).permutation(len(perturbed))
    inverse = np.argsort(perm)
    shuffled = c.snap_mesh(perturbed[perm], inverse.astype(np.uint32)[sphere32["indices"]], **kw)
    for key in ("verts", "residual_before", "residual_after", "displacement", "state", "colors", "normals"):
        assert np.array_equal(_bits(shuffled[key]), _bits(first[key][perm])), key
    assert {k: shuffled["stats"][k] for k in COMPARED} == {k: first["stats"][k] for k in COMPARED}


def test_no_vertex_ends_worse_than_it_began(trained, sphere32, perturbed):
    """What the statement guarantees, |residual_after| <= |residual_before| for every vertex that is not INVALID, and the median."""
    got = trained.snap_mesh(perturbed, sphere32["indices"], residuals=True, states=True, displacement=True)
    st = got["stats"]
    n = st["n_selected"]
    print("shares: %s" % {s: round(st["n_" + s] / n, 4) for s in sr.STATE_NAMES if st["n_" + s]})
    print("mean |sdf| %.3e -> %.3e, max %.3e -> %.3e, greatest displacement %.3e, %d rounds" % (st["sum_before_q"] / 2.0 ** 24 / n, st["sum_after_q"] / 2.0 ** 24 / n, st["max_before"],
                                                                                          st["max_after"], st["max_displacement"], st["rounds"]))
    ok = got["state"] != sr.INVALID
    before, after = np.abs(got["residual_before"]), np.abs(got["residual_after"])
    assert (after[ok] <= before[ok]).all()
    assert np.median(after) < np.median(before)
    assert (got["displacement"] <= np.float32(1.0 / 64.0)).all() and sum(st["n_" + s] for s in sr.STATE_NAMES) == len(perturbed)


def test_without_a_step_the_attributes_are_the_extractors(trained, sphere32):
    got = trained.snap_mesh(sphere32["verts"], sphere32["indices"], iterations=0, attributes=BOTH, residuals=True)
    assert np.array_equal(_bits(got["verts"]), _bits(sphere32["verts"]))
    assert np.array_equal(_bits(got["colors"]), _bits(sphere32["colors"])) and np.array_equal(_bits(got["normals"]), _bits(sphere32["normals"]))
    assert np.array_equal(_bits(got["residual_before"]), _bits(got["residual_after"])) and got["stats"]["n_moved"] == 0
    with trained.upload_mesh(sphere32["verts"], sphere32["indices"]) as m:
        residual, stats = m.sdf_residual()
    assert np.array_equal(_bits(residual), _bits(got["residual_before"])) and stats["sum_before_q"] == got["stats"]["sum_before_q"]
    print("the extraction itself: mean |sdf| %.3e, max %.3e" % (stats["sum_before_q"] / 2.0 ** 24 / stats["n_selected"], stats["max_before"]))


def test_a_selection_leaves_the_rest_alone(trained, sphere32, perturbed):
    c = trained
    rng = np.random.default_rng(13)
    sel = rng.random(len(perturbed)) < 0.3
    col, nor = sphere32["colors"], sphere32["normals"]
    got = c.snap_mesh(perturbed, sphere32["indices"], colors=col, select=sel, attributes=("colors", "normals"), residuals=True, states=True, displacement=True)
    want = sr.expected_snap(perturbed, sel, _evaluate(c), 0.0, 1.0, attributes=BOTH, colors=col)
    _assert_equal(got, want, BOTH)
    assert np.array_equal(_bits(got["verts"][~sel]), _bits(perturbed[~sel])) and (got["state"][~sel] == sr.UNSELECTED).all()
    assert np.array_equal(_bits(got["colors"][~sel]), _bits(col[~sel])) and not _bits(got["normals"][~sel]).any()  # carried; zeros where the input has none
    for key in ("residual_before", "residual_after", "displacement"):
        assert not _bits(got[key][~sel]).any(), key
    assert got["stats"]["n_selected"] == sel.sum() and got["stats"]["n_unselected"] == (~sel).sum()
    kept = c.snap_mesh(perturbed, sphere32["indices"], colors=col, normals=nor, select=sel)  # nothing asked for: both carried, whatever moves
    assert np.array_equal(_bits(kept["colors"]), _bits(col)) and np.array_equal(_bits(kept["normals"]), _bits(nor)) and np.array_equal(_bits(kept["verts"]), _bits(got["verts"]))
    none = c.snap_mesh(perturbed, sphere32["indices"], select=np.zeros(len(perturbed)))
    assert np.array_equal(_bits(none["verts"]), _bits(perturbed)) and none["stats"]["rounds"] == 0 and none["stats"]["n_network_points"] == 0


def test_the_snap_leaves_training_untouched():
    """deterministic = 1: 50 steps, two snaps (one with each set of weights), 50 steps == 100 steps, bit for bit (the per-step statistics and the weights)."""
    import rnb_neus2_amd as rnb
    views, normals, albedos = _scene(8, 96)
    verts, tris = tr.octahedron(2)
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(100):
            if interrupt and s == 50:
                c.snap_mesh(verts, tris, attributes=BOTH, residuals=True)
                c.snap_mesh(verts, tris, iterations=5, inference=False, max_points_in_flight=50)
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


def test_refusals(trained, sphere32):
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import _abi
    c = trained
    verts, tris = tr.octahedron(1)
    kw = dict(residuals=True, states=True)
    good = c.snap_mesh(verts, tris, **kw)
    bad = tris.copy()
    bad[5, 1] = len(verts)  # found by the range-check kernel, before anything else
    with pytest.raises(rnb.RnbError, match="out of range") as err:
        c.snap_mesh(verts, bad)
    assert err.value.code == _abi.ERR_INVALID and "rnb_mesh_snap" in str(err.value)
    with c.upload_mesh(verts, tris) as m:  # the raw call: the result comes back zeroed, the input is untouched
        assert c.f.mesh_snap(c._h, None, C.byref(m), C.byref(c._snap_options()), None, C.byref(m), None, None, None, None, None) == _abi.ERR_INVALID
        assert b"different objects" in c.f.last_error() and m.n_indices == tris.size and m.verts
        for field, value, what in (("abi_version", 2, b"abi_version"), ("iterations", 65, b"iterations"), ("tolerance", -1.0, b"tolerance"), ("max_step", 0.0, b"max_step"),
                                   ("max_displacement", float("nan"), b"max_displacement"), ("min_gradient", 0.0, b"min_gradient"), ("attributes", 8, b"attributes"),
                                   ("use_inference_params", 2, b"use_inference_params")):
            opt, out = c._snap_options(), _abi.Mesh()
            setattr(opt, field, value)
            out.n_indices = 9
            assert c.f.mesh_snap(c._h, None, C.byref(m), C.byref(opt), None, C.byref(out), None, None, None, None, None) == _abi.ERR_INVALID and bytes(out) == b"\0" * C.sizeof(out), field
            assert b"rnb_mesh_snap" in c.f.last_error() and what in c.f.last_error()
    with c.upload_mesh(verts, bad) as m:
        out, st = _abi.Mesh(), _abi.MeshSnapStats()
        out.n_indices = 9
        assert c.f.mesh_snap(c._h, None, C.byref(m), C.byref(c._snap_options()), None, C.byref(out), None, None, None, None, C.byref(st)) == _abi.ERR_INVALID
        assert bytes(out) == b"\0" * C.sizeof(out)
    again = c.snap_mesh(verts, tris, **kw)  # the context still works, and gives what it gave
    for key in ("verts", "residual_before", "residual_after", "state"):
        assert np.array_equal(_bits(again[key]), _bits(good[key])), key
    # a mesh without triangles, and one without vertices
    e = np.zeros(0, np.uint32)
    lone = c.snap_mesh(sphere32["verts"][:5], e, residuals=True)
    assert lone["verts"].shape == (5, 3) and lone["stats"]["n_selected"] == 5 and len(lone["indices"]) == 0
    none = c.snap_mesh(np.zeros((0, 3), np.float32), e, attributes=BOTH, residuals=True, states=True, displacement=True)
    assert none["verts"].shape == (0, 3) and none["stats"]["rounds"] == 0 and none["residual_after"].shape == (0,)


def test_build_mesh_snaps_what_the_fill_and_the_smoothing_leave(tmp_path):
    """`build/mesh --fill-holes --smooth 2 --snap 3 --report-residual` on a snapshot trained here for 100 steps: the `snap:` line is there, the triangles are those of the
    run without --snap, and the reported mean residual is below that run's."""
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = os.path.join(scene, "output", "snapshot_100.msgpack")
    base = [os.path.join(ROOT, "build", "mesh"), "--snapshot", snap, "--scene", scene, "--resolution", "64", "--fill-holes", "--smooth", "2", "--report-residual"]
    said, faces = {}, {}
    for name, flags in (("smoothed", []), ("snapped", ["--snap", "3"])):
        out = str(tmp_path / (name + ".obj"))
        r = subprocess.run(base + ["--out", out] + flags, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith('{"residual"')]
        snap_lines = [l for l in r.stdout.splitlines() if l.startswith("snap:")]
        assert len(lines) == 1 and len(snap_lines) == len(flags) // 2, r.stdout
        print(name, lines[0], snap_lines)
        said[name] = json.loads(lines[0])["residual"]
        with open(out) as fh:
            faces[name] = [l for l in fh if l.startswith("f ")]
    assert said["snapped"]["n_verts"] == said["smoothed"]["n_verts"] > 0 and faces["snapped"] == faces["smoothed"]
    assert said["snapped"]["mean"] < said["smoothed"]["mean"]
