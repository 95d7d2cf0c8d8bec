"""CPU tier of the snapping stage (include/rnb_mesh_snap.h): the numpy statement of tests/mesh_snap_reference.py against results known by hand (an analytic sphere and
stand-in SDFs, one per way a vertex can stop), the properties the header promises, the C-ABI of the new header (exports, version, defaults, struct layout, argument
validation without a device), the calls the Python layer makes (through a recording stand-in of the function table), and the command-line / pipeline surface. No GPU
needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_snap_reference as sr
from tests import render_reference as rr
from tests import test_mesh_holes_cpu as hc
from tests import test_mesh_smooth_cpu as sc

from rnb_neus2_amd import _abi as _ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_snap.h")
assert (sr.MAX_ITERATIONS, sr.MAX_IN_FLIGHT, sr.RESIDUAL_LIMIT, sr.Q_SCALE) == (_ABI.MESH_SNAP_MAX_ITERATIONS, _ABI.MESH_SNAP_MAX_IN_FLIGHT, 2.0 ** _ABI.MESH_SNAP_RESIDUAL_LOG2,
                                                                             2.0 ** _ABI.MESH_SNAP_Q_SHIFT)
assert (sr.UNSELECTED, sr.CONVERGED, sr.UNFINISHED, sr.FLAT, sr.LEASHED, sr.OUTSIDE, sr.STALLED, sr.INVALID, sr.REVERTED) == (
    _ABI.MESH_SNAP_UNSELECTED, _ABI.MESH_SNAP_CONVERGED, _ABI.MESH_SNAP_UNFINISHED, _ABI.MESH_SNAP_FLAT, _ABI.MESH_SNAP_LEASHED, _ABI.MESH_SNAP_OUTSIDE, _ABI.MESH_SNAP_STALLED,
    _ABI.MESH_SNAP_INVALID, _ABI.MESH_SNAP_REVERTED) and sr.STATE_NAMES == _ABI.MESH_SNAP_STATE_NAMES

SPHERE = rr.analytic_net(rr.sphere_sdf(radius=0.3))  # outputs rounded to half, as the network's are


def _stand_in(sdf_and_grad):
    """evaluate() from a function of the normalised position (float64[n, 3]) -> (sdf[n], grad[n, 3]); the box is the unit box."""
    def net(coords):
        s, g = sdf_and_grad(coords[:, 0:3].astype(np.float64))
        o = np.zeros((len(coords), 16), np.float32)
        o[:, 3], o[:, 4:7] = s, g
        with np.errstate(over="ignore"):
            return o.astype(np.float16)
    return net


def _on_sphere(n, amplitude, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (0.5 + d * (0.3 + rng.uniform(-amplitude, amplitude, (n, 1)))).astype(np.float32)


def _snap(v, net, select=None, **kw):
    return sr.expected_snap(v, select, net, 0.0, 1.0, **kw)


# ------------------------------------------------------------------------------------------------------------------------ the statement
def test_points_off_a_sphere_converge_within_the_default_iterations():
    """Pushed off the sphere by up to 0.01 (more than one max_step of 1 / 128, so the first step is clipped), every point ends CONVERGED within the default three
    iterations, 0.3 from the centre to within the tolerance and the half's resolution, and has moved along its radius."""
    v = _on_sphere(2000, 0.01, 3)
    r = _snap(v, SPHERE)
    st = r["stats"]
    assert st["n_converged"] == 2000 and st["n_selected"] == 2000 and sum(st["n_" + s] for s in sr.STATE_NAMES) == 2000 and st["rounds"] == 3
    assert (r["state"] == sr.CONVERGED).all()
    radius = np.linalg.norm(r["verts"].astype(np.float64) - 0.5, axis=1)
    assert np.abs(radius - 0.3).max() <= 2.0 ** -13 + 2.0 ** -12  # the tolerance and half an ulp of a half near 0.3 ... the SDF's own rounding
    assert np.abs(r["residual_after"]).max() <= 2.0 ** -13 and 0.009 < np.abs(r["residual_before"]).max() < 0.0101
    d0, d1 = v.astype(np.float64) - 0.5, r["verts"].astype(np.float64) - 0.5
    cos = (d0 * d1).sum(1) / np.linalg.norm(d0, axis=1) / np.linalg.norm(d1, axis=1)
    assert cos.min() > 1 - 1e-6
    assert 0.0099 < st["max_displacement"] < 0.0101 and st["max_displacement"] == float(r["displacement"].max())
    assert st["max_before"] == float(np.abs(r["residual_before"]).max()) and st["max_after"] == float(np.abs(r["residual_after"]).max())  # (level 0: a residual is a half, the float exact)
    assert st["sum_before_q"] == int(np.trunc(np.abs(r["residual_before"].astype(np.float64)) * 2.0 ** 24).sum()) and st["sum_after_q"] < st["sum_before_q"] // 100
    # a point that starts within the tolerance does not move at all
    on = _on_sphere(50, 0.0, 4)
    r = _snap(on, SPHERE)
    assert (r["state"] == sr.CONVERGED).all() and r["verts"].tobytes() == on.tobytes() and r["stats"]["n_moved"] == 0 and r["stats"]["rounds"] == 1 and not r["displacement"].any()


def test_one_case_for_each_way_to_stop():
    p = np.float32([[0.6, 0.5, 0.5]])
    ex = np.float64([1.0, 0.0, 0.0])
    # FLAT: a constant SDF has no gradient to follow
    r = _snap(p, _stand_in(lambda x: (np.full(len(x), 0.1), np.zeros((len(x), 3)))))
    assert list(r["state"]) == [sr.FLAT] and r["verts"].tobytes() == p.tobytes() and r["stats"]["rounds"] == 1 and r["stats"]["n_flat"] == 1
    # ... and a gradient just above min_gradient is followed
    r = _snap(p, _stand_in(lambda x: (np.full(len(x), 0.001), np.tile(0.26 * ex, (len(x), 1)))), iterations=1)
    assert list(r["state"]) == [sr.UNFINISHED] and r["stats"]["n_moved"] == 1
    # INVALID: a NaN, an infinite gradient, a residual of 2^8; the vertex keeps its bits and is left out of the sums
    for s, g in ((np.nan, ex), (0.1, np.float64([np.inf, 0.0, 0.0])), (256.0, ex), (-300.0, ex)):
        r = _snap(p, _stand_in(lambda x, s=s, g=g: (np.full(len(x), s), np.tile(g, (len(x), 1)))))
        assert list(r["state"]) == [sr.INVALID] and r["verts"].tobytes() == p.tobytes() and r["stats"]["n_invalid"] == 1, (s, g)
        assert r["stats"]["sum_before_q"] == 0 and r["stats"]["max_before"] == 0.0 and r["stats"]["max_after"] == 0.0
    # REVERTED: a gradient of the wrong sign walks away from the plane x = 0.55; the second round sees the larger residual and goes back
    r = _snap(p, _stand_in(lambda x: (x[:, 0] - 0.55, np.tile(-ex, (len(x), 1)))))
    assert list(r["state"]) == [sr.REVERTED] and r["verts"].tobytes() == p.tobytes() and r["stats"]["rounds"] == 2 and r["stats"]["n_moved"] == 0
    assert r["residual_after"][0] == r["residual_before"][0] and abs(r["residual_before"][0] - 0.05) < 1e-4
    # LEASHED: a huge step (max_step lets it through) would end further away than max_displacement allows
    far = _stand_in(lambda x: (x[:, 0] - 0.3, np.tile(ex, (len(x), 1))))
    r = _snap(p, far, max_step=1.0)
    assert list(r["state"]) == [sr.LEASHED] and r["verts"].tobytes() == p.tobytes() and r["stats"]["rounds"] == 1
    # ... with the default max_step it walks 1 / 128 per round until the leash of 1 / 64 stops it: two steps taken, the third refused
    r = _snap(p, far, iterations=8)
    assert list(r["state"]) == [sr.LEASHED] and r["stats"]["rounds"] == 3 and abs(float(r["verts"][0, 0]) - (0.6 - 2 / 128)) < 1e-6 and abs(r["displacement"][0] - 1 / 64) < 1e-6
    # OUTSIDE: a point at the box face whose step leaves the box
    face = np.float32([[1.0, 0.5, 0.5]])
    r = _snap(face, _stand_in(lambda x: (np.full(len(x), -0.005), np.tile(ex, (len(x), 1)))))
    assert list(r["state"]) == [sr.OUTSIDE] and r["verts"].tobytes() == face.tobytes()
    r = _snap(face, _stand_in(lambda x: (np.full(len(x), 0.005), np.tile(ex, (len(x), 1)))), iterations=1)  # ... inwards it moves
    assert list(r["state"]) == [sr.UNFINISHED] and float(r["verts"][0, 0]) < 1.0
    # STALLED: the step is below half an ulp of the position (2^-24 / 16 * 4 = 2^-26 at 0.9) and the tolerance is 0
    at = np.float32([[0.9, 0.5, 0.5]])
    r = _snap(at, _stand_in(lambda x: (np.full(len(x), 2.0 ** -24), np.tile(4 * ex, (len(x), 1)))), tolerance=0.0)
    assert list(r["state"]) == [sr.STALLED] and r["verts"].tobytes() == at.tobytes() and r["stats"]["rounds"] == 1
    # UNFINISHED: 0.01 off the sphere is more than one step of 1 / 128
    v = (np.float32([[0.5 + 0.31, 0.5, 0.5]]))
    r = _snap(v, SPHERE, iterations=1)
    assert list(r["state"]) == [sr.UNFINISHED] and r["stats"]["rounds"] == 2 and abs(float(r["verts"][0, 0]) - (0.81 - 1 / 128)) < 1e-6
    assert abs(r["residual_after"][0] - (0.01 - 1 / 128)) < 2e-4


def test_the_first_rule_that_applies_decides():
    p = np.float32([[0.6, 0.5, 0.5]])
    ex = np.float64([1.0, 0.0, 0.0])
    # within the tolerance and flat: CONVERGED comes before FLAT; invalid and within nothing: INVALID comes first
    r = _snap(p, _stand_in(lambda x: (np.zeros(len(x)), np.zeros((len(x), 3)))))
    assert list(r["state"]) == [sr.CONVERGED]
    r = _snap(p, _stand_in(lambda x: (np.zeros(len(x)), np.full((len(x), 3), np.nan))))
    assert list(r["state"]) == [sr.INVALID]
    # the last round: UNFINISHED comes before FLAT
    r = _snap(p, _stand_in(lambda x: (np.full(len(x), 0.1), np.zeros((len(x), 3)))), iterations=0)
    assert list(r["state"]) == [sr.UNFINISHED]
    # leashed and outside at once: LEASHED
    face = np.float32([[1.0, 0.5, 0.5]])
    r = _snap(face, _stand_in(lambda x: (np.full(len(x), -0.5), np.tile(ex, (len(x), 1)))), max_step=1.0)
    assert list(r["state"]) == [sr.LEASHED]


def test_no_vertex_ends_worse_than_it_began():
    """The monotone property on an SDF made to mislead: a sphere with a ripple whose reported gradient is the plain sphere's, from far enough that steps are clipped,
    leashed and reverted. Every vertex that is not INVALID has |residual_after| <= |residual_before|."""
    def ripple(x):
        v = x - 0.5
        n = np.linalg.norm(v, axis=1)
        return (n - 0.3) + 0.004 * np.sin(900.0 * n), v / n[:, None]
    v = _on_sphere(3000, 0.03, 9)
    for it in (1, 3, 8):
        r = _snap(v, _stand_in(ripple), iterations=it, tolerance=2.0 ** -16)
        ok = r["state"] != sr.INVALID
        assert ok.all() and (np.abs(r["residual_after"]) <= np.abs(r["residual_before"])).all(), it
        assert r["stats"]["sum_after_q"] <= r["stats"]["sum_before_q"] and r["stats"]["max_after"] <= r["stats"]["max_before"]
        assert (r["displacement"] <= np.float32(1.0 / 64.0)).all()
        if it == 8:
            assert r["stats"]["n_reverted"] > 0 and r["stats"]["n_leashed"] > 0  # the case is what it is meant to be
            assert np.median(np.abs(r["residual_after"])) < np.median(np.abs(r["residual_before"]))


def test_zero_iterations_is_a_census():
    v = _on_sphere(500, 0.01, 5)
    r = _snap(v, SPHERE, iterations=0, attributes=("colors", "normals"))
    assert r["verts"].tobytes() == v.tobytes() and r["stats"]["rounds"] == 1 and r["stats"]["n_moved"] == 0 and not r["displacement"].any()
    assert set(np.unique(r["state"])) <= {sr.CONVERGED, sr.UNFINISHED} and r["stats"]["n_converged"] + r["stats"]["n_unfinished"] == 500
    assert r["residual_before"].tobytes() == r["residual_after"].tobytes() and r["stats"]["sum_before_q"] == r["stats"]["sum_after_q"]
    want = np.linalg.norm(v.astype(np.float64) - 0.5, axis=1) - 0.3
    assert np.abs(r["residual_before"] - want).max() < 2.0 ** -12
    # the attributes: the analytic net's albedo logits through the logistic, the radial direction
    assert np.allclose(r["colors"], 1 / (1 + np.exp(-np.float64([0.0, 1.0, -1.0]))), atol=1e-3) and r["normals"].dtype == np.float32
    radial = (v.astype(np.float64) - 0.5) / np.linalg.norm(v.astype(np.float64) - 0.5, axis=1)[:, None]
    assert np.abs(r["normals"] - radial).max() < 2e-3 and np.abs(np.linalg.norm(r["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_a_selection_leaves_the_rest_alone():
    v = _on_sphere(400, 0.01, 6)
    rng = np.random.default_rng(7)
    sel = rng.random(400) < 0.4
    col, nor = rng.random((400, 3)).astype(np.float32), rng.random((400, 3)).astype(np.float32)
    every = _snap(v, SPHERE)
    r = _snap(v, SPHERE, select=sel.astype(np.uint32) * 7, attributes=("colors",), colors=col, normals=nor)
    assert r["verts"][~sel].tobytes() == v[~sel].tobytes() and r["verts"][sel].tobytes() == every["verts"][sel].tobytes()  # a vertex is computed from its own data alone
    assert (r["state"][~sel] == sr.UNSELECTED).all() and (r["state"][sel] == sr.CONVERGED).all()
    for key in ("residual_before", "residual_after", "displacement"):
        assert not r[key][~sel].view(np.uint32).any(), key  # +0
        assert r[key][sel].tobytes() == every[key][sel].tobytes(), key
    assert np.array_equal(r["colors"][~sel], col[~sel].astype(np.float64)) and not np.array_equal(r["colors"][sel], col[sel].astype(np.float64))
    assert r["normals"].tobytes() == nor.tobytes()  # not asked for: carried
    st = r["stats"]
    assert st["n_selected"] == int(sel.sum()) and st["n_unselected"] == int((~sel).sum()) and st["n_converged"] == int(sel.sum())
    # an attribute that is asked for and that the input does not have: zeros for the unselected
    r = _snap(v, SPHERE, select=sel, attributes=("normals",))
    assert "colors" not in r and not r["normals"][~sel].any() and np.abs(np.linalg.norm(r["normals"][sel].astype(np.float64), axis=1) - 1).max() < 1e-6
    # nothing selected: a copy, no round
    r = _snap(v, SPHERE, select=np.zeros(400))
    assert r["verts"].tobytes() == v.tobytes() and r["stats"]["rounds"] == 0 and r["stats"]["n_unselected"] == 400
    # the order of the vertices changes nothing
    perm = rng.permutation(400)
    shuffled = _snap(v[perm], SPHERE)
    assert shuffled["verts"].tobytes() == every["verts"][perm].tobytes() and shuffled["stats"] == every["stats"]


def test_the_network_input_is_the_bakers():
    """network_input against the recipe tests/test_gpu_mesh_texture.py::test_values_are_the_networks spells out, and the clamp."""
    v = _on_sphere(100, 0.01, 8)
    c = sr.network_input(v, 0.0, 1.0)
    d = v - np.float32(0.5)
    l = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(np.float32)
    assert c.dtype == np.float32 and np.array_equal(c[:, 0:3], v) and not c[:, 3].any() and np.array_equal(c[:, 4:7], (d / l[:, None] + np.float32(1.0)) * np.float32(0.5))
    out = sr.network_input(np.float32([[1.5, -0.25, 0.5], [np.nan, 0.5, 2.0]]), 0.0, 1.0)
    assert out[:, 0:3].tolist() == [[1.0, 0.0, 0.5], [0.0, 0.5, 1.0]]
    big = sr.network_input(np.float32([[1.5, -0.5, 0.5]]), -0.5, 2.0)  # aabb_scale 2
    assert big[:, 0:3].tolist() == [[1.0, 0.0, 0.5]]


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def _built():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api
    return api.load_library()


def test_snap_header_is_exported_by_the_hip_library():
    fns = _built()
    from rnb_neus2_amd import api, _abi, build
    names = hc._functions(HEADER)
    assert names == ["rnb_mesh_snap", "rnb_mesh_snap_abi_version", "rnb_mesh_snap_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_SNAP_PROTOTYPES) == set(names)
    others = [getattr(_abi, n) for n in dir(_abi) if n.endswith("PROTOTYPES") and n != "MESH_SNAP_PROTOTYPES"]
    assert len(others) >= 13 and not any(set(_abi.MESH_SNAP_PROTOTYPES) & set(o) for o in others)  # a table of its own
    assert fns.mesh_snap_abi_version() == _abi.MESH_SNAP_ABI_VERSION == 1
    o = _abi.MeshSnapOptions()
    assert fns.mesh_snap_default_options(C.byref(o)) == 0
    assert (o.abi_version, o.iterations, o.level, o.tolerance, o.max_step, o.max_displacement, o.min_gradient, o.attributes, o.use_inference_params, o.max_points_in_flight,
            list(o.reserved)) == (1, 3, 0.0, 2.0 ** -13, 1.0 / 128, 1.0 / 64, 0.25, 0, 1, 0, [0] * 4)
    d = sr.DEFAULTS
    assert (o.iterations, o.level, o.tolerance, o.max_step, o.max_displacement, o.min_gradient) == (d["iterations"], d["level"], d["tolerance"], d["max_step"], d["max_displacement"], d["min_gradient"])
    assert fns.mesh_snap_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.Context, "snap_mesh") and hasattr(api.DeviceMesh, "snap") and hasattr(api.DeviceMesh, "sdf_residual")
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS
    text = open(HEADER).read()
    for needle in ("NORMALISED position", "kernels_net.cuh", "|residual_after| <= |residual_before|", "max_points_in_flight", "bit for bit the colour and the normal rnb_extract_mesh"):
        assert needle in text, needle  # the gradient's units and the consequences are said where a caller reads them


def test_snap_validates_its_arguments_without_a_device():
    """Null pointers, a wrong version, every option outside its range, reserved words, n_indices % 3, null buffers and in == out are refused before the context or the
    device is touched: the context handed in here is a block of zeros, and no device exists where this test runs."""
    fns = _built()
    from rnb_neus2_amd import _abi
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def sopt(**kw):
        o = _abi.MeshSnapOptions()
        assert fns.mesh_snap_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def snap(ctx_, m, o, out):
        return fns.mesh_snap(ctx_, None, m, o, None, out, None, None, None, None, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    E = _abi.ERR_INVALID
    assert snap(None, C.byref(src), C.byref(sopt()), C.byref(dst)) == E and snap(ctx, None, C.byref(sopt()), C.byref(dst)) == E
    assert snap(ctx, C.byref(src), None, C.byref(dst)) == E and snap(ctx, C.byref(src), C.byref(sopt()), None) == E and b"rnb_mesh_snap" in fns.last_error()
    assert snap(ctx, C.byref(src), C.byref(sopt()), C.byref(src)) == E and b"different objects" in fns.last_error() and b"rnb_mesh_snap" in fns.last_error()  # in place
    res4 = (C.c_uint32 * 4)(0, 0, 1, 0)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(abi_version=2), dict(abi_version=0), dict(iterations=65), dict(level=nan), dict(level=inf), dict(tolerance=-1e-6), dict(tolerance=nan), dict(tolerance=inf),
               dict(max_step=0.0), dict(max_step=-1.0), dict(max_step=nan), dict(max_step=inf), dict(max_displacement=-0.5), dict(max_displacement=nan), dict(max_displacement=inf),
               dict(min_gradient=0.0), dict(min_gradient=-0.25), dict(min_gradient=nan), dict(min_gradient=inf), dict(attributes=4), dict(attributes=0x80000001),
               dict(use_inference_params=2), dict(reserved=res4)):
        dst.n_verts = 7
        assert snap(ctx, C.byref(src), C.byref(sopt(**kw)), C.byref(dst)) == E, kw
        assert dst.n_verts == 0 and not dst.verts and b"rnb_mesh_snap" in fns.last_error()  # zeroed on failure
    src.n_indices, src.n_verts = 4, 3  # not a multiple of 3
    assert snap(ctx, C.byref(src), C.byref(sopt()), C.byref(dst)) == E and b"multiple of 3" in fns.last_error()
    src.n_indices = 3  # null buffers
    assert snap(ctx, C.byref(src), C.byref(sopt()), C.byref(dst)) == E
    assert fake.raw == b"\0" * 4096


def test_snap_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = {"rnb_mesh_snap_options": _abi.MeshSnapOptions, "rnb_mesh_snap_stats": _abi.MeshSnapStats}
    lines, want = [], []
    for cname, S in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(S))
        for field, _ in S._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field))
            want.append(getattr(S, field).offset)
    for name in ("RNB_MESH_SNAP_ABI_VERSION", "RNB_MESH_SNAP_MAX_ITERATIONS", "RNB_MESH_SNAP_MAX_IN_FLIGHT", "RNB_MESH_SNAP_RESIDUAL_LOG2", "RNB_MESH_SNAP_Q_SHIFT") + tuple(
            "RNB_MESH_SNAP_" + s.upper() for s in sr.STATE_NAMES):
        lines.append('printf("%%llu\\n", (unsigned long long)%s);' % name)
        want.append(getattr(_abi, name[4:]))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnb_mesh_snap.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want
    assert set(sr.SNAP_STATS) | {"n_network_points", "peak_workspace", "ms", "ms_network"} == set(_abi.MeshSnapStats().as_dict())


# ------------------------------------------------------------------------------------------------------------------------ the calls of the Python layer
DEVICE_CALLS = sc.DEVICE_CALLS + ("mesh_snap",)


class RecordingLibrary(sc.RecordingLibrary):
    """The smoothing stage's stand-in (tests/test_mesh_smooth_cpu.py) with this header's entry point: mesh_snap returns a mesh shaped like its input (an attribute too
    when it is asked for) and logs (input verts, output verts, select given, the four arrays asked for, iterations, attributes, use_inference_params, level)."""

    def device_log(self):
        return [e for e in self.log if e[0] in DEVICE_CALLS]

    def __getattr__(self, name):
        if name != "mesh_snap":
            return sc.RecordingLibrary.__getattr__(self, name)
        from rnb_neus2_amd import _abi

        def call(*args):
            if name == self.fail:
                self.log.append((name, ()))
                return _abi.ERR_INVALID
            src, opt, m = args[2]._obj, args[3]._obj, args[5]._obj
            m.verts, m.indices, m.n_indices = self._ptr(), self._ptr(), src.n_indices
            _abi.Mesh.n_verts.__set__(m, _abi.Mesh.n_verts.__get__(src))
            if src.colors or opt.attributes & _abi.MESH_ATTR_COLORS:
                m.colors = self._ptr()
            if src.normals or opt.attributes & _abi.MESH_ATTR_NORMALS:
                m.normals = self._ptr()
            self.meshes.add(m.verts)
            st = args[10]._obj
            st.ms, st.n_moved, st.rounds = 0.5, 4, opt.iterations + 1
            self.log.append((name, (src.verts, m.verts, int(args[4] is not None)) + tuple(int(a is not None) for a in args[6:10]) + (opt.iterations, opt.attributes, opt.use_inference_params,
                                                                                                                               opt.level)))
            return 0
        return call


def _context(fail=None):
    from rnb_neus2_amd import _abi, api
    fake = RecordingLibrary(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


V, I, COL, UP = hc.V, hc.I, hc.COL, hc.UP


def _residual(c):
    with c.upload_mesh(V, I) as m:
        return m.sdf_residual(level=0.25)


CALLS = {
    "snap_mesh": lambda c: c.snap_mesh(V, I, colors=COL, iterations=5, select=[1, 0, 0, 1], attributes=("colors", "normals"), inference=False, residuals=True, states=True, displacement=True),
    "snap_mesh_plain": lambda c: c.snap_mesh(V, I),
    "sdf_residual": lambda c: _residual(c),
    "extract_mesh": lambda c: c.extract_mesh(16, thresh=0.125, simplify=8, error=True, colors=True, fill_holes=True, smooth=dict(passes=6, only_fills=2), snap=dict(iterations=4, only_fills=True),
                                             topology=True),
    "extract_mesh_iterations": lambda c: c.extract_mesh(16, snap=2),
    "extract_mesh_defaults": lambda c: c.extract_mesh(16, snap=True, inference=False),
}
EXPECTED = {
    "snap_mesh": UP * 3 + UP + ["device_malloc"] * 4 + ["mesh_snap"] + ["memcpy"] * 4 + ["device_free"] * 5 + ["device_free"] * 3 + ["memcpy"] * 4 + ["mesh_free"],
    "snap_mesh_plain": UP * 2 + ["mesh_snap"] + ["device_free"] * 2 + ["memcpy"] * 2 + ["mesh_free"],
    "sdf_residual": UP * 2 + ["device_malloc"] * 2 + ["mesh_snap"] + ["memcpy"] * 2 + ["device_free"] * 2 + ["mesh_free"] + ["device_free"] * 2,
    "extract_mesh": ["extract_mesh", "mesh_simplify", "mesh_fill_holes"] + UP + ["device_malloc", "mesh_smooth", "memcpy", "device_free", "device_free"] + UP + ["mesh_snap", "device_free"] + [
        "mesh_distance", "mesh_distance", "mesh_topology"] + ["memcpy"] * 3 + ["mesh_free"] * 5,
    "extract_mesh_iterations": ["extract_mesh", "mesh_snap"] + ["memcpy"] * 2 + ["mesh_free"] * 2,
    "extract_mesh_defaults": ["extract_mesh", "mesh_snap"] + ["memcpy"] * 2 + ["mesh_free"] * 2,
}


def test_the_python_calls_make_the_expected_c_calls_in_order():
    from rnb_neus2_amd import _abi
    both = _abi.MESH_ATTR_COLORS | _abi.MESH_ATTR_NORMALS
    for name, call in CALLS.items():
        c, fake = _context()
        call(c)
        assert fake.names() == EXPECTED[name], (name, fake.names())
        assert not fake.buffers and not fake.meshes and not fake.errors, name
    c, fake = _context()
    out = CALLS["snap_mesh"](c)
    assert [e for e in fake.log if e[0] == "mesh_snap"][0][1][2:] == (1, 1, 1, 1, 1, 5, both, 0, 0.0)
    assert out["stats"]["n_moved"] == 4 and out["snap_stats"] is out["stats"] and all(len(out[k]) == 4 for k in ("residual_before", "residual_after", "state", "displacement"))
    assert out["state"].dtype == np.uint32 and out["residual_after"].dtype == np.float32 and "colors" in out and "normals" in out
    c, fake = _context()
    out = CALLS["snap_mesh_plain"](c)
    assert [e for e in fake.log if e[0] == "mesh_snap"][0][1][2:] == (0, 0, 0, 0, 0, 3, 0, 1, 0.0)
    assert not {"residual_before", "state", "displacement", "colors", "normals"} & set(out)
    c, fake = _context()
    res, st = CALLS["sdf_residual"](c)
    assert [e for e in fake.log if e[0] == "mesh_snap"][0][1][2:] == (0, 1, 1, 0, 0, 0, 0, 1, 0.25) and res.shape == (4,) and st["rounds"] == 1
    assert not fake.buffers and not fake.meshes and not fake.errors
    c, fake = _context()
    out = CALLS["extract_mesh"](c)
    log = {e[0]: e[1] for e in fake.device_log() if e[0].startswith("mesh_") and e[0] not in ("mesh_distance", "mesh_free")}
    assert log["mesh_smooth"][0] == log["mesh_fill_holes"][1] and log["mesh_snap"][0] == log["mesh_smooth"][1] and log["mesh_topology"][0] == log["mesh_snap"][1]  # fill -> smooth -> snap -> census
    assert log["mesh_smooth"][2:6] == (1, 0, 0, 1)  # the smoothing is asked how far it moved every vertex: the snap's selection
    assert log["mesh_snap"][2:] == (1, 0, 0, 0, 0, 4, 0, 1, 0.125)  # a selection; level = thresh
    dist = [e[1] for e in fake.device_log() if e[0] == "mesh_distance"]
    assert dist == [(log["mesh_simplify"][0], log["mesh_snap"][1]), (log["mesh_snap"][1], log["mesh_simplify"][0])]  # the error: simplifier's input <-> the snapped mesh
    assert {"simplify_stats", "fill_stats", "smooth_stats", "snap_stats", "topology", "simplify_error"} <= set(out) and out["snap_stats"]["rounds"] == 5
    c, fake = _context()
    assert CALLS["extract_mesh_iterations"](c)["snap_stats"]["rounds"] == 3
    c, fake = _context()
    assert CALLS["extract_mesh_defaults"](c)["snap_stats"]["rounds"] == 4
    assert [e for e in fake.log if e[0] == "mesh_snap"][0][1][2:] == (0, 0, 0, 0, 0, 3, 0, 0, 0.0)  # the weights of `inference`
    for bad in (dict(snap=dict(sigma=1)), dict(snap=False), dict(snap="yes"), dict(snap=dict(only_fills=True)), dict(snap=dict(iterations=65)), dict(snap=-1), dict(snap=dict(tolerance=-1.0)),
                dict(snap=dict(max_step=0.0)), dict(snap=dict(max_step=float("nan"))), dict(snap=dict(max_displacement=float("inf"))), dict(snap=dict(min_gradient=0.0)),
                dict(snap=dict(attributes=("uv",))), dict(snap=dict(level=1.0)), dict(snap=dict(inference=True))):
        c, fake = _context()
        with pytest.raises(ValueError):
            c.extract_mesh(16, **bad)
        assert not fake.device_log(), bad
    c, fake = _context()
    o = c._snap_options(iterations=7, tolerance=0.5, max_step=0.25, max_displacement=0.0, min_gradient=0.125, level=-0.5, attributes="normals", inference=False, max_points_in_flight=64)
    assert (o.iterations, o.tolerance, o.max_step, o.max_displacement, o.min_gradient, o.level, o.attributes, o.use_inference_params, o.max_points_in_flight) == (
        7, 0.5, 0.25, 0.0, 0.125, -0.5, _abi.MESH_ATTR_NORMALS, 0, 64)
    with c.upload_mesh(V, I) as m:
        with pytest.raises(ValueError):
            m.snap(select=[1, 0, 1])  # one value per vertex


def test_extract_mesh_without_snap_makes_exactly_the_calls_it_made():
    c, fake = _context()
    out = sc.CALLS["extract_mesh"](c)
    assert fake.names() == sc.EXPECTED["extract_mesh"] and "snap_stats" not in out
    assert [e for e in fake.log if e[0] == "mesh_smooth"][0][1][2:6] == (1, 0, 0, 0)  # no displacement array: nothing asks for it
    c, fake = _context()
    out = c.extract_mesh(16, simplify=8, error=True, colors=True, repair=dict(duplicates="cancel"), fill_holes=dict(max_edges=5), topology=True, snap=None)
    assert fake.names() == hc.EXPECTED["extract_mesh"] and "snap_stats" not in out
    c, fake = _context()
    c.extract_mesh(16)
    assert fake.names() == ["extract_mesh"] + ["memcpy"] * 2 + ["mesh_free"]


@pytest.mark.parametrize("stage", ["extract_mesh", "mesh_fill_holes", "mesh_smooth", "mesh_snap", "mesh_distance", "mesh_topology"])
def test_a_failing_stage_leaves_nothing_allocated(stage):
    from rnb_neus2_amd import _abi, api
    reached = 0
    for name, call in CALLS.items():
        c, fake = _context(fail=stage)
        try:
            call(c)
        except api.RnbError as e:
            assert e.code == _abi.ERR_INVALID
            reached += 1
            assert stage in [e[0] for e in fake.log], name
        else:
            assert stage not in [e[0] for e in fake.log], name
        assert not fake.buffers and not fake.meshes and not fake.errors, (name, fake.buffers, fake.meshes, fake.errors)
    assert reached >= 1
    c, fake = _context(fail=stage)
    with pytest.raises(api.RnbError):
        with c.extract_mesh_device(16, colors=True) as m, m.fill_holes() as fm, fm.smooth() as s, s.snap(select=np.ones(5), residuals=True, states=True, displacement=True) as p:
            p.sdf_residual()
            p.topology()
            m.distance_to(p)
            raise api.RnbError(_abi.ERR_INVALID, "a stage the chain does not reach")
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_a_freed_handle_stops_in_python():
    c, fake = _context()
    m = c.upload_mesh(V, I, COL)
    s = m.snap(residuals=True, states=True)
    assert isinstance(s.residual_before, np.ndarray) and len(s.residual_after) == 4 and len(s.state) == 4 and s.displacement is None and s.has_colors and s.stats["ms"] == 0.5 and m.state is None
    m.free()
    n = len(fake.log)
    for call in (lambda: m.snap(), lambda: m.snap(select=[1, 1, 1, 1], states=True), lambda: m.sdf_residual()):
        with pytest.raises(ValueError):
            call()
    assert len(fake.log) == n
    s.free()
    with pytest.raises(ValueError):
        s.sdf_residual()
    assert not fake.buffers and not fake.meshes and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    _built()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--snap=", "--snap-tolerance", "--snap-max-step", "--snap-max-displacement", "--snap-only-fills", "--snap-attributes", "--report-residual"):
        assert flag in r.stdout, flag
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--snap"], ["--snap", "x"], ["--snap", "-1"], ["--snap", "65"], ["--snap-tolerance", "0.5"], ["--snap-max-step", "0.5"], ["--snap-max-displacement", "0.5"],
                ["--snap-attributes", "keep"], ["--snap-only-fills"], ["--fill-holes", "--snap-only-fills"], ["--snap", "3", "--snap-only-fills"], ["--snap", "3", "--snap-tolerance", "-1"],
                ["--snap", "3", "--snap-tolerance", "nan"], ["--snap", "3", "--snap-max-step", "0"], ["--snap", "3", "--snap-max-step", "inf"], ["--snap", "3", "--snap-max-displacement", "-0.1"],
                ["--snap", "3", "--snap-attributes", "fresh"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    for good in (["--snap", "3"], ["--snap", "0"], ["--snap", "64", "--snap-tolerance", "0", "--snap-max-step", "0.01", "--snap-max-displacement", "0"], ["--report-residual"],
                 ["--fill-holes", "--smooth", "2", "--snap", "3", "--snap-only-fills", "--snap-attributes", "keep", "--report-residual"],
                 ["--normals", "gradient", "--snap", "5", "--snap-attributes", "resample"],
                 ["--keep-seen", "faces", "--fill-holes", "--smooth", "10", "--snap", "2", "--report-topology", "--keep", "largest", "--orient", "outward", "--texture", "64"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, good  # the flags parse; the snapshot is what is missing


def test_the_pipeline_passes_the_flags_through():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    plain = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces", fill_holes=True, smooth=2)
    assert "--snap" not in plain and "--report-residual" not in plain
    argv = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces", fill_holes=True, smooth=2,
                                            snap=dict(iterations=5, tolerance=0.001, max_step=0.01, max_displacement=0.02, only_fills=True, attributes="keep"), report_residual=True)
    assert argv[:len(plain)] == plain and argv[len(plain):] == ["--snap", "5", "--snap-tolerance", "0.001", "--snap-max-step", "0.01", "--snap-max-displacement", "0.02", "--snap-only-fills",
                                                                 "--snap-attributes", "keep", "--report-residual"]
    assert pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", snap=3)[-2:] == ["--snap", "3"]
    assert pipeline.snap_flags(dict(iterations=0)) == ["--snap", "0"] and pipeline.snap_flags(dict(iterations=1, only_fills=False)) == ["--snap", "1"]
    for bad in (dict(iterations=65), dict(tolerance=0.5), dict(iterations=3, tolerance=-1), dict(iterations=3, max_step=0), dict(iterations=3, max_displacement=float("inf")),
                dict(iterations=3, attributes="x"), dict(iterations=3, sigma=1), True, "3"):
        with pytest.raises(ValueError):
            pipeline.snap_flags(bad)
    with pytest.raises(ValueError):
        pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", snap=dict(iterations=3, only_fills=True))  # needs fill_holes
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "tb", "out", snap=3)
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "tb", "out", report_residual=True)
    common = ["-i", "in", "-t", "tb", "-o", "out"]
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--fill-holes", "--snap", "5", "--snap-tolerance", "0.001", "--snap-max-step", "0.01",
                                                          "--snap-max-displacement", "0.02", "--snap-only-fills", "--snap-attributes", "keep", "--report-residual"])
    kw = run_pipeline.pipeline_kwargs(ns)
    assert kw["snap"] == dict(iterations=5, tolerance=0.001, max_step=0.01, max_displacement=0.02, only_fills=True, attributes="keep") and kw["report_residual"] is True
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--snap", "3"])
    assert run_pipeline.pipeline_kwargs(ns)["snap"] == dict(iterations=3)
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert not [k for k in kw if k.startswith("snap") or k == "report_residual"]
    for bad in (["--snap", "3"], ["--report-residual"], ["--device-postprocess", "--snap-tolerance", "0.5"], ["--device-postprocess", "--snap-attributes", "keep"],
                ["--device-postprocess", "--snap", "65"], ["--device-postprocess", "--snap", "3", "--snap-only-fills"], ["--device-postprocess", "--snap", "3", "--snap-max-step", "0"],
                ["--device-postprocess", "--snap", "3", "--snap-attributes", "x"], ["--device-postprocess", "--snap-only-fills", "--fill-holes"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(common + bad)


def test_the_bench_tool_uses_the_public_interface():
    with open(os.path.join(ROOT, "tools", "bench_mesh_snap.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".snap(" in text and ".smooth(" in text and ".mesh_view_metrics(" in text and ".distance_to(" in text and ".self_intersections(" in text
    assert ".forward_infer_staged(" in text and "Not measured" in text and "mesh_snap_reference" in text


def test_the_documents_name_the_stage():
    for doc, needles in (("README.md", ("--snap", "rnb_mesh_snap.h", "--report-residual")), ("DESIGN.md", ("rnb_mesh_snap", "Newton")), ("INTEGRATION.md", ("rnb_mesh_snap",))):
        text = open(os.path.join(ROOT, doc), encoding="utf-8").read()
        for needle in needles:
            assert needle in text, (doc, needle)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_snap.cuh")).read())
    assert "getenv" not in src
