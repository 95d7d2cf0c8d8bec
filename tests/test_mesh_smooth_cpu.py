"""CPU tier of the smoothing stage (include/rnb_mesh_smooth.h): the numpy statement of tests/mesh_smooth_reference.py against numbers known by hand and against the
properties smoothing is run for, the C-ABI of the new header (exports, version, defaults, struct layout, argument validation without a device), the calls the Python
layer makes (through a recording stand-in of the function table), and the command-line / pipeline surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_holes_reference as hr
from tests import mesh_smooth_reference as sr
from tests import mesh_topology_reference as tr
from tests import test_mesh_holes_cpu as hc

from rnb_neus2_amd import _abi as _ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_smooth.h")
assert (sr.MAX_RING, sr.MAX_PASSES, sr.MAX_SELECT_RINGS) == (_ABI.MESH_SMOOTH_MAX_RING, _ABI.MESH_SMOOTH_MAX_PASSES, _ABI.MESH_SMOOTH_MAX_SELECT_RINGS)
assert (sr.UNUSED, sr.INTERIOR, sr.BOUNDARY, sr.NONMANIFOLD) == (_ABI.MESH_SMOOTH_KIND_UNUSED, _ABI.MESH_SMOOTH_KIND_INTERIOR, _ABI.MESH_SMOOTH_KIND_BOUNDARY, _ABI.MESH_SMOOTH_KIND_NONMANIFOLD)


# ------------------------------------------------------------------------------------------------------------------------ the statement
def test_results_known_by_hand():
    # the cube: every vertex interior; one pass with lambda 1 puts a vertex at the centroid of its neighbours. Vertex 0 has the three along its edges and the far ends of
    # the three face diagonals its faces are cut by or not: whatever they are, the statement's census says which
    v, t = tr.cube()
    r = sr.expected_smooth(v, t, passes=1, lam=1.0, mu=0.0)
    assert r["stats"] == dict(n_edges=18, n_interior=8, n_boundary=0, n_nonmanifold=0, n_unused=0, n_selected=8, n_moving=8, max_valence=int(r["valence"].max()), passes=1,
                              max_displacement=float(r["displacement"].max()))
    assert r["valence"].sum() == 36 and (r["kind"] == sr.INTERIOR).all()
    for k in range(8):
        nb = hr.neighbours(t, k)
        assert len(nb) == r["valence"][k] and np.allclose(r["verts"][k], v[nb].astype(np.float64).mean(0), atol=2.0 ** -31)
    # disc(9): the centre is interior with 9 neighbours, the rim is boundary with 3 (two along the rim, the centre)
    v, t = tr.disc(9)
    pin = sr.expected_smooth(v, t, passes=1, lam=1.0, mu=0.0)
    assert list(pin["kind"]) == [sr.INTERIOR] + [sr.BOUNDARY] * 9 and list(pin["valence"]) == [9] + [3] * 9 and pin["stats"]["n_moving"] == 1
    assert pin["verts"][1:].tobytes() == v[1:].tobytes() and np.allclose(pin["verts"][0], [0.5, 0.5, 0.5], atol=1e-7)  # the rim pinned; the centre is the rim's centroid already
    slide = sr.expected_smooth(v, t, passes=1, lam=1.0, mu=0.0, boundary="slide")
    free = sr.expected_smooth(v, t, passes=1, lam=1.0, mu=0.0, boundary="free")
    assert slide["stats"]["n_moving"] == free["stats"]["n_moving"] == 10
    p = v.astype(np.float64)
    assert np.allclose(slide["verts"][1], (p[2] + p[9]) / 2, atol=1e-7)  # the midpoint of its two neighbours along the rim
    assert np.allclose(free["verts"][1], (p[2] + p[9] + p[0]) / 3, atol=1e-7)  # ... and the centre
    radius = lambda x: np.linalg.norm(x.astype(np.float64)[1:, :2] - 0.5, axis=1)
    assert np.allclose(radius(slide["verts"]), 0.3 * np.cos(2 * np.pi / 9), atol=1e-6) and (radius(free["verts"]) < radius(slide["verts"])).all()
    assert np.allclose(slide["displacement"][1:], 0.3 * (1 - np.cos(2 * np.pi / 9)), atol=1e-6) and slide["stats"]["max_displacement"] == float(slide["displacement"].max())
    # a vertex on an edge with three faces stays, whatever the boundary mode; so does a vertex nothing uses, and one only a degenerate triangle uses
    v, t = tr.book(3)
    v = np.concatenate([v, [[0.1, 0.2, 0.3], [0.4, 0.4, 0.4]]]).astype(np.float32)
    t = np.concatenate([t, [[6, 6, 2]]])
    for boundary in ("pin", "slide", "free"):
        r = sr.expected_smooth(v, t, boundary=boundary)
        assert list(r["kind"][:2]) == [sr.NONMANIFOLD] * 2 and list(r["kind"][5:]) == [sr.UNUSED] * 2 and (r["kind"][2:5] == sr.BOUNDARY).all()
        assert r["verts"][[0, 1, 5, 6]].tobytes() == v[[0, 1, 5, 6]].tobytes() and not r["moving"][[0, 1, 5, 6]].any() and r["stats"]["n_edges"] == 7
        assert r["moving"][2:5].all() == (boundary != "pin")
    # passes = 0: a copy and the census
    r = sr.expected_smooth(v, t, passes=0, boundary="free")
    assert r["verts"].tobytes() == v.tobytes() and (r["displacement"] == 0).all() and r["stats"]["n_moving"] == 3
    # odd passes use lambda, even ones mu
    v, t = tr.sphere(32)
    one, two = sr.expected_smooth(v, t, passes=1), sr.expected_smooth(v, t, passes=2)
    back = sr.expected_smooth(one["verts"], t, passes=1, lam=0.53)  # a step of +0.53 from there is not the step of -0.53
    assert two["verts"].tobytes() != back["verts"].tobytes() and sr.expected_smooth(v, t, passes=2, mu=0.0)["verts"].tobytes() != two["verts"].tobytes()
    with pytest.raises(ValueError):
        far = v.copy()
        far[0, 0] = 2.0 ** 11
        sr.expected_smooth(far, t)
    with pytest.raises(ValueError):
        nan = v.copy()
        nan[0, 2] = np.nan
        sr.expected_smooth(nan, t)


def test_the_statement_does_not_depend_on_the_order_of_the_triangles_or_the_numbering():
    v, t, _ = hr.grid_sheet_with_holes(12, 12)
    rng = np.random.default_rng(3)
    v = (v + rng.normal(0, 0.002, v.shape)).astype(np.float32)
    a = sr.expected_smooth(v, t, boundary="slide", passes=6)
    b = sr.expected_smooth(v, t[rng.permutation(len(t))], boundary="slide", passes=6)
    assert a["verts"].tobytes() == b["verts"].tobytes() and a["displacement"].tobytes() == b["displacement"].tobytes() and a["stats"] == b["stats"]
    v2, t2, new_of_old = tr.renumber(v, t, rng)
    c = sr.expected_smooth(v2, t2, boundary="slide", passes=6)
    assert c["verts"][new_of_old].tobytes() == a["verts"].tobytes() and c["kind"][new_of_old].tobytes() == a["kind"].tobytes() and c["stats"] == a["stats"]
    na, nc = sr.expected_normals(v, t), sr.expected_normals(v2, t2)
    assert nc["normals"][new_of_old].tobytes() == na["normals"].tobytes() and na["stats"] == nc["stats"]


def test_selection_rings_on_a_strip():
    n = 20
    v, t = tr.strip(n)  # vertex k neighbours k - 2 .. k + 2
    ends = sr.edges(len(v), t)[0]
    select = np.zeros(n + 2, bool)
    select[10] = True
    for rings in (0, 1, 2, 3, 1024):
        sel = sr.selection(n + 2, ends, select, rings)
        want = np.abs(np.arange(n + 2) - 10) <= 2 * rings
        assert np.array_equal(sel, want), rings
        r = sr.expected_smooth(v, t, select=select, select_rings=rings, boundary="free")
        assert r["stats"]["n_selected"] == want.sum() == r["stats"]["n_moving"] and r["verts"][~want].tobytes() == v[~want].tobytes()
    assert sr.selection(n + 2, ends, None, 0).all()
    assert sr.expected_smooth(v, t, select=select, select_rings=3)["stats"]["n_moving"] == 0  # every vertex of a strip is on its boundary: pinned


def _volume(v, t):
    p = v.astype(np.float64)[t]
    return abs(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def test_taubin_keeps_the_volume_and_laplacian_does_not():
    """sphere(32) with N(0, 0.01 r) noise, seed 1, 20 passes. Measured on the statement: Taubin (0.5, -0.53) volume ratio to the clean sphere 1.0031, plain Laplacian
    (0.5, 0) 0.8724; the standard deviation of the radius, in units of r, 0.0099 -> 0.0039 under Taubin."""
    v, t = tr.sphere(32)
    c = v.astype(np.float64).mean(0)
    r0 = np.linalg.norm(v - c, axis=1).mean()
    noisy = (v + np.random.default_rng(1).normal(0, 0.01 * r0, v.shape)).astype(np.float32)
    taubin = sr.expected_smooth(noisy, t, passes=20)["verts"]
    laplace = sr.expected_smooth(noisy, t, passes=20, mu=0.0)["verts"]
    deviation = lambda x: (np.linalg.norm(x.astype(np.float64) - c, axis=1) - r0).std() / r0
    ratios = _volume(taubin, t) / _volume(v, t), _volume(laplace, t) / _volume(v, t)
    print("volume ratios", ratios, "deviation", deviation(noisy), "->", deviation(taubin))
    assert abs(ratios[0] - 1.0) < 0.01 and ratios[1] < 0.90 and deviation(taubin) < 0.5 * deviation(noisy)
    assert abs(ratios[0] - 1.0031) < 5e-4 and abs(ratios[1] - 0.8724) < 5e-4 and abs(deviation(noisy) - 0.0099) < 5e-4 and abs(deviation(taubin) - 0.0039) < 5e-4  # as measured


def _angle_deg(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    s = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arcsin(np.clip(s, 0, 1))), (a * b).sum(1)


def _host_normals(tmp_path, v, t):
    """mesh::compute_normals (host/mesh.hpp), compiled into a small program."""
    src = tmp_path / "n.cpp"
    src.write_text('''#include "mesh.hpp"
#include <cstdio>
int main(int argc, char** argv) {
	mesh::Mesh m;
	FILE* f = std::fopen(argv[1], "rb");
	uint32_t n[2];
	if (!f || std::fread(n, 4, 2, f) != 2) return 1;
	m.verts.resize(n[0]); m.indices.resize(n[1]);
	if (std::fread(m.verts.data(), 12, n[0], f) != n[0] || std::fread(m.indices.data(), 4, n[1], f) != n[1]) return 1;
	std::fclose(f);
	mesh::compute_normals(m);
	f = std::fopen(argv[2], "wb");
	std::fwrite(m.normals.data(), 12, n[0], f);
	std::fclose(f);
	return 0;
}
''')
    exe = tmp_path / "n"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "rnb-neus2_amd", "host"), str(src), "-o", str(exe), "-lz"])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.uint32([len(v), 3 * len(t)]).tobytes() + np.ascontiguousarray(v, np.float32).tobytes() + np.ascontiguousarray(t, np.uint32).tobytes())
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    return np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 3)


def test_normals_are_unit_outward_and_minus_the_hosts(tmp_path):
    v, t = tr.sphere(32)
    c = np.float32([0.5, 0.5, 0.5])
    n = sr.expected_normals(v, t)
    assert n["stats"] == dict(n_zero=0, max_corners=int(np.bincount(t.ravel()).max()))
    assert np.abs(np.linalg.norm(n["normals"].astype(np.float64), axis=1) - 1).max() < 1e-7
    assert ((n["normals"] * (v - c)).sum(1) > 0.9 * np.linalg.norm(v - c, axis=1)).all()  # outward: the sphere is wound counter-clockwise seen from outside
    flipped = sr.expected_normals(v, t, flip=True)["normals"]
    assert np.array_equal(flipped, -n["normals"])
    # a vertex without a triangle, and one whose triangles cancel: zero
    lone = sr.expected_normals(np.concatenate([v, [[0, 0, 0]]]).astype(np.float32), t)
    assert lone["stats"]["n_zero"] == 1 and lone["normals"][-1].tobytes() == np.zeros(3, np.float32).tobytes()
    # the truncation: on the sphere scaled to a mean edge of 2^-11 the statement turns the normal by at most 6.6e-4 degrees against unquantised float64 sums (measured
    # here: 6.61e-4); the host's mesh::compute_normals sums the same cross products, negated, in float32, and may differ from the statement by twice that
    p = v.astype(np.float64)[t]
    edge = np.linalg.norm(p[:, 1] - p[:, 0], axis=1).mean()
    small = ((v - c) * np.float32(2.0 ** -11 / edge) + c).astype(np.float32)
    q = sr.expected_normals(small, t)["normals"]
    d = small.astype(np.float64)
    cr = np.cross(d[t[:, 1]] - d[t[:, 0]], d[t[:, 2]] - d[t[:, 0]])
    exact = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(exact, t[:, k], cr)
    measured = _angle_deg(q, exact)[0].max()
    print("statement against float64 sums: %.3g degrees" % measured)
    assert 3.3e-4 < measured < 1.0e-3  # about the 6.6e-4 written above (the issue's sphere, a little finer, gave 1.0e-3)
    host = _host_normals(tmp_path, small, t)
    angle, dot = _angle_deg(q, -host)
    print("statement against minus the host's: %.3g degrees" % angle.max())
    assert (dot > 0).all() and angle.max() <= 2 * 6.61e-4
    angle, dot = _angle_deg(n["normals"], -_host_normals(tmp_path, v, t))
    assert (dot > 0).all() and angle.max() <= 2 * 6.61e-4  # at the mesh's own size the truncation is far below that


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def _built():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api
    return api.load_library()


def test_smooth_header_is_exported_by_the_hip_library():
    fns = _built()
    from rnb_neus2_amd import api, _abi, build
    names = hc._functions(HEADER)
    assert names == ["rnb_mesh_smooth", "rnb_mesh_smooth_abi_version", "rnb_mesh_smooth_default_options", "rnb_mesh_vertex_normals", "rnb_mesh_vertex_normals_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_SMOOTH_PROTOTYPES) == set(names)
    others = [getattr(_abi, n) for n in dir(_abi) if n.endswith("PROTOTYPES") and n != "MESH_SMOOTH_PROTOTYPES"]
    assert len(others) >= 12 and not any(set(_abi.MESH_SMOOTH_PROTOTYPES) & set(o) for o in others)  # a table of its own
    assert fns.mesh_smooth_abi_version() == _abi.MESH_SMOOTH_ABI_VERSION == 1
    o = _abi.MeshSmoothOptions()
    assert fns.mesh_smooth_default_options(C.byref(o)) == 0
    assert (o.abi_version, o.passes, o.lambda_, o.mu, o.boundary, o.select_rings, o.normals, o.buckets_log2, list(o.reserved)) == (1, 2, 0.5, -0.53, 0, 0, 0, 0, [0] * 4)
    n = _abi.MeshVertexNormalsOptions()
    assert fns.mesh_vertex_normals_default_options(C.byref(n)) == 0 and (n.abi_version, n.flip, list(n.reserved)) == (1, 0, [0] * 4)
    assert fns.mesh_smooth_default_options(None) == _abi.ERR_INVALID and fns.mesh_vertex_normals_default_options(None) == _abi.ERR_INVALID
    for name in ("smooth_mesh", "mesh_vertex_normals"):
        assert hasattr(api.Context, name)
    for name in ("smooth", "vertex_normals"):
        assert hasattr(api.DeviceMesh, name)
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS
    text = open(HEADER).read()
    assert "counter-clockwise" in text and "compute_normals" in text and "flip = 1" in text  # the sign of the normals is said where a caller reads it


def test_smooth_validates_its_arguments_without_a_device():
    """Null pointers, a wrong version, every option outside its range, reserved words, n_indices % 3, null buffers and in == out are refused before the context or the
    device is touched: the context handed in here is a block of zeros, and no device exists where this test runs."""
    fns = _built()
    from rnb_neus2_amd import _abi
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def sopt(**kw):
        o = _abi.MeshSmoothOptions()
        assert fns.mesh_smooth_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def nopt(**kw):
        o = _abi.MeshVertexNormalsOptions()
        assert fns.mesh_vertex_normals_default_options(C.byref(o)) == 0
        for k, val in kw.items():
            setattr(o, k, val)
        return o

    def smooth(ctx_, m, o, out):
        return fns.mesh_smooth(ctx_, None, m, o, None, out, None, None, None, None)

    def normals(ctx_, m, o, buf=None):
        return fns.mesh_vertex_normals(ctx_, None, m, o, buf, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    E = _abi.ERR_INVALID
    assert smooth(None, C.byref(src), C.byref(sopt()), C.byref(dst)) == E and smooth(ctx, None, C.byref(sopt()), C.byref(dst)) == E
    assert smooth(ctx, C.byref(src), None, C.byref(dst)) == E and smooth(ctx, C.byref(src), C.byref(sopt()), None) == E and b"rnb_mesh_smooth" in fns.last_error()
    assert smooth(ctx, C.byref(src), C.byref(sopt()), C.byref(src)) == E and b"different objects" in fns.last_error() and b"rnb_mesh_smooth" in fns.last_error()  # in place
    assert normals(None, C.byref(src), C.byref(nopt())) == E and normals(ctx, None, C.byref(nopt())) == E and normals(ctx, C.byref(src), None) == E
    assert b"rnb_mesh_vertex_normals" in fns.last_error()
    res4 = (C.c_uint32 * 4)(0, 0, 1, 0)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(abi_version=2), dict(abi_version=0), dict(passes=10001), dict(lambda_=0.0), dict(lambda_=1.5), dict(lambda_=-0.5), dict(lambda_=nan), dict(lambda_=inf), dict(mu=0.1),
               dict(mu=-1.6), dict(mu=nan), dict(mu=-inf), dict(boundary=3), dict(select_rings=1025), dict(normals=2), dict(buckets_log2=3), dict(buckets_log2=31), dict(reserved=res4)):
        dst.n_verts = 7
        assert smooth(ctx, C.byref(src), C.byref(sopt(**kw)), C.byref(dst)) == E, kw
        assert dst.n_verts == 0 and not dst.verts and b"rnb_mesh_smooth" in fns.last_error()  # zeroed on failure
    for kw in (dict(abi_version=2), dict(flip=2), dict(reserved=res4)):
        assert normals(ctx, C.byref(src), C.byref(nopt(**kw))) == E and b"rnb_mesh_vertex_normals" in fns.last_error(), kw
    src.n_indices, src.n_verts = 4, 3  # not a multiple of 3
    assert smooth(ctx, C.byref(src), C.byref(sopt()), C.byref(dst)) == E and b"multiple of 3" in fns.last_error() and normals(ctx, C.byref(src), C.byref(nopt())) == E
    src.n_indices = 3  # null buffers
    assert smooth(ctx, C.byref(src), C.byref(sopt()), C.byref(dst)) == E and normals(ctx, C.byref(src), C.byref(nopt())) == E
    assert fake.raw == b"\0" * 4096


def test_smooth_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    structs = {"rnb_mesh_smooth_options": _abi.MeshSmoothOptions, "rnb_mesh_smooth_stats": _abi.MeshSmoothStats, "rnb_mesh_vertex_normals_options": _abi.MeshVertexNormalsOptions,
               "rnb_mesh_vertex_normals_stats": _abi.MeshVertexNormalsStats}
    lines, want = [], []
    for cname, S in structs.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(S))
        for field, _ in S._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, field.rstrip("_")))  # (lambda is a keyword in Python)
            want.append(getattr(S, field).offset)
    for name in ("RNB_MESH_SMOOTH_ABI_VERSION", "RNB_MESH_SMOOTH_MAX_RING", "RNB_MESH_SMOOTH_MAX_PASSES", "RNB_MESH_SMOOTH_MAX_SELECT_RINGS", "RNB_MESH_SMOOTH_Q_SHIFT",
                 "RNB_MESH_SMOOTH_Q_TERM_LOG2", "RNB_MESH_SMOOTH_NORMAL_Q_SHIFT", "RNB_MESH_SMOOTH_NORMAL_Q_TERM_LOG2", "RNB_MESH_SMOOTH_KIND_UNUSED", "RNB_MESH_SMOOTH_KIND_INTERIOR",
                 "RNB_MESH_SMOOTH_KIND_BOUNDARY", "RNB_MESH_SMOOTH_KIND_NONMANIFOLD", "RNB_MESH_SMOOTH_BOUNDARY_PIN", "RNB_MESH_SMOOTH_BOUNDARY_SLIDE", "RNB_MESH_SMOOTH_BOUNDARY_FREE",
                 "RNB_MESH_SMOOTH_NORMALS_KEEP", "RNB_MESH_SMOOTH_NORMALS_RECOMPUTE"):
        lines.append('printf("%%llu\\n", (unsigned long long)%s);' % name)
        want.append(getattr(_abi, name[4:]))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rnb_mesh_smooth.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want
    assert (sr.Q_SCALE, sr.TERM_LIMIT, sr.NORMAL_Q_SCALE, sr.NORMAL_TERM_LIMIT) == (2.0 ** _abi.MESH_SMOOTH_Q_SHIFT, 2.0 ** _abi.MESH_SMOOTH_Q_TERM_LOG2, 2.0 ** _abi.MESH_SMOOTH_NORMAL_Q_SHIFT,
                                                                                 2.0 ** _abi.MESH_SMOOTH_NORMAL_Q_TERM_LOG2)
    assert set(sr.SMOOTH_STATS) | {"n_wide", "peak_workspace", "ms", "ms_passes"} == set(_abi.MeshSmoothStats().as_dict())
    assert set(sr.NORMALS_STATS) | {"peak_workspace", "ms"} == set(_abi.MeshVertexNormalsStats().as_dict())


# ------------------------------------------------------------------------------------------------------------------------ the calls of the Python layer
DEVICE_CALLS = hc.DEVICE_CALLS + ("mesh_smooth", "mesh_vertex_normals", "mesh_intersections", "mesh_intersections_select")


class RecordingLibrary(hc.RecordingLibrary):
    """The hole stage's stand-in (tests/test_mesh_holes_cpu.py) with the two entry points of this header: mesh_smooth returns a mesh shaped like its input (normals too
    when asked to recompute) and logs (input verts, output verts, select given, the arrays asked for, passes, select_rings, boundary, normals); mesh_vertex_normals logs
    (input verts, flip)."""

    def device_log(self):
        return [e for e in self.log if e[0] in DEVICE_CALLS]

    def __getattr__(self, name):
        if name not in ("mesh_smooth", "mesh_vertex_normals"):
            return hc.RecordingLibrary.__getattr__(self, name)
        from rnb_neus2_amd import _abi

        def call(*args):
            if name == self.fail:
                self.log.append((name, ()))
                return _abi.ERR_INVALID
            src, opt = args[2]._obj, args[3]._obj
            if name == "mesh_vertex_normals":
                args[5]._obj.ms = 0.25
                self.log.append((name, (src.verts, opt.flip)))
                return 0
            m = args[5]._obj
            m.verts, m.indices, m.n_indices = self._ptr(), self._ptr(), src.n_indices
            _abi.Mesh.n_verts.__set__(m, _abi.Mesh.n_verts.__get__(src))
            if src.colors:
                m.colors = self._ptr()
            if src.normals or opt.normals == _abi.MESH_SMOOTH_NORMALS_RECOMPUTE:
                m.normals = self._ptr()
            self.meshes.add(m.verts)
            st = args[9]._obj
            st.ms, st.n_moving, st.passes = 0.5, 4, opt.passes
            self.log.append((name, (src.verts, m.verts, int(args[4] is not None)) + tuple(int(a is not None) for a in args[6:9]) + (opt.passes, opt.select_rings, opt.boundary, opt.normals)))
            return 0
        return call


def _context(fail=None):
    from rnb_neus2_amd import _abi, api
    fake = RecordingLibrary(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


V, I, COL, UP = hc.V, hc.I, hc.COL, hc.UP
CALLS = {
    "smooth_mesh": lambda c: c.smooth_mesh(V, I, colors=COL, passes=4, boundary="slide", select=[1, 0, 0, 1], select_rings=2, displacement=True, census=True),
    "smooth_mesh_plain": lambda c: c.smooth_mesh(V, I),
    "mesh_vertex_normals": lambda c: c.mesh_vertex_normals(V, I, flip=True),
    "extract_mesh": lambda c: c.extract_mesh(16, simplify=8, error=True, colors=True, fill_holes=True, smooth=dict(passes=6, only_fills=2), topology=True),
    "extract_mesh_passes": lambda c: c.extract_mesh(16, smooth=3),
    "extract_mesh_defaults": lambda c: c.extract_mesh(16, smooth=True),
}
EXPECTED = {
    "smooth_mesh": UP * 3 + UP + ["device_malloc"] * 3 + ["mesh_smooth"] + ["memcpy"] * 3 + ["device_free"] * 4 + ["device_free"] * 3 + ["memcpy"] * 3 + ["mesh_free"],
    "smooth_mesh_plain": UP * 2 + ["mesh_smooth"] + ["device_free"] * 2 + ["memcpy"] * 2 + ["mesh_free"],
    "mesh_vertex_normals": UP * 2 + ["device_malloc", "mesh_vertex_normals", "memcpy", "device_free"] + ["device_free"] * 2,
    "extract_mesh": ["extract_mesh", "mesh_simplify", "mesh_fill_holes"] + UP + ["mesh_smooth", "device_free", "mesh_distance", "mesh_distance", "mesh_topology"] + ["memcpy"] * 3 + ["mesh_free"] * 4,
    "extract_mesh_passes": ["extract_mesh", "mesh_smooth"] + ["memcpy"] * 2 + ["mesh_free"] * 2,
    "extract_mesh_defaults": ["extract_mesh", "mesh_smooth"] + ["memcpy"] * 2 + ["mesh_free"] * 2,
}


def test_the_python_calls_make_the_expected_c_calls_in_order():
    from rnb_neus2_amd import _abi
    for name, call in CALLS.items():
        c, fake = _context()
        call(c)
        assert fake.names() == EXPECTED[name], (name, fake.names())
        assert not fake.buffers and not fake.meshes and not fake.errors, name
    c, fake = _context()
    out = CALLS["smooth_mesh"](c)
    assert [e for e in fake.log if e[0] == "mesh_smooth"][0][1][2:] == (1, 1, 1, 1, 4, 2, _abi.MESH_SMOOTH_BOUNDARY_SLIDE, _abi.MESH_SMOOTH_NORMALS_KEEP)
    assert out["stats"]["n_moving"] == 4 and out["smooth_stats"] is out["stats"] and all(len(out[k]) == 4 for k in ("displacement", "valence", "kind")) and "colors" in out
    assert out["displacement"].dtype == np.float32 and out["kind"].dtype == np.uint32
    c, fake = _context()
    out = CALLS["smooth_mesh_plain"](c)
    assert [e for e in fake.log if e[0] == "mesh_smooth"][0][1][2:] == (0, 0, 0, 0, 2, 0, _abi.MESH_SMOOTH_BOUNDARY_PIN, _abi.MESH_SMOOTH_NORMALS_KEEP)
    assert "displacement" not in out and "kind" not in out and "normals" not in out
    c, fake = _context()
    assert "normals" in c.smooth_mesh(V, I, normals="recompute")  # made by the stage, whether or not the input has any
    c, fake = _context()
    out = CALLS["mesh_vertex_normals"](c)
    assert [e for e in fake.log if e[0] == "mesh_vertex_normals"][0][1][1] == 1 and out["normals"].shape == (4, 3) and out["ms"] == 0.25
    c, fake = _context()
    out = CALLS["extract_mesh"](c)
    log = {e[0]: e[1] for e in fake.device_log() if e[0].startswith("mesh_") and e[0] not in ("mesh_distance", "mesh_free")}
    assert log["mesh_smooth"][0] == log["mesh_fill_holes"][1] and log["mesh_topology"][0] == log["mesh_smooth"][1]  # fill -> smooth -> the census of the result
    assert log["mesh_smooth"][2:] == (1, 0, 0, 0, 6, 2, _abi.MESH_SMOOTH_BOUNDARY_PIN, _abi.MESH_SMOOTH_NORMALS_KEEP)  # a selection, grown by only_fills rings
    dist = [e[1] for e in fake.device_log() if e[0] == "mesh_distance"]
    assert dist == [(log["mesh_simplify"][0], log["mesh_smooth"][1]), (log["mesh_smooth"][1], log["mesh_simplify"][0])]  # the error: simplifier's input <-> the smoothed mesh
    assert {"simplify_stats", "fill_stats", "smooth_stats", "topology", "simplify_error"} <= set(out) and out["smooth_stats"]["passes"] == 6
    c, fake = _context()
    assert CALLS["extract_mesh_passes"](c)["smooth_stats"]["passes"] == 3
    c, fake = _context()
    assert CALLS["extract_mesh_defaults"](c)["smooth_stats"]["passes"] == 2
    for bad in (dict(smooth=dict(sigma=1)), dict(smooth=False), dict(smooth="yes"), dict(smooth=dict(only_fills=1)), dict(smooth=dict(only_fills=1, select_rings=1), fill_holes=True),
                dict(smooth=dict(passes=10001)), dict(smooth=dict(lam=0.0)), dict(smooth=dict(mu=0.5)), dict(smooth=dict(boundary="loose")), dict(smooth=-1)):
        c, fake = _context()
        with pytest.raises(ValueError):
            c.extract_mesh(16, **bad)
        assert not fake.device_log(), bad
    c, fake = _context()
    o = c._smooth_options(passes=7, lam=0.25, mu=-0.3, boundary="free", select_rings=9, normals="recompute", buckets_log2=5)
    assert (o.passes, o.lambda_, o.mu, o.boundary, o.select_rings, o.normals, o.buckets_log2) == (7, 0.25, -0.3, 2, 9, 1, 5) and c._vertex_normals_options(True).flip == 1
    with c.upload_mesh(V, I) as m:
        with pytest.raises(ValueError):
            m.smooth(select=[1, 0, 1])  # one value per vertex


def test_extract_mesh_without_smooth_makes_exactly_the_calls_it_made():
    c, fake = _context()
    out = c.extract_mesh(16, simplify=8, error=True, colors=True, repair=dict(duplicates="cancel"), fill_holes=dict(max_edges=5), topology=True, smooth=None)
    assert fake.names() == hc.EXPECTED["extract_mesh"] and "smooth_stats" not in out
    c, fake = _context()
    out = c.extract_mesh(16, fill_holes=True)
    assert fake.names() == hc.EXPECTED["extract_mesh_defaults"] and "smooth_stats" not in out
    c, fake = _context()
    c.extract_mesh(16)
    assert fake.names() == ["extract_mesh"] + ["memcpy"] * 2 + ["mesh_free"]


@pytest.mark.parametrize("stage", ["extract_mesh", "mesh_simplify", "mesh_fill_holes", "mesh_smooth", "mesh_vertex_normals", "mesh_distance", "mesh_topology"])
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
        with c.extract_mesh_device(16, colors=True) as m, m.simplify((0, 0, 0), 0.25, 4) as sm, sm.fill_holes() as fm, fm.smooth(select=np.ones(5), displacement=True, census=True) as s:
            s.vertex_normals()
            c.device_free(s.vertex_normals(on_device=True)["normals"])  # the caller's to release
            s.topology()
            sm.distance_to(s)
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_a_freed_handle_stops_in_python():
    c, fake = _context()
    m = c.upload_mesh(V, I, COL)
    s = m.smooth(displacement=True, census=True)
    assert isinstance(s.displacement, np.ndarray) and len(s.displacement) == 4 and len(s.kind) == 4 and s.has_colors and s.stats["ms"] == 0.5 and m.displacement is None
    on = s.vertex_normals(on_device=True)
    assert on["normals"] in fake.buffers  # the caller's from here on
    c.device_free(on["normals"])
    m.free()
    n = len(fake.log)
    for call in (lambda: m.smooth(), lambda: m.smooth(select=[1, 1, 1, 1], census=True), lambda: m.vertex_normals(), lambda: m.vertex_normals(on_device=True)):
        with pytest.raises(ValueError):
            call()
    assert len(fake.log) == n
    s.free()
    with pytest.raises(ValueError):
        s.vertex_normals()
    assert not fake.buffers and not fake.meshes and not fake.errors


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    _built()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--smooth=", "--smooth-lambda", "--smooth-mu", "--smooth-boundary", "--smooth-only-fills", "--smooth-normals"):
        assert flag in r.stdout, flag
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--smooth"], ["--smooth", "x"], ["--smooth", "-1"], ["--smooth", "10001"], ["--smooth-lambda", "0.5"], ["--smooth-mu", "-0.5"], ["--smooth-boundary", "slide"],
                ["--smooth-normals", "keep"], ["--smooth", "10", "--smooth-only-fills", "2"], ["--fill-holes", "--smooth-only-fills", "2"], ["--smooth", "10", "--smooth-lambda", "0"],
                ["--smooth", "10", "--smooth-lambda", "1.5"], ["--smooth", "10", "--smooth-lambda", "nan"], ["--smooth", "10", "--smooth-mu", "0.1"], ["--smooth", "10", "--smooth-mu", "-2"],
                ["--smooth", "10", "--smooth-boundary", "loose"], ["--smooth", "10", "--smooth-normals", "ring"], ["--fill-holes", "--smooth", "10", "--smooth-only-fills", "1025"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    for good in (["--smooth", "10"], ["--smooth", "0"], ["--fill-holes", "--smooth", "20", "--smooth-lambda", "0.33", "--smooth-mu", "-0.34", "--smooth-boundary", "slide", "--smooth-only-fills", "3"],
                 ["--normals", "gradient", "--smooth", "5", "--smooth-normals", "keep"], ["--smooth", "5", "--smooth-mu", "0", "--smooth-boundary", "free", "--smooth-normals", "recompute"],
                 ["--keep-seen", "faces", "--fill-holes", "--smooth", "10", "--report-topology", "--keep", "largest", "--orient", "outward", "--texture", "64"]):
        r = subprocess.run([exe] + base + good, capture_output=True, text=True)
        assert r.returncode == 1 and "does not exist" in r.stderr, good  # the flags parse; the snapshot is what is missing


def test_the_pipeline_passes_the_flags_through():
    import run_pipeline
    from rnb_neus2_amd import pipeline
    plain = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces", fill_holes=True)
    assert "--smooth" not in plain
    argv = pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", simplify=8, keep_seen="faces", fill_holes=True,
                                            smooth=dict(passes=20, lam=0.4, mu=-0.41, boundary="slide", only_fills=2, normals="recompute"))
    assert argv[:len(plain)] == plain and argv[len(plain):] == ["--smooth", "20", "--smooth-lambda", "0.4", "--smooth-mu", "-0.41", "--smooth-boundary", "slide", "--smooth-only-fills", "2",
                                                                 "--smooth-normals", "recompute"]
    assert pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", smooth=10)[-2:] == ["--smooth", "10"]
    assert pipeline.smooth_flags(dict(passes=0)) == ["--smooth", "0"]
    for bad in (dict(passes=10001), dict(lam=0.5), dict(passes=5, lam=0), dict(passes=5, mu=0.2), dict(passes=5, boundary="x"), dict(passes=5, sigma=1), True, "10"):
        with pytest.raises(ValueError):
            pipeline.smooth_flags(bad)
    with pytest.raises(ValueError):
        pipeline.plan_device_postprocess("/d", 100, 128, "/o/mesh.obj", "/b/mesh", smooth=dict(passes=5, only_fills=1))  # needs fill_holes
    with pytest.raises(ValueError):
        pipeline.run_full_pipeline("in", "tb", "out", smooth=10)
    common = ["-i", "in", "-t", "tb", "-o", "out"]
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--fill-holes", "--smooth", "20", "--smooth-lambda", "0.4", "--smooth-mu", "-0.41", "--smooth-boundary", "slide",
                                                          "--smooth-only-fills", "2", "--smooth-normals", "keep"])
    assert run_pipeline.pipeline_kwargs(ns)["smooth"] == dict(passes=20, lam=0.4, mu=-0.41, boundary="slide", only_fills=2, normals="keep")
    ns = run_pipeline.build_parser().parse_args(common + ["--device-postprocess", "--smooth", "10"])
    assert run_pipeline.pipeline_kwargs(ns)["smooth"] == dict(passes=10)
    kw = run_pipeline.pipeline_kwargs(run_pipeline.build_parser().parse_args(common + ["--device-postprocess"]))
    assert not [k for k in kw if k.startswith("smooth")]
    for bad in (["--smooth", "10"], ["--device-postprocess", "--smooth-lambda", "0.5"], ["--device-postprocess", "--smooth-boundary", "pin"], ["--device-postprocess", "--smooth", "10001"],
                ["--device-postprocess", "--smooth", "10", "--smooth-only-fills", "2"], ["--device-postprocess", "--smooth", "10", "--smooth-mu", "0.5"],
                ["--device-postprocess", "--smooth", "10", "--smooth-boundary", "x"]):
        with pytest.raises(SystemExit):
            run_pipeline.main(common + bad)


def test_the_bench_tool_uses_the_public_interface():
    with open(os.path.join(ROOT, "tools", "bench_mesh_smooth.py")) as f:
        text = f.read()
    for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
        assert needle not in text, needle
    assert "mesh_bench_common" in text and ".smooth(" in text and ".vertex_normals(" in text and ".topology(" in text and ".mesh_view_metrics(" in text and ".distance_to(" in text
    assert ".self_intersections(" in text and "mesh_smooth_reference" in text and "Not measured" in text
    assert os.path.exists(os.path.join(ROOT, "profiles", "mesh_smooth.md"))


def test_the_documents_name_the_stage():
    for doc, needles in (("README.md", ("--smooth", "rnb_mesh_smooth.h")), ("DESIGN.md", ("rnb_mesh_smooth", "Taubin")), ("INTEGRATION.md", ("rnb_mesh_smooth",))):
        text = open(os.path.join(ROOT, doc), encoding="utf-8").read()
        for needle in needles:
            assert needle in text, (doc, needle)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "rnb-neus2_amd", "csrc", "kernels_mesh_smooth.cuh")).read())
    assert "getenv" not in src
