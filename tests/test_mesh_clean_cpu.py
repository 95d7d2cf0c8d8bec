"""CPU tier of the mesh cleaner (include/rnb_mesh_clean.h): the C-ABI of the new header (exports, version, defaults, struct layout, argument validation without a
device), the numpy statement of tests/mesh_clean_reference.py against the code it replaces (meshproc.Mesh.split + max(area) + fix_normals) on a three-sphere mesh,
hand-made cases of the rules, and the command-line / pipeline surface. No GPU needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_mesh_clean.h")


def _functions(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_[a-z_0-9]+)\s*\(", src)) - {"rnb_ctx"})


# ------------------------------------------------------------------------------------------------------------------------ the C-ABI
def test_clean_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = _functions(HEADER)
    assert names == ["rnb_mesh_clean", "rnb_mesh_clean_abi_version", "rnb_mesh_clean_default_options", "rnb_mesh_clean_table_free"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.MESH_CLEAN_PROTOTYPES) == set(names)
    assert not set(_abi.MESH_CLEAN_PROTOTYPES) & (set(_abi.PROTOTYPES) | set(_abi.RENDER_PROTOTYPES) | set(_abi.MESH_PROTOTYPES))  # a table of its own
    # the other headers are as they were
    assert len(_functions(os.path.join(ROOT, "include", "rnb_neus2.h"))) == 54
    assert _functions(os.path.join(ROOT, "include", "rnb_mesh.h")) == ["rnb_extract_mesh", "rnb_mesh_abi_version", "rnb_mesh_default_options", "rnb_mesh_free"]
    fns = api.load_library()
    assert fns.abi_version() == _abi.ABI_VERSION == 5 and fns.mesh_abi_version() == _abi.MESH_ABI_VERSION == 1
    assert fns.mesh_clean_abi_version() == _abi.MESH_CLEAN_ABI_VERSION == 1
    opt = _abi.MeshCleanOptions()
    assert fns.mesh_clean_default_options(C.byref(opt)) == 0
    assert (opt.abi_version, opt.keep, opt.orient, list(opt.reserved)) == (1, _abi.MESH_KEEP_LARGEST, _abi.MESH_ORIENT_OUTWARD, [0] * 4)
    assert fns.mesh_clean_default_options(None) == _abi.ERR_INVALID
    assert hasattr(api.Context, "clean_mesh")


def test_clean_validates_its_arguments_without_a_device():
    """Null pointers, a wrong version, an unknown keep / orient, n_indices % 3 and null buffers are refused before the context or the device is touched: the context
    handed in here is not one (a block of zeros), and no device exists where this test runs."""
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    fns = api.load_library()
    fake = C.create_string_buffer(4096)
    ctx = C.cast(fake, C.c_void_p)

    def good():
        o = _abi.MeshCleanOptions()
        assert fns.mesh_clean_default_options(C.byref(o)) == 0
        return o

    def call(ctx_, m_in, o, m_out):
        return fns.mesh_clean(ctx_, None, m_in, o, m_out, None, None)

    src, dst = _abi.Mesh(), _abi.Mesh()
    dst.n_verts = 7
    assert call(None, C.byref(src), C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, None, C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), None, C.byref(dst)) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), C.byref(good()), None) == _abi.ERR_INVALID
    assert call(ctx, C.byref(src), C.byref(good()), C.byref(src)) == _abi.ERR_INVALID  # in place
    for field, value in (("abi_version", 2), ("abi_version", 0), ("keep", 2), ("orient", 2), ("orient", 0xFFFFFFFF)):
        o = good()
        setattr(o, field, value)
        dst.n_verts = 7
        assert call(ctx, C.byref(src), C.byref(o), C.byref(dst)) == _abi.ERR_INVALID, field
        assert dst.n_verts == 0 and not dst.verts  # zeroed on failure
        assert fns.last_error()
    src.n_indices = 4  # not a multiple of 3
    src.n_verts = 3
    assert call(ctx, C.byref(src), C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    src.n_indices = 3  # null buffers
    assert call(ctx, C.byref(src), C.byref(good()), C.byref(dst)) == _abi.ERR_INVALID
    tab = C.c_void_p(1)
    assert fns.mesh_clean(ctx, None, C.byref(src), C.byref(good()), C.byref(dst), C.byref(tab), None) == _abi.ERR_INVALID and not tab.value
    assert fns.mesh_clean_table_free(None, None) == _abi.ERR_INVALID
    assert fake.raw == b"\0" * 4096


def test_clean_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    src = tmp_path / "layout.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "rnb_mesh_clean.h"
int main(void) {
  printf("%zu %zu %zu %zu\\n", sizeof(rnb_mesh_clean_options), offsetof(rnb_mesh_clean_options, keep), offsetof(rnb_mesh_clean_options, orient), offsetof(rnb_mesh_clean_options, reserved));
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh_component), offsetof(rnb_mesh_component, n_vertices), offsetof(rnb_mesh_component, n_triangles), offsetof(rnb_mesh_component, kept),
         offsetof(rnb_mesh_component, area_q), offsetof(rnb_mesh_component, volume_q));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_mesh_clean_stats), offsetof(rnb_mesh_clean_stats, n_verts_in), offsetof(rnb_mesh_clean_stats, n_tris_out),
         offsetof(rnb_mesh_clean_stats, largest_label), offsetof(rnb_mesh_clean_stats, flatten_passes), offsetof(rnb_mesh_clean_stats, area_q_in), offsetof(rnb_mesh_clean_stats, area_q_out),
         offsetof(rnb_mesh_clean_stats, peak_workspace), offsetof(rnb_mesh_clean_stats, ms));
  printf("%d %d %d %d %d %d %d %u\\n", RNB_MESH_CLEAN_ABI_VERSION, RNB_MESH_KEEP_ALL, RNB_MESH_KEEP_LARGEST, RNB_MESH_ORIENT_NONE, RNB_MESH_ORIENT_OUTWARD, RNB_MESH_Q_SHIFT, RNB_MESH_Q_TERM_LOG2,
         RNB_MESH_NO_LABEL);
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    O, T, S = _abi.MeshCleanOptions, _abi.MeshComponent, _abi.MeshCleanStats
    assert out[:4] == [C.sizeof(O), O.keep.offset, O.orient.offset, O.reserved.offset]
    assert out[4:10] == [C.sizeof(T), T.n_vertices.offset, T.n_triangles.offset, T.kept.offset, T.area_q.offset, T.volume_q.offset]
    assert out[10:19] == [C.sizeof(S), S.n_verts_in.offset, S.n_tris_out.offset, S.largest_label.offset, S.flatten_passes.offset, S.area_q_in.offset, S.area_q_out.offset,
                          S.peak_workspace.offset, S.ms.offset]
    assert out[19:] == [_abi.MESH_CLEAN_ABI_VERSION, _abi.MESH_KEEP_ALL, _abi.MESH_KEEP_LARGEST, _abi.MESH_ORIENT_NONE, _abi.MESH_ORIENT_OUTWARD, _abi.MESH_Q_SHIFT, _abi.MESH_Q_TERM_LOG2,
                        _abi.MESH_NO_LABEL]
    # the numpy record of the table is the C record, and the reference's constants are the header's
    dt = np.dtype(_abi.MESH_COMPONENT_DTYPE)
    assert dt == mc.TABLE_DTYPE and dt.itemsize == C.sizeof(T) and [dt.fields[n][1] for n in dt.names] == [getattr(T, n).offset for n in dt.names]
    assert (mc.Q_SHIFT, mc.Q_TERM_LOG2, mc.NO_LABEL) == (_abi.MESH_Q_SHIFT, _abi.MESH_Q_TERM_LOG2, _abi.MESH_NO_LABEL)


# ------------------------------------------------------------------------------------------------------------------------ the statement against meshproc
def _oriented_keys(verts, tris):
    """Each triangle as its three positions, rotated so that the smallest corner comes first (the winding is kept): rows sorted."""
    p = np.asarray(verts, np.float64)[np.asarray(tris, np.int64).reshape(-1, 3)]  # [n, 3, 3]
    order = np.lexsort((p[:, :, 2], p[:, :, 1], p[:, :, 0]), axis=1)[:, 0] if len(p) else np.empty(0, np.int64)
    rolled = np.stack([p[np.arange(len(p)), (order + k) % 3] for k in range(3)], axis=1).reshape(-1, 9)
    return rolled[np.lexsort(rolled.T[::-1])]


def _meshproc_result(v, i):
    from rnb_neus2_amd import meshproc
    parts = meshproc.Mesh(v, i.reshape(-1, 3)).split()
    figures = sorted((len(m.faces), len(m.vertices), m.area, m.signed_volume) for m in parts)  # as they came in: fix_normals below changes the part it is applied to
    best = max(parts, key=lambda m: m.area)
    best.fix_normals()
    return parts, best, figures


@pytest.mark.parametrize("reverse", [None, 0, 1, 2])
def test_statement_equals_meshproc_on_three_spheres(reverse):
    v, i = mc.three_spheres(64, reverse)
    assert (len(v), len(i) // 3) == (3974, 7936)
    parts, best, figures = _meshproc_result(v, i)
    assert len(parts) == 3  # no sphere fell apart
    areas = sorted(p.area for p in parts)
    assert areas[2] / areas[1] >= 1.5 and areas[1] / areas[0] >= 1.5
    e = mc.expected(v, i, keep="largest", orient="outward")
    assert e["stats"]["n_components"] == 3 and e["stats"]["n_kept"] == 1
    # the table agrees with meshproc's double-precision figures to the fixed point's resolution times the number of terms
    tab = np.sort(e["table"], order="n_triangles")
    for (n_faces, n_vertices, area, volume), rec in zip(figures, tab):
        assert (n_faces, n_vertices) == (rec["n_triangles"], rec["n_vertices"])
        assert abs(area - rec["area_q"] / 2.0 ** mc.Q_SHIFT) < 1e-9 and abs(volume - rec["volume_q"] / 2.0 ** mc.Q_SHIFT) < 1e-9
    assert (e["table"]["volume_q"] < 0).sum() == (0 if reverse is None else 1)
    # same triangle set, same orientation
    assert len(best.vertices) == len(e["verts"]) and len(best.faces) == len(e["indices"]) // 3
    assert np.array_equal(_oriented_keys(best.vertices, best.faces), _oriented_keys(e["verts"], e["indices"]))
    if reverse == 0:  # the largest sphere was the reversed one: ORIENT_NONE leaves it inside out, OUTWARD turns every triangle
        n = mc.expected(v, i, keep="largest", orient="none")
        assert np.array_equal(n["indices"].reshape(-1, 3)[:, [0, 2, 1]], e["indices"].reshape(-1, 3))
    # KEEP_ALL keeps every triangle in order and turns only the reversed sphere
    a = mc.expected(v, i, keep="all", orient="outward")
    assert np.array_equal(a["verts"], v) and a["stats"]["n_kept"] == 3
    ref_v, ref_i = mc.three_spheres(64, None)
    assert np.array_equal(a["indices"], ref_i)


# ------------------------------------------------------------------------------------------------------------------------ hand-made cases of the rules
def _tri(*p):
    return np.array(p, np.float32)


def test_two_triangles_sharing_one_vertex_are_one_component():
    v = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0))
    e = mc.expected(v, [0, 1, 2, 0, 3, 4], keep="all", orient="none")
    assert e["stats"]["n_components"] == 1 and list(e["labels"]) == [0] * 5 and e["table"]["n_triangles"][0] == 2 and e["table"]["n_vertices"][0] == 5
    assert e["table"]["area_q"][0] == 1 << mc.Q_SHIFT  # two triangles of area 1/2, exact in fixed point


def test_unused_vertices_vanish_under_keep_all():
    v = _tri((9, 9, 9), (0, 0, 0), (1, 0, 0), (8, 8, 8), (0, 1, 0), (7, 7, 7))
    c = np.arange(18, dtype=np.float32).reshape(6, 3)
    e = mc.expected(v, [1, 2, 4], colors=c, normals=-c, keep="all", orient="none")
    assert list(e["labels"]) == [mc.NO_LABEL, 1, 1, mc.NO_LABEL, 1, mc.NO_LABEL]
    assert np.array_equal(e["verts"], v[[1, 2, 4]]) and list(e["indices"]) == [0, 1, 2]
    assert np.array_equal(e["colors"], c[[1, 2, 4]]) and np.array_equal(e["normals"], -c[[1, 2, 4]])
    assert e["stats"]["n_verts_out"] == 3 and e["stats"]["largest_label"] == 1 and list(e["table"]["label"]) == [1]


def test_equal_areas_keep_the_smaller_label():
    v = _tri((5, 0, 0), (6, 0, 0), (5, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 2, 2), (2.5, 2, 2), (2, 2.5, 2))
    e = mc.expected(v, [3, 4, 5, 6, 7, 8, 0, 1, 2], keep="largest", orient="none")
    assert list(e["table"]["label"]) == [0, 3, 6] and e["table"]["area_q"][0] == e["table"]["area_q"][1] > e["table"]["area_q"][2]
    assert list(e["table"]["kept"]) == [1, 0, 0] and e["stats"]["largest_label"] == 0
    assert np.array_equal(e["verts"], v[:3]) and list(e["indices"]) == [0, 1, 2] and list(e["tri_kept"]) == [False, False, True]


def test_empty_mesh_and_single_triangle():
    e = mc.expected(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
    assert e["verts"].shape == (0, 3) and e["indices"].shape == (0,) and len(e["table"]) == 0
    assert e["stats"]["n_components"] == 0 and e["stats"]["largest_label"] == mc.NO_LABEL and e["stats"]["area_q_in"] == 0
    e = mc.expected(np.zeros((4, 3), np.float32), np.zeros(0, np.uint32), keep="all")  # vertices, no triangles
    assert e["verts"].shape == (0, 3) and e["stats"]["n_verts_in"] == 4 and e["stats"]["n_verts_out"] == 0
    v = _tri((0, 0, 1), (1, 0, 1), (0, 1, 1))
    e = mc.expected(v, [0, 1, 2])
    assert e["stats"]["n_components"] == 1 and list(e["indices"]) == [0, 1, 2]  # volume 1/6 > 0: as it came
    assert e["table"]["area_q"][0] == 1 << (mc.Q_SHIFT - 1) and e["table"]["volume_q"][0] == int(np.trunc((1.0 / 6.0) * 2.0 ** mc.Q_SHIFT))
    with pytest.raises(ValueError):
        mc.expected(v, [0, 1, 3])
    with pytest.raises(ValueError):
        mc.expected(_tri((0, 0, 0), (np.inf, 0, 0), (0, 1, 0)), [0, 1, 2])


def test_open_strip_follows_the_sign_of_its_fixed_point_volume():
    n = 16
    x = np.arange(n + 1, dtype=np.float32)
    v = np.concatenate([np.stack([x, np.zeros_like(x), np.ones_like(x)], 1), np.stack([x, np.ones_like(x), np.ones_like(x)], 1)]).astype(np.float32)
    lo, hi = np.arange(n), np.arange(n) + n + 1
    t = np.concatenate([np.stack([lo, lo + 1, hi], 1), np.stack([lo + 1, hi + 1, hi], 1)]).astype(np.uint32)  # normal +z at z = 1: the terms are positive
    e = mc.expected(v, t.ravel())
    assert e["table"]["volume_q"][0] > 0 and np.array_equal(e["indices"].reshape(-1, 3), t)
    back = t[:, [0, 2, 1]]
    e = mc.expected(v, back.ravel())
    assert e["table"]["volume_q"][0] < 0 and np.array_equal(e["indices"].reshape(-1, 3), t)  # swapped back
    assert np.array_equal(mc.expected(v, back.ravel(), orient="none")["indices"].reshape(-1, 3), back)
    # the sums are integers: any order of the triangles gives the same table
    perm = np.random.default_rng(3).permutation(len(t))
    assert mc.expected(v, t[perm].ravel())["table"].tobytes() == mc.expected(v, t.ravel())["table"].tobytes()


# ------------------------------------------------------------------------------------------------------------------------ command line and pipeline
def test_mesh_program_lists_and_checks_the_new_flags():
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "--keep" in r.stdout and "--orient" in r.stdout
    base = ["--snapshot", "a", "--scene", "b", "--out", "c"]
    for bad in (["--keep", "biggest"], ["--orient", "inward"], ["--keep"], ["--keep", "largest", "--orient", "1"]):
        r = subprocess.run([exe] + base + bad, capture_output=True, text=True)
        assert r.returncode == 255, bad
    r = subprocess.run([exe] + base + ["--keep", "largest", "--orient", "outward"], capture_output=True, text=True)
    assert r.returncode == 1 and "does not exist" in r.stderr  # the flags parse; the snapshot is what is missing
    from rnb_neus2_amd import build
    assert HEADER in build.MESH_DEPS and HEADER in build.DEPS


def test_plan_device_postprocess_and_the_default_path(tmp_path, monkeypatch):
    from rnb_neus2_amd import pipeline
    argv = pipeline.plan_device_postprocess("/d/prepared_data", 10000, 1024, "/out/mesh.obj", "/b/build/mesh")
    assert argv == ["/b/build/mesh", "--snapshot", "/d/prepared_data/output/snapshot_10000.msgpack", "--scene", "/d/prepared_data", "--out", "/out/mesh.obj",
                    "--resolution", "1024", "--keep", "largest", "--orient", "outward"]
    assert pipeline.default_mesh_exe("/b/build/testbed") == "/b/build/mesh"
    # the default path still plans what the reference's recorded runs did
    with open(os.path.join(ROOT, "tests", "golden", "pipeline_argv.json")) as f:
        golden = {c["name"]: c for c in json.load(f)["cases"]}
    first, second = pipeline.plan_two_stage("<ROOT>/out/prepared_data", 10000, pipeline.common_flags(), resolution=1024, no_albedo=True)
    want = golden["full_default"]["testbed_argv"]
    assert [first.argv("tb", "<ROOT>/out/prepared_data")[1:], second.argv("tb", "<ROOT>/out/prepared_data")[1:]] == want
    # run_full_pipeline: off = postprocess_mesh and no mesh process; on = the planned process (with the snapshot that exists), then the output directory goes
    import run_pipeline
    from rnb_neus2_amd import dataloaders, prepare
    calls = []
    stub = tmp_path / "testbed"
    stub.write_text("#!/bin/sh\nexit 0\n")
    stub.chmod(0o755)
    mesh = tmp_path / "mesh"
    mesh.write_text("#!/bin/sh\necho \"$@\" > %s/mesh_argv.txt\necho clean: 3 components found\nexit 0\n" % tmp_path)
    mesh.chmod(0o755)
    monkeypatch.setattr(dataloaders, "load_data", lambda p, **kw: {"views": []})
    monkeypatch.setattr(prepare, "prepare_testbed_data", lambda data, out, logger, **kw: os.makedirs(os.path.join(out, "output"), exist_ok=True))
    monkeypatch.setattr(pipeline, "run_two_stage", lambda tb, d, steps, flags, **kw: [calls.append(["run_two_stage", steps, kw["resolution"]]),
                                                                                    open(os.path.join(d, "output", "snapshot_%d.msgpack" % steps), "wb").close()])
    monkeypatch.setattr(pipeline, "postprocess_mesh", lambda d, o, logger=None: calls.append(["postprocess_mesh", d, o]))
    out = str(tmp_path / "out")
    ns = run_pipeline.build_parser().parse_args(["-i", "in", "-t", str(stub), "-o", out, "--max-steps", "300", "--mesh-resolution", "128"])
    assert "device_postprocess" not in run_pipeline.pipeline_kwargs(ns)
    assert pipeline.run_full_pipeline(**run_pipeline.pipeline_kwargs(ns)) == os.path.join(out, "mesh.obj")
    assert calls == [["run_two_stage", 300, 128], ["postprocess_mesh", os.path.join(out, "prepared_data"), os.path.join(out, "mesh.obj")]]
    assert not (tmp_path / "mesh_argv.txt").exists()
    del calls[:]
    ns = run_pipeline.build_parser().parse_args(["-i", "in", "-t", str(stub), "-o", out, "--max-steps", "300", "--mesh-resolution", "128", "--device-postprocess"])
    kw = run_pipeline.pipeline_kwargs(ns)
    assert kw["device_postprocess"] is True and kw["mesh_exe"] is None  # build/mesh beside the testbed
    pipeline.run_full_pipeline(**kw)
    data_dir = os.path.join(out, "prepared_data")
    assert calls == [["run_two_stage", 300, 128]]
    assert (tmp_path / "mesh_argv.txt").read_text().split() == pipeline.plan_device_postprocess(data_dir, 300, 128, os.path.join(out, "mesh.obj"), str(mesh))[1:]
    assert not os.path.exists(os.path.join(data_dir, "output"))
    failing = tmp_path / "failing_mesh"
    failing.write_text("#!/bin/sh\nexit 1\n")
    failing.chmod(0o755)
    ns = run_pipeline.build_parser().parse_args(["-i", "in", "-t", str(stub), "-o", out, "--device-postprocess", "--mesh-exe", str(failing), "--max-steps", "300"])
    with pytest.raises(RuntimeError, match="Device post-processing failed with code 1"):
        pipeline.run_full_pipeline(**run_pipeline.pipeline_kwargs(ns))
    with pytest.raises(SystemExit):  # --mesh-exe means nothing without --device-postprocess: refused, not ignored
        run_pipeline.main(["-i", "in", "-t", str(stub), "-o", out, "--mesh-exe", str(mesh)])
