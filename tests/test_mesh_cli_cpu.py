"""CPU tier of `build/mesh` (rnb-neus2_amd/host/mesh_main.cpp): it builds from the tree through __graft_entry__.build(), lists its flags, and exits as the
testbed does -- 255 on a command-line error, 1 on a missing path -- before it touches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "mesh")


@pytest.fixture(scope="module")
def mesh_exe():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(EXE)
    return EXE


def test_mesh_is_built_from_its_sources(mesh_exe):
    from rnb_neus2_amd import build
    assert build.MESH_OUT == EXE and os.path.basename(build.MESH_SRC) == "mesh_main.cpp"
    for f in ("snapshot.hpp", "mesh.hpp"):
        assert os.path.join(ROOT, "rnb-neus2_amd", "host", f) in build.MESH_DEPS
    assert os.path.join(ROOT, "include", "rnb_mesh.h") in build.MESH_DEPS and os.path.join(ROOT, "include", "rnb_mesh.h") in build.DEPS
    assert os.path.getmtime(mesh_exe) >= max(os.path.getmtime(d) for d in build.MESH_DEPS)


def test_mesh_help_lists_its_flags(mesh_exe):
    r = subprocess.run([mesh_exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--snapshot", "--scene", "--out", "--resolution", "--cull", "--brick", "--normals", "--help"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("argv", [["--bogus"], ["--scene", "x"], ["--snapshot"], ["--snapshot", "a", "--scene", "b"], ["--snapshot", "a", "--scene", "b", "--out", "c", "--resolution", "0"],
                                  ["--snapshot", "a", "--scene", "b", "--out", "c", "--resolution", "5000"], ["--snapshot", "a", "--scene", "b", "--out", "c", "--cull", "maybe"],
                                  ["--snapshot", "a", "--scene", "b", "--out", "c", "--brick", "12"], ["--snapshot", "a", "--scene", "b", "--out", "c", "--normals", "x"], ["positional"]])
def test_mesh_command_line_errors_exit_255(mesh_exe, argv):
    r = subprocess.run([mesh_exe] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255, (argv, r.stderr)


def test_mesh_missing_paths_exit_1(mesh_exe, tmp_path):
    scene = tmp_path / "scene"
    scene.mkdir()
    snap = tmp_path / "snap.msgpack"
    out = str(tmp_path / "m.obj")
    r = subprocess.run([mesh_exe, "--snapshot", str(snap), "--scene", str(scene), "--out", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Snapshot path" in r.stderr
    snap.write_bytes(b"\x80")
    r = subprocess.run([mesh_exe, "--snapshot", str(snap), "--scene", str(tmp_path / "missing"), "--out", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Scene path" in r.stderr
