"""CPU tier of `build/render` (rnb-neus2_amd/host/render_main.cpp): it builds from the tree through __graft_entry__.build(), lists its flags, and exits as the
testbed does -- 255 on a command-line error, 1 on a missing path -- before it touches a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "render")


@pytest.fixture(scope="module")
def render_exe():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(EXE)
    return EXE


def test_render_is_built_from_its_sources(render_exe):
    from rnb_neus2_amd import build
    assert build.RENDER_OUT == EXE and os.path.basename(build.RENDER_SRC) == "render_main.cpp"
    assert os.path.join(ROOT, "rnb-neus2_amd", "host", "snapshot.hpp") in build.RENDER_DEPS
    assert os.path.join(ROOT, "rnb-neus2_amd", "host", "snapshot.hpp") in build.TESTBED_DEPS
    assert os.path.getmtime(render_exe) >= max(os.path.getmtime(d) for d in build.RENDER_DEPS)


def test_render_help_lists_its_flags(render_exe):
    r = subprocess.run([render_exe, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--snapshot", "--scene", "--out", "--views", "--downscale", "--min-transmittance", "--help"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("argv", [["--bogus"], ["--scene", "x"], ["--snapshot"], ["--snapshot", "a", "--scene", "b", "--downscale", "0"],
                                  ["--snapshot", "a", "--scene", "b", "--min-transmittance", "x"], ["positional"]])
def test_render_command_line_errors_exit_255(render_exe, argv):
    r = subprocess.run([render_exe] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 255, (argv, r.stderr)


def test_render_missing_paths_exit_1(render_exe, tmp_path):
    scene = tmp_path / "scene"
    scene.mkdir()
    snap = tmp_path / "snap.msgpack"
    r = subprocess.run([render_exe, "--snapshot", str(snap), "--scene", str(scene)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Snapshot path" in r.stderr
    snap.write_bytes(b"\x80")
    r = subprocess.run([render_exe, "--snapshot", str(snap), "--scene", str(tmp_path / "missing")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Scene path" in r.stderr
