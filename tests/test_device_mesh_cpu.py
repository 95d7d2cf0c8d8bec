"""DeviceMesh (rnb-neus2_amd/api.py) without a device: a recording stand-in for the library's function table shows which C calls the Python mesh API makes, in which order
and on which meshes, that everything handed out is released exactly once when a stage fails, and that a freed handle stops in Python. The sequences below were recorded
with this same stand-in under the api.py before DeviceMesh existed (five private helpers on Context, the chains written out in every caller); the calls that only fill an
options struct on the host (*_default_options) are left out of them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rnb_neus2_amd import _abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["bench_mesh.py", "bench_mesh_clean.py", "bench_mesh_simplify.py", "bench_mesh_distance.py", "bench_mesh_raster.py"]
DEVICE_CALLS = ("extract_mesh", "mesh_clean", "mesh_simplify", "mesh_distance", "mesh_raster", "device_malloc", "device_free", "memcpy", "mesh_free", "mesh_clean_table_free")
STAGES = DEVICE_CALLS[:5]
MESH_ARGS = dict(extract_mesh=((), 3), mesh_clean=((2,), 4), mesh_simplify=((2,), 4), mesh_distance=((2, 3), None), mesh_raster=((2,), None), mesh_free=((1,), None))


class FakeLibrary:
    """Every entry point returns 0 (`fail` names the one that returns ERR_INVALID instead). A call that returns a mesh fills it with made-up pointers and small counts (the
    attributes its input has, or the options ask for); device_malloc hands out made-up pointers; memcpy copies nothing (a download fills
    its destination with zeros). `log` holds (name, the `verts` pointers of the meshes
    passed, inputs then output); `buffers` and `meshes` hold what is handed out and not yet released, `errors` every release of something that is not."""

    def __init__(self, fail=None):
        self.fail, self.log, self.buffers, self.meshes, self.errors, self._next = fail, [], set(), set(), [], 0x1000

    def _ptr(self):
        self._next += 0x100
        return self._next

    def device_log(self):
        return [e for e in self.log if e[0] in DEVICE_CALLS]

    def last_error(self):
        return b"made to fail"

    def __getattr__(self, name):
        def call(*args):
            obj = lambda k: args[k]._obj  # the struct behind a byref()
            if name == self.fail:
                self.log.append((name, ()))
                return _abi.ERR_INVALID
            ins, out = MESH_ARGS.get(name, ((), None))
            seen = tuple(obj(k).verts for k in ins)
            if name == "create":
                obj(1).value = self._ptr()
            elif name == "device_malloc":
                obj(2).value = self._ptr()
                self.buffers.add(obj(2).value)
            elif name == "memcpy" and args[4] == _abi.D2H:
                C.memset(args[1], 0, args[3])  # a download reads zeros
            elif name == "device_free":
                self._release(self.buffers, args[1].value, name)
            elif name == "mesh_clean_table_free":
                self._release(self.buffers, args[1].value, name)
            elif name == "mesh_free":
                m = obj(1)
                if m.verts:
                    self._release(self.meshes, m.verts, name)
                C.memset(C.byref(m), 0, C.sizeof(_abi.Mesh))
            if out is not None:
                m = obj(out)
                src = obj(ins[0]) if ins else None
                m.verts, m.indices, m.n_indices = self._ptr(), self._ptr(), 9
                _abi.Mesh.n_verts.__set__(m, 5)  # (as C writes it: the handle's own n_verts is read-only)
                if src.colors if src is not None else obj(2).attributes & _abi.MESH_ATTR_COLORS:
                    m.colors = self._ptr()
                if src.normals if src is not None else obj(2).attributes & _abi.MESH_ATTR_NORMALS:
                    m.normals = self._ptr()
                self.meshes.add(m.verts)
                seen += (m.verts,)
                obj(len(args) - 1).ms = 0.5
            if name == "mesh_clean":
                obj(6).n_components = 2
                if args[5] is not None:
                    obj(5).value = self._ptr()
                    self.buffers.add(obj(5).value)
            if name == "mesh_distance":
                st = obj(7)
                st.sum_w, st.sum_wd, st.sum_wd2, st.n_samples, st.max_distance = 1 << 40, 1 << 38, 1 << 36, 12, 0.25
            self.log.append((name, seen))
            return 0
        return call

    def _release(self, held, ptr, name):
        if ptr in held:
            held.remove(ptr)
        else:
            self.errors.append((name, ptr))


def context(fail=None):
    fake = FakeLibrary(fail)
    return api.Context(cfg=_abi.Config(), fns=fake), fake


V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
I = np.uint32([0, 1, 2, 0, 2, 3])
B = (V + np.float32(0.1), I[:3])
COL = np.full((4, 3), 0.5, np.float32)
VIEW = dict(width=6, height=4, focal_length=(5.0, 5.0), principal_point=(0.5, 0.5), xform=np.eye(3, 4, dtype=np.float32))
NORMAL_MAP = np.zeros((4, 6, 4), np.uint16)

CALLS = {
    "extract_mesh": lambda c: c.extract_mesh(16, keep="largest", simplify=8, error=True, colors=True),
    "clean_mesh": lambda c: c.clean_mesh(V, I, colors=COL, table=True),
    "simplify_mesh": lambda c: c.simplify_mesh(V, I, cell=0.5, dims=2),
    "mesh_distance": lambda c: c.mesh_distance(V, I, *B, symmetric=True, per_vertex=True),
    "rasterize_mesh": lambda c: c.rasterize_mesh(V, I, VIEW, faces=True),
    "mesh_view_metrics": lambda c: c.mesh_view_metrics(V, I, [VIEW, VIEW], [NORMAL_MAP, NORMAL_MAP]),
}

UP = "device_malloc memcpy "  # one uploaded array


def _seq(text):
    """'mesh_clean:1200,1500 device_free*3' -> [("mesh_clean", (0x1200, 0x1500)), ("device_free", ())] * 3: the log entries of FakeLibrary, the meshes by their pointers in hex."""
    out = []
    for word in text.split():
        word, _, n = word.partition("*")
        name, _, ptrs = word.partition(":")
        out += [(name, tuple(int(x, 16) for x in ptrs.split(",")) if ptrs else ())] * int(n or 1)
    return out


# What the api.py before DeviceMesh did for CALLS (meshes: 0x1200 the first one made, then in the order they were made).
RECORDED = {
    "extract_mesh": _seq("extract_mesh:1200 mesh_clean:1200,1500 mesh_simplify:1500,1800 mesh_distance:1500,1800 mesh_distance:1800,1500 memcpy*3 "
                         "mesh_free:1200 mesh_free:1500 mesh_free:1800"),
    "clean_mesh": _seq(UP * 3 + "mesh_clean:1200,1500 device_free*3 memcpy*4 mesh_free:1500 mesh_clean_table_free"),
    "simplify_mesh": _seq(UP * 2 + "mesh_simplify:1200,1400 device_free*2 memcpy*2 mesh_free:1400"),
    "mesh_distance": _seq(UP * 4 + "device_malloc*2 mesh_distance:1200,1400 memcpy*2 device_free*2 device_malloc*2 mesh_distance:1400,1200 memcpy*2 device_free*2 device_free*4"),
    "rasterize_mesh": _seq(UP * 2 + "device_malloc*2 mesh_raster:1200 memcpy*2 device_free*2 device_free*2"),
    "mesh_view_metrics": _seq(UP * 2 + "device_malloc mesh_raster:1200 memcpy device_free device_malloc mesh_raster:1200 memcpy device_free device_free*2"),
}


def test_the_calls_and_their_order_are_those_of_the_api_before_the_handle():
    for name, call in CALLS.items():
        c, fake = context()
        call(c)
        assert fake.device_log() == RECORDED[name], name
        assert not fake.buffers and not fake.meshes and not fake.errors, name


@pytest.mark.parametrize("stage", STAGES)
def test_a_failing_stage_leaves_nothing_allocated(stage):
    """Each stage call made to return ERR_INVALID in every public call that reaches it: RnbError comes out, and every mesh and buffer handed out before is released once."""
    reached = 0
    for name, call in CALLS.items():
        c, fake = context(fail=stage)
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
    # the chain written out on the handle, the failing stage wherever it comes
    c, fake = context(fail=stage)
    with pytest.raises(api.RnbError):
        with c.extract_mesh_device(16, colors=True) as m, m.clean(table=True) as cm, cm.simplify((0, 0, 0), 0.25, 4) as sm, c.upload_mesh(V, I) as up:
            cm.table
            sm.distance_to(up, symmetric=True, per_vertex=True)
            sm.rasterize(VIEW, faces=True)
    assert not fake.buffers and not fake.meshes and not fake.errors


def _handle_calls(m, other):
    return [lambda: m.clean(), lambda: m.simplify((0, 0, 0), 0.5, 2), lambda: m.distance_to(other), lambda: other.distance_to(m), lambda: m.rasterize(VIEW), lambda: m.download(),
            lambda: m.__enter__()]


@pytest.mark.parametrize("made_by", ["upload_mesh", "extract_mesh_device", "clean"])
def test_a_freed_handle_stops_in_python(made_by):
    c, fake = context()
    other = c.upload_mesh(*B)
    if made_by == "clean":
        with c.extract_mesh_device(16) as e:
            m = e.clean(table=True)
    else:
        m = c.upload_mesh(V, I, COL) if made_by == "upload_mesh" else c.extract_mesh_device(16, normals=True)
    assert (m.n_verts, m.n_triangles, m.has_colors, m.has_normals) == ((4, 2, True, False) if made_by == "upload_mesh" else (5, 3, False, made_by == "extract_mesh_device"))
    assert (m.stats is None) == (made_by == "upload_mesh") and (m.table is not None) == (made_by == "clean")
    with pytest.raises(AttributeError):
        m.n_verts = 3
    for call in _handle_calls(m, other)[:-1]:  # alive: every one goes through
        r = call()
        if isinstance(r, api.DeviceMesh):
            r.free()
    m.free()
    n = len(fake.log)
    for call in _handle_calls(m, other):
        with pytest.raises(ValueError):
            call()
    m.free()  # a second free is nothing
    assert len(fake.log) == n and m.n_verts == 0
    other.free()
    assert not fake.buffers and not fake.meshes and not fake.errors


def test_free_after_the_context_closed_does_nothing():
    c, fake = context()
    up, ex = c.upload_mesh(V, I), c.extract_mesh_device(16)
    c.close()
    n = len(fake.log)
    up.free(), ex.free()
    del up, ex
    assert len(fake.log) == n


def test_upload_mesh_refuses_an_attribute_of_the_wrong_length():
    c, fake = context()
    with pytest.raises(ValueError, match="colors must have one row per vertex"):
        c.upload_mesh(V, I, colors=np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError, match="normals must have one row per vertex"):
        c.upload_mesh(V, I, normals=np.zeros((3, 3), np.float32))
    assert not fake.device_log()
    with c.upload_mesh(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)) as m:  # an empty array still gets a buffer
        assert (m.n_verts, m.n_triangles) == (0, 0) and m.verts and m.indices and fake.device_log() == _seq("device_malloc*2")
    assert not fake.buffers


def test_the_tools_and_the_api_hold_no_private_plumbing():
    for name in TOOLS:
        with open(os.path.join(ROOT, "tools", name)) as f:
            text = f.read()
        for needle in ("c.f.", "c._", "_abi.Mesh(", "C.byref"):
            assert needle not in text, (name, needle)
        assert "mesh_bench_common" in text
    with open(os.path.join(ROOT, "rnb-neus2_amd", "api.py")) as f:
        text = f.read()
    for gone in ("_device_mesh", "_download_mesh", "_mesh_distance_device", "_mesh_distance_symmetric", "_rasterize_device"):
        assert not re.search(r"def %s\b" % gone, text) and not hasattr(api.Context, gone), gone
    for name in ("extract_mesh", "clean_mesh", "simplify_grid", "simplify_mesh", "mesh_distance", "rasterize_mesh", "mesh_view_metrics", "sdf_lattice", "marching_cubes",
                 "upload_mesh", "extract_mesh_device", "_clean_options", "_simplify_options", "_distance_options", "_raster_options"):
        assert hasattr(api.Context, name), name
    import rnb_neus2_amd
    assert rnb_neus2_amd.DeviceMesh is api.DeviceMesh
