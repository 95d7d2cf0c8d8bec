"""The input checks rnb_mesh_clean and rnb_mesh_simplify share, on one tetrahedron (4 vertices, 4 triangles): an index equal to n_verts, an index of 0xFFFFFFFF,
n_indices = 11, in == out, n_verts = 0 with indices present. Each returns ERR_INVALID with its text in last_error and leaves *out zeroed (in == out: the call returns
before it touches the object, which is the input -- it is left as it was); the next valid call on the same context gives the bits of the numpy statements."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_simplify_reference as sr

pytestmark = pytest.mark.gpu

TETRA_V = np.array([(0.3, 0.4, 0.2), (1.6, 0.3, 0.4), (0.4, 1.7, 0.6), (1.3, 1.4, 1.8)], np.float32)  # one corner per cell of GRID
TETRA_T = np.array([0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2], np.uint32)
GRID = dict(origin=(0.0, 0.0, 0.0), cell=1.0, dims=2)
#        name: (index to overwrite, its value, n_verts, n_indices, in == out, text in last_error)
CASES = {"index_equals_n_verts": (7, 4, 4, 12, False, b"out of range"),
         "index_all_ones": (4, 0xFFFFFFFF, 4, 12, False, b"out of range"),
         "eleven_indices": (None, None, 4, 11, False, b"not a multiple of 3"),
         "in_is_out": (None, None, 4, 12, True, b"different objects"),
         "no_vertices": (None, None, 0, 12, False, b"out of range")}


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
    c.init_params()
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    return dict(clean=mc.expected(TETRA_V, TETRA_T), simplify=sr.expected(TETRA_V, TETRA_T, **GRID))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry", ["clean", "simplify"])
def test_invalid_mesh_is_refused_and_the_next_call_is_right(ctx, want, entry, case):
    from rnb_neus2_amd import _abi
    at, value, n_verts, n_indices, same, text = CASES[case]
    idx = TETRA_T.copy()
    if at is not None:
        idx[at] = value
    f = ctx.f
    pv, pi = ctx.upload(TETRA_V), ctx.upload(idx)
    try:
        m, out = _abi.Mesh(), _abi.Mesh()
        m.verts, m.indices, m.n_verts, m.n_indices = pv, pi, n_verts, n_indices
        out.n_verts, out.verts, out.n_indices = 5, 64, 9
        before = bytes(m)
        dst = m if same else out
        if entry == "clean":
            opt, tab = ctx._clean_options("largest", "outward"), C.c_void_p(1)
            rc = f.mesh_clean(ctx._h, None, C.byref(m), C.byref(opt), C.byref(dst), C.byref(tab), None)
            assert not tab.value
        else:
            opt = ctx._simplify_options(GRID["origin"], GRID["cell"], GRID["dims"], "quadric")
            rc = f.mesh_simplify(ctx._h, None, C.byref(m), C.byref(opt), C.byref(dst), None)
        err = f.last_error()
        assert rc == _abi.ERR_INVALID and text in err and ("rnb_mesh_" + entry).encode() in err, (rc, err)
        assert bytes(m) == before
        if not same:
            assert bytes(out) == b"\0" * C.sizeof(out)
    finally:
        ctx.device_free(pv)
        ctx.device_free(pi)
    if entry == "clean":
        got = ctx.clean_mesh(TETRA_V, TETRA_T, table=True)
        mc.assert_equal_bits(got, want["clean"])
        assert got["stats"]["n_tris_out"] == 4
    else:
        got = ctx.simplify_mesh(TETRA_V, TETRA_T, **GRID)
        sr.assert_equal_bits(got, want["simplify"])
        assert got["stats"]["n_tris_out"] == 4 and got["stats"]["n_clusters"] == 4
