"""The mesh cleaner on the MI355X (include/rnb_mesh_clean.h) against the numpy statement of tests/mesh_clean_reference.py, bit for bit: vertices, indices, colours,
normals, the component table and the counts of the statistics, on uploaded meshes (three spheres, thousands of components under a random numbering, a strip of 2^20
triangles, strips laid out for the corners of the wavefront reduction), under permutations of the triangles, on invalid input, on the mesh of a model, beside training, and through build/mesh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_clean_reference as mc
from tests import mesh_sparse_reference as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)


@pytest.fixture(scope="module")
def ctx():
    import rnb_neus2_amd as rnb
    c = rnb.Context(**KW)
    c.init_params()
    yield c
    c.close()


def _check(c, v, i, colors=None, normals=None, keep="largest", orient="outward"):
    got = c.clean_mesh(v, i, colors=colors, normals=normals, keep=keep, orient=orient, table=True)
    want = mc.expected(v, i, colors=colors, normals=normals, keep=keep, orient=orient)
    mc.assert_equal_bits(got, want)
    assert got["stats"]["hook_passes"] == 1 and got["stats"]["flatten_passes"] == 1  # the bound the header states: one launch each, for every input
    return got, want


@pytest.mark.parametrize("reverse", [None, 0, 2])
def test_three_spheres(ctx, reverse):
    v, i = mc.three_spheres(64, reverse)
    rng = np.random.default_rng(5)
    col, nrm = rng.random((len(v), 3), dtype=np.float32), rng.standard_normal((len(v), 3)).astype(np.float32)
    for keep in ("all", "largest"):
        for orient in ("none", "outward"):
            got, want = _check(ctx, v, i, col, nrm, keep, orient)
            assert got["stats"]["n_components"] == 3 and got["stats"]["n_kept"] == (3 if keep == "all" else 1)
    got, _ = _check(ctx, v, i)  # without attributes
    assert "colors" not in got and "normals" not in got
    assert got["stats"]["n_tris_out"] == int(got["table"]["n_triangles"].max()) and got["stats"]["largest_label"] == 0


def _patches(n_comp, quads, rng):
    """n_comp flat square patches of quads x quads cells (2 triangles each) on a cubic arrangement in [0, 1)^3, each of its own size."""
    g = np.arange(quads + 1)
    gy, gx = np.meshgrid(g, g, indexing="ij")
    local = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1).astype(np.float64) / quads
    q = (gy[:-1, :-1] * (quads + 1) + gx[:-1, :-1]).ravel()
    tri = np.concatenate([np.stack([q, q + 1, q + quads + 1], 1), np.stack([q + 1, q + quads + 2, q + quads + 1], 1)])
    side = int(np.ceil(n_comp ** (1.0 / 3.0)))
    k = np.arange(n_comp)
    origin = np.stack([k % side, (k // side) % side, k // (side * side)], 1) / side + 0.05 / side
    size = (0.3 + 0.6 * rng.permutation(n_comp) / n_comp) / side
    v = (origin[:, None, :] + local[None, :, :] * size[:, None, None]).reshape(-1, 3).astype(np.float32)
    t = (tri[None, :, :] + (k * len(local))[:, None, None]).reshape(-1, 3)
    return v, t


def _renumber(v, t, rng):
    """The same mesh under a random numbering of its vertices."""
    new_of_old = rng.permutation(len(v))
    out = np.empty_like(v)
    out[new_of_old] = v
    return out, new_of_old[t]


def test_thousands_of_components_and_a_long_strip_under_random_numbering(ctx):
    rng = np.random.default_rng(11)
    v, t = _patches(4096, 12, rng)  # 4096 x 288 = 1 179 648 triangles, 692 224 vertices
    v, t = _renumber(v, t, rng)
    t = t[rng.permutation(len(t))]
    for keep in ("largest", "all"):
        got, want = _check(ctx, v, t.astype(np.uint32).ravel(), keep=keep)
        assert got["stats"]["n_components"] == 4096 and got["stats"]["n_tris_in"] == 1179648
    print("4096 patches: %.2f ms, peak workspace %.1f MB" % (got["stats"]["ms"], got["stats"]["peak_workspace"] / 1e6))
    # one strip of 2^20 triangles, numbered along its length, then under a random numbering
    n = 1 << 19
    x = np.arange(n + 1, dtype=np.float64) / n
    sv = np.concatenate([np.stack([x, np.zeros(n + 1), np.full(n + 1, 0.5)], 1), np.stack([x, np.full(n + 1, 2.0 ** -10), np.full(n + 1, 0.5)], 1)]).astype(np.float32)
    lo, hi = np.arange(n), np.arange(n) + n + 1
    st = np.concatenate([np.stack([lo, lo + 1, hi], 1), np.stack([lo + 1, hi + 1, hi], 1)])
    assert len(st) == 1 << 20
    for label, (pv, pt) in (("in order", (sv, st)), ("random numbering", _renumber(sv, st, rng))):
        got, want = _check(ctx, pv, pt.astype(np.uint32).ravel(), keep="all", orient="outward")
        assert got["stats"]["n_components"] == 1 and got["table"]["label"][0] == 0 and got["table"]["n_triangles"][0] == 1 << 20
        print("strip of 2^20 triangles, %s: %.2f ms" % (label, got["stats"]["ms"]))


def _strips(sizes):
    """Disjoint triangle strips of the given numbers of triangles, one component each, vertices and triangles numbered strip after strip: strip c has sizes[c] + 2
    vertices zigzagging along x at height z = 0.1 * (c + 1), its rows 0.01 * (c + 1) apart (every component its own area)."""
    v, t, base = [], [], 0
    for c, n in enumerate(sizes):
        k = np.arange(n + 2)
        v.append(np.stack([0.002 * k, 0.01 * (c + 1) * (k % 2), np.full(n + 2, 0.1 * (c + 1))], 1))
        t.append(base + np.stack([k[:-2], k[:-2] + 1, k[:-2] + 2], 1))
        base += n + 2
    return np.concatenate(v).astype(np.float32), np.concatenate(t)


@pytest.mark.parametrize("sizes", [(256,), (64, 64, 64, 64), (10, 20, 30, 4), (10, 20, 14, 12, 8), (257,)])
def test_wavefront_reduction_corners(ctx, sizes):
    """What one 256-thread workgroup of k_cl_sums<true> (one triangle per lane, in input order) can meet: one component in all four wavefronts (one set of atomics from
    LDS), a component per wavefront (four sets from LDS), exactly 4 components inside one wavefront (the last shuffle round), 5 inside one (the fifth falls back to one
    set per lane), and 257 triangles (a tail workgroup with a single live lane). Each as built and with the triangles shuffled inside every wavefront, so that the lanes
    of a group are not neighbours and the leader is not the first of its strip."""
    v, t = _strips(sizes)
    assert len(t) == sum(sizes)
    rng = np.random.default_rng(len(sizes))
    shuffled = np.concatenate([t[w:w + 64][rng.permutation(len(t[w:w + 64]))] for w in range(0, len(t), 64)])
    for tris in (t, shuffled):
        for keep in ("all", "largest"):
            got, _ = _check(ctx, v, tris.astype(np.uint32).ravel(), keep=keep)
            assert got["stats"]["n_components"] == len(sizes) and sorted(got["table"]["n_triangles"]) == sorted(sizes)


def test_permuted_triangles_and_repeated_calls(ctx):
    v, i = mc.three_spheres(64, 1)
    t = i.reshape(-1, 3)
    a = ctx.clean_mesh(v, i, keep="largest", orient="outward", table=True)
    b = ctx.clean_mesh(v, i, keep="largest", orient="outward", table=True)
    for key in ("verts", "indices", "table"):
        assert a[key].tobytes() == b[key].tobytes(), key  # two calls: the same bits
    perm = np.random.default_rng(2).permutation(len(t))
    for keep in ("largest", "all"):
        a = ctx.clean_mesh(v, i, keep=keep, table=True)
        p = ctx.clean_mesh(v, t[perm].ravel(), keep=keep, table=True)
        mc.assert_equal_bits(p, mc.expected(v, t[perm].ravel(), keep=keep))
        assert p["table"].tobytes() == a["table"].tobytes() and p["verts"].tobytes() == a["verts"].tobytes()  # same table, same kept set
        kept = mc.expected(v, i, keep=keep)["tri_kept"]
        pos = np.cumsum(kept) - 1  # input triangle -> its row in a's output
        assert np.array_equal(p["indices"].reshape(-1, 3), a["indices"].reshape(-1, 3)[pos[perm[kept[perm]]]])  # out permuted accordingly, nothing else


def test_invalid_input_fails_cleanly_and_the_context_stays_usable(ctx):
    from rnb_neus2_amd import _abi
    v, i = mc.three_spheres(64)
    f = ctx.f
    opt = ctx._clean_options("largest", "outward")
    pv = ctx.upload(v)
    try:
        for bad_value in (len(v), 0xFFFFFFFF):
            bad = i.copy()
            bad[len(bad) // 2] = bad_value
            pi = ctx.upload(bad)
            try:
                m, out, tab = _abi.Mesh(), _abi.Mesh(), C.c_void_p(1)
                m.verts, m.indices, m.n_verts, m.n_indices = pv, pi, len(v), len(bad)
                out.n_verts, out.verts = 5, 64
                assert f.mesh_clean(ctx._h, None, C.byref(m), C.byref(opt), C.byref(out), C.byref(tab), None) == _abi.ERR_INVALID
                assert bytes(out) == b"\0" * C.sizeof(out) and not tab.value
                assert b"out of range" in f.last_error()
                m.n_indices = len(bad) - 2  # not a multiple of 3
                out.n_indices = 9
                assert f.mesh_clean(ctx._h, None, C.byref(m), C.byref(opt), C.byref(out), None, None) == _abi.ERR_INVALID
                assert bytes(out) == b"\0" * C.sizeof(out)
            finally:
                ctx.device_free(pi)
            _check(ctx, v, i)  # a following valid call succeeds
    finally:
        ctx.device_free(pv)
    # a non-finite position used by a triangle fails the call; one no triangle uses does not matter
    w = np.concatenate([v, np.full((1, 3), np.nan, np.float32)])
    _check(ctx, w, i)
    w = v.copy()
    w[i[7]] = np.inf
    with pytest.raises(Exception, match="not finite"):
        ctx.clean_mesh(w, i)
    _check(ctx, v, i)
    got = ctx.clean_mesh(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), colors=np.zeros((5, 3), np.float32), table=True)  # empty input: an empty mesh
    mc.assert_equal_bits(got, mc.expected(np.zeros((5, 3), np.float32), np.zeros(0, np.uint32), colors=np.zeros((5, 3), np.float32)))


MODEL_STEPS = 60


def _two_sided_cells(verts, lo=1.0 / 3, hi=2.0 / 3):
    """Occupancy cells of cascade 0 (bool[128^3] in the bitfield's morton order) for the caller to write: the cells that hold a vertex of `verts` or touch such a cell,
    minus every cell whose centre lies between the fractions lo and hi of the mesh's extent along x. Culled through it, a surface that spans the extent loses a
    whole slab of bricks and falls into (at least) two parts. Returns the cells and the width of the slab."""
    from tests import render_reference as rr
    verts = np.asarray(verts, np.float64)
    cell = np.clip(np.floor(verts * 128).astype(np.int64), 0, 127)
    occ = np.zeros((128, 128, 128), bool)  # [z, y, x]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = np.clip(cell + (dx, dy, dz), 0, 127)
                occ[q[:, 2], q[:, 1], q[:, 0]] = True
    x0, x1 = float(verts[:, 0].min()), float(verts[:, 0].max())
    centre = (np.arange(128) + 0.5) / 128
    occ[:, :, (centre > x0 + (x1 - x0) * lo) & (centre < x0 + (x1 - x0) * hi)] = False
    g = np.arange(128, dtype=np.uint32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    flat = np.zeros(128 ** 3, bool)
    flat[rr.morton3d(x.ravel(), y.ravel(), z.ravel()).astype(np.int64)] = occ.ravel()
    return flat, (x1 - x0) * (hi - lo)


def _two_sided_bitfield(verts, n_bytes):
    flat, slab = _two_sided_cells(verts)
    bits = np.zeros(n_bytes, np.uint8)
    bits[: 128 ** 3 // 8] = np.packbits(flat.reshape(-1, 8)[:, ::-1], axis=1).ravel()
    return bits, slab


def _three_way(c, kw):
    """extract_mesh(keep, orient) == clean_mesh(extract_mesh()) == the numpy statement on the downloaded mesh; returns the statement."""
    raw = c.extract_mesh(**kw)
    assert "clean_stats" not in raw
    want = mc.expected(raw["verts"], raw["indices"], colors=raw["colors"], normals=raw["normals"])
    direct = c.extract_mesh(keep="largest", orient="outward", **kw)
    mc.assert_equal_bits(direct, want, table=False)
    assert direct["stats"]["n_bricks"] == raw["stats"]["n_bricks"] and direct["clean_stats"]["n_components"] == want["stats"]["n_components"]
    mc.assert_equal_bits(c.clean_mesh(raw["verts"], raw["indices"], raw["colors"], raw["normals"], table=True), want)
    for only, e in ((dict(keep="largest"), dict(keep="largest", orient="none")), (dict(orient="outward"), dict(keep="all", orient="outward"))):  # the one not given leaves its part alone
        mc.assert_equal_bits(c.extract_mesh(**only, **kw), mc.expected(raw["verts"], raw["indices"], colors=raw["colors"], normals=raw["normals"], **e), table=False)
    return raw, want


def test_on_the_mesh_of_a_model():
    """A model trained for MODEL_STEPS steps. Seen on the MI355X: without culling, at threshold 0, its 128^3 mesh is ONE component of 12 092 triangles -- the sphere
    initialisation leaves no floaters after 60 steps -- so that extraction alone would say little. The second extraction therefore culls through a caller-written
    occupancy bitfield (rnb_mesh.h allows one) that covers the surface except a slab across the middle third of its extent along x: at 256^3 with bricks of 8 points a
    brick, grown by one step, is 10 / 256 wide and starts every 8 / 256, so at least one whole layer of bricks fits into the slab (asserted: the slab is wider than
    18 / 256), every brick of that layer is dropped, and what is left on either side cannot be connected. The statement must find at least 2 components there
    (asserted first; seen on the MI355X: 38 116 of the 48 400 triangles are left, in 2 components). On both meshes: extract_mesh(keep="largest", orient="outward", colors, normals) == clean_mesh(extract_mesh(colors, normals)) == the numpy
    statement, bit for bit, and extract_mesh() without the new arguments returns the same buffers as before."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(16, 128, 1400.0 * 128 / 800.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        c.set_dataset(views, normals, albedos)
        for _ in range(MODEL_STEPS):
            c.train_step()
        kw = dict(res=128, cull="none", colors=True, normals=True)
        raw, want = _three_way(c, kw)
        print("the model's mesh without culling: %d triangles in %d components" % (len(raw["indices"]) // 3, want["stats"]["n_components"]))
        again = c.extract_mesh(**kw)
        for key in ("verts", "indices", "colors", "normals"):
            assert again[key].tobytes() == raw[key].tobytes()  # the default call is what it was
        whole = c.extract_mesh(res=256, cull="none")
        bits, slab = _two_sided_bitfield(whole["verts"], c.get("DENSITY_BITFIELD").size)
        assert slab > 18.0 / 256
        c.put("DENSITY_BITFIELD", bits)
        c.bitfield_changed()
        kw = dict(res=256, cull="occupancy", brick=8, colors=True, normals=True)
        parts = c.extract_mesh(**kw)
        n_comp = mc.expected(parts["verts"], parts["indices"])["stats"]["n_components"]
        print("culled through the two-sided bitfield: %d of %d triangles in %d components" % (len(parts["indices"]) // 3, len(whole["indices"]) // 3, n_comp))
        assert n_comp >= 2 and 0 < len(parts["indices"]) < len(whole["indices"])
        raw, want = _three_way(c, kw)
        assert want["stats"]["n_components"] == n_comp and 0 < want["stats"]["n_tris_out"] < len(raw["indices"]) // 3


def test_cleaning_leaves_training_untouched():
    """deterministic = 1: 40 steps, a clean_mesh and an extract_mesh(keep=...), 40 steps == 80 steps, bit for bit."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    views, normals, albedos = synthetic.make_scene(8, 96, 1400.0 * 96 / 800.0)
    v, i = mc.three_spheres(64)
    runs = []
    for interrupt in (True, False):
        c = rnb.Context(deterministic=1, **KW)
        c.init_params()
        c.set_dataset(views, normals, albedos)
        stats = []
        for s in range(80):
            if interrupt and s == 40:
                c.clean_mesh(v, i, table=True)
                c.extract_mesh(64, cull="none", keep="largest", colors=True)
            stats.append(c.train_step().as_dict())
        state = {k: c.get(k).copy() for k in ("PARAMS_FP32", "PARAMS_EMA", "ADAM_M", "ADAM_V", "DENSITY_GRID", "DENSITY_BITFIELD")}
        for st in stats:
            st.pop("prep_ms"), st.pop("step_ms")
        runs.append((state, stats))
        c.close()
    (sa, ta), (sb, tb) = runs
    assert ta == tb
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


def _obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if p and p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p and p[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in p[1:4]])
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.uint32).reshape(-1, 3)


def _write_snapshot_grid(path, cells):
    """Overwrites the occupancy grid a snapshot holds (the half values of `density_grid_binary`, a msgpack bin32 blob, morton order, cascade 0 first), in place: 1 in
    `cells`, 0 elsewhere. The bitfield the programs derive from it (grid > min(0.1, mean)) is then exactly `cells`."""
    raw = bytearray(open(path, "rb").read())
    key = b"density_grid_binary"
    p = raw.find(key)
    assert p >= 0 and raw.find(key, p + 1) < 0 and raw[p + len(key)] == 0xC6
    p += len(key) + 1
    n = int.from_bytes(raw[p:p + 4], "big")
    assert n % 2 == 0 and n // 2 >= cells.size
    grid = np.zeros(n // 2, np.float16)
    grid[:cells.size][cells] = 1.0
    raw[p + 4:p + 4 + n] = grid.tobytes()
    with open(path, "wb") as f:
        f.write(raw)


def _clean_line(stdout):
    """The numbers of build/mesh's `clean:` line: components found, kept, triangles before and after."""
    import re
    line = [l for l in stdout.splitlines() if l.startswith("clean:")]
    assert len(line) == 1, stdout
    print(line[0])
    m = re.match(r"clean: (\d+) components found, (\d+) kept, (\d+) -> (\d+) triangles", line[0])
    return tuple(int(x) for x in m.groups())


def test_build_mesh_with_the_flags_equals_postprocess_mesh(tmp_path):
    """`build/mesh --keep largest --orient outward` against pipeline.postprocess_mesh applied to the OBJ `build/mesh` writes without the flags: the same vertex and
    triangle counts and the same set of oriented triangles, positions as the decimals mesh::save_obj writes. So that there is something to remove whatever the model
    does, the snapshot's occupancy grid is overwritten with one that leaves out a slab of the surface between 50 % and 80 % of its extent along x (see
    test_on_the_mesh_of_a_model for why that separates it; the two parts differ clearly in area): asserted first, the un-flagged mesh has at least 2 components and the
    flagged one fewer triangles. Run twice: on the scene as written (`from_na`: faces as extracted, positive volume) and on a copy without `from_na`, whose un-flagged OBJ
    has every face reversed -- a component of negative volume for postprocess_mesh to turn, and the case in which --orient outward has to write the faces as they are."""
    import json
    import shutil
    from rnb_neus2_amd import pipeline, synthetic
    views, normals, albedos = synthetic.make_scene(12, 160, 280.0)
    scene = str(tmp_path / "scene")
    synthetic.write_scene(scene, views, normals, albedos)
    r = subprocess.run([os.path.join(ROOT, "build", "testbed"), "--scene", scene, "--maxiter", "100", "--no-gui", "--mask-weight", "1.0", "--no-albedo", "--save-snapshot"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    snap = str(tmp_path / "snapshot.msgpack")
    shutil.copy(os.path.join(scene, "output", "snapshot_100.msgpack"), snap)
    exe = os.path.join(ROOT, "build", "mesh")
    r = subprocess.run([exe, "--snapshot", snap, "--scene", scene, "--resolution", "256", "--cull", "none", "--out", str(tmp_path / "whole.obj")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "clean:" not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
    wv, wf = _obj(str(tmp_path / "whole.obj"))  # (the scene is written with scale 1 and no offset: the file's positions are the lattice's)
    cells, slab = _two_sided_cells(wv, 0.5, 0.8)
    assert slab > 18.0 / 256 and len(wf) > 1000
    _write_snapshot_grid(snap, cells)
    plain = str(tmp_path / "scene_plain")
    shutil.copytree(scene, plain, ignore=shutil.ignore_patterns("output"))
    with open(os.path.join(plain, "transform.json")) as f:
        meta = json.load(f)
    del meta["from_na"]
    with open(os.path.join(plain, "transform.json"), "w") as f:
        json.dump(meta, f)
    for name, sc in (("from_na", scene), ("plain", plain)):
        base = [exe, "--snapshot", snap, "--scene", sc, "--resolution", "256", "--brick", "8"]
        work = tmp_path / ("pp_" + name)
        os.makedirs(work / "output")
        r = subprocess.run(base + ["--out", str(work / "output" / "mesh_100.obj")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "clean:" not in r.stdout, r.stderr[-2000:] + r.stdout[-2000:]
        uv, uf = _obj(str(work / "output" / "mesh_100.obj"))
        un = mc.expected(uv, uf.ravel(), keep="all", orient="none")
        print("%s: the un-flagged mesh has %d triangles in %d components, signed volumes %s" % (name, len(uf), un["stats"]["n_components"], (un["table"]["volume_q"] / 2.0 ** mc.Q_SHIFT).round(5)))
        assert un["stats"]["n_components"] >= 2 and 0 < len(uf) < len(wf)
        assert (un["table"]["volume_q"][np.argmax(un["table"]["area_q"])] < 0) == (name == "plain")  # (fragments of a few triangles may have either sign)
        python_obj, device_obj = str(tmp_path / (name + "_python.obj")), str(tmp_path / (name + "_device.obj"))
        pipeline.postprocess_mesh(str(work), python_obj)
        r = subprocess.run(base + ["--out", device_obj, "--keep", "largest", "--orient", "outward"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        found, kept, tris_in, tris_out = _clean_line(r.stdout)
        assert found == un["stats"]["n_components"] and kept == 1 and tris_in == len(uf) and 0 < tris_out < tris_in
        (pv, pf), (dv, df) = _obj(python_obj), _obj(device_obj)
        assert len(df) == tris_out and (len(pv), len(pf)) == (len(dv), len(df))
        assert np.array_equal(ms.triangle_keys(pv, pf.ravel()), ms.triangle_keys(dv, df.ravel()))
        assert mc.expected(dv, df.ravel(), keep="all", orient="none")["table"]["volume_q"][0] > 0  # outward in the file, whatever the scene's flag
        # --keep alone selects and turns nothing: the kept triangles of the un-flagged file, wound as there
        r = subprocess.run(base + ["--out", device_obj, "--keep", "largest"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        kv, kf = _obj(device_obj)
        want = mc.expected(uv, uf.ravel(), keep="largest", orient="none")
        assert np.array_equal(ms.triangle_keys(kv, kf.ravel()), ms.triangle_keys(want["verts"], want["indices"]))
