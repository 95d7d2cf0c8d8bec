"""CPU tier of the march-geometry cases (tests/march_geometry_cases.py): the ORACLE alone marches every (family, shape) pair that test_gpu_march_geometry.py
sends to a GPU, and every pair is held to what it claims -- the reference's loop terminates and writes finite words, no ray is dropped except in the declared overflow
case, every view yields what it is declared to yield, and each family reaches the range of t / the directions / the empty stretches it exists for."""
import numpy as np
import pytest

from tests import march_geometry_cases as mg

KW = dict(max_rays_per_batch=1 << 13, initial_rays_per_batch=512, apply_no_albedo=1)
PAIRS = mg.PAIRS
_ctx = {}      # (family, big) -> oracle context
_marched = {}  # (family, shape) -> Marched of 4200 rays, n_rays_total 0: marched once, shared, never written


def _context(fam, big):
    from tests import oracle_lib
    if (fam, big) not in _ctx:
        for k in [k for k in _ctx if k[0] != fam]:  # (pairs come family by family)
            _ctx.pop(k).close()
        c = oracle_lib.context(target_batch_size=mg.batch_size(big), **KW)
        c.set_dataset(*mg.family(fam))
        _ctx[(fam, big)] = c
    return _ctx[(fam, big)]


def _march(fam, shape, n_rays_total=0, max_samples=None):
    big = shape in mg.BIG_SHAPES
    c = _context(fam, big)
    n_views = len(mg.FAMILIES[fam]())
    if n_rays_total == 0 and max_samples is None:
        if (fam, shape) not in _marched:
            _marched[(fam, shape)] = mg.march(c, mg.bitfield(shape, c.get("DENSITY_BITFIELD").size), mg.N_RAYS, 0, mg.batch_size(big) * 16, n_views)
        return _marched[(fam, shape)]
    return mg.march(c, mg.bitfield(shape, c.get("DENSITY_BITFIELD").size), mg.N_RAYS, n_rays_total, max_samples or mg.batch_size(big) * 16, n_views)


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    while _ctx:
        _ctx.popitem()[1].close()
    _marched.clear()


def test_the_cases_are_what_they_say():
    """The inputs themselves: image sizes, the maps' red halves, eyes where the families put them, the shapes' block counts on both sides of the LDS budget."""
    for fam in mg.FAMILIES:
        views, normals, _ = mg.family(fam)
        assert 3 <= len(views) <= 18
        for v, nm in zip(views, normals):
            assert 9 <= v["width"] <= 33 and 9 <= v["height"] <= 33
            assert not nm[:, : v["width"] // 2, 0].any() and (nm[:, v["width"] // 2:, 0] == 65535).all() and (nm[..., 3] == 65535).all()
    eyes = lambda fam: np.stack([np.asarray(v["xform"], dtype=np.float64)[:, 3] for v in mg.family(fam)[0]])
    assert np.all((eyes("inside") > 0) & (eyes("inside") < 1))
    out = np.maximum(np.maximum(-eyes("near_face"), eyes("near_face") - 1).max(axis=1), 0)
    assert np.allclose(np.sort(out), [1e-4, 0.01, 0.1, 0.24], rtol=1e-5)
    assert np.allclose(np.sort(np.linalg.norm(eyes("far") - 0.5, axis=1)), [3, 6, 9, 14, 20], rtol=1e-6)
    assert np.array_equal(np.sort(eyes("graze")[:5, 0]).astype(np.float32), np.float32([-1e-3, -1e-6, 0.0, 1e-6, 1e-3]))
    nonsquare = [v for v in mg.family("wide")[0] if v["width"] != v["height"]]
    assert len(nonsquare) == 1 and nonsquare[0]["focal_length"][0] != nonsquare[0]["focal_length"][1] and nonsquare[0]["principal_point"] == (0.31, 0.64)
    assert mg.n_blocks("blocks_checker") == 16384 and mg.n_blocks("thin_shell") <= 4096 and mg.n_blocks("dense") == 32 ** 3
    assert set(mg.EXCLUDED_PAIRS) <= {(f, s) for f in mg.FAMILIES for s in mg.SHAPES} and len(PAIRS) + len(mg.EXCLUDED_PAIRS) == len(mg.FAMILIES) * len(mg.SHAPES)
    assert set(mg.SKIP_PAIRS) <= set(PAIRS) and {s for _, s in mg.SKIP_PAIRS} >= {"thin_shell", "two_blobs_30", "two_blobs_60", "two_blobs_120", "one_cell_hi"}
    assert {f for f, _ in PAIRS} == set(mg.FAMILIES) and {s for _, s in PAIRS} == set(mg.SHAPES)  # every family and every shape runs
    for name, n in (("one_cell_mid", 1), ("one_cell_lo", 1), ("one_cell_hi", 1), ("sheets_x", 4 * 128 * 128), ("sheets_y", 4 * 128 * 128), ("dense", 128 ** 3)):
        assert int(np.unpackbits(mg.shape(name)).sum()) == n, name
    assert abs(int(np.count_nonzero(mg.shape("noise"))) - mg.N0 // 100) <= 1


@pytest.mark.parametrize("fam,shape", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_case_terminates_and_yields_what_it_declares(fam, shape):
    """Termination and finiteness, no dropped ray, and every view in its declared class -- with n_rays_total 0 (the run the classes and predicates are stated for);
    with n_rays_total 12345, the other run of the GPU tier, termination, finiteness and no dropped ray."""
    m = _march(fam, shape)
    assert np.isfinite(m.coords).all() and np.isfinite(m.rays).all()
    assert m.counters[0] == m.counters[3], "rays dropped: %s" % m.counters
    got = [mg.class_of(n) for n in m.rays_with_samples_per_view()]
    assert got == mg.view_classes(fam, shape, m.n_views), m.rays_with_samples_per_view().tolist()
    assert m.numsteps[:, 0].min(initial=1) >= 1 and m.numsteps[:, 0].max(initial=0) <= mg.MAX_STEPS
    m2 = _march(fam, shape, n_rays_total=12345)
    assert np.isfinite(m2.coords).all() and m2.counters[0] == m2.counters[3]


@pytest.mark.parametrize("fam", list(mg.FAMILIES))
def test_overflow_case_drops_rays(fam):
    """The one case per family that overflows on purpose: max_samples at 60 % of what the case marches."""
    m = _march(fam, mg.OVERFLOW_SHAPE)
    cap = mg.overflow_max_samples(int(m.counters[0]))
    o = _march(fam, mg.OVERFLOW_SHAPE, max_samples=cap)
    assert o.counters[0] == m.counters[0] > cap >= o.counters[3] > 0 and 0 < o.kept < m.kept
    assert np.isfinite(o.coords).all()


@pytest.mark.parametrize("fam", ["inside", "near_face"])
def test_near_field_first_samples_lie_below_a_quarter(fam):
    t = _march(fam, "dense").first_sample_t()
    assert (t < 0.25).mean() >= 0.9, (t < 0.25).mean()
    if fam == "inside":  # startt in [0, one step)
        assert t.max() < mg.STEP * 1.001


def test_binade_edges_enter_within_eight_steps_below_the_boundary():
    m = _march("binade_edges", "dense")
    t, view = m.first_sample_t(), m.view_of_ray()
    for k, T in enumerate((0.25, 0.5, 1.0, 2.0, 4.0)):
        tk = t[view == k]
        assert tk.size >= mg.MIN_RAYS and np.all((tk >= T - 8 * mg.STEP) & (tk < T)), (T, tk.min(), tk.max())


@pytest.mark.parametrize("shape", ["dense", "thin_shell", "noise"])
def test_far_first_samples_lie_beyond_eight(shape):
    t = _march("far", shape).first_sample_t()
    assert np.count_nonzero(t >= 8.0) >= 100 and t.max() < 32.0
    assert np.count_nonzero((t >= 2.0) & (t < 4.0)) >= mg.MIN_RAYS and np.count_nonzero((t >= 4.0) & (t < 8.0)) >= mg.MIN_RAYS


@pytest.mark.parametrize("shape", ["dense", "thin_shell", "cells_checker"])
def test_axis_rays_have_exact_zero_and_tiny_components(shape):
    m = _march("axis", shape)
    assert m.n_exact_zero_component() >= 100
    d = np.abs(m.rays[:, 3:])
    assert np.count_nonzero(((d > 0) & (d < 1e-12)).any(axis=1)) >= 100  # the 1e38 focal length: non-zero, below the bounding-box stop's 1e-12f


@pytest.mark.parametrize("shape", list(mg.POOLED))
def test_pooled_shapes_are_the_librarys_own_pyramid(shape):
    """The hand-made pyramids equal what update_density_bitfield builds from a grid with those cells (and only those) above the threshold."""
    c = _context("graze", True)
    occ = mg.POOLED[shape]()
    grid = np.zeros(128 ** 3, dtype=np.float32)
    bits = np.unpackbits(mg.shape(shape), bitorder="little")
    grid[bits.astype(bool)] = 1.0  # (the grid is in Morton order, as the bitfield)
    c.put("DENSITY_GRID", grid)
    c.update_density_bitfield()
    own = c.get("DENSITY_BITFIELD")
    assert occ.sum() == bits.sum() and np.array_equal(own, mg.bitfield(shape, own.size))
    assert own[mg.N0:2 * mg.N0].any()


@pytest.mark.parametrize("fam,shape,at_least", [("graze", "pooled_dense", 1000), ("graze", "pooled_planes_1", 1000)])
def test_positions_on_a_face_are_sampled_from_cascade_one(fam, shape, at_least):
    """The occupied side of the face case: the oracle emits samples AT positions with |p - 0.5| = 0.5 (looked up in cascade 1). graze: the view whose rays run in the low
    face x = 2^-27 (under pooled_planes_1 the cascade-0 cell of those positions is EMPTY: only cascade 1 can have said yes; under plain dense, whose cascade 1 is empty, that
    view has no sample at all). The inside cameras run over the same shapes in the GPU tier; their rare face positions are those that round to exactly 1, where cascade 1
    is empty, so the oracle has no such sample to show for them."""
    m = _march(fam, shape)
    n = int(np.count_nonzero(mg.on_face(m.coords[:, :3])))
    assert n >= at_least, n
    if fam == "graze":
        per = m.rays_with_samples_per_view()
        assert per[6] >= mg.MIN_RAYS and _march("graze", "dense").rays_with_samples_per_view()[6] == 0
        if shape == "pooled_planes_1":
            cells = np.floor(m.coords[mg.on_face(m.coords[:, :3]), :3].astype(np.float64) * 128).astype(int)
            assert np.count_nonzero(~mg.POOLED[shape]()[cells[:, 2], cells[:, 1], cells[:, 0]]) >= at_least


def test_diagonal_reaches_the_step_cap():
    m = _march("diagonal", "dense")
    assert m.n_full_length() >= 1


def test_graze_eyes_lie_in_and_beside_a_face_and_their_rays_run_along_it():
    m = _march("graze", "dense")
    assert np.count_nonzero(m.rays[:, 0] == 0.0) >= 100 and np.count_nonzero(np.abs(m.rays[:, 0]) == np.float32(1e-6)) >= 100
    first = m.coords[m.numsteps[:, 1].astype(np.int64), :3]
    assert np.count_nonzero(first.min(axis=1) < 1e-3) >= 100  # first samples within a tenth of a cell of a face


def test_wide_rays_miss_the_box_and_cut_corners():
    m = _march("wide", "dense")
    assert m.kept < 0.5 * mg.N_RAYS                      # most rays miss the box
    assert np.count_nonzero(m.numsteps[:, 0] <= 8) >= 3  # corners cut in a few steps (a chord under 8 steps is ~1 % of the rays that hit the box at all)


@pytest.mark.parametrize("fam,shape", mg.SKIP_PAIRS, ids=["%s-%s" % p for p in mg.SKIP_PAIRS])
def test_outside_cameras_see_long_empty_stretches(fam, shape):
    """Skips the kernel will take: at least 200 rays with an empty run of at least 150 steps (in front of the first sample or between two samples)."""
    first, gap = _march(fam, shape).longest_empty_run()
    assert np.count_nonzero(np.maximum(first, gap) >= 150) >= 200


def test_two_blobs_gaps_straddle_the_skip_threshold():
    """Just under the kernel's "skip only if n >= 32": at least 50 rays whose longest gap between samples is 20 .. 31 steps; the wider pairs of blobs leave 50 .. 130."""
    _, gap = _march("axis", "two_blobs_30").longest_empty_run()
    assert np.count_nonzero((gap >= 20) & (gap <= 31)) >= 50
    for shape, lo in (("two_blobs_60", 50), ("two_blobs_120", 110)):
        _, gap = _march("axis", shape).longest_empty_run()
        assert np.count_nonzero((gap >= lo) & (gap <= lo + 25)) >= 50, shape


# ---------------------------------------------------------------------------------------------------------------------------------------------
# multi-cascade cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", mg.MULTI_CASCADE_FAMILIES)
@pytest.mark.parametrize("aabb_scale", [2, 4])
def test_multi_cascade_case(aabb_scale, fam):
    from tests import oracle_lib
    views, normals, albedos = mg.multi_cascade_family(fam, aabb_scale)
    c = oracle_lib.context(target_batch_size=mg.batch_size(True), aabb_scale=aabb_scale, **KW)
    try:
        c.set_dataset(views, normals, albedos)
        c.put("DENSITY_GRID", mg.own_density_grid(aabb_scale))
        c.update_density_bitfield()
        own = c.get("DENSITY_BITFIELD").copy()
        assert own[:mg.N0].any() and own[mg.N0:2 * mg.N0].any()
        for bf in (own, mg.multi_cascade_shell(own.size)):
            for n_rays in (1500, mg.N_RAYS):
                m = mg.march(c, bf, n_rays, 0, mg.batch_size(True) * 16, len(views))
                assert np.isfinite(m.coords).all() and m.counters[0] == m.counters[3]
                assert np.unique(m.coords[:, 3]).size > 1  # dt varies: the cone stepping is live
                if n_rays == mg.N_RAYS:
                    assert m.rays_with_samples_per_view().min() >= mg.MIN_RAYS, m.rays_with_samples_per_view().tolist()
        eyes = np.stack([np.asarray(v["xform"], dtype=np.float64)[:, 3] for v in views])
        inside = np.all(np.abs(eyes - 0.5) < 0.5 * aabb_scale, axis=1)
        assert inside.all() if fam == "inside" else not inside.any()
    finally:
        c.close()
