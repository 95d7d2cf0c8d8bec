"""The training march on camera placements the synthetic ring never produces (tests/march_geometry_cases.py; the CPU tier, test_march_geometry_cpu.py, holds every
case to what it claims): eyes inside the box and on its faces, box entries at t < 0.25 and t >= 8, binade boundaries inside the first round, exact-zero and 1e-37
direction components, grazing rays, the 1024-step diagonal, rays that miss the box -- over caller-written occupancy shapes from one cell to a dense box. Every march
form against the oracle's walk, bit for bit: COUNTERS[0, 2, 3], RAY_INDICES, NUMSTEPS, RAYS and every word of COORDS. There is no tolerance anywhere in the march part.

  form                                                                   selected by
  one wavefront per ray, k_march_count_wide<64, true>                    1000 rays (and 999: a workgroup with a wavefront that has no ray)
  the skipping march, k_march_count_skip                                 4200 rays (not a multiple of 64)
  its start-over path                                                    RNB_MARCH_SKIP=2
  k_march_count_wide<16, true>                                           RNB_MARCH_SKIP=0
  thread per ray with the bounding-box stop, k_march_count<true>         RNB_MARCH_NARROW_FROM=256
  ... without the stop / with the jump (k_march_count_bbox)              + RNB_MARCH_BBOX=0 / =2 (and =2 with RNB_MARCH_SKIP=2: no re-entry cell accepted)
  k_march_count_skip_narrow                                              + RNB_MARCH_SKIP_NARROW=1 (and with RNB_MARCH_SKIP=2)
  multi-cascade: k_march_count_wide<16, false> / k_march_count<false>    aabb_scale 2, 4: 1500 rays / RNB_MARCH_NARROW_FROM=256 with 4200 rays
"""
import numpy as np
import pytest

from tests import march_geometry_cases as mg
from tests.test_gpu_parity import _assert_samples_equal, _env, _half_close

pytestmark = pytest.mark.gpu

KW = dict(max_rays_per_batch=1 << 13, initial_rays_per_batch=512, apply_no_albedo=1)
NARROW = {"RNB_MARCH_NARROW_FROM": "256"}
# name -> (RNB_* read at rnb_create, ray counts marched in that context)
FORMS = {
    "default": (None, (1000, mg.N_RAYS)),  # 1000 rays: one wavefront per ray; 4200: the skipping march
    "skip_start_over": ({"RNB_MARCH_SKIP": "2"}, (mg.N_RAYS,)),
    "wide16": ({"RNB_MARCH_SKIP": "0"}, (mg.N_RAYS,)),
    "thread_bbox_stop": (NARROW, (mg.N_RAYS,)),
    "thread_plain": (dict(NARROW, RNB_MARCH_BBOX="0"), (mg.N_RAYS,)),
    "thread_bbox_jump": (dict(NARROW, RNB_MARCH_BBOX="2"), (mg.N_RAYS,)),
    "thread_bbox_jump_refused": (dict(NARROW, RNB_MARCH_BBOX="2", RNB_MARCH_SKIP="2"), (mg.N_RAYS,)),
    "skip_narrow": (dict(NARROW, RNB_MARCH_SKIP_NARROW="1"), (mg.N_RAYS,)),
    "skip_narrow_refused": (dict(NARROW, RNB_MARCH_SKIP_NARROW="1", RNB_MARCH_SKIP="2"), (mg.N_RAYS,)),
}
RUNS = [(n, total) for n in (1000, mg.N_RAYS) for total in (0, 12345)]
PAIRS = mg.PAIRS  # (mg.EXCLUDED_PAIRS: the pairs that cannot be declared view by view are not run)


class _Contexts:
    """One oracle context and one HIP context per march form, for each of the two batch sizes; made on first use, kept for the module, handed a family's views when the
    family changes (rnb_set_dataset replaces the dataset)."""

    def __init__(self):
        self.ctx, self.family = {}, {}

    def get(self, big, fam):
        import rnb_neus2_amd as rnb
        from tests import oracle_lib
        if big not in self.ctx:
            B = mg.batch_size(big)
            gpus = {}
            for name, (env, _) in FORMS.items():
                with _env(env):
                    gpus[name] = rnb.Context(target_batch_size=B, **KW)
            self.ctx[big] = (oracle_lib.context(target_batch_size=B, **KW), gpus)
        cpu, gpus = self.ctx[big]
        if self.family.get(big) != fam:
            data = mg.family(fam)
            for c in [cpu] + list(gpus.values()):
                c.set_dataset(*data)
            self.family[big] = fam
        return cpu, gpus, mg.batch_size(big) * 16

    def close(self):
        for cpu, gpus in self.ctx.values():
            for c in [cpu] + list(gpus.values()):
                c.close()
        self.ctx.clear()


@pytest.fixture(scope="module")
def contexts():
    c = _Contexts()
    yield c
    c.close()


def _compare(gpu, cpu, what):
    """_assert_samples_equal, which insists on samples; where the oracle marched none the counters say all there is to say."""
    cc = cpu.get("COUNTERS")
    if int(cc[2]) == 0:
        cg = gpu.get("COUNTERS")
        assert np.array_equal(cg[[0, 2, 3]], cc[[0, 2, 3]]) and cc[0] == 0 and cc[3] == 0, (what, cg, cc)
        return cc
    try:
        return _assert_samples_equal(gpu, cpu)
    except AssertionError as e:
        raise AssertionError("%s: %s\n%s" % (what, _describe_difference(gpu, cpu), e)) from None


def _describe_difference(gpu, cpu):
    """Which rays differ, and where along them (for the failure message only)."""
    cg, cc = gpu.get("COUNTERS"), cpu.get("COUNTERS")
    if not np.array_equal(cg[[0, 2, 3]], cc[[0, 2, 3]]):
        return "COUNTERS hip %s oracle %s" % (cg.tolist(), cc.tolist())
    kept, written = int(cc[2]), int(cc[3])
    ng, nc = gpu.get("NUMSTEPS", kept * 2).reshape(-1, 2), cpu.get("NUMSTEPS", kept * 2).reshape(-1, 2)
    if not np.array_equal(ng, nc):
        bad = np.flatnonzero((ng != nc).any(axis=1))
        return "NUMSTEPS differ on %d of %d rays, first %s: hip %s oracle %s" % (bad.size, kept, bad[:5].tolist(), ng[bad[:5]].tolist(), nc[bad[:5]].tolist())
    a, b = gpu.get("COORDS", written * 7).reshape(-1, 7), cpu.get("COORDS", written * 7).reshape(-1, 7)
    rows = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))
    if rows.size == 0:
        return "RAY_INDICES or RAYS differ"
    ray = np.searchsorted(nc[:, 1].astype(np.int64), rows, side="right") - 1
    rays = cpu.get("RAYS", kept * 6).reshape(-1, 6).astype(np.float64)
    d = rays[ray, 3:] / np.linalg.norm(rays[ray, 3:], axis=1, keepdims=True)
    t = ((b[rows, :3].astype(np.float64) - rays[ray, :3]) * d).sum(axis=1)
    return "COORDS differ in %d of %d samples on %d of %d rays; t of the differing samples %.6g .. %.6g; largest position difference %.3g; first rows %s" % (
        rows.size, written, np.unique(ray).size, kept, t.min(), t.max(), np.abs(a[rows, :3].astype(np.float64) - b[rows, :3]).max(), rows[:4].tolist())


def _march_and_compare(cpu, gpus, bf, max_samples, tag, runs=RUNS):
    """Every form against the oracle for every run; the forms that differ are reported together, each with the rays it differs on."""
    for c in [cpu] + list(gpus.values()):
        c.put("DENSITY_BITFIELD", bf)
    counters, failures = {}, []
    for n_rays, n_rays_total in runs:
        cpu.generate_training_samples(n_rays, n_rays_total, max_samples)  # the oracle marches once; every form is compared with that one result
        counters[(n_rays, n_rays_total)] = cpu.get("COUNTERS").copy()
        for name, (_, counts) in FORMS.items():
            if n_rays in counts:
                gpus[name].generate_training_samples(n_rays, n_rays_total, max_samples)
                try:
                    _compare(gpus[name], cpu, "%s, form %s, %d rays, n_rays_total %d" % (tag, name, n_rays, n_rays_total))
                except AssertionError as e:
                    failures.append(str(e).split("\n")[0])
    assert not failures, "%d form runs differ from the oracle:\n%s" % (len(failures), "\n".join(failures))
    return counters


@pytest.mark.parametrize("fam,shape", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_march_bit_exact(contexts, fam, shape):
    cpu, gpus, max_samples = contexts.get(shape in mg.BIG_SHAPES, fam)
    bf = mg.bitfield(shape, cpu.get("DENSITY_BITFIELD").size)
    counters = _march_and_compare(cpu, gpus, bf, max_samples, "%s / %s" % (fam, shape))
    cc = counters[(mg.N_RAYS, 0)]
    assert cc[0] == cc[3]                                                                                # no ray dropped
    assert (cc[2] > 0) == ("samples" in mg.view_classes(fam, shape, len(mg.FAMILIES[fam]())))


@pytest.mark.parametrize("fam", list(mg.FAMILIES))
def test_march_overflow_bit_exact(contexts, fam):
    """max_samples at 60 % of what the case marches: the rays the reference's rule drops are dropped, the rest written as before."""
    cpu, gpus, max_samples = contexts.get(False, fam)
    bf = mg.bitfield(mg.OVERFLOW_SHAPE, cpu.get("DENSITY_BITFIELD").size)
    cpu.put("DENSITY_BITFIELD", bf)
    for n_rays in (1000, mg.N_RAYS):
        cpu.generate_training_samples(n_rays, 0, max_samples)
        cap = mg.overflow_max_samples(int(cpu.get("COUNTERS")[0]))
        cc = _march_and_compare(cpu, gpus, bf, cap, "%s / overflow" % fam, runs=[(n_rays, 0)])[(n_rays, 0)]
        assert cc[0] > cap >= cc[3] > 0


@pytest.mark.parametrize("fam", list(mg.FAMILIES))
def test_march_empty_bitfield(contexts, fam):
    """Not one occupied cell: the stage call returns the same status on both sides (none raises) and the counters agree on nothing marched."""
    cpu, gpus, max_samples = contexts.get(False, fam)
    bf = np.zeros(cpu.get("DENSITY_BITFIELD").size, dtype=np.uint8)
    counters = _march_and_compare(cpu, gpus, bf, max_samples, "%s / empty" % fam)
    assert all(cc[0] == 0 and cc[2] == 0 and cc[3] == 0 for cc in counters.values())


def test_march_wavefront_per_ray_with_rayless_lanes(contexts):
    """999 rays in the one-wavefront-per-ray form: 250 workgroups of 4 rays, the last of which has a wavefront without a ray (the 1000 rays of the other tests fill every
    workgroup). Eyes inside the box and far outside it over the thin shell; every ray that has one is marched as the oracle marches it."""
    for fam in ("inside", "far"):
        cpu, gpus, max_samples = contexts.get(False, fam)
        gpu = gpus["default"]
        bf = mg.bitfield("thin_shell", cpu.get("DENSITY_BITFIELD").size)
        for c in (cpu, gpu):
            c.put("DENSITY_BITFIELD", bf)
        for n_rays_total in (0, 12345):
            for c in (cpu, gpu):
                c.generate_training_samples(999, n_rays_total, max_samples)
            cc = _compare(gpu, cpu, "%s / thin_shell, form default, 999 rays, n_rays_total %d" % (fam, n_rays_total))
            assert cc[2] > 0 and cc[0] == cc[3]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# multi-cascade scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", mg.MULTI_CASCADE_FAMILIES)
@pytest.mark.parametrize("aabb_scale", [2, 4])
def test_multi_cascade_march_bit_exact(aabb_scale, fam):
    """aabb_scale 2 and 4 (box [0.5 - s/2, 0.5 + s/2]^3, cone stepping): eyes inside the box, far outside it, and axis-parallel rays with exact-zero components, over the
    oracle's own start grid and over a thin shell in cascade 0 under coarser cascades all ones; 16 lanes per ray (1500 rays) and one thread per ray (4200)."""
    import rnb_neus2_amd as rnb
    from tests import oracle_lib
    B = mg.batch_size(True)
    kw = dict(KW, target_batch_size=B, aabb_scale=aabb_scale)
    cpu = oracle_lib.context(**kw)
    wide = rnb.Context(**kw)
    with _env(NARROW):
        thread = rnb.Context(**kw)
    try:
        data = mg.multi_cascade_family(fam, aabb_scale)
        for c in (cpu, wide, thread):
            c.set_dataset(*data)
        cpu.put("DENSITY_GRID", mg.own_density_grid(aabb_scale))
        cpu.update_density_bitfield()
        for c in (wide, thread):  # (_sync_occupancy of test_gpu_parity.py)
            c.put("DENSITY_GRID", cpu.get("DENSITY_GRID"))
            c.update_density_bitfield()
            assert np.array_equal(c.get("DENSITY_BITFIELD"), cpu.get("DENSITY_BITFIELD"))
        own = cpu.get("DENSITY_BITFIELD").copy()
        for tag, bf in (("own grid", own), ("shell", mg.multi_cascade_shell(own.size))):
            for c in (cpu, wide, thread):
                c.put("DENSITY_BITFIELD", bf)
            for gpu, n_rays in ((wide, 1500), (thread, mg.N_RAYS)):
                for n_rays_total in (0, 12345):
                    for c in (cpu, gpu):
                        c.generate_training_samples(n_rays, n_rays_total, B * 16)
                    cc = _compare(gpu, cpu, "aabb_scale %d / %s / %s, %d rays, n_rays_total %d" % (aabb_scale, fam, tag, n_rays, n_rays_total))
                    assert cc[3] > 0 and cc[0] == cc[3]
                    assert np.unique(cpu.get("COORDS", int(cc[3]) * 7).reshape(-1, 7)[:, 3]).size > 1  # dt takes more than one value: the cone stepping is live
    finally:
        for c in (cpu, wide, thread):
            c.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the loss kernels rebuild each ray from its index (k_ray_constants, pixel and target fetch)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [dict(), dict(apply_no_albedo=0)], ids=["no_albedo", "albedo"])
@pytest.mark.parametrize("fam", ["wide", "inside"])
def test_loss_over_unusual_views(fam, flags):
    """A non-square view with fx != fy and an off-centre principal point (wide), eyes inside the box (inside): one thin_shell case carried on through the oracle's network
    outputs into compute_loss; test_compute_loss's assertions with its tolerances."""
    import rnb_neus2_amd as rnb
    from tests import oracle_lib
    B = mg.batch_size(False)
    kw = dict(KW, target_batch_size=B)
    kw.update(flags)
    gpu, cpu = rnb.Context(**kw), oracle_lib.context(**kw)
    try:
        data = mg.family(fam)
        for c in (gpu, cpu):
            c.init_params()
            c.set_dataset(*data)
            c.set_training_step(0)
            c.put("DENSITY_BITFIELD", mg.bitfield("thin_shell", cpu.get("DENSITY_BITFIELD").size))
        n_rays, n_rays_total = (mg.N_RAYS if fam == "wide" else 1000), 0  # (wide: the shell takes 2 % of a view's rays)
        for c in (gpu, cpu):
            c.generate_training_samples(n_rays, n_rays_total)
        _assert_samples_equal(gpu, cpu)
        per_view = mg.Marched(cpu, n_rays, n_rays_total, len(data[0])).rays_with_samples_per_view()
        assert fam != "wide" or (data[0][2]["width"] != data[0][2]["height"] and per_view[2] >= mg.MIN_RAYS)  # the non-square view takes part
        written = int(cpu.get("COUNTERS")[3])
        cpu.forward_infer_staged(written)
        gpu.put("MLP_OUT", cpu.get("MLP_OUT", written * 16))
        for c in (gpu, cpu):
            c.compute_loss(n_rays, n_rays_total)
        cg, cc = gpu.get("COUNTERS"), cpu.get("COUNTERS")
        assert np.array_equal(cg, cc)
        kept = int(cc[2])
        assert kept >= mg.MIN_RAYS
        assert np.array_equal(gpu.get("NUMSTEPS", kept * 2), cpu.get("NUMSTEPS", kept * 2))
        assert np.array_equal(gpu.get("COORDS_COMPACTED").view(np.uint32), cpu.get("COORDS_COMPACTED").view(np.uint32))
        for name in ("LOSS", "EK_LOSS", "MASK_LOSS"):
            a, b = gpu.get(name, n_rays).astype(np.float64), cpu.get(name, n_rays).astype(np.float64)
            assert abs(a.sum() - b.sum()) <= 1e-4 * abs(b.sum()) + 1e-12, (name, a.sum(), b.sum())
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-9, err_msg=name)
        a = gpu.get("DLOSS_DOUT").astype(np.float32).reshape(B, 16)
        b = cpu.get("DLOSS_DOUT").astype(np.float32).reshape(B, 16)
        _half_close(a[:, :11], b[:, :11], rel=3e-3, abs_=1e-6, frac=0.998, name="dL/doutput")
    finally:
        gpu.close()
        cpu.close()
