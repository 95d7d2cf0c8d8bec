"""The inference tracer (include/rnb_render.h) away from the unit cube: aabb_scale 2 and 4 -- a box larger than [0, 1]^3, cone-angle stepping (dt grows with t),
coarser occupancy cascades chosen from dt -- and the options no other test reaches: cameras inside the box, near_distance, an off-centre principal point,
fx != fy, the training weights, apply_no_albedo, an unaligned output pointer, the 1024-sample cap. The statement is tests/render_reference.py.

No training: the weights are the initialisation plus seeded noise, the occupancy bitfield is written by hand (load_state). What the inputs must provide -- both kinds
of pixel, coarse cascades consulted, a varying dt -- is asserted next to each comparison."""
import functools

import numpy as np
import pytest

from tests import render_reference as rr

pytestmark = pytest.mark.gpu

KW = dict(target_batch_size=1 << 14, max_rays_per_batch=1 << 12, initial_rays_per_batch=1 << 10)
NB = rr.GRIDSIZE ** 3 // 8  # bytes of one cascade of the bitfield
# The variance parameter (output 7 of the network; inv_s = exp(10 variance)). The initialisation's 0.3 gives inv_s = 20: a sample deep inside the surface takes a
# weight of a few per cent, every ray through occupied cells ends half transparent and the weights along it are nearly equal (ties for the depth). 0.8, the value
# of render_reference.analytic_net, gives inv_s = 2981: a sample inside the surface is opaque, one outside transparent.
VARIANCE = 0.8
# For the test against the independent network only, the colour head's weights (three layers) are scaled by this after the noise. Unscaled, its albedo logits reach 5,
# and where 1 <= |x| < 2 one half-precision ulp of a logit (2^-10) moves logistic(x) by up to 1.9e-4: two correctly rounding networks could then not meet the 1e-4
# albedo cap of the parity tests. With 0.35^3 the logits stay below 0.25, where one ulp (2^-13) moves the albedo by 3e-5; the albedo map still varies by +-0.03, 300
# times the cap. Every other test keeps the unscaled head and its whole logit range: there both sides share the network.
RGB_SCALE = 0.35


def noisy_params(init, lay, seed, rgb_scale=1.0):
    """The initialisation + noise in the manner of test_gpu_parity._randomize, then the variance above (and a scale of the colour head, see RGB_SCALE)."""
    rng = np.random.default_rng(seed)
    p = init.copy()
    p[lay["sdf"]:lay["rgb"]] += rng.standard_normal(lay["rgb"] - lay["sdf"]).astype(np.float32) * 0.03
    p[lay["rgb"]:lay["grid"]] += rng.standard_normal(lay["grid"] - lay["rgb"]).astype(np.float32) * 0.03
    p[lay["rgb"]:lay["grid"]] *= np.float32(rgb_scale)
    p[lay["grid"]:lay["variance"]] = (rng.random(lay["variance"] - lay["grid"], dtype=np.float32) - 0.5) * 0.1
    p[lay["variance"]:lay["end"]] = VARIANCE
    return p


def _pack(occ_zyx):
    """bool [z, y, x] cells of one cascade -> its NB bitfield bytes (Morton order, bit i of a byte = cell 8 b + i)."""
    g = np.arange(rr.GRIDSIZE, dtype=np.uint32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    flat = np.zeros(rr.GRIDSIZE ** 3, bool)
    flat[rr.morton3d(x.ravel(), y.ravel(), z.ravel()).astype(np.int64)] = occ_zyx.ravel()
    return np.packbits(flat.reshape(-1, 8)[:, ::-1], axis=1).ravel()


def hand_bitfield():
    """Cascade 0: a spherical shell of radius 0.16 about the centre, 0.04 thick (inside the zero set of the noisy network, a blob of
    radius ~0.11 of the box: 0.22 at aabb_scale 2, 0.44 at 4). Cascades 1 and 2: 400 random non-zero bytes each (a byte is a 2 x 2 x 2 block of
    cells). Cascade 1 also: a slab five cells thick through the centre with the normal (4, 2, 1) / sqrt(21), which no axis and none of the cameras' rays is
    parallel to. Cascade 2 also: a thick shell, 0.5 .. 1.3 from the centre, around a cascade 1 that is all but empty there. The cameras' rays pass t = 2, where dt alone
    raises the cascade from 1 to 2, inside empty cascade-1 cells within that shell: the skip has to run to the end of the 1 / 64 cell before cascade 2 is asked, so a
    march that skips by a finer voxel grid than GRIDSIZE >> mip stops early, finds cascade 2 set and writes samples the true march jumps over. Cascades 3 .. 7 stay empty."""
    bits = np.zeros(NB * rr.CASCADES, np.uint8)
    bits[:NB] = rr.bitfield_from_sdf(rr.sphere_sdf(radius=0.16), band=0.02)[:NB]
    rng = np.random.default_rng(7)
    for m in (1, 2):
        bits[m * NB + rng.choice(NB, 400, replace=False)] = rng.integers(1, 256, 400).astype(np.uint8)
    g = np.arange(rr.GRIDSIZE, dtype=np.float64) + 0.5 - rr.GRIDSIZE / 2
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    bits[NB:2 * NB] |= _pack(np.abs(4 * x + 2 * y + z) / np.sqrt(21.0) < 2.5)
    r2 = np.sqrt(x * x + y * y + z * z) * 4.0 / rr.GRIDSIZE  # a cascade-2 cell is 4 / 128 wide
    bits[2 * NB:3 * NB] |= _pack((r2 > 0.5) & (r2 < 1.3))
    return bits


def load_state(c, bits=None, rgb_scale=1.0):
    """The same weights, EMA weights (another noise seed) and bitfield into a context, the library's or the CPU checker's."""
    c.init_params()
    init, lay = c.get("PARAMS_FP32"), c.param_layout()
    c.set_params(noisy_params(init, lay, 0, rgb_scale))
    c.put("PARAMS_EMA", noisy_params(init, lay, 1, rgb_scale))
    c.put("DENSITY_BITFIELD", hand_bitfield() if bits is None else bits)


def look(eye, target, w, h, fy, fx=None, principal_point=(0.5, 0.5)):
    from rnb_neus2_amd import synthetic
    m = synthetic.look_at_c2w(np.asarray(eye, np.float64), np.asarray(target, np.float64))
    return dict(width=w, height=h, focal_length=(fy if fx is None else fx, fy), principal_point=principal_point, xform=m.astype(np.float32))


CENTRE = np.array([0.5, 0.5, 0.5])


@functools.lru_cache(maxsize=None)
def _dirs():
    from rnb_neus2_amd import synthetic
    return synthetic.fibonacci_sphere(16)


def eye_at(radius, k=3):
    """Camera position k of the 16 on the synthetic scene's Fibonacci sphere, at `radius` from the centre."""
    return CENTRE + radius * _dirs()[k]


def inside_box(eye, aabb_scale):
    mn, mx, _ = rr.scene_box(aabb_scale)
    return bool(np.all((np.asarray(eye) > mn) & (np.asarray(eye) < mx)))


# The parity views (48 x 40, looking at the centre): name -> (aabb_scale, distance from the centre, fy, inside the box). Checked on the CPU with the numpy tracer
# around the CPU checker's network: 32 .. 53 % of the pixels opaque, 0.4 .. 1.6 % between 0.05 and 0.95, no pixel with tied weights.
PARITY = {"2-inside": (2, 0.9, 80.0, True), "2-outside": (2, 1.5, 100.0, False), "4-inside": (4, 1.5, 50.0, True)}


def parity_view(name, w=48, h=40):
    s, radius, fy, inside = PARITY[name]
    eye = eye_at(radius)
    assert inside_box(eye, s) == inside
    return s, look(eye, CENTRE, w, h, fy * w / 48.0)


@pytest.fixture(scope="module")
def states():
    """One context per aabb_scale with the hand-made state; no dataset, no training."""
    import rnb_neus2_amd as rnb
    bits = hand_bitfield()
    ctx = {}
    for s in (2, 4):
        ctx[s] = rnb.Context(aabb_scale=s, **KW)
        load_state(ctx[s], bits)
    yield ctx, bits
    for c in ctx.values():
        c.close()


def _stack(r):
    return np.concatenate([r["normal"], r["albedo"], r["opacity"][..., None], r["depth"][..., None], r["n_samples"][..., None].astype(np.float32)], axis=-1)


def _angle_deg(a, b):
    cos = np.clip((a * b).sum(-1) / np.maximum(np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1), 1e-30), -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def _numpy_counts(view, bits, aabb_scale, near):
    o, d = rr.camera_rays(view)
    mn, mx, cone = rr.scene_box(aabb_scale)
    st = {}
    _, coords, cnt = rr.march(o, d, bits, near, mn, mx, cone, st)
    return cnt.reshape(view["height"], view["width"]), coords, st["mips"]


@functools.lru_cache(maxsize=None)
def march_cases(s):
    """name -> (view, near_distance) of the march test at aabb_scale s."""
    r_in, r_out = {2: (0.9, 2.5), 4: (1.5, 4.0)}[s]  # 1.5: the synthetic scene's own cameras, inside the aabb_scale 4 box
    r_near = 0.9  # the cascade-0 shell begins 0.72 from this camera: near_distance 0.75 starts behind its front
    fy = {2: 80.0, 4: 50.0}[s]
    on_shell = CENTRE + 0.16 * np.array([2.0, -1.0, 2.0]) / 3.0  # in a cell of the cascade-0 shell; looks through the centre and out of the other side
    cases = {
        "outside": (look(eye_at(r_out), CENTRE, 48, 40, 60.0), 0.2),
        "inside-near-0": (look(eye_at(r_near), CENTRE, 48, 40, fy), 0.0),
        "inside-near-0.2": (look(eye_at(r_in), CENTRE, 48, 40, fy), 0.2),
        "inside-near-0.75": (look(eye_at(r_near), CENTRE, 48, 40, fy), 0.75),
        "in-occupied-cell": (look(on_shell, CENTRE, 48, 40, 40.0), 0.0),
        "principal-point": (look(eye_at(r_in), CENTRE, 48, 40, fy, principal_point=(0.37, 0.61)), 0.2),
        "fx-1.3-fy": (look(eye_at(r_in, 7), CENTRE, 48, 40, fy, fx=1.3 * fy), 0.2),
        "1x1": (look(eye_at(r_in, 5), CENTRE, 1, 1, 1.0), 0.2),
        "67x5": (look(eye_at(r_in, 11), CENTRE, 67, 5, 90.0), 0.2),
    }
    assert not inside_box(eye_at(r_out), s) and inside_box(eye_at(r_in), s) and inside_box(on_shell, s)
    return cases


MARCH_CASES = ["outside", "inside-near-0", "inside-near-0.2", "inside-near-0.75", "in-occupied-cell", "principal-point", "fx-1.3-fy", "1x1", "67x5"]


@pytest.mark.parametrize("case", MARCH_CASES)
@pytest.mark.parametrize("aabb_scale", [2, 4])
def test_march_is_bit_exact(states, aabb_scale, case):
    """min_transmittance 0 composites every sample the march wrote: n_samples of every pixel is the numpy march's count. The march is float32 in the same
    operation order on both sides -- the ray, the box, calc_dt, mip_from_dt, the cell, advance_to_next_voxel at GRIDSIZE >> mip -- so one differing step shows."""
    ctx, bits = states
    view, near = march_cases(aabb_scale)[case]
    cnt, coords, mips = _numpy_counts(view, bits, aabb_scale, near)
    r = ctx[aabb_scale].render(view, min_transmittance=0.0, near_distance=near)
    print("aabb_scale %d %s: %d samples, at most %d a ray, cascades consulted %s" % (aabb_scale, case, cnt.sum(), cnt.max(), mips.tolist()))
    assert r["n_samples"].shape == cnt.shape and r["stats"]["n_rays"] == cnt.size
    assert np.array_equal(r["n_samples"], cnt.astype(np.uint32))
    assert r["stats"]["n_samples"] == cnt.sum() and np.all(np.isfinite(_stack(r)))
    if case == "1x1":
        assert cnt.sum() > 0
        return
    # the inputs: differing counts, coarse cascades consulted, a varying dt. (From the shell no ray of the aabb_scale 2 box reaches t = 2 or leaves cascade 1.)
    assert np.unique(cnt).size > 2
    assert mips[1:].sum() >= 0.1 * mips.sum() and (mips[2:].sum() > 0 or (case, aabb_scale) == ("in-occupied-cell", 2))
    assert np.unique(coords[:, 3]).size > 1
    if case == "in-occupied-cell":
        eye = np.asarray(view["xform"], np.float32).reshape(3, 4)[None, :, 3]
        assert rr.occupied(eye, bits, rr.mip_from_dt(rr.calc_dt(np.float32([1e-6]), rr.scene_box(aabb_scale)[2]), eye))[0]
        assert np.all(cnt > 0)  # every ray starts with a sample
    if case == "inside-near-0.75":
        d0, _, _ = _numpy_counts(view, bits, aabb_scale, 0.2)
        assert (d0 != cnt).sum() > 0.1 * cnt.size  # the near distance decides the start


def test_march_without_occupancy_meets_the_sample_cap():
    """aabb_scale 1, occupancy off, near_distance 0, a camera just inside the corner (0, 0, 0) looking at (1, 1, 1): the diagonal is sqrt(3) = 1024 steps long, so the
    central rays end at the RNB_MAX_STEPS cap -- spread over several rounds, nmax = min(n, 1024 - nsamp) -- or just below it, and the others leave through a face."""
    import rnb_neus2_amd as rnb
    view = look([1e-5, 1e-5, 1e-5], [1.0, 1.0, 1.0], 9, 7, 150.0)
    o, d = rr.camera_rays(view)
    _, _, cnt = rr.march(o, d, None, 0.0)
    with rnb.Context(**KW) as c:
        c.init_params()
        r = c.render(view, min_transmittance=0.0, occupancy=False, near_distance=0.0)
    print("samples per ray: %d .. %d, %d rays at the cap" % (cnt.min(), cnt.max(), (cnt == rr.MAX_STEPS).sum()))  # 979 .. 1024, the central ray at the cap
    assert np.array_equal(r["n_samples"].ravel(), cnt.astype(np.uint32))
    assert r["n_samples"].max() <= rr.MAX_STEPS and cnt.max() >= rr.MAX_STEPS - 1 and cnt.min() < rr.MAX_STEPS - 1
    assert r["stats"]["rounds"] > 1


def test_march_on_the_models_own_grid():
    """The occupancy grid the library builds itself at step 0 (update_density_grid: every cascade of the aabb_scale 2 scene sampled, the cells no training camera
    sees cleared, the cascades above max-pooled) instead of the hand-made one."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    with rnb.Context(aabb_scale=2, **KW) as c:
        load_state(c)
        c.set_dataset(*synthetic.make_scene(4, 96, 168.0))
        c.set_training_step(0)
        c.update_density_grid()
        bits = c.get("DENSITY_BITFIELD")
        own = [int(np.unpackbits(bits[m * NB:(m + 1) * NB]).sum()) for m in range(rr.CASCADES)]
        print("cells set per cascade:", own)
        assert 0 < own[0] < rr.GRIDSIZE ** 3 and 0 < own[1] < rr.GRIDSIZE ** 3 and own[2] > 0
        for name, near in (("inside-near-0.2", 0.2), ("outside", 0.2)):
            view = march_cases(2)[name][0]
            cnt, coords, mips = _numpy_counts(view, bits, 2, near)
            r = c.render(view, min_transmittance=0.0, near_distance=near)
            assert np.array_equal(r["n_samples"], cnt.astype(np.uint32))
            assert cnt.sum() > 0 and mips[1:].sum() > 0 and np.unique(coords[:, 3]).size > 1


def _compare(g, ref, st, label):
    """The tolerances of test_gpu_render.test_parity_with_the_numpy_tracer. The depth is the max-weight sample's: it is compared where the reference's two largest
    weights differ by more than 1e-4 relative (a tie may change places); the excluded share of the pixels with a depth must stay below 1 %."""
    gi = _stack(g)
    op = ref[..., 6]
    assert (op > 0.5).mean() >= 0.2 and (op < 0.5).mean() >= 0.2, ((op > 0.5).mean(), (op < 0.5).mean())
    d_op = np.abs(gi[..., 6] - op)
    both = (gi[..., 6] > 0.5) & (op > 0.5)
    ang = _angle_deg(gi[both][:, 0:3], ref[both][:, 0:3])
    d_alb = np.abs(gi[both][:, 3:6] - ref[both][:, 3:6])
    dep = (gi[..., 6] > 0.2) & (op > 0.2)
    clear = ((st["wmax"] - st["w2"]) > 1e-4 * st["wmax"]).reshape(op.shape)
    excluded = (dep & ~clear).sum() / max(dep.sum(), 1)
    d_dep = np.abs(gi[dep & clear][:, 7] - ref[dep & clear][:, 7])
    print("%s: opacity |d| mean %.2e max %.2e; normal angle mean %.4f max %.4f deg; albedo |d| max %.2e; depth |d| median %.2e max %.2e (%.2f %% excluded); hit %d of %d, "
          "%d between 0.05 and 0.95" % (label, d_op.mean(), d_op.max(), ang.mean(), ang.max(), d_alb.max(), np.median(d_dep), d_dep.max(), 100 * excluded, both.sum(), both.size,
                                        ((op > 0.05) & (op < 0.95)).sum()))
    assert both.sum() > 0.2 * both.size
    assert d_op.mean() < 2e-5 and d_op.max() < 5e-3
    assert ang.mean() < 0.02 and ang.max() < 0.5
    assert d_alb.max() < 1e-4
    assert excluded < 0.01
    assert np.median(d_dep) < 1e-5 and d_dep.max() < 0.02
    assert np.array_equal(gi[..., 8] > 0, ref[..., 8] > 0)


@pytest.mark.parametrize("name", list(PARITY))
def test_tracer_around_the_librarys_own_network(states, name):
    """The numpy tracer with the library's forward_infer as its network: what is left to differ is the tracer's own arithmetic (the warps with mn != 0 and
    diag != 1, dt carried through warp_dt / unwarp_dt into the alpha, the composite, the depth un-warp) and the device-count path of the network launch. Both weight
    sets; the tolerances were set for two differently rounding networks, so here they are caps."""
    ctx, bits = states
    s, view = parity_view(name)
    c = ctx[s]
    chunk = KW["target_batch_size"] * 8
    imgs = {}
    for inference in (True, False):
        def net(coords):
            return np.concatenate([c.forward_infer(coords[k:k + chunk], inference=inference) for k in range(0, len(coords), chunk)])
        st = {}
        ref, _ = rr.render(view, net, bitfield=bits, aabb_scale=s, stats=st)
        assert st["mips"][1:].sum() >= 0.1 * st["mips"].sum() and st["mips"][2:].sum() > 0 and np.unique(st["coords"][:, 3]).size > 1
        g = c.render(view, inference=inference)
        _compare(g, ref, st, "%s inference=%d" % (name, inference))
        imgs[inference] = _stack(g)
    # observed on the first MI355X run, over the three views and both weight sets (701 .. 868 of 1920 pixels hit, 8 .. 31 between 0.05 and 0.95): opacity |d| mean
    # 4.3e-10 .. 1.7e-9, max 6.0e-8 .. 1.8e-7; normal angle mean <= 1e-4, max 0.028 deg (float32 acos of a cosine one ulp below 1); albedo |d| max 1.8e-7;
    # depth |d| 0 everywhere, no pixel excluded
    assert not np.array_equal(imgs[True][..., 0:8], imgs[False][..., 0:8])
    assert np.abs(imgs[True][..., 0:3] - imgs[False][..., 0:3]).max() > 1e-3  # two weight sets, two images


@pytest.mark.parametrize("name", ["2-inside", "4-inside"])
def test_parity_with_the_independent_network(states, name):
    """As test_gpu_render.test_parity_with_the_numpy_tracer, in the larger boxes: the CPU checker's forward_infer on the same weights, EMA and bitfield."""
    import rnb_neus2_amd as rnb
    from tests import oracle_lib
    _, bits = states
    s, view = parity_view(name, 24, 20)
    cpu, gpu = oracle_lib.context(aabb_scale=s, **KW), rnb.Context(aabb_scale=s, **KW)
    try:
        for c in (cpu, gpu):
            load_state(c, bits, RGB_SCALE)  # the one test with two networks: see RGB_SCALE
        st = {}
        ref, _ = rr.render(view, lambda coords: cpu.forward_infer(coords, inference=True), bitfield=bits, aabb_scale=s, stats=st)
        # observed on the first MI355X run (209 and 191 of 480 pixels hit): opacity |d| mean 5.6e-10 and 8.7e-10, max 8.9e-8 and 1.2e-7; normal angle 0;
        # albedo |d| max 3.8e-6 and 1.2e-7; depth |d| 0, no pixel excluded. (With the colour head unscaled the albedo differed by 3.0e-5 and 1.02e-4: one half ulp
        # of a logit near 0.9, see RGB_SCALE.)
        _compare(gpu.render(view), ref, st, "%s, independent network" % name)
    finally:
        cpu.close()
        gpu.close()


def test_no_albedo_gives_ones(states):
    """apply_no_albedo = 1: the albedo is sum(w * 1) / sum(w), the same sum in the same order twice: exactly 1 wherever anything was hit, 0 elsewhere."""
    import rnb_neus2_amd as rnb
    _, bits = states
    s, view = parity_view("2-inside")
    with rnb.Context(aabb_scale=s, apply_no_albedo=1, **KW) as c:
        load_state(c, bits)
        for mt in (0.01, 0.0):
            r = c.render(view, min_transmittance=mt)
            hit = r["opacity"] > 0
            print("min_transmittance %g: %d of %d pixels hit" % (mt, hit.sum(), hit.size))
            assert hit.sum() > 0.2 * hit.size and (~hit).sum() > 0  # both kinds of pixel
            assert np.all(r["albedo"][hit] == 1.0) and np.all(r["albedo"][~hit] == 0.0)
            assert ((r["opacity"] > 0) & (r["opacity"] < 1)).sum() > 0  # not only early stops: sums that are not 1 divide to 1 too


@pytest.mark.parametrize("w,h,tile", [(67, 5, 0), (160, 120, 4096)])
def test_unaligned_output_takes_the_scalar_write_path(states, w, h, tile):
    """An image 4 bytes past a 16-byte boundary: k_render_write<false>, one pixel a thread. The same bits as the aligned render, and nothing written around it."""
    ctx, _ = states
    c = ctx[2]
    view = look(eye_at(0.9), CENTRE, w, h, 80.0 * w / 48.0)
    n = w * h * rr.CHANNELS
    want = c.render(view, max_rays_in_flight=tile)
    assert want["stats"]["n_hit"] > 0 and (tile == 0 or w * h > 4 * tile)  # several tiles
    sentinel = np.float32(-12345.5)
    buf = c.upload(np.full(1 + n + 64, sentinel, np.float32))
    try:
        assert buf % 16 == 0
        st = c.render_into(view, buf + 4, max_rays_in_flight=tile)
        got = c.download(buf, 1 + n + 64, np.float32)
    finally:
        c.device_free(buf)
    assert got[0] == sentinel and np.all(got[1 + n:] == sentinel)
    img = got[1:1 + n].reshape(h, w, rr.CHANNELS)
    assert np.array_equal(img.view(np.uint32), _stack(want).view(np.uint32))
    assert st["n_hit"] == want["stats"]["n_hit"] and st["rounds"] == want["stats"]["rounds"]


def test_tilings_and_repeats_give_the_same_bits(states):
    ctx, _ = states
    s, view = parity_view("4-inside")
    a = ctx[s].render(view)
    imgs = [_stack(ctx[s].render(view, max_rays_in_flight=m)) for m in (64, 4096, 0)]
    rounds = [ctx[s].render(view, max_rays_in_flight=m)["stats"]["rounds"] for m in (64, 0)]
    assert rounds[0] > rounds[1]  # 30 tiles of 64 pixels: another round schedule
    for img in imgs:
        assert np.array_equal(img.view(np.uint32), _stack(a).view(np.uint32))
    assert a["stats"]["n_hit"] == (a["opacity"] > 0.001).sum() > 0
    assert a["stats"]["n_rays"] == 48 * 40
