"""The corner-parallel hash-grid encode (RNB_PRIM_ENCODE_FORM of rnb_eval_primitives; csrc/common.cuh: level_issue_corners / level_collect_corners) gives the bits of the
sample-per-lane encode: the same table entries reach the same level_consume, only which lane fetched which entry differs.

Two contexts per case, set to the masks 0 and 7 (all three kernel groups: network evaluation, point query, training kernels), fed the same
parameters and inputs; raw bytes of rnb_forward_infer (all 16 halfs per sample), rnb_sdf / rnb_density and, after one deterministic-mode training step,
PARAMS_FP32. Shapes are the ones at which the lane mapping can go wrong: partial groups of 8 and partial tiles of 64, fewer than 14 live levels (a level
that is not live gathers from the last live one), positions on lattice planes, odd and even x cells of a hashed level, the last cell of a dense level."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(target_batch_size=1 << 13, max_rays_per_batch=1 << 13, initial_rays_per_batch=512, deterministic=1)
COUNTS = (1, 7, 8, 9, 63, 64, 65, 129)
STEPS = (0, 304)  # step 0: all 14 levels live; step 304 (below 660): fewer -- and, a multiple of 16, a step that updates the occupancy grid as step 0 does

HASHED_LEVEL = 8  # 2^19 entries for 231^3 cells


class _env:
    """The library reads its RNB_* knobs once, in rnb_create: set them around the construction of a context only."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        import os
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _contexts(env=None, **over):
    """(old form, new form) with the same randomised parameters: noise on every weight and O(0.05) hash-grid entries, so that every level carries signal."""
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    kw = dict(KW)
    kw.update(over)
    views, normals, albedos = synthetic.make_scene(4, 96, 168.0)
    pair = []
    for corners in (0, 7):
        with _env(env or {}):
            c = rnb.Context(**kw)
        assert c.set_encode_corners(corners) == 5  # the default: network evaluation and training kernels
        assert c.set_encode_corners(corners) == corners
        c.init_params()
        c.set_dataset(views, normals, albedos)
        pair.append(c)
    rng = np.random.default_rng(5)
    p = pair[0].get("PARAMS_FP32").copy()
    lay = pair[0].param_layout()
    p[lay["sdf"]:lay["grid"]] += rng.standard_normal(lay["grid"] - lay["sdf"]).astype(np.float32) * 0.03
    p[lay["grid"]:lay["variance"]] = (rng.random(lay["variance"] - lay["grid"], dtype=np.float32) - 0.5) * 0.1
    return pair[0], pair[1], p


def _positions(ctx):
    """129 positions: the special ones first, random ones behind them."""
    _, res, scale = ctx.grid_tables()
    below_one = np.nextafter(np.float32(1.0), np.float32(0.0))
    special = []
    for v in (0.0, 0.5, below_one):  # on lattice planes of every level (0), of some (0.5), and the last cell of every dense level in every axis (just below 1: index wrap)
        special += [(v, v, v), (v, 0.3, 0.7), (0.3, v, 0.7), (0.3, 0.7, v)]
    s = float(scale[HASHED_LEVEL])
    for k in (100, 101, 37, 42, int(res[HASHED_LEVEL]) - 2, int(res[HASHED_LEVEL]) - 1):  # x cell k of the hashed level: pos_fract's cell is floor(x * scale + 0.5)
        x = (k - 0.25) / s
        assert int(np.floor(np.float32(x) * np.float32(s) + np.float32(0.5))) == k
        special += [(x, 0.41, 0.59), (x, x, 0.2)]
    special = np.array(special, dtype=np.float32)
    rng = np.random.default_rng(11)
    rest = rng.random((129 - len(special), 3), dtype=np.float32)
    return np.concatenate([special, rest]).astype(np.float32)


def _rolled(a, n):
    """n rows, the special ones at other lanes for every n."""
    return np.ascontiguousarray(np.roll(a, n, axis=0)[:n])


@pytest.fixture(scope="module", params=[0, 1], ids=["fp32", "half"])
def evalpair(request):
    old, new, p = _contexts(accumulate=request.param, apply_no_albedo=0)
    for c in (old, new):
        c.set_params(p)
    yield old, new
    old.close()
    new.close()


@pytest.mark.parametrize("step", STEPS)
def test_forward_infer_bits(evalpair, step):
    old, new = evalpair
    xyz = _positions(old)
    rng = np.random.default_rng(step)
    coords = np.concatenate([xyz, rng.random((len(xyz), 4), dtype=np.float32)], axis=1)
    for c in (old, new):
        c.set_training_step(step)
    assert old.valid_level == new.valid_level and (old.valid_level >= 14) == (step == 0)  # compute_valid_level
    for n in COUNTS:
        cn = _rolled(coords, n)
        a, b = old.forward_infer(cn), new.forward_infer(cn)
        assert a.shape == b.shape == (n, 16)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), "forward_infer, %d samples, step %d" % (n, step)
    assert np.abs(a[:, 3].astype(np.float32)).max() > 0 and np.abs(a[:, 4:7].astype(np.float32)).max() > 0  # (the encode reaches the outputs)


@pytest.mark.parametrize("step", STEPS)
def test_point_query_bits(evalpair, step):
    old, new = evalpair
    xyz = _positions(old)
    for c in (old, new):
        c.set_training_step(step)
    for n in COUNTS:
        pn = _rolled(xyz, n)
        for inference in (False, True):
            a, b = old.sdf(pn, inference=inference), new.sdf(pn, inference=inference)
            assert a.shape == b.shape == (n,)
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), "sdf, %d points, step %d" % (n, step)
        a, b = old.density(pn), new.density(pn)
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)), "density, %d points, step %d" % (n, step)


# the six training kernels: SDF-only / albedo mode's second part; fp32 / half accumulators, the latter with the weight gradients in the kernel (RNB_DW_SLICED=0) or exported
@pytest.mark.parametrize("accumulate,no_albedo,sliced", [(0, 1, 1), (1, 1, 1), (1, 1, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)])
def test_training_step_bits(accumulate, no_albedo, sliced):
    old, new, p = _contexts(env=None if sliced else {"RNB_DW_SLICED": "0"}, accumulate=accumulate, apply_no_albedo=no_albedo)
    try:
        for step in STEPS:
            stats = []
            for c in (old, new):
                c.set_params(p)
                c.set_training_step(step)
                stats.append(c.train_step().as_dict())
            assert stats[0]["measured_batch_size"] == stats[1]["measured_batch_size"] > 0
            assert stats[0]["loss"] == stats[1]["loss"]
            a, b = old.get("PARAMS_FP32"), new.get("PARAMS_FP32")
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "PARAMS_FP32 after the step from %d" % step
            assert not np.array_equal(a.view(np.uint32), p.view(np.uint32))
    finally:
        old.close()
        new.close()
