"""GPU test: a context gives back all the device memory it took. One cycle = create, one training step, one render, one mesh through extract -> clean ->
simplify -> rasterize (so that every lazily allocated workspace exists), close. Free device memory is read after each close; it must not fall from one cycle
to the next.

The bound is the parent's: with the hand-written list of .free() calls in rnb_destroy (before the device buffers released themselves) this test measured a
fall of 0 bytes after cycles 2, 3 and 4 in each of the four modes on an MI355X (profiles/split_driver.md), so the assertion is equality or better."""
import pytest

pytestmark = pytest.mark.gpu

SMOKE = dict(target_batch_size=1 << 13, max_rays_per_batch=1 << 13, initial_rays_per_batch=256)
MODES = {"fp32": dict(apply_no_albedo=1), "half": dict(apply_no_albedo=1, accumulate=1), "deterministic": dict(apply_no_albedo=1, deterministic=1),
         "albedo": dict(apply_no_albedo=0)}
PARENT_FALL_BYTES = 0  # per cycle, every mode (see the docstring)


def one_cycle(rnb, scene, view, kw):
    views, normals, albedos = scene
    with rnb.Context(**kw) as ctx:
        ctx.init_params()
        ctx.set_dataset(views, normals, albedos)
        ctx.train_step()
        ctx.render(view)
        with ctx.extract_mesh_device(res=32) as mesh, mesh.clean() as cleaned, cleaned.simplify(*ctx.simplify_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 16)) as simple:
            simple.rasterize(view)
            n_triangles = mesh.n_triangles
    return n_triangles


@pytest.mark.parametrize("mode", sorted(MODES))
def test_closing_a_context_returns_its_device_memory(mode):
    import torch
    import rnb_neus2_amd as rnb
    from rnb_neus2_amd import synthetic
    from rnb_neus2_amd.api import scaled_view

    scene = synthetic.make_scene(4, 96, 168.0)
    view = scaled_view(scene[0][0], 32.0 / 96.0)
    assert (view["width"], view["height"]) == (32, 32)
    free = []
    for _ in range(4):
        assert one_cycle(rnb, scene, view, dict(SMOKE, **MODES[mode])) > 0  # the stages had a mesh to work on
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    falls = [free[k] - free[k + 1] for k in (1, 2)]  # after the first cycle: it absorbs the runtime's own one-time allocations
    print("free bytes after each close (%s): %s; falls after cycles 2 -> 3 -> 4: %s" % (mode, free, falls))
    assert all(f <= PARENT_FALL_BYTES for f in falls), (free, falls)
