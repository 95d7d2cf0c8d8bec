"""CPU tier of the inference tracer (include/rnb_render.h): the numpy statement of the tracer against the analytic maps of the synthetic scene (unit cube and a
larger box) and its march helpers against the reference's own fragments (tests/golden/int_fixtures.json), the C-ABI of the render header (exports, version,
defaults, struct layout against the Python declarations) and the view-scaling helper. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import render_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rnb_render.h")


def render_header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rnb_render[a-z_0-9]*)\s*\(", src)))


def _angles_and_iou(img, view, normal16):
    """Mean angle (degrees) between the rendered and the encoded camera-frame normals where both masks hold, and the IoU of the masks."""
    mask_in = normal16[..., 3] > 0
    mask_r = img[..., 6] > 0.5
    both = mask_in & mask_r
    R = np.asarray(view["xform"], np.float64).reshape(3, 4)[:, :3]
    m = normal16[..., :3].astype(np.float64) / 65535.0 * 2.0 - 1.0
    n_in = np.stack([m[..., 0], -m[..., 1], -m[..., 2]], axis=-1)
    n_r = img[..., 0:3].astype(np.float64) @ R  # R^T n: the camera frame
    a, b = n_in[both], n_r[both]
    cos = np.clip((a * b).sum(-1) / np.linalg.norm(a, axis=-1) / np.linalg.norm(b, axis=-1), -1.0, 1.0)
    return np.degrees(np.arccos(cos)), (both.sum() / max((mask_in | mask_r).sum(), 1))


@pytest.mark.parametrize("use_bitfield", [True, False])
def test_numpy_tracer_reproduces_the_analytic_sphere(use_bitfield):
    from rnb_neus2_amd import synthetic
    res = 96
    views, normals, _ = synthetic.make_scene(3, res, 1400.0 * res / 800.0)
    sdf = rr.sphere_sdf()
    bits = rr.bitfield_from_sdf(sdf) if use_bitfield else None
    for k in range(len(views)):
        img, n_net = rr.render(views[k], rr.analytic_net(sdf), bitfield=bits)
        assert img.shape == (res, res, rr.CHANNELS) and n_net > 0
        ang, iou = _angles_and_iou(img, views[k], normals[k])
        assert iou > 0.99, iou
        assert ang.mean() < 1.0, ang.mean()
        hit = img[..., 6] > 0.5
        # the logits (0, 1, -1) of analytic_net, not premultiplied; depth of a sphere of radius 0.25 seen from 1.5: within [1.25, 1.5]
        assert np.allclose(img[hit][:, 3:6], [0.5, 1 / (1 + np.exp(-1)), 1 / (1 + np.exp(1))], atol=2e-4)
        assert img[hit][:, 7].min() > 1.24 and img[hit][:, 7].max() < 1.5
        assert np.all(img[img[..., 6] == 0][:, 0:6] == 0)
        assert np.all(img[..., 7][img[..., 6] <= 0.2] == 0)


def test_numpy_tracer_without_early_stop_marches_to_the_box_exit():
    """min_transmittance 0: every sample of the march is composited, so n_samples is the march's own count; with the default the rays stop inside the sphere."""
    from rnb_neus2_amd import synthetic
    views, _, _ = synthetic.make_scene(1, 48, 1400.0 * 48 / 800.0)
    sdf = rr.sphere_sdf()
    bits = rr.bitfield_from_sdf(sdf)
    o, d = rr.camera_rays(views[0])
    _, _, cnt = rr.march(o, d, bits)
    full, _ = rr.render(views[0], rr.analytic_net(sdf), bitfield=bits, min_transmittance=0.0)
    assert np.array_equal(full[..., 8].ravel().astype(np.int64), cnt)
    early, _ = rr.render(views[0], rr.analytic_net(sdf), bitfield=bits)
    stopped = early[..., 6] == 1.0
    assert stopped.sum() > 0.9 * (early[..., 6] > 0.5).sum()
    assert np.all(early[..., 8][stopped] < full[..., 8][stopped])
    assert np.array_equal(early[~stopped], full[~stopped])


def _pcg32_draws(seed, n):
    """The first n outputs of pcg32{seed} (stream 1)."""
    M, mult, inc = (1 << 64) - 1, 0x5851f42d4c957f2d, 3
    state = ((inc + seed) * mult + inc) & M  # seed(): state 0, one step, + seed, one step
    out = []
    for _ in range(n):
        x, rot = (((state >> 18) ^ state) >> 27) & 0xffffffff, state >> 59
        out.append(((x >> rot) | (x << ((-rot) & 31))) & 0xffffffff)
        state = (state * mult + inc) & M
    return out


def test_numpy_march_helpers_reproduce_the_reference_fragments():
    """calc_dt, mip_from_pos, mip_from_dt, the cell index, the occupancy bit, the distance to the next voxel and advance_to_next_voxel of
    tests/render_reference.py over the `march` rows of tests/golden/int_fixtures.json (the reference's own functions, compiled for the host): bit for bit.
    Half of the rows are cone angle 0 in the unit cube, half cone angle 1 / 256 in the aabb_scale 4 box at t up to 4, recorded with the scene's max_cascade
    (0 and 2). The tracer clamps at CASCADES - 1 instead (render_reference.mip_from_dt); a row is used where that clamp gives the recorded cascade too --
    which is every row, since neither the positions (|p - 0.5| < 1.95) nor dt * 256 < 4 ask for more than cascade 2."""
    from tests import int_fixture_cases
    fx = int_fixture_cases.load()
    assert _pcg32_draws(1337, 6) + _pcg32_draws(42, 6) == fx["pcg32_next_uint_seeds_1337_42_0_deadbeefcafe_x6"][:12]
    a = np.array(fx["march_cone_maxcascade_p3_d3_t_dt_mipfrompos_mip_idx_occupied_dist_advance"], dtype=np.uint32).reshape(-1, 16)
    f = lambda c: a[:, c].view(np.float32)
    cone, maxc, t = f(0), a[:, 1].astype(np.int64), f(8)
    pos, d = np.stack([f(2), f(3), f(4)], axis=1), np.stack([f(5), f(6), f(7)], axis=1)
    idir = (np.float32(1) / d).astype(np.float32)
    dt = np.concatenate([rr.calc_dt(t[k:k + 1], cone[k]) for k in range(len(a))])
    assert dt.dtype == np.float32 and np.array_equal(dt.view(np.uint32), a[:, 9])
    assert np.array_equal(rr.mip_from_pos(pos, maxc), a[:, 10])
    mip = rr.mip_from_dt(dt, pos, maxc)
    assert np.array_equal(mip, a[:, 11])
    used = rr.mip_from_dt(dt, pos) == a[:, 11]  # the tracer's clamp
    assert used.sum() == len(a) == 128
    assert (cone[used] > 0).sum() == 64 and (a[used, 11] > 0).sum() >= 32 and (a[used, 11] > 1).sum() > 0
    assert (a[used, 11] > a[used, 10]).sum() > 0  # dt, not the position, chose the cascade
    idx = rr.cell_index(pos, mip)
    assert np.array_equal(idx, a[:, 12])
    # the fragments' bitfield: byte i = draw i of pcg32{5}, top 8 bits; generated as far as the rows look (cascades 0 .. 2)
    bits = np.zeros(rr.GRIDSIZE ** 3 // 8 * rr.CASCADES, np.uint8)
    n = int((idx // 8 + rr.GRIDSIZE ** 3 // 8 * mip).max()) + 1
    bits[:n] = np.array(_pcg32_draws(5, n), np.uint32) >> 24
    occ = rr.occupied(pos, bits, mip)
    assert np.array_equal(occ.astype(np.uint32), a[:, 13]) and 0 < occ.sum() < len(a)
    res = (rr.GRIDSIZE >> mip).astype(np.int64)
    assert np.array_equal(rr.distance_to_next_voxel(pos, d, idir, res).view(np.uint32), a[:, 14])
    adv = np.concatenate([rr.advance_to_next_voxel(t[k:k + 1], pos[k:k + 1], d[k:k + 1], idir[k:k + 1], res[k:k + 1], cone[k]) for k in range(len(a))])
    assert adv.dtype == np.float32 and np.array_equal(adv.view(np.uint32), a[:, 15])
    # under the cone angle a voxel is left in steps that differ from the constant step: the rows tell the two apart
    flat = np.concatenate([rr.advance_to_next_voxel(t[k:k + 1], pos[k:k + 1], d[k:k + 1], idir[k:k + 1], res[k:k + 1]) for k in range(len(a))])
    assert (flat.view(np.uint32) != a[:, 15]).sum() >= 32


@pytest.mark.parametrize("where,cam_radius,fx", [("outside", 2.5, 300.0), ("inside", 0.9, 100.0)])
def test_numpy_tracer_reproduces_the_analytic_sphere_in_a_larger_box(where, cam_radius, fx):
    """aabb_scale 2: the box [-0.5, 1.5]^3, cone angle 1 / 256, the bitfield's cascades 0 .. 2 around the sphere. From outside the box (2.5 from the centre) the
    sphere is reached at t ~ 2.25, where dt = t / 256 is five times the constant step and the march consults cascade 2; from inside it (0.9 from the centre, t ~ 0.65)
    the ray starts at near_distance and steps by the constant step in cascade 0. The same thresholds as in the unit cube."""
    from rnb_neus2_amd import synthetic
    res = 96
    views, normals, _ = synthetic.make_scene(2, res, fx, cam_radius=cam_radius)
    mn, mx, cone = rr.scene_box(2)
    assert (mn, mx, cone) == (-0.5, 1.5, 1.0 / 256.0)
    sdf = rr.sphere_sdf()
    bits = rr.bitfield_from_sdf(sdf, cascades=3)
    assert np.array_equal(bits[: len(bits) // rr.CASCADES], rr.bitfield_from_sdf(sdf)[: len(bits) // rr.CASCADES]) and bits[len(bits) // rr.CASCADES:].any()
    for k in range(len(views)):
        eye = np.asarray(views[k]["xform"], np.float64).reshape(3, 4)[:, 3]
        assert bool(np.all((eye > mn) & (eye < mx))) == (where == "inside")
        st = {}
        img, n_net = rr.render(views[k], rr.analytic_net(sdf, mn=mn, mx=mx), bitfield=bits, aabb_scale=2, stats=st)
        assert img.shape == (res, res, rr.CHANNELS) and n_net > 0
        ang, iou = _angles_and_iou(img, views[k], normals[k])
        print("%s view %d: IoU %.4f, normal angle mean %.3f deg, cascades consulted %s" % (where, k, iou, ang.mean(), st["mips"].tolist()))
        assert iou > 0.99, iou
        assert ang.mean() < 1.0, ang.mean()
        hit = img[..., 6] > 0.5
        assert np.allclose(img[hit][:, 3:6], [0.5, 1 / (1 + np.exp(-1)), 1 / (1 + np.exp(1))], atol=2e-4)
        assert img[hit][:, 7].min() > cam_radius - 0.26 and img[hit][:, 7].max() < cam_radius
        assert np.all(img[img[..., 6] == 0][:, 0:6] == 0)
        assert np.all(img[..., 7][img[..., 6] <= 0.2] == 0)
        if where == "outside":
            assert st["mips"][2] > 0 and np.unique(st["coords"][:, 3]).size > 1  # cascade 2 consulted, dt varies
        else:
            assert st["mips"][0] > 0 and st["mips"][1] > 0


def test_render_header_is_exported_by_the_hip_library():
    import __graft_entry__ as g
    g.build()
    from rnb_neus2_amd import api, _abi
    names = render_header_functions()
    assert names == ["rnb_render", "rnb_render_abi_version", "rnb_render_default_options"], names
    lib = C.CDLL(api.library_path())
    assert all(hasattr(lib, n) for n in names)
    assert set("rnb_" + k for k in _abi.RENDER_PROTOTYPES) == set(names)
    assert not set(_abi.RENDER_PROTOTYPES) & set(_abi.PROTOTYPES)  # a table of its own: rnb_neus2.h's set is unchanged
    fns = api.load_library()
    assert fns.render_abi_version() == _abi.RENDER_ABI_VERSION == 1
    opt = _abi.RenderOptions()
    assert fns.render_default_options(C.byref(opt)) == 0
    assert opt.abi_version == 1 and opt.use_inference_params == 1 and opt.use_occupancy == 1 and opt.max_rays_in_flight == 0
    assert abs(opt.min_transmittance - 0.01) < 1e-7 and abs(opt.near_distance - 0.2) < 1e-7
    assert fns.render_default_options(None) == _abi.ERR_INVALID
    # rnb_render validates its arguments before it touches a context or the device
    v = _abi.View()
    v.width, v.height = 4, 4
    v.focal_length[:] = [4.0, 4.0]
    assert fns.render(None, None, C.byref(v), C.byref(opt), None, None) == _abi.ERR_INVALID


def test_render_structs_match_the_header(tmp_path):
    from rnb_neus2_amd import _abi
    src = tmp_path / "layout.c"
    src.write_text("""#include <stdio.h>
#include <stddef.h>
#include "rnb_render.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(rnb_render_options), offsetof(rnb_render_options, max_rays_in_flight), offsetof(rnb_render_options, reserved),
         sizeof(rnb_render_stats), offsetof(rnb_render_stats, n_samples), offsetof(rnb_render_stats, ms));
  printf("%d %d\\n", RNB_RENDER_ABI_VERSION, RNB_RENDER_CHANNELS);
  return 0;
}
""")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    O, S = _abi.RenderOptions, _abi.RenderStats
    assert [int(x) for x in out[:6]] == [C.sizeof(O), O.max_rays_in_flight.offset, O.reserved.offset, C.sizeof(S), S.n_samples.offset, S.ms.offset]
    assert [int(x) for x in out[6:]] == [_abi.RENDER_ABI_VERSION, _abi.RENDER_CHANNELS]


def test_scaled_view_keeps_the_principal_point():
    from rnb_neus2_amd import api, synthetic
    views, _, _ = synthetic.make_scene(1, 800)
    v = dict(views[0], principal_point=(0.45, 0.55))
    q = api.scaled_view(v, 0.25)
    assert (q["width"], q["height"]) == (200, 200)
    assert np.allclose(q["focal_length"], [350.0, 350.0])
    assert tuple(q["principal_point"]) == (0.45, 0.55)
    assert np.array_equal(q["xform"], np.asarray(v["xform"], np.float32).reshape(3, 4))
    # the camera rays of matching pixel centres coincide (the same ray through the same normalised image position)
    o1, d1 = rr.camera_rays(v)
    o2, d2 = rr.camera_rays(q)
    # pixel (2, 2) of the quarter image = the centre of pixels (8..11, 8..11) of the full one, i.e. the corner point (10, 10) shared by four of them
    u = (np.array([10.0]) - 0.45 * 800) / 1400.0
    w = (np.array([10.0]) - 0.55 * 800) / 1400.0
    dd = np.array([u[0], w[0], 1.0]) @ np.asarray(v["xform"], np.float64).reshape(3, 4)[:, :3].T
    assert np.allclose(d2[2 * 200 + 2], dd / np.linalg.norm(dd), atol=1e-6)
    with pytest.raises(ValueError):
        api.scaled_view(v, 0)
