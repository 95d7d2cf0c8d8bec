"""Host-side mirror of the reference's training interface over the C-ABI of include/rnb_neus2.h.

The reference drives this path through ``Testbed`` (src/testbed.cu:2776-2872, src/testbed_nerf.cu:3560-4138);
``Context`` keeps the same verbs (reset_network/init params, load dataset, train step, per-stage calls) and hands
everything to ``librnb_neus2_hip.so``. There is no CPU fallback: if the HIP library is missing, loading fails.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _abi
from ._abi import Config, View, StepStats, BUF, BUF_DTYPE

__all__ = ["Context", "DeviceMesh", "Config", "View", "StepStats", "load_library", "default_config", "library_path",
           "load_sdf_init_weights", "RnbError", "BUF", "scaled_view", "RENDER_CHANNELS"]

RENDER_CHANNELS = _abi.RENDER_CHANNELS

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_REPO_ROOT = os.path.dirname(_PKG_DIR)
_LIB_NAME = "librnb_neus2_hip.so"


class RnbError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("rnb error %d: %s" % (code, message))
        self.code = code


def library_path():
    return os.path.join(_PKG_DIR, _LIB_NAME)


_FUNCS = None


def load_library():
    """Load the HIP library. Fails loudly when it has not been built (no fallback path exists)."""
    global _FUNCS
    if _FUNCS is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError(
                "%s not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                "There is no CPU fallback for the hot path." % path)
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        _FUNCS = _abi.declare(lib, "rnb_", render=True, mesh=True, mesh_clean=True, mesh_simplify=True, mesh_distance=True, mesh_raster=True, mesh_texture=True,
                              mesh_visibility=True, mesh_project=True, mesh_draw=True, mesh_topology=True, mesh_holes=True, mesh_intersect=True, mesh_smooth=True, mesh_snap=True)
        if _FUNCS.abi_version() != _abi.ABI_VERSION:
            raise RuntimeError("ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.render_abi_version() != _abi.RENDER_ABI_VERSION:
            raise RuntimeError("render ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_abi_version() != _abi.MESH_ABI_VERSION:
            raise RuntimeError("mesh ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_clean_abi_version() != _abi.MESH_CLEAN_ABI_VERSION:
            raise RuntimeError("mesh-clean ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_simplify_abi_version() != _abi.MESH_SIMPLIFY_ABI_VERSION:
            raise RuntimeError("mesh-simplify ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_distance_abi_version() != _abi.MESH_DISTANCE_ABI_VERSION:
            raise RuntimeError("mesh-distance ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_raster_abi_version() != _abi.MESH_RASTER_ABI_VERSION:
            raise RuntimeError("mesh-raster ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_texture_abi_version() != _abi.MESH_TEXTURE_ABI_VERSION:
            raise RuntimeError("mesh-texture ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_visibility_abi_version() != _abi.MESH_VISIBILITY_ABI_VERSION:
            raise RuntimeError("mesh-visibility ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_project_abi_version() != _abi.MESH_PROJECT_ABI_VERSION:
            raise RuntimeError("mesh-project ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_draw_abi_version() != _abi.MESH_DRAW_ABI_VERSION:
            raise RuntimeError("mesh-draw ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_topology_abi_version() != _abi.MESH_TOPOLOGY_ABI_VERSION:
            raise RuntimeError("mesh-topology ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_holes_abi_version() != _abi.MESH_HOLES_ABI_VERSION:
            raise RuntimeError("mesh-holes ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_intersect_abi_version() != _abi.MESH_INTERSECT_ABI_VERSION:
            raise RuntimeError("mesh-intersect ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_smooth_abi_version() != _abi.MESH_SMOOTH_ABI_VERSION:
            raise RuntimeError("mesh-smooth ABI version mismatch between %s and the Python host side" % path)
        if _FUNCS.mesh_snap_abi_version() != _abi.MESH_SNAP_ABI_VERSION:
            raise RuntimeError("mesh-snap ABI version mismatch between %s and the Python host side" % path)
    return _FUNCS


def default_config(fns=None, **overrides):
    fns = fns or load_library()
    cfg = Config()
    rc = fns.default_config(C.byref(cfg))
    if rc != 0:
        raise RnbError(rc, fns.last_error().decode())
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError("rnb_config has no field %r" % k)
        setattr(cfg, k, v)
    return cfg


def load_sdf_init_weights(path=None):
    """The sphere-SDF initialisation of the density MLP (nerf_network.h:585-623)."""
    path = path or os.path.join(_REPO_ROOT, "utils", "mlp_weights_hidden_layer_num_1_hidden_size_32.txt")
    w = np.loadtxt(path, dtype=np.float64).astype(np.float32).ravel()
    if w.size != _abi.N_SDF_MLP_PARAMS:
        raise ValueError("expected %d SDF-MLP weights in %s, found %d" % (_abi.N_SDF_MLP_PARAMS, path, w.size))
    return np.ascontiguousarray(w)


def _stream_handle(stream):
    if stream is None:
        return None
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(getattr(stream, "cuda_stream"))  # torch.cuda.Stream


def _view_struct(v):
    """A view dict (width, height, focal_length, principal_point, xform 3x4 camera-to-world) -> rnb_view."""
    out = View()
    out.width = int(v["width"])
    out.height = int(v["height"])
    out.focal_length[:] = [float(x) for x in v["focal_length"]]
    out.principal_point[:] = [float(x) for x in v["principal_point"]]
    out.xform[:] = [float(x) for x in np.asarray(v["xform"], dtype=np.float32).reshape(12)]
    return out


def view_normal_metrics(image, view, normal_map):
    """One view's comparison of a [H,W,9] image (the layout of rnb_render and of rasterize_mesh's `image`: world-frame normal in channels 0-2, coverage or opacity in 6) with the
    scene's input normal map (uint16 [h,w,4]: the camera-frame normal as (x, -y, -z) in [0, 1], alpha = mask), by the definitions of host/view_metrics.hpp, which
    build/render (render_metrics.json) and build/mesh --report-views use: mask = channel 6 > 0.5, input mask = alpha > 0, the input pixel whose area holds the pixel's
    centre, the angle between the decoded input normal and the image's normal in the camera frame where both masks hold and both are non-zero. Returns a dict of
    mean_angle_deg, median_angle_deg, mask_iou, pixels_compared."""
    img = np.asarray(image, dtype=np.float32)
    h, w = img.shape[:2]
    t = np.asarray(normal_map)
    if t.dtype != np.uint16 or t.ndim != 3 or t.shape[2] != 4:
        raise ValueError("normal_map must be uint16 [h, w, 4]")
    ih, iw = t.shape[:2]
    x = np.asarray(view["xform"], dtype=np.float32).reshape(3, 4)
    mask = img[..., 6] > np.float32(0.5)
    nc = np.stack([(x[0, k] * img[..., 0] + x[1, k] * img[..., 1]) + x[2, k] * img[..., 2] for k in range(3)], axis=-1)  # R^T n, float32, in this order
    ix = np.minimum(iw - 1, ((np.arange(w, dtype=np.float64) + 0.5) * iw / w).astype(np.int64))
    iy = np.minimum(ih - 1, ((np.arange(h, dtype=np.float64) + 0.5) * ih / h).astype(np.int64))
    t = t[iy][:, ix]
    mask_in = t[..., 3] > 0
    inter, uni = int((mask & mask_in).sum()), int((mask | mask_in).sum())
    both = mask & mask_in
    d = t[both][:, :3].astype(np.float64) / 65535.0 * 2.0 - 1.0
    ti = d * np.array([1.0, -1.0, -1.0])
    n = nc[both].astype(np.float64)
    ln = np.sqrt((ti[:, 0] * ti[:, 0] + ti[:, 1] * ti[:, 1]) + ti[:, 2] * ti[:, 2])
    lr = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = (ln > 0) & (lr > 0)
    cs = ((ti[ok, 0] * n[ok, 0] + ti[ok, 1] * n[ok, 1]) + ti[ok, 2] * n[ok, 2]) / (ln[ok] * lr[ok])
    angles = np.arccos(np.minimum(1.0, np.maximum(-1.0, cs))) * 180.0 / math.pi
    mean = median = 0.0
    if angles.size:
        mean = float(sum(float(a) for a in angles) / angles.size)  # summed in pixel order, as the header does
        a = np.sort(angles)
        k = a.size
        median = float(a[k // 2]) if k % 2 else float(0.5 * (a[k // 2 - 1] + a[k // 2]))
    return dict(mean_angle_deg=mean, median_angle_deg=median, mask_iou=(inter / uni if uni else 1.0), pixels_compared=int(angles.size))


def view_albedo_metrics(image, view, albedo_map):
    """One view's comparison of a [H,W,9] image (colour in channels 3-5, coverage or opacity in 6) with the scene's input albedo map (uint16 or uint8 [h,w,4], read as
    x / 65535 or x / 255; alpha = mask), by the definitions of host/view_metrics.hpp with the masks and the choice of input pixel of view_normal_metrics: over the pixels
    where both masks hold, in row-major order and in double, e = image - input per channel, the sums of (|e_0| + |e_1|) + |e_2| and of (e_0^2 + e_1^2) + e_2^2. Returns a
    dict of albedo_mae (the first sum / 3n), albedo_rmse (sqrt(mse), mse = the second sum / 3n), albedo_psnr_db = 10 log10(1 / mse) (values in [0, 1]; inf for mse 0) and
    pixels_compared (n; all three numbers are 0 when it is 0). `view` is not read: the images are compared pixel by pixel."""
    img = np.asarray(image, dtype=np.float32)
    h, w = img.shape[:2]
    t = np.asarray(albedo_map)
    if t.dtype not in (np.uint16, np.uint8) or t.ndim != 3 or t.shape[2] != 4:
        raise ValueError("albedo_map must be uint16 or uint8 [h, w, 4]")
    scale = 65535.0 if t.dtype == np.uint16 else 255.0
    ih, iw = t.shape[:2]
    mask = img[..., 6] > np.float32(0.5)
    ix = np.minimum(iw - 1, ((np.arange(w, dtype=np.float64) + 0.5) * iw / w).astype(np.int64))
    iy = np.minimum(ih - 1, ((np.arange(h, dtype=np.float64) + 0.5) * ih / h).astype(np.int64))
    t = t[iy][:, ix]
    both = mask & (t[..., 3] > 0)
    n = int(both.sum())
    if n == 0:
        return dict(albedo_mae=0.0, albedo_rmse=0.0, albedo_psnr_db=0.0, pixels_compared=0)
    e = img[both][:, 3:6].astype(np.float64) - t[both][:, :3].astype(np.float64) / scale
    a = np.abs(e)
    sum_abs = float(np.cumsum((a[:, 0] + a[:, 1]) + a[:, 2])[-1])  # one after the other, in pixel order, as the header does
    sum_sq = float(np.cumsum((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])[-1])
    mse = sum_sq / (3.0 * n)
    return dict(albedo_mae=sum_abs / (3.0 * n), albedo_rmse=math.sqrt(mse), albedo_psnr_db=(10.0 * math.log10(1.0 / mse) if mse > 0 else math.inf), pixels_compared=n)


def scaled_view(view, factor):
    """The same camera at another resolution: width, height and the focal lengths (pixels) scaled by `factor`, the principal point (normalised to [0, 1])
    kept. factor 0.25 = a quarter of the resolution; the width and height are rounded and at least 1."""
    f = float(factor)
    if not f > 0:
        raise ValueError("scale factor must be positive")
    w, h = max(1, int(round(int(view["width"]) * f))), max(1, int(round(int(view["height"]) * f)))
    fx, fy = (float(x) for x in view["focal_length"])
    out = dict(view)
    out.update(width=w, height=h, focal_length=(fx * w / int(view["width"]), fy * h / int(view["height"])), principal_point=tuple(float(x) for x in view["principal_point"]),
               xform=np.asarray(view["xform"], dtype=np.float32).reshape(3, 4).copy())
    return out


class Context:
    """One training context on the current HIP device (``rnb_ctx``)."""

    def __init__(self, cfg=None, fns=None, **overrides):
        self.f = fns or load_library()
        self.cfg = cfg if cfg is not None else default_config(self.f, **overrides)
        self._h = C.c_void_p()
        self._check(self.f.create(C.byref(self.cfg), C.byref(self._h)))
        self._keep = []

    # -- plumbing -------------------------------------------------------
    def _check(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise RnbError(rc, self.f.last_error().decode(errors="replace"))
        return rc

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.f.destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def update_config(self, **overrides):
        """Run-time switches (loss flags, weights, optimizer hyper-parameters, only_sdf_training)."""
        for k, v in overrides.items():
            if not hasattr(self.cfg, k):
                raise AttributeError("rnb_config has no field %r" % k)
            setattr(self.cfg, k, v)
        self._check(self.f.update_config(self._h, C.byref(self.cfg)))

    @property
    def n_params(self):
        return int(self.f.n_params(self._h))

    def param_layout(self):
        off = (C.c_uint64 * 5)()
        self._check(self.f.param_layout(self._h, off))
        return dict(sdf=off[0], rgb=off[1], grid=off[2], variance=off[3], end=off[4])

    def grid_tables(self):
        n = self.cfg.n_levels
        off = (C.c_uint32 * (n + 1))()
        res = (C.c_uint32 * n)()
        sc = (C.c_float * n)()
        self._check(self.f.grid_tables(self._h, off, res, sc))
        return np.array(off, dtype=np.uint32), np.array(res, dtype=np.uint32), np.array(sc, dtype=np.float32)

    def buffer(self, name, read_only=False):
        """(pointer, n_bytes) of a context buffer; a device pointer for the HIP library. Without ``read_only`` the library assumes the
        caller writes through the pointer before its next call (cached forms of weights / occupancy are dropped, the optimizer-state
        views are packed back); see rnb_buffer in include/rnb_neus2.h."""
        ptr = C.c_void_p()
        nb = C.c_uint64()
        self._check(self.f.buffer(self._h, BUF[name] | (_abi.BUF_READONLY if read_only else 0), C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def params_changed(self):
        """Training weights were written through a pointer kept from buffer("PARAMS_FP16"): drop the cached LDS weight images."""
        self._check(self.f.params_changed(self._h))

    def bitfield_changed(self):
        """The occupancy bitfield was written through a pointer kept from buffer("DENSITY_BITFIELD") (put() calls this itself)."""
        self._check(self.f.bitfield_changed(self._h))

    def get(self, name, count=None, offset=0):
        """Copy (part of) a context buffer to a numpy array; count/offset in elements."""
        ptr, nb = self.buffer(name, read_only=True)
        dt = np.dtype(BUF_DTYPE[name])
        total = nb // dt.itemsize
        if count is None:
            count = total - offset
        if offset + count > total:
            raise ValueError("%s: range [%d, %d) exceeds %d elements" % (name, offset, offset + count, total))
        out = np.empty(count, dtype=dt)
        if count:
            self._check(self.f.memcpy(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr + offset * dt.itemsize),
                                      count * dt.itemsize, _abi.D2H))
        return out

    def put(self, name, array, offset=0):
        """Copy a numpy array into (part of) a context buffer; offset in elements.
        DENSITY_BITFIELD of a single-cascade scene (aabb_scale 1): the march looks a position ON a face of the box up in cascade 1, as the reference does, while the
        skipping and bounding-box forms of the march plan a ray from cascade 0 alone. So cascade 1 may be set, where a face position reads it, only above a non-empty
        4^3 block of cascade 0 -- as in every bitfield update_density_bitfield() builds (cascade 1 = the max-pool of cascade 0). A bitfield written otherwise gives
        samples at face positions that differ from the reference's in those forms; nothing checks it."""
        ptr, nb = self.buffer(name)
        dt = np.dtype(BUF_DTYPE[name])
        a = np.ascontiguousarray(array, dtype=dt).ravel()
        if (offset + a.size) * dt.itemsize > nb:
            raise ValueError("%s: write of %d elements at %d exceeds buffer" % (name, a.size, offset))
        if a.size:
            self._check(self.f.memcpy(self._h, C.c_void_p(ptr + offset * dt.itemsize), a.ctypes.data_as(C.c_void_p),
                                      a.size * dt.itemsize, _abi.H2D))
            if name == "DENSITY_BITFIELD":
                self.bitfield_changed()
            elif name == "PARAMS_FP16":
                self.params_changed()

    # -- parameters -----------------------------------------------------
    def init_params(self, sdf_weights=None):
        w = load_sdf_init_weights() if sdf_weights is None else np.ascontiguousarray(sdf_weights, dtype=np.float32)
        self._check(self.f.init_params(self._h, w.ctypes.data_as(C.POINTER(C.c_float))))

    def set_params(self, params_fp32):
        p = np.ascontiguousarray(params_fp32, dtype=np.float32).ravel()
        if p.size != self.n_params:
            raise ValueError("expected %d params, got %d" % (self.n_params, p.size))
        self._check(self.f.set_params(self._h, p.ctypes.data_as(C.POINTER(C.c_float))))

    # -- dataset --------------------------------------------------------
    def set_dataset(self, views, normals, albedos):
        """views: sequence of dicts(width, height, focal_length(2), principal_point(2), xform(3x4 c2w));
        normals/albedos: per view uint16 arrays [H, W, 4] (RGBA16, alpha = mask)."""
        n = len(views)
        if n == 0 or len(normals) != n or len(albedos) != n:
            raise ValueError("views / normals / albedos must be non-empty and of equal length")
        arr = (View * n)()
        nptr = (C.c_void_p * n)()
        aptr = (C.c_void_p * n)()
        keep = []
        for i, v in enumerate(views):
            arr[i].width = int(v["width"])
            arr[i].height = int(v["height"])
            arr[i].focal_length[:] = [float(x) for x in v["focal_length"]]
            arr[i].principal_point[:] = [float(x) for x in v["principal_point"]]
            arr[i].xform[:] = [float(x) for x in np.asarray(v["xform"], dtype=np.float32).reshape(12)]
            nm = np.ascontiguousarray(normals[i], dtype=np.uint16)
            al = np.ascontiguousarray(albedos[i], dtype=np.uint16)
            if nm.size != arr[i].width * arr[i].height * 4 or al.size != nm.size:
                raise ValueError("view %d: image size does not match width*height*4" % i)
            keep += [nm, al]
            nptr[i] = nm.ctypes.data
            aptr[i] = al.ctypes.data
        self._check(self.f.set_dataset(self._h, n, arr, nptr, aptr))

    # -- stages ---------------------------------------------------------
    def set_training_step(self, step):
        self._check(self.f.set_training_step(self._h, int(step)))

    @property
    def valid_level(self):
        return int(self.f.valid_level(self._h))

    @property
    def training_step(self):
        return int(self.f.training_step(self._h))

    @property
    def rays_per_batch(self):
        return int(self.f.rays_per_batch(self._h))

    def set_controller(self, training_step, rays_per_batch, measured_before_compaction=0, n_rays_total=0):
        self._check(self.f.set_controller(self._h, int(training_step), int(rays_per_batch), int(measured_before_compaction), int(n_rays_total)))

    def eval_primitives(self, kind, items):
        """rnb_eval_primitives: uint32 items [n, words_in(kind)] -> uint32 [n, words_out(kind)] (floats as bit patterns)."""
        k = _abi.PRIM[kind]
        a = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, _abi.PRIM_IN_WORDS[k])
        out = np.empty((a.shape[0], _abi.PRIM_OUT_WORDS[k]), dtype=np.uint32)
        self._check(self.f.eval_primitives(self._h, k, a.ctypes.data_as(C.c_void_p), a.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def set_encode_corners(self, mask):
        """RNB_PRIM_ENCODE_FORM: which kernel groups gather the hash grid with eight lanes per sample (bit 0 network evaluation, 1 point query, 2 training kernels) from the
        next launch on; returns the mask that was in force. Same results either way."""
        return int(self.eval_primitives("ENCODE_FORM", [int(mask)])[0, 0])

    # -- a training state as data (what a snapshot holds, src/testbed.cu:3333-3390, plus the optimizer's moments) ---------------------------
    def training_state(self, last_stats=None):
        """Everything a fresh context needs to continue this run: master weights, Adam moments and per-parameter step counts, EMA weights, the number of optimizer
        steps taken (= the learning-rate schedule's position), the occupancy grid and the ray controller. `last_stats`: the rnb_step_stats of the last step
        (its un-compacted sample count feeds the controller). The ray generator's position is not part of it (nor of the reference's snapshot)."""
        return dict(params=self.get("PARAMS_FP32").copy(), adam_m=self.get("ADAM_M").copy(), adam_v=self.get("ADAM_V").copy(), adam_steps=self.get("ADAM_STEPS").copy(),
                    ema=self.get("PARAMS_EMA").copy(), grid=self.get("DENSITY_GRID").copy(), step=self.training_step, rays=self.rays_per_batch,
                    before=int(last_stats.measured_batch_size_before_compaction) if last_stats is not None else 0)

    def load_training_state(self, state):
        """The inverse: set_params resets the optimizer (trainer.h:263-275), then the moments, step counts and EMA weights are put back, the schedule's position,
        the occupancy grid (and its bitfield) and the controller. Works across accumulate / deterministic modes: the state is mode-independent data."""
        self.set_params(state["params"])
        self.put("ADAM_M", state["adam_m"])
        self.put("ADAM_V", state["adam_v"])
        self.put("ADAM_STEPS", state["adam_steps"])
        self.put("PARAMS_EMA", state["ema"])
        self.set_optimizer_step(state["step"])
        self.put("DENSITY_GRID", state["grid"])
        self.update_density_bitfield()
        self.set_controller(state["step"], state["rays"], state["before"], 0)

    def set_optimizer_step(self, step):
        """Optimizer steps taken so far (adam.h:486-495, exponential_decay.h:143-147): step counter + learning-rate factor."""
        self._check(self.f.set_optimizer_step(self._h, int(step)))

    def gradient_parts(self):
        """[(first, last+1), ...] blocks of GRADS_FP32 in the order they become final during the queued backward pass."""
        arr = (C.c_uint64 * 2 * 3)()
        n = C.c_uint32()
        self._check(self.f.gradient_parts(self._h, C.byref(arr), C.byref(n)))
        return [(int(arr[k][0]), int(arr[k][1])) for k in range(n.value)]

    def train_step_apply_early(self, stream_handle):
        self._check(self.f.train_step_apply_early(self._h, C.c_void_p(stream_handle)))

    def gradient_part_wait(self, part, stream_handle):
        self._check(self.f.gradient_part_wait(self._h, int(part), C.c_void_p(stream_handle)))

    def shard_layout(self):
        """([(lo, hi, own_lo, own_hi), ...], capacity): blocks of the sharded data-parallel optimizer in completion order
        (rnb_shard_layout); every parameter-shaped buffer is allocated up to `capacity` elements."""
        arr = (C.c_uint64 * 4 * 3)()  # RNB_MAX_SHARD_PARTS
        n = C.c_uint32()
        cap = C.c_uint64()
        self._check(self.f.shard_layout(self._h, C.byref(arr), C.byref(n), C.byref(cap)))
        return [tuple(int(arr[k][j]) for j in range(4)) for k in range(n.value)], int(cap.value)

    def train_step_apply_shard(self, part, stream_handle=None):
        self._check(self.f.train_step_apply_shard(self._h, int(part), C.c_void_p(stream_handle)))

    def train_step_apply_done(self, stream_handle=None):
        self._check(self.f.train_step_apply_done(self._h, C.c_void_p(stream_handle)))

    def profile_enable(self, on=True):
        self._check(self.f.profile_enable(self._h, int(bool(on))))

    def profile(self):
        """Per-kernel-group HIP-event timings accumulated since profile_enable(True)."""
        out = []
        for i in range(self.f.profile_count(self._h)):
            name, ms, n, units = C.c_char_p(), C.c_double(), C.c_uint64(), C.c_double()
            self._check(self.f.profile_get(self._h, i, C.byref(name), C.byref(ms), C.byref(n), C.byref(units)))
            out.append(dict(kernel=name.value.decode(), total_ms=ms.value, launches=n.value, units=units.value))
        return out

    def update_density_grid(self, stream=None):
        self._check(self.f.update_density_grid(self._h, _stream_handle(stream)))

    def update_density_grid_begin(self, stream=None):
        """First half of an occupancy update: samples + network on this rank's share (rnb_update_density_grid_begin)."""
        self._check(self.f.update_density_grid_begin(self._h, _stream_handle(stream)))

    def update_density_grid_end(self, stream=None):
        self._check(self.f.update_density_grid_end(self._h, _stream_handle(stream)))

    def set_grid_exchange(self, fn):
        """fn(grid_tmp_ptr, n_elements, stream_handle) -> None takes the element-wise max of DENSITY_GRID_TMP over the data-parallel ranks (stream-ordered);
        None removes it (replicated occupancy updates). rnb_set_grid_exchange."""
        if fn is None:
            self._grid_cb = None
            self._check(self.f.set_grid_exchange(self._h, None, None))
            return

        def trampoline(_user, ptr, n, stream):
            try:
                fn(ptr, int(n), stream)
                return 0
            except Exception:  # no exception may cross the C boundary
                import traceback
                traceback.print_exc()
                return -1
        self._grid_cb = _abi.GRID_EXCHANGE_FN(trampoline)  # kept alive with the context
        self._check(self.f.set_grid_exchange(self._h, C.cast(self._grid_cb, C.c_void_p), None))

    def update_density_bitfield(self, stream=None):
        self._check(self.f.update_density_bitfield(self._h, _stream_handle(stream)))

    def _point_query(self, fn, xyz, inference):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        cptr, cb = self.buffer("COORDS")
        optr, ob = self.buffer("MLP_OUT")
        if n * 12 > cb or n * 2 > ob:
            raise ValueError("too many points for the scratch buffers")
        self.put("COORDS", xyz)
        self._check(fn(self._h, None, C.c_void_p(cptr), n, C.c_void_p(optr), int(bool(inference))))
        return self.get("MLP_OUT", n)

    def density(self, xyz, inference=False):
        """NerfNetwork::density on host points [n,3] -> float16[n] (staged through the context's scratch)."""
        return self._point_query(self.f.density, xyz, inference)

    def sdf(self, xyz, inference=True):
        return self._point_query(self.f.sdf, xyz, inference)

    def forward_infer(self, coords, inference=False):
        """NerfNetwork::inference_mixed_precision on host coords [n,7] -> float16[n,16]."""
        coords = np.ascontiguousarray(coords, dtype=np.float32).reshape(-1, 7)
        n = coords.shape[0]
        cptr, cb = self.buffer("COORDS")
        optr, ob = self.buffer("MLP_OUT")
        if n * 28 > cb or n * 32 > ob:
            raise ValueError("too many samples for the scratch buffers")
        self.put("COORDS", coords)
        self._check(self.f.forward_infer(self._h, None, C.c_void_p(cptr), n, C.c_void_p(optr), int(bool(inference))))
        return self.get("MLP_OUT", n * 16).reshape(n, 16)

    # -- rendering (include/rnb_render.h; Testbed::render_nerf / NerfTracer::trace, src/testbed_nerf.cu:2499-2770) ----------------------
    def _render_options(self, min_transmittance, inference, occupancy, max_rays_in_flight, near_distance):
        opt = _abi.RenderOptions()
        self._check(self.f.render_default_options(C.byref(opt)))
        opt.min_transmittance = float(min_transmittance)
        opt.use_inference_params = int(bool(inference))
        opt.use_occupancy = int(bool(occupancy))
        opt.max_rays_in_flight = int(max_rays_in_flight)
        if near_distance is not None:
            opt.near_distance = float(near_distance)
        return opt

    def render_into(self, view, out_ptr, min_transmittance=0.01, inference=True, occupancy=True, max_rays_in_flight=0, near_distance=None, stream=None):
        """rnb_render into device memory: out_ptr receives view height x width x RENDER_CHANNELS float32 (see include/rnb_render.h for the channels).
        Returns the rnb_render_stats as a dict. Leaves the training state as it was."""
        st = _abi.RenderStats()
        opt = self._render_options(min_transmittance, inference, occupancy, max_rays_in_flight, near_distance)
        self._check(self.f.render(self._h, _stream_handle(stream), C.byref(_view_struct(view)), C.byref(opt), C.c_void_p(out_ptr), C.byref(st)))
        return st.as_dict()

    def render(self, view, min_transmittance=0.01, inference=True, occupancy=True, max_rays_in_flight=0, near_distance=None, stream=None):
        """The maps the model predicts for one camera (a view dict as set_dataset takes): normal [H,W,3] (unit, world frame, 0 where nothing is hit),
        albedo [H,W,3], opacity, depth (camera-forward, of the max-weight sample; 0 where opacity <= 0.2) and n_samples [H,W], plus `stats`; numpy arrays on the host.
        inference: EMA weights (what a snapshot holds); occupancy: skip the cells the occupancy bitfield marks empty; min_transmittance: 0 composites every ray to the
        box exit; max_rays_in_flight (0 = 2^19) bounds the workspace and does not change the image."""
        h, w = int(view["height"]), int(view["width"])
        n = h * w * RENDER_CHANNELS
        ptr = self.device_malloc(max(n, 1) * 4)
        try:
            stats = self.render_into(view, ptr, min_transmittance, inference, occupancy, max_rays_in_flight, near_distance, stream)
            img = self.download(ptr, n, np.float32).reshape(h, w, RENDER_CHANNELS)
        finally:
            self.device_free(ptr)
        return dict(normal=img[..., 0:3].copy(), albedo=img[..., 3:6].copy(), opacity=img[..., 6].copy(), depth=img[..., 7].copy(),
                    n_samples=img[..., 8].astype(np.uint32), stats=stats)

    # -- mesh extraction (src/testbed_nerf.cu:4218-4269, src/marching_cubes.cu:794-822) ----------------------
    def device_malloc(self, n_bytes):
        ptr = C.c_void_p()
        self._check(self.f.device_malloc(self._h, int(n_bytes), C.byref(ptr)))
        return ptr.value

    def device_free(self, ptr):
        self._check(self.f.device_free(self._h, C.c_void_p(ptr)))

    def sdf_lattice(self, res, lattice_min=0.0, lattice_max=1.0, inference=True):
        """SDF on the lattice res^3 (int or 3 ints, x fastest) of [lattice_min, lattice_max)^3 -> library-side pointer to
        float[res^3] (device memory for the HIP library); release with device_free."""
        r = (C.c_uint32 * 3)(*([int(res)] * 3 if np.isscalar(res) else [int(x) for x in res]))
        ptr = self.device_malloc(int(r[0]) * int(r[1]) * int(r[2]) * 4)
        self._check(self.f.sdf_lattice(self._h, None, r, float(lattice_min), float(lattice_max), C.c_void_p(ptr), int(bool(inference))))
        return ptr

    def marching_cubes(self, density_ptr, res, aabb_min=(0.0, 0.0, 0.0), aabb_max=(1.0, 1.0, 1.0), thresh=0.0):
        """Iso-surface of a library-side lattice -> (verts float32[n,3], indices uint32[m]) on the host."""
        r = (C.c_uint32 * 3)(*([int(res)] * 3 if np.isscalar(res) else [int(x) for x in res]))
        mn, mx = (C.c_float * 3)(*[float(x) for x in aabb_min]), (C.c_float * 3)(*[float(x) for x in aabb_max])
        pv, pi, nv, ni = C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
        self._check(self.f.marching_cubes(self._h, None, C.c_void_p(density_ptr), r, mn, mx, float(thresh), C.byref(pv), C.byref(pi), C.byref(nv), C.byref(ni)))
        verts = np.empty((nv.value, 3), np.float32)
        idx = np.empty(ni.value, np.uint32)
        if nv.value:
            self._check(self.f.memcpy(self._h, verts.ctypes.data_as(C.c_void_p), pv, nv.value * 12, _abi.D2H))
        if ni.value:
            self._check(self.f.memcpy(self._h, idx.ctypes.data_as(C.c_void_p), pi, ni.value * 4, _abi.D2H))
        self.device_free(pv.value)
        self.device_free(pi.value)
        return verts, idx

    def extract_mesh_device(self, res=256, lattice_min=0.0, lattice_max=1.0, aabb_min=(0.0, 0.0, 0.0), aabb_max=(1.0, 1.0, 1.0), thresh=0.0, inference=True,
                            cull="occupancy", brick=0, colors=False, normals=False, max_points_in_flight=0, max_active_points=0, stream=None):
        """rnb_extract_mesh (include/rnb_mesh.h) -> a DeviceMesh, its `stats` the rnb_mesh_stats of the call: the lattice and attribute arguments of extract_mesh, which
        describes them; the mesh stays on the device for clean / simplify / distance_to / rasterize / download. Leaves the training state as it was."""
        opt = _abi.MeshOptions()
        self._check(self.f.mesh_default_options(C.byref(opt)))
        opt.res[:] = [int(res)] * 3 if np.isscalar(res) else [int(x) for x in res]
        opt.lattice_min, opt.lattice_max = float(lattice_min), float(lattice_max)
        opt.aabb_min[:] = [float(x) for x in aabb_min]
        opt.aabb_max[:] = [float(x) for x in aabb_max]
        opt.thresh = float(thresh)
        opt.use_inference_params = int(bool(inference))
        if cull not in ("none", "occupancy", _abi.MESH_CULL_NONE, _abi.MESH_CULL_OCCUPANCY):
            raise ValueError("cull must be 'none' or 'occupancy'")
        opt.cull = {"none": _abi.MESH_CULL_NONE, "occupancy": _abi.MESH_CULL_OCCUPANCY}.get(cull, cull)
        opt.brick = int(brick)
        opt.attributes = (_abi.MESH_ATTR_COLORS if colors else 0) | (_abi.MESH_ATTR_NORMALS if normals else 0)
        opt.max_points_in_flight = int(max_points_in_flight)
        opt.max_active_points = int(max_active_points)
        st = _abi.MeshStats()
        return _returned_mesh(self, st, lambda m: self.f.extract_mesh(self._h, _stream_handle(stream), C.byref(opt), m, C.byref(st)))

    def extract_mesh(self, res=256, lattice_min=0.0, lattice_max=1.0, aabb_min=(0.0, 0.0, 0.0), aabb_max=(1.0, 1.0, 1.0), thresh=0.0, inference=True,
                     cull="occupancy", brick=0, colors=False, normals=False, max_points_in_flight=0, max_active_points=0, stream=None, keep=None, orient=None,
                     simplify=None, placement="quadric", error=False, texture=None, texture_maps=("albedo",), seen_by=None, seen_masks=None, texture_from=None, repair=None, topology=False, fill_holes=None,
                     self_intersections=None, smooth=None, snap=None):
        """rnb_extract_mesh (include/rnb_mesh.h): the iso-surface on the lattice res (int or 3 ints) extracted brick by brick, the bricks the occupancy bitfield
        marks empty skipped (cull="occupancy", the default; "none" keeps every brick and gives the mesh of sdf_lattice + marching_cubes in brick-major order).
        Returns a dict of numpy arrays: verts float32[n,3], indices uint32[m], colors / normals float32[n,3] when asked for, and `stats`.
        The device mesh is released before returning. Leaves the training state as it was.
        keep ("all" / "largest") and / or orient ("none" / "outward"): the device mesh goes through rnb_mesh_clean (see clean_mesh) before it is downloaded, and the
        dict gains `clean_stats`. The one not given leaves its part alone (keep="all", orient="none"), as build/mesh --keep / --orient do. With both None (the
        default) nothing of that runs.
        simplify = N: after that, still on the device, the mesh goes through rnb_mesh_simplify (see simplify_mesh) on the grid simplify_grid(aabb_min, aabb_max, N) --
        N^3 cubic cells from aabb_min, N along the longest edge of the box, the grid of build/mesh --simplify N -- with `placement`, and the dict gains `simplify_stats`. With None (the default) nothing of that runs.
        error=True (with simplify only): the distance between the mesh handed to the simplifier and the one it returned is measured on the device before anything is
        downloaded (rnb_mesh_distance in both directions, its default options; see mesh_distance) and returned under `simplify_error`: the dict of
        mesh_distance(input, output, symmetric=True), A = the simplifier's input (a simplification that leaves no triangle fails the call: there is nothing to measure against). With False (the default) nothing
        of that runs and the result is as it was.
        texture = S: the final mesh (after keep, orient and simplify), still on the device, gets a texture bake of S texels per side (rnb_mesh_bake_texture, see
        bake_texture) with the maps of `texture_maps`, and the dict gains `texture`: the dict of DeviceMesh.bake_texture. With None (the default) nothing of that runs.
        seen_by = views: after keep / orient and before simplify, still on the device, what none of these cameras sees is removed (DeviceMesh.cull_unseen with its
        defaults: whole components, see cull_unseen_mesh; seen_masks = one mask or None per view), and the dict gains `seen_stats` (the select stats) and
        `visibility_stats`. With None (the default) nothing of that runs and the calls made are exactly those made without it.
        texture_from = (views, images) (with texture = S only): the texture is not baked from the model but projected from these images (rnb_mesh_project_views, see
        project_views, its defaults; the mesh's vertex normals weight the views when normals=True), with the model's albedo as the fallback of the texels no view
        reaches, and `texture` is the dict of DeviceMesh.project_views (`color` where a bake has `albedo`; texture_maps does not apply). With None (the default) nothing
        of that runs.
        repair = dict(...): after simplify and before error / texture, still on the device, the mesh goes through rnb_mesh_repair with these arguments of
        DeviceMesh.repair (weld, drop_degenerate, duplicates, orient, buckets_log2), and the dict gains `repair_stats`; with error=True the distance is then measured to
        the repaired mesh. topology=True: the dict gains `topology`, the statistics of DeviceMesh.topology() of the final mesh. With None / False (the defaults)
        nothing of that runs and the calls made are exactly those made without them.
        fill_holes = True or dict(...): after seen_by and repair and before error / topology / texture, still on the device, the boundary loops of the mesh are closed by
        rnb_mesh_fill_holes (include/rnb_mesh_holes.h) with these arguments of DeviceMesh.fill_holes (max_edges, skip_largest, buckets_log2; True: its defaults), and
        the dict gains `fill_stats`; with error=True the distance is then measured to the filled mesh. With None (the default) nothing of that runs and the calls made
        are exactly those made without it.
        self_intersections = True: the dict gains `self_intersections`, the dict of DeviceMesh.self_intersections() of the final mesh (after fill_holes: a fan can
        fold through its neighbours, and this is the report that tells). "drop": after simplify / repair and before fill_holes, still on the device, the triangles
        with a proper partner are removed (DeviceMesh.drop_intersecting, its defaults; fill_holes then closes the rims), and the dict gains `drop_stats`. A dict
        chooses both: drop ("proper" / "all" / None), rings, cells, report (True / False). With None (the default) nothing of that runs and the calls made are
        exactly those made without it.
        smooth = True, N or dict(...): after fill_holes and before the self-intersection report, error, topology and texture, still on the device, the mesh goes through
        rnb_mesh_smooth (include/rnb_mesh_smooth.h): True = the defaults of DeviceMesh.smooth, N = that many passes, a dict = its arguments passes, lam, mu, boundary,
        select_rings, normals and buckets_log2, or only_fills=R (with fill_holes only): only the vertices fill_holes appended and R rings around them move, which relaxes
        the flat fans and leaves the rest of the mesh as it was. The dict gains `smooth_stats`; with error=True the distance is then measured to the smoothed mesh. With
        None (the default) nothing of that runs and the calls made are exactly those made without it.
        snap = True, N or dict(...): after smooth and before the self-intersection report, error, topology and texture, still on the device, the vertices are moved back
        onto the model's surface by rnb_mesh_snap (include/rnb_mesh_snap.h) at level = thresh with the weights of `inference`: True = the defaults of DeviceMesh.snap,
        N = that many iterations, a dict = its arguments iterations, tolerance, max_step, max_displacement, min_gradient, attributes and max_points_in_flight, or
        only_fills=True (with fill_holes only): only the vertices fill_holes appended move, and those a smoothing moved. The dict gains `snap_stats`; with error=True
        the distance is then measured to the snapped mesh. With None (the default) nothing of that runs and the calls made are exactly those made without it."""
        if snap is True:
            snap = {}
        elif isinstance(snap, (int, np.integer)) and snap is not False:
            snap = dict(iterations=int(snap))
        if snap is not None and not isinstance(snap, dict):
            raise ValueError("snap must be None, True, a number of iterations or a dict of DeviceMesh.snap's arguments")
        if snap is not None and set(snap) - {"iterations", "tolerance", "max_step", "max_displacement", "min_gradient", "attributes", "max_points_in_flight", "only_fills"}:
            raise ValueError("snap takes iterations, tolerance, max_step, max_displacement, min_gradient, attributes, max_points_in_flight and only_fills")
        snap_only_fills = False
        if snap is not None:
            snap = dict(snap)
            snap_only_fills = bool(snap.pop("only_fills", False))
            if snap_only_fills and fill_holes is None:
                raise ValueError("snap['only_fills'] needs fill_holes")
            self._snap_options(level=thresh, inference=inference, **snap)  # a bad argument fails before anything is extracted
        if smooth is True:
            smooth = {}
        elif isinstance(smooth, (int, np.integer)) and smooth is not False:
            smooth = dict(passes=int(smooth))
        if smooth is not None and not isinstance(smooth, dict):
            raise ValueError("smooth must be None, True, a number of passes or a dict of DeviceMesh.smooth's arguments")
        if smooth is not None and set(smooth) - {"passes", "lam", "mu", "boundary", "select_rings", "normals", "buckets_log2", "only_fills"}:
            raise ValueError("smooth takes passes, lam, mu, boundary, select_rings, normals, buckets_log2 and only_fills")
        if smooth is not None:
            smooth = dict(smooth)
            only_fills = smooth.pop("only_fills", None)
            if only_fills is not None and fill_holes is None:
                raise ValueError("smooth['only_fills'] needs fill_holes")
            if only_fills is not None and "select_rings" in smooth:
                raise ValueError("smooth takes only_fills or select_rings, not both")
            if only_fills is not None:
                smooth["select_rings"] = int(only_fills)
            self._smooth_options(**smooth)  # a bad argument fails before anything is extracted
        if self_intersections is True:
            self_intersections = dict(report=True)
        elif self_intersections == "drop":
            self_intersections = dict(drop="proper")
        if self_intersections is not None and not isinstance(self_intersections, dict):
            raise ValueError("self_intersections must be None, True, 'drop' or a dict")
        if self_intersections is not None and set(self_intersections) - {"drop", "rings", "cells", "report"}:
            raise ValueError("self_intersections takes drop, rings, cells and report")
        si = self_intersections or {}
        si_drop, si_report, si_cells = si.get("drop"), bool(si.get("report")), si.get("cells", 0)
        if si_drop not in (None, "proper", "all"):
            raise ValueError("self_intersections['drop'] must be 'proper', 'all' or None")
        if si:
            self._intersect_options(si_cells)
            self._intersect_select_options(si_drop or "proper", si.get("rings", 0))  # a bad argument fails before anything is extracted
        if fill_holes is True:
            fill_holes = {}
        if fill_holes is not None and not isinstance(fill_holes, dict):
            raise ValueError("fill_holes must be None, True or a dict of DeviceMesh.fill_holes' arguments")
        if fill_holes is not None and set(fill_holes) - {"max_edges", "skip_largest", "buckets_log2"}:
            raise ValueError("fill_holes takes max_edges, skip_largest and buckets_log2")
        if repair is not None and not isinstance(repair, dict):
            raise ValueError("repair must be None or a dict of DeviceMesh.repair's arguments")
        if repair is not None and set(repair) - {"weld", "drop_degenerate", "duplicates", "orient", "buckets_log2"}:
            raise ValueError("repair takes weld, drop_degenerate, duplicates, orient and buckets_log2")
        if texture_from is not None and texture is None:
            raise ValueError("texture_from needs texture")
        if texture_from is not None and len(texture_from) != 2:
            raise ValueError("texture_from must be (views, images)")
        if seen_masks is not None and seen_by is None:
            raise ValueError("seen_masks needs seen_by")
        if error and simplify is None:
            raise ValueError("error=True needs simplify")
        grid = None if simplify is None else self.simplify_grid(aabb_min, aabb_max, simplify)
        chain = [self.extract_mesh_device(res, lattice_min, lattice_max, aabb_min, aabb_max, thresh, inference, cull, brick, colors, normals, max_points_in_flight,
                                          max_active_points, stream)]
        try:  # device to device: the extracted mesh never visits the host
            if keep is not None or orient is not None:
                chain.append(chain[-1].clean("all" if keep is None else keep, "none" if orient is None else orient, stream=stream))
            if seen_by is not None:
                culled, seen = chain[-1].cull_unseen(seen_by, seen_masks, stream=stream, report=True)
                chain.append(culled)
            if grid is not None:
                chain.append(chain[-1].simplify(*grid, placement=placement, stream=stream))
                simplified = chain[-1]
                before = chain[-2]
            if repair is not None:
                chain.append(chain[-1].repair(stream=stream, **repair))
                repaired = chain[-1]
            if si_drop is not None:
                chain.append(chain[-1].drop_intersecting(si_drop, si.get("rings", 0), cells=si_cells, stream=stream))
                dropped = chain[-1]
            if fill_holes is not None:
                chain.append(chain[-1].fill_holes(stream=stream, **fill_holes))
                filled = chain[-1]
            if smooth is not None:
                appended = None if only_fills is None else np.arange(filled.n_verts) >= filled.stats["n_verts_out"] - filled.stats["n_verts_added"]
                chain.append(chain[-1].smooth(select=appended, stream=stream, **dict(smooth, displacement=True) if snap_only_fills else smooth))
                smoothed = chain[-1]
            if snap is not None:
                chosen = None
                if snap_only_fills:
                    chosen = np.arange(filled.n_verts) >= filled.stats["n_verts_out"] - filled.stats["n_verts_added"]
                    if smooth is not None:
                        chosen = chosen | (smoothed.displacement > 0)
                chain.append(chain[-1].snap(level=thresh, select=chosen, inference=inference, stream=stream, **snap))
                snapped = chain[-1]
            if si_report:
                si_census = chain[-1].self_intersections(cells=si_cells, stream=stream)
            if grid is not None and error:
                simplify_error = before.distance_to(chain[-1], symmetric=True, stream=stream)
            if topology:
                census = chain[-1].topology(stream=stream)
            if texture is not None and texture_from is not None:
                baked = chain[-1].project_views(texture_from[0], texture_from[1], texture, fallback="model", inference=inference, stream=stream)
            elif texture is not None:
                baked = chain[-1].bake_texture(texture, maps=texture_maps, inference=inference, stream=stream)
            out = chain[-1].download()
            out["stats"] = chain[0].stats
            if texture is not None:
                out["texture"] = baked
            if grid is not None and error:
                out["simplify_error"] = simplify_error
            if seen_by is not None:
                out["seen_stats"], out["visibility_stats"] = seen["select"], seen["visibility"]
            if keep is not None or orient is not None:
                out["clean_stats"] = chain[1].stats
            if grid is not None:
                out["simplify_stats"] = simplified.stats
            if repair is not None:
                out["repair_stats"] = repaired.stats
            if fill_holes is not None:
                out["fill_stats"] = filled.stats
            if smooth is not None:
                out["smooth_stats"] = smoothed.stats
            if snap is not None:
                out["snap_stats"] = snapped.stats
            if topology:
                out["topology"] = census
            if si_drop is not None:
                out["drop_stats"] = dropped.stats
            if si_report:
                out["self_intersections"] = si_census
        finally:
            for m in chain:  # whatever exists by now, oldest first
                m.free()
        return out

    def _clean_options(self, keep, orient):
        keeps = {"all": _abi.MESH_KEEP_ALL, "largest": _abi.MESH_KEEP_LARGEST}
        orients = {"none": _abi.MESH_ORIENT_NONE, "outward": _abi.MESH_ORIENT_OUTWARD}
        if keep not in keeps:
            raise ValueError("keep must be 'all' or 'largest'")
        if orient not in orients:
            raise ValueError("orient must be 'none' or 'outward'")
        opt = _abi.MeshCleanOptions()
        self._check(self.f.mesh_clean_default_options(C.byref(opt)))
        opt.keep, opt.orient = keeps[keep], orients[orient]
        return opt

    def upload_mesh(self, verts, indices, colors=None, normals=None):
        """A host mesh (verts float32[n,3], indices uint32[m] or [m/3,3], optional per-vertex colors / normals) -> a DeviceMesh; free it (or use it in a `with`) to release the uploads."""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        arrays = dict(verts=v, indices=np.ascontiguousarray(indices, dtype=np.uint32).ravel())
        for key, a in (("colors", colors), ("normals", normals)):
            if a is not None:
                arrays[key] = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
                if arrays[key].shape != v.shape:
                    raise ValueError("%s must have one row per vertex" % key)
        m = DeviceMesh(self, buffers=[])
        try:
            for key, a in arrays.items():
                m._buffers.append(self.upload(a) if a.size else self.device_malloc(4))
                setattr(m, key, m._buffers[-1])
            _abi.Mesh.n_verts.__set__(m, v.shape[0])
            m.n_indices = arrays["indices"].size
        except BaseException:
            m.free()
            raise
        return m

    def clean_mesh(self, verts, indices, colors=None, normals=None, keep="largest", orient="outward", table=False, stream=None):
        """rnb_mesh_clean (include/rnb_mesh_clean.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals. The
        connected components (vertices joined by triangles), keep="largest" (greatest area; "all": only unused vertices go), orient="outward" (the triangles of a
        component of negative signed volume get their second and third index swapped; "none": as they come). Returns a dict of numpy arrays (verts, indices, colors /
        normals when given) in the input's order, `stats`, and with table=True `table`: one record per component (label, n_vertices, n_triangles, kept, area_q,
        volume_q), ascending label. For a dict m that extract_mesh returned: clean_mesh(m["verts"], m["indices"], m.get("colors"), m.get("normals")). Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            cleaned = m.clean(keep, orient, table, stream)
        with cleaned:
            out = cleaned.download()
            out["stats"] = cleaned.stats
            if table:
                out["table"] = cleaned.table
        return out

    def _topology_options(self, buckets_log2=0):
        opt = _abi.MeshTopologyOptions()
        self._check(self.f.mesh_topology_default_options(C.byref(opt)))
        opt.buckets_log2 = int(buckets_log2)
        return opt

    def _repair_options(self, weld=False, drop_degenerate=True, duplicates="first", orient="none", buckets_log2=0):
        dups = {"keep": _abi.MESH_DUPLICATES_KEEP, "first": _abi.MESH_DUPLICATES_FIRST, "cancel": _abi.MESH_DUPLICATES_CANCEL}
        orients = {"none": _abi.MESH_REPAIR_ORIENT_NONE, "consistent": _abi.MESH_REPAIR_ORIENT_CONSISTENT}
        if duplicates not in dups:
            raise ValueError("duplicates must be 'keep', 'first' or 'cancel'")
        if orient not in orients:
            raise ValueError("orient must be 'none' or 'consistent'")
        opt = _abi.MeshRepairOptions()
        self._check(self.f.mesh_repair_default_options(C.byref(opt)))
        opt.weld, opt.drop_degenerate, opt.duplicates, opt.orient, opt.buckets_log2 = int(bool(weld)), int(bool(drop_degenerate)), dups[duplicates], orients[orient], int(buckets_log2)
        return opt

    def mesh_topology(self, verts, indices, edges=False, table=False, buckets_log2=0, stream=None):
        """rnb_mesh_topology (include/rnb_mesh_topology.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]): the dict of DeviceMesh.topology, which
        describes the keys. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices) as m:
            return m.topology(edges, table, buckets_log2, stream)

    def repair_mesh(self, verts, indices, colors=None, normals=None, weld=False, drop_degenerate=True, duplicates="first", orient="none", vertex_map=False, buckets_log2=0,
                    stream=None):
        """rnb_mesh_repair (include/rnb_mesh_topology.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals; the
        steps and their arguments are those of DeviceMesh.repair. Returns a dict of numpy arrays like clean_mesh, with `stats` = `repair_stats` and, with
        vertex_map=True, `vertex_map`. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            repaired = m.repair(weld, drop_degenerate, duplicates, orient, vertex_map, buckets_log2, stream)
        with repaired:
            out = repaired.download()
            out["stats"] = out["repair_stats"] = repaired.stats
            if vertex_map:
                out["vertex_map"] = repaired.vertex_map
        return out

    def _boundary_loops_options(self, buckets_log2=0):
        opt = _abi.MeshBoundaryLoopsOptions()
        self._check(self.f.mesh_boundary_loops_default_options(C.byref(opt)))
        opt.buckets_log2 = int(buckets_log2)
        return opt

    def _fill_holes_options(self, max_edges=0, skip_largest=False, buckets_log2=0):
        if int(max_edges) < 0 or int(max_edges) > 0xFFFFFFFF:
            raise ValueError("max_edges must be 0 (every loop) or a positive count")
        opt = _abi.MeshFillHolesOptions()
        self._check(self.f.mesh_fill_holes_default_options(C.byref(opt)))
        opt.max_edges, opt.skip_largest, opt.buckets_log2 = int(max_edges), int(bool(skip_largest)), int(buckets_log2)
        return opt

    def mesh_boundary_loops(self, verts, indices, colors=None, edges=False, table=True, buckets_log2=0, stream=None):
        """rnb_mesh_boundary_loops (include/rnb_mesh_holes.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]; colors only take part in the checks): the
        dict of DeviceMesh.boundary_loops, which describes the keys. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors) as m:
            return m.boundary_loops(edges, table, buckets_log2, stream)

    def fill_mesh_holes(self, verts, indices, colors=None, normals=None, max_edges=0, skip_largest=False, loop_of_tri=False, buckets_log2=0, stream=None):
        """rnb_mesh_fill_holes (include/rnb_mesh_holes.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals; the
        arguments are those of DeviceMesh.fill_holes. Returns a dict of numpy arrays like clean_mesh, with `stats` = `fill_stats` and, with loop_of_tri=True,
        `loop_of_tri`. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            filled = m.fill_holes(max_edges, skip_largest, loop_of_tri, buckets_log2, stream)
        with filled:
            out = filled.download()
            out["stats"] = out["fill_stats"] = filled.stats
            if loop_of_tri:
                out["loop_of_tri"] = filled.loop_of_tri
        return out

    def _smooth_options(self, passes=2, lam=0.5, mu=-0.53, boundary="pin", select_rings=0, normals="keep", buckets_log2=0):
        bounds = {"pin": _abi.MESH_SMOOTH_BOUNDARY_PIN, "slide": _abi.MESH_SMOOTH_BOUNDARY_SLIDE, "free": _abi.MESH_SMOOTH_BOUNDARY_FREE}
        norms = {"keep": _abi.MESH_SMOOTH_NORMALS_KEEP, "recompute": _abi.MESH_SMOOTH_NORMALS_RECOMPUTE}
        if boundary not in bounds:
            raise ValueError("boundary must be 'pin', 'slide' or 'free'")
        if normals not in norms:
            raise ValueError("normals must be 'keep' or 'recompute'")
        if isinstance(passes, bool) or not 0 <= int(passes) <= _abi.MESH_SMOOTH_MAX_PASSES:
            raise ValueError("passes must be 0 .. 10000")
        if not 0 <= int(select_rings) <= _abi.MESH_SMOOTH_MAX_SELECT_RINGS:
            raise ValueError("select_rings must be 0 .. 1024")
        if not 0.0 < float(lam) <= 1.0:
            raise ValueError("lam must be above 0 and at most 1")
        if not -1.5 <= float(mu) <= 0.0:
            raise ValueError("mu must be at least -1.5 and at most 0")
        opt = _abi.MeshSmoothOptions()
        self._check(self.f.mesh_smooth_default_options(C.byref(opt)))
        opt.passes, opt.lambda_, opt.mu, opt.boundary, opt.select_rings, opt.normals, opt.buckets_log2 = int(passes), float(lam), float(mu), bounds[boundary], int(select_rings), norms[normals], int(buckets_log2)
        return opt

    def _vertex_normals_options(self, flip=False):
        opt = _abi.MeshVertexNormalsOptions()
        self._check(self.f.mesh_vertex_normals_default_options(C.byref(opt)))
        opt.flip = int(bool(flip))
        return opt

    def smooth_mesh(self, verts, indices, colors=None, normals_in=None, passes=2, lam=0.5, mu=-0.53, boundary="pin", select=None, select_rings=0, normals="keep", displacement=False,
                    census=False, buckets_log2=0, stream=None):
        """rnb_mesh_smooth (include/rnb_mesh_smooth.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals_in; the
        other arguments are those of DeviceMesh.smooth. Returns a dict of numpy arrays like clean_mesh, with `stats` = `smooth_stats` and, when asked for,
        `displacement`, `valence` and `kind`. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals_in) as m:
            smoothed = m.smooth(passes, lam, mu, boundary, select, select_rings, normals, displacement, census, buckets_log2, stream)
        with smoothed:
            out = smoothed.download()
            out["stats"] = out["smooth_stats"] = smoothed.stats
            if displacement:
                out["displacement"] = smoothed.displacement
            if census:
                out["valence"], out["kind"] = smoothed.valence, smoothed.kind
        return out

    def _snap_options(self, iterations=3, tolerance=None, max_step=None, max_displacement=None, min_gradient=None, level=0.0, attributes=(), inference=True, max_points_in_flight=0):
        """The options of rnb_mesh_snap; None leaves the library's default. The ranges are the header's, checked here before any call."""
        bits = {"colors": _abi.MESH_ATTR_COLORS, "normals": _abi.MESH_ATTR_NORMALS}
        if isinstance(attributes, str):
            attributes = (attributes,)
        if set(attributes) - set(bits):
            raise ValueError("attributes must be a set of 'colors' and 'normals'")
        if isinstance(iterations, bool) or not 0 <= int(iterations) <= _abi.MESH_SNAP_MAX_ITERATIONS:
            raise ValueError("iterations must be 0 .. 64")
        opt = _abi.MeshSnapOptions()
        self._check(self.f.mesh_snap_default_options(C.byref(opt)))
        for name, value, low, strict in (("level", level, None, False), ("tolerance", tolerance, 0.0, False), ("max_step", max_step, 0.0, True),
                                         ("max_displacement", max_displacement, 0.0, False), ("min_gradient", min_gradient, 0.0, True)):
            if value is None:
                continue
            value = float(value)
            if not np.isfinite(value) or (low is not None and (value <= low if strict else value < low)):
                raise ValueError("%s must be finite%s" % (name, "" if low is None else (" and above 0" if strict else " and at least 0")))
            setattr(opt, name, value)
        if not 0 <= int(max_points_in_flight) < 1 << 32:
            raise ValueError("max_points_in_flight must be 0 .. 2^32 - 1")
        opt.iterations, opt.use_inference_params, opt.max_points_in_flight = int(iterations), int(bool(inference)), int(max_points_in_flight)
        opt.attributes = sum(bits[a] for a in set(attributes))
        return opt

    def snap_mesh(self, verts, indices, colors=None, normals=None, iterations=3, tolerance=None, max_step=None, max_displacement=None, min_gradient=None, level=0.0, select=None,
                  attributes=(), inference=True, max_points_in_flight=0, residuals=False, states=False, displacement=False, stream=None):
        """rnb_mesh_snap (include/rnb_mesh_snap.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals; the other
        arguments are those of DeviceMesh.snap. Returns a dict of numpy arrays like clean_mesh, with `stats` = `snap_stats` and, when asked for, `residual_before`,
        `residual_after`, `state` and `displacement`. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            snapped = m.snap(iterations, tolerance, max_step, max_displacement, min_gradient, level, select, attributes, inference, max_points_in_flight, residuals, states, displacement, stream)
        with snapped:
            out = snapped.download()
            out["stats"] = out["snap_stats"] = snapped.stats
            if residuals:
                out["residual_before"], out["residual_after"] = snapped.residual_before, snapped.residual_after
            if states:
                out["state"] = snapped.state
            if displacement:
                out["displacement"] = snapped.displacement
        return out

    def mesh_vertex_normals(self, verts, indices, flip=False, stream=None):
        """rnb_mesh_vertex_normals (include/rnb_mesh_smooth.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]): the dict of DeviceMesh.vertex_normals.
        Leaves the training state as it was."""
        with self.upload_mesh(verts, indices) as m:
            return m.vertex_normals(flip, stream=stream)

    def _intersect_options(self, cells=0):
        if not 0 <= int(cells) <= _abi.MESH_INTERSECT_MAX_CELLS:
            raise ValueError("cells must be 0 .. 256")
        opt = _abi.MeshIntersectOptions()
        self._check(self.f.mesh_intersect_default_options(C.byref(opt)))
        opt.cells = int(cells)
        return opt

    def _intersect_select_options(self, classes="proper", rings=0, drop_unused_vertices=True):
        masks = {"proper": _abi.MESH_INTERSECT_PROPER, "contact": _abi.MESH_INTERSECT_CONTACT, "all": _abi.MESH_INTERSECT_PROPER | _abi.MESH_INTERSECT_CONTACT}
        if classes not in masks:
            raise ValueError("classes must be 'proper', 'contact' or 'all'")
        if not 0 <= int(rings) <= _abi.MESH_INTERSECT_MAX_RINGS:
            raise ValueError("rings must be 0 .. 8")
        opt = _abi.MeshIntersectSelectOptions()
        self._check(self.f.mesh_intersections_select_default_options(C.byref(opt)))
        opt.classes, opt.rings, opt.drop_unused_vertices = masks[classes], int(rings), int(bool(drop_unused_vertices))
        return opt

    def mesh_self_intersections(self, verts, indices, pairs=False, cells=0, stream=None):
        """rnb_mesh_intersections (include/rnb_mesh_intersect.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]): the dict of
        DeviceMesh.self_intersections, which describes the keys. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices) as m:
            return m.self_intersections(pairs, cells, stream=stream)

    def drop_intersecting_mesh(self, verts, indices, colors=None, normals=None, classes="proper", rings=0, drop_unused_vertices=True, cells=0, stream=None):
        """rnb_mesh_intersections, then rnb_mesh_intersections_select (include/rnb_mesh_intersect.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]),
        optional per-vertex colors / normals; the arguments are those of DeviceMesh.drop_intersecting. Returns a dict of numpy arrays like clean_mesh, with `stats` =
        `drop_stats` (the select stats, the census under `census`). Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            dropped = m.drop_intersecting(classes, rings, drop_unused_vertices=drop_unused_vertices, cells=cells, stream=stream)
        with dropped:
            out = dropped.download()
            out["stats"] = out["drop_stats"] = dropped.stats
        return out

    @staticmethod
    def simplify_grid(aabb_min, aabb_max, n):
        """The cell grid `simplify=N` and build/mesh --simplify N lay over a box: (origin, cell, dims) with origin = aabb_min, cell = the longest edge / N (computed in
        double precision, rounded to float32) and dims = N on every axis, N = 1 .. 1024 (N^3 cells is the call's cap). build/mesh's box is the scene's cube; on a box
        that is not a cube the cells stay cubes, so the grid reaches past the box on its shorter axes (cells that stay empty cost one bit each)."""
        n = int(n)
        if not 1 <= n or n ** 3 > _abi.MESH_SIMPLIFY_MAX_CELLS:
            raise ValueError("simplify must be 1 .. 1024")
        lo = np.asarray(aabb_min, np.float32).astype(np.float64)
        hi = np.asarray(aabb_max, np.float32).astype(np.float64)
        cell = np.float32((hi - lo).max() / n)
        if not (np.isfinite(cell) and cell > 0):
            raise ValueError("the box must have a positive, finite extent")
        return tuple(float(x) for x in lo), float(cell), (n, n, n)

    def _simplify_options(self, origin, cell, dims, placement):
        placements = {"quadric": _abi.MESH_PLACE_QUADRIC, "mean": _abi.MESH_PLACE_MEAN}
        if placement not in placements:
            raise ValueError("placement must be 'quadric' or 'mean'")
        opt = _abi.MeshSimplifyOptions()
        self._check(self.f.mesh_simplify_default_options(C.byref(opt)))
        opt.origin[:] = [float(x) for x in origin]
        opt.cell = float(cell)
        opt.dims[:] = [int(dims)] * 3 if np.isscalar(dims) else [int(x) for x in dims]
        opt.placement = placements[placement]
        return opt

    def simplify_mesh(self, verts, indices, colors=None, normals=None, origin=(0.0, 0.0, 0.0), cell=1.0 / 256.0, dims=256, placement="quadric", stream=None):
        """rnb_mesh_simplify (include/rnb_mesh_simplify.h) on a host mesh: verts float32[n,3], indices uint32[m] (or [m/3,3]), optional per-vertex colors / normals.
        Vertex clustering on the grid of dims (int or 3 ints) cells of edge `cell` from `origin`: the used vertices of a cell become one vertex, placed by
        placement="quadric" (the regularised minimiser of the squared distances to the planes of the triangles that touch the cell, kept inside the cell) or "mean";
        colours are averaged, normals summed and normalised; triangles that lose a corner are dropped, the others keep order and winding. Bit-reproducible. Returns a
        dict of numpy arrays like clean_mesh, with `stats` = `simplify_stats` (counts, n_clamped, n_fallback, peak_workspace, ms). Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            simplified = m.simplify(origin, cell, dims, placement, stream)
        with simplified:
            out = simplified.download()
            out["stats"] = out["simplify_stats"] = simplified.stats
        return out

    def _distance_options(self, level=1, max_distance=0.0, unit=2.0 ** -10, thresholds=(), cells=0):
        thresholds = [float(x) for x in thresholds]
        if len(thresholds) > _abi.MESH_DISTANCE_MAX_TAUS:
            raise ValueError("at most %d thresholds" % _abi.MESH_DISTANCE_MAX_TAUS)
        if any(not x > 0 for x in thresholds):
            raise ValueError("a threshold must be > 0 (0 marks an unused slot of the C-ABI)")
        opt = _abi.MeshDistanceOptions()
        self._check(self.f.mesh_distance_default_options(C.byref(opt)))
        if not 0 <= int(level) <= _abi.MESH_DISTANCE_MAX_LEVEL or not 0 <= int(cells) <= _abi.MESH_DISTANCE_MAX_CELLS:
            raise ValueError("level must be 0 .. 3 and cells 0 .. 256")
        opt.level, opt.max_distance, opt.unit, opt.cells = int(level), float(max_distance), float(unit), int(cells)
        opt.tau[:len(thresholds)] = thresholds
        return opt

    def mesh_distance(self, a_verts, a_indices, b_verts, b_indices, level=1, max_distance=0.0, unit=2.0 ** -10, thresholds=(), cells=0, per_vertex=False, symmetric=False,
                      stream=None):
        """rnb_mesh_distance (include/rnb_mesh_distance.h) on two host meshes (verts float32[n,3], indices uint32[m] or [m/3,3]): the one-sided distance from the surface
        of A to the surface of B. A is sampled at the centroids of the 4^level congruent sub-triangles of each of its triangles, each weighted with its area; the
        distance of a sample is that to the nearest point of B (exact point-triangle distances in double precision), capped at max_distance when that is not 0.
        Returns a dict: `mean` (area-weighted mean distance), `rms`, `max` (over the samples and A's used vertices), `within` (per threshold, the area fraction of A
        with d <= threshold), all in the units of the coordinates; `quantisation`, the bound by which the fixed-point truncation of rule 5 can have lowered `mean`
        (n_samples * 2^-48 / area * unit); and the raw sums and counts of rnb_mesh_distance_stats (sum_w, sum_wd, sum_wd2, sum_within in 2^-48 fixed point with
        distances in `unit`; n_samples, n_beyond, the grid, n_pairs, ms). `unit` only scales the sums: choose it near the expected distances (the call refuses
        w * (d / unit)^2 >= 2^12). `cells` (0 = automatic) changes the time, never a bit of the result. per_vertex=True adds `vert_dist` float32[n] and
        `vert_nearest` uint32[n] (the nearest triangle of B, 0xFFFFFFFF for an unused vertex or one beyond max_distance).
        symmetric=True runs B -> A as well (its dict under `reverse`) and adds `chamfer` = mean(A->B) + mean(B->A) (the sum of the two means of unsquared
        distances, not halved), `hausdorff` = the larger of the two maxima, and per threshold `fscore` = 2 P R / (P + R) with precision P = within(A->B) and
        recall R = within(B->A): A is the reconstruction, B the reference. Bit-reproducible. Leaves the training state as it was."""
        with self.upload_mesh(a_verts, a_indices) as a, self.upload_mesh(b_verts, b_indices) as b:
            return a.distance_to(b, level, max_distance, unit, thresholds, cells, per_vertex, symmetric, stream)

    def _raster_options(self, near, cull, shading):
        culls = {"none": _abi.MESH_RASTER_CULL_NONE, "back": _abi.MESH_RASTER_CULL_BACK, "front": _abi.MESH_RASTER_CULL_FRONT}
        shadings = {"face": _abi.MESH_RASTER_NORMALS_FACE, "vertex": _abi.MESH_RASTER_NORMALS_VERTEX}
        if cull not in culls:
            raise ValueError("cull must be 'none', 'back' or 'front'")
        if shading not in shadings:
            raise ValueError("shading must be 'face' or 'vertex'")
        opt = _abi.MeshRasterOptions()
        self._check(self.f.mesh_raster_default_options(C.byref(opt)))
        opt.near, opt.cull, opt.normals = float(near), culls[cull], shadings[shading]
        return opt

    def rasterize_mesh(self, verts, indices, view, colors=None, normals=None, near=2.0 ** -10, cull="none", shading="face", faces=False, stream=None):
        """rnb_mesh_raster (include/rnb_mesh_raster.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3], optional per-vertex colors / normals) and one
        camera (a view dict as set_dataset and render take). Returns a dict: `image` float32 [H,W,9] in the channel layout of the render (0-2 unit normal in the world
        frame, 3-5 colour or ones, 6 coverage, 7 camera-forward depth, 8 the number of triangles over the pixel's centre), with faces=True `faces` uint32 [H,W] (the
        winning triangle, 0xFFFFFFFF where nothing covers), and beside them the fields of rnb_mesh_raster_stats (n_tris, n_behind, ..., n_fragments, peak_workspace, ms), as mesh_distance returns its own. cull: "none", "back" or "front"; shading:
        "face" (the triangle's own normal) or "vertex" (the interpolated `normals`, which must then be given). Coverage is exact on 1/256-pixel snapped vertices, a pixel
        centre on a shared edge belongs to exactly one triangle; a triangle with a vertex nearer than `near` is skipped and counted, not clipped. Bit-reproducible.
        Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            return m.rasterize(view, near, cull, shading, faces, stream)

    def _draw_options(self, near, cull, shading, filter):
        ro = self._raster_options(near, cull, shading)
        filters = {"nearest": _abi.MESH_DRAW_FILTER_NEAREST, "bilinear": _abi.MESH_DRAW_FILTER_BILINEAR}
        if filter not in filters:
            raise ValueError("filter must be 'nearest' or 'bilinear'")
        opt = _abi.MeshDrawOptions()
        self._check(self.f.mesh_draw_default_options(C.byref(opt)))
        opt.near, opt.cull, opt.normals, opt.filter = ro.near, ro.cull, ro.normals, filters[filter]
        return opt

    def draw_textured_mesh(self, verts, indices, view, uv, color=None, normal=None, normals=None, colors=None, near=2.0 ** -10, cull="none", shading="face", filter="bilinear",
                           faces=False, stream=None):
        """rnb_mesh_draw_textured (include/rnb_mesh_draw.h) on a host mesh and one camera: DeviceMesh.draw_textured, which describes every argument and key, on an upload of
        (verts, indices, colors, normals) that is released before the call returns."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            return m.draw_textured(view, uv, color, normal, near, cull, shading, filter, faces, stream)

    def mesh_view_metrics(self, verts, indices, views, normal_maps, normals=None, near=2.0 ** -10, cull="none", shading="face", stream=None, texture=None, albedo_maps=None):
        """The mesh's counterpart of build/render's render_metrics.json: the mesh rasterised into every view of `views` (rasterize_mesh) and compared with that view's
        input normal map (`normal_maps`: uint16 [h,w,4] each) by view_normal_metrics. Returns dict(views=[one dict per view: mean_angle_deg, median_angle_deg, mask_iou,
        pixels_compared, n_back_pixels, odd_count_pixels (pixels an odd number of triangles cover: 0 for a closed mesh), ms], mean={the means of the first three}).
        texture=dict(uv=, color=, normal=) (color or normal may be missing or None): every view is drawn with DeviceMesh.draw_textured instead, the texture uploaded once,
        so the normal numbers describe the normal-mapped surface. albedo_maps (one uint16 or uint8 [h,w,4] per view; needs a texture with a colour map): the per-view dict
        also carries albedo_mae, albedo_rmse and albedo_psnr_db of view_albedo_metrics, and `mean` their means. With neither the call is what it was."""
        if len(views) != len(normal_maps):
            raise ValueError("one normal map per view")
        self._raster_options(near, cull, shading)  # a bad argument fails before anything is uploaded, and with no view at all
        if shading == "vertex" and normals is None:
            raise ValueError("shading='vertex' needs normals")
        if albedo_maps is not None and (texture is None or texture.get("color") is None):
            raise ValueError("albedo_maps need a texture with a colour map")
        if albedo_maps is not None and len(albedo_maps) != len(views):
            raise ValueError("one albedo map per view")
        per_view, keys, own = [], ["mean_angle_deg", "median_angle_deg", "mask_iou"], []
        with self.upload_mesh(verts, indices, None, normals) as m:
            try:
                if texture is not None:
                    opt = self._draw_options(near, cull, shading, "bilinear")
                    tex = m._upload_texture(texture["uv"], texture.get("color"), texture.get("normal"), own)
                for k, (view, nm) in enumerate(zip(views, normal_maps)):
                    r = m.rasterize(view, near, cull, shading, stream=stream) if texture is None else m._draw(tex, view, opt, False, stream, None)
                    e = view_normal_metrics(r["image"], view, nm)
                    if albedo_maps is not None:
                        a = view_albedo_metrics(r["image"], view, albedo_maps[k])
                        e.update(albedo_mae=a["albedo_mae"], albedo_rmse=a["albedo_rmse"], albedo_psnr_db=a["albedo_psnr_db"])
                    e.update(n_back_pixels=r["n_back_pixels"], odd_count_pixels=int((r["image"][..., 8].astype(np.int64) & 1).sum()), ms=r["ms"])
                    per_view.append(e)
            finally:
                for p in own:
                    self.device_free(p)
        if albedo_maps is not None:
            keys += ["albedo_mae", "albedo_rmse", "albedo_psnr_db"]
        k = max(len(per_view), 1)
        return dict(views=per_view, mean={key: sum(e[key] for e in per_view) / k for key in keys})

    def _visibility_options(self, near, cull, min_pixels):
        culls = {"none": _abi.MESH_RASTER_CULL_NONE, "back": _abi.MESH_RASTER_CULL_BACK, "front": _abi.MESH_RASTER_CULL_FRONT}
        if cull not in culls:
            raise ValueError("cull must be 'none', 'back' or 'front'")
        if int(min_pixels) < 1:
            raise ValueError("min_pixels must be at least 1")
        opt = _abi.MeshVisibilityOptions()
        self._check(self.f.mesh_visibility_default_options(C.byref(opt)))
        opt.near, opt.cull, opt.min_pixels = float(near), culls[cull], int(min_pixels)
        return opt

    @staticmethod
    def _visibility_views(views, masks, supersample):
        """The host array of rnb_mesh_visibility_view for `views` (each through scaled_view(view, supersample) when that is not 1), the masks not yet attached."""
        views = list(views)
        if not views:
            raise ValueError("at least one view")
        if masks is not None and len(masks) != len(views):
            raise ValueError("one mask (or None) per view")
        for mk in masks or ():
            if mk is not None and (np.ndim(mk) != 2 or 0 in np.shape(mk)):
                raise ValueError("a mask must be a non-empty 2-D array")
        k = int(supersample)
        if k != supersample or k < 1:
            raise ValueError("supersample must be a positive integer")
        if k != 1:
            views = [scaled_view(v, k) for v in views]
        if any(max(int(v["width"]), int(v["height"])) > _abi.MESH_RASTER_MAX_SIZE for v in views):
            raise ValueError("a view times supersample exceeds %d pixels per side" % _abi.MESH_RASTER_MAX_SIZE)
        arr = (_abi.MeshVisibilityView * len(views))()
        for e, v in zip(arr, views):
            e.view = _view_struct(v)
        return arr

    def _visibility_select_options(self, unit, min_views, max_off_mask, rings):
        units = {"component": _abi.MESH_VISIBILITY_UNIT_COMPONENT, "face": _abi.MESH_VISIBILITY_UNIT_FACE, "faces": _abi.MESH_VISIBILITY_UNIT_FACE}
        if unit not in units:
            raise ValueError("unit must be 'component' or 'face'")
        if not 0 <= int(rings) <= _abi.MESH_VISIBILITY_MAX_RINGS:
            raise ValueError("rings must be 0 .. %d" % _abi.MESH_VISIBILITY_MAX_RINGS)
        if int(min_views) < 0 or (max_off_mask is not None and int(max_off_mask) < 0):
            raise ValueError("min_views and max_off_mask must not be negative")
        opt = _abi.MeshVisibilitySelectOptions()
        self._check(self.f.mesh_visibility_select_default_options(C.byref(opt)))
        opt.unit, opt.min_views_seen, opt.rings = units[unit], int(min_views), int(rings)
        opt.max_views_off_mask = 0xFFFFFFFF if max_off_mask is None else min(int(max_off_mask), 0xFFFFFFFF)
        return opt

    def mesh_visibility(self, verts, indices, views, masks=None, near=2.0 ** -10, cull="none", min_pixels=1, supersample=1, stream=None):
        """rnb_mesh_visibility (include/rnb_mesh_visibility.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]) and a list of cameras (view dicts as
        rasterize_mesh takes one): what the cameras see, per triangle, counted on the device over all views in one call. Returns (records, stats): `records` a numpy
        structured array, one per triangle in the mesh's order, of n_drawn (views that draw it), n_seen (views in which it wins at least min_pixels pixels: the
        rasteriser's winner of a pixel, the nearest triangle over its centre), n_off_mask (views in which less than half of the pixel centres it covers are on the
        mask), best_view (the view in which it wins the most pixels, 0xFFFFFFFF if none), best_pixels, n_pixels_won, n_pixels_covered; `stats` the dict of
        rnb_mesh_visibility_stats (the rasteriser's class counts summed over the views, n_faces_seen, n_faces_off_mask, n_pixels, peak_workspace, ms).
        masks: None, or per view None or a 2-D array, non-zero = object, of any resolution (a view pixel reads the mask pixel whose area holds its centre). near, cull: as
        rasterize_mesh. supersample=k: every view goes through scaled_view(view, k), the masks stay as given. All integers: bit-reproducible. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices) as m:
            return m.visibility(views, masks, near, cull, min_pixels, supersample, stream=stream)

    def cull_unseen_mesh(self, verts, indices, views, masks=None, colors=None, normals=None, unit="component", min_views=1, max_off_mask=None, rings=1, near=2.0 ** -10, cull="none",
                         min_pixels=1, supersample=1, stream=None):
        """A host mesh without what the cameras do not see: rnb_mesh_visibility, then rnb_mesh_visibility_select (include/rnb_mesh_visibility.h). A triangle is a
        candidate if it lies off the mask in at most max_off_mask views (None: the masks carve nothing) and a seed if it is a candidate that at least min_views views
        see. unit="component" (the default): the connected components are those of clean_mesh, and the candidates of every component that holds a seed are kept -- a
        cavity shell inside the object goes, closed surfaces stay closed, a second object any camera saw stays. unit="face": the seeds and, `rings` times, every candidate
        that shares a vertex with a kept triangle; a side of a closed surface that no camera saw becomes a hole. Returns a dict of numpy arrays like clean_mesh (verts,
        indices, colors / normals when given, in the input's order), `kept` uint32[n_triangles] (1 for a kept triangle of the input), `stats` (the select stats) and
        `visibility_stats`. The other arguments are those of mesh_visibility. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, colors, normals) as m:
            culled, rep = m.cull_unseen(views, masks, unit, min_views, max_off_mask, rings, near, cull, min_pixels, supersample, stream, report=True)
        with culled:
            out = culled.download()
            out.update(kept=rep["kept"], stats=rep["select"], visibility_stats=rep["visibility"])
        return out

    def _texture_options(self, size, block, maps, inference, max_texels_in_flight):
        if isinstance(maps, str):
            maps = (maps,)
        if not isinstance(maps, int):
            unknown = [m for m in maps if m not in _abi.MESH_TEXTURE_MAPS]
            if unknown:
                raise ValueError("maps must be of 'albedo', 'normal' and 'position'")
            maps = sum(_abi.MESH_TEXTURE_MAPS[m] for m in set(maps))
        opt = _abi.MeshTextureOptions()
        self._check(self.f.mesh_texture_default_options(C.byref(opt)))
        opt.size, opt.block, opt.maps = int(size), int(block), int(maps)
        opt.use_inference_params = int(bool(inference))
        opt.max_texels_in_flight = int(max_texels_in_flight)
        return opt

    @staticmethod
    def texture_layout(n_tris, size, block=0, fns=None):
        """rnb_mesh_texture_layout (include/rnb_mesh_texture.h): the atlas bake_texture lays out for n_tris triangles in a texture of `size` texels per side, as a dict of
        `block` (the block edge in texels; block=0 asks for the largest that holds the mesh), `blocks_per_row` and `n_blocks` (block k holds the triangles 2k and 2k + 1).
        A mesh that does not fit raises RnbError with ERR_INVALID; its message ends in the smallest size that would. A host function: it needs no context and no GPU."""
        f = fns or load_library()
        b, bpr, nb = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = f.mesh_texture_layout(int(n_tris), int(size), int(block), C.byref(b), C.byref(bpr), C.byref(nb))
        if rc != 0:
            raise RnbError(rc, f.last_error().decode(errors="replace"))
        return dict(block=b.value, blocks_per_row=bpr.value, n_blocks=nb.value)

    def bake_texture(self, verts, indices, size, block=0, maps=("albedo",), inference=True, max_texels_in_flight=0, stream=None):
        """rnb_mesh_bake_texture (include/rnb_mesh_texture.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3]): a per-triangle UV atlas of `size` texels
        per side -- two triangles to a square block of `block` texels (0: the largest that holds the mesh, see texture_layout), laid out so that a bilinear lookup inside
        a triangle reads only that triangle's texels -- and the model sampled at every texel. Returns a dict: `uv` float32[nt,3,2] (U, V of the corners of every
        triangle, in the order of its indices; V = 1 at the top row), one float32[S,S,4] per name in `maps` -- `albedo` (the logistic of the colour head), `normal` (the
        normalised SDF gradient, zeros for a zero gradient), `position` (the texel's point on the triangle's plane) in channels 0-2, channel 3 = 1 on the texels of a
        triangle, all zeros elsewhere; row 0 is the top row of an image file -- and `block`, `blocks_per_row`, `stats` (n_texels, n_batches, peak_workspace, ms).
        inference: the EMA weights; max_texels_in_flight (0 = 2^20) bounds the workspace and does not change a bit. The texels along an edge two triangles share are
        equal bit for bit in both; a corner texel holds what extract_mesh(colors=True, normals=True) gives the vertex. meshproc.save_obj_textured writes the result as
        OBJ + MTL + PNG. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices) as m:
            return m.bake_texture(size, block, maps, inference, max_texels_in_flight, stream)

    def _project_options(self, size, block, mode, normals, weight_power, min_cos, depth_tolerance, near, cull):
        modes = {"blend": _abi.MESH_PROJECT_MODE_BLEND, "best": _abi.MESH_PROJECT_MODE_BEST}
        kinds = {"face": _abi.MESH_PROJECT_NORMALS_FACE, "vertex": _abi.MESH_PROJECT_NORMALS_VERTEX}
        culls = {"none": _abi.MESH_RASTER_CULL_NONE, "back": _abi.MESH_RASTER_CULL_BACK, "front": _abi.MESH_RASTER_CULL_FRONT}
        if mode not in modes:
            raise ValueError("mode must be 'blend' or 'best'")
        if normals not in kinds:
            raise ValueError("normals must be None, 'face' or 'vertex'")
        if cull not in culls:
            raise ValueError("cull must be 'none', 'back' or 'front'")
        if int(weight_power) != weight_power or not 0 <= int(weight_power) <= _abi.MESH_PROJECT_MAX_WEIGHT_POWER:
            raise ValueError("weight_power must be an integer 0 .. %d" % _abi.MESH_PROJECT_MAX_WEIGHT_POWER)
        if not 0.0 <= float(min_cos) < 1.0:
            raise ValueError("min_cos must be in [0, 1)")
        if not (float(depth_tolerance) >= 0.0 and math.isfinite(float(depth_tolerance))):
            raise ValueError("depth_tolerance must be finite and not negative")
        opt = _abi.MeshProjectOptions()
        self._check(self.f.mesh_project_default_options(C.byref(opt)))
        opt.size, opt.block, opt.mode, opt.normals, opt.weight_power = int(size), int(block), modes[mode], kinds[normals], int(weight_power)
        opt.min_cos, opt.depth_tolerance, opt.near, opt.cull = float(min_cos), float(depth_tolerance), float(near), culls[cull]
        return opt

    @staticmethod
    def _project_views(views, images):
        """The host array of rnb_mesh_project_view for `views` and, per view, its image as a contiguous [h, w, 4] array of float32, uint16 or uint8 (a 3-channel image gets
        alpha 1: 1.0, 65535 or 255), not yet uploaded."""
        views, images = list(views), list(images)
        if not views:
            raise ValueError("at least one view")
        if len(images) != len(views):
            raise ValueError("one image per view")
        arrays = []
        for im in images:
            a = np.asarray(im)
            if a.dtype.name not in _abi.MESH_PROJECT_FORMATS:
                raise ValueError("an image must be of dtype float32, uint16 or uint8")
            if a.ndim != 3 or a.shape[2] not in (3, 4) or 0 in a.shape:
                raise ValueError("an image must be a non-empty [h, w, 4] (or [h, w, 3]) array")
            if a.shape[2] == 3:
                one = 1.0 if a.dtype == np.float32 else np.iinfo(a.dtype).max
                a = np.concatenate([a, np.full(a.shape[:2] + (1,), one, a.dtype)], axis=2)
            arrays.append(np.ascontiguousarray(a))
        if any(max(int(v["width"]), int(v["height"])) > _abi.MESH_RASTER_MAX_SIZE for v in views):
            raise ValueError("a view exceeds %d pixels per side" % _abi.MESH_RASTER_MAX_SIZE)
        arr = (_abi.MeshProjectView * len(views))()
        for e, v, a in zip(arr, views, arrays):
            e.view = _view_struct(v)
            e.image_height, e.image_width, e.format = a.shape[0], a.shape[1], _abi.MESH_PROJECT_FORMATS[a.dtype.name]
        return arr, arrays

    def project_views(self, verts, indices, views, images, normals=None, size=1024, block=0, mode="blend", shading=None, weight_power=2, min_cos=0.1, depth_tolerance=2.0 ** -8,
                      near=2.0 ** -10, cull="none", fallback=None, inference=True, stream=None):
        """rnb_mesh_project_views (include/rnb_mesh_project.h) on a host mesh (verts float32[n,3], indices uint32[m] or [m/3,3], optional per-vertex `normals`): the atlas of
        bake_texture (same `size` and `block`, the same `uv`, bit for bit) with every texel coloured from the input images -- projected into each camera of `views` (view
        dicts as rasterize_mesh takes one), skipped where the view looks at it at a flatter angle than min_cos or where the mesh itself is in front of it by more than the
        relative depth_tolerance (the rasteriser's nearest surface of the pixel that holds the projection), sampled bilinearly with alpha as the mask, and blended with
        the weight cos^weight_power * alpha (mode="blend") or taken from the view of the greatest such weight (mode="best").
        images: one per view, numpy [h, w, 4] (or [h, w, 3]: alpha 1) of dtype float32, uint16 (x / 65535) or uint8 (x / 255), of any resolution, row 0 on top; the values
        are blended as stored. shading: "face" or "vertex" -- which normal weights a view; None: "vertex" when normals are given, else "face".
        fallback: None, "model" (the model's albedo baked with the same size and block, see bake_texture; `inference` picks its weights) or a float32 [S, S, 4] array:
        what an owned texel no view contributes to gets; without one it is (0, 0, 0, 1).
        Returns a dict: `uv` float32[nt,3,2], `color` float32[S,S,4] (alpha 1 on the texels of a triangle, zeros elsewhere), `info` uint32[S,S,2] (the number of
        contributing views and the best view, 0xFFFFFFFF if none), `block`, `blocks_per_row` and `stats` (n_texels, n_textured, n_pairs_tested, n_occluded,
        peak_workspace, ms). Reads nothing of the model (but for fallback="model"): any mesh, any calibrated images. Bit-reproducible. meshproc.save_obj_textured
        writes `color` as the albedo map. Leaves the training state as it was."""
        with self.upload_mesh(verts, indices, normals=normals) as m:
            return m.project_views(views, images, size, block, mode, shading, weight_power, min_cos, depth_tolerance, near, cull, fallback, inference, stream)

    def upload(self, array):
        """numpy array -> library-side buffer (device_malloc + copy); release with device_free."""
        a = np.ascontiguousarray(array)
        ptr = self.device_malloc(a.nbytes)
        self._check(self.f.memcpy(self._h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, _abi.H2D))
        return ptr

    def download(self, ptr, count, dtype):
        out = np.empty(int(count), dtype=dtype)
        self._check(self.f.memcpy(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, _abi.D2H))
        return out

    def forward_infer_staged(self, n, stream=None):
        """Evaluate the first n samples already in COORDS into MLP_OUT (what train_nerf_step does, testbed_nerf.cu:3967)."""
        cptr, _ = self.buffer("COORDS")
        optr, _ = self.buffer("MLP_OUT")
        self._check(self.f.forward_infer(self._h, _stream_handle(stream), C.c_void_p(cptr), int(n), C.c_void_p(optr), 0))

    def generate_training_samples(self, n_rays, n_rays_total=0, max_samples=None, stream=None):
        if max_samples is None:
            max_samples = self.cfg.target_batch_size * 16
        self._check(self.f.generate_training_samples(self._h, _stream_handle(stream), int(n_rays), int(n_rays_total), int(max_samples)))

    def compute_loss(self, n_rays, n_rays_total=0, stream=None):
        self._check(self.f.compute_loss(self._h, _stream_handle(stream), int(n_rays), int(n_rays_total)))

    def forward_backward(self, stream=None):
        self._check(self.f.forward_backward(self._h, _stream_handle(stream)))

    def optimizer_step(self, stream=None):
        self._check(self.f.optimizer_step(self._h, _stream_handle(stream)))

    def train_step(self, stream=None, allow_no_samples=False):
        st = StepStats()
        rc = self.f.train_step(self._h, _stream_handle(stream), C.byref(st))
        self._check(rc, allow=(_abi.ERR_NO_SAMPLES,) if allow_no_samples else ())
        return st

    def train_step_begin(self, stream=None):
        self._check(self.f.train_step_begin(self._h, _stream_handle(stream)))

    def train_step_apply(self, stream=None):
        self._check(self.f.train_step_apply(self._h, _stream_handle(stream)))

    def train_step_local(self, stream=None):
        """(counters uint64[4], loss_sums float64[3]) of this rank for the step just applied."""
        cnt = (C.c_uint64 * 4)()
        sums = (C.c_double * 3)()
        self._check(self.f.train_step_local(self._h, _stream_handle(stream), cnt, sums))
        return np.array(cnt, dtype=np.uint64), np.array(sums, dtype=np.float64)

    def train_step_finish(self, counters, loss_sums, allow_no_samples=False):
        cnt = (C.c_uint64 * 4)(*[int(x) for x in counters])
        sums = (C.c_double * 3)(*[float(x) for x in loss_sums])
        st = StepStats()
        rc = self.f.train_step_finish(self._h, cnt, sums, C.byref(st))
        self._check(rc, allow=(_abi.ERR_NO_SAMPLES,) if allow_no_samples else ())
        return st

    def train_step_end(self, stream=None, allow_no_samples=False):
        st = StepStats()
        rc = self.f.train_step_end(self._h, _stream_handle(stream), C.byref(st))
        self._check(rc, allow=(_abi.ERR_NO_SAMPLES,) if allow_no_samples else ())
        return st

def _returned_mesh(ctx, stats, call):
    """One C call that fills a new rnb_mesh (`call(byref(mesh))` returns its status) -> the DeviceMesh that owns it, with `stats` as its dict."""
    out = DeviceMesh(ctx)
    try:
        ctx._check(call(C.byref(out)))
    except BaseException:
        out.free()  # (whatever a failed call left goes the way of a returned mesh)
        raise
    out._stats = stats.as_dict()
    return out


class DeviceMesh(_abi.Mesh):
    """A mesh whose buffers are in device memory: the rnb_mesh of the C-ABI (it is the struct, so C.byref(m) goes to a raw call) together with the Context it belongs to, which
    therefore cannot be collected first. Context.upload_mesh and Context.extract_mesh_device make one; clean and simplify return a new one and leave theirs as it was;
    distance_to and rasterize measure; download brings the arrays to the host. Nothing visits the host in between.
    `with m:` or m.free() releases the buffers, once: rnb_mesh_free for a mesh a stage returned, one device_free per buffer for an uploaded one. After that every method
    raises ValueError before any call into the library. Free the meshes of a context before closing it: free() after Context.close() does nothing (the context's memory is
    gone with it)."""

    def __init__(self, ctx, buffers=None):
        super().__init__()
        self.ctx, self._buffers, self._stats, self._freed = ctx, buffers, None, False
        self._table, self._table_host = C.c_void_p(), None
        self.vertex_map = None  # set by repair(vertex_map=True) on the mesh it returns
        self.loop_of_tri = None  # set by fill_holes(loop_of_tri=True) on the mesh it returns
        self.displacement = self.valence = self.kind = None  # set by smooth(displacement=True / census=True) on the mesh it returns
        self.residual_before = self.residual_after = self.state = None  # set by snap(residuals=True / states=True) on the mesh it returns (displacement=True: `displacement`)

    n_verts = property(lambda self: _abi.Mesh.n_verts.__get__(self))
    n_triangles = property(lambda self: self.n_indices // 3)
    has_colors = property(lambda self: bool(self.colors))
    has_normals = property(lambda self: bool(self.normals))
    stats = property(lambda self: self._stats, doc="The stats dict of the call that produced the mesh (rnb_mesh_stats, rnb_mesh_clean_stats, rnb_mesh_simplify_stats); None for an upload.")

    def _live(self):
        if self._freed:
            raise ValueError("the device mesh has been freed")
        return self.ctx

    def free(self):
        """Release the device buffers; a second call, or one after the context was closed, does nothing."""
        if self._freed:
            return
        self._freed = True
        c = self.ctx
        if not c._h.value:
            return
        if self._buffers is not None:
            for p in self._buffers:
                c.device_free(p)
            C.memset(C.byref(self), 0, C.sizeof(_abi.Mesh))
        else:
            c.f.mesh_free(c._h, C.byref(self))
            if self._table:
                c.f.mesh_clean_table_free(c._h, self._table)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __enter__(self):
        self._live()
        return self

    def __exit__(self, *a):
        self.free()

    def download(self):
        """-> dict of numpy arrays: verts float32[n,3], indices uint32[m], colors / normals float32[n,3] when the mesh has them."""
        c = self._live()
        out = dict(verts=c.download(self.verts, self.n_verts * 3, np.float32).reshape(-1, 3) if self.n_verts else np.empty((0, 3), np.float32),
                   indices=c.download(self.indices, self.n_indices, np.uint32) if self.n_indices else np.empty(0, np.uint32))
        for key, ptr in (("colors", self.colors), ("normals", self.normals)):
            if ptr:
                out[key] = c.download(ptr, self.n_verts * 3, np.float32).reshape(-1, 3) if self.n_verts else np.empty((0, 3), np.float32)
        return out

    def clean(self, keep="largest", orient="outward", table=False, stream=None):
        """rnb_mesh_clean (see Context.clean_mesh) -> the cleaned DeviceMesh; its `stats` are the clean stats. With table=True the component table is made as well and stays
        on the device beside the mesh, released with it; `table` reads it."""
        c = self._live()
        opt, st, tab = c._clean_options(keep, orient), _abi.MeshCleanStats(), C.c_void_p()
        out = _returned_mesh(c, st, lambda m: c.f.mesh_clean(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), m, C.byref(tab) if table else None, C.byref(st)))
        out._table = tab
        return out

    @property
    def table(self):
        """After clean(table=True): one record per component (label, n_vertices, n_triangles, kept, area_q, volume_q), ascending label, as a numpy record array -- downloaded
        when first read, so read it before the mesh is freed. None for any other mesh."""
        if self._table_host is None and self._table:
            dt, n = np.dtype(_abi.MESH_COMPONENT_DTYPE), self._stats["n_components"]
            self._table_host = self._live().download(self._table.value, n, dt) if n else np.empty(0, dt)
        return self._table_host

    def simplify(self, origin, cell, dims, placement="quadric", stream=None):
        """rnb_mesh_simplify on the grid of dims cells of edge `cell` from `origin` (see Context.simplify_mesh; Context.simplify_grid lays one over a box) -> the simplified
        DeviceMesh; its `stats` are the simplify stats."""
        c = self._live()
        opt, st = c._simplify_options(origin, cell, dims, placement), _abi.MeshSimplifyStats()
        return _returned_mesh(c, st, lambda m: c.f.mesh_simplify(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), m, C.byref(st)))

    def topology(self, edges=False, table=False, buckets_log2=0, stream=None):
        """rnb_mesh_topology (include/rnb_mesh_topology.h): the edge census of the mesh -> the dict of rnb_mesh_topology_stats (n_edges, n_boundary_edges,
        n_nonmanifold_edges, n_inconsistent_edges, n_duplicate_tris, n_folded_pairs, n_components, n_patches, n_unorientable_patches, n_boundary_components, euler,
        closed, oriented, ...). edges=True adds `n_faces`, `n_same` and `mate`, uint32[n_indices] per half-edge h = 3t + k (mate 0xFFFFFFFF where the edge is not
        shared by exactly two faces); table=True adds `table`, one record per component (label, n_vertices, n_edges, n_triangles, n_boundary_edges,
        n_nonmanifold_edges, n_inconsistent_edges, n_patches, euler, genus), ascending label. Nothing of the mesh changes; vertex-manifoldness is not examined."""
        c = self._live()
        opt, st, tab = c._topology_options(buckets_log2), _abi.MeshTopologyStats(), C.c_void_p()
        n = max(self.n_indices, 1) * 4
        arrays = []
        try:
            for _ in range(3 if edges else 0):
                arrays.append(c.device_malloc(n))
            ptrs = arrays if edges else [None] * 3
            try:
                c._check(c.f.mesh_topology(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), ptrs[0], ptrs[1], ptrs[2], C.byref(tab) if table else None, C.byref(st)))
                out = st.as_dict()
                if edges:
                    for key, p in zip(("n_faces", "n_same", "mate"), arrays):
                        out[key] = c.download(p, self.n_indices, np.uint32) if self.n_indices else np.empty(0, np.uint32)
                if table:
                    dt = np.dtype(_abi.MESH_TOPOLOGY_COMPONENT_DTYPE)
                    out["table"] = c.download(tab.value, st.n_components, dt) if st.n_components else np.empty(0, dt)
            finally:
                if tab:
                    c.f.mesh_topology_table_free(c._h, tab)
        finally:
            for p in arrays:
                c.device_free(p)
        return out

    def repair(self, weld=False, drop_degenerate=True, duplicates="first", orient="none", vertex_map=False, buckets_log2=0, stream=None):
        """rnb_mesh_repair (include/rnb_mesh_topology.h) -> the repaired DeviceMesh; its `stats` are the repair stats. In this order: weld (used vertices at one
        position become the lowest-indexed of them), drop_degenerate, duplicates ("keep" / "first": the lowest-numbered triangle of a vertex set stays / "cancel":
        opposite windings cancel, a folded pair goes entirely), orient ("none" / "consistent": every orientable patch is wound consistently across its manifold edges
        by the smaller set of flips). vertex_map=True: `vertex_map` of the returned mesh is uint32[n_verts of this mesh], each input vertex's output index or 0xFFFFFFFF."""
        c = self._live()
        opt, st = c._repair_options(weld, drop_degenerate, duplicates, orient, buckets_log2), _abi.MeshRepairStats()
        vmap = c.device_malloc(max(self.n_verts, 1) * 4) if vertex_map else None
        try:
            out = _returned_mesh(c, st, lambda m: c.f.mesh_repair(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), m, vmap, C.byref(st)))
            if vertex_map:
                try:
                    out.vertex_map = c.download(vmap, self.n_verts, np.uint32) if self.n_verts else np.empty(0, np.uint32)
                except BaseException:
                    out.free()
                    raise
        finally:
            if vmap:
                c.device_free(vmap)
        return out

    def boundary_loops(self, edges=False, table=True, buckets_log2=0, stream=None):
        """rnb_mesh_boundary_loops (include/rnb_mesh_holes.h): the boundary of the mesh as loops -> the dict of rnb_mesh_boundary_loops_stats (n_boundary_edges, n_loops,
        n_simple, n_irregular_vertices, max_loop_edges, n_too_long, ...). table=True (the default) adds `table`, one record per boundary component in ascending label
        (label = its lowest boundary half-edge, n_edges, simple, n_irregular, component, centroid, normal, perimeter, area); edges=True adds `loop`, `next` and `pos`,
        uint32[n_indices] per half-edge h = 3t + k (0xFFFFFFFF off the boundary; next and pos also on a component that is not one simple cycle). Nothing of the mesh changes."""
        c = self._live()
        opt, st, tab = c._boundary_loops_options(buckets_log2), _abi.MeshBoundaryLoopsStats(), C.c_void_p()
        n = max(self.n_indices, 1) * 4
        arrays = []
        try:
            for _ in range(3 if edges else 0):
                arrays.append(c.device_malloc(n))
            ptrs = arrays if edges else [None] * 3
            try:
                c._check(c.f.mesh_boundary_loops(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), ptrs[0], ptrs[1], ptrs[2], C.byref(tab) if table else None, C.byref(st)))
                out = st.as_dict()
                if edges:
                    for key, p in zip(("loop", "next", "pos"), arrays):
                        out[key] = c.download(p, self.n_indices, np.uint32) if self.n_indices else np.empty(0, np.uint32)
                if table:
                    dt = np.dtype(_abi.MESH_BOUNDARY_LOOP_DTYPE)
                    out["table"] = c.download(tab.value, st.n_loops, dt) if st.n_loops else np.empty(0, dt)
            finally:
                if tab:
                    c.f.mesh_boundary_loops_free(c._h, tab)
        finally:
            for p in arrays:
                c.device_free(p)
        return out

    def fill_holes(self, max_edges=0, skip_largest=False, loop_of_tri=False, buckets_log2=0, stream=None):
        """rnb_mesh_fill_holes (include/rnb_mesh_holes.h) -> a new DeviceMesh with every selected simple boundary loop closed; its `stats` are the fill stats. The input's
        vertices and triangles come first, unchanged; a loop of 3 edges gets one triangle, a longer one a fan around a new vertex at its centroid (colour and normal
        the loop's mean colour and normal), loop by loop in ascending label. max_edges=N: only loops of up to N edges (0: all, up to 2^20); skip_largest=True: the
        longest simple loop of every connected component stays open (the rim of a relief). Components that are not one simple cycle are never filled (see
        boundary_loops; repair(orient="consistent") first). loop_of_tri=True: `loop_of_tri` of the returned mesh is uint32[its triangles], the label of the loop a
        triangle closes or 0xFFFFFFFF for an input triangle."""
        c = self._live()
        opt, st = c._fill_holes_options(max_edges, skip_largest, buckets_log2), _abi.MeshFillHolesStats()
        lot = c.device_malloc(max(self.n_triangles + self.n_indices, 1) * 4) if loop_of_tri else None  # (at most one new triangle per boundary half-edge)
        try:
            out = _returned_mesh(c, st, lambda m: c.f.mesh_fill_holes(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), m, lot, C.byref(st)))
            if loop_of_tri:
                try:
                    out.loop_of_tri = c.download(lot, out.n_triangles, np.uint32) if out.n_triangles else np.empty(0, np.uint32)
                except BaseException:
                    out.free()
                    raise
        finally:
            if lot:
                c.device_free(lot)
        return out

    def smooth(self, passes=2, lam=0.5, mu=-0.53, boundary="pin", select=None, select_rings=0, normals="keep", displacement=False, census=False, buckets_log2=0, stream=None):
        """rnb_mesh_smooth (include/rnb_mesh_smooth.h) -> a new DeviceMesh with the same vertices (none added, none removed), triangles and colours, the moving vertices
        relaxed towards the centroids of their one-rings by `passes` passes with the factors lam (odd passes) and mu (even ones; mu=0: lam in every pass, plain Laplacian
        smoothing, which shrinks); its `stats` are the smooth stats. Interior vertices move; boundary vertices stay (boundary="pin"), move along the rim ("slide") or like
        interior ones ("free"); vertices on a non-manifold edge and unused ones never move. select: None (every vertex) or one value per vertex (non-zero = selected), grown
        `select_rings` times over the edges; only selected vertices move. normals="recompute": the returned mesh has the normals of vertex_normals() on it, whether or not
        this mesh has normals ("keep": this mesh's normals, if any, unchanged). displacement=True: `displacement` of the returned mesh is float32[n_verts], how far each
        vertex moved; census=True: `valence` and `kind` (0 unused, 1 interior, 2 boundary, 3 non-manifold) are uint32[n_verts]."""
        c = self._live()
        opt, st = c._smooth_options(passes, lam, mu, boundary, select_rings, normals, buckets_log2), _abi.MeshSmoothStats()
        n = self.n_verts
        if select is not None:
            select = np.ascontiguousarray(np.asarray(select).ravel() != 0, dtype=np.uint32)
            if select.size != n:
                raise ValueError("select must have one value per vertex")
        bufs = {}
        try:
            if select is not None:
                bufs["select"] = c.upload(select) if n else c.device_malloc(4)
            for key in (("valence", "kind") if census else ()) + (("displacement",) if displacement else ()):
                bufs[key] = c.device_malloc(max(n, 1) * 4)
            out = _returned_mesh(c, st, lambda m: c.f.mesh_smooth(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), bufs.get("select"), m, bufs.get("valence"), bufs.get("kind"),
                                                                 bufs.get("displacement"), C.byref(st)))
            try:
                for key, dt in (("valence", np.uint32), ("kind", np.uint32), ("displacement", np.float32)):
                    if key in bufs:
                        setattr(out, key, c.download(bufs[key], n, dt) if n else np.empty(0, dt))
            except BaseException:
                out.free()
                raise
        finally:
            for p_ in bufs.values():
                c.device_free(p_)
        return out

    def snap(self, iterations=3, tolerance=None, max_step=None, max_displacement=None, min_gradient=None, level=0.0, select=None, attributes=(), inference=True,
             max_points_in_flight=0, residuals=False, states=False, displacement=False, stream=None):
        """rnb_mesh_snap (include/rnb_mesh_snap.h) -> a new DeviceMesh with the same vertices (none added, none removed) and triangles, every selected vertex moved
        along the model's SDF gradient towards sdf = level by up to `iterations` guarded Newton steps; its `stats` are the snap stats. A step is at most max_step long, a
        vertex never ends further than max_displacement from where it was (both in world units), stops where the gradient is shorter than min_gradient, where
        |sdf - level| <= tolerance, at the box, and goes back one step if a step made the residual larger (None: the library's default). select: None (every vertex) or
        one value per vertex (non-zero = selected). attributes: "colors" and / or "normals" are resampled from the model at the new positions (for the selected
        vertices; () carries this mesh's). inference: the EMA weights. residuals=True: `residual_before` and `residual_after` of the returned mesh are float32[n_verts],
        sdf - level at the old and the new position; states=True: `state` is uint32[n_verts] (_abi.MESH_SNAP_*); displacement=True: `displacement` is float32[n_verts].
        max_points_in_flight bounds the workspace and changes no bit of the result."""
        c = self._live()
        opt, st = c._snap_options(iterations, tolerance, max_step, max_displacement, min_gradient, level, attributes, inference, max_points_in_flight), _abi.MeshSnapStats()
        n = self.n_verts
        if select is not None:
            select = np.ascontiguousarray(np.asarray(select).ravel() != 0, dtype=np.uint32)
            if select.size != n:
                raise ValueError("select must have one value per vertex")
        wanted = (("residual_before", "residual_after") if residuals else ()) + (("state",) if states else ()) + (("displacement",) if displacement else ())
        bufs = {}
        try:
            if select is not None:
                bufs["select"] = c.upload(select) if n else c.device_malloc(4)
            for key in wanted:
                bufs[key] = c.device_malloc(max(n, 1) * 4)
            out = _returned_mesh(c, st, lambda m: c.f.mesh_snap(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), bufs.get("select"), m, bufs.get("residual_before"),
                                                               bufs.get("residual_after"), bufs.get("state"), bufs.get("displacement"), C.byref(st)))
            try:
                for key in wanted:
                    dt = np.uint32 if key == "state" else np.float32
                    setattr(out, key, c.download(bufs[key], n, dt) if n else np.empty(0, dt))
            except BaseException:
                out.free()
                raise
        finally:
            for p_ in bufs.values():
                c.device_free(p_)
        return out

    def sdf_residual(self, level=0.0, inference=True, stream=None):
        """The census of rnb_mesh_snap with iterations = 0: -> (residual float32[n_verts], the model's sdf - level at every vertex; the snap stats, whose max_before and
        sum_before_q / 2^24 / n_selected are the largest and the mean |residual|). Nothing of the mesh changes."""
        with self.snap(iterations=0, level=level, inference=inference, residuals=True, stream=stream) as census:
            return census.residual_before, census.stats

    def vertex_normals(self, flip=False, on_device=False, stream=None):
        """rnb_mesh_vertex_normals (include/rnb_mesh_smooth.h): area-weighted vertex normals from the triangles around every vertex -> the dict of
        rnb_mesh_vertex_normals_stats (n_zero, max_corners, peak_workspace, ms) with `normals`, float32[n_verts, 3]: unit length, counter-clockwise (on an extracted mesh
        the direction of its SDF-gradient normals), 0 for a vertex no triangle with an area uses; flip=True negates them (the sign of the host's compute_normals).
        on_device=True: `normals` is a device pointer instead; the caller releases it with Context.device_free. Nothing of the mesh changes."""
        c = self._live()
        opt, st = c._vertex_normals_options(flip), _abi.MeshVertexNormalsStats()
        n = self.n_verts
        buf = c.device_malloc(max(n, 1) * 12)
        try:
            c._check(c.f.mesh_vertex_normals(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), buf, C.byref(st)))
            out = st.as_dict()
            if on_device:
                out["normals"], buf = buf, None
            else:
                out["normals"] = c.download(buf, n * 3, np.float32).reshape(-1, 3) if n else np.empty((0, 3), np.float32)
        finally:
            if buf:
                c.device_free(buf)
        return out

    def self_intersections(self, pairs=False, cells=0, on_device=False, stream=None):
        """rnb_mesh_intersections (include/rnb_mesh_intersect.h): which triangles of this mesh pass through or touch others -> the dict of rnb_mesh_intersect_stats
        (n_tris, n_degenerate, n_same_set, n_candidates, n_pairs_proper, n_pairs_contact, n_tris_proper, n_tris_contact, n_coplanar_pairs, the grid block dims, cell,
        n_cell_entries, n_large, n_visited, peak_workspace, ms, ms_grid) with `n_proper` and `n_contact`, uint32[n_triangles]: the partners of every triangle in
        each class. PROPER: an edge passes through the other triangle's interior, certain in double precision; CONTACT: touching, folded, coplanar overlap or
        undecided. pairs=True adds `pairs`, uint32[n, 3]: (s, t, class) with s < t, ascending, class 1 = proper, 2 = contact (a second call with the exact capacity is
        made when the first guess was short). on_device=True: `n_proper` and `n_contact` are device pointers instead, for drop_intersecting(counts=...); the caller
        releases both with Context.device_free. `cells` (0 = automatic) changes the time, never a bit of the result. Nothing of the mesh changes."""
        c = self._live()
        opt, st = c._intersect_options(cells), _abi.MeshIntersectStats()
        nt, rec = self.n_triangles, np.dtype(_abi.MESH_INTERSECT_PAIR_DTYPE)
        counts, buf = [], None
        try:
            for _ in range(2):
                counts.append(c.device_malloc(max(nt, 1) * 4))
            cap = max(256, nt // 8) if pairs else 0
            for attempt in range(2 if pairs else 1):
                if pairs:
                    buf = c.device_malloc(cap * rec.itemsize)
                c._check(c.f.mesh_intersections(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), counts[0], counts[1], buf, cap, C.byref(st)))
                if not pairs or st.n_pairs_written_would_be <= cap:
                    break
                c.device_free(buf)  # the guess was short: once more with what the list needs
                buf, cap = None, st.n_pairs_written_would_be
            out = st.as_dict()
            if pairs:
                n = st.n_pairs_written_would_be
                got = c.download(buf, n, rec) if n else np.empty(0, rec)
                out["pairs"] = np.stack([got["s"], got["t"], got["cls"]], 1) if n else np.empty((0, 3), np.uint32)
            if on_device:
                out["n_proper"], out["n_contact"] = counts
                counts = []
            else:
                for key, ptr in zip(("n_proper", "n_contact"), counts):
                    out[key] = c.download(ptr, nt, np.uint32) if nt else np.empty(0, np.uint32)
        finally:
            for ptr in counts + ([buf] if buf else []):
                c.device_free(ptr)
        return out

    def drop_intersecting(self, classes="proper", rings=0, counts=None, drop_unused_vertices=True, cells=0, stream=None):
        """rnb_mesh_intersections_select (include/rnb_mesh_intersect.h) -> a new DeviceMesh without the triangles that have a partner in `classes` ("proper",
        "contact" or "all"), the selection grown `rings` times (0 .. 8) by the triangles that share a vertex with it; input order, colours and normals carried
        along; its `stats` are the select stats. counts: the dict self_intersections(on_device=True) returned for this mesh (it stays the caller's); None: the census
        is run here (with `cells`), its counts released whether or not a stage fails, and its statistics go to `stats["census"]`. Close the rims with fill_holes."""
        c = self._live()
        opt, st = c._intersect_select_options(classes, rings, drop_unused_vertices), _abi.MeshIntersectSelectStats()
        own = counts is None
        if own:
            counts = self.self_intersections(cells=cells, on_device=True, stream=stream)
        try:
            out = _returned_mesh(c, st, lambda m: c.f.mesh_intersections_select(c._h, _stream_handle(stream), C.byref(self), counts["n_proper"], counts["n_contact"], C.byref(opt), m, C.byref(st)))
        finally:
            if own:
                c.device_free(counts["n_proper"])
                c.device_free(counts["n_contact"])
        if own:
            out._stats["census"] = {k: v for k, v in counts.items() if k not in ("n_proper", "n_contact")}
        return out

    def _distance(self, other, opt, per_vertex, stream):
        """One rnb_mesh_distance call, self -> other; the dict distance_to returns for one direction."""
        c = self.ctx
        st = _abi.MeshDistanceStats()
        n_tau = sum(1 for x in opt.tau if x != 0)
        dist = near = None
        try:
            if per_vertex:
                dist, near = c.device_malloc(max(self.n_verts, 1) * 4), c.device_malloc(max(self.n_verts, 1) * 4)
            c._check(c.f.mesh_distance(c._h, _stream_handle(stream), C.byref(self), C.byref(other), C.byref(opt), dist, near, C.byref(st)))
            out = st.as_dict()
            if per_vertex:
                out["vert_dist"] = c.download(dist, self.n_verts, np.float32)
                out["vert_nearest"] = c.download(near, self.n_verts, np.uint32)
        finally:
            for p in (dist, near):
                if p:
                    c.device_free(p)
        unit, sw = float(opt.unit), st.sum_w
        out["unit"] = unit
        out["mean"] = st.sum_wd / sw * unit if sw else 0.0
        out["rms"] = math.sqrt(st.sum_wd2 / sw) * unit if sw else 0.0
        out["max"] = st.max_distance
        out["within"] = [st.sum_within[k] / sw if sw else 0.0 for k in range(n_tau)]
        out["quantisation"] = st.n_samples / sw * unit if sw else 0.0
        return out

    def distance_to(self, other, level=1, max_distance=0.0, unit=2.0 ** -10, thresholds=(), cells=0, per_vertex=False, symmetric=False, stream=None):
        """rnb_mesh_distance from this mesh (A) to `other` (B), both on the device: the dict of Context.mesh_distance, which describes every argument and key."""
        c = self._live()
        other._live()
        opt = c._distance_options(level, max_distance, unit, thresholds, cells)
        out = self._distance(other, opt, per_vertex, stream)
        if symmetric:
            back = other._distance(self, opt, per_vertex, stream)
            out["reverse"] = back
            out["chamfer"] = out["mean"] + back["mean"]
            out["hausdorff"] = max(out["max"], back["max"])
            out["fscore"] = [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["within"], back["within"])]
        return out

    def rasterize(self, view, near=2.0 ** -10, cull="none", shading="face", faces=False, stream=None, out_ptr=None):
        """rnb_mesh_raster of this mesh into one camera: the dict of Context.rasterize_mesh, which describes every argument and key. out_ptr: a device buffer of
        height * width * 9 floats the image is written to and left in; the dict then has no `image`."""
        c = self._live()
        opt = c._raster_options(near, cull, shading)
        if shading == "vertex" and not self.has_normals:
            raise ValueError("shading='vertex' needs normals")
        h, w = int(view["height"]), int(view["width"])
        n = h * w
        st = _abi.MeshRasterStats()
        img, fac, own = out_ptr, None, []
        try:
            if img is None:
                img = c.device_malloc(max(n, 1) * _abi.MESH_RASTER_CHANNELS * 4)
                own.append(img)
            if faces:
                fac = c.device_malloc(max(n, 1) * 4)
                own.append(fac)
            c._check(c.f.mesh_raster(c._h, _stream_handle(stream), C.byref(self), C.byref(_view_struct(view)), C.byref(opt), img, fac, C.byref(st)))
            out = st.as_dict()
            if out_ptr is None:
                out["image"] = c.download(img, n * _abi.MESH_RASTER_CHANNELS, np.float32).reshape(h, w, _abi.MESH_RASTER_CHANNELS)
            if faces:
                out["faces"] = c.download(fac, n, np.uint32).reshape(h, w)
        finally:
            for p in own:
                c.device_free(p)
        return out

    def _texture_arrays(self, uv, color, normal):
        """The host arrays of a texture checked against this mesh: (uv float32[n_triangles,3,2], color, normal float32[S,S,4] or None, S)."""
        if color is None and normal is None:
            raise ValueError("a colour map, a normal map or both must be given")
        uv = np.ascontiguousarray(uv, dtype=np.float32)
        if uv.size != self.n_triangles * 6:
            raise ValueError("uv must hold 3 x 2 floats per triangle (%d triangles, %d floats)" % (self.n_triangles, uv.size))
        maps = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (color, normal)]
        shapes = {a.shape for a in maps if a is not None}
        shape = next(iter(shapes))
        if len(shapes) != 1 or len(shape) != 3 or shape[0] != shape[1] or shape[2] != 4 or shape[0] < 1:
            raise ValueError("color and normal must be float32 arrays [S, S, 4] of one size")
        return uv, maps[0], maps[1], shape[0]

    def _upload_texture(self, uv, color, normal, own):
        """rnb_mesh_draw_texture of the arrays of _texture_arrays, each uploaded once; the device buffers are appended to `own`, which the caller releases."""
        c = self._live()
        uv, color, normal, size = self._texture_arrays(uv, color, normal)
        tex = _abi.MeshDrawTexture()
        tex.size, tex.n_tris = size, self.n_triangles
        for field, a in (("uv_dev", uv), ("color_dev", color), ("normal_dev", normal)):
            if a is not None and a.size:
                own.append(c.upload(a))
                setattr(tex, field, own[-1])
        return tex

    def _draw(self, tex, view, opt, faces, stream, out_ptr):
        """rnb_mesh_draw_textured with a texture that is on the device: the dict of draw_textured."""
        c = self._live()
        h, w = int(view["height"]), int(view["width"])
        n = h * w
        st = _abi.MeshDrawStats()
        img, fac, own = out_ptr, None, []
        try:
            if img is None:
                img = c.device_malloc(max(n, 1) * _abi.MESH_RASTER_CHANNELS * 4)
                own.append(img)
            if faces:
                fac = c.device_malloc(max(n, 1) * 4)
                own.append(fac)
            c._check(c.f.mesh_draw_textured(c._h, _stream_handle(stream), C.byref(self), C.byref(tex), C.byref(_view_struct(view)), C.byref(opt), img, fac, C.byref(st)))
            out = st.as_dict()
            if out_ptr is None:
                out["image"] = c.download(img, n * _abi.MESH_RASTER_CHANNELS, np.float32).reshape(h, w, _abi.MESH_RASTER_CHANNELS)
            if faces:
                out["faces"] = c.download(fac, n, np.uint32).reshape(h, w)
        finally:
            for p in own:
                c.device_free(p)
        return out

    def draw_textured(self, view, uv, color=None, normal=None, near=2.0 ** -10, cull="none", shading="face", filter="bilinear", faces=False, stream=None, out_ptr=None):
        """rnb_mesh_draw_textured (include/rnb_mesh_draw.h) of this mesh into one camera: the dict of rasterize (`image` float32 [H,W,9], with faces=True `faces`, the
        fields of rnb_mesh_raster_stats) and n_bad_uv, n_normal_fallback, n_unowned_taps. uv float32[n_triangles,3,2], color and normal float32[S,S,4] (one of the two
        may be None) are host arrays, such as the `uv` / `albedo` / `color` / `normal` entries of bake_texture or project_views: channels 3-5 of the image are the colour
        map's texels under the pixels (the mesh's own colours without one), channels 0-2 the normal map's, normalised (the normal `shading` selects without one, and
        where the map holds no direction); channels 6-8 and `faces` are those of rasterize. filter: "bilinear" or "nearest". The arrays are uploaded once and released
        whether or not a step raises. out_ptr: as in rasterize. Bit-reproducible. Leaves the training state as it was."""
        c = self._live()
        opt = c._draw_options(near, cull, shading, filter)
        if shading == "vertex" and not self.has_normals:
            raise ValueError("shading='vertex' needs normals")
        own = []
        try:
            tex = self._upload_texture(uv, color, normal, own)
            return self._draw(tex, view, opt, faces, stream, out_ptr)
        finally:
            for p in own:
                c.device_free(p)

    def visibility(self, views, masks=None, near=2.0 ** -10, cull="none", min_pixels=1, supersample=1, on_device=False, stream=None):
        """rnb_mesh_visibility of this mesh in all of `views` at once: (records, stats), described by Context.mesh_visibility. on_device=True: the records stay on the
        device and `records` is the pointer to n_triangles records of 40 bytes, which the caller releases with Context.device_free."""
        c = self._live()
        opt, varr = c._visibility_options(near, cull, min_pixels), c._visibility_views(views, masks, supersample)
        st = _abi.MeshVisibilityStats()
        nt, own, faces = self.n_triangles, [], None
        rec = np.dtype(_abi.MESH_FACE_VISIBILITY_DTYPE)
        try:
            for k, mk in enumerate(masks or ()):
                if mk is not None:
                    a = np.ascontiguousarray(np.asarray(mk) != 0, dtype=np.uint8)
                    varr[k].mask_height, varr[k].mask_width = a.shape
                    own.append(c.upload(a) if a.size else c.device_malloc(4))
                    varr[k].mask_dev = own[-1]
            faces = c.device_malloc(max(nt, 1) * rec.itemsize)
            c._check(c.f.mesh_visibility(c._h, _stream_handle(stream), C.byref(self), varr, len(varr), C.byref(opt), faces, C.byref(st)))
            if on_device:
                out, faces = faces, None
            else:
                out = c.download(faces, nt, rec) if nt else np.empty(0, rec)
        finally:
            for p in own + ([faces] if faces else []):
                c.device_free(p)
        return out, st.as_dict()

    def select_seen(self, records_ptr, unit="component", min_views=1, max_off_mask=None, rings=1, kept=False, stream=None):
        """rnb_mesh_visibility_select on the records visibility(on_device=True) left on the device -> the DeviceMesh of what is kept; its `stats` are the select stats, with
        kept=True also `kept`: uint32[n_triangles], 1 for a kept triangle of this mesh. The arguments are those of Context.cull_unseen_mesh."""
        c = self._live()
        opt, st = c._visibility_select_options(unit, min_views, max_off_mask, rings), _abi.MeshVisibilitySelectStats()
        nt, flags = self.n_triangles, None
        try:
            if kept:
                flags = c.device_malloc(max(nt, 1) * 4)
            out = _returned_mesh(c, st, lambda m: c.f.mesh_visibility_select(c._h, _stream_handle(stream), C.byref(self), records_ptr, C.byref(opt), m, flags, C.byref(st)))
            if kept:
                try:
                    out._stats["kept"] = c.download(flags, nt, np.uint32) if nt else np.empty(0, np.uint32)
                except BaseException:
                    out.free()
                    raise
        finally:
            if flags:
                c.device_free(flags)
        return out

    def cull_unseen(self, views, masks=None, unit="component", min_views=1, max_off_mask=None, rings=1, near=2.0 ** -10, cull="none", min_pixels=1, supersample=1, stream=None,
                    report=False):
        """This mesh without what the cameras do not see: visibility, then select_seen, the records released whether or not a stage fails -> the DeviceMesh of what is kept
        (its `stats`: the select stats). report=True: (mesh, dict(visibility=the statistics of the measurement, select=those of the selection, kept=uint32[n_triangles])).
        The arguments are those of Context.cull_unseen_mesh."""
        c = self._live()
        c._visibility_select_options(unit, min_views, max_off_mask, rings)  # a bad argument fails before anything is measured
        records, vis = self.visibility(views, masks, near, cull, min_pixels, supersample, on_device=True, stream=stream)
        try:
            out = self.select_seen(records, unit, min_views, max_off_mask, rings, kept=report, stream=stream)
        finally:
            c.device_free(records)
        if not report:
            return out
        sel = dict(out.stats)
        return out, dict(visibility=vis, select=sel, kept=sel.pop("kept"))

    def bake_texture(self, size, block=0, maps=("albedo",), inference=True, max_texels_in_flight=0, stream=None):
        """rnb_mesh_bake_texture of this mesh: the dict of Context.bake_texture, which describes every argument and key. The device result is downloaded and released
        before the call returns; nothing stays allocated if a step raises."""
        c = self._live()
        opt = c._texture_options(size, block, maps, inference, max_texels_in_flight)
        tex, st = _abi.MeshTexture(), _abi.MeshTextureStats()
        try:
            c._check(c.f.mesh_bake_texture(c._h, _stream_handle(stream), C.byref(self), C.byref(opt), C.byref(tex), C.byref(st)))
            nt, n = tex.n_tris, tex.size * tex.size * 4
            out = dict(uv=c.download(tex.uv, nt * 6, np.float32).reshape(nt, 3, 2) if nt else np.empty((0, 3, 2), np.float32))
            for name in _abi.MESH_TEXTURE_MAPS:
                if getattr(tex, name):
                    out[name] = c.download(getattr(tex, name), n, np.float32).reshape(tex.size, tex.size, 4)
            out.update(block=tex.block, blocks_per_row=tex.blocks_per_row, stats=st.as_dict())
        finally:
            c.f.mesh_texture_free(c._h, C.byref(tex))  # (whatever a failed call left: a zeroed struct releases nothing)
        return out

    def project_views(self, views, images, size=1024, block=0, mode="blend", normals=None, weight_power=2, min_cos=0.1, depth_tolerance=2.0 ** -8, near=2.0 ** -10, cull="none",
                      fallback=None, inference=True, stream=None):
        """rnb_mesh_project_views of this mesh: the dict of Context.project_views, which describes every argument and key (normals: its `shading`; None means the vertex
        normals when the mesh has them, else the face normals). Every image is uploaded once; the images, the fallback and the device result are released before the call
        returns, whether or not a step raises."""
        c = self._live()
        if normals is None:
            normals = "vertex" if self.has_normals else "face"
        opt = c._project_options(size, block, mode, normals, weight_power, min_cos, depth_tolerance, near, cull)
        if normals == "vertex" and not self.has_normals:
            raise ValueError("normals='vertex' needs a mesh with normals")
        varr, arrays = c._project_views(views, images)
        fb = None
        if fallback is not None and not (isinstance(fallback, str) and fallback == "model"):
            fb = np.ascontiguousarray(fallback, dtype=np.float32)
            if fb.shape != (int(size), int(size), 4):
                raise ValueError("fallback must be None, 'model' or a float32 array [size, size, 4]")
        own, proj, tex, st = [], _abi.MeshProjection(), _abi.MeshTexture(), _abi.MeshProjectStats()
        try:
            for e, a in zip(varr, arrays):
                own.append(c.upload(a))
                e.image_dev = own[-1]
            if fb is not None:
                own.append(c.upload(fb))
                opt.fallback_dev = own[-1]
            elif fallback is not None:
                topt = c._texture_options(size, block, ("albedo",), inference, 0)
                c._check(c.f.mesh_bake_texture(c._h, _stream_handle(stream), C.byref(self), C.byref(topt), C.byref(tex), None))
                opt.fallback_dev = tex.albedo
            c._check(c.f.mesh_project_views(c._h, _stream_handle(stream), C.byref(self), varr, len(varr), C.byref(opt), C.byref(proj), C.byref(st)))
            nt, n = proj.n_tris, proj.size * proj.size
            out = dict(uv=c.download(proj.uv, nt * 6, np.float32).reshape(nt, 3, 2) if nt else np.empty((0, 3, 2), np.float32),
                       color=c.download(proj.color, n * 4, np.float32).reshape(proj.size, proj.size, 4),
                       info=c.download(proj.info, n * 2, np.uint32).reshape(proj.size, proj.size, 2),
                       block=proj.block, blocks_per_row=proj.blocks_per_row, stats=st.as_dict())
        finally:
            c.f.mesh_projection_free(c._h, C.byref(proj))  # (whatever a failed call left: a zeroed struct releases nothing)
            c.f.mesh_texture_free(c._h, C.byref(tex))
            for p in own:
                c.device_free(p)
        return out
