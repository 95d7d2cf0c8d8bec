"""ctypes declarations of include/rnb_neus2.h (structs, enums, prototypes).

``declare(lib, prefix)`` attaches argtypes/restypes to an already loaded CDLL. The product always uses the
prefix ``rnb_`` (librnb_neus2_hip.so); the test suite applies the same declarations to its CPU checker, which exports
the identical signatures under its own prefix.
"""
import ctypes as C

ABI_VERSION = 5

# status codes (rnb_status)
OK, ERR_INVALID, ERR_DEVICE, ERR_NOMEM, ERR_NO_SAMPLES = 0, -1, -2, -3, -4

N_SDF_MLP_PARAMS = 3072
N_RGB_MLP_PARAMS = 8192
N_VARIANCE_PARAMS = 4
GRIDSIZE = 128
CASCADES = 8


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_levels", C.c_uint32),
        ("log2_hashmap_size", C.c_uint32),
        ("base_resolution", C.c_uint32),
        ("per_level_scale", C.c_float),
        ("valid_level_scale", C.c_float),
        ("base_valid_level_scale", C.c_float),
        ("base_training_step", C.c_uint32),
        ("sdf_bias", C.c_float),
        ("target_batch_size", C.c_uint32),
        ("initial_rays_per_batch", C.c_uint32),
        ("max_rays_per_batch", C.c_uint32),
        ("aabb_scale", C.c_uint32),
        ("seed", C.c_uint32),
        ("mask_loss_weight", C.c_float),
        ("ek_loss_weight", C.c_float),
        ("apply_L2", C.c_uint32),
        ("apply_rgbplus", C.c_uint32),
        ("apply_no_albedo", C.c_uint32),
        ("apply_light_opti", C.c_uint32),
        ("apply_supernormal", C.c_uint32),
        ("apply_relu", C.c_uint32),
        ("apply_bce", C.c_uint32),
        ("snap_to_pixel_centers", C.c_uint32),
        ("learning_rate", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("epsilon", C.c_float),
        ("l2_reg", C.c_float),
        ("ema_decay", C.c_float),
        ("lr_decay_start", C.c_uint32),
        ("lr_decay_interval", C.c_uint32),
        ("lr_decay_base", C.c_float),
        ("density_grid_decay", C.c_float),
        ("world_size", C.c_uint32),
        ("rank", C.c_uint32),
        ("only_sdf_training", C.c_uint32),
        ("overlap", C.c_uint32),
        ("accumulate", C.c_uint32),
        ("deterministic", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class View(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("focal_length", C.c_float * 2),
        ("principal_point", C.c_float * 2),
        ("xform", C.c_float * 12),
    ]


class StepStats(C.Structure):
    _fields_ = [
        ("training_step", C.c_uint32),
        ("rays_per_batch", C.c_uint32),
        ("next_rays_per_batch", C.c_uint32),
        ("measured_batch_size", C.c_uint32),
        ("measured_batch_size_before_compaction", C.c_uint32),
        ("n_rays_kept", C.c_uint32),
        ("density_grid_updated", C.c_uint32),
        ("loss", C.c_float),
        ("ek_loss", C.c_float),
        ("mask_loss", C.c_float),
        ("prep_ms", C.c_float),
        ("step_ms", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# rnb_buffer_id
BUF = dict(
    PARAMS_FP32=0, PARAMS_FP16=1, PARAMS_EMA=2, GRADS_FP32=3, ADAM_M=4, ADAM_V=5, ADAM_STEPS=6,
    DENSITY_GRID=7, DENSITY_BITFIELD=8, DENSITY_MEAN=9, RAY_INDICES=10, RAYS=11, NUMSTEPS=12,
    COORDS=13, MLP_OUT=14, DLOSS_DOUT=15, COORDS_COMPACTED=16, LOSS=17, EK_LOSS=18, MASK_LOSS=19,
    COUNTERS=20, DENSITY_GRID_TMP=21, GRID_SAMPLE_POS=22, GRID_SAMPLE_IDX=23, STEP_VECTOR=24, GRID_SAMPLE_POS_EVAL=25, GRID_SAMPLE_IDX_EVAL=26, GRADS_FP16=27,
)
BUF_DTYPE = dict(
    PARAMS_FP32="f4", PARAMS_FP16="f2", PARAMS_EMA="f2", GRADS_FP32="f4", ADAM_M="f4", ADAM_V="f4", ADAM_STEPS="u4",
    DENSITY_GRID="f4", DENSITY_BITFIELD="u1", DENSITY_MEAN="f4", RAY_INDICES="u4", RAYS="f4", NUMSTEPS="u4",
    COORDS="f4", MLP_OUT="f2", DLOSS_DOUT="f2", COORDS_COMPACTED="f4", LOSS="f4", EK_LOSS="f4", MASK_LOSS="f4",
    COUNTERS="u4", DENSITY_GRID_TMP="f4", GRID_SAMPLE_POS="f4", GRID_SAMPLE_IDX="u4", STEP_VECTOR="f8", GRID_SAMPLE_POS_EVAL="f4", GRID_SAMPLE_IDX_EVAL="u4", GRADS_FP16="f2",
)
ACCUM_FP32, ACCUM_HALF = 0, 1  # rnb_accumulate
BUF_READONLY = 0x100  # RNB_BUF_READONLY
GRID_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)  # rnb_grid_exchange_fn(user, grid_tmp, n_elements, stream)
PRIM = dict(PCG32=0, MORTON=1, SRGB=2, RAY_BOX=3, MARCH=4, ACTIVATION=5, WARP=6, LOSS=7, PIXEL=8, GRID=9, READ_RGBA=10, CAMERA_RAY=11, RAY_TARGETS=12, LOSS_SAMPLE=13, RAY_LOSS=14, ENCODE=15, MARCH_RAY=16, SDF_DENSITY=17, PREP_DUE=18, DW_SLICED=19, ENCODE_FORM=20)  # rnb_primitive
PRIM_IN_WORDS, PRIM_OUT_WORDS = (6, 3, 1, 8, 9, 1, 9, 9, 9, 7, 32, 20, 35, 37, 16, 263, 10, 2, 1, 33028, 1), (4, 4, 2, 3, 7, 3, 11, 5, 3, 3, 5, 9, 7, 28, 9, 16, 23, 1, 2, 16, 1)
H2D, D2H, D2D = 0, 1, 2

_ctx = C.c_void_p
_stream = C.c_void_p
_u32, _u64, _i = C.c_uint32, C.c_uint64, C.c_int

# name -> (restype, argtypes); every name here must be exported by the library (tests check this against the header)
PROTOTYPES = {
    "last_error": (C.c_char_p, []),
    "abi_version": (_u32, []),
    "default_config": (_i, [C.POINTER(Config)]),
    "create": (_i, [C.POINTER(Config), C.POINTER(_ctx)]),
    "destroy": (_i, [_ctx]),
    "update_config": (_i, [_ctx, C.POINTER(Config)]),
    "n_params": (_u64, [_ctx]),
    "param_layout": (_i, [_ctx, C.POINTER(_u64)]),
    "grid_tables": (_i, [_ctx, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_float)]),
    "init_params": (_i, [_ctx, C.POINTER(C.c_float)]),
    "set_params": (_i, [_ctx, C.POINTER(C.c_float)]),
    "buffer": (_i, [_ctx, _i, C.POINTER(C.c_void_p), C.POINTER(_u64)]),
    "params_changed": (_i, [_ctx]),
    "bitfield_changed": (_i, [_ctx]),
    "memcpy": (_i, [_ctx, C.c_void_p, C.c_void_p, _u64, _i]),
    "device_malloc": (_i, [_ctx, _u64, C.POINTER(C.c_void_p)]),
    "device_free": (_i, [_ctx, C.c_void_p]),
    "set_dataset": (_i, [_ctx, _u32, C.POINTER(View), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "set_training_step": (_i, [_ctx, _u32]),
    "valid_level": (_u32, [_ctx]),
    "update_density_grid": (_i, [_ctx, _stream]),
    "update_density_bitfield": (_i, [_ctx, _stream]),
    "update_density_grid_begin": (_i, [_ctx, _stream]),
    "update_density_grid_end": (_i, [_ctx, _stream]),
    "set_grid_exchange": (_i, [_ctx, C.c_void_p, C.c_void_p]),
    "density": (_i, [_ctx, _stream, C.c_void_p, _u32, C.c_void_p, _i]),
    "sdf": (_i, [_ctx, _stream, C.c_void_p, _u32, C.c_void_p, _i]),
    "forward_infer": (_i, [_ctx, _stream, C.c_void_p, _u32, C.c_void_p, _i]),
    "sdf_lattice": (_i, [_ctx, _stream, C.POINTER(_u32), C.c_float, C.c_float, C.c_void_p, _i]),
    "marching_cubes": (_i, [_ctx, _stream, C.c_void_p, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float,
                            C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_u32), C.POINTER(_u32)]),
    "generate_training_samples": (_i, [_ctx, _stream, _u32, _u32, _u32]),
    "compute_loss": (_i, [_ctx, _stream, _u32, _u32]),
    "forward_backward": (_i, [_ctx, _stream]),
    "optimizer_step": (_i, [_ctx, _stream]),
    "train_step": (_i, [_ctx, _stream, C.POINTER(StepStats)]),
    "train_step_begin": (_i, [_ctx, _stream]),
    "train_step_end": (_i, [_ctx, _stream, C.POINTER(StepStats)]),
    "profile_enable": (_i, [_ctx, _i]),
    "profile_count": (_i, [_ctx]),
    "profile_get": (_i, [_ctx, _i, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(_u64), C.POINTER(C.c_double)]),
    "train_step_apply": (_i, [_ctx, _stream]),
    "train_step_local": (_i, [_ctx, _stream, C.POINTER(_u64), C.POINTER(C.c_double)]),
    "train_step_finish": (_i, [_ctx, C.POINTER(_u64), C.POINTER(C.c_double), C.POINTER(StepStats)]),
    "training_step": (_u32, [_ctx]),
    "rays_per_batch": (_u32, [_ctx]),
    "set_controller": (_i, [_ctx, _u32, _u32, _u32, _u32]),
    "set_optimizer_step": (_i, [_ctx, _u32]),
    "eval_primitives": (_i, [_ctx, _i, C.c_void_p, _u32, C.c_void_p]),
    "gradient_parts": (_i, [_ctx, C.POINTER(_u64 * 2 * 3), C.POINTER(_u32)]),
    "gradient_part_wait": (_i, [_ctx, _u32, _stream]),
    "train_step_apply_early": (_i, [_ctx, _stream]),
    "shard_layout": (_i, [_ctx, C.POINTER(_u64 * 4 * 3), C.POINTER(_u32), C.POINTER(_u64)]),
    "train_step_apply_shard": (_i, [_ctx, _u32, _stream]),
    "train_step_apply_done": (_i, [_ctx, _stream]),
}


# ---- include/rnb_render.h: the inference tracer, a header of its own with its own version (the HIP library only; the CPU checker has no tracer) ----
RENDER_ABI_VERSION = 1
RENDER_CHANNELS = 9  # normal 3, albedo 3, opacity, depth, samples


class RenderOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("min_transmittance", C.c_float),
        ("near_distance", C.c_float),
        ("use_inference_params", C.c_uint32),
        ("use_occupancy", C.c_uint32),
        ("max_rays_in_flight", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class RenderStats(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint32),
        ("n_hit", C.c_uint32),
        ("rounds", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_samples", C.c_uint64),
        ("ms", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


RENDER_PROTOTYPES = {
    "render_abi_version": (_u32, []),
    "render_default_options": (_i, [C.POINTER(RenderOptions)]),
    "render": (_i, [_ctx, _stream, C.POINTER(View), C.POINTER(RenderOptions), C.c_void_p, C.POINTER(RenderStats)]),
}


# ---- include/rnb_mesh.h: the sparse mesh extractor, a header of its own with its own version (the HIP library only) ----
MESH_ABI_VERSION = 1
MESH_CULL_NONE, MESH_CULL_OCCUPANCY = 0, 1
MESH_ATTR_COLORS, MESH_ATTR_NORMALS = 1, 2
MESH_MAX_RES = 4096


class MeshOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("res", C.c_uint32 * 3),
        ("lattice_min", C.c_float),
        ("lattice_max", C.c_float),
        ("aabb_min", C.c_float * 3),
        ("aabb_max", C.c_float * 3),
        ("thresh", C.c_float),
        ("use_inference_params", C.c_uint32),
        ("cull", C.c_uint32),
        ("brick", C.c_uint32),
        ("attributes", C.c_uint32),
        ("max_points_in_flight", C.c_uint32),
        ("max_active_points", C.c_uint64),
        ("reserved", C.c_uint32 * 4),
    ]


class Mesh(C.Structure):
    _fields_ = [
        ("verts", C.c_void_p),
        ("indices", C.c_void_p),
        ("colors", C.c_void_p),
        ("normals", C.c_void_p),
        ("n_verts", C.c_uint32),
        ("n_indices", C.c_uint32),
    ]


class MeshStats(C.Structure):
    _fields_ = [
        ("n_bricks", C.c_uint64),
        ("n_kept", C.c_uint64),
        ("n_evaluated", C.c_uint64),
        ("n_sign_change", C.c_uint64),
        ("n_points_evaluated", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


MESH_PROTOTYPES = {
    "mesh_abi_version": (_u32, []),
    "mesh_default_options": (_i, [C.POINTER(MeshOptions)]),
    "extract_mesh": (_i, [_ctx, _stream, C.POINTER(MeshOptions), C.POINTER(Mesh), C.POINTER(MeshStats)]),
    "mesh_free": (_i, [_ctx, C.POINTER(Mesh)]),
}


# ---- include/rnb_mesh_clean.h: components / keep-largest / outward orientation of a device mesh, a header of its own with its own version (the HIP library only) ----
MESH_CLEAN_ABI_VERSION = 1
MESH_KEEP_ALL, MESH_KEEP_LARGEST = 0, 1
MESH_ORIENT_NONE, MESH_ORIENT_OUTWARD = 0, 1
MESH_Q_SHIFT, MESH_Q_TERM_LOG2 = 44, 18
MESH_NO_LABEL = 0xFFFFFFFF


class MeshCleanOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("keep", C.c_uint32),
        ("orient", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshComponent(C.Structure):
    _fields_ = [
        ("label", C.c_uint32),
        ("n_vertices", C.c_uint32),
        ("n_triangles", C.c_uint32),
        ("kept", C.c_uint32),
        ("area_q", C.c_int64),
        ("volume_q", C.c_int64),
    ]


# the same record as a numpy dtype (Context.clean_mesh returns the table as a structured array)
MESH_COMPONENT_DTYPE = [("label", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("kept", "<u4"), ("area_q", "<i8"), ("volume_q", "<i8")]


class MeshCleanStats(C.Structure):
    _fields_ = [
        ("n_components", C.c_uint32),
        ("n_kept", C.c_uint32),
        ("n_verts_in", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_in", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("largest_label", C.c_uint32),
        ("hook_passes", C.c_uint32),
        ("flatten_passes", C.c_uint32),
        ("reserved", C.c_uint32),
        ("area_q_in", C.c_int64),
        ("area_q_out", C.c_int64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved2", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_CLEAN_PROTOTYPES = {
    "mesh_clean_abi_version": (_u32, []),
    "mesh_clean_default_options": (_i, [C.POINTER(MeshCleanOptions)]),
    "mesh_clean": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshCleanOptions), C.POINTER(Mesh), C.POINTER(C.c_void_p), C.POINTER(MeshCleanStats)]),
    "mesh_clean_table_free": (_i, [_ctx, C.c_void_p]),
}


# ---- include/rnb_mesh_simplify.h: vertex clustering with quadric placement of a device mesh, a header of its own with its own version (the HIP library only) ----
MESH_SIMPLIFY_ABI_VERSION = 1
MESH_PLACE_QUADRIC, MESH_PLACE_MEAN = 0, 1
MESH_SIMPLIFY_MAX_DIM, MESH_SIMPLIFY_MAX_CELLS = 4096, 1 << 30
MESH_SIMPLIFY_Q_SHIFT, MESH_SIMPLIFY_Q_TERM_LOG2 = 40, 22


class MeshSimplifyOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("origin", C.c_float * 3),
        ("cell", C.c_float),
        ("dims", C.c_uint32 * 3),
        ("placement", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshSimplifyStats(C.Structure):
    _fields_ = [
        ("n_verts_in", C.c_uint32),
        ("n_tris_in", C.c_uint32),
        ("n_clusters", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("n_tris_collapsed", C.c_uint32),
        ("n_clamped", C.c_uint32),
        ("n_fallback", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_SIMPLIFY_PROTOTYPES = {
    "mesh_simplify_abi_version": (_u32, []),
    "mesh_simplify_default_options": (_i, [C.POINTER(MeshSimplifyOptions)]),
    "mesh_simplify": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshSimplifyOptions), C.POINTER(Mesh), C.POINTER(MeshSimplifyStats)]),
}

# ---- include/rnb_mesh_distance.h: the one-sided distance from one device mesh to another, a header of its own with its own version (the HIP library only) ----
MESH_DISTANCE_ABI_VERSION = 1
MESH_DISTANCE_MAX_LEVEL, MESH_DISTANCE_MAX_TAUS, MESH_DISTANCE_NONE = 3, 4, 0xFFFFFFFF
MESH_DISTANCE_MAX_CELLS, MESH_DISTANCE_LARGE_CELLS, MESH_DISTANCE_MAX_LARGE, MESH_DISTANCE_MAX_ENTRIES = 256, 2048, 4096, 1 << 31
MESH_DISTANCE_Q_SHIFT, MESH_DISTANCE_Q_TERM_LOG2 = 48, 12


class MeshDistanceOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("level", C.c_uint32),
        ("max_distance", C.c_float),
        ("unit", C.c_float),
        ("tau", C.c_float * 4),
        ("cells", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshDistanceStats(C.Structure):
    _fields_ = [
        ("n_verts_from_used", C.c_uint32),
        ("n_verts_to_used", C.c_uint32),
        ("n_tris_from", C.c_uint32),
        ("n_tris_to", C.c_uint32),
        ("n_degenerate_from", C.c_uint32),
        ("n_degenerate_to", C.c_uint32),
        ("n_verts_beyond", C.c_uint32),
        ("n_large", C.c_uint32),
        ("n_samples", C.c_uint64),
        ("n_beyond", C.c_uint64),
        ("sum_w", C.c_int64),
        ("sum_wd", C.c_int64),
        ("sum_wd2", C.c_int64),
        ("sum_within", C.c_int64 * 4),
        ("max_distance", C.c_double),
        ("dims", C.c_uint32 * 3),
        ("reserved", C.c_uint32),
        ("cell", C.c_double),
        ("n_cell_entries", C.c_uint64),
        ("n_pairs", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("ms_grid", C.c_float),
    ]

    def as_dict(self):
        return {name: (list(getattr(self, name)) if name in ("sum_within", "dims") else getattr(self, name)) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_DISTANCE_PROTOTYPES = {
    "mesh_distance_abi_version": (_u32, []),
    "mesh_distance_default_options": (_i, [C.POINTER(MeshDistanceOptions)]),
    "mesh_distance": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(Mesh), C.POINTER(MeshDistanceOptions), C.c_void_p, C.c_void_p, C.POINTER(MeshDistanceStats)]),
}

# ---- include/rnb_mesh_raster.h: a device mesh into one camera's depth, normal, colour, coverage and face maps, a header of its own with its own version (the HIP library only) ----
MESH_RASTER_ABI_VERSION = 1
MESH_RASTER_CHANNELS, MESH_RASTER_NONE, MESH_RASTER_MAX_SIZE = 9, 0xFFFFFFFF, 16384
MESH_RASTER_SUBPIXEL_BITS, MESH_RASTER_MAX_COORD_LOG2, MESH_RASTER_SMALL_PIXELS, MESH_RASTER_MAX_COUNT = 8, 28, 16, 1 << 24
MESH_RASTER_CULL_NONE, MESH_RASTER_CULL_BACK, MESH_RASTER_CULL_FRONT = 0, 1, 2
MESH_RASTER_NORMALS_FACE, MESH_RASTER_NORMALS_VERTEX = 0, 1


class MeshRasterOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("near", C.c_float),
        ("cull", C.c_uint32),
        ("normals", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshRasterStats(C.Structure):
    _fields_ = [
        ("n_tris", C.c_uint32),
        ("n_behind", C.c_uint32),
        ("n_out_of_range", C.c_uint32),
        ("n_degenerate", C.c_uint32),
        ("n_culled", C.c_uint32),
        ("n_offscreen", C.c_uint32),
        ("n_small", C.c_uint32),
        ("n_large", C.c_uint32),
        ("n_covered", C.c_uint32),
        ("n_back_pixels", C.c_uint32),
        ("n_fragments", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_RASTER_PROTOTYPES = {
    "mesh_raster_abi_version": (_u32, []),
    "mesh_raster_default_options": (_i, [C.POINTER(MeshRasterOptions)]),
    "mesh_raster": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(View), C.POINTER(MeshRasterOptions), C.c_void_p, C.c_void_p, C.POINTER(MeshRasterStats)]),
}


# ---- include/rnb_mesh_texture.h: a per-triangle UV atlas of a device mesh and the model's albedo, normal and position at its texels, a header of its own with its own version (the HIP library only) ----
MESH_TEXTURE_ABI_VERSION = 1
MESH_TEXTURE_MIN_SIZE, MESH_TEXTURE_MAX_SIZE, MESH_TEXTURE_MIN_BLOCK, MESH_TEXTURE_MAX_IN_FLIGHT = 4, 8192, 4, 1 << 22
MESH_TEXTURE_ALBEDO, MESH_TEXTURE_NORMAL, MESH_TEXTURE_POSITION = 1, 2, 4
MESH_TEXTURE_MAPS = dict(albedo=MESH_TEXTURE_ALBEDO, normal=MESH_TEXTURE_NORMAL, position=MESH_TEXTURE_POSITION)  # the result's fields, in the struct's order


class MeshTextureOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("size", C.c_uint32),
        ("block", C.c_uint32),
        ("maps", C.c_uint32),
        ("use_inference_params", C.c_uint32),
        ("max_texels_in_flight", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshTexture(C.Structure):
    _fields_ = [
        ("uv", C.c_void_p),
        ("albedo", C.c_void_p),
        ("normal", C.c_void_p),
        ("position", C.c_void_p),
        ("size", C.c_uint32),
        ("block", C.c_uint32),
        ("blocks_per_row", C.c_uint32),
        ("n_tris", C.c_uint32),
    ]


class MeshTextureStats(C.Structure):
    _fields_ = [
        ("n_texels", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("n_batches", C.c_uint32),
        ("ms", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


MESH_TEXTURE_PROTOTYPES = {
    "mesh_texture_abi_version": (_u32, []),
    "mesh_texture_default_options": (_i, [C.POINTER(MeshTextureOptions)]),
    "mesh_texture_layout": (_i, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "mesh_bake_texture": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshTextureOptions), C.POINTER(MeshTexture), C.POINTER(MeshTextureStats)]),
    "mesh_texture_free": (_i, [_ctx, C.POINTER(MeshTexture)]),
}


# ---- include/rnb_mesh_visibility.h: what a set of cameras sees of a device mesh, per triangle, and the mesh without the rest; a header of its own with its own version (the HIP library only) ----
MESH_VISIBILITY_ABI_VERSION = 1
MESH_VISIBILITY_NONE, MESH_VISIBILITY_MAX_RINGS = 0xFFFFFFFF, 64
MESH_VISIBILITY_UNIT_COMPONENT, MESH_VISIBILITY_UNIT_FACE = 0, 1


class MeshVisibilityView(C.Structure):
    _fields_ = [
        ("view", View),
        ("mask_dev", C.c_void_p),
        ("mask_width", C.c_uint32),
        ("mask_height", C.c_uint32),
    ]


class MeshVisibilityOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("near", C.c_float),
        ("cull", C.c_uint32),
        ("min_pixels", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshFaceVisibility(C.Structure):
    _fields_ = [
        ("n_drawn", C.c_uint32),
        ("n_seen", C.c_uint32),
        ("n_off_mask", C.c_uint32),
        ("best_view", C.c_uint32),
        ("best_pixels", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_pixels_won", C.c_uint64),
        ("n_pixels_covered", C.c_uint64),
    ]


# one record of rnb_mesh_face_visibility as a numpy structured dtype (40 bytes)
MESH_FACE_VISIBILITY_DTYPE = [("n_drawn", "<u4"), ("n_seen", "<u4"), ("n_off_mask", "<u4"), ("best_view", "<u4"), ("best_pixels", "<u4"), ("reserved", "<u4"),
                              ("n_pixels_won", "<u8"), ("n_pixels_covered", "<u8")]


class MeshVisibilityStats(C.Structure):
    _fields_ = [
        ("n_tris", C.c_uint32),
        ("n_views", C.c_uint32),
        ("n_behind", C.c_uint64),
        ("n_out_of_range", C.c_uint64),
        ("n_degenerate", C.c_uint64),
        ("n_culled", C.c_uint64),
        ("n_offscreen", C.c_uint64),
        ("n_small", C.c_uint64),
        ("n_large", C.c_uint64),
        ("n_pixels", C.c_uint64),
        ("n_faces_seen", C.c_uint32),
        ("n_faces_off_mask", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


class MeshVisibilitySelectOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("unit", C.c_uint32),
        ("min_views_seen", C.c_uint32),
        ("max_views_off_mask", C.c_uint32),
        ("rings", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class MeshVisibilitySelectStats(C.Structure):
    _fields_ = [
        ("n_verts_in", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_in", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("n_seeds", C.c_uint32),
        ("n_candidates", C.c_uint32),
        ("n_components", C.c_uint32),
        ("n_components_kept", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_VISIBILITY_PROTOTYPES = {
    "mesh_visibility_abi_version": (_u32, []),
    "mesh_visibility_default_options": (_i, [C.POINTER(MeshVisibilityOptions)]),
    "mesh_visibility_select_default_options": (_i, [C.POINTER(MeshVisibilitySelectOptions)]),
    "mesh_visibility": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshVisibilityView), _u32, C.POINTER(MeshVisibilityOptions), C.c_void_p, C.POINTER(MeshVisibilityStats)]),
    "mesh_visibility_select": (_i, [_ctx, _stream, C.POINTER(Mesh), C.c_void_p, C.POINTER(MeshVisibilitySelectOptions), C.POINTER(Mesh), C.c_void_p, C.POINTER(MeshVisibilitySelectStats)]),
}


# ---- include/rnb_mesh_project.h: the texels of the baker's atlas coloured from calibrated images (project, test occlusion, blend); a header of its own with its own version (the HIP library only) ----
MESH_PROJECT_ABI_VERSION = 1
MESH_PROJECT_NONE, MESH_PROJECT_MAX_WEIGHT_POWER = 0xFFFFFFFF, 8
MESH_PROJECT_FORMAT_F32, MESH_PROJECT_FORMAT_U16, MESH_PROJECT_FORMAT_U8 = 0, 1, 2
MESH_PROJECT_MODE_BLEND, MESH_PROJECT_MODE_BEST = 0, 1
MESH_PROJECT_NORMALS_FACE, MESH_PROJECT_NORMALS_VERTEX = 0, 1
MESH_PROJECT_FORMATS = {"float32": MESH_PROJECT_FORMAT_F32, "uint16": MESH_PROJECT_FORMAT_U16, "uint8": MESH_PROJECT_FORMAT_U8}  # by numpy dtype name


class MeshProjectView(C.Structure):
    _fields_ = [
        ("view", View),
        ("image_dev", C.c_void_p),
        ("image_width", C.c_uint32),
        ("image_height", C.c_uint32),
        ("format", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class MeshProjectOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("size", C.c_uint32),
        ("block", C.c_uint32),
        ("mode", C.c_uint32),
        ("normals", C.c_uint32),
        ("weight_power", C.c_uint32),
        ("min_cos", C.c_float),
        ("depth_tolerance", C.c_float),
        ("near", C.c_float),
        ("cull", C.c_uint32),
        ("fallback_dev", C.c_void_p),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshProjection(C.Structure):
    _fields_ = [
        ("uv", C.c_void_p),
        ("color", C.c_void_p),
        ("info", C.c_void_p),
        ("size", C.c_uint32),
        ("block", C.c_uint32),
        ("blocks_per_row", C.c_uint32),
        ("n_tris", C.c_uint32),
    ]


class MeshProjectStats(C.Structure):
    _fields_ = [
        ("n_texels", C.c_uint64),
        ("n_textured", C.c_uint64),
        ("n_pairs_tested", C.c_uint64),
        ("n_occluded", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_PROJECT_PROTOTYPES = {
    "mesh_project_abi_version": (_u32, []),
    "mesh_project_default_options": (_i, [C.POINTER(MeshProjectOptions)]),
    "mesh_project_views": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshProjectView), _u32, C.POINTER(MeshProjectOptions), C.POINTER(MeshProjection), C.POINTER(MeshProjectStats)]),
    "mesh_projection_free": (_i, [_ctx, C.POINTER(MeshProjection)]),
}


# ---- include/rnb_mesh_draw.h: a device mesh with a texture atlas into one camera, in the rasteriser's channel layout; a header of its own with its own version (the HIP library only) ----
MESH_DRAW_ABI_VERSION = 1
MESH_DRAW_FILTER_NEAREST, MESH_DRAW_FILTER_BILINEAR = 0, 1


class MeshDrawTexture(C.Structure):
    _fields_ = [
        ("uv_dev", C.c_void_p),
        ("color_dev", C.c_void_p),
        ("normal_dev", C.c_void_p),
        ("size", C.c_uint32),
        ("n_tris", C.c_uint32),
    ]


class MeshDrawOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("near", C.c_float),
        ("cull", C.c_uint32),
        ("normals", C.c_uint32),
        ("filter", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshDrawStats(C.Structure):
    _fields_ = [
        ("raster", MeshRasterStats),
        ("n_bad_uv", C.c_uint32),
        ("n_normal_fallback", C.c_uint32),
        ("n_unowned_taps", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        """The rasteriser's fields flat, as DeviceMesh.rasterize returns them, and the three counts of the draw."""
        return dict(self.raster.as_dict(), n_bad_uv=self.n_bad_uv, n_normal_fallback=self.n_normal_fallback, n_unowned_taps=self.n_unowned_taps)


MESH_DRAW_PROTOTYPES = {
    "mesh_draw_abi_version": (_u32, []),
    "mesh_draw_default_options": (_i, [C.POINTER(MeshDrawOptions)]),
    "mesh_draw_textured": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshDrawTexture), C.POINTER(View), C.POINTER(MeshDrawOptions), C.c_void_p, C.c_void_p, C.POINTER(MeshDrawStats)]),
}

# ---- include/rnb_mesh_topology.h: the edge census and the repair of a device mesh, a header of its own with its own version (the HIP library only) ----
MESH_TOPOLOGY_ABI_VERSION = 1
MESH_TOPOLOGY_NONE, MESH_TOPOLOGY_MAX_BUCKET = 0xFFFFFFFF, 65536
MESH_DUPLICATES_KEEP, MESH_DUPLICATES_FIRST, MESH_DUPLICATES_CANCEL = 0, 1, 2
MESH_REPAIR_ORIENT_NONE, MESH_REPAIR_ORIENT_CONSISTENT = 0, 1


class MeshTopologyOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("buckets_log2", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshTopologyComponent(C.Structure):
    _fields_ = [
        ("label", C.c_uint32),
        ("n_vertices", C.c_uint32),
        ("n_edges", C.c_uint32),
        ("n_triangles", C.c_uint32),
        ("n_boundary_edges", C.c_uint32),
        ("n_nonmanifold_edges", C.c_uint32),
        ("n_inconsistent_edges", C.c_uint32),
        ("n_patches", C.c_uint32),
        ("euler", C.c_int32),
        ("genus", C.c_int32),
    ]


# the same record as a numpy dtype (DeviceMesh.topology returns the table as a structured array)
MESH_TOPOLOGY_COMPONENT_DTYPE = [(name, "<i4" if name in ("euler", "genus") else "<u4") for name, _ in MeshTopologyComponent._fields_]


class MeshTopologyStats(C.Structure):
    _fields_ = [
        ("n_verts_used", C.c_uint32),
        ("n_tris", C.c_uint32),
        ("n_degenerate", C.c_uint32),
        ("n_edges", C.c_uint32),
        ("n_boundary_edges", C.c_uint32),
        ("n_manifold_edges", C.c_uint32),
        ("n_nonmanifold_edges", C.c_uint32),
        ("n_inconsistent_edges", C.c_uint32),
        ("max_faces_on_edge", C.c_uint32),
        ("n_duplicate_tris", C.c_uint32),
        ("n_folded_pairs", C.c_uint32),
        ("n_components", C.c_uint32),
        ("n_patches", C.c_uint32),
        ("n_unorientable_patches", C.c_uint32),
        ("n_boundary_components", C.c_uint32),
        ("closed", C.c_uint32),
        ("oriented", C.c_uint32),
        ("reserved", C.c_uint32),
        ("euler", C.c_int64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved2", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


class MeshRepairOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("weld", C.c_uint32),
        ("drop_degenerate", C.c_uint32),
        ("duplicates", C.c_uint32),
        ("orient", C.c_uint32),
        ("buckets_log2", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshRepairStats(C.Structure):
    _fields_ = [
        ("n_welded", C.c_uint32),
        ("n_degenerate_dropped", C.c_uint32),
        ("n_duplicates_dropped", C.c_uint32),
        ("n_flipped", C.c_uint32),
        ("n_patches", C.c_uint32),
        ("n_unorientable_patches", C.c_uint32),
        ("n_verts_in", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_in", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_TOPOLOGY_PROTOTYPES = {
    "mesh_topology_abi_version": (_u32, []),
    "mesh_topology_default_options": (_i, [C.POINTER(MeshTopologyOptions)]),
    "mesh_topology": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshTopologyOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(MeshTopologyStats)]),
    "mesh_topology_table_free": (_i, [_ctx, C.c_void_p]),
    "mesh_repair_default_options": (_i, [C.POINTER(MeshRepairOptions)]),
    "mesh_repair": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshRepairOptions), C.POINTER(Mesh), C.c_void_p, C.POINTER(MeshRepairStats)]),
}

# ---- include/rnb_mesh_holes.h: the boundary loops of a device mesh and their fill, a header of its own with its own version (the HIP library only) ----
MESH_HOLES_ABI_VERSION = 1
MESH_HOLES_MAX_EDGES, MESH_HOLES_Q_SHIFT, MESH_HOLES_Q_TERM_LOG2 = 1 << 20, 32, 10


class MeshBoundaryLoopsOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("buckets_log2", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshBoundaryLoop(C.Structure):
    _fields_ = [
        ("label", C.c_uint32),
        ("n_edges", C.c_uint32),
        ("simple", C.c_uint32),
        ("n_irregular", C.c_uint32),
        ("component", C.c_uint32),
        ("centroid", C.c_float * 3),
        ("normal", C.c_float * 3),
        ("reserved", C.c_uint32),
        ("perimeter", C.c_double),
        ("area", C.c_double),
    ]


# the same record as a numpy dtype (DeviceMesh.boundary_loops returns the table as a structured array)
MESH_BOUNDARY_LOOP_DTYPE = [("label", "<u4"), ("n_edges", "<u4"), ("simple", "<u4"), ("n_irregular", "<u4"), ("component", "<u4"), ("centroid", "<f4", (3,)), ("normal", "<f4", (3,)),
                            ("reserved", "<u4"), ("perimeter", "<f8"), ("area", "<f8")]


class MeshBoundaryLoopsStats(C.Structure):
    _fields_ = [
        ("n_boundary_edges", C.c_uint32),
        ("n_loops", C.c_uint32),
        ("n_simple", C.c_uint32),
        ("n_irregular_vertices", C.c_uint32),
        ("max_loop_edges", C.c_uint32),
        ("n_too_long", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


class MeshFillHolesOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("max_edges", C.c_uint32),
        ("skip_largest", C.c_uint32),
        ("buckets_log2", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshFillHolesStats(C.Structure):
    _fields_ = [
        ("n_loops", C.c_uint32),
        ("n_filled", C.c_uint32),
        ("n_skipped_not_simple", C.c_uint32),
        ("n_skipped_over_max", C.c_uint32),
        ("n_skipped_largest", C.c_uint32),
        ("n_verts_added", C.c_uint32),
        ("n_tris_added", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("reserved", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved2", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_HOLES_PROTOTYPES = {
    "mesh_holes_abi_version": (_u32, []),
    "mesh_boundary_loops_default_options": (_i, [C.POINTER(MeshBoundaryLoopsOptions)]),
    "mesh_boundary_loops": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshBoundaryLoopsOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(MeshBoundaryLoopsStats)]),
    "mesh_boundary_loops_free": (_i, [_ctx, C.c_void_p]),
    "mesh_fill_holes_default_options": (_i, [C.POINTER(MeshFillHolesOptions)]),
    "mesh_fill_holes": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshFillHolesOptions), C.POINTER(Mesh), C.c_void_p, C.POINTER(MeshFillHolesStats)]),
}

# ---- include/rnb_mesh_intersect.h: the self-intersections of a device mesh and the mesh without them, a header of its own with its own version (the HIP library only) ----
MESH_INTERSECT_ABI_VERSION = 1
MESH_INTERSECT_PROPER, MESH_INTERSECT_CONTACT = 1, 2
MESH_INTERSECT_MAX_RINGS, MESH_INTERSECT_MAX_CELLS = 8, 256
MESH_INTERSECT_PAIR_DTYPE = [("s", "<u4"), ("t", "<u4"), ("cls", "<u4")]  # rnb_mesh_intersect_pair, 12 bytes


class MeshIntersectOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("cells", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshIntersectStats(C.Structure):
    _fields_ = [
        ("n_tris", C.c_uint32),
        ("n_degenerate", C.c_uint32),
        ("n_tris_proper", C.c_uint32),
        ("n_tris_contact", C.c_uint32),
        ("n_same_set", C.c_uint64),
        ("n_candidates", C.c_uint64),
        ("n_pairs_proper", C.c_uint64),
        ("n_pairs_contact", C.c_uint64),
        ("n_coplanar_pairs", C.c_uint64),
        ("n_pairs_written_would_be", C.c_uint64),
        ("dims", C.c_uint32 * 3),
        ("n_large", C.c_uint32),
        ("cell", C.c_double),
        ("n_cell_entries", C.c_uint64),
        ("n_visited", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("ms_grid", C.c_float),
    ]

    def as_dict(self):
        return {name: (list(getattr(self, name)) if name == "dims" else getattr(self, name)) for name, _ in self._fields_}


class MeshIntersectSelectOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("classes", C.c_uint32),
        ("rings", C.c_uint32),
        ("drop_unused_vertices", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshIntersectSelectStats(C.Structure):
    _fields_ = [
        ("n_verts_in", C.c_uint32),
        ("n_verts_out", C.c_uint32),
        ("n_tris_in", C.c_uint32),
        ("n_tris_out", C.c_uint32),
        ("n_selected", C.c_uint32),
        ("n_tris_removed", C.c_uint32),
        ("n_verts_removed", C.c_uint32),
        ("reserved", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved2", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_INTERSECT_PROTOTYPES = {
    "mesh_intersect_abi_version": (_u32, []),
    "mesh_intersect_default_options": (_i, [C.POINTER(MeshIntersectOptions)]),
    "mesh_intersections": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshIntersectOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MeshIntersectStats)]),
    "mesh_intersections_select_default_options": (_i, [C.POINTER(MeshIntersectSelectOptions)]),
    "mesh_intersections_select": (_i, [_ctx, _stream, C.POINTER(Mesh), C.c_void_p, C.c_void_p, C.POINTER(MeshIntersectSelectOptions), C.POINTER(Mesh), C.POINTER(MeshIntersectSelectStats)]),
}


# ---- include/rnb_mesh_smooth.h: Taubin passes over the one-ring and ring normals of a device mesh, a header of its own with its own version (the HIP library only) ----
MESH_SMOOTH_ABI_VERSION = 1
MESH_SMOOTH_MAX_RING, MESH_SMOOTH_MAX_PASSES, MESH_SMOOTH_MAX_SELECT_RINGS = 1 << 20, 10000, 1024
MESH_SMOOTH_Q_SHIFT, MESH_SMOOTH_Q_TERM_LOG2, MESH_SMOOTH_NORMAL_Q_SHIFT, MESH_SMOOTH_NORMAL_Q_TERM_LOG2 = 32, 10, 40, 3
MESH_SMOOTH_KIND_UNUSED, MESH_SMOOTH_KIND_INTERIOR, MESH_SMOOTH_KIND_BOUNDARY, MESH_SMOOTH_KIND_NONMANIFOLD = 0, 1, 2, 3
MESH_SMOOTH_BOUNDARY_PIN, MESH_SMOOTH_BOUNDARY_SLIDE, MESH_SMOOTH_BOUNDARY_FREE = 0, 1, 2
MESH_SMOOTH_NORMALS_KEEP, MESH_SMOOTH_NORMALS_RECOMPUTE = 0, 1


class MeshSmoothOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("passes", C.c_uint32),
        ("lambda_", C.c_double),  # `lambda` in the header
        ("mu", C.c_double),
        ("boundary", C.c_uint32),
        ("select_rings", C.c_uint32),
        ("normals", C.c_uint32),
        ("buckets_log2", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshSmoothStats(C.Structure):
    _fields_ = [
        ("n_edges", C.c_uint32),
        ("n_interior", C.c_uint32),
        ("n_boundary", C.c_uint32),
        ("n_nonmanifold", C.c_uint32),
        ("n_unused", C.c_uint32),
        ("n_selected", C.c_uint32),
        ("n_moving", C.c_uint32),
        ("max_valence", C.c_uint32),
        ("passes", C.c_uint32),
        ("n_wide", C.c_uint32),
        ("max_displacement", C.c_double),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("ms_passes", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MeshVertexNormalsOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("flip", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshVertexNormalsStats(C.Structure):
    _fields_ = [
        ("n_zero", C.c_uint32),
        ("max_corners", C.c_uint32),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


MESH_SMOOTH_PROTOTYPES = {
    "mesh_smooth_abi_version": (_u32, []),
    "mesh_smooth_default_options": (_i, [C.POINTER(MeshSmoothOptions)]),
    "mesh_vertex_normals_default_options": (_i, [C.POINTER(MeshVertexNormalsOptions)]),
    "mesh_smooth": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshSmoothOptions), C.c_void_p, C.POINTER(Mesh), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MeshSmoothStats)]),
    "mesh_vertex_normals": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshVertexNormalsOptions), C.c_void_p, C.POINTER(MeshVertexNormalsStats)]),
}


# ---- include/rnb_mesh_snap.h: guarded Newton steps of a device mesh onto the model's SDF, a header of its own with its own version (the HIP library only) ----
MESH_SNAP_ABI_VERSION = 1
MESH_SNAP_MAX_ITERATIONS, MESH_SNAP_MAX_IN_FLIGHT, MESH_SNAP_RESIDUAL_LOG2, MESH_SNAP_Q_SHIFT = 64, 1 << 22, 8, 24
(MESH_SNAP_UNSELECTED, MESH_SNAP_CONVERGED, MESH_SNAP_UNFINISHED, MESH_SNAP_FLAT, MESH_SNAP_LEASHED, MESH_SNAP_OUTSIDE, MESH_SNAP_STALLED, MESH_SNAP_INVALID,
 MESH_SNAP_REVERTED) = range(9)
MESH_SNAP_STATE_NAMES = ("unselected", "converged", "unfinished", "flat", "leashed", "outside", "stalled", "invalid", "reverted")


class MeshSnapOptions(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("iterations", C.c_uint32),
        ("level", C.c_float),
        ("tolerance", C.c_float),
        ("max_step", C.c_float),
        ("max_displacement", C.c_float),
        ("min_gradient", C.c_float),
        ("attributes", C.c_uint32),
        ("use_inference_params", C.c_uint32),
        ("max_points_in_flight", C.c_uint32),
        ("reserved", C.c_uint32 * 4),
    ]


class MeshSnapStats(C.Structure):
    _fields_ = [
        ("n_selected", C.c_uint32),
        ("n_unselected", C.c_uint32),
        ("n_converged", C.c_uint32),
        ("n_unfinished", C.c_uint32),
        ("n_flat", C.c_uint32),
        ("n_leashed", C.c_uint32),
        ("n_outside", C.c_uint32),
        ("n_stalled", C.c_uint32),
        ("n_invalid", C.c_uint32),
        ("n_reverted", C.c_uint32),
        ("n_moved", C.c_uint32),
        ("rounds", C.c_uint32),
        ("max_displacement", C.c_double),
        ("max_before", C.c_double),
        ("max_after", C.c_double),
        ("sum_before_q", C.c_uint64),
        ("sum_after_q", C.c_uint64),
        ("n_network_points", C.c_uint64),
        ("peak_workspace", C.c_uint64),
        ("ms", C.c_float),
        ("ms_network", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


MESH_SNAP_PROTOTYPES = {
    "mesh_snap_abi_version": (_u32, []),
    "mesh_snap_default_options": (_i, [C.POINTER(MeshSnapOptions)]),
    "mesh_snap": (_i, [_ctx, _stream, C.POINTER(Mesh), C.POINTER(MeshSnapOptions), C.c_void_p, C.POINTER(Mesh), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MeshSnapStats)]),
}


class Functions:
    """Bound, typed entry points of one library."""

    def __init__(self, lib, prefix, tables=(PROTOTYPES,)):
        self.lib = lib
        self.prefix = prefix
        missing = []
        for name, (res, args) in [kv for t in tables for kv in t.items()]:
            try:
                fn = getattr(lib, prefix + name)
            except AttributeError:
                missing.append(prefix + name)
                continue
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)
        if missing:
            raise ImportError("library %s lacks symbols: %s" % (getattr(lib, "_name", lib), ", ".join(missing)))


def declare(lib, prefix="rnb_", render=False, mesh=False, mesh_clean=False, mesh_simplify=False, mesh_distance=False, mesh_raster=False, mesh_texture=False,
            mesh_visibility=False, mesh_project=False, mesh_draw=False, mesh_topology=False, mesh_holes=False, mesh_intersect=False, mesh_smooth=False, mesh_snap=False):
    """render=True also binds RENDER_PROTOTYPES (include/rnb_render.h), mesh=True MESH_PROTOTYPES (include/rnb_mesh.h), mesh_clean=True MESH_CLEAN_PROTOTYPES
    (include/rnb_mesh_clean.h), mesh_simplify=True MESH_SIMPLIFY_PROTOTYPES (include/rnb_mesh_simplify.h), mesh_distance=True MESH_DISTANCE_PROTOTYPES (include/rnb_mesh_distance.h),
    mesh_raster=True MESH_RASTER_PROTOTYPES (include/rnb_mesh_raster.h), mesh_texture=True MESH_TEXTURE_PROTOTYPES (include/rnb_mesh_texture.h),
    mesh_visibility=True MESH_VISIBILITY_PROTOTYPES (include/rnb_mesh_visibility.h), mesh_project=True MESH_PROJECT_PROTOTYPES (include/rnb_mesh_project.h),
    mesh_draw=True MESH_DRAW_PROTOTYPES (include/rnb_mesh_draw.h), mesh_topology=True MESH_TOPOLOGY_PROTOTYPES (include/rnb_mesh_topology.h),
    mesh_holes=True MESH_HOLES_PROTOTYPES (include/rnb_mesh_holes.h), mesh_intersect=True MESH_INTERSECT_PROTOTYPES (include/rnb_mesh_intersect.h),
    mesh_smooth=True MESH_SMOOTH_PROTOTYPES (include/rnb_mesh_smooth.h), mesh_snap=True MESH_SNAP_PROTOTYPES (include/rnb_mesh_snap.h); only the HIP library exports those."""
    return Functions(lib, prefix, (PROTOTYPES,) + ((RENDER_PROTOTYPES,) if render else ()) + ((MESH_PROTOTYPES,) if mesh else ()) + ((MESH_CLEAN_PROTOTYPES,) if mesh_clean else ())
                     + ((MESH_SIMPLIFY_PROTOTYPES,) if mesh_simplify else ()) + ((MESH_DISTANCE_PROTOTYPES,) if mesh_distance else ()) + ((MESH_RASTER_PROTOTYPES,) if mesh_raster else ())
                     + ((MESH_TEXTURE_PROTOTYPES,) if mesh_texture else ()) + ((MESH_VISIBILITY_PROTOTYPES,) if mesh_visibility else ())
                     + ((MESH_PROJECT_PROTOTYPES,) if mesh_project else ()) + ((MESH_DRAW_PROTOTYPES,) if mesh_draw else ()) + ((MESH_TOPOLOGY_PROTOTYPES,) if mesh_topology else ()) + ((MESH_HOLES_PROTOTYPES,) if mesh_holes else ())
                     + ((MESH_INTERSECT_PROTOTYPES,) if mesh_intersect else ()) + ((MESH_SMOOTH_PROTOTYPES,) if mesh_smooth else ()) + ((MESH_SNAP_PROTOTYPES,) if mesh_snap else ()))
