/*
 * rnb_mesh.h — C-ABI of the sparse mesh extractor of librnb_neus2_hip: the iso-surface of the SDF network, extracted brick by brick, with the bricks
 * the occupancy bitfield marks empty skipped, welded across brick faces, with vertex colours and SDF-gradient normals, all on the device. It stands
 * beside rnb_sdf_lattice + rnb_marching_cubes (rnb_neus2.h), which evaluate and hold the whole lattice; those are unchanged.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI
 * (RNB_ABI_VERSION) and the render ABI are not affected by this header.
 */
#ifndef RNB_MESH_H
#define RNB_MESH_H

#include "rnb_neus2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_ABI_VERSION 1

#define RNB_MESH_CULL_NONE 0      /* every brick is kept */
#define RNB_MESH_CULL_OCCUPANCY 1 /* a brick is kept if an occupancy cell whose bit is set can touch it (below) */

#define RNB_MESH_ATTR_COLORS 1u  /* bit 0: vertex colours */
#define RNB_MESH_ATTR_NORMALS 2u /* bit 1: SDF-gradient normals */

#define RNB_MESH_MAX_RES 4096u /* lattice points per axis */

typedef struct rnb_mesh_options {
	uint32_t abi_version;          /* RNB_MESH_ABI_VERSION */
	uint32_t res[3];               /* lattice points per axis, 1 .. RNB_MESH_MAX_RES */
	float    lattice_min;          /* the lattice of rnb_sdf_lattice: point p of axis k is queried at p / res[k] * (lattice_max - lattice_min) + lattice_min */
	float    lattice_max;
	float    aabb_min[3];          /* as rnb_marching_cubes: point p lies at aabb_min + p * (aabb_max - aabb_min) / res in the mesh */
	float    aabb_max[3];
	float    thresh;               /* as rnb_marching_cubes */
	uint32_t use_inference_params; /* 1 (default) = the EMA weights (what a snapshot holds), 0 = the training weights */
	uint32_t cull;                 /* RNB_MESH_CULL_OCCUPANCY (default) or RNB_MESH_CULL_NONE */
	uint32_t brick;                /* lattice points per brick edge: a power of two, 8 .. 64; 0 = the library's default (16) */
	uint32_t attributes;           /* RNB_MESH_ATTR_* bits; default 0 */
	uint32_t max_points_in_flight; /* 0 = default (2^22). Lattice points per network launch = the size of the position staging buffer (rounded down to whole
	                                  bricks, one brick at least). The mesh does not depend on it */
	uint64_t max_active_points;    /* 0 = no limit. A guard on the lattice points whose values are held at once (evaluated bricks * brick^3): above it the call
	                                  fails with RNB_ERR_NOMEM and a message naming the number it would have needed, before it allocates them */
	uint32_t reserved[4];          /* 0 */
} rnb_mesh_options;

typedef struct rnb_mesh {
	float*    verts;     /* device, float[n_verts][3] */
	uint32_t* indices;   /* device, uint32[n_indices], three per triangle */
	float*    colors;    /* device, float[n_verts][3], or NULL when not asked for */
	float*    normals;   /* device, float[n_verts][3], or NULL when not asked for */
	uint32_t  n_verts;
	uint32_t  n_indices;
} rnb_mesh;

typedef struct rnb_mesh_stats {
	uint64_t n_bricks;           /* bricks in the lattice */
	uint64_t n_kept;             /* bricks the cull rule keeps */
	uint64_t n_evaluated;        /* bricks whose lattice points went through the network: the kept ones and the neighbours their cells reach into */
	uint64_t n_sign_change;      /* evaluated bricks that kept their edge table (below) */
	uint64_t n_points_evaluated; /* n_evaluated * brick^3 (the points of a ragged brick that lie outside the lattice are evaluated at clamped indices and not used) */
	uint64_t peak_workspace;     /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;                 /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_stats;

uint32_t rnb_mesh_abi_version(void);
/* Fills *opt with the defaults above: res 256^3, the lattice and the box [0, 1]^3, thresh 0, EMA weights, cull by occupancy, no attributes. */
int rnb_mesh_default_options(rnb_mesh_options* opt);

/* Let D be the mesh rnb_sdf_lattice + rnb_marching_cubes produce for the same lattice, box, threshold and weights. The lattice points are partitioned into
 * bricks of brick^3 (the last brick of an axis may be ragged); a marching-cubes cell belongs to the brick of its lowest corner.
 *
 * Which bricks are kept. RNB_MESH_CULL_NONE: all. RNB_MESH_CULL_OCCUPANCY: a brick is kept if and only if its closed box, grown by one lattice step on every
 * side -- per axis [w(first - 1), w(last + 1)] with w(p) = lattice_min + p / res * (lattice_max - lattice_min) evaluated in double precision -- intersects
 * (closed: touching counts) the closed box of at least one occupancy cell whose bit is set and that the march can consult: cell i of cascade m spans
 * 0.5 + (i - 64) * 2^m / 128 .. 0.5 + (i - 63) * 2^m / 128 per axis, and a cell of cascade m >= 1 that lies inside the cube of cascade m - 1 is never consulted
 * (a position is classified by the finest cascade that contains it: mip_from_pos, src/common_device.cuh). Space outside the coarsest cascade is empty.
 * The bitfield is read as the march reads it (RNB_BUF_DENSITY_BITFIELD, all cascades), a caller-written one included.
 *
 * Which bricks are evaluated: the kept ones and, for each, the up to seven neighbours at +1 along any subset of the axes (the far corners of its cells). An
 * evaluated brick keeps its edge table (and counts in n_sign_change) if the lattice points of its box grown by one step towards +x, +y, +z that are inside the
 * lattice and inside an evaluated brick do not all lie on one side of thresh.
 *
 * The mesh. Triangles: exactly the triangles of D whose cell belongs to a kept brick. Vertices: exactly the vertices of D those triangles use, each once (welded
 * across brick faces), with bit-identical positions: the values come from the point-query kernel of rnb_sdf_lattice at the same float positions and the
 * interpolation uses global lattice coordinates in the arithmetic of rnb_marching_cubes. With RNB_MESH_CULL_NONE the mesh is D up to the order below (and up to
 * the vertices of D no triangle uses, which only a lattice one point thick has).
 *
 * Order (deterministic; prefix sums, no atomics): brick-major. Bricks ascend by bx + nbx * (by + nby * bz); inside a brick lattice points ascend by
 * lx + brick * (ly + brick * lz). Vertices: by the brick and point that carries the edge (its lower end), then axis x, y, z. Triangles: by the brick and point of
 * the cell's lowest corner, then the case table's order. The same state gives the same buffers, for any max_points_in_flight.
 *
 * Colours (RNB_MESH_ATTR_COLORS): the network's outputs 0..2 at the vertex through the logistic, with the view direction pointing outwards from (0.5, 0.5, 0.5)
 * (Testbed::compute_mesh_vertex_colors, src/testbed_nerf.cu:4193-4216). Normals (RNB_MESH_ATTR_NORMALS): the normalised SDF gradient at the vertex (outputs 4..6,
 * the normal of rnb_render's channels 0-2), zero where the gradient is zero.
 *
 * Memory: one 4-byte word per brick; lattice values (2 bytes per point) for evaluated bricks; edge tables (12 bytes per point) for the n_sign_change bricks;
 * nothing else grows with the lattice. On success *out owns its device buffers (two to four): release them with rnb_mesh_free. On failure *out is zeroed.
 * Reads the network weights and the occupancy bitfield only: the training state is left as it was; work pending on the context's side streams is joined first.
 * A handful of 4-byte device-to-host reads (the counts) and one read of the brick words (the kept count of the statistics); syncs. */
int rnb_extract_mesh(rnb_ctx* ctx, void* stream, const rnb_mesh_options* opt, rnb_mesh* out, rnb_mesh_stats* stats /* may be NULL */);
/* Releases the buffers of *mesh and zeroes it. */
int rnb_mesh_free(rnb_ctx* ctx, rnb_mesh* mesh);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_H */
