/*
 * rnb_mesh_clean.h — C-ABI of the mesh cleaner of librnb_neus2_hip: connected components of an indexed triangle mesh in device memory, the largest one kept,
 * its triangles turned outward. It replaces the last stage of the pipeline (trimesh.split + max(area) + fix_normals in the reference, meshproc.py here) for a mesh
 * that already lives on the device, e.g. the one rnb_extract_mesh (rnb_mesh.h) returns.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI
 * and the mesh ABI are not affected by this header.
 */
#ifndef RNB_MESH_CLEAN_H
#define RNB_MESH_CLEAN_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_CLEAN_ABI_VERSION 1

#define RNB_MESH_KEEP_ALL 0     /* every component; only the vertices no triangle uses disappear */
#define RNB_MESH_KEEP_LARGEST 1 /* the component of the greatest fixed-point area; equal areas: the smallest label */

#define RNB_MESH_ORIENT_NONE 0    /* triangles as they come */
#define RNB_MESH_ORIENT_OUTWARD 1 /* the triangles of a kept component whose fixed-point signed volume is negative get their second and third index swapped */

/* Fixed point of the per-triangle terms: q = (int64) trunc(term * 2^RNB_MESH_Q_SHIFT), rounding towards zero. 2^-44 is 5.7e-14: the smallest triangle of a 4096^3
 * lattice over a box of edge 1 has area 2^-25 = 2^19 units. A term must be finite and smaller than 2^RNB_MESH_Q_TERM_LOG2 in magnitude (else the call fails), and
 * a sum cannot overflow while the sum of the magnitudes of its terms stays below 2^(63 - RNB_MESH_Q_SHIFT) = 524 288 (square or cubic mesh units). */
#define RNB_MESH_Q_SHIFT 44
#define RNB_MESH_Q_TERM_LOG2 18

#define RNB_MESH_NO_LABEL 0xFFFFFFFFu

typedef struct rnb_mesh_clean_options {
	uint32_t abi_version; /* RNB_MESH_CLEAN_ABI_VERSION */
	uint32_t keep;        /* RNB_MESH_KEEP_LARGEST (default) or RNB_MESH_KEEP_ALL */
	uint32_t orient;      /* RNB_MESH_ORIENT_OUTWARD (default) or RNB_MESH_ORIENT_NONE */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_clean_options;

/* One record of the component table. */
typedef struct rnb_mesh_component {
	uint32_t label;       /* the smallest vertex index of the component */
	uint32_t n_vertices;
	uint32_t n_triangles;
	uint32_t kept;        /* 1: its vertices and triangles are in the output */
	int64_t  area_q;      /* fixed-point area (below) */
	int64_t  volume_q;    /* fixed-point signed volume of the triangles as they came in (before any swap) */
} rnb_mesh_component;

typedef struct rnb_mesh_clean_stats {
	uint32_t n_components;   /* components found = records in the table */
	uint32_t n_kept;         /* components in the output */
	uint32_t n_verts_in;
	uint32_t n_verts_out;
	uint32_t n_tris_in;
	uint32_t n_tris_out;
	uint32_t largest_label;  /* label of the component KEEP_LARGEST selects (whatever `keep` is); RNB_MESH_NO_LABEL for an empty mesh */
	uint32_t hook_passes;    /* launches of the hooking kernel: 1 for every non-empty input (below), 0 for an empty one */
	uint32_t flatten_passes; /* launches of the flattening kernel: likewise */
	uint32_t reserved;
	int64_t  area_q_in;      /* fixed-point area of all components */
	int64_t  area_q_out;     /* and of the kept ones */
	uint64_t peak_workspace; /* bytes of device memory the call held at its peak, the returned mesh and table included */
	float    ms;             /* wall-clock time of the call */
	uint32_t reserved2;
} rnb_mesh_clean_stats;

uint32_t rnb_mesh_clean_abi_version(void);
/* Fills *opt with the defaults: keep the largest component, orient outward. */
int rnb_mesh_clean_default_options(rnb_mesh_clean_options* opt);

/* in: any indexed triangle mesh in device memory (verts, indices, optionally colors and / or normals); it is not modified and must not be *out.
 *
 * Component. The classes of the closure of "two vertices are corners of one triangle". A vertex no triangle uses belongs to no component and is never in *out. Two
 * vertices at one position are two vertices (nothing is welded). The label of a component is its smallest vertex index. n_indices % 3 != 0 or an index >= n_verts
 * fails with RNB_ERR_INVALID (the indices are range-checked by a kernel before any of them is used as an address and before anything is allocated for *out).
 *
 * Area and signed volume of a component: sums over its triangles (a, b, c) of per-triangle terms, each computed in double precision from the float coordinates with
 * every operation rounded on its own (no fused multiply-add), converted to fixed point (RNB_MESH_Q_SHIFT above) and added as 64-bit integers, so that the sums do
 * not depend on the order of the additions:
 *   u = b - a, v = c - a, n = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x), area = 0.5 * sqrt((n.x * n.x + n.y * n.y) + n.z * n.z)
 *   m = (b.y * c.z - b.z * c.y, b.z * c.x - b.x * c.z, b.x * c.y - b.y * c.x), volume = ((a.x * m.x + a.y * m.y) + a.z * m.z) / 6
 * A term that is not finite or not below 2^RNB_MESH_Q_TERM_LOG2 in magnitude fails the call with RNB_ERR_INVALID.
 *
 * keep: RNB_MESH_KEEP_ALL or RNB_MESH_KEEP_LARGEST. orient: RNB_MESH_ORIENT_OUTWARD swaps the second and third index of every triangle of a kept component whose
 * volume_q is negative. The input is taken to be consistently wound inside each component, as marching-cubes output is: the winding is not repaired across edges
 * (rnb_mesh_repair of rnb_mesh_topology.h does that, and welds: run it first on a mesh that needs either).
 * Vertex attributes are carried unchanged (out->colors / out->normals are set exactly when the input has them).
 *
 * Order: kept vertices in input order, kept triangles in input order, indices renumbered (prefix sums, no atomics). The same input gives the same bits, and a
 * permutation of the input's triangles permutes the output's triangles and changes nothing else.
 *
 * Table (table_dev != NULL): *table_dev receives device memory holding stats->n_components records, ascending label (ask for the statistics with it); release it
 * with rnb_mesh_clean_table_free. area_q and volume_q of the table are the sums above.
 *
 * Passes: the labels come from a union-find over the vertices. The hooking kernel (one thread per triangle) hooks the larger root under the smaller with a 32-bit
 * compare-and-swap and retries a lost one itself, so ONE launch unites everything, and ONE flattening launch points every vertex at its root: hook_passes = 1 and
 * flatten_passes = 1 for every non-empty input. A root is only ever hooked under a smaller one, so the final root is the smallest vertex whatever the order of arrival.
 *
 * An empty input (n_indices == 0) succeeds with an empty *out. On success *out owns its device buffers: release them with rnb_mesh_free. On failure *out is zeroed
 * and *table_dev is NULL. Workspace: three 4-byte words per input vertex, one per 256 triangles, the block sums of the prefix sums (one word per 1024 of those), 36 bytes per
 * component, a 32-byte result record and the output; released before the call returns. Reads nothing of the training state; work pending on the context's side streams is joined first. Every argument is validated before the context or the
 * device is touched. A handful of small device-to-host reads; syncs. */
int rnb_mesh_clean(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_clean_options* opt, rnb_mesh* out, rnb_mesh_component** table_dev /* may be NULL */,
                   rnb_mesh_clean_stats* stats /* may be NULL */);
/* Releases a table rnb_mesh_clean returned (NULL is accepted). */
int rnb_mesh_clean_table_free(rnb_ctx* ctx, rnb_mesh_component* table_dev);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_CLEAN_H */
