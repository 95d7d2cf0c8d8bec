/*
 * rnb_mesh_holes.h — C-ABI of the hole stage of librnb_neus2_hip: the boundary of an indexed device mesh as ordered loops, and their closure. rnb_mesh_boundary_loops is
 * the census (per boundary half-edge: its component, its successor, its position on the loop; per boundary component: size, whether it is one simple cycle, centroid,
 * normal, perimeter, area); rnb_mesh_fill_holes returns a new mesh in which every selected simple loop is closed by a triangle (3 edges) or by a fan around a new
 * vertex at its centroid. It closes what the cull by what the cameras see (triangle by triangle) and rnb_mesh_repair (duplicates = cancel) open on purpose, and what
 * rnb_mesh_topology.h only counts (n_boundary_edges, n_boundary_components).
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: no other ABI is affected by this header.
 */
#ifndef RNB_MESH_HOLES_H
#define RNB_MESH_HOLES_H

#include "rnb_mesh_topology.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_HOLES_ABI_VERSION 1

#define RNB_MESH_HOLES_MAX_EDGES (1u << 20) /* a longer component is counted, has no sums and is never filled */
#define RNB_MESH_HOLES_Q_SHIFT 32           /* fixed point of the sums: q = (int64) trunc(term * 2^32) */
#define RNB_MESH_HOLES_Q_TERM_LOG2 10       /* a term must be finite and below 2^10 in magnitude */

/*
 * Definitions (both entry points).
 *
 * Triangles, half-edges (h = 3t + k, from corner k to corner (k + 1) % 3), degenerate triangles, edges and the faces on an edge are those of rnb_mesh_topology.h.
 *
 * A BOUNDARY HALF-EDGE is a half-edge of a non-degenerate triangle whose edge has exactly one face. It runs from a(h) = indices[h] to b(h) = indices[3t + (k + 1) % 3].
 * A BOUNDARY COMPONENT is a class of the boundary edges under "share a vertex" (what rnb_mesh_topology counts as n_boundary_components); its LABEL is its
 * lowest boundary half-edge, its vertices are the ends of its edges. A vertex of a boundary component is REGULAR if exactly one boundary half-edge starts at it
 * and exactly one ends at it. A component is a SIMPLE LOOP if all its vertices are regular: it is then one directed cycle of n >= 3 edges. Any other component
 * (a pinch where two loops touch in a vertex, a rim whose faces are wound inconsistently) is NON-SIMPLE: it is reported and never filled; run
 * rnb_mesh_repair(orient = RNB_MESH_REPAIR_ORIENT_CONSISTENT) first where the winding is the cause.
 *
 * On a simple loop, next(h) is the boundary half-edge that starts at b(h), pos(label) = 0 and pos(next(h)) = pos(h) + 1; h_k is the half-edge at position k, a_k
 * and b_k its ends (b_k = a_(k+1), b_(n-1) = a_0), n the number of edges.
 *
 * Arithmetic: double precision, every operation rounded on its own (no contraction), floats widened first. A per-component sum S(term) runs over the component's
 * boundary half-edges in no particular order: every term becomes q = (int64) trunc(term * 2^32), the q are added as integers, and the sum is read as
 * (double) q_sum * 2^-32 (the conversion rounds to nearest even). A term that is not finite or not below 2^10 in magnitude fails the call with RNB_ERR_INVALID,
 * and so does a coordinate of a boundary vertex that is not finite. A sum cannot wrap while the component has at most RNB_MESH_HOLES_MAX_EDGES edges; a longer
 * component is TOO LONG: it is reported with label, n_edges, simple, n_irregular and component, its centroid, normal, perimeter and area are 0, and it is never
 * filled (its terms are checked all the same). With o = the position of a(label), a = the position of a(h), b = that of b(h):
 *   S(a - o)                  3 terms
 *   S(|b - a|)                |d| = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z), of d = b - a
 *   S(cross(b - o, a - o))    3 terms; cross(u, v) = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x): twice the area vector of the loop run
 *                             against the existing faces, i.e. of the side a fill faces
 *   S(colour of a)            3 terms, if the mesh has colours
 * and from them centroid[k] = (float)(S(a - o)[k] / n + o[k]); perimeter = S(|b - a|); with A = S(cross) and l = sqrt((A.x * A.x + A.y * A.y) + A.z * A.z):
 * area = 0.5 * l and normal[k] = (float)(A[k] / l), or 0 if l == 0.
 *
 * The groupings, their cost and the bucket-load guard are those of rnb_mesh_topology.h (the half-edges by edge); buckets_log2 must be 0 or 4 .. 30. Determinism:
 * the same input gives the same bits, whatever buckets_log2. Planarity and self-intersection of a fill are not examined here: a fan around the centroid of a strongly
 * non-planar or non-convex loop can fold over itself, and rnb_mesh_intersections (rnb_mesh_intersect.h) on the filled mesh reports where. A lone triangle's fill is its own reversed
 * copy, a folded pair. A filled loop of 3 edges makes an edge non-manifold only if the input already held a triangle on those three vertices.
 */

typedef struct rnb_mesh_boundary_loops_options {
	uint32_t abi_version;  /* RNB_MESH_HOLES_ABI_VERSION */
	uint32_t buckets_log2; /* as in rnb_mesh_topology_options */
	uint32_t reserved[4];  /* 0 */
} rnb_mesh_boundary_loops_options;

/* One record of the loop table: one boundary component. */
typedef struct rnb_mesh_boundary_loop {
	uint32_t label;       /* its lowest boundary half-edge */
	uint32_t n_edges;
	uint32_t simple;      /* 1: a simple loop */
	uint32_t n_irregular; /* its vertices that are not regular */
	uint32_t component;   /* the cleaner's label of its vertices (rnb_mesh_clean.h: the smallest vertex index of the connected component) */
	float    centroid[3];
	float    normal[3];
	uint32_t reserved;
	double   perimeter;
	double   area;
} rnb_mesh_boundary_loop;

typedef struct rnb_mesh_boundary_loops_stats {
	uint32_t n_boundary_edges;
	uint32_t n_loops;              /* boundary components = records in the table = n_boundary_components of rnb_mesh_topology */
	uint32_t n_simple;
	uint32_t n_irregular_vertices; /* the sum of n_irregular */
	uint32_t max_loop_edges;       /* 0 for a mesh without boundary */
	uint32_t n_too_long;           /* components of more than RNB_MESH_HOLES_MAX_EDGES edges */
	uint64_t peak_workspace;       /* bytes of device memory the call held at its peak, the table included */
	float    ms;                   /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_boundary_loops_stats;

uint32_t rnb_mesh_holes_abi_version(void);
/* Fills *opt with the defaults: buckets_log2 = 0. */
int rnb_mesh_boundary_loops_default_options(rnb_mesh_boundary_loops_options* opt);

/* The census. in: any indexed triangle mesh in device memory; it is not modified. Coordinates (and colours, if the mesh has them) are read of boundary vertices only.
 *
 * Per half-edge (each array optional, caller-allocated device memory of n_indices words, written in input order):
 *   loop_dev[h]  the label of h's component for a boundary half-edge, RNB_MESH_TOPOLOGY_NONE for any other
 *   next_dev[h]  next(h) for a boundary half-edge of a simple loop, RNB_MESH_TOPOLOGY_NONE for any other
 *   pos_dev[h]   pos(h), likewise
 * The table (table_dev != NULL) is device memory holding stats->n_loops records in ascending label (ask for the statistics with it), released with
 * rnb_mesh_boundary_loops_free.
 *
 * Fails with RNB_ERR_INVALID as rnb_mesh_topology does (n_indices % 3 != 0; an index >= n_verts, range-checked by a kernel before any is used as an address; the
 * bucket guard), and on a coordinate or a term as said above. A mesh without triangles or without boundary succeeds: all counts 0, an empty table, the per-half-edge
 * arrays RNB_MESH_TOPOLOGY_NONE. On failure *table_dev is NULL. Every argument is validated before the context or the device is touched. Workspace (released before
 * the call returns): eight words per vertex, two per triangle and three per half-edge; 2^b words of buckets; eight per boundary half-edge; 36 per loop. Work pending on
 * the context's side streams is joined first; reads nothing of the training state. A handful of small device-to-host reads; syncs. The loops are ordered by list
 * ranking in ceil(log2(longest simple loop)) rounds, a number fixed on the host. */
int rnb_mesh_boundary_loops(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_boundary_loops_options* opt, uint32_t* loop_dev /* may be NULL */,
                            uint32_t* next_dev /* may be NULL */, uint32_t* pos_dev /* may be NULL */, rnb_mesh_boundary_loop** table_dev /* may be NULL */,
                            rnb_mesh_boundary_loops_stats* stats /* may be NULL */);
/* Releases a table rnb_mesh_boundary_loops returned (NULL is accepted). */
int rnb_mesh_boundary_loops_free(rnb_ctx* ctx, rnb_mesh_boundary_loop* table_dev);

typedef struct rnb_mesh_fill_holes_options {
	uint32_t abi_version;  /* RNB_MESH_HOLES_ABI_VERSION */
	uint32_t max_edges;    /* 0 (default): every simple loop of up to RNB_MESH_HOLES_MAX_EDGES edges; else only those with n_edges <= max_edges */
	uint32_t skip_largest; /* 0 (default) or 1: of every connected component (the cleaner's) the one simple loop with the most edges stays open, on a tie the one of
	                          the lowest label: the rim of a relief, or of a scan that stands on a table */
	uint32_t buckets_log2; /* as in rnb_mesh_topology_options */
	uint32_t reserved[4];  /* 0 */
} rnb_mesh_fill_holes_options;

typedef struct rnb_mesh_fill_holes_stats {
	uint32_t n_loops;              /* boundary components of the input; each is filled or counted by exactly one of the next three, the first that applies */
	uint32_t n_filled;
	uint32_t n_skipped_not_simple;
	uint32_t n_skipped_over_max;   /* simple, but longer than max_edges or RNB_MESH_HOLES_MAX_EDGES */
	uint32_t n_skipped_largest;    /* left open by skip_largest (the largest simple loop of a component is looked for among all its simple loops) */
	uint32_t n_verts_added;        /* filled loops of more than 3 edges */
	uint32_t n_tris_added;
	uint32_t n_verts_out;
	uint32_t n_tris_out;
	uint32_t reserved;
	uint64_t peak_workspace;       /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;
	uint32_t reserved2;
} rnb_mesh_fill_holes_stats;

/* Fills *opt with the defaults: max_edges = 0, skip_largest = 0, buckets_log2 = 0. */
int rnb_mesh_fill_holes_default_options(rnb_mesh_fill_holes_options* opt);

/* The fill. in: any indexed triangle mesh in device memory; it is not modified and must not be *out. The loops are those of rnb_mesh_boundary_loops on the same
 * mesh; the FILLED ones are the simple loops the options select.
 *
 * Output vertices: all input vertices, in input order, with their attributes, those no triangle uses included (this stage does not compact); then one vertex per
 * filled loop of more than 3 edges, in ascending label: its position is the loop's centroid, its colour (float)(S(colour)[k] / n), its normal the loop's normal.
 * out->colors / out->normals are set exactly when the input has them.
 * Output triangles: all input triangles, in input order, unchanged; then, for each filled loop in ascending label, the triangle (b_0, a_0, a_2) and no new vertex if
 * n == 3, else the n triangles (b_k, a_k, c), k = 0 .. n-1, c the loop's new vertex. Each runs its boundary edge against the existing face, so a consistently wound
 * input stays consistently wound.
 * loop_of_tri_dev (optional, caller-allocated device memory of n_tris_out words; n_tris_in plus the input's boundary half-edges is always enough): the label of the
 * loop an output triangle was made for, RNB_MESH_TOPOLOGY_NONE for an input triangle.
 *
 * Failures as for rnb_mesh_boundary_loops; also skip_largest > 1, and an output of 2^32 / 3 triangles or more. A mesh without triangles or without boundary
 * succeeds with a copy of the input. On success *out owns its device buffers: release them with rnb_mesh_free. On failure *out is zeroed. Workspace: that of the
 * census, two words per vertex, three per loop and the output. */
int rnb_mesh_fill_holes(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_fill_holes_options* opt, rnb_mesh* out, uint32_t* loop_of_tri_dev /* may be NULL */,
                        rnb_mesh_fill_holes_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_HOLES_H */
