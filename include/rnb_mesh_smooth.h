/*
 * rnb_mesh_smooth.h — C-ABI of the smoothing stage of librnb_neus2_hip: the vertices of an indexed device mesh moved towards the centroids of their one-rings by
 * Taubin's pairs of passes (rnb_mesh_smooth), and area-weighted vertex normals from the one-ring of triangles (rnb_mesh_vertex_normals). It fairs what the other
 * stages leave behind: the lattice-frequency ripples of marching cubes, the staircase of the cell grid rnb_mesh_simplify places its vertices on, and the flat fans
 * rnb_mesh_fill_holes closes a loop with (rnb_mesh_holes.h). It reads the mesh only; no model is evaluated.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: no other ABI is affected by this header.
 */
#ifndef RNB_MESH_SMOOTH_H
#define RNB_MESH_SMOOTH_H

#include "rnb_mesh_topology.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_SMOOTH_ABI_VERSION 1

#define RNB_MESH_SMOOTH_MAX_RING (1u << 20)  /* the most terms one vertex may have in a sum */
#define RNB_MESH_SMOOTH_MAX_PASSES 10000u
#define RNB_MESH_SMOOTH_MAX_SELECT_RINGS 1024u
#define RNB_MESH_SMOOTH_Q_SHIFT 32           /* the passes: q = (int64) trunc(term * 2^32) */
#define RNB_MESH_SMOOTH_Q_TERM_LOG2 10       /* a term of a pass must be finite and below 2^10 in magnitude */
#define RNB_MESH_SMOOTH_NORMAL_Q_SHIFT 40    /* the normals: q = (int64) trunc(term * 2^40) */
#define RNB_MESH_SMOOTH_NORMAL_Q_TERM_LOG2 3 /* a term of a normal must be finite and below 2^3 in magnitude */

/* kind of a vertex */
#define RNB_MESH_SMOOTH_KIND_UNUSED 0u
#define RNB_MESH_SMOOTH_KIND_INTERIOR 1u
#define RNB_MESH_SMOOTH_KIND_BOUNDARY 2u
#define RNB_MESH_SMOOTH_KIND_NONMANIFOLD 3u

/* rnb_mesh_smooth_options::boundary */
#define RNB_MESH_SMOOTH_BOUNDARY_PIN 0u   /* boundary vertices stay */
#define RNB_MESH_SMOOTH_BOUNDARY_SLIDE 1u /* a boundary vertex moves towards the centroid of its neighbours along the boundary: the rim is smoothed as a curve */
#define RNB_MESH_SMOOTH_BOUNDARY_FREE 2u  /* a boundary vertex moves like an interior one (the rim shrinks inwards) */

/* rnb_mesh_smooth_options::normals */
#define RNB_MESH_SMOOTH_NORMALS_KEEP 0u      /* the input's normals are carried, if it has them */
#define RNB_MESH_SMOOTH_NORMALS_RECOMPUTE 1u /* out->normals = rnb_mesh_vertex_normals of the output */

/*
 * Definitions (both entry points).
 *
 * Triangles, degenerate triangles, half-edges (h = 3t + k), edges and the faces on an edge are those of rnb_mesh_topology.h. E is the set of undirected edges {a, b}
 * of the non-degenerate triangles; an edge is in E once, however many faces lie on it. A BOUNDARY EDGE is an edge with exactly one face.
 *   N(v)    the other ends of the edges of E at v; valence(v) = |N(v)|
 *   N_b(v)  the other ends of the boundary edges at v
 *
 * KIND of a vertex, the first that applies: UNUSED, valence 0 (a vertex only degenerate triangles use is unused); NONMANIFOLD, on an edge with 3 or more faces;
 * BOUNDARY, on an edge with 1 face; INTERIOR, any other.
 *
 * Arithmetic: double precision, every operation rounded on its own (no contraction), floats widened first. A per-vertex sum runs over its terms in no particular
 * order: every term becomes q = (int64) trunc(term * 2^SHIFT), the q are added as integers, and the sum is read as (double) q_sum * 2^-SHIFT (the conversion rounds to
 * nearest even). A term that is not finite, or not below the stated bound in magnitude, fails the call with RNB_ERR_INVALID (the flag is sticky on the device and
 * read once, after the last kernel), and so does a vertex with more than RNB_MESH_SMOOTH_MAX_RING terms in one sum; with that cap no sum can wrap. On failure *out is
 * zeroed. Because the sums are integers, nothing depends on how they are formed, on buckets_log2, or on the order of the triangles: the same input gives the same bits.
 *
 * rnb_mesh_smooth.
 *   SELECTION. D_0 = {v : select_dev[v] != 0}, or every vertex (the unused ones included) when select_dev is NULL; D_(r+1) = D_r + {v : N(v) meets D_r}; the
 *   selection is D_select_rings.
 *   MOVING. v moves iff it is selected and either INTERIOR, or BOUNDARY with boundary != PIN. NONMANIFOLD and UNUSED vertices never move. The neighbour set of a
 *   moving vertex is M(v) = N_b(v) for a BOUNDARY vertex under SLIDE, N(v) otherwise; m = |M(v)| >= 1. With passes >= 1, a moving vertex with
 *   m > RNB_MESH_SMOOTH_MAX_RING fails the call.
 *   THE PASSES. P_0 is the input widened to double. For k = 1 .. passes the factor is f = lambda when k is odd or mu == 0, else f = mu, and for every moving v and
 *   every axis c
 *     S_c = sum over u in M(v) of q(P_(k-1)(u)[c] - P_(k-1)(v)[c])      SHIFT = 32, terms below 2^10
 *     L_c = ((double) S_c * 2^-32) / (double) m
 *     P_k(v)[c] = P_(k-1)(v)[c] + f * L_c                              one multiply, one add
 *   Every other vertex keeps P_(k-1). All of pass k reads pass k-1 (Jacobi, two buffers).
 *   OUTPUTS. out->verts[v] = (float) P_passes(v) for a moving vertex; for any other vertex the input's bits (its coordinates are never examined, unless it is in M(u) of
 *   a moving u). displacement[v] = (float) sqrt((d.x * d.x + d.y * d.y) + d.z * d.z) of d = P_passes(v) - P_0(v) for a moving vertex, 0 for any other;
 *   max_displacement is the largest of these values, as a double.
 *
 * rnb_mesh_vertex_normals. For every triangle (a, b, c), degenerate ones included, the term is n = cross(b - a, c - a) of the widened positions, with
 * cross(u, v) = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); the vertex of each of its three corners gets n added (a vertex that is two
 * corners of one triangle gets it twice): SHIFT = 40, terms below 2^3, at most RNB_MESH_SMOOTH_MAX_RING corners per vertex. (On a sphere with a mean edge of 4.7e-4
 * a shift of 32 turns the normal by up to 0.27 degrees against unquantised sums, 40 by 1.0e-3.) With A the sum of a vertex and
 * l = sqrt((A.x * A.x + A.y * A.y) + A.z * A.z), its normal is (float)(A[k] / l), or (float)(-(A[k] / l)) with flip = 1; it is +0 in every component when l == 0
 * (a vertex without corners among them).
 * This is the counter-clockwise normal: a triangle seen from the side its normal points to runs counter-clockwise. On an extracted mesh that is the direction of the
 * SDF-gradient normals rnb_extract_mesh makes, and the negative of what the host's mesh::compute_normals (host/mesh.hpp) sums; flip = 1 gives the latter's sign.
 *
 * The grouping of the half-edges by edge, its cost and the bucket-load guard are those of rnb_mesh_topology.h; buckets_log2 must be 0 or 4 .. 30.
 */

typedef struct rnb_mesh_smooth_options {
	uint32_t abi_version;  /* RNB_MESH_SMOOTH_ABI_VERSION */
	uint32_t passes;       /* 0 .. RNB_MESH_SMOOTH_MAX_PASSES; default 2 (one Taubin pair; profiles/mesh_smooth.md says why). 0: a copy and the census */
	double   lambda;       /* finite, 0 < lambda <= 1; default 0.5 */
	double   mu;           /* finite, -1.5 <= mu <= 0; default -0.53. 0: every pass uses lambda (plain Laplacian smoothing, which shrinks) */
	uint32_t boundary;     /* RNB_MESH_SMOOTH_BOUNDARY_*; default PIN */
	uint32_t select_rings; /* 0 .. RNB_MESH_SMOOTH_MAX_SELECT_RINGS; default 0 */
	uint32_t normals;      /* RNB_MESH_SMOOTH_NORMALS_*; default KEEP */
	uint32_t buckets_log2; /* as in rnb_mesh_topology_options */
	uint32_t reserved[4];  /* 0 */
} rnb_mesh_smooth_options;

typedef struct rnb_mesh_smooth_stats {
	uint32_t n_edges;       /* |E| */
	uint32_t n_interior;    /* vertices by kind; the four add up to n_verts */
	uint32_t n_boundary;
	uint32_t n_nonmanifold;
	uint32_t n_unused;
	uint32_t n_selected;    /* |D_select_rings| */
	uint32_t n_moving;
	uint32_t max_valence;
	uint32_t passes;        /* as asked for */
	uint32_t n_wide;        /* moving vertices whose sums a workgroup forms, not a thread (m > 32); changes nothing of the result */
	double   max_displacement;
	uint64_t peak_workspace; /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;             /* wall-clock time of the call */
	float    ms_passes;      /* of that, the passes */
} rnb_mesh_smooth_stats;

typedef struct rnb_mesh_vertex_normals_options {
	uint32_t abi_version; /* RNB_MESH_SMOOTH_ABI_VERSION */
	uint32_t flip;        /* 0 (default) or 1 */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_vertex_normals_options;

typedef struct rnb_mesh_vertex_normals_stats {
	uint32_t n_zero;         /* vertices whose normal is 0 */
	uint32_t max_corners;    /* the most corners at one vertex */
	uint64_t peak_workspace;
	float    ms;
	uint32_t reserved;
} rnb_mesh_vertex_normals_stats;

uint32_t rnb_mesh_smooth_abi_version(void);
/* Fills *opt with the defaults: passes = 2, lambda = 0.5, mu = -0.53 (Taubin's usual pair), boundary = PIN, select_rings = 0, normals = KEEP, buckets_log2 = 0. */
int rnb_mesh_smooth_default_options(rnb_mesh_smooth_options* opt);
/* Fills *opt with the defaults: flip = 0. */
int rnb_mesh_vertex_normals_default_options(rnb_mesh_vertex_normals_options* opt);

/* The smoothing. in: any indexed triangle mesh in device memory; it is not modified and must not be *out. select_dev: NULL, or n_verts words of device memory.
 *
 * Output mesh: all input vertices in input order (this stage does not compact), all triangles unchanged and in input order, colours carried. With
 * normals = KEEP out->normals is set exactly when the input has normals, and holds them; with RECOMPUTE it is always set, to the result of
 * rnb_mesh_vertex_normals on the output with its default options (whose failures are then this call's).
 * Per vertex (each array optional, caller-allocated device memory of n_verts words): valence_dev[v] = valence(v), kind_dev[v] = RNB_MESH_SMOOTH_KIND_*,
 * displacement_dev[v] as defined above.
 *
 * Fails with RNB_ERR_INVALID as rnb_mesh_topology does (n_indices % 3 != 0; an index >= n_verts, range-checked by a kernel before any is used as an address; the
 * bucket guard), on an option outside its range, on a term or a ring as said above, and on a mesh of 2^31 edges or more. A mesh without vertices or without triangles
 * succeeds with a copy. On success *out owns its device buffers: release them with rnb_mesh_free. On failure *out is zeroed. Every argument is validated before the
 * context or the device is touched. Workspace (released before the call returns): the output; eight words per vertex, one per half-edge and the edge join's
 * 2^b + n_indices; with passes >= 1 six doubles and one more word per vertex and one word per entry of the neighbour lists (two per edge when every vertex moves). Work pending on the
 * context's side streams is joined first; reads nothing of the training state. One launch per pass, and a second one if a moving vertex has more than 32
 * neighbours; a handful of small device-to-host reads; syncs. */
int rnb_mesh_smooth(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_smooth_options* opt, const uint32_t* select_dev /* may be NULL: every vertex */,
                    rnb_mesh* out, uint32_t* valence_dev /* may be NULL */, uint32_t* kind_dev /* may be NULL */, float* displacement_dev /* may be NULL */,
                    rnb_mesh_smooth_stats* stats /* may be NULL */);

/* The normals. in: any indexed triangle mesh in device memory; it is not modified. normals_dev: float[n_verts][3], caller-allocated device memory.
 * Fails with RNB_ERR_INVALID on n_indices % 3 != 0, an index >= n_verts (range-checked by a kernel before any is used as an address), flip > 1, a term or a ring as
 * said above. A mesh without triangles succeeds with zeros. Workspace: nine words per vertex. */
int rnb_mesh_vertex_normals(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_vertex_normals_options* opt, float* normals_dev,
                            rnb_mesh_vertex_normals_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_SMOOTH_H */
