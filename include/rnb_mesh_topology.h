/*
 * rnb_mesh_topology.h — C-ABI of the mesh topology stage of librnb_neus2_hip: which triangles of an indexed device mesh share an edge. rnb_mesh_topology is the
 * census (per half-edge: faces on the edge, faces that run it the same way, the mate; mesh-wide: edges by kind, duplicates, patches, orientability, boundary loops,
 * Euler characteristic; per component: the same and the genus); rnb_mesh_repair returns a new mesh with coincident vertices welded, degenerate and duplicate
 * triangles removed and every orientable patch wound consistently (the fix_normals half of what rnb_mesh_clean.h replaces). It removes what rnb_mesh_simplify's
 * clustering can create (duplicate triangles, folded pairs); the non-manifold edges it only reports.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: no other ABI is affected by this header.
 */
#ifndef RNB_MESH_TOPOLOGY_H
#define RNB_MESH_TOPOLOGY_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_TOPOLOGY_ABI_VERSION 1

#define RNB_MESH_TOPOLOGY_NONE 0xFFFFFFFFu  /* no mate; no output vertex */
#define RNB_MESH_TOPOLOGY_MAX_BUCKET 65536u /* the bucket-load guard (Cost, below) */

#define RNB_MESH_DUPLICATES_KEEP 0   /* nothing is removed */
#define RNB_MESH_DUPLICATES_FIRST 1  /* of the triangles on one vertex set only the lowest-numbered stays (default) */
#define RNB_MESH_DUPLICATES_CANCEL 2 /* opposite windings cancel pair by pair; a folded pair goes entirely */

#define RNB_MESH_REPAIR_ORIENT_NONE 0       /* windings as they come (default) */
#define RNB_MESH_REPAIR_ORIENT_CONSISTENT 1 /* every orientable patch wound consistently across its manifold edges */

/*
 * Definitions (both entry points).
 *
 * Triangle t has the indices (i0, i1, i2) = indices[3t .. 3t+2]. It is DEGENERATE if two of them are equal. Degenerate triangles are counted and take no part in
 * anything else: they lie on no edge, are nobody's duplicate, belong to no patch. (They do join their corners into one component: that is the cleaner's definition.)
 *
 * Half-edge h = 3t + k (k = 0, 1, 2) of triangle t runs from corner k to corner (k + 1) % 3. Its undirected EDGE is the pair {min, max} of the two indices. The faces
 * ON an edge are the non-degenerate triangles that have a half-edge on it (each has exactly one). An edge is BOUNDARY with 1 face, MANIFOLD with 2, NON-MANIFOLD with 3
 * or more. A manifold edge is INCONSISTENT if its two faces run it in the same direction. Edges exist only where a face lies on them.
 *
 * The VERTEX SET of a non-degenerate triangle is {i0, i1, i2}; its WINDING is EVEN if (i0, i1, i2) is an even permutation of the ascending triple, i.e. if
 * (i0 > i1) + (i0 > i2) + (i1 > i2) is even, else ODD. For a vertex set held by p even and m odd triangles: every one of them but the lowest-numbered is a DUPLICATE
 * (n_duplicate_tris counts p + m - 1), and the set holds min(p, m) FOLDED PAIRS.
 *
 * COMPONENT: the cleaner's (rnb_mesh_clean.h): the classes of the closure of "two vertices are corners of one triangle" (degenerate triangles included); the label is
 * the smallest vertex index. A vertex no triangle uses belongs to none. PATCH: the classes of the non-degenerate triangles under "share a manifold edge"; boundary
 * and non-manifold edges join nothing. A patch is UNORIENTABLE if no choice of flips makes all its manifold edges consistent (the double cover below joins its two
 * sheets). BOUNDARY COMPONENT: the classes of the boundary edges under "share a vertex".
 *
 * Vertex-manifoldness is NOT examined: a vertex where two fans of triangles touch only at that vertex (a pinch) is not reported, by either entry point.
 *
 * Cost and the guard. The three groupings (half-edges by edge, triangles by vertex set, vertices by position) are hash joins: items are counted into 2^b buckets,
 * b = buckets_log2, or with buckets_log2 = 0 the smallest b >= 4 with 2^b >= 2 * items (at most 30); every item then reads every item of its bucket. A key that n items
 * share therefore costs n^2 reads. After the count, a bucket holding more than RNB_MESH_TOPOLOGY_MAX_BUCKET items fails the call with RNB_ERR_INVALID before
 * anything walks it (the message says that an edge, triangle or position is repeated that often, or that the forced bucket count is too small). With the default
 * bucket count hashing alone puts about ten items into the fullest bucket, so the guard fires on true multiplicity only. No result depends on buckets_log2, on the
 * hash or on the order in which a bucket was filled: only counts, minima and the unique other member of a pair are formed. buckets_log2 must be 0 or 4 .. 30.
 *
 * Determinism: the same input gives the same bits. A permutation of the triangles permutes the per-half-edge arrays (mates renumbered) and changes no statistic
 * and no table record. A renumbering of the vertices changes no statistic; of the table it changes the labels and, with them, the order of the records.
 */

typedef struct rnb_mesh_topology_options {
	uint32_t abi_version;  /* RNB_MESH_TOPOLOGY_ABI_VERSION */
	uint32_t buckets_log2; /* 0 (default): chosen per grouping; 4 .. 30: forced, for every grouping */
	uint32_t reserved[4];  /* 0 */
} rnb_mesh_topology_options;

/* One record of the census' component table. Edges and non-degenerate triangles belong to the component of their vertices. */
typedef struct rnb_mesh_topology_component {
	uint32_t label;                /* the smallest vertex index of the component */
	uint32_t n_vertices;
	uint32_t n_edges;
	uint32_t n_triangles;          /* non-degenerate ones */
	uint32_t n_boundary_edges;
	uint32_t n_nonmanifold_edges;
	uint32_t n_inconsistent_edges;
	uint32_t n_patches;
	int32_t  euler;                /* n_vertices - n_edges + n_triangles */
	int32_t  genus;                /* (2 - euler) / 2 if the component has no boundary, non-manifold or inconsistent edge, is exactly one patch (such a patch is
	                                  orientable) and 2 - euler is even and not negative; else -1 */
} rnb_mesh_topology_component;

typedef struct rnb_mesh_topology_stats {
	uint32_t n_verts_used;           /* vertices at least one triangle uses */
	uint32_t n_tris;                 /* n_indices / 3, degenerate ones included */
	uint32_t n_degenerate;
	uint32_t n_edges;
	uint32_t n_boundary_edges;
	uint32_t n_manifold_edges;       /* the inconsistent ones included */
	uint32_t n_nonmanifold_edges;
	uint32_t n_inconsistent_edges;
	uint32_t max_faces_on_edge;      /* 0 for a mesh without edges */
	uint32_t n_duplicate_tris;
	uint32_t n_folded_pairs;         /* what RNB_MESH_DUPLICATES_CANCEL would cancel: the sum over the vertex sets of min(p, m) */
	uint32_t n_components;           /* = records in the table */
	uint32_t n_patches;
	uint32_t n_unorientable_patches;
	uint32_t n_boundary_components;
	uint32_t closed;                 /* 1: no boundary and no non-manifold edge (an empty mesh is closed) */
	uint32_t oriented;               /* 1: closed and no inconsistent edge */
	uint32_t reserved;
	int64_t  euler;                  /* n_verts_used - n_edges + (n_tris - n_degenerate) */
	uint64_t peak_workspace;         /* bytes of device memory the call held at its peak, the table included */
	float    ms;                     /* wall-clock time of the call */
	uint32_t reserved2;
} rnb_mesh_topology_stats;

uint32_t rnb_mesh_topology_abi_version(void);
/* Fills *opt with the defaults: buckets_log2 = 0. */
int rnb_mesh_topology_default_options(rnb_mesh_topology_options* opt);

/* The census. in: any indexed triangle mesh in device memory; it is not modified; coordinates and attributes are never read.
 *
 * Per half-edge (each array optional, caller-allocated device memory of n_indices words, written in input order):
 *   n_faces_dev[h]  the faces on h's edge (exact, not capped); 0 for a half-edge of a degenerate triangle
 *   n_same_dev[h]   those of them whose half-edge on that edge runs in h's direction, h's own triangle included; 0 for a degenerate triangle
 *   mate_dev[h]     the other half-edge on the edge if n_faces is 2, else RNB_MESH_TOPOLOGY_NONE
 * Statistics and table as defined above; the table (table_dev != NULL) is device memory holding stats->n_components records in ascending label (ask for the
 * statistics with it), released with rnb_mesh_topology_table_free.
 *
 * n_indices % 3 != 0 or an index >= n_verts fails with RNB_ERR_INVALID (the indices are range-checked by a kernel before any is used as an address). An empty input
 * (n_indices == 0) succeeds: all counts 0, closed = oriented = 1, an empty table. On failure *table_dev is NULL. Every argument is validated before the context or
 * the device is touched. Workspace (released before the call returns): three words per vertex and one per 1024 for the prefix sums for the components; per grouping
 * 2^b words of buckets and one word per item; two words per triangle for the double cover; two per vertex for the boundary components. Work pending on the context's
 * side streams is joined first; reads nothing of the training state. A handful of small device-to-host reads; syncs. */
int rnb_mesh_topology(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_topology_options* opt, uint32_t* n_faces_dev /* may be NULL */,
                      uint32_t* n_same_dev /* may be NULL */, uint32_t* mate_dev /* may be NULL */, rnb_mesh_topology_component** table_dev /* may be NULL */,
                      rnb_mesh_topology_stats* stats /* may be NULL */);
/* Releases a table rnb_mesh_topology returned (NULL is accepted). */
int rnb_mesh_topology_table_free(rnb_ctx* ctx, rnb_mesh_topology_component* table_dev);

typedef struct rnb_mesh_repair_options {
	uint32_t abi_version;     /* RNB_MESH_TOPOLOGY_ABI_VERSION */
	uint32_t weld;            /* 0 (default) or 1 */
	uint32_t drop_degenerate; /* 1 (default) or 0 */
	uint32_t duplicates;      /* RNB_MESH_DUPLICATES_* (default FIRST) */
	uint32_t orient;          /* RNB_MESH_REPAIR_ORIENT_* (default NONE) */
	uint32_t buckets_log2;    /* as in rnb_mesh_topology_options */
	uint32_t reserved[4];     /* 0 */
} rnb_mesh_repair_options;

typedef struct rnb_mesh_repair_stats {
	uint32_t n_welded;               /* used vertices replaced by a lower-indexed one at the same position; 0 without weld */
	uint32_t n_degenerate_dropped;
	uint32_t n_duplicates_dropped;
	uint32_t n_flipped;
	uint32_t n_patches;              /* of the mesh step 4 works on; 0 with RNB_MESH_REPAIR_ORIENT_NONE (nothing is looked for) */
	uint32_t n_unorientable_patches; /* likewise */
	uint32_t n_verts_in;
	uint32_t n_verts_out;
	uint32_t n_tris_in;
	uint32_t n_tris_out;
	uint64_t peak_workspace;         /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;
	uint32_t reserved;
} rnb_mesh_repair_stats;

/* Fills *opt with the defaults: no weld, degenerate triangles dropped, duplicates FIRST, orient NONE, buckets_log2 = 0. */
int rnb_mesh_repair_default_options(rnb_mesh_repair_options* opt);

/* The repair. in: any indexed triangle mesh in device memory; it is not modified and must not be *out. Four steps, in this order, each defined on the result of the
 * one before it (the triangles keep their input numbers throughout: "lowest-numbered" is by input order):
 *
 * 1. Weld (weld = 1). Among the vertices at least one triangle uses, those whose three coordinates are equal as numbers (-0 equals +0) become the lowest-indexed one
 *    of them: every index is rewritten to it, so its attributes are the ones that survive. A used vertex with a coordinate that is not finite fails the call with
 *    RNB_ERR_INVALID. Without weld no coordinate is read.
 * 2. Degenerate (drop_degenerate = 1). Triangles with a repeated index (after step 1) are removed. With 0 they stay, are carried to the output as they are, and take
 *    no part in steps 3 and 4.
 * 3. Duplicates. The remaining non-degenerate triangles are grouped by vertex set, p even and m odd windings in a group. KEEP: nothing is removed. FIRST: only the
 *    lowest-numbered triangle of the group stays. CANCEL: |p - m| triangles stay, the lowest-numbered ones of the majority winding; none when p == m.
 * 4. Orient (RNB_MESH_REPAIR_ORIENT_CONSISTENT), through the double cover of the remaining non-degenerate triangles. Triangle t has the nodes 2t and 2t+1. Every manifold
 *    edge, between t and u, unites 2t ~ 2u and 2t+1 ~ 2u+1 if it is consistent, 2t ~ 2u+1 and 2t+1 ~ 2u if it is inconsistent; boundary and non-manifold edges unite
 *    nothing. root(x) is the smallest node of x's class. A patch with root(2t) == root(2t+1) (for one t, then for all) is unorientable: it is left as it came and
 *    counted. Any other patch has two sheets: "flip exactly its triangles with root(2t) > root(2t+1)", and the complement within the patch. The sheet that flips
 *    fewer triangles is taken; on a tie the one that leaves the patch's lowest-numbered triangle unflipped (which is the first). A flip swaps the second and third
 *    index of the triangle.
 *
 * Output: the stable compaction of the other mesh stages: the vertices the remaining triangles use, in input order, with their attributes (out->colors / out->normals are
 * set exactly when the input has them); the remaining triangles in input order, indices renumbered. vertex_map_dev (optional, caller-allocated device memory of
 * n_verts words): for every input vertex the output index of the vertex it became (through the weld), RNB_MESH_TOPOLOGY_NONE if that vertex is not in the output.
 *
 * Failures as for rnb_mesh_topology, and an unknown value of weld, drop_degenerate, duplicates or orient. An empty input succeeds with an empty *out. On success *out
 * owns its device buffers: release them with rnb_mesh_free. On failure *out is zeroed. The same input gives the same bits, whatever buckets_log2. Workspace: four
 * words per triangle (working indices, a flag), with orient four more; three per vertex; per grouping 2^b words and one per item; the output. */
int rnb_mesh_repair(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_repair_options* opt, rnb_mesh* out, uint32_t* vertex_map_dev /* may be NULL */,
                    rnb_mesh_repair_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_TOPOLOGY_H */
