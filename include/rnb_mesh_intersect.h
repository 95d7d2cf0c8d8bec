/*
 * rnb_mesh_intersect.h — C-ABI of the self-intersection stage of librnb_neus2_hip: which triangles of an indexed triangle mesh in device memory pass through, touch or
 * overlap other triangles of the same mesh (rnb_mesh_intersections), and the mesh without them (rnb_mesh_intersections_select), whose rims rnb_mesh_fill_holes
 * (rnb_mesh_holes.h) can close again. rnb_mesh_topology (rnb_mesh_topology.h) joins triangles through their indices only; this stage looks at the geometry. It tells
 * what a fan of rnb_mesh_fill_holes, a cluster of rnb_mesh_simplify or a cut that keeps only the seen faces left folded through its neighbours.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: no other ABI is affected by this header.
 */
#ifndef RNB_MESH_INTERSECT_H
#define RNB_MESH_INTERSECT_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_INTERSECT_ABI_VERSION 1

/* The class of a pair, and the bits of rnb_mesh_intersect_select_options.classes. A pair that is neither is APART and is reported nowhere. */
#define RNB_MESH_INTERSECT_PROPER 1u
#define RNB_MESH_INTERSECT_CONTACT 2u
#define RNB_MESH_INTERSECT_MAX_RINGS 8u
#define RNB_MESH_INTERSECT_MAX_CELLS 256u /* the grid and its limits are those of the header of rnb_mesh_distance (RNB_MESH_DISTANCE_LARGE_CELLS, _MAX_LARGE, _MAX_ENTRIES) */

typedef struct rnb_mesh_intersect_options {
	uint32_t abi_version; /* RNB_MESH_INTERSECT_ABI_VERSION */
	uint32_t cells;       /* cells of the search grid along the longest axis of the mesh's box, 1 .. 256; 0 = automatic. Changes the time, never the result */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_intersect_options;

typedef struct rnb_mesh_intersect_pair {
	uint32_t s, t; /* triangle numbers (position in the index list / 3), s < t */
	uint32_t cls;  /* RNB_MESH_INTERSECT_PROPER or RNB_MESH_INTERSECT_CONTACT */
} rnb_mesh_intersect_pair;

typedef struct rnb_mesh_intersect_stats {
	uint32_t n_tris;
	uint32_t n_degenerate;     /* triangles with l == 0: they take no part (rule 4) */
	uint32_t n_tris_proper;    /* triangles with n_proper > 0 */
	uint32_t n_tris_contact;   /* triangles with n_contact > 0 */
	uint64_t n_same_set;       /* pairs of triangles on the same three vertices (rule 4) */
	uint64_t n_candidates;     /* rule 4 */
	uint64_t n_pairs_proper;
	uint64_t n_pairs_contact;
	uint64_t n_coplanar_pairs; /* candidates decided inside a plane: by rule 5 once d_S lies in T's plane, or by step 2 of rule 6 */
	uint64_t n_pairs_written_would_be; /* n_pairs_proper + n_pairs_contact if pairs_dev was given, else 0: the capacity a complete list needs */
	/* the grid block: what `cells` may change, beside peak_workspace and the times */
	uint32_t dims[3];          /* the search grid actually used (all zero for a mesh without a triangle that takes part) */
	uint32_t n_large;          /* triangles in the large list */
	double   cell;
	uint64_t n_cell_entries;   /* (triangle, cell) registrations */
	uint64_t n_visited;        /* pairs the search looked at: those of every cell's list, and (triangle, large entry) */
	uint64_t peak_workspace;   /* bytes of device memory the call held at its peak */
	float    ms;               /* wall-clock time of the call */
	float    ms_grid;          /* of which: bounding box, cell lists */
} rnb_mesh_intersect_stats;

typedef struct rnb_mesh_intersect_select_options {
	uint32_t abi_version;          /* RNB_MESH_INTERSECT_ABI_VERSION */
	uint32_t classes;              /* RNB_MESH_INTERSECT_PROPER | RNB_MESH_INTERSECT_CONTACT, at least one; default PROPER */
	uint32_t rings;                /* 0 .. 8; default 0 */
	uint32_t drop_unused_vertices; /* 0 / 1; default 1 */
	uint32_t reserved[4];          /* 0 */
} rnb_mesh_intersect_select_options;

typedef struct rnb_mesh_intersect_select_stats {
	uint32_t n_verts_in, n_verts_out, n_tris_in, n_tris_out;
	uint32_t n_selected;      /* triangles with a partner in one of `classes` */
	uint32_t n_tris_removed;  /* those and the rings around them */
	uint32_t n_verts_removed;
	uint32_t reserved;
	uint64_t peak_workspace;
	float    ms;
	uint32_t reserved2;
} rnb_mesh_intersect_select_stats;

uint32_t rnb_mesh_intersect_abi_version(void);
/* Fills *opt with the defaults: automatic cells. */
int rnb_mesh_intersect_default_options(rnb_mesh_intersect_options* opt);
/* Fills *opt with the defaults: classes = PROPER, rings = 0, drop_unused_vertices = 1. */
int rnb_mesh_intersections_select_default_options(rnb_mesh_intersect_select_options* opt);

/* in: an indexed triangle mesh in device memory (verts and indices are read; colours and normals are ignored); it is not modified. n_proper_dev, n_contact_dev:
 * uint32[n_tris] in device memory or NULL. pairs_dev: rnb_mesh_intersect_pair[pairs_capacity] in device memory or NULL.
 *
 * Arithmetic.
 *  1. Double precision, floats widened first, every operation rounded on its own (no fused multiply-add). For vectors, u x v = (u.y * v.z - u.z * v.y,
 *     u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x) and dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z, as in rules 1-2 of the header of rnb_mesh_distance. A triangle is its three
 *     corners in the order of the index list; "T; d" below stands for T_0, T_1, T_2, d.
 *  2. orient(a, b, c, d), the side of d of the plane through a, b, c: u = b - a, v = c - a, w = d - a, n = u x v, det = dot(n, w);
 *     m = (|u.y * v.z| + |u.z * v.y|, |u.z * v.x| + |u.x * v.z|, |u.x * v.y| + |u.y * v.x|), P = (m.x * |w.x| + m.y * |w.y|) + m.z * |w.z|. The sign is 0 if
 *     |det| <= 2^-48 * P, else the sign of det. 2^-48 is 32 unit roundoffs e; Shewchuk's static bound on the error of this expression is (7 + 56 e) e P (Adaptive Precision
 *     Floating-Point Arithmetic and Fast Robust Geometric Predicates, 1997), so A SIGN THAT IS NOT 0 IS THE SIGN OF THE EXACT DETERMINANT. (The differences u, v, w of
 *     floats are exact in double unless the coordinates span more than 2^29 in exponent.)
 *  3. orient2(a, b, c; axis), the same in the plane with one axis dropped: (i, j) = (y, z), (z, x), (x, y) for axis x, y, z; l = (b_i - a_i) * (c_j - a_j),
 *     r = (b_j - a_j) * (c_i - a_i); the sign is 0 if |l - r| <= 2^-50 * (|l| + |r|), else the sign of l - r. The axis of a triangle (a, b, c) is the one where
 *     |n|, n = (b - a) x (c - a), is largest; of equals the lowest.
 *
 * Who takes part.
 *  4. A triangle with l == 0 (rule 1 of the header of rnb_mesh_distance: l = sqrt(dot(n, n))) takes no part (n_degenerate); one that names a vertex twice is among them. Of two
 *     triangles that take part: if their three indices are the same set, the pair is skipped (n_same_set: duplicates and folded pairs are rnb_mesh_topology's
 *     business); otherwise it is a CANDIDATE if the closed boxes of their float coordinates overlap on every axis (lo_S <= hi_T and lo_T <= hi_S, exact
 *     comparisons). n_candidates is therefore a property of the mesh, not of the search.
 *
 * The class of a candidate (S, T), S the triangle with the lower number: APART, CONTACT or PROPER.
 *  5. Two indices shared (an edge in common). d_S, d_T = the other corner of each. If orient(T; d_S) != 0 the pair is APART (a hinge). Otherwise, on T's axis, with
 *     (p, q) = the two corners that follow d_T in T's cyclic order: if orient2(p, q, d_S) and orient2(p, q, d_T) are both non-zero and differ, the pair is APART
 *     (a flat hinge); else it is CONTACT (a fold: the two lie on the same side of their edge, or a side is not decided).
 *  6. Otherwise. A corner both share (at most one) is EXEMPT: it is left out of every sign test below, and an edge that contains it is not tested.
 *     sS_i = orient(T; S_i), sT_j = orient(S; T_j) over the corners that are not exempt.
 *     Step 1. If all sS are equal and not 0, or all sT are, the pair is APART.
 *     Step 2. Else, if all sS are 0 or all sT are 0, the pair is COPLANAR: by rule 7 on T's axis it is APART if the two triangles are separated, else CONTACT.
 *     Step 3. Else every tested edge (p, q) of S against F = T, then every tested edge of T against F = S, edges in the order (X_0, X_1), (X_1, X_2), (X_2, X_0), with the
 *             signs sp, sq of its ends from above and F = (a, b, c):
 *               sp * sq > 0: the edge gives nothing.
 *               sp = sq = 0: by rule 7 on F's axis, CONTACT unless the segment and F are separated.
 *               else s1 = orient(p, q, a, b), s2 = orient(p, q, b, c), s3 = orient(p, q, c, a): if +1 and -1 both occur among them the edge gives nothing; if
 *               sp * sq < 0 and s1 = s2 = s3 != 0 the edge gives PROPER; otherwise it gives CONTACT.
 *             The pair is PROPER if an edge gave PROPER, else CONTACT if one gave CONTACT, else APART.
 *  7. Separation in the plane (one axis dropped), NOT STRICT: a sign of 0 means "on the line", and on the line counts as outside. An edge (e_0, e_1) of a triangle
 *     with third corner e_2 SEPARATES a set of points if ref = orient2(e_0, e_1, e_2) != 0 and orient2(e_0, e_1, x) * ref <= 0 for every point x of the set. Two
 *     triangles are separated if an edge of one separates the non-exempt corners of the other (T's edges are tried first; the order cannot matter). A segment
 *     (p, q) and a triangle F are separated if an edge of F separates {p, q}, or if orient2(p, q, F_k) is >= 0 for all three k, or <= 0 for all three.
 *     CONSEQUENCE: coplanar pieces that only touch along their boundaries are APART, so a flat triangulated region reports nothing, T-junctions and collinear
 *     neighbours included; coplanar overlap of positive area is CONTACT.
 *
 * What the classes mean. PROPER is certain: an edge of one triangle passes through the interior of the other, and every sign that says so was decided (rule 2), so it is
 * the sign exact arithmetic gives. CONTACT is everything else that is not clearly apart: touching, grazing, a fold, coplanar overlap, or a sign double precision
 * did not decide. A mesh whose coincident vertices are not welded reports CONTACT all along its seams (the two sides share positions but no index): weld it first
 * (rnb_mesh_repair, weld = 1). APART is not certain in the same way only where a plane test (rules 5, 7) took part.
 *
 * Outputs.
 *  8. n_proper[t], n_contact[t] = the number of candidates in each class triangle t belongs to (0 for a triangle that takes no part). They are integers added
 *     atomically: they depend on no order and on no grid, and they follow their triangle under a permutation of the triangles that keeps every pair's classification
 *     (rules 5-6 name the lower triangle S; a class that depends on which of the two is S can only be a CONTACT / APART case of undecided signs). pairs_dev
 *     receives {s, t, cls}, s < t, for every candidate that is not APART, in ascending (s, t). If there are more than pairs_capacity, the list is cut there (its first
 *     pairs_capacity records are written, nothing beyond) and n_pairs_written_would_be holds the full count: that is no error. More than 2^32 - 1 pairs with
 *     pairs_dev given fail the call.
 *  9. The same input gives the same bits. ONLY dims, cell, n_cell_entries, n_large, n_visited, peak_workspace AND THE TIMES CAN DEPEND ON options.cells.
 *
 * The search (none of it can change a result). The grid of rnb_mesh_distance over the box of the vertices the mesh uses: L = its longest edge, N = options.cells or
 * floor(sqrt(m / 2)) within 1 .. 256 (m = the triangles that take part), cell = L / N, dims_k = min(N, floor((hi_k - lo_k) / cell) + 1), the cell of a coordinate x is
 * min(max(floor((x - lo_k) / cell), 0), dims_k - 1). A triangle is registered in every cell from the cell of the low corner of its box (c0) to that of the high
 * corner (c1); one whose range holds more than RNB_MESH_DISTANCE_LARGE_CELLS cells goes into the large list instead (more than RNB_MESH_DISTANCE_MAX_LARGE of
 * them, or more than 2^31 cell entries, fail the call and ask for a coarser grid). Two registered triangles are examined in the one cell max(c0_S, c0_T) (per
 * axis), and only if both are registered there. Every triangle that takes part is examined against every entry of the large list, a pair of two large ones only
 * from the lower-numbered of the two.
 * Proof that every candidate is examined exactly once. The cell function is monotone in x. If the boxes overlap on axis k, lo_S <= hi_T and lo_T <= hi_S give
 * c0_S <= c1_T and c0_T <= c1_S, so m_k = max(c0_S, c0_T) lies in both ranges [c0_S, c1_S] and [c0_T, c1_T]: both triangles are registered in the cell m, whose
 * list therefore holds both, and no other cell passes the test "this cell is m", so the pair is examined once. Contrapositive: if the ranges do not overlap on some
 * axis the boxes do not, and the pair is no candidate. A pair with a large member is in no cell's list twice (the large one is in none) and is met once in the pass
 * over (triangle, large entry): from the side of the one that is not large, or, with both large, from the lower one. The box test itself is made on the floats.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, in or opt; a wrong version; a reserved word that is not 0; cells > 256;
 * n_indices % 3 != 0 or a null vertex or index buffer; indices without vertices; pairs_capacity > 0 without pairs_dev. After the range-check kernel: an index
 * >= n_verts, a coordinate of a used vertex that is not finite. Later: the large list or the cell lists too long, too many pairs for a list. On failure the
 * outputs hold nothing of use, *stats is zeroed and the context stays usable. A mesh without triangles succeeds with zeros.
 *
 * Workspace: one word per vertex, two words per cell, one word per cell entry; with pairs_dev two words per triangle and 12 bytes per reported pair; released
 * before the call returns. Reads nothing of the training state; work pending on the context's side streams is joined first. A handful of small device-to-host
 * reads; syncs. */
int rnb_mesh_intersections(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_intersect_options* opt, uint32_t* n_proper_dev /* may be NULL */,
                           uint32_t* n_contact_dev /* may be NULL */, rnb_mesh_intersect_pair* pairs_dev /* may be NULL */, uint64_t pairs_capacity,
                           rnb_mesh_intersect_stats* stats /* may be NULL */);

/* *out = a new mesh (release it with rnb_mesh_free): `in` without the SELECTED triangles, the others in input order with their winding, colours and normals carried
 * along. n_proper_dev, n_contact_dev: what rnb_mesh_intersections wrote for this very mesh (a class that is not in options.classes may be NULL). Selected: every
 * triangle t with n_proper[t] > 0 (PROPER in classes) or n_contact[t] > 0 (CONTACT in classes); then, `rings` times, every triangle that shares a vertex index with a
 * selected one. drop_unused_vertices = 1: the vertices no remaining triangle uses go as well (those the input did not use included), the others keep their order;
 * 0: every vertex stays. Removing both partners of every pair is the blunt, order-free choice: afterwards no pair of the reported class is left among the
 * remaining triangles, since removing triangles creates no new pair. A selection of everything returns a mesh without triangles, which is no error; so does an
 * input without triangles (its vertices are then dropped whatever the option says). Bit-reproducible. Fails like rnb_mesh_intersections, and for classes == 0 or
 * with unknown bits, rings > 8, drop_unused_vertices > 1, a needed count array that is NULL, in == out. */
int rnb_mesh_intersections_select(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const uint32_t* n_proper_dev, const uint32_t* n_contact_dev,
                                  const rnb_mesh_intersect_select_options* opt, rnb_mesh* out, rnb_mesh_intersect_select_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_INTERSECT_H */
