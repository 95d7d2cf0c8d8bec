/*
 * rnb_mesh_distance.h — C-ABI of the mesh-to-mesh distance of librnb_neus2_hip: the one-sided distance from the surface of one indexed triangle mesh in device memory
 * to the surface of another (area-weighted mean, rms, maximum, fractions within thresholds, and per vertex). It measures what rnb_mesh_simplify (rnb_mesh_simplify.h)
 * cost in accuracy, and a reconstruction against a ground-truth mesh (Chamfer distance, Hausdorff distance, F-score: two calls, one per direction).
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI, the mesh-clean ABI and the mesh-simplify ABI are not affected by this header.
 */
#ifndef RNB_MESH_DISTANCE_H
#define RNB_MESH_DISTANCE_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_DISTANCE_ABI_VERSION 1

#define RNB_MESH_DISTANCE_MAX_LEVEL 3u        /* 4^level sub-centroids per triangle of A */
#define RNB_MESH_DISTANCE_MAX_TAUS 4
#define RNB_MESH_DISTANCE_NONE 0xFFFFFFFFu    /* vert_nearest of an unused vertex or of a sample beyond max_distance */
#define RNB_MESH_DISTANCE_MAX_CELLS 256u      /* cells per axis of the search grid */
#define RNB_MESH_DISTANCE_LARGE_CELLS 2048u   /* a triangle of B whose box overlaps more cells than this goes into the large list */
#define RNB_MESH_DISTANCE_MAX_LARGE 4096u     /* entries the large list can hold */
#define RNB_MESH_DISTANCE_MAX_ENTRIES (1ull << 31) /* cell-list entries */

/* Fixed point of every summed term (rule 5): q = (uint64) trunc(term * 2^RNB_MESH_DISTANCE_Q_SHIFT). A term must be finite and smaller than
 * 2^RNB_MESH_DISTANCE_Q_TERM_LOG2, else the call fails. */
#define RNB_MESH_DISTANCE_Q_SHIFT 48
#define RNB_MESH_DISTANCE_Q_TERM_LOG2 12

typedef struct rnb_mesh_distance_options {
	uint32_t abi_version;  /* RNB_MESH_DISTANCE_ABI_VERSION */
	uint32_t level;        /* 0 .. 3: every non-degenerate triangle of A is sampled at the centroids of its 4^level congruent sub-triangles; default 1 */
	float    max_distance; /* D of rule 3; 0 = no cap; >= 0 and finite */
	float    unit;         /* distances are summed in this unit (d' = d / unit); > 0 and finite; default 2^-10 */
	float    tau[RNB_MESH_DISTANCE_MAX_TAUS]; /* thresholds of the `within` sums, in the units of the coordinates; 0 = unused; >= 0 and finite */
	uint32_t cells;        /* cells of the search grid along the longest axis of B's box, 1 .. 256; 0 = automatic (below). Changes the time, never the result */
	uint32_t reserved[4];  /* 0 */
} rnb_mesh_distance_options;

typedef struct rnb_mesh_distance_stats {
	uint32_t n_verts_from_used;  /* vertices of A some triangle of A uses: the samples (a) */
	uint32_t n_verts_to_used;
	uint32_t n_tris_from;
	uint32_t n_tris_to;
	uint32_t n_degenerate_from;  /* triangles of A with l == 0: they carry no sample (b) */
	uint32_t n_degenerate_to;    /* triangles of B with l == 0: they take no part */
	uint32_t n_verts_beyond;     /* samples (a) with d > max_distance */
	uint32_t n_large;            /* triangles of B in the large list */
	uint64_t n_samples;          /* samples (b): 4^level per non-degenerate triangle of A */
	uint64_t n_beyond;           /* samples (b) with d > max_distance */
	int64_t  sum_w;              /* S(w) * 2^48: the area of A */
	int64_t  sum_wd;             /* S(w * d') * 2^48 */
	int64_t  sum_wd2;            /* S((w * d') * d') * 2^48 */
	int64_t  sum_within[RNB_MESH_DISTANCE_MAX_TAUS]; /* S(w * [d <= tau_k]) * 2^48; 0 for an unused tau */
	double   max_distance;       /* the largest d over the samples (a) and (b); 0 without samples */
	uint32_t dims[3];            /* the search grid actually used (all zero for an A without triangles: no grid is built) */
	uint32_t reserved;
	double   cell;
	uint64_t n_cell_entries;     /* (triangle, cell) registrations */
	uint64_t n_pairs;            /* point-triangle evaluations of rule 2; deterministic for a given grid */
	uint64_t peak_workspace;     /* bytes of device memory the call held at its peak */
	float    ms;                 /* wall-clock time of the call */
	float    ms_grid;            /* of which: bounding box, cell lists (the rest is validation and the queries) */
} rnb_mesh_distance_stats;

uint32_t rnb_mesh_distance_abi_version(void);
/* Fills *opt with the defaults: level 1, no cap, unit 2^-10, no thresholds, automatic cells. */
int rnb_mesh_distance_default_options(rnb_mesh_distance_options* opt);

/* from (A), to (B): indexed triangle meshes in device memory (verts and indices are read; colours and normals are ignored); neither is modified; they must be different
 * objects. vert_dist_dev: float[A.n_verts] in device memory or NULL; vert_nearest_dev: uint32[A.n_verts] in device memory or NULL. The call measures the one-sided
 * distance from the surface of A to the surface of B; a symmetric measure is two calls.
 *
 * Arithmetic. Everything below is double precision with every operation rounded on its own (no fused multiply-add, IEEE division and square root); floats are widened
 * first. dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z. Sums are 64-bit fixed point (above) added as integers: they depend neither on the order of the additions nor on
 * the launch shape.
 *
 * 1. Triangles of B. For a triangle (a, b, c): u = b - a, v = c - a, n = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x), l = sqrt(dot(n, n)) (rule 3
 *    of rnb_mesh_simplify.h). A triangle with l == 0 takes no part (n_degenerate_to). If B has no other triangle the call fails.
 * 2. s(p, T), the squared distance from a point p to the triangle T = (a, b, c): the closest point q by the Voronoi regions of the triangle, tested in THIS order (the
 *    first test that holds decides; the order decides bits on region boundaries):
 *      ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap)
 *      d1 <= 0 and d2 <= 0:                            q = a
 *      bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp)
 *      d3 >= 0 and d4 <= d3:                           q = b
 *      vc = d1 * d4 - d3 * d2
 *      vc <= 0 and d1 >= 0 and d3 <= 0:                t = d1 / (d1 - d3),                         q = a + ab * t
 *      cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp)
 *      d6 >= 0 and d5 <= d6:                           q = c
 *      vb = d5 * d2 - d1 * d6
 *      vb <= 0 and d2 >= 0 and d6 <= 0:                t = d2 / (d2 - d6),                         q = a + ac * t
 *      va = d3 * d6 - d5 * d4, g = d4 - d3, h = d5 - d6
 *      va <= 0 and g >= 0 and h >= 0:                  t = g / (g + h),                            q = b + (c - b) * t
 *      else (the face):                                k = (va + vb) + vc, y = vb / k, z = vc / k, q = (a + ab * y) + ac * z
 *    (vector times scalar and vector sums per component). Then e = p - q and s = dot(e, e). An s that is not a number never wins the minimum of rule 3.
 * 3. Distance of a point: s(p) = the minimum of s(p, T) over the non-degenerate triangles of B, nearest(p) = the lowest triangle index (position in B's index list / 3)
 *    that attains it, d(p) = sqrt(s(p)). With max_distance D > 0: if d(p) > (double) D then d(p) = D, nearest(p) = RNB_MESH_DISTANCE_NONE and the sample is counted as
 *    beyond; d(p) == D is not beyond.
 * 4. Samples of A.
 *    (a) Every vertex some triangle of A uses: vert_dist = (float) d, vert_nearest = nearest; it takes part in the maximum and in nothing else. A vertex no triangle uses
 *        gets 0 and RNB_MESH_DISTANCE_NONE.
 *    (b) Every triangle (a, b, c) of A with l != 0 (l as in rule 1), n = 2^level: the n^2 centroids of its congruent sub-triangles. Upward ones (i, j), i, j >= 0, i + j <= n - 1,
 *        have the barycentric numerators (A, B, C) = (3i + 1, 3j + 1, 3n - 3i - 3j - 2), downward ones, i + j <= n - 2, (3i + 2, 3j + 2, 3n - 3i - 3j - 4);
 *        al = A / (3n), be = B / (3n), ga = C / (3n) (integers converted exactly, one division each), p = (a * al + b * be) + c * ga, weight w = (0.5 * l) / (double) (n * n).
 * 5. Sums over the samples (b), with d' = d / (double) unit: S(w), S(w * d'), S((w * d') * d'), and for each tau_k != 0, S(w) over the samples with d <= (double) tau_k.
 *    A term is added as trunc(term * 2^48); it must be finite and below 2^12 (otherwise the call fails: choose a larger unit, or a max_distance). Overflow: every term is
 *    split into its low 32 bits and the rest, and the two parts are summed in 64-bit words of their own; a part is below 2^32, the call refuses more than 2^32 - 1 samples,
 *    so neither word can wrap. The words are joined on the host in 128 bits and a sum of 2^63 or more fails the call in the same way; what is reported is therefore the
 *    exact integer sum of the terms. Quantisation: truncation loses less than 2^-48 per term, so each reported sum lies below the sum of the exact terms by less than
 *    n_samples * 2^-48. The maximum of d over the samples (a) and (b) is taken as the maximum of the bit patterns of non-negative doubles (which orders them as numbers).
 * 6. Consequences: the same input gives the same bits. A permutation of A's triangles or a renumbering of either mesh's vertices changes nothing (vert_dist and
 *    vert_nearest follow their vertices). A permutation of B's triangles changes vert_nearest only. NOTHING THAT RULES 1-5 DEFINE DEPENDS ON THE SEARCH GRID: dims,
 *    cell, n_cell_entries, n_large, n_pairs, peak_workspace and the times are the only outputs `cells` can change.
 *
 * The search (how the minimum of rule 3 is found; none of it can change a result). Box: per axis lo_k, hi_k = the smallest and largest coordinate of the vertices B uses.
 * L = the longest edge hi_k - lo_k. N = options.cells, or automatically floor(sqrt(m / 2)) kept within 1 .. 256, m = the non-degenerate triangles of B (a surface of m
 * triangles crosses in the order of N^2 cells of an N^3 grid: about two triangles per occupied cell). cell = L / N; dims_k = min(N, floor((hi_k - lo_k) / cell) + 1);
 * the cell of a coordinate x is min(max(floor((x - lo_k) / cell), 0), dims_k - 1). A triangle is registered in every cell from the cell of the low corner of its box to the
 * cell of the high corner; one whose box overlaps more than RNB_MESH_DISTANCE_LARGE_CELLS cells goes into the large list instead, which every query tests in full
 * (more than RNB_MESH_DISTANCE_MAX_LARGE of them, or more than 2^31 cell entries, fail the call and ask for a coarser grid). A query p: p' = p clamped into the box,
 * c = the cell of p', o2 = |p - p'|^2. After the large list it visits the Chebyshev shells r = 0, 1, 2, ... of cells around c and stops after shell r >= 1 once
 *      best_s <= ((r - 1/16) * cell)^2 + o2 * (1 - 2^-20),
 * or once the shells cover the grid, or, with a cap, once ((r - 1/16) * cell)^2 + o2 * (1 - 2^-20) >= D^2.
 * Proof. The cell function is monotone, so every point q of a registered triangle lies in a cell the triangle is registered in. If that cell is outside shell r, its index
 * differs from c's by more than r on some axis k, so the rounded quotients of q_k and p'_k differ by more than r, and |q_k - p'_k| > (r - 2^-40) * cell (two roundings of
 * relative size 2^-53 on quotients of at most 256). p' is the point of the box nearest to p on every axis, so |q_j - p_j| >= |p'_j - p_j| on every axis j and, on axis k,
 * |q_k - p_k| >= |q_k - p'_k| + |p'_k - p_k| when p_k is outside the box: |q - p|^2 >= ((r - 2^-40) * cell)^2 + o2. The margins (1/16 of a cell, 2^-20 of o2) cover the
 * rounding of rule 2, whose s is relatively accurate to 2^-40 provided cell >= 2^-20 * the largest coordinate magnitude of B -- THE CONDITION THE PROOF NEEDS; it holds
 * for every float mesh whose box is not thinner than 2^-4 of the float spacing at its coordinates along its longest axis. So a triangle in an unvisited cell has a
 * computed s above best_s: every triangle that attains the minimum has been visited, the lowest index among them included. The o2 term is what lets a sample far
 * outside the box stop after a few shells.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, from, to or opt; from == to; both outputs non-null and equal; a wrong version;
 * level > 3; unit, max_distance or a tau negative or not finite; unit == 0; cells > 256; n_indices % 3 != 0 or a null vertex or index buffer on either side; indices
 * without vertices. After the range-check kernel: an index >= n_verts, a coordinate of a used vertex that is not finite (either mesh). Later: B without a non-degenerate
 * triangle, the large list or the cell lists too long, a term or a sum out of range. On failure the outputs hold nothing of use, *stats is zeroed and the context
 * stays usable. An A without triangles succeeds with zero sums, every vertex unused (B is then not looked at beyond its counts, and no grid is built).
 *
 * Workspace: one word per vertex of A and of B, two words per cell, one word per cell entry, a few hundred bytes; released before the call returns. Reads nothing of
 * the training state; work pending on the context's side streams is joined first. A handful of small device-to-host reads; syncs. */
int rnb_mesh_distance(rnb_ctx* ctx, void* stream, const rnb_mesh* from, const rnb_mesh* to, const rnb_mesh_distance_options* opt, float* vert_dist_dev /* may be NULL */,
                      uint32_t* vert_nearest_dev /* may be NULL */, rnb_mesh_distance_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_DISTANCE_H */
