/*
 * rnb_mesh_simplify.h — C-ABI of the mesh simplifier of librnb_neus2_hip: vertex clustering of an indexed triangle mesh in device memory on a uniform cell grid, the
 * representative vertex of a cell placed by quadric error minimisation (or at the mean of its members). It turns a fine extraction (rnb_extract_mesh, rnb_mesh.h;
 * cleaned by rnb_mesh_clean, rnb_mesh_clean.h) into a mesh of a chosen size before it is downloaded and written.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the mesh-clean ABI are not affected by this header.
 */
#ifndef RNB_MESH_SIMPLIFY_H
#define RNB_MESH_SIMPLIFY_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_SIMPLIFY_ABI_VERSION 1

#define RNB_MESH_PLACE_QUADRIC 0 /* the minimiser of the regularised quadric of the cluster, kept inside the cell (below) */
#define RNB_MESH_PLACE_MEAN 1    /* the mean of the member vertices */

#define RNB_MESH_SIMPLIFY_MAX_DIM 4096u              /* cells per axis */
#define RNB_MESH_SIMPLIFY_MAX_CELLS (1ull << 30)     /* dims[0] * dims[1] * dims[2] may not exceed this (1024^3): the call holds one bit per cell and one prefix-sum word per 32 cells */

/* Fixed point of every summed term: q = (int64) trunc(term * 2^RNB_MESH_SIMPLIFY_Q_SHIFT), rounding towards zero. A term must be finite and smaller than
 * 2^RNB_MESH_SIMPLIFY_Q_TERM_LOG2 in magnitude, else the call fails. Why 2^22: a triangle whose corners lie within 64 cells of the cluster's centre per axis has edges
 * below 128 per axis, |n| < 2 * 128^2 * sqrt(3) < 2^16, w < 2^15, |d| <= |a| < 2^7, so w * d * n_i < 2^22 and every other term is smaller: such a triangle is always
 * accepted. A sum cannot overflow while the sum of the magnitudes of its terms stays below 2^(63 - 40) = 8 388 608 (cell units; integer sums wrap, they do not trap). */
#define RNB_MESH_SIMPLIFY_Q_SHIFT 40
#define RNB_MESH_SIMPLIFY_Q_TERM_LOG2 22

typedef struct rnb_mesh_simplify_options {
	uint32_t abi_version; /* RNB_MESH_SIMPLIFY_ABI_VERSION */
	float    origin[3];   /* the low corner of cell (0, 0, 0); finite */
	float    cell;        /* edge of a cell; > 0 and finite */
	uint32_t dims[3];     /* cells per axis, 1 .. RNB_MESH_SIMPLIFY_MAX_DIM each, product <= RNB_MESH_SIMPLIFY_MAX_CELLS */
	uint32_t placement;   /* RNB_MESH_PLACE_QUADRIC (default) or RNB_MESH_PLACE_MEAN */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_simplify_options;

typedef struct rnb_mesh_simplify_stats {
	uint32_t n_verts_in;
	uint32_t n_tris_in;
	uint32_t n_clusters;       /* occupied cells: cells that hold a vertex some triangle uses */
	uint32_t n_verts_out;      /* clusters a surviving triangle uses */
	uint32_t n_tris_out;
	uint32_t n_tris_collapsed; /* n_tris_in - n_tris_out */
	uint32_t n_clamped;        /* output vertices whose position the cell box cut on at least one axis */
	uint32_t n_fallback;       /* output vertices placed at the mean because the system was unusable (RNB_MESH_PLACE_QUADRIC only) */
	uint64_t peak_workspace;   /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;               /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_simplify_stats;

uint32_t rnb_mesh_simplify_abi_version(void);
/* Fills *opt with the defaults: origin (0, 0, 0), cell 1 / 256, dims 256^3 (the unit box in 256 cells per axis), quadric placement. */
int rnb_mesh_simplify_default_options(rnb_mesh_simplify_options* opt);

/* in: any indexed triangle mesh in device memory (verts, indices, optionally colors and / or normals); it is not modified and must not be *out.
 *
 * Arithmetic. Everything below is double precision with every operation rounded on its own (no fused multiply-add, IEEE division and square root); floats are widened
 * first. Sums are 64-bit fixed point (above) added as integers: they depend neither on the order of the additions nor on the launch shape. S(.) below is such a sum
 * read back as (double) sum * 2^-40.
 *
 * 1. Cell of a vertex v that a triangle uses (a vertex no triangle uses takes no part), per axis k:
 *      p_k = ((double) v_k - (double) origin_k) / (double) cell;   i_k = min(max(floor(p_k), 0), dims_k - 1);   key = i_x + dims_x * (i_y + dims_y * i_z)
 *    The cluster id of an occupied cell is the rank of its key among the occupied keys in ascending order.
 * 2. Local frame of a cluster: cell units around its cell centre, x_k = p_k - ((double) i_k + 0.5) with i the cluster's cell. A member lies in [-0.5, 0.5) per axis,
 *    or beyond if it was clamped in from outside the grid.
 * 3. Sums per cluster. Over its member vertices: count, S(x_k) (3), and for carried attributes S(colour_k) (3), S(normal_k) (3). Over every input triangle (a, b, c) one of
 *    whose corners is a member -- once per triangle and cluster, a triangle that will collapse included -- with its three corners taken in the cluster's frame:
 *      u = b - a, v = c - a, n = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x), l = sqrt((n.x * n.x + n.y * n.y) + n.z * n.z)
 *      l == 0: nothing. Else w = 0.5 * l, h_k = n_k / l, d = -((h.x * a.x + h.y * a.y) + h.z * a.z), g_k = w * h_k, and the nine terms
 *      A_xx = g.x * h.x, A_xy = g.x * h.y, A_xz = g.x * h.z, A_yy = g.y * h.y, A_yz = g.y * h.z, A_zz = g.z * h.z, b_k = g_k * d.
 * 4. Placement. m_k = S(x_k) / (double) count. RNB_MESH_PLACE_MEAN: x = m. RNB_MESH_PLACE_QUADRIC: t = (A_xx + A_yy) + A_zz, e = t * 2^-10,
 *      m00 = A_xx + e, m11 = A_yy + e, m22 = A_zz + e, m01 = A_xy, m02 = A_xz, m12 = A_yz, r_k = e * m_k - b_k
 *      c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11, c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01
 *      det = (m00 * c00 + m01 * c01) + m02 * c02
 *      x_0 = ((c00 * r_0 + c01 * r_1) + c02 * r_2) / det, x_1 = ((c01 * r_0 + c11 * r_1) + c12 * r_2) / det, x_2 = ((c02 * r_0 + c12 * r_1) + c22 * r_2) / det
 *    (the minimiser of the summed squared plane distances plus e |x - m|^2). If t == 0, or not det > 0, or an x_k is not finite: x = m (n_fallback).
 *    Then, either placement, x_k is clamped to [-0.5, 0.5] (n_clamped counts the vertices with at least one axis cut), and the position is
 *      (float) ((((double) i_k + 0.5) + x_k) * (double) cell + (double) origin_k).
 *    Colour: (float) (S(colour_k) / (double) count). Normal: s_k = S(normal_k), l = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z), (float) (s_k / l), zero if l == 0.
 * 5. Triangles. Each corner becomes its cluster. A triangle two of whose corners are equal is dropped; the others stay in input order with their winding. Vertices:
 *    the clusters a surviving triangle uses, in ascending key, renumbered by prefix sums. Duplicate triangles and the non-manifold edges clustering can create
 *    are KEPT; removing them is not this call's job (rnb_mesh_repair of rnb_mesh_topology.h removes the duplicates, rnb_mesh_topology counts the edges).
 *
 * Consequences: the same input gives the same bits; a permutation of the input's triangles permutes the output's triangles and changes nothing else; a renumbering
 * of the input's vertices changes nothing at all.
 *
 * Failure with RNB_ERR_INVALID: n_indices % 3 != 0, an index >= n_verts (range-checked by a kernel before any index is used as an address), a coordinate or carried
 * attribute of a used vertex that is not finite, a term that is not below its bound; and, before the context or the device is touched, a null or in-place argument, indices without
 * vertices, a wrong version, an unknown placement, a cell that is not finite and > 0, an origin that is not finite, dims outside 1 .. 4096 or with a product above
 * RNB_MESH_SIMPLIFY_MAX_CELLS. On failure *out is zeroed and the context stays usable. An empty input (n_indices == 0) succeeds with an empty *out.
 *
 * On success *out owns its device buffers (colors / normals exactly when the input has them): release them with rnb_mesh_free. Workspace: two 4-byte words per input
 * vertex, one bit and one prefix-sum word per 32 cells, 164 bytes per cluster, one word per 256 triangles, the output; released before the call returns. Reads nothing of
 * the training state; work pending on the context's side streams is joined first. A handful of small device-to-host reads; syncs. */
int rnb_mesh_simplify(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_simplify_options* opt, rnb_mesh* out, rnb_mesh_simplify_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_SIMPLIFY_H */
