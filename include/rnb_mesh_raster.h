/*
 * rnb_mesh_raster.h — C-ABI of the mesh rasteriser of librnb_neus2_hip: an indexed triangle mesh in device memory seen from one pinhole camera, as the depth, normal,
 * colour, coverage and face maps of that view, in the channel layout of the inference tracer's image. It gives the mesh the pipeline delivers the per-view numbers the
 * model's render has (normal angle against the input maps, mask IoU), where no ground-truth mesh exists to measure against.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the ABIs of the other mesh stages are not affected by this header.
 */
#ifndef RNB_MESH_RASTER_H
#define RNB_MESH_RASTER_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_RASTER_ABI_VERSION 1

#define RNB_MESH_RASTER_CHANNELS 9u           /* = RNB_RENDER_CHANNELS of the inference tracer: what consumes a render consumes this */
#define RNB_MESH_RASTER_NONE 0xFFFFFFFFu      /* face_dev of an uncovered pixel */
#define RNB_MESH_RASTER_MAX_SIZE 16384u       /* pixels per side */
#define RNB_MESH_RASTER_SUBPIXEL_BITS 8       /* screen coordinates are snapped to 1/256 pixel (rule 3) */
#define RNB_MESH_RASTER_MAX_COORD_LOG2 28     /* a snapped coordinate beyond +-2^28 takes its triangle out (rule 3) */
#define RNB_MESH_RASTER_SMALL_PIXELS 16u      /* a triangle whose pixel box holds at most this many pixels is filled by the thread that set it up */
#define RNB_MESH_RASTER_MAX_COUNT 16777216u   /* channel 8 saturates here (2^24: every count below is a float) */

#define RNB_MESH_RASTER_CULL_NONE 0
#define RNB_MESH_RASTER_CULL_BACK 1
#define RNB_MESH_RASTER_CULL_FRONT 2

#define RNB_MESH_RASTER_NORMALS_FACE 0
#define RNB_MESH_RASTER_NORMALS_VERTEX 1

typedef struct rnb_mesh_raster_options {
	uint32_t abi_version; /* RNB_MESH_RASTER_ABI_VERSION */
	float    near;        /* rule 2; > 0 and finite; default 2^-10 */
	uint32_t cull;        /* RNB_MESH_RASTER_CULL_*; default NONE */
	uint32_t normals;     /* RNB_MESH_RASTER_NORMALS_*; default FACE */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_raster_options;

typedef struct rnb_mesh_raster_stats {
	uint32_t n_tris;
	uint32_t n_behind;       /* triangles with a vertex not in front (rule 2) */
	uint32_t n_out_of_range; /* of the others: a screen coordinate not finite or beyond the fixed-point range (rule 3) */
	uint32_t n_degenerate;   /* of the others: A2 == 0 (rule 4) */
	uint32_t n_culled;       /* of the others: taken out by `cull` */
	uint32_t n_offscreen;    /* of the others: the box misses the image or holds no pixel centre */
	uint32_t n_small;        /* of the others: at most RNB_MESH_RASTER_SMALL_PIXELS pixels in the box */
	uint32_t n_large;        /* the rest; the seven counts add up to n_tris */
	uint32_t n_covered;      /* pixels with coverage 1 */
	uint32_t n_back_pixels;  /* of those: the winner is back-facing */
	uint64_t n_fragments;    /* the sum of channel 8 */
	uint64_t peak_workspace; /* bytes of device memory the call held at its peak */
	float    ms;             /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_raster_stats;

uint32_t rnb_mesh_raster_abi_version(void);
/* Fills *opt with the defaults: near 2^-10, no culling, face normals. */
int rnb_mesh_raster_default_options(rnb_mesh_raster_options* opt);

/* mesh: an indexed triangle mesh in device memory, not modified. view: the camera (pinhole, no distortion; the rnb_view of rnb_set_dataset and rnb_render), H = height,
 * W = width. out_dev: float[H][W][RNB_MESH_RASTER_CHANNELS] in device memory. face_dev: uint32[H][W] in device memory, or NULL.
 *
 * The image, per pixel:
 *   0-2  unit normal, world frame (rule 6)
 *   3-5  colour: mesh->colors interpolated, or ones for a mesh without colours
 *   6    coverage, 1 or 0
 *   7    depth along the camera's forward axis
 *   8    the number of triangles that cover the pixel's centre, front and back (the depth complexity), as a float, saturated at 2^24
 * face_dev: the winning triangle (position in the index list / 3), RNB_MESH_RASTER_NONE where nothing covers. An uncovered pixel is all zeros.
 *
 * Arithmetic. Double precision with every operation rounded on its own (no fused multiply-add, IEEE division and square root); floats are widened first.
 * dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z. Coverage is decided in 64-bit integers and is exact.
 *
 * 1. Camera. o = (xform[3], xform[7], xform[11]); col_k = (xform[k], xform[4 + k], xform[8 + k]), k = 0, 1, 2: the camera's right, down and forward axes in the world
 *    (camera_ray of the ray generator). The 3x3 block is taken as a rotation and its transpose as its inverse; the call does not check it. For a vertex p: e = p - o,
 *    xc = dot(col_0, e), yc = dot(col_1, e), zc = dot(col_2, e).
 * 2. In front. A vertex is in front if zc >= (double) near. A triangle with a vertex that is not in front is skipped whole (n_behind): there is no clipping. The cameras
 *    of this workflow stand outside the object, and a triangle drawn in part, with an edge the mesh does not have, would be worse than a triangle counted.
 * 3. Screen, fixed point. sx = fx * (xc / zc) + cx * W, sy = fy * (yc / zc) + cy * H in pixels (fx, fy = focal_length, cx, cy = principal_point, W and H converted
 *    exactly; the products cx * W and cy * H rounded once). Pixel (i, j), column i, row j, has its centre at (i + 0.5, j + 0.5): the convention of camera_ray with the
 *    principal point normalised. X = floor(sx * 256 + 0.5), Y = floor(sy * 256 + 0.5) as 64-bit integers. A triangle (all vertices in front) with a vertex whose sx or
 *    sy is not finite, or whose sx * 256 + 0.5 or sy * 256 + 0.5, floored, exceeds 2^28 in magnitude, is skipped (n_out_of_range). Images are at most 2^14 per side.
 * 4. Coverage, exact. E_pq(P) = (q.X - p.X) * (P.Y - p.Y) - (q.Y - p.Y) * (P.X - p.X) in 64-bit integers (no product exceeds 2^59). For the triangle (a, b, c) in
 *    the mesh's order A2 = E_ab(c). A2 == 0: skipped (n_degenerate). A2 < 0: front-facing; A2 > 0: back-facing (for vertices in front the sign of A2 is that of
 *    dot(cross(b - a, c - a), a - o), up to the snapping: y points down on the screen). cull = BACK skips the back-facing, cull = FRONT the front-facing triangles
 *    (n_culled), before anything is drawn. If A2 < 0, b and c are swapped and A2 negated FOR EVERYTHING BELOW IN RULES 4-6 except the face normal and
 *    n_back_pixels: (a, b, c) is from here on the swapped triple, A2 > 0, and the weights are non-negative inside.
 *    Pixel box: i from max(0, ceil((min X - 128) / 256)) to min(W - 1, floor((max X - 128) / 256)), j likewise with Y and H: the pixels of the image whose centres
 *    lie in the closed box of the three snapped vertices. An empty box: skipped (n_offscreen). At most RNB_MESH_RASTER_SMALL_PIXELS pixels in the box: n_small;
 *    otherwise n_large. Which of the two only decides who fills the triangle, never a bit of the image.
 *    The centre of pixel (i, j) is P = (256 i + 128, 256 j + 128). w_a = E_bc(P), w_b = E_ca(P), w_c = E_ab(P); w_a + w_b + w_c == A2. The pixel is covered if for
 *    each of the three, with its edge (p, q) and (dx, dy) = (q.X - p.X, q.Y - p.Y): w > 0, or w == 0 and (dy > 0 or (dy == 0 and dx > 0)).
 *    Consequence. After the swap the direction of an edge depends only on the side its third vertex lies on. Two triangles on opposite sides of a shared edge therefore
 *    see opposite directions, and a pixel centre on that edge belongs to exactly one of them, whatever their windings: a closed mesh seen from outside covers every
 *    pixel an even number of times, and a plane tiled by triangles covers every interior pixel centre exactly once, those on edges and vertices included.
 * 5. Depth and winner. For a covered pixel l_k = (double) w_k / (double) A2 (k = a, b, c; the conversions round to nearest), r_k = 1 / zc_k,
 *    iz = (l_a * r_a + l_b * r_b) + l_c * r_c, z = 1 / iz. key = ((uint64) bits((float) z) << 32) | triangle index. The winner of a pixel is the minimum key over the
 *    triangles that cover it: the nearest, and the lowest index among equal float depths (z > 0, so the bits order as the numbers). Channel 8 counts every covering
 *    triangle. A minimum and a sum of integers depend neither on the order of the updates nor on the launch shape.
 * 6. Resolve. For the winner w_k, l_k, r_k and z are computed again by the same formulas. m_k = (l_k * r_k) * z (the perspective-correct weights).
 *    Colour = (float) ((m_a * col_a + m_b * col_b) + m_c * col_c) per component; ones without mesh->colors. Depth = (float) z. Coverage = 1.
 *    Normal, normals = FACE: for the triangle in the mesh's own order (not swapped) u = b - a, v = c - a, n = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z,
 *    u.x * v.y - u.y * v.x), l = sqrt(dot(n, n)) (rule 1 of the mesh-to-mesh distance), normal = (float) (n / l) per component, zeros if l == 0.
 *    normals = VERTEX: s = (m_a * n_a + m_b * n_b) + m_c * n_c per component with the vertices' mesh->normals, l = sqrt(dot(s, s)), normal = (float) (s / l), zeros
 *    if l == 0. n_back_pixels counts the winners with A2 > 0 before the swap: 0 for a closed mesh that is turned outward and seen from outside.
 * 7. Consequences. The same input gives the same bits. A permutation of the triangles changes face_dev and, at pixels where several covering triangles have the
 *    winner's float depth, which of them wins there (and with it that pixel's normal and colour), and nothing else: coverage, depth and count never change, nor does
 *    any count of the statistics. A renumbering of the vertices changes nothing.
 *
 * How it is done (none of it can change a result). One thread per triangle does rules 1-4 up to the pixel box; a small triangle is filled by that thread, a large
 * one goes into a list that is sized by counting first (it cannot overflow) and is filled by one wavefront per triangle, 64 pixels per step. Per covered (triangle,
 * pixel): one 64-bit atomic minimum and one 32-bit atomic add. Then one thread per pixel resolves.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, mesh, view, opt or out_dev; out_dev == face_dev; a wrong version; near not
 * finite or <= 0; cull or normals out of range; a focal length not finite or <= 0; a principal point or an entry of xform not finite; width or height 0 or above
 * RNB_MESH_RASTER_MAX_SIZE; n_indices % 3 != 0; a null vertex or index buffer; indices without vertices; normals = VERTEX with mesh->normals null. After the
 * range-check kernel: an index >= n_verts. On failure the outputs hold nothing of use, *stats is zeroed and the context stays usable. A mesh without triangles
 * succeeds with an empty image. Coordinates need not be finite: a vertex that is not is behind or out of range by rules 2 and 3.
 *
 * Workspace: 12 bytes per pixel (keys and counts), one word per vertex, one word per large triangle, a few dozen bytes; released before the call returns. Reads nothing
 * of the training state; work pending on the context's side streams is joined first. Two or three small device-to-host reads; syncs. */
int rnb_mesh_raster(rnb_ctx* ctx, void* stream, const rnb_mesh* mesh, const rnb_view* view, const rnb_mesh_raster_options* opt, float* out_dev, uint32_t* face_dev /* may be NULL */,
                    rnb_mesh_raster_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_RASTER_H */
