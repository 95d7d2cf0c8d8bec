/*
 * rnb_mesh_project.h — C-ABI of the view projection of librnb_neus2_hip: an indexed triangle mesh in device memory gets the texture baker's per-triangle atlas, and every
 * texel of it is coloured from a set of calibrated images -- projected into each camera, tested for occlusion against the mesh rasteriser's depth of that camera, sampled
 * and blended. The call reads nothing of the model: it textures a ground-truth mesh, a mesh from another tool or the pipeline's own mesh alike, from the albedo maps the
 * model was trained on or from the photographs beside them.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the ABIs of the other mesh stages are not affected by this header. The rules of the mesh rasteriser (rnb_mesh_raster and its header, rules 1-6) and the
 * layout and the texel rules of the texture baker (rnb_mesh_texture_layout, rnb_mesh_bake_texture and their header) are used by number and by name below and are not
 * restated: this call runs the rasteriser's fill and the baker's texel function, so what their outputs show is what is used here.
 */
#ifndef RNB_MESH_PROJECT_H
#define RNB_MESH_PROJECT_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_PROJECT_ABI_VERSION 1

#define RNB_MESH_PROJECT_NONE 0xFFFFFFFFu     /* info[..][1] of a texel no view contributes to */
#define RNB_MESH_PROJECT_MAX_WEIGHT_POWER 8u

#define RNB_MESH_PROJECT_FORMAT_F32 0         /* float[h][w][4] */
#define RNB_MESH_PROJECT_FORMAT_U16 1         /* uint16[h][w][4]: a value x reads as (double) x / 65535 */
#define RNB_MESH_PROJECT_FORMAT_U8 2          /* uint8[h][w][4]: a value x reads as (double) x / 255 */

#define RNB_MESH_PROJECT_MODE_BLEND 0
#define RNB_MESH_PROJECT_MODE_BEST 1

#define RNB_MESH_PROJECT_NORMALS_FACE 0
#define RNB_MESH_PROJECT_NORMALS_VERTEX 1

typedef struct rnb_mesh_project_view {
	rnb_view    view;         /* the camera (pinhole, no distortion), W = view.width, H = view.height, each 1 .. 16384 */
	const void* image_dev;    /* RGBA, 4 channels interleaved, row 0 on top, in device memory, aligned to one pixel (16, 8 or 4 bytes); alpha is the mask */
	uint32_t    image_width;  /* iw, ih: any size > 0, not necessarily the view's */
	uint32_t    image_height;
	uint32_t    format;       /* RNB_MESH_PROJECT_FORMAT_* */
	uint32_t    reserved;     /* 0 */
} rnb_mesh_project_view;

typedef struct rnb_mesh_project_options {
	uint32_t     abi_version;     /* RNB_MESH_PROJECT_ABI_VERSION */
	uint32_t     size;            /* S, as in the texture baker's options; default 1024 */
	uint32_t     block;           /* b, likewise; 0 (default) = the largest that holds the mesh. The atlas is rnb_mesh_texture_layout's, unchanged */
	uint32_t     mode;            /* RNB_MESH_PROJECT_MODE_*; default BLEND */
	uint32_t     normals;         /* RNB_MESH_PROJECT_NORMALS_*: which normal weights a view; default FACE. VERTEX needs mesh->normals */
	uint32_t     weight_power;    /* k = 0 .. RNB_MESH_PROJECT_MAX_WEIGHT_POWER: the exponent of the cosine weight; default 2 */
	float        min_cos;         /* [0, 1): a view at a flatter angle is skipped; default 0.1 */
	float        depth_tolerance; /* >= 0 and finite: the relative depth slack of the occlusion test; default 2^-8 */
	float        near;            /* the rasteriser's rule 2; > 0 and finite; default 2^-10 */
	uint32_t     cull;            /* the rasteriser's cull (0 none, 1 back, 2 front), passed to the fill; default none */
	const float* fallback_dev;    /* device float[S][S][4], or NULL (default): copied into the owned texels no view contributes to */
	uint32_t     reserved[4];     /* 0 */
} rnb_mesh_project_options;

typedef struct rnb_mesh_projection {
	float*    uv;    /* device float[n_tris][3][2]: bit for bit the uv of rnb_mesh_bake_texture for the same mesh, size and block */
	float*    color; /* device float[S][S][4]; row 0 is the top row of an image file */
	uint32_t* info;  /* device uint32[S][S][2]: the number of contributing views, and the best view (RNB_MESH_PROJECT_NONE if none) */
	uint32_t  size, block, blocks_per_row, n_tris;
} rnb_mesh_projection;

typedef struct rnb_mesh_project_stats {
	uint64_t n_texels;       /* owned texels: those of an existing triangle */
	uint64_t n_textured;     /* of those: count > 0 */
	uint64_t n_pairs_tested; /* (texel, view) pairs that passed P2 and reached the occlusion test */
	uint64_t n_occluded;     /* of those: occluded (P3) */
	uint64_t peak_workspace; /* bytes of device memory the call held at its peak, the result included */
	float    ms;             /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_project_stats;

uint32_t rnb_mesh_project_abi_version(void);
/* Fills *opt with the defaults: size 1024, block 0, BLEND, FACE, weight_power 2, min_cos 0.1, depth_tolerance 2^-8, near 2^-10, no culling, no fallback. */
int rnb_mesh_project_default_options(rnb_mesh_project_options* opt);

/* mesh: an indexed triangle mesh in device memory, not modified; its colours are not read, its normals only with normals = VERTEX. views: n_views records in HOST memory
 * (their images in device memory). *out receives the atlas and the two maps, in device memory the call allocates; release them with rnb_mesh_projection_free.
 *
 * Arithmetic. Double precision with every operation rounded on its own (no fused multiply-add, IEEE division and square root); floats are widened first;
 * dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z, as in rule 1 of the rasteriser. W, H, iw, ih and the integer weights are converted exactly.
 *
 * P1. Texel. Which triangle owns a texel, its integer weights (a0, a1, a2) over n = b - 3 and its position p (a float, widened again) are the texture baker's.
 *     normals = FACE: for the texel's triangle in the mesh's own order u = v1 - v0, v = v2 - v0, nn = cross(u, v) as in rule 6 of the rasteriser, l = sqrt(dot(nn, nn)),
 *     N = nn / l per component (a double: it is not rounded to float). normals = VERTEX: s = (a0 * n0 + a1 * n1) + a2 * n2 per component with the vertices'
 *     mesh->normals, l = sqrt(dot(s, s)), N = s / l. A texel whose l is 0 or not finite takes no view.
 * P2. Per view v, in ascending order. o, col_k are those of rule 1 of the rasteriser; e = p - o, xc = dot(col_0, e), yc = dot(col_1, e), zc = dot(col_2, e).
 *     Skipped if zc < (double) near. d = -e; c = dot(N, d) / sqrt(dot(d, d)); skipped if !(c > (double) min_cos). sx, sy by rule 3, not snapped;
 *     i = floor(sx), j = floor(sy); skipped if sx or sy is not finite or (i, j) lies outside [0, W) x [0, H).
 * P3. Occlusion. z_win = the rasteriser's float depth of the winner of pixel (i, j) of view v (rule 5), from the same fill with this call's near and cull. The texel
 *     is occluded, and the view skipped, if the pixel has a winner and zc > (double) z_win * (1 + (double) depth_tolerance) (the sum, then the product). A pixel that no
 *     triangle covers occludes nothing.
 * P4. Sample. u = sx * iw / W - 0.5, v = sy * ih / H - 0.5: the product, then the division, then the subtraction. i0 = floor(u), fu = u - i0; j0 = floor(v),
 *     fv = v - j0. The taps 00, 10, 01, 11 are the pixels (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1), each coordinate clamped to the image. Their weights
 *     b = (1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv. With a_k the alpha and c_k a colour channel of tap k, read by the format's rule (F32: widened):
 *     q_a = ((b_0 * a_0 + b_1 * a_1) + b_2 * a_2) + b_3 * a_3 and q_c = ((b_0 * (a_0 * c_0) + b_1 * (a_1 * c_1)) + b_2 * (a_2 * c_2)) + b_3 * (a_3 * c_3): the sample is
 *     premultiplied. Skipped if q_a == 0. The values are blended as stored: there is no colour-space conversion.
 * P5. Weight. g = 1, multiplied k = weight_power times by c, one after the other; wv = g * q_a. The view contributes: count += 1; A += g * q_c per channel and
 *     Q += wv; and if wv > w_best (w_best starts at minus infinity), best = v, w_best = wv, and q_c and q_a are remembered as those of the best view.
 * P6. Result. An owned texel with count > 0: BLEND rgb = (float) (A / Q); BEST rgb = (float) (q_c / q_a) of the best view; alpha 1; info = (count, best). An owned
 *     texel with count == 0: the texel of fallback_dev, all four channels, if a fallback was given, otherwise rgb 0 and alpha 1; info = (0, RNB_MESH_PROJECT_NONE).
 *     Every texel that is not owned is all zeros in both maps, as in the baker. F32 images are taken as they are: an alpha outside [0, 1] or a value that is not finite
 *     goes through these rules as written.
 * P7. Consequences. The same input gives the same bits, and nothing about how the work is cut changes one. With normals = VERTEX the n + 1 texels along an edge two
 *     triangles share are bit-identical in color and info in both: position (the baker's statement), normal (the same two-term sum) and with them every view's decision
 *     are functions of equal bits. A permutation of the views leaves count unchanged (every decision of P2-P4 is made view by view). Views that all hold one constant
 *     opaque colour give that colour on every texel with count > 0, within 1 ulp (expected: exactly).
 *
 * stats: n_texels, n_textured, n_pairs_tested, n_occluded, peak_workspace, ms.
 *
 * How it is done (none of it can change a result). The owned texels are numbered block-major, as the baker numbers them. One kernel writes p and N of every texel.
 * Then view by view: the rasteriser's own fill (the same kernels) into a key buffer allocated once for the largest view, and one thread per texel that does P2-P5 and
 * updates the texel's accumulators in memory -- only that thread writes them, in view order, without atomics. A last kernel does P6 and writes the corners' (U, V).
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, mesh, views, opt or out; n_views == 0; a wrong version; size, block, mode,
 * normals, weight_power, min_cos, depth_tolerance, near or cull out of range; a reserved word not 0; normals = VERTEX with mesh->normals null; per view: a focal length
 * not finite or <= 0, a principal point or an entry of xform not finite, width or height 0 or above 16384, a null or misaligned image, an image size of 0, an unknown
 * format, a reserved word not 0; n_indices % 3 != 0; a null vertex or index buffer; indices without vertices; a mesh the layout does not hold (the layout's message,
 * which ends in the smallest size that would fit). After the range-check kernel: an index >= n_verts. On failure *out and *stats are zeroed, nothing stays allocated and
 * the context stays usable. A mesh without triangles succeeds with all-zero maps.
 *
 * Workspace: the result (24 bytes per texel of the texture, 24 bytes per triangle), 12 bytes per pixel of the largest view, and per owned texel 84 bytes (p, N and the
 * accumulators); all but the result released before the call returns. Reads nothing of the training state; work pending on the context's side streams is joined first.
 * One small device-to-host read per view; syncs. */
int rnb_mesh_project_views(rnb_ctx* ctx, void* stream, const rnb_mesh* mesh, const rnb_mesh_project_view* views /* host */, uint32_t n_views, const rnb_mesh_project_options* opt,
                           rnb_mesh_projection* out, rnb_mesh_project_stats* stats /* may be NULL */);

/* Releases what rnb_mesh_project_views allocated and zeroes *out. */
int rnb_mesh_projection_free(rnb_ctx* ctx, rnb_mesh_projection* out);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_PROJECT_H */
