/*
 * rnb_mesh_draw.h — C-ABI of the textured draw of librnb_neus2_hip: an indexed triangle mesh in device memory with a texture atlas (per-corner texture coordinates, a
 * colour map, a world-frame normal map, or both) seen from one pinhole camera, in the channel layout of the mesh rasteriser's image and of the inference tracer's. It is
 * the inverse of texturing: what the texture baker wrote, or what was blended into its atlas from the input views, is looked at again through a camera, so that the
 * per-view numbers (normal angle against the input normal maps, albedo error against the input albedo maps) cover the delivered asset, normal map and texels included,
 * and not the bare geometry.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the ABIs of the other mesh stages are not affected by this header. The rules of the mesh rasteriser (rnb_mesh_raster and its header, rules 1-7) are used
 * by number below and are not restated: this call runs the rasteriser's fill, so what the rasteriser's image shows in channels 6-8 is what this one shows.
 *
 * rnb_mesh_draw_stats embeds rnb_mesh_raster_stats: include the mesh rasteriser's header before this one.
 */
#ifndef RNB_MESH_DRAW_H
#define RNB_MESH_DRAW_H

#include "rnb_mesh_texture.h"

#ifndef RNB_MESH_RASTER_ABI_VERSION
#error "rnb_mesh_draw.h: include the header of rnb_mesh_raster first (rnb_mesh_draw_stats embeds rnb_mesh_raster_stats)"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_DRAW_ABI_VERSION 1

#define RNB_MESH_DRAW_FILTER_NEAREST 0
#define RNB_MESH_DRAW_FILTER_BILINEAR 1

typedef struct rnb_mesh_draw_texture {
	const float* uv_dev;     /* device float[n_tris][3][2]: (U, V) of the corners in the order of the indices (the uv of rnb_mesh_bake_texture, or any other) */
	const float* color_dev;  /* device float[S][S][4], row 0 on top, 16-byte aligned, or NULL */
	const float* normal_dev; /* device float[S][S][4], world-frame normal in 0-2 (the baker's normal map), 16-byte aligned, or NULL; not both NULL */
	uint32_t     size;       /* S: 1 .. RNB_MESH_TEXTURE_MAX_SIZE */
	uint32_t     n_tris;     /* must equal mesh->n_indices / 3 */
} rnb_mesh_draw_texture;

typedef struct rnb_mesh_draw_options {
	uint32_t abi_version; /* RNB_MESH_DRAW_ABI_VERSION */
	float    near;        /* the rasteriser's rule 2; > 0 and finite; default 2^-10 */
	uint32_t cull;        /* the rasteriser's RNB_MESH_RASTER_CULL_*; default NONE */
	uint32_t normals;     /* the rasteriser's RNB_MESH_RASTER_NORMALS_*: the normal of rule 6, shown where no normal map decides; default FACE */
	uint32_t filter;      /* RNB_MESH_DRAW_FILTER_*; default BILINEAR */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_draw_options;

typedef struct rnb_mesh_draw_stats {
	rnb_mesh_raster_stats raster; /* exactly what rnb_mesh_raster reports for the same mesh, view, near and cull (ms and peak_workspace are this call's) */
	uint32_t n_bad_uv;            /* covered pixels whose texel coordinate is not finite (T3) */
	uint32_t n_normal_fallback;   /* covered pixels where the normal map gave no direction (T5) */
	uint32_t n_unowned_taps;      /* covered pixels with a tap of non-zero weight whose alpha (of the colour map, else of the normal map) is 0 */
	uint32_t reserved;
} rnb_mesh_draw_stats;

uint32_t rnb_mesh_draw_abi_version(void);
/* Fills *opt with the defaults: near 2^-10, no culling, face normals, bilinear. */
int rnb_mesh_draw_default_options(rnb_mesh_draw_options* opt);

/* mesh: an indexed triangle mesh in device memory, not modified; its colours are read only without a colour map, its normals only with normals = VERTEX. tex: the
 * atlas, in HOST memory (its buffers in device memory). view: the camera, H = height, W = width. out_dev: float[H][W][9] in device memory, the rasteriser's layout:
 * 0-2 unit normal in the world frame, 3-5 colour, 6 coverage, 7 depth, 8 depth complexity. face_dev: uint32[H][W] in device memory, or NULL.
 *
 * Arithmetic, as in the rasteriser: double precision with every operation rounded on its own (no fused multiply-add, IEEE division and square root); floats are
 * widened first; S is converted exactly; dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z.
 *
 * T1. Fill. Rules 1-5 of the rasteriser, run by the rasteriser's own kernels. Channels 6, 7 and 8, face_dev and every field of stats.raster except ms (a time) and
 *     peak_workspace (a size) are bit for bit what rnb_mesh_raster writes for the same mesh, view, near and cull. An uncovered pixel is all zeros.
 * T2. Texture coordinate. For the winner of a pixel m_a, m_b, m_c are those of rule 6, after the swap of rule 4; the swap moves the corners' (U, V) with their
 *     vertices. U = (m_a * U_a + m_b * U_b) + m_c * U_c, and V likewise.
 * T3. Texel coordinate. x = U * S - 0.5, y = (1 - V) * S - 0.5: the baker's convention, V = 1 at the top edge of row 0, texel (i, j) of column i and row j has its
 *     centre at (i, j). If x or y is not finite the pixel counts in n_bad_uv, neither map is read for it, its colour is zeros where a colour map was given, and its
 *     normal is that of rule 6; it counts in neither of the other two counters. Otherwise both are clamped to [-1, S] and the maps are sampled:
 *     BILINEAR: i0 = floor(x), fu = x - i0, j0 = floor(y), fv = y - j0. The taps 00, 10, 01, 11 are the texels (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1),
 *     each coordinate clamped to [0, S - 1]. Their weights b = (1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv. A channel's value is
 *     ((b_0 * t_0 + b_1 * t_1) + b_2 * t_2) + b_3 * t_3 with t_k the channel of tap k.
 *     NEAREST: the one texel (floor(x + 0.5), floor(y + 0.5)), clamped likewise, with weight 1: a channel's value is the texel's, widened.
 *     A pixel with a tap whose weight is not 0 and whose alpha (channel 3 of the colour map, or of the normal map where no colour map was given) is 0 counts in
 *     n_unowned_taps: it looked at a texel no triangle owns. Its value is what the rule above gives.
 * T4. Colour. With color_dev: channels 3-5 are (float) of the sampled channels 0-2. Values are straight: no alpha weighting and no colour-space conversion.
 *     Without color_dev: the colour of rule 6.
 * T5. Normal. With normal_dev: s = the sampled channels 0-2, l = sqrt(dot(s, s)). If l is finite and > 0, channels 0-2 are (float) (s / l) per component. Otherwise
 *     they are the normal of rule 6 as `normals` selects it, and n_normal_fallback counts the pixel. Without normal_dev: rule 6.
 * T6. Consequences. The same input gives the same bits, and nothing about the launch shape changes one. If every tap of non-zero weight holds the constant c in the
 *     colour map, the pixel shows c within 1 ulp (expected: exactly). With the baker's atlas and its position map passed as color_dev every covered pixel shows
 *     (m_a * v_a + m_b * v_b) + m_c * v_c, the point of the triangle under the pixel, up to the rounding of uv, of the texels and of the output: the position map is
 *     affine over a triangle's whole block, gutter included. A permutation of the triangles, with uv permuted alongside, changes only what rule 7 allows.
 *
 * stats: raster (n_tris ... n_fragments, peak_workspace, ms), n_bad_uv, n_normal_fallback, n_unowned_taps.
 *
 * How it is done (none of it can change a result). The rasteriser's range check and fill, unchanged. Then one thread per pixel: the winner's setup, weights and depth
 * again by the rasteriser's device functions, T2-T5 with one 16-byte load per tap and map, the nine channels through LDS and out as 16-byte stores when the image is
 * aligned; the three counters packed into one wavefront reduction and added once per wavefront.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, mesh, tex, view, opt or out_dev; out_dev == face_dev; a wrong version; near,
 * cull, normals or filter out of range; a reserved word not 0; both maps null; a map not 16-byte aligned; a null uv_dev with n_tris > 0; size 0 or above
 * RNB_MESH_TEXTURE_MAX_SIZE; tex->n_tris != mesh->n_indices / 3; normals = VERTEX with mesh->normals null; and everything rnb_mesh_raster refuses about the view and
 * the mesh. After the range-check kernel: an index >= n_verts. On failure the outputs hold nothing of use, *stats is zeroed and the context stays usable. A mesh without
 * triangles succeeds with an empty image.
 *
 * Workspace: the rasteriser's (12 bytes per pixel, one word per vertex, one word per large triangle, a few dozen bytes); released before the call returns. Reads nothing
 * of the training state; work pending on the context's side streams is joined first. Two or three small device-to-host reads; syncs. */
int rnb_mesh_draw_textured(rnb_ctx* ctx, void* stream, const rnb_mesh* mesh, const rnb_mesh_draw_texture* tex /* host */, const rnb_view* view, const rnb_mesh_draw_options* opt,
                           float* out_dev, uint32_t* face_dev /* may be NULL */, rnb_mesh_draw_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_DRAW_H */
