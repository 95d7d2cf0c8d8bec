/*
 * rnb_mesh_texture.h — C-ABI of the texture baker of librnb_neus2_hip: an indexed triangle mesh in device memory gets a per-triangle UV atlas, and the model's albedo,
 * SDF-gradient normal and position are sampled at every texel of it. A simplified mesh carries one colour and one normal per grid cell; the trained network still holds
 * both fields at full resolution, and this stage samples them back onto the simplified surface.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the ABIs of the other mesh stages are not affected by this header.
 */
#ifndef RNB_MESH_TEXTURE_H
#define RNB_MESH_TEXTURE_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_TEXTURE_ABI_VERSION 1

#define RNB_MESH_TEXTURE_MIN_SIZE 4u          /* texels per side */
#define RNB_MESH_TEXTURE_MAX_SIZE 8192u
#define RNB_MESH_TEXTURE_MIN_BLOCK 4u         /* a block of 4 has legs of one texel step: the three corner texels and nothing between them */
#define RNB_MESH_TEXTURE_MAX_IN_FLIGHT 4194304u /* 2^22: a larger max_texels_in_flight is taken as this */

#define RNB_MESH_TEXTURE_ALBEDO 1u
#define RNB_MESH_TEXTURE_NORMAL 2u
#define RNB_MESH_TEXTURE_POSITION 4u

typedef struct rnb_mesh_texture_options {
	uint32_t abi_version;          /* RNB_MESH_TEXTURE_ABI_VERSION */
	uint32_t size;                 /* S: texels per side, RNB_MESH_TEXTURE_MIN_SIZE .. RNB_MESH_TEXTURE_MAX_SIZE; default 1024 */
	uint32_t block;                /* b: block edge in texels; 0 (default) = the largest that holds the mesh (layout, below) */
	uint32_t maps;                 /* RNB_MESH_TEXTURE_ALBEDO | _NORMAL | _POSITION, not 0; default ALBEDO */
	uint32_t use_inference_params; /* 1 (default): the EMA weights, as rnb_mesh_options */
	uint32_t max_texels_in_flight; /* texels per network batch; 0 = 2^20. Bounds the workspace; no bit of the result depends on it */
	uint32_t reserved[4];          /* 0 */
} rnb_mesh_texture_options;

typedef struct rnb_mesh_texture {
	float*   uv;       /* device float[n_tris][3][2]: (U, V) of the corners of every triangle, in the order of its indices */
	float*   albedo;   /* device float[S][S][4], or NULL when not asked for; row 0 is the top row of an image file */
	float*   normal;   /* likewise */
	float*   position; /* likewise */
	uint32_t size, block, blocks_per_row, n_tris;
} rnb_mesh_texture;

typedef struct rnb_mesh_texture_stats {
	uint64_t n_texels;       /* texels that went through the network: n_blocks * b * b, or 0 when only the position map was asked for */
	uint64_t peak_workspace; /* bytes of device memory the call held at its peak, the result included */
	uint32_t n_batches;      /* network launches */
	float    ms;             /* wall-clock time of the call */
} rnb_mesh_texture_stats;

uint32_t rnb_mesh_texture_abi_version(void);
/* Fills *opt with the defaults: size 1024, block 0, the albedo map, the EMA weights, max_texels_in_flight 0. */
int rnb_mesh_texture_default_options(rnb_mesh_texture_options* opt);

/* The layout of the atlas for n_tris triangles in a texture of `size` texels per side; `block` as in the options. A pure host function: it needs no context and no GPU.
 * Any of the three outputs may be NULL.
 *
 * Block k holds triangle 2k (the "lower" one) and triangle 2k + 1 (the "upper" one). blocks_per_row = floor(S / b); n_blocks = ceil(n_tris / 2), and it must be
 * <= blocks_per_row^2. With block = 0, b is the largest integer in [4, S] that satisfies this. If even b = 4 does not, or a given block is below 4, above S or does not
 * hold the mesh, the call fails with RNB_ERR_INVALID, as it does for a size out of range; a message about capacity ends in "the smallest size that would fit is N".
 *
 * Let n = b - 3, the length of a leg in texel steps. Block k has its origin at texel (ox, oy) = ((k mod blocks_per_row) * b, (k div blocks_per_row) * b). Within a block
 * texel (i, j) is column i, row j, each 0 .. b - 1; it belongs to the lower triangle if i + j <= b - 1 and to the upper one otherwise. The corners, as texel-centre
 * indices (ci, cj) within the block:
 *                v0                  v1                    v2
 *   lower        (0, 0)              (n, 0)                (0, n)
 *   upper        (b - 1, b - 1)      (b - 1 - n, b - 1)    (b - 1, b - 1 - n)
 * The upper triangle is a half-turn of the lower one, not its mirror image: all UV triangles have the same orientation. A corner at (ci, cj) has
 * U = (ox + ci + 0.5) / S and V = 1 - (oy + cj + 0.5) / S, computed in double precision and rounded to float once.
 *
 * Consequence. A bilinear lookup anywhere inside a triangle's UV triangle, edges included, gives a non-zero weight only to texels with i + j <= b - 2 (lower) or
 * i + j >= b (upper) of its own block: texels that belong to that triangle, never one across a block border (a lookup at a whole texel centre has neighbours of weight
 * zero, which do not count). The diagonal i + j = b - 1 between the two is read by neither. No dilation pass is needed, and there is none. */
int rnb_mesh_texture_layout(uint32_t n_tris, uint32_t size, uint32_t block, uint32_t* block_out, uint32_t* blocks_per_row_out, uint32_t* n_blocks_out);

/* mesh: an indexed triangle mesh in device memory, not modified; its colours and normals are not read. *out receives the atlas and the maps asked for, in device memory
 * the call allocates; release them with rnb_mesh_texture_free.
 *
 * Texel position. Double precision with every operation rounded on its own (no fused multiply-add); floats are widened first. For a lower texel (i, j) of a triangle
 * with the vertices v0, v1, v2 (in the order of its indices): (a0, a1, a2) = (n - i - j, i, j). For an upper texel, with i' = b - 1 - i and j' = b - 1 - j:
 * (a0, a1, a2) = (n - i' - j', i', j'). p = (float) (((a0 * v0 + a1 * v1) + a2 * v2) / n) per component. The integer weights are negative on the texels outside the
 * UV triangle (the gutter): those are the affine continuation of the triangle's plane.
 *   - A corner texel has exactly the vertex's position (a coordinate of -0 comes out as +0).
 *   - The n + 1 texels along an edge have bit-identical positions in both triangles that share it, whatever corner roles the edge has in each: the two-term sum is
 *     commutative and the zero term adds nothing. With them every map is equal there: a closed mesh has no seam at the edge texels.
 *
 * Texel values. The network input is built from p as rnb_extract_mesh builds it from a vertex for the vertex attributes: the position normalised by the scene's box,
 * the direction pointing outward from (0.5, 0.5, 0.5). The normalised position is then clamped to [0, 1] per component: a texel of the gutter, or a vertex handed in,
 * may lie outside the box, where the hash grid has no cells; inside the box the clamp changes nothing. Channels 0-2:
 *   albedo     the logistic of the network's outputs 0 .. 2
 *   normal     outputs 4 .. 6 (the SDF gradient) normalised, zeros for a zero gradient
 *   position   p
 * In every map channel 3 is 1 on a texel of an existing triangle. Every other texel is all zeros: the texels outside the used blocks, and the upper half of the last
 * block when n_tris is odd. The albedo and the normal at a corner texel are bit for bit the colour and the normal rnb_extract_mesh gives that vertex.
 *
 * The same input gives the same bits; neither max_texels_in_flight nor anything else about how the work is cut changes one.
 *
 * How it is done (none of it can change a result). The owned texels are numbered block-major, n_blocks * b * b of them rather than S * S, so that the network batches
 * are dense. Per batch one kernel writes the position and the network input of its texels (a corner texel also the (U, V) of its corner, by the layout's formula),
 * the network runs, and one kernel turns the 16 outputs of a texel into one 16-byte store per map.
 *
 * Failure with RNB_ERR_INVALID, before the device is touched: a null ctx, mesh, opt or out; a wrong version; size, block or maps out of range, maps = 0; a reserved word
 * not 0; n_indices % 3 != 0; a null vertex or index buffer with a non-zero count; indices without vertices; a mesh the layout does not hold. After the range-check
 * kernel: an index >= n_verts. On failure *out and *stats are zeroed, nothing stays allocated and the context stays usable. A mesh without triangles succeeds with
 * all-zero maps.
 *
 * Workspace: the result (16 bytes per texel and map, 24 bytes per triangle), one word per vertex, and 60 bytes per texel of a batch; all but the result released before
 * the call returns. Reads only the weights: the training state is left as it was; work pending on the context's side streams is joined first. Syncs. */
int rnb_mesh_bake_texture(rnb_ctx* ctx, void* stream, const rnb_mesh* mesh, const rnb_mesh_texture_options* opt, rnb_mesh_texture* out, rnb_mesh_texture_stats* stats /* may be NULL */);

/* Releases what rnb_mesh_bake_texture allocated and zeroes *tex. */
int rnb_mesh_texture_free(rnb_ctx* ctx, rnb_mesh_texture* tex);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_TEXTURE_H */
