/*
 * rnb_mesh_visibility.h — C-ABI of the visibility stage of librnb_neus2_hip: which triangles of an indexed device mesh a set of pinhole cameras sees, counted per
 * triangle over all the views in one call (rnb_mesh_visibility), and the mesh without what they do not see (rnb_mesh_visibility_select). An SDF network leaves cavity
 * shells inside the object, double walls and blobs in space the masks call empty; no camera sees the first two, and the masks speak against the third.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: the training ABI, the render ABI, the
 * mesh ABI and the ABIs of the other mesh stages are not affected by this header. The rules of the mesh rasteriser (rnb_mesh_raster and its header, rules 1-5) are
 * used by number below and are not restated: both calls run the same fill, so what the rasteriser's face map shows for a view is what is counted here.
 */
#ifndef RNB_MESH_VISIBILITY_H
#define RNB_MESH_VISIBILITY_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_VISIBILITY_ABI_VERSION 1

#define RNB_MESH_VISIBILITY_NONE 0xFFFFFFFFu /* best_view of a triangle that never won a pixel (= RNB_MESH_RASTER_NONE) */
#define RNB_MESH_VISIBILITY_MAX_RINGS 64u

#define RNB_MESH_VISIBILITY_UNIT_COMPONENT 0 /* a connected component is kept or dropped whole: closed surfaces stay closed */
#define RNB_MESH_VISIBILITY_UNIT_FACE 1      /* triangle by triangle, grown by `rings` */

typedef struct rnb_mesh_visibility_view {
	rnb_view       view;        /* the camera (pinhole, no distortion), W = view.width, H = view.height, each 1 .. 16384 (RNB_MESH_RASTER_MAX_SIZE) */
	const uint8_t* mask_dev;    /* uint8[mask_height][mask_width] in device memory, or NULL: no mask, every pixel is on it */
	uint32_t       mask_width;  /* any size > 0 when mask_dev is given: the mask need not have the view's resolution */
	uint32_t       mask_height;
} rnb_mesh_visibility_view;

typedef struct rnb_mesh_visibility_options {
	uint32_t abi_version; /* RNB_MESH_VISIBILITY_ABI_VERSION */
	float    near;        /* rule 2 of the rasteriser; > 0 and finite; default 2^-10 */
	uint32_t cull;        /* the rasteriser's RNB_MESH_RASTER_CULL_* (0 none, 1 back, 2 front); default none */
	uint32_t min_pixels;  /* a view sees a triangle that wins at least this many pixels of it; >= 1; default 1 */
	uint32_t reserved[4]; /* 0 */
} rnb_mesh_visibility_options;

typedef struct rnb_mesh_face_visibility { /* 40 bytes, one per triangle, in the mesh's order */
	uint32_t n_drawn;          /* views that draw the triangle */
	uint32_t n_seen;           /* views that see it */
	uint32_t n_off_mask;       /* views in which it lies off the mask */
	uint32_t best_view;        /* the view in which it wins the most pixels, the lowest of equals; RNB_MESH_VISIBILITY_NONE if it never won one */
	uint32_t best_pixels;      /* the pixels it wins there; 0 if never */
	uint32_t reserved;         /* 0 */
	uint64_t n_pixels_won;     /* over all views */
	uint64_t n_pixels_covered; /* over all views */
} rnb_mesh_face_visibility;

typedef struct rnb_mesh_visibility_stats {
	uint32_t n_tris;
	uint32_t n_views;
	uint64_t n_behind;         /* the rasteriser's seven classes, each summed over the views; they add up to n_tris * n_views */
	uint64_t n_out_of_range;
	uint64_t n_degenerate;
	uint64_t n_culled;
	uint64_t n_offscreen;
	uint64_t n_small;
	uint64_t n_large;
	uint64_t n_pixels;         /* the sum of W * H over the views */
	uint32_t n_faces_seen;     /* triangles with n_seen >= 1 */
	uint32_t n_faces_off_mask; /* triangles with n_off_mask >= 1 */
	uint64_t peak_workspace;   /* bytes of device memory the call held at its peak */
	float    ms;               /* wall-clock time of the call */
	uint32_t reserved;
} rnb_mesh_visibility_stats;

typedef struct rnb_mesh_visibility_select_options {
	uint32_t abi_version;        /* RNB_MESH_VISIBILITY_ABI_VERSION */
	uint32_t unit;               /* RNB_MESH_VISIBILITY_UNIT_*; default COMPONENT */
	uint32_t min_views_seen;     /* a seed is seen by at least this many views; default 1 */
	uint32_t max_views_off_mask; /* a candidate lies off the mask in at most this many views; default 0xFFFFFFFF: the masks carve nothing */
	uint32_t rings;              /* UNIT_FACE only: 0 .. RNB_MESH_VISIBILITY_MAX_RINGS; default 1 */
	uint32_t reserved[3];        /* 0 */
} rnb_mesh_visibility_select_options;

typedef struct rnb_mesh_visibility_select_stats {
	uint32_t n_verts_in;
	uint32_t n_verts_out;
	uint32_t n_tris_in;
	uint32_t n_tris_out;
	uint32_t n_seeds;
	uint32_t n_candidates;
	uint32_t n_components;      /* UNIT_COMPONENT: the components of the input (those of the mesh cleaner); UNIT_FACE: 0, they are not formed */
	uint32_t n_components_kept; /* UNIT_COMPONENT: those that hold a seed; UNIT_FACE: 0 */
	uint64_t peak_workspace;    /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;
	uint32_t reserved;
} rnb_mesh_visibility_select_stats;

uint32_t rnb_mesh_visibility_abi_version(void);
/* Fills *opt with the defaults: near 2^-10, no culling, min_pixels 1. */
int rnb_mesh_visibility_default_options(rnb_mesh_visibility_options* opt);
/* Fills *opt with the defaults: UNIT_COMPONENT, min_views_seen 1, max_views_off_mask 0xFFFFFFFF, rings 1. */
int rnb_mesh_visibility_select_default_options(rnb_mesh_visibility_select_options* opt);

/* mesh: an indexed triangle mesh in device memory, not modified. views: n_views records in HOST memory (their masks in device memory). faces_dev: the caller's device
 * buffer of n_indices / 3 records, written whole; what it held before does not matter.
 *
 * Per view v (W x H pixels) and triangle t, rules 1-5 of the mesh rasteriser apply unchanged, with this call's near and cull and the rasteriser's keys: the class of
 * the triangle (rules 2-4), the pixel centres it covers (rule 4), the winner of every pixel (rule 5: the nearest in float depth, the lowest index among equals). All
 * that is counted is integers; there is no tolerance in this header.
 *
 * Mask lookup. Pixel (i, j), column i, row j, of a view with a mask of mw x mh reads mask[mj][mi] with mi = min(mw - 1, ((2 i + 1) * mw) / (2 W)) and
 * mj = min(mh - 1, ((2 j + 1) * mh) / (2 H)) in integer arithmetic (the divisions truncate): the mask pixel whose area holds the pixel's centre, the rule by which the
 * per-view metrics of build/render and build/mesh read the input maps. The pixel is ON THE MASK if the view has no mask or if that byte is not 0.
 *
 * Per view:
 *   drawn(t, v)  the triangle's class is small or large (it passed rules 2-4 and its box holds a pixel centre)
 *   cov(t, v)    the number of pixel centres it covers (rule 4); 0 if not drawn
 *   on(t, v)     those of cov that are on the mask
 *   won(t, v)    the number of pixels that are on the mask and whose winner (rule 5, over ALL covering triangles, on the mask or not) is t
 *   seen(t, v)   won(t, v) >= min_pixels
 *   off(t, v)    the view has a mask, cov(t, v) > 0 and 2 * on(t, v) < cov(t, v): less than half of what it covers is on the mask
 * The record of t: n_drawn, n_seen, n_off_mask, n_pixels_won, n_pixels_covered = the sums over the views of drawn, seen, off, won, cov. best_view = the lowest v with
 * the greatest won(t, v) > 0, best_pixels = that won(t, v); RNB_MESH_VISIBILITY_NONE and 0 if no view has one. reserved = 0.
 *
 * Consequences. The same input gives the same bits. A permutation of the views permutes best_view (between views of equal won the lowest number is named) and changes
 * nothing else. A permutation of the triangles permutes the records; it changes n_seen, n_pixels_won, best_view and best_pixels only through the pixels at which rule 7
 * of the rasteriser lets the winner change (several covering triangles with the winner's float depth), and it never changes n_drawn, n_pixels_covered or n_off_mask.
 * A closed mesh turned outward and seen from outside never shows a cavity: every ray to a cavity wall crosses the outer surface first.
 *
 * stats: n_tris, n_views, the seven class counts summed over the views, n_pixels, n_faces_seen, n_faces_off_mask, peak_workspace, ms.
 *
 * How it is done (none of it can change a result). The workspace is allocated once for the largest view: 12 bytes per pixel (the rasteriser's keys and counts), three
 * words per triangle (cov, on, won), one word per vertex for the range check, the list of the large triangles. Per view: the rasteriser's own fill (the same kernels),
 * in which whoever fills a triangle -- its thread for a small one, its wavefront for a large one -- also writes its cov and on, without atomics; one thread per pixel
 * adds the pixel to its winner's won, the lanes of a wavefront that share a winner with one atomic add; one thread per triangle folds the three words into the record
 * and clears them. One small device-to-host read per view (the class counts and the number of large triangles); syncs.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, mesh, views, opt or faces_dev; n_views == 0; a wrong version; near not finite
 * or <= 0; cull out of range; min_pixels == 0; a reserved word of the options not 0; per view: a focal length not finite or <= 0, a principal point or an entry of
 * xform not finite, width or height 0 or above 16384, a mask pointer with mask_width or mask_height 0; n_indices % 3 != 0; a null vertex or index buffer; indices
 * without vertices. After the range-check kernel: an index >= n_verts. On failure faces_dev holds nothing of use, *stats is zeroed and the context stays usable. A mesh
 * without triangles succeeds (there is no record to write). Coordinates need not be finite. Reads nothing of the training state; work pending on the context's side
 * streams is joined first. */
int rnb_mesh_visibility(rnb_ctx* ctx, void* stream, const rnb_mesh* mesh, const rnb_mesh_visibility_view* views /* host */, uint32_t n_views, const rnb_mesh_visibility_options* opt,
                        rnb_mesh_face_visibility* faces_dev, rnb_mesh_visibility_stats* stats /* may be NULL */);

/* in: the mesh the records were measured on, not modified. faces_dev: its n_indices / 3 records (device). kept_dev: uint32[n_indices / 3] in device memory, 1 for a
 * triangle that is kept and 0 for one that is not, or NULL.
 *
 *   candidate(t) = n_off_mask <= max_views_off_mask
 *   seed(t)      = candidate(t) and n_seen >= min_views_seen
 *
 * UNIT_FACE. marked_0 = the seeds; marked_{r+1} = marked_r and every candidate that shares a vertex index with a triangle of marked_r; kept = marked_rings. rings = 1
 * closes the pinholes a coarse view set leaves in a surface it does see (a triangle too thin to hold a pixel centre in any view sits between seen neighbours). WHAT IT
 * DOES TO A CLOSED SURFACE: a side that no camera saw is not kept -- an object photographed from above comes out without its underside, as an open shell with a
 * boundary, and the inside of a double wall goes while the outside stays. Ask for it when that is what is wanted.
 * UNIT_COMPONENT (the default, because it keeps closed surfaces closed). The connected components are those of the mesh cleaner (rnb_mesh_clean: vertices joined by
 * triangles), formed over ALL triangles, candidates or not. kept = the candidates of every component that holds a seed. With the default max_views_off_mask every
 * triangle is a candidate, and a component is kept whole or dropped whole: a cavity shell goes, a second object any camera saw stays.
 *
 * Output, as the cleaner does it: the vertices a kept triangle uses, in input order; the kept triangles, in input order and with their winding; indices renumbered by
 * prefix sums; colours and normals carried. Deterministic. *out owns its device buffers: release them with rnb_mesh_free. On failure *out is zeroed.
 *
 * stats: vertices and triangles in and out, n_seeds, n_candidates, n_components, n_components_kept, peak_workspace, ms.
 *
 * Failure with RNB_ERR_INVALID, before the context or the device is touched: a null ctx, in, opt or out; in == out; faces_dev null for a mesh with triangles; a wrong
 * version; unit out of range; rings above RNB_MESH_VISIBILITY_MAX_RINGS; a reserved word not 0; n_indices % 3 != 0; a null vertex or index buffer; indices without
 * vertices. After the range-check kernel: an index >= n_verts. The context stays usable. An empty mesh gives an empty mesh. Reads nothing of the training state. */
int rnb_mesh_visibility_select(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_face_visibility* faces_dev, const rnb_mesh_visibility_select_options* opt, rnb_mesh* out,
                               uint32_t* kept_dev /* may be NULL */, rnb_mesh_visibility_select_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_VISIBILITY_H */
