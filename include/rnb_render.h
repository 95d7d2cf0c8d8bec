/*
 * rnb_render.h — C-ABI of the inference tracer of librnb_neus2_hip: the normal, albedo, opacity and depth maps that a trained
 * model predicts for one camera. It replaces Testbed::render_nerf / NerfTracer::trace (src/testbed_nerf.cu:2499-2770) in their
 * Normals and Depth modes; the GUI around them has no counterpart here.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own:
 * the training ABI (RNB_ABI_VERSION) is not affected by this header.
 */
#ifndef RNB_RENDER_H
#define RNB_RENDER_H

#include "rnb_neus2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_RENDER_ABI_VERSION 1

/* Per pixel, row-major [height][width][RNB_RENDER_CHANNELS] float:
 *   0-2  unit normal in the frame of the views given to rnb_set_dataset (the normalised sum of weight * normalize(grad sdf)); 0 where the opacity is 0
 *   3-5  albedo, not premultiplied (sum of weight * logistic(outputs 0..2) over the sum of weights; ones under apply_no_albedo)
 *   6    opacity: the sum of the NeuS weights, 1 where the ray stopped early (the reference divides by the sum there, testbed_nerf.cu:1100-1103)
 *   7    depth along the camera's forward axis (column 2 of xform) of the max-weight sample, in the scene's units; 0 where the opacity is <= 0.2
 *        (shade_kernel_nerf, testbed_nerf.cu:2278)
 *   8    samples composited (the ray's samples up to and including the one that stopped it) */
#define RNB_RENDER_CHANNELS 9

typedef struct rnb_render_options {
	uint32_t abi_version;          /* RNB_RENDER_ABI_VERSION */
	float    min_transmittance;    /* 0.01 (testbed.h:723): a ray stops once its opacity exceeds 1 - min_transmittance; 0 = composite to the box exit. In [0, 1) */
	float    near_distance;        /* 0.2 (NERF_RENDERING_NEAR_DISTANCE, testbed_nerf.cu:48): a ray starts at max(box entry, near_distance) + 1e-6 */
	uint32_t use_inference_params; /* 1 (default) = the EMA weights (what a snapshot holds), 0 = the training weights */
	uint32_t use_occupancy;        /* 1 (default) = skip the cells the occupancy bitfield marks empty, as training does; 0 = sample every step of the box */
	uint32_t max_rays_in_flight;   /* 0 = default (2^19). Rays are traced in tiles of at most this many pixels (rounded down to a multiple of 64, at least 64); it
	                                  bounds the render workspace to about 700 bytes per ray. The image does not depend on it */
	uint32_t reserved[4];          /* 0 */
} rnb_render_options;

typedef struct rnb_render_stats {
	uint32_t n_rays;     /* width * height */
	uint32_t n_hit;      /* pixels whose opacity exceeds 0.001 (the reference's hit counter, compact_kernel_nerf :2299) */
	uint32_t rounds;     /* march / network / composite rounds over all tiles */
	uint32_t reserved;
	uint64_t n_samples;  /* network samples the marches wrote (samples past an early stop of their ray included) */
	float    ms;         /* wall-clock time of the call */
} rnb_render_stats;

uint32_t rnb_render_abi_version(void);
/* Fills *opt with the defaults above. */
int rnb_render_default_options(rnb_render_options* opt);
/* Testbed::render_nerf + NerfTracer::trace (src/testbed_nerf.cu:2499-2770) in Normals and Depth modes, one camera (rnb_view: pinhole, no distortion), with
 * the context's bounding box, cone angle and occupancy bitfield and the march rules of the training step. Writes view->width * view->height *
 * RNB_RENDER_CHANNELS floats to out_dev (device memory). Reads the network weights and the occupancy bitfield only: the training state (weights, optimizer,
 * occupancy grid, step scratch, ray generator, controller) is left as it was; work pending on the context's side streams is joined first. The workspace is the
 * context's own, grown on demand and never shrunk: it stays allocated after the call (about 700 bytes per ray of the largest tile used so far, e.g.
 * 1.4 GB after a call with max_rays_in_flight = 2^21) until rnb_destroy. One 4-byte device-to-host read per round, a synchronisation at the end. Bit-reproducible: the same
 * state renders the same bits, for any max_rays_in_flight. Syncs. */
int rnb_render(rnb_ctx* ctx, void* stream, const rnb_view* view, const rnb_render_options* opt, float* out_dev, rnb_render_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_RENDER_H */
