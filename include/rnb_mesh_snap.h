/*
 * rnb_mesh_snap.h — C-ABI of the snapping stage of librnb_neus2_hip: the vertices of an indexed device mesh moved back onto the level set of the trained model's SDF by
 * guarded Newton steps along the SDF gradient (rnb_mesh_snap), with the residual |sdf - level| of every vertex before and after, and colours and normals resampled from
 * the model at the new positions. It brings back what the stages after the extractor moved off the surface: the cell vertices of rnb_mesh_simplify, the flat fans of
 * rnb_mesh_fill_holes, the vertices rnb_mesh_smooth faired. ("snap": the name of putting a mesh back onto a surface is taken here by the stage that maps the input views onto a mesh.) It reads the model and the vertices
 * only; the triangles are carried.
 *
 * Same library and same conventions as rnb_neus2.h (status codes, rnb_last_error, streams as void*), with a version of its own: no other ABI is affected by this header.
 */
#ifndef RNB_MESH_SNAP_H
#define RNB_MESH_SNAP_H

#include "rnb_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RNB_MESH_SNAP_ABI_VERSION 1

#define RNB_MESH_SNAP_MAX_ITERATIONS 64u
#define RNB_MESH_SNAP_MAX_IN_FLIGHT (1u << 22) /* the cap of max_points_in_flight */
#define RNB_MESH_SNAP_RESIDUAL_LOG2 8          /* a residual must be finite and below 2^8 in magnitude, or the vertex is INVALID */
#define RNB_MESH_SNAP_Q_SHIFT 24               /* sum_before_q, sum_after_q: q = (uint64) trunc(|r| * 2^24) */

/* state of a vertex, in the order of the rules below */
#define RNB_MESH_SNAP_UNSELECTED 0u
#define RNB_MESH_SNAP_CONVERGED 1u
#define RNB_MESH_SNAP_UNFINISHED 2u
#define RNB_MESH_SNAP_FLAT 3u
#define RNB_MESH_SNAP_LEASHED 4u
#define RNB_MESH_SNAP_OUTSIDE 5u
#define RNB_MESH_SNAP_STALLED 6u
#define RNB_MESH_SNAP_INVALID 7u
#define RNB_MESH_SNAP_REVERTED 8u

/*
 * The statement.
 *
 * THE NETWORK AT A POSITION. mn and diag are the floats of the scene's box (its lower corner and its edge). The network input of a position v (three floats) is seven
 * floats, every operation in float and rounded on its own (no contraction), expression for expression what the texture baker builds (rnb_mesh_texture.h):
 *   c[k]     = min(max((v[k] - mn) / diag, 0), 1)                      k = 0 .. 2; a NaN becomes 0
 *   c[3]     = 0
 *   d[k]     = v[k] - 0.5,  l = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
 *   c[4 + k] = (d[k] / l + 1) * 0.5
 * and o[0 .. 15] are the sixteen half outputs of rnb_forward_infer for that input (with the EMA weights when use_inference_params = 1). They do not depend on the
 * batch the point is evaluated in.
 *
 * GRADIENT UNITS (read in csrc/kernels_net.cuh, not assumed): outputs 4 .. 6 are the derivative of output 3 with respect to the network's input slots 0 .. 2, that is
 * with respect to the NORMALISED position c: the kernel forms them as the hash-grid encoding's dy/dx, which is taken in c, times the SDF MLP's input gradient, plus the
 * MLP's gradient on the three identity inputs. A Newton step in c is -(r / gg) g; in world units it is that times diag, the factor the step below carries. (With a box
 * edge of 1, which every configuration here has, the factor is 1.)
 *
 * SELECTION. A vertex is SELECTED if select_dev is NULL or its word is not 0. An unselected vertex keeps the input's bits, has state UNSELECTED, residuals and
 * displacement +0, and keeps its input attributes (zeros for an attribute that is asked for and that the input does not have).
 *
 * THE ROUNDS. For a selected vertex P0 is its input position (floats), P = P_prev = P0, a_prev = +infinity, and it is ACTIVE. Rounds k = 1 .. iterations + 1; each
 * evaluates the network at P for every vertex that is still active and then applies, in double precision, every operation rounded on its own, floats and halves widened
 * first:
 *   r = o[3] - level,  g = o[4 .. 6];  in round 1 residual_before = (float) r
 * and the first of these rules that applies decides:
 *    1. INVALID     r or a component of g is not finite, or |r| >= 2^8: P = P_prev; the vertex stops
 *    2. REVERTED    |r| > a_prev: P = P_prev; the vertex stops (the last move made things worse)
 *    3. CONVERGED   |r| <= tolerance: the vertex stops
 *    4. UNFINISHED  k == iterations + 1: the vertex stops
 *    5. FLAT        gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] is below min_gradient * min_gradient: the vertex stops
 *    6. the step    t = r / gg;  d[c] = (t * g[c]) * diag;  L = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);  if L > max_step: d[c] = d[c] * (max_step / L);
 *                   Q[c] = (float)(P[c] - d[c])
 *    7. LEASHED     e[c] = Q[c] - P0[c] and sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) > max_displacement: the vertex stops, P stays
 *    8. OUTSIDE     (Q[c] - mn) / diag, in float as above without the clamp, is below 0 or above 1 for some c: the vertex stops, P stays
 *    9. STALLED     Q equals P bit for bit: the vertex stops
 *   10. otherwise   P_prev = P, a_prev = |r|, P = Q; the vertex stays active
 * The rounds end early when no vertex is active (stats->rounds counts those that evaluated something).
 *
 * THE OUTPUTS. Every selected vertex is then evaluated once more at its final P: residual_after = (float) r of that evaluation; out->verts = P; the colours asked for
 * are 1 / (1 + expf(-o[k])) of outputs 0 .. 2 in float and the normals asked for g / sqrt(g[0] * g[0] + (g[1] * g[1] + g[2] * g[2])) in float, zeros where that root
 * is 0 (the arithmetic of rnb_extract_mesh's vertex attributes); displacement = (float) sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) of e = P - P0 in double, as in
 * rnb_mesh_smooth.
 *
 * CONSEQUENCES.
 *   - For every selected vertex that is not INVALID, |residual_after| <= |residual_before|: every accepted position was checked against the one before it, and a
 *     position that was worse is given up for the one before.
 *   - A vertex that does not move and lies in the box gets bit for bit the colour and the normal rnb_extract_mesh gives it.
 *   - With iterations = 0 the call is a census of the residuals (every selected vertex is CONVERGED, UNFINISHED or INVALID), and it refreshes the attributes if asked.
 *   - Nothing depends on max_points_in_flight, on how the active vertices are packed, or on the order of the vertices: a vertex is computed from its own data alone.
 */

typedef struct rnb_mesh_snap_options {
	uint32_t abi_version;          /* RNB_MESH_SNAP_ABI_VERSION */
	uint32_t iterations;           /* 0 .. RNB_MESH_SNAP_MAX_ITERATIONS; default 3 */
	float    level;                /* finite; default 0, the extractor's thresh */
	float    tolerance;            /* finite, >= 0; default 2^-13: two steps of the spacing the half SDF output has near the surface (profiles/mesh_snap.md) */
	float    max_step;             /* finite, > 0, world units; default 1 / 128 (the box edge / 128 of the unit box) */
	float    max_displacement;     /* finite, >= 0, world units; default 1 / 64 */
	float    min_gradient;         /* finite, > 0; default 0.25 */
	uint32_t attributes;           /* RNB_MESH_ATTR_* bits to resample from the model; default 0: the input's attributes are carried */
	uint32_t use_inference_params; /* 0 or 1; default 1: the EMA weights */
	uint32_t max_points_in_flight; /* points per network launch: 0 = 2^20, capped at RNB_MESH_SNAP_MAX_IN_FLIGHT. Bounds the workspace, changes no bit of the result */
	uint32_t reserved[4];          /* 0 */
} rnb_mesh_snap_options;

typedef struct rnb_mesh_snap_stats {
	uint32_t n_selected;
	uint32_t n_unselected;  /* vertices by state; the nine add up to n_verts */
	uint32_t n_converged;
	uint32_t n_unfinished;
	uint32_t n_flat;
	uint32_t n_leashed;
	uint32_t n_outside;
	uint32_t n_stalled;
	uint32_t n_invalid;
	uint32_t n_reverted;
	uint32_t n_moved;       /* vertices whose output position differs from the input's in a bit */
	uint32_t rounds;        /* rounds that evaluated at least one vertex */
	double   max_displacement; /* the largest displacement value */
	double   max_before;    /* the largest |r| of round 1 and of the final evaluation over the selected vertices that are not INVALID, in double */
	double   max_after;
	uint64_t sum_before_q;  /* the sums of (uint64) trunc(|r| * 2^24) over the same vertices: integers, so they do not depend on the order */
	uint64_t sum_after_q;
	uint64_t n_network_points; /* points handed to the network, the final evaluation included: an honest count, not part of the statement */
	uint64_t peak_workspace;   /* bytes of device memory the call held at its peak, the returned mesh included */
	float    ms;               /* wall-clock time of the call */
	float    ms_network;       /* of that, the network launches */
} rnb_mesh_snap_stats;

uint32_t rnb_mesh_snap_abi_version(void);
/* Fills *opt with the defaults: iterations = 3, level = 0, tolerance = 2^-13, max_step = 1 / 128, max_displacement = 1 / 64, min_gradient = 0.25, attributes = 0,
 * use_inference_params = 1, max_points_in_flight = 0. (profiles/mesh_snap.md records the table they were chosen from.) */
int rnb_mesh_snap_default_options(rnb_mesh_snap_options* opt);

/* The snap. in: any indexed triangle mesh in device memory; it is not modified and must not be *out. select_dev: NULL, or n_verts words of device memory.
 *
 * Output mesh: all input vertices in input order, all triangles unchanged and in input order (they are never read otherwise). out->colors is set when the input has
 * colours or RNB_MESH_ATTR_COLORS is asked for, out->normals likewise. Per vertex (each array optional, caller-allocated device memory of n_verts words):
 * residual_before_dev, residual_after_dev, state_dev (RNB_MESH_SNAP_*), displacement_dev, as defined above.
 *
 * Fails with RNB_ERR_INVALID on a null argument, a wrong version, an option outside its range, a reserved word that is not 0, n_indices % 3 != 0 and an index
 * >= n_verts (range-checked by a kernel before anything else). A mesh without vertices succeeds with a copy. On success *out owns its device buffers: release them with
 * rnb_mesh_free. On failure *out is zeroed. Every argument is validated before the context or the device is touched. Workspace (released before the call returns): the
 * output; 44 bytes per vertex (the previous position, two doubles, the state and three words of the packing) and the block sums of one scan; 60 bytes per point in
 * flight (seven floats in, sixteen halves out). Work pending on the context's side streams is joined first; reads nothing of the training state but the weights. Per
 * round one scan, whose total is the one device-to-host read, and three launches per batch; syncs. */
int rnb_mesh_snap(rnb_ctx* ctx, void* stream, const rnb_mesh* in, const rnb_mesh_snap_options* opt, const uint32_t* select_dev /* may be NULL: every vertex */,
                  rnb_mesh* out, float* residual_before_dev /* may be NULL */, float* residual_after_dev /* may be NULL */, uint32_t* state_dev /* may be NULL */,
                  float* displacement_dev /* may be NULL */, rnb_mesh_snap_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* RNB_MESH_SNAP_H */
