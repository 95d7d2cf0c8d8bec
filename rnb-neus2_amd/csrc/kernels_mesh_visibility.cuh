// kernels_mesh_visibility.cuh — the visibility stage of include/rnb_mesh_visibility.h: per-triangle counts of what a set of cameras sees (rnb_mesh_visibility) and the
// mesh without what they do not (rnb_mesh_visibility_select).
// The fill of every view is the rasteriser's own (k_mr_bin<.., true>, k_mr_fill_large<true> of kernels_mesh_raster.cuh: keys, counts, and per drawn triangle its covered
// and on-mask pixel counts); the components are the cleaner's (k_cl_init, k_cl_hook, k_cl_flatten of kernels_mesh_clean.cuh). Here:
//   k_mv_tally          one thread per pixel instead of k_mr_resolve: a pixel on the mask goes to its winner's `won`; neighbouring pixels share winners, so the lanes of
//                       a wavefront are grouped by face (wave_group_next) and a group issues one atomic add
//   k_mv_fold           one thread per triangle, once per view: cov, on, won into the record (the first view writes it whole), the three words cleared for the next view;
//                       the last view also counts the faces seen and off the mask
//   k_mv_flags          candidate / seed bits per triangle from the records
//   k_mv_ring_mark, k_mv_ring_grow    UNIT_FACE, one ring: the corners of the marked triangles are marked; a candidate with a marked corner joins. Every writer writes 1
//   k_mv_comp_seed, k_mv_comp_keep, k_mv_comp_count    UNIT_COMPONENT: the root of a seed's component is marked; the candidates of marked roots are kept; roots counted
//   k_mv_vflag, MvKeep                                 the corners of the kept triangles flagged; the predicate of the shared compaction (k_compact_verts, k_compact_tris<WRITE>
//                                                      of mesh_common.cuh), keyed by the kept flag of a triangle where the cleaner's is keyed by that of a component
// Integers only: sums, maxima with a fixed order of the views, prefix sums. Nothing depends on the schedule. Vector loads, stores and atomics only.
#pragma once
#include "kernels_mesh_raster.cuh"
#include "kernels_mesh_clean.cuh"
#include "../../include/rnb_mesh_visibility.h"

namespace rnb {

constexpr uint32_t MV_CANDIDATE = 1u, MV_SEED = 2u, MV_KEPT = 4u; // bits of a triangle's flag word

struct MvResult { // written by the kernels, read by the driver
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_faces_seen, n_faces_off_mask;
	uint32_t n_seeds, n_candidates, n_components, n_components_kept;
	uint32_t pad;
};

// one atomic per wavefront for a count of lanes
__device__ __forceinline__ void mv_count(uint32_t* dst, const bool mine) {
	const uint64_t m = __ballot(mine);
	if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((unsigned long long)m) - 1)) (void)atomicAdd(dst, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(MESH_WG) void k_mv_tally(const uint32_t w, const uint32_t h, const uint32_t nt, const MrTally y, const unsigned long long* __restrict__ keys, uint32_t* __restrict__ won) {
	const uint32_t n_pix = w * h, p = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t face = MESH_NONE;
	bool valid = false;
	if (p < n_pix) {
		const unsigned long long key = keys[p];
		face = (uint32_t)key;
		valid = key != ~0ull && face < nt && mr_on_mask(y, w, h, p % w, p / w); // (face < nt always: the key was written by that triangle)
	}
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(face, valid, g)) break;
		if ((int)(threadIdx.x & 63u) == g.leader) (void)atomicAdd(&won[g.key], (uint32_t)__popcll(g.mask));
	}
	if (valid) (void)atomicAdd(&won[face], 1u);
}

__global__ __launch_bounds__(MESH_WG) void k_mv_fold(const uint32_t nt, const uint32_t v, const uint32_t first, const uint32_t last, const uint32_t has_mask, const uint32_t min_pixels,
                                                  uint32_t* __restrict__ cov, uint32_t* __restrict__ on, uint32_t* __restrict__ won, rnb_mesh_face_visibility* __restrict__ faces,
                                                  MvResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	bool seen_ever = false, off_ever = false;
	if (t < nt) {
		const uint32_t cw = cov[t], c = cw & ~MR_DRAWN, o = on[t], wn = won[t];
		cov[t] = 0u; on[t] = 0u; won[t] = 0u;
		rnb_mesh_face_visibility r;
		if (first) {
			r.n_drawn = r.n_seen = r.n_off_mask = 0u;
			r.best_view = RNB_MESH_VISIBILITY_NONE;
			r.best_pixels = 0u; r.reserved = 0u;
			r.n_pixels_won = r.n_pixels_covered = 0ull;
		} else r = faces[t];
		r.n_drawn += (cw & MR_DRAWN) ? 1u : 0u;
		r.n_seen += wn >= min_pixels ? 1u : 0u;
		r.n_off_mask += (has_mask && c > 0u && 2ull * o < (unsigned long long)c) ? 1u : 0u;
		if (wn > r.best_pixels) { r.best_pixels = wn; r.best_view = v; } // the views come in ascending order: the lowest of equals stays
		r.n_pixels_won += wn;
		r.n_pixels_covered += c;
		faces[t] = r;
		seen_ever = r.n_seen >= 1u; off_ever = r.n_off_mask >= 1u;
	}
	if (last) { // (uniform over the launch)
		mv_count(&res->n_faces_seen, seen_ever);
		mv_count(&res->n_faces_off_mask, off_ever);
	}
}

// ---- rnb_mesh_visibility_select ----
__global__ __launch_bounds__(MESH_WG) void k_mv_flags(const rnb_mesh_face_visibility* __restrict__ faces, const uint32_t nt, const uint32_t min_views_seen, const uint32_t max_views_off_mask,
                                                   uint32_t* __restrict__ flag, MvResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	bool cand = false, seed = false;
	if (t < nt) {
		cand = faces[t].n_off_mask <= max_views_off_mask;
		seed = cand && faces[t].n_seen >= min_views_seen;
		flag[t] = (cand ? MV_CANDIDATE : 0u) | (seed ? MV_SEED : 0u);
	}
	mv_count(&res->n_candidates, cand);
	mv_count(&res->n_seeds, seed);
}
// kept <- the seeds (UNIT_FACE, ring 0)
__global__ __launch_bounds__(MESH_WG) void k_mv_seeds_kept(uint32_t* __restrict__ flag, const uint32_t nt) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t < nt && (flag[t] & MV_SEED)) flag[t] |= MV_KEPT;
}
__global__ __launch_bounds__(MESH_WG) void k_mv_ring_mark(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ flag, uint32_t* __restrict__ vmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt || !(flag[t] & MV_KEPT)) return;
	vmark[idx[3 * (size_t)t]] = 1u; vmark[idx[3 * (size_t)t + 1]] = 1u; vmark[idx[3 * (size_t)t + 2]] = 1u;
}
__global__ __launch_bounds__(MESH_WG) void k_mv_ring_grow(const uint32_t* __restrict__ idx, const uint32_t nt, uint32_t* __restrict__ flag, const uint32_t* __restrict__ vmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt) return;
	const uint32_t f = flag[t];
	if (!(f & MV_CANDIDATE) || (f & MV_KEPT)) return;
	if (vmark[idx[3 * (size_t)t]] | vmark[idx[3 * (size_t)t + 1]] | vmark[idx[3 * (size_t)t + 2]]) flag[t] = f | MV_KEPT; // (a thread writes its own word only)
}
// parent: the root of every vertex (k_cl_flatten). rmark[root] <- 1 for the component of a seed.
__global__ __launch_bounds__(MESH_WG) void k_mv_comp_seed(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ parent, uint32_t* __restrict__ rmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t < nt && (flag[t] & MV_SEED)) rmark[parent[idx[3 * (size_t)t]]] = 1u;
}
__global__ __launch_bounds__(MESH_WG) void k_mv_comp_keep(const uint32_t* __restrict__ idx, const uint32_t nt, uint32_t* __restrict__ flag, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt) return;
	const uint32_t f = flag[t];
	if ((f & MV_CANDIDATE) && rmark[parent[idx[3 * (size_t)t]]]) flag[t] = f | MV_KEPT;
}
__global__ __launch_bounds__(MESH_WG) void k_mv_comp_count(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ used, const uint32_t* __restrict__ rmark, const uint32_t nv, MvResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	const bool root = v < nv && used[v] && parent[v] == v;
	mv_count(&res->n_components, root);
	mv_count(&res->n_components_kept, root && rmark[v]);
}
// vkeep[v] <- 1 for the corners of the kept triangles (zero on entry); kept_out (or null) <- 1 / 0 per triangle
__global__ __launch_bounds__(MESH_WG) void k_mv_vflag(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ flag, uint32_t* __restrict__ vkeep, uint32_t* __restrict__ kept_out) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt) return;
	const bool kept = (flag[t] & MV_KEPT) != 0;
	if (kept_out) kept_out[t] = kept ? 1u : 0u;
	if (!kept) return;
	vkeep[idx[3 * (size_t)t]] = 1u; vkeep[idx[3 * (size_t)t + 1]] = 1u; vkeep[idx[3 * (size_t)t + 2]] = 1u;
}
// What MeshCall::compact keeps of the input of rnb_mesh_visibility_select (k_compact_verts, k_compact_tris of mesh_common.cuh): the kept triangles and their corners.
struct MvKeep {
	const uint32_t* flag;  // MV_KEPT per triangle
	const uint32_t* vkeep; // 1 per corner of a kept triangle (k_mv_vflag)
	__device__ __forceinline__ bool vertex(const uint32_t v) const { return vkeep[v] != 0u; }
	__device__ __forceinline__ uint32_t triangle(const uint32_t*, const uint32_t t) const { return (flag[t] & MV_KEPT) ? 1u : 0u; }
};

} // namespace rnb
