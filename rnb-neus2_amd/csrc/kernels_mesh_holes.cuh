// kernels_mesh_holes.cuh — the hole stage of include/rnb_mesh_holes.h (rnb_mesh_boundary_loops, rnb_mesh_fill_holes): the boundary half-edges as ordered loops, their
// sums, the triangles and vertices that close them. The faces per half-edge come from the topology stage's edge join (k_tp_edges, which also unites the boundary
// components over the vertices); everything here works on the compacted list of the nb boundary half-edges ("items", ascending half-edge).
//   k_hl_flag, k_hl_list        boundary half-edges flagged for the exclusive sum that numbers them; the list written
//   k_hl_vertex                 per item: out-count and in-count of its ends, the outgoing half-edge of its start (integer minimum), the component's label (minimum)
//   k_hl_label_flags, k_hl_loops, k_hl_vertices, k_hl_classify   labels -> loop ids by an exclusive sum (ascending label = table order); n_edges, n_irregular, label,
//                               component, simple; the statistics
//   k_hl_rank_init, k_hl_rank_round, k_hl_pos   list ranking by pointer jumping towards the label's item: (next, distance) pairs, one launch per round from one buffer
//                               into the other (in place it would race), the number of rounds fixed by the host; the distance becomes the position
//   k_hl_sums, k_hl_finish      the per-component sums in 64-bit fixed point (the lanes of a wavefront that hit one loop summed first); centroid, normal, perimeter, area
//   k_hl_write                  the per-half-edge arrays of the census
//   k_hl_largest, k_hl_select   skip_largest's 64-bit maximum per connected component; who is filled, what each loop appends
//   k_hl_emit_tris, k_hl_emit_verts   one thread per item writes its triangle at the loop's offset + its position; one per loop its vertex
// Nothing depends on the hash, the bucket count or the order of the atomics: only counts, minima, maxima and integer sums are formed. No kernel loops on device data
// until something converges. Vector loads, stores and atomics only; no LDS.
#pragma once
#include "kernels_mesh_topology.cuh"
#include "../../include/rnb_mesh_holes.h"

namespace rnb {

constexpr uint32_t HL_NOT_FINITE = 2u, HL_BAD_TERM = 4u; // bits of HlResult::flags
constexpr int HL_NSUM = 10;                              // sums per loop: a - o (3), |b - a|, cross (3), colour (3)

struct HlResult { // written by the kernels, read by the driver; zeroed before a call
	uint32_t flags;
	uint32_t n_simple, n_irregular_vertices, max_loop_edges, max_simple_edges, n_too_long;
	uint32_t n_filled, n_not_simple, n_over_max, n_largest;
};

static_assert(sizeof(rnb_mesh_boundary_loop) == 64 && offsetof(rnb_mesh_boundary_loop, n_edges) == 4 && offsetof(rnb_mesh_boundary_loop, n_irregular) == 12,
              "tp_add addresses the records of the loop table as sixteen words");
constexpr uint32_t HL_REC = sizeof(rnb_mesh_boundary_loop) / 4u;

// the ends of half-edge h = 3t + k: from corner k to corner (k + 1) % 3
__device__ __forceinline__ void hl_ends(const uint32_t* __restrict__ idx, const uint32_t h, uint32_t& a, uint32_t& b) {
	const uint32_t t = h / 3u, k = h - 3u * t;
	a = idx[h];
	b = idx[3 * (size_t)t + (k == 2u ? 0u : k + 1u)];
}
__device__ __forceinline__ uint32_t hl_wave_max(uint32_t m) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off, 64));
	return m;
}

// ---- the items ----
__global__ __launch_bounds__(MESH_WG) void k_hl_flag(const uint32_t* __restrict__ n_faces, const uint32_t n_half, uint32_t* __restrict__ bidx) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	if (h < n_half) bidx[h] = n_faces[h] == 1u ? 1u : 0u;
}
// bidx: the exclusive sums of k_hl_flag's flags = the item of a boundary half-edge
__global__ __launch_bounds__(MESH_WG) void k_hl_list(const uint32_t* __restrict__ n_faces, const uint32_t* __restrict__ bidx, const uint32_t n_half, uint32_t* __restrict__ list) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	if (h < n_half && n_faces[h] == 1u) list[bidx[h]] = h;
}
// outc / inc: zero on entry; outh / lab: MESH_NONE on entry. root: the boundary components' flattened parents (k_tp_edges, k_cl_flatten); lab is indexed by the root.
__global__ __launch_bounds__(MESH_WG) void k_hl_vertex(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, const uint32_t nb, const uint32_t* __restrict__ root,
                                                    uint32_t* __restrict__ outc, uint32_t* __restrict__ inc, uint32_t* __restrict__ outh, uint32_t* __restrict__ lab) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= nb) return;
	const uint32_t h = list[i];
	uint32_t a, b;
	hl_ends(idx, h, a, b);
	(void)atomicAdd(outc + a, 1u);
	(void)atomicAdd(inc + b, 1u);
	(void)atomicMin(outh + a, h);
	(void)atomicMin(lab + root[a], h);
}

// ---- the loops ----
// isl[item of a label] = 1 (isl: nb words, zero on entry); its exclusive sums number the loops in ascending label
__global__ __launch_bounds__(MESH_WG) void k_hl_label_flags(const uint32_t* __restrict__ root, const uint32_t* __restrict__ bmark, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ bidx,
                                                         const uint32_t nv, uint32_t* __restrict__ isl) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv && bmark[v] && root[v] == v) isl[bidx[lab[v]]] = 1u;
}
// the loop of a boundary vertex
__device__ __forceinline__ uint32_t hl_loop_of(const uint32_t v, const uint32_t* __restrict__ root, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ bidx, const uint32_t* __restrict__ lrank) {
	return lrank[bidx[lab[root[v]]]];
}
__global__ __launch_bounds__(MESH_WG) void k_hl_loops(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, const uint32_t nb, const uint32_t* __restrict__ root,
                                                   const uint32_t* __restrict__ lab, const uint32_t* __restrict__ bidx, const uint32_t* __restrict__ lrank, uint32_t* __restrict__ iloop,
                                                   rnb_mesh_boundary_loop* __restrict__ table) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	const bool valid = i < nb;
	uint32_t l = MESH_NONE;
	if (valid) {
		l = hl_loop_of(idx[list[i]], root, lab, bidx, lrank);
		iloop[i] = l;
	}
	tp_add((uint32_t*)table, HL_REC, l, valid, 0u, 1u, 0u, 0u); // words 0 .. 3: label, n_edges, simple, n_irregular
}
// one thread per vertex: an irregular one is counted into its loop; the root writes the loop's label and connected component (comp: the cleaner's flattened parents)
__global__ __launch_bounds__(MESH_WG) void k_hl_vertices(const uint32_t* __restrict__ root, const uint32_t* __restrict__ bmark, const uint32_t* __restrict__ outc, const uint32_t* __restrict__ inc,
                                                      const uint32_t* __restrict__ lab, const uint32_t* __restrict__ bidx, const uint32_t* __restrict__ lrank, const uint32_t* __restrict__ comp,
                                                      const uint32_t nv, rnb_mesh_boundary_loop* __restrict__ table) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	const bool on = v < nv && bmark[v];
	uint32_t l = MESH_NONE;
	bool irregular = false;
	if (on) {
		l = hl_loop_of(v, root, lab, bidx, lrank);
		irregular = outc[v] != 1u || inc[v] != 1u;
		if (root[v] == v) { table[l].label = lab[v]; table[l].component = comp[v]; } // (tp_add issues no atomic for a zero addend: nobody else writes these words)
	}
	tp_add((uint32_t*)table, HL_REC, l, irregular, 0u, 0u, 0u, 1u);
}
__global__ __launch_bounds__(MESH_WG) void k_hl_classify(rnb_mesh_boundary_loop* __restrict__ table, const uint32_t n_loops, HlResult* __restrict__ res) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	const bool valid = i < n_loops;
	const uint32_t n = valid ? table[i].n_edges : 0u, irr = valid ? table[i].n_irregular : 0u;
	const bool simple = valid && irr == 0u;
	if (valid) table[i].simple = simple ? 1u : 0u;
	tp_count(&res->n_simple, simple ? 1u : 0u);
	tp_count(&res->n_irregular_vertices, irr);
	tp_count(&res->n_too_long, n > RNB_MESH_HOLES_MAX_EDGES ? 1u : 0u);
	const uint32_t m = hl_wave_max(n), ms = hl_wave_max(simple ? n : 0u);
	if ((threadIdx.x & 63u) == 0u) {
		if (m) (void)atomicMax(&res->max_loop_edges, m);
		if (ms) (void)atomicMax(&res->max_simple_edges, ms);
	}
}

// ---- list ranking ----
// x: the item reached, y: the steps taken to it. The label's item and every item of a non-simple component stand still at distance 0.
__global__ __launch_bounds__(MESH_WG) void k_hl_rank_init(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, const uint32_t nb, const uint32_t* __restrict__ iloop,
                                                       const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t* __restrict__ outh, const uint32_t* __restrict__ bidx, uint2* __restrict__ cur) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= nb) return;
	const uint32_t h = list[i], l = iloop[i];
	uint2 r = make_uint2(i, 0u);
	if (table[l].simple && table[l].label != h) {
		uint32_t a, b;
		hl_ends(idx, h, a, b);
		r = make_uint2(bidx[outh[b]], 1u); // b is regular: exactly one boundary half-edge starts there
	}
	cur[i] = r;
}
__global__ __launch_bounds__(MESH_WG) void k_hl_rank_round(const uint2* __restrict__ cur, uint2* __restrict__ nxt, const uint32_t nb) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= nb) return;
	const uint2 a = cur[i], b = cur[a.x];
	nxt[i] = make_uint2(b.x, a.y + b.y);
}
// d steps before the label = position n - d
__global__ __launch_bounds__(MESH_WG) void k_hl_pos(const uint2* __restrict__ cur, const uint32_t* __restrict__ iloop, const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t nb,
                                                 uint32_t* __restrict__ ipos) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= nb) return;
	const uint32_t l = iloop[i], d = cur[i].y;
	ipos[i] = table[l].simple ? (d ? table[l].n_edges - d : 0u) : MESH_NONE;
}

// ---- the sums ----
// fixed point of one term; false: not finite or not below the bound
__device__ __forceinline__ bool hl_q(const double term, long long* q) {
	const double lim = (double)(1ll << RNB_MESH_HOLES_Q_TERM_LOG2), scale = (double)(1ll << RNB_MESH_HOLES_Q_SHIFT);
	if (!(fabs(term) < lim)) { *q = 0; return false; } // also catches NaN and infinity
	*q = (long long)(term * scale);                    // a power of two: exact; the conversion truncates
	return true;
}
__device__ __forceinline__ double hl_unq(const long long q) { return (double)q * (1.0 / (double)(1ll << RNB_MESH_HOLES_Q_SHIFT)); } // int64 -> double rounds to nearest even
// Adds v[0..N) of every valid lane to sums[l * HL_NSUM + first ..] (the simplifier's sp_accumulate). Called by whole wavefronts.
template <int N>
__device__ __forceinline__ void hl_accumulate(long long* __restrict__ sums, const uint32_t first, const uint32_t l, bool valid, const long long (&v)[N]) {
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(l, valid, g)) return;
		long long out = 0;
#pragma unroll
		for (int k = 0; k < N; ++k) {
			const long long s = wave_sum(g.mine ? v[k] : 0ll);
			if ((int)lane == k) out = s;
		}
		if ((int)lane < N && out) (void)atomicAdd((unsigned long long*)(sums + (size_t)g.key * HL_NSUM + first + lane), (unsigned long long)out);
	}
	if (valid) {
#pragma unroll
		for (int k = 0; k < N; ++k)
			if (v[k]) (void)atomicAdd((unsigned long long*)(sums + (size_t)l * HL_NSUM + first + k), (unsigned long long)v[k]);
	}
}
__device__ __forceinline__ bool hl_load3(const float* __restrict__ p, const uint32_t v, double (&x)[3]) {
	const float f0 = p[3 * (size_t)v], f1 = p[3 * (size_t)v + 1], f2 = p[3 * (size_t)v + 2];
	x[0] = (double)f0; x[1] = (double)f1; x[2] = (double)f2;
	return isfinite(f0) && isfinite(f1) && isfinite(f2);
}
// The terms of include/rnb_mesh_holes.h, operation for operation what tests/mesh_holes_reference.py computes (this file is compiled with -ffp-contract=off; the pragma
// says so once more where it matters). A component that is too long is checked and not summed.
__global__ __launch_bounds__(MESH_WG) void k_hl_sums(const uint32_t* __restrict__ idx, const float* __restrict__ verts, const float* __restrict__ colors, const uint32_t* __restrict__ list,
                                                  const uint32_t nb, const uint32_t* __restrict__ iloop, const rnb_mesh_boundary_loop* __restrict__ table, long long* __restrict__ sums,
                                                  HlResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	const bool valid = i < nb;
	uint32_t l = MESH_NONE;
	bool summed = false;
	long long q[7] = {0, 0, 0, 0, 0, 0, 0}, qc[3] = {0, 0, 0};
	if (valid) {
		l = iloop[i];
		summed = table[l].n_edges <= RNB_MESH_HOLES_MAX_EDGES;
		uint32_t ia, ib;
		hl_ends(idx, list[i], ia, ib);
		double a[3], b[3], o[3];
		const bool finite = hl_load3(verts, ia, a) & hl_load3(verts, ib, b) & hl_load3(verts, idx[table[l].label], o);
		const double u[3] = {b[0] - o[0], b[1] - o[1], b[2] - o[2]}, v[3] = {a[0] - o[0], a[1] - o[1], a[2] - o[2]}, d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
		bool ok = hl_q(v[0], &q[0]) & hl_q(v[1], &q[1]) & hl_q(v[2], &q[2]);
		ok &= hl_q(__dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), &q[3]);
		ok &= hl_q(u[1] * v[2] - u[2] * v[1], &q[4]) & hl_q(u[2] * v[0] - u[0] * v[2], &q[5]) & hl_q(u[0] * v[1] - u[1] * v[0], &q[6]);
		if (colors) {
			double c[3];
			(void)hl_load3(colors, ia, c);
			ok &= hl_q(c[0], &qc[0]) & hl_q(c[1], &qc[1]) & hl_q(c[2], &qc[2]);
		}
		if (!finite) (void)atomicOr(&res->flags, HL_NOT_FINITE);
		else if (!ok) (void)atomicOr(&res->flags, HL_BAD_TERM);
	}
	hl_accumulate<7>(sums, 0u, l, summed, q);
	if (colors) hl_accumulate<3>(sums, 7u, l, summed, qc);
}
__global__ __launch_bounds__(MESH_WG) void k_hl_finish(const uint32_t* __restrict__ idx, const float* __restrict__ verts, rnb_mesh_boundary_loop* __restrict__ table, const long long* __restrict__ sums,
                                                    const uint32_t n_loops) {
#pragma clang fp contract(off)
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= n_loops) return;
	const uint32_t n_edges = table[i].n_edges;
	if (n_edges > RNB_MESH_HOLES_MAX_EDGES) return; // too long: the record's derived values stay 0
	const long long* __restrict__ s = sums + (size_t)i * HL_NSUM;
	const double n = (double)n_edges;
	double o[3];
	(void)hl_load3(verts, idx[table[i].label], o);
	const double A[3] = {hl_unq(s[4]), hl_unq(s[5]), hl_unq(s[6])};
	const double len = __dsqrt_rn((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2]);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		table[i].centroid[k] = (float)(hl_unq(s[k]) / n + o[k]);
		table[i].normal[k] = len == 0.0 ? 0.0f : (float)(A[k] / len);
	}
	table[i].perimeter = hl_unq(s[3]);
	table[i].area = 0.5 * len;
}

// ---- the census' arrays (each may be null) ----
__global__ __launch_bounds__(MESH_WG) void k_hl_write(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ n_faces, const uint32_t* __restrict__ bidx, const uint32_t* __restrict__ iloop,
                                                   const uint32_t* __restrict__ ipos, const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t* __restrict__ outh, const uint32_t n_half,
                                                   uint32_t* __restrict__ loop_out, uint32_t* __restrict__ next_out, uint32_t* __restrict__ pos_out) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	if (h >= n_half) return;
	uint32_t label = MESH_NONE, next = MESH_NONE, pos = MESH_NONE;
	if (n_faces[h] == 1u) {
		const uint32_t i = bidx[h];
		label = table[iloop[i]].label;
		pos = ipos[i];
		if (pos != MESH_NONE) {
			uint32_t a, b;
			hl_ends(idx, h, a, b);
			next = outh[b];
		}
	}
	if (loop_out) loop_out[h] = label;
	if (next_out) next_out[h] = next;
	if (pos_out) pos_out[h] = pos;
}

// ---- the fill ----
__device__ __forceinline__ unsigned long long hl_size_key(const rnb_mesh_boundary_loop& r) { return ((unsigned long long)r.n_edges << 32) | (unsigned long long)(~r.label); }
// big[connected component] (one 64-bit word per vertex, zero on entry) = the greatest (n_edges, ~label) of its simple loops
__global__ __launch_bounds__(MESH_WG) void k_hl_largest(const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t n_loops, unsigned long long* __restrict__ big) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= n_loops) return;
	const rnb_mesh_boundary_loop r = table[i];
	if (r.simple) (void)atomicMax(big + r.component, hl_size_key(r));
}
// fill[l]: whether loop l is filled; vadd / tadd: the vertices and triangles it appends (their exclusive sums are the loops' offsets)
__global__ __launch_bounds__(MESH_WG) void k_hl_select(const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t n_loops, const unsigned long long* __restrict__ big, const uint32_t limit,
                                                    uint32_t* __restrict__ fill, uint32_t* __restrict__ vadd, uint32_t* __restrict__ tadd, HlResult* __restrict__ res) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t why = 4u; // 0 filled, 1 not simple, 2 over the limit, 3 the largest of its component, 4 no loop
	if (i < n_loops) {
		const rnb_mesh_boundary_loop r = table[i];
		why = !r.simple ? 1u : (r.n_edges > limit ? 2u : ((big && big[r.component] == hl_size_key(r)) ? 3u : 0u));
		fill[i] = why == 0u ? 1u : 0u;
		vadd[i] = (why == 0u && r.n_edges > 3u) ? 1u : 0u;
		tadd[i] = why == 0u ? (r.n_edges == 3u ? 1u : r.n_edges) : 0u;
	}
	tp_count(&res->n_filled, why == 0u ? 1u : 0u);
	tp_count(&res->n_not_simple, why == 1u ? 1u : 0u);
	tp_count(&res->n_over_max, why == 2u ? 1u : 0u);
	tp_count(&res->n_largest, why == 3u ? 1u : 0u);
}
// One thread per item of a filled loop: triangle nt + toff[l] + pos = (b, a, c), c the loop's new vertex nv + voff[l]; a loop of 3 edges gets the one triangle
// (b_0, a_0, a_2) from its item at position 0 (a_2 = where the half-edge from b_0 ends). loop_of_tri: may be null.
__global__ __launch_bounds__(MESH_WG) void k_hl_emit_tris(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ list, const uint32_t nb, const uint32_t* __restrict__ iloop,
                                                       const uint32_t* __restrict__ ipos, const rnb_mesh_boundary_loop* __restrict__ table, const uint32_t* __restrict__ fill,
                                                       const uint32_t* __restrict__ voff, const uint32_t* __restrict__ toff, const uint32_t* __restrict__ outh, const uint32_t nv, const uint32_t nt,
                                                       uint32_t* __restrict__ oidx, uint32_t* __restrict__ loop_of_tri) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= nb) return;
	const uint32_t l = iloop[i];
	if (!fill[l]) return;
	const uint32_t n = table[l].n_edges, p = ipos[i];
	if (n == 3u && p != 0u) return;
	uint32_t a, b, c = nv + voff[l];
	hl_ends(idx, list[i], a, b);
	if (n == 3u) {
		uint32_t a1;
		hl_ends(idx, outh[b], a1, c);
	}
	const size_t t = (size_t)nt + toff[l] + p; // p < n = tadd[l]: inside the loop's share of the output
	oidx[3 * t] = b; oidx[3 * t + 1] = a; oidx[3 * t + 2] = c;
	if (loop_of_tri) loop_of_tri[t] = table[l].label;
}
__global__ __launch_bounds__(MESH_WG) void k_hl_emit_verts(const rnb_mesh_boundary_loop* __restrict__ table, const long long* __restrict__ sums, const uint32_t n_loops, const uint32_t* __restrict__ fill,
                                                        const uint32_t* __restrict__ voff, const uint32_t nv, float* __restrict__ overts, float* __restrict__ ocolors, float* __restrict__ onormals) {
#pragma clang fp contract(off)
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= n_loops || !fill[i] || table[i].n_edges <= 3u) return;
	const size_t d = 3 * ((size_t)nv + voff[i]);
	const double n = (double)table[i].n_edges;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		overts[d + k] = table[i].centroid[k];
		if (onormals) onormals[d + k] = table[i].normal[k];
		if (ocolors) ocolors[d + k] = (float)(hl_unq(sums[(size_t)i * HL_NSUM + 7 + k]) / n);
	}
}

} // namespace rnb
