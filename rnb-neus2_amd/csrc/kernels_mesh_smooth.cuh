// kernels_mesh_smooth.cuh — the smoothing stage of include/rnb_mesh_smooth.h (rnb_mesh_smooth, rnb_mesh_vertex_normals). The faces per edge come from the topology
// stage's edge join (TpEdgeKeys, k_tp_count / k_tp_fill); an edge is represented by its lowest half-edge, as there.
//   k_sm_edges                  one thread per half-edge walks its bucket: eface[h] = the faces on the edge where h represents it, else 0; per vertex the valence, the
//                               boundary edges and the non-manifold edges at it (integer sums, the lanes of a wavefront that hit one vertex summed first: tp_add)
//   k_sm_select_init, k_sm_grow the selection as the round a vertex entered it; one launch per ring, in place: a round only reads entries of earlier rounds
//   k_sm_kind                   one thread per vertex: kind, whether it moves and over which edges, the length of its neighbour list, the census' arrays and counts;
//                               a moving vertex with more than SM_THREAD_MAX neighbours is appended to the list of the wide ones (order: arbitrary, nothing reads it)
//   k_sm_fill                   the neighbour lists filled through an atomic cursor (the driver scans the lengths in between); order inside a list: arbitrary
//   k_sm_widen                  P_0 in both buffers
//   k_sm_pass, k_sm_pass_wide   THE HOT PATH: one pass as a pure gather, no atomics. A thread per vertex of up to SM_THREAD_MAX neighbours; a workgroup per wide vertex
//                               (the centre of a fan rnb_mesh_fill_holes made has the loop's length, up to 2^20), wave_sum<long long> and four partial sums in LDS.
//                               The sums are integers: the two paths cannot differ.
//   k_sm_finish                 the output vertices, the displacement and its maximum
//   k_vn_accumulate, k_vn_finish   the normals: one thread per triangle, its cross product into its three corners (64-bit integer atomics, grouped per wavefront); one
//                               thread per vertex normalises
// Operation for operation what tests/mesh_smooth_reference.py computes (compiled with -ffp-contract=off; the pragma says so once more where it matters). No kernel
// loops on device data until something converges. Vector loads, stores and atomics only.
#pragma once
#include "kernels_mesh_topology.cuh"
#include "../../include/rnb_mesh_smooth.h"

namespace rnb {

constexpr uint32_t SM_BAD_TERM = 2u, SM_BAD_RING = 4u; // bits of SmResult::flags / VnResult::flags, beside MESH_BAD_INDEX
constexpr uint32_t SM_THREAD_MAX = 32u;                // a moving vertex with more neighbours gets a workgroup per pass, not a thread
constexpr uint32_t SM_STAY = 0u, SM_MOVE_ALL = 1u, SM_MOVE_BOUNDARY = 2u; // mode[v]: over which edges a vertex moves

struct SmResult { // written by the kernels, read by the driver; zeroed before a call
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_edges, n_interior, n_boundary, n_nonmanifold, n_unused, n_selected, n_moving, max_valence, n_wide;
	uint32_t max_displacement; // the bits of a float >= 0: ordered like the unsigned integer
};
struct VnResult {
	uint32_t flags;
	uint32_t n_zero, max_corners;
};

__device__ __forceinline__ uint32_t sm_wave_max(uint32_t m) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off, 64));
	return m;
}
// fixed point of one term; false: not finite or not below 2^LOG2
template <int SHIFT, int LOG2>
__device__ __forceinline__ bool sm_q(const double term, long long* q) {
	const double lim = (double)(1ll << LOG2), scale = (double)(1ll << SHIFT);
	if (!(fabs(term) < lim)) { *q = 0; return false; } // also catches NaN and infinity
	*q = (long long)(term * scale);                    // a power of two: exact; the conversion truncates
	return true;
}
template <int SHIFT>
__device__ __forceinline__ double sm_unq(const long long q) { return (double)q * (1.0 / (double)(1ll << SHIFT)); } // int64 -> double rounds to nearest even

// ---- the edges ----
// vinfo: four words per vertex, zero on entry: valence, boundary edges, non-manifold edges at it (the fourth is not used).
__global__ __launch_bounds__(MESH_WG) void k_sm_edges(const TpEdgeKeys keys, const uint32_t n_half, const TpJoin join, uint32_t* __restrict__ eface, uint32_t* __restrict__ vinfo,
                                                   SmResult* __restrict__ res) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	k.a = k.b = MESH_NONE;
	const bool valid = h < n_half && keys.key(h, k);
	uint32_t faces = 0, first = h;
	if (valid) {
		uint32_t lo, hi;
		join.range(k, lo, hi);
		for (uint32_t s = lo; s < hi; ++s) {
			const uint32_t g = join.items[s];
			TpKey kg;
			if (!keys.key(g, kg) || !tp_equal(k, kg)) continue;
			++faces;
			first = min(first, g);
		}
	}
	const bool counts = valid && first == h; // the edge is counted by its lowest half-edge
	if (h < n_half) eface[h] = counts ? faces : 0u;
	const uint32_t bd = faces == 1u ? 1u : 0u, nm = faces >= 3u ? 1u : 0u;
	tp_add(vinfo, 4u, k.a, counts, 1u, bd, nm, 0u);
	tp_add(vinfo, 4u, k.b, counts, 1u, bd, nm, 0u);
	tp_count(&res->n_edges, counts ? 1u : 0u);
}

// ---- the selection ----
// sel[v] = the round v entered the selection: 0 for D_0, MESH_NONE while it is outside. select: null = every vertex.
__global__ __launch_bounds__(MESH_WG) void k_sm_select_init(const uint32_t* __restrict__ select, const uint32_t nv, uint32_t* __restrict__ sel) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv) sel[v] = (!select || select[v] != 0u) ? 0u : MESH_NONE;
}
// Round r: the other end of an edge with an end that entered in a round <= r enters in round r + 1. What this launch writes is r + 1, which this launch does not take
// for selected; every writer of an entry writes the same value.
__global__ __launch_bounds__(MESH_WG) void k_sm_grow(const TpEdgeKeys keys, const uint32_t* __restrict__ eface, const uint32_t n_half, const uint32_t r, uint32_t* sel) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	if (h >= n_half || !eface[h]) return;
	TpKey k;
	(void)keys.key(h, k); // eface[h] != 0: h is a half-edge of a non-degenerate triangle
	const uint32_t da = sel[k.a], db = sel[k.b];
	if (da <= r && db == MESH_NONE) sel[k.b] = r + 1u;
	if (db <= r && da == MESH_NONE) sel[k.a] = r + 1u;
}

// ---- per vertex: kind, mode, the length of the neighbour list ----
// len: nv + 1 words (the driver zeroes the last); it receives the entries of v's list: m for a moving vertex when lists are built (passes >= 1), else 0.
__global__ __launch_bounds__(MESH_WG) void k_sm_kind(const uint32_t* __restrict__ vinfo, const uint32_t* __restrict__ sel, const uint32_t nv, const uint32_t boundary, const uint32_t lists,
                                                  uint32_t* __restrict__ mode, uint32_t* __restrict__ len, uint32_t* __restrict__ wide, uint32_t* __restrict__ valence_out,
                                                  uint32_t* __restrict__ kind_out, SmResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	const bool in = v < nv;
	uint32_t deg = 0, bdeg = 0, nm = 0, kind = MESH_NONE, md = SM_STAY, m = 0;
	bool selected = false;
	if (in) {
		deg = vinfo[4 * (size_t)v]; bdeg = vinfo[4 * (size_t)v + 1]; nm = vinfo[4 * (size_t)v + 2];
		kind = !deg ? RNB_MESH_SMOOTH_KIND_UNUSED : (nm ? RNB_MESH_SMOOTH_KIND_NONMANIFOLD : (bdeg ? RNB_MESH_SMOOTH_KIND_BOUNDARY : RNB_MESH_SMOOTH_KIND_INTERIOR));
		selected = sel[v] != MESH_NONE;
		if (selected && kind == RNB_MESH_SMOOTH_KIND_INTERIOR) md = SM_MOVE_ALL;
		if (selected && kind == RNB_MESH_SMOOTH_KIND_BOUNDARY && boundary != RNB_MESH_SMOOTH_BOUNDARY_PIN) md = boundary == RNB_MESH_SMOOTH_BOUNDARY_SLIDE ? SM_MOVE_BOUNDARY : SM_MOVE_ALL;
		m = md == SM_MOVE_BOUNDARY ? bdeg : (md == SM_MOVE_ALL ? deg : 0u);
		mode[v] = md;
		len[v] = lists ? m : 0u;
		if (valence_out) valence_out[v] = deg;
		if (kind_out) kind_out[v] = kind;
		if (lists && m > RNB_MESH_SMOOTH_MAX_RING) (void)atomicOr(&res->flags, SM_BAD_RING);
		if (lists && m > SM_THREAD_MAX) wide[atomicAdd(&res->n_wide, 1u)] = v; // (at most nv of them: inside the list)
	}
	tp_count(&res->n_unused, kind == RNB_MESH_SMOOTH_KIND_UNUSED ? 1u : 0u);
	tp_count(&res->n_interior, kind == RNB_MESH_SMOOTH_KIND_INTERIOR ? 1u : 0u);
	tp_count(&res->n_boundary, kind == RNB_MESH_SMOOTH_KIND_BOUNDARY ? 1u : 0u);
	tp_count(&res->n_nonmanifold, kind == RNB_MESH_SMOOTH_KIND_NONMANIFOLD ? 1u : 0u);
	tp_count(&res->n_selected, selected ? 1u : 0u);
	tp_count(&res->n_moving, md != SM_STAY ? 1u : 0u);
	const uint32_t mx = sm_wave_max(deg);
	if ((threadIdx.x & 63u) == 0u && mx) (void)atomicMax(&res->max_valence, mx);
}
// cursor: a copy of the lists' offsets; every list's cursor runs to its end (the list of v takes exactly len[v] entries: k_sm_kind counted what this writes)
__global__ __launch_bounds__(MESH_WG) void k_sm_fill(const TpEdgeKeys keys, const uint32_t* __restrict__ eface, const uint32_t n_half, const uint32_t* __restrict__ mode,
                                                  uint32_t* __restrict__ cursor, uint32_t* __restrict__ adj) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	if (h >= n_half) return;
	const uint32_t faces = eface[h];
	if (!faces) return;
	TpKey k;
	(void)keys.key(h, k);
	const uint32_t ma = mode[k.a], mb = mode[k.b];
	if (ma == SM_MOVE_ALL || (ma == SM_MOVE_BOUNDARY && faces == 1u)) adj[atomicAdd(cursor + k.a, 1u)] = k.b;
	if (mb == SM_MOVE_ALL || (mb == SM_MOVE_BOUNDARY && faces == 1u)) adj[atomicAdd(cursor + k.b, 1u)] = k.a;
}

// ---- the passes ----
__global__ __launch_bounds__(MESH_WG) void k_sm_widen(const float* __restrict__ verts, const uint64_t n, double* __restrict__ p0, double* __restrict__ p1) {
	const uint64_t i = (uint64_t)blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= n) return;
	const double x = (double)verts[i];
	p0[i] = x; p1[i] = x;
}
// P_k of one vertex from its sums
__device__ __forceinline__ void sm_step(const double (&pv)[3], const long long (&s)[3], const uint32_t m, const double f, double* __restrict__ out) {
#pragma clang fp contract(off)
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		const double L = sm_unq<RNB_MESH_SMOOTH_Q_SHIFT>(s[c]) / (double)m;
		out[c] = pv[c] + f * L;
	}
}
// off: the lists' offsets, nv + 1 words. A thread per vertex with 1 .. SM_THREAD_MAX neighbours; every other entry of nxt keeps what it holds (P_0, or the wide kernel's).
__global__ __launch_bounds__(MESH_WG) void k_sm_pass(const uint32_t* __restrict__ off, const uint32_t* __restrict__ adj, const double* __restrict__ cur, double* __restrict__ nxt, const uint32_t nv,
                                                  const double f, SmResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	const uint32_t lo = off[v], m = off[v + 1] - lo;
	if (!m || m > SM_THREAD_MAX) return;
	const double pv[3] = {cur[3 * (size_t)v], cur[3 * (size_t)v + 1], cur[3 * (size_t)v + 2]};
	long long s[3] = {0, 0, 0};
	bool ok = true;
	for (uint32_t i = 0; i < m; ++i) {
		const size_t u = 3 * (size_t)adj[lo + i];
		long long q[3];
		ok &= sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u] - pv[0], &q[0]) & sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u + 1] - pv[1], &q[1]) &
		      sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u + 2] - pv[2], &q[2]);
		s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
	}
	if (!ok) (void)atomicOr(&res->flags, SM_BAD_TERM);
	sm_step(pv, s, m, f, nxt + 3 * (size_t)v);
}
// A workgroup per wide vertex: its threads stride over the list, the wavefronts sum their lanes, thread 0 adds the four partial sums.
__global__ __launch_bounds__(MESH_WG) void k_sm_pass_wide(const uint32_t* __restrict__ wide, const uint32_t* __restrict__ off, const uint32_t* __restrict__ adj, const double* __restrict__ cur,
                                                       double* __restrict__ nxt, const double f, SmResult* __restrict__ res) {
#pragma clang fp contract(off)
	__shared__ long long part[MESH_WG / 64][3];
	const uint32_t v = wide[blockIdx.x];
	const uint32_t lo = off[v], m = off[v + 1] - lo;
	const double pv[3] = {cur[3 * (size_t)v], cur[3 * (size_t)v + 1], cur[3 * (size_t)v + 2]};
	long long s[3] = {0, 0, 0};
	bool ok = true;
	for (uint32_t i = threadIdx.x; i < m; i += MESH_WG) {
		const size_t u = 3 * (size_t)adj[lo + i];
		long long q[3];
		ok &= sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u] - pv[0], &q[0]) & sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u + 1] - pv[1], &q[1]) &
		      sm_q<RNB_MESH_SMOOTH_Q_SHIFT, RNB_MESH_SMOOTH_Q_TERM_LOG2>(cur[u + 2] - pv[2], &q[2]);
		s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
	}
	if (!ok) (void)atomicOr(&res->flags, SM_BAD_TERM);
#pragma unroll
	for (int c = 0; c < 3; ++c) s[c] = wave_sum(s[c]);
	if ((threadIdx.x & 63u) == 0u) { part[threadIdx.x >> 6][0] = s[0]; part[threadIdx.x >> 6][1] = s[1]; part[threadIdx.x >> 6][2] = s[2]; }
	__syncthreads();
	if (threadIdx.x) return;
#pragma unroll
	for (int c = 0; c < 3; ++c) s[c] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
	sm_step(pv, s, m, f, nxt + 3 * (size_t)v);
}
static_assert(MESH_WG == 256, "k_sm_pass_wide adds the partial sums of four wavefronts");

// overts: the moving vertices rounded from p, the others as the input has them. disp: may be null.
__global__ __launch_bounds__(MESH_WG) void k_sm_finish(const float* __restrict__ verts, const double* __restrict__ p, const uint32_t* __restrict__ mode, const uint32_t nv, float* __restrict__ overts,
                                                    float* __restrict__ disp, SmResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	float dl = 0.0f;
	if (v < nv) {
		const size_t i = 3 * (size_t)v;
		const float x = verts[i], y = verts[i + 1], z = verts[i + 2];
		if (mode[v] != SM_STAY) {
			const double d[3] = {p[i] - (double)x, p[i + 1] - (double)y, p[i + 2] - (double)z};
			dl = (float)__dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
			overts[i] = (float)p[i]; overts[i + 1] = (float)p[i + 1]; overts[i + 2] = (float)p[i + 2];
		} else {
			overts[i] = x; overts[i + 1] = y; overts[i + 2] = z;
		}
		if (disp) disp[v] = dl;
	}
	const uint32_t mx = sm_wave_max(dl > 0.0f ? __float_as_uint(dl) : 0u); // (a NaN compares false; a failed call reports nothing)
	if ((threadIdx.x & 63u) == 0u && mx) (void)atomicMax(&res->max_displacement, mx);
}

// ---- the normals ----
// Adds q[0 .. 2] and one corner to the four 64-bit words of vertex v, the lanes of the wavefront that hold one vertex summed first (the hole stage's hl_accumulate).
// Called by whole wavefronts.
__device__ __forceinline__ void vn_add(long long* __restrict__ sums, const uint32_t v, bool valid, const long long (&q)[3]) {
	const uint32_t lane = threadIdx.x & 63u;
	const long long x[4] = {q[0], q[1], q[2], 1ll};
#pragma unroll 1
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(v, valid, g)) return;
		long long out = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const long long s = wave_sum(g.mine ? x[k] : 0ll);
			if ((int)lane == k) out = s;
		}
		if (lane < 4u && out) (void)atomicAdd((unsigned long long*)(sums + 4 * (size_t)g.key + lane), (unsigned long long)out);
	}
	if (valid) {
#pragma unroll
		for (int k = 0; k < 3; ++k)
			if (q[k]) (void)atomicAdd((unsigned long long*)(sums + 4 * (size_t)v + k), (unsigned long long)q[k]);
		(void)atomicAdd((unsigned long long*)(sums + 4 * (size_t)v + 3), 1ull);
	}
}
// sums: four 64-bit words per vertex, zero on entry: the three components and the corners
__global__ __launch_bounds__(MESH_WG) void k_vn_accumulate(const uint32_t* __restrict__ idx, const float* __restrict__ verts, const uint32_t nt, long long* __restrict__ sums, VnResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	const bool valid = t < nt;
	uint32_t a = MESH_NONE, b = MESH_NONE, c = MESH_NONE;
	long long q[3] = {0, 0, 0};
	if (valid) {
		a = idx[3 * (size_t)t]; b = idx[3 * (size_t)t + 1]; c = idx[3 * (size_t)t + 2];
		const double pa[3] = {(double)verts[3 * (size_t)a], (double)verts[3 * (size_t)a + 1], (double)verts[3 * (size_t)a + 2]};
		const double u[3] = {(double)verts[3 * (size_t)b] - pa[0], (double)verts[3 * (size_t)b + 1] - pa[1], (double)verts[3 * (size_t)b + 2] - pa[2]};
		const double w[3] = {(double)verts[3 * (size_t)c] - pa[0], (double)verts[3 * (size_t)c + 1] - pa[1], (double)verts[3 * (size_t)c + 2] - pa[2]};
		const bool ok = sm_q<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT, RNB_MESH_SMOOTH_NORMAL_Q_TERM_LOG2>(u[1] * w[2] - u[2] * w[1], &q[0]) &
		                sm_q<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT, RNB_MESH_SMOOTH_NORMAL_Q_TERM_LOG2>(u[2] * w[0] - u[0] * w[2], &q[1]) &
		                sm_q<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT, RNB_MESH_SMOOTH_NORMAL_Q_TERM_LOG2>(u[0] * w[1] - u[1] * w[0], &q[2]);
		if (!ok) (void)atomicOr(&res->flags, SM_BAD_TERM);
	}
	vn_add(sums, a, valid, q);
	vn_add(sums, b, valid, q);
	vn_add(sums, c, valid, q);
}
__global__ __launch_bounds__(MESH_WG) void k_vn_finish(const long long* __restrict__ sums, const uint32_t nv, const uint32_t flip, float* __restrict__ normals, VnResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t corners = 0;
	bool zero = false;
	if (v < nv) {
		const long long* __restrict__ s = sums + 4 * (size_t)v;
		const unsigned long long n = (unsigned long long)s[3];
		if (n > RNB_MESH_SMOOTH_MAX_RING) (void)atomicOr(&res->flags, SM_BAD_RING);
		corners = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
		const double A[3] = {sm_unq<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT>(s[0]), sm_unq<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT>(s[1]), sm_unq<RNB_MESH_SMOOTH_NORMAL_Q_SHIFT>(s[2])};
		const double len = __dsqrt_rn((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2]);
		zero = len == 0.0;
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const double x = A[k] / len;
			normals[3 * (size_t)v + k] = zero ? 0.0f : (float)(flip ? -x : x);
		}
	}
	tp_count(&res->n_zero, zero ? 1u : 0u);
	const uint32_t mx = sm_wave_max(corners);
	if ((threadIdx.x & 63u) == 0u && mx) (void)atomicMax(&res->max_corners, mx);
}

} // namespace rnb
