// kernels_mesh_snap.cuh — the snapping stage of include/rnb_mesh_snap.h (rnb_mesh_snap): guarded Newton steps of the vertices of a device mesh onto the level set of the
// model's SDF. The network itself is launch_forward on the packed inputs (the driver); these kernels are what stands around it.
//   (k_mesh_validate of mesh_common.cuh comes first: the triangles are carried, and refused before anything else if an index is out of range)
//   k_sn_init     one thread per vertex: P = P_prev = P0 (P lives in the output mesh's vertices), a_prev = +inf, the state (ACTIVE or UNSELECTED), the per-vertex
//                 outputs of an unselected vertex, the flag the first packing reads
//   k_sn_pack     the vertices whose flag is set, at the places their exclusive sums name (scan_exclusive of the driver in between; its total is the round's host read)
//   k_sn_coords   THE HOT PATH beside the network: the 7-float network input of the packed vertices, the arithmetic of k_mt_texels
//   k_sn_step     one thread per packed vertex: the 16 halves (load_out16), the rules of the header in double precision, state, P, P_prev, a_prev, the flag of the
//                 next packing. A vertex is computed from its own data alone: neither the batch size nor the packing can change a bit
//   k_sn_final    one thread per selected vertex after the evaluation at its final P: residual_after, attributes (the arithmetic of k_ms_vertex_attr), displacement,
//                 the counts per state, the integer sums and the maxima, reduced over the wavefront before the atomics
// Operation for operation what tests/mesh_snap_reference.py computes (compiled with -ffp-contract=off; the pragma says so once more where it matters). No kernel loops on
// device data until something converges: the rounds are the driver's. Vector loads, stores and atomics only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_snap.h"

namespace rnb {

constexpr uint32_t SN_ACTIVE = 9u; // the state of a vertex that is still moving: never leaves the call

struct SnParams { // the options widened once, on the host
	double level, tolerance, max_step, max_displacement, min_gradient2, diag;
	float aabb_min, aabb_diag;
};
struct SnResult { // written by the kernels, read by the driver; zeroed before a call
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_state[9];
	uint32_t n_moved;
	uint32_t max_displacement;                // the bits of a float >= 0: ordered like the unsigned integer
	unsigned long long max_before, max_after; // the bits of doubles >= 0, likewise
	unsigned long long sum_before_q, sum_after_q;
};

__device__ __forceinline__ unsigned long long sn_wave_max64(unsigned long long m) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const unsigned long long o = (unsigned long long)__shfl_xor((long long)m, off, 64);
		m = o > m ? o : m;
	}
	return m;
}
__device__ __forceinline__ uint32_t sn_wave_max32(uint32_t m) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off, 64));
	return m;
}
// |r| as the fixed point of the sums; 0 for a residual outside the range a valid vertex can have
__device__ __forceinline__ unsigned long long sn_q(const double r) {
	const double a = fabs(r);
	return a < (double)(1u << RNB_MESH_SNAP_RESIDUAL_LOG2) ? (unsigned long long)(a * (double)(1u << RNB_MESH_SNAP_Q_SHIFT)) : 0ull; // a power of two: exact; the conversion truncates
}

// verts -> overts (P) and prev (P_prev); select: null = every vertex. before / after / disp / the attributes of an unselected vertex are the driver's memsets and copies
// but for the three per-vertex arrays here, which may be null.
__global__ __launch_bounds__(MESH_WG) void k_sn_init(const float* __restrict__ verts, const uint32_t* __restrict__ select, const uint32_t nv, float* __restrict__ overts, float* __restrict__ prev,
                                                  double* __restrict__ a_prev, double* __restrict__ r_before, uint32_t* __restrict__ state, uint32_t* __restrict__ flag, SnResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	bool unselected = false;
	if (v < nv) {
		const size_t i = 3 * (size_t)v;
		const float x = verts[i], y = verts[i + 1], z = verts[i + 2];
		overts[i] = x; overts[i + 1] = y; overts[i + 2] = z;
		prev[i] = x; prev[i + 1] = y; prev[i + 2] = z;
		a_prev[v] = __longlong_as_double(0x7FF0000000000000ll);
		r_before[v] = 0.0;
		unselected = select && select[v] == 0u;
		state[v] = unselected ? RNB_MESH_SNAP_UNSELECTED : SN_ACTIVE;
		flag[v] = unselected ? 0u : 1u;
	}
	const uint32_t n = (uint32_t)__popcll(__ballot(unselected));
	if ((threadIdx.x & 63u) == 0u && n) (void)atomicAdd(&res->n_state[RNB_MESH_SNAP_UNSELECTED], n);
}

// pos: the exclusive sums of flag. list[pos[v]] = v for every flagged vertex (ascending: the packing is stable, though nothing depends on it).
__global__ __launch_bounds__(MESH_WG) void k_sn_pack(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, const uint32_t nv, uint32_t* __restrict__ list) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv && flag[v]) list[pos[v]] = v;
}
// the flag of the final packing: every selected vertex
__global__ __launch_bounds__(MESH_WG) void k_sn_selected(const uint32_t* __restrict__ state, const uint32_t nv, uint32_t* __restrict__ flag) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv) flag[v] = state[v] != RNB_MESH_SNAP_UNSELECTED ? 1u : 0u;
}

// The network input of the vertices list[0 .. nb - 1] at their positions p: k_mt_texels, expression for expression.
__global__ __launch_bounds__(MESH_WG) void k_sn_coords(const uint32_t* __restrict__ list, const uint32_t nb, const float* __restrict__ p, const float aabb_min, const float aabb_diag,
                                                    float* __restrict__ coords) {
#pragma clang fp contract(off)
	const uint32_t q = blockIdx.x * MESH_WG + threadIdx.x;
	if (q >= nb) return;
	const size_t i = 3 * (size_t)list[q];
	const float v[3] = {p[i], p[i + 1], p[i + 2]};
	const float d[3] = {v[0] - 0.5f, v[1] - 0.5f, v[2] - 0.5f};
	const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	float* c = coords + (size_t)q * 7;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		c[k] = fminf(fmaxf((v[k] - aabb_min) / aabb_diag, 0.f), 1.f);
		c[4 + k] = (d[k] / l + 1.f) * 0.5f;
	}
	c[3] = 0.f;
}

// One round for the vertices list[0 .. nb - 1], whose outputs are net[q]: the rules of the header, in their order. first: round 1; last: round iterations + 1.
__global__ __launch_bounds__(MESH_WG) void k_sn_step(const uint32_t* __restrict__ list, const uint32_t nb, const half_t* __restrict__ net, const float* __restrict__ verts, const SnParams P,
                                                  const uint32_t first, const uint32_t last, float* __restrict__ pos, float* __restrict__ prev, double* __restrict__ a_prev,
                                                  double* __restrict__ r_before, float* __restrict__ before, uint32_t* __restrict__ state, uint32_t* __restrict__ flag) {
#pragma clang fp contract(off)
	const uint32_t q = blockIdx.x * MESH_WG + threadIdx.x;
	if (q >= nb) return;
	const uint32_t v = list[q];
	const size_t i = 3 * (size_t)v;
	half_t o[16];
	load_out16(net + (size_t)q * 16, o);
	const double r = (double)h2f(o[3]) - P.level, ar = fabs(r);
	const double g[3] = {(double)h2f(o[4]), (double)h2f(o[5]), (double)h2f(o[6])};
	if (first) {
		r_before[v] = r;
		if (before) before[v] = (float)r;
	}
	const float p[3] = {pos[i], pos[i + 1], pos[i + 2]};
	uint32_t st = SN_ACTIVE;
	bool back = false; // P = P_prev
	float Q[3] = {p[0], p[1], p[2]};
	const bool finite = ar < (double)(1u << RNB_MESH_SNAP_RESIDUAL_LOG2) && fabs(g[0]) < __longlong_as_double(0x7FF0000000000000ll) && fabs(g[1]) < __longlong_as_double(0x7FF0000000000000ll) &&
	                    fabs(g[2]) < __longlong_as_double(0x7FF0000000000000ll); // (a NaN compares false)
	const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
	if (!finite) { st = RNB_MESH_SNAP_INVALID; back = true; }
	else if (ar > a_prev[v]) { st = RNB_MESH_SNAP_REVERTED; back = true; }
	else if (ar <= P.tolerance) st = RNB_MESH_SNAP_CONVERGED;
	else if (last) st = RNB_MESH_SNAP_UNFINISHED;
	else if (gg < P.min_gradient2) st = RNB_MESH_SNAP_FLAT;
	else {
		const double t = r / gg;
		double d[3] = {(t * g[0]) * P.diag, (t * g[1]) * P.diag, (t * g[2]) * P.diag};
		const double L = __dsqrt_rn((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
		if (L > P.max_step) {
			const double f = P.max_step / L;
			d[0] = d[0] * f; d[1] = d[1] * f; d[2] = d[2] * f;
		}
#pragma unroll
		for (int c = 0; c < 3; ++c) Q[c] = (float)((double)p[c] - d[c]);
		const double e[3] = {(double)Q[0] - (double)verts[i], (double)Q[1] - (double)verts[i + 1], (double)Q[2] - (double)verts[i + 2]};
		const double M = __dsqrt_rn((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
		bool outside = false;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const float n = (Q[c] - P.aabb_min) / P.aabb_diag;
			outside |= n < 0.f || n > 1.f;
		}
		if (M > P.max_displacement) st = RNB_MESH_SNAP_LEASHED;
		else if (outside) st = RNB_MESH_SNAP_OUTSIDE;
		else if (__float_as_uint(Q[0]) == __float_as_uint(p[0]) && __float_as_uint(Q[1]) == __float_as_uint(p[1]) && __float_as_uint(Q[2]) == __float_as_uint(p[2])) st = RNB_MESH_SNAP_STALLED;
	}
	if (back) {
		pos[i] = prev[i]; pos[i + 1] = prev[i + 1]; pos[i + 2] = prev[i + 2];
	} else if (st == SN_ACTIVE) {
		prev[i] = p[0]; prev[i + 1] = p[1]; prev[i + 2] = p[2];
		a_prev[v] = ar;
		pos[i] = Q[0]; pos[i + 1] = Q[1]; pos[i + 2] = Q[2];
	}
	state[v] = st;
	flag[v] = st == SN_ACTIVE ? 1u : 0u;
}

// The selected vertices list[0 .. nb - 1] after the evaluation at their final positions pos. colors / normals: the output's, written only where asked for (null
// otherwise); after / disp / state_out may be null.
__global__ __launch_bounds__(MESH_WG) void k_sn_final(const uint32_t* __restrict__ list, const uint32_t nb, const half_t* __restrict__ net, const float* __restrict__ verts, const float* __restrict__ pos,
                                                   const double level, const double* __restrict__ r_before, const uint32_t* __restrict__ state, float* __restrict__ after, float* __restrict__ disp,
                                                   float* __restrict__ colors, float* __restrict__ normals, SnResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t q = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t st = RNB_MESH_SNAP_UNSELECTED, moved = 0u, dbits = 0u;
	unsigned long long qb = 0, qa = 0, mb = 0, ma = 0;
	if (q < nb) {
		const uint32_t v = list[q];
		const size_t i = 3 * (size_t)v;
		half_t o[16];
		load_out16(net + (size_t)q * 16, o);
		const double r = (double)h2f(o[3]) - level;
		st = state[v];
		if (after) after[v] = (float)r;
		const float p[3] = {pos[i], pos[i + 1], pos[i + 2]}, p0[3] = {verts[i], verts[i + 1], verts[i + 2]};
		const double e[3] = {(double)p[0] - (double)p0[0], (double)p[1] - (double)p0[1], (double)p[2] - (double)p0[2]};
		const float dl = (float)__dsqrt_rn((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
		if (disp) disp[v] = dl;
		dbits = dl > 0.0f ? __float_as_uint(dl) : 0u; // (a NaN compares false)
		moved = (__float_as_uint(p[0]) != __float_as_uint(p0[0]) || __float_as_uint(p[1]) != __float_as_uint(p0[1]) || __float_as_uint(p[2]) != __float_as_uint(p0[2])) ? 1u : 0u;
		if (st != RNB_MESH_SNAP_INVALID) {
			const double rb = r_before[v];
			qb = sn_q(rb); qa = sn_q(r);
			mb = fabs(rb) < (double)(1u << RNB_MESH_SNAP_RESIDUAL_LOG2) ? (unsigned long long)__double_as_longlong(fabs(rb)) : 0ull;
			ma = fabs(r) < (double)(1u << RNB_MESH_SNAP_RESIDUAL_LOG2) ? (unsigned long long)__double_as_longlong(fabs(r)) : 0ull;
		}
		if (colors) {
			colors[i] = logistic(h2f(o[0])); colors[i + 1] = logistic(h2f(o[1])); colors[i + 2] = logistic(h2f(o[2]));
		}
		if (normals) { // k_ms_vertex_attr
			const Vec3 g = v3(h2f(o[4]), h2f(o[5]), h2f(o[6]));
			const float gn = sqrtf(dot(g, g));
			const Vec3 nr = gn > 0.f ? v3(g.x / gn, g.y / gn, g.z / gn) : v3(0.f, 0.f, 0.f);
			normals[i] = nr.x; normals[i + 1] = nr.y; normals[i + 2] = nr.z;
		}
	}
	// whole wavefronts from here on: one atomic per wavefront and quantity
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t mine = 0;
#pragma unroll
	for (uint32_t k = RNB_MESH_SNAP_CONVERGED; k <= RNB_MESH_SNAP_REVERTED; ++k) {
		const uint32_t n = (uint32_t)__popcll(__ballot(q < nb && st == k));
		if (lane == k) mine = n;
	}
	if (lane >= RNB_MESH_SNAP_CONVERGED && lane <= RNB_MESH_SNAP_REVERTED && mine) (void)atomicAdd(&res->n_state[lane], mine);
	const uint32_t n_moved = wave_sum(moved), dmax = sn_wave_max32(dbits);
	const unsigned long long sb = (unsigned long long)wave_sum((long long)qb), sa = (unsigned long long)wave_sum((long long)qa);
	mb = sn_wave_max64(mb); ma = sn_wave_max64(ma);
	if (lane == 0u) {
		if (n_moved) (void)atomicAdd(&res->n_moved, n_moved);
		if (dmax) (void)atomicMax(&res->max_displacement, dmax);
		if (sb) (void)atomicAdd(&res->sum_before_q, sb);
		if (sa) (void)atomicAdd(&res->sum_after_q, sa);
		if (mb) (void)atomicMax(&res->max_before, mb);
		if (ma) (void)atomicMax(&res->max_after, ma);
	}
}

} // namespace rnb
