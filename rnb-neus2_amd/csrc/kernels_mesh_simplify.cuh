// kernels_mesh_simplify.cuh — the mesh simplifier of include/rnb_mesh_simplify.h (rnb_mesh_simplify): vertex clustering on a uniform cell grid, the representative
// of a cell placed by quadric error minimisation.
//   (k_mesh_validate of mesh_common.cuh comes first: nothing is dereferenced through an index before that kernel has passed; it marks used[v])
//   k_sp_cells         used vertex -> finite check, its cell key, one bit per occupied cell set with an atomic OR
//   k_sp_popc          set bits per 32-cell word -> (scan_exclusive) -> the rank of a key among the occupied keys = its cluster id, ascending key
//   k_sp_members       vertex -> cluster id; count, sum of local positions, colours and normals of the cluster's members (fixed point)
//   k_sp_quadric       triangle -> the nine quadric terms in the frame of each of the up to three distinct clusters of its corners (fixed point)
//   k_sp_tris<WRITE>   surviving triangles: per-workgroup counts + the clusters they use -> exclusive sums -> cluster indices, in input order
//   k_sp_solve         one thread per cluster: mean or regularised quadric minimiser by the adjugate, clamped to the cell; position, colour, normal of the output vertex
// Nothing here depends on the schedule: ids and output slots are prefix sums, sums are 64-bit integers. sp_accumulate first adds up the lanes of a wavefront that hold
// the same cluster with shuffles (the extractor's output is brick-major: neighbouring vertices and triangles share cells) and issues the N sums of such a group as ONE
// atomic instruction of N lanes on N neighbouring 8-byte words; lanes left over after MESH_GROUP_ROUNDS groups (wave_group_next) issue their own. Operation for operation what
// tests/mesh_simplify_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters). Vector loads, stores and atomics only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_simplify.h"

namespace rnb {

constexpr uint32_t SP_BAD_VALUE = 2u, SP_BAD_TERM = 4u; // bits of SpResult::flags, beside MESH_BAD_INDEX
// the record of a cluster: SP_NSUM 64-bit sums
constexpr uint32_t SP_A = 0, SP_B = 6, SP_COUNT = 9, SP_X = 10, SP_COL = 13, SP_NRM = 16, SP_NSUM = 19;

struct SpResult { // written by the kernels, read by the driver
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_clamped;
	uint32_t n_fallback;
	uint32_t pad;
};

struct SpGrid {
	double origin[3];
	double cell;
	uint32_t dims[3];
};

__device__ __forceinline__ bool sp_finite3(const float* __restrict__ p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// p = (v - origin) / cell and the cell index of rule 1, per axis
__device__ __forceinline__ void sp_locate(const SpGrid& g, const float* __restrict__ v, double p[3], uint32_t i[3]) {
#pragma clang fp contract(off)
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		p[k] = ((double)v[k] - g.origin[k]) / g.cell;
		double f = floor(p[k]);
		const double hi = (double)(g.dims[k] - 1u);
		f = f < 0.0 ? 0.0 : f;
		f = f > hi ? hi : f;
		i[k] = (uint32_t)f;
	}
}
// fixed point of one term; false: not finite or not below the bound
__device__ __forceinline__ bool sp_q(const double term, long long* q) {
	const double lim = (double)(1ll << RNB_MESH_SIMPLIFY_Q_TERM_LOG2), scale = (double)(1ll << RNB_MESH_SIMPLIFY_Q_SHIFT);
	if (!(fabs(term) < lim)) { *q = 0; return false; } // also catches NaN and infinity
	*q = (long long)(term * scale);                    // a power of two: exact; the conversion truncates
	return true;
}
__device__ __forceinline__ double sp_unq(const long long q) { return (double)q * (1.0 / (double)(1ll << RNB_MESH_SIMPLIFY_Q_SHIFT)); } // int64 -> double rounds to nearest even

// Adds v[0..N) of every valid lane to sums[c * SP_NSUM + first ..]. Called by whole wavefronts.
template <int N>
__device__ __forceinline__ void sp_accumulate(long long* __restrict__ sums, const uint32_t first, const uint32_t c, bool valid, const long long (&v)[N]) {
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(c, valid, g)) return;
		long long out = 0;
#pragma unroll
		for (int k = 0; k < N; ++k) {
			const long long s = wave_sum(g.mine ? v[k] : 0ll);
			if ((int)lane == k) out = s;
		}
		if ((int)lane < N && out) (void)atomicAdd((unsigned long long*)(sums + (size_t)g.key * SP_NSUM + first + lane), (unsigned long long)out);
	}
	if (valid) {
#pragma unroll
		for (int k = 0; k < N; ++k)
			if (v[k]) (void)atomicAdd((unsigned long long*)(sums + (size_t)c * SP_NSUM + first + k), (unsigned long long)v[k]);
	}
}

// vkey[v] = the key of a used vertex (< 2^30: RNB_MESH_SIMPLIFY_MAX_CELLS), MESH_NONE otherwise; bits: one per cell
__global__ __launch_bounds__(MESH_WG) void k_sp_cells(const SpGrid g, const float* __restrict__ verts, const float* __restrict__ colors, const float* __restrict__ normals, const uint32_t nv,
                                                   const uint32_t* __restrict__ used, uint32_t* __restrict__ vkey, uint32_t* __restrict__ bits, SpResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	uint32_t key = MESH_NONE;
	if (used[v]) {
		const size_t s = 3 * (size_t)v;
		if (sp_finite3(verts + s) && (!colors || sp_finite3(colors + s)) && (!normals || sp_finite3(normals + s))) {
			double p[3];
			uint32_t i[3];
			sp_locate(g, verts + s, p, i);
			key = i[0] + g.dims[0] * (i[1] + g.dims[1] * i[2]);
			(void)atomicOr(bits + (key >> 5), 1u << (key & 31u));
		} else (void)atomicOr(&res->flags, SP_BAD_VALUE);
	}
	vkey[v] = key;
}
__global__ __launch_bounds__(MESH_WG) void k_sp_popc(const uint32_t* __restrict__ bits, uint32_t* __restrict__ rank, const uint32_t n_words) {
	const uint32_t w = blockIdx.x * MESH_WG + threadIdx.x;
	if (w < n_words) rank[w] = __popc(bits[w]);
}
// vcl (in) the key of the vertex, (out) its cluster id; rank: the exclusive sums of k_sp_popc's counts
__global__ __launch_bounds__(MESH_WG) void k_sp_members(const SpGrid g, const float* __restrict__ verts, const float* __restrict__ colors, const float* __restrict__ normals, const uint32_t nv,
                                                     const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rank, uint32_t* __restrict__ vcl, uint32_t* __restrict__ ckey,
                                                     long long* __restrict__ sums, SpResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t c = MESH_NONE;
	long long q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // count, x, colour, normal
	const uint32_t key = v < nv ? vcl[v] : MESH_NONE;
	if (key != MESH_NONE) {
		c = rank[key >> 5] + __popc(bits[key >> 5] & ((1u << (key & 31u)) - 1u));
		vcl[v] = c;
		ckey[c] = key; // (every member writes the same value)
		const size_t s = 3 * (size_t)v;
		double p[3];
		uint32_t i[3];
		sp_locate(g, verts + s, p, i);
		bool ok = true;
		q[0] = 1;
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			ok = sp_q(p[k] - ((double)i[k] + 0.5), &q[1 + k]) && ok;
			if (colors) ok = sp_q((double)colors[s + k], &q[4 + k]) && ok;
			if (normals) ok = sp_q((double)normals[s + k], &q[7 + k]) && ok;
		}
		if (!ok) (void)atomicOr(&res->flags, SP_BAD_TERM);
	}
	sp_accumulate<10>(sums, SP_COUNT, c, c != MESH_NONE, q);
}

// the nine terms of rule 3 for the triangle (a, b, c), its corners given in the cluster's frame; false: nothing to add (zero area) -- *bad is set when a term is refused
__device__ __forceinline__ bool sp_quadric_terms(const double a[3], const double b[3], const double c[3], long long (&q)[9], bool* bad) {
#pragma clang fp contract(off)
	const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
	const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
	const double l = __dsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
	if (l == 0.0) return false;
	const double w = 0.5 * l;
	const double h[3] = {n[0] / l, n[1] / l, n[2] / l};
	const double d = -((h[0] * a[0] + h[1] * a[1]) + h[2] * a[2]);
	const double g[3] = {w * h[0], w * h[1], w * h[2]};
	bool ok = sp_q(g[0] * h[0], &q[0]);
	ok = sp_q(g[0] * h[1], &q[1]) && ok;
	ok = sp_q(g[0] * h[2], &q[2]) && ok;
	ok = sp_q(g[1] * h[1], &q[3]) && ok;
	ok = sp_q(g[1] * h[2], &q[4]) && ok;
	ok = sp_q(g[2] * h[2], &q[5]) && ok;
	ok = sp_q(g[0] * d, &q[6]) && ok;
	ok = sp_q(g[1] * d, &q[7]) && ok;
	ok = sp_q(g[2] * d, &q[8]) && ok;
	if (!ok) *bad = true;
	return true;
}
__global__ __launch_bounds__(MESH_WG) void k_sp_quadric(const SpGrid g, const float* __restrict__ verts, const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ vcl,
                                                     long long* __restrict__ sums, SpResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	const bool live = t < nt;
	uint32_t cl[3] = {MESH_NONE, MESH_NONE, MESH_NONE};
	double p[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ctr[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	if (live) {
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const uint32_t vi = idx[3 * (size_t)t + k];
			uint32_t i[3];
			sp_locate(g, verts + 3 * (size_t)vi, p[k], i);
			ctr[k][0] = (double)i[0] + 0.5; ctr[k][1] = (double)i[1] + 0.5; ctr[k][2] = (double)i[2] + 0.5;
			cl[k] = vcl[vi];
		}
	}
	bool bad = false;
#pragma unroll
	for (int s = 0; s < 3; ++s) { // the cluster of corner s, unless an earlier corner has it
		bool valid = live && (s < 1 || cl[s] != cl[0]) && (s < 2 || cl[s] != cl[1]);
		long long q[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
		if (valid) {
			double f[3][3];
#pragma unroll
			for (int k = 0; k < 3; ++k) { f[k][0] = p[k][0] - ctr[s][0]; f[k][1] = p[k][1] - ctr[s][1]; f[k][2] = p[k][2] - ctr[s][2]; }
			valid = sp_quadric_terms(f[0], f[1], f[2], q, &bad);
		}
		sp_accumulate<9>(sums, SP_A, cl[s], valid, q);
	}
	if (bad) (void)atomicOr(&res->flags, SP_BAD_TERM);
}

// vcl: cluster id per vertex. WRITE = false: surviving triangles per workgroup, cused[c] = 1 for the clusters they use; WRITE = true: their indices (cmap: the
// exclusive sums of cused = the output vertex of a cluster) from wg_offset (in triangles) on, in input order.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_sp_tris(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ vcl, uint32_t* __restrict__ cused, const uint32_t* __restrict__ cmap,
                                                  uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ oidx) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t a = 0, b = 0, c = 0, f = 0;
	if (t < nt) {
		a = vcl[idx[3 * (size_t)t]]; b = vcl[idx[3 * (size_t)t + 1]]; c = vcl[idx[3 * (size_t)t + 2]];
		f = (a != b && b != c && a != c) ? 1u : 0u;
	}
	uint32_t total;
	const uint32_t local = wg_exclusive_256(f, &total);
	if (!WRITE) {
		if (f) { cused[a] = 1u; cused[b] = 1u; cused[c] = 1u; }
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (!f) return;
	const size_t d = 3 * ((size_t)wg_offset[blockIdx.x] + local);
	oidx[d] = cmap[a]; oidx[d + 1] = cmap[b]; oidx[d + 2] = cmap[c];
}

// rule 4, one thread per cluster; only the clusters a surviving triangle uses are output vertices
__global__ __launch_bounds__(MESH_WG) void k_sp_solve(const SpGrid g, const uint32_t placement, const uint32_t n_clusters, const long long* __restrict__ sums, const uint32_t* __restrict__ ckey,
                                                   const uint32_t* __restrict__ cused, const uint32_t* __restrict__ cmap, float* __restrict__ overts, float* __restrict__ ocolors,
                                                   float* __restrict__ onormals, SpResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t c = blockIdx.x * MESH_WG + threadIdx.x;
	bool clamped = false, fallback = false;
	if (c < n_clusters && cused[c]) {
		const long long* __restrict__ r = sums + (size_t)c * SP_NSUM;
		const double count = (double)r[SP_COUNT];
		const double m[3] = {sp_unq(r[SP_X]) / count, sp_unq(r[SP_X + 1]) / count, sp_unq(r[SP_X + 2]) / count};
		double x[3] = {m[0], m[1], m[2]};
		if (placement == RNB_MESH_PLACE_QUADRIC) {
			const double axx = sp_unq(r[SP_A]), axy = sp_unq(r[SP_A + 1]), axz = sp_unq(r[SP_A + 2]), ayy = sp_unq(r[SP_A + 3]), ayz = sp_unq(r[SP_A + 4]), azz = sp_unq(r[SP_A + 5]);
			const double tr = (axx + ayy) + azz;
			fallback = true;
			if (tr != 0.0) {
				const double e = tr * (1.0 / 1024.0);
				const double m00 = axx + e, m11 = ayy + e, m22 = azz + e, m01 = axy, m02 = axz, m12 = ayz;
				const double r0 = e * m[0] - sp_unq(r[SP_B]), r1 = e * m[1] - sp_unq(r[SP_B + 1]), r2 = e * m[2] - sp_unq(r[SP_B + 2]);
				const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
				const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
				const double det = (m00 * c00 + m01 * c01) + m02 * c02;
				if (det > 0.0) {
					const double y0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det, y1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det, y2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
					if (isfinite(y0) && isfinite(y1) && isfinite(y2)) { x[0] = y0; x[1] = y1; x[2] = y2; fallback = false; }
				}
			}
		}
		const uint32_t key = ckey[c];
		const uint32_t i[3] = {key % g.dims[0], (key / g.dims[0]) % g.dims[1], key / (g.dims[0] * g.dims[1])};
		const size_t d = 3 * (size_t)cmap[c];
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			if (x[k] < -0.5) { x[k] = -0.5; clamped = true; }
			if (x[k] > 0.5) { x[k] = 0.5; clamped = true; }
			overts[d + k] = (float)((((double)i[k] + 0.5) + x[k]) * g.cell + g.origin[k]);
		}
		if (ocolors) {
#pragma unroll
			for (int k = 0; k < 3; ++k) ocolors[d + k] = (float)(sp_unq(r[SP_COL + k]) / count);
		}
		if (onormals) {
			const double s[3] = {sp_unq(r[SP_NRM]), sp_unq(r[SP_NRM + 1]), sp_unq(r[SP_NRM + 2])};
			const double l = __dsqrt_rn((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
#pragma unroll
			for (int k = 0; k < 3; ++k) onormals[d + k] = l == 0.0 ? 0.0f : (float)(s[k] / l);
		}
	}
	const uint32_t n_cl = (uint32_t)__popcll(__ballot(clamped)), n_fb = (uint32_t)__popcll(__ballot(fallback));
	if ((threadIdx.x & 63u) == 0) {
		if (n_cl) (void)atomicAdd(&res->n_clamped, n_cl);
		if (n_fb) (void)atomicAdd(&res->n_fallback, n_fb);
	}
}

} // namespace rnb
