// kernels_mesh_distance.cuh — the mesh-to-mesh distance of include/rnb_mesh_distance.h (rnb_mesh_distance): for samples of the surface of A, the distance to the nearest
// point of the surface of B, found through uniform cell lists over B's box.
//   (k_mesh_validate of mesh_common.cuh comes first, for A and for B: nothing is dereferenced through an index before that kernel has passed; it marks used[v])
//   k_md_verts            used vertices counted, their coordinates checked to be finite; for B the bounding box, as min / max of an order-preserving integer image of the floats
//   k_md_degenerate       triangles of B with l == 0, counted (the automatic grid size needs the others' number)
//   k_md_register<FILL>   triangle of B -> the cells its box overlaps: counts per cell -> (scan_exclusive) -> the lists; a box over more than RNB_MESH_DISTANCE_LARGE_CELLS
//                         cells -> the large list instead, so that no thread walks millions of cells for one triangle
//   k_md_query<VERTS>     one thread per sample (a vertex of A, or a sub-centroid of a triangle of A): the large list, then Chebyshev shells of cells until the stop rule of
//                         the header holds; per-vertex outputs, or the fixed-point sums, reduced over the wavefront before one lane issues the atomics
// Nothing that leaves the call depends on the schedule: the order inside a cell's list does (atomic cursors), but the minimum with its lowest-index tie-break does not, the
// sums are integers and the maximum is a maximum. Operation for operation what tests/mesh_distance_reference.py computes (this file is compiled with -ffp-contract=off; the
// pragma says so once more where it matters). Vector loads, stores and atomics only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_distance.h"

namespace rnb {

constexpr uint32_t MD_BAD_INDEX_TO = 2u, MD_BAD_VALUE = 4u, MD_BAD_TERM = 8u; // bits of MdResult::flags, beside MESH_BAD_INDEX (an index of from)
constexpr int MD_NSUM = 3 + RNB_MESH_DISTANCE_MAX_TAUS;                                                 // S(w), S(w d'), S(w d'^2), within[4]

struct MdResult { // written by the kernels, read by the driver
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_large;
	uint32_t bmin[3], bmax[3]; // images (md_image) of the box of B's used vertices
	uint32_t n_used_from, n_used_to, n_deg_from, n_deg_to, n_verts_beyond, pad;
	unsigned long long n_entries, n_samples, n_beyond, n_pairs, max_bits;
	unsigned long long lo[MD_NSUM], hi[MD_NSUM]; // every term's low 32 bits and the rest, summed apart: neither word can wrap below 2^32 samples
};

struct MdGrid {
	double lo[3], hi[3];
	double cell;
	uint32_t dims[3];
};
struct MdQuery {
	double cap;  // D, 0 = none
	double unit;
	double tau[RNB_MESH_DISTANCE_MAX_TAUS];
	uint32_t level;
};
struct MdMesh {
	const float* verts;
	const uint32_t* idx;
	uint32_t nv, nt;
};

// order-preserving image of a float that is not a NaN: a < b  <=>  md_image(a) < md_image(b) (-0 sorts below +0, which are the same number)
__device__ __forceinline__ uint32_t md_image(const float x) { const uint32_t u = __float_as_uint(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

__device__ __forceinline__ void md_corners(const MdMesh& m, const uint32_t t, double a[3], double b[3], double c[3]) {
	const uint32_t i0 = m.idx[3 * (size_t)t], i1 = m.idx[3 * (size_t)t + 1], i2 = m.idx[3 * (size_t)t + 2];
#pragma unroll
	for (int k = 0; k < 3; ++k) { a[k] = (double)m.verts[3 * (size_t)i0 + k]; b[k] = (double)m.verts[3 * (size_t)i1 + k]; c[k] = (double)m.verts[3 * (size_t)i2 + k]; }
}
__device__ __forceinline__ double md_dot(const double x[3], const double y[3]) {
#pragma clang fp contract(off)
	return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}
// l of rule 1
__device__ __forceinline__ double md_normal_length(const double a[3], const double b[3], const double c[3]) {
#pragma clang fp contract(off)
	const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
	const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
	return __dsqrt_rn(md_dot(n, n));
}
// the cell of a coordinate along axis k
__device__ __forceinline__ uint32_t md_cell(const MdGrid& g, const int k, const double x) {
#pragma clang fp contract(off)
	double f = floor((x - g.lo[k]) / g.cell);
	const double hi = (double)(g.dims[k] - 1u);
	f = f > 0.0 ? f : 0.0; // (also a NaN, which cannot come: the coordinates were checked)
	f = f > hi ? hi : f;
	return (uint32_t)f;
}

// rule 2: s(p, T)
__device__ __forceinline__ double md_point_triangle(const double p[3], const double a[3], const double b[3], const double c[3]) {
#pragma clang fp contract(off)
	const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
	const double d1 = md_dot(ab, ap), d2 = md_dot(ac, ap);
	const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
	const double d3 = md_dot(ab, bp), d4 = md_dot(ac, bp);
	const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
	const double d5 = md_dot(ab, cp), d6 = md_dot(ac, cp);
	const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, g = d4 - d3, h = d5 - d6;
	double q[3];
	if (d1 <= 0.0 && d2 <= 0.0) { q[0] = a[0]; q[1] = a[1]; q[2] = a[2]; }
	else if (d3 >= 0.0 && d4 <= d3) { q[0] = b[0]; q[1] = b[1]; q[2] = b[2]; }
	else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
		const double t = d1 / (d1 - d3);
		q[0] = a[0] + ab[0] * t; q[1] = a[1] + ab[1] * t; q[2] = a[2] + ab[2] * t;
	} else if (d6 >= 0.0 && d5 <= d6) { q[0] = c[0]; q[1] = c[1]; q[2] = c[2]; }
	else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
		const double t = d2 / (d2 - d6);
		q[0] = a[0] + ac[0] * t; q[1] = a[1] + ac[1] * t; q[2] = a[2] + ac[2] * t;
	} else if (va <= 0.0 && g >= 0.0 && h >= 0.0) {
		const double t = g / (g + h);
		q[0] = b[0] + (c[0] - b[0]) * t; q[1] = b[1] + (c[1] - b[1]) * t; q[2] = b[2] + (c[2] - b[2]) * t;
	} else {
		const double k = (va + vb) + vc, y = vb / k, z = vc / k;
		q[0] = (a[0] + ab[0] * y) + ac[0] * z; q[1] = (a[1] + ab[1] * y) + ac[1] * z; q[2] = (a[2] + ab[2] * y) + ac[2] * z;
	}
	const double e[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
	return md_dot(e, e);
}

// One thread per vertex. Counts the used ones and checks them; BOX: min / max of their images into res->bmin / bmax (reduced over the wavefront first).
template <bool BOX>
__global__ __launch_bounds__(MESH_WG) void k_md_verts(const float* __restrict__ verts, const uint32_t nv, const uint32_t* __restrict__ used, MdResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	const bool live = v < nv && used[v] != 0u;
	uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
	bool bad = false;
	if (live) {
		const float x[3] = {verts[3 * (size_t)v], verts[3 * (size_t)v + 1], verts[3 * (size_t)v + 2]};
		if (isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
#pragma unroll
			for (int k = 0; k < 3; ++k) mn[k] = mx[k] = md_image(x[k]);
		} else bad = true;
	}
	const uint32_t n_live = (uint32_t)__popcll(__ballot(live));
	const bool any_bad = __ballot(bad) != 0ull;
	if (BOX) {
#pragma unroll
		for (int k = 0; k < 3; ++k) {
#pragma unroll
			for (int off = 32; off >= 1; off >>= 1) {
				mn[k] = min(mn[k], (uint32_t)__shfl_xor(mn[k], off, 64));
				mx[k] = max(mx[k], (uint32_t)__shfl_xor(mx[k], off, 64));
			}
		}
	}
	if ((threadIdx.x & 63u) == 0 && n_live) {
		(void)atomicAdd(BOX ? &res->n_used_to : &res->n_used_from, n_live);
		if (any_bad) (void)atomicOr(&res->flags, MD_BAD_VALUE);
		if (BOX) {
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				if (mn[k] <= mx[k]) { (void)atomicMin(&res->bmin[k], mn[k]); (void)atomicMax(&res->bmax[k], mx[k]); }
			}
		}
	}
}

__global__ __launch_bounds__(MESH_WG) void k_md_degenerate(const MdMesh B, MdResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	bool deg = false;
	if (t < B.nt) {
		double a[3], b[3], c[3];
		md_corners(B, t, a, b, c);
		deg = md_normal_length(a, b, c) == 0.0;
	}
	const uint32_t n = (uint32_t)__popcll(__ballot(deg));
	if ((threadIdx.x & 63u) == 0 && n) (void)atomicAdd(&res->n_deg_to, n);
}

// FILL = false: count[cell] += 1 for every cell the box of a non-degenerate triangle overlaps, res->n_entries their number; the triangles of the large list (slots by an atomic
// counter; the list is complete only if res->n_large <= RNB_MESH_DISTANCE_MAX_LARGE). FILL = true: cursor[cell] (in: the exclusive sums of the counts) hands out the slots
// of entries[]; afterwards cursor[cell] is the end of the cell's list.
template <bool FILL>
__global__ __launch_bounds__(MESH_WG) void k_md_register(const MdGrid g, const MdMesh B, uint32_t* __restrict__ cells, uint32_t* __restrict__ entries, uint32_t* __restrict__ large, MdResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	long long mine = 0;
	if (t < B.nt) {
		double a[3], b[3], c[3];
		md_corners(B, t, a, b, c);
		if (md_normal_length(a, b, c) != 0.0) {
			uint32_t c0[3], c1[3];
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				c0[k] = md_cell(g, k, fmin(fmin(a[k], b[k]), c[k]));
				c1[k] = md_cell(g, k, fmax(fmax(a[k], b[k]), c[k]));
			}
			const uint32_t n = (c1[0] - c0[0] + 1u) * (c1[1] - c0[1] + 1u) * (c1[2] - c0[2] + 1u); // <= 2^24
			if (n > RNB_MESH_DISTANCE_LARGE_CELLS) {
				if (!FILL) {
					const uint32_t slot = atomicAdd(&res->n_large, 1u);
					if (slot < RNB_MESH_DISTANCE_MAX_LARGE) large[slot] = t;
				}
			} else {
				mine = (long long)n;
				for (uint32_t z = c0[2]; z <= c1[2]; ++z)
					for (uint32_t y = c0[1]; y <= c1[1]; ++y)
						for (uint32_t x = c0[0]; x <= c1[0]; ++x) {
							const uint32_t cell = x + g.dims[0] * (y + g.dims[1] * z);
							const uint32_t slot = atomicAdd(cells + cell, 1u);
							if (FILL) entries[slot] = t;
						}
			}
		}
	}
	if (!FILL) {
		const long long total = wave_sum(mine);
		if ((threadIdx.x & 63u) == 0 && total) (void)atomicAdd(&res->n_entries, (unsigned long long)total);
	}
}

struct MdSearch { // B and its cell lists
	MdMesh B;
	const uint32_t* start; // exclusive sums of the counts
	const uint32_t* end;   // the cursors after the fill
	const uint32_t* entries;
	const uint32_t* large;
	uint32_t n_large;
};
struct MdBest { double s; uint32_t t; unsigned long long pairs; };

__device__ __forceinline__ void md_try(const MdMesh& B, const double p[3], const uint32_t t, MdBest& best) {
	double a[3], b[3], c[3];
	md_corners(B, t, a, b, c);
	const double s = md_point_triangle(p, a, b, c);
	if (s < best.s || (s == best.s && t < best.t)) { best.s = s; best.t = t; } // (a NaN never wins)
	++best.pairs;
}
__device__ __forceinline__ void md_visit(const MdSearch& S, const MdGrid& g, const double p[3], const uint32_t x, const uint32_t y, const uint32_t z, MdBest& best) {
	const uint32_t cell = x + g.dims[0] * (y + g.dims[1] * z);
	const uint32_t e1 = S.end[cell];
	for (uint32_t e = S.start[cell]; e < e1; ++e) md_try(S.B, p, S.entries[e], best);
}
// rule 3 for one point, by the search of the header
__device__ __forceinline__ void md_search(const MdSearch& S, const MdGrid& g, const double cap, const double p[3], MdBest& best) {
#pragma clang fp contract(off)
	best.s = __longlong_as_double(0x7FF0000000000000ll); best.t = MESH_NONE; best.pairs = 0;
	for (uint32_t k = 0; k < S.n_large; ++k) md_try(S.B, p, S.large[k], best);
	int c[3], rmax = 0;
	double o[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		double q = p[k];
		q = q < g.lo[k] ? g.lo[k] : q;
		q = q > g.hi[k] ? g.hi[k] : q;
		o[k] = p[k] - q;
		c[k] = (int)md_cell(g, k, q);
		rmax = max(rmax, max(c[k], (int)g.dims[k] - 1 - c[k]));
	}
	const double o2 = md_dot(o, o) * (1.0 - 1.0 / 1048576.0), cap2 = cap * cap;
	for (int r = 0; r <= rmax; ++r) {
		const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, (int)g.dims[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, (int)g.dims[1] - 1);
		const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, (int)g.dims[0] - 1);
		for (int z = z0; z <= z1; ++z)
			for (int y = y0; y <= y1; ++y) {
				if (abs(z - c[2]) == r || abs(y - c[1]) == r) {
					for (int x = x0; x <= x1; ++x) md_visit(S, g, p, (uint32_t)x, (uint32_t)y, (uint32_t)z, best);
				} else { // r >= 1 here: the two faces of the shell along x
					if (c[0] - r >= 0) md_visit(S, g, p, (uint32_t)(c[0] - r), (uint32_t)y, (uint32_t)z, best);
					if (c[0] + r <= (int)g.dims[0] - 1) md_visit(S, g, p, (uint32_t)(c[0] + r), (uint32_t)y, (uint32_t)z, best);
				}
			}
		if (r >= 1) {
			const double e = ((double)r - 0.0625) * g.cell;
			const double bound = e * e + o2;
			if (best.s <= bound || (cap > 0.0 && bound >= cap2)) break;
		}
	}
}

// fixed point of one term (rule 5), split into its low 32 bits and the rest; false: not finite or not below the bound
__device__ __forceinline__ bool md_q(const double term, unsigned long long* lo, unsigned long long* hi) {
	const double lim = (double)(1ll << RNB_MESH_DISTANCE_Q_TERM_LOG2), scale = (double)(1ll << RNB_MESH_DISTANCE_Q_SHIFT);
	if (!(term >= 0.0 && term < lim)) { *lo = 0; *hi = 0; return false; } // also catches NaN and infinity
	const unsigned long long q = (unsigned long long)(term * scale);      // a power of two: exact; the conversion truncates
	*lo = q & 0xFFFFFFFFull; *hi = q >> 32;
	return true;
}

// VERTS = true: thread i is vertex i of A (samples (a)): vert_dist / vert_nearest, the maximum, n_verts_beyond. VERTS = false: thread i is sub-centroid i % n^2 of triangle
// i / n^2 of A (samples (b)): the sums, the maximum, the counts.
template <bool VERTS>
__global__ __launch_bounds__(MESH_WG) void k_md_query(const MdGrid g, const MdQuery Q, const MdMesh A, const uint32_t* __restrict__ used, const MdSearch S, float* __restrict__ vert_dist,
                                                   uint32_t* __restrict__ vert_nearest, MdResult* __restrict__ res) {
#pragma clang fp contract(off)
	const unsigned long long i = (unsigned long long)blockIdx.x * MESH_WG + threadIdx.x;
	const uint32_t n = 1u << Q.level, nn = n * n;
	bool sample = false, degenerate = false;
	double p[3] = {0.0, 0.0, 0.0}, w = 0.0;
	if (VERTS) {
		if (i < A.nv) {
			sample = used[i] != 0u;
			if (sample) { p[0] = (double)A.verts[3 * i]; p[1] = (double)A.verts[3 * i + 1]; p[2] = (double)A.verts[3 * i + 2]; }
			else {
				if (vert_dist) vert_dist[i] = 0.0f;
				if (vert_nearest) vert_nearest[i] = MESH_NONE;
			}
		}
	} else if (i < (unsigned long long)A.nt * nn) {
		const uint32_t t = (uint32_t)(i / nn);
		uint32_t k = (uint32_t)(i % nn);
		double a[3], b[3], c[3];
		md_corners(A, t, a, b, c);
		const double l = md_normal_length(a, b, c);
		if (l == 0.0) degenerate = k == 0u;
		else {
			sample = true;
			// sub-triangle k: the n (n + 1) / 2 upward ones row by row (row i holds j = 0 .. n - 1 - i), then the downward ones (row i holds j = 0 .. n - 2 - i)
			const uint32_t n_up = n * (n + 1u) / 2u;
			const bool up = k < n_up;
			if (!up) k -= n_up;
			uint32_t bi = 0, row = up ? n : n - 1u;
			while (k >= row) { k -= row; --row; ++bi; }
			const uint32_t bj = k;
			const uint32_t na = 3u * bi + (up ? 1u : 2u), nb = 3u * bj + (up ? 1u : 2u), nc = 3u * n - na - nb;
			const double den = (double)(3u * n);
			const double al = (double)na / den, be = (double)nb / den, ga = (double)nc / den;
#pragma unroll
			for (int d = 0; d < 3; ++d) p[d] = (a[d] * al + b[d] * be) + c[d] * ga;
			w = (0.5 * l) / (double)nn;
		}
	}
	MdBest best;
	best.s = 0.0; best.t = MESH_NONE; best.pairs = 0;
	double d = 0.0;
	bool beyond = false;
	if (sample) {
		md_search(S, g, Q.cap, p, best);
		d = __dsqrt_rn(best.s);
		if (Q.cap > 0.0 && d > Q.cap) { d = Q.cap; best.t = MESH_NONE; beyond = true; }
	}
	const uint32_t lane = threadIdx.x & 63u;
	unsigned long long mx = sample ? (unsigned long long)__double_as_longlong(d) : 0ull; // d >= 0 (or a NaN, whose pattern is larger than every number's: it shows)
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) { const unsigned long long y = (unsigned long long)__shfl_xor((long long)mx, off, 64); mx = y > mx ? y : mx; }
	const long long pairs = wave_sum((long long)best.pairs);
	const uint32_t n_beyond = (uint32_t)__popcll(__ballot(beyond));
	if (lane == 0) {
		if (mx) (void)atomicMax(&res->max_bits, mx);
		if (pairs) (void)atomicAdd(&res->n_pairs, (unsigned long long)pairs);
	}
	if (VERTS) {
		if (sample) {
			if (vert_dist) vert_dist[i] = (float)d;
			if (vert_nearest) vert_nearest[i] = best.t;
		}
		if (lane == 0 && n_beyond) (void)atomicAdd(&res->n_verts_beyond, n_beyond);
		return;
	}
	unsigned long long lo[MD_NSUM], hi[MD_NSUM];
#pragma unroll
	for (int k = 0; k < MD_NSUM; ++k) { lo[k] = 0; hi[k] = 0; }
	bool ok = true;
	if (sample) {
		const double dp = d / Q.unit, wd = w * dp;
		ok = md_q(w, &lo[0], &hi[0]);
		ok = md_q(wd, &lo[1], &hi[1]) && ok;
		ok = md_q(wd * dp, &lo[2], &hi[2]) && ok;
#pragma unroll
		for (int k = 0; k < RNB_MESH_DISTANCE_MAX_TAUS; ++k)
			if (Q.tau[k] != 0.0 && d <= Q.tau[k]) { lo[3 + k] = lo[0]; hi[3 + k] = hi[0]; }
	}
	const bool any_bad = __ballot(!ok) != 0ull;
	const uint32_t n_samples = (uint32_t)__popcll(__ballot(sample)), n_deg = (uint32_t)__popcll(__ballot(degenerate));
#pragma unroll
	for (int k = 0; k < MD_NSUM; ++k) {
		const long long sl = wave_sum((long long)lo[k]), sh = wave_sum((long long)hi[k]);
		if (lane == 0) {
			if (sl) (void)atomicAdd(&res->lo[k], (unsigned long long)sl);
			if (sh) (void)atomicAdd(&res->hi[k], (unsigned long long)sh);
		}
	}
	if (lane == 0) {
		if (any_bad) (void)atomicOr(&res->flags, MD_BAD_TERM);
		if (n_samples) (void)atomicAdd(&res->n_samples, (unsigned long long)n_samples);
		if (n_beyond) (void)atomicAdd(&res->n_beyond, (unsigned long long)n_beyond);
		if (n_deg) (void)atomicAdd(&res->n_deg_from, n_deg);
	}
}

} // namespace rnb
