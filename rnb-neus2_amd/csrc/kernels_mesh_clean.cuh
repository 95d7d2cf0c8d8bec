// kernels_mesh_clean.cuh — the mesh cleaner of include/rnb_mesh_clean.h (rnb_mesh_clean): connected components of an indexed triangle mesh, keep-largest, outward
// orientation, stable compaction.
//   k_cl_init                   parent[v] = v (beside k_mesh_validate of mesh_common.cuh: nothing is dereferenced through an index before that kernel has passed)
//   k_cl_hook                   union-find: one thread per triangle unites its corners, the larger root hooked under the smaller by compare-and-swap
//   k_cl_flatten                parent[v] = root of v
//   k_cl_roots / k_cl_relabel   roots of used vertices -> component ids by an exclusive sum (ascending label = table order); parent[] becomes the component id per vertex
//   k_cl_sums<TRI>              per-component fixed-point area / volume / triangle count (TRI) or vertex count, summed in the wavefront and the workgroup first
//   k_cl_select                 one workgroup: the component of the greatest area, the kept / flip flag of every component, the totals of the statistics
//   k_cl_vflag, ClKeep          kept vertices: flags -> exclusive sum = the new numbering; the predicate of the shared compaction (k_compact_verts, k_compact_tris<WRITE> of
//                               mesh_common.cuh): renumbered indices, second and third swapped where the component is flipped
// Why the labels do not depend on the schedule: parent[x] <= x always, a compare-and-swap only ever replaces a root r by a smaller root, and a non-root never becomes
// a root again; so when k_cl_hook has finished, the root of a component is its smallest vertex. Path halving only writes an ancestor into a non-root's parent.
// Everything that numbers a vertex or a triangle is a prefix sum, as in kernels_mesh.cuh (mesh_common.cuh). Vector loads, stores and atomics only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_clean.h"

namespace rnb {

constexpr uint32_t CL_BAD_TERM = 2u; // bit of ClResult::flags, beside MESH_BAD_INDEX

struct ClResult { // written by the kernels, read by the driver
	uint32_t flags;     // first: k_mesh_validate is handed its address
	uint32_t best;      // component id KEEP_LARGEST selects
	uint32_t n_kept;
	uint32_t pad;
	long long area_in;
	long long area_out;
};

__device__ __forceinline__ uint32_t cl_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cl_store(uint32_t* p, const uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, with path halving
__device__ __forceinline__ uint32_t cl_find(uint32_t* parent, uint32_t x) {
	for (;;) {
		const uint32_t p = cl_load(parent + x);
		if (p == x) return x;
		const uint32_t g = cl_load(parent + p);
		if (g == p) return p;
		cl_store(parent + x, g); // x is not a root and never will be again: only ancestors are ever written here
		x = g;
	}
}
__device__ __forceinline__ void cl_unite(uint32_t* parent, uint32_t u, uint32_t v) {
	for (;;) {
		u = cl_find(parent, u); v = cl_find(parent, v);
		if (u == v) return;
		if (u < v) { const uint32_t t = u; u = v; v = t; }
		if (atomicCAS(parent + u, u, v) == u) return; // global_atomic_cmpswap, agent scope; lost: u got a parent meanwhile, find again
	}
}

__global__ __launch_bounds__(MESH_WG) void k_cl_init(uint32_t* __restrict__ parent, const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv) parent[v] = v;
}
__global__ __launch_bounds__(MESH_WG) void k_cl_hook(const uint32_t* __restrict__ idx, const uint32_t nt, uint32_t* parent) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt) return;
	const uint32_t a = idx[3 * (size_t)t], b = idx[3 * (size_t)t + 1], c = idx[3 * (size_t)t + 2];
	cl_unite(parent, a, b);
	cl_unite(parent, b, c);
}
__global__ __launch_bounds__(MESH_WG) void k_cl_flatten(uint32_t* parent, const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	// read-only walk: a thread writes its own entry and nothing else, so the last value an entry receives is its root (a halving store of another thread could put a
	// mere ancestor back after it). Entries other threads have already flattened shorten the walk. The roots do not change any more: k_cl_hook has finished.
	uint32_t x = v;
	for (;;) {
		const uint32_t p = cl_load(parent + x);
		if (p == x) break;
		x = p;
	}
	if (x != v) cl_store(parent + v, x);
}
__global__ __launch_bounds__(MESH_WG) void k_cl_roots(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ used, uint32_t* __restrict__ cid, const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v < nv) cid[v] = (used[v] && parent[v] == v) ? 1u : 0u;
}
// parent[v] <- component id of v (MESH_NONE for a vertex no triangle uses); the root writes its label into the table. cid holds the exclusive sums of k_cl_roots' flags.
__global__ __launch_bounds__(MESH_WG) void k_cl_relabel(uint32_t* __restrict__ parent, const uint32_t* __restrict__ used, const uint32_t* __restrict__ cid, rnb_mesh_component* __restrict__ table, const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	if (!used[v]) { parent[v] = MESH_NONE; return; }
	const uint32_t r = parent[v], c = cid[r]; // (a thread writes its own entry only and reads its own entry and cid: no other thread's write is observed)
	if (r == v) table[c].label = v;
	parent[v] = c;
}

// The per-triangle terms of include/rnb_mesh_clean.h, operation for operation what tests/mesh_clean_reference.py computes (this file is compiled with -ffp-contract=off;
// the pragma says so once more where it matters).
__device__ __forceinline__ bool cl_terms(const float* __restrict__ verts, const uint32_t ia, const uint32_t ib, const uint32_t ic, long long* area_q, long long* vol_q) {
#pragma clang fp contract(off)
	const double a[3] = {(double)verts[3 * (size_t)ia], (double)verts[3 * (size_t)ia + 1], (double)verts[3 * (size_t)ia + 2]};
	const double b[3] = {(double)verts[3 * (size_t)ib], (double)verts[3 * (size_t)ib + 1], (double)verts[3 * (size_t)ib + 2]};
	const double c[3] = {(double)verts[3 * (size_t)ic], (double)verts[3 * (size_t)ic + 1], (double)verts[3 * (size_t)ic + 2]};
	const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
	const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
	const double area = 0.5 * __dsqrt_rn((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
	const double m[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
	const double vol = ((a[0] * m[0] + a[1] * m[1]) + a[2] * m[2]) / 6.0;
	const double lim = (double)(1ll << RNB_MESH_Q_TERM_LOG2), scale = (double)(1ll << RNB_MESH_Q_SHIFT);
	if (!(area < lim) || !(fabs(vol) < lim)) { *area_q = 0; *vol_q = 0; return false; } // also catches NaN and infinity
	*area_q = (long long)(area * scale); // a power of two: exact; the conversion truncates
	*vol_q = (long long)(vol * scale);
	return true;
}

__device__ __forceinline__ void cl_emit(rnb_mesh_component* table, const uint32_t c, const long long area, const long long vol, const uint32_t nt, const uint32_t nvx) {
	if (area) (void)atomicAdd((unsigned long long*)&table[c].area_q, (unsigned long long)area);
	if (vol) (void)atomicAdd((unsigned long long*)&table[c].volume_q, (unsigned long long)vol);
	if (nt) (void)atomicAdd(&table[c].n_triangles, nt);
	if (nvx) (void)atomicAdd(&table[c].n_vertices, nvx);
}

// Adds one item per thread (a triangle's terms, or one vertex) to the record of its component. One component usually owns almost every item, so per-item atomics would
// all go to one address. Instead: the lanes of a wavefront that share a component are summed with shuffles (wave_group_next: up to MESH_GROUP_ROUNDS = 4 distinct components per wavefront, the rest falls back
// to one atomic set per lane); a wavefront whose 64 lanes share one component hands its sums to LDS, and if the 4 wavefronts of the workgroup agree the workgroup issues
// ONE set of atomics. Atomics per million triangles of one dominant component: 10^6 / 256 = 3 907 workgroups x 3 (area, volume, count: global_atomic_add_x2 twice and
// global_atomic_add once) = 11.7 k instead of 3 M (derived; not yet checked against a counter pass, profiles/mesh_clean.md); the vertex pass adds 1 per 256 vertices. Integer adds: the sums do not depend on any of this.
// Called by every thread of the workgroup (barriers inside).
__device__ __forceinline__ void cl_accumulate(rnb_mesh_component* __restrict__ table, const uint32_t c, bool valid, const long long area, const long long vol, const uint32_t nt, const uint32_t nvx) {
	__shared__ long long s_area[4], s_vol[4];
	__shared__ uint32_t s_c[4], s_nt[4], s_nv[4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	bool to_lds = false;
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(c, valid, g)) break;
		const long long sa = wave_sum(g.mine ? area : 0ll), sv = wave_sum(g.mine ? vol : 0ll);
		const uint32_t st = wave_sum(g.mine ? nt : 0u), sn = wave_sum(g.mine ? nvx : 0u);
		if (it == 0 && g.mask == ~0ull) { // the whole wavefront is one component
			to_lds = true;
			if (lane == 0) { s_c[wave] = g.key; s_area[wave] = sa; s_vol[wave] = sv; s_nt[wave] = st; s_nv[wave] = sn; }
		} else if ((int)lane == g.leader) cl_emit(table, g.key, sa, sv, st, sn);
	}
	if (valid) cl_emit(table, c, area, vol, nt, nvx);
	if (!to_lds && lane == 0) s_c[wave] = MESH_NONE;
	__syncthreads();
	if (threadIdx.x == 0) {
		if (s_c[0] != MESH_NONE && s_c[0] == s_c[1] && s_c[0] == s_c[2] && s_c[0] == s_c[3])
			cl_emit(table, s_c[0], (s_area[0] + s_area[1]) + (s_area[2] + s_area[3]), (s_vol[0] + s_vol[1]) + (s_vol[2] + s_vol[3]), s_nt[0] + s_nt[1] + s_nt[2] + s_nt[3], s_nv[0] + s_nv[1] + s_nv[2] + s_nv[3]);
		else
			for (uint32_t w = 0; w < 4; ++w) if (s_c[w] != MESH_NONE) cl_emit(table, s_c[w], s_area[w], s_vol[w], s_nt[w], s_nv[w]);
	}
}

// comp: component id per vertex (k_cl_relabel). TRI: n = triangles; else n = vertices.
template <bool TRI>
__global__ __launch_bounds__(MESH_WG) void k_cl_sums(const float* __restrict__ verts, const uint32_t* __restrict__ idx, const uint32_t n, const uint32_t* __restrict__ comp,
                                                  rnb_mesh_component* __restrict__ table, ClResult* __restrict__ res) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t c = MESH_NONE;
	long long area = 0, vol = 0;
	bool valid = false;
	if (i < n) {
		if (TRI) {
			const uint32_t a = idx[3 * (size_t)i], b = idx[3 * (size_t)i + 1], d = idx[3 * (size_t)i + 2];
			c = comp[a];
			valid = true;
			if (!cl_terms(verts, a, b, d, &area, &vol)) atomicOr(&res->flags, CL_BAD_TERM);
		} else {
			c = comp[i];
			valid = c != MESH_NONE;
		}
	}
	cl_accumulate(table, c, valid, area, vol, TRI ? 1u : 0u, TRI ? 0u : 1u);
}

// One workgroup of 1024 threads over the table: which component KEEP_LARGEST selects (greatest area_q; equal: the smallest id = the smallest label), then the kept flag
// of every record, cflags[id] = kept | flip << 1, and the totals.
__global__ __launch_bounds__(1024) void k_cl_select(rnb_mesh_component* __restrict__ table, const uint32_t n_comp, const uint32_t keep, const uint32_t orient,
                                                   uint32_t* __restrict__ cflags, ClResult* __restrict__ res) {
	__shared__ long long s_a[1024], s_sum[1024];
	__shared__ uint32_t s_id[1024];
	const uint32_t t = threadIdx.x;
	long long best_a = -1, sum = 0;
	uint32_t best_id = MESH_NONE;
	for (uint32_t i = t; i < n_comp; i += 1024u) { // ascending ids per thread: the first of equal areas stays
		const long long a = table[i].area_q;
		sum += a;
		if (a > best_a) { best_a = a; best_id = i; }
	}
	s_a[t] = best_a; s_id[t] = best_id; s_sum[t] = sum;
	__syncthreads();
	for (uint32_t w = 512; w >= 1; w >>= 1) {
		if (t < w) {
			s_sum[t] += s_sum[t + w];
			if (s_a[t + w] > s_a[t] || (s_a[t + w] == s_a[t] && s_id[t + w] < s_id[t])) { s_a[t] = s_a[t + w]; s_id[t] = s_id[t + w]; }
		}
		__syncthreads();
	}
	const uint32_t best = s_id[0];
	const long long area_in = s_sum[0];
	__syncthreads();
	long long kept_area = 0;
	uint32_t n_kept = 0;
	for (uint32_t i = t; i < n_comp; i += 1024u) {
		const bool kept = keep == RNB_MESH_KEEP_ALL || i == best;
		table[i].kept = kept ? 1u : 0u;
		cflags[i] = (kept ? 1u : 0u) | ((kept && orient == RNB_MESH_ORIENT_OUTWARD && table[i].volume_q < 0) ? 2u : 0u);
		if (kept) { kept_area += table[i].area_q; n_kept += 1u; }
	}
	s_sum[t] = kept_area; s_id[t] = n_kept;
	__syncthreads();
	for (uint32_t w = 512; w >= 1; w >>= 1) {
		if (t < w) { s_sum[t] += s_sum[t + w]; s_id[t] += s_id[t + w]; }
		__syncthreads();
	}
	if (t == 0) { res->best = best; res->n_kept = s_id[0]; res->area_in = area_in; res->area_out = s_sum[0]; }
}

__global__ __launch_bounds__(MESH_WG) void k_cl_vflag(const uint32_t* __restrict__ comp, const uint32_t* __restrict__ cflags, uint32_t* __restrict__ vmap, const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	const uint32_t c = comp[v];
	vmap[v] = (c != MESH_NONE && (cflags[c] & 1u)) ? 1u : 0u;
}
// What MeshCall::compact keeps of the cleaner's input (k_compact_verts, k_compact_tris of mesh_common.cuh): the vertices and triangles of the kept components, the
// triangles of a flipped component with their second and third corner swapped.
struct ClKeep {
	const uint32_t* comp;   // component id per vertex (k_cl_relabel)
	const uint32_t* cflags; // kept | flip << 1 per component (k_cl_select)
	__device__ __forceinline__ bool vertex(const uint32_t v) const { const uint32_t c = comp[v]; return c != MESH_NONE && (cflags[c] & 1u); }
	__device__ __forceinline__ uint32_t triangle(const uint32_t* __restrict__ idx, const uint32_t t) const { return cflags[comp[idx[3 * (size_t)t]]]; }
};

} // namespace rnb
