// kernels_mesh_topology.cuh — the topology stage of include/rnb_mesh_topology.h (rnb_mesh_topology, rnb_mesh_repair): which half-edges share an edge, which triangles
// a vertex set, which vertices a position; patches and their orientability through the double cover; the repair's flags for the shared compaction.
//   TpEdgeKeys, TpTriKeys, TpPosKeys      the three groupings as keys of three words, recomputed from the index (or vertex) buffer whenever they are needed
//   k_tp_count / k_tp_max_load / k_tp_fill<KEYS>   the hash join they share: items counted per bucket, the fullest bucket (the guard), the bucket lists filled
//                                          through an atomic cursor (the driver's tp_join scans in between); order inside a bucket: arbitrary, and nothing reads it
//   k_tp_edges                             one thread per half-edge walks its bucket: faces on the edge, faces in its direction, the mate; the edge's lowest half-edge
//                                          counts the edge; manifold edges unite the double cover, boundary edges the boundary components (cl_unite, the cleaner's)
//   k_tp_tris<REPAIR>                      one thread per triangle walks its bucket: duplicates and folded pairs (census), who stays (repair)
//   k_tp_weld, k_tp_finite, k_tp_rewrite   one thread per vertex: the lowest vertex at its position; the finiteness check; the indices rewritten
//   k_tp_patches, k_tp_flip                roots of the double cover -> patches, unorientable ones, the sheet sizes; the flip bit of every triangle
//   k_tp_relabel, k_tp_comp_sums, k_tp_boundary_roots, k_tp_table_finish   the component table
//   k_tp_degenerate, k_tp_mark, k_tp_vertex_map, TpKeep   the repair's bookkeeping and its predicate for k_compact_verts / k_compact_tris (mesh_common.cuh)
// Everything a walk forms is an order-free function of the set of items with its key (a count, a minimum, the other one of two), so no result depends on the hash,
// the bucket count or the fill order. Sums into a component or a patch are integer atomics, the lanes of a wavefront that hit one record summed first (tp_add).
// Vector loads, stores and atomics only.
#pragma once
#include "kernels_mesh_clean.cuh"
#include "../../include/rnb_mesh_topology.h"

namespace rnb {

constexpr uint32_t TP_NOT_FINITE = 2u; // bit of TpResult::flags, beside MESH_BAD_INDEX

struct TpResult { // written by the kernels, read by the driver; zeroed before a call
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t max_bucket;
	uint32_t n_verts_used, n_degenerate, n_edges, n_boundary_edges, n_manifold_edges, n_nonmanifold_edges, n_inconsistent_edges, max_faces_on_edge;
	uint32_t n_duplicate_tris, n_folded_pairs, n_patches, n_unorientable_patches, n_boundary_components;
	uint32_t n_welded, n_dropped, n_flipped;
};

struct TpKey { uint32_t a, b, c; };
__device__ __forceinline__ bool tp_equal(const TpKey& x, const TpKey& y) { return x.a == y.a && x.b == y.b && x.c == y.c; }
__device__ __forceinline__ uint64_t tp_mix(uint64_t x) { // the finaliser of splitmix64
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
	x ^= x >> 27; x *= 0x94D049BB133111EBull;
	return x ^ (x >> 31);
}
// bucket of a key among 2^log2 (log2 = 4 .. 30): the top bits of the mixed words
__device__ __forceinline__ uint32_t tp_bucket(const TpKey& k, const uint32_t log2) {
	return (uint32_t)(tp_mix(tp_mix(((uint64_t)k.a << 32) | k.b) + k.c) >> (64u - log2));
}

// A triangle of the working mesh: its corners, and whether it takes part (it is still there and not degenerate). alive: one word per triangle, or null = all.
struct TpTris {
	const uint32_t* idx;
	const uint32_t* alive;
	__device__ __forceinline__ bool load(const uint32_t t, uint32_t& a, uint32_t& b, uint32_t& c) const {
		a = idx[3 * (size_t)t]; b = idx[3 * (size_t)t + 1]; c = idx[3 * (size_t)t + 2];
		return (!alive || (alive[t] & 1u)) && a != b && b != c && a != c;
	}
};
// half-edge h = 3t + k: {min, max} of its ends; *from = the index it leaves (the direction)
struct TpEdgeKeys {
	TpTris tris;
	__device__ __forceinline__ bool key(const uint32_t h, TpKey& k, uint32_t* from = nullptr) const {
		const uint32_t t = h / 3u, e = h - 3u * t;
		uint32_t a, b, c;
		if (!tris.load(t, a, b, c)) return false;
		const uint32_t p = e == 0u ? a : (e == 1u ? b : c), q = e == 0u ? b : (e == 1u ? c : a);
		k.a = p < q ? p : q; k.b = p < q ? q : p; k.c = 0u;
		if (from) *from = p;
		return true;
	}
};
// triangle t: its ascending triple; *odd = its winding
struct TpTriKeys {
	TpTris tris;
	__device__ __forceinline__ bool key(const uint32_t t, TpKey& k, uint32_t* odd = nullptr) const {
		uint32_t a, b, c;
		if (!tris.load(t, a, b, c)) return false;
		if (odd) *odd = ((a > b ? 1u : 0u) + (a > c ? 1u : 0u) + (b > c ? 1u : 0u)) & 1u;
		const uint32_t lo = min(a, min(b, c)), hi = max(a, max(b, c));
		k.a = lo; k.b = a ^ b ^ c ^ lo ^ hi; k.c = hi;
		return true;
	}
};
// used vertex v: the words of its coordinates, -0 as +0 (the coordinates are finite by then: equal words = equal numbers)
struct TpPosKeys {
	const uint32_t* words; // the vertex buffer
	const uint32_t* used;
	__device__ __forceinline__ bool key(const uint32_t v, TpKey& k) const {
		if (!used[v]) return false;
		const uint32_t x = words[3 * (size_t)v], y = words[3 * (size_t)v + 1], z = words[3 * (size_t)v + 2];
		k.a = x == 0x80000000u ? 0u : x; k.b = y == 0x80000000u ? 0u : y; k.c = z == 0x80000000u ? 0u : z;
		return true;
	}
};

// ---- the hash join ----
template <typename KEYS>
__global__ __launch_bounds__(MESH_WG) void k_tp_count(const KEYS keys, const uint32_t n, const uint32_t log2, uint32_t* __restrict__ offs) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	if (i < n && keys.key(i, k)) (void)atomicAdd(offs + tp_bucket(k, log2), 1u);
}
// the fullest bucket, for the guard: one atomic per wavefront
__global__ __launch_bounds__(MESH_WG) void k_tp_max_load(const uint32_t* __restrict__ offs, const uint32_t n_buckets, TpResult* __restrict__ res) {
	const uint32_t b = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t m = b < n_buckets ? offs[b] : 0u;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off, 64));
	if ((threadIdx.x & 63u) == 0u && m) (void)atomicMax(&res->max_bucket, m);
}
// offs: the exclusive sums of the counts on entry; every bucket's cursor runs to its end, so that afterwards bucket b is items[b ? offs[b - 1] : 0 .. offs[b])
template <typename KEYS>
__global__ __launch_bounds__(MESH_WG) void k_tp_fill(const KEYS keys, const uint32_t n, const uint32_t log2, uint32_t* __restrict__ offs, uint32_t* __restrict__ items) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	if (i < n && keys.key(i, k)) items[atomicAdd(offs + tp_bucket(k, log2), 1u)] = i;
}
struct TpJoin { // a filled table
	const uint32_t* offs;
	const uint32_t* items;
	uint32_t log2;
	__device__ __forceinline__ void range(const TpKey& k, uint32_t& lo, uint32_t& hi) const {
		const uint32_t b = tp_bucket(k, log2);
		lo = b ? offs[b - 1u] : 0u; hi = offs[b];
	}
};

// Adds x0 .. x3 (one item per thread; those of an invalid lane are ignored) to the four consecutive words at base + key * stride: the lanes of the wavefront that
// hold one key are summed first (up to MESH_GROUP_ROUNDS keys per wavefront; what is left issues its own atomics). Called by whole wavefronts.
__device__ __forceinline__ void tp_emit(uint32_t* p, const uint32_t x0, const uint32_t x1, const uint32_t x2, const uint32_t x3) {
	if (x0) (void)atomicAdd(p, x0);
	if (x1) (void)atomicAdd(p + 1, x1);
	if (x2) (void)atomicAdd(p + 2, x2);
	if (x3) (void)atomicAdd(p + 3, x3);
}
__device__ __forceinline__ void tp_add(uint32_t* base, const uint32_t stride, const uint32_t key, bool valid, const uint32_t x0, const uint32_t x1, const uint32_t x2, const uint32_t x3) {
	const uint32_t lane = threadIdx.x & 63u;
	for (int it = 0; it < MESH_GROUP_ROUNDS; ++it) {
		WaveGroup g;
		if (!wave_group_next(key, valid, g)) break;
		const uint32_t s0 = wave_sum(g.mine ? x0 : 0u), s1 = wave_sum(g.mine ? x1 : 0u), s2 = wave_sum(g.mine ? x2 : 0u), s3 = wave_sum(g.mine ? x3 : 0u);
		if ((int)lane == g.leader) tp_emit(base + (size_t)g.key * stride, s0, s1, s2, s3);
	}
	if (valid) tp_emit(base + (size_t)key * stride, x0, x1, x2, x3);
}
// one mesh-wide counter: summed over the wavefront, one atomic
__device__ __forceinline__ void tp_count(uint32_t* counter, const uint32_t x) {
	const uint32_t s = wave_sum(x);
	if ((threadIdx.x & 63u) == 0u && s) (void)atomicAdd(counter, s);
}

// ---- components (the cleaner's labels: k_cl_init, k_cl_hook, k_cl_flatten, k_cl_roots before this) ----
static_assert(sizeof(rnb_mesh_topology_component) == 40 && offsetof(rnb_mesh_topology_component, n_edges) == 8 && offsetof(rnb_mesh_topology_component, n_boundary_edges) == 16,
              "tp_add addresses the records of the table as ten words");
constexpr uint32_t TP_REC = sizeof(rnb_mesh_topology_component) / 4u;
// parent[v] <- component id of v (MESH_NONE for an unused vertex); the root writes its label. cid: the exclusive sums of k_cl_roots' flags.
__global__ __launch_bounds__(MESH_WG) void k_tp_relabel(uint32_t* __restrict__ parent, const uint32_t* __restrict__ used, const uint32_t* __restrict__ cid, rnb_mesh_topology_component* __restrict__ table,
                                                      const uint32_t nv) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	if (!used[v]) { parent[v] = MESH_NONE; return; }
	const uint32_t r = parent[v], c = cid[r];
	if (r == v) table[c].label = v;
	parent[v] = c;
}
// n_vertices per component and n_verts_used
__global__ __launch_bounds__(MESH_WG) void k_tp_comp_sums(const uint32_t* __restrict__ comp, const uint32_t nv, rnb_mesh_topology_component* __restrict__ table, TpResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	const uint32_t c = v < nv ? comp[v] : MESH_NONE;
	const bool valid = c != MESH_NONE;
	tp_add((uint32_t*)table, TP_REC, c, valid, 0u, 1u, 0u, 0u); // words 0 .. 3: label, n_vertices, n_edges, n_triangles
	tp_count(&res->n_verts_used, valid ? 1u : 0u);
}

// ---- triangles by vertex set ----
// REPAIR = false (census): n_degenerate, n_duplicate_tris, n_folded_pairs, n_triangles per component. REPAIR = true: stay[t] = whether triangle t is still there
// after step 3 (mode = RNB_MESH_DUPLICATES_FIRST or CANCEL); a degenerate triangle that is still there stays.
template <bool REPAIR>
__global__ __launch_bounds__(MESH_WG) void k_tp_tris(const TpTriKeys keys, const uint32_t nt, const TpJoin join, const uint32_t mode, uint32_t* __restrict__ stay, const uint32_t* __restrict__ comp,
                                                  rnb_mesh_topology_component* __restrict__ table, TpResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	uint32_t odd = 0;
	const bool valid = t < nt && keys.key(t, k, &odd);
	uint32_t n_even = 0, n_odd = 0, first = t, before = 0; // before: members of t's winding with a lower number
	if (valid) {
		uint32_t lo, hi;
		join.range(k, lo, hi);
		for (uint32_t s = lo; s < hi; ++s) {
			const uint32_t u = join.items[s];
			TpKey ku;
			uint32_t odd_u = 0;
			if (!keys.key(u, ku, &odd_u) || !tp_equal(k, ku)) continue;
			n_odd += odd_u; n_even += 1u - odd_u;
			first = min(first, u);
			if (odd_u == odd && u < t) ++before;
		}
	}
	if (REPAIR) {
		if (t >= nt) return;
		const bool there = !keys.tris.alive || (keys.tris.alive[t] & 1u);
		bool s = there;
		if (valid) {
			if (mode == RNB_MESH_DUPLICATES_FIRST) s = first == t;
			else { // CANCEL
				const uint32_t mine = odd ? n_odd : n_even, other = odd ? n_even : n_odd;
				s = mine > other && before < mine - other;
			}
		}
		stay[t] = s ? 1u : 0u;
		return;
	}
	tp_count(&res->n_degenerate, (t < nt && !valid) ? 1u : 0u);
	tp_count(&res->n_duplicate_tris, (valid && first != t) ? 1u : 0u);
	tp_count(&res->n_folded_pairs, (valid && first == t) ? min(n_even, n_odd) : 0u);
	tp_add((uint32_t*)table, TP_REC, valid ? comp[k.a] : MESH_NONE, valid, 0u, 0u, 0u, 1u);
}

// ---- half-edges by edge ----
// One thread per half-edge. n_faces / n_same / mate: optional outputs. cover: the double cover's parents (two nodes per triangle, k_cl_init before); bparent / bmark
// (census only, may be null): the boundary components' parents over the vertices and the mark of a vertex on a boundary edge. comp / table (census only, may be null).
__global__ __launch_bounds__(MESH_WG) void k_tp_edges(const TpEdgeKeys keys, const uint32_t n_half, const TpJoin join, uint32_t* __restrict__ n_faces, uint32_t* __restrict__ n_same, uint32_t* __restrict__ mate,
                                                   uint32_t* cover, uint32_t* bparent, uint32_t* __restrict__ bmark, const uint32_t* __restrict__ comp, rnb_mesh_topology_component* __restrict__ table,
                                                   TpResult* __restrict__ res) {
	const uint32_t h = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	uint32_t from = 0;
	const bool valid = h < n_half && keys.key(h, k, &from);
	uint32_t faces = 0, same = 0, first = h, other = MESH_NONE;
	if (valid) {
		uint32_t lo, hi;
		join.range(k, lo, hi);
		for (uint32_t s = lo; s < hi; ++s) {
			const uint32_t g = join.items[s];
			TpKey kg;
			uint32_t from_g = 0;
			if (!keys.key(g, kg, &from_g) || !tp_equal(k, kg)) continue;
			++faces;
			if (from_g == from) ++same;
			first = min(first, g);
			if (g != h) other = g;
		}
	}
	if (h < n_half) {
		if (n_faces) n_faces[h] = faces;
		if (n_same) n_same[h] = same;
		if (mate) mate[h] = faces == 2u ? other : MESH_NONE;
	}
	const bool counts = valid && first == h; // the edge is counted by its lowest half-edge
	if (counts && faces == 2u) { // manifold: the two sheets of the double cover
		const uint32_t t = h / 3u, u = other / 3u, x = same == 2u ? 1u : 0u;
		cl_unite(cover, 2u * t, 2u * u + x);
		cl_unite(cover, 2u * t + 1u, 2u * u + (1u - x));
	}
	if (counts && faces == 1u && bparent) {
		bmark[k.a] = 1u; bmark[k.b] = 1u; // (every writer writes the same value)
		cl_unite(bparent, k.a, k.b);
	}
	if (!res) return;
	const uint32_t e = counts ? 1u : 0u, bd = (counts && faces == 1u) ? 1u : 0u, nm = (counts && faces >= 3u) ? 1u : 0u, inc = (counts && faces == 2u && same == 2u) ? 1u : 0u;
	tp_count(&res->n_edges, e);
	tp_count(&res->n_boundary_edges, bd);
	tp_count(&res->n_manifold_edges, (counts && faces == 2u) ? 1u : 0u);
	tp_count(&res->n_nonmanifold_edges, nm);
	tp_count(&res->n_inconsistent_edges, inc);
	uint32_t m = counts ? faces : 0u;
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor(m, off, 64));
	if ((threadIdx.x & 63u) == 0u && m) (void)atomicMax(&res->max_faces_on_edge, m);
	if (table) {
		const uint32_t c = counts ? comp[k.a] : MESH_NONE;
		tp_add((uint32_t*)table, TP_REC, c, counts, 0u, 0u, e, 0u);          // words 0 .. 3: n_edges is the third
		tp_add((uint32_t*)table + 4, TP_REC, c, counts && (bd | nm | inc), bd, nm, inc, 0u); // words 4 .. 7: n_boundary_edges, n_nonmanifold_edges, n_inconsistent_edges, n_patches
	}
}

// ---- patches (cover flattened: k_cl_flatten over its 2 * nt nodes) ----
// The smallest node of a patch is 2 * t0 of its lowest-numbered triangle t0, and the smallest node of its other sheet is 2 * t0 + 1: so t0 is the one triangle of
// the patch with cover[2t] == 2t, every triangle finds t0 as cover[2t] >> 1, and "root(2t) > root(2t+1)" is "cover[2t] is odd". sheet (repair, may be null): two
// words per triangle, zero on entry; those of t0 receive the patch's size and how many of its triangles have an odd cover[2t].
__global__ __launch_bounds__(MESH_WG) void k_tp_patches(const TpTris tris, const uint32_t nt, const uint32_t* __restrict__ cover, uint32_t* __restrict__ sheet, const uint32_t* __restrict__ comp,
                                                     rnb_mesh_topology_component* __restrict__ table, TpResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t a = 0, b, c;
	const bool valid = t < nt && tris.load(t, a, b, c);
	const uint32_t r0 = valid ? cover[2 * (size_t)t] : 0u, r1 = valid ? cover[2 * (size_t)t + 1] : 1u;
	const bool root = valid && r0 == 2u * t;
	tp_count(&res->n_patches, root ? 1u : 0u);
	tp_count(&res->n_unorientable_patches, (root && r0 == r1) ? 1u : 0u);
	if (table) tp_add((uint32_t*)table + 4, TP_REC, root ? comp[a] : MESH_NONE, root, 0u, 0u, 0u, 1u);
	if (sheet) tp_add(sheet, 2u, r0 >> 1, valid && r0 != r1, 1u, r0 & 1u, 0u, 0u);
}
// flags[t] |= 2 where triangle t is flipped: it is on the sheet that flips fewer (the odd one unless more than half of the patch is on it)
__global__ __launch_bounds__(MESH_WG) void k_tp_flip(const TpTris tris, const uint32_t nt, const uint32_t* __restrict__ cover, const uint32_t* __restrict__ sheet, uint32_t* flags /* = tris.alive */,
                                                  TpResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t a, b, c;
	bool flip = false;
	if (t < nt && tris.load(t, a, b, c)) {
		const uint32_t r0 = cover[2 * (size_t)t], r1 = cover[2 * (size_t)t + 1];
		if (r0 != r1) {
			const uint32_t t0 = r0 >> 1, size = sheet[2 * (size_t)t0], n_odd = sheet[2 * (size_t)t0 + 1];
			flip = ((r0 & 1u) != 0u) != (2ull * n_odd > size);
		}
	}
	if (flip) flags[t] |= 2u; // (a thread writes its own entry; tris reads bit 0 only)
	tp_count(&res->n_flipped, flip ? 1u : 0u);
}

// the boundary components: the marked vertices that are still their own parent (a root is only ever hooked under a smaller marked vertex)
__global__ __launch_bounds__(MESH_WG) void k_tp_boundary_roots(const uint32_t* __restrict__ bparent, const uint32_t* __restrict__ bmark, const uint32_t nv, TpResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	tp_count(&res->n_boundary_components, (v < nv && bmark[v] && bparent[v] == v) ? 1u : 0u);
}
__global__ __launch_bounds__(MESH_WG) void k_tp_table_finish(rnb_mesh_topology_component* __restrict__ table, const uint32_t n_comp) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i >= n_comp) return;
	const rnb_mesh_topology_component r = table[i];
	const int32_t euler = (int32_t)(r.n_vertices - r.n_edges + r.n_triangles), twice = 2 - euler;
	const bool surface = !r.n_boundary_edges && !r.n_nonmanifold_edges && !r.n_inconsistent_edges && r.n_patches == 1u && twice >= 0 && !(twice & 1);
	table[i].euler = euler;
	table[i].genus = surface ? twice / 2 : -1;
}

// ---- the repair ----
// a used vertex with a coordinate that is not finite (exponent all ones) sets TP_NOT_FINITE
__global__ __launch_bounds__(MESH_WG) void k_tp_finite(const uint32_t* __restrict__ words, const uint32_t* __restrict__ used, const uint32_t nv, TpResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv || !used[v]) return;
	const uint32_t x = words[3 * (size_t)v], y = words[3 * (size_t)v + 1], z = words[3 * (size_t)v + 2], e = 0x7F800000u;
	if ((x & e) == e || (y & e) == e || (z & e) == e) (void)atomicOr(&res->flags, TP_NOT_FINITE);
}
// rep[v] = the lowest used vertex at v's position (v itself for an unused one)
__global__ __launch_bounds__(MESH_WG) void k_tp_weld(const TpPosKeys keys, const uint32_t nv, const TpJoin join, uint32_t* __restrict__ rep, TpResult* __restrict__ res) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	TpKey k;
	uint32_t first = v;
	if (v < nv && keys.key(v, k)) {
		uint32_t lo, hi;
		join.range(k, lo, hi);
		for (uint32_t s = lo; s < hi; ++s) {
			const uint32_t u = join.items[s];
			TpKey ku;
			if (u < first && keys.key(u, ku) && tp_equal(k, ku)) first = u;
		}
	}
	if (v < nv) rep[v] = first;
	tp_count(&res->n_welded, (v < nv && first != v) ? 1u : 0u);
}
__global__ __launch_bounds__(MESH_WG) void k_tp_rewrite(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ rep, const uint32_t n, uint32_t* __restrict__ out) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (i < n) out[i] = rep[idx[i]];
}
// flags[t] = 1 unless triangle t is degenerate and those are dropped
__global__ __launch_bounds__(MESH_WG) void k_tp_degenerate(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t drop, uint32_t* __restrict__ flags, TpResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	bool gone = false;
	if (t < nt) {
		const uint32_t a = idx[3 * (size_t)t], b = idx[3 * (size_t)t + 1], c = idx[3 * (size_t)t + 2];
		gone = drop && (a == b || b == c || a == c);
		flags[t] = gone ? 0u : 1u;
	}
	tp_count(&res->n_degenerate, gone ? 1u : 0u);
}
// flags[t] &= stay[t]; n_dropped counts what went
__global__ __launch_bounds__(MESH_WG) void k_tp_apply(const uint32_t* __restrict__ stay, const uint32_t nt, uint32_t* __restrict__ flags, TpResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	const bool gone = t < nt && (flags[t] & 1u) && !stay[t];
	if (gone) flags[t] = 0u;
	tp_count(&res->n_dropped, gone ? 1u : 0u);
}
// vkeep[v] = 1 for the corners of the triangles that are still there (vkeep zeroed before)
__global__ __launch_bounds__(MESH_WG) void k_tp_mark(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ flags, const uint32_t nt, uint32_t* __restrict__ vkeep) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt || !(flags[t] & 1u)) return;
	vkeep[idx[3 * (size_t)t]] = 1u; vkeep[idx[3 * (size_t)t + 1]] = 1u; vkeep[idx[3 * (size_t)t + 2]] = 1u;
}
// out[v] = the output index of what input vertex v became (rep: null without weld), MESH_NONE if that is not in the output
__global__ __launch_bounds__(MESH_WG) void k_tp_vertex_map(const uint32_t* __restrict__ rep, const uint32_t* __restrict__ vkeep, const uint32_t* __restrict__ vmap, const uint32_t nv, uint32_t* __restrict__ out) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv) return;
	const uint32_t r = rep ? rep[v] : v;
	out[v] = vkeep[r] ? vmap[r] : MESH_NONE;
}
// What MeshCall::compact keeps of the repair's working mesh: the marked vertices; the triangles by their flag word (bit 0 kept, bit 1 flipped).
struct TpKeep {
	const uint32_t* vkeep;
	const uint32_t* flags;
	__device__ __forceinline__ bool vertex(const uint32_t v) const { return vkeep[v] != 0u; }
	__device__ __forceinline__ uint32_t triangle(const uint32_t* __restrict__, const uint32_t t) const { return flags[t]; }
};

} // namespace rnb
