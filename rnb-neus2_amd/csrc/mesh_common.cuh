// mesh_common.cuh — what the mesh stages share (every kernels_mesh*.cuh file); the only header they include from each other (but for kernels_mesh_visibility.cuh, which
// runs the rasteriser's fill and the cleaner's components and includes both, kernels_mesh_topology.cuh, which unites with the cleaner's cl_find / cl_unite, kernels_mesh_holes.cuh, which reads the topology stage's edge join, kernels_mesh_intersect.cuh, which searches the distance stage's cell lists, and kernels_mesh_project.cuh and kernels_mesh_draw.cuh, which call the baker's and the
// rasteriser's device functions):
//   MESH_WG, MESH_NONE, MESH_BAD_INDEX             the workgroup width of every mesh kernel, the "none" index, the bit k_mesh_validate sets in a stage's flag word
//   k_scan_blocks / k_scan_add, wg_exclusive_256   the prefix sums that number every vertex, triangle, brick and cluster (the driver's scan_exclusive; the count / write kernel pairs)
//   k_mesh_validate                                every index of a triangle list range-checked before any is used as an address, used[v] marked
//   k_compact_verts, k_compact_tris<WRITE>         the stable compaction of a mesh to the part a predicate keeps (the cleaner's ClKeep, the visibility stage's MvKeep,
//                                                  the repair's TpKeep of kernels_mesh_topology.cuh, include/rnb_mesh_topology.h; the driver's MeshCall::compact)
//   wave_sum, wave_group_next                      the sums of the lanes of a wavefront that hold the same key, group by group
//   mc_emit_verts, mc_corner, mc_edge, McTable     the marching-cubes arithmetic and numbering: stated once, so the dense and the sparse extractor agree bit for bit by construction
// Vector loads, stores and atomics only.
#pragma once
#include "common.cuh"

namespace rnb {

constexpr uint32_t MESH_WG = 256;           // threads per workgroup of every mesh kernel but the scans and k_cl_select (1024)
constexpr uint32_t MESH_BAD_INDEX = 1u;     // bit of a stage's flag word: k_mesh_validate met an index >= n_verts
constexpr uint32_t MESH_NONE = 0xFFFFFFFFu; // no vertex on this edge, no component, no cluster
constexpr int MESH_GROUP_ROUNDS = 4;         // groups a wavefront sums with shuffles before the lanes left over issue their own atomics

// Exclusive prefix sums over blocks of 1024 values, in place; block totals to `sums` (one per workgroup).
__global__ __launch_bounds__(1024) void k_scan_blocks(uint32_t* __restrict__ data, const uint64_t n, uint32_t* __restrict__ sums) {
	__shared__ uint32_t wsum[16];
	const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t c = i < n ? data[i] : 0u;
	uint32_t v = c;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(v, off, 64); if ((int)lane >= off) v += t; }
	if (lane == 63) wsum[wave] = v;
	__syncthreads();
	uint32_t before = 0, total = 0;
#pragma unroll
	for (uint32_t q = 0; q < 16; ++q) { if (q < wave) before += wsum[q]; total += wsum[q]; }
	if (i < n) data[i] = before + v - c;
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_scan_add(uint32_t* __restrict__ data, const uint64_t n, const uint32_t* __restrict__ block_offsets) {
	const uint64_t i = (uint64_t)blockIdx.x * 1024 + threadIdx.x;
	if (i < n) data[i] += block_offsets[blockIdx.x];
}

// Workgroup-local exclusive sum of one small count per thread (256 threads); returns the thread's offset, *total = workgroup sum.
static_assert(MESH_WG == 256, "wg_exclusive_256 sums the four wavefronts of a 256-thread workgroup");
__device__ __forceinline__ uint32_t wg_exclusive_256(const uint32_t c, uint32_t* total) {
	__shared__ uint32_t wsum[4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t v = c;
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(v, off, 64); if ((int)lane >= off) v += t; }
	__syncthreads(); // wsum may still be read from a previous call
	if (lane == 63) wsum[wave] = v;
	__syncthreads();
	uint32_t before = 0, tot = 0;
#pragma unroll
	for (uint32_t q = 0; q < 4; ++q) { if (q < wave) before += wsum[q]; tot += wsum[q]; }
	*total = tot;
	return before + v - c;
}

// One thread per triangle: bad_bit is set in *flags if one of its indices is >= nv, else used[] of its corners is marked (every writer writes the same value).
__global__ __launch_bounds__(MESH_WG) void k_mesh_validate(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t nv, uint32_t* __restrict__ used, uint32_t* __restrict__ flags, const uint32_t bad_bit) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt) return;
	const uint32_t a = idx[3 * (size_t)t], b = idx[3 * (size_t)t + 1], c = idx[3 * (size_t)t + 2];
	if (a >= nv || b >= nv || c >= nv) { (void)atomicOr(flags, bad_bit); return; }
	used[a] = 1u; used[b] = 1u; used[c] = 1u;
}

// The stable compaction of a mesh to what a predicate object keeps. KEEP has two device members: vertex(v), whether vertex v is kept, and triangle(idx, t), bit 0 whether
// triangle t is kept and bit 1 whether its winding is flipped (its second and third corner swapped). vmap: the exclusive sums of the kept vertices' flags = their new index.
template <typename KEEP>
__global__ __launch_bounds__(MESH_WG) void k_compact_verts(const KEEP keep, const uint32_t* __restrict__ vmap, const uint32_t nv, const float* __restrict__ verts, const float* __restrict__ colors,
                                                          const float* __restrict__ normals, float* __restrict__ overts, float* __restrict__ ocolors, float* __restrict__ onormals) {
	const uint32_t v = blockIdx.x * MESH_WG + threadIdx.x;
	if (v >= nv || !keep.vertex(v)) return;
	const size_t s = 3 * (size_t)v, d = 3 * (size_t)vmap[v];
	overts[d] = verts[s]; overts[d + 1] = verts[s + 1]; overts[d + 2] = verts[s + 2];
	if (colors) { ocolors[d] = colors[s]; ocolors[d + 1] = colors[s + 1]; ocolors[d + 2] = colors[s + 2]; }
	if (normals) { onormals[d] = normals[s]; onormals[d + 1] = normals[s + 1]; onormals[d + 2] = normals[s + 2]; }
}
// WRITE = false: kept triangles per workgroup; WRITE = true: their renumbered indices from wg_offset (in triangles) on, in input order.
template <bool WRITE, typename KEEP>
__global__ __launch_bounds__(MESH_WG) void k_compact_tris(const uint32_t* __restrict__ idx, const uint32_t nt, const KEEP keep, const uint32_t* __restrict__ vmap, uint32_t* __restrict__ wg_count,
                                                         const uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ oidx) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	const uint32_t f = t < nt ? keep.triangle(idx, t) : 0u;
	uint32_t total;
	const uint32_t local = wg_exclusive_256(f & 1u, &total);
	if (!WRITE) {
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (!(f & 1u)) return;
	const uint32_t a = idx[3 * (size_t)t], b = idx[3 * (size_t)t + 1], c = idx[3 * (size_t)t + 2];
	const size_t d = 3 * ((size_t)wg_offset[blockIdx.x] + local);
	const bool flip = (f & 2u) != 0;
	oidx[d] = vmap[a]; oidx[d + 1] = vmap[flip ? c : b]; oidx[d + 2] = vmap[flip ? b : c];
}

template <typename T> // long long or uint32_t
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
	return x;
}

// One round of grouping the lanes of a wavefront by key: the first valid lane leads, the valid lanes that hold its key are `mine` (mask: all of them) and leave `valid`.
// false: no valid lane is left (uniform over the wavefront). The caller sums what the lanes of the group hold (wave_sum(mine ? x : 0)) and emits it once.
struct WaveGroup { uint32_t key; int leader; uint64_t mask; bool mine; };
__device__ __forceinline__ bool wave_group_next(const uint32_t key, bool& valid, WaveGroup& g) {
	const uint64_t todo = __ballot(valid);
	if (!todo) return false;
	g.leader = __ffsll((unsigned long long)todo) - 1;
	g.key = __shfl(key, g.leader, 64);
	g.mine = valid && key == g.key;
	g.mask = __ballot(g.mine);
	valid = valid && !g.mine;
	return true;
}

// gen_vertices (src/marching_cubes.cu:276-327) for one lattice point p whose values are f0 here and f1[d] one step along axis d: bit d of `cross` says that the edge along
// d carries a vertex, at the linear interpolation of the two values; lattice point q sits at mn + q * sc. The vertices are numbered from `id` on in axis order; ids[d] is
// the edge's vertex or MESH_NONE. (Compiled with -ffp-contract=off; the pragma says so once more where it matters.)
__device__ __forceinline__ void mc_emit_verts(const uint32_t (&p)[3], const uint32_t cross, const float thresh, const float f0, const float (&f1)[3], const float (&sc)[3], const float (&mn)[3],
                                              uint32_t id, float* __restrict__ verts, uint32_t (&ids)[3]) {
#pragma clang fp contract(off)
#pragma unroll
	for (int d = 0; d < 3; ++d) {
		ids[d] = MESH_NONE;
		if (cross & (1u << d)) {
			const float dt = (thresh - f0) / (f1[d] - f0);
			float q[3] = {(float)p[0], (float)p[1], (float)p[2]};
			q[d] += dt;
			verts[(size_t)id * 3 + 0] = q[0] * sc[0] + mn[0];
			verts[(size_t)id * 3 + 1] = q[1] * sc[1] + mn[1];
			verts[(size_t)id * 3 + 2] = q[2] * sc[2] + mn[2];
			ids[d] = id++;
		}
	}
}

struct McTable { int8_t tri[256][40]; uint8_t n[256]; }; // edge ids, 3 per triangle; n = number of indices (the case table of host/mesh.hpp)
// The cell whose lowest corner is a lattice point, in the numbering of src/marching_cubes.cu:261-275. Corner c sits at +(x, y, z): 0 (0,0,0) 1 (1,0,0) 2 (1,1,0) 3 (0,1,0),
// 4..7 the same at z + 1. Edge e is carried by the lattice point at +(x, y, z), along `axis`: edges 0-3 in the z plane, 4-7 in the z + 1 plane, 8-11 along z.
struct McOffset { uint32_t x, y, z, axis; };
__device__ __forceinline__ McOffset mc_corner(const uint32_t c) { return {(c ^ (c >> 1)) & 1u, (c >> 1) & 1u, c >> 2, 0u}; }
__device__ __forceinline__ McOffset mc_edge(const uint32_t e) { return {(0x622u >> e) & 1u, (0xC44u >> e) & 1u, (0x0F0u >> e) & 1u, e < 8u ? (e & 1u) : 2u}; }

} // namespace rnb
