// kernels_mesh.cuh — iso-surface extraction on the device:
//   k_lattice_positions + k_half_to_float   get_density_on_grid / generate_grid_samples_nerf_uniform   src/testbed_nerf.cu:541-553, 4218-4269
//   k_mc_verts<WRITE>                       gen_vertices                                               src/marching_cubes.cu:276-327
//   k_mc_faces<WRITE>                       gen_faces                                                  src/marching_cubes.cu:377-430, 676-717
// The reference numbers vertices and triangles with atomicAdd counters (any order). Here both are numbered by prefix sums in
// lattice order -- point index ascending, then axis x, y, z; cell index ascending, then table order -- which is the order of the
// host loop in host/mesh.hpp: the two produce identical buffers (tests/test_gpu_mesh.py), and a mesh is reproducible from run to
// run. The case table is the one host/mesh.hpp generates (same polygon loops as the published table in all 256 cases). The prefix sums, the interpolation arithmetic and
// the corner / edge numbering are mesh_common.cuh's, shared with the sparse extractor.
#pragma once
#include "mesh_common.cuh"

namespace rnb {

struct McArgs {
	const float* density; // [rx * ry * rz], x fastest
	uint32_t rx, ry, rz;
	float thresh;
	float sc[3], mn[3]; // lattice point p sits at mn + p * sc
};

// gen_vertices: one vertex per lattice edge whose ends lie on different sides of the threshold, at the linear interpolation
// of the two values. WRITE = false: per-workgroup counts; WRITE = true: positions + the edge -> vertex index grid [3][res^3]
// (MESH_NONE: no vertex), numbered from wg_offset.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_mc_verts(const McArgs a, uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset, float* __restrict__ verts, uint32_t* __restrict__ vidx) {
	const uint64_t res2 = (uint64_t)a.rx * a.ry, res3 = res2 * a.rz;
	const uint64_t idx = (uint64_t)blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t cross = 0; // bit a: the edge from this point along axis a carries a vertex
	float f0 = 0.f, f1[3] = {0.f, 0.f, 0.f};
	uint32_t p[3] = {0, 0, 0};
	if (idx < res3) {
		p[0] = (uint32_t)(idx % a.rx); p[1] = (uint32_t)((idx / a.rx) % a.ry); p[2] = (uint32_t)(idx / res2);
		f0 = a.density[idx];
		const bool in0 = f0 > a.thresh;
		const uint64_t step[3] = {1, a.rx, res2};
		const uint32_t lim[3] = {a.rx - 1, a.ry - 1, a.rz - 1};
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			if (p[d] >= lim[d]) continue;
			f1[d] = a.density[idx + step[d]];
			if (in0 != (f1[d] > a.thresh)) cross |= 1u << d;
		}
	}
	uint32_t total;
	const uint32_t local = wg_exclusive_256(__popc(cross), &total);
	if (!WRITE) {
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (idx >= res3) return;
	uint32_t ids[3];
	mc_emit_verts(p, cross, a.thresh, f0, f1, a.sc, a.mn, wg_offset[blockIdx.x] + local, verts, ids);
#pragma unroll
	for (int d = 0; d < 3; ++d) vidx[idx + res3 * d] = ids[d];
}

// gen_faces: the cell whose lowest corner is this lattice point.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_mc_faces(const McArgs a, const McTable* __restrict__ T, uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset,
                                                    const uint32_t* __restrict__ vidx, uint32_t* __restrict__ indices) {
	const uint64_t res2 = (uint64_t)a.rx * a.ry, res3 = res2 * a.rz;
	const uint64_t idx = (uint64_t)blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t mask = 0;
	if (idx < res3) {
		const uint32_t x = (uint32_t)(idx % a.rx), y = (uint32_t)((idx / a.rx) % a.ry), z = (uint32_t)(idx / res2);
		if (x + 1 < a.rx && y + 1 < a.ry && z + 1 < a.rz) {
#pragma unroll
			for (uint32_t c = 0; c < 8; ++c) {
				const McOffset o = mc_corner(c);
				if (a.density[idx + o.x + o.y * (uint64_t)a.rx + o.z * res2] > a.thresh) mask |= 1u << c;
			}
			if (mask == 255u) mask = 0;
		}
	}
	const uint32_t n = mask ? T->n[mask] : 0u;
	uint32_t total;
	const uint32_t local = wg_exclusive_256(n, &total);
	if (!WRITE) {
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (!n) return;
	uint32_t* dst = indices + (size_t)wg_offset[blockIdx.x] + local;
	for (uint32_t k = 0; k < n; ++k) {
		const McOffset o = mc_edge((uint32_t)T->tri[mask][k]);
		dst[k] = vidx[idx + o.x + o.y * (uint64_t)a.rx + o.z * res2 + res3 * o.axis];
	}
}

// generate_grid_samples_nerf_uniform (src/testbed_nerf.cu:541-553) for lattice points [first, first + n): warped positions.
__global__ void k_lattice_positions(const uint64_t first, const uint32_t n, const uint32_t rx, const uint32_t ry, const uint32_t rz, const float lat_min, const float lat_size,
                                    const float aabb_min, const float aabb_diag, float* __restrict__ out) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= n) return;
	const uint64_t i = first + q;
	const uint32_t p[3] = {(uint32_t)(i % rx), (uint32_t)((i / rx) % ry), (uint32_t)(i / ((uint64_t)rx * ry))};
	const uint32_t r[3] = {rx, ry, rz};
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float inv = 1.f / (float)r[k];
		const float w = (float)p[k] * inv * lat_size + lat_min;
		out[(size_t)q * 3 + k] = (w - aabb_min) / aabb_diag; // warp_position
	}
}
__global__ void k_half_to_float(const half_t* __restrict__ src, float* __restrict__ dst, const uint32_t n) {
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q < n) dst[q] = h2f(src[q]);
}

} // namespace rnb
