// kernels_mesh_texture.cuh — the texture baker of include/rnb_mesh_texture.h (rnb_mesh_bake_texture): the model's albedo, SDF-gradient normal and position at every
// texel of a per-triangle atlas of a device mesh.
//   (k_mesh_validate of mesh_common.cuh comes first: nothing is dereferenced through an index before that kernel has passed)
//   k_mt_texels   one thread per owned texel of a batch (block-major numbering, n_blocks * b * b of them): its triangle and integer weights, the position in double
//                 precision, the position map's 16-byte store, the 7-float network input by the arithmetic of k_ms_vertex_coords; a corner texel also writes its
//                 corner's (U, V), so the atlas needs neither a host loop nor an upload
//   k_mt_maps     one thread per texel of the batch: the 16 half outputs of the network (two 16-byte loads) into one 16-byte store per map, by the arithmetic of
//                 k_ms_vertex_attr
// A texel is computed from its own number alone and stored to its own address: neither the batch size nor the launch shape can change a bit of the result. Operation for
// operation what tests/mesh_texture_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters).
// Vector loads and stores only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_texture.h"

namespace rnb {


struct MtAtlas {
	uint32_t size, block, bpr; // S, b, blocks per row
	uint32_t n_tris;
	uint32_t n_texels;         // n_blocks * b * b: the owned texels, numbered block-major (block, then row, then column)
};

// Owned texel w -> its place in the texture and in its triangle. false: the texel belongs to no triangle (the upper half of the last block of an odd mesh).
struct MtTexel { uint32_t x, y, tri; int a0, a1, a2; };
__device__ __forceinline__ bool mt_texel(const MtAtlas& A, const uint32_t w, MtTexel& t) {
	const uint32_t b = A.block, bb = b * b, k = w / bb, r = w - k * bb, j = r / b, i = r - j * b;
	t.x = (k % A.bpr) * b + i;
	t.y = (k / A.bpr) * b + j;
	const bool upper = i + j > b - 1u;
	t.tri = 2u * k + (upper ? 1u : 0u);
	const int n = (int)b - 3, ii = (int)(upper ? b - 1u - i : i), jj = (int)(upper ? b - 1u - j : j);
	t.a0 = n - ii - jj; t.a1 = ii; t.a2 = jj;
	return t.tri < A.n_tris;
}

// The position of an owned texel, the header's formula, and (i0, i1, i2) its triangle's vertices (range-checked by k_mesh_validate). Shared with the view projection
// (kernels_mesh_project.cuh), whose texels are these.
__device__ __forceinline__ void mt_position(const MtAtlas& A, const MtTexel& t, const float* __restrict__ verts, const uint32_t* __restrict__ idx, float v[3], uint32_t& i0, uint32_t& i1, uint32_t& i2) {
#pragma clang fp contract(off)
	i0 = idx[3 * (size_t)t.tri]; i1 = idx[3 * (size_t)t.tri + 1]; i2 = idx[3 * (size_t)t.tri + 2];
	const double a0 = (double)t.a0, a1 = (double)t.a1, a2 = (double)t.a2, n = (double)((int)A.block - 3);
#pragma unroll
	for (int k = 0; k < 3; ++k)
		v[k] = (float)(((a0 * (double)verts[3 * (size_t)i0 + k] + a1 * (double)verts[3 * (size_t)i1 + k]) + a2 * (double)verts[3 * (size_t)i2 + k]) / n);
}
// Which corner of its triangle an owned texel is (one weight n, the others 0: they add up to n), or -1; and the corner's (U, V) by the layout's formula.
__device__ __forceinline__ int mt_corner(const MtAtlas& A, const MtTexel& t) {
	const int nn = (int)A.block - 3;
	return (t.a1 == 0 && t.a2 == 0) ? 0 : ((t.a1 == nn && t.a2 == 0) ? 1 : ((t.a1 == 0 && t.a2 == nn) ? 2 : -1));
}
__device__ __forceinline__ void mt_corner_uv(const MtAtlas& A, const MtTexel& t, const int corner, float* __restrict__ uv) {
#pragma clang fp contract(off)
	float* o = uv + ((size_t)t.tri * 3 + (size_t)corner) * 2;
	o[0] = (float)(((double)t.x + 0.5) / (double)A.size);
	o[1] = (float)(1.0 - ((double)t.y + 0.5) / (double)A.size);
}

// Texels w0 .. w0 + nb - 1. uv: float[n_tris][3][2], written by the three corner texels of every triangle. position (or null): the position map. coords (or null): the network input of the batch, 7 floats per texel; a texel without a triangle gets
// the input of the point (0, 0, 0), so that the batch stays dense (its output is not used).
__global__ __launch_bounds__(MESH_WG) void k_mt_texels(const MtAtlas A, const float* __restrict__ verts, const uint32_t* __restrict__ idx, const uint32_t w0, const uint32_t nb,
                                                     const float aabb_min, const float aabb_diag, float* __restrict__ uv, f4* __restrict__ position, float* __restrict__ coords) {
#pragma clang fp contract(off)
	const uint32_t q = blockIdx.x * MESH_WG + threadIdx.x;
	if (q >= nb) return;
	MtTexel t;
	float v[3] = {0.f, 0.f, 0.f};
	if (mt_texel(A, w0 + q, t)) {
		uint32_t i0, i1, i2;
		mt_position(A, t, verts, idx, v, i0, i1, i2);
		if (position) position[(size_t)t.y * A.size + t.x] = f4{v[0], v[1], v[2], 1.0f};
		const int corner = mt_corner(A, t);
		if (corner >= 0) mt_corner_uv(A, t, corner, uv);
	}
	if (!coords) return;
	// k_ms_vertex_coords, expression for expression, for a position inside the scene's box: a corner texel gets the network input of its vertex
	const float d[3] = {v[0] - 0.5f, v[1] - 0.5f, v[2] - 0.5f};
	const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	float* c = coords + (size_t)q * 7;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		c[k] = fminf(fmaxf((v[k] - aabb_min) / aabb_diag, 0.f), 1.f); // (a gutter texel may lie outside the box: the hash grid is indexed by this; inside it nothing changes)
		c[4 + k] = (d[k] / l + 1.f) * 0.5f;
	}
	c[3] = 0.f;
}

// albedo: rgb_activation = Logistic of outputs 0..2; normal: outputs 4..6 normalised, zeros where the gradient is zero (k_ms_vertex_attr). Either may be null.
__global__ __launch_bounds__(MESH_WG) void k_mt_maps(const MtAtlas A, const half_t* __restrict__ net, const uint32_t w0, const uint32_t nb, f4* __restrict__ albedo, f4* __restrict__ normal) {
	const uint32_t q = blockIdx.x * MESH_WG + threadIdx.x;
	if (q >= nb) return;
	MtTexel t;
	if (!mt_texel(A, w0 + q, t)) return;
	half_t o[16];
	load_out16(net + (size_t)q * 16, o);
	const size_t at = (size_t)t.y * A.size + t.x;
	if (albedo) albedo[at] = f4{logistic(h2f(o[0])), logistic(h2f(o[1])), logistic(h2f(o[2])), 1.0f};
	if (normal) {
		const Vec3 g = v3(h2f(o[4]), h2f(o[5]), h2f(o[6]));
		const float gn = sqrtf(dot(g, g));
		const Vec3 nr = gn > 0.f ? v3(g.x / gn, g.y / gn, g.z / gn) : v3(0.f, 0.f, 0.f);
		normal[at] = f4{nr.x, nr.y, nr.z, 1.0f};
	}
}

} // namespace rnb
