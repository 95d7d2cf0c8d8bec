// kernels_mesh_sparse.cuh — the brick-wise iso-surface extractor of include/rnb_mesh.h (rnb_extract_mesh):
//   k_ms_classify            which bricks the occupancy bitfield keeps (one wavefront per brick)
//   k_ms_mark<WRITE>         which bricks are evaluated (kept, or at +1 of a kept one) and their slots, in brick order
//   k_ms_positions           warped lattice positions of a batch of evaluated bricks (k_lattice_positions' formula, global indices)
//   k_ms_sign                does an evaluated brick see both sides of the threshold in its box grown towards +x, +y, +z
//   k_ms_list                the slots that do, in slot order
//   k_ms_verts<WRITE>        k_mc_verts per brick: only the edges a kept cell uses, the far end looked up in the neighbour brick
//   k_ms_faces<WRITE>        k_mc_faces per brick: corners and edge -> vertex entries looked up through the brick words (this welds brick faces)
//   k_ms_vertex_coords / k_ms_vertex_attr   network inputs at the vertices; logistic of the colour head, normalised SDF gradient
// One 32-bit word per brick: bit 0 kept, bit 1 evaluated, bits 2.. the slot of its values. Everything that numbers a vertex or a triangle is a prefix sum in
// brick-major order (workgroup counts + scan_exclusive + wg_exclusive_256, as the dense path): no atomics. The vertex positions and the corner / edge numbering are
// mesh_common.cuh's (mc_emit_verts, mc_corner, mc_edge), which the dense kernels use too: the two paths agree bit for bit by construction.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh.h"

namespace rnb {

struct MsArgs {
	uint32_t r[3];   // lattice points per axis
	uint32_t nb[3];  // bricks per axis
	uint32_t lb;     // log2 of the brick edge
	uint32_t n_bricks;
	uint32_t* word;         // [n_bricks]
	const uint32_t* list;   // [n_eval] slot -> brick
	const half_t* vals;     // [n_eval << 3 lb] lattice values, brick-local order
	const uint32_t* act;    // [n_eval] 1: the slot keeps an edge table
	const uint32_t* aoff;   // [n_eval] its index among those (exclusive sum of act)
	const uint32_t* alist;  // [n_active] -> slot
	float thresh;
	float sc[3], mn[3];     // lattice point p sits at mn + p * sc in the mesh
};

__device__ __forceinline__ uint32_t ms_brick_of(const MsArgs& a, const uint32_t gx, const uint32_t gy, const uint32_t gz) {
	return (gx >> a.lb) + a.nb[0] * ((gy >> a.lb) + a.nb[1] * (gz >> a.lb));
}
__device__ __forceinline__ uint32_t ms_local_of(const MsArgs& a, const uint32_t gx, const uint32_t gy, const uint32_t gz) {
	const uint32_t m = (1u << a.lb) - 1u;
	return (gx & m) | ((gy & m) << a.lb) | ((gz & m) << (2 * a.lb));
}
// the value of global lattice point g (inside the lattice); false if its brick was not evaluated
__device__ __forceinline__ bool ms_value(const MsArgs& a, const uint32_t gx, const uint32_t gy, const uint32_t gz, float* v) {
	const uint32_t w = a.word[ms_brick_of(a, gx, gy, gz)];
	if (!(w & 2u)) return false;
	*v = h2f(a.vals[((size_t)(w >> 2) << (3 * a.lb)) + ms_local_of(a, gx, gy, gz)]);
	return true;
}

// The cull rule of include/rnb_mesh.h in double precision, statement for statement what tests/mesh_sparse_reference.py computes. bitfield == nullptr: keep all.
__global__ __launch_bounds__(256) void k_ms_classify(const MsArgs a, const double lat_min, const double lat_size, const uint8_t* __restrict__ bitfield) {
	const uint32_t brick = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (brick >= a.n_bricks) return; // (uniform over the wavefront)
	if (!bitfield) { if (lane == 0) a.word[brick] = 1u; return; }
	const uint32_t bc[3] = {brick % a.nb[0], (brick / a.nb[0]) % a.nb[1], brick / (a.nb[0] * a.nb[1])};
	double lo[3], hi[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t first = bc[k] << a.lb, last = min(first + (1u << a.lb), a.r[k]) - 1u;
		lo[k] = lat_min + ((double)first - 1.0) / (double)a.r[k] * lat_size;
		hi[k] = lat_min + ((double)last + 1.0) / (double)a.r[k] * lat_size;
	}
	bool found = false;
	for (uint32_t mip = 0; mip < N_CASCADES; ++mip) {
		const double h = (double)(1u << mip) / (double)GRIDSIZE;
		int i0[3], n[3];
		bool empty = false;
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const double ua = fmin(fmax((lo[k] - 0.5) / h + 0.5 * GRIDSIZE, -1e6), 1e6), ub = fmin(fmax((hi[k] - 0.5) / h + 0.5 * GRIDSIZE, -1e6), 1e6);
			const int f = max((int)ceil(ua) - 1, 0), l = min((int)floor(ub), (int)GRIDSIZE - 1);
			i0[k] = f; n[k] = l - f + 1;
			if (l < f) empty = true;
		}
		if (empty) continue;
		const uint32_t count = (uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2];
		const uint8_t* level = bitfield + (size_t)(GRID_CELLS / 8) * mip;
		for (uint32_t t = lane; t < count; t += 64u) {
			const uint32_t x = i0[0] + t % n[0], y = i0[1] + (t / n[0]) % n[1], z = i0[2] + t / ((uint32_t)n[0] * n[1]);
			// a cell of cascade mip >= 1 inside the cube of cascade mip - 1 is shadowed by it: the march never reads it
			const uint32_t q = GRIDSIZE / 4;
			if (mip && x >= q && x < 3 * q && y >= q && y < 3 * q && z >= q && z < 3 * q) continue;
			const uint32_t idx = morton3D(x, y, z);
			if (level[idx / 8] & (1u << (idx % 8))) found = true;
		}
		if (__ballot(found)) break;
	}
	const bool kept = __ballot(found) != 0;
	if (lane == 0) a.word[brick] = kept ? 1u : 0u;
}

// A brick is evaluated if it or one of the bricks at -1 along any subset of the axes is kept. WRITE = false: per-workgroup counts; WRITE = true: the brick words and
// the slot -> brick list, slots numbered in brick order from wg_offset. (Bit 0 of a word is final before this kernel runs and is written back unchanged.)
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_ms_mark(const MsArgs a, uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset, uint32_t* __restrict__ list) {
	const uint32_t brick = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t eval = 0, self = 0;
	if (brick < a.n_bricks) {
		const uint32_t bc[3] = {brick % a.nb[0], (brick / a.nb[0]) % a.nb[1], brick / (a.nb[0] * a.nb[1])};
		self = a.word[brick] & 1u;
#pragma unroll
		for (uint32_t d = 0; d < 8; ++d) {
			const uint32_t dx = d & 1u, dy = (d >> 1) & 1u, dz = d >> 2;
			if (bc[0] < dx || bc[1] < dy || bc[2] < dz) continue;
			eval |= a.word[(bc[0] - dx) + a.nb[0] * ((bc[1] - dy) + a.nb[1] * (bc[2] - dz))] & 1u;
		}
	}
	uint32_t total;
	const uint32_t local = wg_exclusive_256(eval, &total);
	if (!WRITE) {
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (brick >= a.n_bricks) return;
	const uint32_t slot = wg_offset[blockIdx.x] + local;
	a.word[brick] = self | (eval ? (2u | (slot << 2)) : 0u);
	if (eval) list[slot] = brick;
}

// generate_grid_samples_nerf_uniform (k_lattice_positions' arithmetic) for the n points of the slots from first_slot on. A point of a ragged brick that lies outside the
// lattice is given the index of the lattice's last point on that axis: it is evaluated and never read.
__global__ __launch_bounds__(256) void k_ms_positions(const MsArgs a, const uint32_t first_slot, const uint32_t n, const float lat_min, const float lat_size,
                                                      const float aabb_min, const float aabb_diag, float* __restrict__ out) {
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= n) return;
	const uint32_t brick = a.list[first_slot + (q >> (3 * a.lb))], m = (1u << a.lb) - 1u;
	const uint32_t bc[3] = {brick % a.nb[0], (brick / a.nb[0]) % a.nb[1], brick / (a.nb[0] * a.nb[1])};
	const uint32_t l[3] = {q & m, (q >> a.lb) & m, (q >> (2 * a.lb)) & m};
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t p = min((bc[k] << a.lb) + l[k], a.r[k] - 1u);
		const float inv = 1.f / (float)a.r[k];
		const float w = (float)p * inv * lat_size + lat_min;
		out[(size_t)q * 3 + k] = (w - aabb_min) / aabb_diag; // warp_position
	}
}

// One workgroup per slot: act[slot] = 1 if the available lattice points of the brick's box grown by one step towards +x, +y, +z lie on both sides of the threshold.
__global__ __launch_bounds__(256) void k_ms_sign(const MsArgs a, uint32_t* __restrict__ act) {
	const uint32_t slot = blockIdx.x, brick = a.list[slot], B = 1u << a.lb, E = B + 1u;
	const uint32_t base[3] = {(brick % a.nb[0]) << a.lb, ((brick / a.nb[0]) % a.nb[1]) << a.lb, (brick / (a.nb[0] * a.nb[1])) << a.lb};
	const half_t* own = a.vals + ((size_t)slot << (3 * a.lb));
	int above = 0, below = 0;
	for (uint32_t t = threadIdx.x; t < E * E * E; t += 256u) {
		const uint32_t lx = t % E, ly = (t / E) % E, lz = t / (E * E);
		const uint32_t gx = base[0] + lx, gy = base[1] + ly, gz = base[2] + lz;
		if (gx >= a.r[0] || gy >= a.r[1] || gz >= a.r[2]) continue;
		float v;
		if (lx < B && ly < B && lz < B) v = h2f(own[lx | (ly << a.lb) | (lz << (2 * a.lb))]);
		else if (!ms_value(a, gx, gy, gz, &v)) continue;
		if (v > a.thresh) above = 1; else below = 1;
	}
	above = __syncthreads_or(above);
	below = __syncthreads_or(below);
	if (threadIdx.x == 0) act[slot] = (above && below) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_ms_list(const uint32_t n, const uint32_t* __restrict__ act, const uint32_t* __restrict__ aoff, uint32_t* __restrict__ alist) {
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	if (slot < n && act[slot]) alist[aoff[slot]] = slot;
}

struct MsPoint { uint32_t slot, brick, local, g[3]; bool valid; };
// workgroup -> (active slot, 256 consecutive brick-local points)
__device__ __forceinline__ MsPoint ms_point(const MsArgs& a, uint32_t* as_out) {
	const uint32_t sh = 3 * a.lb - 8; // log2 of the workgroups per brick
	const uint32_t as = blockIdx.x >> sh, m = (1u << a.lb) - 1u;
	MsPoint p;
	p.slot = a.alist[as];
	p.brick = a.list[p.slot];
	p.local = ((blockIdx.x & ((1u << sh) - 1u)) << 8) + threadIdx.x;
	p.g[0] = ((p.brick % a.nb[0]) << a.lb) + (p.local & m);
	p.g[1] = (((p.brick / a.nb[0]) % a.nb[1]) << a.lb) + ((p.local >> a.lb) & m);
	p.g[2] = ((p.brick / (a.nb[0] * a.nb[1])) << a.lb) + (p.local >> (2 * a.lb));
	p.valid = p.g[0] < a.r[0] && p.g[1] < a.r[1] && p.g[2] < a.r[2];
	*as_out = as;
	return p;
}

// k_mc_verts for the lattice points of the bricks that kept an edge table. An edge carries a vertex if its ends lie on different sides of the threshold AND one of the
// (up to four) cells around it belongs to a kept brick; then both ends are corners of that cell, so the far end's brick was evaluated. The position is k_mc_verts' own
// arithmetic (mc_emit_verts) on global lattice coordinates. vidx: [n_active][3][brick^3], MESH_NONE = no vertex.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_ms_verts(const MsArgs a, uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset, float* __restrict__ verts, uint32_t* __restrict__ vidx) {
	uint32_t as;
	const MsPoint p = ms_point(a, &as);
	uint32_t cross = 0;
	float f0 = 0.f, f1[3] = {0.f, 0.f, 0.f};
	if (p.valid) {
		f0 = h2f(a.vals[((size_t)p.slot << (3 * a.lb)) + p.local]);
		const bool in0 = f0 > a.thresh;
		const bool self_kept = (a.word[p.brick] & 1u) != 0;
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			if (p.g[d] + 1 >= a.r[d]) continue;
			const int u = (d + 1) % 3, v = (d + 2) % 3;
			bool used = self_kept && p.g[u] + 1 < a.r[u] && p.g[v] + 1 < a.r[v]; // the cell whose lowest corner is this point
			if (!used) {
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k) {
					const uint32_t du = k & 1u, dv = k >> 1;
					if (p.g[u] < du || p.g[v] < dv) continue;
					uint32_t c[3];
					c[d] = p.g[d]; c[u] = p.g[u] - du; c[v] = p.g[v] - dv;
					if (c[u] + 1 >= a.r[u] || c[v] + 1 >= a.r[v]) continue;
					if (a.word[ms_brick_of(a, c[0], c[1], c[2])] & 1u) used = true;
				}
			}
			if (!used) continue;
			uint32_t e[3] = {p.g[0], p.g[1], p.g[2]};
			e[d] += 1;
			if (!ms_value(a, e[0], e[1], e[2], &f1[d])) continue; // (cannot happen for a used edge)
			if (in0 != (f1[d] > a.thresh)) cross |= 1u << d;
		}
	}
	uint32_t total;
	const uint32_t local = wg_exclusive_256(__popc(cross), &total);
	if (!WRITE) {
		if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
		return;
	}
	if (!p.valid) return;
	uint32_t ids[3];
	mc_emit_verts(p.g, cross, a.thresh, f0, f1, a.sc, a.mn, wg_offset[blockIdx.x] + local, verts, ids);
#pragma unroll
	for (int d = 0; d < 3; ++d) vidx[(((size_t)as * 3 + d) << (3 * a.lb)) + p.local] = ids[d];
}

// k_mc_faces for the cells of the kept bricks among those: the cell whose lowest corner is this lattice point.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_ms_faces(const MsArgs a, const McTable* __restrict__ T, uint32_t* __restrict__ wg_count, const uint32_t* __restrict__ wg_offset,
                                                    const uint32_t* __restrict__ vidx, uint32_t* __restrict__ indices) {
	uint32_t as;
	const MsPoint p = ms_point(a, &as);
	uint32_t mask = 0;
	if (p.valid && (a.word[p.brick] & 1u) && p.g[0] + 1 < a.r[0] && p.g[1] + 1 < a.r[1] && p.g[2] + 1 < a.r[2]) {
		bool all = true;
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c) {
			const McOffset o = mc_corner(c);
			float v;
			if (!ms_value(a, p.g[0] + o.x, p.g[1] + o.y, p.g[2] + o.z, &v)) { all = false; continue; } // (cannot happen: a kept brick's +1 neighbours are evaluated)
			if (v > a.thresh) mask |= 1u << c;
		}
		if (mask == 255u || !all) mask = 0;
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
		const uint32_t hx = p.g[0] + o.x, hy = p.g[1] + o.y, hz = p.g[2] + o.z;
		const uint32_t hs = a.word[ms_brick_of(a, hx, hy, hz)] >> 2; // (evaluated, and it keeps a table: the edge carries a vertex)
		dst[k] = vidx[(((size_t)a.aoff[hs] * 3 + o.axis) << (3 * a.lb)) + ms_local_of(a, hx, hy, hz)];
	}
}

// The network's input at n vertices (Testbed::compute_mesh_vertex_colors, src/testbed_nerf.cu:4193-4216): warped position, dt 0, the direction from the box centre.
__global__ __launch_bounds__(256) void k_ms_vertex_coords(const float* __restrict__ verts, const uint32_t n, const float aabb_min, const float aabb_diag, float* __restrict__ coords) {
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= n) return;
	const float v[3] = {verts[(size_t)q * 3], verts[(size_t)q * 3 + 1], verts[(size_t)q * 3 + 2]};
	const float d[3] = {v[0] - 0.5f, v[1] - 0.5f, v[2] - 0.5f};
	const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	float* c = coords + (size_t)q * 7;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		c[k] = (v[k] - aabb_min) / aabb_diag;
		c[4 + k] = (d[k] / l + 1.f) * 0.5f;
	}
	c[3] = 0.f;
}
// colours: rgb_activation = Logistic of outputs 0..2; normals: outputs 4..6 normalised, zero where the gradient is zero. Either may be null.
__global__ __launch_bounds__(256) void k_ms_vertex_attr(const half_t* __restrict__ net, const uint32_t n, float* __restrict__ colors, float* __restrict__ normals) {
	const uint32_t q = blockIdx.x * 256u + threadIdx.x;
	if (q >= n) return;
	half_t o[16];
	load_out16(net + (size_t)q * 16, o);
	if (colors) {
		colors[(size_t)q * 3 + 0] = logistic(h2f(o[0]));
		colors[(size_t)q * 3 + 1] = logistic(h2f(o[1]));
		colors[(size_t)q * 3 + 2] = logistic(h2f(o[2]));
	}
	if (normals) {
		const Vec3 g = v3(h2f(o[4]), h2f(o[5]), h2f(o[6]));
		const float gn = sqrtf(dot(g, g));
		const Vec3 nr = gn > 0.f ? v3(g.x / gn, g.y / gn, g.z / gn) : v3(0.f, 0.f, 0.f);
		normals[(size_t)q * 3 + 0] = nr.x; normals[(size_t)q * 3 + 1] = nr.y; normals[(size_t)q * 3 + 2] = nr.z;
	}
}

} // namespace rnb
