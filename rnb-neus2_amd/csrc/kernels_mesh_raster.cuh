// kernels_mesh_raster.cuh — the mesh rasteriser of include/rnb_mesh_raster.h (rnb_mesh_raster): an indexed device mesh into one camera's depth, normal, colour, coverage
// and face maps.
//   (k_mesh_validate of mesh_common.cuh comes first: nothing is dereferenced through an index before that kernel has passed)
//   k_mr_bin<LIST, VIS> one thread per triangle: rules 1-4 up to the pixel box. LIST = false: the triangle is counted in its class, and one whose box holds at most
//                      RNB_MESH_RASTER_SMALL_PIXELS pixels is filled by this thread. LIST = true (launched only when the first pass counted large triangles, with a list of
//                      exactly that length): the large triangles' indices into the list, in any order
//   k_mr_fill_large    one wavefront per large triangle, 64 pixels of its (clamped) box per step: a screen-filling triangle costs no thread more than a few pixels per step
//   k_mr_resolve<VEC>  one thread per pixel: the winner's weights, depth, colour and normal again by the same formulas; the nine channels through LDS, so that with VEC
//                      (the image 16-byte aligned) a workgroup's 256 pixels leave as 16-byte stores
// VIS (k_mr_bin, k_mr_fill_large): the fill as the visibility stage runs it (kernels_mesh_visibility.cuh) -- the same code, and beside the keys and counts every drawn
// triangle's covered and on-mask pixel counts (MrTally). The rasteriser launches VIS = false.
// Per covered (triangle, pixel) one 64-bit atomic minimum on the key and one 32-bit atomic add on the count, results unused (the no-return forms). A minimum and a sum of
// integers: nothing that leaves the call depends on the schedule, the launch shape or which path filled a triangle. Operation for operation what
// tests/mesh_raster_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters). Vector loads, stores and atomics only.
#pragma once
#include "mesh_common.cuh"
#include "../../include/rnb_mesh_raster.h"

namespace rnb {

enum : uint32_t { MR_BEHIND = 0, MR_OUT_OF_RANGE, MR_DEGENERATE, MR_CULLED, MR_OFFSCREEN, MR_SMALL, MR_LARGE, MR_NCLASS };

struct MrResult { // written by the kernels, read by the driver
	uint32_t flags; // first: k_mesh_validate is handed its address
	uint32_t n_class[MR_NCLASS];
	uint32_t n_listed; // cursor of the large list
	uint32_t n_covered, n_back_pixels;
	uint32_t n_unresolved, pad; // pixels whose key names a triangle that the resolve's own setup does not find covering them: always 0, the driver fails the call otherwise
	unsigned long long n_fragments;
};

struct MrCamera {
	double o[3], col[3][3]; // col[k] = column k of the 3x3 block of xform
	double fx, fy, cxw, cyh; // cxw = cx * W, cyh = cy * H
	double near;
	uint32_t w, h, cull, normals;
};
struct MrMesh {
	const float* verts;
	const uint32_t* idx;
	const float* colors;  // or null
	const float* normals; // or null
	uint32_t nt;
};

// A triangle after rules 1-4's setup: (a, b, c) are the swapped triple when the triangle is front-facing.
struct MrTri {
	long long x[3], y[3], a2; // snapped vertices, A2 > 0
	double r[3];              // 1 / zc
	uint32_t v[3];            // vertex numbers, in the order of x, y, r
	int i0, i1, j0, j1;       // pixel box, inclusive
	bool back;                // A2 > 0 before the swap
};

__device__ __forceinline__ double mr_dot(const double x[3], const double y[3]) {
#pragma clang fp contract(off)
	return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}
__device__ __forceinline__ long long mr_edge(const long long px, const long long py, const long long qx, const long long qy, const long long x, const long long y) {
	return (qx - px) * (y - py) - (qy - py) * (x - px);
}
__device__ __forceinline__ bool mr_top_left(const long long dx, const long long dy) { return dy > 0 || (dy == 0 && dx > 0); }

// Rules 1-4 for triangle t up to the pixel box; returns its class. Only MR_SMALL and MR_LARGE leave a complete *out.
__device__ __forceinline__ uint32_t mr_setup(const MrCamera& cam, const MrMesh& m, const uint32_t t, MrTri* out) {
#pragma clang fp contract(off)
	MrTri T;
	double sx[3], sy[3];
	bool front = true;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const uint32_t v = m.idx[3 * (size_t)t + k];
		T.v[k] = v;
		const double e[3] = {(double)m.verts[3 * (size_t)v] - cam.o[0], (double)m.verts[3 * (size_t)v + 1] - cam.o[1], (double)m.verts[3 * (size_t)v + 2] - cam.o[2]};
		const double xc = mr_dot(cam.col[0], e), yc = mr_dot(cam.col[1], e), zc = mr_dot(cam.col[2], e);
		front = front && zc >= cam.near;
		sx[k] = cam.fx * (xc / zc) + cam.cxw;
		sy[k] = cam.fy * (yc / zc) + cam.cyh;
		T.r[k] = 1.0 / zc;
	}
	if (!front) return MR_BEHIND;
	const double lim = (double)(1ll << RNB_MESH_RASTER_MAX_COORD_LOG2);
	bool in_range = true;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const double fxk = floor(sx[k] * 256.0 + 0.5), fyk = floor(sy[k] * 256.0 + 0.5);
		const bool ok = isfinite(sx[k]) && isfinite(sy[k]) && fabs(fxk) <= lim && fabs(fyk) <= lim;
		in_range = in_range && ok;
		T.x[k] = ok ? (long long)fxk : 0ll;
		T.y[k] = ok ? (long long)fyk : 0ll;
	}
	if (!in_range) return MR_OUT_OF_RANGE;
	T.a2 = mr_edge(T.x[0], T.y[0], T.x[1], T.y[1], T.x[2], T.y[2]);
	if (T.a2 == 0) return MR_DEGENERATE;
	T.back = T.a2 > 0;
	if ((cam.cull == RNB_MESH_RASTER_CULL_BACK && T.back) || (cam.cull == RNB_MESH_RASTER_CULL_FRONT && !T.back)) return MR_CULLED;
	if (!T.back) {
		const long long tx = T.x[1], ty = T.y[1]; T.x[1] = T.x[2]; T.y[1] = T.y[2]; T.x[2] = tx; T.y[2] = ty;
		const double tr = T.r[1]; T.r[1] = T.r[2]; T.r[2] = tr;
		const uint32_t tv = T.v[1]; T.v[1] = T.v[2]; T.v[2] = tv;
		T.a2 = -T.a2;
	}
	const long long xmin = min(T.x[0], min(T.x[1], T.x[2])), xmax = max(T.x[0], max(T.x[1], T.x[2]));
	const long long ymin = min(T.y[0], min(T.y[1], T.y[2])), ymax = max(T.y[0], max(T.y[1], T.y[2]));
	const long long i0 = max(0ll, (xmin - 128 + 255) >> 8), i1 = min((long long)cam.w - 1, (xmax - 128) >> 8); // (>> of a negative number floors)
	const long long j0 = max(0ll, (ymin - 128 + 255) >> 8), j1 = min((long long)cam.h - 1, (ymax - 128) >> 8);
	if (i0 > i1 || j0 > j1) return MR_OFFSCREEN;
	T.i0 = (int)i0; T.i1 = (int)i1; T.j0 = (int)j0; T.j1 = (int)j1;
	*out = T;
	return (uint64_t)(i1 - i0 + 1) * (uint64_t)(j1 - j0 + 1) <= RNB_MESH_RASTER_SMALL_PIXELS ? MR_SMALL : MR_LARGE;
}

// Rule 4 for the centre of pixel (i, j): the three weights; true if the pixel is covered.
__device__ __forceinline__ bool mr_cover(const MrTri& T, const int i, const int j, long long w[3]) {
	const long long px = 256ll * i + 128, py = 256ll * j + 128;
	bool in = true;
#pragma unroll
	for (int k = 0; k < 3; ++k) { // w[k] belongs to vertex k: the edge from vertex k + 1 to vertex k + 2
		const int p = (k + 1) % 3, q = (k + 2) % 3;
		w[k] = mr_edge(T.x[p], T.y[p], T.x[q], T.y[q], px, py);
		in = in && (w[k] > 0 || (w[k] == 0 && mr_top_left(T.x[q] - T.x[p], T.y[q] - T.y[p])));
	}
	return in;
}
// Rule 5: z and the l_k of a covered pixel.
__device__ __forceinline__ double mr_depth(const MrTri& T, const long long w[3], double l[3]) {
#pragma clang fp contract(off)
	const double a2 = (double)T.a2;
#pragma unroll
	for (int k = 0; k < 3; ++k) l[k] = (double)w[k] / a2;
	const double iz = (l[0] * T.r[0] + l[1] * T.r[1]) + l[2] * T.r[2];
	return 1.0 / iz;
}
// What the visibility stage (kernels_mesh_visibility.cuh) has the fill write beside the image's keys and counts: per triangle the pixel centres it covers (bit 31:
// the triangle is drawn) and those of them that are on the view's mask. Written by whoever fills the triangle, without atomics. The rasteriser itself (VIS = false)
// hands in an empty one and compiles to what it was.
struct MrTally {
	const uint8_t* mask; // uint8[mh][mw], or null: every pixel is on the mask
	uint32_t mw, mh;
	uint32_t* cov; // [nt], zero on entry
	uint32_t* on;  // [nt], zero on entry
};
constexpr uint32_t MR_DRAWN = 0x80000000u; // bit of MrTally::cov (a count is at most 2^28)
// The mask pixel whose area holds the centre of pixel (i, j) of a w x h view (include/rnb_mesh_visibility.h): non-zero, or no mask.
__device__ __forceinline__ bool mr_on_mask(const MrTally& y, const uint32_t w, const uint32_t h, const uint32_t i, const uint32_t j) {
	if (!y.mask) return true;
	const uint32_t mi = min(y.mw - 1u, (uint32_t)(((2ull * i + 1ull) * y.mw) / (2ull * w))), mj = min(y.mh - 1u, (uint32_t)(((2ull * j + 1ull) * y.mh) / (2ull * h)));
	return y.mask[(size_t)mj * y.mw + mi] != 0;
}

// One (triangle, pixel): the two atomics if the pixel is covered. (i, j) is inside the image: the box was clamped. Returns 0 if the pixel is not covered, else 1, and
// with VIS 3 if it is also on the mask.
template <bool VIS>
__device__ __forceinline__ uint32_t mr_fragment(const MrTri& T, const uint32_t t, const MrCamera& cam, const MrTally& y, const int i, const int j, unsigned long long* __restrict__ keys,
                                                uint32_t* __restrict__ counts) {
	long long w[3];
	if (!mr_cover(T, i, j, w)) return 0u;
	double l[3];
	const float z = (float)mr_depth(T, w, l);
	const size_t p = (size_t)j * cam.w + (size_t)i;
	(void)atomicMin(&keys[p], ((unsigned long long)__float_as_uint(z) << 32) | t);
	(void)atomicAdd(&counts[p], 1u);
	return (VIS && mr_on_mask(y, cam.w, cam.h, (uint32_t)i, (uint32_t)j)) ? 3u : 1u;
}

template <bool LIST, bool VIS>
__global__ __launch_bounds__(MESH_WG) void k_mr_bin(const MrCamera cam, const MrMesh m, unsigned long long* __restrict__ keys, uint32_t* __restrict__ counts, uint32_t* __restrict__ list,
                                                  const uint32_t list_len, MrResult* __restrict__ res, const MrTally y) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	MrTri T;
	const uint32_t cls = t < m.nt ? mr_setup(cam, m, t, &T) : (uint32_t)MR_NCLASS;
	if (LIST) {
		if (cls == MR_LARGE) {
			const uint32_t slot = atomicAdd(&res->n_listed, 1u);
			if (slot < list_len) list[slot] = t; // (always: the list was sized by the counting pass)
		}
		return;
	}
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
	for (uint32_t k = 0; k < MR_NCLASS; ++k) { // one atomic per class and wavefront
		const uint64_t mask = __ballot(cls == k);
		if (mask && lane == (uint32_t)(__ffsll((unsigned long long)mask) - 1)) (void)atomicAdd(&res->n_class[k], (uint32_t)__popcll(mask));
	}
	if (cls != MR_SMALL) return;
	uint32_t n_cov = 0u, n_on = 0u;
	for (int j = T.j0; j <= T.j1; ++j)
		for (int i = T.i0; i <= T.i1; ++i) {
			const uint32_t f = mr_fragment<VIS>(T, t, cam, y, i, j, keys, counts);
			if (VIS) { n_cov += f & 1u; n_on += f >> 1; }
		}
	if (VIS) { y.cov[t] = MR_DRAWN | n_cov; y.on[t] = n_on; }
}

template <bool VIS>
__global__ __launch_bounds__(MESH_WG) void k_mr_fill_large(const MrCamera cam, const MrMesh m, const uint32_t* __restrict__ list, const uint32_t list_len, unsigned long long* __restrict__ keys,
                                                         uint32_t* __restrict__ counts, const MrTally y) {
	const uint32_t entry = blockIdx.x * (MESH_WG / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (entry >= list_len) return;
	const uint32_t t = list[entry];
	if (t >= m.nt) return; // (never: the list holds what k_mr_bin<true> wrote)
	MrTri T;
	if (mr_setup(cam, m, t, &T) != MR_LARGE) return; // (never; every lane of the wavefront computes the same)
	const uint32_t bw = (uint32_t)(T.i1 - T.i0 + 1), n = bw * (uint32_t)(T.j1 - T.j0 + 1); // at most 2^28 pixels
	uint32_t n_cov = 0u, n_on = 0u;
	for (uint32_t q = lane; q < n; q += 64u) {
		const uint32_t f = mr_fragment<VIS>(T, t, cam, y, T.i0 + (int)(q % bw), T.j0 + (int)(q / bw), keys, counts);
		if (VIS) { n_cov += f & 1u; n_on += f >> 1; }
	}
	if (VIS) { // (the whole wavefront is here: the returns above are uniform over it)
		n_cov = wave_sum(n_cov); n_on = wave_sum(n_on);
		if (lane == 0u) { y.cov[t] = MR_DRAWN | n_cov; y.on[t] = n_on; }
	}
}

template <bool VEC>
__global__ __launch_bounds__(MESH_WG) void k_mr_resolve(const MrCamera cam, const MrMesh m, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ counts, float* __restrict__ out,
                                                      uint32_t* __restrict__ faces, MrResult* __restrict__ res) {
#pragma clang fp contract(off)
	__shared__ __attribute__((aligned(16))) float tile[MESH_WG * RNB_MESH_RASTER_CHANNELS];
	const uint32_t n_pix = cam.w * cam.h, first = blockIdx.x * MESH_WG, p = first + threadIdx.x;
	float ch[RNB_MESH_RASTER_CHANNELS];
#pragma unroll
	for (uint32_t k = 0; k < RNB_MESH_RASTER_CHANNELS; ++k) ch[k] = 0.0f;
	uint32_t covered = 0u, back = 0u, frags = 0u, face = RNB_MESH_RASTER_NONE;
	if (p < n_pix) {
		const unsigned long long key = keys[p];
		if (key != ~0ull) {
			face = (uint32_t)key;
			MrTri T;
			long long w[3];
			if (face < m.nt && mr_setup(cam, m, face, &T) >= MR_SMALL && mr_cover(T, (int)(p % cam.w), (int)(p / cam.w), w)) { // (always: the key was written by this triangle at this pixel)
				double l[3], mk[3];
				const double z = mr_depth(T, w, l);
#pragma unroll
				for (int k = 0; k < 3; ++k) mk[k] = (l[k] * T.r[k]) * z;
				if (cam.normals == RNB_MESH_RASTER_NORMALS_FACE) {
					const uint32_t ia = T.v[0], ib = T.back ? T.v[1] : T.v[2], ic = T.back ? T.v[2] : T.v[1]; // the mesh's own order
					double u[3], v[3];
#pragma unroll
					for (int k = 0; k < 3; ++k) {
						const double a = (double)m.verts[3 * (size_t)ia + k];
						u[k] = (double)m.verts[3 * (size_t)ib + k] - a;
						v[k] = (double)m.verts[3 * (size_t)ic + k] - a;
					}
					const double nn[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
					const double len = __dsqrt_rn(mr_dot(nn, nn));
					if (len != 0.0) { ch[0] = (float)(nn[0] / len); ch[1] = (float)(nn[1] / len); ch[2] = (float)(nn[2] / len); }
				} else {
					double s[3];
#pragma unroll
					for (int k = 0; k < 3; ++k)
						s[k] = (mk[0] * (double)m.normals[3 * (size_t)T.v[0] + k] + mk[1] * (double)m.normals[3 * (size_t)T.v[1] + k]) + mk[2] * (double)m.normals[3 * (size_t)T.v[2] + k];
					const double len = __dsqrt_rn(mr_dot(s, s));
					if (len != 0.0) { ch[0] = (float)(s[0] / len); ch[1] = (float)(s[1] / len); ch[2] = (float)(s[2] / len); }
				}
#pragma unroll
				for (int k = 0; k < 3; ++k)
					ch[3 + k] = m.colors ? (float)((mk[0] * (double)m.colors[3 * (size_t)T.v[0] + k] + mk[1] * (double)m.colors[3 * (size_t)T.v[1] + k]) + mk[2] * (double)m.colors[3 * (size_t)T.v[2] + k]) : 1.0f;
				ch[6] = 1.0f;
				ch[7] = (float)z;
				frags = min(counts[p], RNB_MESH_RASTER_MAX_COUNT);
				ch[8] = (float)frags;
				covered = 1u;
				back = T.back ? 1u : 0u;
			} else { // (never: the fill and the resolve run the same code on the same input)
				face = RNB_MESH_RASTER_NONE;
				(void)atomicAdd(&res->n_unresolved, 1u);
			}
		}
		if (faces) faces[p] = face;
	}
	const uint32_t n_cov = wave_sum(covered), n_back = wave_sum(back), n_frag = wave_sum(frags); // (64 * 2^24 fits a word)
	if ((threadIdx.x & 63u) == 0u && n_cov) {
		(void)atomicAdd(&res->n_covered, n_cov);
		if (n_back) (void)atomicAdd(&res->n_back_pixels, n_back);
		(void)atomicAdd(&res->n_fragments, (unsigned long long)n_frag);
	}
	// the workgroup's pixels are contiguous in the image: 9 floats each, written through LDS in 16-byte pieces when the image is aligned (256 * 36 bytes is a multiple of 16)
#pragma unroll
	for (uint32_t k = 0; k < RNB_MESH_RASTER_CHANNELS; ++k) tile[threadIdx.x * RNB_MESH_RASTER_CHANNELS + k] = ch[k];
	__syncthreads();
	const uint32_t n_here = min(MESH_WG, n_pix - first) * RNB_MESH_RASTER_CHANNELS; // floats of this workgroup (first < n_pix: the grid is ceil(n_pix / MESH_WG))
	float* dst = out + (size_t)first * RNB_MESH_RASTER_CHANNELS;
	if (VEC) {
		const uint32_t n4 = n_here / 4u;
		for (uint32_t q = threadIdx.x; q < n4; q += MESH_WG) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(tile)[q];
		for (uint32_t q = n4 * 4u + threadIdx.x; q < n_here; q += MESH_WG) dst[q] = tile[q];
	} else {
		for (uint32_t q = threadIdx.x; q < n_here; q += MESH_WG) dst[q] = tile[q];
	}
}

} // namespace rnb
