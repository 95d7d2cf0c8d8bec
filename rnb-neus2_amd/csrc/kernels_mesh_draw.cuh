// kernels_mesh_draw.cuh — the textured draw of include/rnb_mesh_draw.h (rnb_mesh_draw_textured): a device mesh with a texture atlas into one camera, in the rasteriser's
// channel layout.
//   (k_mesh_validate of mesh_common.cuh and the rasteriser's fill, k_mr_bin and k_mr_fill_large of kernels_mesh_raster.cuh, come first, launched by the driver as the
//   rasteriser launches them: this file has no fill of its own)
//   k_md_resolve<FILTER, COLOR, NORMAL, VEC>  one thread per pixel: the winner's setup, weights and depth again by the rasteriser's device functions (mr_setup, mr_cover,
//                      mr_depth: shared, not copied), the texture coordinate (T2), the texel coordinate and the taps (T3: one 16-byte load per tap and map), colour
//                      (T4) and normal (T5); the nine channels through LDS as k_mr_resolve writes them, so that with VEC (the image 16-byte aligned) a workgroup's 256
//                      pixels leave as 16-byte stores. COLOR, NORMAL: which maps were given (at least one). The normal and the colour of rule 6 are computed only on
//                      the paths that show them (draw_rule6_normal, draw_rule6_colour: rule 6 as k_mr_resolve states it, which is not touched).
// The three counters of the statistics are packed into one word per lane (each is 0 or 1, a wavefront's sums are at most 64: 8 bits each), summed by one wavefront
// reduction and added once per wavefront and non-zero counter. Integers: their sums do not depend on the order. Operation for operation what
// tests/mesh_draw_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters). Vector loads, stores and
// atomics only.
#pragma once
#include "kernels_mesh_raster.cuh"
#include "../../include/rnb_mesh_draw.h"

namespace rnb {

struct DrawTexture {
	const float* uv;     // [nt][3][2]
	const float* color;  // [S][S][4] or null
	const float* normal; // [S][S][4] or null
	uint32_t size;
};
struct DrawResult { uint32_t n_bad_uv, n_fallback, n_unowned, pad; }; // written by the kernel, read by the driver

// Rule 6's normal of the winner T (the mesh's own order for FACE; the swapped triple's weights mk for VERTEX): zeros if it has no length.
__device__ __forceinline__ void draw_rule6_normal(const MrCamera& cam, const MrMesh& m, const MrTri& T, const double mk[3], float out[3]) {
#pragma clang fp contract(off)
	double s[3];
	if (cam.normals == RNB_MESH_RASTER_NORMALS_FACE) {
		const uint32_t ia = T.v[0], ib = T.back ? T.v[1] : T.v[2], ic = T.back ? T.v[2] : T.v[1];
		double u[3], v[3];
#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const double a = (double)m.verts[3 * (size_t)ia + k];
			u[k] = (double)m.verts[3 * (size_t)ib + k] - a;
			v[k] = (double)m.verts[3 * (size_t)ic + k] - a;
		}
		s[0] = u[1] * v[2] - u[2] * v[1]; s[1] = u[2] * v[0] - u[0] * v[2]; s[2] = u[0] * v[1] - u[1] * v[0];
	} else {
#pragma unroll
		for (int k = 0; k < 3; ++k)
			s[k] = (mk[0] * (double)m.normals[3 * (size_t)T.v[0] + k] + mk[1] * (double)m.normals[3 * (size_t)T.v[1] + k]) + mk[2] * (double)m.normals[3 * (size_t)T.v[2] + k];
	}
	const double len = __dsqrt_rn(mr_dot(s, s));
	out[0] = out[1] = out[2] = 0.0f;
	if (len != 0.0) { out[0] = (float)(s[0] / len); out[1] = (float)(s[1] / len); out[2] = (float)(s[2] / len); }
}
__device__ __forceinline__ void draw_rule6_colour(const MrMesh& m, const MrTri& T, const double mk[3], float out[3]) {
#pragma clang fp contract(off)
#pragma unroll
	for (int k = 0; k < 3; ++k)
		out[k] = m.colors ? (float)((mk[0] * (double)m.colors[3 * (size_t)T.v[0] + k] + mk[1] * (double)m.colors[3 * (size_t)T.v[1] + k]) + mk[2] * (double)m.colors[3 * (size_t)T.v[2] + k]) : 1.0f;
}

// T3's sample of one map at taps at[0..n), weights b: channels 0-2 to s; true if a tap of non-zero weight has alpha 0.
template <int FILTER>
__device__ __forceinline__ bool draw_sample(const float* __restrict__ map, const size_t at[4], const double b[4], double s[3]) {
#pragma clang fp contract(off)
	if (FILTER == RNB_MESH_DRAW_FILTER_NEAREST) {
		const f4 t = reinterpret_cast<const f4*>(map)[at[0]];
		s[0] = (double)t.x; s[1] = (double)t.y; s[2] = (double)t.z;
		return t.w == 0.0f;
	}
	f4 t[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) t[k] = reinterpret_cast<const f4*>(map)[at[k]];
	s[0] = ((b[0] * (double)t[0].x + b[1] * (double)t[1].x) + b[2] * (double)t[2].x) + b[3] * (double)t[3].x;
	s[1] = ((b[0] * (double)t[0].y + b[1] * (double)t[1].y) + b[2] * (double)t[2].y) + b[3] * (double)t[3].y;
	s[2] = ((b[0] * (double)t[0].z + b[1] * (double)t[1].z) + b[2] * (double)t[2].z) + b[3] * (double)t[3].z;
	bool unowned = false;
#pragma unroll
	for (int k = 0; k < 4; ++k) unowned = unowned || (b[k] != 0.0 && t[k].w == 0.0f);
	return unowned;
}

template <int FILTER, bool COLOR, bool NORMAL, bool VEC>
__global__ __launch_bounds__(MESH_WG) void k_md_resolve(const MrCamera cam, const MrMesh m, const DrawTexture tex, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ counts,
                                                      float* __restrict__ out, uint32_t* __restrict__ faces, MrResult* __restrict__ res, DrawResult* __restrict__ dres) {
#pragma clang fp contract(off)
	__shared__ __attribute__((aligned(16))) float tile[MESH_WG * RNB_MESH_RASTER_CHANNELS];
	const uint32_t n_pix = cam.w * cam.h, first = blockIdx.x * MESH_WG, p = first + threadIdx.x;
	float ch[RNB_MESH_RASTER_CHANNELS];
#pragma unroll
	for (uint32_t k = 0; k < RNB_MESH_RASTER_CHANNELS; ++k) ch[k] = 0.0f;
	uint32_t covered = 0u, back = 0u, frags = 0u, face = RNB_MESH_RASTER_NONE, tally = 0u; // tally: bad uv | fallback << 8 | unowned << 16
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
				// T2: the corners' (U, V) in the order of T.v: the mesh's corners 0, 1, 2, or 0, 2, 1 after the swap
				const float* uv = tex.uv + 6 * (size_t)face;
				const uint32_t cb = T.back ? 1u : 2u, cc = T.back ? 2u : 1u;
				const double U = (mk[0] * (double)uv[0] + mk[1] * (double)uv[2 * cb]) + mk[2] * (double)uv[2 * cc];
				const double V = (mk[0] * (double)uv[1] + mk[1] * (double)uv[2 * cb + 1]) + mk[2] * (double)uv[2 * cc + 1];
				// T3
				const double S = (double)tex.size;
				double x = U * S - 0.5, y = (1.0 - V) * S - 0.5;
				bool rule6_normal = !NORMAL;
				if (!isfinite(x) || !isfinite(y)) {
					tally = 1u;
					rule6_normal = true; // (the colour stays zeros where a colour map was given)
				} else {
					x = fmin(fmax(x, -1.0), S); y = fmin(fmax(y, -1.0), S);
					const long long last = (long long)tex.size - 1;
					size_t at[4];
					double b[4] = {1.0, 0.0, 0.0, 0.0};
					if (FILTER == RNB_MESH_DRAW_FILTER_NEAREST) {
						const long long i = min(max((long long)floor(x + 0.5), 0ll), last), j = min(max((long long)floor(y + 0.5), 0ll), last);
						at[0] = at[1] = at[2] = at[3] = (size_t)j * tex.size + (size_t)i;
					} else {
						const double fi = floor(x), fj = floor(y), fu = x - fi, fv = y - fj;
						const long long i0 = (long long)fi, j0 = (long long)fj;
						const size_t x0 = (size_t)min(max(i0, 0ll), last), x1 = (size_t)min(max(i0 + 1, 0ll), last), y0 = (size_t)min(max(j0, 0ll), last), y1 = (size_t)min(max(j0 + 1, 0ll), last);
						at[0] = y0 * tex.size + x0; at[1] = y0 * tex.size + x1; at[2] = y1 * tex.size + x0; at[3] = y1 * tex.size + x1;
						b[0] = (1.0 - fu) * (1.0 - fv); b[1] = fu * (1.0 - fv); b[2] = (1.0 - fu) * fv; b[3] = fu * fv;
					}
					bool unowned = false;
					if (COLOR) { // T4
						double s[3];
						unowned = draw_sample<FILTER>(tex.color, at, b, s);
						ch[3] = (float)s[0]; ch[4] = (float)s[1]; ch[5] = (float)s[2];
					}
					if (NORMAL) { // T5
						double s[3];
						const bool un = draw_sample<FILTER>(tex.normal, at, b, s);
						if (!COLOR) unowned = un;
						const double len = __dsqrt_rn(mr_dot(s, s));
						if (isfinite(len) && len > 0.0) { ch[0] = (float)(s[0] / len); ch[1] = (float)(s[1] / len); ch[2] = (float)(s[2] / len); }
						else { rule6_normal = true; tally |= 1u << 8; }
					}
					if (unowned) tally |= 1u << 16;
				}
				if (rule6_normal) draw_rule6_normal(cam, m, T, mk, ch);
				if (!COLOR) draw_rule6_colour(m, T, mk, ch + 3);
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
	tally = wave_sum(tally); // three sums of at most 64, 8 bits apart
	if ((threadIdx.x & 63u) == 0u && n_cov) {
		(void)atomicAdd(&res->n_covered, n_cov);
		if (n_back) (void)atomicAdd(&res->n_back_pixels, n_back);
		(void)atomicAdd(&res->n_fragments, (unsigned long long)n_frag);
		if (tally & 0xFFu) (void)atomicAdd(&dres->n_bad_uv, tally & 0xFFu);
		if ((tally >> 8) & 0xFFu) (void)atomicAdd(&dres->n_fallback, (tally >> 8) & 0xFFu);
		if (tally >> 16) (void)atomicAdd(&dres->n_unowned, tally >> 16);
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
