// kernels_mesh_project.cuh — the view projection of include/rnb_mesh_project.h (rnb_mesh_project_views): the texels of the texture baker's atlas coloured from calibrated
// images, each projected into every camera, tested against the rasteriser's depth of that camera, sampled and blended.
//   (k_mesh_validate of mesh_common.cuh comes first: nothing is dereferenced through an index before that kernel has passed)
//   k_mp_setup        one thread per owned texel (the baker's block-major numbering and its texel function, mt_texel / mt_position): p and N of P1, the accumulators cleared
//   k_mp_accumulate   per view, after the rasteriser's fill of that view (raster_fill of the driver: the keys), one thread per owned texel: P2-P5. The camera, the image
//                     and the options are kernel arguments (scalar loads); per texel 36 bytes of p and N, one dependent 8-byte key, four taps of 16 (F32), 8 (U16) or
//                     4 (U8) bytes, and the accumulators read and written back only when the view contributes
//   k_mp_finish       one thread per owned texel: P6, one 16-byte store to color and one 8-byte store to info; a corner texel also writes its corner's (U, V)
// The state of a texel lives in memory between the views as a structure of arrays, so that a wavefront's 64 texels read and write whole cache lines. Only the texel's own
// thread touches it, in view order: no atomics but the four counters of the statistics (integers: their sums do not depend on the order). Operation for operation what
// tests/mesh_project_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters). Vector loads and stores only.
#pragma once
#include "kernels_mesh_raster.cuh"
#include "kernels_mesh_texture.cuh"
#include "../../include/rnb_mesh_project.h"

namespace rnb {


struct MpResult { // written by the kernels, read by the driver
	uint32_t flags, pad; // first: k_mesh_validate is handed its address
	unsigned long long n_texels, n_textured, n_tested, n_occluded;
};
struct MpState { // per owned texel w < n: x[k * n + w]
	float* p;         // [3][n] the position
	double* nrm;      // [3][n] N; all zeros: the texel takes no view (no triangle, or a normal without a length)
	double* acc;      // [4][n] BLEND: A and Q; BEST: q_c and q_a of the best view
	double* w_best;   // [n]
	uint32_t* count;  // [n]
	uint32_t* best;   // [n]
	uint32_t n;
};
struct MpImage { const void* data; uint32_t w, h; };
struct MpParams {
	double min_cos, slack; // slack = 1 + (double) depth_tolerance
	uint32_t power, mode, view, pad;
};

typedef uint32_t mp_u2 __attribute__((ext_vector_type(2)));
typedef unsigned short mp_us4 __attribute__((ext_vector_type(4)));
typedef unsigned char mp_uc4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(MESH_WG) void k_mp_setup(const MtAtlas A, const float* __restrict__ verts, const uint32_t* __restrict__ idx, const float* __restrict__ vnormals, const uint32_t normals,
                                                    const MpState st) {
#pragma clang fp contract(off)
	const uint32_t w = blockIdx.x * MESH_WG + threadIdx.x;
	if (w >= st.n) return;
	const size_t n = st.n;
	float p[3] = {0.f, 0.f, 0.f};
	double N[3] = {0.0, 0.0, 0.0};
	MtTexel t;
	if (mt_texel(A, w, t)) {
		uint32_t vi[3];
		mt_position(A, t, verts, idx, p, vi[0], vi[1], vi[2]);
		double s[3];
		if (normals == RNB_MESH_PROJECT_NORMALS_FACE) { // rule 6 of the rasteriser, the mesh's own order
			double u[3], v[3];
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				const double a = (double)verts[3 * (size_t)vi[0] + k];
				u[k] = (double)verts[3 * (size_t)vi[1] + k] - a;
				v[k] = (double)verts[3 * (size_t)vi[2] + k] - a;
			}
			s[0] = u[1] * v[2] - u[2] * v[1]; s[1] = u[2] * v[0] - u[0] * v[2]; s[2] = u[0] * v[1] - u[1] * v[0];
		} else {
			const double a0 = (double)t.a0, a1 = (double)t.a1, a2 = (double)t.a2;
#pragma unroll
			for (int k = 0; k < 3; ++k)
				s[k] = (a0 * (double)vnormals[3 * (size_t)vi[0] + k] + a1 * (double)vnormals[3 * (size_t)vi[1] + k]) + a2 * (double)vnormals[3 * (size_t)vi[2] + k];
		}
		const double len = __dsqrt_rn(mr_dot(s, s));
		if (len != 0.0 && isfinite(len)) { N[0] = s[0] / len; N[1] = s[1] / len; N[2] = s[2] / len; }
	}
#pragma unroll
	for (int k = 0; k < 3; ++k) { st.p[k * n + w] = p[k]; st.nrm[k * n + w] = N[k]; }
#pragma unroll
	for (int k = 0; k < 4; ++k) st.acc[k * n + w] = 0.0;
	st.w_best[w] = -__builtin_inf();
	st.count[w] = 0u;
	st.best[w] = RNB_MESH_PROJECT_NONE;
}

// One tap: the four channels by the format's rule.
template <int FMT>
__device__ __forceinline__ void mp_tap(const void* __restrict__ img, const size_t at, double c[4]) {
#pragma clang fp contract(off)
	if (FMT == RNB_MESH_PROJECT_FORMAT_F32) {
		const f4 t = reinterpret_cast<const f4*>(img)[at];
		c[0] = (double)t.x; c[1] = (double)t.y; c[2] = (double)t.z; c[3] = (double)t.w;
	} else if (FMT == RNB_MESH_PROJECT_FORMAT_U16) {
		const mp_us4 t = reinterpret_cast<const mp_us4*>(img)[at];
		c[0] = (double)t.x / 65535.0; c[1] = (double)t.y / 65535.0; c[2] = (double)t.z / 65535.0; c[3] = (double)t.w / 65535.0;
	} else {
		const mp_uc4 t = reinterpret_cast<const mp_uc4*>(img)[at];
		c[0] = (double)t.x / 255.0; c[1] = (double)t.y / 255.0; c[2] = (double)t.z / 255.0; c[3] = (double)t.w / 255.0;
	}
}

// P2-P5 of one (texel, view). Returns 0: skipped before the occlusion test; 2: occluded; 1: tested and not occluded (it contributes unless q_a == 0).
template <int FMT>
__device__ __forceinline__ uint32_t mp_view(const MrCamera& cam, const MpState& st, const uint32_t w, const double p[3], const double N[3], const unsigned long long* __restrict__ keys,
                                            const MpImage& img, const MpParams& P) {
#pragma clang fp contract(off)
	const double e[3] = {p[0] - cam.o[0], p[1] - cam.o[1], p[2] - cam.o[2]};
	const double xc = mr_dot(cam.col[0], e), yc = mr_dot(cam.col[1], e), zc = mr_dot(cam.col[2], e);
	if (zc < cam.near) return 0u;
	const double d[3] = {-e[0], -e[1], -e[2]};
	const double c = mr_dot(N, d) / __dsqrt_rn(mr_dot(d, d));
	if (!(c > P.min_cos)) return 0u;
	const double sx = cam.fx * (xc / zc) + cam.cxw, sy = cam.fy * (yc / zc) + cam.cyh;
	if (!isfinite(sx) || !isfinite(sy)) return 0u;
	const double fi = floor(sx), fj = floor(sy), W = (double)cam.w, H = (double)cam.h;
	if (!(fi >= 0.0 && fi < W && fj >= 0.0 && fj < H)) return 0u;
	const unsigned long long key = keys[(size_t)(uint32_t)fj * cam.w + (size_t)(uint32_t)fi]; // inside the image: just checked
	if (key != ~0ull && zc > (double)__uint_as_float((uint32_t)(key >> 32)) * P.slack) return 2u;
	const double u = sx * (double)img.w / W - 0.5, v = sy * (double)img.h / H - 0.5;
	const double fu0 = floor(u), fv0 = floor(v), fu = u - fu0, fv = v - fv0;
	const long long i0 = (long long)fu0, j0 = (long long)fv0, iw1 = (long long)img.w - 1, ih1 = (long long)img.h - 1; // u in [-0.5, iw), v in [-0.5, ih): sx in [0, W), sy in [0, H)
	const size_t x0 = (size_t)min(max(i0, 0ll), iw1), x1 = (size_t)min(max(i0 + 1, 0ll), iw1), y0 = (size_t)min(max(j0, 0ll), ih1), y1 = (size_t)min(max(j0 + 1, 0ll), ih1);
	double t[4][4];
	mp_tap<FMT>(img.data, y0 * img.w + x0, t[0]);
	mp_tap<FMT>(img.data, y0 * img.w + x1, t[1]);
	mp_tap<FMT>(img.data, y1 * img.w + x0, t[2]);
	mp_tap<FMT>(img.data, y1 * img.w + x1, t[3]);
	const double b[4] = {(1.0 - fu) * (1.0 - fv), fu * (1.0 - fv), (1.0 - fu) * fv, fu * fv};
	const double qa = ((b[0] * t[0][3] + b[1] * t[1][3]) + b[2] * t[2][3]) + b[3] * t[3][3];
	if (qa == 0.0) return 1u;
	double qc[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) qc[k] = ((b[0] * (t[0][3] * t[0][k]) + b[1] * (t[1][3] * t[1][k])) + b[2] * (t[2][3] * t[2][k])) + b[3] * (t[3][3] * t[3][k]);
	double g = 1.0;
	for (uint32_t k = 0; k < P.power; ++k) g = g * c;
	const double wv = g * qa;
	const size_t n = st.n;
	st.count[w] += 1u;
	const bool better = wv > st.w_best[w];
	if (better) { st.w_best[w] = wv; st.best[w] = P.view; }
	if (P.mode == RNB_MESH_PROJECT_MODE_BLEND) {
#pragma unroll
		for (int k = 0; k < 3; ++k) st.acc[k * n + w] += g * qc[k];
		st.acc[3 * n + w] += wv;
	} else if (better) {
#pragma unroll
		for (int k = 0; k < 3; ++k) st.acc[k * n + w] = qc[k];
		st.acc[3 * n + w] = qa;
	}
	return 1u;
}

template <int FMT>
__global__ __launch_bounds__(MESH_WG) void k_mp_accumulate(const MrCamera cam, const MpState st, const unsigned long long* __restrict__ keys, const MpImage img, const MpParams P,
                                                         MpResult* __restrict__ res) {
	const uint32_t w = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t code = 0u;
	if (w < st.n) {
		const size_t n = st.n;
		const double N[3] = {st.nrm[w], st.nrm[n + w], st.nrm[2 * n + w]};
		if (N[0] != 0.0 || N[1] != 0.0 || N[2] != 0.0) {
			const double p[3] = {(double)st.p[w], (double)st.p[n + w], (double)st.p[2 * n + w]};
			code = mp_view<FMT>(cam, st, w, p, N, keys, img, P);
		}
	}
	const uint32_t n_tested = wave_sum(code ? 1u : 0u), n_occluded = wave_sum(code >> 1); // (the whole wavefront is here)
	if ((threadIdx.x & 63u) == 0u && n_tested) {
		(void)atomicAdd(&res->n_tested, (unsigned long long)n_tested);
		if (n_occluded) (void)atomicAdd(&res->n_occluded, (unsigned long long)n_occluded);
	}
}

// P6. color and info are zero on entry (the texels no triangle owns stay so); fallback: float[S][S][4] or null.
__global__ __launch_bounds__(MESH_WG) void k_mp_finish(const MtAtlas A, const MpState st, const f4* __restrict__ fallback, float* __restrict__ uv, f4* __restrict__ color, mp_u2* __restrict__ info,
                                                     MpResult* __restrict__ res) {
#pragma clang fp contract(off)
	const uint32_t w = blockIdx.x * MESH_WG + threadIdx.x;
	uint32_t owned = 0u, textured = 0u;
	MtTexel t;
	if (w < st.n && mt_texel(A, w, t)) {
		owned = 1u;
		const size_t n = st.n, at = (size_t)t.y * A.size + t.x;
		const uint32_t count = st.count[w];
		f4 c = f4{0.f, 0.f, 0.f, 1.0f};
		if (count) {
			const double q = st.acc[3 * n + w];
			c = f4{(float)(st.acc[w] / q), (float)(st.acc[n + w] / q), (float)(st.acc[2 * n + w] / q), 1.0f};
			textured = 1u;
		} else if (fallback)
			c = fallback[at];
		color[at] = c;
		info[at] = mp_u2{count, st.best[w]}; // (RNB_MESH_PROJECT_NONE since k_mp_setup when no view contributed)
		const int corner = mt_corner(A, t);
		if (corner >= 0) mt_corner_uv(A, t, corner, uv);
	}
	const uint32_t n_owned = wave_sum(owned), n_textured = wave_sum(textured);
	if ((threadIdx.x & 63u) == 0u && n_owned) {
		(void)atomicAdd(&res->n_texels, (unsigned long long)n_owned);
		if (n_textured) (void)atomicAdd(&res->n_textured, (unsigned long long)n_textured);
	}
}

} // namespace rnb
