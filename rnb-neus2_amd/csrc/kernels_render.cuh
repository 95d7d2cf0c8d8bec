// kernels_render.cuh — the inference tracer: normal / albedo / opacity / depth maps of one camera (Testbed::NerfTracer, src/testbed_nerf.cu:2499-2770).
//   k_render_init       init_rays_with_payload_kernel_nerf   testbed_nerf.cu:2308-2432   one thread per pixel of the tile
//   k_render_compact    compact_kernel_nerf                  testbed_nerf.cu:2283-2306   prefix-sum slots (scan_exclusive) instead of an atomicAdd counter
//   k_render_march      generate_next_nerf_network_inputs    testbed_nerf.cu:822-879     up to n occupied steps per ray, sample-major NerfCoordinate records
//   k_render_composite  composite_kernel_nerf                testbed_nerf.cu:881-1118    NeuS alpha (alpha_terms, as the loss), Normals + Depth modes in one pass
//   k_render_write      shade_kernel_nerf                    testbed_nerf.cu:2248-2281   the tile's pixels into the caller's [H][W][9] image, 16-byte stores
// Rays are kept in ray order through every round (exclusive prefix sums), and a ray's march and composite read nothing but the ray itself, the occupancy
// bitfield and the network outputs of its own samples: the image does not depend on the round schedule or the tiling, and two renders are bit-identical.
#pragma once
#include "kernels_ray.cuh"
#include "../../include/rnb_render.h"

namespace rnb {

// One ray in flight: 80 bytes, five 16-byte words.
struct __attribute__((aligned(16))) RenderRay {
	float o[3], t;        // origin, distance marched so far
	float d[3];           // unit direction
	uint32_t pix;         // pixel index within the tile
	float n[3], w;        // sum weight * unit normal, sum weight (the reference's rgba.w)
	float a[3], wmax;     // sum weight * albedo, the largest weight so far
	float depth;          // camera-forward depth of the max-weight sample
	uint32_t nsamp;       // samples composited
	uint32_t nstep;       // samples the last march wrote for this ray
	uint32_t exhausted;   // the last march ended early: the ray left the box or reached RNB_MAX_STEPS
};
static_assert(sizeof(RenderRay) == 80, "RenderRay is five 16-byte words");

constexpr uint32_t RENDER_RES_FLOATS = 12; // per pixel in the tile's result buffer: the 9 output channels + 3 padding (three 16-byte stores)
constexpr uint32_t RENDER_MAX_N = 8;       // network samples per ray of the tile that one round may write (the workspace holds that many; MAX_STEPS_INBETWEEN_COMPACTION, testbed_nerf.cu:58)
constexpr uint32_t RENDER_ROUND_MAX = 64;  // the most samples one ray marches in a round

struct RenderArgs {
	ViewDev view;         // the camera (normal / albedo pointers unused)
	SceneAabb A;
	const uint8_t* bitfield; // null: every cell is occupied
	float near_distance, min_transmittance;
	uint32_t apply_no_albedo;
	uint32_t p0, nt;      // the tile: pixels [p0, p0 + nt) of the image, row-major
	float fwd[3];         // the camera's forward axis (column 2 of the camera matrix)
};

__device__ __forceinline__ void store_res(float* __restrict__ res, const uint32_t pix, const float (&v)[RENDER_RES_FLOATS]) {
	f4* q = reinterpret_cast<f4*>(res + (size_t)pix * RENDER_RES_FLOATS);
	q[0] = f4{v[0], v[1], v[2], v[3]};
	q[1] = f4{v[4], v[5], v[6], v[7]};
	q[2] = f4{v[8], v[9], v[10], v[11]};
}

// Pixel (x, y) at the image position ((x + 0.5) / W, (y + 0.5) / H) -- with snap_to_pixel_centers the ray the training step casts for that pixel.
// t = max(box entry, near distance) + 1e-6 (testbed_nerf.cu:2404); a ray whose start is outside the box is finished with zero coverage.
__global__ __launch_bounds__(256) void k_render_init(const RenderArgs a, RenderRay* __restrict__ rays, uint32_t* __restrict__ keep, float* __restrict__ res) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= a.nt) return;
	const uint32_t p = a.p0 + i;
	const uint32_t x = p % a.view.width, y = p / a.view.width;
	const float xy[2] = {((float)x + 0.5f) / (float)a.view.width, ((float)y + 0.5f) / (float)a.view.height};
	Vec3 o, du, dir;
	camera_ray(a.view, xy, o, du, dir);
	float tmin, tmax;
	ray_intersect(a.A, o, dir, &tmin, &tmax);
	const float t = fmaxf(tmin, a.near_distance) + 1e-6f;
	const bool alive = aabb_contains(a.A, o + t * dir);
	keep[i] = alive ? 1u : 0u;
	if (!alive) {
		float v[RENDER_RES_FLOATS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
		store_res(res, i, v);
		return;
	}
	RenderRay r;
	r.o[0] = o.x; r.o[1] = o.y; r.o[2] = o.z; r.t = t;
	r.d[0] = dir.x; r.d[1] = dir.y; r.d[2] = dir.z; r.pix = i;
	r.n[0] = r.n[1] = r.n[2] = 0.f; r.w = 0.f;
	r.a[0] = r.a[1] = r.a[2] = 0.f; r.wmax = 0.f;
	r.depth = 0.f; r.nsamp = 0u; r.nstep = 0u; r.exhausted = 0u;
	rays[i] = r;
}

// keep[] holds the exclusive prefix sums of the alive flags (scan_exclusive): the alive rays move to dst in ray order.
__global__ __launch_bounds__(256) void k_render_compact(const uint32_t n, const RenderRay* __restrict__ src, const uint32_t* __restrict__ slot, const uint32_t n_alive,
                                                        RenderRay* __restrict__ dst) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n) return;
	const uint32_t s = slot[i];
	const uint32_t next = i + 1 < n ? slot[i + 1] : n_alive;
	if (next != s) dst[s] = src[i]; // the flag was 1
}

// generate_next_nerf_network_inputs (testbed_nerf.cu:822-879) with the training march's step and skip rules (min_mip 0, the context's cone angle). Sample j of ray i
// goes to record j * n_alive + i (the reference's layout); records [nstep, n) of a ray that ended early are filled with a neutral coordinate, so that every record below
// *n_eval -- the largest row any ray wrote, times n_alive; an order-independent atomicMax -- is a valid network input.
__global__ __launch_bounds__(256) void k_render_march(const RenderArgs a, const uint32_t n_alive, const uint32_t n, RenderRay* __restrict__ rays, float* __restrict__ coords,
                                                      uint32_t* __restrict__ n_eval, unsigned long long* __restrict__ n_samples) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n_alive) return;
	RenderRay& r = rays[i];
	const Vec3 o = {r.o[0], r.o[1], r.o[2]}, dir = {r.d[0], r.d[1], r.d[2]};
	const Vec3 idir = {1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z};
	const Vec3 wd = warp_direction(dir);
	const uint32_t nmax = min(n, (uint32_t)RNB_MAX_STEPS - r.nsamp);
	float t = r.t;
	uint32_t j = 0;
	while (j < nmax) {
		const Vec3 pos = o + t * dir;
		if (!aabb_contains(a.A, pos)) break;
		const float dt = calc_dt(t, a.A.cone_angle);
		const uint32_t mip = (uint32_t)mip_from_dt(dt, pos); // (as the training march: the cascade of the position, NERF_CASCADES - 1 at most)
		if (!a.bitfield || density_grid_occupied_at(pos, a.bitfield, mip)) {
			const Vec3 wp = warp_position(a.A, pos);
			float* q = coords + ((size_t)j * n_alive + i) * 7;
			q[0] = wp.x; q[1] = wp.y; q[2] = wp.z; q[3] = warp_dt(dt); q[4] = wd.x; q[5] = wd.y; q[6] = wd.z;
			t += dt;
			++j;
		} else {
			t = advance_to_next_voxel(t, a.A.cone_angle, pos, dir, idir, GRIDSIZE >> mip);
		}
	}
	for (uint32_t k = j; k < n; ++k) {
		float* q = coords + ((size_t)k * n_alive + i) * 7;
		q[0] = 0.5f; q[1] = 0.5f; q[2] = 0.5f; q[3] = 0.f; q[4] = 0.5f; q[5] = 0.5f; q[6] = 0.5f;
	}
	r.t = t;
	r.nstep = j;
	r.exhausted = j < nmax ? 1u : 0u;
	if (j) {
		atomicMax(n_eval, j * n_alive);
		atomicAdd(n_samples, (unsigned long long)j);
	}
}

// The final channels of a finished ray: 0-2 unit normal (0 where the coverage is 0), 3-5 albedo = sum w a / sum w, 6 opacity (1 after the early stop's division,
// testbed_nerf.cu:1100-1103), 7 depth where the opacity exceeds 0.2 (shade_kernel_nerf, :2278), 8 samples composited.
__device__ __forceinline__ void finish_ray(const RenderRay& r, const float opacity, float* __restrict__ res, uint32_t* __restrict__ n_hit) {
	float v[RENDER_RES_FLOATS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	if (r.w > 0.f) {
		const float nn = sqrtf(dot(v3(r.n[0], r.n[1], r.n[2]), v3(r.n[0], r.n[1], r.n[2])));
		if (nn > 0.f) { v[0] = r.n[0] / nn; v[1] = r.n[1] / nn; v[2] = r.n[2] / nn; }
		v[3] = r.a[0] / r.w; v[4] = r.a[1] / r.w; v[5] = r.a[2] / r.w;
	}
	v[6] = opacity;
	v[7] = opacity > 0.2f ? r.depth : 0.f;
	v[8] = (float)r.nsamp;
	store_res(res, r.pix, v);
	if (opacity > 0.001f) atomicAdd(n_hit, 1u); // the reference's hit counter (compact_kernel_nerf, :2299)
}

// composite_kernel_nerf (testbed_nerf.cu:881-1118): the ray's new samples in order, T = 1 - sum w, the NeuS alpha of the loss (alpha_terms with the direction the
// network echoed, BENT_DIR), the normal of Normals mode taken from the SDF gradient (outputs 4..6) and the albedo of the colour head (0..2; ones under no_albedo).
// keep[i] = 1 while the ray goes on.
__global__ __launch_bounds__(256) void k_render_composite(const RenderArgs a, const uint32_t n_alive, RenderRay* __restrict__ rays, const float* __restrict__ coords,
                                                          const half_t* __restrict__ net, uint32_t* __restrict__ keep, float* __restrict__ res, uint32_t* __restrict__ n_hit) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (i >= n_alive) return;
	RenderRay r = rays[i];
	const float diag = a.A.mx - a.A.mn;
	const Vec3 fwd = {a.fwd[0], a.fwd[1], a.fwd[2]}, o = {r.o[0], r.o[1], r.o[2]};
	LossFlags F = {};
	F.apply_no_albedo = a.apply_no_albedo;
	bool stopped = false;
	for (uint32_t j = 0; j < r.nstep; ++j) {
		const size_t s = (size_t)j * n_alive + i;
		half_t out[16];
		load_out16(net + s * 16, out);
		const float* q = coords + s * 7;
		const float dt = unwarp_dt(q[3]);
		const Vec3 dv = normalized(unwarp_direction(v3(h2f(out[8]), h2f(out[9]), h2f(out[10]))));
		const float dir[3] = {dv.x, dv.y, dv.z};
		const AlphaTerms at = alpha_terms(out, dt, dir, 1.0f);
		const float T = 1.f - r.w;
		const float weight = at.alpha * T;
		const Vec3 g = v3(at.g[0], at.g[1], at.g[2]);
		const float gn = sqrtf(dot(g, g));
		const Vec3 nrm = gn > 0.f ? v3(g.x / gn, g.y / gn, g.z / gn) : v3(0.f, 0.f, 0.f);
		float albedo[4];
		albedo_from_output(F, out, albedo);
		r.n[0] += weight * nrm.x; r.n[1] += weight * nrm.y; r.n[2] += weight * nrm.z;
		r.a[0] += weight * albedo[0]; r.a[1] += weight * albedo[1]; r.a[2] += weight * albedo[2];
		r.w += weight;
		++r.nsamp;
		if (weight > r.wmax) {
			r.wmax = weight;
			const Vec3 pos = v3(q[0] * diag + a.A.mn, q[1] * diag + a.A.mn, q[2] * diag + a.A.mn); // unwarp_position
			r.depth = dot(fwd, pos - o);
		}
		if (a.min_transmittance > 0.f && r.w > 1.0f - a.min_transmittance) { stopped = true; break; }
	}
	const bool done = stopped || r.exhausted || r.nsamp >= RNB_MAX_STEPS;
	keep[i] = done ? 0u : 1u;
	if (done) finish_ray(r, stopped ? 1.f : r.w, res, n_hit);
	else rays[i] = r;
}

// The tile's results into the caller's row-major [H][W][9] image: one thread per pixel; with VEC (the image and the tile start 16-byte aligned) one thread per
// four pixels, 9 x 16-byte stores.
template <bool VEC>
__global__ __launch_bounds__(256) void k_render_write(const uint32_t p0, const uint32_t nt, const float* __restrict__ res, float* __restrict__ out) {
	const uint32_t i = threadIdx.x + blockIdx.x * blockDim.x;
	if (VEC) {
		const uint32_t first = i * 4;
		if (first >= nt) return;
		if (first + 4 <= nt) {
			float v[36];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const f4* q = reinterpret_cast<const f4*>(res + (size_t)(first + k) * RENDER_RES_FLOATS);
				const f4 x0 = q[0], x1 = q[1], x2 = q[2];
				v[k * 9 + 0] = x0[0]; v[k * 9 + 1] = x0[1]; v[k * 9 + 2] = x0[2]; v[k * 9 + 3] = x0[3];
				v[k * 9 + 4] = x1[0]; v[k * 9 + 5] = x1[1]; v[k * 9 + 6] = x1[2]; v[k * 9 + 7] = x1[3];
				v[k * 9 + 8] = x2[0];
			}
			f4* dst = reinterpret_cast<f4*>(out + ((size_t)p0 + first) * RNB_RENDER_CHANNELS);
#pragma unroll
			for (int k = 0; k < 9; ++k) dst[k] = f4{v[k * 4 + 0], v[k * 4 + 1], v[k * 4 + 2], v[k * 4 + 3]};
			return;
		}
		for (uint32_t p = first; p < nt; ++p)
			for (int k = 0; k < (int)RNB_RENDER_CHANNELS; ++k) out[((size_t)p0 + p) * RNB_RENDER_CHANNELS + k] = res[(size_t)p * RENDER_RES_FLOATS + k];
		return;
	}
	if (i >= nt) return;
	for (int k = 0; k < (int)RNB_RENDER_CHANNELS; ++k) out[((size_t)p0 + i) * RNB_RENDER_CHANNELS + k] = res[(size_t)i * RENDER_RES_FLOATS + k];
}

} // namespace rnb
