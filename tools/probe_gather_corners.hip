// probe_gather_corners.hip -- is the L1 path of a scattered 4-byte gather paid per distinct LINE of a wave instruction, or per lane address / outstanding miss?
// The hash-grid encode (csrc/common.cuh: level_issue) gives a sample to a lane and fetches corner c of 64 samples per instruction: up to 64 lines per instruction on the
// fine levels, and the x-neighbour of every entry (the next table entry on dense levels, and on hashed levels when x is even) comes one instruction later as a second
// look-up of the same line. Turned round -- 8 lanes per sample, lane = 8 (s mod 8) + c -- an instruction fetches the 8 corners of 8 samples: the x-pair is lanes 2k / 2k + 1,
// and the same line is asked for once per instruction instead of in two or four.
// Three kernels that only gather and sum, on the product's table geometry (14 levels, 16 .. 2048, 2^19 entries per hashed level: 21 MB) and its two access patterns
// (2^18 samples along rays with step sqrt(3)/1024; 2^18 points jittered in Morton-ordered cells of a 64^3 grid); the table indices are formed as level_issue forms them:
//   a   one lane per sample, 8 instructions per level and 64 samples                          (today's mapping)
//   b   lane = 8 (s mod 8) + c, bit 0 of c = x; 8 instructions per level, each 8 samples      (corner-parallel)
//   c   as b with bit 0 of c = z, bit 2 = x: adjacent lanes do not share entries              (control: the regrouping without the pairing)
// Every kernel issues the same number of load instructions for the same entries. Output: lane-gathers per second per pattern and level group.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o tools/probe_gather_corners tools/probe_gather_corners.hip ; tools/probe_gather_corners a|b|c
// (one kernel per process, so that a job can give each its own time limit and stop at the first failure)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

constexpr uint32_t N_LEVELS = 14, LOG2_HASHMAP = 19, BASE_RES = 16, N_SAMPLES = 1u << 18;

struct Level { uint32_t offset, size, res; float scale; uint32_t my, mz, dense, pow2; }; // csrc/common.cuh: LevelMeta
struct Levels { Level l[N_LEVELS]; };

__host__ __device__ inline void pos_grid(float input, float scale, uint32_t* pg) { // pos_fract's cell
	const float p = input * scale + 0.5f;
	*pg = (uint32_t)(int)floorf(p);
}
// the table index of corner (cx, cy, cz) of the sample's cell: level_issue's e0 / e1 for yz = cy + 2 cz
__host__ __device__ inline uint32_t corner_index(const Level& L, float x, float y, float z, uint32_t cx, uint32_t cy, uint32_t cz) {
	uint32_t pg[3];
	pos_grid(x, L.scale, &pg[0]); pos_grid(y, L.scale, &pg[1]); pos_grid(z, L.scale, &pg[2]);
	const uint32_t ty0 = pg[1] * L.my, tz0 = pg[2] * L.mz;
	const uint32_t ty = cy ? ty0 + L.my : ty0, tz = cz ? tz0 + L.mz : tz0;
	const uint32_t d = pg[0] + cx + ty + tz, h = (pg[0] + cx) ^ (ty ^ tz);
	uint32_t e = L.dense ? d : h;
	const uint32_t w = e >= L.size ? e - L.size : e;
	e = L.pow2 ? (e & (L.size - 1u)) : w;
	return e;
}

// a: lane = sample
__global__ __launch_bounds__(256) void p_sample_per_lane(const Levels M, const uint32_t* __restrict__ grid, const float* __restrict__ xyz, uint32_t n, uint32_t l0, uint32_t l1, uint32_t* __restrict__ sink) {
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const float x = xyz[s * 3 + 0], y = xyz[s * 3 + 1], z = xyz[s * 3 + 2];
	uint32_t acc = 0;
#pragma unroll 1
	for (uint32_t l = l0; l < l1; ++l) {
		const Level& L = M.l[l];
		const uint32_t* __restrict__ g = grid + L.offset;
		uint32_t v[8];
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c) v[c] = g[corner_index(L, x, y, z, c & 1u, (c >> 1) & 1u, c >> 2)];
#pragma unroll
		for (uint32_t c = 0; c < 8; ++c) acc += v[c];
	}
	if (acc == 0x12345678u) sink[0] = acc;
}
// b, c: a wavefront's tile is still 64 samples; instruction i serves samples 8 i .. 8 i + 7, lane l takes sample 8 i + (l >> 3) and corner l & 7
template <bool X_FIRST>
__global__ __launch_bounds__(256) void p_corner_per_lane(const Levels M, const uint32_t* __restrict__ grid, const float* __restrict__ xyz, uint32_t n, uint32_t l0, uint32_t l1, uint32_t* __restrict__ sink) {
	const uint32_t lane = threadIdx.x & 63u, tile0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63u;
	if (tile0 >= n) return; // (n is a multiple of 64)
	const uint32_t c = lane & 7u;
	const uint32_t cx = X_FIRST ? (c & 1u) : (c >> 2), cy = (c >> 1) & 1u, cz = X_FIRST ? (c >> 2) : (c & 1u);
	float x[8], y[8], z[8];
#pragma unroll
	for (uint32_t i = 0; i < 8; ++i) {
		const uint32_t s = tile0 + 8u * i + (lane >> 3);
		x[i] = xyz[s * 3 + 0]; y[i] = xyz[s * 3 + 1]; z[i] = xyz[s * 3 + 2];
	}
	uint32_t acc = 0;
#pragma unroll 1
	for (uint32_t l = l0; l < l1; ++l) {
		const Level& L = M.l[l];
		const uint32_t* __restrict__ g = grid + L.offset;
		uint32_t v[8];
#pragma unroll
		for (uint32_t i = 0; i < 8; ++i) v[i] = g[corner_index(L, x[i], y[i], z[i], cx, cy, cz)];
#pragma unroll
		for (uint32_t i = 0; i < 8; ++i) acc += v[i];
	}
	if (acc == 0x12345678u) sink[0] = acc;
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)

static uint32_t morton_compact(uint32_t v) { v &= 0x09249249u; v = (v ^ (v >> 2)) & 0x030c30c3u; v = (v ^ (v >> 4)) & 0x0300f00fu; v = (v ^ (v >> 8)) & 0xff0000ffu; v = (v ^ (v >> 16)) & 0x000003ffu; return v; }

int main(int argc, char** argv) {
	if (argc != 2 || std::strlen(argv[1]) != 1 || argv[1][0] < 'a' || argv[1][0] > 'c') { std::fprintf(stderr, "usage: %s a|b|c\n", argv[0]); return 2; }
	const char which = argv[1][0];
	// the level geometry of the base configuration (rnb_neus2_hip.hip: build_grid_tables; csrc/common.cuh: fill_level_meta)
	Levels M;
	uint32_t offset = 0;
	const float per_level_scale = std::exp(std::log(2048.0f / (float)BASE_RES) / (float)(N_LEVELS - 1));
	for (uint32_t i = 0; i < N_LEVELS; ++i) {
		const float scale = exp2f(i * std::log2(per_level_scale)) * BASE_RES - 1.0f;
		const uint32_t res = (uint32_t)ceilf(scale) + 1;
		uint64_t n3 = (uint64_t)res * res * res;
		n3 = (n3 + 7) / 8 * 8;
		Level& L = M.l[i];
		L.offset = offset; L.size = (uint32_t)std::min<uint64_t>(n3, 1u << LOG2_HASHMAP); L.res = res; L.scale = (float)(res - 1);
		L.dense = (uint64_t)res * res * res <= L.size ? 1u : 0u;
		L.pow2 = (L.size & (L.size - 1u)) == 0u ? 1u : 0u;
		L.my = L.dense ? res : 2654435761u;
		L.mz = L.dense ? res * res : 805459861u;
		offset += L.size;
	}
	const uint32_t n_entries = offset;
	// the two inputs
	std::mt19937 rng(12345);
	std::uniform_real_distribution<float> U(0.f, 1.f);
	std::vector<float> rays((size_t)N_SAMPLES * 3), points((size_t)N_SAMPLES * 3);
	const float step = std::sqrt(3.0f) / 1024.0f;
	for (uint32_t r = 0; r < N_SAMPLES / 256; ++r) { // 1024 rays of 256 samples: origin in [0.02, 0.5]^3, direction into the positive octant (0.5 + 256 step < 1)
		float o[3], d[3], n2 = 0.f;
		for (int k = 0; k < 3; ++k) { o[k] = 0.02f + 0.48f * U(rng); d[k] = 0.05f + U(rng); n2 += d[k] * d[k]; }
		for (int k = 0; k < 3; ++k) d[k] /= std::sqrt(n2);
		for (uint32_t j = 0; j < 256; ++j)
			for (int k = 0; k < 3; ++k) rays[((size_t)r * 256 + j) * 3 + k] = std::min(o[k] + (float)j * step * d[k], 0.999999f);
	}
	for (uint32_t m = 0; m < N_SAMPLES; ++m) { // cell m of a 64^3 grid in Morton order, the point jittered inside it
		const uint32_t ix = morton_compact(m), iy = morton_compact(m >> 1), iz = morton_compact(m >> 2);
		const uint32_t cell[3] = {ix, iy, iz};
		for (int k = 0; k < 3; ++k) points[(size_t)m * 3 + k] = std::min(((float)cell[k] + U(rng)) / 64.0f, 0.999999f);
	}
	// every index the kernels will form lies inside its level's table (checked on the host with the same function)
	for (const std::vector<float>* in : {&rays, &points})
		for (uint32_t s = 0; s < N_SAMPLES; ++s)
			for (uint32_t l = 0; l < N_LEVELS; ++l)
				for (uint32_t c = 0; c < 8; ++c)
					if (corner_index(M.l[l], (*in)[s * 3 + 0], (*in)[s * 3 + 1], (*in)[s * 3 + 2], c & 1u, (c >> 1) & 1u, c >> 2) >= M.l[l].size) { std::fprintf(stderr, "index out of its table: sample %u level %u corner %u\n", s, l, c); return 1; }
	uint32_t *grid = nullptr, *sink = nullptr;
	float* d_in[2] = {nullptr, nullptr};
	CK(hipMalloc((void**)&grid, (size_t)n_entries * 4));
	CK(hipMalloc((void**)&sink, 64));
	{
		std::vector<uint32_t> h(n_entries);
		for (uint32_t& w : h) w = rng();
		CK(hipMemcpy(grid, h.data(), (size_t)n_entries * 4, hipMemcpyHostToDevice));
	}
	for (int p = 0; p < 2; ++p) {
		CK(hipMalloc((void**)&d_in[p], (size_t)N_SAMPLES * 12));
		CK(hipMemcpy(d_in[p], (p ? points : rays).data(), (size_t)N_SAMPLES * 12, hipMemcpyHostToDevice));
	}
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	const dim3 grid_dim(N_SAMPLES / 256), block(256);
	auto launch = [&](const float* in, uint32_t l0, uint32_t l1) {
		if (which == 'a') hipLaunchKernelGGL(p_sample_per_lane, grid_dim, block, 0, 0, M, grid, in, N_SAMPLES, l0, l1, sink);
		else if (which == 'b') hipLaunchKernelGGL(p_corner_per_lane<true>, grid_dim, block, 0, 0, M, grid, in, N_SAMPLES, l0, l1, sink);
		else hipLaunchKernelGGL(p_corner_per_lane<false>, grid_dim, block, 0, 0, M, grid, in, N_SAMPLES, l0, l1, sink);
	};
	const char* kname[3] = {"a sample-per-lane", "b corner-per-lane, x in lane bit 0", "c corner-per-lane, z in lane bit 0"};
	const struct { const char* name; uint32_t l0, l1; } groups[4] = {{"all 0-13", 0, 14}, {"dense 0-4", 0, 5}, {"hashed 5-9", 5, 10}, {"hashed 10-13", 10, 14}};
	constexpr int REPS = 20, INNER = 8; // a timing spans INNER back-to-back launches
	std::printf("kernel %s: table %.1f MB, %u samples, median of %d timings of %d launches each, per launch\n", kname[which - 'a'], n_entries * 4 / 1e6, N_SAMPLES, REPS, INNER);
	for (int p = 0; p < 2; ++p)
		for (const auto& g : groups) {
			for (int w = 0; w < 3; ++w) launch(d_in[p], g.l0, g.l1);
			CK(hipDeviceSynchronize());
			std::vector<float> ms(REPS);
			for (int r = 0; r < REPS; ++r) {
				CK(hipEventRecord(e0, 0));
				for (int q = 0; q < INNER; ++q) launch(d_in[p], g.l0, g.l1);
				CK(hipEventRecord(e1, 0));
				CK(hipEventSynchronize(e1));
				CK(hipEventElapsedTime(&ms[r], e0, e1));
				ms[r] /= (float)INNER;
			}
			CK(hipGetLastError());
			std::sort(ms.begin(), ms.end());
			const double gathers = (double)N_SAMPLES * (g.l1 - g.l0) * 8;
			std::printf("  %-6s  levels %-13s  %8.2f us  [%7.2f .. %7.2f]   %7.1f G lane-gathers/s\n", p ? "points" : "rays", g.name, ms[REPS / 2] * 1e3, ms[0] * 1e3, ms[REPS - 1] * 1e3, gathers / (ms[REPS / 2] * 1e-3) / 1e9);
		}
	return 0;
}
