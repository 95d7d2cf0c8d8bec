// driver_render.hpp -- the inference tracer rnb_render* (include/rnb_render.h) and its workspace.
// Needs, of rnb_neus2_hip.hip, which includes it: the context (aabb, bitfield, cfg, the workspace member `render`), as_stream, fail / HIP_TRY / RNB_GUARD and
// launch_forward; scan_exclusive, declared here and defined with the other scan helpers in driver_mesh.hpp.
namespace {
uint64_t scan_scratch_elems(uint64_t n);
int scan_exclusive(uint32_t* data, uint64_t n, hipStream_t s, uint32_t* total_out, uint32_t* scratch);
} // namespace

extern "C" {

// ---- inference tracer (include/rnb_render.h; Testbed::NerfTracer, src/testbed_nerf.cu:2499-2770) ----
uint32_t rnb_render_abi_version(void) { return RNB_RENDER_ABI_VERSION; }

int rnb_render_default_options(rnb_render_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_RENDER_ABI_VERSION;
	opt->min_transmittance = 0.01f; // testbed.h:723
	opt->near_distance = 0.2f;      // testbed_nerf.cu:48
	opt->use_inference_params = 1;
	opt->use_occupancy = 1;
	opt->max_rays_in_flight = 0;
	return RNB_OK;
} RNB_GUARD

int rnb_render(rnb_ctx* c, void* stream, const rnb_view* view, const rnb_render_options* opt, float* out, rnb_render_stats* stats) try {
	if (!c || !view || !opt) return fail(RNB_ERR_INVALID, "rnb_render: null argument");
	if (opt->abi_version != RNB_RENDER_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_render: options abi_version mismatch (expected RNB_RENDER_ABI_VERSION)");
	if (!out) return fail(RNB_ERR_INVALID, "rnb_render: out_dev is null");
	if (view->width == 0 || view->height == 0) return fail(RNB_ERR_INVALID, "rnb_render: empty view");
	const uint64_t n_pix = (uint64_t)view->width * view->height;
	if (n_pix > (1ull << 31)) return fail(RNB_ERR_INVALID, "rnb_render: more than 2^31 pixels");
	if (!(opt->min_transmittance >= 0.f && opt->min_transmittance < 1.f)) return fail(RNB_ERR_INVALID, "rnb_render: min_transmittance must be in [0, 1)");
	if (!(opt->near_distance >= 0.f) || !std::isfinite(opt->near_distance)) return fail(RNB_ERR_INVALID, "rnb_render: near_distance must be finite and >= 0");
	if (!(view->focal_length[0] > 0.f && view->focal_length[1] > 0.f)) return fail(RNB_ERR_INVALID, "rnb_render: focal lengths must be positive");
	const auto t_begin = std::chrono::steady_clock::now();
	hipStream_t s = as_stream(stream);
	join_tail_host(c); // the side stream's optimizer launch writes the weights the network evaluations read

	// tile size: a multiple of 64 (the write kernel's 16-byte stores start on a 4-pixel boundary), no larger than the image needs
	uint32_t R = opt->max_rays_in_flight ? opt->max_rays_in_flight : (1u << 19);
	R = std::max<uint32_t>(64u, R / 64u * 64u);
	R = (uint32_t)std::min<uint64_t>(R, (n_pix + 63) / 64 * 64);
	RenderWorkspace& w = c->render;
	if (R > w.cap) {
		w.release_arrays();
		if (w.rays[0].alloc(R) != hipSuccess || w.rays[1].alloc(R) != hipSuccess || w.keep.alloc(R) != hipSuccess ||
		    w.scan.alloc(scan_scratch_elems(R)) != hipSuccess || w.res.alloc((size_t)R * RENDER_RES_FLOATS) != hipSuccess ||
		    w.coords.alloc((size_t)R * RENDER_MAX_N * 7) != hipSuccess || w.out.alloc((size_t)R * RENDER_MAX_N * 16) != hipSuccess) {
			w.release_arrays();
			return fail(RNB_ERR_NOMEM, "rnb_render: hipMalloc failed for the render workspace (lower max_rays_in_flight)");
		}
		w.cap = R;
	}
	if (!w.counts.p && w.counts.alloc(4) != hipSuccess) return fail(RNB_ERR_NOMEM, "rnb_render: hipMalloc failed for the counters");
	uint32_t* n_eval = w.counts.p;
	uint32_t* n_hit = w.counts.p + 1;
	unsigned long long* n_samples = reinterpret_cast<unsigned long long*>(w.counts.p + 2);
	HIP_TRY(hipMemsetAsync(w.counts.p, 0, 16, s));

	RenderArgs a;
	std::memset(&a, 0, sizeof(a));
	a.view.width = view->width; a.view.height = view->height;
	a.view.focal[0] = view->focal_length[0]; a.view.focal[1] = view->focal_length[1];
	a.view.principal[0] = view->principal_point[0]; a.view.principal[1] = view->principal_point[1];
	for (int k = 0; k < 12; ++k) a.view.xform[k] = view->xform[k];
	a.view.normal = nullptr; a.view.albedo = nullptr;
	a.A = c->aabb;
	a.bitfield = opt->use_occupancy ? c->bitfield.p : nullptr;
	a.near_distance = opt->near_distance;
	a.min_transmittance = opt->min_transmittance;
	a.apply_no_albedo = c->cfg.apply_no_albedo;
	a.fwd[0] = view->xform[2]; a.fwd[1] = view->xform[6]; a.fwd[2] = view->xform[10];
	const bool inference = opt->use_inference_params != 0;
	const bool vec = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
	uint32_t rounds = 0;
	for (uint64_t p0 = 0; p0 < n_pix; p0 += R) {
		const uint32_t nt = (uint32_t)std::min<uint64_t>(R, n_pix - p0);
		a.p0 = (uint32_t)p0; a.nt = nt;
		hipLaunchKernelGGL(k_render_init, dim3((nt + 255) / 256), dim3(256), 0, s, a, w.rays[0].p, w.keep.p, w.res.p);
		HIP_TRY(hipGetLastError());
		uint32_t cur = 0, n_cur = nt;
		while (true) {
			uint32_t n_alive = 0;
			int rc = scan_exclusive(w.keep.p, n_cur, s, &n_alive, w.scan.p); // the round's one read (and synchronisation)
			if (rc != RNB_OK) return rc;
			if (n_alive == 0) break;
			hipLaunchKernelGGL(k_render_compact, dim3((n_cur + 255) / 256), dim3(256), 0, s, n_cur, w.rays[cur].p, w.keep.p, n_alive, w.rays[cur ^ 1].p);
			cur ^= 1;
			// Samples per ray this round. The reference takes clamp(n_initialised / n_alive, 1, 8) (testbed_nerf.cu:2731): one sample per ray in the first round, and
			// ~20 rounds for an 800 x 800 frame of a trained scene, each paying a read-back and seven launches. Here the round's budget is what the workspace holds,
			// RENDER_MAX_N samples per ray of the tile, spread over the rays still alive (at most RENDER_ROUND_MAX each). The image does not depend on it.
			const uint32_t n = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((uint64_t)RENDER_MAX_N * nt / n_alive, 1), RENDER_ROUND_MAX);
			HIP_TRY(hipMemsetAsync(n_eval, 0, 4, s));
			hipLaunchKernelGGL(k_render_march, dim3((n_alive + 255) / 256), dim3(256), 0, s, a, n_alive, n, w.rays[cur].p, w.coords.p, n_eval, n_samples);
			HIP_TRY(hipGetLastError());
			rc = launch_forward(c, s, w.coords.p, n_eval, n * n_alive, w.out.p, inference);
			if (rc != RNB_OK) return rc;
			hipLaunchKernelGGL(k_render_composite, dim3((n_alive + 255) / 256), dim3(256), 0, s, a, n_alive, w.rays[cur].p, w.coords.p, w.out.p,
			                   w.keep.p, w.res.p, n_hit);
			HIP_TRY(hipGetLastError());
			n_cur = n_alive;
			++rounds;
		}
		if (vec) hipLaunchKernelGGL(k_render_write<true>, dim3((nt / 4 + 1 + 255) / 256), dim3(256), 0, s, (uint32_t)p0, nt, w.res.p, out);
		else hipLaunchKernelGGL(k_render_write<false>, dim3((nt + 255) / 256), dim3(256), 0, s, (uint32_t)p0, nt, w.res.p, out);
		HIP_TRY(hipGetLastError());
	}
	uint32_t counts[4] = {0, 0, 0, 0};
	HIP_TRY(hipMemcpyAsync(counts, w.counts.p, 16, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (stats) {
		stats->n_rays = (uint32_t)n_pix;
		stats->n_hit = counts[1];
		stats->rounds = rounds;
		stats->reserved = 0;
		stats->n_samples = (uint64_t)counts[2] | ((uint64_t)counts[3] << 32);
		stats->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	}
	return RNB_OK;
} RNB_GUARD

} // extern "C"
