// driver_mesh.hpp -- rnb_sdf_lattice, rnb_marching_cubes and the mesh stages rnb_extract_mesh, rnb_mesh_clean, rnb_mesh_simplify, rnb_mesh_distance, rnb_mesh_raster,
// rnb_mesh_draw_textured, rnb_mesh_visibility, rnb_mesh_visibility_select, rnb_mesh_bake_texture, rnb_mesh_project_views, rnb_mesh_topology, rnb_mesh_repair
// (include/rnb_mesh_topology.h; their hash join is tp_join, beside them), rnb_mesh_boundary_loops, rnb_mesh_fill_holes (include/rnb_mesh_holes.h; hl_census is the
// part they share), rnb_mesh_intersections, rnb_mesh_intersections_select (include/rnb_mesh_intersect.h; md_build_lists, beside rnb_mesh_distance, is the grid they
// share with it), rnb_mesh_smooth, rnb_mesh_vertex_normals (include/rnb_mesh_smooth.h; on tp_join too; vn_run is the part they share), rnb_mesh_snap
// (include/rnb_mesh_snap.h; launch_forward round by round). What they share:
//   scan_exclusive, count_and_scan                  the prefix sums behind every numbering, and the count half of a count / write kernel pair
//   MeshWorkspace, alloc_mesh, hand_over            the device memory of one call and the mesh it returns
//   check_mesh_input, check_reserved, free_device   the argument checks every stage makes; the *_free functions
//   MeshCall                                        one call of a stage: its name in every failure, stream, workspace and time; the index check (check_indices)
//                                                   and the compaction of a mesh to its kept part (compact)
//   ensure_mc_table                                 the marching-cubes case table on the device
//   check_near_cull, check_raster_view, check_raster_call, raster_camera, raster_clear, raster_fill, raster_image, launch_md_resolve
//                                                   the rasteriser's checks, camera and fill, for the draw, the visibility stage and the projection too
//   make_atlas, launch_mp_accumulate                the atlas of the baker and the projection; the projection's accumulate launch per image format
// Needs, of rnb_neus2_hip.hip, which includes it: the context (aabb, bitfield, cfg, mc_table), as_stream, join_tail_host, fail / HIP_TRY / RNB_GUARD,
// launch_point_query and launch_forward.
extern "C" {

// ---- mesh extraction (src/testbed_nerf.cu:4218-4269, src/marching_cubes.cu:276-430, 794-822) ----
int rnb_sdf_lattice(rnb_ctx* c, void* stream, const uint32_t res[3], float lattice_min, float lattice_max, float* out, int inference) try {
	if (!c || !res || !out) return fail(RNB_ERR_INVALID, "null argument");
	if (!res[0] || !res[1] || !res[2]) return fail(RNB_ERR_INVALID, "empty lattice");
	hipStream_t s = as_stream(stream);
	const uint64_t n = (uint64_t)res[0] * res[1] * res[2];
	const uint32_t batch = 1u << 22; // lattice points per network launch (the reference: 2^20 per call, same arithmetic per point)
	float* pos = nullptr;
	half_t* val = nullptr;
	if (hipMalloc((void**)&pos, (size_t)batch * 12) != hipSuccess || hipMalloc((void**)&val, (size_t)batch * 2) != hipSuccess) {
		if (pos) (void)hipFree(pos);
		return fail(RNB_ERR_NOMEM, "hipMalloc failed for the lattice batch");
	}
	const float diag = c->aabb.mx - c->aabb.mn;
	int rc = RNB_OK;
	for (uint64_t off = 0; off < n && rc == RNB_OK; off += batch) {
		const uint32_t nb = (uint32_t)std::min<uint64_t>(batch, n - off);
		hipLaunchKernelGGL(k_lattice_positions, dim3((nb + 255) / 256), dim3(256), 0, s, off, nb, res[0], res[1], res[2], lattice_min, lattice_max - lattice_min, c->aabb.mn, diag, pos);
		rc = launch_point_query(c, s, pos, nb, val, nullptr, nullptr, 0, inference != 0);
		if (rc != RNB_OK) break;
		hipLaunchKernelGGL(k_half_to_float, dim3((nb + 255) / 256), dim3(256), 0, s, val, out + off, nb);
		if (hipGetLastError() != hipSuccess) rc = fail(RNB_ERR_DEVICE, "rnb_sdf_lattice: kernel launch failed");
	}
	hipError_t e = hipStreamSynchronize(s);
	(void)hipFree(pos); (void)hipFree(val);
	if (rc != RNB_OK) return rc;
	if (e != hipSuccess) return fail(RNB_ERR_DEVICE, std::string("rnb_sdf_lattice: ") + hipGetErrorString(e));
	return RNB_OK;
} RNB_GUARD

// ---- what the drivers of the mesh stages share ----
extern "C++" {
namespace {
// elements of block-sum scratch scan_exclusive needs for n counts: sum over the levels of ceil(n / 1024^k)
uint64_t scan_scratch_elems(uint64_t n) {
	uint64_t total = 0;
	do { n = (n + 1023) / 1024; total += n; } while (n > 1);
	return total;
}
// in-place exclusive prefix sums of n counts (device), total to *total_out; `scratch` holds scan_scratch_elems(n) uint32 (allocated once per
// call and shared by its scans)
int scan_exclusive(uint32_t* data, uint64_t n, hipStream_t s, uint32_t* total_out, uint32_t* scratch) {
	std::vector<uint32_t*> levels{data};
	std::vector<uint64_t> sizes{n};
	while (true) {
		const uint64_t nb = (sizes.back() + 1023) / 1024;
		uint32_t* sums = scratch;
		scratch += nb;
		hipLaunchKernelGGL(k_scan_blocks, dim3((uint32_t)nb), dim3(1024), 0, s, levels.back(), sizes.back(), sums);
		levels.push_back(sums); sizes.push_back(nb);
		if (nb == 1) break;
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(total_out, levels.back(), 4, hipMemcpyDeviceToHost, s));
	// levels.back() holds one value (the total); every level below gets its block offsets added, top-down
	for (size_t k = levels.size() - 1; k >= 2; --k) { /* levels[k-1] was scanned by the launch that produced levels[k]; add it to levels[k-2] */
		hipLaunchKernelGGL(k_scan_add, dim3((uint32_t)sizes[k - 1]), dim3(1024), 0, s, levels[k - 2], sizes[k - 2], levels[k - 1]);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	return RNB_OK;
}
// workgroups of MESH_WG threads for one thread per item
uint32_t groups(uint64_t n) { return (uint32_t)((n + MESH_WG - 1) / MESH_WG); }
// Phase one of a count / write kernel pair: the <false> instantiation leaves one count per workgroup in wg; they become the workgroups' exclusive offsets, their sum goes
// to *total (synchronises). The write launch stays with the caller, who allocates for the total in between.
template <typename K, typename... A>
int count_and_scan(hipStream_t s, uint32_t n_wg, uint32_t* wg, uint32_t* scratch, uint32_t* total, K count_kernel, A... args) {
	hipLaunchKernelGGL(count_kernel, dim3(n_wg), dim3(MESH_WG), 0, s, args...);
	HIP_TRY(hipGetLastError());
	return scan_exclusive(wg, n_wg, s, total, scratch);
}

// The device memory of one mesh call: what is still held when the object goes out of scope is released; bytes held now and at the peak.
struct MeshWorkspace {
	std::vector<std::pair<void*, size_t>> held;
	size_t cur = 0, peak = 0;
	template <typename T>
	bool alloc(T** p, size_t count) {
		*p = nullptr;
		const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
		if (hipMalloc((void**)p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
		held.emplace_back((void*)*p, bytes);
		cur += bytes; peak = std::max(peak, cur);
		return true;
	}
	template <typename T, typename... U>
	void release(T*& p, U*&... more) { // free now
		for (auto& h : held) if (h.first == (void*)p && p) { (void)hipFree(h.first); cur -= h.second; h.first = nullptr; }
		p = nullptr;
		if constexpr (sizeof...(more) > 0) release(more...);
	}
	void* keep(void* p) { // the caller owns it from here on (it still counts as held)
		for (auto& h : held) if (h.first == p) h.first = nullptr;
		return p;
	}
	~MeshWorkspace() { for (auto& h : held) if (h.first) (void)hipFree(h.first); }
};

// What every stage asks of its input mesh, said in the entry point's name; *out (null for a stage that returns no mesh) is zeroed as soon as it is known not to be
// the input.
int check_mesh_input(const char* name, const rnb_mesh* in, rnb_mesh* out = nullptr) {
	const std::string n(name);
	if (out) {
		if (in == out) return fail(RNB_ERR_INVALID, n + ": in and out must be different objects");
		std::memset(out, 0, sizeof(*out));
	}
	if (in->n_indices % 3u) return fail(RNB_ERR_INVALID, n + ": n_indices is not a multiple of 3");
	if ((in->n_verts && !in->verts) || (in->n_indices && !in->indices)) return fail(RNB_ERR_INVALID, n + ": null vertex or index buffer");
	if (in->n_indices && in->n_verts == 0) return fail(RNB_ERR_INVALID, n + ": an index is out of range (the mesh has no vertices)");
	return RNB_OK;
}
// The output mesh of a stage, held by the workspace: nvo vertices with the attributes asked for, nto triangles (a count of 0 still gets a buffer: MeshWorkspace::alloc).
bool alloc_mesh(MeshWorkspace& ws, rnb_mesh* m, uint32_t nvo, uint32_t nto, bool has_colors, bool has_normals) {
	std::memset(m, 0, sizeof(*m));
	m->n_verts = nvo; m->n_indices = nto * 3u;
	return ws.alloc(&m->verts, (size_t)nvo * 3) && ws.alloc(&m->indices, (size_t)nto * 3) && (!has_colors || ws.alloc(&m->colors, (size_t)nvo * 3)) && (!has_normals || ws.alloc(&m->normals, (size_t)nvo * 3));
}
// *out = m, whose buffers the caller owns from here on.
void hand_over(MeshWorkspace& ws, const rnb_mesh& m, rnb_mesh* out) {
	*out = m;
	ws.keep(m.verts); ws.keep(m.indices); ws.keep(m.colors); ws.keep(m.normals);
}
// The reserved words of an options struct must be 0.
template <size_t N>
int check_reserved(const char* name, const uint32_t (&reserved)[N]) {
	for (uint32_t r : reserved)
		if (r) return fail(RNB_ERR_INVALID, std::string(name) + ": a reserved word of the options is not 0");
	return RNB_OK;
}
// The *_free functions: the device buffers of a result released, the struct zeroed.
template <typename S>
void free_device(S* obj, std::initializer_list<void*> buffers) {
	for (void* p : buffers) if (p) (void)hipFree(p);
	std::memset(obj, 0, sizeof(*obj));
}

// One call of a mesh stage, constructed from the entry point's name once its arguments have passed their checks: the start of the time the statistics report, the
// stream (the side stream's tail joined: its optimizer launch writes the weights the network evaluations read), the workspace; failures said in the entry point's
// name; and what the stages do alike on the device.
struct MeshCall {
	const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
	const std::string name;
	const hipStream_t s;
	MeshWorkspace ws;
	MeshCall(const char* name_, rnb_ctx* c, void* stream) : name(name_), s(as_stream(stream)) { join_tail_host(c); }
	int invalid(const std::string& text) const { return fail(RNB_ERR_INVALID, name + ": " + text); }
	int nomem(const std::string& text) const { return fail(RNB_ERR_NOMEM, name + ": " + text); }
	int device(const std::string& text) const { return fail(RNB_ERR_DEVICE, name + ": " + text); }
	template <typename S>
	void finish(S* stats) const {
		stats->peak_workspace = ws.peak;
		stats->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	}

	// The index check: every index of m is range-checked before any is used as an address (m has a triangle, so n_verts >= 1: check_mesh_input). used[] is
	// cleared and gets a 1 per corner; `bit` is set in the caller's flag word *dflags (device, zero) if an index is >= n_verts. In three parts, for the stages that
	// check two meshes, or read more than the flag, under one synchronise: the launch,
	int check_indices_launch(const rnb_mesh& m, uint32_t* used, uint32_t* dflags, uint32_t bit = MESH_BAD_INDEX) const {
		const uint32_t nt = m.n_indices / 3u;
		HIP_TRY(hipMemsetAsync(used, 0, (size_t)m.n_verts * 4, s));
		hipLaunchKernelGGL(k_mesh_validate, dim3(groups(nt)), dim3(MESH_WG), 0, s, (const uint32_t*)m.indices, nt, m.n_verts, used, dflags, bit);
		HIP_TRY(hipGetLastError());
		return RNB_OK;
	}
	// the flag word read back (synchronises),
	int read_flags(const uint32_t* dflags, uint32_t* hflags) const {
		HIP_TRY(hipMemcpyAsync(hflags, dflags, 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		return RNB_OK;
	}
	// the failure (of: "of from ", "of to " where a stage takes two meshes);
	int bad_index(const char* of = "") const { return invalid(std::string("an index ") + of + "is out of range (>= n_verts)"); }
	// and all three, for a stage that checks one mesh under a synchronise of its own.
	int check_indices(const rnb_mesh& m, uint32_t* used, uint32_t* dflags) const {
		uint32_t hflags = 0;
		if (int rc = check_indices_launch(m, used, dflags); rc != RNB_OK) return rc;
		if (int rc = read_flags(dflags, &hflags); rc != RNB_OK) return rc;
		return (hflags & MESH_BAD_INDEX) ? bad_index() : RNB_OK;
	}

	// kernel(args...) in n_wg workgroups of MESH_WG threads on the call's stream (the topology stage's launches, the cleaner's kernels it reuses among them).
	template <typename K, typename... A>
	void launch(uint32_t n_wg, K kernel, A... args) const { hipLaunchKernelGGL(kernel, dim3(n_wg), dim3(MESH_WG), 0, s, args...); }

	// An output mesh shaped like m (its attributes), held by the workspace.
	int alloc_like(const rnb_mesh& m, rnb_mesh* o, uint32_t nvo, uint32_t nto) {
		return alloc_mesh(ws, o, nvo, nto, m.colors != nullptr, m.normals != nullptr) ? RNB_OK : nomem("hipMalloc failed for the output mesh");
	}
	// The stable compaction of m to what `keep` keeps (ClKeep, MvKeep; k_compact_verts and k_compact_tris of mesh_common.cuh), as the new mesh *o: vmap holds a 1 per
	// kept vertex on entry and the new numbering on return, twg takes one count per workgroup of triangles, scan is the scratch of scan_exclusive for both.
	// The launches are issued; the caller synchronises.
	template <typename KEEP>
	int compact(const rnb_mesh& m, const KEEP& keep, uint32_t* vmap, uint32_t* twg, uint32_t* scan, rnb_mesh* o, uint32_t* nvo, uint32_t* nto) {
		const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, g_v = groups(nv), g_t = groups(nt);
		if (int rc = scan_exclusive(vmap, nv, s, nvo, scan); rc != RNB_OK) return rc;
		if (int rc = count_and_scan(s, g_t, twg, scan, nto, k_compact_tris<false, KEEP>, (const uint32_t*)m.indices, nt, keep, (const uint32_t*)vmap, twg, (const uint32_t*)nullptr, (uint32_t*)nullptr); rc != RNB_OK) return rc;
		if (int rc = alloc_like(m, o, *nvo, *nto); rc != RNB_OK) return rc;
		hipLaunchKernelGGL(k_compact_verts<KEEP>, dim3(g_v), dim3(MESH_WG), 0, s, keep, (const uint32_t*)vmap, nv, (const float*)m.verts, (const float*)m.colors, (const float*)m.normals, o->verts, o->colors, o->normals);
		hipLaunchKernelGGL((k_compact_tris<true, KEEP>), dim3(g_t), dim3(MESH_WG), 0, s, (const uint32_t*)m.indices, nt, keep, (const uint32_t*)vmap, (uint32_t*)nullptr, (const uint32_t*)twg, o->indices);
		HIP_TRY(hipGetLastError());
		return RNB_OK;
	}
};
} // namespace
} // extern "C++"

// the marching-cubes case table of host/mesh.hpp on the device, uploaded on first use
static int ensure_mc_table(rnb_ctx* c) {
	if (c->mc_table.p) return RNB_OK;
	static const mesh::Tables T;
	std::vector<McTable> h(1);
	for (int m = 0; m < 256; ++m) {
		int k = 0;
		for (; T.tri[m][k] >= 0; ++k) h[0].tri[m][k] = T.tri[m][k];
		h[0].n[m] = (uint8_t)k;
		for (; k < 40; ++k) h[0].tri[m][k] = -1;
	}
	if (c->mc_table.alloc(1) != hipSuccess) return fail(RNB_ERR_NOMEM, "hipMalloc failed for the case table");
	HIP_TRY(hipMemcpy(c->mc_table.p, h.data(), sizeof(McTable), hipMemcpyHostToDevice));
	return RNB_OK;
}

int rnb_marching_cubes(rnb_ctx* c, void* stream, const float* density, const uint32_t res[3], const float aabb_min[3], const float aabb_max[3], float thresh,
                       float** verts_out, uint32_t** indices_out, uint32_t* n_verts, uint32_t* n_indices) try {
	if (!c || !density || !res || !aabb_min || !aabb_max || !verts_out || !indices_out || !n_verts || !n_indices) return fail(RNB_ERR_INVALID, "null argument");
	*verts_out = nullptr; *indices_out = nullptr; *n_verts = 0; *n_indices = 0;
	const uint64_t res3 = (uint64_t)res[0] * res[1] * res[2];
	if (res3 == 0 || res3 >= (1ull << 32)) return fail(RNB_ERR_INVALID, "lattice must hold 1 .. 2^32-1 points");
	hipStream_t s = as_stream(stream);
	if (int rc = ensure_mc_table(c); rc != RNB_OK) return rc;
	McArgs a;
	a.density = density; a.rx = res[0]; a.ry = res[1]; a.rz = res[2]; a.thresh = thresh;
	for (int d = 0; d < 3; ++d) { a.sc[d] = (aabb_max[d] - aabb_min[d]) / (float)res[d]; a.mn[d] = aabb_min[d]; }
	const uint32_t n_wg = groups(res3);
	MeshWorkspace ws;
	uint32_t *wg = nullptr, *scan_scratch = nullptr, *vidx = nullptr, *indices = nullptr;
	float* verts = nullptr;
	if (!ws.alloc(&wg, n_wg) || !ws.alloc(&scan_scratch, scan_scratch_elems(n_wg)) || !ws.alloc(&vidx, (size_t)res3 * 3)) return fail(RNB_ERR_NOMEM, "hipMalloc failed for the marching-cubes scratch (12 bytes per lattice point)");
	uint32_t nv = 0, ni = 0;
	if (int rc = count_and_scan(s, n_wg, wg, scan_scratch, &nv, k_mc_verts<false>, a, wg, (const uint32_t*)nullptr, (float*)nullptr, (uint32_t*)nullptr); rc != RNB_OK) return rc;
	if (nv && !ws.alloc(&verts, (size_t)nv * 3)) return fail(RNB_ERR_NOMEM, "hipMalloc failed for the vertices");
	hipLaunchKernelGGL(k_mc_verts<true>, dim3(n_wg), dim3(MESH_WG), 0, s, a, (uint32_t*)nullptr, wg, verts, vidx);
	if (int rc = count_and_scan(s, n_wg, wg, scan_scratch, &ni, k_mc_faces<false>, a, (const McTable*)c->mc_table.p, wg, (const uint32_t*)nullptr, (const uint32_t*)vidx, (uint32_t*)nullptr); rc != RNB_OK) return rc;
	if (ni && !ws.alloc(&indices, (size_t)ni)) return fail(RNB_ERR_NOMEM, "hipMalloc failed for the indices");
	hipLaunchKernelGGL(k_mc_faces<true>, dim3(n_wg), dim3(MESH_WG), 0, s, a, c->mc_table.p, (uint32_t*)nullptr, wg, (const uint32_t*)vidx, indices);
	if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return fail(RNB_ERR_DEVICE, "rnb_marching_cubes: kernel failure");
	*verts_out = (float*)ws.keep(verts); *indices_out = (uint32_t*)ws.keep(indices); *n_verts = nv; *n_indices = ni; // (null where the count is 0; the scratch goes with ws)
	return RNB_OK;
} RNB_GUARD

// ---- sparse mesh extraction (include/rnb_mesh.h) ----
uint32_t rnb_mesh_abi_version(void) { return RNB_MESH_ABI_VERSION; }

int rnb_mesh_default_options(rnb_mesh_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_ABI_VERSION;
	for (int k = 0; k < 3; ++k) { opt->res[k] = 256; opt->aabb_min[k] = 0.f; opt->aabb_max[k] = 1.f; }
	opt->lattice_min = 0.f; opt->lattice_max = 1.f;
	opt->thresh = 0.f;
	opt->use_inference_params = 1;
	opt->cull = RNB_MESH_CULL_OCCUPANCY;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_free(rnb_ctx* c, rnb_mesh* m) try {
	if (!c || !m) return fail(RNB_ERR_INVALID, "null argument");
	free_device(m, {m->verts, m->indices, m->colors, m->normals});
	return RNB_OK;
} RNB_GUARD

constexpr uint32_t MESH_DEFAULT_BRICK = 16; // measured against 32 (tools/bench_mesh.py, profiles/mesh_sparse.md): fewer points evaluated around the surface
int rnb_extract_mesh(rnb_ctx* c, void* stream, const rnb_mesh_options* opt, rnb_mesh* out, rnb_mesh_stats* stats) try {
	if (!c || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: null argument");
	std::memset(out, 0, sizeof(*out));
	if (opt->abi_version != RNB_MESH_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: options abi_version mismatch (expected RNB_MESH_ABI_VERSION)");
	for (int k = 0; k < 3; ++k) if (opt->res[k] == 0 || opt->res[k] > RNB_MESH_MAX_RES) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: res must be 1 .. 4096 per axis");
	if (opt->cull != RNB_MESH_CULL_NONE && opt->cull != RNB_MESH_CULL_OCCUPANCY) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: unknown cull mode");
	if (opt->attributes & ~(RNB_MESH_ATTR_COLORS | RNB_MESH_ATTR_NORMALS)) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: unknown attribute bits");
	const uint32_t B = opt->brick ? opt->brick : MESH_DEFAULT_BRICK;
	if (B < 8 || B > 64 || (B & (B - 1))) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: brick must be a power of two, 8 .. 64 (0 = default)");
	if (!std::isfinite(opt->lattice_min) || !std::isfinite(opt->lattice_max) || !std::isfinite(opt->thresh)) return fail(RNB_ERR_INVALID, "rnb_extract_mesh: lattice bounds and thresh must be finite");
	MeshCall call("rnb_extract_mesh", c, stream);
	const hipStream_t s = call.s;
	if (int rc = ensure_mc_table(c); rc != RNB_OK) return rc;

	MsArgs a;
	std::memset(&a, 0, sizeof(a));
	a.lb = ilog2(B);
	uint64_t n_bricks64 = 1;
	for (int k = 0; k < 3; ++k) {
		a.r[k] = opt->res[k]; a.nb[k] = (opt->res[k] + B - 1) / B; n_bricks64 *= a.nb[k];
		a.sc[k] = (opt->aabb_max[k] - opt->aabb_min[k]) / (float)opt->res[k]; a.mn[k] = opt->aabb_min[k];
	}
	a.thresh = opt->thresh;
	a.n_bricks = (uint32_t)n_bricks64; // at most (4096 / 8)^3 = 2^27
	const uint32_t lb3 = 3 * a.lb;
	const uint64_t brick_points = 1ull << lb3;
	const bool inference = opt->use_inference_params != 0;

	// 1. which bricks are kept, which are evaluated, and their slots
	const uint32_t n_bwg = groups(a.n_bricks);
	uint32_t *bwg = nullptr, *bscan = nullptr, *list = nullptr;
	if (!call.ws.alloc(&a.word, a.n_bricks) || !call.ws.alloc(&bwg, n_bwg) || !call.ws.alloc(&bscan, scan_scratch_elems(n_bwg))) return call.nomem("hipMalloc failed for the brick words");
	hipLaunchKernelGGL(k_ms_classify, dim3((a.n_bricks + 3) / 4), dim3(256), 0, s, a, (double)opt->lattice_min, (double)opt->lattice_max - (double)opt->lattice_min,
	                   opt->cull == RNB_MESH_CULL_OCCUPANCY ? (const uint8_t*)c->bitfield.p : (const uint8_t*)nullptr);
	uint32_t n_eval = 0;
	int rc = count_and_scan(s, n_bwg, bwg, bscan, &n_eval, k_ms_mark<false>, a, bwg, (const uint32_t*)nullptr, (uint32_t*)nullptr);
	if (rc != RNB_OK) return rc;
	if (!call.ws.alloc(&list, n_eval)) return call.nomem("hipMalloc failed for the brick list");
	a.list = list;
	hipLaunchKernelGGL(k_ms_mark<true>, dim3(n_bwg), dim3(MESH_WG), 0, s, a, (uint32_t*)nullptr, bwg, list);
	HIP_TRY(hipGetLastError());
	uint64_t n_kept = 0;
	{ // the kept count, for the statistics: the evaluated count is the scan's total
		std::vector<uint32_t> h(a.n_bricks);
		HIP_TRY(hipMemcpyAsync(h.data(), a.word, (size_t)a.n_bricks * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		for (uint32_t w : h) n_kept += w & 1u;
	}
	call.ws.release(bwg, bscan);
	const uint64_t n_active_points = (uint64_t)n_eval * brick_points;
	if (opt->max_active_points && n_active_points > opt->max_active_points)
		return call.nomem(std::to_string(n_active_points) + " lattice points would be held at once (" + std::to_string(n_eval) + " bricks of " +
		            std::to_string(B) + "^3), max_active_points is " + std::to_string(opt->max_active_points));
	if (n_eval >= (1u << 30)) return call.invalid("more than 2^30 bricks to evaluate");

	uint32_t n_act = 0, nv = 0, ni = 0;
	float* verts = nullptr;
	uint32_t* indices = nullptr;
	if (n_eval) {
		// 2. the lattice values of the evaluated bricks, through the point-query kernel of rnb_sdf_lattice
		half_t* vals = nullptr;
		float* pos = nullptr;
		uint64_t per_launch = opt->max_points_in_flight ? opt->max_points_in_flight : (1u << 22);
		const uint32_t slots_per_launch = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per_launch >> lb3, 1), n_eval);
		if (!call.ws.alloc(&vals, n_active_points) || !call.ws.alloc(&pos, (size_t)slots_per_launch * brick_points * 3))
			return call.nomem("hipMalloc failed for " + std::to_string(n_active_points) + " lattice values (set max_active_points to fail before allocating, or cull)");
		a.vals = vals;
		const float diag = c->aabb.mx - c->aabb.mn;
		for (uint32_t s0 = 0; s0 < n_eval; s0 += slots_per_launch) {
			const uint32_t np = (uint32_t)(std::min<uint32_t>(slots_per_launch, n_eval - s0) * brick_points); // at most 2^22 or one brick (2^18)
			hipLaunchKernelGGL(k_ms_positions, dim3((np + 255) / 256), dim3(256), 0, s, a, s0, np, opt->lattice_min, opt->lattice_max - opt->lattice_min, c->aabb.mn, diag, pos);
			HIP_TRY(hipGetLastError());
			rc = launch_point_query(c, s, pos, np, vals + (size_t)s0 * brick_points, nullptr, nullptr, 0, inference);
			if (rc != RNB_OK) return rc;
		}
		// 3. which of them see both sides of the threshold; only those keep an edge table
		uint32_t *act = nullptr, *aoff = nullptr, *ascan = nullptr, *alist = nullptr;
		if (!call.ws.alloc(&act, n_eval) || !call.ws.alloc(&aoff, n_eval) || !call.ws.alloc(&ascan, scan_scratch_elems(n_eval))) return call.nomem("hipMalloc failed for the brick flags");
		hipLaunchKernelGGL(k_ms_sign, dim3(n_eval), dim3(256), 0, s, a, act);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(aoff, act, (size_t)n_eval * 4, hipMemcpyDeviceToDevice, s));
		rc = scan_exclusive(aoff, n_eval, s, &n_act, ascan);
		if (rc != RNB_OK) return rc;
		call.ws.release(pos, ascan);
		a.act = act; a.aoff = aoff;
		if (n_act) {
			if ((uint64_t)n_act << (lb3 - 8) >= (1ull << 31)) return call.invalid("too many bricks with a sign change for one launch");
			const uint32_t n_wg = n_act << (lb3 - 8);
			uint32_t *wg = nullptr, *wscan = nullptr, *vidx = nullptr;
			if (!call.ws.alloc(&alist, n_act) || !call.ws.alloc(&wg, n_wg) || !call.ws.alloc(&wscan, scan_scratch_elems(n_wg)) || !call.ws.alloc(&vidx, (size_t)n_act * 3 * brick_points))
				return call.nomem("hipMalloc failed for the edge tables of " + std::to_string(n_act) + " bricks");
			a.alist = alist;
			hipLaunchKernelGGL(k_ms_list, dim3((n_eval + 255) / 256), dim3(256), 0, s, n_eval, act, aoff, alist);
			// 4. vertices, then triangles: count, scan, write (the dense path's scheme over the bricks' workgroups)
			if ((rc = count_and_scan(s, n_wg, wg, wscan, &nv, k_ms_verts<false>, a, wg, (const uint32_t*)nullptr, (float*)nullptr, (uint32_t*)nullptr)) != RNB_OK) return rc;
			if (!call.ws.alloc(&verts, (size_t)nv * 3)) return call.nomem("hipMalloc failed for the vertices");
			hipLaunchKernelGGL(k_ms_verts<true>, dim3(n_wg), dim3(MESH_WG), 0, s, a, (uint32_t*)nullptr, wg, verts, vidx);
			if ((rc = count_and_scan(s, n_wg, wg, wscan, &ni, k_ms_faces<false>, a, (const McTable*)c->mc_table.p, wg, (const uint32_t*)nullptr, (const uint32_t*)vidx, (uint32_t*)nullptr)) != RNB_OK) return rc;
			if (!call.ws.alloc(&indices, (size_t)ni)) return call.nomem("hipMalloc failed for the indices");
			hipLaunchKernelGGL(k_ms_faces<true>, dim3(n_wg), dim3(MESH_WG), 0, s, a, c->mc_table.p, (uint32_t*)nullptr, wg, (const uint32_t*)vidx, indices);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(wg, wscan, vidx, alist);
		}
		call.ws.release(vals, act, aoff);
	}
	call.ws.release(a.word, list);
	if (!verts && !call.ws.alloc(&verts, 1)) return call.nomem("hipMalloc failed for the vertices");
	if (!indices && !call.ws.alloc(&indices, 1)) return call.nomem("hipMalloc failed for the indices");

	// 5. attributes: the full network at the vertices, in batches
	float *colors = nullptr, *normals = nullptr;
	if (opt->attributes) {
		if ((opt->attributes & RNB_MESH_ATTR_COLORS) && !call.ws.alloc(&colors, (size_t)nv * 3)) return call.nomem("hipMalloc failed for the colours");
		if ((opt->attributes & RNB_MESH_ATTR_NORMALS) && !call.ws.alloc(&normals, (size_t)nv * 3)) return call.nomem("hipMalloc failed for the normals");
		const uint32_t batch = std::min<uint32_t>(1u << 20, std::max(nv, 1u));
		float* coords = nullptr;
		half_t* net = nullptr;
		if (!call.ws.alloc(&coords, (size_t)batch * 7) || !call.ws.alloc(&net, (size_t)batch * 16)) return call.nomem("hipMalloc failed for the attribute batch");
		const float diag = c->aabb.mx - c->aabb.mn;
		for (uint32_t v0 = 0; v0 < nv; v0 += batch) {
			const uint32_t nb = std::min(batch, nv - v0);
			hipLaunchKernelGGL(k_ms_vertex_coords, dim3((nb + 255) / 256), dim3(256), 0, s, verts + (size_t)v0 * 3, nb, c->aabb.mn, diag, coords);
			HIP_TRY(hipGetLastError());
			rc = launch_forward(c, s, coords, nullptr, nb, net, inference);
			if (rc != RNB_OK) return rc;
			hipLaunchKernelGGL(k_ms_vertex_attr, dim3((nb + 255) / 256), dim3(256), 0, s, net, nb, colors ? colors + (size_t)v0 * 3 : nullptr, normals ? normals + (size_t)v0 * 3 : nullptr);
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(coords, net);
	}
	HIP_TRY(hipStreamSynchronize(s));
	hand_over(call.ws, rnb_mesh{verts, indices, colors, normals, nv, ni}, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_bricks = a.n_bricks; stats->n_kept = n_kept; stats->n_evaluated = n_eval; stats->n_sign_change = n_act;
		stats->n_points_evaluated = n_active_points;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- mesh cleaning (include/rnb_mesh_clean.h) ----
uint32_t rnb_mesh_clean_abi_version(void) { return RNB_MESH_CLEAN_ABI_VERSION; }

int rnb_mesh_clean_default_options(rnb_mesh_clean_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_CLEAN_ABI_VERSION;
	opt->keep = RNB_MESH_KEEP_LARGEST;
	opt->orient = RNB_MESH_ORIENT_OUTWARD;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_clean_table_free(rnb_ctx* c, rnb_mesh_component* table) try {
	if (!c) return fail(RNB_ERR_INVALID, "null argument");
	if (table) (void)hipFree(table);
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_clean(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_clean_options* opt, rnb_mesh* out, rnb_mesh_component** table_dev, rnb_mesh_clean_stats* stats) try {
	if (table_dev) *table_dev = nullptr;
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_clean: null argument");
	if (int rc = check_mesh_input("rnb_mesh_clean", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_CLEAN_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_clean: options abi_version mismatch (expected RNB_MESH_CLEAN_ABI_VERSION)");
	if (opt->keep != RNB_MESH_KEEP_ALL && opt->keep != RNB_MESH_KEEP_LARGEST) return fail(RNB_ERR_INVALID, "rnb_mesh_clean: unknown keep mode");
	if (opt->orient != RNB_MESH_ORIENT_NONE && opt->orient != RNB_MESH_ORIENT_OUTWARD) return fail(RNB_ERR_INVALID, "rnb_mesh_clean: unknown orient mode");
	MeshCall call("rnb_mesh_clean", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	ClResult hres;
	std::memset(&hres, 0, sizeof(hres));
	hres.best = MESH_NONE;
	uint32_t n_comp = 0, nvo = 0, nto = 0;
	rnb_mesh_component* table = nullptr;
	rnb_mesh o;
	if (nt) {
		const uint32_t g_v = groups(nv), g_t = groups(nt);
		uint32_t *parent = nullptr, *used = nullptr, *cid = nullptr, *scan = nullptr, *twg = nullptr, *cflags = nullptr;
		ClResult* dres = nullptr;
		if (!call.ws.alloc(&parent, nv) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&cid, nv) || !call.ws.alloc(&twg, g_t) || !call.ws.alloc(&scan, scan_scratch_elems(std::max<uint64_t>(nv, g_t))) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices");
		HIP_TRY(hipMemcpyAsync(dres, &hres, sizeof(hres), hipMemcpyHostToDevice, s));
		// 1. every index is range-checked before any is used as an address
		hipLaunchKernelGGL(k_cl_init, dim3(g_v), dim3(MESH_WG), 0, s, parent, nv);
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		// 2. labels: one hooking launch, one flattening launch; roots -> component ids in ascending label order
		hipLaunchKernelGGL(k_cl_hook, dim3(g_t), dim3(MESH_WG), 0, s, (const uint32_t*)m.indices, nt, parent);
		hipLaunchKernelGGL(k_cl_flatten, dim3(g_v), dim3(MESH_WG), 0, s, parent, nv);
		hipLaunchKernelGGL(k_cl_roots, dim3(g_v), dim3(MESH_WG), 0, s, (const uint32_t*)parent, (const uint32_t*)used, cid, nv);
		HIP_TRY(hipGetLastError());
		int rc = scan_exclusive(cid, nv, s, &n_comp, scan);
		if (rc != RNB_OK) return rc;
		if (!call.ws.alloc(&table, n_comp) || !call.ws.alloc(&cflags, n_comp)) return call.nomem("hipMalloc failed for the table of " + std::to_string(n_comp) + " components");
		HIP_TRY(hipMemsetAsync(table, 0, std::max<size_t>(n_comp, 1) * sizeof(rnb_mesh_component), s));
		hipLaunchKernelGGL(k_cl_relabel, dim3(g_v), dim3(MESH_WG), 0, s, parent, (const uint32_t*)used, (const uint32_t*)cid, table, nv);
		const uint32_t* comp = parent;
		// 3. per-component sums, the selection
		hipLaunchKernelGGL(k_cl_sums<true>, dim3(g_t), dim3(MESH_WG), 0, s, (const float*)m.verts, (const uint32_t*)m.indices, nt, comp, table, dres);
		hipLaunchKernelGGL(k_cl_sums<false>, dim3(g_v), dim3(MESH_WG), 0, s, (const float*)nullptr, (const uint32_t*)nullptr, nv, comp, table, dres);
		hipLaunchKernelGGL(k_cl_select, dim3(1), dim3(1024), 0, s, table, n_comp, opt->keep, opt->orient, cflags, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (hres.flags & CL_BAD_TERM) return call.invalid("the area or volume term of a triangle is not finite or not below 2^18");
		call.ws.release(used);
		// 4. compaction: the new vertex numbering (cid's memory is reused), the kept triangles per workgroup
		uint32_t* vmap = cid;
		hipLaunchKernelGGL(k_cl_vflag, dim3(g_v), dim3(MESH_WG), 0, s, comp, (const uint32_t*)cflags, vmap, nv);
		HIP_TRY(hipGetLastError());
		if ((rc = call.compact(m, ClKeep{comp, cflags}, vmap, twg, scan, &o, &nvo, &nto)) != RNB_OK) return rc;
		HIP_TRY(hipStreamSynchronize(s));
		if (n_comp && hres.best < n_comp) { // the label of the selected component, for the statistics
			uint32_t label = MESH_NONE;
			HIP_TRY(hipMemcpy(&label, &table[hres.best].label, 4, hipMemcpyDeviceToHost));
			hres.best = label;
		} else hres.best = MESH_NONE;
		call.ws.release(parent, cid, scan, twg, cflags, dres);
	} else if (!alloc_mesh(call.ws, &o, 0, 0, m.colors != nullptr, m.normals != nullptr) || (table_dev && !call.ws.alloc(&table, 1)))
		return call.nomem("hipMalloc failed for the output mesh");
	hand_over(call.ws, o, out);
	if (table_dev) *table_dev = (rnb_mesh_component*)call.ws.keep(table);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_components = n_comp; stats->n_kept = hres.n_kept;
		stats->n_verts_in = nv; stats->n_verts_out = nvo; stats->n_tris_in = nt; stats->n_tris_out = nto;
		stats->largest_label = hres.best;
		stats->hook_passes = nt ? 1u : 0u; stats->flatten_passes = nt ? 1u : 0u;
		stats->area_q_in = hres.area_in; stats->area_q_out = hres.area_out;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- mesh simplification (include/rnb_mesh_simplify.h) ----
uint32_t rnb_mesh_simplify_abi_version(void) { return RNB_MESH_SIMPLIFY_ABI_VERSION; }

int rnb_mesh_simplify_default_options(rnb_mesh_simplify_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_SIMPLIFY_ABI_VERSION;
	opt->cell = 1.0f / 256.0f;
	opt->dims[0] = opt->dims[1] = opt->dims[2] = 256u;
	opt->placement = RNB_MESH_PLACE_QUADRIC;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_simplify(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_simplify_options* opt, rnb_mesh* out, rnb_mesh_simplify_stats* stats) try {
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: null argument");
	if (int rc = check_mesh_input("rnb_mesh_simplify", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_SIMPLIFY_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: options abi_version mismatch (expected RNB_MESH_SIMPLIFY_ABI_VERSION)");
	if (opt->placement != RNB_MESH_PLACE_QUADRIC && opt->placement != RNB_MESH_PLACE_MEAN) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: unknown placement");
	if (!(opt->cell > 0.0f) || !std::isfinite(opt->cell)) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: cell must be finite and > 0");
	uint64_t n_cells = 1;
	for (int k = 0; k < 3; ++k) {
		if (!std::isfinite(opt->origin[k])) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: origin must be finite");
		if (opt->dims[k] == 0 || opt->dims[k] > RNB_MESH_SIMPLIFY_MAX_DIM) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: dims must be 1 .. 4096 per axis");
		n_cells *= opt->dims[k];
	}
	if (n_cells > RNB_MESH_SIMPLIFY_MAX_CELLS) return fail(RNB_ERR_INVALID, "rnb_mesh_simplify: dims hold " + std::to_string(n_cells) + " cells, more than RNB_MESH_SIMPLIFY_MAX_CELLS (2^30)");
	MeshCall call("rnb_mesh_simplify", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	SpResult hres;
	std::memset(&hres, 0, sizeof(hres));
	uint32_t n_cl = 0, nvo = 0, nto = 0;
	rnb_mesh o;
	if (nt) {
		SpGrid g;
		for (int k = 0; k < 3; ++k) { g.origin[k] = (double)opt->origin[k]; g.dims[k] = opt->dims[k]; }
		g.cell = (double)opt->cell;
		const uint32_t n_words = (uint32_t)((n_cells + 31u) / 32u);
		const uint32_t g_v = groups(nv), g_t = groups(nt), g_w = groups(n_words);
		uint32_t *used = nullptr, *vcl = nullptr, *bits = nullptr, *rank = nullptr, *scan = nullptr, *twg = nullptr, *ckey = nullptr, *cused = nullptr, *cmap = nullptr;
		long long* sums = nullptr;
		SpResult* dres = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&vcl, nv) || !call.ws.alloc(&bits, n_words) || !call.ws.alloc(&rank, n_words) || !call.ws.alloc(&twg, g_t) ||
		    !call.ws.alloc(&scan, scan_scratch_elems(std::max<uint64_t>(std::max<uint64_t>(nv, n_words), g_t))) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices and " + std::to_string(n_cells) + " cells");
		HIP_TRY(hipMemsetAsync(bits, 0, (size_t)n_words * 4, s));
		HIP_TRY(hipMemcpyAsync(dres, &hres, sizeof(hres), hipMemcpyHostToDevice, s));
		// 1. every index is range-checked before any is used as an address (the flag arrives with the result below: no synchronise of its own); the occupied cells;
		//    cluster ids = ranks of the occupied keys
		if (int rc = call.check_indices_launch(m, used, &dres->flags); rc != RNB_OK) return rc;
		hipLaunchKernelGGL(k_sp_cells, dim3(g_v), dim3(MESH_WG), 0, s, g, (const float*)m.verts, (const float*)m.colors, (const float*)m.normals, nv, (const uint32_t*)used, vcl, bits, dres);
		hipLaunchKernelGGL(k_sp_popc, dim3(g_w), dim3(MESH_WG), 0, s, (const uint32_t*)bits, rank, n_words);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		int rc = scan_exclusive(rank, n_words, s, &n_cl, scan); // (synchronises: hres has arrived)
		if (rc != RNB_OK) return rc;
		if (hres.flags & MESH_BAD_INDEX) return call.bad_index();
		if (hres.flags & SP_BAD_VALUE) return call.invalid("a coordinate or attribute of a used vertex is not finite");
		call.ws.release(used);
		// 2. the sums of every cluster
		if (!call.ws.alloc(&sums, (size_t)n_cl * SP_NSUM) || !call.ws.alloc(&ckey, n_cl) || !call.ws.alloc(&cused, n_cl) || !call.ws.alloc(&cmap, n_cl))
			return call.nomem("hipMalloc failed for the records of " + std::to_string(n_cl) + " clusters");
		HIP_TRY(hipMemsetAsync(sums, 0, std::max<size_t>(n_cl, 1) * SP_NSUM * sizeof(long long), s));
		HIP_TRY(hipMemsetAsync(cused, 0, std::max<size_t>(n_cl, 1) * 4, s));
		hipLaunchKernelGGL(k_sp_members, dim3(g_v), dim3(MESH_WG), 0, s, g, (const float*)m.verts, (const float*)m.colors, (const float*)m.normals, nv, (const uint32_t*)bits, (const uint32_t*)rank, vcl, ckey, sums, dres);
		hipLaunchKernelGGL(k_sp_quadric, dim3(g_t), dim3(MESH_WG), 0, s, g, (const float*)m.verts, (const uint32_t*)m.indices, nt, (const uint32_t*)vcl, sums, dres);
		// 3. the surviving triangles and the clusters they use, numbered by prefix sums (not count_and_scan: the count launch feeds two scans, the clusters' first)
		hipLaunchKernelGGL(k_sp_tris<false>, dim3(g_t), dim3(MESH_WG), 0, s, (const uint32_t*)m.indices, nt, (const uint32_t*)vcl, cused, (const uint32_t*)nullptr, twg, (const uint32_t*)nullptr, (uint32_t*)nullptr);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(cmap, cused, std::max<size_t>(n_cl, 1) * 4, hipMemcpyDeviceToDevice, s));
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		rc = scan_exclusive(cmap, n_cl, s, &nvo, scan);
		if (rc != RNB_OK) return rc;
		if (hres.flags & SP_BAD_TERM) return call.invalid("a term is not finite or not below 2^22 (a vertex or triangle too far from its cell, in cell units)");
		rc = scan_exclusive(twg, g_t, s, &nto, scan);
		if (rc != RNB_OK) return rc;
		call.ws.release(bits, rank);
		// 4. the output: one solve per cluster, the triangles in input order
		if ((rc = call.alloc_like(m, &o, nvo, nto)) != RNB_OK) return rc;
		hipLaunchKernelGGL(k_sp_solve, dim3(groups(n_cl)), dim3(MESH_WG), 0, s, g, opt->placement, n_cl, (const long long*)sums, (const uint32_t*)ckey, (const uint32_t*)cused, (const uint32_t*)cmap,
		                   o.verts, o.colors, o.normals, dres);
		hipLaunchKernelGGL(k_sp_tris<true>, dim3(g_t), dim3(MESH_WG), 0, s, (const uint32_t*)m.indices, nt, (const uint32_t*)vcl, (uint32_t*)nullptr, (const uint32_t*)cmap, (uint32_t*)nullptr, (const uint32_t*)twg, o.indices);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(vcl, scan, twg, sums, ckey, cused, cmap, dres);
	} else if (int rc = call.alloc_like(m, &o, 0, 0); rc != RNB_OK)
		return rc;
	hand_over(call.ws, o, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_verts_in = nv; stats->n_tris_in = nt; stats->n_clusters = n_cl; stats->n_verts_out = nvo; stats->n_tris_out = nto; stats->n_tris_collapsed = nt - nto;
		stats->n_clamped = hres.n_clamped; stats->n_fallback = hres.n_fallback;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- mesh-to-mesh distance (include/rnb_mesh_distance.h) ----
extern "C++" {
namespace {
// The search grid of rnb_mesh_distance.h and its cell lists, for the distance stage and for the self-intersection stage (rnb_mesh_intersect.h), which searches a mesh's
// own box: hres->bmin / bmax hold the box of B's used vertices (k_md_verts<true>), m = B's non-degenerate triangles (>= 1), cells = the option. *g, and start / cursor
// (the beginning and the end of every cell's list), entries and the large list (hres->n_large, n_entries) as k_md_register leaves them; `of` names B in a failure.
int md_build_lists(MeshCall& call, const MdMesh& B, uint32_t cells, uint32_t m, const char* of, uint32_t* large, MdResult* dres, MdResult* hres, MdGrid* grid, uint32_t** start_out, uint32_t** cursor_out,
                   uint32_t** scan_out, uint32_t** entries_out) {
	const hipStream_t s = call.s;
	const uint32_t g_tb = groups(B.nt);
	MdGrid g;
	std::memset(&g, 0, sizeof(g));
	uint32_t *start = nullptr, *cursor = nullptr, *scan = nullptr, *entries = nullptr, n_entries = 0;
	double longest = 0.0;
	for (int k = 0; k < 3; ++k) {
		const auto value = [](uint32_t image) { const uint32_t u = (image & 0x80000000u) ? (image ^ 0x80000000u) : ~image; float f; std::memcpy(&f, &u, 4); return (double)f; };
		g.lo[k] = value(hres->bmin[k]); g.hi[k] = value(hres->bmax[k]);
		longest = std::max(longest, g.hi[k] - g.lo[k]);
	}
	uint32_t n_axis = cells;
	if (!n_axis) n_axis = (uint32_t)std::min<double>(std::max<double>(std::floor(std::sqrt((double)(m / 2u))), 1.0), (double)RNB_MESH_DISTANCE_MAX_CELLS);
	g.cell = longest / (double)n_axis; // > 0: a non-degenerate triangle has an extent
	uint64_t n_cells = 1;
	for (int k = 0; k < 3; ++k) {
		g.dims[k] = (uint32_t)std::min<double>((double)n_axis, std::floor((g.hi[k] - g.lo[k]) / g.cell) + 1.0);
		n_cells *= g.dims[k];
	}
	if (!call.ws.alloc(&start, n_cells) || !call.ws.alloc(&cursor, n_cells) || !call.ws.alloc(&scan, scan_scratch_elems(n_cells)))
		return call.nomem("hipMalloc failed for the lists of " + std::to_string(n_cells) + " cells");
	HIP_TRY(hipMemsetAsync(start, 0, (size_t)n_cells * 4, s));
	hipLaunchKernelGGL(k_md_register<false>, dim3(g_tb), dim3(MESH_WG), 0, s, g, B, start, (uint32_t*)nullptr, large, dres);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hres, dres, sizeof(*hres), hipMemcpyDeviceToHost, s));
	int rc = scan_exclusive(start, n_cells, s, &n_entries, scan); // (synchronises: hres has arrived)
	if (rc != RNB_OK) return rc;
	if (hres->n_large > RNB_MESH_DISTANCE_MAX_LARGE)
		return call.invalid(std::to_string(hres->n_large) + " triangles " + of + "overlap more than 2048 cells each, the large list holds 4096 (a coarser grid: fewer cells)");
	if (hres->n_entries > RNB_MESH_DISTANCE_MAX_ENTRIES)
		return call.invalid(std::to_string(hres->n_entries) + " cell entries, more than 2^31 (a coarser grid: fewer cells)");
	if (!call.ws.alloc(&entries, n_entries)) return call.nomem("hipMalloc failed for " + std::to_string(n_entries) + " cell entries");
	HIP_TRY(hipMemcpyAsync(cursor, start, (size_t)n_cells * 4, hipMemcpyDeviceToDevice, s));
	hipLaunchKernelGGL(k_md_register<true>, dim3(g_tb), dim3(MESH_WG), 0, s, g, B, cursor, entries, (uint32_t*)nullptr, dres);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	*grid = g; *start_out = start; *cursor_out = cursor; *scan_out = scan; *entries_out = entries;
	return RNB_OK;
}
} // namespace
} // extern "C++"

uint32_t rnb_mesh_distance_abi_version(void) { return RNB_MESH_DISTANCE_ABI_VERSION; }

int rnb_mesh_distance_default_options(rnb_mesh_distance_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_DISTANCE_ABI_VERSION;
	opt->level = 1u;
	opt->unit = 1.0f / 1024.0f;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_distance(rnb_ctx* c, void* stream, const rnb_mesh* from, const rnb_mesh* to, const rnb_mesh_distance_options* opt, float* vert_dist_dev, uint32_t* vert_nearest_dev,
                      rnb_mesh_distance_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !from || !to || !opt) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: null argument");
	if (from == to) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: from and to must be different objects");
	if (vert_dist_dev && (void*)vert_dist_dev == (void*)vert_nearest_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: vert_dist_dev and vert_nearest_dev must be different buffers");
	if (opt->abi_version != RNB_MESH_DISTANCE_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: options abi_version mismatch (expected RNB_MESH_DISTANCE_ABI_VERSION)");
	if (opt->level > RNB_MESH_DISTANCE_MAX_LEVEL) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: level must be 0 .. 3");
	if (!(opt->unit > 0.0f) || !std::isfinite(opt->unit)) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: unit must be finite and > 0");
	if (!(opt->max_distance >= 0.0f) || !std::isfinite(opt->max_distance)) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: max_distance must be finite and >= 0");
	for (int k = 0; k < RNB_MESH_DISTANCE_MAX_TAUS; ++k)
		if (!(opt->tau[k] >= 0.0f) || !std::isfinite(opt->tau[k])) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: a tau must be finite and >= 0");
	if (opt->cells > RNB_MESH_DISTANCE_MAX_CELLS) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: cells must be 0 .. 256");
	if (int rc = check_mesh_input("rnb_mesh_distance (from)", from); rc != RNB_OK) return rc;
	if (int rc = check_mesh_input("rnb_mesh_distance (to)", to); rc != RNB_OK) return rc;
	const rnb_mesh ma = *from, mb = *to;
	const uint32_t nva = ma.n_verts, nta = ma.n_indices / 3u, nvb = mb.n_verts, ntb = mb.n_indices / 3u, nn = 1u << (2u * opt->level);
	if ((uint64_t)nta * nn > 0xFFFFFFFFull) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: more than 2^32 - 1 samples (a lower level)");
	if (nta && ntb == 0) return fail(RNB_ERR_INVALID, "rnb_mesh_distance: to has no non-degenerate triangle");
	MeshCall call("rnb_mesh_distance", c, stream);
	const hipStream_t s = call.s;

	MdResult hres;
	std::memset(&hres, 0, sizeof(hres));
	for (int k = 0; k < 3; ++k) hres.bmin[k] = 0xFFFFFFFFu;
	MdGrid g;
	std::memset(&g, 0, sizeof(g));
	float ms_grid = 0.0f;
	int64_t sums[MD_NSUM] = {};
	if (!nta) { // no sample: every vertex is unused
		if (vert_dist_dev && nva) HIP_TRY(hipMemsetAsync(vert_dist_dev, 0, (size_t)nva * 4, s));
		if (vert_nearest_dev && nva) HIP_TRY(hipMemsetAsync(vert_nearest_dev, 0xFF, (size_t)nva * 4, s));
		HIP_TRY(hipStreamSynchronize(s));
	} else {
		const uint32_t g_va = groups(nva), g_vb = groups(nvb), g_tb = groups(ntb);
		const MdMesh A{ma.verts, ma.indices, nva, nta}, B{mb.verts, mb.indices, nvb, ntb};
		uint32_t *used_a = nullptr, *used_b = nullptr, *start = nullptr, *cursor = nullptr, *scan = nullptr, *entries = nullptr, *large = nullptr;
		MdResult* dres = nullptr;
		if (!call.ws.alloc(&used_a, nva) || !call.ws.alloc(&used_b, nvb) || !call.ws.alloc(&large, RNB_MESH_DISTANCE_MAX_LARGE) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nva) + " and " + std::to_string(nvb) + " vertices");
		HIP_TRY(hipMemcpyAsync(dres, &hres, sizeof(hres), hipMemcpyHostToDevice, s));
		// 1. every index of either mesh is range-checked before any is used as an address (both under one synchronise); used vertices, B's box, B's degenerate triangles
		if (int rc = call.check_indices_launch(ma, used_a, &dres->flags); rc != RNB_OK) return rc;
		if (int rc = call.check_indices_launch(mb, used_b, &dres->flags, MD_BAD_INDEX_TO); rc != RNB_OK) return rc;
		if (int rc = call.read_flags(&dres->flags, &hres.flags); rc != RNB_OK) return rc;
		if (hres.flags & MESH_BAD_INDEX) return call.bad_index("of from ");
		if (hres.flags & MD_BAD_INDEX_TO) return call.bad_index("of to ");
		hipLaunchKernelGGL(k_md_verts<false>, dim3(g_va), dim3(MESH_WG), 0, s, (const float*)ma.verts, nva, (const uint32_t*)used_a, dres);
		hipLaunchKernelGGL(k_md_verts<true>, dim3(g_vb), dim3(MESH_WG), 0, s, (const float*)mb.verts, nvb, (const uint32_t*)used_b, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (hres.flags & MD_BAD_VALUE) return call.invalid("a coordinate of a used vertex is not finite");
		call.ws.release(used_b);
		const auto t_grid = std::chrono::steady_clock::now();
		hipLaunchKernelGGL(k_md_degenerate, dim3(g_tb), dim3(MESH_WG), 0, s, B, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		const uint32_t m = ntb - hres.n_deg_to;
		if (!m) return call.invalid("to has no non-degenerate triangle");
		// 2. the grid over B's box, the cell lists
		if (int rc = md_build_lists(call, B, opt->cells, m, "of to ", large, dres, &hres, &g, &start, &cursor, &scan, &entries); rc != RNB_OK) return rc;
		ms_grid = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_grid).count();
		// 3. the queries: the vertices of A, then the sub-centroids of its triangles
		MdQuery q;
		std::memset(&q, 0, sizeof(q));
		q.cap = (double)opt->max_distance; q.unit = (double)opt->unit; q.level = opt->level;
		for (int k = 0; k < RNB_MESH_DISTANCE_MAX_TAUS; ++k) q.tau[k] = (double)opt->tau[k];
		const MdSearch S{B, start, cursor, entries, large, hres.n_large};
		const uint64_t n_threads = (uint64_t)nta * nn;
		hipLaunchKernelGGL(k_md_query<true>, dim3(g_va), dim3(MESH_WG), 0, s, g, q, A, (const uint32_t*)used_a, S, vert_dist_dev, vert_nearest_dev, dres);
		hipLaunchKernelGGL(k_md_query<false>, dim3(groups(n_threads)), dim3(MESH_WG), 0, s, g, q, A, (const uint32_t*)nullptr, S, (float*)nullptr, (uint32_t*)nullptr, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (hres.flags & MD_BAD_TERM)
			return call.invalid("a term is not finite or not below 2^12 (a larger unit, or a max_distance)");
		for (int k = 0; k < MD_NSUM; ++k) { // the two words of a sum, joined in 128 bits
			const unsigned __int128 total = ((unsigned __int128)hres.hi[k] << 32) + hres.lo[k];
			if (total >> 63) return call.invalid("a sum reaches 2^15 (a larger unit, or a max_distance)");
			sums[k] = (int64_t)total;
		}
		call.ws.release(used_a, start, cursor, scan, entries, large, dres);
	}
	if (stats) {
		stats->n_verts_from_used = hres.n_used_from; stats->n_verts_to_used = hres.n_used_to; stats->n_tris_from = nta; stats->n_tris_to = ntb;
		stats->n_degenerate_from = hres.n_deg_from; stats->n_degenerate_to = hres.n_deg_to; stats->n_verts_beyond = hres.n_verts_beyond; stats->n_large = hres.n_large;
		stats->n_samples = hres.n_samples; stats->n_beyond = hres.n_beyond;
		stats->sum_w = sums[0]; stats->sum_wd = sums[1]; stats->sum_wd2 = sums[2];
		for (int k = 0; k < RNB_MESH_DISTANCE_MAX_TAUS; ++k) stats->sum_within[k] = sums[3 + k];
		std::memcpy(&stats->max_distance, &hres.max_bits, 8);
		for (int k = 0; k < 3; ++k) stats->dims[k] = g.dims[k];
		stats->cell = g.cell;
		stats->n_cell_entries = hres.n_entries; stats->n_pairs = hres.n_pairs;
		stats->ms_grid = ms_grid;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- mesh rasteriser (include/rnb_mesh_raster.h) ----
uint32_t rnb_mesh_raster_abi_version(void) { return RNB_MESH_RASTER_ABI_VERSION; }

int rnb_mesh_raster_default_options(rnb_mesh_raster_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_RASTER_ABI_VERSION;
	opt->near = 1.0f / 1024.0f;
	opt->cull = RNB_MESH_RASTER_CULL_NONE;
	opt->normals = RNB_MESH_RASTER_NORMALS_FACE;
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
// What the rasteriser, the draw, the visibility stage and the projection ask of near and cull, and of a camera, said in the entry point's name.
int check_near_cull(const char* name, float near, uint32_t cull) {
	const std::string n(name);
	if (!(near > 0.0f) || !std::isfinite(near)) return fail(RNB_ERR_INVALID, n + ": near must be finite and > 0");
	if (cull > RNB_MESH_RASTER_CULL_FRONT) return fail(RNB_ERR_INVALID, n + ": cull must be RNB_MESH_RASTER_CULL_NONE, _BACK or _FRONT");
	return RNB_OK;
}
int check_raster_view(const char* name, const rnb_view* view) {
	const std::string n(name);
	for (int k = 0; k < 2; ++k) {
		if (!(view->focal_length[k] > 0.0f) || !std::isfinite(view->focal_length[k])) return fail(RNB_ERR_INVALID, n + ": a focal length must be finite and > 0");
		if (!std::isfinite(view->principal_point[k])) return fail(RNB_ERR_INVALID, n + ": the principal point must be finite");
	}
	for (int k = 0; k < 12; ++k)
		if (!std::isfinite(view->xform[k])) return fail(RNB_ERR_INVALID, n + ": an entry of xform is not finite");
	if (view->width == 0 || view->height == 0 || view->width > RNB_MESH_RASTER_MAX_SIZE || view->height > RNB_MESH_RASTER_MAX_SIZE)
		return fail(RNB_ERR_INVALID, n + ": width and height must be 1 .. 16384");
	return RNB_OK;
}
MrCamera raster_camera(const rnb_view* view, float near, uint32_t cull, uint32_t normals) {
	MrCamera cam;
	std::memset(&cam, 0, sizeof(cam));
	for (int r = 0; r < 3; ++r) {
		cam.o[r] = (double)view->xform[4 * r + 3];
		for (int k = 0; k < 3; ++k) cam.col[k][r] = (double)view->xform[4 * r + k];
	}
	cam.fx = (double)view->focal_length[0]; cam.fy = (double)view->focal_length[1];
	cam.cxw = (double)view->principal_point[0] * (double)view->width; cam.cyh = (double)view->principal_point[1] * (double)view->height;
	cam.near = (double)near;
	cam.w = view->width; cam.h = view->height; cam.cull = cull; cam.normals = normals;
	return cam;
}
// What the fill of a view starts from: the keys of its pixels all ones, their counts zero, *dres and *hres zero.
int raster_clear(hipStream_t s, const MrCamera& cam, unsigned long long* keys, uint32_t* counts, MrResult* dres, MrResult* hres) {
	const size_t n_pix = (size_t)cam.w * cam.h;
	std::memset(hres, 0, sizeof(*hres));
	HIP_TRY(hipMemsetAsync(keys, 0xFF, n_pix * 8, s));
	HIP_TRY(hipMemsetAsync(counts, 0, n_pix * 4, s));
	HIP_TRY(hipMemcpyAsync(dres, hres, sizeof(*hres), hipMemcpyHostToDevice, s));
	return RNB_OK;
}
// The fill of one view, for the rasteriser (VIS = false, an empty tally) and the visibility stage (VIS = true): setup, classes, the small triangles filled; the large
// ones counted, then listed and filled by a wavefront each. On entry the state of raster_clear (and for VIS the tally's words zero); *hres is *dres after the first
// pass (synchronises). The list grows when a view needs a longer one and is the caller's to release; `name` is who is named if it cannot be allocated. M.nt >= 1, the
// indices are range-checked.
template <bool VIS>
int raster_fill(const char* name, MeshCall& call, const MrCamera& cam, const MrMesh& M, unsigned long long* keys, uint32_t* counts, MrResult* dres, MrResult* hres, uint32_t** list,
                uint32_t* list_cap, const MrTally& tally) {
	const hipStream_t s = call.s;
	const uint32_t g_t = groups(M.nt);
	hipLaunchKernelGGL((k_mr_bin<false, VIS>), dim3(g_t), dim3(MESH_WG), 0, s, cam, M, keys, counts, (uint32_t*)nullptr, 0u, dres, tally);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hres, dres, sizeof(*hres), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint32_t n_large = hres->n_class[MR_LARGE];
	if (n_large) {
		if (n_large > *list_cap) {
			call.ws.release(*list);
			*list_cap = 0;
			if (!call.ws.alloc(list, n_large)) return fail(RNB_ERR_NOMEM, std::string(name) + ": hipMalloc failed for the list of " + std::to_string(n_large) + " large triangles");
			*list_cap = n_large;
		}
		hipLaunchKernelGGL((k_mr_bin<true, VIS>), dim3(g_t), dim3(MESH_WG), 0, s, cam, M, keys, counts, *list, n_large, dres, tally);
		hipLaunchKernelGGL(k_mr_fill_large<VIS>, dim3((n_large + MESH_WG / 64u - 1) / (MESH_WG / 64u)), dim3(MESH_WG), 0, s, cam, M, (const uint32_t*)*list, n_large, keys, counts, tally);
		HIP_TRY(hipGetLastError());
	}
	return RNB_OK;
}
// What rnb_mesh_raster and rnb_mesh_draw_textured ask of near, cull, normals, the camera and the mesh, said in the entry point's name.
int check_raster_call(const char* name, float near, uint32_t cull, uint32_t normals, const rnb_view* view, const rnb_mesh* mesh) {
	const std::string n(name);
	if (int rc = check_near_cull(name, near, cull); rc != RNB_OK) return rc;
	if (normals > RNB_MESH_RASTER_NORMALS_VERTEX) return fail(RNB_ERR_INVALID, n + ": normals must be RNB_MESH_RASTER_NORMALS_FACE or _VERTEX");
	if (int rc = check_raster_view(name, view); rc != RNB_OK) return rc;
	if (int rc = check_mesh_input(name, mesh); rc != RNB_OK) return rc;
	if (normals == RNB_MESH_RASTER_NORMALS_VERTEX && !mesh->normals) return fail(RNB_ERR_INVALID, n + ": normals = VERTEX needs a mesh with normals");
	return RNB_OK;
}
// The textured resolve of include/rnb_mesh_draw.h: the instantiation the filter, the maps given and the image's alignment select.
template <int FILTER, bool COLOR, bool NORMAL>
void launch_md_resolve(uint32_t g_p, hipStream_t s, const MrCamera& cam, const MrMesh& M, const DrawTexture& tex, const unsigned long long* keys, const uint32_t* counts, float* out_dev, uint32_t* face_dev,
                       MrResult* dres, DrawResult* ddraw) {
	if (((uintptr_t)out_dev & 15u) == 0)
		hipLaunchKernelGGL((k_md_resolve<FILTER, COLOR, NORMAL, true>), dim3(g_p), dim3(MESH_WG), 0, s, cam, M, tex, keys, counts, out_dev, face_dev, dres, ddraw);
	else
		hipLaunchKernelGGL((k_md_resolve<FILTER, COLOR, NORMAL, false>), dim3(g_p), dim3(MESH_WG), 0, s, cam, M, tex, keys, counts, out_dev, face_dev, dres, ddraw);
}
template <int FILTER>
void launch_md_resolve(uint32_t g_p, hipStream_t s, const MrCamera& cam, const MrMesh& M, const DrawTexture& tex, const unsigned long long* keys, const uint32_t* counts, float* out_dev, uint32_t* face_dev,
                       MrResult* dres, DrawResult* ddraw) {
	if (tex.color && tex.normal) launch_md_resolve<FILTER, true, true>(g_p, s, cam, M, tex, keys, counts, out_dev, face_dev, dres, ddraw);
	else if (tex.color) launch_md_resolve<FILTER, true, false>(g_p, s, cam, M, tex, keys, counts, out_dev, face_dev, dres, ddraw);
	else launch_md_resolve<FILTER, false, true>(g_p, s, cam, M, tex, keys, counts, out_dev, face_dev, dres, ddraw);
}
// One view of a mesh, for rnb_mesh_raster (tex null) and rnb_mesh_draw_textured (tex, filter, *drawn): the range check, the fill and the resolve of whichever of the two,
// on arguments the caller has checked. *stats (may be null) is zero on entry.
int raster_image(const char* name, rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_view* view, float near, uint32_t cull, uint32_t normals, const DrawTexture* tex, uint32_t filter,
                 float* out_dev, uint32_t* face_dev, rnb_mesh_raster_stats* stats, DrawResult* drawn) {
	const rnb_mesh m = *mesh;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, n_pix = view->width * view->height;
	MeshCall call(name, c, stream);
	const hipStream_t s = call.s;

	const MrCamera cam = raster_camera(view, near, cull, normals);
	const MrMesh M{m.verts, m.indices, m.colors, m.normals, nt};

	MrResult hres;
	unsigned long long* keys = nullptr;
	uint32_t *counts = nullptr, *used = nullptr, *list = nullptr;
	MrResult* dres = nullptr;
	DrawResult* ddraw = nullptr;
	if (!call.ws.alloc(&keys, n_pix) || !call.ws.alloc(&counts, n_pix) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&dres, 1) || (tex && !call.ws.alloc(&ddraw, 1)))
		return call.nomem("hipMalloc failed for the workspace of " + std::to_string(n_pix) + " pixels and " + std::to_string(nv) + " vertices");
	if (int rc = raster_clear(s, cam, keys, counts, dres, &hres); rc != RNB_OK) return rc;
	if (tex) HIP_TRY(hipMemsetAsync(ddraw, 0, sizeof(DrawResult), s));
	if (nt) {
		// 1. every index is range-checked before any is used as an address
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		call.ws.release(used);
		// 2. setup, classes, the small triangles filled; the large ones counted, then listed and filled by a wavefront each (the fill is the rasteriser's for both callers,
		//    and names the rasteriser if its list cannot be allocated)
		uint32_t list_cap = 0;
		if (int rc = raster_fill<false>("rnb_mesh_raster", call, cam, M, keys, counts, dres, &hres, &list, &list_cap, MrTally{}); rc != RNB_OK) return rc;
	}
	// 3. one thread per pixel (an empty mesh: every key is still all ones, the image is zeros)
	const uint32_t g_p = groups(n_pix);
	if (tex) {
		if (filter == RNB_MESH_DRAW_FILTER_NEAREST) launch_md_resolve<RNB_MESH_DRAW_FILTER_NEAREST>(g_p, s, cam, M, *tex, keys, counts, out_dev, face_dev, dres, ddraw);
		else launch_md_resolve<RNB_MESH_DRAW_FILTER_BILINEAR>(g_p, s, cam, M, *tex, keys, counts, out_dev, face_dev, dres, ddraw);
	} else if (((uintptr_t)out_dev & 15u) == 0)
		hipLaunchKernelGGL(k_mr_resolve<true>, dim3(g_p), dim3(MESH_WG), 0, s, cam, M, (const unsigned long long*)keys, (const uint32_t*)counts, out_dev, face_dev, dres);
	else
		hipLaunchKernelGGL(k_mr_resolve<false>, dim3(g_p), dim3(MESH_WG), 0, s, cam, M, (const unsigned long long*)keys, (const uint32_t*)counts, out_dev, face_dev, dres);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
	if (tex) HIP_TRY(hipMemcpyAsync(drawn, ddraw, sizeof(DrawResult), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	call.ws.release(keys, counts, used, list, dres, ddraw);
	if (hres.n_unresolved) return call.device(std::to_string(hres.n_unresolved) + " pixels whose winner the resolve pass does not find covering them (the fill and the resolve disagree: a defect of the library)");
	if (stats) {
		stats->n_tris = nt;
		stats->n_behind = hres.n_class[MR_BEHIND]; stats->n_out_of_range = hres.n_class[MR_OUT_OF_RANGE]; stats->n_degenerate = hres.n_class[MR_DEGENERATE];
		stats->n_culled = hres.n_class[MR_CULLED]; stats->n_offscreen = hres.n_class[MR_OFFSCREEN]; stats->n_small = hres.n_class[MR_SMALL]; stats->n_large = hres.n_class[MR_LARGE];
		stats->n_covered = hres.n_covered; stats->n_back_pixels = hres.n_back_pixels; stats->n_fragments = hres.n_fragments;
		call.finish(stats);
	}
	return RNB_OK;
}
} // namespace
} // extern "C++"

int rnb_mesh_raster(rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_view* view, const rnb_mesh_raster_options* opt, float* out_dev, uint32_t* face_dev,
                    rnb_mesh_raster_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !mesh || !view || !opt || !out_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_raster: null argument");
	if ((void*)out_dev == (void*)face_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_raster: out_dev and face_dev must be different buffers");
	if (opt->abi_version != RNB_MESH_RASTER_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_raster: options abi_version mismatch (expected RNB_MESH_RASTER_ABI_VERSION)");
	if (int rc = check_raster_call("rnb_mesh_raster", opt->near, opt->cull, opt->normals, view, mesh); rc != RNB_OK) return rc;
	return raster_image("rnb_mesh_raster", c, stream, mesh, view, opt->near, opt->cull, opt->normals, nullptr, 0u, out_dev, face_dev, stats, nullptr);
} RNB_GUARD

// ---- textured draw (include/rnb_mesh_draw.h) ----
uint32_t rnb_mesh_draw_abi_version(void) { return RNB_MESH_DRAW_ABI_VERSION; }

int rnb_mesh_draw_default_options(rnb_mesh_draw_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_DRAW_ABI_VERSION;
	opt->near = 1.0f / 1024.0f;
	opt->cull = RNB_MESH_RASTER_CULL_NONE;
	opt->normals = RNB_MESH_RASTER_NORMALS_FACE;
	opt->filter = RNB_MESH_DRAW_FILTER_BILINEAR;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_draw_textured(rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_mesh_draw_texture* tex, const rnb_view* view, const rnb_mesh_draw_options* opt, float* out_dev,
                           uint32_t* face_dev, rnb_mesh_draw_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !mesh || !tex || !view || !opt || !out_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: null argument");
	if ((void*)out_dev == (void*)face_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: out_dev and face_dev must be different buffers");
	if (opt->abi_version != RNB_MESH_DRAW_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: options abi_version mismatch (expected RNB_MESH_DRAW_ABI_VERSION)");
	if (opt->filter > RNB_MESH_DRAW_FILTER_BILINEAR) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: filter must be RNB_MESH_DRAW_FILTER_NEAREST or _BILINEAR");
	if (int rc = check_reserved("rnb_mesh_draw_textured", opt->reserved); rc != RNB_OK) return rc;
	if (int rc = check_raster_call("rnb_mesh_draw_textured", opt->near, opt->cull, opt->normals, view, mesh); rc != RNB_OK) return rc;
	if (!tex->color_dev && !tex->normal_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: no map (color_dev and normal_dev are both null)");
	if (((uintptr_t)tex->color_dev | (uintptr_t)tex->normal_dev) & 15u) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: a map is not aligned to 16 bytes");
	if (tex->size == 0 || tex->size > RNB_MESH_TEXTURE_MAX_SIZE) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: size must be 1 .. " + std::to_string(RNB_MESH_TEXTURE_MAX_SIZE));
	if (tex->n_tris != mesh->n_indices / 3u) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: the texture is of " + std::to_string(tex->n_tris) + " triangles, the mesh has " + std::to_string(mesh->n_indices / 3u));
	if (tex->n_tris && !tex->uv_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_draw_textured: uv_dev is null");
	const DrawTexture T{tex->uv_dev, tex->color_dev, tex->normal_dev, tex->size};
	DrawResult drawn;
	std::memset(&drawn, 0, sizeof(drawn));
	const int rc = raster_image("rnb_mesh_draw_textured", c, stream, mesh, view, opt->near, opt->cull, opt->normals, &T, opt->filter, out_dev, face_dev, stats ? &stats->raster : nullptr, &drawn);
	if (stats && rc == RNB_OK) { stats->n_bad_uv = drawn.n_bad_uv; stats->n_normal_fallback = drawn.n_fallback; stats->n_unowned_taps = drawn.n_unowned; }
	return rc;
} RNB_GUARD

// ---- visibility (include/rnb_mesh_visibility.h) ----
uint32_t rnb_mesh_visibility_abi_version(void) { return RNB_MESH_VISIBILITY_ABI_VERSION; }

int rnb_mesh_visibility_default_options(rnb_mesh_visibility_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_VISIBILITY_ABI_VERSION;
	opt->near = 1.0f / 1024.0f;
	opt->cull = RNB_MESH_RASTER_CULL_NONE;
	opt->min_pixels = 1u;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_visibility_select_default_options(rnb_mesh_visibility_select_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_VISIBILITY_ABI_VERSION;
	opt->unit = RNB_MESH_VISIBILITY_UNIT_COMPONENT;
	opt->min_views_seen = 1u;
	opt->max_views_off_mask = 0xFFFFFFFFu;
	opt->rings = 1u;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_visibility(rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_mesh_visibility_view* views, uint32_t n_views, const rnb_mesh_visibility_options* opt,
                        rnb_mesh_face_visibility* faces_dev, rnb_mesh_visibility_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !mesh || !views || !opt || !faces_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility: null argument");
	if (n_views == 0) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility: n_views must be at least 1");
	if (opt->abi_version != RNB_MESH_VISIBILITY_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility: options abi_version mismatch (expected RNB_MESH_VISIBILITY_ABI_VERSION)");
	if (int rc = check_near_cull("rnb_mesh_visibility", opt->near, opt->cull); rc != RNB_OK) return rc;
	if (opt->min_pixels == 0) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility: min_pixels must be at least 1");
	if (int rc = check_reserved("rnb_mesh_visibility", opt->reserved); rc != RNB_OK) return rc;
	uint32_t max_pix = 0;
	uint64_t n_pixels = 0;
	for (uint32_t v = 0; v < n_views; ++v) {
		if (int rc = check_raster_view("rnb_mesh_visibility", &views[v].view); rc != RNB_OK) return rc;
		if (views[v].mask_dev && (views[v].mask_width == 0 || views[v].mask_height == 0)) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility: view " + std::to_string(v) + " has a mask of size 0");
		const uint32_t n = views[v].view.width * views[v].view.height; // at most 2^28
		max_pix = std::max(max_pix, n);
		n_pixels += n;
	}
	if (int rc = check_mesh_input("rnb_mesh_visibility", mesh); rc != RNB_OK) return rc;
	const rnb_mesh m = *mesh;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	MeshCall call("rnb_mesh_visibility", c, stream);
	const hipStream_t s = call.s;

	uint64_t n_class[MR_NCLASS] = {};
	MvResult hv;
	std::memset(&hv, 0, sizeof(hv));
	if (nt) {
		const MrMesh M{m.verts, m.indices, nullptr, nullptr, nt};
		const uint32_t g_t = groups(nt);
		unsigned long long* keys = nullptr;
		uint32_t *counts = nullptr, *used = nullptr, *list = nullptr, *words = nullptr, list_cap = 0;
		MrResult* dres = nullptr;
		MvResult* dv = nullptr;
		if (!call.ws.alloc(&keys, max_pix) || !call.ws.alloc(&counts, max_pix) || !call.ws.alloc(&words, (size_t)nt * 3) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&dres, 1) || !call.ws.alloc(&dv, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(max_pix) + " pixels, " + std::to_string(nt) + " triangles and " + std::to_string(nv) + " vertices");
		uint32_t *cov = words, *on = words + nt, *won = words + 2 * (size_t)nt;
		// 1. every index is range-checked before any is used as an address
		HIP_TRY(hipMemsetAsync(words, 0, (size_t)nt * 12, s));
		HIP_TRY(hipMemcpyAsync(dv, &hv, sizeof(hv), hipMemcpyHostToDevice, s));
		if (int rc = call.check_indices(m, used, &dv->flags); rc != RNB_OK) return rc;
		call.ws.release(used);
		// 2. view by view: the rasteriser's fill, the winners tallied, the three words of every triangle folded into its record
		for (uint32_t v = 0; v < n_views; ++v) {
			const rnb_mesh_visibility_view& V = views[v];
			const uint32_t n_pix = V.view.width * V.view.height;
			const MrCamera cam = raster_camera(&V.view, opt->near, opt->cull, RNB_MESH_RASTER_NORMALS_FACE);
			const MrTally tally{V.mask_dev, V.mask_width, V.mask_height, cov, on};
			MrResult hres;
			if (int rc = raster_clear(s, cam, keys, counts, dres, &hres); rc != RNB_OK) return rc;
			if (int rc = raster_fill<true>("rnb_mesh_visibility", call, cam, M, keys, counts, dres, &hres, &list, &list_cap, tally); rc != RNB_OK) return rc;
			for (uint32_t k = 0; k < MR_NCLASS; ++k) n_class[k] += hres.n_class[k];
			hipLaunchKernelGGL(k_mv_tally, dim3(groups(n_pix)), dim3(MESH_WG), 0, s, V.view.width, V.view.height, nt, tally, (const unsigned long long*)keys, won);
			hipLaunchKernelGGL(k_mv_fold, dim3(g_t), dim3(MESH_WG), 0, s, nt, v, v == 0 ? 1u : 0u, v + 1 == n_views ? 1u : 0u, V.mask_dev ? 1u : 0u, opt->min_pixels, cov, on, won, faces_dev, dv);
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(hipMemcpyAsync(&hv, dv, sizeof(hv), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(keys, counts, words, list, dres, dv);
	}
	if (stats) {
		stats->n_tris = nt; stats->n_views = n_views;
		stats->n_behind = n_class[MR_BEHIND]; stats->n_out_of_range = n_class[MR_OUT_OF_RANGE]; stats->n_degenerate = n_class[MR_DEGENERATE]; stats->n_culled = n_class[MR_CULLED];
		stats->n_offscreen = n_class[MR_OFFSCREEN]; stats->n_small = n_class[MR_SMALL]; stats->n_large = n_class[MR_LARGE];
		stats->n_pixels = n_pixels;
		stats->n_faces_seen = hv.n_faces_seen; stats->n_faces_off_mask = hv.n_faces_off_mask;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_visibility_select(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_face_visibility* faces_dev, const rnb_mesh_visibility_select_options* opt, rnb_mesh* out,
                               uint32_t* kept_dev, rnb_mesh_visibility_select_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility_select: null argument");
	if (int rc = check_mesh_input("rnb_mesh_visibility_select", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_VISIBILITY_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility_select: options abi_version mismatch (expected RNB_MESH_VISIBILITY_ABI_VERSION)");
	if (opt->unit != RNB_MESH_VISIBILITY_UNIT_COMPONENT && opt->unit != RNB_MESH_VISIBILITY_UNIT_FACE) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility_select: unknown unit");
	if (opt->rings > RNB_MESH_VISIBILITY_MAX_RINGS) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility_select: rings must be 0 .. 64");
	if (int rc = check_reserved("rnb_mesh_visibility_select", opt->reserved); rc != RNB_OK) return rc;
	if (m.n_indices && !faces_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_visibility_select: faces_dev is null");
	MeshCall call("rnb_mesh_visibility_select", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	MvResult hv;
	std::memset(&hv, 0, sizeof(hv));
	uint32_t nvo = 0, nto = 0;
	rnb_mesh o;
	if (nt) {
		const uint32_t g_v = groups(nv), g_t = groups(nt);
		const uint32_t* idx = m.indices;
		uint32_t *used = nullptr, *flag = nullptr, *vmark = nullptr, *parent = nullptr, *vmap = nullptr, *scan = nullptr, *twg = nullptr;
		MvResult* dv = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&flag, nt) || !call.ws.alloc(&vmark, nv) || !call.ws.alloc(&vmap, nv) || !call.ws.alloc(&twg, g_t) || !call.ws.alloc(&scan, scan_scratch_elems(std::max<uint64_t>(nv, g_t))) ||
		    !call.ws.alloc(&dv, 1) || (opt->unit == RNB_MESH_VISIBILITY_UNIT_COMPONENT && !call.ws.alloc(&parent, nv)))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices and " + std::to_string(nt) + " triangles");
		HIP_TRY(hipMemsetAsync(vmark, 0, (size_t)nv * 4, s));
		HIP_TRY(hipMemcpyAsync(dv, &hv, sizeof(hv), hipMemcpyHostToDevice, s));
		// 1. every index is range-checked before any is used as an address
		if (int rc = call.check_indices(m, used, &dv->flags); rc != RNB_OK) return rc;
		// 2. candidates and seeds; the kept triangles
		hipLaunchKernelGGL(k_mv_flags, dim3(g_t), dim3(MESH_WG), 0, s, faces_dev, nt, opt->min_views_seen, opt->max_views_off_mask, flag, dv);
		if (opt->unit == RNB_MESH_VISIBILITY_UNIT_FACE) {
			hipLaunchKernelGGL(k_mv_seeds_kept, dim3(g_t), dim3(MESH_WG), 0, s, flag, nt);
			for (uint32_t r = 0; r < opt->rings; ++r) { // (the marks of the earlier rings stay: their triangles are still marked)
				hipLaunchKernelGGL(k_mv_ring_mark, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, (const uint32_t*)flag, vmark);
				hipLaunchKernelGGL(k_mv_ring_grow, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, flag, (const uint32_t*)vmark);
			}
		} else { // the cleaner's labels: the root of a component is its smallest vertex
			hipLaunchKernelGGL(k_cl_init, dim3(g_v), dim3(MESH_WG), 0, s, parent, nv);
			hipLaunchKernelGGL(k_cl_hook, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, parent);
			hipLaunchKernelGGL(k_cl_flatten, dim3(g_v), dim3(MESH_WG), 0, s, parent, nv);
			hipLaunchKernelGGL(k_mv_comp_seed, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, (const uint32_t*)flag, (const uint32_t*)parent, vmark);
			hipLaunchKernelGGL(k_mv_comp_keep, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, flag, (const uint32_t*)parent, (const uint32_t*)vmark);
			hipLaunchKernelGGL(k_mv_comp_count, dim3(g_v), dim3(MESH_WG), 0, s, (const uint32_t*)parent, (const uint32_t*)used, (const uint32_t*)vmark, nv, dv);
		}
		HIP_TRY(hipGetLastError());
		// 3. compaction: the kept vertices numbered (used's memory holds their flags), the kept triangles per workgroup
		uint32_t* vkeep = used;
		HIP_TRY(hipMemsetAsync(vkeep, 0, (size_t)nv * 4, s));
		hipLaunchKernelGGL(k_mv_vflag, dim3(g_t), dim3(MESH_WG), 0, s, idx, nt, (const uint32_t*)flag, vkeep, kept_dev);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(vmap, vkeep, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
		if (int rc = call.compact(m, MvKeep{flag, vkeep}, vmap, twg, scan, &o, &nvo, &nto); rc != RNB_OK) return rc;
		HIP_TRY(hipMemcpyAsync(&hv, dv, sizeof(hv), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(used, flag, vmark, parent, vmap, scan, twg, dv);
	} else if (int rc = call.alloc_like(m, &o, 0, 0); rc != RNB_OK)
		return rc;
	hand_over(call.ws, o, out);
	if (stats) {
		stats->n_verts_in = nv; stats->n_verts_out = nvo; stats->n_tris_in = nt; stats->n_tris_out = nto;
		stats->n_seeds = hv.n_seeds; stats->n_candidates = hv.n_candidates; stats->n_components = hv.n_components; stats->n_components_kept = hv.n_components_kept;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- texture baker (include/rnb_mesh_texture.h) ----
uint32_t rnb_mesh_texture_abi_version(void) { return RNB_MESH_TEXTURE_ABI_VERSION; }

int rnb_mesh_texture_default_options(rnb_mesh_texture_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_TEXTURE_ABI_VERSION;
	opt->size = 1024u;
	opt->maps = RNB_MESH_TEXTURE_ALBEDO;
	opt->use_inference_params = 1;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_texture_layout(uint32_t n_tris, uint32_t size, uint32_t block, uint32_t* block_out, uint32_t* blocks_per_row_out, uint32_t* n_blocks_out) try {
	if (block_out) *block_out = 0;
	if (blocks_per_row_out) *blocks_per_row_out = 0;
	if (n_blocks_out) *n_blocks_out = 0;
	if (size < RNB_MESH_TEXTURE_MIN_SIZE || size > RNB_MESH_TEXTURE_MAX_SIZE) return fail(RNB_ERR_INVALID, "rnb_mesh_texture_layout: size must be 4 .. 8192");
	const uint64_t n_blocks = ((uint64_t)n_tris + 1u) / 2u;
	uint64_t m = (uint64_t)std::sqrt((double)n_blocks); // m = ceil(sqrt(n_blocks)): the blocks per row the mesh needs
	while (m * m > n_blocks) --m;
	while (m * m < n_blocks) ++m;
	const auto smallest = [&](uint64_t b) { return ": the smallest size that would fit is " + std::to_string(std::max<uint64_t>(b * std::max<uint64_t>(m, 1), RNB_MESH_TEXTURE_MIN_SIZE)); };
	uint32_t b = block;
	if (block == 0) {
		b = m ? (uint32_t)(size / m) : size;
		if (b < RNB_MESH_TEXTURE_MIN_BLOCK)
			return fail(RNB_ERR_INVALID, "rnb_mesh_texture_layout: " + std::to_string(n_tris) + " triangles do not fit a texture of " + std::to_string(size) + " texels per side in blocks of 4" + smallest(RNB_MESH_TEXTURE_MIN_BLOCK));
	} else {
		if (block < RNB_MESH_TEXTURE_MIN_BLOCK) return fail(RNB_ERR_INVALID, "rnb_mesh_texture_layout: block must be 0 or at least 4" + smallest(RNB_MESH_TEXTURE_MIN_BLOCK));
		if (block > size || (uint64_t)(size / block) < m)
			return fail(RNB_ERR_INVALID, "rnb_mesh_texture_layout: " + std::to_string(n_tris) + " triangles do not fit a texture of " + std::to_string(size) + " texels per side in blocks of " + std::to_string(block) + smallest(block));
	}
	if (block_out) *block_out = b;
	if (blocks_per_row_out) *blocks_per_row_out = size / b;
	if (n_blocks_out) *n_blocks_out = (uint32_t)n_blocks;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_texture_free(rnb_ctx* c, rnb_mesh_texture* tex) try {
	if (!c || !tex) return fail(RNB_ERR_INVALID, "null argument");
	free_device(tex, {tex->uv, tex->albedo, tex->normal, tex->position});
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
// The atlas of rnb_mesh_texture_layout for nt triangles, for the baker and the projection (the layout's own failures).
int make_atlas(uint32_t nt, uint32_t size, uint32_t block, MtAtlas* A) {
	std::memset(A, 0, sizeof(*A));
	uint32_t n_blocks = 0;
	if (int rc = rnb_mesh_texture_layout(nt, size, block, &A->block, &A->bpr, &n_blocks); rc != RNB_OK) return rc;
	A->size = size; A->n_tris = nt;
	A->n_texels = n_blocks * A->block * A->block; // at most size * size = 2^26
	return RNB_OK;
}
} // namespace
} // extern "C++"

int rnb_mesh_bake_texture(rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_mesh_texture_options* opt, rnb_mesh_texture* out, rnb_mesh_texture_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (out) std::memset(out, 0, sizeof(*out));
	if (!c || !mesh || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_bake_texture: null argument");
	if (opt->abi_version != RNB_MESH_TEXTURE_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_bake_texture: options abi_version mismatch (expected RNB_MESH_TEXTURE_ABI_VERSION)");
	if (opt->size < RNB_MESH_TEXTURE_MIN_SIZE || opt->size > RNB_MESH_TEXTURE_MAX_SIZE) return fail(RNB_ERR_INVALID, "rnb_mesh_bake_texture: size must be 4 .. 8192");
	if (opt->maps == 0 || (opt->maps & ~(RNB_MESH_TEXTURE_ALBEDO | RNB_MESH_TEXTURE_NORMAL | RNB_MESH_TEXTURE_POSITION)))
		return fail(RNB_ERR_INVALID, "rnb_mesh_bake_texture: maps must be a non-empty set of RNB_MESH_TEXTURE_ALBEDO, _NORMAL and _POSITION");
	if (int rc = check_reserved("rnb_mesh_bake_texture", opt->reserved); rc != RNB_OK) return rc;
	if (int rc = check_mesh_input("rnb_mesh_bake_texture", mesh); rc != RNB_OK) return rc;
	const rnb_mesh m = *mesh;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, S = opt->size;
	MtAtlas A;
	if (int rc = make_atlas(nt, S, opt->block, &A); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_bake_texture", c, stream);
	const hipStream_t s = call.s;

	const size_t n_pix = (size_t)S * S;
	const bool network = (opt->maps & (RNB_MESH_TEXTURE_ALBEDO | RNB_MESH_TEXTURE_NORMAL)) != 0;
	float* uv = nullptr;
	f4* map[3] = {nullptr, nullptr, nullptr}; // albedo, normal, position
	if (!call.ws.alloc(&uv, (size_t)nt * 6)) return call.nomem("hipMalloc failed for the UVs of " + std::to_string(nt) + " triangles");
	for (int k = 0; k < 3; ++k)
		if (opt->maps & (1u << k)) {
			if (!call.ws.alloc(&map[k], n_pix)) return call.nomem("hipMalloc failed for a map of " + std::to_string(S) + "^2 texels");
			HIP_TRY(hipMemsetAsync(map[k], 0, n_pix * sizeof(f4), s));
		}
	uint32_t n_batches = 0;
	if (nt) {
		// 1. every index is range-checked before any is used as an address
		uint32_t *used = nullptr, *dflags = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&dflags, 1)) return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices");
		HIP_TRY(hipMemsetAsync(dflags, 0, 4, s));
		if (int rc = call.check_indices(m, used, dflags); rc != RNB_OK) return rc;
		call.ws.release(used, dflags);
		// 2. the texels, in batches: positions, the corners' UVs and network inputs, the network, the maps
		const uint32_t per_launch = std::min<uint32_t>(opt->max_texels_in_flight ? opt->max_texels_in_flight : (1u << 20), RNB_MESH_TEXTURE_MAX_IN_FLIGHT);
		const uint32_t batch = std::min(per_launch, A.n_texels);
		float* coords = nullptr;
		half_t* net = nullptr;
		if (network && (!call.ws.alloc(&coords, (size_t)batch * 7) || !call.ws.alloc(&net, (size_t)batch * 16))) return call.nomem("hipMalloc failed for a batch of " + std::to_string(batch) + " texels");
		const float diag = c->aabb.mx - c->aabb.mn;
		const bool inference = opt->use_inference_params != 0;
		for (uint32_t w0 = 0; w0 < A.n_texels; w0 += batch) {
			const uint32_t nb = std::min(batch, A.n_texels - w0);
			hipLaunchKernelGGL(k_mt_texels, dim3(groups(nb)), dim3(MESH_WG), 0, s, A, (const float*)m.verts, (const uint32_t*)m.indices, w0, nb, c->aabb.mn, diag, uv, map[2], coords);
			HIP_TRY(hipGetLastError());
			if (!network) continue;
			if (int rc = launch_forward(c, s, coords, nullptr, nb, net, inference); rc != RNB_OK) return rc;
			hipLaunchKernelGGL(k_mt_maps, dim3(groups(nb)), dim3(MESH_WG), 0, s, A, (const half_t*)net, w0, nb, map[0], map[1]);
			HIP_TRY(hipGetLastError());
			++n_batches;
		}
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(coords, net);
	}
	HIP_TRY(hipStreamSynchronize(s));
	out->uv = (float*)call.ws.keep(uv);
	out->albedo = (float*)call.ws.keep(map[0]); out->normal = (float*)call.ws.keep(map[1]); out->position = (float*)call.ws.keep(map[2]);
	out->size = S; out->block = A.block; out->blocks_per_row = A.bpr; out->n_tris = nt;
	if (stats) {
		stats->n_texels = network ? A.n_texels : 0u;
		stats->n_batches = n_batches;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- view projection (include/rnb_mesh_project.h) ----
uint32_t rnb_mesh_project_abi_version(void) { return RNB_MESH_PROJECT_ABI_VERSION; }

int rnb_mesh_project_default_options(rnb_mesh_project_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_PROJECT_ABI_VERSION;
	opt->size = 1024u;
	opt->mode = RNB_MESH_PROJECT_MODE_BLEND;
	opt->normals = RNB_MESH_PROJECT_NORMALS_FACE;
	opt->weight_power = 2u;
	opt->min_cos = 0.1f;
	opt->depth_tolerance = 1.0f / 256.0f;
	opt->near = 1.0f / 1024.0f;
	opt->cull = RNB_MESH_RASTER_CULL_NONE;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_projection_free(rnb_ctx* c, rnb_mesh_projection* out) try {
	if (!c || !out) return fail(RNB_ERR_INVALID, "null argument");
	free_device(out, {out->uv, out->color, out->info});
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
constexpr bool MP_FILL_TALLIES = false; // the projection reads the keys of the fill and none of the visibility stage's tallies
template <int FMT>
void launch_mp_accumulate(hipStream_t s, const MrCamera& cam, const MpState& st, const unsigned long long* keys, const MpImage& img, const MpParams& P, MpResult* dres) {
	hipLaunchKernelGGL(k_mp_accumulate<FMT>, dim3(groups(st.n)), dim3(MESH_WG), 0, s, cam, st, keys, img, P, dres);
}
} // namespace
} // extern "C++"

int rnb_mesh_project_views(rnb_ctx* c, void* stream, const rnb_mesh* mesh, const rnb_mesh_project_view* views, uint32_t n_views, const rnb_mesh_project_options* opt,
                           rnb_mesh_projection* out, rnb_mesh_project_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (out) std::memset(out, 0, sizeof(*out));
	if (!c || !mesh || !views || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: null argument");
	if (n_views == 0) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: n_views must be at least 1");
	if (opt->abi_version != RNB_MESH_PROJECT_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: options abi_version mismatch (expected RNB_MESH_PROJECT_ABI_VERSION)");
	if (opt->size < RNB_MESH_TEXTURE_MIN_SIZE || opt->size > RNB_MESH_TEXTURE_MAX_SIZE) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: size must be 4 .. 8192");
	if (opt->mode > RNB_MESH_PROJECT_MODE_BEST) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: mode must be RNB_MESH_PROJECT_MODE_BLEND or _BEST");
	if (opt->normals > RNB_MESH_PROJECT_NORMALS_VERTEX) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: normals must be RNB_MESH_PROJECT_NORMALS_FACE or _VERTEX");
	if (opt->weight_power > RNB_MESH_PROJECT_MAX_WEIGHT_POWER) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: weight_power must be 0 .. 8");
	if (!(opt->min_cos >= 0.0f && opt->min_cos < 1.0f)) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: min_cos must be in [0, 1)");
	if (!(opt->depth_tolerance >= 0.0f) || !std::isfinite(opt->depth_tolerance)) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: depth_tolerance must be finite and >= 0");
	if (int rc = check_near_cull("rnb_mesh_project_views", opt->near, opt->cull); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_project_views", opt->reserved); rc != RNB_OK) return rc;
	if (opt->fallback_dev && ((uintptr_t)opt->fallback_dev & 15u)) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: fallback_dev is not aligned to 16 bytes");
	uint32_t max_pix = 0;
	for (uint32_t v = 0; v < n_views; ++v) {
		const rnb_mesh_project_view& V = views[v];
		const std::string who = "rnb_mesh_project_views: view " + std::to_string(v);
		if (int rc = check_raster_view("rnb_mesh_project_views", &V.view); rc != RNB_OK) return rc;
		if (!V.image_dev) return fail(RNB_ERR_INVALID, who + " has a null image");
		if (V.image_width == 0 || V.image_height == 0) return fail(RNB_ERR_INVALID, who + " has an image of size 0");
		if (V.format > RNB_MESH_PROJECT_FORMAT_U8) return fail(RNB_ERR_INVALID, who + " has an unknown format");
		if ((uintptr_t)V.image_dev & (V.format == RNB_MESH_PROJECT_FORMAT_F32 ? 15u : V.format == RNB_MESH_PROJECT_FORMAT_U16 ? 7u : 3u)) return fail(RNB_ERR_INVALID, who + " has an image that is not aligned to one pixel");
		if (V.reserved) return fail(RNB_ERR_INVALID, who + " has a reserved word that is not 0");
		max_pix = std::max(max_pix, V.view.width * V.view.height); // at most 2^28
	}
	if (int rc = check_mesh_input("rnb_mesh_project_views", mesh); rc != RNB_OK) return rc;
	if (opt->normals == RNB_MESH_PROJECT_NORMALS_VERTEX && !mesh->normals) return fail(RNB_ERR_INVALID, "rnb_mesh_project_views: normals = VERTEX needs a mesh with normals");
	const rnb_mesh m = *mesh;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, S = opt->size;
	MtAtlas A;
	if (int rc = make_atlas(nt, S, opt->block, &A); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_project_views", c, stream);
	const hipStream_t s = call.s;

	const size_t n_pix = (size_t)S * S, n = A.n_texels;
	float* uv = nullptr;
	f4* color = nullptr;
	mp_u2* info = nullptr;
	MpResult hres;
	std::memset(&hres, 0, sizeof(hres));
	if (!call.ws.alloc(&uv, (size_t)nt * 6) || !call.ws.alloc(&color, n_pix) || !call.ws.alloc(&info, n_pix))
		return call.nomem("hipMalloc failed for the maps of " + std::to_string(S) + "^2 texels and the UVs of " + std::to_string(nt) + " triangles");
	HIP_TRY(hipMemsetAsync(color, 0, n_pix * sizeof(f4), s));
	HIP_TRY(hipMemsetAsync(info, 0, n_pix * sizeof(mp_u2), s));
	if (nt) {
		const MrMesh M{m.verts, m.indices, nullptr, nullptr, nt};
		unsigned long long* keys = nullptr;
		uint32_t *counts = nullptr, *used = nullptr, *list = nullptr, list_cap = 0;
		MrResult* dfill = nullptr;
		MpResult* dres = nullptr;
		MpState st;
		std::memset(&st, 0, sizeof(st));
		st.n = A.n_texels;
		if (!call.ws.alloc(&keys, max_pix) || !call.ws.alloc(&counts, max_pix) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&dfill, 1) || !call.ws.alloc(&dres, 1) || !call.ws.alloc(&st.p, 3 * n) || !call.ws.alloc(&st.nrm, 3 * n) ||
		    !call.ws.alloc(&st.acc, 4 * n) || !call.ws.alloc(&st.w_best, n) || !call.ws.alloc(&st.count, n) || !call.ws.alloc(&st.best, n))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(max_pix) + " pixels, " + std::to_string(n) + " texels and " + std::to_string(nv) + " vertices");
		// 1. every index is range-checked before any is used as an address
		HIP_TRY(hipMemcpyAsync(dres, &hres, sizeof(hres), hipMemcpyHostToDevice, s));
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		call.ws.release(used);
		// 2. p and N of every texel, the accumulators cleared
		const uint32_t g_w = groups(A.n_texels);
		hipLaunchKernelGGL(k_mp_setup, dim3(g_w), dim3(MESH_WG), 0, s, A, (const float*)m.verts, (const uint32_t*)m.indices, (const float*)m.normals, opt->normals, st);
		HIP_TRY(hipGetLastError());
		// 3. view by view: the rasteriser's fill, then every texel against its keys and its image
		MpParams P;
		std::memset(&P, 0, sizeof(P));
		P.min_cos = (double)opt->min_cos; P.slack = 1.0 + (double)opt->depth_tolerance;
		P.power = opt->weight_power; P.mode = opt->mode;
		for (uint32_t v = 0; v < n_views; ++v) {
			const rnb_mesh_project_view& V = views[v];
			const MrCamera cam = raster_camera(&V.view, opt->near, opt->cull, RNB_MESH_RASTER_NORMALS_FACE);
			MrResult hfill;
			if (int rc = raster_clear(s, cam, keys, counts, dfill, &hfill); rc != RNB_OK) return rc;
			if (int rc = raster_fill<MP_FILL_TALLIES>("rnb_mesh_project_views", call, cam, M, keys, counts, dfill, &hfill, &list, &list_cap, MrTally{}); rc != RNB_OK) return rc;
			const MpImage img{V.image_dev, V.image_width, V.image_height};
			P.view = v;
			if (V.format == RNB_MESH_PROJECT_FORMAT_F32) launch_mp_accumulate<RNB_MESH_PROJECT_FORMAT_F32>(s, cam, st, keys, img, P, dres);
			else if (V.format == RNB_MESH_PROJECT_FORMAT_U16) launch_mp_accumulate<RNB_MESH_PROJECT_FORMAT_U16>(s, cam, st, keys, img, P, dres);
			else launch_mp_accumulate<RNB_MESH_PROJECT_FORMAT_U8>(s, cam, st, keys, img, P, dres);
			HIP_TRY(hipGetLastError());
		}
		// 4. the result
		hipLaunchKernelGGL(k_mp_finish, dim3(g_w), dim3(MESH_WG), 0, s, A, st, (const f4*)opt->fallback_dev, uv, color, info, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(keys, counts, list, dfill, dres, st.p, st.nrm, st.acc, st.w_best, st.count, st.best);
	}
	HIP_TRY(hipStreamSynchronize(s));
	out->uv = (float*)call.ws.keep(uv); out->color = (float*)call.ws.keep(color); out->info = (uint32_t*)call.ws.keep(info);
	out->size = S; out->block = A.block; out->blocks_per_row = A.bpr; out->n_tris = nt;
	if (stats) {
		stats->n_texels = hres.n_texels; stats->n_textured = hres.n_textured; stats->n_pairs_tested = hres.n_tested; stats->n_occluded = hres.n_occluded;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD


// ---- mesh topology: census and repair (include/rnb_mesh_topology.h) ----
uint32_t rnb_mesh_topology_abi_version(void) { return RNB_MESH_TOPOLOGY_ABI_VERSION; }

int rnb_mesh_topology_default_options(rnb_mesh_topology_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_TOPOLOGY_ABI_VERSION;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_repair_default_options(rnb_mesh_repair_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_TOPOLOGY_ABI_VERSION;
	opt->drop_degenerate = 1;
	opt->duplicates = RNB_MESH_DUPLICATES_FIRST;
	opt->orient = RNB_MESH_REPAIR_ORIENT_NONE;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_topology_table_free(rnb_ctx* c, rnb_mesh_topology_component* table) try {
	if (!c) return fail(RNB_ERR_INVALID, "null argument");
	if (table) (void)hipFree(table);
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
// The hash join of kernels_mesh_topology.cuh over n items: buckets counted, the guard, offsets, lists filled. j->join is ready for a walk; the caller releases j->offs and
// j->items after it.
struct TpTable { uint32_t* offs = nullptr; uint32_t* items = nullptr; TpJoin join{nullptr, nullptr, 0}; };
template <typename KEYS>
int tp_join(MeshCall& call, const KEYS& keys, uint32_t n, uint32_t forced_log2, TpResult* dres, TpTable* j) {
	uint32_t log2 = forced_log2;
	if (!log2) for (log2 = 4; log2 < 30 && (1ull << log2) < 2ull * n; ++log2) {}
	const uint32_t n_buckets = 1u << log2;
	uint32_t* scan = nullptr;
	if (!call.ws.alloc(&j->offs, n_buckets) || !call.ws.alloc(&j->items, n) || !call.ws.alloc(&scan, scan_scratch_elems(n_buckets)))
		return call.nomem("hipMalloc failed for " + std::to_string(n_buckets) + " buckets of " + std::to_string(n) + " items");
	HIP_TRY(hipMemsetAsync(j->offs, 0, (size_t)n_buckets * 4, call.s));
	call.launch(groups(n), k_tp_count<KEYS>, keys, n, log2, j->offs);
	call.launch(groups(n_buckets), k_tp_max_load, (const uint32_t*)j->offs, n_buckets, dres);
	HIP_TRY(hipGetLastError());
	uint32_t fullest = 0, total = 0;
	HIP_TRY(hipMemcpyAsync(&fullest, &dres->max_bucket, 4, hipMemcpyDeviceToHost, call.s));
	HIP_TRY(hipStreamSynchronize(call.s));
	if (fullest > RNB_MESH_TOPOLOGY_MAX_BUCKET)
		return call.invalid("a bucket of the grouping holds " + std::to_string(fullest) + " items (more than RNB_MESH_TOPOLOGY_MAX_BUCKET = 65536): an edge, triangle or position is repeated that often" +
		                    (forced_log2 ? ", or buckets_log2 forces too few buckets" : ""));
	if (int rc = scan_exclusive(j->offs, n_buckets, call.s, &total, scan); rc != RNB_OK) return rc;
	call.ws.release(scan);
	call.launch(groups(n), k_tp_fill<KEYS>, keys, n, log2, j->offs, j->items);
	HIP_TRY(hipGetLastError());
	j->join = TpJoin{j->offs, j->items, log2};
	return RNB_OK;
}
int tp_check_buckets(const char* name, uint32_t b) {
	return (b == 0 || (b >= 4 && b <= 30)) ? RNB_OK : fail(RNB_ERR_INVALID, std::string(name) + ": buckets_log2 must be 0 or 4 .. 30");
}
} // namespace
} // extern "C++"

int rnb_mesh_topology(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_topology_options* opt, uint32_t* n_faces, uint32_t* n_same, uint32_t* mate,
                      rnb_mesh_topology_component** table_dev, rnb_mesh_topology_stats* stats) try {
	if (table_dev) *table_dev = nullptr;
	if (!c || !in || !opt) return fail(RNB_ERR_INVALID, "rnb_mesh_topology: null argument");
	if (int rc = check_mesh_input("rnb_mesh_topology", in); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_TOPOLOGY_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_topology: options abi_version mismatch (expected RNB_MESH_TOPOLOGY_ABI_VERSION)");
	if (int rc = tp_check_buckets("rnb_mesh_topology", opt->buckets_log2); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_topology", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_topology", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	TpResult hres;
	std::memset(&hres, 0, sizeof(hres));
	uint32_t n_comp = 0;
	rnb_mesh_topology_component* table = nullptr;
	if (nt) {
		const uint32_t g_v = groups(nv), g_t = groups(nt), g_h = groups(m.n_indices);
		uint32_t *parent = nullptr, *used = nullptr, *cid = nullptr, *scan = nullptr;
		TpResult* dres = nullptr;
		if (!call.ws.alloc(&parent, nv) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&cid, nv) || !call.ws.alloc(&scan, scan_scratch_elems(nv)) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices");
		HIP_TRY(hipMemsetAsync(dres, 0, sizeof(hres), s));
		// 1. every index is range-checked before any is used as an address
		call.launch(g_v, k_cl_init, parent, nv);
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		// 2. the cleaner's components; the table's labels and vertex counts
		call.launch(g_t, k_cl_hook, (const uint32_t*)m.indices, nt, parent);
		call.launch(g_v, k_cl_flatten, parent, nv);
		call.launch(g_v, k_cl_roots, (const uint32_t*)parent, (const uint32_t*)used, cid, nv);
		HIP_TRY(hipGetLastError());
		if (int rc = scan_exclusive(cid, nv, s, &n_comp, scan); rc != RNB_OK) return rc;
		if (!call.ws.alloc(&table, n_comp)) return call.nomem("hipMalloc failed for the table of " + std::to_string(n_comp) + " components");
		HIP_TRY(hipMemsetAsync(table, 0, std::max<size_t>(n_comp, 1) * sizeof(rnb_mesh_topology_component), s));
		call.launch(g_v, k_tp_relabel, parent, (const uint32_t*)used, (const uint32_t*)cid, table, nv);
		const uint32_t* comp = parent;
		call.launch(g_v, k_tp_comp_sums, comp, nv, table, dres);
		HIP_TRY(hipGetLastError());
		call.ws.release(used, cid, scan);
		const TpTris tris{(const uint32_t*)m.indices, nullptr};
		// 3. triangles by vertex set: degenerate ones, duplicates, folded pairs
		{
			TpTable j;
			const TpTriKeys keys{tris};
			if (int rc = tp_join(call, keys, nt, opt->buckets_log2, dres, &j); rc != RNB_OK) return rc;
			call.launch(g_t, k_tp_tris<false>, keys, nt, j.join, 0u, (uint32_t*)nullptr, comp, table, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items);
		}
		// 4. half-edges by edge: the per-half-edge arrays, the edge counts, the double cover and the boundary components united
		uint32_t *cover = nullptr, *bparent = nullptr, *bmark = nullptr;
		if (!call.ws.alloc(&cover, 2 * (size_t)nt) || !call.ws.alloc(&bparent, nv) || !call.ws.alloc(&bmark, nv)) return call.nomem("hipMalloc failed for the double cover of " + std::to_string(nt) + " triangles");
		call.launch(groups(2 * (uint64_t)nt), k_cl_init, cover, 2u * nt);
		call.launch(g_v, k_cl_init, bparent, nv);
		HIP_TRY(hipMemsetAsync(bmark, 0, (size_t)nv * 4, s));
		{
			TpTable j;
			const TpEdgeKeys keys{tris};
			if (int rc = tp_join(call, keys, m.n_indices, opt->buckets_log2, dres, &j); rc != RNB_OK) return rc;
			call.launch(g_h, k_tp_edges, keys, m.n_indices, j.join, n_faces, n_same, mate, cover, bparent, bmark, comp, table, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items);
		}
		// 5. patches, boundary components, the table's derived columns
		call.launch(groups(2 * (uint64_t)nt), k_cl_flatten, cover, 2u * nt);
		call.launch(g_t, k_tp_patches, tris, nt, (const uint32_t*)cover, (uint32_t*)nullptr, comp, table, dres);
		call.launch(g_v, k_tp_boundary_roots, (const uint32_t*)bparent, (const uint32_t*)bmark, nv, dres);
		call.launch(groups(std::max(n_comp, 1u)), k_tp_table_finish, table, n_comp);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(parent, cover, bparent, bmark, dres);
	} else if (table_dev && !call.ws.alloc(&table, 1))
		return call.nomem("hipMalloc failed for the table");
	if (table_dev) *table_dev = (rnb_mesh_topology_component*)call.ws.keep(table);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_verts_used = hres.n_verts_used; stats->n_tris = nt; stats->n_degenerate = hres.n_degenerate;
		stats->n_edges = hres.n_edges; stats->n_boundary_edges = hres.n_boundary_edges; stats->n_manifold_edges = hres.n_manifold_edges;
		stats->n_nonmanifold_edges = hres.n_nonmanifold_edges; stats->n_inconsistent_edges = hres.n_inconsistent_edges; stats->max_faces_on_edge = hres.max_faces_on_edge;
		stats->n_duplicate_tris = hres.n_duplicate_tris; stats->n_folded_pairs = hres.n_folded_pairs;
		stats->n_components = n_comp; stats->n_patches = hres.n_patches; stats->n_unorientable_patches = hres.n_unorientable_patches;
		stats->n_boundary_components = hres.n_boundary_components;
		stats->closed = (!hres.n_boundary_edges && !hres.n_nonmanifold_edges) ? 1u : 0u;
		stats->oriented = (stats->closed && !hres.n_inconsistent_edges) ? 1u : 0u;
		stats->euler = (int64_t)hres.n_verts_used - (int64_t)hres.n_edges + ((int64_t)nt - (int64_t)hres.n_degenerate);
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_repair(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_repair_options* opt, rnb_mesh* out, uint32_t* vertex_map, rnb_mesh_repair_stats* stats) try {
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_repair: null argument");
	if (int rc = check_mesh_input("rnb_mesh_repair", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_TOPOLOGY_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_repair: options abi_version mismatch (expected RNB_MESH_TOPOLOGY_ABI_VERSION)");
	if (opt->weld > 1u || opt->drop_degenerate > 1u) return fail(RNB_ERR_INVALID, "rnb_mesh_repair: weld and drop_degenerate must be 0 or 1");
	if (opt->duplicates > RNB_MESH_DUPLICATES_CANCEL) return fail(RNB_ERR_INVALID, "rnb_mesh_repair: unknown duplicates mode");
	if (opt->orient > RNB_MESH_REPAIR_ORIENT_CONSISTENT) return fail(RNB_ERR_INVALID, "rnb_mesh_repair: unknown orient mode");
	if (int rc = tp_check_buckets("rnb_mesh_repair", opt->buckets_log2); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_repair", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_repair", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	TpResult hres;
	std::memset(&hres, 0, sizeof(hres));
	uint32_t nvo = 0, nto = 0;
	rnb_mesh o;
	if (nt) {
		const uint32_t g_v = groups(nv), g_t = groups(nt), g_h = groups(m.n_indices);
		uint32_t *used = nullptr, *widx = nullptr, *flags = nullptr, *rep = nullptr;
		TpResult* dres = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&widx, m.n_indices) || !call.ws.alloc(&flags, nt) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nt) + " triangles");
		HIP_TRY(hipMemsetAsync(dres, 0, sizeof(hres), s));
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		// 1. weld: the working indices point at the lowest vertex of every position
		if (opt->weld) {
			uint32_t hflags = 0;
			call.launch(g_v, k_tp_finite, (const uint32_t*)m.verts, (const uint32_t*)used, nv, dres);
			HIP_TRY(hipGetLastError());
			if (int rc = call.read_flags(&dres->flags, &hflags); rc != RNB_OK) return rc;
			if (hflags & TP_NOT_FINITE) return call.invalid("a coordinate of a used vertex is not finite (weld compares coordinates)");
			if (!call.ws.alloc(&rep, nv)) return call.nomem("hipMalloc failed for the weld map");
			TpTable j;
			const TpPosKeys keys{(const uint32_t*)m.verts, used};
			if (int rc = tp_join(call, keys, nv, opt->buckets_log2, dres, &j); rc != RNB_OK) return rc;
			call.launch(g_v, k_tp_weld, keys, nv, j.join, rep, dres);
			call.launch(g_h, k_tp_rewrite, (const uint32_t*)m.indices, (const uint32_t*)rep, m.n_indices, widx);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items);
		} else HIP_TRY(hipMemcpyAsync(widx, m.indices, (size_t)m.n_indices * 4, hipMemcpyDeviceToDevice, s));
		call.ws.release(used);
		// 2. degenerate triangles
		call.launch(g_t, k_tp_degenerate, (const uint32_t*)widx, nt, opt->drop_degenerate, flags, dres);
		HIP_TRY(hipGetLastError());
		const TpTris tris{widx, flags};
		// 3. duplicates
		if (opt->duplicates != RNB_MESH_DUPLICATES_KEEP) {
			uint32_t* stay = nullptr;
			if (!call.ws.alloc(&stay, nt)) return call.nomem("hipMalloc failed for the duplicate flags");
			TpTable j;
			const TpTriKeys keys{tris};
			if (int rc = tp_join(call, keys, nt, opt->buckets_log2, dres, &j); rc != RNB_OK) return rc;
			call.launch(g_t, k_tp_tris<true>, keys, nt, j.join, opt->duplicates, stay, (const uint32_t*)nullptr, (rnb_mesh_topology_component*)nullptr, dres);
			call.launch(g_t, k_tp_apply, (const uint32_t*)stay, nt, flags, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items, stay);
		}
		// 4. orient: the double cover over the manifold edges of what is left, the sheet that flips fewer
		if (opt->orient == RNB_MESH_REPAIR_ORIENT_CONSISTENT) {
			uint32_t *cover = nullptr, *sheet = nullptr;
			if (!call.ws.alloc(&cover, 2 * (size_t)nt) || !call.ws.alloc(&sheet, 2 * (size_t)nt)) return call.nomem("hipMalloc failed for the double cover of " + std::to_string(nt) + " triangles");
			call.launch(groups(2 * (uint64_t)nt), k_cl_init, cover, 2u * nt);
			HIP_TRY(hipMemsetAsync(sheet, 0, 2 * (size_t)nt * 4, s));
			TpTable j;
			const TpEdgeKeys keys{tris};
			if (int rc = tp_join(call, keys, m.n_indices, opt->buckets_log2, dres, &j); rc != RNB_OK) return rc;
			call.launch(g_h, k_tp_edges, keys, m.n_indices, j.join, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, cover, (uint32_t*)nullptr, (uint32_t*)nullptr,
			                   (const uint32_t*)nullptr, (rnb_mesh_topology_component*)nullptr, (TpResult*)nullptr);
			call.launch(groups(2 * (uint64_t)nt), k_cl_flatten, cover, 2u * nt);
			call.launch(g_t, k_tp_patches, tris, nt, (const uint32_t*)cover, sheet, (const uint32_t*)nullptr, (rnb_mesh_topology_component*)nullptr, dres);
			call.launch(g_t, k_tp_flip, tris, nt, (const uint32_t*)cover, (const uint32_t*)sheet, flags, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items, cover, sheet);
		}
		// 5. compaction: the vertices the remaining triangles use, the new numbering
		uint32_t *vkeep = nullptr, *vmap = nullptr, *twg = nullptr, *scan = nullptr;
		if (!call.ws.alloc(&vkeep, nv) || !call.ws.alloc(&vmap, nv) || !call.ws.alloc(&twg, g_t) || !call.ws.alloc(&scan, scan_scratch_elems(std::max<uint64_t>(nv, g_t))))
			return call.nomem("hipMalloc failed for the compaction of " + std::to_string(nv) + " vertices");
		HIP_TRY(hipMemsetAsync(vkeep, 0, (size_t)nv * 4, s));
		call.launch(g_t, k_tp_mark, (const uint32_t*)widx, (const uint32_t*)flags, nt, vkeep);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(vmap, vkeep, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
		rnb_mesh w = m;
		w.indices = widx;
		if (int rc = call.compact(w, TpKeep{vkeep, flags}, vmap, twg, scan, &o, &nvo, &nto); rc != RNB_OK) return rc;
		if (vertex_map) call.launch(g_v, k_tp_vertex_map, (const uint32_t*)rep, (const uint32_t*)vkeep, (const uint32_t*)vmap, nv, vertex_map);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(widx, flags, rep, vkeep, vmap, twg, scan, dres);
	} else {
		if (!alloc_mesh(call.ws, &o, 0, 0, m.colors != nullptr, m.normals != nullptr)) return call.nomem("hipMalloc failed for the output mesh");
		if (vertex_map && nv) { HIP_TRY(hipMemsetAsync(vertex_map, 0xFF, (size_t)nv * 4, s)); HIP_TRY(hipStreamSynchronize(s)); }
	}
	hand_over(call.ws, o, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_welded = hres.n_welded; stats->n_degenerate_dropped = hres.n_degenerate; stats->n_duplicates_dropped = hres.n_dropped; stats->n_flipped = hres.n_flipped;
		stats->n_patches = hres.n_patches; stats->n_unorientable_patches = hres.n_unorientable_patches;
		stats->n_verts_in = nv; stats->n_verts_out = nvo; stats->n_tris_in = nt; stats->n_tris_out = nto;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- holes: the boundary loops and their fill (include/rnb_mesh_holes.h) ----
uint32_t rnb_mesh_holes_abi_version(void) { return RNB_MESH_HOLES_ABI_VERSION; }

int rnb_mesh_boundary_loops_default_options(rnb_mesh_boundary_loops_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_HOLES_ABI_VERSION;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_fill_holes_default_options(rnb_mesh_fill_holes_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_HOLES_ABI_VERSION;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_boundary_loops_free(rnb_ctx* c, rnb_mesh_boundary_loop* table) try {
	if (!c) return fail(RNB_ERR_INVALID, "null argument");
	if (table) (void)hipFree(table);
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
// What the census leaves on the device for its caller (all held by the call's workspace): the boundary half-edges as a list of nb items, and per item its loop and
// its position; per half-edge the faces on its edge and its item; per vertex the outgoing boundary half-edge; per loop its record and its sums.
struct HlCensus {
	uint32_t nb = 0, n_loops = 0;
	uint32_t *n_faces = nullptr, *bidx = nullptr, *list = nullptr, *iloop = nullptr, *ipos = nullptr, *outh = nullptr, *comp = nullptr;
	rnb_mesh_boundary_loop* table = nullptr;
	long long* sums = nullptr;
	HlResult* dres = nullptr;
	HlResult hres;
};
// The census of a mesh with at least one triangle: steps 1 .. 6 of the header's definitions. Synchronised on return.
int hl_census(MeshCall& call, const rnb_mesh& m, uint32_t buckets_log2, HlCensus* C) {
	const hipStream_t s = call.s;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, nh = m.n_indices;
	const uint32_t g_v = groups(nv), g_t = groups(nt), g_h = groups(nh);
	const uint32_t* idx = (const uint32_t*)m.indices;
	std::memset(&C->hres, 0, sizeof(C->hres));
	uint32_t *used = nullptr, *cover = nullptr, *broot = nullptr, *bmark = nullptr, *scan = nullptr;
	TpResult* tres = nullptr;
	if (!call.ws.alloc(&C->comp, nv) || !call.ws.alloc(&used, nv) || !call.ws.alloc(&broot, nv) || !call.ws.alloc(&bmark, nv) || !call.ws.alloc(&cover, 2 * (size_t)nt) ||
	    !call.ws.alloc(&C->n_faces, nh) || !call.ws.alloc(&C->bidx, nh) || !call.ws.alloc(&scan, scan_scratch_elems(nh)) || !call.ws.alloc(&tres, 1) || !call.ws.alloc(&C->dres, 1))
		return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nt) + " triangles");
	HIP_TRY(hipMemsetAsync(tres, 0, sizeof(TpResult), s));
	HIP_TRY(hipMemsetAsync(C->dres, 0, sizeof(HlResult), s));
	// 1. every index is range-checked before any is used as an address; the cleaner's components
	if (int rc = call.check_indices(m, used, &tres->flags); rc != RNB_OK) return rc;
	call.ws.release(used);
	call.launch(g_v, k_cl_init, C->comp, nv);
	call.launch(g_t, k_cl_hook, idx, nt, C->comp);
	call.launch(g_v, k_cl_flatten, C->comp, nv);
	// 2. the topology stage's edge join: faces per half-edge; the boundary edges unite their ends (the double cover is its by-product)
	call.launch(groups(2 * (uint64_t)nt), k_cl_init, cover, 2u * nt);
	call.launch(g_v, k_cl_init, broot, nv);
	HIP_TRY(hipMemsetAsync(bmark, 0, (size_t)nv * 4, s));
	{
		TpTable j;
		const TpEdgeKeys keys{TpTris{idx, nullptr}};
		if (int rc = tp_join(call, keys, nh, buckets_log2, tres, &j); rc != RNB_OK) return rc;
		call.launch(g_h, k_tp_edges, keys, nh, j.join, C->n_faces, (uint32_t*)nullptr, (uint32_t*)nullptr, cover, broot, bmark, (const uint32_t*)nullptr, (rnb_mesh_topology_component*)nullptr,
		            (TpResult*)nullptr);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(j.offs, j.items, cover);
	}
	call.launch(g_v, k_cl_flatten, broot, nv);
	// 3. the boundary half-edges as a list
	call.launch(g_h, k_hl_flag, (const uint32_t*)C->n_faces, nh, C->bidx);
	HIP_TRY(hipGetLastError());
	if (int rc = scan_exclusive(C->bidx, nh, s, &C->nb, scan); rc != RNB_OK) return rc;
	const uint32_t nb = C->nb;
	if (!nb) { call.ws.release(broot, bmark, scan, tres); return RNB_OK; }
	const uint32_t g_b = groups(nb);
	uint32_t *outc = nullptr, *inc = nullptr, *lab = nullptr, *lrank = nullptr;
	if (!call.ws.alloc(&C->list, nb) || !call.ws.alloc(&C->iloop, nb) || !call.ws.alloc(&C->ipos, nb) || !call.ws.alloc(&lrank, nb) || !call.ws.alloc(&outc, nv) || !call.ws.alloc(&inc, nv) ||
	    !call.ws.alloc(&C->outh, nv) || !call.ws.alloc(&lab, nv))
		return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nb) + " boundary edges");
	HIP_TRY(hipMemsetAsync(outc, 0, (size_t)nv * 4, s));
	HIP_TRY(hipMemsetAsync(inc, 0, (size_t)nv * 4, s));
	HIP_TRY(hipMemsetAsync(C->outh, 0xFF, (size_t)nv * 4, s));
	HIP_TRY(hipMemsetAsync(lab, 0xFF, (size_t)nv * 4, s));
	HIP_TRY(hipMemsetAsync(lrank, 0, (size_t)nb * 4, s));
	call.launch(g_h, k_hl_list, (const uint32_t*)C->n_faces, (const uint32_t*)C->bidx, nh, C->list);
	// 4. per vertex: counts, the outgoing half-edge; per component: the label; the loops numbered in ascending label
	call.launch(g_b, k_hl_vertex, idx, (const uint32_t*)C->list, nb, (const uint32_t*)broot, outc, inc, C->outh, lab);
	call.launch(g_v, k_hl_label_flags, (const uint32_t*)broot, (const uint32_t*)bmark, (const uint32_t*)lab, (const uint32_t*)C->bidx, nv, lrank);
	HIP_TRY(hipGetLastError());
	if (int rc = scan_exclusive(lrank, nb, s, &C->n_loops, scan); rc != RNB_OK) return rc;
	const uint32_t nl = C->n_loops, g_l = groups(nl);
	if (!call.ws.alloc(&C->table, nl) || !call.ws.alloc(&C->sums, (size_t)nl * HL_NSUM)) return call.nomem("hipMalloc failed for the table of " + std::to_string(nl) + " loops");
	HIP_TRY(hipMemsetAsync(C->table, 0, (size_t)nl * sizeof(rnb_mesh_boundary_loop), s));
	HIP_TRY(hipMemsetAsync(C->sums, 0, (size_t)nl * HL_NSUM * 8, s));
	call.launch(g_b, k_hl_loops, idx, (const uint32_t*)C->list, nb, (const uint32_t*)broot, (const uint32_t*)lab, (const uint32_t*)C->bidx, (const uint32_t*)lrank, C->iloop, C->table);
	call.launch(g_v, k_hl_vertices, (const uint32_t*)broot, (const uint32_t*)bmark, (const uint32_t*)outc, (const uint32_t*)inc, (const uint32_t*)lab, (const uint32_t*)C->bidx,
	            (const uint32_t*)lrank, (const uint32_t*)C->comp, nv, C->table);
	call.launch(g_l, k_hl_classify, C->table, nl, C->dres);
	// 5. the sums (they need the labels only), then the longest simple loop read back: it fixes the number of ranking rounds
	call.launch(g_b, k_hl_sums, idx, (const float*)m.verts, (const float*)m.colors, (const uint32_t*)C->list, nb, (const uint32_t*)C->iloop, (const rnb_mesh_boundary_loop*)C->table, C->sums, C->dres);
	call.launch(g_l, k_hl_finish, idx, (const float*)m.verts, C->table, (const long long*)C->sums, nl);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(&C->hres, C->dres, sizeof(HlResult), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	call.ws.release(broot, bmark, outc, inc, lab, lrank, scan, tres);
	if (C->hres.flags & HL_NOT_FINITE) return call.invalid("a coordinate of a boundary vertex is not finite");
	if (C->hres.flags & HL_BAD_TERM) return call.invalid("a term of a boundary component's sums is not below 2^10 in magnitude (a boundary vertex too far from its component's first, or a colour)");
	// 6. list ranking: ceil(log2(longest simple loop)) rounds of pointer jumping, each from one buffer into the other
	uint2 *cur = nullptr, *nxt = nullptr;
	if (!call.ws.alloc(&cur, nb) || !call.ws.alloc(&nxt, nb)) return call.nomem("hipMalloc failed for the ranking of " + std::to_string(nb) + " boundary edges");
	call.launch(g_b, k_hl_rank_init, idx, (const uint32_t*)C->list, nb, (const uint32_t*)C->iloop, (const rnb_mesh_boundary_loop*)C->table, (const uint32_t*)C->outh, (const uint32_t*)C->bidx, cur);
	uint32_t rounds = 0;
	while ((1ull << rounds) < C->hres.max_simple_edges) ++rounds;
	for (uint32_t r = 0; r < rounds; ++r) {
		call.launch(g_b, k_hl_rank_round, (const uint2*)cur, nxt, nb);
		std::swap(cur, nxt);
	}
	call.launch(g_b, k_hl_pos, (const uint2*)cur, (const uint32_t*)C->iloop, (const rnb_mesh_boundary_loop*)C->table, nb, C->ipos);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(s));
	call.ws.release(cur, nxt);
	return RNB_OK;
}
} // namespace
} // extern "C++"

int rnb_mesh_boundary_loops(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_boundary_loops_options* opt, uint32_t* loop_dev, uint32_t* next_dev, uint32_t* pos_dev,
                            rnb_mesh_boundary_loop** table_dev, rnb_mesh_boundary_loops_stats* stats) try {
	if (table_dev) *table_dev = nullptr;
	if (!c || !in || !opt) return fail(RNB_ERR_INVALID, "rnb_mesh_boundary_loops: null argument");
	if (int rc = check_mesh_input("rnb_mesh_boundary_loops", in); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_HOLES_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_boundary_loops: options abi_version mismatch (expected RNB_MESH_HOLES_ABI_VERSION)");
	if (int rc = tp_check_buckets("rnb_mesh_boundary_loops", opt->buckets_log2); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_boundary_loops", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_boundary_loops", c, stream);
	const hipStream_t s = call.s;

	HlCensus C;
	std::memset(&C.hres, 0, sizeof(C.hres));
	const uint32_t nh = m.n_indices;
	if (nh) {
		if (int rc = hl_census(call, m, opt->buckets_log2, &C); rc != RNB_OK) return rc;
		if (loop_dev || next_dev || pos_dev) {
			if (C.nb)
				call.launch(groups(nh), k_hl_write, (const uint32_t*)m.indices, (const uint32_t*)C.n_faces, (const uint32_t*)C.bidx, (const uint32_t*)C.iloop, (const uint32_t*)C.ipos,
				            (const rnb_mesh_boundary_loop*)C.table, (const uint32_t*)C.outh, nh, loop_dev, next_dev, pos_dev);
			else
				for (uint32_t* p : {loop_dev, next_dev, pos_dev})
					if (p) HIP_TRY(hipMemsetAsync(p, 0xFF, (size_t)nh * 4, s));
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
		}
	}
	if (table_dev) {
		if (!C.table && !call.ws.alloc(&C.table, 1)) return call.nomem("hipMalloc failed for the table");
		*table_dev = (rnb_mesh_boundary_loop*)call.ws.keep(C.table);
	}
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_boundary_edges = C.nb; stats->n_loops = C.n_loops; stats->n_simple = C.hres.n_simple; stats->n_irregular_vertices = C.hres.n_irregular_vertices;
		stats->max_loop_edges = C.hres.max_loop_edges; stats->n_too_long = C.hres.n_too_long;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_fill_holes(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_fill_holes_options* opt, rnb_mesh* out, uint32_t* loop_of_tri, rnb_mesh_fill_holes_stats* stats) try {
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_fill_holes: null argument");
	if (int rc = check_mesh_input("rnb_mesh_fill_holes", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_HOLES_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_fill_holes: options abi_version mismatch (expected RNB_MESH_HOLES_ABI_VERSION)");
	if (opt->skip_largest > 1u) return fail(RNB_ERR_INVALID, "rnb_mesh_fill_holes: skip_largest must be 0 or 1");
	if (int rc = tp_check_buckets("rnb_mesh_fill_holes", opt->buckets_log2); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_fill_holes", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_fill_holes", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	HlCensus C;
	std::memset(&C.hres, 0, sizeof(C.hres));
	if (nt)
		if (int rc = hl_census(call, m, opt->buckets_log2, &C); rc != RNB_OK) return rc;
	const uint32_t nb = C.nb, nl = C.n_loops;
	uint32_t nva = 0, nta = 0;
	uint32_t *fill = nullptr, *voff = nullptr, *toff = nullptr;
	if (nl) {
		// who is filled; what each loop appends, and from where
		unsigned long long* big = nullptr;
		uint32_t* scan = nullptr;
		if (!call.ws.alloc(&fill, nl) || !call.ws.alloc(&voff, nl) || !call.ws.alloc(&toff, nl) || !call.ws.alloc(&scan, scan_scratch_elems(nl)) || (opt->skip_largest && !call.ws.alloc(&big, nv)))
			return call.nomem("hipMalloc failed for the selection among " + std::to_string(nl) + " loops");
		if (big) {
			HIP_TRY(hipMemsetAsync(big, 0, (size_t)nv * 8, s));
			call.launch(groups(nl), k_hl_largest, (const rnb_mesh_boundary_loop*)C.table, nl, big);
		}
		const uint32_t limit = opt->max_edges ? std::min<uint32_t>(opt->max_edges, RNB_MESH_HOLES_MAX_EDGES) : RNB_MESH_HOLES_MAX_EDGES;
		call.launch(groups(nl), k_hl_select, (const rnb_mesh_boundary_loop*)C.table, nl, (const unsigned long long*)big, limit, fill, voff, toff, C.dres);
		HIP_TRY(hipGetLastError());
		if (int rc = scan_exclusive(voff, nl, s, &nva, scan); rc != RNB_OK) return rc;
		if (int rc = scan_exclusive(toff, nl, s, &nta, scan); rc != RNB_OK) return rc;
		HIP_TRY(hipMemcpyAsync(&C.hres, C.dres, sizeof(HlResult), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(big, scan);
	}
	const uint64_t nvo = (uint64_t)nv + nva, nto = (uint64_t)nt + nta;
	if (nvo > 0xFFFFFFFEull || 3 * nto > 0xFFFFFFFFull) return call.invalid("the filled mesh would hold " + std::to_string(nto) + " triangles: more than an index count of 32 bits takes");
	rnb_mesh o;
	if (int rc = call.alloc_like(m, &o, (uint32_t)nvo, (uint32_t)nto); rc != RNB_OK) return rc;
	if (nv) {
		HIP_TRY(hipMemcpyAsync(o.verts, m.verts, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
		if (m.colors) HIP_TRY(hipMemcpyAsync(o.colors, m.colors, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
		if (m.normals) HIP_TRY(hipMemcpyAsync(o.normals, m.normals, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
	}
	if (nt) HIP_TRY(hipMemcpyAsync(o.indices, m.indices, (size_t)nt * 12, hipMemcpyDeviceToDevice, s));
	if (loop_of_tri && nto) HIP_TRY(hipMemsetAsync(loop_of_tri, 0xFF, (size_t)nto * 4, s));
	if (nta) {
		call.launch(groups(nb), k_hl_emit_tris, (const uint32_t*)m.indices, (const uint32_t*)C.list, nb, (const uint32_t*)C.iloop, (const uint32_t*)C.ipos, (const rnb_mesh_boundary_loop*)C.table,
		            (const uint32_t*)fill, (const uint32_t*)voff, (const uint32_t*)toff, (const uint32_t*)C.outh, nv, nt, o.indices, loop_of_tri);
		if (nva)
			call.launch(groups(nl), k_hl_emit_verts, (const rnb_mesh_boundary_loop*)C.table, (const long long*)C.sums, nl, (const uint32_t*)fill, (const uint32_t*)voff, nv, o.verts, o.colors, o.normals);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipStreamSynchronize(s));
	hand_over(call.ws, o, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_loops = nl; stats->n_filled = C.hres.n_filled; stats->n_skipped_not_simple = C.hres.n_not_simple; stats->n_skipped_over_max = C.hres.n_over_max;
		stats->n_skipped_largest = C.hres.n_largest; stats->n_verts_added = nva; stats->n_tris_added = nta; stats->n_verts_out = (uint32_t)nvo; stats->n_tris_out = (uint32_t)nto;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- self-intersections (include/rnb_mesh_intersect.h) ----
uint32_t rnb_mesh_intersect_abi_version(void) { return RNB_MESH_INTERSECT_ABI_VERSION; }

int rnb_mesh_intersect_default_options(rnb_mesh_intersect_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_INTERSECT_ABI_VERSION;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_intersections_select_default_options(rnb_mesh_intersect_select_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_INTERSECT_ABI_VERSION;
	opt->classes = RNB_MESH_INTERSECT_PROPER;
	opt->drop_unused_vertices = 1u;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_intersections(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_intersect_options* opt, uint32_t* n_proper_dev, uint32_t* n_contact_dev,
                           rnb_mesh_intersect_pair* pairs_dev, uint64_t pairs_capacity, rnb_mesh_intersect_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !in || !opt) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections: null argument");
	if (opt->abi_version != RNB_MESH_INTERSECT_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections: options abi_version mismatch (expected RNB_MESH_INTERSECT_ABI_VERSION)");
	if (opt->cells > RNB_MESH_INTERSECT_MAX_CELLS) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections: cells must be 0 .. 256");
	if (int rc = check_reserved("rnb_mesh_intersections", opt->reserved); rc != RNB_OK) return rc;
	if (pairs_capacity && !pairs_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections: pairs_capacity without pairs_dev");
	if (n_proper_dev && n_proper_dev == n_contact_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections: n_proper_dev and n_contact_dev must be different buffers");
	if (int rc = check_mesh_input("rnb_mesh_intersections", in); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	MeshCall call("rnb_mesh_intersections", c, stream);
	const hipStream_t s = call.s;

	MdResult hres;
	std::memset(&hres, 0, sizeof(hres));
	for (int k = 0; k < 3; ++k) hres.bmin[k] = 0xFFFFFFFFu;
	MiResult hmi;
	std::memset(&hmi, 0, sizeof(hmi));
	MdGrid g;
	std::memset(&g, 0, sizeof(g));
	float ms_grid = 0.0f;
	if (nt) {
		const uint32_t g_t = groups(nt);
		const MdMesh M{m.verts, m.indices, nv, nt};
		uint32_t *used = nullptr, *large = nullptr, *own_proper = nullptr, *own_contact = nullptr;
		MdResult* dres = nullptr;
		MiResult* dmi = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&large, RNB_MESH_DISTANCE_MAX_LARGE) || !call.ws.alloc(&dres, 1) || !call.ws.alloc(&dmi, 1) || (!n_proper_dev && !call.ws.alloc(&own_proper, nt)) ||
		    (!n_contact_dev && !call.ws.alloc(&own_contact, nt)))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices and " + std::to_string(nt) + " triangles");
		uint32_t *np = n_proper_dev ? n_proper_dev : own_proper, *nc = n_contact_dev ? n_contact_dev : own_contact;
		HIP_TRY(hipMemcpyAsync(dres, &hres, sizeof(hres), hipMemcpyHostToDevice, s));
		HIP_TRY(hipMemsetAsync(dmi, 0, sizeof(MiResult), s));
		HIP_TRY(hipMemsetAsync(np, 0, (size_t)nt * 4, s));
		HIP_TRY(hipMemsetAsync(nc, 0, (size_t)nt * 4, s));
		// 1. every index is range-checked before any is used as an address; the used vertices, their box, the triangles that take part
		if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
		hipLaunchKernelGGL(k_md_verts<true>, dim3(groups(nv)), dim3(MESH_WG), 0, s, (const float*)m.verts, nv, (const uint32_t*)used, dres);
		hipLaunchKernelGGL(k_md_degenerate, dim3(g_t), dim3(MESH_WG), 0, s, M, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		if (hres.flags & MD_BAD_VALUE) return call.invalid("a coordinate of a used vertex is not finite");
		call.ws.release(used);
		const uint32_t live = nt - hres.n_deg_to;
		if (live) {
			// 2. the grid over the mesh's own box, the cell lists (the distance stage's)
			const auto t_grid = std::chrono::steady_clock::now();
			uint32_t *start = nullptr, *cursor = nullptr, *scan = nullptr, *entries = nullptr, *own = nullptr, *offs = nullptr, *pscan = nullptr;
			rnb_mesh_intersect_pair* tmp = nullptr;
			if (int rc = md_build_lists(call, M, opt->cells, live, "", large, dres, &hres, &g, &start, &cursor, &scan, &entries); rc != RNB_OK) return rc;
			ms_grid = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_grid).count();
			// 3. the pairs: cell by cell, then against the large list
			const bool want_pairs = pairs_dev && pairs_capacity;
			if (want_pairs) {
				if (!call.ws.alloc(&own, (size_t)nt + 1) || !call.ws.alloc(&offs, (size_t)nt + 1) || !call.ws.alloc(&pscan, scan_scratch_elems((uint64_t)nt + 1)))
					return call.nomem("hipMalloc failed for the pair counts of " + std::to_string(nt) + " triangles");
				HIP_TRY(hipMemsetAsync(own, 0, ((size_t)nt + 1) * 4, s));
			}
			const unsigned long long n_cells = (unsigned long long)g.dims[0] * g.dims[1] * g.dims[2];
			const uint32_t g_c = (uint32_t)std::min<unsigned long long>((n_cells + MESH_WG / 64 - 1) / (MESH_WG / 64), 1u << 16);
			const dim3 g_l(g_t, std::max(hres.n_large, 1u));
			MiOut out{np, nc, own, nullptr, nullptr};
			hipLaunchKernelGGL(k_mi_cells<false>, dim3(g_c), dim3(MESH_WG), 0, s, g, M, (const uint32_t*)start, (const uint32_t*)cursor, (const uint32_t*)entries, n_cells, out, dmi);
			if (hres.n_large) hipLaunchKernelGGL(k_mi_large<false>, g_l, dim3(MESH_WG), 0, s, g, M, (const uint32_t*)large, out, dmi);
			hipLaunchKernelGGL(k_mi_tally, dim3(g_t), dim3(MESH_WG), 0, s, (const uint32_t*)np, (const uint32_t*)nc, nt, dmi);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(&hmi, dmi, sizeof(hmi), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			// 4. the pair list: the same pass again, every reported pair into its lower triangle's segment, then ranked inside it
			const unsigned long long n_reported = hmi.n_proper + hmi.n_contact;
			if (want_pairs && n_reported) {
				if (n_reported > 0xFFFFFFFFull) return call.invalid(std::to_string(n_reported) + " pairs: more than 2^32 - 1, too many for a list");
				uint32_t total = 0;
				HIP_TRY(hipMemcpyAsync(offs, own, ((size_t)nt + 1) * 4, hipMemcpyDeviceToDevice, s));
				if (int rc = scan_exclusive(offs, (uint64_t)nt + 1, s, &total, pscan); rc != RNB_OK) return rc;
				if (total != (uint32_t)n_reported) return call.device("the pair counts do not add up");
				if (!call.ws.alloc(&tmp, total)) return call.nomem("hipMalloc failed for " + std::to_string(total) + " pairs");
				HIP_TRY(hipMemsetAsync(own, 0, ((size_t)nt + 1) * 4, s));
				out = MiOut{np, nc, own, offs, tmp};
				hipLaunchKernelGGL(k_mi_cells<true>, dim3(g_c), dim3(MESH_WG), 0, s, g, M, (const uint32_t*)start, (const uint32_t*)cursor, (const uint32_t*)entries, n_cells, out, dmi);
				if (hres.n_large) hipLaunchKernelGGL(k_mi_large<true>, g_l, dim3(MESH_WG), 0, s, g, M, (const uint32_t*)large, out, dmi);
				hipLaunchKernelGGL(k_mi_rank, dim3(groups(total)), dim3(MESH_WG), 0, s, (const rnb_mesh_intersect_pair*)tmp, (const uint32_t*)offs, total, pairs_dev, (unsigned long long)pairs_capacity);
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipStreamSynchronize(s));
			}
			call.ws.release(start, cursor, scan, entries, own, offs, pscan, tmp);
		}
		call.ws.release(large, dres, dmi, own_proper, own_contact);
	}
	if (stats) {
		stats->n_tris = nt; stats->n_degenerate = hres.n_deg_to; stats->n_tris_proper = hmi.n_tris_proper; stats->n_tris_contact = hmi.n_tris_contact;
		stats->n_same_set = hmi.n_same; stats->n_candidates = hmi.n_cand; stats->n_pairs_proper = hmi.n_proper; stats->n_pairs_contact = hmi.n_contact;
		stats->n_coplanar_pairs = hmi.n_coplanar; stats->n_pairs_written_would_be = pairs_dev ? hmi.n_proper + hmi.n_contact : 0ull;
		for (int k = 0; k < 3; ++k) stats->dims[k] = g.dims[k];
		stats->n_large = hres.n_large; stats->cell = g.cell; stats->n_cell_entries = hres.n_entries; stats->n_visited = hmi.n_visited;
		stats->ms_grid = ms_grid;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_intersections_select(rnb_ctx* c, void* stream, const rnb_mesh* in, const uint32_t* n_proper_dev, const uint32_t* n_contact_dev, const rnb_mesh_intersect_select_options* opt,
                                  rnb_mesh* out, rnb_mesh_intersect_select_stats* stats) try {
	if (stats) std::memset(stats, 0, sizeof(*stats));
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: null argument");
	if (int rc = check_mesh_input("rnb_mesh_intersections_select", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_INTERSECT_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: options abi_version mismatch (expected RNB_MESH_INTERSECT_ABI_VERSION)");
	if (!opt->classes || (opt->classes & ~(RNB_MESH_INTERSECT_PROPER | RNB_MESH_INTERSECT_CONTACT))) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: classes must be PROPER, CONTACT or both");
	if (opt->rings > RNB_MESH_INTERSECT_MAX_RINGS) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: rings must be 0 .. 8");
	if (opt->drop_unused_vertices > 1u) return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: drop_unused_vertices must be 0 or 1");
	if (int rc = check_reserved("rnb_mesh_intersections_select", opt->reserved); rc != RNB_OK) return rc;
	if (m.n_indices && (((opt->classes & RNB_MESH_INTERSECT_PROPER) && !n_proper_dev) || ((opt->classes & RNB_MESH_INTERSECT_CONTACT) && !n_contact_dev)))
		return fail(RNB_ERR_INVALID, "rnb_mesh_intersections_select: the counts of a selected class are null");
	MeshCall call("rnb_mesh_intersections_select", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	MiResult hmi;
	std::memset(&hmi, 0, sizeof(hmi));
	uint32_t nvo = 0, nto = 0;
	rnb_mesh o;
	if (nt) {
		const uint32_t g_t = groups(nt);
		const uint32_t* idx = m.indices;
		uint32_t *used = nullptr, *flag = nullptr, *vmark = nullptr, *vmap = nullptr, *scan = nullptr, *twg = nullptr, *dflags = nullptr;
		MiResult* dmi = nullptr;
		if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&flag, nt) || !call.ws.alloc(&vmark, nv) || !call.ws.alloc(&vmap, nv) || !call.ws.alloc(&twg, g_t) ||
		    !call.ws.alloc(&scan, scan_scratch_elems(std::max<uint64_t>(nv, g_t))) || !call.ws.alloc(&dmi, 1) || !call.ws.alloc(&dflags, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices and " + std::to_string(nt) + " triangles");
		HIP_TRY(hipMemsetAsync(vmark, 0, (size_t)nv * 4, s));
		HIP_TRY(hipMemsetAsync(dmi, 0, sizeof(MiResult), s));
		HIP_TRY(hipMemsetAsync(dflags, 0, 4, s));
		// 1. every index is range-checked before any is used as an address
		if (int rc = call.check_indices(m, used, dflags); rc != RNB_OK) return rc;
		// 2. the selection and its rings (the marks of the earlier rings stay: their triangles are still selected)
		call.launch(g_t, k_mi_sel_flags, n_proper_dev, n_contact_dev, opt->classes, nt, flag, dmi);
		for (uint32_t r = 0; r < opt->rings; ++r) {
			call.launch(g_t, k_mi_sel_mark, idx, nt, (const uint32_t*)flag, vmark);
			call.launch(g_t, k_mi_sel_grow, idx, nt, flag, (const uint32_t*)vmark);
		}
		HIP_TRY(hipGetLastError());
		// 3. compaction: the kept vertices numbered (used's memory holds their flags), the kept triangles per workgroup
		uint32_t* vkeep = used;
		HIP_TRY(hipMemsetAsync(vkeep, 0, (size_t)nv * 4, s));
		call.launch(groups(opt->drop_unused_vertices ? nt : nv), k_mi_sel_vkeep, idx, nt, nv, (const uint32_t*)flag, opt->drop_unused_vertices ? 0u : 1u, vkeep);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(vmap, vkeep, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
		if (int rc = call.compact(m, MiKeep{flag, vkeep}, vmap, twg, scan, &o, &nvo, &nto); rc != RNB_OK) return rc;
		HIP_TRY(hipMemcpyAsync(&hmi, dmi, sizeof(hmi), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(used, flag, vmark, vmap, scan, twg, dmi, dflags);
	} else if (int rc = call.alloc_like(m, &o, 0, 0); rc != RNB_OK)
		return rc;
	hand_over(call.ws, o, out);
	if (stats) {
		stats->n_verts_in = nv; stats->n_verts_out = nvo; stats->n_tris_in = nt; stats->n_tris_out = nto;
		stats->n_selected = hmi.n_selected; stats->n_tris_removed = nt - nto; stats->n_verts_removed = nv - nvo;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- smoothing: Taubin passes over the one-ring, ring normals (include/rnb_mesh_smooth.h) ----
uint32_t rnb_mesh_smooth_abi_version(void) { return RNB_MESH_SMOOTH_ABI_VERSION; }

int rnb_mesh_smooth_default_options(rnb_mesh_smooth_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_SMOOTH_ABI_VERSION;
	opt->passes = 2; // one Taubin pair: the one row of profiles/mesh_smooth.md that lowers the mean normal angle on every mesh measured there
	opt->lambda = 0.5;
	opt->mu = -0.53;
	opt->boundary = RNB_MESH_SMOOTH_BOUNDARY_PIN;
	opt->normals = RNB_MESH_SMOOTH_NORMALS_KEEP;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_vertex_normals_default_options(rnb_mesh_vertex_normals_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_SMOOTH_ABI_VERSION;
	return RNB_OK;
} RNB_GUARD

extern "C++" {
namespace {
// The normals of a mesh with at least one vertex into `normals` (both entry points of the header; steps in the order of its definitions). Synchronised on return.
int vn_run(MeshCall& call, const rnb_mesh& m, uint32_t flip, float* normals, VnResult* hres) {
	const hipStream_t s = call.s;
	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	std::memset(hres, 0, sizeof(*hres));
	if (!nt) { // no corner anywhere: every normal is 0
		HIP_TRY(hipMemsetAsync(normals, 0, (size_t)nv * 12, s));
		HIP_TRY(hipStreamSynchronize(s));
		hres->n_zero = nv;
		return RNB_OK;
	}
	uint32_t* used = nullptr;
	long long* sums = nullptr;
	VnResult* dres = nullptr;
	if (!call.ws.alloc(&used, nv) || !call.ws.alloc(&sums, 4 * (size_t)nv) || !call.ws.alloc(&dres, 1)) return call.nomem("hipMalloc failed for the sums of " + std::to_string(nv) + " vertices");
	HIP_TRY(hipMemsetAsync(dres, 0, sizeof(VnResult), s));
	HIP_TRY(hipMemsetAsync(sums, 0, 4 * (size_t)nv * 8, s));
	if (int rc = call.check_indices(m, used, &dres->flags); rc != RNB_OK) return rc;
	call.launch(groups(nt), k_vn_accumulate, (const uint32_t*)m.indices, (const float*)m.verts, nt, sums, dres);
	call.launch(groups(nv), k_vn_finish, (const long long*)sums, nv, flip, normals, dres);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(hres, dres, sizeof(VnResult), hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	call.ws.release(used, sums, dres);
	if (hres->flags & SM_BAD_TERM) return call.invalid("a component of a triangle's cross product is not finite or not below 2^3 in magnitude");
	if (hres->flags & SM_BAD_RING) return call.invalid("a vertex has more than RNB_MESH_SMOOTH_MAX_RING = 2^20 corners");
	return RNB_OK;
}
} // namespace
} // extern "C++"

int rnb_mesh_vertex_normals(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_vertex_normals_options* opt, float* normals_dev, rnb_mesh_vertex_normals_stats* stats) try {
	if (!c || !in || !opt) return fail(RNB_ERR_INVALID, "rnb_mesh_vertex_normals: null argument");
	if (int rc = check_mesh_input("rnb_mesh_vertex_normals", in); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (m.n_verts && !normals_dev) return fail(RNB_ERR_INVALID, "rnb_mesh_vertex_normals: normals_dev is null");
	if (opt->abi_version != RNB_MESH_SMOOTH_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_vertex_normals: options abi_version mismatch (expected RNB_MESH_SMOOTH_ABI_VERSION)");
	if (opt->flip > 1u) return fail(RNB_ERR_INVALID, "rnb_mesh_vertex_normals: flip must be 0 or 1");
	if (int rc = check_reserved("rnb_mesh_vertex_normals", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_vertex_normals", c, stream);
	VnResult hres;
	std::memset(&hres, 0, sizeof(hres));
	if (m.n_verts)
		if (int rc = vn_run(call, m, opt->flip, normals_dev, &hres); rc != RNB_OK) return rc;
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_zero = hres.n_zero; stats->max_corners = hres.max_corners;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_smooth(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_smooth_options* opt, const uint32_t* select_dev, rnb_mesh* out, uint32_t* valence_dev, uint32_t* kind_dev,
                    float* displacement_dev, rnb_mesh_smooth_stats* stats) try {
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: null argument");
	if (int rc = check_mesh_input("rnb_mesh_smooth", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_SMOOTH_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: options abi_version mismatch (expected RNB_MESH_SMOOTH_ABI_VERSION)");
	if (opt->passes > RNB_MESH_SMOOTH_MAX_PASSES) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: passes must be 0 .. 10000");
	if (!(opt->lambda > 0.0 && opt->lambda <= 1.0)) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: lambda must be finite, above 0 and at most 1");
	if (!(opt->mu >= -1.5 && opt->mu <= 0.0)) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: mu must be finite, at least -1.5 and at most 0");
	if (opt->boundary > RNB_MESH_SMOOTH_BOUNDARY_FREE) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: boundary must be PIN, SLIDE or FREE");
	if (opt->select_rings > RNB_MESH_SMOOTH_MAX_SELECT_RINGS) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: select_rings must be 0 .. 1024");
	if (opt->normals > RNB_MESH_SMOOTH_NORMALS_RECOMPUTE) return fail(RNB_ERR_INVALID, "rnb_mesh_smooth: normals must be KEEP or RECOMPUTE");
	if (int rc = tp_check_buckets("rnb_mesh_smooth", opt->buckets_log2); rc != RNB_OK) return rc;
	if (int rc = check_reserved("rnb_mesh_smooth", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_smooth", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u, nh = m.n_indices;
	const bool recompute = opt->normals == RNB_MESH_SMOOTH_NORMALS_RECOMPUTE;
	SmResult hres;
	std::memset(&hres, 0, sizeof(hres));
	float ms_passes = 0.0f;
	rnb_mesh o;
	if (!alloc_mesh(call.ws, &o, nv, nt, m.colors != nullptr, m.normals != nullptr || recompute)) return call.nomem("hipMalloc failed for the output mesh");
	if (nv) {
		const uint32_t g_v = groups(nv), g_h = groups(nh);
		const TpEdgeKeys keys{TpTris{(const uint32_t*)m.indices, nullptr}};
		uint32_t *vinfo = nullptr, *sel = nullptr, *mode = nullptr, *off = nullptr, *wide = nullptr, *eface = nullptr, *scan = nullptr;
		SmResult* dres = nullptr;
		if (!call.ws.alloc(&vinfo, 4 * (size_t)nv) || !call.ws.alloc(&sel, nv) || !call.ws.alloc(&mode, nv) || !call.ws.alloc(&off, (size_t)nv + 1) || !call.ws.alloc(&wide, nv) ||
		    !call.ws.alloc(&eface, nh) || !call.ws.alloc(&scan, scan_scratch_elems((uint64_t)nv + 1)) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices and " + std::to_string(nt) + " triangles");
		HIP_TRY(hipMemsetAsync(dres, 0, sizeof(SmResult), s));
		HIP_TRY(hipMemsetAsync(vinfo, 0, 4 * (size_t)nv * 4, s));
		HIP_TRY(hipMemsetAsync(off + nv, 0, 4, s));
		if (nt) {
			// 1. every index is range-checked before any is used as an address (sel's memory takes the marks of the check)
			if (int rc = call.check_indices(m, sel, &dres->flags); rc != RNB_OK) return rc;
			// 2. the topology stage's edge join: the faces on every edge, at its lowest half-edge; valence, boundary and non-manifold edges per vertex
			TpTable j;
			TpResult* tres = nullptr;
			if (!call.ws.alloc(&tres, 1)) return call.nomem("hipMalloc failed for the edge join");
			HIP_TRY(hipMemsetAsync(tres, 0, sizeof(TpResult), s));
			if (int rc = tp_join(call, keys, nh, opt->buckets_log2, tres, &j); rc != RNB_OK) return rc;
			call.launch(g_h, k_sm_edges, keys, nh, j.join, eface, vinfo, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(j.offs, j.items, tres);
		}
		// 3. the selection: D_0, then one launch per ring
		call.launch(g_v, k_sm_select_init, select_dev, nv, sel);
		if (select_dev && nt)
			for (uint32_t r = 0; r < opt->select_rings; ++r) call.launch(g_h, k_sm_grow, keys, (const uint32_t*)eface, nh, r, sel);
		// 4. kinds, who moves, the lengths of the neighbour lists and their offsets
		const uint32_t lists = opt->passes ? 1u : 0u;
		call.launch(g_v, k_sm_kind, (const uint32_t*)vinfo, (const uint32_t*)sel, nv, opt->boundary, lists, mode, off, wide, valence_dev, kind_dev, dres);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		uint32_t n_entries = 0;
		if (int rc = scan_exclusive(off, (uint64_t)nv + 1, s, &n_entries, scan); rc != RNB_OK) return rc;
		call.ws.release(vinfo, sel, scan);
		if (hres.n_edges >= (1u << 31)) return call.invalid("the mesh has 2^31 edges or more");
		if (hres.flags & SM_BAD_RING) return call.invalid("a moving vertex has more than RNB_MESH_SMOOTH_MAX_RING = 2^20 neighbours");
		if (n_entries) {
			// 5. the neighbour lists; P_0 in both buffers; the passes, each a gather from one buffer into the other
			uint32_t *cursor = nullptr, *adj = nullptr;
			double *cur = nullptr, *nxt = nullptr;
			if (!call.ws.alloc(&cursor, nv) || !call.ws.alloc(&adj, n_entries) || !call.ws.alloc(&cur, 3 * (size_t)nv) || !call.ws.alloc(&nxt, 3 * (size_t)nv))
				return call.nomem("hipMalloc failed for the neighbour lists of " + std::to_string(n_entries) + " entries and the positions of " + std::to_string(nv) + " vertices");
			HIP_TRY(hipMemcpyAsync(cursor, off, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
			call.launch(g_h, k_sm_fill, keys, (const uint32_t*)eface, nh, (const uint32_t*)mode, cursor, adj);
			call.launch(groups(3 * (uint64_t)nv), k_sm_widen, (const float*)m.verts, 3 * (uint64_t)nv, cur, nxt);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			const auto t_passes = std::chrono::steady_clock::now();
			for (uint32_t k = 1; k <= opt->passes; ++k) {
				const double f = ((k & 1u) || opt->mu == 0.0) ? opt->lambda : opt->mu;
				call.launch(g_v, k_sm_pass, (const uint32_t*)off, (const uint32_t*)adj, (const double*)cur, nxt, nv, f, dres);
				if (hres.n_wide) call.launch(hres.n_wide, k_sm_pass_wide, (const uint32_t*)wide, (const uint32_t*)off, (const uint32_t*)adj, (const double*)cur, nxt, f, dres);
				std::swap(cur, nxt);
			}
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipStreamSynchronize(s));
			ms_passes = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_passes).count();
			// 6. the output vertices and the displacement
			call.launch(g_v, k_sm_finish, (const float*)m.verts, (const double*)cur, (const uint32_t*)mode, nv, o.verts, displacement_dev, dres);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
			HIP_TRY(hipStreamSynchronize(s));
			call.ws.release(cursor, adj, cur, nxt);
			if (hres.flags & SM_BAD_TERM) return call.invalid("a difference between a moving vertex and a neighbour is not finite or not below 2^10 in magnitude");
		} else { // nothing moves, or no pass is asked for: a copy
			HIP_TRY(hipMemcpyAsync(o.verts, m.verts, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
			if (displacement_dev) HIP_TRY(hipMemsetAsync(displacement_dev, 0, (size_t)nv * 4, s));
		}
		call.ws.release(mode, off, wide, eface, dres);
		if (m.colors) HIP_TRY(hipMemcpyAsync(o.colors, m.colors, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
		if (m.normals && !recompute) HIP_TRY(hipMemcpyAsync(o.normals, m.normals, (size_t)nv * 12, hipMemcpyDeviceToDevice, s));
	}
	if (nt) HIP_TRY(hipMemcpyAsync(o.indices, m.indices, (size_t)nt * 12, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (recompute && nv) { // of the output, with the defaults of rnb_mesh_vertex_normals
		VnResult vres;
		if (int rc = vn_run(call, o, 0u, o.normals, &vres); rc != RNB_OK) return rc;
	}
	hand_over(call.ws, o, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_edges = hres.n_edges; stats->n_interior = hres.n_interior; stats->n_boundary = hres.n_boundary; stats->n_nonmanifold = hres.n_nonmanifold; stats->n_unused = hres.n_unused;
		stats->n_selected = hres.n_selected; stats->n_moving = hres.n_moving; stats->max_valence = hres.max_valence; stats->passes = opt->passes; stats->n_wide = hres.n_wide;
		float md;
		std::memcpy(&md, &hres.max_displacement, 4);
		stats->max_displacement = (double)md;
		stats->ms_passes = ms_passes;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

// ---- snapping: guarded Newton steps onto the model's SDF (include/rnb_mesh_snap.h) ----
uint32_t rnb_mesh_snap_abi_version(void) { return RNB_MESH_SNAP_ABI_VERSION; }

int rnb_mesh_snap_default_options(rnb_mesh_snap_options* opt) try {
	if (!opt) return fail(RNB_ERR_INVALID, "opt is null");
	std::memset(opt, 0, sizeof(*opt));
	opt->abi_version = RNB_MESH_SNAP_ABI_VERSION;
	opt->iterations = 3;
	opt->tolerance = 1.0f / 8192.0f;
	opt->max_step = 1.0f / 128.0f;
	opt->max_displacement = 1.0f / 64.0f;
	opt->min_gradient = 0.25f;
	opt->use_inference_params = 1;
	return RNB_OK;
} RNB_GUARD

int rnb_mesh_snap(rnb_ctx* c, void* stream, const rnb_mesh* in, const rnb_mesh_snap_options* opt, const uint32_t* select_dev, rnb_mesh* out, float* residual_before_dev, float* residual_after_dev,
                  uint32_t* state_dev, float* displacement_dev, rnb_mesh_snap_stats* stats) try {
	if (!c || !in || !opt || !out) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: null argument");
	if (int rc = check_mesh_input("rnb_mesh_snap", in, out); rc != RNB_OK) return rc;
	const rnb_mesh m = *in;
	if (opt->abi_version != RNB_MESH_SNAP_ABI_VERSION) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: options abi_version mismatch (expected RNB_MESH_SNAP_ABI_VERSION)");
	if (opt->iterations > RNB_MESH_SNAP_MAX_ITERATIONS) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: iterations must be 0 .. 64");
	if (!std::isfinite(opt->level)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: level must be finite");
	if (!(std::isfinite(opt->tolerance) && opt->tolerance >= 0.0f)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: tolerance must be finite and at least 0");
	if (!(std::isfinite(opt->max_step) && opt->max_step > 0.0f)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: max_step must be finite and above 0");
	if (!(std::isfinite(opt->max_displacement) && opt->max_displacement >= 0.0f)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: max_displacement must be finite and at least 0");
	if (!(std::isfinite(opt->min_gradient) && opt->min_gradient > 0.0f)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: min_gradient must be finite and above 0");
	if (opt->attributes & ~(RNB_MESH_ATTR_COLORS | RNB_MESH_ATTR_NORMALS)) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: attributes must be a set of RNB_MESH_ATTR_COLORS and RNB_MESH_ATTR_NORMALS");
	if (opt->use_inference_params > 1u) return fail(RNB_ERR_INVALID, "rnb_mesh_snap: use_inference_params must be 0 or 1");
	if (int rc = check_reserved("rnb_mesh_snap", opt->reserved); rc != RNB_OK) return rc;
	MeshCall call("rnb_mesh_snap", c, stream);
	const hipStream_t s = call.s;

	const uint32_t nv = m.n_verts, nt = m.n_indices / 3u;
	const bool new_colors = (opt->attributes & RNB_MESH_ATTR_COLORS) != 0, new_normals = (opt->attributes & RNB_MESH_ATTR_NORMALS) != 0;
	SnResult hres;
	std::memset(&hres, 0, sizeof(hres));
	uint32_t rounds = 0;
	uint64_t n_points = 0;
	float ms_network = 0.0f;
	rnb_mesh o;
	if (!alloc_mesh(call.ws, &o, nv, nt, m.colors != nullptr || new_colors, m.normals != nullptr || new_normals)) return call.nomem("hipMalloc failed for the output mesh");
	if (nv) {
		const uint32_t g_v = groups(nv);
		float* prev = nullptr;
		double *a_prev = nullptr, *r_before = nullptr;
		uint32_t *state = nullptr, *flag = nullptr, *pos = nullptr, *list = nullptr, *scan = nullptr;
		SnResult* dres = nullptr;
		if (!call.ws.alloc(&prev, 3 * (size_t)nv) || !call.ws.alloc(&a_prev, nv) || !call.ws.alloc(&r_before, nv) || !call.ws.alloc(&state, nv) || !call.ws.alloc(&flag, nv) ||
		    !call.ws.alloc(&pos, nv) || !call.ws.alloc(&list, nv) || !call.ws.alloc(&scan, scan_scratch_elems(nv)) || !call.ws.alloc(&dres, 1))
			return call.nomem("hipMalloc failed for the workspace of " + std::to_string(nv) + " vertices");
		HIP_TRY(hipMemsetAsync(dres, 0, sizeof(SnResult), s));
		// 1. the triangles are only carried, but an index out of range is refused before anything else (pos's memory takes the marks of the check)
		if (nt)
			if (int rc = call.check_indices(m, pos, &dres->flags); rc != RNB_OK) return rc;
		const uint32_t per_launch = std::min<uint32_t>(opt->max_points_in_flight ? opt->max_points_in_flight : (1u << 20), RNB_MESH_SNAP_MAX_IN_FLIGHT);
		const uint32_t batch = std::min(per_launch, nv);
		float* coords = nullptr;
		half_t* net = nullptr;
		if (!call.ws.alloc(&coords, (size_t)batch * 7) || !call.ws.alloc(&net, (size_t)batch * 16)) return call.nomem("hipMalloc failed for a batch of " + std::to_string(batch) + " points");
		SnParams P;
		P.aabb_min = c->aabb.mn; P.aabb_diag = c->aabb.mx - c->aabb.mn;
		P.level = (double)opt->level; P.tolerance = (double)opt->tolerance; P.max_step = (double)opt->max_step; P.max_displacement = (double)opt->max_displacement;
		P.min_gradient2 = (double)opt->min_gradient * (double)opt->min_gradient; P.diag = (double)P.aabb_diag;
		const bool inference = opt->use_inference_params != 0;
		// 2. P = P_prev = P0; the unselected vertices' outputs; the attributes every vertex starts from
		call.launch(g_v, k_sn_init, (const float*)m.verts, select_dev, nv, o.verts, prev, a_prev, r_before, state, flag, dres);
		HIP_TRY(hipGetLastError());
		for (float* per_vertex : {residual_before_dev, residual_after_dev, displacement_dev})
			if (per_vertex) HIP_TRY(hipMemsetAsync(per_vertex, 0, (size_t)nv * 4, s));
		if (o.colors) { if (m.colors) HIP_TRY(hipMemcpyAsync(o.colors, m.colors, (size_t)nv * 12, hipMemcpyDeviceToDevice, s)); else HIP_TRY(hipMemsetAsync(o.colors, 0, (size_t)nv * 12, s)); }
		if (o.normals) { if (m.normals) HIP_TRY(hipMemcpyAsync(o.normals, m.normals, (size_t)nv * 12, hipMemcpyDeviceToDevice, s)); else HIP_TRY(hipMemsetAsync(o.normals, 0, (size_t)nv * 12, s)); }
		// The vertices whose flag is set, packed into list; their number is the host read. Then, batch by batch: inputs, the network, and `after` on its outputs.
		const auto evaluate = [&](uint32_t* n_out, auto&& after) -> int {
			uint32_t n = 0;
			*n_out = 0;
			HIP_TRY(hipMemcpyAsync(pos, flag, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
			if (int rc = scan_exclusive(pos, nv, s, &n, scan); rc != RNB_OK) return rc;
			*n_out = n;
			if (!n) return RNB_OK;
			call.launch(g_v, k_sn_pack, (const uint32_t*)flag, (const uint32_t*)pos, nv, list);
			for (uint32_t b0 = 0; b0 < n; b0 += batch) {
				const uint32_t nb = std::min(batch, n - b0);
				call.launch(groups(nb), k_sn_coords, (const uint32_t*)list + b0, nb, (const float*)o.verts, P.aabb_min, P.aabb_diag, coords);
				HIP_TRY(hipGetLastError());
				HIP_TRY(hipStreamSynchronize(s));
				const auto t_net = std::chrono::steady_clock::now();
				if (int rc = launch_forward(c, s, coords, nullptr, nb, net, inference); rc != RNB_OK) return rc;
				HIP_TRY(hipStreamSynchronize(s));
				ms_network += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_net).count();
				after((const uint32_t*)list + b0, nb);
				HIP_TRY(hipGetLastError());
				n_points += nb;
			}
			return RNB_OK;
		};
		// 3. the rounds
		for (uint32_t k = 1; k <= opt->iterations + 1u; ++k) {
			uint32_t n_active = 0;
			const int rc = evaluate(&n_active, [&](const uint32_t* l, uint32_t nb) {
				call.launch(groups(nb), k_sn_step, l, nb, (const half_t*)net, (const float*)m.verts, P, k == 1u ? 1u : 0u, k == opt->iterations + 1u ? 1u : 0u, o.verts, prev, a_prev, r_before,
				            residual_before_dev, state, flag);
			});
			if (rc != RNB_OK) return rc;
			if (!n_active) break;
			++rounds;
		}
		// 4. every selected vertex once more, at its final position
		call.launch(g_v, k_sn_selected, (const uint32_t*)state, nv, flag);
		uint32_t n_selected = 0;
		const int rc = evaluate(&n_selected, [&](const uint32_t* l, uint32_t nb) {
			call.launch(groups(nb), k_sn_final, l, nb, (const half_t*)net, (const float*)m.verts, (const float*)o.verts, P.level, (const double*)r_before, (const uint32_t*)state, residual_after_dev,
			            displacement_dev, new_colors ? o.colors : nullptr, new_normals ? o.normals : nullptr, dres);
		});
		if (rc != RNB_OK) return rc;
		if (state_dev) HIP_TRY(hipMemcpyAsync(state_dev, state, (size_t)nv * 4, hipMemcpyDeviceToDevice, s));
		HIP_TRY(hipMemcpyAsync(&hres, dres, sizeof(hres), hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		call.ws.release(prev, a_prev, r_before, state, flag, pos, list, scan);
		call.ws.release(dres, coords, net);
	}
	if (nt) HIP_TRY(hipMemcpyAsync(o.indices, m.indices, (size_t)nt * 12, hipMemcpyDeviceToDevice, s));
	HIP_TRY(hipStreamSynchronize(s));
	hand_over(call.ws, o, out);
	if (stats) {
		std::memset(stats, 0, sizeof(*stats));
		stats->n_unselected = hres.n_state[RNB_MESH_SNAP_UNSELECTED]; stats->n_converged = hres.n_state[RNB_MESH_SNAP_CONVERGED]; stats->n_unfinished = hres.n_state[RNB_MESH_SNAP_UNFINISHED];
		stats->n_flat = hres.n_state[RNB_MESH_SNAP_FLAT]; stats->n_leashed = hres.n_state[RNB_MESH_SNAP_LEASHED]; stats->n_outside = hres.n_state[RNB_MESH_SNAP_OUTSIDE];
		stats->n_stalled = hres.n_state[RNB_MESH_SNAP_STALLED]; stats->n_invalid = hres.n_state[RNB_MESH_SNAP_INVALID]; stats->n_reverted = hres.n_state[RNB_MESH_SNAP_REVERTED];
		stats->n_selected = nv - stats->n_unselected;
		stats->n_moved = hres.n_moved; stats->rounds = rounds;
		float md;
		std::memcpy(&md, &hres.max_displacement, 4);
		stats->max_displacement = (double)md;
		std::memcpy(&stats->max_before, &hres.max_before, 8);
		std::memcpy(&stats->max_after, &hres.max_after, 8);
		stats->sum_before_q = hres.sum_before_q; stats->sum_after_q = hres.sum_after_q;
		stats->n_network_points = n_points;
		stats->ms_network = ms_network;
		call.finish(stats);
	}
	return RNB_OK;
} RNB_GUARD

} // extern "C"
