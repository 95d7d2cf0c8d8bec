// kernels_mesh_intersect.cuh — the self-intersection stage of include/rnb_mesh_intersect.h (rnb_mesh_intersections, rnb_mesh_intersections_select): which pairs of
// triangles of one mesh pass through or touch each other, found through the uniform cell lists of the distance stage over the mesh's own box.
//   (k_mesh_validate of mesh_common.cuh comes first; then k_md_verts<true>, k_md_degenerate and k_md_register<FILL> of kernels_mesh_distance.cuh, unchanged: the used
//    vertices checked, the box, the triangles that take part, the cell lists and the large list. This file includes that header for them.)
//   k_mi_cells<WRITE>     one wavefront per cell list (a workgroup takes four cells at a time): the list staged in LDS, 32 + 32 triangles at a time, as doubles with
//                         their float boxes; the lanes spread over the (a, b) pairs of the tile; a pair is examined in the one cell the header's proof names
//   k_mi_large<WRITE>     one thread per (triangle, entry of the large list)
//   k_mi_tally            triangles with a partner, counted
//   k_mi_rank             the pair list: WRITE = false counts the reported pairs per lower triangle (-> scan_exclusive), WRITE = true writes them into that triangle's
//                         segment in the order the atomics hand out, k_mi_rank moves every record to its rank by t inside the segment
//   k_mi_sel_*, MiKeep    the selection of rnb_mesh_intersections_select and what MeshCall::compact keeps of it
// The class counts are integers added atomically, one atomic per reported pair and triangle: pairs that are not apart are a small fraction of the candidates (a few
// per thousand on an extracted surface), so they are not grouped over the wavefront first; the statistics are, lane by lane and then wave_sum. Operation for operation
// what tests/mesh_intersect_reference.py computes (this file is compiled with -ffp-contract=off; the pragma says so once more where it matters). Every sign routine
// is inlined: as real functions (tried: all of them, and mi_orient alone) the calls keep their live registers in scratch, 1088 and 448 bytes per lane; inlined, the pair
// kernel needs none (141 VGPRs, three wavefronts per SIMD; profiles/mesh_intersections.md).
// Vector loads, stores and atomics only.
#pragma once
#include "kernels_mesh_distance.cuh"
#include "../../include/rnb_mesh_intersect.h"

namespace rnb {

constexpr int MI_APART = 0, MI_COPLANAR = 4; // class of a pair: 0, RNB_MESH_INTERSECT_PROPER or _CONTACT; MI_COPLANAR: the bit mi_classify adds for n_coplanar_pairs
constexpr uint32_t MI_TILE = 32;              // triangles per half of a wavefront's LDS tile

struct MiResult { // written by the kernels, read by the driver
	uint32_t n_tris_proper, n_tris_contact, n_selected, pad;
	unsigned long long n_same, n_cand, n_proper, n_contact, n_coplanar, n_visited;
};
struct MiOut {
	uint32_t* n_proper;  // per triangle
	uint32_t* n_contact;
	uint32_t* own;       // WRITE = false: reported pairs per lower triangle, or null; WRITE = true: the cursors
	const uint32_t* offs; // WRITE = true: the exclusive sums of own
	rnb_mesh_intersect_pair* tmp;
};
struct V3 { double x, y, z; };
struct V2 { double i, j; };
struct MiTri { V3 p[3]; uint32_t i[3]; };
struct MiCount { unsigned long long same, cand, proper, contact, coplanar, visited; };

// rule 2
__device__ __forceinline__ int mi_orient(const V3 a, const V3 b, const V3 c, const V3 d) {
#pragma clang fp contract(off)
	const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z, wx = d.x - a.x, wy = d.y - a.y, wz = d.z - a.z;
	const double p0 = uy * vz, p1 = uz * vy, p2 = uz * vx, p3 = ux * vz, p4 = ux * vy, p5 = uy * vx;
	const double nx = p0 - p1, ny = p2 - p3, nz = p4 - p5;
	const double det = (nx * wx + ny * wy) + nz * wz;
	const double mx = fabs(p0) + fabs(p1), my = fabs(p2) + fabs(p3), mz = fabs(p4) + fabs(p5);
	const double P = (mx * fabs(wx) + my * fabs(wy)) + mz * fabs(wz);
	if (fabs(det) <= 0x1p-48 * P) return 0;
	return det > 0.0 ? 1 : -1;
}
// rule 3, on points already projected (mi_project)
__device__ __forceinline__ int mi_orient2(const V2 a, const V2 b, const V2 c) {
#pragma clang fp contract(off)
	const double l = (b.i - a.i) * (c.j - a.j), r = (b.j - a.j) * (c.i - a.i);
	const double d = l - r;
	if (fabs(d) <= 0x1p-50 * (fabs(l) + fabs(r))) return 0;
	return d > 0.0 ? 1 : -1;
}
__device__ __forceinline__ V2 mi_project(const V3 p, const int axis) { return axis == 0 ? V2{p.y, p.z} : axis == 1 ? V2{p.z, p.x} : V2{p.x, p.y}; }
__device__ __forceinline__ int mi_axis(const V3 a, const V3 b, const V3 c) {
#pragma clang fp contract(off)
	const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
	const double nx = fabs(uy * vz - uz * vy), ny = fabs(uz * vx - ux * vz), nz = fabs(ux * vy - uy * vx);
	int k = 0;
	double best = nx;
	if (ny > best) { k = 1; best = ny; }
	if (nz > best) k = 2;
	return k;
}
__device__ __forceinline__ V3 mi_pick(const V3 a, const V3 b, const V3 c, const int k) { return k == 0 ? a : k == 1 ? b : c; }

// rule 7: does an edge of X separate the corners of Y that are not exempt (eY: the exempt one, 3 = none)?
__device__ __forceinline__ bool mi_edges_separate(const V2 (&X)[3], const V2 (&Y)[3], const int eY) {
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const V2 e0 = X[k], e1 = X[(k + 1) % 3], e2 = X[(k + 2) % 3];
		const int ref = mi_orient2(e0, e1, e2);
		if (ref == 0) continue;
		bool ok = true;
#pragma unroll
		for (int j = 0; j < 3; ++j)
			if (j != eY && mi_orient2(e0, e1, Y[j]) * ref > 0) ok = false;
		if (ok) return true;
	}
	return false;
}
__device__ __forceinline__ bool mi_tri_tri_separated(const V3 s0, const V3 s1, const V3 s2, const V3 t0, const V3 t1, const V3 t2, const int eS, const int eT) {
	const int axis = mi_axis(t0, t1, t2);
	const V2 S[3] = {mi_project(s0, axis), mi_project(s1, axis), mi_project(s2, axis)}, T[3] = {mi_project(t0, axis), mi_project(t1, axis), mi_project(t2, axis)};
	return mi_edges_separate(T, S, eS) || mi_edges_separate(S, T, eT);
}
__device__ __forceinline__ bool mi_seg_tri_separated(const V3 p, const V3 q, const V3 a, const V3 b, const V3 c) {
	const int axis = mi_axis(a, b, c);
	const V2 F[3] = {mi_project(a, axis), mi_project(b, axis), mi_project(c, axis)}, P = mi_project(p, axis), Q = mi_project(q, axis);
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const V2 e0 = F[k], e1 = F[(k + 1) % 3], e2 = F[(k + 2) % 3];
		const int ref = mi_orient2(e0, e1, e2);
		if (ref == 0) continue;
		if (mi_orient2(e0, e1, P) * ref <= 0 && mi_orient2(e0, e1, Q) * ref <= 0) return true;
	}
	const int t0 = mi_orient2(P, Q, F[0]), t1 = mi_orient2(P, Q, F[1]), t2 = mi_orient2(P, Q, F[2]);
	return (t0 >= 0 && t1 >= 0 && t2 >= 0) || (t0 <= 0 && t1 <= 0 && t2 <= 0);
}
// step 3 of rule 6 for one edge (p, q) against F = (a, b, c): MI_APART (nothing), PROPER or CONTACT
__device__ __forceinline__ int mi_edge(const V3 p, const V3 q, const int sp, const int sq, const V3 a, const V3 b, const V3 c) {
	if (sp * sq > 0) return MI_APART;
	if (sp == 0 && sq == 0) return mi_seg_tri_separated(p, q, a, b, c) ? MI_APART : (int)RNB_MESH_INTERSECT_CONTACT;
	const int s1 = mi_orient(p, q, a, b), s2 = mi_orient(p, q, b, c), s3 = mi_orient(p, q, c, a);
	const bool pos = s1 > 0 || s2 > 0 || s3 > 0, neg = s1 < 0 || s2 < 0 || s3 < 0;
	if (pos && neg) return MI_APART;
	if (sp * sq < 0 && s1 == s2 && s2 == s3 && s1 != 0) return (int)RNB_MESH_INTERSECT_PROPER;
	return (int)RNB_MESH_INTERSECT_CONTACT;
}
// the signs of three corners without the exempt one e (3 = none): all equal and not 0; all 0
__device__ __forceinline__ bool mi_one_side(const int s0, const int s1, const int s2, const int e) {
	const int first = e == 0 ? s1 : s0;
	return first != 0 && (e == 0 || s0 == first) && (e == 1 || s1 == first) && (e == 2 || s2 == first);
}
__device__ __forceinline__ bool mi_all_zero(const int s0, const int s1, const int s2, const int e) { return (e == 0 || s0 == 0) && (e == 1 || s1 == 0) && (e == 2 || s2 == 0); }

// rules 5 and 6: the class of the candidate (S, T), S the lower triangle; n_shared indices in common (0 .. 2), at the positions whose sums are sumS, sumT
__device__ __forceinline__ int mi_classify(const V3 s0, const V3 s1, const V3 s2, const V3 t0, const V3 t1, const V3 t2, const int n_shared, const int sumS, const int sumT) {
	if (n_shared == 2) {
		const int kS = 3 - sumS, kT = 3 - sumT;
		const V3 dS = mi_pick(s0, s1, s2, kS);
		if (mi_orient(t0, t1, t2, dS) != 0) return MI_APART;
		const int axis = mi_axis(t0, t1, t2);
		const V2 p = mi_project(mi_pick(t0, t1, t2, (kT + 1) % 3), axis), q = mi_project(mi_pick(t0, t1, t2, (kT + 2) % 3), axis);
		const int a = mi_orient2(p, q, mi_project(dS, axis)), b = mi_orient2(p, q, mi_project(mi_pick(t0, t1, t2, kT), axis));
		return (a * b < 0 ? MI_APART : (int)RNB_MESH_INTERSECT_CONTACT) | MI_COPLANAR;
	}
	const int eS = n_shared ? sumS : 3, eT = n_shared ? sumT : 3;
	const int a0 = eS == 0 ? 0 : mi_orient(t0, t1, t2, s0), a1 = eS == 1 ? 0 : mi_orient(t0, t1, t2, s1), a2 = eS == 2 ? 0 : mi_orient(t0, t1, t2, s2);
	if (mi_one_side(a0, a1, a2, eS)) return MI_APART;
	const int b0 = eT == 0 ? 0 : mi_orient(s0, s1, s2, t0), b1 = eT == 1 ? 0 : mi_orient(s0, s1, s2, t1), b2 = eT == 2 ? 0 : mi_orient(s0, s1, s2, t2);
	if (mi_one_side(b0, b1, b2, eT)) return MI_APART;
	if (mi_all_zero(a0, a1, a2, eS) || mi_all_zero(b0, b1, b2, eT))
		return (mi_tri_tri_separated(s0, s1, s2, t0, t1, t2, eS, eT) ? MI_APART : (int)RNB_MESH_INTERSECT_CONTACT) | MI_COPLANAR;
	int seen = 0; // the classes the edges gave, as bits
	if (eS != 0 && eS != 1) seen |= mi_edge(s0, s1, a0, a1, t0, t1, t2);
	if (eS != 1 && eS != 2) seen |= mi_edge(s1, s2, a1, a2, t0, t1, t2);
	if (eS != 2 && eS != 0) seen |= mi_edge(s2, s0, a2, a0, t0, t1, t2);
	if (eT != 0 && eT != 1) seen |= mi_edge(t0, t1, b0, b1, s0, s1, s2);
	if (eT != 1 && eT != 2) seen |= mi_edge(t1, t2, b1, b2, s0, s1, s2);
	if (eT != 2 && eT != 0) seen |= mi_edge(t2, t0, b2, b0, s0, s1, s2);
	return (seen & RNB_MESH_INTERSECT_PROPER) ? (int)RNB_MESH_INTERSECT_PROPER : (seen & RNB_MESH_INTERSECT_CONTACT) ? (int)RNB_MESH_INTERSECT_CONTACT : MI_APART;
}

// Two triangles that take part and whose boxes overlap, a = triangle ta, b = triangle tb (ta != tb): rule 4's last test, the class, the outputs.
template <bool WRITE>
__device__ __forceinline__ void mi_examine(const MiTri& A, const uint32_t ta, const MiTri& B, const uint32_t tb, const MiOut& out, MiCount& n) {
	const bool a_first = ta < tb;
	const MiTri& S = a_first ? A : B;
	const MiTri& T = a_first ? B : A;
	const uint32_t s = a_first ? ta : tb, t = a_first ? tb : ta;
	int n_shared = 0, sumS = 0, sumT = 0;
#pragma unroll
	for (int x = 0; x < 3; ++x)
#pragma unroll
		for (int y = 0; y < 3; ++y)
			if (S.i[x] == T.i[y]) { ++n_shared; sumS += x; sumT += y; }
	if (n_shared == 3) { ++n.same; return; }
	++n.cand;
	const int r = mi_classify(S.p[0], S.p[1], S.p[2], T.p[0], T.p[1], T.p[2], n_shared, sumS, sumT);
	const uint32_t cls = (uint32_t)(r & 3);
	if (r & MI_COPLANAR) ++n.coplanar;
	if (cls == (uint32_t)MI_APART) return;
	if (WRITE) {
		const uint32_t slot = out.offs[s] + atomicAdd(out.own + s, 1u);
		out.tmp[slot].s = s; out.tmp[slot].t = t; out.tmp[slot].cls = cls;
		return;
	}
	if (cls == RNB_MESH_INTERSECT_PROPER) { ++n.proper; (void)atomicAdd(out.n_proper + s, 1u); (void)atomicAdd(out.n_proper + t, 1u); }
	else { ++n.contact; (void)atomicAdd(out.n_contact + s, 1u); (void)atomicAdd(out.n_contact + t, 1u); }
	if (out.own) (void)atomicAdd(out.own + s, 1u);
}
// the statistics of a wavefront's lanes, summed and added once (WRITE = true repeats the pass and adds nothing)
__device__ __forceinline__ void mi_flush(const MiCount& n, MiResult* __restrict__ res) {
	const long long same = wave_sum((long long)n.same), cand = wave_sum((long long)n.cand), proper = wave_sum((long long)n.proper), contact = wave_sum((long long)n.contact);
	const long long coplanar = wave_sum((long long)n.coplanar), visited = wave_sum((long long)n.visited);
	if ((threadIdx.x & 63u) != 0) return;
	if (same) (void)atomicAdd(&res->n_same, (unsigned long long)same);
	if (cand) (void)atomicAdd(&res->n_cand, (unsigned long long)cand);
	if (proper) (void)atomicAdd(&res->n_proper, (unsigned long long)proper);
	if (contact) (void)atomicAdd(&res->n_contact, (unsigned long long)contact);
	if (coplanar) (void)atomicAdd(&res->n_coplanar, (unsigned long long)coplanar);
	if (visited) (void)atomicAdd(&res->n_visited, (unsigned long long)visited);
}
__device__ __forceinline__ MiTri mi_load(const MdMesh& M, const uint32_t t) {
	MiTri r;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		r.i[k] = M.idx[3 * (size_t)t + k];
		const float* v = M.verts + 3 * (size_t)r.i[k];
		r.p[k] = V3{(double)v[0], (double)v[1], (double)v[2]};
	}
	return r;
}
__device__ __forceinline__ double mi_coord(const V3& p, const int k) { return k == 0 ? p.x : k == 1 ? p.y : p.z; }

// The LDS tile of one wavefront: 2 * MI_TILE triangles, component-major so that the lanes of a read fall on consecutive banks.
struct MiTile {
	double c[9][2 * MI_TILE];
	float lo[3][2 * MI_TILE], hi[3][2 * MI_TILE]; // the float box (the doubles are widened floats: their minimum is the floats')
	uint32_t idx[3][2 * MI_TILE];
	uint32_t tri[2 * MI_TILE];
	uint32_t c0[2 * MI_TILE];                      // the cell of the box's low corner, 8 bits per axis (dims <= 256)
};
static_assert(2 * MI_TILE == 64, "one triangle per lane is staged");
static_assert(RNB_MESH_DISTANCE_MAX_CELLS <= 256u, "a cell coordinate is packed into 8 bits");

__device__ __forceinline__ MiTri mi_from_tile(const MiTile& L, const uint32_t k) {
	MiTri r;
#pragma unroll
	for (int c = 0; c < 3; ++c) {
		r.p[c] = V3{L.c[3 * c][k], L.c[3 * c + 1][k], L.c[3 * c + 2][k]};
		r.i[c] = L.idx[c][k];
	}
	return r;
}

// A wavefront per cell: cell = 4 * blockIdx.x + wave, then on by 4 * gridDim.x. Every control decision below but the innermost `live` is uniform over the wavefront,
// and the four wavefronts of a workgroup never meet (wave_lds_sync orders a wavefront's own LDS traffic).
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_mi_cells(const MdGrid g, const MdMesh M, const uint32_t* __restrict__ start, const uint32_t* __restrict__ end, const uint32_t* __restrict__ entries,
                                                   const unsigned long long n_cells, const MiOut out, MiResult* __restrict__ res) {
	__shared__ MiTile tiles[MESH_WG / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	MiTile& L = tiles[wave];
	MiCount n = {0, 0, 0, 0, 0, 0};
	for (unsigned long long cell = (unsigned long long)blockIdx.x * (MESH_WG / 64) + wave; cell < n_cells; cell += (unsigned long long)gridDim.x * (MESH_WG / 64)) {
		const uint32_t e0 = start[cell], cnt = end[cell] - e0;
		if (cnt < 2u) continue;
		const uint32_t cx = (uint32_t)(cell % g.dims[0]), cy = (uint32_t)((cell / g.dims[0]) % g.dims[1]), cz = (uint32_t)(cell / ((unsigned long long)g.dims[0] * g.dims[1]));
		if (lane == 0) n.visited += (unsigned long long)cnt * (cnt - 1u) / 2u;
		for (uint32_t ib = 0; ib < cnt; ib += MI_TILE)
			for (uint32_t jb = ib; jb < cnt; jb += MI_TILE) {
				wave_lds_sync(); // the reads of the tile before are done
				const uint32_t src = lane < MI_TILE ? ib + lane : jb + (lane - MI_TILE);
				if (src < cnt) {
					const uint32_t t = entries[e0 + src];
					const MiTri tr = mi_load(M, t);
					uint32_t c0 = 0;
#pragma unroll
					for (int k = 0; k < 3; ++k) {
						const double lo = fmin(fmin(mi_coord(tr.p[0], k), mi_coord(tr.p[1], k)), mi_coord(tr.p[2], k)), hi = fmax(fmax(mi_coord(tr.p[0], k), mi_coord(tr.p[1], k)), mi_coord(tr.p[2], k));
						L.lo[k][lane] = (float)lo; L.hi[k][lane] = (float)hi; // exact: they are floats
						c0 |= md_cell(g, k, lo) << (8 * k);
						L.c[3 * k][lane] = tr.p[k].x; L.c[3 * k + 1][lane] = tr.p[k].y; L.c[3 * k + 2][lane] = tr.p[k].z;
						L.idx[k][lane] = tr.i[k];
					}
					L.tri[lane] = t; L.c0[lane] = c0;
				}
				wave_lds_sync();
				const uint32_t na = min(MI_TILE, cnt - ib), nb = min(MI_TILE, cnt - jb);
				for (uint32_t base = 0; base < na * MI_TILE; base += 64u) { // lanes over the pairs (a, j) of the tile: a = p / 32 from the first half, j = p % 32 from the second
					const uint32_t p = base + lane, a = p / MI_TILE, j = p % MI_TILE;
					const uint32_t b = ib == jb ? j : MI_TILE + j; // the same tile twice: every pair once, a < j
					const bool live = a < na && j < nb && (ib != jb || a < j);
					if (live) {
						const uint32_t ca = L.c0[a], cb = L.c0[b];
						const bool owner = max(ca & 0xFFu, cb & 0xFFu) == cx && max((ca >> 8) & 0xFFu, (cb >> 8) & 0xFFu) == cy && max(ca >> 16, cb >> 16) == cz;
						if (owner && L.lo[0][a] <= L.hi[0][b] && L.lo[0][b] <= L.hi[0][a] && L.lo[1][a] <= L.hi[1][b] && L.lo[1][b] <= L.hi[1][a] && L.lo[2][a] <= L.hi[2][b] &&
						    L.lo[2][b] <= L.hi[2][a])
							mi_examine<WRITE>(mi_from_tile(L, a), L.tri[a], mi_from_tile(L, b), L.tri[b], out, n);
					}
				}
			}
	}
	if (!WRITE) mi_flush(n, res);
}

// One thread per (triangle t, entry k of the large list): blockIdx.y = k. t meets the large triangle unless it is that triangle, takes no part, or is large itself
// and the higher-numbered of the two.
template <bool WRITE>
__global__ __launch_bounds__(MESH_WG) void k_mi_large(const MdGrid g, const MdMesh M, const uint32_t* __restrict__ large, const MiOut out, MiResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x, big = large[blockIdx.y];
	MiCount n = {0, 0, 0, 0, 0, 0};
	if (t < M.nt && t != big) {
		const MiTri A = mi_load(M, t);
		double a[3], b[3], c[3];
		md_corners(M, t, a, b, c);
		if (md_normal_length(a, b, c) != 0.0) {
			float lo[3], hi[3];
			uint32_t cells = 1;
#pragma unroll
			for (int k = 0; k < 3; ++k) {
				const double l = fmin(fmin(a[k], b[k]), c[k]), h = fmax(fmax(a[k], b[k]), c[k]);
				lo[k] = (float)l; hi[k] = (float)h;
				cells *= md_cell(g, k, h) - md_cell(g, k, l) + 1u;
			}
			if (cells <= RNB_MESH_DISTANCE_LARGE_CELLS || t < big) {
				++n.visited;
				const MiTri B = mi_load(M, big);
				bool overlap = true;
#pragma unroll
				for (int k = 0; k < 3; ++k) {
					const double l = fmin(fmin(mi_coord(B.p[0], k), mi_coord(B.p[1], k)), mi_coord(B.p[2], k)), h = fmax(fmax(mi_coord(B.p[0], k), mi_coord(B.p[1], k)), mi_coord(B.p[2], k));
					overlap = overlap && lo[k] <= (float)h && (float)l <= hi[k];
				}
				if (overlap) mi_examine<WRITE>(A, t, B, big, out, n);
			}
		}
	}
	if (!WRITE) mi_flush(n, res);
}

__global__ __launch_bounds__(MESH_WG) void k_mi_tally(const uint32_t* __restrict__ n_proper, const uint32_t* __restrict__ n_contact, const uint32_t nt, MiResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	const uint32_t np = (uint32_t)__popcll(__ballot(t < nt && n_proper[t] != 0u)), nc = (uint32_t)__popcll(__ballot(t < nt && n_contact[t] != 0u));
	if ((threadIdx.x & 63u) == 0) {
		if (np) (void)atomicAdd(&res->n_tris_proper, np);
		if (nc) (void)atomicAdd(&res->n_tris_contact, nc);
	}
}

// One thread per record of tmp, where the records of lower triangle s fill [offs[s], offs[s + 1]) in no order: its place is the number of records of the segment with a
// lower t (every t occurs once). Records beyond `capacity` are not written.
__global__ __launch_bounds__(MESH_WG) void k_mi_rank(const rnb_mesh_intersect_pair* __restrict__ tmp, const uint32_t* __restrict__ offs, const uint32_t total, rnb_mesh_intersect_pair* __restrict__ pairs,
                                                  const unsigned long long capacity) {
	const uint32_t e = blockIdx.x * MESH_WG + threadIdx.x;
	if (e >= total) return;
	const rnb_mesh_intersect_pair r = tmp[e];
	const uint32_t b0 = offs[r.s], b1 = offs[r.s + 1u];
	uint32_t rank = 0;
	for (uint32_t j = b0; j < b1; ++j) rank += tmp[j].t < r.t ? 1u : 0u;
	const unsigned long long dest = (unsigned long long)b0 + rank;
	if (dest < capacity) { pairs[dest].s = r.s; pairs[dest].t = r.t; pairs[dest].cls = r.cls; }
}

// ---- rnb_mesh_intersections_select ----
// flag[t] <- 1 for a triangle with a partner in one of `classes`
__global__ __launch_bounds__(MESH_WG) void k_mi_sel_flags(const uint32_t* __restrict__ n_proper, const uint32_t* __restrict__ n_contact, const uint32_t classes, const uint32_t nt, uint32_t* __restrict__ flag,
                                                       MiResult* __restrict__ res) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	bool sel = false;
	if (t < nt) {
		sel = ((classes & RNB_MESH_INTERSECT_PROPER) && n_proper[t] != 0u) || ((classes & RNB_MESH_INTERSECT_CONTACT) && n_contact[t] != 0u);
		flag[t] = sel ? 1u : 0u;
	}
	const uint32_t k = (uint32_t)__popcll(__ballot(sel));
	if ((threadIdx.x & 63u) == 0 && k) (void)atomicAdd(&res->n_selected, k);
}
// one ring: vmark[v] <- 1 for the corners of the selected triangles, then every triangle with a marked corner is selected
__global__ __launch_bounds__(MESH_WG) void k_mi_sel_mark(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t* __restrict__ flag, uint32_t* __restrict__ vmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt || !flag[t]) return;
	vmark[idx[3 * (size_t)t]] = 1u; vmark[idx[3 * (size_t)t + 1]] = 1u; vmark[idx[3 * (size_t)t + 2]] = 1u;
}
__global__ __launch_bounds__(MESH_WG) void k_mi_sel_grow(const uint32_t* __restrict__ idx, const uint32_t nt, uint32_t* __restrict__ flag, const uint32_t* __restrict__ vmark) {
	const uint32_t t = blockIdx.x * MESH_WG + threadIdx.x;
	if (t >= nt || flag[t]) return;
	if (vmark[idx[3 * (size_t)t]] | vmark[idx[3 * (size_t)t + 1]] | vmark[idx[3 * (size_t)t + 2]]) flag[t] = 1u; // (a thread writes its own word only)
}
// vkeep[v] <- 1 for the corners of the triangles that stay (zero on entry), or for every vertex (all)
__global__ __launch_bounds__(MESH_WG) void k_mi_sel_vkeep(const uint32_t* __restrict__ idx, const uint32_t nt, const uint32_t nv, const uint32_t* __restrict__ flag, const uint32_t all, uint32_t* __restrict__ vkeep) {
	const uint32_t i = blockIdx.x * MESH_WG + threadIdx.x;
	if (all) { if (i < nv) vkeep[i] = 1u; return; }
	if (i >= nt || flag[i]) return;
	vkeep[idx[3 * (size_t)i]] = 1u; vkeep[idx[3 * (size_t)i + 1]] = 1u; vkeep[idx[3 * (size_t)i + 2]] = 1u;
}
// What MeshCall::compact keeps of the input of rnb_mesh_intersections_select: the triangles that are not selected, and the vertices of vkeep.
struct MiKeep {
	const uint32_t* flag;  // 1 per selected triangle
	const uint32_t* vkeep; // 1 per kept vertex (k_mi_sel_vkeep)
	__device__ __forceinline__ bool vertex(const uint32_t v) const { return vkeep[v] != 0u; }
	__device__ __forceinline__ uint32_t triangle(const uint32_t*, const uint32_t t) const { return flag[t] ? 0u : 1u; }
};

} // namespace rnb
