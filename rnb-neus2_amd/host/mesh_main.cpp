// mesh_main.cpp — `./build/mesh`: the coloured mesh of a trained snapshot through the sparse extractor of include/rnb_mesh.h (the counterpart of the testbed's
// --save-mesh, which uses the dense path). The scene is read by the testbed's loader (dataset.hpp: scale, offset and the normalisation of the OBJ) and the
// snapshot by snapshot.hpp (its EMA weights, occupancy grid and network configuration).
//
//   mesh --snapshot PATH --scene DIR --out FILE.obj [--resolution R] [--cull none|occupancy] [--brick N] [--normals ring|gradient]
//        [--keep all|largest] [--orient none|outward] [--simplify N [--placement quadric|mean] [--report-error]] [--report-views [--views-out FILE]]
//        [--texture S [--texture-maps albedo[,normal]] [--texture-from views [--texture-mode blend|best] [--texture-depth-tolerance T] [--texture-min-cos C]]]
//        [--keep-seen component|faces [--seen-min-views N] [--seen-rings R] [--seen-masks [--seen-max-off N]] [--seen-supersample K]]
//        [--repair [--weld] [--duplicates keep|first|cancel] [--orient-consistent]] [--report-topology]
//        [--drop-intersecting proper|all [--drop-rings R]] [--fill-holes [--fill-max-edges N] [--fill-skip-largest]] [--report-intersections]
//        [--smooth N [--smooth-lambda L] [--smooth-mu M] [--smooth-boundary pin|slide|free] [--smooth-only-fills R] [--smooth-normals keep|recompute]]
//        [--snap N [--snap-tolerance T] [--snap-max-step S] [--snap-max-displacement D] [--snap-only-fills] [--snap-attributes keep|resample]] [--report-residual]
//
// The lattice is the testbed's: R rounded up to a multiple of 16, over the scene's bounding box, threshold 0. Vertex colours come from the device; the normals are the
// ring normals of mesh::compute_normals (default, as the testbed) or the device's SDF-gradient normals. The OBJ is written by mesh::save_obj as the testbed writes it.
// With --keep and / or --orient the device mesh goes through rnb_mesh_clean (include/rnb_mesh_clean.h) before it is downloaded: connected components, the largest one
// kept, triangles turned outward -- the pipeline's post-processing without the round trip through an OBJ. Without them nothing of that is called; with only one of
// them the other part is left alone (--keep alone does not turn anything, --orient alone keeps every component), as Context.extract_mesh(keep=, orient=) does.
// With --keep-seen the (cleaned) device mesh loses what no camera of the scene sees (rnb_mesh_visibility and rnb_mesh_visibility_select, include/rnb_mesh_visibility.h):
// whole connected components (component: a cavity shell inside the object goes, closed surfaces stay closed) or single triangles grown by --seen-rings rings (faces: a
// side no camera saw becomes a hole). With --seen-masks the alpha of the input normal maps are the masks, and --seen-max-off N also drops what lies off them in more
// than N views. It comes after --keep / --orient and before --simplify, as Context.extract_mesh(seen_by=) places it.
// With --simplify N the (cleaned) device mesh then goes through rnb_mesh_simplify (include/rnb_mesh_simplify.h): vertex clustering on N^3 cells over the scene's box
// (origin aabb_min, cell = (aabb_max - aabb_min) / N), the representative of a cell placed by --placement (quadric by default). Ring normals are those of the simplified mesh.
// With --report-error the distance between the simplifier's input and its output is measured on the device in both directions (rnb_mesh_distance,
// include/rnb_mesh_distance.h, default options) and printed as one more line.
// With --report-views the final mesh, still on the device and in the frame of the loaded views (before save_obj's scale and shift), is rasterised into every camera of the
// scene (rnb_mesh_raster, include/rnb_mesh_raster.h, default options) and compared with the input normal maps by view_metrics.hpp, as build/render compares the model's
// render: one line per view, the means, and <out>.views.json (or --views-out FILE) with the fields of render_metrics.json plus n_back_pixels and odd_count_pixels per view.
// With --texture S the mesh as finally written (after --keep, --orient and --simplify), still on the device, gets a texture bake (rnb_mesh_bake_texture,
// include/rnb_mesh_texture.h): a per-triangle atlas of S x S texels and the model's albedo (and, with --texture-maps albedo,normal, its SDF-gradient normal) at every
// texel. The output is then FILE.obj with vt records (mesh::save_obj_textured), FILE.mtl, FILE_albedo.png and FILE_normal.png.
// With --texture-from views the albedo map is not the model's but the scene's own albedo maps projected onto the mesh (rnb_mesh_project_views, include/rnb_mesh_project.h):
// the images as the loader read them (16 bit, their alpha the mask, the stored values as they are -- the scale the model's albedo and FILE_albedo.png have), every
// camera of the scene, the model's baked albedo as the fallback of the texels no view reaches. The atlas is the same one: the vt records do not change.
// With --texture and --report-views together the textured mesh, with the maps about to be written, is also drawn into every camera (rnb_mesh_draw_textured,
// include/rnb_mesh_draw.h): per view and in the means textured_mean_angle_deg and textured_median_angle_deg (when a normal map was baked: the normal-mapped surface
// against the input normal maps) and albedo_mae, albedo_rmse, albedo_psnr_db (when there is a colour map and the scene has albedo maps), with every digit of a double.
// A PSNR that is not finite (the drawn colours equal the input's: mse 0), per view or in the means, is written as null (view_metrics::num_full).
// With --repair the device mesh goes through rnb_mesh_repair (include/rnb_mesh_topology.h) after --simplify, whose clustering creates what it removes: degenerate
// triangles, duplicate triangles (--duplicates first, the default: one per vertex set stays; cancel: opposite windings cancel, a folded pair goes entirely; keep),
// with --weld vertices at one position first, with --orient-consistent every orientable patch wound consistently across its manifold edges. When --keep / --orient
// are given too, the cleaning then runs after the repair instead of first (extract, keep-seen, simplify, repair, clean), so that --orient outward acts on
// consistently wound components. With --report-topology the census of the mesh as written (rnb_mesh_topology) is printed as one JSON line, {"topology": {...}}.
// With --fill-holes the boundary loops of the device mesh are closed by rnb_mesh_fill_holes (include/rnb_mesh_holes.h) after --keep-seen, --simplify and --repair: a
// triangle for a loop of 3 edges, a fan around a new vertex at the centroid for a longer one; --fill-max-edges N leaves longer loops open, --fill-skip-largest the
// longest loop of every connected component (the rim of a relief). Boundary components that are not one simple cycle stay open and are counted in the `fill:` line.
// --keep / --orient, if given, then act on the filled mesh, as they do on the repaired one; --report-topology and --texture describe the filled mesh.
// With --drop-intersecting the triangles that pass through other triangles of the mesh (proper), or also those that touch or overlap them (all), are removed by
// rnb_mesh_intersections and rnb_mesh_intersections_select (include/rnb_mesh_intersect.h) after --simplify / --repair and before --fill-holes, which closes the rims;
// with --report-intersections the census of the mesh as written is printed as one JSON line, {"intersections": {...}}.
// With --smooth N the device mesh goes through N passes of rnb_mesh_smooth (include/rnb_mesh_smooth.h) right after --fill-holes (before --keep / --orient where they
// run late) and before the reports and --texture: Taubin's pairs with --smooth-lambda and --smooth-mu (0.5 and -0.53; mu 0 is plain Laplacian smoothing), the boundary
// pinned, sliding along itself or free; with --smooth-only-fills R only the vertices --fill-holes appended and R rings around them move, which relaxes the flat fans and
// leaves the rest as extracted. With --normals ring the host's ring normals are those of the smoothed positions; with --normals gradient the SDF-gradient normals would
// be stale, so --smooth-normals defaults to recompute there (the device's ring normals, the same direction) and to keep otherwise. One `smooth:` line is printed.
// With --snap N the vertices are then moved back onto the model's surface by up to N guarded Newton steps of rnb_mesh_snap (include/rnb_mesh_snap.h), right after
// --smooth and before the late --keep / --orient, the reports and --texture: a step of at most --snap-max-step, no vertex further than --snap-max-displacement from where
// it was (defaults: the box edge / 128 and / 64), done where |sdf| <= --snap-tolerance; with --snap-only-fills only the vertices --fill-holes appended and those --smooth
// moved are snapped. --snap-attributes resample (the default) takes the colours, and with --normals gradient the normals, of the snapped vertices from the model at the
// new positions; keep carries the old ones. One `snap:` line is printed. --report-residual prints {"residual": {...}}: mean and maximum |sdf| of the mesh as written.
// Exit codes as the testbed's: 0, 255 on a command-line error, 1 on a missing path or a failure.
#include "../../include/rnb_neus2.h"
#include "../../include/rnb_mesh.h"
#include "../../include/rnb_mesh_clean.h"
#include "../../include/rnb_mesh_simplify.h"
#include "../../include/rnb_mesh_distance.h"
#include "../../include/rnb_mesh_raster.h"
#include "../../include/rnb_mesh_texture.h"
#include "../../include/rnb_mesh_draw.h"
#include "../../include/rnb_mesh_visibility.h"
#include "../../include/rnb_mesh_project.h"
#include "../../include/rnb_mesh_topology.h"
#include "../../include/rnb_mesh_holes.h"
#include "../../include/rnb_mesh_intersect.h"
#include "../../include/rnb_mesh_smooth.h"
#include "../../include/rnb_mesh_snap.h"
#include "dataset.hpp"
#include "json_min.hpp"
#include "mesh.hpp"
#include "msgpack_min.hpp"
#include "png16.hpp"
#include "snapshot.hpp"
#include "view_metrics.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

using namespace hostio;

struct Flag { const char* name; const char* meta; const char* help; };
const Flag FLAGS[] = {
	{"snapshot", "PATH", "Trained snapshot (.msgpack) written by testbed --save-snapshot."},
	{"scene", "DIR", "The scene the snapshot was trained on: its bounding box and the normalisation of the mesh."},
	{"out", "FILE", "Output mesh (.obj)."},
	{"resolution", "R", "Lattice points per axis, rounded up to a multiple of 16 (default 256; at most 4096)."},
	{"cull", "MODE", "occupancy (default): skip the bricks the occupancy grid marks empty; none: evaluate the whole lattice."},
	{"brick", "N", "Lattice points per brick edge: 8, 16, 32 or 64 (default: the library's)."},
	{"normals", "MODE", "ring (default): area-weighted face normals, as the testbed; gradient: the SDF gradient at the vertex, from the device."},
	{"keep", "MODE", "Clean the mesh on the device. largest: only the connected component of the greatest area; all: every component."},
	{"orient", "MODE", "Clean the mesh on the device. outward: components of negative signed volume are turned inside out; none: triangles as extracted."},
	{"simplify", "N", "Simplify the mesh on the device: vertex clustering on N^3 cells over the scene's box (1 .. 1024), after the cleaning."},
	{"placement", "MODE", "--simplify only. quadric (default): the vertex of a cell minimises the quadric error of its triangles; mean: the mean of its vertices."},
	{"report-error", nullptr, "--simplify only (takes no value). Measure the distance between the mesh before and after the simplification, both directions, and print it."},
	{"report-views", nullptr, "(takes no value). Rasterise the final mesh into every camera of the scene and compare it with the input normal maps: normal angle and mask IoU per view."},
	{"views-out", "FILE", "--report-views only. Where the per-view report is written (default: the output mesh's path + .views.json)."},
	{"texture", "S", "Bake a texture of S x S texels (4 .. 8192) for the final mesh on the device: FILE.obj gets vt records, FILE.mtl and FILE_albedo.png are written beside it."},
	{"keep-seen", "MODE", "Drop what no camera of the scene sees, on the device, after the cleaning. component: whole connected components; faces: triangle by triangle (a side nobody saw becomes a hole)."},
	{"seen-min-views", "N", "--keep-seen only. A triangle counts as seen if at least N views see it (default 1)."},
	{"seen-rings", "R", "--keep-seen faces only. Grow the seen triangles by R rings of neighbours that share a vertex (0 .. 64, default 1)."},
	{"seen-masks", nullptr, "--keep-seen only (takes no value). Use the alpha of the input normal maps as masks: a pixel off the mask sees nothing."},
	{"seen-max-off", "N", "--seen-masks only. Also drop what lies off the mask in more than N views (default: the masks carve nothing)."},
	{"seen-supersample", "K", "--keep-seen only. Measure in views of K times the resolution (default 1); the masks stay as they are."},
	{"texture-maps", "LIST", "--texture only. The maps to bake, separated by commas: albedo (default), normal (the SDF gradient, object space, FILE_normal.png)."},
	{"texture-from", "SOURCE", "--texture only. views: the albedo map is projected from the scene's albedo maps through its cameras; the model's albedo fills what no view reaches."},
	{"texture-mode", "MODE", "--texture-from only. blend (default): the views weighted by cos^2 * alpha; best: the view of the greatest weight alone."},
	{"texture-depth-tolerance", "T", "--texture-from only. Relative depth slack of the occlusion test (>= 0, default 0.00390625)."},
	{"texture-min-cos", "C", "--texture-from only. A view that looks at the surface at a cosine of at most C is skipped ([0, 1), default 0.1)."},
	{"repair", nullptr, "(takes no value). Repair the mesh on the device after --simplify: degenerate and duplicate triangles go; --keep / --orient then act on the repaired mesh."},
	{"weld", nullptr, "--repair only (takes no value). Vertices at one position become one vertex first."},
	{"duplicates", "MODE", "--repair only. first (default): one triangle per vertex set stays; cancel: opposite windings cancel, folded pairs go entirely; keep: none is removed."},
	{"orient-consistent", nullptr, "--repair only (takes no value). Wind every orientable patch consistently across its shared edges, by the smaller set of flips."},
	{"fill-holes", nullptr, "(takes no value). Close the boundary loops of the mesh on the device, after --keep-seen, --simplify and --repair; --keep / --orient then act on the filled mesh."},
	{"fill-max-edges", "N", "--fill-holes only. Leave loops of more than N edges open (default: fill every simple loop)."},
	{"fill-skip-largest", nullptr, "--fill-holes only (takes no value). Leave the longest loop of every connected component open: the rim of a relief."},
	{"drop-intersecting", "MODE", "Remove self-intersecting triangles on the device. proper: those an edge of another triangle of the mesh passes through; all: also those that touch or overlap others; after --simplify / --repair and before --fill-holes."},
	{"drop-rings", "R", "--drop-intersecting only. Also remove R rings of triangles around them (0 .. 8, default 0)."},
	{"smooth", "N", "Smooth the mesh on the device with N passes (0 .. 10000) over the one-ring, after --fill-holes and before the reports and --texture: Taubin's lambda / mu pairs."},
	{"smooth-lambda", "L", "--smooth only. The factor of the odd passes (0 < L <= 1, default 0.5)."},
	{"smooth-mu", "M", "--smooth only. The factor of the even passes (-1.5 <= M <= 0, default -0.53); 0: every pass uses lambda (plain Laplacian smoothing, which shrinks)."},
	{"smooth-boundary", "MODE", "--smooth only. pin (default): boundary vertices stay; slide: they move along the boundary; free: they move like interior ones."},
	{"smooth-only-fills", "R", "--smooth with --fill-holes only. Move only the vertices --fill-holes appended and R rings of neighbours around them (0 .. 1024)."},
	{"smooth-normals", "MODE", "--smooth only. keep: the normals the mesh has; recompute: the device's ring normals of the smoothed mesh (default with --normals gradient)."},
	{"report-intersections", nullptr, "(takes no value). Print the self-intersection census of the written mesh as one JSON line: candidates, proper and contact pairs and triangles."},
	{"snap", "N", "Move the vertices back onto the model's surface with up to N guarded Newton steps (0 .. 64) along the SDF gradient, after --smooth and before the reports and --texture."},
	{"snap-tolerance", "T", "--snap only. A vertex is done where |sdf| <= T (T >= 0, default 2^-13)."},
	{"snap-max-step", "S", "--snap only. The longest single step, in world units (S > 0, default the box edge / 128)."},
	{"snap-max-displacement", "D", "--snap only. No vertex ends further than D from where it was, in world units (D >= 0, default the box edge / 64)."},
	{"snap-only-fills", nullptr, "(takes no value). --snap with --fill-holes only. Snap only the vertices --fill-holes appended and those --smooth moved."},
	{"snap-attributes", "MODE", "--snap only. resample (default): colours (and gradient normals) of the snapped vertices from the model at the new positions; keep: the old ones."},
	{"report-residual", nullptr, "(takes no value). Print mean and maximum |sdf| of the written mesh's vertices as one JSON line."},
	{"report-topology", nullptr, "(takes no value). Print the edge census of the written mesh as one JSON line: edges by kind, duplicates, patches, boundary loops, Euler characteristic."},
};
struct ParseError : std::runtime_error { using std::runtime_error::runtime_error; };

void print_help(std::ostream& os, const char* prog) {
	os << "  " << prog << " {OPTIONS}\n\n    coloured mesh of a trained snapshot, extracted brick by brick\n\n  OPTIONS:\n\n      -h, --help\n                                        Display this help menu.\n";
	for (const auto& f : FLAGS) os << "      --" << f.name << (f.meta ? std::string("=[") + f.meta + "]" : std::string()) << "\n                                        " << f.help << "\n";
}

std::map<std::string, std::string> parse_cli(int argc, char** argv, bool& help) {
	std::map<std::string, std::string> a;
	help = false;
	for (int i = 1; i < argc; ++i) {
		std::string tok = argv[i];
		if (tok == "-h" || tok == "--help") { help = true; continue; }
		if (tok.rfind("--", 0) != 0) throw ParseError("Passed in argument, but no positional arguments were ready to receive it: " + tok);
		std::string name = tok.substr(2), value;
		const size_t eq = name.find('=');
		bool inline_value = eq != std::string::npos;
		if (inline_value) { value = name.substr(eq + 1); name = name.substr(0, eq); }
		bool known = false, takes_value = true;
		for (const auto& f : FLAGS)
			if (name == f.name) { known = true; takes_value = f.meta != nullptr; }
		if (!known) throw ParseError("Flag could not be matched: " + name);
		if (!takes_value) {
			if (inline_value) throw ParseError("Flag '" + name + "' takes no argument");
			a[name] = "1";
			continue;
		}
		if (!inline_value) {
			if (i + 1 >= argc) throw ParseError("Flag '" + name + "' requires an argument but received none");
			value = argv[++i];
		}
		a[name] = value;
	}
	return a;
}

uint32_t parse_u32(const std::string& k, const std::string& s) {
	char* e = nullptr;
	const unsigned long long v = std::strtoull(s.c_str(), &e, 10);
	if (s.empty() || *e || s[0] == '-' || v > 0xffffffffull) throw ParseError("Argument '" + k + "' received invalid value type '" + s + "'");
	return (uint32_t)v;
}

double parse_double(const std::string& k, const std::string& s) {
	char* e = nullptr;
	const double v = std::strtod(s.c_str(), &e);
	if (s.empty() || *e || !std::isfinite(v)) throw ParseError("Argument '" + k + "' received invalid value type '" + s + "'");
	return v;
}

float parse_float(const std::string& k, const std::string& s) {
	char* e = nullptr;
	const float v = std::strtof(s.c_str(), &e);
	if (s.empty() || *e || !std::isfinite(v)) throw ParseError("Argument '" + k + "' received invalid value type '" + s + "'");
	return v;
}

#define RNB_CHECK(expr)                                                                          \
	do {                                                                                         \
		int rc_ = (expr);                                                                        \
		if (rc_ != RNB_OK) throw std::runtime_error(std::string(#expr) + ": " + rnb_last_error()); \
	} while (0)

// --report-views: the device mesh rasterised into every camera of the scene and compared with the input normal maps (view_metrics.hpp, as build/render compares the
// model's render). `report`: one line per view and the means, to print; `json`: the text of <out>.views.json. With `tex` (--texture: the maps about to be written, on the
// device) every view is also drawn with the texture (rnb_mesh_draw_textured, include/rnb_mesh_draw.h): the normal angle of the normal-mapped surface when a normal map was
// baked, the albedo error against the scene's albedo maps when there is a colour map and the scene has albedo maps. Without `tex` both texts are what they were.
void report_views(rnb_ctx* ctx, const Dataset& ds, const rnb_mesh& mesh, const rnb_mesh_draw_texture* tex, const std::string& snap_path, std::string& report, std::string& json) {
	using view_metrics::num;
	using view_metrics::num_full;
	rnb_mesh_raster_options ropt;
	RNB_CHECK(rnb_mesh_raster_default_options(&ropt));
	rnb_mesh_draw_options dopt;
	RNB_CHECK(rnb_mesh_draw_default_options(&dopt));
	bool with_albedo = tex && tex->color_dev && ds.albedos.size() == ds.views.size();
	for (size_t vi = 0; with_albedo && vi < ds.albedos.size(); ++vi) with_albedo = !ds.albedos[vi].rgba.empty();
	const bool with_normal = tex && tex->normal_dev;
	float* img_dev = nullptr;
	size_t cap = 0;
	double s_mean = 0, s_median = 0, s_iou = 0, s_ms = 0, s_tmean = 0, s_tmedian = 0, s_mae = 0, s_rmse = 0, s_psnr = 0, s_dms = 0;
	char line[256];
	try {
		for (uint32_t vi = 0; vi < ds.views.size(); ++vi) {
			const rnb_view v = ds.views[vi]; // the loaded view as it is: the camera the model was trained with, at its own size
			const png16::Image& in = ds.normals[vi];
			const size_t np = (size_t)v.width * v.height;
			if (np * RNB_MESH_RASTER_CHANNELS > cap) {
				if (img_dev) RNB_CHECK(rnb_device_free(ctx, img_dev));
				img_dev = nullptr;
				cap = np * RNB_MESH_RASTER_CHANNELS;
				RNB_CHECK(rnb_device_malloc(ctx, cap * 4, (void**)&img_dev));
			}
			rnb_mesh_raster_stats rs;
			RNB_CHECK(rnb_mesh_raster(ctx, nullptr, &mesh, &v, &ropt, img_dev, nullptr, &rs));
			std::vector<float> img(np * RNB_MESH_RASTER_CHANNELS);
			RNB_CHECK(rnb_memcpy(ctx, img.data(), img_dev, img.size() * 4, RNB_D2H));
			const view_metrics::Result vm = view_metrics::compare(img.data(), RNB_MESH_RASTER_CHANNELS, v.width, v.height, v.xform, in.rgba.data(), in.width, in.height);
			uint64_t odd = 0;
			for (size_t p = 0; p < np; ++p) odd += (uint64_t)img[p * RNB_MESH_RASTER_CHANNELS + 8] & 1u;
			s_mean += vm.mean_angle_deg; s_median += vm.median_angle_deg; s_iou += vm.mask_iou; s_ms += rs.ms;
			std::snprintf(line, sizeof(line), "view %u: %ux%u, mesh normal angle mean %.3f median %.3f deg, mask IoU %.4f, %u back-facing and %llu odd-count pixels, %.2f ms\n", vi, v.width,
			              v.height, vm.mean_angle_deg, vm.median_angle_deg, vm.mask_iou, rs.n_back_pixels, (unsigned long long)odd, rs.ms);
			report += line;
			std::string extra;
			if (with_normal || with_albedo) { // the textured mesh in the same camera
				rnb_mesh_draw_stats dst;
				RNB_CHECK(rnb_mesh_draw_textured(ctx, nullptr, &mesh, tex, &v, &dopt, img_dev, nullptr, &dst));
				RNB_CHECK(rnb_memcpy(ctx, img.data(), img_dev, img.size() * 4, RNB_D2H));
				s_dms += dst.raster.ms;
				report += "  textured:";
				if (with_normal) {
					const view_metrics::Result tm = view_metrics::compare(img.data(), RNB_MESH_RASTER_CHANNELS, v.width, v.height, v.xform, in.rgba.data(), in.width, in.height);
					s_tmean += tm.mean_angle_deg; s_tmedian += tm.median_angle_deg;
					extra += ", \"textured_mean_angle_deg\": " + num_full(tm.mean_angle_deg) + ", \"textured_median_angle_deg\": " + num_full(tm.median_angle_deg);
					std::snprintf(line, sizeof(line), " normal angle mean %.3f median %.3f deg,", tm.mean_angle_deg, tm.median_angle_deg);
					report += line;
				}
				if (with_albedo) {
					const png16::Image& al = ds.albedos[vi];
					const view_metrics::AlbedoResult ar = view_metrics::compare_albedo(img.data(), RNB_MESH_RASTER_CHANNELS, v.width, v.height, al.rgba.data(), al.width, al.height);
					s_mae += ar.mae; s_rmse += ar.rmse; s_psnr += ar.psnr_db;
					extra += ", \"albedo_mae\": " + num_full(ar.mae) + ", \"albedo_rmse\": " + num_full(ar.rmse) + ", \"albedo_psnr_db\": " + num_full(ar.psnr_db);
					std::snprintf(line, sizeof(line), " albedo mae %.5f rmse %.5f psnr %.2f dB,", ar.mae, ar.rmse, ar.psnr_db);
					report += line;
				}
				extra += ", \"textured_frame_ms\": " + num(dst.raster.ms);
				std::snprintf(line, sizeof(line), " %.2f ms\n", dst.raster.ms);
				report += line;
			}
			if (!json.empty()) json += ",\n";
			json += "    {\"view\": " + std::to_string(vi) + ", \"width\": " + std::to_string(v.width) + ", \"height\": " + std::to_string(v.height) + ", " +
			              view_metrics::json_fields(vm) + ", \"n_back_pixels\": " + std::to_string(rs.n_back_pixels) + ", \"odd_count_pixels\": " + std::to_string(odd) +
			              ", \"frame_ms\": " + num(rs.ms) + extra + "}";
		}
	} catch (...) {
		if (img_dev) rnb_device_free(ctx, img_dev);
		throw;
	}
	if (img_dev) RNB_CHECK(rnb_device_free(ctx, img_dev));
	const double k = ds.views.empty() ? 1.0 : (double)ds.views.size();
	std::snprintf(line, sizeof(line), "views: %zu, mesh normal angle mean %.3f median %.3f deg, mask IoU %.4f, %.2f ms per view\n", ds.views.size(), s_mean / k, s_median / k, s_iou / k, s_ms / k);
	report += line;
	std::string extra;
	if (with_normal || with_albedo) {
		report += "views textured:";
		if (with_normal) {
			extra += ", \"textured_mean_angle_deg\": " + num_full(s_tmean / k) + ", \"textured_median_angle_deg\": " + num_full(s_tmedian / k);
			std::snprintf(line, sizeof(line), " normal angle mean %.3f median %.3f deg,", s_tmean / k, s_tmedian / k);
			report += line;
		}
		if (with_albedo) {
			extra += ", \"albedo_mae\": " + num_full(s_mae / k) + ", \"albedo_rmse\": " + num_full(s_rmse / k) + ", \"albedo_psnr_db\": " + num_full(s_psnr / k);
			std::snprintf(line, sizeof(line), " albedo mae %.5f rmse %.5f psnr %.2f dB,", s_mae / k, s_rmse / k, s_psnr / k);
			report += line;
		}
		extra += ", \"textured_frame_ms\": " + num(s_dms / k);
		std::snprintf(line, sizeof(line), " %.2f ms per view\n", s_dms / k);
		report += line;
	}
	json = "{\n  \"snapshot\": \"" + snap_path + "\",\n  \"n_triangles\": " + std::to_string(mesh.n_indices / 3u) + ",\n  \"views\": [\n" + json + "\n  ],\n  \"mean\": {\"mean_angle_deg\": " +
	             num(s_mean / k) + ", \"median_angle_deg\": " + num(s_median / k) + ", \"mask_iou\": " + num(s_iou / k) + ", \"frame_ms\": " + num(s_ms / k) + extra + "}\n}\n";
}

// --keep-seen: *dm without what the cameras of the scene do not see, in *out. `report`: the two lines to print.
struct SeenOptions { uint32_t unit = RNB_MESH_VISIBILITY_UNIT_COMPONENT, min_views = 1, rings = 1, max_off = 0xFFFFFFFFu, supersample = 1; bool masks = false; };
void keep_seen(rnb_ctx* ctx, const Dataset& ds, const rnb_mesh& dm, const SeenOptions& so, rnb_mesh* out, std::string& report) {
	std::vector<rnb_mesh_visibility_view> views(ds.views.size());
	std::vector<void*> held;
	rnb_mesh_face_visibility* faces = nullptr;
	rnb_mesh_visibility_stats vs;
	rnb_mesh_visibility_select_stats ss;
	try {
		for (size_t vi = 0; vi < ds.views.size(); ++vi) {
			rnb_mesh_visibility_view& V = views[vi];
			std::memset(&V, 0, sizeof(V));
			V.view = ds.views[vi];
			const uint64_t w = (uint64_t)V.view.width * so.supersample, h = (uint64_t)V.view.height * so.supersample; // api.scaled_view(view, K) for a whole K
			if (w > RNB_MESH_RASTER_MAX_SIZE || h > RNB_MESH_RASTER_MAX_SIZE) throw std::runtime_error("--seen-supersample: view " + std::to_string(vi) + " would exceed 16384 pixels per side");
			V.view.focal_length[0] = (float)((double)V.view.focal_length[0] * (double)w / (double)V.view.width);
			V.view.focal_length[1] = (float)((double)V.view.focal_length[1] * (double)h / (double)V.view.height);
			V.view.width = (uint32_t)w; V.view.height = (uint32_t)h;
			if (so.masks) {
				const png16::Image& in = ds.normals[vi];
				std::vector<uint8_t> m((size_t)in.width * in.height);
				for (size_t p = 0; p < m.size(); ++p) m[p] = in.rgba[4 * p + 3] > 0 ? 1 : 0; // the input mask of view_metrics.hpp
				if (m.empty()) throw std::runtime_error("--seen-masks: the normal map of view " + std::to_string(vi) + " is empty");
				void* d = nullptr;
				RNB_CHECK(rnb_device_malloc(ctx, m.size(), &d));
				held.push_back(d);
				RNB_CHECK(rnb_memcpy(ctx, d, m.data(), m.size(), RNB_H2D));
				V.mask_dev = (const uint8_t*)d; V.mask_width = in.width; V.mask_height = in.height;
			}
		}
		RNB_CHECK(rnb_device_malloc(ctx, std::max<uint64_t>(dm.n_indices / 3u, 1) * sizeof(rnb_mesh_face_visibility), (void**)&faces));
		held.push_back(faces);
		rnb_mesh_visibility_options vo;
		RNB_CHECK(rnb_mesh_visibility_default_options(&vo));
		RNB_CHECK(rnb_mesh_visibility(ctx, nullptr, &dm, views.data(), (uint32_t)views.size(), &vo, faces, &vs));
		rnb_mesh_visibility_select_options lo;
		RNB_CHECK(rnb_mesh_visibility_select_default_options(&lo));
		lo.unit = so.unit; lo.min_views_seen = so.min_views; lo.max_views_off_mask = so.max_off; lo.rings = so.rings;
		RNB_CHECK(rnb_mesh_visibility_select(ctx, nullptr, &dm, faces, &lo, out, nullptr, &ss));
	} catch (...) {
		for (void* p : held) rnb_device_free(ctx, p);
		throw;
	}
	for (void* p : held) RNB_CHECK(rnb_device_free(ctx, p));
	char line[320];
	std::snprintf(line, sizeof(line), "seen: %u views, %llu pixels, %u of %u triangles seen, %u off the mask, peak workspace %.1f MB, %.1f ms\n", vs.n_views, (unsigned long long)vs.n_pixels,
	              vs.n_faces_seen, vs.n_tris, vs.n_faces_off_mask, (double)vs.peak_workspace / 1e6, vs.ms);
	report += line;
	std::snprintf(line, sizeof(line), "keep-seen %s: %u seeds, %u candidates, %u components of which %u kept, %u -> %u triangles, %u -> %u vertices, %.1f ms\n",
	              so.unit == RNB_MESH_VISIBILITY_UNIT_FACE ? "faces" : "component", ss.n_seeds, ss.n_candidates, ss.n_components, ss.n_components_kept, ss.n_tris_in, ss.n_tris_out, ss.n_verts_in,
	              ss.n_verts_out, ss.ms);
	report += line;
}

// --texture-from views: the scene's albedo maps projected onto *dm in the atlas of the bake `dt`, whose albedo is the fallback. `color`: the map, float[S][S][4].
struct ProjectOptions { uint32_t mode = RNB_MESH_PROJECT_MODE_BLEND; float depth_tolerance = 1.0f / 256.0f, min_cos = 0.1f; bool tolerance_given = false, min_cos_given = false; };
void project_views(rnb_ctx* ctx, const Dataset& ds, const rnb_mesh& dm, const rnb_mesh_texture& dt, const ProjectOptions& po, std::vector<float>& color, std::string& report) {
	std::vector<rnb_mesh_project_view> views(ds.views.size());
	std::vector<void*> held;
	rnb_mesh_projection pr;
	rnb_mesh_project_stats ps;
	std::memset(&pr, 0, sizeof(pr));
	try {
		for (size_t vi = 0; vi < ds.views.size(); ++vi) {
			const png16::Image& in = ds.albedos[vi];
			if (in.rgba.empty()) throw std::runtime_error("--texture-from: the albedo map of view " + std::to_string(vi) + " is empty");
			void* d = nullptr;
			RNB_CHECK(rnb_device_malloc(ctx, in.rgba.size() * 2, &d));
			held.push_back(d);
			RNB_CHECK(rnb_memcpy(ctx, d, in.rgba.data(), in.rgba.size() * 2, RNB_H2D));
			rnb_mesh_project_view& V = views[vi];
			std::memset(&V, 0, sizeof(V));
			V.view = ds.views[vi];
			V.image_dev = d; V.image_width = in.width; V.image_height = in.height; V.format = RNB_MESH_PROJECT_FORMAT_U16;
		}
		rnb_mesh_project_options o;
		RNB_CHECK(rnb_mesh_project_default_options(&o));
		o.size = dt.size; o.block = dt.block; o.mode = po.mode;
		o.normals = dm.normals ? RNB_MESH_PROJECT_NORMALS_VERTEX : RNB_MESH_PROJECT_NORMALS_FACE;
		if (po.tolerance_given) o.depth_tolerance = po.depth_tolerance;
		if (po.min_cos_given) o.min_cos = po.min_cos;
		o.fallback_dev = dt.albedo;
		RNB_CHECK(rnb_mesh_project_views(ctx, nullptr, &dm, views.data(), (uint32_t)views.size(), &o, &pr, &ps));
		color.resize((size_t)pr.size * pr.size * 4);
		RNB_CHECK(rnb_memcpy(ctx, color.data(), pr.color, (uint64_t)color.size() * 4, RNB_D2H));
	} catch (...) {
		rnb_mesh_projection_free(ctx, &pr);
		for (void* p : held) rnb_device_free(ctx, p);
		throw;
	}
	RNB_CHECK(rnb_mesh_projection_free(ctx, &pr));
	for (void* p : held) RNB_CHECK(rnb_device_free(ctx, p));
	char line[320];
	std::snprintf(line, sizeof(line), "texture from %zu views (%s): %llu of %llu texels textured, %llu pairs tested of which %llu occluded, peak workspace %.1f MB, %.1f ms\n", ds.views.size(),
	              po.mode == RNB_MESH_PROJECT_MODE_BEST ? "best" : "blend", (unsigned long long)ps.n_textured, (unsigned long long)ps.n_texels, (unsigned long long)ps.n_pairs_tested,
	              (unsigned long long)ps.n_occluded, (double)ps.peak_workspace / 1e6, ps.ms);
	report += line;
}

} // namespace

// The mean |sdf| behind a sum of trunc(|r| * 2^24) over n vertices (rnb_mesh_snap_stats).
static double residual_mean(uint64_t sum_q, uint32_t n) { return n ? (double)sum_q / (double)(1u << RNB_MESH_SNAP_Q_SHIFT) / (double)n : 0.0; }

int main(int argc, char** argv) {
	std::map<std::string, std::string> a;
	uint32_t resolution = 256, brick = 0, cull = RNB_MESH_CULL_OCCUPANCY;
	bool gradient = false, clean = false;
	uint32_t keep = RNB_MESH_KEEP_ALL, orient = RNB_MESH_ORIENT_NONE; // with one of the two flags given, the other one leaves its part alone
	uint32_t simplify = 0, placement = RNB_MESH_PLACE_QUADRIC;           // 0: no simplification
	bool report_error = false, want_views = false;
	uint32_t texture = 0, texture_maps = RNB_MESH_TEXTURE_ALBEDO; // 0: no texture
	bool want_seen = false, texture_from = false;
	SeenOptions seen;
	ProjectOptions project;
	bool repair = false, report_topology = false, fill_holes = false;
	uint32_t fill_max_edges = 0;
	bool report_intersections = false;
	uint32_t drop_classes = 0, drop_rings = 0; // 0: nothing is dropped
	rnb_mesh_repair_options repair_opt;
	std::memset(&repair_opt, 0, sizeof(repair_opt));
	bool smooth = false, smooth_only_fills = false;
	rnb_mesh_smooth_options smooth_opt;
	(void)rnb_mesh_smooth_default_options(&smooth_opt); // (touches no device)
	bool snap = false, snap_only_fills = false, snap_resample = true, snap_step_given = false, snap_leash_given = false, report_residual = false;
	rnb_mesh_snap_options snap_opt;
	(void)rnb_mesh_snap_default_options(&snap_opt); // (touches no device)
	try {
		bool help = false;
		a = parse_cli(argc, argv, help);
		if (help) { print_help(std::cout, argv[0]); return 0; }
		if (!a.count("snapshot") || !a.count("scene") || !a.count("out")) throw ParseError("--snapshot, --scene and --out are required");
		if (a.count("resolution")) resolution = parse_u32("resolution", a["resolution"]);
		if (resolution == 0 || resolution > RNB_MESH_MAX_RES) throw ParseError("Argument 'resolution' must be 1 .. 4096");
		if (a.count("brick")) brick = parse_u32("brick", a["brick"]);
		if (brick != 0 && brick != 8 && brick != 16 && brick != 32 && brick != 64) throw ParseError("Argument 'brick' must be 8, 16, 32 or 64");
		if (a.count("cull")) {
			if (a["cull"] == "none") cull = RNB_MESH_CULL_NONE;
			else if (a["cull"] != "occupancy") throw ParseError("Argument 'cull' must be none or occupancy");
		}
		if (a.count("normals")) {
			if (a["normals"] == "gradient") gradient = true;
			else if (a["normals"] != "ring") throw ParseError("Argument 'normals' must be ring or gradient");
		}
		if (a.count("keep")) {
			clean = true;
			if (a["keep"] == "largest") keep = RNB_MESH_KEEP_LARGEST;
			else if (a["keep"] != "all") throw ParseError("Argument 'keep' must be all or largest");
		}
		if (a.count("orient")) {
			clean = true;
			if (a["orient"] == "outward") orient = RNB_MESH_ORIENT_OUTWARD;
			else if (a["orient"] != "none") throw ParseError("Argument 'orient' must be none or outward");
		}
		if (a.count("simplify")) {
			simplify = parse_u32("simplify", a["simplify"]);
			if (simplify == 0 || (uint64_t)simplify * simplify * simplify > RNB_MESH_SIMPLIFY_MAX_CELLS) throw ParseError("Argument 'simplify' must be 1 .. 1024");
		}
		if (a.count("placement")) {
			if (!simplify) throw ParseError("Argument 'placement' is only used with --simplify");
			if (a["placement"] == "mean") placement = RNB_MESH_PLACE_MEAN;
			else if (a["placement"] != "quadric") throw ParseError("Argument 'placement' must be quadric or mean");
		}
		if (a.count("report-error")) {
			if (!simplify) throw ParseError("Argument 'report-error' is only used with --simplify");
			report_error = true;
		}
		if (a.count("report-views")) want_views = true;
		if (a.count("views-out") && !want_views) throw ParseError("Argument 'views-out' is only used with --report-views");
		if (a.count("keep-seen")) {
			want_seen = true;
			if (a["keep-seen"] == "faces") seen.unit = RNB_MESH_VISIBILITY_UNIT_FACE;
			else if (a["keep-seen"] != "component") throw ParseError("Argument 'keep-seen' must be component or faces");
		}
		for (const char* sub : {"seen-min-views", "seen-rings", "seen-masks", "seen-max-off", "seen-supersample"})
			if (a.count(sub) && !want_seen) throw ParseError(std::string("Argument '") + sub + "' is only used with --keep-seen");
		if (a.count("seen-min-views")) seen.min_views = parse_u32("seen-min-views", a["seen-min-views"]);
		if (a.count("seen-rings")) {
			if (seen.unit != RNB_MESH_VISIBILITY_UNIT_FACE) throw ParseError("Argument 'seen-rings' is only used with --keep-seen faces");
			seen.rings = parse_u32("seen-rings", a["seen-rings"]);
			if (seen.rings > RNB_MESH_VISIBILITY_MAX_RINGS) throw ParseError("Argument 'seen-rings' must be 0 .. 64");
		}
		if (a.count("seen-masks")) seen.masks = true;
		if (a.count("seen-max-off")) {
			if (!seen.masks) throw ParseError("Argument 'seen-max-off' is only used with --seen-masks");
			seen.max_off = parse_u32("seen-max-off", a["seen-max-off"]);
		}
		if (a.count("seen-supersample")) {
			seen.supersample = parse_u32("seen-supersample", a["seen-supersample"]);
			if (seen.supersample == 0 || seen.supersample > RNB_MESH_RASTER_MAX_SIZE) throw ParseError("Argument 'seen-supersample' must be 1 .. 16384");
		}
		if (a.count("texture")) {
			texture = parse_u32("texture", a["texture"]);
			if (texture < RNB_MESH_TEXTURE_MIN_SIZE || texture > RNB_MESH_TEXTURE_MAX_SIZE) throw ParseError("Argument 'texture' must be 4 .. 8192");
		}
		if (a.count("texture-maps")) {
			if (!texture) throw ParseError("Argument 'texture-maps' is only used with --texture");
			texture_maps = 0;
			const std::string list = a["texture-maps"] + ",";
			for (size_t p = 0, q; (q = list.find(',', p)) != std::string::npos; p = q + 1) {
				const std::string name = list.substr(p, q - p);
				if (name == "albedo") texture_maps |= RNB_MESH_TEXTURE_ALBEDO;
				else if (name == "normal") texture_maps |= RNB_MESH_TEXTURE_NORMAL;
				else throw ParseError("Argument 'texture-maps' must be a list of albedo and normal");
			}
		}
		if (a.count("texture-from")) {
			if (!texture) throw ParseError("Argument 'texture-from' is only used with --texture");
			if (a["texture-from"] != "views") throw ParseError("Argument 'texture-from' must be views");
			texture_from = true;
		}
		for (const char* sub : {"texture-mode", "texture-depth-tolerance", "texture-min-cos"})
			if (a.count(sub) && !texture_from) throw ParseError(std::string("Argument '") + sub + "' is only used with --texture-from");
		if (a.count("texture-mode")) {
			if (a["texture-mode"] == "best") project.mode = RNB_MESH_PROJECT_MODE_BEST;
			else if (a["texture-mode"] != "blend") throw ParseError("Argument 'texture-mode' must be blend or best");
		}
		if (a.count("texture-depth-tolerance")) {
			project.depth_tolerance = parse_float("texture-depth-tolerance", a["texture-depth-tolerance"]);
			project.tolerance_given = true;
			if (!(project.depth_tolerance >= 0.0f)) throw ParseError("Argument 'texture-depth-tolerance' must not be negative");
		}
		if (a.count("texture-min-cos")) {
			project.min_cos = parse_float("texture-min-cos", a["texture-min-cos"]);
			project.min_cos_given = true;
			if (!(project.min_cos >= 0.0f && project.min_cos < 1.0f)) throw ParseError("Argument 'texture-min-cos' must be in [0, 1)");
		}
		if (a.count("repair")) repair = true;
		for (const char* sub : {"weld", "duplicates", "orient-consistent"})
			if (a.count(sub) && !repair) throw ParseError(std::string("Argument '") + sub + "' is only used with --repair");
		if (a.count("duplicates") && a["duplicates"] != "keep" && a["duplicates"] != "first" && a["duplicates"] != "cancel") throw ParseError("Argument 'duplicates' must be keep, first or cancel");
		if (a.count("report-topology")) report_topology = true;
		if (a.count("fill-holes")) fill_holes = true;
		for (const char* sub : {"fill-max-edges", "fill-skip-largest"})
			if (a.count(sub) && !fill_holes) throw ParseError(std::string("Argument '") + sub + "' is only used with --fill-holes");
		if (a.count("fill-max-edges")) {
			fill_max_edges = parse_u32("fill-max-edges", a["fill-max-edges"]);
			if (fill_max_edges < 3) throw ParseError("Argument 'fill-max-edges' must be at least 3");
		}
		if (a.count("report-intersections")) report_intersections = true;
		if (a.count("drop-intersecting")) {
			if (a["drop-intersecting"] == "proper") drop_classes = RNB_MESH_INTERSECT_PROPER;
			else if (a["drop-intersecting"] == "all") drop_classes = RNB_MESH_INTERSECT_PROPER | RNB_MESH_INTERSECT_CONTACT;
			else throw ParseError("Argument 'drop-intersecting' must be proper or all");
		}
		if (a.count("drop-rings")) {
			if (!drop_classes) throw ParseError("Argument 'drop-rings' is only used with --drop-intersecting");
			drop_rings = parse_u32("drop-rings", a["drop-rings"]);
			if (drop_rings > RNB_MESH_INTERSECT_MAX_RINGS) throw ParseError("Argument 'drop-rings' must be 0 .. 8");
		}
		if (a.count("smooth")) {
			smooth = true;
			smooth_opt.passes = parse_u32("smooth", a["smooth"]);
			if (smooth_opt.passes > RNB_MESH_SMOOTH_MAX_PASSES) throw ParseError("Argument 'smooth' must be 0 .. 10000");
		}
		for (const char* sub : {"smooth-lambda", "smooth-mu", "smooth-boundary", "smooth-only-fills", "smooth-normals"})
			if (a.count(sub) && !smooth) throw ParseError(std::string("Argument '") + sub + "' is only used with --smooth");
		if (a.count("smooth-lambda")) {
			smooth_opt.lambda = parse_double("smooth-lambda", a["smooth-lambda"]);
			if (!(smooth_opt.lambda > 0.0 && smooth_opt.lambda <= 1.0)) throw ParseError("Argument 'smooth-lambda' must be above 0 and at most 1");
		}
		if (a.count("smooth-mu")) {
			smooth_opt.mu = parse_double("smooth-mu", a["smooth-mu"]);
			if (!(smooth_opt.mu >= -1.5 && smooth_opt.mu <= 0.0)) throw ParseError("Argument 'smooth-mu' must be at least -1.5 and at most 0");
		}
		if (a.count("smooth-boundary")) {
			if (a["smooth-boundary"] == "slide") smooth_opt.boundary = RNB_MESH_SMOOTH_BOUNDARY_SLIDE;
			else if (a["smooth-boundary"] == "free") smooth_opt.boundary = RNB_MESH_SMOOTH_BOUNDARY_FREE;
			else if (a["smooth-boundary"] != "pin") throw ParseError("Argument 'smooth-boundary' must be pin, slide or free");
		}
		if (a.count("smooth-only-fills")) {
			if (!fill_holes) throw ParseError("Argument 'smooth-only-fills' is only used with --fill-holes");
			smooth_only_fills = true;
			smooth_opt.select_rings = parse_u32("smooth-only-fills", a["smooth-only-fills"]);
			if (smooth_opt.select_rings > RNB_MESH_SMOOTH_MAX_SELECT_RINGS) throw ParseError("Argument 'smooth-only-fills' must be 0 .. 1024");
		}
		if (smooth && gradient) smooth_opt.normals = RNB_MESH_SMOOTH_NORMALS_RECOMPUTE; // the SDF-gradient normals of the old positions would be stale
		if (a.count("smooth-normals")) {
			if (a["smooth-normals"] == "recompute") smooth_opt.normals = RNB_MESH_SMOOTH_NORMALS_RECOMPUTE;
			else if (a["smooth-normals"] == "keep") smooth_opt.normals = RNB_MESH_SMOOTH_NORMALS_KEEP;
			else throw ParseError("Argument 'smooth-normals' must be keep or recompute");
		}
		if (a.count("report-residual")) report_residual = true;
		if (a.count("snap")) {
			snap = true;
			snap_opt.iterations = parse_u32("snap", a["snap"]);
			if (snap_opt.iterations > RNB_MESH_SNAP_MAX_ITERATIONS) throw ParseError("Argument 'snap' must be 0 .. 64");
		}
		for (const char* sub : {"snap-tolerance", "snap-max-step", "snap-max-displacement", "snap-only-fills", "snap-attributes"})
			if (a.count(sub) && !snap) throw ParseError(std::string("Argument '") + sub + "' is only used with --snap");
		if (a.count("snap-tolerance")) {
			snap_opt.tolerance = (float)parse_double("snap-tolerance", a["snap-tolerance"]);
			if (!(std::isfinite(snap_opt.tolerance) && snap_opt.tolerance >= 0.0f)) throw ParseError("Argument 'snap-tolerance' must be finite and at least 0");
		}
		if (a.count("snap-max-step")) {
			snap_opt.max_step = (float)parse_double("snap-max-step", a["snap-max-step"]);
			snap_step_given = true;
			if (!(std::isfinite(snap_opt.max_step) && snap_opt.max_step > 0.0f)) throw ParseError("Argument 'snap-max-step' must be finite and above 0");
		}
		if (a.count("snap-max-displacement")) {
			snap_opt.max_displacement = (float)parse_double("snap-max-displacement", a["snap-max-displacement"]);
			snap_leash_given = true;
			if (!(std::isfinite(snap_opt.max_displacement) && snap_opt.max_displacement >= 0.0f)) throw ParseError("Argument 'snap-max-displacement' must be finite and at least 0");
		}
		if (a.count("snap-only-fills")) {
			if (!fill_holes) throw ParseError("Argument 'snap-only-fills' is only used with --fill-holes");
			snap_only_fills = true;
		}
		if (a.count("snap-attributes")) {
			if (a["snap-attributes"] == "keep") snap_resample = false;
			else if (a["snap-attributes"] != "resample") throw ParseError("Argument 'snap-attributes' must be keep or resample");
		}
	} catch (const ParseError& e) {
		std::cerr << e.what() << std::endl;
		print_help(std::cerr, argv[0]);
		return 255;
	}
	const std::string scene = a["scene"], snap_path = a["snapshot"];
	if (!path_exists(snap_path)) { std::fprintf(stderr, "Snapshot path %s does not exist.\n", snap_path.c_str()); return 1; }
	if (!is_dir(scene)) { std::fprintf(stderr, "Scene path %s does not exist.\n", scene.c_str()); return 1; }

	rnb_ctx* ctx = nullptr;
	rnb_mesh dm, cm;
	rnb_mesh_texture dt;
	std::memset(&dm, 0, sizeof(dm));
	std::memset(&cm, 0, sizeof(cm));
	std::memset(&dt, 0, sizeof(dt));
	try {
		const Dataset ds = load_dataset(scene);
		const snapshot::Data sd = snapshot::read(snap_path);
		rnb_config cfg;
		RNB_CHECK(rnb_default_config(&cfg));
		snapshot::apply_network_config(sd.network_config, (float)ds.aabb_scale, cfg);
		const jsonmin::Value& hp = sd.network_config["hyperparams"];
		if (hp.contains("accumulate")) cfg.accumulate = hp["accumulate"].as_string() == "half" ? RNB_ACCUM_HALF : RNB_ACCUM_FP32;
		if (sd.has_aabb_scale) cfg.aabb_scale = sd.aabb_scale;
		RNB_CHECK(rnb_create(&cfg, &ctx));
		const uint64_t n = rnb_n_params(ctx);
		if (sd.params.size() != n) throw std::runtime_error("Can't set params because CPU buffer has the wrong size.");
		RNB_CHECK(rnb_set_params(ctx, sd.params.data())); // master = float(EMA half) and the EMA weights with it, as a resumed testbed run
		RNB_CHECK(rnb_set_training_step(ctx, sd.training_step)); // the hash-grid levels in use (grid.h:1430-1437)
		void* gp; uint64_t gnb;
		RNB_CHECK(rnb_buffer(ctx, RNB_BUF_DENSITY_GRID, &gp, &gnb));
		if (sd.grid.size() != gnb / 4) throw std::runtime_error("Incompatible number of grid cascades.");
		RNB_CHECK(rnb_memcpy(ctx, gp, sd.grid.data(), gnb, RNB_H2D));
		RNB_CHECK(rnb_update_density_bitfield(ctx, nullptr));

		// the testbed's lattice (compute_and_save_marching_cubes_mesh): next_multiple(res, 16) over the scene's box, threshold 0, EMA weights
		const uint32_t res = (resolution + 15u) / 16u * 16u;
		const float amin = 0.5f - 0.5f * (float)cfg.aabb_scale, amax = 0.5f + 0.5f * (float)cfg.aabb_scale;
		rnb_mesh_options mo;
		RNB_CHECK(rnb_mesh_default_options(&mo));
		for (int k = 0; k < 3; ++k) { mo.res[k] = res; mo.aabb_min[k] = amin; mo.aabb_max[k] = amax; }
		mo.lattice_min = amin; mo.lattice_max = amax;
		mo.thresh = 0.0f;
		mo.cull = cull;
		mo.brick = brick;
		mo.attributes = RNB_MESH_ATTR_COLORS | (gradient ? RNB_MESH_ATTR_NORMALS : 0u);
		rnb_mesh_stats st;
		RNB_CHECK(rnb_extract_mesh(ctx, nullptr, &mo, &dm, &st));
		rnb_mesh_clean_stats cs;
		const auto run_clean = [&]() { // device to device; the ring normals below are then those of the cleaned mesh
			rnb_mesh_clean_options co;
			RNB_CHECK(rnb_mesh_clean_default_options(&co));
			co.keep = keep; co.orient = orient;
			RNB_CHECK(rnb_mesh_clean(ctx, nullptr, &dm, &co, &cm, nullptr, &cs));
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		};
		const bool late_clean = repair || fill_holes || drop_classes;
		if (clean && !late_clean) run_clean(); // (with --repair, --drop-intersecting or --fill-holes: after them, below)
		std::string seen_report;
		if (want_seen) { // device to device, after the cleaning and before the simplification
			keep_seen(ctx, ds, dm, seen, &cm, seen_report);
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_simplify_stats ss;
		rnb_mesh_distance_stats es[2];
		double error_unit = 0.0;
		if (simplify) { // device to device, after the cleaning
			rnb_mesh_simplify_options so;
			RNB_CHECK(rnb_mesh_simplify_default_options(&so));
			for (int k = 0; k < 3; ++k) { so.origin[k] = amin; so.dims[k] = simplify; }
			so.cell = (float)(((double)amax - (double)amin) / (double)simplify);
			so.placement = placement;
			RNB_CHECK(rnb_mesh_simplify(ctx, nullptr, &dm, &so, &cm, &ss));
			if (report_error) { // before either mesh leaves the device: input -> output, output -> input
				rnb_mesh_distance_options dopt;
				RNB_CHECK(rnb_mesh_distance_default_options(&dopt));
				RNB_CHECK(rnb_mesh_distance(ctx, nullptr, &dm, &cm, &dopt, nullptr, nullptr, &es[0]));
				RNB_CHECK(rnb_mesh_distance(ctx, nullptr, &cm, &dm, &dopt, nullptr, nullptr, &es[1]));
				error_unit = (double)dopt.unit;
			}
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_repair_stats rs;
		if (repair) { // device to device, after the simplification; the cleaning, if asked for, on what it leaves
			RNB_CHECK(rnb_mesh_repair_default_options(&repair_opt));
			repair_opt.weld = a.count("weld") ? 1u : 0u;
			if (a.count("duplicates")) repair_opt.duplicates = a["duplicates"] == "keep" ? RNB_MESH_DUPLICATES_KEEP : (a["duplicates"] == "cancel" ? RNB_MESH_DUPLICATES_CANCEL : RNB_MESH_DUPLICATES_FIRST);
			if (a.count("orient-consistent")) repair_opt.orient = RNB_MESH_REPAIR_ORIENT_CONSISTENT;
			RNB_CHECK(rnb_mesh_repair(ctx, nullptr, &dm, &repair_opt, &cm, nullptr, &rs));
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_intersect_stats is;
		rnb_mesh_intersect_select_stats xs;
		if (drop_classes) { // device to device, after the repair and before the fill, which closes the rims this leaves
			rnb_mesh_intersect_options io;
			rnb_mesh_intersect_select_options xo;
			RNB_CHECK(rnb_mesh_intersect_default_options(&io));
			RNB_CHECK(rnb_mesh_intersections_select_default_options(&xo));
			xo.classes = drop_classes; xo.rings = drop_rings;
			const uint64_t nt = std::max<uint64_t>(dm.n_indices / 3u, 1);
			void *np = nullptr, *nc = nullptr;
			RNB_CHECK(rnb_device_malloc(ctx, nt * 4, &np));
			int rc = rnb_device_malloc(ctx, nt * 4, &nc);
			if (rc == RNB_OK) rc = rnb_mesh_intersections(ctx, nullptr, &dm, &io, (uint32_t*)np, (uint32_t*)nc, nullptr, 0, &is);
			if (rc == RNB_OK) rc = rnb_mesh_intersections_select(ctx, nullptr, &dm, (const uint32_t*)np, (const uint32_t*)nc, &xo, &cm, &xs);
			(void)rnb_device_free(ctx, np);
			if (nc) (void)rnb_device_free(ctx, nc);
			RNB_CHECK(rc);
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_fill_holes_stats fs;
		if (fill_holes) { // device to device, after the repair
			rnb_mesh_fill_holes_options fo;
			RNB_CHECK(rnb_mesh_fill_holes_default_options(&fo));
			fo.max_edges = fill_max_edges;
			fo.skip_largest = a.count("fill-skip-largest") ? 1u : 0u;
			RNB_CHECK(rnb_mesh_fill_holes(ctx, nullptr, &dm, &fo, &cm, nullptr, &fs));
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_smooth_stats ms;
		std::vector<float> smooth_moved;
		if (smooth) { // device to device, right after the fill: its appended vertices are still the last ones
			void* select = nullptr;
			if (smooth_only_fills && dm.n_verts) {
				std::vector<uint32_t> sel(dm.n_verts, 0u);
				for (uint32_t v = fs.n_verts_out - fs.n_verts_added; v < dm.n_verts; ++v) sel[v] = 1u;
				RNB_CHECK(rnb_device_malloc(ctx, (uint64_t)dm.n_verts * 4, &select));
				int rc = rnb_memcpy(ctx, select, sel.data(), (uint64_t)dm.n_verts * 4, RNB_H2D);
				if (rc != RNB_OK) { (void)rnb_device_free(ctx, select); RNB_CHECK(rc); }
			}
			void* moved = nullptr; // --snap-only-fills: how far the smoothing moved every vertex
			if (snap && snap_only_fills && dm.n_verts) {
				const int rc = rnb_device_malloc(ctx, (uint64_t)dm.n_verts * 4, &moved);
				if (rc != RNB_OK) { if (select) (void)rnb_device_free(ctx, select); RNB_CHECK(rc); }
			}
			int rc = rnb_mesh_smooth(ctx, nullptr, &dm, &smooth_opt, (const uint32_t*)select, &cm, nullptr, nullptr, (float*)moved, &ms);
			if (select) (void)rnb_device_free(ctx, select);
			if (moved) {
				smooth_moved.resize(dm.n_verts);
				if (rc == RNB_OK) rc = rnb_memcpy(ctx, smooth_moved.data(), moved, (uint64_t)dm.n_verts * 4, RNB_D2H);
				(void)rnb_device_free(ctx, moved);
			}
			RNB_CHECK(rc);
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		rnb_mesh_snap_stats sn;
		if (snap) { // device to device, right after the smoothing: the fill's appended vertices are still the last ones
			if (!snap_step_given) snap_opt.max_step = (float)cfg.aabb_scale / 128.0f;
			if (!snap_leash_given) snap_opt.max_displacement = (float)cfg.aabb_scale / 64.0f;
			snap_opt.level = mo.thresh;
			snap_opt.attributes = snap_resample ? mo.attributes : 0u;
			void* select = nullptr;
			if (snap_only_fills && dm.n_verts) {
				std::vector<uint32_t> sel(dm.n_verts, 0u);
				for (uint32_t v = fs.n_verts_out - fs.n_verts_added; v < dm.n_verts; ++v) sel[v] = 1u;
				for (size_t v = 0; v < smooth_moved.size() && v < sel.size(); ++v) if (smooth_moved[v] > 0.0f) sel[v] = 1u;
				RNB_CHECK(rnb_device_malloc(ctx, (uint64_t)dm.n_verts * 4, &select));
				int rc = rnb_memcpy(ctx, select, sel.data(), (uint64_t)dm.n_verts * 4, RNB_H2D);
				if (rc != RNB_OK) { (void)rnb_device_free(ctx, select); RNB_CHECK(rc); }
			}
			const int rc = rnb_mesh_snap(ctx, nullptr, &dm, &snap_opt, (const uint32_t*)select, &cm, nullptr, nullptr, nullptr, nullptr, &sn);
			if (select) (void)rnb_device_free(ctx, select);
			RNB_CHECK(rc);
			RNB_CHECK(rnb_mesh_free(ctx, &dm));
			dm = cm;
			std::memset(&cm, 0, sizeof(cm));
		}
		if (clean && late_clean) run_clean(); // on what the repair, the fill, the smoothing and the snap leave
		rnb_mesh_snap_stats rr;
		if (report_residual) { // of the mesh as it will be written: the census of a snap without a step
			rnb_mesh_snap_options ro;
			RNB_CHECK(rnb_mesh_snap_default_options(&ro));
			ro.iterations = 0; ro.level = mo.thresh;
			RNB_CHECK(rnb_mesh_snap(ctx, nullptr, &dm, &ro, nullptr, &cm, nullptr, nullptr, nullptr, nullptr, &rr));
			RNB_CHECK(rnb_mesh_free(ctx, &cm));
		}
		rnb_mesh_topology_stats tp;
		if (report_topology) { // of the mesh as it will be written
			rnb_mesh_topology_options to;
			RNB_CHECK(rnb_mesh_topology_default_options(&to));
			RNB_CHECK(rnb_mesh_topology(ctx, nullptr, &dm, &to, nullptr, nullptr, nullptr, nullptr, &tp));
		}
		rnb_mesh_intersect_stats ri;
		if (report_intersections) { // of the mesh as it will be written
			rnb_mesh_intersect_options io;
			RNB_CHECK(rnb_mesh_intersect_default_options(&io));
			RNB_CHECK(rnb_mesh_intersections(ctx, nullptr, &dm, &io, nullptr, nullptr, nullptr, 0, &ri));
		}
		// --report-views: made here, while the mesh is on the device and in the frame of the loaded views; printed and written after the mesh's own lines, below
		std::string views_report, views_json;
		if (want_views && !texture) report_views(ctx, ds, dm, nullptr, snap_path, views_report, views_json);
		// --texture: the mesh as it will be written, while it is on the device
		mesh::Texture tex;
		rnb_mesh_texture_stats ts;
		if (texture) {
			rnb_mesh_texture_options to;
			RNB_CHECK(rnb_mesh_texture_default_options(&to));
			to.size = texture; to.maps = texture_maps | (texture_from ? RNB_MESH_TEXTURE_ALBEDO : 0u); // the model's albedo is the projection's fallback
			RNB_CHECK(rnb_mesh_bake_texture(ctx, nullptr, &dm, &to, &dt, &ts));
			tex.size = dt.size;
			tex.uv.resize((size_t)dt.n_tris * 6);
			if (dt.n_tris) RNB_CHECK(rnb_memcpy(ctx, tex.uv.data(), dt.uv, (uint64_t)tex.uv.size() * 4, RNB_D2H));
			const uint64_t n_map = (uint64_t)dt.size * dt.size * 4;
			if (dt.albedo) { tex.albedo.resize(n_map); RNB_CHECK(rnb_memcpy(ctx, tex.albedo.data(), dt.albedo, n_map * 4, RNB_D2H)); }
			if (dt.normal) { tex.normal.resize(n_map); RNB_CHECK(rnb_memcpy(ctx, tex.normal.data(), dt.normal, n_map * 4, RNB_D2H)); }
			std::printf("texture: %u^2 texels, blocks of %u (%u per row) for %u triangles, %llu texels through the network in %u batches, peak workspace %.1f MB, %.1f ms\n", dt.size, dt.block,
			            dt.blocks_per_row, dt.n_tris, (unsigned long long)ts.n_texels, ts.n_batches, (double)ts.peak_workspace / 1e6, ts.ms);
			if (texture_from) { // the same atlas: the albedo map becomes the projection of the scene's albedo maps
				std::string line;
				project_views(ctx, ds, dm, dt, project, tex.albedo, line);
				std::fputs(line.c_str(), stdout);
			}
			if (want_views) { // the maps about to be written, drawn into every camera: the model's bake, or the projected colour (uploaded again: the projection was released)
				rnb_mesh_draw_texture vt;
				std::memset(&vt, 0, sizeof(vt));
				vt.uv_dev = dt.uv; vt.color_dev = dt.albedo; vt.normal_dev = dt.normal; vt.size = dt.size; vt.n_tris = dt.n_tris;
				if (texture_from && dt.albedo) RNB_CHECK(rnb_memcpy(ctx, dt.albedo, tex.albedo.data(), n_map * 4, RNB_H2D));
				report_views(ctx, ds, dm, (vt.color_dev || vt.normal_dev) ? &vt : nullptr, snap_path, views_report, views_json);
			}
			RNB_CHECK(rnb_mesh_texture_free(ctx, &dt));
		}
		mesh::Mesh m;
		m.verts.resize(dm.n_verts); m.colors.resize(dm.n_verts); m.indices.resize(dm.n_indices);
		if (dm.n_verts) {
			RNB_CHECK(rnb_memcpy(ctx, m.verts.data(), dm.verts, (uint64_t)dm.n_verts * 12, RNB_D2H));
			RNB_CHECK(rnb_memcpy(ctx, m.colors.data(), dm.colors, (uint64_t)dm.n_verts * 12, RNB_D2H));
		}
		if (dm.n_indices) RNB_CHECK(rnb_memcpy(ctx, m.indices.data(), dm.indices, (uint64_t)dm.n_indices * 4, RNB_D2H));
		if (gradient) {
			m.normals.resize(dm.n_verts);
			if (dm.n_verts) RNB_CHECK(rnb_memcpy(ctx, m.normals.data(), dm.normals, (uint64_t)dm.n_verts * 12, RNB_D2H));
		} else mesh::compute_normals(m);
		RNB_CHECK(rnb_mesh_free(ctx, &dm));
		std::printf("%u^3: %llu of %llu bricks kept, %llu evaluated (%.1f %% of the lattice), %llu with a sign change, peak workspace %.1f MB, %.1f ms\n", res,
		            (unsigned long long)st.n_kept, (unsigned long long)st.n_bricks, (unsigned long long)st.n_evaluated,
		            100.0 * (double)st.n_points_evaluated / ((double)res * res * res), (unsigned long long)st.n_sign_change, (double)st.peak_workspace / 1e6, st.ms);
		if (clean && !late_clean) std::printf("clean: %u components found, %u kept, %u -> %u triangles, %u -> %u vertices, %.1f ms\n", cs.n_components, cs.n_kept, cs.n_tris_in, cs.n_tris_out,
		                       cs.n_verts_in, cs.n_verts_out, cs.ms);
		if (want_seen) std::fputs(seen_report.c_str(), stdout);
		if (simplify) std::printf("simplify: %u clusters, %u -> %u triangles (%u collapsed), %u -> %u vertices, %u clamped, %u at the mean, %.1f ms\n", ss.n_clusters, ss.n_tris_in,
		                          ss.n_tris_out, ss.n_tris_collapsed, ss.n_verts_in, ss.n_verts_out, ss.n_clamped, ss.n_fallback, ss.ms);
		if (repair) std::printf("repair: %u welded, %u degenerate and %u duplicate triangles dropped, %u flipped, %u patches of which %u unorientable, %u -> %u triangles, %u -> %u vertices, %.1f ms\n",
		                        rs.n_welded, rs.n_degenerate_dropped, rs.n_duplicates_dropped, rs.n_flipped, rs.n_patches, rs.n_unorientable_patches, rs.n_tris_in, rs.n_tris_out, rs.n_verts_in,
		                        rs.n_verts_out, rs.ms);
		if (drop_classes)
			std::printf("drop intersecting: %llu proper and %llu contact pairs among %llu candidates, %u triangles selected, %u -> %u triangles, %u -> %u vertices, %.1f + %.1f ms\n",
			            (unsigned long long)is.n_pairs_proper, (unsigned long long)is.n_pairs_contact, (unsigned long long)is.n_candidates, xs.n_selected, xs.n_tris_in, xs.n_tris_out, xs.n_verts_in,
			            xs.n_verts_out, is.ms, xs.ms);
		if (fill_holes) std::printf("fill: %u loops, %u filled, %u not simple, %u over the limit, %u largest left open, %u vertices and %u triangles added, %u -> %u triangles, %.1f ms\n", fs.n_loops,
		                            fs.n_filled, fs.n_skipped_not_simple, fs.n_skipped_over_max, fs.n_skipped_largest, fs.n_verts_added, fs.n_tris_added, fs.n_tris_out - fs.n_tris_added,
		                            fs.n_tris_out, fs.ms);
		if (smooth) std::printf("smooth: %u passes, %u of %u vertices moving (%u selected; %u interior, %u boundary, %u non-manifold, %u unused), %u edges, valence up to %u, %u on the wide path, "
		                        "greatest displacement %.9g, %.1f ms of which %.1f in the passes\n", ms.passes, ms.n_moving, ms.n_interior + ms.n_boundary + ms.n_nonmanifold + ms.n_unused,
		                        ms.n_selected, ms.n_interior, ms.n_boundary, ms.n_nonmanifold, ms.n_unused, ms.n_edges, ms.max_valence, ms.n_wide, ms.max_displacement, ms.ms, ms.ms_passes);
		if (snap) std::printf("snap: %u iterations, %u of %u vertices selected, %u moved; %u converged, %u unfinished, %u flat, %u leashed, %u outside, %u stalled, %u invalid, %u reverted; "
		                      "mean |sdf| %.9g -> %.9g, max %.9g -> %.9g, greatest displacement %.9g, %u rounds, %llu points through the network, %.1f ms of which %.1f in the network\n",
		                      snap_opt.iterations, sn.n_selected, sn.n_selected + sn.n_unselected, sn.n_moved, sn.n_converged, sn.n_unfinished, sn.n_flat, sn.n_leashed, sn.n_outside, sn.n_stalled,
		                      sn.n_invalid, sn.n_reverted, residual_mean(sn.sum_before_q, sn.n_selected - sn.n_invalid), residual_mean(sn.sum_after_q, sn.n_selected - sn.n_invalid), sn.max_before,
		                      sn.max_after, sn.max_displacement, sn.rounds, (unsigned long long)sn.n_network_points, sn.ms, sn.ms_network);
		if (clean && late_clean) std::printf("clean: %u components found, %u kept, %u -> %u triangles, %u -> %u vertices, %.1f ms\n", cs.n_components, cs.n_kept, cs.n_tris_in, cs.n_tris_out,
		                                 cs.n_verts_in, cs.n_verts_out, cs.ms);
		if (report_topology)
			std::printf("{\"topology\": {\"n_verts_used\": %u, \"n_tris\": %u, \"n_degenerate\": %u, \"n_edges\": %u, \"n_boundary_edges\": %u, \"n_manifold_edges\": %u, \"n_nonmanifold_edges\": %u, "
			            "\"n_inconsistent_edges\": %u, \"max_faces_on_edge\": %u, \"n_duplicate_tris\": %u, \"n_folded_pairs\": %u, \"n_components\": %u, \"n_patches\": %u, "
			            "\"n_unorientable_patches\": %u, \"n_boundary_components\": %u, \"closed\": %u, \"oriented\": %u, \"euler\": %lld}}\n",
			            tp.n_verts_used, tp.n_tris, tp.n_degenerate, tp.n_edges, tp.n_boundary_edges, tp.n_manifold_edges, tp.n_nonmanifold_edges, tp.n_inconsistent_edges, tp.max_faces_on_edge,
			            tp.n_duplicate_tris, tp.n_folded_pairs, tp.n_components, tp.n_patches, tp.n_unorientable_patches, tp.n_boundary_components, tp.closed, tp.oriented, (long long)tp.euler);
		if (report_residual)
			std::printf("{\"residual\": {\"n_verts\": %u, \"n_invalid\": %u, \"mean\": %.9g, \"max\": %.9g, \"ms\": %.3f}}\n", rr.n_selected, rr.n_invalid,
			            residual_mean(rr.sum_before_q, rr.n_selected - rr.n_invalid), rr.max_before, rr.ms);
		if (report_intersections)
			std::printf("{\"intersections\": {\"n_tris\": %u, \"n_degenerate\": %u, \"n_same_set\": %llu, \"n_candidates\": %llu, \"n_pairs_proper\": %llu, \"n_pairs_contact\": %llu, "
			            "\"n_tris_proper\": %u, \"n_tris_contact\": %u, \"n_coplanar_pairs\": %llu, \"dims\": [%u, %u, %u], \"n_large\": %u, \"n_cell_entries\": %llu, \"n_visited\": %llu, "
			            "\"ms\": %.3f}}\n",
			            ri.n_tris, ri.n_degenerate, (unsigned long long)ri.n_same_set, (unsigned long long)ri.n_candidates, (unsigned long long)ri.n_pairs_proper, (unsigned long long)ri.n_pairs_contact,
			            ri.n_tris_proper, ri.n_tris_contact, (unsigned long long)ri.n_coplanar_pairs, ri.dims[0], ri.dims[1], ri.dims[2], ri.n_large, (unsigned long long)ri.n_cell_entries,
			            (unsigned long long)ri.n_visited, ri.ms);
		if (report_error) {
			double mean[2], rms[2];
			for (int k = 0; k < 2; ++k) {
				mean[k] = es[k].sum_w ? (double)es[k].sum_wd / (double)es[k].sum_w * error_unit : 0.0;
				rms[k] = es[k].sum_w ? std::sqrt((double)es[k].sum_wd2 / (double)es[k].sum_w) * error_unit : 0.0;
			}
			std::printf("simplify error: in -> out mean %.9g rms %.9g max %.9g, out -> in mean %.9g rms %.9g max %.9g, %.1f ms\n", mean[0], rms[0], es[0].max_distance, mean[1], rms[1],
			            es[1].max_distance, es[0].ms + es[1].ms);
		}
		if (want_views) {
			std::fputs(views_report.c_str(), stdout);
			const std::string path = a.count("views-out") ? a["views-out"] : a["out"] + ".views.json";
			std::FILE* f = std::fopen(path.c_str(), "wb");
			if (!f) throw std::runtime_error("cannot write " + path);
			std::fputs(views_json.c_str(), f);
			std::fclose(f);
		}
		std::printf("#vertices=%zu #triangles=%zu\n", m.verts.size(), m.indices.size() / 3);
		// --orient outward speaks of the file: the device turned every kept component counter-clockwise seen from outside, and the faces are written as they are
		// (without it, the scene's from_na flag decides whether save_obj reverses them, as in the testbed). save_obj maps positions by a uniform scale and a shift,
		// which keeps the winding as long as the scales are positive (scale > 0 and n2w_s > 0, as every scene the loader accepts has them).
		const bool as_they_are = (clean && orient == RNB_MESH_ORIENT_OUTWARD) ? true : ds.from_na;
		if (texture) mesh::save_obj_textured(a["out"], m, tex, png16::save, ds.scale, ds.offset, ds.n2w_s, ds.n2w_t, as_they_are);
		else mesh::save_obj(a["out"], m, ds.scale, ds.offset, ds.n2w_s, ds.n2w_t, as_they_are);
		rnb_destroy(ctx);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "Uncaught exception: %s\n", e.what());
		if (ctx) { rnb_mesh_free(ctx, &dm); rnb_mesh_free(ctx, &cm); rnb_mesh_texture_free(ctx, &dt); rnb_destroy(ctx); }
		return 1;
	}
	return 0;
}
