// render_main.cpp — `./build/render`: the maps a trained snapshot predicts for the cameras of a scene (Testbed::render_nerf in its Normals / Depth modes,
// src/testbed_nerf.cu:2499-2770, without the GUI), over include/rnb_render.h. The scene is read by the testbed's loader (dataset.hpp: the cameras are
// the training step's, bit for bit) and the snapshot by snapshot.hpp (its EMA weights, occupancy grid and network configuration).
//
//   render --snapshot PATH --scene DIR [--out DIR] [--views 0,5,9] [--downscale N] [--min-transmittance F]
//
// Per view under --out (default <scene>/output/render): normals/NNNNN.png and albedos/NNNNN.png (RGBA16 in the scenes' own encoding, alpha = the rendered
// mask: the directory reads back like an input scene's maps), depth/NNNNN.npy (float32 [H, W], scene units, camera-forward), and render_metrics.json: per view
// the mean and median angle (degrees) between rendered and input normals where both masks hold, the IoU of the two masks, the frame time; their means.
// Exit codes as the testbed's: 0, 255 on a command-line error, 1 on a missing path or a failure.
#include "../../include/rnb_neus2.h"
#include "../../include/rnb_render.h"
#include "dataset.hpp"
#include "json_min.hpp"
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
	{"scene", "DIR", "The scene the snapshot was trained on: its cameras, and the input normal maps the metrics compare with."},
	{"out", "DIR", "Output directory (default <scene>/output/render)."},
	{"views", "LIST", "Comma-separated view indices (default: every view)."},
	{"downscale", "N", "Render at 1/N of each view's resolution (focal length scaled, principal point kept). Default 1."},
	{"min-transmittance", "F", "A ray stops once its opacity exceeds 1 - F (default 0.01; 0 = composite to the box exit)."},
};

struct ParseError : std::runtime_error { using std::runtime_error::runtime_error; };

void print_help(std::ostream& os, const char* prog) {
	os << "  " << prog << " {OPTIONS}\n\n    normal, albedo and depth maps of a trained snapshot\n\n  OPTIONS:\n\n      -h, --help\n                                        Display this help menu.\n";
	for (const auto& f : FLAGS) os << "      --" << f.name << "=[" << f.meta << "]\n                                        " << f.help << "\n";
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
		bool known = false;
		for (const auto& f : FLAGS) known = known || name == f.name;
		if (!known) throw ParseError("Flag could not be matched: " + name);
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

#define RNB_CHECK(expr)                                                                          \
	do {                                                                                         \
		int rc_ = (expr);                                                                        \
		if (rc_ != RNB_OK) throw std::runtime_error(std::string(#expr) + ": " + rnb_last_error()); \
	} while (0)

void save_npy(const std::string& path, const float* data, uint32_t h, uint32_t w) { // NPY format 1.0, little-endian float32, C order
	char shape[96];
	std::snprintf(shape, sizeof(shape), "{'descr': '<f4', 'fortran_order': False, 'shape': (%u, %u), }", h, w);
	std::string header = shape;
	while ((10 + header.size() + 1) % 64 != 0) header += ' ';
	header += '\n';
	std::FILE* f = std::fopen(path.c_str(), "wb");
	if (!f) throw std::runtime_error("cannot write " + path);
	const uint16_t hl = (uint16_t)header.size();
	std::fwrite("\x93NUMPY\x01\x00", 1, 8, f);
	std::fwrite(&hl, 2, 1, f);
	std::fwrite(header.data(), 1, header.size(), f);
	std::fwrite(data, 4, (size_t)h * w, f);
	std::fclose(f);
}

uint16_t to_u16(float v) { return (uint16_t)std::lround(std::min(std::max(v, 0.0f), 1.0f) * 65535.0f); }

using view_metrics::num;

} // namespace

int main(int argc, char** argv) {
	std::map<std::string, std::string> a;
	uint32_t downscale = 1;
	float min_t = 0.01f;
	try {
		bool help = false;
		a = parse_cli(argc, argv, help);
		if (help) { print_help(std::cout, argv[0]); return 0; }
		if (!a.count("snapshot") || !a.count("scene")) throw ParseError("--snapshot and --scene are required");
		if (a.count("downscale")) downscale = parse_u32("downscale", a["downscale"]);
		if (downscale == 0) throw ParseError("Argument 'downscale' must be at least 1");
		if (a.count("min-transmittance")) {
			char* e = nullptr;
			min_t = std::strtof(a["min-transmittance"].c_str(), &e);
			if (a["min-transmittance"].empty() || *e) throw ParseError("Argument 'min-transmittance' received invalid value type '" + a["min-transmittance"] + "'");
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
	float* img_dev = nullptr;
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

		std::vector<uint32_t> sel;
		if (a.count("views")) {
			std::string s = a["views"];
			size_t p = 0;
			while (p <= s.size()) {
				const size_t q = std::min(s.find(',', p), s.size());
				const uint32_t v = parse_u32("views", s.substr(p, q - p));
				if (v >= ds.views.size()) throw std::runtime_error("view " + std::to_string(v) + " out of range (the scene has " + std::to_string(ds.views.size()) + ")");
				sel.push_back(v);
				p = q + 1;
			}
		} else for (uint32_t i = 0; i < ds.views.size(); ++i) sel.push_back(i);

		const std::string out = a.count("out") ? a["out"] : scene + "/output/render";
		make_dir(scene + "/output");
		make_dir(out);
		make_dir(out + "/normals"); make_dir(out + "/albedos"); make_dir(out + "/depth");
		rnb_render_options ro;
		RNB_CHECK(rnb_render_default_options(&ro));
		ro.min_transmittance = min_t;
		std::string views_json;
		double s_mean = 0, s_median = 0, s_iou = 0, s_ms = 0;
		size_t cap = 0;
		for (const uint32_t vi : sel) {
			rnb_view v = ds.views[vi];
			const png16::Image& in = ds.normals[vi];
			v.width = std::max(1u, in.width / downscale); v.height = std::max(1u, in.height / downscale);
			v.focal_length[0] *= (float)v.width / (float)in.width; v.focal_length[1] *= (float)v.height / (float)in.height;
			const size_t np = (size_t)v.width * v.height;
			if (np * RNB_RENDER_CHANNELS > cap) {
				if (img_dev) RNB_CHECK(rnb_device_free(ctx, img_dev));
				img_dev = nullptr;
				cap = np * RNB_RENDER_CHANNELS;
				RNB_CHECK(rnb_device_malloc(ctx, cap * 4, (void**)&img_dev));
			}
			rnb_render_stats st;
			RNB_CHECK(rnb_render(ctx, nullptr, &v, &ro, img_dev, &st));
			std::vector<float> img(np * RNB_RENDER_CHANNELS);
			RNB_CHECK(rnb_memcpy(ctx, img.data(), img_dev, img.size() * 4, RNB_D2H));
			std::vector<uint16_t> nrm(np * 4), alb(np * 4);
			std::vector<float> depth(np);
			view_metrics::Accumulator acc(v.width, v.height, in.rgba.data(), in.width, in.height); // the comparison with the input map: view_metrics.hpp
			for (size_t p = 0; p < np; ++p) {
				const float* c = img.data() + p * RNB_RENDER_CHANNELS;
				const bool mask = c[6] > 0.5f;
				// the camera-frame normal R^T n, stored as (x, -y, -z) in [0, 1] (synthetic.render_view's and the loss's encoding, ray_targets)
				float nc[3];
				view_metrics::camera_normal(v.xform, c, nc);
				const float m[3] = {nc[0], -nc[1], -nc[2]};
				for (int k = 0; k < 3; ++k) nrm[p * 4 + k] = mask ? to_u16((m[k] + 1.0f) * 0.5f) : 0;
				nrm[p * 4 + 3] = mask ? 65535 : 0;
				for (int k = 0; k < 3; ++k) alb[p * 4 + k] = to_u16(c[3 + k]);
				alb[p * 4 + 3] = mask ? 65535 : 0;
				depth[p] = c[7];
				acc.add(p, mask, nc);
			}
			char name[32];
			std::snprintf(name, sizeof(name), "%05u", vi);
			png16::save(out + "/normals/" + name + ".png", nrm.data(), v.width, v.height, 4, 16);
			png16::save(out + "/albedos/" + name + ".png", alb.data(), v.width, v.height, 4, 16);
			save_npy(out + "/depth/" + name + ".npy", depth.data(), v.height, v.width);
			const view_metrics::Result vm = acc.finish();
			const double mean = vm.mean_angle_deg, median = vm.median_angle_deg, iou = vm.mask_iou;
			s_mean += mean; s_median += median; s_iou += iou; s_ms += st.ms;
			std::printf("view %u: %ux%u, normal angle mean %.3f median %.3f deg, mask IoU %.4f, %.2f ms\n", vi, v.width, v.height, mean, median, iou, st.ms);
			if (!views_json.empty()) views_json += ",\n";
			views_json += "    {\"view\": " + std::to_string(vi) + ", \"width\": " + std::to_string(v.width) + ", \"height\": " + std::to_string(v.height) +
			              ", " + view_metrics::json_fields(vm) + ", \"frame_ms\": " + num(st.ms) + "}";
		}
		const double k = sel.empty() ? 1.0 : (double)sel.size();
		std::FILE* f = std::fopen((out + "/render_metrics.json").c_str(), "wb");
		if (!f) throw std::runtime_error("cannot write " + out + "/render_metrics.json");
		std::fprintf(f, "{\n  \"snapshot\": \"%s\",\n  \"downscale\": %u,\n  \"min_transmittance\": %s,\n  \"views\": [\n%s\n  ],\n  \"mean\": {\"mean_angle_deg\": %s, \"median_angle_deg\": %s, \"mask_iou\": %s, \"frame_ms\": %s}\n}\n",
		             snap_path.c_str(), downscale, num(min_t).c_str(), views_json.c_str(), num(s_mean / k).c_str(), num(s_median / k).c_str(), num(s_iou / k).c_str(), num(s_ms / k).c_str());
		std::fclose(f);
		if (img_dev) rnb_device_free(ctx, img_dev);
		rnb_destroy(ctx);
	} catch (const std::exception& e) {
		std::fprintf(stderr, "Uncaught exception: %s\n", e.what());
		if (ctx) { if (img_dev) rnb_device_free(ctx, img_dev); rnb_destroy(ctx); }
		return 1;
	}
	return 0;
}
