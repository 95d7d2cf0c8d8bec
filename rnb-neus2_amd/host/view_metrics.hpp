// view_metrics.hpp — how an image in the channel layout of rnb_render (world-frame normal in channels 0-2, opacity or coverage in channel 6) is compared with a scene's
// input normal map: the one definition behind render_metrics.json (build/render, the model's render) and <out>.views.json (build/mesh --report-views, the mesh's
// rasterisation), and what rnb_neus2_amd.api.view_normal_metrics repeats in numpy.
//   mask         channel 6 > 0.5
//   input mask   alpha > 0, at the input pixel whose area holds this pixel's centre
//   angle        between the image's normal taken to the camera frame (R^T n, float) and the input's decoded one ((x, -y, -z) stored in [0, 1]), in degrees, where both
//                masks hold and both normals are non-zero; mean (summed in pixel order) and median (the mean of the middle two for an even number) over those pixels
//   IoU          of the two masks; 1 if both are empty
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace view_metrics {

struct Result {
	double mean_angle_deg = 0, median_angle_deg = 0, mask_iou = 1;
	size_t pixels_compared = 0;
};

// a number of the JSON reports: six significant digits, 0 for what is not finite
inline std::string num(double v) {
	char b[64];
	std::snprintf(b, sizeof(b), "%.6g", std::isfinite(v) ? v : 0.0);
	return b;
}

// The camera-frame normal R^T n of a pixel's channels 0-2 (xform: camera-to-world 3x4, row-major).
inline void camera_normal(const float xform[12], const float* c, float nc[3]) {
	for (int k = 0; k < 3; ++k) nc[k] = xform[0 * 4 + k] * c[0] + xform[1 * 4 + k] * c[1] + xform[2 * 4 + k] * c[2];
}

// One view's comparison, pixel by pixel in row-major order.
struct Accumulator {
	uint32_t width, height, in_width, in_height;
	const uint16_t* in_rgba; // [in_height][in_width][4]
	std::vector<double> angles;
	uint64_t inter = 0, uni = 0;
	Accumulator(uint32_t w, uint32_t h, const uint16_t* rgba, uint32_t in_w, uint32_t in_h) : width(w), height(h), in_width(in_w), in_height(in_h), in_rgba(rgba) {}

	// pixel p of the image: its mask and its camera-frame normal
	void add(size_t p, bool mask, const float nc[3]) {
		// the input pixel whose area holds this pixel's centre
		const uint32_t x = (uint32_t)(p % width), y = (uint32_t)(p / width);
		const uint32_t ix = std::min(in_width - 1, (uint32_t)(((double)x + 0.5) * in_width / width));
		const uint32_t iy = std::min(in_height - 1, (uint32_t)(((double)y + 0.5) * in_height / height));
		const uint16_t* t = in_rgba + ((size_t)iy * in_width + ix) * 4;
		const bool mask_in = t[3] > 0;
		inter += (mask && mask_in); uni += (mask || mask_in);
		if (mask && mask_in) {
			double ti[3] = {t[0] / 65535.0 * 2.0 - 1.0, -(t[1] / 65535.0 * 2.0 - 1.0), -(t[2] / 65535.0 * 2.0 - 1.0)};
			const double ln = std::sqrt(ti[0] * ti[0] + ti[1] * ti[1] + ti[2] * ti[2]), lr = std::sqrt((double)nc[0] * nc[0] + (double)nc[1] * nc[1] + (double)nc[2] * nc[2]);
			if (ln > 0 && lr > 0) {
				const double cs = (ti[0] * nc[0] + ti[1] * nc[1] + ti[2] * nc[2]) / (ln * lr);
				angles.push_back(std::acos(std::min(1.0, std::max(-1.0, cs))) * 180.0 / M_PI);
			}
		}
	}

	Result finish() {
		Result r;
		r.pixels_compared = angles.size();
		if (!angles.empty()) {
			double mean = 0;
			for (double x : angles) mean += x;
			r.mean_angle_deg = mean / angles.size();
			std::sort(angles.begin(), angles.end());
			const size_t k = angles.size();
			r.median_angle_deg = k % 2 ? angles[k / 2] : 0.5 * (angles[k / 2 - 1] + angles[k / 2]);
		}
		r.mask_iou = uni ? (double)inter / (double)uni : 1.0;
		return r;
	}
};

// A whole image [height][width][channels] (channels >= 7) against an input normal map.
inline Result compare(const float* img, uint32_t channels, uint32_t width, uint32_t height, const float xform[12], const uint16_t* in_rgba, uint32_t in_width, uint32_t in_height) {
	Accumulator acc(width, height, in_rgba, in_width, in_height);
	const size_t np = (size_t)width * height;
	for (size_t p = 0; p < np; ++p) {
		const float* c = img + p * channels;
		float nc[3];
		camera_normal(xform, c, nc);
		acc.add(p, c[6] > 0.5f, nc);
	}
	return acc.finish();
}

// A number of the JSON reports with every digit a double has (what is compared with the Python side's sums, not read by eye). What is not finite is written as
// null: albedo_psnr_db of a view whose drawn colours equal the input's is infinite (mse 0), and so is a mean over views that holds such a view -- the Python side returns
// inf for both. null never stands for a bad result; a reader takes it as "no error to measure".
inline std::string num_full(double v) {
	if (!std::isfinite(v)) return "null";
	char b[64];
	std::snprintf(b, sizeof(b), "%.17g", v);
	return b;
}

// One view's comparison of the image's colour (channels 3-5) with a scene's input albedo map (uint16 RGBA, read as x / 65535; alpha = mask), and what
// rnb_neus2_amd.api.view_albedo_metrics repeats in numpy: the masks and the input pixel of Accumulator::add; over the pixels where both masks hold, in row-major order,
// e = image - input per channel, the sums of (|e_0| + |e_1|) + |e_2| and of (e_0^2 + e_1^2) + e_2^2; mae = the first / 3n, mse = the second / 3n, rmse = sqrt(mse),
// psnr_db = 10 log10(1 / mse) (infinite for mse 0: num_full writes null); all zeros when n is 0.
struct AlbedoResult {
	double mae = 0, rmse = 0, psnr_db = 0;
	size_t pixels_compared = 0;
};
inline AlbedoResult compare_albedo(const float* img, uint32_t channels, uint32_t width, uint32_t height, const uint16_t* in_rgba, uint32_t in_width, uint32_t in_height) {
	AlbedoResult r;
	double sum_abs = 0, sum_sq = 0;
	for (uint32_t y = 0; y < height; ++y)
		for (uint32_t x = 0; x < width; ++x) {
			const float* c = img + ((size_t)y * width + x) * channels;
			const uint32_t ix = std::min(in_width - 1, (uint32_t)(((double)x + 0.5) * in_width / width));
			const uint32_t iy = std::min(in_height - 1, (uint32_t)(((double)y + 0.5) * in_height / height));
			const uint16_t* t = in_rgba + ((size_t)iy * in_width + ix) * 4;
			if (!(c[6] > 0.5f) || !(t[3] > 0)) continue;
			const double e0 = (double)c[3] - t[0] / 65535.0, e1 = (double)c[4] - t[1] / 65535.0, e2 = (double)c[5] - t[2] / 65535.0;
			sum_abs += (std::fabs(e0) + std::fabs(e1)) + std::fabs(e2);
			sum_sq += (e0 * e0 + e1 * e1) + e2 * e2;
			++r.pixels_compared;
		}
	if (r.pixels_compared) {
		const double n3 = 3.0 * (double)r.pixels_compared, mse = sum_sq / n3;
		r.mae = sum_abs / n3;
		r.rmse = std::sqrt(mse);
		r.psnr_db = 10.0 * std::log10(1.0 / mse);
	}
	return r;
}

// The fields a view's entry of the JSON reports share: "mean_angle_deg": ..., "median_angle_deg": ..., "mask_iou": ..., "pixels_compared": ...
inline std::string json_fields(const Result& r) {
	return "\"mean_angle_deg\": " + num(r.mean_angle_deg) + ", \"median_angle_deg\": " + num(r.median_angle_deg) + ", \"mask_iou\": " + num(r.mask_iou) +
	       ", \"pixels_compared\": " + std::to_string(r.pixels_compared);
}

} // namespace view_metrics
