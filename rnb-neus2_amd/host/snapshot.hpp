// snapshot.hpp — reading a training snapshot (Testbed::load_snapshot, src/testbed.cu:3333-3390; tiny-cuda-nn/trainer.h:263-305) and turning its network
// configuration into an rnb_config (Testbed::reset_network, src/testbed.cu:2245-2335). Shared by build/testbed and build/render. Host code only: it calls no
// library function, so the CPU-checker build of testbed_main.cpp (tests/) compiles it as is.
#pragma once
#include "../../include/rnb_neus2.h"
#include "json_min.hpp"
#include "msgpack_min.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace snapshot {

// The parsed network configuration travels inside the snapshot (m_network_config, src/testbed.cu:3282-3313): JSON <-> MessagePack values.
inline mpk::Value json_to_mpk(const jsonmin::Value& j) {
	switch (j.type) {
		case jsonmin::Value::Null: return mpk::Value();
		case jsonmin::Value::Bool: return mpk::Value::boolean(j.b);
		case jsonmin::Value::Number:
			if (j.num >= 0 && j.num == std::floor(j.num) && j.num < 1.8e19) return mpk::Value::uint((uint64_t)j.num);
			return mpk::Value::real(j.num);
		case jsonmin::Value::String: return mpk::Value::str(j.str);
		case jsonmin::Value::Arr: { mpk::Value a = mpk::Value::array(); for (const auto& e : *j.arr) a.arr.push_back(json_to_mpk(e)); return a; }
		default: { mpk::Value o = mpk::Value::object(); for (const auto& kv : *j.obj) o.set(kv.first, json_to_mpk(kv.second)); return o; }
	}
}
inline jsonmin::Value mpk_to_json(const mpk::Value& m) {
	jsonmin::Value j;
	switch (m.type) {
		case mpk::Value::Nil: case mpk::Value::Bin: break;
		case mpk::Value::Bool: j.type = jsonmin::Value::Bool; j.b = m.b; break;
		case mpk::Value::Int: case mpk::Value::UInt: case mpk::Value::Float: j.type = jsonmin::Value::Number; j.num = m.number(); break;
		case mpk::Value::Str: j.type = jsonmin::Value::String; j.str = m.s; break;
		case mpk::Value::Arr: j.type = jsonmin::Value::Arr; j.arr = std::make_shared<jsonmin::Array>(); for (const auto& e : m.arr) j.arr->push_back(mpk_to_json(e)); break;
		default: j.type = jsonmin::Value::Obj; j.obj = std::make_shared<jsonmin::Object>(); for (const auto& kv : m.map) (*j.obj)[kv.first] = mpk_to_json(kv.second); break;
	}
	return j;
}

// What of a network config this build cannot honour is refused by name instead of being ignored. The architecture of the path is the reference's base.json
// (nerf_network.h:40-83): density MLP 32 -> 64 -> 16, colour MLP 48 -> 64 -> 64 -> 16, two features per level.
inline void check_supported(const jsonmin::Value& c) {
	auto need = [](const jsonmin::Value& blk, const char* block, const char* key, double want) {
		if (!blk.contains(key) || blk[key].is_null()) return;
		const double v = blk[key].as_number();
		if (v != want) throw std::runtime_error(std::string("network config: ") + block + "." + key + " = " + std::to_string(v) + " is not supported by this build (fixed at " + std::to_string(want) + ")");
	};
	auto need_str = [](const jsonmin::Value& blk, const char* block, const char* key, const char* want) {
		if (!blk.contains(key) || blk[key].is_null()) return;
		if (blk[key].as_string() != want) throw std::runtime_error(std::string("network config: ") + block + "." + key + " = \"" + blk[key].as_string() + "\" is not supported by this build (fixed at \"" + want + "\")");
	};
	const auto& enc = c["encoding"];
	need(enc, "encoding", "n_features_per_level", 2);
	const uint32_t L = enc.value("n_levels", 16u);
	// NerfNetwork pads the density network's input [x y z | 2 L features] to a multiple of 16 and picks the geometric initialisation by that width
	// (load_sdf_mlp_weight, nerf_network.h:585-604): 32 -> utils/mlp_weights_hidden_layer_num_1_hidden_size_32.txt, 48 -> utils/mlp_weights.txt
	if (3 + 2 * L > 32) throw std::runtime_error("network config: encoding.n_levels = " + std::to_string(L) + " gives a density-network input of width " + std::to_string((3 + 2 * L + 15) / 16 * 16) +
	                                             " (the reference's utils/mlp_weights.txt case, nerf_network.h:595-600); this build supports width 32 only (n_levels <= 14)");
	for (const char* blk : {"network", "rgb_network"}) {
		need(c[blk], blk, "n_neurons", 64);
		need(c[blk], blk, "n_hidden_layers", std::string(blk) == "network" ? 1 : 2);
		need_str(c[blk], blk, "activation", "ReLU");
		need_str(c[blk], blk, "output_activation", "None");
	}
	need_str(c["optimizer"], "optimizer", "otype", "Ema");
}

inline void apply_network_config(const jsonmin::Value& c, float dataset_aabb_scale, rnb_config& cfg) { // Testbed::reset_network, src/testbed.cu:2245-2335
	check_supported(c);
	const auto& enc = c["encoding"];
	cfg.n_levels = enc.value("n_levels", 16u);
	cfg.log2_hashmap_size = enc.value("log2_hashmap_size", 15u);
	cfg.base_resolution = enc.value("base_resolution", 0u);
	if (!cfg.base_resolution) cfg.base_resolution = 1u << (cfg.log2_hashmap_size / 3);
	const float desired_resolution = enc.value("top_resolution", 2048.0f);
	float pls = enc.value("per_level_scale", 0.0f);
	if (pls <= 0.0f && cfg.n_levels > 1) pls = std::exp(std::log(desired_resolution * dataset_aabb_scale / (float)cfg.base_resolution) / (cfg.n_levels - 1));
	cfg.per_level_scale = pls;
	cfg.valid_level_scale = enc.value("valid_level_scale", 0.01f);
	cfg.base_valid_level_scale = enc.value("base_valid_level_scale", 0.5f);
	cfg.base_training_step = enc.value("base_training_step", 200u);
	cfg.sdf_bias = c["network"].value("sdf_bias", -0.1f);
	const auto& hp = c["hyperparams"];
	cfg.target_batch_size = hp.value("batch_size", 1u << 18);
	cfg.mask_loss_weight = hp.value("mask_loss_weight", 0.f);
	cfg.ek_loss_weight = hp.value("ek_loss_weight", 0.01f);
	const jsonmin::Value* opt = &c["optimizer"]; // Ema -> ExponentialDecay -> Adam
	if (opt->contains("decay")) cfg.ema_decay = (*opt)["decay"].as_float();
	if (opt->contains("nested")) {
		opt = &(*opt)["nested"];
		cfg.lr_decay_start = opt->value("decay_start", cfg.lr_decay_start);
		cfg.lr_decay_interval = opt->value("decay_interval", cfg.lr_decay_interval);
		cfg.lr_decay_base = opt->value("decay_base", cfg.lr_decay_base);
		if (opt->contains("nested")) {
			opt = &(*opt)["nested"];
			cfg.learning_rate = opt->value("learning_rate", cfg.learning_rate);
			cfg.beta1 = opt->value("beta1", cfg.beta1); cfg.beta2 = opt->value("beta2", cfg.beta2);
			cfg.epsilon = opt->value("epsilon", cfg.epsilon); cfg.l2_reg = opt->value("l2_reg", cfg.l2_reg);
		}
	}
	cfg.aabb_scale = (uint32_t)dataset_aabb_scale;
}

inline uint16_t f32_to_f16(float f) {
	uint32_t x; std::memcpy(&x, &f, 4);
	const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
	if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (ax > 0x7f800000u ? 0x200u : 0));
	if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
	if (ax < 0x33000001u) return (uint16_t)sign;
	const int e = (int)(ax >> 23) - 127;
	const uint32_t m = (ax & 0x7fffffu) | 0x800000u;
	const int shift = e < -14 ? 13 + (-14 - e) : 13;
	const uint32_t hexp = e < -14 ? 0 : (uint32_t)(e + 15);
	uint32_t hm = m >> shift;
	const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
	if (rem > half || (rem == half && (hm & 1u))) ++hm;
	return (uint16_t)(sign | (hexp == 0 ? hm : ((hexp - 1) << 10) + hm));
}
inline float f16_to_f32(uint16_t h) {
	const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu;
	uint32_t man = h & 0x3ffu, bits;
	if (exp == 0) {
		if (man == 0) bits = sign;
		else { int e = -1; do { ++e; man <<= 1; } while ((man & 0x400u) == 0); bits = sign | (uint32_t)(127 - 15 - e) << 23 | (man & 0x3ffu) << 13; }
	} else if (exp == 31) bits = sign | 0x7f800000u | man << 13;
	else bits = sign | (exp + 127 - 15) << 23 | man << 13;
	float f; std::memcpy(&f, &bits, 4); return f;
}

// What a snapshot holds, decoded: the network configuration (every root block but "snapshot"), the EMA weights and the occupancy grid widened from half to
// float, and the controller state. The sizes are checked against a context by the caller.
struct Data {
	jsonmin::Value network_config;
	std::vector<float> params, grid;
	bool has_aabb_scale = false;
	uint32_t aabb_scale = 1, training_step = 0, rays_per_batch = 0, measured_before = 0;
	float loss = 0.f;
};

inline Data read(const std::string& path) {
	const mpk::Value root = mpk::load(path);
	if (!root.find("snapshot")) throw std::runtime_error("File '" + path + "' does not contain a snapshot.");
	const mpk::Value& snap = root.at("snapshot");
	if ((uint32_t)snap.at("density_grid_size").number() != RNB_GRIDSIZE) throw std::runtime_error("Incompatible grid size.");
	Data d;
	mpk::Value cfg_root = mpk::Value::object();
	for (const auto& kv : root.map) if (kv.first != "snapshot") cfg_root.set(kv.first, kv.second);
	d.network_config = mpk_to_json(cfg_root);
	check_supported(d.network_config);
	if (const mpk::Value* v = snap.at("nerf").find("aabb_scale")) { d.has_aabb_scale = true; d.aabb_scale = (uint32_t)v->number(); }
	const auto& pb = snap.at("params_binary").bin;
	d.params.resize(pb.size() / 2);
	const uint16_t* ph = reinterpret_cast<const uint16_t*>(pb.data());
	for (size_t i = 0; i < d.params.size(); ++i) d.params[i] = f16_to_f32(ph[i]);
	const auto& gb = snap.at("density_grid_binary").bin;
	d.grid.resize(gb.size() / 2);
	const uint16_t* gh = reinterpret_cast<const uint16_t*>(gb.data());
	for (size_t i = 0; i < d.grid.size(); ++i) d.grid[i] = f16_to_f32(gh[i]);
	d.training_step = (uint32_t)snap.at("training_step").number();
	d.loss = (float)snap.at("loss").number();
	const mpk::Value& rgb = snap.at("nerf").at("rgb");
	d.rays_per_batch = (uint32_t)rgb.at("rays_per_batch").number();
	d.measured_before = (uint32_t)rgb.at("measured_batch_size_before_compaction").number();
	return d;
}

} // namespace snapshot
