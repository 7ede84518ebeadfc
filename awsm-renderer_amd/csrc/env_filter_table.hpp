// env_filter_table.hpp — the sample tables of awsm_hip_env_cube_filter.  Host-side, no HIP: awsm_resources.cpp builds a level's table
// here and uploads it; header-only so that tests/test_env_filter_cpu.py can compile it with g++ into a program of its own and compare every entry,
// bit for bit, with the Python restatement (tests/ibl_filter_reference.py).  A table depends on (kind, level, levels, samples, source side) only,
// never on the texel; it is made in f64 — the operations below, in this order — and each number is rounded to f32 once.
//
// The point set is the BRDF LUT's (renderer-core/src/brdf_lut/shader.wgsl): xi_i = (i / S, radical_inverse_vdc(i)), alpha = roughness^2, GGX importance
// sampling of the half vector around N = V.
#pragma once
#include <stdint.h>
#include <cmath>
#include <vector>

namespace awsm {

struct EnvFilterEntry { float x, y, z, w, lod; };      // GGX: h.x h.y h.z, N.L, lod — Lambert: the sample direction in the (T, B, n) frame, 1, lod
static_assert(sizeof(EnvFilterEntry) == 20, "five floats");

enum { kEnvFilterGgx = 0, kEnvFilterLambert = 1 };
constexpr double kEnvFilterPi = 3.141592653589793;

inline double env_filter_radical_inverse(uint32_t bits) {      // van der Corput: the bits of i mirrored about the binary point
    bits = (bits << 16) | (bits >> 16);
    bits = ((bits & 0x55555555u) << 1) | ((bits & 0xAAAAAAAAu) >> 1);
    bits = ((bits & 0x33333333u) << 2) | ((bits & 0xCCCCCCCCu) >> 2);
    bits = ((bits & 0x0F0F0F0Fu) << 4) | ((bits & 0xF0F0F0F0u) >> 4);
    bits = ((bits & 0x00FF00FFu) << 8) | ((bits & 0xFF00FF00u) >> 8);
    return (double)bits * 2.3283064365386963e-10;      // 2^-32
}

// lod of a sample whose density is pdf: the level whose texel subtends the sample's share of the sphere, plus one (the usual bias)
inline double env_filter_lod(double pdf, uint32_t samples, uint32_t src_size) {
    const double omega_p = 4.0 * kEnvFilterPi / (6.0 * (double)src_size * (double)src_size);
    const double lod = 0.5 * std::log2(1.0 / ((double)samples * pdf * omega_p)) + 1.0;
    return lod > 0.0 ? lod : 0.0;      // also NaN
}

// Level `level` of `levels` (GGX: 1 <= level < levels; Lambert: both ignored), `samples` points, a source of side src_size.  Entries whose weight is
// not positive are dropped, the rest keep their order.
inline std::vector<EnvFilterEntry> env_filter_table(uint32_t kind, uint32_t level, uint32_t levels, uint32_t samples, uint32_t src_size) {
    std::vector<EnvFilterEntry> out;
    out.reserve(samples);
    const double r = kind == kEnvFilterGgx ? (double)level / (double)(levels - 1u) : 1.0;
    const double alpha = r * r, a2 = alpha * alpha;
    for (uint32_t i = 0; i < samples; i++) {
        const double xi_x = (double)i / (double)samples, xi_y = env_filter_radical_inverse(i);
        const double phi = 2.0 * kEnvFilterPi * xi_x;
        double c, s_theta, w, pdf;
        if (kind == kEnvFilterGgx) {
            c = std::sqrt((1.0 - xi_y) / (1.0 + (a2 - 1.0) * xi_y));
            const double s2 = 1.0 - c * c;
            s_theta = std::sqrt(s2 > 0.0 ? s2 : 0.0);
            w = 2.0 * (c * c) - 1.0;
            if (!(w > 0.0)) continue;
            const double t = (c * c) * (a2 - 1.0) + 1.0;
            pdf = (a2 / (kEnvFilterPi * (t * t))) / 4.0;
        } else {
            c = std::sqrt(1.0 - xi_y);
            s_theta = std::sqrt(xi_y);
            w = 1.0;
            pdf = c / kEnvFilterPi;
        }
        EnvFilterEntry e;
        e.x = (float)(std::cos(phi) * s_theta); e.y = (float)(std::sin(phi) * s_theta); e.z = (float)c;
        e.w = (float)w; e.lod = (float)env_filter_lod(pdf, samples, src_size);
        out.push_back(e);
    }
    return out;
}

}  // namespace awsm
