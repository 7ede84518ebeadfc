// env_cube.hpp — launch arguments shared by awsm_resources.cpp and kernels_env.hip (environment cubes at run time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frame_params.hpp"

namespace awsm {

// k_env_write: source texels of one of the AwsmCubeFormat formats, gathered through the caller's layout, become RGBA16F
struct EnvWriteArgs {
    const uint8_t* src;         // device staging; byte 0 = data[layout.offset]
    uint2* dst;                 // first texel of the first face written, in the plain chain
    const uint16_t* tables;     // f16 bits: [0, 256) q / 255, [256, 512) the sRGB decode of q / 255
    uint32_t n;                 // side of the level
    uint32_t layers;            // 1 or 6
    uint32_t format;            // AwsmCubeFormat
    uint32_t bytes_per_row;
    uint64_t image_stride;      // bytes_per_row * rows_per_image
};

// k_env_mips: up to five levels below one source level
struct EnvMipArgs {
    uint2* chain;               // the plain chain
    uint32_t src_off;           // first texel of the source level
    uint32_t src_n;             // its side
    uint32_t n_levels;          // levels made by this launch, 1..5
    uint32_t dst_off[5];        // first texel of each
};

// k_env_filter / k_env_filter_level0 (awsm_hip_env_cube_filter): a source cube filtered into levels of a destination chain
constexpr uint32_t kEnvFilterChunk = 1024;      // table entries staged in LDS at a time (20 KB)
struct EnvFilterLevel {
    uint32_t dst_off;           // first texel of the level in the destination's plain chain
    uint32_t n;                 // its side
    uint32_t first_block;       // the level's workgroups are [first_block, first_block + ceil(6 n^2 / 4))
    uint32_t table_off;         // first entry of the level's table
    uint32_t count;             // entries (those with a positive weight), <= 4096
};
struct EnvFilterArgs {
    CubeDev src;                // bordered null: the plain chain with the seam rule
    uint2* dst;                 // the destination's plain chain
    const float* tables;        // EnvFilterEntry records (env_filter_table.hpp), five floats each
    uint32_t n_levels;          // levels made by this launch
    uint32_t lambert;           // 0: sum(w s) / sum(w), directions mirrored about the half vector; 1: k * sum(s)
    float k;
    EnvFilterLevel level[kMaxMipLevels];
};
struct EnvFilterLevel0Args {
    CubeDev src;
    uint2* dst;                 // level 0 of the destination
    uint32_t n;                 // its side
    float lod;                  // max(0, log2(src.size / n)); unused when n == src.size (the bits are copied)
};

// k_env_from_equirect (awsm_hip_env_cube_from_equirect): an equirectangular panorama projected into level 0 of a cube
struct EnvEquirectArgs {
    const uint8_t* src;         // device staging: row y at src + y * bytes_per_row
    uint2* dst;                 // level 0 of the plain chain
    uint32_t n;                 // side of level 0
    uint32_t width, height;     // of the panorama
    uint32_t format;            // AwsmPanoFormat
    uint32_t bytes_per_row;
    uint32_t samples;           // S, 1..8 (auto resolved on the host)
    float turn;                 // yaw / 2 pi reduced to [0, 1) on the host in f64
    float scale;                // 0 resolved to 1 on the host
};

}  // namespace awsm
