// env_cube.hpp — launch arguments shared by awsm_hip.cpp and kernels_env.hip (environment cubes at run time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace awsm
