// cube_seam.hpp — the cube sampling contract and what lies across a face's edge: the one seam table and seam rule, for the cube sampler of the
// shading kernels and k_cube_border (kernels_shade.hip) and for the IBL filter (kernels_env.hip).  Integer work only: nothing here rounds, so it
// compiles the same under either contraction setting.
#pragma once
#include "frame_params.hpp"
#include "device_math.hpp"

namespace awsm {

// ---------------- cubemaps: textureSampleLevel(texture_cube<f32>, linear / linear / linear sampler, direction, level) ----------------
// (skybox.wgsl:37, brdf.wgsl:268-290).  Contract where WebGPU defers to the hardware: the major axis picks the face (z if |z| >= |x|,|y|,
// else y if |y| >= |x|, else x — the Vulkan / D3D table, as are sc, tc in cube_level); bilinear on the level's N x N faces with texel
// centres at (i + 0.5) / N; a tap that falls off the face comes from the face across that edge (seamless, kCubeEdge; a corner tap,
// off in both directions, keeps its row); the level is clamped to the chain and the two nearest levels are blended by its fraction.
// Continuous in the direction everywhere but at the eight corners, which is what lets a relaxed-arithmetic direction stay in tolerance.
// kCubeEdge[face][edge: 0 left (i = -1), 1 right (i = N), 2 up (j = -1), 3 down (j = N)] = face' | swap << 3 | flip << 4 | far << 5:
// the running coordinate k (j for left / right, i for up / down), reversed if flip, becomes j' (swap) or i'; the other one is N - 1 (far) or 0.
__device__ const uint8_t kCubeEdge[6][4] = {{44, 13, 58, 43}, {45, 12, 10, 27}, {1, 16, 21, 4}, {49, 32, 36, 53}, {41, 8, 34, 3}, {40, 9, 18, 51}};
AWSM_DI uint2 cube_texel_raw(const CubeDev& c, uint32_t level_base, int N, uint32_t face, int i, int j) {
    if (i < 0 || i >= N) j = min(max(j, 0), N - 1);     // corner taps keep their row
    if (i < 0 || i >= N || j < 0 || j >= N) {
        const uint32_t e = i < 0 ? 0u : (i >= N ? 1u : (j < 0 ? 2u : 3u));
        const uint32_t t = kCubeEdge[face][e];
        int k = e < 2u ? j : i;
        if (t & 16u) k = N - 1 - k;
        const int far = (t & 32u) ? N - 1 : 0;
        face = t & 7u;
        if (t & 8u) { i = far; j = k; } else { i = k; j = far; }
    }
    return c.texels[level_base + ((size_t)face * (size_t)N + (size_t)j) * (size_t)N + (size_t)i];
}
// The face ladder (the major axis picks the face) is written out by its two users, cube_level (kernels_shade.hip) and env_sample_cube
// (kernels_env.hip), which divide by the major axis differently (rcp / IEEE): as a function shared by the two it compiled to the same instructions with
// the operands of one multiplication exchanged in both filter kernels, and these kernels are held to their instruction text (tools/isa_diff.py).
}  // namespace awsm
