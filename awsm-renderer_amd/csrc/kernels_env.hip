// kernels_env.hip — environment cubes at run time (include/awsm_hip.h: awsm_hip_env_cube_write_face / _write_all_faces / _generate_mips /
// _fill_colors / _fill_sky_gradient): source texels of eight formats -> RGBA16F, the 2x2 mip filter through five levels per launch, and the
// expansion of a per-row colour table.  The reference's counterparts are gpu.write_texture (renderer-core/src/cubemap.rs:180-228) and the mip
// compute pass (renderer-core/src/texture/mipmap.rs:143-232, filter_simple for MipmapTextureKind::Albedo).  The arithmetic is DESIGN.md §12:
// every conversion rounds to f16 once, to nearest even; nothing here may be contracted into an fma (-ffp-contract=off).
// The apron of the changed levels is rebuilt afterwards by k_cube_border (kernels_shade.hip), which owns the seam rule.
#include <hip/hip_runtime.h>

#include "frame_params.hpp"
#include "device_math.hpp"
#include "env_cube.hpp"

namespace awsm {

// ---------------- source texels -> RGBA16F ----------------
// W 32-bit words of a texel at any byte address (bytes_per_row and offset are the caller's): whole-texel loads when the address allows
template <int W>
AWSM_DI void load_texel(const uint8_t* p, uint32_t (&w)[W]) {
    const uintptr_t a = (uintptr_t)p;
    if constexpr (W == 4) { if ((a & 15u) == 0) { const uint4 v = *reinterpret_cast<const uint4*>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; return; } }
    if constexpr (W == 2) { if ((a & 7u) == 0) { const uint2 v = *reinterpret_cast<const uint2*>(p); w[0] = v.x; w[1] = v.y; return; } }
    if ((a & 3u) == 0) {
#pragma unroll
        for (int i = 0; i < W; i++) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < W; i++) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
}

AWSM_DI uint2 pack_half4(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return make_uint2(r | g << 16, b | a << 16); }
constexpr uint32_t kHalfOne = 0x3C00u;

__global__ __launch_bounds__(256) void k_env_write(EnvWriteArgs a) {
    const uint32_t per_face = a.n * a.n;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per_face * a.layers) return;
    const uint32_t face = idx / per_face, q = idx - face * per_face, y = q / a.n, x = q - y * a.n;
    const uint8_t* row = a.src + (uint64_t)face * a.image_stride + (uint64_t)y * a.bytes_per_row;
    uint2 out;
    switch (a.format) {
    case AWSM_CUBE_RGBA16F: {                     // bits are copied
        uint32_t w[2]; load_texel<2>(row + (size_t)x * 8u, w);
        out = make_uint2(w[0], w[1]);
        break;
    }
    case AWSM_CUBE_RGBA32F: {
        uint32_t w[4]; load_texel<4>(row + (size_t)x * 16u, w);
        out = pack_half4(f16_bits(__uint_as_float(w[0])), f16_bits(__uint_as_float(w[1])), f16_bits(__uint_as_float(w[2])), f16_bits(__uint_as_float(w[3])));
        break;
    }
    case AWSM_CUBE_RGBA8_UNORM: case AWSM_CUBE_RGBA8_SRGB: case AWSM_CUBE_BGRA8_UNORM: case AWSM_CUBE_BGRA8_SRGB: {
        uint32_t w[1]; load_texel<1>(row + (size_t)x * 4u, w);
        const uint32_t t = (a.format == AWSM_CUBE_RGBA8_SRGB || a.format == AWSM_CUBE_BGRA8_SRGB) ? 256u : 0u;      // alpha is never sRGB-encoded
        const uint32_t c0 = a.tables[t + (w[0] & 255u)], c1 = a.tables[t + ((w[0] >> 8) & 255u)], c2 = a.tables[t + ((w[0] >> 16) & 255u)], al = a.tables[w[0] >> 24];
        const bool bgr = a.format == AWSM_CUBE_BGRA8_UNORM || a.format == AWSM_CUBE_BGRA8_SRGB;
        out = pack_half4(bgr ? c2 : c0, c1, bgr ? c0 : c2, al);
        break;
    }
    case AWSM_CUBE_B10G11R11_UFLOAT: {
        // unsigned floats with f16's exponent (5 bits, bias 15) and 6 / 6 / 5 mantissa bits: the f16 with the same value has the same exponent field
        // and the mantissa at the top of its 10 bits — zero, denormals, infinity and NaN included.  R bits 0..10, G 11..21, B 22..31.
        uint32_t w[1]; load_texel<1>(row + (size_t)x * 4u, w);
        out = pack_half4((w[0] & 0x7FFu) << 4, ((w[0] >> 11) & 0x7FFu) << 4, (w[0] >> 22) << 5, kHalfOne);
        break;
    }
    default: {                                    // AWSM_CUBE_E5B9G9R9_UFLOAT: m * 2^(e - 24), R bits 0..8, G 9..17, B 18..26, e 27..31
        uint32_t w[1]; load_texel<1>(row + (size_t)x * 4u, w);
        const float scale = __uint_as_float(((w[0] >> 27) + 103u) << 23);      // 2^(e - 24): e - 24 + 127 = e + 103 >= 103, a normal f32
        // m < 2^9 and m * 2^(e - 24) lies in [2^-24, 511 * 2^7]: products and conversions are exact
        out = pack_half4(f16_bits((float)(w[0] & 0x1FFu) * scale), f16_bits((float)((w[0] >> 9) & 0x1FFu) * scale), f16_bits((float)((w[0] >> 18) & 0x1FFu) * scale), kHalfOne);
        break;
    }
    }
    a.dst[idx] = out;
}

// ---------------- level 0 from a per-row colour table (the two fills) ----------------
// rows: [6][n] RGBA8 (R in the low byte), one colour per face row, made on the host in double precision
__global__ __launch_bounds__(256) void k_env_expand_rows(const uint32_t* __restrict__ rows, const uint16_t* __restrict__ tables, uint2* __restrict__ dst, uint32_t n) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= 6u * n * n) return;
    const uint32_t w = rows[idx / n];             // idx / n = face * n + y
    dst[idx] = pack_half4(tables[w & 255u], tables[(w >> 8) & 255u], tables[(w >> 16) & 255u], tables[w >> 24]);
}

// ---------------- mip chain: five levels per launch ----------------
// filter_simple (mipmap.rs:143-232) per channel in f32: sum = +0.0; += s(2x, 2y); += s(2x + 1, 2y); += s(2x, 2y + 1); += s(2x + 1, 2y + 1);
// * 0.25; round to f16 (nearest even); store.  The reference clamps the source coordinates to [0, 2 * dst - 1]; a texel that exists (x < dst) never
// reaches that clamp, because 2 * dst <= src — which is also why the last row and column of an odd source are never read.
AWSM_DI f4 unpack_half4(uint2 h) { return {f16_bits_to_f32((unsigned short)(h.x & 0xFFFFu)), f16_bits_to_f32((unsigned short)(h.x >> 16)), f16_bits_to_f32((unsigned short)(h.y & 0xFFFFu)), f16_bits_to_f32((unsigned short)(h.y >> 16))}; }
AWSM_DI uint2 mip_filter(uint2 s00, uint2 s10, uint2 s01, uint2 s11) {
    const f4 a = unpack_half4(s00), b = unpack_half4(s10), c = unpack_half4(s01), d = unpack_half4(s11);
    const float r = ((((0.0f + a.x) + b.x) + c.x) + d.x) * 0.25f, g = ((((0.0f + a.y) + b.y) + c.y) + d.y) * 0.25f;
    const float bl = ((((0.0f + a.z) + b.z) + c.z) + d.z) * 0.25f, al = ((((0.0f + a.w) + b.w) + c.w) + d.w) * 0.25f;
    return pack_half4(f16_bits(r), f16_bits(g), f16_bits(bl), f16_bits(al));
}

// One workgroup = one 32 x 32 tile of one face of the source level (tiles aligned to 32 at that level).  A texel of level +k depends only on the
// 2^k-square below it, so the tile's 16^2, 8^2, 4^2, 2^2 and 1 texels of the next five levels are made here without leaving the workgroup: each level
// goes to LDS as the f16 bits its store writes, and the next one is filtered from those bits — the same values a launch per level would read back.
// Partial tiles and odd sides need only the bounds check x < side of the level: every source of a texel that exists exists (2 * floor(n / 2) <= n).
__global__ __launch_bounds__(256) void k_env_mips(EnvMipArgs a) {
    __shared__ uint2 lds[2][256];
    const uint32_t t = threadIdx.x, face = blockIdx.z;
    uint32_t side = max(a.src_n >> 1, 1u);                      // of the level being made
    {
        const uint32_t lx = t & 15u, ly = t >> 4, x = blockIdx.x * 16u + lx, y = blockIdx.y * 16u + ly;
        uint2 v = make_uint2(0u, 0u);
        if (x < side && y < side) {
            const uint2* s = a.chain + a.src_off + ((size_t)face * a.src_n + 2u * y) * a.src_n + 2u * x;
            v = mip_filter(s[0], s[1], s[a.src_n], s[a.src_n + 1u]);
            a.chain[a.dst_off[0] + ((size_t)face * side + y) * side + x] = v;
        }
        lds[0][t] = v;
    }
    uint32_t w = 16u;                                            // side of the tile's part of the level in lds[cur]
    int cur = 0;
    for (uint32_t k = 1; k < a.n_levels; k++) {
        __syncthreads();
        const uint32_t h = w >> 1;                               // 8, 4, 2, 1
        side = max(side >> 1, 1u);
        if (t < h * h) {
            const uint32_t lx = t % h, ly = t / h, x = blockIdx.x * h + lx, y = blockIdx.y * h + ly;
            uint2 v = make_uint2(0u, 0u);
            if (x < side && y < side) {
                const uint2* s = &lds[cur][(2u * ly) * w + 2u * lx];
                v = mip_filter(s[0], s[1], s[w], s[w + 1u]);
                a.chain[a.dst_off[k] + ((size_t)face * side + y) * side + x] = v;
            }
            lds[cur ^ 1][t] = v;
        }
        cur ^= 1; w = h;
    }
}

}  // namespace awsm

extern "C" void awsm_launch_env_write(const awsm::EnvWriteArgs* a, hipStream_t s) {
    const uint32_t total = a->n * a->n * a->layers;
    if (total) hipLaunchKernelGGL(awsm::k_env_write, dim3((total + 255u) / 256u), dim3(256), 0, s, *a);
}
extern "C" void awsm_launch_env_expand_rows(const uint32_t* rows, const uint16_t* tables, uint2* dst, uint32_t n, hipStream_t s) {
    const uint32_t total = 6u * n * n;
    if (total) hipLaunchKernelGGL(awsm::k_env_expand_rows, dim3((total + 255u) / 256u), dim3(256), 0, s, rows, tables, dst, n);
}
extern "C" void awsm_launch_env_mips(const awsm::EnvMipArgs* a, hipStream_t s) {
    const uint32_t tiles = (a->src_n + 31u) / 32u;
    hipLaunchKernelGGL(awsm::k_env_mips, dim3(tiles, tiles, 6), dim3(256), 0, s, *a);
}
