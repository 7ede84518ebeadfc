// kernels_texture.hip — the 2D texture pool: level 0 at run time (include/awsm_hip.h: awsm_hip_texture_array_write_layers) and the
// RGBA8 mip chains, a level per launch over a whole array (awsm_hip_texture_array_generate_mips) or five levels per launch over a range of layers
// (_generate_mips_layers).  The reference's counterparts are TexturePool's external-image copy with premultiplied_alpha and its sRGB -> linear pass
// (renderer-core/src/texture/texture_pool.rs:233-303, texture/convert_srgb.rs:52-76) and the mip compute pass (texture/mipmap.rs:95-330).
// k_gen_mip_level and k_tex_mips share one 2x2 filter, tex_mip_filter, and one unorm8 store, tex_to_unorm8: STRICT f32, never contracted into fmas
// (-ffp-contract=off), so that the RGBA8 results are bit-identical everywhere.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "tex_pool.hpp"
#include "launch.hpp"

namespace awsm {

// ---------------- source texels -> level 0 ----------------
// One thread per destination texel.  The 256-byte sRGB table comes by value in the launch arguments and is put into LDS by the first wavefront:
// a lookup is then one ds_read_u8 per channel at a lane-varying index, which kernel-argument (scalar) memory cannot serve.
__global__ __launch_bounds__(256) void k_tex_write(TexWriteArgs a) {
    __shared__ uint32_t table_words[64];
    if (threadIdx.x < 64u) table_words[threadIdx.x] = a.srgb[threadIdx.x];
    __syncthreads();
    const uint8_t* table = reinterpret_cast<const uint8_t*>(table_words);
    const uint32_t per_layer = a.width * a.height;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per_layer * a.n_layers) return;
    const uint32_t layer = idx / per_layer, q = idx - layer * per_layer, y = q / a.width, x = q - y * a.width;
    const uint8_t* p = a.src + (uint64_t)layer * a.image_stride + (uint64_t)y * a.bytes_per_row + (size_t)x * 4u;
    uint32_t w;
    if (((uintptr_t)p & 3u) == 0) w = *reinterpret_cast<const uint32_t*>(p);
    else w = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    if (a.flags & kTexPremultiplyAlpha) w = tex_premultiply(w);      // the external-image copy comes first, the conversion pass second
    if (a.flags & kTexSrgbToLinear) w = (uint32_t)table[w & 255u] | (uint32_t)table[(w >> 8) & 255u] << 8 | (uint32_t)table[(w >> 16) & 255u] << 16 | (w & 0xFF000000u);
    a.dst[idx] = w;
}

// ---------------- mip chains ----------------
// generate_mipmaps (renderer-core/src/texture/mipmap.rs:140-250): 2x2 texel loads, filter by MipmapTextureKind, store as
// unorm8 = floor(clamp(v,0,1)*255 + 0.5)
AWSM_DI uint32_t tex_to_unorm8(float v) {
    if (!(v > 0.0f)) return 0u;          // also NaN
    if (v > 1.0f) v = 1.0f;
    return (uint32_t)floorf(v * 255.0f + 0.5f);
}
// t[k]: the source texels in k order (x + (k & 1), y + (k >> 1)); kind is wave-uniform
AWSM_DI uint32_t tex_mip_filter(const uint32_t (&t)[4], uint32_t kind) {
    float r[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        r[k][0] = (float)(t[k] & 255u) / 255.0f; r[k][1] = (float)((t[k] >> 8) & 255u) / 255.0f;
        r[k][2] = (float)((t[k] >> 16) & 255u) / 255.0f; r[k][3] = (float)(t[k] >> 24) / 255.0f;
    }
    float o0, o1, o2, o3;
    if (kind == 2u) {            // filter_metallic_roughness
        float m = 0.0f, r2 = 0.0f, b = 0.0f, al = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) { m += r[k][0]; r2 += r[k][1] * r[k][1]; b += r[k][2]; al += r[k][3]; }
        o0 = m * 0.25f; o1 = sqrtf(r2 * 0.25f); o2 = b * 0.25f; o3 = al * 0.25f;
    } else {
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) { s0 += r[k][0]; s1 += r[k][1]; s2 += r[k][2]; s3 += r[k][3]; }
        o0 = s0 * 0.25f; o1 = s1 * 0.25f; o2 = s2 * 0.25f; o3 = s3 * 0.25f;          // filter_simple
        if (kind == 1u) {        // filter_normal: renormalise
            const f3 n = normalize(mk3(o0 * 2.0f - 1.0f, o1 * 2.0f - 1.0f, o2 * 2.0f - 1.0f));
            o0 = n.x * 0.5f + 0.5f; o1 = n.y * 0.5f + 0.5f; o2 = n.z * 0.5f + 0.5f;
        }
    }
    return tex_to_unorm8(o0) | (tex_to_unorm8(o1) << 8) | (tex_to_unorm8(o2) << 16) | (tex_to_unorm8(o3) << 24);
}

// One level of a whole array: one thread per destination texel and layer, the loads clamped to 2 x the destination extent (and to the real source
// extent).  On whole arrays a launch per level is faster than k_tex_mips below.
__global__ __launch_bounds__(256) void k_gen_mip_level(uint32_t* __restrict__ chain, uint32_t src_off, uint32_t dst_off, uint32_t sw, uint32_t sh,
                                                       uint32_t dw, uint32_t dh, uint32_t layers, const uint32_t* __restrict__ kinds) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= dw * dh * layers) return;
    const uint32_t x = i % dw, y = (i / dw) % dh, layer = i / (dw * dh);
    const uint32_t kind = kinds[layer];
    const uint32_t* src = chain + src_off + (size_t)layer * sw * sh;
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t sx = min(min(x * 2u + (uint32_t)(k & 1), dw * 2u - 1u), sw - 1u);
        uint32_t sy = min(min(y * 2u + (uint32_t)(k >> 1), dh * 2u - 1u), sh - 1u);
        t[k] = src[(size_t)sy * sw + sx];
    }
    chain[dst_off + ((size_t)layer * dh + y) * dw + x] = tex_mip_filter(t, kind);
}

// ---------------- five levels per launch, a range of layers ----------------
// the 2x2 sources of local texel (lx, ly) in a tile stored `stride` words per row.  k_gen_mip_level reads min(min(2x + k, 2 dw - 1), sw - 1): for a
// source extent of two or more that is 2x + k itself (2 dw <= sw), for an extent of one it is 0 — xinc / yinc say which.
AWSM_DI uint32_t tex_filter_at(const uint32_t* tile, uint32_t stride, uint32_t lx, uint32_t ly, uint32_t xinc, uint32_t yinc, uint32_t kind) {
    const uint32_t* s0 = tile + (2u * ly) * stride + 2u * lx;
    const uint32_t* s1 = s0 + yinc * stride;
    const uint32_t t[4] = {s0[0], s0[xinc], s1[0], s1[xinc]};
    return tex_mip_filter(t, kind);
}

// One workgroup = one 32 x 32 tile of one layer of the source level (tiles aligned to 32 at that level) -> the tile's 16^2, 8^2, 4^2, 2^2 and 1 texels
// of the next five levels.  The source tile is staged in LDS by 16-byte loads (four texels per thread) where the level's rows allow it; every level made
// goes to LDS as the RGBA8 word its store writes (two buffers, ping-pong) and the next is filtered from those words: the bytes a launch per level would
// read back.  A texel of level +k depends only on the aligned 2^k square below it — floor-halved odd extents included, and the clamp to the source
// extent acts only where that extent is 1 — so nothing crosses a workgroup and partial tiles need only x < w, y < h of the level being made.
// kTexStageStride: 48 words per staged row put the two rows a 32-lane half reads with one ds_read_b64 (rows 2 ly and 2 ly + 2: 96 words apart) on
// opposite halves of the 64 banks.
constexpr uint32_t kTexStageStride = 48u;
__global__ __launch_bounds__(256) void k_tex_mips(TexMipArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[32u * kTexStageStride];
    __shared__ uint32_t lv[2][256];
    const uint32_t t = threadIdx.x;
    uint32_t pw = a.sw, ph = a.sh;                                           // extent of the level being read
    uint32_t dw = max(pw >> 1, 1u), dh = max(ph >> 1, 1u);                   // ... and of the level being made
    const uint32_t tiles_x = (dw + 15u) / 16u, tiles_y = (dh + 15u) / 16u, tiles = tiles_x * tiles_y;
    const uint32_t li = blockIdx.x / tiles, tile = blockIdx.x - li * tiles, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    if (li >= a.n_layers) return;                                            // whole workgroup
    const uint32_t layer = a.first_layer + li;
    const uint32_t kind = a.kinds[layer];
    {
        const uint32_t r = t >> 3, c4 = (t & 7u) * 4u, sx = tx * 32u + c4, sy = ty * 32u + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (sy < ph && sx < pw) {
            const uint32_t* s = a.chain + a.src_off + ((size_t)layer * ph + sy) * pw + sx;
            if (((pw | a.src_off) & 3u) == 0u) v = *reinterpret_cast<const uint4*>(s);      // sx + 3 < pw and the address is a multiple of 16
            else {
                v.x = s[0];
                if (sx + 1u < pw) v.y = s[1];
                if (sx + 2u < pw) v.z = s[2];
                if (sx + 3u < pw) v.w = s[3];
            }
        }
        *reinterpret_cast<uint4*>(&stage[r * kTexStageStride + c4]) = v;
    }
    __syncthreads();
    {
        const uint32_t lx = t & 15u, ly = t >> 4, x = tx * 16u + lx, y = ty * 16u + ly;
        uint32_t v = 0u;
        if (x < dw && y < dh) {
            v = tex_filter_at(stage, kTexStageStride, lx, ly, pw > 1u ? 1u : 0u, ph > 1u ? 1u : 0u, kind);
            a.chain[a.dst_off[0] + ((size_t)layer * dh + y) * dw + x] = v;
        }
        lv[0][t] = v;
    }
    uint32_t w = 16u;                                                        // side of the tile's part of the level in lv[cur]
    int cur = 0;
    for (uint32_t k = 1; k < a.n_levels; k++) {
        __syncthreads();
        const uint32_t h = w >> 1;                                           // 8, 4, 2, 1
        pw = dw; ph = dh; dw = max(pw >> 1, 1u); dh = max(ph >> 1, 1u);
        if (t < h * h) {
            const uint32_t lx = t % h, ly = t / h, x = tx * h + lx, y = ty * h + ly;
            uint32_t v = 0u;
            if (x < dw && y < dh) {
                v = tex_filter_at(lv[cur], w, lx, ly, pw > 1u ? 1u : 0u, ph > 1u ? 1u : 0u, kind);
                a.chain[a.dst_off[k] + ((size_t)layer * dh + y) * dw + x] = v;
            }
            lv[cur ^ 1][t] = v;
        }
        cur ^= 1; w = h;
    }
}

}  // namespace awsm

extern "C" void awsm_launch_tex_write(const awsm::TexWriteArgs* a, hipStream_t s) {
    const uint32_t total = a->width * a->height * a->n_layers;
    if (total) hipLaunchKernelGGL(awsm::k_tex_write, dim3((total + 255u) / 256u), dim3(256), 0, s, *a);
}
extern "C" void awsm_launch_gen_mip_level(uint8_t* chain, uint32_t src_off, uint32_t dst_off, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t layers,
                                          const uint32_t* kinds, hipStream_t s) {
    const uint32_t n = dw * dh * layers;
    if (n) hipLaunchKernelGGL(awsm::k_gen_mip_level, dim3((n + 255u) / 256u), dim3(256), 0, s, (uint32_t*)chain, src_off, dst_off, sw, sh, dw, dh, layers, kinds);
}
extern "C" void awsm_launch_tex_mips(const awsm::TexMipArgs* a, hipStream_t s) {
    const uint32_t dw = a->sw > 1u ? a->sw >> 1 : 1u, dh = a->sh > 1u ? a->sh >> 1 : 1u;
    const uint32_t tiles = ((dw + 15u) / 16u) * ((dh + 15u) / 16u);
    if (a->n_layers) hipLaunchKernelGGL(awsm::k_tex_mips, dim3(tiles * a->n_layers), dim3(256), 0, s, *a);
}
