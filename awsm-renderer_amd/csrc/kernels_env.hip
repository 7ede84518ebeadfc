// kernels_env.hip — environment cubes at run time (include/awsm_hip.h: awsm_hip_env_cube_write_face / _write_all_faces / _generate_mips /
// _fill_colors / _fill_sky_gradient): source texels of eight formats -> RGBA16F, the 2x2 mip filter through five levels per launch, and the
// expansion of a per-row colour table; awsm_hip_env_cube_filter: a source cube filtered into a GGX-prefiltered chain or a
// Lambert irradiance level; and awsm_hip_env_cube_from_equirect (§16): an equirectangular panorama projected into level 0.  The reference's counterparts are gpu.write_texture (renderer-core/src/cubemap.rs:180-228) and the mip
// compute pass (renderer-core/src/texture/mipmap.rs:143-232, filter_simple for MipmapTextureKind::Albedo).  The arithmetic is DESIGN.md §12:
// every conversion rounds to f16 once, to nearest even; nothing here may be contracted into an fma (-ffp-contract=off).
// The apron of the changed levels is rebuilt afterwards by k_cube_border (kernels_shade.hip) by the seam rule of cube_seam.hpp.
#include <hip/hip_runtime.h>

#include "frame_params.hpp"
#include "device_math.hpp"
#include "env_cube.hpp"
#include "cube_seam.hpp"
#include "launch.hpp"

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

// ---------------- filtering a source cube into the split-sum inputs (awsm_hip_env_cube_filter) ----------------
// textureSampleLevel on the source by sample_cube's contract (kernels_shade.hip), with its seam rule (cube_seam.hpp; the face ladder is restated, see there): the major
// axis picks the face, bilinear on the level's N x N faces, a tap off the face comes from the face across that edge, the level is clamped to the
// chain and its two nearest levels are blended.  Divisions and square roots are IEEE here; nothing is clamped, so a non-finite texel propagates.
AWSM_DI f3 env_lerp3(f3 a, f3 b, float t) { const float s = 1.0f - t; return {a.x * s + b.x * t, a.y * s + b.y * t, a.z * s + b.z * t}; }
AWSM_DI f3 env_rgb(uint2 h) { return {f16_bits_to_f32((unsigned short)(h.x & 0xFFFFu)), f16_bits_to_f32((unsigned short)(h.x >> 16)), f16_bits_to_f32((unsigned short)(h.y & 0xFFFFu))}; }
// one level; sn, tn = 0.5 (sc / ma) + 0.5 on `face`
AWSM_DI f3 env_cube_level(const CubeDev& c, uint32_t level, uint32_t face, float sn, float tn) {
    const int N = (int)max(c.size >> level, 1u);
    float x = sn * (float)N - 0.5f, y = tn * (float)N - 0.5f;
    if (!(x >= -0.5f)) x = -0.5f;                 // also NaN (zero / non-finite direction): the face's first texel
    if (!(y >= -0.5f)) y = -0.5f;
    x = fminf(x, (float)N - 0.5f); y = fminf(y, (float)N - 0.5f);
    const float flx = floorf(x), fly = floorf(y), fx = x - flx, fy = y - fly;
    const int i0 = (int)flx, j0 = (int)fly;      // -1 .. N - 1
    uint2 t00, t10, t01, t11;
    if (c.bordered) {                             // the footprint lies inside the face's (N + 2)^2 array: two adjacent texels of two rows
        const uint32_t P = (uint32_t)N + 2u;
        const uint2* r0 = c.bordered + c.b_level_off[level] + ((size_t)face * P + (uint32_t)(j0 + 1)) * P + (uint32_t)(i0 + 1);
        t00 = r0[0]; t10 = r0[1]; t01 = r0[P]; t11 = r0[P + 1u];
    } else {
        const uint32_t base = c.level_off[level];
        t00 = cube_texel_raw(c, base, N, face, i0, j0); t10 = cube_texel_raw(c, base, N, face, i0 + 1, j0);
        t01 = cube_texel_raw(c, base, N, face, i0, j0 + 1); t11 = cube_texel_raw(c, base, N, face, i0 + 1, j0 + 1);
    }
    return env_lerp3(env_lerp3(env_rgb(t00), env_rgb(t10), fx), env_lerp3(env_rgb(t01), env_rgb(t11), fx), fy);
}
AWSM_DI f3 env_sample_cube(const CubeDev& c, f3 d, float level) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    uint32_t face; float sc, tc, ma;
    if (az >= ax && az >= ay) { face = d.z < 0.0f ? 5u : 4u; sc = d.z < 0.0f ? -d.x : d.x; tc = -d.y; ma = az; }
    else if (ay >= ax) { face = d.y < 0.0f ? 3u : 2u; sc = d.x; tc = d.y < 0.0f ? -d.z : d.z; ma = ay; }
    else { face = d.x < 0.0f ? 1u : 0u; sc = d.x < 0.0f ? d.z : -d.z; tc = -d.y; ma = ax; }
    const float inv = 1.0f / ma;
    const float sn = 0.5f * (sc * inv) + 0.5f, tn = 0.5f * (tc * inv) + 0.5f;
    const float top = (float)(c.mips - 1u);
    float lod = level > 0.0f ? level : 0.0f;          // also NaN
    lod = fminf(lod, top);
    const float fl = floorf(lod), fr = lod - fl;
    const uint32_t l0 = (uint32_t)fl, l1 = min(l0 + 1u, c.mips - 1u);
    f3 r = env_cube_level(c, l0, face, sn, tn);
    if (fr > 0.0f && l1 != l0) r = env_lerp3(r, env_cube_level(c, l1, face, sn, tn), fr);
    return r;
}
// the direction through the centre of texel (i, j) of `face` on a level of side n: the inverse of sample_cube's face table
AWSM_DI f3 env_texel_dir(uint32_t face, uint32_t i, uint32_t j, uint32_t n) {
    const float s = (2.0f * ((float)i + 0.5f)) / (float)n - 1.0f, t = (2.0f * ((float)j + 0.5f)) / (float)n - 1.0f;
    f3 d;
    switch (face) {
    case 0: d = {1.0f, -t, -s}; break;
    case 1: d = {-1.0f, -t, s}; break;
    case 2: d = {s, 1.0f, t}; break;
    case 3: d = {s, -1.0f, -t}; break;
    case 4: d = {s, -t, 1.0f}; break;
    default: d = {-s, -t, -1.0f}; break;
    }
    return normalize(d);
}

// One wavefront per output texel, four texels of one level per workgroup.  The level's table goes through LDS in chunks of kEnvFilterChunk entries;
// lane l takes entries l, l + 64, ... in that order (a chunk is a multiple of 64 long, so the order does not depend on the chunking), accumulates in
// f32, and the 64 partial sums meet in a fixed xor butterfly — no atomics: the same input gives the same bits.
__global__ __launch_bounds__(256) void k_env_filter(EnvFilterArgs a) {
    __shared__ float tab[kEnvFilterChunk * 5u];
    uint32_t li = 0u;
    while (li + 1u < a.n_levels && blockIdx.x >= a.level[li + 1u].first_block) li++;
    const EnvFilterLevel lv = a.level[li];
    const uint32_t lane = threadIdx.x & 63u, per_face = lv.n * lv.n;
    const uint32_t texel = (blockIdx.x - lv.first_block) * 4u + (threadIdx.x >> 6);
    const bool live = texel < 6u * per_face;      // the padding of the level's last workgroup still stages the table
    const uint32_t face = live ? texel / per_face : 0u, q = live ? texel - face * per_face : 0u;
    const f3 n = env_texel_dir(face, q % lv.n, q / lv.n, lv.n);
    const f3 up = fabsf(n.z) < 0.999f ? mk3(0.0f, 0.0f, 1.0f) : mk3(1.0f, 0.0f, 0.0f);
    const f3 T = normalize(cross(up, n)), B = cross(n, T);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (uint32_t base = 0u; base < lv.count; base += kEnvFilterChunk) {
        const uint32_t m = min(kEnvFilterChunk, lv.count - base);
        __syncthreads();
        const float* src = a.tables + (size_t)(lv.table_off + base) * 5u;
        for (uint32_t k = threadIdx.x; k < m * 5u; k += 256u) tab[k] = src[k];
        __syncthreads();
        if (live) {
            for (uint32_t e = lane; e < m; e += 64u) {
                const float hx = tab[e * 5u], hy = tab[e * 5u + 1u], hz = tab[e * 5u + 2u], w = tab[e * 5u + 3u], lod = tab[e * 5u + 4u];
                f3 L = {(T.x * hx + B.x * hy) + n.x * hz, (T.y * hx + B.y * hy) + n.y * hz, (T.z * hx + B.z * hy) + n.z * hz};
                if (!a.lambert) { const float c2 = 2.0f * hz; L = {c2 * L.x - n.x, c2 * L.y - n.y, c2 * L.z - n.z}; }      // V = N mirrored about H
                const f3 s = env_sample_cube(a.src, L, lod);
                sr += w * s.x; sg += w * s.y; sb += w * s.z; sw += w;
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sr += __shfl_xor(sr, off); sg += __shfl_xor(sg, off); sb += __shfl_xor(sb, off); sw += __shfl_xor(sw, off);
    }
    if (lane == 0u) {
        const float r = a.lambert ? a.k * sr : sr / sw, g = a.lambert ? a.k * sg : sg / sw, b = a.lambert ? a.k * sb : sb / sw;
        a.dst[lv.dst_off + texel] = pack_half4(f16_bits(r), f16_bits(g), f16_bits(b), kHalfOne);
    }
}

// level 0 of a prefiltered chain (roughness 0): the source's own texels, or the source resampled when the sides differ
__global__ __launch_bounds__(256) void k_env_filter_level0(EnvFilterLevel0Args a) {
    const uint32_t per_face = a.n * a.n, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= 6u * per_face) return;
    if (a.n == a.src.size) {
        const uint2 t = a.src.texels[idx];
        a.dst[idx] = make_uint2(t.x, (t.y & 0xFFFFu) | kHalfOne << 16);
        return;
    }
    const uint32_t face = idx / per_face, q = idx - face * per_face;
    const f3 s = env_sample_cube(a.src, env_texel_dir(face, q % a.n, q / a.n, a.n), a.lod);
    a.dst[idx] = pack_half4(f16_bits(s.x), f16_bits(s.y), f16_bits(s.z), kHalfOne);
}

// ---------------- level 0 from an equirectangular panorama (awsm_hip_env_cube_from_equirect) ----------------
// One panorama pixel as RGB in f32.  RGBE8: e == 0 is black, else m * 2^(e - 136) by ldexp — exact (m < 2^8; e - 136 >= -135 stays above f32's last
// denormal bit).  RGBA32F: the first three floats.  Any byte address: a padded bytes_per_row need not be a multiple of the pixel size.
AWSM_DI f3 pano_pixel(const EnvEquirectArgs& a, uint32_t col, uint32_t row) {
    const uint8_t* r = a.src + (uint64_t)row * a.bytes_per_row;
    if (a.format == AWSM_PANO_RGBE8) {
        uint32_t w[1]; load_texel<1>(r + (size_t)col * 4u, w);
        const uint32_t e = w[0] >> 24;
        if (e == 0u) return {0.0f, 0.0f, 0.0f};
        const int k = (int)e - 136;
        return {ldexpf((float)(w[0] & 255u), k), ldexpf((float)((w[0] >> 8) & 255u), k), ldexpf((float)((w[0] >> 16) & 255u), k)};
    }
    uint32_t w[3]; load_texel<3>(r + (size_t)col * 16u, w);
    return {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
}

// One thread per level-0 texel, a workgroup = a 16 x 16 tile of one face (grid padded per face): neighbouring lanes look in neighbouring directions and
// so read neighbouring panorama pixels.  Per texel S x S taps, b outer and a inner; per tap the direction through the sub-sample by §13's face table,
// u = atan2(d.x, -d.z) / 2 pi + 0.5 + turn reduced to [0, 1], v = acos(d.y) / pi, and §3's bilinear rule at x = u W - 0.5, y = v H - 0.5 with columns
// wrapped and rows clamped.  The mean times `scale`, NaN -> 0, clamped to f16's finite range, rounded once; alpha 1.0; one 8-byte store.
__global__ __launch_bounds__(256) void k_env_from_equirect(EnvEquirectArgs a) {
    const uint32_t i = blockIdx.x * 16u + (threadIdx.x & 15u), j = blockIdx.y * 16u + (threadIdx.x >> 4), face = blockIdx.z;
    if (i >= a.n || j >= a.n) return;
    const float fn = (float)a.n, fs = (float)a.samples, fw = (float)a.width, fh = (float)a.height;
    const int wi = (int)a.width, hi = (int)a.height;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (uint32_t sb_i = 0; sb_i < a.samples; sb_i++) {
        const float t = (2.0f * ((float)j + ((float)sb_i + 0.5f) / fs)) / fn - 1.0f;
        for (uint32_t sa_i = 0; sa_i < a.samples; sa_i++) {
            const float s = (2.0f * ((float)i + ((float)sa_i + 0.5f) / fs)) / fn - 1.0f;
            f3 d;
            switch (face) {
            case 0: d = {1.0f, -t, -s}; break;
            case 1: d = {-1.0f, -t, s}; break;
            case 2: d = {s, 1.0f, t}; break;
            case 3: d = {s, -1.0f, -t}; break;
            case 4: d = {s, -t, 1.0f}; break;
            default: d = {-s, -t, -1.0f}; break;
            }
            d = normalize(d);
            float u = (atan2f(d.x, -d.z) * 0.15915494f + 0.5f) + a.turn;                 // 1 / (2 pi)
            u = u - floorf(u);                                                            // [0, 1]: 1.0 itself when u was a hair below an integer
            const float v = acosf(fminf(fmaxf(d.y, -1.0f), 1.0f)) * 0.31830987f;          // 1 / pi
            const float x = u * fw - 0.5f, y = v * fh - 0.5f;
            const float flx = floorf(x), fly = floorf(y), fx = x - flx, fy = y - fly;
            int x0 = (int)flx, x1 = x0 + 1, y0 = (int)fly, y1 = y0 + 1;                   // x0 in [-1, W - 1], y0 in [-1, H - 1]
            if (x0 < 0) x0 += wi;
            if (x1 >= wi) x1 -= wi;
            // the columns are inside [0, W) by the reduction of u and the rows are clamped; the unsigned min keeps every load inside the source whatever u and v were
            const uint32_t c0 = min((uint32_t)x0, a.width - 1u), c1 = min((uint32_t)x1, a.width - 1u);
            const uint32_t r0 = (uint32_t)min(max(y0, 0), hi - 1), r1 = (uint32_t)min(max(y1, 0), hi - 1);
            const f3 p00 = pano_pixel(a, c0, r0), p10 = pano_pixel(a, c1, r0), p01 = pano_pixel(a, c0, r1), p11 = pano_pixel(a, c1, r1);
            const f3 tap = env_lerp3(env_lerp3(p00, p10, fx), env_lerp3(p01, p11, fx), fy);
            sr += tap.x; sg += tap.y; sb += tap.z;
        }
    }
    const float k = 1.0f / (fs * fs);
    float r = (sr * k) * a.scale, g = (sg * k) * a.scale, b = (sb * k) * a.scale;
    r = r == r ? fminf(fmaxf(r, -65504.0f), 65504.0f) : 0.0f;
    g = g == g ? fminf(fmaxf(g, -65504.0f), 65504.0f) : 0.0f;
    b = b == b ? fminf(fmaxf(b, -65504.0f), 65504.0f) : 0.0f;
    a.dst[((size_t)face * a.n + j) * a.n + i] = pack_half4(f16_bits(r), f16_bits(g), f16_bits(b), kHalfOne);
}

}  // namespace awsm

extern "C" void awsm_launch_env_from_equirect(const awsm::EnvEquirectArgs* a, hipStream_t s) {
    const uint32_t tiles = (a->n + 15u) / 16u;
    if (tiles) hipLaunchKernelGGL(awsm::k_env_from_equirect, dim3(tiles, tiles, 6), dim3(256), 0, s, *a);
}
extern "C" void awsm_launch_env_filter(const awsm::EnvFilterArgs* a, uint32_t blocks, hipStream_t s) {
    if (blocks) hipLaunchKernelGGL(awsm::k_env_filter, dim3(blocks), dim3(256), 0, s, *a);
}
extern "C" void awsm_launch_env_filter_level0(const awsm::EnvFilterLevel0Args* a, hipStream_t s) {
    const uint32_t total = 6u * a->n * a->n;
    hipLaunchKernelGGL(awsm::k_env_filter_level0, dim3((total + 255u) / 256u), dim3(256), 0, s, *a);
}
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
