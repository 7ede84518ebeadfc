// tex_pool.hpp — the 2D texture pool at run time: launch arguments shared by awsm_resources.cpp and kernels_texture.hip, and the parts
// of the contract that are plain C++ — the sRGB table, the integer premultiply and the validation of a write — so that the host library and the
// CPU tests use the very same code.  No HIP header is needed to include this file.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define AWSM_TEX_HD __host__ __device__ inline
#else
#define AWSM_TEX_HD inline
#endif

namespace awsm {

constexpr uint32_t kTexPremultiplyAlpha = 1u, kTexSrgbToLinear = 2u;      // AWSM_TEX_PREMULTIPLY_ALPHA, AWSM_TEX_SRGB_TO_LINEAR

// the sRGB decode in f64: this table's and the environment cubes' 8-bit -> f16 table's (awsm_resources.cpp: env_tables)
inline double srgb_to_linear(double c) { return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); }

// sRGB-encoded q / 255 -> linear, stored as unorm8 = floor(clamp(lin, 0, 1) * 255 + 0.5): 256 bytes, evaluated in f64.  No entry lies within 1e-3
// of a rounding tie, so an f32 evaluation of the same expression (the reference's shader) gives the same bytes (tests/test_texture_pool_cpu.py).
inline void tex_srgb_table(uint8_t out[256]) {
    for (int q = 0; q < 256; q++) {
        double lin = srgb_to_linear((double)q / 255.0);
        lin = lin < 0.0 ? 0.0 : (lin > 1.0 ? 1.0 : lin);
        out[q] = (uint8_t)floor(lin * 255.0 + 0.5);
    }
}

// premultiply on the encoded 8-bit values: floor(c * a / 255 + 0.5) = (2 c a + 255) / 510 in integers; alpha is kept
AWSM_TEX_HD uint32_t tex_premultiply(uint32_t rgba) {
    const uint32_t a = rgba >> 24;
    const uint32_t r = (2u * (rgba & 255u) * a + 255u) / 510u, g = (2u * ((rgba >> 8) & 255u) * a + 255u) / 510u, b = (2u * ((rgba >> 16) & 255u) * a + 255u) / 510u;
    return r | g << 8 | b << 16 | a << 24;
}

// What a write needs checked before a byte of `data` is read (WebGPU's writeTexture rules; awsm_hip_texture_array_write_layers).  Mirrors
// AwsmTexWrite of include/awsm_hip.h field by field.
struct TexWriteDesc {
    uint32_t struct_size, format, flags, mipmap_kind;
    uint32_t bytes_per_row, rows_per_image;
    uint64_t offset;
};
enum { kTexOk = 0, kTexInvalid = -1, kTexUnsupported = -6, kTexOutOfRange = -7 };      // AWSM_OK / AWSM_ERR_*
// -> kTexOk and *used = the bytes the gather reads from data + offset (through the last texel of the last row of the last image), or an error and a
// message.  Every comparison is made in 64 bits.
inline int tex_write_validate(uint32_t width, uint32_t height, uint32_t array_layers, uint32_t first_layer, uint32_t n_layers, bool has_data, size_t data_len,
                              const TexWriteDesc* d, size_t* used, char* msg, size_t msg_cap) {
    auto say = [&](int code, const char* text) { if (msg && msg_cap) snprintf(msg, msg_cap, "%s", text); return code; };
    if (!has_data || !d || d->struct_size != sizeof(TexWriteDesc)) return say(kTexInvalid, "data, or an AwsmTexWrite with its struct_size, is missing");
    if (n_layers == 0) return say(kTexInvalid, "n_layers must be non-zero");
    if (d->format != 0u) return say(kTexUnsupported, "unknown source format (0 = RGBA8)");
    if (d->flags & ~(kTexPremultiplyAlpha | kTexSrgbToLinear)) return say(kTexUnsupported, "unknown flag bit");
    if ((uint64_t)first_layer + n_layers > array_layers) return say(kTexOutOfRange, "layers past the array");
    const uint64_t row = (uint64_t)width * 4u;
    if ((uint64_t)d->bytes_per_row < row) return say(kTexInvalid, "bytes_per_row does not cover a row");
    if (n_layers > 1 && d->rows_per_image < height) return say(kTexInvalid, "rows_per_image does not cover an image");
    // offset + (n - 1) * rows_per_image * bytes_per_row + (height - 1) * bytes_per_row + width * 4 <= data_len
    const unsigned long long per_image = (unsigned long long)d->bytes_per_row * d->rows_per_image;      // two 32-bit factors
    unsigned long long need, images, rows, end;
    if (__builtin_mul_overflow(per_image, (unsigned long long)(n_layers - 1u), &images) ||
        __builtin_mul_overflow((unsigned long long)d->bytes_per_row, (unsigned long long)(height - 1u), &rows) ||
        __builtin_add_overflow(rows, (unsigned long long)row, &rows) || __builtin_add_overflow(images, rows, &need) ||
        __builtin_add_overflow(need, (unsigned long long)d->offset, &end))
        return say(kTexInvalid, "layout overflows 64 bits");
    if ((unsigned long long)data_len < end) return say(kTexInvalid, "the source buffer is too small for the layout");
    *used = (size_t)need;
    return kTexOk;
}

// k_tex_write: RGBA8 texels gathered through the caller's layout into level 0 of consecutive layers
struct TexWriteArgs {
    const uint8_t* src;         // device staging; byte 0 = data[offset]
    uint32_t* dst;              // first texel of the first layer written, level 0
    uint32_t width, height, n_layers, flags;
    uint32_t bytes_per_row;
    uint64_t image_stride;      // bytes_per_row * rows_per_image
    uint32_t srgb[64];          // the 256-byte table, byte q of word q / 4
};

// k_tex_mips: up to five levels below one source level, for layers [first_layer, first_layer + n_layers)
struct TexMipArgs {
    uint32_t* chain;
    const uint32_t* kinds;      // MipmapTextureKind per layer of the array
    uint32_t layers;            // of the array: a level's layer l starts layers-independent at level_off + l * w_l * h_l
    uint32_t first_layer, n_layers;
    uint32_t src_off, sw, sh;   // the source level: first texel, extent
    uint32_t n_levels;          // levels made by this launch, 1..5
    uint32_t dst_off[5];
};

}  // namespace awsm
