// ktx2.hpp — KTX2 cube-map container reader (header-only; no device, no allocation).
//
// The counterpart of the reference's create_texture over a ktx2::Reader (crates/renderer-core/src/cubemap/ktx.rs:39-147): the same
// rejections in the same order with the same reasons, for the eight uncompressed formats this renderer stores cubes from.  The container
// layout is the Khronos KTX 2.0 specification's: a 12-byte identifier, nine u32 header fields, the index (dfd / kvd / sgd offsets and
// lengths), then one {byteOffset, byteLength, uncompressedByteLength} u64 triple per level — levels are found through that index only
// (the file stores the smallest level first).  Every offset and length is compared with the buffer's length in 64 bits before any byte is
// read: a truncated or hostile file is an error string, never a read out of bounds.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/awsm_host.h"

namespace awsm_host {
namespace ktx2 {

inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

constexpr size_t kHeaderBytes = 80;      // identifier + header + index
constexpr size_t kLevelIndexBytes = 24;
constexpr uint32_t kMaxLevels = 16;
constexpr uint32_t kMaxSize = 8192;      // the largest cube side the device layer takes

// VkFormat -> AwsmCubeFormat and bytes per texel, for the formats map_ktx_format (ktx.rs:375-598) maps to a WebGPU format this renderer reads
inline bool map_format(uint32_t vk, uint32_t* fmt, uint32_t* bytes_per_texel) {
    switch (vk) {
    case 37: *fmt = AWSM_CUBE_RGBA8_UNORM; *bytes_per_texel = 4; return true;          // R8G8B8A8_UNORM
    case 43: *fmt = AWSM_CUBE_RGBA8_SRGB; *bytes_per_texel = 4; return true;           // R8G8B8A8_SRGB
    case 44: *fmt = AWSM_CUBE_BGRA8_UNORM; *bytes_per_texel = 4; return true;          // B8G8R8A8_UNORM
    case 50: *fmt = AWSM_CUBE_BGRA8_SRGB; *bytes_per_texel = 4; return true;           // B8G8R8A8_SRGB
    case 97: *fmt = AWSM_CUBE_RGBA16F; *bytes_per_texel = 8; return true;              // R16G16B16A16_SFLOAT
    case 109: *fmt = AWSM_CUBE_RGBA32F; *bytes_per_texel = 16; return true;            // R32G32B32A32_SFLOAT
    case 122: *fmt = AWSM_CUBE_B10G11R11_UFLOAT; *bytes_per_texel = 4; return true;    // B10G11R11_UFLOAT_PACK32
    case 123: *fmt = AWSM_CUBE_E5B9G9R9_UFLOAT; *bytes_per_texel = 4; return true;     // E5B9G9R9_UFLOAT_PACK32
    }
    return false;
}
// what an unsupported VkFormat is, for the message: the core block-compressed range (BC, ETC2, EAC, ASTC LDR), the ASTC HDR and PVRTC extensions, depth / stencil
inline const char* format_family(uint32_t vk) {
    if ((vk >= 131 && vk <= 184) || (vk >= 1000066000u && vk <= 1000066013u) || (vk >= 1000054000u && vk <= 1000054007u)) return " (block-compressed)";
    if (vk >= 124 && vk <= 130) return " (depth / stencil)";
    return "";
}

inline int refuse(int code, char* err, size_t cap, const char* text) {
    if (err && cap) snprintf(err, cap, "%s", text);
    return code;
}

// -> AWSM_OK and *out filled (out->struct_size is the caller's, checked), or a negative AwsmStatus with the reason in err
inline int parse(const uint8_t* data, size_t len, AwsmKtx2Info* out, char* err, size_t cap) {
    char msg[256];
    if (err && cap) err[0] = 0;
    if (!data || !out) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "ktx2: no data or no AwsmKtx2Info");
    if (out->struct_size != sizeof(AwsmKtx2Info)) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "ktx2: AwsmKtx2Info.struct_size does not match this library");
    static const uint8_t kId[12] = {0xAB, 0x4B, 0x54, 0x58, 0x20, 0x32, 0x30, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A};
    if (len < kHeaderBytes) { snprintf(msg, sizeof msg, "ktx2: %zu bytes, a KTX2 header takes %zu (truncated file)", len, kHeaderBytes); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
    if (memcmp(data, kId, 12) != 0) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "ktx2: not a KTX2 file (bad identifier)");
    const uint32_t vk = rd32(data + 12), width = rd32(data + 20), height = rd32(data + 24), depth = rd32(data + 28);
    const uint32_t layers = rd32(data + 32), faces = rd32(data + 36), level_count = rd32(data + 40), scheme = rd32(data + 44);
    const uint32_t stored = level_count ? level_count : 1u;
    if (width == 0) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "ktx2: pixelWidth is zero");
    if (stored > 32u || (uint64_t)stored * kLevelIndexBytes > (uint64_t)len - kHeaderBytes) {
        snprintf(msg, sizeof msg, "ktx2: the index of %u levels does not fit the file's %zu bytes (truncated file)", stored, len);
        return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg);
    }
    // ktx.rs:41-63
    if (faces != 6) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "KTX file does not contain a cubemap");
    if (layers != 0) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "KTX file contains array textures, which are not supported for cubemaps");
    if (depth > 1) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "KTX file contains 3D textures, which are not supported for cubemaps");
    if (scheme != 0) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "KTX file uses supercompression, which is not supported");
    // ktx.rs:65-89
    if (vk == 0) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "KTX file does not specify a format");
    uint32_t fmt = 0, bpt = 0;
    if (!map_format(vk, &fmt, &bpt)) {
        snprintf(msg, sizeof msg, "KTX file has unsupported format: vkFormat %u%s", vk, format_family(vk));
        return refuse(AWSM_ERR_UNSUPPORTED, err, cap, msg);
    }
    // a cube: square faces (cubemap/images.rs:236-241; WebGPU requires it of a cube view), within the device layer's range, no more levels than the size has
    if (width != height) { snprintf(msg, sizeof msg, "Cubemap faces must be square, got %ux%u", width, height); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
    if (width > kMaxSize) { snprintf(msg, sizeof msg, "ktx2: cube side %u, at most %u", width, kMaxSize); return refuse(AWSM_ERR_UNSUPPORTED, err, cap, msg); }
    uint32_t full = 1;
    while ((width >> full) != 0) full++;
    if (stored > full || stored > kMaxLevels) { snprintf(msg, sizeof msg, "ktx2: %u levels, a %u^2 cube has at most %u", stored, width, full); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
    // ktx.rs:119-147: every level is exactly six tight faces
    AwsmKtx2Info info;
    memset(&info, 0, sizeof info);
    for (uint32_t l = 0; l < stored; l++) {
        const uint8_t* e = data + kHeaderBytes + (size_t)l * kLevelIndexBytes;
        const uint64_t off = rd64(e), length = rd64(e + 8);
        if (off > (uint64_t)len || length > (uint64_t)len - off) {
            snprintf(msg, sizeof msg, "ktx2: level %u lies at bytes %llu + %llu of a %zu-byte file (truncated file)", l, (unsigned long long)off, (unsigned long long)length, len);
            return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg);
        }
        const uint64_t n = (width >> l) ? (width >> l) : 1u, expected = 6u * n * n * bpt;      // <= 6 * 8192^2 * 16
        if (length != expected) {
            snprintf(msg, sizeof msg, "Level %u byte length %llu doesn't match expected face*rows*tight_bpr %llu (possible KTX per-face padding not supported)", l,
                     (unsigned long long)length, (unsigned long long)expected);
            return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg);
        }
        info.level[l].offset = off; info.level[l].length = length;
    }
    info.struct_size = sizeof info; info.vk_format = vk; info.format = fmt; info.size = width; info.faces = faces; info.layers = layers;
    info.levels = stored; info.mips = level_count ? level_count : full;      // levelCount 0: "generate the full chain" (KTX 2.0 §3.7)
    *out = info;
    return AWSM_OK;
}

}  // namespace ktx2
}  // namespace awsm_host
