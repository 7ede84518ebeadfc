// texture_pool_check.cpp — TEST INFRASTRUCTURE ONLY: a program of its own (tests/test_texture_pool_cpu.py builds it with AddressSanitizer and
// UBSan) over awsm-renderer_amd/csrc/tex_pool.hpp, the code awsm_hip_texture_array_write_layers validates with.
//   1. every validation rule with a source buffer that is exactly one byte short of what its layout needs: an error, and nothing is read — the
//      buffers are heap blocks of exactly data_len bytes, so a read past them is an ASan report;
//   2. accepted layouts are then gathered the way k_tex_write addresses them (layer * image_stride + row * bytes_per_row + x * 4, a 4-byte load
//      where the address allows, bytes otherwise) from a block of exactly `used` bytes, converted, and printed for the test to compare with numpy;
//   3. the 256-byte table and the premultiply of all 65,536 pairs, printed likewise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tex_pool.hpp"

using namespace awsm;

static int check(uint32_t w, uint32_t h, uint32_t layers, uint32_t first, uint32_t n, size_t len, TexWriteDesc d, size_t* used) {
    char msg[128] = "";
    std::vector<uint8_t>* block = new std::vector<uint8_t>(len ? len : 1, 0xCD);      // exactly data_len bytes on the heap
    const int rc = tex_write_validate(w, h, layers, first, n, true, len, &d, used, msg, sizeof msg);
    delete block;
    return rc;
}

int main() {
    const uint32_t W = 5, H = 3, L = 4;
    const TexWriteDesc tight = {(uint32_t)sizeof(TexWriteDesc), 0u, 0u, 0u, W * 4u, H, 0u};
    size_t used = 0;
    int fails = 0;
    auto expect = [&](const char* what, int got, int want) { if (got != want) { printf("FAIL %s: %d, expected %d\n", what, got, want); fails++; } };
    // the exact size passes, one byte less does not — for one image, for three, with padding and with an offset
    expect("tight, 1 layer", check(W, H, L, 0, 1, W * H * 4, tight, &used), kTexOk);
    expect("tight, 1 layer, one short", check(W, H, L, 0, 1, W * H * 4 - 1, tight, &used), kTexInvalid);
    expect("tight, 3 layers", check(W, H, L, 1, 3, 3 * W * H * 4, tight, &used), kTexOk);
    expect("tight, 3 layers, one short", check(W, H, L, 1, 3, 3 * W * H * 4 - 1, tight, &used), kTexInvalid);
    TexWriteDesc padded = tight; padded.bytes_per_row = W * 4 + 7; padded.rows_per_image = H + 2;
    const size_t padded_need = (size_t)2 * padded.bytes_per_row * padded.rows_per_image + (size_t)(H - 1) * padded.bytes_per_row + W * 4;
    expect("padded, 3 layers", check(W, H, L, 0, 3, padded_need, padded, &used), kTexOk);
    expect("padded: used", (int)used, (int)padded_need);
    expect("padded, 3 layers, one short", check(W, H, L, 0, 3, padded_need - 1, padded, &used), kTexInvalid);
    TexWriteDesc off = tight; off.offset = 6;
    expect("offset 6", check(W, H, L, 0, 1, W * H * 4 + 6, off, &used), kTexOk);
    expect("offset 6, one short", check(W, H, L, 0, 1, W * H * 4 + 5, off, &used), kTexInvalid);
    off.offset = ~0ull;
    expect("offset 2^64 - 1", check(W, H, L, 0, 1, W * H * 4, off, &used), kTexInvalid);
    TexWriteDesc bad = tight; bad.bytes_per_row = W * 4 - 1;
    expect("bytes_per_row one short of a row", check(W, H, L, 0, 1, 1 << 20, bad, &used), kTexInvalid);
    bad = tight; bad.rows_per_image = H - 1;
    expect("rows_per_image one short, 2 layers", check(W, H, L, 0, 2, 1 << 20, bad, &used), kTexInvalid);
    expect("rows_per_image unused for 1 layer", check(W, H, L, 0, 1, W * H * 4, bad, &used), kTexOk);
    bad = tight; bad.bytes_per_row = 0xFFFFFFFFu; bad.rows_per_image = 0xFFFFFFFFu;
    expect("huge layout", check(W, H, 65536, 0, 65536, 1 << 20, bad, &used), kTexInvalid);
    bad = tight; bad.format = 1;
    expect("format", check(W, H, L, 0, 1, 1 << 20, bad, &used), kTexUnsupported);
    bad = tight; bad.flags = 4;
    expect("flag bit", check(W, H, L, 0, 1, 1 << 20, bad, &used), kTexUnsupported);
    bad = tight; bad.struct_size = 8;
    expect("struct_size", check(W, H, L, 0, 1, 1 << 20, bad, &used), kTexInvalid);
    expect("layers past the array", check(W, H, L, 2, 3, 1 << 20, tight, &used), kTexOutOfRange);
    expect("first_layer wraps", check(W, H, L, 0xFFFFFFFFu, 2, 1 << 20, tight, &used), kTexOutOfRange);
    expect("n_layers 0", check(W, H, L, 0, 0, 1 << 20, tight, &used), kTexInvalid);
    { char msg[8]; expect("no data", tex_write_validate(W, H, L, 0, 1, false, 1 << 20, &tight, &used, msg, sizeof msg), kTexInvalid); }

    // the gather, from a block of exactly `used` bytes, for each flag value
    uint8_t table[256];
    tex_srgb_table(table);
    printf("TABLE");
    for (int q = 0; q < 256; q++) printf(" %u", table[q]);
    printf("\n");
    unsigned long long sum = 0;
    for (uint32_t c = 0; c < 256; c++) for (uint32_t a = 0; a < 256; a++) {
        const uint32_t p = tex_premultiply(c | 0u << 8 | 255u << 16 | a << 24);
        if ((p >> 24) != a || ((p >> 8) & 255u) != 0u || ((p >> 16) & 255u) != a) { printf("FAIL premultiply(%u, %u)\n", c, a); fails++; }
        sum = sum * 1000003ull + (p & 255u);
    }
    printf("PREMULTIPLY %llu\n", sum);
    for (const TexWriteDesc& d : {tight, padded}) {
        for (uint32_t flags = 0; flags < 4; flags++) {
            const uint32_t n = 2;
            if (check(W, H, L, 0, n, 1 << 20, d, &used) != kTexOk) { printf("FAIL gather layout\n"); fails++; continue; }
            uint8_t* src = (uint8_t*)malloc(used);
            for (size_t i = 0; i < used; i++) src[i] = (uint8_t)((i * 37u + 11u) ^ (i >> 3));
            printf("GATHER %u %u %u", d.bytes_per_row, d.rows_per_image, flags);
            const uint64_t image_stride = (uint64_t)d.bytes_per_row * d.rows_per_image;
            for (uint32_t l = 0; l < n; l++) for (uint32_t y = 0; y < H; y++) for (uint32_t x = 0; x < W; x++) {
                const uint8_t* p = src + l * image_stride + (uint64_t)y * d.bytes_per_row + x * 4u;
                uint32_t v;
                if (((uintptr_t)p & 3u) == 0) memcpy(&v, p, 4);
                else v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
                if (flags & kTexPremultiplyAlpha) v = tex_premultiply(v);
                if (flags & kTexSrgbToLinear) v = (uint32_t)table[v & 255u] | (uint32_t)table[(v >> 8) & 255u] << 8 | (uint32_t)table[(v >> 16) & 255u] << 16 | (v & 0xFF000000u);
                printf(" %u", v);
            }
            printf("\n");
            free(src);
        }
    }
    if (!fails) printf("TEXTURE_POOL_CHECK_OK\n");
    return fails ? 1 : 0;
}
