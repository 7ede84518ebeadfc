// rgbe.hpp — Radiance picture (.hdr) reader (header-only; no device, no allocation: the caller passes the output buffer).
//
// The file format is Greg Ward's "Real Pixels" (Graphics Gems II) as Radiance's color.c / header.c / resolu.c read it: a text header of lines up to
// an empty line, one resolution line, then the scanlines as RGBE quadruples — flat, with the old run pixels, or as four run-length coded channel
// planes.  The output is the W x H quadruples, top-down, 4 bytes each: the device decodes them (k_env_from_equirect).
// Every offset and length is compared with the buffer's length in 64 bits before any byte is read: a truncated or hostile file is an error
// string, never a read out of bounds — and never a write past out_cap.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/awsm_host.h"

namespace awsm_host {
namespace rgbe {

constexpr uint32_t kMaxSide = 32768;
constexpr uint64_t kMaxPixels = 1ull << 28;
constexpr size_t kMaxHeaderLine = 2048;      // a longer header line is not a Radiance header

inline int refuse(int code, char* err, size_t cap, const char* text) {
    if (err && cap) snprintf(err, cap, "%s", text);
    return code;
}

// the line that starts at `at`: [at, *end) without its '\n' (and without a '\r' in front of it); *next is the byte after the '\n'.  false at the end
// of the data or when no '\n' follows within kMaxHeaderLine bytes
inline bool next_line(const uint8_t* data, uint64_t len, uint64_t at, uint64_t* end, uint64_t* next) {
    if (at >= len) return false;
    const uint64_t stop = len - at > kMaxHeaderLine ? at + kMaxHeaderLine : len;
    uint64_t e = at;
    while (e < stop && data[e] != '\n') e++;
    if (e >= stop) return false;
    *next = e + 1;
    if (e > at && data[e - 1] == '\r') e--;
    *end = e;
    return true;
}
inline bool starts_with(const uint8_t* p, uint64_t n, const char* word) {
    const size_t w = strlen(word);
    return n >= w && memcmp(p, word, w) == 0;
}
// a line as a C string for the messages and for strtod: at most cap - 1 bytes, unprintable bytes as '?'
inline void line_text(const uint8_t* p, uint64_t n, char* out, size_t cap) {
    size_t k = 0;
    for (; k + 1 < cap && k < n; k++) out[k] = (p[k] >= 32 && p[k] < 127) ? (char)p[k] : '?';
    out[k] = 0;
}
// "<sign><axis> <digits>" at p[*i ...]: the sign and axis characters and the number (false: not of that shape, or more than nine digits)
inline bool axis_term(const uint8_t* p, uint64_t n, uint64_t* i, char* sign, char* axis, uint64_t* value) {
    while (*i < n && p[*i] == ' ') (*i)++;
    if (n - *i < 4 || (p[*i] != '+' && p[*i] != '-') || (p[*i + 1] != 'X' && p[*i + 1] != 'Y') || p[*i + 2] != ' ') return false;
    *sign = (char)p[*i]; *axis = (char)p[*i + 1];
    *i += 3;
    while (*i < n && p[*i] == ' ') (*i)++;
    uint64_t v = 0; int digits = 0;
    while (*i < n && p[*i] >= '0' && p[*i] <= '9' && digits < 10) { v = v * 10 + (uint64_t)(p[*i] - '0'); (*i)++; digits++; }
    if (digits == 0 || digits > 9) return false;
    *value = v;
    return true;
}

// The text header and the resolution line -> *out (struct_size is the caller's, checked; rle is left 0) and the offset of the first scanline
inline int parse_header(const uint8_t* data, size_t len_, AwsmHdrInfo* out, uint64_t* pixels_at, char* err, size_t cap) {
    char msg[256], text[96];
    if (err && cap) err[0] = 0;
    if (!data || !out) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "hdr: no data or no AwsmHdrInfo");
    if (out->struct_size != sizeof(AwsmHdrInfo)) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "hdr: AwsmHdrInfo.struct_size does not match this library");
    const uint64_t len = (uint64_t)len_;
    uint64_t at = 0, end = 0, next = 0;
    if (!next_line(data, len, at, &end, &next) || !starts_with(data, end, "#?")) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "hdr: not a Radiance picture (the first line does not start with #?)");
    double exposure = 1.0;
    for (;;) {
        at = next;
        if (!next_line(data, len, at, &end, &next)) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "hdr: the header does not end with an empty line (truncated file)");
        const uint8_t* p = data + at;
        const uint64_t n = end - at;
        if (n == 0) break;
        if (starts_with(p, n, "FORMAT=")) {
            line_text(p + 7, n - 7, text, sizeof text);
            if (strcmp(text, "32-bit_rle_rgbe") != 0) {
                snprintf(msg, sizeof msg, "hdr: FORMAT=%s is not supported (only 32-bit_rle_rgbe)", text);
                return refuse(AWSM_ERR_UNSUPPORTED, err, cap, msg);
            }
        } else if (starts_with(p, n, "EXPOSURE=")) {
            line_text(p + 9, n - 9, text, sizeof text);
            char* stop = nullptr;
            const double v = strtod(text, &stop);
            if (stop != text && isfinite(v) && v > 0.0) exposure *= v;      // a value that is no positive number is ignored, as any other line
        }
    }
    at = next;
    if (!next_line(data, len, at, &end, &next)) return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, "hdr: no resolution line (truncated file)");
    const uint8_t* p = data + at;
    const uint64_t n = end - at;
    line_text(p, n, text, sizeof text);
    uint64_t i = 0, v0 = 0, v1 = 0;
    char s0 = 0, a0 = 0, s1 = 0, a1 = 0;
    bool shaped = axis_term(p, n, &i, &s0, &a0, &v0) && axis_term(p, n, &i, &s1, &a1, &v1) && a0 != a1;
    while (shaped && i < n && p[i] == ' ') i++;
    if (!shaped || i != n) { snprintf(msg, sizeof msg, "hdr: bad resolution line \"%s\"", text); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
    if (a0 != 'Y' || s1 != '+') {
        snprintf(msg, sizeof msg, "hdr: orientation \"%s\" is not supported (only -Y H +X W and +Y H +X W)", text);
        return refuse(AWSM_ERR_UNSUPPORTED, err, cap, msg);
    }
    const uint64_t h = v0, w = v1;
    if (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide || w * h > kMaxPixels) {
        snprintf(msg, sizeof msg, "hdr: %llu x %llu pixels (1..%u per side, at most 2^28 in all)", (unsigned long long)w, (unsigned long long)h, kMaxSide);
        return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg);
    }
    out->width = (uint32_t)w; out->height = (uint32_t)h; out->flipped_y = s0 == '+' ? 1u : 0u; out->rle = 0u;
    out->exposure = (float)exposure;
    *pixels_at = next;
    return AWSM_OK;
}

inline bool rle_marker(const uint8_t* p, uint64_t avail, uint32_t w) {
    return w >= 8 && w < 32768 && avail >= 4 && p[0] == 2 && p[1] == 2 && p[2] < 128 && (((uint32_t)p[2] << 8) | p[3]) == w;
}

// awsm_host_hdr_info: the header alone; rle says whether the first scanline is run-length coded in the new style
inline int info(const uint8_t* data, size_t len, AwsmHdrInfo* out, char* err, size_t cap) {
    uint64_t at = 0;
    const int rc = parse_header(data, len, out, &at, err, cap);
    if (rc) return rc;
    out->rle = rle_marker(data + at, (uint64_t)len - at, out->width) ? 1u : 0u;
    return AWSM_OK;
}

// awsm_host_hdr_decode: width * height RGBE quadruples into rgbe_out (out_cap bytes), top-down; rle = 1 when any scanline was coded in the new style
inline int decode(const uint8_t* data, size_t len_, uint8_t* rgbe_out, size_t out_cap, AwsmHdrInfo* out, char* err, size_t cap) {
    char msg[256];
    uint64_t at = 0;
    int rc = parse_header(data, len_, out, &at, err, cap);
    if (rc) return rc;
    const uint64_t len = (uint64_t)len_, w = out->width, h = out->height, need = w * h * 4u;
    if (!rgbe_out || (uint64_t)out_cap < need) {
        snprintf(msg, sizeof msg, "hdr: out_cap %zu, %u x %u pixels take %llu bytes", rgbe_out ? out_cap : (size_t)0, out->width, out->height, (unsigned long long)need);
        return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg);
    }
    uint8_t prev[4] = {0, 0, 0, 0};
    bool have_prev = false;
    for (uint64_t row = 0; row < h; row++) {
        uint8_t* line = rgbe_out + (out->flipped_y ? h - 1u - row : row) * w * 4u;
        if (rle_marker(data + at, len - at, out->width)) {
            out->rle = 1u;
            at += 4;
            for (uint32_t ch = 0; ch < 4; ch++) {
                uint64_t x = 0;
                while (x < w) {
                    if (at >= len) { snprintf(msg, sizeof msg, "hdr: scanline %llu is truncated", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                    const uint32_t count = data[at++];
                    if (count == 0) { snprintf(msg, sizeof msg, "hdr: scanline %llu has a zero count", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                    const uint64_t run = count > 128 ? count - 128 : count;
                    if (run > w - x) { snprintf(msg, sizeof msg, "hdr: scanline %llu has a run over the scanline end", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                    const uint64_t bytes = count > 128 ? 1u : run;
                    if (bytes > len - at) { snprintf(msg, sizeof msg, "hdr: scanline %llu is truncated", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                    if (count > 128) { const uint8_t v = data[at]; for (uint64_t k = 0; k < run; k++) line[(x + k) * 4u + ch] = v; }
                    else for (uint64_t k = 0; k < run; k++) line[(x + k) * 4u + ch] = data[at + k];
                    at += bytes; x += run;
                }
            }
            if (w) { memcpy(prev, line + (w - 1u) * 4u, 4); have_prev = true; }
            continue;
        }
        uint64_t x = 0;
        uint32_t shift = 0;
        while (x < w) {
            if (len - at < 4) { snprintf(msg, sizeof msg, "hdr: scanline %llu is truncated", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
            const uint8_t* q = data + at;
            at += 4;
            if (q[0] == 1 && q[1] == 1 && q[2] == 1) {      // an old-style run of the previous pixel
                if (!have_prev) { snprintf(msg, sizeof msg, "hdr: scanline %llu starts with a run pixel before any pixel", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                const uint64_t run = shift < 32 ? (uint64_t)q[3] << shift : (q[3] ? ~0ull : 0ull);
                if (run > w - x) { snprintf(msg, sizeof msg, "hdr: scanline %llu has a run over the scanline end", (unsigned long long)row); return refuse(AWSM_ERR_INVALID_ARGUMENT, err, cap, msg); }
                for (uint64_t k = 0; k < run; k++) memcpy(line + (x + k) * 4u, prev, 4);
                x += run;
                if (shift < 32) shift += 8;
            } else {
                memcpy(line + x * 4u, q, 4);
                memcpy(prev, q, 4); have_prev = true;
                x++; shift = 0;
            }
        }
    }
    return AWSM_OK;
}

}  // namespace rgbe
}  // namespace awsm_host
