"""Environment cubes at run time, the parts that need no GPU: the KTX2 reader (awsm_host_ktx2_parse over files written here), the host entries
over a backend that lacks the device symbols (tests/mock), the row tables of the two fills against hand-computed bytes, and the reader under
AddressSanitizer + UndefinedBehaviorSanitizer as a program of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from tests.test_host_layer_cpu import MOCK, mock  # noqa: F401  (the module-scoped fixture builds the mock backend)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -6

KTX2_ID = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x32, 0x30, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
# vkFormat -> (AwsmCubeFormat name, bytes per texel)
VK_FORMATS = {37: ("rgba8unorm", 4), 43: ("rgba8unorm-srgb", 4), 44: ("bgra8unorm", 4), 50: ("bgra8unorm-srgb", 4), 97: ("rgba16f", 8),
              109: ("rgba32f", 16), 122: ("rg11b10ufloat", 4), 123: ("rgb9e5ufloat", 4)}


def write_ktx2(vk_format, size, levels, level_count=None, faces=6, layers=0, depth=0, scheme=0, height=None, pad=0, largest_first=False):
    """A KTX2 file: identifier, header, index (no dfd / kvd / sgd), level index, then the level data — the smallest level first, as the
    specification stores them, `pad` bytes apart.  levels: level 0 first, each the bytes of six tight faces."""
    n = len(levels)
    head = KTX2_ID + struct.pack("<9I", vk_format, 1, size, size if height is None else height, depth, layers, faces, n if level_count is None else level_count, scheme)
    head += struct.pack("<4I2Q", 0, 0, 0, 0, 0, 0)
    at = len(head) + 24 * n
    order = list(range(n)) if largest_first else list(range(n - 1, -1, -1))
    offsets, body = [0] * n, b""
    for l in order:
        body += b"\xEE" * pad
        offsets[l] = at + len(body)
        body += levels[l]
    index = b"".join(struct.pack("<3Q", offsets[l], len(levels[l]), len(levels[l])) for l in range(n))
    return head + index + body


def level_bytes(size, level, bpt, seed=0):
    n = max(size >> level, 1)
    return np.random.default_rng(seed + level).integers(0, 256, size=6 * n * n * bpt, dtype=np.uint8).tobytes()


def refused(data, code, text=None):
    with pytest.raises(H.HostError) as e:
        H.ktx2_parse(data)
    assert e.value.code == code, e.value
    if text:
        assert text in str(e.value), e.value
    return str(e.value)


# ------------------------------------------------------------------------------------------------ the reader

@pytest.mark.parametrize("vk", sorted(VK_FORMATS))
def test_ktx2_parse_each_format(vk):
    name, bpt = VK_FORMATS[vk]
    levels = [level_bytes(8, l, bpt) for l in range(4)]
    info = H.ktx2_parse(write_ktx2(vk, 8, levels))
    assert info["vk_format"] == vk and info["format_name"] == name and info["format"] == hip_backend.CUBE_FORMATS[name][0]
    assert (info["size"], info["faces"], info["layers"], info["levels"], info["mips"]) == (8, 6, 0, 4, 4)
    assert [ln for _, ln in info["level"]] == [6 * max(8 >> l, 1) ** 2 * bpt for l in range(4)]


def test_ktx2_levels_are_found_through_the_index():
    levels = [level_bytes(16, l, 8) for l in range(5)]
    for largest_first, pad in ((False, 0), (True, 0), (False, 13)):          # the specification's order, the other order, padding between levels
        data = write_ktx2(97, 16, levels, largest_first=largest_first, pad=pad)
        info = H.ktx2_parse(data)
        offs = [o for o, _ in info["level"]]
        assert offs == sorted(offs, reverse=not largest_first)              # smallest level first in the file unless asked otherwise
        for l, (o, ln) in enumerate(info["level"]):
            assert data[o:o + ln] == levels[l]


def test_ktx2_level_count_zero_means_one_level_and_a_generated_chain():
    info = H.ktx2_parse(write_ktx2(122, 16, [level_bytes(16, 0, 4)], level_count=0))
    assert info["levels"] == 1 and info["mips"] == 5
    info = H.ktx2_parse(write_ktx2(122, 5, [level_bytes(5, 0, 4)], level_count=0))
    assert info["levels"] == 1 and info["mips"] == 3                        # 5, 2, 1


def test_ktx2_rejections_carry_the_reasons():
    lv = [level_bytes(8, l, 8) for l in range(2)]
    refused(write_ktx2(97, 8, lv, faces=1), INVALID, "KTX file does not contain a cubemap")
    refused(write_ktx2(97, 8, lv, layers=2), INVALID, "KTX file contains array textures, which are not supported for cubemaps")
    refused(write_ktx2(97, 8, lv, depth=2), INVALID, "KTX file contains 3D textures, which are not supported for cubemaps")
    refused(write_ktx2(97, 8, lv, scheme=2), INVALID, "KTX file uses supercompression, which is not supported")
    refused(write_ktx2(97, 8, lv, height=4), INVALID, "Cubemap faces must be square, got 8x4")
    refused(write_ktx2(0, 8, lv), INVALID, "KTX file does not specify a format")
    refused(write_ktx2(9, 8, lv), UNSUPPORTED, "KTX file has unsupported format: vkFormat 9")                 # R8_UNORM
    assert "block-compressed" in refused(write_ktx2(145, 8, lv), UNSUPPORTED, "vkFormat 145")                 # BC7_UNORM_BLOCK
    assert "depth" in refused(write_ktx2(126, 8, lv), UNSUPPORTED, "vkFormat 126")                            # D32_SFLOAT
    refused(write_ktx2(97, 8, [lv[0], lv[1] + b"\0" * 8]), INVALID, "Level 1 byte length 776 doesn't match expected face*rows*tight_bpr 768")
    refused(write_ktx2(97, 8, [lv[0][:-8], lv[1]]), INVALID, "Level 0 byte length 3064 doesn't match expected")
    refused(write_ktx2(97, 8, [level_bytes(8, l, 8) for l in range(5)]), INVALID, "5 levels, a 8^2 cube has at most 4")
    refused(b"\0" * 12 + write_ktx2(97, 8, lv)[12:], INVALID, "not a KTX2 file")


def test_ktx2_truncation_anywhere_is_an_error_not_a_read():
    levels = [level_bytes(8, l, 8) for l in range(4)]
    data = write_ktx2(97, 8, levels)
    index_end = 80 + 24 * 4
    cuts = list(range(0, 81, 4)) + list(range(81, index_end)) + [index_end, index_end + 1, len(data) - 1]      # every header field boundary, inside the index, inside the data
    for cut in cuts:
        text = refused(data[:cut], INVALID)
        assert "truncated" in text, (cut, text)
    # a level index that points past the end, or whose offset + length wraps 64 bits
    bad = bytearray(data)
    struct.pack_into("<Q", bad, 80, len(data) - 100)
    assert "truncated" in refused(bytes(bad), INVALID)
    struct.pack_into("<2Q", bad, 80, 2 ** 64 - 8, 6 * 64 * 8)
    assert "truncated" in refused(bytes(bad), INVALID)
    bad = bytearray(data)
    struct.pack_into("<I", bad, 40, 0xFFFFFFFF)                             # levelCount
    assert "truncated" in refused(bytes(bad), INVALID)


# ------------------------------------------------------------------------------------------------ the host over a backend without the symbols

def test_host_over_the_mock_backend_loads_and_refuses_each_call(mock):
    h = H.Host(backend_path=MOCK)
    face = np.zeros((4, 4, 4), dtype=np.float16)
    calls = {
        "awsm_hip_env_cube_create": lambda: h.env_cube_create(0, 4, 3),
        "awsm_hip_env_cube_write_face": lambda: h.env_cube_update_face(0, 2, 0, face),
        "awsm_hip_env_cube_write_all_faces": lambda: h.env_cube_update_all_faces(0, 0, np.zeros((6, 4, 4, 4), dtype=np.float16)),
        "awsm_hip_env_cube_generate_mips": lambda: h.env_cube_regenerate_mipmaps(0),
        "awsm_hip_env_cube_fill_colors": lambda: h.env_cube_colors(0, 4, (0.5, 0.5, 0.5, 1.0)),
        "awsm_hip_env_cube_fill_sky_gradient": lambda: h.env_cube_sky_gradient(0, 4),
    }
    for symbol, call in calls.items():
        with pytest.raises(H.HostError) as e:
            call()
        assert e.value.code == UNSUPPORTED and symbol in str(e.value), (symbol, e.value)
    with pytest.raises(H.HostError) as e:                                   # a good file: refused at the first device call
        h.env_cube_load_ktx2(0, write_ktx2(97, 4, [level_bytes(4, l, 8) for l in range(3)]))
    assert e.value.code == UNSUPPORTED and "awsm_hip_env_cube_create" in str(e.value)
    with pytest.raises(H.HostError) as e:                                   # a bad file: the reader's reason
        h.env_cube_load_ktx2(0, write_ktx2(97, 4, [level_bytes(4, 0, 8)], faces=1))
    assert e.value.code == INVALID and "does not contain a cubemap" in str(e.value)
    h.env_cube(0, [np.zeros((6, 4, 4, 4), dtype=np.float16)])               # the entry the mock does have still works
    h.close()


# ------------------------------------------------------------------------------------------------ the fills' row tables

def color_bytes(rgba):
    """create_color (image/bitmap.rs:183-193): (clamp(c, 0, 1) * 255.0) as u8 in f64 — truncated."""
    return [int(min(max(float(c), 0.0), 1.0) * 255.0) for c in rgba]


def sky_gradient_rows(zenith, nadir, size):
    """create_vertical_gradient (image/bitmap.rs:229-267) in f64: t = y / (size - 1) (0 for size 1), a + (b - a) * t, * 255, round half away
    from zero.  -> (size, 4) uint8, row 0 = zenith."""
    rows = np.zeros((size, 4), dtype=np.uint8)
    for y in range(size):
        t = y / float(size - 1) if size > 1 else 0.0
        for ch in range(4):
            a, b = float(zenith[ch]), float(nadir[ch])
            v = min(max(a + (b - a) * t, 0.0), 1.0) * 255.0
            rows[y, ch] = int(v) + (1 if v - int(v) >= 0.5 else 0)
    return rows


def sky_gradient_level0_bytes(zenith, nadir, size):
    """(6, size, size, 4) uint8: +-X and +-Z carry the gradient, +Y is the zenith colour, -Y the nadir colour (cubemap/images.rs:112-189)."""
    out = np.zeros((6, size, size, 4), dtype=np.uint8)
    out[[0, 1, 4, 5]] = sky_gradient_rows(zenith, nadir, size)[None, :, None, :]
    out[2] = np.array(color_bytes(zenith), dtype=np.uint8)
    out[3] = np.array(color_bytes(nadir), dtype=np.uint8)
    return out


def test_fill_tables_against_hand_computed_bytes():
    # 0.4 -> 0.55 in thirds: 102, 114.75, 127.5, 140.25; 0.65 -> 0.45: 165.75, 148.75, 131.75, 114.75; 1.0 -> 0.35: 255, 199.75, 144.5, 89.25
    rows = sky_gradient_rows(hip_backend.DEFAULT_SKY_ZENITH, hip_backend.DEFAULT_SKY_NADIR, 4)
    assert rows.tolist() == [[102, 166, 255, 255], [115, 149, 200, 255], [128, 132, 145, 255], [140, 115, 89, 255]]
    assert sky_gradient_rows((0.2, 0.2, 0.2, 1.0), (0.9, 0.9, 0.9, 1.0), 1).tolist() == [[51, 51, 51, 255]]          # size 1: t = 0
    assert color_bytes((0.5, 1.0, 0.0, 1.0)) == [127, 255, 0, 255]                                              # 127.5 truncates
    assert color_bytes((-1.0, 2.0, 0.999, 0.4)) == [0, 255, 254, 102]
    lv = sky_gradient_level0_bytes(hip_backend.DEFAULT_SKY_ZENITH, hip_backend.DEFAULT_SKY_NADIR, 4)
    assert lv[2, 3, 1].tolist() == [102, 165, 255, 255] and lv[3, 0, 0].tolist() == [140, 114, 89, 255]        # the solid faces truncate
    assert lv[5, 2, 3].tolist() == [128, 132, 145, 255] and (lv[0] == lv[4]).all()


# ------------------------------------------------------------------------------------------------ the reader under the sanitizers

FUZZ_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "ktx2.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 32); }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> good;
    for (int ch; (ch = fgetc(f)) != EOF;) good.push_back((uint8_t)ch);
    fclose(f);
    char err[256];
    AwsmKtx2Info info;
    info.struct_size = sizeof info;
    if (awsm_host::ktx2::parse(good.data(), good.size(), &info, err, sizeof err) != 0) { fprintf(stderr, "the valid file was refused: %s\n", err); return 3; }
    int accepted = 0, refused = 0;
    for (int i = 0; i < 400; i++) {
        // an exactly sized heap copy, so that a read past the end is a report
        size_t len = good.size();
        if (i % 4 == 0) len = next() % (good.size() + 1);                 // truncations, many of them inside the header and the index
        if (i % 8 == 0) len = next() % 200;
        uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
        for (size_t k = 0; k < len; k++) copy[k] = good[k];
        const int flips = (int)(next() % 4);
        for (int k = 0; k < flips && len; k++) {
            const size_t at = (next() % 3) ? next() % (len < 176 ? len : 176) : next() % len;      // mostly header + index bytes
            copy[at] = (next() % 2) ? (uint8_t)next() : (uint8_t)(copy[at] ^ (1u << (next() % 8)));
        }
        info.struct_size = sizeof info;
        const int rc = awsm_host::ktx2::parse(copy, len, &info, err, sizeof err);
        if (rc == 0) {
            accepted++;
            unsigned sum = 0;                                              // what a loader would read: every accepted level lies inside the buffer
            for (uint32_t l = 0; l < info.levels; l++) for (uint64_t k = 0; k < info.level[l].length; k += 97) sum += copy[info.level[l].offset + k];
            if (sum == 0xFFFFFFFFu) puts("");
        } else refused++;
        free(copy);
    }
    printf("KTX2_FUZZ_OK accepted=%d refused=%d\n", accepted, refused);
    return refused > 100 ? 0 : 4;
}
"""


def test_ktx2_reader_under_asan_and_ubsan_as_a_program(tmp_path):
    src, exe, good = tmp_path / "ktx2_fuzz.cpp", tmp_path / "ktx2_fuzz", tmp_path / "good.ktx2"
    src.write_text(FUZZ_MAIN)
    good.write_bytes(write_ktx2(97, 8, [level_bytes(8, l, 8) for l in range(4)], pad=5))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "awsm-renderer_amd", "host"), "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe), str(good)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "KTX2_FUZZ_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
