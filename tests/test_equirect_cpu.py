"""The skybox from an equirectangular .hdr, the parts that need no GPU: the Radiance reader (host/rgbe.hpp through
awsm_host_hdr_info / awsm_host_hdr_decode) over files written by tests/rgbe_files.py, the reader as a program of its own under AddressSanitizer +
UndefinedBehaviorSanitizer, the numpy restatement (tests/equirect_reference.py) against known answers, the f32 run of the restatement against its
f64 run — where the device test's tolerance comes from — and the host over a backend without the symbol."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from tests import equirect_reference as R
from tests import rgbe_files as F
from tests.test_host_layer_cpu import MOCK, mock  # noqa: F401  (the module-scoped fixture builds the mock backend)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -6

# The f32 run of the restatement against its f64 run on the smooth cases below, relative to the reference: the largest figure is 1.84e-6 = 2^-19.05
# (64 x 32 RGBA32F into 33^2 at S = 1; test_f32_stays_within_the_slack prints it).  The device's bar is half an f16 ulp + 4 x this (DESIGN.md section 3's rule).
EQUIRECT_SLACK_REL = 2.0 ** -19

# the device test's smooth cases: panorama extent x format x cube side x S (0 = auto) x (yaw, scale, padded rows)
SMOOTH_PANOS = [(64, 32), (37, 19), (2, 1)]
SMOOTH_FORMATS = ["rgbe", "f32"]
SMOOTH_SIDES = [16, 33, 1]
SMOOTH_SAMPLES = [1, 2, 0]
SMOOTH_VARIANTS = [(0.0, 1.0, False), (0.3, 0.5, False), (-7.0, 1.0, True), (0.0, 0.5, True)]


def smooth_cases():
    return itertools.product(SMOOTH_PANOS, SMOOTH_FORMATS, SMOOTH_SIDES, SMOOTH_SAMPLES, SMOOTH_VARIANTS)


def refused(call, code, text):
    with pytest.raises(H.HostError) as e:
        call()
    assert e.value.code == code and text in str(e.value), (code, text, e.value)
    return str(e.value)


# ------------------------------------------------------------------------------------------------ the reader: round trips

@pytest.mark.parametrize("w,h", [(w, h) for w in (1, 7, 8, 37, 128) for h in (1, 5)])
def test_every_encoding_decodes_to_the_same_bytes(w, h):
    img = F.sample_image(w, h)
    encodings = ["flat", "old"] + (["rle"] if w >= 8 else [])
    for enc, flip in itertools.product(encodings, (False, True)):
        data = F.write_hdr(img, enc, flip=flip)
        got, info = H.hdr_decode(data)
        assert (got == img).all(), (enc, flip)
        assert (info["width"], info["height"], info["flipped_y"], info["rle"]) == (w, h, int(flip), int(enc == "rle")), (enc, flip, info)
        assert H.hdr_info(data) == info
    if w >= 8:                                                     # run-length coded with every run length folded, and with none
        for min_run in (1, 200):
            assert (H.hdr_decode(F.header(w, h) + b"".join(F.scan_rle(r, min_run) for r in img))[0] == img).all()


def test_the_run_length_writer_makes_a_127_run_and_a_128_literal():
    img = F.sample_image(128, 1)
    line = F.scan_rle(img[0])
    assert line[:4] == bytes([2, 2, 0, 128])
    assert line[4:8] == bytes([128 + 127, 192, 128 + 1, 192])          # the constant plane: a run of 127, then a run of one
    assert line[8] == 128 and line[9:9 + 128] == img[0, :, 1].tobytes()  # the ramp: one literal of 128
    assert (H.hdr_decode(F.header(128, 1) + line)[0] == img).all()


def test_old_runs_with_two_consecutive_run_pixels():
    img = F.sample_image(300, 2)
    img[0, 5:297] = (200, 100, 50, 130)                            # 291 repeats = 35 + (1 << 8)
    assert bytes([200, 100, 50, 130, 1, 1, 1, 35, 1, 1, 1, 1]) in F.scan_old_runs(img[0])
    data = F.write_hdr(img, "old")
    assert len(data) < len(F.write_hdr(img, "flat")) - 280 * 4
    assert (H.hdr_decode(data)[0] == img).all()
    assert (H.hdr_decode(F.write_hdr(img, "old", flip=True))[0] == img).all()


def test_seven_pixels_take_the_flat_path_even_behind_a_two_two():
    img = F.sample_image(7, 2)
    img[0, 0] = (2, 2, 0, 7)                                       # what a run-length coded line of seven pixels would start with
    data = F.header(7, 2) + F.scan_flat(img[0]) + F.scan_flat(img[1])
    got, info = H.hdr_decode(data)
    assert (got == img).all() and info["rle"] == 0


def test_plus_y_is_the_reversed_minus_y():
    img = F.sample_image(8, 5)
    body = b"".join(F.scan_rle(r) for r in img)
    down, up = H.hdr_decode(F.header(8, 5) + body)[0], H.hdr_decode(F.header(8, 5, flip=True) + body)[0]
    assert (down == img).all() and (up == img[::-1]).all()


def test_header_lines():
    img = F.sample_image(8, 1)
    extra = ["# made by a test", "EXPOSURE=2.5", "SOFTWARE=none", "EXPOSURE= 0.5", "PRIMARIES=0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329", "EXPOSURE=bright"]
    got, info = H.hdr_decode(F.write_hdr(img, "rle", extra=extra))
    assert (got == img).all() and info["exposure"] == 1.25         # reported, not applied
    assert H.hdr_decode(F.write_hdr(img, "flat", fmt=None, signature="#?RGBE"))[1]["exposure"] == 1.0      # no FORMAT line, the other signature
    assert (H.hdr_decode(F.write_hdr(img, "rle").replace(b"\n", b"\r\n", 3))[0] == img).all()              # header lines that end in CR LF


def test_float_to_rgbe_round_trip():
    rgb = np.array([[[1.0, 0.5, 0.25], [0.0, 0.0, 0.0], [1000.0, 1.0, 0.0], [3e-5, 2e-5, 1e-5]]])
    q = F.float_to_rgbe(rgb)
    assert q[0, 0].tolist() == [128, 64, 32, 129] and q[0, 1].tolist() == [0, 0, 0, 0] and q[0, 2].tolist() == [250, 0, 0, 138]
    back = F.rgbe_to_float(q)
    assert (back <= rgb).all() and (rgb - back <= rgb.max(axis=-1, keepdims=True) / 128.0).all()      # truncated to 8 bits of the largest channel
    assert (R.decode(q) == back).all() and (R.decode(q, np.float32).astype(np.float64) == back).all()


# ------------------------------------------------------------------------------------------------ the reader: rejections

def test_rejections_carry_the_code_and_the_reason():
    img = F.sample_image(8, 3)
    good = F.write_hdr(img, "rle")
    head = F.header(8, 3)
    refused(lambda: H.hdr_info(b"P6\n8 3\n255\n" + b"\0" * 72), INVALID, "not a Radiance picture")
    refused(lambda: H.hdr_info(b""), INVALID, "not a Radiance picture")
    refused(lambda: H.hdr_info(F.header(8, 3, fmt="32-bit_rle_xyze")), UNSUPPORTED, "32-bit_rle_xyze")
    refused(lambda: H.hdr_info(F.header(8, 3, resolution="+X 8 -Y 3")), UNSUPPORTED, "+X 8 -Y 3")
    refused(lambda: H.hdr_info(F.header(8, 3, resolution="-Y 3 -X 8")), UNSUPPORTED, "-Y 3 -X 8")
    refused(lambda: H.hdr_info(F.header(8, 3, resolution="8 by 3")), INVALID, "bad resolution line")
    refused(lambda: H.hdr_info(F.header(0, 3)), INVALID, "0 x 3 pixels")
    refused(lambda: H.hdr_info(F.header(8, 32769)), INVALID, "8 x 32769 pixels")
    refused(lambda: H.hdr_info(F.header(32768, 16384)), INVALID, "at most 2^28")
    refused(lambda: H.hdr_info(good[:30]), INVALID, "truncated")
    assert H.hdr_info(F.header(16384, 16384))["width"] == 16384           # 2^28 itself is inside
    # scanlines
    lines = [F.scan_rle(r) for r in img]
    refused(lambda: H.hdr_decode(head + lines[0] + lines[1][:-3]), INVALID, "scanline 1 is truncated")
    refused(lambda: H.hdr_decode(head + lines[0] + lines[1]), INVALID, "scanline 2 is truncated")
    refused(lambda: H.hdr_decode(head + F.scan_flat(img[0]) + F.scan_flat(img[1])[:-1]), INVALID, "scanline 1 is truncated")
    refused(lambda: H.hdr_decode(head + bytes([2, 2, 0, 8, 0])), INVALID, "scanline 0 has a zero count")
    refused(lambda: H.hdr_decode(head + bytes([2, 2, 0, 8, 128 + 5, 7, 128 + 4, 7]) + b"\0" * 64), INVALID, "scanline 0 has a run over the scanline end")
    refused(lambda: H.hdr_decode(head + bytes([2, 2, 0, 8, 5, 1, 2, 3, 4, 5, 4, 1, 2, 3, 4]) + b"\0" * 64), INVALID, "scanline 0 has a run over the scanline end")
    refused(lambda: H.hdr_decode(head + bytes([1, 1, 1, 3]) + F.scan_flat(img[0])), INVALID, "run pixel before any pixel")
    refused(lambda: H.hdr_decode(head + F.scan_flat(img[0][:4]) + bytes([1, 1, 1, 5]) + b"\0" * 64), INVALID, "scanline 0 has a run over the scanline end")
    refused(lambda: H.hdr_decode(head + F.scan_flat(img[0][:4]) + bytes([1, 1, 1, 1, 1, 1, 1, 1]) + b"\0" * 64), INVALID, "scanline 0 has a run over the scanline end")      # 1 + (1 << 8)
    refused(lambda: H.hdr_decode(good, out_cap=8 * 3 * 4 - 1), INVALID, "out_cap 95")
    assert (H.hdr_decode(good, out_cap=8 * 3 * 4 + 5)[0] == img).all()


# ------------------------------------------------------------------------------------------------ the reader under the sanitizers

FUZZ_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "rgbe.hpp"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 32); }

int main(int argc, char** argv) {
    int accepted = 0, refused = 0;
    for (int file = 1; file < argc; file++) {
        FILE* f = fopen(argv[file], "rb");
        if (!f) return 2;
        std::vector<uint8_t> good;
        for (int ch; (ch = fgetc(f)) != EOF;) good.push_back((uint8_t)ch);
        fclose(f);
        char err[256];
        AwsmHdrInfo info;
        info.struct_size = sizeof info;
        if (awsm_host::rgbe::info(good.data(), good.size(), &info, err, sizeof err) != 0) { fprintf(stderr, "the valid file %s was refused: %s\n", argv[file], err); return 3; }
        const size_t header = good.size() > 60 ? 60 : good.size();
        for (int i = 0; i < 400; i++) {
            // exactly sized heap copies of the input and of the output, so that a read or a write past either end is a report
            size_t len = good.size();
            if (i % 4 == 0) len = next() % (good.size() + 1);                 // truncations, in the header and in the scanlines
            uint8_t* copy = (uint8_t*)malloc(len ? len : 1);
            for (size_t k = 0; k < len; k++) copy[k] = good[k];
            const int flips = (int)(next() % 4);
            for (int k = 0; k < flips && len; k++) {
                const size_t at = (next() % 3 == 0) ? next() % (len < header ? len : header) : next() % len;      // a third of them in the header
                copy[at] = (next() % 2) ? (uint8_t)next() : (uint8_t)(copy[at] ^ (1u << (next() % 8)));
            }
            info.struct_size = sizeof info;
            int rc = awsm_host::rgbe::info(copy, len, &info, err, sizeof err);
            if (rc == 0) {
                size_t cap = (size_t)info.width * info.height * 4u;
                if (cap > (64u << 20)) cap = 64u << 20;                         // a mutated extent: the reader must refuse the smaller buffer, not overrun it
                if (i % 16 == 1 && cap) cap -= 1;
                uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
                rc = awsm_host::rgbe::decode(copy, len, out, cap, &info, err, sizeof err);
                unsigned sum = 0;
                if (rc == 0) for (size_t k = 0; k < (size_t)info.width * info.height * 4u; k += 13) sum += out[k];      // every decoded byte was written
                if (sum == 0xFFFFFFFFu) puts("");
                free(out);
            }
            if (rc == 0) accepted++; else refused++;
            free(copy);
        }
    }
    printf("RGBE_FUZZ_OK accepted=%d refused=%d\n", accepted, refused);
    return accepted > 50 && refused > 100 ? 0 : 4;
}
"""


def test_reader_under_asan_and_ubsan_as_a_program(tmp_path):
    src, exe = tmp_path / "rgbe_fuzz.cpp", tmp_path / "rgbe_fuzz"
    src.write_text(FUZZ_MAIN)
    img = F.sample_image(37, 5)
    files = []
    for enc, flip in (("flat", False), ("old", True), ("rle", False), ("rle", True)):
        p = tmp_path / ("good_%s_%d.hdr" % (enc, flip))
        p.write_bytes(F.write_hdr(img, enc, flip=flip, extra=["EXPOSURE=2.0"]))
        files.append(str(p))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "awsm-renderer_amd", "host"), "-o", str(exe), str(src)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)] + files, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "RGBE_FUZZ_OK" in p.stdout, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ the restatement: known answers

def central_quarter(n):
    """The texels that lie wholly inside |s|, |t| <= 0.5."""
    q = -(-n // 4)
    return slice(q, n - q)


@pytest.mark.parametrize("n,samples", [(16, 1), (8, 2), (33, 1)])
def test_axis_painted_panorama_gives_each_face_its_colour(n, samples):
    """Forward (-Z at the centre column), right (+X at u = 0.75), up (row 0 the zenith) and no mirroring: a face's central quarter looks only at
    pixels whose dominant axis is the face's, so it holds that axis's colour — computed here from the contract's formulas alone."""
    pano = R.axis_painted(64, 32)
    # the contract's own anchors, in f64: the centre column looks along -Z, u = 0.75 along +X, row 0 up
    for d, (u, v) in {(0.0, 0.0, -1.0): (0.5, 0.5), (1.0, 0.0, 0.0): (0.75, 0.5), (-1.0, 0.0, 0.0): (0.25, 0.5), (0.0, 1.0, 0.0): (None, 0.0), (0.0, -1.0, 0.0): (None, 1.0)}.items():
        gu, gv = R.direction_to_uv(tuple(np.float64(c) for c in d))
        assert abs(gv - v) < 1e-15 and (u is None or abs(gu - u) < 1e-15), (d, gu, gv)
    assert np.allclose(R.direction_to_uv((np.float64(0.0), np.float64(0.0), np.float64(1.0)))[0] % 1.0, 0.0)      # +Z sits on the seam u = 0 / 1
    out = R.project(pano, n, samples)
    q = central_quarter(n)
    for face in range(6):
        assert (out[face, q, q] == R.AXIS_COLORS[face]).all(), face
    # (a mirrored panorama would put -X's colour on the +X face: the six colours are all different)
    assert len({tuple(c) for c in R.AXIS_COLORS}) == 6


def test_uniform_panorama_gives_that_value_everywhere():
    for fmt_value in (np.array([18, 200, 255, 131], dtype=np.uint8), np.array([0.375, 2.5, 1e-3, 9.0], dtype=np.float32)):
        pano = np.broadcast_to(fmt_value, (5, 9, 4)).copy()
        want = R.decode(pano)[0, 0]
        for n, samples in ((1, 1), (5, 3), (16, 0)):
            out = R.project(pano, n, samples, yaw=1.0)
            assert np.abs(out / want - 1.0).max() < 1e-15
            assert (R.f16_bits(out)[..., :3] == want.astype(np.float16).view(np.uint16)).all() and (R.f16_bits(out)[..., 3] == R.HALF_ONE).all()


def test_yaw_of_a_quarter_turn_is_a_roll_by_a_quarter_of_the_width():
    pano = R.smooth_panorama(64, 32, "f32")
    a = R.project(pano, 9, 2, yaw=math.pi / 2)
    b = R.project(np.roll(pano, -16, axis=1), 9, 2)                # u grows by 1/4: the lookup lands 16 columns further right
    assert np.abs(a - b).max() < 5e-6                              # yaw crosses the ABI as an f32: pi / 2 is 4.4e-8 off, 4.5e-7 of a pixel
    c = R.project(pano, 9, 2, yaw=math.pi / 2 - 8 * math.pi)       # whole turns change nothing
    assert np.abs(a - c).max() < 5e-5


def test_a_source_linear_in_height_comes_back_within_its_bilinear_error():
    """a + b d.y rendered into the panorama at the pixel centres: along a row the source is constant, down a column it is a + b cos(pi v), which
    linear interpolation between rows pi / H apart misses by at most b (pi / H)^2 / 8; above the first and below the last row centre the lookup
    clamps, which costs at most b (1 - cos(pi / 2H))."""
    a0, b0, w, h = 1.5, 0.75, 64, 32
    pano = np.ones((h, w, 4), dtype=np.float32)
    pano[..., :3] = (a0 + b0 * R.pixel_dirs(w, h)[..., 1])[..., None]
    n = 12
    out = R.project(pano, n, 1)
    j, i = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
    bound = b0 * max((math.pi / h) ** 2 / 8.0, 1.0 - math.cos(math.pi / (2 * h))) + 1e-6      # + the f32 storage of the panorama
    for face in range(6):
        dx, dy, dz = R.face_dir(face, 2.0 * i / n - 1.0, 2.0 * j / n - 1.0)
        want = a0 + b0 * dy / np.sqrt(dx * dx + dy * dy + dz * dz)
        assert np.abs(out[face, ..., 0] - want).max() <= bound, (face, np.abs(out[face, ..., 0] - want).max(), bound)
    assert np.abs(out[2, ..., 0] - (a0 + b0)).max() > 1e-4         # the bound is not vacuous: the faces differ from a constant


# ------------------------------------------------------------------------------------------------ where the device's tolerance comes from

def test_f32_stays_within_the_slack():
    """Every smooth case of the device test, run through the restatement in f32 and in f64: the two differ by at most EQUIRECT_SLACK_REL of the
    reference, before the store's rounding.  The device test allows four times that on top of the half ulp of the store."""
    worst, where = 0.0, None
    panos = {(w, h, fmt): R.smooth_panorama(w, h, fmt) for (w, h) in SMOOTH_PANOS for fmt in SMOOTH_FORMATS}
    src = np.concatenate([R.smooth_radiance(R.pixel_dirs(w, h)).reshape(-1) for (w, h) in SMOOTH_PANOS])
    assert 0.05 <= src.min() and src.max() <= 10.0 and src.max() > 5.0, (src.min(), src.max())      # the source is what the issue asks for
    for (w, h), fmt, n, samples, (yaw, scale, _) in smooth_cases():
        pano = panos[(w, h, fmt)]
        ref, f32 = R.project(pano, n, samples, yaw, scale), R.project(pano, n, samples, yaw, scale, np.float32)
        assert f32.dtype == np.float32
        rel = float((np.abs(f32.astype(np.float64) - ref) / np.abs(ref)).max())
        if rel > worst:
            worst, where = rel, (w, h, fmt, n, samples, yaw, scale)
    print("f32 against f64, largest relative difference: %.3g = 2^%.2f at %s (EQUIRECT_SLACK_REL: %.3g)" % (worst, math.log2(worst), where, EQUIRECT_SLACK_REL))
    assert worst <= EQUIRECT_SLACK_REL, (worst, where)
    assert worst > EQUIRECT_SLACK_REL / 4.0, worst                 # ... and the constant is not slack of its own


# ------------------------------------------------------------------------------------------------ the host over a backend without the symbol

def test_host_over_the_mock_backend_refuses_the_projection(mock):
    h = H.Host(backend_path=MOCK)
    pano = R.smooth_panorama(8, 4, "rgbe")
    with pytest.raises(H.HostError) as e:
        h.env_cube_from_equirect(0, pano)
    assert e.value.code == UNSUPPORTED and "awsm_hip_env_cube_from_equirect" in str(e.value), e.value
    with pytest.raises(H.HostError) as e:                          # a good file: refused at the first device call
        h.env_cube_load_hdr(0, F.write_hdr(pano, "rle"), 8)
    assert e.value.code == UNSUPPORTED and "awsm_hip_env_cube_create" in str(e.value), e.value
    with pytest.raises(H.HostError) as e:                          # a bad file: the reader's reason
        h.env_cube_load_hdr(0, F.header(8, 4, fmt="32-bit_rle_xyze"), 8)
    assert e.value.code == UNSUPPORTED and "32-bit_rle_xyze" in str(e.value), e.value
    with pytest.raises(TypeError):
        h.env_cube_from_equirect(0, np.zeros((4, 8, 3), dtype=np.float32))
    h.close()
