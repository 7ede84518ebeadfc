"""CPU: the compact bin record (awsm-renderer_amd/csrc/bin_record.hpp, header-only, no HIP types): what k_bin<count> leaves per triangle for k_bin<fill> —
ok / big flags, the first tile column and local tile row of the triangle's window, the window's width - 1 and height - 1, and one bit per tile of the
window, row by row.  Driven through a small g++ program (address + undefined-behaviour sanitizers) and checked against the layout restated here from
the header's comment: every field comes back as it went in, no field reaches into another's bits, and the frame sizes the record can describe are the
ones bin_rec_fits admits."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bin_record") / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", str(exe), os.path.join(ROOT, "tests", "native", "bin_record_driver.cpp")], check=True)

    def run(lines):
        p = subprocess.run([str(exe)], input="\n".join(lines), capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        return [list(map(int, l.split())) for l in p.stdout.splitlines()]
    return run


def layout(ok, big, tx0, ty0, wm1, hm1, mask):
    """The header's comment, restated: word 0 = ok | big << 1 | (w - 1) << 2 | (h - 1) << 6 | column << 10 | row << 20, word 1 = mask."""
    return (ok | big << 1 | wm1 << 2 | hm1 << 6 | tx0 << 10 | ty0 << 20, mask)


def windows(max_tiles):
    """every window of a small triangle: w x h with w * h <= max_tiles (1x1 .. 4x4, 2x8, 1x16, 16x1, ...)"""
    return [(w, h) for w in range(1, max_tiles + 1) for h in range(1, max_tiles + 1) if w * h <= max_tiles]


def test_constants_admit_the_frames_the_renderer_supports(driver):
    (tiles, extent_bits, tile_bits, max_cols, max_rows), = driver(["k"])
    assert tiles == 16                                   # k_bin: more than 16 tiles = a big triangle, which keeps the full record
    assert (1 << extent_bits) >= tiles                   # a 1 x 16 / 16 x 1 window
    assert max_cols == max_rows == 1 << tile_bits
    assert 2 + 2 * extent_bits + 2 * tile_bits <= 32
    # the 4K frame, and the largest frame the set-up record's 15-bit pixel coordinates describe
    assert (3840 + TILE - 1) // TILE <= max_cols and (2160 + TILE - 1) // TILE <= max_rows
    assert (1 << 15) // TILE <= max_cols
    fits = driver(["f 120 68", "f %d %d" % (max_cols, max_rows), "f %d 1" % (max_cols + 1), "f 1 %d" % (max_rows + 1), "f 1 1"])
    assert [f[0] for f in fits] == [1, 1, 0, 0, 1]


def test_every_window_shape_at_the_corners_of_the_frame(driver):
    (tiles, _, _, max_cols, max_rows), = driver(["k"])
    shapes = windows(tiles)
    assert {(1, 1), (4, 4), (1, 16), (16, 1), (2, 8), (3, 5)} <= set(shapes)
    cases = []
    for (w, h) in shapes:
        full = (1 << (w * h)) - 1
        # first column / row: 0, the last window position of the 4K frame, the last the record admits
        for tx0, ty0 in ((0, 0), (120 - w, 68 - h), (max_cols - w, max_rows - h), (max_cols - 1, max_rows - 1), (max_cols - 1, 0), (0, max_rows - 1)):
            for mask in (0, full, 1, 1 << (w * h - 1), 0x5555 & full, 0xAAAA & full):
                cases.append((1, 0, tx0, ty0, w - 1, h - 1, mask))
    out = driver(["p %d %d %d %d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for c, o in zip(cases, out):
        assert tuple(o[:2]) == layout(*c), (c, o)
        assert tuple(o[2:]) == c, (c, o)


def test_flags_and_field_independence(driver):
    (_, extent_bits, tile_bits, _, _), = driver(["k"])
    ext, til = (1 << extent_bits) - 1, (1 << tile_bits) - 1
    # one field at its maximum at a time, all others zero; then all at their maxima; the four flag combinations
    cases = [(0, 0, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0),
             (0, 0, til, 0, 0, 0, 0), (0, 0, 0, til, 0, 0, 0), (0, 0, 0, 0, ext, 0, 0), (0, 0, 0, 0, 0, ext, 0), (0, 0, 0, 0, 0, 0, 0xFFFF),
             (1, 1, til, til, ext, ext, 0xFFFF)]
    cases += [(ok, big, 37, 21, 2, 3, 0x0A5F) for ok, big in itertools.product((0, 1), repeat=2)]
    out = driver(["p %d %d %d %d %d %d %d" % c for c in cases])
    for c, o in zip(cases, out):
        assert tuple(o[:2]) == layout(*c) and tuple(o[2:]) == c, (c, o)
    # the all-zero record (what the fill pass assumes for a rank past the frame's triangles) is "not ok"
    (z,) = driver(["u 0 0"])
    assert z == [0, 0, 0, 0, 0, 0, 0]
    # bits the layout does not use are ignored by unpack: word 0's top two bits, word 1's upper half
    (o,) = driver(["u %d %d" % (layout(1, 0, 5, 6, 1, 2, 0x3F)[0] | 0xC0000000, 0x3F | 0xFFFF0000)])
    assert o == [1, 0, 5, 6, 1, 2, 0x3F]
