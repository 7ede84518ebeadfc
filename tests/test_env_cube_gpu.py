"""Environment cubes at run time on the device (awsm_hip_env_cube_create / _write_face / _write_all_faces / _generate_mips / _fill_colors /
_fill_sky_gradient, and the KTX2 loader through the host): every stored texel against the numpy restatements below of DESIGN.md §12 — the
format conversions (one rounding to f16, nearest even) and the 2x2 mip filter — bit for bit (f16 compared as uint16, no NaN among the inputs);
rendered frames against frames of a fresh context that received the same final chain through awsm_hip_env_cube_upload."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend, scenes
from awsm_renderer_amd import host as H
from awsm_renderer_amd.hip_backend import AwsmCubeLayout, AwsmHipError, HipDevice
from tests import helpers
from tests.test_env_cube_cpu import color_bytes, sky_gradient_level0_bytes, write_ktx2

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, UNSUPPORTED, OUT_OF_RANGE = -1, -5, -6, -7
HALF_ONE = 0x3C00


# ------------------------------------------------------------------------------------------------ numpy restatements

UNORM = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float16)
SRGB = np.array([u / 12.92 if u <= 0.04045 else math.pow((u + 0.055) / 1.055, 2.4) for u in (q / 255.0 for q in range(256))], dtype=np.float64).astype(np.float16)


def full_mips(n):
    return int(n).bit_length()


def small_ufloat(v, mant_bits):
    """An unsigned float with a 5-bit exponent (bias 15) and mant_bits of mantissa, by VALUE (Vulkan's B10G11R11 fields): zero, denormals, inf."""
    e, m = (v >> mant_bits).astype(np.int64), (v & ((1 << mant_bits) - 1)).astype(np.float64)
    frac = m / float(1 << mant_bits)
    val = np.where(e == 0, frac * 2.0 ** -14, (1.0 + frac) * np.exp2((e - 15).astype(np.float64)))
    return np.where(e == 31, np.inf, val)            # the inputs carry no NaN (mantissa 0 wherever e == 31)


def to_f16_bits(fmt, data):
    """Source texels (..., 4) of the format's element type — or (...) uint32 for the packed formats — to (..., 4) f16 bits."""
    with np.errstate(over="ignore"):
        if fmt == "rgba16f":
            return np.ascontiguousarray(data).view(np.uint16).copy()
        if fmt == "rgba32f":
            return data.astype(np.float16).view(np.uint16)
        if fmt in ("rgba8unorm", "rgba8unorm-srgb", "bgra8unorm", "bgra8unorm-srgb"):
            colour = SRGB if fmt.endswith("srgb") else UNORM
            d = data[..., [2, 1, 0, 3]] if fmt.startswith("bgra") else data
            return np.stack([colour[d[..., 0]], colour[d[..., 1]], colour[d[..., 2]], UNORM[d[..., 3]]], axis=-1).view(np.uint16)
        if fmt == "rg11b10ufloat":
            rgb = [small_ufloat(data & 0x7FF, 6), small_ufloat((data >> 11) & 0x7FF, 6), small_ufloat(data >> 22, 5)]
        else:                                        # rgb9e5ufloat: m * 2^(e - 24)
            scale = np.exp2((data >> 27).astype(np.float64) - 24.0)
            rgb = [(data & 0x1FF) * scale, ((data >> 9) & 0x1FF) * scale, ((data >> 18) & 0x1FF) * scale]
        out = np.stack([c.astype(np.float16).view(np.uint16) for c in rgb] + [np.full(data.shape, HALF_ONE, dtype=np.uint16)], axis=-1)
        for c, b in zip(rgb, np.moveaxis(out, -1, 0)):
            assert (b.view(np.float16).astype(np.float64) == c).all()      # "every value is exactly representable in f16"
        return out


def mip_chain(level0_bits, mips):
    """filter_simple per channel in f32: +0.0, + s(2x, 2y), + s(2x+1, 2y), + s(2x, 2y+1), + s(2x+1, 2y+1), * 0.25, round to f16; each level from the
    stored level above; for an odd side the last row and column are never read."""
    chain = [np.ascontiguousarray(level0_bits)]
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(1, mips):
            s = chain[-1].view(np.float16).astype(np.float32)
            d = max(s.shape[1] >> 1, 1)
            acc = np.zeros((6, d, d, 4), dtype=np.float32)
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                acc = acc + s[:, dy:2 * d:2, dx:2 * d:2]
            chain.append((acc * np.float32(0.25)).astype(np.float16).view(np.uint16))
    return chain


def random_f16_bits(rng, shape):
    """Random f16 bit patterns over the whole range — denormals, both zeros, both signs — without NaN or infinity."""
    b = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    return np.where((b & 0x7C00) == 0x7C00, b & 0x83FF, b).astype(np.uint16)


def read_chain(dev, which):
    size, mips = dev.env_cube_info(which)
    return [dev.env_cube_read_level(which, l).view(np.uint16) for l in range(mips)]


def assert_chain(got, want, what):
    assert len(got) == len(want), what
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and (g == w).all(), (what, "level", l, int((g != w).sum()), "texel components differ")


@pytest.fixture(scope="module")
def dev():
    d = HipDevice(parity_tap=True)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ 1. the mip chain

@pytest.mark.parametrize("size", [1, 2, 3, 5, 33, 48, 64, 96])
def test_mip_chain_every_level_bit_for_bit(dev, size):
    """A single texel, odd sides whose last row is never read, partial tiles, whole tiles, and chains that need two launches (64: 6 levels below
    level 0, 96: 96 48 24 12 6 3 1)."""
    rng = np.random.default_rng(1000 + size)
    lv0 = random_f16_bits(rng, (6, size, size, 4))
    lv0[1].reshape(-1)[::7] = 0x7C00                     # +inf on one face, -inf on another: an infinity never meets its opposite, so no NaN
    lv0[2].reshape(-1)[::5] = 0xFC00
    lv0[3] = 0x8000                                      # a face of -0.0 must come out +0.0: the sum starts from +0.0
    mips = full_mips(size)
    dev.env_cube_create(1, size, mips)
    dev.env_cube_write_all_faces(1, 0, lv0.view(np.float16))
    dev.env_cube_generate_mips(1)
    want = mip_chain(lv0, mips)
    assert_chain(read_chain(dev, 1), want, "size %d" % size)
    if mips > 1:
        assert (want[1][3] == 0).all() and (want[1][1] == 0x7C00).any()
    # a chain shorter than the full one stops where it was told to
    if mips > 2:
        dev.env_cube_create(1, size, 2)
        dev.env_cube_write_all_faces(1, 0, lv0.view(np.float16))
        dev.env_cube_generate_mips(1)
        assert_chain(read_chain(dev, 1), want[:2], "size %d, two levels" % size)


# ------------------------------------------------------------------------------------------------ 2. the formats

def source_texels(fmt, rng, shape):
    """Texels of `fmt` in the array form the binding takes: shape + (4,) of the element type, or shape of uint32 for the packed formats."""
    n = int(np.prod(shape))
    if fmt == "rgba16f":
        return random_f16_bits(rng, shape + (4,)).view(np.float16)
    if fmt == "rgba32f":
        special = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.99, 65520.0, 1e9, -1e9, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                            2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 1e-30, -1e-30, 0.1, -0.3, 1000.123, np.inf, -np.inf], dtype=np.float32)
        v = (rng.standard_normal(n * 4) * np.exp2(rng.integers(-30, 18, size=n * 4))).astype(np.float32)
        v[:len(special)] = special
        return rng.permutation(v).reshape(shape + (4,))
    if "8unorm" in fmt:      # every channel sees all 256 codes (n >= 256 texels)
        i = np.arange(n)
        return np.stack([(i * 7 + 64 * c) % 256 for c in range(4)], axis=-1).astype(np.uint8).reshape(shape + (4,))
    w = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    if fmt == "rg11b10ufloat":                       # exponent 31 -> infinity only: no NaN
        for shift, mant in ((0, 6), (11, 6), (22, 5)):
            is_max = ((w >> (shift + mant)) & 31) == 31
            w = np.where(is_max, w & ~np.uint32(((1 << mant) - 1) << shift), w).astype(np.uint32)
        w[:4] = [0, 0xFFFFFFFF & ~((63 << 0) | (63 << 11) | (31 << 22)), 1 | (1 << 11) | (1 << 22), (31 << 6) | (30 << 17) | (1 << 27)]
    else:
        w[:3] = [0, 0xFFFFFFFF, 1 | (1 << 9) | (1 << 18)]
    return w.reshape(shape)


@pytest.mark.parametrize("fmt", sorted(hip_backend.CUBE_FORMATS))
def test_formats_tight_and_padded_layouts(dev, fmt):
    """Level 1 (8^2) of a 16^2 cube: all six faces from a tight buffer, then one face from a padded one (bytes_per_row 256, rows_per_image 11,
    offset 24), then one from a layout no load wider than a byte can follow; nothing outside the written face and level changes."""
    rng = np.random.default_rng(sorted(hip_backend.CUBE_FORMATS).index(fmt))
    bpt = hip_backend.CUBE_FORMATS[fmt][1]
    base = [random_f16_bits(rng, (6, 16 >> l, 16 >> l, 4)) for l in range(5)]
    dev.env_cube_upload(0, [b.view(np.float16) for b in base])
    src = source_texels(fmt, rng, (6, 8, 8))
    dev.env_cube_write_all_faces(0, 1, src, fmt=fmt)
    want = [b.copy() for b in base]
    want[1] = to_f16_bits(fmt, src)
    assert_chain(read_chain(dev, 0), want, fmt + " all faces")

    face_src = source_texels(fmt, np.random.default_rng(77), (1, 16, 16))[0, :8, :8]
    for bytes_per_row, rows_per_image, offset, face in ((256, 11, 24, 3), (8 * bpt + 3, 8, 5, 5)):
        raw = rng.integers(0, 256, size=offset + bytes_per_row * rows_per_image, dtype=np.uint8)
        rows = np.ascontiguousarray(face_src).view(np.uint8).reshape(8, 8 * bpt)
        for y in range(8):
            raw[offset + y * bytes_per_row: offset + y * bytes_per_row + 8 * bpt] = rows[y]
        dev.env_cube_write_face(0, face, 1, raw.tobytes(), fmt=fmt, width=8, height=8, bytes_per_row=bytes_per_row, rows_per_image=rows_per_image, offset=offset)
        want[1][face] = to_f16_bits(fmt, face_src)
        assert_chain(read_chain(dev, 0), want, "%s face %d, bytes_per_row %d" % (fmt, face, bytes_per_row))


def test_eight_bit_tables_are_the_restated_ones(dev):
    """The 256 codes of every channel, UNORM and sRGB, RGBA and BGRA, straight against q / 255 and the sRGB decode in double precision rounded once."""
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    face = np.stack([codes, codes[::-1], codes.T, codes.T[::-1]], axis=-1)
    dev.env_cube_create(2, 16, 1)
    for fmt in ("rgba8unorm", "rgba8unorm-srgb", "bgra8unorm", "bgra8unorm-srgb"):
        dev.env_cube_write_face(2, 4, 0, face, fmt=fmt)
        got = dev.env_cube_read_level(2, 0)
        colour = SRGB if fmt.endswith("srgb") else UNORM
        r, b = (2, 0) if fmt.startswith("bgra") else (0, 2)
        assert (got[4, ..., 0].view(np.uint16) == colour[face[..., r]].view(np.uint16)).all(), fmt
        assert (got[4, ..., 1].view(np.uint16) == colour[face[..., 1]].view(np.uint16)).all(), fmt
        assert (got[4, ..., 2].view(np.uint16) == colour[face[..., b]].view(np.uint16)).all(), fmt
        assert (got[4, ..., 3].view(np.uint16) == UNORM[face[..., 3]].view(np.uint16)).all(), fmt      # alpha is never sRGB
        assert (got[[0, 1, 2, 3, 5]].view(np.uint16) == 0).all()
    assert float(SRGB[255]) == 1.0 and float(SRGB[0]) == 0.0 and abs(float(SRGB[128]) - 0.2158) < 1e-3


def test_a_source_too_large_for_the_staging_ring_is_copied_from_the_callers_memory(dev):
    """Above 4 MiB the write copies from the caller's pointer and waits for that copy: 256^2 x 6 RGBA32F is 6 MiB."""
    rng = np.random.default_rng(5)
    src = (rng.standard_normal((6, 256, 256, 4)) * 8.0).astype(np.float32)
    dev.env_cube_create(2, 256, 1)
    dev.env_cube_write_all_faces(2, 0, src, fmt="rgba32f")
    src[:] = 0.0                                         # the pointer is not retained
    got = dev.env_cube_read_level(2, 0)
    want = (np.random.default_rng(5).standard_normal((6, 256, 256, 4)) * 8.0).astype(np.float32).astype(np.float16)
    assert (got.view(np.uint16) == want.view(np.uint16)).all()


# ------------------------------------------------------------------------------------------------ 3. the apron / 4. overlap: rendered frames

def _sky_scene(direction):
    sc = scenes.box_scene(64, 64)
    eye = tuple(10.0 * c for c in direction)              # the box lies behind the camera: nothing but sky in the frame
    sc.view = scenes.look_at_rh(eye, tuple(11.0 * c for c in direction))
    sc.proj = scenes.perspective_rh(math.radians(100.0), 1.0, 0.1, 100.0)
    sc.camera_position = eye
    return sc


def _sphere_scene(size=64, mips=3, **kw):
    sc = scenes.helmet_scene(size, size, segments=kw.get("segments", 16), rings=kw.get("rings", 12), tex_size=16)
    sc.prefiltered_mip_count, sc.irradiance_mip_count = mips, 1
    return sc


def _cubes(rng, size, mips):
    """Three random HDR chains (finite, positive: colours), as uint16 bits."""
    def chain():
        return [(rng.uniform(0.0, 4.0, size=(6, max(size >> l, 1), max(size >> l, 1), 4))).astype(np.float16).view(np.uint16) for l in range(mips)]
    return {name: chain() for name in ("skybox", "prefiltered", "irradiance")}


def _as_env(cubes):
    return {k: [lv.view(np.float16) for lv in v] for k, v in cubes.items()}


def _frames(device, lut, views):
    """The opaque image of every (scene, has_opaque) in `views` on a device whose cubes are already in place (the scenes carry none)."""
    out = []
    for sc, has_opaque in views:
        helpers.hip_frame(helpers.build_model(sc), lut, has_opaque=has_opaque, dev=device)
        out.append(device.read_opaque())
    return out


def test_a_face_write_refreshes_the_neighbours_aprons(oracle_lut):
    """One face of a 5^2 cube (and one of its 2^2 level) is written in place; frames rendered afterwards equal, bit for bit, the frames of a fresh
    context that got the same final chain through awsm_hip_env_cube_upload — the same kernels on the same texels, aprons included: a stale apron
    of a neighbouring face shows along the cube's edges, which is where the three sky cameras look, and in the sphere's IBL."""
    rng = np.random.default_rng(31)
    before = _cubes(rng, 5, 3)
    after = {k: [lv.copy() for lv in v] for k, v in before.items()}
    writes = []
    for name in before:
        for face, level in ((2, 0), (4, 1), (1, 0)):
            n = 5 >> level
            texels = rng.uniform(0.0, 6.0, size=(n, n, 4)).astype(np.float16)
            after[name][level][face] = texels.view(np.uint16)
            writes.append((hip_backend_slot(name), face, level, texels))
    views = [(_sky_scene(d), False) for d in ((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.02, -1.0))] + [(_sphere_scene(), True)]

    first = dataclasses.replace(views[0][0], env_cubes=_as_env(before))
    a, _ = helpers.hip_frame(helpers.build_model(first), oracle_lut, has_opaque=False)
    stale = a.read_opaque()
    for which, face, level, texels in writes:
        a.env_cube_write_face(which, face, level, texels)
    assert_chain(read_chain(a, 0), after["skybox"], "skybox after the writes")
    got = _frames(a, oracle_lut, views)
    a.close()

    final = dataclasses.replace(views[0][0], env_cubes=_as_env(after))
    b, _ = helpers.hip_frame(helpers.build_model(final), oracle_lut, has_opaque=False)
    want = _frames(b, oracle_lut, views)
    b.close()
    assert (got[0] != stale).any()                       # the writes are visible at all
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g == w).all(), ("view", i, int((g != w).any(axis=-1).sum()), "pixels differ")
    assert len({g.tobytes() for g in got}) == len(got)   # four different pictures


def hip_backend_slot(name):
    return ("skybox", "prefiltered", "irradiance").index(name)


def test_overlapped_frames_keep_their_texels(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES: frame A is submitted, then all three cubes are rewritten and their chains regenerated, then frame B.  A is the
    frame of a context that was never written, B the frame of a context uploaded with the new chain."""
    rng = np.random.default_rng(47)
    size, mips = 16, 5
    old = _cubes(rng, size, mips)
    new0 = {k: rng.uniform(0.0, 5.0, size=(6, size, size, 4)).astype(np.float16).view(np.uint16) for k in old}
    new = {k: mip_chain(v, mips) for k, v in new0.items()}
    sc = _sphere_scene(160, mips, segments=48, rings=36)
    model = helpers.build_model(dataclasses.replace(sc, env_cubes=_as_env(old)))
    draws = model.collect_draws()

    def frame(device):
        device.geometry_pass(draws)
        device.opaque_pass()

    d = HipDevice(parity_tap=True, overlap_frames=True)
    helpers.hip_frame(model, oracle_lut, dev=d)
    frame(d)                                                                # A
    for k, name in enumerate(("skybox", "prefiltered", "irradiance")):
        d.env_cube_write_all_faces(k, 0, new0[name].view(np.float16))
        d.env_cube_generate_mips(k)
    got_a = d.read_opaque()
    frame(d)                                                                # B
    d.frame_end()
    got_b = d.read_opaque()
    d.close()

    ref = HipDevice(parity_tap=True, overlap_frames=True)
    helpers.hip_frame(model, oracle_lut, dev=ref)
    frame(ref); ref.frame_end()
    want_a = ref.read_opaque()
    ref.close()
    ref = HipDevice(parity_tap=True, overlap_frames=True)
    helpers.hip_frame(helpers.build_model(dataclasses.replace(sc, env_cubes=_as_env(new))), oracle_lut, dev=ref)
    frame(ref); ref.frame_end()
    want_b = ref.read_opaque()
    ref.close()
    assert (got_a == want_a).all(), int((got_a != want_a).any(axis=-1).sum())
    assert (got_b == want_b).all(), int((got_b != want_b).any(axis=-1).sum())
    assert (want_a != want_b).any()


# ------------------------------------------------------------------------------------------------ 5. the fills

@pytest.mark.parametrize("size", [4, 256])
def test_fills_every_level(dev, size):
    mips = full_mips(size)
    six = [(0.5, 1.0, 0.0, 1.0), (0.25, 0.2, 0.9, 0.5), (1.5, -0.5, 0.999, 1.0), (0.1, 0.7, 0.3, 0.0), (0.8, 0.8, 0.8, 1.0), (0.05, 0.4, 0.65, 0.75)]
    dev.env_cube_fill_colors(0, size, six)
    lv0 = np.zeros((6, size, size, 4), dtype=np.uint8)
    for f in range(6):
        lv0[f] = np.array(color_bytes(six[f]), dtype=np.uint8)
    assert_chain(read_chain(dev, 0), mip_chain(to_f16_bits("rgba8unorm", lv0), mips), "six colours at %d" % size)
    assert lv0[0, 0, 0].tolist() == [127, 255, 0, 255]
    dev.env_cube_fill_colors(0, size, (0.5, 0.5, 0.5, 1.0))                 # one colour for all faces
    assert (dev.env_cube_read_level(0, mips - 1).view(np.uint16) == UNORM[[127, 127, 127, 255]].view(np.uint16)).all()

    for zenith, nadir in ((hip_backend.DEFAULT_SKY_ZENITH, hip_backend.DEFAULT_SKY_NADIR), ((0.1, 0.2, 0.9, 1.0), (0.9, 0.6, 0.3, 0.25))):
        dev.env_cube_fill_sky_gradient(1, size, zenith, nadir)
        assert dev.env_cube_info(1) == (size, mips)
        lv0 = sky_gradient_level0_bytes(zenith, nadir, size)
        assert_chain(read_chain(dev, 1), mip_chain(to_f16_bits("rgba8unorm", lv0), mips), "gradient at %d" % size)
    dev.env_cube_fill_sky_gradient(1, size)                                 # the defaults are CubemapSkyGradient::default
    assert (dev.env_cube_read_level(1, 0).view(np.uint16) ==
            to_f16_bits("rgba8unorm", sky_gradient_level0_bytes(hip_backend.DEFAULT_SKY_ZENITH, hip_backend.DEFAULT_SKY_NADIR, size))).all()


# ------------------------------------------------------------------------------------------------ 6. KTX2 end to end

def test_ktx2_files_through_the_host(tmp_path):
    rng = np.random.default_rng(61)
    h = H.Host(parity_tap=True)
    d = HipDevice.from_ctx(h.device_ctx, 0, 0)
    # RGBA16F with its own five levels, stored smallest first, read from a path
    levels = [random_f16_bits(rng, (6, 16 >> l, 16 >> l, 4)) for l in range(5)]
    path = tmp_path / "env.ktx2"
    path.write_bytes(write_ktx2(97, 16, [lv.tobytes() for lv in levels], pad=3))
    info = h.env_cube_load_ktx2(1, str(path))
    assert (info["size"], info["levels"], info["mips"], info["format_name"]) == (16, 5, 5, "rgba16f")
    assert_chain(read_chain(d, 1), levels, "rgba16f file")
    # B10G11R11 with levelCount 0: one stored level, the chain made on the device; from memory
    src = source_texels("rg11b10ufloat", rng, (6, 16, 16))
    info = h.env_cube_load_ktx2(0, write_ktx2(122, 16, [src.tobytes()], level_count=0))      # unsigned values: an infinity meets no opposite
    assert (info["levels"], info["mips"], info["format_name"]) == (1, 5, "rg11b10ufloat")
    assert_chain(read_chain(d, 0), mip_chain(to_f16_bits("rg11b10ufloat", src), 5), "b10g11r11 file")
    # a refused file leaves the cube alone
    with pytest.raises(H.HostError, match="does not contain a cubemap"):
        h.env_cube_load_ktx2(1, write_ktx2(97, 16, [lv.tobytes() for lv in levels], faces=1))
    assert_chain(read_chain(d, 1), levels, "after a refused file")
    h.close()


# ------------------------------------------------------------------------------------------------ 7. argument checks

def _write(device, which, face, mip, width, height, fmt, nbytes, bytes_per_row, rows_per_image, offset=0, struct_size=None, data_len=None):
    """The raw entry (face None = all faces) with a layout the binding would never build -> (status, last_error)."""
    buf = (C.c_uint8 * max(nbytes, 1))()
    lay = AwsmCubeLayout(C.sizeof(AwsmCubeLayout) if struct_size is None else struct_size, bytes_per_row, rows_per_image, 0, offset)
    n = nbytes if data_len is None else data_len
    if face is None:
        rc = device.lib.awsm_hip_env_cube_write_all_faces(device.ctx, which, mip, width, height, fmt, buf, n, C.byref(lay))
    else:
        rc = device.lib.awsm_hip_env_cube_write_face(device.ctx, which, face, mip, width, height, fmt, buf, n, C.byref(lay))
    return rc, (device.lib.awsm_hip_last_error(device.ctx) or b"").decode()


def test_argument_checks_leave_the_cube_untouched():
    d = HipDevice(parity_tap=True)
    rng = np.random.default_rng(71)
    base = [random_f16_bits(rng, (6, 8 >> l, 8 >> l, 4)) for l in range(3)]      # 8, 4, 2: not the full chain
    d.env_cube_upload(0, [b.view(np.float16) for b in base])
    F16, big = 0, 1 << 20
    cases = [      # (arguments of _write, status, a piece of the reason)
        (dict(face=0, mip=0, width=0, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "dimensions must be non-zero"),
        (dict(face=0, mip=0, width=8, height=0, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "dimensions must be non-zero"),
        (dict(face=0, mip=0, width=8, height=4, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "must be square, got 8x4"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=0, rows_per_image=8), INVALID, "bytes_per_row must be non-zero"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=0), INVALID, "rows_per_image must be non-zero"),
        (dict(face=None, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=0xFFFFFFFF, rows_per_image=0xFFFFFFFF), INVALID, "overflow while calculating total byte size"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8, offset=2 ** 64 - 100), INVALID, "overflow while applying data offset"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8, data_len=511), INVALID, "need at least 512 bytes, got 511"),
        (dict(face=None, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8, offset=16, data_len=6 * 512 + 15), INVALID, "need at least 3088 bytes"),
        (dict(face=0, mip=1, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "mip level 1 of a 8^2 cube, which is 4x4"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=63, rows_per_image=8), INVALID, "bytes_per_row 63"),
        (dict(face=0, mip=0, width=8, height=8, fmt=1, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "a row of 8 texels takes 128 bytes"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=7), INVALID, "rows_per_image 7 for 8 rows"),
        (dict(face=0, mip=3, width=1, height=1, fmt=F16, nbytes=big, bytes_per_row=8, rows_per_image=1), OUT_OF_RANGE, "mip level 3, the cube has 3"),
        (dict(face=0, mip=0, width=8, height=8, fmt=8, nbytes=big, bytes_per_row=64, rows_per_image=8), UNSUPPORTED, "unknown AwsmCubeFormat 8"),
        (dict(face=6, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8), INVALID, "face 6"),
        (dict(face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8, struct_size=16), INVALID, "struct_size"),
    ]
    for kw, status, reason in cases:
        rc, text = _write(d, 0, **kw)
        assert rc == status and reason in text, (kw, rc, text)
        assert_chain(read_chain(d, 0), base, str(kw))
    # a cube that was never created
    rc, text = _write(d, 2, face=0, mip=0, width=8, height=8, fmt=F16, nbytes=big, bytes_per_row=64, rows_per_image=8)
    assert rc == NOT_READY and "never created or uploaded" in text
    for call in (lambda: d.env_cube_generate_mips(2), lambda: d.env_cube_info(2), lambda: d.env_cube_read_level(2, 0)):
        with pytest.raises(AwsmHipError) as e:
            call()
        assert e.value.code == NOT_READY
    # create / fill: the shape
    for call in (lambda: d.env_cube_create(1, 8, 5), lambda: d.env_cube_create(1, 0, 1), lambda: d.env_cube_create(1, 8, 0), lambda: d.env_cube_create(3, 8, 1),
                 lambda: d.env_cube_fill_colors(1, 0, (0, 0, 0, 1)), lambda: d.env_cube_fill_sky_gradient(1, 8193)):
        with pytest.raises(AwsmHipError) as e:
            call()
        assert e.value.code == INVALID
    with pytest.raises(AwsmHipError) as e:
        d.env_cube_read_level(0, 3)
    assert e.value.code == OUT_OF_RANGE
    assert_chain(read_chain(d, 0), base, "after everything")
    # the accepted neighbours of the refusals: exactly enough bytes, the last level
    rc, text = _write(d, 0, face=5, mip=2, width=2, height=2, fmt=F16, nbytes=32, bytes_per_row=16, rows_per_image=2)
    assert rc == 0, text
    base[2][5] = 0
    assert_chain(read_chain(d, 0), base, "a write of zeros")
    d.close()
