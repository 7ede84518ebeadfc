"""awsm_hip_env_cube_from_equirect on the device against the f64 numpy restatement (tests/equirect_reference.py).

The bar, per component: |device - reference| <= half an f16 ulp of the reference's binade + 4 x EQUIRECT_SLACK_REL x |reference|.  The first term is
the one rounding of the store; the second is four times what the restatement run in f32 spends (tests/test_equirect_cpu.py derives it).  Bilinear
lookup is continuous in the direction, so no texel is ill-conditioned and none is left out.  Uniform panoramas, the axis-painted panorama, and the
whole path against its parts are held to exact bits."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from awsm_renderer_amd.hip_backend import AWSM_PANO_RGBA32F, AWSM_PANO_RGBE8, AwsmEquirect, AwsmHipError, HipDevice
from oracle import oracle_lib
from tests import equirect_reference as R
from tests import rgbe_files as F
from tests.test_equirect_cpu import EQUIRECT_SLACK_REL, SMOOTH_FORMATS, SMOOTH_PANOS, central_quarter, smooth_cases

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, UNSUPPORTED, OUT_OF_RANGE = -1, -5, -6, -7
SKY, PRE, IRR = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    d = HipDevice(parity_tap=True)
    yield d
    d.close()


def raw_project(device, which, buf, width, height, fmt, bytes_per_row=0, samples=0, yaw=0.0, scale=1.0, struct_size=None, data_len=None):
    """The C-ABI call itself -> (status, message)."""
    p = AwsmEquirect(C.sizeof(AwsmEquirect) if struct_size is None else struct_size, width, height, fmt, bytes_per_row, samples, yaw, scale)
    rc = device.lib.awsm_hip_env_cube_from_equirect(device.ctx, which, buf.ctypes.data_as(C.c_void_p), buf.nbytes if data_len is None else data_len, C.byref(p))
    return rc, (device.lib.awsm_hip_last_error(device.ctx) or b"").decode()


def project(device, pano, n, samples=0, yaw=0.0, scale=1.0, padded=False, which=SKY):
    """Level 0 of a fresh n^2 cube from `pano` -> uint16 [6, n, n, 4].  padded: rows 7 bytes further apart than they need be (so that rows start at odd
    addresses), the padding filled with bytes that would show."""
    device.env_cube_create(which, n, 1)
    h, w = pano.shape[:2]
    rows = np.ascontiguousarray(pano).view(np.uint8).reshape(h, -1)
    bpr = 0
    if padded:
        bpr = rows.shape[1] + 7
        buf = np.full((h, bpr), 0xEE, dtype=np.uint8)
        buf[:, :rows.shape[1]] = rows
        rows = buf.reshape(-1)[:bpr * (h - 1) + w * (4 if pano.dtype == np.uint8 else 16)].copy()      # no padding behind the last row: the layout's minimum
    rc, text = raw_project(device, which, rows, w, h, AWSM_PANO_RGBE8 if pano.dtype == np.uint8 else AWSM_PANO_RGBA32F, bpr, samples, yaw, scale)
    assert rc == 0, text
    return device.env_cube_read_level(which, 0).view(np.uint16)


def excess(got_bits, ref):
    """How far over the bar the worst component is, in units of the bar's slack term 4 x EQUIRECT_SLACK_REL x |ref| (<= 0: inside the bar; -1: inside the
    half ulp alone), and the largest error in f16 ulps."""
    err = np.abs(got_bits[..., :3].view(np.float16).astype(np.float64) - ref)
    ulp = R.f16_ulp(ref)
    slack = 4.0 * EQUIRECT_SLACK_REL * np.abs(ref)
    over = (err - 0.5 * ulp - slack) / slack
    return float(over.max()), float((err / ulp).max())


# ------------------------------------------------------------------------------------------------ exact bits

# a dozen RGBE values whose channels are zero or inside f16's normal range: mantissas 1 and 255, the smallest normal, the largest exponent that fits
RGBE_VALUES = [(1, 255, 128, 136), (255, 1, 77, 136), (1, 1, 1, 122), (255, 255, 255, 143), (128, 64, 32, 129), (200, 0, 3, 128), (0, 0, 9, 140),
               (17, 34, 51, 125), (255, 254, 253, 130), (1, 2, 3, 144), (99, 0, 0, 136), (129, 255, 1, 123)]


@pytest.mark.parametrize("n", [1, 3, 16, 33])
def test_uniform_rgbe_panoramas_give_the_exact_bits(dev, n):
    for value, samples in [(v, s) for v in RGBE_VALUES for s in (1, 2, 3, 8)]:
        pano = np.broadcast_to(np.array(value, dtype=np.uint8), (4, 8, 4)).copy()
        want = F.rgbe_to_float(pano[0, 0]).astype(np.float16)
        assert (want.astype(np.float64) == F.rgbe_to_float(pano[0, 0])).all() and np.isfinite(want).all()      # the value is an f16
        got = project(dev, pano, n, samples, yaw=0.7)
        assert (got[..., :3] == want.view(np.uint16)).all() and (got[..., 3] == R.HALF_ONE).all(), (value, samples)


def test_rgba32f_clamp_nan_and_infinity(dev):
    for value, bits in ((2.0 ** 20, 0x7BFF), (np.nan, 0x0000), (-np.inf, 0xFBFF), (np.inf, 0x7BFF), (-3.0, 0xC200)):
        pano = np.full((4, 8, 4), value, dtype=np.float32)
        pano[..., 3] = np.nan                                      # the source alpha is ignored
        for n, samples in ((4, 2), (16, 1)):
            got = project(dev, pano, n, samples)
            assert (got[..., :3] == bits).all() and (got[..., 3] == R.HALF_ONE).all(), (value, n, samples, np.unique(got[..., :3]))


def test_orientation(dev):
    """The axis-painted panorama: forward is -Z, +X is to its right (u = 0.75), row 0 is up, nothing is mirrored."""
    got = project(dev, R.axis_painted(64, 32), 16, 1)
    q = central_quarter(16)
    for face in range(6):
        assert (got[face, q, q, :3] == R.AXIS_COLORS[face].astype(np.float16).view(np.uint16)).all(), face


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.fixture(scope="module")
def smooth_panos():
    return {(w, h, fmt): R.smooth_panorama(w, h, fmt) for (w, h) in SMOOTH_PANOS for fmt in SMOOTH_FORMATS}


def test_smooth_source_against_the_restatement(dev, smooth_panos):
    worst = (-1e9, None)
    for (w, h), fmt, n, samples, (yaw, scale, padded) in smooth_cases():
        pano = smooth_panos[(w, h, fmt)]
        got = project(dev, pano, n, samples, yaw, scale, padded)
        ref = R.project(pano, n, samples, yaw, scale)
        over, ulps = excess(got, ref)
        worst = max(worst, (over, (w, h, fmt, n, samples, yaw, scale, padded, ulps)))
        assert (got[..., 3] == R.HALF_ONE).all()
        assert over <= 0.0, (w, h, fmt, n, samples, yaw, scale, padded, over, ulps)
    print("smooth source: worst excess %.3f of the slack at %s" % worst)


def test_the_seam_face_and_a_half_turn(dev, smooth_panos):
    """+Z straddles u = 0 / 1: its texels meet the bar like any others, and the panorama rolled by half its width with yaw = pi gives the first run."""
    for fmt in SMOOTH_FORMATS:
        pano = smooth_panos[(64, 32, fmt)]
        ref = R.project(pano, 16, 2)
        first = project(dev, pano, 16, 2)
        over, ulps = excess(first[4], ref[4])
        print("%s, the +Z face: worst excess %.3f of the slack, largest error %.3f ulp" % (fmt, over, ulps))
        assert over <= 0.0, (fmt, over, ulps)
        second = project(dev, np.roll(pano, 32, axis=1), 16, 2, yaw=math.pi)
        over, ulps = excess(second, ref)
        print("%s, rolled by half with yaw pi: worst excess %.3f of the slack, largest error %.3f ulp" % (fmt, over, ulps))
        assert over <= 0.0, (fmt, over, ulps)


def test_a_source_over_four_mebibytes(dev):
    """1024 x 1025 RGBE is 4 198 400 bytes: past the staging ring's 4 MiB, so the copy comes from the caller's memory behind one event."""
    pano = R.smooth_panorama(1024, 1025, "rgbe")
    assert pano.nbytes > (4 << 20)
    got = project(dev, pano, 8)
    ref = R.project(pano, 8, 0)
    assert R.auto_samples(1024, 8) == 8
    over, ulps = excess(got, ref)
    print("1024 x 1025 into 8^2 at S = 8: worst excess %.3f of the slack, largest error %.3f ulp" % (over, ulps))
    assert over <= 0.0, (over, ulps)


# ------------------------------------------------------------------------------------------------ the whole path

def read_chain(device, which):
    size, mips = device.env_cube_info(which)
    return [device.env_cube_read_level(which, l) for l in range(mips)]


def test_load_hdr_equals_its_parts(dev, tmp_path):
    rgbe = R.smooth_panorama(96, 48, "rgbe")
    data = F.write_hdr(rgbe, "rle", extra=["EXPOSURE=2.0"])
    decoded, _ = H.hdr_decode(data)
    assert (decoded == rgbe).all()
    dev.env_cube_create(SKY, 32, 6)
    dev.env_cube_from_equirect(SKY, decoded, yaw=0.25, samples=2, scale=0.5)
    dev.env_cube_generate_mips(SKY)
    want = [lv.view(np.uint16).copy() for lv in read_chain(dev, SKY)]
    assert [lv.shape[1] for lv in want] == [32, 16, 8, 4, 2, 1]
    over, _ = excess(want[0], R.project(rgbe, 32, 2, 0.25, 0.5))
    assert over <= 0.0, over

    path = tmp_path / "sky.hdr"
    path.write_bytes(data)
    h = H.Host()
    hd = HipDevice.from_ctx(h.device_ctx, 0, 0)
    for source in (data, str(path)):
        info = h.env_cube_load_hdr(SKY, source, 32, samples=2, yaw=0.25, scale=0.5)
        assert info == {"width": 96, "height": 48, "flipped_y": 0, "rle": 1, "exposure": 2.0}
        got = read_chain(hd, SKY)
        assert len(got) == 6
        for a, b in zip(got, want):
            assert (a.view(np.uint16) == b).all()
    h.env_cube_create(PRE, 32, 6)                                  # the thin wrapper, then the chain on its own
    h.env_cube_from_equirect(PRE, decoded, yaw=0.25, samples=2, scale=0.5)
    h.env_cube_regenerate_mipmaps(PRE)
    for a, b in zip(read_chain(hd, PRE), want):
        assert (a.view(np.uint16) == b).all()
    h.close()


def test_frames_lit_from_a_loaded_panorama(oracle_lut):
    """helmet_scene at 160 x 90 with overlapped frames: a frame is enqueued, the panorama is loaded and the IBL baked, the next frame is enqueued.  That
    frame equals, in every bit, the frame of a fresh context that was given the read-back chains — so the load took effect between the two frames, in
    stream order, and what it made is what the read-back says."""
    sc = scenes.helmet_scene(160, 90, segments=32, rings=24, tex_size=32)
    data = F.write_hdr(R.smooth_panorama(64, 32, "rgbe"), "rle")
    lut = oracle_lib.lut_rg_to_rgba16f(oracle_lut)
    r = H.Renderer(sc, parity_tap=True, overlap_frames=True, lut_rgba16f=lut)
    d = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    r.render(sync=True)
    flat = d.read_opaque().copy()
    r.render(sync=False)
    r.host.env_cube_load_hdr(SKY, data, 16)
    r.host.env_bake_ibl(16, 5, 8, 64)
    r.render(sync=True)
    got = d.read_opaque().copy()
    sky, pre, irr = read_chain(d, SKY), read_chain(d, PRE), read_chain(d, IRR)
    r.close()
    assert [lv.shape[1] for lv in sky] == [16, 8, 4, 2, 1] and [lv.shape[1] for lv in pre] == [16, 8, 4, 2, 1] and [lv.shape[1] for lv in irr] == [8]
    assert (got != flat).any()

    sc2 = dataclasses.replace(sc, env_cubes={"skybox": sky, "prefiltered": pre, "irradiance": irr}, prefiltered_mip_count=5, irradiance_mip_count=1)
    r2 = H.Renderer(sc2, parity_tap=True, overlap_frames=True, lut_rgba16f=lut)
    d2 = HipDevice.from_ctx(r2.host.device_ctx, sc.width, sc.height)
    r2.render(sync=True)
    want = d2.read_opaque().copy()
    r2.close()
    assert (got == want).all(), int((got != want).any(axis=-1).sum())


# ------------------------------------------------------------------------------------------------ error codes

def test_error_codes():
    assert C.sizeof(AwsmEquirect) == 32
    d = HipDevice(parity_tap=True)
    pano = R.smooth_panorama(8, 4, "rgbe")
    buf = pano.reshape(-1)
    ok = dict(width=8, height=4, fmt=AWSM_PANO_RGBE8)
    rc, text = raw_project(d, SKY, buf, **ok)
    assert rc == NOT_READY and "uniform colour" in text, (rc, text)
    d.env_cube_fill_sky_gradient(SKY, 8)
    before = [lv.view(np.uint16).copy() for lv in read_chain(d, SKY)]
    f32 = R.smooth_panorama(8, 4, "f32").reshape(-1)
    for want, kw in ((INVALID, dict(ok, struct_size=28)), (INVALID, dict(ok, width=0)), (INVALID, dict(ok, height=0)), (INVALID, dict(ok, samples=9)),
                     (INVALID, dict(ok, yaw=float("nan"))), (INVALID, dict(ok, yaw=float("inf"))), (INVALID, dict(ok, scale=float("nan"))),
                     (INVALID, dict(ok, scale=float("-inf"))), (INVALID, dict(ok, bytes_per_row=31)), (OUT_OF_RANGE, dict(ok, data_len=8 * 4 * 4 - 1)),
                     (OUT_OF_RANGE, dict(ok, bytes_per_row=40)), (OUT_OF_RANGE, dict(ok, height=5)), (UNSUPPORTED, dict(ok, fmt=2)),
                     (OUT_OF_RANGE, dict(ok, fmt=AWSM_PANO_RGBA32F))):
        rc, text = raw_project(d, SKY, buf, **kw)
        assert rc == want and text, (kw, rc, text)
    rc, text = raw_project(d, 3, buf, **ok)
    assert rc == INVALID, (rc, text)
    rc, text = raw_project(d, PRE, buf, **ok)                      # a cube that is still a colour, whatever the skybox holds
    assert rc == NOT_READY, (rc, text)
    with pytest.raises(AwsmHipError) as e:                         # ... and nothing was created along the way
        d.env_cube_info(PRE)
    assert e.value.code == NOT_READY
    for a, b in zip(read_chain(d, SKY), before):                   # every refusal left the cube as it was
        assert (a.view(np.uint16) == b).all()
    # the accepted neighbours: the tight layout named outright, S = 8, a bytes_per_row that is just long enough, the other format
    for kw, data in ((dict(ok, bytes_per_row=32, samples=8), buf), (dict(ok, bytes_per_row=36, data_len=36 * 3 + 32), np.zeros(36 * 4, dtype=np.uint8)),
                     (dict(ok, fmt=AWSM_PANO_RGBA32F, scale=0.0), f32)):
        rc, text = raw_project(d, SKY, data, **kw)
        assert rc == 0, (kw, text)
    chain = read_chain(d, SKY)
    assert (chain[0].view(np.uint16) != before[0]).any()           # level 0 was written
    for a, b in zip(chain[1:], before[1:]):                        # and only level 0: the chain is generate_mips' to make
        assert (a.view(np.uint16) == b).all()
    over, _ = excess(chain[0].view(np.uint16), R.project(R.smooth_panorama(8, 4, "f32"), 8, 0))      # scale 0 means 1.0
    assert over <= 0.0, over
    d.close()
