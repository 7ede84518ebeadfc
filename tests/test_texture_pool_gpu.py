"""The texture pool at run time on the device: awsm_hip_texture_array_create / _resize_layers / _write_layers /
_generate_mips_layers / _info bit for bit against tests/texture_pool_reference.py, the oracle's mip chain and the per-level entry
awsm_hip_texture_array_generate_mips; then frames through the host layer (sRGB inserts, inserts and updates between frames, glTF colour textures).
A library without the awsm_hip_texture_array_* symbols fails these tests: nothing here skips."""
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend, scenes
from awsm_renderer_amd import host as H
from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
from oracle import oracle_lib
from tests import helpers
from tests import texture_pool_reference as ref

pytestmark = pytest.mark.gpu

INVALID, NOT_READY, UNSUPPORTED, OUT_OF_RANGE = -1, -5, -6, -7


def full_mips(w, h):
    return int(max(w, h)).bit_length()


def random_texels(rng, shape):
    """Random RGBA8 with alpha 0 and 255 among the alphas."""
    t = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
    a = t[..., 3].reshape(-1)
    a[::5] = 0
    a[1::5] = 255
    return t


def read_chain(dev, index):
    _, _, _, mips = dev.texture_array_info(index)
    return [dev.texture_array_read_level(index, l) for l in range(mips)]


@pytest.fixture(scope="module")
def dev():
    d = HipDevice(parity_tap=True)
    yield d
    d.close()


# ------------------------------------------------------------------------------------------------ 1. write_layers

def laid_out(images, layout, rng):
    """images (n, h, w, 4) -> (bytes, bytes_per_row, rows_per_image, offset) with random bytes wherever the layout leaves room."""
    n, h, w, _ = images.shape
    bpr, rpi, off = {"tight": (w * 4, h, 0), "padded": (w * 4 + 8, h + 2, 0), "offset6": (w * 4, h, 6), "odd_pitch": (w * 4 + 6, h + 1, 0)}[layout]
    buf = rng.integers(0, 256, size=off + n * rpi * bpr, dtype=np.uint8)
    for l in range(n):
        for y in range(h):
            p = off + (l * rpi + y) * bpr
            buf[p: p + w * 4] = images[l, y].reshape(-1)
    return buf, bpr, rpi, off


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (33, 7), (64, 64)])
def test_write_layers_bit_for_bit(dev, w, h):
    """Every flag combination, one and three layers per call, tight / padded / offset / odd-pitch sources (the last two are read in bytes); the
    layers outside the range keep every byte."""
    rng = np.random.default_rng(100 * w + h)
    layers = 5
    dev.texture_array_create(1, w, h, layers, full_mips(w, h))
    assert dev.texture_array_info(1) == (w, h, layers, full_mips(w, h))
    assert not dev.texture_array_read_level(1, 0).any()      # created zero-filled
    want = random_texels(rng, (layers, h, w))
    dev.texture_array_write_layers(1, 0, want)                # the ground the writes below land on
    assert (dev.texture_array_read_level(1, 0) == want).all()
    for flags in (0, 1, 2, 3):
        for layout in ("tight", "padded", "offset6", "odd_pitch"):
            for n in (1, 3):
                src = random_texels(rng, (n, h, w))
                buf, bpr, rpi, off = laid_out(src, layout, rng)
                dev.texture_array_write_layers(1, 1, buf.tobytes(), n_layers=n, flags=flags, bytes_per_row=bpr, rows_per_image=rpi, offset=off)
                want[1: 1 + n] = ref.convert(src, flags)
                got = dev.texture_array_read_level(1, 0)
                assert (got == want).all(), (flags, layout, n, int((got != want).sum()))


def test_write_layers_refusals_change_nothing(dev):
    w, h = 6, 4
    dev.texture_array_create(1, w, h, 3, 1)
    base = random_texels(np.random.default_rng(5), (3, h, w))
    dev.texture_array_write_layers(1, 0, base)
    img = np.zeros((2, h, w, 4), dtype=np.uint8).tobytes()

    def refused(code, **kw):
        args = dict(index=1, first_layer=0, data=img, n_layers=2)
        args.update(kw)
        with pytest.raises(AwsmHipError) as e:
            dev.texture_array_write_layers(**args)
        assert e.value.code == code, (kw, e.value)

    refused(NOT_READY, index=40)
    refused(OUT_OF_RANGE, first_layer=2)
    refused(UNSUPPORTED, fmt=1)
    refused(UNSUPPORTED, flags=4)
    refused(INVALID, struct_size=8)
    refused(INVALID, bytes_per_row=w * 4 - 1)
    refused(INVALID, rows_per_image=h - 1)
    refused(INVALID, data=img[:-1])
    refused(INVALID, offset=1)
    refused(INVALID, offset=2 ** 64 - 1)
    refused(INVALID, n_layers=0)
    with pytest.raises(AwsmHipError) as e:
        dev.texture_array_generate_mips_layers(1, 2, 2)
    assert e.value.code == OUT_OF_RANGE
    with pytest.raises(AwsmHipError) as e:
        dev.texture_array_resize_layers(1, 2)
    assert e.value.code == INVALID
    assert (dev.texture_array_read_level(1, 0) == base).all()
    # rows_per_image is not looked at for a single image
    dev.texture_array_write_layers(1, 1, img[: w * h * 4], n_layers=1, rows_per_image=0)
    assert not dev.texture_array_read_level(1, 0)[1].any()


def test_array_shape_refusals_change_nothing():
    """A texture array or a cube of a shape the library does not hold is refused with the documented code by every entry that takes a shape
    (_upload, _create, _resize_layers; env_cube_upload, env_cube_create), and what the context held stays as it was.  The raw entries are called
    where the Python wrapper derives the value from an array."""
    dev = HipDevice(parity_tap=True)
    lib, ctx = dev.lib, dev.ctx
    w, h = 4, 2
    dev.texture_array_create(5, w, h, 2, 3)
    base = random_texels(np.random.default_rng(17), (2, h, w))
    dev.texture_array_write_layers(5, 0, base)
    texels = np.zeros(64, dtype=np.uint8)      # never read: every call below is refused before a copy
    ptr = texels.ctypes.data_as(hip_backend.C.c_void_p)

    def unchanged():
        assert dev.texture_array_info(5) == (w, h, 2, 3)
        assert (dev.texture_array_read_level(5, 0) == base).all()

    for (uw, uh, layers, mips), code in [((0, h, 2, 3), INVALID), ((w, h, 65537, 3), UNSUPPORTED), ((w, h, 2, 4), INVALID)]:
        assert lib.awsm_hip_texture_array_upload(ctx, 5, uw, uh, layers, mips, 0, ptr) == code, ("upload", uw, uh, layers, mips)
        unchanged()
    for (cw, ch, layers, mips), code in [((w, 0, 2, 3), INVALID), ((w, h, 2, 4), INVALID), ((w, h, 65537, 3), UNSUPPORTED),
                                         ((256, 256, 65536, 1), UNSUPPORTED)]:      # the last: 2^32 texels, refused before any allocation
        assert lib.awsm_hip_texture_array_create(ctx, 5, cw, ch, layers, mips) == code, ("create", cw, ch, layers, mips)
        unchanged()
    assert lib.awsm_hip_texture_array_resize_layers(ctx, 5, 65537) == UNSUPPORTED
    unchanged()
    dev.texture_array_create(6, 256, 256, 1, 1)
    assert lib.awsm_hip_texture_array_resize_layers(ctx, 6, 65536) == UNSUPPORTED      # 2^32 texels
    assert dev.texture_array_info(6) == (256, 256, 1, 1)
    unchanged()

    rng = np.random.default_rng(18)
    levels = [rng.random((6, n, n, 4)).astype(np.float16) for n in (8, 4, 2, 1)]
    dev.env_cube_upload(0, levels)
    for size, mips in [(0, 1), (8193, 1), (8, 5)]:      # 8^2 has four levels
        assert lib.awsm_hip_env_cube_upload(ctx, 0, size, mips, ptr) == INVALID, ("env_cube_upload", size, mips)
        assert lib.awsm_hip_env_cube_create(ctx, 0, size, mips) == INVALID, ("env_cube_create", size, mips)
        assert dev.env_cube_info(0) == (8, 4)
        assert (dev.env_cube_read_level(0, 0).view(np.uint16) == levels[0].view(np.uint16)).all()
    unchanged()
    dev.close()


# ------------------------------------------------------------------------------------------------ 2. generate_mips_layers

KINDS = [0, 1, 2, 3, 5]


@pytest.mark.parametrize("w,h", [(1, 1), (2, 2), (3, 5), (5, 3), (33, 33), (64, 4), (4, 64), (48, 96), (96, 32), (128, 128)])
def test_generate_mips_layers_bit_for_bit(dev, w, h):
    """Layers [1, 4) of five (kinds 0 1 2 3 5) against the oracle's chain and against a second array that got the same level 0 and the per-level
    entry; layers 0 and 4 keep what all their levels held.  Non-square extents (one side reaches 1 while the other keeps halving), odd extents,
    partial tiles, and 128 x 128 = seven levels below level 0 = two launches."""
    rng = np.random.default_rng(7000 + 131 * w + h)
    mips = full_mips(w, h)
    before = random_texels(rng, (5, h, w))
    dev.texture_array_upload(1, before, mips)
    dev.texture_array_generate_mips(1, KINDS)                 # every level of every layer holds something that is not zero
    held = read_chain(dev, 1)
    level0 = before.copy()
    level0[1:4] = random_texels(rng, (3, h, w))
    if w >= 2 and h >= 2:                                     # normals whose 2 x 2 mean is the zero vector: 1 / 0 * 0 = NaN, stored as 0
        level0[1, :2, :2, :3] = np.array([[0, 255], [0, 255]], dtype=np.uint8)[..., None]
    for l in (1, 2, 3):
        dev.texture_array_write_layers(1, l, level0[l: l + 1], mip_kind=KINDS[l])
    dev.texture_array_generate_mips_layers(1, 1, 3)
    got = read_chain(dev, 1)

    dev.texture_array_upload(2, level0, mips)
    dev.texture_array_generate_mips(2, KINDS)
    per_level = read_chain(dev, 2)
    chain, levels = oracle_lib.mip_chain(level0, KINDS)
    assert levels == mips == len(got)
    for l in range(mips):
        orc = oracle_lib.mip_level_view(chain, w, h, 5, l)
        assert (got[l][1:4] == per_level[l][1:4]).all(), ("per-level entry", l, int((got[l][1:4] != per_level[l][1:4]).sum()))
        assert (got[l][1:4] == orc[1:4]).all(), ("oracle", l, int((got[l][1:4] != orc[1:4]).sum()))
        assert (got[l][0] == held[l][0]).all() and (got[l][4] == held[l][4]).all(), ("layers outside the range", l)
    if w >= 2 and h >= 2:
        assert (got[1][1, 0, 0, :3] == 0).all()               # the NaN -> 0 store did happen


# ------------------------------------------------------------------------------------------------ 3. resize_layers

def test_resize_layers_keeps_every_level():
    dev = HipDevice(parity_tap=True)
    w, h = 33, 18
    rng = np.random.default_rng(11)
    dev.texture_array_create(3, w, h, 3, full_mips(w, h))
    for l in range(3):
        dev.texture_array_write_layers(3, l, random_texels(rng, (1, h, w)), mip_kind=l)
    dev.texture_array_generate_mips_layers(3, 0, 3)
    before = read_chain(dev, 3)
    dev.texture_array_resize_layers(3, 8)
    assert dev.texture_array_info(3) == (w, h, 8, full_mips(w, h))
    after = read_chain(dev, 3)
    for l, (b, a) in enumerate(zip(before, after)):
        assert a.shape[0] == 8 and (a[:3] == b).all() and not a[3:].any(), l
    # the kinds moved too: regenerating a kept layer gives its bytes again
    dev.texture_array_generate_mips_layers(3, 1, 2)
    for b, a in zip(before, read_chain(dev, 3)):
        assert (a[:3] == b).all()
    dev.texture_array_resize_layers(3, 8)                     # nothing to do
    dev.close()


def test_resize_layers_leaves_a_gradient_mip_frame_as_it_was(oracle_lut):
    """The lean route's closed-form level offsets multiply by the array's layer count: after 5 -> 8 layers the same frame comes out, bit for bit."""
    sc = small_scene()
    r = H.Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), mipmap=True)
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    before = dev.read_opaque().copy()
    assert dev.texture_array_info(0)[2] == 5
    dev.texture_array_resize_layers(0, 8)
    assert dev.texture_array_info(0)[2] == 8
    r.render(sync=True)
    after = dev.read_opaque()
    assert before.any() and (before == after).all(), int((before != after).sum())
    r.close()


# ------------------------------------------------------------------------------------------------ 4. frames through the host layer

def small_scene(**kw):
    return scenes.helmet_scene(96, 64, segments=24, rings=18, tex_size=32, **kw)


def frame_bits(sc, lut, **kw):
    r = H.Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(lut), mipmap=True, **kw)
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    img = dev.read_opaque().copy()
    r.close()
    return img


def test_srgb_inserts_equal_converted_bytes_through_the_old_entry(oracle_lut):
    """Base colour and emissive inserted with srgb_to_linear: the frame of a fresh context that got the numpy-converted bytes through
    awsm_host_texture_insert_kind, bit for bit; the oracle given those bytes, within the suite's bar; the host's mirror holds them."""
    sc = small_scene()
    lin = dataclasses.replace(sc, textures=[ref.convert(t, ref.SRGB_TO_LINEAR) if i in (0, 4) else t for i, t in enumerate(sc.textures)])
    assert not (lin.textures[0] == sc.textures[0]).all()
    r = H.Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), mipmap=True, srgb_textures=(0, 4))
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    got = dev.read_opaque().copy()
    pool = r.host.pool_arrays()
    assert len(pool) == 1 and (pool[0] == np.stack(lin.textures)).all()
    for level in range(dev.texture_array_info(0)[3]):        # the device's chain is the oracle's chain of the converted bytes
        chain, _ = oracle_lib.mip_chain(np.stack(lin.textures), [0, 2, 1, 3, 4])
        assert (dev.texture_array_read_level(0, level) == oracle_lib.mip_level_view(chain, 32, 32, 5, level)).all(), level
    orc = helpers.oracle_frame(helpers.build_model(lin), oracle_lut, mipmap=True)
    res = helpers.compare_frames(orc, dev, rgb_tol=1e-4)
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["alpha_mismatch"] == 0 and res["f16_max_ulp"] <= 2, res
    r.close()
    want = frame_bits(lin, oracle_lut)
    assert (got == want).all(), int((got != want).sum())
    assert not (got == frame_bits(sc, oracle_lut)).all()     # the decode matters


def test_insert_between_frames_equals_everything_up_front(oracle_lut):
    """Render, insert an image into the resident array (it grows on the device; only the new image crosses the bus), point the material at it,
    render: the frame of a fresh context that had all six images from the start, MipmapMode::Gradient included."""
    sc = small_scene()
    new = scenes.value_noise_rgba8(np.random.default_rng(77), 32, 6, base=(0.3, 0.6, 0.4), amp=(0.3, 0.3, 0.3))
    r = H.Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), mipmap=True)
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    first = dev.read_opaque().copy()
    tid = r.host.texture_insert(new, 0)
    assert tid == 5
    mat = dataclasses.replace(sc.materials[0], base_color_tex=scenes.TextureRef(tid))
    r.host.material_update(r.keys.material_keys[0], H.material_struct(mat, r.host, {}))
    r.render(sync=True)
    assert new.nbytes <= r.host.upload_bytes_last_frame() < 5 * new.nbytes      # the new image, the material, the camera: less than the array's level 0
    assert dev.texture_array_info(0)[2] == 10                 # 5 doubled
    got = dev.read_opaque().copy()
    r.close()
    up_front = dataclasses.replace(sc, textures=list(sc.textures) + [new], materials=[mat])
    want = frame_bits(up_front, oracle_lut)
    assert (got == want).all(), int((got != want).sum())
    assert not (got == first).all()


def test_update_between_overlapped_frames(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES: frame A is enqueued, the base colour's pixels are replaced, frame B is enqueued; A shows the old pixels, B the new."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sc = small_scene()
    new = scenes.value_noise_rgba8(np.random.default_rng(78), 32, 5, base=(0.2, 0.3, 0.7), amp=(0.2, 0.3, 0.3))
    nbytes = sc.height * sc.width * 8
    r = H.Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), mipmap=True, overlap_frames=True)
    r.host.set_render_timings(False)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    outs = []
    for _ in range(2):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        outs.append(p)
    dev.bind_output(outs[0].value, nbytes)
    r.host.render(sync=False)
    r.host.texture_update(0, new)
    dev.bind_output(outs[1].value, nbytes)
    r.host.render(sync=False)
    dev.frame_flush()
    assert hip.hipDeviceSynchronize() == 0
    imgs = []
    for p in outs:
        a = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0
        imgs.append(a)
        hip.hipFree(p)
    dev.bind_output(None)
    r.close()
    old_frame = frame_bits(sc, oracle_lut)
    new_frame = frame_bits(dataclasses.replace(sc, textures=[new] + list(sc.textures[1:])), oracle_lut)
    assert not (old_frame == new_frame).all()
    assert (imgs[0] == old_frame).all(), int((imgs[0] != old_frame).sum())
    assert (imgs[1] == new_frame).all(), int((imgs[1] != new_frame).sum())


def test_gltf_colour_textures_are_decoded(tmp_path, oracle_lut):
    """A .glb whose colour PNGs hold sRGB-encoded bytes, loaded with AWSM_GLTF_SRGB_COLOR_TEXTURES, against the .glb of the same scene with linear
    textures loaded as stored.  The linear texels are taken from the table's image, so the encode / decode round trip is exact everywhere.  The
    base colour image is the occlusion image too: it enters the pool twice, decoded and as stored."""
    from awsm_renderer_amd import gltf_export
    sc = small_scene()
    image = ref.table_image().astype(np.int32)
    nearest = image[np.abs(np.arange(256)[:, None] - image[None, :]).argmin(axis=1)].astype(np.uint8)

    def in_image(t):
        out = t.copy()
        out[..., :3] = nearest[t[..., :3]]
        return out

    base_lin, em_lin = in_image(sc.textures[0]), in_image(sc.textures[4])
    base_enc, em_enc = base_lin.copy(), em_lin.copy()
    base_enc[..., :3] = ref.srgb_encode_exact(base_lin[..., :3])
    em_enc[..., :3] = ref.srgb_encode_exact(em_lin[..., :3])
    assert (ref.convert(base_enc, ref.SRGB_TO_LINEAR) == base_lin).all() and not (base_enc == base_lin).all()
    m = sc.materials[0]
    direct = dataclasses.replace(sc, textures=[base_lin, sc.textures[1], sc.textures[2], base_enc, em_lin])
    encoded = dataclasses.replace(sc, textures=[base_enc, sc.textures[1], sc.textures[2], em_enc],
                                  materials=[dataclasses.replace(m, occlusion_tex=scenes.TextureRef(0), emissive_tex=scenes.TextureRef(3))])
    p_direct, p_encoded = str(tmp_path / "direct.glb"), str(tmp_path / "encoded.glb")
    gltf_export.write_glb(direct, p_direct)
    gltf_export.write_glb(encoded, p_encoded)
    r = H.Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), mipmap=True, gltf=p_encoded, srgb_textures=True)
    assert r.gltf_info["images"] == 4
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    got = dev.read_opaque().copy()
    pool = r.host.pool_arrays()
    assert len(pool) == 1 and pool[0].shape[0] == 5           # four images, five layers: image 0 as colour and as data
    assert (pool[0] == np.stack(direct.textures)).all()
    assert (dev.texture_array_read_level(0, 0)[:5] == pool[0]).all()
    r.close()
    want = frame_bits(sc, oracle_lut, gltf=p_direct)
    assert (got == want).all(), int((got != want).sum())
    stored = frame_bits(sc, oracle_lut, gltf=p_encoded)       # without the option the bytes are taken as stored, as before
    assert not (stored == want).all()
