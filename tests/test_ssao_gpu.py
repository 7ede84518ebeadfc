"""GPU tests of the screen-space ambient occlusion: the three layers and the modulated opaque image bit for bit against
tests/ssao_reference.py fed the device's own keys, under MSAA x4, under a transparent pass, in overlap mode, through a replayed frame, with HUD
meshes, through the host layer, and the refusals."""
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc
from oracle import oracle_lib
from tests import helpers
from tests import ssao_reference as sr

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _point(model, cam):
    """The model's camera <- one of the reference's cameras (the scene's f32 matrices, the block the model derives from them)."""
    sc = model.scene
    sr.set_camera(sc, sr.camera(cam, sc.width, sc.height))
    model.update_camera()
    return bytes(model.camera_bytes)


def _frame(dev, model, transparent=False, post=None, end=True):
    """One more frame on a device helpers.hip_frame set up, with the model's camera as it is now; transparent: the world transparent pass too."""
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    if transparent:
        dev.transparent_pass(model.collect_transparent_draws())
    if post:
        dev.post_pass(**post)
    if end:
        dev.frame_end()


def _want(dev, block, params=None):
    """The restatement fed the device's own keys and the camera block the test wrote."""
    H, W = dev.height, dev.width
    return sr.ssao(dev.read_visibility(), block, W, H, params)


def _assert_layers(dev, block, params=None, what=""):
    want = _want(dev, block, params)
    raw, smoothed, view_z = dev.read_ssao()
    for name, got, ref in (("view_z", view_z, want["view_z"]), ("ao_raw", raw, want["ao_raw"]), ("ao_smoothed", smoothed, want["ao_smoothed"])):
        bad = _bits(got) != _bits(ref)
        assert not bad.any(), "%s %s: %d of %d pixels differ, first at %s: device %r, restatement %r" % (
            what, name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])
    return want


def _assert_image(on16, off16, want, on32=None, off32=None, what=""):
    ref = sr.apply(off16, want["m"], want["hit"])
    bad = (on16 != ref).any(axis=-1)
    at = tuple(np.argwhere(bad)[0]) if bad.any() else None
    assert not bad.any(), "%s: %d pixels of the opaque image differ, first at %s: device %s, off %s, restatement %s, m %r (bits %#x)" % (
        what, int(bad.sum()), at, on16[at], off16[at], ref[at], want["m"][at], int(_bits(want["m"])[at]))
    assert (on16[..., 3] == off16[..., 3]).all() and (on16[~want["hit"]] == off16[~want["hit"]]).all()
    if on32 is not None:
        ref32 = sr.apply_f32(off32, want["m"], want["hit"])
        assert (_bits(on32) == _bits(ref32)).all(), "%s: %d pixels of the f32 opaque image differ" % (what, int((_bits(on32) != _bits(ref32)).any(axis=-1).sum()))


# ------------------------------------------------------------------------------------------------ layers and image, bit for bit

@pytest.mark.parametrize("scene", ["corner", "boxes"])
@pytest.mark.parametrize("W,H", sr.SIZES)
def test_layers_are_the_f32_restatement_bit_for_bit(W, H, scene, oracle_lut):
    """view z, A and A' of every pixel under the four cameras.  8x5: less than one tile; 33x17 and 70x45: ragged right and bottom tiles, and (70x45)
    tiles whose apron is all neighbouring tiles."""
    model = helpers.build_model(sr.SCENES[scene](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dev.set_ssao()
    worked = 0
    for cam in sr.CAMERAS:
        block = _point(model, cam)
        _frame(dev, model)
        want = _assert_layers(dev, block, what="%s %s %dx%d" % (scene, cam, W, H))
        worked += int((want["ao_smoothed"] < 1.0).sum())
    assert worked >= 20                                                                      # (at 8x5 the close-up camera's)
    dev.close()


@pytest.mark.parametrize("scene", ["corner", "boxes"])
def test_opaque_image_is_the_modulated_ssao_off_image(scene, oracle_lut):
    """RGBA16F and the f32 parity tap against f16_rne(f32(off) * m) / off * m, `off` from a context that never had SSAO; alpha and pixels nothing hit
    are untouched."""
    W, H = 70, 45
    model = helpers.build_model(sr.SCENES[scene](W, H))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    on.set_ssao()
    moved = 0
    for cam in sr.CAMERAS:
        block = _point(model, cam)
        _frame(on, model); _frame(off, model)
        want = _assert_layers(on, block, what="%s %s" % (scene, cam))
        on16, off16 = on.read_opaque(), off.read_opaque()
        _assert_image(on16, off16, want, on.read_opaque_f32(), off.read_opaque_f32(), what="%s %s" % (scene, cam))
        assert (on.read_visibility() == off.read_visibility()).all()
        moved += int((on16 != off16).any(axis=-1).sum())
    assert moved >= 0.15 * W * H
    on.close(); off.close()


def test_parameters_reach_the_kernels(oracle_lut):
    W, H = 33, 17
    model = helpers.build_model(sr.corner(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    off = dev.read_opaque()
    block = bytes(model.camera_bytes)
    base = None
    for params in ({}, {"radius": 0.3}, {"intensity": 2.5}, {"bias": 0.2}, {"strength": 0.25}, {"radius": 1.25, "intensity": 0.5, "bias": 0.0, "strength": 0.75}):
        dev.set_ssao(**params)
        _frame(dev, model)
        want = _assert_layers(dev, block, params, what=str(params))
        _assert_image(dev.read_opaque(), off, want, what=str(params))
        base = want["m"] if base is None else base
        assert not params or (want["m"] != base).sum() >= 50, params
    dev.close()


@pytest.mark.parametrize("W,H", sr.SIZES[1:])
def test_msaa_layers_take_the_least_of_the_four_sample_depths(W, H, oracle_lut):
    model = helpers.build_model(sr.boxes(W, H))
    on, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    off, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    on.set_ssao()
    for cam in ("perspective", "closeup", "far"):
        block = _point(model, cam)
        _frame(on, model); _frame(off, model)
        keys = on.read_visibility()
        assert keys.shape == (H, W, 4)
        want = _assert_layers(on, block, what="msaa %s %dx%d" % (cam, W, H))
        d_s = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        mixed = (keys != sr.NO_HIT).all(axis=-1) & (d_s.min(axis=-1) != d_s[..., 0])
        assert cam == "far" or mixed.sum() >= 10                                             # pixels where sample 0 is not the nearest
        _assert_image(on.read_opaque(), off.read_opaque(), want, on.read_opaque_f32(), off.read_opaque_f32(), what="msaa %s" % cam)
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ what reads the opaque image afterwards

def _glass_scene(W, H):
    """`corner` with a transmissive quad standing in front of the wall-wall crease."""
    sc = sr.corner(W, H)
    sc.materials.append(MaterialDesc(base_color_factor=(0.95, 0.98, 1.0, 1.0), transmission={"factor": 0.95}, metallic_factor=0.0, roughness_factor=0.1))
    quad = dataclasses.replace(sr._quad((0.15, 0.05, 1.2), (1.05, 0.0, -1.05), (0.0, 1.8, 0.0), 0), material=len(sc.materials) - 1)
    sc.nodes.append(NodeDesc(primitives=[quad]))
    return sc


def test_transparent_pass_reads_the_modulated_image(oracle_lut):
    W, H = 70, 45
    model = helpers.build_model(_glass_scene(W, H))
    model.collect_draws()
    assert len(model.collect_transparent_draws()) == 1
    on, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    off, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    on.set_ssao()
    _frame(on, model, transparent=True)
    touched = (off.read_composite() != off.read_opaque()).any(axis=-1)                        # the glass's fragments (a refracting surface leaves none as it was)
    assert 150 <= touched.sum() <= 0.5 * W * H
    want = _assert_layers(on, bytes(model.camera_bytes))
    on_opaque, on_comp, off_comp = on.read_opaque(), on.read_composite(), off.read_composite()
    _assert_image(on_opaque, off.read_opaque(), want)
    assert (on_comp[~touched] == on_opaque[~touched]).all()                                  # the blit took the modulated image
    behind = touched & (want["m"] < 0.9)
    # refraction sees the occluded crease: its tap lands a few pixels from the fragment, inside the crease's dark band more often than not
    assert behind.sum() >= 30 and (on_comp != off_comp).any(axis=-1)[behind].mean() > 0.5
    on.close(); off.close()


@pytest.mark.parametrize("W,H", [(70, 45), (1920, 1080)])
def test_each_overlapped_frame_is_its_synchronous_twin(W, H, oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES, four frames with a moving camera, enqueue-only, each into its own image: frame i + 2's geometry pass overwrites the keys
    of frame i's slot and must wait until frame i's SSAO has read them.  set_ssao after the last enqueue does not reach a pass already enqueued.
    1920x1080: the SSAO kernels run for a hundred microseconds while this scene's geometry pass takes a few, so a geometry pass let go before them
    would clear keys they are reading; the small size is the one the restatement is run at."""
    import torch
    from awsm_renderer_amd.hip_backend import HipDevice
    small = W * H < 10000
    model = helpers.build_model(sr.boxes(W, H))
    draws = model.collect_draws()
    eyes = [(3.2 - 0.35 * i, 2.6 + 0.1 * i, 3.6 - 0.2 * i) for i in range(4)]
    blocks = [sr.camera_block(eye, (0.6, 0.5, 0.6), W, H) for eye in eyes]
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dev.set_ssao()
    want = []
    for block in blocks:
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
        if small:
            _assert_layers(dev, block)
        want.append(dev.read_opaque())
    dev.close()
    assert all((want[i] != want[i + 1]).any(axis=-1).sum() >= 0.25 * W * H for i in range(3))
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    dev.set_ssao()
    images = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in blocks]
    for block, image in zip(blocks, images):                                                  # no frame_end between the frames
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.bind_output(image.data_ptr(), H * W * 8)
        dev.geometry_pass(draws); dev.opaque_pass()
    dev.set_ssao(intensity=4.0)
    dev.frame_end()
    torch.cuda.synchronize()
    for i, image in enumerate(images):
        got = image.cpu().numpy().view(np.uint16)
        assert (got == want[i]).all(), (i, int((got != want[i]).any(axis=-1).sum()))
    if small:
        _assert_layers(dev, blocks[-1])                                                      # the last frame's layers, with the record it was given
    dev.close()


def test_replayed_frame_is_modulated_once(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST: the frame overflows its (triangle, tile) list and frame_end replays the geometry and opaque passes — the image is the
    one of a context that never overflowed; a second application of the in-place modulation would show as a darker image."""
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.atrium_scene(320, 180, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    ref = HipDevice(parity_tap=True)
    ref.set_ssao()
    ref, st_ref = helpers.hip_frame(model, oracle_lut, dev=ref)
    small = HipDevice(parity_tap=True, small_bin_list=True)
    small.set_ssao()
    small, st = helpers.hip_frame(model, oracle_lut, dev=small)
    assert st["bin_overflow_retries"] >= 1 and st_ref["bin_overflow_retries"] == 0, (st, st_ref)
    off, _ = helpers.hip_frame(model, oracle_lut)
    want16, got16, off16 = ref.read_opaque(), small.read_opaque(), off.read_opaque()
    assert (want16 != off16).any(axis=-1).sum() >= 0.05 * sc.width * sc.height
    assert (got16 == want16).all(), int((got16 != want16).any(axis=-1).sum())
    assert (_bits(small.read_opaque_f32()) == _bits(ref.read_opaque_f32())).all()
    for a, b in zip(small.read_ssao(), ref.read_ssao()):
        assert (_bits(a) == _bits(b)).all()
    ref.close(); small.close(); off.close()


def test_on_then_off_is_a_context_that_never_had_it(oracle_lut):
    W, H = 33, 17
    model = helpers.build_model(sr.corner(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    never = dev.read_opaque(), dev.read_opaque_f32()
    dev.set_ssao()
    _frame(dev, model)
    assert (dev.read_opaque() != never[0]).any(axis=-1).sum() >= 100
    dev.set_ssao(None)
    _frame(dev, model)
    assert (dev.read_opaque() == never[0]).all() and (_bits(dev.read_opaque_f32()) == _bits(never[1])).all()
    dev.close()


def test_hud_pixels_stay_cleared(oracle_lut):
    """A HUD triangle's pixel is left cleared by the opaque pass, and stays so: the occlusion multiplies what is there.  Everywhere else the image is the
    modulated SSAO-off image, with the depth of the WORLD's keys under the HUD meshes."""
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.hud_scene(160, 90, tex_size=16)
    model = helpers.build_model(sc)
    off, _ = helpers.hip_frame(model, oracle_lut, hud=True)
    on = HipDevice(parity_tap=True)
    on.set_ssao(radius=1.0)
    on, _ = helpers.hip_frame(model, oracle_lut, dev=on, hud=True)
    off16, on16 = off.read_opaque(), on.read_opaque()
    want = _assert_layers(on, bytes(model.camera_bytes), {"radius": 1.0})
    cleared = (off16 == 0).all(axis=-1)
    assert cleared.sum() >= 200 and (cleared & want["hit"]).sum() >= 50                      # HUD meshes, some of them over world geometry
    assert (on16[cleared] == 0).all()
    _assert_image(on16, off16, want)
    assert (on16 != off16).any(axis=-1).sum() >= 100
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H = 33, 17
    model = helpers.build_model(sr.corner(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    with pytest.raises(AwsmHipError) as e:                                                   # no frame with SSAO on yet
        dev.read_ssao()
    assert e.value.code == -5                                                                # AWSM_ERR_NOT_READY
    dev.set_ssao(radius=0.4)
    with pytest.raises(AwsmHipError) as e:                                                   # set, but no opaque pass since
        dev.read_ssao()
    assert e.value.code == -5
    _frame(dev, model)
    block = bytes(model.camera_bytes)
    _assert_layers(dev, block, {"radius": 0.4})
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(intensity=float("inf")), dict(bias=float("nan")), dict(strength=1.5),
                dict(strength=-0.1), dict(struct_size=2), dict(struct_size=5000)):
        with pytest.raises(AwsmHipError) as e:
            dev.set_ssao(**bad)
        assert e.value.code == -1, bad                                                       # AWSM_ERR_INVALID_ARGUMENT
    _frame(dev, model)
    _assert_layers(dev, block, {"radius": 0.4})                                              # a refused record changes nothing
    dev.set_ssao(struct_size=8, radius=0.3, intensity=9.0)                                   # only the radius is known: the rest keeps its defaults
    _frame(dev, model)
    _assert_layers(dev, block, {"radius": 0.3})
    dev.close()
    for shard in ("rows", "bands"):
        dev = HipDevice(parity_tap=True)
        dev.set_ssao()
        dev.resize(W, H, 0)
        if shard == "rows":
            dev.set_shard_rows(0, 9)
        else:
            dev.set_shard_bands(2, 0)
        dev.upload_mirrors(model.mirrors())
        for i, smp in enumerate(model.scene.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(model.scene.skybox_rgba, model.scene.prefiltered_rgb, model.scene.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        dev.geometry_pass(model.collect_draws())
        with pytest.raises(AwsmHipError) as e:
            dev.opaque_pass()
        assert e.value.code == -6, shard                                                     # AWSM_ERR_UNSUPPORTED
        dev.set_ssao(None)
        dev.opaque_pass(); dev.frame_end()                                                   # off: the shard renders as ever
        dev.close()


# ------------------------------------------------------------------------------------------------ through the host

def test_ssao_through_the_host_layer(oracle_lut):
    """Host.set_ssao, render(), read_opaque: the bits of driving the C-ABI directly; a post pass after it reads the modulated image."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H = 70, 45
    sc = sr.boxes(W, H)
    model = helpers.build_model(sc)
    direct = HipDevice(parity_tap=True)
    direct.set_ssao(radius=0.6, intensity=1.5)
    direct, _ = helpers.hip_frame(model, oracle_lut, dev=direct)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.set_post_processing(1)
    r.render(sync=True)
    display_off, off16 = dev.read_display(), dev.read_opaque()
    r.set_ssao(True, radius=0.6, intensity=1.5)
    r.render(sync=True)
    block = dev.buffer_read(BUF_CAMERA, 0, 512)
    want = _assert_layers(dev, block, {"radius": 0.6, "intensity": 1.5})
    got16 = dev.read_opaque()
    _assert_image(got16, off16, want)
    assert (got16 == direct.read_opaque()).all()
    moved = (dev.read_display() != display_off).any(axis=-1)
    assert not moved[want["m"] == 1.0].any() and (want["m"] < 0.8).sum() >= 100 and moved[want["m"] < 0.8].mean() > 0.9
    r.set_ssao(False)
    r.render(sync=True)
    assert (dev.read_opaque() == off16).all() and (dev.read_display() == display_off).all()
    r.close(); direct.close()
