"""GPU tests of the shadows: the light's map bit for bit against the CPU oracle's raster of the casters from the light block, the
layers V and m and the modulated opaque image bit for bit against tests/shadow_reference.py fed the device's own keys and map, with SSAO behind
it, under MSAA x4, under a transparent pass, with HUD meshes, in overlap mode, through a replayed frame, and the refusals."""
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc
from oracle import oracle_lib
from tests import helpers
from tests import shadow_reference as shr
from tests import ssao_reference as sr

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
LIGHTS = ("sun", "spot")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _point(model, cam):
    sc = model.scene
    sr.set_camera(sc, sr.camera(cam, sc.width, sc.height))
    model.update_camera()
    return bytes(model.camera_bytes)


def _params(light, S, **params):
    return dict(params, map_size=S, light=shr.light_vec(light))


def _frame(dev, model, light=None, S=96, params=None, casters=None, transparent=False, hud=False, end=True, block=None):
    """One more frame on a device helpers.hip_frame set up, with the model's camera as it is now; light: a name of shr.LIGHTS (or a dict of its
    kind) -> the shadow pass between the geometry pass and the opaque pass.  -> the light block."""
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    draws = model.collect_draws()
    dev.geometry_pass(draws)
    if hud:
        dev.hud_geometry_pass(model.hud_geometry_draws)
    if light is not None:
        block = shr.light_block(light, S) if block is None else block
        dev.shadow_pass(block, draws if casters is None else casters, **_params(light, S, **(params or {})))
    dev.opaque_pass()
    if transparent or hud:
        dev.transparent_pass(model.collect_transparent_draws())
    if hud:
        dev.hud_transparent_pass(model.hud_transparent_draws)
    if end:
        dev.frame_end()
    return block


def _want(dev, cam_block, light_block, light, S, params=None):
    """The restatement fed the device's own keys, its own map and the two blocks the test wrote."""
    H, W = dev.height, dev.width
    return shr.shadow(dev.read_visibility(), cam_block, W, H, dev.read_shadow_map(S), light_block, S, _params(light, S, **(params or {})))


def _assert_layers(dev, cam_block, light_block, light, S, params=None, what=""):
    want = _want(dev, cam_block, light_block, light, S, params)
    V, m = dev.read_shadow()
    for name, got, ref in (("V", V, want["V"]), ("m", m, want["m"])):
        bad = _bits(got) != _bits(ref)
        at = tuple(np.argwhere(bad)[0]) if bad.any() else None
        assert not bad.any(), "%s %s: %d of %d pixels differ, first at %s: device %r, restatement %r" % (what, name, int(bad.sum()), bad.size, at, got[at], ref[at])
    return want


def _assert_image(on16, off16, want, on32=None, off32=None, what=""):
    ref = shr.apply(off16, want["m"], want["hit"])
    bad = (on16 != ref).any(axis=-1)
    at = tuple(np.argwhere(bad)[0]) if bad.any() else None
    assert not bad.any(), "%s: %d pixels of the opaque image differ, first at %s: device %s, off %s, restatement %s, m %r" % (
        what, int(bad.sum()), at, on16[at], off16[at], ref[at], want["m"][at])
    assert (on16[..., 3] == off16[..., 3]).all() and (on16[~want["hit"]] == off16[~want["hit"]]).all()
    if on32 is not None:
        ref32 = shr.apply_f32(off32, want["m"], want["hit"])
        assert (_bits(on32) == _bits(ref32)).all(), "%s: %d pixels of the f32 opaque image differ" % (what, int((_bits(on32) != _bits(ref32)).any(axis=-1).sum()))


# ------------------------------------------------------------------------------------------------ the map

@pytest.mark.parametrize("S", shr.MAP_SIZES)
@pytest.mark.parametrize("light", LIGHTS)
def test_map_is_the_oracles_raster_of_the_casters(light, S, oracle_lut):
    """The S x S keys bit for bit: 40 is one tile and a ragged second, 96 three by three, 200 a ragged seventh.  Then n = 0: all ones, all lit."""
    W, H = 33, 17
    model = helpers.build_model(sr.boxes(W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    world = dev.read_visibility()
    block = _frame(dev, model, light, S)
    want = shr.caster_map(model, block, S)
    got = dev.read_shadow_map()
    assert got.shape == (S, S) and (want != shr.NO_HIT).mean() > 0.3
    assert (got == want).all(), "%d of %d keys differ" % (int((got != want).sum()), S * S)
    assert (dev.read_visibility() == world).all()                                            # the world's keys are the world pass's
    # a subset of the draws casts: the first draw of the list stays out
    draws = model.collect_draws()
    _frame(dev, model, light, S, casters=draws[1:])
    part = shr.caster_map(model, block, S, draws[1:])
    assert (dev.read_shadow_map() == part).all() and (part != want).sum() > 50
    _frame(dev, model, light, S, casters=[])
    assert (dev.read_shadow_map() == shr.NO_HIT).all()
    V, m = dev.read_shadow()
    assert (V == 1.0).all() and (m == 1.0).all()
    dev.close()


# ------------------------------------------------------------------------------------------------ layers and image, bit for bit

@pytest.mark.parametrize("scene", ["corner", "boxes"])
@pytest.mark.parametrize("W,H", shr.SIZES)
def test_layers_are_the_f32_restatement_bit_for_bit(W, H, scene, oracle_lut):
    """V and m of every pixel under the five cameras, both lights and R = 0, 1, 2 (the map size goes round with R)."""
    model = helpers.build_model(sr.SCENES[scene](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dark = partial = 0
    for cam in sr.CAMERAS:
        cam_block = _point(model, cam)
        for light in LIGHTS:
            for R in (0, 1, 2):
                S = shr.MAP_SIZES[R]
                lb = _frame(dev, model, light, S, {"pcf_radius": R})
                want = _assert_layers(dev, cam_block, lb, light, S, {"pcf_radius": R}, what="%s %s %s R=%d %dx%d" % (scene, cam, light, R, W, H))
                dark += int((want["V"] == 0.0).sum()); partial += int(((want["V"] > 0.0) & (want["V"] < 1.0)).sum())
    assert scene == "corner" or (dark >= 20 and partial >= 20)
    dev.close()


PARAMETER_RECORDS = ({}, {"bias": 0.02}, {"slope_bias": 0.0, "max_slope": 0.0}, {"max_slope": 0.0003}, {"strength": 1.0, "facing_fade": 0.6},
                     {"bias": 0.0, "slope_bias": 2.5, "max_slope": 0.2, "strength": 0.35, "facing_fade": 0.02, "pcf_radius": 2})


def test_parameters_reach_the_kernel(oracle_lut):
    W, H, S = 33, 17, 96
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    off = dev.read_opaque()
    cam_block = bytes(model.camera_bytes)
    for light in LIGHTS:
        base = None
        for params in PARAMETER_RECORDS:
            lb = _frame(dev, model, light, S, params)
            want = _assert_layers(dev, cam_block, lb, light, S, params, what="%s %s" % (light, params))
            _assert_image(dev.read_opaque(), off, want, what="%s %s" % (light, params))
            base = want["m"] if base is None else base
            assert not params or (want["m"] != base).sum() >= 10, (light, params)
        lb = _frame(dev, model, light, S, {"strength": 0.0})
        want = _assert_layers(dev, cam_block, lb, light, S, {"strength": 0.0})
        assert (want["m"] == 1.0).all() and (want["V"] < 1.0).sum() >= 50 and (dev.read_opaque() == off).all()
    dev.close()


@pytest.mark.parametrize("scene", ["corner", "boxes"])
def test_opaque_image_is_the_modulated_shadowless_image(scene, oracle_lut):
    """RGBA16F and the f32 parity tap against f16_rne(f32(off) * m) / off * m, `off` from a context that never had a shadow pass; alpha and
    pixels nothing hit are untouched; the world's keys are unchanged."""
    W, H, S = 70, 45, 96
    model = helpers.build_model(sr.SCENES[scene](W, H))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    moved = 0
    for cam in sr.CAMERAS:
        cam_block = _point(model, cam)
        for light in LIGHTS:
            lb = _frame(on, model, light, S); _frame(off, model)
            want = _assert_layers(on, cam_block, lb, light, S, what="%s %s %s" % (scene, cam, light))
            on16, off16 = on.read_opaque(), off.read_opaque()
            _assert_image(on16, off16, want, on.read_opaque_f32(), off.read_opaque_f32(), what="%s %s %s" % (scene, cam, light))
            assert (on.read_visibility() == off.read_visibility()).all()
            moved += int((on16 != off16).any(axis=-1).sum())
    assert moved >= 0.1 * W * H
    on.close(); off.close()


def test_ssao_multiplies_the_shadowed_image(oracle_lut):
    """Both on: the image is SSAO's apply of shadow's apply of the plain image, in that order (each rounds to f16)."""
    W, H, S = 70, 45, 96
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    on.set_ssao()
    cam_block = bytes(model.camera_bytes)
    lb = _frame(on, model, "sun", S)
    want = _assert_layers(on, cam_block, lb, "sun", S)
    ao = sr.ssao(on.read_visibility(), cam_block, W, H)
    off16 = off.read_opaque()
    first = shr.apply(off16, want["m"], want["hit"])
    both = sr.apply(first, ao["m"], ao["hit"])
    other = shr.apply(sr.apply(off16, ao["m"], ao["hit"]), want["m"], want["hit"])
    assert (on.read_opaque() == both).all(), int((on.read_opaque() != both).any(axis=-1).sum())
    assert (both != other).any(axis=-1).sum() >= 5                                           # the order shows
    ref32 = sr.apply_f32(shr.apply_f32(off.read_opaque_f32(), want["m"], want["hit"]), ao["m"], ao["hit"])
    assert (_bits(on.read_opaque_f32()) == _bits(ref32)).all()
    on.close(); off.close()


@pytest.mark.parametrize("W,H", shr.SIZES[1:])
def test_msaa_takes_the_least_of_the_four_sample_depths(W, H, oracle_lut):
    S = 96
    model = helpers.build_model(sr.boxes(W, H))
    on, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    off, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    for cam in ("perspective", "closeup"):
        cam_block = _point(model, cam)
        for light in LIGHTS:
            lb = _frame(on, model, light, S); _frame(off, model)
            assert on.read_visibility().shape == (H, W, 4)
            want = _assert_layers(on, cam_block, lb, light, S, what="msaa %s %s %dx%d" % (cam, light, W, H))
            assert (on.read_shadow_map() == shr.caster_map(model, lb, S)).all()              # the map is single-sampled
            _assert_image(on.read_opaque(), off.read_opaque(), want, on.read_opaque_f32(), off.read_opaque_f32(), what="msaa %s %s" % (cam, light))
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ what reads the opaque image afterwards

def _glass_scene(W, H):
    """`boxes` under the close-up camera with a transmissive quad standing between it and the shadowed floor."""
    sc = sr.boxes(W, H, "closeup")
    sc.materials.append(MaterialDesc(base_color_factor=(0.95, 0.98, 1.0, 1.0), transmission={"factor": 0.95}, metallic_factor=0.0, roughness_factor=0.1))
    quad = dataclasses.replace(sr._quad((0.15, 0.02, 0.6), (0.45, 0.0, -0.45), (0.0, 0.5, 0.0), 0), material=len(sc.materials) - 1)
    sc.nodes.append(NodeDesc(primitives=[quad]))
    return sc


def test_transparent_pass_reads_the_shadowed_image(oracle_lut):
    """Refraction sees the shadow; the quad itself neither casts nor is darkened."""
    W, H, S = 70, 45, 96
    model = helpers.build_model(_glass_scene(W, H))
    draws = model.collect_draws()
    assert len(model.collect_transparent_draws()) == 1
    on, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    off, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    lb = _frame(on, model, "sun", S, transparent=True)
    assert (on.read_shadow_map() == shr.caster_map(model, lb, S, draws)).all()               # the opaque draws alone
    touched = (off.read_composite() != off.read_opaque()).any(axis=-1)
    assert 150 <= touched.sum() <= 0.5 * W * H
    want = _assert_layers(on, bytes(model.camera_bytes), lb, "sun", S)
    on_opaque, on_comp, off_comp = on.read_opaque(), on.read_composite(), off.read_composite()
    _assert_image(on_opaque, off.read_opaque(), want)
    assert (on_comp[~touched] == on_opaque[~touched]).all()                                  # the blit took the shadowed image
    behind = touched & (want["m"] < 0.6)
    assert behind.sum() >= 20 and (on_comp != off_comp).any(axis=-1)[behind].mean() > 0.5
    on.close(); off.close()


def test_hud_pixels_stay_cleared(oracle_lut):
    """A HUD mesh over a shadowed pixel: the opaque pass left it cleared and it stays so; the layers come from the WORLD's keys under it."""
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.hud_scene(160, 90, tex_size=16)
    model = helpers.build_model(sc)
    off, _ = helpers.hip_frame(model, oracle_lut, hud=True)
    on, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True), hud=True)
    S = 200
    eye = tuple(float(v) for v in np.asarray(sc.camera_position, np.float64) + np.array([1.5, 2.5, 0.5]))
    light = dict(kind="spot", position=eye, target=(0.0, 0.5, 0.0), fovy_deg=80.0, near=0.2, far=40.0)
    lb = _frame(on, model, light, S, hud=True)
    off16, on16 = off.read_opaque(), on.read_opaque()
    want = _assert_layers(on, bytes(model.camera_bytes), lb, light, S)
    cleared = (off16 == 0).all(axis=-1)
    assert cleared.sum() >= 200 and (cleared & want["hit"] & (want["m"] < 1.0)).sum() >= 20  # HUD meshes, some of them over shadowed world pixels
    assert (on16[cleared] == 0).all()
    _assert_image(on16, off16, want)
    assert (on16 != off16).any(axis=-1).sum() >= 100
    on.close(); off.close()


@pytest.mark.parametrize("W,H,S", [(70, 45, 96), (1920, 1080, 2048)])
def test_each_overlapped_frame_is_its_synchronous_twin(W, H, S, oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES, four frames with a moving light and camera, enqueue-only, each into its own image: frame i + 2's shadow pass
    overwrites the map of frame i's slot and must wait until frame i's resolve has read it."""
    import torch
    from awsm_renderer_amd.hip_backend import HipDevice
    small = W * H < 10000
    model = helpers.build_model(sr.boxes(W, H))
    draws = model.collect_draws()
    eyes = [(3.2 - 0.35 * i, 2.6 + 0.1 * i, 3.6 - 0.2 * i) for i in range(4)]
    blocks = [sr.camera_block(eye, (0.6, 0.5, 0.6), W, H) for eye in eyes]
    suns = [dict(shr.LIGHTS["sun"], towards=(0.45 - 0.25 * i, 0.8, 0.35 + 0.2 * i)) for i in range(4)]
    lbs = [shr.light_block(sun, S) for sun in suns]
    dev, _ = helpers.hip_frame(model, oracle_lut)
    want = []
    for block, sun, lb in zip(blocks, suns, lbs):
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.geometry_pass(draws); dev.shadow_pass(lb, draws, **_params(sun, S)); dev.opaque_pass(); dev.frame_end()
        if small:
            _assert_layers(dev, block, lb, sun, S)
        want.append(dev.read_opaque())
    dev.close()
    assert all((want[i] != want[i + 1]).any(axis=-1).sum() >= 0.25 * W * H for i in range(3))
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    images = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in blocks]
    for block, sun, lb, image in zip(blocks, suns, lbs, images):                              # no frame_end between the frames
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.bind_output(image.data_ptr(), H * W * 8)
        dev.geometry_pass(draws); dev.shadow_pass(lb, draws, **_params(sun, S)); dev.opaque_pass()
    dev.frame_end()
    torch.cuda.synchronize()
    for i, image in enumerate(images):
        got = image.cpu().numpy().view(np.uint16)
        assert (got == want[i]).all(), (i, int((got != want[i]).any(axis=-1).sum()))
    if small:
        _assert_layers(dev, blocks[-1], lbs[-1], suns[-1], S)
    dev.close()


def _atrium_light(S):
    light = dict(kind="spot", position=(1.0, 8.5, 12.0), target=(0.0, 0.0, -4.0), fovy_deg=95.0, near=0.2, far=60.0)
    return light, shr.light_block(light, S)


def test_replayed_shadow_pass_gives_the_frame_of_a_context_that_never_overflowed(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST: the shadow pass overflows its (triangle, tile) list too; frame_end replays it in order with the others and the opaque
    pass behind it — map, layers and image are those of a context with room; a second application of the in-place multiply would show darker."""
    from awsm_renderer_amd.hip_backend import HipDevice
    S = 512
    sc = scenes.atrium_scene(320, 180, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    light, lb = _atrium_light(S)
    ref, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True))
    small, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, small_bin_list=True))
    off16 = ref.read_opaque()
    before = small.frame_end()["bin_overflow_retries"]
    _frame(ref, model, light, S, block=lb, end=False); st_ref = ref.frame_end()
    _frame(small, model, light, S, block=lb, end=False); st = small.frame_end()
    assert st["bin_overflow_retries"] > before and st_ref["bin_overflow_retries"] == 0, (st, st_ref, before)
    assert (small.read_shadow_map() == ref.read_shadow_map()).all() and (ref.read_shadow_map() != shr.NO_HIT).mean() > 0.5
    want16, got16 = ref.read_opaque(), small.read_opaque()
    assert (want16 != off16).any(axis=-1).sum() >= 0.05 * sc.width * sc.height
    assert (got16 == want16).all(), int((got16 != want16).any(axis=-1).sum())
    assert (_bits(small.read_opaque_f32()) == _bits(ref.read_opaque_f32())).all()
    for a, b in zip(small.read_shadow(), ref.read_shadow()):
        assert (_bits(a) == _bits(b)).all()
    ref.close(); small.close()


def test_a_frame_without_the_pass_is_a_context_that_never_had_it(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError
    W, H = 33, 17
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    never = dev.read_opaque(), dev.read_opaque_f32()
    _frame(dev, model, "sun", 96)
    assert (dev.read_opaque() != never[0]).any(axis=-1).sum() >= 50
    _frame(dev, model)
    assert (dev.read_opaque() == never[0]).all() and (_bits(dev.read_opaque_f32()) == _bits(never[1])).all()
    for read in (dev.read_shadow, lambda: dev.read_shadow_map(96)):
        with pytest.raises(AwsmHipError) as e:
            read()
        assert e.value.code == -5
    dev.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H, S = 33, 17, 40
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    draws = model.collect_draws()
    lb = shr.light_block("sun", S)
    good = _params("sun", S)

    def refused(code, block=lb, **kw):
        with pytest.raises(AwsmHipError) as e:
            dev.shadow_pass(block, draws, **dict(good, **kw))
        assert e.value.code == code, (kw, e.value.code)

    for read in (dev.read_shadow, lambda: dev.read_shadow_map(S)):                           # no frame with the pass yet
        with pytest.raises(AwsmHipError) as e:
            read()
        assert e.value.code == -5                                                            # AWSM_ERR_NOT_READY
    refused(-5)                                                                              # after the frame's opaque pass
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    dev.geometry_pass(draws)
    dev.shadow_pass(lb, draws, **good)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(map_size=0), dict(map_size=8193), dict(pcf_radius=3), dict(strength=1.5), dict(strength=-0.1), dict(facing_fade=0.0), dict(facing_fade=-1.0),
                dict(max_slope=-0.01), dict(light=(0.0, 1.0, 0.0, 0.5)), dict(light=(0.0, 1.0, 0.0, 2.0)), dict(light=(nan, 1.0, 0.0, 0.0)), dict(bias=nan),
                dict(slope_bias=inf), dict(max_slope=inf), dict(strength=nan), dict(facing_fade=nan), dict(struct_size=2), dict(struct_size=5000)):
        refused(-1, **bad)                                                                   # AWSM_ERR_INVALID_ARGUMENT
    refused(-1, block=lb[:508])
    refused(-1, block=lb + bytes(4))
    poisoned = np.frombuffer(lb, np.float32).copy(); poisoned[35] = np.nan
    refused(-1, block=poisoned.tobytes())
    dev.opaque_pass()
    with pytest.raises(AwsmHipError) as e:                                                   # the window has closed
        dev.shadow_pass(lb, draws, **good)
    assert e.value.code == -5
    dev.frame_end()
    _assert_layers(dev, bytes(model.camera_bytes), lb, "sun", S)                             # the refused calls changed nothing
    dev.geometry_pass(draws)
    dev.shadow_pass(lb, draws, **good)
    with pytest.raises(AwsmHipError) as e:                                                   # the pass, but no opaque pass behind it yet
        dev.read_shadow()
    assert e.value.code == -5
    assert dev.read_shadow_map().shape == (S, S)
    dev.opaque_pass(has_opaque=False)
    with pytest.raises(AwsmHipError) as e:                                                   # an opaque pass with nothing to shade resolves nothing
        dev.read_shadow()
    assert e.value.code == -5
    dev.frame_end()
    dev.close()
    for shard in ("rows", "bands"):
        dev = HipDevice(parity_tap=True)
        dev.resize(W, H, 0)
        if shard == "rows":
            dev.set_shard_rows(0, 9)
        else:
            dev.set_shard_bands(2, 0)
        dev.upload_mirrors(model.mirrors())
        for i, smp in enumerate(model.scene.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(model.scene.skybox_rgba, model.scene.prefiltered_rgb, model.scene.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        dev.geometry_pass(draws)
        with pytest.raises(AwsmHipError) as e:
            dev.shadow_pass(lb, draws, **good)
        assert e.value.code == -6, shard                                                     # AWSM_ERR_UNSUPPORTED
        dev.opaque_pass(); dev.frame_end()                                                   # without it the shard renders as ever
        dev.close()


# ------------------------------------------------------------------------------------------------ through the host

def test_shadows_through_the_host_layer(oracle_lut):
    """Renderer.set_shadow, render(): the map is the oracle's raster of the casters awsm_host_shadow_camera reports from the block it reports, the
    layers and the image are the restatement's with that block; off again gives the image of before."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H, S = 70, 45, 200
    sc = sr.boxes(W, H, "closeup")
    sun = {"kind": "directional", "color": (1.0, 0.97, 0.92), "intensity": 1.4, "direction": tuple(float(-c) for c in shr._SUN)}
    spot = {"kind": "spot", "color": (1.0, 1.0, 1.0), "intensity": 20.0, "position": (3.0, 3.2, 2.2), "direction": (-2.0, -3.2, -1.2), "range": 0.0,
            "inner_angle": 0.9063, "outer_angle": 0.8192}      # cosines of 25 and 35 degrees
    sc.lights = [sun, spot]
    model = helpers.build_model(sc)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.render(sync=True)
    off16 = dev.read_opaque()
    for index, light in enumerate(sc.lights):
        r.set_shadow(index, map_size=S, pcf_radius=2, strength=0.9)
        r.render(sync=True)
        block, casters = r.host.shadow_camera()
        assert len(casters) == 6
        got_map = dev.read_shadow_map(S)
        assert (got_map == shr.caster_map(model, block, S, casters)).all() and (got_map != shr.NO_HIT).mean() > 0.2
        vec = shr.host_light_camera(light, shr.scene_aabbs(sc))["light"]
        params = {"pcf_radius": 2, "strength": 0.9, "light": tuple(float(np.float32(c)) for c in vec), "map_size": S}
        cam_block = dev.buffer_read(BUF_CAMERA, 0, 512)
        want = shr.shadow(dev.read_visibility(), cam_block, W, H, got_map, block, S, params)
        V, m = dev.read_shadow()
        assert (_bits(V) == _bits(want["V"])).all() and (_bits(m) == _bits(want["m"])).all()
        assert (want["V"] == 0.0).sum() >= 50 and (want["V"] == 1.0).sum() >= 1000
        _assert_image(dev.read_opaque(), off16, want, what=light["kind"])
    r.set_shadow(False)
    r.render(sync=True)
    assert (dev.read_opaque() == off16).all()
    r.close()
