"""GPU tests of the shadows from several views: every layer of the stack bit for bit against the CPU oracle's raster of its view, the
layers V, m and the view byte bit for bit against tests/shadow_views_reference.py fed the device's own keys and maps, one view against
awsm_hip_shadow_pass, the image against a context that never had the pass, SSAO behind it, MSAA x4, overlap mode, a replayed frame, the two entries and
no pass in turn on one context, and the refusals."""
import numpy as np
import pytest

from awsm_renderer_amd import scenes
from oracle import oracle_lib
from tests import helpers
from tests import shadow_reference as shr
from tests import shadow_views_reference as svr
from tests import ssao_reference as sr

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
MAP_SIZES = (40, 96)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _point(model, cam):
    sc = model.scene
    sr.set_camera(sc, sr.camera(cam, sc.width, sc.height))
    model.update_camera()
    return bytes(model.camera_bytes)


def _frame(dev, model, views=None, S=96, light=None, params=None, end=True):
    """One more frame on a device helpers.hip_frame set up, with the model's camera as it is now.  views: [(block, casters or None = every draw)]
    -> shadow_pass_views between the geometry pass and the opaque pass."""
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    draws = model.collect_draws()
    dev.geometry_pass(draws)
    if views is not None:
        dev.shadow_pass_views([(b, draws if c is None else c) for b, c in views], **dict(params or {}, map_size=S, light=light))
    dev.opaque_pass()
    if end:
        dev.frame_end()


def _want(dev, cam_block, blocks, S, light, params=None):
    """The restatement fed the device's own keys, its own layers and the blocks the test wrote."""
    H, W = dev.height, dev.width
    maps = [dev.read_shadow_map(S, view=i) for i in range(len(blocks))]
    return svr.shadow_views(dev.read_visibility(), cam_block, W, H, maps, list(blocks), S, dict(params or {}, light=light))


def _assert_layers(dev, cam_block, blocks, S, light, params=None, what=""):
    want = _want(dev, cam_block, blocks, S, light, params)
    V, m = dev.read_shadow()
    for name, got, ref in (("V", V, want["V"]), ("m", m, want["m"])):
        bad = _bits(got) != _bits(ref)
        at = tuple(np.argwhere(bad)[0]) if bad.any() else None
        assert not bad.any(), "%s %s: %d of %d pixels differ, first at %s: device %r, restatement %r" % (what, name, int(bad.sum()), bad.size, at, got[at], ref[at])
    view = dev.read_shadow_view()
    bad = view != want["view"]
    assert not bad.any(), "%s view: %d pixels differ, first at %s" % (what, int(bad.sum()), tuple(np.argwhere(bad)[0]))
    return want


def _assert_image(on16, off16, want, on32=None, off32=None, what=""):
    ref = shr.apply(off16, want["m"], want["hit"])
    bad = (on16 != ref).any(axis=-1)
    assert not bad.any(), "%s: %d pixels of the opaque image differ" % (what, int(bad.sum()))
    assert (on16[..., 3] == off16[..., 3]).all() and (on16[~want["hit"]] == off16[~want["hit"]]).all()
    if on32 is not None:
        assert (_bits(on32) == _bits(shr.apply_f32(off32, want["m"], want["hit"]))).all(), "%s: the f32 opaque image differs" % what


def _cube(position, S, R):
    return svr.cube_face_blocks(position, S, R, near=0.05, far=10.0), svr.point_light(position)


def _configs(S, R, scene):
    """name -> (blocks, AwsmShadow.light): the cascade pair of the CPU known answer, the host's four cascades of the sun under the scene's camera as
    it is now, four nested windows of the sun around the boxes, the cube at both positions."""
    out = {"pair": (svr.cascade_pair(S), shr.light_vec("zenith")), "host4": (svr.host_sun_cascades(scene, S), shr.light_vec("sun")),
           "sun4": (svr.sun_windows(S), shr.light_vec("sun"))}
    for i, position in enumerate(svr.POINT_POSITIONS):
        out["cube%d" % i] = _cube(position, S, R)
    return out


# ------------------------------------------------------------------------------------------------ a. the layers

@pytest.mark.parametrize("S", MAP_SIZES)
def test_every_layer_is_the_oracles_raster_of_its_view(S, oracle_lut):
    """K = 2, 4 and 6 views, a view with no casters and one with a part of the draws among them; read_shadow_map is layer 0; a view the pass did not
    have is refused; the world's keys are the world pass's."""
    from awsm_renderer_amd.hip_backend import AwsmHipError
    W, H = 33, 17
    model = helpers.build_model(sr.boxes(W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    world = dev.read_visibility()
    draws = model.collect_draws()
    cube, point = _cube(svr.POINT_POSITIONS[0], S, 1)
    sets = {2: [(shr.light_block("sun", S), None), (shr.light_block("spot", S), [])],
            4: [(b, c) for b, c in zip(svr.sun_windows(S), (None, draws[1:], [], None))],
            6: [(b, draws[2:] if i == 3 else None) for i, b in enumerate(cube)]}
    for K, views in sets.items():
        _frame(dev, model, views, S, light=point if K == 6 else shr.light_vec("sun"))
        filled = 0
        for i, (block, casters) in enumerate(views):
            want = shr.caster_map(model, block, S, draws if casters is None else casters)
            got = dev.read_shadow_map(view=i)
            assert got.shape == (S, S) and (got == want).all(), "K = %d view %d: %d of %d keys differ" % (K, i, int((got != want).sum()), S * S)
            filled += int((want != shr.NO_HIT).sum())
            if i == 0:
                assert (dev.read_shadow_map() == want).all()
        assert filled > 0.3 * S * S
        with pytest.raises(AwsmHipError) as e:
            dev.read_shadow_map(view=K)
        assert e.value.code == -1
        assert (dev.read_visibility() == world).all()
    dev.close()


# ------------------------------------------------------------------------------------------------ b. layers, bit for bit

@pytest.mark.parametrize("scene", ["corner", "boxes"])
@pytest.mark.parametrize("W,H", shr.SIZES)
def test_layers_and_view_are_the_f32_restatement_bit_for_bit(W, H, scene, oracle_lut):
    """V, m and the view byte of every pixel: the cascade pair, four nested windows under the sun and the cube at both positions, R = 0, 1, 2 (the map
    size goes round with R), under two cameras."""
    model = helpers.build_model(sr.SCENES[scene](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dark = views_seen = 0
    for cam in ("perspective", "closeup"):
        cam_block = _point(model, cam)
        for R in (0, 1, 2):
            S = MAP_SIZES[R % 2]
            for name, (blocks, light) in _configs(S, R, model.scene).items():
                _frame(dev, model, [(b, None) for b in blocks], S, light, {"pcf_radius": R})
                want = _assert_layers(dev, cam_block, blocks, S, light, {"pcf_radius": R}, what="%s %s %s R=%d %dx%d" % (scene, cam, name, R, W, H))
                dark += int((want["V"] == 0.0).sum())
                views_seen += len(np.unique(want["view"][want["hit"]]))
    # (each frame has at least one view; past the smallest size the frames see more than that: the selection is exercised)
    assert views_seen >= 2 * 3 * (5 if W < 33 else 8) and (scene == "corner" or dark >= 20)
    dev.close()


@pytest.mark.parametrize("W,H", shr.SIZES[1:])
def test_msaa_takes_the_least_of_the_four_sample_depths(W, H, oracle_lut):
    S = 96
    model = helpers.build_model(sr.boxes(W, H))
    on, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    off, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    cam_block = _point(model, "closeup")
    for name, (blocks, light) in _configs(S, 1, model.scene).items():
        _frame(on, model, [(b, None) for b in blocks], S, light); _frame(off, model)
        assert on.read_visibility().shape == (H, W, 4)
        want = _assert_layers(on, cam_block, blocks, S, light, what="msaa %s %dx%d" % (name, W, H))
        assert (on.read_shadow_map(view=1) == shr.caster_map(model, blocks[1], S)).all()      # the layers are single-sampled
        _assert_image(on.read_opaque(), off.read_opaque(), want, on.read_opaque_f32(), off.read_opaque_f32(), what="msaa " + name)
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ c. one view is the old entry

@pytest.mark.parametrize("light", ["sun", "spot"])
def test_one_view_is_shadow_pass_bit_for_bit(light, oracle_lut):
    """V, m, the image and its f32 tap; the view byte is 0 where the pixel is inside the map and 255 elsewhere."""
    W, H = 70, 45
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    new, _ = helpers.hip_frame(model, oracle_lut)
    old, _ = helpers.hip_frame(model, oracle_lut)
    draws = model.collect_draws()
    for R in (0, 1, 2):
        S = MAP_SIZES[R % 2]
        lb, vec = shr.light_block(light, S), shr.light_vec(light)
        _frame(new, model, [(lb, None)], S, vec, {"pcf_radius": R})
        old.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
        old.geometry_pass(draws); old.shadow_pass(lb, draws, map_size=S, light=vec, pcf_radius=R); old.opaque_pass(); old.frame_end()
        for a, b in zip(new.read_shadow(), old.read_shadow()):
            assert (_bits(a) == _bits(b)).all(), (light, R)
        assert (new.read_shadow_map() == old.read_shadow_map()).all()
        assert (new.read_opaque() == old.read_opaque()).all() and (_bits(new.read_opaque_f32()) == _bits(old.read_opaque_f32())).all()
        want = shr.shadow(old.read_visibility(), bytes(model.camera_bytes), W, H, old.read_shadow_map(), lb, S, {"pcf_radius": R, "light": vec})
        assert (new.read_shadow_view() == np.where(want["inside"], 0, svr.NO_VIEW)).all() and (want["V"] < 1.0).sum() >= 50
    new.close(); old.close()


# ------------------------------------------------------------------------------------------------ d. the image

def test_the_image_is_the_modulated_shadowless_image_and_ssao_follows(oracle_lut):
    """RGBA16F and the f32 tap against apply(off, m), `off` from a context that never had the pass; with SSAO on, SSAO's apply of that (§19's order)."""
    W, H, S = 70, 45, 96
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    cam_block = bytes(model.camera_bytes)
    off16, off32 = off.read_opaque(), off.read_opaque_f32()
    moved = 0
    for name, (blocks, light) in _configs(S, 1, model.scene).items():
        _frame(on, model, [(b, None) for b in blocks], S, light)
        want = _assert_layers(on, cam_block, blocks, S, light, what=name)
        on16 = on.read_opaque()
        _assert_image(on16, off16, want, on.read_opaque_f32(), off32, what=name)
        assert (on.read_visibility() == off.read_visibility()).all()
        moved += int((on16 != off16).any(axis=-1).sum())
    assert moved >= 0.1 * W * H
    on.set_ssao()
    blocks, light = _cube(svr.POINT_POSITIONS[1], S, 1)
    _frame(on, model, [(b, None) for b in blocks], S, light)
    want = _assert_layers(on, cam_block, blocks, S, light)
    ao = sr.ssao(on.read_visibility(), cam_block, W, H)
    both = sr.apply(shr.apply(off16, want["m"], want["hit"]), ao["m"], ao["hit"])
    other = shr.apply(sr.apply(off16, ao["m"], ao["hit"]), want["m"], want["hit"])
    assert (on.read_opaque() == both).all() and (both != other).any(axis=-1).sum() >= 5
    ref32 = sr.apply_f32(shr.apply_f32(off32, want["m"], want["hit"]), ao["m"], ao["hit"])
    assert (_bits(on.read_opaque_f32()) == _bits(ref32)).all()
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ e. overlapped frames

def test_each_overlapped_frame_is_its_synchronous_twin(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES, four frames with a moving point light and camera, enqueue-only, each into its own image: frame i + 2's views
    overwrite the layers of frame i's slot and must wait until frame i's resolve has read them."""
    import torch
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H, S = 70, 45, 96
    model = helpers.build_model(sr.boxes(W, H))
    draws = model.collect_draws()
    eyes = [(3.2 - 0.35 * i, 2.6 + 0.1 * i, 3.6 - 0.2 * i) for i in range(4)]
    cams = [sr.camera_block(eye, (0.6, 0.5, 0.6), W, H) for eye in eyes]
    lights = [_cube((0.6 + 0.3 * i, 2.4 - 0.4 * i, 0.6 + 0.2 * i), S, 1) for i in range(4)]
    dev, _ = helpers.hip_frame(model, oracle_lut)
    want = []
    for cam, (blocks, vec) in zip(cams, lights):
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(cam, np.uint8))
        dev.geometry_pass(draws); dev.shadow_pass_views([(b, draws) for b in blocks], map_size=S, light=vec); dev.opaque_pass(); dev.frame_end()
        _assert_layers(dev, cam, blocks, S, vec)
        want.append(dev.read_opaque())
    dev.close()
    assert all((want[i] != want[i + 1]).any(axis=-1).sum() >= 0.25 * W * H for i in range(3))
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    images = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in cams]
    for cam, (blocks, vec), image in zip(cams, lights, images):                                  # no frame_end between the frames
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(cam, np.uint8))
        dev.bind_output(image.data_ptr(), H * W * 8)
        dev.geometry_pass(draws); dev.shadow_pass_views([(b, draws) for b in blocks], map_size=S, light=vec); dev.opaque_pass()
    dev.frame_end()
    torch.cuda.synchronize()
    for i, image in enumerate(images):
        got = image.cpu().numpy().view(np.uint16)
        assert (got == want[i]).all(), (i, int((got != want[i]).any(axis=-1).sum()))
    _assert_layers(dev, cams[-1], lights[-1][0], S, lights[-1][1])
    dev.close()


# ------------------------------------------------------------------------------------------------ f. a replayed frame

def test_a_replayed_pass_of_views_gives_the_frame_of_a_context_that_never_overflowed(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST: the view that sees the atrium overflows its (triangle, tile) list, the view looking away does not; frame_end replays
    every view in order and the opaque pass behind them — layers, V, m, view and image are those of a context with room."""
    from awsm_renderer_amd.hip_backend import HipDevice
    S = 512
    sc = scenes.atrium_scene(320, 180, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    position = (1.0, 8.5, 12.0)
    towards = dict(kind="spot", position=position, target=(0.0, 0.0, -4.0), fovy_deg=95.0, near=0.2, far=60.0)
    away = dict(towards, target=(1.0, 30.0, 12.5), fovy_deg=20.0)
    blocks = [shr.light_block(away, S), shr.light_block(towards, S)]
    vec = svr.point_light(position)
    ref, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True))
    small, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, small_bin_list=True))
    off16 = ref.read_opaque()
    before = small.frame_end()["bin_overflow_retries"]
    _frame(ref, model, [(b, None) for b in blocks], S, vec, end=False); st_ref = ref.frame_end()
    _frame(small, model, [(b, None) for b in blocks], S, vec, end=False); st = small.frame_end()
    assert st["bin_overflow_retries"] > before and st_ref["bin_overflow_retries"] == 0, (st, st_ref, before)
    for i in range(2):
        assert (small.read_shadow_map(view=i) == ref.read_shadow_map(view=i)).all()
    assert (ref.read_shadow_map(view=1) != shr.NO_HIT).mean() > 0.5
    want16, got16 = ref.read_opaque(), small.read_opaque()
    assert (want16 != off16).any(axis=-1).sum() >= 0.05 * sc.width * sc.height
    assert (got16 == want16).all(), int((got16 != want16).any(axis=-1).sum())
    assert (_bits(small.read_opaque_f32()) == _bits(ref.read_opaque_f32())).all()
    for a, b in zip(small.read_shadow(), ref.read_shadow()):
        assert (_bits(a) == _bits(b)).all()
    assert (small.read_shadow_view() == ref.read_shadow_view()).all() and (ref.read_shadow_view() == 1).sum() >= 1000
    ref.close(); small.close()


# ------------------------------------------------------------------------------------------------ g. the two entries and no pass, in turn

def test_views_the_single_map_and_no_pass_in_turn_on_one_context(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError
    W, H, S = 33, 17, 96
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    never = dev.read_opaque(), dev.read_opaque_f32()
    cam_block = bytes(model.camera_bytes)
    draws = model.collect_draws()
    cube, point = _cube(svr.POINT_POSITIONS[1], S, 1)
    lb, sun = shr.light_block("sun", 40), shr.light_vec("sun")
    # every view looks away from the scene, from far outside it: no pixel has a view
    out_there = (40.0, 40.0, 40.0)
    lost = [shr.light_block(dict(kind="spot", position=out_there, target=(80.0, 80.0 + i, 80.0), fovy_deg=30.0, near=0.5, far=20.0), S) for i in range(2)]
    for turn in range(2):
        _frame(dev, model, [(b, None) for b in cube], S, point)
        want = _assert_layers(dev, cam_block, cube, S, point, what="views, turn %d" % turn)
        _assert_image(dev.read_opaque(), never[0], want, dev.read_opaque_f32(), never[1])
        # the single map, of another size
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
        dev.geometry_pass(draws); dev.shadow_pass(lb, draws, map_size=40, light=sun); dev.opaque_pass(); dev.frame_end()
        assert (dev.read_shadow_map() == shr.caster_map(model, lb, 40)).all()
        one = shr.shadow(dev.read_visibility(), cam_block, W, H, dev.read_shadow_map(), lb, 40, {"light": sun})
        V, m = dev.read_shadow()
        assert (_bits(V) == _bits(one["V"])).all() and (_bits(m) == _bits(one["m"])).all()
        _assert_image(dev.read_opaque(), never[0], one, dev.read_opaque_f32(), never[1])
        for read, code in ((dev.read_shadow_view, -5), (lambda: dev.read_shadow_map(view=1), -1)):      # no view layer; one layer
            with pytest.raises(AwsmHipError) as e:
                read()
            assert e.value.code == code
        assert (dev.read_shadow_map(view=0) == dev.read_shadow_map()).all()
        # views in which nothing lies
        _frame(dev, model, [(b, None) for b in lost], S, svr.point_light(out_there))
        assert (dev.read_shadow_view() == svr.NO_VIEW).all()
        V, m = dev.read_shadow()
        assert (V == 1.0).all() and (m == 1.0).all() and (dev.read_opaque() == never[0]).all()
        # no pass
        _frame(dev, model)
        assert (dev.read_opaque() == never[0]).all() and (_bits(dev.read_opaque_f32()) == _bits(never[1])).all()
        for read in (dev.read_shadow, dev.read_shadow_view, lambda: dev.read_shadow_map(S), lambda: dev.read_shadow_map(S, view=0)):
            with pytest.raises(AwsmHipError) as e:
                read()
            assert e.value.code == -5
    dev.close()


# ------------------------------------------------------------------------------------------------ h. refusals

def test_refusals(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H, S = 33, 17, 40
    model = helpers.build_model(sr.boxes(W, H, "closeup"))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    draws = model.collect_draws()
    blocks = svr.cascade_pair(S)
    vec = shr.light_vec("zenith")
    good_views = [(b, draws) for b in blocks]
    good = dict(map_size=S, light=vec)

    def refused(code, views=good_views, **kw):
        with pytest.raises(AwsmHipError) as e:
            dev.shadow_pass_views(views, **dict(good, **kw))
        assert e.value.code == code, (kw, e.value.code)
        return str(e.value)

    for read in (dev.read_shadow_view, lambda: dev.read_shadow_map(S, view=0)):                  # no frame with the pass yet
        with pytest.raises(AwsmHipError) as e:
            read()
        assert e.value.code == -5                                                                # AWSM_ERR_NOT_READY
    refused(-5)                                                                                  # after the frame's opaque pass
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    dev.geometry_pass(draws)
    dev.shadow_pass_views(good_views, **good)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(map_size=0), dict(map_size=8193), dict(pcf_radius=3), dict(strength=1.5), dict(strength=-0.1), dict(facing_fade=0.0), dict(max_slope=-0.01),
                dict(light=(0.0, 1.0, 0.0, 0.5)), dict(light=(nan, 1.0, 0.0, 0.0)), dict(bias=nan), dict(slope_bias=inf), dict(struct_size=2), dict(struct_size=5000)):
        refused(-1, **bad)                                                                       # AWSM_ERR_INVALID_ARGUMENT
    refused(-1, views=[])                                                                        # no views: a null pointer and a count of 0
    refused(-1, n_views=0)
    refused(-1, views=[(blocks[0], draws)] * 7)
    refused(-1, n_views=7)
    assert "view 1" in refused(-1, views=[(blocks[0], draws), (blocks[1][:508], draws)])
    assert "view 1" in refused(-1, views=[(blocks[0], draws), (blocks[1] + bytes(4), draws)])
    poisoned = np.frombuffer(blocks[0], np.float32).copy(); poisoned[35] = np.nan
    assert "view 0" in refused(-1, views=[(poisoned.tobytes(), draws), (blocks[1], draws)])
    broken = [dict(draws[0], tri_count=1 << 30)]
    assert "view 1" in refused(-7, views=[(blocks[0], draws), (blocks[1], broken)])              # AWSM_ERR_OUT_OF_RANGE, as shadow_pass answers it
    dev.opaque_pass()
    refused(-5)                                                                                  # the window has closed
    dev.frame_end()
    _assert_layers(dev, bytes(model.camera_bytes), blocks, S, vec)                               # the refused calls changed nothing
    dev.geometry_pass(draws)
    dev.shadow_pass_views(good_views, **good)
    with pytest.raises(AwsmHipError) as e:                                                       # the pass, but no opaque pass behind it yet
        dev.read_shadow_view()
    assert e.value.code == -5
    assert dev.read_shadow_map(view=1).shape == (S, S)
    dev.opaque_pass(has_opaque=False)
    with pytest.raises(AwsmHipError) as e:                                                       # an opaque pass with nothing to shade resolves nothing
        dev.read_shadow_view()
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
            dev.shadow_pass_views(good_views, **good)
        assert e.value.code == -6, shard                                                         # AWSM_ERR_UNSUPPORTED
        dev.opaque_pass(); dev.frame_end()
        dev.close()


# ------------------------------------------------------------------------------------------------ i. through the host

def test_point_light_and_cascades_through_the_host_layer(oracle_lut):
    """Renderer.set_shadow on a point light, and on the sun with cascades=3: every layer is the oracle's raster of the casters Host.shadow_views()
    reports from the block it reports, and layers, view and image are those of the manual calls with those blocks."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H, S = 70, 45, 96
    sc = sr.boxes(W, H)      # (the `perspective` camera sees the boxes and what they shadow under both lights)
    sun = {"kind": "directional", "color": (1.0, 0.97, 0.92), "intensity": 1.4, "direction": tuple(float(-c) for c in shr._SUN)}
    lamp = {"kind": "point", "color": (1.0, 1.0, 1.0), "intensity": 6.0, "position": svr.POINT_POSITIONS[1], "range": 0.0}
    sc.lights = [sun, lamp]
    model = helpers.build_model(sc)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.render(sync=True)
    off16 = dev.read_opaque()
    manual, _ = helpers.hip_frame(model, oracle_lut)
    for index, kw, n_views in ((1, {}, None), (0, {"cascades": 3, "cascade_distance": 6.0}, 3)):
        r.set_shadow(index, map_size=S, pcf_radius=1, strength=0.9, **kw)
        r.render(sync=True)
        views = r.host.shadow_views()
        assert len(views) == (n_views or len(views)) and len(views) >= 3
        blocks = [b for b, _ in views]
        for i, (block, casters) in enumerate(views):
            assert (dev.read_shadow_map(S, view=i) == shr.caster_map(model, block, S, casters)).all(), (index, i)
        light = svr.point_light(lamp["position"]) if index == 1 else tuple(float(np.float32(c)) for c in shr.host_light_camera(sun, shr.scene_aabbs(sc))["light"])
        params = {"pcf_radius": 1, "strength": 0.9}
        cam_block = dev.buffer_read(BUF_CAMERA, 0, 512)
        want = _assert_layers(dev, cam_block, blocks, S, light, params, what="host %d" % index)
        # (measured on the CPU oracle's keys: the lamp leaves 901 pixels dark; this camera looks along the sun's shadows and sees 117 pixels of
        # their edges, in three cascades of 658, 2481 and 11 pixels)
        assert (want["V"] < 1.0).sum() >= 50 and (want["V"] == 1.0).sum() >= 500 and (index == 0 or (want["V"] == 0.0).sum() >= 50)
        assert index == 1 or (np.bincount(want["view"][want["hit"]], minlength=3)[:3] >= 5).all()
        _assert_image(dev.read_opaque(), off16, want, what="host %d" % index)
        # the manual calls with the host's blocks and casters
        manual.buffer_write(BUF_CAMERA, 0, np.frombuffer(bytes(cam_block), np.uint8))
        manual.geometry_pass(model.collect_draws())
        manual.shadow_pass_views(views, map_size=S, light=light, **params)
        manual.opaque_pass(); manual.frame_end()
        for a, b in zip(manual.read_shadow(), dev.read_shadow()):
            assert (_bits(a) == _bits(b)).all()
        assert (manual.read_shadow_view() == dev.read_shadow_view()).all() and (manual.read_opaque() == dev.read_opaque()).all()
    r.set_shadow(False)
    r.render(sync=True)
    assert (dev.read_opaque() == off16).all()
    manual.close()
    r.close()
