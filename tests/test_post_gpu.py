"""GPU tests of the effects + display passes (awsm_hip_post_pass): the device's effects and display images against tests/post_oracle.py,
which takes the device's own composite and depth as its input.  Bars: DESIGN.md §11 (effects <= 1 f16 ulp, <= 2 after the bloom chain,
ill-conditioned DoF and SMAA pixels counted apart; display <= 1 LSB and fewer than 0.1 % of the channels off)."""
import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
from tests import helpers, post_oracle

pytestmark = pytest.mark.gpu

BUF_CAMERA = 5
FOCUS, APERTURE = 3.0, 0.7      # a short focus and a wide aperture: CoC from 0 to the 16-pixel cap across the helmet's frame


def _frame(scene, lut, msaa=0, dof=(FOCUS, APERTURE), transparent=False, dev=None):
    """hip_frame with the camera's DoF bytes (496-503) written before the geometry pass takes its snapshot."""
    model = helpers.build_model(scene)
    dev = dev or HipDevice(parity_tap=True)
    dev.resize(scene.width, scene.height, msaa)
    dev.upload_mirrors(model.mirrors())
    if isinstance(dof, tuple):
        dev.buffer_write(BUF_CAMERA, 496, np.array(dof, dtype=np.float32))
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(scene.samplers):
        dev.sampler_set(i, s)
    from oracle import oracle_lib
    dev.env_upload(scene.skybox_rgba, scene.prefiltered_rgb, scene.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    if transparent:
        dev.transparent_pass(model.collect_transparent_draws())
    dev.frame_end()
    cam = np.frombuffer(bytes(model.mirrors()[BUF_CAMERA])[:512], dtype=np.float32).copy()
    if dof is not None:
        cam[124:126] = dof
    return dev, model, cam


def _depth(dev, scene, msaa):
    keys = np.zeros(scene.width * scene.height * (4 if msaa else 1), dtype=np.uint64)
    dev._chk(dev.lib.awsm_hip_read_visibility(dev.ctx, keys.ctypes.data), "read_visibility")
    d = np.where(keys == np.uint64(0xFFFFFFFFFFFFFFFF), np.uint32(0x3F800000), (keys >> np.uint64(32)).astype(np.uint32)).view(np.float32)
    d = d.reshape(scene.height, scene.width, 4 if msaa else 1)
    return np.minimum(np.float32(1.0), d.min(axis=2)) if msaa else d[..., 0]


def _source(dev, transparent):
    return dev.read_composite() if transparent else dev.read_opaque()


def _check(name, dev, cam, depth, src, tonemap=1, smaa=False, bloom=False, dof=False):
    dev.post_pass(tonemap, smaa=smaa, bloom=bloom, dof=dof)
    eff, disp = dev.read_effects(), dev.read_display()
    want_eff, ill = post_oracle.effects(src, depth, cam, smaa_on=smaa, bloom=bloom, dof=dof)
    want_disp = post_oracle.display(want_eff, tonemap)
    ulp = helpers.f16_ulp_distance(eff, want_eff).max(axis=2)
    bar = 2 if bloom else 1
    over = (ulp > bar) & ~ill
    ddiff = np.abs(disp.astype(np.int16) - post_oracle.display(eff, tonemap).astype(np.int16))     # the display pass alone, on the device's effects
    odiff = np.abs(disp.astype(np.int16) - want_disp.astype(np.int16))
    res = {"case": name, "max_ulp_well": int(ulp[~ill].max()) if (~ill).any() else 0, "over_bar": int(over.sum()), "ill_px": int(ill.sum()),
           "ill_off": int(((ulp > bar) & ill).sum()), "display_max_lsb": int(ddiff.max()), "display_frac_off": float((ddiff > 0).mean()),
           "display_vs_oracle_frac_off": float((odiff[~ill] > 0).mean()) if (~ill).any() else 0.0}
    print("post bars:", res)
    assert res["over_bar"] == 0 and res["ill_off"] == 0, res
    assert res["display_max_lsb"] <= 1 and res["display_frac_off"] < 1e-3, res
    assert (eff[..., 3] == 0x3C00).all() and (disp[..., 3] == 255).all()
    return res, disp


def test_display_only_three_tone_maps_atrium_4k(oracle_lut):
    sc = scenes.atrium_scene(3840, 2160, detail=0.25, tex_scale=1 / 16)
    dev, model, cam = _frame(sc, oracle_lut, dof=None)
    src = _source(dev, False)
    for op in (0, 1, 2):
        res, disp = _check(f"atrium4k display tonemap={op}", dev, cam, None, src, tonemap=op)
        want = post_oracle.display(post_oracle.effects(src)[0], op)
        assert np.abs(disp.astype(np.int16) - want.astype(np.int16)).max() <= 1
    dev.close()


@pytest.mark.parametrize("msaa", [0, 4])
@pytest.mark.parametrize("which", ["helmet1080", "atrium4k"])
def test_each_effect_and_all_together(oracle_lut, which, msaa):
    sc = scenes.helmet_scene(1920, 1080, tex_size=256) if which == "helmet1080" else scenes.atrium_scene(3840, 2160, detail=0.25, tex_scale=1 / 16)
    dev, model, cam = _frame(sc, oracle_lut, msaa=msaa)
    src, depth = _source(dev, False), _depth(dev, sc, msaa)
    _, coc = post_oracle.dof_terms(depth, cam)
    # linearize_depth takes near = proj[3][2], negative for a [0, 1] right-handed projection: the linear depth is positive only where nothing
    # was hit (depth 1.0), so the reference's DoF blurs the background and nothing else.  The enclosed atrium shows no background (CoC 0
    # everywhere: its DoF case checks the pass-through); the helmet's frame does.
    if which == "atrium4k":
        assert (coc == 0).all()
    else:
        assert (coc >= 0.5).any() and (coc < 0.5).any(), ("the DoF settings must blur part of the frame and leave part sharp", float(coc.min()), float(coc.max()), cam[124:126])
    cases = [dict(smaa=True), dict(bloom=True), dict(dof=True), dict(smaa=True, bloom=True, dof=True)]
    if which == "helmet1080":
        cases.append(dict(smaa=True, dof=True))
    for kw in cases:
        _check(f"{which} msaa={msaa} {kw}", dev, cam, depth, src, **kw)
    dev.close()


def _transparent_variant(alpha_mode):
    """transparent_scene with every non-opaque material set to `alpha_mode`.  "blend" also turns the alpha-mask material into a blended one,
    so no fragment is discarded and coverage is the same as with "opaque"."""
    import dataclasses
    sc = scenes.transparent_scene(640, 360)
    sc.materials = [m if m.alpha_mode == "opaque" else dataclasses.replace(m, alpha_mode=alpha_mode) for m in sc.materials]
    return sc


@pytest.mark.parametrize("msaa", [0, 4])
def test_dof_reads_depth_after_the_transparent_pass(oracle_lut, msaa):
    """The transparent pipeline writes depth (material_transparent/pipeline.rs:180), and the transparent pass's coverage and depth follow the
    geometry pass's contract: the depth DoF sees is the geometry pass's depth of the same scene with the transparent materials made opaque."""
    sc = _transparent_variant("blend")
    dev, model, cam = _frame(sc, oracle_lut, msaa=msaa, transparent=True)
    assert model.collect_transparent_draws()
    world = _depth(dev, sc, msaa)
    src = dev.read_composite()
    sc_o = _transparent_variant("opaque")
    dev_o, _, cam_o = _frame(sc_o, oracle_lut, msaa=msaa)
    want_depth = _depth(dev_o, sc_o, msaa)
    dev_o.close()
    assert np.array_equal(cam, cam_o) and (want_depth < world).any()
    res, _ = _check(f"transparent msaa={msaa} dof", dev, cam, want_depth, src, dof=True)
    res, _ = _check(f"transparent msaa={msaa} all", dev, cam, want_depth, src, smaa=True, bloom=True, dof=True)
    # not vacuous: with the world depth alone the expected image differs
    with_world, _ = post_oracle.effects(src, world, cam, dof=True)
    with_all, _ = post_oracle.effects(src, want_depth, cam, dof=True)
    assert (with_world != with_all).any()
    dev.close()


def test_post_pass_is_replayed_with_an_overflowing_frame(oracle_lut):
    """A post pass enqueued before awsm_hip_frame_end is enqueued again when frame_end grows an overflowed list and replays the frame."""
    sc = _transparent_variant("blend")
    model = helpers.build_model(sc)
    outs = []
    for before in (True, False):
        dev = HipDevice(parity_tap=True, small_bin_list=True)
        dev, _, cam = _frame(sc, oracle_lut, dev=dev, transparent=True) if not before else (dev, None, None)
        if before:       # the passes, the post pass, then frame_end (which replays the overflowed frame)
            dev.resize(sc.width, sc.height, 0)
            dev.upload_mirrors(model.mirrors())
            dev.buffer_write(BUF_CAMERA, 496, np.array((FOCUS, APERTURE), dtype=np.float32))
            for i, t in enumerate(model.texture_arrays()):
                dev.texture_array_upload(i, t["texels"])
            for i, s in enumerate(sc.samplers):
                dev.sampler_set(i, s)
            from oracle import oracle_lib
            dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
            dev.geometry_pass(model.collect_draws())
            dev.opaque_pass()
            dev.transparent_pass(model.collect_transparent_draws())
            dev.post_pass(1, smaa=True, bloom=True, dof=True)
            stats = dev.frame_end()
            assert stats["bin_overflow_retries"] > 0, "the frame must overflow for this test to mean anything"
        else:
            dev.post_pass(1, smaa=True, bloom=True, dof=True)
        outs.append((dev.read_display(), dev.read_effects(), dev.read_composite()))
        dev.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_post_pass_leaves_keys_opaque_and_composite_alone(oracle_lut):
    sc = scenes.transparent_scene(640, 360)
    outs = []
    for post in (False, True):
        dev, model, cam = _frame(sc, oracle_lut, transparent=True)
        if post:
            dev.post_pass(2, smaa=True, bloom=True, dof=True)
            dev.frame_end()
        keys = np.zeros(sc.width * sc.height, dtype=np.uint64)
        dev._chk(dev.lib.awsm_hip_read_visibility(dev.ctx, keys.ctypes.data), "read_visibility")
        outs.append((keys, dev.read_opaque(), dev.read_composite()))
        dev.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_error_codes(oracle_lut):
    sc = scenes.helmet_scene(320, 180, segments=24, rings=16, tex_size=32)
    dev = HipDevice(parity_tap=True)
    dev.resize(sc.width, sc.height, 0)
    with pytest.raises(AwsmHipError) as e:
        dev.post_pass(1)
    assert e.value.code == -5          # AWSM_ERR_NOT_READY: no opaque pass yet
    dev, model, cam = _frame(sc, oracle_lut, dev=dev)
    with pytest.raises(AwsmHipError) as e:
        dev.post_pass(1, struct_size=8)
    assert e.value.code == -1
    with pytest.raises(AwsmHipError) as e:
        dev.post_pass(3)
    assert e.value.code == -1
    dev.post_pass(1)
    dev.close()
    dev2 = HipDevice(parity_tap=True)
    dev2.resize(sc.width, sc.height, 0)
    dev2.set_shard_rows(0, 90)
    with pytest.raises(AwsmHipError) as e:
        dev2.post_pass(1)
    assert e.value.code == -6          # AWSM_ERR_UNSUPPORTED on a sharded context
    dev2.close()


def test_overlapped_frames_match_synchronous(oracle_lut):
    sc = scenes.helmet_scene(640, 360, segments=48, rings=36, tex_size=64)
    model = helpers.build_model(sc)
    from oracle import oracle_lib

    def run(overlap):
        import torch
        dev = HipDevice(overlap_frames=overlap)
        dev.resize(sc.width, sc.height, 0)
        dev.upload_mirrors(model.mirrors())
        for i, t in enumerate(model.texture_arrays()):
            dev.texture_array_upload(i, t["texels"])
        for i, s in enumerate(sc.samplers):
            dev.sampler_set(i, s)
        dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        cam0 = np.frombuffer(bytes(model.mirrors()[BUF_CAMERA])[:512], dtype=np.float32)
        outs = [torch.zeros(sc.height * sc.width * 4, dtype=torch.uint8, device="cuda") for _ in range(10)]
        for k in range(10):
            cam = cam0.copy()
            cam[32 + 12] += np.float32(0.01 * k)      # view_proj translation: the camera moves every frame
            cam[124:126] = (FOCUS, APERTURE)
            dev.buffer_write(BUF_CAMERA, 0, cam)
            dev.geometry_pass(model.collect_draws())
            dev.opaque_pass()
            dev.bind_display(outs[k].data_ptr(), outs[k].numel())
            dev.post_pass(1, smaa=k % 2 == 0, bloom=k % 3 == 0, dof=True)
            assert dev.display_device_ptr() == outs[k].data_ptr()
            if overlap:
                dev.frame_flush()
            else:
                dev.frame_end()
        dev.frame_end()
        torch.cuda.synchronize()
        frames = [o.cpu().numpy() for o in outs]
        dev.close()
        return frames

    sync, over = run(False), run(True)
    assert not np.array_equal(sync[0], sync[1])
    for k in range(10):
        assert np.array_equal(sync[k], over[k]), k


def test_host_render_with_post_processing_matches_the_c_abi_sequence(oracle_lut):
    from awsm_renderer_amd.host import Renderer
    from oracle import oracle_lib
    sc = scenes.helmet_scene(640, 360, segments=48, rings=36, tex_size=64)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    r.camera_set_dof(FOCUS, APERTURE)
    r.set_post_processing(2, bloom=True, dof=True, smaa=True)
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    got, src = dev.read_display(), dev.read_opaque()
    dev.post_pass(2, smaa=True, bloom=True, dof=True)       # the same sequence by hand, on the same frame
    assert np.array_equal(got, dev.read_display())
    cam = np.frombuffer(r.host.mirror(BUF_CAMERA)[:512], dtype=np.float32)
    assert cam[124] == np.float32(FOCUS) and cam[125] == np.float32(APERTURE)
    want, ill = post_oracle.effects(src, _depth(dev, sc, 0), cam, smaa_on=True, bloom=True, dof=True)
    assert (helpers.f16_ulp_distance(dev.read_effects(), want).max(axis=2)[~ill] <= 2).all()
    dev.close()
    r.close()


def test_host_post_processing_and_sharding_refuse_each_other(oracle_lut):
    from awsm_renderer_amd.host import HostError, Renderer
    from oracle import oracle_lib
    sc = scenes.helmet_scene(320, 180, segments=24, rings=16, tex_size=32)
    r = Renderer(sc, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    r.set_post_processing(1)
    with pytest.raises(HostError, match=r"\(-6\)"):
        r.host.set_shard_rows(0, 90)
    r.clear_post_processing()
    r.host.set_shard_rows(0, 90)
    with pytest.raises(HostError, match=r"\(-6\)"):
        r.set_post_processing(1)
    r.render(sync=True)                  # the sharded frame renders without a post pass
    r.host.set_shard_rows(0, 0)
    r.set_post_processing(1, smaa=True)
    r.render(sync=True)
    r.close()
