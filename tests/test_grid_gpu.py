"""GPU tests of the editor's ground grid: the raw layer bit for bit against tests/grid_reference.py, the grid under an empty and
under a full transparent pass, on shards, under MSAA x4, in overlap mode, through the host layer, and the parameter record's checks."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc, PrimitiveDesc
from oracle import oracle_lib
from tests import grid_reference as gr
from tests import helpers

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_camera(sc, name):
    """The scene's camera <- one of the issue's (f32 matrices, as the scenes build theirs)."""
    c = gr.CAMERAS[name]
    aspect = sc.width / sc.height
    sc.view = scenes.look_at_rh(c["eye"], c["target"])
    sc.proj = (scenes.orthographic_rh(-6.0 * aspect, 6.0 * aspect, -6.0, 6.0, 0.1, 100.0) if "ortho_half_height" in c
               else scenes.perspective_rh(np.radians(50.0), aspect, 0.1, 100.0))
    sc.camera_position = c["eye"]
    return sc


def _frame(dev, model, transparent, post=None):
    """One more frame on a device helpers.hip_frame set up: the model's camera as it is now, the world transparent pass over `transparent`."""
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    dev.transparent_pass(transparent)
    if post:
        dev.post_pass(**post)
    dev.frame_end()


def _assert_layer(dev, block, W, H, params=None):
    want = gr.fragment(block, W, H, np.float32, params)
    rgba, depth, kept = dev.read_editor_grid()
    assert (kept == want["kept"]).all(), int((kept != want["kept"]).sum())
    assert (_bits(rgba) == _bits(want["rgba"])).all(), int((_bits(rgba) != _bits(want["rgba"])).any(axis=-1).sum())
    assert (_bits(depth) == _bits(want["depth"])).all(), int((_bits(depth) != _bits(want["depth"])).sum())
    return want


# ------------------------------------------------------------------------------------------------ the raw layer

@pytest.mark.parametrize("W,H", gr.SIZES)
def test_raw_layer_is_the_f32_restatement_bit_for_bit(W, H, oracle_lut):
    """Kept mask, RGBA and depth of every pixel, every camera.  67x45: the quad partners of the last column and the last row lie outside the image."""
    model = helpers.build_model(scenes.box_scene(W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    for name in gr.CAMERAS:
        block = gr.camera(name, W, H)
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
        want = _assert_layer(dev, block, W, H)
        assert want["kept"].any() == (name != "up"), name
    dev.close()


# ------------------------------------------------------------------------------------------------ an empty transparent pass

def _plane_scene(W, H):
    """A unit box centred at (0, 0.25, 0) — a quarter of it under the plane — and a quad IN the plane y = 0 over x, z in [1, 3]; camera `down`."""
    sc = scenes.box_scene(W, H)
    sc.nodes[0] = dataclasses.replace(sc.nodes[0], translation=(0.0, 0.25, 0.0))
    pos = np.array([(1, 0, 1), (1, 0, 3), (3, 0, 3), (3, 0, 1)], dtype=F)
    quad = PrimitiveDesc(positions=pos, normals=np.tile(np.array([(0, 1, 0)], dtype=F), (4, 1)), indices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint32), material=1)
    sc.nodes.append(NodeDesc(primitives=[quad]))
    sc.materials.append(MaterialDesc(base_color_factor=(0.1, 0.7, 0.2, 1.0), metallic_factor=0.0))
    return _set_camera(sc, "down")


@pytest.mark.parametrize("msaa", [0, 4])
def test_grid_over_an_empty_transparent_pass(msaa, oracle_lut):
    """transparent_pass([]) with the grid on: the composite is blend(device opaque image, layer, device depth) computed in numpy, bit for bit; the opaque
    image and the keys do not move."""
    W, H = 64, 48
    model = helpers.build_model(_plane_scene(W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    _frame(dev, model, [])
    opaque, vis = dev.read_opaque(), dev.read_visibility()
    assert (dev.read_composite() == opaque).all()                                         # grid off: a copy, as ever
    dev.set_editor_grid()
    _frame(dev, model, [])
    layer = _assert_layer(dev, model.camera_bytes, W, H)
    got = dev.read_composite()
    assert (dev.read_opaque() == opaque).all() and (dev.read_visibility() == vis).all()
    depth_s = gr.world_depth(vis)
    want = gr.blend(opaque, layer, depth_s)
    assert (got == want).all(), int((got != want).any(axis=-1).sum())
    # what the scene was built to show
    passes = gr.grid_passes(layer, depth_s)
    hit = (vis != helpers.NO_HIT).reshape(H, W, -1)
    wx, _, wz = layer["world_pos"]
    on_quad = (wx > 1.05) & (wx < 2.95) & (wz > 1.05) & (wz < 2.95)                       # the plane point under the pixel lies on the quad
    assert passes.any(axis=-1).sum() >= 0.25 * W * H
    assert (layer["kept"] & hit.all(axis=-1) & ~passes.any(axis=-1) & ~on_quad).sum() >= 50          # hidden by the box
    # The coplanar quad hides the grid (depth_epsilon's purpose).  Single-sampled: on every pixel of it.  MSAA: the keys carry each SAMPLE's depth and the
    # grid's is the pixel centre's, so across a pixel of this tilted plane the quad's depth moves by more than the epsilon and the quad wins on the
    # samples nearer than the centre only — "hides" is counted per pixel with at least one such sample.
    assert (layer["kept"] & on_quad & hit.all(axis=-1) & ~passes.all(axis=-1)).sum() >= 50
    if not msaa:
        assert (on_quad & passes.any(axis=-1)).sum() == 0
    assert (hit.all(axis=-1) & passes.all(axis=-1) & ~on_quad).sum() >= 20                           # the box under the plane, seen through the grid
    if msaa:
        assert (passes.any(axis=-1) & ~passes.all(axis=-1)).sum() >= 10                              # a mixed per-sample outcome
    assert (got != opaque).any(axis=-1).sum() >= 0.25 * W * H
    dev.set_editor_grid(None)
    _frame(dev, model, [])
    assert (dev.read_composite() == opaque).all()                                         # NULL: the grid-off composite again
    dev.close()


# ------------------------------------------------------------------------------------------------ under transparent meshes

def _opaque_transmission(sc):
    """transparent_scene with its three transmission materials blended instead: nothing samples the opaque image behind it."""
    for i, m in enumerate(sc.materials):
        if m.transmission is not None:
            sc.materials[i] = dataclasses.replace(m, transmission=None, volume=None, alpha_mode="blend", base_color_factor=tuple(m.base_color_factor[:3]) + (0.5,))
    return sc


def _raise_camera(sc):
    eye = (0.4, 1.6, 6.0)                                                                  # above the plane: the grid fills the lower half of the frame
    sc.view, sc.camera_position = scenes.look_at_rh(eye, (0, 0, 0)), eye
    return sc


def _oracle_forward_over(orc, draws, source16):
    """OracleFrame.forward with another image as the pass's source (what the blit leaves): oracle_forward called here, nothing under oracle/ changed."""
    L = oracle_lib.lib()
    arr = (oracle_lib.AwsmDraw * max(1, len(draws)))()
    for i, d in enumerate(draws):
        arr[i] = oracle_lib.AwsmDraw(d["geom_meta_off"], d["vis_data_off"], d["tri_count"], d["flags"], d.get("inst_off", 0), d.get("inst_count", 0))
    n = len(draws)
    L.oracle_forward_total_vertices.restype = C.c_uint32
    nv = int(L.oracle_forward_total_vertices(arr, C.c_uint32(n)))
    clip, nt, wpos = np.zeros((max(1, nv), 4), F), np.zeros((max(1, nv), 8), F), np.zeros((max(1, nv), 4), F)
    c32, c16, touched = np.zeros((orc.height, orc.width, 4), F), np.zeros((orc.height, orc.width, 4), np.uint16), np.zeros((orc.height, orc.width), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    source16 = np.ascontiguousarray(source16, np.uint16)
    assert L.oracle_forward_transform(C.byref(orc.scene), arr, C.c_uint32(n), p(clip), p(nt), p(wpos)) == 0
    assert L.oracle_forward(C.byref(orc.scene), arr, C.c_uint32(n), p(clip), p(nt), p(wpos), p(orc.keys), p(source16), p(c32), p(c16), p(touched), C.c_int(8)) == 0
    return c32, c16, touched


@pytest.mark.parametrize("msaa", [0, 4])
def test_grid_under_transparent_meshes_matches_the_oracle(msaa, oracle_lut):
    """The oracle's forward pass over source = opaque (+) grid against the device's composite, at the suite's composite bar.  MSAA: a pixel whose
    samples disagree on the grid's depth test has no single source colour and is left out (counted, capped)."""
    W, H = 64, 48
    sc = _raise_camera(_opaque_transmission(scenes.transparent_scene(W, H, tex_size=16)))
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa)
    tr = model.collect_transparent_draws()
    assert len(tr) >= 10
    layer = gr.fragment(model.camera_bytes, W, H, np.float32)
    depth_s = gr.world_depth(orc.keys)
    passes = gr.grid_passes(layer, depth_s)
    agree = passes.all(axis=-1) | ~passes.any(axis=-1)
    n_grid = int(passes.any(axis=-1).sum())
    assert n_grid >= 0.25 * W * H and (~agree).sum() <= 0.10 * n_grid, (n_grid, int((~agree).sum()))
    over = gr.resolve(gr.blend_samples(orc.rgba16f, layer, depth_s)[:, :, :1])            # sample 0's outcome = every sample's, where they agree
    want32, want16, touched = _oracle_forward_over(orc, tr, np.where(agree[..., None], over, orc.rgba16f))
    dev, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    dev.set_editor_grid()
    _frame(dev, model, tr)
    _assert_layer(dev, model.camera_bytes, W, H)
    got16, got32 = dev.read_composite(), dev.read_composite_f32()
    dev.close()
    ulp = helpers.f16_ulp_distance(got16, want16)[agree]
    ref = want32.astype(np.float64)
    bound = 2e-3 * np.maximum(1.0, np.abs(ref))                                           # helpers.compare_composite's f32 bound
    c = {"touched_pixels": int(((touched != 0) | passes.any(axis=-1))[agree].sum()), "pixels_over_2ulp": int((ulp > 2).any(axis=-1).sum()),
         "pixels_over_bound": int((np.abs(got32.astype(np.float64) - ref) > bound).any(axis=-1)[agree].sum()),
         "alpha_mismatch": int((got16[..., 3] != want16[..., 3])[agree].sum()), "max_ulp": int(ulp.max())}
    assert ((touched != 0) & passes.any(axis=-1)).sum() >= 100                             # transparent fragments over the grid
    helpers.assert_composite("grid under the transparent scene msaa=%d (left out: %d of %d grid pixels)" % (msaa, int((~agree).sum()), n_grid), c)


def test_pixels_without_the_grid_keep_their_bits_and_transmission_does_not_see_it(oracle_lut):
    """The unmodified transparent_scene (refraction taps of the opaque image anywhere on the screen): where the grid's fragment is discarded or fails the
    depth test on every sample the composite has the grid-off bits — the opaque image is not the grid's target.  Camera `up`: every pixel."""
    W, H = 64, 48
    sc = _raise_camera(scenes.transparent_scene(W, H, tex_size=16))
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut)
    tr = model.collect_transparent_draws()
    _frame(dev, model, tr)
    off, vis = dev.read_composite(), dev.read_visibility()
    dev.set_editor_grid()
    _frame(dev, model, tr)
    on = dev.read_composite()
    layer = _assert_layer(dev, model.camera_bytes, W, H)
    passes = gr.grid_passes(layer, gr.world_depth(vis)).any(axis=-1)
    assert passes.sum() >= 0.25 * W * H and (~passes).sum() >= 0.25 * W * H
    assert (on[~passes] == off[~passes]).all(), int((on != off).any(axis=-1)[~passes].sum())
    assert (on != off).any(axis=-1)[passes].mean() > 0.5                                 # the grid is on (under a fragment of alpha 1 it leaves no trace)
    _set_camera(sc, "up")
    model.update_camera()
    tr_up = model.collect_transparent_draws()
    _frame(dev, model, tr_up)
    on_up = dev.read_composite()
    assert not dev.read_editor_grid()[2].any()
    dev.set_editor_grid(None)
    _frame(dev, model, tr_up)
    assert (dev.read_composite() == on_up).all()
    dev.close()


# ------------------------------------------------------------------------------------------------ shards

@pytest.mark.parametrize("mode,msaa", [("rows", 0), ("rows", 4), ("bands", 0), ("bands", 4)])
def test_grid_on_sharded_contexts(mode, msaa, oracle_lut):
    """Two contexts, each with its rows of a 67x45 frame (strips split a quad row: 23 | 22; bands: rows 0-31 | 32-44), the opaque rows gathered and bound
    as the sharded transparent tests do: the assembled composite is the unsharded one bit for bit — absolute pixel coordinates, partners across the seam."""
    import torch
    from awsm_renderer_amd import sharding
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H, n = 67, 45, 2
    sc = _raise_camera(scenes.transparent_scene(W, H, tex_size=16))
    model = helpers.build_model(sc)
    world, tr = model.collect_draws(), model.collect_transparent_draws()
    ref, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    ref.set_editor_grid()
    _frame(ref, model, tr)
    want, want_opaque = ref.read_composite(), ref.read_opaque()
    ref.set_editor_grid(None)
    _frame(ref, model, tr)
    assert ((want != ref.read_composite()).any(axis=-1)).sum() >= 0.25 * W * H
    ref.close()
    per = (H + n - 1) // n
    rows_of = [np.array(sharding.band_rows(H, n, r)) if mode == "bands" else np.arange(min(r * per, H), min(r * per + per, H)) for r in range(n)]
    devs, opaque, comp, halos = [], [], [], []
    gathered = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r in range(n):
        dev = HipDevice(parity_tap=False)
        opaque.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        comp.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        dev.resize(W, H, msaa)
        dev.upload_mirrors(model.mirrors())
        for i, t in enumerate(model.texture_arrays()):
            dev.texture_array_upload(i, t["texels"])
        for i, smp in enumerate(sc.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        if mode == "bands":
            dev.set_shard_bands(n, r)
        else:
            dev.set_shard_rows(int(rows_of[r][0]), int(rows_of[r][-1]) + 1)
        dev.bind_output(opaque[r].data_ptr(), H * W * 8)
        dev.bind_composite(comp[r].data_ptr(), H * W * 8)
        dev.set_editor_grid()
        dev.geometry_pass(world)
        if mode == "bands" and msaa:                                                      # the bands' boundary keys, exchanged between the two passes
            L = dev.msaa_halo_bands()
            buf = torch.zeros((L, 2, W), dtype=torch.int64, device="cuda")
            dev.msaa_halo_export(buf.data_ptr(), L * 2 * W * 8)
            halos.append(buf)
        devs.append(dev)
    halo = torch.stack(halos).contiguous() if halos else None
    for r, dev in enumerate(devs):
        if halo is not None:
            dev.frame_end()
            dev.msaa_halo_bind(halo.data_ptr(), halo.numel() * 8)
        dev.opaque_pass(); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        gathered[idx] = opaque[r][idx]
    torch.cuda.synchronize()
    assert (gathered.cpu().numpy().view(np.uint16) == want_opaque).all()
    final = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r, dev in enumerate(devs):
        dev.bind_opaque_source(gathered.data_ptr(), H * W * 8)
        dev.transparent_pass(tr); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        final[idx] = comp[r][idx]
        dev.close()
    torch.cuda.synchronize()
    got = final.cpu().numpy().view(np.uint16)
    assert (got == want).all(), int((got != want).any(axis=2).sum())


# ------------------------------------------------------------------------------------------------ overlap mode

def test_grid_uses_the_frames_camera_snapshot_in_overlap_mode(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES: frame A with camera `down`, the camera written again, frame B with `horizon`, both enqueue-only, each into its own
    image: each composite is its synchronous twin's."""
    import torch
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H = 64, 48
    model = helpers.build_model(_plane_scene(W, H))
    blocks = {name: gr.camera(name, W, H) for name in ("down", "horizon")}
    want = {}
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dev.set_editor_grid()
    for name, block in blocks.items():
        model.camera_bytes = block
        _frame(dev, model, [])
        want[name] = dev.read_composite()
    dev.close()
    assert (want["down"] != want["horizon"]).any(axis=-1).sum() >= 0.25 * W * H
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    dev.set_editor_grid()
    images = {name: torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for name in blocks}
    draws = model.collect_draws()
    for name, block in blocks.items():                                                    # no frame_end between the two frames
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.bind_composite(images[name].data_ptr(), H * W * 8)
        dev.geometry_pass(draws); dev.opaque_pass(); dev.transparent_pass([])
    dev.frame_end()
    torch.cuda.synchronize()
    for name in blocks:
        got = images[name].cpu().numpy().view(np.uint16)
        assert (got == want[name]).all(), (name, int((got != want[name]).any(axis=-1).sum()))
    dev.close()


# ------------------------------------------------------------------------------------------------ through the host

def test_grid_through_the_host_layer(oracle_lut):
    """Host.set_editor_grid on a scene without transparent meshes: render() runs the transparent pass with no draws and yields the empty-pass
    composite; with post-processing on the display image moves on the grid's pixels only."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H = 64, 48
    sc = _plane_scene(W, H)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.set_post_processing(1)
    r.render(sync=True)
    display_off, opaque = dev.read_display(), dev.read_opaque()
    r.set_editor_grid(True)
    stats = r.render(sync=True)
    assert stats["forward_triangles"] == 0
    vis = dev.read_visibility()
    block = dev.buffer_read(BUF_CAMERA, 0, 512)
    layer = _assert_layer(dev, block, W, H)
    want = gr.blend(opaque, layer, gr.world_depth(vis))
    got = dev.read_composite()
    assert (dev.read_opaque() == opaque).all() and (got == want).all(), int((got != want).any(axis=-1).sum())
    passes = gr.grid_passes(layer, gr.world_depth(vis)).any(axis=-1)
    moved = (dev.read_display() != display_off).any(axis=-1)
    assert passes.sum() >= 0.25 * W * H and not moved[~passes].any() and moved[passes].mean() > 0.9
    r.set_editor_grid(True, color_background=(0.0, 0.5, 0.0), alpha_background=1.0)
    r.render(sync=True)
    want = gr.blend(opaque, gr.fragment(block, W, H, np.float32, {"color_background": (0.0, 0.5, 0.0), "alpha_background": 1.0}), gr.world_depth(vis))
    assert (dev.read_composite() == want).all()
    r.set_editor_grid(False)
    r.render(sync=True)
    assert (dev.read_display() == display_off).all()
    r.close()


# ------------------------------------------------------------------------------------------------ the parameter record

def test_grid_parameters(oracle_lut):
    """Overrides reach the layer; a struct_size shorter by the last field leaves that field at its default; a NaN is refused and changes nothing; NULL
    restores the grid-off composite."""
    from awsm_renderer_amd.hip_backend import AwsmEditorGrid, AwsmHipError
    W, H = 64, 48
    model = helpers.build_model(_plane_scene(W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    _frame(dev, model, [])
    off = dev.read_composite()
    over = {"color_background": (0.5, 0.25, 0.125), "alpha_background": 0.5, "color_minor": (0.0, 1.0, 0.0), "alpha_minor": 0.75, "color_major": (1.0, 1.0, 0.0),
            "alpha_major": 0.875, "color_z_axis": (0.0, 0.0, 1.0), "alpha_axis": 0.625, "color_x_axis": (1.0, 0.0, 0.0), "depth_epsilon": 0.01}
    dev.set_editor_grid(**over)
    _frame(dev, model, [])
    layer = _assert_layer(dev, model.camera_bytes, W, H, over)
    assert (dev.read_composite() == gr.blend(dev.read_opaque(), layer, gr.world_depth(dev.read_visibility()))).all()
    dev.set_editor_grid(struct_size=C.sizeof(AwsmEditorGrid) - 4, **over)                # depth_epsilon is not read: the default holds
    _assert_layer(dev, model.camera_bytes, W, H, dict(over, depth_epsilon=gr.DEFAULTS["depth_epsilon"]))
    for bad in (dict(color_minor=(0.0, float("nan"), 0.0)), dict(depth_epsilon=float("inf")), dict(struct_size=2), dict(struct_size=5000)):
        with pytest.raises(AwsmHipError) as e:
            dev.set_editor_grid(**bad)
        assert e.value.code == -1                                                         # AWSM_ERR_INVALID_ARGUMENT
    _assert_layer(dev, model.camera_bytes, W, H, dict(over, depth_epsilon=gr.DEFAULTS["depth_epsilon"]))      # a refused record changes nothing
    dev.set_editor_grid(struct_size=4, **over)                                           # only struct_size is known: all defaults
    _assert_layer(dev, model.camera_bytes, W, H)
    dev.set_editor_grid(None)
    _frame(dev, model, [])
    assert (dev.read_composite() == off).all()
    dev.close()
