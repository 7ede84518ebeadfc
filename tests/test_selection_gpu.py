"""GPU tests of the editor's selection overlay: the layers and the blended composite bit for bit against tests/selection_reference.py fed
the device's own keys, under MSAA x4, over transparent meshes and the grid, under HUD meshes, in overlap mode, through a replayed frame, in front of
the post pass, through the host layer, and the refusals.  Frames of 8 x 5, 33 x 17 and 70 x 45 only."""
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc
from oracle import oracle_lib
from oracle.host_mirror import key_as_ffi
from tests import helpers
from tests import selection_reference as sel
from tests import ssao_reference as sr

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
F = np.float32
# colours and alphas that are no round numbers: every product of the blend rounds
LOOK = dict(outline_color=(0.9, 0.55, 0.15, 0.6), box_color=(0.2, 0.7, 0.95, 0.85), hidden_alpha=0.3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _point(model, cam):
    sc = model.scene
    sr.set_camera(sc, sr.camera(cam, sc.width, sc.height))
    model.update_camera()
    return bytes(model.camera_bytes)


def _frame(dev, model, transparent=None, post=None, end=True, hud=False, hud_transparent=True):
    """One more frame on a device helpers.hip_frame set up, with the model's camera as it is now and the world transparent pass (over the model's
    transparent draws unless `transparent` lists others) -> the world draw list the geometry pass was given."""
    dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(model.camera_bytes, np.uint8))
    draws = model.collect_draws()
    dev.geometry_pass(draws)
    if hud:
        dev.hud_geometry_pass(model.hud_geometry_draws)
    dev.opaque_pass()
    dev.transparent_pass(model.collect_transparent_draws() if transparent is None else transparent)
    if hud and hud_transparent:
        dev.hud_transparent_pass(model.hud_transparent_draws)
    if post:
        dev.post_pass(**post)
    if end:
        dev.frame_end()
    return draws


def _want(dev, model, draws, kw, boxes, block, rec):
    """The restatement fed the device's own keys, the draw list the frame was given and the camera block the test wrote."""
    return sel.overlay(dev.read_visibility(), sel.draw_table(draws, model.mirrors()), kw, boxes, block, dev.width, dev.height, rec)


def _first_bad(bad):
    return tuple(int(v) for v in np.argwhere(bad)[0])


def _assert_layers(dev, want, what="", n_boxes=None):
    selected, ring, alpha, edges = dev.read_selection(n_boxes)
    for name, got, ref in (("selected", selected, want["selected"]), ("ring", ring, want["ring"])):
        bad = got != ref
        assert not bad.any(), "%s %s: %d of %d pixels differ, first at (y, x) = %s: device %r, restatement %r" % (
            what, name, int(bad.sum()), bad.size, _first_bad(bad), got[_first_bad(bad)], ref[_first_bad(bad)])
    bad = _bits(edges) != _bits(want["edges"])
    assert edges.shape == want["edges"].shape and not bad.any(), "%s edges: %d words differ, first at (box, edge, word) = %s: device %r, restatement %r" % (
        what, int(bad.sum()), _first_bad(bad), edges[_first_bad(bad)], want["edges"][_first_bad(bad)])
    bad = _bits(alpha) != _bits(want["box_alpha"])
    assert not bad.any(), "%s box_alpha: %d of %d pixels differ, first at (y, x) = %s: device %r (bits %#x), restatement %r (bits %#x)" % (
        what, int(bad.sum()), bad.size, _first_bad(bad), alpha[_first_bad(bad)], int(_bits(alpha)[_first_bad(bad)]),
        want["box_alpha"][_first_bad(bad)], int(_bits(want["box_alpha"])[_first_bad(bad)]))


def _assert_floor(want, floor, what=""):
    c = sel.counts(want)
    print(what, c, "floor", floor)
    for k, least in zip(sel.KINDS, floor):
        assert c[k] >= least, (what, k, c, floor)


def _assert_image(on16, off16, want, rec, on32=None, off32=None, what=""):
    """The composite against the restatement's blend of the composite of a context without a selection; untouched pixels keep its bits."""
    ref = sel.blend(off16, want["ring"], want["box_alpha"], rec)
    touched = want["ring"] | (want["box_alpha"] > 0)
    bad = (on16 != ref).any(axis=-1)
    at = _first_bad(bad) if bad.any() else None
    assert not bad.any(), "%s: %d pixels of the composite differ, first at (y, x) = %s: device %s, off %s, restatement %s, ring %r, A %r (bits %#x)" % (
        what, int(bad.sum()), at, on16[at], off16[at], ref[at], want["ring"][at], want["box_alpha"][at], int(_bits(want["box_alpha"])[at]))
    assert (on16[~touched] == off16[~touched]).all()
    if on32 is not None:
        ref32 = sel.blend_f32(off32, ref, touched)
        bad32 = (_bits(on32) != _bits(ref32)).any(axis=-1)
        assert not bad32.any(), "%s: %d pixels of the f32 composite differ, first at %s: device %s, restatement %s" % (
            what, int(bad32.sum()), _first_bad(bad32), on32[_first_bad(bad32)], ref32[_first_bad(bad32)])
    return touched


# ------------------------------------------------------------------------------------------------ layers, bit for bit

@pytest.mark.parametrize("scene", ["corner", "boxes"])
@pytest.mark.parametrize("W,H", sel.SIZES)
def test_layers_are_the_f32_restatement_bit_for_bit(W, H, scene, oracle_lut):
    """selected, ring, box alpha and the edge table under every camera, at R = 1 with half width 0.5 and R = 4 with 1.75, and no fewer ring and box
    pixels of each kind than the case's floor.  `closeup` stands inside the first box (edges cross the near plane); `ortho` has w = 1."""
    model = helpers.build_model(sel.SCENES[scene](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    for cam in sel.CAMERAS:
        block = _point(model, cam)
        kw, boxes = sel.selection_of(model, scene)
        for R, hw in sel.PARAMS:
            rec = sel.record(outline_radius=R, box_half_width=hw)
            dev.set_selection(kw, boxes, outline_radius=R, box_half_width=hw)
            draws = _frame(dev, model)
            what = "%s %s %dx%d R=%d hw=%g" % (scene, cam, W, H, R, hw)
            want = _want(dev, model, draws, kw, boxes, block, rec)
            _assert_layers(dev, want, what)
            _assert_floor(want, sel.FLOORS[(scene, cam, W, H, R, hw)], what)
    dev.close()


def test_sixty_four_boxes_fill_one_tiles_edge_list(oracle_lut):
    """64 copies of one small box: all 768 edges reach one tile, the LDS index list is full."""
    W, H = 70, 45
    model = helpers.build_model(sel.SCENES["boxes"](W, H, "far"))
    rec4 = list(model.meshes.items())[4]
    boxes = [list(rec4[1].world_aabb.min) + list(rec4[1].world_aabb.max)] * 64
    kw = sel.key_words([key_as_ffi(rec4[0])])
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dev.set_selection(kw, boxes)
    draws = _frame(dev, model)
    want = _want(dev, model, draws, kw, boxes, bytes(model.camera_bytes), sel.record())
    assert sel.tile_list_sizes(want["edges"], W, H, sel.record()).max() == 768
    _assert_layers(dev, want, "64 boxes")
    c = sel.counts(want)
    assert c["ring"] >= 5 and c["partial"] + c["full"] >= 10, c
    dev.close()


# ------------------------------------------------------------------------------------------------ image

@pytest.mark.parametrize("scene", ["corner", "boxes"])
def test_composite_is_the_blended_selection_off_composite(scene, oracle_lut):
    """RGBA16F and the f32 tap against the restatement's blend of the composite of a context that never had a selection; keys and the opaque image do
    not move; after set_selection(NULL) the next frame is the other context's, whole."""
    W, H = 70, 45
    model = helpers.build_model(sel.SCENES[scene](W, H))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    moved = 0
    for cam in sel.CAMERAS:
        block = _point(model, cam)
        kw, boxes = sel.selection_of(model, scene)
        rec = sel.record(**LOOK)
        on.set_selection(kw, boxes, **LOOK)
        draws = _frame(on, model); _frame(off, model)
        what = "%s %s" % (scene, cam)
        want = _want(on, model, draws, kw, boxes, block, rec)
        _assert_layers(on, want, what)
        on16, off16 = on.read_composite(), off.read_composite()
        touched = _assert_image(on16, off16, want, rec, on.read_composite_f32(), off.read_composite_f32(), what)
        assert (on.read_visibility() == off.read_visibility()).all() and (on.read_opaque() == off.read_opaque()).all()
        assert (off16 == off.read_opaque()).all()                                            # (no transparent mesh, no grid: the blit)
        moved += int((on16 != off16).any(axis=-1).sum())
        assert touched.sum() >= sum(sel.FLOORS[(scene, cam, W, H, 1, 0.5)][:2])
    assert moved >= 200
    on.set_selection(on=None)
    _frame(on, model); _frame(off, model)
    assert (on.read_composite() == off.read_composite()).all() and (_bits(on.read_composite_f32()) == _bits(off.read_composite_f32())).all()
    on.close(); off.close()


def test_flags_choose_the_layers(oracle_lut):
    W, H = 33, 17
    model = helpers.build_model(sel.SCENES["boxes"](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    _frame(dev, model)
    off16 = dev.read_composite()
    kw, boxes = sel.selection_of(model, "boxes")
    block = bytes(model.camera_bytes)
    for flags in (sel.OUTLINE, sel.BOXES):
        rec = sel.record(flags=flags)
        dev.set_selection(kw, boxes, flags=flags)
        draws = _frame(dev, model)
        want = _want(dev, model, draws, kw, boxes, block, rec)
        _assert_layers(dev, want, "flags %d" % flags)
        assert want["ring"].any() == (flags == sel.OUTLINE) and (want["box_alpha"] > 0).any() == (flags == sel.BOXES)
        _assert_image(dev.read_composite(), off16, want, rec, what="flags %d" % flags)
    dev.close()


# ------------------------------------------------------------------------------------------------ pass combinations

@pytest.mark.parametrize("W,H", sel.SIZES[1:])
def test_msaa_selected_from_any_sample_and_the_least_depth(W, H, oracle_lut):
    model = helpers.build_model(sel.SCENES["boxes"](W, H))
    on, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    off, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    for cam in ("perspective", "along", "far"):
        block = _point(model, cam)
        kw, boxes = sel.selection_of(model, "boxes")
        rec = sel.record(**LOOK)
        on.set_selection(kw, boxes, **LOOK)
        draws = _frame(on, model); _frame(off, model)
        keys = on.read_visibility()
        assert keys.shape == (H, W, 4)
        want = _want(on, model, draws, kw, boxes, block, rec)
        _assert_layers(on, want, "msaa %s %dx%d" % (cam, W, H))
        # pixels that are selected by some sample but not by sample 0, and pixels whose least depth is not sample 0's
        table = sel.draw_table(draws, model.mirrors())
        s0, d0 = sel.pixels(keys[..., 0], table, want["draw_selected"])
        print("msaa", cam, W, H, "selected by another sample only:", int((want["selected"] & ~s0).sum()), "least depth elsewhere:", int((want["depth"] != d0).sum()))
        assert cam == "far" or ((want["selected"] & ~s0).sum() >= 3 and (want["depth"] != d0).sum() >= 10)
        _assert_image(on.read_composite(), off.read_composite(), want, rec, on.read_composite_f32(), off.read_composite_f32(), "msaa %s" % cam)
        assert want["ring"].sum() >= 4 and (want["box_alpha"] > 0).sum() >= 8
    on.close(); off.close()


def _glass_boxes(W, H):
    """`boxes` with a blended quad standing in front of the first box."""
    sc = sr.boxes(W, H)
    sc.materials.append(MaterialDesc(base_color_factor=(0.2, 0.5, 0.9, 0.5), alpha_mode="blend", metallic_factor=0.0))
    quad = dataclasses.replace(sr._quad((0.3, 0.05, 1.9), (1.4, 0.0, -0.6), (0.0, 1.3, 0.0), 0), material=len(sc.materials) - 1)
    sc.nodes.append(NodeDesc(primitives=[quad]))
    return sc


def test_overlay_lies_over_the_transparent_meshes_and_the_grid(oracle_lut):
    """A blended quad in front of the selected box and the editor's grid, in both contexts: the composite is the restatement's blend of the other
    context's composite — the overlay is the last to draw — and the transparent quad itself is selected by its box alone."""
    W, H = 70, 45
    model = helpers.build_model(_glass_boxes(W, H))
    on, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    off, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    assert len(model.collect_transparent_draws()) == 1
    glass_key, glass = list(model.meshes.items())[6]
    kw, boxes = sel.selection_of(model, "boxes")
    kw = kw + sel.key_words([key_as_ffi(glass_key)])
    boxes = boxes + [list(glass.world_aabb.min) + list(glass.world_aabb.max)]
    rec = sel.record(**LOOK)
    for grid in (False, True):
        if grid:
            on.set_editor_grid(); off.set_editor_grid()
        on.set_selection(kw, boxes, **LOOK)
        draws = _frame(on, model); _frame(off, model)
        want = _want(on, model, draws, kw, boxes, bytes(model.camera_bytes), rec)
        _assert_layers(on, want, "glass grid=%s" % grid)
        off16 = off.read_composite()
        drawn = (off16 != off.read_opaque()).any(axis=-1)                                     # the quad's fragments (and the grid's)
        touched = _assert_image(on.read_composite(), off16, want, rec, on.read_composite_f32(), off.read_composite_f32(), "glass grid=%s" % grid)
        assert (drawn & touched).sum() >= 30, int((drawn & touched).sum())                   # overlay pixels over transparent fragments / the grid
        assert (on.read_opaque() == off.read_opaque()).all()
    assert int(want["edges"][2, :, 6].sum()) >= 4                                            # the transparent quad's own box is drawn
    on.close(); off.close()


def test_hud_meshes_are_drawn_over_the_overlay(oracle_lut):
    """The world composite (no HUD transparent pass) carries the overlay; the HUD transparent pass then draws over it: away from the HUD's pixels the
    final image is the blended one, on them it is not the world composite's."""
    W, H = 70, 45
    sc = scenes.hud_scene(W, H, tex_size=16)
    model = helpers.build_model(sc)
    on, _ = helpers.hip_frame(model, oracle_lut, hud=True)
    off, _ = helpers.hip_frame(model, oracle_lut, hud=True)
    draws = model.collect_draws()
    big = max(draws, key=lambda d: d["tri_count"])
    picked = [(big["mesh_key"], model.meshes.get(big["mesh_key"]))] + [(d["mesh_key"], model.meshes.get(d["mesh_key"])) for d in draws[:3] if d is not big]
    kw = sel.key_words([key_as_ffi(k) for k, _ in picked])
    boxes = [list(r.world_aabb.min) + list(r.world_aabb.max) for _, r in picked]
    rec = sel.record(**LOOK)
    on.set_selection(kw, boxes, **LOOK)
    _frame(off, model, hud=True, hud_transparent=False)
    world_off = off.read_composite()
    draws = _frame(on, model, hud=True, hud_transparent=False)
    want = _want(on, model, draws, kw, boxes, bytes(model.camera_bytes), rec)
    _assert_layers(on, want, "hud")
    touched = _assert_image(on.read_composite(), world_off, want, rec, what="hud, world composite")
    world_on = on.read_composite()
    _frame(off, model, hud=True); _frame(on, model, hud=True)
    final_off, final_on = off.read_composite(), on.read_composite()
    _assert_layers(on, want, "hud, with its transparent pass")                                # the HUD passes change no layer
    hud_px = (final_off != world_off).any(axis=-1)
    near = np.zeros_like(hud_px)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(np.roll(hud_px, dy, 0), dx, 1)
    assert hud_px.sum() >= 50 and (touched & hud_px).sum() >= 5 and (touched & ~near).sum() >= 20, (int(hud_px.sum()), int((touched & hud_px).sum()), int((touched & ~near).sum()))
    assert (final_on[~near] == world_on[~near]).all()
    assert (final_on[touched & hud_px] != world_on[touched & hud_px]).any(axis=-1).mean() > 0.5
    on.close(); off.close()


def test_each_overlapped_frame_keeps_the_record_it_was_given(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES, four frames with a moving camera and the selection changed between them, enqueue-only, each into its own image: every
    frame is its synchronous twin's, and a set_selection after the last enqueue reaches none of them."""
    import torch
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H = 70, 45
    model = helpers.build_model(sr.boxes(W, H))
    draws = model.collect_draws()
    kw, boxes = sel.selection_of(model, "boxes")
    picks = [dict(mesh_keys=kw[:1], boxes=boxes[:1], outline_radius=1), dict(mesh_keys=kw[1:], boxes=boxes[1:], outline_radius=4, box_half_width=1.75),
             dict(mesh_keys=kw, boxes=boxes, **LOOK), dict(mesh_keys=kw[:1], boxes=boxes[1:], flags=sel.BOXES)]
    eyes = [(3.2 - 0.35 * i, 2.6 + 0.1 * i, 3.6 - 0.2 * i) for i in range(4)]
    blocks = [sr.camera_block(eye, (0.6, 0.5, 0.6), W, H) for eye in eyes]
    dev, _ = helpers.hip_frame(model, oracle_lut)
    want = []
    for block, pick in zip(blocks, picks):
        dev.set_selection(**pick)
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.geometry_pass(draws); dev.opaque_pass(); dev.transparent_pass([]); dev.frame_end()
        want.append(dev.read_composite())
    dev.set_selection(on=None)
    dev.geometry_pass(draws); dev.opaque_pass(); dev.transparent_pass([]); dev.frame_end()
    plain = dev.read_composite()
    dev.close()
    assert all((want[i] != want[i + 1]).any(axis=-1).sum() >= 0.25 * W * H for i in range(3))
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    images = [torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in blocks]
    for block, pick, image in zip(blocks, picks, images):                                     # no frame_end between the frames
        dev.set_selection(**pick)
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.bind_composite(image.data_ptr(), H * W * 8)
        dev.geometry_pass(draws); dev.opaque_pass(); dev.transparent_pass([])
    dev.set_selection(kw, boxes, outline_color=(0.0, 1.0, 0.0, 1.0))
    dev.frame_end()
    torch.cuda.synchronize()
    for i, image in enumerate(images):
        got = image.cpu().numpy().view(np.uint16)
        assert (got == want[i]).all(), (i, int((got != want[i]).any(axis=-1).sum()))
    assert (want[3] != plain).any(axis=-1).sum() >= 20                                       # (the last frame shares its camera with the plain one)
    # the last frame's layers, with the record it was given
    rec = sel.record(flags=sel.BOXES)
    ref = sel.overlay(dev.read_visibility(), sel.draw_table(draws, model.mirrors()), kw[:1], boxes[1:], blocks[-1], W, H, rec)
    _assert_layers(dev, ref, "overlap, last frame", n_boxes=1)
    dev.close()


def test_replayed_transparent_pass_draws_the_overlay_once(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST: the frame overflows its (triangle, tile) list and frame_end replays it, the transparent pass and its overlay included —
    the composite is the one of a context that never overflowed; an overlay blended twice at alpha 0.6 would show."""
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H = 70, 45
    sc = scenes.atrium_scene(W, H, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    draws = model.collect_draws()
    big = max(draws, key=lambda d: d["tri_count"])
    rec_big = model.meshes.get(big["mesh_key"])
    kw, boxes = sel.key_words([key_as_ffi(big["mesh_key"])]), [list(rec_big.world_aabb.min) + list(rec_big.world_aabb.max)]
    devs, stats = [], []
    for small in (False, True):
        dev = HipDevice(parity_tap=True, small_bin_list=small)
        dev.set_selection(kw, boxes, **LOOK)
        dev, st = helpers.hip_frame(model, oracle_lut, dev=dev, transparent=True)
        devs.append(dev); stats.append(st)
    ref, small = devs
    assert stats[1]["bin_overflow_retries"] >= 1 and stats[0]["bin_overflow_retries"] == 0, stats
    off, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    want16, got16, off16 = ref.read_composite(), small.read_composite(), off.read_composite()
    want = _want(ref, model, draws, kw, boxes, bytes(model.camera_bytes), sel.record(**LOOK))
    _assert_layers(ref, want, "replay, reference"); _assert_layers(small, want, "replay")
    touched = _assert_image(want16, off16, want, sel.record(**LOOK), what="replay, reference")
    assert want["ring"].sum() >= 10 and touched.sum() >= 40
    assert (got16 == want16).all(), int((got16 != want16).any(axis=-1).sum())
    assert (_bits(small.read_composite_f32()) == _bits(ref.read_composite_f32())).all()
    ref.close(); small.close(); off.close()


def test_post_pass_reads_the_overlay(oracle_lut):
    """Tone mapping alone has no stencil: the display image moves on overlay pixels only, and on most of them.  With SMAA its stencils spread the
    change; the overlay's own pixels still move."""
    W, H = 70, 45
    model = helpers.build_model(sr.boxes(W, H))
    on, _ = helpers.hip_frame(model, oracle_lut)
    off, _ = helpers.hip_frame(model, oracle_lut)
    kw, boxes = sel.selection_of(model, "boxes")
    on.set_selection(kw, boxes)
    for post in (dict(tonemapping=1), dict(tonemapping=1, smaa=True)):
        draws = _frame(on, model, post=post); _frame(off, model, post=post)
        want = _want(on, model, draws, kw, boxes, bytes(model.camera_bytes), sel.record())
        touched = want["ring"] | (want["box_alpha"] > 0)
        moved = (on.read_display() != off.read_display()).any(axis=-1)
        assert touched.sum() >= 200 and moved[touched].mean() > 0.9, (int(touched.sum()), float(moved[touched].mean()))
        if "smaa" not in post:
            assert not moved[~touched].any()                                                 # a superset: nothing moves where the overlay is empty
    on.close(); off.close()


# ------------------------------------------------------------------------------------------------ the host layer

def test_selection_through_the_host_layer(oracle_lut):
    """Renderer.set_selection with a key from Renderer.pick; the box follows a translated node after update_all."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H = 70, 45
    sc = sr.boxes(W, H)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.render(sync=True)
    first_box = r.keys.mesh_keys[3]
    hits = [(x, y) for y in range(0, H, 3) for x in range(0, W, 3) if r.host.pick(x, y) == first_box]
    assert len(hits) >= 5
    opaque = dev.read_opaque()
    r.set_selection([r.host.pick(*hits[0])], **LOOK)
    rec = sel.record(**LOOK)
    mirrors = lambda: {sel.BUF_GEOM_META: r.host.mirror(sel.BUF_GEOM_META), sel.BUF_MATERIAL_META: r.host.mirror(sel.BUF_MATERIAL_META)}      # noqa: E731
    kw = sel.key_words([first_box])

    def box_at(t):      # the host's f32 AABB of the unit box under scale (0.7, 1, 0.7) and translation t: one product and one sum per coordinate
        t, s = np.asarray(t, F), np.array((0.7, 1.0, 0.7), F)
        return np.concatenate([s * F(-0.5) + t, s * F(0.5) + t]).tolist()

    for t in ((0.9, 0.5, 0.9), (2.25, 0.75, 0.5)):
        r.host.transform_set_local(r.keys.node_keys[1], t, (0, 0, 0, 1), (0.7, 1.0, 0.7))
        r.update_all(0.0)
        st = r.render(sync=True)
        assert st["forward_triangles"] == 0                                                  # the transparent pass ran, with no draws
        block = dev.buffer_read(BUF_CAMERA, 0, 512)
        want = sel.overlay(dev.read_visibility(), sel.draw_table(r.host.draw_list(), mirrors()), kw, [box_at(t)], block, W, H, rec)
        _assert_layers(dev, want, "host, box at %s" % (t,), n_boxes=1)
        assert want["ring"].sum() >= 20 and (want["box_alpha"] > 0).sum() >= 50 and int(want["edges"][0, :, 6].sum()) == 12
        _assert_image(dev.read_composite(), dev.read_opaque(), want, rec, what="host, box at %s" % (t,))
    r.set_selection(on=False)
    r.host.transform_set_local(r.keys.node_keys[1], (0.9, 0.5, 0.9), (0, 0, 0, 1), (0.7, 1.0, 0.7))
    r.update_all(0.0)
    r.render(sync=True)
    assert (dev.read_opaque() == opaque).all()
    r.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_leave_the_state_as_it_was(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H = 33, 17
    model = helpers.build_model(sel.SCENES["boxes"](W, H))
    dev, _ = helpers.hip_frame(model, oracle_lut)
    kw, boxes = sel.selection_of(model, "boxes")
    block = bytes(model.camera_bytes)
    with pytest.raises(AwsmHipError) as e:                                                   # no frame with a selection yet
        dev.read_selection(0)
    assert e.value.code == -5                                                                # AWSM_ERR_NOT_READY
    dev.set_selection(kw, boxes, outline_radius=3)
    with pytest.raises(AwsmHipError) as e:                                                   # set, but no transparent pass since
        dev.read_selection()
    assert e.value.code == -5
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
    with pytest.raises(AwsmHipError) as e:                                                   # a frame without a transparent pass
        dev.read_selection()
    assert e.value.code == -5
    rec = sel.record(outline_radius=3)
    draws = _frame(dev, model)
    want = _want(dev, model, draws, kw, boxes, block, rec)
    _assert_layers(dev, want, "before the refusals")
    nan, inf = float("nan"), float("inf")
    lo, hi = boxes[0][:3], boxes[0][3:]
    bad_calls = [dict(outline_color=(1.0, nan, 0.0, 1.0)), dict(box_color=(inf, 0.0, 0.0, 1.0)), dict(box_half_width=nan), dict(hidden_alpha=inf), dict(depth_epsilon=nan),
                 dict(flags=4), dict(flags=7), dict(outline_radius=0), dict(outline_radius=5), dict(box_half_width=0.0), dict(box_half_width=-1.0), dict(box_half_width=4.5),
                 dict(outline_color=(1.0, 1.0, 1.0, 1.5)), dict(box_color=(1.0, 1.0, 1.0, -0.1)), dict(hidden_alpha=1.25), dict(hidden_alpha=-0.5), dict(depth_epsilon=-1e-6),
                 dict(struct_size=2), dict(struct_size=5000),
                 dict(boxes=[hi[:1] + lo[1:] + lo[:1] + hi[1:]]), dict(boxes=[lo[:2] + hi[2:] + hi[:2] + lo[2:]]), dict(boxes=[[nan, 0, 0, 1, 1, 1]]),
                 dict(mesh_keys=[(1, i) for i in range(65)]), dict(boxes=[boxes[0]] * 65), dict(n_keys=3, mesh_keys=[]), dict(n_boxes=2, boxes=[])]
    for bad in bad_calls:
        args = dict(mesh_keys=kw[:1], boxes=boxes[:1])
        args.update(bad)
        with pytest.raises(AwsmHipError) as e:
            dev.set_selection(**args)
        assert e.value.code == -1, bad                                                       # AWSM_ERR_INVALID_ARGUMENT
    draws = _frame(dev, model)
    _assert_layers(dev, _want(dev, model, draws, kw, boxes, block, rec), "after the refusals")      # a refused call changes nothing
    dev.set_selection(kw, boxes, struct_size=12, outline_radius=1, box_half_width=3.0)       # flags and the radius are known: the rest keeps its defaults
    draws = _frame(dev, model)
    _assert_layers(dev, _want(dev, model, draws, kw, boxes, block, sel.record(outline_radius=1)), "struct_size 12")
    dev.set_selection(kw * 32, boxes[:1] * 64)                                               # the caps themselves are fine
    _frame(dev, model)
    # nothing to draw is off: no keys and no boxes, or flags that reach neither
    for nothing in (dict(mesh_keys=[], boxes=[]), dict(mesh_keys=kw, boxes=[], flags=sel.BOXES), dict(mesh_keys=[], boxes=boxes, flags=sel.OUTLINE), dict(mesh_keys=kw, boxes=boxes, flags=0)):
        dev.set_selection(**nothing)
        _frame(dev, model)
        with pytest.raises(AwsmHipError) as e:
            dev.read_selection(0)
        assert e.value.code == -5, nothing
        assert (dev.read_composite() == dev.read_opaque()).all()
    dev.close()
    for shard in ("rows", "bands"):
        dev = HipDevice(parity_tap=True)
        dev.set_selection(kw, boxes)
        dev.resize(W, H, 0)
        if shard == "rows":
            dev.set_shard_rows(0, 9)
        else:
            dev.set_shard_bands(2, 0)
        dev.upload_mirrors(model.mirrors())
        for i, smp in enumerate(model.scene.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(model.scene.skybox_rgba, model.scene.prefiltered_rgb, model.scene.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        dev.geometry_pass(model.collect_draws()); dev.opaque_pass()
        import torch
        gathered = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
        dev.bind_opaque_source(gathered.data_ptr(), H * W * 8)
        with pytest.raises(AwsmHipError) as e:
            dev.transparent_pass([])
        assert e.value.code == -6, shard                                                     # AWSM_ERR_UNSUPPORTED
        dev.set_selection(on=None)
        dev.transparent_pass([]); dev.frame_end()                                            # off: the shard renders as ever
        dev.close()
