"""GPU: clip positions formed in the binning, the geometry cache decided once per draw, the fill pass on compact records (frame_params.hpp:
FrameDev::clip_from_world / draw_hit_at / bin_rec_at; AWSM_CLIP_IN_BIN=0 turns the three off together).

None of it may change a bit: a world geometry pass with a wcache stores no clip positions — k_bin<count> forms view_proj * wcache itself, through the
function the vertex stage's full path uses — a workgroup of an unchanged draw leaves after two loads, and k_bin<fill> takes the tiles of a small
triangle from the count pass's 8-byte record.  So every frame here is compared bit for bit against the oracle AND against a second context created
with AWSM_GEOMETRY_CACHE=0 (no wcache: k_deform_transform writes clip, k_bin reads it): the clip positions awsm_hip_read_transformed returns, the
visibility keys, and the bin statistics (triangles_binned, bin_entries — the set of (triangle, tile) pairs has one size).  Small frames: an atrium at
256x160 whose tiles hold small and big triangles side by side, a skinned + morphed mesh at 128x96."""
import copy
import os

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from oracle import oracle_lib
from tests import helpers

pytestmark = pytest.mark.gpu

THREADS = 8


def _device(env, **kw):
    from awsm_renderer_amd.hip_backend import HipDevice
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return HipDevice(parity_tap=True, **kw)      # the switches are read at awsm_hip_create
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


NEW, CACHE_OFF, KNOB_OFF = {}, {"AWSM_GEOMETRY_CACHE": "0"}, {"AWSM_CLIP_IN_BIN": "0"}


def _write_changes(dev, before, after):
    """awsm_hip_buffer_write for exactly the words in which two mirror sets differ, merged into runs (what a dirty-range writer sends)"""
    for which, new in after.items():
        a, b = np.frombuffer(bytes(before[which]), dtype=np.uint32), np.frombuffer(bytes(new), dtype=np.uint32)
        assert a.size == b.size, which
        idx = np.nonzero(a != b)[0]
        if idx.size == 0:
            continue
        starts = np.concatenate([[0], np.nonzero(np.diff(idx) > 1)[0] + 1])
        ends = np.concatenate([starts[1:], [idx.size]])
        for s, e in zip(starts, ends):
            lo, hi = int(idx[s]) * 4, (int(idx[e - 1]) + 1) * 4
            dev.buffer_write(which, lo, np.frombuffer(bytes(new[lo:hi]), dtype=np.uint8))


class Ctx:
    """One context: its first frame creates and fills every buffer; later frames write what changed in the mirrors and render."""

    def __init__(self, env, model, lut, overlap=True, msaa=0, hud=False):
        self.dev = _device(env, overlap_frames=overlap)
        self.msaa, self.hud = msaa, hud
        _, self.stats = helpers.hip_frame(model, lut, dev=self.dev, msaa=msaa, hud=hud)
        self.mirrors = model.mirrors()

    def frame(self, model, draws=None):
        new = model.mirrors()
        _write_changes(self.dev, self.mirrors, new)
        self.mirrors = new
        d = self.dev
        d.geometry_pass(model.collect_draws() if draws is None else draws)
        if self.hud:
            d.hud_geometry_pass(model.hud_geometry_draws)
        d.opaque_pass()
        if self.hud:
            d.transparent_pass(model.collect_transparent_draws())
            d.hud_transparent_pass(model.hud_transparent_draws)
        self.stats = d.frame_end()
        return self.stats

    def close(self):
        self.dev.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_frame(tag, new, ref, orc=None, rows=None):
    """clip, keys and bin statistics of `new` against the reference context and (given) the oracle, bit for bit; rows: the rows the shard owns"""
    n = 3 * new.stats["triangles_in"]
    clip, nt = new.dev.read_transformed(n)
    rclip, rnt = ref.dev.read_transformed(n)
    assert (_bits(clip) == _bits(rclip)).all() and (_bits(nt) == _bits(rnt)).all(), tag
    keys, rkeys = new.dev.read_visibility(), ref.dev.read_visibility()
    sel = slice(None) if rows is None else rows
    assert (keys[sel] == rkeys[sel]).all(), tag
    for k in ("triangles_binned", "bin_entries", "covered_pixels"):
        assert new.stats[k] == ref.stats[k], (tag, k, new.stats, ref.stats)
    if orc is not None:
        assert n == orc.n_verts and (_bits(clip) == _bits(orc.clip)).all() and (_bits(nt) == _bits(orc.nt)).all(), tag
        assert (keys[sel] == orc.keys[sel]).all(), tag
    return keys


def _placed(draws):
    """a draw as the geometry cache sees it: its place in the list, its first triangle, its record"""
    out, first = set(), 0
    for i, d in enumerate(draws):
        out.add((i, first, tuple(sorted((k, v) for k, v in d.items() if k != "mesh_key"))))
        first += d["tri_count"]
    return out


def _blocks(draws):
    return sum((3 * d["tri_count"] + 255) // 256 for d in draws)


def _atrium():
    return scenes.atrium_scene(256, 160, detail=0.1, tex_scale=1 / 32)


def _atrium_eye(i):
    return (0.4 + 2.5 * np.sin(0.35 * i), 3.1 + 0.05 * i, 17.0 - 0.8 * i)


def _with_camera(scene, eye, target):
    from awsm_renderer_amd.scenes import look_at_rh
    sc = copy.deepcopy(scene)
    eye = tuple(float(x) for x in eye)
    sc.view, sc.camera_position = look_at_rh(eye, target), eye
    return sc


def _skinned():
    """skinned + morphed tube, morphed cube, and a box none of the writes concerns"""
    from awsm_renderer_amd.scene_desc import NodeDesc
    base = scenes.skinned_morph_scene(128, 96, around=12, along=24, tex_size=16)
    box = copy.deepcopy(scenes.box_scene().nodes[1].primitives[0])
    box.material = 1
    base.nodes.append(NodeDesc(translation=(-1.5, 0.3, 0.2), scale=(0.5, 0.5, 0.5), primitives=[box]))
    return base


def _orc(model, lut, rows=(0, 0)):
    return oracle_lib.frame_from_model(model, lut, rows=rows).transform().raster(THREADS)


def _has_big_and_small(clip, width, height):
    """from the clip positions: does the frame hold triangles over more than 16 tiles (the full-record walk) and triangles over fewer (compact records)?"""
    t = clip.reshape(-1, 3, 4).astype(np.float64)
    front = (t[..., 3] > 0).all(axis=1)
    t = t[front]
    x = (t[..., 0] / t[..., 3] * 0.5 + 0.5) * width
    y = (0.5 - t[..., 1] / t[..., 3] * 0.5) * height
    x0, x1 = np.clip(x.min(axis=1), 0, width - 1), np.clip(x.max(axis=1), 0, width - 1)
    y0, y1 = np.clip(y.min(axis=1), 0, height - 1), np.clip(y.max(axis=1), 0, height - 1)
    on = (x.max(axis=1) >= 0) & (x.min(axis=1) < width) & (y.max(axis=1) >= 0) & (y.min(axis=1) < height)
    tiles = ((x1 // 32 - x0 // 32 + 1) * (y1 // 32 - y0 // 32 + 1))[on]
    return bool((tiles > 16).any() and (tiles <= 16).any())


@pytest.mark.parametrize("scene", ["atrium", "skinned"])
def test_moving_camera_overlapped_frames(scene, oracle_lut):
    """Eight overlapped frames of a moving camera: from the third on every draw that kept its place in the slot's list is a cache hit — nothing is written
    per vertex, its clip positions exist only inside k_bin — and every frame is the oracle's and the cache-off context's."""
    base = _atrium() if scene == "atrium" else _skinned()
    target = (-0.2, 3.4, -18.0) if scene == "atrium" else (0.4, 0.1, 0.0)
    eye = _atrium_eye if scene == "atrium" else (lambda i: (1.1 - 0.15 * i, 0.7 + 0.03 * i, 4.9 - 0.1 * i))
    first = helpers.build_model(_with_camera(base, eye(0), target))
    new, ref = Ctx(NEW, first, oracle_lut), Ctx(CACHE_OFF, first, oracle_lut)
    big_and_small, hits, blocks = False, 0, 0
    lists = [_placed(first.collect_draws())]
    for i in range(1, 9):
        model = helpers.build_model(_with_camera(base, eye(i), target))
        draws = model.collect_draws()
        st = new.frame(model, draws); ref.frame(model, draws)
        _same_frame((scene, i), new, ref, _orc(model, oracle_lut))
        assert st["geometry_blocks"] == _blocks(draws) and ref.stats["geometry_cache_blocks"] == 0
        lists.append(_placed(draws))
        if i >= 2:      # a draw hits when it sits where it sat in the list this SLOT's arrays were computed for (the camera's culling and sorting move draws)
            want = sum((3 * dict(p[2])["tri_count"] + 255) // 256 for p in lists[i] if p in lists[i - 2])
            assert st["geometry_cache_blocks"] == want, (scene, i, st, want)
            hits += want; blocks += st["geometry_blocks"]
        big_and_small |= _has_big_and_small(new.dev.read_transformed(3 * st["triangles_in"])[0], base.width, base.height)
    assert hits > 0 and blocks > 0      # workgroups of these frames took the path that writes nothing
    if scene == "atrium":
        assert big_and_small      # triangles over many tiles (walked from the full records) beside small ones (compact records)
    new.close(); ref.close()


def test_writes_between_frames_recompute_one_draw(oracle_lut):
    """A node transform, a joint and a morph weight written between overlapped frames: exactly the written draw's workgroups are recomputed (the decision
    is taken once per draw now), in both frame slots, and both frames are bit-exact — the rewritten draw's wcache and every kept draw's."""
    from awsm_renderer_amd.scenes import quat_axis_angle
    base = _skinned()
    cube_node, joint_node = len(base.nodes) - 2, 6

    def variant(moved=False, joint=False, morph=False):
        sc = _with_camera(base, (1.1, 0.7, 4.9), (0.4, 0.1, 0.0))
        if moved:
            sc.nodes[cube_node].translation = (1.45, 0.25, 0.1)
        if joint:
            sc.nodes[joint_node].rotation = quat_axis_angle((0, 0, 1), 0.31)
        if morph:
            sc.nodes[cube_node].primitives[0].animated_morph_weights = np.array([0.55, 0.2], dtype=np.float32)
        return helpers.build_model(sc)

    model = variant()
    new, ref = Ctx(NEW, model, oracle_lut), Ctx(CACHE_OFF, model, oracle_lut)
    for c in (new, ref):
        c.frame(model)                               # the second slot's first frame
    steps = [("nothing", dict(), None), ("transform", dict(moved=True), "cube"), ("joint", dict(moved=True, joint=True), "tube"),
             ("morph weight", dict(moved=True, joint=True, morph=True), "cube"), ("nothing again", dict(moved=True, joint=True, morph=True), None)]
    for name, kw, written in steps:
        model = variant(**kw)
        draws = model.collect_draws()
        offs = sorted({d["geom_meta_off"] for d in draws})
        assert len(offs) == 3
        mesh_of = dict(zip(offs, ("tube", "cube", "box")))      # mesh insertion order = meta slot order
        recomputed = sum((3 * d["tri_count"] + 255) // 256 for d in draws if mesh_of[d["geom_meta_off"]] == written)
        orc = _orc(model, oracle_lut)
        for rep in range(2):                                   # one frame per frame slot: each slot sees the writes since ITS last frame
            st = new.frame(model, draws); ref.frame(model, draws)
            assert st["geometry_blocks"] == _blocks(draws) and st["geometry_blocks"] - st["geometry_cache_blocks"] == recomputed, (name, rep, st, recomputed)
            assert (written is None) == (recomputed == 0)
            _same_frame((name, rep), new, ref, orc)
    new.close(); ref.close()


def test_draw_list_that_changes_and_returns(oracle_lut):
    """A draw dropped (every draw behind it moves in rank space), the list reversed, cut, and back: per-draw decisions follow the list, keys stay right."""
    model = helpers.build_model(_with_camera(_skinned(), (1.1, 0.7, 4.9), (0.4, 0.1, 0.0)))
    draws = model.collect_draws()
    new, ref = Ctx(NEW, model, oracle_lut), Ctx(CACHE_OFF, model, oracle_lut)
    for k, lst in enumerate((draws, draws[1:], draws, list(reversed(draws)), draws[:2], draws, draws, draws)):
        new.frame(model, lst); ref.frame(model, lst)
        _same_frame(("list", k), new, ref)
    orc = _orc(model, oracle_lut)
    _same_frame("list back", new, ref, orc)
    assert new.stats["geometry_cache_blocks"] == new.stats["geometry_blocks"]      # the list stood still for a frame of this slot: all hits again
    new.close(); ref.close()


def test_band_shards_and_a_row_strip(oracle_lut):
    """set_shard_bands(2, r) for both r on one GPU, then a row strip: the set-up phase drops most triangles from the clip positions it has just formed;
    the keys of the owned rows are the full frame's."""
    from awsm_renderer_amd import sharding
    sc = _atrium()
    model = helpers.build_model(_with_camera(sc, _atrium_eye(2), (-0.2, 3.4, -18.0)))
    orc = _orc(model, oracle_lut)
    new, ref = Ctx(NEW, model, oracle_lut, overlap=False), Ctx(CACHE_OFF, model, oracle_lut, overlap=False)
    _same_frame("full", new, ref, orc)
    for r in range(2):
        rows = np.array(sharding.band_rows(sc.height, 2, r), dtype=np.int64)
        for c in (new, ref):
            c.dev.set_shard_bands(2, r)
        for rep in range(2):                  # the second one: all cache hits
            new.frame(model); ref.frame(model)
            _same_frame(("bands", r, rep), new, ref, orc, rows=rows)
    for c in (new, ref):
        c.dev.set_shard_bands(1, 0)
        c.dev.set_shard_rows(37, 101)
    for rep in range(2):
        new.frame(model); ref.frame(model)
        _same_frame(("rows", rep), new, ref, orc, rows=np.arange(37, 101))
    new.close(); ref.close()


@pytest.mark.parametrize("msaa", [0, 4])
def test_frame_with_hud_meshes(msaa, oracle_lut):
    """A HUD geometry pass behind the world's (MSAA x4: the hud triangles in the world pass's rank space, rank0 > 0, their clip positions stored behind
    the world's by the hud pass's own transform): world keys against the oracle, keys, opaque image and composite against the cache-off context."""
    model = helpers.build_model(scenes.hud_scene(160, 96, tex_size=16))
    new, ref = Ctx(NEW, model, oracle_lut, msaa=msaa, hud=True), Ctx(CACHE_OFF, model, oracle_lut, msaa=msaa, hud=True)
    keys = oracle_lib.frame_with_hud_msaa(model, oracle_lut, threads=THREADS, msaa=4).keys if msaa else _orc(model, oracle_lut).keys
    for rep in range(4):
        if rep:
            new.frame(model); ref.frame(model)
        assert (new.dev.read_visibility() == keys).all() and (ref.dev.read_visibility() == keys).all(), rep
        assert (new.dev.read_opaque() == ref.dev.read_opaque()).all() and (new.dev.read_composite() == ref.dev.read_composite()).all(), rep
        for k in ("triangles_binned", "bin_entries", "covered_pixels"):
            assert new.stats[k] == ref.stats[k], (rep, k)
    assert new.stats["geometry_cache_blocks"] == new.stats["geometry_blocks"] > 0
    new.close(); ref.close()


def test_read_transformed_returns_the_rendered_frames_clip(oracle_lut):
    """After a frame of cache hits no clip position is in memory: awsm_hip_read_transformed forms them from wcache and the camera snapshot the frame was
    submitted with — also after a camera write that no frame has rendered yet, and twice in a row."""
    sc = _atrium()
    target = (-0.2, 3.4, -18.0)
    models = [helpers.build_model(_with_camera(sc, _atrium_eye(i), target)) for i in range(4)]
    new = Ctx(NEW, models[0], oracle_lut)
    for m in models[1:] + [models[3], models[3]]:      # (the last one: the list its slot's arrays were computed for)
        st = new.frame(m)
    assert st["geometry_cache_blocks"] == st["geometry_blocks"] > 0
    orc = _orc(models[3], oracle_lut)
    clip, nt = new.dev.read_transformed(orc.n_verts)
    assert (_bits(clip) == _bits(orc.clip)).all() and (_bits(nt) == _bits(orc.nt)).all()
    other = helpers.build_model(_with_camera(sc, (3.0, 5.0, 9.0), target)).mirrors()
    _write_changes(new.dev, new.mirrors, other)                # the camera block, not rendered
    new.mirrors = other
    for _ in range(2):
        clip2, _nt = new.dev.read_transformed(orc.n_verts)
        assert (_bits(clip2) == _bits(orc.clip)).all()
    # ... and the next frame is the new camera's
    m = helpers.build_model(_with_camera(sc, (3.0, 5.0, 9.0), target))
    new.frame(m)
    o2 = _orc(m, oracle_lut)
    clip3, _nt = new.dev.read_transformed(o2.n_verts)
    assert (_bits(clip3) == _bits(o2.clip)).all() and (new.dev.read_visibility() == o2.keys).all()
    new.close()


@pytest.mark.parametrize("scene", ["atrium", "skinned"])
def test_knob_off_gives_the_same_frames(scene, oracle_lut):
    """AWSM_CLIP_IN_BIN=0: the earlier path in the same library (clip stored by the vertex stage, a decision per workgroup, set-up records in the fill
    pass) — same clip, keys, statistics and cache hits, frame by frame."""
    base = _atrium() if scene == "atrium" else _skinned()
    target = (-0.2, 3.4, -18.0) if scene == "atrium" else (0.4, 0.1, 0.0)
    eye = _atrium_eye if scene == "atrium" else (lambda i: (1.1 - 0.15 * i, 0.7 + 0.03 * i, 4.9 - 0.1 * i))
    first = helpers.build_model(_with_camera(base, eye(0), target))
    new, off = Ctx(NEW, first, oracle_lut), Ctx(KNOB_OFF, first, oracle_lut)
    for i in (1, 2, 3, 4):
        model = helpers.build_model(_with_camera(base, eye(i), target))
        new.frame(model); off.frame(model)
        _same_frame((scene, i), new, off, _orc(model, oracle_lut) if i == 4 else None)
        assert new.stats["geometry_cache_blocks"] == off.stats["geometry_cache_blocks"] and new.stats["geometry_blocks"] == off.stats["geometry_blocks"]
    new.close(); off.close()
