"""GPU tests of picking through the transparent passes: awsm_hip_read_pick_map at EVERY pixel against tests/pick_reference.py (which
never reads the device's fragment lists), awsm_hip_pick_ex and awsm_hip_pick_rect against the map and the restatement, under MSAA x 4, with HUD
passes, in overlap mode, through a replayed frame, through the host layer, and the refusals.  Frames of 8 x 5, 33 x 17 and 70 x 45 only."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers
from tests import pick_reference as pr
from tests.test_pick_cpu import FLOORS, _texture_case, msaa_band

pytestmark = pytest.mark.gpu
NOT_READY, INVALID, UNSUPPORTED = -5, -1, -6
# pick_ex's depth of a fragment is the raster contract's f32 plane evaluation of f32 clip coordinates; the restatement interpolates the same
# corners in f64.  A few f32 roundings (2^-24 each) of values below 1, through a division by w: 1e-5 holds them with room and is a tenth of the
# 1e-4 by which any two compared surfaces differ.  The alpha is f16 on the restatement's side: half an f16 step below 1 is 2^-12.
DEPTH_TOL, ALPHA_TOL = 1e-5, 2.0 ** -11


def _first(bad):
    return tuple(int(v) for v in np.argwhere(bad)[0])


def frame(name, W, H, lut, msaa=0, dev=None, transparent=None, **ref_kw):
    """One frame of a scene on the device and its restatement."""
    model = helpers.build_model(pr.SCENES[name](W, H))
    hud = name == "hud"
    dev, _ = helpers.hip_frame(model, lut, transparent=True, hud=hud, msaa=msaa, dev=dev)
    if transparent is not None:      # the same frame once more with another world transparent list
        model.collect_draws()
        t = transparent(model.collect_transparent_draws())
        again(dev, model, t, hud)
        ref_kw["transparent"] = t
    return dev, pr.Reference(model, lut, hud=hud, **ref_kw), model


def again(dev, model, transparent=None, hud=False, end=True, transparent_pass=True):
    dev.geometry_pass(model.collect_draws())
    if hud:
        dev.hud_geometry_pass(model.hud_geometry_draws)
    dev.opaque_pass()
    if transparent_pass:
        dev.transparent_pass(model.collect_transparent_draws() if transparent is None else transparent)
    if hud:
        dev.hud_transparent_pass(model.hud_transparent_draws)
    if end:
        dev.frame_end()


def assert_map(dev, ref, transparent, thr, what, keep=None, msaa=False):
    """The device's map against the restatement's at every pixel of `keep` (None: all) -> the restatement's answer.  msaa: sample 0 is not the
    pixel's centre, so the triangle index is compared where no 8-neighbour's triangle differs in the restatement."""
    word, tri = dev.read_pick_map(transparent, thr)
    ans = ref.answer(transparent, thr)
    keep = np.ones(word.shape, bool) if keep is None else keep
    if msaa:
        both = ans["word"].astype(np.int64) << 32 | ans["triangle"]
        ans["sure_triangle"] = ans["sure_triangle"] & ~pr.erode_dilate_band([both == v for v in np.unique(both)])
    bad = (word != ans["word"]) & keep
    assert not bad.any(), "%s: %d of %d compared pixels differ, first at (y, x) = %s: device %#x, restatement %#x" % (
        what, int(bad.sum()), int(keep.sum()), _first(bad), int(word[_first(bad)]), int(ans["word"][_first(bad)]))
    bad = (tri != ans["triangle"]) & keep & ans["sure_triangle"]
    assert not bad.any(), "%s: %d triangle indices differ, first at %s: device %d, restatement %d" % (
        what, int(bad.sum()), _first(bad), int(tri[_first(bad)]), int(ans["triangle"][_first(bad)]))
    assert (tri[word == pr.MISS] == pr.MISS).all()
    return ans, word, tri


def assert_floor(ref, ans, case):
    wins = ref.wins(ans)
    print(case, wins, "floor", FLOORS[case])
    assert all(w >= f for w, f in zip(wins, FLOORS[case])), (case, wins, FLOORS[case])


# ------------------------------------------------------------------------------------------------ the flag off

@pytest.mark.parametrize("W,H", pr.SIZES)
def test_without_the_flag_every_pixel_is_awsm_hip_picks_answer(W, H, oracle_lut):
    """valid, key words and triangle index of awsm_hip_pick at every pixel, with HUD geometry, against the map and against pick_ex."""
    dev, ref, _ = frame("hud", W, H, oracle_lut)
    ans, word, tri = assert_map(dev, ref, False, 0.5, "flag off %dx%d" % (W, H))
    assert (ans["layer"] == pr.HUD).sum() >= FLOORS[("hud", W, H, 0.5)][2] and (ans["layer"] == pr.WORLD).sum() >= FLOORS[("hud", W, H, 0.7)][0]
    for y in range(-1, H + 1):
        for x in range(-1, W + 1):
            old, new = dev.pick(x, y), dev.pick_ex(x, y)
            if not (0 <= x < W and 0 <= y < H) or word[y, x] == pr.MISS:
                assert old is None and new is None, (x, y, old, new)
                continue
            layer, draw = int(word[y, x]) >> 28, int(word[y, x]) & 0x0FFFFFFF
            assert old == (ref.key_of(layer, draw), int(tri[y, x])), (x, y, old, hex(word[y, x]))
            assert (new["mesh_key"], new["triangle_index"]) == old and new["layer"] == layer and new["alpha"] == 1.0 and new["depth_bits"] == ans["depth_bits"][y, x], (x, y, new)
    dev.close()


def test_the_flag_without_a_transparent_pass_is_the_opaque_answer(oracle_lut):
    model = helpers.build_model(pr.SCENES["glass"](33, 17))
    dev, _ = helpers.hip_frame(model, oracle_lut)                                             # geometry and opaque passes only
    ref = pr.Reference(model, oracle_lut, transparent_pass=False)
    on, _, _ = assert_map(dev, ref, True, 0.5, "flag, no transparent pass")
    off, _, _ = assert_map(dev, ref, False, 0.5, "no flag, no transparent pass")
    assert (on["word"] == off["word"]).all() and (on["layer"] == pr.WORLD).sum() >= 60
    dev.close()


# ------------------------------------------------------------------------------------------------ the rule, scene by scene

@pytest.mark.parametrize("W,H", pr.SIZES)
def test_a_blend_quad_is_picked_at_0_5_and_seen_through_at_0_7(W, H, oracle_lut):
    dev, ref, _ = frame("glass", W, H, oracle_lut)
    lo, _, _ = assert_map(dev, ref, True, 0.5, "glass 0.5 %dx%d" % (W, H))
    hi, _, _ = assert_map(dev, ref, True, 0.7, "glass 0.7 %dx%d" % (W, H))
    assert_floor(ref, lo, ("glass", W, H, 0.5)); assert_floor(ref, hi, ("glass", W, H, 0.7))
    pane = ref.tr[0]["touched"]
    off = ref.answer(False)
    assert (lo["layer"][pane] == pr.WORLD_TRANSPARENT).all() and (hi["word"] == off["word"]).all()
    assert W < 33 or ((off["layer"][pane] == pr.WORLD).sum() >= 30 and (off["layer"][pane] < 0).sum() >= 30)      # over opaque geometry and over background
    dev.close()


@pytest.mark.parametrize("W,H", pr.SIZES)
def test_the_back_pane_is_picked_through_the_front_one(W, H, oracle_lut):
    dev, ref, _ = frame("panes", W, H, oracle_lut)
    ans, _, _ = assert_map(dev, ref, True, 0.5, "panes %dx%d" % (W, H))
    assert_floor(ref, ans, ("panes", W, H, 0.5))
    both = ref.tr[0]["touched"] & ref.tr[1]["touched"]
    assert both.sum() >= (300 if W == 70 else 4) and (ans["word"][both] == (pr.WORLD_TRANSPARENT << 28 | 0)).all()
    low, _, _ = assert_map(dev, ref, True, 0.25, "panes 0.25 %dx%d" % (W, H))                  # and at 0.25 the front one itself
    assert (low["word"][ref.tr[1]["touched"]] == (pr.WORLD_TRANSPARENT << 28 | 1)).all()
    dev.close()


@pytest.mark.parametrize("W,H", pr.SIZES[1:])
def test_submitted_front_first_the_far_pane_is_absent(W, H, oracle_lut):
    dev, ref, _ = frame("panes", W, H, oracle_lut, transparent=lambda t: [t[1], t[0]])
    ans, _, _ = assert_map(dev, ref, True, 0.5, "panes, front first %dx%d" % (W, H))
    both = ref.tr[0]["touched"] & ref.tr[1]["touched"]
    off = ref.answer(False)
    assert both.sum() >= 40 and (ans["word"][both] == off["word"][both]).all()                 # behind the 0.3 pane's depth nothing was listed
    only_back = ref.tr[1]["touched"] & ~ref.tr[0]["touched"]
    assert only_back.sum() >= 20 and (ans["word"][only_back] == (pr.WORLD_TRANSPARENT << 28 | 1)).all()
    dev.close()


@pytest.mark.parametrize("mode", ["blend", "mask"])
def test_texture_alpha_in_blocks(mode, oracle_lut):
    """A nearest-sampled 0.2 / 0.9 texture in blocks of 19 pixels and more; pixels within one pixel of a block border are left out."""
    ref, uv, inside, band = _texture_case(oracle_lut, mode)
    share = band.sum() / inside.sum()
    assert share <= 0.25, share
    dev, _ = helpers.hip_frame(ref.model, oracle_lut, transparent=True)
    ans, _, _ = assert_map(dev, ref, True, 0.5, "texture %s" % mode, keep=~band)
    assert_floor(ref, ans, ("textured" if mode == "blend" else "mask", 70, 45, 0.5))
    if mode == "mask":
        ys, xs = np.nonzero((ans["layer"] == pr.WORLD_TRANSPARENT) & ~band)
        for y, x in list(zip(ys, xs))[::97]:
            assert dev.pick_ex(int(x), int(y), True, 0.99)["alpha"] == 1.0                      # a fragment that survived its cutoff
    dev.close()


@pytest.mark.parametrize("W,H", pr.SIZES)
def test_instances_and_a_mesh_behind_the_wall(W, H, oracle_lut):
    dev, ref, _ = frame("instanced", W, H, oracle_lut)
    for thr in (0.0, 0.5, 1.0):
        ans, word, _ = assert_map(dev, ref, True, thr, "instanced %g %dx%d" % (thr, W, H))
    assert (ans["layer"] != pr.WORLD_TRANSPARENT).all()                                        # nothing was drawn with alpha 1
    ans = ref.answer(True, 0.5)
    assert_floor(ref, ans, ("instanced", W, H, 0.5))
    hidden = [i for i, d in enumerate(ref.tr) if not d["touched"].any()]
    assert len(hidden) == 1 and not (ans["word"] == (pr.WORLD_TRANSPARENT << 28 | hidden[0])).any()
    dev.close()


@pytest.mark.parametrize("W,H", pr.SIZES)
def test_all_four_layers_win_somewhere(W, H, oracle_lut):
    dev, ref, _ = frame("hud", W, H, oracle_lut)
    for thr in (0.5, 0.7):
        ans, _, _ = assert_map(dev, ref, True, thr, "hud %g %dx%d" % (thr, W, H))
        assert_floor(ref, ans, ("hud", W, H, thr))
    dev.close()


@pytest.mark.parametrize("name", ["glass", "hud"])
def test_msaa_reads_sample_0(name, oracle_lut):
    """MSAA x 4 on the device, one sample in the restatement: compared where a pixel lies one pixel inside or outside every layer's coverage."""
    W, H = 70, 45
    dev, ref, _ = frame(name, W, H, oracle_lut, msaa=4)
    band = msaa_band(ref)
    assert band.mean() <= 0.30, band.mean()
    for transparent in (False, True):
        ans, _, _ = assert_map(dev, ref, transparent, 0.5, "msaa %s flag=%s" % (name, transparent), keep=~band, msaa=True)
    kept = [int(((ans["layer"] == L) & ~band).sum()) for L in range(4)]
    print("msaa", name, "kept per layer", kept, "band", float(band.mean()))
    assert all(k >= f // 2 for k, f in zip(kept, FLOORS[(name, W, H, 0.5)])), kept
    ys, xs = np.nonzero((ans["layer"] == pr.WORLD_TRANSPARENT) & ~band)
    for y, x in list(zip(ys, xs))[::61]:
        hit = dev.pick_ex(int(x), int(y), True, 0.5)
        # (the panes face the camera: their depth is the same at sample 0 as at the centre)
        assert abs(hit["alpha"] - ans["alpha"][y, x]) <= ALPHA_TOL and abs(float(np.uint32(hit["depth_bits"]).view(np.float32)) - ans["depth"][y, x]) <= DEPTH_TOL
    dev.close()


# ------------------------------------------------------------------------------------------------ pick_ex and pick_rect

def test_pick_ex_is_the_map_with_alpha_and_depth(oracle_lut):
    W, H = 70, 45
    dev, ref, _ = frame("hud", W, H, oracle_lut)
    ans, word, tri = assert_map(dev, ref, True, 0.5, "pick_ex")
    seen = set()
    for y in range(1, H, 4):
        for x in range(2, W, 5):
            hit = dev.pick_ex(x, y, True, 0.5)
            if word[y, x] == pr.MISS:
                assert hit is None
                continue
            L, d = int(word[y, x]) >> 28, int(word[y, x]) & 0x0FFFFFFF
            seen.add(L)
            assert (hit["layer"], hit["mesh_key"], hit["triangle_index"]) == (L, ref.key_of(L, d), int(tri[y, x])), (x, y, hit)
            got_depth = float(np.uint32(hit["depth_bits"]).view(np.float32))
            if L in (pr.WORLD, pr.HUD):
                assert hit["alpha"] == 1.0 and hit["depth_bits"] == ans["depth_bits"][y, x], (x, y, hit)
            else:
                assert abs(hit["alpha"] - ans["alpha"][y, x]) <= ALPHA_TOL and abs(got_depth - ans["depth"][y, x]) <= DEPTH_TOL, (x, y, hit, ans["alpha"][y, x], ans["depth"][y, x])
    assert seen == {0, 1, 2, 3}
    dev.close()


@pytest.mark.parametrize("name", ["hud", "instanced"])
def test_pick_rect(name, oracle_lut):
    W, H = 70, 45
    dev, ref, _ = frame(name, W, H, oracle_lut)
    for transparent in (True, False):
        ans, word, _ = assert_map(dev, ref, transparent, 0.5, "rect %s" % name)
        # the whole frame; a rectangle across 16 x 16 borders and over the frame's edge; one inside one tile; rows and columns of one pixel
        for r in ((0, 0, W, H), (10, 7, 80, 40), (-4, -9, 37, 100), (17, 18, 30, 29), (0, 20, W, 21), (33, 0, 34, H)):
            got, n = dev.pick_rect(*r, transparent=transparent)
            want = pr.rect(ans, ref, *r)
            assert got == want and n == len(want), (r, got, want)
            x0, y0, x1, y1 = max(r[0], 0), max(r[1], 0), min(r[2], W), min(r[3], H)
            assert sum(e[2] for e in got) == int((word[y0:y1, x0:x1] != pr.MISS).sum())
        assert len(pr.rect(ans, ref, 0, 0, W, H)) >= ((4 if transparent else 3) if name == "hud" else (2 if transparent else 1))
    # a 1 x 1 rectangle is pick_ex
    for (x, y) in ((5, 5), (30, 22), (52, 12), (69, 44), (12, 6), (58, 8)):
        hit = dev.pick_ex(x, y, True, 0.5)
        got, n = dev.pick_rect(x, y, x + 1, y + 1, True, 0.5)
        assert got == ([(hit["layer"], hit["mesh_key"], 1)] if hit else []) and n == len(got), (x, y, hit, got)
    # empty rectangles
    for r in ((5, 5, 5, 9), (9, 9, 3, 12), (W, 0, W + 5, H), (-9, -9, 0, 0), (0, H, W, H + 1)):
        assert dev.pick_rect(*r, transparent=True) == ([], 0), r
    # cap below the distinct count: n_out says how many there are, the first cap are written
    whole, n = dev.pick_rect(0, 0, W, H, True, 0.5)
    assert n == len(whole) >= 2
    for cap in (0, 1, n - 1):
        got, n_cap = dev.pick_rect(0, 0, W, H, True, 0.5, cap=cap)
        assert n_cap == n and got == whole[:cap], (cap, got)
    # integer sums: the same answer every time
    assert all(dev.pick_rect(0, 0, W, H, True, 0.5) == (whole, n) for _ in range(3))
    dev.close()


# ------------------------------------------------------------------------------------------------ overlap mode, a replayed frame

def test_overlap_mode_reads_the_last_submitted_frames_slot(oracle_lut):
    from awsm_renderer_amd.hip_backend import HipDevice
    W, H = 70, 45
    dev, ref, model = frame("panes", W, H, oracle_lut, dev=HipDevice(parity_tap=True, overlap_frames=True))
    for _ in range(3):                                                                        # enqueue only: the queries wait for every stream
        again(dev, model, end=False)
    ans, _, _ = assert_map(dev, ref, True, 0.5, "overlap")
    got, n = dev.pick_rect(0, 0, W, H, True, 0.5)
    assert got == pr.rect(ans, ref, 0, 0, W, H) and n == 2
    y, x = _first(ans["layer"] == pr.WORLD_TRANSPARENT)
    assert dev.pick_ex(x, y, True, 0.5)["mesh_key"] == ref.key_of(pr.WORLD_TRANSPARENT, int(ans["draw"][y, x]))
    dev.frame_end()
    assert_map(dev, ref, True, 0.5, "overlap, after frame_end")
    dev.close()


def test_an_overflowed_fragment_list_is_refused_until_frame_end_has_replayed_it(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST starts with 4096 fragment slots; three panes over most of a 70 x 45 frame need more."""
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H = 70, 45
    sc = pr._scene(W, H, [pr._rect(*pr.WALL)] + [pr._rect(-3.3 + 0.1 * i, -2.1, 3.3, 2.1, 0.6 * i, 1 + i) for i in range(3)], [pr._blend(a) for a in (0.8, 0.3, 0.6)])
    model = helpers.build_model(sc)
    dev = HipDevice(parity_tap=True, small_bin_list=True)
    helpers.hip_frame(model, oracle_lut, dev=dev)                                              # uploads; a frame without a transparent pass
    again(dev, model, end=False)
    for call in (lambda: dev.read_pick_map(True), lambda: dev.pick_ex(3, 3, True), lambda: dev.pick_rect(0, 0, W, H, True)):
        with pytest.raises(AwsmHipError, match="frame_end") as e:
            call()
        assert e.value.code == NOT_READY
    dev.read_pick_map(False)                                                                  # the keys are whole: no flag, no refusal
    stats = dev.frame_end()
    assert stats["forward_fragment_slots"] > 4096 and stats["bin_overflow_retries"] >= 1, stats
    ref = pr.Reference(model, oracle_lut)
    for thr in (0.5, 0.7, 0.25):
        ans, _, _ = assert_map(dev, ref, True, thr, "replayed %g" % thr)
    assert (ans["word"] == (pr.WORLD_TRANSPARENT << 28 | 2)).sum() >= 1500                    # the nearest pane at 0.25
    dev.close()


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError, HipDevice
    W, H = 33, 17
    model = helpers.build_model(pr.SCENES["glass"](W, H))
    dev = HipDevice(parity_tap=True)
    dev.resize(W, H, 0)

    def refused(code, call):
        with pytest.raises(AwsmHipError) as e:
            call()
        assert e.value.code == code, (code, e.value)

    for call in (lambda: dev.pick_ex(1, 1), lambda: dev.pick_rect(0, 0, 4, 4), lambda: dev.read_pick_map()):
        refused(NOT_READY, call)                                                              # before a geometry pass
    dev, _ = helpers.hip_frame(model, oracle_lut, dev=dev, transparent=True)
    ref = pr.Reference(model, oracle_lut)
    nan = float("nan")
    for bad in (dict(alpha_threshold=-0.01), dict(alpha_threshold=1.01), dict(alpha_threshold=nan), dict(alpha_threshold=0.5, flags=2), dict(alpha_threshold=0.5, flags=3),
                dict(alpha_threshold=0.5, struct_size=2), dict(alpha_threshold=0.5, struct_size=5000)):
        for transparent in (False, True):
            refused(INVALID, lambda: dev.pick_ex(1, 1, transparent, **bad))
            refused(INVALID, lambda: dev.pick_rect(0, 0, 4, 4, transparent, **bad))
            refused(INVALID, lambda: dev.read_pick_map(transparent, **bad))
    n = C.c_uint32(7)
    assert dev.lib.awsm_hip_pick_rect(dev.ctx, 0, 0, 4, 4, None, None, 3, C.byref(n)) == INVALID and dev.lib.awsm_hip_pick_rect(dev.ctx, 0, 0, 4, 4, None, None, 0, None) == INVALID
    assert dev.lib.awsm_hip_pick_ex(dev.ctx, 0, 0, None, None) == INVALID
    assert dev.lib.awsm_hip_pick_rect(dev.ctx, 0, 0, W, H, None, None, 0, C.byref(n)) == 0 and n.value == 1      # a NULL query is the defaults: the wall alone
    assert_map(dev, ref, True, 0.0, "threshold 0"); assert_map(dev, ref, True, 1.0, "threshold 1")      # the ends of the range are fine
    on, _ = dev.read_pick_map(True, 0.9, struct_size=8)                                        # the threshold is not reached: it keeps its default
    assert (on == ref.answer(True, 0.5)["word"]).all()
    dev.close()
    for shard in ("rows", "bands"):
        dev = HipDevice(parity_tap=True)
        dev.resize(W, H, 0)
        if shard == "rows":
            dev.set_shard_rows(0, 9)
        else:
            dev.set_shard_bands(2, 0)
        dev.upload_mirrors(model.mirrors())
        from oracle import oracle_lib
        dev.env_upload(model.scene.skybox_rgba, model.scene.prefiltered_rgb, model.scene.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(oracle_lut))
        for i, smp in enumerate(model.scene.samplers):
            dev.sampler_set(i, smp)
        dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
        refused(UNSUPPORTED, lambda: dev.pick_ex(1, 1, True))
        refused(UNSUPPORTED, lambda: dev.read_pick_map(True))
        refused(UNSUPPORTED, lambda: dev.pick_rect(0, 0, 4, 4))
        refused(UNSUPPORTED, lambda: dev.pick_rect(0, 0, 4, 4, True))
        hits = 0
        for y in range(H):                                                                    # without the flag a shard answers as awsm_hip_pick does
            for x in range(0, W, 3):
                old, new = dev.pick(x, y), dev.pick_ex(x, y)
                assert (old is None and new is None) or (new["mesh_key"], new["triangle_index"]) == old
                hits += old is not None
        assert hits >= 10
        dev.close()


# ------------------------------------------------------------------------------------------------ the host layer

def test_host_picks_the_panes(oracle_lut):
    from awsm_renderer_amd.host import Renderer
    from oracle import oracle_lib
    W, H = 70, 45
    sc = pr.SCENES["panes"](W, H)
    ref = pr.Reference(helpers.build_model(sc), oracle_lut)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    r.render(sync=True)
    wall, back, front = r.keys.mesh_keys[:3]
    ans = ref.answer(True, 0.5)
    y, x = _first((ans["word"] == (pr.WORLD_TRANSPARENT << 28 | 0)) & ref.tr[1]["touched"])      # the back pane behind the front one
    assert r.host.pick(x, y, transparent=True) == back and r.pick(x, y, True, 0.25) == front
    off = ref.answer(False)
    assert r.host.pick(x, y) == (wall if off["layer"][y, x] == pr.WORLD else None)            # the default: today's answer
    got = r.host.pick_rect(0, 0, W, H, transparent=True, alpha_threshold=0.25)
    assert [(k, L) for k, L, _ in got] == [(wall, 0), (back, 1), (front, 1)]
    low = ref.answer(True, 0.25)
    assert [n for _, _, n in got] == [int((low["word"] == w).sum()) for w in (0, pr.WORLD_TRANSPARENT << 28 | 0, pr.WORLD_TRANSPARENT << 28 | 1)]
    assert [k for k, _, _ in r.pick_rect(0, 0, W, H)] == [wall]
    r.close()
