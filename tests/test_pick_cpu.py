"""CPU tests of picking through the transparent passes: the numpy restatement (tests/pick_reference.py) on every scene of the GPU
tests with floors on how many pixels each layer wins, the shares the GPU tests leave out, the records' layout and the library's defaults, and the host
layer over mock backends with and without the entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from tests import helpers
from tests import pick_reference as pr
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, log_of, mock  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (scene, W, H, threshold) -> the least number of pixels layers 0..3 win under the flag: half of what the restatement counts on the oracle
FLOORS = {
    ("glass", 8, 5, 0.5): (1, 7, 0, 0), ("glass", 8, 5, 0.7): (4, 0, 0, 0), ("glass", 33, 17, 0.5): (30, 67, 0, 0), ("glass", 33, 17, 0.7): (66, 0, 0, 0),
    ("glass", 70, 45, 0.5): (208, 480, 0, 0), ("glass", 70, 45, 0.7): (448, 0, 0, 0),
    ("panes", 8, 5, 0.5): (0, 7, 0, 0), ("panes", 33, 17, 0.5): (26, 56, 0, 0), ("panes", 70, 45, 0.5): (137, 437, 0, 0),
    ("textured", 8, 5, 0.5): (1, 7, 0, 0), ("textured", 33, 17, 0.5): (30, 79, 0, 0), ("textured", 70, 45, 0.5): (233, 524, 0, 0),
    ("mask", 8, 5, 0.5): (1, 7, 0, 0), ("mask", 33, 17, 0.5): (30, 79, 0, 0), ("mask", 70, 45, 0.5): (233, 524, 0, 0),
    ("instanced", 8, 5, 0.5): (2, 4, 0, 0), ("instanced", 33, 17, 0.5): (35, 52, 0, 0), ("instanced", 70, 45, 0.5): (211, 392, 0, 0),
    ("hud", 8, 5, 0.5): (2, 5, 1, 2), ("hud", 33, 17, 0.5): (35, 45, 32, 25), ("hud", 70, 45, 0.5): (260, 300, 169, 133),
    ("hud", 8, 5, 0.7): (4, 0, 1, 2), ("hud", 33, 17, 0.7): (59, 0, 32, 25), ("hud", 70, 45, 0.7): (410, 0, 169, 133),
}


def reference(name, W, Hh, lut, **kw):
    model = helpers.build_model(pr.SCENES[name](W, Hh))
    return pr.Reference(model, lut, hud=name == "hud", **kw)


def assert_floor(ref, ans, case):
    wins = ref.wins(ans)
    print(case, wins, "floor", FLOORS[case])
    assert all(w >= f for w, f in zip(wins, FLOORS[case])), (case, wins, FLOORS[case])


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize("case", sorted(FLOORS))
def test_every_layer_wins_its_floor(case, oracle_lut):
    name, W, Hh, thr = case
    ref = reference(name, W, Hh, oracle_lut)
    ans = ref.answer(True, thr)
    assert_floor(ref, ans, case)
    off = ref.answer(False)
    assert not ((off["layer"] == pr.WORLD_TRANSPARENT) | (off["layer"] == pr.HUD_TRANSPARENT)).any()      # flag off: the keys alone
    assert ((ans["word"] == pr.MISS) == (ans["layer"] < 0)).all() and ((ans["word"][ans["layer"] >= 0] >> 28) == ans["layer"][ans["layer"] >= 0]).all()


def test_a_fragment_at_0_6_is_picked_at_0_5_and_seen_through_at_0_7(oracle_lut):
    ref = reference("glass", 33, 17, oracle_lut)
    lo, hi, off = ref.answer(True, 0.5), ref.answer(True, 0.7), ref.answer(False)
    pane = ref.tr[0]["touched"]
    assert pane.sum() >= 100 and (lo["layer"][pane] == pr.WORLD_TRANSPARENT).all()
    assert (hi["word"] == off["word"]).all() and (hi["triangle"] == off["triangle"]).all()      # what is behind: the wall or nothing
    assert (off["layer"][pane] == pr.WORLD).sum() >= 30 and (off["layer"][pane] < 0).sum() >= 30      # over opaque geometry and over background
    assert np.allclose(lo["alpha"][pane], 0.6, atol=2.0 ** -11) and (lo["alpha"][~pane] == 1.0).all()


def test_the_back_pane_is_picked_through_the_front_one_unless_it_was_submitted_behind_it(oracle_lut):
    model = helpers.build_model(pr.SCENES["panes"](70, 45))
    model.collect_draws()
    back, front = model.collect_transparent_draws()                  # back to front: the 0.8 pane first
    ref = pr.Reference(model, oracle_lut)
    ans = ref.answer(True, 0.5)
    both = ref.tr[0]["touched"] & ref.tr[1]["touched"]
    assert both.sum() >= 300 and (ans["word"][both] == (pr.WORLD_TRANSPARENT << 28 | 0)).all()      # the back pane, through the 0.3 one
    assert (ans["layer"][ref.tr[1]["touched"] & ~ref.tr[0]["touched"]] != pr.WORLD_TRANSPARENT).all()      # the front pane alone: seen through
    swapped = pr.Reference(model, oracle_lut, transparent=[front, back])
    ans = swapped.answer(True, 0.5)
    off = swapped.answer(False)
    assert (ans["word"][both] == off["word"][both]).all()                                       # the far pane is absent behind the near one's depth
    only_back = swapped.tr[1]["touched"] & ~swapped.tr[0]["touched"]
    assert only_back.sum() >= 100 and (ans["word"][only_back] == (pr.WORLD_TRANSPARENT << 28 | 1)).all()


def test_the_mesh_behind_the_wall_is_never_picked_and_instances_keep_their_own_draw(oracle_lut):
    ref = reference("instanced", 70, 45, oracle_lut)
    keys = [ref.key_of(pr.WORLD_TRANSPARENT, i) for i in range(len(ref.tr_draws))]
    assert len(keys) == 4 and len(set(keys)) == 2
    hidden = [i for i in range(4) if keys.count(keys[i]) == 1][0]
    assert not ref.tr[hidden]["touched"].any()
    for thr in (0.0, 0.5):
        ans = ref.answer(True, thr)
        won = [int((ans["word"] == (pr.WORLD_TRANSPARENT << 28 | i)).sum()) for i in range(4)]
        assert won[hidden] == 0 and all(w >= 100 for i, w in enumerate(won) if i != hidden), won
    entries = pr.rect(ans, ref, 0, 0, 70, 45)
    assert [e[0] for e in entries] == [pr.WORLD, pr.WORLD_TRANSPARENT] and entries[1][2] == sum(won)      # three instances, one mesh key, one entry


def _texture_case(lut, mode):
    W, Hh = 70, 45
    sc = pr.SCENES["textured" if mode == "blend" else "mask"](W, Hh)
    model = helpers.build_model(sc)
    ref = pr.Reference(model, lut)
    prim = sc.nodes[1].primitives[0]
    uv = pr.uv_of(ref.tr[0]["fit"], prim.uvs[0][prim.indices])
    inside = ref.tr[0]["fit"]["margin"] >= 0
    return ref, uv, inside, pr.border_band(uv, pr.BLOCKS, inside)


@pytest.mark.parametrize("mode", ["blend", "mask"])
def test_texture_alpha_decides_per_block_and_a_quarter_at_most_is_left_out(mode, oracle_lut):
    ref, uv, inside, band = _texture_case(oracle_lut, mode)
    share = band.sum() / inside.sum()
    print("border band:", int(band.sum()), "of", int(inside.sum()), "quad pixels", share)
    assert inside.sum() >= 1500 and share <= 0.25
    ans = ref.answer(True, 0.5)
    cell = np.floor(uv * pr.BLOCKS).astype(int)
    opaque_block = ((cell[..., 0] + cell[..., 1]) & 1) == 1
    keep = inside & ~band
    assert (ans["layer"][keep & opaque_block] == pr.WORLD_TRANSPARENT).all() and (ans["layer"][keep & ~opaque_block] != pr.WORLD_TRANSPARENT).all()
    assert (keep & opaque_block).sum() >= 400 and (keep & ~opaque_block).sum() >= 400
    if mode == "mask":      # a fragment that survived its cutoff was drawn with alpha 1; one that did not is not in the coverage at all
        assert (ans["alpha"][keep & opaque_block] == 1.0).all() and not ref.tr[0]["touched"][keep & ~opaque_block].any()


def test_msaa_comparison_leaves_out_at_most_three_tenths(oracle_lut):
    for name in ("glass", "hud"):
        ref = reference(name, 70, 45, oracle_lut)
        band = msaa_band(ref)
        print(name, "msaa band", int(band.sum()), band.mean())
        assert band.mean() <= 0.30


def msaa_band(ref):
    """The pixels an MSAA x 4 frame is not compared at: those not one pixel inside or outside every layer's single-sampled coverage."""
    masks = [d["touched"] for d in ref.tr + ref.htr] + [np.asarray(ref.world_keys) != pr.NO_HIT]
    if ref.hud_keys is not None:
        masks.append(np.asarray(ref.hud_keys) != pr.NO_HIT)
    # the world layer's coverage per draw, so that an edge between two opaque meshes counts too
    hit, draw, _, _ = ref._from_keys(ref.world_keys, ref.world_table)
    masks += [hit & (draw == i) for i in range(len(ref.world_draws))]
    return pr.erode_dilate_band(masks)


def test_rect_by_hand():
    class Two:
        W, H = 4, 3

        def draws_of(self, layer):
            return [{"mesh_key": (5, 1)}, {"mesh_key": (6, 1)}, {"mesh_key": (5, 1)}] if layer == 0 else [{"mesh_key": (5, 1)}] if layer == 1 else []
    layer = np.array([[0, 0, 1, -1], [0, 0, 1, -1], [0, 0, 0, -1]])
    draw = np.array([[2, 1, 0, 0], [2, 1, 0, 0], [0, 0, 1, 0]])
    ans = dict(layer=layer, draw=draw)
    k5, k6 = (1 << 32) | 5, (1 << 32) | 6
    assert pr.rect(ans, Two(), 0, 0, 4, 3) == [(0, k5, 4), (0, k6, 3), (1, k5, 2)]      # draws 0 and 2 share a key: merged into the first
    assert pr.rect(ans, Two(), -5, -5, 2, 2) == [(0, k5, 2), (0, k6, 2)]
    assert pr.rect(ans, Two(), 3, 0, 9, 9) == [] and pr.rect(ans, Two(), 2, 2, 2, 3) == [] and pr.rect(ans, Two(), 1, 1, 2, 2) == [(0, k6, 1)]


# ------------------------------------------------------------------------------------------------ the records and the library

def test_record_layouts_are_the_headers():
    text = open(os.path.join(ROOT, "include", "awsm_hip.h")).read()
    for name, cls in (("AwsmPickQuery", hip_backend.AwsmPickQuery), ("AwsmPickHit", hip_backend.AwsmPickHit), ("AwsmPickRectEntry", hip_backend.AwsmPickRectEntry)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
        assert fields == [f for f, _ in cls._fields_], name
    assert C.sizeof(hip_backend.AwsmPickQuery) == 12 and C.sizeof(hip_backend.AwsmPickHit) == 28 and C.sizeof(hip_backend.AwsmPickRectEntry) == 16
    assert re.search(r"#define AWSM_PICK_TRANSPARENT 1u", text) and hip_backend.AWSM_PICK_TRANSPARENT == 1
    assert re.search(r"#define AWSM_HIP_ABI_VERSION 2u", text)


def test_the_library_hands_out_the_defaults_and_refuses_null():
    lib = hip_backend.load_library()
    q = hip_backend.AwsmPickQuery()
    assert lib.awsm_hip_pick_query_defaults(C.byref(q)) == 0
    assert (q.struct_size, q.flags, q.alpha_threshold) == (12, 0, 0.5)
    assert lib.awsm_hip_pick_query_defaults(None) == -1
    hit, n = hip_backend.AwsmPickHit(), C.c_uint32()
    assert lib.awsm_hip_pick_ex(None, 0, 0, None, C.byref(hit)) == -1 and lib.awsm_hip_pick_rect(None, 0, 0, 1, 1, None, None, 0, C.byref(n)) == -1
    assert lib.awsm_hip_read_pick_map(None, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ the host layer

@pytest.fixture(scope="module")
def mock_pick(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_pick") / "libmock_backend_pick.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_pick.c")])
    lib = C.CDLL(out)
    lib.mock_log_count.restype = C.c_size_t
    lib.mock_log_count.argtypes = [C.c_void_p]
    lib.mock_log_get.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mock_log_clear.argtypes = [C.c_void_p]
    return out, lib


def _last(lib):
    flags, thr, size, args = C.c_uint32(), C.c_float(), C.c_uint32(), (C.c_int32 * 4)()
    lib.mock_pick_last(C.byref(flags), C.byref(thr), C.byref(size), args)
    return flags.value, thr.value, size.value, list(args)


def test_host_hands_the_query_on_and_checks_its_arguments(mock_pick):
    path, lib = mock_pick
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    r.render()
    ctx = r.host.device_ctx
    lib.mock_log_clear(ctx)
    before = lib.mock_pick_calls()
    assert r.host.pick(3, 4) is None                                                        # the default: awsm_hip_pick, as ever
    assert [x for x in log_of(lib, ctx) if x[0] == "pick"] == [("pick", 0, 3, 4)] and lib.mock_pick_calls() == before
    assert r.host.pick(3, 4, transparent=True) == (7 << 32) | 10 and r.pick(5, 6, True, 0.25) == (7 << 32) | 10
    assert _last(lib)[:3] == (1, 0.25, 12) and _last(lib)[3][:2] == [5, 6]
    assert r.host.pick(0, 4, transparent=True) is None                                      # the mock's miss
    hit, key, layer = C.c_uint32(9), C.c_uint64(9), C.c_uint32(9)
    L = r.host.lib
    assert L.awsm_host_pick_ex(r.host.h, 2, 2, 0, 0.5, C.byref(hit), C.byref(key), C.byref(layer)) == 0
    assert (hit.value, key.value, layer.value) == (1, (7 << 32) | 9, 0) and _last(lib)[0] == 0
    for bad in (-0.1, 1.5, float("nan")):
        calls = lib.mock_pick_calls()
        with pytest.raises(H.HostError, match=r"\(-1\).*alpha_threshold"):
            r.host.pick(1, 1, transparent=True, alpha_threshold=bad)
        with pytest.raises(H.HostError, match=r"\(-1\).*alpha_threshold"):
            r.host.pick_rect(0, 0, 4, 4, alpha_threshold=bad)
        assert lib.mock_pick_calls() == calls                                               # refused before the backend sees it
    with pytest.raises(H.HostError, match=r"\(-5\)"):                                       # a refusal of the backend's comes back as it is
        r.host.pick(-1, 1, transparent=True)
    assert L.awsm_host_pick_ex(r.host.h, 1, 1, 1, 0.5, None, C.byref(key), None) == -1 and L.awsm_host_pick_ex(None, 1, 1, 1, 0.5, C.byref(hit), C.byref(key), None) == -1
    # the rectangle
    assert r.host.pick_rect(-3, 2, 70, 9, transparent=True, alpha_threshold=1.0) == [((100 << 32) | 200, 0, 10), ((101 << 32) | 201, 1, 20), ((102 << 32) | 202, 0, 30)]
    assert _last(lib) == (1, 1.0, 12, [-3, 2, 70, 9])
    assert r.pick_rect(0, 0, 1, 1) == r.host.pick_rect(0, 0, 1, 1) and _last(lib)[0] == 0
    lib.mock_pick_set_entries(5)
    assert len(r.host.pick_rect(0, 0, 8, 8, cap=2)) == 5                                    # asked again with room for all
    keys, n = (C.c_uint64 * 2)(), C.c_uint32()
    assert L.awsm_host_pick_rect(r.host.h, 0, 0, 8, 8, 0, 0.5, keys, None, None, 2, C.byref(n)) == 0 and n.value == 5 and list(keys) == [(100 << 32) | 200, (101 << 32) | 201]
    assert L.awsm_host_pick_rect(r.host.h, 0, 0, 8, 8, 0, 0.5, None, None, None, 0, C.byref(n)) == 0 and n.value == 5
    assert L.awsm_host_pick_rect(r.host.h, 0, 0, 8, 8, 0, 0.5, None, None, None, 2, C.byref(n)) == -1
    assert L.awsm_host_pick_rect(r.host.h, 0, 0, 8, 8, 0, 0.5, keys, None, None, 2, None) == -1
    lib.mock_pick_set_entries(3)
    r.close()


def test_host_over_a_backend_without_the_entries_reports_unsupported_and_names_the_symbol(mock):  # noqa: F811
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    r.render()
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_pick_ex"):
        r.host.pick(1, 1, transparent=True)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_pick_rect"):
        r.host.pick_rect(0, 0, 4, 4)
    assert r.host.pick(1, 1) is None                                                        # and picks as before
    r.close()
