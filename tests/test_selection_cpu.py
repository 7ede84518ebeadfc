"""CPU tests of the editor's selection overlay: the numpy restatement against answers written out by hand, its float64 run against its
float32 run on the CPU oracle's keys, the record's layout and the library's defaults, the host layer over mock backends with and without the entry
points, and the floors that keep tests/test_selection_gpu.py from passing on an empty overlay."""
import ctypes as C
import dataclasses
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc
from oracle import oracle_lib
from tests import helpers
from tests import selection_reference as sel
from tests import ssao_reference as sr
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, log_of, mock  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(view_proj=None):
    """A camera block that holds nothing but a view_proj (column-major [col][row])."""
    b = np.zeros(128, np.float32)
    b[32:48] = np.asarray(np.eye(4) if view_proj is None else view_proj, np.float32).reshape(16)
    return b.tobytes()


def _edge(x0, y0, x1, y1, z0=0.5, z1=0.5):
    return np.array([x0, y0, z0, x1, y1, z1, 1.0, 0.0], np.float32)


# ------------------------------------------------------------------------------------------------ known answers: coverage

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_horizontal_edge_by_hand(dtype):
    """y = 10.0, x in [2.5, 20.5], half width 1 (m = 1.5): the rows of centres 9.5 and 10.5 lie 0.5 away -> min(1.5 - 0.5, 1) = 1; the rows of centres
    8.5 and 11.5 lie 1.5 away -> 0; beyond the ends the distance is to the end point: centre (1.5, 9.5) is sqrt(1 + 0.25) from (2.5, 10)."""
    rec = sel.record(box_half_width=1.0)
    d = np.ones((20, 24), np.float32)
    a = sel.edge_alpha(_edge(2.5, 10.0, 20.5, 10.0), d, 24, 20, rec, dtype)
    assert (a[9, 2:21] == 1.0).all() and (a[10, 2:21] == 1.0).all()
    assert (a[8, :] == 0.0).all() and (a[11, :] == 0.0).all()
    T = np.dtype(dtype).type
    cap = T(1.5) - np.sqrt(T(1.25))
    assert a[9, 1] == cap and a[10, 1] == cap and a[9, 21] == cap and a[10, 21] == cap and 0.38 < cap < 0.39
    assert a[9, 0] == 0.0 and a[9, 22] == 0.0                                               # sqrt(4 + 0.25) > 1.5
    assert a.dtype == T


def test_a_zero_length_edge_is_a_disc():
    rec = sel.record(box_half_width=1.0)
    a = sel.edge_alpha(_edge(5.0, 5.0, 5.0, 5.0), np.ones((10, 10), np.float32), 10, 10, rec)
    yy, xx = np.mgrid[0:10, 0:10]
    dist = np.sqrt(((xx + 0.5 - 5.0) ** 2 + (yy + 0.5 - 5.0) ** 2).astype(np.float32))
    want = np.clip(np.float32(1.5) - dist, 0, 1).astype(np.float32)
    assert (a == want).all() and a[4, 4] == np.float32(1.5) - np.sqrt(np.float32(0.5)) and (a > 0).sum() == 4     # centres at sqrt(0.5), then sqrt(2.5) > 1.5


def test_the_rectangle_gate():
    """Coverage is 0 outside [min - m, max + m]^2 whatever the rest computes, and a pixel the gate lets through lies in a tile whose cull list holds the
    edge: the tile-level cull is conservative."""
    rec = sel.record(box_half_width=1.0)
    e = _edge(3.0 + 2.0 ** -21, 4.0, 9.0, 7.0)
    a, cov, _ = sel.edge_alpha(e, np.ones((12, 16), np.float32), 16, 12, rec, parts=True)
    assert cov[4, 1] == 0.0 and cov[4, 2] > 0.0                                             # centre 1.5 < 3.0000005 - 1.5; centre 2.5 is inside
    assert (cov[:, :2] == 0).all() and (cov[:2, :] == 0).all() and (cov[9:, :] == 0).all() and (cov[:, 11:] == 0).all()
    rng = np.random.default_rng(7)
    W, Hh = 70, 45
    for _ in range(40):
        p = rng.uniform(-30, 100, 4).astype(np.float32)
        e = _edge(p[0], p[1], p[2], p[3])
        hw = float(rng.choice([0.5, 0.75, 1.75, 4.0]))
        r = sel.record(box_half_width=hw)
        _, cov, _ = sel.edge_alpha(e, np.ones((Hh, W), np.float32), W, Hh, r, parts=True)
        listed = sel.tile_list_sizes(e[None], W, Hh, r)
        yy, xx = np.nonzero(cov > 0)
        assert (listed[yy // 16, xx // 16] == 1).all()


def test_hidden_fragments_are_dimmed_and_the_epsilon_is_subtracted():
    rec = sel.record(box_half_width=1.0, hidden_alpha=0.25, depth_epsilon=0.01)
    d = np.full((20, 24), 0.5, np.float32)
    d[:, 12:] = 0.49
    a, cov, visible = sel.edge_alpha(_edge(2.5, 10.0, 20.5, 10.0, 0.505, 0.505), d, 24, 20, rec, parts=True)
    assert visible[:, :12].all() and not visible[:, 12:].any()                              # 0.505 - 0.01 <= 0.5, but > 0.49
    assert (a[9, 2:12] == 1.0).all() and (a[9, 12:21] == 0.25).all()
    A, vb = sel.box_alpha(np.stack([_edge(2.5, 10.0, 20.5, 10.0, 0.505, 0.505), _edge(0, 0, 0, 0) * 0]), d, 24, 20, rec)
    assert (A == a).all() and vb[9, 5] and not vb[9, 15]
    assert not sel.box_alpha(_edge(2.5, 10.0, 20.5, 10.0)[None], d, 24, 20, sel.record(flags=sel.OUTLINE))[0].any()


# ------------------------------------------------------------------------------------------------ known answers: ring

@pytest.mark.parametrize("R", [1, 2, 4])
def test_the_ring_of_one_pixel_is_the_integer_disc_without_its_centre(R):
    s = np.zeros((12, 12), bool)
    s[6, 5] = True
    got = sel.ring(s, R)
    yy, xx = np.mgrid[0:12, 0:12]
    want = ((xx - 5) ** 2 + (yy - 6) ** 2 <= R * R) & ~s
    assert (got == want).all() and got.sum() == {1: 4, 2: 12, 4: 48}[R]
    c = np.zeros((12, 12), bool)
    c[0, 0] = True                                                                          # at the image corner: a quarter of the disc
    got = sel.ring(c, R)
    assert (got == (((xx ** 2 + yy ** 2) <= R * R) & ~c)).all() and got.sum() == {1: 2, 2: 5, 4: 16}[R]
    assert not sel.ring(s, R, outline=False).any()


def test_selected_pixels_and_depth_from_the_keys():
    """Two draws of 2 and 3 triangles, the second selected; MSAA: s from any sample, d the least over the samples that hit."""
    def key(depth, rank):
        return (np.uint64(np.float32(depth).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - rank)
    table = (np.array([0, 2], np.int64), np.array([[7, 1], [7, 2]], np.uint32))
    chosen = sel.selected_draws(table, [(7, 2)])
    assert chosen.tolist() == [False, True] and not sel.selected_draws(table, [(2, 7), (8, 1)]).any()
    keys = np.array([[key(0.5, 1), key(0.25, 2), sel.NO_HIT, key(0.75, 4)]], np.uint64)
    s, d = sel.pixels(keys, table, chosen)
    assert s.tolist() == [[False, True, False, True]] and d.tolist() == [[0.5, 0.25, 1.0, 0.75]]
    ms = np.array([[[key(0.5, 0), key(0.25, 1), sel.NO_HIT, key(0.75, 3)], [sel.NO_HIT] * 4, [key(0.5, 0), key(0.6, 1), key(0.7, 0), key(0.4, 1)]]], np.uint64)
    s, d = sel.pixels(ms, table, chosen)
    assert s.tolist() == [[True, False, False]] and d.tolist() == [[0.25, 1.0, np.float32(0.4)]]


# ------------------------------------------------------------------------------------------------ known answers: edges

def test_the_twelve_edges_of_the_unit_box_in_order():
    assert sel.EDGE_CORNERS == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]
    # view_proj = identity: sx = (X / 2 + 1/2) W, sy = (1/2 - Y / 2) H, sz = Z; W = H = 2 -> sx = X + 1, sy = 1 - Y
    t = sel.edges([[0, 0, 0, 1, 1, 1]], _block(), 2, 2)
    assert t.shape == (1, 12, 8) and (t[0, :, 6] == 1).all() and (t[0, :, 7] == 0).all()
    for j, (k0, k1) in enumerate(sel.EDGE_CORNERS):
        for e, k in enumerate((k0, k1)):
            X, Y, Z = (k >> 0) & 1, (k >> 1) & 1, (k >> 2) & 1
            assert t[0, j, 3 * e:3 * e + 3].tolist() == [X + 1.0, 1.0 - Y, float(Z)], (j, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_near_plane_crossings_land_on_z_zero_exactly(dtype):
    """view_proj = identity, box z in [-0.25, 0.75]: the four edges in z = -0.25 are wholly behind (invalid, all zeros), the four in z = 0.75 are
    whole, and the four along z start at z = 0 exactly with t = 0.25 (x and y are constant along them)."""
    t = sel.edges([[-0.5, -0.5, -0.25, 0.5, 0.5, 0.75]], _block(), 2, 2, dtype)[0]
    behind = [j for j, (k0, k1) in enumerate(sel.EDGE_CORNERS) if not (k0 & 4) and not (k1 & 4)]
    along = [j for j, (k0, k1) in enumerate(sel.EDGE_CORNERS) if (k0 ^ k1) == 4]
    assert behind == [0, 1, 4, 5] and along == [8, 9, 10, 11]
    assert (t[behind] == 0).all()
    for j in along:
        assert t[j, 6] == 1 and t[j, 2] == 0.0 and not np.signbit(t[j, 2]) and t[j, 5] == 0.75 and t[j, 0] == t[j, 3] and t[j, 1] == t[j, 4]
    assert (t[[2, 3, 6, 7], 6] == 1).all() and (t[[2, 3, 6, 7]][:, [2, 5]] == 0.75).all()
    # an oblique crossing: x follows z; from (-1, 0, -0.5) to (1, 0, 0.5) the plane is met half way, at x = 0 -> sx = 1
    vp = np.eye(4)
    vp[0][0], vp[2][0] = 0.0, 2.0                                                           # clip x = 2 Z (column-major [col][row])
    t = sel.edges([[0, 0, -0.5, 0, 0, 0.5]], _block(vp), 2, 2, dtype)[0]
    assert t[8, 6] == 1 and t[8, 0] == 1.0 and t[8, 2] == 0.0 and t[8, 3] == 2.0 and t[8, 5] == 0.5


def test_w_at_or_under_zero_and_non_finite_coordinates_are_invalid():
    vp = np.eye(4)
    vp[3][3] = 0.0                                                                          # w = 0 everywhere
    assert (sel.edges([[0, 0, 0, 1, 1, 1]], _block(vp), 8, 8) == 0).all()
    vp = np.eye(4) * 1e38
    vp[3][3] = 1e-38
    assert (sel.edges([[1, 1, 0, 2, 2, 1]], _block(vp), 8, 8) == 0).all()                   # x / w overflows


def test_an_orthographic_camera_never_clips_by_w():
    W, Hh = 70, 45
    block = sel.camera("ortho", W, Hh)
    vp = np.frombuffer(block, np.float32, 16, 128).reshape(4, 4)
    assert vp[:, 3].tolist() == [0.0, 0.0, 0.0, 1.0]                                        # the w row
    t = sel.edges([[0.5, 0.0, 0.5, 1.3, 1.0, 1.3], [-40, -40, -40, 40, 40, 40]], block, W, Hh)
    assert (t[0, :, 6] == 1).all()
    assert 0 < t[1, :, 6].sum() <= 12 and np.isfinite(t[1]).all()                           # (a box around the camera: only the near plane clips it)


# ------------------------------------------------------------------------------------------------ float64 against float32

@functools.lru_cache(maxsize=None)
def _oracle_case(scene, cam, W, Hh):
    """The CPU oracle's keys of a scene (no GPU), the draw table, the case's selection and the camera block."""
    model = helpers.build_model(sel.SCENES[scene](W, Hh, cam))
    draws = model.collect_draws()
    orc = helpers.oracle_frame(model, oracle_lib.brdf_lut(16, 16))
    keys = np.asarray(orc.keys, np.uint64).reshape(Hh, W).copy()
    kw, boxes = sel.selection_of(model, scene)
    return keys, sel.draw_table(draws, model.mirrors()), kw, boxes, bytes(model.camera_bytes)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("cam", list(sel.CAMERAS))
def test_f64_run_agrees_with_the_f32_run_within_a_few_ulps_of_the_coordinates(cam):
    """`boxes` at 70 x 45.  The bound, with u = ulp_f32 of the largest magnitude among the edges' screen coordinates and the frame's size:
      an end point that was not clipped: a clip coordinate is four products and three sums, x / w one division, the mapping to pixels three more
        roundings — x and w together <= 16 roundings of half an ulp of the coordinate that comes out: E = 8 u, doubled for the two of them: 16 u;
      an end point moved onto the near plane is c0 + t (c1 - c0) with a w far smaller than the w0 and w1 it is formed from: the cancellation
        multiplies the relative error by |w0| / w, which has no bound in ulps of the result.  To first order that error is an error in t, which moves
        the point ALONG its edge — the distance of a pixel to the edge's line does not see it, and the moved point lies outside the frame (the near
        plane projects far outside it under these cameras).  Such end points are held by the bound on A alone;
      the distance: t = (r . e) / l2 is 3 + 3 + 1 roundings (3.5 ulps relative), q = r - t e two more on a value <= |e|, so |e| dt + 2 u <= 4 u, plus the
        end points' own 16 u moving the segment;
      A = clamp(m - dist): one more rounding.  So |A32 - A64| <= 16 u + 5 u = 21 u wherever both runs decide `visible` alike; they may decide
      differently only where z - depth_epsilon is within the same few ulps of d, and those pixels are counted and capped at 2 % of the box pixels."""
    W, Hh = 70, 45
    keys, table, kw, boxes, block = _oracle_case("boxes", cam, W, Hh)
    for R, hw in sel.PARAMS:
        rec = sel.record(outline_radius=R, box_half_width=hw)
        o32 = sel.overlay(keys, table, kw, boxes, block, W, Hh, rec, np.float32)
        o64 = sel.overlay(keys, table, kw, boxes, block, W, Hh, rec, np.float64)
        assert (o32["selected"] == o64["selected"]).all() and (o32["ring"] == o64["ring"]).all() and (o32["edges"][..., 6] == o64["edges"][..., 6]).all()
        coords = o64["edges"][..., [0, 1, 3, 4]]
        u = _ulp32(max(float(np.abs(coords).max()), W))
        diff = np.abs(o32["edges"].astype(np.float64) - o64["edges"])
        whole = [(o64["edges"][..., 2] != 0), (o64["edges"][..., 5] != 0)]                      # end point 0 / 1 was not moved onto the near plane
        e_err = max(float(diff[..., [0, 1]][whole[0]].max(initial=0.0)), float(diff[..., [3, 4]][whole[1]].max(initial=0.0)))
        same = o32["box_visible"] == o64["box_visible"]
        boxpx = (o64["box_alpha"] > 0) | (o32["box_alpha"] > 0)
        a_err = float(np.abs(o32["box_alpha"].astype(np.float64) - o64["box_alpha"])[same].max())
        print("boxes %-11s R=%d hw=%.2f: largest coordinate %.1f, u=%.3e, end points off by %.3e (%.1f u), A off by %.3e (%.1f u), %d of %d box pixels decide differently"
              % (cam, R, hw, float(np.abs(coords).max()), u, e_err, e_err / u, a_err, a_err / u, int((boxpx & ~same).sum()), int(boxpx.sum())))
        assert e_err <= 16 * u and a_err <= 21 * u
        assert (boxpx & ~same).sum() <= 0.02 * boxpx.sum()


# ------------------------------------------------------------------------------------------------ floors

CASES = sorted({k[:4] for k in sel.FLOORS})


def test_every_case_of_the_gpu_tests_has_a_floor():
    want = {(s, c, W, Hh, R, hw) for s in ("corner", "boxes") for c in sel.CAMERAS for (W, Hh) in sel.SIZES for (R, hw) in sel.PARAMS}
    assert set(sel.FLOORS) == want


@pytest.mark.parametrize("scene,cam,W,Hh", CASES)
def test_floors_are_half_of_what_the_restatement_counts_on_the_oracles_keys(scene, cam, W, Hh):
    keys, table, kw, boxes, block = _oracle_case(scene, cam, W, Hh)
    unseen = scene == "boxes" and (cam == "closeup" or (cam == "far" and (W, Hh) == (8, 5)))     # nothing selected is seen: boxes only
    for R, hw in sel.PARAMS:
        out = sel.overlay(keys, table, kw, boxes, block, W, Hh, sel.record(outline_radius=R, box_half_width=hw))
        c = sel.counts(out)
        floor = dict(zip(sel.KINDS, sel.FLOORS[(scene, cam, W, Hh, R, hw)]))
        print(scene, cam, W, Hh, R, hw, c, floor)
        for k in sel.KINDS:
            assert floor[k] == (0 if c[k] == 0 else max(1, c[k] // 2)), (k, c, floor)
        # what every case is there to show: box pixels with partial coverage, hidden or visible ones; a ring unless nothing selected is seen; at the wide
        # half width pixels of full coverage (boxes scene)
        assert floor["partial"] >= 1 and floor["visible"] + floor["hidden"] >= 1
        assert unseen or floor["ring"] >= 1
        assert (floor["ring"] == 0) == unseen or scene == "corner"
        if scene == "boxes" and hw > 1:
            assert floor["full"] >= 1
        if scene == "boxes" and cam not in ("closeup",) and (W, Hh) != (8, 5):
            assert floor["visible"] >= 1 and floor["hidden"] >= 1


def full_list_boxes():
    """The 64-box case of the GPU tests: `boxes` under `far` at 70 x 45, 64 copies of the second box — a few pixels wide, inside one tile."""
    W, Hh = 70, 45
    model = helpers.build_model(sel.SCENES["boxes"](W, Hh, "far"))
    rec = list(model.meshes.items())[4][1]
    return model, [list(rec.world_aabb.min) + list(rec.world_aabb.max)] * 64


def test_the_64_box_case_fills_one_tiles_list():
    model, boxes = full_list_boxes()
    t = sel.edges(boxes, model.camera_bytes, 70, 45)
    assert t.shape == (64, 12, 8) and (t[..., 6] == 1).all()
    sizes = sel.tile_list_sizes(t, 70, 45, sel.record())
    assert sizes.max() == 768 == sel.MAX_BOXES * 12, sizes


# ------------------------------------------------------------------------------------------------ the record and the library

def test_record_layout_is_the_headers():
    text = open(os.path.join(ROOT, "include", "awsm_hip.h")).read()
    body = re.search(r"typedef struct AwsmSelection \{(.*?)\} AwsmSelection;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t|float)\s+(\w+)(?:\[(\d)\])?;", body)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    got = [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in fields]
    assert [(n, C.sizeof(t)) for n, t in got] == [(n, C.sizeof(t)) for n, t in hip_backend.AwsmSelection._fields_]
    assert C.sizeof(hip_backend.AwsmSelection) == 56
    assert int(re.search(r"#define AWSM_SELECTION_OUTLINE (\d)u", text).group(1)) == sel.OUTLINE == hip_backend.AWSM_SELECTION_OUTLINE
    assert int(re.search(r"#define AWSM_SELECTION_BOXES (\d)u", text).group(1)) == sel.BOXES == hip_backend.AWSM_SELECTION_BOXES
    hpp = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "selection.hpp")).read()
    assert int(re.search(r"kMaxKeys = (\d+)", hpp).group(1)) == sel.MAX_KEYS and int(re.search(r"kMaxBoxes = (\d+)", hpp).group(1)) == sel.MAX_BOXES
    assert "AWSM_HIP_ABI_VERSION 2u" in text


def test_the_library_hands_out_the_defaults():
    lib = hip_backend.load_library()      # links against the HIP runtime and loads without a GPU; a library that does not load is a failure
    s = hip_backend.AwsmSelection()
    assert lib.awsm_hip_selection_defaults(C.byref(s)) == 0 and lib.awsm_hip_selection_defaults(None) == -1
    assert s.struct_size == C.sizeof(hip_backend.AwsmSelection)
    for k, v in sel.DEFAULTS.items():
        got = getattr(s, k)
        assert (list(got) == np.float32(v).tolist()) if k.endswith("_color") else (got == (v if isinstance(v, int) else float(np.float32(v)))), (k, got, v)
    assert lib.awsm_hip_set_selection(None, C.byref(s), None, 0, None, 0) == -1             # no context
    assert lib.awsm_hip_read_selection(None, None, None, None, None) == -1
    with pytest.raises(TypeError):
        s.override(outline_colour=(1, 1, 1, 1))
    assert hip_backend.selection_key_words([(7 << 32) | 5, 1]).tolist() == [[7, 5], [0, 1]] and hip_backend.selection_key_words([(7, 5)]).tolist() == [[7, 5]]


# ------------------------------------------------------------------------------------------------ the host layer

@pytest.fixture(scope="module")
def mock_selection(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_selection") / "libmock_backend_selection.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_selection.c")])
    lib = C.CDLL(out)
    lib.mock_selection_record.restype = lib.mock_selection_keys.restype = lib.mock_selection_boxes.restype = C.c_uint32
    lib.mock_log_count.restype = C.c_size_t
    lib.mock_log_count.argtypes = [C.c_void_p]
    lib.mock_log_get.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mock_log_clear.argtypes = [C.c_void_p]
    return out, lib


def _handed(lib):
    """What the mock's set_selection was last handed -> (record bytes or None for NULL, [(high, low)], boxes [n, 6])."""
    rec, keys, boxes = (C.c_uint8 * 64)(), (C.c_uint32 * 128)(), (C.c_float * 384)()
    n = lib.mock_selection_record(rec, 64)
    nk, nb = lib.mock_selection_keys(keys, 64), lib.mock_selection_boxes(boxes, 64)
    return (None if n == 0xFFFFFFFF else bytes(rec[:n])), [(keys[2 * i], keys[2 * i + 1]) for i in range(nk)], np.array(boxes[:6 * nb], np.float32).reshape(nb, 6)


def _editor_scene(W, Hh):
    """`boxes` plus a blended quad (a transparent mesh) and a HUD quad."""
    sc = sr.boxes(W, Hh)
    sc.materials.append(MaterialDesc(base_color_factor=(0.2, 0.4, 0.9, 0.5), alpha_mode="blend", metallic_factor=0.0))
    glass = dataclasses.replace(sr._quad((0.2, 0.1, 1.5), (1.0, 0.0, -0.5), (0.0, 1.2, 0.0), 0), material=len(sc.materials) - 1)
    sc.nodes.append(NodeDesc(primitives=[glass]))
    hud = dataclasses.replace(sr._quad((0.2, 0.2, 0.2), (0.3, 0.0, 0.0), (0.0, 0.3, 0.0), 0), hud=True)
    sc.nodes.append(NodeDesc(primitives=[hud]))
    return sc


def _world_aabb(r, node, prim):
    """The world AABB the host's cull step holds: the primitive's corners through the node's world matrix, f32 as the host computes it."""
    world = np.asarray(r.host.transform_world(r.keys.node_keys[node]), np.float32).reshape(4, 4)      # [col][row]
    mn, mx = prim.positions.min(axis=0), prim.positions.max(axis=0)
    pts = np.array([[(mx if k & 1 else mn)[0], (mx if k & 2 else mn)[1], (mx if k & 4 else mn)[2], 1.0] for k in range(8)], np.float32)
    out = pts @ world
    return np.concatenate([out[:, :3].min(axis=0), out[:, :3].max(axis=0)])


def test_host_hands_on_keys_and_world_aabbs(mock_selection):
    path, lib = mock_selection
    W, Hh = 64, 48
    sc = _editor_scene(W, Hh)
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    mk = r.keys.mesh_keys                      # 3 corner quads, 3 boxes, the glass, the hud quad
    assert len(mk) == 8
    hidden = r.host.mesh_insert(sc.nodes[1].primitives[0], r.keys.node_keys[1], r.keys.material_keys[1], hidden=True)
    before = lib.mock_selection_calls()
    r.set_selection([mk[3], mk[6], mk[7], hidden, mk[5]], outline_radius=3)
    assert lib.mock_selection_calls() == before + 1                                         # the backend judges the record at once
    r.render()
    rec, keys, boxes = _handed(lib)
    want_rec = hip_backend.AwsmSelection(56, 3, 3, (C.c_float * 4)(1.0, 0.6, 0.1, 1.0), (C.c_float * 4)(1.0, 0.6, 0.1, 0.9), 0.75, 0.25, 1e-5)
    assert rec == bytes(want_rec)
    assert keys == sel.key_words([mk[3], mk[6], mk[5]])                                     # the hud and the hidden mesh are left out; the transparent one is in
    want = np.stack([_world_aabb(r, 1, sc.nodes[1].primitives[0]), _world_aabb(r, 4, sc.nodes[4].primitives[0]), _world_aabb(r, 3, sc.nodes[3].primitives[0])])
    assert np.allclose(boxes, want, rtol=0, atol=1e-6), (boxes, want)
    assert np.allclose(boxes[0], [0.9 - 0.35, 0.0, 0.9 - 0.35, 0.9 + 0.35, 1.0, 0.9 + 0.35], atol=1e-6)      # the first box of `boxes`, by hand
    # the box follows its transform after update_world, with nothing more to call
    r.host.transform_set_local(r.keys.node_keys[1], (2.9, 0.5, 0.9), (0, 0, 0, 1), (0.7, 1.0, 0.7))
    r.render()
    assert np.allclose(_handed(lib)[2][0], boxes[0], atol=1e-6)                              # not before update_transforms
    r.update()
    r.render()
    assert np.allclose(_handed(lib)[2][0], boxes[0] + [2, 0, 0, 2, 0, 0], atol=1e-6)
    # a removed mesh drops out silently
    r.host.mesh_remove(mk[5])
    r.render()
    rec, keys, boxes = _handed(lib)
    assert keys == sel.key_words([mk[3], mk[6]]) and len(boxes) == 2
    # a refusal of the backend's comes back as it is and leaves the selection as it was
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.set_selection([mk[4]], outline_radius=9)
    r.render()
    assert _handed(lib)[1] == sel.key_words([mk[3], mk[6]])
    # struct_size: at least its own four bytes, at most 4096; nothing beyond it reaches the backend
    for bad in (2, 5000):
        with pytest.raises(H.HostError, match=r"\(-1\)"):
            r.host.set_selection([mk[4]], struct_size=bad)
    r.host.set_selection([mk[4]], struct_size=12, outline_radius=4, box_half_width=3.0)
    rec, keys, _ = _handed(lib)
    assert rec == bytes(hip_backend.AwsmSelection(12, 3, 4))[:12] and keys == sel.key_words([mk[4]])
    r.set_selection(on=False)
    assert _handed(lib)[0] is None
    calls = lib.mock_selection_calls()
    r.render()
    assert lib.mock_selection_calls() == calls                                              # off: nothing is handed on
    assert r.host.lib.awsm_host_set_selection(None, None, None, 0) == -1 and r.host.lib.awsm_host_selection_defaults(r.host.h, None) == -1
    r.close()


def test_host_runs_the_transparent_pass_without_draws_while_a_selection_is_set(mock_selection):
    path, lib = mock_selection
    sc = sr.boxes(64, 48)                       # no transparent mesh, no hud mesh
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    ctx = r.host.device_ctx
    lib.mock_log_clear(ctx)
    r.render()
    assert [x for x in log_of(lib, ctx) if x[0] == "transparent"] == []
    r.set_selection([r.keys.mesh_keys[3]])
    lib.mock_log_clear(ctx)
    r.render()
    assert [x[2] for x in log_of(lib, ctx) if x[0] == "transparent"] == [0]                 # called, with no draws
    r.set_selection(on=False)
    lib.mock_log_clear(ctx)
    r.render()
    assert [x for x in log_of(lib, ctx) if x[0] == "transparent"] == []
    r.close()


def test_host_over_a_backend_without_selection_reports_unsupported_and_names_the_symbol(mock):  # noqa: F811
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    s = hip_backend.AwsmSelection(56, 3, 2)
    keys = (C.c_uint64 * 1)(r.keys.mesh_keys[0])
    assert r.host.lib.awsm_host_set_selection(r.host.h, C.byref(s), keys, 1) == -6          # AWSM_ERR_UNSUPPORTED
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_set_selection"):
        r.host.set_selection(on=False)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_selection_defaults"):
        r.host.set_selection([r.keys.mesh_keys[0]])
    r.render()                                                                              # and renders as before
    r.close()
