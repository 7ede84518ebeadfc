"""CPU tests of the shadows from several views: the numpy restatement against §19's with one view, a cascade pair and a point
light's cube against known answers on the CPU oracle's keys, the records' layout and the constants, and the conditions that keep
tests/test_shadow_views_gpu.py informative."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from tests import shadow_reference as shr
from tests import shadow_views_reference as svr
from tests import ssao_reference as sr
from tests.test_shadow_cpu import _scene      # the CPU oracle's keys of a scene, computed once for both modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SIZES = (40, 96)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _layer(scene, block, S):
    """The oracle's raster of a scene's opaque draws from one light block."""
    return shr.caster_map(_scene(scene, "perspective", 33, 17)[2], block, S)


def _views(scene, cam, W, Hh, blocks, S, params, dtype=np.float32):
    keys, block, _ = _scene(scene, cam, W, Hh)
    return svr.shadow_views(keys, block, W, Hh, [_layer(scene, b, S) for b in blocks], list(blocks), S, params, dtype)


# ------------------------------------------------------------------------------------------------ 1. one view is §19

@pytest.mark.parametrize("scene", ["boxes", "corner"])
@pytest.mark.parametrize("W,Hh", sr.SIZES)
def test_one_view_is_the_single_map_restatement_bit_for_bit(W, Hh, scene):
    """V, m and every intermediate; u, v, z and the slopes where the pixel is inside (outside, §19 carries values nothing reads and this one zeros).
    Two identical views: the same, and view 0 wherever the pixel is inside."""
    keys, block, _ = _scene(scene, "perspective", W, Hh)
    inside_px = 0
    for light in ("sun", "spot"):
        for S in MAP_SIZES:
            lb = shr.light_block(light, S)
            layer = _layer(scene, lb, S)
            for R in (0, 1, 2):
                p = {"pcf_radius": R, "light": shr.light_vec(light)}
                want = shr.shadow(keys, block, W, Hh, layer, lb, S, p)
                for K in (1, 2):
                    got = svr.shadow_views(keys, block, W, Hh, [layer] * K, [lb] * K, S, p)
                    ins = want["inside"]
                    for name in ("hit", "inside", "has_normal", "V", "m", "g", "cos"):
                        assert np.array_equal(_bits(got[name]), _bits(want[name])), (light, S, R, K, name)
                    for name in ("Pw", "normal"):
                        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got[name], want[name])), (light, S, R, K, name)
                    for name in ("u", "v", "z", "zu", "zv"):
                        assert np.array_equal(_bits(got[name])[ins], _bits(want[name])[ins]), (light, S, R, K, name)
                    assert (got["view"][ins] == 0).all() and (got["view"][~ins] == svr.NO_VIEW).all()
                inside_px += int(ins.sum())
    assert inside_px >= 12 * 0.5 * W * Hh


# ------------------------------------------------------------------------------------------------ 2. the cascade known answer

@pytest.mark.parametrize("S", MAP_SIZES)
@pytest.mark.parametrize("R", [0, 1, 2])
def test_a_cascade_pair_shadows_the_floor_under_the_quad_from_the_view_it_lies_in(R, S):
    """floating_quad under `zenith` in two views, tightest first: a window of half height 1.75 centred on the quad, then the whole block.  Every floor
    pixel: V == 0 under the quad by more than R + 1 texels of ITS view, V == 1 outside it by more than that, with §19's exemption (and its bound on
    V) for the pixels beside a non-floor neighbour.  The view layer is 0 exactly where the floor point's f64 (u_0, v_0) lies in [M, S - M)^2, pixels
    within 1e-3 texel of that border left out; no hit pixel is without a view."""
    W, Hh = 70, 45
    blocks = svr.cascade_pair(S)
    p = {"pcf_radius": R, "light": shr.light_vec("zenith")}
    out = _views("floating_quad", "perspective", W, Hh, blocks, S, p)
    ref = _views("floating_quad", "perspective", W, Hh, blocks, S, p, np.float64)
    x, y, z = out["Pw"]
    floor = out["hit"] & (np.abs(y) < 1e-3)
    interior = sr._shift(floor, 0, 1) & sr._shift(floor, 0, -1) & sr._shift(floor, 1, 0) & sr._shift(floor, -1, 0)
    view = out["view"]
    assert not (out["hit"] & (view == svr.NO_VIEW)).any()
    half = np.where(view == 0, 1.75, shr.LIGHTS["zenith"]["ortho_half_height"])
    t = (R + 1) * 2.0 * half / S
    (xa, xb), (za, zb) = shr.QUAD["x"], shr.QUAD["z"]
    under = floor & (x > xa + t) & (x < xb - t) & (z > za + t) & (z < zb - t)
    outside = floor & ((x < xa - t) | (x > xb + t) | (z < za - t) | (z > zb + t))
    V = out["V"]
    print("S = %d R = %d: %d floor pixels under, %d outside; %d in view 0, %d in view 1" % (S, R, under.sum(), outside.sum(), (floor & (view == 0)).sum(), (floor & (view == 1)).sum()))
    assert under.sum() >= 4 and outside.sum() >= 100 and (outside & (view == 0)).sum() >= 5 and (outside & (view == 1)).sum() >= 5      # both views are exercised
    assert (V[under] == 0.0).all(), int((V[under] != 0).sum())
    assert (V[outside & interior] == 1.0).all(), int((V[outside & interior] != 1).sum())
    beside = outside & ~interior
    assert beside.sum() < 2 * (W + Hh) and (V[beside] >= np.float32((R + 1) ** 2) / np.float32((2 * R + 1) ** 2)).all()
    # the view layer against f64: view 0's own coordinates of the floor point
    lvp = shr._mat(blocks[0], 128, np.float64)
    Pw = ref["Pw"]
    q = [shr._row(lvp, r, Pw[0], Pw[1], Pw[2]) for r in range(4)]
    u0, v0 = (q[0] / q[3] * 0.5 + 0.5) * S, (0.5 - q[1] / q[3] * 0.5) * S
    M = R + 1.0
    edge = np.minimum.reduce([np.abs(u0 - M), np.abs(u0 - (S - M)), np.abs(v0 - M), np.abs(v0 - (S - M))])
    sure = floor & (edge > 1e-3)
    deep0 = (u0 >= M) & (u0 < S - M) & (v0 >= M) & (v0 < S - M)
    print("  %d floor pixels within 1e-3 texel of view 0's border left out" % int((floor & ~sure).sum()))
    assert ((view == 0) == deep0)[sure].all(), int(((view == 0) != deep0)[sure].sum())


# ------------------------------------------------------------------------------------------------ 3. a point light's cube

def _segment_hits_box(P, L, lo, hi):
    """Slab test in f64: does the segment P -> L (arrays [..., 3] and [3]) meet the box [lo, hi]?"""
    d = L - P
    with np.errstate(all="ignore"):
        t0, t1 = (lo - P) / d, (hi - P) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    par = d == 0.0
    inside_slab = (P >= lo) & (P <= hi)
    near = np.where(par, np.where(inside_slab, -np.inf, np.inf), near)
    far = np.where(par, np.where(inside_slab, np.inf, -np.inf), far)
    return np.maximum(near.max(axis=-1), 0.0) <= np.minimum(far.min(axis=-1), 1.0)


def _point_run(position, W, Hh, S=96, R=0):
    sc = sr.boxes(W, Hh)
    aabbs = shr.scene_aabbs(sc)
    corners = [np.array([(b if (k >> i) & 1 else a)[i] for i in range(3)]) for a, b in [(np.min([a for a, _ in aabbs], axis=0), np.max([b for _, b in aabbs], axis=0))] for k in range(8)]
    far = max(np.linalg.norm(c - np.asarray(position)) for c in corners)
    blocks = tuple(svr.cube_face_blocks(position, S, R, near=max(0.05, far * 1e-3), far=far))
    out = _views("boxes", "perspective", W, Hh, blocks, S, {"pcf_radius": R, "light": svr.point_light(position)})
    return out, aabbs[3:]


@pytest.mark.parametrize("W,Hh", sr.SIZES[1:])
def test_a_point_lights_faces_are_chosen_by_the_major_axis_and_its_boxes_cast(W, Hh):
    """`boxes` under a point light high in the room and one low in the corner (svr.POINT_POSITIONS), S = 96, R = 0.  The view of a pixel is the face
    of the largest component of Pw - position (where it leads by more than 1e-3 relative); over the two lights every face is taken by at least 5
    pixels.  A hit, facing pixel whose segment to the light crosses one of the three boxes shrunk by two texels of its face is dark, one whose segment
    clears the boxes grown by as much is lit — pixels with a non-coplanar image neighbour exempt, as in §19.  Over the two lights at least half of
    the hit, facing pixels are classified, at least 5 % in each class.

    Measured, 33 x 17 / 70 x 45: high light dark 0.2 / 0.9 %, lit 78.1 / 79.3 %; low light dark 13.9 / 18.5 %, lit 44.3 / 59.1 %;
    faces of the two lights together [388, 14, 84, 221, 399, 16] / [1936, 97, 602, 1555, 2006, 104].

    What this test found: with a receiver plane fitted only when both neighbours are inside the pixel's own view, 4 wall pixels of
    the low light at 70 x 45 that geometry calls lit had V = 0 — each within 7 texels of its face's border, its image neighbour three texels
    further, past the face's one-texel apron, so the plane was flat and the texel's own depth nearer than z - bias.  Step 6' therefore lets a
    neighbour serve that another view holds; with it no pixel is wrong here, nor at the six worst of the other positions tried."""
    S = 96
    faces = np.zeros(6, np.int64)
    n_facing = n_dark = n_lit = 0
    wrong = []
    for position in svr.POINT_POSITIONS:
        out, boxes = _point_run(position, W, Hh, S)
        hit, view, V = out["hit"], out["view"], out["V"]
        P = np.stack([np.asarray(c, np.float64) for c in out["Pw"]], axis=-1)
        L = np.asarray(position, np.float64)
        d = P - L
        order = np.sort(np.abs(d), axis=-1)
        clear_axis = hit & (order[..., 2] > order[..., 1] * (1.0 + 1e-3))
        axis = np.argmax(np.abs(d), axis=-1)
        major = 2 * axis + (np.take_along_axis(d, axis[..., None], axis=-1)[..., 0] < 0)
        assert clear_axis.sum() >= 0.8 * hit.sum()
        assert (view[clear_axis] == major[clear_axis]).all(), int((view[clear_axis] != major[clear_axis]).sum())
        faces += np.bincount(view[hit], minlength=256)[:6]
        # dark and lit, from geometry alone
        n = np.stack([np.asarray(c, np.float64) for c in out["normal"]], axis=-1)
        flat = out["has_normal"].copy()
        for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            Pq = np.stack([sr._shift(P[..., i], dy, dx) for i in range(3)], axis=-1)
            flat &= sr._shift(hit, dy, dx) & (np.abs(((Pq - P) * n).sum(axis=-1)) < 1e-3)
        facing = hit & (out["g"] > 0.0)
        texel = 2.0 * order[..., 2] * svr.face_tan(S, 0) / S      # a texel of the face at the receiver's depth along the face's axis: no smaller than at a box nearer the light
        margin = (2.0 * texel)[..., None]
        crosses = np.zeros(hit.shape, bool)
        clears = np.ones(hit.shape, bool)
        for lo, hi in boxes:
            crosses |= _segment_hits_box(P, L, lo + margin, hi - margin)
            clears &= ~_segment_hits_box(P, L, lo - margin, hi + margin)
        sel = facing & flat & (view != svr.NO_VIEW)
        dark, lit = sel & crosses, sel & clears
        print("%s %dx%d: %d hit, %d facing, %d of them flat; dark %.3f, lit %.3f of the facing; dark with V != 0: %d, lit with V != 1: %d; faces so far %s" % (
            position, W, Hh, hit.sum(), facing.sum(), sel.sum(), dark.sum() / facing.sum(), lit.sum() / facing.sum(), (V[dark] != 0).sum(), (V[lit] != 1).sum(), faces.tolist()))
        n_facing += int(facing.sum()); n_dark += int(dark.sum()); n_lit += int(lit.sum())
        wrong.append((position, int((V[dark] != 0.0).sum()), int((V[lit] != 1.0).sum())))
    assert (faces >= 5).all(), faces.tolist()
    assert n_dark + n_lit >= 0.5 * n_facing and n_dark >= 0.05 * n_facing and n_lit >= 0.05 * n_facing, (n_dark, n_lit, n_facing)
    assert all(nd == 0 and nl == 0 for _, nd, nl in wrong), wrong


# ------------------------------------------------------------------------------------------------ records, constants, the library

def test_constants_and_records_are_the_headers():
    text = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "shadow.hpp")).read()
    assert int(re.search(r"kMaxViews = (\d+)", text).group(1)) == svr.MAX_VIEWS == hip_backend.AWSM_SHADOW_MAX_VIEWS
    assert int(re.search(r"kNoView = (\d+)u", text).group(1)) == svr.NO_VIEW == hip_backend.SHADOW_NO_VIEW
    header = open(os.path.join(ROOT, "include", "awsm_hip.h")).read()
    assert int(re.search(r"#define AWSM_SHADOW_MAX_VIEWS (\d+)", header).group(1)) == svr.MAX_VIEWS
    body = re.search(r"typedef struct AwsmShadowView \{(.*?)\} AwsmShadowView;", header, re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in hip_backend.AwsmShadowView._fields_]
    assert C.sizeof(hip_backend.AwsmShadowView) == 32 and hip_backend.AwsmShadowView.casters.offset == 16 and hip_backend.AwsmShadowView.n_casters.offset == 24
    assert C.sizeof(hip_backend.AwsmShadow) == 48


def test_the_library_exports_the_entries_and_refuses_null():
    lib = hip_backend.load_library()      # links against the HIP runtime and loads without a GPU
    s = hip_backend.AwsmShadow()
    assert lib.awsm_hip_shadow_defaults(C.byref(s)) == 0
    assert lib.awsm_hip_shadow_pass_views(None, C.byref(s), None, 0) == -1
    assert lib.awsm_hip_read_shadow_map_view(None, 0, None) == -1 and lib.awsm_hip_read_shadow_view(None, None) == -1
    for name in ("awsm_hip_shadow_pass_views", "awsm_hip_read_shadow_map_view", "awsm_hip_read_shadow_view"):
        assert name in hip_backend.EXPORTS


# ------------------------------------------------------------------------------------------------ 4. the host's rules against f64

import subprocess      # noqa: E402

from awsm_renderer_amd import host as H      # noqa: E402
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, mock  # noqa: E402, F401  (the module-scoped fixture)


@pytest.fixture(scope="module")
def mock_views(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_views") / "libmock_backend_shadow_views.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_shadow_views.c")])
    lib = C.CDLL(out)
    for f in (lib.mock_views_count, lib.mock_views_view, lib.mock_shadow_last):
        f.restype = C.c_uint32
    lib.mock_views_at.restype = C.c_size_t
    return out, lib


def _sent(lib):
    """What the mock's views entry was last handed -> (record, [(block, [caster bytes])])."""
    rec = hip_backend.AwsmShadow()
    n = lib.mock_views_count(C.byref(rec))
    out = []
    for i in range(n):
        block, draws = (C.c_uint8 * 512)(), (hip_backend.AwsmDraw * 256)()
        k = lib.mock_views_view(i, block, draws, 256)
        out.append((bytes(block), [bytes(draws[j]) for j in range(k)]))
    return rec, out


# (components exactly representable in f32: the host reads the light as f32, the restatement as given)
POINT = {"kind": "point", "color": (1.0, 1.0, 1.0), "intensity": 5.0, "position": (0.625, 2.375, 0.625), "range": 0.0}
POINT_RANGED = dict(POINT, position=(0.4375, 0.5, 0.4375), range=7.5)
SUNS = {"oblique": {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 1.0, "direction": (0.125, -0.375, -1.0)},
        "rolled": {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 1.0, "direction": (-0.625, -0.40625, 0.3125)},
        "down": {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 1.0, "direction": (0.0, -1.0, 0.0)}}
# The worst distance measured between the host's f32 blocks and the f64 restatement, per matrix and relative to the matrix's largest entry, over the six
# faces of the two point lights and N = 2, 3, 4 cascades of the three suns under the `perspective`, `ortho` and `far` cameras (the test prints them;
# DESIGN.md §22): the f32 rounding of the entries and one f32 matrix product, as in §19.  The tolerance is 4 x that.
VIEWS_MEASURED = {"view": 3.5e-8, "proj": 4.6e-8, "view_proj": 7.6e-8}
VIEWS_TOLERANCE = {k: 4 * v for k, v in VIEWS_MEASURED.items()}


def _distances(block, want, worst, what):
    for k, byte in (("view", 0), ("proj", 64), ("view_proj", 128)):
        got = np.frombuffer(block, np.float32, 16, byte).reshape(4, 4).astype(np.float64)
        dist = np.abs(got - want[k]).max() / np.abs(want[k]).max()
        worst[k] = max(worst[k], dist)
        assert dist <= VIEWS_TOLERANCE[k], (what, k, dist)


@pytest.mark.parametrize("cam", ["perspective", "ortho", "far"])
def test_host_faces_and_cascades_are_the_f64_restatement(mock_views, cam):
    path, lib = mock_views
    S, R = 96, 1
    sc = sr.boxes(64, 48, cam)
    sc.lights = [POINT, POINT_RANGED] + list(SUNS.values())
    aabbs = shr.scene_aabbs(sc)
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    worst = {k: 0.0 for k in VIEWS_TOLERANCE}
    for i, light in enumerate((POINT, POINT_RANGED)):
        r.set_shadow(i, map_size=S, pcf_radius=R)
        r.render()
        rec, sent = _sent(lib)
        want = svr.host_cube_faces(light, aabbs, S, R)
        assert tuple(rec.light) == tuple(float(np.float32(c)) for c in light["position"]) + (1.0,)
        keep = [k for k in range(6) if shr.host_casters(want[k]["view_proj"], aabbs)]
        assert len(sent) == len(keep)                                                        # a face without candidates is not sent
        for (block, casters), k in zip(sent, keep):
            _distances(block, want[k], worst, ("face", i, k))
            assert len(casters) == len(shr.host_casters(want[k]["view_proj"], aabbs)) and tuple(np.frombuffer(block, np.float32, 4, 480)) == (0, 0, S, S)
    for j, (name, sun) in enumerate(SUNS.items()):
        for N in (2, 3, 4):
            r.set_shadow(2 + j, map_size=S, pcf_radius=R, cascades=N)
            r.render()
            rec, sent = _sent(lib)
            want = svr.host_cascades(sun, aabbs, sc.view, sc.proj, S, N)
            assert len(sent) == N and rec.light[3] == 0.0
            for k, (block, casters) in enumerate(sent):
                _distances(block, want[k], worst, (name, N, k))
                assert len(casters) == len(shr.host_casters(want[k]["view_proj"], aabbs)), (name, N, k)
            assert [w["r"] for w in want] == sorted(w["r"] for w in want)                    # tightest first
    print("host views against f64 under %s, worst relative distance per matrix: %s" % (cam, worst))
    r.close()


@pytest.mark.parametrize("cam", ["perspective", "ortho", "far"])
def test_cascade_and_face_properties_in_f64(cam):
    S = 40
    sc = sr.boxes(64, 48, cam)
    aabbs = shr.scene_aabbs(sc)
    for sun in SUNS.values():
        for N in (2, 3, 4):
            for w in svr.host_cascades(sun, aabbs, sc.view, sc.proj, S, N):
                # every slice corner lies in the cascade's deep region for R <= 2 (M = 3) at S >= 40
                q = np.c_[w["corners"], np.ones(8)] @ w["view_proj"]      # rows: corners; [col][row] storage applied from the left
                u, v = (q[:, 0] / q[:, 3] * 0.5 + 0.5) * S, (0.5 - q[:, 1] / q[:, 3] * 0.5) * S
                assert (u >= 3.0).all() and (u < S - 3.0).all() and (v >= 3.0).all() and (v < S - 3.0).all(), (N, u, v)
                # the window's origin is a whole multiple of its texel
                assert np.allclose(w["window"] / w["texel"], np.round(w["window"] / w["texel"]), rtol=0, atol=1e-6)
            # a tenth of a texel across the light: the window stays or moves by one texel
            base = svr.host_cascades(sun, aabbs, sc.view, sc.proj, S, N)
            side = base[0]["view"][:3, 0]      # the light's x axis in world space
            moved_view = np.asarray(sc.view, np.float64).copy()
            step = 0.1 * base[0]["texel"]
            moved_view[3][:3] -= moved_view[:3, :3].T @ (step * side)      # the camera moved by `step` along `side`
            moved = svr.host_cascades(sun, aabbs, moved_view, sc.proj, S, N)
            for a, b in zip(base, moved):
                shift = (b["window"] - a["window"]) / a["texel"]
                assert a["r"] == b["r"] and all(min(abs(s), abs(abs(s) - 1.0)) < 1e-6 for s in shift), shift
    # the six faces' deep regions are the cube's faces: 64 directions per face, each deep in its own face and in no other
    S, R = 96, 2
    faces = svr.host_cube_faces(POINT, aabbs, S, R)
    M = R + 1.0
    rng = np.random.default_rng(5)
    for k, axis in enumerate(svr.FACE_AXES):
        a = np.asarray(axis)
        for _ in range(64):
            d = a + (rng.uniform(-0.98, 0.98, 3)) * (1.0 - np.abs(a))
            p = np.append(np.asarray(POINT["position"]) + 2.0 * d, 1.0)
            for j, f in enumerate(faces):
                q = p @ f["view_proj"]
                u, v = (q[0] / q[3] * 0.5 + 0.5) * S, (0.5 - q[1] / q[3] * 0.5) * S
                deep = q[3] > 0 and M <= u < S - M and M <= v < S - M
                assert deep == (j == k), (k, j, d, u, v)


# ------------------------------------------------------------------------------------------------ 5. the host over the mocks

def test_host_hands_the_views_on_unchanged_and_in_order(mock_views):
    path, lib = mock_views
    sc = sr.boxes(64, 48)
    sc.lights = [SUNS["oblique"], POINT, dict(POINT, position=(30.0, 30.0, 30.0))]
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    old0, new0 = lib.mock_shadow_calls(), lib.mock_views_calls()      # (the library is the module's: earlier tests called it)
    calls = lambda: (lib.mock_shadow_calls() - old0, lib.mock_views_calls() - new0)
    # count = 1 calls the old entry only
    r.set_shadow(0, map_size=128, cascades=1)
    r.render()
    assert calls() == (1, 0)
    assert len(r.host.shadow_views()) == 1 and r.host.shadow_views()[0] == r.host.shadow_camera()
    # cascades: the views entry, and what it received is what shadow_views reports
    r.set_shadow(0, map_size=128, pcf_radius=2, strength=0.5, cascades=3, cascade_lambda=0.75, cascade_distance=12.0)
    r.render()
    assert calls() == (1, 1)
    rec, sent = _sent(lib)
    assert (rec.struct_size, rec.map_size, rec.pcf_radius, rec.strength) == (48, 128, 2, 0.5) and len(sent) == 3
    got = r.host.shadow_views()
    assert [b for b, _ in got] == [b for b, _ in sent] and [[bytes(hip_backend.AwsmDraw(**d)) for d in c] for _, c in got] == [c for _, c in sent]
    assert r.host.shadow_camera()[0] == sent[0][0]
    n, f, _ = svr.camera_planes(sc.proj)
    want = svr.host_cascades(SUNS["oblique"], shr.scene_aabbs(sc), sc.view, sc.proj, 128, 3, 0.75, 12.0)
    assert abs(1.0 / np.frombuffer(sent[2][0], np.float32, 16, 64)[0] - want[2]["r"]) < 1e-5 and f > 12.0
    ops = [op for op, _, _, _ in _log(lib, r.host.device_ctx)]
    at = lib.mock_views_at()
    assert ops[at - 1] == 7 and ops[at] == 8, ops[at - 2:at + 2]                             # between the geometry pass and the opaque pass
    # a point light ignores the cascades; inside the room every face sees a wall, the floor or (above y = 6, beyond x = 6 and z = 6) nothing ...
    r.set_shadow(1, map_size=96)
    r.render()
    rec, sent = _sent(lib)
    assert calls() == (1, 2) and len(sent) == len([k for k in range(6) if shr.host_casters(svr.host_cube_faces(POINT, shr.scene_aabbs(sc), 96, 1)[k]["view_proj"], shr.scene_aabbs(sc))]) and rec.light[3] == 1.0 and len(r.host.shadow_views()) == len(sent)
    # ... and from far outside the scene three faces see it: a face without candidates is not sent
    r.set_shadow(2, map_size=96)
    r.render()
    assert len(_sent(lib)[1]) == 3
    # refusals
    r.set_shadow(1, map_size=8)
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.render()
    r.set_shadow(1, map_size=96)
    lib.mock_views_refuse(-6)
    with pytest.raises(H.HostError, match=r"\(-6\)"):
        r.render()
    lib.mock_views_refuse(0)
    for bad in (dict(count=0), dict(count=5), dict(lambda_=-0.1), dict(lambda_=1.5), dict(max_distance=-1.0), dict(struct_size=12)):
        with pytest.raises(H.HostError, match=r"\(-1\)"):
            r.host.set_shadow_cascades(**bad)
    r.set_shadow(False); r.render()
    with pytest.raises(H.HostError, match=r"\(-5\)"):
        r.host.shadow_views()
    r.close()


def _log(lib, ctx):
    lib.mock_log_count.restype = C.c_size_t
    lib.mock_log_count.argtypes = [C.c_void_p]
    lib.mock_log_get.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    out = []
    for i in range(lib.mock_log_count(ctx)):
        op, which, a, b = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        lib.mock_log_get(ctx, i, C.byref(op), C.byref(which), C.byref(a), C.byref(b))
        out.append((op.value, which.value, a.value, b.value))
    return out


def test_host_over_a_backend_without_the_views_entry_names_the_symbol(tmp_path):
    """Over mock_backend_shadow.c (shadows, but one map): a point light and count > 1 are refused, naming the symbol; count = 1 is accepted."""
    out = str(tmp_path / "libmock_backend_shadow.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_shadow.c")])
    sc = sr.boxes(64, 48)
    sc.lights = [SUNS["oblique"], POINT]
    r = H.Renderer(sc, backend_path=out, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_shadow_pass_views"):
        r.set_shadow(1)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_shadow_pass_views"):
        r.host.set_shadow_cascades(2)
    r.host.set_shadow_cascades(1)
    r.set_shadow(0)
    r.render()
    assert len(r.host.shadow_views()) == 1
    r.close()


def test_host_record_layouts_are_the_headers():
    header = open(os.path.join(ROOT, "include", "awsm_host.h")).read()
    body = re.search(r"typedef struct AwsmHostShadowCascades \{(.*?)\} AwsmHostShadowCascades;", header, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", body) == ["struct_size", "count", "lambda", "max_distance"]
    assert [n.rstrip("_") for n, _ in H.HostShadowCascades._fields_] == ["struct_size", "count", "lambda", "max_distance"] and C.sizeof(H.HostShadowCascades) == 16
    c = H.HostShadowCascades()
    assert H.load_library().awsm_host_shadow_cascades_defaults(C.byref(c)) == 0 and (c.struct_size, c.count, c.lambda_, c.max_distance) == (16, 1, 0.5, 0.0)
    assert C.sizeof(H.HostShadow) == 48
