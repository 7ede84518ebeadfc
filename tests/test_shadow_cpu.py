"""CPU tests of the shadows: the numpy restatement against known answers on the CPU oracle's keys — from the scene's camera and from
the light block —, the records' layout and the library's defaults, the host layer over mock backends with and without the entry points, the host's
light camera against its f64 restatement, and the conditions that keep tests/test_shadow_gpu.py informative."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from oracle import oracle_lib
from tests import helpers
from tests import shadow_reference as shr
from tests import ssao_reference as sr
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, mock  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = dict(sr.SCENES, floating_quad=shr.floating_quad)


@functools.lru_cache(maxsize=None)
def _scene(scene, cam, W, Hh):
    """The CPU oracle's keys of a scene (no GPU), the camera block its model wrote, and the model."""
    model = helpers.build_model(SCENES[scene](W, Hh, cam))
    orc = helpers.oracle_frame(model, oracle_lib.brdf_lut(16, 16))
    return np.asarray(orc.keys, np.uint64).reshape(Hh, W).copy(), bytes(model.camera_bytes), model


def _freeze(light):
    return light if isinstance(light, str) else tuple(sorted(light.items()))


@functools.lru_cache(maxsize=None)
def _map(scene, cam, W, Hh, light, S):
    light = light if isinstance(light, str) else dict(light)
    block = shr.light_block(light, S)
    return shr.caster_map(_scene(scene, cam, W, Hh)[2], block, S), block


def _run(scene, cam, W, Hh, light, S, params=None, dtype=np.float32):
    keys, block, _ = _scene(scene, cam, W, Hh)
    map_keys, light_block = _map(scene, cam, W, Hh, _freeze(light), S)
    p = dict(params or {}, light=shr.light_vec(light))
    return shr.shadow(keys, block, W, Hh, map_keys, light_block, S, p, dtype)


# ------------------------------------------------------------------------------------------------ known answers

@pytest.mark.parametrize("cam", ["perspective", "ortho"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_oblique_plane_under_a_light_it_faces_has_no_acne(cam, dtype):
    """Every hit pixel V == 1: the receiver plane's slope carries each tap's depth along the plane, the constant bias covers the rounding."""
    for S in (40, 96):
        for R in (0, 1, 2):
            out = _run("plane", cam, 70, 45, shr.plane_light(cam), S, {"pcf_radius": R}, dtype)
            hit = out["hit"]
            assert hit.sum() >= 3000 and out["inside"][hit].all() and (out["g"][hit] == 1.0).all()
            assert (out["V"][hit] == 1.0).all() and (out["m"] == 1.0).all(), (S, R, int((out["V"][hit] != 1.0).sum()))


@pytest.mark.parametrize("S", shr.MAP_SIZES)
@pytest.mark.parametrize("R", [0, 1, 2])
def test_a_floating_quad_shadows_the_floor_under_it_and_nothing_else(R, S):
    """A vertical directional light, every floor pixel of the frame (y = 0 to the depth's precision): those whose position lies under the quad by more
    than R + 1 texels have V == 0; those outside it by more than R + 1 texels have V == 1 — from geometry alone — unless one of their four image
    neighbours is not a floor pixel.  There (the floor-wall creases, the pixels next to the quad's outline) step 4 may hand steps 5 and 6 a neighbour on
    another surface and the receiver plane's slope belongs to neither.  What still holds for such a pixel, whatever the slope: the floor's own depth in
    the map is z, so a tap is unlit only if zu cu + zv cv > bias + |zu| + |zv|, which needs cu > 1 on the side of zu's sign or cv > 1 on the side of
    zv's; cu lies in (dx - 1/2, dx + 1/2], so the taps with dx and dy on the other side or at 0 — (R + 1)^2 of the (2R + 1)^2 — are lit:
    V >= (R + 1)^2 / (2R + 1)^2, and V == 1 at R = 0.  Those pixels form one-pixel lines: fewer than 2 (W + H) of them (each crease and each edge of
    the outline crosses a row or a column once)."""
    W, Hh = 70, 45
    out = _run("floating_quad", "perspective", W, Hh, "zenith", S, {"pcf_radius": R})
    x, y, z = out["Pw"]
    floor = out["hit"] & (np.abs(y) < 1e-3)
    interior = sr._shift(floor, 0, 1) & sr._shift(floor, 0, -1) & sr._shift(floor, 1, 0) & sr._shift(floor, -1, 0)      # (the frame's edge repeats the pixel itself)
    t = (R + 1) * 2.0 * shr.LIGHTS["zenith"]["ortho_half_height"] / S
    (xa, xb), (za, zb) = shr.QUAD["x"], shr.QUAD["z"]
    under = floor & (x > xa + t) & (x < xb - t) & (z > za + t) & (z < zb - t)
    outside = floor & ((x < xa - t) | (x > xb + t) | (z < za - t) | (z > zb + t))
    V = out["V"]
    print("S = %d R = %d: %d floor pixels under, %d outside, of them %d beside another surface, %d of those with V < 1 (least %.3f)" % (
        S, R, under.sum(), outside.sum(), (outside & ~interior).sum(), (outside & (V != 1.0)).sum(), V[outside].min()))
    assert under.sum() >= 4 and outside.sum() >= 100, (int(under.sum()), int(outside.sum()))
    assert (V[under] == 0.0).all(), int((V[under] != 0).sum())
    assert (V[outside & interior] == 1.0).all(), int((V[outside & interior] != 1).sum())
    beside = outside & ~interior
    assert beside.sum() < 2 * (W + Hh) and (V[beside] >= np.float32((R + 1) ** 2) / np.float32((2 * R + 1) ** 2)).all(), (int(beside.sum()), float(V[beside].min()))
    assert (out["g"][floor & interior] == 1.0).all()
    assert np.array_equal(out["m"][under & interior], np.full(int((under & interior).sum()), np.float32(1.0) - np.float32(0.7) * np.float32(1.0), np.float32))


def test_pixels_the_light_does_not_reach_or_the_surface_turns_from_keep_their_colour():
    """Outside the map, behind a spot (q.w <= 0), not hit, or turned away from the light: m == 1."""
    W, Hh, S = 70, 45, 96
    # a narrow map around the boxes: most of the floor and the walls fall outside it
    narrow = dict(shr.LIGHTS["sun"], ortho_half_height=0.8)
    out = _run("boxes", "perspective", W, Hh, narrow, S)
    outside = out["hit"] & ~out["inside"]
    assert outside.sum() >= 500 and (out["V"][outside] == 1.0).all() and (out["m"][outside] == 1.0).all() and (out["V"][out["inside"]] < 1.0).sum() >= 20
    # a spot in the middle of the room looking away from the corner: the corner is behind it
    away = dict(kind="spot", position=(2.0, 1.0, 2.0), target=(4.0, 0.5, 4.0), fovy_deg=70.0, near=0.5, far=20.0)
    out = _run("boxes", "perspective", W, Hh, away, S)
    keys, block, _ = _scene("boxes", "perspective", W, Hh)
    lvp = np.frombuffer(shr.light_block(away, S), np.float32, 16, 128).reshape(4, 4).astype(np.float64)
    qw = sum(lvp[i][3] * np.asarray(out["Pw"][i], np.float64) for i in range(3)) + lvp[3][3]
    behind = out["hit"] & (qw <= 0)
    assert behind.sum() >= 500 and not out["inside"][behind].any() and (out["m"][behind] == 1.0).all()
    # nothing hit: the `far` camera sees the scene small in an empty frame
    out = _run("boxes", "far", W, Hh, "sun", S)
    assert (~out["hit"]).sum() >= 1000 and (out["V"][~out["hit"]] == 1.0).all() and (out["m"][~out["hit"]] == 1.0).all()
    # turned away: under the sun (it comes from +x +y +z) no wall or floor is, under a light from below the floor every upward face is
    below = dict(kind="directional", towards=(0.1, -1.0, 0.2), target=(1.2, 0.4, 1.2), distance=8.0, ortho_half_height=4.6, near=0.5, far=20.0)
    out = _run("boxes", "perspective", W, Hh, below, S)
    x, y, z = out["Pw"]
    on_floor = out["hit"] & (np.abs(y) < 1e-3)
    floor = on_floor & sr._shift(on_floor, 0, 1) & sr._shift(on_floor, 0, -1) & sr._shift(on_floor, 1, 0) & sr._shift(on_floor, -1, 0)      # (its normal is the floor's)
    assert floor.sum() >= 500 and out["has_normal"][floor].all() and (out["g"][floor] == 0.0).all() and (out["m"][floor] == 1.0).all()


@pytest.mark.parametrize("light", ["sun", "spot"])
def test_one_tap_gives_zero_or_one(light):
    out = _run("boxes", "closeup", 70, 45, light, 96, {"pcf_radius": 0})
    V = out["V"]
    assert ((V == 0.0) | (V == 1.0)).all() and (V == 0.0).sum() >= 200 and (V == 1.0).sum() >= 200
    many = _run("boxes", "closeup", 70, 45, light, 96, {"pcf_radius": 2})["V"]
    assert set(np.unique(np.round(many * 25).astype(int))) >= set(range(0, 26, 5)) and np.allclose(many * 25, np.round(many * 25), atol=1e-5)


def test_strength_and_facing_enter_the_multiplier_only():
    base = _run("boxes", "closeup", 33, 17, "sun", 96)
    off = _run("boxes", "closeup", 33, 17, "sun", 96, {"strength": 0.0})
    assert (off["m"] == 1.0).all() and np.array_equal(off["V"], base["V"]) and (base["m"] < 1.0).sum() >= 50
    full = _run("boxes", "closeup", 33, 17, "sun", 96, {"strength": 1.0, "facing_fade": 1e-6})
    lit = full["hit"] & (full["g"] == 1.0)
    assert lit.sum() >= 300 and np.array_equal(full["m"][lit], np.float32(1.0) - (np.float32(1.0) - full["V"][lit]))      # m = 1 - (1 * 1) (1 - V), as f32 forms it


# ------------------------------------------------------------------------------------------------ what keeps the GPU tests informative

@pytest.mark.parametrize("W,Hh", sr.SIZES)
@pytest.mark.parametrize("light", ["sun", "spot"])
def test_the_close_up_camera_sees_shadow_light_and_penumbra(light, W, Hh):
    """`boxes` under the `closeup` camera, R = 1, S = 96: among the pixels that are hit, facing the light and inside the map at least 10 % have V == 0,
    at least 25 % V == 1, and at least 5 pixels lie strictly between — at each frame size of the GPU tests.  Measured:
    sun 17.5 / 12.1 / 15.1 % at 0, 45.0 / 63.6 / 56.8 % at 1, 15 / 136 / 886 between; spot 40.0 / 34.4 / 40.7 %, 30.0 / 39.4 / 34.5 %, 12 / 147 / 783."""
    out = _run("boxes", "closeup", W, Hh, light, 96, {"pcf_radius": 1})
    sel = out["hit"] & out["inside"] & (out["g"] > 0.0)
    V, n = out["V"][sel], int(sel.sum())
    print("%s %dx%d: %d pixels; V == 0 on %.3f, V == 1 on %.3f, %d between" % (light, W, Hh, n, (V == 0).mean(), (V == 1).mean(), ((V > 0) & (V < 1)).sum()))
    assert n >= 0.9 * W * Hh
    assert (V == 0.0).sum() >= 0.10 * n and (V == 1.0).sum() >= 0.25 * n and ((V > 0.0) & (V < 1.0)).sum() >= 5


# ------------------------------------------------------------------------------------------------ records, defaults, constants

def _fields(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for t, names in re.findall(r"(uint32_t|float|AwsmKey)\s+([^;]+);", body):
        for n in names.split(","):
            n = n.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", n)
            out.append((arr.group(1), t, int(arr.group(2))) if arr else (n, t, 1))
    return out


def _check_layout(header, name, ctype):
    base = {"uint32_t": C.c_uint32, "float": C.c_float, "AwsmKey": C.c_uint64}
    fields = _fields(header, name)
    assert [n for n, _, _ in fields] == [n for n, _ in ctype._fields_]
    at = 0
    for (n, t, k), (_, ct) in zip(fields, ctype._fields_):
        assert ct is (base[t] * k if k > 1 else base[t]) or (k > 1 and C.sizeof(ct) == 4 * k), n
        at = (at + C.alignment(ct) - 1) // C.alignment(ct) * C.alignment(ct)      # the C compiler's rule
        assert getattr(ctype, n).offset == at, n
        at += C.sizeof(ct)
    return at


def test_record_layouts_are_the_headers():
    assert _check_layout("awsm_hip.h", "AwsmShadow", hip_backend.AwsmShadow) == 48 == C.sizeof(hip_backend.AwsmShadow)
    assert _check_layout("awsm_host.h", "AwsmHostShadow", H.HostShadow) == 44 and C.sizeof(H.HostShadow) == 48 and H.HostShadow.light.offset == 8
    text = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "shadow.hpp")).read()
    assert int(re.search(r"kTile = (\d+)", text).group(1)) == shr.TILE and int(re.search(r"kMaxRadius = (\d+)", text).group(1)) == shr.MAX_RADIUS
    assert float(re.search(r"kDetMin = ([0-9.e+-]+)f", text).group(1)) == shr.DET_MIN and shr.WIN == shr.TILE + 2


def test_the_library_hands_out_the_defaults():
    lib = hip_backend.load_library()      # links against the HIP runtime and loads without a GPU; a library that does not load is a failure
    s = hip_backend.AwsmShadow()
    assert lib.awsm_hip_shadow_defaults(C.byref(s)) == 0 and lib.awsm_hip_shadow_defaults(None) == -1
    assert s.struct_size == C.sizeof(hip_backend.AwsmShadow)
    for k, v in shr.DEFAULTS.items():
        got = tuple(s.light) if k == "light" else getattr(s, k)
        assert got == (tuple(v) if k == "light" else (v if isinstance(v, int) else float(np.float32(v)))), k
    with pytest.raises(TypeError):
        s.override(strenght=1.0)
    assert lib.awsm_hip_shadow_pass(None, C.byref(s), None, 0, None, 0) == -1 and lib.awsm_hip_read_shadow(None, None, None) == -1


# ------------------------------------------------------------------------------------------------ the host layer

@pytest.fixture(scope="module")
def mock_shadow(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_shadow") / "libmock_backend_shadow.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_shadow.c")])
    lib = C.CDLL(out)
    lib.mock_shadow_last.restype = C.c_uint32
    lib.mock_shadow_at.restype = C.c_size_t
    return out, lib


def _last(lib):
    rec, block, draws = hip_backend.AwsmShadow(), (C.c_uint8 * 512)(), (hip_backend.AwsmDraw * 256)()
    n = lib.mock_shadow_last(C.byref(rec), block, draws, 256)
    return rec, bytes(block), [bytes(draws[i]) for i in range(n)]


SPOT = {"kind": "spot", "color": (1.0, 1.0, 1.0), "intensity": 20.0, "position": (3.0, 3.2, 2.2), "direction": (-2.0, -3.2, -1.2), "range": 0.0,
        "inner_angle": 0.9063, "outer_angle": 0.8192}      # cosines of 25 and 35 degrees


def _boxes_with(lights, W=64, Hh=48):
    sc = sr.boxes(W, Hh)
    sc.lights = list(lights)
    return sc


def test_host_hands_the_block_and_the_casters_on_unchanged(mock_shadow):
    path, lib = mock_shadow
    sun = {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 1.0, "direction": tuple(-shr._SUN)}
    sc = _boxes_with([sun, SPOT, {"kind": "point", "color": (1.0, 1.0, 1.0), "intensity": 1.0, "position": (1.0, 2.0, 1.0), "range": 9.0}])
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    r.render()
    assert lib.mock_shadow_calls() == 0                                                      # off until it is set
    with pytest.raises(H.HostError, match=r"\(-5\)"):
        r.host.shadow_camera()
    r.set_shadow(True, map_size=512, pcf_radius=2, bias=0.002, strength=0.5)
    r.render()
    assert lib.mock_shadow_calls() == 1
    rec, block, casters = _last(lib)
    assert (rec.struct_size, rec.map_size, rec.pcf_radius, rec.bias, rec.strength) == (48, 512, 2, float(np.float32(0.002)), 0.5)
    assert (rec.slope_bias, rec.max_slope, rec.facing_fade) == (1.0, float(np.float32(0.05)), float(np.float32(0.1)))
    assert tuple(rec.light) == tuple(float(np.float32(c)) for c in shr._SUN) + (0.0,)
    got_block, got_casters = r.host.shadow_camera()
    assert got_block == block and [bytes(hip_backend.AwsmDraw(**d)) for d in got_casters] == casters
    assert len(casters) == 6                                                                 # the floor, two walls, three boxes: all of it inside the sun's box
    # ... between the geometry pass and the opaque pass
    ops = [op for op, _, _, _ in _log(lib, r.host.device_ctx)]
    at = lib.mock_shadow_at()
    assert ops[at - 1] == 7 and ops[at] == 8, ops[at - 2:at + 2]
    # the spot sees less than everything; every frame has its pass
    r.set_shadow(1)
    r.render(); r.render()
    assert lib.mock_shadow_calls() == 3
    rec, block, casters_spot = _last(lib)
    assert tuple(rec.light) == (3.0, float(np.float32(3.2)), float(np.float32(2.2)), 1.0) and rec.map_size == 2048
    want = shr.host_light_camera(SPOT, shr.scene_aabbs(sc))
    keep = shr.host_casters(want["view_proj"], shr.scene_aabbs(sc))
    assert len(casters_spot) == len(keep) and set(casters_spot) <= set(casters)
    # refusals: the backend's come back from render(), a point light and an unknown key from set_shadow
    r.set_shadow(1, strength=1.5)
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.render()
    lib.mock_shadow_refuse(-6)
    r.set_shadow(1)
    with pytest.raises(H.HostError, match=r"\(-6\)"):
        r.render()
    lib.mock_shadow_refuse(0)
    with pytest.raises(H.HostError, match=r"\(-6\)"):
        r.set_shadow(2)
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.host.set_shadow(0xDEAD)
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.host.set_shadow(r.keys.light_keys[0], struct_size=40)
    r.render()                                                                               # the refused calls left the spot on
    assert _last(lib)[0].light[3] == 1.0
    # a removed light turns the feature off, said once
    r.host.light_remove(r.keys.light_keys[1])
    calls = lib.mock_shadow_calls()
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.render()
    r.render()
    assert lib.mock_shadow_calls() == calls
    with pytest.raises(H.HostError, match=r"\(-5\)"):
        r.host.shadow_camera()
    r.set_shadow(True); r.render()
    r.set_shadow(False); r.render()
    assert lib.mock_shadow_calls() == calls + 1
    assert r.host.lib.awsm_host_set_shadow(None, None) == -1 and r.host.lib.awsm_host_shadow_defaults(r.host.h, None) == -1
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


def test_host_over_a_backend_without_shadows_reports_unsupported_and_names_the_symbol(mock):  # noqa: F811
    r = H.Renderer(sr.boxes(64, 48), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_shadow_pass"):
        r.host.set_shadow(None)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_shadow_defaults"):
        r.set_shadow(True)
    s = H.HostShadow(48, r.keys.light_keys[0], 2048, 1, 1e-3, 1.0, 0.05, 0.7, 0.1)
    assert r.host.lib.awsm_host_set_shadow(r.host.h, C.byref(s)) == -6                       # AWSM_ERR_UNSUPPORTED
    r.render()                                                                               # and renders as before
    r.close()


# The worst distance measured between the host's f32 block and the f64 restatement over HOST_LIGHTS, per matrix and relative to the matrix's largest
# entry: view 3.2e-8, proj 3.6e-8, view_proj 6.9e-8 (the f32 rounding of the entries and one f32 matrix product; the test prints them).  The
# tolerance is 4 x that.
HOST_TOLERANCE = {"view": 4 * 3.2e-8, "proj": 4 * 3.6e-8, "view_proj": 4 * 6.9e-8}
_D = {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 1.0}
HOST_LIGHTS = {
    "directional": dict(_D, direction=(0.1, -0.35, -1.0)),
    "rolled": dict(_D, direction=(-0.62, -0.41, 0.33)),
    "down": dict(_D, direction=(0.0, -1.0, 0.0)),
    "up": dict(_D, direction=(0.0, 2.0, 0.0)),
    "spot": SPOT,
    "spot with range": dict(SPOT, range=7.5),
    # what the glTF reader makes of a spot without cone angles: cos(0) and cos(pi / 4)
    "glTF default spot": dict(SPOT, inner_angle=1.0, outer_angle=float(np.float32(np.cos(np.float32(0.7853981633974483))))),
}


def _cone_in_map(block, light, scale):
    """Directions at `scale` times the outer cone's half angle around the spot's axis, 5 units out, through the block's view_proj -> the largest |ndc x|,
    |ndc y| among them (inf if one is behind the camera)."""
    axis = shr._unit(light["direction"])
    side = shr._unit(np.cross(axis, (0.0, 1.0, 0.0)))
    other = np.cross(axis, side)
    half = scale * np.arccos(float(np.float32(light["outer_angle"])))
    vp = np.frombuffer(block, np.float32, 16, 128).reshape(4, 4).astype(np.float64)
    worst = 0.0
    for a in np.linspace(0.0, 2.0 * np.pi, 64, endpoint=False):
        d = np.cos(half) * axis + np.sin(half) * (np.cos(a) * side + np.sin(a) * other)
        p = np.append(np.asarray(light["position"], np.float64) + 5.0 * d, 1.0)
        q = vp.T @ p
        worst = max(worst, np.inf if q[3] <= 0 else max(abs(q[0] / q[3]), abs(q[1] / q[3])))
    return worst


@pytest.mark.parametrize("empty", [False, True])
def test_host_light_camera_is_the_f64_restatement(mock_shadow, empty):
    path, lib = mock_shadow
    sc = _boxes_with(HOST_LIGHTS.values())
    if empty:
        sc.nodes = []
    aabbs = shr.scene_aabbs(sc)
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    worst = {k: 0.0 for k in HOST_TOLERANCE}
    for i, (name, light) in enumerate(HOST_LIGHTS.items()):
        r.set_shadow(i, map_size=256)
        r.render()
        rec, block, casters = _last(lib)
        want = shr.host_light_camera(light, aabbs)
        assert np.allclose(tuple(rec.light), want["light"], rtol=0, atol=1e-6), name
        for k, byte in (("view", 0), ("proj", 64), ("view_proj", 128)):
            got = np.frombuffer(block, np.float32, 16, byte).reshape(4, 4).astype(np.float64)
            dist = np.abs(got - want[k]).max() / np.abs(want[k]).max()
            worst[k] = max(worst[k], dist)
            assert dist <= HOST_TOLERANCE[k], (name, k, dist)
        assert np.allclose(np.frombuffer(block, np.float32, 3, 384), want["eye"], rtol=1e-6, atol=1e-6) and tuple(np.frombuffer(block, np.float32, 4, 480)) == (0, 0, 256, 256)
        assert len(casters) == len(shr.host_casters(want["view_proj"], aabbs)), name
        if light["kind"] == "spot":                                                            # the map spans the lit cone, and no more than it
            assert _cone_in_map(block, light, 0.999) < 1.0 and 1.0 < _cone_in_map(block, light, 1.02) < 1.1, name
        if light["kind"] == "directional" and not empty:                                     # the box is square, holds every candidate, and does not depend on the roll
            assert len(casters) == len(aabbs)
            assert want["proj"][0][0] == want["proj"][1][1]
    print("host light block against f64, worst relative distance per matrix (%s): %s" % ("empty" if empty else "boxes", worst))
    r.close()
