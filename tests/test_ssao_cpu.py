"""CPU tests of the screen-space ambient occlusion: the numpy restatement against known answers on the CPU oracle's depth, the
header's literals against their derivation, the record's layout, the host layer over mock backends with and without the entry points, and the
conditions that keep tests/test_ssao_gpu.py informative."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from oracle import oracle_lib
from tests import helpers
from tests import ssao_reference as sr
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, mock  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle_keys(scene, cam, W, Hh):
    """The CPU oracle's keys of a scene (no GPU) and the camera block its model wrote."""
    model = helpers.build_model(sr.SCENES[scene](W, Hh, cam))
    orc = helpers.oracle_frame(model, oracle_lib.brdf_lut(16, 16))
    return np.asarray(orc.keys, np.uint64).reshape(Hh, W).copy(), bytes(model.camera_bytes)


def _run(scene, cam, W, Hh, dtype=np.float32, params=None):
    keys, block = _oracle_keys(scene, cam, W, Hh)
    return sr.ssao(keys, block, W, Hh, params, dtype), block


def _world(out, block):
    """World positions of the view positions of a run (f64)."""
    iv = np.frombuffer(block, np.float32, 16, 320).reshape(4, 4).astype(np.float64)      # [col][row]
    P = [np.asarray(c, np.float64) for c in out["P"]]
    return tuple(iv[0][r] * P[0] + iv[1][r] * P[1] + iv[2][r] * P[2] + iv[3][r] for r in range(3))


# ------------------------------------------------------------------------------------------------ known answers

@pytest.mark.parametrize("cam", ["perspective", "ortho"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_oblique_plane_is_not_occluded(cam, dtype):
    """v . n = 0 for every tap on the plane itself; the bias (1 % of a world unit) is far above what the depth's 24 bits leave of it."""
    out, _ = _run("plane", cam, 70, 45, dtype)
    hit = out["hit"]
    assert hit.sum() >= 3000 and out["active"][hit].mean() > 0.95
    assert (out["ao_raw"][hit] == 1.0).all() and (out["ao_smoothed"][hit] == 1.0).all() and (out["m"] == 1.0).all()


def test_the_view_position_is_the_surface():
    """The reconstructed positions of `corner` lie on the floor or on a wall (one world coordinate 0), to the depth's precision."""
    out, block = _run("corner", "perspective", 70, 45, np.float64)
    wx, wy, wz = _world(out, block)
    hit = out["hit"]
    assert hit.all()
    assert np.minimum(np.minimum(np.abs(wx), np.abs(wy)), np.abs(wz))[hit].max() < 2e-4
    assert (out["view_z"][hit] < 0).all()                                                   # view space looks down -z


def test_creases_are_darker_than_open_floor():
    out, block = _run("corner", "perspective", 70, 45, np.float64)
    wx, wy, wz = _world(out, block)
    near0 = lambda a: np.abs(a) < 0.06      # noqa: E731
    crease = (near0(wx).astype(int) + near0(wy).astype(int) + near0(wz).astype(int)) >= 2
    open_floor = near0(wy) & (wx > 1.2) & (wz > 1.2)
    assert crease.sum() >= 60 and open_floor.sum() >= 150      # enough of each to mean something
    As = out["ao_smoothed"]
    assert (As[open_floor] == 1.0).all()
    assert As[crease].max() < 0.93 and As[crease].mean() < 0.85, (As[crease].max(), As[crease].mean())
    normal_y = out["normal"][1][open_floor]                                                 # the floor's normal, in view space: the view matrix's image of +y
    view = np.frombuffer(block, np.float32, 16, 0).reshape(4, 4).astype(np.float64)
    assert np.abs(normal_y - view[1][1]).max() < 1e-3


def test_background_and_small_radius_pixels_are_not_occluded():
    keys, block = _oracle_keys("corner", "far", 70, 45)
    out = sr.ssao(keys, block, 70, 45)
    hit = out["hit"]
    assert (~hit).sum() >= 1000 and (out["ao_raw"][~hit] == 1.0).all() and (out["ao_smoothed"][~hit] == 1.0).all() and (out["m"][~hit] == 1.0).all()
    assert np.isnan(out["view_z"][~hit]).all()
    small = hit & (out["r"] < 1.0)
    assert small.sum() >= 20 and (out["ao_raw"][small] == 1.0).all()
    # one key by hand: depth 0.5 at the centre of a frame that hit nothing else has no neighbour to take a normal from
    alone = np.full((5, 8), sr.NO_HIT, np.uint64)
    alone[2, 4] = (np.uint64(np.float32(0.5).view(np.uint32)) << np.uint64(32)) | np.uint64(3)
    o = sr.ssao(alone, sr.camera("closeup", 8, 5), 8, 5)
    assert o["hit"].sum() == 1 and not o["active"].any() and (o["ao_raw"] == 1.0).all() and (o["ao_smoothed"] == 1.0).all()


def test_msaa_takes_the_least_depth_and_any_sample_hits():
    f = lambda v: (np.uint64(np.float32(v).view(np.uint32)) << np.uint64(32)) | np.uint64(1)      # noqa: E731
    keys = np.array([[[f(0.5), sr.NO_HIT, f(0.25), f(0.75)], [sr.NO_HIT] * 4]], np.uint64)
    d, hit = sr.depth_and_hit(keys)
    assert d.tolist() == [[0.25, 0.0]] and hit.tolist() == [[True, False]]


def test_apply_rounds_to_f16_once_and_keeps_alpha():
    bits = np.array([[[1.0, 0.5, 0.3, 0.7], [1.0, 0.5, 0.3, 0.7]]], np.float16).view(np.uint16)
    m, hit = np.array([[0.6, 0.6]], np.float32), np.array([[True, False]])
    got = sr.apply(bits, m, hit)
    want = (np.array([1.0, 0.5, 0.3], np.float16).astype(np.float32) * np.float32(0.6)).astype(np.float16).view(np.uint16)
    assert (got[0, 0, :3] == want).all() and got[0, 0, 3] == bits[0, 0, 3] and (got[0, 1] == bits[0, 1]).all()
    img = np.array([[[1.0, 0.5, 0.3, 0.7]] * 2], np.float32)
    g32 = sr.apply_f32(img, m, hit)
    assert (g32[0, 0, :3] == img[0, 0, :3] * np.float32(0.6)).all() and g32[0, 0, 3] == img[0, 0, 3] and (g32[0, 1] == img[0, 1]).all()


# ------------------------------------------------------------------------------------------------ what keeps the GPU tests informative

CORNER_CASES = [("along", W, Hh) for (W, Hh) in sr.SIZES] + [("perspective", W, Hh) for (W, Hh) in sr.SIZES[1:]]


@pytest.mark.parametrize("cam,W,Hh", CORNER_CASES)
def test_corner_has_occluded_and_open_pixels(cam, W, Hh):
    """At least 15 % of `corner`'s hit pixels with A' < 0.95 and at least 15 % with A' == 1: under the `along` camera at all three sizes, under the
    `perspective` camera at the two where half a world unit is more than a pixel for it."""
    out, _ = _run("corner", cam, W, Hh)
    As, n = out["ao_smoothed"][out["hit"]], out["hit"].sum()
    print("corner %s %dx%d: A' < 0.95 on %.3f, A' == 1 on %.3f of %d hit pixels" % (cam, W, Hh, (As < 0.95).mean(), (As == 1.0).mean(), n))
    assert n >= 0.9 * W * Hh and (As < 0.95).sum() >= 0.15 * n and (As == 1.0).sum() >= 0.15 * n


def test_close_up_clamps_the_radius_and_far_goes_under_a_pixel():
    out, _ = _run("corner", "closeup", 70, 45)
    r, n = out["r"][out["hit"]], out["hit"].sum()
    print("closeup 70x45: r >= R_MAX on %.3f of %d hit pixels, least r %.2f" % ((r >= sr.R_MAX).mean(), n, r.min()))
    assert (r >= sr.R_MAX).sum() >= 0.25 * n and (r < sr.R_MAX).sum() >= 20
    for scene in ("corner", "boxes"):
        out, _ = _run(scene, "far", 70, 45)
        r, act = out["r"][out["hit"]], out["active"][out["hit"]]
        print("far %s 70x45: r < 1 on %d, active on %d of %d hit pixels" % (scene, (r < 1.0).sum(), act.sum(), out["hit"].sum()))
        assert (r < 1.0).sum() >= 20 and act.sum() >= 20


# ------------------------------------------------------------------------------------------------ the header

def _header_table(name):
    text = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "ssao.hpp")).read()
    body = re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, text, re.S).group(1)
    return np.array([float(v.rstrip("f")) for v in re.findall(r"-?\d+\.\d+e[+-]\d+f", body)], dtype=np.float32)


def test_header_literals_are_the_derivation():
    assert np.array_equal(_header_table("kSpiral"), sr.SPIRAL.reshape(-1))
    assert np.array_equal(_header_table("kRotation"), sr.ROTATION.reshape(-1))
    text = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "ssao.hpp")).read()
    assert int(re.search(r"kTaps = (\d+)", text).group(1)) == sr.K and int(re.search(r"kRMax = (\d+)", text).group(1)) == sr.R_MAX
    assert int(re.search(r"kBlur = (\d+)", text).group(1)) == sr.BLUR
    # a rotated tap is shorter than one radius: the rounded offset never leaves the staged apron
    reach = np.abs(sr.ROTATION.reshape(16, 1, 2).astype(np.float64)).max() * np.sqrt((sr.SPIRAL.astype(np.float64) ** 2).sum(-1)).max()
    assert np.floor(reach * 1.001 * sr.R_MAX + 0.5) <= sr.R_MAX


def test_record_layout_is_the_headers():
    text = open(os.path.join(ROOT, "include", "awsm_hip.h")).read()
    body = re.search(r"typedef struct AwsmSsao \{(.*?)\} AwsmSsao;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t|float)\s+(\w+);", body)
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(hip_backend.AwsmSsao._fields_)
    for i, (_, n) in enumerate(fields):
        assert getattr(hip_backend.AwsmSsao, n).offset == 4 * i
    assert C.sizeof(hip_backend.AwsmSsao) == 4 * len(fields) == 20


def test_the_library_hands_out_the_defaults():
    lib = hip_backend.load_library()      # links against the HIP runtime and loads without a GPU; a library that does not load is a failure
    s = hip_backend.AwsmSsao()
    assert lib.awsm_hip_ssao_defaults(C.byref(s)) == 0 and lib.awsm_hip_ssao_defaults(None) == -1
    assert s.struct_size == C.sizeof(hip_backend.AwsmSsao)
    for k, v in sr.DEFAULTS.items():
        assert getattr(s, k) == float(np.float32(v)), k
    with pytest.raises(TypeError):
        s.override(radious=1.0)


# ------------------------------------------------------------------------------------------------ the host layer

@pytest.fixture(scope="module")
def mock_ssao(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_ssao") / "libmock_backend_ssao.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_ssao.c")])
    return out, C.CDLL(out)


def test_host_passes_the_record_through_unchanged(mock_ssao):
    path, lib = mock_ssao
    lib.mock_ssao_record.restype = C.c_uint32
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    got = (C.c_uint8 * 64)()
    before = lib.mock_ssao_calls()
    r.set_ssao(True, radius=0.75, intensity=1.5, bias=0.03125, strength=0.5)
    assert lib.mock_ssao_calls() == before + 1 and lib.mock_ssao_record(got, 64) == 20
    want = hip_backend.AwsmSsao(20, 0.75, 1.5, 0.03125, 0.5)
    assert bytes(got[:20]) == bytes(want)
    # a shorter record, raw: the host does not read or complete it
    short = hip_backend.AwsmSsao(12, 2.0, 3.0, -1.0, -1.0)
    assert r.host.lib.awsm_host_set_ssao(r.host.h, C.byref(short)) == 0
    assert lib.mock_ssao_record(got, 64) == 12 and bytes(got[:12]) == bytes(short)[:12]
    # the backend's refusal comes back as it is, and the call before it stands
    bad = hip_backend.AwsmSsao(20, -1.0, 1.0, 0.02, 1.0)
    assert r.host.lib.awsm_host_set_ssao(r.host.h, C.byref(bad)) == -1
    with pytest.raises(H.HostError, match=r"\(-1\)"):
        r.set_ssao(True, radius=0.0)
    assert lib.mock_ssao_record(got, 64) == 12
    r.set_ssao(False)
    assert lib.mock_ssao_record(got, 64) == 0xFFFFFFFF                                      # NULL went through
    assert r.host.lib.awsm_host_set_ssao(None, None) == -1 and r.host.lib.awsm_host_ssao_defaults(r.host.h, None) == -1
    r.render()
    r.close()


def test_host_over_a_backend_without_ssao_reports_unsupported_and_names_the_symbol(mock):  # noqa: F811
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    s = hip_backend.AwsmSsao(20, 0.5, 1.0, 0.02, 1.0)
    assert r.host.lib.awsm_host_set_ssao(r.host.h, C.byref(s)) == -6                        # AWSM_ERR_UNSUPPORTED
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_set_ssao"):
        r.host.set_ssao(False)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_ssao_defaults"):
        r.host.set_ssao(True)
    r.render()                                                                              # and renders as before
    r.close()
