"""The lean opaque kernel's deferred light window (lean_core: the BRDF table's texels are issued behind the surface terms and consumed behind the
first kLeanDeferredLights = 2 lights' arithmetic; the lights' terms wait in registers and are accumulated afterwards in light order, nothing for a
light the wavefront skipped).

A 64 x 32 Box frame — a handful of 16 x 4 strips, every one on the lean route — under the first 0, 1, 2, 3, 4, 5 and 7 lights of LIGHTS: below, at and
beyond the window (and at and beyond a window of four, the atrium's count).  The list mixes what the window has to get right: a directional light
behind every visible face (skipped by whole wavefronts), a narrow spot that lights part of the top face (a strip half inside its cone), a point
light far outside its range, a spot whose cone misses, and plainly lit ones.  Each count is compared with the oracle at the parity tests' bar, single-sampled, with MipmapMode::Gradient (the gradient
instantiation) and with MSAA x4 (k_shade_msaa_resolve runs lean_core per (pixel, sample) item); and the lean route is compared with the general one,
which this window does not touch.  (FrameDev.lights_cap is the capacity of the per-frame light table, which the library sizes itself: it cannot be
forced below seven from here.)"""
import copy

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from tests import helpers

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4          # tests/test_gpu_parity.py
W, H = 64, 32
COUNTS = (0, 1, 2, 3, 4, 5, 7)
MODES = {"single": {}, "mips": {"mipmap": True}, "msaa4": {"msaa": 4}}

# the camera sits at (1.6, 1.2, 2.2) and sees the faces +x, +y, +z of the unit cube at the origin
LIGHTS = [
    # travels along (+1, +1, +1): n.l < 0 on all three visible faces — every wavefront skips it
    {"kind": "directional", "color": (1.0, 1.0, 1.0), "intensity": 3.0, "direction": (1.0, 1.0, 1.0)},
    # a narrow cone straight down onto one corner of the top face: strips of that face are half inside it, the other faces see it edge-on or not at all
    {"kind": "spot", "color": (0.9, 1.0, 0.8), "intensity": 40.0, "position": (0.3, 2.0, 0.3), "direction": (0.0, -1.0, 0.0), "range": 20.0,
     "inner_angle": 0.995, "outer_angle": 0.985},
    # far outside its range.  (The reference's inverse_square has no cut-off: saturate((1 - d^2 / r^2)^2) is 1 again far out, so this light is NOT a
    # skip — it adds a faint term, 8e-3 at the most, to every face it reaches; test_the_lights_do_what_the_cases_need says so.)
    {"kind": "point", "color": (1.0, 0.7, 0.5), "intensity": 50.0, "position": (0.0, 0.0, 40.0), "range": 2.0},
    scenes.DEFAULT_LIGHTS[0],
    # in range, but the cone points away from the box
    {"kind": "spot", "color": (0.5, 0.7, 1.0), "intensity": 40.0, "position": (0.0, 3.0, 0.0), "direction": (0.0, 1.0, 0.0), "range": 20.0,
     "inner_angle": 0.98, "outer_angle": 0.90},
    scenes.DEFAULT_LIGHTS[3],
    {"kind": "point", "color": (0.6, 0.8, 1.0), "intensity": 6.0, "position": (2.0, 1.0, 1.0), "range": 0.0},
]

# max |lean - general| over the frame's colour channels per (mode, count), measured on the commit before the window existed (same scenes, same
# library otherwise).  On these frames the window changes no word of the lean route's f32 image, so the figures still hold exactly; they are the bar.
PARENT_ROUTE_DIFF = {
    "single": {0: 5.960464477539063e-08, 1: 5.960464477539063e-08, 2: 0.00011217594146728516, 3: 0.00011217594146728516, 4: 0.00011217594146728516, 5: 0.00011217594146728516,
               7: 0.00011229515075683594},
    "mips": {0: 5.960464477539063e-08, 1: 5.960464477539063e-08, 2: 0.00011217594146728516, 3: 0.00011217594146728516, 4: 0.00011217594146728516, 5: 0.00011217594146728516,
             7: 0.00011229515075683594},
    "msaa4": {0: 5.960464477539063e-08, 1: 5.960464477539063e-08, 2: 3.647804260253906e-05, 3: 3.647804260253906e-05, 4: 3.6716461181640625e-05, 5: 3.6716461181640625e-05,
              7: 3.635883331298828e-05},
}


def _scene(n_lights):
    sc = scenes.box_scene(W, H)
    sc.lights = copy.deepcopy(LIGHTS[:n_lights])
    return sc


@pytest.fixture(scope="module")
def models():
    return {n: helpers.build_model(_scene(n)) for n in COUNTS}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_lights", COUNTS)
def test_deferred_window_against_the_oracle(n_lights, mode, models, oracle_lut):
    model = models[n_lights]
    orc = helpers.oracle_frame(model, oracle_lut, **MODES[mode])
    dev, stats = helpers.hip_frame(model, oracle_lut, **MODES[mode])
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    dev.close()
    print(n_lights, mode, r)
    assert stats["shade_general_wavefronts"] == 0, stats          # the lean route shaded the frame
    assert r["covered"] > 0 and r["key_mismatch"] == 0 and r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0, r
    assert r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r


def test_the_lights_do_what_the_cases_need(models, oracle_lut):
    """The list is only worth its cases if the lights behave as labelled — on the oracle: the light from behind, the out-of-range point... add what the
    oracle says they add, and the narrow spot changes part of the top face and not all of it."""
    img = {n: helpers.oracle_frame(models[n], oracle_lut).rgba32f[..., :3].astype(np.float64) for n in (0, 1, 2, 3, 4, 5)}
    assert (img[1] == img[0]).all()                               # the light from behind adds nothing anywhere
    assert (img[5] == img[4]).all()                               # nor does the spot whose cone points away
    far = np.abs(img[3] - img[2])
    assert 0.0 < far.max() < 1e-2                                 # the far point light: no cut-off in inverse_square, a faint term and not a skip
    lit = (img[2] != img[1]).any(axis=-1)
    rows = lit.reshape(H // 4, 4, W // 16, 16).transpose(0, 2, 1, 3).reshape(-1, 64)      # per 16 x 4 strip
    part = (rows.any(axis=1) & ~rows.all(axis=1)).sum()
    assert part > 0, "no strip is partly inside the spot's cone"


@pytest.mark.parametrize("mode", list(MODES))
def test_lean_and_general_routes_differ_no_more_than_before(mode, models, oracle_lut):
    from awsm_renderer_amd.hip_backend import HipDevice
    for n in COUNTS:
        lean, st = helpers.hip_frame(models[n], oracle_lut, **MODES[mode])
        gen, st_gen = helpers.hip_frame(models[n], oracle_lut, dev=HipDevice(parity_tap=True, general_shade_only=True), **MODES[mode])
        a, b = lean.read_opaque_f32().astype(np.float64), gen.read_opaque_f32().astype(np.float64)
        same_keys = bool((lean.read_visibility() == gen.read_visibility()).all())
        lean.close(); gen.close()
        d = float(np.abs(a[..., :3] - b[..., :3]).max())
        print("route difference", mode, n, repr(d))
        assert same_keys and st["shade_general_wavefronts"] == 0, (mode, n, st)
        assert d <= PARENT_ROUTE_DIFF[mode][n], (mode, n, d, PARENT_ROUTE_DIFF[mode][n])
