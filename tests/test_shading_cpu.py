"""The shading stage on the CPU: the C oracle (`oracle_shade.c`, f32) against the float64 restatement written from the WGSL and the scene
description alone (tests/shading_reference.py), at the centre and four off-axis pixels of one small scene per branch (tests/shading_cases.py).
No GPU; tests/test_shading_gpu.py holds the kernels to the same two parties."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_lib
from tests import helpers
from tests import shading_cases as cases
from tests import shading_reference as sr

LUT_SIZE = 64
_cache = {}
_lut = []


def lut():
    if not _lut:
        _lut.append(oracle_lib.brdf_lut(LUT_SIZE, LUT_SIZE))
    return _lut[0]


def restatement(name, model=None):
    case = cases.CASES[name]
    model = model or helpers.build_model(case["scene"]())
    return sr.Restatement(model, lut(), mip_chains=helpers.mip_chain_levels(model.scene) if case.get("mipmap") else None)


def restated_pixels(name, rst):
    case = cases.CASES[name]
    return {xy: (rst.pixel_msaa4(*xy) if case.get("msaa") else rst.pixel(*xy)) for xy in case.get("pixels", cases.PIXELS)}


def prepared(name):
    """(case, model, oracle frame, its G-buffer texels, restatement, {pixel: restated result}) — computed once per case"""
    if name not in _cache:
        case = cases.CASES[name]
        model = helpers.build_model(case["scene"]())
        orc = helpers.oracle_frame(model, lut(), msaa=4 if case.get("msaa") else 0, mipmap=bool(case.get("mipmap")))
        rst = restatement(name, model)
        gbuf = None if case.get("msaa") else orc.gbuffer()      # the oracle exposes its G-buffer texels for single-sampled frames only
        _cache[name] = (case, model, orc, gbuf, rst, restated_pixels(name, rst))
    return _cache[name]


def oracle_bary(orc, rank, x, y):
    """the oracle's unrounded barycentrics of a pixel centre on triangle `rank`"""
    L = oracle_lib.lib()
    out = np.zeros(3, dtype=np.float32)
    v = np.ascontiguousarray(orc.clip[rank * 3: rank * 3 + 3])
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    assert L.oracle_tri_bary_at(p(v[0:1]), p(v[1:2]), p(v[2:3]), C.c_uint32(orc.width), C.c_uint32(orc.height), C.c_int(x), C.c_int(y), p(out))
    return out.astype(np.float64)


def distances(name):
    """[(pixel, colour distance relative to max(1, |ref|), barycentric distance, G-buffer halves equal, visible triangle equal)]"""
    case, model, orc, gbuf, rst, pixels = prepared(name)
    out = []
    for (x, y), p in pixels.items():
        ref = p["color"]
        got = orc.rgba32f[y, x].astype(np.float64)
        assert np.isfinite(got).all(), (name, x, y)
        colour = float((np.abs(got[:3] - ref) / np.maximum(1.0, np.abs(ref))).max())
        keys = orc.keys[y, x].reshape(-1)
        ranks = [0xFFFFFFFF - int(k & np.uint64(0xFFFFFFFF)) for k in keys]
        same_tri = ranks == (p["ranks"] if case.get("msaa") else [p["rank"]])
        halves = gbuf is None or bool(np.array_equal(gbuf[y, x].astype(np.float64), p["gbuffer"]["halves"]))
        bary = float(np.abs(oracle_bary(orc, ranks[0], x, y)[:2] - p["gbuffer"]["bary"]).max())
        out.append(((x, y), colour, bary, halves, same_tri, float(got[3]), p["alpha"]))
    return out


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_inputs_meet_their_conditions(name):
    case, model, orc, gbuf, rst, pixels = prepared(name)
    assert model.scene.width <= 65 and model.scene.height <= 65
    for p in pixels.values():
        cases.check_pixel(name, case, rst, p)
    cases.check_case(name, case, pixels)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_against_the_restatement(name):
    """Every checked pixel: the colour within SHADE_REL_TOL * max(1, |ref|), alpha and the visible triangle exactly, the G-buffer texel's six f16
    halves exactly, the unrounded barycentrics within BARY_ABS_TOL.  No pixel is excused."""
    for xy, colour, bary, halves, same_tri, alpha, ref_alpha in distances(name):
        assert same_tri and halves, (name, xy, same_tri, halves)
        assert colour <= sr.SHADE_REL_TOL, (name, xy, colour)
        assert bary <= sr.BARY_ABS_TOL, (name, xy, bary)
        assert alpha == ref_alpha, (name, xy, alpha, ref_alpha)


def forward_prepared(name):
    """(case, model, oracle frame after the transparent pass, restatement, {pixel: restated result}) of a transparent case"""
    key = "forward/" + name
    if key not in _cache:
        case = cases.FORWARD_CASES[name]
        model = helpers.build_model(case["scene"]())
        orc = helpers.oracle_frame(model, lut())
        orc.forward(model.collect_transparent_draws())
        rst = sr.Restatement(model, lut())
        _cache[key] = (case, model, orc, rst, {xy: rst.pixel_forward(xy[0], xy[1], cases.BACKDROP) for xy in cases.PIXELS})
    return _cache[key]


@pytest.mark.parametrize("name", list(cases.FORWARD_CASES))
def test_transparent_pass_against_the_restatement(name):
    """The composite after the transparent pass is an RGBA16F image on both sides: the oracle's halves against the restatement's value rounded to
    f16.  The unrounded values differ by no more than SHADE_REL_TOL, far below an f16 step, so the halves may differ by one step where a value sits
    on a rounding boundary and not otherwise: at most 1 step, every channel, alpha included.  (Measured: 0 steps at every pixel.)"""
    case, model, orc, rst, pixels = forward_prepared(name)
    assert len(model.collect_draws()) == 1 and len(model.collect_transparent_draws()) == 1
    opaque = orc.rgba32f[..., :3].astype(np.float64)
    assert int((orc.keys != oracle_lib.NO_HIT_KEY).sum()) >= 2          # the opaque corner quad is there
    for (x, y), p in pixels.items():
        r = int(sr.FORWARD_REACH)
        assert (opaque[max(0, y - r): y + r + 1, max(0, x - r): x + r + 1] == np.asarray(cases.BACKDROP)).all()      # the backdrop, unrounded by RGBA16F
        cases.check_forward_pixel(name, case, rst, p)
        assert orc.fwd_touched[y, x] == 1
        steps = helpers.f16_ulp_distance(orc.composite16f[y, x], np.asarray(p["composite"], dtype=np.float16).view(np.uint16))
        print("%-26s (%2d, %2d) f16 steps=%s" % (name, x, y, steps))
        assert steps.max() <= 1, (name, (x, y), steps, orc.composite32f[y, x], p["composite"])


def test_the_committed_tolerances_are_four_times_the_worst_distance():
    """Prints every case's worst distances (pytest -s shows them): SHADE_REL_TOL and BARY_ABS_TOL are the worst values x 4, as measured when the
    cases were written.  A later reader re-measures here; the tolerances must cover what is seen, and the worst colour distance must stay below
    2.5e-5 so that the tolerance stays below the project's 1e-4 bar (a case that needs more is ill-conditioned: change the case)."""
    worst = {"colour": (0.0, None), "bary": (0.0, None)}
    for name in cases.CASES:
        d = distances(name)
        c, b = max(r[1] for r in d), max(r[2] for r in d)
        print("%-28s pixels=%d colour_rel=%.3e bary_abs=%.3e" % (name, len(d), c, b))
        worst["colour"] = max(worst["colour"], (c, name))
        worst["bary"] = max(worst["bary"], (b, name))
    print("worst oracle-to-restatement distances: colour_rel=%.3e (%s) bary_abs=%.3e (%s)   (committed tolerances: %.3e, %.3e)" % (
        worst["colour"] + worst["bary"] + (sr.SHADE_REL_TOL, sr.BARY_ABS_TOL)))
    assert worst["colour"][0] < sr.WORST_ALLOWED, worst
    assert worst["colour"][0] <= sr.SHADE_REL_TOL and worst["bary"][0] <= sr.BARY_ABS_TOL, worst
    assert sr.SHADE_REL_TOL < 1e-4
    # ... and they are no looser than the rule says: 4 x the worst, with room for a later re-measurement to come out up to half as large
    assert sr.SHADE_REL_TOL <= 8 * worst["colour"][0] and sr.BARY_ABS_TOL <= 8 * worst["bary"][0], worst


def test_the_cases_cover_both_triangles_and_both_sides_of_every_switch():
    """what check_pixel cannot see from one pixel: the set of cases as a whole"""
    ranks = {p["rank"] for p in prepared("plain")[5].values()}
    assert ranks == {0, 1}
    c = cases.CASES
    for a, b in (("clearcoat_0", "clearcoat"), ("sheen_zero", "sheen_one_channel"), ("sheen_below_the_floor", "sheen_one_channel"),
                 ("point_range_0", "point_range"), ("spot_inside", "spot_outside"), ("normal_map_right_handed", "normal_map_left_handed"),
                 ("ior_0_9", "ior_1_33"), ("gradient_mips", "gradient_mips_magnified"), ("msaa_fold_interior", "msaa_border")):
        assert a in c and b in c
    # handedness reaches the image: the two normal-map cases differ by far more than the tolerance
    r = np.array([p["color"] for p in prepared("normal_map_right_handed")[5].values()])
    l = np.array([p["color"] for p in prepared("normal_map_left_handed")[5].values()])
    assert np.abs(r - l).max() > 1000 * sr.SHADE_REL_TOL
