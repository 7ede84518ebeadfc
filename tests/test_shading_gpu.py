"""The shade kernels on the scenes of tests/shading_cases.py, through the C-ABI, against the float64 restatement of the WGSL
(tests/shading_reference.py) — so that the test stands even if oracle and kernels share a mistake.  Every case runs on every device route that can
take it, one HipDevice per route:

    lean       the default (`k_shade_lean` where the material allows it)          general    HipDevice(general_shade_only=True): `k_shade`
    msaa4      msaa=4: `k_shade_msaa` and the edge resolve                          mips       mipmap=True: gradient mips
    transparent   the transparent cases through `k_forward_shade` / `k_forward_blend`: the composite within 2 f16 steps

Colour bound: 1e-4 * max(1, |ref|) + SHADE_REL_TOL * max(1, |ref|) — the project's bar plus the tolerance measured on the CPU between
oracle and restatement, by the triangle inequality; nothing is measured on the GPU to set it.  The G-buffer texel's six f16 halves are exact, alpha
is exact.  The worst device-to-restatement distance per route is printed (pytest -s shows it): a measurement, not a bar."""
import numpy as np
import pytest

from tests import helpers
from tests import shading_cases as cases
from tests import shading_reference as sr

pytestmark = pytest.mark.gpu

RGB_BAR = 1e-4
ROUTES = {"lean": {}, "general": {}, "msaa4": {"msaa": 4}, "mips": {"mipmap": True}}


def takes(route, case) -> bool:
    if route == "msaa4":
        return not case.get("mipmap")
    if route == "mips":
        return not case.get("msaa")
    return not case.get("msaa") and not case.get("mipmap")


PAIRS = [(r, n) for r in ROUTES for n, c in cases.CASES.items() if takes(r, c)]
_models, _worst, _forward_steps = {}, {}, {}


def _model(name):
    if name not in _models:
        _models[name] = helpers.build_model(cases.CASES[name]["scene"]())
    return _models[name]


def restated(route, name, lut):
    """{pixel: the restatement's result} for a case as the route renders it (no GPU involved)"""
    case, model = cases.CASES[name], _model(name)
    rst = sr.Restatement(model, lut, mip_chains=helpers.mip_chain_levels(model.scene) if route == "mips" else None)
    pixels = case.get("pixels", cases.PIXELS)
    out = {xy: (rst.pixel_msaa4(*xy) if route == "msaa4" else rst.pixel(*xy)) for xy in pixels}
    for xy, p in out.items():      # the conditions that make the comparison meaningful on this route too
        mg = p["margins"]
        edge = 0.0005 if case.get("border") else cases.EDGE_MARGIN
        assert mg.f16 >= cases.F16_MARGIN and mg.snap >= cases.SNAP_MARGIN and mg.edge >= edge, (route, name, xy, mg.f16, mg.snap, mg.edge)
        assert p["record"].get("nearest_margin", 1.0) >= cases.NEAREST_MARGIN, (route, name, xy)
        if route == "msaa4":
            assert (len(set(p["ranks"])) > 1) == bool(case.get("border")), (route, name, xy, p["ranks"])
    return out


@pytest.fixture(scope="module")
def devices():
    """one HipDevice per route, reused across the cases"""
    from awsm_renderer_amd.hip_backend import HipDevice
    devs = {r: HipDevice(parity_tap=True, general_shade_only=(r == "general")) for r in ROUTES}
    yield devs
    for d in devs.values():
        d.close()
    lines = ["%-8s cases=%d worst_colour_rel=%.3e (%s)" % (r, w[2], w[0], w[1]) for r, w in _worst.items()]
    print("\n".join(lines))


@pytest.mark.parametrize("route,name", PAIRS)
def test_case_on_route_agrees_with_the_restatement(route, name, devices, oracle_lut):
    case, model = cases.CASES[name], _model(name)
    ref = restated(route, name, oracle_lut)
    dev, stats = helpers.hip_frame(model, oracle_lut, dev=devices[route], **ROUTES[route])
    f32 = dev.read_opaque_f32().astype(np.float64)
    gbuf = dev.read_gbuffer().astype(np.float64) if route != "msaa4" else None
    if route == "lean" and case["lean"] is not None:      # the route itself: plain PBR stays on the lean kernel, an extension leaves it
        assert (stats["shade_general_wavefronts"] == 0) == case["lean"], (name, stats["shade_general_wavefronts"])
    worst = 0.0
    for (x, y), p in ref.items():
        want, got = p["color"], f32[y, x]
        assert np.isfinite(got).all(), (route, name, x, y)
        scale = np.maximum(1.0, np.abs(want))
        d = np.abs(got[:3] - want)
        print("%-8s %-28s (%2d, %2d) colour_rel=%.3e" % (route, name, x, y, float((d / scale).max())))
        worst = max(worst, float((d / scale).max()))
        assert (d <= RGB_BAR * scale + sr.SHADE_REL_TOL * scale).all(), (route, name, (x, y), got[:3], want)
        assert got[3] == p["alpha"], (route, name, (x, y), got[3])
        if gbuf is not None:
            assert np.array_equal(gbuf[y, x], p["gbuffer"]["halves"]), (route, name, (x, y), gbuf[y, x], p["gbuffer"]["halves"])
    w = _worst.get(route, (0.0, None, 0))
    _worst[route] = (max(w[0], worst), name if worst >= w[0] else w[1], w[2] + 1)


@pytest.fixture(scope="module")
def forward_device():
    from awsm_renderer_amd.hip_backend import HipDevice
    dev = HipDevice(parity_tap=True)
    yield dev
    dev.close()
    line = "transparent cases=%d worst_f16_steps=%d (%s)" % (len(_forward_steps), max(_forward_steps.values(), default=0),
                                                            max(_forward_steps, key=_forward_steps.get, default=None))
    print(line)


@pytest.mark.parametrize("name", list(cases.FORWARD_CASES))
def test_transparent_case_agrees_with_the_restatement(name, forward_device, oracle_lut):
    """the composite image (RGBA16F) against the restatement's value rounded to f16: within the 2 f16 steps DESIGN §2 allows a composite"""
    case = cases.FORWARD_CASES[name]
    model = helpers.build_model(case["scene"]())
    rst = sr.Restatement(model, oracle_lut)
    dev, stats = helpers.hip_frame(model, oracle_lut, dev=forward_device, transparent=True)
    h16 = dev.read_composite()
    assert stats["forward_triangles"] == 2
    for (x, y) in cases.PIXELS:
        p = rst.pixel_forward(x, y, cases.BACKDROP)
        cases.check_forward_pixel(name, case, rst, p)
        steps = helpers.f16_ulp_distance(h16[y, x], np.asarray(p["composite"], dtype=np.float16).view(np.uint16))
        print("transparent %-26s (%2d, %2d) f16 steps=%s" % (name, x, y, steps))
        _forward_steps[name] = max(_forward_steps.get(name, 0), int(steps.max()))
        assert steps.max() <= 2, (name, (x, y), steps, h16[y, x].view(np.float16), p["composite"])
