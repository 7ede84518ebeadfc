"""CPU tests of the animation players and samplers (host/animation.hpp through the C API, over the mock backend) against the float64
restatement of the reference's Rust in tests/animation_reference.py.  Players are compared exactly; sampled values exactly where no
arithmetic happens (step, exact hits, after-last, one key) and at the measured tolerances elsewhere.  One test each pins the quirks kept."""
import math
import os
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from tests import animation_reference as R

MOCK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mock")
MOCK = os.path.join(MOCK_DIR, "libmock_backend.so")
I3, Q1 = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def host():
    src = os.path.join(MOCK_DIR, "mock_backend.c")
    if not os.path.exists(MOCK) or os.path.getmtime(src) > os.path.getmtime(MOCK):
        subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", MOCK, src])
    h = H.Host(backend_path=MOCK)
    yield h
    h.close()


@pytest.fixture()
def node(host):
    return host.transform_insert((0, 0, 0), Q1, I3)


# ------------------------------------------------------------------------------------------------ players: exact
def _script(host, node, duration, loop_style, direction, steps, start=None, speed=None, paused_at=()):
    """The same scripted updates on the C++ player and on the restatement; yields both states after every step."""
    times = [0.0, duration] if duration > 0 else [0.0, 1.0]
    key = host.animation_insert_transform(node, "translation", times, [[0, 0, 0], [1, 2, 3]], duration=duration)
    ref = R.Player(duration)
    st = host.animation_state(key)
    assert (st["speed"], st["loop_style"], st["direction"], st["state"], st["local_time"]) == (1.0 / 1000.0, R.LOOP, R.FORWARD, R.PLAYING, 0.0)   # player.rs:41-50
    host.animation_set_playback(key, speed=speed, loop_style=loop_style, direction=direction)
    ref.loop_style, ref.direction = loop_style, direction
    if speed is not None:
        ref.speed = speed
    if start is not None:
        host.animation_seek(key, start)
        ref.local_time = start
    out = []
    for i, dt in enumerate(steps):
        if i in paused_at:
            host.animation_set_playback(key, state=R.PAUSED)
            ref.state = R.PAUSED
        host.update_animations(dt)
        ref.update(dt)
        st = host.animation_state(key)
        out.append(((st["local_time"], st["direction"], st["state"]), (ref.local_time, ref.direction, ref.state)))
    host.animation_remove(key)
    return out


STEPS = [130.0, 270.5, 333.25, 90.0, 4310.0, 77.7, 1000.0, 0.0, 512.125, 3999.9]      # in ms at the default speed: one overshoots a 1.3 s clip by several durations


@pytest.mark.parametrize("direction", [R.FORWARD, R.BACKWARD])
@pytest.mark.parametrize("loop_style", [R.LOOP, R.PING_PONG, R.LOOP_NONE])
def test_player_matches_the_restatement_exactly(host, node, loop_style, direction):
    start = 0.9 if direction == R.BACKWARD else None
    for got, want in _script(host, node, 1.3, loop_style, direction, STEPS, start=start):
        assert got == want


def test_player_step_that_overshoots_by_several_durations(host, node):
    (got, want), = _script(host, node, 1.0, R.LOOP, R.FORWARD, [7350.0])
    assert got == want == (R.rem_euclid(7350.0 * (1.0 / 1000.0), 1.0), R.FORWARD, R.PLAYING)
    assert 0.34 < got[0] < 0.36


def test_pin_backward_loop_lands_mirrored(host, node):
    """player.rs:85-86: duration - rem_euclid(local_time, duration).  -0.1 of a 1.0 clip lands at 0.1, not at 0.9."""
    (got, want), = _script(host, node, 1.0, R.LOOP, R.BACKWARD, [1.0], start=0.4, speed=0.5)      # 0.4 - 0.5 = -0.1 (0.5 and 0.4 - 0.5 are exact enough: compare with the f64 expression)
    assert got == want
    assert got[0] == 1.0 - R.rem_euclid(0.4 - 0.5, 1.0)
    assert abs(got[0] - 0.1) < 1e-12 and got[1] == R.BACKWARD


def test_player_ping_pong_turns_at_both_ends(host, node):
    res = _script(host, node, 1.0, R.PING_PONG, R.FORWARD, [600.0, 600.0, 700.0, 700.0, 100.0])
    assert all(g == w for g, w in res)
    got = [g for g, _ in res]
    assert got[1] == (1.0, R.BACKWARD, R.PLAYING)      # clamped to the end it hit, direction flipped
    assert got[3] == (0.0, R.FORWARD, R.PLAYING)
    assert got[4][1] == R.FORWARD and got[4][0] == 100.0 * (1.0 / 1000.0)


def test_player_none_clamps_and_ends_and_then_stays(host, node):
    res = _script(host, node, 1.0, R.LOOP_NONE, R.FORWARD, [900.0, 900.0, 500.0])
    assert all(g == w for g, w in res)
    assert res[1][0] == (1.0, R.FORWARD, R.ENDED) and res[2][0] == (1.0, R.FORWARD, R.ENDED)
    res = _script(host, node, 1.0, R.LOOP_NONE, R.BACKWARD, [900.0, 500.0], start=0.5)
    assert all(g == w for g, w in res)
    assert res[0][0] == (0.0, R.BACKWARD, R.ENDED)


def test_player_paused_does_not_move(host, node):
    res = _script(host, node, 1.0, R.LOOP, R.FORWARD, [250.0, 250.0, 250.0], paused_at=(1,))
    assert all(g == w for g, w in res)
    assert res[0][0][0] == res[1][0][0] == res[2][0][0] == 0.25 and res[2][0][2] == R.PAUSED


@pytest.mark.parametrize("duration", [0.0, -1.0, float("nan")])
def test_player_with_a_duration_that_is_not_positive_never_advances(host, node, duration):
    """Deviation: rem_euclid(x, 0) is NaN in the reference."""
    res = _script(host, node, duration, R.LOOP, R.FORWARD, [500.0, 500.0])
    assert all(g[0] == 0.0 and g[2] == R.PLAYING for g, _ in res)
    assert all(g == w for g, w in res)


# ------------------------------------------------------------------------------------------------ samplers
def _unit(q):
    q = np.asarray(q, np.float64)
    return (q / np.linalg.norm(q)).astype(np.float32)


RNG = np.random.default_rng(20240607)
TIMES = [0.0, 0.25, 0.75, 1.5, 1.75]
AT = [0.1, 0.2499, 0.5, 0.74, 1.0, 1.49, 1.6, 1.7499999]      # strictly between keys


def _quat_keys():
    """Five unit quaternions whose neighbours have |dot| in [0.05, 0.99]; pair (1, 2) has dot < 0; asserted in f64."""
    while True:
        qs = [_unit(RNG.normal(size=4)) for _ in TIMES]
        dots = [float(qs[i].astype(np.float64) @ qs[i + 1].astype(np.float64)) for i in range(len(qs) - 1)]
        if dots[1] > 0:
            qs[2] = -qs[2]
            dots = [float(qs[i].astype(np.float64) @ qs[i + 1].astype(np.float64)) for i in range(len(qs) - 1)]
        if all(0.05 <= abs(d) <= 0.99 for d in dots) and dots[1] < 0:
            return np.array(qs, np.float32), dots


QUATS, QUAT_DOTS = _quat_keys()
VEC3S = (RNG.normal(size=(len(TIMES), 3)) * np.array([1.0, 10.0, 0.1])).astype(np.float32)
WEIGHTS = RNG.uniform(-0.5, 1.5, size=(len(TIMES), 5)).astype(np.float32)
TAN = {"rotation": (RNG.normal(size=(len(TIMES), 4)) * 0.5).astype(np.float32), "translation": RNG.normal(size=(len(TIMES), 3)).astype(np.float32),
       "weights": RNG.normal(size=(len(TIMES), 5)).astype(np.float32)}
TAN_OUT = {k: (v * -0.7 + 0.1).astype(np.float32) for k, v in TAN.items()}
VALUES = {"rotation": QUATS, "translation": VEC3S, "scale": VEC3S, "weights": WEIGHTS}


@pytest.fixture(scope="module")
def morph_mesh(host):
    """A mesh with five morph targets over the mock, for weights clips."""
    from awsm_renderer_amd.scene_desc import MaterialDesc, PrimitiveDesc
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    prim = PrimitiveDesc(positions=pos, normals=np.tile(np.array([[0, 0, 1]], np.float32), (3, 1)), indices=np.array([[0, 1, 2]], np.uint32),
                     morph_targets=[{"positions": pos * 0.1 * (k + 1)} for k in range(5)], morph_weights=np.zeros(5, np.float32))
    t = host.transform_insert((0, 0, 0), Q1, I3)
    m = host.material_insert(H.material_struct(MaterialDesc(), host, {}))
    return host.mesh_insert(prim, t, m)


def _insert(host, node, morph_mesh, path, interpolation, times=TIMES, values=None, in_t=None, out_t=None):
    values = VALUES[path] if values is None else values
    if interpolation == "cubic":
        tk = "translation" if path == "scale" else path
        in_t = TAN[tk] if in_t is None else in_t
        out_t = TAN_OUT[tk] if out_t is None else out_t
    if path == "weights":
        return host.animation_insert_morph(morph_mesh, times, values, interpolation, in_t, out_t), values, in_t, out_t
    return host.animation_insert_transform(node, path, times, values, interpolation, in_t, out_t), values, in_t, out_t


def _sample_at(host, key, t):
    host.animation_seek(key, t)
    return host.animation_sample(key)


def _distance(path, got, want):
    d = float(np.max(np.abs(got.astype(np.float64) - want)))
    return d / float(np.max(np.abs(want))) if path in ("translation", "scale") else d


def _tol(path):
    return {"rotation": R.TOL_QUAT_ABS, "weights": R.TOL_WEIGHTS_ABS}.get(path, R.TOL_VEC3_REL)


def test_sampler_case_preconditions():
    assert all(0.05 <= abs(d) <= 0.99 for d in QUAT_DOTS) and QUAT_DOTS[1] < 0 and any(d > 0 for d in QUAT_DOTS)
    assert all(abs(float(np.linalg.norm(q.astype(np.float64))) - 1.0) < 1e-6 for q in QUATS)
    for t in AT:
        assert t not in TIMES and TIMES[0] < t < TIMES[-1]


@pytest.mark.parametrize("path", ["translation", "rotation", "scale", "weights"])
@pytest.mark.parametrize("interpolation", ["linear", "step", "cubic"])
def test_exact_hits_after_last_and_step_are_exact(host, node, morph_mesh, path, interpolation):
    key, values, _, _ = _insert(host, node, morph_mesh, path, interpolation)
    for i, t in enumerate(TIMES):      # an exact hit returns the key, for every interpolation
        assert _sample_at(host, key, t).tobytes() == values[i].tobytes()
    assert _sample_at(host, key, 99.0).tobytes() == values[-1].tobytes()      # past the last key: the last key
    if interpolation == "step":
        for t in AT:
            left = max(i for i, k in enumerate(TIMES) if k < t)
            assert _sample_at(host, key, t).tobytes() == values[left].tobytes()
    host.animation_remove(key)


@pytest.mark.parametrize("path", ["translation", "rotation", "weights"])
@pytest.mark.parametrize("interpolation", ["linear", "step", "cubic"])
def test_one_key_sampler_returns_its_key_for_any_time(host, node, morph_mesh, path, interpolation):
    """Deviation: Between(0, 1) of a one-key sampler indexes past the end in the reference."""
    v = VALUES[path][:1]
    tan = TAN["translation" if path == "scale" else path][:1]
    key, _, _, _ = _insert(host, node, morph_mesh, path, interpolation, times=[0.5], values=v, in_t=tan, out_t=tan)
    for t in (-1.0, 0.0, 0.5, 3.0):
        assert _sample_at(host, key, t).tobytes() == v[0].tobytes()
    host.animation_remove(key)


@pytest.mark.parametrize("path", ["translation", "rotation", "scale", "weights"])
@pytest.mark.parametrize("interpolation", ["linear", "cubic"])
def test_interpolated_values_match_the_restatement(host, node, morph_mesh, path, interpolation):
    key, values, in_t, out_t = _insert(host, node, morph_mesh, path, interpolation)
    worst = 0.0
    for t in AT:
        got = _sample_at(host, key, t)
        want = R.sample(path, interpolation, TIMES, values, t, in_t, out_t)
        worst = max(worst, _distance(path, got, want))
    print(f"animation sampler {path}/{interpolation}: worst distance {worst:.3e} (tolerance {_tol(path):.3e})")
    assert worst <= _tol(path)
    host.animation_remove(key)


def test_before_the_first_key_extrapolates_keys_0_and_1(host, node):
    """sampler.rs:126-127: Between(0, 1) with a negative factor."""
    times = [1.0, 2.0, 3.0]
    v = np.array([[1, 2, 3], [3, 6, 9], [0, 0, 0]], np.float32)
    key = host.animation_insert_transform(node, "translation", times, v)
    got = _sample_at(host, key, 0.5)      # factor -0.5, exact in f32: 1 + (3 - 1) * -0.5 = 0
    assert got.tobytes() == np.array([0, 0, 0], np.float32).tobytes()
    assert got.tobytes() == R.sample("translation", "linear", times, v, 0.5).astype(np.float32).tobytes()
    host.animation_remove(key)
    key = host.animation_insert_transform(node, "translation", times, v, "step")
    assert _sample_at(host, key, 0.5).tobytes() == v[0].tobytes()      # step: the left key, which is key 0
    host.animation_remove(key)


def test_pin_a_clip_whose_first_key_is_at_one_is_sampled_over_the_wrong_window(host, node):
    """duration = last - first (populate/animation.rs:107,229) while local_time runs over [0, duration]: keys at 1.0 and 3.0 are played over
    [0, 2], so the first half extrapolates backwards and key 3.0 is never reached.  As in the reference."""
    times = [1.0, 3.0]
    v = np.array([[0, 0, 0], [2, 4, 8]], np.float32)
    key = host.animation_insert_transform(node, "translation", times, v)      # duration defaults to last - first
    assert host.animation_state(key)["duration"] == 2.0
    host.update_animations(500.0)      # local time 0.5: factor (0.5 - 1) / 2 = -0.25
    assert host.animation_state(key)["local_time"] == 0.5
    assert host.animation_sample(key).tobytes() == np.array([-0.5, -1.0, -2.0], np.float32).tobytes()
    assert host.transform_get_local(node)[0].tobytes() == np.array([-0.5, -1.0, -2.0], np.float32).tobytes()      # ... and applied
    host.update_animations(1499.0)      # local time 1.999: still short of key 3.0's value
    assert host.animation_sample(key)[0] < 1.0
    host.animation_remove(key)


def test_pin_cubic_uses_out_tangent_of_the_left_key_and_in_tangent_of_the_right(host, node):
    """sampler.rs:96-97.  With values 0 the result is h10 * out[left] * dt + h11 * in[right] * dt: at t = 0.5, dt = 1 that is (out[left] - in[right]) / 8."""
    times = [0.0, 1.0]
    z = np.zeros((2, 3), np.float32)
    in_t = np.array([[100, 100, 100], [8, 16, 24]], np.float32)        # in[left] must not be read
    out_t = np.array([[80, 40, 16], [-100, -100, -100]], np.float32)   # out[right] must not be read
    key = host.animation_insert_transform(node, "translation", times, z, "cubic", in_t, out_t)
    got = _sample_at(host, key, 0.5)
    assert got.tobytes() == np.array([(80 - 8) / 8, (40 - 16) / 8, (16 - 24) / 8], np.float32).tobytes()
    host.animation_remove(key)


def test_slerp_branches(host, node):
    """An identical pair takes the lerp branch and returns the key; a pair with dot < 0 goes the short way (the hemisphere flip)."""
    q = _unit([0.1, 0.7, -0.2, 0.6])
    key = host.animation_insert_transform(node, "rotation", [0.0, 1.0], np.array([q, q]))
    assert float(q.astype(np.float64) @ q.astype(np.float64)) > 1.0 - R.FLT_EPSILON
    got = _sample_at(host, key, 0.3)
    d0 = float(np.max(np.abs(got.astype(np.float64) - R.sample("rotation", "linear", [0.0, 1.0], np.array([q, q]), 0.3))))
    assert d0 <= R.TOL_QUAT_ABS
    assert got.tobytes() == q.tobytes()      # a + (a - a) t
    host.animation_remove(key)
    a, b = _unit([0, 0, 0, 1]), _unit([0, 0, -math.sin(0.4), -math.cos(0.4)])      # b is the rotation by 0.8 rad about z, negated: dot < 0
    assert float(a.astype(np.float64) @ b.astype(np.float64)) < -0.05
    key = host.animation_insert_transform(node, "rotation", [0.0, 1.0], np.array([a, b]))
    got = _sample_at(host, key, 0.5).astype(np.float64)
    d1 = float(np.max(np.abs(got - R.sample("rotation", "linear", [0.0, 1.0], np.array([a, b]), 0.5))))
    print(f"animation sampler slerp branches: distances {d0:.3e} (lerp), {d1:.3e} (dot < 0); tolerance {R.TOL_QUAT_ABS:.3e}")
    assert d1 <= R.TOL_QUAT_ABS
    assert np.max(np.abs(got - np.array([0, 0, math.sin(0.2), math.cos(0.2)]))) <= 1e-6      # half way along the SHORT arc (0.4 rad about z; the keys are f32)
    host.animation_remove(key)


def test_cubic_quaternion_flips_value_and_tangent_and_normalises(host, node):
    a, b = _unit([0, 0, 0, 1]), _unit([0, 0, -math.sin(0.4), -math.cos(0.4)])
    in_t = np.array([[0, 0, 0, 0], [0.3, -0.2, 0.5, 0.1]], np.float32)
    out_t = np.array([[-0.4, 0.2, 0.1, 0.3], [0, 0, 0, 0]], np.float32)
    key = host.animation_insert_transform(node, "rotation", [0.0, 2.0], np.array([a, b]), "cubic", in_t, out_t)
    got = _sample_at(host, key, 0.7).astype(np.float64)
    want = R.sample("rotation", "cubic", [0.0, 2.0], np.array([a, b]), 0.7, in_t, out_t)
    print(f"animation sampler cubic quaternion with dot < 0: distance {float(np.max(np.abs(got - want))):.3e}; tolerance {R.TOL_QUAT_ABS:.3e}")
    assert np.max(np.abs(got - want)) <= R.TOL_QUAT_ABS
    assert abs(np.linalg.norm(got) - 1.0) < 1e-6 and got[3] > 0.5      # normalised, and on a's hemisphere
    host.animation_remove(key)


def test_the_factor_is_taken_in_f64(host, node):
    """(time - left) / (right - left) in f64, cast to f32 once: with keys near 1e7 an f32 subtraction would lose the whole fraction."""
    times = [1.0e7, 1.0e7 + 1.0]
    v = np.array([[0, 0, 0], [64, 128, 256]], np.float32)
    key = host.animation_insert_transform(node, "translation", times, v)
    got = _sample_at(host, key, 1.0e7 + 0.3)      # np.float32(1e7 + 0.3) == 1e7: an f32 factor would be 0
    want = R.sample("translation", "linear", times, v, 1.0e7 + 0.3)
    print(f"animation sampler f64 factor: distance {_distance('translation', got, want):.3e}; tolerance {R.TOL_VEC3_REL:.3e}")
    assert _distance("translation", got, want) <= R.TOL_VEC3_REL
    assert got[0] > 19.0
    host.animation_remove(key)


# ------------------------------------------------------------------------------------------------ what insert refuses
def test_insert_refuses_what_the_reference_panics_on(host, node, morph_mesh):
    with pytest.raises(H.HostError):      # no keys
        host.animation_insert_transform(node, "translation", [], np.zeros((0, 3), np.float32))
    with pytest.raises(H.HostError):      # width mismatch: a rotation of three floats
        host.animation_insert_transform(node, "rotation", [0.0, 1.0], np.zeros((2, 3), np.float32))
    with pytest.raises(H.HostError):      # width mismatch: four weights for five targets
        host.animation_insert_morph(morph_mesh, [0.0, 1.0], np.zeros((2, 4), np.float32))
    with pytest.raises(H.HostError):      # a cubic clip without tangents
        host.animation_insert_transform(node, "translation", [0.0, 1.0], np.zeros((2, 3), np.float32), "cubic")
    with pytest.raises(H.HostError):      # an unknown target
        host.animation_insert_transform(0xDEAD00000001, "translation", [0.0, 1.0], np.zeros((2, 3), np.float32))
    with pytest.raises(H.HostError):
        host.animation_remove(0xDEAD00000001)


def test_update_animations_order_and_apply(host, morph_mesh):
    """animations.rs:84-141: all players advance, transform players apply in key order (the later key wins on one component), then morph players."""
    n = host.transform_insert((5, 6, 7), _unit([0.5, 0.5, 0.5, 0.5]), (2, 2, 2))
    k1 = host.animation_insert_transform(n, "translation", [0.0, 1.0], [[0, 0, 0], [10, 0, 0]])
    k2 = host.animation_insert_transform(n, "translation", [0.0, 1.0], [[0, 0, 0], [0, 10, 0]])
    k3 = host.animation_insert_morph(morph_mesh, [0.0, 1.0], [[0] * 5, [1, 2, 3, 4, 5]])
    host.update_animations(500.0)
    t, r, s = host.transform_get_local(n)
    assert t.tobytes() == np.array([0, 5, 0], np.float32).tobytes()      # k2 ran after k1; only the animated component changed
    assert r.tobytes() == _unit([0.5, 0.5, 0.5, 0.5]).tobytes() and s.tobytes() == np.array([2, 2, 2], np.float32).tobytes()
    assert host.animation_sample(k3).tobytes() == np.array([0.5, 1.0, 1.5, 2.0, 2.5], np.float32).tobytes()
    for k in (k1, k2, k3):
        host.animation_remove(k)


def test_tolerances_are_four_times_the_measured_distance():
    assert R.TOL_QUAT_ABS == 4 * R.MEASURED_QUAT_ABS and R.TOL_WEIGHTS_ABS == 4 * R.MEASURED_WEIGHTS_ABS and R.TOL_VEC3_REL == 4 * R.MEASURED_VEC3_REL
