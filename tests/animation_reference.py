"""A float64 restatement of the reference's animation players and samplers, written from the Rust
(crates/renderer/src/animation/{player,sampler,interpolate,data}.rs), not from host/animation.hpp: what
tests/test_animation_cpu.py holds the C++ host layer to.

The player is IEEE f64 on both sides, so its results are compared exactly.  A sampled value is f32 arithmetic in the product and f64 here;
the tolerances below are the project's own way: the worst distance measured between the two over the cases of
tests/test_animation_cpu.py, times four.  Quaternion components and weights are absolute, translation and scale relative to the largest
component of the expected value.
"""
import math

import numpy as np

LOOP_NONE, LOOP, PING_PONG = -1, 0, 1
FORWARD, BACKWARD = 0, 1
PLAYING, PAUSED, ENDED = 0, 1, 2

# The worst C++-to-restatement distance measured over the cases (each test prints its own; rounded up to two digits), and 4x that:
#   quaternion components: 8.788e-08 (cubic; linear 7.423e-08, the dot < 0 pairs 2.9e-08, the lerp branch 0)
#   weights:               1.765e-07 (cubic; linear 1.395e-07)
#   translation / scale:   3.180e-07 of the largest component (linear; cubic 3.138e-07)
MEASURED_QUAT_ABS = 8.8e-8
MEASURED_WEIGHTS_ABS = 1.8e-7
MEASURED_VEC3_REL = 3.2e-7
TOL_QUAT_ABS = 4 * MEASURED_QUAT_ABS
TOL_WEIGHTS_ABS = 4 * MEASURED_WEIGHTS_ABS
TOL_VEC3_REL = 4 * MEASURED_VEC3_REL

FLT_EPSILON = float(np.finfo(np.float32).eps)


def rem_euclid(a: float, b: float) -> float:
    r = math.fmod(a, b)
    return r + abs(b) if r < 0.0 else r


class Player:
    """player.rs:41-100; `duration <= 0 never advances` is this repository's deviation (rem_euclid by 0 is NaN in the reference)."""

    def __init__(self, duration: float):
        self.speed = 1.0 / 1000.0
        self.loop_style = LOOP
        self.direction = FORWARD
        self.state = PLAYING
        self.local_time = 0.0
        self.duration = duration

    def update(self, global_time_delta: float):
        if self.state != PLAYING:
            return
        if not self.duration > 0.0:
            return
        delta = global_time_delta * self.speed
        if self.direction == FORWARD:
            self.local_time += delta
            if self.local_time >= self.duration:
                if self.loop_style == LOOP:
                    self.local_time = rem_euclid(self.local_time, self.duration)
                elif self.loop_style == PING_PONG:
                    self.direction = BACKWARD
                    self.local_time = self.duration
                else:
                    self.local_time = self.duration
                    self.state = ENDED
        else:
            self.local_time -= delta
            if self.local_time <= 0.0:
                if self.loop_style == LOOP:
                    self.local_time = self.duration - rem_euclid(self.local_time, self.duration)
                elif self.loop_style == PING_PONG:
                    self.direction = FORWARD
                    self.local_time = 0.0
                else:
                    self.local_time = 0.0
                    self.state = ENDED


def search(times, time):
    """sampler.rs:116-136 -> ("exact", i) or ("between", l, r); a one-key sampler returns its key (deviation)."""
    n = len(times)
    if n == 1:
        return ("exact", 0)
    for i, t in enumerate(times):
        if t == time:
            return ("exact", i)
    i = sum(1 for t in times if t < time)      # the insertion point
    if i == 0:
        return ("between", 0, 1)
    if i >= n:
        return ("exact", n - 1)
    return ("between", i - 1, i)


def factor_f32(times, time, l, r) -> float:
    """interpolation_time is f64 and cast to f32 once (sampler.rs:81,92; interpolate.rs `t as f32`); the restatement takes that f32 value in f64."""
    return float(np.float32((time - times[l]) / (times[r] - times[l])))


def slerp(a, b, t):
    """The slerp contract of DESIGN.md section 15, in f64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dot = float(a @ b)
    if dot < 0.0:
        b, dot = -b, -dot
    if dot > 1.0 - FLT_EPSILON:
        return a + (b - a) * t
    theta = math.acos(dot)
    return (a * math.sin(theta * (1.0 - t)) + b * math.sin(theta * t)) * (1.0 / math.sin(theta))


def hermite(t):
    t2 = t * t
    t3 = t2 * t
    return 2.0 * t3 - 3.0 * t2 + 1.0, t3 - 2.0 * t2 + t, -2.0 * t3 + 3.0 * t2, t3 - t2


def sample(path, interpolation, times, values, time, in_tangents=None, out_tangents=None):
    """AnimationSampler::sample in f64 on f32 inputs; path in translation / rotation / scale / weights, interpolation in linear / step / cubic."""
    values = np.asarray(values, np.float32).astype(np.float64)
    b = search(list(times), time)
    if b[0] == "exact":
        return values[b[1]].copy()
    _, l, r = b
    if interpolation == "step":
        return values[l].copy()
    t = factor_f32(times, time, l, r)
    if interpolation == "linear":
        if path == "rotation":
            return slerp(values[l], values[r], t)
        return values[l] + t * (values[r] - values[l])
    dt = float(np.float32(times[r] - times[l]))
    lt = np.asarray(out_tangents, np.float32).astype(np.float64)[l]      # out[left], in[right] (sampler.rs:96-97)
    rt = np.asarray(in_tangents, np.float32).astype(np.float64)[r]
    h00, h10, h01, h11 = hermite(t)
    lv, rv = values[l], values[r]
    if path == "rotation":
        if float(lv @ rv) < 0.0:
            rv, rt = -rv, -rt
        q = lv * h00 + lt * (h10 * dt) + rv * h01 + rt * (h11 * dt)
        return q / math.sqrt(float(q @ q))
    return h00 * lv + h10 * lt * dt + h01 * rv + h11 * rt * dt
