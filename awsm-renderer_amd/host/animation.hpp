// animation.hpp — the reference's animation players and samplers, restated for the C++ host layer (paths relative to
// /root/reference/crates/renderer/src/):
//   animation/player.rs:41-100        AnimationPlayer::new / update (f64 local time, loop styles, direction, state)
//   animation/sampler.rs:62-136       AnimationSampler::sample / binary_search_bounds
//   animation/interpolate.rs:6-114    lerp / slerp / cubic Hermite on Vec3, Quat, f32
//   animation/data.rs:216-393         TransformAnimation / VertexAnimation (one component per clip here: a clip carries one path)
//   animation/clip.rs                 AnimationClip { duration, sampler }
// Header-only and free of the host's state, so that a stand-alone program can drive it.
// Compiled with -ffp-contract=off like glam.hpp: every f32 operation rounds once, in the written order.
//
// The reference's rules are kept, quirks included (DESIGN.md section 15 lists them and the tests that pin each):
//   * backward + loop lands at duration - rem_euclid(local_time, duration): -0.1 of a 1.0 clip is 0.1, not 0.9 (player.rs:85-86)
//   * a time before the first key extrapolates keys (0, 1) with a negative factor (sampler.rs:126-127)
//   * cubic takes out_tangents[left] and in_tangents[right] (sampler.rs:96-97)
// Deviations, each where the reference panics or yields NaN: no keys is refused (valid()), a one-key sampler returns its key for any time,
// a clip whose duration is not > 0 never advances, a width that does not fit the path is refused.
// Quat::slerp: glam's source is not available to this project, so the rule is fixed here (slerp below) and DESIGN.md says so.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

namespace awsm_host {
namespace anim {

enum Path : uint32_t { kTranslation = 0, kRotation = 1, kScale = 2, kWeights = 3 };
enum Interpolation : uint32_t { kLinear = 0, kStep = 1, kCubicSpline = 2 };
enum LoopStyle : int { kNone = -1, kLoop = 0, kPingPong = 1 };
enum Direction : int { kForward = 0, kBackward = 1 };
enum State : int { kPlaying = 0, kPaused = 1, kEnded = 2 };

struct Sampler {
    uint32_t path = kTranslation, interpolation = kLinear, width = 3;
    std::vector<double> times;
    std::vector<float> values, in_tangents, out_tangents;      // n_keys * width each (the tangents: cubic only)

    // what insert refuses: no keys, a width the path does not have, arrays that do not cover the keys
    bool valid() const {
        const size_t n = times.size();
        if (n == 0 || width == 0 || path > kWeights || interpolation > kCubicSpline) return false;
        if ((path == kTranslation || path == kScale) && width != 3) return false;
        if (path == kRotation && width != 4) return false;
        if (values.size() != n * width) return false;
        if (interpolation == kCubicSpline && (in_tangents.size() != n * width || out_tangents.size() != n * width)) return false;
        return true;
    }
};

inline double rem_euclid(double a, double b) {      // f64::rem_euclid
    const double r = std::fmod(a, b);
    return r < 0.0 ? r + std::fabs(b) : r;
}

struct Player {      // player.rs:7-15
    double speed = 1.0 / 1000.0;
    int loop_style = kLoop;
    int direction = kForward;
    int state = kPlaying;
    double local_time = 0.0;
    double duration = 0.0;      // AnimationClip::duration
    Sampler sampler;

    void update(double global_time_delta) {      // player.rs:53-100
        if (state != kPlaying) return;
        if (!(duration > 0.0)) return;      // deviation: rem_euclid(x, 0) is NaN in the reference
        const double local_time_delta = global_time_delta * speed;
        if (direction == kForward) {
            local_time += local_time_delta;
            if (local_time >= duration) {
                if (loop_style == kLoop) local_time = rem_euclid(local_time, duration);
                else if (loop_style == kPingPong) { direction = kBackward; local_time = duration; }
                else { local_time = duration; state = kEnded; }
            }
        } else {
            local_time -= local_time_delta;
            if (local_time <= 0.0) {
                if (loop_style == kLoop) local_time = duration - rem_euclid(local_time, duration);      // the mirrored landing: kept
                else if (loop_style == kPingPong) { direction = kForward; local_time = 0.0; }
                else { local_time = 0.0; state = kEnded; }
            }
        }
    }
};

// ---- interpolate.rs, on `width` floats ----
inline float quat_dot(const float* a, const float* b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// The slerp contract of this repository: flip `end` when dot < 0; lerp when dot > 1 - FLT_EPSILON; else
// theta = acosf(dot) and (a sin(theta (1 - t)) + b sin(theta t)) * (1 / sin(theta)), all in f32.
inline void slerp(const float* a, const float* b_in, float t, float* out) {
    float b[4] = {b_in[0], b_in[1], b_in[2], b_in[3]};
    float dot = quat_dot(a, b);
    if (dot < 0.0f) { for (float& v : b) v = -v; dot = -dot; }
    if (dot > 1.0f - FLT_EPSILON) {
        for (int i = 0; i < 4; i++) out[i] = a[i] + (b[i] - a[i]) * t;
        return;
    }
    const float theta = acosf(dot);
    const float s1 = sinf(theta * (1.0f - t)), s2 = sinf(theta * t), inv = 1.0f / sinf(theta);
    for (int i = 0; i < 4; i++) out[i] = (a[i] * s1 + b[i] * s2) * inv;
}

struct Hermite { float h00, h10, h01, h11; };
inline Hermite hermite(float t) {      // interpolate.rs:37-43
    const float t2 = t * t, t3 = t2 * t;
    return {2.0f * t3 - 3.0f * t2 + 1.0f, t3 - 2.0f * t2 + t, -2.0f * t3 + 3.0f * t2, t3 - t2};
}

// The search of sampler.rs:116-136: exact = 1 and left = the key, or the pair (left, right).  n >= 1.
struct Bounds { bool exact; size_t left, right; };
inline Bounds search(const std::vector<double>& times, double time) {
    const size_t n = times.size();
    if (n == 1) return {true, 0, 0};      // deviation: Between(0, 1) of a one-key sampler indexes past the end in the reference
    size_t lo = 0, hi = n;      // the first index whose time is not less than `time`; an incomparable pair (NaN) counts as Equal, as unwrap_or does
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        const double t = times[mid];
        if (t < time) lo = mid + 1;
        else if (t > time) hi = mid;
        else return {true, mid, mid};
    }
    if (lo == 0) return {false, 0, 1};      // before the first key: extrapolates with a negative factor
    if (lo >= n) return {true, n - 1, n - 1};
    return {false, lo - 1, lo};
}

// AnimationSampler::sample: `width` floats into out
inline void sample(const Sampler& s, double time, float* out) {
    const uint32_t w = s.width;
    const Bounds b = search(s.times, time);
    const float* lv = s.values.data() + b.left * w;
    if (b.exact || s.interpolation == kStep) { for (uint32_t i = 0; i < w; i++) out[i] = lv[i]; return; }
    const float* rv = s.values.data() + b.right * w;
    const double left_time = s.times[b.left], right_time = s.times[b.right];
    const double interpolation_time = (time - left_time) / (right_time - left_time);      // f64, cast once
    const float t = (float)interpolation_time;
    if (s.interpolation == kLinear) {
        if (s.path == kRotation) slerp(lv, rv, t, out);
        else if (s.path == kWeights) for (uint32_t i = 0; i < w; i++) out[i] = lv[i] + t * (rv[i] - lv[i]);      // interpolate_linear_f32
        else for (uint32_t i = 0; i < w; i++) out[i] = lv[i] + (rv[i] - lv[i]) * t;                           // Vec3::lerp
        return;
    }
    const float dt = (float)(right_time - left_time);
    const float* lt = s.out_tangents.data() + b.left * w;      // out[left], in[right]
    const float* rt = s.in_tangents.data() + b.right * w;
    const Hermite h = hermite(t);
    if (s.path == kRotation) {      // interpolate.rs:52-89
        float sv[4], st[4];
        const bool flip = quat_dot(lv, rv) < 0.0f;
        for (int i = 0; i < 4; i++) { sv[i] = flip ? -rv[i] : rv[i]; st[i] = flip ? -rt[i] : rt[i]; }
        float q[4];
        const float k10 = h.h10 * dt, k11 = h.h11 * dt;
        for (int i = 0; i < 4; i++) q[i] = ((lv[i] * h.h00 + lt[i] * k10) + sv[i] * h.h01) + st[i] * k11;
        const float inv = 1.0f / std::sqrt(quat_dot(q, q));      // Quat::normalize
        for (int i = 0; i < 4; i++) out[i] = q[i] * inv;
        return;
    }
    for (uint32_t i = 0; i < w; i++)      // interpolate.rs:45-48,110-113
        out[i] = (((h.h00 * lv[i]) + (h.h10 * lt[i] * dt)) + (h.h01 * rv[i])) + (h.h11 * rt[i] * dt);
}

}  // namespace anim
}  // namespace awsm_host
