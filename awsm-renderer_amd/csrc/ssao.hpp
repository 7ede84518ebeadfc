// ssao.hpp — the constants and the two tables of the screen-space ambient occlusion pass (kernels_ssao.hip).
//
// tests/ssao_reference.py derives both tables from f64 and a CPU test compares the literals below with that derivation, as tests/test_post_cpu.py
// does for the DoF disk.
#pragma once

namespace awsm {
namespace ssao {

constexpr int kTaps = 12;             // K: taps per pixel
constexpr int kRMax = 16;             // R_MAX: the largest sampling radius in pixels = the apron of the staged window
constexpr int kTile = 16;             // one 256-thread workgroup per 16x16 pixels
constexpr int kWin = kTile + 2 * kRMax;      // 48: the window of view positions a workgroup stages for its taps
constexpr int kBlur = 2;              // the depth-aware smoothing is (2 kBlur + 1)^2 = 5x5
constexpr int kBlurWin = kTile + 2 * kBlur;  // 20

#ifdef __HIPCC__
// t_i = sqrt((i + 0.5) / K) * (cos, sin)(i * 2.39996323), i = 0 .. K - 1, rounded once to f32
__constant__ const float kSpiral[kTaps][2] = {
    {2.041241527e-01f, 0.000000000e+00f}, {-2.606992722e-01f, 2.388218790e-01f}, {3.990420327e-02f, -4.546878040e-01f}, {3.285945356e-01f, 4.285933971e-01f},
    {-6.030113697e-01f, -1.066642255e-01f}, {5.712250471e-01f, -3.633666039e-01f}, {-1.910635978e-01f, 7.107470632e-01f}, {-3.643789887e-01f, -7.015895844e-01f},
    {7.905566692e-01f, 2.887100279e-01f}, {-8.224424720e-01f, 3.394922912e-01f}, {3.964716196e-01f, -8.472368121e-01f}, {2.929824293e-01f, 9.340742230e-01f}};
// (cos, sin)(2 pi b / 16), b = the 4x4 Bayer matrix {0 8 2 10 / 12 4 14 6 / 3 11 1 9 / 15 7 13 5}, entry [(y & 3) * 4 + (x & 3)], rounded once to f32
__constant__ const float kRotation[16][2] = {
    {1.000000000e+00f, 0.000000000e+00f}, {-1.000000000e+00f, 1.224646853e-16f}, {7.071067691e-01f, 7.071067691e-01f}, {-7.071067691e-01f, -7.071067691e-01f},
    {-1.836970147e-16f, -1.000000000e+00f}, {6.123234263e-17f, 1.000000000e+00f}, {7.071067691e-01f, -7.071067691e-01f}, {-7.071067691e-01f, 7.071067691e-01f},
    {3.826834261e-01f, 9.238795042e-01f}, {-3.826834261e-01f, -9.238795042e-01f}, {9.238795042e-01f, 3.826834261e-01f}, {-9.238795042e-01f, -3.826834261e-01f},
    {9.238795042e-01f, -3.826834261e-01f}, {-9.238795042e-01f, 3.826834261e-01f}, {3.826834261e-01f, -9.238795042e-01f}, {-3.826834261e-01f, 9.238795042e-01f}};
#endif

}  // namespace ssao
}  // namespace awsm
