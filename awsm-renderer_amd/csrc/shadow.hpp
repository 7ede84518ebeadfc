// shadow.hpp — the constants of the shadow resolve (kernels_shadow.hip).  tests/shadow_reference.py holds the same numbers and a CPU
// test compares the two.
#pragma once

namespace awsm {
namespace shadow {

constexpr int kTile = 16;             // one 256-thread workgroup per 16x16 pixels, one pixel per thread
constexpr int kWin = kTile + 2;       // 18: the tile and a one-pixel apron, staged in LDS
constexpr int kMaxRadius = 2;         // R <= 2: at most 5x5 taps
constexpr float kDetMin = 1e-12f;     // |det| of the receiver plane's 2x2 system below which the plane counts as flat
constexpr unsigned kHit = 1u, kInside = 2u;      // a staged cell's flags
constexpr int kMaxViews = 6;          // views of one light in a frame (AWSM_SHADOW_MAX_VIEWS): a cube's faces, or up to that many cascades
constexpr unsigned kNoView = 255u;    // the view layer's byte of a pixel that lies in no view

}  // namespace shadow
}  // namespace awsm
