// taa.hpp — the constants of the temporal anti-aliasing resolve (kernels_taa.hip).
#pragma once

namespace awsm {
namespace taa {

constexpr int kTile = 16;                    // one 256-thread workgroup per 16x16 pixels
constexpr int kApron = 1;                    // the 3x3 neighbourhood of the clamp
constexpr int kWin = kTile + 2 * kApron;     // 18: the window of the current image a workgroup stages

}  // namespace taa
}  // namespace awsm
