// pick.hpp — the constants and the kernel argument record of the point and rectangle queries that see transparent meshes (kernels_pick.hip,
// awsm_pick.cpp).  Shared by the library (awsm_pick.cpp sizes the scratch from them) and the kernels.
#pragma once
#include <stdint.h>

#include "frame_params.hpp"

namespace awsm {
namespace pick {

// the four layers a pixel's answer can come from, in the order an entry list is sorted by; the rule looks at them 3, 2, 1, 0
constexpr uint32_t kLayerWorld = 0, kLayerWorldTransparent = 1, kLayerHud = 2, kLayerHudTransparent = 3;
constexpr uint32_t kLayers = 4;
constexpr uint32_t kFlagTransparent = 1u;                   // AWSM_PICK_TRANSPARENT
constexpr uint32_t kMiss = 0xFFFFFFFFu;                     // the map's word where nothing is hit
constexpr uint32_t kLayerShift = 28, kDrawMask = (1u << kLayerShift) - 1u;      // map word = layer << 28 | draw index in its pass's list
constexpr int kTile = 16;                                   // k_pick_rect: one 256-thread workgroup per 16x16 pixels of the rectangle
constexpr uint32_t kPointWords = 8;                         // k_pick_point's answer: valid, key high, key low, triangle, layer, alpha bits, depth bits, map word
constexpr uint32_t kEntryWords = 4;                         // one rectangle entry: layer, key high, key low, pixels (AwsmPickRectEntry)
constexpr uint32_t kCollectThreads = 256;

}  // namespace pick

// One pass's draws as the queries reach them.  draw_base: the first index of the pass's own draws in `draws` (the hud draws of an MSAA frame follow
// the world's in one list, frame_params.hpp: rank0); the reported draw index and the counter of a draw are relative to it.
struct PickLayerDev {
    const DrawDev* draws;
    const uint32_t* tri_info;            // per triangle rank: the draw in the low 24 bits
    uint32_t n_draws, total_tris;        // of `draws` / `tri_info` as a whole
    uint32_t draw_base;
    uint32_t counter_base;               // the pass's first word in `counters`
};

// A transparent pass's fragment lists as it left them (FrameDev::frag_first / frag_rec / frag_color); first == null: the pass did not run or drew nothing
struct PickFragsDev {
    const uint32_t* first;
    const uint4* rec;
    const float4* color;
    const TriRec* tri_rec;
    uint32_t cap;
    uint32_t pad;
};

// What the pick kernels read and write: an argument of their own, FrameDev and every other kernel's arguments stay as they are.
struct PickDev {
    uint32_t width, height;
    uint32_t samples;                    // 1 or 4 keys per pixel in vis / hud_vis; the queries read sample 0
    uint32_t sy0, sy1, band_n, band_r;   // the rows the context owns (k_pick's own test): a pixel outside them is a miss
    uint32_t flags;                      // AwsmPickQuery.flags
    float alpha_threshold;
    int32_t x0, y0, x1, y1;              // k_pick_point: the pixel (x0, y0); k_pick_rect: the clamped rectangle [x0, x1) x [y0, y1)
    const uint8_t* geom_meta;            // geometry meta + 36 -> material mesh meta words 0 and 1: the mesh key, as k_pick reaches it
    const uint8_t* material_meta;
    uint32_t geom_meta_bytes, material_meta_bytes;      // an offset past them is a miss
    const unsigned long long* vis;       // the WORLD geometry pass's keys
    const unsigned long long* hud_vis;   // the HUD geometry pass's keys (null: the frame has no hud geometry)
    PickLayerDev layer[pick::kLayers];
    PickFragsDev frags[2];               // [0] the world transparent pass's, [1] the HUD transparent pass's
    uint32_t* counters;                  // k_pick_rect / k_pick_collect: one word per draw of the four passes, zeroed in front of the launch
    uint32_t n_counters;
    uint32_t cap;                        // entries `entries` can hold
    uint32_t* entries;                   // cap x kEntryWords
    uint32_t* n_out;                     // distinct (layer, mesh key) pairs
    uint32_t* draw_keys;                 // k_pick_collect's scratch: {high, low} per counter word, then the merged count per counter word
    uint32_t* merged;
    uint32_t* point_out;                 // k_pick_point: kPointWords
    uint32_t* map_word;                  // k_pick_map: width x height words and triangle indices
    uint32_t* map_triangle;
};

}  // namespace awsm
