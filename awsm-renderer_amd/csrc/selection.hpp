// selection.hpp — the constants and the kernel argument record of the editor's selection overlay (kernels_selection.hip): an outline
// around the visible pixels of the selected meshes and a wire box around every selected mesh's world AABB, drawn as the last step of the world
// transparent pass.  Shared by the library (awsm_hip.cpp checks the caps) and the kernels (the LDS sizes follow from them).
#pragma once
#include <stdint.h>

#include "frame_params.hpp"

namespace awsm {
namespace selection {

constexpr uint32_t kMaxKeys = 64;                           // mesh keys per selection
constexpr uint32_t kMaxBoxes = 64;                          // world-space boxes per selection
constexpr uint32_t kEdgesPerBox = 12;
constexpr uint32_t kMaxEdges = kMaxBoxes * kEdgesPerBox;    // 768: the overlay's LDS index list holds them all, so there is no overflow path
constexpr uint32_t kEdgeFloats = 8;                         // one edge record: x0 y0 z0 x1 y1 z1 valid pad (32 bytes)
constexpr int kTile = 16;                                   // one 256-thread workgroup per 16x16 pixels
constexpr int kMaxRadius = 4;                               // the largest outline radius = the apron of the staged window
constexpr int kWin = kTile + 2 * kMaxRadius;                // 24
constexpr float kMaxHalfWidth = 4.0f;
constexpr uint32_t kFlagOutline = 1u, kFlagBoxes = 2u;      // AWSM_SELECTION_OUTLINE, AWSM_SELECTION_BOXES

}  // namespace selection

// What the selection kernels read and write.  The keys and the boxes travel inside the record, as kernel arguments: a pass already enqueued keeps
// what it was given whatever the caller sets afterwards.
struct SelectionDev {
    uint32_t width, height;
    uint32_t msaa;                       // 1 or 4 keys per pixel in vis
    uint32_t n_draws, total_tris;        // the WORLD geometry pass's draw list (never the hud's) and its triangle count
    uint32_t n_keys, n_boxes;
    uint32_t flags, radius;              // AwsmSelection.flags, outline_radius
    float outline_color[4], box_color[4];
    float half_width, hidden_alpha, depth_epsilon;
    const DevScene* scene;               // geometry meta + 36 -> material mesh meta words 0 and 1: the mesh key, as k_pick reaches it
    uint32_t material_meta_bytes;        // a material meta offset past this is never selected
    const DrawDev* draws;
    const uint32_t* tri_info;            // per triangle rank: the draw in the low 24 bits
    const unsigned long long* vis;       // the WORLD geometry pass's keys
    const uint8_t* camera;               // the frame's camera snapshot (512 B): view_proj at bytes 128..191
    uint8_t* draw_selected;              // per frame slot: one byte per world draw (k_selection_mark)
    float* edges;                        // per frame slot: n_boxes x 12 edge records (k_selection_edges)
    uint2* out16;                        // the composite, blended in place
    float4* out32;                       // its f32 parity tap (may be null)
    const uint32_t* poison;              // FrameDev.poison / frame_serial
    uint32_t frame_serial;
    uint8_t* layer_selected;             // awsm_hip_read_selection only: s, ring and A per pixel
    uint8_t* layer_ring;
    float* layer_box_alpha;
    uint32_t keys[2 * selection::kMaxKeys];      // {high, low} per key, as AwsmPick reports them
    float boxes[6 * selection::kMaxBoxes];       // {min xyz, max xyz} per box, world space
};

}  // namespace awsm
