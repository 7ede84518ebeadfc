// ctx.hpp — the context behind the C ABI of include/awsm_hip.h, declared once: struct AwsmHipCtx and the types it is made of, and the handful of
// helpers through which the resource entry points (awsm_resources.cpp) reach the frame pipeline's state.  The helpers are defined in awsm_hip.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "frame_params.hpp"
#include "dirty_log.hpp"

namespace awsm {

// Frame slots of the overlap mode: frame i's opaque pass reads slot i % kSlots while the geometry pass of frame i + 1 fills the next.  (Three
// slots — the geometry pass of frame i + 2 no longer waiting for frame i's opaque pass — measured no different, and cost a fifth stream.)  AWSM_SLOTS sizes AwsmHipCtx: a -D for it goes to every file that includes this header (csrc/Makefile).
#ifndef AWSM_SLOTS
#define AWSM_SLOTS 2
#endif
constexpr int kSlots = AWSM_SLOTS;
struct DevBuf {
    void* ptr = nullptr;
    size_t size = 0;
};

enum { EV_START = 0, EV_TRANSFORM, EV_BIN, EV_RASTER, EV_SHADE_BEGIN, EV_SHADE_LEAN, EV_SHADE, EV_FWD_BEGIN, EV_FWD, EV_COUNT };

// Which pass a FrameBufs serves: AwsmHipCtx::fb, tr, hud, htr, shadow in that order (set once by awsm_hip_create).
// A pass is named by its kind everywhere on the host: pass_bufs(c, kind) is its device state in the current frame slot, AwsmHipCtx::lists[kind] its draw list.
enum PassKind : uint8_t { kPassWorld = 0, kPassTransparent, kPassHud, kPassHudTransparent, kPassShadow };
constexpr int kPassKinds = 5;

// What the host knows of a pass's draws in the current frame: one DrawDev per (draw, instance) with the running triangle / block prefix sums
// (build_draw_list), their totals (vertices: 3 * total_tris), and the k_deform_transform workgroups they take.
struct PassList {
    std::vector<DrawDev> draws;
    uint32_t total_tris = 0, n_blocks = 0;
};

// Everything the geometry pass produces for one frame and the opaque pass consumes.
struct FrameBufs {
    DevBuf wpos;                           // transparent pass only
    DevBuf frag_rec, frag_color, frag_first;   // transparent pass: per-pixel fragment lists
    uint32_t frag_cap = 0;
    DevBuf tex_slots;                      // n_draws x kCoreTextures TexSlotDev (k_resolve_draws)
    DevBuf draw_mat;                       // n_draws DrawMatDev (k_resolve_draws)
    DevBuf tri_shade, draw_lean;           // geometry pass: per-triangle attribute offsets (k_deform_transform), per-draw lean records (k_resolve_draws)
    DevBuf clip, nrm, tan, tri_rec, tri_flags, draws_dev, draw_shade, tile_count, tile_offset, tile_cursor, tile_order, bin_list, big_list, counters, vis;
    DevBuf camera;                         // snapshot of the camera UBO taken by the geometry pass (overlap mode)
    DevBuf scan_tmp;                       // k_bin_scan's cross-workgroup tables
    DevBuf tile_split, raster_scratch;     // split raster tiles: per-tile {first scratch slot, slices done}; partial tiles (geometry pass only)
    uint32_t raster_extra_cap = 0, raster_slot_cap = 0;
    uint32_t bin_capacity = 0;
    float pix2view[16] = {}, view_rot[9] = {}, cam_pos[3] = {}, ortho_view_dir[3] = {};   // the lean opaque kernel's view of the camera this slot's frame was submitted with
    uint32_t cam_ortho = 0;
    size_t tri_cap = 0, draw_cap = 0;      // triangles / draws the per-pass buffers below are sized for (reserve_pass_buffers)
    uint32_t sized_w = 0, sized_h = 0;     // ... and the frame size their tile tables are sized for
    std::vector<DrawDev> draws_uploaded;   // what draws_dev currently holds
    void* draws_uploaded_ptr = nullptr;
    bool draws_uploaded_valid = false;
    uint64_t draws_version = 0;            // bumped whenever draws_dev receives a new list
    // MSAA frames with hud meshes: the hud draws behind the world's in draws_dev (awsm_hip_hud_geometry_pass), cached by themselves so that the world
    // list's own cache keeps hitting
    std::vector<DrawDev> tail_uploaded;
    void* tail_uploaded_ptr = nullptr;
    size_t tail_uploaded_at = 0;
    bool tail_uploaded_valid = false;
    // Geometry cache (frame_params.hpp; the world geometry pass only): the draw list this slot's wcache / nrm / tan / tri_shade / tri_info were last
    // computed for lives on in draws_prev when a new list arrives (the two buffers swap), so that k_deform_transform can compare draw by draw.
    DevBuf wcache, draws_prev;
    DevBuf block_map;                      // world geometry pass: draw index of every k_deform_transform workgroup (uploaded with the draw list; spares each workgroup a binary search over the list = log2(n) dependent loads in front of everything else)
    bool block_map_valid = false;
    DevBuf cache_mark;                     // one word per k_deform_transform workgroup: the serial of the last frame in which it took the cached path (statistics only)
    uint32_t cached_n_draws = 0;           // draws of the list the arrays were computed for
    bool cache_valid = false;              // ... and whether they were (false after any re-allocation, a frame without geometry, a dropped frame)
    bool cached_is_prev = false;           // that list is in draws_prev (a new list has been uploaded since), else it is draws_dev's
    bool cache_had_tri_shade = false;
    uint64_t cache_seq = 0;                // write_seq when that geometry pass was enqueued: dirty ranges logged after it apply
    uint32_t cache_serial = 0;             // its frame serial
    PassKind kind = kPassWorld;            // which pass this is, and its frame slot (two bytes of the struct's tail padding: every other member keeps its offset)
    uint8_t slot = 0;
    // Clip positions formed in the binning (FrameDev::clip_from_world; the world geometry pass only): where k_draw_decide's word per draw starts in
    // block_map (words; 0: none) and the compact bin records in tri_rec (8-byte records; 0: none) — both share the older buffer's allocation, so that
    // FrameDev names them with a 32-bit offset — and whether the slot's last world pass ran that way: its clip buffer then holds nothing of that
    // frame, and awsm_hip_read_transformed forms it on demand.
    uint32_t draw_hit_at = 0, bin_rec_at = 0;
    bool clip_in_bin_last = false;
};

}  // namespace awsm

using namespace awsm;      // as the files that include this header do: AwsmHipCtx is the C ABI's global type, made of awsm:: parts

struct AwsmHipCtx {
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool stage_timers = true;      // hipEventRecord between the stages of a frame (AwsmFrameStats.ms_*); awsm_hip_set_stage_timers
    std::string last_error;

    DevBuf bufs[AWSM_BUF_COUNT];
    bool camera_written_since_snapshot = false;      // awsm_hip_buffer_write(AWSM_BUF_CAMERA) since the last geometry pass took its snapshot
    uint8_t camera_host[512] = {};   // what the caller last wrote to AWSM_BUF_CAMERA (awsm_hip_buffer_write): compose_pixel_to_view reads it
    DevScene scene{};            // host copy
    DevScene* scene_dev = nullptr;
    bool scene_dirty = true;
    DevBuf tex[kMaxTexArrays];
    DevBuf lut;
    DevBuf cube_tex[3], cube_bordered[3];      // the uploaded chains; the same with a one-texel apron per face (CubeDev.bordered)
    // awsm_hip_env_cube_write_* / fill_*: the source bytes on the device (grow-only, reused), the 8-bit -> f16 tables, the fills' row table,
    // and the event a write waits on when it copied straight from the caller's memory
    DevBuf env_stage, env_tables, env_rows, env_filter_tab;      // env_filter_tab: the sample tables of awsm_hip_env_cube_filter
    hipEvent_t ev_env_copy = nullptr;
    // the texture pool at run time (awsm_hip_texture_array_write_layers / _generate_mips_layers): MipmapTextureKind per layer of each array, on the
    // device and written in stream order; the sRGB table, made once
    DevBuf tex_kinds[kMaxTexArrays];
    uint32_t tex_srgb[64] = {};
    bool tex_srgb_made = false;

    // awsm_hip_skin_pose: the resident records (72 bytes each; grows by doubling) and the host's copy, against which a list's ids and offsets are checked
    DevBuf pose_records;
    std::vector<AwsmSkinPoseRecord> pose_records_host;

    // frame targets
    uint32_t width = 0, height = 0;
    uint32_t y0 = 0, y1 = 0;     // shard rows (0,0 = full)
    uint32_t band_n = 1, band_r = 0, band_compact = 0;   // shard bands (awsm_hip_set_shard_bands)
    uint32_t msaa = 0;           // 0 or 4 (awsm_hip_resize)
    DevBuf mip_kinds;                 // scratch for awsm_hip_texture_array_generate_mips
    // MSAA scratch, per frame slot (frame i + 1's k_shade_lean may run beside frame i's k_msaa_detect / k_shade_msaa_resolve):
    DevBuf msaa_color0[kSlots], msaa_edges[kSlots];   // f32 colour of sample 0 per pixel; per block [count, one-byte pixel slots...] of edge pixels
    DevBuf msaa_edge_bits[kSlots];    // lean route: two u64 per 16x4 strip (FrameDev.msaa_edge_bits)
    DevBuf msaa_cells[kSlots];        // lean route: normal + depth of sample 0 per pixel (FrameDev.msaa_cells)
    DevBuf out16[kSlots], out32[kSlots];        // the opaque image (+ f32 parity tap) per frame slot: with two images two frames' opaque passes need no order between them
    DevBuf digest;                    // 2 x u64 (awsm_hip_visibility_digest)
    uint32_t lean_grid = 0;           // persistent k_shade_lean grid (workgroups), 0 = one workgroup per block
    DevBuf shade_todo[kSlots];             // per frame slot (the per-draw resolve of frame i + 1 resets one while frame i's opaque pass appends to the other); [0] count + entries: the 16x4-pixel groups the lean opaque kernel leaves to the general one
    void* bound_out = nullptr;
    size_t bound_out_bytes = 0;
    const uint8_t* slot_out_lo[kSlots] = {}; const uint8_t* slot_out_hi[kSlots] = {};     // the bound image each slot's last opaque pass wrote (null: the library's own)

    // geometry-pass resources
    // Frame overlap (AWSM_CFG_OVERLAP_FRAMES): the opaque pass of frame i runs on shade_stream while the caller's stream
    // already runs the geometry pass of frame i+1 into the other slot.
    bool overlap = false;
    hipStream_t shade_streams[kSlots] = {};     // one per frame slot: the waits in front of frame i + 1's opaque pass are consumed while frame i's still runs (enqueue_opaque)
    bool shade_recorded[kSlots] = {};
    bool uploads_recorded[kSlots] = {};  // ev_uploads[slot] was recorded by this frame's geometry pass
    // What a slot's per-draw records (k_resolve_draws: draw_shade / draw_mat / tex_slots / draw_lean / lights_pre) were computed from: they are
    // recomputed only when that changed — a frame that moved nothing but the camera reuses them (no kernel, no event).
    struct ResolveKey { uint64_t write_seq, draws_version; const void* ptrs[5]; uint32_t n_draws, mipmap, has_opaque, lights_cap; } resolved[kSlots] = {};   // ev_shade_done[slot] has been recorded since the last full synchronisation
    hipEvent_t ev_geom_done[kSlots] = {}, ev_shade_done[kSlots] = {}, ev_uploads[kSlots] = {} ;
    hipEvent_t ev_flush = nullptr;             // awsm_hip_frame_flush: system-scope release in front of what the CALLER enqueues next (a collective, a peer / host copy)
    uint64_t write_seq = 0, geom_write_seq[kSlots] = {};     // scene writes so far / at the time the slot's geometry pass was enqueued
    // Geometry cache: the byte ranges written (awsm_hip_buffer_write / buffer_create) to the buffers k_deform_transform reads, each with the write_seq it got;
    // a slot's geometry pass hands the kernel those newer than the slot's cache_seq.  all_dirty_seq: everything up to that write_seq counts as "all
    // written" (the log overflowed, or a buffer was written whose every write invalidates every draw).
    DirtyLog dirty_log;                         // (dirty_log.hpp)
    bool geometry_cache = true;                 // AWSM_GEOMETRY_CACHE=0 turns it off (A/B measurements, tests)
    uint32_t cache_blocks_last = 0;             // AwsmFrameStats.geometry_cache_blocks of the frame frame_end last looked at
    bool shade_pending[kSlots] = {};
    // Device-side hand-off between the streams (kernels_geometry.hip: k_handoff_signal / k_handoff_wait) in place of the two cross-stream events
    // on a frame's critical path: geometry pass -> opaque pass of the same frame, opaque pass of frame i -> geometry pass of frame i + kSlots.
    bool handoff = false;
    uint32_t* handoff_flags = nullptr;          // device: [slot] geometry done, [kSlots + slot] shading done, [2 kSlots + slot] k_shade_lean done — the serial number last signalled
    uint32_t geom_sig[kSlots] = {}, shade_sig[kSlots] = {}, lean_sig[kSlots] = {};   // flags [2 kSlots + slot]: the slot's k_shade_lean has ended (stored by k_shade_todo as it starts)
    bool lean_flagged[kSlots] = {};             // the slot's last opaque pass took the lean route with the flag: the next frame's pass may start on lean_sig
    unsigned long long handoff_budget_ticks = 400000000ull;   // a gate's time budget in device-clock ticks (AWSM_HANDOFF_TIMEOUT_MS; default 4 s at 100 MHz):
                                                // far longer than any frame or host stall, short enough that a gate nobody opens ends
    uint32_t clock_khz = 100000;                // hipDeviceAttributeWallClockRate
    uint32_t* handoff_poison = nullptr;         // device: [slot] serial of the slot's last frame whose gate timed out (FrameDev.poison)
    uint32_t handoff_timeouts_seen = 0;
    uint32_t handoff_dropped_frames = 0;        // gates that timed out = frames dropped whole (AwsmFrameStats.frames_dropped_by_handoff)
    bool handoff_error_pending = false;         // a time-out has been counted but not yet reported to the caller
    uint32_t handoff_test_drop = 0;             // AWSM_TEST_HANDOFF_DROP: that many geometry-done signals are withheld (tests of the timeout path)
    FrameBufs fb[kSlots];             // per-frame device state; two slots when frames overlap (AWSM_CFG_OVERLAP_FRAMES), else slot 0 only
    FrameBufs tr[kSlots];             // the same for the transparent pass's own draws (vertices, setup records, bins); no visibility buffer
    FrameBufs hud[kSlots];            // ... and for the HUD geometry pass (render.rs:169-178): its own vertices, bins and visibility keys (= hud_depth + the hud triangles)
    bool hud_geometry_done = false;   // this frame has hud geometry: the opaque pass leaves its pixels cleared
    // MSAA frames: the hud draws follow the world's in ONE rank space (transformed into the world pass's vertex / setup arrays behind the world's, binned and
    // rasterised by themselves into hud[slot].vis), and the opaque pass reads the merged keys (k_hud_merge: hud rank under world depth) — what the
    // reference's targets hold after its HUD geometry pass.  hud_merged: this frame's hud pass went that way.
    bool hud_merged = false;
    DevBuf merged_vis[kSlots];
    std::vector<DrawDev> hud_combined;   // world draws, then the hud draws with first_tri / first_block continued
    // the world transparent pass and the HUD transparent pass: each with its own per-slot device state (tr / htr) and its own list — the HUD pass of a
    // frame is enqueued while the world pass of the same frame may not have started on the shade stream, so they share neither a draw list nor counters
    bool transparent_done = false, hud_transparent_done = false;
    FrameBufs htr[kSlots];
    // the editor's ground grid (awsm_hip_set_editor_grid): what the caller last set, and per frame slot what the slot's world transparent pass was
    // enqueued with (awsm_hip_frame_end replays the pass with that); grid_layer: awsm_hip_read_editor_grid's scratch
    struct GridState { bool on = false; float p[20] = {}; } grid, grid_pass[kSlots];
    DevBuf grid_layer;
    // the editor's selection overlay (awsm_hip_set_selection, kernels_selection.hip): what the caller last set, and per frame slot what the slot's
    // world transparent pass was enqueued with (awsm_hip_frame_end replays the pass with that); sel_tables: per slot the byte per world draw and the
    // edge records; sel_layers: awsm_hip_read_selection's scratch
    struct SelectionState {
        bool on = false;
        uint32_t flags = 0, radius = 0;
        float outline_color[4] = {}, box_color[4] = {}, half_width = 0, hidden_alpha = 0, depth_epsilon = 0;
        std::vector<uint32_t> keys;       // {high, low} per key
        std::vector<float> boxes;         // {min xyz, max xyz} per box
    } sel, sel_pass[kSlots];
    DevBuf sel_tables[kSlots], sel_layers;
    DevBuf comp16, comp32;       // composite image (after the transparent pass) + parity tap
    // the effects + display passes (awsm_hip_post_pass): the display image per frame slot (or the caller's), the effects image (parity tap only),
    // the bloom chain's two f16 images and the per-pixel DoF terms — the last four per context: a post pass waits for the other slot's to end
    DevBuf display8[kSlots], effects16, bloom_a, bloom_b, dof_lc, dof_blur;
    void* bound_display = nullptr;
    size_t bound_display_bytes = 0;
    void* last_display = nullptr;     // what the last post pass wrote
    bool post_done = false;           // a post pass of the current frame was enqueued: awsm_hip_frame_end enqueues it again after replaying the frame
    AwsmPostParams post_params{};     // ... with these parameters
    DevBuf lights_pre[kSlots];        // per frame slot: per-light constants (k_resolve_draws), sized with the lights buffer
    void* bound_comp = nullptr;
    size_t bound_comp_bytes = 0;
    const void* msaa_halo = nullptr;       // awsm_hip_msaa_halo_bind
    size_t msaa_halo_bytes = 0;
    const void* opaque_src = nullptr;      // awsm_hip_bind_opaque_source: the gathered full-frame opaque image (sharded transparent pass)
    size_t opaque_src_bytes = 0;
    int slot = 0;
    PassList lists[kPassKinds];       // by PassKind: the draws each pass of the current frame was given
    std::vector<AwsmDraw> draws_api;
    bool geometry_done = false, opaque_done = false;
    AwsmOpaqueParams last_opaque{};
    uint32_t overflow_retries = 0;
    bool has_opaque_for_stats() const { return !opaque_done || last_opaque.has_opaque != 0; }

    // pinned staging ring for buffer_write / small uploads
    uint8_t* stage = nullptr;
    size_t stage_cap = 0, stage_head = 0;
    uint32_t* counters_host = nullptr;   // pinned, 16 u32: [0..8) geometry pass, [8..16) transparent pass; then kSlots x {entries needed, frame serial} (k_bin_scan)
    uint32_t frame_serial = 0, status_seen[kSlots] = {};
    uint32_t dropped_frames = 0;         // enqueue-only frames that overflowed their bin list
    uint32_t out_first_row = 0;          // awsm_hip_bind_output_rows
    bool out_rows_mode = false;

    hipEvent_t ev[EV_COUNT] = {};
    bool ev_valid[EV_COUNT] = {};

    // frame trace (awsm_hip_frame_trace): device-clock stamps [3][trace_cap] — geometry pass begins / geometry pass done / shading done —
    // of frame `serial` at index serial % trace_cap, written by one-lane kernels in stream order (the hand-off's signal kernels where they exist)
    unsigned long long* trace_dev = nullptr;
    uint32_t trace_cap = 0;

    // screen-space ambient occlusion (awsm_hip_set_ssao): what the caller last set, and per frame slot what the slot's opaque pass was enqueued with
    // (awsm_hip_frame_end replays the pass with that); ssao_layers: per slot [3][px] f32 — A, A', view z — sized for ssao_px pixels.
    // (New state goes to the end of the struct, the shadows' below likewise: every older member keeps the offset it had.)
    struct SsaoState { bool on = false; float p[4] = {}; } ssao, ssao_pass[kSlots];
    DevBuf ssao_layers[kSlots];
    size_t ssao_px[kSlots] = {};     // pixels of the frame the slot's layers were last written for (0: never)

    // shadows (awsm_hip_shadow_pass).  shadow[slot]: the light's geometry pass's own vertex arrays, setup records, tile tables, lists and
    // keys (vis = the S x S map), as hud[slot] is the HUD geometry pass's.  shadow_scene[slot]: a second device copy of the scene table whose camera
    // entry is shadow_cam[slot], the slot's copy of the light block — k_deform_transform reads view_proj through the table (shadow_scene_seq: the
    // scene_uploads count it was copied at).  shadow_pass[slot]: what the slot's pass was enqueued with, into the resolve's arguments and a replay.
    FrameBufs shadow[kSlots];
    DevScene* shadow_scene[kSlots] = {};
    uint64_t shadow_scene_seq[kSlots] = {}, scene_uploads = 0;
    DevBuf shadow_cam[kSlots];
    bool shadow_done = false;        // this frame had a shadow pass
    struct ShadowState { bool on = false; AwsmShadow p{}; float light_view_proj[16] = {}; } shadow_pass[kSlots];
    DevBuf shadow_layers[kSlots];    // per slot [2][px] f32: V, m
    size_t shadow_px[kSlots] = {};   // pixels of the frame the slot's layers were last written for (0: that frame had no resolve)

    // temporal anti-aliasing (awsm_hip_set_taa).  taa: what the caller last set; taa_pass: what the frame's post pass was given
    // (awsm_hip_frame_end enqueues that pass again with it).  taa_img: two RGBA16F images per context — not per frame slot — in ping-pong:
    // taa_img[taa_cur] is what the last resolve wrote, the other one what it read.  The index advances once per frame serial (taa_serial; 0: no
    // resolve since the history was last dropped), so a replayed post pass reads the same history and rewrites the same image.
    struct TaaState {
        bool on = false;
        float feedback = 0.1f;
        uint32_t flags = 0;
        float jitter[2] = {};
        float reproject[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    } taa, taa_pass;
    DevBuf taa_img[2], taa_layers;   // taa_layers: awsm_hip_read_taa's scratch
    int taa_cur = 0;
    bool taa_have = false;           // taa_img[taa_cur] holds a resolved image of this size and mode: the next frame's history
    bool taa_frame_hist = false;     // the resolve of frame taa_serial had a history
    uint32_t taa_serial = 0;
    bool taa_resolved = false;       // the last post pass resolved (awsm_hip_read_taa)
    TaaArgs taa_args{};              // ... with these arguments

    // shadows from several views (awsm_hip_shadow_pass_views).  shadow_views[slot].n: the views of the slot's pass, 0 when it came
    // through awsm_hip_shadow_pass.  With views, shadow[slot].vis is a stack of n layers of S x S keys, and the views share shadow[slot]'s vertex
    // arrays, setup records, tile tables and lists — they run one after another on the caller's stream; what each view has of its own: its draw list
    // (uploaded in front of its kernels, again in a replay), its block (shadow_cam[slot] holds n of them), and its 16 counter words in
    // shadow_view_ctr[slot].  shadow_view_layers[slot]: one byte per pixel, the view k_shadow_resolve_views took.
    struct ShadowViews {
        uint32_t n = 0;
        float view_proj[AWSM_SHADOW_MAX_VIEWS][16] = {};
        PassList lists[AWSM_SHADOW_MAX_VIEWS];
    } shadow_views[kSlots];
    DevBuf shadow_view_ctr[kSlots], shadow_view_layers[kSlots];

    // AWSM_CLIP_IN_BIN=0 (read at awsm_hip_create): the world geometry pass keeps the earlier path — k_deform_transform writes clip, a cache hit too,
    // every workgroup decides its draw's cache hit itself, k_bin reads clip (A/B measurements, tests)
    bool clip_in_bin = true;

    // awsm_hip_pick_ex / pick_rect / read_pick_map (awsm_pick.cpp): their scratch — the point answer, the per-draw counters, the key
    // table, the entry list, the map — grow-only, per context: the queries are synchronous
    DevBuf pick_scratch;
};

#define HIPCHK(c, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((c), e_ == hipErrorOutOfMemory ? AWSM_ERR_OUT_OF_MEMORY : AWSM_ERR_DEVICE, \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Shared between awsm_hip.cpp and awsm_resources.cpp only: hidden, so that the library's dynamic symbol table does not grow
#define AWSM_HIDDEN __attribute__((visibility("hidden")))

namespace awsm {

AWSM_HIDDEN int fail(AwsmHipCtx* c, int code, const char* fmt, ...);
AWSM_HIDDEN hipError_t sync_shade_streams(AwsmHipCtx* c);
AWSM_HIDDEN int dev_realloc(AwsmHipCtx* c, DevBuf& b, size_t bytes, bool zero);
AWSM_HIDDEN int dev_reserve(AwsmHipCtx* c, DevBuf& b, size_t bytes);                      // grow-only, contents not preserved
AWSM_HIDDEN int stage_alloc(AwsmHipCtx* c, size_t len, uint8_t** out);                    // a pinned pointer valid until the copy enqueued from it has executed
AWSM_HIDDEN int upload_small(AwsmHipCtx* c, void* dst, const void* src, size_t len);
AWSM_HIDDEN int scene_write_barrier(AwsmHipCtx* c, bool is_write = true);
AWSM_HIDDEN int sync_all(AwsmHipCtx* c);
AWSM_HIDDEN uint32_t mip_levels_full(uint32_t w, uint32_t h);

}  // namespace awsm
