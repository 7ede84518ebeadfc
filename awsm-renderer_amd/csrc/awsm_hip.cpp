// awsm_hip.cpp — context, device-memory management and the C-ABI entry points of include/awsm_hip.h.
//
// Sits where the reference's `AwsmRendererWebGpu` wrapper sits (crates/renderer-core/src/methods.rs:
// create_buffer :239, write_buffer :339-431, submit_commands :283-287) but knows the two passes of the hot
// path (crates/renderer/src/render.rs:144-221).  No torch, no WebGPU, no CPU fallback: every entry point
// either drives the HIP kernels or fails with a status code.
// The resource entry points (texture arrays, samplers, environment, cubes, BRDF LUT) are in awsm_resources.cpp; the context is declared in ctx.hpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "bin_record.hpp"
#include "launch.hpp"

using namespace awsm;

namespace {

constexpr int kLeanWgsPerCu = 0;   // measured: the one-wavefront-per-strip grid wins once the geometry kernels fit beside it

// A pass's device state, per frame slot / in the current slot.  The kind is the one way a pass is named: its FrameBufs carry it (FrameBufs::kind),
// its draw list is c->lists[kind].
inline FrameBufs* pass_slots(AwsmHipCtx* c, PassKind kind) {
    FrameBufs* const sets[kPassKinds] = {c->fb, c->tr, c->hud, c->htr, c->shadow};      // in PassKind's order
    return sets[kind];
}
inline FrameBufs& pass_bufs(AwsmHipCtx* c, PassKind kind) { return pass_slots(c, kind)[c->slot]; }
inline FrameBufs& FB(AwsmHipCtx* c) { return c->fb[c->slot]; }      // = pass_bufs(c, kPassWorld)
inline uint32_t samples_of(const AwsmHipCtx* c) { return c->msaa == 4 ? 4u : 1u; }
// the context renders a part of the frame: a row range (awsm_hip_set_shard_rows) or every n-th tile row (awsm_hip_set_shard_bands)
inline bool is_sharded(const AwsmHipCtx* c) { return c->band_n > 1 || (c->y1 != 0 && !(c->y0 == 0 && c->y1 >= c->height)); }
inline hipStream_t shade_stream_of(AwsmHipCtx* c) { return c->overlap ? c->shade_streams[c->slot] : c->stream; }
inline int n_slots(const AwsmHipCtx* c) { return c->overlap ? kSlots : 1; }
inline int prev_slot(const AwsmHipCtx* c) { return (c->slot + kSlots - 1) % kSlots; }
inline uint32_t* handoff_timeouts(AwsmHipCtx* c) { return c->counters_host + 16 + 2 * kSlots; }
inline unsigned long long* trace_slot(AwsmHipCtx* c, int which) { return c->trace_dev ? c->trace_dev + (size_t)which * c->trace_cap + c->frame_serial % c->trace_cap : nullptr; }
// the slot's shading is finished: for the host and the rarely taken waits an event, for the next user of the slot's buffers the flag
inline hipError_t mark_shade_done(AwsmHipCtx* c, hipStream_t ss) {
    if (c->handoff) awsm_launch_handoff_signal(c->handoff_flags + kSlots + c->slot, ++c->shade_sig[c->slot], trace_slot(c, 2), ss);
    else if (c->trace_dev) awsm_launch_handoff_signal(nullptr, 0u, trace_slot(c, 2), ss);
    const hipError_t e = hipEventRecord(c->ev_shade_done[c->slot], ss);
    c->shade_pending[c->slot] = true; c->shade_recorded[c->slot] = true;
    return e;
}
// a shade stream goes on once the OTHER slot's passes have finished (one bound image for both frames, bound halo keys, the composite) —
// or, main_kernel_only, once its k_shade_lean has (its k_shade_todo may still run: per-slot images and lists)
inline hipError_t wait_prev_slot(AwsmHipCtx* c, hipStream_t ss, bool main_kernel_only = false) {
    const int p = prev_slot(c);
    if (c->handoff && c->shade_sig[p]) {
        const bool lean = main_kernel_only && c->lean_flagged[p];
        awsm_launch_handoff_wait(c->handoff_flags + (lean ? 2 * kSlots : kSlots) + p, lean ? c->lean_sig[p] : c->shade_sig[p], c->handoff_budget_ticks, handoff_timeouts(c), c->handoff_timeouts_seen,
                                 c->handoff_poison + c->slot, c->frame_serial, ss);
        return hipSuccess;
    }
    return hipStreamWaitEvent(ss, c->ev_shade_done[p], 0);
}
// the caller's stream goes on once the slot's last opaque (or transparent) pass has finished
inline hipError_t wait_slot_free(AwsmHipCtx* c) {
    if (c->handoff) { awsm_launch_handoff_wait(c->handoff_flags + kSlots + c->slot, c->shade_sig[c->slot], c->handoff_budget_ticks, handoff_timeouts(c), c->handoff_timeouts_seen,
                                               c->handoff_poison + c->slot, c->frame_serial, c->stream); return hipSuccess; }
    return hipStreamWaitEvent(c->stream, c->ev_shade_done[c->slot], 0);
}

// AWSM_HOST_TRACE=<microseconds>: report (stderr) every section of an enqueue call that kept the host longer than that — the HIP runtime
// growing a pool, a full queue, a synchronisation nobody asked for.  Diagnostic; off by default.
struct HostTrace {
    static long threshold() { static long t = [] { const char* e = getenv("AWSM_HOST_TRACE"); return e ? atol(e) : 0L; }(); return t; }
    timespec last{};
    uint32_t serial;
    explicit HostTrace(uint32_t frame_serial) : serial(frame_serial) { if (threshold()) clock_gettime(CLOCK_MONOTONIC, &last); }
    void mark(const char* what) {
        if (!threshold()) return;
        timespec now; clock_gettime(CLOCK_MONOTONIC, &now);
        const long us = (now.tv_sec - last.tv_sec) * 1000000L + (now.tv_nsec - last.tv_nsec) / 1000L;
        if (us >= threshold()) fprintf(stderr, "awsm_hip host trace: frame %u: %s took %ld us\n", serial, what, us);
        last = now;
    }
};

// A hand-off gate that ran out of time has dropped the frame it guarded (fail closed: k_handoff_wait poisons it, its kernels exit).  The host
// learns of it from a pinned counter: count the gates, order the streams with events from here on, and tell the caller once — at the next
// awsm_hip_geometry_pass, awsm_hip_frame_flush or awsm_hip_frame_end, whichever comes first, so that an enqueue-only loop hears of it too.
int handoff_check(AwsmHipCtx* c) {
    if (!c->overlap) return AWSM_OK;
    const uint32_t now = *(volatile uint32_t*)handoff_timeouts(c);
    if (now != c->handoff_timeouts_seen) {
        c->handoff_dropped_frames += now - c->handoff_timeouts_seen;
        c->handoff_timeouts_seen = now;
        c->handoff = false;
        c->handoff_error_pending = true;
        for (FrameBufs& b : c->fb) b.cache_valid = false;      // a dropped frame's kernels wrote nothing: the geometry cache's book-keeping no longer describes the arrays
        c->taa_have = false; c->taa_serial = 0;                // ... and its resolve exited: the image it would have written is no history
    }
    if (!c->handoff_error_pending) return AWSM_OK;
    c->handoff_error_pending = false;
    return fail(c, AWSM_ERR_DEVICE, "a device-side stream hand-off timed out (kernels serialised by a profiler, the streams folded onto one hardware queue, or a stall longer than "
                                    "AWSM_HANDOFF_TIMEOUT_MS): %u gate(s) so far, each dropped the frame it guarded whole — that frame's image was not written; this context orders "
                                    "its streams with events from here on (AWSM_DEVICE_HANDOFF=0 selects them from the start)", c->handoff_dropped_frames);
}

}  // namespace

// what awsm_resources.cpp shares with this file (declared in ctx.hpp)
namespace awsm {

int fail(AwsmHipCtx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->last_error = buf;
    return code;
}

hipError_t sync_shade_streams(AwsmHipCtx* c) {
    for (hipStream_t s : c->shade_streams) if (s) { const hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) return e; }
    for (bool& b : c->shade_recorded) b = false;
    return hipSuccess;
}

int dev_realloc(AwsmHipCtx* c, DevBuf& b, size_t bytes, bool zero) {
    if (b.ptr && b.size == bytes) {
        if (zero) HIPCHK(c, hipMemsetAsync(b.ptr, 0, bytes, c->stream));
        return AWSM_OK;
    }
    if (b.ptr) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, sync_shade_streams(c));
        HIPCHK(c, hipFree(b.ptr));
        b.ptr = nullptr; b.size = 0;
    }
    if (bytes == 0) return AWSM_OK;
    HIPCHK(c, hipMalloc(&b.ptr, bytes));
    b.size = bytes;
    if (zero) HIPCHK(c, hipMemsetAsync(b.ptr, 0, bytes, c->stream));
    return AWSM_OK;
}

int dev_reserve(AwsmHipCtx* c, DevBuf& b, size_t bytes) {   // grow-only, contents not preserved
    if (b.size >= bytes && b.ptr) return AWSM_OK;
    size_t want = std::max(bytes, b.size + b.size / 2);
    return dev_realloc(c, b, want, false);
}

constexpr size_t kKernelUploadMax = 256u << 10;   // larger uploads go to the copy engine

// returns a pinned pointer valid until the copy enqueued from it has executed
int stage_alloc(AwsmHipCtx* c, size_t len, uint8_t** out) {
    len = (len + 255) & ~size_t(255);
    if (len > c->stage_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->stage) HIPCHK(c, hipHostFree(c->stage));
        c->stage = nullptr;
        size_t cap = std::max<size_t>(len * 2, 8u << 20);
        HIPCHK(c, hipHostMalloc((void**)&c->stage, cap, hipHostMallocDefault));
        c->stage_cap = cap; c->stage_head = 0;
    }
    if (c->stage_head + len > c->stage_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // everything enqueued from the ring has been consumed
        c->stage_head = 0;
    }
    *out = c->stage + c->stage_head;
    c->stage_head += len;
    return AWSM_OK;
}

int upload_small(AwsmHipCtx* c, void* dst, const void* src, size_t len) {
    uint8_t* st;
    int rc = stage_alloc(c, len, &st);
    if (rc) return rc;
    memcpy(st, src, len);
    if (len <= kKernelUploadMax && (len & 3u) == 0 && ((uintptr_t)dst & 3u) == 0 && ((uintptr_t)st & 3u) == 0) {
        awsm_launch_upload_words(dst, st, (uint32_t)(len >> 2), c->stream);   // pinned memory is device-visible at the same address
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemcpyAsync(dst, st, len, hipMemcpyHostToDevice, c->stream));
    }
    return AWSM_OK;
}

// Overlap mode: anything that writes scene state the opaque pass reads (every buffer but the camera, whose snapshot the
// geometry pass takes; textures; samplers; environment; the DevScene table) is ordered after the opaque passes still in
// flight on the shade stream.  A frame therefore always shades the scene as it was when it was submitted.
int scene_write_barrier(AwsmHipCtx* c, bool is_write) {
    if (is_write) c->write_seq++;
    if (!c->overlap) return AWSM_OK;
    for (int s = 0; s < kSlots; s++)
        if (c->shade_pending[s]) { HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_shade_done[s], 0)); c->shade_pending[s] = false; }
    return AWSM_OK;
}
int sync_all(AwsmHipCtx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, sync_shade_streams(c));
    for (bool& b : c->shade_pending) b = false;
    return AWSM_OK;
}

uint32_t mip_levels_full(uint32_t w, uint32_t h) {   // calculate_mipmap_levels (renderer-core/src/texture/mipmap.rs:60-62)
    uint32_t m = std::max(w, h), n = 0;
    while (m > 1u) { m >>= 1; n++; }
    return n + 1u;
}

}  // namespace awsm

namespace {

void shard(const AwsmHipCtx* c, uint32_t* y0, uint32_t* y1) {
    *y0 = c->y0; *y1 = c->y1;
    if (*y1 == 0 || *y1 > c->height) *y1 = c->height;
    if (*y0 > *y1) *y0 = *y1;
}

// Geometry cache: remember what was written to the buffers k_deform_transform reads (call after the write got its write_seq).
void log_dirty(AwsmHipCtx* c, AwsmBuf which, size_t lo, size_t hi) {
    if (c->geometry_cache) c->dirty_log.log((uint32_t)which, lo, hi, c->write_seq);
}

int sync_scene(AwsmHipCtx* c) {
    if (!c->scene_dirty) return AWSM_OK;
    c->write_seq++;
    { int rcb = scene_write_barrier(c, false); if (rcb) return rcb; }
    for (int i = 0; i < AWSM_BUF_COUNT; i++) c->scene.buf[i] = (const uint8_t*)c->bufs[i].ptr;
    c->scene.lut_rg16f = (const uint16_t*)c->lut.ptr;
    int rc = upload_small(c, c->scene_dev, &c->scene, sizeof(DevScene));
    if (rc) return rc;
    c->scene_dirty = false;
    c->scene_uploads++;
    return AWSM_OK;
}

// The per-pass members of a frame — whose draw list, transformed vertices, setup records, tile tables, lists, counters and keys the kernels of a
// pass work on — from that pass's FrameBufs.  The ONE place they are set: a new per-pass buffer is added here.
void bind_pass(FrameDev& f, const FrameBufs& b) {
    f.bin_capacity = b.bin_capacity;
    f.draws = (const DrawDev*)b.draws_dev.ptr;
    f.clip = (float4*)b.clip.ptr; f.nrm = (float4*)b.nrm.ptr; f.tan = (float4*)b.tan.ptr;
    f.tri_info = (uint32_t*)b.tri_flags.ptr;
    f.tri_rec = (TriRec*)b.tri_rec.ptr;
    f.tile_count = (uint32_t*)b.tile_count.ptr; f.tile_offset = (uint32_t*)b.tile_offset.ptr;
    f.tile_cursor = (uint32_t*)b.tile_cursor.ptr; f.bin_list = (uint32_t*)b.bin_list.ptr;
    f.tile_order = (uint32_t*)b.tile_order.ptr;
    f.scan_tmp = (uint32_t*)b.scan_tmp.ptr;
    f.tile_split = (uint32_t*)b.tile_split.ptr; f.raster_scratch = (unsigned long long*)b.raster_scratch.ptr;
    f.raster_extra_cap = b.raster_extra_cap; f.raster_slot_cap = b.raster_slot_cap;
    f.big_list = (uint32_t*)b.big_list.ptr;
    f.counters = (uint32_t*)b.counters.ptr;
    f.vis = (unsigned long long*)b.vis.ptr;
}

// Which frame a FrameDev describes.  hud_keys: the frame has hud geometry and the pass looks at its keys (the opaque pass leaves those pixels
// cleared); merged: the hud draws follow the world's in one rank space (AwsmHipCtx::hud_merged) — with hud_keys the pass sees the merged keys
// and the combined list, and in any case the lean route's 32-bit offsets must hold for both passes' triangles.
struct FrameView { bool hud_keys, merged; };
inline FrameView world_view() { return {false, false}; }      // the world pass's own: no merged hud keys, no hud ranks
inline FrameView frame_view(const AwsmHipCtx* c) { return {c->hud_geometry_done, c->hud_merged}; }      // the frame as the passes behind the HUD geometry pass see it

void fill_frame(AwsmHipCtx* c, FrameDev* f, FrameView view) {
    memset(f, 0, sizeof *f);
    const PassList& world = c->lists[kPassWorld];
    const PassList& hud = c->lists[kPassHud];
    uint32_t y0, y1;
    shard(c, &y0, &y1);
    f->width = c->width; f->height = c->height; f->y0 = y0; f->y1 = y1; f->sy0 = y0; f->sy1 = y1;
    if (c->msaa && (y0 > 0 || y1 < c->height)) {   // MSAA edge detector reads the rows next to the shard: rasterise one halo row each side
        f->y0 = y0 > 0 ? y0 - 1 : 0; f->y1 = std::min(c->height, y1 + 1);
    }
    f->tiles_x = (c->width + kTile - 1) / kTile;
    f->band_n = 1; f->band_r = 0; f->out_compact = 0;
    f->tile_row0 = f->y0 >> kTileShift;
    f->tiles_y = (f->y1 > f->y0) ? ((f->y1 + kTile - 1) / kTile - f->tile_row0) : 0;
    if (c->band_n > 1) {   // band mode: every band_n-th 32-row tile row, starting at band_r (row range is the full frame)
        const uint32_t rows_full = (c->height + kTile - 1) / kTile;
        f->band_n = c->band_n; f->band_r = c->band_r; f->out_compact = c->band_compact;
        f->tile_row0 = c->band_r;
        f->tiles_y = c->band_r < rows_full ? (rows_full - c->band_r + c->band_n - 1) / c->band_n : 0;
    }
    f->n_draws = (uint32_t)world.draws.size();
    f->total_tris = world.total_tris; f->total_verts = 3u * world.total_tris;
    bind_pass(*f, FB(c));
    f->draw_shade = (DrawShadeDev*)FB(c).draw_shade.ptr;
    f->tex_slots = (TexSlotDev*)FB(c).tex_slots.ptr;
    f->draw_mat = (DrawMatDev*)FB(c).draw_mat.ptr;
    // The lean opaque route (k_shade_lean): frames whose per-pixel key / per-triangle / per-vertex / attribute byte offsets fit 32 bits
    const bool lean_ok = !(c->flags & AWSM_CFG_GENERAL_SHADE_ONLY) && (uint64_t)c->width * c->height * (c->msaa == 4 ? 32u : 8u) < (1ull << 32) && (c->msaa == 0 || (c->msaa_edge_bits[c->slot].ptr && c->msaa_cells[c->slot].ptr)) && FB(c).tri_shade.ptr && FB(c).draw_lean.ptr && c->shade_todo[c->slot].ptr && ((uint64_t)world.total_tris + (view.merged ? hud.total_tris : 0u)) * kTriRecBytes < (1ull << 32) &&
                         c->bufs[AWSM_BUF_ATTR_DATA].size < (1ull << 32) - 64;
    f->tri_shade = lean_ok ? (uint4*)FB(c).tri_shade.ptr : nullptr;
    f->attr_data_bytes = (uint32_t)std::min<size_t>(c->bufs[AWSM_BUF_ATTR_DATA].size, 0xFFFFFFFFu);
    f->draw_lean = lean_ok ? (LeanDrawDev*)FB(c).draw_lean.ptr : nullptr;
    f->shade_todo = (uint32_t*)c->shade_todo[c->slot].ptr;
    f->shade_todo_cap = f->shade_todo ? (uint32_t)(c->shade_todo[c->slot].size / 4 - 4 - 1024) : 0u;
    f->lean_next = f->shade_todo ? f->shade_todo + 4 + f->shade_todo_cap : nullptr;
    f->lean_grid = c->lean_grid;
#ifdef AWSM_STAMP
    {
        static unsigned long long* stamps = nullptr;
        if (!stamps && hipMalloc((void**)&stamps, 4ull * 16384 * 8 * 8) == hipSuccess) (void)hipMemset(stamps, 0, 4ull * 16384 * 8 * 8);
        f->stamps = stamps;
        static bool told = false;
        if (!told) { told = true; FILE* fp = fopen("/tmp/awsm_stamps_ptr", "w"); if (fp) { fprintf(fp, "%llu\n", (unsigned long long)(uintptr_t)stamps); fclose(fp); } }
    }
#endif
    f->poison = c->handoff_poison ? c->handoff_poison + c->slot : nullptr;
    f->host_bin_status = c->counters_host + 16 + 2 * c->slot;
    f->frame_serial = c->frame_serial;
    f->camera = (const uint8_t*)FB(c).camera.ptr;      // the snapshot the geometry pass took: every kernel of a frame, lean or general, sees the camera the frame was submitted with
    f->camera_snap = nullptr; f->camera_snap_words = 0;
    memcpy(f->pix2view, FB(c).pix2view, sizeof f->pix2view); memcpy(f->view_rot, FB(c).view_rot, sizeof f->view_rot); memcpy(f->cam_pos, FB(c).cam_pos, sizeof f->cam_pos);
    memcpy(f->ortho_view_dir, FB(c).ortho_view_dir, sizeof f->ortho_view_dir); f->cam_ortho = FB(c).cam_ortho;
    f->msaa = c->msaa;
    f->msaa_color0 = (float4*)c->msaa_color0[c->slot].ptr;
    f->msaa_edges = (uint32_t*)c->msaa_edges[c->slot].ptr;
    f->msaa_edge_bits = (lean_ok && c->msaa == 4) ? (unsigned long long*)c->msaa_edge_bits[c->slot].ptr : nullptr;
    f->msaa_cells = (uint2*)c->msaa_cells[c->slot].ptr;
    f->hud_vis = view.hud_keys ? (const unsigned long long*)c->hud[c->slot].vis.ptr : nullptr;
    f->hud_draws = (const DrawDev*)c->hud[c->slot].draws_dev.ptr; f->hud_tri_info = (const uint32_t*)c->hud[c->slot].tri_flags.ptr;
    if (view.hud_keys && view.merged) {      // one rank space: the hud draws behind the world's; the opaque pass sees the merged keys
        f->n_draws = (uint32_t)c->hud_combined.size();
        f->total_tris = world.total_tris + hud.total_tris; f->total_verts = 3u * f->total_tris;
        f->vis = (unsigned long long*)c->merged_vis[c->slot].ptr;
        f->hud_draws = f->draws; f->hud_tri_info = f->tri_info;      // (the picker: hud keys name global ranks)
    }
    f->hud_pass = 0;
    f->msaa_halo = (const unsigned long long*)c->msaa_halo;
    f->halo_bands = c->band_n > 1 ? ((c->height + kTile - 1) / kTile + c->band_n - 1) / c->band_n : 0u;
    f->out_rgba16f = (uint16_t*)(c->bound_out ? (uint8_t*)c->bound_out - (size_t)c->out_first_row * c->width * 8 : c->out16[c->slot].ptr);   // kernels address by absolute row
    f->out_rgba32f = (float*)c->out32[c->slot].ptr;
    f->lights_pre = (float4*)c->lights_pre[c->slot].ptr;
    f->lights_cap = (uint32_t)(c->lights_pre[c->slot].size / 32);
}

// standard.wgsl:17-27 as one matrix: view_h = inv_proj * clip with clip = (2 (px + 0.5) / W - 1, 1 - 2 (py + 0.5) / H, depth, 1).  Composed in f64 from the f32
// matrices of the camera UBO as the caller wrote it (camera.rs:169-219: inv_proj at 256, inv_view at 320, position at 384, proj at 64), once per frame at
// awsm_hip_geometry_pass — the camera the frame is shaded with is the camera it was submitted with.
void compose_pixel_to_view(AwsmHipCtx* c, FrameBufs& b) {
    float cam[128];
    memcpy(cam, c->camera_host, 512);
    const float* proj = cam + 16; const float* inv_proj = cam + 64; const float* inv_view = cam + 80;
    const double W = (double)c->width, H = (double)c->height;
    // A: (px, py, depth, 1) -> clip, column-major
    const double A[16] = {2.0 / W, 0, 0, 0,   0, -2.0 / H, 0, 0,   0, 0, 1, 0,   1.0 / W - 1.0, 1.0 - 1.0 / H, 0, 1};
    for (int col = 0; col < 4; col++) for (int row = 0; row < 4; row++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) s += (double)inv_proj[k * 4 + row] * A[col * 4 + k];
        b.pix2view[col * 4 + row] = (float)s;
    }
    for (int col = 0; col < 3; col++) for (int row = 0; row < 3; row++) b.view_rot[col * 3 + row] = inv_view[col * 4 + row];
    for (int i = 0; i < 3; i++) b.cam_pos[i] = cam[96 + i];
    b.cam_ortho = proj[15] > 0.9f ? 1u : 0u;      // standard.wgsl:38: proj[3][3]
    const double vx = inv_view[8], vy = inv_view[9], vz = inv_view[10], l = std::sqrt(vx * vx + vy * vy + vz * vz);
    b.ortho_view_dir[0] = l > 0.0 ? (float)(vx / l) : 0.0f; b.ortho_view_dir[1] = l > 0.0 ? (float)(vy / l) : 0.0f; b.ortho_view_dir[2] = l > 0.0 ? (float)(vz / l) : 1.0f;
}

int record(AwsmHipCtx* c, int which, hipStream_t s = nullptr) {
    if (!c->stage_timers) { c->ev_valid[which] = false; return AWSM_OK; }     // each record is a ~5 us bubble between two kernels
    HIPCHK(c, hipEventRecord(c->ev[which], s ? s : c->stream));
    c->ev_valid[which] = true;
    return AWSM_OK;
}

AwsmHipCtx::ResolveKey resolve_key(AwsmHipCtx* c, const FrameDev& f) {
    AwsmHipCtx::ResolveKey k;
    memset(&k, 0, sizeof k);      // padding too: the keys are compared bytewise
    k.write_seq = c->write_seq + (c->scene_dirty ? 1u : 0u); k.draws_version = FB(c).draws_version;
    k.ptrs[0] = f.draw_shade; k.ptrs[1] = f.draw_mat; k.ptrs[2] = f.tex_slots; k.ptrs[3] = f.draw_lean; k.ptrs[4] = f.lights_pre;
    k.n_draws = f.n_draws; k.mipmap = c->last_opaque.mipmap; k.has_opaque = c->last_opaque.has_opaque; k.lights_cap = f.lights_cap;
    return k;
}
bool resolve_stale(AwsmHipCtx* c, const FrameDev& f) {
    const AwsmHipCtx::ResolveKey k = resolve_key(c, f);
    return memcmp(&k, &c->resolved[c->slot], sizeof k) != 0;
}

// The geometry cache's part of the world pass's frame: which draws may keep what the slot's arrays hold (frame_params.hpp).
void fill_geometry_cache(AwsmHipCtx* c, FrameDev* f, bool replay) {
    FrameBufs& b = FB(c);
    f->wcache = (float4*)b.wcache.ptr;
    f->cache_on = 0; f->prev_draws = nullptr; f->prev_n_draws = 0; f->n_dirty = 0; f->cache_serial = b.cache_serial;
    if (!c->geometry_cache || replay || !b.cache_valid || !b.wcache.ptr || b.cache_had_tri_shade != (f->tri_shade != nullptr)) return;
    // the ranges written since the slot's arrays were computed, merged per buffer; too many: one bounding range per buffer; still too many (or a write that
    // invalidates every draw): no cache this frame
    std::vector<DirtyRange> r;
    if (!c->dirty_log.ranges_since(b.cache_seq, kMaxDirtyRanges, r)) return;
    for (size_t i = 0; i < r.size(); i++) { f->dirty[i][0] = r[i].buf; f->dirty[i][1] = r[i].lo; f->dirty[i][2] = r[i].hi; }
    f->n_dirty = (uint32_t)r.size();
    f->prev_draws = (const DrawDev*)(b.cached_is_prev ? b.draws_prev.ptr : b.draws_dev.ptr);
    f->prev_n_draws = b.cached_n_draws;
    f->cache_on = f->prev_draws ? 1u : 0u;
}


// The binning chain of a pass: count -> big(0) -> scan -> fill -> big(1).  A pass without triangles only scans (k_bin_scan clears tile_cursor and
// orders the tiles for the raster / forward kernels).  Whether the chain runs at all, and what stands around it, is the caller's business.
inline void enqueue_binning(const FrameDev& f, bool has_tris, hipStream_t s) {
    if (has_tris) { awsm_launch_bin_count(&f, s); awsm_launch_bin_big(&f, 0, s); }
    awsm_launch_bin_scan(&f, s);
    if (has_tris) { awsm_launch_bin_fill(&f, s); awsm_launch_bin_big(&f, 1, s); }
}
// A pass without triangles launches no k_deform_transform, which otherwise clears counters + tile_count (k_bin_scan clears tile_cursor).
// counters: the words the pass counts in — the FrameBufs' own, or those of one view of the shadow pass.
int clear_empty_pass(AwsmHipCtx* c, const FrameBufs& b, uint32_t* counters, uint32_t n_tiles, hipStream_t s) {
    HIPCHK(c, hipMemsetAsync(counters, 0, kCtrWords * sizeof(uint32_t), s));
    HIPCHK(c, hipMemsetAsync(counters + 12, 0, 2 * sizeof(uint32_t), s));
    if (n_tiles) HIPCHK(c, hipMemsetAsync(b.tile_count.ptr, 0, n_tiles * sizeof(uint32_t), s));
    return AWSM_OK;
}

// The slot's last world pass formed its clip positions in the binning and stored none (FrameDev::clip_from_world): form them now, from the slot's
// wcache and the camera snapshot that frame was submitted with, into the slot's clip buffer (awsm_hip_read_transformed; and in front of anything
// that replaces the snapshot outside a geometry pass).  Enqueued on the caller's stream, which the world pass ran on.
int materialize_clip(AwsmHipCtx* c) {
    FrameBufs& b = FB(c);
    if (!b.clip_in_bin_last) return AWSM_OK;
    const uint32_t n = 3u * c->lists[kPassWorld].total_tris;
    if (n && b.wcache.ptr && b.clip.ptr && b.camera.ptr) {
        FrameDev f;
        memset(&f, 0, sizeof f);
        f.wcache = (float4*)b.wcache.ptr; f.clip = (float4*)b.clip.ptr; f.camera = (const uint8_t*)b.camera.ptr;
        f.total_verts = n; f.clip_from_world = kClipReadBack;      // (launch.hpp: the transform's wrapper runs k_clip_from_world alone)
        awsm_launch_transform(c->scene_dev, &f, 0, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    b.clip_in_bin_last = false;      // the buffer now holds that frame's clip positions
    return AWSM_OK;
}

// replay: the frame's geometry pass is enqueued again (a bin list that overflowed, world arrays that moved under the hud pass): the camera snapshot the first
// enqueue took stays — pix2view / cam_pos were composed from that camera at awsm_hip_geometry_pass — and the geometry cache is not consulted.
int enqueue_geometry(AwsmHipCtx* c, bool replay = false) {
    HostTrace ht(c->frame_serial);
    const PassList& world = c->lists[kPassWorld];
    FrameDev f;
    fill_frame(c, &f, world_view());
    fill_geometry_cache(c, &f, replay);
    f.block_draw = FB(c).block_map_valid ? (const uint32_t*)FB(c).block_map.ptr : nullptr;
    // AwsmFrameStats.geometry_cache_blocks: marked only when stage times are asked for too (a plain store per workgroup, counted by frame_end on the host)
    f.cache_mark = (c->stage_timers && FB(c).cache_mark.size >= (size_t)world.n_blocks * 4) ? (uint32_t*)FB(c).cache_mark.ptr : nullptr;
    const uint32_t n_tiles = f.tiles_x * f.tiles_y;
    int rc = sync_scene(c);
    if (rc) return rc;
    ht.mark("geometry: sync_scene");
    // this slot's buffers were last read by the opaque pass kSlots frames ago (already ordered by awsm_hip_geometry_pass; a replay comes here directly)
    if (c->overlap && c->shade_pending[c->slot]) { HIPCHK(c, wait_slot_free(c)); c->shade_pending[c->slot] = false; }
    // the camera the frame is shaded with = the camera it was submitted with, in every mode: the lean kernel's pix2view was composed from the caller's
    // bytes at awsm_hip_geometry_pass, the general kernels and the MSAA detector read this snapshot — a camera write between the two passes of a frame
    // cannot give its strips two cameras
    // (copied by k_deform_transform when the frame has geometry: a 512-byte hipMemcpyAsync costs the stream 18 us of gap + copy)
    if (c->bufs[AWSM_BUF_CAMERA].ptr && !replay) {
        const size_t cam_bytes = std::min<size_t>(512, c->bufs[AWSM_BUF_CAMERA].size);
        if (world.total_tris && n_tiles) { f.camera_snap = (uint32_t*)FB(c).camera.ptr; f.camera_snap_words = (uint32_t)(cam_bytes / 4); }
        else HIPCHK(c, hipMemcpyAsync(FB(c).camera.ptr, c->bufs[AWSM_BUF_CAMERA].ptr, cam_bytes, hipMemcpyDeviceToDevice, c->stream));
    }
    if (c->overlap) {
        // everything the per-draw resolve of this frame reads (draw list, scene buffers) is on the stream by now — an event only when a resolve
        // will run (resolve_key): a record packet costs the caller's stream ~19 us between the camera upload and the transform kernel
        c->uploads_recorded[c->slot] = false;
        if (resolve_stale(c, f)) { HIPCHK(c, hipEventRecord(c->ev_uploads[c->slot], c->stream)); c->uploads_recorded[c->slot] = true; }
        c->geom_write_seq[c->slot] = c->write_seq;
    }
    ht.mark("geometry: slot wait + upload event");
    const bool has_geometry = world.total_tris && n_tiles;
    if (!has_geometry && (rc = clear_empty_pass(c, FB(c), (uint32_t*)FB(c).counters.ptr, n_tiles, c->stream))) return rc;
    if (c->trace_dev) awsm_launch_handoff_signal(nullptr, 0u, trace_slot(c, 0), c->stream);
    if ((rc = record(c, EV_START))) return rc;
    // Measurement aid (tools/knockout.sh; static camera only): from the ninth frame on leave out the raster (4), the binning launches as well (6) or
    // the whole pass (7) — the slot's buffers then keep the previous frames' keys, the opaque pass does the same work, and the frame rate
    // says what each stage's kernels take from the kernels they run beside.
#ifdef AWSM_DEBUG_SWITCHES      // tools/build_variants.sh h_debug "-DAWSM_DEBUG_SWITCHES": not in the product library
    static const int knockout_env = getenv("AWSM_DEBUG_KNOCKOUT") ? atoi(getenv("AWSM_DEBUG_KNOCKOUT")) : 0;
    const int knockout = c->frame_serial > 8 ? knockout_env : 0;
#else
    const int knockout = 0;
#endif
    // Clip positions formed in the binning (FrameDev::clip_from_world): a pass with a wcache and a snapshot that covers view_proj (bytes 128..191 of
    // the camera block; in a replay the first enqueue's snapshot stays).  With a cache to consult and a block map the hit is decided once per draw.
    f.clip_from_world = (c->clip_in_bin && f.wcache && FB(c).camera.ptr && c->bufs[AWSM_BUF_CAMERA].ptr && c->bufs[AWSM_BUF_CAMERA].size >= 192) ? 1u : 0u;
    f.draw_hit_at = (f.clip_from_world && f.cache_on && f.block_draw && (size_t)FB(c).draw_hit_at + f.n_draws <= FB(c).block_map.size / 4) ? FB(c).draw_hit_at : 0u;
    // ... and the fill pass of the binning reads the count pass's compact records, where the frame's tile coordinates fit them (bin_record.hpp)
    f.bin_rec_at = (c->clip_in_bin && bin_rec_fits(f.tiles_x, f.tiles_y) && ((size_t)FB(c).bin_rec_at + f.total_tris) * 8 <= FB(c).tri_rec.size) ? FB(c).bin_rec_at : 0u;
    if (has_geometry && !(knockout & 1)) { awsm_launch_transform(c->scene_dev, &f, world.n_blocks, c->stream); FB(c).clip_in_bin_last = f.clip_from_world != 0u; }
    if ((rc = record(c, EV_TRANSFORM))) return rc;
    ht.mark("geometry: transform launch");
    if (n_tiles && !(knockout & 2)) enqueue_binning(f, world.total_tris != 0, c->stream);
    if ((rc = record(c, EV_BIN))) return rc;
    ht.mark("geometry: bin launches");
    if (n_tiles && !(knockout & 4)) awsm_launch_raster(&f, c->stream);
    if ((rc = record(c, EV_RASTER))) return rc;
    ht.mark("geometry: raster launch");
    HIPCHK(c, hipGetLastError());
    {   // the slot's arrays now hold this list's world positions / N / T / per-triangle words (all of them: hits kept theirs, misses were recomputed)
        FrameBufs& b = FB(c);
        b.cache_valid = has_geometry && !(knockout & 1) && b.wcache.ptr != nullptr;
        b.cached_n_draws = (uint32_t)world.draws.size(); b.cached_is_prev = false;
        b.cache_had_tri_shade = f.tri_shade != nullptr;
        b.cache_seq = c->write_seq; b.cache_serial = c->frame_serial;
        // entries every slot has seen are of no further use
        uint64_t oldest = ~0ull;
        for (int sl = 0; sl < n_slots(c); sl++) oldest = std::min(oldest, c->fb[sl].cache_valid ? c->fb[sl].cache_seq : c->write_seq);
        c->dirty_log.prune(oldest);
    }
    return AWSM_OK;
}

int enqueue_opaque(AwsmHipCtx* c) {
    HostTrace ht(c->frame_serial);
    FrameDev f;
    fill_frame(c, &f, frame_view(c));
    f.has_opaque = c->last_opaque.has_opaque;
    f.mipmap = c->last_opaque.mipmap;
    f.aniso = (c->flags & AWSM_CFG_ANISOTROPIC) ? 1u : 0u;
    if (c->bound_out) {
        if (c->out_rows_mode) {   // a row strip's own buffer: rows [first_row, first_row + bytes / (width * 8))
            if (f.out_compact || f.sy0 < c->out_first_row || (size_t)(f.sy1 - c->out_first_row) * c->width * 8 > c->bound_out_bytes)
                return fail(c, AWSM_ERR_INVALID_ARGUMENT, "opaque_pass: bound output starts at row %u and holds %zu bytes, the shard shades rows [%u, %u)", c->out_first_row, c->bound_out_bytes, f.sy0, f.sy1);
        } else {
            const size_t need = (f.out_compact ? (size_t)f.tiles_y * kTile : (size_t)c->height) * c->width * 8;
            if (c->bound_out_bytes < need) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "opaque_pass: bound output holds %zu bytes, this shard layout writes %zu", c->bound_out_bytes, need);
        }
    }
    int rc = sync_scene(c);
    if (rc) return rc;
    hipStream_t ss = shade_stream_of(c);
    // The per-draw resolve only needs the uploads, not the geometry pass, and nothing of the previous frame: its outputs are per frame
    // slot.  In overlap mode it goes first onto this slot's shade stream — idle since the frame before last — and so runs beside the
    // previous frame's opaque pass (on the single shade stream of round 1 it sat between two frames' shading kernels: todo -> 14 us gap ->
    // resolve 30 us -> gap -> lean; on the caller's stream it would lengthen the geometry chain).  No stream of its own: the process has
    // four hardware queues (GPU_MAX_HW_QUEUES), and a fifth stream shares one of them with another stream — seen as 25-30 us of idle GPU
    // at every frame boundary.  A scene write between the two passes falls back to the late order.
    // (with stage timers on it always runs: EV_SHADE_BEGIN must sit behind a kernel of this stream, not right behind the cross-stream wait — see below)
    const bool want_resolve = f.sy1 > f.sy0 && f.has_opaque && (resolve_stale(c, f) || c->stage_timers);
    if (want_resolve) c->resolved[c->slot] = resolve_key(c, f);
    // (With stage timers on the late order stays: an event recorded right behind a cross-stream wait is stamped when the wait is
    // consumed, not when it is satisfied, and ms_shade would include the tail of the raster kernel — seen: 0.40 instead of 0.36 ms.)
    const bool early = c->uploads_recorded[c->slot] && c->overlap && !c->stage_timers && want_resolve && c->geometry_done && c->geom_write_seq[c->slot] == c->write_seq;
    if (early) {      // on this slot's shade stream, ahead of the wait for the geometry pass
        HIPCHK(c, hipStreamWaitEvent(ss, c->ev_uploads[c->slot], 0));
        awsm_launch_resolve_draws(c->scene_dev, &f, ss);
    }
    ht.mark("opaque: sync_scene + early resolve");
    if (c->overlap) {   // the shade stream picks up where the caller's stream is now (geometry pass + uploads of this frame)
        if (c->handoff) {
            ++c->geom_sig[c->slot];
            if (c->handoff_test_drop) c->handoff_test_drop--;
            else awsm_launch_handoff_signal(c->handoff_flags + c->slot, c->geom_sig[c->slot], trace_slot(c, 1), c->stream);
            awsm_launch_handoff_wait(c->handoff_flags + c->slot, c->geom_sig[c->slot], c->handoff_budget_ticks, handoff_timeouts(c), c->handoff_timeouts_seen, c->handoff_poison + c->slot, c->frame_serial, ss);
        } else {
            if (c->trace_dev) awsm_launch_handoff_signal(nullptr, 0u, trace_slot(c, 1), c->stream);
            HIPCHK(c, hipEventRecord(c->ev_geom_done[c->slot], c->stream));
            HIPCHK(c, hipStreamWaitEvent(ss, c->ev_geom_done[c->slot], 0));
        }
        // ... and behind the previous frame's opaque pass on the other slot's shade stream.  Where the two share something — one bound output image
        // for both, the halo keys a caller bound for MSAA + bands — behind all of it.  Otherwise (the library's own images, or a caller alternating
        // between two bound ones: images, per-draw records and todo lists are per slot) behind its main kernel only: frame i + 1's
        // k_shade_lean starts when frame i's has ended, beside frame i's k_shade_todo.  Not earlier, although nothing shared would forbid it:
        // with two frame slots the geometry pass of frame i + 2 waits for frame i's shading, and two opaque passes running into each other
        // push that out — measured 2,780 frames/s free-running against 2,980 in step.  (Last of the waits on purpose: the first two are
        // consumed while the previous frame still shades.)
        const uint8_t* lo = (const uint8_t*)c->bound_out; const uint8_t* hi = lo ? lo + c->bound_out_bytes : nullptr;
        const int p = prev_slot(c);
        const bool same_image = lo && c->slot_out_lo[p] && lo < c->slot_out_hi[p] && c->slot_out_lo[p] < hi;
        if (c->shade_recorded[p]) HIPCHK(c, wait_prev_slot(c, ss, !(same_image || (c->msaa != 0 && c->msaa_halo))));
        c->slot_out_lo[c->slot] = lo; c->slot_out_hi[c->slot] = hi;
    }
    ht.mark("opaque: hand-off launches");
    if (want_resolve && !early) awsm_launch_resolve_draws(c->scene_dev, &f, ss);
    if ((rc = record(c, EV_SHADE_BEGIN, ss))) return rc;      // after the resolve: ms_shade is the shading kernels alone
    c->ev_valid[EV_SHADE_LEAN] = false;
    c->lean_flagged[c->slot] = false;
    if (c->overlap && c->handoff && f.sy1 > f.sy0 && awsm_shade_is_lean(&f)) {
        f.lean_done_flag = c->handoff_flags + 2 * kSlots + c->slot; f.lean_done_serial = ++c->lean_sig[c->slot];
        c->lean_flagged[c->slot] = true;
    }
    if (f.sy1 > f.sy0) {
        awsm_launch_shade(c->scene_dev, &f, ss);
        // the lean kernel alone (AwsmFrameStats.ms_shade_lean): one more event, only when stage times are asked for
        if (c->stage_timers && awsm_shade_is_lean(&f) && (rc = record(c, EV_SHADE_LEAN, ss))) return rc;
        (void)awsm_launch_shade_todo(c->scene_dev, &f, ss);
    }
    // shadows, with the record the frame's shadow pass was submitted with: behind the shading kernels and in FRONT of the occlusion below — both
    // multiply the same image and each rounds to f16, so the order is part of the contract — and in front of the shade-done signal:
    // the kernel reads the slot's keys and the slot's map, which the slot's next geometry and shadow passes overwrite.  A replay comes through here
    // again behind shading kernels that wrote every pixel anew.
    const AwsmHipCtx::ShadowState& sh = c->shadow_pass[c->slot];
    if (sh.on && c->shadow_px[c->slot] && f.has_opaque && f.sy1 > f.sy0) {
        const size_t px = (size_t)c->width * c->height;
        ShadowViewsArgs av{};      // (the launch wrapper is handed the leading member: frame_params.hpp)
        ShadowArgs& a = av.base;
        const AwsmHipCtx::ShadowViews& views = c->shadow_views[c->slot];
        av.n_views = views.n; av.view = (unsigned char*)c->shadow_view_layers[c->slot].ptr;
        memcpy(av.view_proj, views.view_proj, sizeof av.view_proj);
        a.width = c->width; a.height = c->height;
        a.vis = (const unsigned long long*)FB(c).vis.ptr;       // the WORLD's keys (see below)
        a.camera = (const float*)f.camera;
        a.map = (const uint32_t*)c->shadow[c->slot].vis.ptr; a.map_size = sh.p.map_size; a.pcf_radius = (int32_t)sh.p.pcf_radius;
        memcpy(a.light_view_proj, sh.light_view_proj, sizeof a.light_view_proj); memcpy(a.light, sh.p.light, sizeof a.light);
        a.bias = sh.p.bias; a.slope_bias = sh.p.slope_bias; a.max_slope = sh.p.max_slope; a.strength = sh.p.strength; a.facing_fade = sh.p.facing_fade;
        a.visibility = (float*)c->shadow_layers[c->slot].ptr; a.multiplier = a.visibility + px;
        a.out16 = (uint2*)f.out_rgba16f; a.out32 = (float4*)f.out_rgba32f;
        a.poison = f.poison; a.frame_serial = f.frame_serial;
        awsm_launch_shadow_resolve(&a, samples_of(c), ss);
    }
    // screen-space ambient occlusion, with the record this pass was submitted with: behind the shading kernels — it modulates their image in place —
    // and in front of the shade-done signal below: it reads the slot's keys, which the slot's next geometry pass overwrites.  A replay
    // (awsm_hip_frame_end) comes through here again behind shading kernels that wrote every pixel anew, so the image is modulated once.
    const AwsmHipCtx::SsaoState& so = c->ssao_pass[c->slot];
    if (so.on && f.has_opaque && f.sy1 > f.sy0) {
        const size_t px = (size_t)c->width * c->height;
        SsaoArgs sa{};
        sa.width = c->width; sa.height = c->height;
        sa.vis = (const unsigned long long*)FB(c).vis.ptr;      // the WORLD geometry pass's own buffer — not merged_vis, which the opaque pass itself reads in an MSAA frame with hud meshes
        sa.camera = (const float*)f.camera;
        sa.radius = so.p[0]; sa.intensity = so.p[1]; sa.bias = so.p[2]; sa.strength = so.p[3];
        sa.ao_raw = (float*)c->ssao_layers[c->slot].ptr; sa.ao_smoothed = sa.ao_raw + px; sa.view_z = sa.ao_raw + 2 * px;
        sa.out16 = (uint2*)f.out_rgba16f; sa.out32 = (float4*)f.out_rgba32f;
        sa.poison = f.poison; sa.frame_serial = f.frame_serial;
        awsm_launch_ssao(&sa, samples_of(c), ss);
    }
    if ((rc = record(c, EV_SHADE, ss))) return rc;      // behind the SSAO kernels: with SSAO on AwsmFrameStats.ms_shade is the shading kernels and the occlusion
    ht.mark("opaque: shade launches");
    if (c->overlap) HIPCHK(c, mark_shade_done(c, ss));
    else if (c->trace_dev) awsm_launch_handoff_signal(nullptr, 0u, trace_slot(c, 2), ss);
    ht.mark("opaque: shade-done signal + event");
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

// The frame of a transparent pass (kind: the world's or the HUD's): its own draws / vertices / setup records / bins; the geometry pass's
// visibility keys for the depth test; the opaque image as blit source and transmission background; the composite image as target.
void fill_frame_forward(AwsmHipCtx* c, FrameDev* f, PassKind kind) {
    fill_frame(c, f, frame_view(c));
    const FrameBufs& t = pass_bufs(c, kind);
    const PassList& list = c->lists[kind];
    bind_pass(*f, t);
    f->vis = (unsigned long long*)FB(c).vis.ptr;      // the WORLD's depth (render.rs:224-297), whatever the opaque pass read
    f->n_draws = (uint32_t)list.draws.size();
    f->total_tris = list.total_tris; f->total_verts = 3u * list.total_tris;
    f->draw_shade = (DrawShadeDev*)t.draw_shade.ptr;
    f->tex_slots = (TexSlotDev*)t.tex_slots.ptr;
    f->draw_mat = (DrawMatDev*)t.draw_mat.ptr;
    f->wpos = (float4*)t.wpos.ptr;
    f->tri_shade = nullptr; f->draw_lean = nullptr; f->shade_todo = nullptr; f->shade_todo_cap = 0; f->lean_next = nullptr; f->lean_grid = 0;     // the opaque pass's lean route only
    f->raster_scratch = nullptr;      // the transparent pass has its own tile kernel: nothing is split
    f->raster_extra_cap = 0; f->raster_slot_cap = 0;
    f->opaque_rgba16f = c->opaque_src ? (const uint16_t*)c->opaque_src : f->out_rgba16f;
    f->out_compact = 0;                    // the composite is addressed by absolute row
    f->frag_rec = (uint4*)t.frag_rec.ptr; f->frag_color = (float4*)t.frag_color.ptr; f->frag_first = (uint32_t*)t.frag_first.ptr; f->frag_cap = t.frag_cap;
    f->out_rgba16f = (uint16_t*)(c->bound_comp ? c->bound_comp : c->comp16.ptr);
    f->out_rgba32f = (float*)c->comp32.ptr;
    f->has_opaque = c->last_opaque.has_opaque;
    f->mipmap = c->last_opaque.mipmap;
    f->aniso = (c->flags & AWSM_CFG_ANISOTROPIC) ? 1u : 0u;
    if (kind == kPassHudTransparent) {      // the HUD pass: depth starts cleared, the colours it blends over are the composite's own (in place, a pixel per thread)
        f->hud_pass = 1;
        f->opaque_rgba16f = f->out_rgba16f;
    }
}

// The selection kernels' arguments for the current slot's frame with the record `st`: the WORLD geometry pass's keys and draw list (in a frame whose
// hud draws share the world's rank space the world's draws come first), the camera snapshot, the slot's tables.
void fill_selection(AwsmHipCtx* c, const AwsmHipCtx::SelectionState& st, SelectionDev* a) {
    memset(a, 0, sizeof *a);
    a->width = c->width; a->height = c->height; a->msaa = samples_of(c);
    a->n_draws = (uint32_t)c->lists[kPassWorld].draws.size(); a->total_tris = c->lists[kPassWorld].total_tris;
    a->n_keys = (uint32_t)(st.keys.size() / 2); a->n_boxes = (uint32_t)(st.boxes.size() / 6);
    a->flags = st.flags; a->radius = st.radius;
    memcpy(a->outline_color, st.outline_color, sizeof a->outline_color); memcpy(a->box_color, st.box_color, sizeof a->box_color);
    a->half_width = st.half_width; a->hidden_alpha = st.hidden_alpha; a->depth_epsilon = st.depth_epsilon;
    a->scene = c->scene_dev;
    a->material_meta_bytes = (uint32_t)std::min<size_t>(c->bufs[AWSM_BUF_MATERIAL_META].size, 0xFFFFFFFFu);
    a->draws = (const DrawDev*)FB(c).draws_dev.ptr;
    a->tri_info = (const uint32_t*)FB(c).tri_flags.ptr;
    a->vis = (const unsigned long long*)FB(c).vis.ptr;
    a->camera = (const uint8_t*)FB(c).camera.ptr;
    a->edges = (float*)c->sel_tables[c->slot].ptr;                                                     // (32-byte records first: aligned)
    a->draw_selected = (uint8_t*)c->sel_tables[c->slot].ptr + (size_t)selection::kMaxEdges * selection::kEdgeFloats * 4;
    if (a->n_keys) memcpy(a->keys, st.keys.data(), st.keys.size() * 4);
    if (a->n_boxes) memcpy(a->boxes, st.boxes.data(), st.boxes.size() * 4);
}

int enqueue_transparent(AwsmHipCtx* c, PassKind kind) {
    const bool hud = kind == kPassHudTransparent;
    FrameDev f;
    fill_frame_forward(c, &f, kind);
    const uint32_t n_tiles = f.tiles_x * f.tiles_y;
    int rc = sync_scene(c);
    if (rc) return rc;
    hipStream_t ss = shade_stream_of(c);          // in order after the opaque pass
    // the composite image and the fragment lists' bookkeeping are per context: behind the previous frame's passes on the other slot's stream
    if (c->overlap && c->shade_recorded[prev_slot(c)]) HIPCHK(c, wait_prev_slot(c, ss));
    if ((rc = record(c, EV_FWD_BEGIN, ss))) return rc;
    const bool has_geometry = f.total_tris && n_tiles;
    if (!has_geometry) {
        if ((rc = clear_empty_pass(c, pass_bufs(c, kind), (uint32_t*)pass_bufs(c, kind).counters.ptr, n_tiles, ss))) return rc;
    } else {
        awsm_launch_resolve_draws(c->scene_dev, &f, ss);      // first: the transform tags each triangle with its draw's alpha mode
        awsm_launch_transform_forward(c->scene_dev, &f, c->lists[kind].n_blocks, ss);
    }
    if (n_tiles) {
        enqueue_binning(f, f.total_tris != 0, ss);
        // the editor's ground grid: the world pass only, with the record this pass was submitted with and the frame's camera snapshot
        EditorGridDev grid;
        const AwsmHipCtx::GridState& gs = c->grid_pass[c->slot];
        const bool with_grid = gs.on && !hud;
        if (with_grid) { grid.camera = f.camera; memcpy(grid.p, gs.p, sizeof grid.p); }
        awsm_launch_forward(c->scene_dev, &f, with_grid ? &grid : nullptr, ss);
        // the editor's selection overlay, with the record this pass was submitted with: the world pass only, behind the kernels that leave the
        // composite — the grid, the transparent meshes, the MSAA resolve — and in front of the shade-done signal below: it reads the slot's keys,
        // which the slot's next geometry pass overwrites (the ordering argument of the occlusion kernels in enqueue_opaque).  A replay
        // (awsm_hip_frame_end) comes through here again behind a blit that wrote every pixel anew, so the overlay is blended once.
        const AwsmHipCtx::SelectionState& sl = c->sel_pass[c->slot];
        if (sl.on && !hud) {
            SelectionDev sd;
            fill_selection(c, sl, &sd);
            sd.out16 = (uint2*)f.out_rgba16f; sd.out32 = (float4*)f.out_rgba32f;
            sd.poison = f.poison; sd.frame_serial = f.frame_serial;
            awsm_launch_selection(&sd, ss);
        }
    }
    if ((rc = record(c, EV_FWD, ss))) return rc;
    if (c->overlap) HIPCHK(c, mark_shade_done(c, ss));
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int ensure_bin_capacity_of(AwsmHipCtx* c, FrameBufs& b, uint32_t entries) {
    if (entries <= b.bin_capacity && b.bin_list.ptr) return AWSM_OK;
    uint32_t cap = std::max(entries, b.bin_capacity + b.bin_capacity / 2);
    int rc = dev_realloc(c, b.bin_list, (size_t)cap * 4, false);
    if (rc) return rc;
    b.bin_capacity = cap;
    return AWSM_OK;
}

int ensure_fragment_capacity(AwsmHipCtx* c, FrameBufs& b, uint32_t fragments) {
    if (fragments <= b.frag_cap && b.frag_rec.ptr) return AWSM_OK;
    const uint32_t cap = std::max(fragments, b.frag_cap + b.frag_cap / 2);
    int rc = dev_realloc(c, b.frag_rec, (size_t)cap * 16, false);
    if (!rc) rc = dev_realloc(c, b.frag_color, (size_t)cap * 16, false);
    if (rc) return rc;
    b.frag_cap = cap;
    return AWSM_OK;
}

// API draws -> one DrawDev per (draw, instance) with the running triangle / block prefix sums; `data` = the vertex buffer the
// draws index, `bytes_per_tri` the extent check per triangle (0 = the vertices are indexed: not checkable here).
int build_draw_list(AwsmHipCtx* c, const char* pass, const AwsmDraw* draws, uint32_t n, AwsmBuf data, uint32_t bytes_per_tri,
                    std::vector<DrawDev>& out, uint64_t* tris_out, uint64_t* blocks_out) {
    out.clear();
    uint64_t tris = 0, blocks = 0;
    for (uint32_t i = 0; i < n; i++) {
        const AwsmDraw& d = draws[i];
        if (d.inst_count != 0) {   // instanced draw: inst_count mat4s at inst_off of the instance-transform buffer (instances.rs)
            const DevBuf& ib = c->bufs[AWSM_BUF_INSTANCES];
            if (!ib.ptr) return fail(c, AWSM_ERR_NOT_READY, "%s: draw %u: instanced, but the instance-transform buffer was never created", pass, i);
            if ((d.inst_off & 15u) || (uint64_t)d.inst_off + 64ull * d.inst_count > ib.size)
                return fail(c, AWSM_ERR_OUT_OF_RANGE, "%s: draw %u: %u instances at %u exceed the instance-transform buffer", pass, i, d.inst_count, d.inst_off);
        }
        if (d.vis_data_off & (bytes_per_tri ? 15u : 3u)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: draw %u: vertex data offset %u misaligned", pass, i, d.vis_data_off);
        if ((uint64_t)d.vis_data_off + (uint64_t)bytes_per_tri * d.tri_count > c->bufs[data].size || (!bytes_per_tri && d.tri_count && (uint64_t)d.vis_data_off + 40 > c->bufs[data].size))
            return fail(c, AWSM_ERR_OUT_OF_RANGE, "%s: draw %u: %u triangles at %u exceed the vertex buffer", pass, i, d.tri_count, d.vis_data_off);
        if ((uint64_t)d.geom_meta_off + 40 > c->bufs[AWSM_BUF_GEOM_META].size || (d.geom_meta_off & 3u))
            return fail(c, AWSM_ERR_OUT_OF_RANGE, "%s: draw %u: geometry meta offset %u out of range", pass, i, d.geom_meta_off);
        if (d.tri_count == 0) continue;   // draw_indexed(0) draws nothing; keeps first_block strictly increasing
        const uint32_t copies = d.inst_count ? d.inst_count : 1u;
        for (uint32_t k = 0; k < copies; k++) {
            DrawDev dd{};
            dd.geom_meta_off = d.geom_meta_off; dd.vis_data_off = d.vis_data_off; dd.tri_count = d.tri_count; dd.flags = d.flags & 0x7Fu;
            if (d.inst_count) { dd.flags |= kDrawInstanced; dd.inst_off = d.inst_off + 64u * k; }
            dd.first_tri = (uint32_t)tris; dd.first_block = (uint32_t)blocks;
            out.push_back(dd);
            tris += d.tri_count;
            blocks += (3ull * d.tri_count + 255) / 256;
            if (tris > 0x55555555ull) return fail(c, AWSM_ERR_UNSUPPORTED, "%s: more than 2^32/3 triangles in one pass", pass);
            if (out.size() >= (1u << 24)) return fail(c, AWSM_ERR_UNSUPPORTED, "%s: more than 2^24 non-empty draws (instances included) in one pass", pass);
        }
    }
    *tris_out = tris; *blocks_out = blocks;
    return AWSM_OK;
}

// per-pass device state sized for `draws_host` / total_tris; uploads the draw list when it changed
// raster items: one per tile + one per extra slice of a split tile (<= entries / 256); scratch tiles: one per slice of a split tile
// The frame a pass's tile tables are sized for: the context's, or the light's S x S single-sampled map (awsm_hip_shadow_pass).
struct PassDims { uint32_t w, h, samples; };
inline PassDims dims_of(const AwsmHipCtx* c, const FrameBufs& b) {
    if (b.kind == kPassShadow) { const uint32_t S = c->shadow_pass[b.slot].p.map_size; return {S, S, 1u}; }
    return {c->width, c->height, samples_of(c)};
}

int reserve_raster_items(AwsmHipCtx* c, FrameBufs& b, bool forward, PassDims dm) {
    const uint32_t tiles_x = (dm.w + kTile - 1) / kTile, tiles_y_full = (dm.h + kTile - 1) / kTile;
    const size_t n_tiles_full = (size_t)tiles_x * tiles_y_full;
    const uint32_t extra_cap = forward ? 0u : b.bin_capacity / 256u + 1u, slot_cap = forward ? 0u : b.bin_capacity / 128u + 2u;
    int rc;
    if ((rc = dev_reserve(c, b.tile_order, (n_tiles_full + extra_cap) * 4))) return rc;
    if (!forward && (rc = dev_reserve(c, b.raster_scratch, (size_t)slot_cap * kTile * kTile * 8 * dm.samples))) return rc;
    b.raster_extra_cap = extra_cap; b.raster_slot_cap = slot_cap;
    return AWSM_OK;
}

// Device state of one pass in one frame slot, sized for `tri_cap` triangles and `draw_cap` draws.
int size_pass_buffers(AwsmHipCtx* c, FrameBufs& b, size_t tri_cap, size_t draw_cap, bool forward, PassDims dm) {
    int rc;
    const size_t nd = std::max<size_t>(draw_cap, 1), nv = std::max<size_t>(3 * tri_cap, 1), nt = std::max<size_t>(tri_cap, 1);
    if ((rc = dev_reserve(c, b.draws_dev, nd * sizeof(DrawDev)))) return rc;
    const bool world_pass = b.kind == kPassWorld, shadow = b.kind == kPassShadow;
    if (world_pass && c->geometry_cache) {      // geometry cache: the previous list beside the current one, world positions per vertex
        if ((rc = dev_reserve(c, b.draws_prev, nd * sizeof(DrawDev)))) return rc;
        if ((rc = dev_reserve(c, b.wcache, nv * 16))) return rc;
        const size_t blocks_bound = nv / 256 + nd + 1;
        // (behind the map, in its allocation: k_draw_decide's word per draw — FrameDev::draw_hit_at)
        b.draw_hit_at = (c->clip_in_bin && blocks_bound + nd < (1ull << 30)) ? (uint32_t)blocks_bound : 0u;
        if ((rc = dev_reserve(c, b.block_map, (blocks_bound + (b.draw_hit_at ? nd : 0)) * 4))) return rc;
        b.block_map_valid = false;
        if (b.cache_mark.size < blocks_bound * 4) { if ((rc = dev_realloc(c, b.cache_mark, (blocks_bound + blocks_bound / 2) * 4, true))) return rc; }
    }
    b.cache_valid = false;      // the arrays may have moved
    // (the shadow pass has no per-draw resolve and nothing shades from it: no per-draw records, no per-triangle attribute offsets, no lean records)
    if (!shadow && (rc = dev_reserve(c, b.draw_shade, nd * sizeof(DrawShadeDev)))) return rc;
    if (!shadow && (rc = dev_reserve(c, b.tex_slots, nd * kCoreTextures * sizeof(TexSlotDev)))) return rc;
    if (!shadow && (rc = dev_reserve(c, b.draw_mat, nd * sizeof(DrawMatDev)))) return rc;
    if ((rc = dev_reserve(c, b.clip, nv * 16))) return rc;
    if ((rc = dev_reserve(c, b.nrm, nv * 16))) return rc;
    if ((rc = dev_reserve(c, b.tan, nv * 16))) return rc;
    if (forward && (rc = dev_reserve(c, b.wpos, nv * 16))) return rc;
    if ((rc = dev_reserve(c, b.tri_flags, nt * 4))) return rc;
    if (!forward && !shadow && (rc = dev_reserve(c, b.tri_shade, nt * 32))) return rc;
    if (!forward && !shadow && (rc = dev_reserve(c, b.draw_lean, nd * sizeof(LeanDrawDev)))) return rc;
    if ((rc = dev_reserve(c, b.big_list, nt * 4))) return rc;
    // (behind the set-up records, in their allocation: the world pass's compact bin records, 8 bytes per triangle — FrameDev::bin_rec_at, in records)
    b.bin_rec_at = (world_pass && c->clip_in_bin && nt * (kTriRecBytes / 8) <= 0xFFFFFFFFull) ? (uint32_t)(nt * (kTriRecBytes / 8)) : 0u;
    if ((rc = dev_reserve(c, b.tri_rec, nt * kTriRecBytes + (b.bin_rec_at ? nt * 8 : 0)))) return rc;
    const uint32_t tiles_x = (dm.w + kTile - 1) / kTile, tiles_y_full = (dm.h + kTile - 1) / kTile;
    const size_t n_tiles_full = (size_t)tiles_x * tiles_y_full;
    if ((rc = dev_reserve(c, b.tile_count, n_tiles_full * 4))) return rc;
    if ((rc = dev_reserve(c, b.tile_offset, (n_tiles_full + 1) * 4))) return rc;
    if ((rc = dev_reserve(c, b.tile_cursor, n_tiles_full * 4))) return rc;
    if ((rc = dev_reserve(c, b.tile_split, n_tiles_full * 8))) return rc;
    if ((rc = dev_reserve(c, b.scan_tmp, (((n_tiles_full + 255) / 256) * 2 + 1) * 40 * 4))) return rc;      // kScanWords = 40: aggregates, bases, run starts (kernels_geometry.hip)
    if ((rc = ensure_bin_capacity_of(c, b, (c->flags & AWSM_CFG_SMALL_BIN_LIST) ? 4096u : (uint32_t)std::min<size_t>(std::max<size_t>(4 * tri_cap + 65536u, 1u << 18), 0xFFFFFFF0u)))) return rc;
    if ((rc = reserve_raster_items(c, b, forward, dm))) return rc;
    b.tri_cap = tri_cap; b.draw_cap = draw_cap; b.sized_w = dm.w; b.sized_h = dm.h;
    return AWSM_OK;
}

// Sizes the pass's device state for `draws_host` / total_tris (see reserve_pass_buffers).
int ensure_pass_capacity(AwsmHipCtx* c, FrameBufs& b, const std::vector<DrawDev>& draws_host, uint32_t total_tris, bool forward) {
    int rc;
    const PassDims dm = dims_of(c, b);
    if (total_tris > b.tri_cap || draws_host.size() > b.draw_cap || b.sized_w != dm.w || b.sized_h != dm.h || !b.bin_list.ptr) {
        bool instanced = false;
        for (const DrawDev& d : draws_host) instanced |= (d.flags & kDrawInstanced) != 0;
        const size_t tri_bound = forward || instanced ? ~size_t(0) : c->bufs[AWSM_BUF_VIS_GEOM_DATA].size / 168u;
        const size_t tri_cap = std::max<size_t>(std::min<size_t>((size_t)total_tris + total_tris / 4 + 4096, std::max<size_t>(tri_bound, total_tris)), b.tri_cap);
        const size_t draw_cap = std::max<size_t>(draws_host.size() + draws_host.size() / 4 + 64, b.draw_cap);
        const bool shadow = b.kind == kPassShadow;      // (the light's pass: this slot's alone — the other slot's map may have another size)
        FrameBufs* const set = pass_slots(c, b.kind);
        for (int sl = 0; sl < (shadow ? 1 : n_slots(c)); sl++) {
            // (the slot in use first: if memory runs out half-way the current frame still has its buffers)
            FrameBufs& t = set[(c->slot + sl) % kSlots];
            if ((rc = size_pass_buffers(c, t, std::max(tri_cap, t.tri_cap), std::max(draw_cap, t.draw_cap), forward, dm))) return rc;
        }
    }
    return AWSM_OK;
}

int upload_draws_at(AwsmHipCtx* c, FrameBufs& b, size_t at, const std::vector<DrawDev>& list) {
    const size_t bytes = list.size() * sizeof(DrawDev);
    uint8_t* dst = (uint8_t*)b.draws_dev.ptr + at * sizeof(DrawDev);
    if (bytes <= (1u << 20)) return upload_small(c, dst, list.data(), bytes);
    HIPCHK(c, hipMemcpyAsync(dst, list.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AWSM_OK;
}

// The sorted draw list of a static or slowly moving scene repeats frame after frame: upload it only when it changed
// (an in-stream host-to-device copy costs more GPU idle time than the transform kernel takes).
// keep_prev (the world geometry pass): a new list goes into the other one of the slot's two list buffers, so that the list the slot's arrays were
// computed for stays readable beside it (geometry cache: k_deform_transform compares the two draw by draw).
int upload_draw_list(AwsmHipCtx* c, FrameBufs& b, const std::vector<DrawDev>& draws_host, bool keep_prev) {
    const bool same_draws = b.draws_uploaded_valid && b.draws_uploaded_ptr == b.draws_dev.ptr && b.draws_uploaded.size() == draws_host.size() &&
                            (draws_host.empty() || memcmp(b.draws_uploaded.data(), draws_host.data(), draws_host.size() * sizeof(DrawDev)) == 0);
    auto upload_block_map = [&]() -> int {      // the world pass: which draw each transform workgroup belongs to
        b.block_map_valid = false;
        if (!keep_prev || !b.block_map.ptr) return AWSM_OK;
        std::vector<uint32_t> map;
        for (size_t i = 0; i < draws_host.size(); i++) map.insert(map.end(), (3ull * draws_host[i].tri_count + 255) / 256, (uint32_t)i);
        if (map.size() * 4 > b.block_map.size || map.size() * 4 > (1u << 20) || (b.draw_hit_at && map.size() > b.draw_hit_at)) return AWSM_OK;
        const int rc = upload_small(c, b.block_map.ptr, map.data(), map.size() * 4);
        if (!rc) b.block_map_valid = true;
        return rc;
    };
    if (draws_host.empty()) return AWSM_OK;
    if (same_draws) return (keep_prev && !b.block_map_valid) ? upload_block_map() : AWSM_OK;      // (the map's buffer was re-sized under an unchanged list)
    if (keep_prev && b.cache_valid && !b.cached_is_prev && b.draws_prev.ptr && b.draws_prev.size == b.draws_dev.size) {
        std::swap(b.draws_dev, b.draws_prev);
        b.cached_is_prev = true;
    } else if (keep_prev && !b.cached_is_prev) b.cache_valid = false;      // the cached list is about to be overwritten
    b.draws_uploaded = draws_host; b.draws_uploaded_ptr = b.draws_dev.ptr; b.draws_uploaded_valid = true; b.draws_version++;
    b.tail_uploaded_valid = false;
    { const int rc = upload_block_map(); if (rc) return rc; }
    return upload_draws_at(c, b, 0, draws_host);
}

// Per-pass device state for `draws_host` / total_tris; uploads the draw list when it changed.  A frame that fits what the slot was sized for
// touches nothing (the common case: one comparison).  When it does not fit, EVERY frame slot of the pass is re-sized at once and with
// headroom — a re-allocation synchronises all streams, so a camera move that un-culls a few more triangles every frame must not pay it
// per frame and per slot (seen in round 2's driver run: frames 9, 10 and 13 of the process stalled the host for 2.1 / 1.8 / 0.9 ms, a third
// of a 20-frame measurement).  Triangles: need + 25 % + 4096, but no more than the vertex buffer can hold when no draw is instanced
// (then the pass can never outgrow its buffers again); draws: need + 25 % + 64.
int reserve_pass_buffers(AwsmHipCtx* c, FrameBufs& b, const std::vector<DrawDev>& draws_host, uint32_t total_tris, bool forward) {
    int rc = ensure_pass_capacity(c, b, draws_host, total_tris, forward);
    if (rc) return rc;
    return upload_draw_list(c, b, draws_host, b.kind == kPassWorld);
}

// A list that overflowed grows to what its pass measured, with headroom: entries + 25 % + 1024.
inline uint32_t with_headroom(uint32_t need) { return need + need / 4 + 1024; }
// ... a geometry-type pass's bin list (counters: the pass's own, read back), and the raster items that are sized with it
int grow_after_overflow(AwsmHipCtx* c, FrameBufs& b, const uint32_t* counters) {
    const int rc = ensure_bin_capacity_of(c, b, with_headroom(counters[kCtrEntries]));
    return rc ? rc : reserve_raster_items(c, b, false, dims_of(c, b));
}

// A versioned record of the C ABI (first word: struct_size) over the defaults `dst` already holds: the caller's fields as far as it knows them.
int merge_record(AwsmHipCtx* c, const char* entry, const char* type, const void* src, void* dst, size_t size) {
    const uint32_t given = *(const uint32_t*)src;
    if (given < 4u || given > 4096u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: %s.struct_size = %u (set it to sizeof(%s))", entry, type, given, type);
    memcpy((uint8_t*)dst + 4, (const uint8_t*)src + 4, (std::min<size_t>(given, size) & ~(size_t)3) - 4);      // whole fields only; the rest keeps its defaults
    return AWSM_OK;
}
// ... and its first n floats are finite
int check_finite(AwsmHipCtx* c, const char* entry, const float* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: value %zu of the record is not finite", entry, i);
    return AWSM_OK;
}

}  // namespace

extern "C" {

uint32_t awsm_hip_abi_version(void) { return AWSM_HIP_ABI_VERSION; }

const char* awsm_hip_last_error(const AwsmHipCtx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int awsm_hip_create(const AwsmConfig* cfg, AwsmHipCtx** out) {
    if (!cfg || !out || cfg->struct_size < sizeof(AwsmConfig) || cfg->abi_version != AWSM_HIP_ABI_VERSION)
        return AWSM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || cfg->device < 0 || cfg->device >= n_dev) return AWSM_ERR_NO_DEVICE;
    AwsmHipCtx* c = new (std::nothrow) AwsmHipCtx();
    if (!c) return AWSM_ERR_OUT_OF_MEMORY;
    c->device = cfg->device;
    c->flags = cfg->flags;
    for (int k = 0; k < kPassKinds; k++)
        for (int s = 0; s < kSlots; s++) { FrameBufs& b = pass_slots(c, (PassKind)k)[s]; b.kind = (PassKind)k; b.slot = (uint8_t)s; }
    auto bail = [&](int code) { awsm_hip_destroy(c); return code; };
    if (hipSetDevice(c->device) != hipSuccess) return bail(AWSM_ERR_DEVICE);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return bail(AWSM_ERR_DEVICE);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "awsm_hip: device %d is %s; this library carries gfx950 code objects only\n", c->device, prop.gcnArchName);
        return bail(AWSM_ERR_NO_DEVICE);
    }
    if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; c->own_stream = false; }
    else { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(AWSM_ERR_DEVICE); c->own_stream = true; }
    for (int i = 0; i < EV_COUNT; i++) if (hipEventCreate(&c->ev[i]) != hipSuccess) return bail(AWSM_ERR_DEVICE);
    if (hipMalloc((void**)&c->scene_dev, sizeof(DevScene)) != hipSuccess) return bail(AWSM_ERR_OUT_OF_MEMORY);
    c->overlap = (cfg->flags & AWSM_CFG_OVERLAP_FRAMES) != 0;
    { const char* e = getenv("AWSM_GEOMETRY_CACHE"); c->geometry_cache = !(e && e[0] == '0'); }      // "0": k_deform_transform recomputes every draw every frame (A/B measurements, tests)
    { const char* e = getenv("AWSM_CLIP_IN_BIN"); c->clip_in_bin = !(e && e[0] == '0'); }      // "0": k_deform_transform writes clip and decides cache hits per workgroup, k_bin reads clip (ctx.hpp)
    {   // k_shade_lean as a persistent grid of N workgroups per CU (it is VALU-bound from 4 waves/SIMD up): the rest of each CU's
        // wave slots, registers and LDS stays free for the next frame's geometry kernels on the other stream
        const char* e = getenv("AWSM_LEAN_WGS_PER_CU");
        const int per_cu = e ? atoi(e) : (c->overlap ? kLeanWgsPerCu : 0);
        c->lean_grid = per_cu > 0 ? (uint32_t)(per_cu * prop.multiProcessorCount) & ~7u : 0u;
    }
    for (int s = 0; s < n_slots(c); s++) {
        for (PassKind k : {kPassWorld, kPassTransparent, kPassHudTransparent, kPassHud}) {      // (the shadow pass's: at its first use)
            DevBuf& ctr = pass_slots(c, k)[s].counters;   // 8 frame counters + 4 pick words + k_bin_scan's arrival counter [12] and ready flag [13]
            if (hipMalloc(&ctr.ptr, 16 * sizeof(uint32_t)) != hipSuccess || (k == kPassWorld && hipMemset(ctr.ptr, 0, 16 * sizeof(uint32_t)) != hipSuccess)) return bail(AWSM_ERR_OUT_OF_MEMORY);
            ctr.size = 16 * sizeof(uint32_t);
        }
        if (hipMalloc(&c->fb[s].camera.ptr, 512) != hipSuccess || hipMemset(c->fb[s].camera.ptr, 0, 512) != hipSuccess) return bail(AWSM_ERR_OUT_OF_MEMORY);      // per-frame camera snapshot (every mode)
        c->fb[s].camera.size = 512;
    }

    if (c->overlap) {
        for (int s = 0; s < kSlots; s++) {
#ifdef AWSM_DEBUG_SWITCHES
            if (const char* m = getenv("AWSM_SHADE_CU_MASK")) {      // experiment (tools/ab_cu_mask.sh): hex words, least significant first, comma separated
                std::vector<uint32_t> words;
                for (const char* p = m; *p; ) { char* end = nullptr; words.push_back((uint32_t)strtoul(p, &end, 16)); p = (*end == ',') ? end + 1 : end; if (end == p && *p) break; }
                if (words.empty() || hipExtStreamCreateWithCUMask(&c->shade_streams[s], (uint32_t)words.size(), words.data()) != hipSuccess) return bail(AWSM_ERR_DEVICE);
            } else
#endif
            if (hipStreamCreateWithFlags(&c->shade_streams[s], hipStreamNonBlocking) != hipSuccess) return bail(AWSM_ERR_DEVICE);
            // These events order streams of this device among themselves.  Recorded with the default (system-scope) release they write the
            // L2s back and invalidate them each time — behind a raster or shading kernel that is 66 MB of dirty lines: 8-28 us per record on
            // the path between two frames (tools/frame_timeline.sh) — so: device-scope release.
            const unsigned ev_flags = hipEventDisableTiming | hipEventReleaseToDevice;
            if (hipEventCreateWithFlags(&c->ev_geom_done[s], ev_flags) != hipSuccess || hipEventCreateWithFlags(&c->ev_shade_done[s], ev_flags) != hipSuccess ||
                hipEventCreateWithFlags(&c->ev_uploads[s], ev_flags) != hipSuccess) return bail(AWSM_ERR_DEVICE);
            if (s == 0 && hipEventCreateWithFlags(&c->ev_flush, hipEventDisableTiming) != hipSuccess) return bail(AWSM_ERR_DEVICE);
        }
    }
    if (hipHostMalloc((void**)&c->counters_host, (16 + 2 * kSlots + 1) * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return bail(AWSM_ERR_OUT_OF_MEMORY);   // last word: hand-off gates that timed out
    memset(c->counters_host, 0, (16 + 2 * kSlots + 1) * sizeof(uint32_t));
    if (c->overlap) {
        const char* e = getenv("AWSM_DEVICE_HANDOFF");      // "0": cross-stream events instead (for a profiler that serialises kernels: tools/pmc_*.sh)
        c->handoff = !(e && e[0] == '0');
        { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->clock_khz = (uint32_t)khz; }
        double budget_ms = 4000.0;
        if (const char* p = getenv("AWSM_HANDOFF_TIMEOUT_MS")) { const double v = atof(p); if (v > 0.0) budget_ms = v; }
        c->handoff_budget_ticks = (unsigned long long)(budget_ms * (double)c->clock_khz) + 1ull;
        if (hipMalloc((void**)&c->handoff_flags, 3 * kSlots * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&c->handoff_poison, kSlots * sizeof(uint32_t)) != hipSuccess) return bail(AWSM_ERR_OUT_OF_MEMORY);
        if (hipMemset(c->handoff_flags, 0, 3 * kSlots * sizeof(uint32_t)) != hipSuccess || hipMemset(c->handoff_poison, 0xFF, kSlots * sizeof(uint32_t)) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) return bail(AWSM_ERR_DEVICE);
        if (const char* d = getenv("AWSM_TEST_HANDOFF_DROP")) c->handoff_test_drop = (uint32_t)atoi(d);
        // Probe: a gate on one stream, its signal on the other, both directions of every pair the frames will use.  Where the two do not run
        // side by side (kernels serialised by a counter-collecting profiler; two streams on one hardware queue) the gate gives up after ~10 ms
        // and the context orders its streams with events.
        for (int k = 0; c->handoff && k < 2 * kSlots; k++) {
            hipStream_t ss = c->shade_streams[k % kSlots], waiter = k < kSlots ? ss : c->stream, setter = k < kSlots ? c->stream : ss;
            const uint32_t serial = ++c->geom_sig[0];
            awsm_launch_handoff_wait(c->handoff_flags, serial, 10ull * c->clock_khz /* 10 ms */, handoff_timeouts(c), 0u, nullptr, 0u, waiter);
            awsm_launch_handoff_signal(c->handoff_flags, serial, nullptr, setter);
            if (hipStreamSynchronize(waiter) != hipSuccess || hipStreamSynchronize(setter) != hipSuccess) return bail(AWSM_ERR_DEVICE);
            if (*(volatile uint32_t*)handoff_timeouts(c) != 0u) { c->handoff = false; c->handoff_timeouts_seen = *(volatile uint32_t*)handoff_timeouts(c); }
        }
    }
    memset(&c->scene, 0, sizeof c->scene);
    // defaults == AwsmRendererBuilder::new (crates/renderer/src/lib.rs:168-207): black skybox, white IBL
    c->scene.skybox_rgba[3] = 1.0f;
    for (int i = 0; i < 3; i++) { c->scene.prefiltered_rgb[i] = 1.0f; c->scene.irradiance_rgb[i] = 1.0f; }
    *out = c;
    return AWSM_OK;
}

int awsm_hip_destroy(AwsmHipCtx* c) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)sync_shade_streams(c);
    auto fr = [](DevBuf& b) { if (b.ptr) (void)hipFree(b.ptr); b.ptr = nullptr; b.size = 0; };
    for (auto& b : c->bufs) fr(b);
    for (auto& b : c->tex) fr(b);
    for (auto& b : c->tex_kinds) fr(b);
    for (auto& b : c->merged_vis) fr(b);
    fr(c->pose_records);
    fr(c->env_stage); fr(c->env_tables); fr(c->env_rows); fr(c->env_filter_tab); if (c->ev_env_copy) (void)hipEventDestroy(c->ev_env_copy);
    fr(c->lut); for (auto& b : c->cube_tex) fr(b); for (auto& b : c->cube_bordered) fr(b); fr(c->digest); for (auto& b : c->shade_todo) fr(b); for (int sl = 0; sl < kSlots; sl++) { fr(c->msaa_color0[sl]); fr(c->msaa_edges[sl]); fr(c->msaa_edge_bits[sl]); fr(c->msaa_cells[sl]); } fr(c->mip_kinds); for (auto& b : c->out16) fr(b); for (auto& b : c->out32) fr(b); fr(c->comp16); fr(c->comp32); fr(c->grid_layer); for (auto& b : c->lights_pre) fr(b);
    for (auto& b : c->ssao_layers) fr(b);
    for (auto& b : c->taa_img) fr(b); fr(c->taa_layers);
    for (auto& b : c->sel_tables) fr(b);
    fr(c->sel_layers);
    fr(c->pick_scratch);
    for (auto& b : c->shadow_layers) fr(b); for (auto& b : c->shadow_cam) fr(b); for (auto& b : c->shadow_view_ctr) fr(b); for (auto& b : c->shadow_view_layers) fr(b); for (DevScene* sc : c->shadow_scene) if (sc) (void)hipFree(sc);
    for (auto& b : c->display8) fr(b); fr(c->effects16); fr(c->bloom_a); fr(c->bloom_b); fr(c->dof_lc); fr(c->dof_blur);
    for (int k = 0; k < kPassKinds * kSlots; k++) {
        FrameBufs& b = pass_slots(c, (PassKind)(k / kSlots))[k % kSlots];
        fr(b.vis); fr(b.wpos); fr(b.frag_rec); fr(b.frag_color); fr(b.frag_first); fr(b.tex_slots); fr(b.draw_mat); fr(b.clip); fr(b.nrm); fr(b.tan); fr(b.tri_rec); fr(b.tri_flags); fr(b.tri_shade); fr(b.draw_lean); fr(b.draws_dev); fr(b.draw_shade); fr(b.tile_count); fr(b.tile_offset);
        fr(b.wcache); fr(b.draws_prev); fr(b.cache_mark); fr(b.block_map); fr(b.tile_cursor); fr(b.tile_order); fr(b.scan_tmp); fr(b.tile_split); fr(b.raster_scratch); fr(b.bin_list); fr(b.big_list); fr(b.counters); fr(b.camera);
    }
    for (hipStream_t st : c->shade_streams) if (st) (void)hipStreamDestroy(st);
    for (int i = 0; i < kSlots; i++) { if (c->ev_geom_done[i]) (void)hipEventDestroy(c->ev_geom_done[i]); if (c->ev_shade_done[i]) (void)hipEventDestroy(c->ev_shade_done[i]); if (c->ev_uploads[i]) (void)hipEventDestroy(c->ev_uploads[i]); }
    if (c->ev_flush) (void)hipEventDestroy(c->ev_flush);
    if (c->scene_dev) (void)hipFree(c->scene_dev);
    if (c->stage) (void)hipHostFree(c->stage);
    if (c->counters_host) (void)hipHostFree(c->counters_host);
    if (c->handoff_flags) (void)hipFree(c->handoff_flags);
    if (c->handoff_poison) (void)hipFree(c->handoff_poison);
    if (c->trace_dev) (void)hipFree(c->trace_dev);
    for (int i = 0; i < EV_COUNT; i++) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return AWSM_OK;
}

int awsm_hip_device_info(AwsmHipCtx* c, char* name_out, size_t name_cap, uint32_t* cu_count, uint64_t* hbm_bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    if (name_out && name_cap) snprintf(name_out, name_cap, "%s (%s)", prop.name, prop.gcnArchName);
    if (cu_count) *cu_count = (uint32_t)prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return AWSM_OK;
}

int awsm_hip_buffer_create(AwsmHipCtx* c, AwsmBuf which, size_t bytes) {
    if (!c || (int)which < 0 || which >= AWSM_BUF_COUNT) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "buffer_create: bad buffer id %d", (int)which);
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    // +16 bytes of slack so 16-byte vector loads of the last record never leave the allocation (size = the logical size)
    log_dirty(c, which, 0, ~size_t(0));
    if (bytes && c->bufs[which].ptr && c->bufs[which].size == bytes) {     // unchanged size: same allocation, cleared ("contents are NOT preserved")
        if (which == AWSM_BUF_CAMERA) memset(c->camera_host, 0, sizeof c->camera_host);
        HIPCHK(c, hipMemsetAsync(c->bufs[which].ptr, 0, bytes + 16, c->stream));
        return AWSM_OK;
    }
    int rc = dev_realloc(c, c->bufs[which], bytes ? bytes + 16 : 0, true);
    if (rc) return rc;
    if (bytes) c->bufs[which].size = bytes;
    if (which == AWSM_BUF_CAMERA) memset(c->camera_host, 0, sizeof c->camera_host);      // "contents are NOT preserved": the host shadow neither
    if (which == AWSM_BUF_LIGHTS) for (int sl = 0; sl < n_slots(c); sl++) if ((rc = dev_realloc(c, c->lights_pre[sl], std::max<size_t>(bytes / 64, 1) * 32, true))) return rc;   // 2 x float4 per 64-byte light
    c->scene_dirty = true;
    return AWSM_OK;
}

int awsm_hip_buffer_write(AwsmHipCtx* c, AwsmBuf which, size_t dst_off, const void* src, size_t len) {
    if (!c || (int)which < 0 || which >= AWSM_BUF_COUNT || (!src && len)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "buffer_write: bad argument");
    if ((dst_off & 3) || (len & 3)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "buffer_write: offset %zu / size %zu not 4-byte aligned", dst_off, len);
    DevBuf& b = c->bufs[which];
    if (!b.ptr) return fail(c, AWSM_ERR_NOT_READY, "buffer_write: buffer %d was never created", (int)which);
    if (dst_off > b.size || len > b.size - dst_off) return fail(c, AWSM_ERR_OUT_OF_RANGE, "buffer_write: [%zu,+%zu) outside buffer %d of %zu bytes", dst_off, len, (int)which, b.size);
    if (len == 0) return AWSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (which != AWSM_BUF_CAMERA) { int rcb = scene_write_barrier(c); if (rcb) return rcb; log_dirty(c, which, dst_off, dst_off + len); }   // the opaque pass reads a per-frame camera snapshot
    else { if (dst_off < 512) memcpy(c->camera_host + dst_off, src, std::min<size_t>(len, 512 - dst_off)); c->camera_written_since_snapshot = true; }
    uint8_t* dst = (uint8_t*)b.ptr + dst_off;
    if (len <= (1u << 20)) return upload_small(c, dst, src, len);
    // large (resize-time) uploads: the runtime stages pageable memory itself; wait so `src` is not retained
    HIPCHK(c, hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AWSM_OK;
}

// ---- skin matrices composed on the device (include/awsm_hip.h; kernels_pose.hip) ----
int awsm_hip_skin_pose_records_write(AwsmHipCtx* c, uint32_t first, uint32_t n, const AwsmSkinPoseRecord* records) {
    if (!c || (!records && n)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "skin_pose_records_write: bad argument");
    static_assert(sizeof(AwsmSkinPoseRecord) == 72, "k_skin_pose reads 72-byte records");
    std::vector<AwsmSkinPoseRecord>& host = c->pose_records_host;
    if (first > host.size() || n > 0x03000000u - first) return fail(c, AWSM_ERR_OUT_OF_RANGE, "skin_pose_records_write: [%u,+%u) with %zu records resident", first, n, host.size());
    if (n == 0) return AWSM_OK;
    for (uint32_t i = 0; i < n; i++)
        if ((records[i].transform_offset & 3u) || (records[i].matrix_offset & 3u)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "skin_pose_records_write: record %u has an offset that is not a multiple of 4", first + i);
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c, false); if (rcb) return rcb; }
    // the records as they will be: the context's copy, against which lists are checked, takes them only once the device has them
    std::vector<AwsmSkinPoseRecord> next(host.begin(), host.end());
    if (next.size() < (size_t)first + n) next.resize((size_t)first + n);
    memcpy(next.data() + first, records, (size_t)n * sizeof(AwsmSkinPoseRecord));
    size_t lo = first, count = n;
    if (c->pose_records.size < next.size() * sizeof(AwsmSkinPoseRecord)) {      // grow by doubling; dev_realloc keeps nothing, so everything goes up again
        const size_t cap = std::max<size_t>(std::max<size_t>(c->pose_records.size / sizeof(AwsmSkinPoseRecord) * 2, next.size()), 64);
        int rc = dev_realloc(c, c->pose_records, cap * sizeof(AwsmSkinPoseRecord), false);
        if (rc) { host.clear(); return rc; }      // nothing is resident any more
        lo = 0; count = next.size();
    }
    constexpr size_t kChunk = 8192;      // records per staged copy (576 KiB)
    for (size_t at = lo; at < lo + count; at += kChunk) {
        const size_t m = std::min(kChunk, lo + count - at);
        int rc = upload_small(c, (uint8_t*)c->pose_records.ptr + at * sizeof(AwsmSkinPoseRecord), next.data() + at, m * sizeof(AwsmSkinPoseRecord));
        if (rc) { host.clear(); return rc; }      // part of the array may be neither the old nor the new records: no list passes until it is written again from 0
    }
    host.swap(next);
    return AWSM_OK;
}

int awsm_hip_skin_pose(AwsmHipCtx* c, const uint32_t* ids, uint32_t n) {
    if (!c || (!ids && n)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "skin_pose: bad argument");
    if (n == 0) return AWSM_OK;
    const DevBuf& tb = c->bufs[AWSM_BUF_TRANSFORMS];
    const DevBuf& mb = c->bufs[AWSM_BUF_SKIN_MATRICES];
    if (!tb.ptr || !mb.ptr) return fail(c, AWSM_ERR_NOT_READY, "skin_pose: the transforms or the skin matrices buffer was never created");
    const std::vector<AwsmSkinPoseRecord>& host = c->pose_records_host;
    // everything is checked before anything is enqueued: a refused list writes nothing
    std::vector<uint32_t> offs(n);
    for (uint32_t i = 0; i < n; i++) {
        if (ids[i] >= host.size()) return fail(c, AWSM_ERR_OUT_OF_RANGE, "skin_pose: record id %u (list entry %u) with %zu records resident", ids[i], i, host.size());
        const AwsmSkinPoseRecord& r = host[ids[i]];
        if (tb.size < 64 || r.transform_offset > tb.size - 64) return fail(c, AWSM_ERR_OUT_OF_RANGE, "skin_pose: record %u reads [%u,+64) of a transforms buffer of %zu bytes", ids[i], r.transform_offset, tb.size);
        if (mb.size < 64 || r.matrix_offset > mb.size - 64) return fail(c, AWSM_ERR_OUT_OF_RANGE, "skin_pose: record %u writes [%u,+64) of a skin matrices buffer of %zu bytes", ids[i], r.matrix_offset, mb.size);
        offs[i] = r.matrix_offset;
    }
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }      // as awsm_hip_buffer_write(AWSM_BUF_SKIN_MATRICES): behind the opaque passes in flight
    std::sort(offs.begin(), offs.end());
    for (size_t i = 0; i < offs.size();) {      // one dirty range per run of adjacent matrices: the geometry cache recomputes the skinned draws they belong to
        size_t j = i + 1;
        while (j < offs.size() && offs[j] <= offs[j - 1] + 64u) j++;
        log_dirty(c, AWSM_BUF_SKIN_MATRICES, offs[i], (size_t)offs[j - 1] + 64);
        i = j;
    }
    constexpr uint32_t kChunk = 65536;      // ids per launch: 256 KiB of the pinned ring
    for (uint32_t at = 0; at < n; at += kChunk) {
        const uint32_t m = std::min(kChunk, n - at);
        uint8_t* st;
        int rc = stage_alloc(c, (size_t)m * 4, &st);
        if (rc) return rc;
        memcpy(st, ids + at, (size_t)m * 4);
        awsm_launch_skin_pose(c->pose_records.ptr, (const uint32_t*)st, m, tb.ptr, mb.ptr, c->stream);      // pinned memory is device-visible at the same address
        HIPCHK(c, hipGetLastError());
    }
    return AWSM_OK;
}

int awsm_hip_buffer_read(AwsmHipCtx* c, AwsmBuf which, size_t offset, void* dst, size_t len) {
    if (!c || (int)which < 0 || which >= AWSM_BUF_COUNT || (!dst && len)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "buffer_read: bad argument");
    const DevBuf& b = c->bufs[which];
    if (!b.ptr) return fail(c, AWSM_ERR_NOT_READY, "buffer_read: buffer %d was never created", (int)which);
    if (offset > b.size || len > b.size - offset) return fail(c, AWSM_ERR_OUT_OF_RANGE, "buffer_read: [%zu,+%zu) outside buffer %d of %zu bytes", offset, len, (int)which, b.size);
    if (len == 0) return AWSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // every write to a scene buffer is enqueued on the caller's stream
    HIPCHK(c, hipMemcpy(dst, (const uint8_t*)b.ptr + offset, len, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_resize(AwsmHipCtx* c, uint32_t width, uint32_t height, uint32_t msaa) {
    if (!c || width == 0 || height == 0 || width > 16384 || height > 16384) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "resize: bad size %ux%u", width, height);
    if (msaa == 1) msaa = 0;
    if (msaa != 0 && msaa != 4) return fail(c, AWSM_ERR_UNSUPPORTED, "resize: MSAA x%u (the reference supports None or 4, anti_alias.rs:28-38)", msaa);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height, samples = msaa == 4 ? 4 : 1;
    int rc;
    if ((rc = sync_all(c))) return rc;
    for (int s = 0; s < n_slots(c); s++) {
        if ((rc = dev_realloc(c, c->fb[s].vis, px * samples * 8, false))) return rc;
        HIPCHK(c, hipMemsetAsync(c->fb[s].vis.ptr, 0xFF, px * samples * 8, c->stream));
    }
    if (msaa == 4) for (int sl = 0; sl < n_slots(c); sl++) {
        const size_t blocks = (size_t)((width + 15) / 16) * ((height + 15) / 16);
        if ((rc = dev_realloc(c, c->msaa_edge_bits[sl], blocks * 4 * 16, true))) return rc;
        if ((rc = dev_realloc(c, c->msaa_cells[sl], px * 8, false))) return rc;
        if ((rc = dev_realloc(c, c->msaa_color0[sl], px * 16, false))) return rc;
        if ((rc = dev_realloc(c, c->msaa_edges[sl], blocks * 260, false))) return rc;      // per 16x16 block: count + 256 one-byte slots
    }
    c->msaa = msaa;
    for (int sl = 0; sl < n_slots(c); sl++) if ((rc = dev_realloc(c, c->shade_todo[sl], ((size_t)((width + 15) / 16) * ((height + 15) / 16) * 4 + 4 + 1024) * 4, true))) return rc;   // one entry per wavefront of the opaque grid
    for (int sl = 0; sl < n_slots(c); sl++) {
        if ((rc = dev_realloc(c, c->out16[sl], px * 8, true))) return rc;
        if ((c->flags & AWSM_CFG_PARITY_TAP) && (rc = dev_realloc(c, c->out32[sl], px * 16, true))) return rc;
    }
    c->width = width; c->height = height;
    c->y0 = c->y1 = 0;
    c->band_n = 1; c->band_r = 0; c->band_compact = 0;
    c->geometry_done = c->opaque_done = c->transparent_done = c->hud_transparent_done = c->post_done = false;
    c->last_display = nullptr;      // the images are sized for the old frame
    c->taa_have = false; c->taa_serial = 0; c->taa_resolved = false;      // ... and so is the TAA history (a new MSAA mode drops it too)
    return AWSM_OK;
}

int awsm_hip_set_shard_bands(AwsmHipCtx* c, uint32_t n, uint32_t r, uint32_t compact_output) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (c->width == 0) return fail(c, AWSM_ERR_NOT_READY, "set_shard_bands before resize");
    if (n == 0 || r >= n) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_shard_bands: need r < n (got n=%u r=%u)", n, r);
    { int rcs = sync_all(c); if (rcs) return rcs; }
    c->y0 = c->y1 = 0;                                   // bands and row ranges are alternatives
    c->band_n = n; c->band_r = n > 1 ? r : 0; c->band_compact = (n > 1 && compact_output) ? 1u : 0u;
    return AWSM_OK;
}

uint32_t awsm_hip_msaa_halo_bands(AwsmHipCtx* c) {
    return (c && c->band_n > 1 && c->height) ? ((c->height + kTile - 1) / kTile + c->band_n - 1) / c->band_n : 0u;
}

int awsm_hip_msaa_halo_export(AwsmHipCtx* c, void* dst, size_t bytes) {
    if (!c || !dst) return AWSM_ERR_INVALID_ARGUMENT;
    if (c->msaa != 4 || c->band_n <= 1) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "msaa_halo_export: only for MSAA x4 with band sharding");
    if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "msaa_halo_export before geometry_pass");
    const uint32_t bands = awsm_hip_msaa_halo_bands(c);
    if (bytes < (size_t)bands * 2 * c->width * 8) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "msaa_halo_export: %zu bytes, %zu needed (%u bands x 2 rows x %u keys)", bytes, (size_t)bands * 2 * c->width * 8, bands, c->width);
    HIPCHK(c, hipSetDevice(c->device));
    FrameDev f;
    fill_frame(c, &f, frame_view(c));
    awsm_launch_msaa_halo_export(&f, (unsigned long long*)dst, bands, c->stream);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int awsm_hip_msaa_halo_bind(AwsmHipCtx* c, const void* gathered, size_t bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (gathered && bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "msaa_halo_bind: zero-sized array");
    c->msaa_halo = gathered; c->msaa_halo_bytes = bytes;
    return AWSM_OK;
}

int awsm_hip_set_shard_rows(AwsmHipCtx* c, uint32_t y0, uint32_t y1) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (c->width == 0) return fail(c, AWSM_ERR_NOT_READY, "set_shard_rows before resize");
    { int rcs = sync_all(c); if (rcs) return rcs; }
    c->band_n = 1; c->band_r = 0; c->band_compact = 0;   // bands and row ranges are alternatives
    if (y0 == 0 && y1 == 0) { c->y0 = c->y1 = 0; return AWSM_OK; }
    if (y0 >= y1 || y1 > c->height) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_shard_rows: need y0 < y1 <= height (got %u,%u)", y0, y1);

    c->y0 = y0; c->y1 = y1;
    return AWSM_OK;
}

int awsm_hip_geometry_pass(AwsmHipCtx* c, const AwsmDraw* draws, uint32_t n) {
    if (!c || (!draws && n)) return AWSM_ERR_INVALID_ARGUMENT;
    if (c->width == 0) return fail(c, AWSM_ERR_NOT_READY, "geometry_pass before resize");
    static const AwsmBuf need[] = {AWSM_BUF_TRANSFORMS, AWSM_BUF_CAMERA, AWSM_BUF_GEOM_META, AWSM_BUF_VIS_GEOM_DATA};
    if (n) for (AwsmBuf b : need) if (!c->bufs[b].ptr) return fail(c, AWSM_ERR_NOT_READY, "geometry_pass: buffer %d missing", (int)b);
    HIPCHK(c, hipSetDevice(c->device));

    // validate before touching any per-frame state: a failed call leaves the previous frame (and its slot) current
    HostTrace ht(c->frame_serial + 1u);
    std::vector<DrawDev> new_draws;
    uint64_t tris = 0, blocks = 0;
    int rc = build_draw_list(c, "geometry_pass", draws, n, AWSM_BUF_VIS_GEOM_DATA, 168u, new_draws, &tris, &blocks);
    if (rc) return rc;
    ht.mark("geometry_pass: draw list");
    if ((rc = handoff_check(c))) return rc;      // an earlier frame was dropped by a timed-out gate: said once, here or in frame_flush / frame_end
    c->hud_geometry_done = false; c->hud_merged = false;      // (a new frame: no hud pass yet)
    c->frame_serial++;
    if (c->overlap) {
        c->slot = (c->slot + 1) % kSlots;    // the opaque passes of the previous frames may still be reading the other slots
        // ... and the opaque pass of kSlots frames ago may still be reading THIS slot (its draw list, per-draw records): order everything
        // this call puts on the caller's stream — the draw-list upload included — after it
        // (asked on the host first: kSlots frames back it has usually finished, and a barrier packet on the caller's stream costs the frame 6-9 us)
        if (c->shade_pending[c->slot]) {
            if (hipEventQuery(c->ev_shade_done[c->slot]) != hipSuccess) HIPCHK(c, wait_slot_free(c));
            c->shade_pending[c->slot] = false;
        }
    }
    ht.mark("geometry_pass: slot-free wait");
    c->shadow_done = false; c->shadow_pass[c->slot].on = false; c->shadow_px[c->slot] = 0;      // no shadow pass in a frame: no shadow in that frame
    c->shadow_views[c->slot].n = 0;
    c->draws_api.assign(draws, draws + n);
    PassList& world = c->lists[kPassWorld];
    world.draws.swap(new_draws);
    {   // What earlier frames needed in their (triangle, tile) lists, as far as the GPU has reported it (pinned words written by k_bin_scan;
        // no wait).  A frame rendered without frame_end cannot be replayed: size the list ahead of the need instead, and count the
        // frames that did overflow (AwsmFrameStats.frames_with_dropped_bin_entries).
        uint32_t need = 0;
        for (int s = 0; s < kSlots; s++) {
            const volatile uint32_t* st = c->counters_host + 16 + 2 * s;
            const uint32_t entries = st[0], serial = st[1];      // serial: bit 31 = that frame overflowed the list it ran with (k_bin_scan's own verdict)
            if (serial == c->status_seen[s]) continue;
            c->status_seen[s] = serial;
            if (serial >> 31) c->dropped_frames++;
            need = std::max(need, entries);
        }
        for (int s = 0; s < n_slots(c); s++)
            if (need && (uint64_t)need * 4 > (uint64_t)c->fb[s].bin_capacity * 3 && c->fb[s].bin_list.ptr && !(c->flags & AWSM_CFG_SMALL_BIN_LIST)) {
                if ((rc = ensure_bin_capacity_of(c, c->fb[s], need + need / 2 + 1024))) return rc;
                if ((rc = reserve_raster_items(c, c->fb[s], false, dims_of(c, c->fb[s])))) return rc;
            }
    }
    world.total_tris = (uint32_t)tris; world.n_blocks = (uint32_t)blocks;
    ht.mark("geometry_pass: bin capacity");
    compose_pixel_to_view(c, FB(c));
    if ((rc = reserve_pass_buffers(c, FB(c), world.draws, world.total_tris, false))) return rc;
    ht.mark("geometry_pass: reserve + draw-list upload");
    if ((rc = enqueue_geometry(c))) return rc;
    c->camera_written_since_snapshot = false;
    c->geometry_done = true; c->opaque_done = false; c->transparent_done = false; c->hud_transparent_done = false; c->hud_geometry_done = false; c->post_done = false;
    return AWSM_OK;
}

// GeometryRenderPass::render(ctx, &renderables.hud, true) (render.rs:169-178, geometry/render_pass.rs:51-157 with is_hud): the hud meshes are drawn
// over the visibility targets (LoadOp::Load) with a depth buffer of their own, cleared — they hide the world whatever its depth, and depth-test among
// themselves.  Here: the same kernels into the slot's hud key buffer; the world's keys and depth stay as they are (the world transparent pass tests
// against them), and the opaque pass, the picker and the HUD transparent pass look at the hud keys.
static int enqueue_hud_geometry(AwsmHipCtx* c) {
    const FrameBufs& hb = pass_bufs(c, kPassHud);
    const PassList& world = c->lists[kPassWorld];
    const PassList& hud = c->lists[kPassHud];
    FrameDev f;
    fill_frame(c, &f, FrameView{false, c->hud_merged});      // no hud keys yet; merged: the lean route's offsets must hold for both passes' triangles
    bind_pass(f, hb);      // the tile tables, the lists, the counters and the keys are this pass's own in either mode
    f.shade_todo = nullptr; f.shade_todo_cap = 0; f.lean_next = nullptr; f.lean_grid = 0;      // (k_deform_transform's per-frame resets of the opaque pass's lists: the world pass's)
    if (c->hud_merged) {
        // MSAA: the hud draws in the world pass's rank space — vertices, setup records and per-triangle words go behind the world's in the SAME arrays
        // (f keeps the world's list and arrays, and its lean records), only the tile tables, the lists and the keys are this pass's own
        const FrameBufs& wb = FB(c);
        f.draws = (const DrawDev*)wb.draws_dev.ptr;
        f.clip = (float4*)wb.clip.ptr; f.nrm = (float4*)wb.nrm.ptr; f.tan = (float4*)wb.tan.ptr;
        f.tri_info = (uint32_t*)wb.tri_flags.ptr;
        f.tri_rec = (TriRec*)wb.tri_rec.ptr;
        f.n_draws = (uint32_t)c->hud_combined.size();
        f.total_tris = world.total_tris + hud.total_tris; f.total_verts = 3u * f.total_tris;
        f.rank0 = world.total_tris; f.block0 = world.n_blocks;
    } else {
        f.n_draws = (uint32_t)hud.draws.size();
        f.total_tris = hud.total_tris; f.total_verts = 3u * hud.total_tris;
        f.tri_shade = nullptr; f.draw_lean = nullptr;
    }
    f.host_bin_status = nullptr;                 // the world pass's status words are not this pass's to write
    f.camera_snap = nullptr; f.camera_snap_words = 0;
    // (f.vis, this pass's keys: every tile of the frame is written — a tile without hud triangles becomes "no hit")
    int rc;
    if ((rc = sync_scene(c))) return rc;
    const uint32_t n_tiles = f.tiles_x * f.tiles_y;
    awsm_launch_transform(c->scene_dev, &f, hud.n_blocks, c->stream);      // (unconditionally, and no memsets: this pass is enqueued only with triangles)
    if (n_tiles) {
        enqueue_binning(f, true, c->stream);
        awsm_launch_raster(&f, c->stream);
    }
    if (c->hud_merged) {      // what the opaque pass reads: per sample the hud triangle (where one was drawn) under the world's depth
        const size_t spp = samples_of(c), first = (size_t)f.y0 * c->width * spp, n = (size_t)(f.y1 - f.y0) * c->width * spp;
        awsm_launch_hud_merge((const unsigned long long*)FB(c).vis.ptr, (const unsigned long long*)hb.vis.ptr, (unsigned long long*)c->merged_vis[c->slot].ptr, first, n, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int awsm_hip_hud_geometry_pass(AwsmHipCtx* c, const AwsmDraw* draws, uint32_t n) {
    if (!c || (!draws && n)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done || c->opaque_done) return fail(c, AWSM_ERR_NOT_READY, "hud_geometry_pass goes between the geometry pass and the opaque pass of a frame");
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t tris = 0, blocks = 0;
    PassList& hud = c->lists[kPassHud];
    const PassList& world = c->lists[kPassWorld];
    int rc = build_draw_list(c, "hud_geometry_pass", draws, n, AWSM_BUF_VIS_GEOM_DATA, 168u, hud.draws, &tris, &blocks);
    if (rc) return rc;
    hud.total_tris = (uint32_t)tris; hud.n_blocks = (uint32_t)blocks;
    c->hud_merged = false;
    if (!tris) { c->hud_geometry_done = false; return AWSM_OK; }
    FrameBufs& hb = pass_bufs(c, kPassHud);
    const size_t px = (size_t)c->width * c->height, spp = samples_of(c);
    if ((rc = dev_reserve(c, hb.vis, px * 8 * spp))) return rc;
    if ((rc = reserve_pass_buffers(c, hb, hud.draws, hud.total_tris, false))) return rc;      // tile tables, lists (and, single-sampled, the pass's own vertex arrays)
    if (c->msaa == 4) {
        // one rank space with the world pass (see AwsmHipCtx::hud_merged)
        if ((uint64_t)world.total_tris + tris > 0x55555555ull) return fail(c, AWSM_ERR_UNSUPPORTED, "hud_geometry_pass: more than 2^32/3 triangles in the frame");
        c->hud_combined = world.draws;
        for (DrawDev d : hud.draws) { d.first_tri += world.total_tris; d.first_block += world.n_blocks; c->hud_combined.push_back(d); }
        if (c->hud_combined.size() >= (1u << 24)) return fail(c, AWSM_ERR_UNSUPPORTED, "hud_geometry_pass: more than 2^24 draws in the frame");
        FrameBufs& wb = FB(c);
        const void* before[3] = {wb.clip.ptr, wb.tri_rec.ptr, wb.tri_flags.ptr};
        if ((rc = ensure_pass_capacity(c, wb, c->hud_combined, world.total_tris + hud.total_tris, false))) return rc;      // room for the hud draws behind the world's
        // The world's list stays cached as the world pass uploaded it (re-uploaded only if the list buffer just moved); the hud draws go behind it with a
        // cache of their own — a static scene with a hud mesh uploads nothing per frame and keeps its per-draw records (the combined list used to
        // replace the world list's cache, so both were uploaded every frame and k_resolve_draws never rested).
        if ((rc = upload_draw_list(c, wb, world.draws, true))) return rc;
        {
            const size_t at = world.draws.size();
            const std::vector<DrawDev> tail(c->hud_combined.begin() + (long)at, c->hud_combined.end());
            const bool same = wb.tail_uploaded_valid && wb.tail_uploaded_ptr == wb.draws_dev.ptr && wb.tail_uploaded_at == at && wb.tail_uploaded.size() == tail.size() &&
                              memcmp(wb.tail_uploaded.data(), tail.data(), tail.size() * sizeof(DrawDev)) == 0;
            if (!same) {
                if ((rc = upload_draws_at(c, wb, at, tail))) return rc;
                wb.tail_uploaded = tail; wb.tail_uploaded_ptr = wb.draws_dev.ptr; wb.tail_uploaded_at = at; wb.tail_uploaded_valid = true; wb.draws_version++;
                // The upload sits on the caller's stream BEHIND the world geometry pass, after ev_uploads[slot] was recorded: a per-draw resolve that went
                // ahead on that event would read hud entries that are not there yet (out-of-bounds meta offsets on a slot's first frame, the
                // list of two frames ago afterwards).  The resolve of this frame takes the late order, behind the geometry pass's hand-off.
                c->uploads_recorded[c->slot] = false;
            }
        }
        if ((rc = dev_reserve(c, c->merged_vis[c->slot], px * 8 * spp))) return rc;
        if (before[0] != wb.clip.ptr || before[1] != wb.tri_rec.ptr || before[2] != wb.tri_flags.ptr) {
            // the world pass's arrays moved (first frame with this much hud geometry): its results went with them — run it again into the new ones
            if ((rc = enqueue_geometry(c, true))) return rc;
        }
        c->hud_merged = true;
    }
    if ((rc = enqueue_hud_geometry(c))) return rc;
    c->hud_geometry_done = true;
    return AWSM_OK;
}

// ---- shadows: the geometry pass from the light (kernels_shadow.hip holds the resolve) ----
// The casters through the world pass's kernels into the slot's S x S map, with buffers of its own and the precautions of enqueue_hud_geometry: no
// camera snapshot, no status words, the opaque pass's lists nulled, no geometry cache — nothing the world pass left is reset.  k_deform_transform
// reads view_proj through the scene table: it is given the slot's second copy of the table, whose camera entry is the slot's copy of the light block.
// One view of the light: `casters` (already in the pass's list buffer) seen through the light block `block` (already in the slot's second scene
// table) into the S x S keys at `vis`, counting in `counters`.  Both entries and the replay of awsm_hip_frame_end come through here.
static int enqueue_shadow_view(AwsmHipCtx* c, const PassList& casters, const uint8_t* block, uint32_t* counters, unsigned long long* vis) {
    const FrameBufs& sb = pass_bufs(c, kPassShadow);
    const uint32_t S = c->shadow_pass[c->slot].p.map_size;
    FrameDev f;
    memset(&f, 0, sizeof f);
    f.width = S; f.height = S; f.y0 = 0; f.y1 = S; f.sy0 = 0; f.sy1 = S;
    f.tiles_x = (S + kTile - 1) / kTile; f.tiles_y = f.tiles_x; f.tile_row0 = 0;
    f.band_n = 1; f.band_r = 0; f.out_compact = 0;
    f.n_draws = (uint32_t)casters.draws.size();
    f.total_tris = casters.total_tris; f.total_verts = 3u * casters.total_tris;
    f.msaa = 0;                                  // single-sampled, whatever the frame is
    f.camera = block;
    bind_pass(f, sb);
    f.counters = counters;
    f.vis = vis;                                 // (the map: every tile of it is written, a tile without casters becomes "no hit")
    f.poison = c->handoff_poison ? c->handoff_poison + c->slot : nullptr;
    f.frame_serial = c->frame_serial;
    const uint32_t n_tiles = f.tiles_x * f.tiles_y;      // (S >= 1: never 0 — the map is always scanned and rasterised)
    if (!f.total_tris) { const int rc = clear_empty_pass(c, sb, counters, n_tiles, c->stream); if (rc) return rc; }
    else awsm_launch_transform(c->shadow_scene[c->slot], &f, casters.n_blocks, c->stream);      // through the slot's second scene table
    enqueue_binning(f, f.total_tris != 0, c->stream);
    awsm_launch_raster(&f, c->stream);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

// The slot's second scene table: the context's, with `block` as its camera entry
static int upload_shadow_scene(AwsmHipCtx* c, const uint8_t* block) {
    DevScene sc = c->scene;
    sc.buf[AWSM_BUF_CAMERA] = block;
    return upload_small(c, c->shadow_scene[c->slot], &sc, sizeof sc);
}

// awsm_hip_shadow_pass's one view: the pass's own list, counters and map; the table copy is made again only when the scene table was uploaded since
static int enqueue_shadow(AwsmHipCtx* c) {
    const FrameBufs& sb = pass_bufs(c, kPassShadow);
    const uint8_t* const block = (const uint8_t*)c->shadow_cam[c->slot].ptr;
    int rc;
    if ((rc = sync_scene(c))) return rc;
    if (c->shadow_scene_seq[c->slot] != c->scene_uploads) {
        if ((rc = upload_shadow_scene(c, block))) return rc;
        c->shadow_scene_seq[c->slot] = c->scene_uploads;
    }
    return enqueue_shadow_view(c, c->lists[kPassShadow], block, (uint32_t*)sb.counters.ptr, (unsigned long long*)sb.vis.ptr);
}

// awsm_hip_shadow_pass_views' views, in their order on the caller's stream, into layer i of the slot's stack of maps.  The views
// share the pass's vertex arrays, setup records, tile tables and lists: in front of each view's kernels its draw list goes into the pass's list
// buffer and its block into the slot's second table.  Each view counts its overflow in 16 words of its own.
static int enqueue_shadow_views(AwsmHipCtx* c) {
    FrameBufs& sb = pass_bufs(c, kPassShadow);
    const AwsmHipCtx::ShadowViews& views = c->shadow_views[c->slot];
    const size_t S = c->shadow_pass[c->slot].p.map_size;
    int rc;
    if ((rc = sync_scene(c))) return rc;
    c->shadow_scene_seq[c->slot] = ~0ull;      // the slot's second table is rewritten per view: awsm_hip_shadow_pass makes its own copy anew
    for (uint32_t i = 0; i < views.n; i++) {
        const uint8_t* const block = (const uint8_t*)c->shadow_cam[c->slot].ptr + (size_t)i * 512;
        if ((rc = upload_draw_list(c, sb, views.lists[i].draws, false))) return rc;
        if ((rc = upload_shadow_scene(c, block))) return rc;
        if ((rc = enqueue_shadow_view(c, views.lists[i], block, (uint32_t*)c->shadow_view_ctr[c->slot].ptr + (size_t)i * 16, (unsigned long long*)sb.vis.ptr + i * S * S))) return rc;
    }
    return AWSM_OK;
}

// The frame's shadow pass once more (awsm_hip_frame_end's replay; the light blocks are still in the slot's copy), and the counters it is judged
// by: the pass's own, or of a pass of views the largest need of any view and whether any view lost entries.
static int enqueue_frame_shadow(AwsmHipCtx* c) { return c->shadow_views[c->slot].n ? enqueue_shadow_views(c) : enqueue_shadow(c); }
static int read_shadow_counters(AwsmHipCtx* c, uint32_t worst[kCtrWords]) {
    const uint32_t n = c->shadow_views[c->slot].n;
    if (!n) { HIPCHK(c, hipMemcpy(worst, pass_bufs(c, kPassShadow).counters.ptr, kCtrWords * sizeof(uint32_t), hipMemcpyDeviceToHost)); return AWSM_OK; }
    uint32_t per_view[AWSM_SHADOW_MAX_VIEWS][16];
    HIPCHK(c, hipMemcpy(per_view, c->shadow_view_ctr[c->slot].ptr, (size_t)n * sizeof per_view[0], hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) {
        worst[kCtrEntries] = std::max(worst[kCtrEntries], per_view[i][kCtrEntries]);
        worst[kCtrOverflow] |= per_view[i][kCtrOverflow];
    }
    return AWSM_OK;
}

int awsm_hip_shadow_defaults(AwsmShadow* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmShadow d = {(uint32_t)sizeof(AwsmShadow), 2048u, 1u, {0.0f, 1.0f, 0.0f, 0.0f}, 1e-3f, 1.0f, 0.05f, 0.7f, 0.1f};
    *out = d;
    return AWSM_OK;
}

// What the two entries check alike.  `entry` names the caller in every message; `one` is its word for light[3] = 1.
// The AwsmShadow record: the caller's fields over the defaults, finite and in range -> full
static int check_shadow_record(AwsmHipCtx* c, const char* entry, const char* one, const AwsmShadow* s, AwsmShadow& full) {
    awsm_hip_shadow_defaults(&full);
    { const int rcm = merge_record(c, entry, "AwsmShadow", s, &full, sizeof full); if (rcm) return rcm; }
    { const int rcf = check_finite(c, entry, full.light, 9); if (rcf) return rcf; }      // light[4] and the five parameters are contiguous
    static_assert(offsetof(AwsmShadow, facing_fade) == offsetof(AwsmShadow, light) + 8 * sizeof(float) && sizeof(AwsmShadow) == 48, "AwsmShadow: light[4] and five floats behind three words");
    if (full.map_size < 1u || full.map_size > 8192u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: map_size = %u (1 .. 8192)", entry, full.map_size);
    if (full.pcf_radius > 2u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: pcf_radius = %u (0, 1 or 2)", entry, full.pcf_radius);
    if (!(full.strength >= 0.0f && full.strength <= 1.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: strength = %g (0 .. 1)", entry, (double)full.strength);
    if (!(full.facing_fade > 0.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: facing_fade = %g (> 0)", entry, (double)full.facing_fade);
    if (!(full.max_slope >= 0.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: max_slope = %g (>= 0)", entry, (double)full.max_slope);
    if (full.light[3] != 0.0f && full.light[3] != 1.0f) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: light[3] = %g (0: directional, 1: %s)", entry, (double)full.light[3], one);
    return AWSM_OK;
}
// A light block: 512 bytes in the camera buffer's layout with a finite view_proj -> lvp.  label: the entry, or the entry and the view.
static int check_light_block(AwsmHipCtx* c, const char* label, const void* block, size_t bytes, float lvp[16]) {
    if (!block || bytes != 512) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: the light camera is a 512-byte block in the layout of AWSM_BUF_CAMERA (got %zu bytes)", label, bytes);
    memcpy(lvp, (const uint8_t*)block + 128, 16 * sizeof(float));
    for (int k = 0; k < 16; k++) if (!std::isfinite(lvp[k])) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: the light camera's view_proj is not finite", label);
    return AWSM_OK;
}
// The scene buffers a pass with casters reads
static int check_caster_buffers(AwsmHipCtx* c, const char* entry) {
    for (AwsmBuf b : {AWSM_BUF_TRANSFORMS, AWSM_BUF_GEOM_META, AWSM_BUF_VIS_GEOM_DATA}) if (!c->bufs[b].ptr) return fail(c, AWSM_ERR_NOT_READY, "%s: buffer %d missing", entry, (int)b);
    return AWSM_OK;
}
// What a slot's shadow pass has besides its FrameBufs, made at the first use: the pass's 16 counter words, 16 per view for a pass of views
// (view_slots = AWSM_SHADOW_MAX_VIEWS; 0: none), the second scene table, and room for cam_blocks light blocks.
static int reserve_shadow_slot(AwsmHipCtx* c, uint32_t view_slots, uint32_t cam_blocks) {
    DevBuf* const words[2] = {&pass_bufs(c, kPassShadow).counters, &c->shadow_view_ctr[c->slot]};
    const size_t bytes[2] = {16 * sizeof(uint32_t), (size_t)view_slots * 16 * sizeof(uint32_t)};
    for (int k = 0; k < 2; k++) if (bytes[k] && !words[k]->ptr) {
        HIPCHK(c, hipMalloc(&words[k]->ptr, bytes[k]));
        words[k]->size = bytes[k];
        HIPCHK(c, hipMemsetAsync(words[k]->ptr, 0, bytes[k], c->stream));
    }
    if (!c->shadow_scene[c->slot]) { HIPCHK(c, hipMalloc((void**)&c->shadow_scene[c->slot], sizeof(DevScene))); c->shadow_scene_seq[c->slot] = 0; }
    return dev_reserve(c, c->shadow_cam[c->slot], (size_t)cam_blocks * 512);
}

int awsm_hip_shadow_pass(AwsmHipCtx* c, const AwsmShadow* s, const void* light_camera, size_t camera_bytes, const AwsmDraw* casters, uint32_t n) {
    if (!c || !s || (!casters && n)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done || c->opaque_done) return fail(c, AWSM_ERR_NOT_READY, "shadow_pass goes between the geometry pass and the opaque pass of a frame");
    if (is_sharded(c))
        return fail(c, AWSM_ERR_UNSUPPORTED, "shadow_pass on a sharded context: the resolve's neighbours need rows the shard never rasterised (no halo exchange)");
    AwsmShadow full;
    float lvp[16];
    int rc;
    if ((rc = check_shadow_record(c, "shadow_pass", "spot", s, full))) return rc;
    if ((rc = check_light_block(c, "shadow_pass", light_camera, camera_bytes, lvp))) return rc;
    if (n && (rc = check_caster_buffers(c, "shadow_pass"))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<DrawDev> list;
    uint64_t tris = 0, blocks = 0;
    if ((rc = build_draw_list(c, "shadow_pass", casters, n, AWSM_BUF_VIS_GEOM_DATA, 168u, list, &tris, &blocks))) return rc;
    // nothing refused from here on but for memory: the slot's state is this pass's
    FrameBufs& sb = pass_bufs(c, kPassShadow);
    PassList& cast = c->lists[kPassShadow];
    AwsmHipCtx::ShadowState& st = c->shadow_pass[c->slot];
    c->shadow_done = false; st.on = false;
    st.p = full; memcpy(st.light_view_proj, lvp, sizeof lvp);
    cast.draws.swap(list);
    cast.total_tris = (uint32_t)tris; cast.n_blocks = (uint32_t)blocks;
    if ((rc = reserve_shadow_slot(c, 0u, 1u))) return rc;
    if ((rc = dev_reserve(c, sb.vis, (size_t)full.map_size * full.map_size * 8))) return rc;
    if ((rc = reserve_pass_buffers(c, sb, cast.draws, cast.total_tris, false))) return rc;
    if ((rc = upload_small(c, c->shadow_cam[c->slot].ptr, light_camera, 512))) return rc;      // through the pinned ring, as small writes are
    c->shadow_views[c->slot].n = 0;      // (one map, k_shadow_resolve: not a pass of views)
    if ((rc = enqueue_shadow(c))) return rc;
    st.on = true; c->shadow_done = true;
    return AWSM_OK;
}

// Several views of one light
int awsm_hip_shadow_pass_views(AwsmHipCtx* c, const AwsmShadow* s, const AwsmShadowView* views, uint32_t n_views) {
    if (!c || !s) return AWSM_ERR_INVALID_ARGUMENT;
    if (!views || n_views < 1u || n_views > (uint32_t)AWSM_SHADOW_MAX_VIEWS)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "shadow_pass_views: %u views at %p (1 .. %d views)", n_views, (const void*)views, AWSM_SHADOW_MAX_VIEWS);
    if (!c->geometry_done || c->opaque_done) return fail(c, AWSM_ERR_NOT_READY, "shadow_pass_views goes between the geometry pass and the opaque pass of a frame");
    if (is_sharded(c))
        return fail(c, AWSM_ERR_UNSUPPORTED, "shadow_pass_views on a sharded context: the resolve's neighbours need rows the shard never rasterised (no halo exchange)");
    AwsmShadow full;
    int rc;
    if ((rc = check_shadow_record(c, "shadow_pass_views", "positional", s, full))) return rc;
    float lvp[AWSM_SHADOW_MAX_VIEWS][16];
    uint8_t blocks_host[AWSM_SHADOW_MAX_VIEWS * 512];
    char label[AWSM_SHADOW_MAX_VIEWS][40];      // "shadow_pass_views: view i"
    bool any_casters = false;
    for (uint32_t i = 0; i < n_views; i++) {
        const AwsmShadowView& v = views[i];
        snprintf(label[i], sizeof label[i], "shadow_pass_views: view %u", i);
        if (!v.casters && v.n_casters) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "shadow_pass_views: view %u has %u casters at a null pointer", i, v.n_casters);
        if ((rc = check_light_block(c, label[i], v.light_camera, v.camera_bytes, lvp[i]))) return rc;
        memcpy(blocks_host + (size_t)i * 512, v.light_camera, 512);
        any_casters |= v.n_casters != 0;
    }
    if (any_casters && (rc = check_caster_buffers(c, "shadow_pass_views"))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    PassList lists[AWSM_SHADOW_MAX_VIEWS];
    for (uint32_t i = 0; i < n_views; i++) {
        uint64_t tris = 0, blocks = 0;
        if ((rc = build_draw_list(c, label[i], views[i].casters, views[i].n_casters, AWSM_BUF_VIS_GEOM_DATA, 168u, lists[i].draws, &tris, &blocks))) return rc;
        lists[i].total_tris = (uint32_t)tris; lists[i].n_blocks = (uint32_t)blocks;
    }
    // nothing refused from here on but for memory: the slot's state is this pass's
    FrameBufs& sb = pass_bufs(c, kPassShadow);
    AwsmHipCtx::ShadowState& st = c->shadow_pass[c->slot];
    AwsmHipCtx::ShadowViews& vs = c->shadow_views[c->slot];
    c->shadow_done = false; st.on = false;
    st.p = full; memcpy(st.light_view_proj, lvp[0], sizeof st.light_view_proj);
    vs.n = n_views; memcpy(vs.view_proj, lvp, sizeof vs.view_proj);
    for (uint32_t i = 0; i < n_views; i++) { vs.lists[i].draws.swap(lists[i].draws); vs.lists[i].total_tris = lists[i].total_tris; vs.lists[i].n_blocks = lists[i].n_blocks; }
    c->lists[kPassShadow] = PassList();
    if ((rc = reserve_shadow_slot(c, AWSM_SHADOW_MAX_VIEWS, AWSM_SHADOW_MAX_VIEWS))) return rc;      // (the pass's own words too: a later awsm_hip_shadow_pass finds them)
    if ((rc = dev_reserve(c, sb.vis, (size_t)n_views * full.map_size * full.map_size * 8))) return rc;
    for (uint32_t i = 0; i < n_views; i++)      // grow-only: the arrays end up sized for the largest view
        if ((rc = ensure_pass_capacity(c, sb, vs.lists[i].draws, vs.lists[i].total_tris, false))) return rc;
    if ((rc = upload_small(c, c->shadow_cam[c->slot].ptr, blocks_host, (size_t)n_views * 512))) return rc;
    if ((rc = enqueue_shadow_views(c))) return rc;
    st.on = true; c->shadow_done = true;
    return AWSM_OK;
}

// Layer `view` of the last submitted frame's maps; `entry` names the caller in what is refused
static int read_shadow_layer(AwsmHipCtx* c, const char* entry, uint32_t view, uint64_t* keys) {
    if (!c || !keys) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->shadow_done || !c->shadow[c->slot].vis.ptr) return fail(c, AWSM_ERR_NOT_READY, "%s: the last submitted frame had no shadow pass", entry);
    const uint32_t n = std::max(c->shadow_views[c->slot].n, 1u);
    if (view >= n) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: view %u of a pass with %u", entry, view, n);
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    const size_t S = c->shadow_pass[c->slot].p.map_size;
    HIPCHK(c, hipMemcpy(keys, (const uint64_t*)c->shadow[c->slot].vis.ptr + (size_t)view * S * S, S * S * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}
int awsm_hip_read_shadow_map(AwsmHipCtx* c, uint64_t* keys) { return read_shadow_layer(c, "read_shadow_map", 0u, keys); }
int awsm_hip_read_shadow_map_view(AwsmHipCtx* c, uint32_t view, uint64_t* keys) { return read_shadow_layer(c, "read_shadow_map_view", view, keys); }

int awsm_hip_read_shadow_view(AwsmHipCtx* c, uint8_t* view_out) {
    if (!c || !view_out) return AWSM_ERR_INVALID_ARGUMENT;
    const size_t px = (size_t)c->width * c->height;
    if (!px || !c->shadow_done || !c->opaque_done || c->shadow_px[c->slot] != px || !c->shadow_views[c->slot].n || c->shadow_view_layers[c->slot].size < px)
        return fail(c, AWSM_ERR_NOT_READY, "read_shadow_view: the last submitted frame had no shadow_pass_views with an opaque pass (has_opaque) behind it");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(view_out, c->shadow_view_layers[c->slot].ptr, px, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_read_shadow(AwsmHipCtx* c, float* visibility, float* multiplier) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    const size_t px = (size_t)c->width * c->height;
    if (!px || !c->shadow_done || !c->opaque_done || c->shadow_px[c->slot] != px || !c->shadow_layers[c->slot].ptr)
        return fail(c, AWSM_ERR_NOT_READY, "read_shadow: the last submitted frame had no shadow pass with an opaque pass (has_opaque) behind it");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    const float* d = (const float*)c->shadow_layers[c->slot].ptr;
    if (visibility) HIPCHK(c, hipMemcpy(visibility, d, px * 4, hipMemcpyDeviceToHost));
    if (multiplier) HIPCHK(c, hipMemcpy(multiplier, d + px, px * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_opaque_pass(AwsmHipCtx* c, const AwsmOpaqueParams* p) {
    if (!c || !p) return AWSM_ERR_INVALID_ARGUMENT;
    if (p->mipmap > 1) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "opaque_pass: mipmap must be 0 (MipmapMode::None) or 1 (MipmapMode::Gradient)");
    if (c->width == 0) return fail(c, AWSM_ERR_NOT_READY, "opaque_pass before resize");
    if (p->has_opaque) {
        if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "opaque_pass before geometry_pass");
        static const AwsmBuf need[] = {AWSM_BUF_CAMERA, AWSM_BUF_GEOM_META, AWSM_BUF_MATERIAL_META, AWSM_BUF_MATERIALS, AWSM_BUF_ATTR_INDEX,
                                       AWSM_BUF_ATTR_DATA, AWSM_BUF_TEXTURE_TRANSFORMS, AWSM_BUF_LIGHTS_INFO, AWSM_BUF_LIGHTS};
        for (AwsmBuf b : need) if (!c->bufs[b].ptr) return fail(c, AWSM_ERR_NOT_READY, "opaque_pass: buffer %d missing", (int)b);
        if (!c->lut.ptr) return fail(c, AWSM_ERR_NOT_READY, "opaque_pass: no BRDF LUT (env_upload or brdf_lut_generate)");
    }
    if (c->msaa == 4 && c->band_n > 1 && p->has_opaque) {
        const size_t need = (size_t)c->band_n * awsm_hip_msaa_halo_bands(c) * 2 * c->width * 8;
        if (!c->msaa_halo || c->msaa_halo_bytes < need)
            return fail(c, AWSM_ERR_NOT_READY, "opaque_pass: MSAA with band sharding needs the gathered halo keys (awsm_hip_msaa_halo_export -> all-gather -> awsm_hip_msaa_halo_bind, %zu bytes)", need);
    }
    // screen-space ambient occlusion (awsm_hip_set_ssao): this pass carries the record as it stands now, into a replay too
    const bool ssao_on = c->ssao.on && p->has_opaque;
    if (ssao_on && is_sharded(c))
        return fail(c, AWSM_ERR_UNSUPPORTED, "opaque_pass with SSAO on a sharded context: its taps and its smoothing read depth in rows the shard never rasterised (no halo exchange)");
    HIPCHK(c, hipSetDevice(c->device));
    if (ssao_on) { const int rcs = dev_reserve(c, c->ssao_layers[c->slot], (size_t)c->width * c->height * 12); if (rcs) return rcs; }
    c->ssao_pass[c->slot] = c->ssao;
    c->ssao_pass[c->slot].on = ssao_on;
    c->ssao_px[c->slot] = ssao_on ? (size_t)c->width * c->height : 0;
    // shadows: the frame had a shadow pass (awsm_hip_shadow_pass) — its resolve goes behind this pass's shading kernels; V and m per frame slot, allocated at the first use
    const bool shadow_on = c->shadow_done && c->shadow_pass[c->slot].on && p->has_opaque;
    if (shadow_on) { const int rcs = dev_reserve(c, c->shadow_layers[c->slot], (size_t)c->width * c->height * 8); if (rcs) return rcs; }
    if (shadow_on && c->shadow_views[c->slot].n) { const int rcs = dev_reserve(c, c->shadow_view_layers[c->slot], (size_t)c->width * c->height); if (rcs) return rcs; }
    c->shadow_px[c->slot] = shadow_on ? (size_t)c->width * c->height : 0;
    c->last_opaque = *p;
    if (!p->has_opaque && c->camera_written_since_snapshot && c->bufs[AWSM_BUF_CAMERA].ptr) {
        // the "empty" pipeline (skybox only) may run without a geometry pass of its own: it then has no snapshot of the camera it was given.  Rare
        // and cheap to make right: drain, copy, go on.
        int rcs = materialize_clip(c);      // (a geometry pass of this slot may have left its clip positions to this snapshot)
        if (rcs) return rcs;
        if ((rcs = sync_all(c))) return rcs;
        compose_pixel_to_view(c, FB(c));
        HIPCHK(c, hipMemcpy(FB(c).camera.ptr, c->bufs[AWSM_BUF_CAMERA].ptr, std::min<size_t>(512, c->bufs[AWSM_BUF_CAMERA].size), hipMemcpyDeviceToDevice));
        c->camera_written_since_snapshot = false;
    }
    int rc = enqueue_opaque(c);
    if (rc) return rc;
    c->opaque_done = true; c->transparent_done = false; c->hud_transparent_done = false;
    return AWSM_OK;
}

// kind: the world transparent pass or the HUD one
static int transparent_pass_body(AwsmHipCtx* c, const AwsmDraw* draws, uint32_t n, PassKind kind) {
    const bool hud = kind == kPassHudTransparent;
    if (!c || (!draws && n)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done || !c->opaque_done) return fail(c, AWSM_ERR_NOT_READY, "transparent_pass needs the geometry and opaque passes of the same frame first");
    if (hud && !c->transparent_done) return fail(c, AWSM_ERR_NOT_READY, "hud_transparent_pass draws over the composite: call transparent_pass first (n_draws = 0 is valid)");
    const bool sharded = is_sharded(c);
    if (sharded && !c->opaque_src)
        return fail(c, AWSM_ERR_UNSUPPORTED, "transparent_pass on a sharded context: screen-space transmission reads the whole opaque image — gather it and bind it with awsm_hip_bind_opaque_source first");
    if (!hud && c->sel.on && sharded)
        return fail(c, AWSM_ERR_UNSUPPORTED, "transparent_pass with a selection on a sharded context: the outline's ring reads keys in rows the shard never rasterised (no halo exchange)");
    if (!hud && c->sel.on && !c->lists[kPassWorld].draws.empty() && (!c->bufs[AWSM_BUF_GEOM_META].ptr || !c->bufs[AWSM_BUF_MATERIAL_META].ptr))
        return fail(c, AWSM_ERR_NOT_READY, "transparent_pass with a selection: the geometry or material meta buffer is missing");
    if (c->opaque_src && c->opaque_src_bytes < (size_t)c->width * c->height * 8)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "transparent_pass: the bound opaque source holds %zu bytes, the frame needs %zu", c->opaque_src_bytes, (size_t)c->width * c->height * 8);
    static const AwsmBuf need[] = {AWSM_BUF_TRANSFORMS, AWSM_BUF_CAMERA, AWSM_BUF_GEOM_META, AWSM_BUF_MATERIAL_META, AWSM_BUF_MATERIALS, AWSM_BUF_ATTR_INDEX,
                                   AWSM_BUF_ATTR_DATA, AWSM_BUF_TEXTURE_TRANSFORMS, AWSM_BUF_LIGHTS_INFO, AWSM_BUF_LIGHTS, AWSM_BUF_TRANSPARENCY_GEOM_DATA};
    if (n) {
        for (AwsmBuf b : need) if (!c->bufs[b].ptr) return fail(c, AWSM_ERR_NOT_READY, "transparent_pass: buffer %d missing", (int)b);
        if (!c->lut.ptr) return fail(c, AWSM_ERR_NOT_READY, "transparent_pass: no BRDF LUT (env_upload or brdf_lut_generate)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t tris = 0, blocks = 0;
    PassList& list = c->lists[kind];
    FrameBufs& t = pass_bufs(c, kind);
    int rc = build_draw_list(c, hud ? "hud_transparent_pass" : "transparent_pass", draws, n, AWSM_BUF_TRANSPARENCY_GEOM_DATA, 0u, list.draws, &tris, &blocks);
    if (rc) return rc;
    list.total_tris = (uint32_t)tris; list.n_blocks = (uint32_t)blocks;
    const size_t px = (size_t)c->width * c->height;
    if (!c->bound_comp && (rc = dev_reserve(c, c->comp16, px * 8))) return rc;
    if (c->bound_comp && c->bound_comp_bytes < px * 8) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "transparent_pass: bound composite holds %zu bytes, the frame needs %zu", c->bound_comp_bytes, px * 8);
    if ((c->flags & AWSM_CFG_PARITY_TAP) && (rc = dev_reserve(c, c->comp32, px * 16))) return rc;
    if ((rc = reserve_pass_buffers(c, t, list.draws, list.total_tris, true))) return rc;
    if ((rc = dev_reserve(c, t.frag_first, px * 4))) return rc;
    if ((rc = ensure_fragment_capacity(c, t, (c->flags & AWSM_CFG_SMALL_BIN_LIST) ? 4096u : (uint32_t)std::max<size_t>(px / 2, 1u << 20)))) return rc;
    if (c->overlap) {   // the draw-list upload went to the caller's stream; the pass runs on the shade stream
        HIPCHK(c, hipEventRecord(c->ev_geom_done[c->slot], c->stream));
        HIPCHK(c, hipStreamWaitEvent(shade_stream_of(c), c->ev_geom_done[c->slot], 0));
    }
    if (!hud) c->grid_pass[c->slot] = c->grid;
    if (!hud) {      // the selection overlay: this pass carries the record as it stands now, into a replay too
        if (c->sel.on && (rc = dev_reserve(c, c->sel_tables[c->slot], (size_t)selection::kMaxEdges * selection::kEdgeFloats * 4 + std::max<size_t>(c->lists[kPassWorld].draws.size(), 1)))) return rc;
        c->sel_pass[c->slot] = c->sel;
    }
    if ((rc = enqueue_transparent(c, kind))) return rc;
    if (hud) c->hud_transparent_done = true; else { c->transparent_done = true; c->hud_transparent_done = false; }
    return AWSM_OK;
}
int awsm_hip_transparent_pass(AwsmHipCtx* c, const AwsmDraw* draws, uint32_t n) { return transparent_pass_body(c, draws, n, kPassTransparent); }
// MaterialTransparentRenderPass::render(ctx, renderables.hud, true) (render.rs:301-312, begin_hud_transparent_pass :490-521): the hud meshes drawn
// forward over what the frame holds so far (colours LoadOp::Load -> the composite, in place), depth-tested among themselves against hud_depth, cleared.
int awsm_hip_hud_transparent_pass(AwsmHipCtx* c, const AwsmDraw* draws, uint32_t n) { return transparent_pass_body(c, draws, n, kPassHudTransparent); }

int awsm_hip_set_stage_timers(AwsmHipCtx* c, int enabled) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    c->stage_timers = enabled != 0;
    return AWSM_OK;
}

int awsm_hip_frame_trace(AwsmHipCtx* c, uint32_t capacity) {
    if (!c || capacity > (1u << 20)) return AWSM_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    if (c->trace_dev) { HIPCHK(c, hipFree(c->trace_dev)); c->trace_dev = nullptr; c->trace_cap = 0; }
    if (!capacity) return AWSM_OK;
    HIPCHK(c, hipMalloc((void**)&c->trace_dev, (size_t)3 * capacity * 8));
    HIPCHK(c, hipMemset(c->trace_dev, 0, (size_t)3 * capacity * 8));
    c->trace_cap = capacity;
    return AWSM_OK;
}

int awsm_hip_read_frame_trace(AwsmHipCtx* c, uint64_t* ticks_out, uint32_t n_frames, uint32_t* last_serial_out, uint32_t* ticks_per_ms_out) {
    if (!c || !ticks_out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->trace_dev) return fail(c, AWSM_ERR_NOT_READY, "read_frame_trace: tracing is off (awsm_hip_frame_trace)");
    if (n_frames == 0 || n_frames > c->trace_cap) return fail(c, AWSM_ERR_OUT_OF_RANGE, "read_frame_trace: %u frames asked, the ring holds %u", n_frames, c->trace_cap);
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    std::vector<uint64_t> ring((size_t)3 * c->trace_cap);
    HIPCHK(c, hipMemcpy(ring.data(), c->trace_dev, ring.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n_frames; i++) {      // oldest first: frames serial - n + 1 .. serial
        const uint32_t serial = c->frame_serial - (n_frames - 1u - i);
        for (int w = 0; w < 3; w++) ticks_out[(size_t)i * 3 + w] = ring[(size_t)w * c->trace_cap + serial % c->trace_cap];
    }
    if (last_serial_out) *last_serial_out = c->frame_serial;
    if (ticks_per_ms_out) { int khz = 0; *ticks_per_ms_out = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0 ? (uint32_t)khz : 100000u; }
    return AWSM_OK;
}

int awsm_hip_frame_flush(AwsmHipCtx* c) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    // Nothing is batched host-side.  In overlap mode the opaque passes run on an internal stream: order them before whatever the
    // caller enqueues next on its own stream (a collective over the image, a copy, ...).
    { int rch = handoff_check(c); if (rch) return rch; }
    int rc = scene_write_barrier(c, false);
    if (rc || !c->overlap) return rc;
    // The streams' internal events release to device scope only (no cache write-back per record: see awsm_hip_create).  What follows a flush on the
    // caller's stream may be a DMA engine, a peer GPU or the host: one system-scope release here, where the caller asked for it.
    HIPCHK(c, hipEventRecord(c->ev_flush, c->stream));
    return AWSM_OK;
}

static int enqueue_post(AwsmHipCtx* c, const AwsmPostParams& p);
int awsm_hip_frame_end(AwsmHipCtx* c, AwsmFrameStats* out) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->device));
    const PassList& world_list = c->lists[kPassWorld];
    // the passes' counter words as read back (CounterWord): the world geometry pass's and the world transparent pass's in the pinned block
    const uint32_t* const world = c->counters_host;
    const uint32_t* const fwd = c->counters_host + 8;
    bool still_over = false;
    for (int attempt = 0;; attempt++) {
        if (out && c->geometry_done && c->has_opaque_for_stats()) {   // stats only: count covered pixels from the visibility buffer
            FrameDev f;
            fill_frame(c, &f, frame_view(c));
            HIPCHK(c, hipMemsetAsync((uint32_t*)FB(c).counters.ptr + kCtrCovered, 0, sizeof(uint32_t), c->stream));
            awsm_launch_count_covered(&f, c->stream);
        }
        HIPCHK(c, hipMemcpyAsync(c->counters_host, FB(c).counters.ptr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->cache_blocks_last = 0;
        if (out && c->geometry_done && c->stage_timers && world_list.n_blocks && FB(c).cache_mark.size >= (size_t)world_list.n_blocks * 4) {
            std::vector<uint32_t> marks(world_list.n_blocks);
            HIPCHK(c, hipMemcpy(marks.data(), FB(c).cache_mark.ptr, marks.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t m : marks) c->cache_blocks_last += m == c->frame_serial ? 1u : 0u;
        }
        if (c->overlap) { HIPCHK(c, sync_shade_streams(c)); for (bool& b : c->shade_pending) b = false; }
        { int rch = handoff_check(c); if (rch) return rch; }      // a gate ended unopened: the frame it guarded was dropped
        memset(c->counters_host + 8, 0, 8 * sizeof(uint32_t));
        uint32_t hud_fwd[kCtrWords] = {}, hud_geo[kCtrWords] = {}, shadow_geo[kCtrWords] = {};      // the HUD transparent pass's, the HUD geometry pass's and the shadow pass's own counters (same layout)
        if (c->shadow_done) { const int rcs = read_shadow_counters(c, shadow_geo); if (rcs) return rcs; }
        if (c->transparent_done) HIPCHK(c, hipMemcpy(c->counters_host + 8, pass_bufs(c, kPassTransparent).counters.ptr, kCtrWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (c->hud_transparent_done) HIPCHK(c, hipMemcpy(hud_fwd, pass_bufs(c, kPassHudTransparent).counters.ptr, sizeof hud_fwd, hipMemcpyDeviceToHost));
        if (c->hud_geometry_done) HIPCHK(c, hipMemcpy(hud_geo, pass_bufs(c, kPassHud).counters.ptr, sizeof hud_geo, hipMemcpyDeviceToHost));
        const bool geom_over = c->geometry_done && world[kCtrOverflow] != 0, fwd_over = c->transparent_done && fwd[kCtrOverflow] != 0;
        const bool frag_over = c->transparent_done && fwd[kCtrFragOverflow] != 0;      // a pixel's fragment list did not fit
        const bool hud_geo_over = c->hud_geometry_done && hud_geo[kCtrOverflow] != 0, hud_fwd_over = c->hud_transparent_done && hud_fwd[kCtrOverflow] != 0, hud_frag_over = c->hud_transparent_done && hud_fwd[kCtrFragOverflow] != 0;
        const bool shadow_over = c->shadow_done && shadow_geo[kCtrOverflow] != 0;
        still_over = geom_over || fwd_over || frag_over || hud_geo_over || hud_fwd_over || hud_frag_over || shadow_over;
        if (!still_over || attempt >= 4) break;
        // a list overflowed: grow it to the measured need and replay from the first pass that lost entries.  The passes of a frame are replayed in their
        // order — the HUD transparent pass blends into the composite in place, so it is never replayed by itself: the world transparent pass (which
        // starts from the opaque image) always goes first.
        int rc;
        c->overflow_retries++;
        if (geom_over) {
            if ((rc = grow_after_overflow(c, FB(c), world))) return rc;
            if ((rc = enqueue_geometry(c, true))) return rc;
        }
        if (hud_geo_over || (geom_over && c->hud_geometry_done && c->hud_merged)) {      // (merged keys: a new world pass needs a new merge)
            if (hud_geo_over && (rc = grow_after_overflow(c, pass_bufs(c, kPassHud), hud_geo))) return rc;
            if ((rc = enqueue_hud_geometry(c))) return rc;
        }
        if (shadow_over) {      // the light's pass, in its place between the geometry passes and the opaque pass; the light block is still in the slot's copy
            if ((rc = grow_after_overflow(c, pass_bufs(c, kPassShadow), shadow_geo))) return rc;
            if ((rc = enqueue_frame_shadow(c))) return rc;      // (of a pass of views every view again, in order)
        }
        if ((geom_over || hud_geo_over || shadow_over) && c->opaque_done && (rc = enqueue_opaque(c))) return rc;
        // (the transparent passes have a tile kernel of their own: no raster items to size with their lists)
        if (fwd_over && (rc = ensure_bin_capacity_of(c, pass_bufs(c, kPassTransparent), with_headroom(fwd[kCtrEntries])))) return rc;
        if (frag_over && (rc = ensure_fragment_capacity(c, pass_bufs(c, kPassTransparent), with_headroom(fwd[kCtrFragments])))) return rc;
        if (hud_fwd_over && (rc = ensure_bin_capacity_of(c, pass_bufs(c, kPassHudTransparent), with_headroom(hud_fwd[kCtrEntries])))) return rc;
        if (hud_frag_over && (rc = ensure_fragment_capacity(c, pass_bufs(c, kPassHudTransparent), with_headroom(hud_fwd[kCtrFragments])))) return rc;
        if (c->transparent_done) {
            if ((rc = enqueue_transparent(c, kPassTransparent))) return rc;
            if (c->hud_transparent_done && (rc = enqueue_transparent(c, kPassHudTransparent))) return rc;
        }
        if (c->post_done && (rc = enqueue_post(c, c->post_params))) return rc;     // the effects + display of the replayed images (and fragment lists)
    }
    if (still_over) return fail(c, AWSM_ERR_DEVICE, "bin / fragment list overflow persisted after retries");
    if (out) {
        // the caller says how much of the struct it knows (struct_size, ABI 2): nothing beyond that is written
        const uint32_t caller_size = out->struct_size;
        if (caller_size < 8u || caller_size > 4096u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "frame_end: AwsmFrameStats.struct_size = %u (set it to sizeof(AwsmFrameStats))", caller_size);
        AwsmFrameStats st_local;
        AwsmFrameStats* const caller_out = out;
        out = &st_local;
        memset(out, 0, sizeof *out);
        auto ms = [&](int a, int b) { float t = 0.0f; if (c->ev_valid[a] && c->ev_valid[b] && hipEventElapsedTime(&t, c->ev[a], c->ev[b]) == hipSuccess) return t; return 0.0f; };
        if (c->geometry_done) {
            out->ms_transform = ms(EV_START, EV_TRANSFORM);
            out->ms_bin = ms(EV_TRANSFORM, EV_BIN);
            out->ms_raster = ms(EV_BIN, EV_RASTER);
        }
        if (c->opaque_done) { out->ms_shade = ms(EV_SHADE_BEGIN, EV_SHADE); out->ms_shade_lean = ms(EV_SHADE_BEGIN, EV_SHADE_LEAN); }
        if (c->transparent_done) { out->ms_forward = ms(EV_FWD_BEGIN, EV_FWD); out->forward_triangles = c->lists[kPassTransparent].total_tris + (c->hud_transparent_done ? c->lists[kPassHudTransparent].total_tris : 0u); out->forward_fragment_slots = fwd[kCtrFragments]; }
        out->ms_total = (c->geometry_done ? ms(EV_START, EV_RASTER) : 0.0f) + out->ms_shade + out->ms_forward;   // the two passes may run on different streams
        out->triangles_in = world_list.total_tris;
        out->triangles_binned = world[kCtrBinned];
        out->bin_entries = world[kCtrEntries];
        out->covered_pixels = world[kCtrCovered];
        out->bin_overflow_retries = c->overflow_retries;
        out->frames_with_dropped_bin_entries = c->dropped_frames;
        out->handoff_gate_timeouts = c->handoff_dropped_frames;
        out->geometry_cache_blocks = (c->geometry_done && c->stage_timers) ? c->cache_blocks_last : 0u;
        out->geometry_blocks = c->geometry_done ? world_list.n_blocks : 0u;
        if (c->opaque_done && c->shade_todo[c->slot].ptr && c->last_opaque.has_opaque && !(c->flags & AWSM_CFG_GENERAL_SHADE_ONLY) && !world_list.draws.empty())
            HIPCHK(c, hipMemcpy(&out->shade_general_wavefronts, c->shade_todo[c->slot].ptr, 4, hipMemcpyDeviceToHost));
        out->struct_size = (uint32_t)std::min<size_t>(caller_size, sizeof(AwsmFrameStats));
        memcpy(caller_out, out, out->struct_size);
    }
    return AWSM_OK;
}

int awsm_hip_bind_output(AwsmHipCtx* c, void* device_ptr, size_t bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (device_ptr && bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "bind_output: zero-sized image");
    c->bound_out = device_ptr; c->bound_out_bytes = bytes; c->out_first_row = 0; c->out_rows_mode = false;   // checked against the shard layout when the opaque pass is enqueued
    return AWSM_OK;
}

int awsm_hip_bind_output_rows(AwsmHipCtx* c, void* device_ptr, size_t bytes, uint32_t first_row) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!device_ptr || bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "bind_output_rows: null or zero-sized image");
    c->bound_out = device_ptr; c->bound_out_bytes = bytes; c->out_first_row = first_row; c->out_rows_mode = true;
    return AWSM_OK;
}

void* awsm_hip_output_device_ptr(AwsmHipCtx* c) { return c ? (c->bound_out ? c->bound_out : c->out16[c->slot].ptr) : nullptr; }

int awsm_hip_read_visibility(AwsmHipCtx* c, uint64_t* keys_out) {
    if (!c || !keys_out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!FB(c).vis.ptr) return fail(c, AWSM_ERR_NOT_READY, "read_visibility before resize");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(keys_out, FB(c).vis.ptr, (size_t)c->width * c->height * samples_of(c) * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

#ifdef AWSM_STAMP
// diagnostic builds only: the geometry kernels' stamps of the last frame, [4 kernels][16384 workgroups][8] u64
extern "C" int awsm_hip_debug_read_stamps(AwsmHipCtx* c, unsigned long long* out) {
    FrameDev f;
    fill_frame(c, &f, frame_view(c));
    if (sync_all(c)) return AWSM_ERR_DEVICE;
    return hipMemcpy(out, f.stamps, 4ull * 16384 * 8 * 8, hipMemcpyDeviceToHost) == hipSuccess ? AWSM_OK : AWSM_ERR_DEVICE;
}
#endif

int awsm_hip_read_gbuffer(AwsmHipCtx* c, float* out6) {
    if (!c || !out6) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "read_gbuffer before geometry_pass");
    if (c->msaa != 0 || c->band_n > 1) return fail(c, AWSM_ERR_UNSUPPORTED, "read_gbuffer: single-sampled, unsharded-by-bands frames only");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    FrameDev f;
    fill_frame(c, &f, frame_view(c));
    const size_t bytes = (size_t)c->width * c->height * 6 * sizeof(float);
    float* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, bytes));
    awsm_launch_gbuffer_dump(&f, dev, c->stream);
    hipError_t e = hipMemcpyAsync(out6, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(dev);
    HIPCHK(c, e);
    return AWSM_OK;
}

int awsm_hip_stream_handoff(AwsmHipCtx* c) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    return c->overlap && c->handoff ? 1 : 0;
}

int awsm_hip_visibility_digest(AwsmHipCtx* c, uint64_t* out2) {
    if (!c || !out2) return AWSM_ERR_INVALID_ARGUMENT;
    if (!FB(c).vis.ptr) return fail(c, AWSM_ERR_NOT_READY, "visibility_digest before resize");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = dev_reserve(c, c->digest, 16);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(c->digest.ptr, 0, 16, c->stream));
    awsm_launch_vis_digest((const unsigned long long*)FB(c).vis.ptr, (size_t)c->width * c->height * samples_of(c), (unsigned long long*)c->digest.ptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out2, c->digest.ptr, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AWSM_OK;
}

int awsm_hip_read_visibility_unpacked(AwsmHipCtx* c, uint32_t* tri_id, uint32_t* meta_off, float* depth) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!FB(c).vis.ptr) return fail(c, AWSM_ERR_NOT_READY, "read_visibility before resize");
    const size_t n = (size_t)c->width * c->height * samples_of(c);
    std::vector<uint64_t> keys(n);
    int rc = awsm_hip_read_visibility(c, keys.data());
    if (rc) return rc;
    const std::vector<DrawDev>& world_draws = c->lists[kPassWorld].draws;
    std::vector<uint32_t> meta(world_draws.size());
    for (size_t d = 0; d < world_draws.size(); d++)
        HIPCHK(c, hipMemcpy(&meta[d], (const uint8_t*)c->bufs[AWSM_BUF_GEOM_META].ptr + world_draws[d].geom_meta_off + 36, 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) {
        if (keys[i] == ~0ull) {   // cleared texel: 0xFFFF per channel -> join32 == U32_MAX (geometry/render_pass.rs:22-30)
            if (tri_id) tri_id[i] = 0xFFFFFFFFu;
            if (meta_off) meta_off[i] = 0xFFFFFFFFu;
            if (depth) depth[i] = 1.0f;
            continue;
        }
        const uint32_t rank = 0xFFFFFFFFu - (uint32_t)(keys[i] & 0xFFFFFFFFull);
        size_t lo = 0, hi = world_draws.size();
        while (hi - lo > 1) { size_t mid = (lo + hi) / 2; if (world_draws[mid].first_tri <= rank) lo = mid; else hi = mid; }
        if (tri_id) tri_id[i] = rank - world_draws[lo].first_tri;
        if (meta_off) meta_off[i] = meta[lo];
        if (depth) { uint32_t b = (uint32_t)(keys[i] >> 32); memcpy(&depth[i], &b, 4); }
    }
    return AWSM_OK;
}

int awsm_hip_pick(AwsmHipCtx* c, int32_t x, int32_t y, AwsmPick* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "pick before geometry_pass");
    if (!c->bufs[AWSM_BUF_MATERIAL_META].ptr || !c->bufs[AWSM_BUF_GEOM_META].ptr) return fail(c, AWSM_ERR_NOT_READY, "pick: meta buffers missing");
    HIPCHK(c, hipSetDevice(c->device));
    FrameDev f;
    fill_frame(c, &f, frame_view(c));
    int rc = sync_scene(c);
    if (rc) return rc;
    uint32_t* dev_out = (uint32_t*)FB(c).counters.ptr + 8;          // 4 words after the frame counters
    awsm_launch_pick(c->scene_dev, &f, x, y, dev_out, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t host_out[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(host_out, dev_out, sizeof host_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->valid = host_out[0]; out->mesh_key_high = host_out[1]; out->mesh_key_low = host_out[2]; out->triangle_index = host_out[3];
    return AWSM_OK;
}

int awsm_hip_read_opaque(AwsmHipCtx* c, uint16_t* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    void* src = awsm_hip_output_device_ptr(c);
    if (!src) return fail(c, AWSM_ERR_NOT_READY, "read_opaque before resize");
    if (c->bound_out && c->out_rows_mode) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "read_opaque: the bound output is a row strip (bind_output_rows); read it from its owner");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, src, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_read_opaque_f32(AwsmHipCtx* c, float* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->out32[c->slot].ptr) return fail(c, AWSM_ERR_NOT_READY, "read_opaque_f32 needs AWSM_CFG_PARITY_TAP and a resize");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, c->out32[c->slot].ptr, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_bind_opaque_source(AwsmHipCtx* c, const void* device_ptr, size_t bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (device_ptr && bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "bind_opaque_source: zero-sized image");
    c->opaque_src = device_ptr; c->opaque_src_bytes = bytes;
    return AWSM_OK;
}

int awsm_hip_bind_composite(AwsmHipCtx* c, void* device_ptr, size_t bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (device_ptr && bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "bind_composite: zero-sized image");
    c->bound_comp = device_ptr; c->bound_comp_bytes = bytes;
    return AWSM_OK;
}

int awsm_hip_read_composite(AwsmHipCtx* c, uint16_t* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->transparent_done) return fail(c, AWSM_ERR_NOT_READY, "read_composite before transparent_pass");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, c->bound_comp ? c->bound_comp : c->comp16.ptr, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_read_composite_f32(AwsmHipCtx* c, float* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->transparent_done || !c->comp32.ptr) return fail(c, AWSM_ERR_NOT_READY, "read_composite_f32 needs AWSM_CFG_PARITY_TAP and a transparent_pass");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, c->comp32.ptr, (size_t)c->width * c->height * 16, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

// ---- the editor's ground grid (editor_grid.hpp) ----
int awsm_hip_editor_grid_defaults(AwsmEditorGrid* out) {      // grid.wgsl:87-98
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmEditorGrid d = {(uint32_t)sizeof(AwsmEditorGrid), {0.18f, 0.18f, 0.18f}, 0.7f, {0.28f, 0.28f, 0.28f}, 0.9f, {0.38f, 0.38f, 0.38f}, 1.0f,
                                     {0.3f, 0.5f, 0.95f}, 1.0f, {0.95f, 0.3f, 0.3f}, 1e-4f};
    *out = d;
    return AWSM_OK;
}
static_assert(sizeof(AwsmEditorGrid) == 4 + sizeof(EditorGridDev::p) && offsetof(AwsmEditorGrid, color_background) == 4, "EditorGridDev.p is AwsmEditorGrid behind struct_size");
int awsm_hip_set_editor_grid(AwsmHipCtx* c, const AwsmEditorGrid* g) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmEditorGrid full;
    awsm_hip_editor_grid_defaults(&full);
    if (g) {
        int rc = merge_record(c, "set_editor_grid", "AwsmEditorGrid", g, &full, sizeof full);
        if (!rc) rc = check_finite(c, "set_editor_grid", full.color_background, sizeof(EditorGridDev::p) / 4);
        if (rc) return rc;
    }
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }      // scene state like any other; the pass itself carries the record it was enqueued with
    c->grid.on = g != nullptr;
    memcpy(c->grid.p, full.color_background, sizeof c->grid.p);
    return AWSM_OK;
}
int awsm_hip_read_editor_grid(AwsmHipCtx* c, float* rgba, float* depth, uint8_t* kept) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!FB(c).camera.ptr || !c->width || !c->height) return fail(c, AWSM_ERR_NOT_READY, "read_editor_grid before the first geometry pass");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    const size_t px = (size_t)c->width * c->height;
    int rc = dev_reserve(c, c->grid_layer, px * 21);      // [px] float4, [px] float, [px] byte
    if (rc) return rc;
    EditorGridDev g;
    g.camera = (const uint8_t*)FB(c).camera.ptr;
    if (c->grid.on) memcpy(g.p, c->grid.p, sizeof g.p);
    else { AwsmEditorGrid d; awsm_hip_editor_grid_defaults(&d); memcpy(g.p, d.color_background, sizeof g.p); }
    float* d_rgba = (float*)c->grid_layer.ptr; float* d_depth = d_rgba + px * 4; uint8_t* d_kept = (uint8_t*)(d_depth + px);
    awsm_launch_editor_grid_layer(&g, c->width, c->height, d_rgba, d_depth, d_kept, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rgba) HIPCHK(c, hipMemcpy(rgba, d_rgba, px * 16, hipMemcpyDeviceToHost));
    if (depth) HIPCHK(c, hipMemcpy(depth, d_depth, px * 4, hipMemcpyDeviceToHost));
    if (kept) HIPCHK(c, hipMemcpy(kept, d_kept, px, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

// ---- screen-space ambient occlusion (kernels_ssao.hip) ----
int awsm_hip_ssao_defaults(AwsmSsao* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmSsao d = {(uint32_t)sizeof(AwsmSsao), 0.5f, 1.0f, 0.02f, 1.0f};
    *out = d;
    return AWSM_OK;
}
static_assert(sizeof(AwsmSsao) == 4 + sizeof(AwsmHipCtx::SsaoState::p) && offsetof(AwsmSsao, radius) == 4, "SsaoState.p is AwsmSsao behind struct_size");
int awsm_hip_set_ssao(AwsmHipCtx* c, const AwsmSsao* s) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmSsao full;
    awsm_hip_ssao_defaults(&full);
    if (s) {
        int rc = merge_record(c, "set_ssao", "AwsmSsao", s, &full, sizeof full);
        if (!rc) rc = check_finite(c, "set_ssao", &full.radius, 4);
        if (rc) return rc;
        if (!(full.radius > 0.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_ssao: radius = %g (world units, > 0)", (double)full.radius);
        if (!(full.strength >= 0.0f && full.strength <= 1.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_ssao: strength = %g (0 .. 1)", (double)full.strength);
    }
    // host state only: a pass already enqueued carries the record it was enqueued with as kernel arguments
    c->ssao.on = s != nullptr;
    memcpy(c->ssao.p, &full.radius, sizeof c->ssao.p);
    return AWSM_OK;
}
int awsm_hip_read_ssao(AwsmHipCtx* c, float* ao_raw, float* ao_smoothed, float* view_z) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    const size_t px = (size_t)c->width * c->height;
    if (!px || c->ssao_px[c->slot] != px || !c->ssao_layers[c->slot].ptr) return fail(c, AWSM_ERR_NOT_READY, "read_ssao: the last submitted frame had no opaque pass with SSAO on");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    const float* d = (const float*)c->ssao_layers[c->slot].ptr;
    if (ao_raw) HIPCHK(c, hipMemcpy(ao_raw, d, px * 4, hipMemcpyDeviceToHost));
    if (ao_smoothed) HIPCHK(c, hipMemcpy(ao_smoothed, d + px, px * 4, hipMemcpyDeviceToHost));
    if (view_z) HIPCHK(c, hipMemcpy(view_z, d + 2 * px, px * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

// ---- the editor's selection overlay (kernels_selection.hip) ----
int awsm_hip_selection_defaults(AwsmSelection* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmSelection d = {(uint32_t)sizeof(AwsmSelection), AWSM_SELECTION_OUTLINE | AWSM_SELECTION_BOXES, 2u, {1.0f, 0.6f, 0.1f, 1.0f}, {1.0f, 0.6f, 0.1f, 0.9f},
                                    0.75f, 0.25f, 1e-5f};
    *out = d;
    return AWSM_OK;
}
static_assert(sizeof(AwsmSelection) == 56 && sizeof(AwsmSelectionBox) == 24, "AwsmSelection / AwsmSelectionBox layout");
static_assert(selection::kFlagOutline == AWSM_SELECTION_OUTLINE && selection::kFlagBoxes == AWSM_SELECTION_BOXES, "selection.hpp's flags are the header's");
int awsm_hip_set_selection(AwsmHipCtx* c, const AwsmSelection* s, const uint32_t* mesh_keys, uint32_t n_keys, const AwsmSelectionBox* boxes, uint32_t n_boxes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmSelection full;
    awsm_hip_selection_defaults(&full);
    if (s) {
        int rc = merge_record(c, "set_selection", "AwsmSelection", s, &full, sizeof full);
        if (!rc) rc = check_finite(c, "set_selection", full.outline_color, 11);      // two colours and three parameters, contiguous
        if (rc) return rc;
        if (full.flags & ~(AWSM_SELECTION_OUTLINE | AWSM_SELECTION_BOXES)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: unknown flags 0x%x", full.flags);
        if (full.outline_radius < 1u || full.outline_radius > (uint32_t)selection::kMaxRadius) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: outline_radius = %u (1 .. %d pixels)", full.outline_radius, selection::kMaxRadius);
        if (!(full.box_half_width > 0.0f && full.box_half_width <= selection::kMaxHalfWidth)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: box_half_width = %g (pixels, above 0, at most %g)", (double)full.box_half_width, (double)selection::kMaxHalfWidth);
        for (float al : {full.outline_color[3], full.box_color[3], full.hidden_alpha})
            if (!(al >= 0.0f && al <= 1.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: an alpha of %g (0 .. 1)", (double)al);
        if (!(full.depth_epsilon >= 0.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: depth_epsilon = %g (>= 0)", (double)full.depth_epsilon);
        if (n_keys > selection::kMaxKeys || n_boxes > selection::kMaxBoxes) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: %u keys and %u boxes (at most %u and %u)", n_keys, n_boxes, selection::kMaxKeys, selection::kMaxBoxes);
        if ((n_keys && !mesh_keys) || (n_boxes && !boxes)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: a NULL array with a non-zero count");
        for (uint32_t b = 0; b < n_boxes; b++)
            for (int ax = 0; ax < 3; ax++) {
                if (!std::isfinite(boxes[b].min[ax]) || !std::isfinite(boxes[b].max[ax])) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: box %u is not finite", b);
                if (boxes[b].min[ax] > boxes[b].max[ax]) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_selection: box %u has min > max on axis %d", b, ax);
            }
    }
    // host state only: a pass already enqueued carries the record it was enqueued with as kernel arguments
    AwsmHipCtx::SelectionState& st = c->sel;
    st.keys.clear(); st.boxes.clear();
    st.flags = full.flags; st.radius = full.outline_radius;
    memcpy(st.outline_color, full.outline_color, sizeof st.outline_color); memcpy(st.box_color, full.box_color, sizeof st.box_color);
    st.half_width = full.box_half_width; st.hidden_alpha = full.hidden_alpha; st.depth_epsilon = full.depth_epsilon;
    if (s) {
        st.keys.assign(mesh_keys, mesh_keys + 2u * (size_t)n_keys);
        if (n_boxes) st.boxes.assign(boxes[0].min, boxes[0].min + 6u * (size_t)n_boxes);
    }
    // nothing to draw is the same as off: no keys and no boxes, or flags that reach neither
    st.on = s && (((full.flags & AWSM_SELECTION_OUTLINE) && n_keys) || ((full.flags & AWSM_SELECTION_BOXES) && n_boxes));
    return AWSM_OK;
}
int awsm_hip_read_selection(AwsmHipCtx* c, uint8_t* selected, uint8_t* ring, float* box_alpha, float* edges) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    const size_t px = (size_t)c->width * c->height;
    const AwsmHipCtx::SelectionState& st = c->sel_pass[c->slot];
    if (!px || !c->transparent_done || !st.on || !c->sel_tables[c->slot].ptr) return fail(c, AWSM_ERR_NOT_READY, "read_selection: the last submitted frame had no world transparent pass with a selection on");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    int rc = dev_reserve(c, c->sel_layers, px * 6);      // [px] float, [px] byte, [px] byte
    if (rc) return rc;
    if ((rc = sync_scene(c))) return rc;
    SelectionDev sd;
    fill_selection(c, st, &sd);
    sd.layer_box_alpha = (float*)c->sel_layers.ptr; sd.layer_selected = (uint8_t*)(sd.layer_box_alpha + px); sd.layer_ring = sd.layer_selected + px;
    awsm_launch_selection_layers(&sd, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (selected) HIPCHK(c, hipMemcpy(selected, sd.layer_selected, px, hipMemcpyDeviceToHost));
    if (ring) HIPCHK(c, hipMemcpy(ring, sd.layer_ring, px, hipMemcpyDeviceToHost));
    if (box_alpha) HIPCHK(c, hipMemcpy(box_alpha, sd.layer_box_alpha, px * 4, hipMemcpyDeviceToHost));
    if (edges && sd.n_boxes) HIPCHK(c, hipMemcpy(edges, sd.edges, (size_t)sd.n_boxes * selection::kEdgesPerBox * selection::kEdgeFloats * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

// ---- temporal anti-aliasing (kernels_taa.hip) ----
int awsm_hip_taa_defaults(AwsmTaa* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmTaa d = {(uint32_t)sizeof(AwsmTaa), 0.1f, 0u, {0.0f, 0.0f}, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    *out = d;
    return AWSM_OK;
}
int awsm_hip_set_taa(AwsmHipCtx* c, const AwsmTaa* t) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!t) {      // off: the history goes with it
        c->taa.on = false;
        c->taa_have = false; c->taa_serial = 0;
        return AWSM_OK;
    }
    AwsmTaa full;
    awsm_hip_taa_defaults(&full);
    { const int rcm = merge_record(c, "set_taa", "AwsmTaa", t, &full, sizeof full); if (rcm) return rcm; }
    if (!std::isfinite(full.feedback) || !(full.feedback > 0.0f && full.feedback <= 1.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_taa: feedback = %g (0 < feedback <= 1)", (double)full.feedback);
    if (full.flags & ~AWSM_TAA_RESET) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_taa: unknown flags 0x%x", full.flags);
    for (int i = 0; i < 2; i++) if (!std::isfinite(full.jitter_ndc[i])) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_taa: jitter_ndc[%d] is not finite", i);
    for (int i = 0; i < 16; i++) if (!std::isfinite(full.reproject[i])) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "set_taa: reproject[%d] is not finite", i);
    // host state only: a pass already enqueued carries the record it was enqueued with as kernel arguments
    AwsmHipCtx::TaaState& st = c->taa;
    st.on = true;
    st.feedback = full.feedback;
    st.flags |= full.flags;      // a reset asked for stays asked for until a post pass has taken it
    memcpy(st.jitter, full.jitter_ndc, sizeof st.jitter); memcpy(st.reproject, full.reproject, sizeof st.reproject);
    return AWSM_OK;
}
int awsm_hip_read_taa(AwsmHipCtx* c, uint16_t* resolved, float* lookup_xy, uint8_t* used) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    const size_t px = (size_t)c->width * c->height;
    if (!px || !c->taa_resolved || !c->post_done || c->taa_serial != c->frame_serial) return fail(c, AWSM_ERR_NOT_READY, "read_taa: the last post pass did not resolve (awsm_hip_set_taa, then awsm_hip_post_pass)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    if (resolved) HIPCHK(c, hipMemcpy(resolved, c->taa_args.out, px * 8, hipMemcpyDeviceToHost));
    if (lookup_xy || used) {
        // the old history is still what it was and the frame's keys are still in its slot: the layers are computed, not kept
        const int rc = dev_reserve(c, c->taa_layers, px * 9);      // [px][2] float, [px] byte
        if (rc) return rc;
        TaaArgs t = c->taa_args;
        t.layer_xy = (float*)c->taa_layers.ptr; t.layer_used = (uint8_t*)(t.layer_xy + 2 * px);
        t.poison = nullptr;
        awsm_launch_taa_layers(&t, samples_of(c), c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (lookup_xy) HIPCHK(c, hipMemcpy(lookup_xy, t.layer_xy, px * 8, hipMemcpyDeviceToHost));
        if (used) HIPCHK(c, hipMemcpy(used, t.layer_used, px, hipMemcpyDeviceToHost));
    }
    return AWSM_OK;
}

// EffectsRenderPass::render + DisplayRenderPass::render (render.rs:339-356); the kernels and the contract: kernels_post.hip, DESIGN.md §11
int awsm_hip_post_pass(AwsmHipCtx* c, const AwsmPostParams* p) {
    if (!c || !p) return AWSM_ERR_INVALID_ARGUMENT;
    if (p->struct_size != sizeof(AwsmPostParams)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "post_pass: struct_size %u, this library's AwsmPostParams is %zu bytes", p->struct_size, sizeof(AwsmPostParams));
    if (p->tonemapping > 2u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "post_pass: tonemapping %u (0 None, 1 KhronosNeutralPbr, 2 Aces)", p->tonemapping);
    if (p->flags & ~(AWSM_POST_SMAA | AWSM_POST_BLOOM | AWSM_POST_DOF)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "post_pass: unknown flags 0x%x", p->flags);
    if (is_sharded(c)) return fail(c, AWSM_ERR_UNSUPPORTED, "post_pass on a sharded context: the SMAA / bloom / DoF stencils read neighbouring rows (no halo exchange)");
    if (c->width == 0 || !c->geometry_done || !c->opaque_done) return fail(c, AWSM_ERR_NOT_READY, "post_pass needs the frame's opaque pass first");
    // temporal anti-aliasing (awsm_hip_set_taa): this pass carries the record as it stands now, into a replay too
    if (c->taa.on && (c->taa.flags & AWSM_TAA_RESET)) { c->taa_have = false; c->taa_serial = 0; c->taa.flags &= ~AWSM_TAA_RESET; }      // one pass, then cleared
    c->taa_pass = c->taa;
    if (!c->taa.on) c->taa_resolved = false;
    return enqueue_post(c, *p);
}

// the post pass of the current frame with the context's images as they are bound now; awsm_hip_frame_end enqueues it again after a replay
static int enqueue_post(AwsmHipCtx* c, const AwsmPostParams& pp) {
    const AwsmPostParams* p = &pp;
    const size_t px = (size_t)c->width * c->height;
    if (c->bound_display && c->bound_display_bytes < px * 4) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "post_pass: bound display image holds %zu bytes, the frame needs %zu", c->bound_display_bytes, px * 4);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = AWSM_OK;
    if (!c->bound_display && (rc = dev_reserve(c, c->display8[c->slot], px * 4))) return rc;
    const bool bloom = p->flags & AWSM_POST_BLOOM, dof = p->flags & AWSM_POST_DOF, tap = c->flags & AWSM_CFG_PARITY_TAP;
    if (tap && (rc = dev_reserve(c, c->effects16, px * 8))) return rc;
    if (bloom && ((rc = dev_reserve(c, c->bloom_a, px * 8)) || (rc = dev_reserve(c, c->bloom_b, px * 8)))) return rc;
    if (dof && ((rc = dev_reserve(c, c->dof_lc, px * 8)) || (rc = dev_reserve(c, c->dof_blur, px * 16)))) return rc;
    PostArgs a{};
    a.width = c->width; a.height = c->height;
    if (c->transparent_done) a.src = (const uint2*)(c->bound_comp ? c->bound_comp : c->comp16.ptr);
    else a.src = (const uint2*)(c->bound_out ? (const uint8_t*)c->bound_out - (size_t)c->out_first_row * c->width * 8 : (const uint8_t*)c->out16[c->slot].ptr);
    a.vis = (const unsigned long long*)FB(c).vis.ptr;       // the world's keys (not the merged hud ones): hud_depth plays no part
    const FrameBufs& t = pass_bufs(c, kPassTransparent);
    if (dof && c->transparent_done && c->lists[kPassTransparent].total_tris && t.frag_first.ptr) {
        a.frag_first = (const uint32_t*)t.frag_first.ptr; a.frag_rec = (const uint4*)t.frag_rec.ptr; a.frag_cap = t.frag_cap; a.tri_rec = (const TriRec*)t.tri_rec.ptr;
    }
    a.camera = (const float*)FB(c).camera.ptr;
    a.dof_lc = (float2*)c->dof_lc.ptr; a.dof_blur = (float4*)c->dof_blur.ptr;
    a.effects = tap ? (uint2*)c->effects16.ptr : nullptr;
    a.display = (uint32_t*)(c->bound_display ? c->bound_display : c->display8[c->slot].ptr);
    a.tonemap = p->tonemapping; a.dof = dof ? 1u : 0u;
    a.poison = c->handoff_poison ? c->handoff_poison + c->slot : nullptr; a.frame_serial = c->frame_serial;   // a frame a hand-off gate dropped is not post-processed
    if (!a.src || !a.vis || !a.camera) return fail(c, AWSM_ERR_NOT_READY, "post_pass: the frame's images are missing");
    hipStream_t ss = shade_stream_of(c);          // in order after the opaque / transparent passes of the frame
    // the bloom / DoF scratch and the effects image are per context: behind the other slot's passes (its post pass among them)
    if (c->overlap && c->shade_recorded[prev_slot(c)]) HIPCHK(c, wait_prev_slot(c, ss));
    if (c->taa_pass.on) {
        // the resolve first, behind the other slot's passes — its post pass wrote the history this one reads, and read the image this one
        // overwrites — and the resolved image is what everything below takes as src
        if ((rc = dev_reserve(c, c->taa_img[0], px * 8)) || (rc = dev_reserve(c, c->taa_img[1], px * 8))) return rc;
        if (c->taa_serial != c->frame_serial) {      // once per frame serial: a replay reads the same history and rewrites the same image
            c->taa_frame_hist = c->taa_have;
            c->taa_cur ^= 1;
            c->taa_serial = c->frame_serial;
        }
        const AwsmHipCtx::TaaState& ts = c->taa_pass;
        TaaArgs t{};
        t.width = c->width; t.height = c->height;
        t.cur = a.src; t.vis = a.vis;
        t.history = c->taa_frame_hist ? (const uint2*)c->taa_img[c->taa_cur ^ 1].ptr : nullptr;
        t.out = (uint2*)c->taa_img[c->taa_cur].ptr;
        memcpy(t.reproject, ts.reproject, sizeof t.reproject); t.jitter[0] = ts.jitter[0]; t.jitter[1] = ts.jitter[1]; t.feedback = ts.feedback;
        t.poison = a.poison; t.frame_serial = a.frame_serial;
        awsm_launch_taa(&t, samples_of(c), ss);
        a.src = t.out;
        c->taa_args = t; c->taa_have = true; c->taa_resolved = true;
    }
    awsm_launch_post(&a, p->flags, samples_of(c), c->bloom_a.ptr, c->bloom_b.ptr, ss);
    HIPCHK(c, hipGetLastError());
    if (c->overlap) HIPCHK(c, mark_shade_done(c, ss));       // the slot's next geometry pass waits for this too
    c->last_display = a.display;
    c->post_params = pp;
    c->post_done = true;
    return AWSM_OK;
}

int awsm_hip_read_display(AwsmHipCtx* c, uint8_t* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->last_display) return fail(c, AWSM_ERR_NOT_READY, "read_display before post_pass");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, c->last_display, (size_t)c->width * c->height * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_read_effects(AwsmHipCtx* c, uint16_t* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!(c->flags & AWSM_CFG_PARITY_TAP) || !c->effects16.ptr || !c->last_display) return fail(c, AWSM_ERR_NOT_READY, "read_effects needs AWSM_CFG_PARITY_TAP and a post_pass");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    HIPCHK(c, hipMemcpy(out, c->effects16.ptr, (size_t)c->width * c->height * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_bind_display(AwsmHipCtx* c, void* device_ptr, size_t bytes) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (device_ptr && bytes == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "bind_display: zero-sized image");
    c->bound_display = device_ptr; c->bound_display_bytes = bytes;
    return AWSM_OK;
}

void* awsm_hip_display_device_ptr(AwsmHipCtx* c) { return c ? c->last_display : nullptr; }

// the first n transformed vertices of a pass: clip positions, world N and T interleaved, world positions (the transparent passes keep them)
static int read_pass_vertices(AwsmHipCtx* c, const FrameBufs& b, uint32_t n, float* clip_out, float* nt_out, float* wpos_out) {
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    if (n == 0) return AWSM_OK;
    if (clip_out) HIPCHK(c, hipMemcpy(clip_out, b.clip.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (wpos_out) HIPCHK(c, hipMemcpy(wpos_out, b.wpos.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (nt_out) {
        std::vector<float> nn((size_t)n * 4), tt((size_t)n * 4);
        HIPCHK(c, hipMemcpy(nn.data(), b.nrm.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(tt.data(), b.tan.ptr, (size_t)n * 16, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; i++) { memcpy(nt_out + i * 8, &nn[i * 4], 16); memcpy(nt_out + i * 8 + 4, &tt[i * 4], 16); }
    }
    return AWSM_OK;
}

int awsm_hip_read_transformed_forward(AwsmHipCtx* c, float* clip_out, float* nt_out, float* wpos_out, uint32_t max_vertices) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->transparent_done) return fail(c, AWSM_ERR_NOT_READY, "read_transformed_forward before transparent_pass");
    return read_pass_vertices(c, pass_bufs(c, kPassTransparent), std::min(max_vertices, 3u * c->lists[kPassTransparent].total_tris), clip_out, nt_out, wpos_out);
}

int awsm_hip_read_transformed(AwsmHipCtx* c, float* clip_out, float* nt_out, uint32_t max_vertices) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "read_transformed before geometry_pass");
    if (clip_out) { HIPCHK(c, hipSetDevice(c->device)); const int rc = materialize_clip(c); if (rc) return rc; }      // (read_pass_vertices drains every stream before it copies)
    return read_pass_vertices(c, FB(c), std::min(max_vertices, 3u * c->lists[kPassWorld].total_tris), clip_out, nt_out, nullptr);
}

}  // extern "C"
