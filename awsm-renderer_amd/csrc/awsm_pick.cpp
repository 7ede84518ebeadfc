// awsm_pick.cpp — the queries of include/awsm_hip.h that pick through the transparent passes' fragment lists: awsm_hip_pick_ex, awsm_hip_pick_rect,
// awsm_hip_read_pick_map (kernels_pick.hip).  They read what the last submitted frame's passes left in the context's current frame
// slot and enqueue nothing a frame needs: the frame pipeline (awsm_hip.cpp) does not know them, and a frame that never picks launches what it
// launched before.  They reach the context through ctx.hpp, as awsm_resources.cpp does.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "launch.hpp"
#include "pick.hpp"

using namespace awsm;

static_assert(sizeof(AwsmPickQuery) == 12 && sizeof(AwsmPickHit) == 28 && sizeof(AwsmPickRectEntry) == 4 * pick::kEntryWords, "AwsmPickQuery / AwsmPickHit / AwsmPickRectEntry layout");
static_assert(pick::kFlagTransparent == AWSM_PICK_TRANSPARENT, "pick.hpp's flag is the header's");

extern "C" {

namespace {

bool sharded(const AwsmHipCtx* c) { return c->band_n > 1 || (c->y1 != 0 && !(c->y0 == 0 && c->y1 >= c->height)); }

// query (NULL: the defaults) -> the checked record
static int check_query(AwsmHipCtx* c, const char* entry, const AwsmPickQuery* query, AwsmPickQuery* full) {
    awsm_hip_pick_query_defaults(full);
    if (!query) return AWSM_OK;
    const uint32_t given = query->struct_size;
    if (given < 4u || given > 4096u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: AwsmPickQuery.struct_size = %u (set it to sizeof(AwsmPickQuery))", entry, given);
    memcpy((uint8_t*)full + 4, (const uint8_t*)query + 4, (std::min<size_t>(given, sizeof *full) & ~(size_t)3) - 4);      // whole fields only; the rest keeps its defaults
    if (full->flags & ~AWSM_PICK_TRANSPARENT) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", entry, full->flags);
    if (!(full->alpha_threshold >= 0.0f && full->alpha_threshold <= 1.0f)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: alpha_threshold = %g (0 .. 1)", entry, (double)full->alpha_threshold);
    return AWSM_OK;
}

// What every query checks and waits for, then the kernels' arguments for the current slot's frame.  rect: the query merges over the frame.
static int prepare(AwsmHipCtx* c, const char* entry, const AwsmPickQuery& q, bool rect, PickDev* a) {
    if (!c->geometry_done) return fail(c, AWSM_ERR_NOT_READY, "%s before geometry_pass", entry);
    if (!c->bufs[AWSM_BUF_MATERIAL_META].ptr || !c->bufs[AWSM_BUF_GEOM_META].ptr) return fail(c, AWSM_ERR_NOT_READY, "%s: meta buffers missing", entry);
    const bool lists = (q.flags & AWSM_PICK_TRANSPARENT) != 0u;
    if (sharded(c) && (lists || rect))
        return fail(c, AWSM_ERR_UNSUPPORTED, "%s on a sharded context: %s", entry, rect ? "a rectangle's answer would need merging across ranks" : "AWSM_PICK_TRANSPARENT reads fragment lists of rows the shard never drew");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcs = sync_all(c); if (rcs) return rcs; }
    const int s = c->slot;
    const FrameBufs &world = c->fb[s], &tr = c->tr[s], &hud = c->hud[s], &htr = c->htr[s];
    const bool use_tr = lists && c->transparent_done, use_htr = lists && c->hud_transparent_done;
    // a list that overflowed holds a part of the frame's fragments until awsm_hip_frame_end has grown it and replayed the pass
    for (int k = 0; k < 2; k++) {
        const FrameBufs& b = k ? htr : tr;
        if (!(k ? use_htr : use_tr) || !b.counters.ptr) continue;
        uint32_t ctr[kCtrWords] = {};
        HIPCHK(c, hipMemcpy(ctr, b.counters.ptr, sizeof ctr, hipMemcpyDeviceToHost));
        if (ctr[kCtrOverflow] || ctr[kCtrFragOverflow])
            return fail(c, AWSM_ERR_NOT_READY, "%s: the %stransparent pass overflowed its %s list and has not been replayed: call awsm_hip_frame_end first", entry, k ? "HUD " : "",
                        ctr[kCtrFragOverflow] ? "fragment" : "bin");
    }
    memset(a, 0, sizeof *a);
    a->width = c->width; a->height = c->height; a->samples = c->msaa == 4 ? 4u : 1u;
    uint32_t y0 = c->y0, y1 = c->y1;      // the shard's rows, as the frame's kernels have them
    if (y1 == 0 || y1 > c->height) y1 = c->height;
    if (y0 > y1) y0 = y1;
    a->sy0 = y0; a->sy1 = y1; a->band_n = std::max(c->band_n, 1u); a->band_r = c->band_r;
    a->flags = q.flags; a->alpha_threshold = q.alpha_threshold;
    a->geom_meta = (const uint8_t*)c->bufs[AWSM_BUF_GEOM_META].ptr; a->material_meta = (const uint8_t*)c->bufs[AWSM_BUF_MATERIAL_META].ptr;
    a->geom_meta_bytes = (uint32_t)std::min<size_t>(c->bufs[AWSM_BUF_GEOM_META].size, 0xFFFFFFFFu);
    a->material_meta_bytes = (uint32_t)std::min<size_t>(c->bufs[AWSM_BUF_MATERIAL_META].size, 0xFFFFFFFFu);
    a->vis = (const unsigned long long*)world.vis.ptr;
    a->hud_vis = c->hud_geometry_done ? (const unsigned long long*)hud.vis.ptr : nullptr;
    const PassList& wl = c->lists[kPassWorld];
    const PassList& hl = c->lists[kPassHud];
    auto layer = [](PickLayerDev& l, const FrameBufs& b, uint32_t n_draws, uint32_t total_tris, uint32_t base) {
        l.draws = (const DrawDev*)b.draws_dev.ptr; l.tri_info = (const uint32_t*)b.tri_flags.ptr;
        l.n_draws = l.draws && l.tri_info ? n_draws : 0u; l.total_tris = l.n_draws ? total_tris : 0u; l.draw_base = l.n_draws ? base : 0u;
    };
    layer(a->layer[pick::kLayerWorld], world, (uint32_t)wl.draws.size(), wl.total_tris, 0u);
    if (!c->hud_geometry_done) layer(a->layer[pick::kLayerHud], hud, 0u, 0u, 0u);
    else if (c->hud_merged)      // one rank space: the hud draws follow the world's in the world pass's list, and the hud keys name global ranks
        layer(a->layer[pick::kLayerHud], world, (uint32_t)c->hud_combined.size(), wl.total_tris + hl.total_tris, (uint32_t)wl.draws.size());
    else layer(a->layer[pick::kLayerHud], hud, (uint32_t)hl.draws.size(), hl.total_tris, 0u);
    for (int k = 0; k < 2; k++) {
        const FrameBufs& b = k ? htr : tr;
        const PassList& l = c->lists[k ? kPassHudTransparent : kPassTransparent];
        const bool use = (k ? use_htr : use_tr) && l.total_tris && b.frag_first.ptr && b.frag_rec.ptr && b.frag_color.ptr && b.tri_rec.ptr && b.frag_first.size >= (size_t)c->width * c->height * 4;
        layer(a->layer[k ? pick::kLayerHudTransparent : pick::kLayerWorldTransparent], b, use ? (uint32_t)l.draws.size() : 0u, l.total_tris, 0u);
        if (!use || !a->layer[k ? pick::kLayerHudTransparent : pick::kLayerWorldTransparent].n_draws) continue;
        PickFragsDev& f = a->frags[k];
        f.first = (const uint32_t*)b.frag_first.ptr; f.rec = (const uint4*)b.frag_rec.ptr; f.color = (const float4*)b.frag_color.ptr;
        f.tri_rec = (const TriRec*)b.tri_rec.ptr; f.cap = b.frag_cap;
    }
    uint32_t n = 0;
    for (uint32_t L = 0; L < pick::kLayers; L++) { a->layer[L].counter_base = n; n += a->layer[L].n_draws - a->layer[L].draw_base; }
    a->n_counters = n;
    if (!a->vis && c->width && c->height) return fail(c, AWSM_ERR_NOT_READY, "%s before resize", entry);
    return AWSM_OK;
}

}  // namespace

int awsm_hip_pick_query_defaults(AwsmPickQuery* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    static const AwsmPickQuery d = {(uint32_t)sizeof(AwsmPickQuery), 0u, 0.5f};
    *out = d;
    return AWSM_OK;
}

int awsm_hip_pick_ex(AwsmHipCtx* c, int32_t x, int32_t y, const AwsmPickQuery* query, AwsmPickHit* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmPickQuery q;
    int rc = check_query(c, "pick_ex", query, &q);
    if (rc) return rc;
    PickDev a;
    if ((rc = prepare(c, "pick_ex", q, false, &a))) return rc;
    if ((rc = dev_reserve(c, c->pick_scratch, pick::kPointWords * 4))) return rc;
    a.x0 = x; a.y0 = y;
    a.point_out = (uint32_t*)c->pick_scratch.ptr;
    awsm_launch_pick_point(&a, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t w[pick::kPointWords] = {};
    HIPCHK(c, hipMemcpyAsync(w, a.point_out, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->valid = w[0]; out->mesh_key_high = w[1]; out->mesh_key_low = w[2]; out->triangle_index = w[3]; out->layer = w[4];
    memcpy(&out->alpha, &w[5], 4); out->depth_bits = w[6];
    return AWSM_OK;
}

int awsm_hip_pick_rect(AwsmHipCtx* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, const AwsmPickQuery* query, AwsmPickRectEntry* out, uint32_t cap, uint32_t* n_out) {
    if (!c || !n_out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!out && cap) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "pick_rect: out == NULL with cap = %u", cap);
    AwsmPickQuery q;
    int rc = check_query(c, "pick_rect", query, &q);
    if (rc) return rc;
    PickDev a;
    if ((rc = prepare(c, "pick_rect", q, true, &a))) return rc;
    a.x0 = std::max(x0, 0); a.y0 = std::max(y0, 0); a.x1 = std::min<int64_t>(x1, c->width); a.y1 = std::min<int64_t>(y1, c->height);
    const uint32_t n = a.n_counters;
    a.cap = std::min(cap, n);      // there are no more distinct pairs than draws
    // [n_out + 7 words of padding][counters n][key words 2 n][merged n][entries cap x 4]
    const size_t words = 8 + (size_t)n * 4 + (size_t)a.cap * pick::kEntryWords;
    if ((rc = dev_reserve(c, c->pick_scratch, words * 4))) return rc;
    uint32_t* base = (uint32_t*)c->pick_scratch.ptr;
    a.n_out = base; a.counters = base + 8; a.draw_keys = a.counters + n; a.merged = a.draw_keys + 2 * (size_t)n; a.entries = a.merged + n;
    HIPCHK(c, hipMemsetAsync(base, 0, (8 + (size_t)n) * 4, c->stream));
    awsm_launch_pick_rect(&a, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t found = 0;
    HIPCHK(c, hipMemcpyAsync(&found, a.n_out, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t written = std::min(found, a.cap);
    if (written) HIPCHK(c, hipMemcpy(out, a.entries, (size_t)written * sizeof(AwsmPickRectEntry), hipMemcpyDeviceToHost));
    *n_out = found;
    return AWSM_OK;
}

int awsm_hip_read_pick_map(AwsmHipCtx* c, const AwsmPickQuery* query, uint32_t* word, uint32_t* triangle) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmPickQuery q;
    int rc = check_query(c, "read_pick_map", query, &q);
    if (rc) return rc;
    PickDev a;
    if ((rc = prepare(c, "read_pick_map", q, false, &a))) return rc;
    const size_t px = (size_t)c->width * c->height;
    if (!px) return AWSM_OK;
    if ((rc = dev_reserve(c, c->pick_scratch, px * 8))) return rc;
    a.map_word = (uint32_t*)c->pick_scratch.ptr; a.map_triangle = a.map_word + px;
    awsm_launch_pick_map(&a, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (word) HIPCHK(c, hipMemcpy(word, a.map_word, px * 4, hipMemcpyDeviceToHost));
    if (triangle) HIPCHK(c, hipMemcpy(triangle, a.map_triangle, px * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

}  // extern "C"
