// kernels_pick.hip — point and rectangle queries over the last frame that see transparent meshes (gfx950).
//
// k_pick (kernels_shade.hip) reads the visibility keys only, and a transparent mesh has no key.  After a transparent pass every pixel has a fragment
// list (FrameDev::frag_first -> frag_rec, in submission order), frag_color[i].w is the alpha the fragment was blended with, and the pass's own draw
// list leads to the mesh key as k_pick reaches it.  The pipeline tests LessEqual and writes depth, so per sample a pixel's listed fragments are a
// chain of non-increasing depth: a later fragment is nearer.  The rule, over sample 0 only (rec.w & 1, the picker's textureLoad(.., 0)) — the first
// of these that exists:
//   1. the LAST fragment of the HUD transparent pass's list with alpha >= threshold      (layer 3)
//   2. the HUD geometry key                                                              (layer 2)
//   3. the LAST fragment of the world transparent pass's list with alpha >= threshold    (layer 1)
//   4. the world visibility key                                                          (layer 0)
// With AWSM_PICK_TRANSPARENT clear steps 1 and 3 are left out and the answer is k_pick's, word for word.
//
//   k_pick_point    one thread: the rule at one pixel, with the fragment's alpha and its depth bits (tri_sample_key_at / tri_msaa_sample_key on the
//                   pass's set-up record, as k_post_dof_depth derives it).
//   k_pick_map      one thread per pixel of the frame: layer << 28 | draw index in its pass's list (all ones: miss) and the triangle index.
//   k_pick_rect     16 x 16 pixels of the clamped rectangle per workgroup, one pixel per lane; each wavefront reduces its 64 answers to distinct
//                   values with a ballot / readfirstlane loop and issues one atomicAdd per distinct value into the per-draw counters.
//   k_pick_collect  one workgroup: the counters -> the entry list, ordered by layer and draw, draws that share a mesh key merged into the first.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "frame_params.hpp"
#include "raster_setup.hpp"
#include "pick.hpp"
#include "launch.hpp"

namespace awsm {
namespace pick {

constexpr uint32_t kFragNone = 0xFFFFFFFFu;

struct Answer {
    uint32_t word;        // layer << 28 | draw index relative to the pass's own draws; kMiss: nothing
    uint32_t triangle;    // primitive-local
    uint32_t rank;        // the triangle's rank in its pass
    uint32_t frag;        // layers 1 and 3: the fragment's index in its pass's lists
    uint32_t key_hi;      // layers 0 and 2: the key's depth word
};

// the draw a rank of layer L belongs to -> the answer's word and triangle; false where the tables do not hold the rank
__device__ __forceinline__ bool answer_of(const PickDev& a, uint32_t L, uint32_t rank, Answer& out) {
    const PickLayerDev& l = a.layer[L];
    if (rank >= l.total_tris) return false;
    const uint32_t draw = l.tri_info[rank] & 0x00FFFFFFu;
    if (draw >= l.n_draws || draw < l.draw_base) return false;
    out.word = (L << kLayerShift) | ((draw - l.draw_base) & kDrawMask);
    out.triangle = rank - l.draws[draw].first_tri;
    out.rank = rank;
    return true;
}

// the last sample-0 fragment of the pixel's list with alpha >= threshold
__device__ __forceinline__ bool last_fragment(const PickDev& a, const PickFragsDev& fr, size_t p, uint32_t& frag, uint32_t& rank) {
    bool found = false;
    uint32_t i = fr.first[p];
    for (uint32_t guard = 0; i != kFragNone && i < fr.cap && guard < fr.cap; guard++) {
        const uint4 rec = fr.rec[i];
        if ((rec.w & 1u) && rec.x != kFragNone && fr.color[i].w >= a.alpha_threshold) { found = true; frag = i; rank = rec.x; }
        i = rec.z;
    }
    return found;
}

// The rule at pixel (x, y).  Shared by every kernel of this file.
__device__ __forceinline__ Answer pick_pixel(const PickDev& a, int x, int y) {
    Answer out{kMiss, 0xFFFFFFFFu, 0u, kFragNone, 0u};
    if (x < 0 || y < 0 || x >= (int)a.width || y >= (int)a.height || y < (int)a.sy0 || y >= (int)a.sy1) return out;
    if (a.band_n > 1u && (((uint32_t)y >> kTileShift) % a.band_n) != a.band_r) return out;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const bool lists = (a.flags & kFlagTransparent) != 0u;
    uint32_t frag, rank;
    if (lists && a.frags[1].first && last_fragment(a, a.frags[1], p, frag, rank)) {
        if (answer_of(a, kLayerHudTransparent, rank, out)) { out.frag = frag; return out; }
    }
    if (a.hud_vis) {
        const unsigned long long hk = a.hud_vis[p * a.samples];
        if (hk != ~0ull) {      // the HUD geometry pass drew over the visibility target: its triangle hides the world's, as k_pick has it
            if (answer_of(a, kLayerHud, 0xFFFFFFFFu - (uint32_t)(hk & 0xFFFFFFFFull), out)) out.key_hi = (uint32_t)(hk >> 32);
            return out;
        }
    }
    if (lists && a.frags[0].first && last_fragment(a, a.frags[0], p, frag, rank)) {
        if (answer_of(a, kLayerWorldTransparent, rank, out)) { out.frag = frag; return out; }
    }
    const unsigned long long key = a.vis[p * a.samples];
    if (key == ~0ull) return out;
    if (answer_of(a, kLayerWorld, 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull), out)) out.key_hi = (uint32_t)(key >> 32);
    return out;
}

// geometry meta + 36 -> material mesh meta words 0 and 1, bounds-checked
__device__ __forceinline__ bool mesh_key_of(const PickDev& a, const DrawDev& dr, uint32_t& hi, uint32_t& lo) {
    if ((size_t)dr.geom_meta_off + 40u > (size_t)a.geom_meta_bytes) return false;
    const uint32_t material_meta_offset = *reinterpret_cast<const uint32_t*>(a.geom_meta + dr.geom_meta_off + 36);
    const size_t mm_off = (size_t)(material_meta_offset / 256u) * 256u;
    if (mm_off + 8u > (size_t)a.material_meta_bytes) return false;
    const uint32_t* mm = reinterpret_cast<const uint32_t*>(a.material_meta + mm_off);
    hi = mm[0]; lo = mm[1];
    return true;
}

// out = {valid, mesh_key_high, mesh_key_low, triangle_index, layer, alpha bits, depth bits, map word}
__global__ void k_pick_point(PickDev a) {
    uint32_t* out = a.point_out;
    out[0] = 0u; out[1] = 0u; out[2] = 0u; out[3] = 0xFFFFFFFFu; out[4] = 0u; out[5] = 0u; out[6] = 0u; out[7] = kMiss;
    const int x = a.x0, y = a.y0;
    const Answer ans = pick_pixel(a, x, y);
    if (ans.word == kMiss) return;
    const uint32_t L = ans.word >> kLayerShift;
    const PickLayerDev& l = a.layer[L];
    uint32_t hi, lo;
    if (!mesh_key_of(a, l.draws[l.draw_base + (ans.word & kDrawMask)], hi, lo)) return;
    uint32_t alpha = 0x3F800000u, depth = ans.key_hi;
    if (L == kLayerWorldTransparent || L == kLayerHudTransparent) {
        const PickFragsDev& fr = a.frags[L == kLayerHudTransparent ? 1 : 0];
        alpha = __float_as_uint(fr.color[ans.frag].w);
        depth = 0x3F800000u;
        TriSetup t;
        if (tri_rec_load(fr.tri_rec + ans.rank, t)) {
            unsigned long long k;
            if (a.samples == 1u) k = tri_sample_key_at(t, sample_coord((x << 8) + 128), sample_coord((y << 8) + 128), ans.rank);
            else {
                float dz[4];
                const float zc = tri_plane_depth(t, tri_edges_d(t, (double)x, (double)y)) + 0.0f;
                msaa_depth_steps(t.a, t.b, t.zq, dz);
                k = tri_msaa_sample_key(t, x, y, 0, zc, dz, ans.rank);
            }
            if (k != ~0ull) depth = (uint32_t)(k >> 32);
        }
    }
    out[0] = 1u; out[1] = hi; out[2] = lo; out[3] = ans.triangle; out[4] = L; out[5] = alpha; out[6] = depth; out[7] = ans.word;
}

__global__ __launch_bounds__(256) void k_pick_map(PickDev a) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= a.width * a.height) return;
    const Answer ans = pick_pixel(a, (int)(p % a.width), (int)(p / a.width));
    a.map_word[p] = ans.word;
    a.map_triangle[p] = ans.word == kMiss ? 0xFFFFFFFFu : ans.triangle;
}

// the counter of a map word; n_counters where it has none
__device__ __forceinline__ uint32_t counter_of(const PickDev& a, uint32_t word) {
    const PickLayerDev& l = a.layer[word >> kLayerShift];
    const uint32_t d = word & kDrawMask;
    return d < l.n_draws - l.draw_base ? l.counter_base + d : a.n_counters;
}

__global__ __launch_bounds__(256) void k_pick_rect(PickDev a) {
    const int x = a.x0 + (int)blockIdx.x * kTile + (int)(threadIdx.x & 15u), y = a.y0 + (int)blockIdx.y * kTile + (int)(threadIdx.x >> 4);
    uint32_t word = kMiss;
    if (x < a.x1 && y < a.y1) word = pick_pixel(a, x, y).word;
    // the wavefront's 64 answers -> one atomicAdd per distinct value: the first pending lane's value, the lanes that share it, their count
    bool pending = word != kMiss;
    while (__builtin_amdgcn_ballot_w64(pending) != 0ull) {
        if (pending) {
            const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
            const bool mine = word == v;
            const unsigned long long same = __builtin_amdgcn_ballot_w64(mine);
            if (mine) {
                const uint32_t lane = threadIdx.x & 63u;
                const uint32_t c = counter_of(a, v);
                if (lane == (uint32_t)__builtin_ctzll(same) && c < a.n_counters) atomicAdd(a.counters + c, (uint32_t)__builtin_popcountll(same));
                pending = false;
            }
        }
    }
}

// the layer whose counters hold word e
__device__ __forceinline__ uint32_t layer_of_counter(const PickDev& a, uint32_t e) {
    uint32_t L = 0u;
#pragma unroll
    for (uint32_t k = 1; k < kLayers; k++) if (e >= a.layer[k].counter_base) L = k;
    return L;
}

__global__ __launch_bounds__(kCollectThreads) void k_pick_collect(PickDev a) {
    __shared__ uint32_t wave_sum[kCollectThreads / 64], base;
    const uint32_t tid = threadIdx.x, n = a.n_counters;
    // every draw's key words; a draw whose meta offsets lead nowhere has all ones (no pixel names it)
    for (uint32_t e = tid; e < n; e += kCollectThreads) {
        const PickLayerDev& l = a.layer[layer_of_counter(a, e)];
        uint32_t hi = 0xFFFFFFFFu, lo = 0xFFFFFFFFu;
        mesh_key_of(a, l.draws[l.draw_base + (e - l.counter_base)], hi, lo);
        a.draw_keys[2u * e] = hi; a.draw_keys[2u * e + 1u] = lo;
        a.merged[e] = 0u;
    }
    if (tid == 0) base = 0u;
    __syncthreads();
    // a draw's pixels go to the first draw of its pass with the same key
    for (uint32_t e = tid; e < n; e += kCollectThreads) {
        const uint32_t c = a.counters[e];
        if (!c) continue;
        const uint32_t hi = a.draw_keys[2u * e], lo = a.draw_keys[2u * e + 1u];
        uint32_t first = a.layer[layer_of_counter(a, e)].counter_base;
        while (first < e && !(a.draw_keys[2u * first] == hi && a.draw_keys[2u * first + 1u] == lo)) first++;
        atomicAdd(a.merged + first, c);
    }
    __syncthreads();
    // the entries in counter order = by layer, then by draw: an exclusive scan of "holds pixels" over chunks of 256
    for (uint32_t e0 = 0; e0 < n; e0 += kCollectThreads) {
        const uint32_t e = e0 + tid;
        const uint32_t c = e < n ? a.merged[e] : 0u;
        const unsigned long long wave = __builtin_amdgcn_ballot_w64(c != 0u);
        const uint32_t lane = tid & 63u, w = tid >> 6;
        if (lane == 0u) wave_sum[w] = (uint32_t)__builtin_popcountll(wave);
        __syncthreads();
        uint32_t pos = base + (uint32_t)__builtin_popcountll(wave & ((1ull << lane) - 1ull));
        for (uint32_t k = 0; k < w; k++) pos += wave_sum[k];
        if (c != 0u && pos < a.cap) {
            uint32_t* o = a.entries + (size_t)pos * kEntryWords;
            o[0] = layer_of_counter(a, e); o[1] = a.draw_keys[2u * e]; o[2] = a.draw_keys[2u * e + 1u]; o[3] = c;
        }
        __syncthreads();
        if (tid == 0) { uint32_t s = 0u; for (uint32_t k = 0; k < kCollectThreads / 64; k++) s += wave_sum[k]; base += s; }
        __syncthreads();
    }
    if (tid == 0) *a.n_out = base;
}

}  // namespace pick
}  // namespace awsm

using awsm::PickDev;

extern "C" void awsm_launch_pick_point(const PickDev* args, hipStream_t s) { awsm::pick::k_pick_point<<<dim3(1), dim3(1), 0, s>>>(*args); }

extern "C" void awsm_launch_pick_map(const PickDev* args, hipStream_t s) {
    const uint32_t n = args->width * args->height;
    if (n) awsm::pick::k_pick_map<<<dim3((n + 255u) / 256u), dim3(256), 0, s>>>(*args);
}

// the rectangle's counters (zeroed by the caller in front of this), then the entry list; an empty rectangle launches the collection alone
extern "C" void awsm_launch_pick_rect(const PickDev* args, hipStream_t s) {
    const PickDev& a = *args;
    if (a.x1 > a.x0 && a.y1 > a.y0) {
        const dim3 grid((uint32_t)(a.x1 - a.x0 + awsm::pick::kTile - 1) / awsm::pick::kTile, (uint32_t)(a.y1 - a.y0 + awsm::pick::kTile - 1) / awsm::pick::kTile);
        awsm::pick::k_pick_rect<<<grid, dim3(256), 0, s>>>(a);
    }
    awsm::pick::k_pick_collect<<<dim3(1), dim3(awsm::pick::kCollectThreads), 0, s>>>(a);
}
