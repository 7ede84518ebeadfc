// kernels_selection.hip — the editor's selection overlay: an outline around the visible pixels of the selected meshes and a wire box around every
// selected mesh's world AABB, blended into the composite as the last step of the world transparent pass (gfx950).
//
// The contract these kernels follow, and tests/selection_reference.py with them operation for operation: f32 throughout with nothing fused
// (-ffp-contract=off, Makefile), only + - * / and sqrt in their IEEE forms, sums left to right, matrix rows spelled
// ((m[r] X + m[4+r] Y) + m[8+r] Z) + m[12+r].  The device is held to the restatement's exact bits.
//
//   k_selection_mark        one thread per world DrawDev: its mesh key words (geometry meta + 36 -> material mesh meta words 0 and 1, as k_pick
//                           reaches them) against the <= 64 listed keys, into a byte per draw.
//   k_selection_edges       one thread per (box, edge), <= 768: the edge's corners through the camera snapshot's view_proj, clipped against the near
//                           plane, to screen coordinates and NDC depth; a 32-byte record per edge.
//   k_selection_overlay<S>  per 16x16 tile: `selected` of the tile and a 4-pixel apron staged in LDS (24 x 24 bytes), the frame's edges culled
//                           cooperatively against the tile into an LDS index list (sized for all 768: no overflow path), then per pixel the ring from
//                           LDS and the box alpha over the listed edges (each record read wave-uniformly), blended into the RGBA16F composite
//                           (and its f32 tap).  A tile with nothing selected in its window and an empty list touches no image byte.
//   k_selection_layers<S>   awsm_hip_read_selection: the same per-pixel function, its three results stored per pixel instead of blended.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include "frame_params.hpp"
#include "selection.hpp"
#include "launch.hpp"

namespace awsm {
namespace selection {

// a frame whose hand-off gate timed out is dropped whole (frame_params.hpp: frame_poisoned); wave-uniform
__device__ __forceinline__ bool poisoned(const SelectionDev& a) { return a.poison != nullptr && *a.poison == a.frame_serial; }
__device__ __forceinline__ float h2f(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
// the f32 blend result rounds to f16 once, as a value of its own: left to itself the compiler may select a mixed-precision FMA for f16(x + y),
// which rounds the exact sum once (kernels_ssao.hip: mul_f2h)
__device__ __forceinline__ uint32_t f2h(float v) { asm volatile("" : "+v"(v)); return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < __uint_as_float(0x7F800000u); }

// 1: selected draws
__global__ __launch_bounds__(256) void k_selection_mark(SelectionDev a) {
    if (poisoned(a)) return;
    const uint32_t d = blockIdx.x * 256u + threadIdx.x;
    if (d >= a.n_draws) return;
    const DrawDev dr = a.draws[d];
    const uint32_t material_meta_offset = *reinterpret_cast<const uint32_t*>(a.scene->buf[AWSM_BUF_GEOM_META] + dr.geom_meta_off + 36);
    const size_t mm_off = (size_t)(material_meta_offset / 256u) * 256u;
    bool sel = false;
    if (mm_off + 8u <= (size_t)a.material_meta_bytes) {
        const uint32_t* mm = reinterpret_cast<const uint32_t*>(a.scene->buf[AWSM_BUF_MATERIAL_META] + mm_off);
        const uint32_t hi = mm[0], lo = mm[1];
        for (uint32_t k = 0; k < a.n_keys; k++) sel = sel || (a.keys[2u * k] == hi && a.keys[2u * k + 1u] == lo);
    }
    a.draw_selected[d] = sel ? 1 : 0;
}

// 4: one edge of one box -> {sx0, sy0, sz0, sx1, sy1, sz1, valid, 0}; an invalid edge is all zeros
__global__ __launch_bounds__(256) void k_selection_edges(SelectionDev a) {
    if (poisoned(a)) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_boxes * kEdgesPerBox) return;
    const uint32_t b = i / kEdgesPerBox, j = i % kEdgesPerBox;
    const uint32_t axis = j >> 2, n = j & 3u;
    const uint32_t k0 = (n & ((1u << axis) - 1u)) | ((n >> axis) << (axis + 1u));      // the n-th corner without bit `axis`, ascending
    const uint32_t k1 = k0 | (1u << axis);
    const float* bx = a.boxes + 6u * b;
    const float* m = reinterpret_cast<const float*>(a.camera) + 32;      // view_proj, column-major
    float c[2][4];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const uint32_t k = e ? k1 : k0;
        const float X = bx[(k & 1u) ? 3 : 0], Y = bx[(k & 2u) ? 4 : 1], Z = bx[(k & 4u) ? 5 : 2];
#pragma unroll
        for (int r = 0; r < 4; r++) c[e][r] = ((m[r] * X + m[4 + r] * Y) + m[8 + r] * Z) + m[12 + r];
    }
    const bool out0 = !(c[0][2] >= 0.0f), out1 = !(c[1][2] >= 0.0f);
    bool valid = !(out0 && out1);
    if (valid && (out0 || out1)) {      // one endpoint behind the near plane: move it onto the plane
        const int o = out0 ? 0 : 1, q = 1 - o;
        const float t = (0.0f - c[o][2]) / (c[q][2] - c[o][2]);
        c[o][0] = c[o][0] + t * (c[q][0] - c[o][0]);
        c[o][1] = c[o][1] + t * (c[q][1] - c[o][1]);
        c[o][3] = c[o][3] + t * (c[q][3] - c[o][3]);
        c[o][2] = 0.0f;
    }
    if (!(c[0][3] > 0.0f) || !(c[1][3] > 0.0f)) valid = false;
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        const float W = (float)a.width, H = (float)a.height;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            s[3 * e + 0] = ((c[e][0] / c[e][3]) * 0.5f + 0.5f) * W;
            s[3 * e + 1] = (0.5f - (c[e][1] / c[e][3]) * 0.5f) * H;
            s[3 * e + 2] = c[e][2] / c[e][3];
        }
#pragma unroll
        for (int q = 0; q < 6; q++) valid = valid && is_finite(s[q]);
    }
    float4* out = reinterpret_cast<float4*>(a.edges + (size_t)i * kEdgeFloats);
    out[0] = valid ? make_float4(s[0], s[1], s[2], s[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[1] = valid ? make_float4(s[4], s[5], 1.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// 2: s(p) and d(p) from the pixel's S world keys
template <int S>
__device__ __forceinline__ void pixel_state(const SelectionDev& a, size_t p, bool& sel, float& d) {
    sel = false; d = 1.0f;
    bool hit = false;
#pragma unroll
    for (int s = 0; s < S; s++) {
        const unsigned long long k = a.vis[p * S + s];
        if (k == ~0ull) continue;
        const float ds = __uint_as_float((uint32_t)(k >> 32));
        d = hit ? fminf(d, ds) : ds;
        hit = true;
        const uint32_t rank = 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull);
        if (rank < a.total_tris) {
            const uint32_t draw = a.tri_info[rank] & 0x00FFFFFFu;
            if (draw < a.n_draws && a.draw_selected[draw]) sel = true;
        }
    }
}

// 5: one edge's alpha at the pixel centre (cx, cy); e = the edge's record, d = the world's depth at the pixel
__device__ __forceinline__ float edge_alpha(const float* __restrict__ e, float cx, float cy, float m, float d, float depth_epsilon, float hidden_alpha) {
    const float sx0 = e[0], sy0 = e[1], sz0 = e[2], sx1 = e[3], sy1 = e[4], sz1 = e[5];
    if (!(fminf(sx0, sx1) - m <= cx && cx <= fmaxf(sx0, sx1) + m && fminf(sy0, sy1) - m <= cy && cy <= fmaxf(sy0, sy1) + m)) return 0.0f;
    const float ex = sx1 - sx0, ey = sy1 - sy0;
    const float l2 = ex * ex + ey * ey;
    const float rx = cx - sx0, ry = cy - sy0;
    float t = l2 > 0.0f ? (rx * ex + ry * ey) / l2 : 0.0f;
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    const float qx = rx - t * ex, qy = ry - t * ey;
    const float dist = sqrtf(qx * qx + qy * qy);      // IEEE (-fhip-fp32-correctly-rounded-divide-sqrt, the default); __fsqrt_rn is the native approximation here
    const float cov = fminf(fmaxf(m - dist, 0.0f), 1.0f);
    const float z = sz0 + t * (sz1 - sz0);
    return (z - depth_epsilon) <= d ? cov : cov * hidden_alpha;
}

struct PixelOverlay { bool inside, selected, ring; float box_alpha; };

// 2, 3, 5, 6 for the thread's pixel of the workgroup's 16x16 tile.  Every thread of the workgroup calls it (barriers inside).
template <int S>
__device__ __forceinline__ PixelOverlay tile_pixel(const SelectionDev& a) {
    __shared__ unsigned char win[kWin * kWin];      // s of the tile and its apron; 0 outside the image
    __shared__ unsigned short list[kMaxEdges];      // the edges whose rectangle reaches the tile
    __shared__ uint32_t n_list, any_selected;
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    if (threadIdx.x == 0) { n_list = 0u; any_selected = 0u; }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < kWin * kWin; i += 256) {
        const int qx = x0 - kMaxRadius + i % kWin, qy = y0 - kMaxRadius + i / kWin;
        bool sel = false;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) { float d; pixel_state<S>(a, (size_t)qy * a.width + qx, sel, d); }
        win[i] = sel ? 1 : 0;
        if (sel) any_selected = 1u;
    }
    const float m = a.half_width + 0.5f;
    if (a.flags & kFlagBoxes) {
        // the tile's pixel centres span [x0 + 0.5, xl + 0.5] x [y0 + 0.5, yl + 0.5]; step 5's rectangle with the same roundings, so a pixel the gate
        // lets through always finds its edge in the list
        const float cx_lo = (float)x0 + 0.5f, cx_hi = (float)min(x0 + kTile - 1, W - 1) + 0.5f;
        const float cy_lo = (float)y0 + 0.5f, cy_hi = (float)min(y0 + kTile - 1, H - 1) + 0.5f;
        const uint32_t n_edges = a.n_boxes * kEdgesPerBox;
        for (uint32_t e = threadIdx.x; e < n_edges; e += 256u) {
            const float4 r0 = reinterpret_cast<const float4*>(a.edges)[2u * e], r1 = reinterpret_cast<const float4*>(a.edges)[2u * e + 1u];
            if (r1.z == 0.0f) continue;      // invalid
            if (fminf(r0.x, r0.w) - m <= cx_hi && cx_lo <= fmaxf(r0.x, r0.w) + m && fminf(r0.y, r1.x) - m <= cy_hi && cy_lo <= fmaxf(r0.y, r1.x) + m)
                list[atomicAdd(&n_list, 1u)] = (unsigned short)e;      // at most n_edges <= kMaxEdges entries: every edge is appended at most once
        }
    }
    __syncthreads();
    PixelOverlay o{x < W && y < H, false, false, 0.0f};
    const uint32_t count = n_list;
    if (!o.inside || (!any_selected && !count)) return o;
    const int li = (ly + kMaxRadius) * kWin + lx + kMaxRadius;
    o.selected = win[li] != 0;
    // 3: the ring, from the window only
    if (any_selected && (a.flags & kFlagOutline) && !o.selected) {
        const int R = (int)a.radius, R2 = R * R;
#pragma unroll
        for (int dy = -kMaxRadius; dy <= kMaxRadius; dy++)
#pragma unroll
            for (int dx = -kMaxRadius; dx <= kMaxRadius; dx++)
                if (dx * dx + dy * dy <= R2 && win[li + dy * kWin + dx]) o.ring = true;
    }
    // 5 + 6: the box alpha over the listed edges
    if (count) {
        bool sel; float d;
        pixel_state<S>(a, (size_t)y * a.width + x, sel, d);
        const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
        float A = 0.0f;
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t e = __builtin_amdgcn_readfirstlane((uint32_t)list[i]);      // the same for every lane: the record comes through the scalar path
            A = fmaxf(A, edge_alpha(a.edges + (size_t)e * kEdgeFloats, cx, cy, m, d, a.depth_epsilon, a.hidden_alpha));
        }
        o.box_alpha = A;
    }
    return o;
}

// 7: C over `color` with alpha `al`, one channel
__device__ __forceinline__ float over(float C, float color, float al) { return (C * (1.0f - al)) + (color * al); }

template <int S>
__global__ __launch_bounds__(256) void k_selection_overlay(SelectionDev a) {
    if (poisoned(a)) return;
    const PixelOverlay o = tile_pixel<S>(a);
    if (!o.inside || !(o.ring || o.box_alpha > 0.0f)) return;
    const size_t p = (size_t)(blockIdx.y * kTile + (threadIdx.x >> 4)) * a.width + (blockIdx.x * kTile + (threadIdx.x & 15u));
    const uint2 v = a.out16[p];
    float c[4] = {h2f(v.x & 0xFFFFu), h2f(v.x >> 16), h2f(v.y & 0xFFFFu), h2f(v.y >> 16)};
    if (o.ring) {
        const float al = a.outline_color[3];
        c[0] = over(c[0], a.outline_color[0], al); c[1] = over(c[1], a.outline_color[1], al); c[2] = over(c[2], a.outline_color[2], al);
        c[3] = (c[3] * (1.0f - al)) + al;
    }
    if (o.box_alpha > 0.0f) {
        const float al = a.box_color[3] * o.box_alpha;
        c[0] = over(c[0], a.box_color[0], al); c[1] = over(c[1], a.box_color[1], al); c[2] = over(c[2], a.box_color[2], al);
        c[3] = (c[3] * (1.0f - al)) + al;
    }
    const uint32_t h0 = f2h(c[0]), h1 = f2h(c[1]), h2 = f2h(c[2]), h3 = f2h(c[3]);
    a.out16[p] = make_uint2(h0 | (h1 << 16), h2 | (h3 << 16));
    if (a.out32) a.out32[p] = make_float4(h2f(h0), h2f(h1), h2f(h2), h2f(h3));      // the tap's rule in the composite: the stored halves, widened
}

template <int S>
__global__ __launch_bounds__(256) void k_selection_layers(SelectionDev a) {
    const PixelOverlay o = tile_pixel<S>(a);
    if (!o.inside) return;
    const size_t p = (size_t)(blockIdx.y * kTile + (threadIdx.x >> 4)) * a.width + (blockIdx.x * kTile + (threadIdx.x & 15u));
    a.layer_selected[p] = o.selected ? 1 : 0;
    a.layer_ring[p] = o.ring ? 1 : 0;
    a.layer_box_alpha[p] = o.box_alpha;
}

}  // namespace selection
}  // namespace awsm

using awsm::SelectionDev;

static void launch_tables(const SelectionDev& a, hipStream_t s) {
    if (a.n_draws) awsm::selection::k_selection_mark<<<dim3((a.n_draws + 255u) / 256u), dim3(256), 0, s>>>(a);
    const uint32_t n_edges = a.n_boxes * awsm::selection::kEdgesPerBox;
    if (n_edges) awsm::selection::k_selection_edges<<<dim3((n_edges + 255u) / 256u), dim3(256), 0, s>>>(a);
}

// the selection overlay behind the world transparent pass's kernels: mark, edges, overlay
extern "C" void awsm_launch_selection(const SelectionDev* args, hipStream_t s) {
    const SelectionDev& a = *args;
    if (!a.width || !a.height) return;
    launch_tables(a, s);
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    if (a.msaa == 4) awsm::selection::k_selection_overlay<4><<<grid, block, 0, s>>>(a);
    else awsm::selection::k_selection_overlay<1><<<grid, block, 0, s>>>(a);
}

// awsm_hip_read_selection: the same tables and per-pixel function once more, into args->layer_*
extern "C" void awsm_launch_selection_layers(const SelectionDev* args, hipStream_t s) {
    const SelectionDev& a = *args;
    if (!a.width || !a.height) return;
    launch_tables(a, s);
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    if (a.msaa == 4) awsm::selection::k_selection_layers<4><<<grid, block, 0, s>>>(a);
    else awsm::selection::k_selection_layers<1><<<grid, block, 0, s>>>(a);
}
