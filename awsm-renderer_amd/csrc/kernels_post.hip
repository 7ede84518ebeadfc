// kernels_post.hip — the effects pass and the display pass (render.rs:339-356) for gfx950.
//
//   effects  render_passes/effects/{render_pass,pipeline}.rs, effects_wgsl/{compute.wgsl, helpers/{smaa,bloom,dof}.wgsl}
//   display  render_passes/display/render_pass.rs, display_wgsl/{fragment.wgsl, helpers/tonemap.wgsl}, shared_wgsl/color_space.wgsl
//
// The contract these kernels follow (and tests/post_oracle.py with them) is DESIGN.md §11: clamp-to-edge loads for every stencil (SMAA
// included), the two fixed f32 tables below, the WGSL loop order for every sum, an f16 rounding at every former dispatch boundary, and
// unorm8 = floor(clamp(v, 0, 1) * 255 + 0.5) (NaN -> 0) as k_gen_mip_level stores it.  -ffp-contract=off (Makefile) keeps the products
// and sums unfused.
//
//   k_post_dof_depth   DoF only: per pixel, the depth as it stands after the world transparent pass (min over the MSAA samples, 1.0 where
//                      nothing was hit), then linearize_depth and calculate_coc once — the 16 taps of every neighbour read them instead of
//                      evaluating them again.  The transparent pass's writes are recovered from its fragment lists (each listed fragment
//                      passed the depth test for the samples in its mask and wrote its depth there), with the raster contract's own
//                      depth functions (raster_setup.hpp), so the value is the one k_forward_cover held.
//   k_post_dof_blur    DoF only: the 16-tap disk blur of the composite and the blend factor, once per pixel.  Every bloom stage mixes
//                      the same blur (the reference runs apply_dof in each of its five dispatches), so it is computed once for all.
//   k_post_main        bloom off: SMAA (the lumas of a 16x16 tile and its one-texel apron staged once in LDS) -> DoF mix -> f16 ->
//                      tone map -> sRGB -> RGBA8: the effects dispatch and the display pass in one kernel.
//   k_post_bloom       bloom on: one kernel per former dispatch (extract, three blurs, blend); each stages its 20x20 source window in LDS
//                      (the extract stages bloom_threshold of each texel, computed once), stores f16, and the blend stage also writes
//                      the display image.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include "frame_params.hpp"
#include "raster_setup.hpp"
#include "launch.hpp"

namespace awsm {
namespace post {

constexpr int kT = 16;                 // tile edge (one 256-thread workgroup, one pixel per thread)
constexpr uint32_t kFragNone = 0xFFFFFFFFu;

// blur_sample / the extract loop (bloom.wgsl): taps with dx^2 + dy^2 <= BLOOM_RADIUS^2 + 0.5 in (dy, dx) loop order, weights
// exp(-d^2 / (2 sigma^2)) / sum, sigma = 2, rounded once to f32 (tests/post_oracle.py derives the same table; a CPU test compares them)
__constant__ const int kBloomTap[13][2] = {{0, -2}, {-1, -1}, {0, -1}, {1, -1}, {-2, 0}, {-1, 0}, {0, 0}, {1, 0}, {2, 0}, {-1, 1}, {0, 1}, {1, 1}, {0, 2}};
__constant__ const float kBloomW[13] = {6.022359058e-02f, 7.732862234e-02f, 8.762481064e-02f, 7.732862234e-02f, 6.022359058e-02f, 8.762481064e-02f, 9.929191321e-02f,
                                        8.762481064e-02f, 6.022359058e-02f, 7.732862234e-02f, 8.762481064e-02f, 7.732862234e-02f, 6.022359058e-02f};
// get_disk_offset (dof.wgsl): (cos, sin)(f32(i) * 2.39996323) * sqrt((i + 1) / 16), rounded once to f32; offset = table * CoC
__constant__ const float kDisk[16][2] = {
    {2.500000000e-01f, 0.000000000e+00f}, {-2.606992424e-01f, 2.388219088e-01f}, {3.785637394e-02f, -4.313547313e-01f}, {3.042196333e-01f, 3.968002200e-01f},
    {-5.504716039e-01f, -9.737047553e-02f}, {5.166924000e-01f, -3.286775649e-01f}, {-1.717114598e-01f, 6.387606263e-01f}, {-3.259110153e-01f, -6.275205016e-01f},
    {7.044911385e-01f, 2.572784722e-01f}, {-7.307591438e-01f, 3.016472459e-01f}, {3.514342308e-01f, -7.509953380e-01f}, {2.591876388e-01f, 8.263303041e-01f},
    {-7.798917890e-01f, -4.519611001e-01f}, {9.135961533e-01f, -2.008533478e-01f}, {-5.568653345e-01f, 7.920864820e-01f}, {-1.285122484e-01f, -9.917079210e-01f}};


__device__ __forceinline__ float h2f(unsigned short h) { return __half2float(__ushort_as_half(h)); }
__device__ __forceinline__ unsigned short f2h(float v) { return __half_as_ushort(__float2half_rn(v)); }
__device__ __forceinline__ float3 load_rgb(const uint2* img, size_t p) { const uint2 v = img[p]; return make_float3(h2f((unsigned short)(v.x & 0xFFFFu)), h2f((unsigned short)(v.x >> 16)), h2f((unsigned short)(v.y & 0xFFFFu))); }
__device__ __forceinline__ float3 round_f16(float3 c) { return make_float3(h2f(f2h(c.x)), h2f(f2h(c.y)), h2f(f2h(c.z))); }
__device__ __forceinline__ uint2 pack_f16(float3 c) { return make_uint2((uint32_t)f2h(c.x) | ((uint32_t)f2h(c.y) << 16), (uint32_t)f2h(c.z) | (0x3C00u << 16)); }   // vec4(rgb, 1.0)
__device__ __forceinline__ float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }
__device__ __forceinline__ float3 mix3(float3 a, float3 b, float t) { return make_float3(mixf(a.x, b.x, t), mixf(a.y, b.y, t), mixf(a.z, b.z, t)); }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float smoothstepf(float e0, float e1, float x) { const float t = clamp01((x - e0) / (e1 - e0)); return t * t * (3.0f - 2.0f * t); }
__device__ __forceinline__ float luma(float3 c) { return c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f; }      // rgb_to_luma: dot, left to right

// linear_to_srgb (shared_wgsl/color_space.wgsl); the exponent is the f32 nearest 1/2.4
__device__ __forceinline__ float srgb1(float c) { return c <= 0.0031308f ? c * 12.92f : 1.055f * powf(c, 0.416666657f) - 0.055f; }
__device__ __forceinline__ float3 srgb(float3 c) { return make_float3(srgb1(c.x), srgb1(c.y), srgb1(c.z)); }
// The SMAA lumas decide edges by comparison, so a last-bit difference of powf could flip a pixel's blend: there the power is evaluated in f64
// and rounded once to f32 (the correctly rounded value, bar cases below 1e-8 per texel), which the oracle reproduces with numpy's f64 pow.
__device__ __forceinline__ float srgb1_exact(float c) { return c <= 0.0031308f ? c * 12.92f : 1.055f * (float)pow((double)c, (double)0.416666657f) - 0.055f; }
__device__ __forceinline__ float smaa_luma(float3 c) { return luma(make_float3(srgb1_exact(c.x), srgb1_exact(c.y), srgb1_exact(c.z))); }
// a frame whose hand-off gate timed out is dropped whole (frame_params.hpp: frame_poisoned); wave-uniform
__device__ __forceinline__ bool post_poisoned(const PostArgs& a) { return a.poison != nullptr && *a.poison == a.frame_serial; }

// tonemap.wgsl
__device__ __forceinline__ float3 khronos_neutral(float3 c) {
    const float start = 0.8f - 0.04f, desat = 0.15f;
    const float x = fminf(c.x, fminf(c.y, c.z));
    const float offset = x < 0.08f ? x - 6.25f * x * x : 0.04f;
    float3 r = make_float3(c.x - offset, c.y - offset, c.z - offset);
    const float peak = fmaxf(r.x, fmaxf(r.y, r.z));
    if (peak < start) return r;
    const float d = 1.0f - start;
    const float new_peak = 1.0f - d * d / (peak + d - start);
    const float s = new_peak / peak;
    r = make_float3(r.x * s, r.y * s, r.z * s);
    const float g = 1.0f - 1.0f / (desat * (peak - new_peak) + 1.0f);
    return mix3(r, make_float3(new_peak, new_peak, new_peak), g);
}
__device__ __forceinline__ float aces1(float x) { const float num = x * (2.51f * x + 0.03f), den = x * (2.43f * x + 0.59f) + 0.14f; return clamp01(num / den); }
__device__ __forceinline__ float3 tone_map(float3 c, uint32_t op) {
    if (op == 1u) return khronos_neutral(c);
    if (op == 2u) return make_float3(aces1(c.x), aces1(c.y), aces1(c.z));
    return c;
}
__device__ __forceinline__ uint32_t unorm8(float v) { return (uint32_t)floorf(clamp01(v) * 255.0f + 0.5f); }      // fmaxf(NaN, 0) = 0
// display pass on an effects texel that was stored as f16: alpha 1.0 -> 255
__device__ __forceinline__ uint32_t display_texel(float3 stored, uint32_t op) {
    const float3 s = srgb(tone_map(stored, op));
    return unorm8(s.x) | (unorm8(s.y) << 8) | (unorm8(s.z) << 16) | (255u << 24);
}

// dof.wgsl: linearize_depth, calculate_coc
__device__ __forceinline__ float2 dof_linear_coc(float depth, const float* cam) {
    const float near = cam[16 + 14], p22 = cam[16 + 10], p11 = cam[16 + 5];
    float lin;
    if (fabsf(p22) < 0.0001f) lin = near / fmaxf(depth, 0.0001f);
    else { const float far = near / (p22 + 1.0f); lin = (near * far) / (far - depth * (far - near)); }
    const float S = cam[124], N = cam[125], f = 0.012f * p11;
    const float A = f / fmaxf(N, 0.1f);
    const float coc_world = A * f * fabsf(lin - S) / (lin * fmaxf(S, 0.001f));
    const float coc_px = coc_world * cam[123] / 0.024f;
    return make_float2(lin, fminf(fmaxf(coc_px, 0.0f), 16.0f));
}

__device__ __forceinline__ float key_depth(unsigned long long k) { return k == ~0ull ? 1.0f : __uint_as_float((uint32_t)(k >> 32)); }

template <int S>
__global__ __launch_bounds__(256) void k_post_dof_depth(PostArgs a) {
    if (post_poisoned(a)) return;
    const uint32_t x = blockIdx.x * kT + (threadIdx.x & 15u), y = blockIdx.y * kT + (threadIdx.x >> 4);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    float d = S == 1 ? key_depth(a.vis[p]) : 1.0f;
#pragma unroll
    for (int s = 0; S == 4 && s < 4; s++) d = fminf(d, key_depth(a.vis[p * 4 + s]));
    if (a.frag_first) {       // depth write of the transparent pipeline (material_transparent/pipeline.rs:180): what its fragments left
        uint32_t i = a.frag_first[p];
        for (uint32_t guard = 0; i != kFragNone && i < a.frag_cap && guard < a.frag_cap; guard++) {
            const uint4 rec = a.frag_rec[i];
            TriSetup t;
            if (tri_rec_load(a.tri_rec + rec.x, t)) {
                const uint32_t mask = rec.w & 0xFu;
                if (S == 1) {
                    const unsigned long long k = tri_sample_key_at(t, sample_coord(((int)x << 8) + 128), sample_coord(((int)y << 8) + 128), rec.x);
                    if (mask && k != ~0ull) d = fminf(d, __uint_as_float((uint32_t)(k >> 32)));
                } else {
                    float dz[4];
                    const float zc = tri_plane_depth(t, tri_edges_d(t, (double)x, (double)y)) + 0.0f;
                    msaa_depth_steps(t.a, t.b, t.zq, dz);
                    for (int s = 0; s < 4; s++) {
                        if (!(mask & (1u << s))) continue;
                        const unsigned long long k = tri_msaa_sample_key(t, (int)x, (int)y, s, zc, dz, rec.x);
                        if (k != ~0ull) d = fminf(d, __uint_as_float((uint32_t)(k >> 32)));
                    }
                }
            }
            i = rec.z;
        }
    }
    a.dof_lc[p] = dof_linear_coc(d, a.camera);
}

// apply_dof's disk blur (dof.wgsl), per pixel once
__global__ __launch_bounds__(256) void k_post_dof_blur(PostArgs a) {
    if (post_poisoned(a)) return;
    const int x = (int)(blockIdx.x * kT + (threadIdx.x & 15u)), y = (int)(blockIdx.y * kT + (threadIdx.x >> 4));
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float2 c = a.dof_lc[p];
    const float center_linear = c.x, center_coc = c.y;
    if (!(center_coc >= 0.5f)) { a.dof_blur[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f); return; }
    float3 blur = make_float3(0.0f, 0.0f, 0.0f);
    float total = 0.0f;
    for (int i = 0; i < 16; i++) {
        const float ox = kDisk[i][0] * center_coc, oy = kDisk[i][1] * center_coc;
        const int sx = min(max(x + (int)rintf(ox), 0), (int)a.width - 1), sy = min(max(y + (int)rintf(oy), 0), (int)a.height - 1);   // round: halves to even
        const size_t q = (size_t)sy * a.width + sx;
        const float3 sc = load_rgb(a.src, q);
        const float2 s = a.dof_lc[q];
        float w = 1.0f;
        if (s.x > center_linear && s.y < center_coc) w = s.y / fmaxf(center_coc, 0.01f);
        const float dist = sqrtf(ox * ox + oy * oy);
        w *= 1.0f - smoothstepf(center_coc * 0.5f, center_coc, dist);
        w = fmaxf(w, 0.01f);
        blur = make_float3(blur.x + sc.x * w, blur.y + sc.y * w, blur.z + sc.z * w);
        total += w;
    }
    const float inv = fmaxf(total, 0.01f);
    a.dof_blur[p] = make_float4(blur.x / inv, blur.y / inv, blur.z / inv, smoothstepf(0.0f, 2.0f, center_coc));
}

__device__ __forceinline__ float3 apply_dof(float3 rgb, const PostArgs& a, size_t p) {
    const float4 b = a.dof_blur[p];
    return b.w < 0.0f ? rgb : mix3(rgb, make_float3(b.x, b.y, b.z), b.w);
}

// effects (bloom off) + display.  SMAA (smaa.wgsl) on the composite with clamp-to-edge neighbours; lumas once per staged texel.
template <bool SMAA, bool DOF>
__global__ __launch_bounds__(256) void k_post_main(PostArgs a) {
    if (post_poisoned(a)) return;
    constexpr int W = kT + 2;
    __shared__ float4 tile[SMAA ? W * W : 1];     // rgb + sRGB luma
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kT, y0 = (int)blockIdx.y * kT;
    const int x = x0 + lx, y = y0 + ly;
    if (SMAA) {
        for (int i = (int)threadIdx.x; i < W * W; i += 256) {
            const int gx = min(max(x0 - 1 + i % W, 0), (int)a.width - 1), gy = min(max(y0 - 1 + i / W, 0), (int)a.height - 1);
            const float3 c = load_rgb(a.src, (size_t)gy * a.width + gx);
            tile[i] = make_float4(c.x, c.y, c.z, smaa_luma(c));
        }
        __syncthreads();
    }
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    float3 rgb;
    if (SMAA) {
        auto at = [&](int dx, int dy) -> const float4& { return tile[(ly + 1 + dy) * W + lx + 1 + dx]; };
        const float4 c = at(0, 0);
        rgb = make_float3(c.x, c.y, c.z);
        const float cl = c.w;
        const float l_l = at(-1, 0).w, l_r = at(1, 0).w, l_t = at(0, -1).w, l_b = at(0, 1).w;
        const float l_tl = at(-1, -1).w, l_tr = at(1, -1).w, l_bl = at(-1, 1).w, l_br = at(1, 1).w;
        const float d_l = fabsf(cl - l_l), d_r = fabsf(cl - l_r), d_t = fabsf(cl - l_t), d_b = fabsf(cl - l_b);
        const float d_tl = fabsf(cl - l_tl), d_tr = fabsf(cl - l_tr), d_bl = fabsf(cl - l_bl), d_br = fabsf(cl - l_br);
        const float max_h = fmaxf(d_l, d_r), max_v = fmaxf(d_t, d_b), max_d = fmaxf(fmaxf(d_tl, d_tr), fmaxf(d_bl, d_br));
        const float max_delta = fmaxf(fmaxf(max_h, max_v), max_d);
        if (!(max_delta < 0.03f)) {
            if (max_d > fmaxf(max_h, max_v)) {                  // diagonal_blending
                const float wtl = 1.0f / (d_tl + 0.001f), wtr = 1.0f / (d_tr + 0.001f), wbl = 1.0f / (d_bl + 0.001f), wbr = 1.0f / (d_br + 0.001f);
                const float tot = wtl + wtr + wbl + wbr;
                const float ntl = wtl / tot, ntr = wtr / tot, nbl = wbl / tot, nbr = wbr / tot;
                const float4 tl = at(-1, -1), tr = at(1, -1), bl = at(-1, 1), br = at(1, 1);
                const float3 nb = make_float3(tl.x * ntl + tr.x * ntr + bl.x * nbl + br.x * nbr, tl.y * ntl + tr.y * ntr + bl.y * nbl + br.y * nbr,
                                              tl.z * ntl + tr.z * ntr + bl.z * nbl + br.z * nbr);
                rgb = mix3(rgb, nb, 0.6f);
            } else {                                            // calculate_blending_weights_{horizontal,vertical} + neighborhood_blending
                const bool horiz = max_h > max_v;
                const float ca = horiz ? d_t : d_l, cb = horiz ? d_b : d_r;
                float wa = 1.0f / (ca + 0.001f), wb = 1.0f / (cb + 0.001f);
                const float tot = wa + wb;
                wa = wa / tot * 0.6f; wb = wb / tot * 0.6f;
                const float4 na = horiz ? at(0, -1) : at(-1, 0), nbv = horiz ? at(0, 1) : at(1, 0);
                if (wa > 0.0f) rgb = mix3(rgb, make_float3(na.x, na.y, na.z), wa);
                if (wb > 0.0f) rgb = mix3(rgb, make_float3(nbv.x, nbv.y, nbv.z), wb);
            }
        }
    } else {
        rgb = load_rgb(a.src, p);
    }
    if (DOF) rgb = apply_dof(rgb, a, p);
    if (a.effects) a.effects[p] = pack_f16(rgb);
    a.display[p] = display_texel(round_f16(rgb), a.tonemap);
}

// bloom.wgsl, one former dispatch: PHASE 0 extract (composite -> stage_out), 1 blur (stage_in -> stage_out), 2 blend (stage_in + composite
// -> effects + display).  apply_smaa's result is ignored by every apply_bloom (quirk), so SMAA never runs here; DoF runs in every stage.
template <int PHASE, bool DOF>
__global__ __launch_bounds__(256) void k_post_bloom(PostArgs a) {
    if (post_poisoned(a)) return;
    constexpr int W = kT + 4;
    __shared__ float4 tile[W * W];
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kT, y0 = (int)blockIdx.y * kT;
    const int x = x0 + lx, y = y0 + ly;
    const uint2* in = PHASE == 0 ? a.src : a.stage_in;
    for (int i = (int)threadIdx.x; i < W * W; i += 256) {
        const int gx = min(max(x0 - 2 + i % W, 0), (int)a.width - 1), gy = min(max(y0 - 2 + i / W, 0), (int)a.height - 1);
        float3 c = load_rgb(in, (size_t)gy * a.width + gx);
        if (PHASE == 0) {           // bloom_threshold, once per texel
            const float brightness = luma(c);
            const float contribution = fmaxf(brightness - 0.8f, 0.0f);
            const float soft_threshold = 0.8f * 0.8f, knee = 0.8f - soft_threshold;
            const float soft = clamp01((brightness - soft_threshold) / knee);
            const float factor = contribution / fmaxf(brightness, 0.0001f) * soft;
            c = make_float3(c.x * factor, c.y * factor, c.z * factor);
        }
        tile[i] = make_float4(c.x, c.y, c.z, 0.0f);
    }
    __syncthreads();
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    float3 acc = make_float3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const float4 s = tile[(ly + 2 + kBloomTap[k][1]) * W + lx + 2 + kBloomTap[k][0]];
        const float w = kBloomW[k];
        acc = make_float3(acc.x + s.x * w, acc.y + s.y * w, acc.z + s.z * w);
    }
    if (PHASE == 2) {
        const float3 o = load_rgb(a.src, p);
        acc = make_float3(o.x + acc.x * 0.5f, o.y + acc.y * 0.5f, o.z + acc.z * 0.5f);
    }
    if (DOF) acc = apply_dof(acc, a, p);
    if (PHASE < 2) { a.stage_out[p] = pack_f16(acc); return; }
    if (a.stage_out) a.stage_out[p] = pack_f16(acc);
    a.display[p] = display_texel(round_f16(acc), a.tonemap);
}

}  // namespace post
}  // namespace awsm

using awsm::PostArgs;

// flags: 1 SMAA, 2 bloom, 4 DoF (AWSM_POST_*); msaa: 1 or 4.  bloom_a / bloom_b: the two f16 ping-pong images of the bloom chain.
extern "C" void awsm_launch_post(const PostArgs* args, uint32_t flags, uint32_t msaa, void* bloom_a, void* bloom_b, hipStream_t s) {
    PostArgs a = *args;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    const bool smaa = flags & 1u, bloom = flags & 2u, dof = flags & 4u;
    if (dof) {
        if (msaa == 4) awsm::post::k_post_dof_depth<4><<<grid, block, 0, s>>>(a);
        else awsm::post::k_post_dof_depth<1><<<grid, block, 0, s>>>(a);
        awsm::post::k_post_dof_blur<<<grid, block, 0, s>>>(a);
    }
    if (!bloom) {
        if (smaa && dof) awsm::post::k_post_main<true, true><<<grid, block, 0, s>>>(a);
        else if (smaa) awsm::post::k_post_main<true, false><<<grid, block, 0, s>>>(a);
        else if (dof) awsm::post::k_post_main<false, true><<<grid, block, 0, s>>>(a);
        else awsm::post::k_post_main<false, false><<<grid, block, 0, s>>>(a);
        return;
    }
    // extract -> A, blur A -> B, B -> A, A -> B, blend B -> effects (effects/render_pass.rs:40-60, BLOOM_BLUR_PASSES = 3)
    uint2* A = (uint2*)bloom_a; uint2* B = (uint2*)bloom_b;
    uint2* effects = a.effects;
    a.stage_in = nullptr; a.stage_out = A;
    if (dof) awsm::post::k_post_bloom<0, true><<<grid, block, 0, s>>>(a); else awsm::post::k_post_bloom<0, false><<<grid, block, 0, s>>>(a);
    for (int i = 0; i < 3; i++) {
        a.stage_in = (i & 1) ? B : A; a.stage_out = (i & 1) ? A : B;
        if (dof) awsm::post::k_post_bloom<1, true><<<grid, block, 0, s>>>(a); else awsm::post::k_post_bloom<1, false><<<grid, block, 0, s>>>(a);
    }
    a.stage_in = B; a.stage_out = effects;
    if (dof) awsm::post::k_post_bloom<2, true><<<grid, block, 0, s>>>(a); else awsm::post::k_post_bloom<2, false><<<grid, block, 0, s>>>(a);
}
