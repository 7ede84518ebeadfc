// kernels_shadow.hip — the shadow resolve: a pixel's world position looked up in the light's depth map, multiplied into the opaque image
// (gfx950).  The map itself is made by the world geometry pass's kernels from the light's camera (awsm_hip.cpp: enqueue_shadow).
//
// The contract this kernel follows, and tests/shadow_reference.py with it operation for operation: f32 throughout with nothing fused
// (-ffp-contract=off, Makefile), only + - * / and sqrt in their IEEE forms, sums left to right, a matrix row ((m0 x + m1 y) + m2 z) + m3 w.
// The device is held to the restatement's exact bits.
//
//   k_shadow_resolve<S>   per 16x16 tile: for the tile and a one-pixel apron the world position (from the world keys' depth, the least of the S
//                         samples, through the snapshot's inv_view_proj) and the light's (u, v, z) are formed once and staged in LDS,
//                         18 x 18 x {Pw, u, v, z, d, flags}.  Every pixel then picks one horizontal and one vertical neighbour from LDS — they give
//                         the normal for the facing term and the receiver plane's depth slope for the bias — takes its (2R+1)^2 taps as 4-byte
//                         gathers of the map keys' depth words, and multiplies rgb by m = 1 - strength g (1 - V).  Writes V and m per pixel.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstdint>
#include "frame_params.hpp"
#include "shadow.hpp"
#include "launch.hpp"

namespace awsm {
namespace shadow {

// a frame whose hand-off gate timed out is dropped whole (frame_params.hpp: frame_poisoned); wave-uniform
__device__ __forceinline__ bool poisoned(const ShadowArgs& a) { return a.poison != nullptr && *a.poison == a.frame_serial; }
__device__ __forceinline__ float h2f(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
__device__ __forceinline__ uint32_t f2h(float v) { return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
// f16_rne(f32(stored half) * m) rounds twice, to f32 and then to f16: the f32 product is kept a value of its own, as in kernels_ssao.hip — left to
// itself the compiler selects v_fma_mixlo_f16, which rounds the exact product once.  The statement holds no instruction.
__device__ __forceinline__ uint32_t mul_f2h(float h, float m) { float v = h * m; asm volatile("" : "+v"(v)); return f2h(v); }

template <int S>
__global__ __launch_bounds__(256) void k_shadow_resolve(ShadowArgs a) {
    if (poisoned(a)) return;
    __shared__ float wx[kWin * kWin], wy[kWin * kWin], wz[kWin * kWin], wu[kWin * kWin], wv[kWin * kWin], wl[kWin * kWin], wd[kWin * kWin];
    __shared__ unsigned char wf[kWin * kWin];
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    const float* ip = a.camera + 48;      // inv_view_proj, column-major
    const float* lp = a.light_view_proj;
    const float sx2 = 2.0f / (float)W, sy2 = 2.0f / (float)H, Sf = (float)a.map_size;
    // 1 - 3: depth, world position and light coordinates of every window cell inside the image (no neighbour ever names a cell outside it)
    for (int i = (int)threadIdx.x; i < kWin * kWin; i += 256) {
        const int cx = x0 - 1 + i % kWin, cy = y0 - 1 + i / kWin;
        float px = 0.0f, py = 0.0f, pz = 0.0f, u = 0.0f, v = 0.0f, z = 0.0f, d = 0.0f;
        unsigned flags = 0u;
        if (cx >= 0 && cx < W && cy >= 0 && cy < H) {
            const size_t p = (size_t)cy * a.width + cx;
            bool hit = false;
#pragma unroll
            for (int s = 0; s < S; s++) {
                const unsigned long long k = a.vis[p * S + s];
                if (k != ~0ull) { const float ds = __uint_as_float((uint32_t)(k >> 32)); d = hit ? fminf(d, ds) : ds; hit = true; }
            }
            if (hit) {
                const float nx = ((float)cx + 0.5f) * sx2 - 1.0f;
                const float ny = 1.0f - ((float)cy + 0.5f) * sy2;
                const float c0 = ((ip[0] * nx + ip[4] * ny) + ip[8] * d) + ip[12];
                const float c1 = ((ip[1] * nx + ip[5] * ny) + ip[9] * d) + ip[13];
                const float c2 = ((ip[2] * nx + ip[6] * ny) + ip[10] * d) + ip[14];
                const float c3 = ((ip[3] * nx + ip[7] * ny) + ip[11] * d) + ip[15];
                px = c0 / c3; py = c1 / c3; pz = c2 / c3;
                const float q0 = ((lp[0] * px + lp[4] * py) + lp[8] * pz) + lp[12];
                const float q1 = ((lp[1] * px + lp[5] * py) + lp[9] * pz) + lp[13];
                const float q2 = ((lp[2] * px + lp[6] * py) + lp[10] * pz) + lp[14];
                const float q3 = ((lp[3] * px + lp[7] * py) + lp[11] * pz) + lp[15];
                const float l0 = q0 / q3, l1 = q1 / q3;
                z = q2 / q3;
                u = (l0 * 0.5f + 0.5f) * Sf;
                v = (0.5f - l1 * 0.5f) * Sf;
                const bool inside = q3 > 0.0f && u >= 0.0f && u < Sf && v >= 0.0f && v < Sf && z >= 0.0f && z <= 1.0f;      // any NaN: false
                flags = kHit | (inside ? kInside : 0u);
            } else d = 0.0f;
        }
        wx[i] = px; wy[i] = py; wz[i] = pz; wu[i] = u; wv[i] = v; wl[i] = z; wd[i] = d; wf[i] = (unsigned char)flags;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const int li = (ly + 1) * kWin + lx + 1;
    const size_t p = (size_t)y * a.width + x;
    const unsigned fl = wf[li];
    if (!(fl & kHit)) { a.visibility[p] = 1.0f; a.multiplier[p] = 1.0f; return; }
    const float Px = wx[li], Py = wy[li], Pz = wz[li], u = wu[li], v = wv[li], z = wl[li], d = wd[li];
    // 4: one neighbour along each image axis — inside the image and hit, the nearer in depth, the +1 one on a tie
    const bool hf = x + 1 < W && (wf[li + 1] & kHit), hb = x - 1 >= 0 && (wf[li - 1] & kHit);
    const bool vf = y + 1 < H && (wf[li + kWin] & kHit), vb = y - 1 >= 0 && (wf[li - kWin] & kHit);
    const bool use_hf = hf && (!hb || fabsf(wd[li + 1] - d) <= fabsf(wd[li - 1] - d));
    const bool use_vf = vf && (!vb || fabsf(wd[li + kWin] - d) <= fabsf(wd[li - kWin] - d));
    const int qh = use_hf ? li + 1 : li - 1, qv = use_vf ? li + kWin : li - kWin;
    const bool has_h = hf || hb, has_v = vf || vb;
    // differences: neighbour - p for the +1 neighbour, p - neighbour for the -1 one
#define AWSM_DIFF(arr, q, fwd, centre) ((fwd) ? (arr[q] - (centre)) : ((centre) - arr[q]))
    const float hx = AWSM_DIFF(wx, qh, use_hf, Px), hy = AWSM_DIFF(wy, qh, use_hf, Py), hz = AWSM_DIFF(wz, qh, use_hf, Pz);
    const float vx = AWSM_DIFF(wx, qv, use_vf, Px), vy = AWSM_DIFF(wy, qv, use_vf, Py), vz = AWSM_DIFF(wz, qv, use_vf, Pz);
    // 5: normal and facing
    float nx = hy * vz - hz * vy, ny = hz * vx - hx * vz, nz = hx * vy - hy * vx;
    const float* cam = a.camera + 96;
    const float ex = cam[0] - Px, ey = cam[1] - Py, ez = cam[2] - Pz;
    if ((nx * ex + ny * ey) + nz * ez < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float ln = sqrtf(nn);      // IEEE (the default correctly rounded sqrt); __fsqrt_rn is the native approximation here
    nx = nx / ln; ny = ny / ln; nz = nz / ln;
    float Lx = a.light[0], Ly = a.light[1], Lz = a.light[2];
    if (a.light[3] != 0.0f) {
        Lx = Lx - Px; Ly = Ly - Py; Lz = Lz - Pz;
        const float ll = sqrtf((Lx * Lx + Ly * Ly) + Lz * Lz);
        Lx = Lx / ll; Ly = Ly / ll; Lz = Lz / ll;
    }
    const float cos_t = (nx * Lx + ny * Ly) + nz * Lz;
    float g = 1.0f;
    if (has_h && has_v && nn > 0.0f) g = cos_t > 0.0f ? fminf(1.0f, cos_t / a.facing_fade) : 0.0f;
    float V = 1.0f;
    if (fl & kInside) {
        // 6: the receiver plane's depth slope per texel, from the same neighbours
        float zu = 0.0f, zv = 0.0f;
        if (has_h && has_v && (wf[qh] & kInside) && (wf[qv] & kInside)) {
            const float uh = AWSM_DIFF(wu, qh, use_hf, u), vh = AWSM_DIFF(wv, qh, use_hf, v), zh = AWSM_DIFF(wl, qh, use_hf, z);
            const float uv = AWSM_DIFF(wu, qv, use_vf, u), vv = AWSM_DIFF(wv, qv, use_vf, v), zz = AWSM_DIFF(wl, qv, use_vf, z);
            const float det = uh * vv - vh * uv;
            if (fabsf(det) > kDetMin) {
                const float su = (zh * vv - zz * vh) / det, sv = (zz * uh - zh * uv) / det;
                if (fabsf(su) < INFINITY && fabsf(sv) < INFINITY) {      // (false for a NaN too)
                    zu = fminf(fmaxf(su, -a.max_slope), a.max_slope);
                    zv = fminf(fmaxf(sv, -a.max_slope), a.max_slope);
                }
            }
        }
        // 7: the taps
        const int R = min(max(a.pcf_radius, 0), kMaxRadius), Sm = (int)a.map_size;
        const int iu = (int)floorf(u), iv = (int)floorf(v);
        const float tb = a.bias + a.slope_bias * (fabsf(zu) + fabsf(zv));
        int lit = 0;
        for (int dy = -R; dy <= R; dy++) {
            const int ty = min(max(iv + dy, 0), Sm - 1);
            const float cv = ((float)(iv + dy) + 0.5f) - v;
            for (int dx = -R; dx <= R; dx++) {
                const int tx = min(max(iu + dx, 0), Sm - 1);
                const float cu = ((float)(iu + dx) + 0.5f) - u;
                const float zr = ((z + zu * cu) + zv * cv) - tb;
                const uint32_t hi = a.map[((size_t)ty * a.map_size + tx) * 2 + 1];      // a key's depth word; all ones only in the "no hit" key (a depth is in [0, 1])
                lit += (hi == 0xFFFFFFFFu || __uint_as_float(hi) >= zr) ? 1 : 0;
            }
        }
        V = (float)lit / (float)((2 * R + 1) * (2 * R + 1));
    }
#undef AWSM_DIFF
    // 8: into the opaque image
    const float m = 1.0f - (a.strength * g) * (1.0f - V);
    a.visibility[p] = V; a.multiplier[p] = m;
    const uint2 c16 = a.out16[p];
    a.out16[p] = make_uint2(mul_f2h(h2f(c16.x & 0xFFFFu), m) | (mul_f2h(h2f(c16.x >> 16), m) << 16), mul_f2h(h2f(c16.y & 0xFFFFu), m) | (c16.y & 0xFFFF0000u));
    if (a.out32) {
        float4 c = a.out32[p];
        c.x = c.x * m; c.y = c.y * m; c.z = c.z * m;
        a.out32[p] = c;
    }
}

// ---- several views of one light ----
// Step 3 for one point and one view: lp is a view's view_proj, column-major, at a wave-uniform address.
// front: in front of the view and within its depth range, wherever (u, v) lie — what step 6' asks of a neighbour that another view holds
struct LightCoord { float u, v, z; bool inside, front; };
__device__ __forceinline__ LightCoord light_coord(const float* lp, float px, float py, float pz, float Sf) {
    const float q0 = ((lp[0] * px + lp[4] * py) + lp[8] * pz) + lp[12];
    const float q1 = ((lp[1] * px + lp[5] * py) + lp[9] * pz) + lp[13];
    const float q2 = ((lp[2] * px + lp[6] * py) + lp[10] * pz) + lp[14];
    const float q3 = ((lp[3] * px + lp[7] * py) + lp[11] * pz) + lp[15];
    const float l0 = q0 / q3, l1 = q1 / q3;
    LightCoord c;
    c.z = q2 / q3;
    c.u = (l0 * 0.5f + 0.5f) * Sf;
    c.v = (0.5f - l1 * 0.5f) * Sf;
    c.inside = q3 > 0.0f && c.u >= 0.0f && c.u < Sf && c.v >= 0.0f && c.v < Sf && c.z >= 0.0f && c.z <= 1.0f;      // any NaN: false
    c.front = q3 > 0.0f && c.z >= 0.0f && c.z <= 1.0f && fabsf(c.u) < INFINITY && fabsf(c.v) < INFINITY;
    return c;
}

//   k_shadow_resolve_views<S>   k_shadow_resolve with the light's map a stack of n_views layers.  LDS holds {Pw, d, flags} of the tile and its apron;
//                         the light coordinates are formed per pixel, because they depend on the view the pixel takes: the lowest view whose
//                         (u, v) lies M = R + 1 texels inside the layer, else the lowest it is inside of, else none.  The views are walked
//                         wave-uniformly — the loop counter, and with it the address of view i's matrix in the kernel's arguments, is the same in
//                         every lane, so the matrix is read by scalar loads; the lanes that still look for a view take part, and the loop ends
//                         when none is left.  A second walk gives the lanes of view i their two neighbours' coordinates in that view.
template <int S>
__global__ __launch_bounds__(256) void k_shadow_resolve_views(ShadowViewsArgs av) {
    const ShadowArgs& a = av.base;
    if (poisoned(a)) return;
    __shared__ float wx[kWin * kWin], wy[kWin * kWin], wz[kWin * kWin], wd[kWin * kWin];
    __shared__ unsigned char wf[kWin * kWin];
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    const float* ip = a.camera + 48;      // inv_view_proj, column-major
    const float sx2 = 2.0f / (float)W, sy2 = 2.0f / (float)H, Sf = (float)a.map_size;
    // 1, 2: depth and world position of every window cell inside the image
    for (int i = (int)threadIdx.x; i < kWin * kWin; i += 256) {
        const int cx = x0 - 1 + i % kWin, cy = y0 - 1 + i / kWin;
        float px = 0.0f, py = 0.0f, pz = 0.0f, d = 0.0f;
        unsigned flags = 0u;
        if (cx >= 0 && cx < W && cy >= 0 && cy < H) {
            const size_t p = (size_t)cy * a.width + cx;
            bool hit = false;
#pragma unroll
            for (int s = 0; s < S; s++) {
                const unsigned long long k = a.vis[p * S + s];
                if (k != ~0ull) { const float ds = __uint_as_float((uint32_t)(k >> 32)); d = hit ? fminf(d, ds) : ds; hit = true; }
            }
            if (hit) {
                const float nx = ((float)cx + 0.5f) * sx2 - 1.0f;
                const float ny = 1.0f - ((float)cy + 0.5f) * sy2;
                const float c0 = ((ip[0] * nx + ip[4] * ny) + ip[8] * d) + ip[12];
                const float c1 = ((ip[1] * nx + ip[5] * ny) + ip[9] * d) + ip[13];
                const float c2 = ((ip[2] * nx + ip[6] * ny) + ip[10] * d) + ip[14];
                const float c3 = ((ip[3] * nx + ip[7] * ny) + ip[11] * d) + ip[15];
                px = c0 / c3; py = c1 / c3; pz = c2 / c3;
                flags = kHit;
            } else d = 0.0f;
        }
        wx[i] = px; wy[i] = py; wz[i] = pz; wd[i] = d; wf[i] = (unsigned char)flags;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const int li = (ly + 1) * kWin + lx + 1;
    const size_t p = (size_t)y * a.width + x;
    if (!(wf[li] & kHit)) { a.visibility[p] = 1.0f; a.multiplier[p] = 1.0f; av.view[p] = (unsigned char)kNoView; return; }
    const float Px = wx[li], Py = wy[li], Pz = wz[li], d = wd[li];
    // 4: one neighbour along each image axis — inside the image and hit, the nearer in depth, the +1 one on a tie
    const bool hf = x + 1 < W && (wf[li + 1] & kHit), hb = x - 1 >= 0 && (wf[li - 1] & kHit);
    const bool vf = y + 1 < H && (wf[li + kWin] & kHit), vb = y - 1 >= 0 && (wf[li - kWin] & kHit);
    const bool use_hf = hf && (!hb || fabsf(wd[li + 1] - d) <= fabsf(wd[li - 1] - d));
    const bool use_vf = vf && (!vb || fabsf(wd[li + kWin] - d) <= fabsf(wd[li - kWin] - d));
    const int qh = use_hf ? li + 1 : li - 1, qv = use_vf ? li + kWin : li - kWin;
    const bool has_h = hf || hb, has_v = vf || vb;
    // (a neighbour that does not exist names a cell of the window all the same: the pixel is never on the window's rim)
    const float Hx = wx[qh], Hy = wy[qh], Hz = wz[qh], Vx = wx[qv], Vy = wy[qv], Vz = wz[qv];
#define AWSM_DIFF(q, fwd, centre) ((fwd) ? ((q) - (centre)) : ((centre) - (q)))
    const float hx = AWSM_DIFF(Hx, use_hf, Px), hy = AWSM_DIFF(Hy, use_hf, Py), hz = AWSM_DIFF(Hz, use_hf, Pz);
    const float vx = AWSM_DIFF(Vx, use_vf, Px), vy = AWSM_DIFF(Vy, use_vf, Py), vz = AWSM_DIFF(Vz, use_vf, Pz);
    // 5: normal and facing
    float nx = hy * vz - hz * vy, ny = hz * vx - hx * vz, nz = hx * vy - hy * vx;
    const float* cam = a.camera + 96;
    const float ex = cam[0] - Px, ey = cam[1] - Py, ez = cam[2] - Pz;
    if ((nx * ex + ny * ey) + nz * ez < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    const float nn = (nx * nx + ny * ny) + nz * nz;
    const float ln = sqrtf(nn);
    nx = nx / ln; ny = ny / ln; nz = nz / ln;
    float Lx = a.light[0], Ly = a.light[1], Lz = a.light[2];
    if (a.light[3] != 0.0f) {
        Lx = Lx - Px; Ly = Ly - Py; Lz = Lz - Pz;
        const float ll = sqrtf((Lx * Lx + Ly * Ly) + Lz * Lz);
        Lx = Lx / ll; Ly = Ly / ll; Lz = Lz / ll;
    }
    const float cos_t = (nx * Lx + ny * Ly) + nz * Lz;
    float g = 1.0f;
    if (has_h && has_v && nn > 0.0f) g = cos_t > 0.0f ? fminf(1.0f, cos_t / a.facing_fade) : 0.0f;
    // 3': the pixel's view.  (u, v, z) end up those of the view taken: a deep view's replace the first inside view's, and nothing replaces a deep view's
    const int R = min(max(a.pcf_radius, 0), kMaxRadius), Sm = (int)a.map_size;
    const int n_views = min((int)av.n_views, kMaxViews);
    const float M = (float)(R + 1), top = Sf - M;
    unsigned k = kNoView, kin = kNoView;
    float u = 0.0f, v = 0.0f, z = 0.0f;
    for (int i = 0; i < n_views; i++) {
        const bool looking = k == kNoView;
        if (!__any(looking)) break;
        if (looking) {
            const LightCoord c = light_coord(av.view_proj[i], Px, Py, Pz, Sf);
            const bool deep = c.inside && c.u >= M && c.u < top && c.v >= M && c.v < top;
            if (c.inside && (deep || kin == kNoView)) { u = c.u; v = c.v; z = c.z; }
            if (c.inside && kin == kNoView) kin = (unsigned)i;
            if (deep) k = (unsigned)i;
        }
    }
    if (k == kNoView) k = kin;
    float V = 1.0f;
    if (k != kNoView) {
        // 6': the receiver plane's depth slope per texel, the neighbours' coordinates taken in the pixel's view
        float zu = 0.0f, zv = 0.0f;
        if (has_h && has_v) {
            LightCoord ch, cv;
            ch.u = ch.v = ch.z = cv.u = cv.v = cv.z = 0.0f; ch.inside = cv.inside = ch.front = cv.front = false;
            for (int i = 0; i < n_views; i++)
                if (k == (unsigned)i) { ch = light_coord(av.view_proj[i], Hx, Hy, Hz, Sf); cv = light_coord(av.view_proj[i], Vx, Vy, Vz, Sf); }
            // a neighbour past the border of view k serves all the same when another view holds it (a cube's next face, the next cascade) and it
            // lies in front of view k: the plane is the surface's, not the layer's.  Few lanes come here — a third walk, skipped by the others
            bool serves_h = ch.inside, serves_v = cv.inside;
            const bool ask_h = !ch.inside && ch.front, ask_v = !cv.inside && cv.front;
            if (ask_h || ask_v) {
                for (int i = 0; i < n_views; i++) {
                    if (k == (unsigned)i) continue;
                    if (ask_h && !serves_h) serves_h = light_coord(av.view_proj[i], Hx, Hy, Hz, Sf).inside;
                    if (ask_v && !serves_v) serves_v = light_coord(av.view_proj[i], Vx, Vy, Vz, Sf).inside;
                }
            }
            if (serves_h && serves_v) {
                const float uh = AWSM_DIFF(ch.u, use_hf, u), vh = AWSM_DIFF(ch.v, use_hf, v), zh = AWSM_DIFF(ch.z, use_hf, z);
                const float uv = AWSM_DIFF(cv.u, use_vf, u), vv = AWSM_DIFF(cv.v, use_vf, v), zz = AWSM_DIFF(cv.z, use_vf, z);
                const float det = uh * vv - vh * uv;
                if (fabsf(det) > kDetMin) {
                    const float su = (zh * vv - zz * vh) / det, sv = (zz * uh - zh * uv) / det;
                    if (fabsf(su) < INFINITY && fabsf(sv) < INFINITY) {      // (false for a NaN too)
                        zu = fminf(fmaxf(su, -a.max_slope), a.max_slope);
                        zv = fminf(fmaxf(sv, -a.max_slope), a.max_slope);
                    }
                }
            }
        }
        // 7': the taps, from the view's layer
        const uint32_t* layer = a.map + (size_t)k * a.map_size * a.map_size * 2;
        const int iu = (int)floorf(u), iv = (int)floorf(v);
        const float tb = a.bias + a.slope_bias * (fabsf(zu) + fabsf(zv));
        int lit = 0;
        for (int dy = -R; dy <= R; dy++) {
            const int ty = min(max(iv + dy, 0), Sm - 1);
            const float cv = ((float)(iv + dy) + 0.5f) - v;
            for (int dx = -R; dx <= R; dx++) {
                const int tx = min(max(iu + dx, 0), Sm - 1);
                const float cu = ((float)(iu + dx) + 0.5f) - u;
                const float zr = ((z + zu * cu) + zv * cv) - tb;
                const uint32_t hi = layer[((size_t)ty * a.map_size + tx) * 2 + 1];
                lit += (hi == 0xFFFFFFFFu || __uint_as_float(hi) >= zr) ? 1 : 0;
            }
        }
        V = (float)lit / (float)((2 * R + 1) * (2 * R + 1));
    }
#undef AWSM_DIFF
    // 8: into the opaque image
    const float m = 1.0f - (a.strength * g) * (1.0f - V);
    a.visibility[p] = V; a.multiplier[p] = m; av.view[p] = (unsigned char)k;
    const uint2 c16 = a.out16[p];
    a.out16[p] = make_uint2(mul_f2h(h2f(c16.x & 0xFFFFu), m) | (mul_f2h(h2f(c16.x >> 16), m) << 16), mul_f2h(h2f(c16.y & 0xFFFFu), m) | (c16.y & 0xFFFF0000u));
    if (a.out32) {
        float4 c = a.out32[p];
        c.x = c.x * m; c.y = c.y * m; c.z = c.z * m;
        a.out32[p] = c;
    }
}

}  // namespace shadow
}  // namespace awsm

using awsm::ShadowArgs;
using awsm::ShadowViewsArgs;
static_assert(offsetof(ShadowViewsArgs, base) == 0 && awsm::shadow::kMaxViews == AWSM_SHADOW_MAX_VIEWS, "the launch record leads with k_shadow_resolve's arguments");

// msaa: 1 or 4 samples per pixel in args->vis.  args: the leading member of a ShadowViewsArgs (frame_params.hpp) — with views, the whole record goes
// to k_shadow_resolve_views; without, k_shadow_resolve receives the leading member alone.
extern "C" void awsm_launch_shadow_resolve(const ShadowArgs* args, uint32_t msaa, hipStream_t s) {
    const ShadowArgs a = *args;
    if (!a.width || !a.height || !a.map_size) return;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    const ShadowViewsArgs* views = reinterpret_cast<const ShadowViewsArgs*>(args);
    if (views->n_views) {
        if (msaa == 4) awsm::shadow::k_shadow_resolve_views<4><<<grid, block, 0, s>>>(*views);
        else awsm::shadow::k_shadow_resolve_views<1><<<grid, block, 0, s>>>(*views);
        return;
    }
    if (msaa == 4) awsm::shadow::k_shadow_resolve<4><<<grid, block, 0, s>>>(a);
    else awsm::shadow::k_shadow_resolve<1><<<grid, block, 0, s>>>(a);
}
