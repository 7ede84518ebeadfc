// kernels_taa.hip — temporal anti-aliasing: the history resolve in front of the post pass (gfx950).
//
// The contract these kernels follow, and tests/taa_reference.py with them operation for operation: f32 throughout with nothing fused
// (-ffp-contract=off, Makefile), only + - * / floor min max, sums in the written order, coordinates outside the image clamped to its edge, one
// rounding to f16 (RNE) at the store.  The device is held to the restatement's exact bits.
//
//   k_taa_resolve<S>  per 16x16 tile: the current image of the tile and a one-texel apron is staged in LDS (18 x 18: the raw texel, and r g b
//                     unpacked once); every pixel then reprojects itself with the depth of its world key (the least of the S samples, 1.0 where
//                     nothing was hit), takes four history taps from global memory, clamps their bilinear mix to the min / max of its 3x3
//                     neighbourhood and mixes it with the current colour.  Where the history is not usable the current texel is copied.
//   k_taa_layers<S>   awsm_hip_read_taa only: the lookup position and the usable flag per pixel, from the same record.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include "frame_params.hpp"
#include "taa.hpp"
#include "launch.hpp"

namespace awsm {
namespace taa {

// a frame whose hand-off gate timed out is dropped whole (frame_params.hpp: frame_poisoned); wave-uniform
__device__ __forceinline__ bool poisoned(const TaaArgs& a) { return a.poison != nullptr && *a.poison == a.frame_serial; }
__device__ __forceinline__ float h2f(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
// the f32 result is a value of its own before it is rounded to f16: no mixed-precision instruction may round the exact sum once (kernels_ssao.hip: mul_f2h)
__device__ __forceinline__ uint32_t f2h(float v) { asm volatile("" : "+v"(v)); return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
__device__ __forceinline__ float key_depth(unsigned long long k) { return k == ~0ull ? 1.0f : __uint_as_float((uint32_t)(k >> 32)); }

template <int S>
__device__ __forceinline__ float pixel_depth(const TaaArgs& a, size_t p) {
    float d = key_depth(a.vis[p * S]);
#pragma unroll
    for (int s = 1; s < S; s++) d = fminf(d, key_depth(a.vis[p * S + s]));
    return d;
}

// (sx, sy): where the pixel was in the history, in texel-index units; returns whether the history may be read there
__device__ __forceinline__ bool lookup(const TaaArgs& a, int x, int y, float d, float& sx, float& sy) {
    const float fW = (float)a.width, fH = (float)a.height;
    const float nx = (((float)x + 0.5f) * (2.0f / fW) - 1.0f) - a.jitter[0];
    const float ny = (1.0f - ((float)y + 0.5f) * (2.0f / fH)) - a.jitter[1];
    const float* R = a.reproject;
    const float qx = ((R[0] * nx + R[4] * ny) + R[8] * d) + R[12];
    const float qy = ((R[1] * nx + R[5] * ny) + R[9] * d) + R[13];
    const float qw = ((R[3] * nx + R[7] * ny) + R[11] * d) + R[15];
    const float vx = qx / qw - nx, vy = qy / qw - ny;
    sx = (float)x + vx * (0.5f * fW);
    sy = (float)y - vy * (0.5f * fH);
    // any NaN: false
    return a.history != nullptr && qw > 0.0f && sx >= -0.5f && sx <= fW - 0.5f && sy >= -0.5f && sy <= fH - 0.5f;
}

template <int S>
__global__ __launch_bounds__(256) void k_taa_resolve(TaaArgs a) {
    if (poisoned(a)) return;
    __shared__ uint2 raw[kWin * kWin];
    __shared__ float wr[kWin * kWin], wg[kWin * kWin], wb[kWin * kWin];
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    // the window, clamped to the image's edge cell by cell: a neighbour outside the image is the edge texel
    for (int i = (int)threadIdx.x; i < kWin * kWin; i += 256) {
        const int gx = min(max(x0 - kApron + i % kWin, 0), W - 1), gy = min(max(y0 - kApron + i / kWin, 0), H - 1);
        const uint2 v = a.cur[(size_t)gy * a.width + gx];
        raw[i] = v;
        wr[i] = h2f(v.x & 0xFFFFu); wg[i] = h2f(v.x >> 16); wb[i] = h2f(v.y & 0xFFFFu);
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * a.width + x;
    const int li = (ly + kApron) * kWin + lx + kApron;
    const uint2 c = raw[li];
    float sx, sy;
    if (!lookup(a, x, y, pixel_depth<S>(a, p), sx, sy)) { a.out[p] = c; return; }
    // the four taps, clamped to the edge: -1 <= ix <= W - 1 here, so every index is inside the image after the clamp
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    const float fx = sx - fx0, fy = sy - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    const int tx0 = min(max(ix, 0), W - 1), tx1 = min(max(ix + 1, 0), W - 1), ty0 = min(max(iy, 0), H - 1), ty1 = min(max(iy + 1, 0), H - 1);
    const uint2 t00 = a.history[(size_t)ty0 * a.width + tx0], t10 = a.history[(size_t)ty0 * a.width + tx1];
    const uint2 t01 = a.history[(size_t)ty1 * a.width + tx0], t11 = a.history[(size_t)ty1 * a.width + tx1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
    float hr = ((h2f(t00.x & 0xFFFFu) * w00 + h2f(t10.x & 0xFFFFu) * w10) + h2f(t01.x & 0xFFFFu) * w01) + h2f(t11.x & 0xFFFFu) * w11;
    float hg = ((h2f(t00.x >> 16) * w00 + h2f(t10.x >> 16) * w10) + h2f(t01.x >> 16) * w01) + h2f(t11.x >> 16) * w11;
    float hb = ((h2f(t00.y & 0xFFFFu) * w00 + h2f(t10.y & 0xFFFFu) * w10) + h2f(t01.y & 0xFFFFu) * w01) + h2f(t11.y & 0xFFFFu) * w11;
    // the 3x3 neighbourhood of the current image, (dy, dx) order
    float nr0 = wr[li - kWin - 1], nr1 = nr0, ng0 = wg[li - kWin - 1], ng1 = ng0, nb0 = wb[li - kWin - 1], nb1 = nb0;
#pragma unroll
    for (int k = 1; k < 9; k++) {
        const int qi = li + (k / 3 - 1) * kWin + (k % 3 - 1);
        nr0 = fminf(nr0, wr[qi]); nr1 = fmaxf(nr1, wr[qi]);
        ng0 = fminf(ng0, wg[qi]); ng1 = fmaxf(ng1, wg[qi]);
        nb0 = fminf(nb0, wb[qi]); nb1 = fmaxf(nb1, wb[qi]);
    }
    hr = fminf(fmaxf(hr, nr0), nr1); hg = fminf(fmaxf(hg, ng0), ng1); hb = fminf(fmaxf(hb, nb0), nb1);
    const float fb = a.feedback, om = 1.0f - fb;
    const uint32_t r = f2h(hr * om + wr[li] * fb), g = f2h(hg * om + wg[li] * fb), b = f2h(hb * om + wb[li] * fb);
    a.out[p] = make_uint2(r | (g << 16), b | (c.y & 0xFFFF0000u));
}

template <int S>
__global__ __launch_bounds__(256) void k_taa_layers(TaaArgs a) {
    const int x = (int)(blockIdx.x * kTile + (threadIdx.x & 15u)), y = (int)(blockIdx.y * kTile + (threadIdx.x >> 4));
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    float sx, sy;
    const bool used = lookup(a, x, y, pixel_depth<S>(a, p), sx, sy);
    a.layer_xy[2 * p] = sx; a.layer_xy[2 * p + 1] = sy;
    a.layer_used[p] = used ? 1 : 0;
}

}  // namespace taa
}  // namespace awsm

using awsm::TaaArgs;

// msaa: 1 or 4 samples per pixel in args->vis
extern "C" void awsm_launch_taa(const TaaArgs* args, uint32_t msaa, hipStream_t s) {
    const TaaArgs a = *args;
    if (!a.width || !a.height) return;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    if (msaa == 4) awsm::taa::k_taa_resolve<4><<<grid, block, 0, s>>>(a);
    else awsm::taa::k_taa_resolve<1><<<grid, block, 0, s>>>(a);
}
extern "C" void awsm_launch_taa_layers(const TaaArgs* args, uint32_t msaa, hipStream_t s) {
    const TaaArgs a = *args;
    if (!a.width || !a.height) return;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    if (msaa == 4) awsm::taa::k_taa_layers<4><<<grid, block, 0, s>>>(a);
    else awsm::taa::k_taa_layers<1><<<grid, block, 0, s>>>(a);
}
