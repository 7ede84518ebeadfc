// kernels_ssao.hip — screen-space ambient occlusion from the geometry pass's depth, multiplied into the opaque image (gfx950).
//
// The contract these kernels follow, and tests/ssao_reference.py with them operation for operation: f32 throughout with nothing fused
// (-ffp-contract=off, Makefile), only + - * / and sqrt in their IEEE forms, sums in loop order, coordinates outside the image clamped to its edge.
// The device is held to the restatement's exact bits.
//
//   k_ssao_ao<S>     per 16x16 tile: the view positions of the tile and a 16-pixel apron (the largest sampling radius) are formed once from the
//                    world keys' depth (the least of the S samples) and staged in LDS, 48 x 48 x {x, y, z, hit}; every pixel then takes its
//                    normal from its neighbours' positions and its twelve taps from LDS.  Writes A (raw) and view z per pixel.
//   k_ssao_apply     per 16x16 tile: A and view z of the tile and a two-pixel apron staged in LDS, the 5x5 depth-aware mean, then
//                    rgb *= 1 - strength (1 - A') on the RGBA16F opaque image (and the f32 parity tap) where the pixel was hit.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include "frame_params.hpp"
#include "ssao.hpp"
#include "launch.hpp"

namespace awsm {
namespace ssao {

// a frame whose hand-off gate timed out is dropped whole (frame_params.hpp: frame_poisoned); wave-uniform
__device__ __forceinline__ bool poisoned(const SsaoArgs& a) { return a.poison != nullptr && *a.poison == a.frame_serial; }
__device__ __forceinline__ float h2f(uint32_t h) { return __half2float(__ushort_as_half((unsigned short)h)); }
__device__ __forceinline__ uint32_t f2h(float v) { return (uint32_t)__half_as_ushort(__float2half_rn(v)); }
// f16_rne(f32(stored half) * m) rounds twice, to f32 and then to f16.  Left to itself the compiler selects v_fma_mixlo_f16 for it — the exact product
// rounded once, to f16 — which differs where the f32 product lands on an f16 tie; the empty asm keeps the f32 product a value of its own.
__device__ __forceinline__ uint32_t mul_f2h(float h, float m) { float v = h * m; asm volatile("" : "+v"(v)); return f2h(v); }

template <int S>
__global__ __launch_bounds__(256) void k_ssao_ao(SsaoArgs a) {
    if (poisoned(a)) return;
    __shared__ float wx[kWin * kWin], wy[kWin * kWin], wz[kWin * kWin];
    __shared__ unsigned char wh[kWin * kWin];
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    const float* ip = a.camera + 64;      // inv_proj, column-major
    const float sx2 = 2.0f / (float)W, sy2 = 2.0f / (float)H;
    // 1 + 2: depth and view position of every window cell inside the image (no tap and no neighbour ever names a cell outside it)
    for (int i = (int)threadIdx.x; i < kWin * kWin; i += 256) {
        const int cx = x0 - kRMax + i % kWin, cy = y0 - kRMax + i / kWin;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        bool hit = false;
        if (cx >= 0 && cx < W && cy >= 0 && cy < H) {
            const size_t p = (size_t)cy * a.width + cx;
            float d = 0.0f;
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
            }
        }
        wx[i] = px; wy[i] = py; wz[i] = pz; wh[i] = hit ? 1 : 0;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const int li = (ly + kRMax) * kWin + lx + kRMax;
    const size_t p = (size_t)y * a.width + x;
    const bool hit = wh[li] != 0;
    const float Px = wx[li], Py = wy[li], Pz = wz[li];
    a.view_z[p] = hit ? Pz : __uint_as_float(0x7FC00000u);
    float A = 1.0f;
    if (hit) {
        // 3: the normal from the positions of the four neighbours
        const bool hf = x + 1 < W && wh[li + 1], hb = x - 1 >= 0 && wh[li - 1];
        const bool vf = y + 1 < H && wh[li + kWin], vb = y - 1 >= 0 && wh[li - kWin];
        const float hfx = wx[li + 1] - Px, hfy = wy[li + 1] - Py, hfz = wz[li + 1] - Pz;
        const float hbx = Px - wx[li - 1], hby = Py - wy[li - 1], hbz = Pz - wz[li - 1];
        const float vfx = wx[li + kWin] - Px, vfy = wy[li + kWin] - Py, vfz = wz[li + kWin] - Pz;
        const float vbx = Px - wx[li - kWin], vby = Py - wy[li - kWin], vbz = Pz - wz[li - kWin];
        const bool use_hf = hf && (!hb || fabsf(hfz) <= fabsf(hbz)), use_vf = vf && (!vb || fabsf(vfz) <= fabsf(vbz));
        const float hx = use_hf ? hfx : hbx, hy = use_hf ? hfy : hby, hz = use_hf ? hfz : hbz;
        const float vx = use_vf ? vfx : vbx, vy = use_vf ? vfy : vby, vz = use_vf ? vfz : vbz;
        float nx = hy * vz - hz * vy, ny = hz * vx - hx * vz, nz = hx * vy - hy * vx;
        if (nz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        const float nn = (nx * nx + ny * ny) + nz * nz;
        const float ln = sqrtf(nn);      // IEEE (-fhip-fp32-correctly-rounded-divide-sqrt, the default); __fsqrt_rn is the native approximation here
        nx = nx / ln; ny = ny / ln; nz = nz / ln;
        // 4: the radius in pixels
        const float* pr = a.camera + 16;      // proj
        const float cw = ((pr[3] * Px + pr[7] * Py) + pr[11] * Pz) + pr[15];
        float r = ((a.radius * fabsf(pr[5])) * (0.5f * (float)H)) / cw;
        if ((hf || hb) && (vf || vb) && !(nn == 0.0f) && r >= 1.0f) {
            r = fminf(r, (float)kRMax);
            // 5 + 6: the taps
            const float rc = kRotation[(y & 3) * 4 + (x & 3)][0], rs = kRotation[(y & 3) * 4 + (x & 3)][1];
            const float rr = a.radius * a.radius, br = a.bias * a.radius, eps = (1e-4f * a.radius) * a.radius;
            float total = 0.0f;
#pragma unroll
            for (int i = 0; i < kTaps; i++) {
                const float tx = kSpiral[i][0], ty = kSpiral[i][1];
                const float ox = (rc * tx - rs * ty) * r, oy = (rs * tx + rc * ty) * r;
                // |rot t| r < 16, so the rounded offset is at most kRMax: the clamp changes nothing and keeps the index inside the window whatever happens
                const int sx = min(max((int)floorf(ox + 0.5f), -kRMax), kRMax), sy = min(max((int)floorf(oy + 0.5f), -kRMax), kRMax);
                const int qx = min(max(x + sx, 0), W - 1), qy = min(max(y + sy, 0), H - 1);
                const int qi = (qy - (y0 - kRMax)) * kWin + (qx - (x0 - kRMax));
                if ((qx == x && qy == y) || !wh[qi]) continue;
                const float dx = wx[qi] - Px, dy = wy[qi] - Py, dz = wz[qi] - Pz;
                const float vv = (dx * dx + dy * dy) + dz * dz;
                const float vn = (dx * nx + dy * ny) + dz * nz;
                total = total + ((fmaxf(0.0f, vn - br) * fmaxf(0.0f, 1.0f - vv / rr)) * a.radius) / (vv + eps);
            }
            A = fmaxf(0.0f, 1.0f - (a.intensity * total) / (float)kTaps);
        }
    }
    a.ao_raw[p] = A;
}

__global__ __launch_bounds__(256) void k_ssao_apply(SsaoArgs a) {
    if (poisoned(a)) return;
    __shared__ float sa[kBlurWin * kBlurWin], sz[kBlurWin * kBlurWin];      // view z is NaN where nothing was hit
    const int W = (int)a.width, H = (int)a.height;
    const int lx = (int)(threadIdx.x & 15u), ly = (int)(threadIdx.x >> 4);
    const int x0 = (int)blockIdx.x * kTile, y0 = (int)blockIdx.y * kTile;
    const int x = x0 + lx, y = y0 + ly;
    for (int i = (int)threadIdx.x; i < kBlurWin * kBlurWin; i += 256) {
        const int gx = min(max(x0 - kBlur + i % kBlurWin, 0), W - 1), gy = min(max(y0 - kBlur + i / kBlurWin, 0), H - 1);
        const size_t g = (size_t)gy * a.width + gx;
        sa[i] = a.ao_raw[g]; sz[i] = a.view_z[g];
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * a.width + x;
    const float z = sz[(ly + kBlur) * kBlurWin + lx + kBlur];
    const bool hit = z == z;
    // 7: the 5x5 depth-aware mean, (dy, dx) order
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int dy = -kBlur; dy <= kBlur; dy++) {
#pragma unroll
        for (int dx = -kBlur; dx <= kBlur; dx++) {
            // the staged cell of the clamped neighbour: clamp in image coordinates, then into the window
            const int qx = min(max(x + dx, 0), W - 1), qy = min(max(y + dy, 0), H - 1);
            const int qi = (qy - (y0 - kBlur)) * kBlurWin + (qx - (x0 - kBlur));
            const float zq = sz[qi];
            const float w = (dy == 0 && dx == 0) ? 1.0f : (zq == zq ? fmaxf(0.0f, 1.0f - fabsf(zq - z) / a.radius) : 0.0f);
            num = num + w * sa[qi];
            den = den + w;
        }
    }
    const float As = hit ? num / den : 1.0f;
    a.ao_smoothed[p] = As;
    if (!hit) return;
    // 8: into the opaque image
    const float m = 1.0f - a.strength * (1.0f - As);
    const uint2 v = a.out16[p];
    a.out16[p] = make_uint2(mul_f2h(h2f(v.x & 0xFFFFu), m) | (mul_f2h(h2f(v.x >> 16), m) << 16), mul_f2h(h2f(v.y & 0xFFFFu), m) | (v.y & 0xFFFF0000u));
    if (a.out32) {
        float4 c = a.out32[p];
        c.x = c.x * m; c.y = c.y * m; c.z = c.z * m;
        a.out32[p] = c;
    }
}

}  // namespace ssao
}  // namespace awsm

using awsm::SsaoArgs;

// msaa: 1 or 4 samples per pixel in args->vis
extern "C" void awsm_launch_ssao(const SsaoArgs* args, uint32_t msaa, hipStream_t s) {
    const SsaoArgs a = *args;
    if (!a.width || !a.height) return;
    const dim3 grid((a.width + 15) / 16, (a.height + 15) / 16), block(256);
    if (msaa == 4) awsm::ssao::k_ssao_ao<4><<<grid, block, 0, s>>>(a);
    else awsm::ssao::k_ssao_ao<1><<<grid, block, 0, s>>>(a);
    awsm::ssao::k_ssao_apply<<<grid, block, 0, s>>>(a);
}
