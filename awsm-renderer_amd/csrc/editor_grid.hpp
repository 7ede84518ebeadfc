// editor_grid.hpp — the editor's ground grid (crates/editor/src/grid/shaders/grid.wgsl:100-231), a built-in of the world transparent pass.
// STRICT from the first line to the last (DESIGN.md "Editor grid"): IEEE binary32, one rounding per operation, no contraction, `/` is IEEE
// division, whatever the including file set before — the fragment, its quad derivatives and the blend step are held to exact bits against
// tests/grid_reference.py.  The shader has no transcendental: + - * / floor abs min and comparisons.
#pragma once
#include "frame_params.hpp"
#include "device_math.hpp"

#pragma clang fp contract(off)

namespace awsm {

// EditorGridDev::p, the 20 floats of AwsmEditorGrid behind struct_size
enum { kGridBackground = 0, kGridMinor = 4, kGridMajor = 8, kGridZAxis = 12, kGridAlphaAxis = 15, kGridXAxis = 16, kGridDepthEpsilon = 19 };

struct GridHit { f3 world_pos; float ray_dir_y, t; };
struct GridFragment { f4 color; float depth; bool kept; };

// The camera block by wave-uniform loads: the address does not depend on the lane, the block is not written while a frame that reads it runs.
AWSM_DI float grid_cam(const uint8_t* cam, uint32_t byte) { return *(const __attribute__((address_space(4))) float*)(cam + byte); }
AWSM_DI f4 grid_cam4(const uint8_t* cam, uint32_t byte) { return {grid_cam(cam, byte), grid_cam(cam, byte + 4u), grid_cam(cam, byte + 8u), grid_cam(cam, byte + 12u)}; }
AWSM_DI m4 grid_cam_m4(const uint8_t* cam, uint32_t byte) { m4 m; m.c[0] = grid_cam4(cam, byte); m.c[1] = grid_cam4(cam, byte + 16u); m.c[2] = grid_cam4(cam, byte + 32u); m.c[3] = grid_cam4(cam, byte + 48u); return m; }
AWSM_DI bool grid_is_ortho(const uint8_t* cam) { return grid_cam(cam, 64u + 60u) > 0.9f; }      // grid.wgsl:114

// grid.wgsl:102-156 for the pixel (px, py) of a W x H frame, inside the frame or not: where its camera ray meets the plane y = 0
AWSM_DI GridHit grid_hit(const uint8_t* cam, bool is_ortho, float W, float H, int px, int py) {
    const float nx = (((float)px + 0.5f) * 2.0f) / W - 1.0f, ny = 1.0f - (((float)py + 0.5f) * 2.0f) / H;
    f3 origin, dir;
    if (is_ortho) {
        const m4 inv_view_proj = grid_cam_m4(cam, 192u);
        const f4 nh = mul(inv_view_proj, {nx, ny, 0.0f, 1.0f}), fh = mul(inv_view_proj, {nx, ny, 1.0f, 1.0f});
        const f3 world_near = {nh.x / nh.w, nh.y / nh.w, nh.z / nh.w}, world_far = {fh.x / fh.w, fh.y / fh.w, fh.z / fh.w};
        origin = world_near;
        dir = world_far - world_near;                                   // not normalised (:128-129)
    } else {
        const float ux = (nx + 1.0f) * 0.5f, uy = (ny + 1.0f) * 0.5f;
        const f4 r0 = grid_cam4(cam, 416u), r1 = grid_cam4(cam, 432u), r2 = grid_cam4(cam, 448u), r3 = grid_cam4(cam, 464u);
        const f3 ray_bottom = mix3(mk3(r0.x, r0.y, r0.z), mk3(r1.x, r1.y, r1.z), ux), ray_top = mix3(mk3(r2.x, r2.y, r2.z), mk3(r3.x, r3.y, r3.z), ux);
        const f3 view_ray = mix3(ray_bottom, ray_top, uy);
        const f4 c0 = grid_cam4(cam, 320u), c1 = grid_cam4(cam, 336u), c2 = grid_cam4(cam, 352u);
        m3 rot; rot.c[0] = {c0.x, c0.y, c0.z}; rot.c[1] = {c1.x, c1.y, c1.z}; rot.c[2] = {c2.x, c2.y, c2.z};
        origin = {grid_cam(cam, 384u), grid_cam(cam, 388u), grid_cam(cam, 392u)};
        dir = mul(rot, view_ray);
    }
    GridHit h;
    h.ray_dir_y = dir.y;
    h.t = (0.0f - origin.y) / dir.y;
    h.world_pos = origin + dir * h.t;
    return h;
}

AWSM_DI float grid_fract(float x) { return x - floorf(x); }
// (1 - min(distance in pixels, 1)) * alpha (:179-192); fminf drops a NaN distance (0 / 0 on a line with no derivative) for the 1
AWSM_DI float grid_line_alpha(float dist, float alpha) { return (1.0f - fminf(dist, 1.0f)) * alpha; }

// The fragment of pixel (px, py).  fwidth is this repository's: the quad partners px ^ 1 and py ^ 1, each evaluated in full, before any branch.
AWSM_DI GridFragment grid_fragment(const EditorGridDev& g, uint32_t width, uint32_t height, int px, int py) {
    const uint8_t* cam = g.camera;
    const f4 background = {g.p[kGridBackground], g.p[kGridBackground + 1], g.p[kGridBackground + 2], g.p[kGridBackground + 3]};
    const f4 minor = {g.p[kGridMinor], g.p[kGridMinor + 1], g.p[kGridMinor + 2], g.p[kGridMinor + 3]}, major = {g.p[kGridMajor], g.p[kGridMajor + 1], g.p[kGridMajor + 2], g.p[kGridMajor + 3]};
    const f4 z_axis = {g.p[kGridZAxis], g.p[kGridZAxis + 1], g.p[kGridZAxis + 2], g.p[kGridAlphaAxis]}, x_axis = {g.p[kGridXAxis], g.p[kGridXAxis + 1], g.p[kGridXAxis + 2], g.p[kGridAlphaAxis]};
    const float depth_epsilon = g.p[kGridDepthEpsilon];
    const float W = (float)width, H = (float)height;
    const bool is_ortho = grid_is_ortho(cam);
    const GridHit me = grid_hit(cam, is_ortho, W, H, px, py), hx = grid_hit(cam, is_ortho, W, H, px ^ 1, py), hy = grid_hit(cam, is_ortho, W, H, px, py ^ 1);
    const float cx = me.world_pos.x, cz = me.world_pos.z;
    const float dx = fabsf(hx.world_pos.x - cx) + fabsf(hy.world_pos.x - cx), dz = fabsf(hx.world_pos.z - cz) + fabsf(hy.world_pos.z - cz);
    GridFragment o;
    o.color = {0.0f, 0.0f, 0.0f, 0.0f}; o.depth = 0.0f;
    o.kept = !(fabsf(me.ray_dir_y) < 0.001f || (!is_ortho && me.t < 0.0f));                 // :163-170
    if (!o.kept) return o;
    const float minor_alpha = grid_line_alpha(fminf(fabsf(grid_fract(cx - 0.5f) - 0.5f) / dx, fabsf(grid_fract(cz - 0.5f) - 0.5f) / dz), minor.w);
    const float major_alpha = grid_line_alpha(fminf(fabsf(grid_fract(cx / 10.0f - 0.5f) - 0.5f) / (dx / 10.0f), fabsf(grid_fract(cz / 10.0f - 0.5f) - 0.5f) / (dz / 10.0f)), major.w);
    const float x_axis_alpha = grid_line_alpha(fabsf(cz) / dz, x_axis.w), z_axis_alpha = grid_line_alpha(fabsf(cx) / dx, z_axis.w);
    // :195-217, later wins.  Selects between the five colours, each read where every lane reads it: a read under the lane's own condition
    // becomes one read at a per-lane index, and the record then lives in scratch.
    o.color = background;
    if (minor_alpha > 0.01f) o.color = {minor.x, minor.y, minor.z, minor_alpha};
    if (major_alpha > 0.01f) o.color = {major.x, major.y, major.z, major_alpha};
    if (z_axis_alpha > 0.01f) o.color = {z_axis.x, z_axis.y, z_axis.z, z_axis_alpha};
    if (x_axis_alpha > 0.01f) o.color = {x_axis.x, x_axis.y, x_axis.z, x_axis_alpha};
    const f4 view_pos = mul(grid_cam_m4(cam, 0u), {me.world_pos.x, me.world_pos.y, me.world_pos.z, 1.0f});
    const f4 clip_pos = mul(grid_cam_m4(cam, 64u), view_pos);
    o.depth = fminf(fmaxf(clip_pos.z / clip_pos.w + depth_epsilon, 0.0f), 1.0f);  // :219-225
    return o;
}

// SrcAlpha / OneMinusSrcAlpha into the RGBA16F target (pipelines.rs): the two products, their sum, one rounding to f16
AWSM_DI void grid_blend(const f4& src, float (&dst)[4]) {
    const float a = src.w, om = 1.0f - a;
    dst[0] = round_f16(src.x * a + dst[0] * om); dst[1] = round_f16(src.y * a + dst[1] * om);
    dst[2] = round_f16(src.z * a + dst[2] * om); dst[3] = round_f16(a + dst[3] * om);
}

}  // namespace awsm
