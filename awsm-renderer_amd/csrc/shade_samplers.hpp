// shade_samplers.hpp — the RELAXED helpers (fm::), the 2D-array samplers (level 0 / gradient mips / anisotropic probes), the per-pixel attribute
// context, the BRDF terms and the BRDF-LUT sampler.  From here on a shading unit compiles under contract(fast): the pragma below stays in force in
// the files that include this one, until one of them turns it off again.
#pragma once
#include "frame_params.hpp"
#include "raster_setup.hpp"

namespace awsm {

// ================================================================================================
// RELAXED section: everything downstream of the quantised G-buffer values only has to stay within 1e-4 of the
// oracle (BASELINE.json north_star), so it may contract to FMA and use the hardware reciprocal / rsqrt / exp2 /
// log2 / sin / cos units (each ~1 ulp).  Helpers are re-defined here under contract(fast); the strict ones in
// device_math.hpp keep their own flags even when inlined.
// ================================================================================================
#pragma clang fp contract(fast)
namespace fm {
AWSM_DI float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
AWSM_DI float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
AWSM_DI float fdiv(float a, float b) { return a * rcp(b); }
AWSM_DI float fdot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
AWSM_DI f3 fnormalize(f3 a) { return a * rsq(fdot(a, a)); }
AWSM_DI f3 fsafe_normalize(f3 n) { const float l = fdot(n, n); return l > 0.0f ? n * rsq(l) : mk3(0.0f, 0.0f, 1.0f); }
AWSM_DI float pow5(float x) { const float x2 = x * x; return x2 * x2 * x; }
AWSM_DI float powp(float x, float y) { return x > 0.0f ? __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)) : (x == 0.0f ? (y == 0.0f ? 1.0f : 0.0f) : __builtin_nanf("")); }
AWSM_DI f4 fmul(const m4& m, f4 v) {
    return {m.c[0].x * v.x + m.c[1].x * v.y + m.c[2].x * v.z + m.c[3].x * v.w, m.c[0].y * v.x + m.c[1].y * v.y + m.c[2].y * v.z + m.c[3].y * v.w,
            m.c[0].z * v.x + m.c[1].z * v.y + m.c[2].z * v.z + m.c[3].z * v.w, m.c[0].w * v.x + m.c[1].w * v.y + m.c[2].w * v.z + m.c[3].w * v.w};
}
AWSM_DI f3 fdecode_octahedral(f2 e) {         // math.wgsl:55-67
    const float fx = e.x * 2.0f - 1.0f, fy = e.y * 2.0f - 1.0f;
    f3 n = {fx, fy, (1.0f - fabsf(fx)) - fabsf(fy)};
    const float t = clampf(-n.z, 0.0f, 1.0f);
    n.x += (n.x >= 0.0f) ? -t : t;
    n.y += (n.y >= 0.0f) ? -t : t;
    return fnormalize(n);
}
AWSM_DI TBN funpack_normal_tangent(f4 rgba) {  // math.wgsl:104-116
    TBN r;
    r.N = fdecode_octahedral({rgba.x, rgba.y});
    const float theta = rgba.z * kTau - kPi;
    const float s = (rgba.w >= 0.5f) ? 1.0f : -1.0f;
    f3 tt, tb;
    if (r.N.z < -0.98f) {
        // canonical_tb (math.wgsl:73-84) divides by 1 + N.z: towards N = (0, 0, -1) a one-ulp difference in the decoded normal moves the basis
        // by 6e-8 / (1 + N.z) — percent of a radian in the last degrees — so there the normal and the basis are computed with the oracle's
        // operations (IEEE division and square root, no contraction; decode_octahedral / canonical_tb of the STRICT section).  Found by
        // rendering from random viewpoints (tests/diagnostics/viewpoint_survey.py): surfaces facing -z were off by up to 6e-2 in single pixels.
        r.N = decode_octahedral({rgba.x, rgba.y});
        const TB cb = canonical_tb(r.N);
        tt = cb.t; tb = cb.b;
    } else {
        const float a = rcp(1.0f + r.N.z), bb = (-r.N.x * r.N.y) * a;
        tt = {1.0f - (r.N.x * r.N.x) * a, bb, -r.N.x};
        tb = {bb, 1.0f - (r.N.y * r.N.y) * a, -r.N.y};
    }
    const float c = __ocml_native_cos_f32(theta), sn = __ocml_native_sin_f32(theta);
    r.T = fnormalize(tt * c + tb * sn);
    r.B = fnormalize(cross(r.N, r.T)) * s;
    return r;
}

}  // namespace fm

// ---------------- textures.wgsl ----------------
struct TexInfo {
    bool exists;
    uint32_t array_index, layer_index, uv_set_index, sampler_index, uv_transform_index;
};
AWSM_DI TexInfo tex_load(const uint32_t* __restrict__ m, uint32_t i) {      // textures.wgsl:75-114
    TexInfo t;
    const uint32_t array_and_layer = m[i + 1], uv_and_sampler = m[i + 2], extra = m[i + 3], transform_offset = m[i + 4];
    t.array_index = array_and_layer & 0xFFFu; t.layer_index = array_and_layer >> 12;
    t.uv_set_index = uv_and_sampler & 0xFFu; t.sampler_index = uv_and_sampler >> 8;
    t.exists = (extra & 1u) != 0u;
    t.uv_transform_index = transform_offset / 32u;
    return t;
}

// exact integer wrap without an integer divide: power-of-two sizes use masks, other sizes a float quotient + fix-up
AWSM_DI int mod_floor(int i, int n) {
    if ((n & (n - 1)) == 0) return i & (n - 1);
    int r = i - (int)floorf((float)i * fm::rcp((float)n)) * n;
    if (r < 0) r += n;
    if (r >= n) r -= n;
    return r;
}
AWSM_DI int wrap_index(int i, int n, uint32_t mode) {
    if (mode == 1u) return mod_floor(i, n);
    if (mode == 2u) { const int m = mod_floor(i, 2 * n); return m < n ? m : 2 * n - 1 - m; }
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}
AWSM_DI f4 texel_rgba8(const uint8_t* __restrict__ p) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    const float k = 1.0f / 255.0f;
    return {(float)(u & 255u) * k, (float)((u >> 8) & 255u) * k, (float)((u >> 16) & 255u) * k, (float)(u >> 24) * k};
}
AWSM_DI float safe_floor(float x, float& frac) {
    const float fl = floorf(x);
    if (!(fl >= -1073741824.0f && fl <= 1073741824.0f)) { frac = 0.0f; return 0.0f; }
    frac = x - fl;
    return fl;
}
AWSM_DI f4 lerp4(f4 a, f4 b, float t) { const float s = 1.0f - t; return {a.x * s + b.x * t, a.y * s + b.y * t, a.z * s + b.z * t, a.w * s + b.w * t}; }
// textureSampleLevel(tex, sampler, uv, layer, level) on one level of one layer: DESIGN.md §"Texture sampling".  General
// form: any size, any address mode, nearest or linear.  Out of line (one copy for all call sites); the hot path below
// handles the common sampler inline and only falls back here when some lane of the wavefront needs it.
__device__ __attribute__((noinline)) f4 sample_level_generic(const uint8_t* base, uint32_t width, uint32_t height, uint32_t mode_u, uint32_t mode_v,
                                                             uint32_t linear, float u, float v) {
    const int W = (int)width, H = (int)height;
    float fx, fy;
    if (linear == 0u) {
        const int i = wrap_index((int)safe_floor(u * (float)W, fx), W, mode_u);
        const int j = wrap_index((int)safe_floor(v * (float)H, fy), H, mode_v);
        return texel_rgba8(base + ((size_t)j * W + i) * 4u);
    }
    const float x0f = safe_floor(u * (float)W - 0.5f, fx);
    const float y0f = safe_floor(v * (float)H - 0.5f, fy);
    const int i0 = wrap_index((int)x0f, W, mode_u), i1 = wrap_index((int)x0f + 1, W, mode_u);
    const int j0 = wrap_index((int)y0f, H, mode_v), j1 = wrap_index((int)y0f + 1, H, mode_v);
    const uint8_t* r0 = base + (size_t)j0 * W * 4u;
    const uint8_t* r1 = base + (size_t)j1 * W * 4u;
    const f4 c00 = texel_rgba8(r0 + i0 * 4), c10 = texel_rgba8(r0 + i1 * 4), c01 = texel_rgba8(r1 + i0 * 4), c11 = texel_rgba8(r1 + i1 * 4);
    return lerp4(lerp4(c00, c10, fx), lerp4(c01, c11, fx), fy);
}
// The common sampler (linear, repeat/repeat, power-of-two extent) inline: wrap is a mask, no mode selects, no quotients,
// the two taps of a row in one 8-byte load.
AWSM_DI f4 sample_level_fast(const uint32_t* base, uint32_t W, uint32_t H, float u, float v) {
    float fx, fy;
    const float x0f = safe_floor(u * (float)W - 0.5f, fx);
    const float y0f = safe_floor(v * (float)H - 0.5f, fy);
    const uint32_t xi = (uint32_t)(int)x0f, yi = (uint32_t)(int)y0f;
    const uint32_t i0 = xi & (W - 1u), i1 = (xi + 1u) & (W - 1u);
    const uint32_t r0 = (yi & (H - 1u)) * W, r1 = ((yi + 1u) & (H - 1u)) * W;
    uint32_t t00, t10, t01, t11;
    if (i1 == i0 + 1u) {   // neighbours in memory unless the footprint wraps
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2), aligned(4)));
        const u32x2 p0 = *reinterpret_cast<const u32x2*>(base + r0 + i0), p1 = *reinterpret_cast<const u32x2*>(base + r1 + i0);
        t00 = p0.x; t10 = p0.y; t01 = p1.x; t11 = p1.y;
    } else {
        t00 = base[r0 + i0]; t10 = base[r0 + i1]; t01 = base[r1 + i0]; t11 = base[r1 + i1];
    }
    // bilinear on the raw 0..255 values, one scale by 1/255 at the end
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy;
    const float k = 1.0f / 255.0f;
    f4 r;
    r.x = ((float)(t00 & 255u) * w00 + (float)(t10 & 255u) * w10 + (float)(t01 & 255u) * w01 + (float)(t11 & 255u) * w11) * k;
    r.y = ((float)((t00 >> 8) & 255u) * w00 + (float)((t10 >> 8) & 255u) * w10 + (float)((t01 >> 8) & 255u) * w01 + (float)((t11 >> 8) & 255u) * w11) * k;
    r.z = ((float)((t00 >> 16) & 255u) * w00 + (float)((t10 >> 16) & 255u) * w10 + (float)((t01 >> 16) & 255u) * w01 + (float)((t11 >> 16) & 255u) * w11) * k;
    r.w = ((float)(t00 >> 24) * w00 + (float)(t10 >> 24) * w10 + (float)(t01 >> 24) * w01 + (float)(t11 >> 24) * w11) * k;
    return r;
}

// textureSampleGrad's footprint.  WebGPU leaves level selection and anisotropy to the implementation; the contract here:
//   * max_anisotropy 1 (or a context without AWSM_CFG_ANISOTROPIC — the default, the rule the reference itself documents as "mimics the hardware mip
//     selection", helpers/mipmap.wgsl:419-439): rho = max(|ddx * size|, |ddy * size|), lod = log2(max(rho, 1e-6));
//   * max_anisotropy A > 1 (gltf samplers ask for 16, gltf/populate/material.rs:892-902): N = clamp(rho_max / rho_min, 1, A) — a real number — the
//     level is chosen for rho_max / N, and the footprint is covered by probes along the major axis at t_j = j / N, j = -m..m, m = ceil((N - 1) / 2),
//     each weighted by the part of [-1/2, 1/2] its cell [t_j - 1/2N, t_j + 1/2N] covers (a box filter of the footprint's length sampled at the chosen
//     level's spacing), normalised.  Continuous in N — a probe enters with weight zero — so two implementations that disagree in the last bit of a
//     gradient agree in the colour; N = 1 is the isotropic rule bit for bit.
struct GradFootprint { float lod, n, major_u, major_v; int m; };
AWSM_DI GradFootprint grad_footprint(float dxu, float dxv, float dyu, float dyv, float W, float H, uint32_t max_aniso) {
    const float ax = dxu * W, ay = dxv * H, bx = dyu * W, by = dyv * H;
    const float rx2 = ax * ax + ay * ay, ry2 = bx * bx + by * by;
    const float r2max = fmaxf(rx2, ry2);
    GradFootprint fp;
    fp.lod = 0.5f * __builtin_amdgcn_logf(fmaxf(r2max, 1e-12f));      // log2(max(rho, 1e-6))
    fp.n = 1.0f; fp.major_u = 0.0f; fp.major_v = 0.0f; fp.m = 0;
    if (max_aniso > 1u && r2max > 0.0f) {
        const float r2min = fminf(rx2, ry2), A = (float)min(max_aniso, 16u);
        float nf = r2min * (A * A) <= r2max ? A : __builtin_sqrtf(r2max / r2min);
        nf = fminf(fmaxf(nf, 1.0f), A);
        if (nf > 1.0f) {
            fp.n = nf;
            fp.lod = fp.lod - __builtin_amdgcn_logf(nf);
            fp.m = (int)ceilf((nf - 1.0f) * 0.5f);
            const bool xmajor = rx2 >= ry2;
            fp.major_u = xmajor ? dxu : dyu; fp.major_v = xmajor ? dxv : dyv;
        }
    }
    return fp;
}

// grad_footprint's probes: 2 m + 1 trilinear samples along the major axis, weighted and normalised.  levels_modes: lo | hi << 8 | address mode u << 16 |
// v << 18 | linear << 20.  Out of line, per lane: only pixels with an anisotropic footprint on an AWSM_CFG_ANISOTROPIC context come here.
__device__ __attribute__((noinline)) f4 sample_probes(const uint32_t* texels, const uint32_t* level_off, uint32_t W, uint32_t H, uint32_t layer, uint32_t levels_modes, float f,
                                                      float u, float v, float major_u, float major_v, float nf, int m) {
    const uint32_t lo = levels_modes & 255u, hi = (levels_modes >> 8) & 255u, mode_u = (levels_modes >> 16) & 3u, mode_v = (levels_modes >> 18) & 3u, linear = (levels_modes >> 20) & 1u;
    const float inv_n = 1.0f / nf;
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    float wsum = 0.0f;
    const int n = f > 0.0f ? 2 : 1;
    for (int j = -m; j <= m; j++) {
        const float t = (float)j * inv_n, wp = saturate((0.5f - fabsf(t)) * nf + 0.5f);
        const float pu = u + major_u * t, pv = v + major_v * t;
        for (int k = 0; k < n; k++) {
            const uint32_t level = k ? hi : lo;
            const float w = (k ? f : 1.0f - f) * wp;
            const uint32_t Wl = max(W >> level, 1u), Hl = max(H >> level, 1u);
            const uint32_t* base = texels + level_off[level] + (size_t)layer * Wl * Hl;
            const f4 c = sample_level_generic(reinterpret_cast<const uint8_t*>(base), Wl, Hl, mode_u, mode_v, linear, pu, pv);
            acc = {acc.x + c.x * w, acc.y + c.y * w, acc.z + c.z * w, acc.w + c.w * w};
        }
        wsum += wp;
    }
    const float iw = 1.0f / wsum;
    return {acc.x * iw, acc.y * iw, acc.z * iw, acc.w * iw};
}

// ---------------- per-pixel attribute context ----------------
struct Attr {
    const DevScene* sc;
    const float* ad;          // attribute_data (f32 view)
    uint32_t v0, v1, v2;      // vertex_start of the three corners (floats)
    uint32_t uv_sets_index;
    f3 bary;
    f2 uv0;                   // interpolated TEXCOORD_0, computed once per pixel when a core texture uses it
    bool has_uv0;
    f4 bary_derivs;           // MipmapMode::Gradient: the RGBA16F barycentric_derivatives texel (db0/dx, db0/dy, db1/dx, db1/dy)
    f2 duv0_dx, duv0_dy;      // ... and d(TEXCOORD_0)/d(screen), alongside uv0
};
// texture_uvs.wgsl:64-84 (+ helpers/mipmap.wgsl:113-205 get_uv_derivatives when GRAD: chain rule over the vertex UVs)
template <int GRAD>
AWSM_DI f2 attr_uv(const Attr& a, uint32_t set, f2& ddx, f2& ddy) {
    const uint32_t o = a.uv_sets_index + set * 2u;
    const float x0 = a.ad[a.v0 + o], y0 = a.ad[a.v0 + o + 1], x1 = a.ad[a.v1 + o], y1 = a.ad[a.v1 + o + 1];
    const float x2 = a.ad[a.v2 + o], y2 = a.ad[a.v2 + o + 1];
    if (GRAD) {
        const float dAlphaDx = a.bary_derivs.x, dAlphaDy = a.bary_derivs.y, dBetaDx = a.bary_derivs.z, dBetaDy = a.bary_derivs.w;
        const float dGammaDx = -dAlphaDx - dBetaDx, dGammaDy = -dAlphaDy - dBetaDy;
        ddx = {x0 * dAlphaDx + x1 * dBetaDx + x2 * dGammaDx, y0 * dAlphaDx + y1 * dBetaDx + y2 * dGammaDx};
        ddy = {x0 * dAlphaDy + x1 * dBetaDy + x2 * dGammaDy, y0 * dAlphaDy + y1 * dBetaDy + y2 * dGammaDy};
        const bool tiny = (fabsf(dAlphaDx) + fabsf(dAlphaDy) + fabsf(dBetaDx) + fabsf(dBetaDy)) < 1e-20f;
        const bool ok = (ddx.x == ddx.x) && (ddx.y == ddx.y) && (ddy.x == ddy.x) && (ddy.y == ddy.y);   // NaN guard
        if (tiny || !ok) { ddx = {0.0f, 0.0f}; ddy = {0.0f, 0.0f}; }
    }
    return {interp3_strict(a.bary.x, a.bary.y, a.bary.z, x0, x1, x2), interp3_strict(a.bary.x, a.bary.y, a.bary.z, y0, y1, y2)};
}
// texture_uvs.wgsl:64-187 + textures.wgsl:131-150.  GRAD = MipmapMode::Gradient: textureSampleGrad by the contract the
// reference documents as "mimics the hardware mip selection" (helpers/mipmap.wgsl:419-439): rho = max(|ddx*size|, |ddy*size|),
// lod = log2(max(rho, 1e-6)) clamped to the chain; magnification -> mag filter on level 0; otherwise min filter on
// floor(lod) and floor(lod)+1 blended by the fraction (mipmap filter linear) or round(lod) (nearest).  Isotropic.
template <int GRAD>
AWSM_DI f4 sample_tex(const Attr& a, const TexInfo& t) {
    f2 uv = a.uv0, ddx = a.duv0_dx, ddy = a.duv0_dy;
    if (!(a.has_uv0 && t.uv_set_index == 0u)) uv = attr_uv<GRAD>(a, t.uv_set_index, ddx, ddy);
    const float* tt = reinterpret_cast<const float*>(a.sc->buf[AWSM_BUF_TEXTURE_TRANSFORMS] + (size_t)t.uv_transform_index * 32u);
    const float u = affine2_strict(tt[0], tt[1], tt[4], uv.x, uv.y), v = affine2_strict(tt[2], tt[3], tt[5], uv.x, uv.y);
    if (t.array_index >= a.sc->n_tex || t.sampler_index >= a.sc->n_samplers) return {0.0f, 0.0f, 0.0f, 0.0f};
    const TexArrayDev& arr = a.sc->tex[t.array_index];
    const AwsmSampler& smp = a.sc->samplers[t.sampler_index];
    const uint32_t W = arr.width, H = arr.height, layers = arr.layers;
    const uint8_t* texels = arr.texels;
    if (texels == nullptr || W == 0u || H == 0u || layers == 0u) return {0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t layer = min(t.layer_index, layers - 1u);
    const bool common = smp.address_mode_u == 1u && smp.address_mode_v == 1u && (W & (W - 1u)) == 0u && (H & (H - 1u)) == 0u;
    if (!GRAD) {
        // Hot path taken when ALL lanes of the wavefront qualify (one scalar branch)
        const bool fast = common && smp.mag_filter != 0u;
        if (__builtin_amdgcn_ballot_w64(!fast) != 0ull)
            return sample_level_generic(texels + (size_t)layer * W * H * 4u, W, H, smp.address_mode_u, smp.address_mode_v, smp.mag_filter, u, v);
        return sample_level_fast(reinterpret_cast<const uint32_t*>(texels) + (size_t)layer * W * H, W, H, u, v);
    }
    // ---- level selection ----
    const float dxu = tt[0] * ddx.x + tt[1] * ddx.y, dxv = tt[2] * ddx.x + tt[3] * ddx.y;     // texture_uvs.wgsl:27-35
    const float dyu = tt[0] * ddy.x + tt[1] * ddy.y, dyv = tt[2] * ddy.x + tt[3] * ddy.y;
    GradFootprint fp = grad_footprint(dxu, dxv, dyu, dyv, (float)W, (float)H, (GRAD == 2 && smp.mag_filter != 0u && smp.min_filter != 0u && smp.mipmap_filter != 0u) ? smp.max_anisotropy : 1u);
    const uint32_t levels = max(arr.mips, 1u);
    uint32_t lo = 0u, hi = 0u, linear = smp.mag_filter;
    float f = 0.0f;
    if (fp.lod > 0.0f && levels > 1u) {
        const float lod = fminf(fp.lod, (float)(levels - 1u));
        linear = smp.min_filter;
        if (smp.mipmap_filter == 0u) { lo = hi = (uint32_t)floorf(lod + 0.5f); }
        else { const float fl = floorf(lod); lo = (uint32_t)fl; hi = min(lo + 1u, levels - 1u); f = (hi != lo) ? lod - fl : 0.0f; }
    }
    const bool fast = common && linear != 0u;
    const bool all_fast = __builtin_amdgcn_ballot_w64(!fast) == 0ull;
    if (GRAD == 2 && fp.m > 0)      // anisotropic footprint on a context that honours max_anisotropy (the kernels' <2> instantiations): the probes, out of line
        return sample_probes(reinterpret_cast<const uint32_t*>(texels), arr.level_off, W, H, layer, lo | (hi << 8) | (smp.address_mode_u << 16) | (smp.address_mode_v << 18) | (linear << 20), f, u, v, fp.major_u, fp.major_v, fp.n, fp.m);
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n = f > 0.0f ? 2 : 1;
    for (int k = 0; k < n; k++) {            // not unrolled: one copy of the samplers per call site
        const uint32_t level = k ? hi : lo;
        const float w = k ? f : 1.0f - f;
        const uint32_t Wl = max(W >> level, 1u), Hl = max(H >> level, 1u);
        const uint32_t* base = reinterpret_cast<const uint32_t*>(texels) + arr.level_off[level] + (size_t)layer * Wl * Hl;
        const f4 c = all_fast ? sample_level_fast(base, Wl, Hl, u, v)
                              : sample_level_generic(reinterpret_cast<const uint8_t*>(base), Wl, Hl, smp.address_mode_u, smp.address_mode_v, linear, u, v);
        acc = {acc.x + c.x * w, acc.y + c.y * w, acc.z + c.z * w, acc.w + c.w * w};
    }
    return acc;
}
// A core texture through its per-draw slot.  MipmapMode::None: the fast path needs nothing but the slot; any other sampler / size falls
// back to the general route through the material words.  MipmapMode::Gradient: level selection as sample_tex<true>, with the array's
// layout and the sampler's modes taken from the slot.
template <int GRAD>
AWSM_DI f4 sample_slot(const Attr& a, const TexSlotDev* __restrict__ slot, const uint32_t* __restrict__ M, uint32_t word) {
    const uint4* q = reinterpret_cast<const uint4*>(slot);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];        // base lo/hi, width, height | flags, tt0, tt1, tt2 | tt3, tt4, tt5, layer_levels
    const uint32_t flags = q1.x;
    const uint32_t uv_set = flags >> 24;
    const float t0 = __uint_as_float(q1.y), t1 = __uint_as_float(q1.z), t2 = __uint_as_float(q1.w), t3 = __uint_as_float(q2.x), t4 = __uint_as_float(q2.y), t5 = __uint_as_float(q2.z);
    if (!GRAD) {
        if (__builtin_amdgcn_ballot_w64((flags & 6u) != 2u) != 0ull) {       // some lane is not on the fast path
            if (flags & 4u) return {0.0f, 0.0f, 0.0f, 0.0f};
            return sample_tex<false>(a, tex_load(M, word));
        }
        f2 uv = a.uv0, ddx, ddy;
        if (!(a.has_uv0 && uv_set == 0u)) uv = attr_uv<false>(a, uv_set, ddx, ddy);
        const float u = affine2_strict(t0, t1, t4, uv.x, uv.y), v = affine2_strict(t2, t3, t5, uv.x, uv.y);
        const uint32_t* base = reinterpret_cast<const uint32_t*>(((unsigned long long)q0.y << 32) | q0.x);
        return sample_level_fast(base, q0.z, q0.w, u, v);
    }
    if (flags & 4u) return {0.0f, 0.0f, 0.0f, 0.0f};
    f2 uv = a.uv0, ddx = a.duv0_dx, ddy = a.duv0_dy;
    if (!(a.has_uv0 && uv_set == 0u)) uv = attr_uv<GRAD>(a, uv_set, ddx, ddy);
    const float u = affine2_strict(t0, t1, t4, uv.x, uv.y), v = affine2_strict(t2, t3, t5, uv.x, uv.y);
    const uint4 q3 = q[3];                              // level_off pointer, array base
    const uint32_t* level_off = reinterpret_cast<const uint32_t*>(((unsigned long long)q3.y << 32) | q3.x);
    const uint32_t* texels = reinterpret_cast<const uint32_t*>(((unsigned long long)q3.w << 32) | q3.z);
    const uint32_t W = q0.z, H = q0.w, layer = q2.w & 0xFFFFu, levels = q2.w >> 24;
    const uint32_t mode_u = (flags >> 13) & 3u, mode_v = (flags >> 21) & 3u;
    // ---- level selection (texture_uvs.wgsl:27-35 + the LOD contract, grad_footprint) ----
    const float dxu = t0 * ddx.x + t1 * ddx.y, dxv = t2 * ddx.x + t3 * ddx.y;
    const float dyu = t0 * ddy.x + t1 * ddy.y, dyv = t2 * ddy.x + t3 * ddy.y;
    GradFootprint fp = grad_footprint(dxu, dxv, dyu, dyv, (float)W, (float)H, GRAD == 2 ? max((q2.w >> 16) & 31u, 1u) : 1u);
    uint32_t lo = 0u, hi = 0u, linear = (flags >> 4) & 1u;
    float f = 0.0f;
    if (fp.lod > 0.0f && levels > 1u) {
        const float lod = fminf(fp.lod, (float)(levels - 1u));
        linear = (flags >> 5) & 1u;
        if (!(flags & 64u)) { lo = hi = (uint32_t)floorf(lod + 0.5f); }
        else { const float fl = floorf(lod); lo = (uint32_t)fl; hi = min(lo + 1u, levels - 1u); f = (hi != lo) ? lod - fl : 0.0f; }
    }
    const bool fast = (flags & 8u) != 0u && linear != 0u;
    const bool all_fast = __builtin_amdgcn_ballot_w64(!fast) == 0ull;
    if (GRAD == 2 && fp.m > 0) return sample_probes(texels, level_off, W, H, layer, lo | (hi << 8) | (mode_u << 16) | (mode_v << 18) | (linear << 20), f, u, v, fp.major_u, fp.major_v, fp.n, fp.m);
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n = f > 0.0f ? 2 : 1;
    for (int k = 0; k < n; k++) {            // not unrolled: one copy of the samplers per call site
        const uint32_t level = k ? hi : lo;
        const float w = k ? f : 1.0f - f;
        const uint32_t Wl = max(W >> level, 1u), Hl = max(H >> level, 1u);
        const uint32_t* base = texels + level_off[level] + (size_t)layer * Wl * Hl;
        const f4 c = all_fast ? sample_level_fast(base, Wl, Hl, u, v)
                              : sample_level_generic(reinterpret_cast<const uint8_t*>(base), Wl, Hl, mode_u, mode_v, linear, u, v);
        acc = {acc.x + c.x * w, acc.y + c.y * w, acc.z + c.z * w, acc.w + c.w * w};
    }
    return acc;
}

AWSM_DI f4 vertex_color(const Attr& a, uint32_t set_index) {               // vertex_color_attrib.wgsl:1-21
    const uint32_t o = set_index * 4u;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = a.bary.x * a.ad[a.v0 + o + j] + a.bary.y * a.ad[a.v1 + o + j] + a.bary.z * a.ad[a.v2 + o + j];
    return {r[0], r[1], r[2], r[3]};
}

AWSM_DI float mf(const uint32_t* __restrict__ m, uint32_t i) { return __uint_as_float(m[i]); }
AWSM_DI uint32_t abs_index(uint32_t base, uint32_t rel) { return rel != 0u ? base + rel : 0u; }

// pbr_material_color.wgsl:4-32
struct PbrColor {
    f3 base; f2 mr; f3 normal; float occlusion; f3 emissive;
    float specular; f3 specular_color; float ior; float transmission;
    float volume_thickness, volume_attenuation_distance; f3 volume_attenuation_color;
    float clearcoat, clearcoat_roughness; f3 clearcoat_normal;
    f3 sheen_color; float sheen_roughness;
};

template <int GRAD>
AWSM_DI f3 normal_map(const Attr& a, const TexInfo& t, float scale, const TBN& tbn) {   // material_color_calc.wgsl:301-322
    if (!t.exists) return tbn.N;
    const f4 s = sample_tex<GRAD>(a, t);
    const float tx = (s.x * 2.0f - 1.0f) * scale, ty = (s.y * 2.0f - 1.0f) * scale, tz = s.z * 2.0f - 1.0f;
    return fm::fnormalize(tbn.T * tx + tbn.B * ty + tbn.N * tz);
}

// ---------------- brdf.wgsl ----------------
AWSM_DI float ior_to_f0(float ior) { const float v = ior < 1.0f ? 1.5f : ior; const float r = fm::fdiv(v - 1.0f, v + 1.0f); return r * r; }
AWSM_DI f3 volume_attenuation(float distance, f3 color, float att_distance) {           // brdf.wgsl:55-74
    if (distance <= 0.0f) return splat3(1.0f);
    if (att_distance <= 0.0f || att_distance > 1e10f) return splat3(1.0f);
    if (color.x >= 0.999f && color.y >= 0.999f && color.z >= 0.999f) return splat3(1.0f);
    const float e = fm::fdiv(distance, att_distance);
    return {fm::powp(color.x, e), fm::powp(color.y, e), fm::powp(color.z, e)};
}
AWSM_DI bool should_apply_volume_attenuation(float thickness, float att_distance, f3 c) {
    return thickness > 0.0f && att_distance < 1e10f && (c.x < 1.0f || c.y < 1.0f || c.z < 1.0f);
}
AWSM_DI f3 fresnel_schlick_f90(float cos_theta, f3 F0, float f90) {                      // brdf.wgsl:111-115
    const float p = fm::pow5(1.0f - saturate(cos_theta));
    return {F0.x + (f90 - F0.x) * p, F0.y + (f90 - F0.y) * p, F0.z + (f90 - F0.z) * p};
}
AWSM_DI float fresnel_schlick_scalar(float cos_theta, float F0) { return F0 + (1.0f - F0) * fm::pow5(1.0f - saturate(cos_theta)); }
AWSM_DI float distribution_ggx(float n_dot_h, float alpha) {                             // brdf.wgsl:118-124
    const float a = fmaxf(alpha, 0.001f);
    const float a2 = a * a;
    const float ndh = saturate(n_dot_h);
    const float d = (ndh * ndh) * (a2 - 1.0f) + 1.0f;
    return fm::fdiv(a2, (kPi * d) * d + kEps);
}
AWSM_DI float geometry_schlick_ggx(float n_dot_x, float alpha) {                         // brdf.wgsl:127-132
    const float a = fmaxf(alpha, 0.001f);
    const float k = ((a + 1.0f) * (a + 1.0f)) * 0.125f;
    const float ndx = saturate(n_dot_x);
    return fm::fdiv(ndx, ndx * (1.0f - k) + k);
}
constexpr float kClearcoatF0 = 0.04f;
AWSM_DI float clearcoat_fresnel(float clearcoat, float v_dot_h) { return clearcoat <= 0.0f ? 0.0f : clearcoat * fresnel_schlick_scalar(v_dot_h, kClearcoatF0); }
AWSM_DI float sheen_albedo_scaling(f3 sheen_color, float sheen_roughness, float n_dot_v) {   // brdf.wgsl:245-262
    const float sheen_max = fmaxf(fmaxf(sheen_color.x, sheen_color.y), sheen_color.z);
    if (sheen_max <= 0.0f) return 1.0f;
    const float alpha = sheen_roughness * sheen_roughness;
    return 1.0f - sheen_max * (alpha * (0.18f + 0.06f * (1.0f - n_dot_v)));
}
// brdf.wgsl:293-302 — linear, clamp-to-edge, RG of the RGBA16F LUT
AWSM_DI f2 sample_brdf_lut(const DevScene* sc, float n_dot_v, float roughness) {
    const float u = saturate(n_dot_v), v = saturate(roughness);
    const int W = (int)sc->lut_w, H = (int)sc->lut_h;
    float fx, fy;
    const float x0f = safe_floor(u * (float)W - 0.5f, fx);
    const float y0f = safe_floor(v * (float)H - 0.5f, fy);
    const int i0 = wrap_index((int)x0f, W, 0u), i1 = wrap_index((int)x0f + 1, W, 0u);
    const int j0 = wrap_index((int)y0f, H, 0u), j1 = wrap_index((int)y0f + 1, H, 0u);
    const uint32_t* L = reinterpret_cast<const uint32_t*>(sc->lut_rg16f);   // one u32 = (r16, g16)
    const uint32_t t00 = L[(size_t)j0 * W + i0], t10 = L[(size_t)j0 * W + i1], t01 = L[(size_t)j1 * W + i0], t11 = L[(size_t)j1 * W + i1];
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float r_top = f16_bits_to_f32((unsigned short)(t00 & 0xFFFFu)) * gx + f16_bits_to_f32((unsigned short)(t10 & 0xFFFFu)) * fx;
    const float r_bot = f16_bits_to_f32((unsigned short)(t01 & 0xFFFFu)) * gx + f16_bits_to_f32((unsigned short)(t11 & 0xFFFFu)) * fx;
    const float g_top = f16_bits_to_f32((unsigned short)(t00 >> 16)) * gx + f16_bits_to_f32((unsigned short)(t10 >> 16)) * fx;
    const float g_bot = f16_bits_to_f32((unsigned short)(t01 >> 16)) * gx + f16_bits_to_f32((unsigned short)(t11 >> 16)) * fx;
    return {r_top * gy + r_bot * fy, g_top * gy + g_bot * fy};
}

}  // namespace awsm
