// shade_gbuffer.hpp — the STRICT G-buffer reconstruction and the MSAA edge predicates.
// Everything here follows the arithmetic contract (-ffp-contract=off, IEEE div/sqrt), whatever the including file set before.
#pragma once
#include "frame_params.hpp"
#include "raster_setup.hpp"

#pragma clang fp contract(off)

namespace awsm {

// ================================================================================================
// STRICT section (arithmetic contract, -ffp-contract=off, IEEE div/sqrt): what fs_main wrote for this pixel
// (fragment.wgsl:23-54), rounded to the G-buffer storage formats.  Bit-identical to the CPU oracle (tests only).
// ================================================================================================
struct GBufferTexel {
    f4 packed_nt;    // RGBA16F normal_tangent, already rounded to f16
    float bx, by;    // RG16F barycentric, already rounded to f16
    f4 bary_derivs;  // RGBA16F barycentric_derivatives (db0/dx, db0/dy, db1/dx, db1/dy), rounded to f16; MipmapMode::Gradient only
};
// The interpolants are evaluated at the PIXEL CENTRE (@interpolate(perspective, center)); with MSAA the centre may lie
// outside the triangle and the values extrapolate — every sample the triangle covers in the pixel gets the same texel.
// A key in the visibility buffer means the triangle's setup record is valid; its edge coefficients are the bits the
// raster kernel used.
template <bool DERIVS>
AWSM_DI GBufferTexel reconstruct_core(const TriSetup& t, float4 n0, float4 n1, float4 n2, float4 t0, float4 t1, float4 t2, int cx, int cy) {
    GBufferTexel g;
    g.bary_derivs = {0.0f, 0.0f, 0.0f, 0.0f};
    const double Xc = sample_coord((cx << 8) + 128), Yc = sample_coord((cy << 8) + 128);
    const EdgeVals ev = tri_edges_d(t, Xc, Yc);
    // screen-space edge weights -> perspective-correct barycentrics: one IEEE reciprocal, six products
    const float e0 = (float)ev.E[0] * t.iw[0], e1 = (float)ev.E[1] * t.iw[1], e2 = (float)ev.E[2] * t.iw[2];
    const float inv_esum = 1.0f / ((e0 + e1) + e2);
    const float b0 = e0 * inv_esum, b1 = e1 * inv_esum, b2 = e2 * inv_esum;
    const f3 Ni = {(b0 * n0.x + b1 * n1.x) + b2 * n2.x, (b0 * n0.y + b1 * n1.y) + b2 * n2.y, (b0 * n0.z + b1 * n1.z) + b2 * n2.z};
    const f4 Ti = {(b0 * t0.x + b1 * t1.x) + b2 * t2.x, (b0 * t0.y + b1 * t1.y) + b2 * t2.y,
                   (b0 * t0.z + b1 * t1.z) + b2 * t2.z, (b0 * t0.w + b1 * t1.w) + b2 * t2.w};
    const f4 p = pack_normal_tangent(normalize(Ni), normalize(mk3(Ti.x, Ti.y, Ti.z)), Ti.w);
    g.packed_nt = {round_f16(p.x), round_f16(p.y), round_f16(p.z), round_f16(p.w)};
    g.bx = round_f16(b0);
    g.by = round_f16(b1);
    if (DERIVS) {
        // fragment.wgsl:46-51 dpdx/dpdy of the barycentrics.  Contract ("fine" derivatives of a 2x2 quad): the difference
        // between the two pixels of the quad row / column this pixel sits in, both evaluated for THIS triangle (helper
        // invocations extrapolate), right minus left and bottom minus top; then RGBA16F.
        const EdgeVals eh = tri_edges_d(t, sample_coord(((cx ^ 1) << 8) + 128), Yc), evv = tri_edges_d(t, Xc, sample_coord(((cy ^ 1) << 8) + 128));
        const float h0 = (float)eh.E[0] * t.iw[0], h1 = (float)eh.E[1] * t.iw[1], h2 = (float)eh.E[2] * t.iw[2];
        const float w0 = (float)evv.E[0] * t.iw[0], w1 = (float)evv.E[1] * t.iw[1], w2 = (float)evv.E[2] * t.iw[2];
        const float ish = 1.0f / ((h0 + h1) + h2), isv = 1.0f / ((w0 + w1) + w2);
        const float hb0 = h0 * ish, hb1 = h1 * ish, vb0 = w0 * isv, vb1 = w1 * isv;
        const float ddx0 = (cx & 1) ? b0 - hb0 : hb0 - b0, ddx1 = (cx & 1) ? b1 - hb1 : hb1 - b1;
        const float ddy0 = (cy & 1) ? b0 - vb0 : vb0 - b0, ddy1 = (cy & 1) ? b1 - vb1 : vb1 - b1;
        g.bary_derivs = {round_f16(ddx0), round_f16(ddy0), round_f16(ddx1), round_f16(ddy1)};
    }
    return g;
}
template <bool DERIVS>
AWSM_DI GBufferTexel reconstruct_gbuffer(const FrameDev& f, uint32_t rank, int cx, int cy) {
    TriSetup t;
    tri_rec_load(f.tri_rec + rank, t);
    const float4 n0 = f.nrm[(size_t)rank * 3], n1 = f.nrm[(size_t)rank * 3 + 1], n2 = f.nrm[(size_t)rank * 3 + 2];
    const float4 t0 = f.tan[(size_t)rank * 3], t1 = f.tan[(size_t)rank * 3 + 1], t2 = f.tan[(size_t)rank * 3 + 2];
    return reconstruct_core<DERIVS>(t, n0, n1, n2, t0, t1, t2, cx, cy);
}

// The decoded normal of the pixel's G-buffer texel alone — decode_octahedral(packed_nt.xy) — for the MSAA edge detector: the same operations on the
// same values as reconstruct_core + pack_normal_tangent's octahedral half, without the tangent (its interpolation, normalisation, basis and atan2: a
// third of the reconstruction) and without the tangents' 48 bytes per lane.  Bit-identical to unpack_normal_tangent(g.packed_nt).N by construction.
AWSM_DI f2 strict_oct_of(const FrameDev& f, uint32_t rank, int cx, int cy) {
    TriSetup t;
    tri_rec_load(f.tri_rec + rank, t);
    const float4 n0 = f.nrm[(size_t)rank * 3], n1 = f.nrm[(size_t)rank * 3 + 1], n2 = f.nrm[(size_t)rank * 3 + 2];
    const double Xc = sample_coord((cx << 8) + 128), Yc = sample_coord((cy << 8) + 128);
    const EdgeVals ev = tri_edges_d(t, Xc, Yc);
    const float e0 = (float)ev.E[0] * t.iw[0], e1 = (float)ev.E[1] * t.iw[1], e2 = (float)ev.E[2] * t.iw[2];
    const float inv_esum = 1.0f / ((e0 + e1) + e2);
    const float b0 = e0 * inv_esum, b1 = e1 * inv_esum, b2 = e2 * inv_esum;
    const f3 Ni = {(b0 * n0.x + b1 * n1.x) + b2 * n2.x, (b0 * n0.y + b1 * n1.y) + b2 * n2.y, (b0 * n0.z + b1 * n1.z) + b2 * n2.z};
    const f2 oct = encode_octahedral(normalize(Ni));
    return mk2(round_f16(oct.x), round_f16(oct.y));
}
AWSM_DI f3 strict_normal_of(const FrameDev& f, uint32_t rank, int cx, int cy) { return decode_octahedral(strict_oct_of(f, rank, cx, cy)); }
// An octahedral pair as two f16 in a word (its values ARE f16 values: exact both ways)
AWSM_DI uint32_t oct_word(f2 oct) { return (uint32_t)f16_bits(oct.x) | ((uint32_t)f16_bits(oct.y) << 16); }
AWSM_DI f2 oct_of_word(uint32_t w) { return mk2(__half2float(__ushort_as_half((unsigned short)(w & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(w >> 16)))); }

// Is pixel row `py` one this shard shades (row strip: [sy0, sy1); bands: the 32-row tile rows r, r + n, ...)?
AWSM_DI bool row_owned(const FrameDev& f, int py) {
    if (py < (int)f.sy0 || py >= (int)f.sy1) return false;
    return f.band_n <= 1u || (((uint32_t)py >> kTileShift) % f.band_n) == f.band_r;
}

// ---- MSAA edge predicates (helpers/msaa.wgsl), STRICT: a decision that flips between implementations would swap a
// pixel between one-sample and four-sample shading, so every value feeding a threshold follows the arithmetic contract ----
constexpr float kEdgeNormalThreshold = 0.95f, kEdgeDepthThreshold = 0.02f, kEdgeMsaaDepthThreshold = 0.02f;
AWSM_DI float view_space_depth(const m4& inv_proj, float depth, float px, float py, float W, float H) {   // msaa.wgsl:185-199
    // A projection whose view-space z and w depend on the depth alone (every perspective_rh / orthographic_rh: glam's matrices have exact zeros there) makes
    // the x and y terms of those two rows exact zeros, and ((0 x + 0 y) + c2 d) + c3 IS c2 d + c3 bit for bit: the NDC divisions and two thirds of the
    // product drop out (the detector calls this up to nine times per pixel).  Wave-uniform test; anything else takes the full product.
    if (inv_proj.c[0].z == 0.0f && inv_proj.c[1].z == 0.0f && inv_proj.c[0].w == 0.0f && inv_proj.c[1].w == 0.0f)
        return (inv_proj.c[2].z * depth + inv_proj.c[3].z) / (inv_proj.c[2].w * depth + inv_proj.c[3].w);
    const f4 view_pos = mul(inv_proj, mk4((px / W) * 2.0f - 1.0f, 1.0f - (py / H) * 2.0f, depth, 1.0f));
    return view_pos.z / view_pos.w;
}
AWSM_DI float key_depth(unsigned long long k) { return k == ~0ull ? 1.0f : __uint_as_float((uint32_t)(k >> 32)); }   // depth clear = 1.0
AWSM_DI uint32_t key_rank(unsigned long long k) { return 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull); }
AWSM_DI bool edge_mask_depth_msaa(const m4& inv_proj, const unsigned long long k4[4], float pcx, float pcy, float W, float H) {   // msaa.wgsl:116-146
    uint32_t count = 0; float dmin = 1e9f, dmax = -1e9f;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        if (k4[s] == ~0ull) continue;
        count++;
        const float vd = view_space_depth(inv_proj, key_depth(k4[s]), pcx, pcy, W, H);
        dmin = fminf(dmin, vd); dmax = fmaxf(dmax, vd);
    }
    if (count < 2u) return false;
    return fabsf(dmax - dmin) > (kEdgeMsaaDepthThreshold * fabsf((dmax + dmin) * 0.5f));
}

// The two depth predicates with the division behind a filter: a projection whose view depth is (a d + b) / (c d + e) (view_space_depth's first form) is
// evaluated with the hardware reciprocal — numerator and denominator as the strict form computes them, so the quotient is within 2 ulps of the IEEE one —
// and the comparison is accepted when it clears the threshold by more than 4e-6 of the larger depth (ten times that error); anything closer, and any
// other projection, takes the strict form.  Same decisions, a fifth of the instructions (an IEEE division is ten, and the detector makes up to nine).
AWSM_DI bool depth_only_projection(const m4& inv_proj) { return inv_proj.c[0].z == 0.0f && inv_proj.c[1].z == 0.0f && inv_proj.c[0].w == 0.0f && inv_proj.c[1].w == 0.0f; }
AWSM_DI float view_depth_approx(const m4& inv_proj, float depth) { return (inv_proj.c[2].z * depth + inv_proj.c[3].z) * __builtin_amdgcn_rcpf(inv_proj.c[2].w * depth + inv_proj.c[3].w); }
AWSM_DI bool edge_mask_depth_msaa_filtered(const m4& inv_proj, const unsigned long long k4[4], float pcx, float pcy, float W, float H) {
    if (depth_only_projection(inv_proj)) {      // wave-uniform
        uint32_t count = 0; float dmin = 1e9f, dmax = -1e9f;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (k4[s] == ~0ull) continue;
            count++;
            const float vd = view_depth_approx(inv_proj, key_depth(k4[s]));
            dmin = fminf(dmin, vd); dmax = fmaxf(dmax, vd);
        }
        if (count < 2u) return false;
        const float lhs = fabsf(dmax - dmin), rhs = kEdgeMsaaDepthThreshold * fabsf((dmax + dmin) * 0.5f), margin = 4e-6f * fmaxf(fabsf(dmax), fabsf(dmin));
        if (lhs > rhs + margin) return true;
        if (lhs < rhs - margin) return false;     // (a NaN falls through to the strict form)
    }
    return edge_mask_depth_msaa(inv_proj, k4, pcx, pcy, W, H);
}

// standard.wgsl:17-33 operation by operation (IEEE divisions, no contraction: this function sits in the STRICT part of the file): the world position exactly
// as the oracle forms it.  Used by the experiment AWSM_STRICT_POSITION only (tests/diagnostics/abs_bar_survey.py: which pixels over the absolute colour bar
// come from the position's last bits) — the shipped kernels compose pixel -> view on the host (FrameDev.pix2view).
AWSM_DI f3 strict_world_position(const m4& inv_proj, const m4& inv_view, int cx, int cy, float W, float H, float depth) {
    const float uvx = ((float)cx + 0.5f) / W, uvy = ((float)cy + 0.5f) / H;
    const f4 view_h = mul(inv_proj, mk4(uvx * 2.0f - 1.0f, 1.0f - uvy * 2.0f, depth, 1.0f));
    const float vw = fmaxf(view_h.w, 1e-8f);
    const f4 wp = mul(inv_view, mk4(view_h.x / vw, view_h.y / vw, view_h.z / vw, 1.0f));
    return {wp.x, wp.y, wp.z};
}

}  // namespace awsm
