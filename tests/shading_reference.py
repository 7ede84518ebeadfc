"""The shading of one pixel restated in numpy float64, from the scene description and a pixel coordinate (TEST INFRASTRUCTURE ONLY).

`oracle/c/oracle_shade.c` and the shade kernels were written from one reading of the reference's WGSL, by the same hand, so "the kernel meets the
oracle" cannot notice a mistake they share (DESIGN §2 "parity unpinned").  This module is the third party for the shading stage, as
tests/vertex_stage_reference.py is for the vertex stage: written from the WGSL again, function by function with file:line, in float64, from the
SceneDesc's own materials, textures, samplers, lights and camera.  It imports nothing from oracle/, no packer and no kernel; no material word, no
mirror and no packed record is read.  What it takes next to the SceneDesc: the ORDER of the opaque draw list (through vertex_stage_reference, which
restates the vertex stage and is where world positions, normals and tangents of the vertices come from), the BRDF LUT's texels (an input:
oracle_lib.brdf_lut has its own quadrature test) and, for gradient mips, the mip chain's texels (an input: test_mip_chain_generation_bit_exact pins
the generator; what is restated here is the level and the mix).

Restated: the opaque pass single-sampled, with MSAA x4 and with gradient mips (`Restatement.pixel`, `.pixel_msaa4`), and one fragment of the
transparent pass over a uniform backdrop (`.pixel_forward`).

Paths below are relative to the reference's crates/renderer/src/render_passes/ :
    S/   shared/shared_wgsl/                    OW/  material_opaque/shader/material_opaque_wgsl/
    G/   geometry/shader/geometry_wgsl/         TW/  material_transparent/shader/material_transparent_wgsl/

Where WebGPU is silent the contract of DESIGN §3 stands and is followed here, cited at the line: vertices snapped to 1/256 pixel before the edge
functions, varyings interpolated at the pixel centre, "fine" 2x2 derivatives of the barycentrics, the isotropic level-of-detail rule, bilinear
texel addressing `x = u W - 0.5`, the MSAA sample positions.  The quantisation of the G-buffer is part of the reference (render_textures.rs:49-54:
RG16F barycentrics, RGBA16F packed normal / tangent and barycentric derivatives) and is restated with numpy.float16; `atan2` is exact (the
contract's polynomial is within about 2 f32 ulp of it, an f16 step is 8192 of those).  Every rounding to f16 and the snap report how far the
rounded value sat from the nearest rounding boundary, so that the cases can require their inputs to be unambiguous (tests/shading_cases.py).
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np

from tests import vertex_stage_reference as vsr

PI = math.pi                 # S/math.wgsl:2-4
TAU = 2.0 * math.pi
EPSILON = 1e-4
SUBPIXEL = 256               # DESIGN §3 "Raster": vertices snapped to 1/256 px
MSAA4 = ((96, 32), (224, 96), (32, 160), (160, 224))       # WebGPU's standard 4x pattern in 1/256 px (DESIGN §3 "MSAA x4")
CENTRE = (128, 128)
FORWARD_REACH = 16.0         # pixels: pixel_forward wants the opaque image uniform this far around the pixel

# The tolerances of every comparison against this restatement: 4 x the worst distance between the C oracle (f32) and this module over every
# checked pixel of tests/shading_cases.py, the rule DESIGN §3 uses for the vertex stage.
# tests/test_shading_cpu.py::test_the_committed_tolerances_are_four_times_the_worst_distance prints what it sees; DESIGN §3 "Shading stage" records it.
SHADE_REL_TOL = 4 * 1.24e-6       # colour, relative to max(1, |ref|); measured worst 1.238e-06 (spot_between: the cone's smooth step divides by inner - outer)
BARY_ABS_TOL = 4 * 4.73e-8        # unrounded barycentrics of the pixel centre, absolute; measured worst 4.727e-08 (every single-quad perspective case)
WORST_ALLOWED = 2.5e-5            # the measured worst must stay below this, so that SHADE_REL_TOL stays below the project's 1e-4 bar


# The shaders' floors and cut-offs, by name, so that a case can ask what its pixel would be WITHOUT one (`without_floors`) and require the answer to
# differ: a case that names a floor must be able to see it.
FLOORS = {"roughness_direct": 0.04,      # S/lighting/brdf.wgsl:317
          "roughness_ibl": 0.04,         # :408
          "ggx_alpha": 0.001,            # :120, :129 (never the binding one: every caller clamps its alpha to at least as much first)
          "clearcoat_alpha": 0.001,      # :174
          "clearcoat_roughness_ibl": 0.04,   # :497
          "sheen_roughness": 0.07,       # :236
          "near_white": 0.999}           # :69
_REMOVED = {"near_white": 2.0}           # what "no floor" means for a rule that is not a lower clamp: no colour is ever "white"


class without_floors:
    """with without_floors("sheen_roughness"): ... — the named floors do nothing inside the block"""

    def __init__(self, *names):
        self.names = names

    def __enter__(self):
        self.saved = dict(FLOORS)
        for n in self.names:
            assert n in FLOORS, n
            FLOORS[n] = _REMOVED.get(n, 0.0)

    def __exit__(self, *exc):
        FLOORS.update(self.saved)


def _f64(v):
    """an input as the scene stores it (f32), widened"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def saturate(x):                                                         # S/math.wgsl:8
    return min(max(x, 0.0), 1.0)


def mix(a, b, t):
    return a * (1.0 - t) + b * t


def safe_normalize(v):                                                   # S/math.wgsl:21-28
    len_sq = float(v @ v)
    return v / math.sqrt(len_sq) if len_sq > 0.0 else np.array([0.0, 0.0, 1.0])


def normalize(v):
    return v / math.sqrt(float(v @ v))


# ------------------------------------------------------------------------------------------------ f16 rounding with its margin

def round_f16(x: float):
    """(the f16 value nearest to x as a float, how far x is from the nearest rounding boundary in units of the f16 step there)"""
    h = np.float16(x)
    up, down = np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))
    hf, uf, df = float(h), float(up), float(down)
    margin = min(abs((hf + uf) / 2 - x) / (uf - hf), abs(x - (hf + df) / 2) / (hf - df))
    return hf, margin


class Margins:
    """the smallest distances to a rounding boundary met while one pixel was restated"""

    def __init__(self):
        self.f16 = math.inf          # in f16 steps
        self.snap = math.inf         # in 1/256-pixel steps (0.5 = on a grid point)
        self.edge = math.inf         # smallest screen-space barycentric of the pixel centre / sample: how far inside its triangle

    def half(self, x: float) -> float:
        v, m = round_f16(x)
        self.f16 = min(self.f16, m)
        return v


# ------------------------------------------------------------------------------------------------ G-buffer texel (S/math.wgsl:44-116)

def encode_octahedral(n):                                                # S/math.wgsl:44-53
    n = n / (abs(n[0]) + abs(n[1]) + abs(n[2]))
    if n[2] < 0.0:
        wx = (1.0 - abs(n[1])) * np.sign(n[0])
        wy = (1.0 - abs(n[0])) * np.sign(n[1])
        n = np.array([wx, wy, n[2]])
    return n[:2] * 0.5 + 0.5


def decode_octahedral(e):                                                # S/math.wgsl:55-66
    f = e * 2.0 - 1.0
    n = np.array([f[0], f[1], 1.0 - abs(f[0]) - abs(f[1])])
    t = min(max(-n[2], 0.0), 1.0)
    n = np.array([n[0] + (-t if n[0] >= 0.0 else t), n[1] + (-t if n[1] >= 0.0 else t), n[2]])
    return normalize(n)


def canonical_tb(n):                                                     # S/math.wgsl:74-84
    if n[2] < -0.9999999:
        return np.array([0.0, -1.0, 0.0]), np.array([-1.0, 0.0, 0.0])
    a = 1.0 / (1.0 + n[2])
    bb = -n[0] * n[1] * a
    return np.array([1.0 - n[0] * n[0] * a, bb, -n[0]]), np.array([bb, 1.0 - n[1] * n[1] * a, -n[1]])


def pack_normal_tangent(N, T, s):                                        # S/math.wgsl:93-102
    oct_n = encode_octahedral(N)
    t, b = canonical_tb(N)
    theta = math.atan2(float(T @ b), float(T @ t))
    return np.array([oct_n[0], oct_n[1], (theta + PI) / TAU, 1.0 if s > 0.0 else 0.0])


def unpack_normal_tangent(rgba):                                         # S/math.wgsl:107-116
    N = decode_octahedral(rgba[:2])
    theta = rgba[2] * TAU - PI
    s = 1.0 if rgba[3] >= 0.5 else -1.0
    t0, b0 = canonical_tb(N)
    T = normalize(math.cos(theta) * t0 + math.sin(theta) * b0)
    B = s * normalize(np.cross(N, T))
    return N, T, B


# ------------------------------------------------------------------------------------------------ texture sampling

def _wrap(i: int, n: int, mode: int) -> int:
    """GPUAddressMode as the C-ABI's sampler carries it: 0 clamp-to-edge, 1 repeat, 2 mirror-repeat"""
    if mode == 1:
        return i % n
    if mode == 2:
        m = i % (2 * n)
        return m if m < n else 2 * n - 1 - m
    return min(max(i, 0), n - 1)


def sample_level(texels: np.ndarray, sampler: dict, uv, linear: bool, record: Optional[dict] = None):
    """textureSampleLevel at an integer level whose RGBA8 texels are `texels` (h, w, 4).  DESIGN §3 "Texture sampling": nearest takes texel
    floor(u W); bilinear x = u W - 0.5, the four texels around it weighted by the fractions; texel = byte / 255."""
    h, w = texels.shape[:2]
    mu, mv = sampler.get("address_mode_u", 1), sampler.get("address_mode_v", 1)
    t = texels.astype(np.float64) / 255.0
    if not linear:
        if record is not None:      # nearest is the one discontinuous lookup: how far the coordinate sits from a texel edge, in texels
            d = min(abs(v - round(v)) for v in (uv[0] * w, uv[1] * h))
            record["nearest_margin"] = min(record.get("nearest_margin", math.inf), d)
        return t[_wrap(math.floor(uv[1] * h), h, mv), _wrap(math.floor(uv[0] * w), w, mu)]
    x, y = uv[0] * w - 0.5, uv[1] * h - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    i0, i1, j0, j1 = _wrap(x0, w, mu), _wrap(x0 + 1, w, mu), _wrap(y0, h, mv), _wrap(y0 + 1, h, mv)
    top = t[j0, i0] * (1 - fx) + t[j0, i1] * fx
    bot = t[j1, i0] * (1 - fx) + t[j1, i1] * fx
    return top * (1 - fy) + bot * fy


def sample_grad(levels: List[np.ndarray], sampler: dict, uv, ddx, ddy, record: Optional[dict] = None):
    """textureSampleGrad over a mip chain handed in as data (levels[l]: (h_l, w_l, 4) u8).  DESIGN §3: isotropic
    lod = log2(max(|ddx * size|, |ddy * size|)) (OW/helpers/mipmap.wgsl:419-439 documents the rule), clamped to the chain; lod <= 0 is
    magnification (mag filter, level 0); otherwise the min filter on floor(lod) and floor(lod) + 1 mixed by the fraction (mipmap filter linear)
    or on round(lod) (nearest)."""
    h, w = levels[0].shape[:2]
    rho = max(math.hypot(ddx[0] * w, ddx[1] * h), math.hypot(ddy[0] * w, ddy[1] * h))
    lod = math.log2(max(rho, 1e-6))
    if record is not None:
        record["lod"] = lod
    if not lod > 0.0 or len(levels) == 1:
        return sample_level(levels[0], sampler, uv, sampler.get("mag_filter", 1) != 0, record)
    lod = min(lod, float(len(levels) - 1))
    lin = sampler.get("min_filter", 1) != 0
    if sampler.get("mipmap_filter", 1) == 0:
        return sample_level(levels[int(math.floor(lod + 0.5))], sampler, uv, lin, record)
    lo = int(math.floor(lod))
    f = lod - lo
    hi = min(lo + 1, len(levels) - 1)
    a = sample_level(levels[lo], sampler, uv, lin, record)
    if not f > 0.0 or hi == lo:
        return a
    return a * (1 - f) + sample_level(levels[hi], sampler, uv, lin, record) * f


def texture_transform(tr: Optional[dict]):
    """textures.rs:247-284 (KHR_texture_transform): M = [[c sx, s sy], [-s sx, c sy]], B = offset + origin - M origin; the values as f32 stores them"""
    if not tr:
        return np.eye(2), np.zeros(2)
    sx, sy = _f64(tr.get("scale", (1, 1)))
    off, org = _f64(tr.get("offset", (0, 0))), _f64(tr.get("origin", (0, 0)))
    rot = float(np.float32(tr.get("rotation", 0.0)))
    c, s = math.cos(rot), math.sin(rot)
    M = np.array([[c * sx, s * sy], [-s * sx, c * sy]])
    return M, off + org - M @ org


# ------------------------------------------------------------------------------------------------ S/lighting/brdf.wgsl

def effective_ior(ior):                                                  # :16-18
    return 1.5 if ior < 1.0 else ior


def ior_to_f0(ior):                                                      # :22-26
    v = effective_ior(ior)
    r = (v - 1.0) / (v + 1.0)
    return r * r


def refract_direction(incident, normal, eta):                            # :30-47
    if abs(eta - 1.0) < 0.001:
        return incident
    cos_i = -float(incident @ normal)
    sin_t2 = eta * eta * (1.0 - cos_i * cos_i)
    if sin_t2 > 1.0:
        return np.zeros(3)
    return eta * incident + (eta * cos_i - math.sqrt(1.0 - sin_t2)) * normal


def volume_attenuation(distance, colour, att_distance):                  # :55-75
    if distance <= 0.0:
        return np.ones(3)
    if att_distance <= 0.0 or att_distance > 1e10:
        return np.ones(3)
    if (colour >= FLOORS["near_white"]).all():
        return np.ones(3)
    return colour ** (distance / att_distance)


def should_apply_volume_attenuation(thickness, att_distance, colour):    # :78-86
    return thickness > 0.0 and att_distance < 1e10 and bool((colour < 1.0).any())


def safe_half_vector(v, l):                                              # :95-102
    s = v + l
    len_sq = float(s @ s)
    return s / math.sqrt(len_sq) if len_sq > 1e-8 else np.zeros(3)


def fresnel_schlick_f90(cos_theta, F0, f90):                             # :112-116   (:105-109 is f90 = 1)
    return F0 + (f90 - F0) * (1.0 - saturate(cos_theta)) ** 5


def distribution_ggx(n_dot_h, alpha):                                    # :119-125
    a2 = max(alpha, FLOORS["ggx_alpha"]) ** 2
    ndh = saturate(n_dot_h)
    d = ndh * ndh * (a2 - 1.0) + 1.0
    return a2 / (PI * d * d + EPSILON)


def geometry_schlick_ggx(n_dot_x, alpha):                                # :128-133
    a = max(alpha, FLOORS["ggx_alpha"])
    k = (a + 1.0) * (a + 1.0) * 0.125
    ndx = saturate(n_dot_x)
    return ndx / (ndx * (1.0 - k) + k)


def geometry_smith(n, v, l, alpha):                                      # :136-140
    return geometry_schlick_ggx(saturate(float(n @ v)), alpha) * geometry_schlick_ggx(saturate(float(n @ l)), alpha)


CLEARCOAT_F0 = 0.04                                                      # :147


def clearcoat_brdf_direct(clearcoat, cc_roughness, cc_normal, v, l):     # :150-182
    if clearcoat <= 0.0:
        return 0.0
    cc_n = safe_normalize(cc_normal)
    h = safe_half_vector(v, l)
    if float(h @ h) == 0.0:
        return 0.0
    cc_n_dot_l, cc_n_dot_v = max(float(cc_n @ l), 0.0), max(float(cc_n @ v), 1e-4)
    cc_n_dot_h, cc_v_dot_h = max(float(cc_n @ h), 0.0), max(float(v @ h), 0.0)
    cc_alpha = max(cc_roughness * cc_roughness, FLOORS["clearcoat_alpha"])
    Fc = fresnel_schlick_f90(cc_v_dot_h, CLEARCOAT_F0, 1.0)
    return clearcoat * Fc * distribution_ggx(cc_n_dot_h, cc_alpha) * geometry_smith(cc_n, v, l, cc_alpha) / max(4.0 * cc_n_dot_l * cc_n_dot_v, EPSILON)


def clearcoat_fresnel(clearcoat, v_dot_h):                               # :185-190
    return 0.0 if clearcoat <= 0.0 else clearcoat * fresnel_schlick_f90(v_dot_h, CLEARCOAT_F0, 1.0)


def sheen_brdf_direct(sheen_colour, sheen_roughness, n, v, l):           # :199-242
    if (sheen_colour <= 0.0).all():
        return np.zeros(3)
    h = safe_half_vector(v, l)
    if float(h @ h) == 0.0:
        return np.zeros(3)
    n_dot_l, n_dot_v, n_dot_h = max(float(n @ l), 0.0), max(float(n @ v), 1e-4), max(float(n @ h), 0.0)
    roughness = max(sheen_roughness, FLOORS["sheen_roughness"])
    inv_alpha = 1.0 / (roughness * roughness)
    D = (2.0 + inv_alpha) * (1.0 - n_dot_h * n_dot_h) ** (inv_alpha * 0.5) / (2.0 * PI)          # distribution_charlie
    V = 1.0 / (4.0 * (n_dot_l + n_dot_v - n_dot_l * n_dot_v))                                   # visibility_ashikhmin
    return sheen_colour * D * V


def sheen_albedo_scaling(sheen_colour, sheen_roughness, n_dot_v):        # :247-263
    sheen_max = float(sheen_colour.max())
    if sheen_max <= 0.0:
        return 1.0
    E = sheen_roughness * sheen_roughness * (0.18 + 0.06 * (1.0 - n_dot_v))
    return 1.0 - sheen_max * E


def sample_brdf_lut(lut: np.ndarray, n_dot_v, roughness):                # :294-302; linear, clamp-to-edge (renderer-core brdf_lut/generate.rs:150-170)
    return sample_lut_bilinear(lut, saturate(n_dot_v), saturate(roughness))


def sample_lut_bilinear(lut, u, v):
    h, w = lut.shape[:2]
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    fx, fy = x - x0, y - y0
    c = lambda i: min(max(i, 0), w - 1)      # noqa: E731
    r = lambda j: min(max(j, 0), h - 1)      # noqa: E731
    top = lut[r(y0), c(x0)] * (1 - fx) + lut[r(y0), c(x0 + 1)] * fx
    bot = lut[r(y0 + 1), c(x0)] * (1 - fx) + lut[r(y0 + 1), c(x0 + 1)] * fx
    return top * (1 - fy) + bot * fy


def _f0_f90(c):
    """:330-335 / :415-420: KHR_materials_ior and KHR_materials_specular into F0 and f90"""
    metallic = min(max(c["metallic"], 0.0), 1.0)
    dielectric_f0 = np.minimum(ior_to_f0(c["ior"]) * c["specular_color"], 1.0) * c["specular"]
    return metallic, mix(dielectric_f0, c["base"][:3], metallic), mix(c["specular"], 1.0, metallic)


def brdf_direct(c: dict, normal, light_dir, radiance, surface_to_camera):           # :308-381
    n, v, l = safe_normalize(normal), safe_normalize(surface_to_camera), safe_normalize(light_dir)
    h = safe_half_vector(v, l)
    base = c["base"][:3]
    metallic, F0, f90 = _f0_f90(c)
    roughness = max(min(max(c["roughness"], 0.0), 1.0), FLOORS["roughness_direct"])
    alpha = roughness * roughness
    n_dot_l, n_dot_v = max(float(n @ l), 0.0), max(float(n @ v), 1e-4)
    has_half = float(h @ h) > 0.0
    n_dot_h = max(float(n @ h), 0.0) if has_half else 0.0
    v_dot_h = max(float(v @ h), 0.0) if has_half else 0.0
    F = fresnel_schlick_f90(v_dot_h if has_half else n_dot_v, F0, f90)
    D, G = distribution_ggx(n_dot_h, alpha), geometry_smith(n, v, l, alpha)
    specular = F * (D * G) / max(4.0 * n_dot_l * n_dot_v, EPSILON) if has_half else np.zeros(3)
    k_d = (1.0 - float(F.max())) * (1.0 - metallic)
    diffuse = k_d * base * (1.0 / PI)
    result = (diffuse + specular) * radiance * n_dot_l * c["occlusion"]
    sheen = sheen_brdf_direct(c["sheen_color"], c["sheen_roughness"], n, v, l)
    result = result * sheen_albedo_scaling(c["sheen_color"], c["sheen_roughness"], n_dot_v) + sheen * radiance * n_dot_l * c["occlusion"]
    cc_spec = clearcoat_brdf_direct(c["clearcoat"], c["clearcoat_roughness"], c["clearcoat_normal"], v, l)
    return result * (1.0 - clearcoat_fresnel(c["clearcoat"], v_dot_h)) + cc_spec * radiance * n_dot_l


def brdf_ibl_with_transmission(c: dict, normal, surface_to_camera, env: dict, transmission_background):      # :389-514; the cubes are uniform colours
    n, v = safe_normalize(normal), safe_normalize(surface_to_camera)
    base = c["base"][:3]
    metallic, F0, f90 = _f0_f90(c)
    roughness = max(min(max(c["roughness"], 0.0), 1.0), FLOORS["roughness_ibl"])
    n_dot_v = saturate(float(n @ v))
    F_view = fresnel_schlick_f90(n_dot_v, F0, f90)
    effective_transmission = c["transmission"] * (1.0 - metallic)
    irradiance = env["irradiance"]
    diffuse_brdf = base * (1.0 / PI) * irradiance
    if effective_transmission > 0.0:
        att = np.ones(3)
        if should_apply_volume_attenuation(c["volume_thickness"], c["volume_attenuation_distance"], c["volume_attenuation_color"]):
            att = volume_attenuation(c["volume_thickness"], c["volume_attenuation_color"], c["volume_attenuation_distance"])
        base_layer = mix(diffuse_brdf, transmission_background * base * att, effective_transmission)
    else:
        base_layer = diffuse_brdf
    k_d = (1.0 - float(F_view.max())) * (1.0 - metallic)
    base_contribution = k_d * base_layer * c["occlusion"]
    prefiltered = env["prefiltered"]
    lut = sample_brdf_lut(env["lut"], n_dot_v, roughness)
    specular = prefiltered * (F0 * lut[0] + f90 * lut[1]) * mix(1.0, c["occlusion"], 0.5)
    result = base_contribution * sheen_albedo_scaling(c["sheen_color"], c["sheen_roughness"], n_dot_v)
    if (c["sheen_color"] > 0.0).any():
        alpha = c["sheen_roughness"] * c["sheen_roughness"]
        result = result + c["sheen_color"] * irradiance * alpha * (1.0 - n_dot_v) ** 3 * c["occlusion"]
    result = result + specular + c["emissive"]
    if c["clearcoat"] > 0.0:
        cc_n = safe_normalize(c["clearcoat_normal"])
        cc_n_dot_v = saturate(float(cc_n @ v))
        cc_roughness = max(c["clearcoat_roughness"], FLOORS["clearcoat_roughness_ibl"])
        cc_lut = sample_brdf_lut(env["lut"], cc_n_dot_v, cc_roughness)
        cc_specular = prefiltered * (CLEARCOAT_F0 * cc_lut[0] + cc_lut[1])
        result = result * (1.0 - clearcoat_fresnel(c["clearcoat"], n_dot_v)) + c["clearcoat"] * cc_specular
    return result


def brdf_ibl(c: dict, normal, surface_to_camera, env: dict):             # :517-576: the environment in the (refracted) direction; a uniform cube gives its colour
    metallic = min(max(c["metallic"], 0.0), 1.0)
    background = env["prefiltered"] if c["transmission"] * (1.0 - metallic) > 0.0 else np.zeros(3)
    return brdf_ibl_with_transmission(c, normal, surface_to_camera, env, background)


# ------------------------------------------------------------------------------------------------ S/lighting/lights.wgsl, S/math.wgsl:12-19

def inverse_square(rng, dist):                                           # S/math.wgsl:12-19
    if rng == 0.0:
        return 1.0 / max(dist * dist, 0.01)
    falloff = 1.0 - (dist * dist) / (rng * rng)
    return saturate(falloff * falloff) / (dist * dist + 1.0)


def light_to_brdf(light: dict, world_position):                          # S/lighting/lights.wgsl:70-112; (light_dir, radiance)
    colour, intensity = _f64(light["color"]), float(np.float32(light["intensity"]))
    if light["kind"] == "directional":
        return normalize(-_f64(light["direction"])), colour * intensity
    stl = _f64(light["position"]) - world_position
    dist = math.sqrt(float(stl @ stl))
    light_dir = stl / dist
    att = inverse_square(float(np.float32(light["range"])), dist)
    if light["kind"] == "spot":                                          # :92-101, :115-118; the cone values are cosines (lights.rs:447-468)
        cos_l = float(light_dir @ -normalize(_f64(light["direction"])))
        inner, outer = float(np.float32(light["inner_angle"])), float(np.float32(light["outer_angle"]))
        sm = saturate((cos_l - outer) / (inner - outer))
        att = att * sm * sm
    return light_dir, colour * intensity * att


def apply_lighting(c: dict, surface_to_camera, world_position, lights, env, transmission_background=None):    # S/lighting/lights.wgsl:121-188
    if transmission_background is None:
        colour = brdf_ibl(c, c["normal"], surface_to_camera, env)
    else:
        colour = brdf_ibl_with_transmission(c, c["normal"], surface_to_camera, env, transmission_background)
    for light in lights:
        light_dir, radiance = light_to_brdf(light, world_position)
        colour = colour + brdf_direct(c, c["normal"], light_dir, radiance, surface_to_camera)
    return colour


# ------------------------------------------------------------------------------------------------ the frame

class Restatement:
    """One scene, ready to answer for single pixels.  `mip_chains`: None (MipmapMode::None), or per texture of the scene the list of its levels'
    texels (level 0 first) for gradient mips."""

    def __init__(self, model, lut_rg16f: np.ndarray, mip_chains=None):
        sc = model.scene
        self.scene, self.W, self.H = sc, sc.width, sc.height
        self.view, self.proj = _f64(sc.view).T, _f64(sc.proj).T                    # scene matrices are [col][row]
        self.inv_view, self.inv_proj = np.linalg.inv(self.view), np.linalg.inv(self.proj)
        self.cam_pos = _f64(sc.camera_position)
        self.env = {"lut": np.ascontiguousarray(lut_rg16f, dtype=np.uint16).view(np.float16).astype(np.float64),
                    "irradiance": _f64(sc.irradiance_rgb), "prefiltered": _f64(sc.prefiltered_rgb)}
        assert not sc.env_cubes, "texel cubes are not restated: the cases use uniform colours"
        self.mip_chains = mip_chains
        self.tris = self._triangles(model, model.collect_draws())
        self.forward_tris = self._triangles(model, model.collect_transparent_draws())

    def _triangles(self, model, draws) -> List[dict]:
        """every triangle of a draw list in submission order (its rank), instance after instance, with what the vertex stage made of its corners"""
        out = []
        for d in draws:
            r = vsr.restate_draw(model, d)
            _, p = vsr.primitive_of(model, d["mesh_key"])
            idx = np.asarray(p.indices, dtype=np.int64)
            copies = r["clip"].shape[0] // (3 * idx.shape[0])
            for k in range(copies):
                for t in range(idx.shape[0]):
                    s = slice((k * idx.shape[0] + t) * 3, (k * idx.shape[0] + t) * 3 + 3)
                    out.append({"clip": r["clip"][s], "wpos": r["wpos"][s], "normal": r["normal"][s], "tangent": r["tangent"][s], "vidx": idx[t], "prim": p,
                                "material": self.scene.materials[p.material]})
        return out

    # -------------------------------------------------------------------------------------------- raster (DESIGN §3 "Raster")

    def _screen(self, tri, mg: Optional[Margins]):
        """snapped screen positions (pixels, y down), 1 / w and z / w of a triangle's corners"""
        c = tri["clip"]
        assert (c[:, 3] > 0).all(), "a triangle touching w <= 0 is not restated"
        x = (c[:, 0] / c[:, 3] + 1.0) * 0.5 * self.W * SUBPIXEL
        y = (1.0 - c[:, 1] / c[:, 3]) * 0.5 * self.H * SUBPIXEL
        if mg is not None:
            for v in np.concatenate([x, y]):
                mg.snap = min(mg.snap, abs(v - math.floor(v) - 0.5))
        return np.round(x) / SUBPIXEL, np.round(y) / SUBPIXEL, 1.0 / c[:, 3], c[:, 2] / c[:, 3]

    def _lambda(self, tri, X, Y, mg=None):
        """screen-space barycentrics of the point (X, Y) in the snapped triangle, and whether the triangle faces the camera there (counter-clockwise
        with y up: GPUFrontFace "ccw")"""
        x, y, iw, z = self._screen(tri, mg)
        e = np.array([(x[1] - X) * (y[2] - Y) - (x[2] - X) * (y[1] - Y), (x[2] - X) * (y[0] - Y) - (x[0] - X) * (y[2] - Y),
                      (x[0] - X) * (y[1] - Y) - (x[1] - X) * (y[0] - Y)])
        area = e.sum()
        return (e / area if area != 0.0 else None), area < 0.0, iw, z

    def _at(self, tri, X, Y, mg=None):
        """(perspective-correct barycentrics, depth, screen-space barycentrics) of (X, Y) on a triangle's plane — inside it or not"""
        lam, front, iw, z = self._lambda(tri, X, Y, mg)
        b = lam * iw
        return b / b.sum(), float(lam @ z), lam, front

    def visible(self, px, py, sub=CENTRE, mg: Optional[Margins] = None):
        """(rank, depth) of the triangle a sample shows: covered, not culled, inside the depth range, nearest; None for the background"""
        X, Y = px + sub[0] / SUBPIXEL, py + sub[1] / SUBPIXEL
        best = None
        for rank, tri in enumerate(self.tris):
            lam, front, iw, z = self._lambda(tri, X, Y)
            if lam is None or (lam <= 0.0).any() or (not front and not tri["material"].double_sided):
                continue
            depth = float(lam @ z)
            if 0.0 <= depth <= 1.0 and (best is None or depth < best[1]):
                best = (rank, depth, float(lam.min()))
        if best is not None and mg is not None:
            mg.edge = min(mg.edge, best[2])
        return None if best is None else best[:2]

    # -------------------------------------------------------------------------------------------- G/fragment.wgsl:23-54

    def gbuffer_texel(self, rank, px, py, mg: Margins, derivs=False) -> dict:
        """What the geometry pass stored for pixel (px, py) under triangle `rank`: varyings at the pixel centre (WGSL's default
        @interpolate(perspective, center); with MSAA the centre may lie outside the triangle and the values extrapolate), rounded to the targets'
        formats.  `bary` is the unrounded pair."""
        tri = self.tris[rank]
        b, _, _, _ = self._at(tri, px + 0.5, py + 0.5, mg)
        N = normalize(b @ tri["normal"])
        T4 = b @ tri["tangent"]
        packed = pack_normal_tangent(N, normalize(T4[:3]), T4[3])
        out = {"bary": b[:2].copy(), "halves": np.array([mg.half(v) for v in packed] + [mg.half(b[0]), mg.half(b[1])])}
        if derivs:
            # G/fragment.wgsl:47-51 dpdx / dpdy.  DESIGN §3 / oracle contract: "fine" derivatives of the 2x2 quad — the other pixel of the quad's
            # row / column, evaluated for THIS triangle, right minus left and bottom minus top; stored RGBA16F as (ddx.x, ddy.x, ddx.y, ddy.y)
            bh = self._at(tri, (px ^ 1) + 0.5, py + 0.5)[0]
            bv = self._at(tri, px + 0.5, (py ^ 1) + 0.5)[0]
            ddx = (b - bh) if px & 1 else (bh - b)
            ddy = (b - bv) if py & 1 else (bv - b)
            out["bary_derivs"] = np.array([mg.half(ddx[0]), mg.half(ddy[0]), mg.half(ddx[1]), mg.half(ddy[1])])
        return out

    # -------------------------------------------------------------------------------------------- OW/helpers/standard.wgsl:11-62

    def standard_coordinates(self, px, py, depth):
        ndc = np.array([(px + 0.5) / self.W * 2.0 - 1.0, 1.0 - (py + 0.5) / self.H * 2.0, depth, 1.0])
        view_h = self.inv_proj @ ndc
        view_position = view_h[:3] / max(view_h[3], 1e-8)
        world_position = (self.inv_view @ np.append(view_position, 1.0))[:3]
        if self.proj[3, 3] > 0.9:                                        # :36-42 orthographic: the view's z axis
            return world_position, normalize(self.inv_view[:3, 2])
        to_camera = self.cam_pos - world_position                        # :43-51
        return world_position, (safe_normalize(to_camera) if float(to_camera @ to_camera) > 0.0 else np.array([0.0, 0.0, 1.0]))

    # -------------------------------------------------------------------------------------------- material colour

    def _sample(self, ref, tri, bary, derivs, channels=slice(0, 4), record=None):
        """OW/helpers/texture_uvs.wgsl:64-84 (the UV set's interpolation), S/textures.wgsl:131-150 (KHR_texture_transform), then level 0
        (OW/helpers/texture_uvs.wgsl:144-187) or, with gradient mips, the chain rule of OW/helpers/mipmap.wgsl:113-205 and textureSampleGrad
        (OW/helpers/texture_uvs.wgsl:8-43, 90-138)"""
        uvs = _f64(tri["prim"].uvs[ref.uv_index])[tri["vidx"]]
        uv = bary @ uvs
        M, B = texture_transform(ref.transform)
        if record is not None:
            record.setdefault("uv", []).append(M @ uv + B)
        sampler = self.scene.samplers[ref.sampler]
        if self.mip_chains is None:
            return sample_level(self.scene.textures[ref.texture], sampler, M @ uv + B, sampler.get("mag_filter", 1) != 0, record)[channels]
        da_dx, da_dy, db_dx, db_dy = derivs
        ddx = uvs[0] * da_dx + uvs[1] * db_dx + uvs[2] * (-da_dx - db_dx)
        ddy = uvs[0] * da_dy + uvs[1] * db_dy + uvs[2] * (-da_dy - db_dy)
        return sample_grad(self.mip_chains[ref.texture], sampler, M @ uv + B, M @ ddx, M @ ddy, record)[channels]

    def _normal_map(self, ref, scale, tbn, tri, bary, derivs):           # OW/helpers/material_color_calc.wgsl:301-322, :449-471
        if ref is None:
            return tbn[0]
        t = self._sample(ref, tri, bary, derivs)
        tn = np.array([(t[0] * 2.0 - 1.0) * scale, (t[1] * 2.0 - 1.0) * scale, t[2] * 2.0 - 1.0])
        N, T, B = tbn
        return normalize(T * tn[0] + B * tn[1] + N * tn[2])

    def material_color(self, tri, bary, derivs, tbn, forward=False, record=None) -> dict:
        """OW/helpers/material_color_calc.wgsl:25-265 with S/pbr/pbr_material.wgsl:243-415 for what an absent extension reads as"""
        m = tri["material"]
        f = lambda v: float(np.float32(v))      # noqa: E731
        tex = lambda ref, ch=slice(0, 4): self._sample(ref, tri, bary, derivs, ch, record)      # noqa: E731
        c = {}
        base = _f64(m.base_color_factor)                                 # :268-282
        if m.base_color_tex is not None:
            base = base * tex(m.base_color_tex)
        if not forward:
            base[3] = 1.0
        colours = tri["prim"].colors
        if not forward:
            if m.vertex_color_set is not None:                           # :58-68, OW/helpers/vertex_color_attrib.wgsl:1-21
                base = base * (bary @ _f64(colours[m.vertex_color_set])[tri["vidx"]])
        elif colours:                                                    # TW/helpers/material_color_calc.wgsl:38-52: set 0 unless the material names one
            k = m.vertex_color_set if m.vertex_color_set is not None else 0
            if k < len(colours):
                base = base * (bary @ _f64(colours[k])[tri["vidx"]])
        c["base"] = base
        c["metallic"], c["roughness"] = f(m.metallic_factor), f(m.roughness_factor)          # :285-297: metallic from B, roughness from G
        if m.metallic_roughness_tex is not None:
            t = tex(m.metallic_roughness_tex)
            c["metallic"], c["roughness"] = c["metallic"] * t[2], c["roughness"] * t[1]
        c["normal"] = self._normal_map(m.normal_tex, f(m.normal_scale), tbn, tri, bary, derivs)
        c["occlusion"] = 1.0                                             # :325-336
        if m.occlusion_tex is not None:
            c["occlusion"] = mix(1.0, tex(m.occlusion_tex)[0], f(m.occlusion_strength))
        em = _f64(m.emissive_factor)                                     # :339-351
        if m.emissive_tex is not None:
            em = em * tex(m.emissive_tex)[:3]
        c["emissive"] = em * (1.0 if m.emissive_strength is None else f(m.emissive_strength))
        sp = m.specular or {}                                            # :354-377: the factor in A, the colour in RGB
        c["specular"] = f(sp.get("factor", 1.0)) * (tex(sp["tex"])[3] if sp.get("tex") is not None else 1.0)
        c["specular_color"] = _f64(sp.get("color_factor", (1, 1, 1))) * (tex(sp["color_tex"])[:3] if sp.get("color_tex") is not None else 1.0)
        c["ior"] = 1.5 if m.ior is None else f(m.ior)
        tr = m.transmission or {}                                        # :380-394
        c["transmission"] = f(tr.get("factor", 0.0)) * (tex(tr["tex"])[0] if tr.get("tex") is not None else 1.0)
        vo = m.volume or {}                                              # :397-412: thickness from G
        c["volume_thickness"] = f(vo.get("thickness_factor", 0.0)) * (tex(vo["thickness_tex"])[1] if vo.get("thickness_tex") is not None else 1.0)
        c["volume_attenuation_distance"] = f(vo.get("attenuation_distance", 0.0))
        c["volume_attenuation_color"] = _f64(vo.get("attenuation_color", (1, 1, 1)))
        cc = m.clearcoat or {}                                           # :419-471: factor from R, roughness from G
        c["clearcoat"] = f(cc.get("factor", 0.0)) * (tex(cc["tex"])[0] if cc.get("tex") is not None else 1.0)
        c["clearcoat_roughness"] = f(cc.get("roughness_factor", 0.0)) * (tex(cc["roughness_tex"])[1] if cc.get("roughness_tex") is not None else 1.0)
        c["clearcoat_normal"] = self._normal_map(cc.get("normal_tex"), f(cc.get("normal_scale", 1.0)), tbn, tri, bary, derivs)
        sh = m.sheen or {}                                               # :478-501: colour from RGB, roughness from A
        c["sheen_color"] = _f64(sh.get("color_factor", (0, 0, 0))) * (tex(sh["color_tex"])[:3] if sh.get("color_tex") is not None else 1.0)
        c["sheen_roughness"] = f(sh.get("roughness_factor", 0.0)) * (tex(sh["roughness_tex"])[3] if sh.get("roughness_tex") is not None else 1.0)
        return c

    @staticmethod
    def debug_color(bitmask: int, c: dict):                              # S/pbr/pbr_material_color.wgsl:29-60, bits: S/pbr/pbr_material.wgsl:223-240
        if bitmask & 1:
            return c["base"][:3]
        if bitmask & 2:
            return np.array([c["metallic"], c["roughness"], 0.0])
        if bitmask & 4:
            return c["normal"] * 0.5 + 0.5
        if bitmask & 8:
            return np.full(3, c["occlusion"])
        if bitmask & 16:
            return c["emissive"]
        if bitmask & 32:
            return c["specular_color"] * c["specular"]
        return np.array([1.0, 0.0, 1.0])

    # -------------------------------------------------------------------------------------------- one visibility sample (OW/compute.wgsl:171-299)

    def shade_surface(self, rank, px, py, depth_sample, mg: Margins) -> dict:
        """== OW/helpers/material_shading.wgsl:59-174 for one MSAA sample.  `depth_sample`: the depth the standard coordinates are built from."""
        tri = self.tris[rank]
        g = self.gbuffer_texel(rank, px, py, mg, derivs=self.mip_chains is not None)
        h = g["halves"]
        bary = np.array([h[4], h[5], 1.0 - h[4] - h[5]])                 # OW/compute.wgsl:185-186: z = 1 - x - y of the stored pair
        tbn = unpack_normal_tangent(h[:4])
        world_position, surface_to_camera = self.standard_coordinates(px, py, depth_sample)
        m = tri["material"]
        out = {"gbuffer": g, "world_position": world_position, "surface_to_camera": surface_to_camera, "tbn": tbn, "record": {}}
        derivs = g.get("bary_derivs")
        if m.kind == "unlit":                                            # OW/helpers/material_color_calc.wgsl:508-583, S/lighting/unlit.wgsl
            base, em = _f64(m.base_color_factor), _f64(m.emissive_factor)
            if m.base_color_tex is not None:
                base = base * self._sample(m.base_color_tex, tri, bary, derivs, record=out["record"])
            if m.emissive_tex is not None:
                em = em * self._sample(m.emissive_tex, tri, bary, derivs, slice(0, 3))
            out.update(color=base[:3] + em, alpha=1.0)
            return out
        c = self.material_color(tri, bary, derivs, tbn, record=out["record"])
        out["material"] = c
        if m.debug_bitmask:
            out.update(color=self.debug_color(m.debug_bitmask, c), alpha=1.0, debug=True)
            return out
        out.update(color=apply_lighting(c, surface_to_camera, world_position, self.scene.lights, self.env), alpha=float(c["base"][3]))
        return out

    def pixel(self, px, py) -> dict:
        """the opaque pass's output at a single-sampled pixel; `margins` says how unambiguous every rounding on the way was"""
        mg = Margins()
        vis = self.visible(px, py, CENTRE, mg)
        assert vis is not None, ("the pixel shows the background", px, py)
        out = self.shade_surface(vis[0], px, py, vis[1], mg)
        out.update(rank=vis[0], depth=vis[1], margins=mg, xy=(px, py))
        return out

    def pixel_msaa4(self, px, py) -> dict:
        """MSAA x4 (OW/helpers/material_shading.wgsl:177-209, OW/compute.wgsl:155-170, 303-318): every sample's triangle shaded with the pixel centre's
        varyings and the standard coordinates of sample 0's depth; the mean of the four where the samples differ, sample 0's colour where they show
        one triangle (an interior pixel: the edge detector's thresholds are the cases' business)."""
        mg = Margins()
        vis = [self.visible(px, py, s, mg) for s in MSAA4]
        assert all(v is not None for v in vis), ("a sample shows the background", px, py)
        depth0 = vis[0][1]
        ranks = [v[0] for v in vis]
        samples = [self.shade_surface(r, px, py, depth0, mg) for r in (ranks if len(set(ranks)) > 1 else ranks[:1])]
        out = dict(samples[0])
        out.update(color=np.mean([s["color"] for s in samples], axis=0), alpha=float(np.mean([s["alpha"] for s in samples])), ranks=ranks, margins=mg,
                   samples=samples)
        return out

    # -------------------------------------------------------------------------------------------- transparent pass (TW/fragment.wgsl:186-288)

    def pixel_forward(self, px, py, backdrop) -> dict:
        """One fragment of the transparent pass over a uniform backdrop (the opaque image's colour there, as that RGBA16F target holds it):
        TW/vertex.wgsl's varyings interpolated at the pixel centre and NOT quantised, TW/helpers/material_color_calc.wgsl (N, T, B from the
        interpolated vertex normal and tangent, :5-18, :125-152; alpha kept; every mesh with colour sets multiplies by one), then
        TW/fragment.wgsl:219-287: screen-space transmission when transmission * (1 - metallic) > 0 — over a uniform backdrop whatever taps the
        blur takes and wherever the refracted ray lands give that one colour, and so must the environment fallback (asserted) — the colour
        premultiplied by alpha, and the pipeline's blend (material_transparent/pipeline.rs:96-110: One / OneMinusSrcAlpha on colour and alpha).
        Restated for a pixel that exactly one transparent triangle covers, with no opaque geometry within FORWARD_REACH pixels of it (what the
        blur's taps and the refracted ray can reach in the cases); single-sampled, MipmapMode::None."""
        assert self.mip_chains is None, "restated without mips"
        backdrop = np.asarray(backdrop, dtype=np.float64)
        mg = Margins()
        X, Y = px + 0.5, py + 0.5
        for tri in self.tris:
            x, y, _, _ = self._screen(tri, None)
            assert (np.maximum(np.abs(x - X), np.abs(y - Y)) > FORWARD_REACH).all(), ("opaque geometry near the pixel: the backdrop is not uniform", px, py)
        hits = []
        for rank, tri in enumerate(self.forward_tris):
            lam, front, iw, z = self._lambda(tri, X, Y, mg)
            if lam is None or (lam <= 0.0).any() or (not front and not tri["material"].double_sided):
                continue
            if 0.0 <= float(lam @ z) <= 1.0:
                hits.append((rank, front, float(lam.min())))
        assert len(hits) == 1, ("restated for exactly one fragment per pixel", px, py, hits)
        rank, front, mg.edge = hits[0]
        tri = self.forward_tris[rank]
        m = tri["material"]
        assert m.kind == "pbr" and m.alpha_mode != "mask" and not m.debug_bitmask
        b = self._at(tri, X, Y)[0]
        world_position, world_normal, world_tangent = b @ tri["wpos"], b @ tri["normal"], b @ tri["tangent"]
        if not front:                                                    # TW/fragment.wgsl:194-200
            world_normal, world_tangent = -world_normal, world_tangent * np.array([1.0, 1.0, 1.0, -1.0])
        if abs(self.proj[3, 3] - 1.0) < 0.001:                           # TW/fragment.wgsl:206-212
            surface_to_camera = normalize(self.inv_view[:3, 2])
        else:
            surface_to_camera = normalize(self.cam_pos - world_position)
        N = normalize(world_normal)
        t = world_tangent[:3] - N * float(world_tangent[:3] @ N)         # orthonormal_tangent_from_vertex, TW/helpers/material_color_calc.wgsl:5-18
        len_sq = float(t @ t)
        if len_sq > 1e-8:
            T = t / math.sqrt(len_sq)
        else:
            T = normalize(np.cross(np.array([0.0, 1.0, 0.0]) if abs(N[2]) > 0.999 else np.array([0.0, 0.0, 1.0]), N))
        tbn = (N, T, np.cross(N, T) * world_tangent[3])
        record = {"tangent_len_sq": len_sq}
        c = self.material_color(tri, b, None, tbn, forward=True, record=record)
        metallic = min(max(c["metallic"], 0.0), 1.0)
        transmits = c["transmission"] * (1.0 - metallic) > 0.0
        if transmits:
            assert np.array_equal(self.env["prefiltered"], backdrop), "the environment fallback must give the backdrop's colour too"
        colour = apply_lighting(c, surface_to_camera, world_position, self.scene.lights, self.env, backdrop if transmits else None)
        alpha = float(c["base"][3])
        return {"color": colour, "alpha": alpha, "composite": np.append(colour * alpha + backdrop * (1.0 - alpha), alpha + 1.0 * (1.0 - alpha)),
                "material": c, "tbn": tbn, "surface_to_camera": surface_to_camera, "world_position": world_position, "margins": mg, "record": record,
                "rank": rank, "transmits": transmits, "xy": (px, py)}
