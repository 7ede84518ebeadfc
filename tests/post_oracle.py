"""CPU oracle of the effects pass and the display pass (render.rs:339-356), numpy f32, one operation after the other as DESIGN.md §11 fixes them.

fmax / fmin stand for the kernel's fmaxf / fminf (a NaN operand yields the other one).  Inputs are the device's own composite (RGBA16F bits) and depth, so a comparison measures the post pass alone, not shading parity.
  effects(composite_f16, depth, camera, smaa, bloom, dof) -> (effects RGBA16F bits [H, W, 4] uint16, ill-conditioned DoF pixels [H, W] bool)
  display(effects_f16, tonemapping)                       -> RGBA8 [H, W, 4] uint8
Reference WGSL: effects_wgsl/{compute.wgsl, helpers/{smaa,bloom,dof}.wgsl}, display_wgsl/{fragment.wgsl, helpers/tonemap.wgsl},
shared_wgsl/color_space.wgsl.
"""
from __future__ import annotations

import math

import numpy as np

f = np.float32
F0, F1 = f(0.0), f(1.0)

# ---- the two fixed tables (kernels_post.hip holds the same values; tests/test_post_cpu.py compares them) ----
BLOOM_TAPS = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 2.0 * 2.0 + 0.5]
_bw = [math.exp(-(dx * dx + dy * dy) / (2.0 * 2.0 * 2.0)) for dx, dy in BLOOM_TAPS]
BLOOM_W = np.array([w / sum(_bw) for w in _bw], dtype=np.float32)
DISK = np.array([[math.cos(float(f(i) * f(2.39996323))) * math.sqrt((i + 1) / 16.0),
                  math.sin(float(f(i) * f(2.39996323))) * math.sqrt((i + 1) / 16.0)] for i in range(16)], dtype=np.float32)
SRGB_EXP = f(1.0 / 2.4)


def f16_to_f32(bits: np.ndarray) -> np.ndarray:
    return bits.astype(np.uint16).view(np.float16).astype(np.float32)


def f32_to_f16(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return x.astype(np.float32).astype(np.float16).view(np.uint16)


def round_f16(x: np.ndarray) -> np.ndarray:
    return f16_to_f32(f32_to_f16(x))


def mix(a, b, t):
    return a * (F1 - t) + b * t


def clamp01(x):
    return np.fmin(np.fmax(x, F0), F1)


def smoothstep(e0, e1, x):
    t = clamp01((x - e0) / (e1 - e0))
    return t * t * (f(3.0) - f(2.0) * t)


def luma(rgb):
    return rgb[..., 0] * f(0.2126) + rgb[..., 1] * f(0.7152) + rgb[..., 2] * f(0.0722)


def linear_to_srgb(c):
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        high = f(1.055) * np.power(c, SRGB_EXP) - f(0.055)
    return np.where(c <= f(0.0031308), c * f(12.92), high).astype(np.float32)


def linear_to_srgb_exact(c):
    """linear_to_srgb with pow evaluated in f64 and rounded once to f32 (the SMAA lumas: kernels_post.hip srgb1_exact)."""
    c = np.asarray(c, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        p = np.power(c.astype(np.float64), np.float64(SRGB_EXP)).astype(np.float32)
    return np.where(c <= f(0.0031308), c * f(12.92), f(1.055) * p - f(0.055)).astype(np.float32)


def khronos_neutral(c):
    c = np.asarray(c, dtype=np.float32)
    start, desat = f(0.8) - f(0.04), f(0.15)
    x = np.fmin(c[..., 0], np.fmin(c[..., 1], c[..., 2]))
    offset = np.where(x < f(0.08), x - f(6.25) * x * x, f(0.04)).astype(np.float32)
    r = c - offset[..., None]
    peak = np.fmax(r[..., 0], np.fmax(r[..., 1], r[..., 2]))
    d = F1 - start
    with np.errstate(divide="ignore", invalid="ignore"):
        new_peak = F1 - d * d / (peak + d - start)
        s = new_peak / peak
        rr = r * s[..., None]
        g = F1 - F1 / (desat * (peak - new_peak) + F1)
    out = mix(rr, new_peak[..., None], g[..., None])
    return np.where((peak < start)[..., None], r, out).astype(np.float32)


def aces(x):
    x = np.asarray(x, dtype=np.float32)
    num = x * (f(2.51) * x + f(0.03))
    den = x * (f(2.43) * x + f(0.59)) + f(0.14)
    with np.errstate(divide="ignore", invalid="ignore"):
        return clamp01(num / den)


def tone_map(rgb, op: int):
    if op == 1:
        return khronos_neutral(rgb)
    if op == 2:
        return aces(rgb)
    return np.asarray(rgb, dtype=np.float32)


def unorm8(v):
    v = np.nan_to_num(np.asarray(v, dtype=np.float32), nan=0.0)
    return np.floor(clamp01(v) * f(255.0) + f(0.5)).astype(np.uint8)


def display(effects_bits: np.ndarray, tonemapping: int) -> np.ndarray:
    """display_wgsl/fragment.wgsl on the stored effects texels: tone map, linear_to_srgb, unorm8; alpha (1.0) passes through."""
    rgb = f16_to_f32(effects_bits[..., :3])
    s = linear_to_srgb(tone_map(rgb, tonemapping))
    out = np.empty(effects_bits.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = unorm8(s)
    out[..., 3] = unorm8(f16_to_f32(effects_bits[..., 3]))
    return out


def _pad(img, r):
    return np.pad(img, ((r, r), (r, r)) + ((0, 0),) * (img.ndim - 2), mode="edge")


def _shift(padded, r, dx, dy, h, w):
    return padded[r + dy:r + dy + h, r + dx:r + dx + w]


def smaa(rgb):
    """helpers/smaa.wgsl with clamp-to-edge neighbours.  The lumas' power is taken in f64 and rounded once to f32, as the kernel does."""
    h, w = rgb.shape[:2]
    P = _pad(rgb, 1)
    L = luma(linear_to_srgb_exact(P))
    at = lambda dx, dy: _shift(P, 1, dx, dy, h, w)
    lat = lambda dx, dy: _shift(L, 1, dx, dy, h, w)
    cl = lat(0, 0)
    d = {k: np.abs(cl - lat(*k)) for k in [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]}
    max_h = np.fmax(d[(-1, 0)], d[(1, 0)])
    max_v = np.fmax(d[(0, -1)], d[(0, 1)])
    max_d = np.fmax(np.fmax(d[(-1, -1)], d[(1, -1)]), np.fmax(d[(-1, 1)], d[(1, 1)]))
    max_delta = np.fmax(np.fmax(max_h, max_v), max_d)
    edge = ~(max_delta < f(0.03))
    diag = max_d > np.fmax(max_h, max_v)
    horiz = max_h > max_v
    eps, s6 = f(0.001), f(0.6)
    with np.errstate(divide="ignore", invalid="ignore"):
        wtl, wtr, wbl, wbr = (F1 / (d[k] + eps) for k in [(-1, -1), (1, -1), (-1, 1), (1, 1)])
        tot = wtl + wtr + wbl + wbr
        ntl, ntr, nbl, nbr = wtl / tot, wtr / tot, wbl / tot, wbr / tot
        nb = at(-1, -1) * ntl[..., None] + at(1, -1) * ntr[..., None] + at(-1, 1) * nbl[..., None] + at(1, 1) * nbr[..., None]
        diag_out = mix(rgb, nb, s6)
        ca = np.where(horiz, d[(0, -1)], d[(-1, 0)])
        cb = np.where(horiz, d[(0, 1)], d[(1, 0)])
        wa, wb = F1 / (ca + eps), F1 / (cb + eps)
        t2 = wa + wb
        wa = wa / t2 * s6
        wb = wb / t2 * s6
    na = np.where(horiz[..., None], at(0, -1), at(-1, 0))
    nv = np.where(horiz[..., None], at(0, 1), at(1, 0))
    r = np.where((wa > F0)[..., None], mix(rgb, na, wa[..., None]), rgb)
    r = np.where((wb > F0)[..., None], mix(r, nv, wb[..., None]), r)
    out = np.where(diag[..., None], diag_out, r)
    return np.where(edge[..., None], out, rgb).astype(np.float32)


def dof_terms(depth, camera):
    """linearize_depth + calculate_coc (dof.wgsl) per pixel; camera = the 512-byte camera UBO as 128 f32."""
    cam = np.asarray(camera, dtype=np.float32)
    near, p22, p11 = cam[16 + 14], cam[16 + 10], cam[16 + 5]
    depth = np.asarray(depth, dtype=np.float32)
    if abs(p22) < f(0.0001):
        lin = near / np.fmax(depth, f(0.0001))
    else:
        far = near / (p22 + F1)
        lin = (near * far) / (far - depth * (far - near))
    S, N, fl = cam[124], cam[125], f(0.012) * p11
    A = fl / np.fmax(N, f(0.1))
    coc_world = A * fl * np.abs(lin - S) / (lin * np.fmax(S, f(0.001)))
    coc = np.fmin(np.fmax(coc_world * cam[123] / f(0.024), F0), f(16.0))
    return lin.astype(np.float32), coc.astype(np.float32)


def dof_blur(src, lin, coc):
    """apply_dof's disk blur and blend factor per pixel; returns (blur rgb, blend factor, pixel blurs?, ill-conditioned)."""
    h, w = coc.shape
    ys, xs = np.mgrid[0:h, 0:w]
    blur = np.zeros((h, w, 3), dtype=np.float32)
    total = np.zeros((h, w), dtype=np.float32)
    ill = np.abs(coc - f(0.5)) < 1e-5
    for i in range(16):
        ox, oy = DISK[i, 0] * coc, DISK[i, 1] * coc
        for o in (ox, oy):
            ill |= np.abs(np.abs(o - np.floor(o)) - 0.5) < 1e-5
        sx = np.clip(xs + np.rint(ox).astype(np.int64), 0, w - 1)
        sy = np.clip(ys + np.rint(oy).astype(np.int64), 0, h - 1)
        sc, sl, scoc = src[sy, sx], lin[sy, sx], coc[sy, sx]
        with np.errstate(divide="ignore", invalid="ignore"):
            wgt = np.where((sl > lin) & (scoc < coc), scoc / np.fmax(coc, f(0.01)), F1).astype(np.float32)
        dist = np.sqrt(ox * ox + oy * oy)
        wgt = wgt * (F1 - smoothstep(coc * f(0.5), coc, dist))
        wgt = np.fmax(wgt, f(0.01))
        blur = blur + sc * wgt[..., None]
        total = total + wgt
    blur = blur / np.fmax(total, f(0.01))[..., None]
    return blur.astype(np.float32), smoothstep(F0, f(2.0), coc), coc >= f(0.5), ill


def bloom_threshold(c):
    brightness = luma(c)
    contribution = np.fmax(brightness - f(0.8), F0)
    soft_threshold = f(0.8) * f(0.8)
    knee = f(0.8) - soft_threshold
    soft = clamp01((brightness - soft_threshold) / knee)
    factor = contribution / np.fmax(brightness, f(0.0001)) * soft
    return (c * factor[..., None]).astype(np.float32)


def blur13(img):
    h, w = img.shape[:2]
    P = _pad(img, 2)
    acc = np.zeros_like(img, dtype=np.float32)
    for (dx, dy), wt in zip(BLOOM_TAPS, BLOOM_W):
        acc = acc + _shift(P, 2, dx, dy, h, w) * wt
    return acc


def effects(composite_bits: np.ndarray, depth=None, camera=None, smaa_on=False, bloom=False, dof=False):
    """The effects pass (compute.wgsl): -> (effects RGBA16F bits, ill-conditioned DoF pixels)."""
    src = f16_to_f32(composite_bits[..., :3])
    h, w = src.shape[:2]
    ill = np.zeros((h, w), dtype=bool)
    if dof:
        lin, coc = dof_terms(depth, camera)
        db, bf, on, ill = dof_blur(src, lin, coc)
        apply_dof = lambda rgb: np.where(on[..., None], mix(rgb, db, bf[..., None]), rgb).astype(np.float32)
    else:
        apply_dof = lambda rgb: rgb
    if not bloom:
        rgb = apply_dof(smaa(src) if smaa_on else src)
    else:   # extract -> 3 blurs -> blend, every stage stored as f16 and mixed with the DoF blur; SMAA's result is ignored by apply_bloom
        stage = round_f16(apply_dof(blur13(bloom_threshold(src))))
        for _ in range(3):
            stage = round_f16(apply_dof(blur13(stage)))
        rgb = apply_dof(src + blur13(stage) * f(0.5))
        if ill.any():   # a differently rounded tap moves through the three blurs and the blend: 2 px per stage
            for _ in range(4):
                P = np.pad(ill, 2, mode="edge")
                ill = np.logical_or.reduce([P[2 + dy:2 + dy + h, 2 + dx:2 + dx + w] for dx, dy in BLOOM_TAPS])
    out = np.empty((h, w, 4), dtype=np.uint16)
    out[..., :3] = f32_to_f16(rgb)
    out[..., 3] = 0x3C00
    return out, ill
