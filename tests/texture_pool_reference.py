"""The texture pool's contract restated in numpy: what a texel becomes on its way into the pool, and the mip chain below it.
Used by tests/test_texture_pool_cpu.py and tests/test_texture_pool_gpu.py; nothing here calls the library."""
import math

import numpy as np

PREMULTIPLY_ALPHA, SRGB_TO_LINEAR = 1, 2


def srgb_to_linear_f64(q):
    c = q / 255.0
    return c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4)


def srgb_table():
    """256 bytes: floor(clamp(lin, 0, 1) * 255 + 0.5) of the f64 decode."""
    return np.array([int(math.floor(min(max(srgb_to_linear_f64(q), 0.0), 1.0) * 255.0 + 0.5)) for q in range(256)], dtype=np.uint8)


def srgb_table_f32():
    """The same through f32 arithmetic as the conversion shader writes it (convert_srgb.rs:52-76): select(pow((c + 0.055) / 1.055, 2.4), c / 12.92,
    c <= 0.04045), then the rgba8unorm store."""
    f = np.float32
    c = np.arange(256, dtype=np.float32) / f(255.0)
    lo = c / f(12.92)
    hi = np.power((c + f(0.055)) / f(1.055), f(2.4), dtype=np.float32)
    lin = np.where(c <= f(0.04045), lo, hi).astype(np.float32)
    return np.floor(np.clip(lin, f(0.0), f(1.0)) * f(255.0) + f(0.5)).astype(np.uint8)


def tie_distance():
    """Smallest distance of lin * 255 to a rounding tie (k + 0.5), and the q where it occurs."""
    d = [abs((srgb_to_linear_f64(q) * 255.0) % 1.0 - 0.5) for q in range(256)]
    q = int(np.argmin(d))
    return d[q], q


def premultiply(texels):
    """(..., 4) uint8 -> colour channels (2 c a + 255) // 510, alpha kept."""
    t = np.asarray(texels, dtype=np.uint8)
    a = t[..., 3:4].astype(np.uint32)
    out = t.copy()
    out[..., :3] = ((2 * t[..., :3].astype(np.uint32) * a + 255) // 510).astype(np.uint8)
    return out


def convert(texels, flags):
    """What awsm_hip_texture_array_write_layers stores for source texels (..., 4) uint8: premultiply first, decode second; alpha kept."""
    t = np.asarray(texels, dtype=np.uint8)
    if flags & PREMULTIPLY_ALPHA:
        t = premultiply(t)
    if flags & SRGB_TO_LINEAR:
        t = t.copy()
        t[..., :3] = srgb_table()[t[..., :3]]
    return t


def srgb_encode_exact(linear_bytes):
    """For bytes in the table's image: an sRGB byte that decodes to exactly that value (the smallest one)."""
    table = srgb_table()
    inverse = np.full(256, -1, dtype=np.int32)
    for q in range(255, -1, -1):
        inverse[table[q]] = q
    enc = inverse[np.asarray(linear_bytes, dtype=np.uint8)]
    assert (enc >= 0).all(), "a value outside the table's image has no exact encoding"
    return enc.astype(np.uint8)


def table_image():
    """The bytes some sRGB byte decodes to."""
    return np.unique(srgb_table())


def to_unorm8(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        pos = v > np.float32(0.0)                    # false for NaN
        c = np.minimum(np.where(pos, v, np.float32(0.0)), np.float32(1.0)).astype(np.float32)
        return np.where(pos, np.floor(c * np.float32(255.0) + np.float32(0.5)), np.float32(0.0)).astype(np.uint8)


def mip_level(src, kinds):
    """One level below (layers, h, w, 4) uint8, the arithmetic of kernels_texture.hip's tex_mip_filter (which k_gen_mip_level and k_tex_mips share)
    in f32: coordinates min(min(2x + k, 2 dw - 1), sw - 1), q / 255 by division, sums in k order, * 0.25, kind 1 renormalised, kind 2 root mean
    square of channel 1, tex_to_unorm8 with NaN -> 0."""
    f = np.float32
    layers, sh, sw, _ = src.shape
    dw, dh = max(sw >> 1, 1), max(sh >> 1, 1)
    xs = [np.minimum(np.minimum(2 * np.arange(dw) + k, 2 * dw - 1), sw - 1) for k in (0, 1)]
    ys = [np.minimum(np.minimum(2 * np.arange(dh) + k, 2 * dh - 1), sh - 1) for k in (0, 1)]
    r = [src[:, ys[k >> 1]][:, :, xs[k & 1]].astype(np.float32) / f(255.0) for k in range(4)]
    out = np.zeros((layers, dh, dw, 4), dtype=np.uint8)
    with np.errstate(invalid="ignore", divide="ignore"):
        for l in range(layers):
            s = np.zeros((dh, dw, 4), dtype=np.float32)
            if kinds[l] == 2:
                for k in range(4):
                    t = r[k][l].copy()
                    t[..., 1] = t[..., 1] * t[..., 1]
                    s = (s + t).astype(np.float32)
                o = (s * f(0.25)).astype(np.float32)
                o[..., 1] = np.sqrt(o[..., 1], dtype=np.float32)
            else:
                for k in range(4):
                    s = (s + r[k][l]).astype(np.float32)
                o = (s * f(0.25)).astype(np.float32)
                if kinds[l] == 1:
                    n = (o[..., :3] * f(2.0) - f(1.0)).astype(np.float32)
                    d = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]).astype(np.float32) + n[..., 2] * n[..., 2]).astype(np.float32)
                    inv = (f(1.0) / np.sqrt(d, dtype=np.float32)).astype(np.float32)
                    o[..., :3] = ((n * inv[..., None]).astype(np.float32) * f(0.5) + f(0.5)).astype(np.float32)
            out[l] = to_unorm8(o)
    return out


def mip_chain(level0, kinds):
    """[level0, level1, ...] down to 1 x 1, each level from the stored bytes of the level above."""
    chain = [np.ascontiguousarray(level0, dtype=np.uint8)]
    while chain[-1].shape[1] > 1 or chain[-1].shape[2] > 1:
        chain.append(mip_level(chain[-1], kinds))
    return chain
