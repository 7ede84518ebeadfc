"""The numpy restatement of DESIGN.md section 16 (awsm_hip_env_cube_from_equirect): an equirectangular panorama projected into level 0 of a cube.

project() follows the contract step by step in the dtype it is given: float64 is the reference the device is held to; float32 is the run the
tolerance is derived from (tests/test_equirect_cpu.py).  Nothing here is shared with the library."""
import math

import numpy as np

HALF_ONE = 0x3C00
F16_MAX = 65504.0


def auto_samples(width, n):
    """S = clamp(ceil(W / (4 N)), 1, 8): panorama pixels per cube texel along the equator."""
    return int(min(8, max(1, -(-int(width) // (4 * int(n))))))


def face_dir(face, s, t):
    """Section 13's face table: the (unnormalised) direction through (s, t) of `face`, +X -X +Y -Y +Z -Z."""
    one = np.ones_like(s)
    return [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)][face]


def decode(pano, dtype=np.float64):
    """uint8 [H, W, 4] RGBE -> m * 2^(e - 136), black when e == 0; float32 [H, W, 4] -> its first three channels.  Exact in either dtype."""
    pano = np.asarray(pano)
    if pano.dtype == np.uint8:
        e = pano[..., 3].astype(np.int64)
        rgb = np.where((e == 0)[..., None], 0.0, np.ldexp(pano[..., :3].astype(np.float64), (e - 136)[..., None]))
        return rgb.astype(dtype)
    assert pano.dtype == np.float32 and pano.shape[-1] == 4
    return pano[..., :3].astype(dtype)


def direction_to_uv(d, yaw=0.0, dtype=np.float64):
    """u = atan2(d.x, -d.z) / 2 pi + 0.5 + yaw / 2 pi reduced to [0, 1]; v = acos(clamp(d.y, -1, 1)) / pi.  yaw / 2 pi is reduced in f64 first, as the
    library does on the host."""
    turns = float(np.float32(yaw)) / (2.0 * math.pi)
    turn = dtype(turns - math.floor(turns))
    u = np.arctan2(d[0], -d[2]).astype(dtype) * dtype(1.0 / (2.0 * math.pi)) + dtype(0.5) + turn
    u = u - np.floor(u)
    v = np.arccos(np.clip(d[1], dtype(-1.0), dtype(1.0))).astype(dtype) * dtype(1.0 / math.pi)
    return u, v


def lookup(rgb, u, v, dtype=np.float64):
    """Section 3's texel rule on the panorama: x = u W - 0.5, y = v H - 0.5, bilinear; columns wrap, rows clamp; mix(a, b, t) = a (1 - t) + b t,
    first in x and then in y."""
    h, w = rgb.shape[:2]
    x, y = u * dtype(w) - dtype(0.5), v * dtype(h) - dtype(0.5)
    flx, fly = np.floor(x), np.floor(y)
    fx, fy = (x - flx)[..., None], (y - fly)[..., None]
    x0 = flx.astype(np.int64)
    c0, c1 = x0 % w, (x0 + 1) % w
    y0 = fly.astype(np.int64)
    r0, r1 = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    one = dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = rgb[r0, c0] * (one - fx) + rgb[r0, c1] * fx
        bot = rgb[r1, c0] * (one - fx) + rgb[r1, c1] * fx
        return top * (one - fy) + bot * fy


def project(pano, n, samples=0, yaw=0.0, scale=1.0, dtype=np.float64):
    """-> [6, n, n, 3] in `dtype`: the values the store rounds to f16 (NaN already 0, clamped to +-65504)."""
    rgb = decode(pano, dtype)
    S = samples if samples else auto_samples(rgb.shape[1], n)
    assert 1 <= S <= 8
    scale = dtype(1.0 if float(np.float32(scale)) == 0.0 else np.float32(scale))
    j, i = np.meshgrid(np.arange(n, dtype=dtype), np.arange(n, dtype=dtype), indexing="ij")
    out = np.zeros((6, n, n, 3), dtype=dtype)
    two, half, one = dtype(2.0), dtype(0.5), dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for face in range(6):
            total = np.zeros((n, n, 3), dtype=dtype)
            for b in range(S):
                t = (two * (j + (dtype(b) + half) / dtype(S))) / dtype(n) - one
                for a in range(S):
                    s = (two * (i + (dtype(a) + half) / dtype(S))) / dtype(n) - one
                    dx, dy, dz = face_dir(face, s, t)
                    inv = one / np.sqrt((dx * dx + dy * dy) + dz * dz)
                    u, v = direction_to_uv((dx * inv, dy * inv, dz * inv), yaw, dtype)
                    total = total + lookup(rgb, u, v, dtype)
            value = (total * (one / (dtype(S) * dtype(S)))) * scale
            value = np.where(np.isnan(value), dtype(0.0), value)
            out[face] = np.clip(value, dtype(-F16_MAX), dtype(F16_MAX))
    assert out.dtype == dtype
    return out


def f16_bits(values):
    """[6, n, n, 3] -> uint16 [6, n, n, 4]: one rounding to nearest even, alpha 1.0."""
    out = np.full(values.shape[:-1] + (4,), HALF_ONE, dtype=np.uint16)
    out[..., :3] = np.asarray(values, dtype=np.float64).astype(np.float16).view(np.uint16)
    return out


def f16_ulp(ref):
    """The spacing of f16 in the binade of |ref| (2^-24 below the normal range)."""
    a = np.maximum(np.abs(np.asarray(ref, dtype=np.float64)), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(a)) - 10.0)


def pixel_dirs(width, height):
    """[H, W, 3]: the direction a panorama pixel's centre looks in — the inverse of direction_to_uv at yaw 0."""
    u = (np.arange(width) + 0.5) / width
    v = (np.arange(height) + 0.5) / height
    phi, theta = (u[None, :] - 0.5) * 2.0 * math.pi, v[:, None] * math.pi
    return np.stack([np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi), -np.sin(theta) * np.cos(phi)], axis=-1)


# the colours of the axis-painted panorama: +X -X +Y -Y +Z -Z, each a handful of f16 bits
AXIS_COLORS = np.array([[1.0, 0.125, 0.125], [0.25, 2.0, 2.0], [0.125, 1.0, 0.125], [2.0, 0.25, 2.0], [0.125, 0.125, 1.0], [2.0, 2.0, 0.25]])


def axis_painted(width, height):
    """float32 [H, W, 4]: every pixel has the colour of the dominant axis of its own direction."""
    d = pixel_dirs(width, height)
    axis = np.abs(d).argmax(axis=-1)
    face = 2 * axis + (np.take_along_axis(d, axis[..., None], axis=-1)[..., 0] < 0)
    out = np.ones((height, width, 4), dtype=np.float32)
    out[..., :3] = AXIS_COLORS[face]
    return out


SMOOTH_LOBE = np.array([0.48, 0.6, -0.64])      # a unit vector off every axis


def smooth_radiance(d):
    """A gradient plus a max(0, d . s)^8 lobe, per channel, in [0.05, 10] for unit d."""
    d = np.asarray(d, dtype=np.float64)
    lobe = np.maximum(0.0, d @ SMOOTH_LOBE) ** 8
    grad = np.stack([0.55 + 0.5 * d[..., 1], 0.8 + 0.4 * d[..., 0] - 0.3 * d[..., 2], 1.05 - 0.6 * d[..., 1] + 0.35 * d[..., 2]], axis=-1)
    return grad + lobe[..., None] * np.array([8.0, 6.5, 4.0])


def smooth_panorama(width, height, fmt):
    """The smooth source sampled at the pixel centres: fmt "rgbe" -> uint8 [H, W, 4], "f32" -> float32 [H, W, 4] (alpha 7: it must be ignored)."""
    from tests.rgbe_files import float_to_rgbe
    rgb = smooth_radiance(pixel_dirs(width, height))
    if fmt == "rgbe":
        return float_to_rgbe(rgb)
    out = np.full((height, width, 4), 7.0, dtype=np.float32)
    out[..., :3] = rgb
    return out
