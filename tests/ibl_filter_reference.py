"""The numpy restatement of DESIGN.md section 13 (awsm_hip_env_cube_filter): the sample tables, the cube sampler, and the two filters.

The tables are built with Python's `math` in f64 — the operations of csrc/env_filter_table.hpp in the same order — and rounded to f32 once.  What
follows the table (the texel's frame, the sample directions, the cube lookups, the sums) runs in `dtype`: float64 is the reference the device is
held to, float32 is the device's own precision, used to check that the slack the device test grants is not spent by f32 alone.  Nothing here reads the
device code or the oracle; tests/test_env_filter_cpu.py checks the sampler against oracle.oracle_lib.sample_cube and the tables against the C++."""
import math

import numpy as np

GGX, LAMBERT = 0, 1

# the face across each edge of each face: sample_cube's seam rule (cube_seam.hpp kCubeEdge) — face' | swap << 3 | flip << 4 | far << 5 for the
# edges left (i = -1), right (i = N), up (j = -1), down (j = N)
CUBE_EDGE = np.array([[44, 13, 58, 43], [45, 12, 10, 27], [1, 16, 21, 4], [49, 32, 36, 53], [41, 8, 34, 3], [40, 9, 18, 51]], dtype=np.int64)


def radical_inverse(i: int) -> float:
    return int("{:032b}".format(i)[::-1], 2) * 2.3283064365386963e-10      # 2^-32


def sample_lod(pdf: float, samples: int, src_size: int) -> float:
    omega_p = 4.0 * math.pi / (6.0 * float(src_size) * float(src_size))
    lod = 0.5 * math.log2(1.0 / (float(samples) * pdf * omega_p)) + 1.0
    return lod if lod > 0.0 else 0.0


def table(kind: int, level: int, levels: int, samples: int, src_size: int) -> np.ndarray:
    """(n, 5) float32: GGX h.x h.y h.z N.L lod, entries with N.L <= 0 dropped — Lambert: the direction in the (T, B, n) frame, 1, lod."""
    r = float(level) / float(levels - 1) if kind == GGX else 1.0
    alpha = r * r
    a2 = alpha * alpha
    rows = []
    for i in range(samples):
        xi_x, xi_y = float(i) / float(samples), radical_inverse(i)
        phi = 2.0 * math.pi * xi_x
        if kind == GGX:
            c = math.sqrt((1.0 - xi_y) / (1.0 + (a2 - 1.0) * xi_y))
            s2 = 1.0 - c * c
            s_theta = math.sqrt(s2 if s2 > 0.0 else 0.0)
            w = 2.0 * (c * c) - 1.0
            if not w > 0.0:
                continue
            t = (c * c) * (a2 - 1.0) + 1.0
            pdf = (a2 / (math.pi * (t * t))) / 4.0
        else:
            c = math.sqrt(1.0 - xi_y)
            s_theta = math.sqrt(xi_y)
            w = 1.0
            pdf = c / math.pi
        rows.append((math.cos(phi) * s_theta, math.sin(phi) * s_theta, c, w, sample_lod(pdf, samples, src_size)))
    return np.array(rows, dtype=np.float64).reshape(-1, 5).astype(np.float32)


def mip_chain(level0: np.ndarray, mips: int):
    """The f16 chain awsm_hip_env_cube_generate_mips makes: 2x2 sums in f32, * 0.25, rounded to f16, each level from the one above."""
    chain = [np.ascontiguousarray(level0, dtype=np.float16)]
    for _ in range(1, mips):
        s = chain[-1].astype(np.float32)
        d = max(s.shape[1] >> 1, 1)
        acc = np.zeros((6, d, d, 4), dtype=np.float32)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            acc = acc + s[:, dy:2 * d:2, dx:2 * d:2]
        chain.append((acc * np.float32(0.25)).astype(np.float16))
    return chain


def texel_dirs(n: int, dtype=np.float64) -> np.ndarray:
    """(6, n, n, 3) [face][j][i]: the unit direction through each texel centre — the inverse of sample_cube's face table."""
    dt = np.dtype(dtype).type
    c = (dt(2.0) * (np.arange(n, dtype=dtype) + dt(0.5))) / dt(n) - dt(1.0)
    t, s = np.meshgrid(c, c, indexing="ij")      # row j -> t, column i -> s
    one = np.ones_like(s)
    faces = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]
    d = np.stack([np.stack(f, axis=-1) for f in faces]).astype(dtype)
    inv = dt(1.0) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return d * inv[..., None]


def _texel(level: np.ndarray, face, i, j):
    """Texel (i, j) of `face`, i and j in -1 .. N: off the face it comes from the face across that edge; a corner tap keeps its row."""
    n = level.shape[1]
    off_i = (i < 0) | (i >= n)
    j = np.where(off_i, np.clip(j, 0, n - 1), j)
    off = off_i | (j < 0) | (j >= n)
    e = np.where(i < 0, 0, np.where(i >= n, 1, np.where(j < 0, 2, 3)))
    t = CUBE_EDGE[face, e]
    k = np.where(e < 2, j, i)
    k = np.where(t & 16, n - 1 - k, k)
    far = np.where(t & 32, n - 1, 0)
    swap = (t & 8) != 0
    face2 = np.where(off, t & 7, face)
    i2 = np.where(off, np.where(swap, far, k), i)
    j2 = np.where(off, np.where(swap, k, far), j)
    return level[face2, j2, i2]


def _cube_level(level: np.ndarray, face, sn, tn, dtype):
    dt = np.dtype(dtype).type
    n = level.shape[1]
    x, y = sn * dt(n) - dt(0.5), tn * dt(n) - dt(0.5)
    x = np.minimum(np.where(x >= dt(-0.5), x, dt(-0.5)), dt(n) - dt(0.5))
    y = np.minimum(np.where(y >= dt(-0.5), y, dt(-0.5)), dt(n) - dt(0.5))
    flx, fly = np.floor(x), np.floor(y)
    fx, fy = (x - flx)[..., None], (y - fly)[..., None]
    i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
    lv = level.astype(dtype)
    c00, c10 = _texel(lv, face, i0, j0), _texel(lv, face, i0 + 1, j0)
    c01, c11 = _texel(lv, face, i0, j0 + 1), _texel(lv, face, i0 + 1, j0 + 1)
    one = dt(1.0)
    top, bot = c00 * (one - fx) + c10 * fx, c01 * (one - fx) + c11 * fx
    return top * (one - fy) + bot * fy


def sample_cube(levels, dirs, lods, dtype=np.float64) -> np.ndarray:
    """textureSampleLevel by sample_cube's contract: levels [(6, N_l, N_l, C)], dirs (..., 3), lods (...) -> (..., C) in `dtype`."""
    dt = np.dtype(dtype).type
    d = np.asarray(dirs, dtype=dtype)
    shape = d.shape[:-1]
    d = d.reshape(-1, 3)
    lod = np.broadcast_to(np.asarray(lods, dtype=dtype), shape).reshape(-1)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(dx), np.abs(dy), np.abs(dz)
    is_z = (az >= ax) & (az >= ay)
    is_y = ~is_z & (ay >= ax)
    face = np.where(is_z, np.where(dz < 0, 5, 4), np.where(is_y, np.where(dy < 0, 3, 2), np.where(dx < 0, 1, 0)))
    sc = np.where(is_z, np.where(dz < 0, -dx, dx), np.where(is_y, dx, np.where(dx < 0, dz, -dz)))
    tc = np.where(is_z, -dy, np.where(is_y, np.where(dy < 0, -dz, dz), -dy))
    ma = np.where(is_z, az, np.where(is_y, ay, ax))
    inv = dt(1.0) / ma
    sn, tn = dt(0.5) * (sc * inv) + dt(0.5), dt(0.5) * (tc * inv) + dt(0.5)
    top = len(levels) - 1
    lod = np.minimum(np.where(lod > 0, lod, dt(0.0)), dt(top))
    fl = np.floor(lod)
    fr = lod - fl
    l0 = fl.astype(np.int64)
    l1 = np.minimum(l0 + 1, top)
    blend = (fr > 0) & (l1 != l0)
    out = np.zeros((d.shape[0], levels[0].shape[-1]), dtype=dtype)
    for l in range(len(levels)):
        m = l0 == l
        if m.any():
            out[m] = _cube_level(levels[l], face[m], sn[m], tn[m], dtype)
    for l in range(1, len(levels)):
        m = blend & (l1 == l)
        if m.any():
            hi = _cube_level(levels[l], face[m], sn[m], tn[m], dtype)
            f = fr[m][:, None]
            out[m] = out[m] * (dt(1.0) - f) + hi * f
    return out.reshape(shape + (levels[0].shape[-1],))


def _frames(n_dirs: np.ndarray, dtype):
    dt = np.dtype(dtype).type
    up = np.where((np.abs(n_dirs[..., 2]) < dt(0.999))[..., None], np.array([0, 0, 1], dtype=dtype), np.array([1, 0, 0], dtype=dtype))
    t = np.cross(up, n_dirs).astype(dtype)
    t = t * (dt(1.0) / np.sqrt((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]))[..., None]
    return t, np.cross(n_dirs, t).astype(dtype)


def filter_level(src_levels, kind: int, n: int, tab: np.ndarray, samples: int, dtype=np.float64) -> np.ndarray:
    """One destination level of side n from its table: (6, n, n, 3) in `dtype`, not yet rounded to f16."""
    dt = np.dtype(dtype).type
    nd = texel_dirs(n, dtype).reshape(-1, 1, 3)
    t, b = _frames(nd, dtype)
    e = tab.astype(dtype)[None]                       # (1, cnt, 5)
    v = t * e[..., 0:1] + b * e[..., 1:2] + nd * e[..., 2:3]
    if kind == GGX:
        v = (dt(2.0) * e[..., 2:3]) * v - nd
    s = sample_cube(src_levels, v, np.broadcast_to(e[..., 4], v.shape[:-1]), dtype)[..., :3]
    w = e[..., 3:4]
    if kind == GGX:
        out = (w * s).sum(axis=1, dtype=dtype) / w.sum(axis=1, dtype=dtype)
    else:
        out = dt(math.pi / samples) * s.sum(axis=1, dtype=dtype)
    return out.reshape(6, n, n, 3)


def prefiltered(src_levels, size: int, mips: int, samples: int = 1024, dtype=np.float64):
    """The GGX chain: [level] of (6, n, n, 3).  Level 0 is the source's own texels, or the source resampled when the sides differ."""
    ns = src_levels[0].shape[1]
    if size == ns:
        out = [src_levels[0][..., :3].astype(dtype)]
    else:
        out = [sample_cube(src_levels, texel_dirs(size, dtype), np.dtype(dtype).type(max(0.0, math.log2(ns / size))), dtype)[..., :3]]
    for m in range(1, mips):
        out.append(filter_level(src_levels, GGX, max(size >> m, 1), table(GGX, m, mips, samples, ns), samples, dtype))
    return out


def irradiance(src_levels, size: int, samples: int = 1024, dtype=np.float64) -> np.ndarray:
    ns = src_levels[0].shape[1]
    return filter_level(src_levels, LAMBERT, size, table(LAMBERT, 0, 1, samples, ns), samples, dtype)


def f16_ulp(ref: np.ndarray) -> np.ndarray:
    """The spacing of f16 values in the binade of |ref| (the denormal spacing below 2^-14)."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10.0)


def smooth_hdr_source(n: int) -> np.ndarray:
    """(6, n, n, 4) float16: a vertical gradient plus a broad max(0, w.s)^8 lobe, values in [0.05, 10], alpha 1."""
    d = texel_dirs(n)
    s = np.array([0.48, 0.6, -0.64])
    lobe = np.maximum(0.0, d @ s) ** 8
    up = 0.5 + 0.5 * d[..., 1]
    rgb = np.stack([0.05 + 0.45 * up + 9.0 * lobe, 0.1 + 0.9 * up * up + 6.0 * lobe, 0.6 - 0.5 * up + 2.5 * lobe], axis=-1)
    assert rgb.min() >= 0.05 and rgb.max() <= 10.0
    return np.concatenate([rgb, np.ones(rgb.shape[:-1] + (1,))], axis=-1).astype(np.float16)
