"""Temporal anti-aliasing restated in numpy: the host's jitter and reprojection matrix, and the device's resolve.

Test infrastructure.  Every step of the resolve is one numpy operation on arrays of one dtype, so the `float32` run IS the contract — IEEE binary32,
round to nearest even, one rounding per operation, nothing fused, sums left to right — and the device is held to its bits; the `float64` run is the
same arithmetic with 29 more bits, for conditioning.  Both read the same f32 keys, the same RGBA16F images and the same f32 record.

    halton / jitter_ndc / moved      camera.rs:137-143, 257-274 in f32, as the host does it
    jitter_proj                      proj' = translation(jitter) * proj, glam's mul_mat4 in f32
    reproject                        R = view_proj_prev * inverse(view_proj_cur): glam's algorithms with every operation in f64, rounded once
    block                            the 512-byte camera block of a view and a projection (the oracle's writer)
    lookup(keys, rec, W, H)          per pixel: depth, the history position (sx, sy), whether it lies inside
    resolve(cur, keys, rec, hist)    per pixel: the resolved RGBA16F bits, (sx, sy), used
    Sequence                         frames one after another: each frame's output is the next one's history
"""
import numpy as np

from oracle import scene_model
from tests import grid_reference as gr

F = np.float32
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULT_FEEDBACK = 0.1
STRENGTH_STILL, STRENGTH_MOVING = 0.8, 0.2
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
SIZES = ((70, 45), (16, 16), (33, 70))


# ------------------------------------------------------------------------------------------------ the host's part

def halton(index, base):
    result, f = F(0.0), F(1.0)
    while index > 0:
        f = F(f / F(base))
        result = F(result + F(f * F(index % base)))
        index //= base
    return result


def jitter_ndc(frame_count, moved, W, H, strength_still=STRENGTH_STILL, strength_moving=STRENGTH_MOVING):
    """-> float32 [2]: (Halton(2, 3) - 0.5) / (W, H) * strength."""
    s = F(strength_moving if moved else strength_still)
    jx, jy = F(halton(frame_count, 2) - F(0.5)), F(halton(frame_count, 3) - F(0.5))
    return np.array([F(F(jx / F(W)) * s), F(F(jy / F(H)) * s)], dtype=F)


def moved(prev, view, proj, epsilon=1e-6):
    """prev: (view, proj) of the last frame or None.  camera.rs:120-135 (the comparison itself in f32)."""
    if prev is None:
        return True
    eps = F(epsilon)
    return bool((np.abs(np.asarray(prev[0], F) - np.asarray(view, F)) > eps).any() or (np.abs(np.asarray(prev[1], F) - np.asarray(proj, F)) > eps).any())


def _mul_vec4(m, v, T):
    res = m[0] * T(v[0])
    res = res + m[1] * T(v[1])
    res = res + m[2] * T(v[2])
    res = res + m[3] * T(v[3])
    return res


def _mul(a, b, T):
    """glam mul_mat4 on [col][row] arrays of dtype T."""
    return np.stack([_mul_vec4(a, b[c], T) for c in range(4)])


def jitter_proj(proj, jitter):
    """[col][row] f32 projection -> translation(jitter.x, jitter.y, 0) * proj in f32."""
    t = np.eye(4, dtype=F)
    t[3] = [jitter[0], jitter[1], 0.0, 1.0]
    out = _mul(t, np.asarray(proj, F).reshape(4, 4), F)
    assert out.dtype == F
    return out


def _inverse64(m):
    """glam Mat4::inverse on a [col][row] f64 array, operation for operation."""
    (m00, m01, m02, m03), (m10, m11, m12, m13), (m20, m21, m22, m23), (m30, m31, m32, m33) = m
    coef00, coef02, coef03 = m22 * m33 - m32 * m23, m12 * m33 - m32 * m13, m12 * m23 - m22 * m13
    coef04, coef06, coef07 = m21 * m33 - m31 * m23, m11 * m33 - m31 * m13, m11 * m23 - m21 * m13
    coef08, coef10, coef11 = m21 * m32 - m31 * m22, m11 * m32 - m31 * m12, m11 * m22 - m21 * m12
    coef12, coef14, coef15 = m20 * m33 - m30 * m23, m10 * m33 - m30 * m13, m10 * m23 - m20 * m13
    coef16, coef18, coef19 = m20 * m32 - m30 * m22, m10 * m32 - m30 * m12, m10 * m22 - m20 * m12
    coef20, coef22, coef23 = m20 * m31 - m30 * m21, m10 * m31 - m30 * m11, m10 * m21 - m20 * m11
    A = lambda *v: np.array(v, dtype=np.float64)  # noqa: E731
    fac0, fac1, fac2 = A(coef00, coef00, coef02, coef03), A(coef04, coef04, coef06, coef07), A(coef08, coef08, coef10, coef11)
    fac3, fac4, fac5 = A(coef12, coef12, coef14, coef15), A(coef16, coef16, coef18, coef19), A(coef20, coef20, coef22, coef23)
    vec0, vec1, vec2, vec3 = A(m10, m00, m00, m00), A(m11, m01, m01, m01), A(m12, m02, m02, m02), A(m13, m03, m03, m03)
    sign_a, sign_b = A(1, -1, 1, -1), A(-1, 1, -1, 1)
    inv = np.stack([((vec1 * fac0 - vec2 * fac1) + vec3 * fac2) * sign_a, ((vec0 * fac0 - vec2 * fac3) + vec3 * fac4) * sign_b,
                    ((vec0 * fac1 - vec1 * fac3) + vec3 * fac5) * sign_a, ((vec0 * fac2 - vec1 * fac4) + vec2 * fac5) * sign_b])
    dot1 = ((m[0][0] * inv[0][0] + m[0][1] * inv[1][0]) + m[0][2] * inv[2][0]) + m[0][3] * inv[3][0]
    return inv * (1.0 / dot1)


def reproject(prev, view, proj):
    """prev: (view, proj) of the last frame (f32, unjittered) or None -> float32 [16], column-major: the exact identity when there is no last
    frame or its matrices have the same bits."""
    view, proj = np.asarray(view, F).reshape(4, 4), np.asarray(proj, F).reshape(4, 4)
    if prev is None:
        return IDENTITY.copy()
    pv, pp = np.asarray(prev[0], F).reshape(4, 4), np.asarray(prev[1], F).reshape(4, 4)
    if pv.tobytes() == view.tobytes() and pp.tobytes() == proj.tobytes():
        return IDENTITY.copy()
    D = np.float64
    vp_prev = _mul(pp.astype(D), pv.astype(D), D)
    vp_cur = _mul(proj.astype(D), view.astype(D), D)
    r = _mul(vp_prev, _inverse64(vp_cur), D)
    assert r.dtype == D
    return r.astype(F).reshape(-1)


def block(view, proj, position, frame_count, W, H, dof=(0.0, 0.0)) -> bytes:
    return scene_model.camera_ubo(np.asarray(view, F).reshape(4, 4), np.asarray(proj, F).reshape(4, 4), position, frame_count, float(W), float(H), dof[0], dof[1])


def camera_matrices(eye, target, W, H, ortho_half_height=None, fovy_deg=50.0, near=0.1, far=100.0):
    """-> (view, proj) as [col][row] f32 (tests/grid_reference.py's f64 formulas, rounded once)."""
    view = gr.look_at_rh(eye, target)
    aspect = W / H
    proj = gr.orthographic_rh(ortho_half_height * aspect, ortho_half_height, near, far) if ortho_half_height else gr.perspective_rh(np.radians(fovy_deg), aspect, near, far)
    return view.astype(F), proj.astype(F)


def orbit(eye, target, degrees):
    """The eye turned about the vertical through the target."""
    e, t = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    a = np.radians(degrees)
    d = e - t
    return tuple(t + np.array([np.cos(a) * d[0] + np.sin(a) * d[2], d[1], -np.sin(a) * d[0] + np.cos(a) * d[2]]))


def record(feedback=DEFAULT_FEEDBACK, jitter=(0.0, 0.0), R=IDENTITY):
    return {"feedback": F(feedback), "jitter_ndc": np.asarray(jitter, F), "reproject": np.asarray(R, F).reshape(-1)}


# ------------------------------------------------------------------------------------------------ the device's part

def depth(keys):
    """[H, W] or [H, W, S] packed keys -> [H, W] f32: the least depth word of the samples, 1.0 for a sample that hit nothing."""
    keys = np.asarray(keys, np.uint64)
    if keys.ndim == 2:
        keys = keys[..., None]
    d_s = np.where(keys == NO_HIT, np.uint32(0x3F800000), (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    d = d_s[..., 0]
    for s in range(1, keys.shape[-1]):
        d = np.fmin(d, d_s[..., s])
    return d


def lookup(keys, rec, W, H, dtype=np.float32):
    """-> (sx, sy [H, W] of dtype: the history position in texel-index units; inside [H, W] bool: q.w > 0 and within half a texel of the image)."""
    T = np.dtype(dtype).type
    one, half = T(1.0), T(0.5)
    d = depth(keys).astype(T)
    assert d.shape == (H, W)
    R = np.asarray(rec["reproject"], np.float32).reshape(4, 4).astype(T)      # [col][row]
    jx, jy = T(F(rec["jitter_ndc"][0])), T(F(rec["jitter_ndc"][1]))
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fx, fy, fW, fH = px.astype(T), py.astype(T), T(W), T(H)
    with np.errstate(all="ignore"):
        nx = ((fx + half) * (T(2.0) / fW) - one) - jx
        ny = (one - (fy + half) * (T(2.0) / fH)) - jy
        qx, qy, qw = (((R[0][r] * nx + R[1][r] * ny) + R[2][r] * d) + R[3][r] for r in (0, 1, 3))
        vx, vy = qx / qw - nx, qy / qw - ny
        sx = fx + vx * (half * fW)
        sy = fy - vy * (half * fH)
        inside = (qw > T(0.0)) & (sx >= -half) & (sx <= fW - half) & (sy >= -half) & (sy <= fH - half)
    assert sx.dtype == T and sy.dtype == T
    return sx, sy, inside


def _shift(a, dy, dx):
    """a[y + dy, x + dx] with the coordinates clamped to the image."""
    H, W = a.shape[:2]
    return a[np.clip(np.arange(H) + dy, 0, H - 1)][:, np.clip(np.arange(W) + dx, 0, W - 1)]


def resolve(cur_bits, keys, rec, history_bits=None, dtype=np.float32):
    """cur_bits, history_bits: RGBA16F bits [H, W, 4] (history None: there is none) -> dict: resolved (uint16 [H, W, 4]), xy ([H, W, 2]), used
    ([H, W] bool), rgb (the mixed colour before the rounding to f16, of dtype; the current colour where the history was not used)."""
    T = np.dtype(dtype).type
    one = T(1.0)
    cur_bits = np.ascontiguousarray(cur_bits, np.uint16)
    H, W = cur_bits.shape[:2]
    sx, sy, inside = lookup(keys, rec, W, H, dtype)
    used = inside & (history_bits is not None)
    cur = cur_bits[..., :3].view(np.float16).astype(T)
    out = cur_bits.copy()
    rgb = cur.copy()
    if history_bits is not None:
        hist = np.ascontiguousarray(history_bits, np.uint16)[..., :3].view(np.float16).astype(T)
        with np.errstate(all="ignore"):
            fx0, fy0 = np.floor(sx), np.floor(sy)
            fx, fy = (sx - fx0)[..., None], (sy - fy0)[..., None]
            ix, iy = np.where(used, fx0, T(0.0)).astype(np.int64), np.where(used, fy0, T(0.0)).astype(np.int64)
            x0, x1, y0, y1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
            gx, gy = one - fx, one - fy
            w00, w10, w01, w11 = gx * gy, fx * gy, gx * fy, fx * fy
            h = ((hist[y0, x0] * w00 + hist[y0, x1] * w10) + hist[y1, x0] * w01) + hist[y1, x1] * w11
            lo = hi = _shift(cur, -1, -1)
            for k in range(1, 9):
                n = _shift(cur, k // 3 - 1, k % 3 - 1)
                lo, hi = np.fmin(lo, n), np.fmax(hi, n)
            h = np.fmin(np.fmax(h, lo), hi)
            fb = T(F(rec["feedback"]))
            mixed = h * (one - fb) + cur * fb
            assert mixed.dtype == T
            rgb = np.where(used[..., None], mixed, cur)
            out[..., :3] = np.where(used[..., None], mixed.astype(np.float16).view(np.uint16), cur_bits[..., :3])
    return {"resolved": out, "xy": np.stack([sx, sy], axis=-1), "used": used, "rgb": rgb}


class Sequence:
    """Frames one after another.  step(cur_bits, keys, rec) -> resolve()'s dict, with the last output as the history; reset() drops it."""

    def __init__(self, dtype=np.float32):
        self.dtype, self.history = dtype, None

    def reset(self):
        self.history = None

    def step(self, cur_bits, keys, rec):
        out = resolve(cur_bits, keys, rec, self.history, self.dtype)
        self.history = out["resolved"]
        return out
