"""The editor's ground grid restated in numpy from the 512-byte camera block alone (crates/editor/src/grid/shaders/grid.wgsl:100-231).

Test infrastructure.  Every step is one numpy operation on arrays of one dtype, so the `float32` run IS the contract — IEEE binary32, round to nearest
even, one rounding per operation, nothing fused — and the device is held to its bits; the `float64` run is the same arithmetic with 29 more bits, what
the f32 run is measured against.  Both read the same f32 block and the same f32 parameters.

    camera_block(eye, target, W, H, ...)   a block as CameraBuffer::update writes it (camera.rs:111-227, frustum rays :285-306)
    fragment(block, W, H, dtype, params)   per pixel: kept, rgba, depth, colour class, and what the decisions were taken from
    world_depth(keys)                      the f32 in the high half of the geometry pass's keys, 1.0 for "no hit"
    blend(opaque_bits, layer, depth)       the grid over the opaque image per sample, f16 at the blend, resolve4_f16's order under MSAA
"""
import numpy as np

# grid.wgsl:87-98, the fields of AwsmEditorGrid behind struct_size
DEFAULTS = {"color_background": (0.18, 0.18, 0.18), "alpha_background": 0.7, "color_minor": (0.28, 0.28, 0.28), "alpha_minor": 0.9,
            "color_major": (0.38, 0.38, 0.38), "alpha_major": 1.0, "color_z_axis": (0.3, 0.5, 0.95), "alpha_axis": 1.0,
            "color_x_axis": (0.95, 0.3, 0.3), "depth_epsilon": 1e-4}
BACKGROUND, MINOR, MAJOR, Z_AXIS, X_AXIS = range(5)      # colour classes, in the order the shader overwrites them
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)
# f32 run against f64 run over the issue's cameras and sizes, pixels near a decision threshold left out (near_threshold): four times the worst
# distance measured when the cases were written (tests/test_grid_cpu.py re-measures and prints them)
GRID_ALPHA_SLACK = 4 * 3.11e-5      # a line alpha, absolute; measured worst 3.109e-05 (`down` at 64x48: a minor line where fwidth is a few 1e-3)
GRID_DEPTH_SLACK = 4 * 1.19e-7      # the fragment's depth, absolute; measured worst 1.182e-07 (`below` at 67x45), two ulps of a depth just under 1.0
OFF = {"view": 0, "proj": 64, "inv_view_proj": 192, "inv_view": 320, "position": 384, "frustum_rays": 416}


# ------------------------------------------------------------------------------------------------ the camera block

def look_at_rh(eye, target, up=(0.0, 1.0, 0.0)):
    """glam Mat4::look_at_rh, [col][row], f64."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    return np.array([[s[0], u[0], -f[0], 0.0], [s[1], u[1], -f[1], 0.0], [s[2], u[2], -f[2], 0.0], [-eye @ s, -eye @ u, eye @ f, 1.0]])


def perspective_rh(fovy, aspect, near, far):
    """glam Mat4::perspective_rh (depth 0..1), [col][row]."""
    h = 1.0 / np.tan(0.5 * fovy)
    r = far / (near - far)
    m = np.zeros((4, 4))
    m[0][0], m[1][1], m[2][2], m[2][3], m[3][2] = h / aspect, h, r, -1.0, r * near
    return m


def orthographic_rh(half_width, half_height, near, far):
    """glam Mat4::orthographic_rh (depth 0..1) of a box centred on the view axis, [col][row]."""
    r = 1.0 / (near - far)
    m = np.zeros((4, 4))
    m[0][0], m[1][1], m[2][2] = 1.0 / half_width, 1.0 / half_height, r
    m[3] = [0.0, 0.0, r * near, 1.0]
    return m


def camera_block(eye, target, width, height, ortho_half_height=None, fovy_deg=50.0, near=0.1, far=100.0, up=(0.0, 1.0, 0.0)) -> bytes:
    """512 bytes: view 0, proj 64, view_proj 128, inv_view_proj 192, inv_proj 256, inv_view 320, position 384, frame count 400, frustum rays 416,
    viewport 480, dof 496.  Computed in f64, stored as f32 (matrices column-major: [col][row] flattened)."""
    view = look_at_rh(eye, target, up)
    aspect = width / height
    proj = orthographic_rh(ortho_half_height * aspect, ortho_half_height, near, far) if ortho_half_height else perspective_rh(np.radians(fovy_deg), aspect, near, far)
    mul = lambda a, b: (a.T @ b.T).T      # [col][row] storage: the product of the matrices these arrays are the transposes of
    inv = lambda a: np.linalg.inv(a.T).T
    view_proj, inv_proj = mul(proj, view), inv(proj)
    rays = []
    for corner in ((-1, -1, 0, 1), (1, -1, 0, 1), (-1, 1, 0, 1), (1, 1, 0, 1)):      # camera.rs:285-306
        v = inv_proj.T @ np.array(corner, np.float64)
        v = v[:3] / v[3]
        rays.append(np.append(v / np.linalg.norm(v), 0.0))
    f = np.concatenate([m.reshape(-1) for m in (view, proj, view_proj, inv(view_proj), inv_proj, inv(view))] + [np.append(np.asarray(eye, np.float64), 0.0)]).astype(np.float32)
    tail = np.concatenate(rays + [np.array([0.0, 0.0, width, height]), np.zeros(4)]).astype(np.float32)
    out = f.tobytes() + bytes(16) + tail.tobytes()
    assert len(out) == 512
    return out


# The issue's cameras: name -> arguments of camera_block after (width, height)
CAMERAS = {
    "down": dict(eye=(3.0, 2.0, 4.0), target=(0.0, 0.0, 0.0)),
    "horizon": dict(eye=(2.5, 1.5, 6.0), target=(0.0, 1.2, 0.0)),
    "below": dict(eye=(1.0, -2.0, 3.0), target=(0.0, 0.0, 0.0)),
    "up": dict(eye=(0.0, 1.0, 0.0), target=(0.3, 5.0, 1.0)),
    "ortho": dict(eye=(4.0, 5.0, 6.0), target=(0.0, 0.0, 0.0), ortho_half_height=6.0),
}
SIZES = ((64, 48), (67, 45))


def camera(name, width, height) -> bytes:
    return camera_block(width=width, height=height, **CAMERAS[name])


# ------------------------------------------------------------------------------------------------ the fragment

def _mat(block, byte, T):
    return np.frombuffer(block, np.float32, 16, byte).reshape(4, 4).astype(T)      # [col][row]


def _mul4(M, v):
    """M . v by columns: ((M0 v.x + M1 v.y) + M2 v.z) + M3 v.w, per row."""
    return tuple(((M[0][r] * v[0] + M[1][r] * v[1]) + M[2][r] * v[2]) + M[3][r] * v[3] for r in range(4))


def _mix(a, b, t, T):
    return a * (T(1.0) - t) + b * t


def _hit(block, W, H, px, py, T):
    """grid.wgsl:102-156 for pixel columns px and rows py (any integers, inside the frame or not) -> world_pos (x, y, z), ray_dir.y, t."""
    one, half, two, zero = T(1.0), T(0.5), T(2.0), T(0.0)
    nx = ((px.astype(T) + half) * two) / T(W) - one
    ny = one - ((py.astype(T) + half) * two) / T(H)
    if np.frombuffer(block, np.float32, 1, OFF["proj"] + 60)[0] > np.float32(0.9):
        M = _mat(block, OFF["inv_view_proj"], T)
        nh, fh = _mul4(M, (nx, ny, np.full_like(nx, zero), np.full_like(nx, one))), _mul4(M, (nx, ny, np.full_like(nx, one), np.full_like(nx, one)))
        origin = tuple(nh[i] / nh[3] for i in range(3))
        direction = tuple(fh[i] / fh[3] - origin[i] for i in range(3))
    else:
        ux, uy = (nx + one) * half, (ny + one) * half
        R = np.frombuffer(block, np.float32, 16, OFF["frustum_rays"]).reshape(4, 4).astype(T)
        bottom = tuple(_mix(R[0][i], R[1][i], ux, T) for i in range(3))
        top = tuple(_mix(R[2][i], R[3][i], ux, T) for i in range(3))
        ray = tuple(_mix(bottom[i], top[i], uy, T) for i in range(3))
        V = _mat(block, OFF["inv_view"], T)
        direction = tuple((V[0][r] * ray[0] + V[1][r] * ray[1]) + V[2][r] * ray[2] for r in range(3))
        pos = np.frombuffer(block, np.float32, 3, OFF["position"]).astype(T)
        origin = tuple(np.full_like(nx, pos[i]) for i in range(3))
    t = (zero - origin[1]) / direction[1]
    return tuple(origin[i] + direction[i] * t for i in range(3)), direction[1], t


def is_ortho(block) -> bool:
    return bool(np.frombuffer(block, np.float32, 1, OFF["proj"] + 60)[0] > np.float32(0.9))


def fragment(block, W, H, dtype=np.float32, params=None):
    """Every pixel of a W x H frame -> dict of [H, W] arrays: kept (bool), rgba [H, W, 4], depth, cls (colour class), the four line alphas `alphas`
    [H, W, 4] (minor, major, z axis, x axis), ray_dir_y and t.  rgba and depth are zero where the fragment is discarded."""
    T = np.dtype(dtype).type
    p = dict(DEFAULTS, **(params or {}))
    par = lambda k: T(np.float32(p[k]))                                        # the record holds f32
    col = lambda k: [T(np.float32(c)) for c in p[k]]
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        (cx, cy, cz), dir_y, t = _hit(block, W, H, px, py, T)
        (hx, _, hz), _, _ = _hit(block, W, H, px ^ 1, py, T)                   # the quad partners, each in full, before any branch
        (vx, _, vz), _, _ = _hit(block, W, H, px, py ^ 1, T)
        dx = np.abs(hx - cx) + np.abs(vx - cx)
        dz = np.abs(hz - cz) + np.abs(vz - cz)
        kept = ~((np.abs(dir_y) < T(0.001)) | ((not is_ortho(block)) & (t < T(0.0))))
        fract = lambda x: x - np.floor(x)
        line = lambda dist, alpha: (T(1.0) - np.fmin(dist, T(1.0))) * alpha
        half, ten = T(0.5), T(10.0)
        minor = line(np.fmin(np.abs(fract(cx - half) - half) / dx, np.abs(fract(cz - half) - half) / dz), par("alpha_minor"))
        major = line(np.fmin(np.abs(fract(cx / ten - half) - half) / (dx / ten), np.abs(fract(cz / ten - half) - half) / (dz / ten)), par("alpha_major"))
        x_axis = line(np.abs(cz) / dz, par("alpha_axis"))
        z_axis = line(np.abs(cx) / dx, par("alpha_axis"))
        cls = np.zeros((H, W), np.int32)
        alpha = np.full((H, W), par("alpha_background"))
        for k, a in ((MINOR, minor), (MAJOR, major), (Z_AXIS, z_axis), (X_AXIS, x_axis)):      # later wins
            on = a > T(0.01)
            cls = np.where(on, k, cls)
            alpha = np.where(on, a, alpha)
        colours = np.array([col("color_background"), col("color_minor"), col("color_major"), col("color_z_axis"), col("color_x_axis")], dtype=T)
        rgba = np.concatenate([colours[cls], alpha[..., None]], axis=-1)
        view_pos = _mul4(_mat(block, OFF["view"], T), (cx, cy, cz, np.full_like(cx, T(1.0))))
        clip = _mul4(_mat(block, OFF["proj"], T), view_pos)
        ndc_depth = clip[2] / clip[3]
        depth = np.fmin(np.fmax(ndc_depth + par("depth_epsilon"), T(0.0)), T(1.0))
    assert rgba.dtype == T and depth.dtype == T and cx.dtype == T
    return {"kept": kept, "rgba": np.where(kept[..., None], rgba, T(0.0)), "depth": np.where(kept, depth, T(0.0)), "cls": np.where(kept, cls, -1),
            "alphas": np.stack([minor, major, z_axis, x_axis], axis=-1), "ray_dir_y": dir_y, "t": t, "ndc_depth": ndc_depth, "world_pos": (cx, cy, cz)}


# ------------------------------------------------------------------------------------------------ the blend

def world_depth(keys):
    """[H, W] or [H, W, S] packed keys -> [H, W, S] f32: the depth in the high half, 1.0 (the clear value) for "no hit"."""
    keys = np.asarray(keys, np.uint64)
    if keys.ndim == 2:
        keys = keys[..., None]
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return np.where(keys == NO_HIT, np.float32(1.0), d)


def grid_passes(layer, depth_s):
    """[H, W, S] bool: the samples whose depth test (`Less` against the world depth) the pixel's fragment passes."""
    return layer["kept"][..., None] & (layer["depth"].astype(np.float32)[..., None] < depth_s)


def blend_samples(dst_bits, layer, depth_s):
    """dst_bits [H, W, 4] u16 (RGBA16F) -> [H, W, S, 4] f32 holding f16 values: every sample starts as dst, the grid goes over where it passes:
    rgb = f16(src.rgb * a + dst.rgb * (1 - a)), a = f16(a + dst.a * (1 - a)); products first, then the sum, all f32."""
    S = depth_s.shape[-1]
    dst = np.repeat(np.asarray(dst_bits, np.uint16).view(np.float16).astype(np.float32)[:, :, None, :], S, axis=2)
    src = layer["rgba"].astype(np.float32)[:, :, None, :]
    a = src[..., 3:4]
    om = np.float32(1.0) - a
    f16 = lambda x: x.astype(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        rgb = f16(src[..., :3] * a + dst[..., :3] * om)
        al = f16(a + dst[..., 3:4] * om)
    over = np.concatenate([rgb, al], axis=-1)
    return np.where(grid_passes(layer, depth_s)[..., None], over, dst)


def resolve(samples):
    """[H, W, S, 4] f32 -> RGBA16F bits [H, W, 4]: one sample as it is, four as resolve4_f16 adds them."""
    if samples.shape[2] == 1:
        out = samples[:, :, 0]
    else:
        with np.errstate(all="ignore"):
            out = (((samples[:, :, 0] + samples[:, :, 1]) + samples[:, :, 2]) + samples[:, :, 3]) * np.float32(0.25)
    return out.astype(np.float16).view(np.uint16)


def blend(opaque_bits, layer, depth_s):
    """The composite of a transparent pass with no fragments: the grid over the opaque image."""
    return resolve(blend_samples(opaque_bits, layer, depth_s))


def near_threshold(f64):
    """Pixels whose decisions the f32 run may take the other way: in f64, a line alpha within 1e-3 of 0.01, |ray_dir.y| within 1e-5 of 0.001, or |t| below 1e-5."""
    with np.errstate(all="ignore"):
        return (np.abs(f64["alphas"] - 0.01) < 1e-3).any(axis=-1) | (np.abs(np.abs(f64["ray_dir_y"]) - 0.001) < 1e-5) | (np.abs(f64["t"]) < 1e-5)
