"""Shadows from several views of one light restated in numpy, on tests/shadow_reference.py's operations: the resolve that picks each
pixel's view among K light blocks and K map layers, and the rule for the six faces of a cube around a point light in f64.

Test infrastructure.  As in shadow_reference.shadow every step is one numpy operation on arrays of one dtype: the `float32` run is the contract and
the device is held to its bits; the `float64` run is the same arithmetic for known answers.

    shadow_views(keys, block, W, H, maps, light_blocks, S, params, dtype)      steps 1, 2, 3', 4, 5, 6', 7', 8 per pixel
    cube_face_blocks(position, S, R, near, far)      the six blocks of a point light: +X, -X, +Y, -Y, +Z, -Z
    cascade_pair(S)                                  the known answer's two views of `zenith`: a tight window on the quad, then the block as it is
"""
import numpy as np

from tests import grid_reference as gr
from tests import shadow_reference as shr
from tests import ssao_reference as sr

MAX_VIEWS, NO_VIEW = 6, 255      # csrc/shadow.hpp: kMaxViews, kNoView
NO_HIT = shr.NO_HIT
FACE_AXES = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))


def _light_coords(lvp, Pw, hit, Sf, T):
    """Step 3 for one view, every pixel from its own Pw -> (u, v, z, inside)."""
    one, half, zero = T(1.0), T(0.5), T(0.0)
    q = tuple(shr._row(lvp, r, Pw[0], Pw[1], Pw[2]) for r in range(4))
    l0, l1, z = q[0] / q[3], q[1] / q[3], q[2] / q[3]
    u = (l0 * half + half) * Sf
    v = (half - l1 * half) * Sf
    inside = hit & (q[3] > zero) & (u >= zero) & (u < Sf) & (v >= zero) & (v < Sf) & (z >= zero) & (z <= one)
    # in front of the view and within its depth range, wherever (u, v) lie: what step 6' asks of a neighbour that another view holds
    front = hit & (q[3] > zero) & (z >= zero) & (z <= one) & (np.abs(u) < T(np.inf)) & (np.abs(v) < T(np.inf))
    return u, v, z, inside, front


def shadow_views(keys, block, W, H, maps, light_blocks, S, params=None, dtype=np.float32):
    """Every pixel of a W x H frame -> dict of [H, W] arrays: shadow_reference.shadow's (inside, u, v, z: in the pixel's view) and `view` (uint8, 255 = none)
    and `deep`.  maps: K layers of S x S keys; light_blocks: K blocks."""
    T = np.dtype(dtype).type
    p = dict(shr.DEFAULTS, **(params or {}))
    bias, slope_bias, max_slope, strength, facing_fade = (T(np.float32(p[k])) for k in ("bias", "slope_bias", "max_slope", "strength", "facing_fade"))
    light = [T(np.float32(c)) for c in p["light"]]
    R = int(p["pcf_radius"])
    K = len(light_blocks)
    assert 0 <= R <= shr.MAX_RADIUS and 1 <= S <= 8192 and 1 <= K <= MAX_VIEWS and len(maps) == K
    one, half, zero = T(1.0), T(0.5), T(0.0)
    d32, hit = sr.depth_and_hit(keys)
    assert d32.shape == (H, W)
    d = d32.astype(T)
    maps = np.stack([np.asarray(m, np.uint64).reshape(S, S) for m in maps])
    map_none = maps == NO_HIT
    map_d = (maps >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(T)
    ivp = shr._mat(block, 192, T)
    lvps = [shr._mat(lb, 128, T) for lb in light_blocks]
    cam = np.frombuffer(block, np.float32, 3, 384).astype(T)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Sf = T(S)
    with np.errstate(all="ignore"):
        # 2. world position
        nx = (px.astype(T) + half) * (T(2.0) / T(W)) - one
        ny = one - (py.astype(T) + half) * (T(2.0) / T(H))
        c = tuple(shr._row(ivp, r, nx, ny, d) for r in range(4))
        Pw = tuple(c[i] / c[3] for i in range(3))
        # 3'. every view's coordinates of every pixel; the pixel's view: the lowest deep one, else the lowest it is inside of, else none
        per_view = [_light_coords(lvp, Pw, hit, Sf, T) for lvp in lvps]
        M = T(R + 1)
        top = Sf - M
        view = np.full((H, W), NO_VIEW, np.int64)
        first_inside = np.full((H, W), NO_VIEW, np.int64)
        deep_any = np.zeros((H, W), bool)
        for i, (ui, vi, zi, ins, _) in enumerate(per_view):
            deep = ins & (ui >= M) & (ui < top) & (vi >= M) & (vi < top)
            view = np.where((view == NO_VIEW) & deep, i, view)
            first_inside = np.where((first_inside == NO_VIEW) & ins, i, first_inside)
            deep_any |= deep
        view = np.where(view == NO_VIEW, first_inside, view)
        has_view = view != NO_VIEW
        sel = lambda arrays, none: np.select([view == i for i in range(K)], arrays, none)
        u, v, z = (sel([pv[j] for pv in per_view], zero) for j in range(3))
        inside = has_view
        # 4. neighbours
        use_hf, has_h = shr._pick(d, hit, 0)
        use_vf, has_v = shr._pick(d, hit, 1)
        # 5. normal and facing
        h = tuple(shr._diff(Pw[i], use_hf, 0) for i in range(3))
        w = tuple(shr._diff(Pw[i], use_vf, 1) for i in range(3))
        n = (h[1] * w[2] - h[2] * w[1], h[2] * w[0] - h[0] * w[2], h[0] * w[1] - h[1] * w[0])
        e = tuple(cam[i] - Pw[i] for i in range(3))
        flip = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2] < zero
        n = tuple(np.where(flip, -n[i], n[i]) for i in range(3))
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        ln = np.sqrt(nn)
        n = tuple(n[i] / ln for i in range(3))
        if light[3] == zero:
            L = tuple(np.full((H, W), light[i]) for i in range(3))
        else:
            Lv = tuple(light[i] - Pw[i] for i in range(3))
            ll = np.sqrt((Lv[0] * Lv[0] + Lv[1] * Lv[1]) + Lv[2] * Lv[2])
            L = tuple(Lv[i] / ll for i in range(3))
        cos_t = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2]
        has_normal = has_h & has_v & (nn > zero)
        g = np.where(has_normal, np.where(cos_t > zero, np.fmin(one, cos_t / facing_fade), zero), one)
        # 6'. receiver plane: the neighbours' coordinates in the PIXEL's view, from their own Pw — view i's array at the neighbour.  A neighbour
        # serves in view i when it is inside view i, or when another view holds it and it lies in front of view i within its depth range
        held = sum(pv[3].astype(np.int64) for pv in per_view)
        serves = [pv[3] | (pv[4] & (held - pv[3].astype(np.int64) > 0)) for pv in per_view]
        plane = has_h & has_v & sel([shr._of_neighbour(sv_, use_hf, 0) & shr._of_neighbour(sv_, use_vf, 1) for sv_ in serves], False)
        uh, vh, zh = (sel([shr._diff(pv[j], use_hf, 0) for pv in per_view], zero) for j in range(3))
        uv, vv, zz = (sel([shr._diff(pv[j], use_vf, 1) for pv in per_view], zero) for j in range(3))
        det = uh * vv - vh * uv
        su = (zh * vv - zz * vh) / det
        sv = (zz * uh - zh * uv) / det
        sloped = plane & (np.abs(det) > T(np.float32(shr.DET_MIN))) & np.isfinite(su) & np.isfinite(sv)
        zu = np.where(sloped, np.fmin(np.fmax(su, -max_slope), max_slope), zero)
        zv = np.where(sloped, np.fmin(np.fmax(sv, -max_slope), max_slope), zero)
        # 7'. PCF in the view's layer
        layer = np.where(has_view, view, 0)
        iu = np.where(inside, np.floor(u), zero).astype(np.int64)
        iv = np.where(inside, np.floor(v), zero).astype(np.int64)
        tb = bias + slope_bias * (np.abs(zu) + np.abs(zv))
        lit = np.zeros((H, W), np.int64)
        for dy in range(-R, R + 1):
            ty = np.clip(iv + dy, 0, S - 1)
            cv = ((iv + dy).astype(T) + half) - v
            for dx in range(-R, R + 1):
                tx = np.clip(iu + dx, 0, S - 1)
                cu = ((iu + dx).astype(T) + half) - u
                zr = ((z + zu * cu) + zv * cv) - tb
                lit = lit + (map_none[layer, ty, tx] | (map_d[layer, ty, tx] >= zr)).astype(np.int64)
        V = np.where(inside, lit.astype(T) / T((2 * R + 1) * (2 * R + 1)), one)
        # 8. the multiplier
        m = np.where(hit, one - (strength * g) * (one - V), one)
    assert V.dtype == T and m.dtype == T and g.dtype == T
    return {"hit": hit, "inside": inside, "Pw": Pw, "u": u, "v": v, "z": z, "normal": n, "has_normal": has_normal, "cos": cos_t, "g": np.where(hit, g, one),
            "zu": zu, "zv": zv, "V": V, "m": m, "view": view.astype(np.uint8), "deep": deep_any & has_view}


# ------------------------------------------------------------------------------------------------ the views of the tests

def face_tan(S, R):
    """tan(fovy / 2) of a cube face: the 90-degree face lands on the layer's deep region [M, S - M)^2, M = R + 1; the rest is the apron the taps read."""
    return S / (S - 2.0 * (R + 1))


def cube_face_blocks(position, S, R, near=0.05, far=20.0):
    """A point light's six blocks in the order +X, -X, +Y, -Y, +Z, -Z: eye at the light, forward the axis, up +Y (+Z for the two Y faces: §19's rule),
    perspective of aspect 1."""
    assert S >= 16
    eye = np.asarray(position, np.float64)
    fovy_deg = float(np.degrees(2.0 * np.arctan(face_tan(S, R))))
    out = []
    for f in FACE_AXES:
        up = (0.0, 0.0, 1.0) if abs(f[1]) > 0.999 else (0.0, 1.0, 0.0)
        out.append(gr.camera_block(tuple(eye), tuple(eye + np.asarray(f)), S, S, fovy_deg=fovy_deg, near=near, far=far, up=up))
    return out


def point_light(position):
    return tuple(float(np.float32(c)) for c in position) + (1.0,)


def cascade_pair(S):
    """The cascade known answer's views of `zenith` over floating_quad, tightest first: a window of half height 1.75 centred on the quad, then the
    block as it is."""
    (xa, xb), (za, zb) = shr.QUAD["x"], shr.QUAD["z"]
    centre = (0.5 * (xa + xb), 0.0, 0.5 * (za + zb))
    return [shr.light_block("zenith", S, target=centre, ortho_half_height=1.75), shr.light_block("zenith", S)]


# ------------------------------------------------------------------------------------------------ the host's rules, in f64 (include/awsm_host.h)

def _look_to(eye, f):
    up = np.array([0.0, 0.0, 1.0]) if abs(f[1]) > 0.999 else np.array([0.0, 1.0, 0.0])
    s = shr._unit(np.cross(f, up))
    u = np.cross(s, f)
    return np.array([[s[0], u[0], -f[0], 0.0], [s[1], u[1], -f[1], 0.0], [s[2], u[2], -f[2], 0.0], [-(s @ eye), -(u @ eye), f @ eye, 1.0]])      # [col][row]


def _union(aabbs):
    return np.min([a for a, _ in aabbs], axis=0), np.max([b for _, b in aabbs], axis=0)


def host_cube_faces(light, aabbs, S, R):
    """A point light (a dict of SceneDesc.lights) -> six dicts(view, proj, view_proj: [col][row] f64), +X, -X, +Y, -Y, +Z, -Z."""
    eye = np.asarray(light["position"], np.float64)
    fa = float(light.get("range", 0.0))
    if not fa > 0.0:
        lo, hi = _union(aabbs)
        fa = max([np.linalg.norm(np.array([(hi if (k >> i) & 1 else lo)[i] for i in range(3)]) - eye) for k in range(8)] + [1.0])
    n = max(0.05, fa * 1e-3)
    proj = np.zeros((4, 4))
    proj[0][0] = proj[1][1] = 1.0 / face_tan(S, R)
    proj[2][2], proj[2][3], proj[3][2] = fa / (n - fa), -1.0, n * fa / (n - fa)
    out = []
    for f in FACE_AXES:
        view = _look_to(eye, np.asarray(f))
        out.append({"view": view, "proj": proj, "view_proj": (proj.T @ view.T).T, "eye": eye})
    return out


def camera_planes(cam_proj):
    """A camera projection ([col][row], depth 0 .. 1, right-handed) -> (near, far, orthographic)."""
    p = np.asarray(cam_proj, np.float64)
    ortho = p[3][3] != 0.0
    n = p[3][2] / p[2][2]
    f = (p[3][2] - 1.0) / p[2][2] if ortho else p[3][2] / (p[2][2] + 1.0)
    return n, f, ortho


def cascade_splits(n, f, N, lam, max_distance=0.0):
    fu = min(f, max_distance) if max_distance > 0.0 else f
    j = np.arange(N + 1) / N
    return lam * n * (fu / n) ** j + (1.0 - lam) * (n + (fu - n) * j)


def slice_corners(cam_view, cam_proj, d0, d1):
    """The eight world corners of the camera's frustum between view depths d0 and d1: on its corner rays."""
    v, p = np.asarray(cam_view, np.float64), np.asarray(cam_proj, np.float64)
    _, _, ortho = camera_planes(p)
    inv_view = np.linalg.inv(v.T)      # (the matrix these [col][row] arrays are the transpose of)
    out = []
    for d in (d0, d1):
        for ny in (-1.0, 1.0):
            for nx in (-1.0, 1.0):
                x, y = ((nx - p[3][0]) / p[0][0], (ny - p[3][1]) / p[1][1]) if ortho else ((nx + p[2][0]) * d / p[0][0], (ny + p[2][1]) * d / p[1][1])
                out.append((inv_view @ np.array([x, y, -d, 1.0]))[:3])
    return np.array(out)


def host_cascades(light, aabbs, cam_view, cam_proj, S, N, lam=0.5, max_distance=0.0):
    """A directional light under a camera -> N dicts(view, proj, view_proj, eye, r, window = (x, y), texel, corners), tightest first."""
    base = shr.host_light_camera(light, aabbs)
    view = base["view"]
    n, f, _ = camera_planes(cam_proj)
    d = cascade_splits(n, f, N, lam, max_distance)
    out = []
    for j in range(N):
        corners = slice_corners(cam_view, cam_proj, d[j], d[j + 1])
        c = corners.mean(axis=0)
        # (widened so that every corner lies M = 3 texels inside the window after the snap: r + 2 w / S <= w (1 - 6 / S))
        r = np.ceil(np.linalg.norm(corners - c, axis=1).max() * (S / (S - 8.0) if S > 16 else 2.0) * 16.0) / 16.0
        texel = 2.0 * r / S
        xy = np.floor((view.T @ np.append(c, 1.0))[:2] / texel) * texel
        proj = base["proj"].copy()
        proj[0][0] = proj[1][1] = 1.0 / r
        proj[3][0], proj[3][1] = -xy[0] / r, -xy[1] / r
        out.append({"view": view, "proj": proj, "view_proj": (proj.T @ view.T).T, "eye": base["eye"], "r": r, "window": xy, "texel": texel, "corners": corners})
    return out


def block_of(rule, S) -> bytes:
    """A 512-byte camera block from one of the dicts above (f64 view and proj, [col][row]): grid_reference.camera_block's layout and arithmetic."""
    view, proj = np.asarray(rule["view"], np.float64), np.asarray(rule["proj"], np.float64)
    mul = lambda a, b: (a.T @ b.T).T
    inv = lambda a: np.linalg.inv(a.T).T
    view_proj, inv_proj = mul(proj, view), inv(proj)
    rays = []
    for corner in ((-1, -1, 0, 1), (1, -1, 0, 1), (-1, 1, 0, 1), (1, 1, 0, 1)):
        v = inv_proj.T @ np.array(corner, np.float64)
        v = v[:3] / v[3]
        rays.append(np.append(v / np.linalg.norm(v), 0.0))
    f = np.concatenate([m.reshape(-1) for m in (view, proj, view_proj, inv(view_proj), inv_proj, inv(view))] + [np.append(np.asarray(rule["eye"], np.float64), 0.0)]).astype(np.float32)
    tail = np.concatenate(rays + [np.array([0.0, 0.0, S, S]), np.zeros(4)]).astype(np.float32)
    out = f.tobytes() + bytes(16) + tail.tobytes()
    assert len(out) == 512
    return out


SUN_LIGHT = {"kind": "directional", "direction": tuple(float(-c) for c in shr._SUN)}      # `sun` as a scene light


def host_sun_cascades(scene, S, N=4, lam=0.5, max_distance=0.0):
    """The host's N cascades of `sun` under a scene's camera, as blocks, tightest first."""
    return [block_of(w, S) for w in host_cascades(SUN_LIGHT, shr.scene_aabbs(scene), scene.view, scene.proj, S, N, lam, max_distance)]


def sun_windows(S, halves=(0.9, 1.6, 2.8, 4.6)):
    """Nested windows of `sun`, tightest first: one view matrix and one depth range (so depth, and with it bias, mean the same in every layer), an
    orthographic window of each half height around the boxes."""
    return [shr.light_block("sun", S, ortho_half_height=h) for h in halves]


# The point lights of the tests in `boxes`: high in the room and low in the corner.  Both stand on the corner's side of the boxes, so that the cameras
# see the shadows the boxes cast towards them (from (2.2, 2.4, 1.8), on the cameras' side, no pixel of the `perspective` frame is dark), and at least
# 0.45 away from the walls and the floor.
POINT_POSITIONS = ((0.6, 2.4, 0.6), (0.45, 0.5, 0.45))
