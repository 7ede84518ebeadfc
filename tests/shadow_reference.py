"""Shadows restated in numpy: the resolve from the geometry pass's keys, the camera block, the light's map and the light block, and
the host's rules for the light camera and the casters restated in f64.

Test infrastructure.  Every step of `shadow` is one numpy operation on arrays of one dtype, so the `float32` run IS the contract — IEEE binary32,
round to nearest even, one rounding per operation, nothing fused, sums left to right, a matrix row ((m0 x + m1 y) + m2 z) + m3 w — and the device is
held to its bits; the `float64` run is the same arithmetic with 29 more bits, for known answers.

    LIGHTS / light_block / light_vec     the two lights of the tests: a camera block at the light, and AwsmShadow.light
    caster_map(model, block, S, draws)   the CPU oracle's raster of draws from a light block at S x S: what the device's map must equal
    shadow(keys, block, W, H, map_keys, light_block, S, params, dtype)      steps 1-8 per pixel
    apply / apply_f32                    step 8 on an RGBA16F image / the parity tap (tests/ssao_reference.py's: the same operation)
    host_light_camera / host_casters     the host layer's rules, in f64
"""
import numpy as np

from tests import grid_reference as gr
from tests import ssao_reference as sr

DEFAULTS = {"map_size": 2048, "pcf_radius": 1, "light": (0.0, 1.0, 0.0, 0.0), "bias": 1e-3, "slope_bias": 1.0, "max_slope": 0.05, "strength": 0.7,
            "facing_fade": 0.1}
TILE, WIN, MAX_RADIUS, DET_MIN = 16, 18, 2, 1e-12      # csrc/shadow.hpp
NO_HIT = sr.NO_HIT
BUF_CAMERA = 5
SIZES = sr.SIZES
MAP_SIZES = (40, 96, 200)
apply, apply_f32 = sr.apply, sr.apply_f32
SCENES, CAMERAS, camera, set_camera = sr.SCENES, sr.CAMERAS, sr.camera, sr.set_camera


# ------------------------------------------------------------------------------------------------ the lights of the tests

def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# name -> what the light block is made of, and the light vector.  Both look at the boxes standing in the corner from the side the cameras look from.
_SUN = _unit((0.45, 0.8, 0.35))
LIGHTS = {
    "sun": dict(kind="directional", towards=tuple(_SUN), target=(1.2, 0.4, 1.2), distance=8.0, ortho_half_height=4.6, near=0.5, far=20.0),
    "spot": dict(kind="spot", position=(3.0, 3.2, 2.2), target=(1.0, 0.0, 1.0), fovy_deg=70.0, near=0.5, far=20.0),
    # straight down on the floor (the known answer of floating_quad): a texel is 2 * 3.5 / S world units
    "zenith": dict(kind="directional", towards=(0.0, 1.0, 0.0), target=(1.5, 0.0, 1.5), distance=8.0, ortho_half_height=3.5, near=0.5, far=20.0, up=(0.0, 0.0, -1.0)),
}
QUAD = dict(x=(0.7, 2.7), z=(0.7, 2.7), y=1.0)      # floating_quad's quad: wide enough that floor lies under it by more than 3 texels of a 40 x 40 map


def floating_quad(width, height, camera_name="perspective"):
    """`corner` with a quad floating over its floor at y = 1, facing up."""
    from awsm_renderer_amd.scene_desc import NodeDesc
    sc = sr.corner(width, height, camera_name)
    (xa, xb), (za, zb), y = QUAD["x"], QUAD["z"], QUAD["y"]
    sc.nodes.append(NodeDesc(primitives=[sr._quad((xa, y, za), (0.0, 0.0, zb - za), (xb - xa, 0.0, 0.0), 1)]))
    return sc


def plane_light(camera_name="perspective", tilt=0.6):
    """A directional light the oblique `plane` faces, `tilt` off its normal: entries for light_block / light_vec."""
    du, dv = np.array([8.0, -2.0, -3.0]), np.array([-1.0, 6.0, -5.0])
    n = _unit(np.cross(du, dv))
    if n @ (np.array(sr.CAMERAS[camera_name]["eye"]) - np.array([0.6, 0.5, 0.6])) < 0:
        n = -n
    return dict(kind="directional", towards=tuple(_unit(n + tilt * _unit(du))), target=(0.6, 0.5, 0.6), distance=8.0, ortho_half_height=4.0, near=0.5, far=20.0)


def light_block(name, S, **moved) -> bytes:
    """The 512-byte camera block of a camera sitting at the light, for an S x S map.  moved: entries of LIGHTS[name] replaced."""
    L = dict(LIGHTS[name] if isinstance(name, str) else name, **moved)
    up = L.get("up", (0.0, 1.0, 0.0))
    if L["kind"] == "directional":
        target = np.asarray(L["target"], np.float64)
        eye = target + L["distance"] * _unit(L["towards"])
        return gr.camera_block(tuple(eye), tuple(target), S, S, ortho_half_height=L["ortho_half_height"], near=L["near"], far=L["far"], up=up)
    return gr.camera_block(L["position"], L["target"], S, S, fovy_deg=L["fovy_deg"], near=L["near"], far=L["far"], up=up)


def light_vec(name, **moved):
    """AwsmShadow.light: (unit vector towards the light, 0) or (position, 1); the unit vector rounded to f32 as the record holds it."""
    L = dict(LIGHTS[name] if isinstance(name, str) else name, **moved)
    if L["kind"] == "directional":
        return tuple(float(np.float32(c)) for c in _unit(L["towards"])) + (0.0,)
    return tuple(float(np.float32(c)) for c in L["position"]) + (1.0,)


def caster_map(model, block, S, draws=None, threads=8):
    """The CPU oracle's keys of `draws` (default: the model's opaque draws) seen from a light block at S x S — §3's raster, unchanged."""
    from oracle import oracle_lib
    mirrors = dict(model.mirrors())
    mirrors[BUF_CAMERA] = bytes(block)
    sc = model.scene
    draws = model.collect_draws() if draws is None else draws
    if not draws:
        return np.full((S, S), NO_HIT, np.uint64)
    fr = oracle_lib.OracleFrame(mirrors, draws, S, S, model.texture_arrays(), sc.samplers, oracle_lib.brdf_lut(4, 4))
    return np.asarray(fr.transform().raster(threads).keys, np.uint64).reshape(S, S).copy()


# ------------------------------------------------------------------------------------------------ steps 1-8

def _mat(block, byte, T):
    return np.frombuffer(block, np.float32, 16, byte).reshape(4, 4).astype(T)      # [col][row]


def _row(M, r, x, y, z):
    return ((M[0][r] * x + M[1][r] * y) + M[2][r] * z) + M[3][r]


def _pick(d, hit, axis):
    """Step 4 along one image axis -> (use the +1 neighbour, a neighbour exists).  The one inside the image and hit with the smaller |d(q) - d(p)|, the
    +1 one on a tie."""
    H, W = hit.shape
    dy, dx = (0, 1) if axis == 0 else (1, 0)
    idx = np.arange(W)[None, :] if axis == 0 else np.arange(H)[:, None]
    n = W if axis == 0 else H
    ok_f = (idx + 1 < n) & sr._shift(hit, dy, dx)
    ok_b = (idx - 1 >= 0) & sr._shift(hit, -dy, -dx)
    use_f = ok_f & (~ok_b | (np.abs(sr._shift(d, dy, dx) - d) <= np.abs(sr._shift(d, -dy, -dx) - d)))
    return use_f, ok_f | ok_b


def _diff(a, use_f, axis):
    """neighbour - p for the +1 neighbour, p - neighbour for the -1 one."""
    dy, dx = (0, 1) if axis == 0 else (1, 0)
    return np.where(use_f, sr._shift(a, dy, dx) - a, a - sr._shift(a, -dy, -dx))


def _of_neighbour(a, use_f, axis):
    dy, dx = (0, 1) if axis == 0 else (1, 0)
    return np.where(use_f, sr._shift(a, dy, dx), sr._shift(a, -dy, -dx))


def shadow(keys, block, W, H, map_keys, light_block, S, params=None, dtype=np.float32):
    """Every pixel of a W x H frame -> dict of [H, W] arrays: hit, inside, Pw (x, y, z), u, v, z, normal, has_normal, cos, g, zu, zv, V, m."""
    T = np.dtype(dtype).type
    p = dict(DEFAULTS, **(params or {}))
    bias, slope_bias, max_slope, strength, facing_fade = (T(np.float32(p[k])) for k in ("bias", "slope_bias", "max_slope", "strength", "facing_fade"))
    light = [T(np.float32(c)) for c in p["light"]]
    R = int(p["pcf_radius"])
    assert 0 <= R <= MAX_RADIUS and 1 <= S <= 8192
    one, half, zero = T(1.0), T(0.5), T(0.0)
    d32, hit = sr.depth_and_hit(keys)
    assert d32.shape == (H, W)
    d = d32.astype(T)
    map_keys = np.asarray(map_keys, np.uint64).reshape(S, S)
    map_none = map_keys == NO_HIT
    map_d = (map_keys >> np.uint64(32)).astype(np.uint32).view(np.float32).astype(T)
    ivp, lvp = _mat(block, 192, T), _mat(light_block, 128, T)
    cam = np.frombuffer(block, np.float32, 3, 384).astype(T)
    py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Sf = T(S)
    with np.errstate(all="ignore"):
        # 2. world position
        nx = (px.astype(T) + half) * (T(2.0) / T(W)) - one
        ny = one - (py.astype(T) + half) * (T(2.0) / T(H))
        c = tuple(_row(ivp, r, nx, ny, d) for r in range(4))
        Pw = tuple(c[i] / c[3] for i in range(3))
        # 3. light coordinates
        q = tuple(_row(lvp, r, Pw[0], Pw[1], Pw[2]) for r in range(4))
        l0, l1, z = q[0] / q[3], q[1] / q[3], q[2] / q[3]
        u = (l0 * half + half) * Sf
        v = (half - l1 * half) * Sf
        inside = hit & (q[3] > zero) & (u >= zero) & (u < Sf) & (v >= zero) & (v < Sf) & (z >= zero) & (z <= one)
        # 4. neighbours
        use_hf, has_h = _pick(d, hit, 0)
        use_vf, has_v = _pick(d, hit, 1)
        # 5. normal and facing
        h = tuple(_diff(Pw[i], use_hf, 0) for i in range(3))
        w = tuple(_diff(Pw[i], use_vf, 1) for i in range(3))
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
        # 6. receiver plane
        plane = has_h & has_v & _of_neighbour(inside, use_hf, 0) & _of_neighbour(inside, use_vf, 1)
        uh, vh, zh = (_diff(a, use_hf, 0) for a in (u, v, z))
        uv, vv, zz = (_diff(a, use_vf, 1) for a in (u, v, z))
        det = uh * vv - vh * uv
        su = (zh * vv - zz * vh) / det
        sv = (zz * uh - zh * uv) / det
        sloped = plane & (np.abs(det) > T(np.float32(DET_MIN))) & np.isfinite(su) & np.isfinite(sv)
        zu = np.where(sloped, np.fmin(np.fmax(su, -max_slope), max_slope), zero)
        zv = np.where(sloped, np.fmin(np.fmax(sv, -max_slope), max_slope), zero)
        # 7. PCF
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
                lit = lit + (map_none[ty, tx] | (map_d[ty, tx] >= zr)).astype(np.int64)
        V = np.where(inside, lit.astype(T) / T((2 * R + 1) * (2 * R + 1)), one)
        # 8. the multiplier
        m = np.where(hit, one - (strength * g) * (one - V), one)
    assert V.dtype == T and m.dtype == T and g.dtype == T
    return {"hit": hit, "inside": inside, "Pw": Pw, "u": u, "v": v, "z": z, "normal": n, "has_normal": has_normal, "cos": cos_t, "g": np.where(hit, g, one),
            "zu": zu, "zv": zv, "V": V, "m": m}


# ------------------------------------------------------------------------------------------------ the host's rules, in f64

def scene_aabbs(scene):
    """World boxes (min, max; f64) of the shadow candidates of a scene whose nodes are translated and scaled only: the opaque, non-HUD primitives."""
    out = []
    for node in scene.nodes:
        assert tuple(getattr(node, "rotation", (0, 0, 0, 1))) == (0, 0, 0, 1) and not getattr(node, "children", None)
        t, s = np.asarray(node.translation, np.float64), np.asarray(node.scale, np.float64)
        for prim in node.primitives:
            p = np.asarray(prim.positions, np.float64) * s + t
            out.append((p.min(axis=0), p.max(axis=0)))
    return out


def host_light_camera(light, aabbs):
    """A scene light (the dicts of SceneDesc.lights) and the candidates' world boxes -> dict(view, proj, view_proj: [col][row] f64 4 x 4; eye;
    light: AwsmShadow.light).  include/awsm_host.h states the rules."""
    f = _unit(light["direction"])
    up = np.array([0.0, 0.0, 1.0]) if abs(f[1]) > 0.999 else np.array([0.0, 1.0, 0.0])
    lo = np.min([a for a, _ in aabbs], axis=0) if aabbs else np.zeros(3)
    hi = np.max([b for _, b in aabbs], axis=0) if aabbs else np.zeros(3)
    proj = np.zeros((4, 4))
    if light.get("kind", "directional") == "directional":
        c, r = (0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)) if aabbs else (np.zeros(3), 1.0)
        r = r if r > 0 else 1.0
        eye, n, fa = c - 2.0 * r * f, r, 3.0 * r
        proj[0][0] = proj[1][1] = 1.0 / r
        proj[2][2], proj[3][2], proj[3][3] = 1.0 / (n - fa), n / (n - fa), 1.0
        vec = tuple(-f) + (0.0,)
    else:
        assert light["kind"] == "spot"
        eye = np.asarray(light["position"], np.float64)
        fa = float(light.get("range", 0.0))
        if not fa > 0.0:
            corners = [np.array([(hi if (k >> i) & 1 else lo)[i] for i in range(3)]) for k in range(8)] if aabbs else []
            fa = max([np.linalg.norm(p - eye) for p in corners] + [1.0])
        n = max(0.05, fa * 1e-3)
        cone = np.arccos(min(max(float(np.float32(light["outer_angle"])), -1.0), 1.0))      # the field holds the cosine of the cone's half angle
        fovy = min(max(2.0 * cone, np.pi / 180.0), 170.0 * np.pi / 180.0)
        t = 1.0 / np.tan(0.5 * fovy)
        proj[0][0] = proj[1][1] = t
        proj[2][2], proj[2][3], proj[3][2] = fa / (n - fa), -1.0, n * fa / (n - fa)
        vec = tuple(eye) + (1.0,)
    s = _unit(np.cross(f, up))
    u = np.cross(s, f)
    view = np.array([[s[0], u[0], -f[0], 0.0], [s[1], u[1], -f[1], 0.0], [s[2], u[2], -f[2], 0.0], [-(s @ eye), -(u @ eye), f @ eye, 1.0]])
    view_proj = (proj.T @ view.T).T
    return {"view": view, "proj": proj, "view_proj": view_proj, "eye": eye, "light": vec}


def host_casters(view_proj, aabbs):
    """Which candidates cast: the boxes that meet the frustum of view_proj ([col][row]; frustum.rs's planes and its positive-vertex test), in f64."""
    M = np.asarray(view_proj, np.float64).T      # rows
    planes = [M[3] + M[0], M[3] - M[0], M[3] + M[1], M[3] - M[1], M[2], M[3] - M[2]]
    keep = []
    for i, (a, b) in enumerate(aabbs):
        ok = True
        for pl in planes:
            n = pl[:3]
            ln = np.linalg.norm(n)
            pt = np.where(n >= 0, b, a)
            ok = ok and (n @ pt + pl[3]) / (ln if ln > 0 else 1.0) >= 0.0
        if ok:
            keep.append(i)
    return keep
