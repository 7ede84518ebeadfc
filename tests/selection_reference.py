"""The editor's selection overlay restated in numpy from the geometry pass's keys, the draw list and the 512-byte camera block.

Test infrastructure.  Every step is one numpy operation on arrays of one dtype, so the `float32` run IS the contract — IEEE binary32, round to nearest
even, one rounding per operation, nothing fused, sums left to right — and the device is held to its bits; the `float64` run is the same arithmetic
with 29 more bits.  Both read the same keys, the same f32 block, the same f32 boxes and the same f32 record.

    SCENES / CAMERAS / SIZES / camera / set_camera   tests/ssao_reference.py's, by import
    draw_table(draws, mirrors)       per DrawDev of a draw list (an instanced draw is one per instance): first triangle rank and mesh key words
    selected_draws(table, keys)      step 1: one byte per DrawDev
    pixels(vis, table, sel)          step 2: s(p) and d(p)
    ring(s, R)                       step 3
    edges(boxes, block, W, H)        step 4: [n_boxes, 12, 8] records
    box_alpha(edges, d, W, H, rec)   steps 5 and 6
    blend / blend_f32                step 7 on RGBA16F bits / on the f32 tap
    overlay(...)                     all of it -> dict of layers
"""
import struct

import numpy as np

from tests.ssao_reference import CAMERAS, SCENES, SIZES, camera, set_camera  # noqa: F401  (re-exported)

OUTLINE, BOXES = 1, 2
MAX_KEYS = MAX_BOXES = 64
DEFAULTS = {"flags": OUTLINE | BOXES, "outline_radius": 2, "outline_color": (1.0, 0.6, 0.1, 1.0), "box_color": (1.0, 0.6, 0.1, 0.9), "box_half_width": 0.75,
            "hidden_alpha": 0.25, "depth_epsilon": 1e-5}
NO_HIT = np.uint64(0xFFFFFFFFFFFFFFFF)
BUF_GEOM_META, BUF_MATERIAL_META = 10, 11

# the 12 edges of a box as corner pairs (k, k | 1 << a): by axis a = 0, 1, 2, then k ascending over the corners without bit a
EDGE_CORNERS = [(k, k | (1 << a)) for a in range(3) for k in range(8) if not k & (1 << a)]


def record(**overrides):
    bad = set(overrides) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **overrides)


def key_words(mesh_keys):
    """64-bit mesh keys -> [(high, low)] as the picker reports them."""
    return [((int(k) >> 32) & 0xFFFFFFFF, int(k) & 0xFFFFFFFF) for k in mesh_keys]


# ------------------------------------------------------------------------------------------------ steps 1 and 2

def draw_table(draws, mirrors):
    """The WORLD geometry pass's draw list as the device expands it -> (first_tri [n] int64, words [n, 2] uint32): a draw without triangles is dropped,
    an instanced draw gives one entry per instance; the key words are read as k_pick reads them: geometry meta + 36 -> material mesh meta words 0, 1."""
    gm, mm = mirrors[BUF_GEOM_META], mirrors[BUF_MATERIAL_META]
    first, words, tris = [], [], 0
    for d in draws:
        if d["tri_count"] == 0:
            continue
        off = struct.unpack_from("<I", gm, d["geom_meta_off"] + 36)[0] // 256 * 256
        w = struct.unpack_from("<2I", mm, off)
        for _ in range(d.get("inst_count", 0) or 1):
            first.append(tris)
            words.append(w)
            tris += d["tri_count"]
    return np.array(first, np.int64), np.array(words, np.uint32).reshape(-1, 2)


def selected_draws(table, keys):
    """Step 1 -> one bool per DrawDev: its key words equal some listed (high, low)."""
    _, words = table
    sel = np.zeros(len(words), bool)
    for hi, lo in keys:
        sel |= (words[:, 0] == np.uint32(hi)) & (words[:, 1] == np.uint32(lo))
    return sel


def pixels(vis, table, sel):
    """Step 2: [H, W] or [H, W, S] packed keys -> (s [H, W] bool: some sample shows a triangle of a selected draw; d [H, W] f32: the depth word, the
    least over the samples that hit, 1.0 where none did)."""
    vis = np.asarray(vis, np.uint64)
    if vis.ndim == 2:
        vis = vis[..., None]
    hit = vis != NO_HIT
    d_s = (vis >> np.uint64(32)).astype(np.uint32).view(np.float32)
    d = np.where(hit, d_s, np.float32(np.inf)).min(axis=-1)
    d = np.where(hit.any(axis=-1), d, np.float32(1.0)).astype(np.float32)
    first, _ = table
    s = np.zeros(vis.shape[:2], bool)
    if len(first):
        rank = (np.uint64(0xFFFFFFFF) - (vis & np.uint64(0xFFFFFFFF))).astype(np.int64)
        draw = np.clip(np.searchsorted(first, rank, side="right") - 1, 0, len(first) - 1)
        s = (hit & sel[draw]).any(axis=-1)
    return s, d


# ------------------------------------------------------------------------------------------------ step 3

def ring(s, R, outline=True):
    """Unselected pixels with a selected pixel inside the image at integer distance^2 <= R^2."""
    H, W = s.shape
    near = np.zeros((H, W), bool)
    if outline:
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if dx * dx + dy * dy > R * R:
                    continue
                shifted = np.zeros((H, W), bool)
                ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
                xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
                shifted[yd, xd] = s[ys, xs]                      # shifted[y, x] = s[y + dy, x + dx] where that lies inside the image
                near |= shifted
    return near & ~s


# ------------------------------------------------------------------------------------------------ step 4

def corner(box, k, T=np.float32):
    b = np.asarray(box, np.float32).reshape(6)
    return tuple(T(b[3 + a] if k & (1 << a) else b[a]) for a in range(3))


def edges(boxes, block, W, H, dtype=np.float32):
    """[n, 6] world boxes -> [n, 12, 8] records x0 y0 z0 x1 y1 z1 valid pad; an invalid edge is all zeros."""
    T = np.dtype(dtype).type
    m = np.frombuffer(block, np.float32, 16, 128).astype(T)      # view_proj, column-major as stored
    boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
    out = np.zeros((len(boxes), 12, 8), T)
    zero, half = T(0.0), T(0.5)
    with np.errstate(all="ignore"):
        for b, box in enumerate(boxes):
            for j, (k0, k1) in enumerate(EDGE_CORNERS):
                c = []
                for k in (k0, k1):
                    X, Y, Z = corner(box, k, T)
                    c.append([((m[r] * X + m[4 + r] * Y) + m[8 + r] * Z) + m[12 + r] for r in range(4)])
                behind = [not (c[e][2] >= zero) for e in (0, 1)]
                if behind[0] and behind[1]:
                    continue
                if behind[0] or behind[1]:
                    o = 0 if behind[0] else 1
                    q = 1 - o
                    t = (zero - c[o][2]) / (c[q][2] - c[o][2])
                    for i in (0, 1, 3):
                        c[o][i] = c[o][i] + t * (c[q][i] - c[o][i])
                    c[o][2] = zero
                if not (c[0][3] > zero) or not (c[1][3] > zero):
                    continue
                rec = []
                for e in (0, 1):
                    rec += [((c[e][0] / c[e][3]) * half + half) * T(W), (half - (c[e][1] / c[e][3]) * half) * T(H), c[e][2] / c[e][3]]
                if not np.isfinite(np.array(rec, T)).all():
                    continue
                out[b, j, :6] = rec
                out[b, j, 6] = T(1.0)
    return out


# ------------------------------------------------------------------------------------------------ steps 5 and 6

def edge_alpha(e, d, W, H, rec, dtype=np.float32, parts=False):
    """One edge record over the whole frame -> a_e [H, W] (with parts: also coverage and visible)."""
    T = np.dtype(dtype).type
    sx0, sy0, sz0, sx1, sy1, sz1 = (T(v) for v in e[:6])
    zero, one = T(0.0), T(1.0)
    m = T(np.float32(rec["box_half_width"])) + T(0.5)
    cy, cx = np.meshgrid(np.arange(H).astype(T) + T(0.5), np.arange(W).astype(T) + T(0.5), indexing="ij")
    with np.errstate(all="ignore"):
        gate = (np.fmin(sx0, sx1) - m <= cx) & (cx <= np.fmax(sx0, sx1) + m) & (np.fmin(sy0, sy1) - m <= cy) & (cy <= np.fmax(sy0, sy1) + m)
        ex, ey = sx1 - sx0, sy1 - sy0
        l2 = ex * ex + ey * ey
        rx, ry = cx - sx0, cy - sy0
        t = (rx * ex + ry * ey) / l2 if l2 > zero else np.zeros((H, W), T)
        t = np.fmin(np.fmax(t, zero), one)
        qx, qy = rx - t * ex, ry - t * ey
        dist = np.sqrt(qx * qx + qy * qy)
        cov = np.fmin(np.fmax(m - dist, zero), one)
        cov = np.where(gate, cov, zero)
        z = sz0 + t * (sz1 - sz0)
        visible = (z - T(np.float32(rec["depth_epsilon"]))) <= np.asarray(d, np.float32).astype(T)
        a = np.where(visible, cov, cov * T(np.float32(rec["hidden_alpha"])))
    assert a.dtype == T
    return (a, cov, visible) if parts else a


def box_alpha(edge_table, d, W, H, rec, dtype=np.float32):
    """A(p): the greatest a_e over the valid edges (0 with BOXES off) -> (A, on_visible: the greatest comes from an edge visible there)."""
    T = np.dtype(dtype).type
    A = np.zeros((H, W), T)
    vis_best = np.zeros((H, W), bool)
    if rec["flags"] & BOXES:
        for e in np.asarray(edge_table).reshape(-1, 8):
            if e[6] == 0:
                continue
            a, cov, visible = edge_alpha(e, d, W, H, rec, dtype, parts=True)
            better = a > A
            vis_best = np.where(better, visible, vis_best)
            A = np.fmax(A, a)
    return A, vis_best


# ------------------------------------------------------------------------------------------------ step 7

def _over(C, color, a):
    out = np.empty_like(C)
    for ch in range(3):
        out[..., ch] = (C[..., ch] * (np.float32(1.0) - a)) + (np.float32(color[ch]) * a)
    out[..., 3] = (C[..., 3] * (np.float32(1.0) - a)) + a
    return out


def blend(bits, ring_mask, A, rec):
    """RGBA16F bits [H, W, 4] -> the same with the ring and then the boxes blended in f32 and rounded to f16 once; other pixels keep their bits."""
    bits = np.asarray(bits, np.uint16)
    A = np.asarray(A, np.float32)
    with np.errstate(all="ignore"):
        C = bits.view(np.float16).astype(np.float32)
        oc, bc = [np.float32(v) for v in rec["outline_color"]], [np.float32(v) for v in rec["box_color"]]
        C = np.where(ring_mask[..., None], _over(C, oc, np.full(A.shape, oc[3], np.float32)), C)
        C = np.where((A > 0)[..., None], _over(C, bc, bc[3] * A), C)
        out = C.astype(np.float16).view(np.uint16)
    touched = ring_mask | (A > 0)
    return np.where(touched[..., None], out, bits)


def blend_f32(img, bits_on, touched):
    """The composite's f32 tap: the stored halves widened where the overlay touched the pixel, the tap as it was elsewhere."""
    return np.where(touched[..., None], np.asarray(bits_on, np.uint16).view(np.float16).astype(np.float32), np.asarray(img, np.float32))


# ------------------------------------------------------------------------------------------------ all of it

def overlay(vis, table, keys, boxes, block, W, H, rec=None, dtype=np.float32):
    """-> dict: draw_selected, selected, depth, ring, edges, box_alpha, box_visible (the greatest edge alpha of the pixel is a visible edge's)."""
    rec = rec or record()
    sel = selected_draws(table, keys)
    s, d = pixels(vis, table, sel)
    assert s.shape == (H, W)
    et = edges(boxes, block, W, H, dtype)
    A, vb = box_alpha(et, d, W, H, rec, dtype)
    return {"draw_selected": sel, "selected": s, "depth": d, "ring": ring(s, int(rec["outline_radius"]), bool(rec["flags"] & OUTLINE)), "edges": et,
            "box_alpha": A, "box_visible": vb}


def counts(out):
    """What a GPU test's floor is made of: ring pixels, box pixels with 0 < A < 1, with A = 1, and box pixels whose strongest edge is visible / hidden."""
    A = out["box_alpha"]
    return {"ring": int(out["ring"].sum()), "partial": int(((A > 0) & (A < 1)).sum()), "full": int((A == 1).sum()),
            "visible": int(((A > 0) & out["box_visible"]).sum()), "hidden": int(((A > 0) & ~out["box_visible"]).sum())}


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests and their floors

PARAMS = ((1, 0.5), (4, 1.75))                      # (outline_radius, box_half_width)
SELECTED_MESHES = {"corner": (1,), "boxes": (3, 5)}  # indices into the model's meshes in insertion order: corner's second quad; the first and third box of boxes


def selection_of(model, scene):
    """The selection a case uses -> (key words [(high, low)], boxes [[min xyz, max xyz]]) from the model's mesh records."""
    from oracle.host_mirror import key_as_ffi
    items = list(model.meshes.items())
    picked = [items[i] for i in SELECTED_MESHES[scene]]
    return key_words([key_as_ffi(mk) for mk, _ in picked]), [list(rec.world_aabb.min) + list(rec.world_aabb.max) for _, rec in picked]


def tile_list_sizes(edge_table, W, H, rec):
    """Per 16x16 tile, how many valid edges the overlay kernel's cull keeps: step 5's rectangle against the tile's pixel-centre range."""
    m = np.float32(np.float32(rec["box_half_width"]) + np.float32(0.5))
    e = np.asarray(edge_table, np.float32).reshape(-1, 8)
    e = e[e[:, 6] != 0]
    out = np.zeros(((H + 15) // 16, (W + 15) // 16), np.int64)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            x_lo, x_hi = np.float32(16 * tx + 0.5), np.float32(min(16 * tx + 15, W - 1) + 0.5)
            y_lo, y_hi = np.float32(16 * ty + 0.5), np.float32(min(16 * ty + 15, H - 1) + 0.5)
            keep = ((np.fmin(e[:, 0], e[:, 3]) - m <= x_hi) & (x_lo <= np.fmax(e[:, 0], e[:, 3]) + m)
                    & (np.fmin(e[:, 1], e[:, 4]) - m <= y_hi) & (y_lo <= np.fmax(e[:, 1], e[:, 4]) + m))
            out[ty, tx] = int(keep.sum())
    return out


KINDS = ("ring", "partial", "full", "visible", "hidden")
# (scene, camera, W, H, outline_radius, box_half_width) -> the least count of each of KINDS a GPU test accepts: half of what the restatement counts
# on the CPU oracle's keys (tests/test_selection_cpu.py recomputes them), so that no GPU test passes on an empty overlay.  0: the case does not show that
# kind — `full` needs a pixel centre ON a line at half width 0.5; under `closeup` the camera stands inside the first box and the third is culled, so
# nothing selected is seen and only the near-clipped box is drawn; under `far` at 8 x 5 the boxes are smaller than a pixel.
FLOORS = {
    ("corner", "perspective", 8, 5, 1, 0.5): (3, 6, 0, 0, 6),
    ("corner", "perspective", 8, 5, 4, 1.75): (12, 13, 0, 0, 13),
    ("corner", "perspective", 33, 17, 1, 0.5): (11, 26, 0, 1, 25),
    ("corner", "perspective", 33, 17, 4, 1.75): (45, 58, 1, 1, 58),
    ("corner", "perspective", 70, 45, 1, 0.5): (28, 61, 0, 1, 60),
    ("corner", "perspective", 70, 45, 4, 1.75): (120, 144, 1, 1, 144),
    ("corner", "ortho", 8, 5, 1, 0.5): (3, 8, 0, 2, 6),
    ("corner", "ortho", 8, 5, 4, 1.75): (11, 12, 2, 5, 9),
    ("corner", "ortho", 33, 17, 1, 0.5): (18, 40, 0, 17, 23),
    ("corner", "ortho", 33, 17, 4, 1.75): (58, 64, 17, 34, 47),
    ("corner", "ortho", 70, 45, 1, 0.5): (27, 61, 0, 1, 60),
    ("corner", "ortho", 70, 45, 4, 1.75): (114, 142, 1, 1, 142),
    ("corner", "closeup", 8, 5, 1, 0.5): (3, 7, 0, 0, 7),
    ("corner", "closeup", 8, 5, 4, 1.75): (11, 13, 0, 0, 13),
    ("corner", "closeup", 33, 17, 1, 0.5): (11, 18, 3, 4, 17),
    ("corner", "closeup", 33, 17, 4, 1.75): (46, 54, 4, 4, 54),
    ("corner", "closeup", 70, 45, 1, 0.5): (29, 62, 0, 0, 62),
    ("corner", "closeup", 70, 45, 4, 1.75): (121, 135, 0, 0, 135),
    ("corner", "far", 8, 5, 1, 0.5): (2, 5, 0, 4, 1),
    ("corner", "far", 8, 5, 4, 1.75): (17, 7, 4, 12, 0),
    ("corner", "far", 33, 17, 1, 0.5): (7, 14, 0, 11, 3),
    ("corner", "far", 33, 17, 4, 1.75): (45, 19, 13, 23, 8),
    ("corner", "far", 70, 45, 1, 0.5): (20, 40, 0, 23, 17),
    ("corner", "far", 70, 45, 4, 1.75): (96, 57, 29, 54, 32),
    ("corner", "along", 8, 5, 1, 0.5): (3, 6, 0, 0, 6),
    ("corner", "along", 8, 5, 4, 1.75): (11, 12, 0, 0, 12),
    ("corner", "along", 33, 17, 1, 0.5): (10, 24, 0, 0, 24),
    ("corner", "along", 33, 17, 4, 1.75): (43, 55, 0, 0, 55),
    ("corner", "along", 70, 45, 1, 0.5): (28, 62, 0, 0, 62),
    ("corner", "along", 70, 45, 4, 1.75): (116, 135, 0, 0, 135),
    ("boxes", "perspective", 8, 5, 1, 0.5): (4, 7, 0, 5, 2),
    ("boxes", "perspective", 8, 5, 4, 1.75): (18, 8, 7, 10, 5),
    ("boxes", "perspective", 33, 17, 1, 0.5): (14, 38, 0, 27, 11),
    ("boxes", "perspective", 33, 17, 4, 1.75): (69, 30, 30, 49, 12),
    ("boxes", "perspective", 70, 45, 1, 0.5): (39, 139, 0, 71, 68),
    ("boxes", "perspective", 70, 45, 4, 1.75): (170, 141, 88, 147, 82),
    ("boxes", "ortho", 8, 5, 1, 0.5): (4, 6, 0, 4, 2),
    ("boxes", "ortho", 8, 5, 4, 1.75): (18, 10, 4, 6, 8),
    ("boxes", "ortho", 33, 17, 1, 0.5): (11, 25, 0, 19, 5),
    ("boxes", "ortho", 33, 17, 4, 1.75): (60, 23, 25, 36, 12),
    ("boxes", "ortho", 70, 45, 1, 0.5): (30, 102, 0, 53, 49),
    ("boxes", "ortho", 70, 45, 4, 1.75): (136, 97, 66, 110, 53),
    ("boxes", "closeup", 8, 5, 1, 0.5): (0, 5, 0, 5, 0),
    ("boxes", "closeup", 8, 5, 4, 1.75): (0, 5, 6, 12, 0),
    ("boxes", "closeup", 33, 17, 1, 0.5): (0, 17, 0, 17, 0),
    ("boxes", "closeup", 33, 17, 4, 1.75): (0, 17, 23, 40, 0),
    ("boxes", "closeup", 70, 45, 1, 0.5): (0, 47, 0, 46, 1),
    ("boxes", "closeup", 70, 45, 4, 1.75): (0, 47, 58, 105, 1),
    ("boxes", "far", 8, 5, 1, 0.5): (0, 2, 0, 1, 1),
    ("boxes", "far", 8, 5, 4, 1.75): (0, 7, 2, 7, 1),
    ("boxes", "far", 33, 17, 1, 0.5): (2, 4, 0, 2, 2),
    ("boxes", "far", 33, 17, 4, 1.75): (24, 10, 2, 3, 9),
    ("boxes", "far", 70, 45, 1, 0.5): (5, 11, 0, 8, 3),
    ("boxes", "far", 70, 45, 4, 1.75): (39, 15, 9, 13, 11),
    ("boxes", "along", 8, 5, 1, 0.5): (3, 11, 0, 7, 3),
    ("boxes", "along", 8, 5, 4, 1.75): (12, 6, 8, 10, 4),
    ("boxes", "along", 33, 17, 1, 0.5): (15, 84, 0, 53, 30),
    ("boxes", "along", 33, 17, 4, 1.75): (60, 67, 60, 89, 38),
    ("boxes", "along", 70, 45, 1, 0.5): (25, 238, 0, 116, 122),
    ("boxes", "along", 70, 45, 4, 1.75): (105, 280, 149, 248, 181),
}
