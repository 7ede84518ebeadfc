"""The vertex stage restated in numpy float64, from the scene description alone (TEST INFRASTRUCTURE ONLY).

`k_deform_transform` and `oracle_geometry.c` were written from the same reading of apply_vertex.wgsl, skin.wgsl and morph.wgsl with the same operation
order, so "bit-equal to the oracle" cannot notice a mistake they share.  This module is the third party: no mirrors, no packed records, no f32 — the rules
of DESIGN §3 "Vertex stage" applied to the SceneDesc's own arrays:

  * world(node) = world(parent) . T . R . S, composed here from the node tree;  joint matrix = world(joint) . inverse_bind
  * morph deltas first (position, normal, tangent xyz), weighted by the EFFECTIVE morph weights (below)
  * then the skin: the plain weighted sum of the joint matrices over every set, applied to the position; its raw upper 3x3 — no inverse-transpose —
    to normal and tangent
  * then the mesh node's model matrix (times the instance matrix): world position, clip = (proj . view) . world
  * normal through cof(M) / det when |det| > 1e-8, else through M; normalised
  * tangent through M, Gram-Schmidt against the normal; when the squared remainder is <= 1e-8 the tangent is normalize(axis x n), axis = z, or y when
    |n.z| > 0.999;  the handedness is the input's w, untouched.

What it takes from the model next to its SceneDesc: the ORDER of the draw lists (which mesh is drawn when: renderable.rs sorts by pipeline and depth) and
one mirror read, `effective_morph_weights`.  Inputs are the f32 values the scene holds (a TRS component, a vertex, a weight), widened; nothing is rounded
after that.

It also reports, per vertex, which side of the two thresholds it took and by what factor, so that tests can require their inputs to sit well away from
them (tests/vertex_stage_cases.py) and compare the branch itself.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from oracle import host_mirror as hm
from oracle import scene_model as sm

DET_THRESHOLD = 1e-8          # apply_vertex.wgsl:92
TLEN_SQ_THRESHOLD = 1e-8      # apply_vertex.wgsl:100
FALLBACK_Y_ABOVE = 0.999      # apply_vertex.wgsl:107

# The two tolerances of every comparison against this restatement: 4 x the worst distance between the C oracle (f32, the only rounded party on the CPU
# side; the cases chain between a dozen and roughly a hundred roundings) and this module over all of tests/vertex_stage_cases.py.
# tests/test_vertex_stage_cpu.py::test_the_committed_tolerances_are_four_times_the_worst_distance prints the worst values it sees; DESIGN §3 records them too.
POSITION_REL_TOL = 4 * 5.66e-7     # clip and world position, per vertex, relative to the vertex's largest |component|; measured worst 5.654e-07
                                   # (blend_twins, world position of the skinned and morphed tube; worst clip 2.7e-07, three_sets)
DIRECTION_ABS_TOL = 4 * 2.13e-7    # unit normal and unit tangent, absolute per component; measured worst 2.120e-07 (morph_then_skin's mesh, a tangent; worst normal 2.0e-07, scaled_joints)


def _f64(v):
    """an input as the scene stores it (f32), widened"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def trs_matrix(translation, rotation, scale) -> np.ndarray:
    """T . R . S as an ordinary (row, column) 4x4; rotation = quaternion xyzw, taken as given (not renormalised: glam does not either)."""
    t, (x, y, z, w), s = _f64(translation), _f64(rotation), _f64(scale)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    m = np.eye(4)
    m[:3, :3] = r * s[None, :]
    m[:3, 3] = t
    return m


def node_world(scene, i: int) -> np.ndarray:
    n = scene.nodes[i]
    local = trs_matrix(n.translation, n.rotation, n.scale)
    return local if n.parent is None else node_world(scene, n.parent) @ local


def effective_morph_weights(model, morph_key, n: int) -> np.ndarray:
    """The one mirror read.  morph.wgsl:17-19 reads weight i at float [off/4 + 1 + i] ("[target_count, weight0, ...]"), while Morphs::insert_raw
    (meshes/morphs.rs:148-170) writes a mesh's static glTF `weights` at floats [0, n) of the block; only the animation path (morphs.rs:197-217)
    writes [1, n + 1).  So what the shader blends with is the n floats BEHIND the first one, wherever they came from."""
    off = model.morph_weights.offset(morph_key)
    raw = np.frombuffer(bytes(model.morph_weights.raw), dtype=np.float32)
    return raw[off // 4 + 1: off // 4 + 1 + n].astype(np.float64)


def naive_morph_weights(model, morph_key, n: int) -> np.ndarray:
    """what a reader of the glTF alone would expect: the floats at [off/4, off/4 + n).  For the test that pins the offset rule; never used by restate()."""
    off = model.morph_weights.offset(morph_key)
    raw = np.frombuffer(bytes(model.morph_weights.raw), dtype=np.float32)
    return raw[off // 4: off // 4 + n].astype(np.float64)


def primitive_of(model, mesh_key):
    """(node index, PrimitiveDesc) of a draw's mesh: the node whose transform the mesh hangs on, the primitive by its place among that node's meshes."""
    rec = model.meshes.get(mesh_key)
    node = model.node_keys.index(rec.transform_key)
    return node, model.scene.nodes[node].primitives[model.transform_to_meshes[rec.transform_key].index(mesh_key)]


def _normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def restate_draw(model, draw: dict, weights_fn=effective_morph_weights) -> Dict[str, np.ndarray]:
    """One draw, instance after instance, vertices in exploded index order (`indices.reshape(-1)`: the order of both the 56-byte records of the
    geometry pass and the indexed walk of the transparent pass)."""
    scene = model.scene
    node, p = primitive_of(model, draw["mesh_key"])
    rec = model.meshes.get(draw["mesh_key"])
    for sk in scene.skins:
        assert node not in sk.joints, "a mesh on a joint node gets a transform of its own (populate/mesh.rs:36-52): not restated here"
    V = np.asarray(p.positions).shape[0]
    pos, nrm = _f64(p.positions), _f64(p.normals)
    tan = _f64(p.tangents) if p.tangents is not None else np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (V, 1))
    txyz, hand = tan[:, :3].copy(), tan[:, 3].copy()

    if p.morph_targets:
        w = weights_fn(model, rec.morph_key, len(p.morph_targets))
        for wi, tg in zip(w, p.morph_targets):
            if tg.get("positions") is not None:
                pos = pos + wi * _f64(tg["positions"])
            if tg.get("normals") is not None:
                nrm = nrm + wi * _f64(tg["normals"])
            if tg.get("tangents") is not None:
                txyz = txyz + wi * _f64(tg["tangents"])

    skin_det = np.ones(V)
    if scene.nodes[node].skin is not None and p.joints:
        sk = scene.skins[scene.nodes[node].skin]
        jm = np.stack([node_world(scene, j) @ _f64(sk.inverse_bind[k]).T for k, j in enumerate(sk.joints)])      # inverse_bind is [col][row]
        blend = np.zeros((V, 4, 4))
        for j, w in zip(p.joints, p.weights):
            j = np.asarray(j, dtype=np.int64)
            assert j.min() >= 0 and j.max() < len(sk.joints), "joint index outside the skin"
            blend += (_f64(w)[:, :, None, None] * jm[j]).sum(axis=1)
        pos = np.einsum("vij,vj->vi", blend[:, :3, :3], pos) + blend[:, :3, 3]
        nrm = np.einsum("vij,vj->vi", blend[:, :3, :3], nrm)
        txyz = np.einsum("vij,vj->vi", blend[:, :3, :3], txyz)
        skin_det = np.linalg.det(blend[:, :3, :3])

    flat = np.asarray(p.indices, dtype=np.int64).reshape(-1)
    pos, nrm, txyz, hand, skin_det = pos[flat], nrm[flat], txyz[flat], hand[flat], skin_det[flat]
    view_proj = _f64(scene.proj).T @ _f64(scene.view).T                                                      # scene matrices are [col][row]
    world = node_world(scene, node)
    models = [world] if p.instances is None else [world @ trs_matrix(t, r, s) for (t, r, s) in p.instances]

    out: Dict[str, List[np.ndarray]] = {}

    def put(key, v):
        out.setdefault(key, []).append(v)

    for m in models:
        n_v = pos.shape[0]
        m3 = m[:3, :3]
        wpos = pos @ m3.T + m[:3, 3]
        clip = np.concatenate([wpos, np.ones((n_v, 1))], axis=1) @ view_proj.T
        r0, r1, r2 = m3
        cof = np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)])
        det = float(r0 @ cof[0])
        cofactor = abs(det) > DET_THRESHOLD
        n_un = (nrm @ cof.T) / det if cofactor else nrm @ m3.T
        n_len = np.linalg.norm(n_un, axis=1)
        n_w = n_un / n_len[:, None]
        t_raw = txyz @ m3.T
        t_ortho = t_raw - n_w * (t_raw * n_w).sum(axis=1, keepdims=True)
        tlen_sq = (t_ortho * t_ortho).sum(axis=1)
        gs = tlen_sq > TLEN_SQ_THRESHOLD
        use_y = np.abs(n_w[:, 2]) > FALLBACK_Y_ABOVE
        axis = np.where(use_y[:, None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
        fb = np.cross(axis, n_w)
        fb_len = np.linalg.norm(fb, axis=1)
        fb = fb / fb_len[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            t_w = np.where(gs[:, None], t_ortho / np.sqrt(tlen_sq)[:, None], fb)
            tan_factor = np.where(gs, tlen_sq / TLEN_SQ_THRESHOLD, TLEN_SQ_THRESHOLD / tlen_sq)
            ratio = np.sqrt(tlen_sq) / np.linalg.norm(t_raw, axis=1)
        put("clip", clip); put("wpos", wpos); put("normal", n_w); put("tangent", np.concatenate([t_w, hand[:, None]], axis=1))
        put("det", np.full(n_v, det)); put("det_cofactor", np.full(n_v, cofactor))
        put("det_factor", np.full(n_v, abs(det) / DET_THRESHOLD if cofactor else (DET_THRESHOLD / abs(det) if det != 0.0 else np.inf)))
        put("tlen_sq", tlen_sq); put("tan_gram_schmidt", gs); put("tan_factor", tan_factor)
        put("fallback_axis", np.where(gs, 0, np.where(use_y, 2, 1)))          # 0 = not taken, 1 = z, 2 = y
        put("fallback_tangent", fb)                                           # what the fallback WOULD give (the cases keep Gram-Schmidt results away from it)
        put("ortho_ratio", ratio)                                             # |t_ortho| / |t_raw|
        put("normal_len", n_len); put("skin_det", skin_det)
    return {k: np.concatenate(v) for k, v in out.items()}


def restate(model, transparent: bool = False, weights_fn=effective_morph_weights, draws=None):
    """(per-draw results, all draws concatenated) for the opaque list (the order of OracleFrame.transform) or, transparent=True, the transparent list
    (the order of OracleFrame.forward).  collect_draws() fills both lists."""
    opaque = model.collect_draws()
    if draws is None:
        draws = model.collect_transparent_draws() if transparent else opaque
    per_draw = [restate_draw(model, d, weights_fn) for d in draws]
    if not per_draw:
        return per_draw, {}
    return per_draw, {k: np.concatenate([r[k] for r in per_draw]) for k in per_draw[0]}


def distances(ref: Dict[str, np.ndarray], clip, nt, wpos=None) -> Dict[str, float]:
    """Worst distances of an f32 vertex stage (oracle or device: clip (N,4), nt (N,8) = normal xyz0 + tangent xyzw, optional world position) from the
    restatement: positions per vertex relative to that vertex's largest |component| of the restatement, directions absolute; handedness mismatches
    counted.  Every vertex takes part."""
    clip, nt = np.asarray(clip, dtype=np.float64), np.asarray(nt, dtype=np.float64)
    n = ref["clip"].shape[0]
    assert clip.shape[0] == n and nt.shape[0] == n, (clip.shape, nt.shape, n)
    assert np.isfinite(clip).all() and np.isfinite(nt).all()
    out = {"clip_rel": float((np.abs(clip - ref["clip"]).max(axis=1) / np.abs(ref["clip"]).max(axis=1)).max()),
           "normal_abs": float(np.abs(nt[:, 0:3] - ref["normal"]).max()),
           "tangent_abs": float(np.abs(nt[:, 4:7] - ref["tangent"][:, :3]).max()),
           "handedness_mismatch": int((nt[:, 7] != ref["tangent"][:, 3]).sum()),
           "normal_w_nonzero": int((nt[:, 3] != 0.0).sum())}
    if wpos is not None:
        wpos = np.asarray(wpos, dtype=np.float64)
        assert np.isfinite(wpos).all()
        out["wpos_rel"] = float((np.abs(wpos[:, :3] - ref["wpos"]).max(axis=1) / np.abs(ref["wpos"]).max(axis=1)).max())
        out["wpos_w_not_one"] = int((wpos[:, 3] != 1.0).sum())
    return out


def assert_within_tolerances(name: str, d: Dict[str, float]):
    assert d["clip_rel"] <= POSITION_REL_TOL and d.get("wpos_rel", 0.0) <= POSITION_REL_TOL, (name, d)
    assert d["normal_abs"] <= DIRECTION_ABS_TOL and d["tangent_abs"] <= DIRECTION_ABS_TOL, (name, d)
    assert d["handedness_mismatch"] == 0 and d["normal_w_nonzero"] == 0 and d.get("wpos_w_not_one", 0) == 0, (name, d)


# ------------------------------------------------------------------------------------------------ the f32 side's branches
# What an f32 vertex stage DID at the two thresholds, for the exact comparison of the branch taken.  These read mirrors and outputs of the side under
# test; restate() never calls them.

def f32_det_branch(model, draws) -> np.ndarray:
    """Per vertex of the draw list: did |det_model| > 1e-8 hold in f32?  The determinant as apply_vertex forms it (rows, cross, dot: left to right,
    every operation rounded once) from the transforms and instances mirrors."""
    mir = model.mirrors()
    tr = np.frombuffer(mir[sm.BUF_TRANSFORMS], dtype=np.float32)
    gm = np.frombuffer(mir[sm.BUF_GEOM_META], dtype=np.uint32)
    inst = np.frombuffer(mir[sm.BUF_INSTANCES], dtype=np.float32)
    out = []
    for d in draws:
        toff = int(gm[d["geom_meta_off"] // 4 + 8]) // 64 * 16
        base = tr[toff:toff + 16].reshape(4, 4)
        for k in range(max(1, d.get("inst_count", 0))):
            m = base
            if d.get("inst_count", 0):
                o = d["inst_off"] // 4 + 16 * k
                m = hm.mat4_mul(base, inst[o:o + 16].reshape(4, 4))
            c0, c1, c2 = m[0][:3], m[1][:3], m[2][:3]
            r0, r1, r2 = (np.array([c0[i], c1[i], c2[i]], dtype=np.float32) for i in range(3))
            cof0 = np.array([r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]], dtype=np.float32)
            det = (r0[0] * cof0[0] + r0[1] * cof0[1]) + r0[2] * cof0[2]
            out.append(np.full(3 * d["tri_count"], bool(np.abs(det) > np.float32(DET_THRESHOLD))))
    return np.concatenate(out)


def f32_fallback_axis(nt) -> np.ndarray:
    """Per vertex of an f32 result (nt: normal xyz0, tangent xyzw): 0 = the tangent is not the fallback's, 1 = it is normalize(z x n), 2 = it is
    normalize(y x n) — recognised by value (the cases keep Gram-Schmidt tangents at least 1e-3 away from the fallback's)."""
    nt = np.asarray(nt, dtype=np.float64)
    n, t = nt[:, 0:3], nt[:, 4:7]
    use_y = np.abs(n[:, 2]) > float(np.float32(FALLBACK_Y_ABOVE))          # the comparison as f32 makes it
    axis = np.where(use_y[:, None], np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    fb = _normalize(np.cross(axis, n))
    is_fb = np.abs(t - fb).max(axis=1) < 1e-5
    return np.where(is_fb, np.where(use_y, 2, 1), 0)
