"""Small scenes for the vertex stage, each built to reach named code of `k_deform_transform` / `oracle_geometry.c: apply_vertex`
(TEST INFRASTRUCTURE ONLY).  160x100 frames, meshes of a few hundred vertices, fixed seeds; every mesh has tangents and a normal-mapped material, so
tangent bits reach the image.

  two_sets, three_sets     the `set > 0` accumulation: later sets name arbitrary valid joints, weights sum to 1 over all sets, the last set has three
                           zero-weight slots with joint 0 (how real glTF pads)
  scaled_joints            joints rotated about different axes and scaled non-uniformly: the blended matrix is not rigid, so "raw upper 3x3, no
                           inverse-transpose" differs from every other rule
  weights_not_normalised   weights sum to 0.7
  tangent_morphs           > 512 vertices (three 256-vertex workgroups and more), 3 targets with position, normal AND tangent deltas, weights through the
                           animation path, one negative
  morph_then_skin          both on one mesh
  static_morph_weights     two morphed meshes, weights given as glTF `mesh.weights` only: they reach the shader shifted by one
  mirrored                 node scale (-1, 1, 1), an instance with a negative scale; one back-face-culled and one double-sided material
  tiny_model, just_above   uniform and non-uniform scales either side of |det| > 1e-8
  instanced_morphed        a morphed cube drawn 3 times, one instance mirrored, one tiny
  tangent_parallel         tangents exactly along the normal, under normals with |n.z| > 0.999 (both signs) and oblique ones: both fallback axes
  block_edges              draws of 1, 85, 86, 171 and 256 triangles = 3, 255, 258, 513, 768 vertices: last workgroups of 3, 255 and 2 vertices, the
                           odd counts 255 and 1 (8-byte tail of the LDS staging), exact multiples of 256; two of the draws skinned
  blend_twins              morph_then_skin and mirrored with blend materials: the indexed variant of the kernel (transparent pass)

`check_inputs` asserts, on the float64 restatement, the conditions that make a comparison meaningful: thresholds at least a factor 4 away, no
Gram-Schmidt step that amplifies rounding, no zero normal, everything finite, joint indices inside their skin, something on screen.

On tiny_model / just_above: a uniform scale of 0.002 (det 8e-9, an asset authored in millimetres) sits a factor 1.25 under the switch, which the factor-4
condition excludes; the cases use the nearest scales that satisfy it (det about 2e-9 and 4.3e-8).
"""
from __future__ import annotations

import math

import numpy as np

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc, PrimitiveDesc, SceneDesc, SkinDesc, TextureRef

from tests import vertex_stage_reference as vsr

F = np.float32
WIDTH, HEIGHT = 160, 100
MARGIN = 4.0                 # thresholds: every |det| and squared tangent remainder at least this factor away, on its intended side
MIN_ORTHO_RATIO = 0.1        # outside tangent_parallel: |t_ortho| >= 0.1 |t_raw|
NZ_MARGIN = 1e-4             # |n.z| this far from the 0.999 switch of the fallback axis (where the fallback is taken)


# ------------------------------------------------------------------------------------------------ building blocks

def _textures(rng):
    return [scenes.value_noise_rgba8(rng, 16, 4, base=(0.6, 0.5, 0.4), amp=(0.3, 0.3, 0.3)), scenes.value_noise_rgba8(rng, 16, 4, kind="normal")]


def _mat(**kw):
    kw.setdefault("metallic_factor", 0.1)
    kw.setdefault("roughness_factor", 0.6)
    return MaterialDesc(base_color_tex=TextureRef(0), normal_tex=TextureRef(1), **kw)


def _blend(**kw):
    return _mat(alpha_mode="blend", base_color_factor=(0.9, 0.8, 0.7, 0.6), **kw)


def _scene(nodes, mats, rng, eye, target=(0.0, 0.0, 0.0), skins=(), near=0.1, far=100.0):
    return SceneDesc(nodes=nodes, materials=mats, textures=_textures(rng), samplers=[dict(scenes.REPEAT_LINEAR)], skins=list(skins),
                     lights=list(scenes.DEFAULT_LIGHTS[:2]), width=WIDTH, height=HEIGHT, view=scenes.look_at_rh(eye, target),
                     proj=scenes.perspective_rh(math.radians(45), WIDTH / HEIGHT, near, far), camera_position=eye)


LENGTH = 2.4


def _tube(around, along, radius=0.35):
    def fn(U, V):
        th = U * 2 * math.pi
        r = radius + 0.05 * np.sin(V * 9.0)
        return np.stack([r * np.cos(th), V * LENGTH - LENGTH / 2, -r * np.sin(th)], axis=-1)
    return scenes.grid_patch(fn, around, along, uv_scale=(2.0, 4.0))


def _ball(nu=12, nv=9, radius=0.5, k=(2.0, 3.0, 4.0)):
    k = np.asarray(k)

    def fn(U, V):
        th, phi = U * 2 * math.pi, (0.05 + 0.9 * V) * math.pi
        d = np.stack([np.sin(phi) * np.cos(th), np.cos(phi), -np.sin(phi) * np.sin(th)], axis=-1)
        return d * (radius * (1.0 + 0.1 * np.sin(d @ k * 3.0)))[..., None]
    return scenes.grid_patch(fn, nu, nv, uv_scale=(2.0, 1.0))


def _prim(patch, material, **kw):
    pos, nrm, tan, uvs, idx = patch
    return PrimitiveDesc(positions=pos, normals=nrm, tangents=tan, uvs=[uvs], indices=idx, material=material, **kw)


def _rig(nodes, rng, n_joints=6, scaled=False, parent=0):
    """A chain of joints along y under `parent`, posed: each rotated about an axis of its own (and, scaled=True, scaled non-uniformly).  The inverse
    bind matrices undo the REST pose (translations only), so the skin moves the mesh.  Returns (SkinDesc, the joints' rest heights)."""
    jy = np.linspace(-LENGTH / 2, LENGTH / 2, n_joints)
    joint_nodes = []
    for j in range(n_joints):
        trans = (0.0, float(jy[0]), 0.0) if j == 0 else (0.0, float(jy[1] - jy[0]), 0.0)
        axis = rng.normal(size=3)
        ang = float(rng.uniform(0.08, 0.25)) * (1 if j % 2 else -1)
        scale = tuple(float(v) for v in rng.uniform(0.85, 1.15, size=3)) if scaled else (1.0, 1.0, 1.0)
        nodes.append(NodeDesc(translation=trans, rotation=scenes.quat_axis_angle(axis, ang), scale=scale, parent=parent if j == 0 else joint_nodes[-1]))
        joint_nodes.append(len(nodes) - 1)
    inv_bind = np.zeros((n_joints, 4, 4), dtype=F)
    for j in range(n_joints):
        m = np.eye(4, dtype=F)
        m[3][1] = -jy[j]
        inv_bind[j] = m
    return SkinDesc(joints=joint_nodes, inverse_bind=inv_bind), jy


def _skin_sets(rng, pos, jy, sets, total=1.0):
    """Set 0: the four nearest joints.  Later sets: arbitrary valid joints.  Weights positive, `total` over all sets; the last of several sets ends in
    three zero-weight slots naming joint 0."""
    V, J = pos.shape[0], len(jy)
    joints = [np.argsort(np.abs(pos[:, 1:2] - jy[None, :]), axis=1)[:, :4].astype(np.uint32)]
    for _ in range(1, sets):
        joints.append(rng.integers(0, J, size=(V, 4)).astype(np.uint32))
    w = rng.dirichlet(np.ones(4 * sets), size=V).reshape(V, sets, 4)
    if sets > 1:
        joints[-1][:, 1:] = 0
        w[:, -1, 1:] = 0.0
    w = w / w.sum(axis=(1, 2), keepdims=True) * total
    return joints, [w[:, s].astype(F) for s in range(sets)]


def _morph_targets(rng, pos, nrm, tan, n=3, amp=0.12):
    """position, normal and tangent deltas: smooth waves plus noise, small enough to leave normals and tangents well conditioned"""
    out = []
    for i in range(n):
        k = rng.uniform(2.0, 6.0, size=3)
        wave = np.sin(pos @ k + i)[:, None]
        out.append({"positions": (amp * wave * nrm + 0.02 * rng.normal(size=pos.shape)).astype(F),
                    "normals": (0.15 * np.cos(pos @ k)[:, None] * tan[:, :3] + 0.05 * rng.normal(size=pos.shape)).astype(F),
                    "tangents": (0.15 * wave * np.cross(nrm, tan[:, :3]) + 0.05 * rng.normal(size=pos.shape)).astype(F)})
    return out


ANIMATED = np.array([0.6, -0.4, 0.8], dtype=F)


def _skinned_tube_scene(seed, sets, scaled=False, total=1.0, morphs=False, around=12, along=20, material=None):
    rng = np.random.default_rng(seed)
    nodes = [NodeDesc()]
    skin, jy = _rig(nodes, rng, scaled=scaled)
    patch = _tube(around, along)
    joints, weights = _skin_sets(rng, patch[0], jy, sets, total)
    kw = dict(joints=joints, weights=weights)
    if morphs:
        kw.update(morph_targets=_morph_targets(rng, patch[0], patch[1], patch[2]), morph_weights=np.zeros(3, dtype=F), animated_morph_weights=ANIMATED.copy())
    nodes.append(NodeDesc(parent=0, rotation=scenes.quat_axis_angle((0.2, 1.0, 0.1), 0.4), primitives=[_prim(patch, 0, **kw)], skin=0))
    return _scene(nodes, [material or _mat()], rng, eye=(0.9, 0.5, 3.6), skins=[skin])


# ------------------------------------------------------------------------------------------------ the cases

def two_sets():
    return _skinned_tube_scene(0x5E7502, 2)


def three_sets():
    return _skinned_tube_scene(0x5E7503, 3)


def scaled_joints():
    return _skinned_tube_scene(0x5CA1ED, 2, scaled=True)


def weights_not_normalised():
    return _skinned_tube_scene(0x0707, 2, total=0.7)


def tangent_morphs():
    rng = np.random.default_rng(0x7A6E)
    patch = _tube(24, 22)                      # 25 x 23 = 575 vertices, 1056 triangles
    assert patch[0].shape[0] > 512
    prim = _prim(patch, 0, morph_targets=_morph_targets(rng, patch[0], patch[1], patch[2]), morph_weights=np.zeros(3, dtype=F), animated_morph_weights=ANIMATED.copy())
    nodes = [NodeDesc(), NodeDesc(parent=0, rotation=scenes.quat_axis_angle((0.3, 1.0, 0.2), 0.6), scale=(1.1, 0.9, 1.2), primitives=[prim])]
    return _scene(nodes, [_mat()], rng, eye=(0.9, 0.5, 3.6))


def morph_then_skin(material=None):
    return _skinned_tube_scene(0x304F, 3, morphs=True, around=24, along=22, material=material)


def static_morph_weights():
    rng = np.random.default_rng(0x57A71C)
    nodes = [NodeDesc()]
    for i, w in enumerate(([0.9, -0.5, 0.7], [0.4, 0.6, -0.3])):
        patch = _ball(10, 8, radius=0.6, k=(2.0 + i, 3.0, 4.0 - i))
        prim = _prim(patch, 0, morph_targets=_morph_targets(rng, patch[0], patch[1], patch[2], amp=0.2), morph_weights=np.array(w, dtype=F))
        nodes.append(NodeDesc(parent=0, translation=(-0.8 + 1.6 * i, 0.0, 0.0), rotation=scenes.quat_axis_angle((0.1, 1.0, 0.3), 0.5 + i), primitives=[prim]))
    return _scene(nodes, [_mat()], rng, eye=(0.2, 0.4, 3.4))


def mirrored(blend=False):
    rng = np.random.default_rng(0x3122)
    mk = _blend if blend else _mat
    mats = [mk(double_sided=False), mk(double_sided=True, metallic_factor=0.6)]
    inst = [((1.3, 0.5, 0.0), scenes.quat_axis_angle((0.2, 1.0, 0.0), 0.3), (0.7, 0.7, 0.7)),
            ((1.3, -0.6, 0.2), scenes.quat_axis_angle((1.0, 0.3, 0.2), 0.8), (0.8, -0.6, 0.7))]
    nodes = [NodeDesc(),
             NodeDesc(parent=0, translation=(-1.3, 0.0, 0.0), rotation=scenes.quat_axis_angle((0.3, 1.0, 0.1), 0.5), scale=(-1.0, 1.0, 1.0), primitives=[_prim(_ball(), 0)]),
             NodeDesc(parent=0, translation=(0.0, 0.1, 0.0), rotation=scenes.quat_axis_angle((1.0, 0.2, 0.4), 0.9), scale=(-1.0, 1.0, 1.0),
                      primitives=[_prim(_ball(k=(4.0, 2.0, 3.0)), 1)]),
             NodeDesc(parent=0, primitives=[_prim(_ball(10, 7, radius=0.45), 0, instances=inst)]),
             NodeDesc(parent=0, translation=(0.0, -0.1, -0.6), primitives=[_prim(_ball(10, 7, radius=0.4, k=(3.0, 3.0, 1.0)), 1, instances=[
                 ((-0.4, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (-0.9, 0.8, 1.1))])])]
    return _scene(nodes, mats, rng, eye=(0.3, 0.4, 4.2))


def _scaled_models(seed, scales):
    """bumpy spheres under the given node scales, seen from close enough to cover pixels (the near plane scaled with them)"""
    rng = np.random.default_rng(seed)
    size = float(np.mean([abs(v) for s in scales for v in s]))
    nodes = [NodeDesc()]
    for i, s in enumerate(scales):
        x = (i - (len(scales) - 1) / 2) * 1.3 * size
        nodes.append(NodeDesc(parent=0, translation=(x, 0.0, 0.0), rotation=scenes.quat_axis_angle((0.3, 1.0, 0.2), 0.4 + i), scale=s, primitives=[_prim(_ball(), 0)]))
    return _scene(nodes, [_mat()], rng, eye=(0.3 * size, 0.4 * size, 3.2 * size), near=0.1 * size, far=100.0 * size)


def tiny_model():
    return _scaled_models(0x7101, [(0.00125,) * 3, (0.001, 0.002, 0.001)])          # det 1.95e-9, 2e-9: the fallback  M * normal


def just_above():
    return _scaled_models(0x7102, [(0.0035,) * 3, (0.002, 0.004, 0.0055)])          # det 4.29e-8, 4.4e-8: the cofactor path


def _cube_with_tangents():
    box = scenes.box_scene().nodes[1].primitives[0]
    faces_a = [(1, 0, 0), (-1, 0, 0), (0, 0, -1), (0, 0, 1), (1, 0, 0), (1, 0, 0)]           # box_scene's first in-face axis per face
    tan = np.array([list(a) + [1.0] for a in faces_a for _ in range(4)], dtype=F)
    uv = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=F), (6, 1))
    return box.positions.copy(), box.normals.copy(), tan, uv, box.indices.copy()


def instanced_morphed():
    rng = np.random.default_rng(0x1257)
    pos, nrm, tan, uv, idx = _cube_with_tangents()
    inst = [((-1.2, 0.0, 0.0), scenes.quat_axis_angle((0.2, 1.0, 0.1), 0.5), (0.9, 0.9, 0.9)),
            ((1.1, 0.1, 0.0), scenes.quat_axis_angle((0.5, 1.0, 0.3), 1.1), (-0.8, 0.9, 1.0)),              # mirrored
            ((0.0, 0.9, 0.5), scenes.quat_axis_angle((0.0, 1.0, 0.0), 0.2), (0.00125, 0.00125, 0.00125))]  # tiny: det 1.95e-9
    prim = PrimitiveDesc(positions=pos, normals=nrm, tangents=tan, uvs=[uv], indices=idx, material=0, instances=inst,
                         morph_targets=_morph_targets(rng, pos, nrm, tan, amp=0.25), morph_weights=np.zeros(3, dtype=F), animated_morph_weights=ANIMATED.copy())
    nodes = [NodeDesc(), NodeDesc(parent=0, rotation=scenes.quat_axis_angle((1.0, 0.2, 0.0), 0.3), primitives=[prim])]
    return _scene(nodes, [_mat(double_sided=True)], rng, eye=(0.4, 0.6, 4.0))


def tangent_parallel():
    rng = np.random.default_rng(0x7A11)

    def cap(sign):
        def fn(U, V):
            d = np.stack([sign * (U - 0.5) * 0.3, (V - 0.5) * 0.3, np.full_like(U, float(sign))], axis=-1)
            return d / np.linalg.norm(d, axis=-1, keepdims=True)
        return fn

    prims = []
    for patch in (scenes.grid_patch(cap(1.0), 9, 9), scenes.grid_patch(cap(-1.0), 9, 9), _ball(10, 8, radius=0.6)):
        pos, nrm, tan, uvs, idx = patch
        tan = np.concatenate([nrm, np.ones((len(nrm), 1), dtype=F)], axis=1).astype(F)         # tangent exactly along the normal
        prims.append(PrimitiveDesc(positions=pos, normals=nrm, tangents=tan, uvs=[uvs], indices=idx, material=0))
    nodes = [NodeDesc(),
             NodeDesc(parent=0, translation=(-0.5, 0.0, -1.0), scale=(1.5, 1.5, 1.5), primitives=[prims[0]]),       # normals around +z: |n.z| > 0.999 in the middle
             NodeDesc(parent=0, translation=(0.5, 0.0, 1.0), scale=(1.5, 1.5, 1.5), primitives=[prims[1]]),        # normals around -z
             NodeDesc(parent=0, translation=(0.0, 0.8, 0.0), rotation=scenes.quat_axis_angle((0.4, 1.0, 0.2), 0.7), primitives=[prims[2]])]   # oblique
    return _scene(nodes, [_mat(double_sided=True)], rng, eye=(0.3, 0.5, 3.6))


BLOCK_EDGE_TRIANGLES = (1, 85, 86, 171, 256)


def block_edges():
    rng = np.random.default_rng(0xB10C)
    nodes = [NodeDesc()]
    skin, jy = _rig(nodes, rng)
    for i, t in enumerate(BLOCK_EDGE_TRIANGLES):
        pos, nrm, tan, uvs, idx = _tube(12, 11, radius=0.2)        # 264 triangles, cut to the count wanted (the unused vertices stay in the mesh)
        kw = {}
        skinned = t in (85, 171)
        if skinned:
            j, w = _skin_sets(rng, pos, jy, 2)
            kw = dict(joints=j, weights=w)
        prim = PrimitiveDesc(positions=pos, normals=nrm, tangents=tan, uvs=[uvs], indices=idx[:t].copy(), material=i % 2, **kw)
        nodes.append(NodeDesc(parent=0, translation=(-1.4 + 0.7 * i, 0.0, 0.1 * i), rotation=scenes.quat_axis_angle((0.1, 1.0, 0.2), 0.3 * i), primitives=[prim],
                              skin=0 if skinned else None))
    return _scene(nodes, [_mat(double_sided=True), _mat(double_sided=False, metallic_factor=0.5)], rng, eye=(0.2, 0.3, 4.0), skins=[skin])


def blend_twins():
    """morph_then_skin's mesh and mirrored's nodes once more, with blend materials, in front of a small opaque wall"""
    a, b = morph_then_skin(material=_blend(double_sided=True)), mirrored(blend=True)
    rng = np.random.default_rng(0xB7E4D)
    nodes = list(a.nodes)
    shift = len(nodes) - 1                           # b's root (its node 0) becomes a's root
    for n in b.nodes[1:]:
        nodes.append(NodeDesc(translation=n.translation, rotation=n.rotation, scale=n.scale, parent=0 if n.parent == 0 else n.parent + shift, skin=n.skin,
                              primitives=[PrimitiveDesc(**{**p.__dict__, "material": p.material + 1}) for p in n.primitives]))
    wall = scenes.grid_patch(lambda U, V: np.stack([(U - 0.5) * 6.0, (V - 0.5) * 4.0, np.full_like(U, -1.5)], axis=-1), 6, 4)
    nodes.append(NodeDesc(parent=0, rotation=scenes.quat_axis_angle((1.0, 0.6, 0.3), 0.25), primitives=[_prim(wall, 3)]))      # tilted: its tangent is not the fallback's
    sc = _scene(nodes, [a.materials[0]] + list(b.materials) + [_mat()], rng, eye=(0.3, 0.4, 4.4), skins=a.skins)
    return sc


CASES = {
    "two_sets": two_sets, "three_sets": three_sets, "scaled_joints": scaled_joints, "weights_not_normalised": weights_not_normalised,
    "tangent_morphs": tangent_morphs, "morph_then_skin": morph_then_skin, "static_morph_weights": static_morph_weights, "mirrored": mirrored,
    "tiny_model": tiny_model, "just_above": just_above, "instanced_morphed": instanced_morphed, "tangent_parallel": tangent_parallel,
    "block_edges": block_edges, "blend_twins": blend_twins,
}


# ------------------------------------------------------------------------------------------------ conditions on the inputs

def check_inputs(name: str, model, ref: dict):
    """`ref`: the restatement's concatenated result for every draw of the case (opaque and transparent lists).  Every vertex takes part."""
    scene = model.scene
    for node in scene.nodes:                                     # no case may read outside a buffer
        for p in node.primitives:
            assert all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in (p.positions, p.normals, p.tangents)), name
            assert int(np.asarray(p.indices).max()) < p.positions.shape[0], name
            if p.joints:
                assert node.skin is not None and len(p.joints) == len(p.weights), name
                n_joints = len(scene.skins[node.skin].joints)
                for j, w in zip(p.joints, p.weights):
                    assert j.shape == w.shape == (p.positions.shape[0], 4) and int(j.max()) < n_joints, name
            for t in p.morph_targets:
                assert all(v.shape == p.positions.shape for v in t.values()), name
    for k in ("clip", "wpos", "normal", "tangent"):
        assert np.isfinite(ref[k]).all(), (name, k)
    assert (ref["normal_len"] > 0.0).all() and np.isfinite(ref["normal_len"]).all(), name            # no zero normal after morph, skin or model matrix
    assert (ref["det_factor"] >= MARGIN).all(), (name, "det", float(ref["det_factor"].min()))
    assert (ref["tan_factor"] >= MARGIN).all(), (name, "tlen_sq", float(ref["tan_factor"].min()))
    gs = ref["tan_gram_schmidt"]
    if name == "tangent_parallel":
        assert not gs.any(), name
        assert set(np.unique(ref["fallback_axis"])) == {1, 2}, name                                  # both fallback axes
        nz = ref["normal"][:, 2]
        assert (nz > 0.999).any() and (nz < -0.999).any() and (np.abs(nz) < 0.9).any(), name
        assert (np.abs(np.abs(nz) - vsr.FALLBACK_Y_ABOVE) >= NZ_MARGIN).all(), (name, float(np.abs(np.abs(nz) - vsr.FALLBACK_Y_ABOVE).min()))
    else:
        assert gs.all(), name
        assert (ref["ortho_ratio"] >= MIN_ORTHO_RATIO).all(), (name, float(ref["ortho_ratio"].min()))
        # a Gram-Schmidt tangent is told from a fallback one by its value (tests compare the branch taken): keep them apart
        assert (np.abs(ref["tangent"][:, :3] - ref["fallback_tangent"]).max(axis=1) >= 1e-3).all(), name
    # something on screen: vertices inside the frustum spanning at least a few pixels
    c = ref["clip"]
    inside = (c[:, 3] > 0) & (np.abs(c[:, 0]) < c[:, 3]) & (np.abs(c[:, 1]) < c[:, 3]) & (c[:, 2] > 0) & (c[:, 2] < c[:, 3])
    assert inside.sum() >= 3, name
    px = (c[inside, 0] / c[inside, 3]) * WIDTH / 2
    py = (c[inside, 1] / c[inside, 3]) * HEIGHT / 2
    assert px.max() - px.min() >= 8 and py.max() - py.min() >= 8, name
