"""The vertex stage on the CPU: the C oracle (`oracle_geometry.c: apply_vertex`, f32) against the float64 restatement written from the scene
description alone (tests/vertex_stage_reference.py), on scenes built to reach every branch and loop of the stage (tests/vertex_stage_cases.py).
No GPU; tests/test_vertex_stage_gpu.py holds the kernel to the same two parties."""
import numpy as np
import pytest

from oracle import oracle_lib
from tests import helpers
from tests import vertex_stage_cases as cases
from tests import vertex_stage_reference as vsr

_cache = {}


def prepared(name):
    """(model, oracle frame after transform() [and forward-vertices for the transparent list], restatement of both lists) — computed once per case"""
    if name not in _cache:
        scene = cases.CASES[name]()
        model = helpers.build_model(scene)
        lut = np.zeros((4, 4, 2), dtype=np.uint16)
        orc = oracle_lib.frame_from_model(model, lut).transform()
        per_draw, ref = vsr.restate(model)
        tr_draws = model.collect_transparent_draws()
        fwd_ref = vsr.restate(model, transparent=True)[1] if tr_draws else None
        _cache[name] = (model, orc, per_draw, ref, tr_draws, fwd_ref)
    return _cache[name]


def forward_vertices(orc, draws):
    """the transparent pass's vertex stage alone (OracleFrame.forward without the fragment work)"""
    import ctypes as C
    L = oracle_lib.lib()
    arr = (oracle_lib.AwsmDraw * max(1, len(draws)))()
    for i, d in enumerate(draws):
        arr[i] = oracle_lib.AwsmDraw(d["geom_meta_off"], d["vis_data_off"], d["tri_count"], d["flags"], d.get("inst_off", 0), d.get("inst_count", 0))
    L.oracle_forward_total_vertices.restype = C.c_uint32
    nv = int(L.oracle_forward_total_vertices(arr, C.c_uint32(len(draws))))
    clip, nt, wpos = np.zeros((nv, 4), dtype=np.float32), np.zeros((nv, 8), dtype=np.float32), np.zeros((nv, 4), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.oracle_forward_transform(C.byref(orc.scene), arr, C.c_uint32(len(draws)), p(clip), p(nt), p(wpos)) == 0
    return clip, nt, wpos


def _all_ref(ref, fwd_ref):
    return ref if fwd_ref is None else {k: np.concatenate([ref[k], fwd_ref[k]]) for k in ref}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_inputs_meet_their_conditions(name):
    model, orc, per_draw, ref, tr_draws, fwd_ref = prepared(name)
    cases.check_inputs(name, model, _all_ref(ref, fwd_ref))
    if name == "block_edges":
        assert sorted(len(r["clip"]) for r in per_draw) == [3, 255, 258, 513, 768]
        assert sum(1 for r in per_draw if (r["skin_det"] != 1.0).any()) == 2
    if name in ("mirrored", "instanced_morphed", "blend_twins"):
        assert (_all_ref(ref, fwd_ref)["det"] < 0).any() and (_all_ref(ref, fwd_ref)["det"] > 0).any()
    if name in ("tiny_model", "instanced_morphed"):
        assert (~ref["det_cofactor"]).any()
    if name == "tiny_model":
        assert not ref["det_cofactor"].any()
    if name == "just_above":
        assert ref["det_cofactor"].all() and (ref["det_factor"] < 8).all()
    if name == "scaled_joints":      # not rigid: the blended 3x3 is far from a rotation
        assert np.abs(ref["skin_det"] - 1.0).max() > 0.05
    if name == "blend_twins":
        assert len(tr_draws) >= 5 and any(d.get("inst_count", 0) for d in tr_draws)
    # covers pixels: the oracle's own raster of the opaque list (every case has one)
    assert int((orc.raster(2).keys != oracle_lib.NO_HIT_KEY).sum()) > 20, name


def _compare(name):
    """[(which list, distances, restatement, the oracle's normal/tangent, draws)] of a case: the opaque list and, where there is one, the transparent"""
    model, orc, per_draw, ref, tr_draws, fwd_ref = prepared(name)
    runs = [("opaque", vsr.distances(ref, orc.clip[:orc.n_verts], orc.nt[:orc.n_verts]), ref, orc.nt[:orc.n_verts], model.collect_draws())]
    if tr_draws:
        clip, nt, wpos = forward_vertices(orc, tr_draws)
        runs.append(("forward", vsr.distances(fwd_ref, clip, nt, wpos), fwd_ref, nt, tr_draws))
    return model, runs


@pytest.mark.parametrize("name", list(cases.CASES))
def test_oracle_against_the_restatement(name):
    """Every vertex: clip (and world position where the oracle returns it) relative to the vertex's largest component, normal and tangent
    absolutely, handedness and the branch taken exactly."""
    model, runs = _compare(name)
    for which, d, r, nt, draws in runs:
        vsr.assert_within_tolerances(name + "/" + which, d)
        assert np.array_equal(vsr.f32_det_branch(model, draws), r["det_cofactor"]), (name, which)
        assert np.array_equal(vsr.f32_fallback_axis(nt), r["fallback_axis"]), (name, which)


def test_the_committed_tolerances_are_four_times_the_worst_distance():
    """Prints every case's distances and the worst of each kind (pytest -s shows them): POSITION_REL_TOL and DIRECTION_ABS_TOL are those worst values
    x 4, as measured when the cases were written.  A later reader re-measures here; the tolerances must at least cover what is seen."""
    worst = {"position_rel": 0.0, "direction_abs": 0.0}
    for name in cases.CASES:
        for which, d, r, nt, draws in _compare(name)[1]:
            print("%-24s %-8s verts=%6d clip_rel=%.3e wpos_rel=%.3e normal_abs=%.3e tangent_abs=%.3e" % (
                name, which, len(r["clip"]), d["clip_rel"], d.get("wpos_rel", 0.0), d["normal_abs"], d["tangent_abs"]))
            worst["position_rel"] = max(worst["position_rel"], d["clip_rel"], d.get("wpos_rel", 0.0))
            worst["direction_abs"] = max(worst["direction_abs"], d["normal_abs"], d["tangent_abs"])
    print("worst oracle-to-restatement distances: position_rel=%.3e direction_abs=%.3e   (committed tolerances: %.3e, %.3e)" % (
        worst["position_rel"], worst["direction_abs"], vsr.POSITION_REL_TOL, vsr.DIRECTION_ABS_TOL))
    assert worst["position_rel"] <= vsr.POSITION_REL_TOL and worst["direction_abs"] <= vsr.DIRECTION_ABS_TOL, worst


def test_static_morph_weights_reach_the_shader_shifted_by_one():
    """morph.wgsl reads weight i at float [off/4 + 1 + i]; Morphs::insert_raw writes glTF `mesh.weights` at [0, n).  Faithful to the reference, and
    surprising: the effective weights of a mesh with static weights w are w[1:] followed by the float behind them.  The oracle agrees with the
    restatement under exactly this reading and disagrees, by far more than the tolerance, under the naive one."""
    model, orc, per_draw, ref, _, _ = prepared("static_morph_weights")
    draws = model.collect_draws()
    offs = []
    for d in draws:
        node, p = vsr.primitive_of(model, d["mesh_key"])
        rec = model.meshes.get(d["mesh_key"])
        n = len(p.morph_targets)
        assert p.animated_morph_weights is None and n == 3
        off = model.morph_weights.offset(rec.morph_key)
        offs.append(off)
        raw = np.frombuffer(bytes(model.morph_weights.raw), dtype=np.float32)
        behind = raw[off // 4 + n]
        eff = vsr.effective_morph_weights(model, rec.morph_key, n)
        assert np.array_equal(eff, np.concatenate([np.asarray(p.morph_weights, dtype=np.float32)[1:], [behind]]).astype(np.float64))
        assert np.array_equal(vsr.naive_morph_weights(model, rec.morph_key, n), np.asarray(p.morph_weights, dtype=np.float32).astype(np.float64))
        assert behind == 0.0          # padding of the mesh's own 256-byte block, not its neighbour's first weight
    assert abs(offs[0] - offs[1]) == 256          # neighbours
    vsr.assert_within_tolerances("static_morph_weights", vsr.distances(ref, orc.clip[:orc.n_verts], orc.nt[:orc.n_verts]))
    naive = vsr.restate(model, weights_fn=vsr.naive_morph_weights)[1]
    d = vsr.distances(naive, orc.clip[:orc.n_verts], orc.nt[:orc.n_verts])
    print("under the naive reading: clip_rel=%.3e normal_abs=%.3e tangent_abs=%.3e" % (d["clip_rel"], d["normal_abs"], d["tangent_abs"]))
    assert d["clip_rel"] > 1000 * vsr.POSITION_REL_TOL and d["normal_abs"] > 1000 * vsr.DIRECTION_ABS_TOL and d["tangent_abs"] > 1000 * vsr.DIRECTION_ABS_TOL, d


def test_animated_weights_land_where_they_are_read():
    """the other half of the rule: weights written through the animation path are the effective ones, unshifted"""
    model = prepared("tangent_morphs")[0]
    d = model.collect_draws()[0]
    rec = model.meshes.get(d["mesh_key"])
    assert np.array_equal(vsr.effective_morph_weights(model, rec.morph_key, 3), cases.ANIMATED.astype(np.float64))
    assert (cases.ANIMATED < 0).sum() == 1
