"""`k_deform_transform` on the scenes of tests/vertex_stage_cases.py: bit-equal to the C oracle through the C-ABI (vertices, keys; colours at the bar of
compare_frames), and — so that the test stands even if oracle and kernel share a mistake — within the two measured tolerances of the float64 restatement
(tests/vertex_stage_reference.py).  Every vertex of every draw takes part in both."""
import numpy as np
import pytest

from tests import helpers
from tests import vertex_stage_cases as cases
from tests import vertex_stage_reference as vsr
from tests.test_gpu_parity import RGB_TOL, _check_host

pytestmark = pytest.mark.gpu

OPAQUE_CASES = [n for n in cases.CASES if n != "blend_twins"]
_models, _frames = {}, {}


def _model(name):
    if name not in _models:
        _models[name] = helpers.build_model(cases.CASES[name]())
    return _models[name]


def _frame(name, lut):
    """one single-sampled device frame per case, compared with the oracle's; the device's vertices are kept for the comparison with the restatement"""
    if name not in _frames:
        model = _model(name)
        orc = helpers.oracle_frame(model, lut)
        dev, stats = helpers.hip_frame(model, lut)
        r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
        clip, nt = dev.read_transformed(orc.n_verts)
        dev.close()
        _frames[name] = (r, stats, clip[:orc.n_verts].copy(), nt[:orc.n_verts].copy())
    return _frames[name]


def _assert_frame(r, stats=None):
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0, r
    assert r["key_mismatch"] == 0, r
    assert r["covered"] > 0, r
    assert r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    if stats is not None:
        assert stats["covered_pixels"] == r["covered"], (stats, r)


def _assert_restated(name, model, draws, ref, clip, nt, wpos=None):
    d = vsr.distances(ref, clip, nt, wpos)
    print("%-24s verts=%6d clip_rel=%.3e wpos_rel=%.3e normal_abs=%.3e tangent_abs=%.3e" % (
        name, len(ref["clip"]), d["clip_rel"], d.get("wpos_rel", 0.0), d["normal_abs"], d["tangent_abs"]))
    vsr.assert_within_tolerances(name, d)
    assert np.array_equal(vsr.f32_fallback_axis(nt), ref["fallback_axis"]), name
    assert np.array_equal(vsr.f32_det_branch(model, draws), ref["det_cofactor"]), name


@pytest.mark.parametrize("name", OPAQUE_CASES)
def test_case_is_bit_equal_to_the_oracle(name, oracle_lut):
    r, stats, _, _ = _frame(name, oracle_lut)
    _assert_frame(r, stats)


@pytest.mark.parametrize("name", OPAQUE_CASES)
def test_case_agrees_with_the_restatement(name, oracle_lut):
    _, _, clip, nt = _frame(name, oracle_lut)
    model = _model(name)
    _assert_restated(name, model, model.collect_draws(), vsr.restate(model)[1], clip, nt)


def test_mirrored_with_msaa4(oracle_lut):
    """facing decides which samples exist: the mirrored node's and instance's flipped winding under 4 samples per pixel"""
    model = _model("mirrored")
    orc = helpers.oracle_frame(model, oracle_lut, msaa=4)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=4)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    dev.close()
    _assert_frame(r, stats)


def test_blend_twins_through_the_indexed_variant(oracle_lut):
    """k_deform_transform<true>: the skinned and morphed tube and the mirrored meshes with blend materials, through the transparent pass"""
    model = _model("blend_twins")
    orc = helpers.oracle_frame(model, oracle_lut)
    tr = model.collect_transparent_draws()
    assert len(tr) >= 5
    orc.forward(tr)
    dev, stats = helpers.hip_frame(model, oracle_lut, transparent=True)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)          # the opaque wall underneath
    clip, nt = dev.read_transformed(orc.n_verts)
    c = helpers.compare_composite(orc, dev)
    fclip, fnt, fwpos = dev.read_transformed_forward(orc.fwd_n_verts)
    dev.close()
    _assert_frame(r)
    assert c["clip_mismatch"] == 0 and c["nt_mismatch"] == 0 and c["wpos_mismatch"] == 0, c
    assert c["touched_pixels"] > 500 and c["untouched_changed"] == 0, c
    helpers.assert_composite("vertex stage: blend_twins", c)
    assert stats["forward_triangles"] == sum(d["tri_count"] * max(1, d.get("inst_count", 0)) for d in tr)
    _assert_restated("blend_twins/opaque", model, model.collect_draws(), vsr.restate(model)[1], clip[:orc.n_verts], nt[:orc.n_verts])
    n = orc.fwd_n_verts
    _assert_restated("blend_twins/forward", model, tr, vsr.restate(model, transparent=True)[1], fclip[:n], fnt[:n], fwpos[:n])


@pytest.mark.parametrize("name", ["morph_then_skin", "instanced_morphed"])
def test_case_through_the_host_layer(name, oracle_lut):
    """host.cpp's multi-set skin packing, tangent deltas and instanced morphed meshes, on the product path"""
    _check_host(cases.CASES[name](), oracle_lut)


class _Reordered:
    """a model whose opaque draw list comes out in another order (everything else is the model's own)"""

    def __init__(self, model, order):
        self._model, self._order = model, order

    def __getattr__(self, k):
        return getattr(self._model, k)

    def collect_draws(self):
        d = self._model.collect_draws()
        return [d[i] for i in self._order]


def test_block_edges_with_the_draws_in_reverse_order(oracle_lut):
    """The same draws submitted back to front: every draw's vertices come back, bit for bit, at their new places (the first_block search and the
    block -> draw map), and the frame still equals the oracle's of that order."""
    _, _, clip, nt = _frame("block_edges", oracle_lut)
    model = _model("block_edges")
    draws = model.collect_draws()
    sizes = [3 * d["tri_count"] for d in draws]
    assert sorted(sizes) == [3, 255, 258, 513, 768]
    rev = _Reordered(model, list(range(len(draws)))[::-1])
    orc = helpers.oracle_frame(rev, oracle_lut)
    dev, stats = helpers.hip_frame(rev, oracle_lut)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    rclip, rnt = dev.read_transformed(orc.n_verts)
    dev.close()
    _assert_frame(r, stats)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    at = sum(sizes)
    for i, n in enumerate(sizes):          # draw i of the first order is draw len-1-i of the second
        at -= n
        assert np.array_equal(rclip[at:at + n].view(np.uint32), clip[starts[i]:starts[i] + n].view(np.uint32)), i
        assert np.array_equal(rnt[at:at + n].view(np.uint32), nt[starts[i]:starts[i] + n].view(np.uint32)), i
    assert at == 0
    _assert_restated("block_edges/reversed", model, rev.collect_draws(), vsr.restate(model, draws=rev.collect_draws())[1], rclip[:orc.n_verts], rnt[:orc.n_verts])
