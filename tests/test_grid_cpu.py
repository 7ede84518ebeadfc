"""CPU tests of the editor's ground grid: the numpy restatement against known answers and against itself in f64, the host layer over a
backend that lacks the entry points, and the defaults the library hands out."""
import ctypes as C

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from tests import grid_reference as gr
from tests.test_host_layer_cpu import MOCK, mock  # noqa: F401  (the module-scoped fixture)

CASES = [(name, W, Hh) for name in gr.CAMERAS for (W, Hh) in gr.SIZES]


# ------------------------------------------------------------------------------------------------ known answers, f64

def _top_down(W=240, half=12.0):
    """A straight-down orthographic camera over the origin: 2 * half world units on W pixels, +X to the right, +Z down the image."""
    block = gr.camera_block((0.0, 10.0, 0.0), (0.0, 0.0, 0.0), W, W, ortho_half_height=half, up=(0.0, 0.0, -1.0))
    f = gr.fragment(block, W, W, np.float64)
    px = 2.0 * half / W                                                        # world units per pixel
    centre = (np.arange(W) + 0.5) * px - half                                  # world x of a column, world z of a row
    return f, px, centre


def test_top_down_camera_draws_lines_at_integers_and_major_lines_at_tens():
    f, px, centre = _top_down()
    assert f["kept"].all()
    wx, _, wz = f["world_pos"]
    assert np.abs(wx - centre[None, :]).max() < 1e-5 and np.abs(wz - centre[:, None]).max() < 1e-5      # (the block's f32 entries)
    # fwidth of a coordinate: one pixel along its own axis, nothing along the other
    dist = lambda c, period: np.abs((c / period - 0.5) % 1.0 - 0.5) * period / px      # distance to the nearest line, in pixels
    dmin = np.minimum(dist(centre, 1.0)[None, :], dist(centre, 1.0)[:, None])
    dmaj = np.minimum(dist(centre, 10.0)[None, :], dist(centre, 10.0)[:, None])
    axis = (np.abs(centre)[None, :] < px) | (np.abs(centre)[:, None] < px)
    clear = lambda d, edge: np.abs(d - edge) > 0.02                                 # away from the rim of a line's footprint
    on_minor = (dmin < 0.99 - 0.01 / 0.9) & clear(dmin, 0.99)
    assert on_minor.sum() > 5000 and (f["cls"][on_minor & (dmaj > 1.01) & ~axis] == gr.MINOR).all()
    assert (f["cls"][(dmin > 1.01) & (dmaj > 1.01) & ~axis] == gr.BACKGROUND).all() and ((dmin > 1.01) & ~axis).sum() > 20000
    on_major = (dmaj < 0.98) & ~axis
    assert on_major.sum() > 1500 and (f["cls"][on_major] == gr.MAJOR).all()
    # a column through world x = 10 and one through x = 3: a major line and a minor one, away from the other lines' rows
    col10, col3, row = int(np.argmin(np.abs(centre - 10.0))), int(np.argmin(np.abs(centre - 3.0))), int(np.argmin(np.abs(centre - 4.5)))
    assert f["cls"][row, col10] == gr.MAJOR and f["cls"][row, col3] == gr.MINOR
    assert np.allclose(f["rgba"][row, col10, :3], np.float32(0.38)) and np.allclose(f["rgba"][row, col3, :3], np.float32(0.28))


def test_x_axis_wins_over_z_axis_at_the_origin():
    f, px, centre = _top_down()
    c = int(np.argmin(np.abs(centre)))                                         # the pixel nearest the origin: both axes pass through its footprint
    a = f["alphas"][c, c]
    assert a[2] > 0.01 and a[3] > 0.01 and f["cls"][c, c] == gr.X_AXIS
    assert np.allclose(f["rgba"][c, c, :3], np.float32([0.95, 0.3, 0.3]))
    far = int(np.argmin(np.abs(centre - 4.5)))
    assert f["cls"][c, far] == gr.X_AXIS and f["cls"][far, c] == gr.Z_AXIS    # along z = 0 red, along x = 0 blue


@pytest.mark.parametrize("name", ["down", "below", "ortho"])
def test_depth_is_the_projected_depth_of_the_hit_plus_epsilon(name):
    W, Hh = 64, 48
    block = gr.camera(name, W, Hh)
    f = gr.fragment(block, W, Hh, np.float64)
    view = np.frombuffer(block, np.float32, 16, 0).reshape(4, 4).astype(np.float64).T       # as matrices
    proj = np.frombuffer(block, np.float32, 16, 64).reshape(4, 4).astype(np.float64).T
    wx, wy, wz = f["world_pos"]
    assert np.abs(wy[f["kept"]]).max() < 1e-9                                               # on the plane
    clip = np.einsum("ij,hwj->hwi", proj @ view, np.stack([wx, wy, wz, np.ones_like(wx)], axis=-1))
    want = np.clip(clip[..., 2] / clip[..., 3] + float(np.float32(1e-4)), 0.0, 1.0)
    k = f["kept"]
    assert k.sum() > 2500 and np.abs(f["depth"][k] - want[k]).max() < 1e-12
    eps = gr.fragment(block, W, Hh, np.float64, {"depth_epsilon": 0.25})
    inside = k & (want < 0.7)
    if inside.any():
        assert np.abs((eps["depth"] - f["depth"])[inside] - (0.25 - float(np.float32(1e-4)))).max() < 1e-12


def test_rows_above_the_horizon_discard_and_the_plane_shows_from_underneath():
    for W, Hh in gr.SIZES:
        f = gr.fragment(gr.camera("horizon", W, Hh), W, Hh, np.float64)
        k = f["kept"]
        assert not k[0].any() and k[-1].all() and 0.40 < 1.0 - k.mean() < 0.50             # about 45 % of the pixels
        assert (np.diff(k.astype(np.int8), axis=0) >= 0).all()                              # down a column: discarded, then kept, never back
        assert (f["t"][~k & (np.abs(f["ray_dir_y"]) >= 0.001)] < 0).all()                   # what is discarded looks away from the plane
        below = gr.fragment(gr.camera("below", W, Hh), W, Hh, np.float64)
        assert below["kept"].all() and (below["t"] > 0).all() and (below["ray_dir_y"] > 0).all()
        assert not gr.fragment(gr.camera("up", W, Hh), W, Hh, np.float64)["kept"].any()


def test_every_colour_class_occurs():
    for name in ("down", "horizon", "below", "ortho"):
        for W, Hh in gr.SIZES:
            cls = gr.fragment(gr.camera(name, W, Hh), W, Hh, np.float64)["cls"]
            counts = [int((cls == c).sum()) for c in range(5)]
            assert min(counts[1:]) >= 110 and (counts[0] >= 110 or name == "ortho"), (name, W, Hh, counts)


# ------------------------------------------------------------------------------------------------ f32 against f64

def _distances(name, W, Hh):
    block = gr.camera(name, W, Hh)
    f32, f64 = gr.fragment(block, W, Hh, np.float32), gr.fragment(block, W, Hh, np.float64)
    near = gr.near_threshold(f64)
    kept = f64["kept"]
    sure = ~near
    with np.errstate(all="ignore"):
        da = np.abs(f32["alphas"].astype(np.float64) - f64["alphas"])
        da = np.where(np.isnan(f32["alphas"]) & np.isnan(f64["alphas"]), 0.0, da)
    pick = sure & kept
    return {"f32": f32, "f64": f64, "near_kept": int((near & kept).sum()), "kept": int(kept.sum()), "sure": sure,
            "alpha": float(da[pick].max()) if pick.any() else 0.0,
            "depth": float(np.abs(f32["depth"].astype(np.float64) - f64["depth"])[pick].max()) if pick.any() else 0.0}


@pytest.mark.parametrize("name,W,Hh", CASES)
def test_f32_run_decides_as_the_f64_run_away_from_the_thresholds(name, W, Hh):
    d = _distances(name, W, Hh)
    print("%-8s %dx%d kept=%d near_threshold=%d alpha=%.3e depth=%.3e" % (name, W, Hh, d["kept"], d["near_kept"], d["alpha"], d["depth"]))
    s = d["sure"]
    assert (d["f32"]["kept"][s] == d["f64"]["kept"][s]).all() and (d["f32"]["cls"][s] == d["f64"]["cls"][s]).all()
    assert d["near_kept"] <= 0.01 * d["kept"], d["near_kept"]                               # the cap: at most 1 % of a case's kept pixels
    assert d["alpha"] <= gr.GRID_ALPHA_SLACK and d["depth"] <= gr.GRID_DEPTH_SLACK, (d["alpha"], d["depth"])
    if name == "up":
        assert d["kept"] == 0 and not d["f32"]["kept"].any()


def test_the_committed_slacks_are_four_times_the_worst_distance():
    """GRID_ALPHA_SLACK and GRID_DEPTH_SLACK are the worst f32-to-f64 distances x 4, as measured when the cases were written (DESIGN.md §17 has
    the table).  A later reader re-measures here (pytest -s prints them); the slacks must cover what is seen and not be idle."""
    worst = {"alpha": 0.0, "depth": 0.0}
    for name, W, Hh in CASES:
        d = _distances(name, W, Hh)
        worst = {k: max(worst[k], d[k]) for k in worst}
    print("worst f32-to-f64 distances: alpha=%.3e depth=%.3e   (committed slacks: %.3e, %.3e)" % (worst["alpha"], worst["depth"], gr.GRID_ALPHA_SLACK, gr.GRID_DEPTH_SLACK))
    assert worst["alpha"] <= gr.GRID_ALPHA_SLACK <= 8 * worst["alpha"] and worst["depth"] <= gr.GRID_DEPTH_SLACK <= 8 * worst["depth"], worst


def test_blend_rounds_to_f16_once_and_tests_each_sample():
    """One pixel by hand: src (0.28, 0.28, 0.28, 0.5) over dst (1, 0.5, 0.25, 1) where two of four samples pass."""
    layer = {"kept": np.array([[True]]), "rgba": np.array([[[0.28, 0.28, 0.28, 0.5]]], np.float32), "depth": np.array([[0.5]], np.float32)}
    dst = np.array([[[1.0, 0.5, 0.25, 1.0]]], np.float16).view(np.uint16)
    depth_s = np.array([[[0.6, 0.5, 0.4, 1.0]]], np.float32)                               # Less: 0.5 < 0.5 fails
    assert gr.grid_passes(layer, depth_s).tolist() == [[[True, False, False, True]]]
    s = gr.blend_samples(dst, layer, depth_s)[0, 0]
    over = np.float32(0.28) * np.float32(0.5) + np.array([1.0, 0.5, 0.25], np.float32) * np.float32(0.5)
    assert (s[0, :3] == over.astype(np.float16).astype(np.float32)).all() and s[0, 3] == 1.0 and (s[1] == [1.0, 0.5, 0.25, 1.0]).all() and (s[3] == s[0]).all()
    want = ((((s[0] + s[1]) + s[2]) + s[3]) * np.float32(0.25)).astype(np.float16)
    assert (gr.blend(dst, layer, depth_s)[0, 0] == want.view(np.uint16)).all()
    assert (gr.blend(dst, layer, depth_s[..., :1])[0, 0] == s[0].astype(np.float16).view(np.uint16)).all()
    keys = np.array([[gr.NO_HIT, (np.uint64(np.float32(0.25).view(np.uint32)) << np.uint64(32)) | np.uint64(7)]], np.uint64)
    assert gr.world_depth(keys)[0, :, 0].tolist() == [1.0, 0.25]


# ------------------------------------------------------------------------------------------------ the libraries

def test_host_over_a_backend_without_the_grid_reports_unsupported_and_names_the_symbol(mock):
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    g = hip_backend.AwsmEditorGrid(struct_size=C.sizeof(hip_backend.AwsmEditorGrid))
    assert r.host.lib.awsm_host_set_editor_grid(r.host.h, C.byref(g)) == -6                 # AWSM_ERR_UNSUPPORTED
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_set_editor_grid"):
        r.host._chk(r.host.lib.awsm_host_set_editor_grid(r.host.h, C.byref(g)), "set_editor_grid")
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_set_editor_grid"):
        r.host.set_editor_grid(False)
    with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_editor_grid_defaults"):
        r.host.set_editor_grid(True)
    r.render()                                                                              # and renders as before
    r.close()


def test_the_library_hands_out_the_shader_constants():
    try:
        lib = hip_backend.load_library()
    except (OSError, FileNotFoundError) as e:
        pytest.skip("libawsm_hip does not load here: %s" % e)
    g = hip_backend.AwsmEditorGrid()
    assert lib.awsm_hip_editor_grid_defaults(C.byref(g)) == 0 and lib.awsm_hip_editor_grid_defaults(None) == -1
    assert g.struct_size == C.sizeof(hip_backend.AwsmEditorGrid) == 84
    for k, v in gr.DEFAULTS.items():
        got = getattr(g, k)
        want = np.float32(v)
        assert (list(got) == want.tolist()) if k.startswith("color_") else (got == float(want)), (k, got, v)
    with pytest.raises(TypeError):
        g.override(colour_minor=(1, 1, 1))
