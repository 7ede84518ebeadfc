"""CPU tests of the temporal anti-aliasing: the host's jitter, jittered camera block and reprojection matrix against their numpy
restatement over mock backends with and without the entry point, the record's layout, properties of the resolve's restatement, and the conditions
that keep tests/test_taa_gpu.py informative."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from oracle import oracle_lib
from tests import helpers
from tests import ssao_reference as sr
from tests import taa_reference as tr
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, mock  # noqa: F401  (the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BUF_CAMERA = 5
EYE, TARGET = (3.2, 2.6, 3.6), (0.6, 0.5, 0.6)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the host layer over the recording mock

@pytest.fixture(scope="module")
def mock_taa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mock_taa") / "libmock_backend_taa.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", out, os.path.join(MOCK_DIR, "mock_backend_taa.c")])
    lib = C.CDLL(out)
    lib.mock_buffer.restype = C.c_void_p
    lib.mock_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    lib.mock_taa_record.restype = C.c_uint32
    lib.mock_taa_record.argtypes = [C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    lib.mock_taa_calls.restype = C.c_uint32
    lib.mock_taa_posts.restype = C.c_uint32
    return out, lib


def _renderer(path, W=64, Hh=48, ortho=False):
    sc = scenes.box_scene(W, Hh)
    view, proj = tr.camera_matrices(EYE, TARGET, W, Hh, ortho_half_height=2.2 if ortho else None)
    sc.view, sc.proj, sc.camera_position = view, proj, tuple(float(F(v)) for v in EYE)
    r = H.Renderer(sc, backend_path=path, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    return r, sc


def _camera_on_device(lib, r):
    n = C.c_size_t()
    p = lib.mock_buffer(r.host.device_ctx, BUF_CAMERA, C.byref(n))
    return C.string_at(p, n.value)


def _last_record(lib):
    """-> (AwsmTaa or None for NULL, post passes the mock had seen before it)."""
    raw, posts = (C.c_uint8 * C.sizeof(hip_backend.AwsmTaa))(), C.c_uint32()
    size = lib.mock_taa_record(lib.mock_taa_calls() - 1, raw, C.sizeof(hip_backend.AwsmTaa), C.byref(posts))
    if size == 0xFFFFFFFF:
        return None, posts.value
    assert size == C.sizeof(hip_backend.AwsmTaa)
    return hip_backend.AwsmTaa.from_buffer_copy(bytes(raw)), posts.value


def test_host_jitter_is_the_f32_restatement_bit_for_bit(mock_taa):
    path, _ = mock_taa
    for W, Hh in ((64, 48), (70, 45), (33, 70)):
        r, _ = _renderer(path, W, Hh)
        for fc in range(64):
            for mv, s in ((False, tr.STRENGTH_STILL), (True, tr.STRENGTH_MOVING)):
                got, want = r.host.taa_jitter(fc, mv), tr.jitter_ndc(fc, mv, W, Hh)
                assert (_bits(got) == _bits(want)).all(), (W, Hh, fc, mv, got, want)
                s32 = float(F(s)) * (1.0 + 2.0 ** -22)      # the strength as the f32 it is, and the two roundings of (j / W) * s; frame 0 sits on the bound
                assert abs(float(got[0])) <= 0.5 * s32 / W and abs(float(got[1])) <= 0.5 * s32 / Hh
        r.set_taa(True, strength_still=1.0, strength_moving=0.5)      # an override reaches the rule
        assert (_bits(r.host.taa_jitter(7, False)) == _bits(tr.jitter_ndc(7, False, W, Hh, 1.0, 0.5))).all()
        assert (_bits(r.host.taa_jitter(7, True)) == _bits(tr.jitter_ndc(7, True, W, Hh, 1.0, 0.5))).all()
        r.close()
    assert tr.halton(0, 2) == 0 and tr.halton(1, 2) == F(0.5) and tr.halton(2, 2) == F(0.25) and tr.halton(3, 2) == F(0.75) and tr.halton(1, 3) == F(1) / F(3)


@pytest.mark.parametrize("ortho", [False, True])
def test_host_writes_the_jittered_block_and_composes_the_record(mock_taa, ortho):
    """Every frame: the 512 bytes on the (mock) device are the block packed from translation(jitter) * proj, and the record handed over in front of
    the post pass holds that jitter and view_proj_prev * inverse(view_proj_cur) — the exact identity while the camera stands, the f64 composition
    rounded once after an orbit step.  AWSM_TAA_RESET goes out with the first record and once more after a resize."""
    path, lib = mock_taa
    W, Hh = 70, 45
    r, sc = _renderer(path, W, Hh, ortho)
    pos = sc.camera_position
    r.render()
    plain = tr.block(sc.view, sc.proj, pos, 0, W, Hh)      # awsm_host_camera_update packed it before the first render: frame count 0
    assert _camera_on_device(lib, r) == plain
    with pytest.raises(H.HostError, match=r"\(-1\).*awsm_host_set_post_processing"):      # it resolves in the post pass
        r.set_taa(True)
        r.render()
    r.set_post_processing(1)
    calls0, fc, prev = lib.mock_taa_calls(), 2, None
    flags = []
    for step in (0, 0, 0, 5.0, 5.0, 0, "resize", 0):
        if step == "resize":
            r.host.resize(W, Hh)
        elif step:
            view, _ = tr.camera_matrices(tr.orbit(EYE, TARGET, step * (len(flags) - 1)), TARGET, W, Hh, ortho_half_height=2.2 if ortho else None)
            r.scene.view = view
            r.update()
        view, proj = np.asarray(r.scene.view, F), np.asarray(r.scene.proj, F)
        posts0 = lib.mock_taa_posts()
        r.render()
        fc += 1
        mv = tr.moved(prev, view, proj)
        j = tr.jitter_ndc(fc, mv, W, Hh)
        assert _camera_on_device(lib, r) == tr.block(view, tr.jitter_proj(proj, j), pos, fc, W, Hh), (step, fc)
        rec, posts_before = _last_record(lib)
        assert posts_before == posts0 and lib.mock_taa_posts() == posts0 + 1                 # the record first, then the frame's post pass
        assert rec.struct_size == C.sizeof(hip_backend.AwsmTaa) and rec.feedback == F(0.1)
        assert (_bits(np.array(rec.jitter_ndc[:], F)) == _bits(j)).all()
        want_R = tr.reproject(prev, view, proj)
        assert (_bits(np.array(rec.reproject[:], F)) == _bits(want_R)).all(), (step, np.array(rec.reproject[:]), want_R)
        if prev is not None and not mv:
            assert (want_R == tr.IDENTITY).all()
        if step and step != "resize":
            assert mv and (want_R != tr.IDENTITY).any()
        flags.append(rec.flags)
        prev = (view.copy(), proj.copy())
    assert lib.mock_taa_calls() == calls0 + len(flags)
    assert flags == [1, 0, 0, 0, 0, 0, 1, 0], flags
    # off: NULL goes through, and the block awsm_host_camera_update packed goes up again as it was
    r.set_taa(False)
    assert _last_record(lib)[0] is None
    r.render()
    kept = tr.block(r.scene.view, r.scene.proj, pos, 6, W, Hh)      # packed by the last r.update(), when six renders had been counted
    assert _camera_on_device(lib, r) == kept
    r.close()


def test_host_refusals_and_overrides(mock_taa):
    path, lib = mock_taa
    r, _ = _renderer(path)
    r.set_post_processing(1)
    for bad in (H.HostTaa(0, 0.1, 0.8, 0.2), H.HostTaa(3, 0.1, 0.8, 0.2), H.HostTaa(4097, 0.1, 0.8, 0.2), H.HostTaa(16, 0.0, 0.8, 0.2), H.HostTaa(16, 1.5, 0.8, 0.2),
                H.HostTaa(16, float("nan"), 0.8, 0.2), H.HostTaa(16, 0.1, float("inf"), 0.2)):
        assert r.host.lib.awsm_host_set_taa(r.host.h, C.byref(bad)) == -1
    assert r.host.lib.awsm_host_set_taa(None, None) == -1
    calls = lib.mock_taa_calls()
    r.render()
    assert lib.mock_taa_calls() == calls                                                      # a refused record turns nothing on
    short = H.HostTaa(8, 0.25, 7.0, 7.0)                                                     # only the feedback is known: the strengths keep their defaults
    assert r.host.lib.awsm_host_set_taa(r.host.h, C.byref(short)) == 0
    assert (_bits(r.host.taa_jitter(3, False)) == _bits(tr.jitter_ndc(3, False, 64, 48))).all()
    r.render()
    assert _last_record(lib)[0].feedback == F(0.25)
    with pytest.raises(TypeError):
        r.set_taa(True, feedbak=0.5)
    # a singular camera has no inverse to reproject with: the identity goes out, and the frame starts over
    assert _last_record(lib)[0].flags == 1
    r.render()
    assert _last_record(lib)[0].flags == 0
    r.scene.proj = np.zeros((4, 4), F)
    r.update()
    r.render()
    rec, _ = _last_record(lib)
    assert rec.flags == 1 and list(rec.reproject) == list(tr.IDENTITY)
    r.close()


def test_host_over_a_backend_without_taa_reports_unsupported_and_names_the_symbol(mock):  # noqa: F811
    r = H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))
    t = H.HostTaa(16, 0.1, 0.8, 0.2)
    assert r.host.lib.awsm_host_set_taa(r.host.h, C.byref(t)) == -6                          # AWSM_ERR_UNSUPPORTED
    for on in (True, False):
        with pytest.raises(H.HostError, match=r"\(-6\).*awsm_hip_set_taa"):
            r.host.set_taa(on)
    r.render()                                                                              # and renders as before
    r.close()


# ------------------------------------------------------------------------------------------------ the records

def test_record_layouts_are_the_headers():
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    for header, name, cls, size in (("awsm_hip.h", "AwsmTaa", hip_backend.AwsmTaa, 84), ("awsm_host.h", "AwsmHostTaa", H.HostTaa, 16)):
        text = open(os.path.join(ROOT, "include", header)).read()
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        fields = re.findall(r"(uint32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
        want = [(n, ctype[t] * int(k) if k else ctype[t]) for t, n, k in fields]
        got = list(cls._fields_)
        assert [n for n, _ in want] == [n for n, _ in got]
        offset = 0
        for (n, t), (_, g) in zip(want, got):
            assert C.sizeof(t) == C.sizeof(g) and getattr(cls, n).offset == offset, n
            offset += C.sizeof(t)
        assert C.sizeof(cls) == offset == size
    text = open(os.path.join(ROOT, "include", "awsm_hip.h")).read()
    assert int(re.search(r"#define AWSM_TAA_RESET (\d+)u", text).group(1)) == hip_backend.AWSM_TAA_RESET


def test_the_library_hands_out_the_defaults():
    lib = hip_backend.load_library()      # links against the HIP runtime and loads without a GPU; a library that does not load is a failure
    t = hip_backend.AwsmTaa()
    assert lib.awsm_hip_taa_defaults(C.byref(t)) == 0 and lib.awsm_hip_taa_defaults(None) == -1
    assert t.struct_size == C.sizeof(hip_backend.AwsmTaa) and t.feedback == F(0.1) and t.flags == 0
    assert list(t.jitter_ndc) == [0.0, 0.0] and list(t.reproject) == list(tr.IDENTITY)
    with pytest.raises(TypeError):
        t.override(feedbak=1.0)
    t.override(reproject=np.arange(16), jitter_ndc=(0.5, -0.5), flags=1, feedback=0.5)
    assert list(t.reproject) == list(range(16)) and list(t.jitter_ndc) == [0.5, -0.5] and t.flags == 1 and t.feedback == 0.5


# ------------------------------------------------------------------------------------------------ properties of the restatement

def _random_image(rng, W, Hh):
    """Finite RGBA16F bits without -0: normal and subnormal magnitudes of both signs, alpha anything."""
    v = (rng.standard_normal((Hh, W, 4)) * np.exp(rng.uniform(-12, 8, (Hh, W, 4)))).astype(np.float16)
    v = np.where(np.isfinite(v), v, np.float16(1.0))
    bits = v.view(np.uint16).copy()
    bits[bits == 0x8000] = 0
    return bits


def _keys_of_depth(d):
    return (np.asarray(d, F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(7)


@pytest.mark.parametrize("W,Hh", tr.SIZES)
def test_a_still_image_under_a_still_camera_stays_as_it_is(W, Hh):
    """(a) c (1 - a) + c a is within an f32 step or two of the f16 value c and rounds back to it, at every frame and for every feedback."""
    rng = np.random.default_rng(W * 100 + Hh)
    img = _random_image(rng, W, Hh)
    keys = _keys_of_depth(rng.uniform(0.1, 0.999, (Hh, W)))
    keys[rng.uniform(size=(Hh, W)) < 0.2] = tr.NO_HIT
    for fb in (0.1, 0.5, 1.0, 0.013):
        seq = tr.Sequence()
        for frame in range(8):
            out = seq.step(img, keys, tr.record(feedback=fb))
            assert out["used"].all() == (frame > 0) and (out["used"].any() == (frame > 0))
            assert (out["resolved"] == img).all(), (fb, frame, int((out["resolved"] != img).any(axis=-1).sum()))
            assert (out["xy"][..., 0] == np.arange(W, dtype=F)[None, :]).all() and (out["xy"][..., 1] == np.arange(Hh, dtype=F)[:, None]).all()


def test_unusable_history_yields_the_current_colour():
    """(d) q.w <= 0, or a position outside the image by more than half a texel: the current texel, used = 0; on the edge of that range: used."""
    W, Hh = 33, 17
    rng = np.random.default_rng(5)
    cur, hist = _random_image(rng, W, Hh), _random_image(rng, W, Hh)
    keys = _keys_of_depth(np.full((Hh, W), 0.5))
    behind = np.diag([1.0, 1.0, 1.0, -1.0]).astype(F).reshape(-1)
    zero_w = np.diag([1.0, 1.0, 1.0, 0.0]).astype(F).reshape(-1)
    far_right = tr.IDENTITY.copy(); far_right[12] = 3.0                                      # q.x = n.x + 3: beyond the right edge everywhere
    for R in (behind, zero_w, far_right):
        out = tr.resolve(cur, keys, tr.record(R=R), hist)
        assert not out["used"].any() and (out["resolved"] == cur).all()
    half_right = tr.IDENTITY.copy(); half_right[12] = F(1.0) / F(W)                          # half a texel to the right
    out = tr.resolve(cur, keys, tr.record(R=half_right), hist)
    sx = out["xy"][..., 0]
    assert np.abs(sx - (np.arange(W) + 0.5)[None, :]).max() < 1e-3
    assert out["used"][:, :-1].all() and (out["used"] == (sx <= F(W) - F(0.5))).all()      # the last column: on the edge or just past it
    assert (out["resolved"][out["used"]][..., :3] != cur[out["used"]][..., :3]).any() and (out["resolved"][..., 3] == cur[..., 3]).all()
    out = tr.resolve(cur, keys, tr.record(R=half_right), None)                               # no history at all
    assert not out["used"].any() and (out["resolved"] == cur).all()


def test_the_history_is_clamped_to_the_neighbourhood_and_mixed():
    """One pixel by hand: history 4.0 over a current image of 1.0 with one neighbour at 2.0 -> clamped to 2.0, then 2 * 0.75 + 1 * 0.25."""
    cur = np.full((5, 5, 4), np.float16(1.0)).view(np.uint16)
    cur[1, 2, :3] = np.float16(2.0).view(np.uint16)
    cur[..., 3] = np.float16(0.5).view(np.uint16)
    hist = np.full((5, 5, 4), np.float16(4.0)).view(np.uint16)
    keys = np.full((5, 5), tr.NO_HIT, np.uint64)
    out = tr.resolve(cur, keys, tr.record(feedback=0.25), hist)
    got = out["resolved"].view(np.float16)
    assert got[2, 2, :3].tolist() == [1.75] * 3 and got[4, 0, :3].tolist() == [1.0] * 3 and got[1, 2, :3].tolist() == [2.0] * 3
    assert (out["resolved"][..., 3] == cur[..., 3]).all() and out["used"].all()
    hist[...] = np.float16(-3.0).view(np.uint16)                                              # below the neighbourhood: clamped to its least value
    assert tr.resolve(cur, keys, tr.record(feedback=0.25), hist)["resolved"].view(np.float16)[2, 2, 0] == 1.0


# (b) |f32 lookup - analytic f64 lookup| in texels: the worst f32-to-f64 distance of the restatement over the cases below measured 1.76e-5 (70x45,
# the step (-0.3, 0.1, -0.2): a position 70 texels wide, so one f32 step of q.x / q.w near 1 is 4e-6 texels, and the row sums and the division
# leave a few of them); the bar is four times that.  The analytic position also differs by the depth's and R's rounding to f32.
LOOKUP_SLACK = 4 * 1.76e-5
PLANE_STEPS = ((0.05, 0.0, 0.0), (0.0, 0.02, 0.3), (-0.3, 0.1, -0.2))


def _plane_case(W, Hh, step):
    """A camera looking at the plane z = 0 from (0.4, 0.3, 5), then translated by `step`: the analytic depth of every pixel under the current
    camera, and the analytic history position, all in f64 from the f32 matrices."""
    eye0 = np.array([0.4, 0.3, 5.0])
    eye1 = eye0 + np.array(step)
    look = np.array([0.2, -0.1, -5.0])
    prev = tr.camera_matrices(eye0, eye0 + look, W, Hh)
    view, proj = tr.camera_matrices(eye1, eye1 + look, W, Hh)
    D = np.float64
    vp = tr._mul(proj.astype(D), view.astype(D), D)
    vp_prev = tr._mul(prev[1].astype(D), prev[0].astype(D), D)
    inv = np.linalg.inv(vp.T).T                                                              # [col][row]
    py, px = np.meshgrid(np.arange(Hh), np.arange(W), indexing="ij")
    j = tr.jitter_ndc(9, True, W, Hh).astype(D)
    nx, ny = 2.0 * (px + 0.5) / W - 1.0 - j[0], 1.0 - 2.0 * (py + 0.5) / Hh - j[1]
    # the world point of the pixel on z = 0: along the ray through the unjittered NDC position
    near = [sum(inv[c][r] * v for c, v in enumerate((nx, ny, 0.0, 1.0))) for r in range(4)]
    far = [sum(inv[c][r] * v for c, v in enumerate((nx, ny, 1.0, 1.0))) for r in range(4)]
    a, b = [near[i] / near[3] for i in range(3)], [far[i] / far[3] for i in range(3)]
    t = a[2] / (a[2] - b[2])
    world = [a[i] + (b[i] - a[i]) * t for i in range(3)] + [1.0]
    clip = [sum(vp[c][r] * world[c] for c in range(4)) for r in range(4)]
    clip_prev = [sum(vp_prev[c][r] * world[c] for c in range(4)) for r in range(4)]
    depth = clip[2] / clip[3]
    assert np.abs(clip[0] / clip[3] - nx).max() < 1e-9 and (depth > 0).all() and (depth < 1).all()
    sx = px + (clip_prev[0] / clip_prev[3] - nx) * (W / 2.0)
    sy = py - (clip_prev[1] / clip_prev[3] - ny) * (Hh / 2.0)
    rec = tr.record(jitter=j.astype(F), R=tr.reproject(prev, view, proj))
    return _keys_of_depth(depth), rec, sx, sy


def test_lookup_follows_a_plane_under_a_translating_camera():
    worst32, worst = 0.0, 0.0
    for W, Hh in tr.SIZES:
        for step in PLANE_STEPS:
            keys, rec, sx, sy = _plane_case(W, Hh, step)
            x32, y32, in32 = tr.lookup(keys, rec, W, Hh, np.float32)
            x64, y64, in64 = tr.lookup(keys, rec, W, Hh, np.float64)
            d32 = max(np.abs(x32 - x64).max(), np.abs(y32 - y64).max())
            d = max(np.abs(x32 - sx).max(), np.abs(y32 - sy).max())
            print("plane %dx%d step %s: f32 to f64 %.3e, f32 to analytic %.3e texels; moved by up to %.2f texels; inside %d of %d" % (
                W, Hh, step, d32, d, max(np.abs(sx - np.arange(W)[None, :]).max(), np.abs(sy - np.arange(Hh)[:, None]).max()), in32.sum(), in32.size))
            worst32, worst = max(worst32, d32), max(worst, d)
            assert in32.sum() >= 0.5 * W * Hh and np.abs(sx - np.arange(W)[None, :]).max() > 0.1      # the history position moves, and mostly stays inside
            assert d <= LOOKUP_SLACK, (W, Hh, step, d)
    print("worst f32 to f64 distance %.3e texels (LOOKUP_SLACK = 4 x 1.76e-5), worst f32 to analytic %.3e" % (worst32, worst))
    assert worst32 <= LOOKUP_SLACK / 4 * 1.0001                                              # the figure the bar was taken from still holds


@functools.lru_cache(maxsize=None)
def _jittered_oracle_frames(W, Hh, n):
    """The CPU oracle's frames of `boxes` under a still camera whose projection is jittered as frames 1 .. n are: images (RGBA16F bits), keys, records."""
    sc = sr.boxes(W, Hh)
    view, proj = tr.camera_matrices(EYE, TARGET, W, Hh)
    lut = oracle_lib.brdf_lut(16, 16)
    model = helpers.build_model(sc)
    orc = oracle_lib.frame_from_model(model, lut)
    camera = next(a for a in orc._keep if a.ctypes.data == orc.scene.buf[BUF_CAMERA])      # the frame's copy of the camera mirror: rewritten per frame
    images, keys, recs, prev = [], [], [], None
    for fc in range(1, n + 1):
        j = tr.jitter_ndc(fc, tr.moved(prev, view, proj), W, Hh)
        camera[:512] = np.frombuffer(tr.block(view, tr.jitter_proj(proj, j), sc.camera_position, fc, W, Hh), np.uint8)
        orc.run(8)
        images.append(np.asarray(orc.rgba16f, np.uint16).reshape(Hh, W, 4).copy())
        keys.append(np.asarray(orc.keys, np.uint64).reshape(Hh, W).copy())
        recs.append(tr.record(jitter=j, R=tr.reproject(prev, view, proj)))
        prev = (view, proj)
    return images, keys, recs


def test_a_still_view_converges_on_its_silhouettes():
    """(c) 32 frames of the oracle under the jitter of frames 1 .. 32, resolved with feedback a = 0.1.  At a pixel a silhouette crosses — its key names
    one surface in some frames and another in the others — the resolve is r_k = (1 - a) r_(k-1) + a c_k from r_0 = c_0, so after
    frame 31  r = sum_k w_k c_k + (1 - a)^32 c_0  with the geometric weights w_k = a (1 - a)^(31 - k), whose sum is S = 1 - (1 - a)^32.  With
    G = sum_k w_k c_k / S, the mean of the 32 inputs under those weights, r - G = (1 - a)^32 (c_0 - G), and |c_0 - G| is at most the distance
    between the two sides' colours: |r - G| <= (1 - a)^32 |A - B|, plus the roundings to f16 (2 steps allowed).  A and B: the mean input colour
    over the frames of either side."""
    W, Hh, n, a = 64, 48, 32, 0.1
    images, keys, recs = _jittered_oracle_frames(W, Hh, n)
    seq = tr.Sequence()
    for img, k, rec in zip(images, keys, recs):
        out = seq.step(img, k, dict(rec, feedback=F(a)))
    assert out["used"].all()
    resolved = out["resolved"][..., :3].view(np.float16).astype(np.float64)
    c = np.stack([im[..., :3].view(np.float16).astype(np.float64) for im in images])          # [n, H, W, 3]
    # the two sides of a pixel: its 32 inputs split at the middle of their range; a silhouette crosses it when both sides occur and every input
    # lies within a tenth of the sides' distance of its side's mean colour (two surfaces, not a gradient)
    lum = c.sum(axis=-1)
    side = lum > 0.5 * (lum.max(axis=0) + lum.min(axis=0))[None]
    w = a * (1.0 - a) ** (n - 1 - np.arange(n))
    G = (w[:, None, None, None] * c).sum(axis=0) / w.sum()
    nA, nB = (~side).sum(axis=0)[..., None], side.sum(axis=0)[..., None]
    A = (c * ~side[..., None]).sum(axis=0) / np.maximum(nA, 1)
    B = (c * side[..., None]).sum(axis=0) / np.maximum(nB, 1)
    spread = np.abs(c - np.where(side[..., None], B[None], A[None])).max(axis=(0, 3))
    crossed = (nA[..., 0] > 0) & (nB[..., 0] > 0) & (spread <= 0.1 * np.abs(A - B).max(axis=-1))
    step16 = np.spacing(np.maximum(np.abs(resolved), np.abs(G)).astype(np.float16)).astype(np.float64)
    bound = (1.0 - a) ** n * np.abs(A - B) + 2.0 * step16
    # channels on which the two sides differ by more than the roundings could hide
    clear = crossed[..., None] & (np.abs(A - B) > 16 * step16)
    pixels = clear.any(axis=-1)
    print("silhouette pixels %d (crossed %d); worst |r - G| / bound %.3f" % (pixels.sum(), crossed.sum(), (np.abs(resolved - G) / bound)[clear].max()))
    assert pixels.sum() >= 8
    lo, hi = np.minimum(A, B), np.maximum(A, B)
    assert ((resolved > lo) & (resolved < hi))[clear].all()
    assert (np.abs(resolved - G) <= bound)[clear].all()


# ------------------------------------------------------------------------------------------------ what keeps the GPU tests informative

@pytest.mark.parametrize("W,Hh", tr.SIZES)
def test_the_orbit_step_of_the_gpu_sequence_leaves_the_image_and_lands_between_texels(W, Hh):
    """tests/test_taa_gpu.py orbits by ORBIT_DEGREES a frame, three times: on the oracle's keys each step reprojects at least four pixels out of
    the image and gives most of the others a fractional position, at every size (16x16 is what asks for as much as 10 degrees)."""
    from tests.test_taa_gpu import ORBIT_DEGREES
    sc = sr.boxes(W, Hh)
    model = helpers.build_model(sc)
    for k in (1, 2, 3):
        prev = tr.camera_matrices(tr.orbit(EYE, TARGET, ORBIT_DEGREES * (k - 1)), TARGET, W, Hh)
        view, proj = tr.camera_matrices(tr.orbit(EYE, TARGET, ORBIT_DEGREES * k), TARGET, W, Hh)
        sc.view, sc.proj = view, proj
        model.update_camera()
        orc = helpers.oracle_frame(model, oracle_lib.brdf_lut(16, 16))
        keys = np.asarray(orc.keys, np.uint64).reshape(Hh, W)
        sx, sy, inside = tr.lookup(keys, tr.record(R=tr.reproject(prev, view, proj)), W, Hh)
        fractional = inside & ((sx != np.floor(sx)) | (sy != np.floor(sy)))
        print("%dx%d step %d: %d pixels leave the image, %d land between texels" % (W, Hh, k, (~inside).sum(), fractional.sum()))
        assert (~inside).sum() >= 4 and fractional.sum() >= 0.5 * W * Hh
