"""GPU tests of the temporal anti-aliasing: the resolved image, the history positions and the used flags bit for bit against
tests/taa_reference.py fed the device's own pre-resolve image and keys and its own previous output — single-sampled and MSAA x4, under a
transparent pass, in overlap mode, through a replayed frame, on / off / reset / resize, the post chain behind it, the refusals, and the host layer."""
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.scene_desc import MaterialDesc, NodeDesc
from oracle import oracle_lib
from tests import helpers
from tests import ssao_reference as sr
from tests import taa_reference as tr

pytestmark = pytest.mark.gpu
BUF_CAMERA = 5
F = np.float32
EYE, TARGET = (3.2, 2.6, 3.6), (0.6, 0.5, 0.6)
ORBIT_DEGREES = 10.0     # per frame, about the vertical through TARGET: at 4 degrees one pixel of the 16x16 frame leaves the image, at 10 seven or more do (tests/test_taa_cpu.py, on the oracle's keys)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device(**kw):
    from awsm_renderer_amd.hip_backend import HipDevice
    return HipDevice(parity_tap=True, **kw)


def _error():
    from awsm_renderer_amd.hip_backend import AwsmHipError
    return AwsmHipError


def _setup(dev, model, lut, msaa=0):
    """helpers.hip_frame's uploads without its frame."""
    sc = model.scene
    dev.resize(sc.width, sc.height, msaa)
    dev.upload_mirrors(model.mirrors())
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    return dev


class _Driver:
    """Frames through the C-ABI as the host layer would send them: the camera orbited by `k` steps, its projection jittered by the rule of the frame
    count, the record composed from the last frame's unjittered matrices."""

    def __init__(self, dev, model, transparent=False, feedback=tr.DEFAULT_FEEDBACK, eye=EYE, target=TARGET, dof=(0.0, 0.0), draws=None, fovy_deg=50.0):
        self.dev, self.model, self.transparent, self.feedback, self.eye, self.target, self.dof, self.fovy = dev, model, transparent, feedback, eye, target, dof, fovy_deg
        self.W, self.H = model.scene.width, model.scene.height
        self.draws = model.collect_draws() if draws is None else draws
        self.tr_draws = model.collect_transparent_draws() if transparent else None
        self.restart()

    def restart(self):
        self.fc, self.prev = 0, None

    def frame(self, k=0, post=None, end=True, taa=True, flags=0, draws=None):
        """-> (the record, the camera block).  taa: hand the record over (False: leave the context's TAA state as it is)."""
        dev = self.dev
        eye = tr.orbit(self.eye, self.target, ORBIT_DEGREES * k)
        view, proj = tr.camera_matrices(eye, self.target, self.W, self.H, fovy_deg=self.fovy)
        self.fc += 1
        j = tr.jitter_ndc(self.fc, tr.moved(self.prev, view, proj), self.W, self.H)
        rec = tr.record(self.feedback, j, tr.reproject(self.prev, view, proj))
        block = tr.block(view, tr.jitter_proj(proj, j), eye, self.fc, self.W, self.H, self.dof)
        dev.buffer_write(BUF_CAMERA, 0, np.frombuffer(block, np.uint8))
        dev.geometry_pass(self.draws if draws is None else draws)
        dev.opaque_pass()
        if self.transparent:
            dev.transparent_pass(self.tr_draws)
        if taa:
            dev.set_taa(feedback=rec["feedback"], jitter_ndc=rec["jitter_ndc"], reproject=rec["reproject"], flags=flags)
        dev.post_pass(**(post or {}))
        self.stats = dev.frame_end() if end else None
        self.prev = (view, proj)
        return rec, block

    def source(self):
        """What the post pass took as the current image."""
        return self.dev.read_composite() if self.transparent else self.dev.read_opaque()


def _assert_resolve(drv, seq, rec, what=""):
    """The device's resolve of the last frame against the restatement's step from the device's own inputs -> the restatement's dict."""
    dev = drv.dev
    want = seq.step(drv.source(), dev.read_visibility(), rec)
    resolved, xy, used = dev.read_taa()
    assert (used == want["used"]).all(), "%s: used differs at %d pixels" % (what, int((used != want["used"]).sum()))
    bad = (_bits(xy) != _bits(want["xy"])).any(axis=-1)
    at = tuple(np.argwhere(bad)[0]) if bad.any() else None
    assert not bad.any(), "%s: the lookup position differs at %d pixels, first %s: device %r, restatement %r" % (what, int(bad.sum()), at, xy[at], want["xy"][at])
    bad = (resolved != want["resolved"]).any(axis=-1)
    at = tuple(np.argwhere(bad)[0]) if bad.any() else None
    assert not bad.any(), "%s: %d resolved pixels differ, first %s: device %s, restatement %s (used %s, position %s)" % (
        what, int(bad.sum()), at, resolved[at], want["resolved"][at], want["used"][at], want["xy"][at])
    return want


# ------------------------------------------------------------------------------------------------ the resolve, bit for bit

@pytest.mark.parametrize("msaa", [0, 4])
@pytest.mark.parametrize("W,H", tr.SIZES)
def test_six_frames_are_the_f32_restatement_bit_for_bit(W, H, msaa, oracle_lut):
    """Three still frames under three jitters, then three orbit steps.  Frame 0 is its input.  Among the frames after it there are pixels whose
    history is not used — every orbit frame has some; a still frame has none, its lookup is the pixel itself by construction — and pixels whose
    position lies between texels.  70x45: ragged tiles on both axes; 16x16: one tile, every apron texel a clamp; 33x70: taller than wide."""
    model = helpers.build_model(sr.boxes(W, H))
    dev = _setup(_device(), model, oracle_lut, msaa)
    drv, seq = _Driver(dev, model), tr.Sequence()
    unused = fractional = 0
    for i, k in enumerate((0, 0, 0, 1, 2, 3)):
        rec, _ = drv.frame(k)
        want = _assert_resolve(drv, seq, rec, "%dx%d msaa %d frame %d" % (W, H, msaa, i))
        src = drv.source()
        if i == 0:
            assert not want["used"].any() and (want["resolved"] == src).all()
        else:
            frac = want["used"] & ((want["xy"][..., 0] != np.floor(want["xy"][..., 0])) | (want["xy"][..., 1] != np.floor(want["xy"][..., 1])))
            if k == 0:
                assert want["used"].all() and not frac.any()
                assert (want["resolved"] != src).any(axis=-1).sum() >= 0.02 * W * H           # the jitter moved the silhouettes: the history counts
            else:
                assert (~want["used"]).sum() >= 4 and frac.sum() >= 0.5 * W * H, (i, int((~want["used"]).sum()), int(frac.sum()))
            unused += int((~want["used"]).sum()); fractional += int(frac.sum())
        if msaa:
            keys = dev.read_visibility()
            assert keys.shape == (H, W, 4)
    assert unused > 0 and fractional > 0
    dev.close()


def test_msaa_depth_is_the_least_of_the_four_samples(oracle_lut):
    """At 70x45 under MSAA x4 the orbit frames have pixels whose sample 0 is not the nearest, or hit nothing while another sample did: the history
    position there follows the least depth, which test_six_frames holds to the restatement; here: such pixels exist and the rule matters."""
    W, H = 70, 45
    model = helpers.build_model(sr.boxes(W, H))
    dev = _setup(_device(), model, oracle_lut, 4)
    drv, seq = _Driver(dev, model), tr.Sequence()
    for k in (0, 1):
        rec, _ = drv.frame(k)
        want = _assert_resolve(drv, seq, rec, "msaa frame %d" % k)
    keys = dev.read_visibility()
    first = tr.lookup(keys[..., 0], rec, W, H)
    differs = (_bits(first[0]) != _bits(want["xy"][..., 0])) | (_bits(first[1]) != _bits(want["xy"][..., 1]))
    assert differs.sum() >= 10, int(differs.sum())
    dev.close()


# ------------------------------------------------------------------------------------------------ what stands behind and in front of the resolve

def test_the_post_chain_reads_the_resolved_image(oracle_lut):
    """Display-only, and SMAA + bloom + DoF together: the effects and display images are tests/post_oracle.py's of the RESOLVED image, within that
    module's own bars (tests/test_post_gpu.py's checker, as it is)."""
    from tests import post_oracle
    from tests.test_post_gpu import _check, _depth
    W, H = 70, 45
    sc = sr.boxes(W, H)
    model = helpers.build_model(sc)
    dev = _setup(_device(), model, oracle_lut)
    drv, seq = _Driver(dev, model, dof=(3.0, 0.7)), tr.Sequence()
    for k in (0, 0, 1):
        rec, block = drv.frame(k)
        want = _assert_resolve(drv, seq, rec)
    resolved, src = want["resolved"], drv.source()
    assert (resolved != src).any(axis=-1).sum() >= 0.1 * W * H
    cam = np.frombuffer(block, np.float32).copy()
    # the same frame's post pass once more per case (the resolve too: same history, same image)
    _, disp = _check("taa display-only", dev, cam, None, resolved, tonemap=1)
    assert (dev.read_taa(layers=False) == resolved).all()
    not_it = post_oracle.display(post_oracle.effects(src)[0], 1)
    assert (np.abs(disp.astype(np.int16) - not_it.astype(np.int16)) > 1).any(axis=-1).sum() >= 20      # the unresolved image would show
    _check("taa smaa+bloom+dof", dev, cam, _depth(dev, sc, 0), resolved, tonemap=1, smaa=True, bloom=True, dof=True)
    assert (dev.read_taa(layers=False) == resolved).all()
    dev.close()


def _glass_scene(W, H):
    """`boxes` with a transmissive quad standing in front of them."""
    sc = sr.boxes(W, H)
    sc.materials.append(MaterialDesc(base_color_factor=(0.95, 0.98, 1.0, 1.0), transmission={"factor": 0.95}, metallic_factor=0.0, roughness_factor=0.1))
    quad = dataclasses.replace(sr._quad((0.15, 0.05, 1.2), (1.05, 0.0, -1.05), (0.0, 1.8, 0.0), 0), material=len(sc.materials) - 1)
    sc.nodes.append(NodeDesc(primitives=[quad]))
    return sc


def test_a_frame_with_a_transparent_pass_resolves_the_composite(oracle_lut):
    W, H = 70, 45
    model = helpers.build_model(_glass_scene(W, H))
    model.collect_draws()
    assert len(model.collect_transparent_draws()) == 1
    dev = _setup(_device(), model, oracle_lut)
    drv, seq, other = _Driver(dev, model, transparent=True), tr.Sequence(), tr.Sequence()
    for i, k in enumerate((0, 0, 1)):
        rec, _ = drv.frame(k)
        want = _assert_resolve(drv, seq, rec, "glass frame %d" % i)
        opaque, keys = dev.read_opaque(), dev.read_visibility()
        from_opaque = other.step(opaque, keys, rec)                                           # what a resolve of the opaque image would give
        touched = (drv.source() != opaque).any(axis=-1)
        assert 150 <= touched.sum() <= 0.5 * W * H
        assert (want["resolved"] != from_opaque["resolved"]).any(axis=-1)[touched].mean() > 0.9
    dev.close()


@pytest.mark.parametrize("W,H", [(70, 45), (1920, 1080)])
def test_each_overlapped_frame_is_its_synchronous_twin(W, H, oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES, eight frames of an orbiting camera, enqueue-only: frame i's resolve runs on slot i % 2's stream, reads what frame
    i - 1's wrote on the other stream and overwrites what frame i - 1's read.  read_taa synchronises, so frame i is read after the frames 0 .. i
    were enqueued with nothing between them, and the next round starts over under AWSM_TAA_RESET: 36 frames in all.  1920x1080: the resolve
    takes tens of microseconds, longer than this scene's geometry pass; the small size is the one the restatement runs at."""
    small = W * H < 10000
    model = helpers.build_model(sr.boxes(W, H))
    dev = _setup(_device(), model, oracle_lut)
    drv, seq, want = _Driver(dev, model), tr.Sequence(), []
    for i in range(8):
        rec, _ = drv.frame(i)
        if small:
            _assert_resolve(drv, seq, rec, "synchronous frame %d" % i)
        want.append(dev.read_taa(layers=False))
    dev.close()
    assert all((want[i] != want[i + 1]).any(axis=-1).sum() >= 0.1 * W * H for i in range(7))
    dev = _setup(_device(overlap_frames=True), model, oracle_lut)
    drv = _Driver(dev, model)
    for last in range(8):
        drv.restart()
        for i in range(last + 1):                                                            # no frame_end, no read-back between the frames
            drv.frame(i, end=False, flags=1 if i == 0 else 0)
        got = dev.read_taa(layers=False)
        assert (got == want[last]).all(), (last, int((got != want[last]).any(axis=-1).sum()))
    dev.frame_end()
    dev.close()


def test_a_replayed_frame_is_resolved_once(oracle_lut):
    """AWSM_CFG_SMALL_BIN_LIST: frame 1 draws a few meshes and fits its (triangle, tile) list; frame 2 draws them all, overflows, and frame_end
    replays the geometry and opaque passes and the post pass.  The replayed resolve reads the history frame 1 wrote — not what the first attempt
    of frame 2 wrote — into the same image: it is the restatement's single resolve, and frame 3's history is that image."""
    sc = scenes.atrium_scene(320, 180, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    dev = _setup(_device(small_bin_list=True), model, oracle_lut)
    f = np.frombuffer(bytes(model.camera_bytes), np.float32)
    eye = tuple(float(v) for v in f[96:99])
    inv_view = f[80:96].reshape(4, 4)
    target = tuple(float(v) for v in (np.asarray(eye) - 5.0 * inv_view[2][:3]))              # five units down the view axis
    draws = model.collect_draws()
    drv, seq = _Driver(dev, model, eye=eye, target=target, draws=draws, fovy_deg=60.0), tr.Sequence()
    rec, _ = drv.frame(0, draws=draws[:2])
    assert drv.stats["bin_overflow_retries"] == 0, drv.stats
    _assert_resolve(drv, seq, rec, "frame 1")
    rec, _ = drv.frame(1)
    assert drv.stats["bin_overflow_retries"] >= 1, drv.stats
    want = _assert_resolve(drv, seq, rec, "the replayed frame")
    assert want["used"].sum() >= 0.5 * sc.width * sc.height and (want["resolved"] != drv.source()).any(axis=-1).sum() >= 0.1 * sc.width * sc.height
    retries = drv.stats["bin_overflow_retries"]
    rec, _ = drv.frame(1)
    assert drv.stats["bin_overflow_retries"] == retries
    want = _assert_resolve(drv, seq, rec, "the frame after it")
    assert want["used"].all()
    dev.close()


def test_on_then_off_then_on_and_the_resets(oracle_lut):
    W, H = 33, 70
    model = helpers.build_model(sr.boxes(W, H))
    never = _setup(_device(), model, oracle_lut)
    dev = _setup(_device(), model, oracle_lut)
    drv_never, drv, seq = _Driver(never, model), _Driver(dev, model), tr.Sequence()

    def both(k, **kw):
        drv_never.frame(k, taa=False)
        return drv.frame(k, **kw)

    def starts_over(what):
        want = _assert_resolve(drv, seq, rec, what)
        assert not want["used"].any() and (want["resolved"] == drv.source()).all(), what

    def goes_on(what):
        want = _assert_resolve(drv, seq, rec, what)
        assert want["used"].all() and (want["resolved"] != drv.source()).any(), what

    for k in (0, 0):
        rec, _ = both(k)
        _assert_resolve(drv, seq, rec)
    assert (dev.read_display() != never.read_display()).any()
    dev.set_taa(None)
    both(0, taa=False)
    assert (dev.read_display() == never.read_display()).all() and (dev.read_opaque() == never.read_opaque()).all()
    with pytest.raises(_error()) as e:
        dev.read_taa()
    assert e.value.code == -5
    seq.reset()
    rec, _ = both(0); starts_over("on again")
    rec, _ = both(0); goes_on("the frame after")
    dev.resize(W, H, 0); never.resize(W, H, 0)
    seq.reset()
    rec, _ = both(0); starts_over("after resize")
    rec, _ = both(0); goes_on("the frame after the resize")
    seq.reset()
    rec, _ = both(0, flags=1); starts_over("AWSM_TAA_RESET")
    rec, _ = both(0); goes_on("the reset applied to one pass")
    dev.resize(W, H, 4)                                                                       # a new MSAA mode drops it as well
    seq.reset()
    rec, _ = drv.frame(0); starts_over("after the change of MSAA mode")
    dev.close(); never.close()


def test_refusals(oracle_lut):
    W, H = 16, 16
    model = helpers.build_model(sr.boxes(W, H))
    dev = _setup(_device(), model, oracle_lut)
    drv, seq = _Driver(dev, model, feedback=0.3), tr.Sequence()
    with pytest.raises(_error()) as e:                                                # nothing resolved yet
        dev.read_taa()
    assert e.value.code == -5                                                                # AWSM_ERR_NOT_READY
    dev.set_taa(feedback=0.3)
    with pytest.raises(_error()) as e:                                                # set, but no post pass since
        dev.read_taa()
    assert e.value.code == -5
    rec, _ = drv.frame(0)
    _assert_resolve(drv, seq, rec)
    nan_matrix, inf_matrix = tr.IDENTITY.copy(), tr.IDENTITY.copy()
    nan_matrix[7], inf_matrix[12] = np.nan, np.inf
    for bad in (dict(struct_size=0), dict(struct_size=3), dict(struct_size=4097), dict(feedback=0.0), dict(feedback=1.5), dict(feedback=-0.1),
                dict(feedback=float("nan")), dict(reproject=nan_matrix), dict(reproject=inf_matrix), dict(jitter_ndc=(float("inf"), 0.0)), dict(flags=2), dict(flags=0x80000001)):
        with pytest.raises(_error()) as e:
            dev.set_taa(**bad)
        assert e.value.code == -1, bad                                                       # AWSM_ERR_INVALID_ARGUMENT
    rec, _ = drv.frame(0, taa=False)                                                         # a refused record changes nothing: feedback 0.3, identity, the old jitter
    want = _assert_resolve(drv, seq, dict(rec, jitter_ndc=tr.jitter_ndc(1, True, W, H)), "after the refusals")
    assert want["used"].all()
    dev.set_taa(struct_size=8, feedback=0.5, jitter_ndc=(0.25, 0.25), reproject=inf_matrix)   # only the feedback is known: the rest keeps its defaults
    rec, _ = drv.frame(0, taa=False)
    _assert_resolve(drv, seq, tr.record(feedback=0.5), "a record of eight bytes")
    dev.set_taa(feedback=1.0)                                                                # the upper end is allowed: the current image, clamped history or not
    rec, _ = drv.frame(0, taa=False)
    want = _assert_resolve(drv, seq, tr.record(feedback=1.0))
    assert (want["resolved"] == drv.source()).all()
    dev.close()


# ------------------------------------------------------------------------------------------------ through the host

def test_taa_through_the_host_layer(oracle_lut):
    """Host.set_post_processing(); Host.set_taa(); five renders of a still scene: the camera block on the device is the restated jittered one, the
    resolve is the restatement's with the record the host composed (jitter of the frame count, identity), and a resize starts over."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    W, H = 70, 45
    sc = sr.boxes(W, H)
    view, proj = tr.camera_matrices(EYE, TARGET, W, H)
    sc.view, sc.proj, sc.camera_position = view, proj, tuple(float(F(v)) for v in EYE)
    r = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut))
    dev = HipDevice.from_ctx(r.host.device_ctx, W, H)
    dev.msaa = 0
    r.set_post_processing(1)
    r.set_taa()
    seq, prev, fc = tr.Sequence(), None, 0

    def frame(what):
        nonlocal prev, fc
        r.render(sync=True)
        fc += 1
        j = tr.jitter_ndc(fc, tr.moved(prev, view, proj), W, H)
        assert dev.buffer_read(BUF_CAMERA, 0, 512) == tr.block(view, tr.jitter_proj(proj, j), sc.camera_position, fc, W, H), what
        want = seq.step(dev.read_opaque(), dev.read_visibility(), tr.record(jitter=j, R=tr.reproject(prev, view, proj)))
        resolved, xy, used = dev.read_taa()
        assert (resolved == want["resolved"]).all() and (used == want["used"]).all() and (_bits(xy) == _bits(want["xy"])).all(), what
        prev = (view, proj)
        return want, dev.read_opaque()

    for i in range(5):
        want, src = frame("render %d" % i)
        assert want["used"].all() == (i > 0)
    assert (want["resolved"] != src).any(axis=-1).sum() >= 0.02 * W * H
    r.host.resize(W, H)
    seq.reset()
    want, src = frame("after resize")
    assert not want["used"].any() and (want["resolved"] == src).all()
    want, _ = frame("the frame after the resize")
    assert want["used"].all()
    r.set_taa(False)
    r.render(sync=True)
    assert dev.buffer_read(BUF_CAMERA, 0, 512) == tr.block(view, proj, sc.camera_position, 0, W, H)      # the block awsm_host_camera_update packed
    with pytest.raises(_error()):
        dev.read_taa()
    r.close()
