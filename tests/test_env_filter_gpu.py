"""awsm_hip_env_cube_filter on the device against the f64 numpy restatement (tests/ibl_filter_reference.py).

The bar, per component: |device - reference| <= half an f16 ulp of the reference's binade + 2^-16 |reference|.  The first term is the one rounding
of the store; the second is the budget for the f32 frame, sampling and sums (about ten times the ~1e-6 estimated for them;
tests/test_env_filter_cpu.py shows the restatement run in f32 spends under a quarter of it).  Level 0 at equal sides and the constant source are
held to exact bits.  Rendered frames after Host.env_bake_ibl are compared bit for bit with a fresh context that received the read-back chains, and
with the oracle given those chains."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from awsm_renderer_amd.hip_backend import AwsmEnvFilter, AwsmHipError, HipDevice
from tests import helpers
from tests import ibl_filter_reference as R
from tests.test_env_filter_cpu import CONSTANT, GGX_CASES, LAMBERT_CASES, constant_expectations, source_chain

pytestmark = pytest.mark.gpu

INVALID, NOT_READY = -1, -5
HALF_ONE = 0x3C00
RGB_TOL = 1e-4                                           # the suite's bar for a frame against the oracle (tests/test_gpu_parity.py)
SKY, PRE, IRR = 0, 1, 2


@pytest.fixture(scope="module")
def dev():
    d = HipDevice(parity_tap=True)
    yield d
    d.close()


@pytest.fixture(scope="module")
def chains():
    return {n: source_chain(n) for n in (16, 12)}


def read_chain(device, which):
    size, mips = device.env_cube_info(which)
    return [device.env_cube_read_level(which, l) for l in range(mips)]


def excess(got_f16, ref):
    """How far over the bar the worst component is, in units of the bar's slack term (<= 0: inside), and the largest error in f16 ulps."""
    err = np.abs(got_f16[..., :3].astype(np.float64) - ref)
    ulp = R.f16_ulp(ref)
    over = (err - 0.5 * ulp) / (2.0 ** -16 * np.abs(ref))
    return float(over.max()), float((err / ulp).max())


def assert_alpha_one(levels):
    for lv in levels:
        assert (lv.view(np.uint16)[..., 3] == HALF_ONE).all()


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("ns,size,mips,samples", GGX_CASES)
def test_prefiltered_chain_against_the_restatement(dev, chains, ns, size, mips, samples):
    """16^2 -> 16^2 x 5 with 64 and 256 samples (one and four per lane); 16^2 -> 8^2 x 4 (level 0 resampled); 12^2 -> 12^2 x 4 (sides 12 6 3 1)."""
    src = chains[ns]
    dev.env_cube_upload(SKY, src)
    dev.env_cube_filter(SKY, PRE, "ggx", size, mips, samples)
    assert dev.env_cube_info(PRE) == (size, mips)
    got = read_chain(dev, PRE)
    want = R.prefiltered(src, size, mips, samples)
    assert [g.shape[1] for g in got] == [max(size >> l, 1) for l in range(mips)]
    assert_alpha_one(got)
    if size == ns:                                        # the source's RGB bits
        assert (got[0].view(np.uint16)[..., :3] == src[0].view(np.uint16)[..., :3]).all()
    for l, (g, w) in enumerate(zip(got, want)):
        over, ulps = excess(g, w)
        print("ggx %d -> %d x %d, S %d, level %d: worst excess %.3f of the slack, largest error %.3f ulp" % (ns, size, mips, samples, l, over, ulps))
        assert over <= 0.0, (l, over, ulps)
    for a, b in zip(read_chain(dev, SKY), src):           # the source is not modified
        assert (a.view(np.uint16) == b.view(np.uint16)).all()
    # a second bake of the same input: the same bits
    dev.env_cube_filter(SKY, PRE, "ggx", size, mips, samples)
    for a, b in zip(read_chain(dev, PRE), got):
        assert (a.view(np.uint16) == b.view(np.uint16)).all()


@pytest.mark.parametrize("ns,size,samples", LAMBERT_CASES)
def test_irradiance_against_the_restatement(dev, chains, ns, size, samples):
    src = chains[ns]
    dev.env_cube_upload(SKY, src)
    dev.env_cube_filter(SKY, IRR, "lambert", size, 1, samples)
    assert dev.env_cube_info(IRR) == (size, 1)
    got = read_chain(dev, IRR)
    assert_alpha_one(got)
    over, ulps = excess(got[0], R.irradiance(src, size, samples))
    print("lambert %d -> %d, S %d: worst excess %.3f of the slack, largest error %.3f ulp" % (ns, size, samples, over, ulps))
    assert over <= 0.0, (over, ulps)
    dev.env_cube_filter(SKY, IRR, "lambert", size, 1, samples)
    assert (read_chain(dev, IRR)[0].view(np.uint16) == got[0].view(np.uint16)).all()


def test_a_constant_source_gives_the_exact_bits(dev):
    chain, pre, irr = constant_expectations()
    dev.env_cube_upload(SKY, chain)
    dev.env_cube_filter(SKY, PRE, "ggx", 8, 4, 64)
    dev.env_cube_filter(SKY, IRR, "lambert", 4, 1, 64)
    c16 = np.array(CONSTANT, dtype=np.float16).view(np.uint16)
    for lv in read_chain(dev, PRE):
        assert (lv.view(np.uint16)[..., :3] == c16).all() and (lv.view(np.uint16)[..., 3] == HALF_ONE).all()
    want = irr.astype(np.float16).view(np.uint16)
    got = read_chain(dev, IRR)[0].view(np.uint16)
    assert (got[..., :3] == want).all() and (got[..., 3] == HALF_ONE).all()


def test_the_default_sample_count_is_1024(dev, chains):
    dev.env_cube_upload(SKY, chains[16])
    dev.env_cube_filter(SKY, IRR, "lambert", 2, 1, 0)
    a = read_chain(dev, IRR)[0].view(np.uint16).copy()
    dev.env_cube_filter(SKY, IRR, "lambert", 2, 1, 1024)
    assert (read_chain(dev, IRR)[0].view(np.uint16) == a).all()
    over, _ = excess(a.view(np.float16), R.irradiance(chains[16], 2, 1024))
    assert over <= 0.0, over


# ------------------------------------------------------------------------------------------------ error codes

def _filter(device, src, dst, kind=0, size=8, mips=1, samples=64, struct_size=None):
    f = AwsmEnvFilter(C.sizeof(AwsmEnvFilter) if struct_size is None else struct_size, kind, size, mips, samples, 0)
    rc = device.lib.awsm_hip_env_cube_filter(device.ctx, src, dst, C.byref(f))
    return rc, (device.lib.awsm_hip_last_error(device.ctx) or b"").decode()


def test_error_codes(chains):
    assert C.sizeof(AwsmEnvFilter) == 24
    d = HipDevice(parity_tap=True)
    rc, text = _filter(d, SKY, PRE)
    assert rc == NOT_READY and "uniform colour" in text, (rc, text)
    d.env_cube_upload(SKY, chains[16])
    before = [lv.view(np.uint16).copy() for lv in read_chain(d, SKY)]
    for kw in (dict(src=SKY, dst=SKY), dict(src=SKY, dst=3), dict(src=-1, dst=PRE), dict(src=SKY, dst=PRE, samples=48), dict(src=SKY, dst=PRE, samples=8),
               dict(src=SKY, dst=PRE, samples=8192), dict(src=SKY, dst=PRE, size=0), dict(src=SKY, dst=PRE, size=8193), dict(src=SKY, dst=PRE, mips=0),
               dict(src=SKY, dst=PRE, size=8, mips=5), dict(src=SKY, dst=IRR, kind=1, mips=2), dict(src=SKY, dst=PRE, kind=2), dict(src=SKY, dst=PRE, struct_size=20)):
        rc, text = _filter(d, **kw)
        assert rc == INVALID and text, (kw, rc, text)
    with pytest.raises(AwsmHipError) as e:                # nothing was created along the way
        d.env_cube_info(PRE)
    assert e.value.code == NOT_READY
    rc, text = _filter(d, PRE, IRR, kind=1)               # a source that is still a colour, whatever the skybox holds
    assert rc == NOT_READY
    rc, text = _filter(d, SKY, PRE, size=8, mips=4)       # the accepted neighbour: the full chain of 8
    assert rc == 0, text
    assert d.env_cube_info(PRE) == (8, 4)
    for a, b in zip(read_chain(d, SKY), before):
        assert (a.view(np.uint16) == b).all()
    d.close()


# ------------------------------------------------------------------------------------------------ frames

def test_frames_lit_by_the_baked_cubes(oracle_lut, chains):
    """helmet_scene at 160 x 90: after Host.env_bake_ibl the frame equals, bit for bit, the frame of a fresh context that received the read-back
    chains through awsm_host_env_cube + awsm_host_set_ibl_mip_counts, and that frame meets the suite's bar against the oracle given those chains."""
    sc = scenes.helmet_scene(160, 90, segments=32, rings=24, tex_size=32)
    sc = dataclasses.replace(sc, env_cubes={"skybox": chains[16]})
    r, d, _ = helpers.host_frame(sc, oracle_lut)
    flat = d.read_opaque().copy()
    r.host.env_bake_ibl(16, 5, 8, 64)
    r.render(sync=True)
    got = d.read_opaque().copy()
    pre, irr = read_chain(d, PRE), read_chain(d, IRR)
    r.close()
    assert [lv.shape[1] for lv in pre] == [16, 8, 4, 2, 1] and [lv.shape[1] for lv in irr] == [8]
    assert (got != flat).any()

    sc2 = dataclasses.replace(sc, env_cubes={"skybox": chains[16], "prefiltered": pre, "irradiance": irr}, prefiltered_mip_count=5, irradiance_mip_count=1)
    r2, d2, _ = helpers.host_frame(sc2, oracle_lut)
    want = d2.read_opaque().copy()
    assert (got == want).all(), int((got != want).any(axis=-1).sum())
    orc = helpers.oracle_frame(helpers.build_model(sc2), oracle_lut)
    res = helpers.compare_frames(orc, d2, rgb_tol=RGB_TOL)
    r2.close()
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["alpha_mismatch"] == 0 and res["f16_max_ulp"] <= 2, res
