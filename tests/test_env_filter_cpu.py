"""awsm_hip_env_cube_filter, the parts that need no GPU: the numpy restatement (tests/ibl_filter_reference.py) against the
oracle's cube sampler and against known answers, the C++ table builder against the restatement's tables bit for bit (a program of its own under
AddressSanitizer + UndefinedBehaviorSanitizer), the f32 pass of the restatement against its f64 pass, and the host over a backend without the symbol."""
import math
import os
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from oracle import oracle_lib
from tests import ibl_filter_reference as R
from tests.test_host_layer_cpu import MOCK, mock  # noqa: F401  (the module-scoped fixture builds the mock backend)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -6

# the device test's cases: (source side, destination side, levels, samples) and (source side, irradiance side, samples)
GGX_CASES = [(16, 16, 5, 64), (16, 16, 5, 256), (16, 8, 4, 128), (12, 12, 4, 128)]
LAMBERT_CASES = [(16, 8, 256), (16, 1, 256)]


def source_chain(n):
    return R.mip_chain(R.smooth_hdr_source(n), int(n).bit_length())


# ------------------------------------------------------------------------------------------------ the sampler

@pytest.mark.parametrize("size", [16, 12, 1])
def test_the_restated_sampler_is_the_oracles(size):
    """Random directions and lods — below 0 and past the chain among them — plus directions on the seams and towards the corners.  The oracle works
    in f32: the two agree to f32 rounding of values up to 10 (the sampler is continuous in the direction, so a tap that flips sides moves nothing)."""
    rng = np.random.default_rng(size)
    mips = int(size).bit_length()
    chain = [rng.uniform(0.0, 10.0, size=(6, max(size >> l, 1), max(size >> l, 1), 4)).astype(np.float16) for l in range(mips)]
    d = rng.standard_normal((4000, 3))
    d[:300, 0] = d[:300, 1]                                    # on an x = y seam
    d[300:600] = np.sign(d[300:600]) * (1.0 + 1e-3 * rng.standard_normal((300, 3)))      # near the corners
    d[600:700, 2] = 0.0
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    lods = rng.uniform(-1.0, mips + 0.5, size=4000).astype(np.float32)
    lods[::7] = np.floor(lods[::7])
    want = oracle_lib.sample_cube(chain, d, lods).astype(np.float64)
    got = R.sample_cube(chain, d.astype(np.float64), lods.astype(np.float64))
    corner = (np.abs(np.abs(d) - np.abs(d).max(axis=1, keepdims=True)) < 5e-3).all(axis=1)      # the one place the contract is not continuous
    err = np.abs(got - want)
    assert err[~corner].max() <= 2e-5, err[~corner].max()
    assert (~corner).sum() > 3500
    got32 = R.sample_cube(chain, d, lods, np.float32)
    assert np.abs(got32.astype(np.float64) - want)[~corner].max() <= 2e-5


# ------------------------------------------------------------------------------------------------ the tables

TABLE_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "env_filter_table.hpp"

// argv: groups of five numbers (kind level levels samples source side); prints each table as "T <count>" and one line of five hex words per entry
int main(int argc, char** argv) {
    for (int k = 1; k + 4 < argc; k += 5) {
        const std::vector<awsm::EnvFilterEntry> t = awsm::env_filter_table((uint32_t)atoi(argv[k]), (uint32_t)atoi(argv[k + 1]), (uint32_t)atoi(argv[k + 2]),
                                                                           (uint32_t)atoi(argv[k + 3]), (uint32_t)atoi(argv[k + 4]));
        printf("T %zu\n", t.size());
        for (const awsm::EnvFilterEntry& e : t) {
            uint32_t w[5];
            memcpy(w, &e, sizeof w);
            printf("%08x %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3], w[4]);
        }
    }
    return 0;
}
"""


def test_the_cpp_tables_are_the_restated_ones_bit_for_bit_under_asan_and_ubsan(tmp_path):
    src, exe = tmp_path / "env_filter_table_main.cpp", tmp_path / "env_filter_table_main"
    src.write_text(TABLE_MAIN)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "awsm-renderer_amd", "csrc"), "-o", str(exe), str(src)])
    cases = [(R.GGX, 1, 5, 64, 16), (R.GGX, 4, 5, 64, 16), (R.GGX, 2, 5, 256, 16), (R.GGX, 3, 4, 128, 12), (R.GGX, 1, 14, 4096, 8192), (R.GGX, 1, 2, 16, 1),
             (R.GGX, 7, 9, 1024, 256), (R.LAMBERT, 0, 1, 256, 16), (R.LAMBERT, 0, 1, 1024, 256), (R.LAMBERT, 0, 1, 16, 1)]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    lines = p.stdout.split("\n")
    at = 0
    for case in cases:
        want = R.table(*case)
        assert lines[at] == "T %d" % len(want), (case, lines[at], len(want))
        got = np.array([[int(w, 16) for w in lines[at + 1 + i].split()] for i in range(len(want))], dtype=np.uint32).reshape(-1, 5)
        assert (got == want.view(np.uint32)).all(), (case, int((got != want.view(np.uint32)).sum()))
        at += 1 + len(want)
    # what the tables must look like whatever built them
    t = R.table(R.GGX, 4, 5, 64, 16)                            # roughness 1: N.L = 1 - 2 xi.y, so half the points are dropped (xi.y = 1/2 sits on the edge)
    assert len(t) in (32, 33) and (t[:, 3] > 0).all()
    assert len(R.table(R.GGX, 1, 5, 64, 16)) == 64 and len(R.table(R.LAMBERT, 0, 1, 256, 16)) == 256
    assert np.abs(np.linalg.norm(R.table(R.LAMBERT, 0, 1, 256, 16)[:, :3].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert (R.table(R.LAMBERT, 0, 1, 256, 16)[:, 4] >= 0).all()


# ------------------------------------------------------------------------------------------------ known answers

def test_irradiance_of_a_linear_source():
    """L = a + b w.y has irradiance pi (a + 2/3 b n.y).  The source is a 32^2 cube of f64 texels with its 2x2 chain; 1024 Hammersley points.
    Observed on the CPU: the largest error over all texels of an 8^2 cube is 9.14e-3 (2.9e-3 of pi a), on the +-Y faces, where the gradient runs
    along n.  It is the quadrature error: it falls as 1 / S (3.4e-2 with 256 points, 2.1e-3 with 4096) and does not move with the source's side
    (9.4e-3 from a 64^2 source).  Twice the observed figure is asserted."""
    a, b = 1.0, 0.75
    lv = a + b * R.texel_dirs(32)[..., 1:2]
    chain = [np.repeat(lv, 4, axis=-1)]
    while chain[-1].shape[1] > 1:
        s = chain[-1]
        chain.append(0.25 * (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]))
    got = R.irradiance(chain, 8, 1024)
    want = math.pi * (a + (2.0 / 3.0) * b * R.texel_dirs(8)[..., 1])
    err = np.abs(got - want[..., None]).max()
    print("irradiance of a linear source: largest error", err)
    assert err <= 2.0 * 9.14e-3, err


CONSTANT = (0.75, 0.375, 1.5)


def constant_expectations():
    """(prefiltered levels, irradiance) of the constant source in f64, checked to lie clear of every f16 rounding midpoint."""
    src = np.ones((6, 8, 8, 4), dtype=np.float16)
    src[..., :3] = np.array(CONSTANT, dtype=np.float16)
    chain = R.mip_chain(src, 4)
    pre = R.prefiltered(chain, 8, 4, 64)
    irr = R.irradiance(chain, 4, 64)
    return chain, pre, irr


def test_a_constant_source_stays_constant():
    """f16(c) in every prefiltered level, f16(pi c) in the irradiance — and the f64 values lie at least 0.05 ulp from a rounding midpoint, so the
    device, whose f32 sums differ in the last bits, can be held to the exact f16 bits."""
    chain, pre, irr = constant_expectations()
    c = np.array(CONSTANT)
    for values, want in [(lv, c) for lv in pre] + [(irr, math.pi * c)]:
        assert (values.astype(np.float16) == want.astype(np.float16)).all()
        ulp = R.f16_ulp(values)
        frac = values / ulp - np.floor(values / ulp)             # position between two f16 values; the midpoint is 0.5
        assert (np.abs(frac - 0.5) >= 0.05).all(), float(np.abs(frac - 0.5).min())
        assert np.abs(values - want).max() <= 1e-12 * want.max()


# ------------------------------------------------------------------------------------------------ f32 leaves the slack alone

def test_f32_spends_at_most_a_quarter_of_the_slack():
    """The device test allows half an f16 ulp (the store) plus 2^-16 |ref| for the f32 frame, sampling and sums.  The restatement run in f32 on the
    same inputs stays within a quarter of that second term of its f64 run."""
    worst = 0.0
    chains = {n: source_chain(n) for n in (16, 12)}
    for ns, size, mips, samples in GGX_CASES:
        ref = R.prefiltered(chains[ns], size, mips, samples)
        f32 = R.prefiltered(chains[ns], size, mips, samples, np.float32)
        for a, b in zip(ref, f32):
            worst = max(worst, float((np.abs(b.astype(np.float64) - a) / np.abs(a)).max()))
    for ns, size, samples in LAMBERT_CASES:
        a, b = R.irradiance(chains[ns], size, samples), R.irradiance(chains[ns], size, samples, np.float32)
        worst = max(worst, float((np.abs(b.astype(np.float64) - a) / np.abs(a)).max()))
    print("f32 against f64, largest relative difference: %.3g (a quarter of the slack: %.3g)" % (worst, 2.0 ** -18))
    assert worst <= 2.0 ** -18, worst


def test_the_source_and_the_filtered_levels_are_what_the_issue_asks_for():
    src = R.smooth_hdr_source(16).astype(np.float64)
    assert src[..., :3].min() >= 0.05 and src[..., :3].max() <= 10.0 and src[..., :3].max() > 5.0 and (src[..., 3] == 1.0).all()
    chain = source_chain(16)
    pre = R.prefiltered(chain, 16, 5, 64)
    assert [p.shape for p in pre] == [(6, 16, 16, 3), (6, 8, 8, 3), (6, 4, 4, 3), (6, 2, 2, 3), (6, 1, 1, 3)]
    assert (pre[0] == chain[0][..., :3]).all()
    spread = [float(p.max() - p.min()) for p in pre]
    assert all(a > b for a, b in zip(spread[1:], spread[2:])), spread      # rougher levels are smoother
    assert [p.shape for p in R.prefiltered(source_chain(12), 12, 4, 128)] == [(6, 12, 12, 3), (6, 6, 6, 3), (6, 3, 3, 3), (6, 1, 1, 3)]


# ------------------------------------------------------------------------------------------------ the host over a backend without the symbol

def test_host_over_the_mock_backend_refuses_the_bake(mock):
    h = H.Host(backend_path=MOCK)
    with pytest.raises(H.HostError) as e:
        h.env_bake_ibl(16, 5, 8, 64)
    assert e.value.code == UNSUPPORTED and "awsm_hip_env_cube_filter" in str(e.value), e.value
    h.close()
