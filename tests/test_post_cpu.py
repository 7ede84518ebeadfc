"""CPU tests of the effects + display passes: the oracle's known answers (tests/post_oracle.py), its tables against the kernel's
(kernels_post.hip), and the AwsmPostParams layout against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import hip_backend
from tests import post_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


def test_khronos_neutral_known_answers():
    np.testing.assert_allclose(po.khronos_neutral(np.array([0.5, 0.5, 0.5], f)), [0.46, 0.46, 0.46], rtol=1e-6)
    np.testing.assert_allclose(po.khronos_neutral(np.array([2.0, 1.0, 0.5], f)), [0.96, 0.53409, 0.32114], atol=1e-5)
    np.testing.assert_allclose(po.khronos_neutral(np.array([0.05, 0.2, 0.3], f)), [0.015625, 0.165625, 0.265625], atol=1e-6)


def test_aces_and_srgb_known_answers():
    np.testing.assert_allclose(po.aces(np.array([1.0, 0.18], f)), [0.803797, 0.266899], atol=1e-6)
    s = po.linear_to_srgb(np.array([0.5], f))
    np.testing.assert_allclose(s, [0.735357], atol=1e-6)
    assert po.unorm8(s)[0] == 188
    assert po.unorm8(np.array([np.nan, -1.0, 2.0], f)).tolist() == [0, 0, 255]


def test_bloom_has_thirteen_taps_and_unit_weight():
    assert len(po.BLOOM_TAPS) == 13 and len(po.BLOOM_W) == 13
    assert abs(float(po.BLOOM_W.astype(np.float64).sum()) - 1.0) < 1e-6
    flat = np.full((9, 11, 3), 0.25, f)
    assert np.array_equal(po.blur13(flat), np.full_like(flat, po.blur13(flat)[0, 0]))


def _kernel_table(name):
    text = open(os.path.join(ROOT, "awsm-renderer_amd", "csrc", "kernels_post.hip")).read()
    body = re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, text, re.S).group(1)
    return np.array([float(v.rstrip("f")) for v in re.findall(r"-?\d+\.\d+e[+-]\d+f", body)], dtype=np.float32)


def test_kernel_tables_are_the_oracles():
    assert np.array_equal(_kernel_table("kBloomW"), po.BLOOM_W)
    assert np.array_equal(_kernel_table("kDisk"), po.DISK.reshape(-1))


def _dof_camera(focus, aperture):
    """A reverse-Z infinite projection (proj[2][2] = 0, proj[3][2] = near = 0.1): linearize_depth's near / depth branch, positive depths."""
    cam = np.zeros(128, f)
    cam[16 + 5], cam[16 + 10], cam[16 + 14], cam[16 + 11] = 1.7, 0.0, 0.1, -1.0
    cam[123], cam[124], cam[125] = 24.0, focus, aperture
    return cam


def test_in_focus_image_is_unchanged_by_dof_and_a_defocused_one_changes():
    rng = np.random.default_rng(1)
    comp = po.f32_to_f16(rng.random((24, 32, 4), dtype=np.float32) * 3)
    depth = np.full((24, 32), 0.05, f)                     # linear depth 0.1 / 0.05 = 2
    lin, coc = po.dof_terms(depth, _dof_camera(2.0, 5.6))
    assert (lin == f(2.0)).all() and (coc == 0).all()      # focused exactly on the (flat) scene
    out, ill = po.effects(comp, depth, _dof_camera(2.0, 5.6), dof=True)
    assert not ill.any()
    assert np.array_equal(out[..., :3], comp[..., :3]) and (out[..., 3] == 0x3C00).all()
    _, coc = po.dof_terms(depth, _dof_camera(0.5, 0.1))
    assert (coc > 2.0).all()                                # focused at 0.5: every pixel a full blur
    out, _ = po.effects(comp, depth, _dof_camera(0.5, 0.1), dof=True)
    assert (out[..., :3] != comp[..., :3]).mean() > 0.9


def test_flat_image_is_unchanged_by_smaa():
    comp = po.f32_to_f16(np.full((16, 20, 4), 0.3, f))
    out, _ = po.effects(comp, smaa_on=True)
    assert np.array_equal(out[..., :3], comp[..., :3])


def test_post_params_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = [n for n, _ in hip_backend.AwsmPostParams._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "awsm_hip.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(AwsmPostParams));']
    lines += ['  printf("%s %%zu\\n", offsetof(AwsmPostParams, %s));' % (n, n) for n in fields]
    lines += ['  printf("post_flags %u %u %u\\n", AWSM_POST_SMAA, AWSM_POST_BLOOM, AWSM_POST_DOF);', "  return 0; }"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(l.split(" ", 1) for l in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(hip_backend.AwsmPostParams)
    for n in fields:
        assert int(out[n]) == getattr(hip_backend.AwsmPostParams, n).offset, n
    assert out["post_flags"].split() == [str(hip_backend.AWSM_POST_SMAA), str(hip_backend.AWSM_POST_BLOOM), str(hip_backend.AWSM_POST_DOF)]
