"""CPU tests of the host layer's post-processing entry points over the recording mock backend (tests/mock/mock_backend.c), which has no
awsm_hip_post_pass: the host still loads, set_post_processing reports AWSM_ERR_UNSUPPORTED, and camera_set_dof lands in the camera mirror."""
import numpy as np
import pytest

from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from tests.test_host_layer_cpu import MOCK, device_bytes, log_of, mock  # noqa: F401  (the module-scoped fixture)

BUF_CAMERA = 5


def _renderer():
    return H.Renderer(scenes.box_scene(64, 64), backend_path=MOCK, lut_rgba16f=np.zeros((4, 4, 4), dtype=np.uint16))


def test_host_without_post_pass_symbol_still_loads_and_refuses_post_processing(mock):
    r = _renderer()
    with pytest.raises(H.HostError, match=r"\(-6\)"):          # AWSM_ERR_UNSUPPORTED
        r.host.set_post_processing(1, bloom=True)
    r.render()                         # and renders as before
    r.close()


def test_camera_set_dof_writes_bytes_496_to_503(mock):
    r = _renderer()
    r.render()
    cam = np.frombuffer(device_bytes(mock, r.host.device_ctx, BUF_CAMERA), dtype=np.float32)
    assert cam[124] == 0.0 and cam[125] == 0.0         # the host writes 0, 0 until camera_set_dof
    mock.mock_log_clear(r.host.device_ctx)
    r.host.camera_set_dof(10.0, 5.6)
    r.render()
    writes = [(a, b) for op, w, a, b in log_of(mock, r.host.device_ctx) if op == "write" and w == BUF_CAMERA]
    assert any(a <= 496 and a + b >= 504 for a, b in writes), writes      # a dirty range covers bytes 496-503
    cam = np.frombuffer(device_bytes(mock, r.host.device_ctx, BUF_CAMERA), dtype=np.float32)
    assert cam[124] == np.float32(10.0) and cam[125] == np.float32(5.6)
    r.update()                                         # camera_update keeps the DoF parameters
    r.render()
    cam = np.frombuffer(device_bytes(mock, r.host.device_ctx, BUF_CAMERA), dtype=np.float32)
    assert cam[124] == np.float32(10.0) and cam[125] == np.float32(5.6)
    r.close()
