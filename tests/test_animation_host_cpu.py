"""CPU tests of the run-time key API that animation rests on, of update_animations through to the bytes the device receives, and of the host
side of device skin posing — over the recording mock backends (tests/mock/mock_backend.c; tests/mock/mock_skin_pose.c adds the pose entries).
The reference for the bytes is oracle/scene_model.HostModel of a SceneDesc rebuilt from what the host reports (transform_get_local, the
sampled weights)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from awsm_renderer_amd.scenes import quat_axis_angle
from oracle import scene_model as sm
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK_DIR = os.path.join(ROOT, "tests", "mock")
MOCK = os.path.join(MOCK_DIR, "libmock_backend.so")
LUT = np.zeros((4, 4, 4), dtype=np.uint16)
JOINTS = 18


def _bind(lib):
    lib.mock_log_count.restype = C.c_size_t
    lib.mock_log_count.argtypes = [C.c_void_p]
    lib.mock_log_get.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mock_log_clear.argtypes = [C.c_void_p]
    lib.mock_buffer.restype = C.c_void_p
    lib.mock_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    return lib


@pytest.fixture(scope="module")
def mock():
    src = os.path.join(MOCK_DIR, "mock_backend.c")
    if not os.path.exists(MOCK) or os.path.getmtime(src) > os.path.getmtime(MOCK):
        subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", MOCK, src])
    return _bind(C.CDLL(MOCK))


@pytest.fixture(scope="module")
def pose_mock(tmp_path_factory):
    """mock_backend.c + the pose entries, recording."""
    so = str(tmp_path_factory.mktemp("mock") / "libmock_skin_pose.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(MOCK_DIR, "mock_skin_pose.c")])
    lib = _bind(C.CDLL(so))
    lib.mock_pose_ids.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]
    lib.mock_pose_ids.restype = C.c_uint32
    lib.path = so
    return lib


def log_of(mock, ctx):
    out = []
    for i in range(mock.mock_log_count(ctx)):
        op, which, a, b = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        mock.mock_log_get(ctx, i, C.byref(op), C.byref(which), C.byref(a), C.byref(b))
        out.append((op.value, which.value, a.value, b.value))
    return out


def device_bytes(mock, ctx, which):
    n = C.c_size_t()
    p = mock.mock_buffer(ctx, which, C.byref(n))
    return C.string_at(p, n.value) if p else None


def _scene():
    return scenes.skinned_morph_scene(64, 64, around=8, along=12, tex_size=16)


CUBE_NODE = JOINTS + 2      # nodes: rig root, the joints, the tube's node, the cube's node


# ------------------------------------------------------------------------------------------------ the key API
def test_mesh_update_morph_weights_writes_floats_1_to_n_plus_1(mock):
    r = H.Renderer(_scene(), backend_path=MOCK, lut_rgba16f=LUT)
    r.render()
    ctx, cube = r.host.device_ctx, r.keys.mesh_keys[1]
    before = device_bytes(mock, ctx, sm.BUF_MORPH_WEIGHTS)
    gm = np.frombuffer(r.host.mirror(sm.BUF_GEOM_META), np.uint32)
    off = [int(gm[s * 64 + 3]) for s in range(2) if gm[s * 64 + 2] == 2][0]      # the cube's geometry meta: 2 targets, its weights offset
    mock.mock_log_clear(ctx)
    w = np.array([0.625, -0.25], np.float32)
    r.host.mesh_update_morph_weights(cube, w)
    r.render()
    after = device_bytes(mock, ctx, sm.BUF_MORPH_WEIGHTS)
    changed = [i for i in range(len(after)) if after[i] != before[i]]
    assert changed and min(changed) >= off + 4 and max(changed) < off + 4 + 8
    assert after[off + 4: off + 12] == w.tobytes() and after[:off + 4] == before[:off + 4] and after[off + 12:] == before[off + 12:]
    assert after == r.host.mirror(sm.BUF_MORPH_WEIGHTS)
    writes = [(a, b) for op, which, a, b in log_of(mock, ctx) if op == 2 and which == sm.BUF_MORPH_WEIGHTS]
    assert len(writes) == 1 and writes[0][0] <= off + 4 and writes[0][0] + writes[0][1] >= off + 12      # one ranged write that covers them
    for bad, n in ((cube, 3), (cube, 1), (r.keys.mesh_keys[0], 2)):      # a wrong count; a mesh without morph targets
        with pytest.raises(H.HostError) as e:
            r.host.mesh_update_morph_weights(bad, np.zeros(n, np.float32))
        assert e.value.code == -1
    r.close()


def test_light_update_rewrites_the_lights_64_bytes(mock):
    scene = _scene()
    r = H.Renderer(scene, backend_path=MOCK, lut_rgba16f=LUT)
    r.render()
    ctx = r.host.device_ctx
    assert len(scene.lights) >= 2
    before = device_bytes(mock, ctx, sm.BUF_LIGHTS)
    new = {"kind": "spot", "color": (0.25, 0.5, 0.75), "intensity": 3.5, "position": (1, 2, 3), "range": 9.0, "direction": (0, -1, 0), "inner_angle": 0.2, "outer_angle": 0.4}
    mock.mock_log_clear(ctx)
    r.host.light_update(r.keys.light_keys[1], new)
    r.render()
    after = device_bytes(mock, ctx, sm.BUF_LIGHTS)
    want = np.zeros(16, np.float32)
    want[0:4] = (1, 2, 3, 9.0); want[4:8] = (0, -1, 0, 0.2); want[8:12] = (0.25, 0.5, 0.75, 3.5); want[12] = 3.0; want[13] = 0.4      # lights.rs:354-473
    assert after[64:128] == want.tobytes() and after[:64] == before[:64] and after[128:] == before[128:]
    ops = [(op, which) for op, which, _, _ in log_of(mock, ctx)]
    assert (2, sm.BUF_LIGHTS) in ops and (2, sm.BUF_LIGHTS_INFO) not in ops      # the punctual_dirty path alone: the count did not change
    with pytest.raises(H.HostError):
        r.host.light_update(0xDEAD00000001, new)
    r.close()


def test_transform_duplicate_and_get_local(mock):
    h = H.Host(backend_path=MOCK)
    q = np.array(quat_axis_angle((0, 1, 0), 0.3), np.float32)
    parent = h.transform_insert((1, 2, 3), (0, 0, 0, 1), (1, 1, 1))
    child = h.transform_insert((0.5, 0.25, -4), q, (2, 3, 4), parent)
    grand = h.transform_insert((9, 9, 9), (0, 0, 0, 1), (1, 1, 1), child)
    t, r_, s = h.transform_get_local(child)
    assert t.tobytes() == np.array([0.5, 0.25, -4], np.float32).tobytes() and r_.tobytes() == q.tobytes() and s.tobytes() == np.array([2, 3, 4], np.float32).tobytes()
    dup = h.transform_duplicate(child)      # transforms.rs:151-155: same local, same parent; children are not copied
    assert dup not in (parent, child, grand) and h.transform_parent(dup) == parent
    assert [a.tobytes() for a in h.transform_get_local(dup)] == [a.tobytes() for a in h.transform_get_local(child)]
    h.update_transforms()
    assert h.transform_world(dup).tobytes() == h.transform_world(child).tobytes()
    assert h.transform_parent(grand) == child
    top = h.transform_duplicate(parent)      # a node under the root duplicates under the root
    assert h.transform_parent(top) == h.transform_parent(parent)
    h.transform_set_local(dup, (0, 0, 0), (0, 0, 0, 1), (1, 1, 1))      # the copy is its own node
    assert h.transform_get_local(child)[0].tobytes() == np.array([0.5, 0.25, -4], np.float32).tobytes()
    with pytest.raises(H.HostError):
        h.transform_duplicate(0xDEAD00000001)
    with pytest.raises(H.HostError):
        h.transform_get_local(0xDEAD00000001)
    h.close()


# ------------------------------------------------------------------------------------------------ animated frames
def _add_players(r):
    """Rotation on three joints (linear / step / cubic), translation on the cube's node, linear weights on the cube."""
    hst, nk = r.host, r.keys.node_keys
    q = lambda a: np.array(quat_axis_angle((0, 0, 1), a), np.float32)      # noqa: E731
    times = [0.0, 0.4, 1.0]
    keys = {}
    keys["lin"] = hst.animation_insert_transform(nk[3], "rotation", times, [q(-0.3), q(0.2), q(0.5)])
    keys["step"] = hst.animation_insert_transform(nk[7], "rotation", times, [q(0.1), q(-0.25), q(0.3)], "step")
    tan = np.array([[0, 0, 0.2, 0], [0, 0, -0.1, 0.05], [0, 0, 0.3, 0]], np.float32)
    keys["cubic"] = hst.animation_insert_transform(nk[12], "rotation", times, [q(0.0), q(0.35), q(-0.2)], "cubic", tan, -tan)
    keys["move"] = hst.animation_insert_transform(nk[CUBE_NODE], "translation", [0.0, 1.0], [[1.6, 0, 0], [1.2, 0.4, 0.3]])
    keys["morph"] = hst.animation_insert_morph(r.keys.mesh_keys[1], [0.0, 0.5, 1.0], [[0, 0], [1, 0.25], [0.2, 0.9]])
    hst.animation_set_playback(keys["step"], loop_style=H.ANIM_PING_PONG)
    hst.animation_set_playback(keys["cubic"], loop_style=H.ANIM_LOOP_NONE)
    return keys


def _scene_as_the_host_reports_it(base, r, keys):
    sc = copy.deepcopy(base)
    for i, n in enumerate(sc.nodes):
        t, q, s = r.host.transform_get_local(r.keys.node_keys[i])
        n.translation, n.rotation, n.scale = tuple(float(x) for x in t), tuple(float(x) for x in q), tuple(float(x) for x in s)
    sc.nodes[CUBE_NODE].primitives[0].animated_morph_weights = r.host.animation_sample(keys["morph"])
    return sc


DTS = [130.0, 90.0, 410.0, 250.0, 333.0, 61.0]


@pytest.mark.parametrize("posing", ["host", "device"])
def test_animated_frames_reach_the_device_as_the_model_has_them(posing, pose_mock):
    base = _scene()
    r = H.Renderer(base, backend_path=pose_mock.path, lut_rgba16f=LUT)
    if posing == "device":
        r.host.set_device_skin_posing(True)
    keys = _add_players(r)
    ctx = r.host.device_ctx
    for dt in DTS:
        r.update_all(dt)
        r.render()
        model = helpers.build_model(_scene_as_the_host_reports_it(base, r, keys))
        for which in (sm.BUF_TRANSFORMS, sm.BUF_SKIN_MATRICES, sm.BUF_MORPH_WEIGHTS, sm.BUF_NORMAL_MATS):
            want = bytes(model.mirrors()[which])
            assert device_bytes(pose_mock, ctx, which) == want, (dt, which)
            assert r.host.mirror(which) == want, (dt, which)
    st = {k: r.host.animation_state(v) for k, v in keys.items()}
    assert st["cubic"]["state"] == H.ANIM_ENDED and st["step"]["direction"] == H.ANIM_BACKWARD and st["lin"]["local_time"] < 0.3      # ended, reversed, wrapped
    r.close()


def test_device_posing_sends_ids_not_matrices(pose_mock):
    base = _scene()
    off = H.Renderer(base, backend_path=pose_mock.path, lut_rgba16f=LUT)      # the posing-off host beside it: same scene, same players, same steps
    on = H.Renderer(base, backend_path=pose_mock.path, lut_rgba16f=LUT)
    on.host.set_device_skin_posing(True)
    k_off, k_on = _add_players(off), _add_players(on)
    ctx = on.host.device_ctx
    for frame, dt in enumerate(DTS):
        for r in (off, on):
            r.update_all(dt)
        pose_mock.mock_log_clear(ctx)
        off.render(); on.render()
        log = log_of(pose_mock, ctx)
        if frame > 0:
            assert not [e for e in log if e[0] in (1, 2) and e[1] == sm.BUF_SKIN_MATRICES], "a skin matrix crossed the bus"
            assert not [e for e in log if e[0] == 30], "records are resident after the first frame"
        # joints 3, 7 and 12 carry players (set_local every frame marks them dirty) and every joint below joint 3 in the chain moves with it:
        # records 2 .. 17 of the one skin (record id = joint index; node j + 1 is joint j)
        want_ids = list(range(2, JOINTS))
        ids = (C.c_uint32 * 64)()
        n = pose_mock.mock_pose_ids(ctx, ids, 64)
        assert list(ids[:n]) == want_ids and on.host.skin_pose_ids_last_frame() == want_ids
        assert [e[2] for e in log if e[0] == 31] == [len(want_ids)]
        assert on.host.mirror(sm.BUF_SKIN_MATRICES) == off.host.mirror(sm.BUF_SKIN_MATRICES)
        assert device_bytes(pose_mock, ctx, sm.BUF_SKIN_MATRICES) == device_bytes(pose_mock, off.host.device_ctx, sm.BUF_SKIN_MATRICES)
        if frame > 0:
            assert off.host.upload_bytes_last_frame() - on.host.upload_bytes_last_frame() == 60 * len(want_ids)      # 64 bytes of matrix against 4 of id
    # nothing moves: nothing is posed
    for k in k_on.values():
        on.host.animation_remove(k)
    on.update_all(16.0); on.render()
    assert on.host.skin_pose_ids_last_frame() == []
    # back to the host: the joints that moved since are composed on the CPU and uploaded
    on.host.transform_set_local(on.keys.node_keys[5], (0, 0.2, 0), quat_axis_angle((0, 0, 1), 0.4), (1, 1, 1))
    off.host.transform_set_local(off.keys.node_keys[5], (0, 0.2, 0), quat_axis_angle((0, 0, 1), 0.4), (1, 1, 1))
    for k in k_off.values():
        off.host.animation_remove(k)
    on.host.update_transforms(); off.host.update_transforms()
    on.host.set_device_skin_posing(False)
    pose_mock.mock_log_clear(ctx)
    on.render(); off.render()
    assert [e for e in log_of(pose_mock, ctx) if e[0] == 2 and e[1] == sm.BUF_SKIN_MATRICES] and not [e for e in log_of(pose_mock, ctx) if e[0] == 31]
    assert device_bytes(pose_mock, ctx, sm.BUF_SKIN_MATRICES) == device_bytes(pose_mock, off.host.device_ctx, sm.BUF_SKIN_MATRICES) == off.host.mirror(sm.BUF_SKIN_MATRICES)
    off.close(); on.close()


def _same_as_posing_off(pose_mock, off, on, tag):
    want = off.host.mirror(sm.BUF_SKIN_MATRICES)
    assert on.host.mirror(sm.BUF_SKIN_MATRICES) == want, tag
    assert device_bytes(pose_mock, off.host.device_ctx, sm.BUF_SKIN_MATRICES) == want, tag
    assert device_bytes(pose_mock, on.host.device_ctx, sm.BUF_SKIN_MATRICES) == want, tag


@pytest.mark.parametrize("pending", [False, True])
def test_a_second_skin_on_shared_joints_rewrites_the_records_it_changed(pending, pose_mock):
    """inverse_bind is keyed by the joint (host.cpp skin_insert): a later skin's matrices replace an earlier one's for the joints they share, from the
    joint's next move on — not before.  So what the device composed with the earlier matrices, and (pending) what update_transforms had already
    handed over for the next frame when the skin came, stays composed with them; the resident records follow for later moves; and the insert, which
    grows the buffer here, takes the cold path (the whole mirror goes up) unharmed.  Mirror and device are compared with the posing-off host's
    straight after the insert, before any shared joint moves, and again after one does."""
    base = _scene()
    rs = []
    for posing in (False, True):
        r = H.Renderer(base, backend_path=pose_mock.path, lut_rgba16f=LUT)
        r.host.set_device_skin_posing(posing)
        r.render()
        r.host.transform_set_local(r.keys.node_keys[4], (0, 0.2, 0), quat_axis_angle((0, 0, 1), 0.3), (1, 1, 1))      # joints 3 .. 17 move: 5 and 8 are shared below
        r.update()
        if not pending:
            r.render()
        rs.append(r)
    off, on = rs
    if not pending:
        _same_as_posing_off(pose_mock, off, on, "before the insert")
    size_before = len(off.host.mirror(sm.BUF_SKIN_MATRICES))
    for r in rs:
        ib = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
        ib[:, 3, 0] = (0.5, -0.25, 2.0)
        prim = base.nodes[JOINTS + 1].primitives[0]
        nk = r.keys.node_keys
        r.host.skin_insert([nk[6], nk[2], nk[9]], ib, [np.zeros_like(prim.joints[0])], prim.weights)
        r.render()      # nothing has moved since the insert
    assert len(off.host.mirror(sm.BUF_SKIN_MATRICES)) > size_before      # the insert grew the buffer
    _same_as_posing_off(pose_mock, off, on, "after the insert, before a shared joint moves")
    for r in rs:
        r.host.transform_set_local(r.keys.node_keys[2], (0, 0.2, 0), quat_axis_angle((0, 0, 1), -0.2), (1, 1, 1))
        r.update(); r.render()
    assert on.host.skin_pose_ids_last_frame() == sorted(list(range(1, JOINTS)) + [JOINTS, JOINTS + 1, JOINTS + 2])
    _same_as_posing_off(pose_mock, off, on, "after a shared joint moved")
    off.close(); on.close()


def test_host_posing_uploads_the_moved_joints_matrices_alone(pose_mock):
    """Posing off: a moved joint marks the 64 bytes of its own matrix dirty, not the skin's whole block as the reference's update_with_unchecked does
    (skins.rs:182-188; DESIGN.md section 15: a deviation in the upload range, not in the bytes).  Adjacent matrices go up as one write."""
    base = _scene()
    r = H.Renderer(base, backend_path=pose_mock.path, lut_rgba16f=LUT)
    r.render()
    ctx = r.host.device_ctx
    gm = np.frombuffer(r.host.mirror(sm.BUF_GEOM_META), np.uint32)
    off = [int(gm[s * 64 + 6]) for s in range(2) if gm[s * 64 + 5]][0]      # the tube's geometry meta: its skin matrices offset
    before = device_bytes(pose_mock, ctx, sm.BUF_SKIN_MATRICES)
    pose_mock.mock_log_clear(ctx)
    r.host.transform_set_local(r.keys.node_keys[JOINTS], (0, 0.2, 0), quat_axis_angle((0, 0, 1), 0.3), (1, 1, 1))      # the last joint of the chain: it alone moves
    r.update(); r.render()
    writes = [(a, b) for op, which, a, b in log_of(pose_mock, ctx) if op == 2 and which == sm.BUF_SKIN_MATRICES]
    assert writes == [(off + 64 * (JOINTS - 1), 64)]
    after = device_bytes(pose_mock, ctx, sm.BUF_SKIN_MATRICES)
    assert after == r.host.mirror(sm.BUF_SKIN_MATRICES) and after[:writes[0][0]] == before[:writes[0][0]] and after[writes[0][0] + 64:] == before[writes[0][0] + 64:]
    pose_mock.mock_log_clear(ctx)
    r.host.transform_set_local(r.keys.node_keys[JOINTS - 3], (0, 0.2, 0), quat_axis_angle((0, 0, 1), 0.1), (1, 1, 1))      # joints 14 .. 17 move
    r.update(); r.render()
    assert [(a, b) for op, which, a, b in log_of(pose_mock, ctx) if op == 2 and which == sm.BUF_SKIN_MATRICES] == [(off + 64 * (JOINTS - 4), 256)]
    r.close()


def test_plain_backend_refuses_device_posing_and_animates_on_the_host(mock):
    base = _scene()
    r = H.Renderer(base, backend_path=MOCK, lut_rgba16f=LUT)
    with pytest.raises(H.HostError) as e:
        r.host.set_device_skin_posing(True)
    assert e.value.code == -5 and "awsm_hip_skin_pose_records_write" in str(e.value)      # AWSM_ERR_NOT_READY, naming the symbol
    r.host.set_device_skin_posing(False)
    keys = _add_players(r)
    r.update_all(200.0)
    r.render()
    model = helpers.build_model(_scene_as_the_host_reports_it(base, r, keys))
    assert device_bytes(mock, r.host.device_ctx, sm.BUF_SKIN_MATRICES) == bytes(model.mirrors()[sm.BUF_SKIN_MATRICES])
    assert r.host.skin_pose_ids_last_frame() == []
    r.close()


def test_abi_versions_stay_2():
    lib = H.load_library()
    lib.awsm_host_abi_version.restype = C.c_uint32
    assert lib.awsm_host_abi_version() == 2
