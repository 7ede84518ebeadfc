"""GPU test of animated frames end to end: players advance (update_all), the host uploads what moved, and after every one of 8 overlapped frames the
transformed vertices and visibility keys are bit-exact against the oracle's frame of the scene as it then is (a SceneDesc rebuilt from
transform_get_local and the sampled weights, the pattern of test_geometry_cache_recomputes_what_was_written_and_nothing_else); colours at the
compare_frames bar.  The geometry cache keeps the static box's workgroups and recomputes the animated draws'.  Run with skin posing on the host,
on the device, and with AWSM_GEOMETRY_CACHE=0; the device run must hit the cache exactly as the host run does.

The scene is the geometry-cache test's: skinned_morph_scene(480, 270, around=16, along=40, tex_size=16) plus a small static box.  Players: rotation
on three joints (linear and looping, step and ping-pong, cubic and not looping), translation on the cube's node, linear weights on the cube.
"""
import copy

import numpy as np
import pytest

from awsm_renderer_amd import gltf_export, scenes
from awsm_renderer_amd import host as H
from awsm_renderer_amd.hip_backend import HipDevice
from awsm_renderer_amd.scene_desc import NodeDesc
from awsm_renderer_amd.scenes import quat_axis_angle
from oracle import oracle_lib
from tests import helpers

JOINTS = 18
CUBE_NODE = JOINTS + 2
DTS = [130.0, 90.0, 210.0, 170.0, 250.0, 110.0, 230.0, 60.0]      # ms; 1250 in all over clips of 1.0 s: one wrap, one reversal, one end
TIMES = [0.0, 0.4, 1.0]


def _q(a):
    return np.array(quat_axis_angle((0, 0, 1), a), np.float32)


CUBIC_TAN = np.array([[0, 0, 0.2, 0], [0, 0, -0.1, 0.05], [0, 0, 0.3, 0]], np.float32)
CHANNELS = [      # in the order the glTF reader makes its players: joints in node order, then the cube's node, then the cube's weights
    dict(node=3, path="rotation", interpolation="linear", times=TIMES, values=[_q(-0.3), _q(0.2), _q(0.5)]),
    dict(node=7, path="rotation", interpolation="step", times=TIMES, values=[_q(0.1), _q(-0.25), _q(0.3)]),
    dict(node=12, path="rotation", interpolation="cubic", times=TIMES, values=[_q(0.0), _q(0.35), _q(-0.2)], in_tangents=CUBIC_TAN, out_tangents=-CUBIC_TAN),
    dict(node=CUBE_NODE, path="translation", interpolation="linear", times=[0.0, 1.0], values=[[1.6, 0, 0], [1.45, 0.25, 0.1]]),
    dict(node=CUBE_NODE, path="weights", interpolation="linear", times=[0.0, 0.5, 1.0], values=[[0, 0], [1, 0.25], [0.2, 0.9]]),
]
NAMES = ["lin", "step", "cubic", "move", "morph"]


def _base():
    base = scenes.skinned_morph_scene(480, 270, around=16, along=40, tex_size=16)
    box = copy.deepcopy(scenes.box_scene().nodes[1].primitives[0])
    box.material = 1
    base.nodes.append(NodeDesc(translation=(-1.5, 0.3, 0.2), scale=(0.5, 0.5, 0.5), primitives=[box]))      # a mesh no player concerns
    return base


def _add_players(r):
    keys = {}
    for name, ch in zip(NAMES, CHANNELS):
        args = (ch["times"], ch["values"], ch["interpolation"], ch.get("in_tangents"), ch.get("out_tangents"))
        if ch["path"] == "weights":
            keys[name] = r.host.animation_insert_morph(r.keys.mesh_keys[1], *args)
        else:
            keys[name] = r.host.animation_insert_transform(r.keys.node_keys[ch["node"]], ch["path"], *args)
    return keys


def _styles(host, keys):
    host.animation_set_playback(keys["step"], loop_style=H.ANIM_PING_PONG)
    host.animation_set_playback(keys["cubic"], loop_style=H.ANIM_LOOP_NONE)


def _scene_as_the_host_reports_it(base, r, keys):
    sc = copy.deepcopy(base)
    for i, n in enumerate(sc.nodes):
        t, q, s = r.host.transform_get_local(r.keys.node_keys[i])
        n.translation, n.rotation, n.scale = tuple(float(x) for x in t), tuple(float(x) for x in q), tuple(float(x) for x in s)
    sc.nodes[CUBE_NODE].primitives[0].animated_morph_weights = r.host.animation_sample(keys["morph"])
    return sc


_ORACLE = {}      # frame index -> OracleFrame: the scene of a frame does not depend on where the skin matrices are composed
_RUNS = {}        # variant -> per-frame records


def _run(variant, lut, monkeypatch):
    if variant in _RUNS:
        return _RUNS[variant]
    if variant == "cache_off":
        monkeypatch.setenv("AWSM_GEOMETRY_CACHE", "0")
    else:
        monkeypatch.delenv("AWSM_GEOMETRY_CACHE", raising=False)
    base = _base()
    r = H.Renderer(base, parity_tap=True, overlap_frames=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(lut))
    r.host.set_device_skin_posing(variant == "device")
    keys = _add_players(r)
    _styles(r.host, keys)
    dev = HipDevice.from_ctx(r.host.device_ctx, base.width, base.height)
    blocks = lambda d: (3 * d["tri_count"] + 255) // 256      # noqa: E731
    frames, prev_lists, wraps, flips = [], {}, 0, 0
    last_t, last_dir = 0.0, H.ANIM_FORWARD
    for i, dt in enumerate(DTS):
        r.update_all(dt)
        st = r.render(sync=True)
        lin, step = r.host.animation_state(keys["lin"]), r.host.animation_state(keys["step"])
        wraps += lin["local_time"] < last_t
        flips += step["direction"] != last_dir
        last_t, last_dir = lin["local_time"], step["direction"]
        if i not in _ORACLE:
            _ORACLE[i] = helpers.oracle_frame(helpers.build_model(_scene_as_the_host_reports_it(base, r, keys)), lut)
        orc = _ORACLE[i]
        res = helpers.compare_frames(orc, dev)
        print(f"animated frame {i} ({variant}): {res}")
        assert res["clip_mismatch"] == 0 and res["nt_mismatch"] == 0 and res["key_mismatch"] == 0, (variant, i, res)      # bit-exact
        assert res["rgb_over_tol"] == 0 and res["f16_max_ulp"] <= 2, (variant, i, res)
        # the test's own model of the cache: a draw keeps its workgroups when it sits where it sat in this slot's last frame and nothing it reads was
        # written since; the tube (joints) and the cube (node, weights) are written before every frame, the box never
        draws = r.host.draw_list()
        placed, first = [], 0
        for k, d in enumerate(draws):
            placed.append((k, first, tuple(sorted(d.items()))))
            first += d["tri_count"]
        slot = i % 2
        box = [p for p in placed if dict(p[2])["tri_count"] == 12 and dict(p[2])["vis_data_off"] == max(dict(q[2])["vis_data_off"] for q in placed)]
        assert len(box) == 1
        kept = blocks(dict(box[0][2])) if variant != "cache_off" and box[0] in prev_lists.get(slot, ()) else 0
        prev_lists[slot] = placed
        total = sum(blocks(d) for d in draws)
        assert st["geometry_blocks"] == total and st["geometry_cache_blocks"] == kept, (variant, i, st["geometry_blocks"], st["geometry_cache_blocks"], total, kept)
        if i >= 2 and variant != "cache_off":      # from each slot's second frame: the box's workgroups are kept, the animated draws' are not
            assert 0 < st["geometry_cache_blocks"] < st["geometry_blocks"], (variant, i, st)
        frames.append({"cache_blocks": st["geometry_cache_blocks"], "blocks": st["geometry_blocks"], "upload": r.host.upload_bytes_last_frame(),
                       "posed": len(r.host.skin_pose_ids_last_frame()), "clip": dev.read_transformed(orc.n_verts)})
    states = {k: r.host.animation_state(v) for k, v in keys.items()}
    assert wraps == 1 and flips == 1 and states["step"]["direction"] == H.ANIM_BACKWARD and states["cubic"]["state"] == H.ANIM_ENDED, (wraps, flips, states)
    dev.close(); r.close()
    _RUNS[variant] = frames
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["host", "device", "cache_off"])
def test_animated_frames_are_the_oracles_and_the_cache_keeps_the_static_box(variant, oracle_lut, monkeypatch):
    frames = _run(variant, oracle_lut, monkeypatch)
    if variant == "cache_off":
        assert all(f["cache_blocks"] == 0 for f in frames)
    if variant == "device":
        host = _run("host", oracle_lut, monkeypatch)
        assert [f["cache_blocks"] for f in frames] == [f["cache_blocks"] for f in host]      # the pose kernel's dirty ranges are a buffer_write's
        assert all(f["posed"] == JOINTS - 2 for f in frames[1:]) and all(f["posed"] == 0 for f in host)      # joints 2 .. 17 hang below the first animated one
        assert all(d["upload"] < h["upload"] for d, h in zip(frames[1:], host[1:]))


@pytest.mark.gpu
def test_device_posing_uploads_60_bytes_less_per_dirty_joint(oracle_lut, monkeypatch):
    """A matrix is 64 bytes, an id 4: posing on the device saves 60 bytes per dirty joint.  The host path marks the 64 bytes of each moved joint's
    matrix dirty (not the skin's whole block, as the reference's update_with_unchecked would: DESIGN.md section 15), and the 16 joints that move here
    are adjacent, so they go up as one 1024-byte write against 64 bytes of ids."""
    host, device = _run("host", oracle_lut, monkeypatch), _run("device", oracle_lut, monkeypatch)
    for i in range(1, len(DTS)):
        print(f"frame {i}: host posing uploads {host[i]['upload']} bytes, device posing {device[i]['upload']}, {device[i]['posed']} joints posed")
    for i in range(1, len(DTS)):
        assert host[i]["upload"] - device[i]["upload"] == 60 * device[i]["posed"], (i, host[i]["upload"], device[i]["upload"], device[i]["posed"])


@pytest.mark.gpu
def test_scene_loaded_from_a_glb_with_its_animations_moves_the_same(oracle_lut, monkeypatch, tmp_path):
    """One frame of the same scene loaded from an exported .glb, its players advanced by the same dt: the same transformed vertices, bit for bit."""
    want = _run("host", oracle_lut, monkeypatch)[0]["clip"]
    monkeypatch.delenv("AWSM_GEOMETRY_CACHE", raising=False)
    base = _base()
    base.animations = [{"channels": CHANNELS}]
    path = str(tmp_path / "animated.glb")
    gltf_export.write_glb(base, path)
    r = H.Renderer(base, parity_tap=True, overlap_frames=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), gltf=path)
    assert r.gltf_info["animations"] == len(CHANNELS) and r.gltf_info["animation_channels_skipped"] == 0
    _styles(r.host, dict(zip(NAMES, r.host.gltf_animation_keys())))
    r.update_all(DTS[0])
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, base.width, base.height)
    clip, nt = dev.read_transformed(want[0].shape[0])
    assert (clip.view(np.uint32) == want[0].view(np.uint32)).all() and (nt.view(np.uint32) == want[1].view(np.uint32)).all()
    dev.close(); r.close()
