"""CPU tests of glTF animations: gltf_export writes SceneDesc.animations, the native reader (host/gltf.cpp) makes players from them — the first
sampler per (node, path) wins, cubic outputs are split per key, unusable channels are counted — and a scene without animations is exported
byte for byte as before.  Over the mock backend."""
import copy
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import gltf_export
from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from awsm_renderer_amd.scenes import quat_axis_angle

MOCK_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mock")
MOCK = os.path.join(MOCK_DIR, "libmock_backend.so")
JOINTS = 18
TUBE_NODE, CUBE_NODE = JOINTS + 1, JOINTS + 2


@pytest.fixture(scope="module", autouse=True)
def _mock():
    src = os.path.join(MOCK_DIR, "mock_backend.c")
    if not os.path.exists(MOCK) or os.path.getmtime(src) > os.path.getmtime(MOCK):
        subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-o", MOCK, src])


def _scene():
    return scenes.skinned_morph_scene(64, 64, around=8, along=12, tex_size=16)


def _q(a):
    return np.array(quat_axis_angle((0, 0, 1), a), np.float32)


def _channels():
    """T / R / S channels in all three interpolations on the rig, one morph channel, a duplicate on one (node, path), an unknown path, an integer output."""
    rng = np.random.default_rng(5)
    t3 = [0.25, 0.5, 1.0, 2.0]      # the first key is not at 0: the clips are played over the wrong window, as in the reference
    tan3 = lambda: rng.normal(size=(4, 3)).astype(np.float32)      # noqa: E731
    tan4 = lambda: (rng.normal(size=(4, 4)) * 0.2).astype(np.float32)      # noqa: E731
    first = [
        dict(node=2, path="rotation", interpolation="linear", times=t3, values=[_q(0.1), _q(-0.2), _q(0.4), _q(0.0)]),
        dict(node=2, path="translation", interpolation="step", times=t3, values=rng.normal(size=(4, 3)).astype(np.float32)),
        dict(node=5, path="rotation", interpolation="cubic", times=t3, values=[_q(0.3), _q(0.2), _q(-0.4), _q(0.1)], in_tangents=tan4(), out_tangents=tan4()),
        dict(node=5, path="scale", interpolation="cubic", times=t3, values=rng.uniform(0.5, 1.5, size=(4, 3)).astype(np.float32), in_tangents=tan3(), out_tangents=tan3()),
        dict(node=9, path="rotation", interpolation="step", times=t3, values=[_q(0.0), _q(0.2), _q(0.1), _q(-0.1)]),
        dict(node=9, path="scale", interpolation="linear", times=t3, values=rng.uniform(0.5, 1.5, size=(4, 3)).astype(np.float32)),
        dict(node=CUBE_NODE, path="translation", interpolation="linear", times=[0.0, 1.0], values=[[1.6, 0, 0], [1.2, 0.4, 0.3]]),
        dict(node=CUBE_NODE, path="translation", interpolation="cubic", times=[0.0, 1.0], values=[[9, 9, 9], [8, 8, 8]], in_tangents=np.zeros((2, 3)), out_tangents=np.zeros((2, 3))),      # duplicate (node, path): ignored
        dict(node=CUBE_NODE, path="weights", interpolation="cubic", times=[0.0, 0.5, 1.5], values=[[0, 0], [1, 0.25], [0.2, 0.9]],
             in_tangents=rng.normal(size=(3, 2)).astype(np.float32), out_tangents=rng.normal(size=(3, 2)).astype(np.float32)),
    ]
    second = [
        dict(node=2, path="rotation", interpolation="step", times=[0.0, 1.0], values=[_q(1.0), _q(2.0)]),      # duplicate in a later animation: ignored
        dict(node=3, path="pointer", interpolation="linear", times=[0.0, 1.0], values=[[0.0], [1.0]]),          # a path the reader does not know: skipped
        dict(node=4, path="rotation", interpolation="linear", times=[0.0, 1.0], values=[_q(0.0), _q(0.5)]),      # its output is made a normalised i16 accessor below: skipped
        dict(node=7, path="translation", interpolation="linear", times=[0.0, 3.0], values=[[0, 0, 0], [0, 1, 0]]),
    ]
    return [{"name": "a", "channels": first}, {"channels": second}]


def _write_glb(doc, blob, path):
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * ((4 - len(js) % 4) % 4)
    blob += b"\0" * ((4 - len(blob) % 4) % 4)
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(blob)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A)); f.write(js)
        f.write(struct.pack("<II", len(blob), 0x004E4942)); f.write(blob)


# what the reader makes, in its insertion order: nodes depth first (the joints are a chain: 1, 2, ... 18; then the cube's node), T then R then S per
# node; the morph player when the cube's mesh is inserted
def _expected(anims):
    a, b = anims[0]["channels"], anims[1]["channels"]
    return [a[1], a[0], a[2], a[3], b[3], a[4], a[5], a[6], a[8]]


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    scene = _scene()
    scene.animations = _channels()
    path = str(tmp_path_factory.mktemp("gltf") / "animated.glb")
    doc, blob, _ = gltf_export.scene_to_gltf(scene, embed_images=True)
    acc = doc["accessors"][doc["animations"][1]["samplers"][2]["output"]]      # node 4's rotation: an integer output, which the reader passes over
    assert acc["type"] == "VEC4" and acc["componentType"] == 5126
    acc["componentType"], acc["normalized"] = 5122, True      # the view's 32 bytes hold two i16 VEC4s and more
    _write_glb(doc, blob, path)
    h = H.Host(backend_path=MOCK)
    h.resize(64, 64)
    info = h.load_gltf(path)
    yield scene, h, info
    h.close()


def test_reader_makes_the_players_and_counts_what_it_skips(loaded):
    scene, h, info = loaded
    assert info["animations"] == 9 and info["animation_channels_skipped"] == 2
    keys = h.gltf_animation_keys()
    assert len(keys) == 9 and len(set(keys)) == 9
    want = _expected(scene.animations)
    for k, ch in zip(keys, want):
        st = h.animation_state(k)
        t = np.asarray(ch["times"], np.float32)
        assert st["duration"] == float(np.float32(t[-1] - t[0])) and st["speed"] == 1.0 / 1000.0 and st["loop_style"] == H.ANIM_LOOP      # last - first; AnimationPlayer::new
        assert len(h.animation_sample(k)) == np.asarray(ch["values"]).reshape(len(t), -1).shape[1]


def test_loaded_players_sample_like_players_inserted_from_the_same_arrays(loaded):
    scene, h, info = loaded
    direct = H.Host(backend_path=MOCK)
    populated = H.populate(direct, _scene())
    want = _expected(scene.animations)
    for k, ch in zip(h.gltf_animation_keys(), want):
        times = np.asarray(ch["times"], np.float32).astype(np.float64)      # f32 in the file, f64 in the clip
        args = (times, ch["values"], ch["interpolation"], ch.get("in_tangents"), ch.get("out_tangents"))
        if ch["path"] == "weights":
            dk = direct.animation_insert_morph(populated.mesh_keys[1], *args)
        else:
            dk = direct.animation_insert_transform(populated.node_keys[ch["node"]], ch["path"], *args)
        assert direct.animation_state(dk)["duration"] == h.animation_state(k)["duration"]
        for t in (0.0, 0.3, 0.5, 0.77, 1.25):
            h.animation_seek(k, t); direct.animation_seek(dk, t)
            assert h.animation_sample(k).tobytes() == direct.animation_sample(dk).tobytes(), (ch["node"], ch["path"], t)
    direct.close()


def test_first_sampler_per_node_and_path_wins(loaded):
    scene, h, info = loaded
    keys = h.gltf_animation_keys()
    h.animation_seek(keys[7], 1.0)      # the cube node's translation: the linear channel, not the cubic duplicate after it
    assert h.animation_sample(keys[7]).tobytes() == np.array([1.2, 0.4, 0.3], np.float32).tobytes()
    h.animation_seek(keys[1], 0.25)     # node 2's rotation: animation 0's, not animation 1's
    assert h.animation_sample(keys[1]).tobytes() == _q(0.1).tobytes()


def test_loaded_players_animate_the_loaded_scene(loaded):
    scene, h, info = loaded
    for k in h.gltf_animation_keys():
        h.animation_seek(k, 0.0)
    h.update_animations(500.0)
    h.update_transforms()
    for k in h.gltf_animation_keys():
        assert h.animation_state(k)["local_time"] == 0.5


def test_export_without_animations_is_byte_identical(tmp_path):
    """The exporter's output for a scene with animations=[] against the document it wrote before it knew the field: the same scene through a
    SceneDesc that has no such attribute at all."""
    scene = _scene()
    assert scene.animations == []
    doc, blob, pngs = gltf_export.scene_to_gltf(scene)
    bare = copy.copy(scene)
    del bare.__dict__["animations"]
    doc0, blob0, pngs0 = gltf_export.scene_to_gltf(bare)
    assert "animations" not in doc and json.dumps(doc) == json.dumps(doc0) and blob == blob0 and pngs == pngs0
    a, b = str(tmp_path / "a.glb"), str(tmp_path / "b.glb")
    gltf_export.write_glb(scene, a); gltf_export.write_glb(bare, b)
    assert open(a, "rb").read() == open(b, "rb").read()
    # ... and adding animations appends: every accessor and buffer view of the plain export keeps its index and its bytes
    scene.animations = _channels()
    doc2, blob2, _ = gltf_export.scene_to_gltf(scene)
    assert doc2["accessors"][:len(doc["accessors"])] == doc["accessors"] and doc2["bufferViews"][:len(doc["bufferViews"])] == doc["bufferViews"]
    assert blob2[:len(blob)] == blob and {k: v for k, v in doc2.items() if k not in ("animations", "accessors", "bufferViews", "buffers")} == {k: v for k, v in doc.items() if k not in ("accessors", "bufferViews", "buffers")}
