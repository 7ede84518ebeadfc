#!/usr/bin/env python3
"""Animated frames on one MI355X: what playing animations costs, and where composing skin matrices on the device pays.

    python tools/animated_times.py [--frames 200] [--out profiles/animated_times.txt]

Rows, each a fresh Renderer with overlapped frames:
    configs[2] (skinned rig + morph cube, 1920x1080) static                          the frame loop without update_animations
    ... animated, skin matrices composed on the host
    ... animated, skin matrices composed on the device (Host.set_device_skin_posing)
    ... animated, host posing, AWSM_GEOMETRY_CACHE=0
    R small copies of the rig (18 joints each, R chosen for >= 10,000 joints), every joint moving, host posing / device posing
The players: rotation on three joints of the rig (linear, step ping-pong, cubic), translation on the cube's node, linear weights on the cube; in
the many-rigs rows one rotation player on each rig's root joint, so every joint of every rig moves every frame.
Per row: frames/s over `--frames` frames enqueued back to back (update_all + render, one synchronise at the end; host clock); then, over 9
synchronised frames, the median k_deform_transform time (AwsmFrameStats.ms_transform), the bytes uploaded per frame, the host time per frame in
update_animations + update_transforms, and the fraction of k_deform_transform workgroups that kept their cached outputs.  Recorded, not gated.
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from awsm_renderer_amd import scenes                                  # noqa: E402
from awsm_renderer_amd.host import ANIM_LOOP_NONE, ANIM_PING_PONG, Renderer      # noqa: E402
from awsm_renderer_amd.scene_desc import SkinDesc                     # noqa: E402
from awsm_renderer_amd.scenes import quat_axis_angle                  # noqa: E402

JOINTS = 18
DT = 16.6


def q(a):
    return np.array(quat_axis_angle((0, 0, 1), a), np.float32)


def rig_players(r):
    h, nk = r.host, r.keys.node_keys
    times = [0.0, 0.4, 1.0]
    tan = np.array([[0, 0, 0.2, 0], [0, 0, -0.1, 0.05], [0, 0, 0.3, 0]], np.float32)
    h.animation_insert_transform(nk[3], "rotation", times, [q(-0.3), q(0.2), q(0.5)])
    k = h.animation_insert_transform(nk[7], "rotation", times, [q(0.1), q(-0.25), q(0.3)], "step")
    h.animation_set_playback(k, loop_style=ANIM_PING_PONG)
    h.animation_insert_transform(nk[12], "rotation", times, [q(0.0), q(0.35), q(-0.2)], "cubic", tan, -tan)
    h.animation_insert_transform(nk[JOINTS + 2], "translation", [0.0, 1.0], [[1.6, 0, 0], [1.45, 0.25, 0.1]])
    h.animation_insert_morph(r.keys.mesh_keys[1], [0.0, 0.5, 1.0], [[0, 0], [1, 0.25], [0.2, 0.9]])


def many_rigs(copies):
    """`copies` small rigs (tube of 8 x 12 quads, 18 joints) side by side; returns the scene and the node index of every rig's root joint."""
    one = scenes.skinned_morph_scene(1920, 1080, around=8, along=12, tex_size=16)
    rig_nodes = one.nodes[:JOINTS + 2]      # rig root, 18 joints, the tube's node
    sc = copy.copy(one)
    sc.nodes, sc.skins, roots = [], [], []
    per_row = 32
    for c in range(copies):
        base = len(sc.nodes)
        for i, n in enumerate(rig_nodes):
            m = copy.copy(n)
            m.parent = None if n.parent is None else n.parent + base
            if i == 0:
                m.translation = ((c % per_row - per_row / 2) * 1.0, 0.0, -(c // per_row) * 1.5 - 6.0)
            if m.skin is not None:
                m.skin = c
            sc.nodes.append(m)
        sc.skins.append(SkinDesc(joints=[j + base for j in one.skins[0].joints], inverse_bind=one.skins[0].inverse_bind))
        roots.append(base + 1)
    return sc, roots


def measure(name, scene, frames, players=None, device_posing=False, cache=True):
    os.environ["AWSM_GEOMETRY_CACHE"] = "1" if cache else "0"
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    r = Renderer(scene, stream=stream.cuda_stream, lut_size=256, overlap_frames=True)
    r.host.set_device_skin_posing(device_posing)
    if players:
        players(r)
    step = (lambda: r.update_all(DT)) if players else r.update
    for _ in range(10):
        step(); r.render(sync=False)
    r.render(sync=True)
    t0 = time.perf_counter()
    for _ in range(frames):
        step(); r.render(sync=False)
    stream.synchronize()
    fps = frames / (time.perf_counter() - t0)
    ms_t, up, host_us, hit = [], [], [], []
    for _ in range(9):
        h0 = time.perf_counter()
        if players:
            r.host.update_animations(DT)
        r.host.update_transforms()
        host_us.append((time.perf_counter() - h0) * 1e6)
        r.host.camera_update(scene.view, scene.proj, scene.camera_position)
        st = r.render(sync=True)
        ms_t.append(st["ms_transform"]); up.append(r.host.upload_bytes_last_frame())
        hit.append(st["geometry_cache_blocks"] / max(1, st["geometry_blocks"]))
    posed = len(r.host.skin_pose_ids_last_frame())
    r.close()
    return (f"{name:<58} {fps:9.1f} frames/s   k_deform_transform {statistics.median(ms_t) * 1e3:8.1f} us   upload {int(statistics.median(up)):9d} B/frame   "
            f"host update {statistics.median(host_us):9.1f} us/frame   cache hits {statistics.median(hit):5.3f}   joints posed on the device {posed}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("animated_times.py needs the GPU: there is nothing to time without one")
    lines = [f"# tools/animated_times.py --frames {a.frames} on {torch.cuda.get_device_name(0)}: {a.frames} overlapped frames for frames/s, medians of 9 synchronised frames for the rest"]
    cfg2 = lambda: scenes.skinned_morph_scene(1920, 1080)      # noqa: E731
    lines.append(measure("configs[2] static", cfg2(), a.frames))
    lines.append(measure("configs[2] animated, host posing", cfg2(), a.frames, rig_players))
    lines.append(measure("configs[2] animated, device posing", cfg2(), a.frames, rig_players, device_posing=True))
    lines.append(measure("configs[2] animated, host posing, AWSM_GEOMETRY_CACHE=0", cfg2(), a.frames, rig_players, cache=False))
    copies = -(-10000 // JOINTS)
    sc, roots = many_rigs(copies)

    def root_players(r):
        for n in roots:
            r.host.animation_insert_transform(r.keys.node_keys[n], "rotation", [0.0, 0.5, 1.0], [q(-0.2), q(0.2), q(-0.2)])

    for posing in (False, True):
        lines.append(measure(f"{copies} small rigs ({copies * JOINTS} joints), {'device' if posing else 'host'} posing", sc, a.frames, root_players, device_posing=posing))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
