#!/usr/bin/env python3
"""What temporal anti-aliasing costs the post pass on one MI355X.

    python tools/taa_times.py [--iters 100] [--warmup 10] [--parent-tree DIR] [--out profiles/taa_times.txt]

At 1920x1080 and 3840x2160, single-sampled and MSAA x4, with the atrium's frame resident:

sync     the context runs on the caller's stream; `iters` display-only post passes of one rendered frame enqueued back to back between two device
         events, with TAA off, on with a still camera (identity: the four taps of neighbouring pixels coincide) and on with a moving one (the
         matrix of a 2-degree orbit step: the taps scatter), interleaved twice (the second round is reported).  Every pass of a frame resolves
         again from the same history into the same image, so on - off is k_taa_resolve<S> alone.  The host's time to enqueue a pass is printed too:
         where it is not clearly under the device time of the off run, that run waited for the host and on - off understates the kernel.
overlap  AWSM_CFG_OVERLAP_FRAMES; `iters` whole frames (geometry + opaque + display-only post pass) enqueued back to back with frame_flush and
         device-synchronised at the end: the frame period with TAA minus the period without.
parent   --parent-tree: a built checkout of the parent commit; its tools/post_times.py runs in a child process and its display-only figures are
         quoted beside this build's TAA-off figure.

Bytes the resolve needs per pixel, from the layout as built (the one-texel apron and the shared history taps are re-reads of lines that
neighbouring lanes and workgroups fetch too and are not counted): current image 8 + keys 8 S + history 8 + store 8 = 24 + 8 S.  The time those
bytes take at the 5 TB/s a streaming kernel reaches on this part is printed beside the measured time.
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from tests import helpers                                           # noqa: E402
from tests import taa_reference as tr                               # noqa: E402

STREAM_TBS = 5.0
MODES = ("off", "still", "moving")


def setup(dev, sc, model, lut, msaa):
    dev.resize(sc.width, sc.height, msaa)
    dev.upload_mirrors(model.mirrors())
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.set_stage_timers(False)


def orbit_matrix(model):
    """R of a 2-degree turn of the scene's camera about the vertical through the point five units ahead of it."""
    f = np.frombuffer(bytes(model.camera_bytes), np.float32)
    view, proj, inv_view = f[0:16].reshape(4, 4), f[16:32].reshape(4, 4), f[80:96].reshape(4, 4)
    eye = inv_view[3][:3].astype(np.float64)
    target = eye - 5.0 * inv_view[2][:3].astype(np.float64)
    import tests.grid_reference as gr
    prev_view = gr.look_at_rh(tr.orbit(eye, target, 2.0), target).astype(np.float32)
    return tr.reproject((prev_view, proj), view, proj)


def record_of(mode, R):
    return None if mode == "off" else dict(feedback=0.1, jitter_ndc=(0.0, 0.0), reproject=tr.IDENTITY if mode == "still" else R)


def time_sync(sc, model, lut, msaa, iters, warmup):
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    setup(dev, sc, model, lut, msaa)
    R = orbit_matrix(model)
    draws = model.collect_draws()
    out = {}
    for mode in MODES + MODES:
        rec = record_of(mode, R)
        for _ in range(2):      # two frames: the second one's resolve has a history
            dev.geometry_pass(draws)
            dev.opaque_pass()
            dev.set_taa(**rec) if rec else dev.set_taa(None)
            dev.post_pass(1)
            dev.frame_end()
        for _ in range(warmup):
            dev.post_pass(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        for _ in range(iters):
            dev.post_pass(1)
        out["host", mode] = (time.perf_counter() - t0) * 1e6 / iters
        b.record(stream)
        b.synchronize()
        out[mode] = a.elapsed_time(b) * 1000.0 / iters
        if rec:
            _, _, used = dev.read_taa()
            out["used", mode] = float(used.mean())
    dev.close()
    return out


def time_overlap(sc, model, lut, msaa, iters, warmup):
    dev = HipDevice(overlap_frames=True)
    setup(dev, sc, model, lut, msaa)
    R = orbit_matrix(model)
    draws = model.collect_draws()
    out = {}
    for mode in MODES + MODES:
        rec = record_of(mode, R)
        dev.set_taa(**rec) if rec else dev.set_taa(None)
        for k in range(warmup + iters):
            if k == warmup:
                dev.frame_end()
                t0 = time.perf_counter()
            dev.geometry_pass(draws)
            dev.opaque_pass()
            dev.post_pass(1)
            dev.frame_flush()
        dev.frame_end()
        out[mode] = (time.perf_counter() - t0) * 1e6 / iters
    dev.close()
    return out


def parent_display_only(tree, iters):
    """{scene label: us} of the parent's tools/post_times.py, run in a child process from its own tree."""
    tree = os.path.abspath(tree)
    text = subprocess.run([sys.executable, os.path.join(tree, "tools", "post_times.py"), "--iters", str(iters)], cwd=tree, check=True,
                          capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "AWSM_HIP_LIB"}).stdout
    out, label = {}, None
    for line in text.split("\n"):
        m = re.match(r"(\S+ \d+x\d+): display only", line)
        label = m.group(1) if m else label
        m = re.match(r"\s+display only\s+sync\s+([\d.]+) us", line)
        if m and label:
            out[label] = float(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lut = oracle_lib.brdf_lut(64, 64)
    lines = [f"# tools/taa_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: the atrium, display-only post pass, microseconds",
             "# taa = on - off = k_taa_resolve<S>; bytes = (24 + 8 S) per pixel; at-5-TB/s = the time those bytes alone would take; still: identity, moving: a 2-degree orbit step",
             "# host = the host's time to enqueue one pass (off / still); overlap = the overlapped frame period (geometry + opaque + post), off -> still / moving"]
    for (W, H) in ((1920, 1080), (3840, 2160)):
        sc = scenes.atrium_scene(W, H, detail=0.25, tex_scale=1 / 16)
        model = helpers.build_model(sc)
        for msaa in (0, 4):
            S = 4 if msaa else 1
            t = time_sync(sc, model, lut, msaa, a.iters, a.warmup)
            o = time_overlap(sc, model, lut, msaa, a.iters, a.warmup)
            mb = W * H * (24 + 8 * S) / 1e6
            floor_us = mb / STREAM_TBS
            still, moving = t["still"] - t["off"], t["moving"] - t["off"]
            host_bound = t["host", "off"] > 0.8 * t["off"]
            lines.append(f"{W}x{H} S = {S}: off {t['off']:7.1f}   still {t['still']:7.1f} (taa {still:+7.1f} us = {mb / max(still, 1e-3):5.2f} TB/s)   "
                         f"moving {t['moving']:7.1f} (taa {moving:+7.1f} us = {mb / max(moving, 1e-3):5.2f} TB/s, history used on {100 * t['used', 'moving']:.1f} %)   "
                         f"{mb:6.1f} MB, at-5-TB/s {floor_us:5.1f} us   host {t['host', 'off']:5.1f} / {t['host', 'still']:5.1f} us"
                         f"{'   OFF RUN HOST-BOUND: taa is a lower bound' if host_bound else ''}   "
                         f"overlap {o['off']:7.1f} -> {o['still']:7.1f} / {o['moving']:7.1f} us/frame")
            if W == 3840 and not msaa:
                off_4k = t["off"]
    if a.parent_tree:
        p = parent_display_only(a.parent_tree, a.iters)
        lines.append("parent commit, its own tools/post_times.py in a child process, display only, sync: "
                     + ", ".join(f"{k} {v:.1f} us" for k, v in p.items()) + f"; this build, TAA off, atrium 3840x2160: {off_4k:.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
