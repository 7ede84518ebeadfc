#!/usr/bin/env python3
"""What the editor's ground grid costs the world transparent pass on one MI355X.

    python tools/grid_times.py [--iters 200] [--warmup 20] [--out profiles/grid_times.txt]

At 3840x2160, single-sampled and MSAA x4, grid off against grid on, after a warm-up:
  empty pass   the atrium's keys and opaque image resident, awsm_hip_transparent_pass with n_draws = 0: two small fills, k_bin_scan, k_forward_cover over
               empty tiles and the blend kernel — k_forward_blend<S> (off) or k_forward_blend_grid<S> (on).  Device events around `iters` passes
               enqueued back to back on one stream; everything but the blend kernel is the same work in both, so the difference of the two is
               k_forward_blend_grid<S> minus k_forward_blend<S>.
  fragments    transparent_scene's opaque backdrop resident and its transparent draws submitted (fragment lists of that class), the same way.
  kernels      --kernel-stats DIR: the two blend kernels' own average times, read from the kernel_stats.csv a
               `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/grid_times.py ...` run of this script left in DIR
               (all instantiations and both scenes together), appended to the table.
  overlapped   AWSM_CFG_OVERLAP_FRAMES: whole frames (geometry + opaque + empty transparent pass) enqueued back to back with frame_flush, host clock
               over `iters` frames -> frames per second with the grid off and on.
Bytes moved per pixel by the blend kernel: 8 S key bytes are read by the grid variant only (the depth test), 8 opaque bytes + 4 fragment-list head
bytes read and 8 composite bytes written by both.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from tests import helpers                                           # noqa: E402

W, H = 3840, 2160


def setup(dev, sc, model, lut, msaa):
    dev.resize(sc.width, sc.height, msaa)
    dev.upload_mirrors(model.mirrors())
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.set_stage_timers(False)


def time_passes(sc, model, lut, msaa, transparent, iters, warmup):
    """-> {grid on?: microseconds per transparent pass}"""
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    setup(dev, sc, model, lut, msaa)
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    draws = dev.make_draws(transparent)
    dev.transparent_pass(draws, len(transparent))
    dev.frame_end()                                     # the pass's lists are sized now
    out = {}
    for on in (False, True, False, True):               # twice, interleaved: the second pair is what is reported
        dev.set_editor_grid(True if on else None)
        for _ in range(warmup):
            dev.transparent_pass(draws, len(transparent))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(iters):
            dev.transparent_pass(draws, len(transparent))
        b.record(stream)
        b.synchronize()
        out[on] = a.elapsed_time(b) * 1000.0 / iters
    dev.close()
    return out


def time_overlap(sc, model, lut, msaa, iters, warmup):
    """-> {grid on?: microseconds per overlapped frame}"""
    dev = HipDevice(overlap_frames=True)
    setup(dev, sc, model, lut, msaa)
    draws = dev.make_draws(model.collect_draws())
    n = len(model.collect_draws())
    out = {}
    for on in (False, True, False, True):
        dev.set_editor_grid(True if on else None)
        for k in range(warmup + iters):
            if k == warmup:
                dev.frame_end()
                t0 = time.perf_counter()
            dev.geometry_pass(draws, n)
            dev.opaque_pass()
            dev.transparent_pass([])
            dev.frame_flush()
        dev.frame_end()
        out[on] = (time.perf_counter() - t0) * 1e6 / iters
    dev.close()
    return out


def kernel_stats(directory, out):
    import csv
    import glob
    lines = ["# per kernel, rocprofv3 --kernel-trace --stats over a run of this script (empty passes and fragment passes, 3840x2160): calls, average microseconds"]
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_forward_blend" in r["Name"] or "k_forward_cover" in r["Name"]:
                lines.append("  %-44s calls %6s   avg %8.1f us" % (r["Name"].split("(")[0].replace("void awsm::", ""), r["Calls"], float(r["AverageNs"]) / 1e3))
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="append the blend kernels' times from a rocprofv3 --stats run left in DIR; measures nothing")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    lut = oracle_lib.brdf_lut(64, 64)
    lines = [f"# tools/grid_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: {W}x{H}, microseconds"]
    atrium = scenes.atrium_scene(W, H, detail=0.25, tex_scale=1 / 16)
    atrium_model = helpers.build_model(atrium)
    tscene = scenes.transparent_scene(W, H, tex_size=64)
    tmodel = helpers.build_model(tscene)
    tmodel.collect_draws()
    tdraws = tmodel.collect_transparent_draws()
    px = W * H
    for msaa in (0, 4):
        S = 4 if msaa else 1
        e = time_passes(atrium, atrium_model, lut, msaa, [], a.iters, a.warmup)
        f = time_passes(tscene, tmodel, lut, msaa, tdraws, a.iters, a.warmup)
        o = time_overlap(atrium, atrium_model, lut, msaa, max(20, a.iters // 4), a.warmup)
        mb_off, mb_on = px * 20 / 1e6, px * (20 + 8 * S) / 1e6
        lines.append(f"S = {S}: the blend kernel moves {mb_off:.1f} MB (grid off), {mb_on:.1f} MB (grid on)")
        lines.append(f"  empty pass (atrium keys)        off {e[False]:8.1f}   on {e[True]:8.1f}   grid = k_forward_blend_grid<{S}> - k_forward_blend<{S}> = {e[True] - e[False]:+7.1f} us"
                     f" = {(mb_on - mb_off) / max(e[True] - e[False], 1e-3):.2f} TB/s for the {mb_on - mb_off:.1f} MB of keys it adds")
        lines.append(f"  transparent_scene fragments     off {f[False]:8.1f}   on {f[True]:8.1f}   grid = {f[True] - f[False]:+7.1f} us")
        lines.append(f"  overlapped frame (atrium)       off {o[False]:8.1f} us = {1e6 / o[False]:7.1f} fps   on {o[True]:8.1f} us = {1e6 / o[True]:7.1f} fps")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
