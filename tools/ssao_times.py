#!/usr/bin/env python3
"""What screen-space ambient occlusion costs the opaque pass on one MI355X.

    python tools/ssao_times.py [--iters 100] [--warmup 10] [--out profiles/ssao_times.txt]

At 1920x1080 and 3840x2160, single-sampled and MSAA x4, with the atrium's keys resident: `iters` opaque passes enqueued back to back on one stream
between two device events, synchronised at the end, with SSAO off and on, interleaved twice (the second pair is reported).  The shading kernels do
the same work in both, so the difference is k_ssao_ao<S> + k_ssao_apply — provided the device, not the host's enqueue rate, bounds both runs.  The
host's own time to enqueue a pass is measured in the same loop and printed: where it is not clearly below the device time of the SSAO-off pass, that
run waited for the host, and on - off understates the two kernels by up to the idle time of the off run (the row says so).  The kernels have not been
bracketed by events of their own.

Bytes the algorithm needs per pixel, from the layout as built (the staged aprons are re-reads of lines other workgroups fetch too and are not counted):
  k_ssao_ao<S>   8 S key bytes read; A and view z written, 4 bytes each
  k_ssao_apply   A and view z read, 4 bytes each; A' written, 4 bytes; the RGBA16F opaque image read and written, 8 bytes each
= 8 S + 36 bytes.  The time those bytes take at the 5 TB/s a streaming kernel reaches on this part is printed beside the measured time: the ratio says
which of bytes or arithmetic bounds the pair.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd import scenes                                # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from oracle import oracle_lib                                       # noqa: E402
from tests import helpers                                           # noqa: E402

STREAM_TBS = 5.0


def time_passes(sc, model, lut, msaa, iters, warmup):
    """-> {SSAO on?: microseconds per opaque pass}"""
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    dev.resize(sc.width, sc.height, msaa)
    dev.upload_mirrors(model.mirrors())
    for i, t in enumerate(model.texture_arrays()):
        dev.texture_array_upload(i, t["texels"])
    for i, s in enumerate(sc.samplers):
        dev.sampler_set(i, s)
    dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib.lut_rg_to_rgba16f(lut))
    dev.set_stage_timers(False)
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    dev.frame_end()
    out = {}
    for on in (False, True, False, True):
        dev.set_ssao(True if on else None)
        for _ in range(warmup):
            dev.opaque_pass()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        t0 = time.perf_counter()
        for _ in range(iters):
            dev.opaque_pass()
        out["host", on] = (time.perf_counter() - t0) * 1e6 / iters      # before the synchronisation: the enqueue calls alone
        b.record(stream)
        b.synchronize()
        out[on] = a.elapsed_time(b) * 1000.0 / iters
    if True in out:
        raw, smoothed, _ = dev.read_ssao()
        out["occluded"] = float((smoothed < 0.95).mean())
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lut = oracle_lib.brdf_lut(64, 64)
    lines = [f"# tools/ssao_times.py --iters {a.iters} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: the atrium, microseconds per opaque pass",
             "# ssao = on - off = k_ssao_ao<S> + k_ssao_apply; bytes = (8 S + 36) per pixel; at-5-TB/s = the time those bytes alone would take",
             "# host = the host's time to enqueue one pass (off / on); an off run whose host time is not under 80 % of its device time waited for the host,",
             "# and ssao then understates the two kernels by up to the difference (marked)"]
    for (W, H) in ((1920, 1080), (3840, 2160)):
        sc = scenes.atrium_scene(W, H, detail=0.25, tex_scale=1 / 16)
        model = helpers.build_model(sc)
        for msaa in (0, 4):
            S = 4 if msaa else 1
            t = time_passes(sc, model, lut, msaa, a.iters, a.warmup)
            mb = W * H * (8 * S + 36) / 1e6
            ssao = t[True] - t[False]
            floor_us = mb / STREAM_TBS
            bound = "arithmetic and LDS, not bytes" if ssao > 2.0 * floor_us else "bytes"
            host_bound = t["host", False] > 0.8 * t[False]
            lines.append(f"{W}x{H} S = {S}: off {t[False]:8.1f}   on {t[True]:8.1f}   ssao {ssao:+8.1f} us   {mb:7.1f} MB = {mb / max(ssao, 1e-3):5.2f} TB/s, at-5-TB/s {floor_us:6.1f} us"
                         f" -> bound by {bound}   host {t['host', False]:5.1f} / {t['host', True]:5.1f} us"
                         f"{'   OFF RUN HOST-BOUND: ssao is a lower bound' if host_bound else ''}   (A' < 0.95 on {100 * t['occluded']:.1f} % of the frame)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
