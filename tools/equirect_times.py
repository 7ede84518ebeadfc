#!/usr/bin/env python3
"""Device time of awsm_hip_env_cube_from_equirect on one MI355X.

    python tools/equirect_times.py [--reps 20] [--warmup 3] [--out profiles/equirect_times.txt]

Three rows, each timed twice per repetition — a pair of events on the context's stream around the calls (device time) and the host's clock from
before the first event to after the second has been waited for (wall time, which also holds whatever the host did meanwhile: staging a pageable
source, decoding the file) — median [min .. max] over the repetitions:
    2048 x 1024 RGBE into 512^2 (auto S = 1)          the projection and the apron rebuild, source copy included (8 MB: from the caller's memory)
    8192 x 4096 RGBE into 1024^2 (auto S = 2)         the same, a 134 MB source
    load_hdr end to end, 2048 x 1024 into 512^2       Host.env_cube_load_hdr of a run-length coded file in memory: decode on the host, create,
                                                      project, generate the chain — events around the call, so the host's decode time is inside
The cubes exist before the first two rows' timed calls, so nothing is allocated inside them.  Counted from the shapes alone: taps (6 N^2 S^2) and the
bytes they name (four pixels of 4 bytes each).  The times are recorded, not gated.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from awsm_renderer_amd import host as H                             # noqa: E402
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402
from tests import rgbe_files                                        # noqa: E402


def fmt(ms):
    return f"{statistics.median(ms):9.3f} ms [{min(ms):8.3f} .. {max(ms):8.3f}]"


def panorama(width, height):
    """uint8 [H, W, 4] RGBE: a sky gradient with a small bright sun, so that runs and literals both occur in a run-length coded file."""
    v = (np.arange(height) + 0.5)[:, None] / height
    u = (np.arange(width) + 0.5)[None, :] / width
    sky = np.stack([0.3 + 0.4 * v + 0.0 * u, 0.5 + 0.2 * v + 0.05 * np.sin(6.283185307179586 * u), 1.0 - 0.5 * v + 0.0 * u], axis=-1)
    sun = 5000.0 * np.exp(-((u - 0.6) ** 2 + (v - 0.3) ** 2) / 2e-5)
    return rgbe_files.float_to_rgbe(sky + sun[..., None])


def timed(stream, reps, warmup, call):
    ms, wall = [], []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return ms, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("equirect_times.py needs the GPU: there is nothing to time without one")
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    lines = [f"# tools/equirect_times.py --reps {a.reps} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: device events and the host's clock, median [min .. max]"]
    small = None
    for (w, h), n in (((2048, 1024), 512), ((8192, 4096), 1024)):
        pano = panorama(w, h)
        small = pano if small is None else small
        s = min(8, max(1, -(-w // (4 * n))))
        dev.env_cube_create(0, n, n.bit_length())
        ms, wall = timed(stream, a.reps, a.warmup, lambda: dev.env_cube_from_equirect(0, pano))
        taps = 6 * n * n * s * s
        t = statistics.median(ms) * 1e-3
        lines.append(f"{w} x {h} RGBE ({pano.nbytes / 1e6:.0f} MB) into {n}^2, S = {s}")
        lines.append(f"  copy + projection + apron, events {fmt(ms)}")
        lines.append(f"  the same, host clock              {fmt(wall)}")
        lines.append(f"  taps                      {taps:.4g} -> {taps / t:.3g} taps/s; bytes named by the taps {16.0 * taps:.4g} -> {16.0 * taps / t / 1e12:.3f} TB/s")
    dev.close()
    data = rgbe_files.write_hdr(small, "rle")
    host = H.Host(stream=stream.cuda_stream)
    ms, wall = timed(stream, a.reps, a.warmup, lambda: host.env_cube_load_hdr(0, data, 512))
    host.close()
    lines.append(f"load_hdr end to end: a run-length coded 2048 x 1024 file ({len(data) / 1e6:.1f} MB) into 512^2 with its chain")
    lines.append(f"  decode + create + projection + mips, events {fmt(ms)}")
    lines.append(f"  the same, host clock                        {fmt(wall)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
