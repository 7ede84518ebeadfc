#!/usr/bin/env python3
"""Times of the run-time environment-cube entries on one MI355X against what the library offered before them.

    python tools/env_cube_times.py [--reps 20] [--warmup 3] [--out profiles/env_cube_times.txt]

At 256^2 and 1024^2 (RGBA16F source, full chain):
    write_all_faces      level 0 of all six faces, in place
    generate_mips        levels 1.. on the device
    one face + mips      one face of level 0, then the chain
    baseline             the mip chain in numpy on the host + awsm_hip_env_cube_upload of the whole cube (a full re-upload with a stream
                         synchronise; the only way in before); its two parts are listed too
Every repetition is a host clock around the call(s) and a synchronise of the context's stream, so a time is what a caller waits for, copies and
launch overheads included; generate_mips is also given as device time (events around `reps` calls back to back).  Median [min .. max] over the
repetitions, microseconds.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402


def numpy_chain(level0: np.ndarray):
    """The chain the device makes, on the host: 2x2 sums in f32 from +0.0, * 0.25, rounded to f16, level by level."""
    chain = [level0]
    while chain[-1].shape[1] > 1:
        s = chain[-1].astype(np.float32)
        d = s.shape[1] >> 1
        acc = np.zeros((6, d, d, 4), dtype=np.float32)
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            acc = acc + s[:, dy:2 * d:2, dx:2 * d:2]
        chain.append((acc * np.float32(0.25)).astype(np.float16))
    return chain


def timed(fn, stream, reps, warmup):
    out = []
    for k in range(warmup + reps):
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return out


def fmt(us):
    return f"{statistics.median(us):10.1f} [{min(us):9.1f} .. {max(us):9.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("env_cube_times.py needs the GPU: there is nothing to time without one")
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    lines = [f"# tools/env_cube_times.py --reps {a.reps} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: microseconds, median [min .. max]"]
    rng = np.random.default_rng(7)
    for size in (256, 1024):
        mips = size.bit_length()
        level0 = rng.uniform(0.0, 4.0, size=(6, size, size, 4)).astype(np.float16)
        face = np.ascontiguousarray(level0[2])
        dev.env_cube_create(0, size, mips)
        rows = {}
        rows["write_all_faces (level 0)"] = timed(lambda: dev.env_cube_write_all_faces(0, 0, level0), stream, a.reps, a.warmup)
        rows["generate_mips"] = timed(lambda: dev.env_cube_generate_mips(0), stream, a.reps, a.warmup)
        rows["write_all_faces + generate_mips"] = timed(lambda: (dev.env_cube_write_all_faces(0, 0, level0), dev.env_cube_generate_mips(0)), stream, a.reps, a.warmup)
        rows["one face + generate_mips"] = timed(lambda: (dev.env_cube_write_face(0, 2, 0, face), dev.env_cube_generate_mips(0)), stream, a.reps, a.warmup)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream.synchronize()
        e0.record(stream)
        for _ in range(a.reps):
            dev.env_cube_generate_mips(0)
        e1.record(stream)
        e1.synchronize()
        device_us = e0.elapsed_time(e1) * 1000.0 / a.reps
        got = [dev.env_cube_read_level(0, l) for l in range(mips)]
        chain = numpy_chain(level0)
        same = all((g.view(np.uint16) == w.view(np.uint16)).all() for g, w in zip(got, chain))      # faster and different is not faster
        host_chain = []
        for k in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            chain = numpy_chain(level0)
            host_chain.append((time.perf_counter() - t0) * 1e6)
        rows["baseline: env_cube_upload of the chain"] = timed(lambda: dev.env_cube_upload(0, chain), stream, a.reps, a.warmup)
        rows["baseline: numpy chain on the host"] = host_chain
        total = statistics.median(host_chain) + statistics.median(rows["baseline: env_cube_upload of the chain"])
        texels = sum(6 * max(size >> l, 1) ** 2 for l in range(mips))
        lines.append(f"{size}^2, {mips} levels, {texels * 8 / 1e6:.1f} MB chain; device chain equals the numpy chain bit for bit: {same}")
        for name, us in rows.items():
            lines.append(f"  {name:40s} {fmt(us)}")
        lines.append(f"  {'generate_mips, device time (events)':40s} {device_us:10.1f}   = {(6 * size * size * 8 + (texels - 6 * size * size) * 8) / device_us / 1e6:.2f} TB/s of chain read + written, apron rebuild included")
        lines.append(f"  {'baseline total (chain + upload, medians)':40s} {total:10.1f}   = {total / statistics.median(rows['write_all_faces + generate_mips']):.1f} x write_all_faces + generate_mips, "
                     f"{total / statistics.median(rows['one face + generate_mips']):.1f} x one face + generate_mips")
    dev.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
