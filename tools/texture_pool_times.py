#!/usr/bin/env python3
"""Times of the run-time texture-pool entries on one MI355X against the path the library offered before them.

    python tools/texture_pool_times.py [--reps 10] [--warmup 2] [--out profiles/texture_pool_times.txt]

One image added to a resident array (1024^2 with 16 layers, 2048^2 with 4 layers; full chains):
    write_layers + generate_mips_layers   the new image alone, into a layer the array has room for (growth doubles, so most inserts find room)
    resize_layers                         the growth step itself: 16 -> 32 / 4 -> 8 layers, every level moved on the device
    baseline                              awsm_hip_texture_array_upload of the whole array with the new image + awsm_hip_texture_array_generate_mips:
                                          what an insert cost before
and k_tex_mips (generate_mips_layers over all layers) against the per-level launches (generate_mips) on a whole 2048^2 x 8 array.
Every repetition is a host clock around the call(s) and a synchronise of the context's stream, so a time is what a caller waits for; the mip
entries are also given as device time (events around `reps` calls back to back).  Median [min .. max], microseconds.
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


def timed(fn, stream, reps, warmup, before=None):
    out = []
    for k in range(warmup + reps):
        if before:
            before()
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e6)
    return out


def device_us(fn, stream, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps


def fmt(us):
    return f"{statistics.median(us):10.1f} [{min(us):9.1f} .. {max(us):9.1f}]"


def chains_equal(dev, a, b, layers):
    mips = dev.texture_array_info(a)[3]
    return all((dev.texture_array_read_level(a, l)[:layers] == dev.texture_array_read_level(b, l)[:layers]).all() for l in range(mips))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("texture_pool_times.py needs the GPU: there is nothing to time without one")
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    lines = [f"# tools/texture_pool_times.py --reps {a.reps} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: microseconds, median [min .. max]"]
    rng = np.random.default_rng(9)
    for size, layers in ((1024, 16), (2048, 4)):
        mips = size.bit_length()
        kinds = [l % 3 for l in range(layers + 1)]
        texels = rng.integers(0, 256, size=(layers + 1, size, size, 4), dtype=np.uint8)
        new = np.ascontiguousarray(texels[layers:])
        # array 0: resident with `layers` images and room for twice as many; array 1: the baseline's
        dev.texture_array_upload(0, texels[:layers], mips)
        dev.texture_array_generate_mips(0, kinds[:layers])
        rows = {}
        rows["resize_layers (x2)"] = timed(lambda: dev.texture_array_resize_layers(0, 2 * layers), stream, 1, 0)
        insert = lambda: (dev.texture_array_write_layers(0, layers, new, mip_kind=kinds[layers]), dev.texture_array_generate_mips_layers(0, layers, 1))      # noqa: E731
        rows["write_layers + generate_mips_layers (1 image)"] = timed(insert, stream, a.reps, a.warmup)
        rows["  write_layers alone"] = timed(lambda: dev.texture_array_write_layers(0, layers, new, mip_kind=kinds[layers]), stream, a.reps, a.warmup)
        mips_dev = device_us(lambda: dev.texture_array_generate_mips_layers(0, layers, 1), stream, a.reps)
        baseline = lambda: (dev.texture_array_upload(1, texels, mips), dev.texture_array_generate_mips(1, kinds))      # noqa: E731
        rows["baseline: upload of the whole array + generate_mips"] = timed(baseline, stream, a.reps, a.warmup)
        same = chains_equal(dev, 0, 1, layers + 1)      # faster and different is not faster
        lines.append(f"{size}^2, {layers} layers resident + 1 new, {mips} levels; new path equals the baseline bit for bit: {same}")
        for name, us in rows.items():
            lines.append(f"  {name:52s} {fmt(us)}")
        lines.append(f"  {'generate_mips_layers of the image, device time':52s} {mips_dev:10.1f}")
        ratio = statistics.median(rows["baseline: upload of the whole array + generate_mips"]) / statistics.median(rows["write_layers + generate_mips_layers (1 image)"])
        lines.append(f"  baseline / new path (medians): {ratio:.1f} x; bytes over the bus {new.nbytes / 1e6:.1f} MB against {texels.nbytes / 1e6:.1f} MB")
    # k_tex_mips against the per-level launches, a whole array
    size, layers = 2048, 8
    mips = size.bit_length()
    kinds = [l % 3 for l in range(layers)]
    texels = rng.integers(0, 256, size=(layers, size, size, 4), dtype=np.uint8)
    dev.texture_array_upload(0, texels, mips)
    dev.texture_array_upload(1, texels, mips)
    for l in range(layers):      # record the kinds of array 0 where generate_mips_layers reads them
        dev.texture_array_write_layers(0, l, texels[l: l + 1], mip_kind=kinds[l])
    per_level = timed(lambda: dev.texture_array_generate_mips(1, kinds), stream, a.reps, a.warmup)
    fused = timed(lambda: dev.texture_array_generate_mips_layers(0, 0, layers), stream, a.reps, a.warmup)
    per_level_dev = device_us(lambda: dev.texture_array_generate_mips(1, kinds), stream, a.reps)      # includes that entry's own stream synchronise
    fused_dev = device_us(lambda: dev.texture_array_generate_mips_layers(0, 0, layers), stream, a.reps)
    same = chains_equal(dev, 0, 1, layers)
    chain_bytes = sum(layers * max(size >> l, 1) ** 2 * 4 for l in range(mips))
    lines.append(f"{size}^2 x {layers} layers, whole chain ({chain_bytes / 1e6:.0f} MB); k_tex_mips equals the per-level launches bit for bit: {same}")
    lines.append(f"  {'generate_mips (one launch per level, 11 launches)':52s} {fmt(per_level)}   between events: {per_level_dev:10.1f}")
    lines.append(f"  {'generate_mips_layers (k_tex_mips, 3 launches)':52s} {fmt(fused)}   between events: {fused_dev:10.1f}   = {chain_bytes / fused_dev / 1e6:.2f} TB/s of chain read + written")
    dev.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
