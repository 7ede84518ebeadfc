#!/usr/bin/env python3
"""Device time of awsm_hip_env_cube_filter on one MI355X.

    python tools/ibl_bake_times.py [--reps 20] [--warmup 3] [--out profiles/ibl_bake_times.txt] [--no-frame]

Two bakes, 1024 samples per texel, each the pair of calls Host.env_bake_ibl makes:
    skybox 256^2  -> prefiltered 256^2, full chain (9 levels) + irradiance 32^2
    skybox 1024^2 -> prefiltered 512^2, full chain (10 levels) + irradiance 32^2
The destinations exist before the timed calls, so nothing is allocated inside them.  Every repetition is timed with a pair of events on the
context's stream around the two calls (table upload, level-0 kernel, filter kernel, apron rebuild, twice); median [min .. max] over the
repetitions.  Counted from the shapes alone: the samples (texels of a level times the level's table entries — those with N.L > 0) and the bytes
their taps name (two levels x four RGBA16F texels = 64 B per sample; lanes of one texel sample inside one lobe, so most of these are cache
hits, not HBM traffic).  The last line is one frame of `bench.py --config 2` on the same device, for scale (a child process; --no-frame skips it).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from awsm_renderer_amd.hip_backend import HipDevice                 # noqa: E402

SAMPLES = 1024
HBM_BYTES_PER_S = 8.0e12            # the MI355X's specified peak
LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9      # 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz: one f32 VALU operation per lane and clock


def ggx_entries(level: int, levels: int, samples: int) -> int:
    """Entries of a level's table: Hammersley points whose N.L = 2 c^2 - 1 is positive (csrc/env_filter_table.hpp)."""
    i = np.arange(samples, dtype=np.uint64)
    rev = np.zeros(samples, dtype=np.uint64)
    for b in range(32):
        rev |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    y = rev.astype(np.float64) * 2.0 ** -32
    a2 = (level / (levels - 1)) ** 4
    c2 = (1.0 - y) / (1.0 + (a2 - 1.0) * y)
    return int((2.0 * c2 - 1.0 > 0.0).sum())


def fmt(ms):
    return f"{statistics.median(ms):9.3f} ms [{min(ms):8.3f} .. {max(ms):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-frame", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ibl_bake_times.py needs the GPU: there is nothing to time without one")
    stream = torch.cuda.Stream()
    dev = HipDevice(stream=stream.cuda_stream)
    lines = [f"# tools/ibl_bake_times.py --reps {a.reps} --warmup {a.warmup} on {torch.cuda.get_device_name(0)}: device time (events), median [min .. max]"]
    rng = np.random.default_rng(11)
    for ns, size in ((256, 256), (1024, 512)):
        mips = size.bit_length()
        dev.env_cube_create(0, ns, ns.bit_length())
        dev.env_cube_write_all_faces(0, 0, rng.uniform(0.05, 10.0, size=(6, ns, ns, 4)).astype(np.float16))
        dev.env_cube_generate_mips(0)

        def bake():
            dev.env_cube_filter(0, 1, "ggx", size, mips, SAMPLES)
            dev.env_cube_filter(0, 2, "lambert", 32, 1, SAMPLES)

        ms = []
        for k in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            bake()
            e1.record(stream)
            e1.synchronize()
            if k >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        samples = sum(6 * max(size >> l, 1) ** 2 * ggx_entries(l, mips, SAMPLES) for l in range(1, mips)) + 6 * 32 * 32 * SAMPLES
        t = statistics.median(ms) * 1e-3
        rate, tap_bytes = samples / t, 64.0 * samples / t
        src_bytes = sum(6 * max(ns >> l, 1) ** 2 for l in range(ns.bit_length())) * 8
        lines.append(f"skybox {ns}^2 -> prefiltered {size}^2 x {mips} levels + irradiance 32^2, {SAMPLES} samples per texel")
        lines.append(f"  bake                      {fmt(ms)}")
        lines.append(f"  samples                   {samples:.4g} -> {rate:.3g} samples/s")
        lines.append(f"  bytes named by the taps   {64.0 * samples:.4g} (64 B per sample) -> {tap_bytes / 1e12:.2f} TB/s; the source chain is {src_bytes / 1e6:.1f} MB")
        lines.append(f"  against the bounds        taps / HBM peak (8 TB/s) = {tap_bytes / HBM_BYTES_PER_S:.2f}; "
                     f"f32 lane operations available per sample = {LANE_OPS_PER_S / rate:.0f}")
        lines.append("                            (a ratio over 1 against HBM means the taps are served by the caches; the kernel spends on the order of 150 lane "
                     "operations per sample, so a figure near that says VALU-bound, a much larger one says latency- or cache-bound)")
    dev.close()
    if not a.no_frame:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2", "--steps", "100", "--warmup", "20", "--no-cpu-baseline"],
                           capture_output=True, text=True, timeout=900)
        frame = None
        for ln in p.stdout.splitlines():
            if ln.startswith("{"):
                frame = json.loads(ln).get("ms_per_step")
        lines.append(f"for scale: one frame of bench.py --config 2 on this device = {frame} ms" if frame is not None else
                     f"for scale: bench.py --config 2 gave no result (exit {p.returncode})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
