#!/usr/bin/env python3
"""What the pick queries cost on one MI355X.

    python tools/pick_times.py [--iters 50] [--warmup 5] [--detail 1.0] [--out profiles/pick_times.txt]

The bench frame (the atrium at 3840x2160, detail 1.0; small textures: no query samples one) after one whole frame — geometry, opaque and world
transparent pass, awsm_hip_frame_end — with its keys and fragment lists resident.  Every query is synchronous (it waits for every stream, launches,
copies its answer back), so a call is timed with the host's clock around it: the figure is the call as a caller sees it, launch and copy included.
Each row is the median and the least of `iters` calls after `warmup` (a tenth as many for the host-side alternative); the rows alternate over two
rounds and the second is reported.  The bench scene has no transparent mesh — with the flag its rows show the flag's fixed cost — so the same
rows follow for scenes.transparent_scene at the same size, which has.

    pick / pick_ex                  one pixel at the frame's centre
    pick_rect                       64 x 64 at the centre, a quarter of the frame, the whole frame; without and with AWSM_PICK_TRANSPARENT
    read_visibility + numpy.unique  the only way to the same answer before: the whole key image to the host (8 bytes a pixel), then a unique
                                    over the rectangle's triangle ranks on the host (the draw lookup that would follow is not timed)
"""
import argparse
import os
import statistics
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


def measure(name, sc, lut, a):
    model = helpers.build_model(sc)
    dev, stats = helpers.hip_frame(model, lut, dev=HipDevice(), transparent=True)
    dev.set_stage_timers(False)
    n_world, n_tr = len(model.collect_draws()), len(model.collect_transparent_draws())
    cx, cy = W // 2, H // 2
    rects = [("64 x 64", (cx - 32, cy - 32, cx + 32, cy + 32)), ("quarter frame", (W // 4, H // 4, W // 4 + W // 2, H // 4 + H // 2)), ("whole frame", (0, 0, W, H))]

    def unique_on_host(r):
        keys = dev.read_visibility()[r[1]:r[3], r[0]:r[2]]
        return np.unique(keys & np.uint64(0xFFFFFFFF))

    rows = [("pick (keys only, awsm_hip_pick)", lambda: dev.pick(cx, cy)), ("pick_ex", lambda: dev.pick_ex(cx, cy)), ("pick_ex, transparent", lambda: dev.pick_ex(cx, cy, True))]
    for label, r in rects:
        rows.append(("pick_rect %s" % label, lambda r=r: dev.pick_rect(*r)))
        rows.append(("pick_rect %s, transparent" % label, lambda r=r: dev.pick_rect(*r, transparent=True)))
        rows.append(("read_visibility + numpy.unique %s" % label, lambda r=r: unique_on_host(r)))
    out = {}
    for _ in range(2):                                  # twice: the second round is what is reported
        for label, call in rows:
            slow = label.startswith("read_visibility")      # tens of milliseconds to a second per call: a tenth of the calls
            for _ in range(1 if slow else a.warmup):
                call()
            t = []
            for _ in range(max(3, a.iters // 10) if slow else a.iters):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e6)
            out[label] = (statistics.median(t), min(t))
    found = {label: dev.pick_rect(*r, transparent=True)[1] for label, r in rects}
    dev.close()
    lines = [f"# tools/pick_times.py --iters {a.iters} --warmup {a.warmup} --detail {a.detail} on {torch.cuda.get_device_name(0)}: {name} at {W}x{H}, {n_world} world draws"
             f" and {n_tr} transparent draws ({stats['forward_fragment_slots']} fragment slots); microseconds per synchronous call, host clock, median / least of {a.iters}",
             "# distinct (layer, mesh) pairs with the flag: " + ", ".join("%s %d" % kv for kv in found.items())]
    lines += ["%-52s %10.1f / %10.1f us" % (label, *out[label]) for label, _ in rows]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--detail", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pick_times.py measures on the GPU: none is visible")
    lut = oracle_lib.brdf_lut(64, 64)
    lines = []
    # the bench scene has no transparent mesh (with the flag its rows show the flag's fixed cost: the counters read back); scenes.transparent_scene has
    for name, sc in (("the atrium", scenes.atrium_scene(W, H, detail=a.detail, tex_scale=1 / 16)), ("scenes.transparent_scene", scenes.transparent_scene(W, H, tex_size=64))):
        lines += measure(name, sc, lut, a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
