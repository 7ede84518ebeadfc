"""driver.py — the launch trace of the C-ABI host layer (test infrastructure; no GPU).

Builds csrc/awsm_hip.cpp and csrc/awsm_resources.cpp host-only, links them with tests/trace/trace_hip.cpp — a stand-in for the HIP runtime and for
every launch wrapper — and runs one fixed script of small frames over awsm-renderer_amd/hip_backend.py.  The library writes what the host layer
enqueued: one line per launch wrapper (`L name stream scalars args=<hash of the argument struct>`), per traced runtime call (`H ...`), per
scenario (`== name`) and per note of this script (`-- ...`: the frame statistics, a refused call's status and text).  Two trees whose host layers enqueue the same thing give the
same file byte for byte; --verbose adds the argument structs' words, so that a difference names its offset.

    python tests/trace/driver.py --out trace.txt [--csrc DIR] [--verbose] [--only NAME]
    python tests/trace/driver.py --diff OTHER_CSRC       # this tree's trace against another tree's csrc/: hashes, line counts, verdict
"""
import argparse
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "awsm-renderer_amd", "csrc")
W, H = 64, 48


def build(csrc, out_dir):
    """-> the path of the trace library made of `csrc`'s two host files (fails where hipcc is missing)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: the host layer cannot be compiled for the launch trace")
    with open(os.path.join(csrc, "Makefile")) as fh:
        flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", fh.read(), re.M).group(1).replace("$(ARCH)", "gfx950").split()
    objs = []
    for src in (os.path.join(csrc, "awsm_hip.cpp"), os.path.join(csrc, "awsm_resources.cpp"), os.path.join(HERE, "trace_hip.cpp")):
        obj = os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        subprocess.check_call([hipcc, "--offload-host-only"] + flags + ["-I", csrc, "-c", "-o", obj, src])
        objs.append(obj)
    so = os.path.join(out_dir, "libawsm_trace.so")
    # g++ and not hipcc: nothing of the real runtime is linked; -Bsymbolic: the host files' hip* calls bind to the stand-ins of this library
    subprocess.check_call(["g++", "-shared", "-fPIC", "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-o", so] + objs)
    return so


# ---- the script ----
def draws_of(*tri_counts, stride=168):
    """One draw per count, packed one after the other in the vertex buffer (16-byte aligned offsets)."""
    out, off = [], 0
    for n in tri_counts:
        out.append({"geom_meta_off": 0, "vis_data_off": off, "tri_count": n, "flags": 0})
        off += (n * stride + 15) & ~15
    return out


WORLD = draws_of(4, 2, 6)
WORLD_B = draws_of(4, 3, 6, 1)
HUD = draws_of(2, 2)
BIG_HUD = draws_of(6000)           # more than the world pass's arrays were sized for: they move under the MSAA hud pass
CASTERS = draws_of(4, 2)
TRANSPARENT = draws_of(3, 2, stride=40)
HUD_TRANSPARENT = draws_of(2, stride=40)


class Script:
    def __init__(self, lib_path):
        os.environ["AWSM_HIP_LIB"] = lib_path
        sys.path.insert(0, ROOT)
        import numpy as np
        from awsm_renderer_amd import hip_backend
        self.np, self.hb = np, hip_backend
        assert hip_backend.LIB_PATH == lib_path
        self.lib = hip_backend.load_library()
        self.lib.awsm_trace_alloc.restype = C.c_void_p
        self.lib.awsm_trace_alloc.argtypes = [C.c_size_t]

    def begin(self, name, env=None):
        for k in ("AWSM_DEVICE_HANDOFF", "AWSM_GEOMETRY_CACHE"):
            os.environ.pop(k, None)
        os.environ.update(env or {})
        self.lib.awsm_trace_begin(name.encode())

    def note(self, text):
        self.lib.awsm_trace_note(str(text).encode())

    def device(self, msaa=0, **cfg):
        hb, np = self.hb, self.np
        d = hb.HipDevice(**cfg)
        for which in range(hb.BUF_COUNT):
            d.buffer_create(which, 168 * 6016 if hb.BUF_NAMES[which] == "VIS_GEOM_DATA" else 4096)
        cam = np.zeros(128, np.float32)
        for m in range(6):      # identity in every matrix of the block
            cam[16 * m:16 * m + 16] = np.eye(4, dtype=np.float32).reshape(-1)
        d.buffer_write(hb.BUF_NAMES.index("CAMERA"), 0, cam.view(np.uint8))
        d.brdf_lut_generate(32, 32)
        d.resize(W, H, msaa)
        return d

    def frame(self, label):
        """What follows, up to the next mark, is the frame `label` of the scenario (tests/test_launch_trace_cpu.py looks launches up by it)."""
        self.note("frame: %s" % label)

    def end(self, d):
        self.note(sorted(d.frame_end().items()))

    def arm(self, which, needed=6000, skip=0):
        self.lib.awsm_trace_arm(which, skip, needed)

    def refused(self, call):
        """`call` must be refused by the backend: its status and text go into the trace (pointer values, which differ from run to run, do not)."""
        try:
            call()
        except self.hb.AwsmHipError as e:
            self.note("refused: " + re.sub(r"0x[0-9a-f]+", "0x*", str(e)))
        else:
            raise AssertionError("the backend accepted what the script expects it to refuse")

    def light(self):
        return self.np.tile(self.np.eye(4, dtype=self.np.float32).reshape(-1), 8).tobytes()

    # -- scenarios --
    def basic(self, name, **cfg):
        self.begin(name)
        d = self.device(**cfg)
        for frame in ("first", "same list"):      # the second frame finds its draw list uploaded (its per-draw records are resolved again: stage timers)
            self.frame(frame); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
        self.frame("new list"); d.geometry_pass(WORLD_B); d.opaque_pass(mipmap=1); self.end(d)
        self.frame("no draws"); d.geometry_pass([]); d.opaque_pass(has_opaque=False); self.end(d)
        self.frame("has_opaque = 0"); d.geometry_pass(WORLD); d.opaque_pass(has_opaque=False); self.end(d)
        d.set_stage_timers(False)
        for frame in ("no timers", "no timers, nothing changed"):      # ... and without them the second one keeps its records
            self.frame(frame); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
        d.close()

    def overlap(self, name, env, query_ready):
        self.begin(name, env)
        d = self.device(overlap_frames=True)
        d.set_stage_timers(False)
        self.lib.awsm_trace_event_query(1 if query_ready else 0)
        for frame in range(5):
            self.frame(frame)
            d.geometry_pass(WORLD if frame != 2 else WORLD_B)
            d.opaque_pass()
            if frame == 3:
                d.transparent_pass(TRANSPARENT)
            if frame in (1, 4):      # (a flush orders the caller's stream behind the shade streams: the frames without one show the slot-free waits)
                d.frame_flush()
        self.frame("frame_end"); self.end(d)
        d.frame_trace(8)
        self.frame("traced"); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
        d.close()

    def hud(self, name, msaa, overlap=False):
        self.begin(name)
        d = self.device(msaa=msaa, overlap_frames=overlap)
        for frame, hud in enumerate((HUD, HUD, BIG_HUD, BIG_HUD, [])):      # MSAA: the third frame's hud draws move the world pass's arrays
            self.frame(frame)
            d.geometry_pass(WORLD if frame != 1 else WORLD_B)
            d.hud_geometry_pass(hud)
            d.opaque_pass()
            d.transparent_pass(TRANSPARENT if frame else [])
            d.hud_transparent_pass(HUD_TRANSPARENT)
            self.note(d.pick(5, 5))
            if not overlap or frame == 4:
                self.end(d)
        d.close()

    def shadow(self, name, msaa=0):
        self.begin(name)
        d = self.device(msaa=msaa)
        for casters, size in ((CASTERS, 64), ([], 64), (CASTERS, 96)):
            self.frame("%d casters, map %d" % (len(casters), size))
            d.geometry_pass(WORLD); d.shadow_pass(self.light(), casters, map_size=size); d.opaque_pass(); self.end(d)
        self.note(d.read_shadow_map().shape)
        self.frame("no shadow pass"); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)      # no shadow pass in a frame: no resolve in that frame
        d.close()

    def shadow_views(self, name, msaa=0):
        """Passes of several views, then the two entries in turn on one device (MSAA: the first two frames only)."""
        self.begin(name)
        d = self.device(msaa=msaa)
        view, empty = (self.light(), CASTERS), (self.light(), [])
        frames = [("2 views, map 64", [view, view]), ("3 views, the middle one empty", [view, empty, view])]
        if not msaa:
            frames += [("6 views", [view] * 6), ("shadow_pass after views", None), ("1 view", [view])]
        for label, views in frames:
            self.frame(label)
            d.geometry_pass(WORLD)
            if views is None:      # the slot's scene-table copy was overwritten per view: this pass makes its own anew
                d.shadow_pass(self.light(), CASTERS, map_size=64)
            else:
                d.shadow_pass_views(views, map_size=64)
            d.opaque_pass(); self.end(d)
            if label.startswith("2 views"):
                self.note(d.read_shadow_map(view=1).shape)
                self.note(d.read_shadow_map().shape)
        if not msaa:
            self.frame("no shadow pass"); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
            self.refused(lambda: d.read_shadow_map(view=1))      # nothing to read: each entry answers in its own words
            self.refused(lambda: d.read_shadow_map())
        d.close()

    def shadow_refusals(self, name):
        """What the two entries refuse, in the words they refuse it with (the texts are part of the trace: two trees must agree on them)."""
        self.begin(name)
        d = self.device()
        np = self.np
        nan, inf = float("nan"), float("inf")
        poisoned = np.frombuffer(self.light(), np.float32).copy(); poisoned[35] = nan
        broken = [dict(CASTERS[0], tri_count=1 << 30)]
        bad_records = (dict(map_size=0), dict(map_size=8193), dict(pcf_radius=3), dict(strength=1.5), dict(strength=-0.1), dict(facing_fade=0.0), dict(max_slope=-0.01),
                       dict(light=(0.0, 1.0, 0.0, 0.5)), dict(light=(nan, 1.0, 0.0, 0.0)), dict(bias=nan), dict(slope_bias=inf), dict(struct_size=2), dict(struct_size=5000))
        single = lambda block=self.light(), casters=CASTERS, **kw: d.shadow_pass(block, casters, **kw)
        views = lambda v=((self.light(), CASTERS), (self.light(), CASTERS)), **kw: d.shadow_pass_views(v, **kw)
        self.refused(single); self.refused(views)      # before the frame's geometry pass
        self.frame("refused"); d.geometry_pass(WORLD)
        for bad in bad_records:
            self.refused(lambda: single(**bad)); self.refused(lambda: views(**bad))
        for block in (self.light()[:508], self.light() + bytes(4), b"", poisoned.tobytes()):
            self.refused(lambda: single(block)); self.refused(lambda: views([(self.light(), CASTERS), (block, CASTERS)]))
        self.refused(lambda: single(casters=broken)); self.refused(lambda: views([(self.light(), CASTERS), (self.light(), broken)]))
        for bad in (dict(v=[]), dict(n_views=0), dict(v=[(self.light(), CASTERS)] * 7), dict(n_views=7)):
            self.refused(lambda: views(**bad))
        d.opaque_pass(); self.end(d)      # no pass was accepted: no resolve
        self.refused(single); self.refused(views)      # the window has closed
        d.close()
        self.frame("sharded context")
        d = self.device()
        d.set_shard_rows(16, 40)
        d.geometry_pass(WORLD)
        self.refused(single); self.refused(views)      # a sharded context
        d.close()

    def transparent(self, name, msaa=0):
        self.begin(name)
        d = self.device(msaa=msaa, parity_tap=True)
        d.set_editor_grid(alpha_minor=0.5)
        d.set_selection(mesh_keys=[(1, 2), (3, 4)], boxes=[(0, 0, 0, 1, 1, 1)])
        self.frame("grid + selection"); d.geometry_pass(WORLD); d.opaque_pass(); d.transparent_pass(TRANSPARENT); self.end(d)
        self.frame("readbacks")
        self.note([a.shape for a in d.read_selection()])
        self.note([a.shape for a in d.read_editor_grid()])
        self.note([a.shape for a in d.read_transformed_forward(15)])
        self.frame("no transparent draws"); d.geometry_pass(WORLD); d.opaque_pass(); d.transparent_pass([]); self.end(d)      # the grid and the overlay without a transparent mesh
        d.set_editor_grid(None); d.set_selection(on=None)
        self.frame("both off"); d.geometry_pass(WORLD); d.opaque_pass(); d.transparent_pass(TRANSPARENT); d.hud_transparent_pass(HUD_TRANSPARENT); self.end(d)
        d.close()

    def ssao(self, name, msaa=0):
        self.begin(name)
        d = self.device(msaa=msaa)
        d.set_ssao(radius=0.4)
        self.frame("on"); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
        self.frame("on, hud"); d.geometry_pass(WORLD); d.hud_geometry_pass(HUD); d.opaque_pass(); self.end(d)
        d.set_ssao(None)
        self.frame("off"); d.geometry_pass(WORLD); d.opaque_pass(); self.end(d)
        d.close()

    def post(self, name, msaa=0, overlap=False):
        self.begin(name)
        d = self.device(msaa=msaa, overlap_frames=overlap)
        d.set_taa(feedback=0.2, jitter_ndc=(0.01, -0.01))
        for frame in range(3):
            self.frame(frame)
            d.geometry_pass(WORLD); d.opaque_pass()
            if frame:
                d.transparent_pass(TRANSPARENT)
            d.post_pass(tonemapping=frame % 3, smaa=True, bloom=frame > 0, dof=frame > 0)
            if not overlap:
                self.end(d)
        self.frame("frame_end"); self.end(d)
        self.note([a.shape for a in d.read_taa()])
        d.close()

    def shards(self, name, bands, msaa=0):
        self.begin(name)
        d = self.device(msaa=msaa)
        if bands:
            d.set_shard_bands(2, 1, compact_output=True)
        else:
            d.set_shard_rows(16, 40)
        self.frame("sharded")
        d.geometry_pass(WORLD)
        if msaa and bands:
            n = d.msaa_halo_bands() * 2 * W * 8
            halo = self.lib.awsm_trace_alloc(2 * n)
            d.msaa_halo_export(halo, n)
            d.msaa_halo_bind(halo, 2 * n)
        d.opaque_pass()
        d.bind_opaque_source(self.lib.awsm_trace_alloc(W * H * 8), W * H * 8)
        d.transparent_pass(TRANSPARENT)
        self.end(d)
        self.note(d.visibility_digest())
        d.close()

    def replay(self, name, what, msaa=0, overlap=False):
        """One frame with every pass; the list named by `what` overflows once and awsm_hip_frame_end replays from there."""
        self.begin(name)
        d = self.device(msaa=msaa, overlap_frames=overlap, small_bin_list=True)
        d.set_editor_grid(); d.set_ssao(); d.set_taa()
        d.set_selection(mesh_keys=[(1, 2)], boxes=[(0, 0, 0, 1, 1, 1)])
        for frame in range(3 if overlap else 1):
            last = frame == (2 if overlap else 0)
            self.frame("overflowing" if last else frame)
            if last and what == "world": self.arm(0)
            d.geometry_pass(WORLD)
            if last and what == "hud_geometry": self.arm(0)
            d.hud_geometry_pass(HUD)
            if last and what == "shadow": self.arm(0)
            if last and what == "shadow_views": self.arm(0, skip=1)      # the second view's scan: the flag goes up in that view's own counter words
            if what == "shadow_views":
                d.shadow_pass_views([(self.light(), CASTERS)] * 3, map_size=64)
            else:
                d.shadow_pass(self.light(), CASTERS, map_size=64)
            d.opaque_pass()
            if last and what == "transparent_bins": self.arm(0)
            if last and what == "transparent_fragments": self.arm(1)
            d.transparent_pass(TRANSPARENT)
            if last and what == "hud_transparent_bins": self.arm(0)
            if last and what == "hud_transparent_fragments": self.arm(1)
            d.hud_transparent_pass(HUD_TRANSPARENT)
            d.post_pass(bloom=True)
        self.frame("frame_end"); self.end(d)
        self.frame("readbacks")
        self.note([a.shape for a in d.read_transformed(12)])
        self.note(d.read_visibility_unpacked()[0].shape)
        d.close()

    def scenarios(self):
        yield "sync", lambda n: self.basic(n)
        yield "sync_general_shade_only", lambda n: self.basic(n, general_shade_only=True)
        yield "sync_msaa", lambda n: self.basic(n, msaa=4)
        yield "overlap_handoff", lambda n: self.overlap(n, {}, True)
        yield "overlap_events", lambda n: self.overlap(n, {"AWSM_DEVICE_HANDOFF": "0"}, False)
        yield "hud", lambda n: self.hud(n, 0)
        yield "hud_msaa", lambda n: self.hud(n, 4)
        yield "hud_msaa_overlap", lambda n: self.hud(n, 4, overlap=True)
        yield "shadow", lambda n: self.shadow(n)
        yield "shadow_msaa", lambda n: self.shadow(n, 4)
        yield "shadow_views", lambda n: self.shadow_views(n)
        yield "shadow_views_msaa", lambda n: self.shadow_views(n, 4)
        yield "shadow_refusals", lambda n: self.shadow_refusals(n)
        yield "transparent_grid_selection", lambda n: self.transparent(n)
        yield "transparent_grid_selection_msaa", lambda n: self.transparent(n, 4)
        yield "ssao", lambda n: self.ssao(n)
        yield "ssao_msaa", lambda n: self.ssao(n, 4)
        yield "post_taa", lambda n: self.post(n)
        yield "post_taa_msaa_overlap", lambda n: self.post(n, 4, overlap=True)
        yield "shard_rows", lambda n: self.shards(n, False)
        yield "shard_rows_msaa", lambda n: self.shards(n, False, 4)
        yield "shard_bands", lambda n: self.shards(n, True)
        yield "shard_bands_msaa", lambda n: self.shards(n, True, 4)
        for what in ("world", "hud_geometry", "shadow", "shadow_views", "transparent_bins", "transparent_fragments", "hud_transparent_bins", "hud_transparent_fragments"):
            yield "replay_" + what, lambda n, w=what: self.replay(n, w)
        yield "replay_world_msaa", lambda n: self.replay(n, "world", msaa=4)             # the merged hud keys: a new world pass needs a new merge
        yield "all_at_once", lambda n: self.replay(n, "world", msaa=4, overlap=True)     # every pass, overlapped, MSAA, and a replay of all of it


def run(lib_path, out_path, verbose=False, only=None):
    s = Script(lib_path)
    if s.lib.awsm_trace_open(out_path.encode(), 1 if verbose else 0) != 0:
        raise RuntimeError("cannot write " + out_path)
    for name, fn in s.scenarios():
        if only is None or name in only:
            fn(name)
    s.lib.awsm_trace_close()


def trace_of(csrc, verbose=False):
    """The trace of `csrc` as text: built and run in a process of its own (the library's path is fixed when hip_backend is imported)."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "trace.txt")
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--csrc", csrc, "--out", out, "--build-dir", tmp] + (["--verbose"] if verbose else []))
        with open(out) as fh:
            return fh.read()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", default=CSRC, help="the csrc/ directory whose host files are traced (default: this tree's)")
    ap.add_argument("--out", help="where the trace goes")
    ap.add_argument("--build-dir")
    ap.add_argument("--verbose", action="store_true", help="the argument structs as 32-bit words behind their hashes")
    ap.add_argument("--only", action="append", help="run these scenarios only")
    ap.add_argument("--diff", metavar="OTHER_CSRC", help="compare this tree's trace with that of another csrc/ directory")
    a = ap.parse_args()
    if a.diff:
        texts = [trace_of(os.path.abspath(a.diff)), trace_of(CSRC)]
        for label, t in zip(("parent", "this tree"), texts):
            print("%-9s sha256 %s  %d lines, %d launches, %d scenarios" % (label, hashlib.sha256(t.encode()).hexdigest(), t.count("\n"), t.count("\nL "), t.count("== ")))
        print("identical" if texts[0] == texts[1] else "DIFFERENT")
        return 0 if texts[0] == texts[1] else 1
    if not a.out:
        ap.error("--out or --diff")
    tmp = a.build_dir or tempfile.mkdtemp(prefix="awsm_trace_")
    run(build(os.path.abspath(a.csrc), tmp), a.out, a.verbose, a.only)
    return 0


if __name__ == "__main__":
    sys.exit(main())
