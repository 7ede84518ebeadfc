"""The order in which the C-ABI host layer (csrc/awsm_hip.cpp) launches a frame's kernels, and the stream each launch goes to, checked without a GPU.

tests/trace/ compiles the two host files host-only and links them with a stand-in for the HIP runtime and for every launch wrapper of csrc/launch.hpp;
tests/trace/driver.py runs one fixed script of small frames over it and the stand-ins write down what was enqueued.  This module asserts, per frame of
that script, the sequence of (wrapper, stream role) against lists written out by hand from DESIGN.md's description of each pass — names and streams
only, not the argument structs' bytes, so that a feature which adds a FrameDev member has nothing to regenerate here.  (Byte-for-byte comparison of two
trees' traces is the driver's --diff; profiles/launch_trace_diff.txt holds the last one.)  awsm_launch_upload_words — the scene table, a draw list or a
camera block on their way to the device — is data movement, not a pass's kernel, and is left out of the sequences.

hipcc is needed to compile the host files: where it is missing the module fails, it does not skip."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("awsm_trace_driver", os.path.join(ROOT, "tests", "trace", "driver.py"))
driver = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(driver)


@pytest.fixture(scope="module")
def frames():
    """{(scenario, frame label): [(wrapper, stream role), ...]} of this tree's trace, and the trace's text."""
    text = driver.trace_of(driver.CSRC)
    out, scenario, cur = {}, None, None
    for line in text.split("\n"):
        if line.startswith("== "):
            scenario, cur = line[3:], None
        elif line.startswith("-- frame: "):
            cur = out.setdefault((scenario, line[10:]), [])
        elif line.startswith("L ") and cur is not None:
            name, stream = line.split()[1:3]
            assert name.startswith("awsm_launch_")
            if name != "awsm_launch_upload_words":
                cur.append((name[len("awsm_launch_"):], stream))
    return out, text


def on(stream, *names):
    return [(n, stream) for n in names]


# ---- the passes, as DESIGN.md describes them ----
BIN = ("bin_count", "bin_big", "bin_scan", "bin_fill", "bin_big")      # count -> big triangles -> scan -> fill -> big triangles


def geometry(s="caller"):
    """A geometry-type pass with triangles (world, hud, shadow): transform, the binning chain, the tile raster."""
    return on(s, "transform", *BIN, "raster")


def empty_geometry(s="caller"):
    """... without triangles: memsets instead of the transform, the scan alone, the raster (every tile becomes "no hit")."""
    return on(s, "bin_scan", "raster")


def opaque(s="caller", resolve=True, behind=()):
    """The opaque pass: the per-draw resolve (when its inputs changed), the lean kernel's launch, the general kernel for what it left, then shadow / SSAO."""
    return on(s, *(("resolve_draws",) if resolve else ()), "shade", "shade_todo", *behind)


def forward(s="caller", behind=()):
    """A transparent pass with triangles: per-draw resolve first, its own transform, the binning chain, the forward kernels, then the overlay."""
    return on(s, "resolve_draws", "transform_forward", *BIN, "forward", *behind)


def empty_forward(s="caller", behind=()):
    return on(s, "bin_scan", "forward", *behind)


COVERED = on("caller", "count_covered")      # awsm_hip_frame_end with a stats struct: the covered pixels, counted from the keys


def test_the_script_covers_what_it_should(frames):
    by_frame, text = frames
    scenarios = {k[0] for k in by_frame}
    assert {"sync", "overlap_handoff", "overlap_events", "hud", "hud_msaa", "hud_msaa_overlap", "shadow", "shadow_views", "shadow_views_msaa",
            "shadow_refusals", "transparent_grid_selection", "ssao", "post_taa",
            "shard_rows", "shard_bands", "shard_bands_msaa", "all_at_once"} <= scenarios
    assert {"replay_" + w for w in ("world", "hud_geometry", "shadow", "shadow_views", "transparent_bins", "transparent_fragments", "hud_transparent_bins",
                                    "hud_transparent_fragments")} <= scenarios
    assert text.count("raises-overflow=") == 10      # one per replay scenario (the eight, the MSAA one, all_at_once)
    # the slot-free wait appears: a slot whose shading the host finds unfinished makes the caller's stream wait for it
    assert re.search(r"^H hipEventQuery (ev\d+)\nH hipStreamWaitEvent caller \1$", text, re.M)


def test_synchronous_frames(frames):
    f, _ = frames
    assert f["sync", "first"] == geometry() + opaque() + COVERED
    assert f["sync", "same list"] == geometry() + opaque() + COVERED             # (stage timers on: the resolve always runs)
    assert f["sync", "new list"] == geometry() + opaque() + COVERED
    assert f["sync", "no draws"] == empty_geometry() + opaque(resolve=False)     # has_opaque = 0: no resolve, no covered-pixel count
    assert f["sync", "has_opaque = 0"] == geometry() + opaque(resolve=False)
    assert f["sync", "no timers"] == geometry() + opaque() + COVERED
    assert f["sync", "no timers, nothing changed"] == geometry() + opaque(resolve=False) + COVERED      # the per-draw records are kept


def test_overlapped_frames_alternate_between_the_shade_streams(frames):
    f, _ = frames
    # device-side hand-off: the resolve goes ahead on the slot's shade stream, the geometry pass signals, the shade stream waits for it — and, from the
    # second frame on, for the other slot's shading — and signals its own end
    def frame(s, wait_prev, resolve=True):
        early = on(s, "resolve_draws") if resolve else []
        return geometry() + early + on("caller", "handoff_signal") + on(s, "handoff_wait", *(("handoff_wait",) if wait_prev else ())) + opaque(s, resolve=False) + on(s, "handoff_signal")
    assert f["overlap_handoff", "0"] == frame("shade1", False)
    assert f["overlap_handoff", "1"] == frame("shade0", True)
    assert f["overlap_handoff", "2"] == frame("shade1", True)
    assert f["overlap_handoff", "3"] == frame("shade0", True, resolve=False) + on("shade0", "handoff_wait") + forward("shade0") + on("shade0", "handoff_signal")
    assert f["overlap_handoff", "4"] == frame("shade1", True)
    # ordered by events instead: the same kernels on the same streams, no hand-off kernels
    for k, s in enumerate(("shade1", "shade0", "shade1")):
        assert f["overlap_events", str(k)] == geometry() + opaque(s)
    assert f["overlap_events", "3"] == geometry() + opaque("shade0", resolve=False) + forward("shade0")
    assert f["overlap_events", "4"] == geometry() + opaque("shade1")
    assert f["overlap_events", "frame_end"] == COVERED


def test_hud_passes(frames):
    f, _ = frames
    # single-sampled: the hud geometry pass has arrays of its own; the transparent passes follow the opaque pass, the HUD one last
    assert f["hud", "0"] == geometry() + geometry() + opaque() + empty_forward() + forward() + on("caller", "pick") + COVERED
    assert f["hud", "2"] == geometry() + geometry() + opaque() + forward() + forward() + on("caller", "pick") + COVERED
    assert f["hud", "4"] == geometry() + opaque() + forward() + forward() + on("caller", "pick") + COVERED      # no hud draws: no hud geometry pass
    # MSAA: one rank space, and a merge of the two passes' keys for the opaque pass
    merged = geometry() + geometry() + on("caller", "hud_merge")
    assert f["hud_msaa", "0"] == merged + opaque() + empty_forward() + forward() + on("caller", "pick") + COVERED
    assert f["hud_msaa", "1"] == merged + opaque() + forward() + forward() + on("caller", "pick") + COVERED
    # the world pass's arrays moved under the hud draws: the world pass runs again into the new ones, in front of the hud pass
    assert f["hud_msaa", "2"] == geometry() + merged + opaque() + forward() + forward() + on("caller", "pick") + COVERED
    assert f["hud_msaa", "3"] == merged + opaque() + forward() + forward() + on("caller", "pick") + COVERED
    assert f["hud_msaa", "4"] == geometry() + opaque() + forward() + forward() + on("caller", "pick") + COVERED


def test_shadow_pass(frames):
    f, _ = frames
    assert f["shadow", "2 casters, map 64"] == geometry() + geometry() + opaque(behind=("shadow_resolve",)) + COVERED
    assert f["shadow", "0 casters, map 64"] == geometry() + empty_geometry() + opaque(behind=("shadow_resolve",)) + COVERED
    assert f["shadow", "2 casters, map 96"] == geometry() + geometry() + opaque(behind=("shadow_resolve",)) + COVERED
    assert f["shadow", "no shadow pass"] == geometry() + opaque() + COVERED


def test_shadow_pass_views(frames):
    f, _ = frames
    resolved = opaque(behind=("shadow_resolve",)) + COVERED      # one resolve for all the views, behind the opaque pass's kernels
    # the world pass, then every view's chain in the views' order on the caller's stream
    assert f["shadow_views", "2 views, map 64"] == geometry() + geometry() + geometry() + resolved
    assert f["shadow_views", "3 views, the middle one empty"] == geometry() + geometry() + empty_geometry() + geometry() + resolved
    assert f["shadow_views", "6 views"] == geometry() + 6 * geometry() + resolved
    assert f["shadow_views", "shadow_pass after views"] == geometry() + geometry() + resolved
    assert f["shadow_views", "1 view"] == geometry() + geometry() + resolved
    assert f["shadow_views", "no shadow pass"] == geometry() + opaque() + COVERED
    assert f["shadow_views_msaa", "2 views, map 64"] == geometry() + geometry() + geometry() + resolved      # (the maps are single-sampled)
    assert f["shadow_views_msaa", "3 views, the middle one empty"] == geometry() + geometry() + empty_geometry() + geometry() + resolved
    assert f["shadow_refusals", "refused"] == geometry() + opaque() + COVERED      # a refused pass enqueues nothing and leaves no resolve behind


def test_transparent_pass_with_grid_and_selection(frames):
    f, _ = frames
    assert f["transparent_grid_selection", "grid + selection"] == geometry() + opaque() + forward(behind=("selection",)) + COVERED
    assert f["transparent_grid_selection", "readbacks"] == on("caller", "selection_layers", "editor_grid_layer")
    assert f["transparent_grid_selection", "no transparent draws"] == geometry() + opaque() + empty_forward(behind=("selection",)) + COVERED
    assert f["transparent_grid_selection", "both off"] == geometry() + opaque() + forward() + forward() + COVERED


def test_ssao_and_post_passes(frames):
    f, _ = frames
    assert f["ssao", "on"] == geometry() + opaque(behind=("ssao",)) + COVERED
    assert f["ssao", "on, hud"] == geometry() + geometry() + opaque(behind=("ssao",)) + COVERED
    assert f["ssao", "off"] == geometry() + opaque() + COVERED
    assert f["post_taa", "0"] == geometry() + opaque() + on("caller", "taa", "post") + COVERED      # the resolve in front of the effects
    assert f["post_taa", "1"] == geometry() + opaque() + forward() + on("caller", "taa", "post") + COVERED
    assert f["post_taa", "frame_end"] == COVERED + on("caller", "taa_layers")


def test_sharded_contexts(frames):
    f, _ = frames
    for scenario in ("shard_rows", "shard_rows_msaa", "shard_bands"):
        assert f[scenario, "sharded"] == geometry() + opaque() + forward() + COVERED + on("caller", "vis_digest")
    assert f["shard_bands_msaa", "sharded"] == geometry() + on("caller", "msaa_halo_export") + opaque() + forward() + COVERED + on("caller", "vis_digest")


def test_frame_end_replays_from_the_first_pass_that_lost_entries(frames):
    f, _ = frames
    frame = geometry() + geometry() + geometry() + opaque(behind=("shadow_resolve", "ssao")) + forward(behind=("selection",)) + forward() + on("caller", "taa", "post")
    # behind a geometry-type pass: that pass, the opaque pass, both transparent passes in their order, the post pass
    tail_transparent = forward(behind=("selection",)) + forward() + on("caller", "taa", "post") + COVERED
    tail_opaque = opaque(behind=("shadow_resolve", "ssao")) + tail_transparent
    for what in ("world", "hud_geometry", "shadow"):
        assert f["replay_" + what, "overflowing"] == frame
        assert f["replay_" + what, "frame_end"] == COVERED + geometry() + tail_opaque
    # a pass of views whose second view lost entries: every view again, in the views' order, then the opaque pass
    views = geometry() + geometry() + geometry()
    assert f["replay_shadow_views", "overflowing"] == geometry() + geometry() + views + frame[len(3 * geometry()):]
    assert f["replay_shadow_views", "frame_end"] == COVERED + views + tail_opaque
    # behind a transparent pass's list, bins or fragments, the world's or the HUD's: the world transparent pass first, always
    for what in ("transparent_bins", "transparent_fragments", "hud_transparent_bins", "hud_transparent_fragments"):
        assert f["replay_" + what, "overflowing"] == frame
        assert f["replay_" + what, "frame_end"] == COVERED + tail_transparent
    # MSAA with hud meshes: a new world pass needs a new merge
    assert f["replay_world_msaa", "frame_end"] == COVERED + geometry() + geometry() + on("caller", "hud_merge") + tail_opaque


def test_every_pass_at_once_overlapped_and_replayed(frames):
    f, _ = frames
    s = "shade1"
    geo = geometry() + geometry() + on("caller", "hud_merge") + geometry()      # world, hud (merged), shadow
    # (the hud draws arrive on the caller's stream behind the world pass's upload event: the resolve takes the late order, behind the hand-off)
    def passes(waits):
        w = on(s, "handoff_wait") if waits else []
        return (on("caller", "handoff_signal") + on(s, "handoff_wait") + w + opaque(s, behind=("shadow_resolve", "ssao")) + on(s, "handoff_signal")
                + w + forward(s, behind=("selection",)) + on(s, "handoff_signal") + w + forward(s) + on(s, "handoff_signal")
                + w + on(s, "taa", "post") + on(s, "handoff_signal"))
    assert f["all_at_once", "overflowing"] == geo + passes(True)
    # the replay: the streams were drained, nothing is waited for but the geometry pass; no shadow pass (its list held)
    assert f["all_at_once", "frame_end"] == COVERED + geometry() + geometry() + on("caller", "hud_merge") + passes(False) + COVERED
