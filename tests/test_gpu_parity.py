"""GPU parity: the HIP path (through the C-ABI) against the CPU oracle on the same seeded scenes.

Bar (BASELINE.json north_star): triangle-id + depth bit-exact; shaded RGB within 1e-4 — absolute for values up to 1.0,
relative (1e-4 * |ref|) for HDR values above 1.0 — checked on the f32 parity tap; the RGBA16F image must be within
2 f16 ulp of the oracle's (1e-4 is below half an f16 ulp for values above 0.125, so the stored halves can legitimately
round apart).  A pixel over the colour bar is accepted only when its condition number, measured on the oracle itself, explains the
difference, and only a handful per frame may need that (tests/helpers.py: compare_frames)."""
import dataclasses
import math
import os

import numpy as np
import pytest

from awsm_renderer_amd import scenes
from oracle import oracle_lib
from tests import helpers

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4


def _check(scene, lut, rows=(0, 0)):
    model = helpers.build_model(scene)
    orc = helpers.oracle_frame(model, lut, rows=rows)
    dev, stats = helpers.hip_frame(model, lut, rows=rows)
    r = helpers.compare_frames(orc, dev, rows=None if rows == (0, 0) else rows, rgb_tol=RGB_TOL)
    dev.close()
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0, r
    assert r["key_mismatch"] == 0, r
    assert r["covered"] > 0, r
    assert stats["covered_pixels"] == r["covered"], (stats, r)
    assert r["rgb_over_tol"] == 0, r
    assert r["alpha_mismatch"] == 0, r
    assert r["f16_max_ulp"] <= 2, r
    return r, stats


def _check_host(scene, lut, rows=(0, 0)):
    """Same bar, but through the C++ host layer (the path bench.py and smoke() use)."""
    model = helpers.build_model(scene)
    orc = helpers.oracle_frame(model, lut, rows=rows)
    r, dev, stats = helpers.host_frame(scene, lut, rows=rows)
    res = helpers.compare_frames(orc, dev, rows=None if rows == (0, 0) else rows, rgb_tol=RGB_TOL)
    # a second frame with nothing changed uploads nothing and renders the same image
    st2 = r.render(sync=True)
    uploaded = r.host.upload_bytes_last_frame()
    res2 = helpers.compare_frames(orc, dev, rows=None if rows == (0, 0) else rows, rgb_tol=RGB_TOL)
    dev.close()
    r.close()
    for x in (res, res2):
        assert x["clip_mismatch"] == 0 and x["nt_mismatch"] == 0 and x["key_mismatch"] == 0, x
        assert x["rgb_over_tol"] == 0 and x["alpha_mismatch"] == 0 and x["f16_max_ulp"] <= 2, x
    assert uploaded == 0, uploaded
    assert st2["covered_pixels"] == stats["covered_pixels"] == res["covered"]


@pytest.mark.parametrize("name", ["box", "helmet", "skinned_morph", "atrium"])
def test_through_host_layer(name, oracle_lut):
    scene = {"box": lambda: scenes.box_scene(200, 160),
             "helmet": lambda: scenes.helmet_scene(400, 240, segments=48, rings=36, tex_size=64),
             "skinned_morph": lambda: scenes.skinned_morph_scene(400, 240, around=24, along=64, tex_size=32),
             "atrium": lambda: scenes.atrium_scene(512, 288, detail=0.25, tex_scale=1 / 16)}[name]()
    _check_host(scene, oracle_lut)


def test_host_layer_shard_rows(oracle_lut):
    _check_host(scenes.atrium_scene(384, 224, detail=0.125, tex_scale=1 / 32), oracle_lut, rows=(101, 197))


def test_box(oracle_lut):
    _check(scenes.box_scene(256, 256), oracle_lut)


def test_helmet_small(oracle_lut):
    _check(scenes.helmet_scene(480, 270, segments=64, rings=48, tex_size=128), oracle_lut)


def test_skinned_morph_small(oracle_lut):
    _check(scenes.skinned_morph_scene(480, 270, around=32, along=96, tex_size=64), oracle_lut)


def test_atrium_small(oracle_lut):
    _check(scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 16), oracle_lut)


def test_atrium_odd_size_and_shard(oracle_lut):
    # width/height not multiples of the 32-px tile or the 16-px shade block; shard rows [64, 201)
    _check(scenes.atrium_scene(333, 201, detail=0.125, tex_scale=1 / 32), oracle_lut)
    _check(scenes.atrium_scene(333, 201, detail=0.125, tex_scale=1 / 32), oracle_lut, rows=(64, 201))


def test_material_zoo_every_shading_feature(oracle_lut):
    """vertex colour, emissive strength, ior, specular, volume, clearcoat, sheen, unlit, debug views, second UV set, texture
    transforms, clamp/mirror/nearest samplers, non-pow2 textures, point + spot lights, dangling texture ids."""
    r, stats = _check(scenes.material_zoo_scene(640, 360), oracle_lut)
    assert r["covered"] > 50000
    _check_host(scenes.material_zoo_scene(333, 187, tex_size=32), oracle_lut)


def test_orthographic_camera(oracle_lut):
    _check(scenes.ortho_scene(), oracle_lut)


def test_empty_pipeline_is_skybox_only(oracle_lut):
    scene = scenes.box_scene(128, 96)
    scene.skybox_rgba = (0.25, 0.5, 0.75, 1.0)
    model = helpers.build_model(scene)
    dev, _ = helpers.hip_frame(model, oracle_lut, has_opaque=False)
    img = dev.read_opaque_f32()
    dev.close()
    assert np.all(img == np.array([0.25, 0.5, 0.75, 1.0], dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3, 5])
def test_band_sharding_rows_identical_to_full_frame(oracle_lut, n):
    """awsm_hip_set_shard_bands: every shard's rows (visibility keys, f32 tap, RGBA16F) are bit-identical to the same rows
    of the unsharded frame rendered by the same device; compact output lands where sharding.bands_to_image expects it."""
    from awsm_renderer_amd import sharding
    sc = scenes.atrium_scene(1000, 563, detail=0.25, tex_scale=0.125)      # 18 tile rows (the last one partial), odd width
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut)
    full_keys, full_f32, full_f16 = dev.read_visibility(), dev.read_opaque_f32(), dev.read_opaque()
    draws = model.collect_draws()
    H, W = sc.height, sc.width
    L = sharding.bands_per_rank(H, n)
    gathered = np.zeros((n, L * 32, W, 4), dtype=np.uint16)
    covered = 0
    for r in range(n):
        rows = np.array(sharding.band_rows(H, n, r), dtype=np.int64)
        dev.set_shard_bands(n, r, compact_output=False)
        dev.geometry_pass(draws); dev.opaque_pass(); st = dev.frame_end()
        covered += st["covered_pixels"]
        assert (dev.read_visibility()[rows] == full_keys[rows]).all()
        assert (dev.read_opaque_f32()[rows].view(np.uint32) == full_f32[rows].view(np.uint32)).all()
        dev.set_shard_bands(n, r, compact_output=True)
        dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
        comp = dev.read_opaque()
        assert (comp[: len(rows)] == full_f16[rows]).all()
        gathered[r, : len(rows)] = comp[: len(rows)]
    assert covered == int((full_keys != helpers.NO_HIT).sum())
    img = sharding.bands_to_image(gathered.reshape(n, L, 32, W, 4), H, n)
    assert (img == full_f16).all()
    dev.set_shard_bands(1, 0)
    dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
    assert (dev.read_visibility() == full_keys).all()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("launcher", ["self", "torchrun"])
@pytest.mark.parametrize("msaa,extra", [(0, []), (4, []), (4, ["--strips"]), (0, ["--gather", "root"])])
def test_bench_two_rank_rehearsal_on_one_gpu(msaa, extra, launcher):
    """bench.py's N > 1 path (band sharding, compact outputs, double-buffered gather, de-interleave) run as two processes
    sharing this box's one GPU, with the collectives staged through gloo; --check compares the gathered image with an
    unsharded render bit for bit (with --gather root: on rank 0, the only rank that holds the frame).  (RCCL itself needs one GPU per rank: the driver's 8-GPU node runs that.)
    launcher "self": `python bench.py --gpus 2 ...` exactly as the driver types it — bench.py starts its own ranks as child processes before anything
    touches the GPU; "torchrun": the same under torch.distributed.run (WORLD_SIZE set: bench.py is a rank).  One case of the latter is enough."""
    import json, os, socket, subprocess, sys
    if launcher == "torchrun" and (msaa or extra):
        pytest.skip("the external launcher is covered by the plain bands case")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(AWSM_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable]
    if launcher == "torchrun":
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port)]
    cmd += [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--width", "640", "--height", "363", "--detail", "0.125",
            "--tex-scale", "0.0625", "--no-cpu-baseline", "--check", "--profile-frames", "1", "--msaa", str(msaa), "--full"] + extra
    p = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]          # ONE JSON line on stdout, rank 0's
    out = json.loads(lines[0])
    assert out["check"] == "ok" and out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["value"] > 0
    assert [pr["rank"] for pr in out["per_rank"]] == [0, 1] and all(pr["kernel_ms"]["k_raster_tile"] > 0 for pr in out["per_rank"])
    assert out["collective"]["alone_ms"] > 0 and ("child processes" in out["collective"]["launcher"]) == (launcher == "self")
    assert ("gather to rank 0" in out["config"]["sharding"]) == ("root" in extra)
    assert ("row strips" in out["config"]["sharding"]) == ("--strips" in extra) and ("boundary sample-0 keys" in out["config"]["sharding"]) == (msaa == 4 and not extra)


@pytest.mark.gpu
def test_rccl_one_rank_carries_what_the_library_rendered():
    """The collectives of bench.py's N > 1 loop on RCCL itself, as far as one GPU goes: world size 1 (tests/rccl_one_rank.py, in a process of its
    own).  Frames rendered into torch tensors on the library's shade streams, flushed, gathered on RCCL's stream while the next frame renders:
    every gathered frame equals the library's own image bit for bit.  What stays for the driver's 8-GPU node is more than one peer."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "rccl_one_rank.py")], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    if p.returncode != 0 and any(m in p.stderr for m in ("no socket interface found", "Bootstrap : no", "ncclSystemError", "ncclInternalError: Internal check failed")) \
            and "AssertionError" not in p.stderr:
        pytest.skip("RCCL could not initialise on this box (its bootstrap, not this repo): " + p.stderr.strip().splitlines()[-1][:200])
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-2000:] + p.stderr[-4000:]


@pytest.mark.gpu
def test_picker_matches_visibility_buffer(oracle_lut):
    """awsm_hip_pick / awsm_host_pick (picker.rs:55-121, picker_wgsl/compute.wgsl): the mesh key under a pixel is the one
    the oracle's visibility buffer attributes to it; background, out-of-frame and other-shard pixels miss."""
    from oracle.host_mirror import key_as_ffi
    sc = scenes.atrium_scene(640, 360, detail=0.125, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut)
    draws = model.collect_draws()
    first = np.concatenate([[0], np.cumsum([d["tri_count"] for d in draws])])
    r, dev, _ = helpers.host_frame(sc, oracle_lut)
    rng = np.random.default_rng(7)
    pts = [(int(x), int(y)) for x, y in zip(rng.integers(0, sc.width, 40), rng.integers(0, sc.height, 40))] + [(0, 0), (sc.width - 1, sc.height - 1)]
    hits = 0
    for x, y in pts:
        key = orc.keys[y, x]
        got_dev, got_host = dev.pick(x, y), r.host.pick(x, y)
        if key == helpers.NO_HIT:
            assert got_dev is None and got_host is None
            continue
        rank = 0xFFFFFFFF - int(key & np.uint64(0xFFFFFFFF))
        d = int(np.searchsorted(first, rank, side="right") - 1)
        want_key = key_as_ffi(draws[d]["mesh_key"])
        assert got_dev == (want_key, rank - int(first[d])), (x, y)
        assert got_host == want_key and want_key in r.keys.mesh_keys
        hits += 1
    assert hits > 20
    for x, y in [(-1, 5), (5, -1), (sc.width, 5), (5, sc.height), (2 ** 31 - 1, 0)]:
        assert dev.pick(x, y) is None and r.host.pick(x, y) is None
    # a pixel of another shard misses; one of this shard still hits
    dev.set_shard_bands(2, 1)
    dev.geometry_pass(HipDeviceDraws(model)); dev.opaque_pass(); dev.frame_end()
    ys = [y for y in range(sc.height) if (y // 32) % 2 == 0 and orc.keys[y, 100] != helpers.NO_HIT]
    yo = [y for y in range(sc.height) if (y // 32) % 2 == 1 and orc.keys[y, 100] != helpers.NO_HIT]
    assert dev.pick(100, ys[0]) is None and dev.pick(100, yo[0]) is not None
    r.close()


def HipDeviceDraws(model):
    return model.collect_draws()


@pytest.mark.gpu
def test_bin_list_overflow_grows_and_replays(oracle_lut):
    """A (triangle, tile) list that is too small (AWSM_CFG_SMALL_BIN_LIST: 4096 entries) overflows in the counting pass;
    frame_end grows it to the measured need and replays the frame — the result is the same frame."""
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut)
    dev, stats = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, small_bin_list=True))
    assert stats["bin_entries"] > 4096 and stats["bin_overflow_retries"] >= 1, stats
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and stats["covered_pixels"] == r["covered"], (r, stats)
    # the list keeps its new size: the next frame needs no replay
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); st2 = dev.frame_end()
    assert st2["bin_overflow_retries"] == stats["bin_overflow_retries"] and (dev.read_visibility() == orc.keys).all()
    dev.close()


def _host_threads():
    """Threads for the oracle on a full-size frame: every core this process may use (the GPU box's share may be smaller than os.cpu_count())."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 16
    return max(8, min(n, 128))


def _assert_full_frame(name, orc, dev, stats):
    """The whole frame against the oracle, every pixel: vertices, keys (all samples) bit-exact; colours at the bar of compare_frames; the bars reported."""
    H = orc.height
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    helpers.report_bars(name, (0, H), r)
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0 and r["key_mismatch"] == 0, (name, r)
    assert r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, (name, r)
    assert stats["covered_pixels"] == r["covered"], (name, stats, r)
    return r


@pytest.mark.gpu
def test_full_size_4k_frame_properties(oracle_lut):
    """BASELINE configs[3] at its full size (3840x2160, 262,144 triangles): EVERY pixel of the frame against the oracle (round 5; until then two strips =
    4 % of the frame: the oracle shades a 4K frame in seconds on all host threads) — vertices and keys bit-exact, colours at the bar of
    helpers.compare_frames, the counts over the absolute / relative / conditioned bars reported (profiles/r05_parity_bars.txt).  Then the
    size-independent properties as before: a re-render is bit-identical, band shards reproduce the unsharded rows exactly, the covered-pixel count
    matches the visibility buffer, and some tile holds more than 256 distinct visible triangles (the raster stage's split-tile merge is in the frame)."""
    sc = scenes.atrium_scene(3840, 2160)
    model = helpers.build_model(sc)
    dev, stats = helpers.hip_frame(model, oracle_lut)
    keys, img = dev.read_visibility(), dev.read_opaque()
    assert stats["covered_pixels"] == int((keys != helpers.NO_HIT).sum()) > 8_000_000
    ranks = (keys[:2144] & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(67, 32, 120, 32).transpose(0, 2, 1, 3).reshape(67, 120, 1024)
    srt = np.sort(ranks, axis=2)
    distinct = 1 + (srt[:, :, 1:] != srt[:, :, :-1]).sum(axis=2)
    assert int(distinct.max()) > 256, int(distinct.max())
    orc = helpers.oracle_frame(model, oracle_lut, threads=_host_threads())
    _assert_full_frame("configs[3] atrium 3840x2160 single-sampled", orc, dev, stats)
    del orc
    draws = model.collect_draws()
    dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
    assert (dev.read_visibility() == keys).all() and (dev.read_opaque() == img).all()           # deterministic
    from awsm_renderer_amd import sharding
    dev.set_shard_bands(4, 2)
    dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
    mine = np.array(sharding.band_rows(sc.height, 4, 2))
    assert (dev.read_visibility()[mine] == keys[mine]).all() and (dev.read_opaque()[mine] == img[mine]).all()
    dev.close()


@pytest.mark.gpu
def test_full_size_4k_reference_default_mode(oracle_lut):
    """The same 4K frame in the mode the reference actually defaults to — AntiAliasing::default() = MSAA x4 + MipmapMode::Gradient
    (anti_alias.rs:28-38; compute.wgsl:100-322, helpers/msaa.wgsl:42-146) — every pixel against the oracle: four keys per pixel bit-exact over the whole
    frame, the resolved colours at the same bar."""
    sc = scenes.atrium_scene(3840, 2160)
    model = helpers.build_model(sc)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=4, mipmap=True)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=4, mipmap=True, threads=_host_threads())
    r = _assert_full_frame("configs[3] atrium 3840x2160 MSAA x4 + gradient mips", orc, dev, stats)
    assert r["covered"] > 8_000_000
    ranks = orc.keys & np.uint64(0xFFFFFFFF)
    assert 0.02 < float((ranks != ranks[..., :1]).any(axis=2).mean()) < 0.9          # both outcomes of the edge test are in the frame
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", [2, 3])
def test_full_size_configs_2_and_3(config, oracle_lut):
    """BASELINE configs[1] (helmet-class mesh, one PBR material, five 2048^2 textures) and configs[2] (61k-triangle skinned rig + morph
    cube) at their stated 1920x1080: every pixel against the oracle (round 5), then the size-independent properties — a re-render is bit-identical,
    band shards reproduce the unsharded rows, the covered-pixel count equals the visibility buffer's."""
    sc = scenes.helmet_scene() if config == 2 else scenes.skinned_morph_scene()
    assert (sc.width, sc.height) == (1920, 1080)
    if config == 2:
        assert scenes.total_triangles(sc) > 15000 and all(t.shape[0] == 2048 for t in sc.textures)
    else:
        assert scenes.total_triangles(sc) > 60000
    model = helpers.build_model(sc)
    dev, stats = helpers.hip_frame(model, oracle_lut)
    keys, img = dev.read_visibility(), dev.read_opaque()
    hit = keys != helpers.NO_HIT
    assert stats["covered_pixels"] == int(hit.sum()) > 100_000
    orc = helpers.oracle_frame(model, oracle_lut, threads=_host_threads())
    _assert_full_frame("configs[%d] %s 1920x1080" % (config - 1, "helmet" if config == 2 else "skinned+morph"), orc, dev, stats)
    del orc
    draws = model.collect_draws()
    dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
    assert (dev.read_visibility() == keys).all() and (dev.read_opaque() == img).all()           # deterministic
    from awsm_renderer_amd import sharding
    dev.set_shard_bands(3, 1)
    dev.geometry_pass(draws); dev.opaque_pass(); dev.frame_end()
    mine = np.array(sharding.band_rows(sc.height, 3, 1))
    assert (dev.read_visibility()[mine] == keys[mine]).all() and (dev.read_opaque()[mine] == img[mine]).all()
    dev.close()


def _digest_of(keys):
    k = keys.reshape(-1).astype(np.uint64)
    i = np.arange(k.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = int((k * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))
        r = i & np.uint64(63)
        x = int(np.bitwise_xor.reduce((k << r) | np.where(r != 0, k >> ((np.uint64(64) - r) & np.uint64(63)), np.uint64(0))))
    return s, x


@pytest.mark.gpu
@pytest.mark.parametrize("msaa", [0, 4])
def test_split_tile_handoff_is_stable_over_500_frames(msaa, oracle_lut):
    """k_raster_tile hands partial tiles of lists longer than 256 triangles between workgroups on different XCDs (sc1 scratch stores,
    every storing wavefront's s_waitcnt vmcnt(0), barrier, arrival counter; the last arriver folds the slices).  geometry/render_pass.rs:51-157:
    every draw's fragments land, every frame.  500 geometry passes of the 4K atrium (it has tiles with > 256 distinct visible triangles,
    test_full_size_4k_frame_properties) must reproduce frame 0's key buffer exactly; compared through a device-side digest, which is itself
    checked against the keys read back."""
    sc = scenes.atrium_scene(3840, 2160, tex_scale=1 / 16)      # the geometry of BASELINE configs[3]; textures play no part here
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    keys = dev.read_visibility()
    k0 = keys[..., 0] if msaa == 4 else keys
    ranks = (k0[:2144] & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(67, 32, 120, 32).transpose(0, 2, 1, 3).reshape(67, 120, 1024)
    srt = np.sort(ranks, axis=2)
    assert int((1 + (srt[:, :, 1:] != srt[:, :, :-1]).sum(axis=2)).max()) > 256        # some tile's list is certainly split
    d0 = dev.visibility_digest()
    assert d0 == _digest_of(keys)
    draws = model.collect_draws()
    bad = []
    for i in range(500):
        dev.geometry_pass(draws)
        d = dev.visibility_digest()
        if d != d0:
            bad.append(i)
    stats = dev.frame_end()
    dev.close()
    assert not bad, f"{len(bad)} of 500 frames differ from frame 0 (first: {bad[:5]})"
    assert stats["bin_overflow_retries"] == 0


# ------------------------------------------------------------------------------------------------ MSAA x4 (the reference's default AntiAliasing)
def _check_msaa(scene, lut):
    model = helpers.build_model(scene)
    orc = helpers.oracle_frame(model, lut, msaa=4)
    dev, stats = helpers.hip_frame(model, lut, msaa=4)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    dev.close()
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0 and r["key_mismatch"] == 0, r      # four samples per pixel, bit-exact
    assert stats["covered_pixels"] == r["covered"] > 0, (stats, r)
    assert r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    return orc


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "helmet", "skinned_morph", "atrium", "zoo"])
def test_msaa4_geometry_and_edge_resolve(name, oracle_lut):
    """resize(.., msaa=4): per-sample visibility keys bit-exact; edge detection (strict) + per-sample resolve within the
    shading tolerance.  A flipped edge decision would show up as a large error on that pixel."""
    sc = {"box": lambda: scenes.box_scene(160, 120), "helmet": lambda: scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=64),
          "skinned_morph": lambda: scenes.skinned_morph_scene(320, 200, around=16, along=24, tex_size=16),
          "atrium": lambda: scenes.atrium_scene(641, 363, detail=0.25, tex_scale=1 / 32),
          "zoo": lambda: scenes.material_zoo_scene(400, 300)}[name]()
    orc = _check_msaa(sc, oracle_lut)
    if name == "atrium":   # the scene must actually exercise both outcomes of the edge test
        ranks = orc.keys & np.uint64(0xFFFFFFFF)
        assert 0.05 < float((ranks != ranks[..., :1]).any(axis=2).mean()) < 0.95


@pytest.mark.gpu
def test_msaa4_band_sharding_needs_the_halo_and_switching_back(oracle_lut):
    from awsm_renderer_amd.hip_backend import HipDevice, AwsmHipError
    sc = scenes.box_scene(96, 64)
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    dev.set_shard_bands(2, 0)                              # bands + MSAA: allowed, but the opaque pass needs the neighbours' boundary keys
    dev.geometry_pass(model.collect_draws())
    with pytest.raises(AwsmHipError, match="halo"):
        dev.opaque_pass()
    dev.resize(sc.width, sc.height, 0)                       # back to single-sample on the same context
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
    orc = helpers.oracle_frame(model, oracle_lut)
    assert (dev.read_visibility() == orc.keys).all()
    with pytest.raises(AwsmHipError):
        dev.resize(sc.width, sc.height, 2)
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_msaa4_band_sharding_with_halo_exchange(n, oracle_lut):
    """MSAA x4 + bands: after the geometry pass every rank exports the sample-0 keys of its bands' first and last rows, the arrays are
    gathered in rank order (here: a torch.stack on the one GPU; with real ranks the frame's one RCCL all-gather), bound, and the opaque
    pass's edge detector reads its vertical neighbours across band borders from them.  Every owned row must equal the unsharded
    MSAA frame bit for bit — keys (4 samples) and resolved colours; 363 rows: the last band is partial, n = 3 leaves ranks with
    unequal band counts."""
    import torch
    from awsm_renderer_amd import sharding
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.atrium_scene(641, 363, detail=0.25, tex_scale=1 / 32)
    W, H = sc.width, sc.height
    model = helpers.build_model(sc)
    ref, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    want_keys, want = ref.read_visibility(), ref.read_opaque()
    ref.close()
    devs, mine = [], []
    for r in range(n):
        dev = HipDevice(parity_tap=False)
        dev.resize(W, H, 4)
        dev.upload_mirrors(model.mirrors())
        for i, t in enumerate(model.texture_arrays()):
            dev.texture_array_upload(i, t["texels"])
        for i, smp in enumerate(sc.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib_rgba16f(oracle_lut))
        dev.set_shard_bands(n, r)
        dev.geometry_pass(model.collect_draws())
        L = dev.msaa_halo_bands()
        assert L == -(-(-(-H // 32)) // n)
        buf = torch.zeros((L, 2, W), dtype=torch.int64, device="cuda")
        dev.msaa_halo_export(buf.data_ptr(), L * 2 * W * 8)
        devs.append(dev); mine.append(buf)
    for dev in devs:
        dev.frame_end()
    gathered = torch.stack(mine).contiguous()                       # [n][L][2][W]
    for r, dev in enumerate(devs):
        dev.msaa_halo_bind(gathered.data_ptr(), gathered.numel() * 8)
        dev.opaque_pass(); dev.frame_end()
        rows = np.array(sharding.band_rows(H, n, r))
        assert (dev.read_visibility()[rows] == want_keys[rows]).all()
        got = dev.read_opaque()
        assert (got[rows] == want[rows]).all(), (r, int((got[rows] != want[rows]).any(axis=2).sum()))
        dev.close()


@pytest.mark.gpu
def test_msaa4_through_host_layer(oracle_lut):
    """AwsmRenderer::set_anti_aliasing(Some(4)) through the C++ host: same bar; switching back to None re-renders single-sampled."""
    sc = scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=64)
    model = helpers.build_model(sc)
    orc4 = helpers.oracle_frame(model, oracle_lut, msaa=4)
    r, dev, stats = helpers.host_frame(sc, oracle_lut, msaa=4)
    res = helpers.compare_frames(orc4, dev, rgb_tol=RGB_TOL)
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["f16_max_ulp"] <= 2 and stats["covered_pixels"] == res["covered"], (res, stats)
    assert r.host.pick(160, 90) == dev.pick(160, 90)[0]
    r.host.set_anti_aliasing(0, False)
    dev.msaa = 0
    r.render(sync=True)
    orc1 = helpers.oracle_frame(model, oracle_lut)
    res1 = helpers.compare_frames(orc1, dev, rgb_tol=RGB_TOL)
    assert res1["key_mismatch"] == 0 and res1["rgb_over_tol"] == 0, res1
    with pytest.raises(Exception):
        r.host.set_anti_aliasing(2)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [(0, 121), (121, 250), (250, 363), (96, 97)])
def test_msaa4_row_strips_carry_the_edge_detector_halo(oracle_lut, rows):
    """MSAA + set_shard_rows: the geometry pass rasterises one extra row on each side of the strip so that the edge detector
    sees the same neighbours as in the unsharded frame; the strip's rows of the image are bit-identical to the full frame's."""
    sc = scenes.atrium_scene(641, 363, detail=0.25, tex_scale=1 / 32)
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut, msaa=4)
    full_img, full_f32, full_keys = dev.read_opaque(), dev.read_opaque_f32(), dev.read_visibility()
    dev.set_shard_rows(*rows)
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); st = dev.frame_end()
    y0, y1 = rows
    assert (dev.read_visibility()[y0:y1] == full_keys[y0:y1]).all()
    assert (dev.read_opaque_f32()[y0:y1].view(np.uint32) == full_f32[y0:y1].view(np.uint32)).all()
    assert (dev.read_opaque()[y0:y1] == full_img[y0:y1]).all()
    assert st["covered_pixels"] == int((full_keys[y0:y1] != helpers.NO_HIT).any(axis=2).sum())
    dev.close()


# ------------------------------------------------------------------------------------------------ MipmapMode::Gradient
@pytest.mark.gpu
def test_mip_chain_generation_bit_exact():
    """awsm_hip_texture_array_generate_mips == the oracle's restatement of renderer-core generate_mipmaps, every level, every
    MipmapTextureKind, power-of-two / odd / 1-texel-wide extents; RGBA8 bit for bit."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from oracle import oracle_lib
    rng = np.random.default_rng(11)
    dev = HipDevice()
    dev.resize(16, 16, 0)
    shapes = [(9, 64, 64), (3, 20, 12), (2, 33, 7), (1, 1, 16), (4, 16, 1), (1, 1, 1), (2, 128, 32)]
    for idx, (layers, h, w) in enumerate(shapes):
        tex = rng.integers(0, 256, size=(layers, h, w, 4), dtype=np.uint8)
        tex[0, :, :, :3] = 128                                  # a flat normal map: renormalisation of (0,0,0) -> NaN -> 0
        kinds = [(k % 9) for k in range(1, layers + 1)]
        chain, levels = oracle_lib.mip_chain(tex, kinds)
        dev.texture_array_upload(idx, tex, mips=levels)
        dev.texture_array_generate_mips(idx, kinds)
        for l in range(levels):
            want = oracle_lib.mip_level_view(chain, w, h, layers, l)
            got = dev.texture_array_read_level(idx, l)
            assert got.shape == want.shape and (got == want).all(), (layers, h, w, l, int((got != want).sum()))
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,msaa", [("helmet", 0), ("atrium", 0), ("zoo", 0), ("skinned_morph", 0), ("atrium", 4), ("zoo", 4)])
def test_gradient_mipmaps(name, msaa, oracle_lut):
    """AwsmOpaqueParams.mipmap = 1 (MipmapMode::Gradient, the reference's default): barycentric-derivative reconstruction,
    per-texture UV gradients, LOD selection and trilinear sampling from the generated chains, same parity bar."""
    sc = {"helmet": lambda: scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256),
          "skinned_morph": lambda: scenes.skinned_morph_scene(320, 200, around=16, along=24, tex_size=64),
          "atrium": lambda: scenes.atrium_scene(641, 363, detail=0.25, tex_scale=1 / 8),
          "zoo": lambda: scenes.material_zoo_scene(400, 300)}[name]()
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa, mipmap=True)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=msaa, mipmap=True)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    if name == "atrium" and msaa == 0:      # the mips must matter: the unmipped frame differs visibly
        base = helpers.oracle_frame(model, oracle_lut)
        assert float(np.abs(base.rgba32f - orc.rgba32f).max()) > 0.02
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,msaa,transparent", [("atrium", 0, False), ("zoo", 0, True), ("atrium", 4, False), ("helmet", 0, False)])
def test_anisotropic_probes(name, msaa, transparent, oracle_lut):
    """AWSM_CFG_ANISOTROPIC: MipmapMode::Gradient honours the samplers' max_anisotropy (16 on every linear sampler of these scenes, as the reference's glTF
    ingest sets it) — N = clamp(rho_max / rho_min, 1, 16), the level for rho_max / N, weighted probes along the major axis (tests/test_anisotropic_cpu.py
    holds the rule's properties; here the HIP samplers against the oracle's, same parity bar, opaque and transparent pass).  Draws with such samplers
    leave the lean route under the flag: the general kernels' <2> instantiations carry the probes."""
    sc = {"helmet": lambda: scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256),
          "atrium": lambda: scenes.atrium_scene(641, 363, detail=0.25, tex_scale=1 / 8),
          "zoo": lambda: scenes.material_zoo_scene(400, 300)}[name]()
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa, mipmap=True, anisotropic=True)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=msaa, mipmap=True, anisotropic=True, transparent=transparent)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    if transparent:
        orc.forward(model.collect_transparent_draws())
        c = helpers.compare_composite(orc, dev)
        helpers.assert_composite("anisotropic zoo", c)
    if name == "atrium" and msaa == 0:      # the probes must matter: a visible share of the frame differs from the isotropic rule's
        iso = helpers.oracle_frame(model, oracle_lut, mipmap=True)
        assert float((np.abs(iso.rgba32f - orc.rgba32f).max(axis=-1) > 2e-3).mean()) > 0.02
        # ... and a context without the flag still renders the isotropic frame with the same samplers
        dev2, _ = helpers.hip_frame(model, oracle_lut, mipmap=True)
        r2 = helpers.compare_frames(iso, dev2, rgb_tol=RGB_TOL)
        assert r2["rgb_over_tol"] == 0, r2
        dev2.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "mips", "msaa_mips", "aniso"])
def test_shared_texture_transform_stays_on_the_lean_route(mode, oracle_lut):
    """KHR_texture_transform on every texture of a material (the usual way to tile one): the lean kernel applies the draw's ONE transform to the pixel's
    TEXCOORD_0 and its derivatives before all fetches (LeanDrawDev.tt) — no wavefront goes to the general kernel, colours within the parity bar.  With two
    different transforms in one material the draw is not lean and the general route shades it, same bar."""
    from awsm_renderer_amd.scene_desc import TextureRef
    xf = {"offset": (0.13, -0.21), "origin": (0.5, 0.5), "rotation": 0.4, "scale": (2.7, 1.6)}
    xf2 = {"offset": (0.0, 0.3), "origin": (0.0, 0.0), "rotation": -0.2, "scale": (1.5, 1.5)}
    kw = {"none": {}, "mips": {"mipmap": True}, "msaa_mips": {"mipmap": True, "msaa": 4}, "aniso": {"mipmap": True, "anisotropic": True}}[mode]
    for shared in (True, False):
        ov = {"base_color_tex": TextureRef(0, transform=xf), "metallic_roughness_tex": TextureRef(1, transform=xf), "normal_tex": TextureRef(2, transform=xf),
              "occlusion_tex": TextureRef(3, transform=xf), "emissive_tex": TextureRef(4, transform=xf if shared else xf2)}
        sc = scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256, material_overrides=ov)
        model = helpers.build_model(sc)
        orc = helpers.oracle_frame(model, oracle_lut, **kw)
        dev, stats = helpers.hip_frame(model, oracle_lut, **kw)
        r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
        assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, (shared, r)
        assert (stats["shade_general_wavefronts"] == 0) == shared, (shared, stats)
        if shared and mode == "none":      # the transform must matter: the untransformed frame differs visibly
            base = helpers.oracle_frame(helpers.build_model(scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256)), oracle_lut)
            assert float(np.abs(base.rgba32f - orc.rgba32f).max()) > 0.02
        dev.close()
    # two meshes side by side, each material with a shared transform of its own (and a third without): strips that straddle draws take the per-lane
    # form of the same code
    import copy
    from awsm_renderer_amd.scene_desc import NodeDesc
    sc = scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256, material_overrides={k: TextureRef(i, transform=xf) for i, k in enumerate(
        ("base_color_tex", "metallic_roughness_tex", "normal_tex", "occlusion_tex", "emissive_tex"))})
    for j, t in enumerate((xf2, None)):
        m = copy.deepcopy(sc.materials[0])
        for k in ("base_color_tex", "metallic_roughness_tex", "normal_tex", "occlusion_tex", "emissive_tex"):
            getattr(m, k).transform = t
        sc.materials.append(m)
        prim = copy.copy(sc.nodes[0].primitives[0]); prim.material = j + 1
        sc.nodes.append(NodeDesc(translation=(0.55 * (j + 1), 0.1 * j, -0.3 * (j + 1)), rotation=sc.nodes[0].rotation, scale=(0.8, 0.8, 0.8), primitives=[prim]))
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, **kw)
    dev, stats = helpers.hip_frame(model, oracle_lut, **kw)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    assert stats["shade_general_wavefronts"] == 0, stats
    dev.close()


@pytest.mark.gpu
def test_anisotropic_probes_through_the_host_layer_and_a_glb_file(oracle_lut, tmp_path):
    """The product path with AWSM_CFG_ANISOTROPIC: SceneDesc -> .glb (samplers carry max_anisotropy) -> native reader -> C++ host layer -> HIP kernels,
    against the oracle fed from the same scene."""
    from awsm_renderer_amd import gltf_export
    sc = scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=256)
    path = str(tmp_path / "helmet.glb")
    gltf_export.write_glb(sc, path)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, mipmap=True, anisotropic=True)
    r, dev, stats = helpers.host_frame(sc, oracle_lut, mipmap=True, gltf=path, anisotropic=True)
    res = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["f16_max_ulp"] <= 2, res
    r.close()


@pytest.mark.gpu
def test_reference_default_anti_aliasing_through_host_layer(oracle_lut):
    """AntiAliasing::default() = {msaa_sample_count: Some(4), mipmap: true} (anti_alias.rs:28-38) through the C++ host: the
    host generates every array's mip chain with the per-role kinds and selects the MSAA + gradient pipeline."""
    sc = scenes.atrium_scene(480, 270, detail=0.25, tex_scale=1 / 16)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=4, mipmap=True)
    r, dev, stats = helpers.host_frame(sc, oracle_lut, msaa=4, mipmap=True)
    res = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["f16_max_ulp"] <= 2 and stats["covered_pixels"] == res["covered"], (res, stats)
    r.close()


@pytest.mark.gpu
def test_integer_raster_walk_around_its_size_limit(oracle_lut):
    """k_raster_tile steps the edge functions of 'small' exact triangles (extent <= 21000 sub-pixels = 82 px, raster_setup.hpp) in 32-bit integers,
    the others in f64.  900 random triangles whose screen extents straddle that limit (40 .. 130 px), at every screen position of a 1920x1080
    frame including across its borders, double-sided, overlapping at random depths, a third of them sharing edges with a neighbour (top-left
    rule): every key equals the oracle's (which knows one arithmetic only), single-sampled and with MSAA (per-sample constants on the same integers)."""
    import math
    from awsm_renderer_amd.scene_desc import SceneDesc, NodeDesc, PrimitiveDesc, MaterialDesc
    from awsm_renderer_amd.scenes import look_at_rh, perspective_rh, REPEAT_LINEAR, DEFAULT_LIGHTS
    rng = np.random.default_rng(82)
    W, H = 1920, 1080
    fov = math.radians(50.0)
    dist = 10.0
    px_per_unit = (H / 2) / (math.tan(fov / 2) * dist)          # pixels per world unit on the plane z = 0
    pos, idx = [], []
    for k in range(900):
        ext = rng.uniform(40.0, 130.0) / px_per_unit
        c = np.array([rng.uniform(-1.05, 1.05) * (W / 2) / px_per_unit, rng.uniform(-1.05, 1.05) * (H / 2) / px_per_unit, rng.uniform(-2.0, 2.0)])
        a = c + np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)]) * ext
        b = a + np.array([ext, rng.uniform(-1.0, 1.0) * ext * 0.5, rng.uniform(-0.3, 0.3) * ext])
        d = a + np.array([rng.uniform(0.0, 1.0) * ext, rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0) * ext, rng.uniform(-0.3, 0.3) * ext])
        o = len(pos)
        pos += [a, b, d]
        idx.append([o, o + 1, o + 2])
        if k % 3 == 0:      # a neighbour across the edge a-b
            e = a + b - d + np.array([0.0, 0.0, rng.uniform(-0.2, 0.2) * ext])
            pos.append(e)
            idx.append([o + 1, o, o + 3])
    pos = np.array(pos, dtype=np.float32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (pos.shape[0], 1))
    prim = PrimitiveDesc(positions=pos, normals=nrm, indices=np.array(idx, dtype=np.uint32), material=0)
    eye = (0.0, 0.0, dist)
    sc = SceneDesc(nodes=[NodeDesc(primitives=[prim])], materials=[MaterialDesc(base_color_factor=(0.7, 0.6, 0.5, 1.0), metallic_factor=0.0, double_sided=True)],
                   samplers=[dict(REPEAT_LINEAR)], lights=list(DEFAULT_LIGHTS), width=W, height=H,
                   view=look_at_rh(eye, (0, 0, 0)), proj=perspective_rh(fov, W / H, 0.1, 100.0), camera_position=eye)
    model = helpers.build_model(sc)
    from oracle import oracle_lib
    for msaa in (0, 4):
        fr = oracle_lib.frame_from_model(model, oracle_lut, msaa=msaa).transform().raster(16)
        dev, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa)
        keys = dev.read_visibility()
        assert keys.shape == fr.keys.shape
        assert (keys == fr.keys).all(), (msaa, int((keys != fr.keys).sum()))
        assert int((fr.keys != np.uint64(0xFFFFFFFFFFFFFFFF)).sum()) > 200000
        dev.close()


@pytest.mark.gpu
def test_stream_handoff_flags_events_and_timeout_fallback(oracle_lut, monkeypatch):
    """The overlapped pipeline hands a frame from stream to stream through device-side flags (k_handoff_signal / k_handoff_wait) instead of
    cross-stream events.  48 frames with a moving camera, submitted without a synchronisation, each into its own image: bit-identical to a
    plain context's frames with the flags (the default: awsm_hip_stream_handoff() == 1) and with AWSM_DEVICE_HANDOFF=0 (events).  Then the
    failure path: one geometry-done signal withheld (AWSM_TEST_HANDOFF_DROP) with a short time budget — the gate gives up and FAILS CLOSED: the
    frame it guarded is dropped whole (its image keeps the pattern it held), awsm_hip_frame_flush / frame_end report it once, the counter says one
    gate, the context goes on with events and renders correct frames again."""
    import ctypes as C
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    from awsm_renderer_amd.scenes import look_at_rh
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sc = scenes.atrium_scene(480, 270, detail=0.25, tex_scale=1 / 16)
    n = 48
    eyes = [(0.4 + 0.11 * i, 3.1 + 0.03 * i, 17.0 - 0.6 * i) for i in range(n)]
    lut = oracle_lib_rgba16f(oracle_lut)
    nbytes = sc.height * sc.width * 8

    def run(overlap, want_handoff):
        r = Renderer(sc, lut_rgba16f=lut, overlap_frames=overlap)
        r.host.set_render_timings(False)
        dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
        assert dev.stream_handoff() == want_handoff
        outs = []
        for _ in eyes:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            outs.append(p)
        for i, eye in enumerate(eyes):
            r.host.camera_update(look_at_rh(eye, (-0.2, 3.4, -18.0)), sc.proj, eye)
            dev.bind_output(outs[i].value, nbytes)
            r.host.render(sync=not overlap)
        dev.frame_flush()
        assert hip.hipDeviceSynchronize() == 0
        imgs = []
        for p in outs:
            a = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0
            imgs.append(a)
            hip.hipFree(p)
        dev.bind_output(None)
        r.close()
        return imgs

    plain = run(False, 0)
    flags = run(True, 1)
    monkeypatch.setenv("AWSM_DEVICE_HANDOFF", "0")
    events = run(True, 0)
    monkeypatch.delenv("AWSM_DEVICE_HANDOFF")
    for i, (a, b, e) in enumerate(zip(plain, flags, events)):
        assert (a == b).all(), f"flags, frame {i}: {(a != b).sum()} values differ"
        assert (a == e).all(), f"events, frame {i}: {(a != e).sum()} values differ"
    assert not (plain[0] == plain[n - 1]).all()

    monkeypatch.setenv("AWSM_TEST_HANDOFF_DROP", "1")
    monkeypatch.setenv("AWSM_HANDOFF_TIMEOUT_MS", "5")
    r = Renderer(sc, lut_rgba16f=lut, overlap_frames=True)
    r.host.set_render_timings(False)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    assert dev.stream_handoff() == 1
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    img = C.c_void_p()
    assert hip.hipMalloc(C.byref(img), nbytes) == 0 and hip.hipMemset(img, 0x5A, nbytes) == 0 and hip.hipDeviceSynchronize() == 0
    r.host.camera_update(look_at_rh(eyes[0], (-0.2, 3.4, -18.0)), sc.proj, eyes[0])
    dev.bind_output(img.value, nbytes)
    r.host.render(sync=False)            # its opaque pass starts behind a gate nobody opens: the gate times out and poisons the frame
    assert hip.hipDeviceSynchronize() == 0
    got = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
    assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), img, nbytes, 2) == 0
    assert (got == 0x5A5A).all(), f"the withheld frame wrote {(got != 0x5A5A).sum()} values: a timed-out gate must drop its frame, not shade it"
    with pytest.raises(Exception, match="hand-off timed out"):      # an enqueue-only caller hears of it too
        dev.frame_flush()
    assert dev.stream_handoff() == 0
    dev.bind_output(None)
    hip.hipFree(img)
    for i in (5, 17):
        r.host.camera_update(look_at_rh(eyes[i], (-0.2, 3.4, -18.0)), sc.proj, eyes[i])
        r.host.render(sync=False)
        st = r.host.render(sync=True)      # said once: no second error
        assert st["handoff_gate_timeouts"] == 1, st
        assert (dev.read_opaque() == plain[i]).all(), i
    r.close()


@pytest.mark.gpu
def test_device_brdf_lut_against_the_oracle(oracle_lut):
    """BrdfLut::new (renderer-core/src/brdf_lut/generate.rs:47-96, shader.wgsl:1-78) on the device: k_brdf_lut through
    awsm_hip_brdf_lut_generate / awsm_hip_read_brdf_lut against oracle/c/oracle_brdf_lut.c, at the test size (64^2) and at the reference's default
    (1024^2).  The kernel and the oracle sum the same 1,024 samples per texel in the same order; what differs is the math library (device sin / cos /
    pow against glibc's), so the bound is stated in f16 steps of the stored texel: at most 1 step, and all but a fraction of the texels identical.
    Then a frame shaded with the DEVICE's LUT against the oracle's frame with the ORACLE's LUT, within the shading tolerance: what a caller
    without a LUT of its own (bench.py, Renderer(lut_rgba16f=None)) gets."""
    from awsm_renderer_amd.hip_backend import HipDevice
    for n in (64, 1024):
        dev = HipDevice()
        dev.brdf_lut_generate(n, n)
        got = dev.read_brdf_lut()
        dev.close()
        want = oracle_lut if n == 64 else oracle_lib.brdf_lut(n, n, threads=os.cpu_count() or 8)
        assert got.shape == want.shape == (n, n, 2)
        step = np.abs(got.astype(np.int32) - want.astype(np.int32))      # positive finite f16 values: the bit patterns are ordered like the values
        assert (got < 0x7C00).all() and (want < 0x7C00).all()
        assert step.max() <= 1, f"{n}^2: a texel differs by {step.max()} f16 steps"
        assert (step != 0).mean() < 0.02, f"{n}^2: {(step != 0).mean():.4f} of the values differ by one step"
    from awsm_renderer_amd.host import Renderer
    scene = scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=64)
    r = Renderer(scene, parity_tap=True, lut_rgba16f=None, lut_size=64)       # the device generates its own LUT
    r.render(sync=True)
    dev = HipDevice.from_ctx(r.host.device_ctx, scene.width, scene.height)
    res = helpers.compare_frames(helpers.oracle_frame(helpers.build_model(scene), oracle_lut), dev)
    dev.close()
    r.close()
    assert res["key_mismatch"] == 0 and res["clip_mismatch"] == 0, res
    assert res["rgb_over_tol"] == 0 and res["f16_max_ulp"] <= 2, res


@pytest.mark.gpu
@pytest.mark.parametrize("aa", [dict(), dict(msaa=4, mipmap=True)], ids=["single", "msaa_mips"])
def test_overlapped_frames_shade_what_was_submitted(aa, oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES: the opaque pass of frame i runs on the library's shade stream while the geometry pass of frame
    i+1 is already enqueued.  Six frames with a moving camera (and a material change half-way) are submitted without any
    synchronisation in between, each into its own output image; every image must be bit-identical to the same frame
    rendered on a plain (non-overlapping) context.  Also with MSAA x4 + mipmaps: the MSAA scratch is per frame slot, so frame i + 1's lean kernel runs
    beside frame i's edge detector and resolve."""
    import ctypes as C
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer, material_struct
    from awsm_renderer_amd.scenes import look_at_rh
    hip = C.CDLL("libamdhip64.so")        # the runtime the library itself uses (torch would bring a second copy into this process)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sc = scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 16)
    eyes = [(0.4 + 0.3 * i, 3.1 + 0.1 * i, 17.0 - 1.5 * i) for i in range(6)]
    lut = oracle_lib_rgba16f(oracle_lut)
    nbytes = sc.height * sc.width * 8

    def run(overlap, timers=True):
        r = Renderer(sc, lut_rgba16f=lut, overlap_frames=overlap, **aa)
        r.host.set_render_timings(timers)      # off: no stage events, and the per-draw resolve moves ahead of the wait for the geometry pass
        dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
        outs = []
        for _ in eyes:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            outs.append(p)
        for i, eye in enumerate(eyes):
            r.host.camera_update(look_at_rh(eye, (-0.2, 3.4, -18.0)), sc.proj, eye)
            if i == 3:   # a scene write other than the camera: must wait for the opaque passes in flight
                m = sc.materials[0]
                m2 = type(m)(**{**m.__dict__, "base_color_factor": (0.2, 0.9, 0.3, 1.0)})
                r.host.material_update(r.keys.material_keys[0], material_struct(m2, r.host, {}))
            dev.bind_output(outs[i].value, nbytes)
            r.host.render(sync=not overlap)
        dev.frame_flush()
        assert hip.hipDeviceSynchronize() == 0
        imgs = []
        for p in outs:
            a = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0      # hipMemcpyDeviceToHost
            imgs.append(a)
        dev.bind_output(None)
        r.close()
        for p in outs:
            hip.hipFree(p)
        return imgs

    plain, over, over_quiet = run(False), run(True), run(True, timers=False)
    for i, (a, b, q) in enumerate(zip(plain, over, over_quiet)):
        assert (a == b).all(), f"frame {i}: {(a != b).sum()} values differ"
        assert (a == q).all(), f"frame {i} without stage timers: {(a != q).sum()} values differ"
    assert not (plain[0] == plain[5]).all() and not (plain[2] == plain[3]).all()

    # The same six frames into the library's own images (one per frame slot: nothing orders two frames' opaque passes then, and the per-draw
    # records are reused while only the camera moves): after any number of frames read_opaque is the last one submitted.
    r = Renderer(sc, lut_rgba16f=lut, overlap_frames=True, **aa)
    r.host.set_render_timings(False)
    dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
    for i, eye in enumerate(eyes):
        r.host.camera_update(look_at_rh(eye, (-0.2, 3.4, -18.0)), sc.proj, eye)
        if i == 3:
            m = sc.materials[0]
            r.host.material_update(r.keys.material_keys[0], material_struct(type(m)(**{**m.__dict__, "base_color_factor": (0.2, 0.9, 0.3, 1.0)}), r.host, {}))
        r.host.render(sync=False)
        if i in (1, 4, 5):
            got = dev.read_opaque()
            assert (got == plain[i]).all(), f"own image, frame {i}: {(got != plain[i]).sum()} values differ"
    r.close()


def oracle_lib_rgba16f(lut):
    from oracle import oracle_lib
    return oracle_lib.lut_rg_to_rgba16f(lut)


# ------------------------------------------------------------------------------------------------ GPU instancing
@pytest.mark.gpu
@pytest.mark.parametrize("msaa", [0, 4])
def test_instanced_meshes(msaa, oracle_lut):
    """AwsmDraw.inst_off / inst_count: one draw per instanced mesh, model * instance per vertex, instances rasterised in order.
    C-ABI path and host-layer path (awsm_host_mesh_set_instances), same bar; the picker reports the instanced mesh."""
    sc = scenes.instanced_scene(640, 360)
    model = helpers.build_model(sc)
    draws = model.collect_draws()
    assert sorted(d.get("inst_count", 0) for d in draws) == [0, 0, 9, 24]
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0 and r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["f16_max_ulp"] <= 2, r
    assert stats["triangles_in"] == sum(d["tri_count"] * max(1, d.get("inst_count", 0)) for d in draws)
    tri, meta, _ = dev.read_visibility_unpacked()
    otri, ometa, _ = orc.unpack_visibility()
    assert (tri == otri).all() and (meta == ometa).all()        # primitive-local triangle ids, whichever instance was hit
    dev.close()
    rr, hdev, _ = helpers.host_frame(sc, oracle_lut, msaa=msaa)
    res = helpers.compare_frames(orc, hdev, rgb_tol=RGB_TOL)
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0, res
    from awsm_renderer_amd import scene_desc  # noqa: F401
    assert rr.host.mirror(helpers.scene_model.BUF_INSTANCES) == model.mirrors()[helpers.scene_model.BUF_INSTANCES]
    rr.close()


# ------------------------------------------------------------------------------------------------ the two opaque routes

@pytest.mark.gpu
def test_lean_and_general_opaque_routes_agree(oracle_lut):
    """k_shade_lean + k_shade_todo against k_shade (AWSM_CFG_GENERAL_SHADE_ONLY) on the same frames: same keys, colours within the
    shading tolerance of each other (same formulas, different instruction order; all but a thousandth of the pixels within a fifth of it).  The atrium is all lean; the zoo mixes lean
    draws with every kind that is not (unlit, optional blocks, debug views, non-repeat samplers, texture transforms), so wavefronts that
    straddle both kinds go to the general kernel; the scene below adds texture coordinates in the millions, beyond the lean sampler's range."""
    from awsm_renderer_amd.hip_backend import HipDevice
    big_uv = scenes.helmet_scene(320, 180, segments=32, rings=24, tex_size=32)
    for n in big_uv.nodes:
        for p in n.primitives:
            p.uvs = [uv * np.float32(3.0e6) for uv in p.uvs]
    cases = {"atrium": scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 32), "zoo": scenes.material_zoo_scene(400, 300), "huge_uv": big_uv}
    for name, sc in cases.items():
        model = helpers.build_model(sc)
        lean, st_lean = helpers.hip_frame(model, oracle_lut)
        gen, st_gen = helpers.hip_frame(model, oracle_lut, dev=HipDevice(parity_tap=True, general_shade_only=True))
        a, b = lean.read_opaque_f32().astype(np.float64), gen.read_opaque_f32().astype(np.float64)
        assert (lean.read_visibility() == gen.read_visibility()).all()
        waves = int(st_lean["shade_general_wavefronts"])
        lean.close(); gen.close()
        # each route is within the bar + the pixel's conditioning term of the oracle (the parity tests), so within twice that of the other; asserted
        # here: the plain bar + twice the conditioning term between them, and at most a thousandth of the pixels beyond a fifth of the bar
        orc = helpers.oracle_frame(model, oracle_lut)
        cond = orc.conditioning(os.cpu_count() or 16)
        bound = RGB_TOL * np.maximum(1.0, np.abs(b)) + 2.0 * cond
        assert (np.abs(a - b) <= bound).all(), (name, float((np.abs(a - b) / bound).max()))
        assert int((np.abs(a - b) > 2e-5 * np.maximum(1.0, np.abs(b))).any(axis=2).sum()) <= 1e-3 * a.shape[0] * a.shape[1], name
        assert st_gen["shade_general_wavefronts"] == 0
        total_waves = ((sc.width + 15) // 16) * ((sc.height + 15) // 16) * 4
        if name == "atrium":
            assert waves == 0
        elif name == "zoo":
            assert 0 < waves < total_waves                     # both kernels shaded part of the frame
        else:
            assert waves > 0                                   # the range guard sent covered wavefronts to the general kernel
            assert (np.abs(a - orc.rgba32f.astype(np.float64)) <= RGB_TOL * np.maximum(1.0, np.abs(orc.rgba32f)) + cond).all()


@pytest.mark.gpu
def test_random_viewpoints_gbuffer_exact_and_routes_agree(oracle_lut):
    """A dozen random viewpoints inside the atrium — along walls, up into the arches, through columns at grazing angles, triangles crossing
    the near plane — instead of the scenes' own cameras (tests/diagnostics/viewpoint_survey.py is the exploratory version; it found the basis of
    unpack_normal_tangent blowing one-ulp differences up to 6e-2 where N.z -> -1, now computed with the oracle's operations there).  In EVERY view:
      * keys and the reconstructed G-buffer texel (packed normal / tangent, barycentric: awsm_hip_read_gbuffer) equal the oracle's bit for bit
        in every pixel — the STRICT section, checked value for value rather than through the colour;
      * both opaque routes are within the CONDITIONED bound of the oracle in every pixel, no exceptions:
            |hip - oracle| <= 1e-4 * max(1, |oracle|) + cond,
        cond = how far the oracle's own colour moves when the decoded normal or the reconstructed position is off by 16 ulps
        (OracleFrame.conditioning: four perturbed oracle frames; measured, not modelled).  Ordinary pixels have cond << 1e-4 and hold the plain bar;
        a GGX peak on a near-mirror texel (relative error of D ~ 4 d(n.h) / alpha^4) or a silhouette with n.v -> 0 is allowed exactly what its
        condition number explains.  The test also reports how many pixels needed that (a few per 0.9-Mpixel view);
      * the lean and the general route (separate code over the same formulas) agree within the plain bar + twice cond (each is within bar + cond of the oracle)."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.scenes import look_at_rh
    from oracle import oracle_lib
    rng = np.random.default_rng(20260104)
    sc = scenes.atrium_scene(1280, 720, detail=0.5, tex_scale=1 / 16)
    lean_dev, gen_dev = HipDevice(parity_tap=True), HipDevice(parity_tap=True, general_shade_only=True)
    no_hit = np.uint64(0xFFFFFFFFFFFFFFFF)
    threads = os.cpu_count() or 16
    needed = 0
    for k in range(12):
        eye = (float(rng.uniform(-5.5, 5.5)), float(rng.uniform(0.3, 9.5)), float(rng.uniform(-17.0, 17.0)))
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        if abs(d[1]) > 0.95:
            d = np.array([0.6, 0.5, -0.62])
        target = tuple(float(v) for v in np.asarray(eye) + 10.0 * d)
        sc.view, sc.camera_position = look_at_rh(eye, target), eye
        model = helpers.build_model(sc)
        helpers.hip_frame(model, oracle_lut, dev=lean_dev)
        helpers.hip_frame(model, oracle_lut, dev=gen_dev)
        keys = lean_dev.read_visibility()
        assert (keys == gen_dev.read_visibility()).all(), k
        a, b = lean_dev.read_opaque_f32().astype(np.float64), gen_dev.read_opaque_f32().astype(np.float64)
        fr = oracle_lib.frame_from_model(model, oracle_lut).transform().raster(threads)
        assert (keys == fr.keys).all(), k
        go, gh = fr.gbuffer(threads), lean_dev.read_gbuffer()
        hit = keys != no_hit
        assert not ((go.view(np.uint32) != gh.view(np.uint32)) & hit[..., None]).any(), k
        fr.shade(threads)
        o = fr.rgba32f.astype(np.float64)
        cond = fr.conditioning(threads)
        base = RGB_TOL * np.maximum(1.0, np.abs(o))
        # the conditioned bound must not be a blanket: the typical pixel's condition term is far below the bar, and few pixels have a large one
        ch = cond[hit][:, :3].max(axis=1)
        assert float(np.median(ch)) < 1e-5 and float((ch > RGB_TOL).mean()) < 0.02, (k, float(np.median(ch)), float((ch > RGB_TOL).mean()))
        for name, x in (("lean", a), ("general", b)):
            err = np.abs(x - o)
            over = err > base + cond
            assert not over.any(), (k, name, eye, target, int(over.any(axis=2).sum()), float((err / (base + cond)).max()))
            needed += int((err > base).any(axis=2).sum())
        routes = np.abs(a - b) > base + 2.0 * cond
        assert not routes.any(), (k, "lean vs general", int(routes.any(axis=2).sum()))
    assert needed <= 12 * 2 * 64, needed       # a few ill-conditioned pixels per view and route, not a population
    lean_dev.close(); gen_dev.close()


@pytest.mark.gpu
def test_random_viewpoints_in_every_mode(oracle_lut):
    """The same idea through the other modes (tests/diagnostics/mode_survey.py): three random viewpoints each around the material zoo (every optional
    PBR block, unlit, debug views, sampler modes, point + spot lights; single-sampled and with gradient mipmaps), the helmet, the skinned + morphed
    strip, inside the atrium with MSAA x4 / gradient mipmaps / both / anisotropic probes, and around the transparent scene with its forward pass
    (single-sampled, MSAA).
    Vertices, keys and (single-sampled modes) the reconstructed G-buffer texel bit-exact in every view; colours within the CONDITIONED bound in every
    pixel (1e-4 * max(1, |ref|) + what 16 ulps of input noise do to the oracle's own colour there: helpers.compare_frames, OracleFrame.conditioning), the
    RGBA16F image within two f16 steps wherever the pixel is well conditioned, and at most a handful of pixels per view needing their condition number;
    the composite within two f16 steps everywhere, pixels no fragment reached untouched."""
    from tests.diagnostics import mode_survey
    seen = 0
    for name, k, eye, c, cc in mode_survey.survey(3, lut=oracle_lut):
        tag = (name, k, eye, c, cc)
        assert c["key_mismatch"] == 0 and c["clip_mismatch"] == 0 and c["nt_mismatch"] == 0 and c.get("gbuffer_mismatch", 0) == 0, tag
        assert c["rgb_over_tol"] == 0 and c["f16_max_ulp"] <= 2, tag
        if cc is not None:
            assert cc["clip_mismatch"] == 0 and cc["nt_mismatch"] == 0 and cc["wpos_mismatch"] == 0 and cc["untouched_changed"] == 0, tag
            helpers.report_composite("mode survey %s view %d" % (name, k), cc)
            assert cc["pixels_over_2ulp"] <= 4 and cc["pixels_over_bound"] <= 4 and cc["alpha_mismatch"] == 0, tag
        seen += 1
    assert seen == 3 * len(mode_survey.MODES)


@pytest.mark.gpu
def test_persistent_lean_grid_is_bit_identical(oracle_lut, monkeypatch):
    """k_shade_lean<true> (AWSM_LEAN_WGS_PER_CU workgroups per CU taking 16x4-pixel strips from per-XCD counters; off by default, see
    DESIGN section 6) shades every pixel with the code of the one-wavefront-per-strip grid: same bits, same list for the general kernel.  Frame
    widths below, at and above a power of two of 16-pixel blocks exercise the padded strip numbering; two frames per device reuse the counters."""
    from awsm_renderer_amd.hip_backend import HipDevice
    for name, sc in (("atrium", scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 32)), ("zoo", scenes.material_zoo_scene(400, 300)),
                     ("zoo_pow2", scenes.material_zoo_scene(512, 256)), ("zoo_odd", scenes.material_zoo_scene(531, 173))):
        model = helpers.build_model(sc)
        monkeypatch.delenv("AWSM_LEAN_WGS_PER_CU", raising=False)
        ref, st_ref = helpers.hip_frame(model, oracle_lut)
        want = ref.read_opaque_f32()
        ref.close()
        monkeypatch.setenv("AWSM_LEAN_WGS_PER_CU", "4")
        dev = HipDevice(parity_tap=True)
        for _ in range(2):
            _, st = helpers.hip_frame(model, oracle_lut, dev=dev)
            got = dev.read_opaque_f32()
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), name
            assert st["shade_general_wavefronts"] == st_ref["shade_general_wavefronts"]
        dev.close()


# ------------------------------------------------------------------------------------------------ texel cubemaps

def _with_environment(sc, size=32):
    sc.env_cubes = scenes.procedural_environment(size, 8)
    sc.prefiltered_mip_count = len(sc.env_cubes["prefiltered"])        # what IblTexture.mip_count reports (lights.rs:300-305)
    sc.irradiance_mip_count = 1
    return sc


@pytest.mark.gpu
@pytest.mark.parametrize("name,msaa", [("helmet", 0), ("zoo", 0), ("atrium", 0), ("helmet", 4)])
def test_texel_cubemaps_skybox_and_ibl(name, msaa, oracle_lut):
    """skybox.wgsl:1-41 + brdf.wgsl:268-290,389-576 with real cubemaps: the background is the skybox cube along the pixel's view ray, the
    diffuse term samples the irradiance cube along N, the specular (and clearcoat) term the prefiltered chain along the reflection at level
    roughness * (mips - 1).  A non-uniform HDR environment, so a wrong face, orientation, seam or level shows."""
    sc = {"helmet": lambda: scenes.helmet_scene(480, 270, segments=64, rings=48, tex_size=128), "zoo": lambda: scenes.material_zoo_scene(400, 300),
          "atrium": lambda: scenes.atrium_scene(640, 360, detail=0.25, tex_scale=1 / 32)}[name]()
    _with_environment(sc)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa)
    flat = helpers.oracle_frame(helpers.build_model(dataclasses.replace(sc, env_cubes=None)), oracle_lut, msaa=msaa)
    assert float(np.abs(orc.rgba32f - flat.rgba32f).max()) > 0.5                        # the cubes do change the picture
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=msaa)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    dev.close()
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["alpha_mismatch"] == 0 and r["f16_max_ulp"] <= 2, r
    if name == "atrium":
        assert stats["shade_general_wavefronts"] == 0, stats                            # texel cubes ride the lean route (round 2: any cube sent the frame to k_shade)
    if name == "helmet":
        assert r["covered"] < sc.width * sc.height * 0.6                                # sky pixels are in the comparison
    # through the host layer: Renderer uploads the cubes with awsm_host_env_cube
    rr, hdev, _ = helpers.host_frame(sc, oracle_lut, msaa=msaa)
    res = helpers.compare_frames(orc, hdev, rgb_tol=RGB_TOL)
    rr.close()
    assert res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0, res


@pytest.mark.gpu
def test_texel_cubemap_is_the_transmission_fallback(oracle_lut):
    """material_transparent fragment.wgsl:68-81: a refracted ray that leaves the screen samples the prefiltered cube along the
    refracted direction at roughness * (mips - 1)."""
    sc = _with_environment(scenes.transparent_scene(480, 270, tex_size=64))
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut)
    orc.forward(model.collect_transparent_draws())
    dev, _ = helpers.hip_frame(model, oracle_lut, transparent=True)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    c = helpers.compare_composite(orc, dev)
    dev.close()
    assert r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0, r
    assert c["untouched_changed"] == 0, c
    helpers.assert_composite("transmission fallback to the prefiltered cube", c)


@pytest.mark.gpu
def test_cube_upload_argument_checks_and_reset(oracle_lut):
    from awsm_renderer_amd.hip_backend import AwsmHipError
    sc = scenes.box_scene(160, 120)
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut)
    base = dev.read_opaque()
    env = scenes.procedural_environment(16, 8)
    for k, name in enumerate(("skybox", "prefiltered", "irradiance")):
        dev.env_cube_upload(k, env[name])
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
    assert (dev.read_opaque() != base).any()
    for k in range(3):
        dev.env_cube_upload(k, None)                                                    # back to the uniform colours
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
    assert (dev.read_opaque() == base).all()
    with pytest.raises(AwsmHipError):
        dev._chk(dev.lib.awsm_hip_env_cube_upload(dev.ctx, 0, 16, 9, env["skybox"][0].ctypes.data), "env_cube_upload")      # a 16^2 cube has 5 levels
    with pytest.raises(AwsmHipError):
        dev._chk(dev.lib.awsm_hip_env_cube_upload(dev.ctx, 5, 16, 1, env["skybox"][0].ctypes.data), "env_cube_upload")
    dev.close()


# ------------------------------------------------------------------------------------------------ transparent pass

@pytest.mark.gpu
@pytest.mark.parametrize("msaa,mipmap", [(0, False), (4, False), (0, True), (4, True)])
def test_transparent_pass_matches_the_oracle(msaa, mipmap, oracle_lut):
    """Opaque backdrop + the world transparent pass (alpha blend, mask, vertex-colour alpha, unlit, transmission with and without
    refraction / blur, morph targets, instancing, overlapping layers): transformed vertices bit-exact, pixels no transparent
    fragment reached identical to the opaque image, blended pixels within two f16 steps of the oracle.  The transmission
    background is an integer texel fetch at a position computed by relaxed arithmetic, so isolated pixels may pick the
    neighbouring texel: those are bounded in number, not in value."""
    sc = scenes.transparent_scene(480, 270, tex_size=64)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=msaa, mipmap=mipmap)
    tr = model.collect_transparent_draws()
    assert len(tr) >= 10
    orc.forward(tr)
    dev, stats = helpers.hip_frame(model, oracle_lut, msaa=msaa, mipmap=mipmap, transparent=True)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["clip_mismatch"] == 0 and r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0, r        # the opaque image underneath
    c = helpers.compare_composite(orc, dev)
    dev.close()
    assert c["clip_mismatch"] == 0 and c["nt_mismatch"] == 0 and c["wpos_mismatch"] == 0, c
    assert c["touched_pixels"] > 10000 and c["untouched_changed"] == 0, c
    assert c["alpha_mismatch"] <= c["touched_pixels"] // 1000, c
    helpers.assert_composite("transparent scene msaa=%d mipmap=%d" % (msaa, int(mipmap)), c)
    assert stats["forward_triangles"] == sum(d["tri_count"] * max(1, d.get("inst_count", 0)) for d in tr)


@pytest.mark.gpu
def test_transparent_pass_through_the_host_layer(oracle_lut):
    """The product path: SceneDesc -> C++ host layer (alpha modes, transparency geometry, both draw lists) -> C-ABI -> HIP, with the
    reference's default anti-aliasing (MSAA x4 + gradient mips)."""
    sc = scenes.transparent_scene(400, 240, tex_size=32)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut, msaa=4, mipmap=True)
    orc.forward(model.collect_transparent_draws())
    r, dev, stats = helpers.host_frame(sc, oracle_lut, msaa=4, mipmap=True)
    c = helpers.compare_composite(orc, dev)
    r.close()
    assert c["clip_mismatch"] == 0 and c["nt_mismatch"] == 0 and c["wpos_mismatch"] == 0 and c["untouched_changed"] == 0, c
    helpers.assert_composite("transparent scene through the host layer, MSAA x4 + mips", c)
    assert stats["forward_triangles"] > 0 and stats["ms_forward"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode,n,msaa", [("bands", 2, 0), ("bands", 3, 0), ("rows", 2, 0), ("rows", 3, 4)])
def test_transparent_pass_on_sharded_contexts(mode, n, msaa, oracle_lut):
    """N contexts, each shading its rows (bands or strips): opaque pass per shard, the ranks' opaque rows gathered into one full image
    (here: row copies between torch tensors on the one GPU; with real ranks an all-gather), awsm_hip_bind_opaque_source, transparent
    pass per shard, composite rows gathered — must equal the unsharded composite bit for bit (screen-space transmission samples the
    opaque image anywhere on the screen, the blend is per pixel)."""
    import torch
    from awsm_renderer_amd import sharding
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.transparent_scene(480, 270, tex_size=64)
    W, H = sc.width, sc.height
    model = helpers.build_model(sc)
    model.collect_draws()
    tr = model.collect_transparent_draws()
    ref, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa, transparent=True)
    want = ref.read_composite()
    want_opaque = ref.read_opaque()
    ref.close()
    assert (want != want_opaque).any()
    per = (H + n - 1) // n
    rows_of = [np.array(sharding.band_rows(H, n, r)) if mode == "bands" else np.arange(min(r * per, H), min(r * per + per, H)) for r in range(n)]
    devs, opaque, comp = [], [], []
    gathered = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r in range(n):
        dev = HipDevice(parity_tap=False)
        opaque.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        comp.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        dev.resize(W, H, msaa)
        dev.upload_mirrors(model.mirrors())
        for i, t in enumerate(model.texture_arrays()):
            dev.texture_array_upload(i, t["texels"])
        for i, smp in enumerate(sc.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib_rgba16f(oracle_lut))
        if mode == "bands":
            dev.set_shard_bands(n, r)
        else:
            dev.set_shard_rows(int(rows_of[r][0]), int(rows_of[r][-1]) + 1)
        dev.bind_output(opaque[r].data_ptr(), H * W * 8)
        dev.bind_composite(comp[r].data_ptr(), H * W * 8)
        dev.geometry_pass(model.collect_draws()); dev.opaque_pass(); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        gathered[idx] = opaque[r][idx]                         # the "all-gather" of the opaque rows
        devs.append(dev)
    torch.cuda.synchronize()
    assert (gathered.cpu().numpy().view(np.uint16) == want_opaque).all()
    final = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r, dev in enumerate(devs):
        dev.bind_opaque_source(gathered.data_ptr(), H * W * 8)
        dev.transparent_pass(tr); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        final[idx] = comp[r][idx]
        dev.close()
    torch.cuda.synchronize()
    got = final.cpu().numpy().view(np.uint16)
    assert (got == want).all(), int((got != want).any(axis=2).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("mode,n,msaa", [("bands", 2, 0), ("rows", 3, 0), ("rows", 2, 4)])
def test_hud_passes_on_sharded_contexts(mode, n, msaa, oracle_lut):
    """The five passes of a frame with hud meshes on N contexts that each own part of the rows (bands; row strips, also with MSAA x4, where a strip
    rasterises its own halo rows — of the hud meshes too): the gathered composite must equal the unsharded one bit for bit."""
    import torch
    from awsm_renderer_amd import sharding
    from awsm_renderer_amd.hip_backend import HipDevice
    sc = scenes.hud_scene(480, 270)
    W, H = sc.width, sc.height
    model = helpers.build_model(sc)
    world, tr = model.collect_draws(), model.collect_transparent_draws()
    ref, _ = helpers.hip_frame(model, oracle_lut, msaa=msaa, hud=True)
    want, want_opaque = ref.read_composite(), ref.read_opaque()
    ref.close()
    assert (want != want_opaque).any()
    per = (H + n - 1) // n
    rows_of = [np.array(sharding.band_rows(H, n, r)) if mode == "bands" else np.arange(min(r * per, H), min(r * per + per, H)) for r in range(n)]
    devs, opaque, comp = [], [], []
    gathered = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r in range(n):
        dev = HipDevice(parity_tap=False)
        opaque.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        comp.append(torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
        dev.resize(W, H, msaa)
        dev.upload_mirrors(model.mirrors())
        for i, t in enumerate(model.texture_arrays()):
            dev.texture_array_upload(i, t["texels"])
        for i, smp in enumerate(sc.samplers):
            dev.sampler_set(i, smp)
        dev.env_upload(sc.skybox_rgba, sc.prefiltered_rgb, sc.irradiance_rgb, oracle_lib_rgba16f(oracle_lut))
        if mode == "bands":
            dev.set_shard_bands(n, r)
        else:
            dev.set_shard_rows(int(rows_of[r][0]), int(rows_of[r][-1]) + 1)
        dev.bind_output(opaque[r].data_ptr(), H * W * 8)
        dev.bind_composite(comp[r].data_ptr(), H * W * 8)
        dev.geometry_pass(world); dev.hud_geometry_pass(model.hud_geometry_draws); dev.opaque_pass(); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        gathered[idx] = opaque[r][idx]
        devs.append(dev)
    torch.cuda.synchronize()
    assert (gathered.cpu().numpy().view(np.uint16) == want_opaque).all()
    final = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    for r, dev in enumerate(devs):
        dev.bind_opaque_source(gathered.data_ptr(), H * W * 8)
        dev.transparent_pass(tr); dev.hud_transparent_pass(model.hud_transparent_draws); dev.frame_end()
        idx = torch.as_tensor(rows_of[r], device="cuda")
        final[idx] = comp[r][idx]
        dev.close()
    torch.cuda.synchronize()
    got = final.cpu().numpy().view(np.uint16)
    assert (got == want).all(), int((got != want).any(axis=2).sum())


@pytest.mark.gpu
def test_transparent_pass_edge_cases(oracle_lut):
    """An empty transparent list copies the opaque image; a sharded context refuses; the pass needs the opaque pass first."""
    from awsm_renderer_amd.hip_backend import AwsmHipError
    sc = scenes.transparent_scene(200, 120, tex_size=16)
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut)
    dev.transparent_pass([])
    dev.frame_end()
    assert (dev.read_composite() == dev.read_opaque()).all()
    dev.geometry_pass(model.collect_draws())
    with pytest.raises(AwsmHipError):
        dev.transparent_pass(model.collect_transparent_draws())          # no opaque pass yet this frame
    dev.set_shard_rows(0, 60)
    dev.geometry_pass(model.collect_draws())
    dev.opaque_pass()
    with pytest.raises(AwsmHipError):
        dev.transparent_pass(model.collect_transparent_draws())
    dev.close()


# ------------------------------------------------------------------------------------------------ glTF ingest

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["helmet", "skinned_morph", "transparent", "morph_then_skin"])
def test_frames_rendered_from_a_glb_file(name, oracle_lut, tmp_path):
    """File -> native glTF reader -> host layer -> HIP kernels, against the oracle's frame of the scene the file was written from."""
    from awsm_renderer_amd import gltf_export
    from tests import vertex_stage_cases
    sc = {"helmet": lambda: scenes.helmet_scene(320, 180, segments=48, rings=36, tex_size=64),
          "skinned_morph": lambda: scenes.skinned_morph_scene(320, 200, around=16, along=24, tex_size=16),
          "transparent": lambda: scenes.transparent_scene(320, 180, tex_size=32),
          "morph_then_skin": vertex_stage_cases.morph_then_skin}[name]()      # JOINTS_0..2, morph TANGENT deltas
    path = str(tmp_path / (name + ".glb"))
    gltf_export.write_glb(sc, path)
    model = helpers.build_model(sc)
    orc = helpers.oracle_frame(model, oracle_lut)
    r, dev, stats = helpers.host_frame(sc, oracle_lut, gltf=path)
    res = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert res["clip_mismatch"] == 0 and res["nt_mismatch"] == 0 and res["key_mismatch"] == 0 and res["rgb_over_tol"] == 0 and res["covered"] > 0, res
    if name == "transparent":
        orc.forward(model.collect_transparent_draws())
        c = helpers.compare_composite(orc, dev)
        assert c["clip_mismatch"] == 0 and c["untouched_changed"] == 0, c
        helpers.assert_composite("transparent scene from a .glb file", c)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mipmap", [False, True])
def test_hud_passes_with_msaa(oracle_lut, mipmap):
    """The reference's default anti-aliasing with hud meshes (VERDICT r3 "next" #4), quirk included: after the HUD geometry pass a covered sample shows
    the hud triangle and still the world's depth; a pixel whose sample 0 is a hud triangle stays cleared, the edge detector sees hud normals beside world
    depths, and msaa_resolve_samples shades hud samples like any other (compute.wgsl:176-180: "this may bleed a little").  The oracle composes exactly
    that from its ordinary MSAA code (oracle_lib.frame_with_hud_msaa); here: world keys bit-exact, every opaque pixel within the shading tolerance (the
    bleeding ones included), cleared pixels exactly zero, the composite after both transparent passes within two f16 steps, the picker on hud pixels."""
    from oracle.host_mirror import key_as_ffi
    sc = scenes.hud_scene(480, 270)
    model = helpers.build_model(sc)
    orc = oracle_lib.frame_with_hud_msaa(model, oracle_lut, threads=16, msaa=4, mipmap=mipmap)
    hud0 = orc.merged_keys[..., 0] != orc.keys[..., 0]                       # sample 0 is a hud triangle
    bleed = (orc.merged_keys != orc.keys).any(axis=-1) & ~hud0               # some other sample is: the pixel is shaded, and may be resolved over a hud sample
    assert int(hud0.sum()) > 2000 and int(bleed.sum()) > 50
    dev, _ = helpers.hip_frame(model, oracle_lut, hud=True, msaa=4, mipmap=mipmap)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["clip_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["f16_max_ulp"] <= 2, r
    opaque = dev.read_opaque()
    assert (opaque[hud0] == 0).all()
    assert (orc.rgba16f[bleed] != orc._world.shade(16).rgba16f[bleed]).any(axis=-1).sum() > 10      # the quirk is there to be matched: hud samples do change those pixels
    orc.forward(model.collect_transparent_draws(), 16)
    orc.forward(model.hud_transparent_draws, 16, hud=True)
    ulp = helpers.f16_ulp_distance(dev.read_composite(), orc.composite16f)
    assert int((ulp > 2).any(axis=-1).sum()) <= 4, int((ulp > 2).any(axis=-1).sum())
    first = np.concatenate([[0], np.cumsum([d["tri_count"] for d in model.hud_geometry_draws])])
    ys, xs = np.nonzero(hud0)
    for i in range(0, len(ys), max(1, len(ys) // 16)):
        y, x = int(ys[i]), int(xs[i])
        rank = 0xFFFFFFFF - int(orc.hud_keys[y, x, 0] & np.uint64(0xFFFFFFFF))
        di = int(np.searchsorted(first, rank, side="right") - 1)
        got = dev.pick(x, y)
        assert got is not None and got[0] == key_as_ffi(model.hud_geometry_draws[di]["mesh_key"]) and got[1] == rank - int(first[di]), (x, y, got)
    dev.close()
    rr, hdev, _ = helpers.host_frame(sc, oracle_lut, msaa=4, mipmap=mipmap)      # the C++ host layer: the reference's default AntiAliasing with a hud mesh renders
    ulp = helpers.f16_ulp_distance(hdev.read_composite(), orc.composite16f)
    assert int((ulp > 2).any(axis=-1).sum()) <= 4
    rr.close()


@pytest.mark.gpu
def test_hud_passes(oracle_lut):
    """The two HUD passes (render.rs:169-178,301-312): hud meshes rasterised over the visibility targets with a depth buffer of their own, the opaque
    pass leaving the pixels they cover cleared (compute.wgsl:176-179), the world transparent pass still depth-tested against the WORLD's depth, then the
    hud meshes forward-shaded over the composite against hud_depth, cleared.  Against the oracle: world keys bit-exact, the opaque image within the
    shading tolerance with exact zeros under the hud meshes, the composite within two f16 steps; the picker reports the hud mesh; a hud quad that
    lies behind the world's back wall still shows."""
    from oracle.host_mirror import key_as_ffi
    sc = scenes.hud_scene(480, 270)
    model = helpers.build_model(sc)
    orc = oracle_lib.frame_from_model(model, oracle_lut).transform().raster(16)
    hud_keys = orc.hud_geometry(model, 16)
    covered = hud_keys != helpers.NO_HIT
    assert 2000 < int(covered.sum()) < sc.width * sc.height // 2
    orc.shade(16).apply_hud_clear()
    dev, _ = helpers.hip_frame(model, oracle_lut, hud=True)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["key_mismatch"] == 0 and r["clip_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["f16_max_ulp"] <= 2, r
    opaque = dev.read_opaque()
    assert (opaque[covered] == 0).all()                                     # cleared, alpha included
    assert (opaque[~covered][:, 3] == 0x3C00).all()                          # everything else was shaded (or sky): alpha 1
    # the composite: world transparent pass, then the hud meshes over it
    orc.forward(model.collect_transparent_draws(), 16)
    world_comp = orc.composite16f.copy()
    orc.forward(model.hud_transparent_draws, 16, hud=True)
    h16 = dev.read_composite()
    ulp = helpers.f16_ulp_distance(h16, orc.composite16f)
    assert int((ulp > 2).any(axis=-1).sum()) <= 4, int((ulp > 2).any(axis=-1).sum())
    touched = orc.fwd_touched != 0
    assert int(helpers.f16_ulp_distance(h16, world_comp)[~touched].max()) <= 2       # pixels no hud fragment reached keep the world's composite
    assert int(touched.sum()) >= int(covered.sum())                          # every hud-covered pixel received a hud fragment (hud_depth starts cleared)
    # the quad behind the wall: the world is in front of it everywhere, and it still shows (its pixels changed the composite)
    wall_in_front = covered & (orc.keys != helpers.NO_HIT) & ((orc.keys >> np.uint64(32)) < (hud_keys >> np.uint64(32)))
    assert int(wall_in_front.sum()) > 500 and (h16[wall_in_front] != world_comp[wall_in_front]).any(axis=-1).mean() > 0.9
    # picker: a hud-covered pixel reports the hud mesh whose triangle the hud keys hold
    first = np.concatenate([[0], np.cumsum([d["tri_count"] for d in model.hud_geometry_draws])])
    ys, xs = np.nonzero(covered)
    for i in range(0, len(ys), max(1, len(ys) // 24)):
        y, x = int(ys[i]), int(xs[i])
        rank = 0xFFFFFFFF - int(hud_keys[y, x] & np.uint64(0xFFFFFFFF))
        di = int(np.searchsorted(first, rank, side="right") - 1)
        got = dev.pick(x, y)
        assert got is not None and got[0] == key_as_ffi(model.hud_geometry_draws[di]["mesh_key"]) and got[1] == rank - int(first[di]), (x, y, got)
    dev.close()
    # through the C++ host layer: awsm_host_mesh_insert_hud + render() issue the same five passes
    rr, hdev, _ = helpers.host_frame(sc, oracle_lut)
    ulp = helpers.f16_ulp_distance(hdev.read_composite(), orc.composite16f)
    assert int((ulp > 2).any(axis=-1).sum()) <= 4
    assert (hdev.read_opaque()[covered] == 0).all()
    rr.close()
    # pipelined frames (AWSM_CFG_OVERLAP_FRAMES): the HUD transparent pass of a frame is enqueued — its draw list uploaded on the caller's stream — while the
    # world transparent pass of the same frame may not have started on the shade stream.  The two have their own lists and counters (they used to
    # share them, and the world pass could shade with the HUD pass's draw records); several frames in flight, then the last one against the oracle.
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    assert len(model.collect_transparent_draws()) > 0 and model.collect_transparent_draws() != model.hud_transparent_draws
    ro = Renderer(sc, parity_tap=True, lut_rgba16f=oracle_lib.lut_rg_to_rgba16f(oracle_lut), overlap_frames=True)
    for _ in range(6):
        ro.host.render(sync=False)
    ro.host.render(sync=True)
    odev = HipDevice.from_ctx(ro.host.device_ctx, sc.width, sc.height)
    ulp = helpers.f16_ulp_distance(odev.read_composite(), orc.composite16f)
    assert int((ulp > 2).any(axis=-1).sum()) <= 4, int((ulp > 2).any(axis=-1).sum())
    assert (odev.read_opaque()[covered] == 0).all()
    ro.close()



@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["atrium", "zoo"])
def test_camera_written_between_the_passes_does_not_split_the_frame(oracle_lut, scene_name):
    """A frame is shaded with the camera it was submitted with: the lean kernel's pixel -> view matrix is composed at awsm_hip_geometry_pass,
    the general kernels read the camera buffer — a snapshot the geometry pass takes, in every mode.  A camera write between the two passes of a frame
    must therefore change nothing of that frame: neither the lean strips nor the general ones (the zoo's optional-block materials take the general code)."""
    from awsm_renderer_amd.hip_backend import HipDevice
    from oracle import scene_model as sm
    sc = scenes.atrium_scene(640, 360, detail=0.125, tex_scale=1 / 32) if scene_name == "atrium" else scenes.material_zoo_scene(480, 270)
    model = helpers.build_model(sc)
    dev, _ = helpers.hip_frame(model, oracle_lut)
    want = dev.read_opaque().copy()
    other = bytearray(model.mirrors()[sm.BUF_CAMERA])
    other[384:396] = np.asarray([100.0, -50.0, 25.0], dtype=np.float32).tobytes()      # CameraUniform.position (camera.rs:72-87): somewhere else entirely
    other[256:320] = np.eye(4, dtype=np.float32).tobytes()                              # inv_proj
    dev.geometry_pass(model.collect_draws())
    dev.buffer_write(sm.BUF_CAMERA, 0, np.frombuffer(bytes(other), dtype=np.uint8))
    dev.opaque_pass()
    dev.frame_end()
    assert (dev.read_opaque() == want).all()
    dev.close()


# ------------------------------------------------------------------------------------------------ geometry cache (round 5)

def _write_mirror_changes(dev, before, after):
    """awsm_hip_buffer_write for exactly the 4-byte words in which two mirror sets differ (what write_buffer_with_dirty_ranges sends: the ranges a host
    marked dirty), merged into runs.  Returns the number of writes per buffer."""
    n = {}
    for which, new in after.items():
        old = before[which]
        assert len(old) == len(new), which
        a, b = np.frombuffer(bytes(old), dtype=np.uint32), np.frombuffer(bytes(new), dtype=np.uint32)
        idx = np.nonzero(a != b)[0]
        if idx.size == 0:
            continue
        starts = np.concatenate([[0], np.nonzero(np.diff(idx) > 1)[0] + 1])
        ends = np.concatenate([starts[1:], [idx.size]])
        for s, e in zip(starts, ends):
            lo, hi = int(idx[s]) * 4, (int(idx[e - 1]) + 1) * 4
            dev.buffer_write(which, lo, np.frombuffer(bytes(new[lo:hi]), dtype=np.uint8))
            n[which] = n.get(which, 0) + 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("cache", ["on", "off"])
def test_geometry_cache_recomputes_what_was_written_and_nothing_else(cache, oracle_lut, monkeypatch):
    """k_deform_transform keeps a draw's world positions / normals / tangents / per-triangle words in the frame slot from one frame of the slot to the next
    and only forms clip = view_proj * world, unless the draw moved in the list or something it reads was written (frame_params.hpp: geometry cache;
    transforms.rs:390-435 is the dirty propagation that produces those writes, apply_vertex.wgsl:24-118 what is recomputed).  Overlapped frames, so both
    frame slots: a camera move, then a node transform, a joint and a morph weight written between frames — through awsm_hip_buffer_write with exactly the
    changed words, as the dirty-range writer does.  After every frame: transformed vertices (clip, N, T) and keys bit-exact against the oracle's frame of the
    scene as it then is; AwsmFrameStats.geometry_cache_blocks says how many workgroups kept their draw's cached outputs — all of them after a camera move,
    all but the written draw's after a write, in BOTH slots (each slot sees the writes since ITS last frame).  AWSM_GEOMETRY_CACHE=0: same frames, no hits."""
    import copy
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.scene_desc import NodeDesc
    from awsm_renderer_amd.scenes import look_at_rh, quat_axis_angle
    from oracle import scene_model as sm
    if cache == "off":
        monkeypatch.setenv("AWSM_GEOMETRY_CACHE", "0")
    base = scenes.skinned_morph_scene(480, 270, around=16, along=40, tex_size=16)
    box = copy.deepcopy(scenes.box_scene().nodes[1].primitives[0])
    box.material = 1
    base.nodes.append(NodeDesc(translation=(-1.5, 0.3, 0.2), scale=(0.5, 0.5, 0.5), primitives=[box]))      # a mesh none of the writes below concerns
    cube_node, joint_node, static_node = len(base.nodes) - 2, 6, len(base.nodes) - 1
    assert base.nodes[cube_node].primitives[0].morph_targets and base.nodes[static_node].primitives

    def variant(camera=False, moved=False, joint=False, morph=False):
        sc = copy.deepcopy(base)
        if camera:
            eye = (1.1, 0.7, 4.9)
            sc.view, sc.camera_position = look_at_rh(eye, (0.4, 0.1, 0.0)), eye
        if moved:
            sc.nodes[cube_node].translation = (1.45, 0.25, 0.1)
        if joint:
            sc.nodes[joint_node].rotation = quat_axis_angle((0, 0, 1), 0.31)
        if morph:
            sc.nodes[cube_node].primitives[0].animated_morph_weights = np.array([0.55, 0.2], dtype=np.float32)
        return sc

    steps = [("first", dict(), ()), ("camera", dict(camera=True), ()), ("transform", dict(camera=True, moved=True), ("cube",)),
             ("joint", dict(camera=True, moved=True, joint=True), ("tube",)), ("morph weight", dict(camera=True, moved=True, joint=True, morph=True), ("cube",)),
             ("nothing", dict(camera=True, moved=True, joint=True, morph=True), ())]
    dev = HipDevice(parity_tap=True, overlap_frames=True)
    model = helpers.build_model(variant())
    threads = _host_threads()
    # the test's own model of the cache: per frame slot the list its arrays were computed for and the meshes written since
    slot, slot_list, dirty_since = [0], {}, {0: set(), 1: set()}

    def placed(draws):
        out, first = [], 0
        for i, d in enumerate(draws):
            out.append((i, first, tuple(sorted((k, v) for k, v in d.items() if k != "mesh_key"))))
            first += d["tri_count"]
        return out

    def frame(draws, mesh_of, orc, tag):
        slot[0] = (slot[0] + 1) % 2                                        # awsm_hip_geometry_pass takes the next slot
        prev = slot_list.get(slot[0])
        want = 0
        for p in placed(draws):
            if cache == "on" and prev is not None and p in prev and mesh_of[dict(p[2])["geom_meta_off"]] not in dirty_since[slot[0]]:
                want += (3 * dict(p[2])["tri_count"] + 255) // 256
        dev.geometry_pass(draws); dev.opaque_pass(); st = dev.frame_end()
        slot_list[slot[0]], dirty_since[slot[0]] = set(placed(draws)), set()
        total = sum((3 * d["tri_count"] + 255) // 256 for d in draws)
        assert st["geometry_blocks"] == total and st["geometry_cache_blocks"] == want, (tag, st, total, want)
        if orc is not None:
            clip, nt = dev.read_transformed(orc.n_verts)
            assert (clip.view(np.uint32) == orc.clip.view(np.uint32)).all(), tag
            assert (nt.view(np.uint32) == orc.nt.view(np.uint32)).all(), tag
            assert (dev.read_visibility() == orc.keys).all(), tag
        return want, total

    helpers.hip_frame(model, oracle_lut, dev=dev)                      # creates and fills every buffer; the context's first frame
    slot[0] = 1
    slot_list[1] = set(placed(model.collect_draws()))
    mirrors = model.mirrors()
    seen_writes, hits = {}, {}
    for name, kw, written in steps:
        model = helpers.build_model(variant(**kw))
        new = model.mirrors()
        for which, cnt in _write_mirror_changes(dev, mirrors, new).items():
            seen_writes.setdefault(name, {})[which] = cnt
        mirrors = new
        for sl in dirty_since:
            dirty_since[sl] |= set(written)
        draws = model.collect_draws()
        offs = sorted({d["geom_meta_off"] for d in draws})
        assert len(offs) == 3
        mesh_of = dict(zip(offs, ("tube", "cube", "box")))                 # mesh insertion order = meta slot order
        orc = oracle_lib.frame_from_model(model, oracle_lut).transform().raster(threads)
        hits[name] = [frame(draws, mesh_of, orc, (name, rep)) for rep in range(2)]     # two frames: one per frame slot
    if cache == "on":
        assert sm.BUF_TRANSFORMS in seen_writes["transform"] and sm.BUF_SKIN_MATRICES in seen_writes["joint"] and sm.BUF_MORPH_WEIGHTS in seen_writes["morph weight"], seen_writes
        assert hits["camera"][0][0] == hits["camera"][0][1] > 4 and hits["nothing"][1][0] == hits["nothing"][1][1]      # a camera move recomputes nothing
        for name in ("transform", "joint", "morph weight"):                                                              # a write: its mesh, in both slots, nothing else
            assert 0 < hits[name][0][0] < hits[name][0][1] and hits[name][0] == hits[name][1], (name, hits)
        assert hits["joint"][0][0] <= 2                                                                                 # the tube is nearly all of the geometry
    else:
        assert all(h[0] == 0 for v in hits.values() for h in v)
    # the last frame in full: shading reads the cached normals / tangents / per-triangle words
    orc = helpers.oracle_frame(model, oracle_lut, threads=threads)
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0 and r["key_mismatch"] == 0 and r["rgb_over_tol"] == 0 and r["f16_max_ulp"] <= 2, r
    # a draw list that changes (a draw dropped, so every draw behind it moves in rank space; the order reversed) and comes back: draws that moved are
    # recomputed, draws that did not keep their outputs, the image is right
    for k, lst in enumerate((draws[1:], draws, list(reversed(draws)), draws[:2], draws)):
        frame(lst, mesh_of, None, ("list", k))
    frame(draws, mesh_of, None, ("list", "back"))
    assert (dev.read_visibility() == orc.keys).all()
    r = helpers.compare_frames(orc, dev, rgb_tol=RGB_TOL)
    assert r["clip_mismatch"] == 0 and r["nt_mismatch"] == 0 and r["rgb_over_tol"] == 0, r
    dev.close()


@pytest.mark.gpu
def test_geometry_cache_in_enqueue_only_frames_with_a_moving_camera(oracle_lut):
    """The bench's situation: frames enqueued without a synchronisation, the camera moving every frame, the sorted draw list changing now and then.  Every
    frame's image must equal the same frame rendered by a context with the cache off."""
    import ctypes as C
    from awsm_renderer_amd.hip_backend import HipDevice
    from awsm_renderer_amd.host import Renderer
    from awsm_renderer_amd.scenes import look_at_rh
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sc = scenes.atrium_scene(480, 270, detail=0.25, tex_scale=1 / 16)
    n = 40
    eyes = [(0.4 + 2.5 * math.sin(0.35 * i), 3.1 + 0.05 * i, 17.0 - 0.8 * i) for i in range(n)]
    lut = oracle_lib_rgba16f(oracle_lut)
    nbytes = sc.height * sc.width * 8

    def run(cache_on):
        if not cache_on:
            os.environ["AWSM_GEOMETRY_CACHE"] = "0"
        try:
            r = Renderer(sc, lut_rgba16f=lut, overlap_frames=True)
        finally:
            os.environ.pop("AWSM_GEOMETRY_CACHE", None)
        r.host.set_render_timings(False)
        dev = HipDevice.from_ctx(r.host.device_ctx, sc.width, sc.height)
        outs, lists = [], []
        for _ in eyes:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            outs.append(p)
        for i, eye in enumerate(eyes):
            r.host.camera_update(look_at_rh(eye, (-0.2, 3.4, -18.0)), sc.proj, eye)
            dev.bind_output(outs[i].value, nbytes)
            r.host.render(sync=False)
            lists.append(tuple(tuple(sorted(d.items())) for d in r.host.draw_list()))
        dev.frame_flush()
        assert hip.hipDeviceSynchronize() == 0
        imgs = []
        for p in outs:
            a = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0
            imgs.append(a)
            hip.hipFree(p)
        dev.bind_output(None)
        r.close()
        return imgs, lists

    on, lists = run(True)
    off, _ = run(False)
    assert len(set(lists)) > 3, "the camera path must change the sorted draw list several times"
    for i, (a, b) in enumerate(zip(on, off)):
        assert (a == b).all(), f"frame {i}: {(a != b).sum()} values differ between cache on and off"


@pytest.mark.gpu
def test_overlapped_msaa_frames_with_hud_meshes_and_a_changing_world_list(oracle_lut):
    """AWSM_CFG_OVERLAP_FRAMES + MSAA x4 + a HUD geometry pass.  The hud draws are uploaded behind the world's list AFTER the world geometry pass
    recorded its uploads event; a per-draw resolve that started on that event read hud entries that were not there yet (garbage meta offsets on a slot's
    first frame, the list of two frames ago afterwards — wrong materials and is_hud flags whenever the world draw count changes).  Ten frames without a
    synchronisation, stage timers off (the early resolve's precondition), the world list losing and regaining draws from frame to frame: every image equals
    the same frame from a plain (non-overlapping) context."""
    import ctypes as C
    from awsm_renderer_amd.hip_backend import HipDevice
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    sc = scenes.hud_scene(480, 270)
    model = helpers.build_model(sc)
    world, hud = model.collect_draws(), model.hud_geometry_draws
    assert len(world) >= 3 and len(hud) >= 1
    lists = [world, world[:-1], world[:-2], world, world[1:], world, world[:-1], world[:-1], world, world]
    nbytes = sc.height * sc.width * 8

    def run(overlap):
        dev = HipDevice(parity_tap=False, overlap_frames=overlap)
        helpers.hip_frame(model, oracle_lut, dev=dev, msaa=4, mipmap=True, hud=True)
        dev.set_stage_timers(False)
        outs = []
        for _ in lists:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            outs.append(p)
        for i, lst in enumerate(lists):
            dev.bind_output(outs[i].value, nbytes)
            dev.geometry_pass(lst); dev.hud_geometry_pass(hud); dev.opaque_pass(mipmap=1)
            if not overlap:
                dev.frame_end()
        dev.frame_flush()
        assert hip.hipDeviceSynchronize() == 0
        imgs = []
        for p in outs:
            a = np.zeros((sc.height, sc.width, 4), dtype=np.uint16)
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0
            imgs.append(a)
            hip.hipFree(p)
        dev.bind_output(None)
        dev.close()
        return imgs

    plain, over = run(False), run(True)
    for i, (a, b) in enumerate(zip(plain, over)):
        assert (a == b).all(), f"frame {i}: {(a != b).sum()} values differ"
    assert not (plain[0] == plain[2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mips", "msaa"])
def test_full_size_4k_other_modes(mode, oracle_lut):
    """The 4K frame in the two modes between the BASELINE's and the reference's default — MipmapMode::Gradient alone (k_shade_lean<., 1, false>: the
    shared-footprint route at full size) and MSAA x4 alone — every pixel against the oracle, as test_full_size_4k_frame_properties does for the others."""
    kw = dict(mipmap=True) if mode == "mips" else dict(msaa=4)
    sc = scenes.atrium_scene(3840, 2160)
    model = helpers.build_model(sc)
    dev, stats = helpers.hip_frame(model, oracle_lut, **kw)
    orc = helpers.oracle_frame(model, oracle_lut, threads=_host_threads(), **kw)
    _assert_full_frame("configs[3] atrium 3840x2160 " + ("gradient mips" if mode == "mips" else "MSAA x4"), orc, dev, stats)
    assert stats["shade_general_wavefronts"] == 0
    dev.close()


@pytest.mark.gpu
def test_frame_stats_struct_size_is_honoured(oracle_lut):
    """ABI 2: AwsmFrameStats grows by appending (round 5: geometry_cache_blocks, geometry_blocks) and awsm_hip_frame_end writes nothing beyond the size the
    caller states — a caller compiled against the struct of an earlier round keeps working, its memory behind the struct untouched."""
    import ctypes as C
    from awsm_renderer_amd.hip_backend import AwsmFrameStats
    model = helpers.build_model(scenes.box_scene(96, 64))
    dev, full = helpers.hip_frame(model, oracle_lut)
    old_size = AwsmFrameStats.geometry_cache_blocks.offset      # the struct as round 4 knew it
    buf = (C.c_uint8 * (C.sizeof(AwsmFrameStats) + 64))()
    C.memset(buf, 0xA5, len(buf))
    st = AwsmFrameStats.from_buffer(buf)
    st.struct_size = old_size
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass()
    dev._chk(dev.lib.awsm_hip_frame_end(dev.ctx, C.byref(st)), "frame_end")
    assert st.struct_size == old_size and st.triangles_in == full["triangles_in"] and st.covered_pixels == full["covered_pixels"]
    assert bytes(buf[old_size:]) == b"\xA5" * (len(buf) - old_size)
    st.struct_size = C.sizeof(AwsmFrameStats)
    dev.geometry_pass(model.collect_draws()); dev.opaque_pass()
    dev._chk(dev.lib.awsm_hip_frame_end(dev.ctx, C.byref(st)), "frame_end")
    assert st.struct_size == C.sizeof(AwsmFrameStats) and st.geometry_blocks >= 1 and st.geometry_cache_blocks == st.geometry_blocks      # nothing moved: every workgroup kept its draw
    assert bytes(buf[C.sizeof(AwsmFrameStats):]) == b"\xA5" * 64
    dev.close()
