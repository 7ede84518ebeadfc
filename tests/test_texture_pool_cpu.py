"""The texture pool's contract without a GPU: the sRGB table and the integer premultiply, the validation and the gather of
awsm_hip_texture_array_write_layers as a sanitised program over the library's own header, and the host layer over two mock backends — the
existing one, which lacks the awsm_hip_texture_array_* pool symbols, and one that records them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from awsm_renderer_amd import host as H
from awsm_renderer_amd import scenes
from tests import texture_pool_reference as ref
from tests.test_host_layer_cpu import MOCK, MOCK_DIR, log_of, mock  # noqa: F401  (the module-scoped fixture builds the mock backend)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -6
LUT = np.zeros((4, 4, 4), dtype=np.uint16)
OPS = {20: "create", 21: "resize_layers", 22: "write_layers", 23: "generate_mips_layers"}


# ------------------------------------------------------------------------------------------------ the arithmetic

def test_srgb_table_does_not_depend_on_who_evaluates_it():
    t64, t32 = ref.srgb_table(), ref.srgb_table_f32()
    assert (t64 == t32).all()
    d, q = ref.tie_distance()
    assert d >= 1e-3, (d, q)
    assert t64[0] == 0 and t64[255] == 255 and (np.diff(t64.astype(np.int32)) >= 0).all()
    assert list(t64[[1, 10, 11, 36, 128, 188]]) == [0, 1, 1, 4, 55, 128]      # by hand; 10 / 255 = 0.0392 <= 0.04045 is still the linear branch


def test_integer_premultiply_is_the_float_form_for_every_pair():
    c, a = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    integer = (2 * c * a + 255) // 510
    assert (integer == np.floor(c * a / 255.0 + 0.5).astype(np.int64)).all()
    f = np.float32
    as_f32 = np.floor((c.astype(f) / f(255.0)) * (a.astype(f) / f(255.0)) * f(255.0) + f(0.5)).astype(np.int64)      # (c/255)(a/255) stored as unorm8
    assert (integer == as_f32).all()
    texels = np.stack([c, c[::-1], (c * 7) % 256, a], axis=-1).astype(np.uint8)
    got = ref.premultiply(texels)
    assert (got[..., 0] == integer).all() and (got[..., 3] == a).all()


def test_numpy_mip_chain_is_the_oracles():
    from oracle import oracle_lib
    rng = np.random.default_rng(3)
    kinds = [0, 1, 2, 3, 5]
    for w, h in [(1, 1), (2, 2), (3, 5), (64, 4), (33, 33)]:
        level0 = rng.integers(0, 256, size=(5, h, w, 4), dtype=np.uint8)
        if w >= 2 and h >= 2:
            level0[1, :2, :2, :3] = np.array([[0, 255], [0, 255]], dtype=np.uint8)[..., None]      # mean normal = zero vector -> NaN -> 0
        chain, levels = oracle_lib.mip_chain(level0, kinds)
        mine = ref.mip_chain(level0, kinds)
        assert len(mine) == levels
        for l in range(levels):
            assert (oracle_lib.mip_level_view(chain, w, h, 5, l) == mine[l]).all(), (w, h, l)


# ------------------------------------------------------------------------------------------------ validation + gather, sanitised

def test_write_validation_and_gather_under_asan_and_ubsan_as_a_program(tmp_path):
    """Every rule with a buffer one byte short is an error and no read; the gather of accepted layouts, the table and the premultiply of the
    library's header equal the numpy restatement."""
    exe = tmp_path / "texture_pool_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "awsm-renderer_amd", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "texture_pool_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "TEXTURE_POOL_CHECK_OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    lines = [l.split() for l in p.stdout.splitlines()]
    table = [l for l in lines if l[0] == "TABLE"][0]
    assert (np.array(table[1:], dtype=np.int64) == ref.srgb_table()).all()
    W, Hh, n = 5, 3, 2
    gathers = [l for l in lines if l[0] == "GATHER"]
    assert len(gathers) == 8
    for g in gathers:
        bpr, rpi, flags = int(g[1]), int(g[2]), int(g[3])
        used = (n - 1) * bpr * rpi + (Hh - 1) * bpr + W * 4
        i = np.arange(used, dtype=np.uint64)
        src = (((i * 37 + 11) ^ (i >> 3)) & 0xFF).astype(np.uint8)
        img = np.zeros((n, Hh, W, 4), dtype=np.uint8)
        for l in range(n):
            for y in range(Hh):
                o = l * bpr * rpi + y * bpr
                img[l, y] = src[o: o + W * 4].reshape(W, 4)
        want = ref.convert(img, flags).reshape(-1, 4).astype(np.uint32)
        want = want[:, 0] | want[:, 1] << 8 | want[:, 2] << 16 | want[:, 3] << 24
        assert (np.array(g[4:], dtype=np.uint64) == want).all(), (bpr, rpi, flags)


# ------------------------------------------------------------------------------------------------ the host over the mock backends

@pytest.fixture(scope="module")
def pool_mock(tmp_path_factory):
    """mock_backend.c + the five pool entries, recording."""
    so = str(tmp_path_factory.mktemp("mock") / "libmock_texture_pool.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(MOCK_DIR, "mock_texture_pool.c")])
    lib = C.CDLL(so)
    lib.mock_log_count.restype = C.c_size_t
    lib.mock_log_count.argtypes = [C.c_void_p]
    lib.mock_log_get.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.mock_log_clear.argtypes = [C.c_void_p]
    lib.mock_texture_bytes.restype = C.c_uint64
    return so, lib


def texture_log(lib, ctx):
    out = []
    for i in range(lib.mock_log_count(ctx)):
        op, which, a, b = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        lib.mock_log_get(ctx, i, C.byref(op), C.byref(which), C.byref(a), C.byref(b))
        if op.value in (4, 14):
            out.append(({4: "upload", 14: "generate_mips"}[op.value], which.value))
        elif op.value in OPS:
            out.append((OPS[op.value], which.value, a.value & 0xFFFFFFFF, a.value >> 32, b.value & 0xFFFFFFFF, b.value >> 32))
    return out


def small_scene():
    return scenes.helmet_scene(64, 48, segments=8, rings=6, tex_size=16)


def noise(seed, size=16):
    return np.random.default_rng(seed).integers(0, 256, size=(size, size, 4), dtype=np.uint8)


def test_without_the_symbols_the_old_calls_are_made_and_flags_are_refused_by_name(mock):  # noqa: F811
    sc = small_scene()
    r = H.Renderer(sc, backend_path=MOCK, lut_rgba16f=LUT)
    r.render()
    ctx = r.host.device_ctx
    assert [e for e in log_of(mock, ctx) if e[0] in ("texture", "generate_mips")] == [("texture", 0, (16 << 32) | 16, 5), ("generate_mips", 0, 0, 0)]
    # one more image into the resident array: the whole array goes up again, as it always did
    mock.mock_log_clear(ctx)
    r.host.texture_insert(noise(1), 0)
    r.render()
    assert [e for e in log_of(mock, ctx) if e[0] in ("texture", "generate_mips")] == [("texture", 0, (16 << 32) | 16, 6), ("generate_mips", 0, 0, 0)]
    for call, symbol in ((lambda: r.host.texture_insert(noise(2), 0, srgb=True), "awsm_hip_texture_array_create"),
                         (lambda: r.host.texture_insert(noise(2), 0, premultiply=True), "awsm_hip_texture_array_create"),
                         (lambda: r.host.texture_update(0, noise(3)), "awsm_hip_texture_array_create")):
        with pytest.raises(H.HostError) as e:
            call()
        assert e.value.code == UNSUPPORTED and symbol in str(e.value), e.value
    assert len(r.host.pool_arrays()[0]) == 6                    # the refused inserts left nothing behind
    mock.mock_log_clear(ctx)
    r.render()
    assert not [e for e in log_of(mock, ctx) if e[0] in ("texture", "generate_mips")]
    r.close()


def test_with_the_symbols_only_the_new_images_travel(pool_mock):
    so, lib = pool_mock
    sc = small_scene()
    r = H.Renderer(sc, backend_path=so, lut_rgba16f=LUT)
    r.render()
    ctx = r.host.device_ctx
    assert texture_log(lib, ctx) == [("upload", 0), ("generate_mips", 0)]      # nothing flagged, nothing resident: today's calls
    # growth doubles: 5 -> 10 for the sixth image, nothing for the seventh ... tenth, 20 for the eleventh
    sent0 = lib.mock_texture_bytes()
    lib.mock_log_clear(ctx)
    r.host.texture_insert(noise(1), 4)
    r.render()
    assert texture_log(lib, ctx) == [("resize_layers", 0, 10, 0, 0, 0), ("write_layers", 0, 5, 1, 0, 4), ("generate_mips_layers", 0, 5, 0, 1, 0)]
    assert lib.mock_texture_bytes() - sent0 == 16 * 16 * 4
    assert r.host.upload_bytes_last_frame() >= 16 * 16 * 4
    lib.mock_log_clear(ctx)
    for i in range(4):
        r.host.texture_insert(noise(10 + i), 0, srgb=(i >= 2))
    r.render()      # one call per run of layers with the same kind and flags, one mip call for the range
    assert texture_log(lib, ctx) == [("write_layers", 0, 6, 2, 0, 0), ("write_layers", 0, 8, 2, 2, 0), ("generate_mips_layers", 0, 6, 0, 4, 0)]
    lib.mock_log_clear(ctx)
    r.host.texture_insert(noise(20), 0)
    r.host.texture_update(7, noise(21))                            # texture 7 = layer 7: not flagged
    r.host.texture_update(8, noise(22))                            # flagged: its flags travel again
    r.render()
    assert texture_log(lib, ctx) == [("resize_layers", 0, 20, 0, 0, 0), ("write_layers", 0, 7, 1, 0, 0), ("generate_mips_layers", 0, 7, 0, 1, 0),
                                     ("write_layers", 0, 8, 1, 2, 0), ("generate_mips_layers", 0, 8, 0, 1, 0),
                                     ("write_layers", 0, 10, 1, 0, 0), ("generate_mips_layers", 0, 10, 0, 1, 0)]
    lib.mock_log_clear(ctx)
    r.render()
    assert texture_log(lib, ctx) == []
    r.close()


def test_a_flagged_array_is_created_and_the_lazy_mirror_is_the_numpy_restatement(pool_mock):
    so, lib = pool_mock
    h = H.Host(so)
    h.resize(32, 32)
    imgs = [noise(30 + i, 8) for i in range(4)]
    for i in (0, 1):
        imgs[i][::2, ::3, 3] = 0
        imgs[i][1::2, ::3, 3] = 255
    ids = [h.texture_insert(imgs[0], 0, srgb=True), h.texture_insert(imgs[1], 4, srgb=True, premultiply=True),
           h.texture_insert(imgs[2], 1), h.texture_insert(imgs[3], 0, premultiply=True)]
    assert ids == [0, 1, 2, 3]
    want = np.stack([ref.convert(imgs[0], 2), ref.convert(imgs[1], 3), imgs[2], ref.convert(imgs[3], 1)])
    assert (h.pool_arrays()[0] == want).all()
    assert (h.pool_arrays()[0] == want).all()                   # asked twice: converted once
    # the mirror was asked first, so the converted bytes travel with no flags left to apply
    h.env((0, 0, 0, 1), (1, 1, 1), (1, 1, 1), LUT)
    h.camera_update(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), (0, 0, 0))
    lib.mock_log_clear(h.device_ctx)
    h.render()
    assert texture_log(lib, h.device_ctx) == [("upload", 0), ("generate_mips", 0)]
    h.texture_update(1, imgs[0])                                   # new pixels, the flags it was inserted with
    want[1] = ref.convert(imgs[0], 3)
    lib.mock_log_clear(h.device_ctx)
    h.render()
    assert texture_log(lib, h.device_ctx) == [("write_layers", 0, 1, 1, 3, 4), ("generate_mips_layers", 0, 1, 0, 1, 0)]
    assert (h.pool_arrays()[0] == want).all()
    h.close()
    # not asked first: the array is created and the flags travel
    h = H.Host(so)
    h.resize(32, 32)
    h.texture_insert(imgs[0], 0, srgb=True)
    h.texture_insert(imgs[2], 1)
    h.env((0, 0, 0, 1), (1, 1, 1), (1, 1, 1), LUT)
    h.camera_update(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), (0, 0, 0))
    lib.mock_log_clear(h.device_ctx)
    h.render()
    assert texture_log(lib, h.device_ctx) == [("create", 0, 8, 8, 2, 4), ("write_layers", 0, 0, 1, 2, 0), ("write_layers", 0, 1, 1, 0, 1), ("generate_mips_layers", 0, 0, 0, 2, 0)]
    assert (h.pool_arrays()[0] == np.stack([ref.convert(imgs[0], 2), imgs[2]])).all()
    h.close()


def test_gltf_option_keys_pool_entries_by_texture_and_colour_info(pool_mock, tmp_path):
    """base colour + occlusion from one image: two layers, the first decoded; without the option one layer, as stored."""
    from awsm_renderer_amd import gltf_export
    import dataclasses
    so, _ = pool_mock
    sc = small_scene()
    m = dataclasses.replace(sc.materials[0], occlusion_tex=scenes.TextureRef(0), emissive_tex=scenes.TextureRef(3))
    enc = dataclasses.replace(sc, textures=[sc.textures[0], sc.textures[1], sc.textures[2], sc.textures[4]], materials=[m])
    path = str(tmp_path / "enc.glb")
    gltf_export.write_glb(enc, path)
    r = H.Renderer(sc, backend_path=so, lut_rgba16f=LUT, gltf=path, srgb_textures=True)
    pool = r.host.pool_arrays()
    want = np.stack([ref.convert(sc.textures[0], 2), sc.textures[1], sc.textures[2], sc.textures[0], ref.convert(sc.textures[4], 2)])
    assert len(pool) == 1 and (pool[0] == want).all()
    r.close()
    r = H.Renderer(sc, backend_path=so, lut_rgba16f=LUT, gltf=path)
    pool = r.host.pool_arrays()
    assert len(pool) == 1 and (pool[0] == np.stack(enc.textures)).all()
    r.close()
    r = H.Renderer(sc, backend_path=MOCK, lut_rgba16f=LUT, gltf=path)      # a backend without the symbols still loads a file as stored
    r.close()
    with pytest.raises(H.HostError, match="awsm_hip_texture_array_create"):
        H.Renderer(sc, backend_path=MOCK, lut_rgba16f=LUT, gltf=path, srgb_textures=True)
