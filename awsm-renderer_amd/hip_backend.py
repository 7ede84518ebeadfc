"""
hip_backend.py — thin ctypes binding of libawsm_hip.so (include/awsm_hip.h).  No fallback: if the HIP library
is missing or fails to load, importing callers get an exception.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import PACKAGE_DIR

LIB_PATH = os.environ.get("AWSM_HIP_LIB") or os.path.join(PACKAGE_DIR, "libawsm_hip.so")   # AWSM_HIP_LIB: A/B builds of the same ABI
BUF_COUNT = 19
AWSM_CFG_PARITY_TAP = 1
AWSM_CFG_SMALL_BIN_LIST = 2
AWSM_CFG_OVERLAP_FRAMES = 4
AWSM_CFG_GENERAL_SHADE_ONLY = 8
AWSM_CFG_ANISOTROPIC = 16

BUF_NAMES = ["TRANSFORMS", "NORMAL_MATS", "MATERIALS", "LIGHTS", "LIGHTS_INFO", "CAMERA", "SKIN_MATRICES", "SKIN_INDEX_WEIGHTS",
             "MORPH_WEIGHTS", "MORPH_VALUES", "GEOM_META", "MATERIAL_META", "VIS_GEOM_DATA", "VIS_GEOM_INDEX", "ATTR_DATA", "ATTR_INDEX",
             "TEXTURE_TRANSFORMS", "INSTANCES", "TRANSPARENCY_GEOM_DATA"]

# every symbol include/awsm_hip.h declares (tests/test_abi_symbols.py checks the header against this list too)
EXPORTS = ["awsm_hip_create", "awsm_hip_destroy", "awsm_hip_last_error", "awsm_hip_abi_version", "awsm_hip_buffer_create",
           "awsm_hip_buffer_write", "awsm_hip_resize", "awsm_hip_set_shard_rows", "awsm_hip_set_shard_bands", "awsm_hip_set_stage_timers", "awsm_hip_pick", "awsm_hip_texture_array_upload", "awsm_hip_texture_array_generate_mips", "awsm_hip_texture_array_read_level", "awsm_hip_sampler_set",
           "awsm_hip_env_upload", "awsm_hip_brdf_lut_generate", "awsm_hip_read_brdf_lut", "awsm_hip_geometry_pass", "awsm_hip_opaque_pass",
           "awsm_hip_frame_end", "awsm_hip_frame_flush", "awsm_hip_read_gbuffer", "awsm_hip_stream_handoff", "awsm_hip_bind_output", "awsm_hip_output_device_ptr", "awsm_hip_read_visibility",
           "awsm_hip_read_visibility_unpacked", "awsm_hip_read_opaque", "awsm_hip_read_opaque_f32", "awsm_hip_read_transformed",
           "awsm_hip_device_info", "awsm_hip_transparent_pass", "awsm_hip_read_composite", "awsm_hip_read_composite_f32", "awsm_hip_bind_composite",
           "awsm_hip_read_transformed_forward", "awsm_hip_visibility_digest", "awsm_hip_bind_output_rows", "awsm_hip_env_cube_upload", "awsm_hip_bind_opaque_source", "awsm_hip_msaa_halo_bands", "awsm_hip_msaa_halo_export", "awsm_hip_msaa_halo_bind",
           "awsm_hip_frame_trace", "awsm_hip_read_frame_trace", "awsm_hip_hud_geometry_pass", "awsm_hip_hud_transparent_pass",
           "awsm_hip_post_pass", "awsm_hip_read_display", "awsm_hip_read_effects", "awsm_hip_bind_display", "awsm_hip_display_device_ptr",
           "awsm_hip_env_cube_create", "awsm_hip_env_cube_write_face", "awsm_hip_env_cube_write_all_faces", "awsm_hip_env_cube_generate_mips",
           "awsm_hip_env_cube_fill_colors", "awsm_hip_env_cube_fill_sky_gradient", "awsm_hip_env_cube_info", "awsm_hip_env_cube_read_level",
           "awsm_hip_env_cube_filter", "awsm_hip_env_cube_from_equirect",
           "awsm_hip_texture_array_create", "awsm_hip_texture_array_resize_layers", "awsm_hip_texture_array_write_layers",
           "awsm_hip_texture_array_generate_mips_layers", "awsm_hip_texture_array_info",
           "awsm_hip_skin_pose_records_write", "awsm_hip_skin_pose", "awsm_hip_buffer_read",
           "awsm_hip_editor_grid_defaults", "awsm_hip_set_editor_grid", "awsm_hip_read_editor_grid",
           "awsm_hip_ssao_defaults", "awsm_hip_set_ssao", "awsm_hip_read_ssao",
           "awsm_hip_shadow_defaults", "awsm_hip_shadow_pass", "awsm_hip_read_shadow_map", "awsm_hip_read_shadow",
           "awsm_hip_shadow_pass_views", "awsm_hip_read_shadow_map_view", "awsm_hip_read_shadow_view",
           "awsm_hip_selection_defaults", "awsm_hip_set_selection", "awsm_hip_read_selection",
           "awsm_hip_taa_defaults", "awsm_hip_set_taa", "awsm_hip_read_taa",
           "awsm_hip_pick_query_defaults", "awsm_hip_pick_ex", "awsm_hip_pick_rect", "awsm_hip_read_pick_map"]

AWSM_PICK_TRANSPARENT = 1
PICK_LAYERS = ("world", "world_transparent", "hud", "hud_transparent")      # AwsmPickHit.layer / AwsmPickRectEntry.layer
PICK_MISS = 0xFFFFFFFF                                                      # read_pick_map's word where nothing is hit


class AwsmPickQuery(C.Structure):
    """A pick query (awsm_hip_pick_ex / pick_rect / read_pick_map): AWSM_PICK_TRANSPARENT and the alpha a fragment must have been blended with."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("alpha_threshold", C.c_float)]


class AwsmPickHit(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("mesh_key_high", C.c_uint32), ("mesh_key_low", C.c_uint32), ("triangle_index", C.c_uint32), ("layer", C.c_uint32),
                ("alpha", C.c_float), ("depth_bits", C.c_uint32)]


class AwsmPickRectEntry(C.Structure):
    _fields_ = [("layer", C.c_uint32), ("mesh_key_high", C.c_uint32), ("mesh_key_low", C.c_uint32), ("pixels", C.c_uint32)]


class AwsmConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32), ("stream", C.c_void_p)]


class AwsmDraw(C.Structure):
    _fields_ = [("geom_meta_off", C.c_uint32), ("vis_data_off", C.c_uint32), ("tri_count", C.c_uint32), ("flags", C.c_uint32),
                ("inst_off", C.c_uint32), ("inst_count", C.c_uint32)]


class AwsmOpaqueParams(C.Structure):
    _fields_ = [("mipmap", C.c_uint32), ("has_opaque", C.c_uint32)]


class AwsmPostParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tonemapping", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AwsmEditorGrid(C.Structure):
    """The editor's ground grid (awsm_hip_set_editor_grid): the constants of grid.wgsl:87-98 as a record."""
    _fields_ = [("struct_size", C.c_uint32), ("color_background", C.c_float * 3), ("alpha_background", C.c_float), ("color_minor", C.c_float * 3), ("alpha_minor", C.c_float),
                ("color_major", C.c_float * 3), ("alpha_major", C.c_float), ("color_z_axis", C.c_float * 3), ("alpha_axis", C.c_float),
                ("color_x_axis", C.c_float * 3), ("depth_epsilon", C.c_float)]

    def override(self, **overrides):
        """Set fields by name (a colour from any three numbers); an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k == "struct_size":
                raise TypeError("AwsmEditorGrid has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[1:])))
            setattr(self, k, (C.c_float * 3)(*v) if k.startswith("color_") else float(v))
        return self


class AwsmSsao(C.Structure):
    """Screen-space ambient occlusion (awsm_hip_set_ssao): radius in world units, intensity, bias as a fraction of the radius, strength 0 .. 1."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_float), ("intensity", C.c_float), ("bias", C.c_float), ("strength", C.c_float)]

    def override(self, **overrides):
        """Set fields by name; an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k == "struct_size":
                raise TypeError("AwsmSsao has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[1:])))
            setattr(self, k, float(v))
        return self


AWSM_TAA_RESET = 1


class AwsmTaa(C.Structure):
    """Temporal anti-aliasing (awsm_hip_set_taa): the weight of the current image, AWSM_TAA_RESET, the NDC offset the frame's projection was
    translated by, and the column-major matrix from this frame's unjittered NDC to the previous frame's unjittered clip space."""
    _fields_ = [("struct_size", C.c_uint32), ("feedback", C.c_float), ("flags", C.c_uint32), ("jitter_ndc", C.c_float * 2), ("reproject", C.c_float * 16)]

    def override(self, **overrides):
        """Set fields by name (a sequence for jitter_ndc and reproject); an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k == "struct_size":
                raise TypeError("AwsmTaa has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[1:])))
            if k == "flags":
                self.flags = int(v)
            elif k == "feedback":
                self.feedback = float(v)
            else:
                vals = [float(x) for x in np.asarray(v, dtype=np.float32).reshape(-1)]
                if len(vals) != len(getattr(self, k)):
                    raise ValueError("AwsmTaa.%s takes %d values" % (k, len(getattr(self, k))))
                setattr(self, k, names[k](*vals))
        return self


class AwsmShadow(C.Structure):
    """One shadowed light (awsm_hip_shadow_pass): map_size S, pcf_radius R, light = (unit vector towards the light, 0) or (position, 1), the depth
    bias, the slope bias, the largest slope (NDC depth per texel), strength 0 .. 1, and the cosine from which a surface counts as facing the light."""
    _fields_ = [("struct_size", C.c_uint32), ("map_size", C.c_uint32), ("pcf_radius", C.c_uint32), ("light", C.c_float * 4),
                ("bias", C.c_float), ("slope_bias", C.c_float), ("max_slope", C.c_float), ("strength", C.c_float), ("facing_fade", C.c_float)]

    def override(self, **overrides):
        """Set fields by name; an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k == "struct_size":
                raise TypeError("AwsmShadow has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[1:])))
            if k == "light":
                self.light = (C.c_float * 4)(*[float(x) for x in v])
            else:
                setattr(self, k, int(v) if k in ("map_size", "pcf_radius") else float(v))
        return self


AWSM_SHADOW_MAX_VIEWS = 6
SHADOW_NO_VIEW = 255      # read_shadow_view's byte of a pixel that lies in no view


class AwsmShadowView(C.Structure):
    """One view of awsm_hip_shadow_pass_views: a 512-byte light block and the draws that cast in it."""
    _fields_ = [("light_camera", C.c_void_p), ("camera_bytes", C.c_size_t), ("casters", C.c_void_p), ("n_casters", C.c_uint32)]


AWSM_SELECTION_OUTLINE, AWSM_SELECTION_BOXES = 1, 2


class AwsmSelection(C.Structure):
    """The editor's selection overlay (awsm_hip_set_selection): flags (outline, boxes), the outline's radius in pixels and colour, the boxes' colour,
    half width in pixels, the factor on a box fragment behind the world's depth, and what is subtracted from a fragment's depth before the test."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("outline_radius", C.c_uint32), ("outline_color", C.c_float * 4), ("box_color", C.c_float * 4),
                ("box_half_width", C.c_float), ("hidden_alpha", C.c_float), ("depth_epsilon", C.c_float)]

    def override(self, **overrides):
        """Set fields by name (a colour from any four numbers); an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k == "struct_size":
                raise TypeError("AwsmSelection has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[1:])))
            setattr(self, k, (C.c_float * 4)(*[float(x) for x in v]) if k.endswith("_color") else int(v) if k in ("flags", "outline_radius") else float(v))
        return self


def selection_key_words(mesh_keys) -> np.ndarray:
    """Mesh keys as the device takes them: [n, 2] uint32 {high, low}, from 64-bit keys or from (high, low) pairs."""
    if len(mesh_keys) == 0:
        return np.zeros((0, 2), np.uint32)
    if np.ndim(mesh_keys[0]) == 1:
        return np.ascontiguousarray(np.array([[int(h), int(l)] for h, l in mesh_keys], dtype=np.uint32))
    a = np.array([int(k) for k in mesh_keys], dtype=np.uint64)
    return np.ascontiguousarray(np.stack([a >> np.uint64(32), a & np.uint64(0xFFFFFFFF)], axis=-1).astype(np.uint32))


class AwsmCubeLayout(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bytes_per_row", C.c_uint32), ("rows_per_image", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64)]


class AwsmEnvFilter(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("size", C.c_uint32), ("mips", C.c_uint32), ("sample_count", C.c_uint32), ("reserved", C.c_uint32)]


class AwsmEquirect(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("bytes_per_row", C.c_uint32),
                ("samples", C.c_uint32), ("yaw", C.c_float), ("scale", C.c_float)]


AWSM_PANO_RGBE8, AWSM_PANO_RGBA32F = 0, 1


def equirect_source(array, yaw=0.0, samples=0, scale=1.0):
    """(contiguous array, AwsmEquirect) for a panorama: uint8 [H, W, 4] is RGBE, float32 [H, W, 4] is RGBA32F; anything else is a TypeError."""
    a = np.ascontiguousarray(array)
    if a.ndim != 3 or a.shape[2] != 4 or a.dtype not in (np.uint8, np.float32):
        raise TypeError("a panorama is uint8 [H, W, 4] (RGBE) or float32 [H, W, 4], got %s %s" % (a.dtype, a.shape))
    fmt = AWSM_PANO_RGBE8 if a.dtype == np.uint8 else AWSM_PANO_RGBA32F
    return a, AwsmEquirect(C.sizeof(AwsmEquirect), a.shape[1], a.shape[0], fmt, 0, samples, yaw, scale)


class AwsmTexWrite(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_uint32), ("flags", C.c_uint32), ("mipmap_kind", C.c_uint32),
                ("bytes_per_row", C.c_uint32), ("rows_per_image", C.c_uint32), ("offset", C.c_uint64)]


AWSM_TEX_PREMULTIPLY_ALPHA, AWSM_TEX_SRGB_TO_LINEAR = 1, 2

ENV_FILTER_KINDS = {"ggx": 0, "lambert": 1}

# AwsmCubeFormat: name -> (value, bytes per texel)
CUBE_FORMATS = {"rgba16f": (0, 8), "rgba32f": (1, 16), "rgba8unorm": (2, 4), "rgba8unorm-srgb": (3, 4), "bgra8unorm": (4, 4), "bgra8unorm-srgb": (5, 4),
                "rg11b10ufloat": (6, 4), "rgb9e5ufloat": (7, 4)}
CUBE_FORMAT_NAMES = {v[0]: k for k, v in CUBE_FORMATS.items()}
DEFAULT_SKY_ZENITH, DEFAULT_SKY_NADIR = (0.4, 0.65, 1.0, 1.0), (0.55, 0.45, 0.35, 1.0)      # CubemapSkyGradient::default (cubemap/images.rs:54-61)


def cube_source(data, fmt, width, bytes_per_row=None, rows_per_image=None, offset=0):
    """(format value, contiguous uint8 view of `data`, AwsmCubeLayout) for the cube writes; the layout defaults to the tight one."""
    value, bpt = CUBE_FORMATS[fmt] if isinstance(fmt, str) else (int(fmt), {0: 8, 1: 16}.get(int(fmt), 4))
    raw = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    layout = AwsmCubeLayout(C.sizeof(AwsmCubeLayout), width * bpt if bytes_per_row is None else bytes_per_row,
                            width if rows_per_image is None else rows_per_image, 0, offset)
    return value, raw, layout


AWSM_POST_SMAA, AWSM_POST_BLOOM, AWSM_POST_DOF = 1, 2, 4
TONEMAP = {"none": 0, "khronos": 1, "aces": 2}


class AwsmSampler(C.Structure):
    _fields_ = [("address_mode_u", C.c_uint32), ("address_mode_v", C.c_uint32), ("mag_filter", C.c_uint32), ("min_filter", C.c_uint32),
                ("mipmap_filter", C.c_uint32), ("max_anisotropy", C.c_uint32)]


class AwsmEnv(C.Structure):
    _fields_ = [("skybox_rgba", C.c_float * 4), ("prefiltered_rgb", C.c_float * 4), ("irradiance_rgb", C.c_float * 4),
                ("brdf_lut_width", C.c_uint32), ("brdf_lut_height", C.c_uint32), ("brdf_lut_rgba16f", C.c_void_p)]


class AwsmFrameStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ms_transform", C.c_float), ("ms_bin", C.c_float), ("ms_raster", C.c_float), ("ms_shade", C.c_float), ("ms_total", C.c_float),
                ("triangles_in", C.c_uint32), ("triangles_binned", C.c_uint32), ("bin_entries", C.c_uint32), ("covered_pixels", C.c_uint32),
                ("bin_overflow_retries", C.c_uint32), ("ms_forward", C.c_float), ("forward_triangles", C.c_uint32), ("forward_fragment_slots", C.c_uint32),
                ("ms_shade_lean", C.c_float), ("shade_general_wavefronts", C.c_uint32), ("frames_with_dropped_bin_entries", C.c_uint32),
                ("handoff_gate_timeouts", C.c_uint32), ("geometry_cache_blocks", C.c_uint32), ("geometry_blocks", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k not in ("reserved", "struct_size")}


class AwsmHipError(RuntimeError):
    def __init__(self, code: int, where: str, text: str):
        super().__init__(f"{where} failed with status {code}: {text}")
        self.code = code


_lib = None


def load_library():
    """dlopen libawsm_hip.so.  Raises if it is missing — there is no CPU fallback for the product path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950); awsm-renderer_amd has no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    lib.awsm_hip_last_error.restype = C.c_char_p
    lib.awsm_hip_last_error.argtypes = [C.c_void_p]
    lib.awsm_hip_abi_version.restype = C.c_uint32
    lib.awsm_hip_output_device_ptr.restype = C.c_void_p
    lib.awsm_hip_output_device_ptr.argtypes = [C.c_void_p]
    lib.awsm_hip_buffer_create.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.awsm_hip_buffer_write.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.awsm_hip_bind_output.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_bind_output_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]
    lib.awsm_hip_geometry_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_opaque_pass.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_frame_end.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_frame_flush.argtypes = [C.c_void_p]
    lib.awsm_hip_resize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.awsm_hip_set_shard_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.awsm_hip_set_stage_timers.argtypes = [C.c_void_p, C.c_int]
    lib.awsm_hip_set_shard_bands.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.awsm_hip_pick.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.awsm_hip_texture_array_generate_mips.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.awsm_hip_texture_array_read_level.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.awsm_hip_texture_array_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.awsm_hip_texture_array_resize_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.awsm_hip_texture_array_write_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.awsm_hip_texture_array_generate_mips_layers.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.awsm_hip_texture_array_info.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_texture_array_upload.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    lib.awsm_hip_sampler_set.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.awsm_hip_env_upload.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_env_cube_upload.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.awsm_hip_brdf_lut_generate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.awsm_hip_read_brdf_lut.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_visibility.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_visibility_digest.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_visibility_unpacked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_opaque.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_opaque_f32.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_transformed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_device_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.awsm_hip_destroy.argtypes = [C.c_void_p]
    lib.awsm_hip_transparent_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_read_composite.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_composite_f32.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_bind_composite.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_bind_opaque_source.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_msaa_halo_bands.argtypes = [C.c_void_p]
    lib.awsm_hip_msaa_halo_bands.restype = C.c_uint32
    lib.awsm_hip_msaa_halo_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_msaa_halo_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_read_transformed_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_hud_geometry_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_hud_transparent_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_frame_trace.argtypes = [C.c_void_p, C.c_uint32]
    lib.awsm_hip_post_pass.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_display.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_effects.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_bind_display.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.awsm_hip_display_device_ptr.restype = C.c_void_p
    lib.awsm_hip_display_device_ptr.argtypes = [C.c_void_p]
    lib.awsm_hip_read_frame_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.awsm_hip_env_cube_create.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    lib.awsm_hip_env_cube_write_face.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.awsm_hip_env_cube_write_all_faces.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.awsm_hip_env_cube_generate_mips.argtypes = [C.c_void_p, C.c_int]
    lib.awsm_hip_env_cube_fill_colors.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    lib.awsm_hip_env_cube_fill_sky_gradient.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.awsm_hip_env_cube_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.awsm_hip_env_cube_read_level.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    lib.awsm_hip_env_cube_filter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.awsm_hip_env_cube_from_equirect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.awsm_hip_skin_pose_records_write.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.awsm_hip_skin_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_buffer_read.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.awsm_hip_editor_grid_defaults.argtypes = [C.c_void_p]
    lib.awsm_hip_set_editor_grid.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_editor_grid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_selection_defaults.argtypes = [C.c_void_p]
    lib.awsm_hip_set_selection.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.awsm_hip_read_selection.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_ssao_defaults.argtypes = [C.c_void_p]
    lib.awsm_hip_set_ssao.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_ssao.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_taa_defaults.argtypes = [C.c_void_p]
    lib.awsm_hip_set_taa.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_taa.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_shadow_defaults.argtypes = [C.c_void_p]
    lib.awsm_hip_shadow_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]
    lib.awsm_hip_read_shadow_map.argtypes = [C.c_void_p, C.c_void_p]
    lib.awsm_hip_read_shadow.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.awsm_hip_shadow_pass_views.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.awsm_hip_read_shadow_map_view.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    lib.awsm_hip_read_shadow_view.argtypes = [C.c_void_p, C.c_void_p]
    # optional symbols (AWSM_HIP_ABI_VERSION unchanged): a library of the same ABI built without them loads, and the methods that need them say so
    for name, argtypes in (("awsm_hip_pick_query_defaults", [C.c_void_p]), ("awsm_hip_pick_ex", [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
                           ("awsm_hip_pick_rect", [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
                           ("awsm_hip_read_pick_map", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    _lib = lib
    return lib


class HipDevice:
    """One AwsmHipCtx: one HIP device + stream."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, parity_tap: bool = False, small_bin_list: bool = False, overlap_frames: bool = False,
                 general_shade_only: bool = False, anisotropic: bool = False):
        self.lib = load_library()
        flags = (AWSM_CFG_ANISOTROPIC if anisotropic else 0) | (AWSM_CFG_PARITY_TAP if parity_tap else 0) | (AWSM_CFG_SMALL_BIN_LIST if small_bin_list else 0) | (AWSM_CFG_OVERLAP_FRAMES if overlap_frames else 0) | (AWSM_CFG_GENERAL_SHADE_ONLY if general_shade_only else 0)
        cfg = AwsmConfig(C.sizeof(AwsmConfig), self.lib.awsm_hip_abi_version(), device, flags, stream)
        ctx = C.c_void_p()
        rc = self.lib.awsm_hip_create(C.byref(cfg), C.byref(ctx))
        if rc != 0:
            raise AwsmHipError(rc, "awsm_hip_create", "no usable gfx950 device" if rc == -4 else "see status code")
        self.ctx = ctx
        self.owns = True
        self.width = self.height = 0
        self.lut_size = (0, 0)
        self._shadow_size = None      # map_size of the last shadow_pass made through this object (read_shadow_map's default)

    @classmethod
    def from_ctx(cls, ctx: int, width: int, height: int) -> "HipDevice":
        """Non-owning view over an AwsmHipCtx created elsewhere (the host layer's), for the readback helpers."""
        self = cls.__new__(cls)
        self.lib, self.ctx, self.owns = load_library(), C.c_void_p(ctx), False
        self.width, self.height, self.lut_size = width, height, (0, 0)
        self._shadow_size = None
        return self

    def _chk(self, rc: int, where: str):
        if rc != 0:
            raise AwsmHipError(rc, where, (self.lib.awsm_hip_last_error(self.ctx) or b"").decode())

    def close(self):
        if self.ctx and self.owns:
            self.lib.awsm_hip_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- buffers ----
    def buffer_create(self, which: int, nbytes: int):
        self._chk(self.lib.awsm_hip_buffer_create(self.ctx, which, nbytes), f"buffer_create({BUF_NAMES[which]})")

    def buffer_write(self, which: int, offset: int, data):
        arr = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        self._chk(self.lib.awsm_hip_buffer_write(self.ctx, which, offset, arr.ctypes.data_as(C.c_void_p), arr.nbytes), f"buffer_write({BUF_NAMES[which]})")

    def buffer_read(self, which: int, offset: int, nbytes: int) -> bytes:
        """awsm_hip_buffer_read: a synchronising read-back of a scene buffer (tests, diagnostics)."""
        out = np.zeros(max(1, nbytes), dtype=np.uint8)
        self._chk(self.lib.awsm_hip_buffer_read(self.ctx, which, offset, out.ctypes.data_as(C.c_void_p), nbytes), f"buffer_read({BUF_NAMES[which]})")
        return out[:nbytes].tobytes()

    def skin_pose_records_write(self, first: int, records: np.ndarray):
        """records: (n, 18) uint32 / float32 words — transform_offset, matrix_offset, inverse_bind[16] (AwsmSkinPoseRecord)."""
        r = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 18)
        self._chk(self.lib.awsm_hip_skin_pose_records_write(self.ctx, first, r.shape[0], r.ctypes.data_as(C.c_void_p)), "skin_pose_records_write")

    def skin_pose(self, record_ids):
        """awsm_hip_skin_pose: AWSM_BUF_SKIN_MATRICES[matrix_offset] = world * inverse_bind for the listed records."""
        ids = np.ascontiguousarray(record_ids, dtype=np.uint32)
        self._chk(self.lib.awsm_hip_skin_pose(self.ctx, ids.ctypes.data_as(C.c_void_p), ids.size), "skin_pose")

    def upload_mirrors(self, mirrors: Dict[int, bytes]):
        """create + full write of every mirror (what the reference does on the first frame / after a resize)."""
        for which, data in mirrors.items():
            n = (len(data) + 3) & ~3
            self.buffer_create(which, n)
            if len(data):
                self.buffer_write(which, 0, np.frombuffer(bytes(data) + bytes(n - len(data)), dtype=np.uint8))

    # ---- targets / environment ----
    def resize(self, width: int, height: int, msaa: int = 0):
        self._chk(self.lib.awsm_hip_resize(self.ctx, width, height, msaa), "resize")
        self.width, self.height, self.msaa = width, height, (4 if msaa == 4 else 0)

    def set_shard_rows(self, y0: int, y1: int):
        self._chk(self.lib.awsm_hip_set_shard_rows(self.ctx, y0, y1), "set_shard_rows")

    def pick(self, x: int, y: int):
        """picker.rs:55-121 -> (mesh_key u64, primitive-local triangle index) or None for background / outside the frame."""
        out = (C.c_uint32 * 4)()
        self._chk(self.lib.awsm_hip_pick(self.ctx, x, y, out), "pick")
        return ((out[1] << 32) | out[2], out[3]) if out[0] else None

    def _pick_fn(self, name: str):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise AwsmHipError(-6, name, "%s does not export %s" % (LIB_PATH, name))
        return fn

    def _pick_query(self, transparent, alpha_threshold, struct_size=None, flags=None):
        q = AwsmPickQuery(C.sizeof(AwsmPickQuery) if struct_size is None else struct_size,
                          (AWSM_PICK_TRANSPARENT if transparent else 0) if flags is None else flags, alpha_threshold)
        return C.byref(q)

    def pick_ex(self, x: int, y: int, transparent: bool = False, alpha_threshold: float = 0.5, **raw):
        """awsm_hip_pick_ex: the hit at (x, y) of the last submitted frame, through the transparent passes' fragment lists when `transparent` ->
        dict(mesh_key, triangle_index, layer, alpha, depth_bits) or None.  layer indexes PICK_LAYERS.  raw: struct_size / flags as given (tests)."""
        hit = AwsmPickHit()
        self._chk(self._pick_fn("awsm_hip_pick_ex")(self.ctx, x, y, self._pick_query(transparent, alpha_threshold, **raw), C.byref(hit)), "pick_ex")
        if not hit.valid:
            return None
        return {"mesh_key": (hit.mesh_key_high << 32) | hit.mesh_key_low, "triangle_index": hit.triangle_index, "layer": hit.layer, "alpha": hit.alpha,
                "depth_bits": hit.depth_bits}

    def pick_rect(self, x0: int, y0: int, x1: int, y1: int, transparent: bool = False, alpha_threshold: float = 0.5, cap: int = 4096, **raw):
        """awsm_hip_pick_rect over [x0, x1) x [y0, y1) -> ([(layer, mesh_key, pixels)] of at most `cap` entries, the number of distinct pairs)."""
        out = (AwsmPickRectEntry * max(1, cap))()
        n = C.c_uint32(0)
        self._chk(self._pick_fn("awsm_hip_pick_rect")(self.ctx, x0, y0, x1, y1, self._pick_query(transparent, alpha_threshold, **raw), out if cap else None, cap,
                                                      C.byref(n)), "pick_rect")
        return [(e.layer, (e.mesh_key_high << 32) | e.mesh_key_low, e.pixels) for e in out[:min(n.value, cap)]], n.value

    def read_pick_map(self, transparent: bool = False, alpha_threshold: float = 0.5, **raw):
        """awsm_hip_read_pick_map -> (word [H, W] uint32: layer << 28 | draw index in its pass's expanded list, PICK_MISS for a miss;
        triangle [H, W] uint32)."""
        word = np.zeros((self.height, self.width), np.uint32)
        tri = np.zeros((self.height, self.width), np.uint32)
        self._chk(self._pick_fn("awsm_hip_read_pick_map")(self.ctx, self._pick_query(transparent, alpha_threshold, **raw), word.ctypes.data, tri.ctypes.data), "read_pick_map")
        return word, tri

    def set_stage_timers(self, enabled: bool):
        """hipEventRecord between the stages of a frame (frame_end's ms_* fields); off = no bubbles between the kernels."""
        self._chk(self.lib.awsm_hip_set_stage_timers(self.ctx, 1 if enabled else 0), "set_stage_timers")

    def set_shard_bands(self, n: int, r: int, compact_output: bool = False):
        self._chk(self.lib.awsm_hip_set_shard_bands(self.ctx, n, r, 1 if compact_output else 0), "set_shard_bands")

    def texture_array_upload(self, index: int, texels: np.ndarray, mips: int = 1):
        """Level 0 of a pool array; `mips` levels are reserved (see texture_array_generate_mips)."""
        layers, h, w, _ = texels.shape
        t = np.ascontiguousarray(texels, dtype=np.uint8)
        self._chk(self.lib.awsm_hip_texture_array_upload(self.ctx, index, w, h, layers, mips, 0, t.ctypes.data_as(C.c_void_p)), "texture_array_upload")
        self._tex_shapes = getattr(self, "_tex_shapes", {})
        self._tex_shapes[index] = (layers, h, w)

    def texture_array_generate_mips(self, index: int, kinds=None):
        layers = self._tex_shapes[index][0]
        k = None if kinds is None else (C.c_uint32 * layers)(*[int(x) for x in kinds])
        self._chk(self.lib.awsm_hip_texture_array_generate_mips(self.ctx, index, k), "texture_array_generate_mips")

    # ---- the texture pool at run time ----
    def texture_array_create(self, index: int, width: int, height: int, layers: int, mips: int = 1):
        """A zero-filled array; `mips` levels are reserved."""
        self._chk(self.lib.awsm_hip_texture_array_create(self.ctx, index, width, height, layers, mips), "texture_array_create")

    def texture_array_resize_layers(self, index: int, layers: int):
        """More layers: the existing ones keep every level, the new ones read zero."""
        self._chk(self.lib.awsm_hip_texture_array_resize_layers(self.ctx, index, layers), "texture_array_resize_layers")

    def texture_array_write_layers(self, index: int, first_layer: int, data, n_layers: Optional[int] = None, flags: int = 0, mip_kind: int = 0,
                                   bytes_per_row: Optional[int] = None, rows_per_image: Optional[int] = None, offset: int = 0, fmt: int = 0,
                                   struct_size: Optional[int] = None):
        """Level 0 of layers [first_layer, +n): an (n, h, w, 4) uint8 array, or raw bytes with a layout; flags = AWSM_TEX_*."""
        w, h, _, _ = self.texture_array_info(index)
        if isinstance(data, (bytes, bytearray, memoryview)):
            raw = np.frombuffer(data, dtype=np.uint8)
        else:
            if n_layers is None and getattr(data, "ndim", 0) == 4:
                n_layers = data.shape[0]
            raw = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        wr = AwsmTexWrite(C.sizeof(AwsmTexWrite) if struct_size is None else struct_size, fmt, flags, mip_kind, w * 4 if bytes_per_row is None else bytes_per_row,
                          h if rows_per_image is None else rows_per_image, offset)
        self._chk(self.lib.awsm_hip_texture_array_write_layers(self.ctx, index, first_layer, 1 if n_layers is None else n_layers,
                                                               raw.ctypes.data_as(C.c_void_p) if raw.size else None, raw.nbytes, C.byref(wr)), "texture_array_write_layers")

    def texture_array_generate_mips_layers(self, index: int, first_layer: int, n_layers: int):
        self._chk(self.lib.awsm_hip_texture_array_generate_mips_layers(self.ctx, index, first_layer, n_layers), "texture_array_generate_mips_layers")

    def texture_array_info(self, index: int):
        """-> (width, height, layers, mips) of an array the device holds."""
        v = [C.c_uint32(0) for _ in range(4)]
        self._chk(self.lib.awsm_hip_texture_array_info(self.ctx, index, *[C.byref(x) for x in v]), "texture_array_info")
        return tuple(int(x.value) for x in v)

    def texture_array_read_level(self, index: int, level: int) -> np.ndarray:
        w, h, layers, _ = self.texture_array_info(index)      # the device knows: the array may have been created, resized, or be a host's
        out = np.zeros((layers, max(1, h >> level), max(1, w >> level), 4), dtype=np.uint8)
        self._chk(self.lib.awsm_hip_texture_array_read_level(self.ctx, index, level, out.ctypes.data_as(C.c_void_p)), "texture_array_read_level")
        return out

    def sampler_set(self, index: int, s: dict):
        smp = AwsmSampler(s.get("address_mode_u", 1), s.get("address_mode_v", 1), s.get("mag_filter", 1), s.get("min_filter", 1),
                          s.get("mipmap_filter", 1), s.get("max_anisotropy", 1))
        self._chk(self.lib.awsm_hip_sampler_set(self.ctx, index, C.byref(smp)), "sampler_set")

    def env_cube_upload(self, which: int, levels):
        """levels: [level0, level1, ...] of (6, N_l, N_l, 4) float16 (faces +X -X +Y -Y +Z -Z), or None for the uniform colour."""
        if not levels:
            self._chk(self.lib.awsm_hip_env_cube_upload(self.ctx, which, 0, 0, None), "env_cube_upload")
            return
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a, dtype=np.float16).reshape(-1) for a in levels])).view(np.uint16)
        self._chk(self.lib.awsm_hip_env_cube_upload(self.ctx, which, levels[0].shape[1], len(levels), flat.ctypes.data), "env_cube_upload")

    # ---- environment cubes at run time (environment.rs, textures.rs:118-165; awsm_hip.h) ----
    def env_cube_create(self, which: int, size: int, mips: int):
        """A zero-filled RGBA16F chain of `mips` levels in place of whatever the binding held."""
        self._chk(self.lib.awsm_hip_env_cube_create(self.ctx, which, size, mips), "env_cube_create")

    def env_cube_write_face(self, which: int, face: int, mip: int, data, fmt="rgba16f", width: Optional[int] = None, height: Optional[int] = None,
                            bytes_per_row: Optional[int] = None, rows_per_image: Optional[int] = None, offset: int = 0):
        """One face (0..5 = +X -X +Y -Y +Z -Z) of one level, in place.  data: an (N, N, 4) array of the format's element type (float16 / float32 / uint8),
        an (N, N) uint32 array for the packed formats, or raw bytes with width / height and, if not tight, the byte layout."""
        width = np.asarray(data).shape[1] if width is None else width
        value, raw, layout = cube_source(data, fmt, width, bytes_per_row, rows_per_image, offset)
        self._chk(self.lib.awsm_hip_env_cube_write_face(self.ctx, which, face, mip, width, width if height is None else height, value,
                                                        raw.ctypes.data_as(C.c_void_p), raw.nbytes, C.byref(layout)), "env_cube_write_face")

    def env_cube_write_all_faces(self, which: int, mip: int, data, fmt="rgba16f", width: Optional[int] = None, height: Optional[int] = None,
                                 bytes_per_row: Optional[int] = None, rows_per_image: Optional[int] = None, offset: int = 0):
        """All six faces of one level from one buffer in face order: a (6, N, N, 4) array ((6, N, N) uint32 for the packed formats) or raw bytes."""
        width = np.asarray(data).shape[2] if width is None else width
        value, raw, layout = cube_source(data, fmt, width, bytes_per_row, rows_per_image, offset)
        self._chk(self.lib.awsm_hip_env_cube_write_all_faces(self.ctx, which, mip, width, width if height is None else height, value,
                                                             raw.ctypes.data_as(C.c_void_p), raw.nbytes, C.byref(layout)), "env_cube_write_all_faces")

    def env_cube_generate_mips(self, which: int):
        """Levels 1.. from level 0 on the device (regenerate_skybox_mipmaps / regenerate_cubemap_texture_mipmaps)."""
        self._chk(self.lib.awsm_hip_env_cube_generate_mips(self.ctx, which), "env_cube_generate_mips")

    def env_cube_fill_colors(self, which: int, size: int, colors):
        """Skybox::new_colors / IblTexture::new_colors: one RGBA colour for all faces, or six in face order; full mip chain."""
        c = np.asarray(colors, dtype=np.float32).reshape(-1, 4)
        c = np.ascontiguousarray(np.tile(c, (6, 1)) if c.shape[0] == 1 else c)
        assert c.shape == (6, 4), "one RGBA colour or six"
        self._chk(self.lib.awsm_hip_env_cube_fill_colors(self.ctx, which, size, c.ctypes.data_as(C.c_void_p)), "env_cube_fill_colors")

    def env_cube_fill_sky_gradient(self, which: int, size: int, zenith=DEFAULT_SKY_ZENITH, nadir=DEFAULT_SKY_NADIR):
        """CubemapImage::new_sky_gradient: the side faces blend zenith (row 0) to nadir, +Y is the zenith, -Y the nadir colour; full mip chain."""
        z, n = (C.c_float * 4)(*zenith), (C.c_float * 4)(*nadir)
        self._chk(self.lib.awsm_hip_env_cube_fill_sky_gradient(self.ctx, which, size, z, n), "env_cube_fill_sky_gradient")

    def env_cube_info(self, which: int):
        """(size, mips) of a texel cube."""
        size, mips = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.awsm_hip_env_cube_info(self.ctx, which, C.byref(size), C.byref(mips)), "env_cube_info")
        return int(size.value), int(mips.value)

    def env_cube_read_level(self, which: int, level: int) -> np.ndarray:
        """One level of the cube as it is stored: (6, N, N, 4) float16."""
        size, mips = self.env_cube_info(which)
        n = max(size >> level, 1)
        out = np.zeros((6, n, n, 4), dtype=np.float16)
        self._chk(self.lib.awsm_hip_env_cube_read_level(self.ctx, which, level, out.ctypes.data_as(C.c_void_p)), "env_cube_read_level")
        return out

    def env_cube_filter(self, src: int, dst: int, kind="ggx", size: int = 0, mips: Optional[int] = None, sample_count: int = 0):
        """Cube `src` filtered into cube `dst`: kind "ggx" makes the prefiltered chain of `mips` levels (default: the full chain of
        `size`), "lambert" one level of irradiance.  size 0 takes the source's side; sample_count 0 means 1024.  The source should carry its mip chain."""
        k = ENV_FILTER_KINDS[kind] if isinstance(kind, str) else int(kind)
        if not size:
            size = self.env_cube_info(src)[0]
        if mips is None:
            mips = 1 if k == 1 else int(size).bit_length()
        f = AwsmEnvFilter(C.sizeof(AwsmEnvFilter), k, size, mips, sample_count, 0)
        self._chk(self.lib.awsm_hip_env_cube_filter(self.ctx, src, dst, C.byref(f)), "env_cube_filter")

    def env_cube_from_equirect(self, which: int, array, yaw: float = 0.0, samples: int = 0, scale: float = 1.0):
        """An equirectangular panorama (uint8 [H, W, 4] RGBE or float32 [H, W, 4]) projected into level 0 of an existing texel cube (DESIGN.md section
        16): row 0 is the zenith, the centre column looks along -Z at yaw 0.  samples 0 picks S from the sizes.  env_cube_generate_mips follows."""
        a, pano = equirect_source(array, yaw, samples, scale)
        self._chk(self.lib.awsm_hip_env_cube_from_equirect(self.ctx, which, a.ctypes.data_as(C.c_void_p), a.nbytes, C.byref(pano)), "env_cube_from_equirect")

    def env_upload(self, skybox=(0, 0, 0, 1), prefiltered=(1, 1, 1), irradiance=(1, 1, 1), lut_rgba16f: Optional[np.ndarray] = None):
        env = AwsmEnv()
        for i in range(4):
            env.skybox_rgba[i] = skybox[i]
        for i in range(3):
            env.prefiltered_rgb[i] = prefiltered[i]
            env.irradiance_rgb[i] = irradiance[i]
        keep = None
        if lut_rgba16f is not None:
            keep = np.ascontiguousarray(lut_rgba16f, dtype=np.uint16)
            env.brdf_lut_height, env.brdf_lut_width = keep.shape[0], keep.shape[1]
            env.brdf_lut_rgba16f = keep.ctypes.data
            self.lut_size = (keep.shape[1], keep.shape[0])
        self._chk(self.lib.awsm_hip_env_upload(self.ctx, C.byref(env)), "env_upload")

    def brdf_lut_generate(self, width: int, height: int):
        self._chk(self.lib.awsm_hip_brdf_lut_generate(self.ctx, width, height), "brdf_lut_generate")
        self.lut_size = (width, height)

    def read_brdf_lut(self) -> np.ndarray:
        w, h = self.lut_size
        out = np.zeros((h, w, 2), dtype=np.uint16)
        self._chk(self.lib.awsm_hip_read_brdf_lut(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_brdf_lut")
        return out

    # ---- passes ----
    @staticmethod
    def make_draws(draws: Sequence[dict]):
        arr = (AwsmDraw * max(1, len(draws)))()
        for i, d in enumerate(draws):
            arr[i] = AwsmDraw(d["geom_meta_off"], d["vis_data_off"], d["tri_count"], d["flags"], d.get("inst_off", 0), d.get("inst_count", 0))
        return arr

    def geometry_pass(self, draws, n: Optional[int] = None):
        if not isinstance(draws, C.Array):
            n = len(draws)
            draws = self.make_draws(draws)
        self._chk(self.lib.awsm_hip_geometry_pass(self.ctx, draws, n if n is not None else len(draws)), "geometry_pass")

    def opaque_pass(self, has_opaque: bool = True, mipmap: int = 0):
        p = AwsmOpaqueParams(mipmap, 1 if has_opaque else 0)
        self._chk(self.lib.awsm_hip_opaque_pass(self.ctx, C.byref(p)), "opaque_pass")

    def transparent_pass(self, draws, n: Optional[int] = None):
        """World transparent pass over the back-to-front draw list (after opaque_pass); the result is the composite image."""
        if not isinstance(draws, C.Array):
            n = len(draws)
            draws = self.make_draws(draws)
        self._chk(self.lib.awsm_hip_transparent_pass(self.ctx, draws, n if n is not None else len(draws)), "transparent_pass")

    def editor_grid_defaults(self) -> AwsmEditorGrid:
        g = AwsmEditorGrid()
        self._chk(self.lib.awsm_hip_editor_grid_defaults(C.byref(g)), "editor_grid_defaults")
        return g

    def set_editor_grid(self, on=True, struct_size: Optional[int] = None, **overrides):
        """The editor's ground grid in every later transparent_pass: the defaults of grid.wgsl with `overrides` (AwsmEditorGrid's field names);
        set_editor_grid(None) turns it off.  struct_size: what the record claims as its size (tests)."""
        if not on:
            return self._chk(self.lib.awsm_hip_set_editor_grid(self.ctx, None), "set_editor_grid")
        g = self.editor_grid_defaults().override(**overrides)
        if struct_size is not None:
            g.struct_size = struct_size
        self._chk(self.lib.awsm_hip_set_editor_grid(self.ctx, C.byref(g)), "set_editor_grid")

    def read_editor_grid(self):
        """The raw grid layer for the last submitted frame's camera and size -> (rgba float32 [H, W, 4], depth float32 [H, W], kept bool [H, W])."""
        rgba = np.empty((self.height, self.width, 4), np.float32)
        depth = np.empty((self.height, self.width), np.float32)
        kept = np.empty((self.height, self.width), np.uint8)
        self._chk(self.lib.awsm_hip_read_editor_grid(self.ctx, rgba.ctypes.data, depth.ctypes.data, kept.ctypes.data), "read_editor_grid")
        return rgba, depth, kept.astype(bool)

    def ssao_defaults(self) -> AwsmSsao:
        s = AwsmSsao()
        self._chk(self.lib.awsm_hip_ssao_defaults(C.byref(s)), "ssao_defaults")
        return s

    def set_ssao(self, on=True, struct_size: Optional[int] = None, **overrides):
        """Screen-space ambient occlusion in every later opaque_pass: the defaults with `overrides` (radius, intensity, bias, strength);
        set_ssao(None) turns it off.  struct_size: what the record claims as its size (tests)."""
        if not on:
            return self._chk(self.lib.awsm_hip_set_ssao(self.ctx, None), "set_ssao")
        s = self.ssao_defaults().override(**overrides)
        if struct_size is not None:
            s.struct_size = struct_size
        self._chk(self.lib.awsm_hip_set_ssao(self.ctx, C.byref(s)), "set_ssao")

    def read_ssao(self):
        """The last submitted frame's layers -> (A before the smoothing, A' after it, view z; float32 [H, W] each, view z NaN where nothing was hit)."""
        raw, smoothed, view_z = (np.empty((self.height, self.width), np.float32) for _ in range(3))
        self._chk(self.lib.awsm_hip_read_ssao(self.ctx, raw.ctypes.data, smoothed.ctypes.data, view_z.ctypes.data), "read_ssao")
        return raw, smoothed, view_z

    def selection_defaults(self) -> AwsmSelection:
        s = AwsmSelection()
        self._chk(self.lib.awsm_hip_selection_defaults(C.byref(s)), "selection_defaults")
        return s

    def set_selection(self, mesh_keys=(), boxes=(), on=True, struct_size: Optional[int] = None, n_keys: Optional[int] = None, n_boxes: Optional[int] = None, **overrides):
        """The editor's selection overlay in every later transparent_pass: an outline around the visible pixels of the meshes `mesh_keys` (64-bit keys, or
        (high, low) pairs as pick() reports them) and a wire box around every box of `boxes` ((min xyz, max xyz) in world space), with the defaults and
        `overrides` (AwsmSelection's field names).  set_selection(on=None) turns it off.  struct_size, n_keys, n_boxes: what the call claims (tests)."""
        if not on:
            return self._chk(self.lib.awsm_hip_set_selection(self.ctx, None, None, 0, None, 0), "set_selection")
        s = self.selection_defaults().override(**overrides)
        if struct_size is not None:
            s.struct_size = struct_size
        keys = selection_key_words(mesh_keys)
        bx = np.ascontiguousarray(np.asarray(boxes, np.float32).reshape(-1, 6))
        self._chk(self.lib.awsm_hip_set_selection(self.ctx, C.byref(s), keys.ctypes.data if keys.size else None, len(keys) if n_keys is None else n_keys,
                                                  bx.ctypes.data if bx.size else None, len(bx) if n_boxes is None else n_boxes), "set_selection")
        self._selection_boxes = len(bx)

    def read_selection(self, n_boxes: Optional[int] = None):
        """The last submitted frame's selection layers -> (selected bool [H, W], ring bool [H, W], box alpha float32 [H, W], edges float32
        [n_boxes, 12, 8]: x0 y0 z0 x1 y1 z1 valid pad).  n_boxes: the count the frame's record holds; it may be left out when the selection was set
        through this object's set_selection."""
        nb = int(n_boxes if n_boxes is not None else getattr(self, "_selection_boxes", 0))
        selected, ring = np.empty((self.height, self.width), np.uint8), np.empty((self.height, self.width), np.uint8)
        alpha = np.empty((self.height, self.width), np.float32)
        edges = np.zeros((nb, 12, 8), np.float32)
        self._chk(self.lib.awsm_hip_read_selection(self.ctx, selected.ctypes.data, ring.ctypes.data, alpha.ctypes.data, edges.ctypes.data if nb else None), "read_selection")
        return selected.astype(bool), ring.astype(bool), alpha, edges

    def shadow_defaults(self) -> AwsmShadow:
        s = AwsmShadow()
        self._chk(self.lib.awsm_hip_shadow_defaults(C.byref(s)), "shadow_defaults")
        return s

    def shadow_pass(self, light_camera, casters, struct_size: Optional[int] = None, **overrides):
        """The shadow map of this frame, between geometry_pass and opaque_pass: `casters` (draws) rasterised from `light_camera` (512 bytes in the
        camera buffer's layout), with the defaults and `overrides` (map_size, pcf_radius, light, bias, slope_bias, max_slope, strength,
        facing_fade).  The frame's opaque pass then multiplies the shadow in.  struct_size: what the record claims as its size (tests)."""
        s = self.shadow_defaults().override(**overrides)
        if struct_size is not None:
            s.struct_size = struct_size
        block = np.frombuffer(bytes(light_camera), dtype=np.uint8)
        arr = self.make_draws(casters)
        self._chk(self.lib.awsm_hip_shadow_pass(self.ctx, C.byref(s), block.ctypes.data if block.size else None, block.size, arr, len(casters)), "shadow_pass")
        self._shadow_size = int(s.map_size)

    def shadow_pass_views(self, views, struct_size: Optional[int] = None, n_views: Optional[int] = None, **overrides):
        """The shadow maps of this frame from several views of one light, in shadow_pass's place: views = [(light_camera, casters), ...], 1 .. 6 of
        them, each a 512-byte block and the draws that cast in it (none is legal).  The frame's opaque pass resolves every pixel in the first view
        that holds it.  n_views: what the call claims as the count (tests)."""
        s = self.shadow_defaults().override(**overrides)
        if struct_size is not None:
            s.struct_size = struct_size
        views = list(views)
        arr = (AwsmShadowView * max(1, len(views)))()
        keep = []      # what the records point to
        for i, (light_camera, casters) in enumerate(views):
            block = np.frombuffer(bytes(light_camera), dtype=np.uint8)
            draws = self.make_draws(casters)
            keep.append((block, draws))
            arr[i] = AwsmShadowView(block.ctypes.data if block.size else None, block.size, C.cast(draws, C.c_void_p), len(casters))
        n = len(views) if n_views is None else n_views
        self._chk(self.lib.awsm_hip_shadow_pass_views(self.ctx, C.byref(s), arr if views else None, n), "shadow_pass_views")
        self._shadow_size = int(s.map_size)

    def read_shadow_map(self, size: Optional[int] = None, view: Optional[int] = None) -> np.ndarray:
        """The last submitted frame's shadow map -> (S, S) uint64 keys (no hit = all ones).  size: the map's S; it may be left out when the pass was
        made through this object's shadow_pass (a host's pass was not: give the size Host.set_shadow was given).  view: the layer of a pass of
        several views (shadow_pass_views); left out, layer 0 through awsm_hip_read_shadow_map."""
        if size is None and self._shadow_size is None:
            raise ValueError("read_shadow_map: no shadow_pass was made through this object; give the map's size")
        S = int(size if size is not None else self._shadow_size)
        keys = np.empty((S, S), np.uint64)
        if view is None:
            self._chk(self.lib.awsm_hip_read_shadow_map(self.ctx, keys.ctypes.data), "read_shadow_map")
        else:
            self._chk(self.lib.awsm_hip_read_shadow_map_view(self.ctx, int(view), keys.ctypes.data), "read_shadow_map_view")
        return keys

    def read_shadow_view(self) -> np.ndarray:
        """The last submitted frame's view layer -> uint8 [H, W]: the view each pixel was resolved in, 255 = none (shadow_pass_views only)."""
        view = np.empty((self.height, self.width), np.uint8)
        self._chk(self.lib.awsm_hip_read_shadow_view(self.ctx, view.ctypes.data), "read_shadow_view")
        return view

    def read_shadow(self):
        """The last submitted frame's layers -> (V, m), float32 [H, W] each: the light's visibility and the multiplier the opaque image received."""
        vis, mul = (np.empty((self.height, self.width), np.float32) for _ in range(2))
        self._chk(self.lib.awsm_hip_read_shadow(self.ctx, vis.ctypes.data, mul.ctypes.data), "read_shadow")
        return vis, mul

    def hud_geometry_pass(self, draws):
        """The hud meshes' visibility geometry, between geometry_pass and opaque_pass (render.rs:169-178)."""
        arr = self.make_draws(draws)
        self._chk(self.lib.awsm_hip_hud_geometry_pass(self.ctx, arr, len(draws)), "hud_geometry_pass")

    def hud_transparent_pass(self, draws):
        """The hud meshes' transparency geometry over the composite, after transparent_pass (render.rs:301-312)."""
        arr = self.make_draws(draws)
        self._chk(self.lib.awsm_hip_hud_transparent_pass(self.ctx, arr, len(draws)), "hud_transparent_pass")

    def frame_end(self) -> dict:
        st = AwsmFrameStats()
        st.struct_size = C.sizeof(AwsmFrameStats)
        self._chk(self.lib.awsm_hip_frame_end(self.ctx, C.byref(st)), "frame_end")
        return st.as_dict()

    def frame_flush(self):
        """Order everything enqueued so far (incl. overlapped opaque passes) before later work on the caller's stream."""
        self._chk(self.lib.awsm_hip_frame_flush(self.ctx), "frame_flush")

    def frame_trace(self, capacity: int):
        """Device-clock stamps per frame (geometry begins / geometry done / shading done) in a ring of `capacity` frames; 0 = off."""
        self._chk(self.lib.awsm_hip_frame_trace(self.ctx, capacity), "frame_trace")

    def read_frame_trace(self, n_frames: int):
        """-> (ms[n_frames, 3] relative to the first stamp of the oldest frame, serial of the newest frame); synchronises."""
        ticks = np.zeros((n_frames, 3), dtype=np.uint64)
        serial, rate = C.c_uint32(), C.c_uint32()
        self._chk(self.lib.awsm_hip_read_frame_trace(self.ctx, ticks.ctypes.data_as(C.c_void_p), n_frames, C.byref(serial), C.byref(rate)), "read_frame_trace")
        t0 = int(ticks[ticks > 0].min()) if (ticks > 0).any() else 0
        return (ticks.astype(np.int64) - t0) / float(rate.value), int(serial.value)

    def bind_output(self, device_ptr: Optional[int], nbytes: int = 0):
        self._chk(self.lib.awsm_hip_bind_output(self.ctx, device_ptr, nbytes), "bind_output")

    def msaa_halo_bands(self) -> int:
        return int(self.lib.awsm_hip_msaa_halo_bands(self.ctx))

    def msaa_halo_export(self, device_ptr: int, nbytes: int):
        """MSAA + bands: this rank's [bands][2][width] u64 boundary keys into device memory (to be all-gathered)."""
        self._chk(self.lib.awsm_hip_msaa_halo_export(self.ctx, device_ptr, nbytes), "msaa_halo_export")

    def msaa_halo_bind(self, device_ptr: Optional[int], nbytes: int = 0):
        """The gathered [n][bands][2][width] u64 array the next opaque pass reads its neighbours' rows from."""
        self._chk(self.lib.awsm_hip_msaa_halo_bind(self.ctx, device_ptr, nbytes), "msaa_halo_bind")

    def bind_opaque_source(self, device_ptr: Optional[int], nbytes: int = 0):
        """Sharded transparent pass: the gathered full-frame opaque image (None = the context's own output)."""
        self._chk(self.lib.awsm_hip_bind_opaque_source(self.ctx, device_ptr, nbytes), "bind_opaque_source")

    def bind_output_rows(self, device_ptr: int, nbytes: int, first_row: int):
        """Row-strip shards: device_ptr receives frame row first_row onwards."""
        self._chk(self.lib.awsm_hip_bind_output_rows(self.ctx, device_ptr, nbytes, first_row), "bind_output_rows")

    def output_device_ptr(self) -> int:
        return self.lib.awsm_hip_output_device_ptr(self.ctx)

    # ---- readback ----
    def _vis_shape(self):
        return (self.height, self.width, 4) if getattr(self, "msaa", 0) == 4 else (self.height, self.width)

    def stream_handoff(self) -> int:
        """1: the overlapped pipeline hands frames between its streams through device-side flags, 0: through hipEvents (awsm_hip.h)."""
        self.lib.awsm_hip_stream_handoff.argtypes = [C.c_void_p]
        return int(self.lib.awsm_hip_stream_handoff(self.ctx))

    def read_gbuffer(self) -> np.ndarray:
        """(height, width, 6) f32: the reconstructed G-buffer texel per pixel (packed normal / tangent, barycentric), zeros where nothing was hit."""
        out = np.zeros((self.height, self.width, 6), dtype=np.float32)
        self.lib.awsm_hip_read_gbuffer.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.lib.awsm_hip_read_gbuffer(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_gbuffer")
        return out

    def read_visibility(self) -> np.ndarray:
        """Packed keys [H, W] (with MSAA x4: [H, W, 4], sample-minor)."""
        out = np.zeros(self._vis_shape(), dtype=np.uint64)
        self._chk(self.lib.awsm_hip_read_visibility(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_visibility")
        return out

    def visibility_digest(self):
        """(sum key_i * (2 i + 1) mod 2^64, xor rotl(key_i, i mod 64)) of the last geometry pass's keys, computed on the device."""
        out = np.zeros(2, dtype=np.uint64)
        self._chk(self.lib.awsm_hip_visibility_digest(self.ctx, out.ctypes.data_as(C.c_void_p)), "visibility_digest")
        return int(out[0]), int(out[1])

    def read_visibility_unpacked(self):
        tri = np.zeros(self._vis_shape(), dtype=np.uint32)
        meta = np.zeros(self._vis_shape(), dtype=np.uint32)
        depth = np.zeros(self._vis_shape(), dtype=np.float32)
        self._chk(self.lib.awsm_hip_read_visibility_unpacked(self.ctx, tri.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p),
                                                             depth.ctypes.data_as(C.c_void_p)), "read_visibility_unpacked")
        return tri, meta, depth

    def read_opaque(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint16)
        self._chk(self.lib.awsm_hip_read_opaque(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_opaque")
        return out

    def read_opaque_f32(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.awsm_hip_read_opaque_f32(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_opaque_f32")
        return out

    def read_composite(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint16)
        self._chk(self.lib.awsm_hip_read_composite(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_composite")
        return out

    def read_composite_f32(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.awsm_hip_read_composite_f32(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_composite_f32")
        return out

    def bind_composite(self, device_ptr: Optional[int], nbytes: int = 0):
        self._chk(self.lib.awsm_hip_bind_composite(self.ctx, device_ptr, nbytes), "bind_composite")

    # ---- effects + display passes (awsm_hip_post_pass) ----
    def post_pass(self, tonemapping: int = 1, smaa: bool = False, bloom: bool = False, dof: bool = False, struct_size: Optional[int] = None):
        """Effects pass + display pass of the current frame (after opaque_pass / transparent_pass, before the next geometry_pass)."""
        flags = (AWSM_POST_SMAA if smaa else 0) | (AWSM_POST_BLOOM if bloom else 0) | (AWSM_POST_DOF if dof else 0)
        p = AwsmPostParams(C.sizeof(AwsmPostParams) if struct_size is None else struct_size, tonemapping, flags, 0)
        self._chk(self.lib.awsm_hip_post_pass(self.ctx, C.byref(p)), "post_pass")

    def taa_defaults(self) -> AwsmTaa:
        t = AwsmTaa()
        self._chk(self.lib.awsm_hip_taa_defaults(C.byref(t)), "taa_defaults")
        return t

    def set_taa(self, on=True, struct_size: Optional[int] = None, **overrides):
        """Temporal anti-aliasing in every later post_pass: the defaults with `overrides` (feedback, flags, jitter_ndc, reproject — column-major,
        16 values); set_taa(None) turns it off and drops the history.  struct_size: what the record claims as its size (tests)."""
        if not on:
            return self._chk(self.lib.awsm_hip_set_taa(self.ctx, None), "set_taa")
        t = self.taa_defaults().override(**overrides)
        if struct_size is not None:
            t.struct_size = struct_size
        self._chk(self.lib.awsm_hip_set_taa(self.ctx, C.byref(t)), "set_taa")

    def read_taa(self, layers: bool = True):
        """Of the last post pass -> (the resolved image, uint16 [H, W, 4] f16 bits; the history position (sx, sy) per pixel in texel-index
        units, float32 [H, W, 2]; whether the history was used, bool [H, W]).  layers=False: the image alone (the layers cost a kernel)."""
        resolved = np.zeros((self.height, self.width, 4), dtype=np.uint16)
        if not layers:
            self._chk(self.lib.awsm_hip_read_taa(self.ctx, resolved.ctypes.data, None, None), "read_taa")
            return resolved
        xy = np.zeros((self.height, self.width, 2), dtype=np.float32)
        used = np.zeros((self.height, self.width), dtype=np.uint8)
        self._chk(self.lib.awsm_hip_read_taa(self.ctx, resolved.ctypes.data, xy.ctypes.data, used.ctypes.data), "read_taa")
        return resolved, xy, used.astype(bool)

    def read_display(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self.lib.awsm_hip_read_display(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_display")
        return out

    def read_effects(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint16)
        self._chk(self.lib.awsm_hip_read_effects(self.ctx, out.ctypes.data_as(C.c_void_p)), "read_effects")
        return out

    def bind_display(self, device_ptr: Optional[int], nbytes: int = 0):
        self._chk(self.lib.awsm_hip_bind_display(self.ctx, device_ptr, nbytes), "bind_display")

    def display_device_ptr(self) -> Optional[int]:
        return self.lib.awsm_hip_display_device_ptr(self.ctx)

    def read_transformed_forward(self, n_vertices: int):
        clip = np.zeros((max(1, n_vertices), 4), dtype=np.float32)
        nt = np.zeros((max(1, n_vertices), 8), dtype=np.float32)
        wpos = np.zeros((max(1, n_vertices), 4), dtype=np.float32)
        self._chk(self.lib.awsm_hip_read_transformed_forward(self.ctx, clip.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p),
                                                             wpos.ctypes.data_as(C.c_void_p), n_vertices), "read_transformed_forward")
        return clip, nt, wpos

    def read_transformed(self, n_vertices: int):
        clip = np.zeros((max(1, n_vertices), 4), dtype=np.float32)
        nt = np.zeros((max(1, n_vertices), 8), dtype=np.float32)
        self._chk(self.lib.awsm_hip_read_transformed(self.ctx, clip.ctypes.data_as(C.c_void_p), nt.ctypes.data_as(C.c_void_p), n_vertices), "read_transformed")
        return clip, nt

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus, mem = C.c_uint32(), C.c_uint64()
        self._chk(self.lib.awsm_hip_device_info(self.ctx, name, 256, C.byref(cus), C.byref(mem)), "device_info")
        return {"name": name.value.decode(), "cu_count": cus.value, "hbm_bytes": mem.value}
