"""
host.py — ctypes binding of libawsm_host.so (include/awsm_host.h) and `populate()`, which feeds a SceneDesc through
the key-based API in the order the reference's populate_gltf does (crates/renderer/src/gltf/populate.rs:185-205:
node transforms -> skins -> meshes, and per primitive morph -> skin -> material -> mesh, populate/mesh.rs:89-311).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np

from . import PACKAGE_DIR, hip_backend
from .hip_backend import AwsmDraw, AwsmEnv, AwsmFrameStats, AwsmSampler
from .scene_desc import MaterialDesc, SceneDesc, TextureRef, texture_mip_kinds

LIB_PATH = os.environ.get("AWSM_HOST_LIB") or os.path.join(PACKAGE_DIR, "libawsm_host.so")   # AWSM_HOST_LIB: instrumented builds of the same ABI (tests)
F32P = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)


class TexRef(C.Structure):
    _fields_ = [("texture", C.c_int32), ("sampler", C.c_uint32), ("uv_index", C.c_uint32), ("pad", C.c_uint32), ("transform", C.c_uint64)]


class HostMaterial(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("shader", C.c_uint32), ("double_sided", C.c_uint32), ("base_color_factor", C.c_float * 4), ("metallic_factor", C.c_float),
                ("roughness_factor", C.c_float), ("normal_scale", C.c_float), ("occlusion_strength", C.c_float), ("emissive_factor", C.c_float * 3),
                ("debug_bitmask", C.c_uint32), ("base_color_tex", TexRef), ("metallic_roughness_tex", TexRef), ("normal_tex", TexRef),
                ("occlusion_tex", TexRef), ("emissive_tex", TexRef),
                ("has_vertex_color", C.c_uint32), ("vertex_color_set", C.c_uint32), ("has_emissive_strength", C.c_uint32), ("emissive_strength", C.c_float),
                ("has_ior", C.c_uint32), ("ior", C.c_float),
                ("has_specular", C.c_uint32), ("specular_factor", C.c_float), ("specular_color_factor", C.c_float * 3), ("specular_tex", TexRef), ("specular_color_tex", TexRef),
                ("has_transmission", C.c_uint32), ("transmission_factor", C.c_float), ("transmission_tex", TexRef),
                ("has_volume", C.c_uint32), ("volume_thickness_factor", C.c_float), ("volume_attenuation_distance", C.c_float),
                ("volume_attenuation_color", C.c_float * 3), ("volume_thickness_tex", TexRef),
                ("has_clearcoat", C.c_uint32), ("clearcoat_factor", C.c_float), ("clearcoat_roughness_factor", C.c_float), ("clearcoat_normal_scale", C.c_float),
                ("clearcoat_tex", TexRef), ("clearcoat_roughness_tex", TexRef), ("clearcoat_normal_tex", TexRef),
                ("has_sheen", C.c_uint32), ("sheen_roughness_factor", C.c_float), ("sheen_color_factor", C.c_float * 3), ("sheen_roughness_tex", TexRef), ("sheen_color_tex", TexRef),
                ("alpha_mode", C.c_uint32), ("alpha_cutoff", C.c_float),
                ("has_diffuse_transmission", C.c_uint32), ("diffuse_transmission_factor", C.c_float), ("diffuse_transmission_color_factor", C.c_float * 3),
                ("diffuse_transmission_tex", TexRef), ("diffuse_transmission_color_tex", TexRef),
                ("has_dispersion", C.c_uint32), ("dispersion", C.c_float),
                ("has_anisotropy", C.c_uint32), ("anisotropy_strength", C.c_float), ("anisotropy_rotation", C.c_float), ("anisotropy_tex", TexRef),
                ("has_iridescence", C.c_uint32), ("iridescence_factor", C.c_float), ("iridescence_ior", C.c_float), ("iridescence_thickness_min", C.c_float),
                ("iridescence_thickness_max", C.c_float), ("iridescence_tex", TexRef), ("iridescence_thickness_tex", TexRef)]


class HostTextureDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mipmap_kind", C.c_uint32), ("srgb_to_linear", C.c_uint32), ("premultiply_alpha", C.c_uint32)]


class GltfOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("scene_index", C.c_int32), ("flags", C.c_uint32)]


AWSM_GLTF_SRGB_COLOR_TEXTURES = 1


class MorphTarget(C.Structure):
    _fields_ = [("positions", F32P), ("normals", F32P), ("tangents", F32P)]


class HostPrimitive(C.Structure):
    _fields_ = [("vertex_count", C.c_uint32), ("triangle_count", C.c_uint32), ("positions", F32P), ("normals", F32P), ("tangents", F32P),
                ("indices", U32P), ("n_uv_sets", C.c_uint32), ("uv_sets", F32P * 8), ("n_color_sets", C.c_uint32), ("color_sets", F32P * 4),
                ("n_morph_targets", C.c_uint32), ("morph_targets", C.POINTER(MorphTarget)), ("morph_weights", F32P), ("animated_morph_weights", F32P),
                ("front_face_cw", C.c_uint32)]


class HostLight(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("color", C.c_float * 3), ("intensity", C.c_float), ("position", C.c_float * 3), ("range", C.c_float),
                ("direction", C.c_float * 3), ("inner_angle", C.c_float), ("outer_angle", C.c_float)]


class HostShadow(C.Structure):
    """AwsmHostShadow (awsm_host_set_shadow): the light's key and hip_backend.AwsmShadow's parameters."""
    _fields_ = [("struct_size", C.c_uint32), ("light", C.c_uint64), ("map_size", C.c_uint32), ("pcf_radius", C.c_uint32), ("bias", C.c_float),
                ("slope_bias", C.c_float), ("max_slope", C.c_float), ("strength", C.c_float), ("facing_fade", C.c_float)]

    def override(self, **overrides):
        """Set fields by name; an unknown name is a TypeError."""
        names = dict(self._fields_)
        for k, v in overrides.items():
            if k not in names or k in ("struct_size", "light"):
                raise TypeError("AwsmHostShadow has no field %r (fields: %s)" % (k, ", ".join(n for n, _ in self._fields_[2:])))
            setattr(self, k, int(v) if k in ("map_size", "pcf_radius") else float(v))
        return self


class HostShadowCascades(C.Structure):
    """AwsmHostShadowCascades (awsm_host_set_shadow_cascades): how many nested windows a shadowed directional light gets along the camera's depth, the
    blend of the logarithmic and the uniform split, and the depth the last one ends at (0: the camera's far)."""
    _fields_ = [("struct_size", C.c_uint32), ("count", C.c_uint32), ("lambda_", C.c_float), ("max_distance", C.c_float)]


class HostTaa(C.Structure):
    """AwsmHostTaa (awsm_host_set_taa): the weight of the current frame and the jitter amplitudes for a still and a moving camera."""
    _fields_ = [("struct_size", C.c_uint32), ("feedback", C.c_float), ("strength_still", C.c_float), ("strength_moving", C.c_float)]


class AnimationClip(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_uint32), ("interpolation", C.c_uint32), ("n_keys", C.c_uint32), ("width", C.c_uint32),
                ("times", C.POINTER(C.c_double)), ("values", F32P), ("in_tangents", F32P), ("out_tangents", F32P), ("duration", C.c_double)]


class AnimationState(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("direction", C.c_int32), ("state", C.c_int32), ("loop_style", C.c_int32),
                ("local_time", C.c_double), ("duration", C.c_double), ("speed", C.c_double)]


ANIM_PATHS = {"translation": 0, "rotation": 1, "scale": 2, "weights": 3}
ANIM_INTERPOLATIONS = {"linear": 0, "step": 1, "cubic": 2}
ANIM_LOOP_NONE, ANIM_LOOP, ANIM_PING_PONG = -1, 0, 1
ANIM_FORWARD, ANIM_BACKWARD = 0, 1
ANIM_PLAYING, ANIM_PAUSED, ANIM_ENDED = 0, 1, 2

_lib = None


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not found: run __graft_entry__.build()")
    lib = C.CDLL(LIB_PATH)
    u64, vp, i64, sz = C.c_uint64, C.c_void_p, C.c_int64, C.c_size_t
    sig = {
        "awsm_host_create": (C.c_int, [C.c_char_p, C.c_int, vp, C.c_uint32, C.POINTER(vp)]),
        "awsm_host_destroy": (C.c_int, [vp]), "awsm_host_last_error": (C.c_char_p, [vp]), "awsm_host_device_ctx": (vp, [vp]),
        "awsm_host_transform_root": (u64, [vp]), "awsm_host_transform_insert": (u64, [vp, F32P, F32P, F32P, u64]),
        "awsm_host_transform_set_local": (C.c_int, [vp, u64, F32P, F32P, F32P]), "awsm_host_transform_set_parent": (C.c_int, [vp, u64, u64]),
        "awsm_host_transform_remove": (C.c_int, [vp, u64]), "awsm_host_transform_parent": (u64, [vp, u64]),
        "awsm_host_transform_world": (C.c_int, [vp, u64, F32P]),
        "awsm_host_texture_insert": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32]), "awsm_host_sampler_insert": (C.c_int, [vp, vp]),
        "awsm_host_texture_transform_insert": (u64, [vp, F32P, F32P, C.c_float, F32P]),
        "awsm_host_material_insert": (u64, [vp, vp]), "awsm_host_material_update": (C.c_int, [vp, u64, vp]), "awsm_host_material_offset": (i64, [vp, u64]),
        "awsm_host_skin_insert": (u64, [vp, C.POINTER(u64), C.c_uint32, F32P, C.c_uint32, C.POINTER(U32P), C.POINTER(F32P), C.c_uint32]),
        "awsm_host_mesh_insert": (u64, [vp, vp, u64, u64, u64, C.c_uint32]), "awsm_host_mesh_insert_hud": (u64, [vp, vp, u64, u64, u64, C.c_uint32]),
        "awsm_host_hud_draw_lists": (C.c_int, [vp, vp, vp, C.c_uint32, U32P]), "awsm_host_mesh_remove": (C.c_int, [vp, u64]),
        "awsm_host_light_insert": (u64, [vp, vp]), "awsm_host_light_remove": (C.c_int, [vp, u64]),
        "awsm_host_set_ibl_mip_counts": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "awsm_host_camera_update": (C.c_int, [vp, F32P, F32P, F32P]), "awsm_host_env": (C.c_int, [vp, vp]),
        "awsm_host_env_cube": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, vp]),
        "awsm_host_env_cube_create": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
        "awsm_host_env_cube_update_face": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, sz, vp]),
        "awsm_host_env_cube_update_all_faces": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, vp, sz, vp]),
        "awsm_host_env_cube_regenerate_mipmaps": (C.c_int, [vp, C.c_int]),
        "awsm_host_env_cube_colors": (C.c_int, [vp, C.c_int, C.c_uint32, vp]),
        "awsm_host_env_cube_sky_gradient": (C.c_int, [vp, C.c_int, C.c_uint32, vp, vp]),
        "awsm_host_env_bake_ibl": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "awsm_host_ktx2_parse": (C.c_int, [vp, sz, vp, C.c_char_p, sz]),
        "awsm_host_env_cube_load_ktx2": (C.c_int, [vp, C.c_int, C.c_char_p, vp, C.c_char_p, sz]),
        "awsm_host_env_cube_load_ktx2_memory": (C.c_int, [vp, C.c_int, vp, sz, vp, C.c_char_p, sz]),
        "awsm_host_hdr_info": (C.c_int, [vp, sz, vp, C.c_char_p, sz]), "awsm_host_hdr_decode": (C.c_int, [vp, sz, vp, sz, vp, C.c_char_p, sz]),
        "awsm_host_env_cube_from_equirect": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "awsm_host_env_cube_load_hdr": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp, C.c_char_p, sz]),
        "awsm_host_env_cube_load_hdr_memory": (C.c_int, [vp, C.c_int, vp, sz, C.c_uint32, C.c_uint32, C.c_float, C.c_float, vp, C.c_char_p, sz]),
        "awsm_host_set_render_hooks": (C.c_int, [vp, vp, vp, vp, vp]),
        "awsm_host_brdf_lut_generate": (C.c_int, [vp, C.c_uint32, C.c_uint32]), "awsm_host_resize": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "awsm_host_set_shard_rows": (C.c_int, [vp, C.c_uint32, C.c_uint32]), "awsm_host_set_shard_bands": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32]), "awsm_host_set_render_timings": (C.c_int, [vp, C.c_int]),
        "awsm_host_pick": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
        "awsm_host_pick_ex": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int, C.c_float, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "awsm_host_pick_rect": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int, C.c_float, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]),
        "awsm_host_set_anti_aliasing": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "awsm_host_set_post_processing": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_int, C.c_int]),
        "awsm_host_clear_post_processing": (C.c_int, [vp]),
        "awsm_host_camera_set_dof": (C.c_int, [vp, C.c_float, C.c_float]),
        "awsm_host_editor_grid_defaults": (C.c_int, [vp, vp]), "awsm_host_set_editor_grid": (C.c_int, [vp, vp]),
        "awsm_host_selection_defaults": (C.c_int, [vp, vp]), "awsm_host_set_selection": (C.c_int, [vp, vp, vp, C.c_uint32]),
        "awsm_host_ssao_defaults": (C.c_int, [vp, vp]), "awsm_host_set_ssao": (C.c_int, [vp, vp]),
        "awsm_host_set_taa": (C.c_int, [vp, vp]), "awsm_host_taa_jitter": (C.c_int, [vp, C.c_uint32, C.c_int, F32P]),
        "awsm_host_shadow_defaults": (C.c_int, [vp, vp]), "awsm_host_set_shadow": (C.c_int, [vp, vp]),
        "awsm_host_shadow_camera": (C.c_int, [vp, vp, vp, C.c_uint32, vp]),
        "awsm_host_shadow_cascades_defaults": (C.c_int, [vp]), "awsm_host_set_shadow_cascades": (C.c_int, [vp, vp]),
        "awsm_host_shadow_view_count": (C.c_int, [vp, vp]), "awsm_host_shadow_view": (C.c_int, [vp, C.c_uint32, vp, vp, C.c_uint32, vp]),
        "awsm_host_mesh_set_instances": (C.c_int, [vp, u64, F32P, C.c_uint32]), "awsm_host_mesh_append_instances": (C.c_int, [vp, u64, F32P, C.c_uint32]),
        "awsm_host_texture_insert_kind": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32]), "awsm_host_update_transforms": (C.c_int, [vp]),
        "awsm_host_render": (C.c_int, [vp, C.c_int, vp]), "awsm_host_mirror": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "awsm_host_load_gltf": (C.c_int, [vp, C.c_char_p, C.c_int, vp, C.c_char_p, C.c_size_t]),
        "awsm_host_decode_image": (C.c_int, [C.c_char_p, C.c_size_t, vp, C.c_size_t, U32P, U32P, C.c_char_p, C.c_size_t]),
        "awsm_host_draw_list": (C.c_int, [vp, vp, C.c_uint32, U32P]), "awsm_host_transparent_draw_list": (C.c_int, [vp, vp, C.c_uint32, U32P]), "awsm_host_texture_array_count": (C.c_uint32, [vp]),
        "awsm_host_texture_array_info": (C.c_int, [vp, C.c_uint32, U32P, U32P, U32P, C.POINTER(vp)]),
        "awsm_host_texture_insert_ex": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp]), "awsm_host_texture_update": (C.c_int, [vp, C.c_int, vp]),
        "awsm_host_load_gltf_ex": (C.c_int, [vp, C.c_char_p, vp, vp, C.c_char_p, C.c_size_t]),
        "awsm_host_upload_bytes_last_frame": (u64, [vp]),
        "awsm_host_transform_get_local": (C.c_int, [vp, u64, F32P, F32P, F32P]), "awsm_host_transform_duplicate": (u64, [vp, u64]),
        "awsm_host_mesh_update_morph_weights": (C.c_int, [vp, u64, F32P, C.c_uint32]), "awsm_host_light_update": (C.c_int, [vp, u64, vp]),
        "awsm_host_animation_insert_transform": (u64, [vp, vp, u64]), "awsm_host_animation_insert_morph": (u64, [vp, vp, u64]),
        "awsm_host_animation_remove": (C.c_int, [vp, u64]),
        "awsm_host_animation_set_playback": (C.c_int, [vp, u64, C.c_double, C.c_int, C.c_int, C.c_int]),
        "awsm_host_animation_seek": (C.c_int, [vp, u64, C.c_double]), "awsm_host_animation_state": (C.c_int, [vp, u64, vp]),
        "awsm_host_animation_sample": (C.c_int, [vp, u64, F32P, C.c_uint32]), "awsm_host_update_animations": (C.c_int, [vp, C.c_double]),
        "awsm_host_skin_matrices_offset": (i64, [vp, u64]),
        "awsm_host_gltf_animation_keys": (C.c_int, [vp, C.POINTER(u64), C.c_uint32, U32P]),
        "awsm_host_set_device_skin_posing": (C.c_int, [vp, C.c_int]), "awsm_host_skin_pose_ids_last_frame": (C.c_int, [vp, U32P, C.c_uint32, U32P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def _f(arr):
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return a, a.ctypes.data_as(F32P)


class HostError(RuntimeError):
    code = None      # the AwsmStatus, where the failure came with one


class Ktx2Level(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64)]


class Ktx2Info(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("vk_format", C.c_uint32), ("format", C.c_uint32), ("size", C.c_uint32), ("faces", C.c_uint32),
                ("layers", C.c_uint32), ("levels", C.c_uint32), ("mips", C.c_uint32), ("level", Ktx2Level * 16)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("vk_format", "format", "size", "faces", "layers", "levels", "mips")}
        d["format_name"] = hip_backend.CUBE_FORMAT_NAMES.get(d["format"])
        d["level"] = [(int(self.level[i].offset), int(self.level[i].length)) for i in range(d["levels"])]
        return d


class HdrInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("flipped_y", C.c_uint32), ("rle", C.c_uint32), ("exposure", C.c_float)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("width", "height", "flipped_y", "rle")}
        d["exposure"] = float(self.exposure)
        return d


def _hdr_error(where: str, rc: int, err) -> "HostError":
    e = HostError(f"{where} failed ({rc}): {err.value.decode(errors='replace')}")
    e.code = rc
    return e


def hdr_info(data: bytes) -> dict:
    """awsm_host_hdr_info: the header of a Radiance .hdr picture (no host, no device); raises HostError with the reason."""
    info = HdrInfo(struct_size=C.sizeof(HdrInfo))
    err = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    rc = load_library().awsm_host_hdr_info(buf, len(data), C.byref(info), err, 512)
    if rc != 0:
        raise _hdr_error("hdr_info", rc, err)
    return info.as_dict()


def hdr_decode(data: bytes, out_cap: Optional[int] = None):
    """awsm_host_hdr_decode: -> (uint8 [H, W, 4] RGBE, top-down; the header dict).  out_cap: the size of the output buffer handed to the reader
    (default: what the header asks for)."""
    head = hdr_info(data)
    need = head["width"] * head["height"] * 4
    out = np.zeros(need if out_cap is None else out_cap, dtype=np.uint8)
    info = HdrInfo(struct_size=C.sizeof(HdrInfo))
    err = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    rc = load_library().awsm_host_hdr_decode(buf, len(data), out.ctypes.data if out.size else None, out.size, C.byref(info), err, 512)
    if rc != 0:
        raise _hdr_error("hdr_decode", rc, err)
    return out[:need].reshape(head["height"], head["width"], 4), info.as_dict()


def ktx2_parse(data: bytes) -> dict:
    """awsm_host_ktx2_parse: the header and level index of a KTX2 cube map (no host, no device); raises HostError with the reason."""
    info = Ktx2Info(struct_size=C.sizeof(Ktx2Info))
    err = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) or b"\0")
    rc = load_library().awsm_host_ktx2_parse(buf, len(data), C.byref(info), err, 512)
    if rc != 0:
        e = HostError(f"ktx2_parse failed ({rc}): {err.value.decode(errors='replace')}")
        e.code = rc
        raise e
    return info.as_dict()


class Host:
    """One AwsmHost: scene state + a device context reached through the awsm_hip_* C-ABI of `backend_path`."""

    def __init__(self, backend_path: Optional[str] = None, device: int = 0, stream: Optional[int] = None, parity_tap: bool = False, overlap_frames: bool = False,
                 anisotropic: bool = False):
        self.lib = load_library()
        backend_path = backend_path or hip_backend.LIB_PATH
        if not os.path.exists(backend_path):
            raise FileNotFoundError(f"backend library {backend_path} not found (no CPU fallback exists for the product path)")
        h = C.c_void_p()
        flags = (hip_backend.AWSM_CFG_PARITY_TAP if parity_tap else 0) | (hip_backend.AWSM_CFG_OVERLAP_FRAMES if overlap_frames else 0) | (hip_backend.AWSM_CFG_ANISOTROPIC if anisotropic else 0)
        rc = self.lib.awsm_host_create(backend_path.encode(), device, stream, flags, C.byref(h))
        if rc != 0:
            raise HostError(f"awsm_host_create({backend_path}) failed with status {rc}")
        self.h = h
        self.width = self.height = 0

    def _chk(self, rc, where):
        if rc != 0:
            e = HostError(f"{where} failed ({rc}): {(self.lib.awsm_host_last_error(self.h) or b'').decode()}")
            e.code = rc
            raise e

    def close(self):
        if getattr(self, "h", None):
            self.lib.awsm_host_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_ctx(self) -> int:
        return self.lib.awsm_host_device_ctx(self.h)

    # ---- transforms ----
    def transform_insert(self, t, r, s, parent=0) -> int:
        (_, pt), (_, pr), (_, ps) = _f(t), _f(r), _f(s)
        k1, k2, k3 = _f(t), _f(r), _f(s)
        return self.lib.awsm_host_transform_insert(self.h, k1[1], k2[1], k3[1], parent)

    def transform_set_local(self, key, t, r, s):
        k1, k2, k3 = _f(t), _f(r), _f(s)
        self._chk(self.lib.awsm_host_transform_set_local(self.h, key, k1[1], k2[1], k3[1]), "transform_set_local")

    def transform_get_local(self, key):
        """Transforms::get_local: (translation, rotation xyzw, scale) as float32 arrays."""
        t, r, s = np.zeros(3, np.float32), np.zeros(4, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.awsm_host_transform_get_local(self.h, key, t.ctypes.data_as(F32P), r.ctypes.data_as(F32P), s.ctypes.data_as(F32P)), "transform_get_local")
        return t, r, s

    def transform_duplicate(self, key) -> int:
        """Transforms::duplicate: a new node with the same local transform under the same parent."""
        k = self.lib.awsm_host_transform_duplicate(self.h, key)
        if not k:
            self._chk(-1, "transform_duplicate")
        return k

    def transform_parent(self, key) -> int:
        return self.lib.awsm_host_transform_parent(self.h, key)

    def transform_world(self, key) -> np.ndarray:
        out = np.zeros(16, dtype=np.float32)
        self._chk(self.lib.awsm_host_transform_world(self.h, key, out.ctypes.data_as(F32P)), "transform_world")
        return out.reshape(4, 4)

    # ---- textures / samplers ----
    def texture_insert(self, image: np.ndarray, mip_kind: int = 0, srgb: bool = False, premultiply: bool = False) -> int:
        """An (h, w, 4) uint8 image into the pool; srgb / premultiply: converted on the device as it enters (awsm_host_texture_insert_ex)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if srgb or premultiply:
            desc = HostTextureDesc(C.sizeof(HostTextureDesc), mip_kind, 1 if srgb else 0, 1 if premultiply else 0)
            r = self.lib.awsm_host_texture_insert_ex(self.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], C.byref(desc))
        else:
            r = self.lib.awsm_host_texture_insert_kind(self.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], mip_kind)
        if r < 0:
            self._chk(r, "texture_insert")
        return r

    def texture_update(self, texture_id: int, image: np.ndarray):
        """New pixels (same extent) for a texture of the pool; the next frame submitted sees them."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        self._chk(self.lib.awsm_host_texture_update(self.h, texture_id, img.ctypes.data_as(C.c_void_p)), "texture_update")

    def sampler_insert(self, s: dict) -> int:
        smp = AwsmSampler(s.get("address_mode_u", 1), s.get("address_mode_v", 1), s.get("mag_filter", 1), s.get("min_filter", 1),
                          s.get("mipmap_filter", 1), s.get("max_anisotropy", 1))
        r = self.lib.awsm_host_sampler_insert(self.h, C.byref(smp))
        if r < 0:
            self._chk(r, "sampler_insert")
        return r

    def texture_transform_insert(self, offset=(0, 0), origin=(0, 0), rotation=0.0, scale=(1, 1)) -> int:
        a, b, c = _f(offset), _f(origin), _f(scale)
        return self.lib.awsm_host_texture_transform_insert(self.h, a[1], b[1], float(rotation), c[1])

    # ---- materials ----
    def material_insert(self, m: HostMaterial) -> int:
        k = self.lib.awsm_host_material_insert(self.h, C.byref(m))
        if not k:
            self._chk(-1, "material_insert")
        return k

    def material_update(self, key: int, m: HostMaterial):
        self._chk(self.lib.awsm_host_material_update(self.h, key, C.byref(m)), "material_update")

    # ---- skins / meshes ----
    def skin_insert(self, joint_keys: List[int], inverse_bind: np.ndarray, joints: List[np.ndarray], weights: List[np.ndarray]) -> int:
        n = len(joint_keys)
        keys = (C.c_uint64 * n)(*joint_keys)
        ib = _f(inverse_bind)
        js = [np.ascontiguousarray(j, dtype=np.uint32) for j in joints]
        ws = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        jp = (U32P * len(js))(*[j.ctypes.data_as(U32P) for j in js])
        wp = (F32P * len(ws))(*[w.ctypes.data_as(F32P) for w in ws])
        k = self.lib.awsm_host_skin_insert(self.h, keys, n, ib[1], len(js), jp, wp, js[0].shape[0])
        if not k:
            self._chk(-1, "skin_insert")
        return k

    def skin_matrices_offset(self, key: int) -> int:
        """Byte offset of the skin's first matrix in AWSM_BUF_SKIN_MATRICES (-1: no such skin)."""
        return self.lib.awsm_host_skin_matrices_offset(self.h, key)

    def hud_draw_lists(self):
        """(HUD geometry pass draws, HUD transparent pass draws): the hud meshes, back to front (render.rs:169-178,301-312)."""
        n = C.c_uint32()
        self._chk(self.lib.awsm_host_hud_draw_lists(self.h, None, None, 0, C.byref(n)), "hud_draw_lists")
        g, t = (AwsmDraw * max(1, n.value))(), (AwsmDraw * max(1, n.value))()
        self._chk(self.lib.awsm_host_hud_draw_lists(self.h, g, t, n.value, C.byref(n)), "hud_draw_lists")
        conv = lambda arr: [{"geom_meta_off": d.geom_meta_off, "vis_data_off": d.vis_data_off, "tri_count": d.tri_count, "flags": d.flags,
                             **({"inst_off": d.inst_off, "inst_count": d.inst_count} if d.inst_count else {})} for d in arr[: n.value]]     # noqa: E731
        return conv(g), conv(t)

    def mesh_insert(self, p, transform: int, material: int, skin: int = 0, hidden: bool = False, front_face_cw: bool = False) -> int:
        keep = []

        def fp(a):
            if a is None:
                return None
            arr = np.ascontiguousarray(a, dtype=np.float32)
            keep.append(arr)
            return arr.ctypes.data_as(F32P)

        hp = HostPrimitive()
        idx = np.ascontiguousarray(p.indices, dtype=np.uint32).reshape(-1, 3)
        keep.append(idx)
        hp.vertex_count, hp.triangle_count = p.positions.shape[0], idx.shape[0]
        hp.positions, hp.normals, hp.tangents = fp(p.positions), fp(p.normals), fp(p.tangents)
        hp.indices = idx.ctypes.data_as(U32P)
        hp.n_uv_sets = len(p.uvs)
        for i, u in enumerate(p.uvs):
            hp.uv_sets[i] = fp(u)
        hp.n_color_sets = len(p.colors)
        for i, c in enumerate(p.colors):
            hp.color_sets[i] = fp(c)
        hp.n_morph_targets = len(p.morph_targets)
        if p.morph_targets:
            mts = (MorphTarget * len(p.morph_targets))()
            for i, t in enumerate(p.morph_targets):
                mts[i] = MorphTarget(fp(t.get("positions")), fp(t.get("normals")), fp(t.get("tangents")))
            keep.append(mts)
            hp.morph_targets = C.cast(mts, C.POINTER(MorphTarget))
            hp.morph_weights = fp(p.morph_weights)
            hp.animated_morph_weights = fp(p.animated_morph_weights)
        hp.front_face_cw = 1 if front_face_cw else 0
        insert = self.lib.awsm_host_mesh_insert_hud if getattr(p, "hud", False) else self.lib.awsm_host_mesh_insert
        k = insert(self.h, C.byref(hp), transform, material, skin, 1 if hidden else 0)
        if not k:
            self._chk(-1, "mesh_insert")
        return k

    def mesh_update_morph_weights(self, key: int, weights):
        """Morphs::update_morph_weights_with: the mesh's weights (one per target), uploaded with the next frame."""
        a, ap = _f(weights)
        self._chk(self.lib.awsm_host_mesh_update_morph_weights(self.h, key, ap, a.size), "mesh_update_morph_weights")

    def mesh_remove(self, key: int):
        self._chk(self.lib.awsm_host_mesh_remove(self.h, key), "mesh_remove")

    # ---- lights / camera / env ----
    @staticmethod
    def _light(l: dict) -> HostLight:
        kind = {"directional": 1, "point": 2, "spot": 3}[l["kind"]]
        return HostLight(kind, (C.c_float * 3)(*l["color"]), l["intensity"], (C.c_float * 3)(*l.get("position", (0, 0, 0))), l.get("range", 0.0),
                         (C.c_float * 3)(*l.get("direction", (0, 0, 0))), l.get("inner_angle", 0.0), l.get("outer_angle", 0.0))

    def light_insert(self, l: dict) -> int:
        hl = self._light(l)
        return self.lib.awsm_host_light_insert(self.h, C.byref(hl))

    def light_update(self, key: int, l: dict):
        """Lights::update: the light's new values, uploaded with the next frame."""
        hl = self._light(l)
        self._chk(self.lib.awsm_host_light_update(self.h, key, C.byref(hl)), "light_update")

    def light_remove(self, key: int):
        self._chk(self.lib.awsm_host_light_remove(self.h, key), "light_remove")

    def set_ibl_mip_counts(self, prefiltered: int, irradiance: int):
        self._chk(self.lib.awsm_host_set_ibl_mip_counts(self.h, prefiltered, irradiance), "set_ibl_mip_counts")

    def camera_update(self, view, proj, position):
        a, b, c = _f(view), _f(proj), _f(position)
        self._chk(self.lib.awsm_host_camera_update(self.h, a[1], b[1], c[1]), "camera_update")

    def env(self, skybox=(0, 0, 0, 1), prefiltered=(1, 1, 1), irradiance=(1, 1, 1), lut_rgba16f: Optional[np.ndarray] = None):
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
        self._chk(self.lib.awsm_host_env(self.h, C.byref(env)), "env")

    def env_cube(self, which: int, levels):
        """levels: [level0, ...] of (6, N_l, N_l, 4) float16 (faces +X -X +Y -Y +Z -Z), or None."""
        if not levels:
            self._chk(self.lib.awsm_host_env_cube(self.h, which, 0, 0, None), "env_cube")
            return
        flat = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(a, dtype=np.float16).reshape(-1) for a in levels])).view(np.uint16)
        self._chk(self.lib.awsm_host_env_cube(self.h, which, levels[0].shape[1], len(levels), flat.ctypes.data), "env_cube")

    # ---- environment cubes at run time (environment.rs, textures.rs:118-165, cubemap/ktx.rs) ----
    def env_cube_create(self, which: int, size: int, mips: int):
        self._chk(self.lib.awsm_host_env_cube_create(self.h, which, size, mips), "env_cube_create")

    def env_cube_update_face(self, which: int, face: int, mip: int, data, fmt="rgba16f", width: Optional[int] = None, height: Optional[int] = None,
                             bytes_per_row: Optional[int] = None, rows_per_image: Optional[int] = None, offset: int = 0):
        """update_skybox_face / update_cubemap_texture_face: an (N, N, 4) array ((N, N) uint32 for the packed formats) or raw bytes + layout."""
        width = np.asarray(data).shape[1] if width is None else width
        value, raw, layout = hip_backend.cube_source(data, fmt, width, bytes_per_row, rows_per_image, offset)
        self._chk(self.lib.awsm_host_env_cube_update_face(self.h, which, face, mip, width, width if height is None else height, value,
                                                          raw.ctypes.data, raw.nbytes, C.byref(layout)), "env_cube_update_face")

    def env_cube_update_all_faces(self, which: int, mip: int, data, fmt="rgba16f", width: Optional[int] = None, height: Optional[int] = None,
                                  bytes_per_row: Optional[int] = None, rows_per_image: Optional[int] = None, offset: int = 0):
        """update_skybox_all_faces / update_cubemap_texture_all_faces: a (6, N, N, 4) array ((6, N, N) uint32 for the packed formats) or raw bytes + layout."""
        width = np.asarray(data).shape[2] if width is None else width
        value, raw, layout = hip_backend.cube_source(data, fmt, width, bytes_per_row, rows_per_image, offset)
        self._chk(self.lib.awsm_host_env_cube_update_all_faces(self.h, which, mip, width, width if height is None else height, value,
                                                               raw.ctypes.data, raw.nbytes, C.byref(layout)), "env_cube_update_all_faces")

    def env_cube_regenerate_mipmaps(self, which: int):
        self._chk(self.lib.awsm_host_env_cube_regenerate_mipmaps(self.h, which), "env_cube_regenerate_mipmaps")

    def env_cube_colors(self, which: int, size: int, colors):
        """Skybox::new_colors / IblTexture::new_colors: one RGBA colour or six in face order."""
        c = np.asarray(colors, dtype=np.float32).reshape(-1, 4)
        c = np.ascontiguousarray(np.tile(c, (6, 1)) if c.shape[0] == 1 else c)
        assert c.shape == (6, 4), "one RGBA colour or six"
        self._chk(self.lib.awsm_host_env_cube_colors(self.h, which, size, c.ctypes.data), "env_cube_colors")

    def env_cube_sky_gradient(self, which: int, size: int, zenith=hip_backend.DEFAULT_SKY_ZENITH, nadir=hip_backend.DEFAULT_SKY_NADIR):
        """CubemapImage::new_sky_gradient (the defaults are CubemapSkyGradient::default)."""
        z, n = (C.c_float * 4)(*zenith), (C.c_float * 4)(*nadir)
        self._chk(self.lib.awsm_host_env_cube_sky_gradient(self.h, which, size, z, n), "env_cube_sky_gradient")

    def env_bake_ibl(self, prefiltered_size: int = 128, prefiltered_mips: Optional[int] = None, irradiance_size: int = 32, sample_count: int = 0):
        """The prefiltered chain and the irradiance cube filtered on the device from the skybox as it is now; sets the IBL mip counts.  Call again
        whenever the skybox changes.  prefiltered_mips defaults to the chain down to 4^2 texels (the last levels hold almost no detail)."""
        if prefiltered_mips is None:
            prefiltered_mips = max(1, int(prefiltered_size).bit_length() - 2)
        self._chk(self.lib.awsm_host_env_bake_ibl(self.h, prefiltered_size, prefiltered_mips, irradiance_size, sample_count), "env_bake_ibl")

    def env_cube_load_ktx2(self, which: int, source) -> dict:
        """A KTX2 cube map from a path or from bytes; returns the parsed header (pass info["mips"] to set_ibl_mip_counts for an IBL cube)."""
        info = Ktx2Info(struct_size=C.sizeof(Ktx2Info))
        err = C.create_string_buffer(512)
        if isinstance(source, (bytes, bytearray, memoryview)):
            buf = (C.c_uint8 * max(1, len(source))).from_buffer_copy(bytes(source) or b"\0")
            rc = self.lib.awsm_host_env_cube_load_ktx2_memory(self.h, which, buf, len(source), C.byref(info), err, 512)
        else:
            rc = self.lib.awsm_host_env_cube_load_ktx2(self.h, which, os.fsencode(source), C.byref(info), err, 512)
        if rc != 0:
            e = HostError(f"env_cube_load_ktx2 failed ({rc}): {err.value.decode(errors='replace')}")
            e.code = rc
            raise e
        return info.as_dict()

    def env_cube_from_equirect(self, which: int, array, yaw: float = 0.0, samples: int = 0, scale: float = 1.0) -> dict:
        """An equirectangular panorama (uint8 [H, W, 4] RGBE or float32 [H, W, 4]) into level 0 of an existing texel cube;
        env_cube_regenerate_mipmaps follows.  Returns what was sent: width, height, format, samples (0 = auto), yaw, scale."""
        a, pano = hip_backend.equirect_source(array, yaw, samples, scale)
        self._chk(self.lib.awsm_host_env_cube_from_equirect(self.h, which, a.ctypes.data, a.nbytes, C.byref(pano)), "env_cube_from_equirect")
        return {"width": a.shape[1], "height": a.shape[0], "format": int(pano.format), "samples": samples, "yaw": yaw, "scale": scale}

    def env_cube_load_hdr(self, which: int, source, size: int, samples: int = 0, yaw: float = 0.0, scale: float = 1.0) -> dict:
        """A Radiance .hdr panorama from a path or from bytes: decoded, projected into a `size`^2 cube with its full chain.  Returns the header
        (width, height, flipped_y, rle, exposure: EXPOSURE= is reported, not applied — pass scale = 1 / exposure for radiance)."""
        info = HdrInfo(struct_size=C.sizeof(HdrInfo))
        err = C.create_string_buffer(512)
        if isinstance(source, (bytes, bytearray, memoryview)):
            buf = (C.c_uint8 * max(1, len(source))).from_buffer_copy(bytes(source) or b"\0")
            rc = self.lib.awsm_host_env_cube_load_hdr_memory(self.h, which, buf, len(source), size, samples, yaw, scale, C.byref(info), err, 512)
        else:
            rc = self.lib.awsm_host_env_cube_load_hdr(self.h, which, os.fsencode(source), size, samples, yaw, scale, C.byref(info), err, 512)
        if rc != 0:
            raise _hdr_error("env_cube_load_hdr", rc, err)
        return info.as_dict()

    def brdf_lut_generate(self, w: int, h: int):
        self._chk(self.lib.awsm_host_brdf_lut_generate(self.h, w, h), "brdf_lut_generate")

    def resize(self, w: int, h: int):
        self._chk(self.lib.awsm_host_resize(self.h, w, h), "resize")
        self.width, self.height = w, h

    def set_shard_rows(self, y0: int, y1: int):
        self._chk(self.lib.awsm_host_set_shard_rows(self.h, y0, y1), "set_shard_rows")

    @staticmethod
    def _trs10(instances) -> np.ndarray:
        return np.ascontiguousarray([list(t) + list(r) + list(sc) for (t, r, sc) in instances], dtype=np.float32).reshape(-1, 10)

    def mesh_set_instances(self, mesh_key: int, instances):
        """Meshes::enable_mesh_instancing / set_mesh_instances: [(translation, rotation xyzw, scale), ...]."""
        a, ap = _f(self._trs10(instances))
        self._chk(self.lib.awsm_host_mesh_set_instances(self.h, mesh_key, ap, len(a)), "mesh_set_instances")

    def mesh_append_instances(self, mesh_key: int, instances) -> int:
        a, ap = _f(self._trs10(instances))
        r = self.lib.awsm_host_mesh_append_instances(self.h, mesh_key, ap, len(a))
        if r < 0:
            self._chk(r, "mesh_append_instances")
        return r

    def set_anti_aliasing(self, msaa_sample_count: int = 0, mipmap: bool = False):
        """AwsmRenderer::set_anti_aliasing: msaa 0 (None) or 4, gradient mipmaps on/off (the reference's default: 4, True)."""
        self._chk(self.lib.awsm_host_set_anti_aliasing(self.h, msaa_sample_count, 1 if mipmap else 0), "set_anti_aliasing")

    def set_post_processing(self, tonemapping: int = 1, bloom: bool = False, dof: bool = False, smaa: bool = False):
        """AwsmRenderer::set_post_processing + AntiAliasing.smaa: render() then ends with the effects + display passes (off by default here;
        the reference's default is KhronosNeutralPbr (1) without bloom or DoF).  tonemapping: 0 None, 1 KhronosNeutralPbr, 2 Aces."""
        self._chk(self.lib.awsm_host_set_post_processing(self.h, tonemapping, int(bloom), int(dof), int(smaa)), "set_post_processing")

    def clear_post_processing(self):
        """No post pass again (this library's default)."""
        self._chk(self.lib.awsm_host_clear_post_processing(self.h), "clear_post_processing")

    def set_editor_grid(self, on: bool = True, **overrides):
        """The editor's ground grid (crates/editor/src/grid), drawn by the transparent pass of every later render(): grid.wgsl's constants with
        `overrides` (hip_backend.AwsmEditorGrid's field names).  on=False turns it off."""
        if not on:
            return self._chk(self.lib.awsm_host_set_editor_grid(self.h, None), "set_editor_grid")
        g = hip_backend.AwsmEditorGrid()
        self._chk(self.lib.awsm_host_editor_grid_defaults(self.h, C.byref(g)), "editor_grid_defaults")
        g.override(**overrides)
        self._chk(self.lib.awsm_host_set_editor_grid(self.h, C.byref(g)), "set_editor_grid")

    def set_selection(self, mesh_keys=(), on: bool = True, struct_size: Optional[int] = None, **overrides):
        """The editor's selection overlay in every later render(): an outline around the visible pixels of the meshes `mesh_keys` (as pick() and
        mesh_insert() report them) and a wire box around each one's world AABB, which follows the mesh's transform; the backend's defaults with
        `overrides` (hip_backend.AwsmSelection's field names).  on=False turns it off.  struct_size: what the record claims as its size (tests)."""
        if not on:
            return self._chk(self.lib.awsm_host_set_selection(self.h, None, None, 0), "set_selection")
        s = hip_backend.AwsmSelection()
        self._chk(self.lib.awsm_host_selection_defaults(self.h, C.byref(s)), "selection_defaults")
        s.override(**overrides)
        if struct_size is not None:
            s.struct_size = struct_size
        keys = (C.c_uint64 * max(1, len(mesh_keys)))(*[int(k) for k in mesh_keys])
        self._chk(self.lib.awsm_host_set_selection(self.h, C.byref(s), keys, len(mesh_keys)), "set_selection")

    def set_taa(self, on: bool = True, **overrides):
        """Temporal anti-aliasing in every later render(): the projection is jittered per frame and the post pass (set_post_processing first)
        begins with the history resolve.  overrides: feedback (0.1), strength_still (0.8), strength_moving (0.2).  on=False turns it off."""
        if not on:
            return self._chk(self.lib.awsm_host_set_taa(self.h, None), "set_taa")
        t = HostTaa(C.sizeof(HostTaa), 0.1, 0.8, 0.2)
        for k, v in overrides.items():
            if k not in ("feedback", "strength_still", "strength_moving"):
                raise TypeError("AwsmHostTaa has no field %r (fields: feedback, strength_still, strength_moving)" % k)
            setattr(t, k, float(v))
        self._chk(self.lib.awsm_host_set_taa(self.h, C.byref(t)), "set_taa")

    def taa_jitter(self, frame_count: int, moved: bool = False):
        """The NDC offset (x, y) a render with that frame count jitters the projection by, as float32 (no device work)."""
        out = np.zeros(2, dtype=np.float32)
        self._chk(self.lib.awsm_host_taa_jitter(self.h, frame_count, int(moved), out.ctypes.data_as(F32P)), "taa_jitter")
        return out

    def set_ssao(self, on: bool = True, **overrides):
        """Screen-space ambient occlusion in the opaque pass of every later render(): the backend's defaults with `overrides`
        (hip_backend.AwsmSsao's field names: radius, intensity, bias, strength).  on=False turns it off."""
        if not on:
            return self._chk(self.lib.awsm_host_set_ssao(self.h, None), "set_ssao")
        s = hip_backend.AwsmSsao()
        self._chk(self.lib.awsm_host_ssao_defaults(self.h, C.byref(s)), "ssao_defaults")
        s.override(**overrides)
        self._chk(self.lib.awsm_host_set_ssao(self.h, C.byref(s)), "set_ssao")

    def set_shadow(self, light: Optional[int] = None, struct_size: Optional[int] = None, **overrides):
        """Shadows from one directional or spot light in every later render(): `light` is a key light_insert returned; the backend's defaults with
        `overrides` (map_size, pcf_radius, bias, slope_bias, max_slope, strength, facing_fade).  light=None turns them off."""
        if light is None:
            return self._chk(self.lib.awsm_host_set_shadow(self.h, None), "set_shadow")
        s = HostShadow()
        self._chk(self.lib.awsm_host_shadow_defaults(self.h, C.byref(s)), "shadow_defaults")
        s.override(**overrides)
        s.light = light
        if struct_size is not None:
            s.struct_size = struct_size
        self._chk(self.lib.awsm_host_set_shadow(self.h, C.byref(s)), "set_shadow")

    def set_shadow_cascades(self, count: int = 1, lambda_: float = 0.5, max_distance: float = 0.0, struct_size: Optional[int] = None):
        """Cascades for a shadowed directional light in every later render(): `count` (1 .. 4) nested windows along the camera's depth, tightest
        first; count = 1 is the single map.  Spot and point lights ignore it."""
        c = HostShadowCascades()
        self._chk(self.lib.awsm_host_shadow_cascades_defaults(C.byref(c)), "shadow_cascades_defaults")
        c.count, c.lambda_, c.max_distance = int(count), float(lambda_), float(max_distance)
        if struct_size is not None:
            c.struct_size = struct_size
        self._chk(self.lib.awsm_host_set_shadow_cascades(self.h, C.byref(c)), "set_shadow_cascades")

    def shadow_views(self, cap: int = 65536):
        """What the last render() handed the backend's shadow pass -> [(the 512-byte light block, the caster draws as dicts), ...], one per view."""
        n_views = C.c_uint32(0)
        self._chk(self.lib.awsm_host_shadow_view_count(self.h, C.byref(n_views)), "shadow_view_count")
        fields = [f for f, _ in hip_backend.AwsmDraw._fields_]
        out = []
        for view in range(n_views.value):
            block = (C.c_uint8 * 512)()
            n = C.c_uint32(0)
            self._chk(self.lib.awsm_host_shadow_view(self.h, view, block, None, 0, C.byref(n)), "shadow_view")
            draws = (hip_backend.AwsmDraw * max(1, n.value))()
            self._chk(self.lib.awsm_host_shadow_view(self.h, view, None, draws, n.value, None), "shadow_view")
            out.append((bytes(block), [{f: int(getattr(draws[i], f)) for f in fields} for i in range(n.value)]))
        return out

    def shadow_camera(self, cap: int = 65536):
        """What the last render() handed the backend's shadow pass -> (the 512-byte light block, the caster draws as dicts)."""
        block = (C.c_uint8 * 512)()
        draws = (hip_backend.AwsmDraw * max(1, cap))()
        n = C.c_uint32(0)
        self._chk(self.lib.awsm_host_shadow_camera(self.h, block, draws, cap, C.byref(n)), "shadow_camera")
        if n.value > cap:
            return self.shadow_camera(n.value)
        fields = [f for f, _ in hip_backend.AwsmDraw._fields_]
        return bytes(block), [{f: int(getattr(draws[i], f)) for f in fields} for i in range(n.value)]

    def camera_set_dof(self, focus_distance: float = 10.0, aperture: float = 5.6):
        """CameraMatrices.focus_distance / .aperture (camera bytes 496-503; the reference's defaults 10.0 and 5.6)."""
        self._chk(self.lib.awsm_host_camera_set_dof(self.h, focus_distance, aperture), "camera_set_dof")

    def pick(self, x: int, y: int, transparent: bool = False, alpha_threshold: float = 0.5):
        """AwsmRenderer::pick: the MeshKey under pixel (x, y) of the last rendered frame, or None (PickResult::Miss).  transparent=True: a
        transparent mesh whose fragment there was blended with alpha >= alpha_threshold is hit too (awsm_hip_pick_ex has the rule)."""
        hit, key = C.c_uint32(0), C.c_uint64(0)
        if transparent:
            self._chk(self.lib.awsm_host_pick_ex(self.h, x, y, 1, alpha_threshold, C.byref(hit), C.byref(key), None), "pick_ex")
        else:
            self._chk(self.lib.awsm_host_pick(self.h, x, y, C.byref(hit), C.byref(key)), "pick")
        return key.value if hit.value else None

    def pick_rect(self, x0: int, y0: int, x1: int, y1: int, transparent: bool = False, alpha_threshold: float = 0.5, cap: int = 1024):
        """The meshes the rectangle [x0, x1) x [y0, y1) of the last rendered frame shows -> [(MeshKey, layer, pixels)], ordered by layer (0 world
        opaque, 1 world transparent, 2 HUD opaque, 3 HUD transparent), then by draw order."""
        keys, layers, pixels = (C.c_uint64 * max(1, cap))(), (C.c_uint32 * max(1, cap))(), (C.c_uint32 * max(1, cap))()
        n = C.c_uint32(0)
        self._chk(self.lib.awsm_host_pick_rect(self.h, x0, y0, x1, y1, 1 if transparent else 0, alpha_threshold, keys, layers, pixels, cap, C.byref(n)), "pick_rect")
        if n.value > cap:
            return self.pick_rect(x0, y0, x1, y1, transparent, alpha_threshold, n.value)
        return [(int(keys[i]), int(layers[i]), int(pixels[i])) for i in range(n.value)]

    def set_shard_bands(self, n: int, r: int, compact_output: bool = False):
        self._chk(self.lib.awsm_host_set_shard_bands(self.h, n, r, 1 if compact_output else 0), "set_shard_bands")

    def set_render_timings(self, enabled: bool):
        """AwsmRendererLogging.render_timings (debug.rs:8-12): per-stage times in the frame stats (default on)."""
        self._chk(self.lib.awsm_host_set_render_timings(self.h, 1 if enabled else 0), "set_render_timings")

    # ---- frame ----
    def set_render_hooks(self, after_geometry_pass=None, after_opaque_pass=None):
        """RenderHooks: Python callables (no arguments; an exception aborts the frame) run between the passes of render()."""
        HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p)

        def wrap(fn):
            if fn is None:
                return None

            def call(_user):
                try:
                    fn()
                    return 0
                except Exception as e:      # noqa: BLE001 — reported through the status code
                    self._hook_error = e
                    return -3
            return HOOK(call)
        self._hooks = (wrap(after_geometry_pass), wrap(after_opaque_pass))     # kept alive as long as they are installed
        self._chk(self.lib.awsm_host_set_render_hooks(self.h, C.cast(self._hooks[0], C.c_void_p) if self._hooks[0] else None, None,
                                                      C.cast(self._hooks[1], C.c_void_p) if self._hooks[1] else None, None), "set_render_hooks")

    # ---- animation (animation/animations.rs) ----
    def _animation_insert(self, fn, target, path, times, values, interpolation, in_tangents, out_tangents, duration):
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(len(t), -1) if len(t) else np.zeros((0, 0), np.float32)
        clip = AnimationClip(struct_size=C.sizeof(AnimationClip), path=ANIM_PATHS[path], interpolation=ANIM_INTERPOLATIONS[interpolation],
                             n_keys=len(t), width=v.shape[1])
        keep = [t, v]
        clip.times, clip.values = t.ctypes.data_as(C.POINTER(C.c_double)), v.ctypes.data_as(F32P)
        for name, arr in (("in_tangents", in_tangents), ("out_tangents", out_tangents)):
            if arr is not None:
                a = np.ascontiguousarray(arr, dtype=np.float32).reshape(len(t), -1)
                keep.append(a)
                setattr(clip, name, a.ctypes.data_as(F32P))
        clip.duration = float(t[-1] - t[0]) if duration is None and len(t) else float(duration or 0.0)      # gltf/populate/animation.rs:107,229
        k = fn(self.h, C.byref(clip), target)
        if not k:
            self._chk(-1, "animation_insert")
        return k

    def animation_insert_transform(self, transform: int, path: str, times, values, interpolation: str = "linear", in_tangents=None, out_tangents=None,
                                   duration: Optional[float] = None) -> int:
        """A player (speed 1/1000, Loop, Forward, Playing) for one of a node's translation / rotation / scale; values: (keys, 3 or 4).  duration
        defaults to last key - first key, as the glTF reader sets it."""
        return self._animation_insert(self.lib.awsm_host_animation_insert_transform, transform, path, times, values, interpolation, in_tangents, out_tangents, duration)

    def animation_insert_morph(self, mesh: int, times, values, interpolation: str = "linear", in_tangents=None, out_tangents=None,
                               duration: Optional[float] = None) -> int:
        """A player for a mesh's morph weights; values: (keys, targets)."""
        return self._animation_insert(self.lib.awsm_host_animation_insert_morph, mesh, "weights", times, values, interpolation, in_tangents, out_tangents, duration)

    def animation_remove(self, key: int):
        self._chk(self.lib.awsm_host_animation_remove(self.h, key), "animation_remove")

    def animation_state(self, key: int) -> dict:
        st = AnimationState(struct_size=C.sizeof(AnimationState))
        self._chk(self.lib.awsm_host_animation_state(self.h, key, C.byref(st)), "animation_state")
        return {k: getattr(st, k) for k in ("local_time", "direction", "state", "loop_style", "duration", "speed")}

    def animation_set_playback(self, key: int, speed: Optional[float] = None, loop_style: Optional[int] = None, direction: Optional[int] = None,
                               state: Optional[int] = None):
        """The player's speed, loop style (ANIM_LOOP_NONE / ANIM_LOOP / ANIM_PING_PONG), direction and state; None keeps a value."""
        cur = self.animation_state(key)
        pick = lambda v, name: cur[name] if v is None else v      # noqa: E731
        self._chk(self.lib.awsm_host_animation_set_playback(self.h, key, pick(speed, "speed"), pick(loop_style, "loop_style"), pick(direction, "direction"),
                                                            pick(state, "state")), "animation_set_playback")

    def animation_seek(self, key: int, local_time: float):
        self._chk(self.lib.awsm_host_animation_seek(self.h, key, local_time), "animation_seek")

    def animation_sample(self, key: int) -> np.ndarray:
        """The value at the player's local time (nothing applied): 3, 4 or target-count float32."""
        n = self.lib.awsm_host_animation_sample(self.h, key, None, 0)      # the width
        if n < 0:
            self._chk(n, "animation_sample")
        out = np.zeros(max(1, n), np.float32)
        n = self.lib.awsm_host_animation_sample(self.h, key, out.ctypes.data_as(F32P), out.size)
        if n < 0:
            self._chk(n, "animation_sample")
        return out[:n].copy()

    def update_animations(self, global_time_delta: float):
        """AwsmRenderer::update_animations: every player advances by global_time_delta * speed and is applied."""
        self._chk(self.lib.awsm_host_update_animations(self.h, float(global_time_delta)), "update_animations")

    def set_device_skin_posing(self, on: bool):
        """Skin matrices composed on the device from the world matrices already there (off by default; the same bytes either way)."""
        self._chk(self.lib.awsm_host_set_device_skin_posing(self.h, 1 if on else 0), "set_device_skin_posing")

    def skin_pose_ids_last_frame(self) -> List[int]:
        n = C.c_uint32()
        self._chk(self.lib.awsm_host_skin_pose_ids_last_frame(self.h, None, 0, C.byref(n)), "skin_pose_ids_last_frame")
        arr = (C.c_uint32 * max(1, n.value))()
        self._chk(self.lib.awsm_host_skin_pose_ids_last_frame(self.h, arr, n.value, C.byref(n)), "skin_pose_ids_last_frame")
        return list(arr[: n.value])

    def update_transforms(self):
        self._chk(self.lib.awsm_host_update_transforms(self.h), "update_transforms")

    def render(self, sync: bool = True) -> Optional[dict]:
        st = AwsmFrameStats()
        st.struct_size = C.sizeof(AwsmFrameStats)
        self._chk(self.lib.awsm_host_render(self.h, 1 if sync else 0, C.byref(st) if sync else None), "render")
        return st.as_dict() if sync else None

    # ---- introspection ----
    def mirror(self, which: int) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.awsm_host_mirror(self.h, which, C.byref(p), C.byref(n)), "mirror")
        return C.string_at(p, n.value)

    def load_gltf(self, path: str, scene_index: int = -1, srgb_textures: bool = False) -> dict:
        """Populate this host from a .gltf / .glb file (awsm_host_load_gltf); returns the counts of what was inserted.  srgb_textures: colour
        images (base colour, emissive, specular colour, sheen colour) are decoded from sRGB as they enter the pool (awsm_host_load_gltf_ex)."""
        info = (C.c_uint32 * 12)()
        err = C.create_string_buffer(512)
        if srgb_textures:
            opt = GltfOptions(C.sizeof(GltfOptions), scene_index, AWSM_GLTF_SRGB_COLOR_TEXTURES)
            rc = self.lib.awsm_host_load_gltf_ex(self.h, os.fsencode(path), C.byref(opt), info, err, 512)
        else:
            rc = self.lib.awsm_host_load_gltf(self.h, os.fsencode(path), scene_index, info, err, 512)
        if rc != 0:
            raise HostError(f"load_gltf({path}) failed ({rc}): {err.value.decode(errors='replace')}")
        names = ("nodes", "meshes", "materials", "images", "samplers", "skins", "lights", "triangles", "generated_tangents", "instanced_meshes",
                 "animations", "animation_channels_skipped")
        return {k: int(info[i]) for i, k in enumerate(names)}

    def gltf_animation_keys(self) -> List[int]:
        """The players the last load_gltf made, in insertion order (awsm_host_gltf_animation_keys)."""
        n = C.c_uint32()
        self._chk(self.lib.awsm_host_gltf_animation_keys(self.h, None, 0, C.byref(n)), "gltf_animation_keys")
        arr = (C.c_uint64 * max(1, n.value))()
        self._chk(self.lib.awsm_host_gltf_animation_keys(self.h, arr, n.value, C.byref(n)), "gltf_animation_keys")
        return list(arr[: n.value])

    def transparent_draw_list(self) -> List[dict]:
        """The world transparent pass's list: back to front; vis_data_off = offset into the transparency geometry buffer."""
        return self.draw_list(fn="awsm_host_transparent_draw_list")

    def draw_list(self, fn: str = "awsm_host_draw_list") -> List[dict]:
        n = C.c_uint32()
        f = getattr(self.lib, fn)
        self._chk(f(self.h, None, 0, C.byref(n)), "draw_list")
        arr = (AwsmDraw * max(1, n.value))()
        self._chk(f(self.h, arr, n.value, C.byref(n)), "draw_list")
        out = []
        for d in arr[:n.value]:
            e = {"geom_meta_off": d.geom_meta_off, "vis_data_off": d.vis_data_off, "tri_count": d.tri_count, "flags": d.flags}
            if d.inst_count:
                e["inst_off"], e["inst_count"] = d.inst_off, d.inst_count
            out.append(e)
        return out

    def pool_arrays(self) -> List[np.ndarray]:
        """The pool's content, one (layers, h, w, 4) uint8 array per pool array (awsm_host_texture_array_info: the host's mirror)."""
        out = []
        for i in range(self.lib.awsm_host_texture_array_count(self.h)):
            w, h, n, p = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_void_p()
            self._chk(self.lib.awsm_host_texture_array_info(self.h, i, C.byref(w), C.byref(h), C.byref(n), C.byref(p)), "texture_array_info")
            out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value, h.value, w.value, 4)).copy())
        return out

    def upload_bytes_last_frame(self) -> int:
        return self.lib.awsm_host_upload_bytes_last_frame(self.h)


def _texref(ref: Optional[TextureRef], tt_keys: Dict[tuple, int], host: Host) -> TexRef:
    if ref is None:
        return TexRef(-1, 0, 0, 0, 0)
    tk = 0
    if ref.transform:
        t = ref.transform
        sig = (tuple(t.get("offset", (0, 0))), tuple(t.get("origin", (0, 0))), float(t.get("rotation", 0.0)), tuple(t.get("scale", (1, 1))))
        if sig not in tt_keys:
            tt_keys[sig] = host.texture_transform_insert(*sig)
        tk = tt_keys[sig]
    return TexRef(ref.texture, ref.sampler, ref.uv_index, 0, tk)


def material_struct(m: MaterialDesc, host: Host, tt_keys: Dict[tuple, int]) -> HostMaterial:
    tr = lambda r: _texref(r, tt_keys, host)   # noqa: E731
    hm = HostMaterial()
    hm.struct_size = C.sizeof(HostMaterial)
    hm.shader = 2 if m.kind == "unlit" else 1
    hm.double_sided = 1 if m.double_sided else 0
    hm.base_color_factor = (C.c_float * 4)(*m.base_color_factor)
    hm.metallic_factor, hm.roughness_factor, hm.normal_scale, hm.occlusion_strength = m.metallic_factor, m.roughness_factor, m.normal_scale, m.occlusion_strength
    hm.emissive_factor = (C.c_float * 3)(*m.emissive_factor)
    hm.debug_bitmask = m.debug_bitmask
    hm.alpha_mode = {"opaque": 0, "mask": 1, "blend": 2}[m.alpha_mode]
    hm.alpha_cutoff = m.alpha_cutoff
    hm.base_color_tex, hm.metallic_roughness_tex, hm.normal_tex = tr(m.base_color_tex), tr(m.metallic_roughness_tex), tr(m.normal_tex)
    hm.occlusion_tex, hm.emissive_tex = tr(m.occlusion_tex), tr(m.emissive_tex)
    none = TexRef(-1, 0, 0, 0, 0)
    for name in ("specular_tex", "specular_color_tex", "transmission_tex", "volume_thickness_tex", "clearcoat_tex", "clearcoat_roughness_tex",
                 "clearcoat_normal_tex", "sheen_roughness_tex", "sheen_color_tex", "diffuse_transmission_tex", "diffuse_transmission_color_tex", "anisotropy_tex",
                 "iridescence_tex", "iridescence_thickness_tex"):
        setattr(hm, name, none)
    if m.vertex_color_set is not None:
        hm.has_vertex_color, hm.vertex_color_set = 1, m.vertex_color_set
    if m.emissive_strength is not None:
        hm.has_emissive_strength, hm.emissive_strength = 1, m.emissive_strength
    if m.ior is not None:
        hm.has_ior, hm.ior = 1, m.ior
    if m.specular is not None:
        s = m.specular
        hm.has_specular, hm.specular_factor = 1, s.get("factor", 1.0)
        hm.specular_color_factor = (C.c_float * 3)(*s.get("color_factor", (1, 1, 1)))
        hm.specular_tex, hm.specular_color_tex = tr(s.get("tex")), tr(s.get("color_tex"))
    if m.transmission is not None:
        s = m.transmission
        hm.has_transmission, hm.transmission_factor, hm.transmission_tex = 1, s.get("factor", 0.0), tr(s.get("tex"))
    if m.volume is not None:
        s = m.volume
        hm.has_volume, hm.volume_thickness_factor, hm.volume_attenuation_distance = 1, s.get("thickness_factor", 0.0), s.get("attenuation_distance", 0.0)
        hm.volume_attenuation_color = (C.c_float * 3)(*s.get("attenuation_color", (1, 1, 1)))
        hm.volume_thickness_tex = tr(s.get("thickness_tex"))
    if m.clearcoat is not None:
        s = m.clearcoat
        hm.has_clearcoat, hm.clearcoat_factor, hm.clearcoat_roughness_factor = 1, s.get("factor", 0.0), s.get("roughness_factor", 0.0)
        hm.clearcoat_normal_scale = s.get("normal_scale", 1.0)
        hm.clearcoat_tex, hm.clearcoat_roughness_tex, hm.clearcoat_normal_tex = tr(s.get("tex")), tr(s.get("roughness_tex")), tr(s.get("normal_tex"))
    if m.sheen is not None:
        s = m.sheen
        hm.has_sheen, hm.sheen_roughness_factor = 1, s.get("roughness_factor", 0.0)
        hm.sheen_color_factor = (C.c_float * 3)(*s.get("color_factor", (0, 0, 0)))
        hm.sheen_roughness_tex, hm.sheen_color_tex = tr(s.get("roughness_tex")), tr(s.get("color_tex"))
    if m.diffuse_transmission is not None:
        s = m.diffuse_transmission
        hm.has_diffuse_transmission, hm.diffuse_transmission_factor = 1, s.get("factor", 0.0)
        hm.diffuse_transmission_color_factor = (C.c_float * 3)(*s.get("color_factor", (1, 1, 1)))
        hm.diffuse_transmission_tex, hm.diffuse_transmission_color_tex = tr(s.get("tex")), tr(s.get("color_tex"))
    if m.dispersion is not None:
        hm.has_dispersion, hm.dispersion = 1, m.dispersion
    if m.anisotropy is not None:
        s = m.anisotropy
        hm.has_anisotropy, hm.anisotropy_strength, hm.anisotropy_rotation, hm.anisotropy_tex = 1, s.get("strength", 0.0), s.get("rotation", 0.0), tr(s.get("tex"))
    if m.iridescence is not None:
        s = m.iridescence
        hm.has_iridescence, hm.iridescence_factor, hm.iridescence_ior = 1, s.get("factor", 0.0), s.get("ior", 1.3)
        hm.iridescence_thickness_min, hm.iridescence_thickness_max = s.get("thickness_min", 100.0), s.get("thickness_max", 400.0)
        hm.iridescence_tex, hm.iridescence_thickness_tex = tr(s.get("tex")), tr(s.get("thickness_tex"))
    return hm


def decode_image(data: bytes) -> np.ndarray:
    """PNG / baseline JPEG bytes -> (h, w, 4) u8 through the host library's own decoders (awsm_host_decode_image)."""
    lib = load_library()
    w, h = C.c_uint32(), C.c_uint32()
    err = C.create_string_buffer(256)
    rc = lib.awsm_host_decode_image(data, len(data), None, 0, C.byref(w), C.byref(h), err, 256)
    if rc != 0:
        raise HostError(f"decode_image failed ({rc}): {err.value.decode(errors='replace')}")
    out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    rc = lib.awsm_host_decode_image(data, len(data), out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(w), C.byref(h), err, 256)
    if rc != 0:
        raise HostError(f"decode_image failed ({rc}): {err.value.decode(errors='replace')}")
    return out


class Populated:
    """Keys produced by populate(): what the reference keeps in GltfKeyLookups."""

    def __init__(self):
        self.node_keys: List[int] = []
        self.mesh_keys: List[int] = []
        self.material_keys: Dict[int, int] = {}
        self.skin_keys: Dict[int, int] = {}
        self.light_keys: List[int] = []


def populate(host: Host, scene: SceneDesc, srgb_textures=()) -> Populated:
    """srgb_textures: indices of scene.textures whose bytes are sRGB-encoded (decoded on the device as they enter the pool)."""
    out = Populated()
    kinds = texture_mip_kinds(scene)
    for i, (tex, kind) in enumerate(zip(scene.textures, kinds)):
        host.texture_insert(tex, kind, srgb=i in srgb_textures)
    for s in scene.samplers:
        host.sampler_insert(s)
    host.set_ibl_mip_counts(scene.prefiltered_mip_count, scene.irradiance_mip_count)
    children: Dict[Optional[int], List[int]] = {}
    for i, n in enumerate(scene.nodes):
        children.setdefault(n.parent, []).append(i)
    out.node_keys = [0] * len(scene.nodes)

    def add_transform(i, parent_key):
        n = scene.nodes[i]
        out.node_keys[i] = host.transform_insert(n.translation, n.rotation, n.scale, parent_key)
        for c in children.get(i, []):
            add_transform(c, out.node_keys[i])

    for r in children.get(None, []):
        add_transform(r, 0)
    joint_nodes = set(j for sk in scene.skins for j in sk.joints)
    tt_keys: Dict[tuple, int] = {}

    def add_meshes(i):
        n = scene.nodes[i]
        if n.primitives:
            tk = out.node_keys[i]
            if i in joint_nodes:   # populate/mesh.rs:36-52: a skinned mesh on a joint node gets a fresh identity transform
                tk = host.transform_insert((0, 0, 0), (0, 0, 0, 1), (1, 1, 1), host.transform_parent(tk))
            for p in n.primitives:
                skin_key = 0
                if n.skin is not None and p.joints:   # one Skins::insert per primitive, like populate_gltf_primitive
                    sk = scene.skins[n.skin]
                    skin_key = host.skin_insert([out.node_keys[j] for j in sk.joints], sk.inverse_bind, p.joints, p.weights)
                if p.material not in out.material_keys:
                    out.material_keys[p.material] = host.material_insert(material_struct(scene.materials[p.material], host, tt_keys))
                out.mesh_keys.append(host.mesh_insert(p, tk, out.material_keys[p.material], skin_key))
                if p.instances is not None:
                    host.mesh_set_instances(out.mesh_keys[-1], p.instances)
        for c in children.get(i, []):
            add_meshes(c)

    for r in children.get(None, []):
        add_meshes(r)
    for l in scene.lights:
        out.light_keys.append(host.light_insert(l))
    return out


class Renderer:
    """Convenience wrapper: Host + populated scene, frame loop = update_all -> render (crates/renderer/src/update.rs, render.rs)."""

    def __init__(self, scene: SceneDesc, backend_path: Optional[str] = None, device: int = 0, stream: Optional[int] = None, parity_tap: bool = False,
                 lut_rgba16f: Optional[np.ndarray] = None, lut_size: int = 1024, msaa: int = 0, mipmap: bool = False, overlap_frames: bool = False,
                 gltf: Optional[str] = None, anisotropic: bool = False, srgb_textures=None):
        """gltf: path of a .gltf / .glb file to populate from (AwsmRenderer::populate_gltf); `scene` then only supplies the frame size,
        the camera and the environment.  srgb_textures: with gltf, True decodes the colour images from sRGB (Host.load_gltf); without, the
        indices of scene.textures that hold sRGB-encoded bytes."""
        self.scene = scene
        self.host = Host(backend_path, device, stream, parity_tap, overlap_frames, anisotropic)      # anisotropic: AWSM_CFG_ANISOTROPIC (include/awsm_hip.h)
        self.host.set_anti_aliasing(msaa, mipmap)   # AwsmRendererBuilder::with_anti_aliasing (off unless asked: BASELINE configs are single-sampled, MipmapMode::None)
        self.host.resize(scene.width, scene.height)
        if gltf is not None:
            self.host.set_ibl_mip_counts(scene.prefiltered_mip_count, scene.irradiance_mip_count)
            self.gltf_info = self.host.load_gltf(gltf, srgb_textures=bool(srgb_textures))
            self.keys = None
        else:
            self.keys = populate(self.host, scene, tuple(srgb_textures or ()))
        if lut_rgba16f is not None:
            self.host.env(scene.skybox_rgba, scene.prefiltered_rgb, scene.irradiance_rgb, lut_rgba16f)
        else:
            self.host.env(scene.skybox_rgba, scene.prefiltered_rgb, scene.irradiance_rgb)
            self.host.brdf_lut_generate(lut_size, lut_size)   # BrdfLut::new at build() time (renderer-core brdf_lut/generate.rs)
        for k, name in enumerate(("skybox", "prefiltered", "irradiance")):
            if scene.env_cubes and scene.env_cubes.get(name):
                self.host.env_cube(k, scene.env_cubes[name])
        self.update()

    def update(self):
        self.host.update_transforms()
        self.host.camera_update(self.scene.view, self.scene.proj, self.scene.camera_position)

    def update_all(self, global_time_delta: float):
        """update_all (update.rs:8-18): animations -> transforms -> camera."""
        self.host.update_animations(global_time_delta)
        self.update()

    def render(self, sync: bool = True):
        return self.host.render(sync)

    def set_post_processing(self, tonemapping: int = 1, bloom: bool = False, dof: bool = False, smaa: bool = False):
        self.host.set_post_processing(tonemapping, bloom, dof, smaa)

    def clear_post_processing(self):
        self.host.clear_post_processing()

    def set_editor_grid(self, on: bool = True, **overrides):
        self.host.set_editor_grid(on, **overrides)

    def set_ssao(self, on: bool = True, **overrides):
        self.host.set_ssao(on, **overrides)

    def set_taa(self, on: bool = True, **overrides):
        self.host.set_taa(on, **overrides)

    def set_selection(self, mesh_keys=(), on: bool = True, **overrides):
        """Outline and box the meshes `mesh_keys` (keys from pick()) in every later render(); on=False for off."""
        self.host.set_selection(mesh_keys, on, **overrides)

    def pick(self, x: int, y: int, transparent: bool = False, alpha_threshold: float = 0.5):
        """The MeshKey under pixel (x, y) of the last frame, or None; transparent=True picks through the transparent meshes' fragments."""
        return self.host.pick(x, y, transparent, alpha_threshold)

    def pick_rect(self, x0: int, y0: int, x1: int, y1: int, transparent: bool = False, alpha_threshold: float = 0.5):
        """[(MeshKey, layer, pixels)] of the meshes the rectangle [x0, x1) x [y0, y1) of the last frame shows."""
        return self.host.pick_rect(x0, y0, x1, y1, transparent, alpha_threshold)

    def set_shadow(self, light=True, cascades: Optional[int] = None, cascade_lambda: float = 0.5, cascade_distance: float = 0.0, **overrides):
        """Shadows from one of the scene's lights: an index into scene.lights (directional, spot or point), True for the first directional light
        (the first spot light if there is none), False / None for off.  cascades = N: a directional light's N nested windows along the camera's
        depth (Host.set_shadow_cascades), with cascade_lambda and cascade_distance."""
        if light is None or light is False:
            return self.host.set_shadow(None)
        if cascades is not None:
            self.host.set_shadow_cascades(cascades, cascade_lambda, cascade_distance)
        if light is True:
            kinds = [l.get("kind", "directional") for l in self.scene.lights]
            light = kinds.index("directional") if "directional" in kinds else (kinds.index("spot") if "spot" in kinds else None)
            if light is None:
                raise HostError("set_shadow: the scene has no directional or spot light")
        if self.keys is None:
            raise HostError("set_shadow: a scene populated from a glTF file keeps no light keys here; use Host.set_shadow with a key of light_insert")
        self.host.set_shadow(self.keys.light_keys[light], **overrides)

    def camera_set_dof(self, focus_distance: float = 10.0, aperture: float = 5.6):
        self.host.camera_set_dof(focus_distance, aperture)

    def close(self):
        self.host.close()
