/*
 * awsm_host.h — flat C API of the C++ host layer (libawsm_host.so).
 *
 * The host layer is the MI355X build's counterpart of the reference's Rust scene state: it keeps the
 * key-based update API (TransformKey / MeshKey / MaterialKey ...) and the DynamicUniformBuffer /
 * DynamicStorageBuffer dirty-upload semantics, and drives the kernels ONLY through the C-ABI of
 * include/awsm_hip.h (loaded at run time from the library path given to awsm_host_create).
 * The reference has no C interface; each function names the Rust method it mirrors
 * (paths relative to /root/reference/crates/renderer/src/).  Rust is not available in this environment,
 * so the host is C++ and this header is how Python (ctypes) and the tests reach it.
 *
 * Keys are slotmap `KeyData::as_ffi()` values: (version << 32) | idx, never 0.  0 means "none"/"root".
 * All functions return 0 or a negative AwsmStatus (include/awsm_hip.h) unless stated otherwise.
 */
#ifndef AWSM_HOST_H
#define AWSM_HOST_H

#include <stddef.h>
#include <stdint.h>
#include "awsm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 2: AwsmHostMaterial carries struct_size (fields are only ever appended; a caller compiled against a shorter struct is read up to its
 *    size, the rest defaults to "block absent"); awsm_host_render passes AwsmFrameStats.struct_size through (awsm_hip.h). */
#define AWSM_HOST_ABI_VERSION 2u
uint32_t awsm_host_abi_version(void);

typedef struct AwsmHost AwsmHost;
typedef uint64_t AwsmKey;

/* AwsmRendererBuilder::build (lib.rs:213-259).  backend_path = shared library exporting the awsm_hip_* C-ABI
 * (libawsm_hip.so).  There is no built-in device fallback: a missing library or symbol fails here. */
int awsm_host_create(const char* backend_path, int device, void* stream, uint32_t cfg_flags, AwsmHost** out);
int awsm_host_destroy(AwsmHost* h);
const char* awsm_host_last_error(const AwsmHost* h);
void* awsm_host_device_ctx(AwsmHost* h);     /* the AwsmHipCtx*, for readback helpers */

/* ---- Transforms (transforms.rs:43-446) ---- */
AwsmKey awsm_host_transform_root(AwsmHost* h);
AwsmKey awsm_host_transform_insert(AwsmHost* h, const float translation[3], const float rotation_xyzw[4], const float scale[3], AwsmKey parent);
int awsm_host_transform_set_local(AwsmHost* h, AwsmKey key, const float translation[3], const float rotation_xyzw[4], const float scale[3]);
int awsm_host_transform_set_parent(AwsmHost* h, AwsmKey child, AwsmKey parent);
int awsm_host_transform_remove(AwsmHost* h, AwsmKey key);
AwsmKey awsm_host_transform_parent(AwsmHost* h, AwsmKey child);          /* 0 if none */
int awsm_host_transform_world(AwsmHost* h, AwsmKey key, float out_mat4[16]);
/* Transforms::get_local (transforms.rs:229-233): the node's translation, rotation (xyzw) and scale as last set */
int awsm_host_transform_get_local(AwsmHost* h, AwsmKey key, float translation[3], float rotation_xyzw[4], float scale[3]);
/* Transforms::duplicate (transforms.rs:151-155): a new node with the same local transform under the same parent (children and meshes are not
 * copied); returns its key, 0 on failure */
AwsmKey awsm_host_transform_duplicate(AwsmHost* h, AwsmKey key);

/* ---- Textures (textures.rs; renderer-core texture_pool): decoded RGBA8 images, one array per (w,h) ---- */
int awsm_host_texture_insert(AwsmHost* h, const uint8_t* rgba8, uint32_t width, uint32_t height);   /* returns texture id >= 0; mip kind albedo */
/* with the MipmapTextureKind the image's role implies (0 albedo, 1 normal, 2 metallic-roughness, 3 occlusion, 4 emissive, 5.. box) */
int awsm_host_texture_insert_kind(AwsmHost* h, const uint8_t* rgba8, uint32_t width, uint32_t height, uint32_t mipmap_kind);
/* TexturePool::add_image with its TextureColorInfo (texture_pool.rs:233-303): srgb_to_linear decodes the colour channels on the
 * device as the image enters the pool (base colour, emissive, specular colour and sheen colour images: gltf/populate/material.rs:140,255,348,567),
 * premultiply_alpha multiplies them by alpha first.  Needs a backend with awsm_hip_texture_array_write_layers: without it a flagged insert is
 * AWSM_ERR_UNSUPPORTED.  An image inserted after the array went to the device costs its own bytes and its own mip chain, not the array's. */
typedef struct AwsmHostTextureDesc {
    uint32_t struct_size;      /* sizeof(AwsmHostTextureDesc) */
    uint32_t mipmap_kind;
    uint32_t srgb_to_linear;   /* 0 / 1 */
    uint32_t premultiply_alpha;
} AwsmHostTextureDesc;
int awsm_host_texture_insert_ex(AwsmHost* h, const uint8_t* rgba8, uint32_t width, uint32_t height, const AwsmHostTextureDesc* desc);   /* texture id */
/* new pixels for an existing texture: same extent, same desc.  A frame already submitted (AWSM_CFG_OVERLAP_FRAMES) keeps the old ones. */
int awsm_host_texture_update(AwsmHost* h, int texture_id, const uint8_t* rgba8);
int awsm_host_sampler_insert(AwsmHost* h, const AwsmSampler* sampler);                                /* returns sampler id >= 0 */
AwsmKey awsm_host_texture_transform_insert(AwsmHost* h, const float offset[2], const float origin[2], float rotation, const float scale[2]);

/* ---- Materials (materials.rs:60-241, materials/pbr.rs, materials/unlit.rs) ---- */
typedef struct AwsmHostTexRef {
    int32_t texture;          /* texture id, -1 = none */
    uint32_t sampler;         /* sampler id */
    uint32_t uv_index;
    uint32_t pad;
    AwsmKey transform;        /* texture-transform key, 0 = identity */
} AwsmHostTexRef;

typedef struct AwsmHostMaterial {
    uint32_t struct_size;     /* sizeof(AwsmHostMaterial) as the caller was compiled */
    uint32_t shader;          /* 1 = PBR, 2 = unlit (MaterialShaderId) */
    uint32_t double_sided;
    float base_color_factor[4];
    float metallic_factor, roughness_factor, normal_scale, occlusion_strength;
    float emissive_factor[3];
    uint32_t debug_bitmask;
    AwsmHostTexRef base_color_tex, metallic_roughness_tex, normal_tex, occlusion_tex, emissive_tex;
    /* optional features: has_* selects whether the block is written (pbr.rs:364-573) */
    uint32_t has_vertex_color, vertex_color_set;
    uint32_t has_emissive_strength; float emissive_strength;
    uint32_t has_ior; float ior;
    uint32_t has_specular; float specular_factor; float specular_color_factor[3]; AwsmHostTexRef specular_tex, specular_color_tex;
    uint32_t has_transmission; float transmission_factor; AwsmHostTexRef transmission_tex;
    uint32_t has_volume; float volume_thickness_factor, volume_attenuation_distance; float volume_attenuation_color[3]; AwsmHostTexRef volume_thickness_tex;
    uint32_t has_clearcoat; float clearcoat_factor, clearcoat_roughness_factor, clearcoat_normal_scale;
    AwsmHostTexRef clearcoat_tex, clearcoat_roughness_tex, clearcoat_normal_tex;
    uint32_t has_sheen; float sheen_roughness_factor; float sheen_color_factor[3]; AwsmHostTexRef sheen_roughness_tex, sheen_color_tex;
    /* MaterialAlphaMode (materials.rs:255-273): 0 Opaque, 1 Mask { cutoff }, 2 Blend.  Mask, Blend and any transmission route the
     * meshes that use the material to the transparent pass (pbr.rs:213-224, unlit.rs:36-38; decided when the mesh is inserted,
     * as the glTF loader does: gltf/buffers/mesh.rs:33-57). */
    uint32_t alpha_mode; float alpha_cutoff;
    /* the remaining optional blocks of the word stream (pbr.rs:418-447,529-573): the reference's shaders do not read them yet and its
     * glTF mapper leaves them unset (gltf/populate/material.rs:621-625), but a material built through the API carries them, and the
     * Materials mirror must hold the same bytes */
    uint32_t has_diffuse_transmission; float diffuse_transmission_factor; float diffuse_transmission_color_factor[3];
    AwsmHostTexRef diffuse_transmission_tex, diffuse_transmission_color_tex;
    uint32_t has_dispersion; float dispersion;
    uint32_t has_anisotropy; float anisotropy_strength, anisotropy_rotation; AwsmHostTexRef anisotropy_tex;
    uint32_t has_iridescence; float iridescence_factor, iridescence_ior, iridescence_thickness_min, iridescence_thickness_max;
    AwsmHostTexRef iridescence_tex, iridescence_thickness_tex;
} AwsmHostMaterial;

AwsmKey awsm_host_material_insert(AwsmHost* h, const AwsmHostMaterial* m);
int awsm_host_material_update(AwsmHost* h, AwsmKey key, const AwsmHostMaterial* m);   /* AwsmRenderer::update_material */
int64_t awsm_host_material_offset(AwsmHost* h, AwsmKey key);

/* ---- Skins / morphs (meshes/skins.rs:84-194, meshes/morphs.rs:121-217) ---- */
AwsmKey awsm_host_skin_insert(AwsmHost* h, const AwsmKey* joint_transforms, uint32_t n_joints, const float* inverse_bind_mat4s,
                              uint32_t set_count, const uint32_t* const* joints_per_set, const float* const* weights_per_set, uint32_t vertex_count);

int64_t awsm_host_skin_matrices_offset(AwsmHost* h, AwsmKey skin);      /* Skins::joint_matrices_offset (skins.rs:146-152): byte offset of the skin's first matrix in AWSM_BUF_SKIN_MATRICES, -1 if absent */

/* ---- Meshes (meshes.rs:455-674; the gltf/buffers packers run inside) ---- */
typedef struct AwsmHostMorphTarget { const float* positions; const float* normals; const float* tangents; } AwsmHostMorphTarget;  /* each vertex_count*3 or NULL */
typedef struct AwsmHostPrimitive {
    uint32_t vertex_count, triangle_count;
    const float* positions;        /* vertex_count*3 */
    const float* normals;          /* vertex_count*3 */
    const float* tangents;         /* vertex_count*4 or NULL */
    const uint32_t* indices;       /* triangle_count*3 */
    uint32_t n_uv_sets; const float* uv_sets[8];        /* each vertex_count*2 */
    uint32_t n_color_sets; const float* color_sets[4];  /* each vertex_count*4 */
    uint32_t n_morph_targets; const AwsmHostMorphTarget* morph_targets;
    const float* morph_weights;            /* n_morph_targets (glTF mesh.weights) or NULL */
    const float* animated_morph_weights;   /* optional: written through update_morph_weights_with ([1..n+1)) */
    uint32_t front_face_cw;
} AwsmHostPrimitive;

AwsmKey awsm_host_mesh_insert(AwsmHost* h, const AwsmHostPrimitive* prim, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden);
/* Mesh.hud = true (meshes/mesh.rs:28; what the glTF loader's hints.hud sets): both geometries (gltf/buffers/mesh.rs:37-39), is_hud in the mesh's
 * MaterialMeshMeta, drawn by render() in the two HUD passes (render.rs:169-178,301-312) instead of the world's */
AwsmKey awsm_host_mesh_insert_hud(AwsmHost* h, const AwsmHostPrimitive* prim, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden);
int awsm_host_mesh_remove(AwsmHost* h, AwsmKey mesh);
/* Morphs::update_morph_weights_with (meshes/morphs.rs:197-217) with a callback that copies `weights`: floats [1, n + 1) of the mesh's block in
 * AWSM_BUF_MORPH_WEIGHTS (the reference's offset-by-one), uploaded with the next frame.  n must be the mesh's target count;
 * a mesh without morph targets and a wrong n are AWSM_ERR_INVALID_ARGUMENT. */
int awsm_host_mesh_update_morph_weights(AwsmHost* h, AwsmKey mesh, const float* weights, uint32_t n);

/* ---- Lights (lights.rs:160-310) ---- */
typedef struct AwsmHostLight {
    uint32_t kind;            /* 1 directional, 2 point, 3 spot */
    float color[3]; float intensity;
    float position[3]; float range;
    float direction[3]; float inner_angle, outer_angle;
} AwsmHostLight;
AwsmKey awsm_host_light_insert(AwsmHost* h, const AwsmHostLight* l);
int awsm_host_light_remove(AwsmHost* h, AwsmKey key);
int awsm_host_light_update(AwsmHost* h, AwsmKey key, const AwsmHostLight* l);      /* Lights::update (lights.rs:218-224): punctual_gpu_dirty, as insert */
int awsm_host_set_ibl_mip_counts(AwsmHost* h, uint32_t prefiltered, uint32_t irradiance);

/* ---- Camera (camera.rs:17-28,111-227): column-major mat4s ---- */
int awsm_host_camera_update(AwsmHost* h, const float view[16], const float projection[16], const float position_world[3]);

/* ---- environment pass-through + targets ---- */
int awsm_host_env(AwsmHost* h, const AwsmEnv* env);
/* Skybox / Ibl::{prefiltered_env, irradiance} set to a texel cubemap (crates/renderer/src/environment.rs:79-140, lights/ibl.rs:13-96): RGBA16F
 * [mip][face][y][x][4], faces +X -X +Y -Y +Z -Z; NULL = back to the colour.  The mip counts the shader scales roughness by are the ones of
 * awsm_host_set_ibl_mip_counts (lights.rs:300-305). */
int awsm_host_env_cube(AwsmHost* h, AwsmCube which, uint32_t size, uint32_t mips, const uint16_t* texels_rgba16f);
/* Environment cubes at run time: thin wrappers over awsm_hip_env_cube_create / _write_face / _write_all_faces / _generate_mips / _fill_colors /
 * _fill_sky_gradient (awsm_hip.h has the rules).  The reference's call sites: Skybox::new_colors / IblTexture::new_colors, CubemapImage::new_sky_gradient,
 * update_skybox_face / update_skybox_all_faces / update_cubemap_texture_face / _all_faces, regenerate_skybox_mipmaps / regenerate_cubemap_texture_mipmaps
 * (environment.rs, textures.rs:118-165).  The backend's symbols are optional: with a backend library that lacks one, the host still loads and the
 * call returns AWSM_ERR_UNSUPPORTED, naming the missing symbol.  None of these changes the IBL mip counts (awsm_host_set_ibl_mip_counts). */
int awsm_host_env_cube_create(AwsmHost* h, AwsmCube which, uint32_t size, uint32_t mips);
int awsm_host_env_cube_update_face(AwsmHost* h, AwsmCube which, uint32_t face, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                   const void* data, size_t data_len, const AwsmCubeLayout* layout);
int awsm_host_env_cube_update_all_faces(AwsmHost* h, AwsmCube which, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                        const void* data, size_t data_len, const AwsmCubeLayout* layout);
int awsm_host_env_cube_regenerate_mipmaps(AwsmHost* h, AwsmCube which);
int awsm_host_env_cube_colors(AwsmHost* h, AwsmCube which, uint32_t size, const float rgba[24]);
int awsm_host_env_cube_sky_gradient(AwsmHost* h, AwsmCube which, uint32_t size, const float zenith[4], const float nadir[4]);
/* Image-based lighting from the skybox: AWSM_CUBE_PREFILTERED becomes the GGX chain (prefiltered_size^2, prefiltered_mips levels) and
 * AWSM_CUBE_IRRADIANCE one level of irradiance_size^2, both filtered on the device from AWSM_CUBE_SKYBOX as it is at the call
 * (awsm_hip_env_cube_filter, twice; sample_count 0 = 1024), then awsm_host_set_ibl_mip_counts(prefiltered_mips, 1).  The skybox must be a texel cube
 * and should carry its mip chain (the fills and the KTX2 loader make one).  Call it again whenever the skybox changes.  AWSM_ERR_UNSUPPORTED, naming
 * the symbol, with a backend library that lacks awsm_hip_env_cube_filter. */
int awsm_host_env_bake_ibl(AwsmHost* h, uint32_t prefiltered_size, uint32_t prefiltered_mips, uint32_t irradiance_size, uint32_t sample_count);
/* KTX2 cube maps (renderer-core/src/cubemap/ktx.rs:39-147; the rules and their reasons are restated in host/ktx2.hpp).  Accepted vkFormats: 37, 43,
 * 44, 50 (RGBA8 / BGRA8, UNORM / SRGB), 97 (RGBA16F), 109 (RGBA32F), 122 (B10G11R11), 123 (E5B9G9R9); any other format — block-compressed and
 * depth formats among them — is AWSM_ERR_UNSUPPORTED with the vkFormat number in the message; every other rejection is AWSM_ERR_INVALID_ARGUMENT.
 * awsm_host_ktx2_parse is a pure function: no host, no device.  The loaders parse, create the cube with info.mips levels, write each stored
 * level with the tight layout, and — levelCount 0, "generate the chain" — make the other levels on the device.  The caller passes
 * info.mips to awsm_host_set_ibl_mip_counts, as it does for awsm_host_env_cube. */
typedef struct AwsmKtx2Level { uint64_t offset, length; } AwsmKtx2Level;
typedef struct AwsmKtx2Info {
    uint32_t struct_size;     /* IN: sizeof(AwsmKtx2Info) */
    uint32_t vk_format;       /* as stored */
    uint32_t format;          /* the AwsmCubeFormat it maps to */
    uint32_t size;            /* pixelWidth == pixelHeight */
    uint32_t faces, layers;   /* faceCount (6), layerCount (0) */
    uint32_t levels;          /* levels stored in the file: levelCount, or 1 when it is 0 */
    uint32_t mips;            /* levels of the cube made from it: levelCount, or the full chain when it is 0 */
    AwsmKtx2Level level[16];  /* byte range of each stored level, level 0 (the largest) first */
} AwsmKtx2Info;
int awsm_host_ktx2_parse(const uint8_t* data, size_t len, AwsmKtx2Info* out, char* err_out, size_t err_cap);
int awsm_host_env_cube_load_ktx2(AwsmHost* h, AwsmCube which, const char* path, AwsmKtx2Info* info_out, char* err_out, size_t err_cap);
int awsm_host_env_cube_load_ktx2_memory(AwsmHost* h, AwsmCube which, const uint8_t* data, size_t len, AwsmKtx2Info* info_out, char* err_out, size_t err_cap);
/* Radiance pictures (.hdr) and the skybox from an equirectangular panorama (host/rgbe.hpp has the reader's rules).
 * awsm_host_hdr_info and awsm_host_hdr_decode are pure functions: no host, no device.  The first line must start with "#?"; FORMAT=32-bit_rle_rgbe (or no
 * FORMAT line) is read, 32-bit_rle_xyze is AWSM_ERR_UNSUPPORTED; EXPOSURE= values are multiplied into `exposure` and NOT applied (pass 1 / exposure as
 * `scale` for radiance); "-Y H +X W" and "+Y H +X W" are read (flipped_y = 1 for the second: its rows are reversed, the output is always top-down),
 * any other orientation is AWSM_ERR_UNSUPPORTED; 1 <= W, H <= 32768 and W * H <= 2^28.  Flat scanlines, the old run pixels and the new run-length
 * coded planes are all read; every other rejection is AWSM_ERR_INVALID_ARGUMENT with the reason (a truncated scanline names its index).
 * awsm_host_hdr_decode writes width * height RGBE quadruples (4 bytes each) to rgbe_out, which must hold them (out_cap): AWSM_PANO_RGBE8 as it is.
 * awsm_host_env_cube_from_equirect is the thin wrapper over awsm_hip_env_cube_from_equirect (awsm_hip.h has the rules; AWSM_ERR_UNSUPPORTED, naming
 * the symbol, with a backend library that lacks it).  awsm_host_env_cube_load_hdr[_memory] decode the file, create the cube `size`^2 with its full
 * chain, project the panorama into level 0 (samples 0 = auto, yaw in radians, scale 0 = 1.0) and generate the mips.  None of them changes the IBL
 * mip counts; awsm_host_env_bake_ibl afterwards lights the scene from the new skybox. */
typedef struct AwsmHdrInfo { uint32_t struct_size, width, height, flipped_y, rle; float exposure; } AwsmHdrInfo;
int awsm_host_hdr_info(const uint8_t* data, size_t len, AwsmHdrInfo* out, char* err, size_t err_cap);
int awsm_host_hdr_decode(const uint8_t* data, size_t len, uint8_t* rgbe_out, size_t out_cap, AwsmHdrInfo* out, char* err, size_t err_cap);
int awsm_host_env_cube_from_equirect(AwsmHost* h, AwsmCube which, const void* data, size_t len, const AwsmEquirect* pano);
int awsm_host_env_cube_load_hdr(AwsmHost* h, AwsmCube which, const char* path, uint32_t size, uint32_t samples, float yaw, float scale, AwsmHdrInfo* info_out,
                                char* err, size_t err_cap);
int awsm_host_env_cube_load_hdr_memory(AwsmHost* h, AwsmCube which, const uint8_t* data, size_t len, uint32_t size, uint32_t samples, float yaw, float scale,
                                       AwsmHdrInfo* info_out, char* err, size_t err_cap);
int awsm_host_brdf_lut_generate(AwsmHost* h, uint32_t w, uint32_t height);
int awsm_host_resize(AwsmHost* h, uint32_t width, uint32_t height);
/* AwsmRenderer::set_anti_aliasing (anti_alias.rs:9-45): msaa_sample_count 0 (None) or 4 (recreates the render targets);
 * mipmap != 0 selects MipmapMode::Gradient in the opaque pass.  The reference's default is {Some(4), mipmap: true}. */
int awsm_host_set_anti_aliasing(AwsmHost* h, uint32_t msaa_sample_count, uint32_t mipmap);
/* AwsmRenderer::set_post_processing (post_process.rs: PostProcessing {tonemapping, bloom, dof}) with AntiAliasing.smaa (anti_alias.rs):
 * after this call awsm_host_render enqueues awsm_hip_post_pass after the last transparent pass (read the result with awsm_hip_read_display).
 * Off by default here; the reference's default is {KhronosNeutralPbr (1), bloom off, dof off}.  tonemapping: 0 None, 1 KhronosNeutralPbr,
 * 2 Aces.  AWSM_ERR_UNSUPPORTED when the backend library has no awsm_hip_post_pass, or when the host renders a shard of the frame
 * (awsm_host_set_shard_rows / _bands; those are refused the other way round while post-processing is on).  Calling it again replaces the
 * settings; awsm_host_clear_post_processing turns the post pass off again. */
int awsm_host_set_post_processing(AwsmHost* h, uint32_t tonemapping, int bloom, int dof, int smaa);
int awsm_host_clear_post_processing(AwsmHost* h);
/* The editor's ground grid (crates/editor/src/grid; the reference's editor draws it in its before_transparent_pass hook,
 * crates/frontend/src/pages/app/scene/editor.rs:87-99).  Here it is a built-in of the backend's transparent pass (awsm_hip_set_editor_grid in
 * awsm_hip.h has the rules): set it once at set-up.  With the grid on awsm_host_render runs the world transparent pass in every frame — with no draws
 * when the scene has no transparent or hud mesh — so the composite image is what the post pass and the caller read.  NULL turns it off again.
 * editor_grid_defaults fills the constants of grid.wgsl, to change a colour from.  AWSM_ERR_UNSUPPORTED, naming the symbol, when the backend library
 * lacks awsm_hip_set_editor_grid / awsm_hip_editor_grid_defaults; the backend's own refusals (a non-finite value, a bad struct_size) pass through. */
int awsm_host_editor_grid_defaults(AwsmHost* h, AwsmEditorGrid* out);
int awsm_host_set_editor_grid(AwsmHost* h, const AwsmEditorGrid* grid /* NULL = off */);
/* The editor's selection overlay (awsm_hip_set_selection in awsm_hip.h has the rules): an outline around the visible pixels of the selected meshes
 * and a wire box around each one's world AABB, drawn by the backend's world transparent pass.  The host remembers `mesh_keys` (as awsm_host_pick
 * reports them); every awsm_host_render hands the backend the key words of those that still exist and are neither hidden nor HUD, and one box per
 * such mesh that has a world AABB — the cull step's, as awsm_host_update_transforms left it — so the box follows a moved or animated transform with
 * nothing more to call.  Transparent meshes get a box (they have no visibility key to be outlined by).  A removed mesh drops out silently.  While
 * a selection is set awsm_host_render runs the world transparent pass in every frame, with no draws if need be.  NULL turns it off.
 * selection_defaults fills the backend's defaults, to change a field from.  AWSM_ERR_UNSUPPORTED, naming the symbol, when the backend library
 * lacks awsm_hip_set_selection / awsm_hip_selection_defaults; the backend's own refusals pass through and leave the selection as it was. */
int awsm_host_selection_defaults(AwsmHost* h, AwsmSelection* out);
int awsm_host_set_selection(AwsmHost* h, const AwsmSelection* selection /* NULL = off */, const uint64_t* mesh_keys, uint32_t n);
/* Screen-space ambient occlusion (awsm_hip_set_ssao in awsm_hip.h has the rules): a built-in of the backend's opaque pass, off until this is called;
 * the record is passed through unchanged and holds for every later awsm_host_render.  NULL turns it off again.  ssao_defaults fills the backend's
 * defaults, to change a field from.  AWSM_ERR_UNSUPPORTED, naming the symbol, when the backend library lacks awsm_hip_set_ssao /
 * awsm_hip_ssao_defaults; the backend's own refusals (a non-finite value, radius <= 0, strength outside [0, 1], a bad struct_size) pass through, and
 * so does its AWSM_ERR_UNSUPPORTED from the render of a sharded host. */
int awsm_host_ssao_defaults(AwsmHost* h, AwsmSsao* out);
int awsm_host_set_ssao(AwsmHost* h, const AwsmSsao* ssao /* NULL = off */);
/* Temporal anti-aliasing (awsm_hip_set_taa in awsm_hip.h has the resolve's rules): with it on, every awsm_host_render
 *   - jitters the projection as the reference's camera.rs does (Halton(2, 3) - 0.5 of the frame count the block carries, divided by the frame size
 *     and scaled by strength_still when view and projection equal the last render's within 1e-6 per element, else by strength_moving; the first
 *     frame counts as moved): proj' = translation(jitter_ndc) * proj, and uploads the 512-byte camera block packed from proj' — inv_proj,
 *     view_proj, inv_view_proj and the frustum rays are the jittered ones — in place of the block awsm_host_camera_update packed, which the host
 *     keeps: with TAA off again that block goes up as it was;
 *   - composes reproject = view_proj_previous * inverse(view_proj_current) from the unjittered f32 matrices, every operation in f64, rounded once
 *     to f32 — the exact identity when both matrices have the bits they had in the last render;
 *   - hands the backend that record (awsm_hip_set_taa) in front of its post pass, with AWSM_TAA_RESET in the first record after this call, after
 *     awsm_host_resize / awsm_host_set_anti_aliasing, and when the reprojection matrix is not finite.
 * It resolves in the post pass: while TAA is on and awsm_host_set_post_processing is not, awsm_host_render returns AWSM_ERR_INVALID_ARGUMENT and
 * says so.  NULL turns it off (the backend drops its history).  struct_size as for the backend's records: at least its own four bytes, at most
 * 4096, fields it does not reach keep their defaults (feedback 0.1, strength_still 0.8, strength_moving 0.2 — the reference's amplitudes).
 * AWSM_ERR_INVALID_ARGUMENT, the state unchanged, for a non-finite field or feedback outside (0, 1]; AWSM_ERR_UNSUPPORTED, naming the symbol, when
 * the backend library lacks awsm_hip_set_taa.  The limits are the backend's: no motion vectors for moved or animated meshes, unsharded hosts only.
 * awsm_host_taa_jitter returns the NDC offset a render with that frame count would use at the host's current size (moved != 0: the moving
 * strength); no device work. */
typedef struct AwsmHostTaa {
    uint32_t struct_size;
    float    feedback;          /* weight of the current frame, 0 < feedback <= 1 */
    float    strength_still;    /* jitter amplitude in pixels (full range) for an unchanged camera */
    float    strength_moving;   /* ... and for a camera that moved */
} AwsmHostTaa;
int awsm_host_set_taa(AwsmHost* h, const AwsmHostTaa* taa /* NULL = off */);
int awsm_host_taa_jitter(AwsmHost* h, uint32_t frame_count, int moved, float out_ndc[2]);

/* Shadows from one directional or spot light (awsm_hip_shadow_pass in awsm_hip.h has the device's rules).  While it is on,
 * awsm_host_render calls the backend's shadow pass after the geometry pass, every frame, with a camera it fits to the light and the casters it
 * chooses:
 *   light camera  composed in f64, packed as the scene camera's block is.  Forward f = the light's direction; up = +Y, or +Z when |f.y| > 0.999.
 *                 Directional: c, r = centre and half diagonal of the union of the world AABBs of the candidates (opaque, non-HUD, not hidden
 *                 meshes; none: c = 0, r = 1); eye = c - 2 r f; orthographic, half extent r both ways, near r, far 3 r.
 *                 Spot: eye = the position; perspective, aspect 1, fovy = clamp(2 acos(outer_angle), 1 deg, 170 deg) — outer_angle holds the cosine of the cone's half angle, as the shading reads it; far = range if range > 0, else
 *                 the distance to the farthest corner of that union (at least 1); near = max(0.05, far / 1000).
 *   casters       the candidates whose world AABB meets that camera's frustum, in the order the world list would hold them.  Transparent and
 *                 HUD meshes neither cast nor are looked up.
 * set_shadow(NULL) turns it off.  AWSM_ERR_UNSUPPORTED, naming the symbol, when the backend library lacks awsm_hip_shadow_pass /
 * awsm_hip_shadow_defaults, and for a point light when it lacks awsm_hip_shadow_pass_views (below); AWSM_ERR_INVALID_ARGUMENT for a key that names no light.  A light removed later turns the
 * feature off with AWSM_ERR_INVALID_ARGUMENT at the next awsm_host_render.  The record's other fields reach the backend unchanged, and its
 * refusals (and AWSM_ERR_UNSUPPORTED on a sharded host) come back from awsm_host_render.
 * shadow_camera: what the last awsm_host_render used — the 512-byte block, and up to `cap` caster draws (n_out: how many there were).
 * AWSM_ERR_NOT_READY when that render had no shadow pass. */
typedef struct AwsmHostShadow {
    uint32_t struct_size;
    AwsmKey light;            /* at byte 8 */
    uint32_t map_size;
    uint32_t pcf_radius;
    float bias, slope_bias, max_slope, strength, facing_fade;
} AwsmHostShadow;
int awsm_host_shadow_defaults(AwsmHost* h, AwsmHostShadow* out);      /* the backend's defaults; light = 0 */
int awsm_host_set_shadow(AwsmHost* h, const AwsmHostShadow* shadow /* NULL = off */);
int awsm_host_shadow_camera(AwsmHost* h, void* block512, AwsmDraw* casters_out, uint32_t cap, uint32_t* n_out);
/* Shadows from several views of the shadowed light (awsm_hip_shadow_pass_views), when the backend library has that entry.
 * A POINT light: set_shadow accepts it (AWSM_ERR_UNSUPPORTED, naming the symbol, over a backend without the entry).  Six views in the order
 *   +X, -X, +Y, -Y, +Z, -Z: eye = the light's position, forward = the axis, up by the rule above; perspective of aspect 1 with
 *   tan(fovy / 2) = S / (S - 2 (pcf_radius + 1)) — the 90-degree face lands on the layer's inner region, the rest is the apron the taps read —, near
 *   and far by the spot's rule.  map_size < 16: AWSM_ERR_INVALID_ARGUMENT at the render.  Casters per face by that face's frustum, in the world
 *   list's order; a face whose frustum meets no candidate is not sent (its pixels find no view and are lit); light = (position, 1).
 * CASCADES for a directional light: set_shadow_cascades {count 1 .. 4, lambda 0 .. 1, max_distance >= 0 (0: the camera's far)}; defaults 1, 0.5, 0.
 *   Spot and point lights ignore it; count = 1 is the single map above, call for call.  count = N > 1, with n, f the camera's near and far and
 *   f' = min(f, max_distance or f): split depths d_j = lambda n (f'/n)^(j/N) + (1 - lambda) (n + (f' - n) j/N); slice j's eight corners lie on the
 *   camera's corner rays at view depths d_j and d_j+1; c_j is their mean and r_j the largest distance from c_j to a corner times S / (S - 8) (2 at S <= 16: every
 *   corner then lies three texels inside the window after the snap below), rounded up to a multiple of 1/16.  Every cascade has the directional view matrix and the near = r, far = 3 r above (the scene's union: depth means the same in every
 *   layer) and the orthographic window [x - r_j, x + r_j] x [y - r_j, y + r_j], (x, y) = c_j in light space, each snapped down to a multiple of
 *   the texel 2 r_j / S.  Composed in f64.  Casters per view by its frustum; views are sent tightest first; beyond the last a pixel is lit.
 *   AWSM_ERR_UNSUPPORTED, naming the symbol, for count > 1 over a backend without the entry; AWSM_ERR_INVALID_ARGUMENT for the ranges.
 * shadow_view_count / shadow_view: what the last awsm_host_render sent — how many views, and view i's block and casters as shadow_camera hands out
 *   view 0's.  AWSM_ERR_NOT_READY when that render had no shadow pass; AWSM_ERR_INVALID_ARGUMENT for a view it did not have. */
typedef struct AwsmHostShadowCascades {
    uint32_t struct_size;
    uint32_t count;
    float lambda, max_distance;
} AwsmHostShadowCascades;
int awsm_host_shadow_cascades_defaults(AwsmHostShadowCascades* out);
int awsm_host_set_shadow_cascades(AwsmHost* h, const AwsmHostShadowCascades* cascades);
int awsm_host_shadow_view_count(AwsmHost* h, uint32_t* n_out);
int awsm_host_shadow_view(AwsmHost* h, uint32_t view, void* block512, AwsmDraw* casters_out, uint32_t cap, uint32_t* n_out);
/* CameraMatrices.focus_distance / .aperture (camera.rs:40-52; the reference's defaults are 10.0 and 5.6): camera bytes 496-503, uploaded with
 * the next frame.  Until this is called the host writes 0 and 0. */
int awsm_host_camera_set_dof(AwsmHost* h, float focus_distance, float aperture);
int awsm_host_set_shard_rows(AwsmHost* h, uint32_t y0, uint32_t y1);
/* GPU instancing (meshes.rs:176-290, instances.rs): n transforms of 10 floats each (translation xyz, rotation xyzw, scale xyz);
 * the first call enables instancing for the mesh (enable_mesh_instancing), later calls replace the list (set_mesh_instances);
 * append returns the index of the first appended instance (append_mesh_instances). */
int awsm_host_mesh_set_instances(AwsmHost* h, AwsmKey mesh, const float* trs10, uint32_t n);
int awsm_host_mesh_append_instances(AwsmHost* h, AwsmKey mesh, const float* trs10, uint32_t n);
/* AwsmRenderer::pick (picker.rs:55-121): *hit = 1 and *mesh_key = the MeshKey (KeyData::as_ffi) under pixel (x, y) of the last frame, else *hit = 0 */
int awsm_host_pick(AwsmHost* h, int32_t x, int32_t y, uint32_t* hit, uint64_t* mesh_key);
/* The same through the transparent passes of the last frame (awsm_hip_pick_ex in awsm_hip.h has the rule): transparent != 0 lets a fragment
 * that was blended with alpha >= alpha_threshold be hit.  *layer (may be NULL): 0 world opaque, 1 world transparent, 2 HUD opaque, 3 HUD
 * transparent.  awsm_host_pick_rect: the distinct (layer, MeshKey) pairs the rectangle [x0, x1) x [y0, y1) shows, with the pixels each holds, in
 * the backend's order; *n_out = how many there are, of which at most cap are written (layers and pixels may be NULL).
 * AWSM_ERR_INVALID_ARGUMENT for a threshold outside [0, 1] or a NULL keys with cap > 0; AWSM_ERR_UNSUPPORTED, naming the symbol, on a backend
 * library without awsm_hip_pick_ex / awsm_hip_pick_rect; the backend's own refusals otherwise. */
int awsm_host_pick_ex(AwsmHost* h, int32_t x, int32_t y, int transparent, float alpha_threshold, uint32_t* hit, uint64_t* mesh_key, uint32_t* layer);
int awsm_host_pick_rect(AwsmHost* h, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int transparent, float alpha_threshold, uint64_t* keys, uint32_t* layers,
                        uint32_t* pixels, uint32_t cap, uint32_t* n_out);
int awsm_host_set_shard_bands(AwsmHost* h, uint32_t n, uint32_t r, uint32_t compact_output);   /* awsm_hip_set_shard_bands */
/* AwsmRendererLogging.render_timings (debug.rs:8-12; the spans of render.rs:150-320): per-stage times in the frame stats, on by default;
 * off = awsm_hip_set_stage_timers(ctx, 0), the ms_* fields of the stats read 0 and the frame loses its event bubbles */
int awsm_host_set_render_timings(AwsmHost* h, int enabled);

/* ---- Animation (animation/{player,sampler,interpolate,data,clip,animations}.rs; host/animation.hpp has the rules, DESIGN.md section 15 the
 * quirks kept and the deviations).  A clip animates one path of one target. ---- */
enum { AWSM_ANIM_TRANSLATION = 0, AWSM_ANIM_ROTATION = 1, AWSM_ANIM_SCALE = 2, AWSM_ANIM_WEIGHTS = 3 };      /* path: width 3, 4, 3, the mesh's target count */
enum { AWSM_ANIM_LINEAR = 0, AWSM_ANIM_STEP = 1, AWSM_ANIM_CUBICSPLINE = 2 };                                  /* interpolation */
enum { AWSM_ANIM_LOOP_NONE = -1, AWSM_ANIM_LOOP = 0, AWSM_ANIM_PING_PONG = 1 };                                /* loop_style (Option<AnimationLoopStyle>) */
enum { AWSM_ANIM_FORWARD = 0, AWSM_ANIM_BACKWARD = 1 };                                                        /* direction */
enum { AWSM_ANIM_PLAYING = 0, AWSM_ANIM_PAUSED = 1, AWSM_ANIM_ENDED = 2 };                                     /* state */
typedef struct AwsmHostAnimationClip {
    uint32_t struct_size;      /* sizeof(AwsmHostAnimationClip) */
    uint32_t path, interpolation, n_keys, width;
    const double* times;       /* n_keys, ascending */
    const float* values;       /* n_keys * width */
    const float* in_tangents;  /* n_keys * width, AWSM_ANIM_CUBICSPLINE only */
    const float* out_tangents;
    double duration;           /* AnimationClip::duration; the glTF reader passes last key - first key (gltf/populate/animation.rs:107,229) */
} AwsmHostAnimationClip;
typedef struct AwsmHostAnimationState {
    uint32_t struct_size;      /* IN: sizeof(AwsmHostAnimationState) */
    int32_t direction, state, loop_style;
    double local_time, duration, speed;
} AwsmHostAnimationState;
/* Animations::insert_transform / insert_morph with AnimationPlayer::new(clip) (speed 1/1000, Loop, Forward, Playing, local time 0).  Returns the
 * AnimationKey, 0 on failure: no keys, a width other than the path's (the mesh's target count for weights), a path the target cannot take, an
 * unknown target.  The arrays are copied. */
AwsmKey awsm_host_animation_insert_transform(AwsmHost* h, const AwsmHostAnimationClip* clip, AwsmKey transform);
AwsmKey awsm_host_animation_insert_morph(AwsmHost* h, const AwsmHostAnimationClip* clip, AwsmKey mesh);
int awsm_host_animation_remove(AwsmHost* h, AwsmKey key);
/* the player's public fields (player.rs:8-15): speed, loop_style, play_direction, and its state */
int awsm_host_animation_set_playback(AwsmHost* h, AwsmKey key, double speed, int loop_style, int direction, int state);
int awsm_host_animation_seek(AwsmHost* h, AwsmKey key, double local_time);      /* a finite time; nothing is applied until the next update */
int awsm_host_animation_state(AwsmHost* h, AwsmKey key, AwsmHostAnimationState* out);
/* AnimationPlayer::sample: the value at the player's local time into out[0, width), nothing applied.  Returns the width, or a negative status
 * (cap < width: AWSM_ERR_OUT_OF_RANGE).  out = NULL asks for the width alone. */
int awsm_host_animation_sample(AwsmHost* h, AwsmKey key, float* out, uint32_t cap);
/* AwsmRenderer::update_animations (animations.rs:84-141): every player advances by global_time_delta * speed; then the transform players, in
 * key order, overwrite their component of the node's local transform (get_local -> apply -> set_local); then the morph players write their mesh's
 * weights (awsm_host_mesh_update_morph_weights).  Call it before awsm_host_update_transforms (update.rs:8-18). */
int awsm_host_update_animations(AwsmHost* h, double global_time_delta);

/* ---- Skin matrices composed on the device.  Off by default.  On: awsm_host_update_transforms no longer multiplies
 * world * inverse_bind for the joints that moved; it collects their record ids, and awsm_host_render, after it has uploaded AWSM_BUF_TRANSFORMS,
 * has the device compose them (awsm_hip_skin_pose) from the world matrices that are already there: 4 bytes per joint cross the bus instead of 64.
 * The result is byte-identical to the host's, and awsm_host_mirror(AWSM_BUF_SKIN_MATRICES) still returns it (composed on the CPU when asked).
 * AWSM_ERR_NOT_READY, naming the symbol, with a backend library that lacks awsm_hip_skin_pose_records_write or awsm_hip_skin_pose. ---- */
int awsm_host_set_device_skin_posing(AwsmHost* h, int on);
/* the record ids the last awsm_host_render handed to awsm_hip_skin_pose (sorted); n = their count */
int awsm_host_skin_pose_ids_last_frame(AwsmHost* h, uint32_t* out, uint32_t cap, uint32_t* n);

/* ---- frame: update_all (update.rs:8-18) + AwsmRenderer::render (render.rs:53-383, hot path only) ---- */
int awsm_host_update_transforms(AwsmHost* h);      /* after awsm_host_update_animations, before awsm_host_camera_update */
/* sync != 0: ends with awsm_hip_frame_end (stats filled if non-NULL); sync == 0: enqueue only */
int awsm_host_render(AwsmHost* h, int sync, AwsmFrameStats* stats);
/* RenderHooks (crates/renderer/src/render.rs:54-63,181-190: pre_render / after_geometry_pass / ...): callbacks render() makes between
 * its passes, on the calling thread, after the pass has been enqueued.  A multi-GPU caller uses them for the exchanges the passes of a
 * sharded frame need (MSAA + bands: the halo keys after the geometry pass; a sharded transparent pass: the opaque image after the opaque
 * pass).  A hook returning non-zero aborts the frame with that status.  NULL removes a hook. */
typedef int (*AwsmHostHook)(void* user);
int awsm_host_set_render_hooks(AwsmHost* h, AwsmHostHook after_geometry_pass, void* user_geometry, AwsmHostHook after_opaque_pass, void* user_opaque);

/* ---- introspection (tests, parity, INTEGRATION) ---- */
int awsm_host_mirror(AwsmHost* h, AwsmBuf which, const uint8_t** data, size_t* len);
/* ---- glTF ingest (crates/renderer/src/gltf/{loader,buffers,populate}.rs): reads a .gltf (external / data-URI buffers and images)
 * or a .glb, decodes the images (PNG), converts every accessor, generates missing normals / tangents, and populates this host
 * through the key API above in the reference's order (transforms, skins, meshes; populate.rs:185-205).  scene_index < 0 = the
 * document's default scene.  The camera is not taken from the file.  On failure returns a negative AwsmStatus and, if err_out is
 * given, the reason (AWSM_ERR_UNSUPPORTED for arithmetic-coded / 12-bit / CMYK JPEG and KTX2 images, sparse accessors, point / line primitives, unknown required
 * extensions); objects inserted before the failure stay inserted. ---- */
typedef struct AwsmGltfInfo {
    uint32_t nodes, meshes, materials, images, samplers, skins, lights, triangles, generated_tangents, instanced_meshes;
    /* the two words that were reserved (the struct carries no struct_size; its size and the fields before are unchanged): the players made from
     * animations[].channels, and the channels passed over — a path other than translation / rotation / scale / weights, an input or output that is
     * not a float accessor, a sampler without keys.  A second channel on a (node, path) is neither: the first one wins (populate.rs:229-268). */
    uint32_t animations, animation_channels_skipped;
} AwsmGltfInfo;
int awsm_host_load_gltf(AwsmHost* h, const char* path, int scene_index, AwsmGltfInfo* info_out, char* err_out, size_t err_cap);
/* The same with options.  AWSM_GLTF_SRGB_COLOR_TEXTURES: base colour, emissive, specular colour and sheen colour images are decoded from sRGB as
 * they enter the pool (material.rs:140,255,348,567); pool entries are then keyed by (texture index, colour info) as create_material_cache_key does
 * (material.rs:812-857), so an image used as colour and as data enters twice.  Without the flag: awsm_host_load_gltf. */
enum { AWSM_GLTF_SRGB_COLOR_TEXTURES = 1u };
typedef struct AwsmGltfOptions {
    uint32_t struct_size;      /* sizeof(AwsmGltfOptions) */
    int32_t scene_index;       /* < 0: the document's default scene */
    uint32_t flags;            /* AWSM_GLTF_* */
} AwsmGltfOptions;
int awsm_host_load_gltf_ex(AwsmHost* h, const char* path, const AwsmGltfOptions* options, AwsmGltfInfo* info_out, char* err_out, size_t err_cap);
/* the AnimationKeys of the players the last awsm_host_load_gltf[_ex] on this host made, in insertion order: per node (depth first) translation,
 * rotation, scale; then, as the meshes are inserted, one per primitive with targets of a node that has a weights channel.  *n = their count. */
int awsm_host_gltf_animation_keys(AwsmHost* h, AwsmKey* out, uint32_t cap, uint32_t* n);
/* the image decoders the reader uses (PNG: all colour types / bit depths, non-interlaced; JPEG: baseline / extended sequential Huffman,
 * 8-bit, grayscale or YCbCr) on their own: rgba_out = NULL queries the size; needs width * height * 4 bytes. */
int awsm_host_decode_image(const uint8_t* data, size_t len, uint8_t* rgba_out, size_t cap, uint32_t* width, uint32_t* height, char* err_out, size_t err_cap);

/* the world transparent pass's list (back to front), as awsm_host_draw_list gives the geometry pass's */
int awsm_host_transparent_draw_list(AwsmHost* h, AwsmDraw* out, uint32_t cap, uint32_t* n);
int awsm_host_draw_list(AwsmHost* h, AwsmDraw* out, uint32_t cap, uint32_t* n);   /* the list render() would submit */
/* the hud meshes (back to front) as the HUD geometry pass and the HUD transparent pass receive them: n entries in each array */
int awsm_host_hud_draw_lists(AwsmHost* h, AwsmDraw* geometry_out, AwsmDraw* transparent_out, uint32_t cap, uint32_t* n);
uint32_t awsm_host_texture_array_count(AwsmHost* h);
/* the pool's content: layers inserted with srgb_to_linear / premultiply_alpha are converted here, on the host, by the device's table and
 * integer rule, when this is first asked (tests and the oracle ask; rendering never does) */
int awsm_host_texture_array_info(AwsmHost* h, uint32_t array_idx, uint32_t* width, uint32_t* height, uint32_t* layers, const uint8_t** texels);
uint64_t awsm_host_upload_bytes_last_frame(AwsmHost* h);

/* ---- raw allocators for the restated reference unit tests ---- */
typedef struct AwsmHostDub AwsmHostDub;   /* DynamicUniformBuffer */
typedef struct AwsmHostDsb AwsmHostDsb;   /* DynamicStorageBuffer */
AwsmHostDub* awsm_host_dub_new(size_t initial_capacity, size_t byte_size, size_t aligned_slice_size /*0 = byte_size*/, uint8_t zero);
void awsm_host_dub_free(AwsmHostDub* b);
int awsm_host_dub_update(AwsmHostDub* b, AwsmKey key, const uint8_t* data, size_t len);          /* -1 if oversized */
int awsm_host_dub_update_offset(AwsmHostDub* b, AwsmKey key, size_t offset, const uint8_t* data, size_t len);
int awsm_host_dub_remove(AwsmHostDub* b, AwsmKey key);                                             /* 1 removed, 0 absent */
int64_t awsm_host_dub_offset(AwsmHostDub* b, AwsmKey key);                                         /* -1 absent */
int64_t awsm_host_dub_slot(AwsmHostDub* b, AwsmKey key);
size_t awsm_host_dub_size(AwsmHostDub* b);
size_t awsm_host_dub_len(AwsmHostDub* b);
size_t awsm_host_dub_capacity(AwsmHostDub* b);
size_t awsm_host_dub_next_slot(AwsmHostDub* b);
size_t awsm_host_dub_free_slots(AwsmHostDub* b, size_t* out, size_t cap);                          /* returns count */
const uint8_t* awsm_host_dub_raw(AwsmHostDub* b);
int64_t awsm_host_dub_take_resize(AwsmHostDub* b);                                                 /* -1 = None */
size_t awsm_host_dub_take_dirty(AwsmHostDub* b, size_t* out_pairs, size_t cap_pairs);
void awsm_host_dub_force_state(AwsmHostDub* b, size_t next_slot);                                  /* free_slots.clear(); next_slot = n */

AwsmHostDsb* awsm_host_dsb_new(size_t initial_bytes, uint8_t zero);
void awsm_host_dsb_free(AwsmHostDsb* b);
size_t awsm_host_dsb_update(AwsmHostDsb* b, AwsmKey key, const uint8_t* data, size_t len);         /* returns offset */
int awsm_host_dsb_patch(AwsmHostDsb* b, AwsmKey key, size_t at, const uint8_t* data, size_t len);  /* update_with_unchecked; -1 = missing key */
void awsm_host_dsb_remove(AwsmHostDsb* b, AwsmKey key);
int64_t awsm_host_dsb_offset(AwsmHostDsb* b, AwsmKey key);
int64_t awsm_host_dsb_size_of(AwsmHostDsb* b, AwsmKey key);
size_t awsm_host_dsb_used_size(AwsmHostDsb* b);
size_t awsm_host_dsb_len(AwsmHostDsb* b);
size_t awsm_host_dsb_capacity(AwsmHostDsb* b);
size_t awsm_host_dsb_tree_root(AwsmHostDsb* b);
const uint8_t* awsm_host_dsb_raw(AwsmHostDsb* b);
int64_t awsm_host_dsb_take_resize(AwsmHostDsb* b);
size_t awsm_host_dsb_take_dirty(AwsmHostDsb* b, size_t* out_pairs, size_t cap_pairs);
size_t awsm_host_round_pow2(size_t n);
size_t awsm_host_index_to_offset(size_t idx, size_t leaves);
size_t awsm_host_offset_to_index(size_t off, size_t leaves);
/* write_buffer_with_dirty_ranges plan: pairs in, pairs out; returns number of output pairs */
size_t awsm_host_write_plan(size_t raw_len, const size_t* in_pairs, size_t n_in, size_t* out_pairs, size_t cap_pairs);
/* Frustum::from_view_projection(...).intersects_aabb (frustum.rs:42-89) */
int awsm_host_frustum_intersects(const float view_projection[16], const float aabb_min[3], const float aabb_max[3]);
/* Aabb::transformed (bounds.rs:38-61) */
void awsm_host_aabb_transformed(const float mat4[16], const float aabb_min[3], const float aabb_max[3], float out_min[3], float out_max[3]);

#ifdef __cplusplus
}
#endif
#endif /* AWSM_HOST_H */
