/*
 * awsm_hip.h — C-ABI drop-in boundary for awsm-renderer's per-frame hot path on MI355X (gfx950).
 *
 * The reference (dakom/awsm-renderer, Rust -> wasm32 -> browser WebGPU) has no FFI/plugin interface;
 * its device seam is the Rust type `AwsmRendererWebGpu` (crates/renderer-core/src/renderer.rs:36-41)
 * and the ~10 methods the hot path calls on it.  Every entry point below replaces one of those call
 * sites for the Geometry Pass + Opaque Pass only.  Reference paths are relative to
 * /root/reference/.
 *
 * Conventions
 *   - plain C: opaque context pointer, plain pointers + sizes, no C++/torch types.
 *   - every function returns 0 (AWSM_OK) or a negative AwsmStatus; never aborts.  The text of the
 *     last failure on a context is available from awsm_hip_last_error().
 *     (reference: Result<_, AwsmCoreError>, crates/renderer-core/src/error.rs)
 *   - thread-compatible, not thread-safe: one ctx <-> one host thread <-> one HIP device + stream
 *     (the reference is single-threaded wasm).
 *   - no pointer handed across the boundary is retained after the call returns, except the
 *     optional externally-owned output image (awsm_hip_bind_output).
 *   - all byte offsets/sizes given to awsm_hip_buffer_write must be 4-byte aligned
 *     (crates/renderer/src/buffer/dynamic_storage.rs:196-211).
 */
#ifndef AWSM_HIP_H
#define AWSM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: AwsmFrameStats carries struct_size (the caller sets it; awsm_hip_frame_end writes no byte beyond it) and handoff_gate_timeouts;
 *    awsm_hip_frame_trace / awsm_hip_read_frame_trace; a timed-out hand-off gate drops its frame (fail closed) and is reported by
 *    awsm_hip_geometry_pass / awsm_hip_frame_flush as well.  A library and a caller of different versions refuse each other in awsm_hip_create. */
#define AWSM_HIP_ABI_VERSION 2u

typedef struct AwsmHipCtx AwsmHipCtx;

typedef enum AwsmStatus {
    AWSM_OK = 0,
    AWSM_ERR_INVALID_ARGUMENT = -1,
    AWSM_ERR_OUT_OF_MEMORY = -2,
    AWSM_ERR_DEVICE = -3,          /* a HIP runtime call failed (text in last_error) */
    AWSM_ERR_NO_DEVICE = -4,       /* no gfx950 device visible */
    AWSM_ERR_NOT_READY = -5,       /* a required buffer / size / env was never provided */
    AWSM_ERR_UNSUPPORTED = -6,     /* a combination this library does not implement; the message names it (awsm_hip_last_error) */
    AWSM_ERR_OUT_OF_RANGE = -7     /* an offset/size points outside the destination buffer */
} AwsmStatus;

/* Device buffers, one per CPU mirror the reference uploads.
 * The record layout of each is exactly the reference's; file:line of the writer is given. */
typedef enum AwsmBuf {
    AWSM_BUF_TRANSFORMS = 0,        /* mat4 col-major, stride 64          crates/renderer/src/transforms.rs:68-72,396-410 */
    AWSM_BUF_NORMAL_MATS = 1,       /* mat3, stride 36 (uploaded, unread) crates/renderer/src/transforms.rs:412-422 */
    AWSM_BUF_MATERIALS = 2,         /* u32 word stream per material       crates/renderer/src/materials/pbr.rs:258-589 */
    AWSM_BUF_LIGHTS = 3,            /* 64 B / light, dense                crates/renderer/src/lights.rs:354-473 */
    AWSM_BUF_LIGHTS_INFO = 4,       /* 16 B                                crates/renderer/src/lights.rs:293-305 */
    AWSM_BUF_CAMERA = 5,            /* 512 B                               crates/renderer/src/camera.rs:72-87,169-219 */
    AWSM_BUF_SKIN_MATRICES = 6,     /* mat4 / joint                        crates/renderer/src/meshes/skins.rs:162-194 */
    AWSM_BUF_SKIN_INDEX_WEIGHTS = 7,/* {u32 joint,f32 weight}x4 / set / vertex  crates/renderer/src/gltf/buffers/skin.rs:22-113 */
    AWSM_BUF_MORPH_WEIGHTS = 8,     /* f32 / target (+1 quirk)             crates/renderer/src/meshes/morphs.rs:148-217 */
    AWSM_BUF_MORPH_VALUES = 9,      /* 10 f32 / target / vertex            crates/renderer/src/gltf/buffers/morph.rs:31-190 */
    AWSM_BUF_GEOM_META = 10,        /* 40 B in 256-B slots                 crates/renderer/src/meshes/meta/geometry_meta.rs:44-113 */
    AWSM_BUF_MATERIAL_META = 11,    /* 68 B in 256-B slots                 crates/renderer/src/meshes/meta/material_meta.rs:96-185 */
    AWSM_BUF_VIS_GEOM_DATA = 12,    /* 56 B / exploded vertex              crates/renderer/src/gltf/buffers/mesh/visibility.rs:35-165 */
    AWSM_BUF_VIS_GEOM_INDEX = 13,   /* identity u32 (accepted, unread: redundant for a SW rasteriser) crates/renderer/src/meshes.rs:514-520 */
    AWSM_BUF_ATTR_DATA = 14,        /* interleaved f32 custom attributes   crates/renderer/src/gltf/buffers/attributes.rs:113-160 */
    AWSM_BUF_ATTR_INDEX = 15,       /* 3 x u32 / triangle                  crates/renderer/src/meshes.rs:434-446 */
    AWSM_BUF_TEXTURE_TRANSFORMS = 16,/* 32 B records                       crates/renderer/src/textures.rs:247-284 */
    AWSM_BUF_INSTANCES = 17,        /* mat4 / instance                       crates/renderer/src/instances.rs:30-57 */
    AWSM_BUF_TRANSPARENCY_GEOM_DATA = 18, /* 40 B / original vertex {pos, normal, tangent}, drawn through AWSM_BUF_ATTR_INDEX
                                       crates/renderer/src/gltf/buffers/mesh/transparency.rs:31-175, meshes.rs:1116-1125 */
    AWSM_BUF_COUNT = 19
} AwsmBuf;

/* Replaces AwsmRendererBuilder::build() (crates/renderer/src/lib.rs:213-259) for the two passes. */
typedef struct AwsmConfig {
    uint32_t struct_size;   /* sizeof(AwsmConfig), for forward compatibility */
    uint32_t abi_version;   /* AWSM_HIP_ABI_VERSION */
    int32_t  device;        /* HIP device ordinal */
    uint32_t flags;         /* AWSM_CFG_* */
    void*    stream;        /* hipStream_t to run on; NULL = the library creates its own */
} AwsmConfig;
#define AWSM_CFG_PARITY_TAP 1u   /* also keep the shaded RGBA in f32 (readable via awsm_hip_read_opaque_f32) */
#define AWSM_CFG_OVERLAP_FRAMES 4u /* pipelining across frames: the opaque pass runs on an internal stream and overlaps the NEXT frame's
                                     geometry pass (per-frame device state is double-buffered; a frame is shaded with the camera it was
                                     submitted with; any other scene write waits for the opaque passes in flight).  Work the caller
                                     enqueues on its own stream after a frame must be preceded by awsm_hip_frame_flush(); awsm_hip_frame_end
                                     and the read-back calls wait for everything. */
#define AWSM_CFG_GENERAL_SHADE_ONLY 8u /* never take the lean opaque route (k_shade_lean): every pixel through the general kernel.  For A/B
                                         measurements and for tests that compare the two routes; results must agree within the shading tolerance. */
#define AWSM_CFG_ANISOTROPIC 16u /* MipmapMode::Gradient honours AwsmSampler.max_anisotropy (gltf samplers ask for 16,
                                  * gltf/populate/material.rs:892-902): up to 17 weighted trilinear probes along the footprint's major axis,
                                  * the level chosen for rho_max / N (the contract: DESIGN.md §2, grad_footprint in shade_samplers.hpp).  Off by
                                  * default: textureSampleGrad's anisotropy is implementation-defined in WebGPU, and the default here is the
                                  * isotropic rule the reference itself documents (helpers/mipmap.wgsl:419-439).  Draws whose core textures
                                  * ask for anisotropy leave the lean opaque route under this flag. */
#define AWSM_CFG_SMALL_BIN_LIST 2u /* start with a 4096-entry (triangle, tile) list instead of sizing it from the triangle count:
                                     exercises the overflow -> grow -> replay path of awsm_hip_frame_end (tests) */

/* One geometry-pass draw == Mesh::push_geometry_pass_commands (crates/renderer/src/meshes/mesh.rs:70-126):
 * set_bind_group(2, meta, [geom_meta_off]); set_vertex_buffer(0, vis_data, vis_data_off);
 * draw_indexed(3*tri_count); cull mode from the pipeline key (mesh.rs:54-67).
 * Order of the array == the reference's sorted renderable order (crates/renderer/src/renderable.rs:38-150). */
typedef struct AwsmDraw {
    uint32_t geom_meta_off;   /* byte offset of the 256-B GeometryMeshMeta slot */
    uint32_t vis_data_off;    /* byte offset of the first exploded vertex in AWSM_BUF_VIS_GEOM_DATA (geometry pass), or of the mesh's
                                 first 40-byte vertex in AWSM_BUF_TRANSPARENCY_GEOM_DATA (transparent pass) */
    uint32_t tri_count;
    uint32_t flags;           /* AWSM_DRAW_* */
    uint32_t inst_off;        /* instanced mesh: byte offset of its first mat4 in AWSM_BUF_INSTANCES (meshes/mesh.rs:91-121) */
    uint32_t inst_count;      /* instanced mesh: instance count; 0 = not instanced */
} AwsmDraw;
#define AWSM_DRAW_CULL_BACK 1u   /* CullMode::Back (single-sided); 0 = CullMode::None */

/* MaterialOpaqueRenderPass::render (crates/renderer/src/render_passes/material_opaque/render_pass.rs:47-96). */
typedef struct AwsmOpaqueParams {
    uint32_t mipmap;        /* MipmapMode: 0 = None (textureSampleLevel 0), 1 = Gradient (textureSampleGrad from the barycentric derivatives; the
                               arrays must hold their mip chain: awsm_hip_texture_array_generate_mips) */
    uint32_t has_opaque;    /* 0 -> the "empty" pipeline: skybox only (render_pass.rs:64-71) */
} AwsmOpaqueParams;

typedef enum AwsmTexFormat { AWSM_TEX_RGBA8_UNORM = 0 } AwsmTexFormat;

/* GPUSamplerDescriptor subset used by the texture pool (crates/renderer/src/materials/writer.rs:53-63). */
typedef struct AwsmSampler {
    uint32_t address_mode_u;  /* 0 clamp-to-edge, 1 repeat, 2 mirror-repeat */
    uint32_t address_mode_v;
    uint32_t mag_filter;      /* 0 nearest, 1 linear (level-0 sampling uses the mag filter) */
    uint32_t min_filter;
    uint32_t mipmap_filter;
    uint32_t max_anisotropy;  /* 1..16; counts under MipmapMode::Gradient on a context created with AWSM_CFG_ANISOTROPIC, and only with three linear filters */
} AwsmSampler;

/* Environment: skybox + IBL cubes + BRDF LUT (opaque bind group 0, bindings 14-21:
 * crates/renderer/src/render_passes/material_opaque/shader/material_opaque_wgsl/bind_groups.wgsl:22-29).
 * The three colours are the uniform cubes AwsmRendererBuilder creates by default (crates/renderer/src/lib.rs:176-207);
 * texel cubemaps go through awsm_hip_env_cube_upload. */
typedef struct AwsmEnv {
    float skybox_rgba[4];
    float prefiltered_rgb[4];
    float irradiance_rgb[4];
    uint32_t brdf_lut_width, brdf_lut_height;
    const uint16_t* brdf_lut_rgba16f;  /* width*height*4 halfs, row 0 first; NULL = keep the current LUT */
} AwsmEnv;

typedef struct AwsmFrameStats {
    uint32_t struct_size; /* IN: sizeof(AwsmFrameStats) as the caller was compiled (fields are only ever appended); OUT: bytes written */
    float ms_transform;   /* k_deform_transform */
    float ms_bin;         /* k_bin_count + scan + k_bin_fill */
    float ms_raster;      /* k_raster_tile */
    float ms_shade;       /* k_shade; with SSAO on (awsm_hip_set_ssao) k_ssao_ao + k_ssao_apply too */
    float ms_total;       /* first kernel start -> last kernel end */
    uint32_t triangles_in;      /* sum of tri_count over draws */
    uint32_t triangles_binned;  /* survived cull */
    uint32_t bin_entries;       /* (triangle, tile) pairs */
    uint32_t covered_pixels;    /* pixels with a hit (inside the shard rect) */
    uint32_t bin_overflow_retries;
    float ms_forward;           /* transparent pass: transform + binning + k_forward_tile */
    uint32_t forward_triangles; /* sum of tri_count (x instances) over the transparent draws */
    uint32_t forward_fragment_slots; /* fragment-list slots the transparent pass used (fragments + the unused tails of the wavefronts' chunks) */
    float ms_shade_lean;          /* k_shade_lean alone when the opaque pass took the lean route (then ms_shade = this + k_shade_todo), else 0; with SSAO on the two SSAO kernels are in ms_shade as well */
    uint32_t shade_general_wavefronts; /* 16x4-pixel groups of the last opaque pass that went through the general kernel instead of the lean one */
    uint32_t frames_with_dropped_bin_entries; /* enqueue-only frames (no frame_end) whose (triangle, tile) list overflowed since the context was created:
                                         such a frame lost geometry.  The library sizes the list from the need the GPU reports for earlier
                                         frames (growing it ahead of the need), so this stays 0 unless the need jumps by more than a third
                                         between two frames; awsm_hip_frame_end additionally replays an overflowed frame. */
    uint32_t handoff_gate_timeouts;  /* AWSM_CFG_OVERLAP_FRAMES with device-side hand-off: gates that ran out of time since the context was created.  Each one
                                         dropped the frame it guarded whole (its kernels exit at once: the image is not written, nothing is shaded from
                                         half-written buffers) and was reported once with AWSM_ERR_DEVICE. */
    uint32_t geometry_cache_blocks;  /* k_deform_transform workgroups (256 exploded vertices of one draw each) of this frame's geometry pass that kept the frame
                                         slot's cached world positions / normals / tangents / per-triangle words and only formed clip = view_proj * world,
                                         because their draw sits where it sat in the slot's previous frame and nothing it reads but the camera was written
                                         since (awsm_hip_buffer_write / buffer_create ranges).  Counted only while stage timers are on. */
    uint32_t geometry_blocks;        /* ... out of this many */
} AwsmFrameStats;

/* ---- lifecycle: AwsmRendererBuilder::build() / Drop (crates/renderer/src/meshes.rs:1349-1357) ---- */
int awsm_hip_create(const AwsmConfig* cfg, AwsmHipCtx** out);
int awsm_hip_destroy(AwsmHipCtx* ctx);
const char* awsm_hip_last_error(const AwsmHipCtx* ctx);
uint32_t awsm_hip_abi_version(void);

/* ---- gpu.create_buffer(desc{size,..}) (crates/renderer-core/src/methods.rs:239; callers e.g.
 * crates/renderer/src/meshes.rs:1313-1322): the new buffer replaces the old wholesale, contents are NOT
 * preserved — the host re-uploads the full mirror right after.  Idempotent for an unchanged size. ---- */
int awsm_hip_buffer_create(AwsmHipCtx* ctx, AwsmBuf which, size_t bytes);

/* ---- gpu.write_buffer(buf, Some(offset), &raw[off..off+len]) (crates/renderer-core/src/methods.rs:339-431,
 * via write_buffer_with_dirty_ranges, crates/renderer/src/buffer/helpers.rs:170-193).  Ordered before the
 * next pass on the ctx stream; `src` is copied to a pinned staging ring before the call returns. ---- */
int awsm_hip_buffer_write(AwsmHipCtx* ctx, AwsmBuf which, size_t dst_off, const void* src, size_t len);

/* ---- render_textures.views() realloc on size/AA change (crates/renderer/src/render_textures.rs:103-147).
 * msaa: 0 (or 1) = single sample; 4 = the reference's default AntiAliasing (anti_alias.rs:28-38): the geometry pass keeps
 * four visibility samples per pixel at WebGPU's standard 4x positions (per-sample coverage and depth; the interpolants
 * are evaluated at the pixel centre, as @interpolate(perspective, center) does), and the opaque pass runs the edge
 * detector + per-sample resolve of material_opaque_wgsl/helpers/{msaa,material_shading}.wgsl.  The output image stays
 * single-sampled.  Sharding with MSAA: row strips (awsm_hip_set_shard_rows; one halo row each side is rasterised for the
 * edge detector), or bands with the halo exchange below. ---- */
int awsm_hip_resize(AwsmHipCtx* ctx, uint32_t width, uint32_t height, uint32_t msaa);

/* ---- multi-GPU screen sharding (new; no reference counterpart): this ctx rasterises and shades only
 * pixel rows [y0, y1) (full width).  y0 == y1 == 0 restores the full frame.  Any row boundary is allowed: tiles that
 * straddle it are clipped per pixel, so a shard's rows are bit-identical to the same rows of the full frame. ---- */
int awsm_hip_set_shard_rows(AwsmHipCtx* ctx, uint32_t y0, uint32_t y1);

/* Interleaved sharding for load balance (no reference counterpart): this context rasterises and shades the
 * 32-row tile rows ty with ty % n == r (n = 1 restores the full frame; replaces any set_shard_rows range).  Work per
 * shard is then proportional to 1/n wherever the expensive part of the screen lies.  With compact_output != 0 the
 * opaque image is written densely: output row = (ty / n) * 32 + (y & 31), ceil((ceil(H/32) - r) / n) * 32 rows — the
 * layout an all-gather wants; otherwise rows keep their absolute position.  The visibility buffer is always
 * addressed by absolute row.  Rows owned by a shard are bit-identical to the same rows of the unsharded frame. */
int awsm_hip_set_shard_bands(AwsmHipCtx* ctx, uint32_t n, uint32_t r, uint32_t compact_output);
/* MSAA x4 with band sharding.  The edge detector (helpers/msaa.wgsl:42-112) compares a pixel with sample 0 of its four neighbours; for the
 * first and last row of a band the vertical neighbour lies in a band another rank rasterised.  So the frame gets ONE exchange step:
 * after the geometry pass every rank exports the sample-0 keys of the first and last row of each of its bands
 * (awsm_hip_msaa_halo_export: awsm_hip_msaa_halo_bands() x 2 x width u64, enqueued on the context's stream), the ranks all-gather those
 * arrays in rank order (RCCL), and every rank binds the gathered [n][bands][2][width] array before its opaque pass
 * (awsm_hip_msaa_halo_bind; kept by reference).  Every rank holds every triangle's setup record and vertex normals (the scene is
 * replicated, vertices are transformed redundantly), so a key is all a neighbour needs.  Without a bound array the opaque pass of an
 * MSAA band shard fails with AWSM_ERR_NOT_READY. */
uint32_t awsm_hip_msaa_halo_bands(AwsmHipCtx* ctx);     /* ceil(ceil(height / 32) / n): bands per rank in both arrays */
int awsm_hip_msaa_halo_export(AwsmHipCtx* ctx, void* dst_device, size_t bytes);
int awsm_hip_msaa_halo_bind(AwsmHipCtx* ctx, const void* gathered_device, size_t bytes);

/* ---- texture pool bind (crates/renderer/src/render_passes/material_opaque/bind_group.rs:331-360):
 * array `array_idx` is a texture_2d_array of `layers` w x h images; texels = layers*h*w*4 bytes, layer-major: mip
 * level 0 (what copyExternalImageToTexture writes, renderer-core/src/texture/texture_pool.rs:252-300).  `mips` = number
 * of levels the array holds (1, or up to floor(log2(max(w,h))) + 1): the space is reserved here and levels >= 1 are
 * produced by awsm_hip_texture_array_generate_mips. ---- */
int awsm_hip_texture_array_upload(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t width, uint32_t height,
                                  uint32_t layers, uint32_t mips, AwsmTexFormat fmt, const void* texels);
/* generate_mipmaps (renderer-core/src/texture/mipmap.rs:95-330): every level from the previous one, 2x2 texels, filter
 * chosen per layer by MipmapTextureKind (0 albedo, 1 normal: renormalised, 2 metallic-roughness: roughness averaged as
 * r^2, 3 occlusion, 4 emissive, 5.. = box filter); kind_per_layer = `layers` values or NULL (all albedo).  Results are
 * stored as RGBA8 (floor(clamp(v,0,1)*255 + 0.5)). */
int awsm_hip_texture_array_generate_mips(AwsmHipCtx* ctx, uint32_t array_idx, const uint32_t* kind_per_layer);
/* texels of one mip level back to the host (tests): layers*h_l*w_l*4 bytes */
int awsm_hip_texture_array_read_level(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t level, void* texels_out);
int awsm_hip_sampler_set(AwsmHipCtx* ctx, uint32_t sampler_idx, const AwsmSampler* sampler);
int awsm_hip_env_upload(AwsmHipCtx* ctx, const AwsmEnv* env);
/* Texel cubemaps for the same three bindings (skybox_tex, ibl_filtered_env_tex, ibl_irradiance_tex: bind_groups.wgsl:22-27; sampled by
 * helpers/skybox.wgsl:37 and shared_wgsl/lighting/brdf.wgsl:268-290 with the linear / linear / linear clamp samplers of lights/ibl.rs:38-47).
 * texels: RGBA16F, [mip][face][y][x][4 halfs], mip m has extent max(size >> m, 1), faces in layer order +X -X +Y -Y +Z -Z (what
 * CubemapImage::create_texture_and_view uploads; decoding KTX2 / EXR files is the caller's business).  mips = levels present (>= 1).
 * texels == NULL returns the binding to the uniform colour of awsm_hip_env_upload.  The prefiltered lookup's level is
 * roughness * (IblInfo.prefiltered_env_mip_count - 1) with the count the host wrote into AWSM_BUF_LIGHTS_INFO, clamped to the chain. */
typedef enum AwsmCube { AWSM_CUBE_SKYBOX = 0, AWSM_CUBE_PREFILTERED = 1, AWSM_CUBE_IRRADIANCE = 2 } AwsmCube;
int awsm_hip_env_cube_upload(AwsmHipCtx* ctx, AwsmCube which, uint32_t size, uint32_t mips, const uint16_t* texels_rgba16f);

/* ---- BrdfLut::new (crates/renderer-core/src/brdf_lut/generate.rs:47-96 + shader.wgsl): renders the
 * split-sum LUT on the device into the ctx's LUT slot (RGBA16F semantics, RG kept). ---- */
int awsm_hip_brdf_lut_generate(AwsmHipCtx* ctx, uint32_t width, uint32_t height);
int awsm_hip_read_brdf_lut(AwsmHipCtx* ctx, uint16_t* rg16f_out /* width*height*2 halfs */);

/* ---- GeometryRenderPass::render (crates/renderer/src/render_passes/geometry/render_pass.rs:51-157):
 * clear (vis = "no hit", depth = 1.0) + one draw per entry, depth LessEqual, later primitive wins ties. ---- */
int awsm_hip_geometry_pass(AwsmHipCtx* ctx, const AwsmDraw* draws, uint32_t n_draws);

/* ---- render_textures.clear_opaque() + MaterialOpaqueRenderPass::render
 * (crates/renderer/src/render.rs:209,219-221): one dispatch over the screen. ---- */
int awsm_hip_opaque_pass(AwsmHipCtx* ctx, const AwsmOpaqueParams* params);

/* ---- opaque -> transparent blit + MaterialTransparentRenderPass::render(.., is_hud = false) (+ the MSAA resolve into `composite`)
 * (crates/renderer/src/render.rs:224-297, render_passes/material_transparent/{render_pass,pipeline}.rs,
 * material_transparent_wgsl/{vertex,fragment}.wgsl).  `draws` = the transparent renderables in the reference's order (grouped by
 * pipeline, then back to front: renderable.rs:90,131-135); each mesh's 40-byte vertices (AWSM_BUF_TRANSPARENCY_GEOM_DATA at
 * vis_data_off) are drawn through its custom-attribute indices.  Forward shading per fragment with the premultiplied "over" blend
 * (One / OneMinusSrcAlpha), depth test LessEqual against the geometry pass's depth, depth write, screen-space transmission from
 * the opaque image.  Call after awsm_hip_opaque_pass of the same frame (it uses that call's mipmap mode and the context's MSAA
 * mode).  The result is the `composite` image (awsm_hip_read_composite / awsm_hip_bind_composite); the opaque image is
 * unchanged.  n_draws = 0 is valid (composite = opaque).
 * On a sharded context (row strip or bands) the pass covers, shades and blends this shard's rows only, but screen-space transmission
 * reads the WHOLE opaque image: gather the ranks' opaque rows first and hand the full [height][width] RGBA16F image in with
 * awsm_hip_bind_opaque_source (without it: AWSM_ERR_UNSUPPORTED).  The composite is addressed by absolute row (full-size target),
 * whatever layout the opaque output has.
 * Overflow of the pass's own lists (its (triangle, tile) list, the fragment slots) is detected and replayed by awsm_hip_frame_end only: a
 * pipelined loop that never calls frame_end must call it at least once after the transparent workload changes size (the lists then stay
 * sized for it), or check AwsmFrameStats.bin_overflow_retries from time to time — an overflowed enqueue-only frame drops fragments. ---- */
int awsm_hip_transparent_pass(AwsmHipCtx* ctx, const AwsmDraw* draws, uint32_t n_draws);
/* ---- the HUD passes (crates/renderer/src/render.rs:169-178,301-312; Mesh.hud, MaterialMeshMeta.is_hud):
 *   awsm_hip_hud_geometry_pass    GeometryRenderPass::render(ctx, &renderables.hud, true) — between awsm_hip_geometry_pass and awsm_hip_opaque_pass.  The
 *                                 hud meshes' visibility geometry (draws as in awsm_hip_geometry_pass) is rasterised over the visibility targets with a
 *                                 depth buffer of its own, cleared (geometry/render_pass.rs:51-157 with is_hud): they hide the world whatever its depth.
 *                                 The opaque pass then leaves every pixel a hud mesh covers cleared, (0, 0, 0, 0) (compute.wgsl:176-179), and
 *                                 awsm_hip_pick reports the hud mesh.  The world's keys and depth are not touched (the world transparent pass tests
 *                                 against them, as the reference's does against `depth`).
 *   awsm_hip_hud_transparent_pass MaterialTransparentRenderPass::render(ctx, renderables.hud, true) — after awsm_hip_transparent_pass (call that with
 *                                 n_draws = 0 when the frame has no world-transparent mesh).  The hud meshes' transparency geometry, back to front,
 *                                 forward-shaded and blended over the composite (colour LoadOp::Load), depth-tested against hud_depth, cleared
 *                                 (render.rs:490-521).  A hud mesh carries both geometries (gltf/buffers/mesh.rs:33-39).
 * With MSAA x4 (the reference's default AntiAliasing) the reference's quirk is reproduced, because its own opaque pass reads it: the HUD geometry pass
 * draws over the multisampled visibility / barycentric / normal targets but tests and writes hud_depth, so a covered sample shows the hud triangle and
 * still the WORLD's depth.  A pixel whose sample 0 is a hud triangle stays cleared; elsewhere the edge detector sees hud normals beside world depths
 * and msaa_resolve_samples shades hud samples like any other (compute.wgsl:176-180: "this may bleed a little").  Internally the hud draws then share the
 * world pass's rank space and the opaque pass reads merged keys (hud rank under world depth); awsm_hip_read_visibility still returns the world's.
 * Sharded contexts (row strips, bands) rasterise and shade their own rows of the hud meshes; the two transparent passes need the gathered opaque
 * image as usual (awsm_hip_bind_opaque_source).  MSAA with BAND sharding: the halo keys exported after this pass are the merged ones. ---- */
int awsm_hip_hud_geometry_pass(AwsmHipCtx* ctx, const AwsmDraw* draws, uint32_t n_draws);
int awsm_hip_hud_transparent_pass(AwsmHipCtx* ctx, const AwsmDraw* draws, uint32_t n_draws);
/* the full-frame opaque image the transparent pass of a sharded context blits from and refracts through (device memory, width*height*8
 * bytes, kept by reference until replaced; NULL = this context's own opaque output, which is complete only when unsharded) */
int awsm_hip_bind_opaque_source(AwsmHipCtx* ctx, const void* device_ptr, size_t bytes);

/* ---- gpu.submit_commands(encoder.finish()) (crates/renderer/src/render.rs:370): waits for the frame,
 * fills per-kernel times.  `out` may be NULL. ---- */
int awsm_hip_frame_end(AwsmHipCtx* ctx, AwsmFrameStats* out);

/* Stage timers: by default every frame records HIP events between its stages so that awsm_hip_frame_end can report
 * AwsmFrameStats.ms_*.  Each record costs a ~5 us bubble between two kernels; a render loop that does not read the stage times
 * turns them off (the ms_* fields then read 0; counters are unaffected).  No reference counterpart (the reference's timings are
 * tracing spans around command encoding, render.rs:150-320). */
int awsm_hip_set_stage_timers(AwsmHipCtx* ctx, int enabled);

/* Frame trace (measurement aid; the reference's counterpart are the tracing spans of render.rs:150-320): with capacity > 0 every frame
 * leaves three device-clock stamps in a ring of `capacity` frames — geometry pass begins, geometry pass done, shading (+ transparent pass)
 * done — written in stream order by one-lane kernels (the hand-off's own signal kernels where the pipeline has them: no extra launch on
 * the critical path).  capacity = 0 turns it off.  read_frame_trace synchronises and returns the last n_frames frames, oldest first, as
 * ticks_out[n_frames][3] in ticks of the constant-rate device clock (ticks_per_ms_out), plus the serial number of the newest frame. */
int awsm_hip_frame_trace(AwsmHipCtx* ctx, uint32_t capacity);
int awsm_hip_read_frame_trace(AwsmHipCtx* ctx, uint64_t* ticks_out, uint32_t n_frames, uint32_t* last_serial_out, uint32_t* ticks_per_ms_out);

/* ---- frame loop without a host sync (bench / multi-frame pipelines): enqueue only. ---- */
int awsm_hip_frame_flush(AwsmHipCtx* ctx);

/* ---- output image: RGBA16F, row-major, width*height*8 bytes == the reference's `opaque` render
 * texture (crates/renderer/src/render_textures.rs:49-54).  bind_output lets the caller own the memory
 * (e.g. a torch tensor that RCCL all-gathers); NULL returns to the internal image.  `bytes` must cover what the
 * current shard layout writes: width*height*8, or bands*32*width*8 with awsm_hip_set_shard_bands(compact_output);
 * checked when the opaque pass is enqueued. ---- */
int awsm_hip_bind_output(AwsmHipCtx* ctx, void* device_ptr, size_t bytes);
/* The same for a row-strip shard (awsm_hip_set_shard_rows): device_ptr is where frame row `first_row` goes and `bytes` covers the rows from
 * there on (width*8 each); the shard's rows must lie inside.  Lets a rank hand in its [rows, width] strip of an all-gather buffer. */
int awsm_hip_bind_output_rows(AwsmHipCtx* ctx, void* device_ptr, size_t bytes, uint32_t first_row);
/* the image the last submitted frame's opaque pass writes (the bound one, else the library's; with AWSM_CFG_OVERLAP_FRAMES the library keeps
 * one image per frame slot, so the pointer alternates from frame to frame) */
void* awsm_hip_output_device_ptr(AwsmHipCtx* ctx);

/* ---- readback for parity (new).  keys: width*height u64 (x4 with MSAA: the samples of a pixel are adjacent) =
 * (depth_f32_bits << 32) | (0xFFFFFFFF - rank),
 * rank = index of the triangle in draw order over the whole draw list; all ones = no hit.
 * unpack gives the reference's visibility_data texel: triangle_index (primitive-local) and
 * material_mesh_meta_offset, plus the Depth32Float value.
 * "Bit-exact" for these keys means: bit-exact to the arithmetic contract of DESIGN.md section 3, which this repository defines where WebGPU leaves the
 * implementation free — vertex snapping to 1/256 pixel, the top-left rule, the operation order of the depth interpolation, and the depth of an MSAA sample
 * (the plane's value at the pixel's corner plus the sample's step: a rule CHANGED IN ROUND 4 FOR SPEED, oracle first, kernel second; within 1.25 f32 steps
 * of the plane in f64).  The CPU oracle (oracle/) implements the same contract without shared code and the GPU tests compare every key.  What the
 * reference's own tests pin are the buffer allocators, the dirty-range writer and the frustum — not these keys. ---- */
int awsm_hip_read_visibility(AwsmHipCtx* ctx, uint64_t* keys_out);
/* 128-bit position-dependent digest of the keys the last geometry pass left (the caller's stream; synchronous):
 * out2[0] = sum key_i * (2 i + 1) mod 2^64, out2[1] = xor rotl(key_i, i mod 64).  For tests that compare many frames
 * without reading 8 bytes per pixel back. */
int awsm_hip_visibility_digest(AwsmHipCtx* ctx, uint64_t* out2);
/* AWSM_CFG_OVERLAP_FRAMES: how the context orders its streams at the two hand-offs on a frame's critical path (geometry pass -> opaque pass of
 * the same frame; opaque pass -> the geometry pass that reuses its frame slot).  1 = device-side flags (a one-lane kernel at the end of the
 * producer stream stores the frame's serial number, a one-lane kernel at the head of the consumer stream polls it: ~2 us instead of the
 * 20-30 us a cross-stream hipEvent takes to release the waiting queue), 0 = hipEvents (contexts without overlap; AWSM_DEVICE_HANDOFF=0 in
 * the environment; the probe at create found that kernels of two streams do not run side by side, e.g. under a counter-collecting
 * profiler; or a gate timed out later, which awsm_hip_frame_end reports once with AWSM_ERR_DEVICE).  Negative = AWSM_ERR_*.
 * A gate that runs out of time fails closed: the frame it guarded is dropped whole (every kernel of it exits at its first instruction, its image
 * is not written), the streams go on, the context falls back to events, and the next awsm_hip_geometry_pass / awsm_hip_frame_flush /
 * awsm_hip_frame_end returns AWSM_ERR_DEVICE once (AwsmFrameStats.handoff_gate_timeouts counts them).
 * Environment, read at create: AWSM_DEVICE_HANDOFF=0 (events from the start), AWSM_HANDOFF_TIMEOUT_MS=x (a gate's time budget on the device clock,
 * default 4000), AWSM_TEST_HANDOFF_DROP=n (tests: withhold the first n geometry-done signals to exercise the timeout path). */
int awsm_hip_stream_handoff(AwsmHipCtx* ctx);
/* test aid: the G-buffer texel fs_main would have written for every pixel of the last geometry pass (fragment.wgsl:23-54) as the opaque pass
 * reconstructs it — 6 floats / pixel: normal_tangent RGBA16F and barycentric RG16F, each already rounded to f16; zeros where nothing was hit.
 * Single-sampled frames, no band sharding. */
int awsm_hip_read_gbuffer(AwsmHipCtx* ctx, float* out6);
int awsm_hip_read_visibility_unpacked(AwsmHipCtx* ctx, uint32_t* tri_id_out, uint32_t* meta_off_out, float* depth_out);
int awsm_hip_read_opaque(AwsmHipCtx* ctx, uint16_t* rgba16f_out);
/* the image after the transparent pass == the reference's `composite` render texture (render_textures.rs:49-54; what the
 * display pass tone-maps): RGBA16F, width*height*8 bytes.  bind_composite lets the caller own the memory (NULL = internal). */
int awsm_hip_read_composite(AwsmHipCtx* ctx, uint16_t* rgba16f_out);
int awsm_hip_read_composite_f32(AwsmHipCtx* ctx, float* rgba32f_out);  /* needs AWSM_CFG_PARITY_TAP: the same f16 values, widened */
int awsm_hip_bind_composite(AwsmHipCtx* ctx, void* device_ptr, size_t bytes);
/* transformed vertices of the last transparent pass, one per triangle corner in draw order: clip xyzw (16 B),
 * {world N xyz, pad, world T xyzw} (32 B), world position xyz1 (16 B) == vert_main outputs (material_transparent_wgsl/vertex.wgsl) */
int awsm_hip_read_transformed_forward(AwsmHipCtx* ctx, float* clip_out, float* normal_tangent_out, float* world_pos_out, uint32_t max_vertices);
int awsm_hip_read_opaque_f32(AwsmHipCtx* ctx, float* rgba32f_out);  /* needs AWSM_CFG_PARITY_TAP */

/* ---- the effects pass + the display pass of the current frame (crates/renderer/src/render.rs:339-356):
 * EffectsRenderPass::render (render_passes/effects/{render_pass,pipeline}.rs, effects_wgsl/compute.wgsl + helpers/{smaa,bloom,dof}.wgsl) then
 * DisplayRenderPass::render (render_passes/display/render_pass.rs, display_wgsl/fragment.wgsl + helpers/tonemap.wgsl, shared_wgsl/color_space.wgsl).
 * tonemapping: ToneMapping (post_process.rs) 0 None, 1 KhronosNeutralPbr (the reference's default), 2 Aces.
 * flags: PostProcessing.bloom / .dof (post_process.rs) and AntiAliasing.smaa (anti_alias.rs).
 * The effects pass always runs: SMAA, then DoF, stored as vec4(rgb, 1.0) in RGBA16F; with bloom it is five dispatches (extract, three blurs,
 * blend), each compiled with the SMAA and DoF flags — so SMAA has no effect under bloom and DoF mixes into every bloom stage (the reference's
 * quirks, kept).  DoF reads the world depth as the transparent pass left it (min over the MSAA samples) and camera bytes 496-503
 * (focus_distance, aperture: camera.rs:200-215).  The display pass tone-maps the effects RGB, encodes sRGB and writes 8-bit RGBA (alpha 1.0).
 * Where WebGPU leaves it open (edge texels, float -> unorm8, the blur tables, operation order, f16 at every former dispatch boundary) the
 * rules are DESIGN.md §11's.
 * Valid from the point where the frame's opaque pass (and its transparent passes, if any) are enqueued until the next geometry pass, also
 * after awsm_hip_frame_end.  Reads the composite when the frame ran awsm_hip_transparent_pass, else the opaque image.  Enqueued on the shade
 * stream; with AWSM_CFG_OVERLAP_FRAMES the slot's images and depth are read before a later geometry pass reuses the slot.
 * AWSM_ERR_UNSUPPORTED on a sharded context (row strips or bands: the stencils need neighbouring rows), AWSM_ERR_NOT_READY before the opaque
 * pass, AWSM_ERR_INVALID_ARGUMENT for a struct_size other than sizeof(AwsmPostParams), a tonemapping value above 2 or unknown flags. ---- */
typedef struct AwsmPostParams {
    uint32_t struct_size;   /* sizeof(AwsmPostParams) */
    uint32_t tonemapping;   /* 0 None, 1 KhronosNeutralPbr, 2 Aces */
    uint32_t flags;         /* AWSM_POST_* */
    uint32_t reserved;      /* 0 */
} AwsmPostParams;
#define AWSM_POST_SMAA 1u
#define AWSM_POST_BLOOM 2u
#define AWSM_POST_DOF 4u
int awsm_hip_post_pass(AwsmHipCtx* ctx, const AwsmPostParams* p);
/* the display image of the last post pass: width*height*4 bytes, R G B A byte order, row 0 first (synchronous) */
int awsm_hip_read_display(AwsmHipCtx* ctx, uint8_t* rgba8_out);
/* the effects image of the last post pass: RGBA16F, width*height*8 bytes.  Needs AWSM_CFG_PARITY_TAP (the effects image need not exist otherwise). */
int awsm_hip_read_effects(AwsmHipCtx* ctx, uint16_t* rgba16f_out);
/* the display image's memory (width*height*4 bytes, checked when the post pass is enqueued); NULL = internal, one image per frame slot */
int awsm_hip_bind_display(AwsmHipCtx* ctx, void* device_ptr, size_t bytes);
/* the image the last post pass wrote (NULL before the first) */
void* awsm_hip_display_device_ptr(AwsmHipCtx* ctx);
/* ---- picking (crates/renderer/src/picker.rs:55-121 + picker/shader/picker_wgsl/compute.wgsl): the mesh under pixel
 * (x, y) of the last geometry pass, read from the visibility buffer: key -> draw -> geometry meta -> material mesh meta
 * -> mesh key words.  valid = 0 for background and for coordinates outside the frame (or outside this shard).
 * triangle_index is the primitive-local triangle (the visibility texel's first component).  Synchronous. ---- */
typedef struct AwsmPick {
    uint32_t valid;
    uint32_t mesh_key_high, mesh_key_low;   /* slotmap KeyData::as_ffi >> 32, & 0xFFFFFFFF */
    uint32_t triangle_index;
} AwsmPick;
int awsm_hip_pick(AwsmHipCtx* ctx, int32_t x, int32_t y, AwsmPick* out);

/* transformed vertices of the last geometry pass: per exploded vertex clip xyzw (16 B) and
 * {world N xyz, pad, world T xyzw} (32 B) == vert_main outputs (geometry_wgsl/vertex.wgsl:36-63). */
int awsm_hip_read_transformed(AwsmHipCtx* ctx, float* clip_out, float* normal_tangent_out, uint32_t max_vertices);

/* ---- device information for the measurement harness ---- */
int awsm_hip_device_info(AwsmHipCtx* ctx, char* name_out, size_t name_cap, uint32_t* cu_count, uint64_t* hbm_bytes);

/* ---- environment cubes at run time (crates/renderer/src/environment.rs, textures.rs:118-165; renderer-core/src/cubemap.rs:180-323,
 * cubemap/images.rs, texture/mipmap.rs).  Storage is what awsm_hip_env_cube_upload makes: an RGBA16F chain plus its aproned copy; these entries
 * fill and change it in place on the device.  The arithmetic (one rounding to f16, nearest even, per conversion; the 2x2 mip filter) is DESIGN.md §12.
 *   create            a zero-filled chain of `mips` levels (1 .. the full chain); may reallocate, like awsm_hip_env_cube_upload.
 *   write_face        update_skybox_face / update_cubemap_texture_face: `width` x `height` texels of `format` into level `mip` of one face, read
 *                     from data[layout.offset + row * bytes_per_row ...]; write_all_faces: six images, rows_per_image rows apart, in face order.
 *                     Validation follows cubemap.rs:265-323, then WebGPU's own rules for writeTexture (the extent is the level's, bytes_per_row
 *                     covers a row, rows_per_image covers the image); a refused write leaves the cube as it was.  AWSM_ERR_NOT_READY for a cube
 *                     never created or uploaded, AWSM_ERR_OUT_OF_RANGE for a level past the chain, AWSM_ERR_UNSUPPORTED for an unknown format.
 *   generate_mips     regenerate_skybox_mipmaps / regenerate_cubemap_texture_mipmaps: levels 1.. from level 0, each from the stored level above.
 *   fill_colors       Skybox::new_colors / IblTexture::new_colors: six solid faces (8-bit quantised as create_color does) + the full mip chain.
 *   fill_sky_gradient CubemapImage::new_sky_gradient: +-X / +-Z carry the gradient (row 0 = zenith), +Y the zenith, -Y the nadir colour + full chain.
 * Everything is enqueued on the context's stream behind the opaque passes in flight: a frame submitted earlier (AWSM_CFG_OVERLAP_FRAMES) keeps
 * the old texels, the next one sees the new.  write_* and generate_mips neither reallocate the cube nor synchronise the stream: a source of up
 * to 4 MiB is copied to the pinned staging ring before the call returns; a larger one is copied from the caller's memory and the call waits for
 * that copy alone (one event), so `data` is never retained. ---- */
typedef enum AwsmCubeFormat {
    AWSM_CUBE_RGBA16F = 0, AWSM_CUBE_RGBA32F = 1, AWSM_CUBE_RGBA8_UNORM = 2, AWSM_CUBE_RGBA8_SRGB = 3,
    AWSM_CUBE_BGRA8_UNORM = 4, AWSM_CUBE_BGRA8_SRGB = 5, AWSM_CUBE_B10G11R11_UFLOAT = 6, AWSM_CUBE_E5B9G9R9_UFLOAT = 7
} AwsmCubeFormat;
/* CubemapBytesLayout (cubemap.rs): where the texels lie in `data` */
typedef struct AwsmCubeLayout {
    uint32_t struct_size;      /* sizeof(AwsmCubeLayout) */
    uint32_t bytes_per_row;
    uint32_t rows_per_image;
    uint32_t reserved;         /* 0 */
    uint64_t offset;
} AwsmCubeLayout;
int awsm_hip_env_cube_create(AwsmHipCtx* ctx, AwsmCube which, uint32_t size, uint32_t mips);
int awsm_hip_env_cube_write_face(AwsmHipCtx* ctx, AwsmCube which, uint32_t face /* 0..5 = +X -X +Y -Y +Z -Z */, uint32_t mip, uint32_t width, uint32_t height,
                                 AwsmCubeFormat format, const void* data, size_t data_len, const AwsmCubeLayout* layout);
int awsm_hip_env_cube_write_all_faces(AwsmHipCtx* ctx, AwsmCube which, uint32_t mip, uint32_t width, uint32_t height,
                                      AwsmCubeFormat format, const void* data, size_t data_len, const AwsmCubeLayout* layout);
int awsm_hip_env_cube_generate_mips(AwsmHipCtx* ctx, AwsmCube which);
int awsm_hip_env_cube_fill_colors(AwsmHipCtx* ctx, AwsmCube which, uint32_t size, const float rgba[24] /* six RGBA colours in face order */);
int awsm_hip_env_cube_fill_sky_gradient(AwsmHipCtx* ctx, AwsmCube which, uint32_t size, const float zenith[4], const float nadir[4]);
int awsm_hip_env_cube_info(AwsmHipCtx* ctx, AwsmCube which, uint32_t* size, uint32_t* mips);   /* AWSM_ERR_NOT_READY while the binding is a uniform colour */
/* one level of the plain chain back to the host (tests): 6 * N * N * 4 halfs, N = max(size >> level, 1); synchronous */
int awsm_hip_env_cube_read_level(AwsmHipCtx* ctx, AwsmCube which, uint32_t level, uint16_t* rgba16f_out);

/* ---- image-based lighting from a source cube (the reference takes its filtered cubes from an offline tool) ----
 * Filters cube `src` into cube `dst`, which becomes an RGBA16F chain of `size`^2 x `mips` (alpha 1.0), reallocated like awsm_hip_env_cube_create when
 * its shape differs:
 *   kind 0  the GGX-prefiltered chain the opaque pass samples at roughness * (mips - 1): level m holds roughness m / (mips - 1), alpha = roughness^2,
 *           importance-sampled with the BRDF LUT's Hammersley set; level 0 is the source itself (its bits when the sides are equal, else resampled).
 *   kind 1  one level of cosine-weighted irradiance (the integral of L cos over the hemisphere: the shader multiplies by base_color / pi).
 * Samples read the source at a level chosen from their density, so the source should carry its full mip chain: call awsm_hip_env_cube_generate_mips
 * on it first (a short chain simply clamps the level).  The source is not modified.  Non-finite source texels propagate; nothing is clamped.
 * Enqueued on the context's stream like the other env_cube writes, with no stream synchronise unless the destination is reallocated; two calls on the
 * same input give the same bits.  AWSM_ERR_NOT_READY: the source is a uniform colour; AWSM_ERR_INVALID_ARGUMENT: src == dst, bad counts or sizes. ---- */
typedef struct AwsmEnvFilter {
    uint32_t struct_size;  /* sizeof(AwsmEnvFilter) */
    uint32_t kind;         /* 0 GGX chain, 1 Lambert */
    uint32_t size;         /* 1..8192 */
    uint32_t mips;         /* GGX: 1..full chain of size; Lambert: 1 */
    uint32_t sample_count; /* power of two, 16..4096; 0 = 1024 */
    uint32_t reserved;     /* 0 */
} AwsmEnvFilter;
int awsm_hip_env_cube_filter(AwsmHipCtx* ctx, AwsmCube src, AwsmCube dst, const AwsmEnvFilter* filter);

/* ---- a cube's level 0 from an equirectangular panorama (the reference gets its skybox from an offline tool) ----
 * Projects a `width` x `height` panorama — row 0 the zenith, the centre column along -Z at yaw 0, +X at u = 0.75 — into level 0 of an existing texel
 * cube (awsm_hip_env_cube_create first) and rebuilds that level's apron.  It makes no mips: awsm_hip_env_cube_generate_mips follows.  Each texel is the
 * mean of samples x samples bilinear taps (columns wrap, rows clamp), times `scale`, NaN -> 0, clamped to +-65504 and rounded to f16 once; alpha 1.0.
 *   AWSM_PANO_RGBE8    4 bytes per pixel, Radiance's R G B E: e == 0 is black, else m * 2^(e - 136) per channel (what awsm_host_hdr_decode writes).
 *   AWSM_PANO_RGBA32F  four floats per pixel; the fourth is ignored.
 * The §12 rules hold: enqueued on the context's stream behind the opaque passes in flight, no reallocation of the cube and no stream synchronise; a
 * source of up to 4 MiB goes through the pinned staging ring, a larger one is copied from the caller's memory and the call waits for that copy alone.
 * AWSM_ERR_NOT_READY: the cube is a uniform colour or was never created; AWSM_ERR_INVALID_ARGUMENT: a wrong struct_size, zero width or height,
 * samples > 8, a non-finite yaw or scale, bytes_per_row below a tight row; AWSM_ERR_OUT_OF_RANGE: data_len too short for the layout;
 * AWSM_ERR_UNSUPPORTED: an unknown format.  A refused call leaves the cube as it was. ---- */
typedef enum AwsmPanoFormat { AWSM_PANO_RGBE8 = 0, AWSM_PANO_RGBA32F = 1 } AwsmPanoFormat;
typedef struct AwsmEquirect {
    uint32_t struct_size;     /* sizeof(AwsmEquirect) */
    uint32_t width, height;   /* of the panorama, in pixels */
    uint32_t format;          /* AwsmPanoFormat */
    uint32_t bytes_per_row;   /* 0 = tight */
    uint32_t samples;         /* S: S x S taps per texel; 0 = auto = clamp(ceil(width / (4 N)), 1, 8), else 1..8 */
    float    yaw;             /* radians added to the azimuth */
    float    scale;           /* multiplies every value; 0 means 1.0 */
} AwsmEquirect;
int awsm_hip_env_cube_from_equirect(AwsmHipCtx* ctx, AwsmCube which, const void* data, size_t data_len, const AwsmEquirect* pano);

/* ---- the texture pool at run time (renderer-core/src/texture/texture_pool.rs:233-303, texture/convert_srgb.rs, texture/mipmap.rs).
 * Storage is what awsm_hip_texture_array_upload makes — RGBA8 UNORM, [level][layer][y][x] — and these entries fill and change it in place.
 *   create               a zero-filled array of `layers` images and `mips` levels (0 = 1); may reallocate and synchronise, as _upload does.
 *   resize_layers        more layers: every level of every existing layer is kept (moved on the device to its new offset), new layers read zero;
 *                        reallocates and synchronises as _upload does.  Fewer layers than the array has: AWSM_ERR_INVALID_ARGUMENT.
 *   write_layers         `n_layers` images of the array's extent into level 0 of layers [first_layer, first_layer + n_layers), read from
 *                        data[offset + layer * rows_per_image * bytes_per_row + row * bytes_per_row ...] (any offset; rows_per_image is read only
 *                        when n_layers > 1).  A texel is premultiplied (AWSM_TEX_PREMULTIPLY_ALPHA: c' = (2 c a + 255) / 510 on the encoded bytes)
 *                        and then decoded (AWSM_TEX_SRGB_TO_LINEAR: the 256-entry table of DESIGN.md §14); alpha is kept.  mipmap_kind is recorded
 *                        for those layers (layers never written this way have kind 0).  WebGPU's writeTexture rules are checked in 64 bits before
 *                        anything is read: bytes_per_row covers a row, rows_per_image covers an image, the last byte read lies inside data_len.
 *                        A refused write changes nothing.
 *   generate_mips_layers levels 1.. of the named layers only, each from the stored level above, with the layers' recorded kinds: the bytes
 *                        awsm_hip_texture_array_generate_mips gives.
 * write_layers and generate_mips_layers neither reallocate nor synchronise the stream: a source of up to 4 MiB goes through the pinned staging
 * ring, a larger one is copied from the caller's memory and the call waits for that copy alone.  Everything is enqueued behind the opaque passes in
 * flight (AWSM_CFG_OVERLAP_FRAMES: a frame already submitted keeps the old texels).  AWSM_ERR_NOT_READY: the array was never created or uploaded;
 * AWSM_ERR_OUT_OF_RANGE: layers past the array; AWSM_ERR_UNSUPPORTED: an unknown format or flag bit. ---- */
enum { AWSM_TEX_PREMULTIPLY_ALPHA = 1u, AWSM_TEX_SRGB_TO_LINEAR = 2u };
typedef struct AwsmTexWrite {
    uint32_t struct_size;      /* sizeof(AwsmTexWrite) */
    uint32_t format;           /* 0 = RGBA8 */
    uint32_t flags;            /* AWSM_TEX_* */
    uint32_t mipmap_kind;      /* MipmapTextureKind of the layers written */
    uint32_t bytes_per_row;
    uint32_t rows_per_image;
    uint64_t offset;
} AwsmTexWrite;
int awsm_hip_texture_array_create(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t width, uint32_t height, uint32_t layers, uint32_t mips);
int awsm_hip_texture_array_resize_layers(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t layers);
int awsm_hip_texture_array_write_layers(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t first_layer, uint32_t n_layers, const void* data, size_t data_len,
                                        const AwsmTexWrite* write);
int awsm_hip_texture_array_generate_mips_layers(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t first_layer, uint32_t n_layers);
int awsm_hip_texture_array_info(AwsmHipCtx* ctx, uint32_t array_idx, uint32_t* width, uint32_t* height, uint32_t* layers, uint32_t* mips);

/* ---- skin matrices composed on the device (crates/renderer/src/meshes/skins.rs:162-194 does it on the CPU).  A record names one
 * joint of one skin: where its world matrix lies in AWSM_BUF_TRANSFORMS, where its skin matrix goes in AWSM_BUF_SKIN_MATRICES (both byte offsets,
 * multiples of 4), and its inverse bind matrix (column-major).  Records live in an array the context owns, which grows by doubling.
 *   skin_pose_records_write   records [first, first + n); first may be at most the current count (no holes).  In stream order.
 *   skin_pose                 for each listed record id, AWSM_BUF_SKIN_MATRICES[matrix_offset, +64) = world * inverse_bind, with the products and
 *                             sums of glam's Mat4::mul_mat4 in its order, unfused: the bits the host computes.  Enqueued on the caller's stream with
 *                             the ordering of an awsm_hip_buffer_write to AWSM_BUF_SKIN_MATRICES (behind the opaque passes in flight), and logged for
 *                             the geometry cache like one, a range per run of adjacent matrices.  Neither reallocates nor synchronises.  Every id
 *                             and every offset of a listed record is checked against the record count and the two buffers' sizes before anything is
 *                             enqueued: AWSM_ERR_OUT_OF_RANGE, and nothing is written.  An id may be listed twice.
 *   buffer_read               a synchronising read-back of bytes [offset, offset + len) of a scene buffer (tests, diagnostics). ---- */
typedef struct AwsmSkinPoseRecord {
    uint32_t transform_offset;
    uint32_t matrix_offset;
    float inverse_bind[16];
} AwsmSkinPoseRecord;
int awsm_hip_skin_pose_records_write(AwsmHipCtx* ctx, uint32_t first, uint32_t n, const AwsmSkinPoseRecord* records);
int awsm_hip_skin_pose(AwsmHipCtx* ctx, const uint32_t* record_ids, uint32_t n);
int awsm_hip_buffer_read(AwsmHipCtx* ctx, AwsmBuf which, size_t offset, void* dst, size_t len);

/* ---- the editor's ground grid (crates/editor/src/grid/{shaders/grid.wgsl,render.rs,pipelines.rs}, drawn by the reference's editor in
 * its before_transparent_pass hook).  A built-in of awsm_hip_transparent_pass: between the opaque -> transparent blit and the transparent meshes every
 * pixel intersects its camera ray with the plane y = 0 and draws anti-aliased minor lines (every unit), major lines (every 10) and the X and Z axes over
 * a background tint, tested `Less` per sample against the WORLD's depth (the geometry pass's; never hud_depth, never what the transparent meshes
 * write), writing no depth, blended SrcAlpha / OneMinusSrcAlpha into the RGBA16F target.  The opaque image is untouched, so screen-space transmission
 * does not see the grid, and the depth-of-field pass's depth does not change.  Off by default; with the grid off the pass runs the kernels it ran
 * before this entry existed.
 *   defaults         the constants of grid.wgsl:87-98 (struct_size = sizeof(AwsmEditorGrid)).
 *   set_editor_grid  NULL turns the grid off.  struct_size says how much of the record the caller knows (at least the four bytes of struct_size, at
 *                    most 4096): nothing is read beyond it and fields it does not reach keep their defaults.  A non-finite value:
 *                    AWSM_ERR_INVALID_ARGUMENT, and the grid stays as it was.  Takes effect from the next awsm_hip_transparent_pass; a pass already
 *                    enqueued (AWSM_CFG_OVERLAP_FRAMES) keeps the record it was enqueued with.  The HUD transparent pass never draws it.
 *   read_editor_grid the raw layer for the last submitted frame's camera snapshot and size, whether the grid is on or off (off: the defaults) and
 *                    whatever the shard: per pixel RGBA f32, depth f32 and 1 = kept / 0 = discarded (zeros where discarded).  Any pointer may be
 *                    NULL.  Synchronous.  AWSM_ERR_NOT_READY before the first geometry pass.
 * The grid runs on sharded contexts (this shard's rows, absolute pixel coordinates), under MSAA x4 and with n_draws = 0.  awsm_hip_frame_end's replay
 * of an overflowed transparent pass needs nothing of its own: the grid is part of that pass and is replayed with the record the pass was given. ---- */
typedef struct AwsmEditorGrid {
    uint32_t struct_size;
    float color_background[3], alpha_background;
    float color_minor[3], alpha_minor;
    float color_major[3], alpha_major;
    float color_z_axis[3], alpha_axis;      /* one alpha for both axes */
    float color_x_axis[3], depth_epsilon;   /* added to the fragment's depth: coplanar scene geometry wins */
} AwsmEditorGrid;
int awsm_hip_editor_grid_defaults(AwsmEditorGrid* out);
int awsm_hip_set_editor_grid(AwsmHipCtx* ctx, const AwsmEditorGrid* grid /* NULL = off */);
int awsm_hip_read_editor_grid(AwsmHipCtx* ctx, float* rgba_out, float* depth_out, uint8_t* kept_out);

/* ---- screen-space ambient occlusion (the open "SSAO" box of the reference's docs/ROADMAP.md).  A built-in of awsm_hip_opaque_pass:
 * behind the shading kernels an occlusion term is estimated per pixel from the WORLD geometry pass's depth (the least of the four samples with MSAA;
 * never hud_depth, never what the transparent pass writes later) — view positions through the camera snapshot's inv_proj, a normal from the
 * neighbours' positions, twelve spiral taps within `radius` world units (at most 16 pixels), a 5x5 depth-aware mean — and the RGB of the opaque
 * image (and of its f32 parity tap) is multiplied by 1 - strength (1 - A') where the pixel was hit: before the opaque -> transparent blit, the
 * transmission background, the HUD passes, the post pass and any collective read that image.  Transparent meshes and the editor's grid are drawn
 * over it and not darkened; refraction sees it; the skybox and alpha are untouched.  The whole opaque colour is multiplied, direct light included
 * (the roadmap would multiply the ambient term inside the shader: no shading kernel is touched here).  Off by default; with it off the pass
 * runs the kernels it ran before this entry existed.
 *   defaults   radius 0.5 (world units), intensity 1.0, bias 0.02 (a fraction of the radius), strength 1.0; struct_size = sizeof(AwsmSsao).
 *   set_ssao   NULL turns it off.  struct_size as for awsm_hip_set_editor_grid (at least its own four bytes, at most 4096; nothing beyond it is
 *              read, fields it does not reach keep their defaults).  A non-finite value, radius <= 0 or strength outside [0, 1]:
 *              AWSM_ERR_INVALID_ARGUMENT, and the state stays as it was.  Takes effect from the next awsm_hip_opaque_pass; a pass already
 *              enqueued (AWSM_CFG_OVERLAP_FRAMES) and a replay by awsm_hip_frame_end keep the record the pass was given.
 *   read_ssao  the layers of the last submitted frame, width x height f32 each: A before the smoothing, A' after it, and view-space z (NaN where
 *              nothing was hit).  Any pointer may be NULL.  Synchronous.  AWSM_ERR_NOT_READY unless that frame's opaque pass ran with SSAO on.
 * On a sharded context (row strips or bands) an opaque pass with SSAO on returns AWSM_ERR_UNSUPPORTED, like the post pass: the stencil needs
 * rows the shard never rasterised.  A pass with has_opaque = 0 runs without it. ---- */
typedef struct AwsmSsao {
    uint32_t struct_size;
    float radius;        /* world units, > 0 */
    float intensity;
    float bias;          /* a fraction of the radius */
    float strength;      /* 0 .. 1 */
} AwsmSsao;
int awsm_hip_ssao_defaults(AwsmSsao* out);
int awsm_hip_set_ssao(AwsmHipCtx* ctx, const AwsmSsao* ssao /* NULL = off */);
int awsm_hip_read_ssao(AwsmHipCtx* ctx, float* ao_raw_out, float* ao_smoothed_out, float* view_z_out);

/* ---- shadows from one directional or spot light ("Shadows" of the reference's "Next up" list).
 *   shadow_pass      between awsm_hip_geometry_pass and awsm_hip_opaque_pass (before or after awsm_hip_hud_geometry_pass): `casters` are rasterised
 *                    single-sampled, by the world geometry pass's kernels under its depth contract, from `light_camera` — a 512-byte block in
 *                    the layout of AWSM_BUF_CAMERA (view 0, proj 64, view_proj 128, ...), as the caller would write it for a camera at the light —
 *                    into the frame slot's map_size x map_size key buffer.  n = 0 is legal: an empty map, everything is lit.
 *                    The frame's opaque pass (has_opaque set) then runs k_shadow_resolve behind its shading kernels and in front of SSAO's: per
 *                    pixel the world position from the WORLD keys' depth (the least of the four samples with MSAA) and the camera snapshot's
 *                    inv_view_proj, the light's texel, a receiver-plane depth bias from the neighbours, (2 pcf_radius + 1)^2 taps -> the
 *                    visibility V; rgb *= 1 - strength g (1 - V) on the opaque image and its f32 tap, g the facing term (0 where the surface is
 *                    turned away from the light, 1 from cos >= facing_fade on).  The whole opaque colour is multiplied, not the light's direct
 *                    term inside the light loop ("modulative" shadows); V is kept for a consumer that does.
 *                    Parameters travel with the pass: no shadow pass in a frame, no shadow in that frame.
 *                    AWSM_ERR_UNSUPPORTED on a sharded context; AWSM_ERR_NOT_READY outside that window; AWSM_ERR_INVALID_ARGUMENT (state unchanged)
 *                    for a non-finite value, map_size outside [1, 8192], pcf_radius > 2, strength outside [0, 1], facing_fade <= 0,
 *                    max_slope < 0, light[3] other than 0 or 1, camera_bytes != 512.
 *   read_shadow_map  the map_size^2 keys of the last submitted frame's pass (no hit = all ones).  AWSM_ERR_NOT_READY unless that frame had one.
 *   read_shadow      V and the multiplier m, width x height f32 each (either may be NULL).  AWSM_ERR_NOT_READY unless that frame had the pass
 *                    and an opaque pass with has_opaque behind it.
 *   defaults         map_size 2048, pcf_radius 1, light (0, 1, 0, 0), bias 1e-3, slope_bias 1, max_slope 0.05 (NDC depth per texel),
 *                    strength 0.7, facing_fade 0.1. ---- */
typedef struct AwsmShadow {
    uint32_t struct_size;
    uint32_t map_size;      /* S: the map is S x S keys, 1 <= S <= 8192 */
    uint32_t pcf_radius;    /* R in {0, 1, 2}: (2R+1)^2 taps */
    float    light[4];      /* w == 0: xyz = unit vector TOWARDS the light (directional); w == 1: xyz = the light's position (positional: spot or point) */
    float    bias, slope_bias, max_slope, strength, facing_fade;
} AwsmShadow;
int awsm_hip_shadow_defaults(AwsmShadow* out);
int awsm_hip_shadow_pass(AwsmHipCtx* ctx, const AwsmShadow* shadow, const void* light_camera, size_t camera_bytes, const AwsmDraw* casters, uint32_t n);
int awsm_hip_read_shadow_map(AwsmHipCtx* ctx, uint64_t* keys_out /* map_size^2 */);
int awsm_hip_read_shadow(AwsmHipCtx* ctx, float* visibility_out, float* multiplier_out /* width x height each */);

/* ---- shadows from several views of one light: the six faces of a cube around a point light, or nested windows (cascades) along the
 * camera's depth for a directional one.
 *   shadow_pass_views     in shadow_pass's window and in its place: view i's casters are rasterised from view i's block into layer i of the frame
 *                         slot's stack of n_views map_size x map_size key layers, one view after another on the caller's stream, each by the chain
 *                         shadow_pass runs.  A view with no casters is legal: an empty layer.  The frame's opaque pass then runs
 *                         k_shadow_resolve_views in k_shadow_resolve's place: with M = pcf_radius + 1, a pixel's view is the lowest i whose
 *                         (u_i, v_i) lies in [M, S - M)^2 with the pixel inside view i's volume; failing that the lowest i it is inside of; failing
 *                         that none (255): V = 1.  Its receiver plane and its taps are taken in that view and from that layer; a neighbour
 *                         serves the plane when it is inside that view, or when another view holds it and it lies in front of that view within
 *                         its depth range (a cube's next face, the next cascade).  With one view this is shadow_pass's resolve, operation for
 *                         operation.  A later shadow_pass or shadow_pass_views in the same frame replaces an
 *                         earlier one; a refused call leaves the earlier one standing.
 *                         AWSM_ERR_INVALID_ARGUMENT for n_views outside 1 .. AWSM_SHADOW_MAX_VIEWS or views == NULL; per view what shadow_pass
 *                         refuses for its camera and casters, naming the view; everything else as shadow_pass.
 *   read_shadow_map_view  layer `view` of the last submitted frame's pass.  AWSM_ERR_INVALID_ARGUMENT for a view that pass did not have (a pass through
 *                         shadow_pass has view 0 alone); awsm_hip_read_shadow_map returns layer 0.
 *   read_shadow_view      per pixel the view it was resolved in, 255 = none.  AWSM_ERR_NOT_READY as read_shadow, and when the frame's pass came
 *                         through shadow_pass (k_shadow_resolve writes no such layer). ---- */
#define AWSM_SHADOW_MAX_VIEWS 6
typedef struct AwsmShadowView {
    const void*     light_camera;   /* a 512-byte block in AWSM_BUF_CAMERA's layout, as awsm_hip_shadow_pass takes it */
    size_t          camera_bytes;
    const AwsmDraw* casters;
    uint32_t        n_casters;      /* 0 is legal: an empty layer */
} AwsmShadowView;
int awsm_hip_shadow_pass_views(AwsmHipCtx* ctx, const AwsmShadow* shadow, const AwsmShadowView* views, uint32_t n_views /* 1 .. 6 */);
int awsm_hip_read_shadow_map_view(AwsmHipCtx* ctx, uint32_t view, uint64_t* keys_out /* map_size^2 */);
int awsm_hip_read_shadow_view(AwsmHipCtx* ctx, uint8_t* view_out /* width x height: the chosen view, 255 = none */);

/* ---- the editor's selection overlay ("Visual bounding box around selected objects" of the reference's "Next up" list).  A built-in
 * of awsm_hip_transparent_pass, drawn as its last step — over the grid, the transparent meshes and the MSAA resolve, under the HUD transparent pass,
 * in front of the post pass: an OUTLINE around the visible pixels of the selected meshes (opaque meshes: from the WORLD visibility keys; a pixel is
 * selected when any of its samples shows a triangle of a selected mesh, and the ring is every unselected pixel within outline_radius pixels of a
 * selected one), and a WIRE BOX around every listed world-space box (opaque and transparent meshes alike), anti-aliased lines of half width
 * box_half_width, tested against the WORLD's depth (the least of the samples; never hud_depth, never what the transparent meshes wrote) and
 * multiplied by hidden_alpha where behind it.  Both blend SrcAlpha / OneMinusSrcAlpha into the RGBA16F composite, ring first; the opaque image and
 * the keys are untouched.  Off by default; with it off the pass runs the kernels it ran before this entry existed.
 *   defaults       both flags, outline_radius 2, outline (1, 0.6, 0.1, 1), box (1, 0.6, 0.1, 0.9), box_half_width 0.75, hidden_alpha 0.25,
 *                  depth_epsilon 1e-5; struct_size = sizeof(AwsmSelection).
 *   set_selection  NULL turns it off.  struct_size as for awsm_hip_set_editor_grid.  mesh_keys: n_keys x {high, low} as AwsmPick reports them,
 *                  n_keys <= 64; boxes: n_boxes <= 64.  Keys and boxes are copied.  AWSM_ERR_INVALID_ARGUMENT, with the state unchanged, for a
 *                  non-finite value, unknown flag bits, outline_radius outside 1..4, box_half_width outside (0, 4], an alpha or hidden_alpha
 *                  outside [0, 1], depth_epsilon < 0, a box with min > max on some axis, a count over its cap, a NULL array with a non-zero
 *                  count.  No keys and no boxes, or flags that leave nothing to draw, is the same as off.  Takes effect from the next
 *                  awsm_hip_transparent_pass; a pass already enqueued (AWSM_CFG_OVERLAP_FRAMES) and a replay by awsm_hip_frame_end keep the
 *                  record the pass was given.  The HUD transparent pass never draws it.
 *   read_selection the layers of the last submitted frame, computed once more from its keys, draw list and camera snapshot with the record its pass
 *                  was given: selected and ring (1 / 0) and the box alpha A per pixel, and the edge table, 8 floats per edge in box order, edges
 *                  by axis then corner: x0 y0 z0 x1 y1 z1 (pixels, pixels, NDC depth) valid pad, all zero for an edge that is clipped away.  Any
 *                  pointer may be NULL.  Synchronous.  AWSM_ERR_NOT_READY unless that frame's world transparent pass ran with selection on.
 * On a sharded context (row strips or bands) a world transparent pass with selection on returns AWSM_ERR_UNSUPPORTED, as SSAO does: the ring
 * needs rows the shard never rasterised. ---- */
#define AWSM_SELECTION_OUTLINE 1u
#define AWSM_SELECTION_BOXES 2u
typedef struct AwsmSelection {
    uint32_t struct_size;
    uint32_t flags;            /* AWSM_SELECTION_OUTLINE | AWSM_SELECTION_BOXES */
    uint32_t outline_radius;   /* R, 1..4 pixels */
    float    outline_color[4]; /* rgb, alpha */
    float    box_color[4];     /* rgb, alpha */
    float    box_half_width;   /* pixels, 0 < hw <= 4 */
    float    hidden_alpha;     /* 0..1: factor on a box fragment behind the world's depth */
    float    depth_epsilon;    /* subtracted from the fragment's depth before the test */
} AwsmSelection;
typedef struct AwsmSelectionBox { float min[3], max[3]; } AwsmSelectionBox;   /* world space */
int awsm_hip_selection_defaults(AwsmSelection* out);
int awsm_hip_set_selection(AwsmHipCtx* ctx, const AwsmSelection* selection /* NULL = off */,
                           const uint32_t* mesh_keys /* n_keys x {high, low} */, uint32_t n_keys, const AwsmSelectionBox* boxes, uint32_t n_boxes);
int awsm_hip_read_selection(AwsmHipCtx* ctx, uint8_t* selected_out, uint8_t* ring_out, float* box_alpha_out /* width x height each */,
                            float* edges_out /* n_boxes x 12 x 8 floats */);

/* ---- temporal anti-aliasing (the "TAA" box of the reference's docs/ROADMAP.md, whose camera still carries the jitter).  State of
 * awsm_hip_post_pass, as SSAO is state of the opaque pass: with it on, the post pass begins with k_taa_resolve.  Per pixel the resolve takes the depth
 * of the WORLD key (the least of the four samples with MSAA, 1.0 where nothing was hit; never hud_depth), forms the pixel's unjittered NDC position
 * n = pixel centre - jitter_ndc, q = reproject * (n, depth, 1) and the history position pixel + (q.xy / q.w - n) in texels, samples the last
 * resolved image there bilinearly (taps clamped to the edge), clamps the sample per channel to the min / max of the current image's 3x3
 * neighbourhood and writes history * (1 - feedback) + current * feedback, alpha from the current image.  "Current image" is what the post pass
 * reads anyway: the composite when the frame had a transparent pass, else the opaque image.  The history is usable when there is one, q.w > 0 and
 * the position lies within half a texel of the image; elsewhere the current texel is copied.  The resolved image is the next frame's history AND
 * the source of everything behind it in the post pass (SMAA, bloom, DoF, tone map, display): two RGBA16F images per context, in ping-pong, the
 * index advancing once per frame — a post pass awsm_hip_frame_end enqueues again for a replayed frame reads the same history and rewrites the same
 * image.  The caller jitters its projection by jitter_ndc (proj' = translation(jitter_ndc, 0) * proj) and hands over
 * reproject = view_proj_previous * inverse(view_proj_current), both unjittered; the host layer does both (awsm_host_set_taa).
 *   defaults  feedback 0.1, flags 0, jitter_ndc (0, 0), reproject = identity; struct_size = sizeof(AwsmTaa).
 *   set_taa   NULL turns it off and drops the history.  struct_size as for awsm_hip_set_ssao (at least its own four bytes, at most 4096; nothing
 *             beyond it is read, fields it does not reach keep their defaults).  A non-finite value, feedback outside (0, 1] or an unknown flag:
 *             AWSM_ERR_INVALID_ARGUMENT, and the state stays as it was.  Takes effect from the next awsm_hip_post_pass; a pass already enqueued
 *             (AWSM_CFG_OVERLAP_FRAMES) and a replay keep the record they were given.  AWSM_TAA_RESET drops the history in front of the next
 *             post pass and is cleared by it.
 *   read_taa  of the last post pass: the resolved image (width x height x 4 f16), the history position (sx, sy) per pixel in texel-index units
 *             (width x height x 2 f32) and whether the history was used (width x height bytes) — the last two computed once more from the frame's
 *             keys and the record.  Any pointer may be NULL.  Synchronous.  AWSM_ERR_NOT_READY unless the last post pass resolved.
 * The history is also dropped by awsm_hip_resize (a new size or MSAA mode) and by a frame a hand-off gate dropped.
 * Limits: no per-object motion vectors — a moving or animated mesh is reprojected as if it stood still, and only the neighbourhood clamp bounds its
 * ghost; transparent and HUD pixels are reprojected with the world depth behind them; no depth-based disocclusion test (the history's depth is not
 * kept); no luma weighting; unsharded contexts only (the post pass refuses shards). ---- */
#define AWSM_TAA_RESET 1u
typedef struct AwsmTaa {
    uint32_t struct_size;
    float    feedback;        /* weight of the current image, 0 < feedback <= 1 */
    uint32_t flags;           /* AWSM_TAA_RESET */
    float    jitter_ndc[2];   /* what the frame's projection was translated by */
    float    reproject[16];   /* column-major: unjittered NDC of this frame -> unjittered clip space of the previous one */
} AwsmTaa;
int awsm_hip_taa_defaults(AwsmTaa* out);
int awsm_hip_set_taa(AwsmHipCtx* ctx, const AwsmTaa* taa /* NULL = off, history dropped */);
int awsm_hip_read_taa(AwsmHipCtx* ctx, uint16_t* resolved_rgba16f_out, float* lookup_xy_out, uint8_t* used_out);

/* ---- picking that sees transparent meshes: point and rectangle queries ("Make transparent meshes pickable" of the reference's
 * "Next up" list).  awsm_hip_pick reads the visibility keys, and a transparent mesh has none; these queries also read the fragment lists the
 * transparent passes of the last submitted frame left.  Over sample 0, the hit at a pixel is the first of these that exists:
 *   1. the LAST fragment of the HUD transparent pass's list with alpha >= alpha_threshold   (layer 3; only if that pass ran this frame)
 *   2. the HUD geometry key                                                                 (layer 2)
 *   3. the LAST fragment of the world transparent pass's list with alpha >= alpha_threshold (layer 1)
 *   4. the world visibility key                                                             (layer 0)
 * The pipeline tests LessEqual and writes depth, so a later fragment of a list is nearer.  The alpha is the one the fragment was blended with (a MASK
 * fragment that survived its cutoff: 1).  What the lists do not hold cannot be picked: a fragment the depth test or a cutoff discarded, and one
 * behind a fragment that wrote depth, whatever that one's alpha.  With AWSM_PICK_TRANSPARENT clear steps 1 and 3 are left out and every answer is
 * awsm_hip_pick's.  With it set and no transparent pass in the frame, the opaque layers alone answer.
 *   pick_query_defaults  flags 0, alpha_threshold 0.5; struct_size = sizeof(AwsmPickQuery).
 *   pick_ex        the rule at (x, y).  triangle_index: primitive-local, in the pass the hit belongs to; alpha: 1 for layers 0 and 2; depth_bits:
 *                  the key's depth word for layers 0 and 2, for a fragment the depth its triangle's set-up record gives at the pixel (sample 0).
 *   pick_rect      the rule at every pixel of [x0, x1) x [y0, y1) clamped to the frame -> the distinct (layer, mesh key) pairs with the pixels each
 *                  holds, ordered by layer, then by the draw's place in its pass's list; draws that share a mesh key are merged into the first.
 *                  *n_out = the distinct pairs, of which at most cap are written; an empty rectangle gives 0.  Integer sums: deterministic.
 *   read_pick_map  test aid: the rule at every pixel of the frame, word = layer << 28 | index of the draw in its pass's list as the device expands
 *                  it (a draw without triangles dropped, one entry per instance), all ones for a miss; triangle = triangle_index.  Either may be NULL.
 * query == NULL: the defaults.  All three are synchronous, read the last submitted frame's slot and wait for every stream first.
 * AWSM_ERR_NOT_READY before a geometry pass, and with the flag set while a transparent pass's counters show a bin or fragment list overflow that
 * awsm_hip_frame_end has not replayed yet; AWSM_ERR_INVALID_ARGUMENT for a wrong struct_size, unknown flags, a threshold outside [0, 1] or NaN,
 * out == NULL with cap > 0; AWSM_ERR_UNSUPPORTED on a sharded context for the flag and for pick_rect (a rectangle's answer would need merging
 * across ranks).  Optional symbols: AWSM_HIP_ABI_VERSION is unchanged. ---- */
#define AWSM_PICK_TRANSPARENT 1u
typedef struct AwsmPickQuery {
    uint32_t struct_size;
    uint32_t flags;             /* AWSM_PICK_TRANSPARENT */
    float    alpha_threshold;   /* 0..1 */
} AwsmPickQuery;
typedef struct AwsmPickHit {
    uint32_t valid;             /* 0 = background / outside the frame */
    uint32_t mesh_key_high, mesh_key_low;
    uint32_t triangle_index;
    uint32_t layer;             /* 0 world opaque, 1 world transparent, 2 HUD opaque, 3 HUD transparent */
    float    alpha;
    uint32_t depth_bits;        /* f32 bits */
} AwsmPickHit;
typedef struct AwsmPickRectEntry { uint32_t layer, mesh_key_high, mesh_key_low, pixels; } AwsmPickRectEntry;
int awsm_hip_pick_query_defaults(AwsmPickQuery* out);
int awsm_hip_pick_ex(AwsmHipCtx* ctx, int32_t x, int32_t y, const AwsmPickQuery* query, AwsmPickHit* out);
int awsm_hip_pick_rect(AwsmHipCtx* ctx, int32_t x0, int32_t y0, int32_t x1, int32_t y1, const AwsmPickQuery* query, AwsmPickRectEntry* out, uint32_t cap,
                       uint32_t* n_out);
int awsm_hip_read_pick_map(AwsmHipCtx* ctx, const AwsmPickQuery* query, uint32_t* word_out, uint32_t* triangle_out /* width x height each */);

#ifdef __cplusplus
}
#endif
#endif /* AWSM_HIP_H */
