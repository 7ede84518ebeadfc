// host.cpp — C++ host layer: the reference's key-based scene API + dirty-upload semantics over the C-ABI.
//
// Mirrors, for the hot path only (paths relative to /root/reference/crates/renderer/src/):
//   transforms.rs:43-446          Transforms (TRS tree, dirty propagation, world mat4 + normal mat3 mirrors)
//   camera.rs:111-227,285-306     CameraBuffer::update
//   lights.rs:160-310,354-473     Lights
//   textures.rs:226-320           texture transforms (identity slot), pool bookkeeping
//   materials.rs:60-241, materials/{pbr,unlit,writer}.rs   material word streams in a DynamicStorageBuffer
//   meshes.rs:317-674,872-939,1241-1346   Meshes (4 hot-path DynamicStorageBuffers), update_world, write_gpu
//   meshes/meta.rs, meta/{geometry,material}_meta.rs       40-B / 68-B metas in 256-B slots
//   meshes/skins.rs:84-194, meshes/morphs.rs:121-217
//   gltf/buffers/mesh/visibility.rs:35-165, attributes.rs:113-160, skin.rs:22-113, morph.rs:31-190   packers
//   renderable.rs:38-150, frustum.rs:42-89, bounds.rs:38-61   cull + sort -> draw list
//   render.rs:71-97,144-221,370   write_gpu order, geometry pass, opaque pass, submit
//   buffer/helpers.rs:124-220     write_buffer_with_dirty_ranges
//   animation/animations.rs:39-141   Animations, update_animations (players and samplers: animation.hpp)
// The device is reached only through the awsm_hip_* C-ABI, resolved with dlsym from the backend library.
#include "../../include/awsm_host.h"

#include <dlfcn.h>
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "animation.hpp"
#include "buffers.hpp"
#include "glam.hpp"
#include "ktx2.hpp"
#include "rgbe.hpp"
#include "../csrc/tex_pool.hpp"      // the sRGB table and the integer premultiply, shared with the device library

using namespace awsm_host;

namespace {

struct Backend {
    void* dl = nullptr;
    int (*create)(const AwsmConfig*, AwsmHipCtx**) = nullptr;
    int (*destroy)(AwsmHipCtx*) = nullptr;
    const char* (*last_error)(const AwsmHipCtx*) = nullptr;
    uint32_t (*abi_version)(void) = nullptr;
    int (*buffer_create)(AwsmHipCtx*, AwsmBuf, size_t) = nullptr;
    int (*buffer_write)(AwsmHipCtx*, AwsmBuf, size_t, const void*, size_t) = nullptr;
    int (*resize)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t) = nullptr;
    int (*set_shard_rows)(AwsmHipCtx*, uint32_t, uint32_t) = nullptr;
    int (*set_shard_bands)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t) = nullptr;
    int (*set_stage_timers)(AwsmHipCtx*, int) = nullptr;
    int (*pick)(AwsmHipCtx*, int32_t, int32_t, AwsmPick*) = nullptr;
    int (*texture_array_upload)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, AwsmTexFormat, const void*) = nullptr;
    int (*texture_array_generate_mips)(AwsmHipCtx*, uint32_t, const uint32_t*) = nullptr;
    int (*sampler_set)(AwsmHipCtx*, uint32_t, const AwsmSampler*) = nullptr;
    int (*env_upload)(AwsmHipCtx*, const AwsmEnv*) = nullptr;
    int (*env_cube_upload)(AwsmHipCtx*, AwsmCube, uint32_t, uint32_t, const uint16_t*) = nullptr;
    int (*brdf_lut_generate)(AwsmHipCtx*, uint32_t, uint32_t) = nullptr;
    int (*geometry_pass)(AwsmHipCtx*, const AwsmDraw*, uint32_t) = nullptr;
    int (*opaque_pass)(AwsmHipCtx*, const AwsmOpaqueParams*) = nullptr;
    int (*transparent_pass)(AwsmHipCtx*, const AwsmDraw*, uint32_t) = nullptr;
    int (*hud_geometry_pass)(AwsmHipCtx*, const AwsmDraw*, uint32_t) = nullptr;
    int (*hud_transparent_pass)(AwsmHipCtx*, const AwsmDraw*, uint32_t) = nullptr;
    int (*frame_end)(AwsmHipCtx*, AwsmFrameStats*) = nullptr;
    int (*post_pass)(AwsmHipCtx*, const AwsmPostParams*) = nullptr;     // optional: a backend without it cannot post-process
    int (*editor_grid_defaults)(AwsmEditorGrid*) = nullptr;             // optional: the editor's ground grid (awsm_host_set_editor_grid)
    int (*set_editor_grid)(AwsmHipCtx*, const AwsmEditorGrid*) = nullptr;
    int (*ssao_defaults)(AwsmSsao*) = nullptr;                          // optional: screen-space ambient occlusion (awsm_host_set_ssao)
    int (*set_ssao)(AwsmHipCtx*, const AwsmSsao*) = nullptr;
    int (*set_taa)(AwsmHipCtx*, const AwsmTaa*) = nullptr;              // optional: temporal anti-aliasing (awsm_host_set_taa)
    int (*selection_defaults)(AwsmSelection*) = nullptr;                // optional: the editor's selection overlay (awsm_host_set_selection)
    int (*set_selection)(AwsmHipCtx*, const AwsmSelection*, const uint32_t*, uint32_t, const AwsmSelectionBox*, uint32_t) = nullptr;
    int (*pick_ex)(AwsmHipCtx*, int32_t, int32_t, const AwsmPickQuery*, AwsmPickHit*) = nullptr;      // optional: picking through the transparent passes (awsm_host_pick_ex / _pick_rect)
    int (*pick_rect)(AwsmHipCtx*, int32_t, int32_t, int32_t, int32_t, const AwsmPickQuery*, AwsmPickRectEntry*, uint32_t, uint32_t*) = nullptr;
    int (*shadow_defaults)(AwsmShadow*) = nullptr;                      // optional: shadows (awsm_host_set_shadow)
    int (*shadow_pass)(AwsmHipCtx*, const AwsmShadow*, const void*, size_t, const AwsmDraw*, uint32_t) = nullptr;
    int (*shadow_pass_views)(AwsmHipCtx*, const AwsmShadow*, const AwsmShadowView*, uint32_t) = nullptr;      // optional: point lights, cascades
    // optional: environment cubes at run time (awsm_host_env_cube_*)
    int (*env_cube_create)(AwsmHipCtx*, AwsmCube, uint32_t, uint32_t) = nullptr;
    int (*env_cube_write_face)(AwsmHipCtx*, AwsmCube, uint32_t, uint32_t, uint32_t, uint32_t, AwsmCubeFormat, const void*, size_t, const AwsmCubeLayout*) = nullptr;
    int (*env_cube_write_all_faces)(AwsmHipCtx*, AwsmCube, uint32_t, uint32_t, uint32_t, AwsmCubeFormat, const void*, size_t, const AwsmCubeLayout*) = nullptr;
    int (*env_cube_generate_mips)(AwsmHipCtx*, AwsmCube) = nullptr;
    int (*env_cube_fill_colors)(AwsmHipCtx*, AwsmCube, uint32_t, const float*) = nullptr;
    int (*env_cube_fill_sky_gradient)(AwsmHipCtx*, AwsmCube, uint32_t, const float*, const float*) = nullptr;
    int (*env_cube_filter)(AwsmHipCtx*, AwsmCube, AwsmCube, const AwsmEnvFilter*) = nullptr;      // optional (awsm_host_env_bake_ibl)
    int (*env_cube_from_equirect)(AwsmHipCtx*, AwsmCube, const void*, size_t, const AwsmEquirect*) = nullptr;      // optional (awsm_host_env_cube_from_equirect / _load_hdr)
    // optional: the texture pool at run time (awsm_host_texture_insert_ex / _update; finalize of a resident array)
    int (*texture_array_create)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) = nullptr;
    int (*texture_array_resize_layers)(AwsmHipCtx*, uint32_t, uint32_t) = nullptr;
    int (*texture_array_write_layers)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t, const void*, size_t, const AwsmTexWrite*) = nullptr;
    int (*texture_array_generate_mips_layers)(AwsmHipCtx*, uint32_t, uint32_t, uint32_t) = nullptr;
    int (*texture_array_info)(AwsmHipCtx*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*) = nullptr;
    // optional: skin matrices composed on the device (awsm_host_set_device_skin_posing)
    int (*skin_pose_records_write)(AwsmHipCtx*, uint32_t, uint32_t, const AwsmSkinPoseRecord*) = nullptr;
    int (*skin_pose)(AwsmHipCtx*, const uint32_t*, uint32_t) = nullptr;
    // the name of the first of them the library lacks, or null
    const char* texture_pool_missing() const {
        return !texture_array_create ? "awsm_hip_texture_array_create" : !texture_array_resize_layers ? "awsm_hip_texture_array_resize_layers"
             : !texture_array_write_layers ? "awsm_hip_texture_array_write_layers" : !texture_array_generate_mips_layers ? "awsm_hip_texture_array_generate_mips_layers"
             : !texture_array_info ? "awsm_hip_texture_array_info" : nullptr;
    }
};

struct Transform { Vec3 t; Quat r; Vec3 s; };
struct Aabb { Vec3 min, max; };

Aabb aabb_transformed(const Aabb& a, const Mat4& m) {   // bounds.rs:38-61
    const Vec3 mn = a.min, mx = a.max;
    const Vec3 corners[8] = {{mn.x, mn.y, mn.z}, {mx.x, mn.y, mn.z}, {mn.x, mx.y, mn.z}, {mx.x, mx.y, mn.z},
                             {mn.x, mn.y, mx.z}, {mx.x, mn.y, mx.z}, {mn.x, mx.y, mx.z}, {mx.x, mx.y, mx.z}};
    Vec3 first = mat4_transform_point3(m, corners[0]);
    Aabb out{first, first};
    for (int i = 1; i < 8; i++) {
        Vec3 t = mat4_transform_point3(m, corners[i]);
        out.min = v3_min(out.min, t);
        out.max = v3_max(out.max, t);
    }
    return out;
}

struct Plane { Vec3 n; float d; };
struct Frustum {   // frustum.rs:42-89
    Plane planes[6];
    explicit Frustum(const Mat4& vp) {
        const Vec4 row0 = {vp.c[0].x, vp.c[1].x, vp.c[2].x, vp.c[3].x}, row1 = {vp.c[0].y, vp.c[1].y, vp.c[2].y, vp.c[3].y};
        const Vec4 row2 = {vp.c[0].z, vp.c[1].z, vp.c[2].z, vp.c[3].z}, row3 = {vp.c[0].w, vp.c[1].w, vp.c[2].w, vp.c[3].w};
        const Vec4 raw[6] = {v4_add(row3, row0), v4_sub(row3, row0), v4_add(row3, row1), v4_sub(row3, row1), row2, v4_sub(row3, row2)};
        for (int i = 0; i < 6; i++) {
            Vec3 n = {raw[i].x, raw[i].y, raw[i].z};
            float d = raw[i].w;
            const float len = std::sqrt((n.x * n.x + n.y * n.y) + n.z * n.z);
            if (len > 0.0f) { n = {n.x / len, n.y / len, n.z / len}; d = d / len; }
            planes[i] = {n, d};
        }
    }
    bool intersects(const Aabb& a) const {
        for (const Plane& p : planes) {
            const Vec3 pt = {p.n.x >= 0.0f ? a.max.x : a.min.x, p.n.y >= 0.0f ? a.max.y : a.min.y, p.n.z >= 0.0f ? a.max.z : a.min.z};
            if (v3_dot(p.n, pt) + p.d < 0.0f) return false;
        }
        return true;
    }
};

void push_f32(std::vector<uint8_t>& d, float v) { uint8_t b[4]; memcpy(b, &v, 4); d.insert(d.end(), b, b + 4); }
void push_u32(std::vector<uint8_t>& d, uint32_t v) { uint8_t b[4]; memcpy(b, &v, 4); d.insert(d.end(), b, b + 4); }

struct MeshRec {
    SlotKey transform_key = 0, material_key = 0, resource_key = 0, skin_key = 0, morph_key = 0;
    bool double_sided = false, hidden = false, hud = false, has_world_aabb = true, instanced = false;
    bool transparent = false;   // transparency geometry instead of visibility geometry (gltf/buffers/mesh.rs:33-57)
    Aabb local_aabb{}, world_aabb{};
    uint32_t tri_count = 0;
    size_t vis_off = 0, tr_off = 0;
};

}  // namespace

struct AwsmHost {
    Backend be;
    AwsmHipCtx* ctx = nullptr;
    std::string last_error;
    AwsmHostHook after_geometry = nullptr, after_opaque = nullptr;     // RenderHooks (render.rs:54-63,181-190)
    void* after_geometry_user = nullptr; void* after_opaque_user = nullptr;

    // ---- transforms.rs ----
    SlotMap<Transform> locals;
    std::unordered_map<SlotKey, Mat4> world;
    std::unordered_map<SlotKey, std::vector<SlotKey>> children;
    std::unordered_map<SlotKey, SlotKey> parents;
    std::unordered_set<SlotKey> dirties;
    std::vector<SlotKey> dirty_meshes;
    bool transforms_gpu_dirty = true;
    SlotKey root = 0;
    DynamicUniformBuffer transforms_buf{32, 64};
    DynamicUniformBuffer normals_buf{32, 36};

    // ---- textures.rs ----
    struct PoolArray {
        uint32_t w, h; std::vector<uint8_t> texels; uint32_t layers = 0; bool dirty = true; std::vector<uint32_t> kinds;   // kinds: MipmapTextureKind per layer
        // Run-time pool.  flags: AWSM_TEX_* per layer, still to be applied to the layer's bytes in `texels` — by the device when the layer
        // is written there, by the host when the mirror is asked for, whichever comes first; 0 once the bytes are the pool's content.
        std::vector<uint32_t> flags, desc_flags;      // desc_flags: what the layer was inserted with (awsm_host_texture_update applies it again)
        uint32_t dev_layers = 0;                      // layers the device's array has room for (0: not on the device)
        uint32_t sent_layers = 0;                     // layers [0, sent_layers) are there
        std::vector<uint32_t> resend;                 // layers below sent_layers whose pixels were replaced
    };
    std::vector<PoolArray> pool;
    std::vector<std::pair<uint32_t, uint32_t>> tex_entries;   // texture id -> (array, layer)
    std::vector<AwsmSampler> samplers;
    SlotMap<int> tex_transform_keys;
    DynamicUniformBuffer tex_transforms_buf{32, 32};
    size_t tex_transform_identity_offset = 0;
    bool tex_transforms_dirty = true;

    // ---- materials.rs ----
    SlotMap<AwsmHostMaterial> materials;
    DynamicStorageBuffer materials_buf{8192};
    bool materials_dirty = true;

    // ---- lights.rs ----
    SlotMap<AwsmHostLight> lights;
    size_t punctual_gpu_size = 64;
    bool punctual_dirty = true, lights_info_dirty = true, lights_created = false, lights_info_created = false;
    uint32_t prefiltered_mips = 9, irradiance_mips = 9;

    // ---- meshes.rs / meta / skins / morphs ----
    static constexpr size_t kIndicesInitial = 512 * 3 * 1000;
    SlotMap<MeshRec> meshes;              // DenseSlotMap<MeshKey, Mesh>
    SlotMap<int> resources;
    std::unordered_map<SlotKey, std::vector<SlotKey>> transform_to_meshes;
    DynamicStorageBuffer vis_data{kIndicesInitial * 56}, vis_index{kIndicesInitial}, attr_data{kIndicesInitial * 16}, attr_index{kIndicesInitial};
    bool vis_data_dirty = true, vis_index_dirty = true, attr_data_dirty = true, attr_index_dirty = true;
    DynamicStorageBuffer tr_data{kIndicesInitial * 40};   // meshes.rs:358-359,403-415: 40 B / original vertex of the transparent meshes
    bool tr_data_dirty = true;

    // ---- instances.rs: per-instance mat4s, keyed by the instanced mesh's transform key ----
    DynamicStorageBuffer instances{64 * 32};
    std::unordered_map<SlotKey, uint32_t> instance_count;
    std::unordered_map<SlotKey, std::vector<Transform>> instance_list;
    bool instances_dirty = false;   // Instances::transform_gpu_dirty: set by the first transform_insert
    DynamicUniformBuffer geom_meta{512, 40, 256}, material_meta{512, 68, 256};
    bool geom_meta_dirty = true, material_meta_dirty = true;
    SlotMap<std::vector<SlotKey>> skins;   // skeleton joint transforms
    std::unordered_map<SlotKey, Mat4> inverse_bind;
    std::unordered_map<SlotKey, uint32_t> skin_sets;
    DynamicStorageBuffer skin_matrices{16 * 4 * 32}, skin_index_weights{4096 * 2};
    bool skin_matrices_dirty = true, skin_iw_dirty = true;
    // One record per (skin, joint), in insertion order: what skins.rs:162-194 walks, indexed by the joint's transform key so that a frame costs
    // O(joints that moved).  With device posing on, a record is also resident on the device under the same id (awsm_hip_skin_pose_records_write).
    struct PoseRecord { SlotKey skin, joint; uint32_t joint_index; };
    std::vector<PoseRecord> pose_records;
    std::unordered_map<SlotKey, std::vector<uint32_t>> joint_records;      // transform key -> record ids
    bool device_posing = false;
    uint32_t pose_records_sent = 0;              // records [0, sent) are on the device as they are here
    std::vector<uint32_t> pose_records_resend;   // ... but for these, whose inverse bind matrix a later skin replaced
    std::vector<uint32_t> pose_ids;              // records the next render has the device compose (sorted at render)
    std::vector<uint32_t> pose_ids_last;         // ... and what the last render handed over
    std::unordered_set<uint32_t> pose_stale;     // records whose matrix in the host mirror is older than the device's
    SlotMap<uint32_t> morphs;             // targets_len
    DynamicStorageBuffer morph_weights{4096}, morph_values{4096};
    bool morph_weights_dirty = true, morph_values_dirty = true;

    // ---- animation/animations.rs:39-44: players; SecondaryMaps iterate in slot order ----
    SlotMap<anim::Player> players;
    std::map<uint32_t, std::pair<SlotKey, SlotKey>> anim_transforms, anim_morphs;      // slot index -> (animation key, transform key / mesh key)
    std::vector<AwsmKey> gltf_animation_keys;      // what the last awsm_host_load_gltf made

    // ---- camera.rs ----
    uint8_t camera_raw[512] = {};
    bool camera_dirty = true, camera_created = false, have_camera = false;
    float dof_params[2] = {0.0f, 0.0f};        // focus_distance, aperture (camera bytes 496-503): 0, 0 until awsm_host_camera_set_dof
    // ---- post_process.rs + AntiAliasing.smaa: off until awsm_host_set_post_processing ----
    bool post_on = false;
    AwsmPostParams post{};
    bool grid_on = false;                      // awsm_host_set_editor_grid: the world transparent pass runs every frame, with no draws if need be
    // awsm_host_set_selection: the record as the caller gave it (its struct_size says how much of it counts) and the mesh keys; every render hands
    // the backend the key words and the world AABBs of those that are there, shown and not HUD.  While on, the world transparent pass runs every frame.
    bool selection_on = false;
    AwsmSelection selection{};
    std::vector<AwsmKey> selection_keys;
    bool sharded = false;                      // awsm_host_set_shard_rows / _bands gave this host a part of the frame (the post pass needs all of it)
    // ---- shadows (awsm_host_set_shadow): the record, and what the last render handed the backend (awsm_host_shadow_camera) ----
    bool shadow_on = false, shadow_rendered = false;
    AwsmHostShadow shadow{};
    uint8_t shadow_block[512] = {};
    std::vector<AwsmDraw> shadow_casters;
    Mat4 cam_view = mat4_identity(), cam_proj = mat4_identity();
    // ---- temporal anti-aliasing (awsm_host_set_taa): the record; the jittered block of the frame (camera_raw stays the unjittered
    // one awsm_host_camera_update packed); the unjittered matrices of the last render with TAA on, as camera.rs keeps last_matrices ----
    bool taa_on = false, taa_reset = true, taa_have_last = false;
    AwsmHostTaa taa{(uint32_t)sizeof(AwsmHostTaa), 0.1f, 0.8f, 0.2f};
    uint8_t taa_block[512] = {};
    Mat4 taa_last_view = mat4_identity(), taa_last_proj = mat4_identity();
    AwsmTaa taa_sent{};                        // what the last render handed the backend
    uint32_t frame_count = 0;
    uint32_t width = 0, height = 0;
    uint32_t msaa_sample_count = 0;   // AntiAliasing::msaa_sample_count: 0 = None, 4 = Some(4)
    bool mipmap = false;              // AntiAliasing::mipmap: MipmapMode::Gradient vs None in the opaque pass

    bool created[AWSM_BUF_COUNT] = {};
    uint64_t upload_bytes = 0;
    std::vector<AwsmDraw> last_draws, last_transparent_draws, last_hud_geometry_draws, last_hud_transparent_draws;
    bool has_hud_meshes = false;
    uint32_t n_hud_meshes = 0, n_world_transparent_meshes = 0;   // what the two flags are kept from (a removed mesh takes its pass with it: ADVICE r3)
    bool has_transparent_meshes = false;
    // ---- shadows from several views: the cascades record, and every view the last render sent (view 0 is shadow_block /
    // shadow_casters too).  At the struct's end: every older member keeps its offset. ----
    AwsmHostShadowCascades shadow_cascades{(uint32_t)sizeof(AwsmHostShadowCascades), 1u, 0.5f, 0.0f};
    struct ShadowViewRec { uint8_t block[512]; std::vector<AwsmDraw> casters; };
    std::vector<ShadowViewRec> shadow_views;
};

namespace {

int fail(AwsmHost* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->last_error = buf;
    return code;
}

int dev_fail(AwsmHost* h, int rc, const char* where) {
    return fail(h, rc, "%s: %s", where, h->be.last_error ? h->be.last_error(h->ctx) : "device error");
}

// ---- write_gpu for a mirror with dirty ranges (e.g. transforms.rs:255-328, meshes.rs:1241-1346) ----
template <typename Buf>
int flush_buffer(AwsmHost* h, Buf& b, AwsmBuf which, bool& dirty) {
    if (!dirty) return AWSM_OK;
    bool resized = false;
    long long new_size = b.take_gpu_needs_resize();
    if (new_size >= 0 || !h->created[which]) {
        int rc = h->be.buffer_create(h->ctx, which, b.raw().size());   // gpu.create_buffer: replaces the old buffer wholesale
        if (rc) return dev_fail(h, rc, "buffer_create");
        h->created[which] = true;
        resized = true;
    }
    if (resized) {
        b.clear_dirty_ranges();
        if (!b.raw().empty()) {
            int rc = h->be.buffer_write(h->ctx, which, 0, b.raw().data(), b.raw().size());
            if (rc) return dev_fail(h, rc, "buffer_write(full)");
            h->upload_bytes += b.raw().size();
        }
    } else {
        for (const DirtyRange& r : write_plan(b.raw().size(), b.take_dirty_ranges())) {
            int rc = h->be.buffer_write(h->ctx, which, r.first, b.raw().data() + r.first, r.second);
            if (rc) return dev_fail(h, rc, "buffer_write(range)");
            h->upload_bytes += r.second;
        }
    }
    dirty = false;
    return AWSM_OK;
}

Mat4 to_matrix(const Transform& t) { return mat4_from_srt(t.s, t.r, t.t); }

void unset_parent(AwsmHost* h, SlotKey child) {
    auto it = h->parents.find(child);
    if (it == h->parents.end()) return;
    auto& ch = h->children[it->second];
    ch.erase(std::remove(ch.begin(), ch.end(), child), ch.end());
    h->parents.erase(it);
}

void set_parent(AwsmHost* h, SlotKey child, SlotKey parent) {   // transforms.rs:196-216
    if (child == h->root) return;
    if (parent == 0) parent = h->root;
    auto it = h->parents.find(child);
    if (it != h->parents.end()) {
        if (it->second == parent) return;
        unset_parent(h, child);
    }
    h->children[parent].push_back(child);
    h->parents[child] = parent;
}

bool update_inner(AwsmHost* h, SlotKey key, bool dirty_tracker) {   // transforms.rs:390-435
    const bool dirty = h->dirties.count(key) != 0 || dirty_tracker;
    if (dirty) {
        const Mat4 local = to_matrix(*h->locals.get(key));
        Mat4 w = local;
        auto pit = h->parents.find(key);
        if (pit != h->parents.end()) w = mat4_mul(h->world[pit->second], local);
        h->world[key] = w;
        h->transforms_buf.update(key, reinterpret_cast<const uint8_t*>(&w), 64);
        const Mat4 nm = mat4_transpose(mat4_inverse(w));
        const float n9[9] = {nm.c[0].x, nm.c[0].y, nm.c[0].z, nm.c[1].x, nm.c[1].y, nm.c[1].z, nm.c[2].x, nm.c[2].y, nm.c[2].z};
        h->normals_buf.update(key, reinterpret_cast<const uint8_t*>(n9), 36);
        h->dirty_meshes.push_back(key);
    }
    const std::vector<SlotKey> kids = h->children[key];
    for (SlotKey c : kids) update_inner(h, c, dirty);
    return dirty;
}

// ---- writer.rs:100-197 ----
void write_tex(AwsmHost* h, std::vector<uint8_t>& d, const AwsmHostTexRef& r) {
    if (r.texture < 0 || (size_t)r.texture >= h->tex_entries.size() || r.sampler >= h->samplers.size()) {
        d.insert(d.end(), 20, 0);   // Value::SkipTexture
        return;
    }
    const auto [ai, li] = h->tex_entries[r.texture];
    const AwsmHost::PoolArray& arr = h->pool[ai];
    const AwsmSampler& smp = h->samplers[r.sampler];
    push_u32(d, (arr.h << 16) | (arr.w & 0xFFFFu));
    push_u32(d, (li << 12) | (ai & 0xFFFu));
    push_u32(d, (r.sampler << 8) | (r.uv_index & 0xFFu));
    const uint32_t flags = 1u | 2u;   // bit 0 exists; bit 1 has mipmaps: pool arrays are always created with mipmap = true (texture_pool.rs:166-176, writer.rs:163-171)
    push_u32(d, flags | ((smp.address_mode_u & 0xFFu) << 8) | ((smp.address_mode_v & 0xFFu) << 16));
    long long toff = r.transform ? h->tex_transforms_buf.offset(r.transform) : -1;
    push_u32(d, (uint32_t)(toff >= 0 ? (size_t)toff : h->tex_transform_identity_offset));
}

std::vector<uint8_t> material_bytes(AwsmHost* h, const AwsmHostMaterial& m) {
    std::vector<uint8_t> d;
    d.reserve(256);
    if (m.shader == 2u) {   // unlit.rs:72-105
        push_u32(d, 2u); push_u32(d, m.alpha_mode); push_f32(d, m.alpha_mode == 1u ? m.alpha_cutoff : 0.0f);   // unlit.rs:72-105
        write_tex(h, d, m.base_color_tex);
        for (int i = 0; i < 4; i++) push_f32(d, m.base_color_factor[i]);
        write_tex(h, d, m.emissive_tex);
        for (int i = 0; i < 3; i++) push_f32(d, m.emissive_factor[i]);
        return d;
    }
    // pbr.rs:258-589
    push_u32(d, 1u); push_u32(d, m.alpha_mode); push_f32(d, m.alpha_mode == 1u ? m.alpha_cutoff : 0.0f);   // shader id, alpha_mode, alpha_cutoff (pbr.rs:268-269)
    write_tex(h, d, m.base_color_tex);
    for (int i = 0; i < 4; i++) push_f32(d, m.base_color_factor[i]);
    write_tex(h, d, m.metallic_roughness_tex);
    push_f32(d, m.metallic_factor); push_f32(d, m.roughness_factor);
    write_tex(h, d, m.normal_tex); push_f32(d, m.normal_scale);
    write_tex(h, d, m.occlusion_tex); push_f32(d, m.occlusion_strength);
    write_tex(h, d, m.emissive_tex);
    for (int i = 0; i < 3; i++) push_f32(d, m.emissive_factor[i]);
    push_u32(d, m.debug_bitmask);
    const size_t indices_offset = d.size();
    d.insert(d.end(), 48, 0);
    uint32_t fi[12] = {};
    auto cur = [&]() { return (uint32_t)(d.size() / 4 - 1); };   // pbr.rs:358-362: word index relative to the header
    if (m.has_vertex_color) { fi[0] = cur(); push_u32(d, m.vertex_color_set); }
    if (m.has_emissive_strength) { fi[1] = cur(); push_f32(d, m.emissive_strength); }
    if (m.has_ior) { fi[2] = cur(); push_f32(d, m.ior); }
    if (m.has_specular) {
        fi[3] = cur();
        write_tex(h, d, m.specular_tex); push_f32(d, m.specular_factor); write_tex(h, d, m.specular_color_tex);
        for (int i = 0; i < 3; i++) push_f32(d, m.specular_color_factor[i]);
    }
    if (m.has_transmission) { fi[4] = cur(); write_tex(h, d, m.transmission_tex); push_f32(d, m.transmission_factor); }
    if (m.has_diffuse_transmission) {   // pbr.rs:418-447
        fi[5] = cur();
        write_tex(h, d, m.diffuse_transmission_tex); push_f32(d, m.diffuse_transmission_factor); write_tex(h, d, m.diffuse_transmission_color_tex);
        for (int i = 0; i < 3; i++) push_f32(d, m.diffuse_transmission_color_factor[i]);
    }
    if (m.has_volume) {
        fi[6] = cur();
        write_tex(h, d, m.volume_thickness_tex); push_f32(d, m.volume_thickness_factor); push_f32(d, m.volume_attenuation_distance);
        for (int i = 0; i < 3; i++) push_f32(d, m.volume_attenuation_color[i]);
    }
    if (m.has_clearcoat) {
        fi[7] = cur();
        write_tex(h, d, m.clearcoat_tex); push_f32(d, m.clearcoat_factor);
        write_tex(h, d, m.clearcoat_roughness_tex); push_f32(d, m.clearcoat_roughness_factor);
        write_tex(h, d, m.clearcoat_normal_tex); push_f32(d, m.clearcoat_normal_scale);
    }
    if (m.has_sheen) {
        fi[8] = cur();
        write_tex(h, d, m.sheen_roughness_tex); push_f32(d, m.sheen_roughness_factor); write_tex(h, d, m.sheen_color_tex);
        for (int i = 0; i < 3; i++) push_f32(d, m.sheen_color_factor[i]);
    }
    if (m.has_dispersion) { fi[9] = cur(); push_f32(d, m.dispersion); }                         // pbr.rs:529-532
    if (m.has_anisotropy) {                                                                       // pbr.rs:534-551
        fi[10] = cur();
        write_tex(h, d, m.anisotropy_tex); push_f32(d, m.anisotropy_strength); push_f32(d, m.anisotropy_rotation);
    }
    if (m.has_iridescence) {                                                                      // pbr.rs:553-581
        fi[11] = cur();
        write_tex(h, d, m.iridescence_tex); push_f32(d, m.iridescence_factor); push_f32(d, m.iridescence_ior);
        write_tex(h, d, m.iridescence_thickness_tex); push_f32(d, m.iridescence_thickness_min); push_f32(d, m.iridescence_thickness_max);
    }
    memcpy(d.data() + indices_offset, fi, 48);
    return d;
}

void light_bytes(const AwsmHostLight& l, uint8_t out[64]) {   // lights.rs:354-473
    float f[16] = {};
    if (l.kind == 1u) { f[4] = l.direction[0]; f[5] = l.direction[1]; f[6] = l.direction[2]; }
    else { f[0] = l.position[0]; f[1] = l.position[1]; f[2] = l.position[2]; f[3] = l.range; }
    if (l.kind == 3u) { f[4] = l.direction[0]; f[5] = l.direction[1]; f[6] = l.direction[2]; f[7] = l.inner_angle; f[13] = l.outer_angle; }
    f[8] = l.color[0]; f[9] = l.color[1]; f[10] = l.color[2]; f[11] = l.intensity;
    f[12] = (float)l.kind;
    memcpy(out, f, 64);
}

void texture_transform_bytes(const float offset[2], const float origin[2], float rotation, const float scale[2], uint8_t out[32]) {   // textures.rs:247-284
    const float sx = scale[0], sy = scale[1], ox = offset[0], oy = offset[1], px = origin[0], py = origin[1];
    const float c = (float)std::cos((double)rotation), s = (float)std::sin((double)rotation);
    const float m00 = c * sx, m01 = s * sy, m10 = -s * sx, m11 = c * sy;
    const float bx = ox + px - (m00 * px + m01 * py);
    const float by = oy + py - (m10 * px + m11 * py);
    const float f[8] = {m00, m01, m10, m11, bx, by, 0.0f, 0.0f};
    memcpy(out, f, 32);
}

// f32::total_cmp key
int32_t total_key(float x) { int32_t b; memcpy(&b, &x, 4); return b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1); }

bool is_transparency_pass(const AwsmHostMaterial& m) {   // pbr.rs:213-224, unlit.rs:36-38
    if (m.alpha_mode == 1u || m.alpha_mode == 2u) return true;
    return m.shader != 2u && m.has_transmission && (m.transmission_factor > 0.0f || m.transmission_tex.texture >= 0);
}

void collect_draws(AwsmHost* h, std::vector<AwsmDraw>& out_opaque, std::vector<AwsmDraw>* transparent_out = nullptr,
                   std::vector<AwsmDraw>* hud_geometry_out = nullptr, std::vector<AwsmDraw>* hud_transparent_out = nullptr,
                   const Mat4* cull_view_proj = nullptr) {   // renderable.rs:38-150.  cull_view_proj: the frustum that culls instead of the camera's (the shadow casters: the light's); the order stays the camera's
    out_opaque.clear();
    if (transparent_out) transparent_out->clear();
    if (hud_geometry_out) hud_geometry_out->clear();
    if (hud_transparent_out) hud_transparent_out->clear();
    struct Item { SlotKey key; const MeshRec* rec; int pipeline; float closest; bool has_aabb; };
    std::vector<Item> items;
    const Mat4 view_proj = mat4_mul(h->cam_proj, h->cam_view);
    std::unique_ptr<Frustum> fr;
    if (cull_view_proj) fr.reset(new Frustum(*cull_view_proj));
    else if (h->have_camera) fr.reset(new Frustum(view_proj));
    const auto& keys = h->meshes.keys();
    const auto& vals = h->meshes.values();
    for (size_t i = 0; i < keys.size(); i++) {
        const MeshRec& m = vals[i];
        if (m.hidden) continue;
        if (fr && m.has_world_aabb && !fr->intersects(m.world_aabb)) continue;
        // pipeline key creation order (G/pipeline.rs:179-265): no_instancing {no_cull, back_cull, front_cull}, instancing {no_cull, back_cull, front_cull}
        Item it{keys[i], &m, (m.instanced ? 3 : 0) + (m.double_sided ? 0 : 1), 0.0f, m.has_world_aabb};
        if (m.has_world_aabb) {
            const float a = mat4_transform_point3(view_proj, m.world_aabb.min).z, b = mat4_transform_point3(view_proj, m.world_aabb.max).z;
            it.closest = std::fmin(a, b);
        }
        items.push_back(it);
    }
    std::vector<Item> tr_items, hud_items;   // renderable.rs:77-84: hud, else transparent by material, else opaque
    {
        std::vector<Item> op;
        for (const Item& it : items) (it.rec->hud ? hud_items : (it.rec->transparent ? tr_items : op)).push_back(it);
        items.swap(op);
    }
    if (h->have_camera) {
        std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
            if (a.pipeline != b.pipeline) return a.pipeline < b.pipeline;
            if (a.has_aabb && b.has_aabb) return total_key(a.closest) < total_key(b.closest);   // front to back
            if (a.has_aabb != b.has_aabb) return a.has_aabb;                                     // (Some, None) => Less
            return false;
        });
        auto back_to_front = [](const Item& a, const Item& b) {   // same pipeline grouping, then back to front (renderable.rs:89-90,131-135)
            if (a.pipeline != b.pipeline) return a.pipeline < b.pipeline;
            if (a.has_aabb && b.has_aabb) return total_key(b.closest) < total_key(a.closest);
            if (a.has_aabb != b.has_aabb) return a.has_aabb;
            return false;
        };
        std::stable_sort(tr_items.begin(), tr_items.end(), back_to_front);
        std::stable_sort(hud_items.begin(), hud_items.end(), back_to_front);
    }
    // pass 0: the geometry pass's list; 1: the world transparent pass's; 2 / 3: the hud list through the HUD geometry pass (visibility geometry)
    // and the HUD transparent pass (transparency geometry) — render.rs:169-178,301-312
    for (int pass = 0; pass < 4; pass++)
    for (const Item& it : (pass == 0 ? items : (pass == 1 ? tr_items : hud_items))) {
        std::vector<AwsmDraw>* outp = pass == 0 ? &out_opaque : (pass == 1 ? transparent_out : (pass == 2 ? hud_geometry_out : hud_transparent_out));
        if (!outp) break;
        std::vector<AwsmDraw>& out = *outp;
        AwsmDraw d{};
        d.geom_meta_off = (uint32_t)h->geom_meta.offset(it.key);
        d.vis_data_off = (uint32_t)((pass == 0 || pass == 2) ? it.rec->vis_off : it.rec->tr_off);
        d.tri_count = it.rec->tri_count;
        d.flags = it.rec->double_sided ? 0u : AWSM_DRAW_CULL_BACK;
        if (it.rec->instanced) {   // meshes/mesh.rs:91-121: instance buffer bound at the transform key's offset, draw_indexed_with_instance_count
            d.inst_off = (uint32_t)h->instances.offset(it.rec->transform_key);
            d.inst_count = h->instance_count[it.rec->transform_key];
            if (d.inst_count == 0) continue;
        }
        out.push_back(d);
    }
}

// One pool array whose host side changed (finalize_gpu_textures).  An array that is not on the device and whose layers need no conversion goes up
// whole, as it always did.  Otherwise the device does the work: the array grows there by doubling, and only the new or replaced
// images cross the bus and get their mip chains made.
int finalize_pool_array(AwsmHost* h, uint32_t i, uint32_t levels) {
    AwsmHost::PoolArray& a = h->pool[i];
    int rc;
    bool flagged = false;
    for (uint32_t f : a.flags) flagged = flagged || f != 0u;
    const bool run_time = !h->be.texture_pool_missing();
    if ((a.dev_layers == 0 && !flagged) || !run_time) {
        if (flagged || !a.resend.empty()) return fail(h, AWSM_ERR_UNSUPPORTED, "the backend library has no %s", h->be.texture_pool_missing());      // refused at insert / update already
        if ((rc = h->be.texture_array_upload(h->ctx, i, a.w, a.h, a.layers, levels, AWSM_TEX_RGBA8_UNORM, a.texels.data()))) return dev_fail(h, rc, "texture_array_upload");
        if ((rc = h->be.texture_array_generate_mips(h->ctx, i, a.kinds.data()))) return dev_fail(h, rc, "texture_array_generate_mips");
        a.dev_layers = a.sent_layers = a.layers;
        return AWSM_OK;
    }
    if (a.dev_layers == 0) {
        if ((rc = h->be.texture_array_create(h->ctx, i, a.w, a.h, a.layers, levels))) return dev_fail(h, rc, "texture_array_create");
        a.dev_layers = a.layers;
    } else if (a.layers > a.dev_layers) {
        // doubling; the lean gradient route wants fewer than 4096 layers, so the step stops at 4095 until the images themselves pass it
        uint64_t want = std::max<uint64_t>((uint64_t)a.dev_layers * 2u, a.layers);
        if (want > 4095u) want = std::max<uint64_t>(a.layers, std::min<uint64_t>(4095u, want));
        if ((rc = h->be.texture_array_resize_layers(h->ctx, i, (uint32_t)want))) return dev_fail(h, rc, "texture_array_resize_layers");
        a.dev_layers = (uint32_t)want;
    }
    const size_t bytes = (size_t)a.w * a.h * 4;
    auto send = [&](uint32_t first, uint32_t n) -> int {      // layers with one kind and one set of flags
        AwsmTexWrite w{};
        w.struct_size = sizeof w; w.format = 0u; w.flags = a.flags[first]; w.mipmap_kind = a.kinds[first];
        w.bytes_per_row = a.w * 4u; w.rows_per_image = a.h; w.offset = 0;
        int r = h->be.texture_array_write_layers(h->ctx, i, first, n, a.texels.data() + (size_t)first * bytes, (size_t)n * bytes, &w);
        if (r) return dev_fail(h, r, "texture_array_write_layers");
        h->upload_bytes += (uint64_t)n * bytes;
        return AWSM_OK;
    };
    std::sort(a.resend.begin(), a.resend.end());
    for (uint32_t l : a.resend) {
        if ((rc = send(l, 1u))) return rc;
        if ((rc = h->be.texture_array_generate_mips_layers(h->ctx, i, l, 1u))) return dev_fail(h, rc, "texture_array_generate_mips_layers");
    }
    a.resend.clear();
    for (uint32_t l = a.sent_layers; l < a.layers;) {
        uint32_t n = 1;
        while (l + n < a.layers && a.flags[l + n] == a.flags[l] && a.kinds[l + n] == a.kinds[l]) n++;
        if ((rc = send(l, n))) return rc;
        l += n;
    }
    if (a.layers > a.sent_layers && (rc = h->be.texture_array_generate_mips_layers(h->ctx, i, a.sent_layers, a.layers - a.sent_layers))) return dev_fail(h, rc, "texture_array_generate_mips_layers");
    a.sent_layers = a.layers;
    return AWSM_OK;
}

// skins.rs:162-194 for one record: world * inverse_bind of the joint, as the mirror holds it
Mat4 skin_matrix(AwsmHost* h, const AwsmHost::PoseRecord& r) {
    Mat4 wm = h->world[r.joint];
    auto ib = h->inverse_bind.find(r.joint);
    if (ib != h->inverse_bind.end()) wm = mat4_mul(wm, ib->second);
    return wm;
}

// Device posing: the matrices the device composed since the mirror was last looked at, composed here too (a cold path: awsm_host_mirror, and in
// front of a flush that may write the whole mirror).  The bytes are the device's, so nothing is marked dirty.
void sync_skin_mirror(AwsmHost* h) {
    for (uint32_t id : h->pose_stale) {
        const AwsmHost::PoseRecord& r = h->pose_records[id];
        if (!h->skin_matrices.contains(r.skin) || !h->world.count(r.joint)) continue;
        const Mat4 wm = skin_matrix(h, r);
        h->skin_matrices.write_untracked(r.skin, (size_t)r.joint_index * 64, reinterpret_cast<const uint8_t*>(&wm), 64);
    }
    h->pose_stale.clear();
}

// Device posing: everything the device has composed or was still to compose, settled on the host with the inverse bind matrices as they are now —
// the mirror brought up to date, and the joints not yet handed to the device composed here and marked for upload.  Called before anything changes
// what a record means (a skin insert replaces the inverse bind matrices of the joints it shares; posing is switched off).
void settle_pose_on_host(AwsmHost* h) {
    sync_skin_mirror(h);
    for (uint32_t id : h->pose_ids) {
        const AwsmHost::PoseRecord& r = h->pose_records[id];
        if (!h->skin_matrices.contains(r.skin) || !h->world.count(r.joint)) continue;
        const Mat4 wm = skin_matrix(h, r);
        h->skin_matrices.write_range(r.skin, (size_t)r.joint_index * 64, reinterpret_cast<const uint8_t*>(&wm), 64);
        h->skin_matrices_dirty = true;
    }
    h->pose_ids.clear();
}

AwsmSkinPoseRecord device_record(AwsmHost* h, const AwsmHost::PoseRecord& r) {
    AwsmSkinPoseRecord d{};
    const long long to = h->transforms_buf.offset(r.joint), mo = h->skin_matrices.offset(r.skin);      // a removed joint or skin is never listed again
    d.transform_offset = to < 0 ? 0u : (uint32_t)to;
    d.matrix_offset = mo < 0 ? 0u : (uint32_t)(mo + (long long)r.joint_index * 64);
    Mat4 ib = mat4_identity();
    auto it = h->inverse_bind.find(r.joint);
    if (it != h->inverse_bind.end()) ib = it->second;
    memcpy(d.inverse_bind, &ib, 64);
    return d;
}

// the records the device does not have yet, or has with an older inverse bind matrix
int send_pose_records(AwsmHost* h) {
    int rc;
    std::sort(h->pose_records_resend.begin(), h->pose_records_resend.end());
    for (uint32_t id : h->pose_records_resend) {
        if (id >= h->pose_records_sent) continue;
        const AwsmSkinPoseRecord d = device_record(h, h->pose_records[id]);
        if ((rc = h->be.skin_pose_records_write(h->ctx, id, 1u, &d))) return dev_fail(h, rc, "skin_pose_records_write");
        h->upload_bytes += sizeof d;
    }
    h->pose_records_resend.clear();
    const uint32_t total = (uint32_t)h->pose_records.size();
    if (h->pose_records_sent < total) {
        std::vector<AwsmSkinPoseRecord> recs;
        recs.reserve(total - h->pose_records_sent);
        for (uint32_t id = h->pose_records_sent; id < total; id++) recs.push_back(device_record(h, h->pose_records[id]));
        if ((rc = h->be.skin_pose_records_write(h->ctx, h->pose_records_sent, (uint32_t)recs.size(), recs.data()))) return dev_fail(h, rc, "skin_pose_records_write");
        h->upload_bytes += recs.size() * sizeof(AwsmSkinPoseRecord);
        h->pose_records_sent = total;
    }
    return AWSM_OK;
}

template <typename T>
bool load_sym(AwsmHost* h, T& fn, const char* name) {
    fn = reinterpret_cast<T>(dlsym(h->be.dl, name));
    if (!fn) { fail(h, AWSM_ERR_NOT_READY, "backend library lacks symbol %s", name); return false; }
    return true;
}

}  // namespace

extern "C" {

int awsm_host_create(const char* backend_path, int device, void* stream, uint32_t cfg_flags, AwsmHost** out) {
    if (!backend_path || !out) return AWSM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::unique_ptr<AwsmHost> h(new AwsmHost());
    h->be.dl = dlopen(backend_path, RTLD_NOW | RTLD_LOCAL);
    if (!h->be.dl) { fprintf(stderr, "awsm_host: cannot load backend %s: %s\n", backend_path, dlerror()); return AWSM_ERR_NOT_READY; }
    Backend& b = h->be;
    bool ok = load_sym(h.get(), b.create, "awsm_hip_create") && load_sym(h.get(), b.destroy, "awsm_hip_destroy") &&
              load_sym(h.get(), b.last_error, "awsm_hip_last_error") && load_sym(h.get(), b.abi_version, "awsm_hip_abi_version") &&
              load_sym(h.get(), b.buffer_create, "awsm_hip_buffer_create") && load_sym(h.get(), b.buffer_write, "awsm_hip_buffer_write") &&
              load_sym(h.get(), b.resize, "awsm_hip_resize") && load_sym(h.get(), b.set_shard_rows, "awsm_hip_set_shard_rows") && load_sym(h.get(), b.set_shard_bands, "awsm_hip_set_shard_bands") && load_sym(h.get(), b.set_stage_timers, "awsm_hip_set_stage_timers") && load_sym(h.get(), b.pick, "awsm_hip_pick") &&
              load_sym(h.get(), b.texture_array_upload, "awsm_hip_texture_array_upload") && load_sym(h.get(), b.texture_array_generate_mips, "awsm_hip_texture_array_generate_mips") && load_sym(h.get(), b.sampler_set, "awsm_hip_sampler_set") &&
              load_sym(h.get(), b.env_upload, "awsm_hip_env_upload") && load_sym(h.get(), b.env_cube_upload, "awsm_hip_env_cube_upload") && load_sym(h.get(), b.brdf_lut_generate, "awsm_hip_brdf_lut_generate") &&
              load_sym(h.get(), b.geometry_pass, "awsm_hip_geometry_pass") && load_sym(h.get(), b.opaque_pass, "awsm_hip_opaque_pass") && load_sym(h.get(), b.transparent_pass, "awsm_hip_transparent_pass") &&
              load_sym(h.get(), b.hud_geometry_pass, "awsm_hip_hud_geometry_pass") && load_sym(h.get(), b.hud_transparent_pass, "awsm_hip_hud_transparent_pass") &&
              load_sym(h.get(), b.frame_end, "awsm_hip_frame_end");
    if (!ok) { fprintf(stderr, "awsm_host: %s\n", h->last_error.c_str()); dlclose(b.dl); return AWSM_ERR_NOT_READY; }
    b.post_pass = reinterpret_cast<decltype(b.post_pass)>(dlsym(b.dl, "awsm_hip_post_pass"));      // optional (awsm_host_set_post_processing)
    b.editor_grid_defaults = reinterpret_cast<decltype(b.editor_grid_defaults)>(dlsym(b.dl, "awsm_hip_editor_grid_defaults"));      // optional (awsm_host_set_editor_grid)
    b.set_editor_grid = reinterpret_cast<decltype(b.set_editor_grid)>(dlsym(b.dl, "awsm_hip_set_editor_grid"));
    b.ssao_defaults = reinterpret_cast<decltype(b.ssao_defaults)>(dlsym(b.dl, "awsm_hip_ssao_defaults"));      // optional (awsm_host_set_ssao)
    b.set_ssao = reinterpret_cast<decltype(b.set_ssao)>(dlsym(b.dl, "awsm_hip_set_ssao"));
    b.set_taa = reinterpret_cast<decltype(b.set_taa)>(dlsym(b.dl, "awsm_hip_set_taa"));      // optional (awsm_host_set_taa)
    b.selection_defaults = reinterpret_cast<decltype(b.selection_defaults)>(dlsym(b.dl, "awsm_hip_selection_defaults"));      // optional (awsm_host_set_selection)
    b.set_selection = reinterpret_cast<decltype(b.set_selection)>(dlsym(b.dl, "awsm_hip_set_selection"));
    b.pick_ex = reinterpret_cast<decltype(b.pick_ex)>(dlsym(b.dl, "awsm_hip_pick_ex"));      // optional (awsm_host_pick_ex)
    b.pick_rect = reinterpret_cast<decltype(b.pick_rect)>(dlsym(b.dl, "awsm_hip_pick_rect"));      // optional (awsm_host_pick_rect)
    b.shadow_defaults = reinterpret_cast<decltype(b.shadow_defaults)>(dlsym(b.dl, "awsm_hip_shadow_defaults"));      // optional (awsm_host_set_shadow)
    b.shadow_pass = reinterpret_cast<decltype(b.shadow_pass)>(dlsym(b.dl, "awsm_hip_shadow_pass"));
    b.shadow_pass_views = reinterpret_cast<decltype(b.shadow_pass_views)>(dlsym(b.dl, "awsm_hip_shadow_pass_views"));
    b.env_cube_create = reinterpret_cast<decltype(b.env_cube_create)>(dlsym(b.dl, "awsm_hip_env_cube_create"));      // optional (awsm_host_env_cube_*)
    b.env_cube_write_face = reinterpret_cast<decltype(b.env_cube_write_face)>(dlsym(b.dl, "awsm_hip_env_cube_write_face"));
    b.env_cube_write_all_faces = reinterpret_cast<decltype(b.env_cube_write_all_faces)>(dlsym(b.dl, "awsm_hip_env_cube_write_all_faces"));
    b.env_cube_generate_mips = reinterpret_cast<decltype(b.env_cube_generate_mips)>(dlsym(b.dl, "awsm_hip_env_cube_generate_mips"));
    b.env_cube_fill_colors = reinterpret_cast<decltype(b.env_cube_fill_colors)>(dlsym(b.dl, "awsm_hip_env_cube_fill_colors"));
    b.env_cube_fill_sky_gradient = reinterpret_cast<decltype(b.env_cube_fill_sky_gradient)>(dlsym(b.dl, "awsm_hip_env_cube_fill_sky_gradient"));
    b.env_cube_filter = reinterpret_cast<decltype(b.env_cube_filter)>(dlsym(b.dl, "awsm_hip_env_cube_filter"));
    b.env_cube_from_equirect = reinterpret_cast<decltype(b.env_cube_from_equirect)>(dlsym(b.dl, "awsm_hip_env_cube_from_equirect"));
    b.texture_array_create = reinterpret_cast<decltype(b.texture_array_create)>(dlsym(b.dl, "awsm_hip_texture_array_create"));      // optional (the texture pool at run time)
    b.texture_array_resize_layers = reinterpret_cast<decltype(b.texture_array_resize_layers)>(dlsym(b.dl, "awsm_hip_texture_array_resize_layers"));
    b.texture_array_write_layers = reinterpret_cast<decltype(b.texture_array_write_layers)>(dlsym(b.dl, "awsm_hip_texture_array_write_layers"));
    b.texture_array_generate_mips_layers = reinterpret_cast<decltype(b.texture_array_generate_mips_layers)>(dlsym(b.dl, "awsm_hip_texture_array_generate_mips_layers"));
    b.texture_array_info = reinterpret_cast<decltype(b.texture_array_info)>(dlsym(b.dl, "awsm_hip_texture_array_info"));
    b.skin_pose_records_write = reinterpret_cast<decltype(b.skin_pose_records_write)>(dlsym(b.dl, "awsm_hip_skin_pose_records_write"));      // optional (awsm_host_set_device_skin_posing)
    b.skin_pose = reinterpret_cast<decltype(b.skin_pose)>(dlsym(b.dl, "awsm_hip_skin_pose"));
    if (b.abi_version() != AWSM_HIP_ABI_VERSION) { dlclose(b.dl); return AWSM_ERR_INVALID_ARGUMENT; }
    AwsmConfig cfg{};
    cfg.struct_size = sizeof cfg; cfg.abi_version = AWSM_HIP_ABI_VERSION; cfg.device = device; cfg.flags = cfg_flags; cfg.stream = stream;
    int rc = b.create(&cfg, &h->ctx);
    if (rc) { dlclose(b.dl); return rc; }
    // Transforms::new (transforms.rs:64-110): root node, identity world, no buffer slot
    h->root = h->locals.insert(Transform{{0, 0, 0}, {0, 0, 0, 1}, {1, 1, 1}});
    h->world[h->root] = mat4_identity();
    h->children[h->root] = {};
    // Textures::new (textures.rs:311-320): identity texture transform pre-inserted
    {
        SlotKey k = h->tex_transform_keys.insert(0);
        const float z2[2] = {0, 0}, o2[2] = {1, 1};
        uint8_t bytes[32];
        texture_transform_bytes(z2, z2, 0.0f, o2, bytes);
        h->tex_transforms_buf.update(k, bytes, 32);
        h->tex_transform_identity_offset = (size_t)h->tex_transforms_buf.offset(k);
    }
    *out = h.release();
    return AWSM_OK;
}

int awsm_host_destroy(AwsmHost* h) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (h->ctx) h->be.destroy(h->ctx);
    if (h->be.dl) dlclose(h->be.dl);
    delete h;
    return AWSM_OK;
}

const char* awsm_host_last_error(const AwsmHost* h) { return h ? h->last_error.c_str() : "null host"; }
void* awsm_host_device_ctx(AwsmHost* h) { return h ? h->ctx : nullptr; }

// ------------------------------------------------------------------------------------------------ transforms
AwsmKey awsm_host_transform_root(AwsmHost* h) { return h->root; }

AwsmKey awsm_host_transform_insert(AwsmHost* h, const float t[3], const float r[4], const float s[3], AwsmKey parent) {   // transforms.rs:112-127
    Transform tr{{t[0], t[1], t[2]}, {r[0], r[1], r[2], r[3]}, {s[0], s[1], s[2]}};
    SlotKey key = h->locals.insert(tr);
    h->world[key] = to_matrix(tr);
    h->children[key] = {};
    h->dirties.insert(key);
    const uint8_t zeros[64] = {};
    h->transforms_buf.update(key, zeros, 64);
    h->normals_buf.update(key, zeros, 36);
    set_parent(h, key, parent);
    return key;
}

int awsm_host_transform_set_local(AwsmHost* h, AwsmKey key, const float t[3], const float r[4], const float s[3]) {   // transforms.rs:176-190
    if (key == h->root) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] cannot modify root node");
    Transform* tr = h->locals.get(key);
    if (!tr) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] local transform does not exist");
    *tr = Transform{{t[0], t[1], t[2]}, {r[0], r[1], r[2], r[3]}, {s[0], s[1], s[2]}};
    h->dirties.insert(key);
    return AWSM_OK;
}

int awsm_host_transform_set_parent(AwsmHost* h, AwsmKey child, AwsmKey parent) {
    if (!h->locals.contains(child) || (parent && !h->locals.contains(parent))) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] unknown key");
    set_parent(h, child, parent);   // like the reference, re-parenting alone does not mark the node dirty
    return AWSM_OK;
}

int awsm_host_transform_remove(AwsmHost* h, AwsmKey key) {   // transforms.rs:137-151
    if (key == h->root) return AWSM_OK;
    if (!h->locals.contains(key)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] unknown key");
    unset_parent(h, key);
    h->locals.remove(key);
    h->world.erase(key);
    h->children.erase(key);
    h->dirties.erase(key);
    h->transforms_buf.remove(key);
    h->normals_buf.remove(key);
    h->transforms_gpu_dirty = true;
    return AWSM_OK;
}

AwsmKey awsm_host_transform_parent(AwsmHost* h, AwsmKey child) { auto it = h->parents.find(child); return it == h->parents.end() ? 0 : it->second; }

int awsm_host_transform_world(AwsmHost* h, AwsmKey key, float out[16]) {
    auto it = h->world.find(key);
    if (it == h->world.end()) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] world transform does not exist");
    memcpy(out, &it->second, 64);
    return AWSM_OK;
}

int awsm_host_transform_get_local(AwsmHost* h, AwsmKey key, float t[3], float r[4], float s[3]) {   // transforms.rs:229-233
    const Transform* tr = h->locals.get(key);
    if (!tr) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] local transform does not exist");
    if (t) { t[0] = tr->t.x; t[1] = tr->t.y; t[2] = tr->t.z; }
    if (r) { r[0] = tr->r.x; r[1] = tr->r.y; r[2] = tr->r.z; r[3] = tr->r.w; }
    if (s) { s[0] = tr->s.x; s[1] = tr->s.y; s[2] = tr->s.z; }
    return AWSM_OK;
}

AwsmKey awsm_host_transform_duplicate(AwsmHost* h, AwsmKey key) {   // transforms.rs:151-155
    const Transform* tr = h->locals.get(key);
    if (!tr) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] local transform does not exist"); return 0; }
    const Transform copy = *tr;
    const float t[3] = {copy.t.x, copy.t.y, copy.t.z}, r[4] = {copy.r.x, copy.r.y, copy.r.z, copy.r.w}, s[3] = {copy.s.x, copy.s.y, copy.s.z};
    auto pit = h->parents.find(key);      // get_parent(key).ok(): the root has none, and insert(.., None) parents to the root
    return awsm_host_transform_insert(h, t, r, s, pit == h->parents.end() ? 0 : pit->second);
}

// ------------------------------------------------------------------------------------------------ textures
int awsm_host_texture_insert(AwsmHost* h, const uint8_t* rgba8, uint32_t w, uint32_t ht) { return awsm_host_texture_insert_kind(h, rgba8, w, ht, 0u); }

// TexturePool::add_image with TextureColorInfo{mipmap_kind} (gltf/populate/material.rs:128-260): the kind selects the
// filter the array's mip generation applies to this layer.
int awsm_host_texture_insert_kind(AwsmHost* h, const uint8_t* rgba8, uint32_t w, uint32_t ht, uint32_t mipmap_kind) {
    if (!rgba8 || !w || !ht || w > 0xFFFF || ht > 0xFFFF) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "texture_insert: bad image");
    uint32_t ai = 0;
    for (; ai < h->pool.size(); ai++) if (h->pool[ai].w == w && h->pool[ai].h == ht) break;
    if (ai == h->pool.size()) {
        if (h->pool.size() >= 64) return fail(h, AWSM_ERR_UNSUPPORTED, "more than 64 pool arrays");
        AwsmHost::PoolArray fresh; fresh.w = w; fresh.h = ht;
        h->pool.push_back(std::move(fresh));
    }
    AwsmHost::PoolArray& a = h->pool[ai];
    a.texels.insert(a.texels.end(), rgba8, rgba8 + (size_t)w * ht * 4);
    a.kinds.push_back(mipmap_kind);
    a.flags.push_back(0u); a.desc_flags.push_back(0u);
    a.dirty = true;
    h->tex_entries.push_back({ai, a.layers});
    a.layers++;
    return (int)h->tex_entries.size() - 1;
}

int awsm_host_texture_insert_ex(AwsmHost* h, const uint8_t* rgba8, uint32_t w, uint32_t ht, const AwsmHostTextureDesc* desc) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!desc || desc->struct_size != sizeof(AwsmHostTextureDesc)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "texture_insert_ex: a desc with struct_size %zu is missing", sizeof(AwsmHostTextureDesc));
    const uint32_t flags = (desc->premultiply_alpha ? (uint32_t)AWSM_TEX_PREMULTIPLY_ALPHA : 0u) | (desc->srgb_to_linear ? (uint32_t)AWSM_TEX_SRGB_TO_LINEAR : 0u);
    if (flags && h->be.texture_pool_missing())
        return fail(h, AWSM_ERR_UNSUPPORTED, "texture_insert_ex: srgb_to_linear / premultiply_alpha need %s, which the backend library lacks", h->be.texture_pool_missing());
    const int id = awsm_host_texture_insert_kind(h, rgba8, w, ht, desc->mipmap_kind);
    if (id < 0) return id;
    AwsmHost::PoolArray& a = h->pool[h->tex_entries[(size_t)id].first];
    a.flags.back() = flags; a.desc_flags.back() = flags;
    return id;
}

int awsm_host_texture_update(AwsmHost* h, int texture_id, const uint8_t* rgba8) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!rgba8 || texture_id < 0 || (size_t)texture_id >= h->tex_entries.size()) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "texture_update: no pixels, or no texture %d", texture_id);
    if (h->be.texture_pool_missing()) return fail(h, AWSM_ERR_UNSUPPORTED, "texture_update: the backend library has no %s", h->be.texture_pool_missing());
    const auto [ai, li] = h->tex_entries[(size_t)texture_id];
    AwsmHost::PoolArray& a = h->pool[ai];
    const size_t bytes = (size_t)a.w * a.h * 4;
    memcpy(a.texels.data() + (size_t)li * bytes, rgba8, bytes);
    a.flags[li] = a.desc_flags[li];
    if (li < a.sent_layers && std::find(a.resend.begin(), a.resend.end(), li) == a.resend.end()) a.resend.push_back(li);
    a.dirty = true;
    return AWSM_OK;
}

int awsm_host_sampler_insert(AwsmHost* h, const AwsmSampler* s) {
    if (!s || h->samplers.size() >= 32) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "sampler_insert: bad argument / more than 32 samplers");
    int rc = h->be.sampler_set(h->ctx, (uint32_t)h->samplers.size(), s);
    if (rc) return dev_fail(h, rc, "sampler_set");
    h->samplers.push_back(*s);
    return (int)h->samplers.size() - 1;
}

AwsmKey awsm_host_texture_transform_insert(AwsmHost* h, const float offset[2], const float origin[2], float rotation, const float scale[2]) {
    SlotKey k = h->tex_transform_keys.insert(0);
    uint8_t bytes[32];
    texture_transform_bytes(offset, origin, rotation, scale, bytes);
    h->tex_transforms_buf.update(k, bytes, 32);
    h->tex_transforms_dirty = true;
    return k;
}

// ------------------------------------------------------------------------------------------------ materials
// The caller's struct may be shorter than this library's (AwsmHostMaterial.struct_size: fields are only appended): read what it has, the rest
// means "block absent" (has_* = 0, no texture).
static bool material_in(AwsmHost* h, const AwsmHostMaterial* in, AwsmHostMaterial* full, const char* who) {
    if (!in || in->struct_size < offsetof(AwsmHostMaterial, has_vertex_color) || in->struct_size > 4096u) {
        fail(h, AWSM_ERR_INVALID_ARGUMENT, "%s: AwsmHostMaterial.struct_size = %u (set it to sizeof(AwsmHostMaterial))", who, in ? in->struct_size : 0u);
        return false;
    }
    memset(full, 0, sizeof *full);
    AwsmHostTexRef none; none.texture = -1; none.sampler = 0; none.uv_index = 0; none.pad = 0; none.transform = 0;
    AwsmHostTexRef* refs[] = {&full->specular_tex, &full->specular_color_tex, &full->transmission_tex, &full->volume_thickness_tex, &full->clearcoat_tex, &full->clearcoat_roughness_tex,
                              &full->clearcoat_normal_tex, &full->sheen_roughness_tex, &full->sheen_color_tex, &full->diffuse_transmission_tex, &full->diffuse_transmission_color_tex,
                              &full->anisotropy_tex, &full->iridescence_tex, &full->iridescence_thickness_tex};
    for (AwsmHostTexRef* r : refs) *r = none;
    memcpy(full, in, std::min<size_t>(in->struct_size, sizeof *full));
    full->struct_size = (uint32_t)sizeof *full;
    return true;
}

uint32_t awsm_host_abi_version(void) { return AWSM_HOST_ABI_VERSION; }

AwsmKey awsm_host_material_insert(AwsmHost* h, const AwsmHostMaterial* m_in) {   // materials.rs:120-128
    AwsmHostMaterial mfull;
    if (!material_in(h, m_in, &mfull, "material_insert")) return 0;
    const AwsmHostMaterial* m = &mfull;
    if (m->shader != 1u && m->shader != 2u) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "material_insert: bad shader id"); return 0; }
    SlotKey k = h->materials.insert(*m);
    const std::vector<uint8_t> d = material_bytes(h, *m);
    h->materials_buf.update(k, d.data(), d.size());
    h->materials_dirty = true;
    return k;
}

int awsm_host_material_update(AwsmHost* h, AwsmKey key, const AwsmHostMaterial* m_in) {   // materials.rs:147-186
    AwsmHostMaterial* cur = h->materials.get(key);
    if (!cur || !m_in) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[material] not found");
    AwsmHostMaterial mfull;
    if (!material_in(h, m_in, &mfull, "material_update")) return AWSM_ERR_INVALID_ARGUMENT;
    const AwsmHostMaterial* m = &mfull;
    *cur = *m;
    const std::vector<uint8_t> d = material_bytes(h, *m);
    h->materials_buf.update(key, d.data(), d.size());
    h->materials_dirty = true;
    return AWSM_OK;
}

int64_t awsm_host_material_offset(AwsmHost* h, AwsmKey key) { return h->materials_buf.offset(key); }

// ------------------------------------------------------------------------------------------------ skins
AwsmKey awsm_host_skin_insert(AwsmHost* h, const AwsmKey* joints, uint32_t n_joints, const float* inverse_bind, uint32_t set_count,
                              const uint32_t* const* joints_per_set, const float* const* weights_per_set, uint32_t vertex_count) {
    if (!joints || !n_joints || !set_count || !joints_per_set || !weights_per_set) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "skin_insert: bad argument"); return 0; }
    // before inverse_bind changes below: what was composed, or is still to be, with the matrices of the earlier skins is theirs (and the insert
    // may grow the buffer, after which the whole mirror goes up)
    if (h->device_posing) settle_pose_on_host(h);
    std::vector<uint8_t> fill;
    std::vector<SlotKey> jv(joints, joints + n_joints);
    for (uint32_t j = 0; j < n_joints; j++) {   // skins.rs:84-143
        Mat4 m = mat4_identity();
        if (inverse_bind) memcpy(&m, inverse_bind + (size_t)j * 16, 64);
        const uint8_t* p = reinterpret_cast<const uint8_t*>(&m);
        fill.insert(fill.end(), p, p + 64);
        h->inverse_bind[joints[j]] = m;
    }
    SlotKey sk = h->skins.insert(jv);
    h->skin_matrices.update(sk, fill.data(), fill.size());
    for (uint32_t j = 0; j < n_joints; j++) {
        std::vector<uint32_t>& ids = h->joint_records[joints[j]];
        for (uint32_t id : ids) h->pose_records_resend.push_back(id);      // inverse_bind is keyed by the joint: an earlier skin's record now has this one's
        ids.push_back((uint32_t)h->pose_records.size());
        h->pose_records.push_back({sk, joints[j], j});
    }
    h->skin_sets[sk] = set_count;
    // gltf/buffers/skin.rs:22-113: per vertex, per set, 4 x {u32 joint, f32 weight}
    std::vector<uint8_t> iw((size_t)vertex_count * set_count * 32);
    for (uint32_t v = 0; v < vertex_count; v++)
        for (uint32_t s = 0; s < set_count; s++)
            for (int k = 0; k < 4; k++) {
                uint8_t* dst = iw.data() + (((size_t)v * set_count + s) * 4 + k) * 8;
                memcpy(dst, &joints_per_set[s][(size_t)v * 4 + k], 4);
                memcpy(dst + 4, &weights_per_set[s][(size_t)v * 4 + k], 4);
            }
    h->skin_index_weights.update(sk, iw.data(), iw.size());
    h->skin_matrices_dirty = h->skin_iw_dirty = true;
    return sk;
}

int64_t awsm_host_skin_matrices_offset(AwsmHost* h, AwsmKey skin) { return h->skin_matrices.offset(skin); }   // skins.rs:146-152

// ------------------------------------------------------------------------------------------------ meshes
static AwsmKey mesh_insert_impl(AwsmHost* h, const AwsmHostPrimitive* p, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden, bool hud);
AwsmKey awsm_host_mesh_insert(AwsmHost* h, const AwsmHostPrimitive* p, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden) {
    return mesh_insert_impl(h, p, transform, material, skin, hidden, false);
}
// Mesh.hud = true (meshes/mesh.rs:28; the glTF loader's hints.hud): the mesh carries BOTH geometries (gltf/buffers/mesh.rs:37-39), its
// MaterialMeshMeta says is_hud (material_meta.rs:181-182), and render() draws it in the two HUD passes instead of the world's.
AwsmKey awsm_host_mesh_insert_hud(AwsmHost* h, const AwsmHostPrimitive* p, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden) {
    return mesh_insert_impl(h, p, transform, material, skin, hidden, true);
}
static AwsmKey mesh_insert_impl(AwsmHost* h, const AwsmHostPrimitive* p, AwsmKey transform, AwsmKey material, AwsmKey skin, uint32_t hidden, bool hud) {
    if (!p || !p->positions || !p->normals || !p->indices || !p->vertex_count) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "mesh_insert: bad primitive"); return 0; }
    if (!h->locals.contains(transform) || transform == h->root) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] buffer slot missing"); return 0; }
    const AwsmHostMaterial* mat = h->materials.get(material);
    if (!mat) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "[material] not found"); return 0; }
    if (skin && !h->skins.contains(skin)) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "[skin] not found"); return 0; }
    if (p->n_uv_sets > 8 || p->n_color_sets > 4) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "mesh_insert: too many attribute sets"); return 0; }
    const uint32_t V = p->vertex_count, T = p->triangle_count;
    for (size_t i = 0; i < (size_t)T * 3; i++) if (p->indices[i] >= V) { fail(h, AWSM_ERR_OUT_OF_RANGE, "mesh_insert: index %u >= vertex count %u", p->indices[i], V); return 0; }

    // ---- populate/mesh.rs:107-160: morph first, then (already inserted) skin ----
    SlotKey morph_key = 0;
    if (p->n_morph_targets) {
        const uint32_t nt = p->n_morph_targets;
        std::vector<float> weights(nt, 0.0f);
        if (p->morph_weights) memcpy(weights.data(), p->morph_weights, nt * 4);
        std::vector<float> values((size_t)V * nt * 10, 0.0f);   // gltf/buffers/morph.rs:31-190
        for (uint32_t v = 0; v < V; v++)
            for (uint32_t t = 0; t < nt; t++) {
                float* dst = values.data() + ((size_t)v * nt + t) * 10;
                const AwsmHostMorphTarget& mt = p->morph_targets[t];
                if (mt.positions) memcpy(dst, mt.positions + (size_t)v * 3, 12);
                if (mt.normals) memcpy(dst + 3, mt.normals + (size_t)v * 3, 12);
                if (mt.tangents) memcpy(dst + 6, mt.tangents + (size_t)v * 3, 12);
            }
        morph_key = h->morphs.insert(nt);
        h->morph_weights.update(morph_key, reinterpret_cast<const uint8_t*>(weights.data()), nt * 4);   // morphs.rs:148-170 insert_raw
        h->morph_values.update(morph_key, reinterpret_cast<const uint8_t*>(values.data()), values.size() * 4);
        if (p->animated_morph_weights) {   // morphs.rs:197-217: the callback sees [1..n+1) of the block
            const float* aw = p->animated_morph_weights;
            h->morph_weights.update_with_unchecked(morph_key, [&](size_t, uint8_t* blk, size_t) { memcpy(blk + 4, aw, nt * 4); });
        }
        h->morph_weights_dirty = h->morph_values_dirty = true;
    }

    // ---- gltf/buffers/mesh.rs:33-57: visibility geometry XOR transparency geometry, by the material ----
    const bool transparent = is_transparency_pass(*mat);
    const bool need_vis = !transparent || hud, need_tr = transparent || hud;
    // ---- gltf/buffers/mesh/visibility.rs:35-165: vertex explosion, 56 B / corner ----
    std::vector<uint8_t> vis(need_vis ? (size_t)T * 3 * 56 : 0);
    static const float kBary[3][2] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {0.0f, 0.0f}};
    const float default_tangent[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    for (uint32_t t = 0; t < T && need_vis; t++) {
        uint32_t vi[3] = {p->indices[t * 3], p->indices[t * 3 + 1], p->indices[t * 3 + 2]};
        int bi[3] = {0, 1, 2};
        if (p->front_face_cw) { std::swap(vi[1], vi[2]); std::swap(bi[1], bi[2]); }
        for (int c = 0; c < 3; c++) {
            uint8_t* dst = vis.data() + ((size_t)t * 3 + c) * 56;
            memcpy(dst, p->positions + (size_t)vi[c] * 3, 12);
            memcpy(dst + 12, &t, 4);
            memcpy(dst + 16, kBary[bi[c]], 8);
            memcpy(dst + 24, p->normals + (size_t)vi[c] * 3, 12);
            memcpy(dst + 36, p->tangents ? p->tangents + (size_t)vi[c] * 4 : default_tangent, 16);
            memcpy(dst + 52, &vi[c], 4);
        }
    }
    // ---- gltf/buffers/attributes.rs:113-160: COLOR_n then TEXCOORD_n, per original vertex ----
    const uint32_t stride_f = p->n_color_sets * 4 + p->n_uv_sets * 2;
    std::vector<float> attr((size_t)V * stride_f);
    for (uint32_t v = 0; v < V; v++) {
        float* dst = attr.data() + (size_t)v * stride_f;
        for (uint32_t c = 0; c < p->n_color_sets; c++) { memcpy(dst, p->color_sets[c] + (size_t)v * 4, 16); dst += 4; }
        for (uint32_t u = 0; u < p->n_uv_sets; u++) { memcpy(dst, p->uv_sets[u] + (size_t)v * 2, 8); dst += 2; }
    }
    // ---- meshes.rs:486-560 insert_resource: vis index, vis data, attr index, attr data ----
    SlotKey rk = h->resources.insert(0);
    size_t vis_off = 0, tr_off = 0;
    if (need_vis) {
        std::vector<uint32_t> ident((size_t)T * 3);
        for (size_t i = 0; i < ident.size(); i++) ident[i] = (uint32_t)i;
        h->vis_index.update(rk, reinterpret_cast<const uint8_t*>(ident.data()), ident.size() * 4);
        vis_off = h->vis_data.update(rk, vis.data(), vis.size());
    }
    if (need_tr) {   // gltf/buffers/mesh/transparency.rs:31-175: 40 B per ORIGINAL vertex, drawn through the custom-attribute indices
        std::vector<uint8_t> tv((size_t)V * 40);
        for (uint32_t v = 0; v < V; v++) {
            uint8_t* dst = tv.data() + (size_t)v * 40;
            memcpy(dst, p->positions + (size_t)v * 3, 12);
            memcpy(dst + 12, p->normals + (size_t)v * 3, 12);
            memcpy(dst + 24, p->tangents ? p->tangents + (size_t)v * 4 : default_tangent, 16);
        }
        tr_off = h->tr_data.update(rk, tv.data(), tv.size());
        h->tr_data_dirty = true;
    }
    const size_t attr_index_off = h->attr_index.update(rk, reinterpret_cast<const uint8_t*>(p->indices), (size_t)T * 12);
    const size_t attr_data_off = h->attr_data.update(rk, reinterpret_cast<const uint8_t*>(attr.data()), attr.size() * 4);
    h->vis_index_dirty = h->vis_data_dirty = h->attr_index_dirty = h->attr_data_dirty = true;

    MeshRec rec;
    rec.transform_key = transform; rec.material_key = material; rec.resource_key = rk; rec.skin_key = skin; rec.morph_key = morph_key;
    rec.double_sided = mat->double_sided != 0; rec.hidden = hidden != 0; rec.tri_count = T; rec.vis_off = vis_off; rec.transparent = transparent; rec.tr_off = tr_off;
    rec.hud = hud;
    if (transparent && !hud) { h->n_world_transparent_meshes++; h->has_transparent_meshes = true; }
    if (hud) { h->n_hud_meshes++; h->has_hud_meshes = true; }
    Vec3 mn = {p->positions[0], p->positions[1], p->positions[2]}, mx = mn;   // accessor min/max (populate/mesh.rs try_position_aabb)
    for (uint32_t v = 1; v < V; v++) {
        const Vec3 q = {p->positions[(size_t)v * 3], p->positions[(size_t)v * 3 + 1], p->positions[(size_t)v * 3 + 2]};
        mn = v3_min(mn, q); mx = v3_max(mx, q);
    }
    rec.local_aabb = {mn, mx};
    rec.world_aabb = rec.local_aabb;   // meshes.rs:596-598: until the next update_world
    SlotKey mk = h->meshes.insert(rec);
    h->transform_to_meshes[transform].push_back(mk);

    // ---- meta.rs:89-146: material meta first, then geometry meta ----
    const uint32_t hi = (uint32_t)(mk >> 32), lo = (uint32_t)(mk & 0xFFFFFFFFull);
    const uint32_t mm[17] = {hi, lo, 0, 0, 0, 0, (uint32_t)h->materials_buf.offset(material), (uint32_t)h->transforms_buf.offset(transform),
                             (uint32_t)h->normals_buf.offset(transform), (uint32_t)attr_index_off, (uint32_t)attr_data_off, stride_f * 4,
                             p->n_color_sets * 4, p->n_uv_sets, p->n_color_sets, (uint32_t)vis_off, hud ? 1u : 0u};      // last: is_hud
    h->material_meta.update(mk, reinterpret_cast<const uint8_t*>(mm), 68);
    uint32_t gm[10] = {hi, lo, 0, 0, 0, 0, 0, 0, (uint32_t)h->transforms_buf.offset(transform), (uint32_t)h->material_meta.offset(mk)};
    if (morph_key) { gm[2] = p->n_morph_targets; gm[3] = (uint32_t)h->morph_weights.offset(morph_key); gm[4] = (uint32_t)h->morph_values.offset(morph_key); }
    if (skin) { gm[5] = h->skin_sets[skin]; gm[6] = (uint32_t)h->skin_matrices.offset(skin); gm[7] = (uint32_t)h->skin_index_weights.offset(skin); }
    h->geom_meta.update(mk, reinterpret_cast<const uint8_t*>(gm), 40);
    h->geom_meta_dirty = h->material_meta_dirty = true;
    return mk;
}

int awsm_host_mesh_remove(AwsmHost* h, AwsmKey mesh) {
    MeshRec* rec = h->meshes.get(mesh);
    if (!rec) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[mesh] not found");
    const SlotKey rk = rec->resource_key, tk = rec->transform_key, mk = rec->morph_key;
    h->vis_index.remove(rk); h->vis_data.remove(rk); h->tr_data.remove(rk); h->attr_index.remove(rk); h->attr_data.remove(rk);
    if (rec->transparent || rec->hud) h->tr_data_dirty = true;
    if (rec->hud) { if (h->n_hud_meshes) h->n_hud_meshes--; h->has_hud_meshes = h->n_hud_meshes != 0; }
    else if (rec->transparent) { if (h->n_world_transparent_meshes) h->n_world_transparent_meshes--; h->has_transparent_meshes = h->n_world_transparent_meshes != 0; }
    h->resources.remove(rk);
    if (mk) { h->morph_weights.remove(mk); h->morph_values.remove(mk); h->morphs.remove(mk); h->morph_weights_dirty = h->morph_values_dirty = true; }
    auto& v = h->transform_to_meshes[tk];
    v.erase(std::remove(v.begin(), v.end(), mesh), v.end());
    if (h->geom_meta.remove(mesh)) h->geom_meta_dirty = true;
    if (h->material_meta.remove(mesh)) h->material_meta_dirty = true;
    h->meshes.remove(mesh);
    h->vis_index_dirty = h->vis_data_dirty = h->attr_index_dirty = h->attr_data_dirty = true;
    return AWSM_OK;
}

int awsm_host_mesh_update_morph_weights(AwsmHost* h, AwsmKey mesh, const float* weights, uint32_t n) {   // morphs.rs:197-217
    const MeshRec* rec = h->meshes.get(mesh);
    if (!rec) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[mesh] not found");
    const uint32_t* targets = rec->morph_key ? h->morphs.get(rec->morph_key) : nullptr;
    if (!targets) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "mesh_update_morph_weights: the mesh has no morph targets");
    if (n != *targets || !weights) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "mesh_update_morph_weights: %u weights for %u targets", n, *targets);
    // the callback sees floats [1, n + 1) of the block (the reference's offset-by-one, kept: DESIGN.md section 3)
    h->morph_weights.update_with_unchecked(rec->morph_key, [&](size_t, uint8_t* blk, size_t) { memcpy(blk + 4, weights, (size_t)n * 4); });
    h->morph_weights_dirty = true;
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ instancing (meshes.rs:176-290, instances.rs)
static std::vector<uint8_t> instance_bytes(const Transform* list, size_t n) {   // Instances::transforms_to_bytes: to_matrix().to_cols_array() each
    std::vector<uint8_t> out(n * 64);
    for (size_t i = 0; i < n; i++) { const Mat4 m = to_matrix(list[i]); memcpy(out.data() + i * 64, &m, 64); }
    return out;
}
static Transform trs_at(const float* trs10, size_t i) {
    const float* p = trs10 + i * 10;
    return Transform{{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}, {p[7], p[8], p[9]}};
}
// Meshes::enable_mesh_instancing (first call) / set_mesh_instances (later calls): `n` transforms as 10 floats each
// (translation xyz, rotation xyzw, scale xyz)
int awsm_host_mesh_set_instances(AwsmHost* h, AwsmKey mesh, const float* trs10, uint32_t n) {
    MeshRec* rec = h->meshes.get(mesh);
    if (!rec || (!trs10 && n)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[mesh] not found / null transforms");
    rec->instanced = true;
    std::vector<Transform> list(n);
    for (uint32_t i = 0; i < n; i++) list[i] = trs_at(trs10, i);
    const std::vector<uint8_t> bytes = instance_bytes(list.data(), n);
    h->instances.update(rec->transform_key, bytes.data(), bytes.size());     // Instances::transform_insert
    h->instance_count[rec->transform_key] = n;
    h->instance_list[rec->transform_key] = std::move(list);
    h->instances_dirty = true;
    return AWSM_OK;
}
// Meshes::append_mesh_instances -> Instances::transform_extend: appended in place while the block has room, else re-inserted whole
int awsm_host_mesh_append_instances(AwsmHost* h, AwsmKey mesh, const float* trs10, uint32_t n) {
    MeshRec* rec = h->meshes.get(mesh);
    if (!rec || !rec->instanced) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[mesh] not found or not instanced");
    if (n == 0) return (int)h->instance_count[rec->transform_key];
    std::vector<Transform>& list = h->instance_list[rec->transform_key];
    const size_t start = list.size();
    for (uint32_t i = 0; i < n; i++) list.push_back(trs_at(trs10, i));
    const std::vector<uint8_t> bytes = instance_bytes(list.data(), list.size());
    h->instances.update(rec->transform_key, bytes.data(), bytes.size());     // same bytes either way; update() keeps the block when it fits
    h->instance_count[rec->transform_key] = (uint32_t)list.size();
    h->instances_dirty = true;
    return (int)start;
}

// ------------------------------------------------------------------------------------------------ lights / camera / env
AwsmKey awsm_host_light_insert(AwsmHost* h, const AwsmHostLight* l) {
    if (!l || l->kind < 1 || l->kind > 3) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "light_insert: bad kind"); return 0; }
    h->punctual_dirty = h->lights_info_dirty = true;
    return h->lights.insert(*l);
}
int awsm_host_light_remove(AwsmHost* h, AwsmKey key) {
    if (!h->lights.remove(key)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[light] not found");
    h->punctual_dirty = h->lights_info_dirty = true;
    return AWSM_OK;
}
int awsm_host_light_update(AwsmHost* h, AwsmKey key, const AwsmHostLight* l) {   // lights.rs:218-224
    AwsmHostLight* cur = h->lights.get(key);
    if (!cur) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[light] not found");
    if (!l || l->kind < 1 || l->kind > 3) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "light_update: bad kind");
    *cur = *l;
    h->punctual_dirty = true;
    return AWSM_OK;
}
int awsm_host_set_ibl_mip_counts(AwsmHost* h, uint32_t prefiltered, uint32_t irradiance) {
    h->prefiltered_mips = prefiltered; h->irradiance_mips = irradiance; h->lights_info_dirty = true;
    return AWSM_OK;
}

// The 512-byte camera block (camera.rs:111-227) from an f32 view and projection: the scene camera's, and the shadow pass's camera at the light
static void pack_camera_block(const AwsmHost* h, const Mat4& v, const Mat4& p, const float pos[3], float width, float height, uint8_t* o) {
    const Mat4 inv_proj = mat4_inverse(p);
    const Mat4 view_proj = mat4_mul(p, v);
    const Mat4 inv_view_proj = mat4_inverse(view_proj);
    const Mat4 inv_view = mat4_inverse(v);
    memcpy(o, &v, 64); memcpy(o + 64, &p, 64); memcpy(o + 128, &view_proj, 64);
    memcpy(o + 192, &inv_view_proj, 64); memcpy(o + 256, &inv_proj, 64); memcpy(o + 320, &inv_view, 64);
    const float posw[4] = {pos[0], pos[1], pos[2], 0.0f};
    memcpy(o + 384, posw, 16);
    const uint32_t fc[4] = {h->frame_count, 0, 0, 0};
    memcpy(o + 400, fc, 16);
    const Vec4 corners[4] = {{-1, -1, 0, 1}, {1, -1, 0, 1}, {-1, 1, 0, 1}, {1, 1, 0, 1}};   // camera.rs:285-306
    for (int i = 0; i < 4; i++) {
        Vec4 vs = mat4_mul_vec4(inv_proj, corners[i]);
        vs = {vs.x / vs.w, vs.y / vs.w, vs.z / vs.w, vs.w / vs.w};
        const Vec3 d = v3_normalize({vs.x, vs.y, vs.z});
        const float ray[4] = {d.x, d.y, d.z, 0.0f};
        memcpy(o + 416 + i * 16, ray, 16);
    }
    const float viewport[4] = {0.0f, 0.0f, width, height};
    memcpy(o + 480, viewport, 16);
    const float dof[4] = {h->dof_params[0], h->dof_params[1], 0.0f, 0.0f};
    memcpy(o + 496, dof, 16);
}

int awsm_host_camera_update(AwsmHost* h, const float view[16], const float projection[16], const float pos[3]) {
    Mat4 v, p;
    memcpy(&v, view, 64); memcpy(&p, projection, 64);
    pack_camera_block(h, v, p, pos, (float)h->width, (float)h->height, h->camera_raw);
    h->cam_view = v; h->cam_proj = p; h->have_camera = true; h->camera_dirty = true;
    return AWSM_OK;
}

// Environment / Ibl texture swap (environment.rs, lights/ibl.rs: the cubes a caller loaded from KTX2 / EXR replace the builder's colours)
int awsm_host_env_cube(AwsmHost* h, AwsmCube which, uint32_t size, uint32_t mips, const uint16_t* texels_rgba16f) {
    int rc = h->be.env_cube_upload(h->ctx, which, size, mips, texels_rgba16f);
    return rc ? dev_fail(h, rc, "env_cube_upload") : AWSM_OK;
}
// Environment cubes at run time (environment.rs, textures.rs:118-165): the backend does the work; its symbols are optional
#define AWSM_ENV_CUBE_CALL(fn, symbol, ...)                                                                                             \
    do {                                                                                                                                \
        if (!h) return AWSM_ERR_INVALID_ARGUMENT;                                                                                       \
        if (!h->be.fn) return fail(h, AWSM_ERR_UNSUPPORTED, "the backend library has no %s", symbol);                                   \
        const int rc_ = h->be.fn(h->ctx, __VA_ARGS__);                                                                                  \
        return rc_ ? dev_fail(h, rc_, symbol + 9) : AWSM_OK;                                                                            \
    } while (0)
int awsm_host_env_cube_create(AwsmHost* h, AwsmCube which, uint32_t size, uint32_t mips) { AWSM_ENV_CUBE_CALL(env_cube_create, "awsm_hip_env_cube_create", which, size, mips); }
int awsm_host_env_cube_update_face(AwsmHost* h, AwsmCube which, uint32_t face, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                   const void* data, size_t data_len, const AwsmCubeLayout* layout) {
    AWSM_ENV_CUBE_CALL(env_cube_write_face, "awsm_hip_env_cube_write_face", which, face, mip, width, height, format, data, data_len, layout);
}
int awsm_host_env_cube_update_all_faces(AwsmHost* h, AwsmCube which, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                        const void* data, size_t data_len, const AwsmCubeLayout* layout) {
    AWSM_ENV_CUBE_CALL(env_cube_write_all_faces, "awsm_hip_env_cube_write_all_faces", which, mip, width, height, format, data, data_len, layout);
}
int awsm_host_env_cube_regenerate_mipmaps(AwsmHost* h, AwsmCube which) { AWSM_ENV_CUBE_CALL(env_cube_generate_mips, "awsm_hip_env_cube_generate_mips", which); }
int awsm_host_env_cube_colors(AwsmHost* h, AwsmCube which, uint32_t size, const float rgba[24]) { AWSM_ENV_CUBE_CALL(env_cube_fill_colors, "awsm_hip_env_cube_fill_colors", which, size, rgba); }
int awsm_host_env_cube_sky_gradient(AwsmHost* h, AwsmCube which, uint32_t size, const float zenith[4], const float nadir[4]) {
    AWSM_ENV_CUBE_CALL(env_cube_fill_sky_gradient, "awsm_hip_env_cube_fill_sky_gradient", which, size, zenith, nadir);
}
int awsm_host_env_cube_from_equirect(AwsmHost* h, AwsmCube which, const void* data, size_t len, const AwsmEquirect* pano) {
    AWSM_ENV_CUBE_CALL(env_cube_from_equirect, "awsm_hip_env_cube_from_equirect", which, data, len, pano);
}
#undef AWSM_ENV_CUBE_CALL
// The two cubes the opaque pass lights with, filtered on the device from the skybox as it is now (the reference loads them ready-made: ibl.rs:19-28)
int awsm_host_env_bake_ibl(AwsmHost* h, uint32_t prefiltered_size, uint32_t prefiltered_mips, uint32_t irradiance_size, uint32_t sample_count) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.env_cube_filter) return fail(h, AWSM_ERR_UNSUPPORTED, "the backend library has no %s", "awsm_hip_env_cube_filter");
    const AwsmEnvFilter ggx = {(uint32_t)sizeof(AwsmEnvFilter), 0u, prefiltered_size, prefiltered_mips, sample_count, 0u};
    const AwsmEnvFilter lambert = {(uint32_t)sizeof(AwsmEnvFilter), 1u, irradiance_size, 1u, sample_count, 0u};
    int rc = h->be.env_cube_filter(h->ctx, AWSM_CUBE_SKYBOX, AWSM_CUBE_PREFILTERED, &ggx);
    if (!rc) rc = h->be.env_cube_filter(h->ctx, AWSM_CUBE_SKYBOX, AWSM_CUBE_IRRADIANCE, &lambert);
    if (rc) return dev_fail(h, rc, "env_cube_filter");
    return awsm_host_set_ibl_mip_counts(h, prefiltered_mips, 1u);
}

int awsm_host_ktx2_parse(const uint8_t* data, size_t len, AwsmKtx2Info* out, char* err_out, size_t err_cap) { return ktx2::parse(data, len, out, err_out, err_cap); }

// cubemap/ktx.rs:39-191: parse, create the texture with the file's level count, one write per level
int awsm_host_env_cube_load_ktx2_memory(AwsmHost* h, AwsmCube which, const uint8_t* data, size_t len, AwsmKtx2Info* info_out, char* err_out, size_t err_cap) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmKtx2Info info{};
    info.struct_size = sizeof info;
    int rc = ktx2::parse(data, len, &info, err_out, err_cap);
    if (rc) { h->last_error = (err_out && err_cap) ? err_out : "ktx2: the file was refused"; return rc; }
    if ((rc = awsm_host_env_cube_create(h, which, info.size, info.mips)) == AWSM_OK) {
        for (uint32_t l = 0; l < info.levels && rc == AWSM_OK; l++) {
            const uint32_t n = std::max(1u, info.size >> l);
            AwsmCubeLayout layout{};
            layout.struct_size = sizeof layout; layout.bytes_per_row = (uint32_t)(info.level[l].length / (6u * n)); layout.rows_per_image = n;      // tight: the parser checked the length
            rc = awsm_host_env_cube_update_all_faces(h, which, l, n, n, (AwsmCubeFormat)info.format, data + info.level[l].offset, (size_t)info.level[l].length, &layout);
        }
        if (rc == AWSM_OK && info.mips > info.levels) rc = awsm_host_env_cube_regenerate_mipmaps(h, which);      // levelCount 0
    }
    if (rc) { if (err_out && err_cap) snprintf(err_out, err_cap, "%s", h->last_error.c_str()); return rc; }
    if (info_out) { const uint32_t theirs = info_out->struct_size; memcpy(info_out, &info, std::min<size_t>(theirs, sizeof info)); info_out->struct_size = std::min<uint32_t>(theirs, sizeof info); }
    return AWSM_OK;
}

int awsm_host_env_cube_load_ktx2(AwsmHost* h, AwsmCube which, const char* path, AwsmKtx2Info* info_out, char* err_out, size_t err_cap) {
    if (!h || !path) return AWSM_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> bytes;
    FILE* f = fopen(path, "rb");
    bool ok = f != nullptr;
    if (ok) {
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        ok = !ferror(f);
        fclose(f);
    }
    if (!ok) {
        fail(h, AWSM_ERR_INVALID_ARGUMENT, "ktx2: cannot read %s", path);
        if (err_out && err_cap) snprintf(err_out, err_cap, "%s", h->last_error.c_str());
        return AWSM_ERR_INVALID_ARGUMENT;
    }
    return awsm_host_env_cube_load_ktx2_memory(h, which, bytes.data(), bytes.size(), info_out, err_out, err_cap);
}

// Radiance pictures (host/rgbe.hpp) and the skybox from one: the reference's first offline step, `cmgen -x skybox`, on the device
int awsm_host_hdr_info(const uint8_t* data, size_t len, AwsmHdrInfo* out, char* err, size_t err_cap) { return rgbe::info(data, len, out, err, err_cap); }
int awsm_host_hdr_decode(const uint8_t* data, size_t len, uint8_t* rgbe_out, size_t out_cap, AwsmHdrInfo* out, char* err, size_t err_cap) {
    return rgbe::decode(data, len, rgbe_out, out_cap, out, err, err_cap);
}

// decode, create(size, full chain), from_equirect, generate_mips
int awsm_host_env_cube_load_hdr_memory(AwsmHost* h, AwsmCube which, const uint8_t* data, size_t len, uint32_t size, uint32_t samples, float yaw, float scale,
                                       AwsmHdrInfo* info_out, char* err_out, size_t err_cap) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmHdrInfo info{};
    info.struct_size = sizeof info;
    int rc = rgbe::info(data, len, &info, err_out, err_cap);
    std::vector<uint8_t> pixels;
    if (!rc) {
        try { pixels.resize((size_t)info.width * info.height * 4u); }      // at most 2^30 bytes: the reader checked the extent
        catch (const std::bad_alloc&) { return fail(h, AWSM_ERR_OUT_OF_MEMORY, "hdr: no memory for %u x %u pixels", info.width, info.height); }
        rc = rgbe::decode(data, len, pixels.data(), pixels.size(), &info, err_out, err_cap);
    }
    if (rc) { h->last_error = (err_out && err_cap) ? err_out : "hdr: the file was refused"; return rc; }
    uint32_t mips = 0;
    for (uint32_t s = size; s; s >>= 1) mips++;
    if (size == 0) rc = fail(h, AWSM_ERR_INVALID_ARGUMENT, "env_cube_load_hdr: size 0");
    if (!rc) rc = awsm_host_env_cube_create(h, which, size, mips);
    if (!rc) {
        AwsmEquirect pano{};
        pano.struct_size = sizeof pano; pano.width = info.width; pano.height = info.height; pano.format = AWSM_PANO_RGBE8;
        pano.samples = samples; pano.yaw = yaw; pano.scale = scale;
        rc = awsm_host_env_cube_from_equirect(h, which, pixels.data(), pixels.size(), &pano);
    }
    if (!rc && mips > 1) rc = awsm_host_env_cube_regenerate_mipmaps(h, which);
    if (rc) { if (err_out && err_cap) snprintf(err_out, err_cap, "%s", h->last_error.c_str()); return rc; }
    if (info_out) { const uint32_t theirs = info_out->struct_size; memcpy(info_out, &info, std::min<size_t>(theirs, sizeof info)); info_out->struct_size = std::min<uint32_t>(theirs, sizeof info); }
    return AWSM_OK;
}

int awsm_host_env_cube_load_hdr(AwsmHost* h, AwsmCube which, const char* path, uint32_t size, uint32_t samples, float yaw, float scale, AwsmHdrInfo* info_out,
                                char* err_out, size_t err_cap) {
    if (!h || !path) return AWSM_ERR_INVALID_ARGUMENT;
    std::vector<uint8_t> bytes;
    FILE* f = fopen(path, "rb");
    bool ok = f != nullptr;
    if (ok) {
        uint8_t chunk[65536];
        size_t got;
        while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        ok = !ferror(f);
        fclose(f);
    }
    if (!ok) {
        fail(h, AWSM_ERR_INVALID_ARGUMENT, "hdr: cannot read %s", path);
        if (err_out && err_cap) snprintf(err_out, err_cap, "%s", h->last_error.c_str());
        return AWSM_ERR_INVALID_ARGUMENT;
    }
    return awsm_host_env_cube_load_hdr_memory(h, which, bytes.data(), bytes.size(), size, samples, yaw, scale, info_out, err_out, err_cap);
}

int awsm_host_env(AwsmHost* h, const AwsmEnv* env) { int rc = h->be.env_upload(h->ctx, env); return rc ? dev_fail(h, rc, "env_upload") : AWSM_OK; }
int awsm_host_brdf_lut_generate(AwsmHost* h, uint32_t w, uint32_t ht) { int rc = h->be.brdf_lut_generate(h->ctx, w, ht); return rc ? dev_fail(h, rc, "brdf_lut_generate") : AWSM_OK; }
int awsm_host_resize(AwsmHost* h, uint32_t w, uint32_t ht) {
    int rc = h->be.resize(h->ctx, w, ht, h->msaa_sample_count);
    if (rc) return dev_fail(h, rc, "resize");
    h->width = w; h->height = ht;
    h->taa_reset = true;      // the backend dropped its history; said once more with the next record
    return AWSM_OK;
}
// AwsmRenderer::set_anti_aliasing (anti_alias.rs:42-45): {msaa_sample_count None (0) or Some(4), mipmap}; other counts are
// AwsmError::UnsupportedMsaaCount (anti_alias.rs:19-25).  The render targets are recreated (TextureViewRecreate).
int awsm_host_set_anti_aliasing(AwsmHost* h, uint32_t msaa_sample_count, uint32_t mipmap) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (msaa_sample_count != 0 && msaa_sample_count != 4) { h->last_error = "UnsupportedMsaaCount"; return AWSM_ERR_UNSUPPORTED; }
    h->mipmap = mipmap != 0;
    if (h->msaa_sample_count == msaa_sample_count) return AWSM_OK;
    h->msaa_sample_count = msaa_sample_count;
    return h->width ? awsm_host_resize(h, h->width, h->height) : AWSM_OK;
}
int awsm_host_set_shard_rows(AwsmHost* h, uint32_t y0, uint32_t y1) {
    const bool part = !(y0 == 0 && (y1 == 0 || y1 >= h->height));
    if (part && h->post_on) return fail(h, AWSM_ERR_UNSUPPORTED, "set_shard_rows: post-processing is on and needs the whole frame (awsm_host_clear_post_processing first)");
    int rc = h->be.set_shard_rows(h->ctx, y0, y1);
    if (rc) return dev_fail(h, rc, "set_shard_rows");
    h->sharded = part;
    return AWSM_OK;
}
// picker.rs:55-121: PickResult::Hit(MeshKey) / Miss for the pixel under the cursor, from the last rendered frame
int awsm_host_pick(AwsmHost* h, int32_t x, int32_t y, uint32_t* hit, uint64_t* mesh_key) {
    if (!h || !hit || !mesh_key) return AWSM_ERR_INVALID_ARGUMENT;
    AwsmPick p{};
    int rc = h->be.pick(h->ctx, x, y, &p);
    if (rc) return dev_fail(h, rc, "pick");
    *hit = p.valid;
    *mesh_key = p.valid ? (((uint64_t)p.mesh_key_high << 32) | p.mesh_key_low) : 0;   // KeyData::from_ffi
    return AWSM_OK;
}
// ... and through the transparent passes' fragment lists (include/awsm_hip.h: awsm_hip_pick_ex): the query's record from the two plain arguments
static int pick_query(AwsmHost* h, const char* entry, int transparent, float alpha_threshold, AwsmPickQuery* q) {
    if (!(alpha_threshold >= 0.0f && alpha_threshold <= 1.0f)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "%s: alpha_threshold = %g (0 .. 1)", entry, (double)alpha_threshold);
    q->struct_size = (uint32_t)sizeof(AwsmPickQuery); q->flags = transparent ? AWSM_PICK_TRANSPARENT : 0u; q->alpha_threshold = alpha_threshold;
    return AWSM_OK;
}
int awsm_host_pick_ex(AwsmHost* h, int32_t x, int32_t y, int transparent, float alpha_threshold, uint32_t* hit, uint64_t* mesh_key, uint32_t* layer) {
    if (!h || !hit || !mesh_key) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.pick_ex) return fail(h, AWSM_ERR_UNSUPPORTED, "pick_ex: the backend library has no %s", "awsm_hip_pick_ex");
    AwsmPickQuery q;
    int rc = pick_query(h, "pick_ex", transparent, alpha_threshold, &q);
    if (rc) return rc;
    AwsmPickHit p{};
    if ((rc = h->be.pick_ex(h->ctx, x, y, &q, &p))) return dev_fail(h, rc, "pick_ex");
    *hit = p.valid;
    *mesh_key = p.valid ? (((uint64_t)p.mesh_key_high << 32) | p.mesh_key_low) : 0;
    if (layer) *layer = p.valid ? p.layer : 0u;
    return AWSM_OK;
}
int awsm_host_pick_rect(AwsmHost* h, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int transparent, float alpha_threshold, uint64_t* keys, uint32_t* layers,
                        uint32_t* pixels, uint32_t cap, uint32_t* n_out) {
    if (!h || !n_out) return AWSM_ERR_INVALID_ARGUMENT;
    if (cap && !keys) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "pick_rect: keys == NULL with cap = %u", cap);
    if (!h->be.pick_rect) return fail(h, AWSM_ERR_UNSUPPORTED, "pick_rect: the backend library has no %s", "awsm_hip_pick_rect");
    AwsmPickQuery q;
    int rc = pick_query(h, "pick_rect", transparent, alpha_threshold, &q);
    if (rc) return rc;
    std::vector<AwsmPickRectEntry> entries(cap);
    uint32_t n = 0;
    if ((rc = h->be.pick_rect(h->ctx, x0, y0, x1, y1, &q, cap ? entries.data() : nullptr, cap, &n))) return dev_fail(h, rc, "pick_rect");
    for (uint32_t i = 0; i < std::min(n, cap); i++) {
        keys[i] = ((uint64_t)entries[i].mesh_key_high << 32) | entries[i].mesh_key_low;
        if (layers) layers[i] = entries[i].layer;
        if (pixels) pixels[i] = entries[i].pixels;
    }
    *n_out = n;
    return AWSM_OK;
}
int awsm_host_set_render_timings(AwsmHost* h, int enabled) { int rc = h->be.set_stage_timers(h->ctx, enabled); return rc ? dev_fail(h, rc, "set_stage_timers") : AWSM_OK; }
int awsm_host_set_shard_bands(AwsmHost* h, uint32_t n, uint32_t r, uint32_t compact) {
    if (n > 1 && h->post_on) return fail(h, AWSM_ERR_UNSUPPORTED, "set_shard_bands: post-processing is on and needs the whole frame (awsm_host_clear_post_processing first)");
    int rc = h->be.set_shard_bands(h->ctx, n, r, compact);
    if (rc) return dev_fail(h, rc, "set_shard_bands");
    h->sharded = n > 1;
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ animation (animation/animations.rs)
static bool clip_to_player(AwsmHost* h, const AwsmHostAnimationClip* c, anim::Player& p) {
    if (!c || c->struct_size < sizeof(AwsmHostAnimationClip)) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert: struct_size %u", c ? c->struct_size : 0u); return false; }
    if (c->n_keys == 0 || !c->times || !c->values) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert: a clip without keys"); return false; }   // deviation: the reference panics at the first sample
    if (c->interpolation == AWSM_ANIM_CUBICSPLINE && (!c->in_tangents || !c->out_tangents)) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert: a cubic clip without tangents"); return false; }
    anim::Sampler& s = p.sampler;
    s.path = c->path; s.interpolation = c->interpolation; s.width = c->width;
    const size_t total = (size_t)c->n_keys * c->width;
    s.times.assign(c->times, c->times + c->n_keys);
    s.values.assign(c->values, c->values + total);
    if (c->interpolation == AWSM_ANIM_CUBICSPLINE) { s.in_tangents.assign(c->in_tangents, c->in_tangents + total); s.out_tangents.assign(c->out_tangents, c->out_tangents + total); }
    if (!s.valid()) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert: path %u, interpolation %u, width %u do not fit", c->path, c->interpolation, c->width); return false; }
    p.duration = c->duration;
    return true;
}

AwsmKey awsm_host_animation_insert_transform(AwsmHost* h, const AwsmHostAnimationClip* clip, AwsmKey transform) {   // animations.rs:60-68
    anim::Player p;
    if (!clip_to_player(h, clip, p)) return 0;
    if (p.sampler.path == anim::kWeights) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert_transform: a weights clip animates a mesh"); return 0; }
    if (!h->locals.contains(transform) || transform == h->root) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] local transform does not exist"); return 0; }
    const SlotKey k = h->players.insert(std::move(p));
    h->anim_transforms[key_idx(k)] = {k, transform};
    return k;
}

AwsmKey awsm_host_animation_insert_morph(AwsmHost* h, const AwsmHostAnimationClip* clip, AwsmKey mesh) {   // animations.rs:71-79
    anim::Player p;
    if (!clip_to_player(h, clip, p)) return 0;
    if (p.sampler.path != anim::kWeights) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert_morph: only a weights clip animates a mesh"); return 0; }
    const MeshRec* rec = h->meshes.get(mesh);
    const uint32_t* targets = rec && rec->morph_key ? h->morphs.get(rec->morph_key) : nullptr;
    if (!targets) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert_morph: the mesh has no morph targets"); return 0; }
    if (p.sampler.width != *targets) { fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_insert_morph: width %u for %u targets", p.sampler.width, *targets); return 0; }
    const SlotKey k = h->players.insert(std::move(p));
    h->anim_morphs[key_idx(k)] = {k, mesh};
    return k;
}

int awsm_host_animation_remove(AwsmHost* h, AwsmKey key) {   // animations.rs:53-57
    if (!h->players.remove(key)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] not found");
    h->anim_transforms.erase(key_idx(key));
    h->anim_morphs.erase(key_idx(key));
    return AWSM_OK;
}

int awsm_host_animation_set_playback(AwsmHost* h, AwsmKey key, double speed, int loop_style, int direction, int state) {
    anim::Player* p = h->players.get(key);
    if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] not found");
    if (loop_style < -1 || loop_style > 1 || direction < 0 || direction > 1 || state < 0 || state > 2) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_set_playback: loop style %d, direction %d, state %d", loop_style, direction, state);
    p->speed = speed; p->loop_style = loop_style; p->direction = direction; p->state = state;
    return AWSM_OK;
}

int awsm_host_animation_seek(AwsmHost* h, AwsmKey key, double local_time) {
    anim::Player* p = h->players.get(key);
    if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] not found");
    if (!std::isfinite(local_time)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_seek: the time is not finite");
    p->local_time = local_time;
    return AWSM_OK;
}

int awsm_host_animation_state(AwsmHost* h, AwsmKey key, AwsmHostAnimationState* out) {
    const anim::Player* p = h->players.get(key);
    if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] not found");
    if (!out || out->struct_size < sizeof(AwsmHostAnimationState)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "animation_state: struct_size");
    out->direction = p->direction; out->state = p->state; out->loop_style = p->loop_style;
    out->local_time = p->local_time; out->duration = p->duration; out->speed = p->speed;
    return AWSM_OK;
}

int awsm_host_animation_sample(AwsmHost* h, AwsmKey key, float* out, uint32_t cap) {   // player.rs:105-107
    const anim::Player* p = h->players.get(key);
    if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] not found");
    if (!out) return (int)p->sampler.width;      // the query
    if (cap < p->sampler.width) return fail(h, AWSM_ERR_OUT_OF_RANGE, "animation_sample: room for %u of %u floats", cap, p->sampler.width);
    anim::sample(p->sampler, p->local_time, out);
    return (int)p->sampler.width;
}

int awsm_host_update_animations(AwsmHost* h, double global_time_delta) {   // animations.rs:84-141
    for (anim::Player& p : h->players.values()) p.update(global_time_delta);
    std::vector<float> v;
    for (const auto& kv : h->anim_transforms) {
        const anim::Player* p = h->players.get(kv.second.first);
        if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] missing key");
        const SlotKey tk = kv.second.second;
        const Transform* cur = h->locals.get(tk);      // get_local
        if (!cur) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[transform] local transform does not exist");
        Transform t = *cur;
        float q[4];
        anim::sample(p->sampler, p->local_time, q);
        if (p->sampler.path == anim::kTranslation) t.t = {q[0], q[1], q[2]};      // TransformAnimation::apply (data.rs:188-199)
        else if (p->sampler.path == anim::kRotation) t.r = {q[0], q[1], q[2], q[3]};
        else t.s = {q[0], q[1], q[2]};
        const float tt[3] = {t.t.x, t.t.y, t.t.z}, rr[4] = {t.r.x, t.r.y, t.r.z, t.r.w}, ss[3] = {t.s.x, t.s.y, t.s.z};
        int rc = awsm_host_transform_set_local(h, tk, tt, rr, ss);
        if (rc) return rc;
    }
    for (const auto& kv : h->anim_morphs) {
        const anim::Player* p = h->players.get(kv.second.first);
        if (!p) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "[animation] missing key");
        v.resize(p->sampler.width);
        anim::sample(p->sampler, p->local_time, v.data());
        int rc = awsm_host_mesh_update_morph_weights(h, kv.second.second, v.data(), (uint32_t)v.size());
        if (rc) return rc;
    }
    return AWSM_OK;
}

// the glTF reader (gltf.cpp) leaves the keys of the players it made here; hidden: internal to the library
__attribute__((visibility("hidden"))) void awsm_host_gltf_set_animation_keys(AwsmHost* h, const AwsmKey* keys, uint32_t n) { h->gltf_animation_keys.assign(keys, keys + n); }
int awsm_host_gltf_animation_keys(AwsmHost* h, AwsmKey* out, uint32_t cap, uint32_t* n) {
    if (!h || !n) return AWSM_ERR_INVALID_ARGUMENT;
    *n = (uint32_t)h->gltf_animation_keys.size();
    if (out) memcpy(out, h->gltf_animation_keys.data(), std::min<size_t>(cap, h->gltf_animation_keys.size()) * sizeof(AwsmKey));
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ device skin posing
int awsm_host_set_device_skin_posing(AwsmHost* h, int on) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (on && (!h->be.skin_pose_records_write || !h->be.skin_pose))
        return fail(h, AWSM_ERR_NOT_READY, "set_device_skin_posing: the backend library has no %s", !h->be.skin_pose_records_write ? "awsm_hip_skin_pose_records_write" : "awsm_hip_skin_pose");
    if (!on && h->device_posing) settle_pose_on_host(h);      // back to the host: what the device was still to compose is composed here and uploaded
    h->device_posing = on != 0;
    return AWSM_OK;
}

int awsm_host_skin_pose_ids_last_frame(AwsmHost* h, uint32_t* out, uint32_t cap, uint32_t* n) {
    if (!h || !n) return AWSM_ERR_INVALID_ARGUMENT;
    *n = (uint32_t)h->pose_ids_last.size();
    if (out) memcpy(out, h->pose_ids_last.data(), std::min<size_t>(cap, h->pose_ids_last.size()) * 4);
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ frame
int awsm_host_update_transforms(AwsmHost* h) {   // transforms.rs:29-39 + meshes.rs:872-939
    h->transforms_gpu_dirty = h->transforms_gpu_dirty || !h->dirties.empty();
    update_inner(h, h->root, false);
    h->dirties.clear();
    std::unordered_map<SlotKey, Mat4> dirty;
    for (SlotKey k : h->dirty_meshes) dirty[k] = h->world[k];
    h->dirty_meshes.clear();
    for (auto& kv : dirty) {
        auto it = h->transform_to_meshes.find(kv.first);
        if (it == h->transform_to_meshes.end()) continue;
        for (SlotKey mk : it->second) {
            MeshRec* m = h->meshes.get(mk);
            if (m) { m->world_aabb = aabb_transformed(m->local_aabb, kv.second); m->has_world_aabb = true; }
        }
    }
    // skins.rs:162-194 walks every joint of every skin and asks whether it is dirty; the index built at skin_insert finds the same (skin, joint)
    // pairs from the dirty keys, and the bytes written are the same
    for (auto& kv : dirty) {
        auto rit = h->joint_records.find(kv.first);
        if (rit == h->joint_records.end()) continue;
        for (uint32_t id : rit->second) {
            const AwsmHost::PoseRecord& r = h->pose_records[id];
            if (h->device_posing) { h->pose_ids.push_back(id); h->pose_stale.insert(id); continue; }      // composed by the device at the next render
            const Mat4 wm = skin_matrix(h, r);
            // the matrix's 64 bytes alone are marked dirty: the reference marks the skin's whole block (update_with_unchecked, skins.rs:182-188) and
            // uploads it whichever joints moved; the bytes that reach the device are the same
            h->skin_matrices.write_range(r.skin, (size_t)r.joint_index * 64, reinterpret_cast<const uint8_t*>(&wm), 64);
            h->skin_matrices_dirty = true;
        }
    }
    return AWSM_OK;
}

static int render_shadow_pass(AwsmHost* h);
static int send_selection(AwsmHost* h);

// ---- temporal anti-aliasing ----
// camera.rs:263-274, in f32 as it stands there
static float taa_halton(uint32_t index, uint32_t base) {
    float result = 0.0f, f = 1.0f;
    while (index > 0) {
        f /= (float)base;
        result += f * (float)(index % base);
        index /= base;
    }
    return result;
}
// camera.rs:137-143: Halton(2, 3) - 0.5 over the frame size, scaled by the strength
static void taa_jitter_ndc(uint32_t frame_count, float strength, float width, float height, float out[2]) {
    const float jx = taa_halton(frame_count, 2) - 0.5f, jy = taa_halton(frame_count, 3) - 0.5f;
    out[0] = (jx / width) * strength;
    out[1] = (jy / height) * strength;
}
// camera.rs:122-129
static bool taa_matrices_equal(const Mat4& a, const Mat4& b, float epsilon) {
    const float* pa = &a.c[0].x; const float* pb = &b.c[0].x;
    for (int i = 0; i < 16; i++) if (std::fabs(pa[i] - pb[i]) > epsilon) return false;
    return true;
}
// glam's mul_mat4 and inverse (glam.hpp) with every operation in f64, on column-major arrays
static void taa_mul64(const double a[16], const double b[16], double r[16]) {
    for (int c = 0; c < 4; c++)
        for (int i = 0; i < 4; i++) r[c * 4 + i] = ((a[i] * b[c * 4] + a[4 + i] * b[c * 4 + 1]) + a[8 + i] * b[c * 4 + 2]) + a[12 + i] * b[c * 4 + 3];
}
static void taa_inverse64(const double m[16], double out[16]) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3], m10 = m[4], m11 = m[5], m12 = m[6], m13 = m[7];
    const double m20 = m[8], m21 = m[9], m22 = m[10], m23 = m[11], m30 = m[12], m31 = m[13], m32 = m[14], m33 = m[15];
    const double coef00 = m22 * m33 - m32 * m23, coef02 = m12 * m33 - m32 * m13, coef03 = m12 * m23 - m22 * m13;
    const double coef04 = m21 * m33 - m31 * m23, coef06 = m11 * m33 - m31 * m13, coef07 = m11 * m23 - m21 * m13;
    const double coef08 = m21 * m32 - m31 * m22, coef10 = m11 * m32 - m31 * m12, coef11 = m11 * m22 - m21 * m12;
    const double coef12 = m20 * m33 - m30 * m23, coef14 = m10 * m33 - m30 * m13, coef15 = m10 * m23 - m20 * m13;
    const double coef16 = m20 * m32 - m30 * m22, coef18 = m10 * m32 - m30 * m12, coef19 = m10 * m22 - m20 * m12;
    const double coef20 = m20 * m31 - m30 * m21, coef22 = m10 * m31 - m30 * m11, coef23 = m10 * m21 - m20 * m11;
    const double fac[6][4] = {{coef00, coef00, coef02, coef03}, {coef04, coef04, coef06, coef07}, {coef08, coef08, coef10, coef11},
                              {coef12, coef12, coef14, coef15}, {coef16, coef16, coef18, coef19}, {coef20, coef20, coef22, coef23}};
    const double vec[4][4] = {{m10, m00, m00, m00}, {m11, m01, m01, m01}, {m12, m02, m02, m02}, {m13, m03, m03, m03}};
    static const double sign_a[4] = {1.0, -1.0, 1.0, -1.0}, sign_b[4] = {-1.0, 1.0, -1.0, 1.0};
    for (int i = 0; i < 4; i++) {
        out[i] = ((vec[1][i] * fac[0][i] - vec[2][i] * fac[1][i]) + vec[3][i] * fac[2][i]) * sign_a[i];
        out[4 + i] = ((vec[0][i] * fac[0][i] - vec[2][i] * fac[3][i]) + vec[3][i] * fac[4][i]) * sign_b[i];
        out[8 + i] = ((vec[0][i] * fac[1][i] - vec[1][i] * fac[3][i]) + vec[3][i] * fac[5][i]) * sign_a[i];
        out[12 + i] = ((vec[0][i] * fac[2][i] - vec[1][i] * fac[4][i]) + vec[2][i] * fac[5][i]) * sign_b[i];
    }
    const double dot1 = ((m[0] * out[0] + m[1] * out[4]) + m[2] * out[8]) + m[3] * out[12];
    const double rcp_det = 1.0 / dot1;
    for (int i = 0; i < 16; i++) out[i] = out[i] * rcp_det;
}
// R = view_proj_prev * inverse(view_proj_cur), both unjittered: composed in f64 from the f32 matrices, rounded once to f32
static void taa_reproject(const Mat4& view_prev, const Mat4& proj_prev, const Mat4& view, const Mat4& proj, float out[16]) {
    double vp[16], pp[16], v[16], p[16], vp_prev[16], vp_cur[16], inv_cur[16], r[16];
    for (int i = 0; i < 16; i++) { vp[i] = (&view_prev.c[0].x)[i]; pp[i] = (&proj_prev.c[0].x)[i]; v[i] = (&view.c[0].x)[i]; p[i] = (&proj.c[0].x)[i]; }
    taa_mul64(pp, vp, vp_prev);
    taa_mul64(p, v, vp_cur);
    taa_inverse64(vp_cur, inv_cur);
    taa_mul64(vp_prev, inv_cur, r);
    for (int i = 0; i < 16; i++) out[i] = (float)r[i];
}
static int taa_prepare_frame(AwsmHost* h) {
    if (!h->post_on) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "render: awsm_host_set_taa is on and resolves in the post pass; call awsm_host_set_post_processing first (or awsm_host_set_taa(NULL))");
    const Mat4& v = h->cam_view; const Mat4& p = h->cam_proj;
    const bool same_bits = h->taa_have_last && memcmp(&v, &h->taa_last_view, 64) == 0 && memcmp(&p, &h->taa_last_proj, 64) == 0;
    const bool moved = !h->taa_have_last || !taa_matrices_equal(h->taa_last_view, v, 1e-6f) || !taa_matrices_equal(h->taa_last_proj, p, 1e-6f);      // the first frame counts as moved
    AwsmTaa& t = h->taa_sent;
    t = AwsmTaa{};
    t.struct_size = (uint32_t)sizeof(AwsmTaa);
    t.feedback = h->taa.feedback;
    taa_jitter_ndc(h->frame_count, moved ? h->taa.strength_moving : h->taa.strength_still, (float)h->width, (float)h->height, t.jitter_ndc);
    const Mat4 identity = mat4_identity();
    memcpy(t.reproject, &identity, 64);
    if (h->taa_have_last && !same_bits) taa_reproject(h->taa_last_view, h->taa_last_proj, v, p, t.reproject);
    bool finite = true;
    for (float f : t.reproject) finite = finite && std::isfinite(f);
    if (!finite) { memcpy(t.reproject, &identity, 64); h->taa_reset = true; }      // a singular camera: nothing to reproject with, this frame starts over
    if (!h->taa_have_last) h->taa_reset = true;
    t.flags = h->taa_reset ? AWSM_TAA_RESET : 0u;
    h->taa_reset = false;
    // proj' = translation(jitter) * proj, glam's mul_mat4; the block from it as from any projection
    Mat4 jitter = mat4_identity();
    jitter.c[3] = {t.jitter_ndc[0], t.jitter_ndc[1], 0.0f, 1.0f};
    float pos[3];
    memcpy(pos, h->camera_raw + 384, sizeof pos);      // the position as awsm_host_camera_update was given it
    pack_camera_block(h, v, mat4_mul(jitter, p), pos, (float)h->width, (float)h->height, h->taa_block);
    h->taa_last_view = v; h->taa_last_proj = p; h->taa_have_last = true;
    return AWSM_OK;
}
int awsm_host_render(AwsmHost* h, int sync, AwsmFrameStats* stats) {   // render.rs:53-383 (hot path only)
    if (!h->width) return fail(h, AWSM_ERR_NOT_READY, "render before resize");
    h->shadow_rendered = false;
    if (h->shadow_on && !h->lights.get(h->shadow.light)) {      // the shadowed light was removed: the feature goes off, said once
        h->shadow_on = false;
        return fail(h, AWSM_ERR_INVALID_ARGUMENT, "render: the light awsm_host_set_shadow named was removed; shadows are off from here on");
    }
    h->upload_bytes = 0;
    h->frame_count += 1;   // render_textures.next_frame()
    int rc;
    if (h->taa_on && (rc = taa_prepare_frame(h))) return rc;      // the jittered camera block and the record of this frame
    // ---- write_gpu, in the reference's order (render.rs:73-97) ----
    if (h->transforms_gpu_dirty) {
        bool d1 = true, d2 = true;
        if ((rc = flush_buffer(h, h->transforms_buf, AWSM_BUF_TRANSFORMS, d1))) return rc;
        if ((rc = flush_buffer(h, h->normals_buf, AWSM_BUF_NORMAL_MATS, d2))) return rc;
        h->transforms_gpu_dirty = false;
    }
    if ((rc = flush_buffer(h, h->materials_buf, AWSM_BUF_MATERIALS, h->materials_dirty))) return rc;
    if (h->punctual_dirty) {   // lights.rs:226-291: dense rebuild
        std::vector<uint8_t> buf(h->lights.size() * 64);
        for (size_t i = 0; i < h->lights.size(); i++) light_bytes(h->lights.values()[i], buf.data() + i * 64);
        size_t target = h->punctual_gpu_size;
        if (buf.size() > h->punctual_gpu_size) target = std::max<size_t>(buf.size() * 2, 64);
        else if (buf.size() < h->punctual_gpu_size / 2) target = std::max<size_t>(buf.size(), 64);
        if (target != h->punctual_gpu_size || !h->lights_created) {
            if ((rc = h->be.buffer_create(h->ctx, AWSM_BUF_LIGHTS, target))) return dev_fail(h, rc, "buffer_create(lights)");
            h->punctual_gpu_size = target; h->lights_created = true;
        }
        if (!buf.empty()) { if ((rc = h->be.buffer_write(h->ctx, AWSM_BUF_LIGHTS, 0, buf.data(), buf.size()))) return dev_fail(h, rc, "buffer_write(lights)"); h->upload_bytes += buf.size(); }
        h->punctual_dirty = false;
    }
    if (h->lights_info_dirty) {   // lights.rs:293-305
        const uint32_t info[4] = {(uint32_t)h->lights.size(), h->prefiltered_mips, h->irradiance_mips, 0};
        if (!h->lights_info_created) { if ((rc = h->be.buffer_create(h->ctx, AWSM_BUF_LIGHTS_INFO, 16))) return dev_fail(h, rc, "buffer_create(lights info)"); h->lights_info_created = true; }
        if ((rc = h->be.buffer_write(h->ctx, AWSM_BUF_LIGHTS_INFO, 0, info, 16))) return dev_fail(h, rc, "buffer_write(lights info)");
        h->upload_bytes += 16;
        h->lights_info_dirty = false;
    }
    if ((rc = flush_buffer(h, h->instances, AWSM_BUF_INSTANCES, h->instances_dirty))) return rc;   // instances.write_gpu: after lights, before skins (render.rs:73-80)
    if (h->device_posing && h->skin_matrices_dirty) sync_skin_mirror(h);      // a skin came or went: the flush may write the whole mirror, so it has to be the device's bytes
    if ((rc = flush_buffer(h, h->skin_matrices, AWSM_BUF_SKIN_MATRICES, h->skin_matrices_dirty))) return rc;
    h->pose_ids_last.clear();
    if (h->device_posing) {      // AWSM_BUF_TRANSFORMS went up above: the device composes the joints that moved from the world matrices it has
        if ((rc = send_pose_records(h))) return rc;
        std::sort(h->pose_ids.begin(), h->pose_ids.end());
        h->pose_ids.erase(std::unique(h->pose_ids.begin(), h->pose_ids.end()), h->pose_ids.end());
        if (!h->pose_ids.empty()) {
            if ((rc = h->be.skin_pose(h->ctx, h->pose_ids.data(), (uint32_t)h->pose_ids.size()))) return dev_fail(h, rc, "skin_pose");
            h->upload_bytes += (uint64_t)h->pose_ids.size() * 4;
        }
        h->pose_ids_last.swap(h->pose_ids);
        h->pose_ids.clear();
    }
    if ((rc = flush_buffer(h, h->skin_index_weights, AWSM_BUF_SKIN_INDEX_WEIGHTS, h->skin_iw_dirty))) return rc;
    if ((rc = flush_buffer(h, h->morph_weights, AWSM_BUF_MORPH_WEIGHTS, h->morph_weights_dirty))) return rc;
    if ((rc = flush_buffer(h, h->morph_values, AWSM_BUF_MORPH_VALUES, h->morph_values_dirty))) return rc;
    if ((rc = flush_buffer(h, h->geom_meta, AWSM_BUF_GEOM_META, h->geom_meta_dirty))) return rc;
    if ((rc = flush_buffer(h, h->material_meta, AWSM_BUF_MATERIAL_META, h->material_meta_dirty))) return rc;
    if ((rc = flush_buffer(h, h->tex_transforms_buf, AWSM_BUF_TEXTURE_TRANSFORMS, h->tex_transforms_dirty))) return rc;
    if ((rc = flush_buffer(h, h->vis_data, AWSM_BUF_VIS_GEOM_DATA, h->vis_data_dirty))) return rc;
    // VisGeomIndex (identity indices) stays a host mirror only: a software rasteriser has no index fetch.  The
    // mirror still tracks the reference's allocation; nothing is uploaded (SURVEY Appendix A "redundant").
    h->vis_index.take_dirty_ranges(); h->vis_index.take_gpu_needs_resize(); h->vis_index_dirty = false;
    if ((rc = flush_buffer(h, h->tr_data, AWSM_BUF_TRANSPARENCY_GEOM_DATA, h->tr_data_dirty))) return rc;   // meshes.rs:1268: between the visibility and the attribute buffers
    if ((rc = flush_buffer(h, h->attr_data, AWSM_BUF_ATTR_DATA, h->attr_data_dirty))) return rc;
    if ((rc = flush_buffer(h, h->attr_index, AWSM_BUF_ATTR_INDEX, h->attr_index_dirty))) return rc;
    if (h->camera_dirty || h->taa_on) {   // camera.rs:232-251; with TAA on the block is another one every frame
        if (!h->camera_created) { if ((rc = h->be.buffer_create(h->ctx, AWSM_BUF_CAMERA, 512))) return dev_fail(h, rc, "buffer_create(camera)"); h->camera_created = true; }
        if ((rc = h->be.buffer_write(h->ctx, AWSM_BUF_CAMERA, 0, h->taa_on ? h->taa_block : h->camera_raw, 512))) return dev_fail(h, rc, "buffer_write(camera)");
        h->upload_bytes += 512;
        h->camera_dirty = false;
    }
    for (uint32_t i = 0; i < h->pool.size(); i++) {   // finalize_gpu_textures: (re)upload arrays that gained layers
        AwsmHost::PoolArray& a = h->pool[i];
        if (!a.dirty) continue;
        // TexturePoolArray::new: mipmap = true for every array -> full chain (texture_pool.rs:166-176,187-192,317-319)
        uint32_t levels = 1;
        for (uint32_t m = std::max(a.w, a.h); m > 1u; m >>= 1) levels++;
        if ((rc = finalize_pool_array(h, i, levels))) return rc;
        a.dirty = false;
    }
    // ---- collect_renderables -> geometry pass -> opaque pass (render.rs:144-221) ----
    collect_draws(h, h->last_draws, &h->last_transparent_draws, &h->last_hud_geometry_draws, &h->last_hud_transparent_draws);
    if ((rc = h->be.geometry_pass(h->ctx, h->last_draws.data(), (uint32_t)h->last_draws.size()))) return dev_fail(h, rc, "geometry_pass");
    if (h->has_hud_meshes && (rc = h->be.hud_geometry_pass(h->ctx, h->last_hud_geometry_draws.data(), (uint32_t)h->last_hud_geometry_draws.size()))) return dev_fail(h, rc, "hud_geometry_pass");   // render.rs:169-178
    if (h->shadow_on && (rc = render_shadow_pass(h))) return rc;      // the shadow map of this frame, from the light
    if (h->after_geometry && (rc = h->after_geometry(h->after_geometry_user))) { h->last_error = "after_geometry_pass hook failed"; return rc; }   // hooks.after_geometry_pass (render.rs:181-190)
    AwsmOpaqueParams op{};
    op.mipmap = h->mipmap ? 1u : 0u; op.has_opaque = h->last_draws.empty() ? 0u : 1u;   // material_opaque/render_pass.rs:64-71
    if ((rc = h->be.opaque_pass(h->ctx, &op))) return dev_fail(h, rc, "opaque_pass");
    if (h->after_opaque && (rc = h->after_opaque(h->after_opaque_user))) { h->last_error = "after_opaque_pass hook failed"; return rc; }
    // ---- opaque -> transparent blit + world transparent pass (render.rs:224-297).  A scene without transparent meshes skips it:
    // the composite image then IS the opaque image (the reference would copy it) — unless the editor's grid is on, which that pass draws. ----
    if (h->selection_on && (rc = send_selection(h))) return rc;      // the selected meshes' boxes as update_world left them
    if (h->has_transparent_meshes || h->has_hud_meshes || h->grid_on || h->selection_on) { if ((rc = h->be.transparent_pass(h->ctx, h->last_transparent_draws.data(), (uint32_t)h->last_transparent_draws.size()))) return dev_fail(h, rc, "transparent_pass"); }
    // ---- the HUD transparent pass over the composite (render.rs:301-312) ----
    if (h->has_hud_meshes && (rc = h->be.hud_transparent_pass(h->ctx, h->last_hud_transparent_draws.data(), (uint32_t)h->last_hud_transparent_draws.size()))) return dev_fail(h, rc, "hud_transparent_pass");
    // ---- the effects + display passes (render.rs:339-356), when post-processing was turned on ----
    if (h->taa_on && (rc = h->be.set_taa(h->ctx, &h->taa_sent))) return dev_fail(h, rc, "set_taa");
    if (h->post_on && (rc = h->be.post_pass(h->ctx, &h->post))) return dev_fail(h, rc, "post_pass");
    if (sync) { if ((rc = h->be.frame_end(h->ctx, stats))) return dev_fail(h, rc, "frame_end"); }   // gpu.submit_commands (render.rs:370)
    return AWSM_OK;
}

// AwsmRenderer::set_post_processing (post_process.rs) + AntiAliasing.smaa (anti_alias.rs): from now on awsm_host_render ends with the post pass
int awsm_host_set_post_processing(AwsmHost* h, uint32_t tonemapping, int bloom, int dof, int smaa) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.post_pass) return fail(h, AWSM_ERR_UNSUPPORTED, "set_post_processing: the backend library has no awsm_hip_post_pass");
    if (tonemapping > 2u) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_post_processing: tonemapping %u (0 None, 1 KhronosNeutralPbr, 2 Aces)", tonemapping);
    if (h->sharded) return fail(h, AWSM_ERR_UNSUPPORTED, "set_post_processing: this host renders a shard of the frame; the post pass needs all of it");
    h->post.struct_size = sizeof(AwsmPostParams); h->post.tonemapping = tonemapping; h->post.reserved = 0;
    h->post.flags = (smaa ? AWSM_POST_SMAA : 0u) | (bloom ? AWSM_POST_BLOOM : 0u) | (dof ? AWSM_POST_DOF : 0u);
    h->post_on = true;
    return AWSM_OK;
}

// The editor's ground grid (crates/editor/src/grid, drawn by the reference's editor in its before_transparent_pass hook): a built-in of the
// backend's transparent pass.
int awsm_host_editor_grid_defaults(AwsmHost* h, AwsmEditorGrid* out) {
    if (!h || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.editor_grid_defaults) return fail(h, AWSM_ERR_UNSUPPORTED, "editor_grid_defaults: the backend library has no %s", "awsm_hip_editor_grid_defaults");
    const int rc = h->be.editor_grid_defaults(out);
    return rc ? dev_fail(h, rc, "editor_grid_defaults") : AWSM_OK;
}
int awsm_host_set_editor_grid(AwsmHost* h, const AwsmEditorGrid* grid) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.set_editor_grid) return fail(h, AWSM_ERR_UNSUPPORTED, "set_editor_grid: the backend library has no %s", "awsm_hip_set_editor_grid");
    const int rc = h->be.set_editor_grid(h->ctx, grid);
    if (rc) return dev_fail(h, rc, "set_editor_grid");
    h->grid_on = grid != nullptr;
    return AWSM_OK;
}

// The editor's selection overlay: a built-in of the backend's world transparent pass.  The host remembers the mesh keys; what the
// backend gets is the key words of the selected meshes that are there, shown and not HUD, and one box per such mesh that has a world AABB — the
// cull step's, as update_world left it — so a box follows its mesh's transform with nothing more to call.
static int send_selection(AwsmHost* h) {
    std::vector<uint32_t> words;
    std::vector<AwsmSelectionBox> boxes;
    for (AwsmKey k : h->selection_keys) {
        const MeshRec* m = h->meshes.get(k);
        if (!m || m->hidden || m->hud) continue;      // a removed mesh drops out silently
        words.push_back((uint32_t)(k >> 32)); words.push_back((uint32_t)(k & 0xFFFFFFFFull));
        if (m->has_world_aabb) boxes.push_back(AwsmSelectionBox{{m->world_aabb.min.x, m->world_aabb.min.y, m->world_aabb.min.z}, {m->world_aabb.max.x, m->world_aabb.max.y, m->world_aabb.max.z}});
    }
    const int rc = h->be.set_selection(h->ctx, &h->selection, words.data(), (uint32_t)(words.size() / 2), boxes.data(), (uint32_t)boxes.size());
    return rc ? dev_fail(h, rc, "set_selection") : AWSM_OK;
}
int awsm_host_selection_defaults(AwsmHost* h, AwsmSelection* out) {
    if (!h || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.selection_defaults) return fail(h, AWSM_ERR_UNSUPPORTED, "selection_defaults: the backend library has no %s", "awsm_hip_selection_defaults");
    const int rc = h->be.selection_defaults(out);
    return rc ? dev_fail(h, rc, "selection_defaults") : AWSM_OK;
}
int awsm_host_set_selection(AwsmHost* h, const AwsmSelection* selection, const uint64_t* mesh_keys, uint32_t n) {
    if (!h || (n && !mesh_keys)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.set_selection) return fail(h, AWSM_ERR_UNSUPPORTED, "set_selection: the backend library has no %s", "awsm_hip_set_selection");
    if (!selection) {
        const int rc = h->be.set_selection(h->ctx, nullptr, nullptr, 0, nullptr, 0);
        if (rc) return dev_fail(h, rc, "set_selection");
        h->selection_on = false; h->selection_keys.clear();
        return AWSM_OK;
    }
    if (selection->struct_size < 4u || selection->struct_size > 4096u) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_selection: AwsmSelection.struct_size = %u (set it to sizeof(AwsmSelection))", selection->struct_size);
    // the backend judges the record, now, with the meshes as they stand; its refusal leaves the selection as it was
    const AwsmSelection was = h->selection;
    std::vector<AwsmKey> keys_were(mesh_keys, mesh_keys + n);
    keys_were.swap(h->selection_keys);
    memset(&h->selection, 0, sizeof h->selection);
    memcpy(&h->selection, selection, std::min<size_t>(selection->struct_size, sizeof h->selection));
    h->selection.struct_size = (uint32_t)std::min<size_t>(selection->struct_size, sizeof h->selection);      // nothing beyond the caller's size is read, here or there
    const int rc = send_selection(h);
    if (rc) {
        h->selection = was; h->selection_keys.swap(keys_were);      // (a refusing backend keeps its own state unchanged)
        return rc;
    }
    h->selection_on = true;
    return AWSM_OK;
}

// Screen-space ambient occlusion: a built-in of the backend's opaque pass; the record goes through as it is.
int awsm_host_ssao_defaults(AwsmHost* h, AwsmSsao* out) {
    if (!h || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.ssao_defaults) return fail(h, AWSM_ERR_UNSUPPORTED, "ssao_defaults: the backend library has no %s", "awsm_hip_ssao_defaults");
    const int rc = h->be.ssao_defaults(out);
    return rc ? dev_fail(h, rc, "ssao_defaults") : AWSM_OK;
}
int awsm_host_set_ssao(AwsmHost* h, const AwsmSsao* ssao) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.set_ssao) return fail(h, AWSM_ERR_UNSUPPORTED, "set_ssao: the backend library has no %s", "awsm_hip_set_ssao");
    const int rc = h->be.set_ssao(h->ctx, ssao);
    return rc ? dev_fail(h, rc, "set_ssao") : AWSM_OK;
}

// Shadows: the host fits a camera to the light and chooses the casters; the backend rasterises them and resolves.
int awsm_host_shadow_defaults(AwsmHost* h, AwsmHostShadow* out) {
    if (!h || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.shadow_defaults) return fail(h, AWSM_ERR_UNSUPPORTED, "shadow_defaults: the backend library has no %s", "awsm_hip_shadow_defaults");
    AwsmShadow d{};
    const int rc = h->be.shadow_defaults(&d);
    if (rc) return dev_fail(h, rc, "shadow_defaults");
    *out = AwsmHostShadow{(uint32_t)sizeof(AwsmHostShadow), 0, d.map_size, d.pcf_radius, d.bias, d.slope_bias, d.max_slope, d.strength, d.facing_fade};
    return AWSM_OK;
}
int awsm_host_set_shadow(AwsmHost* h, const AwsmHostShadow* s) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.shadow_pass) return fail(h, AWSM_ERR_UNSUPPORTED, "set_shadow: the backend library has no %s", "awsm_hip_shadow_pass");
    if (!h->be.shadow_defaults) return fail(h, AWSM_ERR_UNSUPPORTED, "set_shadow: the backend library has no %s", "awsm_hip_shadow_defaults");
    if (!s) { h->shadow_on = false; return AWSM_OK; }
    if (s->struct_size != sizeof(AwsmHostShadow)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow: AwsmHostShadow.struct_size = %u (set it to sizeof(AwsmHostShadow))", s->struct_size);
    const AwsmHostLight* l = h->lights.get(s->light);
    if (!l) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow: [light] not found");
    if (l->kind == 2u && !h->be.shadow_pass_views)
        return fail(h, AWSM_ERR_UNSUPPORTED, "set_shadow: a point light needs a cube map of depths, and the backend library has no %s; directional and spot lights only", "awsm_hip_shadow_pass_views");
    h->shadow = *s;
    h->shadow_on = true;
    return AWSM_OK;
}
int awsm_host_shadow_camera(AwsmHost* h, void* block512, AwsmDraw* casters_out, uint32_t cap, uint32_t* n_out) {
    if (!h || (!casters_out && cap)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->shadow_rendered) return fail(h, AWSM_ERR_NOT_READY, "shadow_camera: the last render had no shadow pass");
    if (block512) memcpy(block512, h->shadow_block, 512);
    const uint32_t n = (uint32_t)h->shadow_casters.size();
    if (n_out) *n_out = n;
    if (casters_out) memcpy(casters_out, h->shadow_casters.data(), (size_t)std::min(n, cap) * sizeof(AwsmDraw));
    return AWSM_OK;
}

int awsm_host_shadow_cascades_defaults(AwsmHostShadowCascades* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    *out = AwsmHostShadowCascades{(uint32_t)sizeof(AwsmHostShadowCascades), 1u, 0.5f, 0.0f};
    return AWSM_OK;
}
int awsm_host_set_shadow_cascades(AwsmHost* h, const AwsmHostShadowCascades* c) {
    if (!h || !c) return AWSM_ERR_INVALID_ARGUMENT;
    if (c->struct_size != sizeof(AwsmHostShadowCascades))
        return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow_cascades: AwsmHostShadowCascades.struct_size = %u (set it to sizeof(AwsmHostShadowCascades))", c->struct_size);
    if (c->count < 1u || c->count > 4u) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow_cascades: count = %u (1 .. 4)", c->count);
    if (!(c->lambda >= 0.0f && c->lambda <= 1.0f)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow_cascades: lambda = %g (0 .. 1)", (double)c->lambda);
    if (!(c->max_distance >= 0.0f) || !std::isfinite(c->max_distance)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_shadow_cascades: max_distance = %g (>= 0; 0: the camera's far)", (double)c->max_distance);
    if (c->count > 1u && !h->be.shadow_pass_views) return fail(h, AWSM_ERR_UNSUPPORTED, "set_shadow_cascades: the backend library has no %s", "awsm_hip_shadow_pass_views");
    h->shadow_cascades = *c;
    return AWSM_OK;
}
int awsm_host_shadow_view_count(AwsmHost* h, uint32_t* n_out) {
    if (!h || !n_out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->shadow_rendered) return fail(h, AWSM_ERR_NOT_READY, "shadow_view_count: the last render had no shadow pass");
    *n_out = (uint32_t)h->shadow_views.size();
    return AWSM_OK;
}
int awsm_host_shadow_view(AwsmHost* h, uint32_t view, void* block512, AwsmDraw* casters_out, uint32_t cap, uint32_t* n_out) {
    if (!h || (!casters_out && cap)) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->shadow_rendered) return fail(h, AWSM_ERR_NOT_READY, "shadow_view: the last render had no shadow pass");
    if (view >= h->shadow_views.size()) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "shadow_view: view %u of %zu", view, h->shadow_views.size());
    const AwsmHost::ShadowViewRec& rec = h->shadow_views[view];
    if (block512) memcpy(block512, rec.block, 512);
    const uint32_t n = (uint32_t)rec.casters.size();
    if (n_out) *n_out = n;
    if (casters_out) memcpy(casters_out, rec.casters.data(), (size_t)std::min(n, cap) * sizeof(AwsmDraw));
    return AWSM_OK;
}

// The camera at the light (include/awsm_host.h has the rules), composed in f64 and rounded once to the f32 view and projection the packer takes.
static void shadow_light_camera(AwsmHost* h, const AwsmHostLight& l, uint32_t S, uint8_t block[512], float light_out[4]) {
    double f[3] = {l.direction[0], l.direction[1], l.direction[2]};
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (fl > 0.0) { f[0] /= fl; f[1] /= fl; f[2] /= fl; } else { f[0] = 0.0; f[1] = -1.0; f[2] = 0.0; }
    // the union of the candidates' world boxes
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    for (const MeshRec& m : h->meshes.values()) {
        if (m.hidden || m.hud || m.transparent || !m.has_world_aabb) continue;
        const double a[3] = {m.world_aabb.min.x, m.world_aabb.min.y, m.world_aabb.min.z}, b[3] = {m.world_aabb.max.x, m.world_aabb.max.y, m.world_aabb.max.z};
        for (int i = 0; i < 3; i++) { lo[i] = any ? std::min(lo[i], a[i]) : a[i]; hi[i] = any ? std::max(hi[i], b[i]) : b[i]; }
        any = true;
    }
    double eye[3], proj[16] = {};
    if (l.kind == 1u) {
        double c[3] = {0, 0, 0}, r = 1.0;
        if (any) {
            double dd = 0.0;
            for (int i = 0; i < 3; i++) { c[i] = 0.5 * (lo[i] + hi[i]); dd += (hi[i] - lo[i]) * (hi[i] - lo[i]); }
            r = 0.5 * std::sqrt(dd);
            if (!(r > 0.0)) r = 1.0;
        }
        for (int i = 0; i < 3; i++) eye[i] = c[i] - 2.0 * r * f[i];
        const double n = r, fa = 3.0 * r;      // Mat4::orthographic_rh(-r, r, -r, r, near, far), depth 0 .. 1
        proj[0] = 1.0 / r; proj[5] = 1.0 / r; proj[10] = 1.0 / (n - fa); proj[14] = n / (n - fa); proj[15] = 1.0;
        for (int i = 0; i < 3; i++) light_out[i] = (float)-f[i];
        light_out[3] = 0.0f;
    } else {
        for (int i = 0; i < 3; i++) eye[i] = l.position[i];
        double fa = l.range;
        if (!(fa > 0.0)) {
            fa = 0.0;
            if (any) for (int k = 0; k < 8; k++) {
                double dd = 0.0;
                for (int i = 0; i < 3; i++) { const double p = ((k >> i) & 1) ? hi[i] : lo[i]; dd += (p - eye[i]) * (p - eye[i]); }
                fa = std::max(fa, std::sqrt(dd));
            }
            fa = std::max(fa, 1.0);
        }
        const double n = std::max(0.05, fa * 1e-3), kPi = 3.14159265358979323846;
        // AwsmHostLight.outer_angle holds the COSINE of the outer cone's half angle (the glTF reader stores cos(outerConeAngle); the spot falloff compares it with cos)
        const double cone = std::acos(std::min(std::max((double)l.outer_angle, -1.0), 1.0));
        const double fovy = std::min(std::max(2.0 * cone, kPi / 180.0), 170.0 * kPi / 180.0);
        const double t = 1.0 / std::tan(0.5 * fovy);      // Mat4::perspective_rh(fovy, 1, near, far), depth 0 .. 1
        proj[0] = t; proj[5] = t; proj[10] = fa / (n - fa); proj[11] = -1.0; proj[14] = n * fa / (n - fa);
        for (int i = 0; i < 3; i++) light_out[i] = l.position[i];
        light_out[3] = 1.0f;
    }
    // Mat4::look_to_rh(eye, f, up)
    const double up[3] = {0.0, std::fabs(f[1]) > 0.999 ? 0.0 : 1.0, std::fabs(f[1]) > 0.999 ? 1.0 : 0.0};
    double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int i = 0; i < 3; i++) s[i] /= sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    const double view[16] = {s[0], u[0], -f[0], 0.0,   s[1], u[1], -f[1], 0.0,   s[2], u[2], -f[2], 0.0,
                             -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]), -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]), f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2], 1.0};
    float vf[16], pf[16];
    for (int i = 0; i < 16; i++) { vf[i] = (float)view[i]; pf[i] = (float)proj[i]; }
    Mat4 v, p;
    memcpy(&v, vf, 64); memcpy(&p, pf, 64);
    const float pos[3] = {(float)eye[0], (float)eye[1], (float)eye[2]};
    pack_camera_block(h, v, p, pos, (float)S, (float)S, block);
}

// ---- several views of the shadowed light (include/awsm_host.h has the rules) ----
// The union of the shadow candidates' world boxes -> whether there is any.
static bool shadow_scene_union(const AwsmHost* h, double lo[3], double hi[3]) {
    bool any = false;
    for (int i = 0; i < 3; i++) lo[i] = hi[i] = 0.0;
    for (const MeshRec& m : h->meshes.values()) {
        if (m.hidden || m.hud || m.transparent || !m.has_world_aabb) continue;
        const double a[3] = {m.world_aabb.min.x, m.world_aabb.min.y, m.world_aabb.min.z}, b[3] = {m.world_aabb.max.x, m.world_aabb.max.y, m.world_aabb.max.z};
        for (int i = 0; i < 3; i++) { lo[i] = any ? std::min(lo[i], a[i]) : a[i]; hi[i] = any ? std::max(hi[i], b[i]) : b[i]; }
        any = true;
    }
    return any;
}
// Mat4::look_to_rh(eye, f, up) in f64, up by §19's rule: +Y, or +Z when |f.y| > 0.999
static void shadow_look_to(const double eye[3], const double f[3], double view[16]) {
    const double up[3] = {0.0, std::fabs(f[1]) > 0.999 ? 0.0 : 1.0, std::fabs(f[1]) > 0.999 ? 1.0 : 0.0};
    double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int i = 0; i < 3; i++) s[i] /= sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    const double v[16] = {s[0], u[0], -f[0], 0.0,   s[1], u[1], -f[1], 0.0,   s[2], u[2], -f[2], 0.0,
                          -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]), -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]), f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2], 1.0};
    memcpy(view, v, sizeof v);
}
// an f64 view and projection, rounded once to f32, into a block for an S x S map
static void shadow_pack(AwsmHost* h, const double view[16], const double proj[16], const double eye[3], uint32_t S, uint8_t block[512]) {
    float vf[16], pf[16];
    for (int i = 0; i < 16; i++) { vf[i] = (float)view[i]; pf[i] = (float)proj[i]; }
    Mat4 v, p;
    memcpy(&v, vf, 64); memcpy(&p, pf, 64);
    const float pos[3] = {(float)eye[0], (float)eye[1], (float)eye[2]};
    pack_camera_block(h, v, p, pos, (float)S, (float)S, block);
}

// A point light's six faces -> the blocks, in the order +X, -X, +Y, -Y, +Z, -Z
static void shadow_cube_faces(AwsmHost* h, const AwsmHostLight& l, uint32_t S, uint32_t R, uint8_t blocks[6][512]) {
    double lo[3], hi[3];
    const bool any = shadow_scene_union(h, lo, hi);
    const double eye[3] = {l.position[0], l.position[1], l.position[2]};
    double fa = l.range;      // near and far by the spot's rule
    if (!(fa > 0.0)) {
        fa = 0.0;
        if (any) for (int k = 0; k < 8; k++) {
            double dd = 0.0;
            for (int i = 0; i < 3; i++) { const double p = ((k >> i) & 1) ? hi[i] : lo[i]; dd += (p - eye[i]) * (p - eye[i]); }
            fa = std::max(fa, std::sqrt(dd));
        }
        fa = std::max(fa, 1.0);
    }
    const double n = std::max(0.05, fa * 1e-3);
    const double t = ((double)S - 2.0 * ((double)R + 1.0)) / (double)S;      // 1 / tan(fovy / 2): the 90-degree face lands on [M, S - M)^2, M = R + 1
    double proj[16] = {};
    proj[0] = t; proj[5] = t; proj[10] = fa / (n - fa); proj[11] = -1.0; proj[14] = n * fa / (n - fa);
    for (int face = 0; face < 6; face++) {
        double f[3] = {0.0, 0.0, 0.0}, view[16];
        f[face >> 1] = (face & 1) ? -1.0 : 1.0;
        shadow_look_to(eye, f, view);
        shadow_pack(h, view, proj, eye, S, blocks[face]);
    }
}

// A directional light's N cascades, tightest first -> the blocks and AwsmShadow.light
static void shadow_cascades(AwsmHost* h, const AwsmHostLight& l, uint32_t S, uint32_t N, uint8_t blocks[4][512], float light_out[4]) {
    double f[3] = {l.direction[0], l.direction[1], l.direction[2]};
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (fl > 0.0) { f[0] /= fl; f[1] /= fl; f[2] /= fl; } else { f[0] = 0.0; f[1] = -1.0; f[2] = 0.0; }
    for (int i = 0; i < 3; i++) light_out[i] = (float)-f[i];
    light_out[3] = 0.0f;
    // §19's directional view matrix and depth range, of the scene's union
    double lo[3], hi[3], c[3] = {0, 0, 0}, r = 1.0;
    if (shadow_scene_union(h, lo, hi)) {
        double dd = 0.0;
        for (int i = 0; i < 3; i++) { c[i] = 0.5 * (lo[i] + hi[i]); dd += (hi[i] - lo[i]) * (hi[i] - lo[i]); }
        r = 0.5 * std::sqrt(dd);
        if (!(r > 0.0)) r = 1.0;
    }
    double eye[3], view[16];
    for (int i = 0; i < 3; i++) eye[i] = c[i] - 2.0 * r * f[i];
    shadow_look_to(eye, f, view);
    const double ln = r, lf = 3.0 * r;
    // the camera: its near and far, and its corner rays in world space (the view matrix is rigid: world = R^T (p - t))
    const float* cp = (const float*)&h->cam_proj;
    const float* cv = (const float*)&h->cam_view;
    const bool ortho = cp[15] != 0.0f;
    const double p0 = cp[0], p5 = cp[5], p10 = cp[10], p14 = cp[14];
    const double cn = p14 / p10, cf = ortho ? (p14 - 1.0) / p10 : p14 / (p10 + 1.0);
    const double far_used = h->shadow_cascades.max_distance > 0.0f ? std::min(cf, (double)h->shadow_cascades.max_distance) : cf;
    const double lambda = h->shadow_cascades.lambda;
    auto split = [&](uint32_t j) {
        const double uni = cn + (far_used - cn) * (double)j / (double)N;
        const double lg = cn > 0.0 ? cn * std::pow(far_used / cn, (double)j / (double)N) : uni;      // (no logarithmic split from a near plane at or behind the eye)
        return lambda * lg + (1.0 - lambda) * uni;
    };
    auto corner = [&](int k, double d, double out[3]) {      // corner ray k (NDC x, y = -1 or +1) at view depth d
        const double nx = (k & 1) ? 1.0 : -1.0, ny = (k & 2) ? 1.0 : -1.0;
        double pv[3];
        if (ortho) { pv[0] = (nx - cp[12]) / p0; pv[1] = (ny - cp[13]) / p5; }
        else { pv[0] = (nx + cp[8]) * d / p0; pv[1] = (ny + cp[9]) * d / p5; }
        pv[2] = -d;
        for (int i = 0; i < 3; i++) pv[i] -= cv[12 + i];
        for (int i = 0; i < 3; i++) out[i] = (double)cv[4 * i + 0] * pv[0] + (double)cv[4 * i + 1] * pv[1] + (double)cv[4 * i + 2] * pv[2];
    };
    for (uint32_t j = 0; j < N; j++) {
        double pts[8][3], cj[3] = {0, 0, 0};
        for (int k = 0; k < 8; k++) {
            corner(k & 3, split(j + (uint32_t)(k >> 2)), pts[k]);
            for (int i = 0; i < 3; i++) cj[i] += pts[k][i] / 8.0;
        }
        double rj = 0.0;
        for (int k = 0; k < 8; k++) {
            double dd = 0.0;
            for (int i = 0; i < 3; i++) dd += (pts[k][i] - cj[i]) * (pts[k][i] - cj[i]);
            rj = std::max(rj, std::sqrt(dd));
        }
        // the window is wider than the slice's sphere by what keeps every corner in the layer's inner region at pcf_radius <= 2: three texels on
        // each side and one for the snap below, r + 2 w / S <= w (1 - 6 / S)
        rj *= S > 16u ? (double)S / ((double)S - 8.0) : 2.0;
        rj = std::ceil(rj * 16.0) / 16.0;
        if (!(rj > 0.0)) rj = 1.0 / 16.0;
        const double texel = 2.0 * rj / (double)S;
        double xy[2];
        for (int a = 0; a < 2; a++) {
            const double v = view[a] * cj[0] + view[4 + a] * cj[1] + view[8 + a] * cj[2] + view[12 + a];
            xy[a] = std::floor(v / texel) * texel;
        }
        double proj[16] = {};
        proj[0] = 1.0 / rj; proj[5] = 1.0 / rj; proj[12] = -xy[0] / rj; proj[13] = -xy[1] / rj;
        proj[10] = 1.0 / (ln - lf); proj[14] = ln / (ln - lf); proj[15] = 1.0;
        shadow_pack(h, view, proj, eye, S, blocks[j]);
    }
}

// called by awsm_host_render between the geometry passes and the opaque pass: the light's views into h->shadow_views (one for a spot light or an
// uncascaded sun, the cube's faces with casters for a point light, the cascades otherwise), then through awsm_hip_shadow_pass or ..._views
static int render_shadow_pass(AwsmHost* h) {
    const AwsmHostLight* l = h->lights.get(h->shadow.light);
    if (!l) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "render: the shadowed light is gone");      // (checked at the top of the render too)
    AwsmShadow s{};
    s.struct_size = (uint32_t)sizeof s;
    s.map_size = h->shadow.map_size; s.pcf_radius = h->shadow.pcf_radius;
    s.bias = h->shadow.bias; s.slope_bias = h->shadow.slope_bias; s.max_slope = h->shadow.max_slope; s.strength = h->shadow.strength; s.facing_fade = h->shadow.facing_fade;
    h->shadow_views.clear();
    const bool cube = l->kind == 2u, several = cube || (l->kind == 1u && h->shadow_cascades.count > 1u);
    uint8_t blocks[6][512];
    uint32_t n_blocks = 1;
    if (several && !h->be.shadow_pass_views) return fail(h, AWSM_ERR_UNSUPPORTED, "render: the backend library has no %s", "awsm_hip_shadow_pass_views");
    if (cube) {
        if (s.map_size < 16u) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "render: a point light's shadow map_size = %u (16 at the least: a face keeps an apron of pcf_radius + 1 texels)", s.map_size);
        shadow_cube_faces(h, *l, s.map_size, s.pcf_radius, blocks);
        for (int i = 0; i < 3; i++) s.light[i] = l->position[i];
        s.light[3] = 1.0f;
        n_blocks = 6;
    } else if (several) {
        n_blocks = h->shadow_cascades.count;
        shadow_cascades(h, *l, std::max(1u, s.map_size), n_blocks, blocks, s.light);
    } else shadow_light_camera(h, *l, std::max(1u, s.map_size), blocks[0], s.light);
    for (uint32_t i = 0; i < n_blocks; i++) {
        AwsmHost::ShadowViewRec rec;
        memcpy(rec.block, blocks[i], 512);
        Mat4 lvp;
        memcpy(&lvp, blocks[i] + 128, 64);
        collect_draws(h, rec.casters, nullptr, nullptr, nullptr, &lvp);
        if (cube && rec.casters.empty()) continue;      // a face whose frustum meets no candidate is not sent
        h->shadow_views.push_back(std::move(rec));
    }
    if (h->shadow_views.empty()) return AWSM_OK;      // no face sees a candidate: no pass, every pixel lit
    std::vector<AwsmShadowView> views(h->shadow_views.size());
    for (size_t i = 0; i < views.size(); i++)
        views[i] = AwsmShadowView{h->shadow_views[i].block, 512, h->shadow_views[i].casters.data(), (uint32_t)h->shadow_views[i].casters.size()};
    const int rc = several ? h->be.shadow_pass_views(h->ctx, &s, views.data(), (uint32_t)views.size())
                           : h->be.shadow_pass(h->ctx, &s, views[0].light_camera, 512, views[0].casters, views[0].n_casters);
    if (rc) { h->shadow_views.clear(); return dev_fail(h, rc, several ? "shadow_pass_views" : "shadow_pass"); }
    memcpy(h->shadow_block, h->shadow_views[0].block, 512);      // (view 0, for what reads one block and one list)
    h->shadow_casters = h->shadow_views[0].casters;
    h->shadow_rendered = true;
    return AWSM_OK;
}

// Temporal anti-aliasing: the host jitters the projection, composes the reprojection matrix and hands the backend a record per frame.
int awsm_host_set_taa(AwsmHost* h, const AwsmHostTaa* taa) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->be.set_taa) return fail(h, AWSM_ERR_UNSUPPORTED, "set_taa: the backend library has no %s", "awsm_hip_set_taa");
    if (!taa) {
        const int rc = h->be.set_taa(h->ctx, nullptr);
        if (rc) return dev_fail(h, rc, "set_taa");
        if (h->taa_on) h->camera_dirty = true;      // the unjittered block goes up again
        h->taa_on = false; h->taa_have_last = false; h->taa_reset = true;
        return AWSM_OK;
    }
    if (taa->struct_size < 4u || taa->struct_size > 4096u) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_taa: AwsmHostTaa.struct_size = %u (set it to sizeof(AwsmHostTaa))", taa->struct_size);
    AwsmHostTaa full{(uint32_t)sizeof(AwsmHostTaa), 0.1f, 0.8f, 0.2f};
    const size_t known = std::min<size_t>(taa->struct_size, sizeof full) & ~(size_t)3;      // whole fields only
    memcpy((uint8_t*)&full + 4, (const uint8_t*)taa + 4, known - 4);
    if (!std::isfinite(full.feedback) || !(full.feedback > 0.0f && full.feedback <= 1.0f)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_taa: feedback = %g (0 < feedback <= 1)", (double)full.feedback);
    if (!std::isfinite(full.strength_still) || !std::isfinite(full.strength_moving)) return fail(h, AWSM_ERR_INVALID_ARGUMENT, "set_taa: a jitter strength is not finite");
    if (!h->taa_on) { h->taa_have_last = false; h->taa_reset = true; }
    h->taa = full;
    h->taa_on = true;
    return AWSM_OK;
}
int awsm_host_taa_jitter(AwsmHost* h, uint32_t frame_count, int moved, float out_ndc[2]) {
    if (!h || !out_ndc) return AWSM_ERR_INVALID_ARGUMENT;
    if (!h->width) return fail(h, AWSM_ERR_NOT_READY, "taa_jitter before resize");
    taa_jitter_ndc(frame_count, moved ? h->taa.strength_moving : h->taa.strength_still, (float)h->width, (float)h->height, out_ndc);
    return AWSM_OK;
}

// back to no post pass (this library's default; the reference always runs the effects and display passes)
int awsm_host_clear_post_processing(AwsmHost* h) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    h->post_on = false;
    return AWSM_OK;
}

// CameraMatrices.focus_distance / .aperture (camera.rs:40-52, written at bytes 496-503 by camera.rs:200-215)
int awsm_host_camera_set_dof(AwsmHost* h, float focus_distance, float aperture) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    h->dof_params[0] = focus_distance; h->dof_params[1] = aperture;
    memcpy(h->camera_raw + 496, h->dof_params, 8);
    h->camera_dirty = true;
    return AWSM_OK;
}

int awsm_host_set_render_hooks(AwsmHost* h, AwsmHostHook after_geometry_pass, void* user_geometry, AwsmHostHook after_opaque_pass, void* user_opaque) {
    if (!h) return AWSM_ERR_INVALID_ARGUMENT;
    h->after_geometry = after_geometry_pass; h->after_geometry_user = user_geometry;
    h->after_opaque = after_opaque_pass; h->after_opaque_user = user_opaque;
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ introspection
int awsm_host_mirror(AwsmHost* h, AwsmBuf which, const uint8_t** data, size_t* len) {
    const std::vector<uint8_t>* v = nullptr;
    switch (which) {
        case AWSM_BUF_TRANSFORMS: v = &h->transforms_buf.raw(); break;
        case AWSM_BUF_NORMAL_MATS: v = &h->normals_buf.raw(); break;
        case AWSM_BUF_MATERIALS: v = &h->materials_buf.raw(); break;
        case AWSM_BUF_SKIN_MATRICES: sync_skin_mirror(h); v = &h->skin_matrices.raw(); break;
        case AWSM_BUF_SKIN_INDEX_WEIGHTS: v = &h->skin_index_weights.raw(); break;
        case AWSM_BUF_MORPH_WEIGHTS: v = &h->morph_weights.raw(); break;
        case AWSM_BUF_MORPH_VALUES: v = &h->morph_values.raw(); break;
        case AWSM_BUF_GEOM_META: v = &h->geom_meta.raw(); break;
        case AWSM_BUF_MATERIAL_META: v = &h->material_meta.raw(); break;
        case AWSM_BUF_VIS_GEOM_DATA: v = &h->vis_data.raw(); break;
        case AWSM_BUF_VIS_GEOM_INDEX: v = &h->vis_index.raw(); break;
        case AWSM_BUF_ATTR_DATA: v = &h->attr_data.raw(); break;
        case AWSM_BUF_ATTR_INDEX: v = &h->attr_index.raw(); break;
        case AWSM_BUF_TEXTURE_TRANSFORMS: v = &h->tex_transforms_buf.raw(); break;
        case AWSM_BUF_INSTANCES: v = &h->instances.raw(); break;
        case AWSM_BUF_TRANSPARENCY_GEOM_DATA: v = &h->tr_data.raw(); break;
        case AWSM_BUF_CAMERA: *data = h->camera_raw; *len = 512; return AWSM_OK;
        default: return fail(h, AWSM_ERR_INVALID_ARGUMENT, "mirror: buffer %d has no persistent mirror", (int)which);
    }
    *data = v->data(); *len = v->size();
    return AWSM_OK;
}

int awsm_host_transparent_draw_list(AwsmHost* h, AwsmDraw* out, uint32_t cap, uint32_t* n) {
    std::vector<AwsmDraw> d, t;
    collect_draws(h, d, &t);
    *n = (uint32_t)t.size();
    if (out) memcpy(out, t.data(), std::min<size_t>(cap, t.size()) * sizeof(AwsmDraw));
    return AWSM_OK;
}

int awsm_host_hud_draw_lists(AwsmHost* h, AwsmDraw* geometry_out, AwsmDraw* transparent_out, uint32_t cap, uint32_t* n) {
    std::vector<AwsmDraw> d, t, hg, ht;
    collect_draws(h, d, &t, &hg, &ht);
    *n = (uint32_t)hg.size();      // the same meshes through both passes
    if (geometry_out) memcpy(geometry_out, hg.data(), std::min<size_t>(cap, hg.size()) * sizeof(AwsmDraw));
    if (transparent_out) memcpy(transparent_out, ht.data(), std::min<size_t>(cap, ht.size()) * sizeof(AwsmDraw));
    return AWSM_OK;
}

int awsm_host_draw_list(AwsmHost* h, AwsmDraw* out, uint32_t cap, uint32_t* n) {
    std::vector<AwsmDraw> d;
    collect_draws(h, d);
    *n = (uint32_t)d.size();
    if (out) memcpy(out, d.data(), std::min<size_t>(cap, d.size()) * sizeof(AwsmDraw));
    return AWSM_OK;
}

uint32_t awsm_host_texture_array_count(AwsmHost* h) { return (uint32_t)h->pool.size(); }
int awsm_host_texture_array_info(AwsmHost* h, uint32_t i, uint32_t* w, uint32_t* ht, uint32_t* layers, const uint8_t** texels) {
    if (i >= h->pool.size()) return AWSM_ERR_OUT_OF_RANGE;
    {   // layers whose conversion is still owed get it now, by the device's table and integer rule (tex_pool.hpp)
        AwsmHost::PoolArray& a = h->pool[i];
        uint8_t table[256];
        awsm::tex_srgb_table(table);
        const size_t texels = (size_t)a.w * a.h;
        for (uint32_t l = 0; l < a.layers; l++) {
            const uint32_t f = a.flags[l];
            if (!f) continue;
            uint8_t* p = a.texels.data() + (size_t)l * texels * 4;
            for (size_t t = 0; t < texels; t++, p += 4) {
                uint32_t v; memcpy(&v, p, 4);
                if (f & awsm::kTexPremultiplyAlpha) v = awsm::tex_premultiply(v);
                memcpy(p, &v, 4);
                if (f & awsm::kTexSrgbToLinear) { p[0] = table[p[0]]; p[1] = table[p[1]]; p[2] = table[p[2]]; }
            }
            a.flags[l] = 0u;
        }
    }
    *w = h->pool[i].w; *ht = h->pool[i].h; *layers = h->pool[i].layers; *texels = h->pool[i].texels.data();
    return AWSM_OK;
}
uint64_t awsm_host_upload_bytes_last_frame(AwsmHost* h) { return h->upload_bytes; }

// ------------------------------------------------------------------------------------------------ raw allocators (unit tests)
struct AwsmHostDub { DynamicUniformBuffer b; };
struct AwsmHostDsb { DynamicStorageBuffer b; };

AwsmHostDub* awsm_host_dub_new(size_t cap, size_t byte_size, size_t aligned, uint8_t zero) { return new AwsmHostDub{DynamicUniformBuffer(cap, byte_size, aligned, zero)}; }
void awsm_host_dub_free(AwsmHostDub* b) { delete b; }
int awsm_host_dub_update(AwsmHostDub* b, AwsmKey k, const uint8_t* d, size_t n) { return b->b.update(k, d, n) ? 0 : -1; }
int awsm_host_dub_update_offset(AwsmHostDub* b, AwsmKey k, size_t off, const uint8_t* d, size_t n) { return b->b.update_offset(k, off, d, n) ? 0 : -1; }
int awsm_host_dub_remove(AwsmHostDub* b, AwsmKey k) { return b->b.remove(k) ? 1 : 0; }
int64_t awsm_host_dub_offset(AwsmHostDub* b, AwsmKey k) { return b->b.offset(k); }
int64_t awsm_host_dub_slot(AwsmHostDub* b, AwsmKey k) { return b->b.slot_index(k); }
size_t awsm_host_dub_size(AwsmHostDub* b) { return b->b.size(); }
size_t awsm_host_dub_len(AwsmHostDub* b) { return b->b.len(); }
size_t awsm_host_dub_capacity(AwsmHostDub* b) { return b->b.capacity(); }
size_t awsm_host_dub_next_slot(AwsmHostDub* b) { return b->b.next_slot(); }
size_t awsm_host_dub_free_slots(AwsmHostDub* b, size_t* out, size_t cap) {
    const auto& f = b->b.free_slots();
    for (size_t i = 0; i < f.size() && i < cap; i++) out[i] = f[i];
    return f.size();
}
const uint8_t* awsm_host_dub_raw(AwsmHostDub* b) { return b->b.raw().data(); }
int64_t awsm_host_dub_take_resize(AwsmHostDub* b) { return b->b.take_gpu_needs_resize(); }
size_t awsm_host_dub_take_dirty(AwsmHostDub* b, size_t* out, size_t cap) {
    auto r = b->b.take_dirty_ranges();
    for (size_t i = 0; i < r.size() && i < cap; i++) { out[2 * i] = r[i].first; out[2 * i + 1] = r[i].second; }
    return r.size();
}
void awsm_host_dub_force_state(AwsmHostDub* b, size_t next_slot) { b->b.test_force_state(next_slot); }

AwsmHostDsb* awsm_host_dsb_new(size_t initial_bytes, uint8_t zero) { return new AwsmHostDsb{DynamicStorageBuffer(initial_bytes, zero)}; }
void awsm_host_dsb_free(AwsmHostDsb* b) { delete b; }
size_t awsm_host_dsb_update(AwsmHostDsb* b, AwsmKey k, const uint8_t* d, size_t n) { return b->b.update(k, d, n); }
int awsm_host_dsb_patch(AwsmHostDsb* b, AwsmKey k, size_t at, const uint8_t* d, size_t n) {
    return b->b.update_with_unchecked(k, [&](size_t, uint8_t* blk, size_t size) { if (at + n <= size) memcpy(blk + at, d, n); }) ? 0 : -1;
}
void awsm_host_dsb_remove(AwsmHostDsb* b, AwsmKey k) { b->b.remove(k); }
int64_t awsm_host_dsb_offset(AwsmHostDsb* b, AwsmKey k) { return b->b.offset(k); }
int64_t awsm_host_dsb_size_of(AwsmHostDsb* b, AwsmKey k) { return b->b.size_of(k); }
size_t awsm_host_dsb_used_size(AwsmHostDsb* b) { return b->b.used_size(); }
size_t awsm_host_dsb_len(AwsmHostDsb* b) { return b->b.len(); }
size_t awsm_host_dsb_capacity(AwsmHostDsb* b) { return b->b.capacity(); }
size_t awsm_host_dsb_tree_root(AwsmHostDsb* b) { return b->b.tree_root(); }
const uint8_t* awsm_host_dsb_raw(AwsmHostDsb* b) { return b->b.raw().data(); }
int64_t awsm_host_dsb_take_resize(AwsmHostDsb* b) { return b->b.take_gpu_needs_resize(); }
size_t awsm_host_dsb_take_dirty(AwsmHostDsb* b, size_t* out, size_t cap) {
    auto r = b->b.take_dirty_ranges();
    for (size_t i = 0; i < r.size() && i < cap; i++) { out[2 * i] = r[i].first; out[2 * i + 1] = r[i].second; }
    return r.size();
}
size_t awsm_host_round_pow2(size_t n) { return DynamicStorageBuffer::round_pow2(n); }
size_t awsm_host_index_to_offset(size_t idx, size_t leaves) { return DynamicStorageBuffer::index_to_offset(idx, leaves); }
size_t awsm_host_offset_to_index(size_t off, size_t leaves) { return DynamicStorageBuffer::offset_to_index(off, leaves); }
size_t awsm_host_write_plan(size_t raw_len, const size_t* in_pairs, size_t n_in, size_t* out_pairs, size_t cap) {
    std::vector<DirtyRange> r;
    for (size_t i = 0; i < n_in; i++) r.push_back({in_pairs[2 * i], in_pairs[2 * i + 1]});
    auto plan = write_plan(raw_len, r);
    for (size_t i = 0; i < plan.size() && i < cap; i++) { out_pairs[2 * i] = plan[i].first; out_pairs[2 * i + 1] = plan[i].second; }
    return plan.size();
}
int awsm_host_frustum_intersects(const float vp[16], const float mn[3], const float mx[3]) {
    Mat4 m; memcpy(&m, vp, 64);
    return Frustum(m).intersects(Aabb{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}}) ? 1 : 0;
}
void awsm_host_aabb_transformed(const float mat[16], const float mn[3], const float mx[3], float omn[3], float omx[3]) {
    Mat4 m; memcpy(&m, mat, 64);
    Aabb o = aabb_transformed(Aabb{{mn[0], mn[1], mn[2]}, {mx[0], mx[1], mx[2]}}, m);
    omn[0] = o.min.x; omn[1] = o.min.y; omn[2] = o.min.z; omx[0] = o.max.x; omx[1] = o.max.y; omx[2] = o.max.z;
}

}  // extern "C"
