// awsm_resources.cpp — the load-time and edit-time resource entry points of include/awsm_hip.h: texture arrays and the texture pool at run time
// (DESIGN.md §14), samplers, the environment and its cubes (§12), the device IBL bake (§13) and the BRDF LUT.  They reach the frame pipeline
// (awsm_hip.cpp) through the context and the helpers declared in ctx.hpp, and no further.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "launch.hpp"
#include "env_filter_table.hpp"

using namespace awsm;

extern "C" {

// ---- texture arrays, and the texture pool at run time ----
// (An unnamed namespace inside extern "C" keeps external C names with this compiler, and the library's symbol table is to stay as it is:
// a helper added to one of these blocks is static.)
namespace {

// first texel of each level of a w x h x layers array -> texels in all; false past 2^32 texels
bool tex_level_offsets(uint32_t w, uint32_t h, uint32_t layers, uint32_t mips, uint32_t* level_off, size_t* total) {
    size_t n = 0;
    for (uint32_t l = 0; l < mips; l++) { level_off[l] = (uint32_t)n; n += (size_t)layers * std::max(1u, w >> l) * std::max(1u, h >> l); }
    *total = n;
    return n <= 0xFFFFFFFFull;
}
// The shape of a w x h array of `layers` layers and `mips` levels (0 = 1) -> t's extent and level offsets (t.texels is the caller's) and the texels
// of the whole chain; or the refusal, under the entry's name.  Nothing has been allocated, waited for or written when it refuses.
static int tex_shape(AwsmHipCtx* c, const char* where, uint32_t w, uint32_t h, uint32_t layers, uint32_t mips, TexArrayDev* t, size_t* texels_total) {
    if (layers > 65536u) return fail(c, AWSM_ERR_UNSUPPORTED, "%s: %u layers (the per-draw texture records hold a 16-bit layer)", where, layers);
    const uint32_t full = mip_levels_full(w, h);
    if (mips == 0) mips = 1;
    if (mips > full || mips > (uint32_t)kMaxMipLevels) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: %u mip levels, a %ux%u texture has at most %u", where, mips, w, h, full);
    if (!tex_level_offsets(w, h, layers, mips, t->level_off, texels_total)) return fail(c, AWSM_ERR_UNSUPPORTED, "%s: array larger than 2^32 texels", where);
    t->width = w; t->height = h; t->layers = layers; t->mips = mips;
    return AWSM_OK;
}
// A source of more than 4 MiB (texture layers, cube faces) goes to env_stage straight from the caller's memory: `src` may be pageable and is not
// retained, so this is the one wait of a write.  env_stage grows (and then waits for the stream) only until it fits the largest source seen.
static int stage_large_source(AwsmHipCtx* c, const uint8_t* src, size_t used) {
    int rc = dev_reserve(c, c->env_stage, used);
    if (rc) return rc;
    if (!c->ev_env_copy) HIPCHK(c, hipEventCreateWithFlags(&c->ev_env_copy, hipEventDisableTiming));
    HIPCHK(c, hipMemcpyAsync(c->env_stage.ptr, src, used, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_env_copy, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev_env_copy));
    return AWSM_OK;
}
// The per-array kinds buffer holds a word per layer.  An array made by awsm_hip_texture_array_upload gets its buffer here, zero-filled, at the first
// call that needs it: a fresh allocation, nothing to wait for.  (After an _upload with more layers than before the old buffer is replaced, which
// waits like any reallocation; _create and _resize_layers size it themselves.)
int tex_kinds_ready(AwsmHipCtx* c, uint32_t array_idx, uint32_t layers) {
    DevBuf& k = c->tex_kinds[array_idx];
    if (k.ptr && k.size >= (size_t)layers * 4) return AWSM_OK;
    return dev_realloc(c, k, (size_t)layers * 4, true);
}
const TexArrayDev* tex_array(AwsmHipCtx* c, uint32_t array_idx, const char* where, int* rc) {
    if (!c) { *rc = AWSM_ERR_INVALID_ARGUMENT; return nullptr; }
    if (array_idx >= (uint32_t)kMaxTexArrays) { *rc = fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: array %u (0..%d)", where, array_idx, kMaxTexArrays - 1); return nullptr; }
    const TexArrayDev* t = &c->scene.tex[array_idx];
    if (!t->texels) { *rc = fail(c, AWSM_ERR_NOT_READY, "%s: array %u was never created or uploaded", where, array_idx); return nullptr; }
    return t;
}

}  // namespace

int awsm_hip_texture_array_upload(AwsmHipCtx* c, uint32_t array_idx, uint32_t width, uint32_t height, uint32_t layers,
                                  uint32_t mips, AwsmTexFormat fmt, const void* texels) {
    if (!c || array_idx >= (uint32_t)kMaxTexArrays || !texels || width == 0 || height == 0 || layers == 0)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "texture_array_upload: bad argument");
    if (fmt != AWSM_TEX_RGBA8_UNORM) return fail(c, AWSM_ERR_UNSUPPORTED, "texture_array_upload: only RGBA8_UNORM");
    TexArrayDev t{};
    size_t texels_total = 0;
    int rc = tex_shape(c, "texture_array_upload", width, height, layers, mips, &t, &texels_total);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    if ((rc = dev_realloc(c, c->tex[array_idx], texels_total * 4 + 16, false))) return rc;   // +16: the shade kernel's paired row loads may read one texel past the end
    HIPCHK(c, hipMemcpyAsync(c->tex[array_idx].ptr, texels, (size_t)width * height * layers * 4, hipMemcpyHostToDevice, c->stream));      // level 0
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t.texels = (const uint8_t*)c->tex[array_idx].ptr;
    c->scene.tex[array_idx] = t;
    c->scene.n_tex = std::max(c->scene.n_tex, array_idx + 1);
    c->scene_dirty = true;
    return AWSM_OK;
}

int awsm_hip_texture_array_generate_mips(AwsmHipCtx* c, uint32_t array_idx, const uint32_t* kind_per_layer) {
    if (!c || array_idx >= (uint32_t)kMaxTexArrays) return AWSM_ERR_INVALID_ARGUMENT;
    const TexArrayDev& t = c->scene.tex[array_idx];
    if (!t.texels) return fail(c, AWSM_ERR_NOT_READY, "generate_mips: array %u was never uploaded", array_idx);
    if (t.mips < 2) return AWSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    std::vector<uint32_t> kinds(t.layers, 0u);
    if (kind_per_layer) kinds.assign(kind_per_layer, kind_per_layer + t.layers);
    int rc = dev_reserve(c, c->mip_kinds, kinds.size() * 4);
    if (rc) return rc;
    if ((rc = upload_small(c, c->mip_kinds.ptr, kinds.data(), kinds.size() * 4))) return rc;
    for (uint32_t l = 1; l < t.mips; l++)
        awsm_launch_gen_mip_level((uint8_t*)c->tex[array_idx].ptr, t.level_off[l - 1], t.level_off[l], std::max(1u, t.width >> (l - 1)), std::max(1u, t.height >> (l - 1)),
                                  std::max(1u, t.width >> l), std::max(1u, t.height >> l), t.layers, (const uint32_t*)c->mip_kinds.ptr, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));   // mip_kinds may be reused by the next call
    return AWSM_OK;
}

int awsm_hip_texture_array_read_level(AwsmHipCtx* c, uint32_t array_idx, uint32_t level, void* out) {
    if (!c || !out || array_idx >= (uint32_t)kMaxTexArrays) return AWSM_ERR_INVALID_ARGUMENT;
    const TexArrayDev& t = c->scene.tex[array_idx];
    if (!t.texels || level >= t.mips) return fail(c, AWSM_ERR_OUT_OF_RANGE, "texture_array_read_level: array %u has %u levels", array_idx, t.mips);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)t.layers * std::max(1u, t.width >> level) * std::max(1u, t.height >> level) * 4;
    HIPCHK(c, hipMemcpy(out, t.texels + (size_t)t.level_off[level] * 4, n, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

int awsm_hip_texture_array_create(AwsmHipCtx* c, uint32_t array_idx, uint32_t width, uint32_t height, uint32_t layers, uint32_t mips) {
    if (!c || array_idx >= (uint32_t)kMaxTexArrays || width == 0 || height == 0 || layers == 0)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "texture_array_create: bad argument");
    TexArrayDev t{};
    size_t texels_total = 0;
    int rc = tex_shape(c, "texture_array_create", width, height, layers, mips, &t, &texels_total);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    if ((rc = dev_realloc(c, c->tex[array_idx], texels_total * 4 + 16, true))) return rc;   // +16: as awsm_hip_texture_array_upload
    if ((rc = dev_realloc(c, c->tex_kinds[array_idx], (size_t)layers * 4, true))) return rc;
    t.texels = (const uint8_t*)c->tex[array_idx].ptr;
    c->scene.tex[array_idx] = t;
    c->scene.n_tex = std::max(c->scene.n_tex, array_idx + 1);
    c->scene_dirty = true;
    return AWSM_OK;
}

int awsm_hip_texture_array_resize_layers(AwsmHipCtx* c, uint32_t array_idx, uint32_t layers) {
    int rc = AWSM_OK;
    const TexArrayDev* tp = tex_array(c, array_idx, "texture_array_resize_layers", &rc);
    if (!tp) return rc;
    const TexArrayDev old = *tp;
    if (layers < old.layers) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "texture_array_resize_layers: %u layers, the array holds %u (layers are never removed)", layers, old.layers);
    if (layers == old.layers) return AWSM_OK;
    TexArrayDev t = old;
    size_t texels_total = 0;
    if ((rc = tex_shape(c, "texture_array_resize_layers", old.width, old.height, layers, old.mips, &t, &texels_total))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    // the new chain and the new kinds, filled on the device in stream order: each level's layers go to their new offset, the rest is zero
    DevBuf chain{}, kinds{};
    const size_t chain_bytes = texels_total * 4 + 16;
    HIPCHK(c, hipMalloc(&chain.ptr, chain_bytes));
    chain.size = chain_bytes;
    hipError_t e = hipMalloc(&kinds.ptr, (size_t)layers * 4);
    if (e != hipSuccess) { (void)hipFree(chain.ptr); return fail(c, e == hipErrorOutOfMemory ? AWSM_ERR_OUT_OF_MEMORY : AWSM_ERR_DEVICE, "texture_array_resize_layers: hipMalloc failed: %s", hipGetErrorString(e)); }
    kinds.size = (size_t)layers * 4;
    auto step = [&](hipError_t err) { if (e == hipSuccess) e = err; };
    for (uint32_t l = 0; l < old.mips; l++) {
        const size_t per_layer = (size_t)std::max(1u, old.width >> l) * std::max(1u, old.height >> l) * 4;
        uint8_t* dst = (uint8_t*)chain.ptr + (size_t)t.level_off[l] * 4;
        step(hipMemcpyAsync(dst, old.texels + (size_t)old.level_off[l] * 4, per_layer * old.layers, hipMemcpyDeviceToDevice, c->stream));
        step(hipMemsetAsync(dst + per_layer * old.layers, 0, per_layer * (layers - old.layers), c->stream));
    }
    step(hipMemsetAsync((uint8_t*)chain.ptr + texels_total * 4, 0, 16, c->stream));
    step(hipMemsetAsync(kinds.ptr, 0, kinds.size, c->stream));
    if (c->tex_kinds[array_idx].ptr)
        step(hipMemcpyAsync(kinds.ptr, c->tex_kinds[array_idx].ptr, std::min(c->tex_kinds[array_idx].size, (size_t)old.layers * 4), hipMemcpyDeviceToDevice, c->stream));
    // as a reallocation in awsm_hip_texture_array_upload: nothing in flight may still read the old chain when it is freed
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = sync_shade_streams(c);
    if (e != hipSuccess) {
        (void)hipFree(chain.ptr); (void)hipFree(kinds.ptr);
        return fail(c, AWSM_ERR_DEVICE, "texture_array_resize_layers: %s", hipGetErrorString(e));
    }
    (void)hipFree(c->tex[array_idx].ptr);
    if (c->tex_kinds[array_idx].ptr) (void)hipFree(c->tex_kinds[array_idx].ptr);
    c->tex[array_idx] = chain;
    c->tex_kinds[array_idx] = kinds;
    t.texels = (const uint8_t*)chain.ptr;
    c->scene.tex[array_idx] = t;
    c->scene_dirty = true;      // k_resolve_draws forms the lean records again: their closed-form level offsets multiply by `layers`
    return AWSM_OK;
}

int awsm_hip_texture_array_write_layers(AwsmHipCtx* c, uint32_t array_idx, uint32_t first_layer, uint32_t n_layers, const void* data, size_t data_len,
                                        const AwsmTexWrite* write) {
    int rc = AWSM_OK;
    const TexArrayDev* tp = tex_array(c, array_idx, "texture_array_write_layers", &rc);
    if (!tp) return rc;
    const TexArrayDev t = *tp;
    static_assert(sizeof(TexWriteDesc) == sizeof(AwsmTexWrite), "TexWriteDesc mirrors AwsmTexWrite");
    size_t used = 0;
    char why[128];
    if ((rc = tex_write_validate(t.width, t.height, t.layers, first_layer, n_layers, data != nullptr, data_len, reinterpret_cast<const TexWriteDesc*>(write), &used, why, sizeof why)))
        return fail(c, rc, "texture_array_write_layers: %s (array %u: %ux%u x %u layers; layers [%u, +%u), %zu bytes)", why, array_idx, t.width, t.height, t.layers, first_layer, n_layers, data_len);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = tex_kinds_ready(c, array_idx, t.layers))) return rc;
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    if (!c->tex_srgb_made) { tex_srgb_table(reinterpret_cast<uint8_t*>(c->tex_srgb)); c->tex_srgb_made = true; }
    const uint8_t* src = (const uint8_t*)data + write->offset;
    TexWriteArgs a{};
    if (used <= (4u << 20)) {      // the kernel gathers from the pinned ring itself (device-visible at the same address): no device copy of the source
        uint8_t* st;               // (cube_write copies its slice of the ring to env_stage first: the two small-source routes differ on purpose, neither measured against the other)
        if ((rc = stage_alloc(c, used, &st))) return rc;
        memcpy(st, src, used);
        a.src = st;
    } else {
        if ((rc = stage_large_source(c, src, used))) return rc;
        a.src = (const uint8_t*)c->env_stage.ptr;
    }
    a.dst = (uint32_t*)c->tex[array_idx].ptr + (size_t)first_layer * t.width * t.height;
    a.width = t.width; a.height = t.height; a.n_layers = n_layers; a.flags = write->flags;
    a.bytes_per_row = write->bytes_per_row; a.image_stride = (uint64_t)write->bytes_per_row * write->rows_per_image;
    memcpy(a.srgb, c->tex_srgb, sizeof a.srgb);
    awsm_launch_tex_write(&a, c->stream);
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> kinds(n_layers, write->mipmap_kind);
    return upload_small(c, (uint32_t*)c->tex_kinds[array_idx].ptr + first_layer, kinds.data(), kinds.size() * 4);
}

int awsm_hip_texture_array_generate_mips_layers(AwsmHipCtx* c, uint32_t array_idx, uint32_t first_layer, uint32_t n_layers) {
    int rc = AWSM_OK;
    const TexArrayDev* tp = tex_array(c, array_idx, "texture_array_generate_mips_layers", &rc);
    if (!tp) return rc;
    const TexArrayDev t = *tp;
    if (n_layers == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "texture_array_generate_mips_layers: n_layers must be non-zero");
    if ((uint64_t)first_layer + n_layers > t.layers)
        return fail(c, AWSM_ERR_OUT_OF_RANGE, "texture_array_generate_mips_layers: layers [%u, +%u) of an array of %u", first_layer, n_layers, t.layers);
    if (t.mips < 2) return AWSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = tex_kinds_ready(c, array_idx, t.layers))) return rc;
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    for (uint32_t l = 1; l < t.mips; l += 5u) {      // five levels per launch, each launch from the stored level above its first
        TexMipArgs a{};
        a.chain = (uint32_t*)c->tex[array_idx].ptr; a.kinds = (const uint32_t*)c->tex_kinds[array_idx].ptr;
        a.layers = t.layers; a.first_layer = first_layer; a.n_layers = n_layers;
        a.src_off = t.level_off[l - 1]; a.sw = std::max(1u, t.width >> (l - 1)); a.sh = std::max(1u, t.height >> (l - 1));
        a.n_levels = std::min(5u, t.mips - l);
        for (uint32_t k = 0; k < a.n_levels; k++) a.dst_off[k] = t.level_off[l + k];
        awsm_launch_tex_mips(&a, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int awsm_hip_texture_array_info(AwsmHipCtx* c, uint32_t array_idx, uint32_t* width, uint32_t* height, uint32_t* layers, uint32_t* mips) {
    int rc = AWSM_OK;
    const TexArrayDev* t = tex_array(c, array_idx, "texture_array_info", &rc);
    if (!t) return rc;
    if (width) *width = t->width;
    if (height) *height = t->height;
    if (layers) *layers = t->layers;
    if (mips) *mips = t->mips;
    return AWSM_OK;
}

int awsm_hip_sampler_set(AwsmHipCtx* c, uint32_t idx, const AwsmSampler* s) {
    if (!c || !s || idx >= (uint32_t)kMaxSamplers) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "sampler_set: bad argument");
    if (s->address_mode_u > 2 || s->address_mode_v > 2 || s->mag_filter > 1) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "sampler_set: bad enum value");
    c->scene.samplers[idx] = *s;
    c->scene.n_samplers = std::max(c->scene.n_samplers, idx + 1);
    c->scene_dirty = true;
    return AWSM_OK;
}

int awsm_hip_env_upload(AwsmHipCtx* c, const AwsmEnv* env) {
    if (!c || !env) return AWSM_ERR_INVALID_ARGUMENT;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    memcpy(c->scene.skybox_rgba, env->skybox_rgba, 16);
    memcpy(c->scene.prefiltered_rgb, env->prefiltered_rgb, 16);
    memcpy(c->scene.irradiance_rgb, env->irradiance_rgb, 16);
    if (env->brdf_lut_rgba16f) {
        if (env->brdf_lut_width == 0 || env->brdf_lut_height == 0 || env->brdf_lut_width > 8192 || env->brdf_lut_height > 8192)
            return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_upload: LUT size %ux%u (1..8192 per side)", env->brdf_lut_width, env->brdf_lut_height);
        const size_t n = (size_t)env->brdf_lut_width * env->brdf_lut_height;
        DevBuf tmp;
        int rc = dev_realloc(c, tmp, n * 8, false);
        if (rc) return rc;
        if ((rc = dev_realloc(c, c->lut, n * 4, false))) { (void)hipFree(tmp.ptr); return rc; }
        hipError_t e = hipMemcpyAsync(tmp.ptr, env->brdf_lut_rgba16f, n * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) { awsm_launch_rgba16f_to_rg16f((const uint16_t*)tmp.ptr, (uint32_t*)c->lut.ptr, (uint32_t)n, c->stream); e = hipStreamSynchronize(c->stream); }   // only .rg is sampled (brdf.wgsl:301)
        (void)hipFree(tmp.ptr);
        if (e != hipSuccess) return fail(c, AWSM_ERR_DEVICE, "env_upload: LUT upload failed: %s", hipGetErrorString(e));
        c->scene.lut_w = env->brdf_lut_width; c->scene.lut_h = env->brdf_lut_height;
    }
    c->scene_dirty = true;
    return AWSM_OK;
}

namespace {

// a size^2 cube of `mips` levels is one this library holds, or the refusal under the entry's name
static int cube_shape_ok(AwsmHipCtx* c, const char* where, uint32_t size, uint32_t mips) {
    if (size == 0 || size > 8192 || mips == 0 || mips > (uint32_t)kMaxMipLevels || mips > mip_levels_full(size, size))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: %u mip levels of a %u^2 cube (1..8192 per side, at most %u levels)", where, mips, size, size ? mip_levels_full(size, size) : 0u);
    return AWSM_OK;
}
// The chain and the aproned chain of a size^2 cube with `mips` levels: (re)allocates c->cube_tex / c->cube_bordered[which] (contents undefined; the old
// allocation is kept when the byte size is unchanged) and describes them in cd; cd.bordered stays null until the caller has filled the apron.
int cube_reserve(AwsmHipCtx* c, int which, uint32_t size, uint32_t mips, CubeDev& cd, size_t& total, size_t& b_total, bool& aproned) {
    cd = CubeDev{};
    total = 0;
    for (uint32_t l = 0; l < mips; l++) { cd.level_off[l] = (uint32_t)total; const size_t n = std::max(1u, size >> l); total += 6 * n * n; }
    int rc = dev_realloc(c, c->cube_tex[which], total * 8, false);
    if (rc) return rc;
    b_total = 0;
    for (uint32_t l = 0; l < mips; l++) { cd.b_level_off[l] = (uint32_t)b_total; const size_t n = std::max(1u, size >> l) + 2; b_total += 6 * n * n; }
    aproned = b_total < (1ull << 29);      // byte offsets into the aproned chain are 32-bit; a larger cube keeps the general sampler on the lean route too
    rc = dev_realloc(c, c->cube_bordered[which], aproned ? b_total * 8 : 0, false);
    if (rc) return rc;
    cd.texels = (const uint2*)c->cube_tex[which].ptr; cd.size = size; cd.mips = mips;
    return AWSM_OK;
}

}  // namespace

int awsm_hip_env_cube_upload(AwsmHipCtx* c, AwsmCube which, uint32_t size, uint32_t mips, const uint16_t* texels) {
    if (!c || (int)which < 0 || (int)which > 2) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_upload: bad cube id %d", (int)which);
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    CubeDev cd{};
    if (!texels) {   // back to the uniform colour
        int rc = sync_all(c);
        if (rc) return rc;
        rc = dev_realloc(c, c->cube_tex[which], 0, false);
        if (!rc) rc = dev_realloc(c, c->cube_bordered[which], 0, false);
        if (rc) return rc;
        c->scene.cube[which] = cd;
        c->scene_dirty = true;
        return AWSM_OK;
    }
    int rc = cube_shape_ok(c, "env_cube_upload", size, mips);
    if (rc) return rc;
    size_t total, b_total; bool aproned;
    rc = cube_reserve(c, which, size, mips, cd, total, b_total, aproned);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->cube_tex[which].ptr, texels, total * 8, hipMemcpyHostToDevice, c->stream));
    if (aproned) awsm_launch_cube_border(&cd, (uint2*)c->cube_bordered[which].ptr, (uint32_t)b_total, c->stream);      // the apron, from the faces across the edges
    HIPCHK(c, hipStreamSynchronize(c->stream));      // `texels` is not retained
    cd.bordered = aproned ? (const uint2*)c->cube_bordered[which].ptr : nullptr;
    c->scene.cube[which] = cd;
    c->scene_dirty = true;
    return AWSM_OK;
}

// ------------------------------------------------------------------------------------------------ environment cubes at run time
namespace {

// double -> f16 bits, one rounding to nearest even, for v in [0, 1] (the 8-bit tables: "built on the host in double precision and rounded to f16")
uint16_t f16_bits_from_unit_double(double v) {
    if (!(v > 0.0)) return 0;
    int e2;
    (void)std::frexp(v, &e2);                       // v = m * 2^e2, m in [0.5, 1)
    const int e = e2 - 1;                           // v = 1.f * 2^e
    if (e < -14) return (uint16_t)std::nearbyint(std::ldexp(v, 24));       // denormal steps of 2^-24 (1024 = the smallest normal's bits)
    const double m = std::nearbyint(std::ldexp(v, 10 - e));                // 1024 .. 2048, ties to even (the default rounding mode)
    return (uint16_t)(((uint32_t)(e + 15) << 10) + ((uint32_t)m - 1024u)); // m == 2048 carries into the exponent
}

int env_tables(AwsmHipCtx* c) {
    if (c->env_tables.ptr) return AWSM_OK;
    uint16_t t[512];
    for (int q = 0; q < 256; q++) {
        const double u = (double)q / 255.0;
        t[q] = f16_bits_from_unit_double(u);
        t[256 + q] = f16_bits_from_unit_double(srgb_to_linear(u));
    }
    int rc = dev_realloc(c, c->env_tables, sizeof t, false);
    if (!rc) rc = upload_small(c, c->env_tables.ptr, t, sizeof t);
    if (rc && c->env_tables.ptr) { (void)hipFree(c->env_tables.ptr); c->env_tables = DevBuf{}; }
    return rc;
}

// The reference's colours are f64 (Color), written as decimal literals; here they cross the C ABI as f32.  A colour component is therefore read as
// the shortest decimal that names the float — 0.35f means 0.35, not 0.3499999940395355 — so that the 8-bit quantisation below, which the reference
// does in f64, lands on the reference's bytes (the default sky gradient has two exact .5 ties that the float's own value would round the other way).
double color_component(float f) {
    if (!std::isfinite(f)) return (double)f;
    char buf[40];
    for (int digits = 1; digits <= 9; digits++) {
        snprintf(buf, sizeof buf, "%.*g", digits, (double)f);
        if (strtof(buf, nullptr) == f) return strtod(buf, nullptr);
    }
    return (double)f;
}
double clamp_unit(double v) { return v != v ? 0.0 : std::min(std::max(v, 0.0), 1.0); }      // f64::clamp keeps NaN, and `NaN as u8` is 0
// create_color (image/bitmap.rs:183-193): (c.clamp(0.0, 1.0) * 255.0) as u8 per channel — truncated
uint32_t color_rgba8(const float* col) {
    uint32_t w = 0;
    for (int ch = 0; ch < 4; ch++) w |= (uint32_t)(uint8_t)(clamp_unit(color_component(col[ch])) * 255.0) << (8 * ch);
    return w;
}

uint32_t cube_format_bytes(AwsmCubeFormat f) {
    switch (f) {
    case AWSM_CUBE_RGBA16F: return 8;
    case AWSM_CUBE_RGBA32F: return 16;
    case AWSM_CUBE_RGBA8_UNORM: case AWSM_CUBE_RGBA8_SRGB: case AWSM_CUBE_BGRA8_UNORM: case AWSM_CUBE_BGRA8_SRGB:
    case AWSM_CUBE_B10G11R11_UFLOAT: case AWSM_CUBE_E5B9G9R9_UFLOAT: return 4;
    }
    return 0;
}

// the apron of levels [first, end) again, by the seam rule of k_cube_border: the kernel sees those levels as a chain of their own
void cube_reborder(AwsmHipCtx* c, int which, uint32_t first, uint32_t end) {
    const CubeDev& cd = c->scene.cube[which];
    if (!c->cube_bordered[which].ptr || first >= end) return;
    CubeDev sub{};
    sub.texels = cd.texels; sub.size = std::max(1u, cd.size >> first); sub.mips = end - first;
    const size_t p_last = std::max(1u, cd.size >> (end - 1)) + 2, b_end = cd.b_level_off[end - 1] + 6 * p_last * p_last;
    for (uint32_t l = first; l < end; l++) { sub.level_off[l - first] = cd.level_off[l]; sub.b_level_off[l - first] = cd.b_level_off[l] - cd.b_level_off[first]; }
    awsm_launch_cube_border(&sub, (uint2*)c->cube_bordered[which].ptr + cd.b_level_off[first], (uint32_t)(b_end - cd.b_level_off[first]), c->stream);
}

// levels 1.. of the plain chain from level 0, five levels per launch
void cube_mips(AwsmHipCtx* c, int which) {
    const CubeDev& cd = c->scene.cube[which];
    for (uint32_t l = 0; l + 1 < cd.mips; l += 5) {
        EnvMipArgs a{};
        a.chain = (uint2*)c->cube_tex[which].ptr; a.src_off = cd.level_off[l]; a.src_n = std::max(1u, cd.size >> l);
        a.n_levels = std::min(5u, cd.mips - 1 - l);
        for (uint32_t k = 0; k < a.n_levels; k++) a.dst_off[k] = cd.level_off[l + 1 + k];
        awsm_launch_env_mips(&a, c->stream);
    }
}

int cube_id_ok(AwsmHipCtx* c, AwsmCube which, const char* where) {
    if (!c) return AWSM_ERR_INVALID_ARGUMENT;
    if ((int)which < 0 || (int)which > 2) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: bad cube id %d", where, (int)which);
    return AWSM_OK;
}

// a zero-filled (or to-be-filled) cube in place of whatever the binding held; keeps the allocation when the shape is unchanged
int cube_create(AwsmHipCtx* c, AwsmCube which, uint32_t size, uint32_t mips, bool zero, const char* where) {
    int rc = cube_shape_ok(c, where, size, mips);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    CubeDev cd; size_t total, b_total; bool aproned;
    rc = cube_reserve(c, which, size, mips, cd, total, b_total, aproned);
    if (!rc) rc = env_tables(c);
    if (rc) { c->scene.cube[which] = CubeDev{}; c->scene_dirty = true; return rc; }      // a half-made cube is no cube
    if (zero) {
        HIPCHK(c, hipMemsetAsync(c->cube_tex[which].ptr, 0, total * 8, c->stream));
        if (aproned) HIPCHK(c, hipMemsetAsync(c->cube_bordered[which].ptr, 0, b_total * 8, c->stream));      // the apron of zeros is zeros
    }
    cd.bordered = aproned ? (const uint2*)c->cube_bordered[which].ptr : nullptr;
    c->scene.cube[which] = cd;
    c->scene_dirty = true;
    return AWSM_OK;
}

int cube_write(AwsmHipCtx* c, AwsmCube which, uint32_t face, uint32_t layers, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
               const void* data, size_t data_len, const AwsmCubeLayout* layout, const char* where) {
    { int rc = cube_id_ok(c, which, where); if (rc) return rc; }
    if (!data || !layout || layout->struct_size != sizeof(AwsmCubeLayout))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: data, or a layout with struct_size %zu, is missing", where, sizeof(AwsmCubeLayout));
    if (face > 5u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: face %u (0..5 = +X -X +Y -Y +Z -Z)", where, face);
    // validate_dimensions, validate_layout (cubemap.rs:265-323)
    if (width == 0 || height == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update dimensions must be non-zero", where);
    if (width != height) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap faces must be square, got %ux%u", where, width, height);
    if (layout->bytes_per_row == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update bytes_per_row must be non-zero", where);
    if (layout->rows_per_image == 0) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update rows_per_image must be non-zero", where);
    unsigned long long per_layer, total_bytes, required;
    if (__builtin_mul_overflow((unsigned long long)layout->bytes_per_row, (unsigned long long)layout->rows_per_image, &per_layer))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update layout overflow while calculating layer byte size", where);
    if (__builtin_mul_overflow(per_layer, (unsigned long long)layers, &total_bytes))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update layout overflow while calculating total byte size", where);
    if (__builtin_add_overflow((unsigned long long)layout->offset, total_bytes, &required))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update layout overflow while applying data offset", where);
    if ((unsigned long long)data_len < required)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: Cubemap update buffer is too small: need at least %llu bytes, got %zu", where, required, data_len);
    // the destination, and what writeTexture itself would refuse
    const CubeDev cd = c->scene.cube[which];
    if (!cd.texels) return fail(c, AWSM_ERR_NOT_READY, "%s: cube %d was never created or uploaded", where, (int)which);
    if (mip >= cd.mips) return fail(c, AWSM_ERR_OUT_OF_RANGE, "%s: mip level %u, the cube has %u", where, mip, cd.mips);
    const uint32_t bpt = cube_format_bytes(format);
    if (!bpt) return fail(c, AWSM_ERR_UNSUPPORTED, "%s: unknown AwsmCubeFormat %d", where, (int)format);
    const uint32_t n = std::max(1u, cd.size >> mip);
    if (width != n) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: %ux%u texels for mip level %u of a %u^2 cube, which is %ux%u", where, width, height, mip, cd.size, n, n);
    if ((unsigned long long)layout->bytes_per_row < (unsigned long long)width * bpt)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: bytes_per_row %u, a row of %u texels takes %llu bytes", where, layout->bytes_per_row, width, (unsigned long long)width * bpt);
    if (layout->rows_per_image < height) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "%s: rows_per_image %u for %u rows", where, layout->rows_per_image, height);

    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    int rc = env_tables(c);
    if (rc) return rc;
    // only the bytes the gather reads: up to the end of the last row of the last image
    const size_t used = (size_t)per_layer * (layers - 1) + (size_t)layout->bytes_per_row * (height - 1) + (size_t)width * bpt;
    const uint8_t* src = (const uint8_t*)data + layout->offset;
    if (used <= (4u << 20)) {      // through the pinned ring to env_stage; awsm_hip_texture_array_write_layers lets its kernel gather from the ring instead
        uint8_t* st;               // (the two small-source routes differ on purpose, neither measured against the other)
        if ((rc = dev_reserve(c, c->env_stage, used))) return rc;      // as stage_large_source
        if ((rc = stage_alloc(c, used, &st))) return rc;
        memcpy(st, src, used);
        HIPCHK(c, hipMemcpyAsync(c->env_stage.ptr, st, used, hipMemcpyHostToDevice, c->stream));
    } else {
        if ((rc = stage_large_source(c, src, used))) return rc;
    }
    EnvWriteArgs a{};
    a.src = (const uint8_t*)c->env_stage.ptr;
    a.dst = (uint2*)c->cube_tex[which].ptr + cd.level_off[mip] + (size_t)face * n * n;
    a.tables = (const uint16_t*)c->env_tables.ptr;
    a.n = n; a.layers = layers; a.format = (uint32_t)format; a.bytes_per_row = layout->bytes_per_row; a.image_stride = per_layer;
    awsm_launch_env_write(&a, c->stream);
    cube_reborder(c, which, mip, mip + 1);      // the whole level: a face's edge texels are the apron of its four neighbours
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

// level 0 from one RGBA8 colour per face row, then the full chain (CubemapImage::Images { mipmaps: true })
int cube_fill(AwsmHipCtx* c, AwsmCube which, uint32_t size, const std::vector<uint32_t>& rows, const char* where) {
    int rc = cube_create(c, which, size, size ? mip_levels_full(size, size) : 0u, false, where);
    if (rc) return rc;
    if ((rc = dev_reserve(c, c->env_rows, rows.size() * 4))) return rc;
    if ((rc = upload_small(c, c->env_rows.ptr, rows.data(), rows.size() * 4))) return rc;
    awsm_launch_env_expand_rows((const uint32_t*)c->env_rows.ptr, (const uint16_t*)c->env_tables.ptr, (uint2*)c->cube_tex[which].ptr, size, c->stream);
    cube_mips(c, which);
    cube_reborder(c, which, 0, c->scene.cube[which].mips);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

}  // namespace

int awsm_hip_env_cube_create(AwsmHipCtx* c, AwsmCube which, uint32_t size, uint32_t mips) {
    { int rc = cube_id_ok(c, which, "env_cube_create"); if (rc) return rc; }
    return cube_create(c, which, size, mips, true, "env_cube_create");
}

int awsm_hip_env_cube_write_face(AwsmHipCtx* c, AwsmCube which, uint32_t face, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                 const void* data, size_t data_len, const AwsmCubeLayout* layout) {
    return cube_write(c, which, face, 1, mip, width, height, format, data, data_len, layout, "env_cube_write_face");
}

int awsm_hip_env_cube_write_all_faces(AwsmHipCtx* c, AwsmCube which, uint32_t mip, uint32_t width, uint32_t height, AwsmCubeFormat format,
                                      const void* data, size_t data_len, const AwsmCubeLayout* layout) {
    return cube_write(c, which, 0, 6, mip, width, height, format, data, data_len, layout, "env_cube_write_all_faces");
}

int awsm_hip_env_cube_generate_mips(AwsmHipCtx* c, AwsmCube which) {
    { int rc = cube_id_ok(c, which, "env_cube_generate_mips"); if (rc) return rc; }
    const CubeDev& cd = c->scene.cube[which];
    if (!cd.texels) return fail(c, AWSM_ERR_NOT_READY, "env_cube_generate_mips: cube %d was never created or uploaded", (int)which);
    if (cd.mips < 2) return AWSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    cube_mips(c, which);
    cube_reborder(c, which, 1, cd.mips);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int awsm_hip_env_cube_fill_colors(AwsmHipCtx* c, AwsmCube which, uint32_t size, const float rgba[24]) {
    { int rc = cube_id_ok(c, which, "env_cube_fill_colors"); if (rc) return rc; }
    if (!rgba || size == 0 || size > 8192) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_fill_colors: colours missing or size %u (1..8192)", size);
    std::vector<uint32_t> rows((size_t)6 * size);
    for (int f = 0; f < 6; f++) std::fill(rows.begin() + (size_t)f * size, rows.begin() + (size_t)(f + 1) * size, color_rgba8(rgba + f * 4));
    return cube_fill(c, which, size, rows, "env_cube_fill_colors");
}

int awsm_hip_env_cube_fill_sky_gradient(AwsmHipCtx* c, AwsmCube which, uint32_t size, const float zenith[4], const float nadir[4]) {
    { int rc = cube_id_ok(c, which, "env_cube_fill_sky_gradient"); if (rc) return rc; }
    if (!zenith || !nadir || size == 0 || size > 8192) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_fill_sky_gradient: colours missing or size %u (1..8192)", size);
    std::vector<uint32_t> rows((size_t)6 * size);
    const double height_f = size > 1 ? (double)(size - 1) : 1.0;      // create_vertical_gradient (image/bitmap.rs:229-267)
    for (uint32_t y = 0; y < size; y++) {
        const double t = (double)y / height_f;
        uint32_t w = 0;
        for (int ch = 0; ch < 4; ch++) {      // lerp a + (b - a) * t, then (clamp * 255.0).round(): half away from zero
            const double a = color_component(zenith[ch]), b = color_component(nadir[ch]);
            w |= (uint32_t)(uint8_t)std::round(clamp_unit(a + (b - a) * t) * 255.0) << (8 * ch);
        }
        for (int f : {0, 1, 4, 5}) rows[(size_t)f * size + y] = w;
    }
    std::fill(rows.begin() + (size_t)2 * size, rows.begin() + (size_t)3 * size, color_rgba8(zenith));      // +Y: create_color(zenith)
    std::fill(rows.begin() + (size_t)3 * size, rows.begin() + (size_t)4 * size, color_rgba8(nadir));       // -Y: create_color(nadir)
    return cube_fill(c, which, size, rows, "env_cube_fill_sky_gradient");
}

int awsm_hip_env_cube_info(AwsmHipCtx* c, AwsmCube which, uint32_t* size, uint32_t* mips) {
    { int rc = cube_id_ok(c, which, "env_cube_info"); if (rc) return rc; }
    const CubeDev& cd = c->scene.cube[which];
    if (!cd.texels) return fail(c, AWSM_ERR_NOT_READY, "env_cube_info: cube %d is a uniform colour", (int)which);
    if (size) *size = cd.size;
    if (mips) *mips = cd.mips;
    return AWSM_OK;
}

int awsm_hip_env_cube_read_level(AwsmHipCtx* c, AwsmCube which, uint32_t level, uint16_t* out) {
    { int rc = cube_id_ok(c, which, "env_cube_read_level"); if (rc) return rc; }
    if (!out) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_read_level: no destination");
    const CubeDev& cd = c->scene.cube[which];
    if (!cd.texels) return fail(c, AWSM_ERR_NOT_READY, "env_cube_read_level: cube %d was never created or uploaded", (int)which);
    if (level >= cd.mips) return fail(c, AWSM_ERR_OUT_OF_RANGE, "env_cube_read_level: level %u, the cube has %u", level, cd.mips);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = std::max(1u, cd.size >> level);
    HIPCHK(c, hipMemcpy(out, cd.texels + cd.level_off[level], 6 * n * n * 8, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

// DESIGN.md §13.  The destination's levels are made from the source alone: level 0 by k_env_filter_level0, every other prefiltered level (or the one
// irradiance level) by one launch of k_env_filter over tables built here in f64 (env_filter_table.hpp) and uploaded through the staging ring.
int awsm_hip_env_cube_filter(AwsmHipCtx* c, AwsmCube src, AwsmCube dst, const AwsmEnvFilter* f) {
    { int rc = cube_id_ok(c, src, "env_cube_filter"); if (rc) return rc; }
    { int rc = cube_id_ok(c, dst, "env_cube_filter"); if (rc) return rc; }
    if (!f || f->struct_size != sizeof(AwsmEnvFilter)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_filter: a filter with struct_size %zu is missing", sizeof(AwsmEnvFilter));
    if (src == dst) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_filter: cube %d cannot be filtered into itself", (int)src);
    const uint32_t samples = f->sample_count ? f->sample_count : 1024u;
    if (f->kind > 1u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_filter: kind %u (0 GGX chain, 1 Lambert)", f->kind);
    if (samples < 16u || samples > 4096u || (samples & (samples - 1u))) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_filter: %u samples (a power of two, 16..4096)", samples);
    if (f->size == 0 || f->size > 8192 || f->mips == 0 || f->mips > (uint32_t)kMaxMipLevels || f->mips > mip_levels_full(f->size, f->size) || (f->kind == 1u && f->mips != 1u))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_filter: %u mip levels of a %u^2 cube (1..8192 per side; GGX: at most %u levels, Lambert: 1)", f->mips, f->size,
                    f->size ? mip_levels_full(f->size, f->size) : 0u);
    if (!c->scene.cube[src].texels) return fail(c, AWSM_ERR_NOT_READY, "env_cube_filter: source cube %d is a uniform colour", (int)src);
    HIPCHK(c, hipSetDevice(c->device));
    if (c->scene.cube[dst].texels && c->scene.cube[dst].size == f->size && c->scene.cube[dst].mips == f->mips) {
        int rcb = scene_write_barrier(c); if (rcb) return rcb;
    } else {
        int rc = cube_create(c, dst, f->size, f->mips, false, "env_cube_filter"); if (rc) return rc;      // every level is written below
    }
    const CubeDev sd = c->scene.cube[src], dd = c->scene.cube[dst];      // after the create: a reallocation does not move the source
    uint2* out = (uint2*)c->cube_tex[dst].ptr;

    EnvFilterArgs a{};
    a.src = sd; a.dst = out; a.lambert = f->kind; a.k = (float)(kEnvFilterPi / (double)samples);
    std::vector<EnvFilterEntry> tab;
    uint32_t blocks = 0;
    for (uint32_t l = f->kind == 1u ? 0u : 1u; l < f->mips; l++) {
        const std::vector<EnvFilterEntry> t = env_filter_table(f->kind, l, f->mips, samples, sd.size);
        EnvFilterLevel& lv = a.level[a.n_levels++];
        lv.dst_off = dd.level_off[l]; lv.n = std::max(1u, f->size >> l); lv.first_block = blocks;
        lv.table_off = (uint32_t)tab.size(); lv.count = (uint32_t)t.size();
        blocks += (6u * lv.n * lv.n + 3u) / 4u;
        tab.insert(tab.end(), t.begin(), t.end());
    }
    if (!tab.empty()) {
        int rc = dev_reserve(c, c->env_filter_tab, tab.size() * sizeof(EnvFilterEntry));
        if (!rc) rc = upload_small(c, c->env_filter_tab.ptr, tab.data(), tab.size() * sizeof(EnvFilterEntry));
        if (rc) return rc;
        a.tables = (const float*)c->env_filter_tab.ptr;
    }
    if (f->kind == 0u) {
        EnvFilterLevel0Args z{};
        z.src = sd; z.dst = out; z.n = f->size;
        z.lod = (float)std::max(0.0, std::log2((double)sd.size / (double)f->size));
        awsm_launch_env_filter_level0(&z, c->stream);
    }
    awsm_launch_env_filter(&a, blocks, c->stream);
    cube_reborder(c, dst, 0, f->mips);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

// DESIGN.md §16.  Level 0 of an existing texel cube from an equirectangular panorama: the source goes to env_stage as a cube write's does (§12), one
// launch of k_env_from_equirect projects it, and the level's apron is rebuilt.  Everything is checked before anything is enqueued.
int awsm_hip_env_cube_from_equirect(AwsmHipCtx* c, AwsmCube which, const void* data, size_t data_len, const AwsmEquirect* p) {
    { int rc = cube_id_ok(c, which, "env_cube_from_equirect"); if (rc) return rc; }
    if (!data || !p || p->struct_size != sizeof(AwsmEquirect))
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: data, or a panorama description with struct_size %zu, is missing", sizeof(AwsmEquirect));
    if (p->width == 0 || p->height == 0 || p->width > 32768u || p->height > 32768u)
        return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: a %ux%u panorama (1..32768 per side)", p->width, p->height);
    if (p->samples > 8u) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: %u samples per side (0 = auto, else 1..8)", p->samples);
    if (!std::isfinite(p->yaw) || !std::isfinite(p->scale)) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: yaw and scale must be finite");
    if (p->format != (uint32_t)AWSM_PANO_RGBE8 && p->format != (uint32_t)AWSM_PANO_RGBA32F)
        return fail(c, AWSM_ERR_UNSUPPORTED, "env_cube_from_equirect: unknown AwsmPanoFormat %u", p->format);
    const uint32_t bpp = p->format == (uint32_t)AWSM_PANO_RGBE8 ? 4u : 16u;
    const uint64_t tight = (uint64_t)p->width * bpp;
    const uint64_t bpr = p->bytes_per_row ? (uint64_t)p->bytes_per_row : tight;
    if (bpr < tight) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: bytes_per_row %u, a row of %u pixels takes %llu bytes", p->bytes_per_row, p->width, (unsigned long long)tight);
    if (bpr > 0xFFFFFFFFull) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "env_cube_from_equirect: a row of %llu bytes", (unsigned long long)bpr);
    const uint64_t used = bpr * (p->height - 1u) + tight;      // only the bytes the taps read: up to the end of the last row
    if ((uint64_t)data_len < used)
        return fail(c, AWSM_ERR_OUT_OF_RANGE, "env_cube_from_equirect: %zu bytes, a %ux%u panorama with rows of %llu bytes takes %llu", data_len, p->width, p->height,
                    (unsigned long long)bpr, (unsigned long long)used);
    const CubeDev cd = c->scene.cube[which];
    if (!cd.texels) return fail(c, AWSM_ERR_NOT_READY, "env_cube_from_equirect: cube %d is a uniform colour or was never created", (int)which);

    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    int rc;
    if (used <= (4u << 20)) {      // through the pinned ring to env_stage, as cube_write: the taps gather from device memory
        uint8_t* st;
        if ((rc = dev_reserve(c, c->env_stage, (size_t)used))) return rc;
        if ((rc = stage_alloc(c, (size_t)used, &st))) return rc;
        memcpy(st, data, (size_t)used);
        HIPCHK(c, hipMemcpyAsync(c->env_stage.ptr, st, (size_t)used, hipMemcpyHostToDevice, c->stream));
    } else {
        if ((rc = stage_large_source(c, (const uint8_t*)data, (size_t)used))) return rc;
    }
    EnvEquirectArgs a{};
    a.src = (const uint8_t*)c->env_stage.ptr;
    a.dst = (uint2*)c->cube_tex[which].ptr + cd.level_off[0];
    a.n = cd.size; a.width = p->width; a.height = p->height; a.format = p->format; a.bytes_per_row = (uint32_t)bpr;
    // S = clamp(ceil(W / (4 N)), 1, 8): panorama pixels per cube texel along the equator
    a.samples = p->samples ? p->samples : (uint32_t)std::min<uint64_t>(8u, std::max<uint64_t>(1u, ((uint64_t)p->width + 4ull * cd.size - 1u) / (4ull * cd.size)));
    const double turns = (double)p->yaw / 6.283185307179586476925;      // reduced here in f64, so that a yaw of any magnitude costs the kernel's f32 nothing
    a.turn = (float)(turns - std::floor(turns));
    if (!(a.turn < 1.0f)) a.turn = 0.0f;                                 // a hair below a whole turn rounds to 1.0f
    a.scale = p->scale == 0.0f ? 1.0f : p->scale;
    awsm_launch_env_from_equirect(&a, c->stream);
    cube_reborder(c, which, 0, 1);
    HIPCHK(c, hipGetLastError());
    return AWSM_OK;
}

int awsm_hip_brdf_lut_generate(AwsmHipCtx* c, uint32_t width, uint32_t height) {
    if (!c || width == 0 || height == 0 || width > 8192 || height > 8192) return fail(c, AWSM_ERR_INVALID_ARGUMENT, "brdf_lut_generate: bad size");
    HIPCHK(c, hipSetDevice(c->device));
    { int rcb = scene_write_barrier(c); if (rcb) return rcb; }
    int rc = dev_realloc(c, c->lut, (size_t)width * height * 4, false);
    if (rc) return rc;
    awsm_launch_brdf_lut((uint32_t*)c->lut.ptr, width, height, c->stream);
    HIPCHK(c, hipGetLastError());
    c->scene.lut_w = width; c->scene.lut_h = height;
    c->scene_dirty = true;
    return AWSM_OK;
}

int awsm_hip_read_brdf_lut(AwsmHipCtx* c, uint16_t* out) {
    if (!c || !out) return AWSM_ERR_INVALID_ARGUMENT;
    if (!c->lut.ptr) return fail(c, AWSM_ERR_NOT_READY, "no BRDF LUT");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->lut.ptr, (size_t)c->scene.lut_w * c->scene.lut_h * 4, hipMemcpyDeviceToHost));
    return AWSM_OK;
}

}  // extern "C"
