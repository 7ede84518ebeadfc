// launch.hpp — the one declaration of every launch wrapper.  The wrappers are defined in the kernels_*.hip files and called from awsm_hip.cpp and
// awsm_resources.cpp; `extern "C"` names carry no types, so each of those files includes this header and a parameter list that drifts is a
// compile error in the file that defines it and in the files that call it, instead of garbage handed to a kernel launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "frame_params.hpp"
#include "env_cube.hpp"
#include "tex_pool.hpp"
#include "selection.hpp"
#include "pick.hpp"

extern "C" {
// kernels_geometry.hip
void awsm_launch_upload_words(void* dst, const void* src_pinned, uint32_t n_words, hipStream_t s);
void awsm_launch_handoff_signal(uint32_t* flag, uint32_t serial, unsigned long long* stamp, hipStream_t s);
void awsm_launch_handoff_wait(const uint32_t* flag, uint32_t serial, unsigned long long budget_ticks, uint32_t* timeouts_host, uint32_t timeouts_known,
                              uint32_t* poison, uint32_t poison_serial, hipStream_t s);
void awsm_launch_hud_merge(const unsigned long long* world, const unsigned long long* hud, unsigned long long* out, size_t first, size_t n, hipStream_t s);
// (FrameDev::draw_hit_at: k_draw_decide goes in front; FrameDev::clip_from_world == kClipReadBack: the read-back kernel alone — no new wrapper for
// either, the set of wrappers is what the host layer's stand-ins know)
void awsm_launch_transform(const awsm::DevScene* sc, const awsm::FrameDev* f, uint32_t n_blocks, hipStream_t s);
void awsm_launch_transform_forward(const awsm::DevScene* sc, const awsm::FrameDev* f, uint32_t n_blocks, hipStream_t s);
// (FrameDev::bin_rec_at: the count pass writes compact records, bin_record.hpp, the fill pass reads them instead of the set-up records)
void awsm_launch_bin_count(const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_bin_big(const awsm::FrameDev* f, int fill, hipStream_t s);
void awsm_launch_bin_scan(const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_bin_fill(const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_raster(const awsm::FrameDev* f, hipStream_t s);
// kernels_shade.hip
void awsm_launch_resolve_draws(const awsm::DevScene* sc, const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_shade(const awsm::DevScene* sc, const awsm::FrameDev* f, hipStream_t s);
int awsm_shade_is_lean(const awsm::FrameDev* f);
int awsm_launch_shade_todo(const awsm::DevScene* sc, const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_forward(const awsm::DevScene* sc, const awsm::FrameDev* f, const awsm::EditorGridDev* grid, hipStream_t s);
void awsm_launch_editor_grid_layer(const awsm::EditorGridDev* g, uint32_t width, uint32_t height, float* rgba, float* depth, uint8_t* kept, hipStream_t s);
void awsm_launch_msaa_halo_export(const awsm::FrameDev* f, unsigned long long* dst, uint32_t bands_out, hipStream_t s);
void awsm_launch_count_covered(const awsm::FrameDev* f, hipStream_t s);
void awsm_launch_gbuffer_dump(const awsm::FrameDev* f, float* out, hipStream_t s);
void awsm_launch_vis_digest(const unsigned long long* vis, size_t n, unsigned long long* out, hipStream_t s);
void awsm_launch_pick(const awsm::DevScene* sc, const awsm::FrameDev* f, int x, int y, uint32_t* out, hipStream_t s);
void awsm_launch_cube_border(const awsm::CubeDev* cd, uint2* out, uint32_t total, hipStream_t s);
void awsm_launch_brdf_lut(uint32_t* out_rg16f, uint32_t w, uint32_t h, hipStream_t s);
void awsm_launch_rgba16f_to_rg16f(const uint16_t* in, uint32_t* out, uint32_t n, hipStream_t s);
// kernels_post.hip
void awsm_launch_post(const awsm::PostArgs* args, uint32_t flags, uint32_t msaa, void* bloom_a, void* bloom_b, hipStream_t s);
// kernels_ssao.hip
void awsm_launch_ssao(const awsm::SsaoArgs* args, uint32_t msaa, hipStream_t s);
// kernels_shadow.hip
void awsm_launch_shadow_resolve(const awsm::ShadowArgs* args, uint32_t msaa, hipStream_t s);
// kernels_selection.hip
void awsm_launch_selection(const awsm::SelectionDev* args, hipStream_t s);
void awsm_launch_selection_layers(const awsm::SelectionDev* args, hipStream_t s);
// kernels_pick.hip (called from awsm_pick.cpp alone: the frame pipeline's files enqueue none of them)
void awsm_launch_pick_point(const awsm::PickDev* args, hipStream_t s);
void awsm_launch_pick_map(const awsm::PickDev* args, hipStream_t s);
void awsm_launch_pick_rect(const awsm::PickDev* args, hipStream_t s);
// kernels_taa.hip
void awsm_launch_taa(const awsm::TaaArgs* args, uint32_t msaa, hipStream_t s);
void awsm_launch_taa_layers(const awsm::TaaArgs* args, uint32_t msaa, hipStream_t s);
// kernels_env.hip
void awsm_launch_env_write(const awsm::EnvWriteArgs* a, hipStream_t s);
void awsm_launch_env_expand_rows(const uint32_t* rows, const uint16_t* tables, uint2* dst, uint32_t n, hipStream_t s);
void awsm_launch_env_mips(const awsm::EnvMipArgs* a, hipStream_t s);
void awsm_launch_env_filter(const awsm::EnvFilterArgs* a, uint32_t blocks, hipStream_t s);
void awsm_launch_env_filter_level0(const awsm::EnvFilterLevel0Args* a, hipStream_t s);
void awsm_launch_env_from_equirect(const awsm::EnvEquirectArgs* a, hipStream_t s);
// kernels_texture.hip
void awsm_launch_tex_write(const awsm::TexWriteArgs* a, hipStream_t s);
void awsm_launch_tex_mips(const awsm::TexMipArgs* a, hipStream_t s);
void awsm_launch_gen_mip_level(uint8_t* chain, uint32_t src_off, uint32_t dst_off, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t layers,
                               const uint32_t* kinds, hipStream_t s);
// kernels_pose.hip
void awsm_launch_skin_pose(const void* records, const uint32_t* ids_pinned, uint32_t n, const void* transforms, void* skin_matrices, hipStream_t s);
}
