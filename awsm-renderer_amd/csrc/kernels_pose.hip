// kernels_pose.hip — skin matrices composed on the device (include/awsm_hip.h: awsm_hip_skin_pose).
//
// The reference multiplies world * inverse_bind on the CPU for every joint that moved and uploads the 64-byte result
// (/root/reference/crates/renderer/src/meshes/skins.rs:162-194).  The world matrices are already in AWSM_BUF_TRANSFORMS when a frame is submitted,
// so this kernel forms the same products there; 4 bytes of record id per joint cross the bus instead of 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.hpp"

namespace awsm {

constexpr uint32_t kPoseRecordBytes = 72;      // AwsmSkinPoseRecord: u32 transform_offset, u32 matrix_offset, float inverse_bind[16]
constexpr uint32_t kPoseBlock = 256;           // 16 lanes per record: 4 records per wavefront, 16 per workgroup

// Lane (col, row) of a record's 16 stores element [col][row] of W * B exactly as glam's Mat4::mul_mat4 forms it (host/glam.hpp mat4_mul):
//   ((W[0][row] * B[col][0] + W[1][row] * B[col][1]) + W[2][row] * B[col][2]) + W[3][row] * B[col][3]
// with every product and sum rounded on its own (__fmul_rn / __fadd_rn never contract), so the bits are the host's.
// Each lane loads one element of W and one of B — 64 contiguous bytes per record and matrix — and the operands travel between the 16 lanes of the
// group.  The tail of the last wavefront stays in the kernel for those exchanges (its lanes re-read the last valid record) and only skips the store.
// No LDS allocation, no atomics, no scratch.  Bound by launch and memory latency: a frame's list is a few KB.
__global__ __launch_bounds__(kPoseBlock) void k_skin_pose(const uint8_t* __restrict__ records, const uint32_t* __restrict__ ids, uint32_t n,
                                                          const uint8_t* __restrict__ transforms, uint8_t* __restrict__ skin_matrices) {
    const uint32_t item = blockIdx.x * (kPoseBlock / 16u) + (threadIdx.x >> 4);
    const uint32_t lane = threadIdx.x & 15u, col = lane >> 2, row = lane & 3u;
    const bool live = item < n;
    const uint32_t id = __builtin_nontemporal_load(ids + (live ? item : n - 1u));      // the ids lie in pinned host memory: read once
    const uint8_t* rec = records + (size_t)id * kPoseRecordBytes;
    const uint32_t transform_offset = *reinterpret_cast<const uint32_t*>(rec);
    const uint32_t matrix_offset = *reinterpret_cast<const uint32_t*>(rec + 4);
    const float w = *reinterpret_cast<const float*>(transforms + transform_offset + lane * 4u);
    const float b = *reinterpret_cast<const float*>(rec + 8u + lane * 4u);
    const float w0 = __shfl(w, (int)row, 16), w1 = __shfl(w, (int)(4u + row), 16), w2 = __shfl(w, (int)(8u + row), 16), w3 = __shfl(w, (int)(12u + row), 16);
    const float b0 = __shfl(b, (int)(col * 4u), 16), b1 = __shfl(b, (int)(col * 4u + 1u), 16), b2 = __shfl(b, (int)(col * 4u + 2u), 16), b3 = __shfl(b, (int)(col * 4u + 3u), 16);
    const float r = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w0, b0), __fmul_rn(w1, b1)), __fmul_rn(w2, b2)), __fmul_rn(w3, b3));
    if (live) *reinterpret_cast<float*>(skin_matrices + matrix_offset + lane * 4u) = r;
}

}  // namespace awsm

// n >= 1; every id < the record count and every offset inside its buffer: checked by the caller (awsm_hip_skin_pose)
extern "C" void awsm_launch_skin_pose(const void* records, const uint32_t* ids_pinned, uint32_t n, const void* transforms, void* skin_matrices, hipStream_t s) {
    const uint32_t per_block = awsm::kPoseBlock / 16u;
    const uint32_t blocks = (n + per_block - 1u) / per_block;
    if (blocks) hipLaunchKernelGGL(awsm::k_skin_pose, dim3(blocks), dim3(awsm::kPoseBlock), 0, s, (const uint8_t*)records, ids_pinned, n,
                                   (const uint8_t*)transforms, (uint8_t*)skin_matrices);
}
