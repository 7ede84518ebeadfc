/*
 * mock_texture_pool.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the five optional awsm_hip_texture_array_* entries of the run-time
 * texture pool, recording what the host layer asks for (tests/test_texture_pool_cpu.py compiles it when it runs).
 *   op 20 create (which = array; a = width | height << 32; b = layers | mips << 32)      op 21 resize_layers (a = layers)
 *   op 22 write_layers (a = first | n << 32; b = flags | kind << 32; the bytes are summed into mock_texture_bytes)
 *   op 23 generate_mips_layers (a = first, b = n)
 */
#include "mock_backend.c"

static uint32_t pool_w[64], pool_h[64], pool_layers[64], pool_mips[64];
static uint64_t texture_bytes;
int awsm_hip_texture_array_create(AwsmHipCtx* c, uint32_t idx, uint32_t w, uint32_t h, uint32_t layers, uint32_t mips) {
    pool_w[idx] = w; pool_h[idx] = h; pool_layers[idx] = layers; pool_mips[idx] = mips;
    logc(c, 20, (int)idx, (uint64_t)w | (uint64_t)h << 32, (uint64_t)layers | (uint64_t)mips << 32); return 0;
}
int awsm_hip_texture_array_resize_layers(AwsmHipCtx* c, uint32_t idx, uint32_t layers) { pool_layers[idx] = layers; logc(c, 21, (int)idx, layers, 0); return 0; }
int awsm_hip_texture_array_write_layers(AwsmHipCtx* c, uint32_t idx, uint32_t first, uint32_t n, const void* data, size_t len, const AwsmTexWrite* w) {
    (void)data; texture_bytes += len;
    logc(c, 22, (int)idx, (uint64_t)first | (uint64_t)n << 32, (uint64_t)w->flags | (uint64_t)w->mipmap_kind << 32); return 0;
}
int awsm_hip_texture_array_generate_mips_layers(AwsmHipCtx* c, uint32_t idx, uint32_t first, uint32_t n) { logc(c, 23, (int)idx, first, n); return 0; }
int awsm_hip_texture_array_info(AwsmHipCtx* c, uint32_t idx, uint32_t* w, uint32_t* h, uint32_t* layers, uint32_t* mips) {
    (void)c; if (w) *w = pool_w[idx]; if (h) *h = pool_h[idx]; if (layers) *layers = pool_layers[idx]; if (mips) *mips = pool_mips[idx]; return 0;
}
uint64_t mock_texture_bytes(void) { return texture_bytes; }
