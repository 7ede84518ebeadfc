/*
 * mock_backend_shadow.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the two optional shadow entry points the host layer resolves, recording
 * what they are handed byte for byte: the record, the 512-byte light block and the caster draws (tests/test_shadow_cpu.py builds it into a
 * temporary directory).
 */
#include "mock_backend.c"

#define MOCK_SHADOW_MAX_CASTERS 256
static AwsmShadow g_shadow;
static uint8_t g_shadow_block[512];
static AwsmDraw g_shadow_casters[MOCK_SHADOW_MAX_CASTERS];
static uint32_t g_shadow_n;
static size_t g_shadow_bytes;
static int g_shadow_calls, g_shadow_refuse;
static size_t g_shadow_at;      /* the log's length when the pass came: between the geometry pass's entry and the opaque pass's */

int awsm_hip_shadow_defaults(AwsmShadow* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    *out = (AwsmShadow){(uint32_t)sizeof(AwsmShadow), 2048u, 1u, {0.0f, 1.0f, 0.0f, 0.0f}, 1e-3f, 1.0f, 0.05f, 0.7f, 0.1f};
    return AWSM_OK;
}
int awsm_hip_shadow_pass(AwsmHipCtx* c, const AwsmShadow* s, const void* block, size_t bytes, const AwsmDraw* casters, uint32_t n) {
    g_shadow_calls++;
    if (g_shadow_refuse) return g_shadow_refuse;
    if (!s || !block || bytes != 512 || n > MOCK_SHADOW_MAX_CASTERS) return AWSM_ERR_INVALID_ARGUMENT;
    if (!(s->strength >= 0.0f && s->strength <= 1.0f) || s->map_size < 1u || s->map_size > 8192u) return AWSM_ERR_INVALID_ARGUMENT;      /* two of the real backend's refusals */
    g_shadow = *s; g_shadow_bytes = bytes; g_shadow_n = n; g_shadow_at = c->n_log;
    memcpy(g_shadow_block, block, 512);
    if (n) memcpy(g_shadow_casters, casters, n * sizeof(AwsmDraw));
    return AWSM_OK;
}
int mock_shadow_calls(void) { return g_shadow_calls; }
void mock_shadow_refuse(int code) { g_shadow_refuse = code; }
size_t mock_shadow_at(void) { return g_shadow_at; }
uint32_t mock_shadow_last(AwsmShadow* record, uint8_t* block512, AwsmDraw* casters, uint32_t cap) {
    *record = g_shadow;
    memcpy(block512, g_shadow_block, 512);
    memcpy(casters, g_shadow_casters, (g_shadow_n < cap ? g_shadow_n : cap) * sizeof(AwsmDraw));
    return g_shadow_n;
}
