/*
 * mock_backend_ssao.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the two optional SSAO entry points the host layer resolves, recording the
 * record they are handed byte for byte (tests/test_ssao_cpu.py builds it into a temporary directory).
 */
#include "mock_backend.c"

static uint8_t g_record[64];
static uint32_t g_record_size;      /* 0xFFFFFFFF: the last call passed NULL */
static int g_calls;

int awsm_hip_ssao_defaults(AwsmSsao* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    *out = (AwsmSsao){(uint32_t)sizeof(AwsmSsao), 0.5f, 1.0f, 0.02f, 1.0f};
    return AWSM_OK;
}
int awsm_hip_set_ssao(AwsmHipCtx* c, const AwsmSsao* s) {
    (void)c;
    g_calls++;
    if (!s) { g_record_size = 0xFFFFFFFFu; return AWSM_OK; }
    if (s->struct_size < 4u || s->struct_size > sizeof g_record) return AWSM_ERR_INVALID_ARGUMENT;
    if (s->struct_size >= 8u && !(s->radius > 0.0f)) return AWSM_ERR_INVALID_ARGUMENT;      /* one of the real backend's refusals */
    g_record_size = s->struct_size;
    memcpy(g_record, s, s->struct_size);
    return AWSM_OK;
}
int mock_ssao_calls(void) { return g_calls; }
uint32_t mock_ssao_record(uint8_t* out, uint32_t cap) {
    if (g_record_size != 0xFFFFFFFFu && g_record_size <= cap) memcpy(out, g_record, g_record_size);
    return g_record_size;
}
