/*
 * mock_backend_taa.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus awsm_hip_post_pass and the optional awsm_hip_set_taa the host layer resolves,
 * recording every record the host hands over byte for byte, in order (tests/test_taa_cpu.py builds it into a temporary directory).
 */
#include "mock_backend.c"

#define MOCK_TAA_CAP 64
static uint8_t g_records[MOCK_TAA_CAP][sizeof(AwsmTaa)];
static uint32_t g_sizes[MOCK_TAA_CAP];      /* 0xFFFFFFFF: that call passed NULL */
static uint32_t g_posts_at[MOCK_TAA_CAP];   /* post passes seen when the record came */
static uint32_t g_calls, g_posts;

int awsm_hip_post_pass(AwsmHipCtx* c, const AwsmPostParams* p) { (void)c; (void)p; g_posts++; return AWSM_OK; }
int awsm_hip_set_taa(AwsmHipCtx* c, const AwsmTaa* t) {
    (void)c;
    const uint32_t i = g_calls++ % MOCK_TAA_CAP;
    g_posts_at[i] = g_posts;
    if (!t) { g_sizes[i] = 0xFFFFFFFFu; return AWSM_OK; }
    if (t->struct_size < 4u || t->struct_size > sizeof(AwsmTaa)) return AWSM_ERR_INVALID_ARGUMENT;
    g_sizes[i] = t->struct_size;
    memcpy(g_records[i], t, t->struct_size);
    return AWSM_OK;
}
uint32_t mock_taa_calls(void) { return g_calls; }
uint32_t mock_taa_posts(void) { return g_posts; }
/* the i-th call since the library was loaded: its size (0xFFFFFFFF for NULL), its bytes, and how many post passes had run before it */
uint32_t mock_taa_record(uint32_t i, uint8_t* out, uint32_t cap, uint32_t* posts_before) {
    const uint32_t k = i % MOCK_TAA_CAP;
    if (posts_before) *posts_before = g_posts_at[k];
    if (g_sizes[k] != 0xFFFFFFFFu && g_sizes[k] <= cap) memcpy(out, g_records[k], g_sizes[k]);
    return g_sizes[k];
}
