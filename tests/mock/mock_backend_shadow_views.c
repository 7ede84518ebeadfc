/*
 * mock_backend_shadow_views.c — TEST INFRASTRUCTURE ONLY.  mock_backend_shadow.c plus the optional entry for several views of one light, recording
 * what it is handed byte for byte: the record and, per view, the 512-byte light block and the caster draws (tests/test_shadow_views_cpu.py builds
 * it into a temporary directory).
 */
#include "mock_backend_shadow.c"

#define MOCK_VIEWS_MAX 6
static AwsmShadow g_views_record;
static uint8_t g_views_block[MOCK_VIEWS_MAX][512];
static AwsmDraw g_views_casters[MOCK_VIEWS_MAX][MOCK_SHADOW_MAX_CASTERS];
static uint32_t g_views_n_casters[MOCK_VIEWS_MAX];
static uint32_t g_views_n;
static int g_views_calls, g_views_refuse;
static size_t g_views_at;      /* the log's length when the pass came */

int awsm_hip_shadow_pass_views(AwsmHipCtx* c, const AwsmShadow* s, const AwsmShadowView* views, uint32_t n_views) {
    g_views_calls++;
    if (g_views_refuse) return g_views_refuse;
    if (!s || !views || n_views < 1u || n_views > MOCK_VIEWS_MAX) return AWSM_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_views; i++)
        if (!views[i].light_camera || views[i].camera_bytes != 512 || views[i].n_casters > MOCK_SHADOW_MAX_CASTERS) return AWSM_ERR_INVALID_ARGUMENT;
    g_views_record = *s; g_views_n = n_views; g_views_at = c->n_log;
    for (uint32_t i = 0; i < n_views; i++) {
        memcpy(g_views_block[i], views[i].light_camera, 512);
        g_views_n_casters[i] = views[i].n_casters;
        if (views[i].n_casters) memcpy(g_views_casters[i], views[i].casters, views[i].n_casters * sizeof(AwsmDraw));
    }
    return AWSM_OK;
}
int mock_views_calls(void) { return g_views_calls; }
void mock_views_refuse(int code) { g_views_refuse = code; }
size_t mock_views_at(void) { return g_views_at; }
uint32_t mock_views_count(AwsmShadow* record) { *record = g_views_record; return g_views_n; }
uint32_t mock_views_view(uint32_t view, uint8_t* block512, AwsmDraw* casters, uint32_t cap) {
    memcpy(block512, g_views_block[view], 512);
    memcpy(casters, g_views_casters[view], (g_views_n_casters[view] < cap ? g_views_n_casters[view] : cap) * sizeof(AwsmDraw));
    return g_views_n_casters[view];
}
