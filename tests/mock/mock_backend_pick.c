/*
 * mock_backend_pick.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the two optional pick entry points the host layer resolves, recording the
 * query and the rectangle they are handed and answering with fixed values (tests/test_pick_cpu.py builds it into a temporary directory).
 */
#include "mock_backend.c"

static AwsmPickQuery g_pick_query;
static int32_t g_pick_args[4];
static int g_pick_calls;
static uint32_t g_pick_entries = 3;      /* distinct pairs pick_rect reports */

int awsm_hip_pick_ex(AwsmHipCtx* c, int32_t x, int32_t y, const AwsmPickQuery* q, AwsmPickHit* out) {
    (void)c;
    if (!q || !out) return AWSM_ERR_INVALID_ARGUMENT;
    g_pick_calls++; g_pick_query = *q; g_pick_args[0] = x; g_pick_args[1] = y;
    if (x < 0) return AWSM_ERR_NOT_READY;      /* a refusal of the backend's */
    *out = (AwsmPickHit){x != 0, 7u, 9u + (q->flags & AWSM_PICK_TRANSPARENT), 2u, q->flags & AWSM_PICK_TRANSPARENT ? 1u : 0u, q->alpha_threshold, 0x3F000000u};
    return AWSM_OK;
}
int awsm_hip_pick_rect(AwsmHipCtx* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, const AwsmPickQuery* q, AwsmPickRectEntry* out, uint32_t cap, uint32_t* n_out) {
    (void)c;
    if (!q || !n_out || (cap && !out)) return AWSM_ERR_INVALID_ARGUMENT;
    g_pick_calls++; g_pick_query = *q; g_pick_args[0] = x0; g_pick_args[1] = y0; g_pick_args[2] = x1; g_pick_args[3] = y1;
    for (uint32_t i = 0; i < g_pick_entries && i < cap; i++) out[i] = (AwsmPickRectEntry){i & 1u, 100u + i, 200u + i, 10u * (i + 1u)};
    *n_out = g_pick_entries;
    return AWSM_OK;
}
int mock_pick_calls(void) { return g_pick_calls; }
void mock_pick_set_entries(uint32_t n) { g_pick_entries = n; }
void mock_pick_last(uint32_t* flags, float* threshold, uint32_t* struct_size, int32_t* args4) {
    *flags = g_pick_query.flags; *threshold = g_pick_query.alpha_threshold; *struct_size = g_pick_query.struct_size; memcpy(args4, g_pick_args, sizeof g_pick_args);
}
