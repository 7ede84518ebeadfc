/*
 * mock_backend_selection.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the two optional selection entry points the host layer resolves,
 * recording what they are handed: the record byte for byte, the key words and the boxes (tests/test_selection_cpu.py builds it into a temporary
 * directory).
 */
#include "mock_backend.c"

static uint8_t g_sel_record[64];
static uint32_t g_sel_record_size;      /* 0xFFFFFFFF: the last call passed NULL */
static uint32_t g_sel_keys[2 * 64], g_sel_n_keys;
static float g_sel_boxes[6 * 64];
static uint32_t g_sel_n_boxes;
static int g_sel_calls;

int awsm_hip_selection_defaults(AwsmSelection* out) {
    if (!out) return AWSM_ERR_INVALID_ARGUMENT;
    *out = (AwsmSelection){(uint32_t)sizeof(AwsmSelection), AWSM_SELECTION_OUTLINE | AWSM_SELECTION_BOXES, 2u, {1.0f, 0.6f, 0.1f, 1.0f}, {1.0f, 0.6f, 0.1f, 0.9f},
                           0.75f, 0.25f, 1e-5f};
    return AWSM_OK;
}
int awsm_hip_set_selection(AwsmHipCtx* c, const AwsmSelection* s, const uint32_t* keys, uint32_t n_keys, const AwsmSelectionBox* boxes, uint32_t n_boxes) {
    (void)c;
    g_sel_calls++;
    if (!s) { g_sel_record_size = 0xFFFFFFFFu; g_sel_n_keys = g_sel_n_boxes = 0; return AWSM_OK; }
    if (s->struct_size < 4u || s->struct_size > sizeof g_sel_record) return AWSM_ERR_INVALID_ARGUMENT;
    if (s->struct_size >= 12u && (s->outline_radius < 1u || s->outline_radius > 4u)) return AWSM_ERR_INVALID_ARGUMENT;      /* one of the real backend's refusals */
    if (n_keys > 64u || n_boxes > 64u || (n_keys && !keys) || (n_boxes && !boxes)) return AWSM_ERR_INVALID_ARGUMENT;
    g_sel_record_size = s->struct_size;
    memcpy(g_sel_record, s, s->struct_size);
    g_sel_n_keys = n_keys; g_sel_n_boxes = n_boxes;
    if (n_keys) memcpy(g_sel_keys, keys, (size_t)n_keys * 8);
    if (n_boxes) memcpy(g_sel_boxes, boxes, (size_t)n_boxes * 24);
    return AWSM_OK;
}
int mock_selection_calls(void) { return g_sel_calls; }
uint32_t mock_selection_record(uint8_t* out, uint32_t cap) {
    if (g_sel_record_size != 0xFFFFFFFFu && g_sel_record_size <= cap) memcpy(out, g_sel_record, g_sel_record_size);
    return g_sel_record_size;
}
uint32_t mock_selection_keys(uint32_t* out, uint32_t cap) {
    memcpy(out, g_sel_keys, (size_t)(g_sel_n_keys < cap ? g_sel_n_keys : cap) * 8);
    return g_sel_n_keys;
}
uint32_t mock_selection_boxes(float* out, uint32_t cap) {
    memcpy(out, g_sel_boxes, (size_t)(g_sel_n_boxes < cap ? g_sel_n_boxes : cap) * 24);
    return g_sel_n_boxes;
}
