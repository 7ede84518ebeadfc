/*
 * mock_skin_pose.c — TEST INFRASTRUCTURE ONLY.  mock_backend.c plus the entries of device skin posing (include/awsm_hip.h: awsm_hip_skin_pose_records_write,
 * awsm_hip_skin_pose, awsm_hip_buffer_read), recording what the host layer asks for and composing the matrices on the CPU in the order the kernel
 * uses (tests/test_animation_host_cpu.py compiles it, with -ffp-contract=off, when it runs).  The records and the last id list are kept per context.
 *   op 30 skin_pose_records_write (a = first, b = n)      op 31 skin_pose (a = n; the ids of the context's last call: mock_pose_ids)
 */
#define awsm_hip_create mock_base_create
#define awsm_hip_destroy mock_base_destroy
#include "mock_backend.c"
#undef awsm_hip_create
#undef awsm_hip_destroy

typedef struct PoseState {
    AwsmHipCtx* ctx;
    AwsmSkinPoseRecord* records; uint32_t count, cap;
    uint32_t* ids; uint32_t n_ids;
    struct PoseState* next;
} PoseState;
static PoseState* pose_states;

static PoseState* pose_of(AwsmHipCtx* c) {
    for (PoseState* s = pose_states; s; s = s->next) if (s->ctx == c) return s;
    PoseState* s = (PoseState*)calloc(1, sizeof *s);
    s->ctx = c; s->next = pose_states; pose_states = s;
    return s;
}
static void pose_drop(AwsmHipCtx* c) {
    for (PoseState** p = &pose_states; *p; p = &(*p)->next)
        if ((*p)->ctx == c) { PoseState* s = *p; *p = s->next; free(s->records); free(s->ids); free(s); return; }
}
int awsm_hip_create(const AwsmConfig* cfg, AwsmHipCtx** out) { int rc = mock_base_create(cfg, out); if (!rc) pose_drop(*out); return rc; }
int awsm_hip_destroy(AwsmHipCtx* c) { pose_drop(c); return mock_base_destroy(c); }

int awsm_hip_skin_pose_records_write(AwsmHipCtx* c, uint32_t first, uint32_t n, const AwsmSkinPoseRecord* r) {
    PoseState* s = pose_of(c);
    if (first > s->count) return AWSM_ERR_OUT_OF_RANGE;
    if (first + n > s->cap) { s->cap = (first + n) * 2; s->records = (AwsmSkinPoseRecord*)realloc(s->records, s->cap * sizeof *r); }
    memcpy(s->records + first, r, n * sizeof *r);
    if (first + n > s->count) s->count = first + n;
    logc(c, 30, 0, first, n); return 0;
}
int awsm_hip_skin_pose(AwsmHipCtx* c, const uint32_t* ids, uint32_t n) {
    PoseState* s = pose_of(c);
    if (!c->buf[AWSM_BUF_TRANSFORMS] || !c->buf[AWSM_BUF_SKIN_MATRICES]) return AWSM_ERR_NOT_READY;
    for (uint32_t i = 0; i < n; i++) {
        if (ids[i] >= s->count) return AWSM_ERR_OUT_OF_RANGE;
        if (s->records[ids[i]].transform_offset + 64 > c->size[AWSM_BUF_TRANSFORMS] || s->records[ids[i]].matrix_offset + 64 > c->size[AWSM_BUF_SKIN_MATRICES]) return AWSM_ERR_OUT_OF_RANGE;
    }
    for (uint32_t i = 0; i < n; i++) {
        const AwsmSkinPoseRecord* r = &s->records[ids[i]];
        float w[16], out[16];
        memcpy(w, c->buf[AWSM_BUF_TRANSFORMS] + r->transform_offset, 64);
        for (int col = 0; col < 4; col++)
            for (int row = 0; row < 4; row++)
                out[col * 4 + row] = ((w[row] * r->inverse_bind[col * 4] + w[4 + row] * r->inverse_bind[col * 4 + 1]) + w[8 + row] * r->inverse_bind[col * 4 + 2]) + w[12 + row] * r->inverse_bind[col * 4 + 3];
        memcpy(c->buf[AWSM_BUF_SKIN_MATRICES] + r->matrix_offset, out, 64);
    }
    free(s->ids); s->ids = (uint32_t*)malloc((n ? n : 1) * 4); memcpy(s->ids, ids, n * 4); s->n_ids = n;
    logc(c, 31, 0, n, 0); return 0;
}
int awsm_hip_buffer_read(AwsmHipCtx* c, AwsmBuf w, size_t off, void* dst, size_t len) {
    if (!c->buf[w]) return AWSM_ERR_NOT_READY;
    if (off + len > c->size[w]) return AWSM_ERR_OUT_OF_RANGE;
    memcpy(dst, c->buf[w] + off, len); return 0;
}
uint32_t mock_pose_ids(AwsmHipCtx* c, uint32_t* out, uint32_t cap) { PoseState* s = pose_of(c); uint32_t n = s->n_ids < cap ? s->n_ids : cap; if (n) memcpy(out, s->ids, n * 4); return s->n_ids; }
uint32_t mock_pose_record_count(AwsmHipCtx* c) { return pose_of(c)->count; }
