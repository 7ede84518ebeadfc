// trace_hip.cpp — test infrastructure: a stand-in for the HIP runtime functions and for every launch wrapper of csrc/launch.hpp, linked with the
// host-only objects of csrc/awsm_hip.cpp and csrc/awsm_resources.cpp into a library that touches no GPU and writes down what the host layer enqueues.
//
//   memory     "device" and pinned memory are host memory, bump-allocated out of ONE region mapped at a fixed address: two runs that allocate in
//              the same order see the same pointer values.  hipMemcpy* / hipMemset* really copy and fill; hipFree keeps the memory.
//   streams    and events are small numbered handles; everything completes at once (hipEventQuery: see awsm_trace_event_query).
//   wrappers   append one line each: name, stream role (caller / shade<k> of slot k), scalar arguments, and the bytes of the argument struct as a
//              hash — verbose: as 32-bit words too, so that a difference names its offset.
//   hooks      awsm_trace_open / _begin / _arm / _event_query / _alloc / _close, for the driver (tests/trace/driver.py).
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "launch.hpp"

using namespace awsm;

namespace {

constexpr uintptr_t kRegionBase = 0x7e0000000000ull;
constexpr size_t kRegionBytes = 16ull << 30;      // address space only (MAP_NORESERVE): pages exist once written
uint8_t* g_region = nullptr;
size_t g_top = 0, g_high = 0;
FILE* g_out = nullptr;
bool g_verbose = false;
int g_streams = 0, g_events = 0;
int g_arm_skip[2] = {-1, -1};                     // [0] bin_scan, [1] forward: calls to let pass before the flag is raised (-1: not armed)
uint32_t g_arm_need[2] = {0, 0};
int g_query_ready = 1;

// FrameDev::counters (frame_params.hpp)
enum { kBinned = 0, kEntries = 1, kOverflow = 2, kFragments = 5, kFragOverflow = 6 };

void map_region() {
    if (g_region) return;
    void* p = mmap((void*)kRegionBase, kRegionBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE | MAP_FIXED_NOREPLACE, -1, 0);
    if (p != (void*)kRegionBase) { fprintf(stderr, "trace_hip: cannot map %zu bytes at %#" PRIxPTR "\n", kRegionBytes, kRegionBase); abort(); }
    g_region = (uint8_t*)p;
}
void* bump(size_t bytes) {
    map_region();
    const size_t at = (g_top + 4095) & ~size_t(4095);
    if (at + bytes > kRegionBytes) return nullptr;
    g_top = at + bytes;
    if (g_top > g_high) g_high = g_top;
    return g_region + at;
}
void out(const char* fmt, ...) {
    if (!g_out) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(g_out, fmt, ap);
    va_end(ap);
}
// a pointer as the trace names it: its offset in the region, "host" for anything else (the caller's arrays, whose addresses differ from run to run)
std::string P(const void* p) {
    if (!p) return "null";
    const uintptr_t v = (uintptr_t)p;
    if (v < kRegionBase || v >= kRegionBase + kRegionBytes) return "host";
    char b[32];
    snprintf(b, sizeof b, "d+%#zx", (size_t)(v - kRegionBase));
    return b;
}
std::string S(hipStream_t s) {
    const uintptr_t v = (uintptr_t)s;
    if (v == 0) return "null";
    if (v == 1) return "caller";
    return "shade" + std::to_string(v - 2);
}
std::string E(hipEvent_t e) { return "ev" + std::to_string((uintptr_t)e); }
// the argument struct's bytes: FNV-1a 64, and the words behind it when asked
template <class T> std::string A(const T* a) {
    if (!a) return " args=null";
    const uint8_t* b = (const uint8_t*)a;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < sizeof(T); i++) { h ^= b[i]; h *= 1099511628211ull; }
    char buf[48];
    snprintf(buf, sizeof buf, " args=%016" PRIx64, h);
    std::string s = buf;
    if (g_verbose) {
        s += " words=";
        for (size_t i = 0; i + 4 <= sizeof(T); i += 4) { uint32_t w; memcpy(&w, b + i, 4); snprintf(buf, sizeof buf, "%s%x", i ? "," : "", w); s += buf; }
    }
    return s;
}
void L(const char* name, hipStream_t s, const std::string& rest) { out("L awsm_launch_%s %s%s\n", name, S(s).c_str(), rest.c_str()); }
std::string F(const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}
bool fire(int which) {
    if (g_arm_skip[which] < 0) return false;
    if (g_arm_skip[which]-- > 0) return false;
    return true;      // (now -1: once)
}

}  // namespace

extern "C" {

// ---- hooks for the driver ----
int awsm_trace_open(const char* path, int verbose) {
    if (g_out) fclose(g_out);
    g_out = fopen(path, "w");
    g_verbose = verbose != 0;
    return g_out ? 0 : -1;
}
void awsm_trace_close(void) { if (g_out) fclose(g_out); g_out = nullptr; }
// a new scenario (no context alive): handles count from one again, the region is handed out from its start again, zero-filled
void awsm_trace_begin(const char* name) {
    map_region();
    if (g_high) memset(g_region, 0, g_high);
    g_top = g_high = 0;
    g_streams = g_events = 0;
    g_arm_skip[0] = g_arm_skip[1] = -1;
    g_query_ready = 1;
    out("== %s\n", name);
}
// which: 0 = the bin_scan stand-in, 1 = the forward stand-in.  After `skip` more calls of it, the next one raises the overflow flag of its pass and
// reports `needed` entries (fragments) — once.
void awsm_trace_arm(int which, int skip, uint32_t needed) { g_arm_skip[which & 1] = skip; g_arm_need[which & 1] = needed; }
void awsm_trace_event_query(int ready) { g_query_ready = ready; }      // 0: hipEventQuery answers hipErrorNotReady
void* awsm_trace_alloc(size_t bytes) { return bump(bytes); }           // "device" memory for the driver's own bound images
void awsm_trace_note(const char* text) { out("-- %s\n", text); }

// ---- the runtime ----
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
    memset(p, 0, sizeof *p);
    snprintf(p->name, sizeof p->name, "launch trace");
    snprintf(p->gcnArchName, sizeof p->gcnArchName, "gfx950:trace");
    p->multiProcessorCount = 256;
    p->totalGlobalMem = kRegionBytes;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) { *v = 100000; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "launch trace"; }

hipError_t hipMalloc(void** p, size_t bytes) {
    *p = bump(bytes);
    out("H hipMalloc bytes=%zu -> %s\n", bytes, P(*p).c_str());
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) { out("H hipFree %s\n", P(p).c_str()); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
    *p = bump(bytes);
    out("H hipHostMalloc bytes=%zu -> %s\n", bytes, P(*p).c_str());
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { out("H hipHostFree %s\n", P(p).c_str()); return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    memmove(dst, src, n);
    out("H hipMemcpy dst=%s src=%s bytes=%zu kind=%d\n", P(dst).c_str(), P(src).c_str(), n, (int)kind);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
    memmove(dst, src, n);
    out("H hipMemcpyAsync %s dst=%s src=%s bytes=%zu kind=%d\n", S(s).c_str(), P(dst).c_str(), P(src).c_str(), n, (int)kind);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t n) { memset(dst, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t s) {
    memset(dst, v, n);
    out("H hipMemsetAsync %s dst=%s value=%d bytes=%zu\n", S(s).c_str(), P(dst).c_str(), v, n);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) { *s = (hipStream_t)(uintptr_t)(++g_streams); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) { out("H hipStreamWaitEvent %s %s\n", S(s).c_str(), E(e).c_str()); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)(uintptr_t)(++g_events); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { out("H hipEventRecord %s %s\n", E(e).c_str(), S(s).c_str()); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { out("H hipEventQuery %s\n", E(e).c_str()); return g_query_ready ? hipSuccess : hipErrorNotReady; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }

// ---- the launch wrappers (csrc/launch.hpp) ----
void awsm_launch_upload_words(void* dst, const void* src_pinned, uint32_t n_words, hipStream_t s) {
    memcpy(dst, src_pinned, (size_t)n_words * 4);      // what the kernel does: the scene table, the draw lists and the camera arrive
    L("upload_words", s, F(" dst=%s src=%s words=%u", P(dst).c_str(), P(src_pinned).c_str(), n_words));
}
void awsm_launch_handoff_signal(uint32_t* flag, uint32_t serial, unsigned long long* stamp, hipStream_t s) {
    L("handoff_signal", s, F(" flag=%s serial=%u stamp=%s", P(flag).c_str(), serial, P(stamp).c_str()));
}
void awsm_launch_handoff_wait(const uint32_t* flag, uint32_t serial, unsigned long long budget_ticks, uint32_t* timeouts_host, uint32_t timeouts_known, uint32_t* poison,
                              uint32_t poison_serial, hipStream_t s) {
    L("handoff_wait", s, F(" flag=%s serial=%u budget=%llu timeouts=%s known=%u poison=%s poison_serial=%u", P(flag).c_str(), serial, budget_ticks, P(timeouts_host).c_str(),
                           timeouts_known, P(poison).c_str(), poison_serial));
}
void awsm_launch_hud_merge(const unsigned long long* world, const unsigned long long* hud, unsigned long long* o, size_t first, size_t n, hipStream_t s) {
    L("hud_merge", s, F(" world=%s hud=%s out=%s first=%zu n=%zu", P(world).c_str(), P(hud).c_str(), P(o).c_str(), first, n));
}
// k_deform_transform clears the pass's counters (awsm_hip.cpp: the passes without triangles do it with memsets instead)
void awsm_launch_transform(const DevScene* sc, const FrameDev* f, uint32_t n_blocks, hipStream_t s) {
    if (f->counters) memset(f->counters, 0, 8 * sizeof(uint32_t));
    L("transform", s, F(" scene=%s blocks=%u", P(sc).c_str(), n_blocks) + A(f));
}
void awsm_launch_transform_forward(const DevScene* sc, const FrameDev* f, uint32_t n_blocks, hipStream_t s) {
    if (f->counters) memset(f->counters, 0, 8 * sizeof(uint32_t));
    L("transform_forward", s, F(" scene=%s blocks=%u", P(sc).c_str(), n_blocks) + A(f));
}
void awsm_launch_bin_count(const FrameDev* f, hipStream_t s) { L("bin_count", s, A(f)); }
void awsm_launch_bin_big(const FrameDev* f, int fill, hipStream_t s) { L("bin_big", s, F(" fill=%d", fill) + A(f)); }
void awsm_launch_bin_scan(const FrameDev* f, hipStream_t s) {
    std::string note;
    if (f->counters && fire(0)) { f->counters[kOverflow] = 1u; f->counters[kEntries] = g_arm_need[0]; note = F(" raises-overflow=%u", g_arm_need[0]); }
    L("bin_scan", s, note + A(f));
}
void awsm_launch_bin_fill(const FrameDev* f, hipStream_t s) { L("bin_fill", s, A(f)); }
void awsm_launch_raster(const FrameDev* f, hipStream_t s) { L("raster", s, A(f)); }
void awsm_launch_resolve_draws(const DevScene* sc, const FrameDev* f, hipStream_t s) { L("resolve_draws", s, F(" scene=%s", P(sc).c_str()) + A(f)); }
void awsm_launch_shade(const DevScene* sc, const FrameDev* f, hipStream_t s) { L("shade", s, F(" scene=%s", P(sc).c_str()) + A(f)); }
int awsm_shade_is_lean(const FrameDev* f) { return f->tri_shade != nullptr; }
int awsm_launch_shade_todo(const DevScene* sc, const FrameDev* f, hipStream_t s) { L("shade_todo", s, F(" scene=%s", P(sc).c_str()) + A(f)); return 1; }
void awsm_launch_forward(const DevScene* sc, const FrameDev* f, const EditorGridDev* grid, hipStream_t s) {
    std::string note;
    if (f->counters && fire(1)) { f->counters[kFragOverflow] = 1u; f->counters[kFragments] = g_arm_need[1]; note = F(" raises-overflow=%u", g_arm_need[1]); }
    L("forward", s, F(" scene=%s", P(sc).c_str()) + note + A(f) + (grid ? " grid:" + A(grid) : std::string(" grid: null")));
}
void awsm_launch_editor_grid_layer(const EditorGridDev* g, uint32_t width, uint32_t height, float* rgba, float* depth, uint8_t* kept, hipStream_t s) {
    L("editor_grid_layer", s, F(" %ux%u rgba=%s depth=%s kept=%s", width, height, P(rgba).c_str(), P(depth).c_str(), P(kept).c_str()) + A(g));
}
void awsm_launch_msaa_halo_export(const FrameDev* f, unsigned long long* dst, uint32_t bands_out, hipStream_t s) {
    L("msaa_halo_export", s, F(" dst=%s bands=%u", P(dst).c_str(), bands_out) + A(f));
}
void awsm_launch_count_covered(const FrameDev* f, hipStream_t s) { L("count_covered", s, A(f)); }
void awsm_launch_gbuffer_dump(const FrameDev* f, float* o, hipStream_t s) { L("gbuffer_dump", s, F(" out=%s", P(o).c_str()) + A(f)); }
void awsm_launch_vis_digest(const unsigned long long* vis, size_t n, unsigned long long* o, hipStream_t s) { L("vis_digest", s, F(" vis=%s n=%zu out=%s", P(vis).c_str(), n, P(o).c_str())); }
void awsm_launch_pick(const DevScene* sc, const FrameDev* f, int x, int y, uint32_t* o, hipStream_t s) {
    L("pick", s, F(" scene=%s x=%d y=%d out=%s", P(sc).c_str(), x, y, P(o).c_str()) + A(f));
}
void awsm_launch_cube_border(const CubeDev* cd, uint2* o, uint32_t total, hipStream_t s) { L("cube_border", s, F(" out=%s total=%u", P(o).c_str(), total) + A(cd)); }
void awsm_launch_brdf_lut(uint32_t* o, uint32_t w, uint32_t h, hipStream_t s) { L("brdf_lut", s, F(" out=%s %ux%u", P(o).c_str(), w, h)); }
void awsm_launch_rgba16f_to_rg16f(const uint16_t* in, uint32_t* o, uint32_t n, hipStream_t s) { L("rgba16f_to_rg16f", s, F(" in=%s out=%s n=%u", P(in).c_str(), P(o).c_str(), n)); }
void awsm_launch_post(const PostArgs* args, uint32_t flags, uint32_t msaa, void* bloom_a, void* bloom_b, hipStream_t s) {
    L("post", s, F(" flags=%u msaa=%u bloom_a=%s bloom_b=%s", flags, msaa, P(bloom_a).c_str(), P(bloom_b).c_str()) + A(args));
}
void awsm_launch_ssao(const SsaoArgs* args, uint32_t msaa, hipStream_t s) { L("ssao", s, F(" msaa=%u", msaa) + A(args)); }
void awsm_launch_shadow_resolve(const ShadowArgs* args, uint32_t msaa, hipStream_t s) { L("shadow_resolve", s, F(" msaa=%u", msaa) + A(args)); }
void awsm_launch_selection(const SelectionDev* args, hipStream_t s) { L("selection", s, A(args)); }
void awsm_launch_selection_layers(const SelectionDev* args, hipStream_t s) { L("selection_layers", s, A(args)); }
void awsm_launch_taa(const TaaArgs* args, uint32_t msaa, hipStream_t s) { L("taa", s, F(" msaa=%u", msaa) + A(args)); }
void awsm_launch_taa_layers(const TaaArgs* args, uint32_t msaa, hipStream_t s) { L("taa_layers", s, F(" msaa=%u", msaa) + A(args)); }
void awsm_launch_env_write(const EnvWriteArgs* a, hipStream_t s) { L("env_write", s, A(a)); }
void awsm_launch_env_expand_rows(const uint32_t* rows, const uint16_t* tables, uint2* dst, uint32_t n, hipStream_t s) {
    L("env_expand_rows", s, F(" rows=%s tables=%s dst=%s n=%u", P(rows).c_str(), P(tables).c_str(), P(dst).c_str(), n));
}
void awsm_launch_env_mips(const EnvMipArgs* a, hipStream_t s) { L("env_mips", s, A(a)); }
void awsm_launch_env_filter(const EnvFilterArgs* a, uint32_t blocks, hipStream_t s) { L("env_filter", s, F(" blocks=%u", blocks) + A(a)); }
void awsm_launch_env_filter_level0(const EnvFilterLevel0Args* a, hipStream_t s) { L("env_filter_level0", s, A(a)); }
void awsm_launch_env_from_equirect(const EnvEquirectArgs* a, hipStream_t s) { L("env_from_equirect", s, A(a)); }
void awsm_launch_tex_write(const TexWriteArgs* a, hipStream_t s) { L("tex_write", s, A(a)); }
void awsm_launch_tex_mips(const TexMipArgs* a, hipStream_t s) { L("tex_mips", s, A(a)); }
void awsm_launch_gen_mip_level(uint8_t* chain, uint32_t src_off, uint32_t dst_off, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh, uint32_t layers, const uint32_t* kinds, hipStream_t s) {
    L("gen_mip_level", s, F(" chain=%s src=%u dst=%u %ux%u -> %ux%u layers=%u kinds=%s", P(chain).c_str(), src_off, dst_off, sw, sh, dw, dh, layers, P(kinds).c_str()));
}
void awsm_launch_skin_pose(const void* records, const uint32_t* ids_pinned, uint32_t n, const void* transforms, void* skin_matrices, hipStream_t s) {
    L("skin_pose", s, F(" records=%s ids=%s n=%u transforms=%s matrices=%s", P(records).c_str(), P(ids_pinned).c_str(), n, P(transforms).c_str(), P(skin_matrices).c_str()));
}

}  // extern "C"
