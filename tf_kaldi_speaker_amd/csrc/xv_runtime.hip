// Process-wide plumbing of the library: the per-thread error string behind xv_last_error, the XV_* environment switches (xv_env),
// the ABI version / device count queries, live launch timing (xv_profile_*) and the two plain copies of the C-ABI (xv_copy_2d, xv_pad_channels).  gfx950 only.
#include <stdarg.h>

#include <vector>

#include "xv_common.h"
#include "xv_ew.h"
#include "xv_gemm.h"      // XvProfScope

// ------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void xv_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
// ---- environment switches (xv_common.h XvEnv) -----------------------------------------------------------------------------------
extern char** environ;
namespace {
struct XvEnvState { XvEnv env; bool bad; char why[256]; };
// Read once, on first use; a C++11 function-local static is initialised under a lock, so concurrent first calls (loader threads, two
// engines created from two host threads) see one parse.
XvEnvState xv_env_parse() {
    XvEnvState st;
    st.bad = false;
    st.why[0] = 0;
    XvEnv& env = st.env;
    // every XV_* name this package reads anywhere (native library, Python host, tools/, tests/).  Any other XV_* variable is reported ONCE on
    // stderr and otherwise ignored: it may be a typo or a switch of an earlier round (worth a line), but it may equally belong to another
    // program in the user's environment, which must not stop a training run.  A known switch with a value it does not understand still fails.
    static const char* known[] = {"XV_SEGMENT_FUSED", "XV_NT_SCHED", "XV_CONV_WR", "XV_PRECISION", "XV_LOADER", "XV_LOADER_PIN", "XV_SHARE_GPU",
                                  "XV_LIB", "XV_TUNE_TIMES", "XV_DATA_SCALE", "XV_B", "XV_PROBE_OPS", "XV_PROBE_ONLY", "XV_PROBE_PERIODS",
                                  "XV_DIAG_M", "XV_DIAG_N", "XV_DIAG_K", "XV_DIAG_REPS", "XV_DIAG_B", "XV_PROBE_EXTRA", "XV_DZ_SLOTS"};
    for (char** e = environ; e && *e; ++e) {
        if (strncmp(*e, "XV_", 3) != 0) continue;
        const char* eq = strchr(*e, '=');
        const size_t len = eq ? (size_t)(eq - *e) : strlen(*e);
        bool ok = false;
        for (const char* k : known) ok = ok || (strlen(k) == len && strncmp(k, *e, len) == 0);
        if (!ok) fprintf(stderr, "libxvector_hip: ignoring unknown environment switch %.*s (INTEGRATION.md section 6 lists the supported ones)\n", (int)len, *e);
    }
    auto fail = [&](const char* fmt, const char* name, const char* v) {
        if (!st.bad) { snprintf(st.why, sizeof st.why, fmt, name, v); st.bad = true; }
    };
    auto flag = [&](const char* name, int dflt, int* out) {
        const char* v = getenv(name);
        *out = dflt;
        if (!v || !*v) return;
        if (!strcmp(v, "0") || !strcmp(v, "1")) *out = v[0] - '0';
        else fail("%s=%s: expected 0 or 1", name, v);
    };
    flag("XV_SEGMENT_FUSED", 1, &env.segment_fused);
    env.nt_sched = 0;
    if (const char* v = getenv("XV_NT_SCHED")) {
        if (!strcmp(v, "dp")) env.nt_sched = 1;
        else if (!strcmp(v, "sk")) env.nt_sched = 2;
        else if (*v) fail("%s=%s: expected dp or sk", "XV_NT_SCHED", v);
    }
    env.dz_slots = 0;
    if (const char* v = getenv("XV_DZ_SLOTS")) {
        if (!strcmp(v, "2")) env.dz_slots = 2;
        else if (*v) fail("%s=%s: expected 2", "XV_DZ_SLOTS", v);
    }
    env.conv_wr = 0;
    if (const char* v = getenv("XV_CONV_WR")) {
        if (!strcmp(v, "4")) env.conv_wr = 4;
        else if (*v && strcmp(v, "2")) fail("%s=%s: expected 2 or 4", "XV_CONV_WR", v);
    }
    return st;
}
}  // namespace

const XvEnv* xv_env() {
    static const XvEnvState st = xv_env_parse();
    if (st.bad) { xv_set_error("%s", st.why); return nullptr; }
    return &st.env;
}

extern "C" const char* xv_last_error(void) { return g_err; }
extern "C" int xv_abi_version(void) { return XV_ABI_VERSION; }
extern "C" int xv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int xv_copy_2d(void* stream, float* dst, size_t ldd, const float* src, size_t lds, int rows, int cols) {
    XV_REQUIRE(dst && src && rows > 0 && cols > 0 && ldd >= (size_t)cols && lds >= (size_t)cols, "copy_2d: bad arguments");
    XV_CHECK_HIP(hipMemcpy2DAsync(dst, ldd * sizeof(float), src, lds * sizeof(float), (size_t)cols * sizeof(float), rows,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------------------------
// live launch timing of the GEMM launchers (XvProfScope, xv_gemm.h; bench.py roofline leg)
// ------------------------------------------------------------------------------------
namespace {
struct ProfRec { hipEvent_t a, b; int kind; double flops; };
bool g_prof_on = false;
uint32_t g_prof_mask = ~0u;
std::vector<ProfRec> g_prof;
size_t g_prof_cap = 0;
std::vector<hipEvent_t> g_prof_events;   // pool, two per record slot
}  // namespace

XvProfScope::XvProfScope(hipStream_t st, int kind, double flops) : s(st), idx(-1) {
    if (!g_prof_on || !((g_prof_mask >> kind) & 1u) || g_prof.size() >= g_prof_cap) return;
    idx = (int)g_prof.size();
    ProfRec r = {g_prof_events[2 * idx], g_prof_events[2 * idx + 1], kind, flops};
    g_prof.push_back(r);
    (void)hipEventRecord(r.a, s);
}
XvProfScope::~XvProfScope() { if (idx >= 0) (void)hipEventRecord(g_prof[idx].b, s); }

extern "C" int xv_profile_begin(int max_launches) { return xv_profile_begin_kinds(max_launches, ~0u); }

extern "C" int xv_profile_begin_kinds(int max_launches, uint32_t kind_mask) {
    XV_REQUIRE(max_launches > 0, "profile_begin: max_launches must be positive");
    g_prof_mask = kind_mask;
    while (g_prof_events.size() < (size_t)2 * max_launches) {
        hipEvent_t ev;
        // device-scope release: the pair brackets one launch on its own stream; a system-scope fence per record (the default) would be
        // measurement overhead inside the region bench.py times
        XV_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventReleaseToDevice));
        g_prof_events.push_back(ev);
    }
    g_prof.clear();
    g_prof_cap = (size_t)max_launches;
    g_prof_on = true;
    return 0;
}

extern "C" int xv_profile_end(int64_t launches[XV_PROFILE_KINDS], double ms[XV_PROFILE_KINDS], double flops[XV_PROFILE_KINDS]) {
    g_prof_on = false;
    for (int k = 0; k < XV_PROFILE_KINDS; ++k) { launches[k] = 0; ms[k] = 0.0; flops[k] = 0.0; }
    for (auto& r : g_prof) {
        XV_CHECK_HIP(hipEventSynchronize(r.b));
        float t = 0.f;
        XV_CHECK_HIP(hipEventElapsedTime(&t, r.a, r.b));
        launches[r.kind] += 1; ms[r.kind] += (double)t; flops[r.kind] += r.flops;
    }
    g_prof.clear();
    return 0;
}

// ------------------------------------------------------------------------------------
// layout prep
// ------------------------------------------------------------------------------------
__global__ void pad_channels_kernel(const float* __restrict__ src, long rows, int c_src, float* __restrict__ dst, int c_dst) {
    XV_EW_FILLER();
    long total = rows * c_dst;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long r = i / c_dst;
        int c = (int)(i - r * c_dst);
        dst[i] = c < c_src ? src[r * c_src + c] : 0.f;
    }
}

extern "C" int xv_pad_channels(void* stream, const float* src, int rows, int c_src, float* dst, int c_dst) {
    XV_REQUIRE(rows > 0 && c_src > 0 && c_dst >= c_src, "pad_channels: bad shape rows=%d c_src=%d c_dst=%d", rows, c_src, c_dst);
    long total = (long)rows * c_dst;
    hipLaunchKernelGGL(pad_channels_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, src, (long)rows, c_src, dst, c_dst);
    XV_LAUNCH_CHECK();
    return 0;
}
