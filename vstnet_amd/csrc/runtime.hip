// Host-side runtime shared by the launch code of every translation unit: the tuning options of vstnet.h, the HIP-event
// profiler behind vst_prof_scope, and the fp16 range flags collected from the translation units that raise them.
#include <mutex>
#include <stdlib.h>
#include "common.h"

// ---- tuning options (vstnet.h: VST_OPT_*), indexed by option id --------------------------------------------------------
// Initial value: the environment variable if it is "0" or "1", else the default.  An id without a variable is not an option.
static const struct { const char* env; int def; } kOptions[] = {
    {nullptr, 0},
    {"VST_LEAN", 0},         // VST_OPT_STAGE3_LEAN: the stage-3 convs of the bf16x3 mode as half-CU workgroups
    {nullptr, 0},            // VST_OPT_STAGE3_PINGPONG: reserved
    {"VST_WIDE", 1},         // VST_OPT_STAGE3_WIDE: those convs as one wave per SIMD on the 16 x 16 tile instead of two
    {"VST_FOLD16", 1},       // VST_OPT_STAGE1_FOLD: conv.1 of the 16-channel blocks in the tap-folded form, bf16x3
    {"VST_OUT_RGB", 1},      // VST_OPT_OUT_RGB: the last block of an inverse pass writes the image itself
};
constexpr int kNumOptions = sizeof(kOptions) / sizeof(kOptions[0]);
static std::atomic<int> g_options[kNumOptions];
static const bool g_options_ready = [] {
    for (int i = 0; i < kNumOptions; ++i) {
        const char* e = kOptions[i].env ? getenv(kOptions[i].env) : nullptr;
        g_options[i].store(e && (e[0] == '0' || e[0] == '1') ? e[0] - '0' : kOptions[i].def, std::memory_order_relaxed);
    }
    return true;
}();
static bool option_ok(int option) { return option > 0 && option < kNumOptions && kOptions[option].env; }

int vst_option(int option) { return g_options[option].load(std::memory_order_relaxed); }

// ---- optional per-kernel-class timing with HIP events (vst_profile_begin / vst_profile_end) ---------
// All of it is behind one lock: launch sites on any host thread may open records while a session is active.
#define VST_PROFILE_MAX_RECORDS 4096
static std::mutex g_prof_mu;
static std::atomic<int> g_prof_kernel{0};   // 0 = off, else VST_KERNEL_ID(cin, cout, stride)
static int g_prof_count = 0, g_prof_cap = 0;
static int g_prof_id[VST_PROFILE_MAX_RECORDS];
static hipEvent_t g_prof_ev[2 * VST_PROFILE_MAX_RECORDS];
static bool g_prof_ev_created = false;

int vst_prof_open(int kernel_id, hipStream_t st) {
    const int sel = g_prof_kernel.load(std::memory_order_relaxed);
    if (sel != kernel_id && sel != VST_KERNEL_ALL) return -1;                       // the common case: no lock taken
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if ((g_prof_kernel.load() != kernel_id && g_prof_kernel.load() != VST_KERNEL_ALL) || g_prof_count >= g_prof_cap) return -1;
    const int rec = g_prof_count++;
    g_prof_id[rec] = kernel_id;
    (void)hipEventRecord(g_prof_ev[2 * rec], st);
    return rec;
}

void vst_prof_close(int rec, hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (rec < g_prof_count) (void)hipEventRecord(g_prof_ev[2 * rec + 1], st);
}

extern "C" {

int vst_set_option(int option, int value) {
    if (!option_ok(option)) return VST_E_ARG;
    g_options[option].store(value != 0, std::memory_order_relaxed);
    return VST_OK;
}

int vst_get_option(int option) { return option_ok(option) ? vst_option(option) : VST_E_ARG; }

int vst_range_flags(unsigned* flags_host, int reset) {
    if (!flags_host) return VST_E_ARG;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    unsigned v = 0;
    if (int rc = vst_range_tu_conv(&v, reset)) return rc;
    if (int rc = vst_range_tu_conv3(&v, reset)) return rc;
    if (int rc = vst_range_tu_layout(&v, reset)) return rc;
    if (int rc = vst_range_tu_cwct(&v, reset)) return rc;
    *flags_host = v;
    return VST_OK;
}

int vst_range_flags_async(unsigned* flags4_dev, void* stream) {
    if (!flags4_dev) return VST_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = vst_range_tu_conv_async(flags4_dev + 0, st)) return rc;
    if (int rc = vst_range_tu_conv3_async(flags4_dev + 1, st)) return rc;
    if (int rc = vst_range_tu_layout_async(flags4_dev + 2, st)) return rc;
    return vst_range_tu_cwct_async(flags4_dev + 3, st);
}

int vst_profile_begin(int kernel_id, int max_records) {
    if ((kernel_id <= 0 && kernel_id != VST_KERNEL_ALL) || max_records <= 0) return VST_E_ARG;
    if (max_records > VST_PROFILE_MAX_RECORDS) max_records = VST_PROFILE_MAX_RECORDS;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (!g_prof_ev_created) {
        for (int i = 0; i < 2 * VST_PROFILE_MAX_RECORDS; ++i) {
            hipError_t e = hipEventCreate(&g_prof_ev[i]);
            if (e != hipSuccess) return (int)e;
        }
        g_prof_ev_created = true;
    }
    g_prof_count = 0; g_prof_cap = max_records;
    g_prof_kernel.store(kernel_id);
    return VST_OK;
}

int vst_profile_end(double* total_ms, int* launches) {
    if (!total_ms || !launches) return VST_E_ARG;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_kernel.store(0);
    double tot = 0.0;
    for (int i = 0; i < g_prof_count; ++i) {
        hipError_t e = hipEventSynchronize(g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        tot += ms;
    }
    *total_ms = tot; *launches = g_prof_count;
    g_prof_count = 0; g_prof_cap = 0;
    return VST_OK;
}

int vst_profile_end_table(int* ids, double* ms, int* launches, int cap, int* n_ids) {
    if (!ids || !ms || !launches || !n_ids || cap <= 0) return VST_E_ARG;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_kernel.store(0);
    int n = 0;
    for (int i = 0; i < g_prof_count; ++i) {
        hipError_t e = hipEventSynchronize(g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        float t = 0.f;
        e = hipEventElapsedTime(&t, g_prof_ev[2 * i], g_prof_ev[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        int k = 0;
        while (k < n && ids[k] != g_prof_id[i]) ++k;
        if (k == n) {
            if (n == cap) continue;
            ids[n] = g_prof_id[i]; ms[n] = 0.0; launches[n] = 0; ++n;
        }
        ms[k] += t; launches[k] += 1;
    }
    *n_ids = n;
    g_prof_count = 0; g_prof_cap = 0;
    return VST_OK;
}

}  // extern "C"
