// What every launcher of libbrepgen_hip.so shares and no kernel file owns: the thread-local error message behind bg_last_error,
// launch_status, the bg_tune table, the opt-in per-launch hipEvent profiler, and the ABI / launch-partition queries.  No kernel here.
#include "bg_common.h"
#include <stdarg.h>
#include <stdio.h>

namespace bg {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
}

int g_tune[BG_TUNE_ATTN_WALK + 1] = {0};
template <int N> constexpr bool all_below(const int (&keys)[N], int bound) {
    for (int i = 0; i < N; ++i)
        if (keys[i] < 0 || keys[i] >= bound) return false;
    return true;
}

// ---- per-kernel event timing ------------------------------------------------------------------------------
bool g_prof_on = false;
namespace {
struct ProfRec { hipEvent_t e0, e1; int kernel; double flops, bytes; };
ProfRec* g_recs = nullptr;
int g_cap = 0, g_n = 0;
bool g_open = false;
const char* const kProfNames[PK_COUNT] = {"gemm16_persistent_kernel(128x128)", "gemm16_kernel(generic: 128x64 / 64x64 tiles)", "gemm_f32", "attn16_kernel", "attn_f32_kernel",
                                          "ln768_kernel", "ddpm_step_kernel", "pndm_step_kernel", "misc", "embed_ln_silu_kernel", "gemm16_p256_kernel(256x256)",
                                          "gemm16_split_pipe_kernel(128x128)", "gemm16_p256_kernel(256x256, split-residual launches)",
                                          "qkv_attn_kernel(256x192 + attention)", "ln_silu_out_kernel", "ffn_fused_kernel(64-row panels)"};
}  // namespace

void prof_pre(hipStream_t s) {
    g_open = false;
    if (g_n >= g_cap) return;
    if (hipEventRecord(g_recs[g_n].e0, s) == hipSuccess) g_open = true;
}

void prof_post(int kernel, double flops, double bytes, hipStream_t s) {
    if (!g_open) return;
    g_open = false;
    ProfRec& r = g_recs[g_n];
    if (hipEventRecord(r.e1, s) != hipSuccess) return;
    r.kernel = kernel; r.flops = flops; r.bytes = bytes;
    ++g_n;
}

}  // namespace bg

extern "C" int bg_profile_begin(int max_launches) {
    using namespace bg;
    BG_REQUIRE(max_launches > 0 && max_launches <= (1 << 20), BG_E_ARG, "bg_profile_begin: bad max_launches");
    BG_REQUIRE(g_recs == nullptr, BG_E_ARG, "bg_profile_begin: already profiling");
    g_recs = new ProfRec[max_launches];
    for (int i = 0; i < max_launches; ++i) {
        if (hipEventCreate(&g_recs[i].e0) != hipSuccess || hipEventCreate(&g_recs[i].e1) != hipSuccess) {
            set_error("bg_profile_begin: hipEventCreate failed");
            return BG_E_ARG;
        }
    }
    g_cap = max_launches; g_n = 0; g_prof_on = true;
    return 0;
}

extern "C" int bg_profile_end(bg_profile_row* rows, int max_rows) {
    using namespace bg;
    BG_REQUIRE(g_recs != nullptr, BG_E_ARG, "bg_profile_end: not profiling");
    g_prof_on = false;
    (void)hipDeviceSynchronize();            // measurement aid only -- never on the product path
    bg_profile_row agg[PK_COUNT];
    for (int k = 0; k < PK_COUNT; ++k) agg[k] = bg_profile_row{kProfNames[k], 0, 0.0, 0.0, 0.0};
    for (int i = 0; i < g_n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, g_recs[i].e0, g_recs[i].e1) != hipSuccess) continue;
        bg_profile_row& a = agg[g_recs[i].kernel];
        a.launches += 1; a.total_ms += ms; a.flops += g_recs[i].flops; a.bytes += g_recs[i].bytes;
    }
    for (int i = 0; i < g_cap; ++i) { (void)hipEventDestroy(g_recs[i].e0); (void)hipEventDestroy(g_recs[i].e1); }
    delete[] g_recs;
    g_recs = nullptr; g_cap = 0; g_n = 0;
    int n = 0;
    for (int k = 0; k < PK_COUNT && n < max_rows; ++k)
        if (agg[k].launches > 0 && rows) rows[n++] = agg[k];
    return n;
}

extern "C" int bg_tune_set(int key, int value) {
    // the enumerators of bg_tune_key, and nothing between or beyond them (a new key: the enum, this list; the table's size is checked)
    static constexpr int keys[] = {BG_TUNE_GEMM_STAGGER, BG_TUNE_P256_MODE, BG_TUNE_SPLIT_PIPE, BG_TUNE_QKV_ATTN, BG_TUNE_QKV_WALK,
                                   BG_TUNE_SMALL_TILES, BG_TUNE_FFN_FUSED, BG_TUNE_VAE_GN1_FUSED, BG_TUNE_ATTN_WALK};
    static_assert(bg::all_below(keys, (int)(sizeof(bg::g_tune) / sizeof(bg::g_tune[0]))), "a bg_tune_key past the end of g_tune");
    for (const int k : keys)
        if (k == key) {
            bg::g_tune[key] = value;
            return 0;
        }
    bg::set_error("bg_tune_set: unknown key %d", key);
    return BG_E_ARG;
}

extern "C" int bg_gemm_p256_rows(int rows, int n_cols, int split_residual, int concurrent) {
    BG_REQUIRE(rows >= 0 && n_cols > 0 && (n_cols & 255) == 0, BG_E_ARG, "bg_gemm_p256_rows: rows >= 0 and n_cols a positive multiple of 256 expected");
    return bg::p256_rows(rows, n_cols >> 8, split_residual != 0, concurrent != 0);
}

extern "C" int bg_abi_version(void) { return BG_ABI_VERSION; }
extern "C" const char* bg_last_error(void) { return bg::g_err; }
