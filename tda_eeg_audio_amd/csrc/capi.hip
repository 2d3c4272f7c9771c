// capi.hip -- the C ABI of libtdaeeg.so (include/tdaeeg.h): context, argument checks,
// host-pointer twins (stage -> launch -> copy back) and timing helpers.
#include "common.h"
#include <string.h>
#include <cmath>
#include <vector>

static thread_local std::string g_create_err;

#pragma GCC visibility push(default)
extern "C" {

int tda_version(void) { return 100; }

tda_status tda_ctx_create(int device_id, tda_ctx** out)
{
    if (!out) return TDA_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("no HIP device: ") + hipGetErrorString(e);
        return TDA_ERR_HIP;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_err = "device_id out of range"; return TDA_ERR_INVALID; }
    e = hipSetDevice(device_id);
    if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return TDA_ERR_HIP; }
    tda_ctx* c = new (std::nothrow) tda_ctx();
    if (!c) return TDA_ERR_NOMEM;
    c->device = device_id;
    // scratch of the last rung of the Rips ladders, allocated here so that every entry point stays enqueue-only
    e = hipMalloc((void**)&c->total_scratch, rips_total_scratch_bytes());
    if (e != hipSuccess) { g_create_err = std::string("hipMalloc (Rips scratch): ") + hipGetErrorString(e); delete c; return TDA_ERR_HIP; }
    if (retry_lists_reserve(c, 1 << 19) != TDA_OK) { g_create_err = "hipMalloc (retry lists): " + c->err; tda_ctx_destroy(c); return TDA_ERR_HIP; }
    *out = c;
    return TDA_OK;
}

void tda_ctx_destroy(tda_ctx* ctx)
{
    if (!ctx) return;
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->total_scratch) (void)hipFree(ctx->total_scratch);
    for (int i = 0; i < TDA_RETRY_SLOTS; ++i) if (ctx->retry_buf[i]) (void)hipFree(ctx->retry_buf[i]);
    for (void* q : ctx->retired) (void)hipFree(q);
    delete ctx;
}

size_t tda_last_error(const tda_ctx* ctx, char* buf, size_t cap)
{
    const std::string& s = ctx ? ctx->err : g_create_err;
    if (buf && cap) {
        size_t n = s.size() < cap - 1 ? s.size() : cap - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size();
}

tda_status tda_set_class_words(tda_ctx* ctx, int words_dm, int words_cloud)
{
    if (!ctx) return TDA_ERR_INVALID;
    if ((words_dm != 0 && words_dm != 1 && words_dm != 2 && words_dm != 4) || (words_cloud != 1 && words_cloud != 2))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "class words: dm in {0,1,2,4}, cloud in {1,2}");
    ctx->words_dm = words_dm;
    ctx->words_cloud = words_cloud;
    return TDA_OK;
}

tda_status tda_set_h1_order(tda_ctx* ctx, int policy)
{
    if (!ctx) return TDA_ERR_INVALID;
    if (policy != TDA_ORDER_IN_CALL && policy != TDA_ORDER_DEFERRED) TDA_FAIL(ctx, TDA_ERR_INVALID, "unknown order policy");
    ctx->h1_order = policy;
    return TDA_OK;
}

tda_status tda_set_launch_scheme(tda_ctx* ctx, int scheme)
{
    if (!ctx) return TDA_ERR_INVALID;
    if (scheme != TDA_SCHEME_LISTS && scheme != TDA_SCHEME_GRID && scheme != TDA_SCHEME_ONE)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "unknown launch scheme");
    ctx->launch_scheme = scheme;
    return TDA_OK;
}

tda_status tda_set_wasserstein_pruning(tda_ctx* ctx, int on)
{
    if (!ctx) return TDA_ERR_INVALID;
    ctx->ws_prune = on ? 1 : 0;
    return TDA_OK;
}

tda_status tda_set_wasserstein_counter(tda_ctx* ctx, unsigned long long* dev_counters)
{
    if (!ctx) return TDA_ERR_INVALID;
    ctx->ws_ctr = dev_counters;
    return TDA_OK;
}

tda_status tda_diagram_finish_dev(tda_ctx* ctx, const tda_diagram_set* sets, int n_sets, int n_dgm, void* stream)
{
    if (!ctx) return TDA_ERR_INVALID;
    if (n_dgm < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative count");
    if (n_sets && !sets) TDA_FAIL(ctx, TDA_ERR_INVALID, "null pointer");
    return launch_diagram_finish(ctx, sets, n_sets, n_dgm, (hipStream_t)stream);
}

tda_status tda_set_retry_counter(tda_ctx* ctx, void* dev_counters)
{
    if (!ctx) return TDA_ERR_INVALID;
    ctx->retry_ctr = (unsigned long long*)dev_counters;
    return TDA_OK;
}

tda_status tda_set_retry_policy(tda_ctx* ctx, int policy)
{
    if (!ctx) return TDA_ERR_INVALID;
    if (policy < TDA_RETRY_AUTO || policy > TDA_RETRY_LAST_RUNG) TDA_FAIL(ctx, TDA_ERR_INVALID, "unknown retry policy");
    ctx->retry_policy = policy;
    return TDA_OK;
}

#define CHECK_CTX(ctx) do { if (!(ctx)) return TDA_ERR_INVALID; } while (0)
#define CHECK_PTR(ctx, p) do { if (!(p)) TDA_FAIL(ctx, TDA_ERR_INVALID, "null pointer: " #p); } while (0)
#define CHECK_NONNEG(ctx, v) do { if ((v) < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative size: " #v); } while (0)

// ---------------------------------------------------------------- device-pointer API
tda_status tda_corr_dist_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t, double* dist,
                                   double* corr, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, dist); }
    return launch_corr_dist(ctx, win, n_win, n_ch, n_t, dist, corr, (hipStream_t)stream);
}

tda_status tda_corr_dist_sliding_dev(tda_ctx* ctx, const double* sig, int n_ch, int n_samples, int win_len, int step,
                                     double* dist, double* corr, int* n_win, void* stream)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, sig);
    CHECK_NONNEG(ctx, n_samples);
    if (n_samples >= win_len) CHECK_PTR(ctx, dist);     // (a recording shorter than the window has no matrix to write)
    return launch_corr_dist_sliding(ctx, sig, n_ch, n_samples, win_len, step, dist, corr, n_win, (hipStream_t)stream);
}

tda_status tda_corr_to_dist_batch_dev(tda_ctx* ctx, const double* corr, int n_win, int n, int method, double* dist,
                                      void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, corr); CHECK_PTR(ctx, dist); }
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be >= 1");
    return launch_corr_to_dist(ctx, corr, n_win, n, method, dist, (hipStream_t)stream);
}

tda_status tda_rips_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                 double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                 int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, dm); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1);
                 CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    return launch_rips_dm(ctx, dm, n_win, n, thresh, symmetrise, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, status,
                          (hipStream_t)stream);
}

tda_status tda_eeg_window_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t, double thresh,
                                    double* dist, double* corr, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                    int h1_cap, int* h1_cnt, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1);
                 CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (corr && !dist) TDA_FAIL(ctx, TDA_ERR_INVALID, "corr needs dist");
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    return launch_eeg_windows(ctx, win, n_win, n_ch, n_t, thresh, dist, corr, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt,
                              status, (hipStream_t)stream);
}

tda_status tda_eeg_window_sliding_dev(tda_ctx* ctx, const double* sig, int n_rec, int n_ch, int n_samples, int win_len,
                                      int step, const int* sel, int n_sel, double thresh, double* dist, double* corr,
                                      double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                      int* status, int* n_win_per_rec, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_rec); CHECK_NONNEG(ctx, n_sel);
    if (n_rec) { CHECK_PTR(ctx, sig); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1);
                 CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (corr && !dist) TDA_FAIL(ctx, TDA_ERR_INVALID, "corr needs dist");
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    return launch_eeg_sliding(ctx, sig, n_rec, n_ch, n_samples, win_len, step, sel, n_sel, thresh, dist, corr, h0, h0_cap,
                              h0_cnt, h1, h1_cap, h1_cnt, status, n_win_per_rec, (hipStream_t)stream);
}

tda_status tda_eeg_window_ragged_dev(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                     int n_win, int n_ch, int win_len, double thresh, double* dist, double* corr, double* h0,
                                     int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, sig); CHECK_PTR(ctx, win_start); CHECK_PTR(ctx, win_ld); CHECK_PTR(ctx, h0);
                 CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (corr && !dist) TDA_FAIL(ctx, TDA_ERR_INVALID, "corr needs dist");
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    return launch_eeg_ragged(ctx, sig, win_start, win_ld, n_win, n_ch, win_len, thresh, dist, corr, h0, h0_cap, h0_cnt, h1,
                             h1_cap, h1_cnt, status, (hipStream_t)stream);
}

tda_status tda_takens_rips_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                     int subsample, double thresh, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                     int h1_cap, int* h1_cnt, int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt);
                 CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    if (n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be >= 1");
    return launch_rips_cloud(ctx, win, tau, n_win, n_t, dim, subsample, 0, 1, thresh, h0, h0_cap, h0_cnt, h1, h1_cap,
                             h1_cnt, n_points, status, (hipStream_t)stream);
}

tda_status tda_cloud_rips_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                    int normalise, double thresh, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                    int h1_cap, int* h1_cnt, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt);
                 CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    if (p_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "p_cap must be >= 1");
    return launch_rips_cloud(ctx, pc, n_pts, n_win, p_cap, dim, 1, 1, normalise, thresh, h0, h0_cap, h0_cnt, h1,
                             h1_cap, h1_cnt, nullptr, status, (hipStream_t)stream);
}

#define CHECK_LM_PTRS(ctx) do { CHECK_PTR(ctx, lm); CHECK_PTR(ctx, lm_idx); CHECK_PTR(ctx, r_cover); CHECK_PTR(ctx, n_lm); \
                                CHECK_PTR(ctx, n_full); } while (0)

tda_status tda_takens_landmarks_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                    int subsample, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                    double* r_cover, int* n_lm, int* n_full, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_LM_PTRS(ctx); }
    return launch_landmarks(ctx, win, tau, n_win, n_t, dim, subsample, 0, 1, n_perm, lm, lm_idx, lm_lambda, r_cover, n_lm,
                            n_full, (hipStream_t)stream);
}

tda_status tda_cloud_landmarks_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                   int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                   double* r_cover, int* n_lm, int* n_full, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_LM_PTRS(ctx); }
    return launch_landmarks(ctx, pc, n_pts, n_win, p_cap, dim, 1, 1, normalise, n_perm, lm, lm_idx, lm_lambda, r_cover,
                            n_lm, n_full, (hipStream_t)stream);
}

tda_status tda_takens_rips_landmarks_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                         int subsample, int n_perm, double thresh, double* lm, int* lm_idx,
                                         double* lm_lambda, double* r_cover, int* n_lm, int* n_full,
                                         double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                         int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_LM_PTRS(ctx); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt);
                 CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status); }
    // everything the second stage would refuse is refused here, before the first one is launched
    if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    if (n_perm >= 3 && h0_cap < n_perm) TDA_FAIL(ctx, TDA_ERR_INVALID, "h0_cap must be >= n_perm");
    tda_status rc = launch_landmarks(ctx, win, tau, n_win, n_t, dim, subsample, 0, 1, n_perm, lm, lm_idx, lm_lambda,
                                     r_cover, n_lm, n_full, (hipStream_t)stream);
    if (rc != TDA_OK) return rc;
    // the landmark rows are normalised already; a refused window carries a count above TDA_MAX_POINTS
    return launch_rips_cloud(ctx, lm, n_lm, n_win, n_perm, dim, 1, 1, 0, thresh, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt,
                             n_points, status, (hipStream_t)stream);
}

tda_status tda_sosfiltfilt_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos,
                               const double* zi, int n_sections, int edge, double* y, double* work, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, sos); CHECK_PTR(ctx, zi);
    return launch_sosfiltfilt(ctx, x, n_sig, n_samples, sos, zi, n_sections, edge, y, work, (hipStream_t)stream);
}

tda_status tda_filtfilt_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b, const double* a,
                            const double* zi, int ntaps, int edge, double* y, double* work, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, b); CHECK_PTR(ctx, a); CHECK_PTR(ctx, zi);
    return launch_filtfilt(ctx, x, n_sig, n_samples, b, a, zi, ntaps, edge, y, work, (hipStream_t)stream);
}

tda_status tda_sosfiltfilt_bank_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos,
                                    const double* zi, int n_filters, int n_sections, int edge, double* y, double* work,
                                    void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, sos); CHECK_PTR(ctx, zi);
    return launch_sosfiltfilt(ctx, x, n_sig, n_samples, sos, zi, n_sections, edge, y, work, (hipStream_t)stream, n_filters);
}

tda_status tda_filtfilt_bank_dev(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b, const double* a,
                                 const double* zi, int n_filters, int ntaps, int edge, double* y, double* work, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, b); CHECK_PTR(ctx, a); CHECK_PTR(ctx, zi);
    return launch_filtfilt(ctx, x, n_sig, n_samples, b, a, zi, ntaps, edge, y, work, (hipStream_t)stream, n_filters);
}

tda_status tda_sosfiltfilt_bank_ragged_dev(tda_ctx* ctx, const double* x, int n_rec, int n_ch, const long long* len,
                                           const long long* off, const long long* len_host, const double* sos,
                                           const double* zi, int n_filters, int n_sections, int edge, double* y,
                                           double* work, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_rec); CHECK_NONNEG(ctx, n_ch);
    if (n_rec && n_ch) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, len); CHECK_PTR(ctx, off); CHECK_PTR(ctx, len_host);
                         CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, sos); CHECK_PTR(ctx, zi);
    return launch_sosfiltfilt_ragged(ctx, x, n_rec, n_ch, len, off, len_host, sos, zi, n_filters, n_sections, edge, y, work,
                                     (hipStream_t)stream);
}

tda_status tda_filtfilt_bank_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len, const long long* off,
                                        const long long* len_host, const double* b, const double* a, const double* zi,
                                        int n_filters, int ntaps, int edge, double* y, double* work, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, len); CHECK_PTR(ctx, off); CHECK_PTR(ctx, len_host);
                 CHECK_PTR(ctx, y); CHECK_PTR(ctx, work); }
    CHECK_PTR(ctx, b); CHECK_PTR(ctx, a); CHECK_PTR(ctx, zi);
    return launch_filtfilt_ragged(ctx, x, n_sig, len, off, len_host, b, a, zi, n_filters, ntaps, edge, y, work,
                                  (hipStream_t)stream);
}

tda_status tda_gather_windows_dev(tda_ctx* ctx, const double* src, const long long* start, int n_win, int win_len,
                                  double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, src); CHECK_PTR(ctx, start); CHECK_PTR(ctx, out); }
    return launch_gather_windows(ctx, src, start, n_win, win_len, out, (hipStream_t)stream);
}

tda_status tda_upfirdn_dev(tda_ctx* ctx, const double* x, long long n_in, const double* h, int len_h, int up, int down,
                           long long n_pre_remove, long long n_out, double* y, void* stream)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, h); CHECK_PTR(ctx, y);
    return launch_upfirdn(ctx, x, n_in, h, len_h, up, down, n_pre_remove, n_out, y, (hipStream_t)stream);
}

tda_status tda_hilbert_envelope_dev(tda_ctx* ctx, const double* x, int n, const double* g, double* env, void* stream)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, g); CHECK_PTR(ctx, env);
    return launch_hilbert_env(ctx, x, n, g, env, (hipStream_t)stream);
}

tda_status tda_resample_poly_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len, const long long* off,
                                        const long long* len_host, const long long* out_off, const double* hp,
                                        int n_phase_taps, int up, int down, int n_pre_remove, double* y, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, len); CHECK_PTR(ctx, off); CHECK_PTR(ctx, len_host);
                 CHECK_PTR(ctx, out_off); CHECK_PTR(ctx, hp); CHECK_PTR(ctx, y); }
    return launch_resample_poly_ragged(ctx, x, n_sig, len, off, len_host, out_off, hp, n_phase_taps, up, down, n_pre_remove,
                                       y, (hipStream_t)stream);
}

tda_status tda_hilbert_envelope_ragged_dev(tda_ctx* ctx, const double* x, int n_sig, const long long* len,
                                           const long long* off, const long long* len_host, const double* g,
                                           const long long* g_off, double* env, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, len); CHECK_PTR(ctx, off); CHECK_PTR(ctx, len_host);
                 CHECK_PTR(ctx, g); CHECK_PTR(ctx, g_off); CHECK_PTR(ctx, env); }
    return launch_hilbert_env_ragged(ctx, x, n_sig, len, off, len_host, g, g_off, env, (hipStream_t)stream);
}

tda_status tda_tau_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int* tau, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); }
    return launch_tau(ctx, win, n_win, n_t, max_lag, tau, (hipStream_t)stream);
}

tda_status tda_tau_segments_dev(tda_ctx* ctx, const double* win, const int* seg_off, int n_seg, int n_t, int max_lag,
                                int* tau_seg, int* tau_win, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, tau_seg); }
    return launch_tau_segments(ctx, win, seg_off, n_seg, n_t, max_lag, tau_seg, tau_win, (hipStream_t)stream);
}

tda_status tda_recording_rows_dev(tda_ctx* ctx, const double* w_h0, const double* w_h1, const int* tau_seg,
                                  const double* feat_h0, const double* feat_h1, const int* seg_off, int n_seg,
                                  double* out, const int* status_a, const int* status_b, int* seg_flags, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, w_h0); CHECK_PTR(ctx, w_h1); CHECK_PTR(ctx, tau_seg); CHECK_PTR(ctx, feat_h0);
                 CHECK_PTR(ctx, feat_h1); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out); }
    return launch_recording_rows(ctx, w_h0, w_h1, tau_seg, feat_h0, feat_h1, seg_off, n_seg, out, status_a, status_b,
                                 seg_flags, (hipStream_t)stream);
}

tda_status tda_features_batch_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, double* feat,
                                  void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm);
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, feat); }
    return launch_features(ctx, dgm, cnt, n_dgm, cap, feat, (hipStream_t)stream);
}

tda_status tda_aggregate_batch_dev(tda_ctx* ctx, const double* feat_h0, const double* feat_h1, const int* seg_off,
                                   int n_seg, double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, feat_h0); CHECK_PTR(ctx, feat_h1); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out); }
    return launch_aggregate(ctx, feat_h0, feat_h1, seg_off, n_seg, out, (hipStream_t)stream);
}

tda_status tda_segment_nanmean_dev(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg, double* out,
                                   void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out); }
    return launch_nanmean(ctx, x, seg_off, n_seg, out, (hipStream_t)stream);
}

tda_status tda_spearman_batch_dev(tda_ctx* ctx, const double* x, const double* y, int ld, const int* cols, int n_cols,
                                  const int* seg_off, int n_seg, double* r, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, cols); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, r); }
    return launch_spearman(ctx, x, y, ld, cols, n_cols, seg_off, n_seg, r, (hipStream_t)stream);
}

tda_status tda_temporal_corr_dev(tda_ctx* ctx, const double* fa, const double* fe, int ld, const int* cols, int n_cols,
                                 const int* seg_off, int n_seg, const int* status_b, double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg); CHECK_NONNEG(ctx, n_cols);
    if (n_seg == 0 || n_cols == 0) return TDA_OK;
    CHECK_PTR(ctx, fa); CHECK_PTR(ctx, fe); CHECK_PTR(ctx, cols); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    if (ld < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "ld must be >= 1");
    return launch_temporal_corr(ctx, fa, fe, ld, cols, n_cols, seg_off, n_seg, status_b, out, (hipStream_t)stream);
}

tda_status tda_wasserstein_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                     const double* dgm_b, const int* cnt_b, int cap_b, const int* idx_a,
                                     const int* idx_b, int n_pairs, double* out, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if (n_pairs) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b);
                   CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    return launch_wasserstein(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, idx_a, idx_b, n_pairs, out, status,
                              (hipStream_t)stream);
}

tda_status tda_bottleneck_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                    const double* dgm_b, const int* cnt_b, int cap_b, const int* idx_a,
                                    const int* idx_b, int n_pairs, double* out, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if (n_pairs) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b);
                   CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    return launch_bottleneck(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, idx_a, idx_b, n_pairs, out, status,
                             (hipStream_t)stream);
}

tda_status tda_wasserstein_q_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                       const double* dgm_b, const int* cnt_b, int cap_b, const int* idx_a,
                                       const int* idx_b, int n_pairs, int order, int ground, double* out, int* status,
                                       void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if (n_pairs) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b);
                   CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    return launch_wasserstein_q(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, idx_a, idx_b, n_pairs, order, ground, out,
                                status, (hipStream_t)stream);
}

tda_status tda_sliced_wasserstein_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a,
                                            const double* dgm_b, const int* cnt_b, int cap_b, const int* idx_a,
                                            const int* idx_b, int n_pairs, const double* dirs, int n_dirs, double* out,
                                            int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if (n_pairs) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b);
                   CHECK_PTR(ctx, dirs); CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    return launch_sliced(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, idx_a, idx_b, n_pairs, dirs, n_dirs, out, status,
                         (hipStream_t)stream);
}

tda_status tda_landscape_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                                  int n_seg, const int* status, int skip_mask, const double* grid, int n_grid,
                                  int n_levels, double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm); CHECK_NONNEG(ctx, n_seg);
    if (!seg_off && n_seg != n_dgm) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); }
    if (n_seg) { CHECK_PTR(ctx, grid); CHECK_PTR(ctx, out); }
    return launch_landscape_mean(ctx, dgm, cnt, cap, n_dgm, seg_off, n_seg, status, skip_mask, grid, n_grid, n_levels, out,
                                 (hipStream_t)stream);
}

tda_status tda_euler_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                  const double* grid, int n_grid, int max_dim, int* counts, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, dm); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status); }
    return launch_euler(ctx, dm, nullptr, n_win, n, 0, 1, 2, symmetrise, thresh, grid, n_grid, max_dim, counts, nullptr,
                        status, (hipStream_t)stream);
}

tda_status tda_euler_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                     int normalise, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                     int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status); }
    return launch_euler(ctx, pc, n_pts, n_win, p_cap, dim, 1, 1, normalise, thresh, grid, n_grid, max_dim, counts, nullptr,
                        status, (hipStream_t)stream);
}

tda_status tda_euler_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                      int subsample, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                      int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status); }
    return launch_euler(ctx, win, tau, n_win, n_t, dim, subsample, 0, 1, thresh, grid, n_grid, max_dim, counts, n_points,
                        status, (hipStream_t)stream);
}

tda_status tda_euler_mean_dev(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off,
                              int n_seg, const int* status_in, int skip_mask, double* mean, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    if (n_win) CHECK_PTR(ctx, counts);
    if (n_seg) CHECK_PTR(ctx, mean);
    return launch_euler_mean(ctx, counts, n_win, max_dim, n_grid, seg_off, n_seg, status_in, skip_mask, mean,
                             (hipStream_t)stream);
}

// the row inputs and the outputs that the tda_generators_* entry points share, in the header's order
#define GEN_PARAMS                                                                                                     \
    const double* h0, int h0_cap, const int* h0_cnt, const double* h1, int h1_cap, const int* h1_cnt,                  \
    const int* rips_status, int skip_mask, int cyc_cap, short* h1_gen, int* h1_flag, short* cyc, int* cyc_len,         \
    double* part, short* h0_edge, int* work
#define GEN_PASS h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, rips_status, skip_mask, cyc_cap, h1_gen, h1_flag, cyc, cyc_len, \
                 part, h0_edge, work
#define GEN_CHECK_PTRS(ctx) do { CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, h1_gen); CHECK_PTR(ctx, h1_flag); \
                                 CHECK_PTR(ctx, cyc_len); CHECK_PTR(ctx, status); } while (0)

static GenArgs gen_args(GEN_PARAMS)
{
    GenArgs g;
    g.h0 = h0; g.h0_cap = h0_cap; g.h0_cnt = h0_cnt; g.h1 = h1; g.h1_cap = h1_cap; g.h1_cnt = h1_cnt;
    g.rips_status = rips_status; g.skip_mask = skip_mask; g.cyc_cap = cyc_cap;
    g.h1_gen = h1_gen; g.h1_flag = h1_flag; g.cyc = cyc; g.cyc_len = cyc_len; g.part = part; g.h0_edge = h0_edge; g.work = work;
    g.part_ld = 0;
    return g;
}

tda_status tda_generators_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                       GEN_PARAMS, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, dm); GEN_CHECK_PTRS(ctx); }
    return launch_generators(ctx, dm, nullptr, n_win, n, 0, 1, 2, symmetrise, thresh, gen_args(GEN_PASS), nullptr, status,
                             (hipStream_t)stream);
}

tda_status tda_generators_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                          int normalise, double thresh, GEN_PARAMS, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); GEN_CHECK_PTRS(ctx); }
    return launch_generators(ctx, pc, n_pts, n_win, p_cap, dim, 1, 1, normalise, thresh, gen_args(GEN_PASS), nullptr, status,
                             (hipStream_t)stream);
}

tda_status tda_generators_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                           int subsample, double thresh, GEN_PARAMS, int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); GEN_CHECK_PTRS(ctx); }
    return launch_generators(ctx, win, tau, n_win, n_t, dim, subsample, 0, 1, thresh, gen_args(GEN_PASS), n_points, status,
                             (hipStream_t)stream);
}

tda_status tda_generators_mean_dev(tda_ctx* ctx, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                                   const int* status_in, int skip_mask, double* mean, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    if (n_win) CHECK_PTR(ctx, part);
    if (n_seg) CHECK_PTR(ctx, mean);
    return launch_generators_mean(ctx, part, n_win, n, seg_off, n_seg, status_in, skip_mask, mean, (hipStream_t)stream);
}

tda_status tda_frechet_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                                int n_seg, const int* status_in, int skip_mask, int max_iter, double* mean, int* mean_cnt,
                                int cap_out, double* var, int* iters, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm); CHECK_NONNEG(ctx, n_seg);
    if (!seg_off && n_seg != n_dgm) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); }
    if (n_seg) { CHECK_PTR(ctx, mean); CHECK_PTR(ctx, mean_cnt); CHECK_PTR(ctx, var); CHECK_PTR(ctx, iters); CHECK_PTR(ctx, status); }
    return launch_frechet_mean(ctx, dgm, cnt, cap, n_dgm, seg_off, n_seg, status_in, skip_mask, max_iter, mean, mean_cnt,
                               cap_out, var, iters, status, (hipStream_t)stream);
}

tda_status tda_image_mean_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                              int n_seg, const int* status, int skip_mask, const double* xe, int n_x, const double* ye,
                              int n_y, double sigma, int power, double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm); CHECK_NONNEG(ctx, n_seg);
    if (!seg_off && n_seg != n_dgm) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); }
    if (n_seg) { CHECK_PTR(ctx, xe); CHECK_PTR(ctx, ye); CHECK_PTR(ctx, out); }
    return launch_image_mean(ctx, dgm, cnt, cap, n_dgm, seg_off, n_seg, status, skip_mask, xe, n_x, ye, n_y, sigma, power,
                             out, (hipStream_t)stream);
}

tda_status tda_wasserstein_cross_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                     const int* grp_a, const int* seg_off_a, int n_seg_a, const double* dgm_b,
                                     const int* cnt_b, int cap_b, int n_b, const int* seg_off_b, int n_seg_b,
                                     const int* status_b, const int* partner_seg, double* out, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_seg_a); CHECK_NONNEG(ctx, n_b); CHECK_NONNEG(ctx, n_seg_b);
    if (n_a == 0) return TDA_OK;
    if (n_seg_a < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagrams without a group");
    CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, grp_a); CHECK_PTR(ctx, seg_off_a); CHECK_PTR(ctx, partner_seg);
    CHECK_PTR(ctx, out); CHECK_PTR(ctx, status);
    if (n_b && n_seg_b) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); CHECK_PTR(ctx, seg_off_b); CHECK_PTR(ctx, status_b); }
    else { n_b = 0; n_seg_b = 0; }                                     // nothing to pair with: every diagram gets "no pair"
    return launch_wasserstein_cross(ctx, dgm_a, cnt_a, cap_a, n_a, grp_a, seg_off_a, n_seg_a, dgm_b, cnt_b, cap_b, n_b,
                                    seg_off_b, n_seg_b, status_b, partner_seg, out, status, (hipStream_t)stream);
}

tda_status tda_cross_rows_dev(tda_ctx* ctx, const double* w_matched, const int* status_matched, const double* w_mismatched,
                              const int* status_mismatched, const int* seg_off_a, int n_seg, double* out,
                              const int* status_a, int* seg_flags, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, w_matched); CHECK_PTR(ctx, status_matched); CHECK_PTR(ctx, w_mismatched);
                 CHECK_PTR(ctx, status_mismatched); CHECK_PTR(ctx, seg_off_a); CHECK_PTR(ctx, out); }
    return launch_cross_rows(ctx, w_matched, status_matched, w_mismatched, status_mismatched, seg_off_a, n_seg, out,
                             status_a, seg_flags, (hipStream_t)stream);
}

tda_status tda_wasserstein_matrix_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                      const int* seg_off_a, int n_seg_a, const int* cls_a, const double* dgm_b,
                                      const int* cnt_b, int cap_b, int n_b, const int* seg_off_b, int n_cls, int n_col,
                                      const int* status_b, double* out, int* pairs, int* flags, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_seg_a); CHECK_NONNEG(ctx, n_b); CHECK_NONNEG(ctx, n_cls);
    CHECK_NONNEG(ctx, n_col);
    if (n_seg_a == 0 || n_col == 0) return TDA_OK;
    CHECK_PTR(ctx, seg_off_a); CHECK_PTR(ctx, cls_a); CHECK_PTR(ctx, out); CHECK_PTR(ctx, pairs); CHECK_PTR(ctx, flags);
    if (n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if ((long long)n_cls * n_col >= 0x7fffffffll) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "more than 2^31 - 2 B groups");
    if (n_b && n_cls) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); CHECK_PTR(ctx, seg_off_b); CHECK_PTR(ctx, status_b); }
    else { n_b = 0; n_cls = 0; }                                       // nothing to pair with: every entry is NaN with 0 pairs
    return launch_wasserstein_matrix(ctx, dgm_a, cnt_a, cap_a, n_a, seg_off_a, n_seg_a, cls_a, dgm_b, cnt_b, cap_b, n_b,
                                     seg_off_b, n_cls, n_col, status_b, out, pairs, flags, (hipStream_t)stream);
}

tda_status tda_match_rows_dev(tda_ctx* ctx, const double* out, const int* pairs, const int* flags, int n_seg_a, int n_col,
                              const int* own_col, const int* status_a, const int* seg_off_a, double* rows, int* seg_flags,
                              void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg_a); CHECK_NONNEG(ctx, n_col);
    if (n_seg_a == 0) return TDA_OK;
    CHECK_PTR(ctx, own_col); CHECK_PTR(ctx, rows);
    if (n_col) { CHECK_PTR(ctx, out); CHECK_PTR(ctx, pairs); CHECK_PTR(ctx, flags); }
    if (status_a) CHECK_PTR(ctx, seg_off_a);
    return launch_match_rows(ctx, out, pairs, flags, n_seg_a, n_col, own_col, status_a, seg_off_a, rows, seg_flags,
                             (hipStream_t)stream);
}

tda_status tda_sliced_prepare_dev(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const double* dirs,
                                  int n_dirs, const long long* slot_off, double* table, long long table_rows, int* m_clean,
                                  void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm); CHECK_NONNEG(ctx, table_rows);
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, dirs); CHECK_PTR(ctx, slot_off); CHECK_PTR(ctx, m_clean);
                 if (table_rows) CHECK_PTR(ctx, table); }
    return launch_sliced_prepare(ctx, dgm, cnt, cap, n_dgm, dirs, n_dirs, slot_off, table, table_rows, m_clean,
                                 (hipStream_t)stream);
}

tda_status tda_sliced_prepared_pairs_dev(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a,
                                         int n_a, const double* table_b, const long long* slot_off_b, const int* m_b, int n_b,
                                         const int* idx_a, const int* idx_b, int n_pairs, int n_dirs, double* out, int* status,
                                         void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_b);
    if (n_pairs) { CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    if (n_pairs && n_a) { CHECK_PTR(ctx, table_a); CHECK_PTR(ctx, slot_off_a); CHECK_PTR(ctx, m_a); }
    if (n_pairs && n_b) { CHECK_PTR(ctx, table_b); CHECK_PTR(ctx, slot_off_b); CHECK_PTR(ctx, m_b); }
    return launch_sliced_prepared_pairs(ctx, table_a, slot_off_a, m_a, n_a, table_b, slot_off_b, m_b, n_b, idx_a, idx_b,
                                        n_pairs, n_dirs, out, status, (hipStream_t)stream);
}

tda_status tda_sliced_matrix_dev(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a, int n_a,
                                 const int* seg_off_a, int n_seg_a, const int* cls_a, const double* table_b,
                                 const long long* slot_off_b, const int* m_b, int n_b, const int* seg_off_b, int n_cls,
                                 int n_col, const int* status_b, int n_dirs, double* out, int* pairs, int* flags, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_seg_a); CHECK_NONNEG(ctx, n_b); CHECK_NONNEG(ctx, n_cls);
    CHECK_NONNEG(ctx, n_col);
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_dirs must be 1..TDA_MAX_DIRECTIONS");
    if (n_seg_a == 0 || n_col == 0) return TDA_OK;
    CHECK_PTR(ctx, seg_off_a); CHECK_PTR(ctx, cls_a); CHECK_PTR(ctx, out); CHECK_PTR(ctx, pairs); CHECK_PTR(ctx, flags);
    if (n_a) { CHECK_PTR(ctx, table_a); CHECK_PTR(ctx, slot_off_a); CHECK_PTR(ctx, m_a); }
    if ((long long)n_cls * n_col >= 0x7fffffffll) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "more than 2^31 - 2 B groups");
    if (n_b && n_cls) { CHECK_PTR(ctx, table_b); CHECK_PTR(ctx, slot_off_b); CHECK_PTR(ctx, m_b); CHECK_PTR(ctx, seg_off_b);
                        CHECK_PTR(ctx, status_b); }
    else { n_b = 0; n_cls = 0; }                                       // nothing to pair with: every entry is NaN with 0 pairs
    return launch_sliced_matrix(ctx, table_a, slot_off_a, m_a, n_a, seg_off_a, n_seg_a, cls_a, table_b, slot_off_b, m_b, n_b,
                                seg_off_b, n_cls, n_col, status_b, n_dirs, out, pairs, flags, (hipStream_t)stream);
}

tda_status tda_diagram_kernel_pairs_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                        const int* idx_b, int n_pairs, double ninv, int mirror, double scale, int weight,
                                        double wc, double* out, double* kvals, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_b);
    if (n_pairs) { CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    if (n_pairs && n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (n_pairs && n_b) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); }
    return launch_diagram_kernel_pairs(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, ninv,
                                       mirror, scale, weight, wc, out, kvals, status, (hipStream_t)stream);
}

tda_status tda_diagram_kernel_gram_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                       const int* seg_off_a, int n_seg_a, const int* status_a, const double* dgm_b,
                                       const int* cnt_b, int n_b, int cap_b, const int* seg_off_b, int n_seg_b,
                                       const int* status_b, int skip_mask, double ninv, int mirror, double scale, int weight,
                                       double wc, double* out, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_seg_a);
    if (!seg_off_a && n_seg_a != n_a) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (dgm_b) {
        CHECK_NONNEG(ctx, n_b); CHECK_NONNEG(ctx, n_seg_b); CHECK_PTR(ctx, cnt_b);
        if (!seg_off_b && n_seg_b != n_b) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    }
    if (n_seg_a && (!dgm_b || n_seg_b)) CHECK_PTR(ctx, out);
    return launch_diagram_kernel_gram(ctx, dgm_a, cnt_a, cap_a, n_a, seg_off_a, n_seg_a, status_a, dgm_b, cnt_b, cap_b, n_b,
                                      seg_off_b, n_seg_b, status_b, skip_mask, ninv, mirror, scale, weight, wc, out,
                                      (hipStream_t)stream);
}

tda_status tda_persistence_fisher_batch_dev(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                            const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                            const int* idx_b, int n_pairs, double ninv, double* out, int* status,
                                            void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_b);
    if (n_pairs) { CHECK_PTR(ctx, out); CHECK_PTR(ctx, status); }
    if (n_pairs && n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (n_pairs && n_b) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); }
    return launch_persistence_fisher(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, ninv, out,
                                     status, (hipStream_t)stream);
}

tda_status tda_sublevel_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                  int n_win, int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status,
                                  void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, sig); CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, status); }
    return launch_sublevel(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, dgm, cap, cnt, idx, status, (hipStream_t)stream);
}

tda_status tda_plv_dist_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                  int n_win, int n_ch, int n_t, const double* g, int method, double* dist, double* plv,
                                  int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, sig); CHECK_PTR(ctx, g); CHECK_PTR(ctx, dist); CHECK_PTR(ctx, status); }
    return launch_plv_dist(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, plv, status, (hipStream_t)stream);
}

tda_status tda_connectivity_dist_batch_dev(tda_ctx* ctx, const double* sig, const long long* win_start,
                                           const long long* win_ld, int n_win, int n_ch, int n_t, const double* g,
                                           int measure, int method, double* dist, double* value, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, sig); CHECK_PTR(ctx, g); CHECK_PTR(ctx, dist); CHECK_PTR(ctx, status); }
    return launch_connectivity_dist(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status,
                                    (hipStream_t)stream);
}

tda_status tda_perm_sums_batch_dev(tda_ctx* ctx, const double* D, int n_mat, int n, int ld, const unsigned long long* lab,
                                   int n_perm, double* work, long long work_doubles, double* out, int* n1, void* stream)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, lab);
    if (n_mat > 0) { CHECK_PTR(ctx, D); CHECK_PTR(ctx, work); CHECK_PTR(ctx, out); }
    return launch_perm_sums(ctx, D, n_mat, n, ld, lab, n_perm, work, work_doubles, out, n1, (hipStream_t)stream);
}

// ---------------------------------------------------------------- host-pointer twins
// A bump allocator over the context workspace; everything is staged, launched on the
// default stream, copied back and synchronised.
struct Stage {
    tda_ctx* ctx;
    size_t need = 0, used = 0;
    struct Item { void** dev; const void* src; void* dst; size_t bytes; };
    std::vector<Item> items;
    explicit Stage(tda_ctx* c) : ctx(c) {}
    void add(void** dev, const void* src, void* dst, size_t bytes)
    {
        items.push_back({dev, src, dst, bytes});
        need += (bytes + 255) & ~(size_t)255;
    }
    tda_status upload()
    {
        if (need > ctx->ws_bytes) {
            if (ctx->ws) TDA_HIP(ctx, hipFree(ctx->ws));
            ctx->ws = nullptr; ctx->ws_bytes = 0;
            TDA_HIP(ctx, hipMalloc(&ctx->ws, need));
            ctx->ws_bytes = need;
        }
        char* p = (char*)ctx->ws;
        for (auto& it : items) {
            *it.dev = it.bytes ? p : nullptr;
            if (it.src && it.bytes) TDA_HIP(ctx, hipMemcpyAsync(p, it.src, it.bytes, hipMemcpyHostToDevice, 0));
            p += (it.bytes + 255) & ~(size_t)255;
        }
        return TDA_OK;
    }
    tda_status download()
    {
        for (auto& it : items)
            if (it.dst && it.bytes) TDA_HIP(ctx, hipMemcpyAsync(it.dst, *it.dev, it.bytes, hipMemcpyDeviceToHost, 0));
        TDA_HIP(ctx, hipStreamSynchronize(0));
        return TDA_OK;
    }
};

#define RET_IF(x) do { tda_status s__ = (x); if (s__ != TDA_OK) return s__; } while (0)

tda_status tda_corr_dist_batch(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t, double* dist, double* corr)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, dist);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_win, *d_dist, *d_corr = nullptr;
    const size_t nw = (size_t)n_win;
    s.add((void**)&d_win, win, nullptr, nw * n_ch * n_t * 8);
    s.add((void**)&d_dist, nullptr, dist, nw * n_ch * n_ch * 8);
    if (corr) s.add((void**)&d_corr, nullptr, corr, nw * n_ch * n_ch * 8);
    RET_IF(s.upload());
    RET_IF(tda_corr_dist_batch_dev(ctx, d_win, n_win, n_ch, n_t, d_dist, d_corr, nullptr));
    return s.download();
}

tda_status tda_corr_dist_sliding(tda_ctx* ctx, const double* sig, int n_ch, int n_samples, int win_len, int step,
                                 double* dist, double* corr, int* n_win)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, sig); CHECK_PTR(ctx, dist); CHECK_NONNEG(ctx, n_samples);
    if (win_len < 2 || step < 1 || n_ch < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad window geometry");
    const int nw = n_samples >= win_len ? (n_samples - win_len) / step + 1 : 0;
    if (n_win) *n_win = nw;
    if (nw == 0) return TDA_OK;
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_sig, *d_dist, *d_corr = nullptr;
    s.add((void**)&d_sig, sig, nullptr, (size_t)n_ch * n_samples * 8);
    s.add((void**)&d_dist, nullptr, dist, (size_t)nw * n_ch * n_ch * 8);
    if (corr) s.add((void**)&d_corr, nullptr, corr, (size_t)nw * n_ch * n_ch * 8);
    RET_IF(s.upload());
    RET_IF(tda_corr_dist_sliding_dev(ctx, d_sig, n_ch, n_samples, win_len, step, d_dist, d_corr, nullptr, nullptr));
    return s.download();
}

tda_status tda_corr_to_dist_batch(tda_ctx* ctx, const double* corr, int n_win, int n, int method, double* dist)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, corr); CHECK_PTR(ctx, dist);
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_c, *d_d;
    s.add((void**)&d_c, corr, nullptr, (size_t)n_win * n * n * 8);
    s.add((void**)&d_d, nullptr, dist, (size_t)n_win * n * n * 8);
    RET_IF(s.upload());
    RET_IF(tda_corr_to_dist_batch_dev(ctx, d_c, n_win, n, method, d_d, nullptr));
    return s.download();
}

tda_status tda_rips_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                             double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt);
    CHECK_PTR(ctx, status);
    if (h0_cap < 1 || h1_cap < 1 || n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n, h0_cap, h1_cap must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dm, *d_h0, *d_h1; int *d_c0, *d_c1, *d_st;
    const size_t nw = (size_t)n_win;
    s.add((void**)&d_dm, dm, nullptr, nw * n * n * 8);
    s.add((void**)&d_h0, nullptr, h0, nw * h0_cap * 16);
    s.add((void**)&d_h1, nullptr, h1, nw * h1_cap * 16);
    s.add((void**)&d_c0, nullptr, h0_cnt, nw * 4);
    s.add((void**)&d_c1, nullptr, h1_cnt, nw * 4);
    s.add((void**)&d_st, nullptr, status, nw * 4);
    RET_IF(s.upload());
    RET_IF(tda_rips_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, d_h0, h0_cap, d_c0, d_h1, h1_cap, d_c1, d_st,
                                 nullptr));
    return s.download();
}

tda_status tda_takens_rips_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                 int subsample, double thresh, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                 int h1_cap, int* h1_cnt, int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1);
    CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status);
    if (h0_cap < 1 || h1_cap < 1 || n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t, h0_cap, h1_cap must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_win, *d_h0, *d_h1; int *d_tau, *d_c0, *d_c1, *d_np, *d_st;
    const size_t nw = (size_t)n_win;
    s.add((void**)&d_win, win, nullptr, nw * n_t * 8);
    s.add((void**)&d_tau, tau, nullptr, nw * 4);
    s.add((void**)&d_h0, nullptr, h0, nw * h0_cap * 16);
    s.add((void**)&d_h1, nullptr, h1, nw * h1_cap * 16);
    s.add((void**)&d_c0, nullptr, h0_cnt, nw * 4);
    s.add((void**)&d_c1, nullptr, h1_cnt, nw * 4);
    s.add((void**)&d_np, nullptr, n_points, nw * 4);
    s.add((void**)&d_st, nullptr, status, nw * 4);
    RET_IF(s.upload());
    RET_IF(tda_takens_rips_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, d_h0, h0_cap, d_c0, d_h1,
                                     h1_cap, d_c1, d_np, d_st, nullptr));
    return s.download();
}

tda_status tda_cloud_rips_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                int normalise, double thresh, double* h0, int h0_cap, int* h0_cnt, double* h1,
                                int h1_cap, int* h1_cnt, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1);
    CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status);
    if (h0_cap < 1 || h1_cap < 1 || p_cap < 1 || dim < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_pc, *d_h0, *d_h1; int *d_n, *d_c0, *d_c1, *d_st;
    const size_t nw = (size_t)n_win;
    s.add((void**)&d_pc, pc, nullptr, nw * p_cap * dim * 8);
    s.add((void**)&d_n, n_pts, nullptr, nw * 4);
    s.add((void**)&d_h0, nullptr, h0, nw * h0_cap * 16);
    s.add((void**)&d_h1, nullptr, h1, nw * h1_cap * 16);
    s.add((void**)&d_c0, nullptr, h0_cnt, nw * 4);
    s.add((void**)&d_c1, nullptr, h1_cnt, nw * 4);
    s.add((void**)&d_st, nullptr, status, nw * 4);
    RET_IF(s.upload());
    RET_IF(tda_cloud_rips_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, d_h0, h0_cap, d_c0, d_h1,
                                    h1_cap, d_c1, d_st, nullptr));
    return s.download();
}

// The landmark outputs of a host call: staged in BOTH directions, so what the kernel leaves untouched stays the caller's.
struct LmStage {
    double *lm, *lambda, *rc; int *idx, *n_lm, *n_full;
    void add(Stage& s, int n_win, int n_perm, int dim, double* h_lm, int* h_idx, double* h_lambda, double* h_rc, int* h_nlm,
             int* h_nfull)
    {
        const size_t nw = (size_t)n_win;
        lambda = nullptr;
        s.add((void**)&lm, h_lm, h_lm, nw * n_perm * dim * 8);
        s.add((void**)&idx, h_idx, h_idx, nw * n_perm * 4);
        if (h_lambda) s.add((void**)&lambda, h_lambda, h_lambda, nw * n_perm * 8);
        s.add((void**)&rc, h_rc, h_rc, nw * 8);
        s.add((void**)&n_lm, h_nlm, h_nlm, nw * 4);
        s.add((void**)&n_full, h_nfull, h_nfull, nw * 4);
    }
};
#define CHECK_LM_LIMITS(ctx, cap_ok)                                                                                   \
    do { if (n_perm < 3 || n_perm > TDA_MAX_POINTS || dim < 1 || dim > TDA_MAX_DIM || !(cap_ok))                      \
             TDA_FAIL(ctx, TDA_ERR_INVALID, "landmarks: n_perm, dim or a size outside its limits"); } while (0)

tda_status tda_takens_landmarks(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                int subsample, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                                double* r_cover, int* n_lm, int* n_full)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    CHECK_LM_LIMITS(ctx, subsample >= 1 && n_t >= 1 && n_t <= TDA_LM_MAX_SAMPLES);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_LM_PTRS(ctx);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double* d_win; int* d_tau; LmStage o;
    s.add((void**)&d_win, win, nullptr, (size_t)n_win * n_t * 8);
    s.add((void**)&d_tau, tau, nullptr, (size_t)n_win * 4);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    RET_IF(s.upload());
    RET_IF(tda_takens_landmarks_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, n_perm, o.lm, o.idx, o.lambda, o.rc,
                                    o.n_lm, o.n_full, nullptr));
    return s.download();
}

tda_status tda_cloud_landmarks(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                               int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                               double* r_cover, int* n_lm, int* n_full)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    CHECK_LM_LIMITS(ctx, p_cap >= 1 && p_cap <= TDA_LM_MAX_POINTS);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_LM_PTRS(ctx);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double* d_pc; int* d_n; LmStage o;
    s.add((void**)&d_pc, pc, nullptr, (size_t)n_win * p_cap * dim * 8);
    s.add((void**)&d_n, n_pts, nullptr, (size_t)n_win * 4);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    RET_IF(s.upload());
    RET_IF(tda_cloud_landmarks_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, n_perm, o.lm, o.idx, o.lambda, o.rc,
                                   o.n_lm, o.n_full, nullptr));
    return s.download();
}

tda_status tda_takens_rips_landmarks(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                     int subsample, int n_perm, double thresh, double* lm, int* lm_idx,
                                     double* lm_lambda, double* r_cover, int* n_lm, int* n_full,
                                     double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt,
                                     int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    CHECK_LM_LIMITS(ctx, subsample >= 1 && n_t >= 1 && n_t <= TDA_LM_MAX_SAMPLES && h1_cap >= 1 && h0_cap >= n_perm);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_LM_PTRS(ctx); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt);
    CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt); CHECK_PTR(ctx, status);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_win, *d_h0, *d_h1; int *d_tau, *d_c0, *d_c1, *d_np = nullptr, *d_st; LmStage o;
    const size_t nw = (size_t)n_win;
    s.add((void**)&d_win, win, nullptr, nw * n_t * 8);
    s.add((void**)&d_tau, tau, nullptr, nw * 4);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    s.add((void**)&d_h0, nullptr, h0, nw * h0_cap * 16);
    s.add((void**)&d_h1, nullptr, h1, nw * h1_cap * 16);
    s.add((void**)&d_c0, nullptr, h0_cnt, nw * 4);
    s.add((void**)&d_c1, nullptr, h1_cnt, nw * 4);
    if (n_points) s.add((void**)&d_np, nullptr, n_points, nw * 4);
    s.add((void**)&d_st, nullptr, status, nw * 4);
    RET_IF(s.upload());
    RET_IF(tda_takens_rips_landmarks_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, n_perm, thresh, o.lm, o.idx,
                                         o.lambda, o.rc, o.n_lm, o.n_full, d_h0, h0_cap, d_c0, d_h1, h1_cap, d_c1, d_np,
                                         d_st, nullptr));
    return s.download();
}

tda_status tda_sosfiltfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos, const double* zi,
                           int n_sections, int edge, double* y)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, sos); CHECK_PTR(ctx, zi);
    if (n_samples < 1 || edge < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_y, *d_w;
    s.add((void**)&d_x, x, nullptr, (size_t)n_sig * n_samples * 8);
    s.add((void**)&d_y, nullptr, y, (size_t)n_sig * n_samples * 8);
    s.add((void**)&d_w, nullptr, nullptr, (size_t)n_sig * (n_samples + 2 * edge) * 8);
    RET_IF(s.upload());
    RET_IF(tda_sosfiltfilt_dev(ctx, d_x, n_sig, n_samples, sos, zi, n_sections, edge, d_y, d_w, nullptr));
    return s.download();
}

tda_status tda_filtfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b, const double* a,
                        const double* zi, int ntaps, int edge, double* y)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, b); CHECK_PTR(ctx, a); CHECK_PTR(ctx, zi);
    if (n_samples < 1 || edge < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_y, *d_w;
    s.add((void**)&d_x, x, nullptr, (size_t)n_sig * n_samples * 8);
    s.add((void**)&d_y, nullptr, y, (size_t)n_sig * n_samples * 8);
    s.add((void**)&d_w, nullptr, nullptr, (size_t)n_sig * (n_samples + 2 * edge) * 8);
    RET_IF(s.upload());
    RET_IF(tda_filtfilt_dev(ctx, d_x, n_sig, n_samples, b, a, zi, ntaps, edge, d_y, d_w, nullptr));
    return s.download();
}

tda_status tda_upfirdn(tda_ctx* ctx, const double* x, long long n_in, const double* h, int len_h, int up, int down,
                       long long n_pre_remove, long long n_out, double* y)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, h); CHECK_PTR(ctx, y);
    if (n_in < 1 || n_out < 1 || len_h < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_h, *d_y;
    s.add((void**)&d_x, x, nullptr, (size_t)n_in * 8);
    s.add((void**)&d_h, h, nullptr, (size_t)len_h * 8);
    s.add((void**)&d_y, nullptr, y, (size_t)n_out * 8);
    RET_IF(s.upload());
    RET_IF(tda_upfirdn_dev(ctx, d_x, n_in, d_h, len_h, up, down, n_pre_remove, n_out, d_y, nullptr));
    return s.download();
}

tda_status tda_hilbert_envelope(tda_ctx* ctx, const double* x, int n, const double* g, double* env)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, g); CHECK_PTR(ctx, env);
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_g, *d_e;
    s.add((void**)&d_x, x, nullptr, (size_t)n * 8);
    s.add((void**)&d_g, g, nullptr, (size_t)n * 8);
    s.add((void**)&d_e, nullptr, env, (size_t)n * 8);
    RET_IF(s.upload());
    RET_IF(tda_hilbert_envelope_dev(ctx, d_x, n, d_g, d_e, nullptr));
    return s.download();
}

tda_status tda_tau_batch(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int* tau)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau);
    if (n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double* d_win; int* d_tau;
    s.add((void**)&d_win, win, nullptr, (size_t)n_win * n_t * 8);
    s.add((void**)&d_tau, nullptr, tau, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_tau_batch_dev(ctx, d_win, n_win, n_t, max_lag, d_tau, nullptr));
    return s.download();
}

tda_status tda_features_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, double* feat)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm);
    if (n_dgm == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, feat);
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dgm, *d_feat; int* d_cnt;
    s.add((void**)&d_dgm, dgm, nullptr, (size_t)n_dgm * cap * 16);
    s.add((void**)&d_cnt, cnt, nullptr, (size_t)n_dgm * 4);
    s.add((void**)&d_feat, nullptr, feat, (size_t)n_dgm * TDA_N_FEATURES * 8);
    RET_IF(s.upload());
    RET_IF(tda_features_batch_dev(ctx, d_dgm, d_cnt, n_dgm, cap, d_feat, nullptr));
    return s.download();
}

tda_status tda_aggregate_batch(tda_ctx* ctx, const double* feat_h0, const double* feat_h1, const int* seg_off,
                               int n_seg, int n_total, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg); CHECK_NONNEG(ctx, n_total);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, feat_h0); CHECK_PTR(ctx, feat_h1); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d0, *d1, *d_out; int* d_off;
    s.add((void**)&d0, feat_h0, nullptr, (size_t)n_total * TDA_N_FEATURES * 8);
    s.add((void**)&d1, feat_h1, nullptr, (size_t)n_total * TDA_N_FEATURES * 8);
    s.add((void**)&d_off, seg_off, nullptr, (size_t)(n_seg + 1) * 4);
    s.add((void**)&d_out, nullptr, out, (size_t)n_seg * 4 * TDA_N_FEATURES * 8);
    RET_IF(s.upload());
    RET_IF(tda_aggregate_batch_dev(ctx, d0, d1, d_off, n_seg, d_out, nullptr));
    return s.download();
}

tda_status tda_segment_nanmean(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg, int n_total, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg); CHECK_NONNEG(ctx, n_total);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_out; int* d_off;
    s.add((void**)&d_x, x, nullptr, (size_t)n_total * 8);
    s.add((void**)&d_off, seg_off, nullptr, (size_t)(n_seg + 1) * 4);
    s.add((void**)&d_out, nullptr, out, (size_t)n_seg * 8);
    RET_IF(s.upload());
    RET_IF(tda_segment_nanmean_dev(ctx, d_x, d_off, n_seg, d_out, nullptr));
    return s.download();
}

tda_status tda_spearman_batch(tda_ctx* ctx, const double* x, const double* y, int n_total, int ld, const int* cols,
                              int n_cols, const int* seg_off, int n_seg, double* r)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, cols); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, r);
    if (n_total < 1 || ld < 1 || n_cols < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_x, *d_y, *d_r; int *d_c, *d_o;
    s.add((void**)&d_x, x, nullptr, (size_t)n_total * ld * 8);
    s.add((void**)&d_y, y, nullptr, (size_t)n_total * ld * 8);
    s.add((void**)&d_c, cols, nullptr, (size_t)n_cols * 4);
    s.add((void**)&d_o, seg_off, nullptr, (size_t)(n_seg + 1) * 4);
    s.add((void**)&d_r, nullptr, r, (size_t)n_seg * n_cols * 8);
    RET_IF(s.upload());
    RET_IF(tda_spearman_batch_dev(ctx, d_x, d_y, ld, d_c, n_cols, d_o, n_seg, d_r, nullptr));
    return s.download();
}

tda_status tda_temporal_corr_batch(tda_ctx* ctx, const double* fa, const double* fe, int n_total, int ld, const int* cols,
                                   int n_cols, const int* seg_off, int n_seg, const int* status_b, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, fa); CHECK_PTR(ctx, fe); CHECK_PTR(ctx, cols); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    if (n_total < 1 || ld < 1 || n_cols < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    for (int c = 0; c < n_cols; ++c)
        if (cols[c] < 0 || cols[c] >= ld) TDA_FAIL(ctx, TDA_ERR_INVALID, "column index out of range");
    if (seg_off[0] != 0 || seg_off[n_seg] != n_total) TDA_FAIL(ctx, TDA_ERR_INVALID, "seg_off must run from 0 to n_total");
    for (int g = 0; g < n_seg; ++g)
        if (seg_off[g + 1] < seg_off[g]) TDA_FAIL(ctx, TDA_ERR_INVALID, "seg_off must not decrease");
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_a, *d_e, *d_out; int *d_c, *d_o, *d_st = nullptr;
    s.add((void**)&d_a, fa, nullptr, (size_t)n_total * ld * 8);
    s.add((void**)&d_e, fe, nullptr, (size_t)n_total * ld * 8);
    s.add((void**)&d_c, cols, nullptr, (size_t)n_cols * 4);
    s.add((void**)&d_o, seg_off, nullptr, (size_t)(n_seg + 1) * 4);
    if (status_b) s.add((void**)&d_st, status_b, nullptr, (size_t)n_total * 4);
    s.add((void**)&d_out, nullptr, out, (size_t)n_seg * 2 * n_cols * 8);
    RET_IF(s.upload());
    RET_IF(tda_temporal_corr_dev(ctx, d_a, d_e, ld, d_c, n_cols, d_o, n_seg, d_st, d_out, nullptr));
    return s.download();
}

// The host-pointer twins of the pair distances from their own argument checks on: pointer and size checks, the pair
// indices, staging (with the direction table when dirs is given) and `dev`, a call of the _dev entry point on the staged
// PairDev pointers.
struct PairDev { double *a, *b, *dirs = nullptr, *out; int *ca, *cb, *ia = nullptr, *ib = nullptr, *st; };

extern "C++" {                      // (a template inside the extern "C" block of the ABI)
template <class Dev>
static tda_status pair_batch_host(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a, const double* dgm_b,
                                  const int* cnt_b, int n_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs,
                                  const double* dirs, int n_dirs, double* out, int* status, Dev dev)
{
    if (n_pairs == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); CHECK_PTR(ctx, out);
    CHECK_PTR(ctx, status);
    if (n_a < 1 || n_b < 1 || cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    for (int i = 0; i < n_pairs; ++i) {
        const int a = idx_a ? idx_a[i] : i, b = idx_b ? idx_b[i] : i;
        if (a < 0 || a >= n_a || b < 0 || b >= n_b) TDA_FAIL(ctx, TDA_ERR_INVALID, "pair index out of range");
    }
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    PairDev d;
    s.add((void**)&d.a, dgm_a, nullptr, (size_t)n_a * cap_a * 16);
    s.add((void**)&d.ca, cnt_a, nullptr, (size_t)n_a * 4);
    s.add((void**)&d.b, dgm_b, nullptr, (size_t)n_b * cap_b * 16);
    s.add((void**)&d.cb, cnt_b, nullptr, (size_t)n_b * 4);
    if (idx_a) s.add((void**)&d.ia, idx_a, nullptr, (size_t)n_pairs * 4);
    if (idx_b) s.add((void**)&d.ib, idx_b, nullptr, (size_t)n_pairs * 4);
    if (dirs) s.add((void**)&d.dirs, dirs, nullptr, (size_t)n_dirs * 16);
    s.add((void**)&d.out, nullptr, out, (size_t)n_pairs * 8);
    s.add((void**)&d.st, nullptr, status, (size_t)n_pairs * 4);
    RET_IF(s.upload());
    RET_IF(dev(d));
    return s.download();
}
}

tda_status tda_wasserstein_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                 const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                 const int* idx_b, int n_pairs, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_wasserstein_batch_dev(ctx, d.a, d.ca, cap_a, d.b, d.cb, cap_b, d.ia, d.ib, n_pairs,
                                                                 d.out, d.st, nullptr); });
}

tda_status tda_bottleneck_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                const int* idx_b, int n_pairs, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_bottleneck_batch_dev(ctx, d.a, d.ca, cap_a, d.b, d.cb, cap_b, d.ia, d.ib, n_pairs,
                                                                d.out, d.st, nullptr); });
}

tda_status tda_wasserstein_q_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                   const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                   const int* idx_b, int n_pairs, int order, int ground, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if ((order != 1 && order != 2) || (ground != TDA_GROUND_L2 && ground != TDA_GROUND_LINF))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "order must be 1 or 2 and ground TDA_GROUND_L2 or TDA_GROUND_LINF");
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_wasserstein_q_batch_dev(ctx, d.a, d.ca, cap_a, d.b, d.cb, cap_b, d.ia, d.ib, n_pairs,
                                                                   order, ground, d.out, d.st, nullptr); });
}

tda_status tda_sliced_wasserstein_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                        const int* idx_b, int n_pairs, const double* dirs, int n_dirs, double* out,
                                        int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_dirs must be 1..TDA_MAX_DIRECTIONS");
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    CHECK_PTR(ctx, dirs);
    for (int k = 0; k < 2 * n_dirs; ++k)
        if (!std::isfinite(dirs[k])) TDA_FAIL(ctx, TDA_ERR_INVALID, "directions must be finite");
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, dirs, n_dirs, out, status,
        [&](const PairDev& d) { return tda_sliced_wasserstein_batch_dev(ctx, d.a, d.ca, cap_a, d.b, d.cb, cap_b, d.ia, d.ib, n_pairs,
                                                                        d.dirs, n_dirs, d.out, d.st, nullptr); });
}

// the parameter checks of the diagram kernels, before anything is staged (the launch repeats them)
static bool diagram_kernel_params_ok(double ninv, int mirror, double scale, int weight, double wc)
{
    return std::isfinite(ninv) && ninv < 0.0 && (mirror == 0 || mirror == 1) && std::isfinite(scale) &&
           (weight == TDA_KW_ONE || weight == TDA_KW_PERS || (weight == TDA_KW_ATAN && std::isfinite(wc)));
}

tda_status tda_diagram_kernel_pairs(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                    const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                    const int* idx_b, int n_pairs, double ninv, int mirror, double scale, int weight, double wc,
                                    double* out, double* kvals, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_b);
    if (!diagram_kernel_params_ok(ninv, mirror, scale, weight, wc))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "ninv finite and < 0, mirror 0 or 1, scale finite, weight TDA_KW_*, wc finite");
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_pairs == 0) return TDA_OK;
    CHECK_PTR(ctx, out); CHECK_PTR(ctx, status);
    if (n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (n_b) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); }
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_a = nullptr, *d_b = nullptr, *d_out, *d_kv = nullptr;
    int *d_ca = nullptr, *d_cb = nullptr, *d_ia = nullptr, *d_ib = nullptr, *d_st;
    if (n_a) { s.add((void**)&d_a, dgm_a, nullptr, (size_t)n_a * cap_a * 16); s.add((void**)&d_ca, cnt_a, nullptr, (size_t)n_a * 4); }
    if (n_b) { s.add((void**)&d_b, dgm_b, nullptr, (size_t)n_b * cap_b * 16); s.add((void**)&d_cb, cnt_b, nullptr, (size_t)n_b * 4); }
    if (idx_a) s.add((void**)&d_ia, idx_a, nullptr, (size_t)n_pairs * 4);
    if (idx_b) s.add((void**)&d_ib, idx_b, nullptr, (size_t)n_pairs * 4);
    s.add((void**)&d_out, nullptr, out, (size_t)n_pairs * 8);
    if (kvals) s.add((void**)&d_kv, nullptr, kvals, (size_t)n_pairs * 24);
    s.add((void**)&d_st, nullptr, status, (size_t)n_pairs * 4);
    RET_IF(s.upload());
    RET_IF(tda_diagram_kernel_pairs_dev(ctx, d_a, d_ca, n_a, cap_a, d_b, d_cb, n_b, cap_b, d_ia, d_ib, n_pairs, ninv, mirror, scale,
                                        weight, wc, d_out, d_kv, d_st, nullptr));
    return s.download();
}

tda_status tda_diagram_kernel_gram(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                   const int* seg_off_a, int n_seg_a, const int* status_a, const double* dgm_b,
                                   const int* cnt_b, int n_b, int cap_b, const int* seg_off_b, int n_seg_b,
                                   const int* status_b, int skip_mask, double ninv, int mirror, double scale, int weight,
                                   double wc, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_seg_a);
    const bool sym = dgm_b == nullptr;
    if (sym) { n_b = n_a; n_seg_b = n_seg_a; }
    CHECK_NONNEG(ctx, n_b); CHECK_NONNEG(ctx, n_seg_b);
    if (!diagram_kernel_params_ok(ninv, mirror, scale, weight, wc))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "ninv finite and < 0, mirror 0 or 1, scale finite, weight TDA_KW_*, wc finite");
    if (cap_a < 1 || (!sym && cap_b < 1)) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if ((!seg_off_a && n_seg_a != n_a) || (!sym && !seg_off_b && n_seg_b != n_b))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_seg_a == 0 || n_seg_b == 0) return TDA_OK;
    CHECK_PTR(ctx, out);
    if (n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (!sym) CHECK_PTR(ctx, cnt_b);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_a = nullptr, *d_b = nullptr, *d_out;
    int *d_ca = nullptr, *d_cb = nullptr, *d_oa = nullptr, *d_ob = nullptr, *d_sa = nullptr, *d_sb = nullptr;
    if (n_a) { s.add((void**)&d_a, dgm_a, nullptr, (size_t)n_a * cap_a * 16); s.add((void**)&d_ca, cnt_a, nullptr, (size_t)n_a * 4); }
    if (seg_off_a) s.add((void**)&d_oa, seg_off_a, nullptr, (size_t)(n_seg_a + 1) * 4);
    if (status_a && n_a) s.add((void**)&d_sa, status_a, nullptr, (size_t)n_a * 4);
    if (!sym) {
        // (an empty second set still needs a non-NULL buffer to be told from the symmetric form: 16 bytes of its own)
        s.add((void**)&d_b, n_b ? dgm_b : nullptr, nullptr, n_b ? (size_t)n_b * cap_b * 16 : 16);
        s.add((void**)&d_cb, n_b ? cnt_b : nullptr, nullptr, n_b ? (size_t)n_b * 4 : 4);
        if (seg_off_b) s.add((void**)&d_ob, seg_off_b, nullptr, (size_t)(n_seg_b + 1) * 4);
        if (status_b && n_b) s.add((void**)&d_sb, status_b, nullptr, (size_t)n_b * 4);
    }
    s.add((void**)&d_out, nullptr, out, (size_t)n_seg_a * n_seg_b * 8);
    RET_IF(s.upload());
    RET_IF(tda_diagram_kernel_gram_dev(ctx, d_a, d_ca, n_a, cap_a, d_oa, n_seg_a, d_sa, d_b, d_cb, n_b, cap_b, d_ob, n_seg_b, d_sb,
                                       skip_mask, ninv, mirror, scale, weight, wc, d_out, nullptr));
    return s.download();
}

// (its own staging, not pair_batch_host: an index outside its set is a status of that pair, not a refusal of the call)
tda_status tda_persistence_fisher_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                        const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                        const int* idx_b, int n_pairs, double ninv, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs); CHECK_NONNEG(ctx, n_a); CHECK_NONNEG(ctx, n_b);
    if (!std::isfinite(ninv) || !(ninv < 0.0)) TDA_FAIL(ctx, TDA_ERR_INVALID, "ninv must be finite and < 0");
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_pairs == 0) return TDA_OK;
    CHECK_PTR(ctx, out); CHECK_PTR(ctx, status);
    if (n_a) { CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); }
    if (n_b) { CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); }
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_a = nullptr, *d_b = nullptr, *d_out;
    int *d_ca = nullptr, *d_cb = nullptr, *d_ia = nullptr, *d_ib = nullptr, *d_st;
    if (n_a) { s.add((void**)&d_a, dgm_a, nullptr, (size_t)n_a * cap_a * 16); s.add((void**)&d_ca, cnt_a, nullptr, (size_t)n_a * 4); }
    if (n_b) { s.add((void**)&d_b, dgm_b, nullptr, (size_t)n_b * cap_b * 16); s.add((void**)&d_cb, cnt_b, nullptr, (size_t)n_b * 4); }
    if (idx_a) s.add((void**)&d_ia, idx_a, nullptr, (size_t)n_pairs * 4);
    if (idx_b) s.add((void**)&d_ib, idx_b, nullptr, (size_t)n_pairs * 4);
    s.add((void**)&d_out, nullptr, out, (size_t)n_pairs * 8);
    s.add((void**)&d_st, nullptr, status, (size_t)n_pairs * 4);
    RET_IF(s.upload());
    RET_IF(tda_persistence_fisher_batch_dev(ctx, d_a, d_ca, n_a, cap_a, d_b, d_cb, n_b, cap_b, d_ia, d_ib, n_pairs, ninv, d_out,
                                            d_st, nullptr));
    return s.download();
}

// (the outputs are staged in both directions: the kernel writes only rows [0, cnt) of a signal's block)
tda_status tda_sublevel_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                              int n_win, int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_t < 1 || n_t > TDA_SL_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [1, TDA_SL_MAX_SAMPLES]");
    if (n_ch < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be >= 1");
    if (cap < TDA_SL_ROWS(n_t)) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= TDA_SL_ROWS(n_t)");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, sig); CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, status);
    // the elements of sig the tables reach
    long long n_el = (long long)n_win * n_ch * n_t;
    if (win_start) {
        n_el = 0;
        for (int w = 0; w < n_win; ++w) {
            if (win_start[w] < 0 || win_ld[w] < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative window table entry");
            const long long end = win_start[w] + (long long)(n_ch - 1) * win_ld[w] + n_t;
            n_el = end > n_el ? end : n_el;
        }
    }
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    const size_t n_sig = (size_t)n_win * n_ch;
    double *d_sig, *d_dgm;
    long long *d_ws = nullptr, *d_wl = nullptr;
    int *d_cnt, *d_idx = nullptr, *d_st;
    s.add((void**)&d_sig, sig, nullptr, (size_t)n_el * 8);
    if (win_start) { s.add((void**)&d_ws, win_start, nullptr, (size_t)n_win * 8); s.add((void**)&d_wl, win_ld, nullptr, (size_t)n_win * 8); }
    s.add((void**)&d_dgm, dgm, dgm, n_sig * cap * 16);
    if (idx) s.add((void**)&d_idx, idx, idx, n_sig * cap * 8);
    s.add((void**)&d_cnt, nullptr, cnt, n_sig * 4);
    s.add((void**)&d_st, nullptr, status, n_sig * 4);
    RET_IF(s.upload());
    RET_IF(tda_sublevel_batch_dev(ctx, d_sig, d_ws, d_wl, n_win, n_ch, n_t, d_dgm, cap, d_cnt, d_idx, d_st, nullptr));
    return s.download();
}

// The host form shared by tda_plv_dist_batch and tda_connectivity_dist_batch: the limits (before anything is staged), the
// elements of sig the tables reach, the staging; dev(d_sig, d_ws, d_wl, d_g, d_dist, d_mat, d_st) enqueues the _dev form.
extern "C++" {
template <class Dev>
static tda_status window_dist_host(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                   int n_win, int n_ch, int n_t, const double* g, int method, double* dist, double* mat,
                                   int* status, Dev dev)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_ch < 2 || n_ch > TDA_PLV_MAX_CHANNELS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be in [2, TDA_PLV_MAX_CHANNELS]");
    if (n_t < 2 || n_t > TDA_PLV_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [2, TDA_PLV_MAX_SAMPLES]");
    if (method < 0 || method > 3) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown method");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, sig); CHECK_PTR(ctx, g); CHECK_PTR(ctx, dist); CHECK_PTR(ctx, status);
    // the elements of sig the tables reach
    long long n_el = (long long)n_win * n_ch * n_t;
    if (win_start) {
        n_el = 0;
        for (int w = 0; w < n_win; ++w) {
            if (win_start[w] < 0 || win_ld[w] < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative window table entry");
            const long long end = win_start[w] + (long long)(n_ch - 1) * win_ld[w] + n_t;
            n_el = end > n_el ? end : n_el;
        }
    }
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    const size_t nn = (size_t)n_win * n_ch * n_ch;
    double *d_sig, *d_g, *d_dist, *d_mat = nullptr;
    long long *d_ws = nullptr, *d_wl = nullptr;
    int* d_st;
    s.add((void**)&d_sig, sig, nullptr, (size_t)n_el * 8);
    s.add((void**)&d_g, g, nullptr, (size_t)n_t * 8);
    if (win_start) { s.add((void**)&d_ws, win_start, nullptr, (size_t)n_win * 8); s.add((void**)&d_wl, win_ld, nullptr, (size_t)n_win * 8); }
    s.add((void**)&d_dist, nullptr, dist, nn * 8);
    if (mat) s.add((void**)&d_mat, nullptr, mat, nn * 8);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(dev(d_sig, d_ws, d_wl, d_g, d_dist, d_mat, d_st));
    return s.download();
}
}   // extern "C++"

tda_status tda_plv_dist_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                              int n_win, int n_ch, int n_t, const double* g, int method, double* dist, double* plv,
                              int* status)
{
    return window_dist_host(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, plv, status,
        [&](const double* d_sig, const long long* d_ws, const long long* d_wl, const double* d_g, double* d_dist, double* d_plv,
            int* d_st) {
            return tda_plv_dist_batch_dev(ctx, d_sig, d_ws, d_wl, n_win, n_ch, n_t, d_g, method, d_dist, d_plv, d_st, nullptr);
        });
}

tda_status tda_connectivity_dist_batch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                       int n_win, int n_ch, int n_t, const double* g, int measure, int method, double* dist,
                                       double* value, int* status)
{
    CHECK_CTX(ctx);
    if (measure < 0 || measure > TDA_CONN_AEC) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown measure");
    return window_dist_host(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, value, status,
        [&](const double* d_sig, const long long* d_ws, const long long* d_wl, const double* d_g, double* d_dist, double* d_value,
            int* d_st) {
            return tda_connectivity_dist_batch_dev(ctx, d_sig, d_ws, d_wl, n_win, n_ch, n_t, d_g, measure, method, d_dist,
                                                   d_value, d_st, nullptr);
        });
}

// (the limits are checked before anything is staged; of the last row of D only its n entries are copied)
tda_status tda_perm_sums_batch(tda_ctx* ctx, const double* D, int n_mat, int n, int ld, const unsigned long long* lab,
                               int n_perm, double* out, int* n1)
{
    CHECK_CTX(ctx);
    if (n < 2 || n > TDA_PT_MAX_ITEMS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [2, TDA_PT_MAX_ITEMS]");
    if (n_perm < 1 || n_perm > TDA_PT_MAX_PERM) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_perm must be in [1, TDA_PT_MAX_PERM]");
    if (n_mat < 0 || n_mat > TDA_PT_MAX_MATRICES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_mat must be in [0, TDA_PT_MAX_MATRICES]");
    if (ld < n) TDA_FAIL(ctx, TDA_ERR_INVALID, "ld must be >= n");
    CHECK_PTR(ctx, lab);
    if (n_mat) { CHECK_PTR(ctx, D); CHECK_PTR(ctx, out); }
    if (n_mat == 0 && !n1) return TDA_OK;
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    const long long wd = TDA_PT_WORK_DOUBLES(n_mat, n, n_perm);
    double *d_D = nullptr, *d_work = nullptr, *d_out = nullptr;
    unsigned long long* d_lab;
    int* d_n1 = nullptr;
    if (n_mat) {
        s.add((void**)&d_D, D, nullptr, (((size_t)n_mat * n - 1) * ld + n) * 8);
        s.add((void**)&d_work, nullptr, nullptr, (size_t)wd * 8);
        s.add((void**)&d_out, nullptr, out, (size_t)n_mat * 3 * n_perm * 8);
    }
    s.add((void**)&d_lab, lab, nullptr, (size_t)TDA_PT_WORDS(n_perm) * n * 8);
    if (n1) s.add((void**)&d_n1, nullptr, n1, (size_t)n_perm * 4);
    RET_IF(s.upload());
    RET_IF(tda_perm_sums_batch_dev(ctx, d_D, n_mat, n, ld, d_lab, n_perm, d_work, wd, d_out, d_n1, nullptr));
    return s.download();
}

tda_status tda_landscape_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, const double* grid,
                               int n_grid, int n_levels, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm);
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= 1");
    if (n_levels < 1 || n_levels > TDA_MAX_LANDSCAPES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_levels must be 1..TDA_MAX_LANDSCAPES");
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be 1..TDA_MAX_GRID");
    if (n_dgm == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, out);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dgm, *d_grid, *d_out; int* d_cnt;
    s.add((void**)&d_dgm, dgm, nullptr, (size_t)n_dgm * cap * 16);
    s.add((void**)&d_cnt, cnt, nullptr, (size_t)n_dgm * 4);
    s.add((void**)&d_grid, grid, nullptr, (size_t)n_grid * 8);
    s.add((void**)&d_out, nullptr, out, (size_t)n_dgm * (n_levels + 1) * n_grid * 8);
    RET_IF(s.upload());
    RET_IF(tda_landscape_mean_dev(ctx, d_dgm, d_cnt, cap, n_dgm, nullptr, n_dgm, nullptr, 0, d_grid, n_grid, n_levels, d_out,
                                  nullptr));
    return s.download();
}

// (the limits of launch_euler, checked before anything is staged)
#define EULER_LIMITS(ctx, n_grid, max_dim)                                                                             \
    do {                                                                                                               \
        if ((n_grid) < 1 || (n_grid) > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]"); \
        if ((max_dim) < 1 || (max_dim) > TDA_EC_MAX_DIM)                                                               \
            TDA_FAIL(ctx, TDA_ERR_INVALID, "max_dim must be in [1, TDA_EC_MAX_DIM]");                                  \
    } while (0)

tda_status tda_euler_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                              const double* grid, int n_grid, int max_dim, int* counts, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n < 1 || n > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [1, TDA_MAX_POINTS]");
    EULER_LIMITS(ctx, n_grid, max_dim);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dm, *d_grid; int *d_cnt, *d_st;
    s.add((void**)&d_dm, dm, nullptr, (size_t)n_win * n * n * 8);
    s.add((void**)&d_grid, grid, nullptr, (size_t)n_grid * 8);
    s.add((void**)&d_cnt, nullptr, counts, (size_t)n_win * (max_dim + 2) * n_grid * 4);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_euler_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, d_grid, n_grid, max_dim, d_cnt, d_st, nullptr));
    return s.download();
}

tda_status tda_euler_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                 int normalise, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                 int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
    if (p_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "p_cap must be >= 1");
    EULER_LIMITS(ctx, n_grid, max_dim);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_pc, *d_grid; int *d_n, *d_cnt, *d_st;
    s.add((void**)&d_pc, pc, nullptr, (size_t)n_win * p_cap * dim * 8);
    s.add((void**)&d_n, n_pts, nullptr, (size_t)n_win * 4);
    s.add((void**)&d_grid, grid, nullptr, (size_t)n_grid * 8);
    s.add((void**)&d_cnt, nullptr, counts, (size_t)n_win * (max_dim + 2) * n_grid * 4);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_euler_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, d_grid, n_grid, max_dim, d_cnt,
                                     d_st, nullptr));
    return s.download();
}

tda_status tda_euler_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                  int subsample, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                  int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
    if (n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be >= 1");
    EULER_LIMITS(ctx, n_grid, max_dim);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_win, *d_grid; int *d_tau, *d_cnt, *d_np = nullptr, *d_st;
    s.add((void**)&d_win, win, nullptr, (size_t)n_win * n_t * 8);
    s.add((void**)&d_tau, tau, nullptr, (size_t)n_win * 4);
    s.add((void**)&d_grid, grid, nullptr, (size_t)n_grid * 8);
    s.add((void**)&d_cnt, nullptr, counts, (size_t)n_win * (max_dim + 2) * n_grid * 4);
    if (n_points) s.add((void**)&d_np, nullptr, n_points, (size_t)n_win * 4);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_euler_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, d_grid, n_grid, max_dim, d_cnt,
                                      d_np, d_st, nullptr));
    return s.download();
}

tda_status tda_euler_mean(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off, int n_seg,
                          const int* status_in, int skip_mask, double* mean)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    EULER_LIMITS(ctx, n_grid, max_dim);
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    if (n_win) CHECK_PTR(ctx, counts);
    CHECK_PTR(ctx, mean);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    const size_t rg = (size_t)(max_dim + 2) * n_grid;
    int *d_cnt, *d_off = nullptr, *d_si = nullptr; double* d_mean;
    s.add((void**)&d_cnt, counts, nullptr, (size_t)n_win * rg * 4);
    if (seg_off) s.add((void**)&d_off, seg_off, nullptr, ((size_t)n_seg + 1) * 4);
    if (status_in) s.add((void**)&d_si, status_in, nullptr, (size_t)n_win * 4);
    s.add((void**)&d_mean, nullptr, mean, (size_t)n_seg * rg * 8);
    RET_IF(s.upload());
    RET_IF(tda_euler_mean_dev(ctx, d_cnt, n_win, max_dim, n_grid, d_off, n_seg, d_si, skip_mask, d_mean, nullptr));
    return s.download();
}

// (the limits of launch_generators, checked before anything is staged)
#define GEN_LIMITS(ctx)                                                                                                \
    do {                                                                                                               \
        if (cyc_cap < 4 || cyc_cap > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "cyc_cap must be in [4, TDA_MAX_POINTS]"); \
        if (h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");                                         \
        if (part && !cyc) TDA_FAIL(ctx, TDA_ERR_INVALID, "part is summed over the cycles: it needs cyc");              \
        if (h0_edge && (!h0 || !h0_cnt || h0_cap < 1))                                                                 \
            TDA_FAIL(ctx, TDA_ERR_INVALID, "h0_edge needs the H0 rows: h0, h0_cnt and h0_cap >= 1");                   \
    } while (0)

// the device twins of the row inputs and outputs of a host call
struct GenStage {
    double *h0 = nullptr, *h1 = nullptr, *part = nullptr;
    int *h0_cnt = nullptr, *h1_cnt = nullptr, *rips_status = nullptr, *h1_flag = nullptr, *cyc_len = nullptr, *work = nullptr;
    short *h1_gen = nullptr, *cyc = nullptr, *h0_edge = nullptr;
    void add(Stage& s, size_t nw, int part_ld, GEN_PARAMS)
    {
        (void)skip_mask;
        if (h0 && h0_cnt) {
            s.add((void**)&this->h0, h0, nullptr, nw * h0_cap * 16);
            s.add((void**)&this->h0_cnt, h0_cnt, nullptr, nw * 4);
        }
        s.add((void**)&this->h1, h1, nullptr, nw * h1_cap * 16);
        s.add((void**)&this->h1_cnt, h1_cnt, nullptr, nw * 4);
        if (rips_status) s.add((void**)&this->rips_status, rips_status, nullptr, nw * 4);
        s.add((void**)&this->h1_gen, nullptr, h1_gen, nw * h1_cap * 8);
        s.add((void**)&this->h1_flag, nullptr, h1_flag, nw * h1_cap * 4);
        if (cyc) s.add((void**)&this->cyc, nullptr, cyc, nw * h1_cap * cyc_cap * 2);
        s.add((void**)&this->cyc_len, nullptr, cyc_len, nw * h1_cap * 4);
        if (part) s.add((void**)&this->part, nullptr, part, nw * part_ld * 8);
        if (h0_edge) s.add((void**)&this->h0_edge, nullptr, h0_edge, nw * h0_cap * 4);
        if (work) s.add((void**)&this->work, nullptr, work, nw * 8 * 4);
    }
};
#define GEN_STAGED(d) d.h0, h0_cap, d.h0_cnt, d.h1, h1_cap, d.h1_cnt, d.rips_status, skip_mask, cyc_cap, d.h1_gen, d.h1_flag, \
                      d.cyc, d.cyc_len, d.part, d.h0_edge, d.work

tda_status tda_generators_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                   GEN_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n < 1 || n > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [1, TDA_MAX_POINTS]");
    GEN_LIMITS(ctx);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); GEN_CHECK_PTRS(ctx);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    GenStage d;
    double* d_dm; int* d_st;
    s.add((void**)&d_dm, dm, nullptr, (size_t)n_win * n * n * 8);
    d.add(s, (size_t)n_win, n, GEN_PASS);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_generators_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, GEN_STAGED(d), d_st, nullptr));
    return s.download();
}

tda_status tda_generators_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                      int normalise, double thresh, GEN_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
    if (p_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "p_cap must be >= 1");
    GEN_LIMITS(ctx);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); GEN_CHECK_PTRS(ctx);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    GenStage d;
    double* d_pc; int *d_n, *d_st;
    s.add((void**)&d_pc, pc, nullptr, (size_t)n_win * p_cap * dim * 8);
    s.add((void**)&d_n, n_pts, nullptr, (size_t)n_win * 4);
    d.add(s, (size_t)n_win, p_cap, GEN_PASS);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_generators_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, GEN_STAGED(d), d_st, nullptr));
    return s.download();
}

tda_status tda_generators_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                       int subsample, double thresh, GEN_PARAMS, int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
    if (n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be >= 1");
    GEN_LIMITS(ctx);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); GEN_CHECK_PTRS(ctx);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    GenStage d;
    double* d_win; int *d_tau, *d_np = nullptr, *d_st;
    s.add((void**)&d_win, win, nullptr, (size_t)n_win * n_t * 8);
    s.add((void**)&d_tau, tau, nullptr, (size_t)n_win * 4);
    d.add(s, (size_t)n_win, TDA_MAX_POINTS, GEN_PASS);
    if (n_points) s.add((void**)&d_np, nullptr, n_points, (size_t)n_win * 4);
    s.add((void**)&d_st, nullptr, status, (size_t)n_win * 4);
    RET_IF(s.upload());
    RET_IF(tda_generators_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, GEN_STAGED(d), d_np, d_st,
                                           nullptr));
    return s.download();
}

tda_status tda_generators_mean(tda_ctx* ctx, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                               const int* status_in, int skip_mask, double* mean)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be >= 1");
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    if (n_win) CHECK_PTR(ctx, part);
    CHECK_PTR(ctx, mean);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_part, *d_mean; int *d_off = nullptr, *d_si = nullptr;
    s.add((void**)&d_part, part, nullptr, (size_t)n_win * n * 8);
    if (seg_off) s.add((void**)&d_off, seg_off, nullptr, ((size_t)n_seg + 1) * 4);
    if (status_in) s.add((void**)&d_si, status_in, nullptr, (size_t)n_win * 4);
    s.add((void**)&d_mean, nullptr, mean, (size_t)n_seg * n * 8);
    RET_IF(s.upload());
    RET_IF(tda_generators_mean_dev(ctx, d_part, n_win, n, d_off, n_seg, d_si, skip_mask, d_mean, nullptr));
    return s.download();
}

tda_status tda_frechet_mean_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, const int* seg_off,
                                  int n_seg, const int* status_in, int skip_mask, int max_iter, double* mean, int* mean_cnt,
                                  int cap_out, double* var, int* iters, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm); CHECK_NONNEG(ctx, n_seg);
    if (cap < 1 || cap_out < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap and cap_out must be >= 1");
    if (max_iter < 1 || max_iter > TDA_FM_MAX_ITER) TDA_FAIL(ctx, TDA_ERR_INVALID, "max_iter must be 1..TDA_FM_MAX_ITER");
    if (!seg_off && n_seg != n_dgm) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every diagram is a group: n_seg != n_dgm");
    if (n_seg == 0) return TDA_OK;
    if (n_dgm) { CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); }
    CHECK_PTR(ctx, mean); CHECK_PTR(ctx, mean_cnt); CHECK_PTR(ctx, var); CHECK_PTR(ctx, iters); CHECK_PTR(ctx, status);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dgm = nullptr, *d_mean, *d_var; int *d_cnt = nullptr, *d_off = nullptr, *d_sin = nullptr, *d_mc, *d_it, *d_st;
    if (n_dgm) { s.add((void**)&d_dgm, dgm, nullptr, (size_t)n_dgm * cap * 16); s.add((void**)&d_cnt, cnt, nullptr, (size_t)n_dgm * 4); }
    if (seg_off) s.add((void**)&d_off, seg_off, nullptr, (size_t)(n_seg + 1) * 4);
    if (status_in && n_dgm) s.add((void**)&d_sin, status_in, nullptr, (size_t)n_dgm * 4);
    s.add((void**)&d_mean, nullptr, mean, (size_t)n_seg * cap_out * 16);
    s.add((void**)&d_mc, nullptr, mean_cnt, (size_t)n_seg * 4);
    s.add((void**)&d_var, nullptr, var, (size_t)n_seg * 8);
    s.add((void**)&d_it, nullptr, iters, (size_t)n_seg * 4);
    s.add((void**)&d_st, nullptr, status, (size_t)n_seg * 4);
    RET_IF(s.upload());
    RET_IF(tda_frechet_mean_dev(ctx, d_dgm, d_cnt, cap, n_dgm, d_off, n_seg, d_sin, skip_mask, max_iter, d_mean, d_mc, cap_out,
                                d_var, d_it, d_st, nullptr));
    return s.download();
}

static bool image_edges_ok(const double* e, int n)
{
    for (int i = 0; i <= n; ++i)
        if (!std::isfinite(e[i]) || (i && !(e[i] > e[i - 1]))) return false;
    return true;
}

tda_status tda_image_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, const double* xe, int n_x,
                           const double* ye, int n_y, double sigma, int power, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm);
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= 1");
    if (n_x < 1 || n_x > TDA_MAX_IMAGE_SIDE || n_y < 1 || n_y > TDA_MAX_IMAGE_SIDE)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "n_x and n_y must be 1..TDA_MAX_IMAGE_SIDE");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) TDA_FAIL(ctx, TDA_ERR_INVALID, "sigma must be finite and > 0");
    if (power < 0 || power > 2) TDA_FAIL(ctx, TDA_ERR_INVALID, "power must be 0, 1 or 2");
    CHECK_PTR(ctx, xe); CHECK_PTR(ctx, ye);
    if (!image_edges_ok(xe, n_x) || !image_edges_ok(ye, n_y))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "image edges must be finite and strictly ascending");
    if (n_dgm == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, out);
    TDA_HIP(ctx, hipSetDevice(ctx->device));
    Stage s(ctx);
    double *d_dgm, *d_xe, *d_ye, *d_out; int* d_cnt;
    s.add((void**)&d_dgm, dgm, nullptr, (size_t)n_dgm * cap * 16);
    s.add((void**)&d_cnt, cnt, nullptr, (size_t)n_dgm * 4);
    s.add((void**)&d_xe, xe, nullptr, (size_t)(n_x + 1) * 8);
    s.add((void**)&d_ye, ye, nullptr, (size_t)(n_y + 1) * 8);
    s.add((void**)&d_out, nullptr, out, (size_t)n_dgm * n_y * n_x * 8);
    RET_IF(s.upload());
    RET_IF(tda_image_mean_dev(ctx, d_dgm, d_cnt, cap, n_dgm, nullptr, n_dgm, nullptr, 0, d_xe, n_x, d_ye, n_y, sigma, power,
                              d_out, nullptr));
    return s.download();
}

// ---------------------------------------------------------------- timing helpers
tda_status tda_event_create(tda_ctx* ctx, void** ev)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, ev);
    hipEvent_t e;
    TDA_HIP(ctx, hipEventCreate(&e));
    *ev = (void*)e;
    return TDA_OK;
}
tda_status tda_event_record(tda_ctx* ctx, void* ev, void* stream)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, ev);
    TDA_HIP(ctx, hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return TDA_OK;
}
tda_status tda_event_elapsed_ms(tda_ctx* ctx, void* ev_start, void* ev_stop, float* ms)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, ev_start); CHECK_PTR(ctx, ev_stop); CHECK_PTR(ctx, ms);
    TDA_HIP(ctx, hipEventSynchronize((hipEvent_t)ev_stop));
    TDA_HIP(ctx, hipEventElapsedTime(ms, (hipEvent_t)ev_start, (hipEvent_t)ev_stop));
    return TDA_OK;
}
tda_status tda_event_destroy(tda_ctx* ctx, void* ev)
{
    CHECK_CTX(ctx);
    if (ev) TDA_HIP(ctx, hipEventDestroy((hipEvent_t)ev));
    return TDA_OK;
}
tda_status tda_set_kernel_probe(tda_ctx* ctx, int which, void* ev_start, void* ev_stop, void* dev_span)
{
    CHECK_CTX(ctx);
    if (which < TDA_PROBE_NONE || which > TDA_PROBE_CORR_DIST) TDA_FAIL(ctx, TDA_ERR_INVALID, "unknown probe");
    if (which != TDA_PROBE_NONE && !(ev_start && ev_stop) && !dev_span)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "probe needs two events or a span buffer");
    if ((ev_start == nullptr) != (ev_stop == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "probe events come in pairs");
    if (which == TDA_PROBE_NONE) {
        for (int w = 0; w < 4; ++w) ctx->probe[w] = tda_ctx::Probe();
        return TDA_OK;
    }
    ctx->probe[which].start = (hipEvent_t)ev_start;
    ctx->probe[which].stop = (hipEvent_t)ev_stop;
    ctx->probe[which].span = (unsigned long long*)dev_span;
    ctx->probe[which].armed = true;
    return TDA_OK;
}
tda_status tda_stream_sync(tda_ctx* ctx, void* stream)
{
    CHECK_CTX(ctx);
    TDA_HIP(ctx, hipStreamSynchronize((hipStream_t)stream));
    return TDA_OK;
}

}  // extern "C"
#pragma GCC visibility pop
