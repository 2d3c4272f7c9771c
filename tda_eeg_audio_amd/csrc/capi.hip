// capi.hip -- the C ABI of libtdaeeg.so (include/tdaeeg.h): context, argument checks,
// host-pointer twins (stage -> launch -> copy back) and timing helpers.
#include "common.h"
#include "rips_keys_dev.h"
#include <string.h>
#include <cmath>
#include <vector>

static thread_local std::string g_create_err;

#define CHECK_CTX(ctx) do { if (!(ctx)) return TDA_ERR_INVALID; } while (0)
#define CHECK_PTR(ctx, p) do { if (!(p)) TDA_FAIL(ctx, TDA_ERR_INVALID, "null pointer: " #p); } while (0)
#define CHECK_NONNEG(ctx, v) do { if ((v) < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative size: " #v); } while (0)

// ---------------------------------------------------------------- staging of the host-pointer twins
// A bump allocator over the context workspace; everything is staged, launched on the
// default stream, copied back and synchronised.  Sizes are element counts.
namespace {

struct Stage;

// A staged buffer.  It converts to its device pointer where it is used, inside Stage::run, when the workspace has its
// final place; a buffer that was not staged (a null host pointer, no element) converts to nullptr.
template <class T>
struct Dev {
    const Stage* s = nullptr;
    size_t off = 0;
    operator T*() const;
};

struct Stage {
    tda_ctx* ctx;
    size_t need = 0;
    struct Item { size_t off; const void* src; void* dst; size_t bytes; };
    std::vector<Item> items;
    explicit Stage(tda_ctx* c) : ctx(c) {}
    Stage(const Stage&) = delete;

    template <class T> Dev<T> in(const T* host, size_t n) { return add<T>(host, nullptr, host ? n : 0); }    // uploaded
    template <class T> Dev<T> out(T* host, size_t n) { return add<T>(nullptr, host, host ? n : 0); }         // copied back
    template <class T> Dev<T> inout(T* host, size_t n) { return add<T>(host, host, host ? n : 0); }          // both
    template <class T> Dev<T> work(size_t n) { return add<T>(nullptr, nullptr, n); }                         // device only

    // Places the buffers, uploads in the order they were added, calls f (a _dev entry point on the staged buffers) and,
    // only if f succeeded, copies back and synchronises.
    template <class F>
    tda_status run(F f)
    {
        TDA_HIP(ctx, hipSetDevice(ctx->device));
        if (need > ctx->ws_bytes) {
            if (ctx->ws) TDA_HIP(ctx, hipFree(ctx->ws));
            ctx->ws = nullptr; ctx->ws_bytes = 0;
            TDA_HIP(ctx, hipMalloc(&ctx->ws, need));
            ctx->ws_bytes = need;
        }
        char* ws = (char*)ctx->ws;
        for (auto& it : items)
            if (it.src) TDA_HIP(ctx, hipMemcpyAsync(ws + it.off, it.src, it.bytes, hipMemcpyHostToDevice, 0));
        const tda_status st = f();
        if (st != TDA_OK) return st;
        for (auto& it : items)
            if (it.dst) TDA_HIP(ctx, hipMemcpyAsync(it.dst, ws + it.off, it.bytes, hipMemcpyDeviceToHost, 0));
        TDA_HIP(ctx, hipStreamSynchronize(0));
        return TDA_OK;
    }

private:
    template <class T>
    Dev<T> add(const T* src, T* dst, size_t n)
    {
        if (!n) return {};
        const size_t bytes = n * sizeof(T);
        items.push_back({need, src, dst, bytes});
        Dev<T> d{this, need};
        need += (bytes + 255) & ~(size_t)255;
        return d;
    }
};

template <class T>
Dev<T>::operator T*() const { return s ? (T*)((char*)s->ctx->ws + off) : nullptr; }

// a set of diagrams: rows (n, cap, 2) and counts (n)
struct DgmSet { Dev<double> rows; Dev<int> cnt; };
DgmSet dgm_in(Stage& s, const double* rows, const int* cnt, size_t n, int cap)
{
    return {s.in(rows, n * cap * 2), s.in(cnt, n)};
}

// the group inputs of a mean over n items: seg_off (n_seg + 1), or NULL for every item its own group, and the items'
// status words (n), or NULL
struct GroupIn { Dev<int> off, status; };
GroupIn group_in(Stage& s, const int* seg_off, int n_seg, const int* status_in, size_t n)
{
    return {s.in(seg_off, (size_t)n_seg + 1), s.in(status_in, n)};
}

// the outputs of a Rips call on nw windows; n_points may be NULL
struct RipsStage { Dev<double> h0, h1; Dev<int> c0, c1, np, st; };
RipsStage rips_out(Stage& s, size_t nw, double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt, int* n_points,
                   int* status)
{
    return {s.out(h0, nw * h0_cap * 2), s.out(h1, nw * h1_cap * 2), s.out(h0_cnt, nw), s.out(h1_cnt, nw), s.out(n_points, nw),
            s.out(status, nw)};
}

// The elements of sig the window tables reach; without tables, the stacked windows.
tda_status sig_extent(tda_ctx* ctx, const long long* win_start, const long long* win_ld, int n_win, int n_ch, int n_t,
                      long long* n_el)
{
    *n_el = (long long)n_win * n_ch * n_t;
    if (win_start) {
        *n_el = 0;
        for (int w = 0; w < n_win; ++w) {
            if (win_start[w] < 0 || win_ld[w] < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "negative window table entry");
            const long long end = win_start[w] + (long long)(n_ch - 1) * win_ld[w] + n_t;
            *n_el = end > *n_el ? end : *n_el;
        }
    }
    return TDA_OK;
}

// The two sets, the pair indices and the outputs of a call on pairs of diagrams; dirs (the direction table of the sliced
// distance) and kvals (of the diagram kernels) are NULL where the entry point has none.
struct PairDev { DgmSet a, b; Dev<int> ia, ib; Dev<double> dirs, out, kv; Dev<int> st; };
PairDev pair_stage(Stage& s, const double* dgm_a, const int* cnt_a, int n_a, int cap_a, const double* dgm_b, const int* cnt_b,
                   int n_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs, const double* dirs, int n_dirs, double* out,
                   double* kvals, int* status)
{
    return {dgm_in(s, dgm_a, cnt_a, (size_t)n_a, cap_a), dgm_in(s, dgm_b, cnt_b, (size_t)n_b, cap_b), s.in(idx_a, (size_t)n_pairs),
            s.in(idx_b, (size_t)n_pairs), s.in(dirs, (size_t)n_dirs * 2), s.out(out, (size_t)n_pairs),
            s.out(kvals, (size_t)n_pairs * 3), s.out(status, (size_t)n_pairs)};
}

// The host-pointer twins of the pair distances from their own argument checks on: pointer and size checks, the pair
// indices, staging (with the direction table when dirs is given) and `dev`, a call of the _dev entry point on the staged
// PairDev pointers.
template <class Call>
tda_status pair_batch_host(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a, const double* dgm_b,
                           const int* cnt_b, int n_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs,
                           const double* dirs, int n_dirs, double* out, int* status, Call dev)
{
    if (n_pairs == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm_a); CHECK_PTR(ctx, cnt_a); CHECK_PTR(ctx, dgm_b); CHECK_PTR(ctx, cnt_b); CHECK_PTR(ctx, out);
    CHECK_PTR(ctx, status);
    if (n_a < 1 || n_b < 1 || cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    for (int i = 0; i < n_pairs; ++i) {
        const int a = idx_a ? idx_a[i] : i, b = idx_b ? idx_b[i] : i;
        if (a < 0 || a >= n_a || b < 0 || b >= n_b) TDA_FAIL(ctx, TDA_ERR_INVALID, "pair index out of range");
    }
    Stage s(ctx);
    const PairDev d = pair_stage(s, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, dirs, n_dirs, out,
                                 nullptr, status);
    return s.run([&] { return dev(d); });
}

// The host form shared by tda_plv_dist_batch and tda_connectivity_dist_batch: the limits (before anything is staged), the
// elements of sig the tables reach, the staging; dev(d_sig, d_ws, d_wl, d_g, d_dist, d_mat, d_st) enqueues the _dev form.
template <class Call>
tda_status window_dist_host(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                            int n_ch, int n_t, const double* g, int method, double* dist, double* mat, int* status, Call dev)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_ch < 2 || n_ch > TDA_PLV_MAX_CHANNELS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be in [2, TDA_PLV_MAX_CHANNELS]");
    if (n_t < 2 || n_t > TDA_PLV_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [2, TDA_PLV_MAX_SAMPLES]");
    if (method < 0 || method > 3) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown method");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, sig); CHECK_PTR(ctx, g); CHECK_PTR(ctx, dist); CHECK_PTR(ctx, status);
    long long n_el;
    if (tda_status st = sig_extent(ctx, win_start, win_ld, n_win, n_ch, n_t, &n_el)) return st;
    Stage s(ctx);
    const size_t nn = (size_t)n_win * n_ch * n_ch;
    auto d_sig = s.in(sig, (size_t)n_el);
    auto d_g = s.in(g, (size_t)n_t);
    auto d_ws = s.in(win_start, (size_t)n_win);
    auto d_wl = s.in(win_ld, (size_t)n_win);
    auto d_dist = s.out(dist, nn);
    auto d_mat = s.out(mat, nn);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] { return dev(d_sig, d_ws, d_wl, d_g, d_dist, d_mat, d_st); });
}

}   // namespace

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

tda_status tda_ami_batch_dev(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int n_bins, double* ami,
                             int* tau, int* joint, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, ami); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, status); }
    return launch_ami(ctx, win, nullptr, n_win, n_t, max_lag, n_bins, ami, tau, joint, status, nullptr, (hipStream_t)stream);
}

tda_status tda_ami_segments_dev(tda_ctx* ctx, const double* win, const int* seg_off, int n_seg, int n_t, int max_lag,
                                int n_bins, int* tau_seg, int* tau_win, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, tau_seg); }
    return launch_ami(ctx, win, seg_off, n_seg, n_t, max_lag, n_bins, nullptr, tau_seg, nullptr, nullptr, tau_win,
                      (hipStream_t)stream);
}

tda_status tda_fnn_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler,
                             double r_tol, double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn,
                             int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, frac); CHECK_PTR(ctx, dim);
                 CHECK_PTR(ctx, status); }
    return launch_fnn(ctx, win, tau, n_win, n_t, d_max, theiler, r_tol, a_tol, frac_tol, counts, frac, dim, nn, status,
                      (hipStream_t)stream);
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
    return launch_euler(ctx, WinSrc{dm, nullptr, n, 0, 1, 2, symmetrise, 0}, n_win, thresh, grid, n_grid, max_dim, counts,
                        nullptr, status, (hipStream_t)stream);
}

tda_status tda_euler_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                     int normalise, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                     int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status); }
    return launch_euler(ctx, WinSrc{pc, n_pts, p_cap, dim, 1, 1, normalise, 0}, n_win, thresh, grid, n_grid, max_dim, counts,
                        nullptr, status, (hipStream_t)stream);
}

tda_status tda_euler_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                      int subsample, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                      int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status); }
    return launch_euler(ctx, WinSrc{win, tau, n_t, dim, subsample, 0, 1, 0}, n_win, thresh, grid, n_grid, max_dim, counts,
                        n_points, status, (hipStream_t)stream);
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

#define NET_CHECK_PTRS(ctx) do { CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, measures); CHECK_PTR(ctx, status); \
                            } while (0)

tda_status tda_network_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                    const double* grid, int n_grid, int* counts, double* measures, int* nodal, int* status,
                                    void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, dm); NET_CHECK_PTRS(ctx); }
    return launch_network(ctx, WinSrc{dm, nullptr, n, 0, 1, 2, symmetrise, 0}, n_win, thresh, grid, n_grid, counts, measures,
                          nodal, nullptr, status, (hipStream_t)stream);
}

tda_status tda_network_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                       int normalise, double thresh, const double* grid, int n_grid, int* counts,
                                       double* measures, int* nodal, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); NET_CHECK_PTRS(ctx); }
    return launch_network(ctx, WinSrc{pc, n_pts, p_cap, dim, 1, 1, normalise, 0}, n_win, thresh, grid, n_grid, counts, measures,
                          nodal, nullptr, status, (hipStream_t)stream);
}

tda_status tda_network_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                        int subsample, double thresh, const double* grid, int n_grid, int* counts,
                                        double* measures, int* nodal, int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); NET_CHECK_PTRS(ctx); }
    return launch_network(ctx, WinSrc{win, tau, n_t, dim, subsample, 0, 1, 0}, n_win, thresh, grid, n_grid, counts, measures,
                          nodal, n_points, status, (hipStream_t)stream);
}

tda_status tda_network_mean_dev(tda_ctx* ctx, const int* counts, const double* measures, const int* nodal, int n_win,
                                int n_grid, int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                                double* mean_counts, double* mean_measures, double* mean_nodal, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    return launch_network_mean(ctx, counts, measures, nodal, n_win, n_grid, n_node, seg_off, n_seg, status_in, skip_mask,
                               mean_counts, mean_measures, mean_nodal, (hipStream_t)stream);
}

// the parameters that the tda_recurrence_* entry points share behind the grid, in the header's order
#define RQ_PARAMS int theiler, int l_min, int v_min, int* counts, double* measures, int* hist
#define RQ_ARGS theiler, l_min, v_min, counts, measures, hist

tda_status tda_recurrence_dm_batch_dev(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                       const double* grid, int n_grid, RQ_PARAMS, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, dm); NET_CHECK_PTRS(ctx); }
    return launch_recurrence(ctx, WinSrc{dm, nullptr, n, 0, 1, 2, symmetrise, 0}, n_win, thresh, grid, n_grid, RQ_ARGS, nullptr,
                             status, (hipStream_t)stream);
}

tda_status tda_recurrence_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                          int normalise, double thresh, const double* grid, int n_grid, RQ_PARAMS,
                                          int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); NET_CHECK_PTRS(ctx); }
    return launch_recurrence(ctx, WinSrc{pc, n_pts, p_cap, dim, 1, 1, normalise, 0}, n_win, thresh, grid, n_grid, RQ_ARGS,
                             nullptr, status, (hipStream_t)stream);
}

tda_status tda_recurrence_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                           int subsample, double thresh, const double* grid, int n_grid, RQ_PARAMS,
                                           int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); NET_CHECK_PTRS(ctx); }
    return launch_recurrence(ctx, WinSrc{win, tau, n_t, dim, subsample, 0, 1, 0}, n_win, thresh, grid, n_grid, RQ_ARGS,
                             n_points, status, (hipStream_t)stream);
}

tda_status tda_recurrence_mean_dev(tda_ctx* ctx, const int* counts, const double* measures, const int* hist, int n_win,
                                   int n_grid, int n_hist, const int* seg_off, int n_seg, const int* status_in,
                                   int skip_mask, double* mean_counts, double* mean_measures, double* mean_hist,
                                   void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    return launch_recurrence_mean(ctx, counts, measures, hist, n_win, n_grid, n_hist, seg_off, n_seg, status_in, skip_mask,
                                  mean_counts, mean_measures, mean_hist, (hipStream_t)stream);
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
    return launch_generators(ctx, WinSrc{dm, nullptr, n, 0, 1, 2, symmetrise, 0}, n_win, thresh, gen_args(GEN_PASS), nullptr,
                             status, (hipStream_t)stream);
}

tda_status tda_generators_cloud_batch_dev(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                          int normalise, double thresh, GEN_PARAMS, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); GEN_CHECK_PTRS(ctx); }
    return launch_generators(ctx, WinSrc{pc, n_pts, p_cap, dim, 1, 1, normalise, 0}, n_win, thresh, gen_args(GEN_PASS), nullptr,
                             status, (hipStream_t)stream);
}

tda_status tda_generators_takens_batch_dev(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                           int subsample, double thresh, GEN_PARAMS, int* n_points, int* status, void* stream)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win) { CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); GEN_CHECK_PTRS(ctx); }
    return launch_generators(ctx, WinSrc{win, tau, n_t, dim, subsample, 0, 1, 0}, n_win, thresh, gen_args(GEN_PASS), n_points,
                             status, (hipStream_t)stream);
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
// Each one checks its arguments, stages its buffers (Stage, above) and runs its _dev entry point on them.
tda_status tda_corr_dist_batch(tda_ctx* ctx, const double* win, int n_win, int n_ch, int n_t, double* dist, double* corr)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, dist);
    Stage s(ctx);
    const size_t nw = (size_t)n_win;
    auto d_win = s.in(win, nw * n_ch * n_t);
    auto d_dist = s.out(dist, nw * n_ch * n_ch);
    auto d_corr = s.out(corr, nw * n_ch * n_ch);
    return s.run([&] { return tda_corr_dist_batch_dev(ctx, d_win, n_win, n_ch, n_t, d_dist, d_corr, nullptr); });
}

tda_status tda_corr_dist_sliding(tda_ctx* ctx, const double* sig, int n_ch, int n_samples, int win_len, int step,
                                 double* dist, double* corr, int* n_win)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, sig); CHECK_PTR(ctx, dist); CHECK_NONNEG(ctx, n_samples);
    if (win_len < 2 || step < 1 || n_ch < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad window geometry");
    const int nw = n_samples >= win_len ? (n_samples - win_len) / step + 1 : 0;
    if (n_win) *n_win = nw;
    if (nw == 0) return TDA_OK;
    Stage s(ctx);
    auto d_sig = s.in(sig, (size_t)n_ch * n_samples);
    auto d_dist = s.out(dist, (size_t)nw * n_ch * n_ch);
    auto d_corr = s.out(corr, (size_t)nw * n_ch * n_ch);
    return s.run([&] {
        return tda_corr_dist_sliding_dev(ctx, d_sig, n_ch, n_samples, win_len, step, d_dist, d_corr, nullptr, nullptr);
    });
}

tda_status tda_corr_to_dist_batch(tda_ctx* ctx, const double* corr, int n_win, int n, int method, double* dist)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, corr); CHECK_PTR(ctx, dist);
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be >= 1");
    Stage s(ctx);
    auto d_c = s.in(corr, (size_t)n_win * n * n);
    auto d_d = s.out(dist, (size_t)n_win * n * n);
    return s.run([&] { return tda_corr_to_dist_batch_dev(ctx, d_c, n_win, n, method, d_d, nullptr); });
}

tda_status tda_rips_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                             double* h0, int h0_cap, int* h0_cnt, double* h1, int h1_cap, int* h1_cnt, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); CHECK_PTR(ctx, h0); CHECK_PTR(ctx, h0_cnt); CHECK_PTR(ctx, h1); CHECK_PTR(ctx, h1_cnt);
    CHECK_PTR(ctx, status);
    if (h0_cap < 1 || h1_cap < 1 || n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n, h0_cap, h1_cap must be >= 1");
    Stage s(ctx);
    const size_t nw = (size_t)n_win;
    auto d_dm = s.in(dm, nw * n * n);
    const RipsStage o = rips_out(s, nw, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, nullptr, status);
    return s.run([&] {
        return tda_rips_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, o.h0, h0_cap, o.c0, o.h1, h1_cap, o.c1, o.st, nullptr);
    });
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
    Stage s(ctx);
    const size_t nw = (size_t)n_win;
    auto d_win = s.in(win, nw * n_t);
    auto d_tau = s.in(tau, nw);
    const RipsStage o = rips_out(s, nw, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, n_points, status);
    return s.run([&] {
        return tda_takens_rips_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, o.h0, h0_cap, o.c0, o.h1, h1_cap,
                                         o.c1, o.np, o.st, nullptr);
    });
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
    Stage s(ctx);
    const size_t nw = (size_t)n_win;
    auto d_pc = s.in(pc, nw * p_cap * dim);
    auto d_n = s.in(n_pts, nw);
    const RipsStage o = rips_out(s, nw, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, nullptr, status);
    return s.run([&] {
        return tda_cloud_rips_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, o.h0, h0_cap, o.c0, o.h1, h1_cap, o.c1,
                                        o.st, nullptr);
    });
}

namespace {
// The landmark outputs of a host call: staged in BOTH directions, so what the kernel leaves untouched stays the caller's.
struct LmStage {
    Dev<double> lm, lambda, rc; Dev<int> idx, n_lm, n_full;
    void add(Stage& s, int n_win, int n_perm, int dim, double* h_lm, int* h_idx, double* h_lambda, double* h_rc, int* h_nlm,
             int* h_nfull)
    {
        const size_t nw = (size_t)n_win;
        lm = s.inout(h_lm, nw * n_perm * dim);
        idx = s.inout(h_idx, nw * n_perm);
        lambda = s.inout(h_lambda, nw * n_perm);
        rc = s.inout(h_rc, nw);
        n_lm = s.inout(h_nlm, nw);
        n_full = s.inout(h_nfull, nw);
    }
};
}   // namespace
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
    Stage s(ctx);
    LmStage o;
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.in(tau, (size_t)n_win);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    return s.run([&] {
        return tda_takens_landmarks_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, n_perm, o.lm, o.idx, o.lambda, o.rc, o.n_lm,
                                        o.n_full, nullptr);
    });
}

tda_status tda_cloud_landmarks(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                               int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                               double* r_cover, int* n_lm, int* n_full)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    CHECK_LM_LIMITS(ctx, p_cap >= 1 && p_cap <= TDA_LM_MAX_POINTS);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_LM_PTRS(ctx);
    Stage s(ctx);
    LmStage o;
    auto d_pc = s.in(pc, (size_t)n_win * p_cap * dim);
    auto d_n = s.in(n_pts, (size_t)n_win);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    return s.run([&] {
        return tda_cloud_landmarks_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, n_perm, o.lm, o.idx, o.lambda, o.rc, o.n_lm,
                                       o.n_full, nullptr);
    });
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
    Stage s(ctx);
    LmStage o;
    const size_t nw = (size_t)n_win;
    auto d_win = s.in(win, nw * n_t);
    auto d_tau = s.in(tau, nw);
    o.add(s, n_win, n_perm, dim, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full);
    const RipsStage r = rips_out(s, nw, h0, h0_cap, h0_cnt, h1, h1_cap, h1_cnt, n_points, status);
    return s.run([&] {
        return tda_takens_rips_landmarks_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, n_perm, thresh, o.lm, o.idx, o.lambda,
                                             o.rc, o.n_lm, o.n_full, r.h0, h0_cap, r.c0, r.h1, h1_cap, r.c1, r.np, r.st, nullptr);
    });
}

tda_status tda_sosfiltfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* sos, const double* zi,
                           int n_sections, int edge, double* y)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, sos); CHECK_PTR(ctx, zi);
    if (n_samples < 1 || edge < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n_sig * n_samples);
    auto d_y = s.out(y, (size_t)n_sig * n_samples);
    auto d_w = s.work<double>((size_t)n_sig * (n_samples + 2 * edge));
    return s.run([&] { return tda_sosfiltfilt_dev(ctx, d_x, n_sig, n_samples, sos, zi, n_sections, edge, d_y, d_w, nullptr); });
}

tda_status tda_filtfilt(tda_ctx* ctx, const double* x, int n_sig, int n_samples, const double* b, const double* a,
                        const double* zi, int ntaps, int edge, double* y)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_sig);
    if (n_sig == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, b); CHECK_PTR(ctx, a); CHECK_PTR(ctx, zi);
    if (n_samples < 1 || edge < 0) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n_sig * n_samples);
    auto d_y = s.out(y, (size_t)n_sig * n_samples);
    auto d_w = s.work<double>((size_t)n_sig * (n_samples + 2 * edge));
    return s.run([&] { return tda_filtfilt_dev(ctx, d_x, n_sig, n_samples, b, a, zi, ntaps, edge, d_y, d_w, nullptr); });
}

tda_status tda_upfirdn(tda_ctx* ctx, const double* x, long long n_in, const double* h, int len_h, int up, int down,
                       long long n_pre_remove, long long n_out, double* y)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, h); CHECK_PTR(ctx, y);
    if (n_in < 1 || n_out < 1 || len_h < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n_in);
    auto d_h = s.in(h, (size_t)len_h);
    auto d_y = s.out(y, (size_t)n_out);
    return s.run([&] { return tda_upfirdn_dev(ctx, d_x, n_in, d_h, len_h, up, down, n_pre_remove, n_out, d_y, nullptr); });
}

tda_status tda_hilbert_envelope(tda_ctx* ctx, const double* x, int n, const double* g, double* env)
{
    CHECK_CTX(ctx); CHECK_PTR(ctx, x); CHECK_PTR(ctx, g); CHECK_PTR(ctx, env);
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "bad sizes");
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n);
    auto d_g = s.in(g, (size_t)n);
    auto d_e = s.out(env, (size_t)n);
    return s.run([&] { return tda_hilbert_envelope_dev(ctx, d_x, n, d_g, d_e, nullptr); });
}

tda_status tda_tau_batch(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int* tau)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau);
    if (n_t < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be >= 1");
    Stage s(ctx);
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.out(tau, (size_t)n_win);
    return s.run([&] { return tda_tau_batch_dev(ctx, d_win, n_win, n_t, max_lag, d_tau, nullptr); });
}

tda_status tda_ami_batch(tda_ctx* ctx, const double* win, int n_win, int n_t, int max_lag, int n_bins, double* ami, int* tau,
                         int* joint, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    int lag = max_lag;                                             // resolved: the rows of ami and joint have lag + 1 entries
    TDA_TRY(ami_check(ctx, n_t, n_bins, &lag));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, ami); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, status);
    Stage s(ctx);
    const size_t nw = (size_t)n_win, nl = (size_t)lag + 1;
    auto d_win = s.in(win, nw * n_t);
    auto d_ami = s.out(ami, nw * nl);
    auto d_tau = s.out(tau, nw);
    auto d_joint = s.out(joint, nw * nl * n_bins * n_bins);
    auto d_st = s.out(status, nw);
    return s.run([&] { return tda_ami_batch_dev(ctx, d_win, n_win, n_t, max_lag, n_bins, d_ami, d_tau, d_joint, d_st, nullptr); });
}

tda_status tda_fnn_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler,
                         double r_tol, double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(fnn_check(ctx, n_t, d_max, theiler, r_tol, a_tol, frac_tol));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, frac); CHECK_PTR(ctx, dim);
    CHECK_PTR(ctx, status);
    Stage s(ctx);
    const size_t nw = (size_t)n_win;
    auto d_win = s.in(win, nw * n_t);
    auto d_tau = s.in(tau, nw);
    auto d_cnt = s.out(counts, nw * d_max * TDA_FNN_COLS);
    auto d_frac = s.out(frac, nw * d_max);
    auto d_dim = s.out(dim, nw);
    auto d_nn = s.out(nn, nw * d_max * n_t);
    auto d_st = s.out(status, nw);
    return s.run([&] {
        return tda_fnn_batch_dev(ctx, d_win, d_tau, n_win, n_t, d_max, theiler, r_tol, a_tol, frac_tol, d_cnt, d_frac, d_dim, d_nn,
                                 d_st, nullptr);
    });
}

tda_status tda_features_batch(tda_ctx* ctx, const double* dgm, const int* cnt, int n_dgm, int cap, double* feat)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_dgm);
    if (n_dgm == 0) return TDA_OK;
    CHECK_PTR(ctx, dgm); CHECK_PTR(ctx, cnt); CHECK_PTR(ctx, feat);
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= 1");
    Stage s(ctx);
    const DgmSet d = dgm_in(s, dgm, cnt, (size_t)n_dgm, cap);
    auto d_feat = s.out(feat, (size_t)n_dgm * TDA_N_FEATURES);
    return s.run([&] { return tda_features_batch_dev(ctx, d.rows, d.cnt, n_dgm, cap, d_feat, nullptr); });
}

tda_status tda_aggregate_batch(tda_ctx* ctx, const double* feat_h0, const double* feat_h1, const int* seg_off,
                               int n_seg, int n_total, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg); CHECK_NONNEG(ctx, n_total);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, feat_h0); CHECK_PTR(ctx, feat_h1); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    Stage s(ctx);
    auto d0 = s.in(feat_h0, (size_t)n_total * TDA_N_FEATURES);
    auto d1 = s.in(feat_h1, (size_t)n_total * TDA_N_FEATURES);
    auto d_off = s.in(seg_off, (size_t)(n_seg + 1));
    auto d_out = s.out(out, (size_t)n_seg * 4 * TDA_N_FEATURES);
    return s.run([&] { return tda_aggregate_batch_dev(ctx, d0, d1, d_off, n_seg, d_out, nullptr); });
}

tda_status tda_segment_nanmean(tda_ctx* ctx, const double* x, const int* seg_off, int n_seg, int n_total, double* out)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg); CHECK_NONNEG(ctx, n_total);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, out);
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n_total);
    auto d_off = s.in(seg_off, (size_t)(n_seg + 1));
    auto d_out = s.out(out, (size_t)n_seg);
    return s.run([&] { return tda_segment_nanmean_dev(ctx, d_x, d_off, n_seg, d_out, nullptr); });
}

tda_status tda_spearman_batch(tda_ctx* ctx, const double* x, const double* y, int n_total, int ld, const int* cols,
                              int n_cols, const int* seg_off, int n_seg, double* r)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_seg);
    if (n_seg == 0) return TDA_OK;
    CHECK_PTR(ctx, x); CHECK_PTR(ctx, y); CHECK_PTR(ctx, cols); CHECK_PTR(ctx, seg_off); CHECK_PTR(ctx, r);
    if (n_total < 1 || ld < 1 || n_cols < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "sizes must be >= 1");
    Stage s(ctx);
    auto d_x = s.in(x, (size_t)n_total * ld);
    auto d_y = s.in(y, (size_t)n_total * ld);
    auto d_c = s.in(cols, (size_t)n_cols);
    auto d_o = s.in(seg_off, (size_t)(n_seg + 1));
    auto d_r = s.out(r, (size_t)n_seg * n_cols);
    return s.run([&] { return tda_spearman_batch_dev(ctx, d_x, d_y, ld, d_c, n_cols, d_o, n_seg, d_r, nullptr); });
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
    Stage s(ctx);
    auto d_a = s.in(fa, (size_t)n_total * ld);
    auto d_e = s.in(fe, (size_t)n_total * ld);
    auto d_c = s.in(cols, (size_t)n_cols);
    auto d_o = s.in(seg_off, (size_t)(n_seg + 1));
    auto d_st = s.in(status_b, (size_t)n_total);
    auto d_out = s.out(out, (size_t)n_seg * 2 * n_cols);
    return s.run([&] { return tda_temporal_corr_dev(ctx, d_a, d_e, ld, d_c, n_cols, d_o, n_seg, d_st, d_out, nullptr); });
}

tda_status tda_wasserstein_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                 const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                 const int* idx_b, int n_pairs, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_wasserstein_batch_dev(ctx, d.a.rows, d.a.cnt, cap_a, d.b.rows, d.b.cnt, cap_b, d.ia, d.ib,
                                                                 n_pairs, d.out, d.st, nullptr); });
}

tda_status tda_bottleneck_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                const int* idx_b, int n_pairs, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_bottleneck_batch_dev(ctx, d.a.rows, d.a.cnt, cap_a, d.b.rows, d.b.cnt, cap_b, d.ia, d.ib,
                                                                n_pairs, d.out, d.st, nullptr); });
}

tda_status tda_wasserstein_q_batch(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                   const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                   const int* idx_b, int n_pairs, int order, int ground, double* out, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_pairs);
    if ((order != 1 && order != 2) || (ground != TDA_GROUND_L2 && ground != TDA_GROUND_LINF))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "order must be 1 or 2 and ground TDA_GROUND_L2 or TDA_GROUND_LINF");
    return pair_batch_host(ctx, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, status,
        [&](const PairDev& d) { return tda_wasserstein_q_batch_dev(ctx, d.a.rows, d.a.cnt, cap_a, d.b.rows, d.b.cnt, cap_b, d.ia, d.ib,
                                                                   n_pairs, order, ground, d.out, d.st, nullptr); });
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
        [&](const PairDev& d) { return tda_sliced_wasserstein_batch_dev(ctx, d.a.rows, d.a.cnt, cap_a, d.b.rows, d.b.cnt, cap_b, d.ia,
                                                                        d.ib, n_pairs, d.dirs, n_dirs, d.out, d.st, nullptr); });
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
    Stage s(ctx);
    const PairDev d = pair_stage(s, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out, kvals,
                                 status);
    return s.run([&] {
        return tda_diagram_kernel_pairs_dev(ctx, d.a.rows, d.a.cnt, n_a, cap_a, d.b.rows, d.b.cnt, n_b, cap_b, d.ia, d.ib, n_pairs,
                                            ninv, mirror, scale, weight, wc, d.out, d.kv, d.st, nullptr);
    });
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
    Stage s(ctx);
    const DgmSet a = dgm_in(s, dgm_a, cnt_a, (size_t)n_a, cap_a);
    const GroupIn ga = group_in(s, seg_off_a, n_seg_a, status_a, (size_t)n_a);
    DgmSet b;
    GroupIn gb;
    if (!sym) {
        // (an empty second set still needs a non-NULL buffer to be told from the symmetric form: two doubles and an int of
        // its own)
        if (n_b) b = dgm_in(s, dgm_b, cnt_b, (size_t)n_b, cap_b);
        else b = {s.work<double>(2), s.work<int>(1)};
        gb = group_in(s, seg_off_b, n_seg_b, status_b, (size_t)n_b);
    }
    auto d_out = s.out(out, (size_t)n_seg_a * n_seg_b);
    return s.run([&] {
        return tda_diagram_kernel_gram_dev(ctx, a.rows, a.cnt, n_a, cap_a, ga.off, n_seg_a, ga.status, b.rows, b.cnt, n_b, cap_b,
                                           gb.off, n_seg_b, gb.status, skip_mask, ninv, mirror, scale, weight, wc, d_out, nullptr);
    });
}

// (not pair_batch_host: an index outside its set is a status of that pair, not a refusal of the call)
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
    Stage s(ctx);
    const PairDev d = pair_stage(s, dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, nullptr, 0, out,
                                 nullptr, status);
    return s.run([&] {
        return tda_persistence_fisher_batch_dev(ctx, d.a.rows, d.a.cnt, n_a, cap_a, d.b.rows, d.b.cnt, n_b, cap_b, d.ia, d.ib,
                                                n_pairs, ninv, d.out, d.st, nullptr);
    });
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
    long long n_el;
    if (tda_status st = sig_extent(ctx, win_start, win_ld, n_win, n_ch, n_t, &n_el)) return st;
    Stage s(ctx);
    const size_t n_sig = (size_t)n_win * n_ch;
    auto d_sig = s.in(sig, (size_t)n_el);
    auto d_ws = s.in(win_start, (size_t)n_win);
    auto d_wl = s.in(win_ld, (size_t)n_win);
    auto d_dgm = s.inout(dgm, n_sig * cap * 2);
    auto d_idx = s.inout(idx, n_sig * cap * 2);
    auto d_cnt = s.out(cnt, n_sig);
    auto d_st = s.out(status, n_sig);
    return s.run([&] {
        return tda_sublevel_batch_dev(ctx, d_sig, d_ws, d_wl, n_win, n_ch, n_t, d_dgm, cap, d_cnt, d_idx, d_st, nullptr);
    });
}

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
    Stage s(ctx);
    const long long wd = TDA_PT_WORK_DOUBLES(n_mat, n, n_perm);
    Dev<double> d_D, d_work, d_out;
    if (n_mat) {
        d_D = s.in(D, ((size_t)n_mat * n - 1) * ld + n);
        d_work = s.work<double>((size_t)wd);
        d_out = s.out(out, (size_t)n_mat * 3 * n_perm);
    }
    auto d_lab = s.in(lab, (size_t)TDA_PT_WORDS(n_perm) * n);
    auto d_n1 = s.out(n1, (size_t)n_perm);
    return s.run([&] { return tda_perm_sums_batch_dev(ctx, d_D, n_mat, n, ld, d_lab, n_perm, d_work, wd, d_out, d_n1, nullptr); });
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
    Stage s(ctx);
    const DgmSet d = dgm_in(s, dgm, cnt, (size_t)n_dgm, cap);
    auto d_grid = s.in(grid, (size_t)n_grid);
    auto d_out = s.out(out, (size_t)n_dgm * (n_levels + 1) * n_grid);
    return s.run([&] {
        return tda_landscape_mean_dev(ctx, d.rows, d.cnt, cap, n_dgm, nullptr, n_dgm, nullptr, 0, d_grid, n_grid, n_levels, d_out,
                                      nullptr);
    });
}

// The host twins refuse by the launchers' own rules (win_src_limits of rips_keys_dev.h, ec_check, gn_check) before anything
// is staged.
tda_status tda_euler_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                              const double* grid, int n_grid, int max_dim, int* counts, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 2, n, 0, 1, nullptr, nullptr));
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    Stage s(ctx);
    auto d_dm = s.in(dm, (size_t)n_win * n * n);
    auto d_grid = s.in(grid, (size_t)n_grid);
    auto d_cnt = s.out(counts, (size_t)n_win * (max_dim + 2) * n_grid);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_euler_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, d_grid, n_grid, max_dim, d_cnt, d_st, nullptr);
    });
}

tda_status tda_euler_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                 int normalise, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                 int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 1, p_cap, dim, 1, nullptr, nullptr));
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    Stage s(ctx);
    auto d_pc = s.in(pc, (size_t)n_win * p_cap * dim);
    auto d_n = s.in(n_pts, (size_t)n_win);
    auto d_grid = s.in(grid, (size_t)n_grid);
    auto d_cnt = s.out(counts, (size_t)n_win * (max_dim + 2) * n_grid);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_euler_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, d_grid, n_grid, max_dim, d_cnt, d_st,
                                         nullptr);
    });
}

tda_status tda_euler_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                  int subsample, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                                  int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 0, n_t, dim, subsample, nullptr, nullptr));
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); CHECK_PTR(ctx, grid); CHECK_PTR(ctx, counts); CHECK_PTR(ctx, status);
    Stage s(ctx);
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.in(tau, (size_t)n_win);
    auto d_grid = s.in(grid, (size_t)n_grid);
    auto d_cnt = s.out(counts, (size_t)n_win * (max_dim + 2) * n_grid);
    auto d_np = s.out(n_points, (size_t)n_win);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_euler_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, d_grid, n_grid, max_dim, d_cnt, d_np,
                                          d_st, nullptr);
    });
}

tda_status tda_euler_mean(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off, int n_seg,
                          const int* status_in, int skip_mask, double* mean)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    if (n_win) CHECK_PTR(ctx, counts);
    CHECK_PTR(ctx, mean);
    Stage s(ctx);
    const size_t rg = (size_t)(max_dim + 2) * n_grid;
    auto d_cnt = s.in(counts, (size_t)n_win * rg);
    const GroupIn g = group_in(s, seg_off, n_seg, status_in, (size_t)n_win);
    auto d_mean = s.out(mean, (size_t)n_seg * rg);
    return s.run([&] {
        return tda_euler_mean_dev(ctx, d_cnt, n_win, max_dim, n_grid, g.off, n_seg, g.status, skip_mask, d_mean, nullptr);
    });
}

namespace {
// the device twins of the outputs of a tda_network_* host call; n_node: the columns of nodal
struct NetStage {
    Dev<double> grid, measures;
    Dev<int> counts, nodal, status;
    NetStage(Stage& s, size_t nw, const double* grid, int n_grid, int n_node, int* counts, double* measures, int* nodal, int* status)
        : grid(s.in(grid, (size_t)n_grid)), measures(s.out(measures, nw * TDA_NET_MEASURES * n_grid)),
          counts(s.out(counts, nw * TDA_NET_ROWS * n_grid)), nodal(s.out(nodal, nw * TDA_NET_NODAL * n_grid * n_node)),
          status(s.out(status, nw)) {}
};
}   // namespace

tda_status tda_network_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                const double* grid, int n_grid, int* counts, double* measures, int* nodal, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 2, n, 0, 1, nullptr, nullptr));
    TDA_TRY(nt_check(ctx, n_grid));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_dm = s.in(dm, (size_t)n_win * n * n);
    const NetStage d(s, (size_t)n_win, grid, n_grid, n, counts, measures, nodal, status);
    return s.run([&] {
        return tda_network_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, d.grid, n_grid, d.counts, d.measures, d.nodal,
                                        d.status, nullptr);
    });
}

tda_status tda_network_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                   int normalise, double thresh, const double* grid, int n_grid, int* counts,
                                   double* measures, int* nodal, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 1, p_cap, dim, 1, nullptr, nullptr));
    TDA_TRY(nt_check(ctx, n_grid));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_pc = s.in(pc, (size_t)n_win * p_cap * dim);
    auto d_n = s.in(n_pts, (size_t)n_win);
    const NetStage d(s, (size_t)n_win, grid, n_grid, p_cap, counts, measures, nodal, status);
    return s.run([&] {
        return tda_network_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, d.grid, n_grid, d.counts,
                                           d.measures, d.nodal, d.status, nullptr);
    });
}

tda_status tda_network_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                    int subsample, double thresh, const double* grid, int n_grid, int* counts,
                                    double* measures, int* nodal, int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 0, n_t, dim, subsample, nullptr, nullptr));
    TDA_TRY(nt_check(ctx, n_grid));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.in(tau, (size_t)n_win);
    const NetStage d(s, (size_t)n_win, grid, n_grid, TDA_MAX_POINTS, counts, measures, nodal, status);
    auto d_np = s.out(n_points, (size_t)n_win);
    return s.run([&] {
        return tda_network_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, d.grid, n_grid, d.counts,
                                            d.measures, d.nodal, d_np, d.status, nullptr);
    });
}

tda_status tda_network_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* nodal, int n_win,
                            int n_grid, int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                            double* mean_counts, double* mean_measures, double* mean_nodal)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    TDA_TRY(nt_mean_check(ctx, counts, measures, nodal, n_win, n_grid, n_node, seg_off, n_seg, mean_counts, mean_measures,
                          mean_nodal));
    if (n_seg == 0) return TDA_OK;
    Stage s(ctx);
    const size_t ng = (size_t)n_grid, nn = nodal || mean_nodal ? (size_t)n_node : 0;
    auto d_cnt = s.in(counts, (size_t)n_win * TDA_NET_ROWS * ng);
    auto d_mea = s.in(measures, (size_t)n_win * TDA_NET_MEASURES * ng);
    auto d_nod = s.in(nodal, (size_t)n_win * TDA_NET_NODAL * ng * nn);
    const GroupIn g = group_in(s, seg_off, n_seg, status_in, (size_t)n_win);
    auto d_mc = s.out(mean_counts, (size_t)n_seg * TDA_NET_ROWS * ng);
    auto d_mm = s.out(mean_measures, (size_t)n_seg * TDA_NET_MEASURES * ng);
    auto d_mn = s.out(mean_nodal, (size_t)n_seg * TDA_NET_NODAL * ng * nn);
    return s.run([&] {
        return tda_network_mean_dev(ctx, d_cnt, d_mea, d_nod, n_win, n_grid, n_node, g.off, n_seg, g.status, skip_mask, d_mc,
                                    d_mm, d_mn, nullptr);
    });
}

namespace {
// the device twins of the outputs of a tda_recurrence_* host call; n_hist: the columns of hist
struct RqStage {
    Dev<double> grid, measures;
    Dev<int> counts, hist, status;
    RqStage(Stage& s, size_t nw, const double* grid, int n_grid, int n_hist, int* counts, double* measures, int* hist, int* status)
        : grid(s.in(grid, (size_t)n_grid)), measures(s.out(measures, nw * TDA_RQA_MEASURES * n_grid)),
          counts(s.out(counts, nw * TDA_RQA_ROWS * n_grid)), hist(s.out(hist, nw * 2 * n_grid * n_hist)),
          status(s.out(status, nw)) {}
};
}   // namespace

tda_status tda_recurrence_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                   const double* grid, int n_grid, RQ_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 2, n, 0, 1, nullptr, nullptr));
    TDA_TRY(rq_check(ctx, n_grid, theiler, l_min, v_min));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_dm = s.in(dm, (size_t)n_win * n * n);
    const RqStage d(s, (size_t)n_win, grid, n_grid, n, counts, measures, hist, status);
    return s.run([&] {
        return tda_recurrence_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, d.grid, n_grid, theiler, l_min, v_min,
                                           d.counts, d.measures, d.hist, d.status, nullptr);
    });
}

tda_status tda_recurrence_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                      int normalise, double thresh, const double* grid, int n_grid, RQ_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 1, p_cap, dim, 1, nullptr, nullptr));
    TDA_TRY(rq_check(ctx, n_grid, theiler, l_min, v_min));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_pc = s.in(pc, (size_t)n_win * p_cap * dim);
    auto d_n = s.in(n_pts, (size_t)n_win);
    const RqStage d(s, (size_t)n_win, grid, n_grid, p_cap, counts, measures, hist, status);
    return s.run([&] {
        return tda_recurrence_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, d.grid, n_grid, theiler,
                                              l_min, v_min, d.counts, d.measures, d.hist, d.status, nullptr);
    });
}

tda_status tda_recurrence_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                       int subsample, double thresh, const double* grid, int n_grid, RQ_PARAMS,
                                       int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 0, n_t, dim, subsample, nullptr, nullptr));
    TDA_TRY(rq_check(ctx, n_grid, theiler, l_min, v_min));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); NET_CHECK_PTRS(ctx);
    Stage s(ctx);
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.in(tau, (size_t)n_win);
    const RqStage d(s, (size_t)n_win, grid, n_grid, TDA_MAX_POINTS, counts, measures, hist, status);
    auto d_np = s.out(n_points, (size_t)n_win);
    return s.run([&] {
        return tda_recurrence_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, d.grid, n_grid, theiler,
                                               l_min, v_min, d.counts, d.measures, d.hist, d_np, d.status, nullptr);
    });
}

tda_status tda_recurrence_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* hist, int n_win,
                               int n_grid, int n_hist, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                               double* mean_counts, double* mean_measures, double* mean_hist)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win); CHECK_NONNEG(ctx, n_seg);
    TDA_TRY(rq_mean_check(ctx, counts, measures, hist, n_win, n_grid, n_hist, seg_off, n_seg, mean_counts, mean_measures,
                          mean_hist));
    if (n_seg == 0) return TDA_OK;
    Stage s(ctx);
    const size_t ng = (size_t)n_grid, nh = hist || mean_hist ? (size_t)n_hist : 0;
    auto d_cnt = s.in(counts, (size_t)n_win * TDA_RQA_ROWS * ng);
    auto d_mea = s.in(measures, (size_t)n_win * TDA_RQA_MEASURES * ng);
    auto d_his = s.in(hist, (size_t)n_win * 2 * ng * nh);
    const GroupIn g = group_in(s, seg_off, n_seg, status_in, (size_t)n_win);
    auto d_mc = s.out(mean_counts, (size_t)n_seg * TDA_RQA_ROWS * ng);
    auto d_mm = s.out(mean_measures, (size_t)n_seg * TDA_RQA_MEASURES * ng);
    auto d_mh = s.out(mean_hist, (size_t)n_seg * 2 * ng * nh);
    return s.run([&] {
        return tda_recurrence_mean_dev(ctx, d_cnt, d_mea, d_his, n_win, n_grid, n_hist, g.off, n_seg, g.status, skip_mask, d_mc,
                                       d_mm, d_mh, nullptr);
    });
}

namespace {
// the device twins of the row inputs and outputs of a host call
struct GenStage {
    DgmSet h0, h1;
    Dev<int> rips_status, h1_flag, cyc_len, work;
    Dev<short> h1_gen, cyc, h0_edge;
    Dev<double> part;
    void add(Stage& s, size_t nw, int part_ld, GEN_PARAMS)
    {
        (void)skip_mask;
        if (h0 && h0_cnt) this->h0 = dgm_in(s, h0, h0_cnt, nw, h0_cap);
        this->h1 = dgm_in(s, h1, h1_cnt, nw, h1_cap);
        this->rips_status = s.in(rips_status, nw);
        this->h1_gen = s.out(h1_gen, nw * h1_cap * 4);
        this->h1_flag = s.out(h1_flag, nw * h1_cap);
        this->cyc = s.out(cyc, nw * h1_cap * cyc_cap);
        this->cyc_len = s.out(cyc_len, nw * h1_cap);
        this->part = s.out(part, nw * part_ld);
        this->h0_edge = s.out(h0_edge, nw * h0_cap * 2);
        this->work = s.out(work, nw * 8);
    }
};
}   // namespace
#define GEN_STAGED(d) d.h0.rows, h0_cap, d.h0.cnt, d.h1.rows, h1_cap, d.h1.cnt, d.rips_status, skip_mask, cyc_cap, d.h1_gen, \
                      d.h1_flag, d.cyc, d.cyc_len, d.part, d.h0_edge, d.work

tda_status tda_generators_dm_batch(tda_ctx* ctx, const double* dm, int n_win, int n, double thresh, int symmetrise,
                                   GEN_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 2, n, 0, 1, nullptr, nullptr));
    TDA_TRY(gn_check(ctx, gen_args(GEN_PASS)));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, dm); GEN_CHECK_PTRS(ctx);
    Stage s(ctx);
    GenStage d;
    auto d_dm = s.in(dm, (size_t)n_win * n * n);
    d.add(s, (size_t)n_win, n, GEN_PASS);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_generators_dm_batch_dev(ctx, d_dm, n_win, n, thresh, symmetrise, GEN_STAGED(d), d_st, nullptr);
    });
}

tda_status tda_generators_cloud_batch(tda_ctx* ctx, const double* pc, const int* n_pts, int n_win, int p_cap, int dim,
                                      int normalise, double thresh, GEN_PARAMS, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 1, p_cap, dim, 1, nullptr, nullptr));
    TDA_TRY(gn_check(ctx, gen_args(GEN_PASS)));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, pc); CHECK_PTR(ctx, n_pts); GEN_CHECK_PTRS(ctx);
    Stage s(ctx);
    GenStage d;
    auto d_pc = s.in(pc, (size_t)n_win * p_cap * dim);
    auto d_n = s.in(n_pts, (size_t)n_win);
    d.add(s, (size_t)n_win, p_cap, GEN_PASS);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_generators_cloud_batch_dev(ctx, d_pc, d_n, n_win, p_cap, dim, normalise, thresh, GEN_STAGED(d), d_st, nullptr);
    });
}

tda_status tda_generators_takens_batch(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int dim,
                                       int subsample, double thresh, GEN_PARAMS, int* n_points, int* status)
{
    CHECK_CTX(ctx); CHECK_NONNEG(ctx, n_win);
    TDA_TRY(win_src_limits(ctx, 0, n_t, dim, subsample, nullptr, nullptr));
    TDA_TRY(gn_check(ctx, gen_args(GEN_PASS)));
    if (n_win == 0) return TDA_OK;
    CHECK_PTR(ctx, win); CHECK_PTR(ctx, tau); GEN_CHECK_PTRS(ctx);
    Stage s(ctx);
    GenStage d;
    auto d_win = s.in(win, (size_t)n_win * n_t);
    auto d_tau = s.in(tau, (size_t)n_win);
    d.add(s, (size_t)n_win, TDA_MAX_POINTS, GEN_PASS);
    auto d_np = s.out(n_points, (size_t)n_win);
    auto d_st = s.out(status, (size_t)n_win);
    return s.run([&] {
        return tda_generators_takens_batch_dev(ctx, d_win, d_tau, n_win, n_t, dim, subsample, thresh, GEN_STAGED(d), d_np, d_st,
                                               nullptr);
    });
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
    Stage s(ctx);
    auto d_part = s.in(part, (size_t)n_win * n);
    const GroupIn g = group_in(s, seg_off, n_seg, status_in, (size_t)n_win);
    auto d_mean = s.out(mean, (size_t)n_seg * n);
    return s.run([&] {
        return tda_generators_mean_dev(ctx, d_part, n_win, n, g.off, n_seg, g.status, skip_mask, d_mean, nullptr);
    });
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
    Stage s(ctx);
    const DgmSet d = dgm_in(s, dgm, cnt, (size_t)n_dgm, cap);
    const GroupIn g = group_in(s, seg_off, n_seg, status_in, (size_t)n_dgm);
    auto d_mean = s.out(mean, (size_t)n_seg * cap_out * 2);
    auto d_mc = s.out(mean_cnt, (size_t)n_seg);
    auto d_var = s.out(var, (size_t)n_seg);
    auto d_it = s.out(iters, (size_t)n_seg);
    auto d_st = s.out(status, (size_t)n_seg);
    return s.run([&] {
        return tda_frechet_mean_dev(ctx, d.rows, d.cnt, cap, n_dgm, g.off, n_seg, g.status, skip_mask, max_iter, d_mean, d_mc, cap_out,
                                    d_var, d_it, d_st, nullptr);
    });
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
    Stage s(ctx);
    const DgmSet d = dgm_in(s, dgm, cnt, (size_t)n_dgm, cap);
    auto d_xe = s.in(xe, (size_t)(n_x + 1));
    auto d_ye = s.in(ye, (size_t)(n_y + 1));
    auto d_out = s.out(out, (size_t)n_dgm * n_y * n_x);
    return s.run([&] {
        return tda_image_mean_dev(ctx, d.rows, d.cnt, cap, n_dgm, nullptr, n_dgm, nullptr, 0, d_xe, n_x, d_ye, n_y, sigma, power,
                                  d_out, nullptr);
    });
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
