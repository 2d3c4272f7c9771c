// common.h -- shared host/device helpers of libtdaeeg (gfx950 only, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/tdaeeg.h"

typedef unsigned long long u64;
typedef uint32_t u32;
typedef uint16_t u16;

struct tda_ctx {
    int device = 0;
    int words_dm = 2;       // H1 class capacity (x64) for distance-matrix input
    int words_cloud = 1;    // ... for point clouds
    int retry_policy = 0;   // TDA_RETRY_*
    unsigned long long* retry_ctr = nullptr;   // tda_set_retry_counter: device u64[4]
    unsigned long long* total_scratch = nullptr;   // class vectors of the last rung of the Rips ladders (rips.hip: TOT_SLOTS x 8.3 MB)
    int h1_order = 0;       // TDA_ORDER_*
    int launch_scheme = 0;  // TDA_SCHEME_*
    int ws_prune = 1;       // tda_set_wasserstein_pruning
    unsigned long long* ws_ctr = nullptr;      // tda_set_wasserstein_counter: device u64[3]
    // Lists of the windows a widening pass has to redo (rips.hip: retry_collect): one buffer per STREAM -- the Rips calls
    // of a stream, eager or replayed from a HIP graph captured on it, run one after the other, so a stream's list is never
    // in use twice, while calls on different streams never share one.  TDA_RETRY_SLOTS buffers, allocated with the context
    // and assigned to streams in the order they are first seen (more streams than buffers: the last one is shared and
    // retry_shared counts it).  [0] = entries, [1] = workgroups done, the window indices from [4] on.  A call with more
    // windows than retry_cap replaces all buffers (the old ones stay alive for graphs that hold their addresses).
    // fin_list / ws_list: the same per stream for the diagrams the packed finishing kernel leaves to the wide one
    // (features.hip) and for the pairs the small Wasserstein launch defers (wasserstein.hip).  The three lists of a slot
    // are one allocation (retry_buf[i] is its base) and have the same layout and capacity.
    int* retry_buf[32] = {};
    int* fin_list[32] = {};
    int* ws_list[32] = {};
    hipStream_t retry_stream[32] = {};
    int retry_streams = 0;
    int retry_shared = 0;
    int retry_cap = 0;
    std::vector<void*> retired;
    // host-API staging workspace (grown on demand, only by the host-pointer twins)
    void* ws = nullptr;
    size_t ws_bytes = 0;
    std::string err;
    // one-shot kernel probes (tda_set_kernel_probe), one slot per probed kernel
    struct Probe { hipEvent_t start = nullptr, stop = nullptr; unsigned long long* span = nullptr; bool armed = false; };
    Probe probe[4];
};

// brackets ONE kernel launch with the armed probe of `which` (if any) and disarms it
struct ProbeScope {
    tda_ctx* ctx; hipStream_t st; int which; bool on; unsigned long long* span;
    ProbeScope(tda_ctx* c, int w, hipStream_t s)
        : ctx(c), st(s), which(w), on(w > 0 && w < 4 && c->probe[w].armed), span(nullptr)
    {
        if (on) {
            span = ctx->probe[which].span;
            if (ctx->probe[which].start) (void)hipEventRecord(ctx->probe[which].start, st);
        }
    }
    ~ProbeScope()
    {
        if (on) {
            if (ctx->probe[which].stop) (void)hipEventRecord(ctx->probe[which].stop, st);
            ctx->probe[which] = tda_ctx::Probe();
        }
    }
};

#define TDA_HIP(ctx, call)                                                          \
    do {                                                                            \
        hipError_t e__ = (call);                                                    \
        if (e__ != hipSuccess) {                                                    \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);        \
            return TDA_ERR_HIP;                                                     \
        }                                                                           \
    } while (0)

#define TDA_FAIL(ctx, code, msg)                                                    \
    do { (ctx)->err = (msg); return (code); } while (0)

// passes a refusal on
#define TDA_TRY(call)                                                               \
    do { const tda_status rc__ = (call); if (rc__ != TDA_OK) return rc__; } while (0)

// ---- wave64 cross-lane helpers (lane index must be wave-uniform) ----
__device__ __forceinline__ u32 rl32(u32 v, int lane) { return (u32)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ u64 rl64(u64 v, int lane)
{
    u32 lo = rl32((u32)v, lane), hi = rl32((u32)(v >> 32), lane);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 uni64(u64 v)
{
    u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
    u32 hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}
// sqrt of a double >= 0, bit for bit what sqrt() returns: the library's own sequence (v_rsq_f64 and three fused
// corrections) without its rescaling of tiny arguments and its class test.  Arguments outside {0} u [2^-767, inf) --
// squares of coordinates below 1e-115, infinities, NaNs -- take the library's path, decided per wave on the high word.
__device__ __forceinline__ double sqrt_rn(double x)
{
    const bool zero = x == 0.0;
    const u32 hi = (u32)(__double_as_longlong(x) >> 32);
    if (__builtin_expect(__ballot(hi - 0x10000000u > 0x6fefffffu && !zero) != 0ull, 0)) return sqrt(x);
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    double d = fma(-g, g, x);
    g = fma(d, h, g);
    d = fma(-g, g, x);
    g = fma(d, h, g);
    return zero ? x : g;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// ---- wave64 reductions on the DPP network (a few VALU cycles per step; __shfl_xor goes through
// ds_bpermute and costs an LDS round trip per step).  Result is wave-uniform.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const int hi2 = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double uni_f64(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
#define TDA_DPP_REDUCE_F64(v, OP)                                                     \
    do {                                                                              \
        double o__;                                                                   \
        o__ = dpp_f64<0xB1, 0xF>(v); v = OP(o__, v);   /* quad_perm [1,0,3,2] */      \
        o__ = dpp_f64<0x4E, 0xF>(v); v = OP(o__, v);   /* quad_perm [2,3,0,1] */      \
        o__ = dpp_f64<0x141, 0xF>(v); v = OP(o__, v);  /* row_half_mirror     */      \
        o__ = dpp_f64<0x140, 0xF>(v); v = OP(o__, v);  /* row_mirror          */      \
        o__ = dpp_f64<0x142, 0xA>(v); v = OP(o__, v);  /* row_bcast:15        */      \
        o__ = dpp_f64<0x143, 0xC>(v); v = OP(o__, v);  /* row_bcast:31        */      \
    } while (0)
#define TDA_MIN_(a, b) ((a) < (b) ? (a) : (b))
#define TDA_MAX_(a, b) ((a) > (b) ? (a) : (b))
#define TDA_ADD_(a, b) ((a) + (b))
__device__ __forceinline__ double wave_min_f64_dpp(double v) { TDA_DPP_REDUCE_F64(v, TDA_MIN_); return uni_f64(v, 63); }
__device__ __forceinline__ double wave_max_f64_dpp(double v) { TDA_DPP_REDUCE_F64(v, TDA_MAX_); return uni_f64(v, 63); }

// The DPP modifier sits on the min / max instruction itself (one instruction per step; the builtin route costs a
// v_mov_b32_dpp plus the operation).  s_nop 1 = the two wait states between a VALU write and a DPP read of a VGPR.
#define TDA_DPP_STEPS_(OP)                                                                   \
    "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"        \
    "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"        \
    "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"            \
    "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"                 \
    "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"               \
    "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"               \
    "s_nop 1"
__device__ __forceinline__ int wave_max_i32_dpp(int v)
{
    asm volatile(TDA_DPP_STEPS_("v_max_i32_dpp") : "+v"(v));
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ u32 wave_min_u32_dpp(u32 x)
{
    int v = (int)x;
    asm volatile(TDA_DPP_STEPS_("v_min_u32_dpp") : "+v"(v));
    return (u32)__builtin_amdgcn_readlane(v, 63);
}

// order-preserving float32 <-> uint32 (handles negative values; NaN sorts last)
__device__ __forceinline__ u32 f32_sortable(float f)
{
    u32 b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sortable_f32(u32 s)
{
    u32 b = (s & 0x80000000u) ? (s & 0x7fffffffu) : ~s;
    return __uint_as_float(b);
}

// mean[g][j] = the mean over the windows w of group g (seg_off[g] <= w < seg_off[g + 1]; seg_off == NULL: every window its
// own group) of val[w][j], j < row_len, without the windows whose status_in has a bit of skip_mask: one thread per (g, j)
// adds them in window order in ACC; NaN for a group with none left.  (euler.hip: int32 in int64; generators.hip: double)
template <typename T, typename ACC>
__global__ void __launch_bounds__(256)
group_mean_kernel(const T* __restrict__ val, int n_win, int row_len, const int* __restrict__ seg_off, int n_seg,
                  const int* __restrict__ status_in, int skip_mask, double* __restrict__ mean)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_seg * row_len) return;
    const int g = (int)(idx / row_len), j = (int)(idx - (long long)g * row_len);
    int w0 = g, w1 = g + 1;
    if (seg_off) { w0 = seg_off[g]; w1 = seg_off[g + 1]; }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_win ? n_win : w1;
    ACC S = 0;
    int m = 0;
    for (int w = w0; w < w1; ++w) {
        if (status_in && (status_in[w] & skip_mask)) continue;
        S += val[(size_t)w * row_len + j];
        ++m;
    }
    mean[idx] = m ? (double)S / (double)m : __longlong_as_double(0x7ff8000000000000ll);
}

// launch-side entry points implemented in the .hip files
size_t rips_total_scratch_bytes();
#define TDA_RETRY_SLOTS 32
tda_status retry_lists_reserve(tda_ctx*, int n_win);      // (rips.hip) all slots to at least n_win entries
// (rips.hip) slot of the stream, lists of at least n entries: -1 when they would have to grow while st is being captured
// (never a hipMalloc inside a capture) -- the caller then takes its launch over the whole batch
tda_status stream_lists_take(tda_ctx*, int n, hipStream_t st, int* slot);
tda_status launch_corr_dist(tda_ctx*, const double*, int, int, int, double*, double*, hipStream_t);
tda_status launch_corr_dist_sliding(tda_ctx*, const double*, int, int, int, int, double*, double*, int*, hipStream_t);
tda_status launch_corr_to_dist(tda_ctx*, const double*, int, int, int, double*, hipStream_t);
tda_status launch_rips_dm(tda_ctx*, const double*, int, int, double, int, double*, int, int*, double*, int, int*,
                          int*, hipStream_t);
tda_status launch_eeg_windows(tda_ctx*, const double*, int, int, int, double, double*, double*, double*, int, int*, double*,
                              int, int*, int*, hipStream_t);
tda_status launch_eeg_sliding(tda_ctx*, const double*, int, int, int, int, int, const int*, int, double, double*, double*,
                              double*, int, int*, double*, int, int*, int*, int*, hipStream_t);
tda_status launch_rips_cloud(tda_ctx*, const double* win_or_pc, const int* tau_or_npts, int n_win, int n_t_or_pcap,
                             int dim, int subsample, int mode, int normalise, double thresh, double*, int, int*,
                             double*, int, int*, int* n_points, int*, hipStream_t);
// (landmarks.hip) mode 0: Takens windows + tau; mode 1: explicit clouds + n_pts.  Checks the limits of the header itself.
tda_status launch_landmarks(tda_ctx*, const double* win_or_pc, const int* tau_or_npts, int n_win, int n_t_or_pcap, int dim,
                            int subsample, int mode, int normalise, int n_perm, double* lm, int* lm_idx, double* lm_lambda,
                            double* r_cover, int* n_lm, int* n_full, hipStream_t);
// (sublevel.hip) H0 of the sublevel-set filtration of n_win * n_ch signals.  Checks the limits of the header itself.
tda_status launch_sublevel(tda_ctx*, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                           int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status, hipStream_t);
// (plv.hip) phase-locking value matrix of every window and its distance matrix.  Checks the limits of the header itself.
tda_status launch_plv_dist(tda_ctx*, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                           int n_ch, int n_t, const double* g, int method, double* dist, double* plv, int* status, hipStream_t);
// (connectivity.hip) wPLI / imaginary coherency / coherence / envelope correlation of every window and its distance matrix.
// Checks the limits of the header itself.
tda_status launch_connectivity_dist(tda_ctx*, const double* sig, const long long* win_start, const long long* win_ld,
                                    int n_win, int n_ch, int n_t, const double* g, int measure, int method, double* dist,
                                    double* value, int* status, hipStream_t);
// (permutation.hip) S00 / S11 / S01 of n_mat matrices under n_perm relabellings.  Checks the limits of the header itself.
tda_status launch_perm_sums(tda_ctx*, const double* D, int n_mat, int n, int ld, const unsigned long long* lab, int n_perm,
                            double* work, long long work_doubles, double* out, int* n1, hipStream_t);
// (euler.hip) simplex counts and Euler characteristic on a grid, for the windows of a WinSrc (rips_keys_dev.h) as the entry
// point has them: src, aux, n_in, dim, subsample, mode, flag.  Checks the limits of the header itself: ec_check (the grid),
// then win_src_limits.
struct WinSrc;
tda_status ec_check(tda_ctx*, int n_grid, int max_dim);
tda_status launch_euler(tda_ctx*, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid, int max_dim,
                        int* counts, int* n_points, int* status, hipStream_t);
tda_status launch_euler_mean(tda_ctx*, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off, int n_seg,
                             const int* status_in, int skip_mask, double* mean, hipStream_t);
// (network.hip) graph measures of the thresholded graphs on a grid, for the windows as launch_euler takes them.  Checks the
// limits of the header itself: nt_check (the grid), then win_src_limits; nt_mean_check for the means (which pairs are
// given, n_seg without a table, the row length of nodal).
tda_status nt_check(tda_ctx*, int n_grid);
tda_status launch_network(tda_ctx*, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid, int* counts,
                          double* measures, int* nodal, int* n_points, int* status, hipStream_t);
tda_status nt_mean_check(tda_ctx*, const void* counts, const void* measures, const void* nodal, int n_win, int n_grid,
                         int n_node, const int* seg_off, int n_seg, const void* mean_counts, const void* mean_measures,
                         const void* mean_nodal);
tda_status launch_network_mean(tda_ctx*, const int* counts, const double* measures, const int* nodal, int n_win, int n_grid,
                               int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                               double* mean_counts, double* mean_measures, double* mean_nodal, hipStream_t);
// (recurrence.hip) recurrence quantification of the same windows on a grid: the plot is the adjacency matrix in time order
// without a Theiler band.  Checks the limits of the header itself: rq_check (grid, theiler, l_min, v_min), then
// win_src_limits; rq_mean_check for the means, as nt_mean_check.
tda_status rq_check(tda_ctx*, int n_grid, int theiler, int l_min, int v_min);
tda_status launch_recurrence(tda_ctx*, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid, int theiler,
                             int l_min, int v_min, int* counts, double* measures, int* hist, int* n_points, int* status,
                             hipStream_t);
tda_status rq_mean_check(tda_ctx*, const void* counts, const void* measures, const void* hist, int n_win, int n_grid,
                         int n_hist, const int* seg_off, int n_seg, const void* mean_counts, const void* mean_measures,
                         const void* mean_hist);
tda_status launch_recurrence_mean(tda_ctx*, const int* counts, const double* measures, const int* hist, int n_win, int n_grid,
                                  int n_hist, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                                  double* mean_counts, double* mean_measures, double* mean_hist, hipStream_t);
// (generators.hip) the edges behind the rows of a Rips diagram and a representative cycle per H1 row.  GenArgs: the rows the
// Rips entry points wrote and the outputs, as the tda_generators_* entry points take them (part_ld is the launcher's).
struct GenArgs {
    const double* h0; int h0_cap; const int* h0_cnt;
    const double* h1; int h1_cap; const int* h1_cnt;
    const int* rips_status; int skip_mask; int cyc_cap;
    short* h1_gen; int* h1_flag; short* cyc; int* cyc_len;
    double* part; short* h0_edge; int* work;
    int part_ld;
};
// The windows as launch_euler takes them.  Checks the limits of the header itself: gn_check (the capacities, and which
// output needs which), then win_src_limits.
tda_status gn_check(tda_ctx*, const GenArgs& g);
tda_status launch_generators(tda_ctx*, const WinSrc& src, int n_win, double thresh, const GenArgs& g, int* n_points,
                             int* status, hipStream_t);
tda_status launch_generators_mean(tda_ctx*, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                                  const int* status_in, int skip_mask, double* mean, hipStream_t);
tda_status launch_sosfiltfilt(tda_ctx*, const double*, int, int, const double*, const double*, int, int, double*, double*,
                              hipStream_t, int n_filt = 1);
tda_status launch_filtfilt(tda_ctx*, const double*, int, int, const double*, const double*, const double*, int, int, double*,
                           double*, hipStream_t, int n_filt = 1);
tda_status launch_upfirdn(tda_ctx*, const double*, long long, const double*, int, int, int, long long, long long, double*,
                          hipStream_t);
tda_status launch_sosfiltfilt_ragged(tda_ctx*, const double*, int, int, const long long*, const long long*, const long long*,
                                     const double*, const double*, int, int, int, double*, double*, hipStream_t);
tda_status launch_filtfilt_ragged(tda_ctx*, const double*, int, const long long*, const long long*, const long long*,
                                  const double*, const double*, const double*, int, int, int, double*, double*, hipStream_t);
tda_status launch_gather_windows(tda_ctx*, const double*, const long long*, int, int, double*, hipStream_t);
tda_status launch_eeg_ragged(tda_ctx*, const double*, const long long*, const long long*, int, int, int, double, double*,
                             double*, double*, int, int*, double*, int, int*, int*, hipStream_t);
tda_status launch_hilbert_env(tda_ctx*, const double*, int, const double*, double*, hipStream_t);
tda_status launch_resample_poly_ragged(tda_ctx*, const double*, int, const long long*, const long long*, const long long*,
                                       const long long*, const double*, int, int, int, int, double*, hipStream_t);
tda_status launch_hilbert_env_ragged(tda_ctx*, const double*, int, const long long*, const long long*, const long long*,
                                     const double*, const long long*, double*, hipStream_t);
tda_status launch_tau(tda_ctx*, const double*, int, int, int, int*, hipStream_t);
tda_status launch_tau_segments(tda_ctx*, const double*, const int*, int, int, int, int*, int*, hipStream_t);
// (embedding.hip) delay and dimension selection.  launch_ami: seg_off == NULL: the batch form, n_groups windows; otherwise
// the segments form (ami, joint, status NULL; tau is tau_seg).  Both check the limits of the header themselves: ami_check
// (which also resolves max_lag: a negative one is n_t / 4, then the cut to n_t - 2) and fnn_check.
tda_status ami_check(tda_ctx*, int n_t, int n_bins, int* max_lag);
tda_status launch_ami(tda_ctx*, const double* win, const int* seg_off, int n_groups, int n_t, int max_lag, int n_bins,
                      double* ami, int* tau, int* joint, int* status, int* tau_win, hipStream_t);
tda_status fnn_check(tda_ctx*, int n_t, int d_max, int theiler, double r_tol, double a_tol, double frac_tol);
tda_status launch_fnn(tda_ctx*, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler, double r_tol,
                      double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn, int* status, hipStream_t);
tda_status launch_recording_rows(tda_ctx*, const double*, const double*, const int*, const double*, const double*, const int*,
                                 int, double*, const int*, const int*, int*, hipStream_t);
tda_status launch_features(tda_ctx*, const double*, const int*, int, int, double*, hipStream_t);
tda_status launch_diagram_finish(tda_ctx*, const tda_diagram_set*, int, int, hipStream_t);
tda_status launch_aggregate(tda_ctx*, const double*, const double*, const int*, int, double*, hipStream_t);
tda_status launch_nanmean(tda_ctx*, const double*, const int*, int, double*, hipStream_t);
tda_status launch_spearman(tda_ctx*, const double*, const double*, int, const int*, int, const int*, int, double*, hipStream_t);
tda_status launch_temporal_corr(tda_ctx*, const double*, const double*, int, const int*, int, const int*, int, const int*,
                                double*, hipStream_t);
tda_status launch_wasserstein(tda_ctx*, const double*, const int*, int, const double*, const int*, int, const int*,
                              const int*, int, double*, int*, hipStream_t);
tda_status launch_bottleneck(tda_ctx*, const double*, const int*, int, const double*, const int*, int, const int*,
                             const int*, int, double*, int*, hipStream_t);
tda_status launch_wasserstein_q(tda_ctx*, const double*, const int*, int, const double*, const int*, int, const int*,
                                const int*, int, int order, int ground, double*, int*, hipStream_t);
tda_status launch_sliced(tda_ctx*, const double*, const int*, int, const double*, const int*, int, const int*, const int*,
                         int, const double*, int, double*, int*, hipStream_t);
tda_status launch_sliced_prepare(tda_ctx*, const double*, const int*, int, int, const double*, int, const long long*, double*,
                                 long long, int*, hipStream_t);
tda_status launch_sliced_prepared_pairs(tda_ctx*, const double*, const long long*, const int*, int, const double*,
                                        const long long*, const int*, int, const int*, const int*, int, int, double*, int*,
                                        hipStream_t);
tda_status launch_sliced_matrix(tda_ctx*, const double*, const long long*, const int*, int, const int*, int, const int*,
                                const double*, const long long*, const int*, int, const int*, int, int, const int*, int, double*,
                                int*, int*, hipStream_t);
tda_status launch_frechet_mean(tda_ctx*, const double*, const int*, int, int, const int*, int, const int*, int, int, double*,
                               int*, int, double*, int*, int*, hipStream_t);
tda_status launch_landscape_mean(tda_ctx*, const double*, const int*, int, int, const int*, int, const int*, int,
                                 const double*, int, int, double*, hipStream_t);
tda_status launch_image_mean(tda_ctx*, const double*, const int*, int, int, const int*, int, const int*, int, const double*,
                             int, const double*, int, double, int, double*, hipStream_t);
tda_status launch_diagram_kernel_pairs(tda_ctx*, const double*, const int*, int, int, const double*, const int*, int, int,
                                       const int*, const int*, int, double ninv, int mirror, double scale, int weight, double wc,
                                       double*, double*, int*, hipStream_t);
tda_status launch_diagram_kernel_gram(tda_ctx*, const double*, const int*, int, int, const int*, int, const int*, const double*,
                                      const int*, int, int, const int*, int, const int*, int, double ninv, int mirror,
                                      double scale, int weight, double wc, double*, hipStream_t);
tda_status launch_persistence_fisher(tda_ctx*, const double*, const int*, int, int, const double*, const int*, int, int,
                                     const int*, const int*, int, double ninv, double*, int*, hipStream_t);
tda_status launch_wasserstein_cross(tda_ctx*, const double*, const int*, int, int, const int*, const int*, int, const double*,
                                    const int*, int, int, const int*, int, const int*, const int*, double*, int*, hipStream_t);
tda_status launch_cross_rows(tda_ctx*, const double*, const int*, const double*, const int*, const int*, int, double*,
                             const int*, int*, hipStream_t);
tda_status launch_wasserstein_matrix(tda_ctx*, const double*, const int*, int, int, const int*, int, const int*, const double*,
                                     const int*, int, int, const int*, int, int, const int*, double*, int*, int*, hipStream_t);
tda_status launch_match_rows(tda_ctx*, const double*, const int*, const int*, int, int, const int*, const int*, const int*,
                             double*, int*, hipStream_t);
