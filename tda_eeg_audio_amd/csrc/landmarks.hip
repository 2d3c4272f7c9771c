// landmarks.hip -- greedy permutation (furthest-point sampling) of point clouds of up to TDA_LM_MAX_POINTS points:
// ripser's n_perm, in front of the point-cloud Rips kernel (include/tdaeeg.h, "Landmark Rips").
//
// One workgroup of 256 threads per window.  Thread t owns the points t, t + 256, t + 512, t + 768: their coordinates,
// |x|^2 and running distance ds stay in registers for the whole selection (the kernel is a template over dim, so every
// array index is a compile-time constant).  The normalised cloud also lies in LDS, where all lanes read the pivot row by
// its index (one address per wave: a broadcast).  Per selected landmark:
//   1. ds = min(ds, d(., pivot))                                        registers only
//   2. arg-max over (value, lowest index): DPP max of the value inside each wave, DPP min of the indices of the lanes
//      that hold it, one (value, index) pair per wave to LDS, ONE barrier, every thread folds the four pairs
// The pairs are double-buffered on the parity of the iteration: a wave writes the pairs of iteration t + 2 only after
// the barrier of iteration t + 1, which every wave reaches after it has read those of iteration t.  No atomics.
#include "common.h"
#include "rips_keys_dev.h"
#include <climits>

#define LM_NT 256
#define LM_PPT (TDA_LM_MAX_POINTS / LM_NT)     // points per thread
#define LM_WAVES (LM_NT / 64)
static_assert(LM_PPT * LM_NT == TDA_LM_MAX_POINTS, "every point has an owner");

template <int DIM>
__global__ void __launch_bounds__(LM_NT)
landmarks_kernel(const double* __restrict__ src, const int* __restrict__ tau_or_npts, int n_t_or_pcap, int subsample,
                 int mode, int normalise, int n_perm, double* __restrict__ lm, int* __restrict__ lm_idx,
                 double* __restrict__ lm_lambda, double* __restrict__ r_cover, int* __restrict__ n_lm,
                 int* __restrict__ n_full)
{
    __shared__ double pts[TDA_LM_MAX_POINTS * DIM];
    __shared__ double nrm[TDA_LM_MAX_POINTS];
    __shared__ double mm[LM_WAVES][DIM][2];
    __shared__ double red_v[2][LM_WAVES];
    __shared__ u32 red_i[2][LM_WAVES];
    __shared__ int sel[TDA_MAX_POINTS];

    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the points of the window as every Rips consumer counts them (csrc/rips_keys_dev.h); the limit and what a refused
    // window gets are this kernel's own
    const WinSrc S{src, tau_or_npts, n_t_or_pcap, DIM, subsample, mode, normalise, 0};
    const WinExtent X = win_extent(S, win);
    const long long P64 = X.P;
    const int p_lim = (mode == 1 && n_t_or_pcap < TDA_LM_MAX_POINTS) ? n_t_or_pcap : TDA_LM_MAX_POINTS;
    if ((mode == 0 && X.tau < 1) || P64 > p_lim) {
        if (tid == 0) {
            n_lm[win] = TDA_MAX_POINTS + 1;            // the cloud Rips flags this count as TDA_WIN_TOO_LARGE itself
            n_full[win] = P64 > INT_MAX ? INT_MAX : (int)P64;
            r_cover[win] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }
    const int P = P64 < 0 ? 0 : (int)P64;
    lm += (size_t)win * n_perm * DIM;
    lm_idx += (size_t)win * n_perm;
    if (lm_lambda) lm_lambda += (size_t)win * n_perm;

    // the thread's points (slots past P hold zeros and never take part)
    double x[LM_PPT][DIM];
#pragma unroll
    for (int j = 0; j < LM_PPT; ++j) {
        const int i = tid + j * LM_NT;
#pragma unroll
        for (int k = 0; k < DIM; ++k)
            x[j][k] = i < P ? (mode == 0 ? X.base[(size_t)i * subsample + (size_t)k * X.tau] : X.base[(size_t)i * DIM + k]) : 0.0;
    }
    if (normalise && P > 0) {
        // per-column min-max over the whole cloud (range 0 -> 1), utils.py:127-130
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            double mn = INFINITY, mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < LM_PPT; ++j)
                if (tid + j * LM_NT < P) { mn = x[j][k] < mn ? x[j][k] : mn; mx = x[j][k] > mx ? x[j][k] : mx; }
            mn = wave_min_f64_dpp(mn);
            mx = wave_max_f64_dpp(mx);
            if (lane == 0) { mm[wave][k][0] = mn; mm[wave][k][1] = mx; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            double mn = mm[0][k][0], mx = mm[0][k][1];
#pragma unroll
            for (int w = 1; w < LM_WAVES; ++w) {
                mn = mm[w][k][0] < mn ? mm[w][k][0] : mn;
                mx = mm[w][k][1] > mx ? mm[w][k][1] : mx;
            }
            double rg = mx - mn;
            if (rg == 0.0) rg = 1.0;
#pragma unroll
            for (int j = 0; j < LM_PPT; ++j) x[j][k] = (x[j][k] - mn) / rg;
        }
    }
    double nr[LM_PPT];
#pragma unroll
    for (int j = 0; j < LM_PPT; ++j) {
        const int i = tid + j * LM_NT;
        double n = x[j][0] * x[j][0];                  // 0.0 + x0^2 is x0^2 exactly
#pragma unroll
        for (int k = 1; k < DIM; ++k) n += x[j][k] * x[j][k];
        nr[j] = n;
        if (i < P) {
#pragma unroll
            for (int k = 0; k < DIM; ++k) pts[i * DIM + k] = x[j][k];
            nrm[i] = n;
        }
    }
    __syncthreads();

    if (P <= n_perm) {
        // identity: every point is a landmark, in its own order
        for (int e = tid; e < P * DIM; e += LM_NT) lm[e] = pts[e];
        if (tid < P) {
            lm_idx[tid] = tid;
            if (lm_lambda) lm_lambda[tid] = 0.0;
        }
        if (tid == 0) { n_lm[win] = P; n_full[win] = P; r_cover[win] = 0.0; }
        return;
    }

    double ds[LM_PPT];
#pragma unroll
    for (int j = 0; j < LM_PPT; ++j) ds[j] = (tid + j * LM_NT < P) ? INFINITY : -1.0;
    if (tid == 0) sel[0] = 0;
    int p = 0;
    double val = 0.0;
    for (int t = 1; t <= n_perm; ++t) {
        // 1. ds = min(ds, d(., p)); the pivot row is one LDS address for the whole wave
        double xp[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xp[k] = pts[p * DIM + k];
        const double np_ = nrm[p];
#pragma unroll
        for (int j = 0; j < LM_PPT; ++j) {
            if (j * LM_NT < P) {                       // uniform over the workgroup
                const int i = tid + j * LM_NT;
                double dot = x[j][0] * xp[0];
#pragma unroll
                for (int k = 1; k < DIM; ++k) dot = fma(x[j][k], xp[k], dot);
                double d2 = -2.0 * dot;
                d2 += nr[j];
                d2 += np_;
                if (!(d2 > 0.0)) d2 = 0.0;
                double d = sqrt_rn(d2);
                if (i == p) d = 0.0;
                ds[j] = (i < P && d < ds[j]) ? d : ds[j];
            }
        }
        // 2. arg-max over (value, lowest index)
        double bv = ds[0];
        u32 bi = (u32)tid;
#pragma unroll
        for (int j = 1; j < LM_PPT; ++j)
            if (ds[j] > bv) { bv = ds[j]; bi = (u32)(tid + j * LM_NT); }
        const double wv = wave_max_f64_dpp(bv);
        const u32 wi = wave_min_u32_dpp(bv == wv ? bi : 0xffffffffu);
        const int buf = t & 1;
        if (lane == 0) { red_v[buf][wave] = wv; red_i[buf][wave] = wi; }
        __syncthreads();
        val = red_v[buf][0];
        u32 pi = red_i[buf][0];
#pragma unroll
        for (int w = 1; w < LM_WAVES; ++w) {
            const double v = red_v[buf][w];
            const u32 iw = red_i[buf][w];
            if (v > val || (v == val && iw < pi)) { val = v; pi = iw; }
        }
        if (pi >= (u32)P) pi = 0u;                     // non-finite samples: unspecified, but inside the cloud
        p = (int)pi;
        if (tid == 0) {
            if (lm_lambda) lm_lambda[t - 1] = val;
            if (t < n_perm) sel[t] = p;
        }
    }
    __syncthreads();
    for (int e = tid; e < n_perm * DIM; e += LM_NT) {
        const int t = e / DIM, k = e - t * DIM;
        lm[e] = pts[sel[t] * DIM + k];
    }
    if (tid < n_perm) lm_idx[tid] = sel[tid];
    if (tid == 0) { n_lm[win] = n_perm; n_full[win] = P; r_cover[win] = val; }
}

tda_status launch_landmarks(tda_ctx* ctx, const double* src, const int* aux, int n_win, int n_t_or_pcap, int dim,
                            int subsample, int mode, int normalise, int n_perm, double* lm, int* lm_idx,
                            double* lm_lambda, double* r_cover, int* n_lm, int* n_full, hipStream_t st)
{
    if (n_perm < 3 || n_perm > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_perm must be in [3, TDA_MAX_POINTS]");
    if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
    if (subsample < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "subsample must be >= 1");
    if (mode == 0 && (n_t_or_pcap < 1 || n_t_or_pcap > TDA_LM_MAX_SAMPLES))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [1, TDA_LM_MAX_SAMPLES]");
    if (mode == 1 && (n_t_or_pcap < 1 || n_t_or_pcap > TDA_LM_MAX_POINTS))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "p_cap must be in [1, TDA_LM_MAX_POINTS]");
    if (n_win == 0) return TDA_OK;
#define LM_LAUNCH(D)                                                                                                   \
    hipLaunchKernelGGL(landmarks_kernel<D>, dim3(n_win), dim3(LM_NT), 0, st, src, aux, n_t_or_pcap, subsample, mode,   \
                       normalise, n_perm, lm, lm_idx, lm_lambda, r_cover, n_lm, n_full)
    switch (dim) {
    case 1: LM_LAUNCH(1); break;
    case 2: LM_LAUNCH(2); break;
    case 3: LM_LAUNCH(3); break;
    default: LM_LAUNCH(4); break;
    }
#undef LM_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
