// embedding.hip -- the two parameters of a delay embedding, chosen from the signal itself: the delay at the first minimum of
// the average mutual information (ami_kernel) and the dimension at which the false nearest neighbours vanish (fnn_kernel)
// (include/tdaeeg.h, "Delay and dimension selection").  The integers are the bits of tests/embedding_ref.py
// or they are wrong; so is every float64 of fnn_kernel, whose operations the header writes out one by one.  The mutual
// information holds the rounding of log and of a sum in this file's own fixed order.
//
// ami_kernel: one workgroup of 256 threads (four waves) per window.
//   a.  Minimum, maximum and the finite test in one sweep of the window from global memory; the waves meet once in LDS.
//   b.  The bin of every sample as a byte in LDS (n_t bytes), by the header's three operations.
//   c.  A wave per lag: wave w of round r takes L = 4 r + w and has its own n_bins x n_bins histogram in LDS (rows padded by
//       one word, so that row sums and column sums both run over distinct banks).  The counts are integer LDS atomics of the
//       wave on its own histogram: integer addition commutes, the table is bytes.  Lanes 0..31 then hold the row sums, lanes
//       32..63 the column sums; every lane adds the terms of its cells c = lane, lane + 64, ... in that order and the wave
//       adds the 64 partial sums on the xor butterfly (the same value in every lane).  One order, the same for a window alone
//       and in a batch.
//   d.  The first minimum is read off the values as they are stored: a ring in LDS holds the two values before the round and
//       the round's own, every thread makes the same comparisons.  Two barriers per round.  Without ami and joint (the
//       segments form) the rounds end with the first minimum.
//   Loop bounds, all known before the loop starts: n_t, max_lag, n_bins.  No float atomics, no global atomics, no polls.
//
// fnn_kernel: one workgroup of 256 threads per window, the window in LDS (8 n_t bytes).
//   A thread owns point i (and i + 256, ... above 256 points).  j is a wave-uniform loop: x[j + k tau] is an LDS broadcast.
//   The running sum s of the header is carried from d to d + 1 -- D2_{d+1} = D2_d + e * e is the written order -- so all
//   d_max dimensions cost one sweep of the pairs, with the best distance and its j of every dimension in registers.  Which
//   dimensions a pair (i, j) has: i + d tau < n_t is the lane's own (di), j + d tau < n_t is wave-uniform (a branch).
//   Counts: ballots and popcounts per wave, the waves meet once in LDS.  No atomics.  Loop bounds: n_t, d_max.
#include "common.h"

#define AMI_NT 256
#define AMI_WAVES (AMI_NT / 64)
#define FNN_NT 256
#define FNN_WAVES (FNN_NT / 64)

// the LDS accesses of ONE wave are served in program order: a compiler fence orders a wave's own histogram
__device__ __forceinline__ void emb_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool emb_finite(double v)
{
    return ((u32)(__double_as_longlong(v) >> 32) & 0x7ff00000u) != 0x7ff00000u;
}

// bytes of LDS of ami_kernel: ring | per-wave min, max | per-wave flag | histograms | bins
static size_t ami_lds_bytes(int n_t, int n_bins)
{
    return (size_t)(AMI_WAVES + 2) * 8 + 2 * AMI_WAVES * 8 + AMI_WAVES * 4 + (size_t)AMI_WAVES * n_bins * (n_bins + 1) * 4 +
           (size_t)n_t;
}

// seg_off != nullptr: workgroup g handles the FIRST window of group g, as tau_kernel, and writes the delay (with
// compute_tau's fallback) to every window of the group in tau_win; ami, joint and status are NULL then.
__global__ void __launch_bounds__(AMI_NT)
ami_kernel(const double* __restrict__ win, int n_t, int max_lag, int n_bins, double* __restrict__ ami, int* __restrict__ tau,
           int* __restrict__ joint, int* __restrict__ status, const int* __restrict__ seg_off, int* __restrict__ tau_win)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* ring = reinterpret_cast<double*>(smem);                // I(L0 - 2), I(L0 - 1), then the round's I(L0 + w)
    double* red = ring + AMI_WAVES + 2;                            // per-wave minimum, then per-wave maximum
    int* flag = reinterpret_cast<int*>(red + 2 * AMI_WAVES);       // per-wave: a sample that is not finite
    int* hist_all = flag + AMI_WAVES;
    const int hs = n_bins * (n_bins + 1), cells = n_bins * n_bins, ld = n_bins + 1;
    unsigned char* bin = reinterpret_cast<unsigned char*>(hist_all + AMI_WAVES * hs);
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int w = g, w_end = g + 1;
    if (seg_off) {
        w = seg_off[g]; w_end = seg_off[g + 1];
        if (w_end <= w) { if (tid == 0) tau[g] = 0; return; }      // empty group
    }
    const double* x = win + (size_t)w * n_t;
    const int n_lag = max_lag + 1;

    // a. minimum, maximum, finite
    double lo = __longlong_as_double(0x7ff0000000000000ll), hi = -lo;
    bool bad = false;
    for (int t = tid; t < n_t; t += AMI_NT) {
        const double v = x[t];
        bad |= !emb_finite(v);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    lo = wave_min_f64_dpp(lo);
    hi = wave_max_f64_dpp(hi);
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) { red[wave] = lo; red[AMI_WAVES + wave] = hi; flag[wave] = wave_bad; }
    __syncthreads();
    int any_bad = 0;
#pragma unroll
    for (int k = 0; k < AMI_WAVES; ++k) {
        const double a = red[k], b = red[AMI_WAVES + k];
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        any_bad |= flag[k];
    }
    const int st = any_bad ? TDA_WIN_NOT_FINITE : (hi == lo ? TDA_WIN_DEGENERATE : 0);
    if (status && tid == 0) status[g] = st;
    int found = 0;
    if (st) {
        const double fill = any_bad ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
        if (ami)
            for (int i = tid; i < n_lag; i += AMI_NT) ami[(size_t)g * n_lag + i] = fill;
        if (joint) {
            int* jw = joint + (size_t)g * n_lag * cells;
            for (size_t i = tid; i < (size_t)n_lag * cells; i += AMI_NT) jw[i] = 0;
        }
    } else {
        // b. bins
        const double wd = hi - lo, nb = (double)n_bins;
        for (int t = tid; t < n_t; t += AMI_NT) {
            const double u = ((x[t] - lo) / wd) * nb;
            const int b = (int)u;
            bin[t] = (unsigned char)(b < n_bins - 1 ? b : n_bins - 1);
        }
        __syncthreads();
        // c. a wave per lag, four lags per round
        const bool need_all = ami != nullptr || joint != nullptr;
        int* h = hist_all + wave * hs;
        for (int L0 = 0; L0 <= max_lag; L0 += AMI_WAVES) {
            const int L = L0 + wave;
            if (L <= max_lag) {
                const int N = n_t - L;
                for (int c = lane; c < hs; c += 64) h[c] = 0;
                emb_wave_sync();
                for (int i = lane; i < N; i += 64) atomicAdd(&h[(int)bin[i] * ld + (int)bin[i + L]], 1);
                emb_wave_sync();
                // lanes 0..31: r_p of row p = lane; lanes 32..63: s_q of column q = lane - 32
                int marg = 0;
                {
                    const int p = lane & 31;
                    if (p < n_bins) {
                        const int base = lane < 32 ? p * ld : p, step = lane < 32 ? 1 : ld;
                        for (int q = 0; q < n_bins; ++q) marg += h[base + q * step];
                    }
                }
                int* jw = joint ? joint + ((size_t)g * n_lag + L) * cells : nullptr;
                const double dn = (double)N;
                double acc = 0.0;
                for (int c0 = 0; c0 < cells; c0 += 64) {
                    const int c = c0 + lane;
                    const bool in = c < cells;
                    const int p = in ? c / n_bins : 0, q = in ? c - p * n_bins : 0;
                    const int J = in ? h[p * ld + q] : 0;
                    const int rp = __shfl(marg, p, 64), sq = __shfl(marg, 32 + q, 64);
                    if (jw && in) jw[c] = J;
                    if (J > 0) acc = acc + ((double)J / dn) * log((double)(J * N) / (double)(rp * sq));
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
                if (lane == 0) {
                    ring[2 + wave] = acc;
                    if (ami) ami[(size_t)g * n_lag + L] = acc;
                }
                emb_wave_sync();                                   // the histogram is read before the next round clears it
            }
            __syncthreads();
            // d. the candidates whose right neighbour this round has written: L0 - 1 .. L0 + AMI_WAVES - 2
            if (!found) {
#pragma unroll
                for (int k = 0; k < AMI_WAVES; ++k) {
                    const int Lc = L0 - 1 + k;
                    if (Lc >= 1 && Lc + 1 <= max_lag && !found) {
                        const double a = ring[k], b = ring[k + 1], c = ring[k + 2];
                        if (b < a && b <= c) found = Lc;
                    }
                }
            }
            const double keep0 = ring[AMI_WAVES], keep1 = ring[AMI_WAVES + 1];
            __syncthreads();
            if (tid == 0) { ring[0] = keep0; ring[1] = keep1; }
            if (found && !need_all) break;                         // (workgroup-uniform)
        }
    }
    if (seg_off && !found) { found = max_lag / 10; if (found < 1) found = 1; }     // compute_tau's fallback
    if (tid == 0) tau[g] = found;
    if (tau_win)
        for (int i = w + tid; i < w_end; i += AMI_NT) tau_win[i] = found;
}

__global__ void __launch_bounds__(FNN_NT)
fnn_kernel(const double* __restrict__ win, const int* __restrict__ tau_in, int n_t, int d_max, int theiler, double r_tol,
           double a_tol, double frac_tol, int* __restrict__ counts, double* __restrict__ frac, int* __restrict__ dim,
           int* __restrict__ nn, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* xs = reinterpret_cast<double*>(smem);                  // the window
    int* part = reinterpret_cast<int*>(xs + n_t);                  // per wave TDA_FNN_MAX_DIM x TDA_FNN_COLS counts
    int* tot = part + FNN_WAVES * TDA_FNN_MAX_DIM * TDA_FNN_COLS;   // their sums
    int* flag = tot + TDA_FNN_MAX_DIM * TDA_FNN_COLS;
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* x = win + (size_t)g * n_t;
    int* cnt_out = counts + (size_t)g * d_max * TDA_FNN_COLS;
    double* frac_out = frac + (size_t)g * d_max;
    int* nn_out = nn ? nn + (size_t)g * d_max * n_t : nullptr;

    bool bad = false;
    for (int t = tid; t < n_t; t += FNN_NT) {
        const double v = x[t];
        xs[t] = v;
        bad |= !emb_finite(v);
    }
    const bool wave_bad = __ballot(bad) != 0ull;
    if (lane == 0) flag[wave] = wave_bad;
    __syncthreads();
    int any_bad = 0;
#pragma unroll
    for (int k = 0; k < FNN_WAVES; ++k) any_bad |= flag[k];
    const int tau = tau_in[g];
    const int st = any_bad ? TDA_WIN_NOT_FINITE : tau < 1 ? TDA_WIN_TOO_LARGE : (n_t - tau < 2 ? TDA_WIN_DEGENERATE : 0);
    if (tid == 0) status[g] = st;
    if (st) {
        for (int i = tid; i < d_max * TDA_FNN_COLS; i += FNN_NT) cnt_out[i] = 0;
        for (int i = tid; i < d_max; i += FNN_NT) frac_out[i] = 0.0;
        if (tid == 0) dim[g] = 0;
        if (nn_out)
            for (int i = tid; i < d_max * n_t; i += FNN_NT) nn_out[i] = -1;
        return;
    }
    // R2: every thread the same two sequential sums (1 <= tau <= n_t - 2 from here on)
    double S = 0.0;
    for (int t = 0; t < n_t; ++t) S = S + xs[t];
    const double m = S / (double)n_t;
    S = 0.0;
    for (int t = 0; t < n_t; ++t) { const double dv = xs[t] - m; S = S + dv * dv; }
    const double R2 = (a_tol * a_tol) * (S / (double)n_t), rr = r_tol * r_tol;

    const int M1 = n_t - tau;
    int cnt[TDA_FNN_MAX_DIM][TDA_FNN_COLS];
#pragma unroll
    for (int k = 0; k < TDA_FNN_MAX_DIM; ++k)
#pragma unroll
        for (int c = 0; c < TDA_FNN_COLS; ++c) cnt[k][c] = 0;

    for (int i0 = 0; i0 < M1; i0 += FNN_NT) {
        const int i = i0 + tid;
        double xi[TDA_FNN_MAX_DIM], best[TDA_FNN_MAX_DIM];
        int bj[TDA_FNN_MAX_DIM];
        int di = 0;                                                // the dimensions d <= di have the point i: i < M_d
#pragma unroll
        for (int k = 0; k < TDA_FNN_MAX_DIM; ++k) {
            xi[k] = (k < d_max && i + k * tau < n_t) ? xs[i + k * tau] : 0.0;
            best[k] = 0.0; bj[k] = -1;
            if (k < d_max && i + (k + 1) * tau < n_t) di = k + 1;
        }
        for (int j = 0; j < M1; ++j) {
            const int dist = i > j ? i - j : j - i;
            const bool cand = dist >= theiler;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < TDA_FNN_MAX_DIM; ++k) {
                if (k >= d_max || j + (k + 1) * tau >= n_t) break;         // (wave-uniform) j < M_{k+1}
                const double e = xi[k] - xs[j + k * tau];
                s = s + e * e;
                const bool take = cand && k < di && (bj[k] < 0 || s < best[k]);
                best[k] = take ? s : best[k];
                bj[k] = take ? j : bj[k];
            }
        }
#pragma unroll
        for (int k = 0; k < TDA_FNN_MAX_DIM; ++k) {
            if (k >= d_max) break;
            const int d = k + 1;
            const bool has = k < di && bj[k] >= 0;
            bool c1 = false, c2 = false;
            if (has) {
                const double e = xs[i + d * tau] - xs[bj[k] + d * tau];
                const double e2 = e * e, D2 = best[k];
                c1 = D2 > 0.0 ? e2 > rr * D2 : e2 > 0.0;
                c2 = (D2 + e2) > R2;
            }
            cnt[k][0] += __popcll(__ballot(has));
            cnt[k][1] += __popcll(__ballot(c1));
            cnt[k][2] += __popcll(__ballot(c2));
            cnt[k][3] += __popcll(__ballot(c1 || c2));
            if (nn_out && i < M1) nn_out[(size_t)k * n_t + i] = has ? bj[k] : -1;
        }
    }
    if (nn_out)
        for (int k = 0; k < d_max; ++k)
            for (int i = M1 + tid; i < n_t; i += FNN_NT) nn_out[(size_t)k * n_t + i] = -1;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < TDA_FNN_MAX_DIM; ++k)
#pragma unroll
            for (int c = 0; c < TDA_FNN_COLS; ++c) part[(wave * TDA_FNN_MAX_DIM + k) * TDA_FNN_COLS + c] = cnt[k][c];
    }
    __syncthreads();
    if (tid < TDA_FNN_MAX_DIM * TDA_FNN_COLS) {
        int s = 0;
#pragma unroll
        for (int wv = 0; wv < FNN_WAVES; ++wv) s += part[wv * TDA_FNN_MAX_DIM * TDA_FNN_COLS + tid];
        tot[tid] = s;
        if (tid < d_max * TDA_FNN_COLS) cnt_out[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int first = 0;
        for (int k = 0; k < d_max; ++k) {
            const int valid = tot[k * TDA_FNN_COLS], either = tot[k * TDA_FNN_COLS + 3];
            frac_out[k] = valid ? (double)either / (double)valid : 0.0;
            if (!first && valid > 0 && (double)either <= frac_tol * (double)valid) first = k + 1;
        }
        dim[g] = first;
    }
}

tda_status ami_check(tda_ctx* ctx, int n_t, int n_bins, int* max_lag)
{
    if (n_t < 4 || n_t > TDA_AMI_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "ami: n_t must be in [4, TDA_AMI_MAX_SAMPLES]");
    if (n_bins < 2 || n_bins > TDA_AMI_MAX_BINS) TDA_FAIL(ctx, TDA_ERR_INVALID, "ami: n_bins must be in [2, TDA_AMI_MAX_BINS]");
    if (*max_lag < 0) *max_lag = n_t / 4;
    if (*max_lag > n_t - 2) *max_lag = n_t - 2;
    return TDA_OK;
}

tda_status launch_ami(tda_ctx* ctx, const double* win, const int* seg_off, int n_groups, int n_t, int max_lag, int n_bins,
                      double* ami, int* tau, int* joint, int* status, int* tau_win, hipStream_t st)
{
    TDA_TRY(ami_check(ctx, n_t, n_bins, &max_lag));
    if (n_groups == 0) return TDA_OK;
    hipLaunchKernelGGL(ami_kernel, dim3(n_groups), dim3(AMI_NT), ami_lds_bytes(n_t, n_bins), st, win, n_t, max_lag, n_bins, ami,
                       tau, joint, status, seg_off, tau_win);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status fnn_check(tda_ctx* ctx, int n_t, int d_max, int theiler, double r_tol, double a_tol, double frac_tol)
{
    if (n_t < 4 || n_t > TDA_FNN_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "fnn: n_t must be in [4, TDA_FNN_MAX_SAMPLES]");
    if (d_max < 1 || d_max > TDA_FNN_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "fnn: d_max must be in [1, TDA_FNN_MAX_DIM]");
    if (theiler < 1 || theiler > n_t) TDA_FAIL(ctx, TDA_ERR_INVALID, "fnn: theiler must be in [1, n_t]");
    if (!(r_tol > 0.0) || !(a_tol > 0.0)) TDA_FAIL(ctx, TDA_ERR_INVALID, "fnn: r_tol and a_tol must be > 0");
    if (!(frac_tol >= 0.0 && frac_tol <= 1.0)) TDA_FAIL(ctx, TDA_ERR_INVALID, "fnn: frac_tol must be in [0, 1]");
    return TDA_OK;
}

tda_status launch_fnn(tda_ctx* ctx, const double* win, const int* tau, int n_win, int n_t, int d_max, int theiler, double r_tol,
                      double a_tol, double frac_tol, int* counts, double* frac, int* dim, int* nn, int* status, hipStream_t st)
{
    TDA_TRY(fnn_check(ctx, n_t, d_max, theiler, r_tol, a_tol, frac_tol));
    if (n_win == 0) return TDA_OK;
    const size_t lds = (size_t)n_t * 8 + (size_t)(FNN_WAVES + 1) * TDA_FNN_MAX_DIM * TDA_FNN_COLS * 4 + FNN_WAVES * 4;
    hipLaunchKernelGGL(fnn_kernel, dim3(n_win), dim3(FNN_NT), lds, st, win, tau, n_t, d_max, theiler, r_tol, a_tol, frac_tol,
                       counts, frac, dim, nn, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
