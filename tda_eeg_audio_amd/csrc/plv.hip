// plv.hip -- phase-locking value of the channels of a window and its distance matrix (include/tdaeeg.h, "Phase-locking
// value"), float64, gfx950.
//
// One 512-thread workgroup per window (the window alone is 94 KB of LDS: one workgroup a CU, so two waves a SIMD have to
// hide each other's LDS latency).  The window stays in LDS (row stride n_t | 1 doubles: lanes that differ in the channel
// hit different banks), the Hilbert table g twice over (GE[k] = g[k mod n_t]: no modulo in the loop).  All phasors of a
// 47 x 250 window are 188 KB, more than a CU has, so the time axis is taken in blocks of TB samples:
//   a. Hilbert values of the block: a thread takes one channel and T consecutive samples; over m it reads x[c][m] once and
//      slides a register window of g over it (one new value per m), T independent fma chains, sequential in m;
//      then the unit phasors of its samples into the block's tile U[t][c] (time-major double2, padded channels are (0, 0)).
//      For an even n_t every even entry of the host table is an exact zero (the kernel looks, it does not assume): the
//      products with them add +-0 and are left out, half of the chain, the same bytes
//   b. the complex Gram sums of the block: a thread owns a 2 x 4 tile of channel pairs (only tiles that reach above the
//      diagonal exist: nbt^2 + nbt <= 272 for nbt = ncp / 4 column tiles) and keeps its 8 (R, I) accumulators in registers
//      across the blocks, sequential in t
// TB is the largest of 64 / 32 / 16 whose tile fits beside the window and the kernel's static LDS (T = 8 / 4 / 4: up to
// TB / T * ncp = 512 tasks).
// At the end the matrix is staged in LDS over the window (pair (i, j), i < j, is computed once and stored at both places:
// symmetric as bytes) and every thread stores plv and dist rows coalesced.  No atomics, no global scratch.
#include "common.h"
#include <climits>

#define PLV_NT 512
#define PLV_LDS_MAX (160 * 1024)              // what a CU has: a workgroup's static and dynamic LDS together

// correlation_to_distance (nb2:100-122) on one value, the four methods of corr_to_dist_kernel restated (corr_dist.hip keeps
// its code object)
__device__ __forceinline__ double plv_to_dist(double r, int method)
{
    if (r > 1.0) r = 1.0;
    if (r < -1.0) r = -1.0;
    double d;
    if (method == 0) d = sqrt(2.0 * (1.0 - r));
    else if (method == 1) d = 1.0 - fabs(r);
    else if (method == 2) d = 1.0 - r;
    else d = sqrt(1.0 - r * r);
    if (d < 0.0) d = 0.0;
    return d;
}

__host__ __device__ inline int plv_xsz(int n_ch, int n_t)
{
    const int a = n_ch * (n_t | 1), b = n_ch * n_ch;
    return ((a > b ? a : b) + 1) & ~1;
}
static size_t plv_lds_bytes(int n_ch, int n_t, int tb)
{
    return (size_t)8 * (plv_xsz(n_ch, n_t) + 2 * n_t + 18) + (size_t)16 * tb * ((n_ch + 3) & ~3);
}

// Hilbert values of samples t0 .. t0 + T - 1 of the row xr: acc[j] = sum_m xr[m] * g[(t0 + j - m) mod n_t], sequential in m;
// ge = GE + t0 + n_t, so that ge[j - m] is that entry of g.  PAR: n_t and t0 are even and g[k] = 0 for every even k -- for
// an even m only the odd j have a term, for an odd m only the even j; W[k] = ge[2k - 1 - m] (m even) serves both.
template <int T, bool PAR>
__device__ __forceinline__ void plv_hilbert(const double* __restrict__ xr, const double* __restrict__ ge, int n_t, double* acc)
{
#pragma unroll
    for (int j = 0; j < T; ++j) acc[j] = 0.0;
    if constexpr (PAR) {
        constexpr int H = T / 2;
        double W[H + 1];
#pragma unroll
        for (int k = 0; k <= H; ++k) W[k] = ge[2 * k - 1];
#pragma unroll H
        for (int m = 0; m < n_t; m += 2) {
            const double x0 = xr[m], x1 = xr[m + 1];
#pragma unroll
            for (int k = 0; k < H; ++k) acc[2 * k + 1] = fma(x0, W[k + 1], acc[2 * k + 1]);
#pragma unroll
            for (int k = 0; k < H; ++k) acc[2 * k] = fma(x1, W[k], acc[2 * k]);
#pragma unroll
            for (int k = H; k > 0; --k) W[k] = W[k - 1];
            W[0] = ge[-(m + 3)];               // (the last one is not used: GE has two slots in front)
        }
    } else {
        double gw[T];
#pragma unroll
        for (int j = 0; j < T; ++j) gw[j] = ge[j];
#pragma unroll T
        for (int m = 0; m < n_t; ++m) {
            const double xv = xr[m];
#pragma unroll
            for (int j = 0; j < T; ++j) acc[j] = fma(xv, gw[j], acc[j]);
#pragma unroll
            for (int j = T - 1; j > 0; --j) gw[j] = gw[j - 1];
            gw[0] = ge[-(m + 1)];
        }
    }
}

template <int TB, int T>
__global__ void __launch_bounds__(PLV_NT)
plv_dist_kernel(const double* __restrict__ sig, const long long* __restrict__ win_start, const long long* __restrict__ win_ld,
                int n_ch, int n_t, const double* __restrict__ g, int method, double* __restrict__ dist,
                double* __restrict__ plv, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int ldx = n_t | 1, ncp = (n_ch + 3) & ~3, nn = n_ch * n_ch;
    double* X = reinterpret_cast<double*>(smem);
    double* GE = X + plv_xsz(n_ch, n_t) + 2;           // two slots in front: GE[-1], GE[-2] are addressable
    double2* U = reinterpret_cast<double2*>(GE + 2 * n_t + 16);
    const double* src = win_start ? sig + win_start[w] : sig + (size_t)w * n_ch * n_t;
    const long long ld = win_ld ? win_ld[w] : (long long)n_t;
    double* Dw = dist + (size_t)w * nn;
    double* Pw = plv ? plv + (size_t)w * nn : nullptr;

    // 1. the window and the table; lanes run along a row
    bool bad = false, odd_zero = (n_t & 1) != 0;       // odd_zero: the table does not have the zeros of an even length
    for (int e = tid; e < n_ch * n_t; e += PLV_NT) {
        const int c = e / n_t, t = e - c * n_t;
        const double v = src[c * ld + t];
        X[c * ldx + t] = v;
        bad |= !__builtin_isfinite(v);
    }
    for (int k = tid - 2; k < 2 * n_t + 16; k += PLV_NT) {
        const double v = k < 0 ? 0.0 : g[k % n_t];
        GE[k] = v;
        odd_zero |= k >= 0 && k < n_t && !(k & 1) && v != 0.0;
    }
    if (__syncthreads_or(bad)) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int e = tid; e < nn; e += PLV_NT) { Dw[e] = nan; if (Pw) Pw[e] = nan; }
        if (tid == 0) status[w] = TDA_WIN_NOT_FINITE;
        return;
    }
    const bool par = !__syncthreads_or(odd_zero);

    // the thread's tile: tile k of column tile b = rows 2a, 2a + 1 and columns 4b .. 4b + 3, a = k - (b^2 + b) <= 2b + 1
    const int nbt = ncp >> 2, n_tiles = nbt * nbt + nbt;
    const bool live = tid < n_tiles;
    int i0 = 0, j0 = 0;
    if (live) {
        int b = 0;
        while ((b + 1) * (b + 1) + (b + 1) <= tid) ++b;
        i0 = 2 * (tid - (b * b + b));
        j0 = 4 * b;
    }
    double aR[2][4], aI[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) aR[r][q] = aI[r][q] = 0.0;

    constexpr int NSUB = TB / T;
    for (int tb0 = 0; tb0 < n_t; tb0 += TB) {
        // a. Hilbert values and phasors of samples [tb0, tb0 + TB)
        for (int q = tid; q < NSUB * ncp; q += PLV_NT) {
            const int sub = q / ncp, c = q - sub * ncp, t0 = tb0 + sub * T;
            double2* Uq = U + (sub * T) * ncp + c;
            if (c < n_ch && t0 < n_t) {
                const double* xr = X + c * ldx;
                double acc[T];
                if (par) plv_hilbert<T, true>(xr, GE + t0 + n_t, n_t, acc);
                else plv_hilbert<T, false>(xr, GE + t0 + n_t, n_t, acc);
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    double2 u = make_double2(0.0, 0.0);
                    if (t0 + j < n_t) {
                        const double xv = xr[t0 + j], h = acc[j];
                        const double mag = sqrt(xv * xv + h * h);
                        u = mag == 0.0 ? make_double2(1.0, 0.0) : make_double2(xv / mag, h / mag);
                    }
                    Uq[j * ncp] = u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < T; ++j) Uq[j * ncp] = make_double2(0.0, 0.0);
            }
        }
        __syncthreads();
        // b. R + iI += u_i * conj(u_j) over the block's samples
        const int tlen = n_t - tb0 < TB ? n_t - tb0 : TB;
        if (live) {
            const double2* ui = U + i0;
            const double2* uj = U + j0;
#pragma unroll 2
            for (int tt = 0; tt < tlen; ++tt) {
                double2 a[2], b[4];
#pragma unroll
                for (int r = 0; r < 2; ++r) a[r] = ui[tt * ncp + r];
#pragma unroll
                for (int q = 0; q < 4; ++q) b[q] = uj[tt * ncp + q];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        aR[r][q] = fma(a[r].x, b[q].x, aR[r][q]);
                        aR[r][q] = fma(a[r].y, b[q].y, aR[r][q]);
                        aI[r][q] = fma(a[r].y, b[q].x, aI[r][q]);
                        aI[r][q] = fma(-a[r].x, b[q].y, aI[r][q]);
                    }
            }
        }
        __syncthreads();                   // the tile is read; the next block (or the matrix, over X) may be written
    }

    // 2. the matrix over the window: every pair once, stored at (i, j) and (j, i)
    const double den = (double)n_t;
    if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + r, j = j0 + q;
                if (i < j && j < n_ch) {
                    const double R = aR[r][q], I = aI[r][q];
                    const double p = sqrt(R * R + I * I) / den;
                    X[i * n_ch + j] = p;
                    X[j * n_ch + i] = p;
                }
            }
    }
    if (tid < n_ch) X[tid * n_ch + tid] = 1.0;
    __syncthreads();
    for (int e = tid; e < nn; e += PLV_NT) {
        const int i = e / n_ch, j = e - i * n_ch;
        const double p = X[e];
        if (Pw) Pw[e] = p;
        Dw[e] = i == j ? 0.0 : plv_to_dist(p, method);
    }
    if (tid == 0) status[w] = TDA_WIN_OK;
}

template <int TB, int T>
static tda_status plv_launch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                             int n_ch, int n_t, const double* g, int method, double* dist, double* plv, int* status,
                             hipStream_t st, bool* fits)
{
    const size_t lds = plv_lds_bytes(n_ch, n_t, TB);
    auto kern = plv_dist_kernel<TB, T>;
    // the kernel's static LDS (the workgroup reduction behind __syncthreads_or reserves some) lies in front of the dynamic
    // part: asked of the runtime once per instantiation; *fits = false leaves the shape to the next smaller tile
    static int lds_static = -1;
    if (lds_static < 0) {
        hipFuncAttributes attr;
        TDA_HIP(ctx, hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kern)));
        lds_static = (int)attr.sharedSizeBytes;
    }
    *fits = lds + (size_t)lds_static <= PLV_LDS_MAX;
    if (!*fits) return TDA_OK;
    if (lds > 48 * 1024)
        TDA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(n_win), dim3(PLV_NT), lds, st, sig, win_start, win_ld, n_ch, n_t, g, method, dist, plv, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_plv_dist(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                           int n_ch, int n_t, const double* g, int method, double* dist, double* plv, int* status,
                           hipStream_t st)
{
    if (n_ch < 2 || n_ch > TDA_PLV_MAX_CHANNELS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be in [2, TDA_PLV_MAX_CHANNELS]");
    if (n_t < 2 || n_t > TDA_PLV_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [2, TDA_PLV_MAX_SAMPLES]");
    if (method < 0 || method > 3) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown method");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    if (n_win == 0) return TDA_OK;
    // the largest tile that fits; the 16-sample one fits every shape inside the limits (64 x 256: 256 + 152,208 bytes)
    bool fits = false;
    tda_status rc = plv_launch<64, 8>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, plv, status, st, &fits);
    if (rc != TDA_OK || fits) return rc;
    rc = plv_launch<32, 4>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, plv, status, st, &fits);
    if (rc != TDA_OK || fits) return rc;
    rc = plv_launch<16, 4>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, method, dist, plv, status, st, &fits);
    if (rc == TDA_OK && !fits) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "window does not fit the LDS of a CU");
    return rc;
}
