// connectivity.hip -- analytic-signal connectivity of the channels of a window and its distance matrix: the weighted
// phase-lag index, the imaginary part of coherency, coherence and amplitude-envelope correlation (include/tdaeeg.h,
// "Analytic-signal connectivity"), float64, gfx950.
//
// The LDS plan of plv.hip: one 512-thread workgroup per window, the window resident in LDS (row stride
// n_t | 1 doubles), the Hilbert table g twice over (GE[k] = g[k mod n_t]), the time axis in blocks of TB samples:
//   a. Hilbert values of the block, a thread one channel and T consecutive samples (conn_hilbert: plv_hilbert restated, so
//      that plv.hip keeps its code object), then what the measure needs into the block's tile, time-major: (x, h) as a
//      double2 for wpli / imcoh / coh, the envelope sqrt(x*x + h*h) as a double for aec; padded channels are zeros
//   b. the pair sums of the block: a thread owns a 2 x 4 tile of channel pairs (the tiles of plv.hip, at most 272 threads) and
//      keeps its accumulators in registers across the blocks, sequential in t.  The kernel is instantiated per family, so
//      that no measure carries another's accumulators:
//        FAM_WPLI  s = h_i x_j - x_i h_j (two rounded products and their difference: exactly 0 for identical channels),
//                  S += s, A += |s|
//        FAM_COH   the same s, S += s, R = fma(x_i, x_j, R), R = fma(h_i, h_j, R)       (imcoh and coh)
//        FAM_AEC   C = fma(a_i - k_i, a_j - k_j, C); the shift k_c is the mean of channel c's envelope over the first block
//                  (covariance is shift-invariant; the shift only has to be near the mean)
//      beside them the last wave (threads 448 .. 511, never owners of a tile) keeps the per-channel sums, thread 448 + c
//      those of channel c, by the same operations in the same order as the pair sums: P = fma(x, x, P), P = fma(h, h, P);
//      for aec D1 += d, D2 = fma(d, d, D2), d = a - k.  So a duplicated channel has R == P_i == P_j and C == D2 as bytes.
// At the end the per-channel sums go to LDS (over the tile), the matrix is staged over the window (pair (i, j), i < j, computed
// once and stored at both places) and every thread stores value and dist rows coalesced.  No atomics, no global scratch.
#include "common.h"
#include <climits>

#define CONN_NT 512
#define CONN_STAT0 (CONN_NT - 64)             // first thread of the wave of the per-channel sums
#define CONN_LDS_MAX (160 * 1024)             // what a CU has: a workgroup's static and dynamic LDS together

enum { FAM_WPLI = 0, FAM_COH = 1, FAM_AEC = 2 };

// correlation_to_distance (nb2:100-122) on one value, the four methods of corr_to_dist_kernel restated (corr_dist.hip and
// plv.hip keep their code objects)
__device__ __forceinline__ double conn_to_dist(double r, int method)
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

__host__ __device__ inline int conn_xsz(int n_ch, int n_t)
{
    const int a = n_ch * (n_t | 1), b = n_ch * n_ch;
    return ((a > b ? a : b) + 1) & ~1;
}
// the tile is sized for the double2 families; aec's envelopes take the first half of it and its shifts K the second
static size_t conn_lds_bytes(int n_ch, int n_t, int tb)
{
    return (size_t)8 * (conn_xsz(n_ch, n_t) + 2 * n_t + 18) + (size_t)16 * tb * ((n_ch + 3) & ~3);
}

// Hilbert values of samples t0 .. t0 + T - 1 of the row xr: acc[j] = sum_m xr[m] * g[(t0 + j - m) mod n_t], sequential in m;
// ge = GE + t0 + n_t, so that ge[j - m] is that entry of g.  PAR: n_t and t0 are even and g[k] = 0 for every even k -- for
// an even m only the odd j have a term, for an odd m only the even j; W[k] = ge[2k - 1 - m] (m even) serves both.
template <int T, bool PAR>
__device__ __forceinline__ void conn_hilbert(const double* __restrict__ xr, const double* __restrict__ ge, int n_t, double* acc)
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

template <int FAM, int TB, int T>
__global__ void __launch_bounds__(CONN_NT)
connectivity_dist_kernel(const double* __restrict__ sig, const long long* __restrict__ win_start,
                         const long long* __restrict__ win_ld, int n_ch, int n_t, const double* __restrict__ g, int measure,
                         int method, double* __restrict__ dist, double* __restrict__ value, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int ldx = n_t | 1, ncp = (n_ch + 3) & ~3, nn = n_ch * n_ch;
    double* X = reinterpret_cast<double*>(smem);
    double* GE = X + conn_xsz(n_ch, n_t) + 2;          // two slots in front: GE[-1], GE[-2] are addressable
    double* TILE = GE + 2 * n_t + 16;                  // 2 * TB * ncp doubles
    double2* U = reinterpret_cast<double2*>(TILE);     // wpli / imcoh / coh: (x, h), U[t * ncp + c]
    double* K = TILE + TB * ncp;                       // aec: the envelopes are TILE[t * ncp + c], the shifts K[c]
    const double* src = win_start ? sig + win_start[w] : sig + (size_t)w * n_ch * n_t;
    const long long ld = win_ld ? win_ld[w] : (long long)n_t;
    double* Dw = dist + (size_t)w * nn;
    double* Vw = value ? value + (size_t)w * nn : nullptr;

    // 1. the window and the table; lanes run along a row
    bool bad = false, odd_zero = (n_t & 1) != 0;       // odd_zero: the table does not have the zeros of an even length
    for (int e = tid; e < n_ch * n_t; e += CONN_NT) {
        const int c = e / n_t, t = e - c * n_t;
        const double v = src[c * ld + t];
        X[c * ldx + t] = v;
        bad |= !__builtin_isfinite(v);
    }
    for (int k = tid - 2; k < 2 * n_t + 16; k += CONN_NT) {
        const double v = k < 0 ? 0.0 : g[k % n_t];
        GE[k] = v;
        odd_zero |= k >= 0 && k < n_t && !(k & 1) && v != 0.0;
    }
    if (__syncthreads_or(bad)) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int e = tid; e < nn; e += CONN_NT) { Dw[e] = nan; if (Vw) Vw[e] = nan; }
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
    const int pc = tid - CONN_STAT0;                   // the channel whose sums this thread keeps
    const bool stat = pc >= 0 && pc < n_ch;
    // a0: S (wpli, coh) or C (aec); a1: A (wpli) or R (coh).  c0: P (wpli, coh) or D1 (aec); c1: D2 (aec)
    double a0[2][4], a1[2][4], c0 = 0.0, c1 = 0.0;
    double ki[2] = {0.0, 0.0}, kj[4] = {0.0, 0.0, 0.0, 0.0}, kc = 0.0;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) a0[r][q] = a1[r][q] = 0.0;

    constexpr int NSUB = TB / T;
    for (int tb0 = 0; tb0 < n_t; tb0 += TB) {
        // a. Hilbert values of samples [tb0, tb0 + TB) and the tile
        for (int q = tid; q < NSUB * ncp; q += CONN_NT) {
            const int sub = q / ncp, c = q - sub * ncp, t0 = tb0 + sub * T;
            const int at = (sub * T) * ncp + c;
            if (c < n_ch && t0 < n_t) {
                const double* xr = X + c * ldx;
                double acc[T];
                if (par) conn_hilbert<T, true>(xr, GE + t0 + n_t, n_t, acc);
                else conn_hilbert<T, false>(xr, GE + t0 + n_t, n_t, acc);
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const bool in = t0 + j < n_t;
                    const double xv = in ? xr[t0 + j] : 0.0, h = in ? acc[j] : 0.0;
                    if constexpr (FAM == FAM_AEC) TILE[at + j * ncp] = sqrt(xv * xv + h * h);
                    else U[at + j * ncp] = make_double2(xv, h);
                }
            } else {
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    if constexpr (FAM == FAM_AEC) TILE[at + j * ncp] = 0.0;
                    else U[at + j * ncp] = make_double2(0.0, 0.0);
                }
            }
        }
        __syncthreads();
        const int tlen = n_t - tb0 < TB ? n_t - tb0 : TB;
        if constexpr (FAM == FAM_AEC) {
            if (tb0 == 0) {                            // the shifts: the first block's mean envelope of every channel
                if (pc >= 0 && pc < ncp) {
                    double s = 0.0;
                    if (pc < n_ch) {
                        for (int tt = 0; tt < tlen; ++tt) s += TILE[tt * ncp + pc];
                        s /= (double)tlen;
                    }
                    K[pc] = s;
                }
                __syncthreads();
                if (live) {
#pragma unroll
                    for (int r = 0; r < 2; ++r) ki[r] = K[i0 + r];
#pragma unroll
                    for (int q = 0; q < 4; ++q) kj[q] = K[j0 + q];
                }
                if (stat) kc = K[pc];
            }
        }
        // b. the pair sums and the per-channel sums over the block's samples
        if (live) {
            if constexpr (FAM == FAM_AEC) {
                const double* ei = TILE + i0;
                const double* ej = TILE + j0;
#pragma unroll 2
                for (int tt = 0; tt < tlen; ++tt) {
                    double a[2], b[4];
#pragma unroll
                    for (int r = 0; r < 2; ++r) a[r] = ei[tt * ncp + r] - ki[r];
#pragma unroll
                    for (int q = 0; q < 4; ++q) b[q] = ej[tt * ncp + q] - kj[q];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int q = 0; q < 4; ++q) a0[r][q] = fma(a[r], b[q], a0[r][q]);
                }
            } else {
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
                            const double p1 = a[r].y * b[q].x, p2 = a[r].x * b[q].y;
                            const double s = p1 - p2;
                            a0[r][q] += s;
                            if constexpr (FAM == FAM_WPLI) {
                                a1[r][q] += fabs(s);
                            } else {
                                a1[r][q] = fma(a[r].x, b[q].x, a1[r][q]);
                                a1[r][q] = fma(a[r].y, b[q].y, a1[r][q]);
                            }
                        }
                }
            }
        } else if (stat) {
            if constexpr (FAM == FAM_AEC) {
                for (int tt = 0; tt < tlen; ++tt) {
                    const double d = TILE[tt * ncp + pc] - kc;
                    c0 += d;
                    c1 = fma(d, d, c1);
                }
            } else {
                for (int tt = 0; tt < tlen; ++tt) {
                    const double2 u = U[tt * ncp + pc];
                    c0 = fma(u.x, u.x, c0);
                    c0 = fma(u.y, u.y, c0);
                }
            }
        }
        __syncthreads();                   // the tile is read; the next block (or the sums and the matrix) may be written
    }

    // 2. the per-channel sums over the tile: Q0[c] = P_c (aec: the envelope's centred sum of squares, 0 where it is flat),
    //    Q1[c] = D1_c (aec)
    double* Q0 = TILE;
    double* Q1 = TILE + ncp;
    const double den = (double)n_t;
    if (stat) {
        if constexpr (FAM == FAM_AEC) {
            const double var = c1 - c0 * c0 / den;
            const double tm = TDA_CONN_TAU * (kc + c0 / den);
            Q0[pc] = var > den * (tm * tm) ? var : 0.0;
            Q1[pc] = c0;
        } else {
            Q0[pc] = c0;
        }
    }
    __syncthreads();
    // 3. the matrix over the window: every pair once, stored at (i, j) and (j, i)
    if (live) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + r, j = j0 + q;
                if (i < j && j < n_ch) {
                    double v;
                    if constexpr (FAM == FAM_AEC) {
                        const double vi = Q0[i], vj = Q0[j];
                        const double cov = a0[r][q] - Q1[i] * Q1[j] / den;
                        v = (vi == 0.0 || vj == 0.0) ? 0.0 : cov / sqrt(vi * vj);
                    } else {
                        const double pp = Q0[i] * Q0[j], S = a0[r][q];
                        if constexpr (FAM == FAM_WPLI) {
                            const double A = a1[r][q];
                            v = A <= TDA_CONN_TAU * sqrt(pp) ? 0.0 : fabs(S) / A;
                        } else {
                            const double R = a1[r][q];
                            if (pp == 0.0) v = 0.0;
                            else if (measure == TDA_CONN_IMCOH) v = fabs(S) / sqrt(pp);
                            else v = sqrt(S * S + R * R) / sqrt(pp);
                        }
                    }
                    X[i * n_ch + j] = v;
                    X[j * n_ch + i] = v;
                }
            }
    }
    if (tid < n_ch) X[tid * n_ch + tid] = 1.0;
    __syncthreads();
    for (int e = tid; e < nn; e += CONN_NT) {
        const int i = e / n_ch, j = e - i * n_ch;
        const double v = X[e];
        if (Vw) Vw[e] = v;
        Dw[e] = i == j ? 0.0 : conn_to_dist(v, method);
    }
    if (tid == 0) status[w] = TDA_WIN_OK;
}

template <int FAM, int TB, int T>
static tda_status conn_launch(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                              int n_ch, int n_t, const double* g, int measure, int method, double* dist, double* value,
                              int* status, hipStream_t st, bool* fits)
{
    const size_t lds = conn_lds_bytes(n_ch, n_t, TB);
    auto kern = connectivity_dist_kernel<FAM, TB, T>;
    // the kernel's static LDS (the workgroup reduction behind __syncthreads_or reserves some) lies in front of the dynamic
    // part: asked of the runtime once per instantiation; *fits = false leaves the shape to the next smaller tile
    static int lds_static = -1;
    if (lds_static < 0) {
        hipFuncAttributes attr;
        TDA_HIP(ctx, hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kern)));
        lds_static = (int)attr.sharedSizeBytes;
    }
    *fits = lds + (size_t)lds_static <= CONN_LDS_MAX;
    if (!*fits) return TDA_OK;
    if (lds > 48 * 1024)
        TDA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(n_win), dim3(CONN_NT), lds, st, sig, win_start, win_ld, n_ch, n_t, g, measure, method, dist,
                       value, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// the largest tile that fits; the 16-sample one fits every shape inside the limits (64 x 256: 256 + 152,208 bytes)
template <int FAM>
static tda_status conn_ladder(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                              int n_ch, int n_t, const double* g, int measure, int method, double* dist, double* value,
                              int* status, hipStream_t st)
{
    bool fits = false;
    tda_status rc = conn_launch<FAM, 64, 8>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st, &fits);
    if (rc != TDA_OK || fits) return rc;
    rc = conn_launch<FAM, 32, 4>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st, &fits);
    if (rc != TDA_OK || fits) return rc;
    rc = conn_launch<FAM, 16, 4>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st, &fits);
    if (rc == TDA_OK && !fits) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "window does not fit the LDS of a CU");
    return rc;
}

tda_status launch_connectivity_dist(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld,
                                    int n_win, int n_ch, int n_t, const double* g, int measure, int method, double* dist,
                                    double* value, int* status, hipStream_t st)
{
    if (n_ch < 2 || n_ch > TDA_PLV_MAX_CHANNELS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be in [2, TDA_PLV_MAX_CHANNELS]");
    if (n_t < 2 || n_t > TDA_PLV_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [2, TDA_PLV_MAX_SAMPLES]");
    if (measure < 0 || measure > TDA_CONN_AEC) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown measure");
    if (method < 0 || method > 3) TDA_FAIL(ctx, TDA_ERR_INVALID, "Unknown method");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    if (n_win == 0) return TDA_OK;
    if (measure == TDA_CONN_WPLI)
        return conn_ladder<FAM_WPLI>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st);
    if (measure == TDA_CONN_AEC)
        return conn_ladder<FAM_AEC>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st);
    return conn_ladder<FAM_COH>(ctx, sig, win_start, win_ld, n_win, n_ch, n_t, g, measure, method, dist, value, status, st);
}
