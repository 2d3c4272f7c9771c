// recurrence.hip -- recurrence quantification of a window on a grid of scales: the recurrence plot R_g is the adjacency
// matrix of the thresholded graph on the vertices in time order, with a Theiler band cleared around the diagonal; the
// kernel counts its points and reads its diagonal and vertical lines (include/tdaeeg.h, "Recurrence curves"; DESIGN.md
// 3.25).  The integers are the bits of tests/recurrence_ref.py or they are wrong; the float64 measures are written
// functions of those integers in one written order of IEEE operations.
//
// One workgroup of 256 threads (four waves) per window, as csrc/network.hip.
//   Keys.   window_keys of csrc/rips_keys_dev.h fills the LDS triangle; its workgroup barriers all come before the grid loop.
//   Grid.   A wave per grid point: wave w takes the grid points w, w + 4, ...  Nothing inside the grid loop waits for
//           another wave, and the masks never leave the registers.  Lane v owns row / column v (and v + 64 above 64 points),
//           diagonal v (and v + 64) and the line length v + 1 (and v + 65).
//     a.    A[v] = { u : |u - v| >= theiler and the edge {u, v} is present }, one u64 per 64 vertices, read from the triangle
//           as network.hip reads it.  R is symmetric, so A[v] is column v: the vertical lines are the runs of its bits.
//     b.    Diagonals.  Lane i shifts its row down by i, so that bit k is R[i][i + k]; the mask of diagonal k over the rows i
//           is the ballot of bit k, and lane k keeps it.  Only k >= theiler of the upper triangle: the lower one is its
//           mirror and every diagonal count is doubled.
//     c.    Run lengths by erosion: E_1 = m, E_{l+1} = E_l & (E_l >> 1) keeps bit i while the run that starts at i has more
//           than l bits, so C_l = sum over the lines of popc(E_l) = sum over the runs of max(len - l + 1, 0).  One loop over l
//           erodes the columns and the diagonals together; the two popcounts share one wave sum (16 bits each: C_l <=
//           128 * 127 < 2^16), and lane l - 1 keeps C_l.  Then H(l) = C_l - 2 C_{l+1} + C_{l+2}, the lines of length >= l are
//           C_l - C_{l+1}, their points C_l + (l - 1)(C_l - C_{l+1}), and the longest line is the last l with C_l > 0.
//     d.    Entropy: every lane has p log p of its own length; the sum runs over the lengths that occur, in ascending order,
//           the same chain of subtractions in every lane.
//     e.    The edge sets of two grid points are nested, so a wave whose recurrence count equals that of its previous grid
//           point has the same plot in hand and keeps that grid point's results (they live in registers).
//   Loop bounds, all known before the loop starts: n, n_grid, n_hist, a popcount.  No polls, no atomics, nothing is
//   allocated.
// What diverges: nothing inside a grid point but the tail of (a) for lanes past n; the l loop of (c) is wave-uniform.
//
// The group means are up to three launches of group_mean_kernel (common.h): int32 in int64 for counts and hist, float64
// added in window order for measures.
#include "common.h"
#include "rips_keys_dev.h"

#define RQ_NT 256
#define RQ_WAVES (RQ_NT / 64)

__device__ __forceinline__ u32 rq_wave_sum(u32 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (u32)__shfl_xor((int)v, m, 64);
    return v;
}

// C[idx >> 6] of lane idx & 63; 0 past the last word
template <int NW>
__device__ __forceinline__ u32 rq_at(const u32 (&C)[NW], int idx)
{
    u32 r = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const u32 x = (u32)__shfl((int)C[w], idx & 63, 64);
        r = (idx >> 6) == w ? x : r;
    }
    return r;
}

// one erosion step of a mask of NW words: bit i stays while bit i + 1 is set too
template <int NW>
__device__ __forceinline__ void rq_erode(u64 (&E)[NW])
{
#pragma unroll
    for (int w = 0; w < NW; ++w) E[w] &= (E[w] >> 1) | (w + 1 < NW ? E[w + 1 < NW ? w + 1 : w] << 63 : 0ull);
}

// S = 0.0; for l ascending with H(l) > 0 and l >= lo: p = (double)H(l) / (double)lines; S = S - p * log(p).  Lane v holds
// H(v + 1 + 64 j) in H[j]; every lane returns S.
template <int NW>
__device__ __forceinline__ double rq_entropy(const u32 (&H)[NW], u32 lines, int lo, int lane)
{
    double term[NW];
    u64 has[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const bool ok = H[j] > 0 && lane + 64 * j + 1 >= lo;
        const double p = ok ? (double)H[j] / (double)lines : 1.0;
        term[j] = p * log(p);
        has[j] = __ballot(ok);
    }
    double S = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        u64 f = has[j];
        while (f) {
            const int bit = __builtin_ctzll(f);
            f &= f - 1;
            S = S - __shfl(term[j], bit, 64);
        }
    }
    return S;
}

template <int NW>
__global__ void __launch_bounds__(RQ_NT)
recurrence_kernel(WinSrc src, float thresh, KeyLayout L, const double* __restrict__ grid, int n_grid, int theiler, int l_min,
                  int v_min, int n_hist, int* __restrict__ counts, double* __restrict__ measures, int* __restrict__ hist,
                  int* __restrict__ n_points, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float* key = reinterpret_cast<const float*>(smem);
    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* cnt_out = counts + (size_t)win * TDA_RQA_ROWS * n_grid;
    double* mea_out = measures + (size_t)win * TDA_RQA_MEASURES * n_grid;
    const size_t hist_len = (size_t)2 * n_grid * n_hist;
    int* his_out = hist ? hist + (size_t)win * hist_len : nullptr;

    const WinExtent X = win_extent(src, win);
    const int st = win_status(src, X, win, n_points);
    if (tid == 0) status[win] = st;
    if (st) {
        for (int i = tid; i < TDA_RQA_ROWS * n_grid; i += RQ_NT) cnt_out[i] = 0;
        for (int i = tid; i < TDA_RQA_MEASURES * n_grid; i += RQ_NT) mea_out[i] = 0.0;
        if (his_out)
            for (size_t i = tid; i < hist_len; i += RQ_NT) his_out[i] = 0;
        return;
    }
    const int n = (int)X.P;
    window_keys<RQ_NT>(src, X, n, smem, L);

    // the ordered pairs outside the band
    const u32 n_out = theiler <= n ? (u32)(n - theiler) * (u32)(n - theiler + 1) : 0u;
    // what a grid point leaves behind; HD(l), HV(l) of this lane's lengths l = lane + 64 j + 1
    u32 Hd[NW], Hv[NW];
    u32 rec = 0, d_lines = 0, d_points = 0, d_long = 0, v_lines = 0, v_points = 0, v_long = 0;
    double d_ent = 0.0, v_ent = 0.0;
    u32 prev_rec = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) Hd[j] = Hv[j] = 0;

    for (int g = wave; g < n_grid; g += RQ_WAVES) {
        const double t = grid[g];
        // a. rows of the plot: adjacency masks without the band
        u64 A[NW][NW];
        u32 pc = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int v = lane + 64 * j;
#pragma unroll
            for (int w = 0; w < NW; ++w) A[j][w] = 0ull;
            if (v < n) {
                const float* row = key + tri2(v);
                for (int u = 0; u < n; ++u) {
                    const int d = u > v ? u - v : v - u;
                    if (d < theiler) continue;
                    const float k = u < v ? row[u] : key[tri2(u) + v];
                    const bool in = k <= thresh && (double)k <= t;
                    if (NW == 1) A[j][0] |= (u64)in << u;
                    else A[j][u >> 6] |= (u64)in << (u & 63);
                }
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) pc += (u32)__popcll(A[j][w]);
        }
        rec = rq_wave_sum(pc);
        // e. nested edge sets ({k <= min(t, thresh)}) under one band: equal counts mean equal plots
        const bool again = g != wave && rec == prev_rec;
        prev_rec = rec;
        if (!again) {
            // b. the diagonals of the upper triangle: S[j] = row v shifted down by v, bit k = R[v][v + k]
            u64 S[NW][NW], D[NW][NW];
            if (NW == 1) {
                S[0][0] = A[0][0] >> lane;
            } else {
                S[0][0] = lane ? (A[0][0] >> lane) | (A[0][NW - 1] << (64 - lane)) : A[0][0];
                S[0][NW - 1] = A[0][NW - 1] >> lane;
                S[NW - 1][0] = A[NW - 1][NW - 1] >> lane;
                S[NW - 1][NW - 1] = 0ull;
            }
#pragma unroll
            for (int j = 0; j < NW; ++j)
#pragma unroll
                for (int w = 0; w < NW; ++w) D[j][w] = 0ull;
            for (int k = theiler; k < n; ++k) {
                u64 b[NW];
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    const u64 word = (NW > 1 && k >= 64) ? S[j][NW - 1] : S[j][0];
                    b[j] = __ballot((int)((word >> (k & 63)) & 1ull));
                }
                if (lane == (k & 63)) {
#pragma unroll
                    for (int j = 0; j < NW; ++j)
                        if (j == (k >> 6)) {
#pragma unroll
                            for (int w = 0; w < NW; ++w) D[j][w] = b[w];
                        }
                }
            }
            // c. erosion: C_l of the columns in the low half, of the diagonals in the high half, in lane l - 1
            u32 Cl[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) Cl[j] = 0;
            v_long = d_long = 0;
            for (int l = 1; l < n; ++l) {
                u32 pv = 0, pd = 0;
#pragma unroll
                for (int j = 0; j < NW; ++j)
#pragma unroll
                    for (int w = 0; w < NW; ++w) { pv += (u32)__popcll(A[j][w]); pd += (u32)__popcll(D[j][w]); }
                const u32 c = rq_wave_sum(pv | (pd << 16));
                if (c == 0) break;
                v_long = (c & 0xffffu) ? (u32)l : v_long;
                d_long = (c >> 16) ? (u32)l : d_long;
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (j == ((l - 1) >> 6) && lane == ((l - 1) & 63)) Cl[j] = c;
#pragma unroll
                for (int j = 0; j < NW; ++j) { rq_erode<NW>(A[j]); rq_erode<NW>(D[j]); }
            }
            // histograms of this lane's lengths; both triangles for the diagonals
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int idx = lane + 64 * j;
                const u32 c0 = Cl[j], c1 = rq_at<NW>(Cl, idx + 1), c2 = rq_at<NW>(Cl, idx + 2);
                Hv[j] = (c0 & 0xffffu) - 2u * (c1 & 0xffffu) + (c2 & 0xffffu);
                Hd[j] = 2u * ((c0 >> 16) - 2u * (c1 >> 16) + (c2 >> 16));
            }
            // lines of at least l_min / v_min and their points
            {
                const u32 a = rq_at<NW>(Cl, l_min - 1) >> 16, b = rq_at<NW>(Cl, l_min) >> 16;
                d_lines = 2u * (a - b);
                d_points = 2u * (a + (u32)(l_min - 1) * (a - b));
                const u32 e = rq_at<NW>(Cl, v_min - 1) & 0xffffu, f = rq_at<NW>(Cl, v_min) & 0xffffu;
                v_lines = e - f;
                v_points = e + (u32)(v_min - 1) * (e - f);
            }
            // d. entropies
            d_ent = rq_entropy<NW>(Hd, d_lines, l_min, lane);
            v_ent = rq_entropy<NW>(Hv, v_lines, v_min, lane);
        }
        if (lane == 0) {
            cnt_out[0 * n_grid + g] = (int)rec;
            cnt_out[1 * n_grid + g] = (int)d_lines;
            cnt_out[2 * n_grid + g] = (int)d_points;
            cnt_out[3 * n_grid + g] = (int)d_long;
            cnt_out[4 * n_grid + g] = (int)v_lines;
            cnt_out[5 * n_grid + g] = (int)v_points;
            cnt_out[6 * n_grid + g] = (int)v_long;
            mea_out[0 * n_grid + g] = n_out ? (double)rec / (double)n_out : 0.0;
            mea_out[1 * n_grid + g] = rec ? (double)d_points / (double)rec : 0.0;
            mea_out[2 * n_grid + g] = d_lines ? (double)d_points / (double)d_lines : 0.0;
            mea_out[3 * n_grid + g] = d_ent;
            mea_out[4 * n_grid + g] = rec ? (double)v_points / (double)rec : 0.0;
            mea_out[5 * n_grid + g] = v_lines ? (double)v_points / (double)v_lines : 0.0;
            mea_out[6 * n_grid + g] = v_ent;
        }
        if (his_out) {
            for (int i = lane; i < n_hist; i += 64) {
                u32 hd = 0, hv = 0;
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (i == lane + 64 * j) { hd = Hd[j]; hv = Hv[j]; }
                his_out[((size_t)0 * n_grid + g) * n_hist + i] = (int)hd;
                his_out[((size_t)1 * n_grid + g) * n_hist + i] = (int)hv;
            }
        }
    }
}

tda_status rq_check(tda_ctx* ctx, int n_grid, int theiler, int l_min, int v_min)
{
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]");
    if (theiler < 1 || theiler > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "theiler must be in [1, TDA_MAX_POINTS]");
    if (l_min < 1 || l_min > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "l_min must be in [1, TDA_MAX_POINTS]");
    if (v_min < 1 || v_min > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "v_min must be in [1, TDA_MAX_POINTS]");
    return TDA_OK;
}

tda_status launch_recurrence(tda_ctx* ctx, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid,
                             int theiler, int l_min, int v_min, int* counts, double* measures, int* hist, int* n_points,
                             int* status, hipStream_t st)
{
    TDA_TRY(rq_check(ctx, n_grid, theiler, l_min, v_min));
    WinSrc s = src;
    int n_max;
    TDA_TRY(win_src_limits(ctx, s.mode, s.n_in, s.dim, s.subsample, &s, &n_max));
    if (n_win == 0) return TDA_OK;
    // the columns of hist: the `nodal` convention of the network curves
    const int n_hist = s.mode == 2 ? s.n_in : s.mode == 1 ? s.n_in : TDA_MAX_POINTS;
    if (hist && (long long)2 * n_grid * n_hist > 0x7fffffffll)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "2 * n_grid * n_hist must fit an int");
    const KeyLayout L = key_layout(n_max, s.dim);
    if (n_max <= 64)
        hipLaunchKernelGGL(recurrence_kernel<1>, dim3(n_win), dim3(RQ_NT), L.total, st, s, (float)thresh, L, grid, n_grid,
                           theiler, l_min, v_min, n_hist, counts, measures, hist, n_points, status);
    else
        hipLaunchKernelGGL(recurrence_kernel<2>, dim3(n_win), dim3(RQ_NT), L.total, st, s, (float)thresh, L, grid, n_grid,
                           theiler, l_min, v_min, n_hist, counts, measures, hist, n_points, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status rq_mean_check(tda_ctx* ctx, const void* counts, const void* measures, const void* hist, int n_win, int n_grid,
                         int n_hist, const int* seg_off, int n_seg, const void* mean_counts, const void* mean_measures,
                         const void* mean_hist)
{
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]");
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg && n_win &&
        ((counts == nullptr) != (mean_counts == nullptr) || (measures == nullptr) != (mean_measures == nullptr) ||
         (hist == nullptr) != (mean_hist == nullptr)))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "counts, measures and hist are each nullable together with their mean");
    if ((hist || mean_hist) && (n_hist < 1 || (long long)2 * n_grid * n_hist > 0x7fffffffll))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "n_hist must be >= 1 and 2 * n_grid * n_hist must fit an int");
    return TDA_OK;
}

tda_status launch_recurrence_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* hist, int n_win,
                                  int n_grid, int n_hist, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                                  double* mean_counts, double* mean_measures, double* mean_hist, hipStream_t st)
{
    TDA_TRY(rq_mean_check(ctx, counts, measures, hist, n_win, n_grid, n_hist, seg_off, n_seg, mean_counts, mean_measures,
                          mean_hist));
    if (n_seg == 0) return TDA_OK;
    const auto blocks = [&](int row_len) { return dim3((unsigned)(((long long)n_seg * row_len + 255) / 256)); };
    if (mean_counts) {
        const int rl = TDA_RQA_ROWS * n_grid;
        hipLaunchKernelGGL((group_mean_kernel<int, long long>), blocks(rl), dim3(256), 0, st, counts, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_counts);
        TDA_HIP(ctx, hipGetLastError());
    }
    if (mean_measures) {
        const int rl = TDA_RQA_MEASURES * n_grid;
        hipLaunchKernelGGL((group_mean_kernel<double, double>), blocks(rl), dim3(256), 0, st, measures, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_measures);
        TDA_HIP(ctx, hipGetLastError());
    }
    if (mean_hist) {
        const int rl = 2 * n_grid * n_hist;
        hipLaunchKernelGGL((group_mean_kernel<int, long long>), blocks(rl), dim3(256), 0, st, hist, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_hist);
        TDA_HIP(ctx, hipGetLastError());
    }
    return TDA_OK;
}
