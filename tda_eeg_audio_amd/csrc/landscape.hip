// landscape.hip -- persistence landscapes and Betti curves of diagrams, averaged per group.
//
// The definition (include/tdaeeg.h has it in full): for a diagram with rows (b_i, d_i), i < min(cnt, cap), and a grid
// point t,
//   tent_i(t)   = min(t - b_i, d_i - t), 0.0 where that is not > 0          (rows with both values finite only)
//   lambda_k(t) = the k-th largest tent, k = 1..K                           (0.0 when there are fewer than k)
//   beta(t)     = the number of rows with b_i <= t < d_i                    (every row, d = +inf included)
// and per group the elementwise sum of V = [lambda_1 .. lambda_K, beta] over the kept diagrams IN BUFFER ORDER, divided
// by their number.  Every operation is one correctly rounded float64 operation or a selection, so the output is the bits
// of tests/landscape_ref.py.  No multiply-add: the file is compiled with -ffp-contract=off and has no product anyway.
//
// Mapping: one wavefront per (group, block of 64 grid points); lane l owns grid point 64 * blockIdx.y + l and keeps its
// K + 1 running sums and the K largest tents of the current diagram in registers.  The wavefront walks the diagrams of its
// group in order.  A diagram is staged 64 rows at a time in LDS (one coalesced 16-byte load per lane), then every lane
// reads the same row (a broadcast read, no bank conflict) and inserts its tent into the sorted register file by K
// (max, min) pairs.  Only the group means are written, coalesced along the grid.
//
// Latency: the first 64 rows of the NEXT diagram, its count and its status word are requested before the current diagram
// is processed (the rows do not need the count: the buffer has cap rows for every diagram), and inside a diagram of more
// than 64 rows the next 64 are requested before the current 64 are processed.
//
// Loop bounds, all known before the loop starts: diagrams seg_off[g+1] - seg_off[g] (clamped to [0, n_dgm]); chunks
// ceil(min(cnt, cap) / 64); rows per chunk <= 64; insertion K (unrolled).  Nothing is allocated, nothing synchronises,
// no scratch, 1 KiB of LDS for the staged rows.
#include "common.h"

#define LS_ROWS 64          // rows staged per chunk: one per lane

struct ls_row { double b, d; };

template <int K>
__global__ void __launch_bounds__(64)
landscape_mean_kernel(const double* __restrict__ dgm, const int* __restrict__ cnt, int cap, int n_dgm,
                      const int* __restrict__ seg_off, int n_seg, const int* __restrict__ status, int skip_mask,
                      const double* __restrict__ grid, int n_grid, double* __restrict__ out)
{
    __shared__ ls_row rows[LS_ROWS];
    const int g = blockIdx.x, lane = lane_id();
    const int j = blockIdx.y * 64 + lane;
    const bool live = j < n_grid;
    const double t = live ? grid[j] : 0.0;
    int w0 = g, w1 = g + 1;                                          // seg_off == NULL: every diagram its own group
    if (seg_off) { w0 = uni(seg_off[g]); w1 = uni(seg_off[g + 1]); }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_dgm ? n_dgm : w1;
    const ls_row* __restrict__ src = reinterpret_cast<const ls_row*>(dgm);

    double sum[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) sum[k] = 0.0;
    int n_kept = 0;

    // the diagram in hand: its first LS_ROWS rows (one per lane), row count and status word
    ls_row first = {0.0, 0.0};
    int k_rows = 0, st = 0;
    if (w0 < w1) {
        if (lane < cap) first = src[(size_t)w0 * cap + lane];
        k_rows = uni(cnt[w0]);
        st = status ? uni(status[w0]) : 0;
    }
    for (int w = w0; w < w1; ++w) {
        ls_row first_n = {0.0, 0.0};
        int k_n = 0, st_n = 0;
        if (w + 1 < w1) {                                            // requested now, used after this diagram
            if (lane < cap) first_n = src[(size_t)(w + 1) * cap + lane];
            k_n = cnt[w + 1];
            st_n = status ? status[w + 1] : 0;
        }
        if (!(st & skip_mask)) {
            int m = k_rows < cap ? k_rows : cap;                     // a truncated diagram (cnt > cap) has cap rows
            m = m < 0 ? 0 : m;
            double top[K];
#pragma unroll
            for (int k = 0; k < K; ++k) top[k] = 0.0;
            int beta = 0;
            ls_row cur = first;
            for (int c0 = 0; c0 < m; c0 += LS_ROWS) {
                __syncthreads();                                     // the previous chunk has been read by every lane
                rows[lane] = cur;
                __syncthreads();
                if (c0 + LS_ROWS + lane < m) cur = src[(size_t)w * cap + c0 + LS_ROWS + lane];
                const int mc = m - c0 < LS_ROWS ? m - c0 : LS_ROWS;
#pragma unroll 4
                for (int i = 0; i < mc; ++i) {
                    const ls_row r = rows[i];                        // the same address in every lane
                    beta += (r.b <= t && t < r.d) ? 1 : 0;
                    if (isfinite(r.b) && isfinite(r.d)) {            // wave-uniform
                        double v = fmin(t - r.b, r.d - t);
                        v = v > 0.0 ? v : 0.0;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const double hi = fmax(top[k], v);
                            v = fmin(top[k], v);
                            top[k] = hi;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) sum[k] = sum[k] + top[k];
            sum[K] = sum[K] + (double)beta;
            ++n_kept;
        }
        first = first_n; k_rows = uni(k_n); st = uni(st_n);
    }
    if (live) {
        const double n = (double)n_kept;
        double* o = out + (size_t)g * (K + 1) * n_grid + j;
#pragma unroll
        for (int k = 0; k <= K; ++k) o[(size_t)k * n_grid] = n_kept ? sum[k] / n : __longlong_as_double(0x7ff8000000000000ll);
    }
}

tda_status launch_landscape_mean(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                                 int n_seg, const int* status, int skip_mask, const double* grid, int n_grid, int n_levels,
                                 double* out, hipStream_t st)
{
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_levels < 1 || n_levels > TDA_MAX_LANDSCAPES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_levels must be 1..TDA_MAX_LANDSCAPES");
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be 1..TDA_MAX_GRID");
    if (n_seg == 0) return TDA_OK;
    const dim3 blocks(n_seg, (n_grid + 63) / 64);
#define LS_LAUNCH(KV)                                                                                                  \
    case KV:                                                                                                           \
        hipLaunchKernelGGL(landscape_mean_kernel<KV>, blocks, dim3(64), 0, st, dgm, cnt, cap, n_dgm, seg_off, n_seg,   \
                           status, skip_mask, grid, n_grid, out);                                                      \
        break
    switch (n_levels) {
        LS_LAUNCH(1); LS_LAUNCH(2); LS_LAUNCH(3); LS_LAUNCH(4); LS_LAUNCH(5); LS_LAUNCH(6); LS_LAUNCH(7); LS_LAUNCH(8);
    }
#undef LS_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
