// image.hip -- persistence images of diagrams, averaged per group.
//
// The definition (include/tdaeeg.h has it in full): a diagram has rows (b_i, d_i), i < min(cnt, cap); F is the set of rows
// with both values finite; p_i = d_i - b_i; w_i = 1, p_i or p_i * p_i (power 0, 1, 2); s = sigma * sqrt(2);
//   Phi(e, c) = 0.5 * erfc(-((e - c) / s))
//   fx_i[c]   = Phi(xe[c + 1], b_i) - Phi(xe[c], b_i)           fy_i[r] = Phi(ye[r + 1], p_i) - Phi(ye[r], p_i)
//   I[r, c]   = sum over i in F of (w_i * fy_i[r]) * fx_i[c]
// and per group (sum of the images of the kept diagrams) / n_kept, NaN without a kept diagram.  erfc is the device
// library's, so the result agrees with a CPU evaluation to rounding, not bit for bit (the tolerance: DESIGN.md 3.10).
//
// Mapping: one workgroup of 256 threads per group.  The image is a sum of rank-1 terms, one per row, so the group's image
// is the sum over ALL rows of its kept diagrams: thread t owns the pixels t, t + 256, ... (PPT of them, a template
// parameter, at most 4 for 32 x 32) and keeps their running sums in registers from the first diagram to the last; no
// per-diagram image exists anywhere.  The workgroup walks the diagrams of its group in buffer order, a diagram in chunks of
// IM_ROWS rows.  Per chunk:
//   1. the rows go to LDS (threads 0..31, one 16-byte load each, requested one chunk ahead);
//   2. every (row, edge) pair of the chunk gets its Phi ONCE, the pairs dealt round-robin to the 256 threads:
//      n_x + n_y + 2 <= 66 erfc per row, never one per pixel -> cdf[row][edge] in LDS;
//   3. the differences: fac[row][c] = fx[c], fac[row][n_x + r] = w * fy[r] (0.0 for a row outside F) -> LDS;
//   4. every thread adds (w * fy[r]) * fx[c] of every row of the chunk to each of its pixels: one multiply and one add
//      per (row, pixel), the two factors read from LDS (consecutive threads read consecutive fx and, mostly, one fy:
//      conflict-free and a broadcast).
// The additions of a pixel run in buffer order of (diagram, row) whatever the launch is, so a group gives the same bytes
// alone, inside a batch, or through seg_off = NULL.  No atomics.  The means are written once, coalesced along c.
//
// Latency: the first chunk of the NEXT diagram, its count and its status word are requested before the current diagram is
// processed (the rows do not need the count: every diagram owns cap rows of the buffer).
//
// Loop bounds, all known before the loop starts: diagrams seg_off[g + 1] - seg_off[g] (clamped to [0, n_dgm]); chunks
// ceil(min(cnt, cap) / IM_ROWS); (row, edge) pairs and (row, factor) pairs of a chunk; rows of a chunk; PPT (unrolled).
// Nothing is allocated, nothing synchronises, no scratch.
#include "common.h"
#include <cmath>

#define IM_ROWS    32                                   // rows staged per chunk
#define IM_THREADS 256
#define IM_EDGES   (2 * TDA_MAX_IMAGE_SIDE + 2)         // edge values of a row: n_x + 1 and n_y + 1
#define IM_FACS    (2 * TDA_MAX_IMAGE_SIDE)             // factors of a row: n_x of fx and n_y of w * fy

template <int PPT>
__global__ void __launch_bounds__(IM_THREADS)
image_mean_kernel(const double* __restrict__ dgm, const int* __restrict__ cnt, int cap, int n_dgm,
                  const int* __restrict__ seg_off, int n_seg, const int* __restrict__ status, int skip_mask,
                  const double* __restrict__ xe, int n_x, const double* __restrict__ ye, int n_y, double sigma, int power,
                  double* __restrict__ out)
{
    __shared__ double2 rows[IM_ROWS];
    __shared__ double edges[IM_EDGES];
    __shared__ double cdf[IM_ROWS * IM_EDGES];
    __shared__ double fac[IM_ROWS * IM_FACS];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n_e = n_x + n_y + 2, n_f = n_x + n_y, n_pix = n_x * n_y;
    const double s = sigma * 1.4142135623730951;
    if (tid < n_e) edges[tid] = tid <= n_x ? xe[tid] : ye[tid - n_x - 1];
    int w0 = g, w1 = g + 1;                                          // seg_off == NULL: every diagram its own group
    if (seg_off) { w0 = uni(seg_off[g]); w1 = uni(seg_off[g + 1]); }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_dgm ? n_dgm : w1;
    const double2* __restrict__ src = reinterpret_cast<const double2*>(dgm);

    // the pixels of this thread; one past the image computes on pixel 0 and stores nothing
    int ic[PPT], ir[PPT];
    double sum[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        int p = tid + k * IM_THREADS;
        p = p < n_pix ? p : 0;
        ir[k] = n_x + p / n_x; ic[k] = p % n_x;
        sum[k] = 0.0;
    }
    int n_kept = 0;

    // the diagram in hand: its first IM_ROWS rows (threads 0..31), row count and status word
    const bool loader = tid < IM_ROWS;
    double2 first = make_double2(0.0, 0.0);
    int k_rows = 0, st = 0;
    if (w0 < w1) {
        if (loader && tid < cap) first = src[(size_t)w0 * cap + tid];
        k_rows = uni(cnt[w0]);
        st = status ? uni(status[w0]) : 0;
    }
    for (int w = w0; w < w1; ++w) {
        double2 first_n = make_double2(0.0, 0.0);
        int k_n = 0, st_n = 0;
        if (w + 1 < w1) {                                            // requested now, used after this diagram
            if (loader && tid < cap) first_n = src[(size_t)(w + 1) * cap + tid];
            k_n = cnt[w + 1];
            st_n = status ? status[w + 1] : 0;
        }
        if (!(st & skip_mask)) {
            int m = k_rows < cap ? k_rows : cap;                     // a truncated diagram (cnt > cap) has cap rows
            m = m < 0 ? 0 : m;
            double2 cur = first;
            for (int c0 = 0; c0 < m; c0 += IM_ROWS) {
                // rows, cdf and fac are free: every thread has passed the barrier after step 3 of the previous chunk
                // (rows, cdf) and nobody writes fac before the barrier after step 1, which is after everyone's step 4
                if (loader) rows[tid] = cur;
                __syncthreads();
                if (loader && c0 + IM_ROWS + tid < m) cur = src[(size_t)w * cap + c0 + IM_ROWS + tid];
                const int mc = m - c0 < IM_ROWS ? m - c0 : IM_ROWS;
                // 2. Phi of every (row, edge) pair of the chunk
                const int n_cdf = mc * n_e;
                for (int idx = tid; idx < n_cdf; idx += IM_THREADS) {
                    const int i = idx / n_e, e = idx - i * n_e;
                    const double2 r = rows[i];
                    const double c = e <= n_x ? r.x : r.y - r.x;
                    cdf[i * IM_EDGES + e] = 0.5 * erfc(-((edges[e] - c) / s));
                }
                __syncthreads();
                // 3. the factors: fx[c], then w * fy[r]; 0.0 for a row with a value that is not finite
                const int n_fac = mc * n_f;
                for (int idx = tid; idx < n_fac; idx += IM_THREADS) {
                    const int i = idx / n_f, f = idx - i * n_f;
                    const double2 r = rows[i];
                    const int e = f < n_x ? f : f + 1;               // the y edges start at n_x + 1
                    double v = cdf[i * IM_EDGES + e + 1] - cdf[i * IM_EDGES + e];
                    if (f >= n_x) {
                        const double p = r.y - r.x;
                        const double wgt = power == 0 ? 1.0 : power == 1 ? p : p * p;
                        v = wgt * v;
                    }
                    fac[i * IM_FACS + f] = (isfinite(r.x) && isfinite(r.y)) ? v : 0.0;
                }
                __syncthreads();
                // 4. the rank-1 terms of the chunk's rows, in row order
                for (int i = 0; i < mc; ++i) {
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const double t = fac[i * IM_FACS + ir[k]] * fac[i * IM_FACS + ic[k]];
                        sum[k] = sum[k] + t;
                    }
                }
            }
            ++n_kept;
        }
        first = first_n; k_rows = uni(k_n); st = uni(st_n);
    }
    const double n = (double)n_kept;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * IM_THREADS;
        if (p < n_pix) out[(size_t)g * n_pix + p] = n_kept ? sum[k] / n : __longlong_as_double(0x7ff8000000000000ll);
    }
}

tda_status launch_image_mean(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                             int n_seg, const int* status, int skip_mask, const double* xe, int n_x, const double* ye,
                             int n_y, double sigma, int power, double* out, hipStream_t st)
{
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_x < 1 || n_x > TDA_MAX_IMAGE_SIDE || n_y < 1 || n_y > TDA_MAX_IMAGE_SIDE)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "n_x and n_y must be 1..TDA_MAX_IMAGE_SIDE");
    if (!(sigma > 0.0) || !std::isfinite(sigma)) TDA_FAIL(ctx, TDA_ERR_INVALID, "sigma must be finite and > 0");
    if (power < 0 || power > 2) TDA_FAIL(ctx, TDA_ERR_INVALID, "power must be 0, 1 or 2");
    if (n_seg == 0) return TDA_OK;
#define IM_LAUNCH(P)                                                                                                   \
    case P:                                                                                                            \
        hipLaunchKernelGGL(image_mean_kernel<P>, dim3(n_seg), dim3(IM_THREADS), 0, st, dgm, cnt, cap, n_dgm, seg_off,  \
                           n_seg, status, skip_mask, xe, n_x, ye, n_y, sigma, power, out);                             \
        break
    switch ((n_x * n_y + IM_THREADS - 1) / IM_THREADS) {
        IM_LAUNCH(1); IM_LAUNCH(2); IM_LAUNCH(3); IM_LAUNCH(4);
    }
#undef IM_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
