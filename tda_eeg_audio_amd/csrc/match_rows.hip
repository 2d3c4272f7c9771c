// match_rows.hip -- the rows of the match-mismatch matrix (tda_match_rows_dev), gfx950 / wave64.  A file of its own:
// features.hip's kernels stay instruction for instruction what they were (tools/isa_diff.py --files features).
#include "common.h"

// ---------------------------------------------------------------------------------
// The rows of the match-mismatch matrix (mvm:86-95, 134-145 against EVERY candidate audio): per A group g, from row g
// of tda_wasserstein_matrix_dev's out / pairs / flags,
//   [ w_own, n_own_pairs, n_valid, n_less, n_equal, null_mean ]
// w_own = out[g, own_col[g]]; the others = the columns c != own_col[g] with a finite entry: their number, how many lie
// below / at w_own (midrank of the true audio among n_valid + 1 candidates: 1 + n_less + n_equal / 2), their mean.
// One wave per group, lane l takes the columns l, l + 64, ...; the counts are integer sums, the mean a sum of per-lane
// partial sums (all terms >= 0: within (n_valid + 1) 2^-52 relative of any other order).
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
match_rows_kernel(const double* __restrict__ out, const int* __restrict__ pairs, const int* __restrict__ flags, int n_seg,
                  int n_col, const int* __restrict__ own_col, const int* __restrict__ status_a,
                  const int* __restrict__ seg_off_a, double* __restrict__ rows, int* __restrict__ seg_flags)
{
    const int g = blockIdx.x;
    if (g >= n_seg) return;
    const int lane = lane_id();
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double* x = out + (size_t)g * n_col;
    int own = uni(own_col[g]);
    if (own < 0 || own >= n_col) own = -1;
    double w_own = own >= 0 ? x[own] : qnan;
    const int n_own = own >= 0 ? pairs[(size_t)g * n_col + own] : 0;
    const bool has_own = w_own == w_own;
    if (!has_own) w_own = qnan;
    int n_valid = 0, n_less = 0, n_equal = 0, fl = 0;
    double part = 0.0;
    for (int c = lane; c < n_col; c += 64) {
        const double v = x[c];
        fl |= flags[(size_t)g * n_col + c];
        if (c == own || !isfinite(v)) continue;
        ++n_valid;
        part += v;
        if (has_own) { n_less += v < w_own ? 1 : 0; n_equal += v == w_own ? 1 : 0; }
    }
    if (seg_flags && status_a) {
        const int s0 = uni(seg_off_a[g]), s1 = uni(seg_off_a[g + 1]);
        for (int i = s0 + lane; i < s1; i += 64) fl |= status_a[i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_valid += __shfl_xor(n_valid, off, 64);
        n_less += __shfl_xor(n_less, off, 64);
        n_equal += __shfl_xor(n_equal, off, 64);
        fl |= __shfl_xor(fl, off, 64);
        part += __shfl_xor(part, off, 64);
    }
    if (lane == 0) {
        double* row = rows + (size_t)g * 6;
        row[0] = w_own; row[1] = (double)n_own; row[2] = (double)n_valid; row[3] = (double)n_less; row[4] = (double)n_equal;
        row[5] = n_valid > 0 ? part / (double)n_valid : qnan;
        if (seg_flags) seg_flags[g] = fl & ~(TDA_WIN_NO_PAIR | TDA_WIN_DEGENERATE);
    }
}

tda_status launch_match_rows(tda_ctx* ctx, const double* out, const int* pairs, const int* flags, int n_seg, int n_col,
                             const int* own_col, const int* status_a, const int* seg_off_a, double* rows, int* seg_flags,
                             hipStream_t st)
{
    if (n_seg == 0) return TDA_OK;
    hipLaunchKernelGGL(match_rows_kernel, dim3(n_seg), dim3(64), 0, st, out, pairs, flags, n_seg, n_col, own_col, status_a,
                       seg_off_a, rows, seg_flags);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
