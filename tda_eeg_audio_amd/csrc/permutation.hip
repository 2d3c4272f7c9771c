// permutation.hip -- within- and between-group sums of distance / Gram matrices under many relabellings (include/tdaeeg.h,
// "Two-sample permutation sums"), float64, gfx950.
//
// One LANE per relabelling.  The labels are stored transposed, one 64-bit word per (group of 64 relabellings, item), so the
// word of item j IS the lane mask "label of j is 1" of the wave that owns the group, and ~(word_i ^ word_j) the mask "same
// label as row i".  D[i][j] and the words are the same for every lane: both arrive by scalar loads (wave-uniform addresses
// on __restrict__ const pointers), eight entries of a row at a time, and the mask becomes EXEC for the two additions of a
// step (the remainder of a row and the row's own label take it as the condition of a select, an inverse ballot), never
// through a per-lane shift.  A lane that is off keeps its partial: "added to one and not at all to the other".
//   perm_rows_kernel    a 256-thread workgroup = 4 waves = 4 label words x one block of TDA_PT_ROW_BLOCK rows x one matrix;
//                       the waves share nothing but the cache lines of D they read.  Per row a lane keeps `same` and `diff`,
//                       sequential over ascending j; per block p00 / p11 / p01, sequential over ascending i.  The block
//                       partials go to `work` with plain vector stores, lane-contiguous.
//   perm_finish_kernel  one lane per (matrix, sum, relabelling): the block partials in ascending block order; the last grid
//                       row counts n1.
// No atomics, no LDS, no barriers: the order of every sum is the header's, whatever the launch geometry.
#include "common.h"

#define PT_WAVES 4
#define PT_NT (64 * PT_WAVES)
#define PT_R TDA_PT_ROW_BLOCK
#define PT_UNROLL 8

// the lane's bit of a wave-uniform 64-bit mask, as a condition the compiler keeps in a scalar register pair
__device__ __forceinline__ bool pt_lane_bit(u64 mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }

__global__ __launch_bounds__(PT_NT) void perm_rows_kernel(const double* __restrict__ D, int n, int ld,
                                                           const u64* __restrict__ lab, int n_words, int nblk,
                                                           double* __restrict__ work)
{
    const int g = uni((int)blockIdx.x * PT_WAVES + (int)(threadIdx.x >> 6));
    if (g >= n_words) return;
    const int b = (int)blockIdx.y, m = (int)blockIdx.z;
    const double* __restrict__ Dm = D + (size_t)m * n * ld;
    const u64* __restrict__ L = lab + (size_t)g * n;
    const int i0 = b * PT_R, i1 = i0 + PT_R < n ? i0 + PT_R : n;
    double p00 = 0.0, p11 = 0.0, p01 = 0.0;
    for (int i = i0; i < i1; ++i) {
        const u64 wi = L[i];
        const double* __restrict__ row = Dm + (size_t)i * ld;
        double same = 0.0, diff = 0.0;
        int j = i + 1;
        for (; j + PT_UNROLL <= n; j += PT_UNROLL) {
            // eight steps with the lane mask as EXEC itself: `same` is added under word_i XNOR word_j, `diff` under its
            // complement, two scalar and two vector instructions a step (the loop below is the same step as the compiler
            // writes it, both additions and four v_cndmask_b32: the same bytes at 1.5 times the time).
            // Every lane is on again at the end: a workgroup is 256 live lanes and all control flow of this kernel is
            // wave-uniform, so EXEC is all ones on entry.
#define PT_STEP_(K) "s_xnor_b64 exec, %[wi], %[w" #K "]\n\tv_add_f64 %[s], %[s], %[d" #K "]\n\t" \
                    "s_not_b64 exec, exec\n\tv_add_f64 %[f], %[f], %[d" #K "]\n\t"
            asm volatile(PT_STEP_(0) PT_STEP_(1) PT_STEP_(2) PT_STEP_(3) PT_STEP_(4) PT_STEP_(5) PT_STEP_(6) PT_STEP_(7)
                         "s_mov_b64 exec, -1"
                         : [s] "+v"(same), [f] "+v"(diff)
                         : [wi] "s"(wi), [w0] "s"(L[j]), [w1] "s"(L[j + 1]), [w2] "s"(L[j + 2]), [w3] "s"(L[j + 3]),
                           [w4] "s"(L[j + 4]), [w5] "s"(L[j + 5]), [w6] "s"(L[j + 6]), [w7] "s"(L[j + 7]),
                           [d0] "s"(row[j]), [d1] "s"(row[j + 1]), [d2] "s"(row[j + 2]), [d3] "s"(row[j + 3]),
                           [d4] "s"(row[j + 4]), [d5] "s"(row[j + 5]), [d6] "s"(row[j + 6]), [d7] "s"(row[j + 7])
                         : "scc");
#undef PT_STEP_
        }
        for (; j < n; ++j) {
            const double d = row[j];
            if (pt_lane_bit(~(wi ^ L[j]))) same += d;
            else diff += d;
        }
        if (pt_lane_bit(wi)) p11 += same;
        else p00 += same;
        p01 += diff;
    }
    const size_t np = (size_t)n_words * 64;
    double* o = work + ((size_t)m * nblk + b) * 3 * np + (size_t)g * 64 + lane_id();
    o[0] = p00;
    o[np] = p11;
    o[2 * np] = p01;
}

// grid (ceil(64 n_words / 256), 3 n_mat + 1): row y < 3 n_mat is sum y % 3 of matrix y / 3, the last row is n1
__global__ __launch_bounds__(PT_NT) void perm_finish_kernel(const double* __restrict__ work, const u64* __restrict__ lab, int n,
                                                             int n_words, int nblk, int n_mat, int n_perm,
                                                             double* __restrict__ out, int* __restrict__ n1)
{
    const int p = (int)blockIdx.x * PT_NT + (int)threadIdx.x;
    const int y = (int)blockIdx.y;
    const size_t np = (size_t)n_words * 64;
    if (y < 3 * n_mat) {
        if (p >= n_perm) return;
        const int m = y / 3, k = y - 3 * m;
        const double* w = work + ((size_t)m * nblk * 3 + k) * np + p;
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += w[(size_t)b * 3 * np];
        out[((size_t)m * 3 + k) * n_perm + p] = s;
        return;
    }
    const int g = uni(p >> 6);
    if (g >= n_words || !n1) return;
    const u64* __restrict__ L = lab + (size_t)g * n;
    int c = 0;
    for (int j = 0; j < n; ++j) c += pt_lane_bit(L[j]) ? 1 : 0;
    if (p < n_perm) n1[p] = c;
}

tda_status launch_perm_sums(tda_ctx* ctx, const double* D, int n_mat, int n, int ld, const unsigned long long* lab, int n_perm,
                            double* work, long long work_doubles, double* out, int* n1, hipStream_t st)
{
    if (n < 2 || n > TDA_PT_MAX_ITEMS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [2, TDA_PT_MAX_ITEMS]");
    if (n_perm < 1 || n_perm > TDA_PT_MAX_PERM) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_perm must be in [1, TDA_PT_MAX_PERM]");
    if (n_mat < 0 || n_mat > TDA_PT_MAX_MATRICES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_mat must be in [0, TDA_PT_MAX_MATRICES]");
    if (ld < n) TDA_FAIL(ctx, TDA_ERR_INVALID, "ld must be >= n");
    if (work_doubles < TDA_PT_WORK_DOUBLES(n_mat, n, n_perm)) TDA_FAIL(ctx, TDA_ERR_INVALID, "work is smaller than TDA_PT_WORK_DOUBLES");
    const int n_words = TDA_PT_WORDS(n_perm), nblk = TDA_PT_BLOCKS(n);
    if (n_mat)
        hipLaunchKernelGGL(perm_rows_kernel, dim3((n_words + PT_WAVES - 1) / PT_WAVES, nblk, n_mat), dim3(PT_NT), 0, st, D, n, ld,
                           (const u64*)lab, n_words, nblk, work);
    hipLaunchKernelGGL(perm_finish_kernel, dim3((n_words * 64 + PT_NT - 1) / PT_NT, 3 * n_mat + 1), dim3(PT_NT), 0, st, work,
                       (const u64*)lab, n, n_words, nblk, n_mat, n_perm, out, n1);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
