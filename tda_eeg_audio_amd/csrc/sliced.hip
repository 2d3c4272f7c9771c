// sliced.hip -- batched sliced Wasserstein distance between persistence diagrams (Carriere, Cuturi, Oudot 2017).
//
// The definition is the text in include/tdaeeg.h.  Diagrams A (m rows after cleaning) and B (n rows) are cleaned as
// safe_wasserstein cleans them (rows with a non-finite entry dropped, an empty diagram -> {(0,0)}); a row (b, d) has the
// diagonal image (h, h), h = 0.5 * (b + d).  A' = rows of A, then images of B; B' = rows of B, then images of A; both
// have N = m + n points.  Per direction (c, s) of the caller's table every point is projected as p = (c * x) + (s * y)
// (two rounded products, one rounded sum, no multiply-add: the file is compiled with contraction off and says so again
// below), both lists are sorted, L_k = sum_i fabs(u_i - v_i), and the result is (sum_k L_k) / M.
//
// One workgroup of SW_WAVES waves per pair:
//   1. wave 0 compacts the finite rows of A into LDS (ballot + popcount, order kept) with their h values, wave 1 those
//      of B; the counts m, n go through LDS.  Nothing behind cnt or beyond cap is read; cnt is clamped to [0, cap].
//   2. the waves take the directions in turn, k = wave, wave + SW_WAVES, ...  A wave projects both lists into registers,
//      V = 1, 2, 4 or 8 values per lane and list (element e = 64 r + lane sits in register r of that lane; the elements
//      e >= N are +inf), and sorts each list with a bitonic network on 64 V elements: for k = 2, 4, .., 64 V and
//      j = k/2, .., 1 element e is compared with e ^ j, ascending where (e & k) == 0.  The exchanges with j >= 64 are
//      between two registers of the same lane; j = 1, 2 go through DPP quad permutes, j = 4, 8, 16 through ds_swizzle,
//      j = 32 through ds_bpermute (none of them touches LDS memory).  An exchange swaps or does not swap: the values
//      are moved, never recomputed, so the sorted list is the multiset of the projections bit for bit.
//   3. t_i = fabs(u_i - v_i) for the ranks i < N only (the ranks behind are inf - inf = NaN and never enter a sum: they
//      are masked by the rank, not by their value); per lane the registers r = 0.. in turn, then a butterfly over the
//      lanes (partner lane ^ 1, 2, .., 32 -- every lane ends with the same bits).  L_k goes to LDS.
//   4. wave 0 adds the L_k (lane l: k = l, then l + 64; the same butterfly) and divides by M.
// The order of every addition depends on the rank and the direction index alone: no atomics, the same bytes for a pair
// alone and inside a batch, and for (A, B) and (B, A), which only swaps u and v under the fabs.
//
// V is picked per pair from N (N <= 64 -> 1, <= 128 -> 2, <= 256 -> 4, else 8) by a workgroup-uniform branch; the
// launch compiles in only the sizes its buffers can hold (MAXV from cap_a + cap_b), so the H1 buffers of a step, whose
// pairs have N around 60 or less, sort one value per lane whatever their capacity.
// Loop bounds, all known before the loop starts: cleaning ceil(cap / 64) rounds per diagram; directions
// ceil(M / SW_WAVES) <= 32 per wave; the network is straight-line code; the last sum ceil(M / 64) <= 2 rounds.
#include "sliced_dev.h"      // the network, the butterfly sum and the cleaning: shared with sliced_matrix.hip

#pragma clang fp contract(off)

// projections of one augmented list: the np own points, then the images of the other diagram's rows; +inf behind N
template <int V>
__device__ __forceinline__ void sw_project(const double* pts, int np, const double* h_other, int N, double c, double s,
                                           int lane, double (&x)[V])
{
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int e = 64 * r + lane;
        double px = 0.0, py = 0.0;
        if (e < np) { px = pts[2 * e]; py = pts[2 * e + 1]; }
        else if (e < N) { px = h_other[e - np]; py = px; }
        const double p = (c * px) + (s * py);
        x[r] = e < N ? p : INF;
    }
}

// L_k of one direction, by one wave: the same bits on every lane
template <int V>
__device__ __forceinline__ double sw_direction(const double* pa, const double* pb, const double* ha, const double* hb,
                                               int m, int n, double c, double s, int lane)
{
    const int N = m + n;
    double u[V], v[V];
    sw_project<V>(pa, m, hb, N, c, s, lane, u);
    sw_project<V>(pb, n, ha, N, c, s, lane, v);
    sw_sort<V, 2>(u, lane);
    sw_sort<V, 2>(v, lane);
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < V; ++r)
        if (64 * r + lane < N) acc += fabs(u[r] - v[r]);
    return sw_wave_sum(acc);
}

// LDS: rows of A (2 max_a) | rows of B (2 max_b) | h of A (max_a) | h of B (max_b) | L_k (TDA_MAX_DIRECTIONS) | m, n
template <int MAXV>
__global__ void __launch_bounds__(64 * SW_WAVES)
sliced_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
              const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
              const int* __restrict__ idx_a, const int* __restrict__ idx_b, int n_pairs, int max_a, int max_b,
              const double* __restrict__ dirs, int n_dirs, double* __restrict__ out, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    double* pa = reinterpret_cast<double*>(smem);
    double* pb = pa + 2 * max_a;
    double* ha = pb + 2 * max_b;
    double* hb = ha + max_a;
    double* Ls = hb + max_b;
    int* mn = reinterpret_cast<int*>(Ls + TDA_MAX_DIRECTIONS);

    const int ia = idx_a ? idx_a[pr] : pr, ib = idx_b ? idx_b[pr] : pr;
    if (wave == 0) {
        int ka = uni(cnt_a[ia]); ka = ka < cap_a ? ka : cap_a; ka = ka < 0 ? 0 : ka;
        const int m = sw_load(dgm_a + (size_t)ia * cap_a * 2, ka, max_a, pa, ha);
        if (lane == 0) mn[0] = m;
    } else if (wave == 1) {
        int kb = uni(cnt_b[ib]); kb = kb < cap_b ? kb : cap_b; kb = kb < 0 ? 0 : kb;
        const int n = sw_load(dgm_b + (size_t)ib * cap_b * 2, kb, max_b, pb, hb);
        if (lane == 0) mn[1] = n;
    }
    __syncthreads();
    const int m = uni(mn[0]), n = uni(mn[1]), N = m + n;
    if (N > TDA_SW_MAX_POINTS || N > 64 * MAXV || m > max_a || n > max_b) {       // (the same for every thread of the workgroup)
        if (threadIdx.x == 0) { out[pr] = __longlong_as_double(0x7ff8000000000000ll); status[pr] = TDA_WIN_TOO_LARGE; }
        return;
    }
    for (int k = wave; k < n_dirs; k += SW_WAVES) {
        const double c = dirs[2 * k], s = dirs[2 * k + 1];
        double L;
        if (MAXV == 1 || N <= 64) L = sw_direction<1>(pa, pb, ha, hb, m, n, c, s, lane);
        else if (MAXV == 2 || N <= 128) L = sw_direction<(MAXV >= 2 ? 2 : 1)>(pa, pb, ha, hb, m, n, c, s, lane);
        else if (MAXV == 4 || N <= 256) L = sw_direction<(MAXV >= 4 ? 4 : 1)>(pa, pb, ha, hb, m, n, c, s, lane);
        else L = sw_direction<(MAXV >= 8 ? 8 : 1)>(pa, pb, ha, hb, m, n, c, s, lane);
        if (lane == 0) Ls[k] = L;
    }
    __syncthreads();
    if (wave == 0) {
        double acc = 0.0;
        for (int k = lane; k < n_dirs; k += 64) acc += Ls[k];
        acc = sw_wave_sum(acc);
        if (lane == 0) { out[pr] = acc / (double)n_dirs; status[pr] = 0; }
    }
}

// ---------------------------------------------------------------------------------
// One launch.  The LDS is sized by the capacities of the two buffers (at most TDA_SW_MAX_POINTS rows each: a buffer may
// be larger, a pair with N above that is TDA_WIN_TOO_LARGE), the largest network compiled in by their sum.
tda_status launch_sliced(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                         const int* cnt_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs, const double* dirs,
                         int n_dirs, double* out, int* status, hipStream_t st)
{
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "1 <= n_dirs <= TDA_MAX_DIRECTIONS");
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_pairs == 0) return TDA_OK;
    const int max_a = cap_a < TDA_SW_MAX_POINTS ? cap_a : TDA_SW_MAX_POINTS;
    const int max_b = cap_b < TDA_SW_MAX_POINTS ? cap_b : TDA_SW_MAX_POINTS;
    const int most = max_a + max_b;                                  // N <= cap_a + cap_b
    const size_t lds = (size_t)(3 * max_a + 3 * max_b + TDA_MAX_DIRECTIONS + 1) * 8;     // <= 25.6 KB
#define SW_LAUNCH(MV)                                                                                                \
    hipLaunchKernelGGL(sliced_kernel<MV>, dim3(n_pairs), dim3(64 * SW_WAVES), lds, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, \
                       cap_b, idx_a, idx_b, n_pairs, max_a, max_b, dirs, n_dirs, out, status)
    if (most <= 64) SW_LAUNCH(1);
    else if (most <= 128) SW_LAUNCH(2);
    else if (most <= 256) SW_LAUNCH(4);
    else SW_LAUNCH(8);
#undef SW_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
