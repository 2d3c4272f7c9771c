// fisher.hip -- the persistence Fisher distance between persistence diagrams (Le and Yamada, NeurIPS 2018): the Fisher
// information metric between two diagrams smoothed by Gaussians on a support made of both diagrams and their diagonal
// images.  The persistence Fisher kernel exp(-t * distance) is formed by the Python layer.
//
// The definition is the text in include/tdaeeg.h.  F_A / F_B: the rows of A / B with both values finite, in stored order;
// m = |F_A|, n = |F_B|, N = m + n.  The image of a row (b, d) is (h, h), h = 0.5 * (b + d).
//   P = F_A, images of F_B          Q = F_B, images of F_A          Theta = P, Q           (2N points)
//   g(x, u) = exp((dx * dx + dy * dy) * ninv),  r_P(x) = sum over u in P,  r_Q(x) = sum over u in Q,  x in Theta
//   Z_P = sum over x of r_P(x), Z_Q likewise;  a_x = sqrt(r_P(x) / Z_P), b_x = sqrt(r_Q(x) / Z_Q)
//   c2 = sum over x of (a_x - b_x)^2;  out = 2 * asin(min(0.5 * sqrt(c2), 1))
// No multiply-add: contraction is off for the file and said again below.  exp, sqrt and asin are the device library's.
//
// One workgroup of PF_THREADS = 256 threads per pair (a step's H0 pairs have 2N around 318 points, five wave-rounds of
// 64 points that four waves take in two rounds and one wave in five; a wavefront per pair measured slower):
//   * every wave walks both diagrams in chunks of 64 rows and counts the finite rows with a ballot (m, n: the same value
//     in every wave, no barrier); a pair with a bad index or N > TDA_PF_MAX_POINTS leaves here, before anything is staged;
//   * the same walk again, now writing: the ballot's prefix count gives a finite row its place, so the stored order is
//     kept; wave v writes the chunks v, v + waves, ..  Theta lies in LDS as (x1, x2) pairs, Q directly behind P;
//   * thread t owns the points t, t + PF_THREADS, ..: pf_row_sum walks a list of N staged points (every lane reads the SAME
//     LDS address: a broadcast, no bank conflict) and adds in list order; it is called for P and for Q.  The two sums
//     go back to LDS as (r_P, r_Q);
//   * Z_P, Z_Q and c2 are workgroup sums by pf_block_sum: a thread adds its own points in ascending order, lane l of every
//     wave adds the partials l, l + 64, .., then a butterfly over the lanes (partner lane ^ 32, 16, .., 1).
// r_P and r_Q, and Z_P and Z_Q, come from the same code in the same order, so two diagrams with the same finite rows in
// the same order give c2 == 0.0 and out == 0.0 exactly.  The order of every addition depends on the pair's m and n alone:
// no atomics, the same bytes for a pair alone and inside a batch.  The dynamic LDS is sized from the capacities and is
// only room: no value depends on it.
// Loop bounds, all known before the loop starts: chunks ceil(rows / 64), points of a thread, N points of a list.  No
// barrier sits under a divergent branch.  Nothing is allocated, nothing synchronises with the host, no scratch.
#include "common.h"
#include <cmath>

#pragma clang fp contract(off)

#ifndef PF_THREADS
#define PF_THREADS 256              // make VARIANT=pf64 EXTRA=-DPF_THREADS=64: one wavefront per pair, for the A/B of 3.16
#endif
#define PF_WAVES (PF_THREADS / 64)

__device__ __forceinline__ int pf_rows(const int* cnt, int w, int cap)
{
    int m = uni(cnt[w]);
    m = m < cap ? m : cap;
    return m < 0 ? 0 : m;
}

// finite rows among the first `rows` rows (every wave computes the same number)
__device__ __forceinline__ int pf_count(const double2* rows_p, int rows)
{
    const int lane = (int)threadIdx.x & 63;
    int c = 0;
    for (int r0 = 0; r0 < rows; r0 += 64) {
        bool ok = false;
        if (r0 + lane < rows) { const double2 x = rows_p[r0 + lane]; ok = isfinite(x.x) && isfinite(x.y); }
        c += __popcll(__ballot(ok));
    }
    return c;
}

// the finite rows, in stored order, to own[0..) and their diagonal images to img[0..); wave v writes chunks v, v + waves, ..
__device__ __forceinline__ void pf_stage(const double2* rows_p, int rows, double2* own, double2* img)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int base = 0, chunk = 0;
    for (int r0 = 0; r0 < rows; r0 += 64, ++chunk) {
        bool ok = false;
        double2 x = {0.0, 0.0};
        if (r0 + lane < rows) { x = rows_p[r0 + lane]; ok = isfinite(x.x) && isfinite(x.y); }
        const unsigned long long mask = __ballot(ok);
        if (ok && (chunk % PF_WAVES) == wave) {
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            const double h = 0.5 * (x.x + x.y);
            own[pos] = x;
            img[pos] = make_double2(h, h);
        }
        base += __popcll(mask);
    }
}

// sum over the N points of `list` of g(x, u), in list order
__device__ __forceinline__ double pf_row_sum(const double2 x, const double2* list, int N, double ninv)
{
    double r = 0.0;
#pragma unroll 2
    for (int u = 0; u < N; ++u) {
        const double2 p = list[u];
        const double dx = x.x - p.x, dy = x.y - p.y;
        r = r + exp((dx * dx + dy * dy) * ninv);
    }
    return r;
}

// sum of v over the workgroup, on every thread: red holds PF_THREADS doubles
__device__ __forceinline__ double pf_block_sum(double v, double* red)
{
    if (PF_WAVES > 1) {
        const int lane = (int)threadIdx.x & 63;
        __syncthreads();                                             // red is free: everyone is past its last read
        red[threadIdx.x] = v;
        __syncthreads();
        v = 0.0;
#pragma unroll
        for (int k = 0; k < PF_THREADS; k += 64) v = v + red[k + lane];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(PF_THREADS)
persistence_fisher_pairs(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int n_a, int cap_a,
                         const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int n_b, int cap_b,
                         const int* __restrict__ idx_a, const int* __restrict__ idx_b, int n_pairs, double ninv,
                         int max_pts, double* __restrict__ out, int* __restrict__ status)
{
    extern __shared__ double2 pf_lds[];                              // theta[max_pts], then (r_P, r_Q)[max_pts]
    __shared__ double red[PF_THREADS];
    const int pr = blockIdx.x, tid = (int)threadIdx.x;
    if (pr >= n_pairs) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int ia = uni(idx_a ? idx_a[pr] : pr), ib = uni(idx_b ? idx_b[pr] : pr);
    if (ia < 0 || ia >= n_a || ib < 0 || ib >= n_b) {                 // (the same for every thread)
        if (tid == 0) { out[pr] = qnan; status[pr] = TDA_WIN_NO_PAIR; }
        return;
    }
    const double2* ra = reinterpret_cast<const double2*>(dgm_a) + (size_t)ia * cap_a;
    const double2* rb = reinterpret_cast<const double2*>(dgm_b) + (size_t)ib * cap_b;
    const int rows_a = pf_rows(cnt_a, ia, cap_a), rows_b = pf_rows(cnt_b, ib, cap_b);
    const int m = uni(pf_count(ra, rows_a)), n = uni(pf_count(rb, rows_b));
    const int N = m + n;                                             // (m <= cap_a, n <= cap_b: 2N <= max_pts unless refused)
    if (N > TDA_PF_MAX_POINTS || 2 * N > max_pts) {                   // (the same for every thread)
        if (tid == 0) { out[pr] = qnan; status[pr] = TDA_WIN_TOO_LARGE; }
        return;
    }
    if (N == 0) {
        if (tid == 0) { out[pr] = 0.0; status[pr] = 0; }
        return;
    }
    double2* theta = pf_lds;
    double2* rr = pf_lds + max_pts;
    pf_stage(ra, rows_a, theta, theta + N + n);                      // P = F_A, images of F_B; Q = F_B, images of F_A
    pf_stage(rb, rows_b, theta + N, theta + m);
    __syncthreads();
    const int M = 2 * N;
    double zp = 0.0, zq = 0.0;
    for (int k = tid; k < M; k += PF_THREADS) {
        const double2 x = theta[k];
        const double rp = pf_row_sum(x, theta, N, ninv);
        const double rq = pf_row_sum(x, theta + N, N, ninv);
        rr[k] = make_double2(rp, rq);                                // (read back by this thread alone)
        zp = zp + rp;
        zq = zq + rq;
    }
    const double Zp = pf_block_sum(zp, red);
    const double Zq = pf_block_sum(zq, red);
    double c = 0.0;
    for (int k = tid; k < M; k += PF_THREADS) {
        const double2 r = rr[k];
        const double a = sqrt(r.x / Zp), b = sqrt(r.y / Zq);
        const double d = a - b;
        c = c + d * d;
    }
    const double c2 = pf_block_sum(c, red);
    if (tid == 0) {
        double h = 0.5 * sqrt(c2);
        h = h < 1.0 ? h : 1.0;
        out[pr] = 2.0 * asin(h);
        status[pr] = 0;
    }
}

// ---------------------------------------------------------------------------------
tda_status launch_persistence_fisher(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                     const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                     const int* idx_b, int n_pairs, double ninv, double* out, int* status, hipStream_t st)
{
    if (!std::isfinite(ninv) || !(ninv < 0.0)) TDA_FAIL(ctx, TDA_ERR_INVALID, "ninv must be finite and < 0");
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_pairs == 0) return TDA_OK;
    // room for Theta of the largest pair the capacities allow, TDA_PF_MAX_POINTS at the most: 32 bytes a point
    long long pts = 2ll * ((long long)cap_a + (long long)cap_b);
    if (pts > 2 * TDA_PF_MAX_POINTS) pts = 2 * TDA_PF_MAX_POINTS;
    const int max_pts = (int)pts;
    hipLaunchKernelGGL(persistence_fisher_pairs, dim3(n_pairs), dim3(PF_THREADS), (size_t)max_pts * 2 * sizeof(double2), st,
                       dgm_a, cnt_a, n_a, cap_a, dgm_b, cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, ninv, max_pts, out, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
