// diagram_kernel.hip -- kernels (in the machine-learning sense) on persistence diagrams: the persistence scale-space kernel
// (Reininghaus, Huber, Bauer, Kwitt 2015) and the persistence weighted Gaussian kernel (Kusano, Fukumizu, Hiraoka 2016),
// between pairs of diagrams and between the mean embeddings of groups of diagrams.
//
// The definition is the text in include/tdaeeg.h.  A side is a run of diagrams [w0, w1) of one buffer; its rows are the
// rows i < min(cnt, cap) of its kept diagrams, in buffer order.  For a row (b, d): p = d - b and the weight w is 1.0, p
// or atan(wc * p), computed ONCE when the row is staged.  For a row i of side A and a row j of side B
//   dx = b_i - b_j, dy = d_i - d_j, a1 = (dx * dx + dy * dy) * ninv, E1 = exp(a1)
//   ex = b_i - d_j, ey = d_i - b_j, a2 = (ex * ex + ey * ey) * ninv, E2 = exp(a2)            (mirror only)
//   t_ij = (w_i * w_j) * (E1 - E2)      or (w_i * w_j) * E1
// and S(A, B) is the sum of the t_ij over the rows with both values finite.  No multiply-add: contraction is off for the
// file and said again below.  exp and atan are the device library's.
//
// One tile routine, dk_tile_sum<NT>, for a workgroup of NT threads:
//   * dk_stage packs the next up to NT rows of a side into LDS as (b, d, w) triples, across diagram boundaries (a group of
//     15 diagrams of 46 rows is 690 rows = 2.7 chunks of 256, not 15 chunks of 46).  A row outside F is staged as
//     (0, 0, 0): its terms are (w * 0) * E = 0 and leave every sum as it is.
//   * an A block: every thread takes one staged row of A into registers;
//   * the B rows are staged chunk by chunk; in the inner loop every lane reads the SAME LDS address (a broadcast: no bank
//     conflict) and adds its term to its own float64 partial sum;
//   * after the last A block the NT partial sums go to LDS and wave 0 adds them in a fixed order: lane l takes the
//     partials l, l + 64, ..., then a butterfly over the lanes (partner lane ^ 32, 16, .., 1).
// The order of every addition depends on the two sides alone: no atomics, the same bytes for a pair or a tile alone and
// inside a batch.
//
// Kernels:
//   diagram_kernel_pairs  one wavefront per pair (NT = 64: a step's H0 diagrams have 46 finite rows, 72 % of a wave and
//                         18 % of a 256-thread workgroup): S(A, B), S(A, A), S(B, B), then the distance.
//   diagram_kernel_gram   one workgroup of 256 threads per (g, h) tile.  The symmetric form launches only the tiles
//                         h >= g (rows g and n - 1 - g of the triangle share one row of n + 1 workgroups) and writes
//                         G[h, g] as a copy of G[g, h].
// Loop bounds, all known before the loop starts: diagrams of a side, chunks ceil(rows / NT), rows of a chunk.  Nothing is
// allocated, nothing synchronises with the host, no scratch.
#include "common.h"
#include <cmath>

#pragma clang fp contract(off)

#define DK_GRAM_THREADS 256
#ifndef DK_PAIR_THREADS
#define DK_PAIR_THREADS 64          // make VARIANT=wg EXTRA=-DDK_PAIR_THREADS=256: a workgroup per pair, for the A/B of 3.15
#endif

struct dk_side {
    const double2* rows; const int* cnt; const int* status;      // status may be NULL
    int cap, w0, w1, skip_mask;
};

__device__ __forceinline__ double dk_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// rows of a kept diagram: min(cnt, cap), 0 for a diagram that is left out (wave-uniform)
__device__ __forceinline__ int dk_rows(const dk_side& S, int w)
{
    if (S.status && (uni(S.status[w]) & S.skip_mask)) return 0;
    int m = uni(S.cnt[w]);
    m = m < S.cap ? m : S.cap;
    return m < 0 ? 0 : m;
}

// The next rows of side S from the cursor (w, r) on, at most NT, into lds as (b, d, w) triples; returns how many.
// The cursor moves on; it is the same on every thread.
template <int NT>
__device__ __forceinline__ int dk_stage(const dk_side& S, int& w, int& r, int weight, double wc, double* lds)
{
    const int tid = (int)threadIdx.x;
    int fill = 0;
    while (w < S.w1 && fill < NT) {
        const int m = dk_rows(S, w);
        int take = m - r;
        take = take < NT - fill ? take : NT - fill;
        if (tid < take) {
            const double2 x = S.rows[(size_t)w * S.cap + r + tid];
            const bool ok = isfinite(x.x) && isfinite(x.y);
            const double p = x.y - x.x;
            double wt = 1.0;
            if (weight == TDA_KW_PERS) wt = p;
            else if (weight == TDA_KW_ATAN) wt = atan(wc * p);
            double* dst = lds + 3 * (fill + tid);
            dst[0] = ok ? x.x : 0.0; dst[1] = ok ? x.y : 0.0; dst[2] = ok ? wt : 0.0;
        }
        if (take > 0) { fill += take; r += take; }
        if (r >= m) { ++w; r = 0; }
    }
    return fill;
}

// S(A, B) by the NT threads of the workgroup: the value is valid on every lane of wave 0.  lds: 3 * NT doubles.
template <int NT, bool MIRROR>
__device__ __forceinline__ double dk_tile_sum(const dk_side& A, const dk_side& B, double ninv, int weight, double wc,
                                              double* lds)
{
    const int tid = (int)threadIdx.x;
    double part = 0.0;
    int wa = A.w0, ra = 0;
    for (;;) {
        __syncthreads();                                             // lds is free: everyone is past its last read
        const int na = dk_stage<NT>(A, wa, ra, weight, wc, lds);
        if (na == 0) break;                                          // (the same for every thread)
        __syncthreads();
        double bi = 0.0, di = 0.0, wi = 0.0;
        if (tid < na) { bi = lds[3 * tid]; di = lds[3 * tid + 1]; wi = lds[3 * tid + 2]; }
        int wb = B.w0, rb = 0;
        for (;;) {
            __syncthreads();
            const int nb = dk_stage<NT>(B, wb, rb, weight, wc, lds);
            if (nb == 0) break;
            __syncthreads();
            if (tid < na) {
#pragma unroll 2
                for (int j = 0; j < nb; ++j) {
                    const double bj = lds[3 * j], dj = lds[3 * j + 1], wj = lds[3 * j + 2];
                    const double dx = bi - bj, dy = di - dj;
                    const double a1 = (dx * dx + dy * dy) * ninv;
                    double e = exp(a1);
                    if (MIRROR) {
                        const double ex = bi - dj, ey = di - bj;
                        const double a2 = (ex * ex + ey * ey) * ninv;
                        e = e - exp(a2);
                    }
                    part = part + (wi * wj) * e;
                }
            }
        }
    }
    // every thread left both loops through a barrier: lds is free
    lds[tid] = part;
    __syncthreads();
    double v = 0.0;
    if (tid < 64) {
#pragma unroll
        for (int k = 0; k < NT; k += 64) v = v + lds[k + tid];
        v = dk_wave_sum(v);
    }
    return v;
}

template <bool MIRROR>
__global__ void __launch_bounds__(DK_PAIR_THREADS)
diagram_kernel_pairs(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int n_a, int cap_a,
                     const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int n_b, int cap_b,
                     const int* __restrict__ idx_a, const int* __restrict__ idx_b, int n_pairs, double ninv, double scale,
                     int weight, double wc, double* __restrict__ out, double* __restrict__ kvals, int* __restrict__ status)
{
    __shared__ double lds[3 * DK_PAIR_THREADS];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int ia = uni(idx_a ? idx_a[pr] : pr), ib = uni(idx_b ? idx_b[pr] : pr);
    if (ia < 0 || ia >= n_a || ib < 0 || ib >= n_b) {                 // (the same for every thread)
        if (threadIdx.x == 0) {
            out[pr] = qnan; status[pr] = TDA_WIN_NO_PAIR;
            if (kvals) { kvals[3 * (size_t)pr] = qnan; kvals[3 * (size_t)pr + 1] = qnan; kvals[3 * (size_t)pr + 2] = qnan; }
        }
        return;
    }
    const dk_side A = {reinterpret_cast<const double2*>(dgm_a), cnt_a, nullptr, cap_a, ia, ia + 1, 0};
    const dk_side B = {reinterpret_cast<const double2*>(dgm_b), cnt_b, nullptr, cap_b, ib, ib + 1, 0};
    const double k_ab = scale * dk_tile_sum<DK_PAIR_THREADS, MIRROR>(A, B, ninv, weight, wc, lds);
    const double k_aa = scale * dk_tile_sum<DK_PAIR_THREADS, MIRROR>(A, A, ninv, weight, wc, lds);
    const double k_bb = scale * dk_tile_sum<DK_PAIR_THREADS, MIRROR>(B, B, ninv, weight, wc, lds);
    if (threadIdx.x == 0) {
        const double s = k_aa + k_bb, t = k_ab + k_ab;
        const double d2 = s - t;
        out[pr] = sqrt(d2 > 0.0 ? d2 : 0.0);
        status[pr] = 0;
        if (kvals) { kvals[3 * (size_t)pr] = k_ab; kvals[3 * (size_t)pr + 1] = k_aa; kvals[3 * (size_t)pr + 2] = k_bb; }
    }
}

// diagrams [w0, w1) of group g and how many of them are kept
__device__ __forceinline__ dk_side dk_group(const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                                            const int* status, int skip_mask, int g, int* n_kept)
{
    int w0 = g, w1 = g + 1;                                          // seg_off == NULL: every diagram its own group
    if (seg_off) { w0 = uni(seg_off[g]); w1 = uni(seg_off[g + 1]); }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_dgm ? n_dgm : w1;
    int n = 0;
    for (int w = w0; w < w1; ++w) n += (status && (uni(status[w]) & skip_mask)) ? 0 : 1;
    *n_kept = n;
    const dk_side S = {reinterpret_cast<const double2*>(dgm), cnt, status, cap, w0, w1, skip_mask};
    return S;
}

// SYM: set B is set A; the grid holds ceil(n / 2) rows of n + 1 tiles, row r = the tiles (r, r..n-1) and (n-1-r, n-1-r..n-1)
template <bool MIRROR, bool SYM>
__global__ void __launch_bounds__(DK_GRAM_THREADS)
diagram_kernel_gram(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a, int n_a,
                    const int* __restrict__ seg_off_a, int n_ga, const int* __restrict__ status_a,
                    const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b, int n_b,
                    const int* __restrict__ seg_off_b, int n_gb, const int* __restrict__ status_b, int skip_mask,
                    double ninv, double scale, int weight, double wc, double* __restrict__ out)
{
    __shared__ double lds[3 * DK_GRAM_THREADS];
    int g, h;
    if (SYM) {
        const int r = (int)(blockIdx.x / (unsigned)(n_ga + 1)), c = (int)(blockIdx.x % (unsigned)(n_ga + 1));
        if (c < n_ga - r) { g = r; h = r + c; }
        else {
            g = n_ga - 1 - r; h = g + (c - (n_ga - r));
            if (g == r) return;                                      // the middle row of an odd n: already taken above
        }
    } else {
        g = (int)(blockIdx.x / (unsigned)n_gb); h = (int)(blockIdx.x % (unsigned)n_gb);
    }
    int n_g, n_h;
    const dk_side A = dk_group(dgm_a, cnt_a, cap_a, n_a, seg_off_a, status_a, skip_mask, g, &n_g);
    const dk_side B = dk_group(dgm_b, cnt_b, cap_b, n_b, seg_off_b, status_b, skip_mask, h, &n_h);
    double v = __longlong_as_double(0x7ff8000000000000ll);
    if (n_g > 0 && n_h > 0) {                                         // (the same for every thread)
        const double s = dk_tile_sum<DK_GRAM_THREADS, MIRROR>(A, B, ninv, weight, wc, lds);
        v = (scale * s) / (double)((long long)n_g * (long long)n_h);
    }
    if (threadIdx.x == 0) {
        out[(size_t)g * n_gb + h] = v;
        if (SYM) out[(size_t)h * n_gb + g] = v;
    }
}

// ---------------------------------------------------------------------------------
static tda_status dk_check(tda_ctx* ctx, double ninv, int mirror, double scale, int weight, double wc)
{
    if (!std::isfinite(ninv) || !(ninv < 0.0)) TDA_FAIL(ctx, TDA_ERR_INVALID, "ninv must be finite and < 0");
    if (mirror != 0 && mirror != 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "mirror must be 0 or 1");
    if (!std::isfinite(scale)) TDA_FAIL(ctx, TDA_ERR_INVALID, "scale must be finite");
    if (weight != TDA_KW_ONE && weight != TDA_KW_PERS && weight != TDA_KW_ATAN)
        TDA_FAIL(ctx, TDA_ERR_INVALID, "weight must be TDA_KW_ONE, TDA_KW_PERS or TDA_KW_ATAN");
    if (weight == TDA_KW_ATAN && !std::isfinite(wc)) TDA_FAIL(ctx, TDA_ERR_INVALID, "wc must be finite");
    return TDA_OK;
}

tda_status launch_diagram_kernel_pairs(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int n_a, int cap_a,
                                       const double* dgm_b, const int* cnt_b, int n_b, int cap_b, const int* idx_a,
                                       const int* idx_b, int n_pairs, double ninv, int mirror, double scale, int weight,
                                       double wc, double* out, double* kvals, int* status, hipStream_t st)
{
    const tda_status rc = dk_check(ctx, ninv, mirror, scale, weight, wc);
    if (rc != TDA_OK) return rc;
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_pairs == 0) return TDA_OK;
#define DK_LAUNCH(M)                                                                                                     \
    hipLaunchKernelGGL(diagram_kernel_pairs<M>, dim3(n_pairs), dim3(DK_PAIR_THREADS), 0, st, dgm_a, cnt_a, n_a, cap_a, dgm_b, \
                       cnt_b, n_b, cap_b, idx_a, idx_b, n_pairs, ninv, scale, weight, wc, out, kvals, status)
    if (mirror) DK_LAUNCH(true); else DK_LAUNCH(false);
#undef DK_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_diagram_kernel_gram(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                      const int* seg_off_a, int n_ga, const int* status_a, const double* dgm_b,
                                      const int* cnt_b, int cap_b, int n_b, const int* seg_off_b, int n_gb,
                                      const int* status_b, int skip_mask, double ninv, int mirror, double scale, int weight,
                                      double wc, double* out, hipStream_t st)
{
    const tda_status rc = dk_check(ctx, ninv, mirror, scale, weight, wc);
    if (rc != TDA_OK) return rc;
    const bool sym = dgm_b == nullptr;
    if (cap_a < 1 || (!sym && cap_b < 1)) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_ga == 0 || (!sym && n_gb == 0)) return TDA_OK;
    const long long tiles = sym ? (long long)((n_ga + 1) / 2) * (n_ga + 1) : (long long)n_ga * n_gb;
    if (tiles >= 0x7fffffffll) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "more than 2^31 - 2 tiles");
#define DK_LAUNCH(M, S)                                                                                                  \
    hipLaunchKernelGGL((diagram_kernel_gram<M, S>), dim3((unsigned)tiles), dim3(DK_GRAM_THREADS), 0, st, dgm_a, cnt_a, cap_a, \
                       n_a, seg_off_a, n_ga, status_a, S ? dgm_a : dgm_b, S ? cnt_a : cnt_b, S ? cap_a : cap_b,            \
                       S ? n_a : n_b, S ? seg_off_a : seg_off_b, S ? n_ga : n_gb, S ? status_a : status_b, skip_mask, ninv, \
                       scale, weight, wc, out)
    if (sym) { if (mirror) DK_LAUNCH(true, true); else DK_LAUNCH(false, true); }
    else { if (mirror) DK_LAUNCH(true, false); else DK_LAUNCH(false, false); }
#undef DK_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
