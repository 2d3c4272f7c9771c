// sublevel.hip -- H0 of the sublevel-set (lower-star) filtration of 1-D signals (include/tdaeeg.h, "Sublevel-set
// persistence of time series").
//
// The kernel evaluates the per-maximum form of the definition: every interior vertex p above both neighbours in the total
// order (x[i], i) gives the row (x[y], x[p], y, p), y the larger of the minima of the two maximal runs below p that touch
// it; no maximum needs another one's result.  A group of NT threads handles a signal:
//   1. coalesced load into LDS, the finiteness test and the global minimum (value, lowest index) on the way
//   2. classification of NT vertices at a time; the maxima are compacted in index order by ballot and prefix
//   3. one maximum per thread and pass: two scans over LDS, left and right, until a vertex above p ends the run --
//      sample by sample to the next block of SL_BLK samples, then block by block on the blocks' maxima and minima
//      (made after step 1), then sample by sample inside the block that holds the end: at most
//      2 * SL_BLK + n_t / SL_BLK steps where the plain scan of the global maximum takes n_t
//   4. the rows with birth < death are compacted the same way into LDS
//   5. every row counts the rows in front of it in (death, birth, death index) order (all threads read the same row:
//      broadcasts; the death alone unless a ballot finds equal deaths among the wave's rows) and goes to its rank in
//      LDS, over the samples, which nobody reads any more
//   6. coalesced store of rows [0, cnt) and of their indices
// NT = 64 for n_t <= 512: a wavefront per signal, four signals per workgroup, each wave with its own LDS slice and no
// barrier (the LDS serves the accesses of one wave in program order).  NT = 256 for n_t <= TDA_SL_MAX_SAMPLES: a
// workgroup per signal.  No atomics, nothing but rows [0, cnt) of the signal's own block is written.
#include "common.h"
#include <climits>

#define SL_BLOCK 256
#ifndef SL_BLK
#define SL_BLK 8                           // samples per block of the scans (a power of two; -DSL_BLK=: A/B builds)
#endif

template <int NT>
__device__ __forceinline__ void sl_sync()
{
    if constexpr (NT == 64) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

template <int NT, int NMAX>
struct SlLds {
    double x[NMAX + 2];                    // the samples; from step 5 on the ranked rows, (birth, death) interleaved
    double b[NMAX / 2], d[NMAX / 2];       // the kept rows in index order
    int y[NMAX / 2], p[NMAX / 2];          // p: first the maxima, then the kept rows' death indices
    union {
        int oi[NMAX + 2];                  // step 5: the ranked index pairs
        struct {                           // steps 2-3: per block of SL_BLK samples the maximum, the minimum and the
            double bmax[NMAX / SL_BLK], bmin[NMAX / SL_BLK];       // lowest index that holds the minimum
            int bmi[NMAX / SL_BLK];
        } blk;
    } u;
    double rv[NT / 64];                    // NT > 64: a (value, index) pair and a count per wave
    u32 ri[NT / 64];
    int wcnt[NT / 64];
};

// Slot of this thread's element among the flagged ones of the group, in thread order, behind `base`; base moves on by
// the group's count.  NT > 64: every thread of the workgroup calls it.
template <int NT>
__device__ __forceinline__ int sl_compact(bool f, int& base, int* wcnt)
{
    const u64 m = __ballot(f);
    const int lane = lane_id();
    int pos = __popcll(m & ((1ull << lane) - 1ull));
    if constexpr (NT == 64) {
        pos += base;
        base += __popcll(m);
    } else {
        const int wave = (int)threadIdx.x >> 6;
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const int c = wcnt[w];
            if (w < wave) pos += c;
            tot += c;
        }
        __syncthreads();
        pos += base;
        base += tot;
    }
    return pos;
}

template <int NT, int NMAX>
__global__ void __launch_bounds__(SL_BLOCK)
sublevel_kernel(const double* __restrict__ sig, const long long* __restrict__ win_start,
                const long long* __restrict__ win_ld, long long n_sig, int n_ch, int n_t, double* __restrict__ dgm, int cap,
                int* __restrict__ cnt, int* __restrict__ idx, int* __restrict__ status)
{
    constexpr int G = SL_BLOCK / NT;       // signals per workgroup
    constexpr int EPT = NMAX / NT;         // samples per thread
    constexpr int RPT = NMAX / 2 / NT;     // maxima per thread: a signal has at most (n_t - 1) / 2 < NMAX / 2
    __shared__ SlLds<NT, NMAX> lds[G];

    const int t = (int)threadIdx.x & (NT - 1), grp = (int)threadIdx.x / NT, lane = lane_id();
    const long long s = (long long)blockIdx.x * G + grp;
    if (s >= n_sig) return;                // a whole wave (NT = 64) or nobody (NT = 256: one signal per workgroup)
    SlLds<NT, NMAX>& L = lds[grp];
    const long long w = s / n_ch;
    const int c = (int)(s - w * n_ch);
    const double* src = win_start ? sig + win_start[w] + (long long)c * win_ld[w] : sig + s * n_t;

    // 1. load; the thread's minimum in the total order (strict <: its lowest index wins a tie)
    bool bad = false;
    double mv = INFINITY;
    u32 mi = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int i = t + j * NT;
        if (i < n_t) {
            const double v = src[i];
            L.x[i] = v;
            bad |= !__builtin_isfinite(v);
            if (v < mv) { mv = v; mi = (u32)i; }
        }
    }
    bool any_bad;
    if constexpr (NT == 64) { any_bad = __ballot(bad) != 0ull; sl_sync<NT>(); }
    else any_bad = __syncthreads_or(bad) != 0;
    if (any_bad) {
        if (t == 0) { cnt[s] = 0; status[s] = TDA_WIN_NOT_FINITE; }
        return;
    }
    double gv = wave_min_f64_dpp(mv);
    u32 gi = wave_min_u32_dpp(mv == gv ? mi : 0xffffffffu);
    if constexpr (NT > 64) {
        const int wave = (int)threadIdx.x >> 6;
        if (lane == 0) { L.rv[wave] = gv; L.ri[wave] = gi; }
        __syncthreads();
        gv = L.rv[0]; gi = L.ri[0];
#pragma unroll
        for (int k = 1; k < NT / 64; ++k) {
            const double v = L.rv[k];
            const u32 iv = L.ri[k];
            if (v < gv || (v == gv && iv < gi)) { gv = v; gi = iv; }
        }
    }
    const double xg = L.x[gi];             // gi < n_t: wave 0 holds sample 0, and every sample is finite

    // the blocks of the scans (only the last one may be short)
    for (int b = t; b * SL_BLK < n_t; b += NT) {
        const int i0 = b * SL_BLK;
        double hi = L.x[i0], lo = hi;
        int li = i0;
#pragma unroll
        for (int e = 1; e < SL_BLK; ++e) {
            if (i0 + e < n_t) {
                const double v = L.x[i0 + e];
                hi = v > hi ? v : hi;
                if (v < lo) { lo = v; li = i0 + e; }
            }
        }
        L.u.blk.bmax[b] = hi; L.u.blk.bmin[b] = lo; L.u.blk.bmi[b] = li;
    }

    // 2. the maxima: x[p - 1] <= x[p] (the left neighbour wins a tie by its index) and x[p + 1] < x[p]
    int M = 0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        if (j * NT < n_t - 1) {            // uniform over the group
            const int i = t + j * NT;
            bool f = false;
            if (i > 0 && i < n_t - 1) {
                const double xi = L.x[i];
                f = L.x[i - 1] <= xi && L.x[i + 1] < xi;
            }
            const int pos = sl_compact<NT>(f, M, L.wcnt);
            if (f) L.p[pos] = i;
        }
    }
    sl_sync<NT>();

    // 3. the two runs of every maximum.  Both are non-empty (the neighbours are below p) and end inside the signal or at
    // a vertex above p.  Leftwards a later vertex has the lower index and wins a tie; rightwards the earlier one does.
    double rb[RPT], rd[RPT];
    int ry[RPT], rp[RPT];
    bool keep[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int r = t + j * NT;
        rb[j] = rd[j] = 0.0; ry[j] = rp[j] = 0; keep[j] = false;
        if (r < M) {
            const int p = L.p[r];
            const double xp = L.x[p];
            int ml = p - 1, mr = p + 1;
            double vl = L.x[ml], vr = L.x[mr];
            {
                int q = p - 2;
                bool open = true;          // no vertex above p met yet
                for (; q >= 0 && (q & (SL_BLK - 1)) != SL_BLK - 1; --q) {
                    const double v = L.x[q];
                    if (!(v <= xp)) { open = false; break; }
                    if (v <= vl) { vl = v; ml = q; }
                }
                if (open) {
                    for (; q >= 0; q -= SL_BLK) {          // q is the last sample of a whole block
                        const int b = q / SL_BLK;
                        if (!(L.u.blk.bmax[b] <= xp)) break;
                        const double v = L.u.blk.bmin[b];
                        if (v <= vl) { vl = v; ml = L.u.blk.bmi[b]; }
                    }
                    for (; q >= 0; --q) {
                        const double v = L.x[q];
                        if (!(v <= xp)) break;
                        if (v <= vl) { vl = v; ml = q; }
                    }
                }
            }
            {
                int q = p + 2;
                bool open = true;
                for (; q < n_t && (q & (SL_BLK - 1)) != 0; ++q) {
                    const double v = L.x[q];
                    if (!(v < xp)) { open = false; break; }
                    if (v < vr) { vr = v; mr = q; }
                }
                if (open) {
                    for (; q < n_t; q += SL_BLK) {         // q is the first sample of a block, the last one maybe short
                        const int b = q / SL_BLK;
                        if (!(L.u.blk.bmax[b] < xp)) break;
                        const double v = L.u.blk.bmin[b];
                        if (v < vr) { vr = v; mr = L.u.blk.bmi[b]; }
                    }
                    for (; q < n_t; ++q) {
                        const double v = L.x[q];
                        if (!(v < xp)) break;
                        if (v < vr) { vr = v; mr = q; }
                    }
                }
            }
            const bool right = vr >= vl;   // ml < mr: the right minimum is the larger one on a tie
            rb[j] = right ? vr : vl; ry[j] = right ? mr : ml;
            rd[j] = xp; rp[j] = p;
            keep[j] = rb[j] < xp;          // birth == death: dropped
        }
    }
    sl_sync<NT>();                         // L.p is read; it takes the kept rows now

    // 4. the kept rows, in index order
    int K = 0;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        if (j * NT < M) {
            const int pos = sl_compact<NT>(keep[j], K, L.wcnt);
            if (keep[j]) { L.b[pos] = rb[j]; L.d[pos] = rd[j]; L.y[pos] = ry[j]; L.p[pos] = rp[j]; }
        }
    }
    sl_sync<NT>();
    K = uni(K);

    // 5. rank by counting: (death, birth, death index) ascending; the death indices differ, so the ranks do
    int rank[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        const int r = t + j * NT;
        rank[j] = 0;
        rd[j] = __longlong_as_double(0x7ff8000000000000ll);       // no row: NaN is neither above nor equal to any death
        if (r < K) { rb[j] = L.b[r]; rd[j] = L.d[r]; ry[j] = L.y[r]; rp[j] = L.p[r]; }
    }
    for (int k = 0; k < K; ++k) {
        const double dk = L.d[k];
        bool tie = false;
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            rank[j] += dk < rd[j] ? 1 : 0;
            tie |= dk == rd[j] && k != t + j * NT;
        }
        if (__ballot(tie) != 0ull) {       // equal deaths in this wave's rows: births, then death indices decide
            const double bk = L.b[k];
            const int pk = L.p[k];
#pragma unroll
            for (int j = 0; j < RPT; ++j)
                rank[j] += (dk == rd[j] && (bk < rb[j] || (bk == rb[j] && pk < rp[j]))) ? 1 : 0;
        }
    }
    // (x was last read in step 3, two synchronisations back: the ranked rows may go over it)
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        if (t + j * NT < K) {
            L.x[2 * rank[j]] = rb[j]; L.x[2 * rank[j] + 1] = rd[j];
            L.u.oi[2 * rank[j]] = ry[j]; L.u.oi[2 * rank[j] + 1] = rp[j];
        }
    }
    if (t == 0) {                          // the component of the global minimum never dies
        L.x[2 * K] = xg; L.x[2 * K + 1] = INFINITY;
        L.u.oi[2 * K] = (int)gi; L.u.oi[2 * K + 1] = -1;
    }
    sl_sync<NT>();

    // 6. rows [0, K]: K + 1 <= TDA_SL_ROWS(n_t) <= cap
    double* out = dgm + (size_t)s * cap * 2;
    for (int e = t; e < 2 * (K + 1); e += NT) out[e] = L.x[e];
    if (idx) {
        int* oi = idx + (size_t)s * cap * 2;
        for (int e = t; e < 2 * (K + 1); e += NT) oi[e] = L.u.oi[e];
    }
    if (t == 0) { cnt[s] = K + 1; status[s] = TDA_WIN_OK; }
}

tda_status launch_sublevel(tda_ctx* ctx, const double* sig, const long long* win_start, const long long* win_ld, int n_win,
                           int n_ch, int n_t, double* dgm, int cap, int* cnt, int* idx, int* status, hipStream_t st)
{
    if (n_t < 1 || n_t > TDA_SL_MAX_SAMPLES) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_t must be in [1, TDA_SL_MAX_SAMPLES]");
    if (n_ch < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_ch must be >= 1");
    if (cap < TDA_SL_ROWS(n_t)) TDA_FAIL(ctx, TDA_ERR_INVALID, "cap must be >= TDA_SL_ROWS(n_t)");
    if ((win_start == nullptr) != (win_ld == nullptr)) TDA_FAIL(ctx, TDA_ERR_INVALID, "win_start and win_ld go together");
    const long long n_sig = (long long)n_win * n_ch;
    if (n_sig == 0) return TDA_OK;
    if (n_sig > INT_MAX) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "more than 2^31 - 1 signals in one call");
#define SL_LAUNCH(NT, NMAX)                                                                                            \
    hipLaunchKernelGGL((sublevel_kernel<NT, NMAX>), dim3((unsigned)((n_sig + SL_BLOCK / NT - 1) / (SL_BLOCK / NT))),   \
                       dim3(SL_BLOCK), 0, st, sig, win_start, win_ld, n_sig, n_ch, n_t, dgm, cap, cnt, idx, status)
    if (n_t <= 256) SL_LAUNCH(64, 256);
    else if (n_t <= 512) SL_LAUNCH(64, 512);
    else SL_LAUNCH(256, TDA_SL_MAX_SAMPLES);
#undef SL_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
