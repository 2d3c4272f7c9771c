// bottleneck.hip -- batched bottleneck distance between persistence diagrams.
//
// Diagrams A and B are cleaned as safe_wasserstein cleans them (scripts/utils.py:182-187: rows with a non-finite entry
// are dropped, an empty diagram becomes {(0,0)}).  Ground cost between points: L-infinity,
//   C_ij = fmax(fabs(a_b - b_b), fabs(a_d - b_d));
// a point may go to the diagonal at cost 0.5 * (d - b), diagonal to diagonal is free; the distance is the minimum over
// matchings of the LARGEST matched cost (the definition of Hera, GUDHI and persim.bottleneck).  Every cost is one
// correctly rounded float64 operation on the inputs and the answer is one of them, picked by comparisons only: the value
// is the bits a CPU computes (tests/bottleneck_ref.py), not a close value.
//
// The solver, one pair per wavefront:
//   "distance <= v"  <=>  in the point-to-point graph with the edges C_ij <= v there is a matching that covers every
//   point whose own diagonal cost is > v, on both sides at once  <=>  (Mendelsohn-Dulmage) there is a matching that
//   covers those points of A AND there is a (possibly different) matching that covers those points of B.
// So a threshold is tested by two independent cover problems (bn_cover): adjacency rows of the points that must be
// matched as bit words (one __ballot per 64 points of the other side), then one augmenting-path search per such point,
// breadth first over the words.  The thresholds tested are real costs: the search bisects the BIT PATTERNS of the
// non-negative doubles between a lower bound (every point's cheapest option) and an upper bound (everything to the
// diagonal), and one pass over all cells (bn_scan) snaps each probe to the nearest cost below the middle, or, if there
// is none, to the nearest one above.  Every probe halves the interval of bit patterns: at most 64 probes.  No sort.
//
// Loop bounds, all known before the loop starts: probes <= 64; augmenting searches per cover <= points of the side;
// expansions per search <= points of the side + 1; path flips <= points of the side + 1.  A bound that is hit gives NaN
// and TDA_WIN_NOT_CONVERGED.
// Which pair a wavefront solves is a template parameter of the kernel (resolve(pr, ia, ib), the shape of
// wasserstein.hip's pair sources).
#include "assign_dev.h"         // ws_index_pairs, the pair source of the explicit index arrays

#ifdef TDA_PROFILE
// cycles: [0] load, [1] bounds, [2] candidate scans, [3] adjacency builds, [4] cover searches; counts: [5] pairs,
// [6] probes (feasibility tests), [7] augmenting searches, [8] expansions, [9] points of A, [10] points of B
__device__ unsigned long long g_prof_bn[16];
extern "C" __attribute__((visibility("default"))) int tda_profile_read_bn(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof_bn), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof_bn), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#define BPROF(i, v) do { if (lane_id() == 0) atomicAdd(&g_prof_bn[i], (unsigned long long)(v)); } while (0)
#define BCLK() clock64()
#else
#define BPROF(i, v) do {} while (0)
#define BCLK() 0ull
#endif

#define BN_MAX_POINTS 512       // points per diagram the kernel has LDS and lanes for (8 per lane)
#define BN_MAX_PROBES 64        // one per bit of the pattern of a non-negative double

// the same bits whichever diagram x comes from: fabs(x - y) == fabs(y - x)
__device__ __forceinline__ double bn_cost(double xb, double xd, double yb, double yd)
{
    return fmax(fabs(xb - yb), fabs(xd - yd));
}

__device__ __forceinline__ double bn_diag(double b, double d) { return 0.5 * (d - b); }

// a wave-uniform point out of LDS, as scalars
__device__ __forceinline__ void bn_point(const double* p, int i, double& b, double& d)
{
    b = uni_f64(p[2 * i], 0);
    d = uni_f64(p[2 * i + 1], 0);
}

// finite rows of one diagram into LDS as (b, d) pairs, order kept; none: {(0, 0)}
__device__ __forceinline__ void bn_load(const double* __restrict__ src, int k, int n_fin, double* dst)
{
    const int lane = lane_id();
    int m = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {
        const int i = i0 + lane;
        double b = 0, d = 0; bool fin = false;
        if (i < k) { b = src[2 * i]; d = src[2 * i + 1]; fin = isfinite(b) && isfinite(d); }
        const u64 bal = __ballot(fin);
        const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
        if (fin) { dst[2 * pos] = b; dst[2 * pos + 1] = d; }
        m += __popcll(bal);
    }
    if (n_fin == 0 && lane == 0) { dst[0] = 0.0; dst[1] = 0.0; }
}

// Every point of P (on lanes) against all of Q: lo = the largest "cheapest option" min(s_p, min_q C_pq), hi = the
// largest s_p.  Per lane; the caller reduces.
__device__ __forceinline__ void bn_bounds(const double* P, int NP, const double* Q, int NQ, double& lo, double& hi)
{
    const int lane = lane_id();
    for (int p0 = 0; p0 < NP; p0 += 64) {
        const int p = p0 + lane < NP ? p0 + lane : NP - 1;
        const double pb = P[2 * p], pd = P[2 * p + 1];
        const double s = bn_diag(pb, pd);
        double mn = s;
        for (int q = 0; q < NQ; ++q) mn = fmin(mn, bn_cost(pb, pd, Q[2 * q], Q[2 * q + 1]));
        lo = fmax(lo, mn);
        hi = fmax(hi, s);
    }
}

// One pass over every cost of the pair -- the cells (the points of X on lanes, those of Y one after the other) and the
// two sets of diagonal costs: dn = the largest cost <= mid (or -1), up = the smallest cost > mid (or +inf).  Wave-uniform.
__device__ __forceinline__ void bn_scan(const double* X, int NX, const double* Y, int NY, double mid, double& dn, double& up)
{
    const int lane = lane_id();
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double d = -1.0, u = INF;
    auto take = [&](double c) {
        d = fmax(d, c <= mid ? c : -1.0);
        u = fmin(u, c > mid ? c : INF);
    };
    for (int x0 = 0; x0 < NX; x0 += 64) {
        const int x = x0 + lane < NX ? x0 + lane : NX - 1;        // (the lanes past the end repeat the last point)
        const double xb = X[2 * x], xd = X[2 * x + 1];
        take(bn_diag(xb, xd));
        for (int y = 0; y < NY; ++y) take(bn_cost(xb, xd, Y[2 * y], Y[2 * y + 1]));
    }
    for (int y = lane; y < NY; y += 64) take(bn_diag(Y[2 * y], Y[2 * y + 1]));
    dn = wave_max_f64_dpp(d);
    up = wave_min_f64_dpp(u);
}

// Is there a matching in the graph {C_uv <= thr} that covers every point u of U with s_u > thr?  The points of V sit on
// lanes (v = lane + 64 c), match / parent per lane in registers; adj: NU x wv words, mu: partner of every u, q: the
// points of U whose rows the running search still has to look at.  -1: a loop bound was hit.
template <int CW>
__device__ __forceinline__ int bn_cover(const double* U, int NU, const double* V, int NV, double thr, u64* adj, int* mu, int* q)
{
    const int lane = lane_id();
    const int wv = (NV + 63) >> 6;
    unsigned long long t0 = BCLK();
    (void)t0;
    double vb[CW], vd[CW];
    int match[CW], par[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int v = lane + 64 * c < NV ? lane + 64 * c : NV - 1;
        vb[c] = V[2 * v]; vd[c] = V[2 * v + 1];
        match[c] = -1; par[c] = -1;
    }
    __syncthreads();                                                 // (the last search of the cover before is done with adj / mu / q)
    for (int u = lane; u < NU; u += 64) mu[u] = -1;
    for (int u = 0; u < NU; ++u) {
        double ub, ud;
        bn_point(U, u, ub, ud);
        if (!(bn_diag(ub, ud) > thr)) continue;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (c >= wv) break;
            const u64 bal = __ballot(lane + 64 * c < NV && bn_cost(ub, ud, vb[c], vd[c]) <= thr);
            if (lane == 0) adj[u * wv + c] = bal;
        }
    }
    __syncthreads();
    BPROF(3, BCLK() - t0); t0 = BCLK();
    int res = 1;
    for (int u0 = 0; u0 < NU && res == 1; ++u0) {
        double ub, ud;
        bn_point(U, u0, ub, ud);
        if (!(bn_diag(ub, ud) > thr)) continue;
        BPROF(7, 1);
        // ---- breadth-first search from u0 over alternating paths, one row of U per step
        u64 reached[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) reached[c] = 0ull;
        int head = 0, tail = 0, u = u0, vend = -1;
        bool open = true;
        for (int it = 0; it <= NU && open; ++it) {
            BPROF(8, 1);
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c >= wv || vend >= 0) break;
                const u64 nw = uni64(adj[u * wv + c]) & ~reached[c];
                if (nw == 0ull) continue;
                reached[c] |= nw;
                const bool mine = (nw >> lane) & 1ull;
                if (mine) par[c] = u;
                const u64 fb = __ballot(mine && match[c] < 0);
                if (fb) { vend = 64 * c + __builtin_ctzll(fb); break; }          // a free point of V: the path ends
                // every new point of V is matched: its partner's row is looked at later.  A partner enters once (each
                // v is new once), so at most NU - 1 entries.
                if (mine) q[tail + __popcll(nw & ((1ull << lane) - 1ull))] = match[c];
                tail += __popcll(nw);
            }
            if (vend >= 0 || head == tail) { open = false; break; }
            __syncthreads();
            u = uni(q[head]);
            ++head;
        }
        if (vend < 0) { res = open ? -1 : 0; break; }                          // nothing left to look at: u0 cannot be covered
        // ---- flip the path back to u0
        int v = vend;
        bool back = false;
        for (int g = 0; g <= NU; ++g) {
            int pu = -1;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == (v >> 6)) pu = (int)rl32((u32)par[c], v & 63);
            const int vprev = pu == u0 ? -1 : uni(mu[pu]);
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == (v >> 6) && lane == (v & 63)) match[c] = pu;
            if (lane == 0) mu[pu] = v;
            if (vprev < 0) { back = true; break; }
            v = vprev;
        }
        __syncthreads();
        if (!back) res = -1;
    }
    BPROF(4, BCLK() - t0);
    return res;
}

// pair pr, by the one wave of the workgroup.  LDS: points of A | points of B | adj | mu | q  (bn_lds_bytes)
template <int CW, class SRC>
__device__ __forceinline__ void bn_solve(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                                         const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                                         const SRC& src, int pr, int max_a, int max_b, int adj_words,
                                         double* __restrict__ out, int* __restrict__ status, unsigned char* smem)
{
    const int lane = lane_id();
    const double QNAN = __longlong_as_double(0x7ff8000000000000ll);
    unsigned long long t0 = BCLK();
    (void)t0;
    double* pa = reinterpret_cast<double*>(smem);
    double* pb = pa + 2 * max_a;
    u64* adj = reinterpret_cast<u64*>(pb + 2 * max_b);
    int* mu = reinterpret_cast<int*>(adj + adj_words);
    int* q = mu + (max_a > max_b ? max_a : max_b);

    int ia, ib;
    if (!src.resolve(pr, ia, ib)) {
        if (lane == 0) { out[pr] = QNAN; status[pr] = TDA_WIN_NO_PAIR; }
        return;
    }
    const double* A = dgm_a + (size_t)ia * cap_a * 2;
    const double* B = dgm_b + (size_t)ib * cap_b * 2;
    int ka = uni(cnt_a[ia]); ka = ka < cap_a ? ka : cap_a; ka = ka < 0 ? 0 : ka;
    int kb = uni(cnt_b[ib]); kb = kb < cap_b ? kb : cap_b; kb = kb < 0 ? 0 : kb;
    int M = 0, N = 0;                                                // finite rows (utils.py:185-186)
    for (int i0 = 0; i0 < ka; i0 += 64) {
        const int i = i0 + lane;
        M += __popcll(__ballot(i < ka && isfinite(A[2 * i]) && isfinite(A[2 * i + 1])));
    }
    for (int i0 = 0; i0 < kb; i0 += 64) {
        const int i = i0 + lane;
        N += __popcll(__ballot(i < kb && isfinite(B[2 * i]) && isfinite(B[2 * i + 1])));
    }
    const int Me = M > 0 ? M : 1, Ne = N > 0 ? N : 1;                // empty -> {(0,0)}  (utils.py:184,187)
    if (Me > max_a || Ne > max_b || Me > 64 * CW || Ne > 64 * CW) {  // more points than the launch has room for
        if (lane == 0) { out[pr] = QNAN; status[pr] = TDA_WIN_NOT_CONVERGED; }
        return;
    }
    bn_load(A, ka, M, pa);
    bn_load(B, kb, N, pb);
    __syncthreads();
    BPROF(0, BCLK() - t0); t0 = BCLK();
    BPROF(5, 1); BPROF(9, Me); BPROF(10, Ne);

    // ---- bounds: every point's cheapest option below, everything to the diagonal above (both are costs of the pair)
    double lo = 0.0, hi = 0.0;
    bn_bounds(pa, Me, pb, Ne, lo, hi);
    bn_bounds(pb, Ne, pa, Me, lo, hi);
    lo = wave_max_f64_dpp(lo);
    hi = wave_max_f64_dpp(hi);
    BPROF(1, BCLK() - t0);

    auto feasible = [&](double v) -> int {
        BPROF(6, 1);
        const int ra = bn_cover<CW>(pa, Me, pb, Ne, v, adj, mu, q);
        if (ra != 1) return ra;
        return bn_cover<CW>(pb, Ne, pa, Me, v, adj, mu, q);
    };
    // the larger diagram on the lanes of the scans
    const bool a_wide = Me >= Ne;
    const double* X = a_wide ? pa : pb; const double* Y = a_wide ? pb : pa;
    const int NX = a_wide ? Me : Ne, NY = a_wide ? Ne : Me;

    // ---- the smallest feasible cost in [lo, hi]: hi is feasible (nothing has to be matched)
    bool done = !(lo < hi), failed = false;
    if (!done) {
        const int f = feasible(lo);
        if (f < 0) failed = true;
        else if (f == 1) { hi = lo; done = true; }
    }
    // now: lo is not feasible, hi is, both are costs.  Bisection on the bit patterns (monotone for doubles >= 0).
    for (int it = 0; it < BN_MAX_PROBES && !done && !failed; ++it) {
        const u64 lb = (u64)__double_as_longlong(lo), hb = (u64)__double_as_longlong(hi);
        const double mid = __longlong_as_double((long long)(lb + ((hb - lb) >> 1)));
        unsigned long long t1 = BCLK();
        (void)t1;
        double dn, up;
        bn_scan(X, NX, Y, NY, mid, dn, up);
        BPROF(2, BCLK() - t1);
        if (dn > lo) {                                  // the largest cost in (lo, mid]
            const int f = feasible(dn);
            if (f < 0) failed = true;
            else if (f == 1) hi = dn;
            else lo = mid;                              // (no cost in (dn, mid])
        } else if (!(up < hi)) {
            done = true;                                // no cost between lo and hi: hi is the answer
        } else {                                        // no cost in (lo, mid]: the smallest one above
            const int f = feasible(up);
            if (f < 0) failed = true;
            else if (f == 1) { hi = up; done = true; }  // (no cost in (lo, up))
            else lo = up;
        }
    }
    if (lane == 0) {
        const bool ok = done && !failed;
        out[pr] = ok ? hi : QNAN;
        status[pr] = ok ? 0 : TDA_WIN_NOT_CONVERGED;
    }
}

template <int CW, class SRC>
__global__ void __launch_bounds__(64)
bottleneck_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                  const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                  const SRC src, int n_pairs, int max_a, int max_b, int adj_words,
                  double* __restrict__ out, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    bn_solve<CW, SRC>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, pr, max_a, max_b, adj_words, out, status, smem);
}

// ---------------------------------------------------------------------------------
// One launch, sized by the capacities of the two diagram buffers (at most BN_MAX_POINTS points each: a buffer may be
// larger, a pair with more finite points than that is TDA_WIN_NOT_CONVERGED).
template <class SRC>
static tda_status launch_bottleneck_src(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                                        const int* cnt_b, int cap_b, const SRC& src, int n_pairs, double* out, int* status,
                                        hipStream_t st)
{
    if (n_pairs == 0) return TDA_OK;
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    const int max_a = cap_a < BN_MAX_POINTS ? cap_a : BN_MAX_POINTS, max_b = cap_b < BN_MAX_POINTS ? cap_b : BN_MAX_POINTS;
    const int wa = (max_a + 63) >> 6, wb = (max_b + 63) >> 6;
    const int adj_words = max_a * wb > max_b * wa ? max_a * wb : max_b * wa;
    const int hi = max_a > max_b ? max_a : max_b;
    // points 16 B each, adjacency words, partner table, search list (padded to 8 B)
    const size_t lds = (size_t)(2 * max_a + 2 * max_b + adj_words + hi + 1) * 8;
#define BN_LAUNCH(CWV)                                                                                         \
    do {                                                                                                       \
        auto kern = bottleneck_kernel<CWV, SRC>;                                                               \
        if (lds > 48 * 1024)                                                                                   \
            TDA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                              \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));           \
        hipLaunchKernelGGL(kern, dim3(n_pairs), dim3(64), lds, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b,   \
                           src, n_pairs, max_a, max_b, adj_words, out, status);                                \
    } while (0)
    if (hi <= 128) BN_LAUNCH(2);
    else if (hi <= 256) BN_LAUNCH(4);
    else BN_LAUNCH(8);
#undef BN_LAUNCH
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_bottleneck(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                             const int* cnt_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs,
                             double* out, int* status, hipStream_t st)
{
    return launch_bottleneck_src(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, ws_index_pairs{idx_a, idx_b}, n_pairs, out,
                                 status, st);
}
