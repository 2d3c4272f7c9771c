// frechet.hip -- Frechet means and Frechet variances of persistence diagrams, per group (tda_frechet_mean[_dev|_batch];
// the contract is in include/tdaeeg.h).
//
// The algorithm of Turner, Mileyko, Mukherjee and Harer (2014): start from the first kept diagram of the group, match the
// iterate Y to every kept diagram X_i with the order-2 L2 costs of wasserstein_q.hip, replace every row of Y by the mean of
// its matches (pulled towards the diagonal for the diagrams that left it unmatched), let every unmatched row of an X_i
// spawn a row, and stop when the iterate does not change a byte.  Every cost and every update is one correctly rounded
// float64 operation of the header's text (the file is compiled with -ffp-contract=off).
//
// Mapping: one workgroup of ONE wavefront per group.  The solver is assign_dev.h's assign_solve, which holds the duals and
// the column state of one matching in the registers of one wavefront and synchronises with workgroup barriers in its
// row-reduction start; wavefronts of one workgroup solving different diagrams would have to meet those barriers in step,
// also the ones without a diagram in a round or with an empty one, which is not solved at all.  So the
// diagrams of a group are solved one after the other by the group's wavefront, and the
// parallelism across wavefronts comes from the groups (a pass has thousands).  The wavefront folds each matching into
// the accumulators at once, in ascending i: the order of the additions is the order of the diagrams.
//
// LDS (sized on the host: P rows of an iterate, Q = min(512, cap) rows of a diagram):
//   Y  b, d, s | accumulators sb, sd | spawned rows b, d        7 P doubles
//   X_i b, d, t                                                  3 Q doubles
//   k[P], mate[P] (the X row matched to Y row j, or -1), owner[P] (the solver's), xm[Q] (X row is matched)   ints
// Two launches.  The kernel is a chain of dependent steps, so what it delivers grows with the wavefronts a CU holds, and
// those are set by the LDS of a workgroup, which P dominates.  Means seldom have many more rows than their diagrams, so
// the first launch runs with P1 = max(128, cap rounded up to 64) rows (at most 512).  A group whose iterate outgrows P1
// leaves the marker -1 in mean_cnt and is done again from the start by the second launch, with P = 512; every other
// workgroup of that launch reads the count and leaves.  P limits an iterate and changes nothing else: a group gives the
// same bytes from either launch.  With P1 = 512 there is no second launch.
// Y never lies in global memory, so the loader is this file's own; of assign_lds only owner[] is used.
//
// The solver instance is chosen per matching from the number of columns (2, 4 or 8 column slots per lane): an iterate may
// grow past the capacity of the input buffers, up to FM_MAX_POINTS rows.  The matching assign_solve leaves does not
// depend on the instance: slots at or beyond cw_used take no part.
//
// Loop bounds, all known before the loop starts: diagrams of the group seg_off[g+1] - seg_off[g]; iterations max_iter;
// rows <= P, Q; the solver's are in assign_dev.h.  No atomics on floating point; spawn positions come from ballots and a
// running count.
#include "assign_dev.h"

#define FM_MAX_POINTS TDA_FM_MAX_POINTS
#define FM_MAX_GROUP  64
#define FM_AGAIN      (-1)      // mean_cnt of a group the first launch leaves to the second

struct fm_lds {
    double *yb, *yd, *ys, *sb, *sd, *nb, *nd, *xb, *xd, *xt;
    int *k, *mate, *owner, *xm;
    __device__ __forceinline__ fm_lds(unsigned char* smem, int P, int Q)
    {
        yb = reinterpret_cast<double*>(smem);
        yd = yb + P; ys = yd + P; sb = ys + P; sd = sb + P; nb = sd + P; nd = nb + P;
        xb = nd + P; xd = xb + Q; xt = xd + Q;
        k = reinterpret_cast<int*>(xt + Q);
        mate = k + P; owner = mate + P; xm = owner + P;
    }
};
static inline size_t fm_lds_bytes(int P, int Q) { return (size_t)(7 * P + 3 * Q) * 8 + (size_t)(3 * P + Q) * 4; }

__device__ __forceinline__ double fm_cost(double xb, double xd, double yb, double yd)
{
    const double dx = fabs(yb - xb), dy = fabs(yd - xd);
    return (dx * dx) + (dy * dy);
}
__device__ __forceinline__ double fm_diag(double b, double d)
{
    const double p = d - b;
    return 0.5 * (p * p);
}

// The finite rows of diagram w, in row order, with their diagonal costs; returns their number, or -1 (nothing loaded) if
// there are more than `limit`.  Wave-uniform.
__device__ __forceinline__ int fm_load(const double* __restrict__ dgm, const int* __restrict__ cnt, int cap, int w, int limit,
                                       double* pb, double* pd, double* pc)
{
    const int lane = lane_id();
    const double* D = dgm + (size_t)w * cap * 2;
    int kk = uni(cnt[w]); kk = kk < cap ? kk : cap; kk = kk < 0 ? 0 : kk;
    int n = 0;
    for (int i0 = 0; i0 < kk; i0 += 64) {
        const int i = i0 + lane;
        n += __popcll(__ballot(i < kk && isfinite(D[2 * i]) && isfinite(D[2 * i + 1])));
    }
    if (n > limit) return -1;
    int m = 0;
    for (int i0 = 0; i0 < kk; i0 += 64) {
        const int i = i0 + lane;
        double b = 0, d = 0; bool fin = false;
        if (i < kk) { b = D[2 * i]; d = D[2 * i + 1]; fin = isfinite(b) && isfinite(d); }
        const u64 bal = __ballot(fin);
        const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
        if (fin) { pb[pos] = b; pd[pos] = d; pc[pos] = fm_diag(b, d); }     // pos < n <= limit
        m += __popcll(bal);
    }
    return n;
}

// One matching: Y (n >= 1 rows) against X_i (ni >= 1 rows), rows = the smaller one (Y on a tie).  Leaves mate[] and xm[]
// (both cleared by the caller) for the real matches; false if a solver bound was hit.
template <int CW>
__device__ __forceinline__ bool fm_match(const fm_lds& F, int n, int ni)
{
    const int lane = lane_id();
    const bool y_row = n <= ni;
    assign_shape S;
    S.M = n; S.N = ni; S.a_is_row = y_row;
    S.R = y_row ? n : ni; S.Cn = y_row ? ni : n;
    S.cw_used = (S.Cn + 63) >> 6;
    assign_lds L(reinterpret_cast<unsigned char*>(F.yb), 0, 0);          // only owner[] is the solver's own
    L.owner = F.owner;
    const double* const rb = y_row ? F.yb : F.xb; const double* const rd = y_row ? F.yd : F.xd;
    const double* const rs = y_row ? F.ys : F.xt;
    const double* const cb = y_row ? F.xb : F.yb; const double* const cd = y_row ? F.xd : F.yd;
    const double* const ct = y_row ? F.xt : F.ys;
    auto cfull = [&](int i, int j) -> double { return fm_cost(rb[i], rd[i], cb[j], cd[j]); };
    auto gain = [&](int i, int j) -> double {
        const double g = cfull(i, j) - rs[i] - ct[j];
        return g < 0.0 ? g : 0.0;
    };
    int prow[CW], nsteps = 0;
    if (!assign_solve<CW>(S, L, gain, false, prow, nsteps)) return false;
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int j = lane + 64 * c;
        if (j < S.Cn && prow[c] >= 0 && prow[c] < S.R) {
            const int i = prow[c];
            if (cfull(i, j) - rs[i] - ct[j] < 0.0) {                     // a real match: the rule of assign_resum
                if (y_row) { F.mate[i] = j; F.xm[j] = 1; }
                else { F.mate[j] = i; F.xm[i] = 1; }
            }
        }
    }
    return true;
}

__global__ void __launch_bounds__(64)
frechet_mean_kernel(const double* __restrict__ dgm, const int* __restrict__ cnt, int cap, int n_dgm,
                    const int* __restrict__ seg_off, int n_seg, const int* __restrict__ status_in, int skip_mask,
                    int max_iter, int P, int Q, int second, double* __restrict__ mean, int* __restrict__ mean_cnt, int cap_out,
                    double* __restrict__ var, int* __restrict__ iters, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int g = blockIdx.x, lane = lane_id();
    if (g >= n_seg) return;
    if (second && uni(mean_cnt[g]) != FM_AGAIN) return;                  // done by the first launch
    const double QNAN = __longlong_as_double(0x7ff8000000000000ll);
    const fm_lds F(smem, P, Q);

    int w0 = g, w1 = g + 1;                                              // seg_off == NULL: every diagram its own group
    if (seg_off) { w0 = uni(seg_off[g]); w1 = uni(seg_off[g + 1]); }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_dgm ? n_dgm : w1;

    auto kept = [&](int w) -> bool { return !(status_in && (status_in[w] & skip_mask)); };
    auto kept_u = [&](int w) -> bool { return !(status_in && (uni(status_in[w]) & skip_mask)); };      // w wave-uniform
    auto leave = [&](int st, int it) {                                   // no mean: cnt 0, var NaN
        if (lane == 0) { mean_cnt[g] = 0; var[g] = QNAN; iters[g] = it; status[g] = st; }
    };

    int m = 0, first = -1;
    for (int wb = w0; wb < w1; wb += 64) {
        const int w = wb + lane;
        const u64 bal = __ballot(w < w1 && kept(w));
        if (first < 0 && bal) first = wb + __builtin_ctzll(bal);
        m += __popcll(bal);
    }
    if (m == 0) { leave(0, 0); return; }
    if (m > FM_MAX_GROUP) { leave(TDA_WIN_TOO_LARGE, 0); return; }
    const double md = (double)m;

    int n = fm_load(dgm, cnt, cap, first, Q, F.yb, F.yd, F.ys);
    if (n < 0) { leave(TDA_WIN_TOO_LARGE, 0); return; }

    int st_out = 0, it = 0;
    double Ft = 0.0;
    for (int t = 0; t < max_iter; ++t) {
        __syncthreads();
        for (int j = lane; j < n; j += 64) { F.sb[j] = 0.0; F.sd[j] = 0.0; F.k[j] = 0; }
        int ns = 0;                                                      // rows spawned so far, in the order (i, row)
        Ft = 0.0;
        for (int w = w0; w < w1; ++w) {
            if (!kept_u(w)) continue;
            __syncthreads();                                             // the previous diagram has been folded
            const int ni = fm_load(dgm, cnt, cap, w, Q, F.xb, F.xd, F.xt);
            if (ni < 0) { leave(TDA_WIN_TOO_LARGE, t); return; }
            for (int j = lane; j < n; j += 64) F.mate[j] = -1;
            for (int r = lane; r < ni; r += 64) F.xm[r] = 0;
            __syncthreads();
            if (n > 0 && ni > 0) {
                const int cols = n <= ni ? ni : n;
                bool ok;
                if (cols <= 128) ok = fm_match<2>(F, n, ni);
                else if (cols <= 256) ok = fm_match<4>(F, n, ni);
                else ok = fm_match<8>(F, n, ni);
                if (!ok) { leave(TDA_WIN_NOT_CONVERGED, t); return; }
            }
            __syncthreads();
            // fold: the matched births and deaths into the accumulators, V_i into 64 partial sums by index mod 64
            double part = 0.0;
            for (int j = lane; j < n; j += 64) {
                const int x = F.mate[j];
                if (x >= 0) {
                    F.sb[j] = F.sb[j] + F.xb[x]; F.sd[j] = F.sd[j] + F.xd[x]; F.k[j] = F.k[j] + 1;
                    part = part + fm_cost(F.xb[x], F.xd[x], F.yb[j], F.yd[j]);
                } else part = part + F.ys[j];
            }
            for (int r0 = 0; r0 < ni; r0 += 64) {
                const int r = r0 + lane;
                const bool un = r < ni && F.xm[r] == 0;
                const u64 bal = __ballot(un);
                const int pos = ns + __popcll(bal & ((1ull << lane) - 1ull));
                if (un) {
                    part = part + F.xt[r];
                    if (pos < P) {
                        double b = F.xb[r], d = F.xd[r];
                        if (m != 1) {
                            const double h = 0.5 * (b + d), far = (md - 1.0) * h;
                            b = ((1.0 * b) + far) / md; d = ((1.0 * d) + far) / md;
                        }
                        F.nb[pos] = b; F.nd[pos] = d;
                    }
                }
                ns += __popcll(bal);
            }
            Ft = Ft + wave_sum_f64(part);
        }
        it = t + 1;
        __syncthreads();
        // the new rows of the survivors, in place in the accumulators
        for (int j = lane; j < n; j += 64) {
            const int kk = F.k[j];
            if (kk > 0) {
                const double kd = (double)kk;
                double wb = F.sb[j] / kd, wd = F.sd[j] / kd;
                if (kk != m) {
                    const double h = 0.5 * (wb + wd), far = (md - kd) * h;
                    wb = ((kd * wb) + far) / md; wd = ((kd * wd) + far) / md;
                }
                F.sb[j] = wb; F.sd[j] = wd;
            }
        }
        __syncthreads();
        // Y^{t+1} = survivors in the order of j, then the spawned rows: its size, and whether it has the bytes of Y^t
        int s = 0; bool same = true;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool alive = j < n && F.k[j] > 0;
            const u64 bal = __ballot(alive);
            const int pos = s + __popcll(bal & ((1ull << lane) - 1ull));      // pos <= j < n
            if (alive) same = same && __double_as_longlong(F.sb[j]) == __double_as_longlong(F.yb[pos]) &&
                                       __double_as_longlong(F.sd[j]) == __double_as_longlong(F.yd[pos]);
            s += __popcll(bal);
        }
        const int n1 = s + ns;
        if (n1 == n)
            for (int q = lane; q < ns; q += 64)                                // s + q < n <= P, q < ns <= n <= P
                same = same && __double_as_longlong(F.nb[q]) == __double_as_longlong(F.yb[s + q]) &&
                               __double_as_longlong(F.nd[q]) == __double_as_longlong(F.yd[s + q]);
        same = n1 == n && __ballot(!same) == 0ull;
        if (same) break;                                                 // converged at t
        if (n1 > FM_MAX_POINTS) { leave(TDA_WIN_TOO_LARGE, it); return; }
        if (n1 > P) {                                                    // (first launch only: the second has P = FM_MAX_POINTS)
            if (lane == 0) mean_cnt[g] = FM_AGAIN;
            return;
        }
        if (t + 1 == max_iter) { st_out = TDA_WIN_NOT_CONVERGED; break; }    // the output stays Y^t with its own energy
        // Y <- Y^{t+1}
        s = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool alive = j < n && F.k[j] > 0;
            const u64 bal = __ballot(alive);
            const int pos = s + __popcll(bal & ((1ull << lane) - 1ull));
            if (alive) { F.yb[pos] = F.sb[j]; F.yd[pos] = F.sd[j]; }    // Y is not read in this pass
            s += __popcll(bal);
        }
        for (int q = lane; q < ns; q += 64) { F.yb[s + q] = F.nb[q]; F.yd[s + q] = F.nd[q]; }      // s + q < n1 <= P
        __syncthreads();
        n = n1;
        for (int j = lane; j < n; j += 64) F.ys[j] = fm_diag(F.yb[j], F.yd[j]);
    }
    __syncthreads();
    const int n_out = n < cap_out ? n : cap_out;
    double* o = mean + (size_t)g * cap_out * 2;
    for (int j = lane; j < n_out; j += 64) { o[2 * j] = F.yb[j]; o[2 * j + 1] = F.yd[j]; }
    if (lane == 0) {
        mean_cnt[g] = n; var[g] = Ft / md; iters[g] = it;
        status[g] = st_out | (n > cap_out ? TDA_WIN_H1_TRUNCATED : 0);
    }
}

tda_status launch_frechet_mean(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const int* seg_off,
                               int n_seg, const int* status_in, int skip_mask, int max_iter, double* mean, int* mean_cnt,
                               int cap_out, double* var, int* iters, int* status, hipStream_t st)
{
    if (cap < 1 || cap_out < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (max_iter < 1 || max_iter > TDA_FM_MAX_ITER) TDA_FAIL(ctx, TDA_ERR_INVALID, "max_iter must be 1..TDA_FM_MAX_ITER");
    if (n_seg == 0) return TDA_OK;
    const int Q = cap < FM_MAX_POINTS ? cap : FM_MAX_POINTS;
    int P1 = (Q + 63) & ~63;
    P1 = P1 < 128 ? 128 : P1;
    // LDS of a workgroup, first / second launch: 10,496 / 36,608 B at cap 64, 12,288 / 38,400 B at cap 128, 49,152 B at
    // cap 512 (one launch)
    for (int second = 0; second < 2; ++second) {
        const int P = second ? FM_MAX_POINTS : P1;
        hipLaunchKernelGGL(frechet_mean_kernel, dim3(n_seg), dim3(64), fm_lds_bytes(P, Q), st, dgm, cnt, cap, n_dgm, seg_off,
                           n_seg, status_in, skip_mask, max_iter, P, Q, second, mean, mean_cnt, cap_out, var, iters, status);
        if (P1 == FM_MAX_POINTS) break;
    }
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
