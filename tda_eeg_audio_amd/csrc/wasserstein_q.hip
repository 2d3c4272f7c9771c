// wasserstein_q.hip -- batched Wasserstein distances of order 1 and 2 between persistence diagrams, with the L2 or the
// L-infinity ground metric (tda_wasserstein_q_batch[_dev]; the contract is in include/tdaeeg.h).
//
// Diagrams are cleaned as safe_wasserstein cleans them (scripts/utils.py:182-187).  With dx = fabs(a_b - b_b),
// dy = fabs(a_d - b_d) and p = d - b, every line one correctly rounded float64 operation (no multiply-add):
//   L2:    e = (dx * dx) + (dy * dy);  order 1: C = sqrt(e), diagonal p * 0.7071067811865476
//                                      order 2: C = e,       diagonal 0.5 * (p * p)
//   L-inf: m = fmax(dx, dy), h = 0.5 * p;  order 1: C = m, diagonal h;  order 2: C = m * m, diagonal h * h
// V = min over partial matchings of the matched C plus the diagonal costs of every unmatched point; the result is V
// (order 1) or sqrt(V) (order 2).  The costs are symmetric in the two diagrams (fabs), so which one plays the row role
// does not change a bit of any cost.
//
// The pair prologue, the solver and the re-summation are assign_dev.h's, the ones wasserstein.hip runs: the rectangular
// assignment with gains g_ij = min(0, C_ij - s_i - t_j), rows = the smaller diagram, points and diagonal costs in LDS
// and no cost matrix, shortest augmenting paths after a row-reduction start, and a returned value that re-sums the
// ORIGINAL costs of the optimal matching.  This file hands in its costs and keeps its own pruning tests and its own
// equal-birth recurrence: two diagrams whose points all have one birth and ascending deaths take that instead (below).
// Order and ground metric are template parameters: a cell of the order-2 L2 solver has no root and no select.
//
// One launch, sized by the capacities of the two buffers (launch_bottleneck_src's): the small-launch-plus-list scheme
// of the order-1 kernel is not part of this.
//
// Loop bounds: the solver's are in assign_dev.h; wavefront steps = live rows + live columns - 1.  A bound that is hit
// gives NaN and TDA_WIN_NOT_CONVERGED.
#include "assign_dev.h"

#define WQ_MAX_POINTS 512       // points per diagram the kernel has LDS and lanes for (8 per lane)
#define WQ_CP 0.7071067811865476

// the point cost from the two coordinate differences (both >= 0)
template <int ORDER, int GROUND>
__device__ __forceinline__ double wq_of_diffs(double dx, double dy)
{
    if (GROUND == TDA_GROUND_L2) {
        const double e = (dx * dx) + (dy * dy);
        return ORDER == 1 ? sqrt_rn(e) : e;             // (sqrt() bit for bit: common.h)
    }
    const double m = fmax(dx, dy);
    return ORDER == 1 ? m : m * m;
}

// the same bits whichever diagram x comes from: fabs(x - y) == fabs(y - x)
template <int ORDER, int GROUND>
__device__ __forceinline__ double wq_cost(double xb, double xd, double yb, double yd)
{
    return wq_of_diffs<ORDER, GROUND>(fabs(xb - yb), fabs(xd - yd));
}

// the point cost when dx is +0.0 (equal births): 0.0 + dy * dy and fmax(0.0, dy) are dy * dy and dy, bit for bit
template <int ORDER, int GROUND>
__device__ __forceinline__ double wq_cost_line(double dy)
{
    if (GROUND == TDA_GROUND_L2) {
        const double e = dy * dy;
        return ORDER == 1 ? sqrt_rn(e) : e;
    }
    return ORDER == 1 ? dy : dy * dy;
}

template <int ORDER, int GROUND>
__device__ __forceinline__ double wq_diag(double b, double d)
{
    const double p = d - b;
    if (GROUND == TDA_GROUND_L2) return ORDER == 1 ? p * WQ_CP : 0.5 * (p * p);
    const double h = 0.5 * p;
    return ORDER == 1 ? h : h * h;
}

// ---- the margins of the pruning tests ----
// wq_solve leaves out cells whose gain g = min(0, C - s - t) is known to be 0.  What has to be 0 is the COMPUTED gain,
// (C_c - s_c) - t_c in floating point (the subscript c: the float64 the kernel holds).  It is 0 whenever
// C_c >= s_c + t_c as reals: rounding is monotone and t_c is a float64, so fl(C_c - s_c) >= t_c and the second
// difference is >= 0 (+inf included).  Unlike sklearn's expansion in wasserstein.hip these costs are built from direct
// differences: no cancellation term, and most of the argument needs no margin at all.
//
// General path (boxes).  gx = fmax(0, cb_lo - rb_hi, rb_lo - cb_hi) is one rounded subtraction of a real gap that no
// cell's |a_b - b_b| falls below, so gx <= dx_c in EVERY cell, as computed values; likewise gy.  wq_of_diffs() is a
// chain of monotone, correctly rounded operations of (dx, dy) >= 0 (product, sum, root, fmax), so
// L_c = wq_of_diffs(gx, gy) <= C_c in every cell, exactly.  (The L-infinity distance of two boxes is fmax(gx, gy), not the
// root; the order-2 form compares L^2 with s^2 + t^2, the tight test, because L_c and the diagonal costs are already the
// order-2 costs.)  What is left is one addition: T = fl(s_hi + t_hi) may fall below the real s_c + t_c of a cell by a
// factor (1 - u), u = 2^-53.  The test is L_c > fl(T * (1 + WQ_PRUNE_REL)): in the normal range
// fl(T * k) >= (s + t)(1 - u)^2 k > s + t, and where T is subnormal the addition was exact and fl(T * k) >= T.
// WQ_PRUNE_REL = 1e-12 is some thousand times what is needed.
// Overflow (there are squares): if s_hi or t_hi is +inf the test is false and nothing is left out; if L_c is +inf and
// the right side finite, C_c = +inf in every cell and the computed gain is +inf, clamped to 0.  NaN on either side makes
// the test false.
//
// Equal-birth path (live ranges).  Here s grows with the row, so a bound over the rows would prune nothing; the test
// is on the ratio r >= 1 of the larger to the smaller persistence of a cell.  As reals, with C = |p - q|^o,
// s = kappa p^o, t = kappa q^o (kappa = 1/sqrt 2, 1/2 for L2; 1/2, 1/4 for L-infinity): g < 0 exactly when r < cut,
//      (1, L2) 3 + 2 sqrt 2     (2, L2) 2 + sqrt 3     (1, L-inf) 3     (2, L-inf) (4 + sqrt 7) / 3
// and C / (s + t) grows with r; at r = cut (1 + delta) it is 1 + k delta with k between 0.35 and 2 for the four
// variants.  The computed C_c, s_c, t_c carry at most four relative errors of u each (one subtraction, then one or two
// products), so delta = WQ_LINE_REL = 1e-9 leaves C_c / (s_c + t_c) >= 1 + 3e-10 - 12 u > 1; the test's own product
// and sum cost 2 u more.  Underflow breaks relative bounds, so the larger persistence of a trimmed cell must be at
// least WQ_LINE_ABS = 1e-150, which the test adds: then p - q >= 0.54 p and the squares of p, p / 2 and p - q are
// normal numbers (>= 2.5e-301), while the smaller point's square may underflow by at most 2^-1074, far below
// 3e-10 (s + t).  Overflow: pairs with a |coordinate| >= WQ_LINE_MAX = 1e150 are not trimmed.
#define WQ_PRUNE_REL 1e-12
#define WQ_LINE_REL 1e-9
#define WQ_LINE_ABS 1e-150
#define WQ_LINE_MAX 1e150

template <int ORDER, int GROUND>
__device__ __forceinline__ constexpr double wq_cut()
{
    return (GROUND == TDA_GROUND_L2 ? (ORDER == 1 ? 5.828427124746190 : 3.7320508075688772)
                                    : (ORDER == 1 ? 3.0 : 2.2152504370215302)) * (1.0 + WQ_LINE_REL);
}

// pair pr, by the one wave of the workgroup
template <int CW, int ORDER, int GROUND, class SRC>
__device__ __forceinline__ void wq_solve(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                                         const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                                         const SRC& src, int pr, int max_rows, int max_cols,
                                         double* __restrict__ out, int* __restrict__ status, const ws_opts& opt,
                                         unsigned char* smem)
{
    const int lane = lane_id();
    const double QNAN = __longlong_as_double(0x7ff8000000000000ll);
    const assign_lds L(smem, max_rows, max_cols);
    double* const rb = L.rb; double* const rd = L.rd; double* const rs = L.rs;
    double* const cb = L.cb; double* const cd = L.cd; double* const ct = L.ct;

    int ia, ib;
    // (ws_index_pairs, the one source today, always has a pair: the branch is for a source that reads group tables, as
    // ws_table_pairs does, and no test can reach it until there is one)
    if (!src.resolve(pr, ia, ib)) {                                     // no pair: leave before the solver
        if (lane == 0) { out[pr] = QNAN; status[pr] = TDA_WIN_NO_PAIR; }
        return;
    }
    assign_shape S;
    auto diag = [](double b, double d) -> double { return wq_diag<ORDER, GROUND>(b, d); };
    if (!assign_load_pair<CW>(dgm_a, cnt_a, cap_a, ia, dgm_b, cnt_b, cap_b, ib, L, diag, S)) {
        if (lane == 0) {                                                // more points than the launch has room for
            out[pr] = QNAN; status[pr] = TDA_WIN_NOT_CONVERGED;
            if (opt.ctr) atomicAdd(&opt.ctr[2], 1ull);                  // counted like a pair whose solver hit a bound
        }
        return;
    }
    const int R = S.R, Cn = S.Cn;

    auto cfull = [&](int i, int j) -> double {   // original point-to-point cost of row i, col j
        return wq_cost<ORDER, GROUND>(rb[i], rd[i], cb[j], cd[j]);
    };
    auto gain = [&](int i, int j) -> double {
        const double g = cfull(i, j) - rs[i] - ct[j];
        return g < 0.0 ? g : 0.0;
    };
    auto finish = [&](double V) -> double { return ORDER == 1 ? V : sqrt_rn(V); };
    unsigned long long n_cut = 0, n_trim = 0;           // for opt.ctr
    auto count = [&]() {
        if (opt.ctr && lane == 0) {
            if (n_cut) atomicAdd(&opt.ctr[0], n_cut);
            if (n_trim) atomicAdd(&opt.ctr[1], n_trim);
            atomicAdd(&opt.ctr[2], 1ull);
        }
    };

    // ---- equal-birth path ---------------------------------------------------------------
    // If every point of both diagrams has the same birth (two H0 diagrams) the points lie on a line, the ground cost is
    // a convex function of |d_i - d_j| (|x| or x^2, either metric) and, for any fixed sets of matched points, the sorted
    // (non-crossing) pairing is optimal.  The optimum over partial matchings is then the edit-distance style recurrence
    //   F[i][j] = min(F[i-1][j], F[i][j-1], F[i-1][j-1] + g_ij)
    // over death-sorted diagrams: an anti-diagonal wavefront with one row per lane, R + C - 1 steps instead of hundreds
    // of Dijkstra steps.  Same gains g_ij as the general solver: dx is +0.0 here, and wq_cost_line() gives wq_cost()'s bits.
    {
        const double b0 = rb[0];
        if (assign_on_sorted_line(S, L)) {
            // ---- live ranges ----
            // With p the persistence of a row and q of a column, a cell with p >= cut q or q >= cut p (by the margins
            // above) has a computed gain of 0.  A column with cut q + abs <= p_min or q >= cut p_max + abs is dead for
            // EVERY row; both tests are monotone in q and the deaths are sorted, so the dead columns are a prefix and a
            // suffix, counted by ballots; then the same for the rows against the live columns.  F is 0 over a dead
            // prefix and constant over a dead suffix (F never increases along a row or a column, and min() is exact), so
            // the wavefront over the live ranges, zero boundary included, performs in every live cell what the full one
            // performs there: the same operations on the same operands in the same order, hence the same bits.
            int ilo = 0, jlo = 0, Rl = R, Cl = Cn;
            constexpr double CUT = wq_cut<ORDER, GROUND>();
            double mx = WQ_LINE_MAX;
            if (opt.prune)
                mx = fmax(fabs(b0), fmax(fmax(fabs(rd[0]), fabs(rd[R - 1])), fmax(fabs(cd[0]), fabs(cd[Cn - 1]))));
            if (mx < WQ_LINE_MAX) {
                const double p_min = rd[0] - b0, p_max = rd[R - 1] - b0;
                const double hi_c = p_max * CUT + WQ_LINE_ABS;
                int n_lo = 0, n_hi = 0;
                for (int j0 = 0; j0 < Cn; j0 += 64) {
                    const int j = j0 + lane;
                    const double q = cd[j < Cn ? j : Cn - 1] - b0;
                    n_lo += __popcll(__ballot(j < Cn && q * CUT + WQ_LINE_ABS <= p_min));
                    n_hi += __popcll(__ballot(j < Cn && q >= hi_c));
                }
                jlo = n_lo;
                const int jhi = Cn - n_hi > jlo ? Cn - n_hi : jlo;
                Cl = jhi - jlo;
                Rl = 0;
                if (Cl > 0) {
                    const double q_min = cd[jlo] - b0, q_max = cd[jhi - 1] - b0;
                    const double hi_r = q_max * CUT + WQ_LINE_ABS;
                    const double p = rd[lane < R ? lane : R - 1] - b0;
                    ilo = __popcll(__ballot(lane < R && p * CUT + WQ_LINE_ABS <= q_min));
                    const int ihi = R - __popcll(__ballot(lane < R && p >= hi_r));
                    Rl = ihi > ilo ? ihi - ilo : 0;
                }
                n_trim = (unsigned long long)((R - Rl) + (Cn - Cl));
            }
            double cur = 0.0, nb1 = 0.0, nb2 = 0.0;      // own F, neighbour row's F one / two steps ago
            const int nsteps1d = (Rl > 0 && Cl > 0) ? Rl + Cl - 1 : 0;      // an empty live range: no wavefront, fbest = 0
            const int li = lane < Rl ? ilo + lane : 0;                      // lane = live row index
            const double r_d = rd[li], r_s = rs[li];
            for (int t = 0; t < nsteps1d; ++t) {
                const int j0 = t - lane;
                // neighbour (row lane-1) value of the previous step; row 0 sees the zero boundary
                const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(cur), 0x138, 0xF, 0xF, false);
                const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(cur), 0x138, 0xF, 0xF, false);
                nb2 = nb1;
                nb1 = __hiloint2double(hi, lo);
                if (lane < Rl && j0 >= 0 && j0 < Cl) {
                    double g = wq_cost_line<ORDER, GROUND>(fabs(r_d - cd[jlo + j0])) - r_s - ct[jlo + j0];
                    g = g < 0.0 ? g : 0.0;
                    const double up = nb1;                          // F[row][j0+1] of the row above
                    const double dg = (j0 == 0 ? 0.0 : nb2) + g;    // F[row above][j0] + g
                    double m = up < cur ? up : cur;                 // cur still holds F[row+1][j0] (left)
                    m = dg < m ? dg : m;
                    cur = m;
                }
            }
            const double fbest = nsteps1d ? uni_f64(cur, Rl - 1) : 0.0;
            double part = 0.0;
            for (int i = lane; i < R; i += 64) part += rs[i];
            for (int j = lane; j < Cn; j += 64) part += ct[j];
            double total1d = wave_sum_f64(part) + fbest;
            // V >= 0; the sum of the diagonal costs and the sum of the gains are rounded separately, so a V of 0 may come
            // out a few ulps of the diagonal costs below it
            if (total1d < 0.0) total1d = 0.0;
            if (lane == 0) { out[pr] = finish(total1d); status[pr] = 0; }
            count();
            return;
        }
    }

    // ---- every cell dead? ---------------------------------------------------------------
    // If every point is nearer to the diagonal than to any point of the other diagram, every gain clamps to 0: the row
    // reduction finds u = 0, nothing is augmented, and the final summation adds every s and every t in its usual order.
    // Then that summation alone gives the same bits.  The test: the cost between the two bounding boxes against
    // s_max + t_max (one compare), else each row's cost to the box of the columns against s_i + t_max.  A pair with a
    // live cell runs the solver unchanged: compacting a partly live problem could break ties differently.
    bool all_dead = false;
    if (opt.prune) {
        const auto [rb_lo, rb_hi, rd_lo, rd_hi, s_hi, cb_lo, cb_hi, cd_lo, cd_hi, t_hi] = assign_box_stats(S, L);
        const double k = 1.0 + WQ_PRUNE_REL;
        const double gx = fmax(0.0, fmax(cb_lo - rb_hi, rb_lo - cb_hi));
        const double gy = fmax(0.0, fmax(cd_lo - rd_hi, rd_lo - cd_hi));
        all_dead = wq_of_diffs<ORDER, GROUND>(gx, gy) > (s_hi + t_hi) * k;
        if (!all_dead) {
            bool live = false;
            for (int i0 = 0; i0 < R; i0 += 64) {
                const int i = i0 + lane < R ? i0 + lane : R - 1;
                const double dx = fmax(0.0, fmax(cb_lo - rb[i], rb[i] - cb_hi));
                const double dy = fmax(0.0, fmax(cd_lo - rd[i], rd[i] - cd_hi));
                live = live || __ballot(!(wq_of_diffs<ORDER, GROUND>(dx, dy) > (rs[i] + t_hi) * k)) != 0ull;
            }
            all_dead = !live;
        }
        if (all_dead) n_cut = 1;
    }

    int prow[CW], nsteps = 0;
    if (!assign_solve<CW>(S, L, gain, all_dead, prow, nsteps)) {
        if (lane == 0) { out[pr] = QNAN; status[pr] = TDA_WIN_NOT_CONVERGED; }
        count();
        return;
    }
    // V = sum over real matches of C_ij + unmatched rows' s + unmatched cols' t
    const double total = assign_resum<CW>(S, L, cfull, prow);
    if (lane == 0) { out[pr] = finish(total); status[pr] = 0; }
    count();
}

template <int CW, int ORDER, int GROUND, class SRC>
__global__ void __launch_bounds__(64)
wasserstein_q_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                     const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                     const SRC src, int n_pairs, int max_rows, int max_cols,
                     double* __restrict__ out, int* __restrict__ status, const ws_opts opt)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    wq_solve<CW, ORDER, GROUND, SRC>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, pr, max_rows, max_cols, out, status,
                                     opt, smem);
}

// ---------------------------------------------------------------------------------
// One launch, sized by the capacities of the two diagram buffers (at most WQ_MAX_POINTS points each: a buffer may be
// larger, a pair with more finite points than that is TDA_WIN_NOT_CONVERGED).
template <int ORDER, int GROUND, class SRC>
static tda_status launch_wq_src(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                                const int* cnt_b, int cap_b, const SRC& src, int n_pairs, double* out, int* status,
                                hipStream_t st)
{
    const int max_a = cap_a < WQ_MAX_POINTS ? cap_a : WQ_MAX_POINTS, max_b = cap_b < WQ_MAX_POINTS ? cap_b : WQ_MAX_POINTS;
    const int max_rows = max_a < max_b ? max_a : max_b, max_cols = max_a < max_b ? max_b : max_a;
    const ws_opts opt{ctx->ws_ctr, ctx->ws_prune};
    // assign_lds: rows b, d, s, u; columns b, d, t, owner (ints, padded to 8 B).  30.5 KB at 512 x 512.
    const size_t lds = (size_t)(4 * max_rows + 3 * max_cols + ((max_cols + 1) >> 1)) * 8;
    assign_with_cw(max_cols, [&](auto cw) -> tda_status {
        auto kern = wasserstein_q_kernel<decltype(cw)::value, ORDER, GROUND, SRC>;
        hipLaunchKernelGGL(kern, dim3(n_pairs), dim3(64), lds, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, n_pairs,
                           max_rows, max_cols, out, status, opt);
        return TDA_OK;
    });
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_wasserstein_q(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                                const int* cnt_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs, int order,
                                int ground, double* out, int* status, hipStream_t st)
{
    if ((order != 1 && order != 2) || (ground != TDA_GROUND_L2 && ground != TDA_GROUND_LINF))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "order must be 1 or 2 and ground TDA_GROUND_L2 or TDA_GROUND_LINF");
    if (n_pairs == 0) return TDA_OK;
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    const ws_index_pairs src{idx_a, idx_b};
#define WQ_VARIANT(O, G) launch_wq_src<O, G>(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, n_pairs, out, status, st)
    if (ground == TDA_GROUND_L2) return order == 1 ? WQ_VARIANT(1, TDA_GROUND_L2) : WQ_VARIANT(2, TDA_GROUND_L2);
    return order == 1 ? WQ_VARIANT(1, TDA_GROUND_LINF) : WQ_VARIANT(2, TDA_GROUND_LINF);
#undef WQ_VARIANT
}
