// wasserstein.hip -- batched order-1 Wasserstein distance between persistence diagrams.
//
// Replaces safe_wasserstein (scripts/utils.py:180-191) -> persim.wasserstein(dgm1, dgm2):
// Euclidean ground metric (sklearn's |x|^2 - 2x.y + |y|^2 expansion, float64), every point
// may instead go to the diagonal at cost (d-b)cos(pi/4)-ish (persim's 45-degree rotation),
// result = plain sum of matched costs.
//
// persim solves one (M+N)x(M+N) assignment with +inf blocks.  The same optimum is the
// min over PARTIAL matchings mu of  sum_mu C_ij + sum_{i not in mu} s_i + sum_{j not in mu} t_j
//   =  sum s + sum t + min_mu sum_mu (C_ij - s_i - t_j),
// i.e. a rectangular assignment (rows = the smaller diagram) with costs
// g_ij = min(0, C_ij - s_i - t_j) <= 0 and no forbidden entries.  It is solved EXACTLY in
// float64 by shortest augmenting paths with dual variables (Jonker-Volgenant class), one
// pair per wavefront: columns live on lanes (CW per lane), one Dijkstra step = CW LDS reads
// per lane + one wave min-reduction.  At most R(R+1)/2 steps for R rows.
// The returned value re-sums the ORIGINAL costs (C_ij, s_i, t_j) of the optimal matching.
// The pair prologue, the solver and the re-summation are assign_dev.h's, shared with wasserstein_q.hip; this file
// keeps what is order 1's own: the cost, the pruning margin and tests, the equal-birth wavefront, the pair sources
// other than index arrays, the matrix kernels and the two-launch scheme.
// Which pair a wavefront solves is a template parameter of the kernel: explicit index arrays (tda_wasserstein_batch)
// or group tables read on the device (tda_wasserstein_cross_dev: scripts/matched_vs_mismatched.py:86-95).
#include "assign_dev.h"

#ifdef TDA_PROFILE
__device__ unsigned long long g_prof_ws[16];
extern "C" __attribute__((visibility("default"))) int tda_profile_read_ws(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof_ws), sizeof(unsigned long long) * 16) != hipSuccess) return 1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof_ws), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}
#define WPROF(i, v) do { if (lane_id() == 0) atomicAdd(&g_prof_ws[i], (unsigned long long)(v)); } while (0)
#define WCLK() clock64()
#else
#define WPROF(i, v) do {} while (0)
#define WCLK() 0ull
#endif

#define WS_DEFERRED 0x40000000      // status of a pair between the small and the wide launch (never seen by the caller)
#define WS_CP 0.7071067811865476   // np.cos(np.pi/4)
#define WS_SP 0.7071067811865475   // np.sin(np.pi/4)

// C(a_i, b_j) with a from the FIRST diagram and b from the SECOND, independent of which one
// plays the row role (mirrors oracle/tda_oracle.c::orc_wasserstein)
__device__ __forceinline__ double ws_cost(double ab, double ad, double bb, double bd)
{
    const double xx = ab * ab + ad * ad;
    const double yy = bb * bb + bd * bd;
    const double dot = fma(ad, bd, ab * bb);
    double d2 = -2.0 * dot;
    d2 += xx;
    d2 += yy;
    if (!(d2 > 0.0)) d2 = 0.0;
    return sqrt_rn(d2);                         // (sqrt() bit for bit, six instructions less: common.h)
}

// ---- the margin of the pruning tests ----
// ws_solve leaves out cells whose gain g = min(0, C - s - t) is known to be 0.  What has to be 0 is the COMPUTED
// gain, (ws_cost() - s_c) - t_c in floating point; that holds whenever ws_cost() >= s_c + t_c as reals (rounding is
// monotone and t_c is a float64: fl(C_c - s_c) >= t_c, so the second difference is >= 0).  The tests prove
// L > s + t + m for a lower bound L on the true distance C; m has to cover what separates that from the computed
// quantities.  With X = the largest |coordinate| of the pair and u = 2^-53:
//   d2:  five products and five sums, each with relative error u, of terms that add up to at most
//        |x|^2 + |y|^2 + 2|x.y| <= 2 (|x|^2 + |y|^2) <= 8 X^2: |d2_c - d2| <= 6u * 8 X^2 = E, and since
//        sqrt(max(0, L^2 - E)) >= L - sqrt(E), the cancellation costs at most sqrt(48 u) X = 7.3e-8 X;
//   sqrt_rn, s_c = fma(d, cos, -(b sin)), t_c, and the tests' own few operations: relative errors of a few u on
//        values <= 3 X, below 1e-14 X together;
//   underflow: an absolute 2^-1075 per product, 2^-1072 in d2, 2^-536 = 4.4e-162 after the square root.
// m = 1e-6 X + 1e-150 is more than ten times the sum.  It moves the cut by a millionth of the coordinates' scale.
// Pairs with X >= 1e150 are not pruned: their squares overflow and ws_cost() clamps NaNs to 0.
#define WS_PRUNE_REL 1e-6
#define WS_PRUNE_ABS 1e-150
#define WS_PRUNE_MAX 1e150

// Where workgroup pr finds its pair: the kernel's compile-time switch (one solver, three sources).
// ws_index_pairs (assign_dev.h): explicit index arrays, every workgroup has a pair.
// ws_table_pairs: grouped diagrams paired by position (mvm:89-93).  A diagram pr, at position i of its group g =
// grp_a[pr], is paired with B diagram seg_off_b[p] + i of the group p = partner_seg[g] -- if g has a partner, the
// partner's group is that long, and that B diagram is a diagram at all (mvm:60 leaves out clouds with < 3 points).
// Every table is indexed from blockIdx.x alone: the reads are wave-uniform (scalar loads).  Indices that leave the
// tables mean "no pair", never a read out of bounds.
struct ws_table_pairs {
    const int* grp_a; const int* seg_off_a; const int* seg_off_b; const int* partner_seg; const int* status_b;
    int n_seg_a, n_seg_b, n_b;
    __device__ __forceinline__ bool resolve(int pr, int& ia, int& ib) const
    {
        ia = pr;
        const int g = grp_a[pr];
        if (g < 0 || g >= n_seg_a) return false;
        const int p = partner_seg[g];
        if (p < 0 || p >= n_seg_b) return false;
        const int i = pr - seg_off_a[g];
        const int b0 = seg_off_b[p];
        if (i < 0 || i >= seg_off_b[p + 1] - b0) return false;
        ib = b0 + i;
        if (ib < 0 || ib >= n_b) return false;
        return !(status_b[ib] & TDA_WIN_DEGENERATE);
    }
};

// ws_matrix_pairs: the pairs of ONE entry (A group g, candidate column c) of tda_wasserstein_matrix_dev; pr is the
// position within the group.  The kernel has resolved the two groups (a0: first A diagram of g, b0 / len_b: the B group
// of (class of g, column c)) and made sure that a0 + pr stays inside the A table for every position it asks for.
struct ws_matrix_pairs {
    const int* status_b; int a0, b0, len_b, n_b;
    __device__ __forceinline__ bool resolve(int pr, int& ia, int& ib) const
    {
        ia = a0 + pr;
        if (pr >= len_b) return false;
        ib = b0 + pr;
        if (ib < 0 || ib >= n_b) return false;
        return !(status_b[ib] & TDA_WIN_DEGENERATE);
    }
};

// pair pr, by the one wave of the workgroup
template <int CW, class SRC>
__device__ __forceinline__ void ws_solve(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                                         const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                                         const SRC& src, int pr, int max_rows, int max_cols,
                                         double* __restrict__ out, int* __restrict__ status, int mode, int* list,
                                         const ws_opts& opt, unsigned char* smem)
{
    const int lane = lane_id();
    unsigned long long wt0 = WCLK();
    (void)wt0;
    // LDS: the solver's arrays (assign_dev.h) | |y|^2 of the columns (1-D path)
    const assign_lds L(smem, max_rows, max_cols);
    double* const rb = L.rb; double* const rd = L.rd; double* const rs = L.rs;
    double* const cb = L.cb; double* const cd = L.cd; double* const ct = L.ct;
    double* G = L.end();                                                // max_cols doubles

    int ia, ib;
    if (!src.resolve(pr, ia, ib)) {                                     // no pair: leave before the solver
        if (lane == 0) { out[pr] = __longlong_as_double(0x7ff8000000000000ll); status[pr] = TDA_WIN_NO_PAIR; }
        return;
    }
    assign_shape S;
    auto diag = [](double b, double d) -> double { return fma(d, WS_CP, -(b * WS_SP)); };
    if (!assign_load_pair<CW>(dgm_a, cnt_a, cap_a, ia, dgm_b, cnt_b, cap_b, ib, L, diag, S)) {
        if (lane == 0) {                                                // does not fit this launch
            if (mode == 1) {
                status[pr] = WS_DEFERRED;
                if (list) list[4 + atomicAdd(&list[0], 1)] = pr;        // (one wave and one pair per workgroup: nothing to aggregate)
            }
            else { out[pr] = __longlong_as_double(0x7ff8000000000000ll); status[pr] = TDA_WIN_NOT_CONVERGED; }
        }
        return;
    }
    const bool a_is_row = S.a_is_row;
    const int R = S.R, Cn = S.Cn;

    auto cfull = [&](int i, int j) -> double {   // original point-to-point cost of row i, col j
        return a_is_row ? ws_cost(rb[i], rd[i], cb[j], cd[j]) : ws_cost(cb[j], cd[j], rb[i], rd[i]);
    };
    auto gain = [&](int i, int j) -> double {
        const double g = cfull(i, j) - rs[i] - ct[j];
        return g < 0.0 ? g : 0.0;
    };
    WPROF(0, WCLK() - wt0); wt0 = WCLK();
    WPROF(4, 1); WPROF(5, R); WPROF(6, Cn);
    unsigned long long n_cut = 0, n_trim = 0;           // for opt.ctr
    auto count = [&]() {
        if (opt.ctr && lane == 0) {
            if (n_cut) atomicAdd(&opt.ctr[0], n_cut);
            if (n_trim) atomicAdd(&opt.ctr[1], n_trim);
            atomicAdd(&opt.ctr[2], 1ull);
        }
    };

    // ---- 1-D fast path ------------------------------------------------------------------
    // If every point of both diagrams has the same birth (two H0 diagrams: births 0) the points lie
    // on a line, the ground cost is |d_i - d_j| and, for any fixed sets of matched points, the sorted
    // (non-crossing) pairing is optimal.  The optimum over partial matchings is then the edit-distance
    // style recurrence  F[i][j] = min(F[i-1][j], F[i][j-1], F[i-1][j-1] + g_ij)  over death-sorted
    // diagrams - an anti-diagonal wavefront with one row per lane, R + C - 1 steps instead of
    // hundreds of Dijkstra steps.  Same gains g_ij as the general solver (so the same rounding of
    // C_ij); the value differs from the assignment optimum by at most the rounding noise of C.
    {
        const double b0 = rb[0];
        if (assign_on_sorted_line(S, L)) {
            // ---- live ranges ----
            // With p = d - b0 the persistence of a row and q of a column, the true gain of a cell is at least
            // max(p (1-c) - q (1+c), q (1-c) - p (1+c)), c = 1/sqrt 2 (|p - q| >= either difference): a column is dead
            // for EVERY row if q (1+c) + m <= p_min (1-c) or q (1-c) >= p_max (1+c) + m, m the margin above.  Both tests
            // are monotone in q and the deaths are sorted, so the dead columns are a prefix and a suffix, counted by
            // ballots; then the same for the rows against the live columns.  F is 0 over a dead prefix and constant
            // over a dead suffix, so the wavefront over the live ranges, zero boundary included, does what the full one
            // does in every live cell: same operands, same order, same bits.
            int ilo = 0, jlo = 0, Rl = R, Cl = Cn;
            const double c1p = 1.0 + WS_CP, c1m = 1.0 - WS_CP;
            double mx = WS_PRUNE_MAX;
            if (opt.prune)
                mx = fmax(fabs(b0), fmax(fmax(fabs(rd[0]), fabs(rd[R - 1])), fmax(fabs(cd[0]), fabs(cd[Cn - 1]))));
            if (mx < WS_PRUNE_MAX) {
                const double p_min = rd[0] - b0, p_max = rd[R - 1] - b0;
                const double m = WS_PRUNE_REL * mx + WS_PRUNE_ABS;
                const double lo_c = p_min * c1m - m, hi_c = p_max * c1p + m;
                int n_lo = 0, n_hi = 0;
                for (int j0 = 0; j0 < Cn; j0 += 64) {
                    const int j = j0 + lane;
                    const double q = cd[j < Cn ? j : Cn - 1] - b0;
                    n_lo += __popcll(__ballot(j < Cn && q * c1p <= lo_c));
                    n_hi += __popcll(__ballot(j < Cn && q * c1m >= hi_c));
                }
                jlo = n_lo;
                const int jhi = Cn - n_hi > jlo ? Cn - n_hi : jlo;
                Cl = jhi - jlo;
                Rl = 0;
                if (Cl > 0) {
                    const double q_min = cd[jlo] - b0, q_max = cd[jhi - 1] - b0;
                    const double lo_r = q_min * c1m - m, hi_r = q_max * c1p + m;
                    const double p = rd[lane < R ? lane : R - 1] - b0;
                    ilo = __popcll(__ballot(lane < R && p * c1p <= lo_r));
                    const int ihi = R - __popcll(__ballot(lane < R && p * c1m >= hi_r));
                    Rl = ihi > ilo ? ihi - ilo : 0;
                }
                n_trim = (unsigned long long)((R - Rl) + (Cn - Cl));
            }
            WPROF(8, 1); WPROF(9, Rl); WPROF(10, Cl);
            double cur = 0.0, nb1 = 0.0, nb2 = 0.0;      // own F, neighbour row's F one / two steps ago
            const int nsteps1d = (Rl > 0 && Cl > 0) ? Rl + Cl - 1 : 0;      // an empty live range: no wavefront, fbest = 0
            // gains on the fly: the row's part of sklearn's expansion is a per-lane constant, the column's |y|^2 is
            // tabulated once -- the same operations in the same order as ws_cost(), 40 instead of 58 instructions per cell
            for (int j = lane; j < Cn; j += 64) G[j] = cb[j] * cb[j] + cd[j] * cd[j];
            __syncthreads();
            const int li = lane < Rl ? ilo + lane : 0;                      // lane = live row index
            const double r_b = rb[li], r_d = rd[li], r_s = rs[li], r_n = r_b * r_b + r_d * r_d;
            // every birth equals b0: r_b * c_b is one constant; which diagram comes first in the sums is uniform per pair,
            // so the wavefront exists twice instead of selecting per cell (34 -> 29 instructions per cell)
            const double bb = b0 * b0;
            auto wavefront = [&](auto AROW) {
                constexpr bool A_ROW = decltype(AROW)::value;
                for (int t = 0; t < nsteps1d; ++t) {
                    const int j0 = t - lane;
                    // neighbour (row lane-1) value of the previous step; row 0 sees the zero boundary
                    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(cur), 0x138, 0xF, 0xF, false);
                    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(cur), 0x138, 0xF, 0xF, false);
                    nb2 = nb1;
                    nb1 = __hiloint2double(hi, lo);
                    if (lane < Rl && j0 >= 0 && j0 < Cl) {
                        const double c_d = cd[jlo + j0], c_n = G[jlo + j0];
                        const double dot = fma(r_d, c_d, bb);                   // = fma(ad, bd, ab * bb) either way round
                        double d2 = -2.0 * dot;
                        d2 += A_ROW ? r_n : c_n;                                // |x|^2 of the FIRST diagram's point, then the second's
                        d2 += A_ROW ? c_n : r_n;
                        if (!(d2 > 0.0)) d2 = 0.0;
                        double g = sqrt_rn(d2) - r_s - ct[jlo + j0];
                        g = g < 0.0 ? g : 0.0;
                        const double up = nb1;                          // F[row][j0+1] of the row above
                        const double dg = (j0 == 0 ? 0.0 : nb2) + g;    // F[row above][j0] + g
                        double m = up < cur ? up : cur;                 // cur still holds F[row+1][j0] (left)
                        m = dg < m ? dg : m;
                        cur = m;
                    }
                }
            };
            if (a_is_row) wavefront(std::true_type{}); else wavefront(std::false_type{});
            const double fbest = nsteps1d ? uni_f64(cur, Rl - 1) : 0.0;
            double part = 0.0;
            for (int i = lane; i < R; i += 64) part += rs[i];
            for (int j = lane; j < Cn; j += 64) part += ct[j];
            const double total1d = wave_sum_f64(part) + fbest;
            if (lane == 0) { out[pr] = total1d; status[pr] = 0; }
            count();
            return;
        }
    }

    // ---- every cell dead? ---------------------------------------------------------------
    // If every point is nearer to the diagonal than to any point of the other diagram (by the margin above), every
    // gain clamps to 0: the row reduction finds u = 0, nothing is augmented, and the final summation adds every s and
    // every t in its usual order.  Then that summation alone gives the same bits.  The test: the distance between the
    // two bounding boxes against s_max + t_max (one compare), else each row's distance to the box of the columns
    // against s_i + t_max.  A pair with a live cell runs the solver unchanged: compacting a partly live problem could
    // break ties differently.
    bool all_dead = false;
    if (opt.prune) {
        const auto [rb_lo, rb_hi, rd_lo, rd_hi, s_hi, cb_lo, cb_hi, cd_lo, cd_hi, t_hi] = assign_box_stats(S, L);
        const double mx = fmax(fmax(fmax(fabs(rb_lo), fabs(rb_hi)), fmax(fabs(rd_lo), fabs(rd_hi))),
                               fmax(fmax(fabs(cb_lo), fabs(cb_hi)), fmax(fabs(cd_lo), fabs(cd_hi))));
        if (mx < WS_PRUNE_MAX) {
            const double m = WS_PRUNE_REL * mx + WS_PRUNE_ABS;
            const double gx = fmax(0.0, fmax(cb_lo - rb_hi, rb_lo - cb_hi));
            const double gy = fmax(0.0, fmax(cd_lo - rd_hi, rd_lo - cd_hi));
            all_dead = sqrt_rn(gx * gx + gy * gy) > s_hi + t_hi + m;
            if (!all_dead) {
                bool live = false;
                for (int i0 = 0; i0 < R; i0 += 64) {
                    const int i = i0 + lane < R ? i0 + lane : R - 1;
                    const double dx = fmax(0.0, fmax(cb_lo - rb[i], rb[i] - cb_hi));
                    const double dy = fmax(0.0, fmax(cd_lo - rd[i], rd[i] - cd_hi));
                    live = live || __ballot(!(sqrt_rn(dx * dx + dy * dy) > rs[i] + t_hi + m)) != 0ull;
                }
                all_dead = !live;
            }
        }
        if (all_dead) n_cut = 1;
    }
    WPROF(7, all_dead ? 1 : 0);

    int prow[CW], nsteps = 0;
    if (!assign_solve<CW>(S, L, gain, all_dead, prow, nsteps)) {
        if (lane == 0) { out[pr] = __longlong_as_double(0x7ff8000000000000ll); status[pr] = TDA_WIN_NOT_CONVERGED; }
        count();
        return;
    }
    WPROF(1, WCLK() - wt0); wt0 = WCLK();
    WPROF(3, nsteps);
    // total = sum over real matches of C_ij + unmatched rows' s + unmatched cols' t
    const double total = assign_resum<CW>(S, L, cfull, prow);
    if (lane == 0) { out[pr] = total; status[pr] = 0; }
    count();
    WPROF(2, WCLK() - wt0);
}

template <int CW, class SRC>
__global__ void __launch_bounds__(64)
wasserstein_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                   const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                   const SRC src, int n_pairs,
                   int max_rows, int max_cols,
                   double* __restrict__ out, int* __restrict__ status, int mode, int* list, const ws_opts opt)
{
    // mode 1: the SMALL first launch (LDS for 64 x 64 points whatever the capacities of the diagram buffers: four times
    // the workgroups per CU of a launch sized by a capacity of 256) leaves pairs that do not fit marked WS_DEFERRED and,
    // given a list, appends them to it; mode 2: the launch sized by the capacities takes exactly the marked ones
    // (TDA_SCHEME_GRID; under TDA_SCHEME_LISTS wasserstein_list_kernel takes the listed ones); mode 0: one launch for
    // everything
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    if (mode == 2 && status[pr] != WS_DEFERRED) return;
    ws_solve<CW, SRC>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, pr, max_rows, max_cols, out, status, mode, list, opt, smem);
}

// The pairs on the list of the small launch, on a grid that does not depend on the batch: workgroup b takes entries b,
// b + gridDim.x, ...  [0] = entries, [1] = workgroups done (the last one through clears both: no memset node between a
// step and the next), the pairs from [4] on.  A pair that does not fit here either is TDA_WIN_NOT_CONVERGED, as in mode 2.
template <int CW, class SRC>
__global__ void __launch_bounds__(64)
wasserstein_list_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                        const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                        const SRC src, int n_pairs,
                        int max_rows, int max_cols,
                        double* __restrict__ out, int* __restrict__ status, int* list, const ws_opts opt)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int nl = uni(list[0]);
    nl = nl < n_pairs ? nl : n_pairs;
    for (int j = blockIdx.x; j < nl; j += gridDim.x) {
        const int pr = uni(list[4 + j]);
        if (pr >= 0 && pr < n_pairs)
            ws_solve<CW, SRC>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, pr, max_rows, max_cols, out, status, 0, nullptr, opt, smem);
        __syncthreads();
    }
    if (threadIdx.x == 0 && atomicAdd(&list[1], 1) == (int)gridDim.x - 1) { list[0] = 0; list[1] = 0; }
}

// ---------------------------------------------------------------------------------
// the two-launch scheme, whatever the source of the pairs
template <class SRC>
static tda_status launch_wasserstein_src(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                                         const int* cnt_b, int cap_b, const SRC& src, int n_pairs, double* out, int* status,
                                         hipStream_t st)
{
    if (n_pairs == 0) return TDA_OK;
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    const int lo = cap_a < cap_b ? cap_a : cap_b, hi = cap_a < cap_b ? cap_b : cap_a;
    const int max_rows = lo, max_cols = hi;
    const ws_opts opt{ctx->ws_ctr, ctx->ws_prune};
    if (max_cols > 512) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "diagrams with more than 512 rows are not supported");
    // No cost matrix in LDS: gains are evaluated where they are needed.  A per-pair matrix (16 KB for a 45 x 45 H1
    // pair) left room for 5-7 one-wave workgroups per CU; without it the H0 pairs of a pass take 1.7 instead of 2.9 ms
    // and the H1 pairs 0.73 instead of 1.17 ms (latency-bound solver: residency matters more than the re-evaluation).
    const size_t lds = (size_t)(4 * max_rows + 4 * max_cols + ((max_cols + 1) >> 1)) * 8;
    // diagram buffers with room for more than 128 rows (H1: 256) are mostly far from full (35 x 41 rows on the bench's
    // windows): a first launch with LDS for 64 x 64 points, the launch sized by the capacities for the pairs it defers
    // (TDA_SCHEME_LISTS: the second launch runs over the list of the deferred pairs, TDA_SCHEME_GRID: over the whole batch)
    static const bool one_launch = getenv("TDA_WS_ONE_LAUNCH") != nullptr;
    const int scheme = one_launch ? TDA_SCHEME_ONE : ctx->launch_scheme;
    const int mode = (scheme != TDA_SCHEME_ONE && max_cols > 128) ? 2 : 0;
    int* list = nullptr;
    if (mode && scheme == TDA_SCHEME_LISTS) {
        int slot = -1;
        const tda_status rc = stream_lists_take(ctx, n_pairs, st, &slot);
        if (rc != TDA_OK) return rc;
        if (slot >= 0) list = ctx->ws_list[slot];        // (else: no list of that size, the launch over the batch)
    }
    if (mode) {
        const int sr = max_rows < 64 ? max_rows : 64;
        const size_t lds_s = (size_t)(4 * sr + 4 * 64 + 32) * 8;
        hipLaunchKernelGGL((wasserstein_kernel<1, SRC>), dim3(n_pairs), dim3(64), lds_s, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b,
                           cap_b, src, n_pairs, sr, 64, out, status, 1, list, opt);
    }
    const tda_status rc = assign_with_cw(max_cols, [&](auto cw) -> tda_status {
        constexpr int CWV = decltype(cw)::value;
        auto kern = wasserstein_kernel<CWV, SRC>;
        auto lkern = wasserstein_list_kernel<CWV, SRC>;
        if (lds > 48 * 1024)
            TDA_HIP(ctx, hipFuncSetAttribute(list ? reinterpret_cast<const void*>(lkern) : reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (list)
            hipLaunchKernelGGL(lkern, dim3(n_pairs < 256 ? n_pairs : 256), dim3(64), lds, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b,
                               cap_b, src, n_pairs, max_rows, max_cols, out, status, list, opt);
        else
            hipLaunchKernelGGL(kern, dim3(n_pairs), dim3(64), lds, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, n_pairs,
                               max_rows, max_cols, out, status, mode, (int*)nullptr, opt);
        return TDA_OK;
    });
    if (rc != TDA_OK) return rc;
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_wasserstein(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, const double* dgm_b,
                              const int* cnt_b, int cap_b, const int* idx_a, const int* idx_b, int n_pairs,
                              double* out, int* status, hipStream_t st)
{
    return launch_wasserstein_src(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, ws_index_pairs{idx_a, idx_b}, n_pairs, out,
                                  status, st);
}

// one workgroup per A diagram; the pairs come from the group tables (ws_table_pairs)
tda_status launch_wasserstein_cross(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                    const int* grp_a, const int* seg_off_a, int n_seg_a, const double* dgm_b,
                                    const int* cnt_b, int cap_b, int n_b, const int* seg_off_b, int n_seg_b,
                                    const int* status_b, const int* partner_seg, double* out, int* status, hipStream_t st)
{
    const ws_table_pairs src{grp_a, seg_off_a, seg_off_b, partner_seg, status_b, n_seg_a, n_seg_b, n_b};
    return launch_wasserstein_src(ctx, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, n_a, out, status, st);
}

// ---------------------------------------------------------------------------------
// The match-mismatch matrix (tda_wasserstein_matrix_dev): entry (g, c) = the row tda_wasserstein_cross_dev +
// tda_cross_rows_dev give A group g against the B group of (class of g, column c) -- mean distance, pair count, flags --
// without a per-pair array in HBM.
// One workgroup of ONE wave per entry.  The wave takes the positions of the group one after the other through ws_solve
// -- the solver as it is: its pair source is ws_matrix_pairs, and its `out` / `status` are the entry's result slots in
// LDS, behind the solver's own region -- then lane 0 reduces the slots with cross_rows_kernel's arithmetic and writes
// the entry's three words.  One wave, not four taking the positions in turn: ws_solve synchronises with workgroup
// barriers that its early exits leave out, which is sound for one wave only; a launch has n_seg_a * n_col entries (1.7
// million for a shard of the corpus), so the machine is full either way; a wave needs its own 4.3 KB of solver LDS in
// both designs; and four-wave workgroups would idle three waves on the short groups.  (Not measured against the
// four-wave form.)
// The two-launch scheme is the pairs': the first launch has LDS for 64 x 64 points; an entry with a pair that does not
// fit is put on the stream's list (TDA_SCHEME_LISTS, relative to the chunk of entries of the launch) or marked
// WS_DEFERRED in flags (TDA_SCHEME_GRID) and redone as a whole by the launch sized by the capacities.
// ---------------------------------------------------------------------------------
#define WS_MATRIX_MAX_GROUP 64          // A diagrams per group: 768 B of result slots, 5,120 B of LDS per wave in the first launch
struct ws_matrix_args {
    const int* seg_off_a; const int* cls_a; const int* seg_off_b; const int* status_b;
    int n_a, n_b, n_cls, n_col;
    double* out; int* pairs; int* flags;
};

// numpy's sum of n <= 128 terms: eight interleaved accumulators (np_pairwise_leaf of features.hip, restated -- a header
// shared with features.hip moved instructions in that file's kernels)
template <class F>
__device__ __forceinline__ double ws_np_sum(const F& f, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += f(i);
        return res;
    }
    double r0 = f(0), r1 = f(1), r2 = f(2), r3 = f(3), r4 = f(4), r5 = f(5), r6 = f(6), r7 = f(7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += f(i + 0); r1 += f(i + 1); r2 += f(i + 2); r3 += f(i + 3);
        r4 += f(i + 4); r5 += f(i + 5); r6 += f(i + 6); r7 += f(i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += f(i);
    return res;
}

// smem: the solver's region (solver_bytes), then the slots
template <int CW>
__device__ __forceinline__ void ws_matrix_entry(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                                                const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                                                const ws_matrix_args& M, size_t e, int e_rel, int max_rows, int max_cols,
                                                int solver_bytes, int mode, int* list, const ws_opts& opt,
                                                unsigned char* smem)
{
    const int lane = lane_id();
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int g = (int)(e / (size_t)M.n_col), c = (int)(e % (size_t)M.n_col);
    // the two groups; indices that leave a table: no pair
    const int a0 = uni(M.seg_off_a[g]), a1 = uni(M.seg_off_a[g + 1]);
    const int len = (a0 >= 0 && a1 >= a0 && a1 <= M.n_a) ? a1 - a0 : 0;
    const int k = uni(M.cls_a[g]);
    int b0 = 0, len_b = 0;
    if (k >= 0 && k < M.n_cls) {
        const size_t p = (size_t)k * M.n_col + c;
        b0 = uni(M.seg_off_b[p]);
        len_b = uni(M.seg_off_b[p + 1]) - b0;
    }
    if (len > WS_MATRIX_MAX_GROUP) {
        if (lane == 0) { M.out[e] = qnan; M.pairs[e] = 0; M.flags[e] = TDA_WIN_TOO_LARGE; }
        return;
    }
    double* xs = reinterpret_cast<double*>(smem + solver_bytes);
    int* ss = reinterpret_cast<int*>(xs + WS_MATRIX_MAX_GROUP);
    const ws_matrix_pairs src{M.status_b, a0, b0, len_b, M.n_b};
    const int n_try = len < len_b ? len : len_b;
    if (lane >= n_try && lane < len) { xs[lane] = qnan; ss[lane] = TDA_WIN_NO_PAIR; }      // positions past the B group
    bool deferred = false;
    for (int i = 0; i < n_try && !deferred; ++i) {
        ws_solve<CW>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, src, i, max_rows, max_cols, xs, ss, mode ? 1 : 0, nullptr, opt, smem);
        __syncthreads();
        deferred = mode && uni(ss[i]) == WS_DEFERRED;
    }
    if (deferred) {                                                      // the whole entry again, in the wide launch
        if (lane == 0) {
            if (list) list[4 + atomicAdd(&list[0], 1)] = e_rel;
            else M.flags[e] = WS_DEFERRED;
        }
        return;
    }
    __syncthreads();
    if (lane == 0) {                                                     // cross_rows_kernel's arithmetic
        int n = 0, cnt = 0, fl = 0;
        for (int i = 0; i < len; ++i) n += (ss[i] & TDA_WIN_NO_PAIR) ? 0 : 1;
        for (int i = 0; i < n; ++i) {
            cnt += (ss[i] == 0 && xs[i] == xs[i]) ? 1 : 0;
            fl |= ss[i];
        }
        auto val = [=](int j) { const double v = xs[j]; return (ss[j] == 0 && v == v) ? v : 0.0; };
        const double sum = ws_np_sum(val, n);                             // (n <= 64: numpy's tree is its leaf)
        M.out[e] = cnt > 0 ? sum / (double)cnt : qnan;
        M.pairs[e] = n;
        M.flags[e] = fl & ~(TDA_WIN_NO_PAIR | TDA_WIN_DEGENERATE);
    }
}

// modes as wasserstein_kernel's: 1 = small first launch, 2 = the marked entries with the layout of the capacities,
// 0 = one launch for everything.  Entries e0 .. e0 + n_e - 1.
template <int CW>
__global__ void __launch_bounds__(64)
wasserstein_matrix_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                          const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                          const ws_matrix_args M, size_t e0, int n_e, int max_rows, int max_cols, int solver_bytes, int mode,
                          int* list, const ws_opts opt)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if ((int)blockIdx.x >= n_e) return;
    const size_t e = e0 + blockIdx.x;
    if (mode == 2 && M.flags[e] != WS_DEFERRED) return;
    ws_matrix_entry<CW>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, M, e, (int)blockIdx.x, max_rows, max_cols, solver_bytes,
                        mode == 1, list, opt, smem);
}

// the entries on the list of the small launch (the layout and the clearing of wasserstein_list_kernel's)
template <int CW>
__global__ void __launch_bounds__(64)
wasserstein_matrix_list_kernel(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                               const double* __restrict__ dgm_b, const int* __restrict__ cnt_b, int cap_b,
                               const ws_matrix_args M, size_t e0, int n_e, int max_rows, int max_cols, int solver_bytes,
                               int* list, const ws_opts opt)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int nl = uni(list[0]);
    nl = nl < n_e ? nl : n_e;
    for (int j = blockIdx.x; j < nl; j += gridDim.x) {
        const int r = uni(list[4 + j]);
        if (r >= 0 && r < n_e)
            ws_matrix_entry<CW>(dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, M, e0 + (size_t)r, r, max_rows, max_cols, solver_bytes, 0,
                                nullptr, opt, smem);
        __syncthreads();
    }
    if (threadIdx.x == 0 && atomicAdd(&list[1], 1) == (int)gridDim.x - 1) { list[0] = 0; list[1] = 0; }
}

#define WS_MATRIX_CHUNK (1 << 16)        // entries per launch under TDA_SCHEME_LISTS: the capacity asked of the stream's list
#define WS_MATRIX_GRID_CHUNK (1 << 30)   // ... per launch otherwise (gridDim.x)
#define WS_MATRIX_LIST_GRID 2048         // workgroups over a list: a listed entry is up to 64 wide solves, and 2,048 one-wave
                                         // workgroups with the LDS of capacity 256 are what 256 CUs hold at once

tda_status launch_wasserstein_matrix(tda_ctx* ctx, const double* dgm_a, const int* cnt_a, int cap_a, int n_a,
                                     const int* seg_off_a, int n_seg_a, const int* cls_a, const double* dgm_b,
                                     const int* cnt_b, int cap_b, int n_b, const int* seg_off_b, int n_cls, int n_col,
                                     const int* status_b, double* out, int* pairs, int* flags, hipStream_t st)
{
    const size_t n_ent = (size_t)n_seg_a * (size_t)n_col;
    if (n_ent == 0) return TDA_OK;
    if (cap_a < 1 || cap_b < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    const int lo = cap_a < cap_b ? cap_a : cap_b, hi = cap_a < cap_b ? cap_b : cap_a;
    const int max_rows = lo, max_cols = hi;
    if (max_cols > 512) TDA_FAIL(ctx, TDA_ERR_UNSUPPORTED, "diagrams with more than 512 rows are not supported");
    const ws_matrix_args M{seg_off_a, cls_a, seg_off_b, status_b, n_a, n_b, n_cls, n_col, out, pairs, flags};
    const ws_opts opt{ctx->ws_ctr, ctx->ws_prune};
    // the solver's layouts (launch_wasserstein_src), each followed by the result slots of the entry
    const size_t lds_res = (size_t)WS_MATRIX_MAX_GROUP * 12;
    const int lds_solver = (4 * max_rows + 4 * max_cols + ((max_cols + 1) >> 1)) * 8;
    const size_t lds_w = lds_solver + lds_res;
    const int sr = max_rows < 64 ? max_rows : 64;
    const int lds_solver_s = (4 * sr + 4 * 64 + 32) * 8;
    const size_t lds_s = lds_solver_s + lds_res;
    static const bool one_launch = getenv("TDA_WS_ONE_LAUNCH") != nullptr;
    const int scheme = one_launch ? TDA_SCHEME_ONE : ctx->launch_scheme;
    const int mode = (scheme != TDA_SCHEME_ONE && max_cols > 128) ? 2 : 0;
    int* list = nullptr;
    if (mode && scheme == TDA_SCHEME_LISTS) {
        int slot = -1;
        const tda_status rc = stream_lists_take(ctx, (int)(n_ent < WS_MATRIX_CHUNK ? n_ent : WS_MATRIX_CHUNK), st, &slot);
        if (rc != TDA_OK) return rc;
        if (slot >= 0) list = ctx->ws_list[slot];        // (else: no list of that size, the launch over the batch)
    }
    const size_t chunk = list ? WS_MATRIX_CHUNK : WS_MATRIX_GRID_CHUNK;
    for (size_t e0 = 0; e0 < n_ent; e0 += chunk) {
        const int n_e = (int)(n_ent - e0 < chunk ? n_ent - e0 : chunk);
        if (mode)
            hipLaunchKernelGGL(wasserstein_matrix_kernel<1>, dim3(n_e), dim3(64), lds_s, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b,
                               cap_b, M, e0, n_e, sr, 64, lds_solver_s, 1, list, opt);
        const tda_status rc = assign_with_cw(max_cols, [&](auto cw) -> tda_status {
            constexpr int CWV = decltype(cw)::value;
            auto kern = wasserstein_matrix_kernel<CWV>;
            auto lkern = wasserstein_matrix_list_kernel<CWV>;
            if (lds_w > 48 * 1024)
                TDA_HIP(ctx, hipFuncSetAttribute(list ? reinterpret_cast<const void*>(lkern) : reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w));
            if (list)
                hipLaunchKernelGGL(lkern, dim3(n_e < WS_MATRIX_LIST_GRID ? n_e : WS_MATRIX_LIST_GRID), dim3(64), lds_w, st, dgm_a,
                                   cnt_a, cap_a, dgm_b, cnt_b, cap_b, M, e0, n_e, max_rows, max_cols, lds_solver, list, opt);
            else
                hipLaunchKernelGGL(kern, dim3(n_e), dim3(64), lds_w, st, dgm_a, cnt_a, cap_a, dgm_b, cnt_b, cap_b, M, e0, n_e,
                                   max_rows, max_cols, lds_solver, mode, (int*)nullptr, opt);
            return TDA_OK;
        });
        if (rc != TDA_OK) return rc;
    }
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
