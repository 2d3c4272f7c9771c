// assign_dev.h -- what the Wasserstein kernels of every order share (wasserstein.hip: order 1 with sklearn's expansion
// of the Euclidean cost; wasserstein_q.hip: orders 1 and 2 from direct differences, L2 or L-infinity): the pair
// prologue, the rectangular assignment solver and the re-summation of the matching it leaves.
//
// The problem, for either file: rows = the smaller diagram, gains g_ij = min(0, C_ij - s_i - t_j) <= 0 with s, t the
// diagonal costs, no forbidden entries.  Points and diagonal costs lie in LDS and there is no cost matrix: each file
// hands in `gain(i, j)` and `cfull(i, j)` as callables that evaluate a cell where it is needed.  One pair per
// wavefront; the duals and the column state live in registers across the lanes, CW column slots per lane.
//
// Loop bounds, all known before the loop starts: rows to augment <= R; Dijkstra steps per row <= C + 2; path flips
// <= C + 2.  A bound that is hit makes assign_solve() return false (the callers: NaN and TDA_WIN_NOT_CONVERGED).
//
// Not here: the cost functions, the pruning margins and tests, the equal-birth wavefronts, the pair sources other than
// the index arrays, the launch schemes.  (bottleneck.hip takes ws_index_pairs from here and nothing else: its LDS layout
// is interleaved and its loader its own.)
#pragma once
#include "common.h"
#include <type_traits>

// Where workgroup pr finds its pair: explicit index arrays (NULL = identity), every workgroup has a pair.  Two pointers,
// laid out as the two kernel arguments they replace.
struct ws_index_pairs {
    const int* idx_a; const int* idx_b;
    __device__ __forceinline__ bool resolve(int pr, int& ia, int& ib) const
    {
        ia = idx_a ? idx_a[pr] : pr;
        ib = idx_b ? idx_b[pr] : pr;
        return true;
    }
};

// What tda_set_wasserstein_pruning / tda_set_wasserstein_counter hand to the kernels.
struct ws_opts {
    unsigned long long* ctr;    // NULL, or device u64[3]: short cuts, rows + columns trimmed, pairs that had a pair to
                                // solve (those that end with TDA_WIN_NOT_CONVERGED included)
    int prune;
};

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// LDS of one pair: row points (b, d, s) | u[rows] | col points (b, d, t) | owner[cols] (ints, padded to 8 B);
// (4 * max_rows + 3 * max_cols + ((max_cols + 1) >> 1)) * 8 bytes, and end() is what follows.
struct assign_lds {
    double* rb; double* rd; double* rs; double* ru; double* cb; double* cd; double* ct; int* owner;
    int max_rows, max_cols;
    __device__ __forceinline__ assign_lds(unsigned char* smem, int mr, int mc) : max_rows(mr), max_cols(mc)
    {
        rb = reinterpret_cast<double*>(smem);
        rd = rb + mr; rs = rd + mr; ru = rs + mr;
        cb = ru + mr; cd = cb + mc; ct = cd + mc;
        owner = reinterpret_cast<int*>(ct + mc);
    }
    __device__ __forceinline__ double* end() const { return ct + max_cols + ((max_cols + 1) >> 1); }
};

// The pair as the solver sees it.  M, N: finite points of the first / second diagram (an empty one counts as {(0,0)});
// R rows, Cn columns; a_is_row: the first diagram plays the row role.
struct assign_shape {
    int M, N, R, Cn, cw_used;           // cw_used: column slots per lane actually in use
    bool a_is_row;
};

// ---- the pair prologue ----
// Diagrams ia of (dgm_a, cnt_a, cap_a) and ib of (dgm_b, ...), cleaned as safe_wasserstein cleans them
// (scripts/utils.py:182-187): finite points only, order kept, with their diagonal costs diag(b, d), rows = the smaller
// diagram; ru[] zeroed; ends with a barrier.  Returns false, with S filled and nothing loaded, if the pair does not fit
// the launch: more rows or columns than the LDS layout or than 64 * CW lanes' slots.
template <int CW, class DIAG>
__device__ __forceinline__ bool assign_load_pair(const double* __restrict__ dgm_a, const int* __restrict__ cnt_a, int cap_a,
                                                 int ia, const double* __restrict__ dgm_b, const int* __restrict__ cnt_b,
                                                 int cap_b, int ib, const assign_lds& L, const DIAG& diag, assign_shape& S)
{
    const int lane = lane_id();
    const double* A = dgm_a + (size_t)ia * cap_a * 2;
    const double* B = dgm_b + (size_t)ib * cap_b * 2;
    int ka = cnt_a[ia]; ka = ka < cap_a ? ka : cap_a; ka = ka < 0 ? 0 : ka;
    int kb = cnt_b[ib]; kb = kb < cap_b ? kb : cap_b; kb = kb < 0 ? 0 : kb;
    int M = 0, N = 0;                                                   // finite rows (utils.py:185-186)
    for (int i0 = 0; i0 < ka; i0 += 64) {
        const int i = i0 + lane;
        M += __popcll(__ballot(i < ka && isfinite(A[2 * i]) && isfinite(A[2 * i + 1])));
    }
    for (int i0 = 0; i0 < kb; i0 += 64) {
        const int i = i0 + lane;
        N += __popcll(__ballot(i < kb && isfinite(B[2 * i]) && isfinite(B[2 * i + 1])));
    }
    const int Me = M > 0 ? M : 1, Ne = N > 0 ? N : 1;                   // empty -> {(0,0)}  (utils.py:184,187)
    S.M = M; S.N = N;
    S.a_is_row = Me <= Ne;                                              // rows = the smaller diagram
    S.R = S.a_is_row ? Me : Ne; S.Cn = S.a_is_row ? Ne : Me;
    S.cw_used = (S.Cn + 63) >> 6;
    if (S.R > L.max_rows || S.Cn > L.max_cols || S.Cn > 64 * CW) return false;
    // finite points, order kept, with their diagonal costs
    auto load = [&](const double* __restrict__ P, int k, int n_fin, double* pb, double* pd, double* pc) {
        int m = 0;
        for (int i0 = 0; i0 < k; i0 += 64) {
            const int i = i0 + lane;
            double b = 0, d = 0; bool fin = false;
            if (i < k) { b = P[2 * i]; d = P[2 * i + 1]; fin = isfinite(b) && isfinite(d); }
            const u64 bal = __ballot(fin);
            const int pos = m + __popcll(bal & ((1ull << lane) - 1ull));
            if (fin) { pb[pos] = b; pd[pos] = d; pc[pos] = diag(b, d); }
            m += __popcll(bal);
        }
        if (n_fin == 0 && lane == 0) { pb[0] = 0.0; pd[0] = 0.0; pc[0] = 0.0; }
    };
    const bool ar = S.a_is_row;                 // (selected pointers, not a loader per role: 130 instructions less per kernel)
    load(A, ka, M, ar ? L.rb : L.cb, ar ? L.rd : L.cd, ar ? L.rs : L.ct);
    load(B, kb, N, ar ? L.cb : L.rb, ar ? L.cd : L.rd, ar ? L.ct : L.rs);
    for (int i = lane; i < S.R; i += 64) L.ru[i] = 0.0;
    __syncthreads();
    return true;
}

// Every point of both diagrams has the birth of row 0 and the deaths ascend, in at most 64 rows: the pair for the
// anti-diagonal recurrence that each file keeps for itself.
__device__ __forceinline__ bool assign_on_sorted_line(const assign_shape& S, const assign_lds& L)
{
    const int lane = lane_id();
    bool ok = S.R <= 64;
    const double b0 = L.rb[0];
    for (int i0 = 0; i0 < S.R; i0 += 64) {
        const int i = i0 + lane;
        ok = ok && !__ballot(i < S.R && (L.rb[i] != b0 || (i + 1 < S.R && L.rd[i + 1] < L.rd[i])));
    }
    for (int j0 = 0; j0 < S.Cn; j0 += 64) {
        const int j = j0 + lane;
        ok = ok && !__ballot(j < S.Cn && (L.cb[j] != b0 || (j + 1 < S.Cn && L.cd[j + 1] < L.cd[j])));
    }
    return ok;
}

// The bounding boxes of the rows and of the columns and their largest diagonal costs, wave-uniform: what the
// "every cell dead?" tests of the two files start from.
struct assign_boxes {
    double rb_lo, rb_hi, rd_lo, rd_hi, s_hi;
    double cb_lo, cb_hi, cd_lo, cd_hi, t_hi;
};
__device__ __forceinline__ assign_boxes assign_box_stats(const assign_shape& S, const assign_lds& L)
{
    const int lane = lane_id();
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    assign_boxes b{INF, -INF, INF, -INF, -INF, INF, -INF, INF, -INF, -INF};
    for (int i = lane; i < S.R; i += 64) {
        b.rb_lo = fmin(b.rb_lo, L.rb[i]); b.rb_hi = fmax(b.rb_hi, L.rb[i]);
        b.rd_lo = fmin(b.rd_lo, L.rd[i]); b.rd_hi = fmax(b.rd_hi, L.rd[i]);
        b.s_hi = fmax(b.s_hi, L.rs[i]);
    }
    for (int j = lane; j < S.Cn; j += 64) {
        b.cb_lo = fmin(b.cb_lo, L.cb[j]); b.cb_hi = fmax(b.cb_hi, L.cb[j]);
        b.cd_lo = fmin(b.cd_lo, L.cd[j]); b.cd_hi = fmax(b.cd_hi, L.cd[j]);
        b.t_hi = fmax(b.t_hi, L.ct[j]);
    }
    b.rb_lo = wave_min_f64_dpp(b.rb_lo); b.rb_hi = wave_max_f64_dpp(b.rb_hi);
    b.rd_lo = wave_min_f64_dpp(b.rd_lo); b.rd_hi = wave_max_f64_dpp(b.rd_hi);
    b.cb_lo = wave_min_f64_dpp(b.cb_lo); b.cb_hi = wave_max_f64_dpp(b.cb_hi);
    b.cd_lo = wave_min_f64_dpp(b.cd_lo); b.cd_hi = wave_max_f64_dpp(b.cd_hi);
    b.s_hi = wave_max_f64_dpp(b.s_hi); b.t_hi = wave_max_f64_dpp(b.t_hi);
    return b;
}

// ---- the solve ----
// Shortest augmenting paths with dual variables (Jonker-Volgenant class), exact in float64, at most R (R + 1) / 2
// Dijkstra steps: one step = CW gain evaluations per lane + one wave min-reduction.  Leaves prow[c] = the row matched
// to column lane + 64 * c (or -1) and adds the Dijkstra steps to nsteps; false if a loop bound was hit.  all_dead (the
// caller knows that every gain is 0): nothing to do, every prow stays -1.
template <int CW, class GAIN>
__device__ __forceinline__ bool assign_solve(const assign_shape& S, const assign_lds& L, const GAIN& gain, bool all_dead,
                                             int (&prow)[CW], int& nsteps)
{
    const int lane = lane_id();
    const int R = S.R, Cn = S.Cn, cw_used = S.cw_used;
    int* owner = L.owner;
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    // per-lane state, all in registers: column j = lane + 64*c holds v, minv, way, used, prow;
    // row i = lane + 64*c holds its dual u and the "row is in the alternating tree" flag.
    // The Dijkstra step therefore touches LDS only for the cost row (one read per column slot).
    double v[CW], minv[CW], u[CW];
    int way[CW];
    bool used[CW], rowin[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) { v[c] = 0.0; u[c] = 0.0; prow[c] = -1; way[c] = -1; }

    bool failed = false;
    // ---- row-reduction start: u_i = min_j g_ij, v = 0 is dual feasible; every row whose arg-min
    // column is not claimed by a lower row is assigned at once (tight pair), the rest augment ----
    bool rowdone[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) rowdone[c] = false;
    if (!all_dead) {
        int myarg[CW];
        for (int j = lane; j < Cn; j += 64) owner[j] = 0x7fffffff;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            const int r = lane + 64 * c;
            myarg[c] = -1;
            if (c < cw_used && r < R) {
                // scan starts at column r (rotated): rows whose gains tie (typically all zero: the
                // point prefers the diagonal) then claim DIFFERENT columns instead of all column 0
                double mn = INF; int arg = 0;
                int j = r < Cn ? r : 0;
#pragma unroll 4
                for (int t = 0; t < Cn; ++t) {
                    const double g = gain(r, j);
                    if (g < mn) { mn = g; arg = j; }
                    j = (j + 1 == Cn) ? 0 : j + 1;
                }
                u[c] = mn; myarg[c] = arg;
                atomicMin(&owner[arg], r);
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            if (myarg[c] >= 0) rowdone[c] = owner[myarg[c]] == lane + 64 * c;
            const int j = lane + 64 * c;
            if (c < cw_used && j < Cn) { const int o = owner[j]; prow[c] = (o != 0x7fffffff) ? o : -1; }
        }
    }
    for (int i = 0; i < R && !failed && !all_dead; ++i) {
        {
            int dn = 0;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == (i >> 6)) dn = (int)rl32((u32)(rowdone[c] ? 1 : 0), i & 63);
            if (dn) continue;
        }
#pragma unroll
        for (int c = 0; c < CW; ++c) { minv[c] = INF; used[c] = false; rowin[c] = (lane + 64 * c) == i; }
        int i0 = i, j0 = -1;            // j0 = -1 is the virtual start column holding row i
        int steps = 0;
        while (true) {
            double ui0 = 0.0;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == (i0 >> 6)) ui0 = uni_f64(u[c], i0 & 63);
            // branch-free column update: all cost reads are issued first, invalid / used columns
            // carry +inf candidates
            double best = INF, gg[CW];
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c >= cw_used) break;
                const int j = lane + 64 * c;
                const int jc = j < Cn ? j : Cn - 1;
                gg[c] = gain(i0, jc);
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c >= cw_used) break;
                const bool open = (lane + 64 * c) < Cn && !used[c];
                const double cur = gg[c] - ui0 - v[c];
                const bool upd = open && cur < minv[c];
                minv[c] = upd ? cur : minv[c];
                way[c] = upd ? j0 : way[c];
                const double cnd = open ? minv[c] : INF;
                best = cnd < best ? cnd : best;
            }
            const double delta = wave_min_f64_dpp(best);
            ++nsteps;
            // a column attaining delta; ties go to an unassigned column (ends the path at once),
            // the rule scipy's linear_sum_assignment uses too
            int j1 = -1, j1free = -1;
#pragma unroll
            for (int c = CW - 1; c >= 0; --c) {
                if (c >= cw_used) continue;
                const int j = lane + 64 * c;
                const bool at = j < Cn && !used[c] && minv[c] == delta;
                const u64 bal = __ballot(at);
                const u64 balf = __ballot(at && prow[c] < 0);
                if (bal) j1 = 64 * c + __builtin_ctzll(bal);
                if (balf) j1free = 64 * c + __builtin_ctzll(balf);
            }
            if (j1free >= 0) j1 = j1free;
            if (j1 < 0 || !(delta < INF) || ++steps > Cn + 2) { failed = true; break; }
            // dual update: rows in the tree, used / unused columns
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                if (c >= cw_used) break;
                if (rowin[c]) u[c] += delta;
                if (used[c]) v[c] -= delta;
                else minv[c] -= delta;
            }
            // mark j1 used, continue from its row
            const int c1 = j1 >> 6, l1 = j1 & 63;
            int p1 = -1;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == c1) {
                    p1 = (int)rl32((u32)prow[c], l1);
                    if (lane == l1) used[c] = true;
                }
            j0 = j1;
            if (p1 < 0) break;          // free column reached: augment
            i0 = p1;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == (p1 >> 6) && lane == (p1 & 63)) rowin[c] = true;
        }
        if (failed) break;
        // augment along way[] back to the virtual column
        int guard = 0;
        while (j0 >= 0 && guard++ < Cn + 2) {
            const int c0 = j0 >> 6, l0 = j0 & 63;
            int jprev = -1;
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == c0) jprev = (int)rl32((u32)way[c], l0);
            int newrow = i;
            if (jprev >= 0) {
                const int cp = jprev >> 6, lp = jprev & 63;
#pragma unroll
                for (int c = 0; c < CW; ++c)
                    if (c == cp) newrow = (int)rl32((u32)prow[c], lp);
            }
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (c == c0 && lane == l0) prow[c] = newrow;
            j0 = jprev;
        }
        // the flips ran into their bound (cannot fire: a path has one column per Dijkstra step, and those are <= Cn + 2)
        if (j0 >= 0) failed = true;
    }
    return !failed;
}

// ---- the re-summation ----
// The value of the matching in prow[], from the ORIGINAL costs: cfull(i, j) of the real matches (gain < 0), the diagonal
// cost of every other point.  Uses ru[] as "row is really matched" flag.  Wave-uniform.
template <int CW, class CFULL>
__device__ __forceinline__ double assign_resum(const assign_shape& S, const assign_lds& L, const CFULL& cfull,
                                               const int (&prow)[CW])
{
    const int lane = lane_id();
    double part = 0.0;
    __syncthreads();
    for (int i = lane; i < S.R; i += 64) L.ru[i] = 0.0;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CW; ++c) {
        const int j = lane + 64 * c;
        if (j < S.Cn) {
            bool real = false;
            if (prow[c] >= 0) {
                const double cf = cfull(prow[c], j);
                if (cf - L.rs[prow[c]] - L.ct[j] < 0.0) { real = true; part += cf; L.ru[prow[c]] = 1.0; }
            }
            if (!real) part += L.ct[j];
        }
    }
    __syncthreads();
    for (int i = lane; i < S.R; i += 64)
        if (L.ru[i] == 0.0) part += L.rs[i];
    return wave_sum_f64(part);
}

// ---- host side: the column slots per lane of a launch whose diagrams have up to max_cols columns ----
// f(std::integral_constant<int, CW>) with CW = 2, 4 or 8; returns what f returns.
template <class F>
static inline tda_status assign_with_cw(int max_cols, const F& f)
{
    if (max_cols <= 128) return f(std::integral_constant<int, 2>{});
    if (max_cols <= 256) return f(std::integral_constant<int, 4>{});
    return f(std::integral_constant<int, 8>{});
}
