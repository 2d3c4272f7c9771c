// sliced_matrix.hip -- the sliced Wasserstein distance with every diagram sorted ONCE (tda_sliced_prepare_dev) and the
// pairs reduced to two merges and a sum (tda_sliced_prepared_pairs_dev, tda_sliced_matrix_dev).  gfx950 / wave64.
//
// The definition is the text in include/tdaeeg.h, the pair kernel is sliced.hip.  For a pair (A, B) and a direction the
// sorted projections of A' = rows of A + images of B are the merge of two lists that depend on one diagram each: the
// sorted projections of A's rows and the sorted projections of B's images.  A merge of two sorted lists is the sorted
// list of their union, so every u_i, v_i and t_i = fabs(u_i - v_i) is the float64 of the pair kernel; the additions are
// made in the pair kernel's order (rank e = 64 r + lane belongs to `lane`, r = 0, 1, .. in turn and only e < N, the
// butterfly lane ^ 1, 2, .., 32, L_k to LDS, one wave adds the L_k as k = lane, lane + 64, the butterfly, / n_dirs), so
// a prepared pair returns the bytes of tda_sliced_wasserstein_batch_dev.
//
// 1. sliced_prepare_kernel, one workgroup of SW_WAVES waves per diagram.  Wave 0 cleans the diagram into LDS (sw_load:
//    cnt clamped to [0, cap], rows with a non-finite entry dropped, none -> {(0, 0)}; ceil(cap / 64) rounds).  The waves
//    take the 2 n_dirs lists in turn, q = wave, wave + SW_WAVES, .. (direction q >> 1, kind q & 1): project -- kind 0
//    (c * b) + (s * d), kind 1 (c * h) + (s * h), the formula of the header, contraction off --, pad with +inf to 64 V
//    elements, sort with the network of sliced_dev.h (V = 1, 2, 4, 8 by m, workgroup-uniform; MAXV by cap), write the
//    ranks < m.  Loop bounds: ceil(2 n_dirs / SW_WAVES) <= 64 lists per wave; the network is straight-line code.
// 2. the merge.  A wave stages the four lists of (pair, direction) in its own 8 KB of LDS -- [A kind 0 (m) | B kind 1 (n) |
//    B kind 0 (n) | A kind 1 (m)], 2 N <= 1,024 doubles, ceil(m / 64) + ceil(n / 64) rounds of coalesced loads -- and the
//    lane of rank e finds u_e and v_e by a co-rank search: with K = e + 1, the smallest i in [max(0, K - ny), min(K, nx)]
//    with i at its upper end or X[i] > Y[K - i - 1] is the number of elements of X among the first K of the merge, and
//    the element of rank e is max(X[i - 1], Y[K - i - 1]).  SM_SEARCH = 10 = ceil(log2(TDA_SW_MAX_POINTS + 1)) halvings,
//    always: a lane that has found its i goes through the remaining rounds without moving; the two searches of a rank
//    run side by side.  Ties may fall either way: the value of rank e is the same, and 0.0 against -0.0 does not change
//    a t_i.
// 3. sliced_pairs_kernel, one workgroup per pair: the waves take the directions in turn, k = k0 + wave, with a workgroup
//    barrier between the staging of a round and its searches and one behind them (the staging of a wave is read by all
//    its lanes); ceil(n_dirs / SW_WAVES) <= 32 rounds, the same for every wave.
// 4. sliced_matrix_kernel, one workgroup per entry (A group g, column c); block b is g = b % n_seg_a, c = b / n_seg_a, so
//    the workgroups in flight at one time read the same few columns of the bank (its B groups of the n_cls classes) while
//    the A side, a shard's table, is small.  The threads resolve the positions of the group by the rules of
//    ws_matrix_entry (wasserstein.hip); the (position, direction) items of SM_CHUNK_L / n_dirs positions at a time are
//    dealt to the waves, item = it0 + wave, their L_k land in LDS, the waves add the L_k of a position each (the pair
//    kernel's last sum), and thread 0 reduces the group's values with ws_matrix_entry's arithmetic (numpy's pairwise leaf:
//    a group has at most 64 diagrams).  Loop bounds: ceil(n_try / P) chunks, ceil(P n_dirs / SW_WAVES) <= 256 rounds per
//    chunk, ceil(P / SW_WAVES) sums.  The A lists are read again for every column (from L2: see DESIGN.md 3.12 for what
//    staging them per tile of columns would take); no per-pair array exists in HBM, nothing is cleared, no atomics.
#include "sliced_dev.h"

#pragma clang fp contract(off)

#define SM_SEARCH 10                     // ceil(log2(TDA_SW_MAX_POINTS + 1))
#define SM_STAGE (2 * TDA_SW_MAX_POINTS)  // doubles of staging per wave
#define SM_CHUNK_L 1024                  // L_k slots of the matrix kernel: 1024 / n_dirs >= 8 positions at a time
#define SM_MAX_GROUP 64                  // WS_MATRIX_MAX_GROUP

static_assert((1 << SM_SEARCH) >= TDA_SW_MAX_POINTS + 1 && (1 << (SM_SEARCH - 1)) < TDA_SW_MAX_POINTS + 1, "trip count");

// ---- prepare ---------------------------------------------------------------------------------------------------------
template <int V>
__device__ __forceinline__ void sm_sorted_list(const double* pts, const double* hs, int m, int kind, double c, double s,
                                               int lane, double* __restrict__ dst)
{
    const double INF = __longlong_as_double(0x7ff0000000000000ll);
    double x[V];
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int e = 64 * r + lane;
        double px = 0.0, py = 0.0;
        if (e < m) {
            if (kind == 0) { px = pts[2 * e]; py = pts[2 * e + 1]; }
            else { px = hs[e]; py = px; }
        }
        const double p = (c * px) + (s * py);
        x[r] = e < m ? p : INF;
    }
    sw_sort<V, 2>(x, lane);
#pragma unroll
    for (int r = 0; r < V; ++r) {
        const int e = 64 * r + lane;
        if (e < m) dst[e] = x[r];
    }
}

// LDS: rows (2 max_m) | h (max_m) | m
template <int MAXV>
__global__ void __launch_bounds__(64 * SW_WAVES)
sliced_prepare_kernel(const double* __restrict__ dgm, const int* __restrict__ cnt, int cap, int n_dgm, int max_m,
                      const double* __restrict__ dirs, int n_dirs, const long long* __restrict__ slot_off,
                      double* __restrict__ table, long long table_rows, int* __restrict__ m_clean)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int i = blockIdx.x;
    if (i >= n_dgm) return;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    double* pts = reinterpret_cast<double*>(smem);
    double* hs = pts + 2 * max_m;
    int* mm = reinterpret_cast<int*>(hs + max_m);
    if (wave == 0) {
        int k = uni(cnt[i]); k = k < cap ? k : cap; k = k < 0 ? 0 : k;
        const int m = sw_load(dgm + (size_t)i * cap * 2, k, max_m, pts, hs);
        if (lane == 0) mm[0] = m;
    }
    __syncthreads();
    const int m = uni(mm[0]);
    const long long o0 = slot_off[i], o1 = slot_off[i + 1];
    // (the same for every thread of the workgroup)
    if (m > TDA_SW_MAX_POINTS || m > max_m || m > 64 * MAXV || o0 < 0 || o1 < o0 || (long long)m > o1 - o0 || o1 > table_rows) {
        if (threadIdx.x == 0) m_clean[i] = -1;
        return;
    }
    const size_t slot = (size_t)(o1 - o0);
    double* reg = table + (size_t)2 * (size_t)n_dirs * (size_t)o0;
    for (int q = wave; q < 2 * n_dirs; q += SW_WAVES) {
        const int k = q >> 1, kind = q & 1;
        const double c = dirs[2 * k], s = dirs[2 * k + 1];
        double* dst = reg + (size_t)q * slot;
        if (MAXV == 1 || m <= 64) sm_sorted_list<1>(pts, hs, m, kind, c, s, lane, dst);
        else if (MAXV == 2 || m <= 128) sm_sorted_list<(MAXV >= 2 ? 2 : 1)>(pts, hs, m, kind, c, s, lane, dst);
        else if (MAXV == 4 || m <= 256) sm_sorted_list<(MAXV >= 4 ? 4 : 1)>(pts, hs, m, kind, c, s, lane, dst);
        else sm_sorted_list<(MAXV >= 8 ? 8 : 1)>(pts, hs, m, kind, c, s, lane, dst);
    }
    if (threadIdx.x == 0) m_clean[i] = m;
}

tda_status launch_sliced_prepare(tda_ctx* ctx, const double* dgm, const int* cnt, int cap, int n_dgm, const double* dirs,
                                 int n_dirs, const long long* slot_off, double* table, long long table_rows, int* m_clean,
                                 hipStream_t st)
{
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "1 <= n_dirs <= TDA_MAX_DIRECTIONS");
    if (cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "diagram capacity must be >= 1");
    if (n_dgm == 0) return TDA_OK;
    const int max_m = cap < TDA_SW_MAX_POINTS ? cap : TDA_SW_MAX_POINTS;
    const size_t lds = (size_t)(3 * max_m + 1) * 8;                       // <= 12.3 KB
#define SM_PREP(MV)                                                                                                   \
    hipLaunchKernelGGL(sliced_prepare_kernel<MV>, dim3(n_dgm), dim3(64 * SW_WAVES), lds, st, dgm, cnt, cap, n_dgm, max_m, \
                       dirs, n_dirs, slot_off, table, table_rows, m_clean)
    if (max_m <= 64) SM_PREP(1);
    else if (max_m <= 128) SM_PREP(2);
    else if (max_m <= 256) SM_PREP(4);
    else SM_PREP(8);
#undef SM_PREP
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---- the merge -------------------------------------------------------------------------------------------------------
// one prepared diagram: its region of the table, the rows of its slot, its m (< 0: not prepared)
struct sm_dgm { const double* reg; size_t slot; int m; };

__device__ __forceinline__ sm_dgm sm_resolve(const double* __restrict__ table, const long long* __restrict__ slot_off,
                                             const int* __restrict__ m_clean, int i, int n_dirs)
{
    const long long o0 = slot_off[i], o1 = slot_off[i + 1];
    int m = m_clean[i];
    if (o0 < 0 || o1 < o0 || (long long)m > o1 - o0) m = -1;             // (a table that prepare did not write)
    return sm_dgm{table + (size_t)2 * (size_t)n_dirs * (size_t)(o0 < 0 ? 0 : o0), (size_t)(o1 > o0 ? o1 - o0 : 0), m};
}

// the four lists of direction k into the wave's staging: A kind 0 (m) | B kind 1 (n) | B kind 0 (n) | A kind 1 (m)
__device__ __forceinline__ void sm_stage(double* stg, const sm_dgm& A, const sm_dgm& B, int k, int lane)
{
    const int m = A.m, n = B.m, N = m + n;
    const double* a0 = A.reg + (size_t)(2 * k) * A.slot;
    const double* a1 = a0 + A.slot;
    const double* b0 = B.reg + (size_t)(2 * k) * B.slot;
    const double* b1 = b0 + B.slot;
    for (int e = lane; e < m; e += 64) { stg[e] = a0[e]; stg[N + n + e] = a1[e]; }
    for (int e = lane; e < n; e += 64) { stg[m + e] = b1[e]; stg[N + e] = b0[e]; }
}

// one co-rank search: the range of i for rank e, a halving, the element once i is found
struct sm_search {
    const double* X; const double* Y; int nx, ny, K, lo, hi;
    __device__ __forceinline__ sm_search(const double* X_, int nx_, const double* Y_, int ny_, int e)
        : X(X_), Y(Y_), nx(nx_), ny(ny_), K(e + 1), lo(e + 1 - ny_ > 0 ? e + 1 - ny_ : 0), hi(e + 1 < nx_ ? e + 1 : nx_) {}
    __device__ __forceinline__ void halve()
    {
        const bool active = lo < hi;
        const int mid = (lo + hi) >> 1;                                   // active: lo <= mid < hi <= nx, 0 <= K - mid - 1 < ny
        int jy = K - mid - 1; jy = jy < 0 ? 0 : jy; jy = jy < ny ? jy : ny - 1;
        const double xi = X[mid < nx ? mid : nx - 1], yj = Y[jy];
        const bool above = xi > yj;
        hi = (active && above) ? mid : hi;
        lo = (active && !above) ? mid + 1 : lo;
    }
    __device__ __forceinline__ double value() const
    {
        const int i = lo, j = K - lo;
        const double NINF = __longlong_as_double(0xfff0000000000000ll);
        const double a = i > 0 ? X[i - 1] : NINF, b = j > 0 ? Y[j - 1] : NINF;
        return a > b ? a : b;
    }
};

// L_k of one staged direction, by one wave: the same bits on every lane.  The two searches of a rank (u_e in the merge of
// A kind 0 with B kind 1, v_e in the merge of B kind 0 with A kind 1) go through their SM_SEARCH halvings side by side:
// they are independent, and a halving is one LDS round trip that the other one's hides.
__device__ __forceinline__ double sm_direction(const double* stg, int m, int n, int lane)
{
    const int N = m + n;
    double acc = 0.0;
    for (int e0 = 0; e0 < N; e0 += 64) {                                  // register r = e0 / 64 of the pair kernel
        const int e = e0 + lane;
        if (e < N) {
            sm_search su(stg, m, stg + m, n, e), sv(stg + N, n, stg + N + n, m, e);
#pragma unroll
            for (int t = 0; t < SM_SEARCH; ++t) { su.halve(); sv.halve(); }
            acc += fabs(su.value() - sv.value());
        }
    }
    return sw_wave_sum(acc);
}

// ---- prepared pairs ----------------------------------------------------------------------------------------------------
struct sm_side { const double* table; const long long* slot_off; const int* m; int n; };

__global__ void __launch_bounds__(64 * SW_WAVES)
sliced_pairs_kernel(const sm_side SA, const sm_side SB, const int* __restrict__ idx_a, const int* __restrict__ idx_b,
                    int n_pairs, int n_dirs, double* __restrict__ out, int* __restrict__ status)
{
    __shared__ double stage[SW_WAVES][SM_STAGE];
    __shared__ double Ls[TDA_MAX_DIRECTIONS];
    const int pr = blockIdx.x;
    if (pr >= n_pairs) return;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const int ia = uni(idx_a ? idx_a[pr] : pr), ib = uni(idx_b ? idx_b[pr] : pr);
    if (ia < 0 || ia >= SA.n || ib < 0 || ib >= SB.n) {                  // (the same for every thread of the workgroup)
        if (threadIdx.x == 0) { out[pr] = qnan; status[pr] = TDA_WIN_NO_PAIR; }
        return;
    }
    const sm_dgm A = sm_resolve(SA.table, SA.slot_off, SA.m, ia, n_dirs);
    const sm_dgm B = sm_resolve(SB.table, SB.slot_off, SB.m, ib, n_dirs);
    if (A.m < 1 || B.m < 1 || A.m + B.m > TDA_SW_MAX_POINTS) {
        if (threadIdx.x == 0) { out[pr] = qnan; status[pr] = TDA_WIN_TOO_LARGE; }
        return;
    }
    for (int k0 = 0; k0 < n_dirs; k0 += SW_WAVES) {
        const int k = k0 + wave;
        if (k < n_dirs) sm_stage(stage[wave], A, B, k, lane);
        __syncthreads();
        if (k < n_dirs) {
            const double L = sm_direction(stage[wave], A.m, B.m, lane);
            if (lane == 0) Ls[k] = L;
        }
        __syncthreads();
    }
    if (wave == 0) {
        double acc = 0.0;
        for (int k = lane; k < n_dirs; k += 64) acc += Ls[k];
        acc = sw_wave_sum(acc);
        if (lane == 0) { out[pr] = acc / (double)n_dirs; status[pr] = 0; }
    }
}

tda_status launch_sliced_prepared_pairs(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a,
                                        int n_a, const double* table_b, const long long* slot_off_b, const int* m_b, int n_b,
                                        const int* idx_a, const int* idx_b, int n_pairs, int n_dirs, double* out, int* status,
                                        hipStream_t st)
{
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "1 <= n_dirs <= TDA_MAX_DIRECTIONS");
    if (n_pairs == 0) return TDA_OK;
    const sm_side SA{table_a, slot_off_a, m_a, n_a}, SB{table_b, slot_off_b, m_b, n_b};
    hipLaunchKernelGGL(sliced_pairs_kernel, dim3(n_pairs), dim3(64 * SW_WAVES), 0, st, SA, SB, idx_a, idx_b, n_pairs, n_dirs,
                       out, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

// ---- the matrix ------------------------------------------------------------------------------------------------------
struct sm_matrix_args {
    const int* seg_off_a; const int* cls_a; const int* seg_off_b; const int* status_b;
    int n_seg_a, n_cls, n_col;
    double* out; int* pairs; int* flags;
};

// numpy's sum of n <= 128 terms (ws_np_sum of wasserstein.hip, restated: that file's kernels are not to move)
template <class F>
__device__ __forceinline__ double sm_np_sum(const F& f, int n)
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

// entries b0 .. b0 + gridDim.x - 1 in the order g fastest
__global__ void __launch_bounds__(64 * SW_WAVES)
sliced_matrix_kernel(const sm_side SA, const sm_side SB, const sm_matrix_args M, size_t blk0, int n_dirs)
{
    __shared__ double stage[SW_WAVES][SM_STAGE];
    __shared__ double Ls[SM_CHUNK_L];
    __shared__ double xs[SM_MAX_GROUP];
    __shared__ int ss[SM_MAX_GROUP], pib[SM_MAX_GROUP];                   // status word, B diagram (-1: nothing to compute)
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), tid = (int)threadIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const size_t blk = blk0 + blockIdx.x;
    const int g = (int)(blk % (size_t)M.n_seg_a), c = (int)(blk / (size_t)M.n_seg_a);
    const size_t e = (size_t)g * (size_t)M.n_col + (size_t)c;
    // the two groups; indices that leave a table: no pair (ws_matrix_entry)
    const int a0 = uni(M.seg_off_a[g]), a1 = uni(M.seg_off_a[g + 1]);
    const int len = (a0 >= 0 && a1 >= a0 && a1 <= SA.n) ? a1 - a0 : 0;
    const int cls = uni(M.cls_a[g]);
    int b0 = 0, len_b = 0;
    if (cls >= 0 && cls < M.n_cls) {
        const size_t p = (size_t)cls * M.n_col + c;
        b0 = uni(M.seg_off_b[p]);
        len_b = uni(M.seg_off_b[p + 1]) - b0;
    }
    if (len > SM_MAX_GROUP) {
        if (tid == 0) { M.out[e] = qnan; M.pairs[e] = 0; M.flags[e] = TDA_WIN_TOO_LARGE; }
        return;
    }
    const int n_try = len < len_b ? len : len_b;                          // (<= 0: no position has a partner)
    if (tid < len) {
        double x = qnan; int s = TDA_WIN_NO_PAIR, ibw = -1;
        if (tid < n_try) {
            const int ib = b0 + tid;
            if (ib >= 0 && ib < SB.n && !(M.status_b[ib] & TDA_WIN_DEGENERATE)) {
                const sm_dgm A = sm_resolve(SA.table, SA.slot_off, SA.m, a0 + tid, n_dirs);
                const sm_dgm B = sm_resolve(SB.table, SB.slot_off, SB.m, ib, n_dirs);
                if (A.m < 1 || B.m < 1 || A.m + B.m > TDA_SW_MAX_POINTS) s = TDA_WIN_TOO_LARGE;
                else { s = 0; ibw = ib; }
            }
        }
        xs[tid] = x; ss[tid] = s; pib[tid] = ibw;
    }
    __syncthreads();
    const int P = SM_CHUNK_L / n_dirs;                                    // positions per chunk, >= 8
    for (int i0 = 0; i0 < n_try; i0 += P) {
        const int np = n_try - i0 < P ? n_try - i0 : P, items = np * n_dirs;
        for (int it0 = 0; it0 < items; it0 += SW_WAVES) {
            const int it = it0 + wave;
            const int j = it / n_dirs, k = it - j * n_dirs;
            const int ib = it < items ? uni(pib[i0 + j]) : -1;
            sm_dgm A{nullptr, 0, 0}, B{nullptr, 0, 0};
            if (ib >= 0) {
                A = sm_resolve(SA.table, SA.slot_off, SA.m, a0 + i0 + j, n_dirs);
                B = sm_resolve(SB.table, SB.slot_off, SB.m, ib, n_dirs);
                sm_stage(stage[wave], A, B, k, lane);
            }
            __syncthreads();
            if (ib >= 0) {
                const double L = sm_direction(stage[wave], A.m, B.m, lane);
                if (lane == 0) Ls[it] = L;
            }
            __syncthreads();
        }
        for (int j = wave; j < np; j += SW_WAVES) {                       // the pair kernel's last sum, a position per wave
            if (uni(pib[i0 + j]) < 0) continue;
            double acc = 0.0;
            for (int k = lane; k < n_dirs; k += 64) acc += Ls[j * n_dirs + k];
            acc = sw_wave_sum(acc);
            if (lane == 0) xs[i0 + j] = acc / (double)n_dirs;
        }
        __syncthreads();
    }
    if (tid == 0) {                                                       // cross_rows_kernel's arithmetic, as ws_matrix_entry
        int n = 0, cnt = 0, fl = 0;
        for (int i = 0; i < len; ++i) n += (ss[i] & TDA_WIN_NO_PAIR) ? 0 : 1;
        for (int i = 0; i < n; ++i) {
            cnt += (ss[i] == 0 && xs[i] == xs[i]) ? 1 : 0;
            fl |= ss[i];
        }
        auto val = [&](int j) { const double v = xs[j]; return (ss[j] == 0 && v == v) ? v : 0.0; };
        const double sum = sm_np_sum(val, n);
        M.out[e] = cnt > 0 ? sum / (double)cnt : qnan;
        M.pairs[e] = n;
        M.flags[e] = fl & ~(TDA_WIN_NO_PAIR | TDA_WIN_DEGENERATE);
    }
}

#define SM_MATRIX_GRID_CHUNK ((size_t)1 << 30)   // entries per launch (gridDim.x)

tda_status launch_sliced_matrix(tda_ctx* ctx, const double* table_a, const long long* slot_off_a, const int* m_a, int n_a,
                                const int* seg_off_a, int n_seg_a, const int* cls_a, const double* table_b,
                                const long long* slot_off_b, const int* m_b, int n_b, const int* seg_off_b, int n_cls,
                                int n_col, const int* status_b, int n_dirs, double* out, int* pairs, int* flags, hipStream_t st)
{
    if (n_dirs < 1 || n_dirs > TDA_MAX_DIRECTIONS) TDA_FAIL(ctx, TDA_ERR_INVALID, "1 <= n_dirs <= TDA_MAX_DIRECTIONS");
    const size_t n_ent = (size_t)n_seg_a * (size_t)n_col;
    if (n_ent == 0) return TDA_OK;
    const sm_side SA{table_a, slot_off_a, m_a, n_a}, SB{table_b, slot_off_b, m_b, n_b};
    const sm_matrix_args M{seg_off_a, cls_a, seg_off_b, status_b, n_seg_a, n_cls, n_col, out, pairs, flags};
    for (size_t b0 = 0; b0 < n_ent; b0 += SM_MATRIX_GRID_CHUNK) {
        const size_t nb = n_ent - b0 < SM_MATRIX_GRID_CHUNK ? n_ent - b0 : SM_MATRIX_GRID_CHUNK;
        hipLaunchKernelGGL(sliced_matrix_kernel, dim3((unsigned)nb), dim3(64 * SW_WAVES), 0, st, SA, SB, M, b0, n_dirs);
    }
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
