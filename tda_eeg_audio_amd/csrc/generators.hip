// generators.hip -- the simplices behind the rows of a Rips diagram and a representative cycle of every H1 row
// (include/tdaeeg.h, "Generators and representative cycles").  Integers: the output is the bytes of
// tests/generators_ref.py or it is wrong.  The Rips kernels are not touched: the edges are recovered after the fact from
// the keys and the rows, by a local rule.
//
// One workgroup of 256 threads (four waves) per window.
//   Keys.   The float32 keys k[a][b], a > b, once per window into an LDS triangle (32.5 KB at 128 points) by window_keys of
//           csrc/rips_keys_dev.h, the one statement of the key rules of the Rips kernels (tests/test_gpu_generators.py
//           pins them to the oracle).  The edges are ordered by (key, flat index tri2(a) + b); G_e is the graph of the
//           edges with k <= (float)thresh that precede e.
//   Items.  A work item is a maximal run of H1 rows with equal birth, or of H0 rows with equal death.  Every wave walks the
//           rows (a loop of known length over values every lane reads alike) and takes the runs w, w + 4, ...  Nothing in
//           the row loop waits for another wave.
//   Lookup. For the value x of its item the wave's lanes scan the keys 64 at a time for (double)k == x and ballot: the
//           candidates come in flat-index order.  Per candidate e = (a, b):
//             cn(e)     lane u reads k[a][u] and k[b][u] (two key reads), judges both edges against e, ballots: one mask
//                       row of a AND one of b.  A candidate with a common neighbour is a death edge, never searched.
//             search    lane v builds the adjacency masks of the vertices v and v + 64 in G_e (n key reads each), then a
//                       breadth-first search from b in level sets: the frontier is a 128-bit mask every lane holds, a
//                       vertex joins when adj & frontier != 0, its parent is ctz(adj & frontier).  At most n levels.
//                       a reached: e is a birth edge, the cycle is a, parent(a), ..., b.  Not reached: a forest edge.
//           The searches of a window are bounded by |F| + |B| however many keys tie.
//   Loop bounds, all known before the loop: the row counts, the number of key chunks, a popcount, n levels.  No polls, no
//   atomics, nothing allocated.  Every row below the count is written whole by the wave that owns its run; the rows above
//   it, and every row of a skipped, degenerate or refused window, get the fill values.
//   Part.   After one workgroup barrier thread v adds d - b over the unflagged rows with finite d whose cycle holds v, in
//           row order.
// The group means are a second small launch: one thread per (group, vertex) adds the windows of its group in order
// (group_mean_kernel of common.h).
#include "common.h"
#include "rips_keys_dev.h"

#define GN_NT 256
#define GN_WAVES (GN_NT / 64)

// is the edge of key k and flat index f in G_e, e of key ke and flat index fe?  (a NaN key is no edge)
__device__ __forceinline__ bool gn_before(float k, int f, float ke, int fe, float thresh)
{
    return k <= thresh && (k < ke || (k == ke && f < fe));
}

// what a wave knows about its window
struct GnWin {
    const float* key;
    int n, E, lane;
    float thresh;
};

// the candidates of chunk `base` for the value x: bit l = edge base + l has (double)k == x and k <= thresh
__device__ __forceinline__ u64 gn_match(const GnWin& W, int base, double x)
{
    const int e = base + W.lane;
    bool m = false;
    if (e < W.E) {
        const float k = W.key[e];
        m = k <= W.thresh && (double)k == x;
    }
    return __ballot(m);
}

template <int NW>
__device__ __forceinline__ bool gn_cn(const GnWin& W, int a, int b, float ke, int fe)
{
    bool any = false;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int u = W.lane + 64 * w;
        bool in = false;
        if (u < W.n && u != a && u != b) {
            const int fa = pair_index(a, u), fb = pair_index(b, u);
            in = gn_before(W.key[fa], fa, ke, fe, W.thresh) && gn_before(W.key[fb], fb, ke, fe, W.thresh);
        }
        any |= __ballot(in) != 0ull;
    }
    return any;
}

// Breadth-first search from b in G_e, e = (a, b).  Returns the length of the walk a, parent(a), ..., b (0: a is not
// reached); lane l then holds its vertices l and l + 64 in walk[0] and walk[NW - 1].
template <int NW>
__device__ __forceinline__ int gn_search(const GnWin& W, int a, int b, float ke, int fe, int (&walk)[NW], int& levels)
{
    const int n = W.n, lane = W.lane;
    u64 adj[NW][NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
        for (int x = 0; x < NW; ++x) adj[w][x] = 0ull;
        const int v = lane + 64 * w;
        if (v < n) {
            for (int u = 0; u < n; ++u) {
                if (u == v) continue;
                const int f = pair_index(v, u);
                const bool in = gn_before(W.key[f], f, ke, fe, W.thresh);
                if (NW == 1) adj[w][0] |= (u64)in << u;
                else if (u < 64) adj[w][0] |= (u64)in << u;
                else adj[w][NW - 1] |= (u64)in << (u - 64);
            }
        }
    }
    u64 vis[NW], fr[NW];
    int par[NW];
#pragma unroll
    for (int x = 0; x < NW; ++x) {
        vis[x] = ((b >> 6) == x) ? 1ull << (b & 63) : 0ull;
        fr[x] = vis[x];
        par[x] = -1;
        walk[x] = -1;
    }
    bool reached = false;
    for (int lvl = 0; lvl < n && !reached; ++lvl) {
        u64 nf[NW];
        bool some = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            bool hit = false;
            if (!((vis[w] >> lane) & 1ull)) {                       // (a lane past n has no adjacency)
#pragma unroll
                for (int x = 0; x < NW; ++x) {
                    const u64 m = adj[w][x] & fr[x];
                    if (m && !hit) { hit = true; par[w] = 64 * x + __builtin_ctzll(m); }
                }
            }
            nf[w] = __ballot(hit);
            some |= nf[w] != 0ull;
        }
        if (!some) break;
        ++levels;
#pragma unroll
        for (int x = 0; x < NW; ++x) { vis[x] |= nf[x]; fr[x] = nf[x]; }
        reached = (((NW == 2 && a >= 64) ? nf[NW - 1] : nf[0]) >> (a & 63)) & 1ull;
    }
    if (!reached) return 0;
    int len = 0, cur = a;
    for (int step = 0; step < n; ++step) {
        if ((len & 63) == lane) {
            if (NW == 1 || len < 64) walk[0] = cur; else walk[NW - 1] = cur;
        }
        ++len;
        if (cur == b) break;
        const int p = (NW == 2 && cur >= 64) ? par[NW - 1] : par[0];
        cur = __shfl(p, cur & 63, 64);
    }
    return len;
}

// the cycle slots of one row: lane l owns the slots l and l + 64
__device__ __forceinline__ void gn_store_cycle(short* row, int cyc_cap, int lane, int len, int w0, int w1)
{
    if (!row) return;                                                // (cyc is optional)
    if (lane < cyc_cap) row[lane] = (short)(lane < len ? w0 : -1);
    if (lane + 64 < cyc_cap) row[lane + 64] = (short)(lane + 64 < len ? w1 : -1);
}

template <int NW>
__global__ void __launch_bounds__(GN_NT)
generators_kernel(WinSrc src, float thresh, KeyLayout L, GenArgs io, int* __restrict__ n_points, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float* key = reinterpret_cast<const float*>(smem);
    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h1_cap = io.h1_cap, h0_cap = io.h0_cap, cyc_cap = io.cyc_cap;
    short* gen = io.h1_gen + (size_t)win * h1_cap * 4;
    int* rflag = io.h1_flag + (size_t)win * h1_cap;
    short* cyc = io.cyc ? io.cyc + (size_t)win * h1_cap * cyc_cap : nullptr;
    int* clen = io.cyc_len + (size_t)win * h1_cap;
    short* h0e = io.h0_edge ? io.h0_edge + (size_t)win * h0_cap * 2 : nullptr;
    double* part = io.part ? io.part + (size_t)win * io.part_ld : nullptr;

    const WinExtent X = win_extent(src, win);
    const int st = win_status(src, X, win, n_points), n = st ? 0 : (int)X.P;
    if (tid == 0) status[win] = st;
    const bool skip = st != 0 || (io.rips_status && (io.rips_status[win] & io.skip_mask));
    int R1 = 0, R0 = 0;
    if (!skip) {
        R1 = io.h1_cnt[win]; R1 = R1 < 0 ? 0 : (R1 > h1_cap ? h1_cap : R1);
        if (h0e) { R0 = io.h0_cnt[win]; R0 = R0 < 0 ? 0 : (R0 > h0_cap ? h0_cap : R0); }
    }
    // fill values for every row no run owns
    for (int r = R1 + (tid >> 6); r < h1_cap; r += GN_WAVES) {
        if (lane < 4) gen[r * 4 + lane] = -1;
        if (lane == 0) { rflag[r] = 0; clen[r] = 0; }
        gn_store_cycle(cyc ? cyc + (size_t)r * cyc_cap : nullptr, cyc_cap, lane, 0, -1, -1);
    }
    if (h0e) for (int i = 2 * R0 + tid; i < 2 * h0_cap; i += GN_NT) h0e[i] = -1;
    if (skip) {
        if (io.work && tid < 2 * GN_WAVES) io.work[(size_t)win * 2 * GN_WAVES + tid] = 0;
        if (part) for (int v = tid; v < io.part_ld; v += GN_NT) part[v] = 0.0;
        return;
    }

    window_keys<GN_NT>(src, X, n, smem, L);

    GnWin W;
    W.key = key; W.n = n; W.E = tri2(n); W.lane = lane; W.thresh = thresh;
    const double* h1 = io.h1 + (size_t)win * h1_cap * 2;
    int searches = 0, levels = 0, run = 0;
    // the last death looked up by this wave: rows of equal death share one lookup
    double last_d = 0.0; int last_e = -1, last_cnt = -1;

    for (int r0 = 0; r0 < R1;) {
        const double bv = h1[2 * r0];
        int r1 = r0 + 1;
        while (r1 < R1 && h1[2 * r1] == bv) ++r1;
        if ((run++ & (GN_WAVES - 1)) == wave) {
            // a. the birth edges: the candidates of B with this key in order, one per row
            int found = 0;
            for (int cb = 0; cb < W.E; cb += 64) {
                u64 m = gn_match(W, cb, bv);
                while (m) {
                    const int e = cb + __builtin_ctzll(m);
                    m &= m - 1;
                    const int a = edge_row(e), b = e - tri2(a);
                    const float ke = key[e];
                    if (gn_cn<NW>(W, a, b, ke, e)) continue;
                    int walk[NW];
                    ++searches;
                    const int len = gn_search<NW>(W, a, b, ke, e, walk, levels);
                    if (len == 0) continue;                          // a forest edge
                    if (r0 + found < r1) {
                        const int r = r0 + found;
                        if (lane == 0) {
                            gen[r * 4] = (short)a; gen[r * 4 + 1] = (short)b;
                            clen[r] = len;
                            rflag[r] = len > cyc_cap ? TDA_GEN_CYCLE_TRUNCATED : 0;
                        }
                        gn_store_cycle(cyc ? cyc + (size_t)r * cyc_cap : nullptr, cyc_cap, lane, len, walk[0], walk[NW - 1]);
                    }
                    ++found;
                }
            }
            // b. the death edges and the flags, row by row
            for (int r = r0; r < r1; ++r) {
                const double d = h1[2 * r + 1];
                int fl = found != r1 - r0 ? TDA_GEN_BIRTH_TIED : 0;
                if (r - r0 >= found) fl |= TDA_GEN_NO_EDGE;
                int de = -1;
                if (d != (double)INFINITY) {
                    if (last_cnt < 0 || !(d == last_d)) {
                        last_d = d; last_e = -1; last_cnt = 0;
                        for (int cb = 0; cb < W.E; cb += 64) {
                            u64 m = gn_match(W, cb, d);
                            while (m && last_cnt < 2) {
                                const int e = cb + __builtin_ctzll(m);
                                m &= m - 1;
                                const int a = edge_row(e), b = e - tri2(a);
                                if (gn_cn<NW>(W, a, b, key[e], e)) { if (last_cnt == 0) last_e = e; ++last_cnt; }
                            }
                        }
                    }
                    de = last_e;
                    if (last_cnt == 0) fl |= TDA_GEN_NO_EDGE;
                    else if (last_cnt > 1) fl |= TDA_GEN_DEATH_TIED;
                }
                if (fl & TDA_GEN_NO_EDGE) {
                    // (lane 0 wrote the birth edge above: it takes it back itself)
                    if (lane == 0) { gen[r * 4] = gen[r * 4 + 1] = gen[r * 4 + 2] = gen[r * 4 + 3] = -1; rflag[r] = fl; clen[r] = 0; }
                    gn_store_cycle(cyc ? cyc + (size_t)r * cyc_cap : nullptr, cyc_cap, lane, 0, -1, -1);
                } else if (lane == 0) {
                    const int da = de >= 0 ? edge_row(de) : -1;
                    gen[r * 4 + 2] = (short)da;
                    gen[r * 4 + 3] = (short)(de >= 0 ? de - tri2(da) : -1);
                    rflag[r] |= fl;                                  // (this lane wrote the truncation bit above)
                }
            }
        }
        r0 = r1;
    }

    if (h0e) {
        const double* h0 = io.h0 + (size_t)win * h0_cap * 2;
        for (int r0 = 0; r0 < R0;) {
            const double dv = h0[2 * r0 + 1];
            int r1 = r0 + 1;
            while (r1 < R0 && h0[2 * r1 + 1] == dv) ++r1;
            if ((run++ & (GN_WAVES - 1)) == wave) {
                // the forest edges with this key in order, one per row
                int found = 0;
                for (int cb = 0; cb < W.E && dv != (double)INFINITY; cb += 64) {     // an essential row has no edge
                    u64 m = gn_match(W, cb, dv);
                    while (m && r0 + found < r1) {
                        const int e = cb + __builtin_ctzll(m);
                        m &= m - 1;
                        const int a = edge_row(e), b = e - tri2(a);
                        const float ke = key[e];
                        if (gn_cn<NW>(W, a, b, ke, e)) continue;
                        int walk[NW];
                        ++searches;
                        if (gn_search<NW>(W, a, b, ke, e, walk, levels) != 0) continue;
                        if (lane == 0) { h0e[2 * (r0 + found)] = (short)a; h0e[2 * (r0 + found) + 1] = (short)b; }
                        ++found;
                    }
                }
                if (lane == 0) for (int r = r0 + found; r < r1; ++r) { h0e[2 * r] = -1; h0e[2 * r + 1] = -1; }
            }
            r0 = r1;
        }
    }
    if (io.work && lane == 0) {
        io.work[(size_t)win * 2 * GN_WAVES + 2 * wave] = searches;
        io.work[(size_t)win * 2 * GN_WAVES + 2 * wave + 1] = levels;
    }
    if (!part) return;

    // the rows of the other waves: one barrier, then thread v reads what they wrote
    __threadfence_block();
    __syncthreads();
    for (int v = tid; v < io.part_ld; v += GN_NT) {
        double s = 0.0;
        if (v < n) {
            for (int r = 0; r < R1; ++r) {
                const double b = h1[2 * r], d = h1[2 * r + 1];
                if (rflag[r] != 0 || !(fabs(d) < (double)INFINITY)) continue;
                const short* row = cyc + (size_t)r * cyc_cap;
                const int len = clen[r];
                bool on = false;
                for (int j = 0; j < len; ++j) on |= row[j] == (short)v;
                if (on) s += d - b;
            }
        }
        part[v] = s;
    }
}

tda_status gn_check(tda_ctx* ctx, const GenArgs& g)
{
    if (g.cyc_cap < 4 || g.cyc_cap > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "cyc_cap must be in [4, TDA_MAX_POINTS]");
    if (g.h1_cap < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "h1_cap must be >= 1");
    if (g.part && !g.cyc) TDA_FAIL(ctx, TDA_ERR_INVALID, "part is summed over the cycles: it needs cyc");
    if (g.h0_edge && (!g.h0 || !g.h0_cnt || g.h0_cap < 1))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "h0_edge needs the H0 rows: h0, h0_cnt and h0_cap >= 1");
    return TDA_OK;
}

tda_status launch_generators(tda_ctx* ctx, const WinSrc& src, int n_win, double thresh, const GenArgs& g, int* n_points,
                             int* status, hipStream_t st)
{
    TDA_TRY(gn_check(ctx, g));
    WinSrc s = src;
    int n_max;
    TDA_TRY(win_src_limits(ctx, s.mode, s.n_in, s.dim, s.subsample, &s, &n_max));
    if (n_win == 0) return TDA_OK;
    GenArgs io = g;
    io.part_ld = s.mode == 0 ? TDA_MAX_POINTS : s.n_in;              // the columns of part: whatever tau gives, p_cap, n
    const KeyLayout L = key_layout(n_max, s.dim);
    if (n_max <= 64)
        hipLaunchKernelGGL(generators_kernel<1>, dim3(n_win), dim3(GN_NT), L.total, st, s, (float)thresh, L, io, n_points, status);
    else
        hipLaunchKernelGGL(generators_kernel<2>, dim3(n_win), dim3(GN_NT), L.total, st, s, (float)thresh, L, io, n_points, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_generators_mean(tda_ctx* ctx, const double* part, int n_win, int n, const int* seg_off, int n_seg,
                                  const int* status_in, int skip_mask, double* mean, hipStream_t st)
{
    if (n < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be >= 1");
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    const long long total = (long long)n_seg * n;
    hipLaunchKernelGGL((group_mean_kernel<double, double>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, n_win, n,
                       seg_off, n_seg, status_in, skip_mask, mean);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
