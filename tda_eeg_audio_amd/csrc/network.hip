// network.hip -- the conventional graph measures of the thresholded graph G_g of a window on a grid of scales: degree,
// triangles, clustering and transitivity, hop distances (characteristic path length, global efficiency, diameter), the
// components, and their per-group means (include/tdaeeg.h, "Network curves").  The integers are the bits
// of tests/network_ref.py or they are wrong; the four float64 measures are written functions of those integers in one
// written order of IEEE operations.
//
// One workgroup of 256 threads (four waves) per window, as csrc/euler.hip.
//   Keys.   window_keys of csrc/rips_keys_dev.h fills the LDS triangle; its workgroup barriers all come before the grid loop.
//   Grid.   A wave per grid point: wave w takes the grid points w, w + 4, ...  Nothing inside the grid loop waits for
//           another wave.  Lane v owns vertex v (and v + 64 above 64 points), as a vertex and as a search source.
//     a.    The FULL adjacency masks A[v] = { u != v : the edge {u, v} is present }, one u64 per 64 vertices, in the wave's
//           own slice of LDS: lane v reads row v of the triangle for u < v and key[tri2(u) + v] for u > v.  deg = popc.
//     b.    tri(v) = (sum over u in A[v] of popc(A[v] & A[u])) / 2.
//     c.    Hop distances by breadth-first search in lockstep: every lane keeps `visited` and `frontier` of its sources in
//           registers; at level d, next = (OR over u in frontier of A[u]) & ~visited.  popc(next) feeds reach, farness and
//           eccentricity of that source; summed over the wave and halved it is p_d, the unordered pairs at hop distance d,
//           which feeds pairs, hops, diameter and the running efficiency sum in ascending d.  The level loop is bounded by
//           n - 1 and ends when no source of the wave found a new vertex.  A source that has visited all n vertices drops
//           its frontier (its next level would be empty).
//     d.    Components: source s represents its component when s is the lowest bit of its final `visited`.
//     e.    Clustering: the quotients c_v go to the wave's LDS scratch; every lane adds them in ascending v.
//     f.    The edge sets of two grid points are nested, so a wave whose edge count equals that of its previous grid point
//           has the same graph in hand and keeps that grid point's results (they live in registers).
//   Loop bounds, all known before the loop starts: n, n_grid, n_node, n - 1 levels, a popcount.  No polls, no atomics,
//   nothing is allocated.
// What diverges: the loops over the set bits of A[v] (b) and of a frontier (c) run as long as the lane with the most bits;
// DESIGN.md 3.24 says what that costs.
//
// The group means are up to three launches of group_mean_kernel (common.h): int32 in int64 for counts and nodal, float64
// added in window order for measures.
#include "common.h"
#include "rips_keys_dev.h"

#define NT_NT 256
#define NT_WAVES (NT_NT / 64)

__device__ __forceinline__ u32 nt_wave_sum(u32 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (u32)__shfl_xor((int)v, m, 64);
    return v;
}
__device__ __forceinline__ u32 nt_wave_max(u32 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const u32 o = (u32)__shfl_xor((int)v, m, 64); v = o > v ? o : v; }
    return v;
}

// `off_masks`, `off_quot`: the byte offsets of the waves' mask slices and quotient scratch, behind the LDS of the key pass
template <int NW>
__global__ void __launch_bounds__(NT_NT)
network_kernel(WinSrc src, float thresh, KeyLayout L, int off_masks, int off_quot, const double* __restrict__ grid, int n_grid,
               int n_node, int* __restrict__ counts, double* __restrict__ measures, int* __restrict__ nodal,
               int* __restrict__ n_points, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float* key = reinterpret_cast<const float*>(smem);
    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* cnt_out = counts + (size_t)win * TDA_NET_ROWS * n_grid;
    double* mea_out = measures + (size_t)win * TDA_NET_MEASURES * n_grid;
    const size_t nodal_len = (size_t)TDA_NET_NODAL * n_grid * n_node;
    int* nod_out = nodal ? nodal + (size_t)win * nodal_len : nullptr;

    const WinExtent X = win_extent(src, win);
    const int st = win_status(src, X, win, n_points);
    if (tid == 0) status[win] = st;
    if (st) {
        for (int i = tid; i < TDA_NET_ROWS * n_grid; i += NT_NT) cnt_out[i] = 0;
        for (int i = tid; i < TDA_NET_MEASURES * n_grid; i += NT_NT) mea_out[i] = 0.0;
        if (nod_out)
            for (size_t i = tid; i < nodal_len; i += NT_NT) nod_out[i] = 0;
        return;
    }
    const int n = (int)X.P;
    window_keys<NT_NT>(src, X, n, smem, L);

    u64* Am = reinterpret_cast<u64*>(smem + off_masks) + (size_t)wave * n * NW;         // this wave's masks: A[v][NW]
    double* quot = reinterpret_cast<double*>(smem + off_quot) + (size_t)wave * n;       // this wave's c_v
    // what a grid point leaves behind; the per-vertex values of this lane's vertices lane + 64 j
    u32 deg[NW], tri[NW], reach[NW], far[NW], ecc[NW];
    u32 edges = 0, isolated = 0, max_deg = 0, wedges = 0, tri3 = 0, comps = 0, largest = 0, pairs = 0, hops = 0, diam = 0;
    double clus = 0.0, eff = 0.0;
    u32 prev_edges = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j) deg[j] = tri[j] = reach[j] = far[j] = ecc[j] = 0;

    for (int g = wave; g < n_grid; g += NT_WAVES) {
        const double t = grid[g];
        // a. full adjacency masks of this grid point
        u32 dsum = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int v = lane + 64 * j;
            deg[j] = 0;
            if (v < n) {
                const float* row = key + tri2(v);
                u64 m[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w) m[w] = 0ull;
                for (int u = 0; u < n; ++u) {
                    if (u == v) continue;
                    const float k = u < v ? row[u] : key[tri2(u) + v];
                    const bool in = k <= thresh && (double)k <= t;
                    if (NW == 1) m[0] |= (u64)in << u;
                    else m[u >> 6] |= (u64)in << (u & 63);
                }
#pragma unroll
                for (int w = 0; w < NW; ++w) { Am[v * NW + w] = m[w]; deg[j] += (u32)__popcll(m[w]); }
            }
            dsum += deg[j];
        }
        // the masks are read by other lanes of this wave only
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        edges = nt_wave_sum(dsum) >> 1;
        // f. nested edge sets ({k <= min(t, thresh)}): equal edge counts mean equal graphs, the previous results stand
        const bool again = g != wave && edges == prev_edges;
        prev_edges = edges;
        if (!again) {
            // b. triangles at every vertex; degree statistics
            u32 iso = 0, mx = 0, wed = 0, tsum = 0;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int v = lane + 64 * j;
                tri[j] = 0;
                if (v < n) {
                    u64 Av[NW];
#pragma unroll
                    for (int w = 0; w < NW; ++w) Av[w] = Am[v * NW + w];
                    u32 s = 0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        u64 f = Av[w];
                        while (f) {
                            const int bit = __builtin_ctzll(f);
                            f &= f - 1;
                            const u64* Au = Am + (w * 64 + bit) * NW;
#pragma unroll
                            for (int x = 0; x < NW; ++x) s += (u32)__popcll(Av[x] & Au[x]);
                        }
                    }
                    tri[j] = s >> 1;
                    iso += deg[j] == 0;
                    mx = deg[j] > mx ? deg[j] : mx;
                    wed += (deg[j] * (deg[j] - 1)) >> 1;
                }
                tsum += tri[j];
            }
            isolated = nt_wave_sum(iso);
            max_deg = nt_wave_max(mx);
            wedges = nt_wave_sum(wed);
            tri3 = nt_wave_sum(tsum);                                        // 3 * triangles
            // e. clustering: quotients in parallel, the sum in ascending v
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int v = lane + 64 * j;
                if (v < n) quot[v] = deg[j] < 2 ? 0.0 : (double)tri[j] / (double)((deg[j] * (deg[j] - 1)) >> 1);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            double S = 0.0;
            for (int v = 0; v < n; ++v) S += quot[v];
            clus = S / (double)n;
            // c. hop distances: lockstep breadth-first search, a source per owned vertex
            u64 vis[NW][NW], fr[NW][NW];
            u32 seen[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int s = lane + 64 * j;
#pragma unroll
                for (int w = 0; w < NW; ++w) vis[j][w] = fr[j][w] = (s < n && (s >> 6) == w) ? 1ull << (s & 63) : 0ull;
                seen[j] = s < n ? 1u : 0u;
                reach[j] = far[j] = ecc[j] = 0;
            }
            pairs = hops = diam = 0;
            double E = 0.0;
            for (int d = 1; d < n; ++d) {
                u32 found = 0;
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    u64 nx[NW];
#pragma unroll
                    for (int x = 0; x < NW; ++x) nx[x] = 0ull;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        u64 f = fr[j][w];
                        while (f) {
                            const int bit = __builtin_ctzll(f);
                            f &= f - 1;
                            const u64* Au = Am + (w * 64 + bit) * NW;
#pragma unroll
                            for (int x = 0; x < NW; ++x) nx[x] |= Au[x];
                        }
                    }
                    u32 c = 0;
#pragma unroll
                    for (int x = 0; x < NW; ++x) {
                        nx[x] &= ~vis[j][x];
                        vis[j][x] |= nx[x];
                        c += (u32)__popcll(nx[x]);
                    }
                    seen[j] += c;
                    reach[j] += c;
                    far[j] += (u32)d * c;
                    ecc[j] = c ? (u32)d : ecc[j];
                    // a source that has seen every vertex has no next level
                    const bool full = seen[j] == (u32)n;
#pragma unroll
                    for (int x = 0; x < NW; ++x) fr[j][x] = full ? 0ull : nx[x];
                    found += c;
                }
                const u32 pd = nt_wave_sum(found) >> 1;
                if (pd == 0) break;
                pairs += pd;
                hops += (u32)d * pd;
                diam = (u32)d;
                E += (double)pd / (double)d;
            }
            eff = n < 2 ? 0.0 : E / (double)tri2(n);
            // d. components: the source that is the lowest bit of its own visited set represents it
            u32 rep = 0, big = 0;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int s = lane + 64 * j;
                if (s < n) {
                    int low = 0;
                    if (NW == 1) low = __builtin_ctzll(vis[j][0]);
                    else low = vis[j][0] ? __builtin_ctzll(vis[j][0]) : 64 + __builtin_ctzll(vis[j][NW - 1]);
                    rep += low == s;
                    big = seen[j] > big ? seen[j] : big;
                }
            }
            comps = nt_wave_sum(rep);
            largest = nt_wave_max(big);
        }
        if (lane == 0) {
            const u32 triangles = tri3 / 3u;
            cnt_out[0 * n_grid + g] = (int)edges;
            cnt_out[1 * n_grid + g] = (int)isolated;
            cnt_out[2 * n_grid + g] = (int)max_deg;
            cnt_out[3 * n_grid + g] = (int)wedges;
            cnt_out[4 * n_grid + g] = (int)triangles;
            cnt_out[5 * n_grid + g] = (int)comps;
            cnt_out[6 * n_grid + g] = (int)largest;
            cnt_out[7 * n_grid + g] = (int)pairs;
            cnt_out[8 * n_grid + g] = (int)hops;
            cnt_out[9 * n_grid + g] = (int)diam;
            mea_out[0 * n_grid + g] = wedges ? (double)(3u * triangles) / (double)wedges : 0.0;
            mea_out[1 * n_grid + g] = clus;
            mea_out[2 * n_grid + g] = eff;
            mea_out[3 * n_grid + g] = pairs ? (double)hops / (double)pairs : 0.0;
        }
        if (nod_out) {
            for (int v = lane; v < n_node; v += 64) {
                u32 r[TDA_NET_NODAL] = {0, 0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < NW; ++j)
                    if (v == lane + 64 * j && v < n) { r[0] = deg[j]; r[1] = tri[j]; r[2] = reach[j]; r[3] = far[j]; r[4] = ecc[j]; }
#pragma unroll
                for (int q = 0; q < TDA_NET_NODAL; ++q) nod_out[((size_t)q * n_grid + g) * n_node + v] = (int)r[q];
            }
        }
        // the next grid point overwrites the masks and the quotients: every lane has finished reading them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

tda_status nt_check(tda_ctx* ctx, int n_grid)
{
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]");
    return TDA_OK;
}

tda_status launch_network(tda_ctx* ctx, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid,
                          int* counts, double* measures, int* nodal, int* n_points, int* status, hipStream_t st)
{
    TDA_TRY(nt_check(ctx, n_grid));
    WinSrc s = src;
    int n_max;
    TDA_TRY(win_src_limits(ctx, s.mode, s.n_in, s.dim, s.subsample, &s, &n_max));
    if (n_win == 0) return TDA_OK;
    // the columns of nodal: the `part` convention of the generators
    const int n_node = s.mode == 2 ? s.n_in : s.mode == 1 ? s.n_in : TDA_MAX_POINTS;
    const KeyLayout L = key_layout(n_max, s.dim);
    const int nw = n_max > 64 ? 2 : 1;
    const int off_masks = L.total, off_quot = off_masks + NT_WAVES * n_max * nw * 8, lds = off_quot + NT_WAVES * n_max * 8;
    if (nw == 1)
        hipLaunchKernelGGL(network_kernel<1>, dim3(n_win), dim3(NT_NT), lds, st, s, (float)thresh, L, off_masks, off_quot, grid,
                           n_grid, n_node, counts, measures, nodal, n_points, status);
    else
        hipLaunchKernelGGL(network_kernel<2>, dim3(n_win), dim3(NT_NT), lds, st, s, (float)thresh, L, off_masks, off_quot, grid,
                           n_grid, n_node, counts, measures, nodal, n_points, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status nt_mean_check(tda_ctx* ctx, const void* counts, const void* measures, const void* nodal, int n_win, int n_grid,
                         int n_node, const int* seg_off, int n_seg, const void* mean_counts, const void* mean_measures,
                         const void* mean_nodal)
{
    TDA_TRY(nt_check(ctx, n_grid));
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg && n_win &&
        ((counts == nullptr) != (mean_counts == nullptr) || (measures == nullptr) != (mean_measures == nullptr) ||
         (nodal == nullptr) != (mean_nodal == nullptr)))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "counts, measures and nodal are each nullable together with their mean");
    if ((nodal || mean_nodal) && (n_node < 1 || (long long)TDA_NET_NODAL * n_grid * n_node > 0x7fffffffll))
        TDA_FAIL(ctx, TDA_ERR_INVALID, "n_node must be >= 1 and TDA_NET_NODAL * n_grid * n_node must fit an int");
    return TDA_OK;
}

tda_status launch_network_mean(tda_ctx* ctx, const int* counts, const double* measures, const int* nodal, int n_win, int n_grid,
                               int n_node, const int* seg_off, int n_seg, const int* status_in, int skip_mask,
                               double* mean_counts, double* mean_measures, double* mean_nodal, hipStream_t st)
{
    TDA_TRY(nt_mean_check(ctx, counts, measures, nodal, n_win, n_grid, n_node, seg_off, n_seg, mean_counts, mean_measures,
                          mean_nodal));
    if (n_seg == 0) return TDA_OK;
    const auto blocks = [&](int row_len) { return dim3((unsigned)(((long long)n_seg * row_len + 255) / 256)); };
    if (mean_counts) {
        const int rl = TDA_NET_ROWS * n_grid;
        hipLaunchKernelGGL((group_mean_kernel<int, long long>), blocks(rl), dim3(256), 0, st, counts, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_counts);
        TDA_HIP(ctx, hipGetLastError());
    }
    if (mean_measures) {
        const int rl = TDA_NET_MEASURES * n_grid;
        hipLaunchKernelGGL((group_mean_kernel<double, double>), blocks(rl), dim3(256), 0, st, measures, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_measures);
        TDA_HIP(ctx, hipGetLastError());
    }
    if (mean_nodal) {
        const int rl = TDA_NET_NODAL * n_grid * n_node;
        hipLaunchKernelGGL((group_mean_kernel<int, long long>), blocks(rl), dim3(256), 0, st, nodal, n_win, rl, seg_off, n_seg,
                           status_in, skip_mask, mean_nodal);
        TDA_HIP(ctx, hipGetLastError());
    }
    return TDA_OK;
}
