// euler.hip -- simplex counts f_0 .. f_K and the Euler characteristic of the Vietoris-Rips complex of a window on a grid
// of scales, K <= TDA_EC_MAX_DIM = 3, and their per-group means (include/tdaeeg.h, "Euler characteristic curves";
// DESIGN.md 3.21).  Integers: the output is the bits of tests/euler_ref.py or it is wrong.
//
// One workgroup of 256 threads (four waves) per window.
//   Keys.   The float32 keys k[a][b], a > b, are computed once per window into an LDS triangle (4 * n (n - 1) / 2 bytes:
//           32.5 KB at 128 points, 4.3 KB at 47) by window_keys of csrc/rips_keys_dev.h, the one statement of the key rules
//           of the Rips kernels: the symmetrised distance matrix, or the Takens / min-max / sklearn distance of a cloud
//           (tests/test_gpu_euler.py pins them to the oracle).  Its workgroup barriers all come before the grid loop.
//   Grid.   A wave per grid point: wave w takes the grid points w, w + 4, ...  Nothing inside the grid loop waits for
//           another wave.  For its grid point t the wave builds, in its own slice of LDS, the lower adjacency masks
//               L[v] = { u < v : k[v][u] <= (float)thresh and (double)k[v][u] <= t }          one u64 per 64 vertices
//           (lane v reads row v of the triangle), and then its lanes run over the edge indices e = lane, lane + 64, ...
//           < n (n - 1) / 2, e -> (a, b), a > b.  For an edge that is present (bit b of L[a]):
//               C = L[a] & L[b]                         the common neighbours below b;   f_2 += popc(C)
//               for every c in C, highest first:        C loses bit c, so it holds the members below c;
//                                                       f_3 += popc(C & L[c])
//           Every simplex is counted once, as a > b > c > d, because every mask holds lower neighbours only.
//           f_1 = sum_v popc(L[v]).  The lane sums are added over the wave by shuffles; lane 0 stores the column.
//           The edge sets of two grid points are nested, so a wave whose f_1 equals that of its previous grid point has
//           the same complex in hand and keeps that grid point's counts.
//   Loop bounds, all known before the loop starts: n, n_grid, the number of edge slots of a lane, a popcount.  No polls,
//   no atomics, nothing is allocated; the integers do not depend on the order of any sum.
// The inner `c` loop diverges across the lanes of a wave (a lane with few common neighbours waits for the one with
// most); it is not balanced here (DESIGN.md 3.21 says what that costs).
//
// The group means are a second small launch: one thread per (group, row, grid point) walks the windows of its group and
// adds their int32 values in int64; (double)S / (double)m, NaN for m = 0 (group_mean_kernel of common.h).
#include "common.h"
#include "rips_keys_dev.h"

#define EC_NT 256
#define EC_WAVES (EC_NT / 64)

__device__ __forceinline__ u32 ec_wave_sum(u32 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (u32)__shfl_xor((int)v, m, 64);
    return v;
}

// `off_masks`: the byte offset of the waves' mask slices, behind the LDS of the key pass
template <int NW>
__global__ void __launch_bounds__(EC_NT)
euler_kernel(WinSrc src, float thresh, KeyLayout L, int off_masks, const double* __restrict__ grid, int n_grid, int max_dim,
             int* __restrict__ counts, int* __restrict__ n_points, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const float* key = reinterpret_cast<const float*>(smem);
    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* out = counts + (size_t)win * (max_dim + 2) * n_grid;

    const WinExtent X = win_extent(src, win);
    const int st = win_status(src, X, win, n_points);
    if (tid == 0) status[win] = st;
    if (st) {
        for (int i = tid; i < (max_dim + 2) * n_grid; i += EC_NT) out[i] = 0;
        return;
    }
    const int n = (int)X.P;
    window_keys<EC_NT>(src, X, n, smem, L);

    u64* Lm = reinterpret_cast<u64*>(smem + off_masks) + (size_t)wave * n * NW;      // this wave's masks: L[v][NW]
    const int E = tri2(n);
    u32 prev_f1 = 0, prev_f2 = 0, prev_f3 = 0;
    for (int g = wave; g < n_grid; g += EC_WAVES) {
        const double t = grid[g];
        // a. lower adjacency masks of this grid point; lane v owns vertices v, v + 64
        u32 f1 = 0, f2 = 0, f3 = 0;
        for (int v = lane; v < n; v += 64) {
            const float* row = key + tri2(v);
            u64 m[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) m[w] = 0ull;
            for (int u = 0; u < v; ++u) {
                const float k = row[u];
                const bool in = k <= thresh && (double)k <= t;
                if (NW == 1) m[0] |= (u64)in << u;
                else m[u >> 6] |= (u64)in << (u & 63);
            }
#pragma unroll
            for (int w = 0; w < NW; ++w) { Lm[v * NW + w] = m[w]; f1 += (u32)__popcll(m[w]); }
        }
        // the masks are read by other lanes of this wave only
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        // The edge sets of two grid points are nested ({k <= min(t, thresh)}), so equal edge counts mean equal complexes:
        // the counts of the wave's previous grid point stand (every scale past the largest key, for one)
        f1 = ec_wave_sum(f1);
        const bool again = g != wave && f1 == prev_f1;
        // b. triangles and tetrahedra, counted at their edge a > b
        if (max_dim >= 2 && !again) {
            for (int e = lane; e < E; e += 64) {
                const int a = edge_row(e), b = e - tri2(a);
                u64 C[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w) C[w] = Lm[a * NW + w];
                const bool present = (C[NW == 1 ? 0 : (b >> 6)] >> (b & 63)) & 1ull;
                if (!present) continue;
#pragma unroll
                for (int w = 0; w < NW; ++w) { C[w] &= Lm[b * NW + w]; f2 += (u32)__popcll(C[w]); }
                if (max_dim >= 3) {
#pragma unroll
                    for (int w = NW - 1; w >= 0; --w) {
                        u64 cw = C[w];
                        while (cw) {
                            const int bit = 63 - __clzll((long long)cw);
                            cw &= ~(1ull << bit);
                            const u64* Lc = Lm + (w * 64 + bit) * NW;
                            f3 += (u32)__popcll(cw & Lc[w]);
                            if (w == 1) f3 += (u32)__popcll(C[0] & Lc[0]);
                        }
                    }
                }
            }
        }
        if (again) {
            f2 = prev_f2; f3 = prev_f3;
        } else {
            if (max_dim >= 2) f2 = ec_wave_sum(f2);
            if (max_dim >= 3) f3 = ec_wave_sum(f3);
        }
        prev_f1 = f1; prev_f2 = f2; prev_f3 = f3;
        if (lane == 0) {
            int chi = n - (int)f1;
            out[g] = n;
            out[n_grid + g] = (int)f1;
            if (max_dim >= 2) { out[2 * n_grid + g] = (int)f2; chi += (int)f2; }
            if (max_dim >= 3) { out[3 * n_grid + g] = (int)f3; chi -= (int)f3; }
            out[(max_dim + 1) * n_grid + g] = chi;
        }
        // the next grid point overwrites the masks: every lane has finished reading them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

tda_status ec_check(tda_ctx* ctx, int n_grid, int max_dim)
{
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]");
    if (max_dim < 1 || max_dim > TDA_EC_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "max_dim must be in [1, TDA_EC_MAX_DIM]");
    return TDA_OK;
}

tda_status launch_euler(tda_ctx* ctx, const WinSrc& src, int n_win, double thresh, const double* grid, int n_grid,
                        int max_dim, int* counts, int* n_points, int* status, hipStream_t st)
{
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    WinSrc s = src;
    int n_max;
    TDA_TRY(win_src_limits(ctx, s.mode, s.n_in, s.dim, s.subsample, &s, &n_max));
    if (n_win == 0) return TDA_OK;
    const KeyLayout L = key_layout(n_max, s.dim);
    const int nw = n_max > 64 ? 2 : 1, lds = L.total + EC_WAVES * n_max * nw * 8;
    if (nw == 1)
        hipLaunchKernelGGL(euler_kernel<1>, dim3(n_win), dim3(EC_NT), lds, st, s, (float)thresh, L, L.total, grid, n_grid, max_dim,
                           counts, n_points, status);
    else
        hipLaunchKernelGGL(euler_kernel<2>, dim3(n_win), dim3(EC_NT), lds, st, s, (float)thresh, L, L.total, grid, n_grid, max_dim,
                           counts, n_points, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_euler_mean(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off,
                             int n_seg, const int* status_in, int skip_mask, double* mean, hipStream_t st)
{
    TDA_TRY(ec_check(ctx, n_grid, max_dim));
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    const int rows_grid = (max_dim + 2) * n_grid;
    const long long total = (long long)n_seg * rows_grid;
    hipLaunchKernelGGL((group_mean_kernel<int, long long>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts,
                       n_win, rows_grid, seg_off, n_seg, status_in, skip_mask, mean);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
