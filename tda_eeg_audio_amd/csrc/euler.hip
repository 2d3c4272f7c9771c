// euler.hip -- simplex counts f_0 .. f_K and the Euler characteristic of the Vietoris-Rips complex of a window on a grid
// of scales, K <= TDA_EC_MAX_DIM = 3, and their per-group means (include/tdaeeg.h, "Euler characteristic curves";
// DESIGN.md 3.21).  Integers: the output is the bits of tests/euler_ref.py or it is wrong.
//
// One workgroup of 256 threads (four waves) per window.
//   Keys.   The float32 keys k[a][b], a > b, are computed once per window into an LDS triangle (4 * n (n - 1) / 2 bytes:
//           32.5 KB at 128 points, 4.3 KB at 47), by the rules of the Rips kernels for the same input: the symmetrised
//           distance matrix of rips_dm_window, or the Takens / min-max / sklearn distance of rips_cloud_window and
//           KeyFromPtsTab, restated here operation for operation (csrc/rips.hip is not touched; tests/test_gpu_euler.py
//           pins the restatement to the oracle).  Two workgroup barriers, both before the grid loop.
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
// adds their int32 values in int64; (double)S / (double)m, NaN for m = 0.
#include "common.h"

#define EC_NT 256
#define EC_WAVES (EC_NT / 64)

__device__ __forceinline__ int ec_tri(int a) { return a * (a - 1) / 2; }

// e -> the row a of the triangle that holds it: tri(a) <= e < tri(a) + a.  e < 8128: the float root is within one row.
__device__ __forceinline__ int ec_edge_row(int e)
{
    int a = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)e)) * 0.5f);
    if (ec_tri(a) > e) --a;
    if (ec_tri(a + 1) <= e) ++a;
    return a;
}

__device__ __forceinline__ u32 ec_wave_sum(u32 v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (u32)__shfl_xor((int)v, m, 64);
    return v;
}

struct EcLayout {
    int off_masks, off_pts, off_nrm, off_mm, total;     // bytes; the keys are at 0
};

static EcLayout ec_layout(int n_max, int nw, int dim)
{
    EcLayout L;
    int o = (n_max * (n_max - 1) / 2 * 4 + 15) & ~15;
    L.off_masks = o; o += EC_WAVES * n_max * nw * 8;
    L.off_pts = o;   o += n_max * dim * 8;
    L.off_nrm = o;   o += n_max * 8;
    L.off_mm = o;    o += 2 * TDA_MAX_DIM * 8;
    L.total = o;
    return L;
}

// mode 0: Takens windows (src (n_win, n_t), aux = tau);  mode 1: clouds (src (n_win, p_cap, dim), aux = n_pts);
// mode 2: distance matrices (src (n_win, n, n), aux unused, n_in = n, `flag` = symmetrise; in modes 0 / 1 `flag` = normalise)
template <int NW>
__global__ void __launch_bounds__(EC_NT)
euler_kernel(const double* __restrict__ src, const int* __restrict__ aux, int n_in, int dim, int subsample, int mode,
             int flag, float thresh, int p_lim, EcLayout L, const double* __restrict__ grid, int n_grid, int max_dim,
             int* __restrict__ counts, int* __restrict__ n_points, int* __restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* key = reinterpret_cast<float*>(smem);
    const int win = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* out = counts + (size_t)win * (max_dim + 2) * n_grid;

    int n;
    if (mode == 2) {
        n = n_in;
        const double* D = src + (size_t)win * n * n;
        // utils.py:137-139 then ripser's float32 cast, as rips_dm_window
        for (int i = tid; i < n * n; i += EC_NT) {
            const int a = i / n, b = i - a * n;
            if (b < a) {
                double v;
                if (flag) {
                    v = (D[(size_t)a * n + b] + D[(size_t)b * n + a]) / 2.0;
                    if (v < 0.0) v = 0.0;
                } else {
                    v = D[(size_t)b * n + a];
                }
                key[ec_tri(a) + b] = (float)v;
            }
        }
        if (tid == 0) status[win] = 0;
    } else {
        // P exactly as rips_cloud_window counts it (in 64 bits: tau is the caller's)
        long long P64;
        const double* base;
        int tau = 1;
        if (mode == 0) {
            tau = aux[win];
            const long long nn = (long long)n_in - (long long)(dim - 1) * tau;
            P64 = nn > 0 ? (nn + subsample - 1) / subsample : 0;
            base = src + (size_t)win * n_in;
        } else {
            P64 = aux[win];
            base = src + (size_t)win * n_in * dim;
        }
        if (n_points && tid == 0) n_points[win] = P64 > 0x7fffffffll ? 0x7fffffff : (int)P64;
        const bool too_large = P64 > p_lim || (mode == 0 && tau < 1);
        if (too_large || P64 < 3) {
            for (int i = tid; i < (max_dim + 2) * n_grid; i += EC_NT) out[i] = 0;
            if (tid == 0) status[win] = too_large ? TDA_WIN_TOO_LARGE : TDA_WIN_DEGENERATE;
            return;
        }
        n = (int)P64;
        double* pts = reinterpret_cast<double*>(smem + L.off_pts);
        double* nrm = reinterpret_cast<double*>(smem + L.off_nrm);
        double* mm = reinterpret_cast<double*>(smem + L.off_mm);
        for (int idx = tid; idx < n * dim; idx += EC_NT) {
            const int i = idx / dim, k = idx - i * dim;
            pts[idx] = (mode == 0) ? base[(size_t)i * subsample + (size_t)k * tau] : base[idx];
        }
        __syncthreads();
        if (flag) {
            // per-column min-max over the whole cloud (range 0 -> 1), utils.py:127-130: one wave per column
            if (wave < dim) {
                double mn = INFINITY, mx = -INFINITY;
                for (int i = lane; i < n; i += 64) {
                    const double v = pts[i * dim + wave];
                    mn = v < mn ? v : mn;
                    mx = v > mx ? v : mx;
                }
                mn = wave_min_f64_dpp(mn);
                mx = wave_max_f64_dpp(mx);
                if (lane == 0) { double rg = mx - mn; if (rg == 0.0) rg = 1.0; mm[2 * wave] = mn; mm[2 * wave + 1] = rg; }
            }
            __syncthreads();
            for (int idx = tid; idx < n * dim; idx += EC_NT) {
                const int k = idx % dim;
                pts[idx] = (pts[idx] - mm[2 * k]) / mm[2 * k + 1];
            }
            __syncthreads();
        }
        if (tid < n) {
            double s = 0.0;
            for (int k = 0; k < dim; ++k) s += pts[tid * dim + k] * pts[tid * dim + k];
            nrm[tid] = s;
        }
        __syncthreads();
        // sklearn euclidean_distances: -2 x.y + |x|^2 + |y|^2, clamp, sqrt, float32 -- KeyFromPtsTab of csrc/rips.hip
        const int E = ec_tri(n);
        for (int e = tid; e < E; e += EC_NT) {
            const int a = ec_edge_row(e), b = e - ec_tri(a);
            double dot = pts[a * dim] * pts[b * dim];
            for (int k = 1; k < dim; ++k) dot = fma(pts[a * dim + k], pts[b * dim + k], dot);
            double d2 = -2.0 * dot;
            d2 += nrm[a];
            d2 += nrm[b];
            if (!(d2 > 0.0)) d2 = 0.0;
            key[e] = (float)sqrt_rn(d2);
        }
        if (tid == 0) status[win] = 0;
    }
    __syncthreads();

    u64* Lm = reinterpret_cast<u64*>(smem + L.off_masks) + (size_t)wave * n * NW;      // this wave's masks: L[v][NW]
    const int E = ec_tri(n);
    u32 prev_f1 = 0, prev_f2 = 0, prev_f3 = 0;
    for (int g = wave; g < n_grid; g += EC_WAVES) {
        const double t = grid[g];
        // a. lower adjacency masks of this grid point; lane v owns vertices v, v + 64
        u32 f1 = 0, f2 = 0, f3 = 0;
        for (int v = lane; v < n; v += 64) {
            const float* row = key + ec_tri(v);
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
                const int a = ec_edge_row(e), b = e - ec_tri(a);
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

__global__ void __launch_bounds__(256)
euler_mean_kernel(const int* __restrict__ counts, int n_win, int rows_grid, const int* __restrict__ seg_off, int n_seg,
                  const int* __restrict__ status_in, int skip_mask, double* __restrict__ mean)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_seg * rows_grid) return;
    const int g = (int)(idx / rows_grid), j = (int)(idx - (long long)g * rows_grid);
    int w0 = g, w1 = g + 1;                                          // seg_off == NULL: every window its own group
    if (seg_off) { w0 = seg_off[g]; w1 = seg_off[g + 1]; }
    w0 = w0 < 0 ? 0 : w0; w1 = w1 > n_win ? n_win : w1;
    long long S = 0;
    int m = 0;
    for (int w = w0; w < w1; ++w) {
        if (status_in && (status_in[w] & skip_mask)) continue;
        S += counts[(size_t)w * rows_grid + j];
        ++m;
    }
    mean[idx] = m ? (double)S / (double)m : __longlong_as_double(0x7ff8000000000000ll);
}

static tda_status ec_check(tda_ctx* ctx, int n_grid, int max_dim)
{
    if (n_grid < 1 || n_grid > TDA_MAX_GRID) TDA_FAIL(ctx, TDA_ERR_INVALID, "n_grid must be in [1, TDA_MAX_GRID]");
    if (max_dim < 1 || max_dim > TDA_EC_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "max_dim must be in [1, TDA_EC_MAX_DIM]");
    return TDA_OK;
}

// mode 2 (distance matrices): n_in = n, flag = symmetrise, aux = NULL.  mode 0 / 1: as launch_rips_cloud, flag = normalise.
tda_status launch_euler(tda_ctx* ctx, const double* src, const int* aux, int n_win, int n_in, int dim, int subsample,
                        int mode, int flag, double thresh, const double* grid, int n_grid, int max_dim, int* counts,
                        int* n_points, int* status, hipStream_t st)
{
    const tda_status rc = ec_check(ctx, n_grid, max_dim);
    if (rc != TDA_OK) return rc;
    // n_max sizes the LDS layout; p_lim is the largest cloud a window may have (never more than its buffer holds)
    int n_max, p_lim = TDA_MAX_POINTS;
    if (mode == 2) {
        if (n_in < 1 || n_in > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [1, TDA_MAX_POINTS]");
        n_max = n_in; dim = 0; subsample = 1;
    } else {
        if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
        if (n_in < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, mode == 0 ? "n_t must be >= 1" : "p_cap must be >= 1");
        if (subsample < 1) subsample = 1;
        if (mode == 0) {
            // tau >= 1 in the reference (utils.py:103-104); P is largest at tau = 1
            const int nn = n_in - (dim - 1);
            n_max = nn > 0 ? (nn + subsample - 1) / subsample : 0;
        } else {
            n_max = n_in;
            if (n_in < p_lim) p_lim = n_in;
        }
        if (n_max > TDA_MAX_POINTS) n_max = TDA_MAX_POINTS;          // larger clouds are flagged per window
        if (n_max < 3) n_max = 3;
    }
    if (n_win == 0) return TDA_OK;
    const int nw = n_max > 64 ? 2 : 1;
    const EcLayout L = ec_layout(n_max, nw, dim);
    if (nw == 1)
        hipLaunchKernelGGL(euler_kernel<1>, dim3(n_win), dim3(EC_NT), L.total, st, src, aux, n_in, dim, subsample, mode, flag,
                           (float)thresh, p_lim, L, grid, n_grid, max_dim, counts, n_points, status);
    else
        hipLaunchKernelGGL(euler_kernel<2>, dim3(n_win), dim3(EC_NT), L.total, st, src, aux, n_in, dim, subsample, mode, flag,
                           (float)thresh, p_lim, L, grid, n_grid, max_dim, counts, n_points, status);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}

tda_status launch_euler_mean(tda_ctx* ctx, const int* counts, int n_win, int max_dim, int n_grid, const int* seg_off,
                             int n_seg, const int* status_in, int skip_mask, double* mean, hipStream_t st)
{
    const tda_status rc = ec_check(ctx, n_grid, max_dim);
    if (rc != TDA_OK) return rc;
    if (!seg_off && n_seg != n_win) TDA_FAIL(ctx, TDA_ERR_INVALID, "without seg_off every window is a group: n_seg != n_win");
    if (n_seg == 0) return TDA_OK;
    const int rows_grid = (max_dim + 2) * n_grid;
    const long long total = (long long)n_seg * rows_grid;
    hipLaunchKernelGGL(euler_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, n_win, rows_grid,
                       seg_off, n_seg, status_in, skip_mask, mean);
    TDA_HIP(ctx, hipGetLastError());
    return TDA_OK;
}
