// rips_keys_dev.h -- the float32 edge keys of a window, stated once: which points a window has, how a pair of them gets its
// key, and where the keys lie.  Every consumer of a Rips complex reads the rules here: the Rips kernels themselves
// (csrc/rips.hip), the Euler curves (csrc/euler.hip), the generators (csrc/generators.hip), the network curves
// (csrc/network.hip), the recurrence curves (csrc/recurrence.hip) and the landmark selection (csrc/landmarks.hip, the point count only).  The keys are the bytes of the reference or they are wrong, so a rule is
// changed here or nowhere.
//
// What csrc/rips.hip still keeps to itself: the staging inside rips_cloud_window (its LDS layout is shared with the ranking
// and the sweep, its 32-bit point count is bounded by its own limits and its reductions are shuffles), KeyFromPts (keys
// recomputed inside the sweep, without the |x|^2 table), the constant edge table, and the fused EEG window kernel, whose
// keys come from a correlation matrix it never writes out.  They are tuned against register limits that this header
// does not know; they call dm_key, edge_row and KeyFromPtsTab from here.
#pragma once
#include "common.h"

// ---- the triangle: the key of {a, b}, a > b, lies at tri2(a) + b ----
__device__ __forceinline__ int tri2(int v) { return (v * (v - 1)) >> 1; }
// index of unordered pair {x,y}, x != y
__device__ __forceinline__ int pair_index(int x, int y) { return x > y ? tri2(x) + y : tri2(y) + x; }

// flat edge index e = tri2(a)+b (a > b)  ->  a
__device__ __forceinline__ int edge_row(int e)
{
    // e < 2^13: 1 + 8e is exact in float and the hardware's v_sqrt_f32 (one ulp, no denormal / class fix-ups: the
    // correctly rounded sqrtf of -fno-fast-math costs 18 instructions more, tools/probes/valu_rate.hip) puts the estimate
    // within 1e-4 of (1 + sqrt(1 + 8e)) / 2, i.e. off by at most one row -- one branch-free correction
    const int a = (int)((1.0f + __builtin_amdgcn_sqrtf(1.0f + 8.0f * (float)e)) * 0.5f);
    const int t = tri2(a);
    return a + (t + a <= e ? 1 : 0) - (t > e ? 1 : 0);
}

// ---- the key of a distance-matrix entry: utils.py:137-139 (symmetrise, clamp at 0), then ripser's float32 cast ----
__device__ __forceinline__ float dm_key(const double* __restrict__ D, int n, int a, int b, int symmetrise)
{
    double v;
    if (symmetrise) {
        v = (D[(size_t)a * n + b] + D[(size_t)b * n + a]) / 2.0;
        if (v < 0.0) v = 0.0;
    } else {
        v = D[(size_t)b * n + a];
    }
    return (float)v;
}

// ---- the key of two points of a (normalised) cloud: sklearn euclidean_distances, -2 x.y + |x|^2 + |y|^2, clamp, sqrt,
// float32, with |x|^2 of every point from a table (every point takes part in P - 1 edges; the table holds exactly the
// value KeyFromPts of csrc/rips.hip computes in place, so the keys are bit-identical) ----
struct KeyFromPtsTab {
    const double* pts; const double* nrm; int dim;
    __device__ __forceinline__ static double norm2(const double* p, int dim)
    {
        if (dim == 3) return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        double n = 0.0;
        for (int k = 0; k < dim; ++k) n += p[k] * p[k];
        return n;
    }
    __device__ __forceinline__ float operator()(int, int a, int b) const
    {
        double dot = 0.0;
        if (dim == 3) {
            const double* pa = pts + 3 * a;
            const double* pb = pts + 3 * b;
            dot = fma(pa[2], pb[2], fma(pa[1], pb[1], pa[0] * pb[0]));
        } else
        for (int k = 0; k < dim; ++k) {
            const double xa = pts[a * dim + k], xb = pts[b * dim + k];
            dot = (k == 0) ? xa * xb : fma(xa, xb, dot);
        }
        double d2 = -2.0 * dot;
        d2 += nrm[a];
        d2 += nrm[b];
        if (!(d2 > 0.0)) d2 = 0.0;
        return (float)sqrt_rn(d2);
    }
};

// ---- where the windows of a launch come from ----
//   mode 0  Takens windows: src (n_win, n_in = n_t) samples, aux = tau per window; point i of a window is
//           (x[i * subsample + k * tau])_{k < dim} (utils.py:107-116); flag = normalise (always 1 in the entry points)
//   mode 1  explicit clouds: src (n_win, n_in = p_cap, dim), aux = n_pts per window; flag = normalise
//   mode 2  distance matrices: src (n_win, n_in = n, n_in), aux unused, dim = 0, subsample = 1; flag = symmetrise
// p_lim: the most points a window may have (win_src_limits; never more than its buffer holds).
struct WinSrc {
    const double* src; const int* aux;
    int n_in, dim, subsample, mode, flag, p_lim;
};

// the points of window `win`, counted in 64 bits (tau is the caller's), its delay and its first value
struct WinExtent {
    long long P; int tau; const double* base;
};
__device__ __forceinline__ WinExtent win_extent(const WinSrc& s, int win)
{
    WinExtent x;
    x.tau = 1;
    if (s.mode == 0) {
        x.tau = s.aux[win];
        const long long nn = (long long)s.n_in - (long long)(s.dim - 1) * x.tau;
        x.P = nn > 0 ? (nn + s.subsample - 1) / s.subsample : 0;
        x.base = s.src + (size_t)win * s.n_in;
    } else if (s.mode == 1) {
        x.P = s.aux[win];
        x.base = s.src + (size_t)win * s.n_in * s.dim;
    } else {
        x.P = s.n_in;
        x.base = s.src + (size_t)win * s.n_in * s.n_in;
    }
    return x;
}

// The status word of a window and its saturated point count (n_points is optional; thread 0 writes it).  A matrix is
// never refused here: its n is a limit of the launch.  tau >= 1 in the reference (utils.py:103-104).
__device__ __forceinline__ int win_status(const WinSrc& s, const WinExtent& x, int win, int* __restrict__ n_points)
{
    if (s.mode == 2) return 0;
    if (n_points && threadIdx.x == 0) n_points[win] = x.P > 0x7fffffffll ? 0x7fffffff : (int)x.P;
    if (x.P > s.p_lim || (s.mode == 0 && x.tau < 1)) return TDA_WIN_TOO_LARGE;
    return x.P < 3 ? TDA_WIN_DEGENERATE : 0;
}

// ---- the LDS of a key pass: the triangle at 0, then (clouds) the points, their |x|^2 and the min / range per column ----
struct KeyLayout {
    int off_pts, off_nrm, off_mm, total;                // bytes
};
inline KeyLayout key_layout(int n_max, int dim)
{
    KeyLayout L;
    int o = (n_max * (n_max - 1) / 2 * 4 + 15) & ~15;
    L.off_pts = o; o += n_max * dim * 8;
    L.off_nrm = o; o += n_max * 8;
    L.off_mm = o;  o += 2 * TDA_MAX_DIM * 8;
    L.total = o;
    return L;
}

// key[tri2(a) + b] of the n points of an accepted window (win_status == 0), by a workgroup of NT threads (NT / 64 >= dim
// waves); ends with the workgroup barrier.  Barriers: one for a matrix; three for a cloud, five when it is normalised.
template <int NT>
__device__ __forceinline__ void window_keys(const WinSrc& s, const WinExtent& x, int n, unsigned char* smem, const KeyLayout& L)
{
    float* key = reinterpret_cast<float*>(smem);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, dim = s.dim;
    if (s.mode == 2) {
        for (int i = tid; i < n * n; i += NT) {
            const int a = i / n, b = i - a * n;
            if (b < a) key[tri2(a) + b] = dm_key(x.base, n, a, b, s.flag);
        }
    } else {
        double* pts = reinterpret_cast<double*>(smem + L.off_pts);
        double* nrm = reinterpret_cast<double*>(smem + L.off_nrm);
        double* mm = reinterpret_cast<double*>(smem + L.off_mm);
        for (int idx = tid; idx < n * dim; idx += NT) {
            const int i = idx / dim, k = idx - i * dim;
            pts[idx] = (s.mode == 0) ? x.base[(size_t)i * s.subsample + (size_t)k * x.tau] : x.base[idx];
        }
        __syncthreads();
        if (s.flag) {
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
            for (int idx = tid; idx < n * dim; idx += NT) {
                const int k = idx % dim;
                pts[idx] = (pts[idx] - mm[2 * k]) / mm[2 * k + 1];
            }
            __syncthreads();
        }
        if (tid < n) nrm[tid] = KeyFromPtsTab::norm2(pts + tid * dim, dim);
        __syncthreads();
        const KeyFromPtsTab kft{pts, nrm, dim};
        const int E = tri2(n);
        for (int e = tid; e < E; e += NT) {
            const int a = edge_row(e);
            key[e] = kft(0, a, e - tri2(a));
        }
    }
    __syncthreads();
}

// ---- host side: the limits of a window source, and what they mean for the launch ----
// Fills n_in, dim, subsample, mode and p_lim of *s (src, aux and flag are the caller's) and *n_max, the point count that
// sizes the LDS layout; either may be NULL for a caller that only wants the refusal.
inline tda_status win_src_limits(tda_ctx* ctx, int mode, int n_in, int dim, int subsample, WinSrc* s, int* n_max)
{
    int nm, p_lim = TDA_MAX_POINTS;
    if (mode == 2) {
        if (n_in < 1 || n_in > TDA_MAX_POINTS) TDA_FAIL(ctx, TDA_ERR_INVALID, "n must be in [1, TDA_MAX_POINTS]");
        nm = n_in; dim = 0; subsample = 1;
    } else {
        if (dim < 1 || dim > TDA_MAX_DIM) TDA_FAIL(ctx, TDA_ERR_INVALID, "dim must be in [1, TDA_MAX_DIM]");
        if (n_in < 1) TDA_FAIL(ctx, TDA_ERR_INVALID, mode == 0 ? "n_t must be >= 1" : "p_cap must be >= 1");
        if (subsample < 1) subsample = 1;
        if (mode == 0) {
            // tau >= 1 in the reference (utils.py:103-104); P is largest at tau = 1
            const int nn = n_in - (dim - 1);
            nm = nn > 0 ? (nn + subsample - 1) / subsample : 0;
        } else {
            nm = n_in;
            if (n_in < p_lim) p_lim = n_in;                          // never more than its buffer holds
        }
        if (nm > TDA_MAX_POINTS) nm = TDA_MAX_POINTS;                // larger clouds are flagged per window
        if (nm < 3) nm = 3;
    }
    if (s) { s->n_in = n_in; s->dim = dim; s->subsample = subsample; s->mode = mode; s->p_lim = p_lim; }
    if (n_max) *n_max = nm;
    return TDA_OK;
}
